// Sample-quality report of prior draws: precision / recall (Kynkaanniemi et al. 2019) and density / coverage (Naeem et al. 2020) need "is
// query q inside reference j's k-NN ball" -- a compare against a PER-COLUMN radius behind the distance tile -- and the k-NN radius of a
// set against itself with self excluded by index.  The definitions are pinned in include/splitvae.h (sv_prdc_*).
//   prdc_radius_kernel   thread per row i of sv_knn_classify's (k + 1)-list of the set against itself (ascending in (d, index)): index i
//                        is dropped where it stands, the k-th of what remains is the radius.  Self is in the list unless k + 1 other rows
//                        come before it under (d, index) -- rows at d(i, i) with lower indices -- and then the k-th entry is the answer too
//   prdc_norm_kernel     sv_knn_classify's norms (dist_tile.hip.h) of Q and R
//   prdc_count_kernel    THE HOT KERNEL.  workgroup = (64-query tile, chunk of PR_CHUNK references): for each 64-reference tile of the
//                        chunk the distance tile; a lane owns column n0 + lane and loads its radius once per tile; wave w takes the rows
//                        16 w .. 16 w + 15: one compare d <= rad[column] into an integer count and a strict d < best into (best, index)
//                        per row (a lane's columns ascend, so it keeps its lowest index); at the end of the chunk an integer butterfly
//                        and a lexicographic (d, index) butterfly per row -> partials cnt / dmin / imin [nchunks][Nq]
//   prdc_fold_kernel     thread per query: the chunk partials in ascending chunk order, a strict < keeps the lower index
// Integer counts and minima only, no atomics, every output element written once: a repeat gives the same bits.  The Nq x Nr matrix never
// exists.
#include "dist_tile.hip.h"
#include "kernels.h"

namespace {

constexpr int PR_CHUNK = 2048;                   // reference rows per chunk of the count pass (sv_prdc_chunk_rows)
constexpr int PR_MAX_L = 512, PR_MAX_NQ = 8 * 65536, PR_MAX_NR = 1 << 24, PR_MAX_K = 31;
constexpr int PR_IDX_NONE = 0x7fffffff;

// ============================================================================ sv_prdc_radius
__global__ __launch_bounds__(256) void prdc_radius_kernel(const int32_t* __restrict__ nn_i, const float* __restrict__ nn_d, int N, int k,
                                                          float* __restrict__ rad) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int32_t* li = nn_i + (int64_t)i * (k + 1);
  const float* ld = nn_d + (int64_t)i * (k + 1);
  int kept = 0;
  float r = 0.f;
  for (int e = 0; e <= k; ++e) {
    if (li[e] == i) continue;                      // self, by index: a duplicate of row i at another index stays
    if (++kept == k) { r = ld[e]; break; }
  }
  rad[i] = r;
}

// ============================================================================ sv_prdc_count
struct PrdcArgs {
  const float* q; const float* r; const float* rad;
  const float* nq; const float* nr;                      // workspace: row norms of Q, R
  int32_t* pc; float* pd; int32_t* pi;                   // workspace: partials [nchunks][Nq]
  int32_t* cnt; float* dmin; int32_t* imin;
  int ldq, ldr, Nq, Nr, L, nchunks, vecq, vecr;
};

__global__ __launch_bounds__(256) void prdc_norm_kernel(const float* __restrict__ v, int ld, int N, int L, float* __restrict__ out) {
  dist_norm_rows(v, ld, N, L, out);
}

__device__ __forceinline__ void prdc_row_norms(const float* __restrict__ nq, int m0, int Nq, float (&nqv)[2][4]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = (wave >> 1) * 32, lk = lane >> 4;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = m0 + wm + i * 16 + lk * 4 + r;
      nqv[i][r] = m < Nq ? nq[m] : 0.f;
    }
}

__global__ __launch_bounds__(256) void prdc_count_kernel(const PrdcArgs a) {
  __shared__ __attribute__((aligned(16))) float sA[2][DT_BK * DT_LP];
  __shared__ __attribute__((aligned(16))) float sB[2][DT_BK * DT_LP];
  __shared__ __attribute__((aligned(16))) float sD[DT_BM * DT_DP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.x * DT_BM, chunk = blockIdx.y;
  const int c0 = chunk * PR_CHUNK, c1 = min(a.Nr, c0 + PR_CHUNK);
  float nqv[2][4];
  prdc_row_norms(a.nq, m0, a.Nq, nqv);
  int cnt[16], bi[16];
  float bd[16];
#pragma unroll
  for (int rr = 0; rr < 16; ++rr) { cnt[rr] = 0; bd[rr] = __builtin_inff(); bi[rr] = PR_IDX_NONE; }
  for (int n0 = c0; n0 < c1; n0 += DT_BN) {
    const int idx = n0 + lane;
    const bool valid = idx < c1;                   // a padded column neither counts nor wins the minimum
    const float rv = valid ? a.rad[idx] : 0.f;     // this lane's column: once per tile
    dist_tile_64x64(a.q, a.ldq, m0, a.Nq, a.vecq, a.r, a.ldr, n0, c1, a.vecr, a.L, nqv, a.nr, sA, sB, sD);
#pragma unroll
    for (int rr = 0; rr < 16; ++rr) {
      const float d = sD[(wave * 16 + rr) * DT_DP + lane];
      cnt[rr] += (valid && d <= rv) ? 1 : 0;
      if (valid && d < bd[rr]) { bd[rr] = d; bi[rr] = idx; }
    }
  }
#pragma unroll
  for (int rr = 0; rr < 16; ++rr) {
    int v = cnt[rr], i = bi[rr];
    float d = bd[rr];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      v += __shfl_xor(v, o, 64);
      const float od = __shfl_xor(d, o, 64);
      const int oi = __shfl_xor(i, o, 64);
      if (od < d || (od == d && oi < i)) { d = od; i = oi; }
    }
    const int m = m0 + wave * 16 + rr;
    if (lane == 0 && m < a.Nq) {
      const int64_t o = (int64_t)chunk * a.Nq + m;
      a.pc[o] = v; a.pd[o] = d; a.pi[o] = i;
    }
  }
}

__global__ __launch_bounds__(256) void prdc_fold_kernel(const PrdcArgs a) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= a.Nq) return;
  int v = 0, i = PR_IDX_NONE;
  float d = __builtin_inff();
  for (int c = 0; c < a.nchunks; ++c) {
    const int64_t o = (int64_t)c * a.Nq + q;
    v += a.pc[o];
    const float cd = a.pd[o];
    if (cd < d) { d = cd; i = a.pi[o]; }           // chunks ascend: a strict < keeps the lower index
  }
  a.cnt[q] = v;
  if (a.dmin) a.dmin[q] = d;
  if (a.imin) a.imin[q] = i;
}

struct PrdcCountLayout { int64_t nq, nr, pc, pd, pi, total; int nchunks; };
inline PrdcCountLayout prdc_count_layout(int64_t Nq, int64_t Nr) {
  PrdcCountLayout w;
  w.nchunks = (int)((Nr + PR_CHUNK - 1) / PR_CHUNK);
  w.nq = 0;
  w.nr = w.nq + up256(Nq * 4);
  w.pc = w.nr + up256(Nr * 4);
  w.pd = w.pc + up256((int64_t)w.nchunks * Nq * 4);
  w.pi = w.pd + up256((int64_t)w.nchunks * Nq * 4);
  w.total = w.pi + up256((int64_t)w.nchunks * Nq * 4);
  return w;
}
// the radius pass: the (k + 1)-lists, sv_knn_classify's class ids and predictions (unused: any contents), then its own workspace
struct PrdcRadiusLayout { int64_t nn_i, nn_d, cls, pred, knn, total; };
inline int prdc_radius_layout(int32_t N, int32_t k, PrdcRadiusLayout* w) {
  int64_t knn = 0;
  const int rc = sv_knn_workspace_bytes(N, N, k + 1, &knn);
  if (rc) return rc;
  w->nn_i = 0;
  w->nn_d = w->nn_i + up256((int64_t)N * (k + 1) * 4);
  w->cls = w->nn_d + up256((int64_t)N * (k + 1) * 4);
  w->pred = w->cls + up256((int64_t)N);
  w->knn = w->pred + up256((int64_t)N * 4);
  w->total = w->knn + up256(knn);
  return SV_OK;
}
inline int prdc_count_sizes(int32_t Nq, int32_t Nr, int32_t L) {
  if (Nq <= 0 || Nr <= 0 || L <= 0) return SV_E_BADARG;
  if (Nq > PR_MAX_NQ || Nr > PR_MAX_NR || L > PR_MAX_L) return SV_E_UNSUPPORTED;
  return SV_OK;
}
inline int prdc_radius_sizes(int32_t N, int32_t L, int32_t k) {
  if (N <= 0 || L <= 0) return SV_E_BADARG;
  if (k < 1 || k > PR_MAX_K || N < k + 1 || N > PR_MAX_NQ || L > PR_MAX_L) return SV_E_UNSUPPORTED;
  return SV_OK;
}

}  // namespace

extern "C" int sv_prdc_chunk_rows(void) { return PR_CHUNK; }

extern "C" int sv_prdc_workspace_bytes(int32_t Nq, int32_t Nr, int32_t L, int32_t k, int64_t* bytes) {
  if (!bytes) return SV_E_BADARG;
  const int rc = prdc_count_sizes(Nq, Nr, L);
  if (rc) return rc;
  if (k < 1 || k > PR_MAX_K) return SV_E_UNSUPPORTED;
  int64_t n = prdc_count_layout(Nq, Nr).total;
  if (Nq == Nr && Nr >= k + 1) {                   // the shape sv_prdc_radius takes: one workspace serves both
    PrdcRadiusLayout w;
    const int rr = prdc_radius_layout(Nr, k, &w);
    if (rr) return rr;
    if (w.total > n) n = w.total;
  }
  *bytes = n;
  return SV_OK;
}

extern "C" int sv_prdc_radius(const float* x, int32_t ldx, int32_t N, int32_t L, int32_t k, float* rad, void* workspace,
                              int64_t workspace_bytes, void* stream) {
  if (!x || !rad || !workspace) return SV_E_BADARG;
  if (!al(x, 4) || !al(rad, 4) || !al(workspace, 16)) return SV_E_BADARG;
  const int rc = prdc_radius_sizes(N, L, k);
  if (rc == SV_E_BADARG) return rc;
  if (ldx < L) return SV_E_BADARG;
  if (rc) return rc;
  PrdcRadiusLayout w;
  const int rl = prdc_radius_layout(N, k, &w);
  if (rl) return rl;
  if (workspace_bytes < w.total) return SV_E_WORKSPACE;
  char* ws = (char*)workspace;
  int32_t* nn_i = (int32_t*)(ws + w.nn_i);
  float* nn_d = (float*)(ws + w.nn_d);
  // the class ids are read for the lists' entries only and vote for a prediction nobody reads: whatever the workspace holds will do
  const int rk = sv_knn_classify(x, ldx, x, ldx, (const uint8_t*)(ws + w.cls), N, N, L, k + 1, 2, nn_i, nn_d, (int32_t*)(ws + w.pred),
                                 nullptr, nullptr, ws + w.knn, w.total - w.knn, stream);
  if (rk) return rk;                               // refused before its first launch: every check above covers its own
  hipLaunchKernelGGL(prdc_radius_kernel, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, nn_i, nn_d, N, k, rad);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

extern "C" int sv_prdc_count(const float* q, int32_t ldq, const float* r, int32_t ldr, const float* rad, int32_t Nq, int32_t Nr, int32_t L,
                             int32_t* cnt, float* dmin, int32_t* imin, void* workspace, int64_t workspace_bytes, void* stream) {
  if (!q || !r || !rad || !cnt || !workspace) return SV_E_BADARG;
  if (!al(q, 4) || !al(r, 4) || !al(rad, 4) || !al(cnt, 4) || !al(dmin, 4) || !al(imin, 4) || !al(workspace, 16)) return SV_E_BADARG;
  const int rc = prdc_count_sizes(Nq, Nr, L);
  if (rc == SV_E_BADARG) return rc;
  if (ldq < L || ldr < L) return SV_E_BADARG;
  if (rc) return rc;
  const PrdcCountLayout w = prdc_count_layout(Nq, Nr);
  if (workspace_bytes < w.total) return SV_E_WORKSPACE;
  char* ws = (char*)workspace;
  hipStream_t st = (hipStream_t)stream;
  PrdcArgs a = {q, r, rad, (const float*)(ws + w.nq), (const float*)(ws + w.nr), (int32_t*)(ws + w.pc), (float*)(ws + w.pd),
                (int32_t*)(ws + w.pi), cnt, dmin, imin, ldq, ldr, Nq, Nr, L, w.nchunks, !(ldq & 3) && al(q, 16), !(ldr & 3) && al(r, 16)};
  hipLaunchKernelGGL(prdc_norm_kernel, dim3((Nq + 3) / 4), dim3(256), 0, st, q, ldq, Nq, L, (float*)(ws + w.nq));
  SV_LAUNCH_CHECK();
  hipLaunchKernelGGL(prdc_norm_kernel, dim3((Nr + 3) / 4), dim3(256), 0, st, r, ldr, Nr, L, (float*)(ws + w.nr));
  SV_LAUNCH_CHECK();
  hipLaunchKernelGGL(prdc_count_kernel, dim3((Nq + DT_BM - 1) / DT_BM, w.nchunks), dim3(256), 0, st, a);
  SV_LAUNCH_CHECK();
  hipLaunchKernelGGL(prdc_fold_kernel, dim3((Nq + 255) / 256), dim3(256), 0, st, a);
  SV_LAUNCH_CHECK();
  return SV_OK;
}
