// k-nearest-neighbour label probe of the latents: an Nq x Nr squared-distance GEMM in exact fp32 on the matrix cores with the
// top-k selection fused behind it, then a merge-and-vote pass.  The definition (norms, distance, the (d, index) order, the vote)
// is pinned in include/splitvae.h (sv_knn_classify); the Nq x Nr matrix never exists in memory.
//   knn_norm_kernel   n(v) = sum_j v_j^2 per row: one wave per row, lanes stride j, then the 64-lane butterfly -- one order per row
//   knn_tile_kernel   workgroup = (64-query tile, chunk of KNN_CHUNK references): for each 64-reference tile of the chunk the
//                     dense_f32.hip K loop (v_mfma_f32_16x16x4_f32 over the whole of L, zero-padded to 32), the accumulators
//                     turned into distances in LDS, and a per-row running top-k list: one sorted k-list per (query, chunk)
//   knn_merge_kernel  one wave per query folds the chunk lists in chunk order, votes, writes pred / the neighbours, counts hits
// Selection: wave w owns rows 16 w .. 16 w + 15 of the tile and keeps their lists in registers (lane i = list entry i, k <= 32).
// Per row the 64 lanes each hold one column's distance and compare it with the row's current k-th entry; a wave-wide ballot finds
// the columns that enter (none, for most tiles after the first few), and those are inserted one by one with a ballot / shuffle.
// The list is a set under a total order, so the result does not depend on the insertion order: same inputs -> same bits.
// LDS: operands as [k][m] images with rows of 80 floats (320 B: 16-B aligned; the ds_read_b32 bank is dword % 32 per 32-lane half,
// a half reads k rows 2 apart in lk = 0 / 1, 80 % 32 = 16: conflict-free; the staging writes put 32 consecutive m of one k row
// into a half: conflict-free); the distance tile as [m][68] (the accumulator rows lk 4 apart land 16 banks apart).
#include "eval_common.hip.h"

namespace {

constexpr int BM = 64, BN = 64, BK = 32, LP = 80, DP = 68, KMAX = 32;
constexpr int KNN_CHUNK = 4096;                  // reference rows per chunk (sv_knn_chunk_rows)
constexpr int IDX_NONE = 0x7fffffff;

struct KnnArgs {
  const float* q; const float* r; const uint8_t* r_class; const uint8_t* q_class;
  const float* nq; const float* nr;               // workspace: row norms
  float* ws_d; int32_t* ws_i;                     // workspace: [Nq][nchunks][k]
  int32_t* nn_index; float* nn_dist; int32_t* pred; unsigned long long* acc;
  int ldq, ldr, Nq, Nr, L, k, n_class, nchunks, vecq, vecr;
};

__device__ __forceinline__ bool knn_less(float da, int ia, float db, int ib) { return da < db || (da == db && ia < ib); }

// lanes 0 .. k-1 hold a list sorted under (d, index); offer the lanes' candidates (d, idx, valid) to it
__device__ __forceinline__ void topk_offer(float& ld, int& li, const int k, const int lane, const float d, const int idx, const bool valid) {
  const float tk = __shfl(ld, k - 1, 64);
  const int ik = __shfl(li, k - 1, 64);
  unsigned long long mask = __ballot(valid && knn_less(d, idx, tk, ik));
  while (mask) {                                   // wave-uniform
    const int c = __ffsll((long long)mask) - 1;
    mask &= mask - 1;
    const float dc = __shfl(d, c, 64);
    const int ic = __shfl(idx, c, 64);
    const int pos = __popcll(__ballot(lane < k && knn_less(ld, li, dc, ic)));   // sorted: the entries before the candidate are a prefix
    if (pos >= k) continue;                        // the list tightened since the ballot
    const float dp = __shfl_up(ld, 1, 64);
    const int ip = __shfl_up(li, 1, 64);
    if (lane == pos) { ld = dc; li = ic; }
    else if (lane > pos) { ld = dp; li = ip; }
  }
}

__global__ __launch_bounds__(256) void knn_norm_kernel(const float* __restrict__ v, int ld, int N, int L, float* __restrict__ out) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= N) return;                            // whole waves leave
  const float* __restrict__ p = v + row * ld;
  float s = 0.f;
  for (int j = lane; j < L; j += 64) s += p[j] * p[j];
  s = wave_sum(s);
  if (lane == 0) out[row] = s;
}

// rows mn0 + (tid & 63), k piece k0 + (tid >> 6) * 8: 8 floats of one row (k contiguous)
__device__ __forceinline__ void knn_load(const float* __restrict__ P, int ld, int mn0, int k0, int MN, int L, int tid, bool vec, float (&r)[8]) {
  const int row = mn0 + (tid & 63), k = k0 + (tid >> 6) * 8;
  const bool any = row < MN;
  const int lim = L - k;
  const float* p = P + (int64_t)row * ld + k;
  if (any && vec && lim >= 8) {
    const float4 a = *(const float4*)p, b = *(const float4*)(p + 4);
    r[0] = a.x; r[1] = a.y; r[2] = a.z; r[3] = a.w; r[4] = b.x; r[5] = b.y; r[6] = b.z; r[7] = b.w;
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) r[i] = (any && i < lim) ? p[i] : 0.f;
  }
}
__device__ __forceinline__ void knn_store(float* s, int tid, const float (&r)[8]) {
  const int m = tid & 63, k = (tid >> 6) * 8;
#pragma unroll
  for (int i = 0; i < 8; ++i) s[(k + i) * LP + m] = r[i];
}

__global__ __launch_bounds__(256) void knn_tile_kernel(const KnnArgs g) {
  __shared__ __attribute__((aligned(16))) float sA[2][BK * LP];
  __shared__ __attribute__((aligned(16))) float sB[2][BK * LP];
  __shared__ __attribute__((aligned(16))) float sD[BM * DP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.x * BM, chunk = blockIdx.y;
  const int c0 = chunk * KNN_CHUNK, c1 = min(g.Nr, c0 + KNN_CHUNK);
  const int nks = (g.L + BK - 1) / BK;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32, lr = lane & 15, lk = lane >> 4;
  float nqv[2][4];                                 // norms of this lane's accumulator rows
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = m0 + wm + i * 16 + lk * 4 + r;
      nqv[i][r] = m < g.Nq ? g.nq[m] : 0.f;
    }
  float ld_[16]; int li_[16];                      // rows wave * 16 + rr: lane i = entry i of the row's list
#pragma unroll
  for (int rr = 0; rr < 16; ++rr) { ld_[rr] = __builtin_inff(); li_[rr] = IDX_NONE; }
  float ra[8], rb[8];
  for (int n0 = c0; n0 < c1; n0 += BN) {
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    knn_load(g.q, g.ldq, m0, 0, g.Nq, g.L, tid, g.vecq, ra);
    knn_load(g.r, g.ldr, n0, 0, c1, g.L, tid, g.vecr, rb);
    knn_store(sA[0], tid, ra);
    knn_store(sB[0], tid, rb);
    __syncthreads();                               // (also: every wave is done with the previous tile's sD)
    for (int ks = 0; ks < nks; ++ks) {
      const int buf = ks & 1;
      const bool more = ks + 1 < nks;
      if (more) {
        knn_load(g.q, g.ldq, m0, (ks + 1) * BK, g.Nq, g.L, tid, g.vecq, ra);
        knn_load(g.r, g.ldr, n0, (ks + 1) * BK, c1, g.L, tid, g.vecr, rb);
      }
      const float* cA = sA[buf];
      const float* cB = sB[buf];
#pragma unroll
      for (int kk = 0; kk < BK / 4; ++kk) {
        const int k = kk * 4 + lk;
        const float a0 = cA[k * LP + wm + lr], a1 = cA[k * LP + wm + 16 + lr];
        const float b0 = cB[k * LP + wn + lr], b1 = cB[k * LP + wn + 16 + lr];
        acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
      }
      if (more) {
        knn_store(sA[buf ^ 1], tid, ra);
        knn_store(sB[buf ^ 1], tid, rb);
      }
      __syncthreads();
    }
    // D: row = (lane >> 4) * 4 + reg, column = lane & 15 of each fragment.  d = max(0, (n(q) + n(r)) - 2 dot)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int nl = wn + j * 16 + lr;
      const float nrv = n0 + nl < c1 ? g.nr[n0 + nl] : 0.f;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int ml = wm + i * 16 + lk * 4 + r;
          sD[ml * DP + nl] = fmaxf(0.f, (nqv[i][r] + nrv) - 2.f * acc[i][j][r]);
        }
    }
    __syncthreads();
    const int idx = n0 + lane;
    const bool valid = idx < c1;
#pragma unroll
    for (int rr = 0; rr < 16; ++rr) topk_offer(ld_[rr], li_[rr], g.k, lane, sD[(wave * 16 + rr) * DP + lane], idx, valid);
  }
  if (lane < g.k) {
#pragma unroll
    for (int rr = 0; rr < 16; ++rr) {
      const int m = m0 + wave * 16 + rr;
      if (m < g.Nq) {
        const int64_t o = ((int64_t)m * g.nchunks + chunk) * g.k + lane;
        g.ws_d[o] = ld_[rr];
        g.ws_i[o] = li_[rr];
      }
    }
  }
}

__global__ __launch_bounds__(256) void knn_merge_kernel(const KnnArgs g) {
  const int64_t qi = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (blockIdx.x == 0 && threadIdx.x == 0 && g.acc) atomicAdd(g.acc + 1, (unsigned long long)g.Nq);
  if (qi >= g.Nq) return;                          // whole waves leave
  float ld = __builtin_inff();
  int li = IDX_NONE;
  for (int c = 0; c < g.nchunks; ++c) {
    const int64_t o = (qi * g.nchunks + c) * g.k + lane;
    float d = 0.f;
    int idx = IDX_NONE;
    if (lane < g.k) { d = g.ws_d[o]; idx = g.ws_i[o]; }
    topk_offer(ld, li, g.k, lane, d, idx, lane < g.k && (unsigned)idx < (unsigned)g.Nr);
  }
  const bool have = lane < g.k && (unsigned)li < (unsigned)g.Nr;
  if (lane < g.k) {
    if (g.nn_index) g.nn_index[qi * g.k + lane] = li;
    if (g.nn_dist) g.nn_dist[qi * g.k + lane] = ld;
  }
  const int cls = have ? (int)g.r_class[li] : -1;
  int votes = 0;                                   // lane c counts the votes of class c
  for (int i = 0; i < g.k; ++i) votes += __shfl(cls, i, 64) == lane;
  int key = lane < g.n_class ? votes * 64 + (63 - lane) : -1;       // most votes, then the lowest class id
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) key = max(key, __shfl_xor(key, o, 64));
  const int p = 63 - (key & 63);
  if (lane == 0) {
    g.pred[qi] = p;
    if (g.acc && g.q_class && (int)g.q_class[qi] == p) atomicAdd(g.acc, 1ull);      // integer counters: any order, same sum
  }
}

struct KnnLayout { int64_t nq, nr, d, i, total; int nchunks; };
inline KnnLayout knn_layout(int64_t Nq, int64_t Nr, int64_t k) {
  KnnLayout w;
  w.nchunks = (int)((Nr + KNN_CHUNK - 1) / KNN_CHUNK);
  w.nq = 0;
  w.nr = w.nq + up256(Nq * 4);
  w.d = w.nr + up256(Nr * 4);
  w.i = w.d + up256(Nq * w.nchunks * k * 4);
  w.total = w.i + up256(Nq * w.nchunks * k * 4);
  return w;
}
inline bool knn_sizes_ok(int32_t Nq, int32_t Nr, int32_t k) {
  return Nq >= 1 && k >= 1 && k <= KMAX && Nr >= k && (Nr + KNN_CHUNK - 1) / KNN_CHUNK <= 65535;
}

}  // namespace

extern "C" int sv_knn_chunk_rows(void) { return KNN_CHUNK; }

extern "C" int sv_knn_workspace_bytes(int32_t Nq, int32_t Nr, int32_t k, int64_t* bytes) {
  if (!bytes) return SV_E_BADARG;
  if (!knn_sizes_ok(Nq, Nr, k)) return SV_E_UNSUPPORTED;
  *bytes = knn_layout(Nq, Nr, k).total;
  return SV_OK;
}

extern "C" int sv_knn_classify(const float* q, int32_t ldq, const float* r, int32_t ldr, const uint8_t* r_class, int32_t Nq, int32_t Nr,
                               int32_t L, int32_t k, int32_t n_class, int32_t* nn_index, float* nn_dist, int32_t* pred,
                               const uint8_t* q_class, int64_t* acc, void* workspace, int64_t workspace_bytes, void* stream) {
  if (!q || !r || !r_class || !pred || !workspace) return SV_E_BADARG;
  if (!al(q, 4) || !al(r, 4) || !al(pred, 4) || !al(nn_index, 4) || !al(nn_dist, 4) || !al(acc, 8) || !al(workspace, 16)) return SV_E_BADARG;
  if (!knn_sizes_ok(Nq, Nr, k) || L < 1 || L > 512 || ldq < L || ldr < L || n_class < 2 || n_class > 64) return SV_E_UNSUPPORTED;
  const KnnLayout w = knn_layout(Nq, Nr, k);
  if (workspace_bytes < w.total) return SV_E_WORKSPACE;
  char* ws = (char*)workspace;
  hipStream_t st = (hipStream_t)stream;
  KnnArgs g = {q, r, r_class, q_class, (const float*)(ws + w.nq), (const float*)(ws + w.nr), (float*)(ws + w.d), (int32_t*)(ws + w.i),
               nn_index, nn_dist, pred, (unsigned long long*)acc, ldq, ldr, Nq, Nr, L, k, n_class, w.nchunks,
               !(ldq & 3) && al(q, 16), !(ldr & 3) && al(r, 16)};
  hipLaunchKernelGGL(knn_norm_kernel, dim3((Nq + 3) / 4), dim3(256), 0, st, q, ldq, Nq, L, (float*)(ws + w.nq));
  SV_LAUNCH_CHECK();
  hipLaunchKernelGGL(knn_norm_kernel, dim3((Nr + 3) / 4), dim3(256), 0, st, r, ldr, Nr, L, (float*)(ws + w.nr));
  SV_LAUNCH_CHECK();
  hipLaunchKernelGGL(knn_tile_kernel, dim3((Nq + BM - 1) / BM, w.nchunks), dim3(256), 0, st, g);
  SV_LAUNCH_CHECK();
  hipLaunchKernelGGL(knn_merge_kernel, dim3((Nq + 3) / 4), dim3(256), 0, st, g);
  SV_LAUNCH_CHECK();
  return SV_OK;
}
