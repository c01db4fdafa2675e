// Exact t-SNE map of the latents (van der Maaten & Hinton 2008, the O(N^2) form).  The definition (distance, the beta search, the
// symmetrisation, the Philox key of the initial map, gradient, delta-bar-delta update, the summation orders) is pinned in
// include/splitvae.h (sv_tsne_*); this file is the kernels.
//   ts_norm_kernel, ts_dist_kernel   sv_knn_classify's norms and distance tile (dist_tile.hip.h: the code knn.hip runs) -> D [N, N]
//   ts_row_kernel      one workgroup per row: the row of D in LDS, dmin, then TSNE_BETA_STEPS steps of the beta search with the entropy
//                      sums in fp64 (thread u takes the columns u, u + 256, ... ascending, then the threads in thread order), then the
//                      conditional row over the distances, beta and the row's entropy
//   ts_sym_kernel      32 x 32 tile pairs of the upper triangle through LDS: the thread that owns (i, j), i < j, writes both
//   ts_pstat_kernel, ts_pfold_kernel   sum P and sum P log P per row in fp64, folded in row order
//   ts_init_kernel     Y0, inc = 0, gain = 1, the counter
//   ts_pair_kernel     THE HOT KERNEL.  workgroup = (64 rows, one chunk of TS_CHUNK columns): the chunk's Y in LDS (8 KiB), wave w takes
//                      the rows w, w + 4, ...; a lane's 16 P values of the row segment are in flight at once (256 B per wave load), six
//                      fp32 accumulators per lane, one butterfly per (row, chunk) -> partials [N][nchunks][6].  P is read once; nothing
//                      of size N x N is written.
//   ts_fold_kernel     thread per row: the chunk partials in chunk order in fp64 -> rowsum [N][6]; Z and sum P log w per workgroup
//   ts_update_kernel   folds the workgroup partials (every workgroup alike), the gradient, gains, inc, Y; column sums per workgroup; KL
//   ts_centre_kernel   folds the column sums, subtracts the means, bumps the counter
//   ts_score_kernel    one wave per row over the two neighbour lists: integer sums
#include "dist_tile.hip.h"

namespace {

constexpr int TS_CHUNK = 1024;                   // columns per fp32 partial of the pair pass (sv_tsne_chunk_rows)
constexpr int TS_ROWS = 64;                      // rows per workgroup of the pair pass
constexpr int TS_MAX_N = 32768;                  // a 4-GiB P; a row of D fills 128 KiB of the row search's LDS
constexpr int TS_BETA_STEPS = 100;
constexpr double TS_BETA_MIN = 0x1p-60, TS_BETA_MAX = 0x1p60;
constexpr uint64_t TS_KEY = 0x1a7e475e3a9ULL;    // sv_tsne_init (no other kernel of the library uses it)
constexpr uint32_t TS_TAG = 0x74730000u;         // 'ts'

__global__ __launch_bounds__(256) void ts_norm_kernel(const float* __restrict__ v, int ld, int N, int L, float* __restrict__ out) {
  dist_norm_rows(v, ld, N, L, out);
}

__global__ __launch_bounds__(256) void ts_dist_kernel(const float* __restrict__ x, int ldx, int N, int L, int vec, const float* __restrict__ nx,
                                                      float* __restrict__ D) {
  __shared__ __attribute__((aligned(16))) float sA[2][DT_BK * DT_LP];
  __shared__ __attribute__((aligned(16))) float sB[2][DT_BK * DT_LP];
  __shared__ __attribute__((aligned(16))) float sD[DT_BM * DT_DP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.y * DT_BM, n0 = blockIdx.x * DT_BN;
  const int wm = (wave >> 1) * 32, lk = lane >> 4;
  float nqv[2][4];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = m0 + wm + i * 16 + lk * 4 + r;
      nqv[i][r] = m < N ? nx[m] : 0.f;
    }
  dist_tile_64x64(x, ldx, m0, N, vec, x, ldx, n0, N, vec, L, nqv, nx, sA, sB, sD);
  const int j = n0 + lane;
  if (j < N)
    for (int rr = wave; rr < DT_BM; rr += 4) {
      const int i = m0 + rr;
      if (i < N) D[(int64_t)i * N + j] = sD[rr * DT_DP + lane];
    }
}

// the 256 fp64 values of a workgroup, added in thread order; every thread gets the total
__device__ __forceinline__ double ts_block_sum(double v, double* part) { return block_sum_ordered(v, part); }

__global__ __launch_bounds__(256) void ts_row_kernel(float* __restrict__ D, int N, double log_perp, double* __restrict__ beta_out,
                                                     double* __restrict__ h_out) {
  extern __shared__ __attribute__((aligned(16))) float srow[];      // [N]
  __shared__ double part[256];
  __shared__ float smin[256];
  const int i = blockIdx.x, tid = threadIdx.x;
  float* __restrict__ row = D + (int64_t)i * N;
  float mn = 3.402823466e38f;
  for (int j = tid; j < N; j += 256) {
    float d = row[j];
    if (!(d <= 3.402823466e38f)) d = 3.402823466e38f;                // NaN or +inf (an overflowed norm): the largest finite distance
    srow[j] = d;
    if (j != i) mn = fminf(mn, d);
  }
  smin[tid] = mn;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {                                // a minimum: the tree's shape does not matter
    if (tid < o) smin[tid] = fminf(smin[tid], smin[tid + o]);
    __syncthreads();
  }
  const double dmin = (double)smin[0];
  double beta = 1.0, lo = 0.0, hi = 0.0, H = 0.0, S = 1.0;
  bool have_lo = false, have_hi = false;
  for (int step = 0; step <= TS_BETA_STEPS; ++step) {                // the last pass evaluates the final beta only
    double s = 0.0, t = 0.0;
    for (int j = tid; j < N; j += 256)
      if (j != i) {
        const double dd = (double)srow[j] - dmin;
        const double e = exp(-beta * dd);
        s += e;
        t += e * dd;
      }
    S = ts_block_sum(s, part);
    const double T = ts_block_sum(t, part);
    H = log(S) + beta * T / S;
    if (step == TS_BETA_STEPS) break;
    if (H > log_perp) {                                              // too flat: raise beta
      lo = beta; have_lo = true;
      beta = have_hi ? 0.5 * (lo + hi) : beta * 2.0;
    } else {
      hi = beta; have_hi = true;
      beta = have_lo ? 0.5 * (lo + hi) : beta * 0.5;
    }
    beta = fmin(fmax(beta, TS_BETA_MIN), TS_BETA_MAX);
  }
  for (int j = tid; j < N; j += 256) row[j] = j == i ? 0.f : (float)(exp(-beta * ((double)srow[j] - dmin)) / S);
  if (tid == 0) { beta_out[i] = beta; h_out[i] = H; }
}

__global__ __launch_bounds__(256) void ts_sym_kernel(float* __restrict__ P, int N) {
  __shared__ float ta[32][33], tb[32][33];
  const int bx = blockIdx.x, by = blockIdx.y;
  if (bx < by) return;                                               // the upper triangle's tile pairs
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;            // 32 x 8
  const int i0 = by * 32, j0 = bx * 32;
  for (int r = ty; r < 32; r += 8) {
    const int i = i0 + r, j = j0 + tx;
    ta[r][tx] = (i < N && j < N) ? P[(int64_t)i * N + j] : 0.f;      // p(j|i): tile (by, bx)
    const int i2 = j0 + r, j2 = i0 + tx;
    tb[r][tx] = (i2 < N && j2 < N) ? P[(int64_t)i2 * N + j2] : 0.f;  // tile (bx, by)
  }
  __syncthreads();
  const double two_n = 2.0 * (double)N;
  // thread (r, tx) owns (i, j) = (i0 + r, j0 + tx) where i < j: one value, written to (i, j) and to (j, i)
  if (bx == by) {                                                    // the diagonal tile: ta and tb hold the same tile
    for (int r = ty; r < 32; r += 8) {
      const int i = i0 + r, j = j0 + tx;
      if (i >= N || j >= N) continue;
      if (i == j) P[(int64_t)i * N + j] = 0.f;
      if (i < j) {
        const float v = (float)(((double)ta[r][tx] + (double)tb[tx][r]) / two_n);
        P[(int64_t)i * N + j] = v;
        P[(int64_t)j * N + i] = v;
      }
    }
    return;
  }
  for (int r = ty; r < 32; r += 8) {                                 // every (i, j) of the tile has i < j
    const int i = i0 + r, j = j0 + tx;
    const float v = (float)(((double)ta[r][tx] + (double)tb[tx][r]) / two_n);
    if (i < N && j < N) P[(int64_t)i * N + j] = v;
    ta[r][tx] = v;                                                   // (read by this thread only until here) for the mirrored tile's coalesced store
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int i2 = j0 + r, j2 = i0 + tx;
    if (i2 < N && j2 < N) P[(int64_t)i2 * N + j2] = ta[tx][r];
  }
}

// one wave per row: lane l takes the columns l, l + 64, ... ascending in fp64, then the 64 lanes in lane order
__global__ __launch_bounds__(256) void ts_pstat_kernel(const float* __restrict__ P, int N, double* __restrict__ prow) {
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (i >= N) return;                                                // whole waves leave
  const float* __restrict__ row = P + i * N;
  double s = 0.0, t = 0.0;
  for (int j = lane; j < N; j += 64) {
    const double p = (double)row[j];
    s += p;
    if (p > 0.0) t += p * log(p);
  }
  double st = 0.0, tt = 0.0;
  for (int l = 0; l < 64; ++l) { st += __shfl(s, l, 64); tt += __shfl(t, l, 64); }
  if (lane == 0) { prow[2 * i] = st; prow[2 * i + 1] = tt; }
}

// one workgroup: thread u takes the rows u, u + 256, ... ascending, then the threads in thread order
__global__ __launch_bounds__(256) void ts_pfold_kernel(const double* __restrict__ prow, int N, double* __restrict__ p_const) {
  __shared__ double part[256];
  double s = 0.0, t = 0.0;
  for (int i = threadIdx.x; i < N; i += 256) { s += prow[2 * i]; t += prow[2 * i + 1]; }
  s = ts_block_sum(s, part);
  t = ts_block_sum(t, part);
  if (threadIdx.x == 0) { p_const[0] = s; p_const[1] = t; }
}

__global__ __launch_bounds__(256) void ts_init_kernel(int N, uint64_t seed, float* __restrict__ Y, float* __restrict__ inc, float* __restrict__ gain,
                                                      int32_t* __restrict__ state) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e == 0) { state[0] = 0; state[1] = 0; state[2] = 0; state[3] = 0; }
  if (e >= 2 * N) return;
  const Philox ph(seed ^ TS_KEY);
  Y[e] = 1e-4f * philox_normal(ph, (uint32_t)(e & 1), (uint64_t)(e >> 1), TS_TAG, 0u);
  inc[e] = 0.f;
  gain[e] = 1.f;
}

__global__ __launch_bounds__(256) void ts_pair_kernel(const float* __restrict__ P, const float* __restrict__ Y, int N, int nchunks,
                                                      float* __restrict__ part) {
  __shared__ float2 sy[TS_CHUNK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int chunk = blockIdx.y, c0 = chunk * TS_CHUNK, r0 = blockIdx.x * TS_ROWS;
  for (int c = tid; c < TS_CHUNK; c += 256) {
    const int j = c0 + c;
    sy[c] = j < N ? make_float2(Y[2 * j], Y[2 * j + 1]) : make_float2(0.f, 0.f);
  }
  __syncthreads();
  constexpr int M = TS_CHUNK / 64;
  for (int rr = wave; rr < TS_ROWS; rr += 4) {
    const int i = r0 + rr;
    if (i >= N) break;                                               // wave-uniform
    const float* __restrict__ row = P + (int64_t)i * N + c0;
    float p[M];
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const int c = lane + 64 * m;
      p[m] = c0 + c < N ? row[c] : 0.f;
    }
    const float yi0 = Y[2 * i], yi1 = Y[2 * i + 1];
    float a0 = 0.f, a1 = 0.f, b0 = 0.f, b1 = 0.f, z = 0.f, plw = 0.f;
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const int c = lane + 64 * m, j = c0 + c;
      const float2 yj = sy[c];
      const float dx = yi0 - yj.x, dy = yi1 - yj.y;
      const float q = (1.f + dx * dx) + dy * dy;
      float w = __builtin_amdgcn_rcpf(q);                             // v_rcp_f32: 1 ulp
      if (j >= N || j == i) w = 0.f;                                 // no pair: the column is past N, or the row itself
      const float pw = p[m] * w, ww = w * w;
      a0 += pw * dx; a1 += pw * dy;
      b0 += ww * dx; b1 += ww * dy;
      z += w;
      if (p[m] > 0.f) plw += p[m] * __builtin_amdgcn_logf(q);        // - P log2 w (v_log_f32, q >= 1: 1 ulp); ln 2 joins in the fp64 fold
    }
    a0 = wave_sum(a0); a1 = wave_sum(a1); b0 = wave_sum(b0); b1 = wave_sum(b1); z = wave_sum(z); plw = wave_sum(plw);
    if (lane == 0) {
      float* __restrict__ o = part + ((int64_t)i * nchunks + chunk) * 6;
      o[0] = a0; o[1] = a1; o[2] = b0; o[3] = b1; o[4] = z; o[5] = plw;
    }
  }
}

// thread per row: the chunk partials in chunk order -> rowsum [N][6] fp64; the workgroup's rows' (z, plw) in thread order -> wgpart [nwg][2]
__global__ __launch_bounds__(256) void ts_fold_kernel(const float* __restrict__ part, int N, int nchunks, double* __restrict__ rowsum,
                                                      double* __restrict__ wgpart) {
  __shared__ double red[256];
  const int i = blockIdx.x * 256 + threadIdx.x;
  double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (i < N) {
    const float* __restrict__ p = part + (int64_t)i * nchunks * 6;
    for (int c = 0; c < nchunks; ++c)
#pragma unroll
      for (int k = 0; k < 6; ++k) s[k] += (double)p[c * 6 + k];
    s[5] *= 0.69314718055994530942;                                  // log2 -> ln
#pragma unroll
    for (int k = 0; k < 6; ++k) rowsum[(int64_t)i * 6 + k] = s[k];
  }
  const double z = ts_block_sum(s[4], red);
  const double l = ts_block_sum(s[5], red);
  if (threadIdx.x == 0) { wgpart[2 * blockIdx.x] = z; wgpart[2 * blockIdx.x + 1] = l; }
}

struct TsUpdate {
  const double* rowsum; const double* wgpart; const double* p_const; double* colpart; double* trace; double* zsum;
  float* Y; float* inc; float* gain; const int32_t* state;
  int N, nwg, exag_iters, trace_cap; float exag, eta;
};

__global__ __launch_bounds__(256) void ts_update_kernel(const TsUpdate g) {
  __shared__ double red[256];
  const int tid = threadIdx.x, i = blockIdx.x * 256 + tid;
  const int it = g.state[0];
  double Z = 0.0, plw = 0.0;
  for (int w = 0; w < g.nwg; ++w) { Z += g.wgpart[2 * w]; plw += g.wgpart[2 * w + 1]; }      // workgroup order; every thread alike
  const bool early = it < g.exag_iters;
  const double e = early ? (double)g.exag : 1.0;
  const float mom = early ? 0.5f : 0.8f;
  double y0 = 0.0, y1 = 0.0;
  if (i < g.N) {
    const double* __restrict__ s = g.rowsum + (int64_t)i * 6;
    float yn[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const float gr = (float)(4.0 * (e * s[c] - s[2 + c] / Z));
      const float ic = g.inc[2 * i + c];
      float ga = g.gain[2 * i + c];
      ga = ((gr > 0.f) != (ic > 0.f)) ? ga + 0.2f : ga * 0.8f;
      ga = fmaxf(ga, 0.01f);
      const float in = mom * ic - (g.eta * ga) * gr;
      yn[c] = g.Y[2 * i + c] + in;
      g.gain[2 * i + c] = ga;
      g.inc[2 * i + c] = in;
      g.Y[2 * i + c] = yn[c];
    }
    y0 = (double)yn[0]; y1 = (double)yn[1];
  }
  y0 = ts_block_sum(y0, red);
  y1 = ts_block_sum(y1, red);
  if (tid == 0) {
    g.colpart[2 * blockIdx.x] = y0;
    g.colpart[2 * blockIdx.x + 1] = y1;
    if (blockIdx.x == 0) {
      // KL = sum P log P + sum P (-log w) + log Z sum P
      if (it >= 0 && it < g.trace_cap) g.trace[it] = g.p_const[1] + plw + log(Z) * g.p_const[0];
      if (g.zsum) *g.zsum = Z;
    }
  }
}

__global__ __launch_bounds__(256) void ts_centre_kernel(const double* __restrict__ colpart, int N, int nwg, float* __restrict__ Y,
                                                        int32_t* __restrict__ state) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  double m0 = 0.0, m1 = 0.0;
  for (int w = 0; w < nwg; ++w) { m0 += colpart[2 * w]; m1 += colpart[2 * w + 1]; }          // workgroup order; every thread alike
  const float f0 = (float)(m0 / (double)N), f1 = (float)(m1 / (double)N);
  if (i < N) { Y[2 * i] -= f0; Y[2 * i + 1] -= f1; }
  if (i == 0) state[0] += 1;                                         // read by the launches that follow
}

// one wave per row: lanes 0 .. k hold the row's two (k + 1)-lists
__global__ __launch_bounds__(256) void ts_score_kernel(const int32_t* __restrict__ nn_lat, const int32_t* __restrict__ nn_map,
                                                       const uint8_t* __restrict__ labels, int N, int k1, int n_class,
                                                       unsigned long long* __restrict__ counts) {
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (i >= N) return;                                                // whole waves leave
  const bool in = lane < k1;
  const int ia = in ? nn_lat[i * k1 + lane] : -1, ib = in ? nn_map[i * k1 + lane] : -1;
  // self: the entry with index i if the list has it, else the last entry
  const unsigned long long sa = __ballot(in && ia == (int)i), sb = __ballot(in && ib == (int)i);
  const int pa = sa ? __ffsll((long long)sa) - 1 : k1 - 1, pb = sb ? __ffsll((long long)sb) - 1 : k1 - 1;
  const bool va = in && lane != pa && (unsigned)ia < (unsigned)N, vb = in && lane != pb && (unsigned)ib < (unsigned)N;
  bool found = false;
  for (int t = 0; t < k1; ++t) {
    const int jb = __shfl(ib, t, 64);
    const bool okb = __shfl((int)vb, t, 64) != 0;
    found = found || (okb && jb == ia);
  }
  const int kept = __popcll(__ballot(va && found));
  int hit[2] = {0, 0};
  if (labels) {
    const int want = (int)labels[i];
#pragma unroll
    for (int side = 0; side < 2; ++side) {
      const bool v = side ? va : vb;                                 // side 0: the map, side 1: the latent
      const int idx = side ? ia : ib;
      const int cls = v ? (int)labels[idx] : -1;
      int votes = 0;                                                 // lane c counts the votes of class c
      for (int t = 0; t < k1; ++t) votes += __shfl(cls, t, 64) == lane;
      int key = lane < n_class ? votes * 64 + (63 - lane) : -1;      // most votes, then the lowest class id
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) key = max(key, __shfl_xor(key, o, 64));
      hit[side] = (63 - (key & 63)) == want;
    }
  }
  if (lane == 0) {                                                   // integer counters: any order, same sum
    if (kept) atomicAdd(counts, (unsigned long long)kept);
    if (hit[0]) atomicAdd(counts + 1, 1ull);
    if (hit[1]) atomicAdd(counts + 2, 1ull);
  }
}

struct TsLayout { int64_t nx, part, rowsum, wgpart, colpart, prow, total; int nchunks, nwg; };
inline TsLayout ts_layout(int64_t N) {
  TsLayout w;
  w.nchunks = (int)((N + TS_CHUNK - 1) / TS_CHUNK);
  w.nwg = (int)((N + 255) / 256);
  w.nx = 0;
  w.part = w.nx + up256(N * 4);
  w.rowsum = w.part + up256(N * w.nchunks * 6 * 4);
  w.wgpart = w.rowsum + up256(N * 6 * 8);
  w.colpart = w.wgpart + up256((int64_t)w.nwg * 2 * 8);
  w.prow = w.colpart + up256((int64_t)w.nwg * 2 * 8);
  w.total = w.prow + up256(N * 2 * 8);
  return w;
}
inline bool ts_n_ok(int32_t N) { return N >= 4 && N <= TS_MAX_N; }

}  // namespace

extern "C" int sv_tsne_chunk_rows(void) { return TS_CHUNK; }

extern "C" int sv_tsne_workspace_bytes(int32_t N, int64_t* bytes) {
  if (!bytes) return SV_E_BADARG;
  if (!ts_n_ok(N)) return SV_E_UNSUPPORTED;
  *bytes = ts_layout(N).total;
  return SV_OK;
}

extern "C" int sv_tsne_affinities(const float* x, int32_t ldx, int32_t N, int32_t L, double perplexity, int32_t stages, float* P, double* beta,
                                  double* row_entropy, double* p_const, void* workspace, int64_t workspace_bytes, void* stream) {
  if (!x || !P || !beta || !row_entropy || !p_const || !workspace) return SV_E_BADARG;
  if (!al(x, 4) || !al(P, 4) || !al(beta, 8) || !al(row_entropy, 8) || !al(p_const, 8) || !al(workspace, 16)) return SV_E_BADARG;
  if (!ts_n_ok(N) || L < 1 || L > 512 || ldx < L || !(perplexity > 1.0) || !(perplexity < (double)(N - 1)) || stages < 1 || stages > 3)
    return SV_E_UNSUPPORTED;
  const TsLayout w = ts_layout(N);
  if (workspace_bytes < w.total) return SV_E_WORKSPACE;
  char* ws = (char*)workspace;
  hipStream_t st = (hipStream_t)stream;
  float* nx = (float*)(ws + w.nx);
  const int nt = (N + DT_BM - 1) / DT_BM;
  hipLaunchKernelGGL(ts_norm_kernel, dim3((N + 3) / 4), dim3(256), 0, st, x, ldx, N, L, nx);
  SV_LAUNCH_CHECK();
  hipLaunchKernelGGL(ts_dist_kernel, dim3(nt, nt), dim3(256), 0, st, x, ldx, N, L, (int)(!(ldx & 3) && al(x, 16)), (const float*)nx, P);
  SV_LAUNCH_CHECK();
  if (stages < 2) return SV_OK;
  const size_t lds = (size_t)N * 4;
  sv_ensure_dynamic_lds((const void*)ts_row_kernel, lds);
  hipLaunchKernelGGL(ts_row_kernel, dim3(N), dim3(256), lds, st, P, N, log(perplexity), beta, row_entropy);
  SV_LAUNCH_CHECK();
  if (stages < 3) return SV_OK;
  const int nb = (N + 31) / 32;
  hipLaunchKernelGGL(ts_sym_kernel, dim3(nb, nb), dim3(256), 0, st, P, N);
  SV_LAUNCH_CHECK();
  double* prow = (double*)(ws + w.prow);
  hipLaunchKernelGGL(ts_pstat_kernel, dim3((N + 3) / 4), dim3(256), 0, st, (const float*)P, N, prow);
  SV_LAUNCH_CHECK();
  hipLaunchKernelGGL(ts_pfold_kernel, dim3(1), dim3(256), 0, st, (const double*)prow, N, p_const);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

extern "C" int sv_tsne_init(int32_t N, uint64_t seed, float* Y, float* inc, float* gain, int32_t* state, void* stream) {
  if (!Y || !inc || !gain || !state) return SV_E_BADARG;
  if (!al(Y, 4) || !al(inc, 4) || !al(gain, 4) || !al(state, 4)) return SV_E_BADARG;
  if (!ts_n_ok(N)) return SV_E_UNSUPPORTED;
  hipLaunchKernelGGL(ts_init_kernel, dim3((2 * N + 255) / 256), dim3(256), 0, (hipStream_t)stream, N, seed, Y, inc, gain, state);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

extern "C" int sv_tsne_iterate(const float* P, const double* p_const, int32_t N, int32_t iters, float exaggeration, int32_t exag_iters, float eta,
                               float* Y, float* inc, float* gain, int32_t* state, double* kl_trace, int32_t trace_len, double* z_last,
                               void* workspace, int64_t workspace_bytes, void* stream) {
  if (!P || !p_const || !Y || !inc || !gain || !state || !kl_trace || !workspace) return SV_E_BADARG;
  if (!al(P, 4) || !al(p_const, 8) || !al(Y, 4) || !al(inc, 4) || !al(gain, 4) || !al(state, 4) || !al(kl_trace, 8) || !al(z_last, 8) ||
      !al(workspace, 16))
    return SV_E_BADARG;
  if (!ts_n_ok(N) || iters < 0 || trace_len < 0 || exag_iters < 0 || !(exaggeration >= 1.f) || !(exaggeration <= 1e6f) || !(eta > 0.f) ||
      !(eta <= 1e9f))
    return SV_E_UNSUPPORTED;
  const TsLayout w = ts_layout(N);
  if (workspace_bytes < w.total) return SV_E_WORKSPACE;
  char* ws = (char*)workspace;
  hipStream_t st = (hipStream_t)stream;
  float* part = (float*)(ws + w.part);
  double* rowsum = (double*)(ws + w.rowsum);
  double* wgpart = (double*)(ws + w.wgpart);
  double* colpart = (double*)(ws + w.colpart);
  TsUpdate u = {rowsum, wgpart, p_const, colpart, kl_trace, z_last, Y, inc, gain, state, N, w.nwg, exag_iters, trace_len, exaggeration, eta};
  for (int it = 0; it < iters; ++it) {
    hipLaunchKernelGGL(ts_pair_kernel, dim3((N + TS_ROWS - 1) / TS_ROWS, w.nchunks), dim3(256), 0, st, P, (const float*)Y, N, w.nchunks, part);
    SV_LAUNCH_CHECK();
    hipLaunchKernelGGL(ts_fold_kernel, dim3(w.nwg), dim3(256), 0, st, (const float*)part, N, w.nchunks, rowsum, wgpart);
    SV_LAUNCH_CHECK();
    hipLaunchKernelGGL(ts_update_kernel, dim3(w.nwg), dim3(256), 0, st, u);
    SV_LAUNCH_CHECK();
    hipLaunchKernelGGL(ts_centre_kernel, dim3(w.nwg), dim3(256), 0, st, (const double*)colpart, N, w.nwg, Y, state);
    SV_LAUNCH_CHECK();
  }
  return SV_OK;
}

extern "C" int sv_tsne_neighbour_scores(const int32_t* nn_latent, const int32_t* nn_map, const uint8_t* labels, int32_t N, int32_t k,
                                        int32_t n_class, int64_t* counts, void* stream) {
  if (!nn_latent || !nn_map || !counts) return SV_E_BADARG;
  if (!al(nn_latent, 4) || !al(nn_map, 4) || !al(counts, 8)) return SV_E_BADARG;
  if (!ts_n_ok(N) || k < 1 || k + 1 > 32 || k + 1 > N || (labels && (n_class < 2 || n_class > 64))) return SV_E_UNSUPPORTED;
  hipLaunchKernelGGL(ts_score_kernel, dim3((N + 3) / 4), dim3(256), 0, (hipStream_t)stream, nn_latent, nn_map, labels, N, k + 1, n_class,
                     (unsigned long long*)counts);
  SV_LAUNCH_CHECK();
  return SV_OK;
}
