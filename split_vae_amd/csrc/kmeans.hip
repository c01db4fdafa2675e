// k-means cluster report of the latents: Lloyd iterations with R restarts in one pass, k-means++ seeding as an exponential race.
// The definition (norm, distance, the (d, index) order, the race, the fp64 update, the fit loop) is pinned in include/splitvae.h
// (sv_kmeans_*); this file is the kernels.
//   km_norm_kernel     n(v) per row in sv_knn_classify's order (knn.hip's kernel, repeated here: that one is local to its file)
//   km_tile_kernel<P>  workgroup = 64 rows of x against up to 256 columns at a time: knn_tile_kernel's K loop (v_mfma_f32_16x16x4_f32
//                      over the whole of L, k = 4 kk + lane / 16 ascending) with the columns' rows staged beside the x tile.
//                      P = 0: seeding step -- the columns are the R restarts' newest centres; m <- min(m, d), the race key, the
//                             workgroup's argmin under (key, row) per restart
//                      P = 4, 5, 6: assign pass -- restart r owns the columns r 2^P .. r 2^P + K - 1 (K padded to 16 / 32 / 64, so a
//                             16-column fragment belongs to one restart); argmin under (d, k) in registers behind the accumulators
//                             (in-lane over the restart's fragments, then a 16-lane butterfly), then per workgroup: the changed
//                             count and the inertia partial (rows in ascending order, fp64) and the cluster counts (integer atomics)
//   km_pick_kernel     folds the seeding partials in workgroup order: the centre's row -> centroids, its norm, picks
//   km_finish_kernel   folds an assign pass's partials in workgroup order: inertia, changed -> n_iter and the converged flag
//   km_sum_kernel      segmented sum: a thread owns (restart, column) and one of the 8 runs of 128 rows of a chunk; its rows go in
//                      ascending order into fp64 LDS accumulators indexed by the row's cluster (no two threads share one), the next
//                      eight rows in flight meanwhile; the runs are folded in run order
//   km_update_kernel   one workgroup per centroid: folds the chunk partials in chunk order, divides, writes the centroid and its norm
//   km_best_kernel, contingency_kernel
// x is read once per assign pass whatever R while R * Kp <= 256 columns; wider sets re-read the workgroup's own 64-row tile once per
// further 256 columns; fragments and waves past the last column issue no MFMA.  The segmented sum reads a chunk's columns once per
// restart; the workgroups of one chunk are adjacent in the grid.  Once every restart has converged (a counter behind the state, bumped
// by km_finish_kernel) the kernels of the launches that follow return at once: the bits would be the same.
// LDS of the tile kernel: operands as [k][m] images, rows of 80 (x) and 272 (columns) floats: 16-B aligned, pitch % 32 = 16, so the
// two k rows a 32-lane half reads land 16 banks apart and the staging writes put consecutive m of one k row into a wave.
#include "eval_common.hip.h"

namespace {

constexpr int BM = 64, BK = 16, LPA = 80;
constexpr int KM_CHUNK = 1024;                   // rows per chunk of the segmented sum (sv_kmeans_chunk_rows)
constexpr int SUM_G = 8, KM_SUB = KM_CHUNK / SUM_G;   // a chunk is summed as 8 runs of 128 rows, folded in run order
constexpr int IDX_NONE = 0x7fffffff;

struct KmArgs {
  const float* x; const float* cent;             // cent: the first column's row; column (r, k) at cent + r * cstride + k * L
  const float* nx; const float* nc;              // row norms; column (r, k)'s norm at nc[r * nstride + k]
  float* m; float* part_key; int32_t* part_idx;  // seeding: m [N][16], partials [nwg][16]
  int32_t* assign; int32_t* counts; double* part_inertia; int32_t* part_changed;   // assign: partials [nwg][R]
  const int32_t* all_done;                       // assign: state[2 R], the number of converged restarts (NULL: seeding)
  int64_t cstride; uint64_t seed;
  int ldx, N, L, K, R, nstride, step, vecx, vecc;
};

__device__ __forceinline__ bool km_less(float da, int ia, float db, int ib) { return da < db || (da == db && ia < ib); }

__global__ __launch_bounds__(256) void km_norm_kernel(const float* __restrict__ v, int ld, int N, int L, float* __restrict__ out) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= N) return;                            // whole waves leave
  const float* __restrict__ p = v + row * ld;
  float s = 0.f;
  for (int j = lane; j < L; j += 64) s += p[j] * p[j];
  s = wave_sum(s);
  if (lane == 0) out[row] = s;
}

template <int P> struct KmShape {
  static constexpr bool SEED = P == 0;
  static constexpr int BN = SEED ? 16 : 256, NI = SEED ? 1 : 4, NJ = SEED ? 1 : 4, LPB = BN + (SEED ? 32 : 16);
  static constexpr int NB = BN * BK / 256;       // floats of the column tile per thread
};

template <int P> __global__ __launch_bounds__(256) void km_tile_kernel(const KmArgs g) {
  typedef KmShape<P> S;
  constexpr int BN = S::BN, NI = S::NI, NJ = S::NJ, LPB = S::LPB, NB = S::NB;
  constexpr int KP = 1 << P;                       // columns per restart
  __shared__ __attribute__((aligned(16))) float sA[2][BK * LPA];
  __shared__ __attribute__((aligned(16))) float sB[2][BK * LPB];
  __shared__ float sD[16 * 64];                    // assign: the winner's distance per (restart of the group, row); seed: keys per (wave, restart)
  __shared__ int sI[16 * 64];                      // assign: changed flag; seed: rows
  __shared__ int sCnt[S::SEED ? 1 : 1024];         // assign: counts per (restart of the group, cluster)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lk = lane >> 4;
  const int m0 = blockIdx.x * BM;
  if (!S::SEED && *g.all_done == g.R) return;     // every restart sits at its fixed point: the pass would reproduce the same bits
  const int nks = (g.L + BK - 1) / BK;
  const int wm = S::SEED ? wave * 16 : 0, wn = S::SEED ? 0 : wave * 64;
  const int ncols = g.R << P;
  // staging roles: x -- row tid & 63, 4 floats at k = (tid >> 6) * 4; columns -- assign: column tid, 16 floats; seed: column tid & 15, k = tid >> 4
  const int arow = m0 + (tid & 63), ak = (tid >> 6) * 4;
  const float* ap = g.x + (int64_t)arow * g.ldx + ak;
  const bool aok = arow < g.N;
  float nxv[NI][4];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = m0 + wm + i * 16 + lk * 4 + r;
      nxv[i][r] = m < g.N ? g.nx[m] : 0.f;
    }
  for (int col0 = 0; col0 < ncols; col0 += BN) {
    const int bcol = col0 + (S::SEED ? (tid & 15) : tid), bk = S::SEED ? (tid >> 4) : 0;
    const int brr = bcol >> P, bkk = bcol & (KP - 1);
    const bool bok = brr < g.R && bkk < g.K;
    const float* bp = g.cent + (int64_t)brr * g.cstride + (int64_t)bkk * g.L + bk;
    float ra[4], rb[NB];
    auto load = [&](int k0) {
      const int la = g.L - (k0 + ak);
      if (aok && g.vecx && la >= 4) {
        const float4 v = *(const float4*)(ap + k0);
        ra[0] = v.x; ra[1] = v.y; ra[2] = v.z; ra[3] = v.w;
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) ra[i] = (aok && i < la) ? ap[k0 + i] : 0.f;
      }
      const int lb = g.L - (k0 + bk);
      if (NB == 16 && bok && g.vecc && lb >= NB) {
#pragma unroll
        for (int q = 0; q < NB / 4; ++q) {
          const float4 v = *(const float4*)(bp + k0 + q * 4);
          rb[q * 4] = v.x; rb[q * 4 + 1] = v.y; rb[q * 4 + 2] = v.z; rb[q * 4 + 3] = v.w;
        }
      } else {
#pragma unroll
        for (int i = 0; i < NB; ++i) rb[i] = (bok && i < lb) ? bp[k0 + i] : 0.f;
      }
    };
    auto store = [&](int buf) {
#pragma unroll
      for (int i = 0; i < 4; ++i) sA[buf][(ak + i) * LPA + (tid & 63)] = ra[i];
#pragma unroll
      for (int i = 0; i < NB; ++i) sB[buf][(bk + i) * LPB + (S::SEED ? (tid & 15) : tid)] = rb[i];
    };
    const int njv = S::SEED ? 1 : min(NJ, max(0, (ncols - col0 - wn + 15) >> 4));   // this wave's fragments that hold a column (wave-uniform)
    f32x4 acc[NI][NJ];
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if constexpr (!S::SEED)
      for (int e = tid; e < 1024; e += 256) sCnt[e] = 0;
    load(0);
    store(0);
    __syncthreads();                               // (also: every thread is done with the previous group's sD / sI / sCnt)
    for (int ks = 0; ks < nks; ++ks) {
      const int buf = ks & 1;
      const bool more = ks + 1 < nks;
      if (more) load((ks + 1) * BK);
      const float* cA = sA[buf];
      const float* cB = sB[buf];
#pragma unroll
      for (int kk = 0; kk < BK / 4; ++kk) {
        if (njv == 0) break;                       // a wave without a column only stages
        const int k = kk * 4 + lk;
        float a[NI], b[NJ];
#pragma unroll
        for (int i = 0; i < NI; ++i) a[i] = cA[k * LPA + wm + i * 16 + lr];
#pragma unroll
        for (int j = 0; j < NJ; ++j) b[j] = cB[k * LPB + wn + j * 16 + lr];
#pragma unroll
        for (int j = 0; j < NJ; ++j)
          if (j < njv) {
#pragma unroll
            for (int i = 0; i < NI; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
          }
      }
      if (more) store(buf ^ 1);
      __syncthreads();
    }
    // D: row = (lane >> 4) * 4 + reg, column = lane & 15 of each fragment.  d = max(0, (n(x) + n(c)) - 2 dot)
    if constexpr (S::SEED) {
      const int rho = lr;
      const bool cok = rho < g.R;
      const float ncv = cok ? g.nc[rho * g.nstride] : 0.f;
      const Philox ph(g.seed ^ KM_KEY);
      float bkey = __builtin_inff();
      int bidx = IDX_NONE;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + wm + lk * 4 + r;
        if (cok && m < g.N) {
          float d = fmaxf(0.f, (nxv[0][r] + ncv) - 2.f * acc[0][0][r]);
          float* mp = g.m + (int64_t)m * 16 + rho;
          if (g.step > 1) d = fminf(*mp, d);
          *mp = d;
          uint32_t c[4] = {(uint32_t)m, (uint32_t)rho, (uint32_t)g.step, KM_TAG};
          ph(c);
          const float key = d == 0.f ? __builtin_inff() : -logf(u32_to_unit_open(c[0])) / d;
          if (km_less(key, m, bkey, bidx)) { bkey = key; bidx = m; }
        }
      }
#pragma unroll
      for (int o = 16; o < 64; o <<= 1) {
        const float ok_ = __shfl_xor(bkey, o, 64);
        const int oi = __shfl_xor(bidx, o, 64);
        if (km_less(ok_, oi, bkey, bidx)) { bkey = ok_; bidx = oi; }
      }
      if (lk == 0) { sD[wave * 16 + lr] = bkey; sI[wave * 16 + lr] = bidx; }
      __syncthreads();
      if (tid < 16) {
        float k0 = sD[tid];
        int i0 = sI[tid];
#pragma unroll
        for (int w = 1; w < 4; ++w)
          if (km_less(sD[w * 16 + tid], sI[w * 16 + tid], k0, i0)) { k0 = sD[w * 16 + tid]; i0 = sI[w * 16 + tid]; }
        g.part_key[(int64_t)blockIdx.x * 16 + tid] = k0;
        g.part_idx[(int64_t)blockIdx.x * 16 + tid] = i0;
      }
    } else {
      constexpr int FR = KP / 16;                  // fragments per restart
      constexpr int NG = NJ / FR;                  // restarts per wave slab
      const int rho0 = col0 >> P;                  // first restart of this column group
      float bd[NG][NI][4];
      int bi[NG][NI][4];
#pragma unroll
      for (int gq = 0; gq < NG; ++gq) {
        const int rho = (col0 + wn + gq * KP) >> P;
        if (rho >= g.R) continue;                  // wave-uniform: no restart behind these columns
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
          for (int r = 0; r < 4; ++r) { bd[gq][i][r] = __builtin_inff(); bi[gq][i][r] = IDX_NONE; }
#pragma unroll
        for (int f = 0; f < FR; ++f) {
          const int j = gq * FR + f, kk = f * 16 + lr;
          const bool cok = rho < g.R && kk < g.K;  // a padded column never wins: it stays (+inf, IDX_NONE)
          const float ncv = cok ? g.nc[rho * g.nstride + kk] : 0.f;
#pragma unroll
          for (int i = 0; i < NI; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const float d = fmaxf(0.f, (nxv[i][r] + ncv) - 2.f * acc[i][j][r]);
              if (cok && km_less(d, kk, bd[gq][i][r], bi[gq][i][r])) { bd[gq][i][r] = d; bi[gq][i][r] = kk; }
            }
        }
#pragma unroll
        for (int o = 1; o < 16; o <<= 1)
#pragma unroll
          for (int i = 0; i < NI; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const float od = __shfl_xor(bd[gq][i][r], o, 64);
              const int oi = __shfl_xor(bi[gq][i][r], o, 64);
              if (km_less(od, oi, bd[gq][i][r], bi[gq][i][r])) { bd[gq][i][r] = od; bi[gq][i][r] = oi; }
            }
        // every lane of a 16-lane row holds the winners; lane lr = reg writes the rows (lane >> 4) * 4 + reg
        {
          const int rl = rho - rho0;
#pragma unroll
          for (int i = 0; i < NI; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int ml = i * 16 + lk * 4 + r, m = m0 + ml;
              if (lr == r && m < g.N) {
                int32_t* ap_ = g.assign + (int64_t)rho * g.N + m;
                const int old = *ap_;
                *ap_ = bi[gq][i][r];
                sD[rl * 64 + ml] = bd[gq][i][r];
                sI[rl * 64 + ml] = old != bi[gq][i][r];
                if ((unsigned)bi[gq][i][r] < 64u) atomicAdd(&sCnt[rl * 64 + bi[gq][i][r]], 1);   // integer: any order, same sum (always true for finite inputs)
              }
            }
        }
      }
      __syncthreads();
      const int nrho = min(BN >> P, g.R - rho0);
      if (tid < nrho) {
        const int rows = min(BM, g.N - m0);
        double s = 0.0;
        int ch = 0;
        for (int ml = 0; ml < rows; ++ml) { s += (double)sD[tid * 64 + ml]; ch += sI[tid * 64 + ml]; }
        g.part_inertia[(int64_t)blockIdx.x * g.R + rho0 + tid] = s;
        g.part_changed[(int64_t)blockIdx.x * g.R + rho0 + tid] = ch;
      }
      for (int e = tid; e < nrho * 64; e += 256) {
        const int v = sCnt[e], kk = e & 63;
        if (v && kk < g.K) atomicAdd(&g.counts[(rho0 + (e >> 6)) * g.K + kk], v);
      }
    }
  }
}

// one workgroup per restart: the centre of seeding step `step` -> centroids[r][step], nc, picks
__global__ __launch_bounds__(256) void km_pick_kernel(const float* __restrict__ x, int ldx, int N, int L, int K, int step, uint64_t seed,
                                                      const float* __restrict__ nx, const float* __restrict__ part_key,
                                                      const int32_t* __restrict__ part_idx, int nwg, float* __restrict__ cent,
                                                      float* __restrict__ nc, int32_t* __restrict__ picks) {
  __shared__ float sk[256];
  __shared__ int si[256];
  const int r = blockIdx.x, tid = threadIdx.x;
  int row;
  if (step == 0) {
    uint32_t c[4] = {0u, (uint32_t)r, 0u, KM_TAG};
    Philox(seed ^ KM_KEY)(c);
    row = (int)(((uint64_t)c[0] * (uint64_t)N) >> 32);
  } else {
    float bk = __builtin_inff();
    int bi = IDX_NONE;
    for (int w = tid; w < nwg; w += 256) {
      const float k = part_key[(int64_t)w * 16 + r];
      const int i = part_idx[(int64_t)w * 16 + r];
      if (km_less(k, i, bk, bi)) { bk = k; bi = i; }
    }
    sk[tid] = bk; si[tid] = bi;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {            // a minimum under a total order: the tree's shape does not matter
      if (tid < o && km_less(sk[tid + o], si[tid + o], sk[tid], si[tid])) { sk[tid] = sk[tid + o]; si[tid] = si[tid + o]; }
      __syncthreads();
    }
    row = si[0];
    if ((unsigned)row >= (unsigned)N) row = 0;     // (cannot happen: every workgroup holds at least one row)
  }
  const float* __restrict__ p = x + (int64_t)row * ldx;
  float* __restrict__ q = cent + ((int64_t)r * K + step) * L;
  for (int j = tid; j < L; j += 256) q[j] = p[j];
  if (tid == 0) {
    nc[r * K + step] = nx[row];
    if (picks) picks[r * K + step] = row;
  }
}

// one wave per restart: the partials of an assign pass in workgroup order (lane l takes l, l + 64, ..., then the lanes in lane order)
__global__ __launch_bounds__(64) void km_finish_kernel(const double* __restrict__ part_inertia, const int32_t* __restrict__ part_changed, int nwg,
                                                       int R, double* __restrict__ inertia, int32_t* __restrict__ n_iter, int32_t* __restrict__ state) {
  const int r = blockIdx.x, lane = threadIdx.x;
  if (state[2 * R] == R) return;                   // (set by an earlier launch: every workgroup of this one reads the same value)
  double s = 0.0;
  int ch = 0;
  for (int w = lane; w < nwg; w += 64) { s += part_inertia[(int64_t)w * R + r]; ch += part_changed[(int64_t)w * R + r]; }
  double tot = 0.0;
  int cht = 0;
  for (int l = 0; l < 64; ++l) { tot += __shfl(s, l, 64); cht += __shfl(ch, l, 64); }
  if (lane == 0) {
    const int t = state[2 * r], done = state[2 * r + 1];
    inertia[r] = tot;
    if (!done) {
      n_iter[r] = t;
      if (t > 0 && cht == 0) {
        state[2 * r + 1] = 1;
        atomicAdd(&state[2 * R], 1);               // integer: read by the launches that follow
      }
    }
    state[2 * r] = t + 1;
  }
}

// C columns x SUM_G row runs per workgroup (C = 32, or 16 when K > 32: the accumulators fill 64 KiB at most; 16 columns at K = 30 -- half the LDS,
// 64-byte row segments -- measured 158 us against 109 us at N = 73 257, L = 256, R = 8).  Thread (run g, column c)
// walks the 128 rows of its run in ascending order; the runs are then folded in run order.
template <int C> __global__ __launch_bounds__(SUM_G * C) void km_sum_kernel(const float* __restrict__ x, int ldx, int N, int L, int K, int R,
                                                                            const int32_t* __restrict__ assign, double* __restrict__ part,
                                                                            const int32_t* __restrict__ all_done) {
  extern __shared__ __attribute__((aligned(16))) double acc[];      // [SUM_G][K][C]
  if (*all_done == R) return;
  const int tid = threadIdx.x, c = tid % C, g = tid / C, chunk = blockIdx.x;
  const int s = blockIdx.y * C + c;
  const bool valid = s < R * L;
  const int r = valid ? s / L : 0, j = valid ? s - r * L : 0;
  double* __restrict__ mine = acc + (size_t)g * K * C + c;
  for (int k = 0; k < K; ++k) mine[k * C] = 0.0;
  const int i0 = chunk * KM_CHUNK + g * KM_SUB, i1 = min(N, i0 + KM_SUB);
  const int32_t* __restrict__ a = assign + (int64_t)r * N;
  const float* __restrict__ xp = x + j;
  if (valid) {
    int av[8], an[8];
    float xv[8], xn[8];
    auto load = [&](int i, int (&ao)[8], float (&xo)[8]) {
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const bool ok = i + u < i1;
        ao[u] = ok ? a[i + u] : -1;
        xo[u] = ok ? xp[(int64_t)(i + u) * ldx] : 0.f;
      }
    };
    load(i0, av, xv);
    for (int i = i0; i < i1; i += 8) {
      load(i + 8, an, xn);                         // the next eight rows are in flight while these go into the accumulators
#pragma unroll
      for (int u = 0; u < 8; ++u)                  // ascending rows
        if ((unsigned)av[u] < (unsigned)K) mine[av[u] * C] += (double)xv[u];
#pragma unroll
      for (int u = 0; u < 8; ++u) { av[u] = an[u]; xv[u] = xn[u]; }
    }
  }
  __syncthreads();
  for (int e = tid; e < K * C; e += SUM_G * C) {
    const int k = e / C, cc = e - k * C, s2 = blockIdx.y * C + cc;
    if (s2 >= R * L) continue;
    double sum = 0.0;
#pragma unroll
    for (int q = 0; q < SUM_G; ++q) sum += acc[((size_t)q * K + k) * C + cc];      // run order
    const int r2 = s2 / L, j2 = s2 - r2 * L;
    part[(((int64_t)chunk * R + r2) * K + k) * L + j2] = sum;
  }
}

// one workgroup per centroid: thread t takes the columns t, t + 256 (chunk partials in chunk order, the division), then wave 0 takes the norm
// of the new row in km_norm_kernel's order
__global__ __launch_bounds__(256) void km_update_kernel(const double* __restrict__ part, int nchunks, int RK, int L, int32_t* __restrict__ counts,
                                                        float* __restrict__ cent, float* __restrict__ nc, const int32_t* __restrict__ all_done, int R) {
  __shared__ float sv[512];
  if (*all_done == R) return;
  const int rk = blockIdx.x, tid = threadIdx.x;
  const int cnt = counts[rk];
  float* __restrict__ c = cent + (int64_t)rk * L;
  for (int j = tid; j < L; j += 256) {
    float v;
    if (cnt > 0) {
      const double* __restrict__ p = part + (int64_t)rk * L + j;
      const int64_t stride = (int64_t)RK * L;
      double sum = 0.0;
      int ch = 0;
      for (; ch + 8 <= nchunks; ch += 8) {          // eight loads in flight, added in chunk order
        double t[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) t[u] = p[(ch + u) * stride];
#pragma unroll
        for (int u = 0; u < 8; ++u) sum += t[u];
      }
      for (; ch < nchunks; ++ch) sum += p[ch * stride];
      v = (float)(sum / (double)cnt);
      c[j] = v;
    } else {
      v = c[j];                                    // an empty cluster keeps its centroid
    }
    sv[j] = v;
  }
  __syncthreads();
  if (tid < 64) {
    float s = 0.f;
    for (int j = tid; j < L; j += 64) s += sv[j] * sv[j];
    s = wave_sum(s);                               // km_norm_kernel's order
    if (tid == 0) {
      nc[rk] = s;
      counts[rk] = 0;                              // the next assign pass counts from zero
    }
  }
}

__global__ __launch_bounds__(64) void km_best_kernel(const double* __restrict__ inertia, int R, int32_t* __restrict__ best) {
  if (threadIdx.x == 0) {
    int b = 0;
    for (int r = 1; r < R; ++r)
      if (inertia[r] < inertia[b]) b = r;          // ties to the lower r
    *best = b;
  }
}

__global__ __launch_bounds__(256) void contingency_kernel(const int32_t* __restrict__ a, const int32_t* __restrict__ b, int N, int Ka, int Kb,
                                                          int32_t* __restrict__ counts) {
  __shared__ int h[64 * 64];
  const int tid = threadIdx.x, cells = Ka * Kb;
  for (int e = tid; e < cells; e += 256) h[e] = 0;
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < N; i += (int64_t)gridDim.x * 256) {
    const int u = a[i], v = b[i];
    if ((unsigned)u < (unsigned)Ka && (unsigned)v < (unsigned)Kb) atomicAdd(&h[u * Kb + v], 1);
  }
  __syncthreads();
  for (int e = tid; e < cells; e += 256)
    if (h[e]) atomicAdd(&counts[e], h[e]);         // integer counters: any order, same sum
}

struct KmLayout { int64_t nx, nc, m, pkey, pidx, pin, pch, sums, total; int nwg, nchunks; };
inline KmLayout km_layout(int64_t N, int64_t L, int64_t K, int64_t R) {
  KmLayout w;
  w.nwg = (int)((N + BM - 1) / BM);
  w.nchunks = (int)((N + KM_CHUNK - 1) / KM_CHUNK);
  w.nx = 0;
  w.nc = w.nx + up256(N * 4);
  w.m = w.nc + up256(R * K * 4);
  w.pkey = w.m + up256(N * 16 * 4);
  w.pidx = w.pkey + up256((int64_t)w.nwg * 16 * 4);
  w.pin = w.pidx + up256((int64_t)w.nwg * 16 * 4);
  w.pch = w.pin + up256((int64_t)w.nwg * R * 8);
  w.sums = w.pch + up256((int64_t)w.nwg * R * 4);
  w.total = w.sums + up256((int64_t)w.nchunks * R * K * L * 8);
  return w;
}
inline bool km_sizes_ok(int32_t N, int32_t L, int32_t K, int32_t R) {
  return L >= 1 && L <= 512 && K >= 2 && K <= 64 && R >= 1 && R <= 16 && N >= K && N < (1 << 24);
}

void km_launch_tile(int P, int nwg, hipStream_t st, const KmArgs& g) {
  if (P == 0) hipLaunchKernelGGL(km_tile_kernel<0>, dim3(nwg), dim3(256), 0, st, g);
  else if (P == 4) hipLaunchKernelGGL(km_tile_kernel<4>, dim3(nwg), dim3(256), 0, st, g);
  else if (P == 5) hipLaunchKernelGGL(km_tile_kernel<5>, dim3(nwg), dim3(256), 0, st, g);
  else hipLaunchKernelGGL(km_tile_kernel<6>, dim3(nwg), dim3(256), 0, st, g);
}

}  // namespace

extern "C" int sv_kmeans_chunk_rows(void) { return KM_CHUNK; }

extern "C" int sv_kmeans_workspace_bytes(int32_t N, int32_t L, int32_t K, int32_t R, int64_t* bytes) {
  if (!bytes) return SV_E_BADARG;
  if (!km_sizes_ok(N, L, K, R)) return SV_E_UNSUPPORTED;
  *bytes = km_layout(N, L, K, R).total;
  return SV_OK;
}

extern "C" int sv_kmeans_seed(const float* x, int32_t ldx, int32_t N, int32_t L, int32_t K, int32_t R, uint64_t seed, float* centroids,
                              int32_t* picks, void* workspace, int64_t workspace_bytes, void* stream) {
  if (!x || !centroids || !workspace) return SV_E_BADARG;
  if (!al(x, 4) || !al(centroids, 4) || !al(picks, 4) || !al(workspace, 16)) return SV_E_BADARG;
  if (!km_sizes_ok(N, L, K, R) || ldx < L) return SV_E_UNSUPPORTED;
  const KmLayout w = km_layout(N, L, K, R);
  if (workspace_bytes < w.total) return SV_E_WORKSPACE;
  char* ws = (char*)workspace;
  hipStream_t st = (hipStream_t)stream;
  float* nx = (float*)(ws + w.nx);
  float* nc = (float*)(ws + w.nc);
  hipLaunchKernelGGL(km_norm_kernel, dim3((N + 3) / 4), dim3(256), 0, st, x, ldx, N, L, nx);
  SV_LAUNCH_CHECK();
  KmArgs g = {};
  g.x = x; g.nx = nx; g.m = (float*)(ws + w.m); g.part_key = (float*)(ws + w.pkey); g.part_idx = (int32_t*)(ws + w.pidx);
  g.cstride = (int64_t)K * L; g.seed = seed; g.ldx = ldx; g.N = N; g.L = L; g.K = 1; g.R = R; g.nstride = K;
  g.vecx = !(ldx & 3) && al(x, 16); g.vecc = 0;
  for (int k = 0; k < K; ++k) {
    if (k) {                                       // distances to centre k - 1, the race for centre k
      g.cent = centroids + (int64_t)(k - 1) * L;
      g.nc = nc + (k - 1);
      g.step = k;
      km_launch_tile(0, w.nwg, st, g);
      SV_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(km_pick_kernel, dim3(R), dim3(256), 0, st, x, ldx, N, L, K, k, seed, (const float*)nx, (const float*)g.part_key,
                       (const int32_t*)g.part_idx, w.nwg, centroids, nc, picks);
    SV_LAUNCH_CHECK();
  }
  return SV_OK;
}

extern "C" int sv_kmeans_iterate(const float* x, int32_t ldx, int32_t N, int32_t L, int32_t K, int32_t R, int32_t iters, int32_t resume,
                                 float* centroids, int32_t* assign, int32_t* counts, double* inertia, int32_t* n_iter, int32_t* state,
                                 void* workspace, int64_t workspace_bytes, void* stream) {
  if (!x || !centroids || !assign || !counts || !inertia || !n_iter || !state || !workspace) return SV_E_BADARG;
  if (!al(x, 4) || !al(centroids, 4) || !al(assign, 4) || !al(counts, 4) || !al(inertia, 8) || !al(n_iter, 4) || !al(state, 4) ||
      !al(workspace, 16))
    return SV_E_BADARG;
  if (!km_sizes_ok(N, L, K, R) || ldx < L || iters < 0 || (resume != 0 && resume != 1)) return SV_E_UNSUPPORTED;
  const KmLayout w = km_layout(N, L, K, R);
  if (workspace_bytes < w.total) return SV_E_WORKSPACE;
  char* ws = (char*)workspace;
  hipStream_t st = (hipStream_t)stream;
  float* nx = (float*)(ws + w.nx);
  float* nc = (float*)(ws + w.nc);
  double* sums = (double*)(ws + w.sums);
  const int P = K <= 16 ? 4 : K <= 32 ? 5 : 6;
  KmArgs g = {};
  g.x = x; g.cent = centroids; g.nx = nx; g.nc = nc; g.assign = assign; g.counts = counts;
  g.part_inertia = (double*)(ws + w.pin); g.part_changed = (int32_t*)(ws + w.pch);
  g.cstride = (int64_t)K * L; g.ldx = ldx; g.N = N; g.L = L; g.K = K; g.R = R; g.nstride = K; g.all_done = state + 2 * R;
  g.vecx = !(ldx & 3) && al(x, 16); g.vecc = !(L & 3) && al(centroids, 16);
  // the norms belong to (x, centroids), not to the call: a resumed call recomputes the same bits
  hipLaunchKernelGGL(km_norm_kernel, dim3((N + 3) / 4), dim3(256), 0, st, x, ldx, N, L, nx);
  SV_LAUNCH_CHECK();
  hipLaunchKernelGGL(km_norm_kernel, dim3((R * K + 3) / 4), dim3(256), 0, st, (const float*)centroids, L, R * K, L, nc);
  SV_LAUNCH_CHECK();
  auto assign_pass = [&]() -> int {
    km_launch_tile(P, w.nwg, st, g);
    SV_LAUNCH_CHECK();
    hipLaunchKernelGGL(km_finish_kernel, dim3(R), dim3(64), 0, st, (const double*)g.part_inertia, (const int32_t*)g.part_changed, w.nwg, R,
                       inertia, n_iter, state);
    SV_LAUNCH_CHECK();
    return SV_OK;
  };
  if (!resume) {
    if (hipMemsetAsync(state, 0, ((size_t)R * 2 + 1) * 4, st) != hipSuccess) return (int)hipGetLastError();
    if (hipMemsetAsync(counts, 0, (size_t)R * K * 4, st) != hipSuccess) return (int)hipGetLastError();
    const int rc = assign_pass();
    if (rc) return rc;
  }
  for (int it = 0; it < iters; ++it) {
    if (K <= 32)
      hipLaunchKernelGGL(km_sum_kernel<32>, dim3(w.nchunks, (R * L + 31) / 32), dim3(SUM_G * 32), (size_t)SUM_G * K * 32 * 8, st, x, ldx, N, L, K, R,
                         (const int32_t*)assign, sums, (const int32_t*)(state + 2 * R));
    else
      hipLaunchKernelGGL(km_sum_kernel<16>, dim3(w.nchunks, (R * L + 15) / 16), dim3(SUM_G * 16), (size_t)SUM_G * K * 16 * 8, st, x, ldx, N, L, K, R,
                         (const int32_t*)assign, sums, (const int32_t*)(state + 2 * R));
    SV_LAUNCH_CHECK();
    hipLaunchKernelGGL(km_update_kernel, dim3(R * K), dim3(256), 0, st, (const double*)sums, w.nchunks, R * K, L, counts, centroids, nc,
                       (const int32_t*)(state + 2 * R), R);
    SV_LAUNCH_CHECK();
    const int rc = assign_pass();
    if (rc) return rc;
  }
  return SV_OK;
}

extern "C" int sv_kmeans_best(const double* inertia, int32_t R, int32_t* best, void* stream) {
  if (!inertia || !best || !al(inertia, 8) || !al(best, 4)) return SV_E_BADARG;
  if (R < 1 || R > 16) return SV_E_UNSUPPORTED;
  hipLaunchKernelGGL(km_best_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, inertia, R, best);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

extern "C" int sv_contingency(const int32_t* a, const int32_t* b, int32_t N, int32_t Ka, int32_t Kb, int32_t* counts, void* stream) {
  if (!a || !b || !counts || !al(a, 4) || !al(b, 4) || !al(counts, 4)) return SV_E_BADARG;
  if (N < 1 || Ka < 1 || Ka > 64 || Kb < 1 || Kb > 64) return SV_E_UNSUPPORTED;
  const int grid = (int)((((int64_t)N + 255) / 256 + 15) / 16);   // 16 rows per thread
  hipLaunchKernelGGL(contingency_kernel, dim3(grid < 1 ? 1 : grid), dim3(256), 0, (hipStream_t)stream, a, b, N, Ka, Kb, counts);
  SV_LAUNCH_CHECK();
  return SV_OK;
}
