// Per-dimension latent report: active units (Burda et al. 2016) and Chen et al. 2018's decomposition of a block's KL term into
// index-code MI, total correlation and dimension-wise KL.  Every sample z_ij is scored under every image's posterior of the SAME
// dimension, q(z_j | x_n): one log-sum-exp per (image, dimension) over all images, N * N * L exponentials; the scores never exist
// in memory.  The definitions are pinned in include/splitvae.h (sv_latent_dims_prepare / _lse / _finish).
//   ld_elem_kernel    one thread per (image, dimension): lc = -log sig - 1/2 log 2 pi (fp32), own = lc - 1/2 eps^2 (fp64); eps is
//                     an input or the Philox stream of sv_latent_info_draw
//   ld_cols_kernel    one workgroup per dimension: mean, population variance (two passes) and closed-form KL of the column, fp64
//   ld_tile_kernel    workgroup = (32 queries, 64 dimensions, chunk of LD_CHUNK references).  A LANE OWNS A DIMENSION, a wave owns
//                     8 queries: their z and the running (max, sum) per (query, dimension) stay in registers -- no cross-lane
//                     step anywhere.  The four waves share the references: 32 rows x 64 dimensions of (mu, rsig, lc) are staged
//                     through LDS, double-buffered (global -> registers before the tile is computed, registers -> LDS after it,
//                     one barrier per tile); a lane reads its column as ds_read_b32 of consecutive dwords (conflict-free).
//                     References are pushed in groups of 8 rows: the group's maximum, ONE rescale of the running sum, then one
//                     v_exp_f32 per element -- 9/8 exponentials per element and no select, where a per-element push costs one
//                     exponential, two selects and a dependent chain.  The kernel is bound by the transcendental pipe and the
//                     plain VALU together (an exponential issues at a quarter of the rate of a v_fma_f32).
//   ld_merge_kernel   one thread per (query, dimension) folds the chunk partials in chunk order, in fp64
//   ld_mean_kernel    one workgroup per dimension: MI_j, dwKL_j and the mean of lse_.j, in the fixed order of ld_cols_kernel
//   ld_block_kernel   one workgroup: TC and the block's dwKL, the dimensions added in ascending order
// No atomics; the partial of (query, dimension, chunk) depends on z_ij and column j of the chunk's rows only: the same inputs give
// the same bits wherever the query row or the column sits.
#include "eval_common.hip.h"

namespace {

constexpr int LD_CHUNK = 4096;                     // reference rows per chunk (sv_latent_dims_chunk_rows)
constexpr int QT = 32, QW = 8, RT = 32, DT = 64, GR = 8;   // queries per workgroup / per wave, rows per tile, dimensions, rows per group
constexpr int LMAX = 512;

struct ElemArgs {
  const float* mu; const float* sig; const float* eps;
  float* lc; double* own; double* cols;
  int ldm, lds, lde, ldc, N, L, block;
  uint64_t seed; int64_t sample_offset;
};

__global__ __launch_bounds__(256) void ld_elem_kernel(const ElemArgs g) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)g.N * g.L) return;
  const int64_t b = idx / g.L;
  const int j = (int)(idx - b * g.L);
  const float sg = g.sig[b * g.lds + j];
  // eps = NULL: the numbers sv_latent_info_draw drew for this image, block and dimension
  const float ep = g.eps ? g.eps[b * g.lde + j] : LATENT_INFO_EPS(latent_info_stream(g.seed), (uint64_t)(g.sample_offset + b), g.block, j);
  const float lc = (float)(-(double)logf(sg) - HALF_LOG_2PI);
  g.lc[b * g.ldc + j] = lc;
  g.own[idx] = (double)lc - 0.5 * (double)ep * (double)ep;
}

__global__ __launch_bounds__(256) void ld_cols_kernel(const ElemArgs g) {
  __shared__ double part[256];
  const int j = blockIdx.x;
  double sm = 0.0, sk = 0.0;
  for (int b = threadIdx.x; b < g.N; b += 256) {
    const double mu = (double)g.mu[(int64_t)b * g.ldm + j], sg = (double)g.sig[(int64_t)b * g.lds + j];
    sm += mu;
    sk += 0.5 * (mu * mu + sg * sg - 1.0) - log(sg);
  }
  const double mean = block_sum_ordered(sm, part) / (double)g.N;
  const double kl = block_sum_ordered(sk, part) / (double)g.N;
  double sv = 0.0;
  for (int b = threadIdx.x; b < g.N; b += 256) {
    const double d = (double)g.mu[(int64_t)b * g.ldm + j] - mean;
    sv += d * d;
  }
  const double var = block_sum_ordered(sv, part) / (double)g.N;
  if (threadIdx.x == 0) {
    g.cols[j] = mean; g.cols[g.L + j] = var; g.cols[2 * g.L + j] = kl;
  }
}

struct LseArgs {
  const float* z; const float* mu; const float* rsig; const float* lc;
  float* ws;                                       // [Nq][nchunks][L][2]: (max, sum)
  double* lse;                                     // [Nq, L], row pitch ldl
  int ldz, ldm, ldr, ldc, ldl, Nq, Nr, L, nchunks, vecm, vecr, vecc;
};

// 4 floats of row `row` from column `col` (lim of them exist); rows past `rows` and columns past lim read as 0
__device__ __forceinline__ f32x4 ld_load4(const float* __restrict__ P, int ld, int row, int rows, int col, int lim, bool vec) {
  f32x4 r = {0.f, 0.f, 0.f, 0.f};
  if (row < rows && lim > 0) {
    const float* p = P + (int64_t)row * ld + col;
    if (vec && lim >= 4) {
      r = *(const f32x4*)p;
    } else {
      r[0] = p[0];
      if (lim > 1) r[1] = p[1];
      if (lim > 2) r[2] = p[2];
      if (lim > 3) r[3] = p[3];
    }
  }
  return r;
}

// (m, s) <- (m, s) + sum_k exp(e[k]), k < nv (FULL: nv = GR).  m = -inf, s = 0 is the empty state; a group whose scores are all
// -inf (a quadratic form that overflowed) leaves s = 0 at a finite m.
template <bool FULL>
__device__ __forceinline__ void ld_push(float& m, float& s, const float zq, const float (&rm)[GR], const float (&rr)[GR],
                                        const float (&rc)[GR], const int nv) {
  float e[GR];
#pragma unroll
  for (int k = 0; k < GR; ++k) {
    const float u = (zq - rm[k]) * rr[k];
    e[k] = __builtin_fmaf(-0.5f, u * u, rc[k]);    // 0.5 * u^2 is exact: one rounding of lc - 0.5 u^2
    if (!FULL) e[k] = k < nv ? e[k] : -__builtin_inff();
  }
  float gm = e[0];
#pragma unroll
  for (int k = 1; k < GR; ++k) gm = __builtin_fmaxf(gm, e[k]);
  const float mn = __builtin_fmaxf(m, __builtin_fmaxf(gm, -3.0e38f));          // finite: (-inf) - (-inf) never evaluated
  float acc = s * __builtin_amdgcn_exp2f((m - mn) * LOG2E);
#pragma unroll
  for (int k = 0; k < GR; ++k) acc += __builtin_amdgcn_exp2f((e[k] - mn) * LOG2E);
  s = acc;
  m = mn;
}

__global__ __launch_bounds__(256) void ld_tile_kernel(const LseArgs g) {
  __shared__ __attribute__((aligned(16))) float sR[2][RT][3][DT];              // 48 KiB: [buffer][row][mu, rsig, lc][dimension]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q0 = blockIdx.x * QT + wave * QW, j0 = blockIdx.y * DT, chunk = blockIdx.z;
  const int c0 = chunk * LD_CHUNK, c1 = min(g.Nr, c0 + LD_CHUNK);
  const int j = j0 + lane;
  const bool jin = j < g.L;
  float zq[QW], sm[QW], ss[QW];
#pragma unroll
  for (int q = 0; q < QW; ++q) {
    const int qi = q0 + q;
    zq[q] = (jin && qi < g.Nq) ? g.z[(int64_t)qi * g.ldz + j] : 0.f;
    sm[q] = -__builtin_inff();
    ss[q] = 0.f;
  }
  // staging roles: rows tid >> 4 and 16 + (tid >> 4) of the tile, 4 dimensions from (tid & 15) * 4
  const int srow = tid >> 4, sc = (tid & 15) * 4, lim = g.L - j0 - sc;
  f32x4 rg[2][3];
  auto load = [&](int n0) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int row = n0 + srow + 16 * h;
      rg[h][0] = ld_load4(g.mu, g.ldm, row, c1, j0 + sc, lim, g.vecm);
      rg[h][1] = ld_load4(g.rsig, g.ldr, row, c1, j0 + sc, lim, g.vecr);
      rg[h][2] = ld_load4(g.lc, g.ldc, row, c1, j0 + sc, lim, g.vecc);
    }
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int a = 0; a < 3; ++a) *(f32x4*)&sR[buf][srow + 16 * h][a][sc] = rg[h][a];
  };
  load(c0);
  store(0);
  __syncthreads();
  int buf = 0;
  for (int n0 = c0; n0 < c1; n0 += RT, buf ^= 1) {
    const bool more = n0 + RT < c1;
    if (more) load(n0 + RT);
    const int rows = min(RT, c1 - n0);
    for (int r0 = 0; r0 < rows; r0 += GR) {        // RT is a multiple of GR: r0 + k < RT
      float rm[GR], rr[GR], rc[GR];
#pragma unroll
      for (int k = 0; k < GR; ++k) {
        rm[k] = sR[buf][r0 + k][0][lane]; rr[k] = sR[buf][r0 + k][1][lane]; rc[k] = sR[buf][r0 + k][2][lane];
      }
      const int nv = rows - r0;                    // >= 1; rows of the tile past the chunk's end hold zeros and are masked
      if (nv >= GR) {
#pragma unroll
        for (int q = 0; q < QW; ++q) ld_push<true>(sm[q], ss[q], zq[q], rm, rr, rc, GR);
      } else {
#pragma unroll
        for (int q = 0; q < QW; ++q) ld_push<false>(sm[q], ss[q], zq[q], rm, rr, rc, nv);
      }
    }
    if (more) store(buf ^ 1);                      // every wave left buf ^ 1 at the previous barrier
    __syncthreads();
  }
  if (jin) {
#pragma unroll
    for (int q = 0; q < QW; ++q) {
      const int qi = q0 + q;
      if (qi < g.Nq) *(float2*)(g.ws + (((int64_t)qi * g.nchunks + chunk) * g.L + j) * 2) = make_float2(sm[q], ss[q]);
    }
  }
}

__global__ __launch_bounds__(256) void ld_merge_kernel(const LseArgs g) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)g.Nq * g.L) return;
  const int64_t qi = idx / g.L;
  const int j = (int)(idx - qi * g.L);
  double m = -__builtin_inf(), s = 0.0;
  for (int c = 0; c < g.nchunks; ++c) lse_fold_partial(m, s, g.ws + ((qi * g.nchunks + c) * g.L + j) * 2);
  g.lse[qi * g.ldl + j] = m + log(s) - log((double)g.Nr);
}

struct FinArgs {
  const double* lse; const double* own; const float* z; const double* lse_block; double* out;
  int ldl, ldz, N, L;
};

__global__ __launch_bounds__(256) void ld_mean_kernel(const FinArgs g) {
  __shared__ double part[256];
  const int j = blockIdx.x;
  double smi = 0.0, sdw = 0.0, sl = 0.0;
  for (int b = threadIdx.x; b < g.N; b += 256) {
    const double l = g.lse[(int64_t)b * g.ldl + j], o = g.own[(int64_t)b * g.L + j], zz = (double)g.z[(int64_t)b * g.ldz + j];
    smi += o - l;
    sdw += l - (-HALF_LOG_2PI - 0.5 * zz * zz);
    sl += l;
  }
  const double mi = block_sum_ordered(smi, part), dw = block_sum_ordered(sdw, part), ml = block_sum_ordered(sl, part);
  if (threadIdx.x == 0) {
    g.out[j] = mi / (double)g.N; g.out[g.L + j] = dw / (double)g.N; g.out[2 * g.L + j] = ml / (double)g.N;
  }
}

__global__ __launch_bounds__(256) void ld_block_kernel(const FinArgs g) {
  __shared__ double part[256];
  double sb = 0.0;
  for (int b = threadIdx.x; b < g.N; b += 256) sb += g.lse_block[b];
  const double mb = block_sum_ordered(sb, part) / (double)g.N;
  if (threadIdx.x == 0) {
    double sl = 0.0, sd = 0.0;
    for (int j = 0; j < g.L; ++j) { sl += g.out[2 * g.L + j]; sd += g.out[g.L + j]; }
    g.out[3 * g.L] = mb - sl;
    g.out[3 * g.L + 1] = sd;
  }
}

inline int ld_nchunks(int64_t Nr) { return (int)((Nr + LD_CHUNK - 1) / LD_CHUNK); }
inline bool ld_sizes_ok(int32_t Nq, int32_t Nr, int32_t L) { return Nq >= 1 && Nr >= 1 && ld_nchunks(Nr) <= 65535 && L >= 1 && L <= LMAX; }
inline int64_t ld_bytes(int64_t Nq, int64_t Nr, int64_t L) { return up256(Nq * ld_nchunks(Nr) * L * 2 * 4); }

}  // namespace

extern "C" int sv_latent_dims_chunk_rows(void) { return LD_CHUNK; }

extern "C" int sv_latent_dims_workspace_bytes(int32_t Nq, int32_t Nr, int32_t L, int64_t* bytes) {
  if (!bytes) return SV_E_BADARG;
  if (!ld_sizes_ok(Nq, Nr, L)) return SV_E_UNSUPPORTED;
  *bytes = ld_bytes(Nq, Nr, L);
  return SV_OK;
}

extern "C" int sv_latent_dims_prepare(const float* mu, int32_t ldm, const float* sig, int32_t lds, const float* eps, int32_t lde, float* lc,
                                      int32_t ldc, double* own, double* cols, int32_t N, int32_t L, int32_t block, uint64_t seed,
                                      int64_t sample_offset, void* stream) {
  if (!mu || !sig || !lc || !own || !cols) return SV_E_BADARG;
  if (!al(mu, 4) || !al(sig, 4) || !al(eps, 4) || !al(lc, 4) || !al(own, 8) || !al(cols, 8)) return SV_E_BADARG;
  if (N < 1 || L < 1 || L > LMAX || block < 0 || block > 1 || sample_offset < 0) return SV_E_UNSUPPORTED;
  if (ldm < L || lds < L || ldc < L || (eps && lde < L)) return SV_E_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const ElemArgs g = {mu, sig, eps, lc, own, cols, ldm, lds, lde, ldc, N, L, block, seed, sample_offset};
  hipLaunchKernelGGL(ld_elem_kernel, dim3((unsigned)(((int64_t)N * L + 255) / 256)), dim3(256), 0, st, g);
  SV_LAUNCH_CHECK();
  hipLaunchKernelGGL(ld_cols_kernel, dim3(L), dim3(256), 0, st, g);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

extern "C" int sv_latent_dims_lse(const float* z, int32_t ldz, const float* mu, int32_t ldm, const float* rsig, int32_t ldr, const float* lc,
                                  int32_t ldc, int32_t Nq, int32_t Nr, int32_t L, double* lse, int32_t ldl, void* workspace,
                                  int64_t workspace_bytes, void* stream) {
  if (!z || !mu || !rsig || !lc || !lse || !workspace) return SV_E_BADARG;
  if (!al(z, 4) || !al(mu, 4) || !al(rsig, 4) || !al(lc, 4) || !al(lse, 8) || !al(workspace, 16)) return SV_E_BADARG;
  if (!ld_sizes_ok(Nq, Nr, L)) return SV_E_UNSUPPORTED;
  if (ldz < L || ldm < L || ldr < L || ldc < L || ldl < L) return SV_E_UNSUPPORTED;
  if (workspace_bytes < ld_bytes(Nq, Nr, L)) return SV_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const LseArgs g = {z, mu, rsig, lc, (float*)workspace, lse, ldz, ldm, ldr, ldc, ldl, Nq, Nr, L, ld_nchunks(Nr),
                     !(ldm & 3) && al(mu, 16), !(ldr & 3) && al(rsig, 16), !(ldc & 3) && al(lc, 16)};
  hipLaunchKernelGGL(ld_tile_kernel, dim3((Nq + QT - 1) / QT, (L + DT - 1) / DT, g.nchunks), dim3(256), 0, st, g);
  SV_LAUNCH_CHECK();
  hipLaunchKernelGGL(ld_merge_kernel, dim3((unsigned)(((int64_t)Nq * L + 255) / 256)), dim3(256), 0, st, g);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

extern "C" int sv_latent_dims_finish(const double* lse, int32_t ldl, const double* own, const float* z, int32_t ldz, const double* lse_block,
                                     int32_t N, int32_t L, double* out, void* stream) {
  if (!lse || !own || !z || !lse_block || !out) return SV_E_BADARG;
  if (!al(lse, 8) || !al(own, 8) || !al(z, 4) || !al(lse_block, 8) || !al(out, 8)) return SV_E_BADARG;
  if (N < 1 || L < 1 || L > LMAX || ldl < L || ldz < L) return SV_E_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const FinArgs g = {lse, own, z, lse_block, out, ldl, ldz, N, L};
  hipLaunchKernelGGL(ld_mean_kernel, dim3(L), dim3(256), 0, st, g);
  SV_LAUNCH_CHECK();
  hipLaunchKernelGGL(ld_block_kernel, dim3(1), dim3(256), 0, st, g);
  SV_LAUNCH_CHECK();
  return SV_OK;
}
