// Aggregate-posterior information report of the latents (Hoffman & Johnson's "ELBO surgery": average KL = index-code mutual
// information + marginal KL), plus the mutual information of the two latent blocks under the aggregate posterior.  Every sample
// z_i is scored under every image's posterior q(z | x_j); the Nq x Nr score matrix never exists in memory.  The definitions are
// pinned in include/splitvae.h (sv_latent_info_draw / _lse / _finish).
//   li_draw_kernel    one wave per image: z = mu + sig * eps, 1 / sig, the row constants c = -sum log sig - L/2 log 2 pi, the own
//                     and prior terms (block sums in fp64, lanes striding the dimensions, then the 64-lane butterfly)
//   li_tile_kernel    workgroup = (64-query tile, chunk of LI_CHUNK references).  The pair score is computed in its DIRECT form
//                     ((z - mu) * rsig)^2 on the vector ALU: only non-negative terms, so its error is relative to the score (the
//                     expanded z^2.a - 2 z.b + c cancels ~1e5 against ~1e5 at sig ~ 1e-2).  A lane owns one reference row of a
//                     64-row pass: its (mu, rsig) pairs stream by dimension from LDS as one ds_read_b64 per dimension (lane l
//                     reads dwords 2 l, 2 l + 1 of a 128-dword row: conflict-free).  A wave owns 16 queries; their z are
//                     broadcast from LDS ([dimension][16 queries]: four ds_read_b128 of one address per dimension) and go
//                     through the packed fp32 VALU two queries at a time (v_pk_add / v_pk_mul / v_pk_fma).  Per query each lane
//                     keeps a private streaming (max, sum) of the three sums (g, l, g + l); ONE 64-lane butterfly at the end of
//                     the chunk leaves a (max, sum) per (query, chunk, sum) in the workspace.
//   li_merge_kernel   one thread per query folds the chunk partials in chunk order, in fp64: lse = m + log(S) - log Nr
//   li_finish_kernel  one workgroup: the fp64 means, summed in one fixed order
// No atomics; the partial of (query, chunk) depends on the query row and the chunk's rows only: same inputs -> same bits, wherever
// the query sits.
#include "eval_common.hip.h"

namespace {

constexpr int LI_CHUNK = 1024;                     // reference rows per chunk (sv_latent_info_chunk_rows)
constexpr int QT = 64, QW = 16, RT = 64, DK = 32;  // queries per workgroup / per wave, references per pass, dimensions per step
constexpr int LMAX = 512;

struct DrawArgs {
  const float* mu; const float* sig; const float* eps;
  float* z; float* rsig; float* cst; double* own; double* prior;
  int ldm, lds, lde, ldz, ldr, N, Lg, Ll;
  uint64_t seed; int64_t sample_offset;
};

__global__ __launch_bounds__(256) void li_draw_kernel(const DrawArgs g) {
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (b >= g.N) return;                            // whole waves leave
  const Philox ph = latent_info_stream(g.seed);
  const uint64_t gs = (uint64_t)(g.sample_offset + b);
  const int Lg = g.Lg, Lc = g.Lg + g.Ll;
  double slog[2] = {0.0, 0.0}, seps[2] = {0.0, 0.0}, sz[2] = {0.0, 0.0};
  for (int jj = lane; jj < Lc; jj += 64) {
    const int e = jj >= Lg, j = e ? jj - Lg : jj;
    const float mu = g.mu[b * g.ldm + jj];
    const float sg = g.sig[b * g.lds + jj];
    const float ep = g.eps ? g.eps[b * g.lde + jj] : LATENT_INFO_EPS(ph, gs, e, j);
    const float zz = mu + sg * ep;
    g.z[b * g.ldz + jj] = zz;
    g.rsig[b * g.ldr + jj] = 1.f / sg;
    slog[e] += (double)logf(sg);
    seps[e] += (double)ep * (double)ep;
    sz[e] += (double)zz * (double)zz;
  }
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    slog[e] = wave_sum_f64(slog[e]); seps[e] = wave_sum_f64(seps[e]); sz[e] = wave_sum_f64(sz[e]);
  }
  if (lane < 2) {
    const int e = lane;
    const double L = e ? (double)g.Ll : (double)g.Lg;
    const double c = -(e ? slog[1] : slog[0]) - L * HALF_LOG_2PI;
    g.cst[b * 2 + e] = (float)c;
    g.own[b * 2 + e] = c - 0.5 * (e ? seps[1] : seps[0]);
    g.prior[b * 2 + e] = -L * HALF_LOG_2PI - 0.5 * (e ? sz[1] : sz[0]);
  }
}

struct LseArgs {
  const float* z; const float* mu; const float* rsig; const float* cst;
  float* ws;                                       // [Nq][nchunks][3][2]: (max, sum) of g, l, g + l
  double* lse;                                     // [3][Nq]
  int ldz, ldm, ldr, Nq, Nr, Lg, Ll, nchunks, vecz, vecm, vecr;
};

// 8 floats of row `row` from column `col` (lim of them exist); rows past `rows` and columns past lim read as `fill`
__device__ __forceinline__ void li_load(const float* __restrict__ P, int ld, int row, int rows, int col, int lim, bool vec, float fill,
                                        float (&r)[8]) {
  const bool any = row < rows;
  const float* p = P + (int64_t)row * ld + col;
  if (any && vec && lim >= 8) {
    const float4 a = *(const float4*)p, b = *(const float4*)(p + 4);
    r[0] = a.x; r[1] = a.y; r[2] = a.z; r[3] = a.w; r[4] = b.x; r[5] = b.y; r[6] = b.z; r[7] = b.w;
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) r[i] = (any && i < lim) ? p[i] : fill;
  }
}

// (m, s) <- (m, s) + exp(e): one v_exp_f32; m = -inf, s = 0 is the empty state
__device__ __forceinline__ void li_push(float& m, float& s, const float e) {
  const float d = e - m;
  const float x = __builtin_amdgcn_exp2f(-fabsf(d) * LOG2E);
  const bool up = d > 0.f;
  s = up ? __builtin_fmaf(s, x, 1.f) : s + x;
  m = up ? e : m;
}
// (m, s) <- (m, s) + (m2, s2); either may be empty
__device__ __forceinline__ void li_merge(float& m, float& s, const float m2, const float s2) {
  const float mn = fmaxf(m, m2);
  const float a = m == mn ? 1.f : __builtin_amdgcn_exp2f((m - mn) * LOG2E);       // (-inf) - (-inf) never evaluated
  const float b = m2 == mn ? 1.f : __builtin_amdgcn_exp2f((m2 - mn) * LOG2E);
  s = s * a + s2 * b;
  m = mn;
}

template <bool SPLIT>
__global__ __launch_bounds__(256) void li_tile_kernel(const LseArgs g) {
  __shared__ __attribute__((aligned(16))) float sR[2][DK * RT * 2];                // [dimension][reference lane] (mu, rsig)
  __shared__ __attribute__((aligned(16))) float sZ[2][4 * DK * QW];                // [wave][dimension][query of the wave]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q0 = blockIdx.x * QT, chunk = blockIdx.y;
  const int c0 = chunk * LI_CHUNK, c1 = min(g.Nr, c0 + LI_CHUNK);
  const int ng = (g.Lg + DK - 1) / DK, nl = SPLIT ? (g.Ll + DK - 1) / DK : 0, nsteps = ng + nl;
  constexpr int NS = SPLIT ? 3 : 1;
  float sm[NS][QW], ss[NS][QW];
#pragma unroll
  for (int t = 0; t < NS; ++t)
#pragma unroll
    for (int q = 0; q < QW; ++q) { sm[t][q] = -__builtin_inff(); ss[t][q] = 0.f; }
  // staging roles: references -- row tid & 63, 8 dimensions from (tid >> 6) * 8; queries -- row tid >> 2, 8 dimensions from (tid & 3) * 8
  const int rrow = tid & 63, rk = (tid >> 6) * 8, zrow = tid >> 2, zk = (tid & 3) * 8;
  float rm[8], rr[8], rz[8];
  auto load = [&](int n0, int step) {
    const int e = step >= ng, k0 = (e ? step - ng : step) * DK, L = e ? g.Ll : g.Lg, col = (e ? g.Lg : 0) + k0;
    const bool al4 = !(col & 3);
    li_load(g.mu, g.ldm, n0 + rrow, c1, col + rk, L - k0 - rk, g.vecm && al4, 0.f, rm);
    li_load(g.rsig, g.ldr, n0 + rrow, c1, col + rk, L - k0 - rk, g.vecr && al4, 0.f, rr);
    li_load(g.z, g.ldz, q0 + zrow, g.Nq, col + zk, L - k0 - zk, g.vecz && al4, 0.f, rz);
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      *(float2*)&sR[buf][((rk + i) * RT + rrow) * 2] = make_float2(rm[i], rr[i]);
      sZ[buf][((zrow >> 4) * DK + zk + i) * QW + (zrow & 15)] = rz[i];
    }
  };
  for (int n0 = c0; n0 < c1; n0 += RT) {
    const bool valid = n0 + lane < c1;
    float cg = 0.f, cl = 0.f;
    if (valid) {
      cg = g.cst[(int64_t)(n0 + lane) * 2];
      if (SPLIT) cl = g.cst[(int64_t)(n0 + lane) * 2 + 1];
    }
    f32x2 acc[QW / 2];
    float eg[QW];
#pragma unroll
    for (int p = 0; p < QW / 2; ++p) acc[p] = (f32x2){0.f, 0.f};
    load(n0, 0);
    store(0);                                      // (the previous pass ended with a barrier: every wave is done with both buffers)
    __syncthreads();
    for (int step = 0; step < nsteps; ++step) {
      const int buf = step & 1;
      const bool more = step + 1 < nsteps;
      if (more) load(n0, step + 1);
      const float* cR = sR[buf] + lane * 2;
      const float* cZ = sZ[buf] + wave * DK * QW;
      // software pipeline: the LDS reads of dimension kk + 1 are in flight while dimension kk goes through the VALU
      float2 mr = *(const float2*)cR;
      f32x4 zc[QW / 4];
#pragma unroll
      for (int v = 0; v < QW / 4; ++v) zc[v] = ((const f32x4*)cZ)[v];
#pragma unroll
      for (int kk = 0; kk < DK; ++kk) {
        float2 mrn = mr;
        f32x4 zn[QW / 4];
        if (kk + 1 < DK) {
          mrn = *(const float2*)(cR + (kk + 1) * RT * 2);
#pragma unroll
          for (int v = 0; v < QW / 4; ++v) zn[v] = ((const f32x4*)(cZ + (kk + 1) * QW))[v];
        }
        const f32x2 m2 = (f32x2){mr.x, mr.x}, r2 = (f32x2){mr.y, mr.y};
#pragma unroll
        for (int v = 0; v < QW / 4; ++v) {
          const f32x4 zz = zc[v];
          const f32x2 u0 = ((f32x2){zz[0], zz[1]} - m2) * r2, u1 = ((f32x2){zz[2], zz[3]} - m2) * r2;
          acc[2 * v] = __builtin_elementwise_fma(u0, u0, acc[2 * v]);
          acc[2 * v + 1] = __builtin_elementwise_fma(u1, u1, acc[2 * v + 1]);
        }
        if (kk + 1 < DK) {
          mr = mrn;
#pragma unroll
          for (int v = 0; v < QW / 4; ++v) zc[v] = zn[v];
        }
      }
      if (step == ng - 1) {                        // the global block is complete
#pragma unroll
        for (int q = 0; q < QW; ++q) {
          eg[q] = cg - 0.5f * acc[q >> 1][q & 1];
          if (valid && eg[q] > -3.0e38f) li_push(sm[0][q], ss[0][q], eg[q]);
        }
#pragma unroll
        for (int p = 0; p < QW / 2; ++p) acc[p] = (f32x2){0.f, 0.f};
      }
      if constexpr (SPLIT) if (step == nsteps - 1) {
#pragma unroll
        for (int q = 0; q < QW; ++q) {
          const float el = cl - 0.5f * acc[q >> 1][q & 1];
          const float egl = eg[q] + el;
          if (valid && el > -3.0e38f) li_push(sm[NS - 2][q], ss[NS - 2][q], el);
          if (valid && egl > -3.0e38f) li_push(sm[NS - 1][q], ss[NS - 1][q], egl);
        }
      }
      if (more) store(buf ^ 1);
      __syncthreads();
    }
  }
  // one butterfly per (query, sum); lane 0 writes the chunk's partial
#pragma unroll
  for (int t = 0; t < NS; ++t)
#pragma unroll
    for (int q = 0; q < QW; ++q) {
      float m = sm[t][q], s = ss[t][q];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
        li_merge(m, s, m2, s2);
      }
      const int qi = q0 + wave * QW + q;
      if (lane == 0 && qi < g.Nq) {
        float* w = g.ws + (((int64_t)qi * g.nchunks + chunk) * 3 + t) * 2;
        w[0] = m; w[1] = s;
      }
    }
}

__global__ __launch_bounds__(256) void li_merge_kernel(const LseArgs g) {
  const int64_t qi = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (qi >= g.Nq) return;
  const int ns = g.Ll > 0 ? 3 : 1;
  const double logN = log((double)g.Nr);
  for (int t = 0; t < ns; ++t) {
    double m = -__builtin_inf(), s = 0.0;
    for (int c = 0; c < g.nchunks; ++c) lse_fold_partial(m, s, g.ws + ((qi * g.nchunks + c) * 3 + t) * 2);
    g.lse[(int64_t)t * g.Nq + qi] = m + log(s) - logN;
  }
}

// out[8] = KL_g, MI_g, marginal KL_g, KL_l, MI_l, marginal KL_l, overlap, log N.  One workgroup, one fixed order: thread t sums the images
// t, t + 256, ... in ascending order, then thread c adds the 256 partial sums of column c in thread order
__global__ __launch_bounds__(256) void li_finish_kernel(const double* __restrict__ own, const double* __restrict__ prior,
                                                        const double* __restrict__ lse, int N, int Ll, double* __restrict__ out) {
  __shared__ double part[7][256];
  const int nc = Ll > 0 ? 7 : 3;
  double acc[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int b = threadIdx.x; b < N; b += 256) {
    const double og = own[(int64_t)b * 2], pg = prior[(int64_t)b * 2], lg = lse[b];
    acc[0] += og - pg; acc[1] += og - lg; acc[2] += lg - pg;
    if (Ll > 0) {
      const double ol = own[(int64_t)b * 2 + 1], pl = prior[(int64_t)b * 2 + 1], ll = lse[(int64_t)N + b], lgl = lse[2 * (int64_t)N + b];
      acc[3] += ol - pl; acc[4] += ol - ll; acc[5] += ll - pl; acc[6] += lgl - lg - ll;
    }
  }
#pragma unroll
  for (int c = 0; c < 7; ++c) part[c][threadIdx.x] = acc[c];
  __syncthreads();
  if (threadIdx.x < 7) {
    double tot = 0.0;
    if (threadIdx.x < nc)
      for (int i = 0; i < 256; ++i) tot += part[threadIdx.x][i];
    out[threadIdx.x] = tot / (double)N;
  } else if (threadIdx.x == 7) {
    out[7] = log((double)N);
  }
}

inline int li_nchunks(int64_t Nr) { return (int)((Nr + LI_CHUNK - 1) / LI_CHUNK); }
inline bool li_sizes_ok(int32_t Nq, int32_t Nr) { return Nq >= 1 && Nr >= 1 && li_nchunks(Nr) <= 65535; }
inline bool li_widths_ok(int32_t Lg, int32_t Ll) { return Lg >= 1 && Lg <= LMAX && Ll >= 0 && Ll <= LMAX; }
inline int64_t li_bytes(int64_t Nq, int64_t Nr) { return up256(Nq * li_nchunks(Nr) * 3 * 2 * 4); }

}  // namespace

extern "C" int sv_latent_info_chunk_rows(void) { return LI_CHUNK; }

extern "C" int sv_latent_info_workspace_bytes(int32_t Nq, int32_t Nr, int64_t* bytes) {
  if (!bytes) return SV_E_BADARG;
  if (!li_sizes_ok(Nq, Nr)) return SV_E_UNSUPPORTED;
  *bytes = li_bytes(Nq, Nr);
  return SV_OK;
}

extern "C" int sv_latent_info_draw(const float* mu, int32_t ldm, const float* sig, int32_t lds, const float* eps, int32_t lde, float* z,
                                   int32_t ldz, float* rsig, int32_t ldr, float* cst, double* own, double* prior, int32_t N,
                                   int32_t Lg, int32_t Ll, uint64_t seed, int64_t sample_offset, void* stream) {
  if (!mu || !sig || !z || !rsig || !cst || !own || !prior) return SV_E_BADARG;
  if (!al(mu, 4) || !al(sig, 4) || !al(eps, 4) || !al(z, 4) || !al(rsig, 4) || !al(cst, 4) || !al(own, 8) || !al(prior, 8)) return SV_E_BADARG;
  if (N < 1 || !li_widths_ok(Lg, Ll) || sample_offset < 0) return SV_E_UNSUPPORTED;
  const int Lc = Lg + Ll;
  if (ldm < Lc || lds < Lc || ldz < Lc || ldr < Lc || (eps && lde < Lc)) return SV_E_UNSUPPORTED;
  const DrawArgs g = {mu, sig, eps, z, rsig, cst, own, prior, ldm, lds, lde, ldz, ldr, N, Lg, Ll, seed, sample_offset};
  hipLaunchKernelGGL(li_draw_kernel, dim3((N + 3) / 4), dim3(256), 0, (hipStream_t)stream, g);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

extern "C" int sv_latent_info_lse(const float* z, int32_t ldz, const float* mu, int32_t ldm, const float* rsig, int32_t ldr, const float* cst,
                                  int32_t Nq, int32_t Nr, int32_t Lg, int32_t Ll, double* lse, void* workspace, int64_t workspace_bytes,
                                  void* stream) {
  if (!z || !mu || !rsig || !cst || !lse || !workspace) return SV_E_BADARG;
  if (!al(z, 4) || !al(mu, 4) || !al(rsig, 4) || !al(cst, 4) || !al(lse, 8) || !al(workspace, 16)) return SV_E_BADARG;
  if (!li_sizes_ok(Nq, Nr) || !li_widths_ok(Lg, Ll)) return SV_E_UNSUPPORTED;
  const int Lc = Lg + Ll;
  if (ldz < Lc || ldm < Lc || ldr < Lc) return SV_E_UNSUPPORTED;
  if (workspace_bytes < li_bytes(Nq, Nr)) return SV_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const LseArgs g = {z, mu, rsig, cst, (float*)workspace, lse, ldz, ldm, ldr, Nq, Nr, Lg, Ll, li_nchunks(Nr),
                     !(ldz & 3) && al(z, 16), !(ldm & 3) && al(mu, 16), !(ldr & 3) && al(rsig, 16)};
  const dim3 grid((Nq + QT - 1) / QT, g.nchunks);
  if (Ll > 0) hipLaunchKernelGGL(li_tile_kernel<true>, grid, dim3(256), 0, st, g);
  else hipLaunchKernelGGL(li_tile_kernel<false>, grid, dim3(256), 0, st, g);
  SV_LAUNCH_CHECK();
  hipLaunchKernelGGL(li_merge_kernel, dim3((Nq + 255) / 256), dim3(256), 0, st, g);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

extern "C" int sv_latent_info_finish(const double* own, const double* prior, const double* lse, int32_t N, int32_t Ll, double* out,
                                     void* stream) {
  if (!own || !prior || !lse || !out) return SV_E_BADARG;
  if (!al(own, 8) || !al(prior, 8) || !al(lse, 8) || !al(out, 8)) return SV_E_BADARG;
  if (N < 1 || Ll < 0 || Ll > LMAX) return SV_E_UNSUPPORTED;
  hipLaunchKernelGGL(li_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, own, prior, lse, N, Ll, out);
  SV_LAUNCH_CHECK();
  return SV_OK;
}
