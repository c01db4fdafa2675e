// Importance-weighted test log-likelihood of the mixture models (LGGMVae, GMVae): the device code between two decoder passes of a
// K-sample evaluation, with y marginalised on both sides.  The estimator is pinned in include/splitvae.h (sv_iw_gm_advance); per
// image b and sample k
//   c ~ Cat(softmax(logits[b]))   z_g = zm[b,c] + zs[b,c] * eps_g   z_l = mu_l + sig_l * eps_l       written to `zcat`
//   r = lse_c[-log n + g(z_g; pm[c], ps[c])] - lse_c[log pi_c + g(z_g; zm[b,c], zs[b,c])] + local ratio of z_l
// and the fp64 streamed log-sum-exp of sv_iw_advance (same state, finished by sv_iw_finish).
// One 256-thread workgroup per image.  Wave 0: softmax, cumulated in index order, and the pick.  All threads: the draw (z_g stays
// in LDS; dimensions past GM_ZCAP are read back from zcat).  Densities: thread (c, s) = (t / S, t % S) sums component c over
// d = s, s + S, ...; S = min(64, 256 / pow2ceil(n)) adjacent lanes share a component, so one log2(S)-step xor butterfly finishes all
// 2 n sums together; wave 0 then takes both log-sum-exps over n (two components per lane) in one pass.  No atomics.
#include "eval_common.hip.h"

namespace {

constexpr int GM_NMAX = 128;                       // mixture components
constexpr int GM_ZCAP = 2048;                      // dimensions of z_g kept in LDS (8 KB)

struct IwGmArgs {
  const float* logits; const float* zm_all; const float* zs_all; const float* pm; const float* ps;
  const float* z_mean_l; const float* z_sig_l;
  const float* eps; const int32_t* comp; int32_t* comp_out;
  void* zcat; int ldz;
  float* r; const float* nll_x; const float* nll_xh; double* state;
  int B, n, Lg, Ll, k, flags, lgS;
  uint64_t seed; int64_t sample_offset;
};

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

template <typename TZ>
__global__ __launch_bounds__(256) void iw_gm_advance_kernel(const IwGmArgs g) {
  __shared__ float zsh[GM_ZCAP];
  __shared__ float lpi[GM_NMAX], wp[GM_NMAX], wq[GM_NMAX];
  __shared__ float red[4];
  __shared__ int csh;
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int n = g.n, Lg = g.Lg, Ll = g.Ll;
  if ((g.flags & SV_IW_ACCUMULATE) && t == 0) {
    // the pass just finished: sample k - 1, whose r the draw before it left in r[b]
    const double nx = (double)g.nll_x[b], nh = Ll > 0 ? (double)g.nll_xh[b] : 0.0, rr = (double)g.r[b];
    const double lw_j = -nx - nh + rr, lw_x = -nx + rr;
    double* __restrict__ s = g.state + (int64_t)b * 5;
    if (g.k == 1) {
      s[0] = lw_j; s[1] = 1.0; s[2] = lw_x; s[3] = 1.0; s[4] = lw_j;
    } else {
      double mj = s[0], sj = s[1], mx = s[2], sx = s[3];
      lse_push(mj, sj, lw_j);
      lse_push(mx, sx, lw_x);
      s[0] = mj; s[1] = sj; s[2] = mx; s[3] = sx; s[4] += lw_j;
    }
  }
  if (!(g.flags & SV_IW_DRAW)) return;             // the whole workgroup leaves: the barriers below see all of it
  Philox ph(g.seed ^ IW_KEY);
  const uint64_t gs = (uint64_t)(g.sample_offset + b);

  // ---- 1. softmax of the logits and the component (wave 0; every lane of it carries the same cumulated sums)
  if (wave == 0) {
    const float l0 = lane < n ? g.logits[(int64_t)b * n + lane] : -INFINITY;
    const float l1 = lane + 64 < n ? g.logits[(int64_t)b * n + lane + 64] : -INFINITY;
    const float mx = wave_max(fmaxf(l0, l1));
    const float e0 = lane < n ? expf(l0 - mx) : 0.f, e1 = lane + 64 < n ? expf(l1 - mx) : 0.f;
    float total = 0.f;
    for (int j = 0; j < n; ++j) total += j < 64 ? __shfl(e0, j, 64) : __shfl(e1, j - 64, 64);
    int c;
    if (g.comp) {
      c = g.comp[b];
      c = c < 0 ? 0 : (c >= n ? n - 1 : c);
    } else {
      uint32_t ctr[4] = {0u, (uint32_t)gs, (uint32_t)(gs >> 32) ^ (IW_TAG + 2u), (uint32_t)g.k};
      ph(ctr);
      const float thr = u32_to_unit_open(ctr[0]) * total;
      float cum = 0.f;
      c = n - 1;                                   // the last component catches rounding
      bool found = false;                          // the FIRST index whose cumulated mass reaches thr wins
      for (int j = 0; j < n; ++j) {
        cum += j < 64 ? __shfl(e0, j, 64) : __shfl(e1, j - 64, 64);
        if (!found && cum >= thr) { c = j; found = true; }
      }
    }
    const float lt = logf(total);
    if (lane < n) lpi[lane] = (l0 - mx) - lt;
    if (lane + 64 < n) lpi[lane + 64] = (l1 - mx) - lt;
    if (lane == 0) { csh = c; g.comp_out[b] = c; }
  }
  __syncthreads();
  const int c = csh;

  // ---- 2. the draw: z = mu + sig * eps, the expression of reparam_kl_fwd_body; the local ratio rides along
  TZ* __restrict__ z_lp = (TZ*)g.zcat + (int64_t)b * g.ldz;
  const int Lc = Lg + Ll;
  const float* __restrict__ mu_g = g.zm_all + ((int64_t)b * n + c) * Lg;
  const float* __restrict__ sg_g = g.zs_all + ((int64_t)b * n + c) * Lg;
  float loc = 0.f;
  for (int jj = t; jj < Lc; jj += 256) {
    const int e = jj >= Lg, j = e ? jj - Lg : jj;
    const float mu = e ? g.z_mean_l[(int64_t)b * Ll + j] : mu_g[j];
    const float sg = e ? g.z_sig_l[(int64_t)b * Ll + j] : sg_g[j];
    const float ep = g.eps ? g.eps[(int64_t)b * Lc + jj] : philox_normal(ph, (uint32_t)j, gs, IW_TAG + (uint32_t)e, (uint32_t)g.k);   // as reparam_kl_fwd_body
    const TZ zs = from_f32<TZ>(mu + sg * ep);
    z_lp[jj] = zs;
    const float zz = to_f32(zs);                   // every density below is evaluated at the latent the decoder consumes
    if (!e) {
      if (j < GM_ZCAP) zsh[j] = zz;
    } else {
      const float tt = (zz - mu) / sg;
      loc += 0.5f * (tt * tt - zz * zz) + logf(sg);
    }
  }
  loc = wave_sum(loc);
  if (lane == 0) red[wave] = loc;
  __syncthreads();                                 // zsh, red, and this workgroup's stores to zcat (dimensions >= GM_ZCAP)

  // ---- 3. g(z_g; m, s) of both mixtures: thread (cc, s) over d = s, s + S, ...
  const int S = 1 << g.lgS, cc = t >> g.lgS, s = t & (S - 1);
  const int ck = cc < n ? cc : n - 1;              // idle threads read a valid row and drop the result
  const float* __restrict__ pm = g.pm + (int64_t)ck * Lg;
  const float* __restrict__ ps = g.ps + (int64_t)ck * Lg;
  const float* __restrict__ qm = g.zm_all + ((int64_t)b * n + ck) * Lg;
  const float* __restrict__ qs = g.zs_all + ((int64_t)b * n + ck) * Lg;
  float ap = 0.f, aq = 0.f;
  if (cc < n) {
    for (int d = s; d < Lg; d += S) {
      const float z = d < GM_ZCAP ? zsh[d] : to_f32(z_lp[d]);
      const float sp = ps[d], sq = qs[d];
      const float tp = (z - pm[d]) / sp, tq = (z - qm[d]) / sq;
      ap -= 0.5f * (tp * tp) + logf(sp);
      aq -= 0.5f * (tq * tq) + logf(sq);
    }
  }
  for (int o = S >> 1; o > 0; o >>= 1) {           // S is wave-uniform and divides 64: all 64 lanes take every step
    ap += __shfl_xor(ap, o, 64);
    aq += __shfl_xor(aq, o, 64);
  }
  if (s == 0 && cc < n) {
    wp[cc] = ap - logf((float)n);
    wq[cc] = aq + lpi[cc];
  }
  __syncthreads();

  // ---- 4. both log-sum-exps over the components, maximum subtracted; r
  if (wave == 0) {
    const float p0 = lane < n ? wp[lane] : -INFINITY, p1 = lane + 64 < n ? wp[lane + 64] : -INFINITY;
    const float q0 = lane < n ? wq[lane] : -INFINITY, q1 = lane + 64 < n ? wq[lane + 64] : -INFINITY;
    const float mp = wave_max(fmaxf(p0, p1)), mq = wave_max(fmaxf(q0, q1));
    const float sp = wave_sum((lane < n ? expf(p0 - mp) : 0.f) + (lane + 64 < n ? expf(p1 - mp) : 0.f));
    const float sq = wave_sum((lane < n ? expf(q0 - mq) : 0.f) + (lane + 64 < n ? expf(q1 - mq) : 0.f));
    if (lane == 0) {
      const float lp = mp + logf(sp), lq = mq + logf(sq);
      g.r[b] = (lp - lq) + ((red[0] + red[1]) + (red[2] + red[3]));
    }
  }
}

// ---------------------------------------------------------------- component tables
constexpr int TB_CT = 8;                           // components per workgroup: a weight element is loaded once for 8 rows
constexpr int TB_HMAX = 1024;

__device__ __forceinline__ float elu_f(float v) { return v > 0.f ? v : expm1f(v); }

template <typename TH>
__global__ __launch_bounds__(128) void iw_gm_tables_kernel(const TH* __restrict__ he, const float* __restrict__ w_ht,
                                                           const float* __restrict__ b_ht, const float* __restrict__ w_zm,
                                                           const float* __restrict__ b_zm, const float* __restrict__ w_zs,
                                                           const float* __restrict__ b_zs, const float* __restrict__ w_pm,
                                                           const float* __restrict__ b_pm, const float* __restrict__ w_ps,
                                                           const float* __restrict__ b_ps, float* __restrict__ zm_all,
                                                           float* __restrict__ zs_all, float* __restrict__ pm,
                                                           float* __restrict__ ps, int B, int n, int Hd, int L) {
  __shared__ float hh[TB_CT][TB_HMAX];
  const int b = blockIdx.x, c0 = blockIdx.y * TB_CT, t = threadIdx.x;
  const int nc = n - c0 < TB_CT ? n - c0 : TB_CT;
  if (b == B) {                                    // the extra row of workgroups: the prior tables
    for (int i = t; i < nc * L; i += 128) {
      const int c = c0 + i / L, d = i % L;
      pm[(int64_t)c * L + d] = w_pm[(int64_t)c * L + d] + b_pm[d];
      ps[(int64_t)c * L + d] = softplus_f(w_ps[(int64_t)c * L + d] + b_ps[d]);
    }
    return;
  }
  for (int i = t; i < TB_CT * Hd; i += 128) {
    const int cl = i / Hd, h = i - cl * Hd;
    hh[cl][h] = cl < nc ? to_f32(he[(int64_t)b * Hd + h]) + elu_f(w_ht[(int64_t)(c0 + cl) * Hd + h] + b_ht[h]) : 0.f;
  }
  __syncthreads();
  for (int d = t; d < L; d += 128) {
    float am[TB_CT], as[TB_CT];
#pragma unroll
    for (int cl = 0; cl < TB_CT; ++cl) am[cl] = as[cl] = 0.f;
    for (int h = 0; h < Hd; ++h) {
      const float wm = w_zm[(int64_t)h * L + d], ws = w_zs[(int64_t)h * L + d];
#pragma unroll
      for (int cl = 0; cl < TB_CT; ++cl) {
        am[cl] += hh[cl][h] * wm;
        as[cl] += hh[cl][h] * ws;
      }
    }
    const float bm = b_zm[d], bs = b_zs[d];
#pragma unroll
    for (int cl = 0; cl < TB_CT; ++cl) {
      if (cl < nc) {
        const int64_t o = ((int64_t)b * n + c0 + cl) * L + d;
        zm_all[o] = am[cl] + bm;
        zs_all[o] = softplus_f(as[cl] + bs);
      }
    }
  }
}

}  // namespace

extern "C" int sv_iw_gm_advance(const float* logits, const float* zm_all, const float* zs_all, const float* pm, const float* ps,
                                const float* z_mean_xh, const float* z_sig_xh, const float* eps, const int32_t* comp,
                                int32_t* comp_out, void* zcat, int32_t z_dtype, int32_t ldz, float* r, const float* nll_x,
                                const float* nll_xh, double* state, int32_t B, int32_t n, int32_t Lg, int32_t Ll, int32_t k,
                                uint64_t seed, int64_t sample_offset, int32_t flags, void* stream) {
  if (B <= 0 || Lg <= 0 || Ll < 0 || n < 1 || n > GM_NMAX || k < 0 || !r) return SV_E_BADARG;
  if (!flags || (flags & ~(SV_IW_ACCUMULATE | SV_IW_DRAW))) return SV_E_BADARG;
  if (z_dtype != SV_BF16 && z_dtype != SV_F32) return SV_E_BADARG;
  if ((int64_t)Lg + Ll > INT32_MAX) return SV_E_BADARG;
  if ((flags & SV_IW_ACCUMULATE) && (!nll_x || !state || k < 1 || (Ll > 0 && !nll_xh))) return SV_E_BADARG;
  if (flags & SV_IW_DRAW) {
    if (!logits || !zm_all || !zs_all || !pm || !ps || !zcat || !comp_out || ldz < Lg + Ll) return SV_E_BADARG;
    if (Ll > 0 && (!z_mean_xh || !z_sig_xh)) return SV_E_BADARG;
  }
  int np2 = 1, lgn = 0;
  while (np2 < n) { np2 <<= 1; ++lgn; }
  const int lgS = 8 - lgn < 6 ? 8 - lgn : 6;       // S = min(64, 256 / pow2ceil(n))
  const IwGmArgs g = {logits, zm_all, zs_all, pm, ps, z_mean_xh, z_sig_xh, eps, comp, comp_out, zcat, ldz, r, nll_x, nll_xh, state,
                      B, n, Lg, Ll, k, flags, lgS, seed, sample_offset};
  dim3 grid(B), block(256);
  if (z_dtype == SV_BF16) hipLaunchKernelGGL((iw_gm_advance_kernel<bf16_t>), grid, block, 0, (hipStream_t)stream, g);
  else hipLaunchKernelGGL((iw_gm_advance_kernel<float>), grid, block, 0, (hipStream_t)stream, g);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

extern "C" float sv_iw_gm_uniform_host(uint64_t seed, int64_t image, int32_t sample) {
  const uint64_t gs = (uint64_t)image;
  uint32_t ctr[4] = {0u, (uint32_t)gs, (uint32_t)(gs >> 32) ^ (IW_TAG + 2u), (uint32_t)sample};
  Philox ph(seed ^ IW_KEY);
  ph(ctr);
  return ((float)(ctr[0] >> 8) + 1.0f) * (1.0f / 16777216.0f);     // u32_to_unit_open
}

extern "C" int sv_iw_gm_tables(const void* he, int32_t he_dtype, const float* w_ht, const float* b_ht, const float* w_zm,
                               const float* b_zm, const float* w_zs, const float* b_zs, const float* w_pm, const float* b_pm,
                               const float* w_ps, const float* b_ps, float* zm_all, float* zs_all, float* pm, float* ps, int32_t B,
                               int32_t n, int32_t hidden, int32_t L, void* stream) {
  if (!he || !w_ht || !b_ht || !w_zm || !b_zm || !w_zs || !b_zs || !w_pm || !b_pm || !w_ps || !b_ps || !zm_all || !zs_all || !pm || !ps)
    return SV_E_BADARG;
  if (B <= 0 || L <= 0 || hidden <= 0 || hidden > TB_HMAX || n < 1 || n > GM_NMAX) return SV_E_BADARG;
  if (he_dtype != SV_BF16 && he_dtype != SV_F32) return SV_E_BADARG;
  dim3 grid(B + 1, (n + TB_CT - 1) / TB_CT), block(128);
#define SV_TB_ARGS w_ht, b_ht, w_zm, b_zm, w_zs, b_zs, w_pm, b_pm, w_ps, b_ps, zm_all, zs_all, pm, ps, B, n, hidden, L
  if (he_dtype == SV_BF16)
    hipLaunchKernelGGL((iw_gm_tables_kernel<bf16_t>), grid, block, 0, (hipStream_t)stream, (const bf16_t*)he, SV_TB_ARGS);
  else
    hipLaunchKernelGGL((iw_gm_tables_kernel<float>), grid, block, 0, (hipStream_t)stream, (const float*)he, SV_TB_ARGS);
#undef SV_TB_ARGS
  SV_LAUNCH_CHECK();
  return SV_OK;
}
