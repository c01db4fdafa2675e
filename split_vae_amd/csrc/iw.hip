// Importance-weighted test log-likelihood of LGVae (the IW-K bound of Burda et al.): the device code that runs between two
// decoder passes of a K-sample evaluation, and the reduction behind the last one.  The estimator is pinned in
// include/splitvae.h (sv_iw_advance); in short, per image i and sample k
//   z = mu + sig * eps                      written to `zcat` exactly as reparam_kl_fwd_body (pointwise.hip) writes it
//   r = sum_j (eps_j^2 - z_j^2) / 2 + log sig_j       = log p(z) - log q(z | x), over all Lg + Ll dimensions
//   lw_joint = -nll_x - nll_xh + r,  lw_x = -nll_x + r        after the decoder + loss pass over that zcat
// and per image a streamed log-sum-exp (m, s) of each weight plus the running sum of lw_joint, in fp64.
// One wave per image, lanes striding the latent dimensions; lane 0 owns the image's state.  No atomics, nothing depends on
// the launch order: same inputs -> same bits.
#include "eval_common.hip.h"

namespace {

struct IwArgs {
  const float* z_mean[2]; const float* z_sig[2];   // [B,Lg], [B,Ll]
  const float* eps;                                // [B,Lg+Ll] or NULL -> Philox
  void* zcat; int ldz;
  float* r;                                        // [B]
  const float* nll_x; const float* nll_xh;         // [B]
  double* state;                                   // [B,5]: m_joint, s_joint, m_x, s_x, sum lw_joint
  int B, L[2], k, flags;
  uint64_t seed; int64_t sample_offset;
};

template <typename TZ>
__global__ __launch_bounds__(256) void iw_advance_kernel(const IwArgs g) {
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (b >= g.B) return;                            // whole waves leave: the shuffles below see full waves only
  if ((g.flags & SV_IW_ACCUMULATE) && lane == 0) {
    // the pass just finished: sample k - 1, whose r the draw before it left in r[b]
    const double nx = (double)g.nll_x[b], nh = (double)g.nll_xh[b], rr = (double)g.r[b];
    const double lw_j = -nx - nh + rr, lw_x = -nx + rr;
    double* __restrict__ s = g.state + (int64_t)b * 5;
    if (g.k == 1) {                                // first sample: (m, s) = (lw, 1), what the update gives from (-inf, 0)
      s[0] = lw_j; s[1] = 1.0; s[2] = lw_x; s[3] = 1.0; s[4] = lw_j;
    } else {
      double mj = s[0], sj = s[1], mx = s[2], sx = s[3];
      lse_push(mj, sj, lw_j);
      lse_push(mx, sx, lw_x);
      s[0] = mj; s[1] = sj; s[2] = mx; s[3] = sx; s[4] += lw_j;
    }
  }
  if (!(g.flags & SV_IW_DRAW)) return;
  TZ* __restrict__ z_lp = (TZ*)g.zcat;
  Philox ph(g.seed ^ IW_KEY);
  const uint64_t gs = (uint64_t)(g.sample_offset + b);
  const int Lg = g.L[0], Lc = g.L[0] + g.L[1];
  float acc = 0.f;
  for (int jj = lane; jj < Lc; jj += 64) {
    const int e = jj >= Lg, j = e ? jj - Lg : jj, L = g.L[e];
    const float mu = g.z_mean[e][(int64_t)b * L + j];
    const float sg = g.z_sig[e][(int64_t)b * L + j];
    float ep = g.eps ? g.eps[(int64_t)b * Lc + jj] : philox_normal(ph, (uint32_t)j, gs, IW_TAG + (uint32_t)e, (uint32_t)g.k);   // as reparam_kl_fwd_body
    float zz = mu + sg * ep;                       // vae/model.py:13, the expression of reparam_kl_fwd_body
    const TZ zs = from_f32<TZ>(zz);
    z_lp[(int64_t)b * g.ldz + jj] = zs;
    if constexpr (sizeof(TZ) == 2) {               // the weight is evaluated at the latent the decoder consumes
      zz = to_f32(zs);
      ep = (zz - mu) / sg;
    }
    acc += 0.5f * (ep * ep - zz * zz) + logf(sg);
  }
  acc = wave_sum(acc);
  if (lane == 0) g.r[b] = acc;
}

// one workgroup: per-image results, then the batch's sums in image index order
__global__ __launch_bounds__(256) void iw_finish_kernel(const double* __restrict__ state, int K, float* __restrict__ out,
                                                        double* __restrict__ acc, int B) {
  __shared__ double part[3][256];
  const double logK = log((double)K);
  double tot = 0.0;                                // threads 0..2: the running sum of column threadIdx.x
  for (int b0 = 0; b0 < B; b0 += 256) {
    const int b = b0 + threadIdx.x;
    if (b < B) {
      const double* __restrict__ s = state + (int64_t)b * 5;
      const double lj = s[0] + log(s[1]) - logK, lx = s[2] + log(s[3]) - logK, el = s[4] / (double)K;
      out[(int64_t)b * 3 + 0] = (float)lj; out[(int64_t)b * 3 + 1] = (float)lx; out[(int64_t)b * 3 + 2] = (float)el;
      part[0][threadIdx.x] = lj; part[1][threadIdx.x] = lx; part[2][threadIdx.x] = el;
    }
    __syncthreads();
    if (acc && threadIdx.x < 3) {
      const int n = B - b0 < 256 ? B - b0 : 256;
      for (int i = 0; i < n; ++i) tot += part[threadIdx.x][i];
    }
    __syncthreads();
  }
  if (acc) {
    if (threadIdx.x < 3) acc[threadIdx.x] += tot;
    else if (threadIdx.x == 3) acc[3] += (double)B;
  }
}

}  // namespace

extern "C" int sv_iw_advance(const float* z_mean_x, const float* z_sig_x, const float* z_mean_xh, const float* z_sig_xh,
                             const float* eps, void* zcat, int32_t z_dtype, int32_t ldz, float* r, const float* nll_x,
                             const float* nll_xh, double* state, int32_t B, int32_t Lg, int32_t Ll, int32_t k, uint64_t seed,
                             int64_t sample_offset, int32_t flags, void* stream) {
  if (B <= 0 || Lg <= 0 || Ll <= 0 || k < 0 || !r) return SV_E_BADARG;
  if (!flags || (flags & ~(SV_IW_ACCUMULATE | SV_IW_DRAW))) return SV_E_BADARG;
  if (z_dtype != SV_BF16 && z_dtype != SV_F32) return SV_E_BADARG;
  if ((flags & SV_IW_ACCUMULATE) && (!nll_x || !nll_xh || !state || k < 1)) return SV_E_BADARG;
  if ((flags & SV_IW_DRAW) && (!z_mean_x || !z_sig_x || !z_mean_xh || !z_sig_xh || !zcat || ldz < Lg + Ll)) return SV_E_BADARG;
  const IwArgs g = {{z_mean_x, z_mean_xh}, {z_sig_x, z_sig_xh}, eps, zcat, ldz, r, nll_x, nll_xh, state, B, {Lg, Ll}, k, flags,
                    seed, sample_offset};
  dim3 grid((B + 3) / 4), block(256);
  if (z_dtype == SV_BF16) hipLaunchKernelGGL((iw_advance_kernel<bf16_t>), grid, block, 0, (hipStream_t)stream, g);
  else hipLaunchKernelGGL((iw_advance_kernel<float>), grid, block, 0, (hipStream_t)stream, g);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

extern "C" int sv_iw_finish(const double* state, int32_t K, float* out3, double* acc, int32_t B, void* stream) {
  if (!state || !out3 || K <= 0 || B <= 0) return SV_E_BADARG;
  hipLaunchKernelGGL(iw_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, state, K, out3, acc, B);
  SV_LAUNCH_CHECK();
  return SV_OK;
}
