// Label-free reconstruction quality of a decode against its image: per-image MSE (for the PSNR) and SSIM with the defaults of
// tf.image.ssim (Wang et al. 2004: 11 x 11 Gaussian window of sigma 1.5 normalised to sum 1, population moments, C1 = 0.01^2,
// C2 = 0.03^2, max_val 1, valid region only, per channel).  The definitions are pinned in include/splitvae.h (sv_recon_draw /
// sv_recon_quality / sv_recon_finish).
//   rq_draw_kernel    one wave per image: the decoders' input zcat = [z_g | z_l], a block kept at its posterior mean or drawn from its
//                     prior (N(0, I), or component c of the mixture prior table: pm[c] + ps[c] * eps), in the plan's dtype
//   rq_tile_kernel    workgroup = (image, band of RQ_TR output rows, tile of up to RQ_TC output columns), as many whole waves as the tile has (column, channel) pairs.  A thread owns one (column,
//                     channel) of the tile's input columns: it loads its RQ_TR + 10 pixels of both images IN PLACE (pixel pitch and
//                     channel offset per image: the six-channel batch and the plan's out6_x are read as they lie), converts them to fp64
//                     and rescales there ((x + 1) * 0.5 is exact in fp64, so is the clip).  Per output row: the five vertical window
//                     sums (a, b, a^2, b^2, a b) from registers, one LDS row [5][columns * 3] (double-buffered: one barrier per row),
//                     then the horizontal window sums of the output columns from LDS, the SSIM value and the thread's running sum.
//                     The moments live in registers and LDS only.  Every sum is fp64: sum(w x^2) - mu^2 cancels to ~1e-15 absolute
//                     against C2 = 9e-4 (a plain fp32 sum leaves 1.3e-6: 1.5e-3 relative in flat regions).  The squared differences
//                     ride along: each pixel is counted by exactly one tile (the last band / column tile owns the 10 trailing rows /
//                     columns).  One (sum of squares, sum of SSIM) pair per tile goes to the workspace.
//   rq_image_kernel   one thread per image adds its tiles' pairs in tile order and divides: per_image [B,2] = (MSE_i, SSIM_i)
//   rq_finish_kernel  one workgroup: PSNR_i = 10 log10(1 / max(MSE_i, 1e-10)) in parallel, then one thread adds (PSNR_i, SSIM_i, 1)
//                     onto acc [3] in image order
// No atomics, outputs overwritten, the workspace may hold anything on entry: the same inputs give the same bits.
#include "eval_common.hip.h"

namespace {

constexpr uint64_t RQ_KEY = 0x1a7e2c0a11f7ULL;     // Philox key constant of this stream (no other kernel of the library uses it)
constexpr uint32_t RQ_TAG = 0x72710000u;           // 'rq' | mode << 4 | stream (0: global latent, 1: local latent, 2: component pick)
constexpr int RQ_WIN = 11, RQ_PAD = RQ_WIN - 1;
constexpr int RQ_TR = 8;                           // output rows per band
constexpr int RQ_TC = 75, RQ_IN = RQ_TC + RQ_PAD;  // output / input columns per tile: 85 * 3 channels = 255 threads
constexpr int LMAX = 512, NMAX = 4096;
constexpr double RQ_C1 = 0.01 * 0.01, RQ_C2 = 0.03 * 0.03, RQ_MSE_FLOOR = 1e-10;

// ---------------------------------------------------------------- sv_recon_draw
struct DrawArgs {
  const float* mg; const float* ml; const float* eps; const int32_t* comp; const float* pm; const float* ps;
  void* zcat;
  int ldg, ldl, lde, ldz, n, mode, B, Lg, Ll;
  uint64_t seed; int64_t sample_offset;
};

template <typename TZ>
__global__ __launch_bounds__(256) void rq_draw_kernel(const DrawArgs g) {
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (b >= g.B) return;                            // whole waves leave
  Philox ph(g.seed ^ RQ_KEY);
  const uint64_t gs = (uint64_t)(g.sample_offset + b);
  const uint32_t tag = RQ_TAG + ((uint32_t)g.mode << 4);
  const int Lg = g.Lg, Lc = g.Lg + g.Ll;
  const bool draw_g = g.mode == SV_RECON_KEEP_L, draw_l = g.mode == SV_RECON_KEEP_G;
  int c = 0;
  if (draw_g && g.pm) {                            // the mixture prior's component: uniform over the n rows of the table
    if (g.comp) {
      c = g.comp[b];
      c = c < 0 ? 0 : (c >= g.n ? g.n - 1 : c);
    } else {
      uint32_t ctr[4] = {0u, (uint32_t)gs, (uint32_t)(gs >> 32) ^ (tag + 2u), 0u};
      ph(ctr);
      c = (int)(((uint64_t)ctr[0] * (uint64_t)g.n) >> 32);
    }
  }
  TZ* __restrict__ z = (TZ*)g.zcat + b * g.ldz;
  for (int jj = lane; jj < Lc; jj += 64) {
    const int e = jj >= Lg, j = e ? jj - Lg : jj;
    float v;
    if (e ? draw_l : draw_g) {
      const float ep = g.eps ? g.eps[b * g.lde + jj] : philox_normal(ph, (uint32_t)j, gs, tag + (uint32_t)e, 0u);   // as sv_iw_advance
      v = ep;
      if (!e && g.pm) v = g.pm[(int64_t)c * Lg + j] + g.ps[(int64_t)c * Lg + j] * ep;
    } else {
      v = e ? g.ml[b * g.ldl + j] : g.mg[b * g.ldg + j];
    }
    z[jj] = from_f32<TZ>(v);
  }
}

// ---------------------------------------------------------------- sv_recon_quality
struct QArgs {
  const float* a; const float* b; double* ws; double* per_image;
  int pa, oa, pb, ob, B, H, W, clip_b, nrb, nct;
  double w[RQ_WIN];
};

inline int rq_nrb(int H) { return (H - RQ_PAD + RQ_TR - 1) / RQ_TR; }
inline int rq_nct(int W) { return (W - RQ_PAD + RQ_TC - 1) / RQ_TC; }
inline int64_t rq_bytes(int64_t B, int H, int W) { return up256(B * rq_nrb(H) * rq_nct(W) * 2 * 8); }
inline bool rq_sizes_ok(int32_t B, int32_t H, int32_t W) {
  return B >= 1 && H >= RQ_WIN && W >= RQ_WIN && H <= 16384 && W <= 16384 && (int64_t)B * rq_nrb(H) * rq_nct(W) <= 0x7fffffffLL;
}

__global__ __launch_bounds__(256) void rq_tile_kernel(const QArgs g) {
  __shared__ double sV[2][5][RQ_IN * 3];           // 20 400 bytes
  __shared__ double sred[2][4];
  const int tid = threadIdx.x, nt = g.nrb * g.nct;
  const int b = blockIdx.x / nt, tile = blockIdx.x - b * nt, rb = tile / g.nct, ct = tile - rb * g.nct;
  const int Ho = g.H - RQ_PAD, Wo = g.W - RQ_PAD;
  const int r0 = rb * RQ_TR, nout = min(RQ_TR, Ho - r0);
  const int x0 = ct * RQ_TC, twin = min(g.W - x0, RQ_IN), two = twin - RQ_PAD;
  const bool last_r = rb == g.nrb - 1, last_c = ct == g.nct - 1;
  const bool act = tid < twin * 3;
  const int x = tid / 3, c = tid - x * 3;
  // ---- this thread's column of both images, rescaled (in fp64: exactly); the squared differences of the pixels this tile owns
  double va[RQ_TR + RQ_PAD], vb[RQ_TR + RQ_PAD];
  double sq = 0.0, ss = 0.0;
  {
    // every lane loads from an address INSIDE the tile (column and row clamped), unconditionally: 36 loads in flight, no branch and no
    // wait between them (a load per `in ? p[..] : fill` is waited for on the spot); what a clamped lane or row holds is never used
    const int64_t pix = ((int64_t)b * g.H + r0) * g.W + x0 + min(x, twin - 1);
    const float* __restrict__ pa = g.a + pix * g.pa + g.oa + c;
    const float* __restrict__ pb = g.b + pix * g.pb + g.ob + c;
    const int64_t rsa = (int64_t)g.W * g.pa, rsb = (int64_t)g.W * g.pb;
    float fa[RQ_TR + RQ_PAD], fb[RQ_TR + RQ_PAD];
#pragma unroll
    for (int j = 0; j < RQ_TR + RQ_PAD; ++j) {
      const int jr = min(j, nout + RQ_PAD - 1);
      fa[j] = pa[jr * rsa];
      fb[j] = pb[jr * rsb];
    }
    const bool own_c = act && (x < two || last_c);
#pragma unroll
    for (int j = 0; j < RQ_TR + RQ_PAD; ++j) {
      va[j] = ((double)fa[j] + 1.0) * 0.5;
      double v = ((double)fb[j] + 1.0) * 0.5;
      if (g.clip_b) v = v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);
      vb[j] = v;
      const double d = va[j] - v;
      if (own_c && (j < nout || (last_r && j < nout + RQ_PAD))) sq += d * d;
    }
  }

  // ---- per output row: vertical sums from registers -> LDS row -> horizontal sums -> SSIM
#pragma unroll
  for (int r = 0; r < RQ_TR; ++r) {
    if (r < nout) {                                // (the same for the whole workgroup)
      if (act) {
        double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < RQ_WIN; ++k) {
          const double a = va[r + k], bb = vb[r + k], wa = g.w[k] * a, wb = g.w[k] * bb;
          m[0] += wa; m[1] += wb;
          m[2] = fma(wa, a, m[2]); m[3] = fma(wb, bb, m[3]); m[4] = fma(wa, bb, m[4]);
        }
#pragma unroll
        for (int q = 0; q < 5; ++q) sV[r & 1][q][tid] = m[q];
      }
      __syncthreads();
      if (tid < two * 3) {
        double h[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < RQ_WIN; ++k) {
#pragma unroll
          for (int q = 0; q < 5; ++q) h[q] = fma(g.w[k], sV[r & 1][q][tid + 3 * k], h[q]);
        }
        const double ma = h[0], mb = h[1];
        const double saa = h[2] - ma * ma, sbb = h[3] - mb * mb, sab = h[4] - ma * mb;
        ss += ((2.0 * ma * mb + RQ_C1) * (2.0 * sab + RQ_C2)) / ((ma * ma + mb * mb + RQ_C1) * (saa + sbb + RQ_C2));
      }
      // no second barrier: row r + 1 writes the other buffer, and row r + 2 writes this one behind the barrier of row r + 1
    }
  }

  // ---- the tile's pair: 64-lane butterflies, then the waves in wave order
  sq = wave_sum_f64(sq); ss = wave_sum_f64(ss);
  if ((tid & 63) == 0) { sred[0][tid >> 6] = sq; sred[1][tid >> 6] = ss; }
  __syncthreads();
  if (tid < 2) {
    double t = 0.0;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += sred[tid][i];
    g.ws[(int64_t)blockIdx.x * 2 + tid] = t;
  }
}

__global__ __launch_bounds__(256) void rq_image_kernel(const QArgs g) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= g.B) return;
  const int nt = g.nrb * g.nct;
  double sq = 0.0, ss = 0.0;
  for (int t = 0; t < nt; ++t) { sq += g.ws[(b * nt + t) * 2]; ss += g.ws[(b * nt + t) * 2 + 1]; }
  g.per_image[b * 2] = sq / ((double)g.H * (double)g.W * 3.0);
  g.per_image[b * 2 + 1] = ss / ((double)(g.H - RQ_PAD) * (double)(g.W - RQ_PAD) * 3.0);
}

// ---------------------------------------------------------------- sv_recon_finish
__global__ __launch_bounds__(256) void rq_finish_kernel(const double* __restrict__ per_image, int B, double* __restrict__ acc) {
  __shared__ double sp[256];
  double a0 = 0.0, a1 = 0.0;
  if (threadIdx.x == 0) { a0 = acc[0]; a1 = acc[1]; }
  for (int b0 = 0; b0 < B; b0 += 256) {
    const int b = b0 + threadIdx.x;
    if (b < B) sp[threadIdx.x] = 10.0 * log10(1.0 / fmax(per_image[(int64_t)b * 2], RQ_MSE_FLOOR));
    __syncthreads();
    if (threadIdx.x == 0) {
      const int n = min(256, B - b0);
      for (int i = 0; i < n; ++i) { a0 += sp[i]; a1 += per_image[(int64_t)(b0 + i) * 2 + 1]; }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) { acc[0] = a0; acc[1] = a1; acc[2] += (double)B; }
}

}  // namespace

extern "C" int sv_recon_draw(const float* z_mean_x, int32_t ldg, const float* z_mean_xh, int32_t ldl, int32_t mode, const float* eps,
                             int32_t lde, const int32_t* comp, const float* pm, const float* ps, int32_t n, void* zcat, int32_t ldz,
                             int32_t dtype, int32_t B, int32_t Lg, int32_t Ll, uint64_t seed, int64_t sample_offset, void* stream) {
  if (!z_mean_x || !zcat || (Ll > 0 && !z_mean_xh) || (!pm != !ps)) return SV_E_BADARG;
  if (!al(z_mean_x, 4) || !al(z_mean_xh, 4) || !al(eps, 4) || !al(comp, 4) || !al(pm, 4) || !al(ps, 4) || !al(zcat, dtype == SV_F32 ? 4 : 2))
    return SV_E_BADARG;
  if (dtype != SV_F32 && dtype != SV_BF16) return SV_E_UNSUPPORTED;
  if (mode != SV_RECON_MEANS && mode != SV_RECON_KEEP_G && mode != SV_RECON_KEEP_L) return SV_E_UNSUPPORTED;
  if (B < 1 || Lg < 1 || Lg > LMAX || Ll < 0 || Ll > LMAX || sample_offset < 0) return SV_E_UNSUPPORTED;
  const int Lc = Lg + Ll;
  if (ldg < Lg || (Ll > 0 && ldl < Ll) || ldz < Lc || (eps && lde < Lc)) return SV_E_UNSUPPORTED;
  if (pm && (n < 1 || n > NMAX)) return SV_E_UNSUPPORTED;
  const DrawArgs g = {z_mean_x, z_mean_xh, eps, comp, pm, ps, zcat, ldg, ldl, lde, ldz, n, mode, B, Lg, Ll, seed, sample_offset};
  const dim3 grid((B + 3) / 4);
  if (dtype == SV_F32) hipLaunchKernelGGL(rq_draw_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, g);
  else hipLaunchKernelGGL(rq_draw_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, g);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

extern "C" int sv_recon_quality_workspace_bytes(int32_t B, int32_t H, int32_t W, int64_t* bytes) {
  if (!bytes) return SV_E_BADARG;
  if (!rq_sizes_ok(B, H, W)) return SV_E_UNSUPPORTED;
  *bytes = rq_bytes(B, H, W);
  return SV_OK;
}

extern "C" void sv_recon_window(double* w /* [11] */) {
  double s = 0.0;
  for (int i = 0; i < RQ_WIN; ++i) { const double d = (double)(i - RQ_WIN / 2); w[i] = exp(-d * d / (2.0 * 1.5 * 1.5)); s += w[i]; }
  for (int i = 0; i < RQ_WIN; ++i) w[i] /= s;
}

extern "C" int sv_recon_quality(const float* a, int32_t pitch_a, int32_t off_a, const float* b, int32_t pitch_b, int32_t off_b,
                                int32_t clip_b, int32_t B, int32_t H, int32_t W, double* per_image, void* workspace,
                                int64_t workspace_bytes, void* stream) {
  if (!a || !b || !per_image || !workspace) return SV_E_BADARG;
  if (!al(a, 4) || !al(b, 4) || !al(per_image, 8) || !al(workspace, 8)) return SV_E_BADARG;
  if (!rq_sizes_ok(B, H, W)) return SV_E_UNSUPPORTED;
  if (off_a < 0 || off_b < 0 || pitch_a < off_a + 3 || pitch_b < off_b + 3 || pitch_a > 4096 || pitch_b > 4096) return SV_E_UNSUPPORTED;
  if (workspace_bytes < rq_bytes(B, H, W)) return SV_E_WORKSPACE;
  QArgs g = {a, b, (double*)workspace, per_image, pitch_a, off_a, pitch_b, off_b, B, H, W, clip_b != 0, rq_nrb(H), rq_nct(W), {}};
  sv_recon_window(g.w);
  hipStream_t st = (hipStream_t)stream;
  const int threads = ((W < RQ_IN ? W : RQ_IN) * 3 + 63) / 64 * 64;      // whole waves over the widest tile's (column, channel) pairs
  hipLaunchKernelGGL(rq_tile_kernel, dim3((unsigned)(B * g.nrb * g.nct)), dim3(threads), 0, st, g);
  SV_LAUNCH_CHECK();
  hipLaunchKernelGGL(rq_image_kernel, dim3((B + 255) / 256), dim3(256), 0, st, g);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

extern "C" int sv_recon_finish(const double* per_image, int32_t B, double* acc, void* stream) {
  if (!per_image || !acc) return SV_E_BADARG;
  if (!al(per_image, 8) || !al(acc, 8)) return SV_E_BADARG;
  if (B < 1) return SV_E_UNSUPPORTED;
  hipLaunchKernelGGL(rq_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, per_image, B, acc);
  SV_LAUNCH_CHECK();
  return SV_OK;
}
