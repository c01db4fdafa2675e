// The augmentations of augmentation.py:33-38,59-101 besides `scramble` (pointwise.hip): the Gaussian filter behind `blur` and
// `high_low_pass`, the Philox draws of the per-image blur parameters and patch sizes, and the mixed-size scramble.
// Plain C++ loads and stores only; every sum runs in one fixed order (bit-reproducible).
#include "common.hip.h"
#include "kernels.h"

// ============================================================================ A1b Gaussian filter
// augmentation.py:83-101.  low = depthwise_conv2d(pad(x, r, SYMMETRIC), K) with K = outer(v, v) / sum(outer(v, v)),
// v = Normal(mean, std).prob(range(-r, r+1)) (augmentation.py:33-38), VALID, the pointwise filter eye(3) an identity.
// K is separable: K[i][j] = w[i] w[j], w = v / sum(v), so the filter runs as a row pass then a column pass.
// TF's conv is a cross-correlation: low[y][x] = sum_{a,b} w[a] w[b] xpad[y+a][x+b], tap a at offset a - r.
// SYMMETRIC padding mirrors including the edge pixel: -1 -> 0, H -> H-1 (numpy mode='symmetric').
//
// One workgroup per (row band, image).  The band's BR rows plus an RMAX-row mirrored halo above and below are staged in LDS
// (xs), the row pass writes hs beside it, the column pass reads hs and writes the output pixel by pixel: x | low (NOUT 6) or
// x | x - low | low (NOUT 9), and with STAGED the zero-padded 8-channel copies of channels 0-2 and 3-5 in T
// (the contract of sv_scramble_gather_staged).
constexpr int GAUSS_MAX_RADIUS = 64;
constexpr int GAUSS_MAX_LDS = 64 * 1024;
constexpr int GAUSS_MAX_BATCH = 65535;   // the image index is blockIdx.y

__device__ __forceinline__ int sym_index(int i, int n) {   // valid for -n <= i < 2n
  return i < 0 ? -i - 1 : (i >= n ? 2 * n - 1 - i : i);
}

// w[0..2r] = v / sum(v) in fp32; v[k] = Normal(mean, std).prob(k - r) formed as exp(log_prob) the way tfp does
// (log_prob = -0.5 z^2 - (log(std) + 0.5 log(2 pi))).  Sum in index order.  Run by one thread.
__device__ void gauss_taps(float* w, int r, float mean, float std) {
  const float log_norm = logf(std) + 0.91893853320467274178f;
  float s = 0.f;
  for (int k = 0; k <= 2 * r; ++k) {
    const float z = ((float)(k - r) - mean) / std;
    const float v = expf(-0.5f * z * z - log_norm);
    w[k] = v;
    s += v;
  }
  for (int k = 0; k <= 2 * r; ++k) w[k] = w[k] / s;
}

template <typename T, int NOUT, bool STAGED>
__global__ __launch_bounds__(256) void gauss_filter_kernel(const float* __restrict__ x, const int32_t* __restrict__ radius,
                                                           const float* __restrict__ stdv, int fixed_r, float mean, float fixed_std,
                                                           float* __restrict__ out, T* __restrict__ x8, T* __restrict__ xh8,
                                                           int H, int W, int BR, int RMAX) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  __shared__ float wts[2 * GAUSS_MAX_RADIUS + 1];
  const int rows = BR + 2 * RMAX;
  const int rowf = W * 3;
  float* xs = (float*)smem_raw;          // [rows][W][3] input rows y0-RMAX .. y0+BR+RMAX-1 (mirrored)
  float* hs = xs + rows * rowf;          // [rows][W][3] after the row pass
  const int b = blockIdx.y;
  const int y0 = blockIdx.x * BR;
  const int nr = min(BR, H - y0);        // output rows of this band
  int r = fixed_r;
  float sd = fixed_std;
  if (radius) {
    r = min(max(radius[b], 0), RMAX);    // the host bounded RMAX by H and the LDS: a radius beyond it is clamped
    sd = stdv[b];
  }
  if (threadIdx.x == 0) gauss_taps(wts, r, mean, sd);
  // stage the rows this band needs (rows outside [y0-r, y0+nr+r) are not read)
  const float* xb = x + (int64_t)b * H * rowf;
  const int g0 = y0 - r, g1 = y0 + nr + r;
  const int soff = RMAX - r;             // LDS row of global row g0
  const int nstage = g1 - g0;
  if ((rowf & 3) == 0 && ((uintptr_t)x & 15) == 0) {
    const int q = rowf >> 2;
    for (int e = threadIdx.x; e < nstage * q; e += blockDim.x) {
      const int i = e / q, c = e - i * q;
      const int g = sym_index(g0 + i, H);
      *(float4*)(xs + (soff + i) * rowf + 4 * c) = *(const float4*)(xb + (int64_t)g * rowf + 4 * c);
    }
  } else {
    for (int e = threadIdx.x; e < nstage * rowf; e += blockDim.x) {
      const int i = e / rowf, c = e - i * rowf;
      const int g = sym_index(g0 + i, H);
      xs[(soff + i) * rowf + c] = xb[(int64_t)g * rowf + c];
    }
  }
  __syncthreads();
  // row pass: hs[i][px][c] = sum_b w[b] xs[i][sym(px + b - r)][c], b ascending
  for (int e = threadIdx.x; e < nstage * W; e += blockDim.x) {
    const int i = e / W, px = e - i * W;
    const float* xr = xs + (soff + i) * rowf;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int k = 0; k <= 2 * r; ++k) {
      const float wk = wts[k];
      const float* p = xr + sym_index(px + k - r, W) * 3;
      a0 += wk * p[0]; a1 += wk * p[1]; a2 += wk * p[2];
    }
    float* h = hs + (soff + i) * rowf + px * 3;
    h[0] = a0; h[1] = a1; h[2] = a2;
  }
  __syncthreads();
  // column pass + stores: one thread per output pixel, its NOUT channels written in one place
  for (int e = threadIdx.x; e < nr * W; e += blockDim.x) {
    const int oy = e / W, px = e - oy * W;
    float l0 = 0.f, l1 = 0.f, l2 = 0.f;
    for (int k = 0; k <= 2 * r; ++k) {
      const float wk = wts[k];
      const float* p = hs + (RMAX + oy + k - r) * rowf + px * 3;
      l0 += wk * p[0]; l1 += wk * p[1]; l2 += wk * p[2];
    }
    const float* xp = xs + (RMAX + oy) * rowf + px * 3;
    const float a0 = xp[0], a1 = xp[1], a2 = xp[2];
    float c0 = l0, c1 = l1, c2 = l2;             // channels 3-5: low (blur) or x - low (high_low_pass)
    if (NOUT == 9) { c0 = a0 - l0; c1 = a1 - l1; c2 = a2 - l2; }
    const int64_t pix = ((int64_t)b * H + y0 + oy) * W + px;
    float* dst = out + pix * NOUT;
    dst[0] = a0; dst[1] = a1; dst[2] = a2; dst[3] = c0; dst[4] = c1; dst[5] = c2;
    if (NOUT == 9) { dst[6] = l0; dst[7] = l1; dst[8] = l2; }
    if constexpr (STAGED) {
      T u[8], v[8];
      u[0] = from_f32<T>(a0); u[1] = from_f32<T>(a1); u[2] = from_f32<T>(a2);
      v[0] = from_f32<T>(c0); v[1] = from_f32<T>(c1); v[2] = from_f32<T>(c2);
#pragma unroll
      for (int j = 3; j < 8; ++j) { u[j] = from_f32<T>(0.f); v[j] = from_f32<T>(0.f); }
      if constexpr (sizeof(T) == 2) {
        *(uint4*)(x8 + pix * 8) = *(uint4*)u;
        *(uint4*)(xh8 + pix * 8) = *(uint4*)v;
      } else {
        *(uint4*)(x8 + pix * 8) = *(uint4*)u; *(uint4*)(x8 + pix * 8 + 4) = *(uint4*)(u + 4);
        *(uint4*)(xh8 + pix * 8) = *(uint4*)v; *(uint4*)(xh8 + pix * 8 + 4) = *(uint4*)(v + 4);
      }
    }
  }
}

// band height: 16 rows (at B = 512 64 x 64, 8-row bands took the same time, 4-row bands 13-21 % longer), fewer where the LDS would
// exceed GAUSS_MAX_LDS; 0 when not even one row fits
static int gauss_band_rows(int H, int W, int rmax) {
  for (int br = H < 16 ? H : 16; br >= 1; br >>= 1)
    if ((int64_t)(br + 2 * rmax) * W * 3 * 4 * 2 <= GAUSS_MAX_LDS) return br;
  return 0;
}

template <typename T, int NOUT, bool STAGED>
static int gauss_launch(const float* x, const int32_t* radius, const float* stdv, int fixed_r, float mean, float fixed_std, float* out,
                        void* x8, void* xh8, int B, int H, int W, int rmax, hipStream_t stream) {
  const int br = gauss_band_rows(H, W, rmax);
  if (br == 0) return SV_E_UNSUPPORTED;
  const size_t lds = (size_t)(br + 2 * rmax) * W * 3 * 4 * 2;
  auto k = gauss_filter_kernel<T, NOUT, STAGED>;
  sv_ensure_dynamic_lds((const void*)k, lds);
  hipLaunchKernelGGL(k, dim3((H + br - 1) / br, B), dim3(256), lds, stream, x, radius, stdv, fixed_r, mean, fixed_std, out, (T*)x8,
                     (T*)xh8, H, W, br, rmax);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

static int gauss_dispatch(const float* x, const int32_t* radius, const float* stdv, int fixed_r, float mean, float fixed_std, float* out,
                          int nout, void* x8, void* xh8, int32_t dtype, bool staged, int B, int H, int W, int rmax, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!staged)
    return nout == 6 ? gauss_launch<float, 6, false>(x, radius, stdv, fixed_r, mean, fixed_std, out, nullptr, nullptr, B, H, W, rmax, s)
                     : gauss_launch<float, 9, false>(x, radius, stdv, fixed_r, mean, fixed_std, out, nullptr, nullptr, B, H, W, rmax, s);
  if (dtype == SV_BF16)
    return nout == 6 ? gauss_launch<bf16_t, 6, true>(x, radius, stdv, fixed_r, mean, fixed_std, out, x8, xh8, B, H, W, rmax, s)
                     : gauss_launch<bf16_t, 9, true>(x, radius, stdv, fixed_r, mean, fixed_std, out, x8, xh8, B, H, W, rmax, s);
  return nout == 6 ? gauss_launch<float, 6, true>(x, radius, stdv, fixed_r, mean, fixed_std, out, x8, xh8, B, H, W, rmax, s)
                   : gauss_launch<float, 9, true>(x, radius, stdv, fixed_r, mean, fixed_std, out, x8, xh8, B, H, W, rmax, s);
}

// the _staged kernels store x8 / xh8 as uint4
static bool staged_aligned16(const void* x8, const void* xh8) { return (((uintptr_t)x8 | (uintptr_t)xh8) & 15) == 0; }

static int gauss_check(int B, int H, int W, int r) {
  if (B <= 0 || H <= 0 || W <= 0 || r < 0) return SV_E_BADARG;
  if (B > GAUSS_MAX_BATCH) return SV_E_UNSUPPORTED;
  if (H != W || r > H || r > GAUSS_MAX_RADIUS || gauss_band_rows(H, W, r) == 0) return SV_E_UNSUPPORTED;
  return SV_OK;
}

extern "C" int sv_gauss_blur(const float* x, const int32_t* radius, const float* stdv, float* images6, int32_t B, int32_t H, int32_t W,
                             int32_t max_radius, void* stream) {
  if (!x || !radius || !stdv || !images6) return SV_E_BADARG;
  const int rc = gauss_check(B, H, W, max_radius);
  if (rc) return rc;
  return gauss_dispatch(x, radius, stdv, 0, 0.f, 1.f, images6, 6, nullptr, nullptr, SV_F32, false, B, H, W, max_radius, stream);
}

extern "C" int sv_gauss_blur_staged(const float* x, const int32_t* radius, const float* stdv, float* images6, void* x8, void* xh8,
                                    int32_t dtype, int32_t B, int32_t H, int32_t W, int32_t max_radius, void* stream) {
  if (!x || !radius || !stdv || !images6 || !x8 || !xh8) return SV_E_BADARG;
  if (dtype != SV_BF16 && dtype != SV_F32) return SV_E_BADARG;
  if (!staged_aligned16(x8, xh8)) return SV_E_BADARG;
  const int rc = gauss_check(B, H, W, max_radius);
  if (rc) return rc;
  return gauss_dispatch(x, radius, stdv, 0, 0.f, 1.f, images6, 6, x8, xh8, dtype, true, B, H, W, max_radius, stream);
}

extern "C" int sv_high_low_pass(const float* x, float* images9, int32_t B, int32_t H, int32_t W, int32_t size, float mean, float std,
                                void* stream) {
  if (!x || !images9 || !(std > 0.f)) return SV_E_BADARG;
  const int rc = gauss_check(B, H, W, size);
  if (rc) return rc;
  return gauss_dispatch(x, nullptr, nullptr, size, mean, std, images9, 9, nullptr, nullptr, SV_F32, false, B, H, W, size, stream);
}

extern "C" int sv_high_low_pass_staged(const float* x, float* images9, void* x8, void* xh8, int32_t dtype, int32_t B, int32_t H,
                                       int32_t W, int32_t size, float mean, float std, void* stream) {
  if (!x || !images9 || !x8 || !xh8 || !(std > 0.f)) return SV_E_BADARG;
  if (dtype != SV_BF16 && dtype != SV_F32) return SV_E_BADARG;
  if (!staged_aligned16(x8, xh8)) return SV_E_BADARG;
  const int rc = gauss_check(B, H, W, size);
  if (rc) return rc;
  return gauss_dispatch(x, nullptr, nullptr, size, mean, std, images9, 9, x8, xh8, dtype, true, B, H, W, size, stream);
}

// ============================================================================ A1b Philox draws
// Keyed like sv_random_perm: (seed ^ a per-draw tag, step, global sample index), so a shard at sample_offset draws the rows
// of the single-process batch.
__host__ __device__ inline void aug_draw(uint64_t seed, uint64_t tag, uint64_t step, uint64_t gs, uint32_t c[4]) {
  Philox ph(seed ^ tag);
  c[0] = (uint32_t)gs; c[1] = (uint32_t)(gs >> 32); c[2] = (uint32_t)step; c[3] = (uint32_t)(step >> 32);
  ph(c);
}

constexpr uint64_t BLUR_TAG = 0x626c757200000001ULL, MIX_TAG = 0x6d69787300000002ULL;

// augmentation.py:86-87: radius ~ U{3,4,5,6} (tf.random.uniform int32 minval 3 maxval 7), std ~ U[5,10)
__global__ __launch_bounds__(256) void blur_params_kernel(int32_t* __restrict__ radius, float* __restrict__ stdv, int B, uint64_t seed,
                                                          uint64_t step, int64_t sample_offset) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  uint32_t c[4];
  aug_draw(seed, BLUR_TAG, step, (uint64_t)(sample_offset + b), c);
  radius[b] = 3 + (int)(c[0] >> 30);
  float s = 5.f + 5.f * ((float)(c[1] >> 8) * (1.0f / 16777216.0f));
  stdv[b] = s < 10.f ? s : 9.99999905f;            // the largest float below 10: the interval stays half open after rounding
}

extern "C" int sv_blur_params(int32_t* radius, float* stdv, int32_t B, uint64_t seed, uint64_t step, int64_t sample_offset,
                              void* stream) {
  if (!radius || !stdv || B <= 0) return SV_E_BADARG;
  hipLaunchKernelGGL(blur_params_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, radius, stdv, B, seed, step,
                     sample_offset);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// augmentation.py:40-41: np.random.choice([1, 2, 4, 8])
__host__ __device__ inline int32_t mix_size_draw(uint64_t seed, uint64_t step, uint64_t gs) {
  uint32_t c[4];
  aug_draw(seed, MIX_TAG, step, gs, c);
  return 1 << (c[0] >> 30);
}

__global__ __launch_bounds__(256) void mix_sizes_kernel(int32_t* __restrict__ sizes, int B, uint64_t seed, uint64_t step,
                                                        int64_t sample_offset) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) sizes[b] = mix_size_draw(seed, step, (uint64_t)(sample_offset + b));
}

extern "C" int sv_mix_sizes(int32_t* sizes, int32_t B, uint64_t seed, uint64_t step, int64_t sample_offset, void* stream) {
  if (!sizes || B <= 0) return SV_E_BADARG;
  hipLaunchKernelGGL(mix_sizes_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, sizes, B, seed, step, sample_offset);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

extern "C" int32_t sv_mix_size_host(uint64_t seed, uint64_t step, int64_t sample) { return mix_size_draw(seed, step, (uint64_t)sample); }

// ============================================================================ A1b mixed-size scramble
// A row of its own patch size per image: valid when s | H and (H/s)^2 <= min(ld, 4096).  A row whose size is not (the host
// wrappers refuse such sizes) is left unwritten by the permutation kernel and copied through unscrambled by the gathers.
__device__ __forceinline__ bool mix_valid(int s, int H, int ld) {
  if (s <= 0 || s > H || H % s) return false;
  const int g = H / s;
  return g * g <= ld && g * g <= 4096;
}

// row b: the sv_random_perm permutation of (H/s_b)^2 patches (same keys: a batch of one size gives sv_random_perm's rows)
__global__ __launch_bounds__(256) void random_perm_mixed_kernel(int32_t* __restrict__ perm, const int32_t* __restrict__ sizes, int H,
                                                                int ld, uint64_t seed, uint64_t step, int64_t sample_offset) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  uint64_t* keys = (uint64_t*)smem_raw;
  const int b = blockIdx.x;
  const int s = sizes[b];
  if (!mix_valid(s, H, ld)) return;
  const int n = (H / s) * (H / s);
  int npow2 = 1;
  while (npow2 < n) npow2 <<= 1;
  const uint64_t gs = (uint64_t)(sample_offset + b);
  Philox ph(seed ^ 0x5ca1ab1e5eedULL);
  for (int i = threadIdx.x; i < npow2; i += blockDim.x) {
    uint64_t k = ~0ULL;
    if (i < n) {
      uint32_t c[4] = {(uint32_t)i, (uint32_t)gs, (uint32_t)(gs >> 32) ^ 0x7065726du, (uint32_t)step};
      ph(c);
      k = ((uint64_t)c[0] << 32) | (uint32_t)i;
    }
    keys[i] = k;
  }
  __syncthreads();
  for (int k = 2; k <= npow2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < npow2; i += blockDim.x) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const uint64_t a = keys[i], c = keys[ixj];
          const bool up = ((i & k) == 0);
          if ((a > c) == up) { keys[i] = c; keys[ixj] = a; }
        }
      }
      __syncthreads();
    }
  }
  for (int i = threadIdx.x; i < n; i += blockDim.x) perm[(int64_t)b * ld + i] = (int32_t)(uint32_t)keys[i];
}

extern "C" int sv_random_perm_mixed(int32_t* perm, const int32_t* sizes, int32_t B, int32_t H, int32_t ld, uint64_t seed, uint64_t step,
                                    int64_t sample_offset, void* stream) {
  if (!perm || !sizes || B <= 0 || H <= 0 || ld <= 0) return SV_E_BADARG;
  int n = ld < H * H ? ld : H * H;
  if (n > 4096) n = 4096;
  int npow2 = 1;
  while (npow2 < n) npow2 <<= 1;
  const size_t lds = (size_t)npow2 * sizeof(uint64_t);
  sv_ensure_dynamic_lds((const void*)random_perm_mixed_kernel, lds);
  hipLaunchKernelGGL(random_perm_mixed_kernel, dim3(B), dim3(256), lds, (hipStream_t)stream, perm, sizes, H, ld, seed, step,
                     sample_offset);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// x_aug[r*s+i, c*s+j] = x[pr*s+i, pc*s+j], (pr, pc) = divmod(perm[b][r*G+c], G), s = sizes[b], G = H/s (augmentation.py:70-81)
template <typename T, bool STAGED>
__global__ __launch_bounds__(256) void scramble_mixed_kernel(const float* __restrict__ x, const int32_t* __restrict__ perm,
                                                             const int32_t* __restrict__ sizes, int ld, float* __restrict__ out,
                                                             T* __restrict__ x8, T* __restrict__ xh8, int B, int H, int W) {
  const int64_t total = (int64_t)B * H * W;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int xw = (int)(idx % W);
    const int64_t t = idx / W;
    const int y = (int)(t % H);
    const int b = (int)(t / H);
    int64_t src = idx;
    const int s = sizes[b];
    if (mix_valid(s, H, ld)) {
      const int G = H / s;
      const int r = y / s, i = y - r * s, c = xw / s, j = xw - c * s;
      const int p = perm[(int64_t)b * ld + r * G + c];
      if (p >= 0 && p < G * G) {
        const int pr = p / G, pc = p - pr * G;
        src = ((int64_t)b * H + pr * s + i) * W + pc * s + j;
      }
    }
    const float* src0 = x + idx * 3;
    const float* src1 = x + src * 3;
    float* dst = out + idx * 6;
    const float a0 = src0[0], a1 = src0[1], a2 = src0[2];
    const float b0 = src1[0], b1 = src1[1], b2 = src1[2];
    dst[0] = a0; dst[1] = a1; dst[2] = a2; dst[3] = b0; dst[4] = b1; dst[5] = b2;
    if constexpr (STAGED) {
      T u[8], w[8];
      u[0] = from_f32<T>(a0); u[1] = from_f32<T>(a1); u[2] = from_f32<T>(a2);
      w[0] = from_f32<T>(b0); w[1] = from_f32<T>(b1); w[2] = from_f32<T>(b2);
#pragma unroll
      for (int e = 3; e < 8; ++e) { u[e] = from_f32<T>(0.f); w[e] = from_f32<T>(0.f); }
      if constexpr (sizeof(T) == 2) {
        *(uint4*)(x8 + idx * 8) = *(uint4*)u;
        *(uint4*)(xh8 + idx * 8) = *(uint4*)w;
      } else {
        *(uint4*)(x8 + idx * 8) = *(uint4*)u; *(uint4*)(x8 + idx * 8 + 4) = *(uint4*)(u + 4);
        *(uint4*)(xh8 + idx * 8) = *(uint4*)w; *(uint4*)(xh8 + idx * 8 + 4) = *(uint4*)(w + 4);
      }
    }
  }
}

template <typename T, bool STAGED>
static int mixed_launch(const float* x, const int32_t* perm, const int32_t* sizes, int ld, float* out, void* x8, void* xh8, int B, int H,
                        int W, void* stream) {
  const int64_t total = (int64_t)B * H * W;
  int grid = (int)((total + 255) / 256);
  if (grid > 256 * 16) grid = 256 * 16;
  hipLaunchKernelGGL((scramble_mixed_kernel<T, STAGED>), dim3(grid), dim3(256), 0, (hipStream_t)stream, x, perm, sizes, ld, out, (T*)x8,
                     (T*)xh8, B, H, W);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

extern "C" int sv_scramble_gather_mixed(const float* x, const int32_t* perm, const int32_t* sizes, int32_t ld, float* images6, int32_t B,
                                        int32_t H, int32_t W, void* stream) {
  if (!x || !perm || !sizes || !images6 || B <= 0 || H <= 0 || W <= 0 || ld <= 0) return SV_E_BADARG;
  if (H != W) return SV_E_UNSUPPORTED;
  return mixed_launch<float, false>(x, perm, sizes, ld, images6, nullptr, nullptr, B, H, W, stream);
}

extern "C" int sv_scramble_gather_mixed_staged(const float* x, const int32_t* perm, const int32_t* sizes, int32_t ld, float* images6,
                                               void* x8, void* xh8, int32_t dtype, int32_t B, int32_t H, int32_t W, void* stream) {
  if (!x || !perm || !sizes || !images6 || !x8 || !xh8 || B <= 0 || H <= 0 || W <= 0 || ld <= 0) return SV_E_BADARG;
  if (dtype != SV_BF16 && dtype != SV_F32) return SV_E_BADARG;
  if (!staged_aligned16(x8, xh8)) return SV_E_BADARG;
  if (H != W) return SV_E_UNSUPPORTED;
  if (dtype == SV_BF16) return mixed_launch<bf16_t, true>(x, perm, sizes, ld, images6, x8, xh8, B, H, W, stream);
  return mixed_launch<float, true>(x, perm, sizes, ld, images6, x8, xh8, B, H, W, stream);
}
