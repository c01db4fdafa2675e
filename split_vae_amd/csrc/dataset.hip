// Device-resident datasets: the batch fetch of vae/main.py:56-61 (shuffle -> batch) as a gather over a set that stays in HBM,
// alone (sv_dataset_gather, sv_dataset_onehot) or fused with the patch scramble and the step's input staging
// (sv_dataset_gather_scramble = sv_dataset_gather + sv_scramble_gather_staged in one pass).
// uint8 sources are normalised through a 256-entry table the host fills (data.normalise_u8: float64 arithmetic, rounded once),
// so the kernels reproduce vae/data.py:52 bit for bit without doing it.  Plain C++ loads and stores only: no atomics, no
// workspace, every output element written exactly once.  An index outside [0, N) is clamped: nothing is read outside src.
#include "common.hip.h"
#include "kernels.h"

__device__ __forceinline__ int ds_clamp(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

// ============================================================================ A1d gather
// One thread per 4 elements of an image: a 4-byte (uint8) or 16-byte (fp32) load, one 16-byte store; a scalar loop where the
// image's element count is no multiple of 4 (its images then start off the 16-byte grid).
__global__ __launch_bounds__(256) void dataset_gather_u8_kernel(const uint8_t* __restrict__ src, const float* __restrict__ lut,
                                                                const int32_t* __restrict__ index, float* __restrict__ x, int N, int E) {
  __shared__ float lut_s[256];
  lut_s[threadIdx.x] = lut[threadIdx.x];
  __syncthreads();
  const int b = blockIdx.y;
  const uint8_t* sp = src + (int64_t)ds_clamp(index[b], N) * E;
  float* dp = x + (int64_t)b * E;
  if ((E & 3) == 0) {
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < (E >> 2); q += gridDim.x * blockDim.x) {
      const uint32_t w = *(const uint32_t*)(sp + 4 * q);
      float4 o;
      o.x = lut_s[w & 255u]; o.y = lut_s[(w >> 8) & 255u]; o.z = lut_s[(w >> 16) & 255u]; o.w = lut_s[w >> 24];
      *(float4*)(dp + 4 * q) = o;
    }
  } else {
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < E; e += gridDim.x * blockDim.x) dp[e] = lut_s[sp[e]];
  }
}

__global__ __launch_bounds__(256) void dataset_gather_f32_kernel(const float* __restrict__ src, const int32_t* __restrict__ index,
                                                                 float* __restrict__ x, int N, int E) {
  const int b = blockIdx.y;
  const float* sp = src + (int64_t)ds_clamp(index[b], N) * E;
  float* dp = x + (int64_t)b * E;
  if ((E & 3) == 0) {
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < (E >> 2); q += gridDim.x * blockDim.x)
      *(float4*)(dp + 4 * q) = *(const float4*)(sp + 4 * q);
  } else {
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < E; e += gridDim.x * blockDim.x) dp[e] = sp[e];
  }
}

static bool ds_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// B rides in grid.y (<= 65535) and an image's elements in an int
static int ds_check(const void* src, int32_t src_dtype, const float* lut, const int32_t* index, int32_t N, int32_t B, int32_t H, int32_t W) {
  if (!src || !index || N <= 0 || B <= 0 || H <= 0 || W <= 0) return SV_E_BADARG;
  if (src_dtype != SV_SRC_U8 && src_dtype != SV_SRC_F32) return SV_E_BADARG;
  if (src_dtype == SV_SRC_U8 && !lut) return SV_E_BADARG;
  if (!ds_aligned16(src)) return SV_E_BADARG;
  if (B > 65535 || (int64_t)H * W * 3 >= (int64_t)1 << 30) return SV_E_UNSUPPORTED;
  return SV_OK;
}

extern "C" int sv_dataset_gather(const void* src, int32_t src_dtype, const float* lut, const int32_t* index, float* x, int32_t N,
                                 int32_t B, int32_t H, int32_t W, void* stream) {
  if (!x) return SV_E_BADARG;
  const int rc = ds_check(src, src_dtype, lut, index, N, B, H, W);
  if (rc) return rc;
  if (!ds_aligned16(x)) return SV_E_BADARG;
  const int E = H * W * 3;
  int gx = ((E + 3) / 4 + 255) / 256;
  if (gx > 64) gx = 64;
  if (src_dtype == SV_SRC_U8)
    hipLaunchKernelGGL(dataset_gather_u8_kernel, dim3(gx, B), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)src, lut, index, x, N, E);
  else
    hipLaunchKernelGGL(dataset_gather_f32_kernel, dim3(gx, B), dim3(256), 0, (hipStream_t)stream, (const float*)src, index, x, N, E);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// ============================================================================ A1d one-hot labels
// data.one_hot_svhn (vae/data.py:55-57): class y - 1; a label outside 1..depth gives an all-zero row (tf.one_hot).
__global__ __launch_bounds__(256) void dataset_onehot_kernel(const uint8_t* __restrict__ labels, const int32_t* __restrict__ index,
                                                             float* __restrict__ out, int N, int B, int depth) {
  const int total = B * depth;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int b = i / depth, c = i - b * depth;
    const int y = labels[ds_clamp(index[b], N)];
    out[i] = (y - 1 == c) ? 1.0f : 0.0f;
  }
}

extern "C" int sv_dataset_onehot(const uint8_t* labels, const int32_t* index, float* out, int32_t N, int32_t B, int32_t depth,
                                 void* stream) {
  if (!labels || !index || !out || N <= 0 || B <= 0 || depth <= 0) return SV_E_BADARG;
  if ((int64_t)B * depth >= (int64_t)1 << 31) return SV_E_UNSUPPORTED;
  int grid = (B * depth + 255) / 256;
  if (grid > 4096) grid = 4096;
  hipLaunchKernelGGL(dataset_onehot_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, labels, index, out, N, B, depth);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// ============================================================================ A1d gather + scramble + staging
// Destination pixel p = y * W + xw of image b takes its scrambled half from source pixel scr_pixel(p) of the same image
// (augmentation.py:43-57, the arithmetic of scramble_kernel in pointwise.hip).  A permutation entry outside [0, G * G) is
// clamped, so a bad perm cannot read outside the image either.
__device__ __forceinline__ int scr_pixel(const int32_t* __restrict__ perm_b, int p, int W, int s, int G) {
  const int y = p / W, xw = p - y * W;
  const int r = y / s, i = y - r * s, c = xw / s, j = xw - c * s;
  const int q = ds_clamp(perm_b[r * G + c], G * G);
  const int pr = q / G, pc = q - pr * G;
  return (pr * s + i) * W + pc * s + j;
}

// A workgroup works through tiles of DS_TILE consecutive pixels of one image.  Phase 1: thread t fetches pixel t of the tile and
// its scrambled partner and puts the six values into LDS in images6's layout.  Phase 2: the tile leaves through stores whose
// lanes are contiguous 16-byte chunks of each output: images6 is a straight copy of the LDS tile, a padded 8-channel pixel is
// one (bf16) or two (fp32: values + zeros) chunks.  (Measured at B = 512 64 x 64 fp32-staged: a thread that stored its own
// pixel pair as 3 + 8 sixteen-byte stores, lanes 48 / 64 B apart, took 66 us against 42 us for scramble_staged_kernel.)
constexpr int DS_TILE = 256;                // = threads per workgroup
// tiles per workgroup.  fp32 sources: 1 (2 or 4 cost the patch-1 form 17 %: 52 -> 61 us at B = 512 64 x 64); uint8 sources: 4, since
// every workgroup stages the whole image first (1 / 4 / 8 at 64 x 64: 37 / 33.5 / 33 us; at 32 x 32 the image is 4 tiles)
constexpr int DS_TILES_F32 = 1, DS_TILES_U8 = 4;

template <typename T, bool STAGED>
__device__ __forceinline__ void ds_write_tile(const float* __restrict__ t6, float* __restrict__ out, T* __restrict__ x8,
                                              T* __restrict__ xh8, int64_t gp0, int n) {
  float* dst = out + gp0 * 6;
  const int nf = n * 6;
  const int nv = (gp0 & 1) == 0 ? nf >> 2 : 0;             // an even first pixel: the tile starts on images6's 16-byte grid
  for (int c = threadIdx.x; c < nv; c += DS_TILE) ((float4*)dst)[c] = ((const float4*)t6)[c];
  for (int e = 4 * nv + threadIdx.x; e < nf; e += DS_TILE) dst[e] = t6[e];
  if constexpr (STAGED) {
    if constexpr (sizeof(T) == 2) {
      for (int c = threadIdx.x; c < n; c += DS_TILE) {
        T u[8], w[8];
#pragma unroll
        for (int e = 0; e < 3; ++e) { u[e] = from_f32<T>(t6[c * 6 + e]); w[e] = from_f32<T>(t6[c * 6 + 3 + e]); }
#pragma unroll
        for (int e = 3; e < 8; ++e) { u[e] = from_f32<T>(0.f); w[e] = from_f32<T>(0.f); }
        ((uint4*)(x8 + gp0 * 8))[c] = *(uint4*)u;
        ((uint4*)(xh8 + gp0 * 8))[c] = *(uint4*)w;
      }
    } else {
      for (int c = threadIdx.x; c < 2 * n; c += DS_TILE) {   // chunk c: the values (even) or the zero half (odd) of pixel c / 2
        const float* v = t6 + (c >> 1) * 6;
        const bool z = c & 1;
        ((float4*)(x8 + gp0 * 8))[c] = z ? make_float4(0.f, 0.f, 0.f, 0.f) : make_float4(v[0], v[1], v[2], 0.f);
        ((float4*)(xh8 + gp0 * 8))[c] = z ? make_float4(0.f, 0.f, 0.f, 0.f) : make_float4(v[3], v[4], v[5], 0.f);
      }
    }
  }
}

// uint8 source: a workgroup stages its whole image (3 KB at 32 x 32, 48 KB at 128 x 128) and the table in LDS with 16-byte
// loads and reads the identity and the scrambled half from there -- no 3-byte global loads at patch 1.  gridDim.x workgroups
// share an image's tiles (each stages the image: the repeats come out of L2).
template <typename T, bool STAGED>
__global__ __launch_bounds__(DS_TILE) void dataset_scramble_u8_kernel(const uint8_t* __restrict__ src, const float* __restrict__ lut,
                                                                      const int32_t* __restrict__ index,
                                                                      const int32_t* __restrict__ perm, float* __restrict__ out,
                                                                      T* __restrict__ x8, T* __restrict__ xh8, int N, int H, int W, int s,
                                                                      int G) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* lut_s = (float*)smem_raw;                               // [256]
  float* t6 = (float*)(smem_raw + 1024);                         // [DS_TILE][6]
  uint8_t* img = (uint8_t*)(smem_raw + 1024 + DS_TILE * 24);     // [H * W * 3]
  const int b = blockIdx.y;
  const int npix = H * W, E = npix * 3;
  const uint8_t* sp = src + (int64_t)ds_clamp(index[b], N) * E;
  lut_s[threadIdx.x] = lut[threadIdx.x];
  if ((E & 15) == 0) {
    for (int q = threadIdx.x; q < (E >> 4); q += DS_TILE) ((uint4*)img)[q] = ((const uint4*)sp)[q];
  } else {
    for (int e = threadIdx.x; e < E; e += DS_TILE) img[e] = sp[e];
  }
  __syncthreads();
  const int32_t* perm_b = perm + (int64_t)b * G * G;
  for (int tile0 = blockIdx.x * DS_TILE; tile0 < npix; tile0 += gridDim.x * DS_TILE) {
    const int p = tile0 + threadIdx.x;
    if (p < npix) {
      const uint8_t* a = img + p * 3;
      const uint8_t* h = img + scr_pixel(perm_b, p, W, s, G) * 3;
      float* t = t6 + threadIdx.x * 6;
      t[0] = lut_s[a[0]]; t[1] = lut_s[a[1]]; t[2] = lut_s[a[2]]; t[3] = lut_s[h[0]]; t[4] = lut_s[h[1]]; t[5] = lut_s[h[2]];
    }
    __syncthreads();
    ds_write_tile<T, STAGED>(t6, out, x8, xh8, (int64_t)b * npix + tile0, min(DS_TILE, npix - tile0));
    __syncthreads();
  }
}

// fp32 source: 192 KB at 128 x 128 does not fit the LDS, so every size reads both halves from global memory: the scrambled
// half's second read of the same image is served by L2 / Infinity Cache.
template <typename T, bool STAGED>
__global__ __launch_bounds__(DS_TILE) void dataset_scramble_f32_kernel(const float* __restrict__ src, const int32_t* __restrict__ index,
                                                                       const int32_t* __restrict__ perm, float* __restrict__ out,
                                                                       T* __restrict__ x8, T* __restrict__ xh8, int N, int H, int W, int s,
                                                                       int G) {
  __shared__ __attribute__((aligned(16))) float t6[DS_TILE * 6];
  const int b = blockIdx.y;
  const int npix = H * W;
  const float* sp = src + (int64_t)ds_clamp(index[b], N) * npix * 3;
  const int32_t* perm_b = perm + (int64_t)b * G * G;
  for (int tile0 = blockIdx.x * DS_TILE; tile0 < npix; tile0 += gridDim.x * DS_TILE) {
    const int p = tile0 + threadIdx.x;
    if (p < npix) {
      const float* a = sp + p * 3;
      const float* h = sp + scr_pixel(perm_b, p, W, s, G) * 3;
      float* t = t6 + threadIdx.x * 6;
      t[0] = a[0]; t[1] = a[1]; t[2] = a[2]; t[3] = h[0]; t[4] = h[1]; t[5] = h[2];
    }
    __syncthreads();
    ds_write_tile<T, STAGED>(t6, out, x8, xh8, (int64_t)b * npix + tile0, min(DS_TILE, npix - tile0));
    __syncthreads();
  }
}

constexpr int DS_MAX_LDS = 64 * 1024;

template <typename T, bool STAGED>
static int ds_scramble_launch(const void* src, int32_t src_dtype, const float* lut, const int32_t* index, const int32_t* perm, float* out,
                              void* x8, void* xh8, int N, int B, int H, int W, int patch, hipStream_t stream) {
  const int npix = H * W, G = W / patch;
  const int tiles = (npix + DS_TILE - 1) / DS_TILE;
  if (src_dtype == SV_SRC_U8) {
    const size_t lds = 1024 + DS_TILE * 24 + (((size_t)npix * 3 + 15) & ~(size_t)15);
    if (lds > (size_t)DS_MAX_LDS) return SV_E_UNSUPPORTED;
    auto k = dataset_scramble_u8_kernel<T, STAGED>;
    sv_ensure_dynamic_lds((const void*)k, lds);
    hipLaunchKernelGGL(k, dim3((tiles + DS_TILES_U8 - 1) / DS_TILES_U8, B), dim3(DS_TILE), lds, stream, (const uint8_t*)src, lut, index,
                       perm, out, (T*)x8, (T*)xh8, N, H, W, patch, G);
  } else {
    hipLaunchKernelGGL((dataset_scramble_f32_kernel<T, STAGED>), dim3((tiles + DS_TILES_F32 - 1) / DS_TILES_F32, B), dim3(DS_TILE), 0,
                       stream, (const float*)src, index, perm, out, (T*)x8, (T*)xh8, N, H, W, patch, G);
  }
  SV_LAUNCH_CHECK();
  return SV_OK;
}

extern "C" int sv_dataset_gather_scramble(const void* src, int32_t src_dtype, const float* lut, const int32_t* index, const int32_t* perm,
                                          float* images6, void* x8, void* xh8, int32_t dtype, int32_t N, int32_t B, int32_t H, int32_t W,
                                          int32_t patch, void* stream) {
  if (!perm || !images6 || patch <= 0) return SV_E_BADARG;
  if ((x8 == nullptr) != (xh8 == nullptr)) return SV_E_BADARG;
  if (x8 && dtype != SV_BF16 && dtype != SV_F32) return SV_E_BADARG;
  const int rc = ds_check(src, src_dtype, lut, index, N, B, H, W);
  if (rc) return rc;
  if (!ds_aligned16(images6) || !ds_aligned16(x8) || !ds_aligned16(xh8)) return SV_E_BADARG;
  if (H != W || H % patch) return SV_E_UNSUPPORTED;   // augmentation.py:44-46 assumes square, s | H
  hipStream_t s = (hipStream_t)stream;
  if (!x8) return ds_scramble_launch<float, false>(src, src_dtype, lut, index, perm, images6, nullptr, nullptr, N, B, H, W, patch, s);
  if (dtype == SV_BF16) return ds_scramble_launch<bf16_t, true>(src, src_dtype, lut, index, perm, images6, x8, xh8, N, B, H, W, patch, s);
  return ds_scramble_launch<float, true>(src, src_dtype, lut, index, perm, images6, x8, xh8, N, B, H, W, patch, s);
}
