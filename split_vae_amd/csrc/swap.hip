// Swap-consistency report of the latents: decode(z_g of image A, z_l of image B), re-encode the hybrid as the image it is, and rank
// the originals by their distance from the re-encoded latents.  The definitions are pinned in include/splitvae.h (sv_swap_*).
//   swap_pair_kernel        zcat[b] = [mu[ig[b], 0:Lg] | mu[il[b], Lg:Lg+Ll]] in the plan's dtype: one thread per element
//   swap_requantise_kernel  one thread per destination pixel: the means of the pixel and of its scramble source (channels 0..2 of out6,
//                           channels 3..5 are never read) -> pixel levels -> the data's own values through the 256-entry table in LDS;
//                           both halves of the 24-byte output pixel are written by the same thread, once
//   swap_gather_kernel      one wave per (target list, query): the target's row of R into the workspace (G [2][Nq][L])
//   swap_norm_kernel        sv_knn_classify's norms (dist_tile.hip.h) of Q, R and G
//   swap_thresh_kernel      workgroup = (64-query tile, target list): the distance tile of (queries m0 .., gathered rows m0 ..); its
//                           diagonal is d(q, t_s[q]) -- the bits the count pass sees in column t_s[q], since an accumulator element
//                           depends on its own row of A, its own row of B and the fixed K order alone
//   swap_count_kernel       THE HOT KERNEL.  workgroup = (64-query tile, chunk of SW_CHUNK references): for each 64-reference tile of
//                           the chunk the distance tile, then wave w takes the rows 16 w .. 16 w + 15, lane = column: two compares per
//                           (row, list) against the row's thresholds (an LDS broadcast), counted in 32 integer registers per lane;
//                           one integer butterfly per (row, list) at the end of the chunk -> partials [nchunks][Nq][2]
//   swap_fold_kernel        thread per (query, list): the chunk partials in chunk order -> rank [Nq][2]
// Integer counts only, no atomics, every output element written once: a repeat gives the same bits.  The Nq x Nr matrix never exists.
#include "dist_tile.hip.h"
#include "kernels.h"

namespace {

constexpr int SW_CHUNK = 2048;                   // reference rows per chunk of the count pass (sv_swap_chunk_rows)
constexpr int SW_MAX_L = 512, SW_MAX_NQ = 8 * 65536, SW_MAX_NR = 1 << 24;
constexpr uint64_t SW_KEY = 0x1a7e5a9c0de5ULL;   // sv_swap_shift_word_host (no kernel of the library uses it)
constexpr uint32_t SW_TAG = 0x73770000u;         // 'sw'

__device__ __forceinline__ int sw_clamp(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

// ============================================================================ sv_swap_pair
template <typename T>
__global__ __launch_bounds__(256) void swap_pair_kernel(const float* __restrict__ mu, int ldmu, const int32_t* __restrict__ ig,
                                                        const int32_t* __restrict__ il, T* __restrict__ zcat, int N, int B, int Lg, int Lc) {
  const int64_t total = (int64_t)B * Lc;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int b = (int)(e / Lc), j = (int)(e - (int64_t)b * Lc);
    const int row = sw_clamp(j < Lg ? ig[b] : il[b], N);
    zcat[e] = from_f32<T>(mu[(int64_t)row * ldmu + j]);
  }
}

// ============================================================================ sv_swap_requantise
// NaN -> level 0: fmaxf(NaN, -1) = -1 under IEEE maxNum; spelt out so that it does not hang on the lowering
__device__ __forceinline__ int sw_level(float m) {
  if (!(m == m)) return 0;
  const float v = fminf(fmaxf(m, -1.f), 1.f);
  const int l = (int)rintf(__fmaf_rn(v, 127.5f, 127.5f));
  return l < 0 ? 0 : (l > 255 ? 255 : l);
}

__global__ __launch_bounds__(256) void swap_requantise_kernel(const float* __restrict__ out6, const float* __restrict__ lut,
                                                              const int32_t* __restrict__ perm, float* __restrict__ images6, int B, int H,
                                                              int W, int s, int G) {
  __shared__ float lut_s[256];
  lut_s[threadIdx.x] = lut[threadIdx.x];
  __syncthreads();
  const int64_t total = (int64_t)B * H * W;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int xw = (int)(idx % W);
    const int64_t t = idx / W;
    const int y = (int)(t % H);
    const int b = (int)(t / H);
    const int r = y / s, i = y - r * s, c = xw / s, j = xw - c * s;
    const int p = sw_clamp(perm[(int64_t)b * G * G + r * G + c], G * G);     // a bad perm cannot read outside the image
    const int pr = p / G, pc = p - pr * G;
    const float* src0 = out6 + idx * 6;
    const float* src1 = out6 + (((int64_t)b * H + pr * s + i) * W + pc * s + j) * 6;
    float* dst = images6 + idx * 6;
    const float a0 = lut_s[sw_level(src0[0])], a1 = lut_s[sw_level(src0[1])], a2 = lut_s[sw_level(src0[2])];
    const float b0 = lut_s[sw_level(src1[0])], b1 = lut_s[sw_level(src1[1])], b2 = lut_s[sw_level(src1[2])];
    dst[0] = a0; dst[1] = a1; dst[2] = a2; dst[3] = b0; dst[4] = b1; dst[5] = b2;
  }
}

// ============================================================================ sv_swap_rank
struct SwapArgs {
  const float* q; const float* r; const int32_t* t0; const int32_t* t1;
  const float* nq; const float* nr; const float* ng;     // workspace: row norms of Q, R, G
  float* g;                                              // workspace: G [2][Nq][L], the gathered target rows
  float* thr;                                            // workspace: [2][Nq] d(q, t_s[q])
  int32_t* part;                                         // workspace: [nchunks][Nq][2]
  int32_t* rank;
  int ldq, ldr, Nq, Nr, L, nchunks, vecq, vecr, vecg;
};

__global__ __launch_bounds__(256) void swap_gather_kernel(const SwapArgs a) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);          // row = s * Nq + q
  const int lane = threadIdx.x & 63;
  if (row >= 2 * (int64_t)a.Nq) return;                                      // whole waves leave
  const int s = row >= a.Nq, q = (int)(row - (int64_t)s * a.Nq);
  const int t = sw_clamp((s ? a.t1 : a.t0)[q], a.Nr);
  const float* __restrict__ src = a.r + (int64_t)t * a.ldr;
  float* __restrict__ dst = a.g + row * a.L;
  for (int j = lane; j < a.L; j += 64) dst[j] = src[j];
}

__global__ __launch_bounds__(256) void swap_norm_kernel(const float* __restrict__ v, int ld, int N, int L, float* __restrict__ out) {
  dist_norm_rows(v, ld, N, L, out);
}

__device__ __forceinline__ void swap_row_norms(const float* __restrict__ nq, int m0, int Nq, float (&nqv)[2][4]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = (wave >> 1) * 32, lk = lane >> 4;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = m0 + wm + i * 16 + lk * 4 + r;
      nqv[i][r] = m < Nq ? nq[m] : 0.f;
    }
}

__global__ __launch_bounds__(256) void swap_thresh_kernel(const SwapArgs a) {
  __shared__ __attribute__((aligned(16))) float sA[2][DT_BK * DT_LP];
  __shared__ __attribute__((aligned(16))) float sB[2][DT_BK * DT_LP];
  __shared__ __attribute__((aligned(16))) float sD[DT_BM * DT_DP];
  const int m0 = blockIdx.x * DT_BM, s = blockIdx.y;
  float nqv[2][4];
  swap_row_norms(a.nq, m0, a.Nq, nqv);
  const float* gs = a.g + (int64_t)s * a.Nq * a.L;
  dist_tile_64x64(a.q, a.ldq, m0, a.Nq, a.vecq, gs, a.L, m0, a.Nq, a.vecg, a.L, nqv, a.ng + (int64_t)s * a.Nq, sA, sB, sD);
  const int i = threadIdx.x;
  if (i < DT_BM && m0 + i < a.Nq) a.thr[(int64_t)s * a.Nq + m0 + i] = sD[i * DT_DP + i];
}

__global__ __launch_bounds__(256) void swap_count_kernel(const SwapArgs a) {
  __shared__ __attribute__((aligned(16))) float sA[2][DT_BK * DT_LP];
  __shared__ __attribute__((aligned(16))) float sB[2][DT_BK * DT_LP];
  __shared__ __attribute__((aligned(16))) float sD[DT_BM * DT_DP];
  __shared__ __attribute__((aligned(16))) float sThr[DT_BM * 2];
  __shared__ __attribute__((aligned(16))) int sTgt[DT_BM * 2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.x * DT_BM, chunk = blockIdx.y;
  const int c0 = chunk * SW_CHUNK, c1 = min(a.Nr, c0 + SW_CHUNK);
  float nqv[2][4];
  swap_row_norms(a.nq, m0, a.Nq, nqv);
  if (tid < DT_BM * 2) {                           // entry 2 * row + s; rows past Nq count nothing that is stored
    const int row = m0 + (tid >> 1), s = tid & 1;
    const bool in = row < a.Nq;
    sThr[tid] = in ? a.thr[(int64_t)s * a.Nq + row] : 0.f;
    sTgt[tid] = in ? (s ? a.t1 : a.t0)[row] : 0;
  }                                                // visible behind the first tile's barriers
  int cnt[16][2];
#pragma unroll
  for (int rr = 0; rr < 16; ++rr) cnt[rr][0] = cnt[rr][1] = 0;
  for (int n0 = c0; n0 < c1; n0 += DT_BN) {
    dist_tile_64x64(a.q, a.ldq, m0, a.Nq, a.vecq, a.r, a.ldr, n0, c1, a.vecr, a.L, nqv, a.nr, sA, sB, sD);
    const int idx = n0 + lane;
    const bool valid = idx < c1;
#pragma unroll
    for (int rr = 0; rr < 16; ++rr) {
      const int row = wave * 16 + rr;
      const float d = sD[row * DT_DP + lane];
      const float2 th = *(const float2*)(sThr + 2 * row);
      const int2 tg = *(const int2*)(sTgt + 2 * row);
      cnt[rr][0] += (valid && idx != tg.x && (d < th.x || (d == th.x && idx < tg.x))) ? 1 : 0;
      cnt[rr][1] += (valid && idx != tg.y && (d < th.y || (d == th.y && idx < tg.y))) ? 1 : 0;
    }
  }
#pragma unroll
  for (int rr = 0; rr < 16; ++rr)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      int v = cnt[rr][s];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      const int m = m0 + wave * 16 + rr;
      if (lane == 0 && m < a.Nq) a.part[((int64_t)chunk * a.Nq + m) * 2 + s] = v;
    }
}

__global__ __launch_bounds__(256) void swap_fold_kernel(const SwapArgs a) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;          // e = 2 q + s
  if (e >= 2 * (int64_t)a.Nq) return;
  int v = 0;
  for (int c = 0; c < a.nchunks; ++c) v += a.part[(int64_t)c * a.Nq * 2 + e];
  a.rank[e] = v;
}

struct SwapLayout { int64_t nq, nr, ng, g, thr, part, total; int nchunks; };
inline SwapLayout swap_layout(int64_t Nq, int64_t Nr, int64_t L) {
  SwapLayout w;
  w.nchunks = (int)((Nr + SW_CHUNK - 1) / SW_CHUNK);
  w.nq = 0;
  w.nr = w.nq + up256(Nq * 4);
  w.ng = w.nr + up256(Nr * 4);
  w.g = w.ng + up256(2 * Nq * 4);
  w.thr = w.g + up256(2 * Nq * L * 4);
  w.part = w.thr + up256(2 * Nq * 4);
  w.total = w.part + up256((int64_t)w.nchunks * Nq * 2 * 4);
  return w;
}
inline int swap_sizes(int32_t Nq, int32_t Nr, int32_t L) {
  if (Nq <= 0 || Nr <= 0 || L <= 0) return SV_E_BADARG;
  if (Nq > SW_MAX_NQ || Nr > SW_MAX_NR || L > SW_MAX_L) return SV_E_UNSUPPORTED;
  return SV_OK;
}

}  // namespace

extern "C" int sv_swap_pair(const float* mu, int32_t ldmu, const int32_t* ig, const int32_t* il, void* zcat, int32_t dtype, int32_t N,
                            int32_t B, int32_t Lg, int32_t Ll, void* stream) {
  if (!mu || !ig || !il || !zcat || N <= 0 || B <= 0 || Lg <= 0 || Ll <= 0) return SV_E_BADARG;
  if (dtype != SV_BF16 && dtype != SV_F32) return SV_E_BADARG;
  if (!al(mu, 4) || !al(ig, 4) || !al(il, 4) || !al(zcat, dtype == SV_F32 ? 4 : 2) || ldmu < Lg + Ll) return SV_E_BADARG;
  const int Lc = Lg + Ll;
  const int64_t total = (int64_t)B * Lc;
  int grid = (int)((total + 255) / 256);
  if (grid > 4096) grid = 4096;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == SV_BF16)
    hipLaunchKernelGGL((swap_pair_kernel<bf16_t>), dim3(grid), dim3(256), 0, st, mu, ldmu, ig, il, (bf16_t*)zcat, N, B, Lg, Lc);
  else
    hipLaunchKernelGGL((swap_pair_kernel<float>), dim3(grid), dim3(256), 0, st, mu, ldmu, ig, il, (float*)zcat, N, B, Lg, Lc);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

extern "C" int sv_swap_requantise(const float* out6, const float* lut, const int32_t* perm, float* images6, int32_t B, int32_t H, int32_t W,
                                  int32_t patch, void* stream) {
  if (!out6 || !lut || !perm || !images6 || B <= 0 || H <= 0 || W <= 0 || patch <= 0) return SV_E_BADARG;
  if (!al(out6, 4) || !al(lut, 4) || !al(perm, 4) || !al(images6, 4) || (const void*)out6 == (const void*)images6) return SV_E_BADARG;
  if (H != W || H % patch) return SV_E_UNSUPPORTED;   // the scramble assumes square images, s | H (sv_scramble_gather)
  const int64_t total = (int64_t)B * H * W;
  int grid = (int)((total + 255) / 256);
  if (grid > 256 * 16) grid = 256 * 16;
  hipLaunchKernelGGL(swap_requantise_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, out6, lut, perm, images6, B, H, W, patch,
                     W / patch);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

extern "C" int sv_swap_chunk_rows(void) { return SW_CHUNK; }

extern "C" int sv_swap_rank_workspace_bytes(int32_t Nq, int32_t Nr, int32_t L, int64_t* bytes) {
  if (!bytes) return SV_E_BADARG;
  const int rc = swap_sizes(Nq, Nr, L);
  if (rc) return rc;
  *bytes = swap_layout(Nq, Nr, L).total;
  return SV_OK;
}

extern "C" int sv_swap_rank(const float* q, int32_t ldq, const float* r, int32_t ldr, const int32_t* t0, const int32_t* t1, int32_t Nq,
                            int32_t Nr, int32_t L, int32_t* rank, void* workspace, int64_t workspace_bytes, void* stream) {
  if (!q || !r || !t0 || !t1 || !rank || !workspace) return SV_E_BADARG;
  if (!al(q, 4) || !al(r, 4) || !al(t0, 4) || !al(t1, 4) || !al(rank, 4) || !al(workspace, 16)) return SV_E_BADARG;
  const int rc = swap_sizes(Nq, Nr, L);
  if (rc == SV_E_BADARG) return rc;
  if (ldq < L || ldr < L) return SV_E_BADARG;
  if (rc) return rc;
  const SwapLayout w = swap_layout(Nq, Nr, L);
  if (workspace_bytes < w.total) return SV_E_WORKSPACE;
  char* ws = (char*)workspace;
  hipStream_t st = (hipStream_t)stream;
  SwapArgs a = {q, r, t0, t1, (const float*)(ws + w.nq), (const float*)(ws + w.nr), (const float*)(ws + w.ng), (float*)(ws + w.g),
                (float*)(ws + w.thr), (int32_t*)(ws + w.part), rank, ldq, ldr, Nq, Nr, L, w.nchunks,
                !(ldq & 3) && al(q, 16), !(ldr & 3) && al(r, 16), !(L & 3)};
  const int nrows2 = 2 * Nq;
  hipLaunchKernelGGL(swap_gather_kernel, dim3((nrows2 + 3) / 4), dim3(256), 0, st, a);
  SV_LAUNCH_CHECK();
  hipLaunchKernelGGL(swap_norm_kernel, dim3((Nq + 3) / 4), dim3(256), 0, st, q, ldq, Nq, L, (float*)(ws + w.nq));
  SV_LAUNCH_CHECK();
  hipLaunchKernelGGL(swap_norm_kernel, dim3((Nr + 3) / 4), dim3(256), 0, st, r, ldr, Nr, L, (float*)(ws + w.nr));
  SV_LAUNCH_CHECK();
  hipLaunchKernelGGL(swap_norm_kernel, dim3((nrows2 + 3) / 4), dim3(256), 0, st, (const float*)(ws + w.g), L, nrows2, L, (float*)(ws + w.ng));
  SV_LAUNCH_CHECK();
  const int mt = (Nq + DT_BM - 1) / DT_BM;
  hipLaunchKernelGGL(swap_thresh_kernel, dim3(mt, 2), dim3(256), 0, st, a);
  SV_LAUNCH_CHECK();
  hipLaunchKernelGGL(swap_count_kernel, dim3(mt, w.nchunks), dim3(256), 0, st, a);
  SV_LAUNCH_CHECK();
  hipLaunchKernelGGL(swap_fold_kernel, dim3((nrows2 + 255) / 256), dim3(256), 0, st, a);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// The word the report's partner shifts are drawn from (split_vae_amd/swap.py: partner_shifts): Philox keyed by seed ^ SW_KEY, counter
// (attempt, p, 'sw' tag, 0) -- host only.
extern "C" uint32_t sv_swap_shift_word_host(uint64_t seed, int32_t p, int32_t attempt) {
  Philox ph(seed ^ SW_KEY);
  uint32_t c[4] = {(uint32_t)attempt, (uint32_t)p, SW_TAG, 0u};
  ph(c);
  return c[0];
}
