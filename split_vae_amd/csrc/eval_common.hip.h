// Shared pieces of the evaluation-report kernels (iw, iw_gm, knn, latent_info, latent_dims, recon_quality, detect_ap).  No file of
// the training step includes this.
#pragma once
#include "common.hip.h"

constexpr double HALF_LOG_2PI = 0.91893853320467274178;
constexpr float LOG2E = 1.44269504088896340736f;

// ---- host: workspace carving and pointer alignment
inline int64_t up256(int64_t v) { return (v + 255) / 256 * 256; }
inline bool al(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// ---- the Philox streams of the reports that more than one file draws from
constexpr uint64_t IW_KEY = 0x1a7e17a11eedULL;     // sv_iw_advance / sv_iw_gm_advance (no other kernel of the library uses it)
constexpr uint32_t IW_TAG = 0x69770000u;           // 'iw' | stream id (0: global latent, 1: local latent, 2: component pick)
constexpr uint64_t LI_KEY = 0x1a7e27140f0ULL;      // sv_latent_info_draw; sv_latent_dims_prepare with eps = NULL reproduces its numbers
constexpr uint32_t LI_TAG = 0x6c690000u;           // 'li' | block (0: global latent, 1: local latent)
constexpr uint64_t KM_KEY = 0x1a7e3c105fe5ULL;     // sv_kmeans_seed: the first centre and the race keys of k-means++
constexpr uint32_t KM_TAG = 0x6b6d0000u;           // 'km'

// The eps sv_latent_info_draw draws for dimension j of latent block `block` of image `image` (sample_offset + row), ph = latent_info_stream(seed).
// A macro and not a function around philox_normal: the second level of inlining changes li_draw_kernel's register allocation.
__device__ __forceinline__ Philox latent_info_stream(uint64_t seed) { return Philox(seed ^ LI_KEY); }
#define LATENT_INFO_EPS(ph, image, block, j) philox_normal(ph, (uint32_t)(j), image, LI_TAG + (uint32_t)(block), 0u)

// (m, s) <- (m, s) + exp(lw) in fp64: m' = max(m, lw), s' = s exp(m - m') + exp(lw - m')
__device__ __forceinline__ void lse_push(double& m, double& s, double lw) {
  const double mn = fmax(m, lw);
  s = s * exp(m - mn) + exp(lw - mn);
  m = mn;
}

// (m, s) <- (m, s) + a chunk's fp32 (max, sum) partial w[0], w[1], in fp64.  From (-inf, 0), over the chunks in chunk order: lse = m + log(s)
__device__ __forceinline__ void lse_fold_partial(double& m, double& s, const float* w) {
  const double m2 = (double)w[0], s2 = (double)w[1];
  if (s2 > 0.0) {                                  // else an empty partial: every score of the chunk was -inf
    const double mn = fmax(m, m2);
    s = (s > 0.0 ? s * exp(m - mn) : 0.0) + s2 * exp(m2 - mn);
    m = mn;
  }
}

// the 256 partial sums of a workgroup, added in thread order; every thread adds them alike and gets the total
__device__ __forceinline__ double block_sum_ordered(double v, double* part) {
  __syncthreads();                                 // the previous use of `part` is over
  part[threadIdx.x] = v;
  __syncthreads();
  double tot = 0.0;
  for (int i = 0; i < 256; ++i) tot += part[i];    // every thread adds the same values in the same order
  return tot;
}
