// SPAIR evaluation: the object-count metrics of spair/trainer.py:294-301 and tf.image.draw_bounding_boxes
// (spair/visualizer.py:110-111).  Plain C++ loads and stores only, no atomics: the same inputs give the same bits.
#include <math.h>

#include "common.hip.h"

// ============================================================================ bounding boxes
// tf.image.draw_bounding_boxes (TF 2.0 DrawBoundingBoxesOp) restated per output pixel.  TF walks the boxes of an image in
// index order and overwrites the outline pixels with the box's colour, so where outlines overlap the highest-index box wins:
// each thread owns one pixel, finds the last box whose outline covers it and writes that box's colour, or copies the input.
// No pixel is written by two threads, so `out` may alias `images`.

// (int64)(v) as TF's x86 host kernel computes it: truncation toward zero; NaN and values outside the int64 range give
// INT64_MIN (cvttss2si's "integer indefinite").  Keeps the cast defined for any box value.
__device__ __forceinline__ int64_t tf_trunc_i64(float v) {
  if (!(v >= -9.2233720368547758e18f && v < 9.2233720368547758e18f)) return INT64_MIN;
  return (int64_t)v;
}

__global__ __launch_bounds__(256) void draw_bboxes_kernel(const float* images, const float* __restrict__ boxes,
                                                          const float* __restrict__ gate, const float* __restrict__ colors,
                                                          float* out, int H, int W, int C, int NB, int NC, int ldc) {
  const int b = blockIdx.y;
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= H * W) return;
  const int64_t y = p / W, x = p - (p / W) * W;
  const float fh = (float)(H - 1), fw = (float)(W - 1);
  int hit = -1;
  for (int bb = NB - 1; bb >= 0 && hit < 0; --bb) {
    const float* bx = boxes + ((int64_t)b * NB + bb) * 4;
    const float g = gate ? gate[(int64_t)b * NB + bb] : 1.f;
    float v0 = bx[0], v1 = bx[1], v2 = bx[2], v3 = bx[3];
    if (gate) { v0 *= g; v1 *= g; v2 *= g; v3 *= g; }          // obj_bbox_mask * z_pres (spair/visualizer.py:109)
    const int64_t r0 = tf_trunc_i64(v0 * fh), c0 = tf_trunc_i64(v1 * fw);
    const int64_t r1 = tf_trunc_i64(v2 * fh), c1 = tf_trunc_i64(v3 * fw);
    if (r0 > r1 || c0 > c1) continue;                                       // inverted
    if (r0 >= H || r1 < 0 || c0 >= W || c1 < 0) continue;                   // completely outside
    const int64_t r0c = r0 > 0 ? r0 : 0, r1c = r1 < H - 1 ? r1 : H - 1;
    const int64_t c0c = c0 > 0 ? c0 : 0, c1c = c1 < W - 1 ? c1 : W - 1;
    const bool in_cols = x >= c0c && x <= c1c, in_rows = y >= r0c && y <= r1c;
    const bool top = r0 >= 0 && y == r0 && in_cols;
    const bool bottom = r1 < H && y == r1 && in_cols;
    const bool left = c0 >= 0 && x == c0 && in_rows;
    const bool right = c1 < W && x == c1 && in_rows;
    if (top || bottom || left || right) hit = bb;
  }
  const int64_t o = ((int64_t)b * H * W + p) * C;
  if (hit >= 0) {
    const float* col = colors + (int64_t)(hit % NC) * ldc;
    for (int c = 0; c < C; ++c) out[o + c] = col[c];
  } else if (out != images) {
    for (int c = 0; c < C; ++c) out[o + c] = images[o + c];
  }
}

extern "C" int sv_draw_bounding_boxes(const float* images, const float* boxes, const float* gate, const float* colors, float* out,
                                      int32_t B, int32_t H, int32_t W, int32_t C, int32_t NB, int32_t NC, int32_t ldc,
                                      void* stream) {
  if (!images || !boxes || !colors || !out) return SV_E_BADARG;
  if (B <= 0 || H <= 0 || W <= 0 || NB <= 0 || NC <= 0) return SV_E_BADARG;
  if (C != 1 && C != 3 && C != 4) return SV_E_BADARG;
  if (ldc < C) return SV_E_BADARG;
  if ((int64_t)H * W > (int64_t)INT32_MAX - 256 || B > 65535) return SV_E_UNSUPPORTED;
  const dim3 grid((unsigned)(((int64_t)H * W + 255) / 256), (unsigned)B);
  hipLaunchKernelGGL(draw_bboxes_kernel, grid, dim3(256), 0, (hipStream_t)stream, images, boxes, gate, colors, out, H, W, C, NB, NC,
                     ldc);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// ============================================================================ count metrics
// spair/trainer.py:294-301: pred_count = reduce_sum(round(sigmoid(z_pres_logits)), [1,2,3]); the batch's Keras
// mean_absolute_error and mean_absolute_percentage_error; count_acc_test.update_state(labels, pred_count).
// One workgroup: thread t owns images t, t + 256, ...; its partial sums and the LDS tree below run in one fixed order.
constexpr int COUNT_THREADS = 256;

__global__ __launch_bounds__(COUNT_THREADS) void count_metrics_kernel(const float* __restrict__ logits, int ld,
                                                                      const float* __restrict__ labels, float* __restrict__ pred,
                                                                      float* __restrict__ metrics, int32_t* __restrict__ acc, int B,
                                                                      int ncell) {
  __shared__ float s_ae[COUNT_THREADS], s_ape[COUNT_THREADS];
  __shared__ int s_eq[COUNT_THREADS];
  const int t = threadIdx.x;
  float ae = 0.f, ape = 0.f;
  int eq = 0;
  for (int b = t; b < B; b += COUNT_THREADS) {
    const float* lb = logits + (int64_t)b * ld;
    float n = 0.f;
    for (int c = 0; c < ncell; ++c) n += rintf(1.f / (1.f + expf(-lb[c])));   // fp32 sigmoid, round half to even (tf.round)
    if (pred) pred[b] = n;
    const float lab = labels[b];
    const float d = fabsf(lab - n);
    ae += d;
    ape += d / fmaxf(fabsf(lab), 1e-7f);                                          // Keras: |y - p| / max(|y|, epsilon)
    eq += (n == lab) ? 1 : 0;
  }
  s_ae[t] = ae;
  s_ape[t] = ape;
  s_eq[t] = eq;
  __syncthreads();
  for (int s = COUNT_THREADS / 2; s > 0; s >>= 1) {
    if (t < s) {
      s_ae[t] += s_ae[t + s];
      s_ape[t] += s_ape[t + s];
      s_eq[t] += s_eq[t + s];
    }
    __syncthreads();
  }
  if (t == 0) {
    metrics[0] = s_ae[0] / (float)B;
    metrics[1] = 100.f * (s_ape[0] / (float)B);
    if (acc) {                                   // one workgroup owns the counters: a plain read-modify-write
      acc[0] += s_eq[0];
      acc[1] += B;
    }
  }
}

extern "C" int sv_spair_count_metrics(const float* z_pres_logits, int32_t ld, const float* labels, float* pred, float* metrics,
                                      int32_t* acc, int32_t B, int32_t ncell, void* stream) {
  if (!z_pres_logits || !labels || !metrics) return SV_E_BADARG;
  if (B <= 0 || ncell <= 0 || ld < ncell) return SV_E_BADARG;
  hipLaunchKernelGGL(count_metrics_kernel, dim3(1), dim3(COUNT_THREADS), 0, (hipStream_t)stream, z_pres_logits, ld, labels, pred,
                     metrics, acc, B, ncell);
  SV_LAUNCH_CHECK();
  return SV_OK;
}
