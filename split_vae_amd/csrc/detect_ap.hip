// Detection average precision of SPLIT-SPAIR on Multi-Bird canvases (no reference counterpart: spair/data.py drops the positions it
// pastes the birds at).  The definitions are pinned in include/splitvae.h and DESIGN.md section 4.20.
//   sprite_extents_kernel   one wave per sprite: the tight bounds of the pixels the renderer pastes (max(r, g, b) > 0)
//   gt_boxes_kernel         one thread per canvas: layout + extents -> ground-truth boxes
//   detect_match_kernel     one wave per image: keys, the cells x 5 IoU table, local order, nine greedy passes (lane t owns threshold t)
//   ap_sort_kernel          bitonic sort of 4096-record chunks in LDS (key + TP mask)
//   ap_merge_kernel         one round of pairwise merges: a record's place = its own index + a binary search into the sibling run
//   ap_count / ap_prec<false> / ap_prec<true> / ap_final   two-level scans over 4096-record blocks: TP counts, precision maxima, the AP sums
// Plain loads and stores, no atomics: every output word has one writer and every sum one fixed order, so the same inputs give the
// same bits.  The per-image and per-sprite arithmetic is __host__ __device__: the *_host entries run it without a device.
#include <math.h>

#include "eval_common.hip.h"

#pragma clang fp contract(off)                     // inter, the areas and the union are individually rounded (also -ffp-contract=off)

namespace {

constexpr int DA_GT = 5;                           // ground-truth slots per canvas (the generator's 0..5 objects)
constexpr int DA_T = 9;                            // IoU thresholds 0.1 .. 0.9
constexpr int DA_CELLS = 64;                       // cells per image: one lane each
constexpr int DA_SPRITE = 14, DA_CANVAS = 48;
constexpr uint32_t DA_NONDET = 0xFFFFFFFFu;        // high word of a non-detection's key: sorts behind every detection
constexpr int DA_CHUNK = 4096;                     // records per LDS sort chunk and per scan block: 32 KiB of keys + 8 KiB of masks
constexpr int DA_SORT_THREADS = 512;
constexpr int DA_SCAN_THREADS = 256;
constexpr int DA_PER = DA_CHUNK / DA_SCAN_THREADS; // consecutive records per scan thread
constexpr int64_t DA_MAX_RECORDS = 1 << 20;
constexpr uint16_t DA_DET = 0x8000;                // bit 15 of a sorted record's mask: the record is a detection
constexpr int DA_OUT = 29;                         // AP_t[9], AP'_t[9] fp64; TP_t(M)[9], M, G int64

// ---------------------------------------------------------------------------- shared per-image arithmetic
__host__ __device__ inline uint32_t da_bits(float v) {
  union { float f; uint32_t u; } c;
  c.f = v;
  return c.u;
}
__host__ __device__ inline bool da_finite(float v) { return (da_bits(v) & 0x7F800000u) != 0x7F800000u; }
// a box counts as an area iff its four coordinates are finite and ymax > ymin, xmax > xmin
__host__ __device__ inline bool da_valid(const float* b) {
  return da_finite(b[0]) && da_finite(b[1]) && da_finite(b[2]) && da_finite(b[3]) && b[2] > b[0] && b[3] > b[1];
}
// detection d against box g: iou (0 unless the intersection is positive) and the 9-bit mask of thresholds t with
// inter > 0 and 10 * inter >= t * union
__host__ __device__ inline void da_pair(const float* d, const float* g, float& iou, uint32_t& pass) {
  iou = 0.f;
  pass = 0;
  if (!da_valid(d) || !da_valid(g)) return;
  const float ih = fminf(d[2], g[2]) - fmaxf(d[0], g[0]);
  const float iw = fminf(d[3], g[3]) - fmaxf(d[1], g[1]);
  if (!(ih > 0.f) || !(iw > 0.f)) return;
  const float inter = ih * iw;
  const float a = (d[2] - d[0]) * (d[3] - d[1]);
  const float b = (g[2] - g[0]) * (g[3] - g[1]);
  const float sum = a + b;
  const float uni = sum - inter;
  if (!(inter > 0.f)) return;
  iou = inter / uni;
  const float lhs = 10.f * inter;
  for (int t = 1; t <= DA_T; ++t) {
    const float rhs = (float)t * uni;
    if (lhs >= rhs) pass |= 1u << (t - 1);
  }
}
// logit > 0 on the bits (denormals count, whatever the float mode): +0 < u <= +inf.  NaN, +-0 and negatives: no detection
__host__ __device__ inline bool da_detects(float logit) { return da_bits(logit) - 1u < 0x7F800000u; }
// ascending key order = descending logit, then ascending id
__host__ __device__ inline uint64_t da_key(float logit, uint32_t id) {
  if (!da_detects(logit)) return ((uint64_t)DA_NONDET << 32) | id;
  const uint32_t u = da_bits(logit);
  const uint32_t asc = u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
  return ((uint64_t)(~asc) << 32) | id;
}
// the greedy pass of threshold bit t over an image's detections in key order: tp[cell] = 1 for a true positive
__host__ __device__ inline void da_greedy(int t, int n_det, const uint8_t* order, const float* iou, const uint16_t* pass, int n_gt,
                                          uint8_t* tp) {
  uint32_t matched = 0;
  for (int r = 0; r < n_det; ++r) {
    const int j = order[r];
    int best = -1;
    float best_iou = 0.f;
    for (int g = 0; g < n_gt; ++g) {
      if ((matched >> g) & 1u) continue;
      if (!((pass[j * DA_GT + g] >> t) & 1u)) continue;
      const float v = iou[j * DA_GT + g];
      if (best < 0 || v > best_iou) { best = g; best_iou = v; }
    }
    if (best >= 0) matched |= 1u << best;
    tp[j] = best >= 0 ? 1 : 0;
  }
}
__host__ __device__ inline int da_clamp_gt(int n) { return n < 0 ? 0 : n > DA_GT ? DA_GT : n; }

// ---------------------------------------------------------------------------- sprite extents and ground-truth boxes
__host__ __device__ inline bool da_pixel_on(const uint8_t* px) { return (px[0] | px[1] | px[2]) != 0; }

// boxes[5][4], n_gt of one canvas: slot order = object order, objects without a box skipped, unused slots zero
__host__ __device__ inline void da_gt_boxes(const int32_t* layout, const int32_t* extents, int n_sprites, float* boxes, int32_t* n_gt) {
  const int count = da_clamp_gt(layout[0]);
  int n = 0;
  for (int k = 0; k < count; ++k) {
    const int row = layout[1 + k], col = layout[6 + k], s = layout[11 + k];
    if ((unsigned)s >= (unsigned)n_sprites) continue;
    const int32_t* e = extents + (int64_t)s * 4;
    if (e[0] < 0) continue;
    boxes[n * 4 + 0] = (float)(row + e[0]) / (float)DA_CANVAS;
    boxes[n * 4 + 1] = (float)(col + e[1]) / (float)DA_CANVAS;
    boxes[n * 4 + 2] = (float)(row + e[2] + 1) / (float)DA_CANVAS;
    boxes[n * 4 + 3] = (float)(col + e[3] + 1) / (float)DA_CANVAS;
    ++n;
  }
  for (int i = n * 4; i < DA_GT * 4; ++i) boxes[i] = 0.f;
  *n_gt = n;
}

__global__ __launch_bounds__(64) void sprite_extents_kernel(const uint8_t* __restrict__ bank, int32_t* __restrict__ out) {
  const int s = blockIdx.x, lane = threadIdx.x;
  const uint8_t* sp = bank + (int64_t)s * (DA_SPRITE * DA_SPRITE * 3);
  int r0 = DA_SPRITE, c0 = DA_SPRITE, r1 = -1, c1 = -1;
  for (int p = lane; p < DA_SPRITE * DA_SPRITE; p += 64) {
    if (da_pixel_on(sp + p * 3)) {
      const int r = p / DA_SPRITE, c = p - r * DA_SPRITE;
      r0 = min(r0, r); c0 = min(c0, c); r1 = max(r1, r); c1 = max(c1, c);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    r0 = min(r0, __shfl_xor(r0, o, 64)); c0 = min(c0, __shfl_xor(c0, o, 64));
    r1 = max(r1, __shfl_xor(r1, o, 64)); c1 = max(c1, __shfl_xor(c1, o, 64));
  }
  if (lane == 0) {
    const bool any = r1 >= 0;
    int32_t* o = out + (int64_t)s * 4;
    o[0] = any ? r0 : -1; o[1] = any ? c0 : -1; o[2] = any ? r1 : -1; o[3] = any ? c1 : -1;
  }
}

__global__ __launch_bounds__(256) void gt_boxes_kernel(const int32_t* __restrict__ layouts, const int32_t* __restrict__ extents, int n_sprites,
                                                       float* __restrict__ boxes, int32_t* __restrict__ n_gt, int B) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  float bx[DA_GT * 4];
  int32_t n;
  da_gt_boxes(layouts + b * 20, extents, n_sprites, bx, &n);
  for (int i = 0; i < DA_GT * 4; ++i) boxes[b * (DA_GT * 4) + i] = bx[i];
  n_gt[b] = n;
}

// ---------------------------------------------------------------------------- matching
struct MatchArgs {
  const float* bbox; const float* logits; const float* gt; const int32_t* n_gt;
  uint64_t* key; uint16_t* tp;
  int64_t ld_bbox, ld_logits, image_offset;
  int cells, B;
};

__global__ __launch_bounds__(64) void detect_match_kernel(const MatchArgs a) {
  __shared__ uint64_t s_key[DA_CELLS];
  __shared__ float s_iou[DA_CELLS * DA_GT];
  __shared__ uint16_t s_pass[DA_CELLS * DA_GT];
  __shared__ uint8_t s_order[DA_CELLS];
  __shared__ uint8_t s_tp[DA_T][DA_CELLS];
  const int b = blockIdx.x, lane = threadIdx.x, cells = a.cells;
  const int n_gt = da_clamp_gt(a.n_gt[b]);
  const bool have = lane < cells;
  const uint32_t id = (uint32_t)((a.image_offset + b) * cells + lane);
  uint64_t key = ~0ull;
  bool det = false;
  if (have) {
    const float logit = a.logits[(int64_t)b * a.ld_logits + lane];
    det = da_detects(logit);
    key = da_key(logit, id);
    const float* d = a.bbox + (int64_t)b * a.ld_bbox + lane * 4;
    const float dd[4] = {d[0], d[1], d[2], d[3]};
    for (int g = 0; g < DA_GT; ++g) {
      float iou = 0.f;
      uint32_t pass = 0;
      if (g < n_gt) {
        const float* gp = a.gt + ((int64_t)b * DA_GT + g) * 4;
        const float gg[4] = {gp[0], gp[1], gp[2], gp[3]};
        da_pair(dd, gg, iou, pass);
      }
      s_iou[lane * DA_GT + g] = iou;
      s_pass[lane * DA_GT + g] = (uint16_t)pass;
    }
  }
  s_key[lane] = key;
#pragma unroll
  for (int t = 0; t < DA_T; ++t) s_tp[t][lane] = 0;
  __syncthreads();
  int rank = 0;
  for (int k = 0; k < cells; ++k) rank += s_key[k] < key ? 1 : 0;
  if (det) s_order[rank] = (uint8_t)lane;          // detections sort first and keys are unique: ranks 0 .. n_det - 1, one writer each
  const int n_det = __popcll(__ballot(det));
  __syncthreads();
  if (lane < DA_T) da_greedy(lane, n_det, s_order, s_iou, s_pass, n_gt, s_tp[lane]);
  __syncthreads();
  if (have) {
    uint32_t m = 0;
#pragma unroll
    for (int t = 0; t < DA_T; ++t) m |= (uint32_t)s_tp[t][lane] << t;
    a.key[id] = key;
    a.tp[id] = (uint16_t)(det ? m : 0);
  }
}

int match_check(const float* bbox, int64_t ld_bbox, const float* logits, int64_t ld_logits, int32_t cells, const float* gt, const int32_t* n_gt,
                int32_t B, int64_t image_offset, const uint64_t* key, const uint16_t* tp) {
  if (!bbox || !logits || !gt || !n_gt || !key || !tp) return SV_E_BADARG;
  if (((uintptr_t)bbox & 3) || ((uintptr_t)logits & 3) || ((uintptr_t)gt & 3) || ((uintptr_t)n_gt & 3) || ((uintptr_t)key & 7) || ((uintptr_t)tp & 1))
    return SV_E_BADARG;
  if (B <= 0 || cells <= 0 || image_offset < 0 || ld_bbox < (int64_t)cells * 4 || ld_logits < cells) return SV_E_BADARG;
  if (cells > DA_CELLS || image_offset + B > (int64_t)INT32_MAX / DA_CELLS) return SV_E_UNSUPPORTED;
  return SV_OK;
}

// ---------------------------------------------------------------------------- the curve
inline int64_t da_blocks(int64_t n) { return (n + DA_CHUNK - 1) / DA_CHUNK; }
struct ApLayout { int64_t key[2], tp[2], cnt, mx, sum, total; };
inline ApLayout ap_layout(int64_t n) {
  const int64_t nb = da_blocks(n);
  ApLayout L;
  int64_t o = 0;
  for (int i = 0; i < 2; ++i) { L.key[i] = o; o += up256(n * 8); }
  for (int i = 0; i < 2; ++i) { L.tp[i] = o; o += up256(n * 2); }
  L.cnt = o; o += up256(nb * 4 * 8);
  L.mx = o; o += up256(nb * DA_T * 8);
  L.sum = o; o += up256(nb * 2 * DA_T * 8);
  L.total = o;
  return L;
}

__global__ __launch_bounds__(DA_SORT_THREADS) void ap_sort_kernel(const uint64_t* __restrict__ key, const uint16_t* __restrict__ tp,
                                                                   uint64_t* __restrict__ okey, uint16_t* __restrict__ otp, int64_t n) {
  __shared__ uint64_t s_key[DA_CHUNK];
  __shared__ uint16_t s_tp[DA_CHUNK];
  const int64_t base = (int64_t)blockIdx.x * DA_CHUNK;
  const int cnt = (int)min((int64_t)DA_CHUNK, n - base);
  int size = 2;
  while (size < cnt) size <<= 1;                   // the network runs over the next power of two; the padding keys sort last
  for (int i = threadIdx.x; i < size; i += DA_SORT_THREADS) {
    uint64_t k = ~0ull;
    uint16_t m = 0;
    if (i < cnt) {
      k = key[base + i];
      const bool det = (uint32_t)(k >> 32) != DA_NONDET;
      m = det ? (uint16_t)((tp[base + i] & 0x1FF) | DA_DET) : (uint16_t)0;
    }
    s_key[i] = k;
    s_tp[i] = m;
  }
  __syncthreads();
  for (int k = 2; k <= size; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int p = threadIdx.x; p < (size >> 1); p += DA_SORT_THREADS) {
        const int i = 2 * p - (p & (j - 1)), l = i + j;
        const bool up = (i & k) == 0;
        const uint64_t ki = s_key[i], kl = s_key[l];
        if ((ki > kl) == up) {
          s_key[i] = kl; s_key[l] = ki;
          const uint16_t ti = s_tp[i];
          s_tp[i] = s_tp[l]; s_tp[l] = ti;
        }
      }
      __syncthreads();
    }
  }
  for (int i = threadIdx.x; i < cnt; i += DA_SORT_THREADS) {
    okey[base + i] = s_key[i];
    otp[base + i] = s_tp[i];
  }
}

// runs of `run` sorted records -> runs of 2 * run: left records go behind the right records that are smaller, right records behind the
// left records that are not larger (a stable merge: a permutation whatever the keys)
__global__ __launch_bounds__(256) void ap_merge_kernel(const uint64_t* __restrict__ key, const uint16_t* __restrict__ tp,
                                                       uint64_t* __restrict__ okey, uint16_t* __restrict__ otp, int64_t n, int64_t run) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t start = i / (2 * run) * (2 * run);
  const int64_t mid = min(start + run, n), end = min(start + 2 * run, n);
  const uint64_t k = key[i];
  const bool left = i < mid;
  int64_t lo = left ? mid : start, hi = left ? end : mid;
  const int64_t from = lo;
  while (lo < hi) {
    const int64_t m = (lo + hi) >> 1;
    const uint64_t v = key[m];
    if (left ? v < k : v <= k) lo = m + 1; else hi = m;
  }
  const int64_t pos = start + (i - (left ? start : mid)) + (lo - from);
  okey[pos] = k;
  otp[pos] = tp[i];
}

// three 21-bit counters to a word: thresholds 3 w .. 3 w + 2 in words 0 .. 2, the detection count in word 3
struct Cnt4 { uint64_t w[4]; };
__device__ __forceinline__ void cnt_add(Cnt4& c, uint32_t m) {
  c.w[0] += (uint64_t)(m & 1) | ((uint64_t)((m >> 1) & 1) << 21) | ((uint64_t)((m >> 2) & 1) << 42);
  c.w[1] += (uint64_t)((m >> 3) & 1) | ((uint64_t)((m >> 4) & 1) << 21) | ((uint64_t)((m >> 5) & 1) << 42);
  c.w[2] += (uint64_t)((m >> 6) & 1) | ((uint64_t)((m >> 7) & 1) << 21) | ((uint64_t)((m >> 8) & 1) << 42);
  c.w[3] += (uint64_t)((m >> 15) & 1);
}
__device__ __forceinline__ int64_t cnt_get(const Cnt4& c, int t) { return (int64_t)((c.w[t / 3] >> (21 * (t % 3))) & 0x1FFFFF); }

// the masks of this thread's DA_PER consecutive records (0 past the end) and their packed counts
__device__ __forceinline__ Cnt4 load_masks(const uint16_t* __restrict__ tp, int64_t first, int64_t n, uint32_t (&m)[DA_PER]) {
  Cnt4 c = {{0, 0, 0, 0}};
#pragma unroll
  for (int e = 0; e < DA_PER; ++e) {
    m[e] = first + e < n ? tp[first + e] : 0u;
    cnt_add(c, m[e]);
  }
  return c;
}

// exclusive prefix of the packed counts over the workgroup's threads plus the blocks before this one; total (may be NULL): the block's own counts
__device__ __forceinline__ Cnt4 scan_counts(const Cnt4& mine, const uint64_t* __restrict__ blockcnt, int block, uint64_t (*s)[DA_SCAN_THREADS], Cnt4* total) {
  const int t = threadIdx.x;
#pragma unroll
  for (int w = 0; w < 4; ++w) s[w][t] = mine.w[w];
  __syncthreads();
  for (int o = 1; o < DA_SCAN_THREADS; o <<= 1) {
    uint64_t v[4];
#pragma unroll
    for (int w = 0; w < 4; ++w) v[w] = t >= o ? s[w][t - o] : 0;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < 4; ++w) s[w][t] += v[w];
    __syncthreads();
  }
  Cnt4 ex;
#pragma unroll
  for (int w = 0; w < 4; ++w) ex.w[w] = s[w][t] - mine.w[w];
  if (total)
#pragma unroll
    for (int w = 0; w < 4; ++w) total->w[w] = s[w][DA_SCAN_THREADS - 1];
  __syncthreads();
  if (blockcnt) {                                  // the blocks before this one, folded by the same tree in one fixed order (integers: exact)
    Cnt4 p = {{0, 0, 0, 0}};
    for (int c = t; c < block; c += DA_SCAN_THREADS)
#pragma unroll
      for (int w = 0; w < 4; ++w) p.w[w] += blockcnt[(int64_t)c * 4 + w];
#pragma unroll
    for (int w = 0; w < 4; ++w) s[w][t] = p.w[w];
    __syncthreads();
    for (int o = DA_SCAN_THREADS / 2; o > 0; o >>= 1) {
      if (t < o)
#pragma unroll
        for (int w = 0; w < 4; ++w) s[w][t] += s[w][t + o];
      __syncthreads();
    }
#pragma unroll
    for (int w = 0; w < 4; ++w) ex.w[w] += s[w][0];
    __syncthreads();
  }
  return ex;
}

__global__ __launch_bounds__(DA_SCAN_THREADS) void ap_count_kernel(const uint16_t* __restrict__ tp, int64_t n, uint64_t* __restrict__ blockcnt) {
  __shared__ uint64_t s[4][DA_SCAN_THREADS];
  uint32_t m[DA_PER];
  const Cnt4 mine = load_masks(tp, (int64_t)blockIdx.x * DA_CHUNK + threadIdx.x * DA_PER, n, m);
  Cnt4 total;
  scan_counts(mine, nullptr, 0, s, &total);
  if (threadIdx.x < 4) blockcnt[(int64_t)blockIdx.x * 4 + threadIdx.x] = total.w[threadIdx.x];
}

// SUMS false: blockmax[block][t] = max of p over the block's detections.  SUMS true: blocksum[block][t], [9 + t] = the block's terms of AP_t, AP'_t.
// p of the detection at sorted position i is TP_t(i) / (i + 1) in fp64 (i 0-based: detections fill positions 0 .. M - 1)
template <bool SUMS>
__global__ __launch_bounds__(DA_SCAN_THREADS) void ap_prec_kernel(const uint16_t* __restrict__ tp, int64_t n, const uint64_t* __restrict__ blockcnt,
                                                                   double* __restrict__ blockmax, double* __restrict__ blocksum, int nblocks) {
  __shared__ uint64_t s[4][DA_SCAN_THREADS];
  __shared__ double s_d[DA_T][DA_SCAN_THREADS];
  const int t = threadIdx.x, block = blockIdx.x;
  const int64_t first = (int64_t)block * DA_CHUNK + t * DA_PER;
  uint32_t m[DA_PER];
  const Cnt4 mine = load_masks(tp, first, n, m);
  const Cnt4 ex = scan_counts(mine, blockcnt, block, s, nullptr);
  int64_t run[DA_T];
#pragma unroll
  for (int q = 0; q < DA_T; ++q) run[q] = cnt_get(ex, q);
  double mx[DA_T];                                 // p counts as 0 where the record is no detection
#pragma unroll
  for (int q = 0; q < DA_T; ++q) mx[q] = 0.0;
  // (the record loops stay rolled and read the masks again -- they are in the cache --: 16 x 9 inlined fp64 divisions cost every register)
#pragma unroll 1
  for (int e = 0; e < DA_PER; ++e) {
    const uint32_t me = first + e < n ? tp[first + e] : 0u;
    const bool det = (me & DA_DET) != 0;
    const double inv = (double)(first + e + 1);
#pragma unroll
    for (int q = 0; q < DA_T; ++q) {
      run[q] += (me >> q) & 1;
      mx[q] = fmax(mx[q], det ? (double)run[q] / inv : 0.0);
    }
  }
  if constexpr (!SUMS) {
#pragma unroll
    for (int q = 0; q < DA_T; ++q) s_d[q][t] = mx[q];
    __syncthreads();
    for (int o = DA_SCAN_THREADS / 2; o > 0; o >>= 1) {
      if (t < o)
#pragma unroll
        for (int q = 0; q < DA_T; ++q) s_d[q][t] = fmax(s_d[q][t], s_d[q][t + o]);
      __syncthreads();
    }
    if (t < DA_T) blockmax[(int64_t)block * DA_T + t] = s_d[t][0];
  } else {
    // suffix maximum over the later threads of the block (inclusive scan from the right), then over the later blocks
#pragma unroll
    for (int q = 0; q < DA_T; ++q) s_d[q][t] = mx[q];
    __syncthreads();
    for (int o = 1; o < DA_SCAN_THREADS; o <<= 1) {
      double v[DA_T];
#pragma unroll
      for (int q = 0; q < DA_T; ++q) v[q] = t + o < DA_SCAN_THREADS ? s_d[q][t + o] : 0.0;
      __syncthreads();
#pragma unroll
      for (int q = 0; q < DA_T; ++q) s_d[q][t] = fmax(s_d[q][t], v[q]);
      __syncthreads();
    }
    double later[DA_T];
#pragma unroll
    for (int q = 0; q < DA_T; ++q) later[q] = t + 1 < DA_SCAN_THREADS ? s_d[q][t + 1] : 0.0;
    __syncthreads();
    double bm[DA_T];
#pragma unroll
    for (int q = 0; q < DA_T; ++q) bm[q] = 0.0;
    for (int c = block + 1 + t; c < nblocks; c += DA_SCAN_THREADS)
#pragma unroll
      for (int q = 0; q < DA_T; ++q) bm[q] = fmax(bm[q], blockmax[(int64_t)c * DA_T + q]);
#pragma unroll
    for (int q = 0; q < DA_T; ++q) s_d[q][t] = bm[q];
    __syncthreads();
    for (int o = DA_SCAN_THREADS / 2; o > 0; o >>= 1) {
      if (t < o)
#pragma unroll
        for (int q = 0; q < DA_T; ++q) s_d[q][t] = fmax(s_d[q][t], s_d[q][t + o]);
      __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < DA_T; ++q) later[q] = fmax(later[q], s_d[q][0]);
    __syncthreads();
    // this thread's terms, last record first (the running maximum; the counts run back down: the same integers, the same quotients),
    // summed in that order
    double ap[DA_T], apu[DA_T];
#pragma unroll
    for (int q = 0; q < DA_T; ++q) { ap[q] = 0.0; apu[q] = 0.0; }
#pragma unroll 1
    for (int e = DA_PER - 1; e >= 0; --e) {
      const uint32_t me = first + e < n ? tp[first + e] : 0u;
      const bool det = (me & DA_DET) != 0;
      const double inv = (double)(first + e + 1);
#pragma unroll
      for (int q = 0; q < DA_T; ++q) {
        const double p = det ? (double)run[q] / inv : 0.0;
        later[q] = fmax(later[q], p);
        if ((me >> q) & 1) { ap[q] += later[q]; apu[q] += p; }
        run[q] -= (me >> q) & 1;
      }
    }
    // the block's sums: the tree below adds the threads' terms in one fixed order
    for (int half = 0; half < 2; ++half) {
#pragma unroll
      for (int q = 0; q < DA_T; ++q) s_d[q][t] = half ? apu[q] : ap[q];
      __syncthreads();
      for (int o = DA_SCAN_THREADS / 2; o > 0; o >>= 1) {
        if (t < o)
#pragma unroll
          for (int q = 0; q < DA_T; ++q) s_d[q][t] += s_d[q][t + o];
        __syncthreads();
      }
      if (t < DA_T) blocksum[(int64_t)block * (2 * DA_T) + half * DA_T + t] = s_d[t][0];
      __syncthreads();
    }
  }
}

// out[0..8] AP_t, [9..17] AP'_t (fp64); [18..26] TP_t(M), [27] M, [28] G (int64).  One workgroup; the blocks' sums are added in block order
__global__ __launch_bounds__(256) void ap_final_kernel(const uint64_t* __restrict__ blockcnt, const double* __restrict__ blocksum, int nblocks,
                                                       const int32_t* __restrict__ n_gt, int64_t n_images, double* __restrict__ out) {
  __shared__ int64_t s_g[256];
  const int t = threadIdx.x;
  int64_t g = 0;
  for (int64_t b = t; b < n_images; b += 256) g += da_clamp_gt(n_gt[b]);
  s_g[t] = g;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) s_g[t] += s_g[t + o];
    __syncthreads();
  }
  const int64_t G = s_g[0];
  int64_t* iout = (int64_t*)out;
  if (t < 2 * DA_T) {
    double sum = 0.0;
    for (int c = 0; c < nblocks; ++c) sum += blocksum[(int64_t)c * (2 * DA_T) + t];
    out[t] = G > 0 ? sum / (double)G : 0.0;
  } else if (t < 2 * DA_T + DA_T + 1) {
    const int q = t - 2 * DA_T;                    // 0 .. 8: thresholds; 9: detections
    int64_t tot = 0;
    for (int c = 0; c < nblocks; ++c) {
      Cnt4 v;
#pragma unroll
      for (int w = 0; w < 4; ++w) v.w[w] = blockcnt[(int64_t)c * 4 + w];
      tot += q < DA_T ? cnt_get(v, q) : (int64_t)(v.w[3] & 0x1FFFFF);
    }
    iout[t] = tot;
  } else if (t == DA_OUT - 1) {
    iout[t] = G;
  }
}

}  // namespace

// ============================================================================ entries
extern "C" int sv_sprite_extents_host(const uint8_t* bank, int32_t n, int32_t* out) {
  if (!bank || !out || n <= 0) return SV_E_BADARG;
  for (int s = 0; s < n; ++s) {
    const uint8_t* sp = bank + (int64_t)s * (DA_SPRITE * DA_SPRITE * 3);
    int r0 = DA_SPRITE, c0 = DA_SPRITE, r1 = -1, c1 = -1;
    for (int p = 0; p < DA_SPRITE * DA_SPRITE; ++p) {
      if (!da_pixel_on(sp + p * 3)) continue;
      const int r = p / DA_SPRITE, c = p - r * DA_SPRITE;
      r0 = r < r0 ? r : r0; c0 = c < c0 ? c : c0; r1 = r > r1 ? r : r1; c1 = c > c1 ? c : c1;
    }
    const bool any = r1 >= 0;
    int32_t* o = out + (int64_t)s * 4;
    o[0] = any ? r0 : -1; o[1] = any ? c0 : -1; o[2] = any ? r1 : -1; o[3] = any ? c1 : -1;
  }
  return SV_OK;
}

extern "C" int sv_sprite_extents(const uint8_t* bank, int32_t n, int32_t* out, void* stream) {
  if (!bank || !out || n <= 0 || ((uintptr_t)out & 3)) return SV_E_BADARG;
  if (n > (1 << 20)) return SV_E_UNSUPPORTED;
  hipLaunchKernelGGL(sprite_extents_kernel, dim3(n), dim3(64), 0, (hipStream_t)stream, bank, out);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

static int gt_check(const void* layouts, const void* extents, int32_t n_sprites, const void* boxes, const void* n_gt, int32_t B) {
  if (!layouts || !extents || !boxes || !n_gt || n_sprites <= 0 || B <= 0) return SV_E_BADARG;
  if (((uintptr_t)layouts & 3) || ((uintptr_t)extents & 3) || ((uintptr_t)boxes & 3) || ((uintptr_t)n_gt & 3)) return SV_E_BADARG;
  if (n_sprites > (1 << 20)) return SV_E_UNSUPPORTED;
  return SV_OK;
}

extern "C" int sv_multibird_gt_boxes_host(const sv_multibird_layout* layouts, const int32_t* extents, int32_t n_sprites, float* boxes,
                                          int32_t* n_gt, int32_t B) {
  const int rc = gt_check(layouts, extents, n_sprites, boxes, n_gt, B);
  if (rc) return rc;
  for (int64_t b = 0; b < B; ++b) da_gt_boxes((const int32_t*)layouts + b * 20, extents, n_sprites, boxes + b * (DA_GT * 4), n_gt + b);
  return SV_OK;
}

extern "C" int sv_multibird_gt_boxes(const sv_multibird_layout* layouts, const int32_t* extents, int32_t n_sprites, float* boxes,
                                     int32_t* n_gt, int32_t B, void* stream) {
  const int rc = gt_check(layouts, extents, n_sprites, boxes, n_gt, B);
  if (rc) return rc;
  static_assert(sizeof(sv_multibird_layout) == 80, "layout words");
  hipLaunchKernelGGL(gt_boxes_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const int32_t*)layouts, extents, n_sprites, boxes,
                     n_gt, B);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

extern "C" int sv_detect_match_host(const float* bbox, int64_t ld_bbox, const float* logits, int64_t ld_logits, int32_t cells, const float* gt_boxes,
                                    const int32_t* n_gt, int32_t B, int64_t image_offset, uint64_t* rec_key, uint16_t* rec_tp) {
  const int rc = match_check(bbox, ld_bbox, logits, ld_logits, cells, gt_boxes, n_gt, B, image_offset, rec_key, rec_tp);
  if (rc) return rc;
  for (int64_t b = 0; b < B; ++b) {
    uint64_t key[DA_CELLS];
    float iou[DA_CELLS * DA_GT];
    uint16_t pass[DA_CELLS * DA_GT];
    uint8_t order[DA_CELLS], tp[DA_T][DA_CELLS];
    const int ng = da_clamp_gt(n_gt[b]);
    int n_det = 0;
    for (int j = 0; j < cells; ++j) {
      const float logit = logits[b * ld_logits + j];
      key[j] = da_key(logit, (uint32_t)((image_offset + b) * cells + j));
      n_det += da_detects(logit) ? 1 : 0;
      for (int g = 0; g < DA_GT; ++g) {
        float v = 0.f;
        uint32_t p = 0;
        if (g < ng) da_pair(bbox + b * ld_bbox + j * 4, gt_boxes + (b * DA_GT + g) * 4, v, p);
        iou[j * DA_GT + g] = v;
        pass[j * DA_GT + g] = (uint16_t)p;
      }
    }
    for (int j = 0; j < cells; ++j) {
      int rank = 0;
      for (int k = 0; k < cells; ++k) rank += key[k] < key[j] ? 1 : 0;
      if (rank < n_det) order[rank] = (uint8_t)j;
    }
    for (int t = 0; t < DA_T; ++t) {
      for (int j = 0; j < cells; ++j) tp[t][j] = 0;
      da_greedy(t, n_det, order, iou, pass, ng, tp[t]);
    }
    for (int j = 0; j < cells; ++j) {
      const int64_t id = (image_offset + b) * cells + j;
      uint32_t m = 0;
      for (int t = 0; t < DA_T; ++t) m |= (uint32_t)tp[t][j] << t;
      rec_key[id] = key[j];
      rec_tp[id] = (uint16_t)((uint32_t)(key[j] >> 32) != DA_NONDET ? m : 0);
    }
  }
  return SV_OK;
}

extern "C" int sv_detect_match(const float* bbox, int64_t ld_bbox, const float* logits, int64_t ld_logits, int32_t cells, const float* gt_boxes,
                               const int32_t* n_gt, int32_t B, int64_t image_offset, uint64_t* rec_key, uint16_t* rec_tp, void* stream) {
  const int rc = match_check(bbox, ld_bbox, logits, ld_logits, cells, gt_boxes, n_gt, B, image_offset, rec_key, rec_tp);
  if (rc) return rc;
  const MatchArgs a = {bbox, logits, gt_boxes, n_gt, rec_key, rec_tp, ld_bbox, ld_logits, image_offset, cells, B};
  hipLaunchKernelGGL(detect_match_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, a);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

extern "C" int sv_detect_ap_chunk_records(void) { return DA_CHUNK; }

extern "C" int sv_detect_ap_workspace_bytes(int64_t n_records, int64_t* bytes) {
  if (!bytes) return SV_E_BADARG;
  if (n_records < 1 || n_records > DA_MAX_RECORDS) return SV_E_UNSUPPORTED;
  *bytes = ap_layout(n_records).total;
  return SV_OK;
}

extern "C" int sv_detect_ap_finish(const uint64_t* rec_key, const uint16_t* rec_tp, int64_t n_records, const int32_t* n_gt, int64_t n_images,
                                   void* workspace, int64_t workspace_bytes, double* out, void* stream) {
  if (!rec_key || !rec_tp || !n_gt || !workspace || !out) return SV_E_BADARG;
  if (((uintptr_t)rec_key & 7) || ((uintptr_t)rec_tp & 1) || ((uintptr_t)n_gt & 3) || ((uintptr_t)workspace & 15) || ((uintptr_t)out & 7)) return SV_E_BADARG;
  if (n_images < 1) return SV_E_BADARG;
  if (n_records < 1 || n_records > DA_MAX_RECORDS || n_images > DA_MAX_RECORDS) return SV_E_UNSUPPORTED;
  const ApLayout L = ap_layout(n_records);
  if (workspace_bytes < L.total) return SV_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  uint64_t* key[2] = {(uint64_t*)(ws + L.key[0]), (uint64_t*)(ws + L.key[1])};
  uint16_t* tp[2] = {(uint16_t*)(ws + L.tp[0]), (uint16_t*)(ws + L.tp[1])};
  uint64_t* cnt = (uint64_t*)(ws + L.cnt);
  double* mx = (double*)(ws + L.mx);
  double* sum = (double*)(ws + L.sum);
  const int nb = (int)da_blocks(n_records);
  hipLaunchKernelGGL(ap_sort_kernel, dim3(nb), dim3(DA_SORT_THREADS), 0, st, rec_key, rec_tp, key[0], tp[0], n_records);
  SV_LAUNCH_CHECK();
  int cur = 0;
  for (int64_t run = DA_CHUNK; run < n_records; run *= 2) {
    hipLaunchKernelGGL(ap_merge_kernel, dim3((unsigned)((n_records + 255) / 256)), dim3(256), 0, st, key[cur], tp[cur], key[cur ^ 1], tp[cur ^ 1],
                       n_records, run);
    SV_LAUNCH_CHECK();
    cur ^= 1;
  }
  hipLaunchKernelGGL(ap_count_kernel, dim3(nb), dim3(DA_SCAN_THREADS), 0, st, tp[cur], n_records, cnt);
  SV_LAUNCH_CHECK();
  hipLaunchKernelGGL(ap_prec_kernel<false>, dim3(nb), dim3(DA_SCAN_THREADS), 0, st, tp[cur], n_records, cnt, mx, sum, nb);
  SV_LAUNCH_CHECK();
  hipLaunchKernelGGL(ap_prec_kernel<true>, dim3(nb), dim3(DA_SCAN_THREADS), 0, st, tp[cur], n_records, cnt, mx, sum, nb);
  SV_LAUNCH_CHECK();
  hipLaunchKernelGGL(ap_final_kernel, dim3(1), dim3(256), 0, st, cnt, sum, nb, n_gt, n_images, out);
  SV_LAUNCH_CHECK();
  return SV_OK;
}
