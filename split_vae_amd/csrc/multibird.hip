// Multi-Bird canvas synthesis (spair/data.py:39-174 of the reference): the layout draws of a canvas (object count, background
// colours, checkerboard angle, sprite positions under the 15 % overlap rule, sprite ids) and the renderer that paints the
// background and pastes the 14 x 14 hard-masked sprites.  Canvas i of a split is a pure function of (seed, split, i): nothing is
// stored, nothing copied per step.  Plain C++ with vector stores, no atomics; every output pixel is written exactly once.
#include "common.hip.h"

constexpr int MB_SIZE = 48;                      // canvas side (create_dataset(size=48))
constexpr int MB_SPRITE = 14;                    // sprite side
constexpr int MB_OBJ = 5;                        // digits = [0, 5]
constexpr int MB_POS = MB_SIZE - MB_SPRITE;      // np.random.randint(0, 48 - 14): positions 0..33
constexpr int MB_CAP = 4096;                     // tries per object (64 wave rounds)
constexpr int MB_SPRITE_WORDS = MB_SPRITE * MB_SPRITE * 3 / 4;   // 588 bytes = 147 dwords
constexpr int MB_MAX_SPRITES = 1 << 20;
constexpr uint64_t MB_TAG = 0x6d62697264000003ULL;
enum { MB_DRAW_HEAD = 0, MB_DRAW_POS = 1, MB_DRAW_SPRITE = 2 };

// ============================================================================ draws
// Philox4x32-10 keyed by seed ^ tag; counter = (global sample index lo, hi, split, kind | object | try): try t of object k is
// addressable on its own, which is what makes the rejection loop wave-parallel without changing its result.
__host__ __device__ inline void mb_draw(uint64_t seed, int32_t split, uint64_t gs, uint32_t kind, uint32_t k, uint32_t t, uint32_t c[4]) {
  Philox ph(seed ^ MB_TAG);
  c[0] = (uint32_t)gs; c[1] = (uint32_t)(gs >> 32); c[2] = (uint32_t)split; c[3] = (kind << 28) | (k << 16) | t;
  ph(c);
}
// uniform on {0..n-1}: the high word of u * n
__host__ __device__ inline int mb_below(uint32_t u, uint32_t n) { return (int)(((uint64_t)u * n) >> 32); }

#define MB_RGB(r, g, b) (((uint32_t)(r) << 16) | ((uint32_t)(g) << 8) | (uint32_t)(b))
// the colour tables of spair/data.py:52-57 (train_colors, test_colors, train_colors_triad, test_colors_triad) as 0xRRGGBB
__host__ __device__ inline uint32_t mb_colour(int bg, int i) {
  switch (bg) {
    case SV_MB_SOLID_FIXED:
      switch (i) {
        case 0: return MB_RGB(100, 209, 72);
        case 1: return MB_RGB(209, 72, 100);
        case 2: return MB_RGB(209, 127, 72);
        case 3: return MB_RGB(72, 129, 209);
        case 4: return MB_RGB(84, 184, 209);
        case 5: return MB_RGB(209, 109, 84);
        case 6: return MB_RGB(184, 209, 84);
        case 7: return MB_RGB(109, 84, 209);
      }
      break;
    case SV_MB_UNSEEN_SOLID_FIXED:
      switch (i) {
        case 0: return MB_RGB(222, 222, 102);
        case 1: return MB_RGB(100, 100, 219);
        case 2: return MB_RGB(219, 100, 219);
        case 3: return MB_RGB(100, 219, 100);
      }
      break;
    case SV_MB_CKB_ROT_6:
      switch (i) {
        case 0: return MB_RGB(195, 135, 255);
        case 1: return MB_RGB(193, 255, 135);
        case 2: return MB_RGB(255, 165, 135);
        case 3: return MB_RGB(81, 197, 255);
        case 4: return MB_RGB(255, 229, 81);
        case 5: return MB_RGB(255, 81, 139);
      }
      break;
    case SV_MB_UNSEEN_CKB_ROT_6:
      switch (i) {
        case 0: return MB_RGB(255, 125, 227);
        case 1: return MB_RGB(125, 255, 184);
        case 2: return MB_RGB(255, 205, 125);
      }
      break;
  }
  return 0;      // an index outside its table (pinned layouts only): black
}
__host__ __device__ inline int mb_ncolours(int bg) {
  return bg == SV_MB_SOLID_FIXED ? 8 : bg == SV_MB_UNSEEN_SOLID_FIXED ? 4 : bg == SV_MB_CKB_ROT_6 ? 6 : 3;
}
__host__ __device__ inline bool mb_rotated(int bg) { return bg == SV_MB_CKB_ROT_6 || bg == SV_MB_UNSEEN_CKB_ROT_6; }

// count, background colours and angle of one canvas (create_dataset :166, create_sample :70-79, :91-96, :104)
__host__ __device__ inline void mb_head(uint64_t seed, int32_t split, uint64_t gs, int bg, int& count, int& c0, int& c1, float& angle) {
  uint32_t c[4];
  mb_draw(seed, split, gs, MB_DRAW_HEAD, 0, 0, c);
  count = mb_below(c[0], MB_OBJ + 1);
  const int n = mb_ncolours(bg);
  c0 = mb_below(c[1], n);
  if (!mb_rotated(bg)) {
    c1 = c0;
    angle = 0.f;
  } else {                                       // shuffle, take two: a uniform ordered pair of distinct colours
    c1 = mb_below(c[2], n - 1);
    if (c1 >= c0) ++c1;
    const float u = (float)(c[3] >> 8) * (1.0f / 16777216.0f);         // [0, 1)
    angle = (2.0f * u - 1.0f) * 1.57079632679489661923f;               // uniform(-1, 1) * pi / 2; 2u - 1 is exact
  }
}
__host__ __device__ inline void mb_position(uint64_t seed, int32_t split, uint64_t gs, int k, int t, int& row, int& col) {
  uint32_t c[4];
  mb_draw(seed, split, gs, MB_DRAW_POS, (uint32_t)k, (uint32_t)t, c);
  row = mb_below(c[0], MB_POS);
  col = mb_below(c[1], MB_POS);
}
__host__ __device__ inline int mb_sprite_id(uint64_t seed, int32_t split, uint64_t gs, int k, int n_sprites) {
  uint32_t c[4];
  mb_draw(seed, split, gs, MB_DRAW_SPRITE, (uint32_t)k, 0, c);
  return mb_below(c[0], (uint32_t)n_sprites);
}
// calculate_overlap (spair/data.py:31-37) for two 14-wide boxes: intersection area / 196 > 0.15  <=>  ix * iy >= 30
__host__ __device__ inline bool mb_overlaps(int r, int c, int r2, int c2) {
  const int dr = r > r2 ? r - r2 : r2 - r, dc = c > c2 ? c - c2 : c2 - c;
  const int ix = dr < MB_SPRITE ? MB_SPRITE - dr : 0, iy = dc < MB_SPRITE ? MB_SPRITE - dc : 0;
  return ix * iy >= 30;
}
__host__ __device__ inline void mb_clear(sv_multibird_layout& L) {
  L.count = 0; L.max_tries = 0; L.angle = 0.f; L.colour[0] = L.colour[1] = 0;
  for (int k = 0; k < MB_OBJ; ++k) L.row[k] = L.col[k] = L.sprite[k] = -1;
}

// the plain loop of spair/data.py:126-137, bounded by MB_CAP tries per object
static void mb_layout_seq(sv_multibird_layout& L, int bg, int n_sprites, uint64_t seed, int32_t split, uint64_t gs) {
  mb_clear(L);
  int count;
  mb_head(seed, split, gs, bg, count, L.colour[0], L.colour[1], L.angle);
  for (int k = 0; k < count; ++k) {
    int t = 0, r = 0, c = 0;
    for (; t < MB_CAP; ++t) {
      mb_position(seed, split, gs, k, t, r, c);
      bool bad = false;
      for (int j = 0; j < k; ++j) bad = bad || mb_overlaps(r, c, L.row[j], L.col[j]);
      if (!bad) break;
    }
    if (t == MB_CAP) {                           // the cap: this object and all later ones are dropped
      L.max_tries = MB_CAP;
      break;
    }
    L.row[k] = r; L.col[k] = c;
    L.sprite[k] = mb_sprite_id(seed, split, gs, k, n_sprites);
    if (t > L.max_tries) L.max_tries = t;
    L.count = k + 1;
  }
}

// The same layout by one full wave: lane l tests try 64 r + l, the ballot's lowest set bit is the first accepted try, the one
// the sequential loop accepts.  Every lane returns the same L.  All 64 lanes of the wave must be active.
__device__ __forceinline__ void mb_layout_wave(sv_multibird_layout& L, int bg, int n_sprites, uint64_t seed, int32_t split, uint64_t gs) {
  const int lane = threadIdx.x & 63;
  mb_clear(L);
  int count;
  mb_head(seed, split, gs, bg, count, L.colour[0], L.colour[1], L.angle);
  bool capped = false;
#pragma unroll
  for (int k = 0; k < MB_OBJ; ++k) {
    if (k < count && !capped) {
      bool found = false;
      for (int rd = 0; rd < MB_CAP / 64 && !found; ++rd) {
        int r, c;
        mb_position(seed, split, gs, k, rd * 64 + lane, r, c);
        bool bad = false;
#pragma unroll
        for (int j = 0; j < MB_OBJ; ++j)
          if (j < k) bad = bad || mb_overlaps(r, c, L.row[j], L.col[j]);
        const unsigned long long ok = __ballot(!bad);
        if (ok) {
          const int first = __ffsll(ok) - 1;
          L.row[k] = __shfl(r, first, 64);
          L.col[k] = __shfl(c, first, 64);
          const int t = rd * 64 + first;
          if (t > L.max_tries) L.max_tries = t;
          found = true;
        }
      }
      if (found) {
        L.sprite[k] = mb_sprite_id(seed, split, gs, k, n_sprites);
        L.count = k + 1;
      } else {
        capped = true;
        L.max_tries = MB_CAP;
      }
    }
  }
}

static int mb_check(int32_t bg, int32_t n_sprites) {
  if (n_sprites <= 0) return SV_E_BADARG;
  if (bg < SV_MB_SOLID_FIXED || bg > SV_MB_UNSEEN_CKB_ROT_6 || n_sprites > MB_MAX_SPRITES) return SV_E_UNSUPPORTED;
  return SV_OK;
}

extern "C" int sv_multibird_layout_host(sv_multibird_layout* out, int32_t bg, int32_t n_sprites, uint64_t seed, int32_t split,
                                        int64_t sample) {
  if (!out) return SV_E_BADARG;
  const int rc = mb_check(bg, n_sprites);
  if (rc) return rc;
  mb_layout_seq(*out, bg, n_sprites, seed, split, (uint64_t)sample);
  return SV_OK;
}

// one wave per canvas
__global__ __launch_bounds__(64) void multibird_layouts_kernel(sv_multibird_layout* __restrict__ out, const int64_t* __restrict__ index,
                                                               int bg, int n_sprites, uint64_t seed, int32_t split, int64_t sample_offset) {
  const int b = blockIdx.x;
  const uint64_t gs = (uint64_t)(index ? index[b] : sample_offset + b);
  sv_multibird_layout L;
  mb_layout_wave(L, bg, n_sprites, seed, split, gs);
  if (threadIdx.x == 0) out[b] = L;
}

extern "C" int sv_multibird_layouts(sv_multibird_layout* out, const int64_t* index, int32_t bg, int32_t n_sprites, int32_t B, uint64_t seed,
                                    int32_t split, int64_t sample_offset, void* stream) {
  if (!out || B <= 0) return SV_E_BADARG;
  const int rc = mb_check(bg, n_sprites);
  if (rc) return rc;
  hipLaunchKernelGGL(multibird_layouts_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, out, index, bg, n_sprites, seed, split,
                     sample_offset);
  SV_LAUNCH_CHECK();
  return SV_OK;
}

// ============================================================================ renderer
// One workgroup per canvas.  Wave 0 draws the layout (or the pinned one is copied) into LDS, the sprites it names are staged
// beside it once, then every thread paints groups of four pixels of a row (twelve floats, three 16-byte stores).
//   solid:      colour / 255
//   ckb_rot_6:  the 192 x 192 board of 6-pixel cells rotated about its centre (tfa.image.rotate: the projective transform
//               xs = cos x - sin y + xo, ys = sin x + cos y + yo, bilinear), central quarter kept: output (i, j) samples the
//               analytic board at the source point of (y, x) = (72 + i, 72 + j).  The crop stays within 35 pixels of the centre,
//               so the source never leaves the board.
//   sprites:    later objects on top; a sprite pixel replaces the canvas iff max(r, g, b) > 0, value v / 255 (a true fp32
//               division: the same bits as np.float32(v / 255.0) for every v).
__global__ __launch_bounds__(256) void multibird_canvas_kernel(float* __restrict__ x, float* __restrict__ count,
                                                               const uint32_t* __restrict__ sprites, int n_sprites,
                                                               const int64_t* __restrict__ index,
                                                               const sv_multibird_layout* __restrict__ layouts, int bg, uint64_t seed,
                                                               int32_t split, int64_t sample_offset) {
  __shared__ sv_multibird_layout Ls;
  __shared__ uint32_t spr[MB_OBJ][MB_SPRITE_WORDS];
  const int b = blockIdx.x;
  if (layouts) {
    constexpr int NW = sizeof(sv_multibird_layout) / 4;
    if (threadIdx.x < NW) ((uint32_t*)&Ls)[threadIdx.x] = ((const uint32_t*)(layouts + b))[threadIdx.x];
  } else if (threadIdx.x < 64) {
    const uint64_t gs = (uint64_t)(index ? index[b] : sample_offset + b);
    sv_multibird_layout L;
    mb_layout_wave(L, bg, n_sprites, seed, split, gs);
    if (threadIdx.x == 0) Ls = L;
  }
  __syncthreads();
  const int n = min(max(Ls.count, 0), MB_OBJ);
  for (int e = threadIdx.x; e < n * MB_SPRITE_WORDS; e += blockDim.x) {
    const int k = e / MB_SPRITE_WORDS, w = e - k * MB_SPRITE_WORDS;
    const int s = Ls.sprite[k];
    spr[k][w] = (unsigned)s < (unsigned)n_sprites ? sprites[(int64_t)s * MB_SPRITE_WORDS + w] : 0u;   // a pinned id outside the bank: empty
  }
  int row[MB_OBJ], col[MB_OBJ];
#pragma unroll
  for (int k = 0; k < MB_OBJ; ++k) { row[k] = Ls.row[k]; col[k] = Ls.col[k]; }
  const uint32_t rgb0 = mb_colour(bg, Ls.colour[0]), rgb1 = mb_colour(bg, Ls.colour[1]);
  float ca[3], cb[3];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    ca[ch] = (float)((rgb0 >> (16 - 8 * ch)) & 255u) / 255.0f;
    cb[ch] = (float)((rgb1 >> (16 - 8 * ch)) & 255u) / 255.0f;
  }
  const bool rot = mb_rotated(bg);
  float cs = 1.f, sn = 0.f, xo = 0.f, yo = 0.f;
  if (rot) {
    cs = cosf(Ls.angle); sn = sinf(Ls.angle);
    xo = (191.0f - (191.0f * cs - 191.0f * sn)) * 0.5f;
    yo = (191.0f - (191.0f * sn + 191.0f * cs)) * 0.5f;
  }
  __syncthreads();
  if (threadIdx.x == 0 && count) count[b] = (float)n;
  float* xb = x + (int64_t)b * (MB_SIZE * MB_SIZE * 3);
  constexpr int GROUPS = MB_SIZE * MB_SIZE / 4;
  for (int g = threadIdx.x; g < GROUPS; g += blockDim.x) {
    const int i = g / (MB_SIZE / 4), j0 = (g - i * (MB_SIZE / 4)) * 4;
    float v[12];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int j = j0 + p;
      bool hit = false;
#pragma unroll
      for (int k = MB_OBJ - 1; k >= 0; --k) {
        const int dr = i - row[k], dc = j - col[k];
        if (!hit && k < n && (unsigned)dr < (unsigned)MB_SPRITE && (unsigned)dc < (unsigned)MB_SPRITE) {
          const uint8_t* px = (const uint8_t*)spr[k] + (dr * MB_SPRITE + dc) * 3;
          const uint32_t r8 = px[0], g8 = px[1], b8 = px[2];
          if ((r8 | g8 | b8) != 0) {
            v[3 * p] = (float)r8 / 255.0f; v[3 * p + 1] = (float)g8 / 255.0f; v[3 * p + 2] = (float)b8 / 255.0f;
            hit = true;
          }
        }
      }
      if (!hit) {
        if (!rot) {
          v[3 * p] = ca[0]; v[3 * p + 1] = ca[1]; v[3 * p + 2] = ca[2];
        } else {
          const float fx = (float)(72 + j), fy = (float)(72 + i);
          const float xs = cs * fx - sn * fy + xo, ys = sn * fx + cs * fy + yo;
          const float xf = floorf(xs), yf = floorf(ys);
          const int x0 = (int)xf, y0 = (int)yf;
          const float wx1 = xs - xf, wx0 = (xf + 1.0f) - xs, wy1 = ys - yf, wy0 = (yf + 1.0f) - ys;
          const bool s00 = ((y0 / 6) + (x0 / 6)) & 1, s01 = ((y0 / 6) + ((x0 + 1) / 6)) & 1;
          const bool s10 = (((y0 + 1) / 6) + (x0 / 6)) & 1, s11 = (((y0 + 1) / 6) + ((x0 + 1) / 6)) & 1;
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) {
            const float a = ca[ch], c = cb[ch];
            v[3 * p + ch] = wy0 * (wx0 * (s00 ? c : a) + wx1 * (s01 ? c : a)) + wy1 * (wx0 * (s10 ? c : a) + wx1 * (s11 ? c : a));
          }
        }
      }
    }
    float4* dst = (float4*)(xb + (i * MB_SIZE + j0) * 3);
    dst[0] = make_float4(v[0], v[1], v[2], v[3]);
    dst[1] = make_float4(v[4], v[5], v[6], v[7]);
    dst[2] = make_float4(v[8], v[9], v[10], v[11]);
  }
}

extern "C" int sv_multibird_canvases(float* x, float* count, const uint8_t* sprites, int32_t n_sprites, const int64_t* index,
                                     const sv_multibird_layout* layouts, int32_t bg, int32_t B, uint64_t seed, int32_t split,
                                     int64_t sample_offset, void* stream) {
  if (!x || !sprites || B <= 0) return SV_E_BADARG;
  if (((uintptr_t)x & 15) || ((uintptr_t)sprites & 3)) return SV_E_BADARG;
  const int rc = mb_check(bg, n_sprites);
  if (rc) return rc;
  hipLaunchKernelGGL(multibird_canvas_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, x, count, (const uint32_t*)sprites, n_sprites,
                     index, layouts, bg, seed, split, sample_offset);
  SV_LAUNCH_CHECK();
  return SV_OK;
}
