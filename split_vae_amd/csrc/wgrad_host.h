// Host-side glue of the weight-gradient launchers (wgrad_roll / wgrad_p5 / wgrad_e1 / wgrad_e2 / wgrad_tile / wgrad_tile_f32 .hip, wgrad_dispatch.hip):
// what every one of them needs to agree on, each defined here once.  Host code only; the one HIP call is the event record.
#pragma once
#include "../../include/splitvae.h"
#include "kernels.h"

// THE SLAB CARVE.  A slab launch leaves its partial sums in the problem's workspace (WgradArgs::ws): `rows` workgroup rows (blockIdx.x) x `groups`
// (blockIdx.y) slabs of `per` floats, in the fragment order of the reduce (per = 4 waves x TPW * CIF * COF fragments x 256), and behind them
// one 128-float bias partial per row -- unless `bias` is false: the non-lead classes of the fused polyphase-class launch have none.
// svk_wgrad_reduce_all sums the rows in index order.  SV_WGRAD_WS_BYTES (kernels.h) is WgradSlabs(512, 1, 36 * 4 * 256).bytes().
struct WgradSlabs {
  int64_t rows = 0, groups = 0, per = 0;
  bool bias = true;
  int64_t dw_floats() const { return rows * groups * per; }
  int64_t bytes() const { return dw_floats() * 4 + (bias ? rows * 128 * 4 : 0); }
  float* bias_part(float* ws) const { return ws + dw_floats(); }      // [rows][128]
  // do these n problems' workspaces hold the carve?  (A: WgradArgs or WgradTileArgs)
  template <typename A> bool fits(const A* a, int n) const {
    for (int i = 0; i < n; ++i)
      if (!a[i].ws || a[i].ws_bytes < bytes()) return false;
    return true;
  }
};

// What a strip kernel's launch is made of: filled by the kernel's plan function (or the layer is refused), read by its _supported and _multi
struct WgradStripPlan {
  int B;            // images per problem
  int units;        // strips (roll, p5) / tasks (e1) / images (e2) per problem
  int wgs;          // workgroups per problem (gridDim.x)
  int per = 0;      // wgrad_p5: strips per team
  WgradSlabs slabs;
};

// bounding box of the tap offsets, and the input patch a TW x TH tile of output pixels reads at strides (SX, S)
struct WgradTapBox {
  int y_lo, y_hi, x_lo, x_hi;
  int in_w(int TW, int SX) const { return (TW - 1) * SX + (x_hi - x_lo) + 1; }
  int in_h(int TH, int S) const { return (TH - 1) * S + (y_hi - y_lo) + 1; }
};
inline WgradTapBox wgrad_tap_box(const WgradArgs& w) {
  WgradTapBox b = {127, -127, 127, -127};
  for (int i = 0; i < w.ntaps; ++i) {
    b.y_lo = w.dy[i] < b.y_lo ? w.dy[i] : b.y_lo; b.y_hi = w.dy[i] > b.y_hi ? w.dy[i] : b.y_hi;
    b.x_lo = w.dx[i] < b.x_lo ? w.dx[i] : b.x_lo; b.x_hi = w.dx[i] > b.x_hi ? w.dx[i] : b.x_hi;
  }
  return b;
}

// a tile of BM pixels on the (power-of-two) OY x OX grid: 16 columns (the whole row of a narrower grid), rows up to the image, then whole images
struct WgradTileShape { int lTW, lTH, lNB; };
inline WgradTileShape wgrad_tile_shape(const WgradArgs& w, int BM) {
  WgradTileShape s = {w.lOX >= 4 ? 4 : w.lOX, 0, 0};
  while ((1 << (s.lTW + s.lTH)) < BM && s.lTH < w.lOY) ++s.lTH;
  while ((1 << (s.lTW + s.lTH + s.lNB)) < BM) ++s.lNB;
  return s;
}

// the taps are the K x K window at padding P: tap t = (t / K - P, t % K - P) as (dy, dx) -- rows first -- or, x_major (wgrad_p5's list), as (dx, dy)
inline bool wgrad_taps_are_window(const WgradArgs& w, int K, int P, bool x_major = false) {
  for (int t = 0; t < K * K; ++t) {
    const int a = t / K - P, b = t % K - P;
    if (x_major ? (w.dx[t] != a || w.dy[t] != b) : (w.dy[t] != a || w.dx[t] != b)) return false;
  }
  return true;
}

// THE TAIL of a slab launch.  The profiling events, when set, are both recorded between the main kernel and the reduce ...
inline void wgrad_record_mid(const hipEvent_t* ev_mid, hipStream_t st) {
  if (ev_mid && ev_mid[0]) { (void)hipEventRecord(ev_mid[0], st); (void)hipEventRecord(ev_mid[1], st); }
}
// ... then the n reduces run at once, or -- WgradArgs::defer (polyc_wgrad.hip) -- are appended for the caller's one launch.  n = 0: nothing to reduce
inline int wgrad_finish(const WgradArgs& w, const WgradReduceDesc* rd, int n, hipStream_t st) {
  wgrad_record_mid(w.ev_mid, st);
  if (w.defer && w.n_defer && *w.n_defer + n <= 64) {
    for (int i = 0; i < n; ++i) w.defer[(*w.n_defer)++] = rd[i];
    return SV_OK;
  }
  return svk_wgrad_reduce_all(rd, n, st);
}
