// Which kernel takes a weight gradient (no kernels here): the bf16 form chain, the fp32 tile kernel, the im2col kernel.  The trace note (SV_TRACE_DISPATCH,
// common.hip.h) is set here, at the launch of the form that ran; polyc_wgrad.hip, which sequences several launches of its own, names itself after them.
#include "common.hip.h"
#include "kernels.h"
#include "conv_geom.h"
#include "wgrad_host.h"

namespace {

// The bf16 forms in the order they are tried: trace name (include/splitvae.h lists them), supported (null: the launch decides while it plans,
// SV_E_UNSUPPORTED = nothing launched), launch.  A strip kernel launches exactly when its plan succeeds.
struct WgradForm { const char* name; bool (*supported)(const WgradArgs*, int); int (*launch)(const WgradArgs*, int, hipStream_t); };
const WgradForm bf16_forms[] = {
    {"wgrad_roll", svk_wgrad_roll_supported, svk_wgrad_roll_multi},      // d4: 6 x 6 over the upsampled 64-channel input
    {"wgrad_p5", svk_wgrad_p5_supported, svk_wgrad_p5_multi},            // d5: main term of the polyphase form
    {"wgrad_e1", svk_wgrad_e1_supported, svk_wgrad_e1_multi},
    {"wgrad_e2", svk_wgrad_e2_supported, svk_wgrad_e2_multi},
    {"wgrad_tile", nullptr, svk_wgrad_tile_multi},
};
}  // namespace

int svk_wgrad_bf16_forms_multi(const WgradArgs* w, int n, hipStream_t st) {
  if (n < 1 || n > SV_WGRAD_MAX_MULTI) return SV_E_BADARG;
  const bool force_old = sv_tune_force_im2col();
  if (force_old || w[0].lOY < 0 || w[0].lOX < 0 || w[0].S > 2) return SV_E_UNSUPPORTED;   // power-of-two grids, stride <= 2
  for (const WgradForm& f : bf16_forms) {
    if (f.supported && !f.supported(w, n)) continue;
    const int rc = f.launch(w, n, st);
    if (rc == SV_E_UNSUPPORTED) continue;
    sv_trace_note(f.name);
    return rc;
  }
  return SV_E_UNSUPPORTED;
}

// n problems of one geometry (twin networks): one launch of an LDS-tile form when the layer has one (n <= SV_WGRAD_MAX_MULTI), else the im2col kernel -- all
// of them in one launch up to SV_WGRAD_IM2COL_MAX_MULTI, one by one beyond (or with SV_NO_MULTI).  ev_mid of w[0], when set, is recorded after the main kernel.
int svk_wgrad_dispatch_multi(const WgradArgs* w, int n, int dtype, int cfg, hipStream_t st) {
  if (n < 1) return SV_E_BADARG;
  const bool no_multi = sv_tune_no_multi();
  if (n == 1 || (!no_multi && n <= SV_WGRAD_MAX_MULTI)) {
    int rc = SV_E_UNSUPPORTED;
    if (dtype == SV_BF16) rc = svk_wgrad_bf16_forms_multi(w, n, st);
    if (dtype == SV_F32) {
      rc = svk_wgrad_tile_f32_multi(w, n, st);
      if (rc != SV_E_UNSUPPORTED) sv_trace_note("wgrad_tile_f32");
    }
    if (rc != SV_E_UNSUPPORTED) return rc;
  }
  // im2col kernel (no tile instantiation for this shape, or no workspace): it needs the materialised hi-res tensor, cannot fold and reads no views.
  // (svk_wgrad_multi refuses ups / fold_kw too, but only after it has looked at msplit, which the x-packed form does not set for it: the answer
  // here must be SV_E_UNSUPPORTED, on which sv_conv2d_nhwc_wgrad retries with the plain form.)
  for (int i = 0; i < n; ++i)
    if (w[i].ups || w[i].fold_kw || w[i].s2d3 || w[i].clampin || w[i].dy_os || w[i].dy_s2d) return SV_E_UNSUPPORTED;
  int rc = SV_OK;
  if (n == 1 || (!no_multi && n <= SV_WGRAD_IM2COL_MAX_MULTI)) {
    WgradArgs wi[SV_WGRAD_IM2COL_MAX_MULTI];
    for (int i = 0; i < n; ++i) {
      wi[i] = w[i];
      if (n > 1) svg_wgrad_set_msplit(&wi[i], cfg, dtype, 512 / n);   // the problems share the chip
    }
    rc = svk_wgrad_multi(wi, n, dtype, cfg, st);
    if (rc == SV_OK) sv_trace_note("wgrad_im2col");
  } else {
    for (int i = 0; i < n && !rc; ++i) {
      WgradArgs wi = w[i];
      wi.ev_mid[0] = wi.ev_mid[1] = nullptr;
      rc = svk_wgrad_dispatch_multi(&wi, 1, dtype, cfg, st);
    }
  }
  if (rc) return rc;
  wgrad_record_mid(w[0].ev_mid, st);   // no second stage on this path
  return SV_OK;
}

int svk_wgrad_dispatch(const WgradArgs& w, int dtype, int cfg, hipStream_t st) { return svk_wgrad_dispatch_multi(&w, 1, dtype, cfg, st); }
