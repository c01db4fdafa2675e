// Every read of the environment by libsplitvae_hip.so happens in this file (tests/test_knobs.py holds the library to that).
//
// (a) The RUNTIME SWITCHES of the shipped library: the accessors below, nothing else.  Each has a consumer outside csrc/ -- a test, bench.py
//     or the README (LAB_NOTES.md section 7 lists them with their effect).  A switch is read once per process, at its
//     first use; SV_POLYC_K alone is read per call.  Adding one needs such a consumer; a tuning experiment is not one.
// (b) TUNING KNOBS: SV_TUNE_FLAG / SV_TUNE_INT / SV_TUNE_STR at the place of the decision, beside the measurement that set the default.
//     The shipped build compiles them to that default (the name never reaches the binary, so nothing a job inherits can change the step);
//     a -DSV_DEBUG_KNOBS build (SV_EXTRA_FLAGS=-DSV_DEBUG_KNOBS SV_OBJ_TAG=_dbg SV_LIB_NAME=libsplitvae_hip_dbg.so python split_vae_amd/build.py)
//     reads them from the environment, as every build did before they were frozen.
#pragma once
#include <stdlib.h>

#define SV_KNOB_SET(fn, expr) inline bool fn() { static const bool v = (expr); return v; }
// fixed-order reductions everywhere (common.hip.h: sv_deterministic; sv_set_deterministic overrides it per launch)
SV_KNOB_SET(sv_knob_deterministic, getenv("SV_DETERMINISTIC") != nullptr && atoi(getenv("SV_DETERMINISTIC")) != 0)
// one stderr line per sv_conv2d_* call naming the form it launched (common.hip.h: sv_trace_note)
SV_KNOB_SET(sv_knob_trace_dispatch, getenv("SV_TRACE_DISPATCH") != nullptr)
// plan scopes as roctx ranges (lgvae_plan.hip: Roctx)
SV_KNOB_SET(sv_knob_roctx, getenv("SV_ROCTX") != nullptr && atoi(getenv("SV_ROCTX")) != 0)
// the row-ring kernel off everywhere / its merged parity classes back on the tile kernel (row_conv.hip)
SV_KNOB_SET(sv_knob_no_rowconv, getenv("SV_NO_ROWCONV") != nullptr)
SV_KNOB_SET(sv_knob_rc_no_cls, getenv("SV_RC_NO_CLS") != nullptr)
// one problem per stride-2 parity class (conv_api.hip)
SV_KNOB_SET(sv_knob_no_cls_merge, getenv("SV_NO_CLS_MERGE") != nullptr)
// the e1 / e2 / d4 weight gradients back on the tile kernel; images per launch from which e2's pipeline takes over
SV_KNOB_SET(sv_knob_no_wgrad_e1, getenv("SV_NO_WGRAD_E1") != nullptr)
SV_KNOB_SET(sv_knob_no_wgrad_e2, getenv("SV_NO_WGRAD_E2") != nullptr)
SV_KNOB_SET(sv_knob_no_wgrad_roll, getenv("SV_NO_WGRAD_ROLL") != nullptr)
inline int sv_knob_wgrad_e2_min() { static const int v = getenv("SV_WGRAD_E2_MIN") ? atoi(getenv("SV_WGRAD_E2_MIN")) : 512; return v; }
// weight gradients kept on the main stream (layer list; nullptr: the defaults of lgvae_plan.hip), side-stream count (`dflt` when unset)
inline const char* sv_knob_wgrad_main() { static const char* v = getenv("SV_WGRAD_MAIN"); return v; }
inline int sv_knob_side_streams(int dflt) { static const char* e = getenv("SV_SIDE_STREAMS"); return e ? atoi(e) : dflt; }
// the fp32 resize adjoint as one thread per output (pointwise.hip)
SV_KNOB_SET(sv_knob_ups_bwd_plain, getenv("SV_UPS_BWD_PLAIN") != nullptr)
// class count of the polyphase-class form (conv_geom.h).  Read per call: tests/test_gpu_kernels.py switches it for the k = 4 case
inline const char* sv_knob_polyc_k() { const char* e = getenv("SV_POLYC_K"); return e ? e : "6"; }
// the polyphase-class weight gradient's fused form (polyc_wgrad.hip)
inline int sv_knob_wgrad_polyc_fused() { static const int v = getenv("SV_WGRAD_POLYC_FUSED") ? atoi(getenv("SV_WGRAD_POLYC_FUSED")) : 0; return v; }
// latent block: slab sums back in nt_slab_reduce_kernel / split-K launches on the one-slot kernel / fp32 on the im2col launches
SV_KNOB_SET(sv_knob_no_latent_fuse, getenv("SV_NO_LATENT_FUSE") != nullptr)
SV_KNOB_SET(sv_knob_no_nt_ring, getenv("SV_NO_NT_RING") != nullptr)
SV_KNOB_SET(sv_knob_no_latent_gemm_f32, getenv("SV_NO_LATENT_GEMM_F32") != nullptr)
// captures that fork to the side streams / early side work (lgvae_plan.hip; both opt-in)
SV_KNOB_SET(sv_knob_graph_side, getenv("SV_GRAPH_SIDE") != nullptr && atoi(getenv("SV_GRAPH_SIDE")) != 0)
SV_KNOB_SET(sv_knob_early_side, getenv("SV_EARLY_SIDE") != nullptr && atoi(getenv("SV_EARLY_SIDE")) != 0)
// extra streams of the SPLIT-SPAIR tape (tape.hip)
inline int sv_knob_tape_lanes() { static const int v = getenv("SV_TAPE_LANES") ? atoi(getenv("SV_TAPE_LANES")) : 1; return v; }
// fp32 conv forward: K split over workgroups up to this many 128 x 128 output tiles (conv_api.hip; 0 off)
inline int sv_knob_conv_splitk_tiles() { static const int v = getenv("SV_CONV_SPLITK_TILES") ? atoi(getenv("SV_CONV_SPLITK_TILES")) : 32; return v; }
// the pipelined whole-image-tile weight gradient off (wgrad_tile.hip)
SV_KNOB_SET(sv_knob_wt_no_pipe, getenv("SV_WT_NO_PIPE") != nullptr)
#undef SV_KNOB_SET

#ifdef SV_DEBUG_KNOBS
#define SV_TUNE_FLAG(name) (getenv(name) != nullptr)
#define SV_TUNE_INT(name, dflt) (getenv(name) ? atoi(getenv(name)) : (dflt))
#define SV_TUNE_STR(name, dflt) (getenv(name) ? (const char*)getenv(name) : (const char*)(dflt))
#else
#define SV_TUNE_FLAG(name) false
#define SV_TUNE_INT(name, dflt) (dflt)
#define SV_TUNE_STR(name, dflt) ((const char*)(dflt))
#endif

// tuning knobs that two files read: the im2col GEMM kernels instead of the LDS-tile kernels (forward / input gradient: tile_conv.hip, weight gradient:
// wgrad_tile.hip); one launch per problem instead of twin / parity-class / multi-problem launches
inline bool sv_tune_force_im2col() { static const bool v = SV_TUNE_FLAG("SV_FORCE_IM2COL"); return v; }
inline bool sv_tune_no_multi() { static const bool v = SV_TUNE_FLAG("SV_NO_MULTI"); return v; }
