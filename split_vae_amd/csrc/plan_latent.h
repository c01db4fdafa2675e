// Host state of the step plan's latent block: where dL/dz lives between the phases of a step, as a state machine that can be checked without a device
// (no HIP in this header; tests/test_plan_state_host.py drives dz_transition through sv_lgvae_dz_transition).
//
// dL/dz of the two decoders is written by d1's input gradient (phase_bwd_decoders) and read by the adjoint of Sampling + KL (phase_bwd_encoders), or by
// the caller's encoder (SPLIT-GMVAE, GMVae: gz_x).  The split-K launch that writes it has two forms:
//   - latent_gemm.hip: K-slice slabs in lat_ws_*, either left there (Sampling + KL's adjoint sums them itself: one launch less) or summed into gz_* by a
//     reduce that OVERWRITES gz_*;
//   - the im2col kernel's split-K atomics, which ACCUMULATE into gz_*: gz_* must be zero before.
// The heads' forward has the same two forms over pre_*, so one memset (pre_ .. gz_xh) serves both accumulating forms -- and is dropped once both launches of
// a plan have gone through latent_gemm.hip (slab_path).
#pragma once
#include <stdint.h>

enum class DzState : int32_t {
  Zeroed = 0,    // gz_* (and pre_*) were zero-filled since the last writer: an accumulating input gradient may run
  Stale = 1,     // the encoders' forward skipped the zero fill (slab_path: nothing accumulates): gz_* holds an earlier step's values, dL/dz is defined as 0
  InGz = 2,      // dL/dz is summed in gz_*  (also a new plan's state: gz_* holds nothing anyone may add to)
  InSlabs = 3    // dL/dz is the unsummed K-slice slabs in lat_ws_*
};
enum class DzEvent : int32_t {
  EncFwd = 0,       // encoders' forward.  slab_path: both split-K launches of this plan go through latent_gemm.hip
  DecBwdSlabs = 1,  // decoders' backward, d1's input gradient left as slabs
  DecBwdGz = 2,     // decoders' backward, d1's input gradient in gz_*.  slab_path: summed from slabs (overwrites); else accumulated by atomics
  EncHeadBwd = 3    // encoder heads' backward (reads dL/dz)
};
enum class DzZero : int32_t { None = 0, Gz = 1, PreGz = 2 };     // the buffer range to zero BEFORE the event's launches: gz_x .., or pre_x .. gz_xh
struct DzStep { DzState next; DzZero zero; };

inline DzStep dz_transition(DzState s, DzEvent e, bool slab_path) {
  // a decoders' backward already wrote dL/dz since the last forward: a second backward over the same forward re-zeroes the accumulators
  const bool used = s == DzState::InGz || s == DzState::InSlabs;
  switch (e) {
    case DzEvent::EncFwd:
      if (slab_path) return {DzState::Stale, DzZero::None};
      return {DzState::Zeroed, DzZero::PreGz};
    case DzEvent::DecBwdSlabs:
      return {DzState::InSlabs, used ? DzZero::Gz : DzZero::None};
    case DzEvent::DecBwdGz:
      // Stale and accumulating: the forward trusted that nothing accumulates, and the launch fell back to the atomics after all.  No current shape reaches
      // it (Stale needs d1's latent_gemm launch to have succeeded once, and a plan's shapes are fixed), but gz_* was never cleared: clear it.
      if (s == DzState::Stale && !slab_path) return {DzState::InGz, DzZero::Gz};
      return {DzState::InGz, used ? DzZero::Gz : DzZero::None};
    case DzEvent::EncHeadBwd:
      // KL terms only (no decoders' backward since a forward that skipped the zero fill): dL/dz = 0
      if (s == DzState::Stale) return {DzState::Zeroed, DzZero::Gz};
      return {s, DzZero::None};
  }
  return {s, DzZero::None};
}

// the latent block's per-plan host state: dz, what was latched about the two split-K launches, and their K-slice geometry
struct LatentBlock {
  DzState dz = DzState::InGz;
  // the heads' forward / d1's input gradient of this plan run on latent_gemm.hip (shapes are fixed per plan): latched after the first successful launch
  bool head_ok = false, d1_ok = false;
  // K slices and floats between slabs of those two launches per network (x, x-hat), fixed when the plan is created: lat_ws_* is sized from them
  int head_S[2] = {0, 0}, d1_S[2] = {0, 0};
  int64_t head_stride[2] = {0, 0}, d1_stride[2] = {0, 0};
};
