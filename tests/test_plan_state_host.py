"""CPU: the dz state machine of the step plan's latent block (csrc/plan_latent.h, exported as sv_lgvae_dz_transition) against a transcription of the
four host flags it replaced.

The flags -- gz_clean, gz_zero_skipped, dz_valid, dz_slabs of struct sv_lgvae_plan -- are transcribed from csrc/lgvae_plan.hip of commit 08c7130, the
parent of the commit that introduced the state machine, branch by branch:
  :881-896    phase_forward: which range the encoders' forward zeroes and what it leaves in the flags;
  :1051-1052  phase_bwd_decoders: the re-zero of a second backward over one forward;
  :1123-1156  phase_bwd_decoders, d1's input gradient: dz_valid, and dz_slabs where the slabs are left for Sampling + KL's adjoint;
  :1168-1171  phase_bwd_encoders: the zero fill of a KL-only backward after a forward that skipped it (and :1176: the adjoint reads lat_ws_* iff dz_slabs).
Both are driven through the same event sequences; after every step the zero range issued and the buffer Sampling + KL's adjoint would read must agree.
The one intended difference: a decoders' backward that ACCUMULATES d1's input gradient into gz_* (the im2col fall-back) after a forward that skipped the
zero fill.  The flags issued no memset there (the atomics would have added to an earlier step's values; no current shape reaches it), the state machine
zeroes gz_* first."""
import ctypes as C
import itertools
import random

import pytest

ZEROED, STALE, IN_GZ, IN_SLABS = range(4)                    # DzState
ENC_FWD, DEC_BWD_SLABS, DEC_BWD_GZ, ENC_HEAD_BWD = range(4)  # DzEvent
ZERO_NONE, ZERO_GZ, ZERO_PRE_GZ = range(3)                   # DzZero: nothing / gz_x .. / pre_x .. gz_xh
NEW_PLAN = IN_GZ                                             # LatentBlock::dz of a plan that has run nothing

# one step = (event, slab_path).  slab_path matters to ENC_FWD (both split-K launches latched on latent_gemm.hip) and to DEC_BWD_GZ (1: summed from the
# slabs, which overwrites gz_*; 0: accumulated by the atomics)
STEPS = [(ENC_FWD, 0), (ENC_FWD, 1), (DEC_BWD_SLABS, 0), (DEC_BWD_GZ, 0), (DEC_BWD_GZ, 1), (ENC_HEAD_BWD, 0)]


class ParentFlags:
    """struct sv_lgvae_plan's four flags at 08c7130 (all false in a new plan, :162-166) and what each phase did with them."""

    def __init__(self, global_only=False):
        self.gz_clean = self.gz_zero_skipped = self.dz_valid = self.dz_slabs = False
        self.global_only = global_only

    def step(self, event, slab_path):
        zero = ZERO_NONE
        if event == ENC_FWD:                                  # :881-896
            if self.global_only:                              # :881-885  zero(GZ, GZ)
                zero, self.gz_clean, self.gz_zero_skipped = ZERO_GZ, True, False
            elif not slab_path:                               # :886-891  zero(PRE, GZ_XH)
                zero, self.gz_clean, self.gz_zero_skipped = ZERO_PRE_GZ, True, False
            else:                                             # :892-894
                self.gz_clean, self.gz_zero_skipped = True, True
            self.dz_slabs = self.dz_valid = False             # :896
        elif event in (DEC_BWD_SLABS, DEC_BWD_GZ):
            if not self.gz_clean:                             # :1051  zero(GZ, GZ + nd - 1)
                zero = ZERO_GZ
            self.gz_clean = False                             # :1052
            self.dz_slabs, self.dz_valid = False, True        # :1123-1124
            if event == DEC_BWD_SLABS:                        # :1150-1152; every other branch of :1125-1156 leaves dz_slabs false
                self.dz_slabs = True
        else:                                                 # :1168-1171  zero(GZ, GZ_XH)
            if not self.dz_valid and self.gz_zero_skipped:
                zero, self.gz_zero_skipped = ZERO_GZ, False
        return zero

    def adjoint_reads_slabs(self):                            # :1176  src = dz_slabs ? LAT_WS : GZ
        return self.dz_slabs


class Machine:
    def __init__(self, lib, global_only=False):
        self.lib, self.state, self.global_only = lib, NEW_PLAN, global_only

    def step(self, event, slab_path):
        nxt, zero = C.c_int32(-1), C.c_int32(-1)
        assert self.lib.sv_lgvae_dz_transition(self.state, event, slab_path, C.byref(nxt), C.byref(zero)) == 0
        assert 0 <= nxt.value <= 3 and 0 <= zero.value <= 2
        before, self.state = self.state, nxt.value
        # zero_dz of lgvae_plan.hip: a GMVae plan has neither pre_* nor an x-hat network, its whole range is gz_x
        return before, (ZERO_GZ if self.global_only and zero.value == ZERO_PRE_GZ else zero.value)

    def adjoint_reads_slabs(self):
        return self.state == IN_SLABS


def drive(lib, seq, global_only=False):
    """-> how often the one intended difference occurred; asserts agreement everywhere else"""
    old, new = ParentFlags(global_only), Machine(lib, global_only)
    hits = 0
    for k, (event, slab_path) in enumerate(seq):
        z_old = old.step(event, slab_path)
        before, z_new = new.step(event, slab_path)
        if before == STALE and event == DEC_BWD_GZ and not slab_path:
            assert (z_old, z_new) == (ZERO_NONE, ZERO_GZ), (seq, k)      # the accumulating fall-back after a skipped zero fill: zeroed now
            hits += 1
        else:
            assert z_new == z_old, (seq, k, z_old, z_new)
        assert new.adjoint_reads_slabs() == old.adjoint_reads_slabs(), (seq, k)
    return hits


@pytest.fixture(scope="module")
def lib(lib_built):
    from split_vae_amd import _lib
    return _lib.load()


def test_every_sequence_up_to_five_events_matches_the_parent_flags(lib):
    hits = n = 0
    for length in range(1, 6):
        for seq in itertools.product(STEPS, repeat=length):
            hits += drive(lib, seq)
            n += 1
    assert n == sum(6 ** k for k in range(1, 6)) and hits > 0     # (the intended difference is among them)
    # slab_path fixed over a whole sequence (a plan whose launches never / always latched): no difference at all with 0 -- Stale is never entered
    fixed0 = [s for s in STEPS if s[1] == 0]
    assert sum(drive(lib, seq) for length in range(1, 6) for seq in itertools.product(fixed0, repeat=length)) == 0
    # GMVae (global_only): its forward always zeroes gz_x, its encoder heads' phase returns before the state is read
    gm = [s for s in fixed0 if s[0] != ENC_HEAD_BWD]
    assert sum(drive(lib, seq, True) for length in range(1, 6) for seq in itertools.product(gm, repeat=length)) == 0


def test_random_long_sequences_match_the_parent_flags(lib):
    rng = random.Random(20260)
    for _ in range(500):
        drive(lib, [rng.choice(STEPS) for _ in range(20)])


def test_the_one_intended_difference_and_the_argument_checks(lib):
    nxt, zero = C.c_int32(), C.c_int32()
    assert lib.sv_lgvae_dz_transition(STALE, DEC_BWD_GZ, 0, C.byref(nxt), C.byref(zero)) == 0
    assert (nxt.value, zero.value) == (IN_GZ, ZERO_GZ)            # accumulated into a gz_* that was never cleared: cleared first
    assert lib.sv_lgvae_dz_transition(STALE, DEC_BWD_GZ, 1, C.byref(nxt), C.byref(zero)) == 0
    assert (nxt.value, zero.value) == (IN_GZ, ZERO_NONE)          # summed from the slabs: gz_* is overwritten
    assert lib.sv_lgvae_dz_transition(STALE, DEC_BWD_SLABS, 1, C.byref(nxt), C.byref(zero)) == 0
    assert (nxt.value, zero.value) == (IN_SLABS, ZERO_NONE)       # the step every default plan takes: no memset at all
    # phase_bwd_decoders issues the zero of DEC_BWD_SLABS on entry (how d1's input gradient leaves dz is known only at the end) and, where the real event's
    # zero differs, that one before the accumulating launch: the two agree in every state but the one case, so the composition is the single transition
    for state in range(4):
        assert lib.sv_lgvae_dz_transition(state, DEC_BWD_SLABS, 1, C.byref(nxt), C.byref(zero)) == 0
        entry = zero.value
        for slab_path in (0, 1):
            assert lib.sv_lgvae_dz_transition(state, DEC_BWD_GZ, slab_path, C.byref(nxt), C.byref(zero)) == 0
            assert (zero.value == entry) == ((state, slab_path) != (STALE, 0)), (state, slab_path)
    for bad in ((-1, 0), (4, 0), (0, -1), (0, 4)):
        assert lib.sv_lgvae_dz_transition(bad[0], bad[1], 0, C.byref(nxt), C.byref(zero)) != 0
    assert lib.sv_lgvae_dz_transition(0, 0, 0, None, C.byref(zero)) != 0
    assert lib.sv_lgvae_dz_transition(0, 0, 0, C.byref(nxt), None) != 0
