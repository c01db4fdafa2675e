"""GPU: the sv_conv2d_* ABI (include/splitvae.h K3-K10) called with raw descriptors, against fp64 F.conv2d on the same rounded operands,
over every dispatch form the API routes a descriptor to.  CASES names, per descriptor, the form each call is expected to take
(SV_TRACE_DISPATCH's "sv_dispatch <op> <form>" names); test_every_form_is_reached_and_every_case_takes_its_form checks the table
against a traced run in a child process (the knob is read once per process).

Beyond the values, every call checks the header's buffer contract: write-only outputs are prefilled with NaN and must come back with
their pad channels [C, r8(C)) exactly zero and the channels beyond r8(C) untouched or zero; accumulators (dw, dbias, the fp32-atomic dx)
are prefilled with a non-zero pattern and must come back as pattern + gradient; refused calls leave every buffer as it was.

Every case runs its whole call sequence on two input families (tests/conv_ref.py).  Gaussian: the tolerances below, and on top of them the
derived per-element `gauss_bound` against the reference that rounds where the form rounds.  Integer: small integer operands, for which fp32
accumulation is exact in any order -- real channels are compared BIT FOR BIT with the float64 reference cast once to the output type,
accumulators with prefill + gradient (the sign of a zero aside: a sum of signed zeros has no order-independent sign).  BOUND_NOT_BITS names
the forms that round an intermediate the lemma does not cover; they are compared by the bound, on both families."""
import ctypes as C
import os
import subprocess
import sys
from collections import namedtuple

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import torch_ref

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

# as tests/test_gpu_kernels.py: fp32 = exact-f32 MFMA, only the summation order differs; bf16 = rounded operands, fp32 accumulation
F32_RTOL, F32_ATOL = 1e-4, 1e-5
BF16_RTOL, BF16_ATOL = 3e-2, 3e-2

SV_E_BADARG, SV_E_UNSUPPORTED = -1, -2

# every form SV_TRACE_DISPATCH can name for a successful call (plus lowres_unsupported: the refused fused input gradient)
FORMS = {
    "fwd": {"row", "tile", "tile_packx", "tile_s2d3", "im2col", "im2col_small", "dense_splitk", "conv_splitk", "poly_ws", "poly_atomic",
            "polyc", "polyc_direct"},
    "dgrad": {"merged", "multi_class", "per_class", "atomic_splitk"},
    "dgrad_lowres": {"lowres_row", "lowres_polyd", "lowres_unsupported"},
    "wgrad": {"wgrad_tile", "wgrad_tile_f32", "wgrad_roll", "wgrad_e1", "wgrad_e2", "polyc_wgrad", "poly_wgrad", "wgrad_im2col"},
    "wgrad_poly": {"wgrad_tile", "wgrad_p5"},
}

# what a call must return: the float64 reference with the form's rounding points, |a| . |b| of the same contraction, its length n, the folds S on top
# of it (gauss_bound), whether the output is typed bf16, whether the form rounds mid-chain, and a bound added on top (a composed first stage)
Exp = namedtuple("Exp", "ref ab n S out_bf16 two_stage extra")
# forms that contract the LOW-RES tensor with composite polyphase weights (combined in fp32, then converted once): no staged hi-res pixel
COMPOSITE = {"poly_ws", "poly_atomic", "polyc", "lowres_polyd", "polyc_wgrad", "poly_wgrad", "wgrad_p5", "wgrad_poly"}
POLY_HEAD_FWD = {"poly_ws", "poly_atomic"}
SPLIT_FORMS = {"dense_splitk", "conv_splitk", "atomic_splitk"}
# S of gauss_bound.  A composite weight is at most 3 x 3 products cy cx w, two roundings each, summed (9 more), its border terms fold twice more and
# the staged lines carry their lerp: 32 covers it.  Split-K forwards, the atomic input gradient and the weight-gradient slabs / m-split atomics fold at
# most 64 partial sums onto an element (svg_choose_splitk: at most 512 workgroups over at least 8 tiles; SV_POLY_WGRAD_NWG slabs go through a tree).
S_COMPOSITE, S_SPLIT = 32, 64
# Forms compared by the bound and not by bits on the integer family: each rounds an intermediate whose value the lemma does not cover.
BOUND_NOT_BITS = {
    ("dgrad_lowres", "lowres_row", "bf16"): "the row-ring kernel's fused epilogue rounds the hi-res gradient to bf16 before the resize adjoint "
                                            "(adj2x_row_bf16 reads packed bf16): a sum of up to 36 x 64 integer products need not fit 8 bits",
    ("dgrad + sv_upsample2x_bwd", "per_class", "bf16"): "dgrad stores the hi-res gradient as bf16, sv_upsample2x_bwd reads it: the same rounding point",
}

# name, B, H, W, Cin, Cout, KH, KW, stride, act, dtype, ldx (0: r8(Cin)), ldy (0: r8(Cout), or Cout with y_f32), y_f32, ups_in,
# P (distinct images, 0: B -- larger batches repeat P images at power-of-two scales), bias, fold (the weight gradient with a workspace runs the
# x-packed form, whose fold onto the HWIO gradient adds atomically: not bitwise reproducible, header), forms.
# forms: call -> form (or (default mode, deterministic mode)); "unsupported": SV_E_UNSUPPORTED.  Calls: fwd (no workspace), fwd_ws (exact
# workspace; default: as fwd), dgrad (dgrad_atomic is always atomic_splitk), lowres / lowres_ws (ups_in layers), wgrad (no workspace),
# wgrad_ws, wgrad_poly (bf16 polyphase head).
Case = namedtuple("Case", "name B H W Cin Cout KH KW s act dt ldx ldy yf32 ups P bias fold forms")
_F = Case._fields


def case(name, B, H, W, Cin, Cout, KH, KW, s, act, dt, ldx=0, ldy=0, yf32=0, ups=0, P=0, bias=True, fold=0, **forms):
    return Case(name, B, H, W, Cin, Cout, KH, KW, s, act, dt, ldx, ldy, yf32, ups, P, bias, fold, forms)


CASES = [
    # ---- forward: LDS-tile kernel on non-square power-of-two grids, every channel count of the table, both dtypes
    case("tile_16x32_k3_f32", 3, 16, 32, 12, 16, 3, 3, 1, "relu", "f32", fwd="tile", dgrad="per_class", wgrad="wgrad_im2col", wgrad_ws="wgrad_im2col"),
    case("tile_64x16_k4s2_c10_bf16", 2, 64, 16, 5, 10, 4, 4, 2, None, "bf16", fwd="tile", dgrad="multi_class", wgrad="wgrad_im2col", wgrad_ws="wgrad_im2col"),
    case("tile_8x32_k5x3_c6_f32", 5, 8, 32, 30, 6, 5, 3, 1, "relu", "f32", fwd="tile", dgrad="per_class", wgrad="wgrad_im2col", wgrad_ws="wgrad_im2col"),
    case("tile_16x16_k3x5s2_c4_bf16", 3, 16, 16, 3, 4, 3, 5, 2, "relu", "bf16", fwd="tile", dgrad="multi_class", wgrad="wgrad_im2col", wgrad_ws="wgrad_im2col"),
    case("tile_16x16_k1_c1_f32", 2, 16, 16, 1, 1, 1, 1, 1, None, "f32", bias=False, fwd="tile", dgrad="per_class", wgrad="wgrad_im2col", wgrad_ws="wgrad_im2col"),
    case("tile_16x16_k2_c3_bf16", 1, 16, 16, 5, 3, 2, 2, 1, "relu", "bf16", fwd="tile", dgrad="per_class", wgrad="wgrad_im2col", wgrad_ws="wgrad_im2col"),
    case("tile_32x8_k6_c1_bf16", 2, 32, 8, 60, 1, 6, 6, 1, None, "bf16", fwd="tile", dgrad="per_class", wgrad="wgrad_im2col", wgrad_ws="wgrad_im2col"),
    case("tile_16x16_k4_c3_f32", 2, 16, 16, 12, 3, 4, 4, 1, "relu", "f32", fwd="tile", dgrad="per_class", wgrad="wgrad_im2col", wgrad_ws="wgrad_im2col"),
    case("tile_16x16_k3_c4_f32", 2, 16, 16, 30, 4, 3, 3, 1, None, "f32", fwd="tile", dgrad="per_class", wgrad="wgrad_im2col", wgrad_ws="wgrad_tile_f32"),
    case("tile_16x16_k5_c6_bf16", 2, 16, 16, 12, 6, 5, 5, 1, "relu", "bf16", fwd="tile", dgrad="per_class", wgrad="wgrad_im2col", wgrad_ws="wgrad_im2col"),
    # several images per tile (8 x 8 grids) and a batch one past the images per tile
    case("tile_8x8_pack_b5_f32", 5, 8, 8, 60, 32, 2, 2, 1, "relu", "f32", fwd="tile", dgrad="per_class", wgrad="wgrad_im2col", wgrad_ws="wgrad_im2col"),
    case("tile_8x8_pack_b3_bf16", 3, 8, 8, 30, 32, 3, 3, 1, "relu", "bf16", fwd="tile", dgrad="per_class", wgrad="wgrad_im2col", wgrad_ws="wgrad_im2col"),
    # pitches wider than r8(C): ldx > r8(Cin), ldy > r8(Cout)
    case("pitch_wide_c6_f32", 4, 16, 16, 3, 6, 3, 3, 1, "relu", "f32", ldx=16, ldy=16, fwd="tile", dgrad="per_class", wgrad="wgrad_im2col", wgrad_ws="wgrad_im2col"),
    case("pitch_wide_c12_bf16", 3, 16, 16, 5, 12, 3, 3, 1, None, "bf16", ldx=24, ldy=24, fwd="tile", dgrad="per_class", wgrad="wgrad_im2col", wgrad_ws="wgrad_im2col"),
    # fp32 output heads: ldy == Cout and ldy > Cout
    case("yf32_eq_c6", 2, 16, 16, 16, 6, 3, 3, 1, None, "f32", yf32=1, fwd="tile", dgrad="per_class", wgrad="wgrad_im2col", wgrad_ws="wgrad_tile_f32"),
    case("yf32_gt_c6", 2, 16, 16, 16, 6, 3, 3, 1, None, "f32", ldy=8, yf32=1, fwd="tile", dgrad="per_class", wgrad="wgrad_im2col", wgrad_ws="wgrad_tile_f32"),
    case("yf32_gt_c6_bf16_12x20", 2, 12, 20, 16, 6, 3, 3, 1, None, "bf16", ldy=16, yf32=1, fwd="im2col", dgrad="per_class", wgrad="wgrad_im2col", wgrad_ws="wgrad_im2col"),
    # ---- non-power-of-two extents: im2col kernels (cfg 4 = 64 x 32 tiles for small 32-column launches)
    case("im2col_12x20_c32_f32", 2, 12, 20, 60, 32, 3, 3, 1, "relu", "f32", fwd="im2col_small", dgrad="per_class", wgrad="wgrad_im2col", wgrad_ws="wgrad_im2col"),
    case("im2col_12x20_k2_c16_bf16", 1, 12, 20, 1, 16, 2, 2, 1, None, "bf16", fwd="im2col", dgrad="per_class", wgrad="wgrad_im2col", wgrad_ws="wgrad_im2col"),
    case("im2col_24x12_s2_c3_bf16", 2, 24, 12, 12, 3, 4, 4, 2, "relu", "bf16", fwd="im2col", dgrad="multi_class", wgrad="wgrad_im2col", wgrad_ws="wgrad_im2col"),
    case("im2col_24x12_s3_c10_f32", 3, 24, 12, 5, 10, 6, 6, 3, None, "f32", fwd="im2col", dgrad="per_class", wgrad="wgrad_im2col", wgrad_ws="wgrad_im2col"),
    case("im2col_16x16_c48_f32", 2, 16, 16, 12, 48, 3, 3, 1, "relu", "f32", fwd="im2col", dgrad="unsupported", wgrad="wgrad_im2col", wgrad_ws="wgrad_im2col"),
    # ---- split-K forwards (default mode only: SV_DETERMINISTIC keeps one workgroup per output tile)
    case("dense_splitk_f32", 5, 1, 1, 256, 48, 1, 1, 1, None, "f32", yf32=1, fwd=("dense_splitk", "im2col"), dgrad="unsupported", wgrad="wgrad_im2col", wgrad_ws="wgrad_im2col"),
    case("dense_splitk_bf16", 3, 1, 1, 256, 32, 1, 1, 1, None, "bf16", yf32=1, fwd=("dense_splitk", "im2col_small"), dgrad="per_class", wgrad="wgrad_im2col", wgrad_ws="wgrad_im2col"),
    case("dense_relu_c1_f32", 3, 1, 1, 60, 1, 1, 1, 1, "relu", "f32", yf32=1, fwd="im2col", dgrad="per_class", wgrad="wgrad_im2col", wgrad_ws="wgrad_im2col"),
    case("conv_splitk_8x8_k4s2_f32", 3, 8, 8, 60, 32, 4, 4, 2, None, "f32", fwd=("conv_splitk", "tile"), dgrad="multi_class", wgrad="wgrad_im2col", wgrad_ws="wgrad_im2col"),
    case("conv_splitk_out_k3_f32", 3, 8, 8, 60, 32, 3, 3, 2, None, "f32", fwd="tile", dgrad="multi_class", wgrad="wgrad_im2col", wgrad_ws="wgrad_im2col"),
    # ---- stride-2 input gradients: one merged problem (classes share one dY window: k 6) or the classes per launch (k 4)
    case("merged_16x16_k6s2_f32", 3, 16, 16, 16, 32, 6, 6, 2, "relu", "f32", fwd="tile", dgrad="merged", wgrad="wgrad_im2col", wgrad_ws="wgrad_im2col"),
    case("multi_16x32_k4s2_f32", 3, 16, 32, 16, 32, 4, 4, 2, "relu", "f32", fwd="tile", dgrad="multi_class", wgrad="wgrad_im2col", wgrad_ws="wgrad_im2col"),
    # ---- the space-to-depth first layer (fp32, Cin 3, k 6, stride 2, Cout % 16 == 0) and just outside it
    case("s2d3_16x32_f32", 2, 16, 32, 3, 16, 6, 6, 2, "relu", "f32", fwd="tile_s2d3", dgrad="multi_class", wgrad="wgrad_im2col", wgrad_ws="wgrad_im2col"),
    case("s2d3_out_c24_f32", 2, 16, 32, 3, 24, 6, 6, 2, "relu", "f32", fwd="im2col", dgrad="unsupported", wgrad="wgrad_im2col", wgrad_ws="wgrad_im2col"),
    # ---- x-packed thin head (stride 1, Cout <= 8 even, y_f32, ldy == Cout, W >= 32) and just outside (W = 16: yf32_eq_c6)
    case("packx_16x32_k6_f32", 2, 16, 32, 12, 6, 6, 6, 1, None, "f32", yf32=1, fold=1, fwd="tile_packx", dgrad="per_class", wgrad="wgrad_tile_f32", wgrad_ws="wgrad_tile_f32"),
    case("packx_16x32_k5_bf16", 3, 16, 32, 30, 4, 5, 5, 1, None, "bf16", yf32=1, fwd="tile_packx", dgrad="per_class", wgrad="wgrad_im2col", wgrad_ws="wgrad_im2col"),
    # ---- model layers on the row-ring kernel and the weight-gradient forms of the model's layers (batches repeat 4 images)
    case("row_e2_bf16", 2, 32, 32, 32, 64, 6, 6, 2, "relu", "bf16", fwd="row", dgrad="merged", wgrad="wgrad_tile", wgrad_ws="wgrad_tile"),
    case("e2_b512_bf16", 512, 32, 32, 32, 64, 6, 6, 2, "relu", "bf16", P=4, fwd="row", dgrad="merged", wgrad="wgrad_tile", wgrad_ws="wgrad_e2"),
    case("e1_b256_bf16", 256, 64, 64, 3, 32, 6, 6, 2, "relu", "bf16", P=4, fwd="row", dgrad="multi_class", wgrad="wgrad_tile", wgrad_ws="wgrad_e1"),
    case("d4_ups_bf16", 2, 32, 32, 64, 32, 6, 6, 1, "relu", "bf16", ups=1, fwd="row", dgrad="per_class", lowres="lowres_row",
         wgrad="wgrad_tile", wgrad_ws="wgrad_roll"),
    # ---- upsample -> conv at off-model geometries
    case("ups_16x32_k3_c10_bf16", 3, 16, 32, 12, 10, 3, 3, 1, "relu", "bf16", ups=1, fwd="tile", dgrad="per_class", lowres="lowres_unsupported",
         wgrad="unsupported", wgrad_ws="unsupported"),
    case("ups_8x8_k4_c16_f32", 2, 8, 8, 30, 16, 4, 4, 1, None, "f32", ups=1, fwd="tile", dgrad="per_class", lowres="lowres_unsupported",
         wgrad="unsupported", wgrad_ws="unsupported"),
    # ---- polyphase head (ups_in, 6 x 6, Cin 32, Cout <= 8, y_f32): border terms through the workspace or by atomics; its weight gradient
    # (the polyphase weight gradient of the bf16 head needs hi-res extents that are multiples of 32: its frame terms were missing at 16 x 32)
    case("poly_16x32_bf16", 3, 16, 32, 32, 6, 6, 6, 1, None, "bf16", yf32=1, ups=1, fold=1, fwd="poly_atomic", fwd_ws="poly_ws", dgrad="per_class",
         lowres="lowres_unsupported", wgrad="wgrad_tile", wgrad_ws="wgrad_tile"),
    case("poly_32x64_bf16", 2, 32, 64, 32, 6, 6, 6, 1, None, "bf16", yf32=1, ups=1, fold=1, fwd="poly_atomic", fwd_ws="poly_ws", dgrad="per_class",
         lowres="lowres_row", wgrad="wgrad_tile", wgrad_ws="wgrad_tile", wgrad_poly="wgrad_tile"),
    case("poly_16x32_f32", 3, 16, 32, 32, 6, 6, 6, 1, None, "f32", yf32=1, ups=1, fwd="poly_atomic", fwd_ws="poly_ws", dgrad="per_class",
         lowres="lowres_unsupported", wgrad="wgrad_tile_f32", wgrad_ws="poly_wgrad"),
    case("poly_32x32_bf16", 3, 32, 32, 32, 6, 6, 6, 1, None, "bf16", yf32=1, ups=1, fold=1, fwd="poly_atomic", fwd_ws="poly_ws", dgrad="per_class",
         lowres="lowres_unsupported", wgrad="wgrad_tile", wgrad_ws="wgrad_tile", wgrad_poly="wgrad_tile"),
    case("poly_p5_b128_bf16", 128, 64, 64, 32, 6, 6, 6, 1, None, "bf16", yf32=1, ups=1, P=4, fold=1, fwd="poly_atomic", fwd_ws="poly_ws",
         dgrad="per_class", lowres="lowres_row", wgrad="wgrad_tile", wgrad_ws="wgrad_tile", wgrad_poly="wgrad_p5"),
    case("poly_polyd_32x32_f32", 2, 32, 32, 32, 6, 6, 6, 1, None, "f32", yf32=1, ups=1, fwd="poly_atomic", fwd_ws="poly_ws", dgrad="per_class",
         lowres="lowres_unsupported", lowres_ws="lowres_polyd", wgrad="wgrad_tile_f32", wgrad_ws="poly_wgrad"),
    case("poly_out_16x16_bf16", 2, 16, 16, 32, 6, 6, 6, 1, None, "bf16", yf32=1, ups=1, fwd="tile", dgrad="per_class",
         lowres="lowres_unsupported", wgrad="wgrad_tile", wgrad_ws="wgrad_tile"),
    # ---- per-class polyphase (fp32 ups_in 6 x 6, Cout 32, Cin 32 / 64): the class form with a workspace, the direct form without
    case("polyc_16x16_f32", 2, 16, 16, 32, 32, 6, 6, 1, "relu", "f32", ups=1, fwd="polyc_direct", fwd_ws="polyc", dgrad="per_class",
         lowres="lowres_unsupported", wgrad="wgrad_tile_f32", wgrad_ws="polyc_wgrad"),
    case("polyc_16x32_c64_f32", 3, 16, 32, 64, 32, 6, 6, 1, None, "f32", ups=1, fwd="polyc_direct", fwd_ws="polyc", dgrad="per_class",
         lowres="lowres_unsupported", wgrad="wgrad_tile_f32", wgrad_ws="polyc_wgrad"),
    case("polyc_out_8x8_f32", 2, 8, 8, 32, 32, 6, 6, 1, "relu", "f32", ups=1, fwd="tile", dgrad="per_class",
         lowres="lowres_unsupported", wgrad="wgrad_tile_f32", wgrad_ws="wgrad_tile_f32"),
    case("polyd_32x32_f32", 2, 32, 32, 32, 32, 6, 6, 1, "relu", "f32", ups=1, fwd="polyc_direct", fwd_ws="polyc", dgrad="per_class",
         lowres="lowres_unsupported", lowres_ws="lowres_polyd", wgrad="wgrad_tile_f32", wgrad_ws="polyc_wgrad"),
]


def _r8(v):
    return (v + 7) // 8 * 8


def _tdt(c):
    return torch.float32 if c.dt == "f32" else torch.bfloat16


def _geom(c):
    ldx = c.ldx or _r8(c.Cin)
    ldy = c.ldy or (c.Cout if c.yf32 else _r8(c.Cout))
    OH, OW = -(-c.H // c.s), -(-c.W // c.s)
    hin, win = (c.H // 2, c.W // 2) if c.ups else (c.H, c.W)
    return ldx, ldy, OH, OW, hin, win


def _desc(c):
    from split_vae_amd import _lib
    ldx, ldy, *_ = _geom(c)
    return _lib.ConvDesc(c.B, c.H, c.W, c.Cin, c.Cout, c.KH, c.KW, c.s, 1 if c.act == "relu" else 0,
                         _lib.SV_F32 if c.dt == "f32" else _lib.SV_BF16, ldx, ldy, c.yf32, c.ups)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _nan(shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def _pattern(shape):
    """accumulator prefill: a non-zero pattern exact in fp32"""
    n = int(np.prod(shape))
    return ((torch.arange(n, dtype=torch.float32) % 7 - 3) * 0.125).reshape(shape).cuda()


class Layer:
    """one case: seeded operands (P distinct images; image b = scale_b * image b % P, scale_b a power of two so that rounding commutes
    with it), device tensors, prepared weights and the fp64 references"""

    SCALES = R.SCALES

    def __init__(self, c, refs=True, family="gauss"):
        from split_vae_amd import _lib
        self.c, self.lib, self.d = c, _lib.load(), _desc(c)
        self.ldx, self.ldy, self.OH, self.OW, self.hin, self.win = _geom(c)
        self.gdy = _r8(c.Cout)
        dt = _tdt(c)
        self.family, self.ops = family, R.operands(c, family)       # (the Gaussian family: the draws this test always made)
        self.ratios = {}                                            # what -> worst error / bound of the comparisons by gauss_bound
        self._exp = {}
        X, DY, M, ML = (self.ops[k] for k in ("X", "DY", "M", "ML"))
        self.w, self.bias, self.pidx, sidx = (self.ops[k] for k in ("w", "bias", "pidx", "sidx"))
        sc = torch.tensor(self.SCALES, dtype=torch.float32)[sidx]

        def dev(t, ld, scale=None):
            v = t[self.pidx].float()
            if scale is not None:
                v = v * scale.view(-1, 1, 1, 1)
            out = torch.zeros(v.shape[:-1] + (ld,), dtype=dt)
            out[..., :v.shape[-1]] = v.to(dt)
            return out.cuda()

        self.x = dev(X, self.ldx, sc)
        self.dy = dev(DY, self.gdy)
        self.mask = dev(M, self.ldx)
        self.mask_lo = dev(ML, self.ldx) if c.ups else None
        self.w_dev = self.w.cuda()
        self.b_dev = self.bias.cuda() if c.bias else None
        nf = self.lib.sv_conv2d_wprep_elems(C.byref(self.d), 0)
        nd = self.lib.sv_conv2d_wprep_elems(C.byref(self.d), 1)
        assert nf > 0 and nd > 0, c.name
        self.wf = torch.empty((nf,), dtype=dt, device="cuda")
        self.wd = torch.empty((nd,), dtype=dt, device="cuda")
        assert self.lib.sv_conv2d_prep_weights(C.byref(self.d), _p(self.w_dev), _p(self.wf), _p(self.wd), _st()) == 0
        self.rtol, self.atol = (F32_RTOL, F32_ATOL) if c.dt == "f32" else (BF16_RTOL, BF16_ATOL)
        if refs:
            self._refs(X, DY, M, ML, sidx, dt)                      # (autograd's references: what the blanket tolerances of the Gaussian pass compare with)

    def _refs(self, X, DY, M, ML, sidx, dt):
        c = self.c
        keys = sorted(set(zip(self.pidx.tolist(), sidx.tolist())))
        kidx = {k: i for i, k in enumerate(keys)}
        self.uidx = torch.tensor([kidx[k] for k in zip(self.pidx.tolist(), sidx.tolist())])
        cnt = torch.bincount(self.uidx, minlength=len(keys)).double()
        xu = torch.stack([X[p].double() * self.SCALES[s] for p, s in keys]).requires_grad_(True)
        wr = self.w.to(dt).double().requires_grad_(True)
        br = self.bias.double().requires_grad_(True) if c.bias else None
        up = lambda t: torch_ref.resize_bilinear_2x(t) if c.ups else t
        # (CPU autograd refuses a one-filter weight gradient -- "grad_weight must be contiguous": a zero second filter, sliced off)
        one = lambda t: torch.cat([t, torch.zeros_like(t)], -1) if c.Cout == 1 else t
        conv = lambda v, w, b: torch_ref.conv2d_same(v, one(w), None if b is None else one(b), c.s, None)[..., :c.Cout]
        pre = conv(up(xu), wr, br)
        self.y_ref = (F.relu(pre) if c.act == "relu" else pre).detach()
        dyu = torch.stack([DY[p].double() for p, _ in keys])
        pre.backward(dyu * cnt.view(-1, 1, 1, 1))                   # sum over the batch: each distinct image as often as it occurs
        self.dw_ref, self.db_ref = wr.grad, (br.grad if c.bias else None)
        # input gradients (independent of x): per distinct dY image, at the conv's input and (ups_in) at the low-res tensor
        z = torch.zeros(X.shape[0], self.hin, self.win, c.Cin, dtype=torch.float64, requires_grad=True)
        zin = up(z)
        zin.retain_grad()
        conv(zin, wr.detach(), None).backward(DY.double())
        self.dx_ref = zin.grad
        self.dxlo_ref = z.grad if c.ups else None
        self.M, self.ML = M, ML

    # ---------------------------------------------------------------- checks
    # ---------------------------------------------------------------- what a call must return (tests/conv_ref.py)
    def expect(self, key, form=None, mask=None):
        """Exp of one call: key y | dx | dxlo | dw | db, form: the dispatch form the call takes (which rounding points the reference takes)"""
        c, ops, dt = self.c, self.ops, _tdt(self.c)
        composite = form in COMPOSITE
        # the hi-res gradient is rounded to bf16 before the resize adjoint: the forms of BOUND_NOT_BITS, and only those
        two_stage = key == "dxlo" and any((op, form, c.dt) in BOUND_NOT_BITS for op in ("dgrad_lowres", "dgrad + sv_upsample2x_bwd"))
        k = (key, composite, form in POLY_HEAD_FWD, mask, two_stage)
        if k in self._exp:
            return self._exp[k]
        keys, uidx, count, _ = R.unique_images(ops)
        xu, wr = R.x_unique(ops), R.rnd(ops["w"], dt)
        b = None if ops["bias"] is None else ops["bias"].double()
        DY = ops["DY"].double()
        stage = None if composite else dt                # the polyphase forms read the low-res tensor: no staged hi-res pixel
        S = S_COMPOSITE if composite else S_SPLIT if form in SPLIT_FORMS else 0
        extra = None
        out_bf16 = c.dt == "bf16" and not (key == "y" and c.yf32) and key in ("y", "dx", "dxlo")
        if key == "y":
            if form in POLY_HEAD_FWD and c.dt == "bf16":
                ref = R.poly_head_fwd(xu, ops["w"], b, dt)
            else:
                ref = R.conv(xu, wr, b, c.s, c.act, bool(c.ups), stage)
            if composite:                                # (the border terms are added and taken out again: conv_ref.ab_fwd_composite)
                ab = R.ab_fwd_composite(xu.abs(), wr.abs()) + (0.0 if b is None else b.abs())
            else:
                ab = R.conv(xu.abs(), wr.abs(), None if b is None else b.abs(), c.s, None, bool(c.ups))
            ref, ab, n = ref[uidx], ab[uidx], c.KH * c.KW * c.Cin
        elif key == "dx":
            ref, ab = R.dgrad(DY, wr, c.s, c.H, c.W), R.dgrad(DY.abs(), wr.abs(), c.s, c.H, c.W)
            if mask == "hi":
                ref = R.gate(ref, ops["M"])
            ref, ab, n = ref[self.pidx], ab[self.pidx], -(-c.KH // c.s) * -(-c.KW // c.s) * c.Cout
        elif key == "dxlo":
            g_hi = R.dgrad(DY, wr, 1, c.H, c.W)
            ab1 = R.dgrad(DY.abs(), wr.abs(), 1, c.H, c.W)
            if two_stage and self.family == "int":
                # (exact operands: the kernel's fp32 value is g_hi itself, so its rounding is this one, and the bound is the second stage's)
                mid = R.rnd(g_hi, dt)
                ref, ab, n = R.gate(R.resize2x_adjoint(mid), ops["ML"]), R.resize2x_adjoint(mid.abs()), 16
            elif two_stage:
                # the two stages composed and their bounds added: the first stage's bound and the rounding of ITS result (2^-8 |g|) travel through the adjoint
                ref = R.gate(R.resize2x_adjoint(g_hi), ops["ML"])
                e1 = R.gauss_bound(ab1, c.KH * c.KW * c.Cout) + 2.0 ** -8 * g_hi.abs()
                ab, n = R.resize2x_adjoint(g_hi.abs() + e1), 16
                extra = R.resize2x_adjoint(e1)[self.pidx]
            else:
                ab = R.ab_lowres_composite(DY.abs(), wr.abs(), c.H, c.W) if composite else R.resize2x_adjoint(ab1)
                ref, n = R.gate(R.resize2x_adjoint(g_hi), ops["ML"]), c.KH * c.KW * c.Cout + 16
            ref, ab = ref[self.pidx], ab[self.pidx]
        else:
            dyu = torch.stack([DY[p] for p, _ in keys])
            dw, db = R.wgrad(xu, dyu, c.KH, c.KW, c.s, bool(c.ups), stage, count)
            aw, ab_ = R.wgrad(xu.abs(), dyu.abs(), c.KH, c.KW, c.s, bool(c.ups), None, count)
            if composite:
                aw = R.ab_wgrad_composite(xu.abs(), dyu.abs(), c.KH, c.KW, count)
            ref, ab, n = (dw, aw, c.B * self.OH * self.OW) if key == "dw" else (db, ab_, c.B * self.OH * self.OW)
            S = max(S, S_SPLIT)                          # slabs / m-split atomics of the weight-gradient kernels
        e = Exp(ref, ab, n, S, out_bf16, two_stage, extra)
        self._exp[k] = e
        return e

    def judge(self, g, e, what, prefill=None):
        """g: the real channels as float64 (accumulators: what came back); e: Exp.  Integer family: bit for bit (BOUND_NOT_BITS forms: the bound);
        Gaussian family: gauss_bound."""
        out_dt = torch.bfloat16 if e.out_bf16 else torch.float32
        want = e.ref if prefill is None else e.ref + prefill
        ab = e.ab if prefill is None else e.ab + prefill.abs()
        if self.family == "int" and not e.two_stage:
            w, h = want.to(out_dt) + 0.0, g.to(out_dt) + 0.0                 # (+ 0.0: -0 -> +0)
            bad = _bits(w) != _bits(h)
            assert not bool(bad.any()), (f"{self.c.name} {what}: {int(bad.sum())} of {bad.numel()} elements differ from the exact result, first at "
                                         f"{tuple(bad.nonzero()[0].tolist())}: got {float(h[tuple(bad.nonzero()[0])])}, exact {float(w[tuple(bad.nonzero()[0])])}")
            return
        bound = R.gauss_bound(ab, e.n, S=e.S + (1 if prefill is not None else 0), ref=want, bf16_out=e.out_bf16)
        if e.extra is not None:
            bound = bound + e.extra
        err = (g - want).abs()
        ratio = float((err / bound.clamp_min(1e-300)).max())
        self.ratios[what] = max(self.ratios.get(what, 0.0), ratio)
        print(f"conv_api {self.c.name} {self.family} {what}: worst error / bound = {ratio:.3f}")
        assert ratio <= 1.0, f"{self.c.name} {what}: error / gauss_bound = {ratio:.3f} at {tuple((err / bound.clamp_min(1e-300)).flatten().argmax().unsqueeze(0).tolist())}"

    def check_write_only(self, got, ref, C_, ld, what, tol=None, exp=None):
        """real channels against fp64; pad channels [C, r8(C)) exactly zero; beyond r8(C): untouched (NaN) or zero"""
        rtol, atol = tol or (self.rtol, self.atol)
        g = got.double().cpu()
        if self.family == "gauss":
            scale = max(float(ref.abs().max()), 1e-6)
            torch.testing.assert_close(g[..., :C_], ref, rtol=rtol, atol=atol * scale, msg=lambda m: f"{self.c.name} {what}: {m}")
        if exp is not None:
            self.judge(g[..., :C_], exp, what)
        pad = g[..., C_:min(ld, _r8(C_))]
        assert bool((pad == 0).all()), f"{self.c.name} {what}: pad channels [{C_}, {min(ld, _r8(C_))}) not zero ({int((pad != 0).sum())} elements)"
        beyond = g[..., _r8(C_):ld]
        assert bool((torch.isnan(beyond) | (beyond == 0)).all()), f"{self.c.name} {what}: channels beyond r8(C) written"

    def check_accum(self, got, pat, ref, what, exp=None):
        g, pt = got.double().cpu(), pat.double().cpu()
        if self.family == "gauss":
            scale = max(float(ref.abs().max()), 1e-6)
            torch.testing.assert_close(g - pt, ref, rtol=self.rtol, atol=self.atol * scale + 1e-6, msg=lambda m: f"{self.c.name} {what}: {m}")
        if exp is not None:
            self.judge(g, exp, what, prefill=pt)

    # ---------------------------------------------------------------- calls
    def fwd(self, ws=None, nbytes=0):
        c = self.c
        y = _nan((c.B, self.OH, self.OW, self.ldy), torch.float32 if c.yf32 else _tdt(c))
        rc = self.lib.sv_conv2d_nhwc_fwd_ws(C.byref(self.d), _p(self.x), _p(self.wf), _p(self.b_dev), _p(y), _p(ws), nbytes, _st())
        return rc, y

    def dgrad(self, mask=None, atomic=False):
        c = self.c
        dx = _pattern((c.B, c.H, c.W, self.ldx)) if atomic else _nan((c.B, c.H, c.W, self.ldx), _tdt(c))
        before = dx.clone()
        rc = self.lib.sv_conv2d_nhwc_dgrad(C.byref(self.d), _p(self.dy), _p(self.wd), _p(mask), _p(dx), 1 if atomic else 0, _st())
        return rc, dx, before

    def lowres(self, ws=None, nbytes=0, mask=True):
        c = self.c
        dx = _nan((c.B, self.hin, self.win, self.ldx), _tdt(c))
        m = self.mask_lo if mask else None
        rc = self.lib.sv_conv2d_nhwc_dgrad_lowres_ws(C.byref(self.d), _p(self.dy), _p(self.wd), _p(m), _p(dx), _p(ws), nbytes, _st())
        return rc, dx

    def wgrad(self, ws=None, nbytes=0, use_ws_entry=True):
        c = self.c
        dw, db = _pattern((c.KH, c.KW, c.Cin, c.Cout)), _pattern((c.Cout,)) + 0.0625
        pw, pb = dw.clone(), db.clone()
        if use_ws_entry:
            rc = self.lib.sv_conv2d_nhwc_wgrad_ws(C.byref(self.d), _p(self.x), _p(self.dy), _p(dw), _p(db), _p(ws), nbytes, _st())
        else:
            rc = self.lib.sv_conv2d_nhwc_wgrad(C.byref(self.d), _p(self.x), _p(self.dy), _p(dw), _p(db), _st())
        return rc, dw, db, pw, pb

    def wgrad_poly(self, ws, nbytes):
        c = self.c
        dw, db = _pattern((c.KH, c.KW, c.Cin, c.Cout)), _pattern((c.Cout,)) + 0.0625
        pw, pb = dw.clone(), db.clone()
        rc = self.lib.sv_conv2d_nhwc_wgrad_poly(C.byref(self.d), _p(self.x), _p(self.dy), _p(dw), _p(db), _p(ws), nbytes, _st())
        return rc, dw, db, pw, pb

    def workspaces(self, n):
        """(label, tensor, bytes): none, too small (inside a guard region that must stay intact), exact, exact filled with 0xFF"""
        out = [("none", None, 0, None)]
        if n > 0:
            small = (n // 2) & ~255
            if small > 0:
                assert small < n
                guard = torch.full((small + 65536,), 0xA5, dtype=torch.uint8, device="cuda")
                out.append(("small", guard, small, small))
            out += [("exact", torch.zeros((n,), dtype=torch.uint8, device="cuda"), n, None),
                    ("0xff", torch.full((n,), 0xFF, dtype=torch.uint8, device="cuda"), n, None)]
        return out


def _ref_at(L, ref_u):
    return ref_u[L.uidx]


def _check_case(c, family="gauss"):
    L = Layer(c, family=family)
    lib = L.lib
    # the form a call takes (CASES): with a workspace that is too small a call runs as without one
    form = lambda call, det, label="none": _expected(c, call + "_ws" if label in ("exact", "0xff") else call, det)
    ws_f = lib.sv_conv2d_fwd_workspace_bytes(C.byref(L.d))
    ws_l = lib.sv_conv2d_dgrad_lowres_workspace_bytes(C.byref(L.d)) if c.ups else 0
    ws_w = lib.sv_conv2d_wgrad_workspace_bytes(C.byref(L.d))
    ws_p = lib.sv_conv2d_wgrad_poly_workspace_bytes(C.byref(L.d))
    assert min(ws_f, ws_l, ws_w, ws_p) >= 0
    assert (ws_p > 0) == ("wgrad_poly" in c.forms), (c.name, ws_p)
    y_ref = _ref_at(L, L.y_ref)
    dx_ref = L.dx_ref[L.pidx]
    for det in (1, 0):
        assert lib.sv_set_deterministic(det) == 0
        try:
            mode = "det" if det else "default"
            # forward: every workspace variant gives the same result (the polyphase forms fall back to their workspace-free form)
            first = None
            for label, ws, nb, guard_at in L.workspaces(ws_f):
                rc, y = L.fwd(ws, nb)
                assert rc == 0, (c.name, mode, label, rc)
                L.check_write_only(y, y_ref, c.Cout, L.ldy, f"fwd[{mode},{label}]", exp=L.expect("y", form("fwd", det, label)))
                if guard_at is not None:
                    assert bool((ws[guard_at:] == 0xA5).all()), f"{c.name}: forward wrote past the end of a too-small workspace"
                if first is None:
                    first = y
                else:
                    torch.testing.assert_close(y[..., :c.Cout], first[..., :c.Cout], rtol=1e-5, atol=1e-5 * float(y_ref.abs().max()))
            if det:                                  # (without a workspace the polyphase head adds its border terms atomically: header)
                ws = torch.zeros((max(ws_f, 1),), dtype=torch.uint8, device="cuda")
                y1, y2 = L.fwd(ws, ws_f)[1], L.fwd(ws, ws_f)[1]
                assert torch.equal(_bits(y1), _bits(y2)), f"{c.name}: deterministic forward not bitwise reproducible"
            # input gradient: plain, ReLU-masked, fp32-atomic (accumulated into a prefilled fp32 tensor)
            want = c.forms.get("dgrad")
            rc, dx, before = L.dgrad()
            if want == "unsupported":
                assert rc == SV_E_UNSUPPORTED, (c.name, rc)
                assert torch.equal(_bits(dx), _bits(before)), f"{c.name}: refused dgrad wrote its output"
                rc, dx, before = L.dgrad(atomic=True)
                assert rc == SV_E_UNSUPPORTED and torch.equal(dx, before)
            else:
                assert rc == 0, (c.name, mode, rc)
                L.check_write_only(dx, dx_ref, c.Cin, L.ldx, f"dgrad[{mode}]", exp=L.expect("dx", want))
                if det:
                    assert torch.equal(_bits(L.dgrad()[1]), _bits(dx)), f"{c.name}: deterministic dgrad not bitwise reproducible"
                rc, dxm, _ = L.dgrad(mask=L.mask)
                assert rc == 0
                L.check_write_only(dxm, dx_ref * (L.M[L.pidx].double() > 0), c.Cin, L.ldx, f"dgrad masked[{mode}]", exp=L.expect("dx", want, mask="hi"))
                rc, dxa, pat = L.dgrad(atomic=True)
                assert rc == 0
                L.check_accum(dxa[..., :c.Cin], pat[..., :c.Cin], dx_ref, f"dgrad atomic[{mode}]", exp=L.expect("dx", "atomic_splitk"))
                assert torch.equal(dxa[..., c.Cin:], pat[..., c.Cin:]), f"{c.name}: fp32-atomic dgrad wrote channels >= Cin"
                if det:
                    assert torch.equal(L.dgrad(atomic=True)[1], dxa), f"{c.name}: deterministic atomic dgrad not reproducible"
            # the input gradient at the low-res tensor (ups_in): fused, or SV_E_UNSUPPORTED with nothing written -> dgrad + resize adjoint
            if c.ups:
                lo_ref = L.dxlo_ref[L.pidx] * (L.ML[L.pidx].double() > 0)
                for label, ws, nb, guard_at in L.workspaces(ws_l):
                    rc, dxl = L.lowres(ws, nb)
                    if guard_at is not None:
                        assert bool((ws[guard_at:] == 0xA5).all()), f"{c.name}: dgrad_lowres wrote past the end of a too-small workspace"
                    if rc == SV_E_UNSUPPORTED:
                        assert bool(torch.isnan(dxl.float()).all()), f"{c.name}: refused dgrad_lowres wrote its output"
                        rc, dxh, _ = L.dgrad()
                        assert rc == 0
                        dxl = torch.empty_like(dxl)
                        assert lib.sv_upsample2x_bwd(_p(dxh), _p(L.mask_lo), _p(dxl), L.d.dtype, c.B, L.hin, L.win, L.ldx, _st()) == 0
                        # (the hi-res gradient is rounded to the activation dtype before the adjoint)
                        L.check_write_only(dxl, lo_ref, c.Cin, L.ldx, f"dgrad+upsample2x_bwd[{mode},{label}]",
                                           tol=(L.rtol, L.atol if c.dt == "f32" else 2 * L.atol), exp=L.expect("dxlo", "per_class"))
                    else:
                        assert rc == 0, (c.name, label, rc)
                        L.check_write_only(dxl, lo_ref, c.Cin, L.ldx, f"dgrad_lowres[{mode},{label}]", exp=L.expect("dxlo", form("lowres", det, label)))
            # weight gradient: accumulated into prefilled dw / dbias, with every workspace variant; SV_E_UNSUPPORTED leaves both untouched
            results = []
            for label, ws, nb, guard_at in [("entry", None, 0, None)] + L.workspaces(ws_w):
                rc, dw, db, pw, pb = L.wgrad(ws, nb, use_ws_entry=label != "entry")
                if guard_at is not None:
                    assert bool((ws[guard_at:] == 0xA5).all()), f"{c.name}: wgrad wrote past the end of a too-small workspace"
                if rc == SV_E_UNSUPPORTED:
                    assert torch.equal(dw, pw) and torch.equal(db, pb), f"{c.name}: refused wgrad[{label}] wrote dw / dbias"
                    continue
                assert rc == 0, (c.name, mode, label, rc)
                wform = form("wgrad", det, label)
                L.check_accum(dw, pw, L.dw_ref, f"wgrad dw[{mode},{label}]", exp=L.expect("dw", wform))
                if c.bias:
                    L.check_accum(db, pb, L.db_ref, f"wgrad dbias[{mode},{label}]", exp=L.expect("db", wform))
                results.append((label, ws, nb, dw))
            assert results or c.forms.get("wgrad_ws") == "unsupported", f"{c.name}: no weight-gradient call succeeded"
            if det and not c.fold:                   # (reproducible with a workspace: without one the tile kernels add atomically, header)
                for label, ws, nb, dw in [r for r in results if r[0] in ("exact", "0xff")]:
                    if label == "0xff":
                        ws.fill_(0xFF)
                    again = L.wgrad(ws, nb, use_ws_entry=label != "entry")[1]
                    assert torch.equal(again, dw), f"{c.name}: deterministic wgrad[{label}] not bitwise reproducible"
            # polyphase weight gradient of the bf16 head: workspace zeroed before its first use; too small -> SV_E_BADARG, nothing written
            if ws_p > 0:
                ws = torch.zeros((ws_p,), dtype=torch.uint8, device="cuda")
                rc, dw, db, pw, pb = L.wgrad_poly(ws, ws_p)
                assert rc == 0, (c.name, rc)
                L.check_accum(dw, pw, L.dw_ref, f"wgrad_poly dw[{mode}]", exp=L.expect("dw", "wgrad_poly"))
                L.check_accum(db, pb, L.db_ref, f"wgrad_poly dbias[{mode}]", exp=L.expect("db", "wgrad_poly"))
                rc, dw, db, pw, pb = L.wgrad_poly(ws, ws_p // 2)
                assert rc == SV_E_BADARG and torch.equal(dw, pw) and torch.equal(db, pb)
        finally:
            assert lib.sv_set_deterministic(-1) == 0
    return L.ratios


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_descriptor_against_fp64(lib_built, c):
    _check_case(c)


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_descriptor_bit_for_bit_on_integer_operands(lib_built, c):
    """the same call sequence on the integer family: every real channel of every form is the float64 result cast once (BOUND_NOT_BITS aside)"""
    for call in R.calls_of(c):
        R.conv_exact_property(c, call)
    _check_case(c, family="int")


# ---------------------------------------------------------------- refusals
REFUSED = [
    # (name, descriptor fields, code)
    ("stride4", dict(s=4), SV_E_UNSUPPORTED),
    ("cin17_pad24", dict(Cin=17), SV_E_UNSUPPORTED),            # r8(Cin) = 24: not a power of two
    ("ldx_not_mult8", dict(ldx=12), SV_E_BADARG),
    ("ldx_below_cin", dict(Cin=12, ldx=8), SV_E_BADARG),
    ("ldy_below_cout", dict(ldy=8, Cout=12), SV_E_BADARG),
    ("ldy_not_mult8", dict(ldy=12), SV_E_BADARG),
    ("stride2_odd_extent", dict(s=2, H=15), SV_E_UNSUPPORTED),
    ("ups_stride2", dict(s=2, ups=1), SV_E_UNSUPPORTED),
    ("ups_odd_extent", dict(ups=1, W=18 + 1), SV_E_UNSUPPORTED),
    ("taps_over_81", dict(KH=9, KW=10), SV_E_UNSUPPORTED),
    ("zero_batch", dict(B=0), SV_E_BADARG),
    ("bad_dtype", dict(dt="f16"), SV_E_BADARG),
]


@pytest.mark.parametrize("name,over,code", REFUSED, ids=[r[0] for r in REFUSED])
def test_refused_descriptor_leaves_every_buffer_untouched(lib_built, name, over, code):
    from split_vae_amd import _lib
    lib = _lib.load()
    base = dict(B=2, H=16, W=16, Cin=8, Cout=8, KH=3, KW=3, s=1, act=None, dt="f32")
    base.update(over)
    ldx, ldy = base.pop("ldx", _r8(max(base["Cin"], 1))), base.pop("ldy", _r8(base["Cout"]))
    ups = base.pop("ups", 0)
    d = _lib.ConvDesc(base["B"], base["H"], base["W"], base["Cin"], base["Cout"], base["KH"], base["KW"], base["s"], 0,
                      {"f32": _lib.SV_F32, "bf16": _lib.SV_BF16}.get(base["dt"], 7), ldx, ldy, 0, ups)
    assert lib.sv_conv2d_wprep_elems(C.byref(d), 0) == -1 and lib.sv_conv2d_wprep_elems(C.byref(d), 1) == -1
    for f in (lib.sv_conv2d_fwd_workspace_bytes, lib.sv_conv2d_wgrad_workspace_bytes, lib.sv_conv2d_dgrad_lowres_workspace_bytes,
              lib.sv_conv2d_wgrad_poly_workspace_bytes):
        assert f(C.byref(d)) == -1
    n = 1 << 16                                                       # every buffer far larger than any call could address here
    src = torch.ones((n,), dtype=torch.float32, device="cuda")
    bufs = [_nan((n,), torch.float32) for _ in range(2)] + [_pattern((n,)) for _ in range(2)]
    keep = [b.clone() for b in bufs]
    y, dx, dw, db = bufs
    st = _st()
    assert lib.sv_conv2d_prep_weights(C.byref(d), _p(src), _p(y), _p(dx), st) == code
    assert lib.sv_conv2d_nhwc_fwd(C.byref(d), _p(src), _p(src), _p(src), _p(y), st) == code
    assert lib.sv_conv2d_nhwc_fwd_ws(C.byref(d), _p(src), _p(src), _p(src), _p(y), _p(dx), n, st) == code
    assert lib.sv_conv2d_nhwc_dgrad(C.byref(d), _p(src), _p(src), None, _p(dx), 0, st) == code
    assert lib.sv_conv2d_nhwc_dgrad(C.byref(d), _p(src), _p(src), None, _p(dw), 1, st) == code
    assert lib.sv_conv2d_nhwc_dgrad_lowres_ws(C.byref(d), _p(src), _p(src), None, _p(dx), _p(y), n, st) == code
    assert lib.sv_conv2d_nhwc_wgrad(C.byref(d), _p(src), _p(src), _p(dw), _p(db), st) == code
    assert lib.sv_conv2d_nhwc_wgrad_ws(C.byref(d), _p(src), _p(src), _p(dw), _p(db), _p(y), n, st) == code
    assert lib.sv_conv2d_nhwc_wgrad_poly(C.byref(d), _p(src), _p(src), _p(dw), _p(db), _p(y), n, st) == code
    torch.cuda.synchronize()
    for b, k in zip(bufs, keep):
        assert torch.equal(_bits(b), _bits(k)), name


def test_dgrad_lowres_refuses_a_layer_without_ups_in(lib_built):
    c = case("plain", 2, 16, 16, 8, 8, 3, 3, 1, None, "f32")
    L = Layer(c, refs=False)
    dx = _nan((2, 8, 8, 8), torch.float32)
    assert L.lib.sv_conv2d_nhwc_dgrad_lowres(C.byref(L.d), _p(L.dy), _p(L.wd), None, _p(dx), _st()) == SV_E_BADARG
    assert bool(torch.isnan(dx).all())


# ---------------------------------------------------------------- coverage of the dispatch forms
def _trace_calls(c, det, mark):
    """the calls CASES names forms for, each preceded by a marker line on stderr"""
    L = Layer(c, refs=False)
    lib = L.lib
    ws = lambda n: torch.zeros((max(n, 1),), dtype=torch.uint8, device="cuda")
    calls = [("fwd", lambda: L.fwd()), ("dgrad", lambda: L.dgrad()), ("dgrad_atomic", lambda: L.dgrad(atomic=True)),
             ("wgrad", lambda: L.wgrad(use_ws_entry=False))]
    n = lib.sv_conv2d_fwd_workspace_bytes(C.byref(L.d))
    if n > 0:
        calls.append(("fwd_ws", lambda: L.fwd(ws(n), n)))
    if c.ups:
        calls.append(("lowres", lambda: L.lowres()))
        n2 = lib.sv_conv2d_dgrad_lowres_workspace_bytes(C.byref(L.d))
        if n2 > 0:
            calls.append(("lowres_ws", lambda: L.lowres(ws(n2), n2)))
    n3 = lib.sv_conv2d_wgrad_workspace_bytes(C.byref(L.d))
    calls.append(("wgrad_ws", lambda: L.wgrad(ws(n3), n3)))
    n4 = lib.sv_conv2d_wgrad_poly_workspace_bytes(C.byref(L.d))
    if n4 > 0:
        calls.append(("wgrad_poly", lambda: L.wgrad_poly(ws(n4), n4)))
    assert lib.sv_set_deterministic(det) == 0
    try:
        for name, f in calls:
            mark(f"call {c.name} {'det' if det else 'default'} {name}")
            f()
            torch.cuda.synchronize()
    finally:
        assert lib.sv_set_deterministic(-1) == 0


def trace_main():
    """child process (SV_TRACE_DISPATCH=1): every case in both modes"""
    def mark(s):
        sys.stderr.flush()
        os.write(2, (s + "\n").encode())
    for c in CASES:
        for det in (0, 1):
            _trace_calls(c, det, mark)
    mark("done")


def _expected(c, call, det):
    f = c.forms
    if call == "fwd_ws":
        want = f.get("fwd_ws", f.get("fwd"))
    elif call == "lowres_ws":
        want = f.get("lowres_ws", f.get("lowres"))
    elif call == "dgrad_atomic":
        want = "unsupported" if f.get("dgrad") == "unsupported" else "atomic_splitk"
    else:
        want = f.get(call)
    if isinstance(want, tuple):
        want = want[1] if det else want[0]
    return want


def parse_trace(text):
    """-> {(case, mode, call): form or 'unsupported' (no line)}"""
    got, key = {}, None
    for line in text.splitlines():
        if line.startswith("call ") or line == "done":
            if key is not None and key not in got:
                got[key] = "unsupported"
            key = tuple(line.split()[1:]) if line != "done" else None
        elif line.startswith("sv_dispatch ") and key is not None:
            op, form = line.split()[1:3]
            got[key] = form
    return got


def test_every_form_is_reached_and_every_case_takes_its_form(lib_built, tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "import sys; sys.path[:0] = [%r, %r]\nimport test_gpu_conv_api as T\nT.trace_main()\n" % (root, os.path.join(root, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SV_TRACE_DISPATCH="1"), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    got = parse_trace(r.stderr)
    lines = [l.split()[1:3] for l in r.stderr.splitlines() if l.startswith("sv_dispatch ")]
    for op, form in lines:
        assert op in FORMS and form in FORMS[op], f"trace names an unknown form: {op} {form}"
    hit = {(op, form) for op, form in lines}
    missing = sorted((op, f) for op, fs in FORMS.items() for f in fs if (op, f) not in hit)
    wrong = []
    for c in CASES:
        for det in (0, 1):
            for (name, mode, call), form in got.items():
                if name != c.name or mode != ("det" if det else "default"):
                    continue
                want = _expected(c, call, det)
                if want is None or form != want:
                    wrong.append(f"{c.name} {mode} {call}: expected {want}, took {form}")
    assert not wrong and not missing, "\n".join(wrong + [f"form never reached: {op} {f}" for op, f in missing])


# ---------------------------------------------------------------- torch-op level: a thin fp32 output feeding the next layer
def test_chained_fp32_conv2d_with_six_channels_against_fp64(lib_built, monkeypatch):
    """split_vae::conv2d at fp32 with Cout = 6 returns [B,H,W,8]; the next conv requires those pad channels to be zero (torch_ops.conv2d).
    Every torch.empty of the first layer's call returns NaN-filled memory (its output buffer among them), so what the kernel does not write
    stays NaN."""
    import split_vae_amd.torch_ops as tops
    g = torch.Generator().manual_seed(11)
    B, H, W = 3, 16, 16
    x = torch.randn(B, H, W, 3, generator=g)
    w1 = torch.randn(3, 3, 3, 6, generator=g) * 0.3
    b1 = torch.randn(6, generator=g) * 0.1
    w2 = torch.randn(3, 3, 6, 16, generator=g) * 0.3
    b2 = torch.randn(16, generator=g) * 0.1
    xg = torch.zeros(B, H, W, 8)
    xg[..., :3] = x
    xg = xg.cuda()
    params = [t.cuda().requires_grad_(True) for t in (w1, b1, w2, b2)]
    empty = torch.empty

    def nan_empty(*a, **k):
        t = empty(*a, **k)
        return t.fill_(float("nan")) if t.is_floating_point() else t
    monkeypatch.setattr(torch, "empty", nan_empty)
    y1 = tops.conv2d(xg, params[0], params[1], stride=1, act="relu")
    monkeypatch.setattr(torch, "empty", empty)
    assert y1.shape == (B, H, W, 8) and bool((y1[..., 6:] == 0).all()), "pad channels of the fp32 output not zero"
    y2 = tops.conv2d(y1, params[2], params[3], stride=1, act=None)
    y2.sum().backward()
    xr = x.double()
    pr = [p.detach().cpu().double().requires_grad_(True) for p in params]
    r1 = torch_ref.conv2d_same(xr, pr[0], pr[1], 1, "relu")
    r2 = torch_ref.conv2d_same(r1, pr[2], pr[3], 1, None)
    r2.sum().backward()
    torch.testing.assert_close(y2[..., :16].double().cpu(), r2.detach(), rtol=F32_RTOL, atol=F32_ATOL * float(r2.abs().max()))
    for p, q in zip(params, pr):
        torch.testing.assert_close(p.grad.double().cpu(), q.grad, rtol=F32_RTOL, atol=F32_ATOL * float(q.grad.abs().max()))


# ---------------------------------------------------------------- ups_in forwards outside the tile kernels (header: the accepted domain)
UPS_REFUSED = [
    # name, B, H, W, Cin, Cout, k, dtype, ldy, y_f32
    ("ups_12x20_f32", 2, 12, 20, 12, 16, 3, "f32", 0, 0),        # non-power-of-two grid: the im2col kernels cannot upsample
    ("ups_24x12_bf16", 2, 24, 12, 5, 16, 3, "bf16", 0, 0),
    ("ups_4x2_f32", 3, 4, 2, 8, 8, 3, "f32", 0, 0),              # fewer than 16 output pixels
    ("ups_c48_f32", 2, 16, 16, 8, 48, 3, "f32", 0, 0),           # Cout neither <= 16 nor a multiple of 32
    ("ups_c6_ldy7_yf32", 2, 16, 16, 8, 6, 3, "f32", 7, 1),       # stored row of 7 fp32 channels: not an 8-byte multiple
]


@pytest.mark.parametrize("u", UPS_REFUSED, ids=[u[0] for u in UPS_REFUSED])
def test_ups_in_forward_without_a_tile_kernel_is_refused_untouched(lib_built, u):
    """SV_E_UNSUPPORTED with y untouched; the documented way round (sv_upsample2x_fwd, then the layer without ups_in) gives the fp64 answer"""
    from split_vae_amd import _lib
    name, B, H, W, Cin, Cout, k, dt, ldy, yf32 = u
    c = case(name, B, H, W, Cin, Cout, k, k, 1, None, dt, ldy=ldy, yf32=yf32, ups=1)
    L = Layer(c)
    lib = L.lib
    rc, y = L.fwd()
    assert rc == SV_E_UNSUPPORTED, (name, rc)
    torch.cuda.synchronize()
    assert bool(torch.isnan(y.float()).all()), f"{name}: refused forward wrote y"
    hi = torch.empty((B, H, W, L.ldx), dtype=_tdt(c), device="cuda")
    assert lib.sv_upsample2x_fwd(_p(L.x), _p(hi), L.d.dtype, B, H // 2, W // 2, L.ldx, _st()) == 0
    d = _lib.ConvDesc(*[getattr(L.d, f) for f, _ in _lib.ConvDesc._fields_])
    d.ups_in = 0
    wf = torch.empty((lib.sv_conv2d_wprep_elems(C.byref(d), 0),), dtype=_tdt(c), device="cuda")
    assert lib.sv_conv2d_prep_weights(C.byref(d), _p(L.w_dev), _p(wf), None, _st()) == 0
    y2 = _nan(tuple(y.shape), y.dtype)
    assert lib.sv_conv2d_nhwc_fwd(C.byref(d), _p(hi), _p(wf), _p(L.b_dev), _p(y2), _st()) == 0
    # (the upsampled input is rounded to the activation dtype before the conv)
    L.check_write_only(y2, L.y_ref[L.uidx], Cout, L.ldy, "upsample2x_fwd + conv", tol=(L.rtol, L.atol if dt == "f32" else 2 * L.atol))
