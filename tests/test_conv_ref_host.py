"""CPU: tests/conv_ref.py itself -- the integer family's exactness property for every case and call of tests/test_gpu_conv_api.py's CASES, that
every mutant of the references is seen by both input families, and the references against the two independent restatements under oracle/."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_ref as R  # noqa: E402
from test_gpu_conv_api import CASES  # noqa: E402  (the table only: nothing of that module touches the GPU at import)
from oracle import np_ref, torch_ref  # noqa: E402

IDS = [c.name for c in CASES]
F64 = torch.float64


def _exact_in(t, dtype):
    return bool((t.to(F64).to(torch.float32).to(dtype).to(F64) == t.to(F64)).all())


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_integer_family_is_exact_for_every_call(c):
    """the property of the lemma, and every operand and named intermediate (scaled images, staged hi-res pixels, composite polyphase weights and their
    border class sums, the references cast to the output type) exactly representable in the case's dtype"""
    ops = R.operands(c, "int")
    dt = R.tdt(c)
    for call in R.calls_of(c):
        q, worst = R.conv_exact_property(c, call, ops)
        assert worst < 2.0 ** 24 and q <= 1.0
    xu = R.x_unique(ops)
    for name in ("X", "DY", "M", "ML"):
        assert _exact_in(ops[name], dt) and bool((ops[name].to(F64) == ops[name].to(F64).round()).all()), name
    assert _exact_in(xu, dt) and _exact_in(ops["w"], dt)
    if c.bias:
        assert bool((ops["bias"].to(F64) * 16 == (ops["bias"].to(F64) * 16).round()).all())
    if c.ups:
        hi = R.resize2x(xu)
        assert _exact_in(hi, dt), "hi-res pixels"
        assert torch.equal(R.resize2x_staged(xu, dt), hi), "the staged resize of integer operands is the exact one"
        if c.KH == 6 and c.KW == 6:
            wc = R.composite_weights(ops["w"])
            assert _exact_in(wc, dt) and float((wc * 16).abs().max()) < 256, "composite polyphase weights"
            assert torch.equal(R.composite_weights(ops["w"], dt), wc)
    ref = R.references(c, ops)
    # fp32 outputs and accumulators hold the reference exactly (which is what "cast once" relies on)
    for k in ("y", "dx", "dw", "db") + (("dxlo",) if c.ups else ()):
        assert _exact_in(ref[k], torch.float32), k


# ---------------------------------------------------------------------------------------------------------------- mutants
def _applies(c, mut, key):
    """does mutant `mut` change reference `key` of case c?"""
    if mut == "drop_border_tap":
        return key in ("y", "dx", "dw")
    if mut in ("swap_quarters_edge", "zero_pad_resize"):
        return bool(c.ups) and key in ("y", "dxlo", "dw")
    if mut == "no_bias":
        return c.bias and key in ("y", "db")
    if mut == "no_frame_corner":
        return bool(c.ups) and key == "y" and c.KH >= 3 and c.KW >= 3
    if mut == "gate_from_gradient":
        return bool(c.ups) and key == "dxlo"
    raise AssertionError(mut)


N_OF = dict(y=lambda c: c.KH * c.KW * c.Cin, dx=lambda c: c.KH * c.KW * c.Cout, dxlo=lambda c: c.KH * c.KW * c.Cout + 16,
            dw=lambda c: c.B * -(-c.H // c.s) * -(-c.W // c.s), db=lambda c: c.B * -(-c.H // c.s) * -(-c.W // c.s))
OUT_BF16 = dict(y=lambda c: c.dt == "bf16" and not c.yf32, dx=lambda c: c.dt == "bf16", dxlo=lambda c: c.dt == "bf16", dw=lambda c: False, db=lambda c: False)

# mutants the Gaussian bound cannot see at some case, with the reason; the integer family must still see them there (asserted below)
_LONG = ("the weight gradient contracts over n = B OH OW = 2^%d positions: the bound, n 2^-23 sum|terms|, is %s of the sum of ALL |terms|, while the mutant changes "
         "the terms of one row of positions, whose signs are random")
GAUSS_BLIND = {
    ("drop_border_tap", "e1_b256_bf16", "dw"): _LONG % (18, "1/32"),
    ("drop_border_tap", "poly_p5_b128_bf16", "dw"): _LONG % (19, "1/16"),
    ("swap_quarters_edge", "poly_p5_b128_bf16", "dw"): _LONG % (19, "1/16"),
    ("zero_pad_resize", "poly_p5_b128_bf16", "dw"): _LONG % (19, "1/16"),
    ("no_bias", "poly_p5_b128_bf16", "db"): "dbias sums 2^19 gradient pixels of random sign: |dbias| ~ 2^9.5 sigma, the bound is 2^-4 sum|dy| ~ 2^15 sigma",
}

_CACHE = {}


def _refs(c, family, mut=None, absval=False):
    k = (c.name, family, mut, absval)
    if k not in _CACHE:
        _CACHE[k] = R.references(c, R.operands(c, family), mut=mut, absval=absval)
    return _CACHE[k]


def _keys(c, mut):
    return [k for k in ("y", "dx", "dxlo", "dw", "db") if (k != "dxlo" or c.ups) and _applies(c, mut, k)]


PAIRS = [(c, m) for c in CASES for m in R.MUTANTS if _keys(c, m)]        # every case a mutant applies to


@pytest.mark.parametrize("c,mut", PAIRS, ids=[f"{c.name}-{m}" for c, m in PAIRS])
def test_every_mutant_is_seen_by_both_families(c, mut):
    keys = _keys(c, mut)
    for k in keys:
        true_i, mut_i = _refs(c, "int")[k], _refs(c, "int", mut)[k]
        out_dt = torch.bfloat16 if OUT_BF16[k](c) else torch.float32
        assert not torch.equal(true_i.to(out_dt), mut_i.to(out_dt)), f"{c.name} {k}: the integer family does not see {mut}"
        true_g, mut_g, abs_g = _refs(c, "gauss")[k], _refs(c, "gauss", mut)[k], _refs(c, "gauss", absval=True)[k]
        bound = R.gauss_bound(abs_g, N_OF[k](c), S=8, ref=true_g, bf16_out=OUT_BF16[k](c))
        seen = bool(((mut_g - true_g).abs() > bound).any())
        if (mut, c.name, k) in GAUSS_BLIND:
            assert not seen, f"{c.name} {k}: {mut} is listed as invisible to the Gaussian bound, and is seen"
        else:
            assert seen, f"{c.name} {k}: the Gaussian bound does not see {mut}"


# ---------------------------------------------------------------------------------------------------------------- the independent restatements
def _close(a, b):
    a, b = torch.as_tensor(a, dtype=F64), torch.as_tensor(b, dtype=F64)
    assert float((a - b).abs().max()) <= 1e-12 * max(float(b.abs().max()), 1e-300)


GEOMS = [(2, 8, 12, 5, 7, 3, 3, 1), (2, 12, 8, 3, 4, 4, 4, 2), (1, 8, 8, 4, 6, 6, 6, 1), (2, 12, 6, 2, 3, 6, 6, 3), (2, 8, 8, 3, 2, 5, 3, 1), (1, 16, 16, 3, 5, 6, 6, 2)]


GEOMS_UPS = [(g, u) for g in GEOMS for u in (0, 1) if not (u and g[7] != 1)]       # (ups_in layers have stride 1)


@pytest.mark.parametrize("g,ups", GEOMS_UPS, ids=[f"{g}-ups{u}" for g, u in GEOMS_UPS])
def test_references_agree_with_the_numpy_and_torch_restatements(g, ups):
    B, H, W, Cin, Cout, KH, KW, s = g
    gen = torch.Generator().manual_seed(H * 100 + W + KH)
    hin, win = (H // 2, W // 2) if ups else (H, W)
    x = torch.randn(B, hin, win, Cin, generator=gen, dtype=F64)
    w = torch.randn(KH, KW, Cin, Cout, generator=gen, dtype=F64)
    b = torch.randn(Cout, generator=gen, dtype=F64)
    OH, OW = -(-H // s), -(-W // s)
    dy = torch.randn(B, OH, OW, Cout, generator=gen, dtype=F64)
    act_lo = torch.randn(B, hin, win, Cin, generator=gen, dtype=F64)
    # forward: the NumPy restatement (square kernels only there) and the torch one
    hi_np = np_ref.resize_bilinear_2x(x.numpy()) if ups else x.numpy()
    if ups:
        _close(R.resize2x(x), hi_np)
        _close(R.resize2x(x), torch_ref.resize_bilinear_2x(x))
    for act in (None, "relu"):
        got = R.conv(x, w, b, s, act, bool(ups))
        if KH == KW:
            _close(got, np_ref.conv2d_same(hi_np, w.numpy(), b.numpy(), s, act))
        _close(got, torch_ref.conv2d_same(torch.as_tensor(hi_np), w, b, s, act))
    # gradients: autograd through the torch restatement
    xl = x.clone().requires_grad_(True)
    wl, bl = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    hi = torch_ref.resize_bilinear_2x(xl) if ups else xl
    hi.retain_grad()
    torch_ref.conv2d_same(hi, wl, bl, s, None).backward(dy)
    _close(R.dgrad(dy, w, s, H, W), hi.grad)
    dw, db = R.wgrad(x, dy, KH, KW, s, bool(ups))
    _close(dw, wl.grad)
    _close(db, bl.grad)
    if ups:
        _close(R.dgrad_lowres(dy, w, H, W, None), xl.grad)
        _close(R.dgrad_lowres(dy, w, H, W, act_lo), xl.grad * (act_lo > 0))
        # the polyphase head with unrounded weights and lines is the same conv
        if KH == 6 and KW == 6:
            x32 = x.float().double()
            ph = R.poly_head_fwd(x32, w.float(), b, torch.float32)
            ref = R.conv(x32, w.float().double(), b, 1, None, True)
            assert float((ph - ref).abs().max()) <= 1e-5 * float(ref.abs().max())


def test_staged_resize_is_the_resize_rounded_once_up_to_its_fp32_lerps():
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(2, 6, 5, 8, generator=gen).to(torch.bfloat16)
    exact = R.resize2x(x)
    st = R.resize2x_staged(x, torch.bfloat16)
    assert float((st - exact).abs().max()) <= 2.0 ** -8 * float(exact.abs().max())
    assert bool((st == R.rnd(st, torch.bfloat16)).all())
    # fp32: three fp32 roundings of a convex combination
    xf = torch.randn(2, 6, 5, 8, generator=gen)
    assert float((R.resize2x_staged(xf, torch.float32) - R.resize2x(xf)).abs().max()) <= 4 * 2.0 ** -24 * float(xf.abs().max())
    # integers: exact
    xi = torch.randint(-3, 4, (2, 6, 5, 8), generator=gen).to(torch.bfloat16)
    assert torch.equal(R.resize2x_staged(xi, torch.bfloat16), R.resize2x(xi))


def test_gauss_bound_is_the_latent_gemm_one():
    import latent_gemm_ref
    assert R.gauss_bound is latent_gemm_ref.gauss_bound
