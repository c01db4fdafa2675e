"""GPU: the SPLIT-GMVAE glue kernels of csrc/gm_pointwise.hip one by one through ops.*, against the float64 restatements of tests/gm_pointwise_ref.py, at the
shapes where their indexing can go wrong: rows that are no multiple of the 4 waves of a block, one and two columns per lane (K, L around 64 and 128), row pitches
wider than the width, pad columns, in-place calls, the grid-stride loops, and the Philox keys (mirror bit for bit, shard by shard).

The rule for an fp32 output, element by element: |gpu - ref| <= 1e-4 |ref| + 1e-5 scale, 1e-4 the project's fp32 bar (tests/test_gpu_kernels.py: F32_RTOL) and scale
the largest |addend| of that element in the float64 reference -- a cancelling sum is judged by its condition.  A zero reference with a zero scale wants an exact zero.

bf16 outputs: from_f32<bf16_t> is a plain (bf16_t) cast, which gfx950 converts in hardware with round-to-nearest-even, so EQUALITY is expected, not one ulp:
  act / add   against the float64 result computed from the (bf16-rounded) inputs the kernel reads, rounded once to bf16; the generators keep those results a few fp32
              ulps away from the rounding ties (gm_pointwise_ref.settle_away_from_ties), where rounding the kernel's fp32 value may legitimately differ
  the others  (fp32 inputs, sums inside) against the bf16 rounding of the kernel's own fp32 output, which the fp32 call of the same test holds to the rule above

Every compared figure is printed before it is asserted (pytest -s).  Measured on MI355X: LAB_NOTES.md, "GMVAE glue kernels: kernel-level parity"."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gm_pointwise_ref as G  # noqa: E402
from test_gpu_kernels import F32_RTOL  # noqa: E402

pytestmark = pytest.mark.gpu

F64 = torch.float64
ADDEND_ATOL = 1e-5
BF, F32 = torch.bfloat16, torch.float32
SEED, STEP = 0x1234567890ABCDEF, (3 << 32) | 5
OFFSET = (1 << 32) + 5                                            # a global sample index with bits above 2^32: the high word of the key


@pytest.fixture(scope="module")
def ops(lib_built):
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from split_vae_amd import ops as o
    return o


def dev(t, dtype=F32):
    return t.to(dtype).cuda().contiguous()


def filled(shape, dtype=F32, value=3.0):
    """an output buffer with a sentinel in it (3.0 is a bf16 number): what the kernel does not write stays visible"""
    return torch.full(shape, value, dtype=dtype, device="cuda")


def close(what, got, ref, scale=None, rtol=F32_RTOL, floor=0.0):
    got, ref = got.detach().to(F64).cpu(), ref.to(F64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    scale = ref.abs() if scale is None else scale.to(F64)
    err = (got - ref).abs()
    bound = rtol * ref.abs() + ADDEND_ATOL * scale + floor
    nz = ref != 0
    rel = float((err[nz] / ref.abs()[nz]).max()) if bool(nz.any()) else 0.0
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print("%-58s worst rel %.3e   worst err / bound %.4f" % (what, rel, ratio))
    assert bool(torch.isfinite(got).all()), what
    assert bool((err <= bound).all()), (what, "worst rel %.3e, worst err / bound %.3f at flat index %d" % (rel, ratio, int((err / bound.clamp_min(1e-300)).argmax())))
    return rel


def same_bf16(what, got, ref64):
    """a bf16 output == the float64 reference rounded once (the module docstring says when that is the right question)"""
    got, want = got.detach().to(F64).cpu(), G.bf16_rne(ref64.to(F64))
    bad = int((got != want).sum())
    print("%-58s bf16 mismatches %d of %d" % (what, bad, got.numel()))
    assert got.shape == want.shape and bad == 0, (what, bad)


def bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int16 if a.dtype == BF else torch.int32), b.view(torch.int16 if b.dtype == BF else torch.int32))


# ------------------------------------------------------------------------------------------------------------------- act_fwd
DT_PAIRS = ((F32, F32), (F32, BF), (BF, BF))
RATE = 0.3


def _check_act_out(what, got, ref, C, x_dt):
    assert float(got[:, C:].float().abs().max() if got.shape[1] > C else 0.0) == 0.0, (what, "pad columns are not zero")
    if x_dt == BF:
        same_bf16(what, got, ref)
    else:
        close(what, got, ref)


@pytest.mark.parametrize("kind", [None, "relu", "elu"])
@pytest.mark.parametrize("a_dt,x_dt", DT_PAIRS, ids=["f32_f32", "f32_bf16", "bf16_bf16"])
@pytest.mark.parametrize("rows,C,lda,ldx,rps", G.ACT_SHAPES)
def test_act_fwd(ops, rows, C, lda, ldx, rps, a_dt, x_dt, kind):
    """x = dropout(act(a)) and the stored pre-dropout activation: no dropout, a pinned mask at rate 0.3, in place (a is x, y_act = None: how gm_encoder.hip calls it)
    where the pitches allow it, and the Philox mask -- keep_out against the mirror bit for bit, reproducible, shard-invariant, keyed by stream id and step."""
    tag = "act_fwd %s %dx%d %s->%s" % (kind, rows, C, "bf16" if a_dt == BF else "f32", "bf16" if x_dt == BF else "f32")
    a = G.settled_act_inputs(rows, C, lda, rows + C, kind, RATE, a_dt == BF) if x_dt == BF else G.act_inputs(rows, C, lda, rows + C, a_dt == BF)
    ad = dev(a, a_dt)
    # no dropout
    y, x = filled((rows, ldx), x_dt), filled((rows, ldx), x_dt)
    ops.act_fwd(ad, C, x, act=kind, y_act=y)
    yr, xr = G.act_fwd_ref(a, C, ldx, kind)
    _check_act_out(tag + " y_act", y, yr, C, x_dt)
    _check_act_out(tag + " x", x, xr, C, x_dt)
    assert bits_equal(x, y)
    # a pinned mask
    keep = G.pinned_keep(rows, C, RATE, 5)
    y2, x2, ko = filled((rows, ldx), x_dt), filled((rows, ldx), x_dt), filled((rows, C))
    ops.act_fwd(ad, C, x2, act=kind, y_act=y2, rate=RATE, keep_in=dev(keep), keep_out=ko)
    _check_act_out(tag + " x, pinned mask", x2, G.act_fwd_ref(a, C, ldx, kind, RATE, keep)[1], C, x_dt)
    assert bits_equal(y2, y) and torch.equal(ko.cpu(), keep)
    # in place
    if lda == ldx and a_dt == x_dt:
        for rate in (0.0, RATE):
            xi = ad.clone()
            ops.act_fwd(xi, C, xi, act=kind, rate=rate, keep_in=dev(keep) if rate else None)
            assert bits_equal(xi, x2 if rate else x), (tag, "the in-place call differs", rate)
    # the Philox mask
    mirror = G.dropout_keep(rows, C, RATE, SEED, STEP, 2, OFFSET, rps)
    kw = dict(act=kind, rate=RATE, seed=SEED, step=STEP, stream_id=2, sample_offset=OFFSET, rows_per_sample=rps)
    x3, k3 = filled((rows, ldx), x_dt), filled((rows, C))
    ops.act_fwd(ad, C, x3, keep_out=k3, **kw)
    assert torch.equal(k3.cpu(), mirror), (tag, "keep_out is not the Philox mirror", int((k3.cpu() != mirror).sum()))
    _check_act_out(tag + " x, Philox mask", x3, G.act_fwd_ref(a, C, ldx, kind, RATE, mirror)[1], C, x_dt)
    x4, k4 = filled((rows, ldx), x_dt), filled((rows, C))
    ops.act_fwd(ad, C, x4, keep_out=k4, **kw)
    assert bits_equal(x3, x4) and torch.equal(k3, k4)
    r0 = (rows // rps // 2) * rps if rows // rps >= 2 else rows // 2            # two shards, cut between two samples
    if rps == 1 or rows // rps >= 2:
        for lo, hi in ((0, r0), (r0, rows)):
            xs, ks = filled((hi - lo, ldx), x_dt), filled((hi - lo, C))
            ops.act_fwd(ad[lo:hi], C, xs, keep_out=ks, **dict(kw, sample_offset=OFFSET + lo // rps))
            assert bits_equal(xs, x3[lo:hi]) and torch.equal(ks, k3[lo:hi]), (tag, "shard", lo, hi)
    for other in (dict(stream_id=3), dict(step=STEP + 1), dict(seed=SEED + 1)):
        ko2 = filled((rows, C))
        ops.act_fwd(ad, C, filled((rows, ldx), x_dt), keep_out=ko2, **dict(kw, **other))
        assert not torch.equal(ko2, k3), (tag, "the draws do not depend on", other)
        assert torch.equal(ko2.cpu(), G.dropout_keep(rows, C, RATE, **{**dict(seed=SEED, step=STEP, stream_id=2), **other}, sample_offset=OFFSET, rows_per_sample=rps))


def test_act_fwd_philox_keep_fraction(ops):
    """48 x 128 draws at rate 0.3: the kept fraction within 4 binomial standard deviations of 0.7"""
    rows, C, lda, ldx, rps = G.ACT_SHAPES[2]
    k = filled((rows, C))
    ops.act_fwd(dev(G.act_inputs(rows, C, lda, 1)), C, filled((rows, ldx)), act="elu", rate=RATE, keep_out=k, seed=SEED, step=STEP, stream_id=1, rows_per_sample=rps)
    n = rows * C
    frac = float(k.double().mean())
    print("kept fraction %.4f of %d draws (sd %.4f)" % (frac, n, (0.7 * 0.3 / n) ** 0.5))
    assert set(k.unique().tolist()) <= {0.0, 1.0} and abs(frac - 0.7) <= 4.0 * (0.7 * 0.3 / n) ** 0.5


# ------------------------------------------------------------------------------------------------------------------- act_bwd
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("rows,C,lda,ldx,rps", G.ACT_SHAPES)
def test_act_bwd(ops, rows, C, lda, ldx, rps, bf16):
    """ga = (gx keep / (1 - rate) + gx2) act'(y_act), with and without gx2, with and without y_act; elu with stored outputs down to -1 + 6e-6 (-1 itself in bf16), where
    act' = y + 1 is a difference; relu and no activation once each.  The reference takes the stored y_act (fp32- or bf16-rounded) as the kernel does.  Pad columns of ga
    are zero."""
    dt = BF if bf16 else F32
    a = G.act_inputs(rows, C, lda, rows + C)
    keep = G.pinned_keep(rows, C, RATE, 5)
    for kind, with_y, with_g2, rate in (("elu", True, True, RATE), ("elu", True, False, RATE), ("elu", False, True, 0.0), ("elu", False, False, RATE),
                                        ("relu", True, True, 0.0), (None, True, True, RATE)):
        yr = G.act_fwd_ref(a, C, ldx, kind)[0]
        y = (G.bf16_rne(yr) if bf16 else yr.float().double()) if with_y else None           # the stored activation
        if kind == "elu" and with_y:
            assert float(y[:, :C].min()) < -0.99999
        gx, gx2 = G.grads_like(rows, C, ldx, 6, bf16), G.grads_like(rows, C, ldx, 7, bf16) if with_g2 else None
        if bf16 and (with_y or rate):                                             # (neither: ga = gx + gx2, exact in fp32 like sv_add -- a sum ON a tie rounds the same way)
            gx, gx2 = G.settled_act_bwd_grads(gx, gx2, C, y, kind, rate, keep, True)
        ref, scale = G.act_bwd_ref(gx, C, ldx, y, kind, rate, keep, gx2)
        ga = filled((rows, ldx), dt)
        ops.act_bwd(dev(gx, dt), C, ga, y_act=dev(y, dt) if with_y else None, act=kind, rate=rate, keep=dev(keep) if rate else None,
                    gx2=dev(gx2, dt) if with_g2 else None)
        what = "act_bwd %s %dx%d %s y_act %d gx2 %d" % (kind, rows, C, "bf16" if bf16 else "f32", with_y, with_g2)
        assert float(ga[:, C:].float().abs().max() if ldx > C else 0.0) == 0.0, (what, "pad columns are not zero")
        if bf16:
            same_bf16(what, ga, ref)
        else:
            close(what, ga, ref, scale)


def test_act_grid_stride(ops):
    """2100 x 1024 = 2 150 400 elements: more than the 8192 blocks x 256 threads grid_for allows, so the loops of act_fwd and act_bwd take a second trip; checked whole"""
    rows, ld, C = G.GRID_ROWS, G.GRID_LD, G.GRID_LD - 3
    a = G.act_inputs(rows, C, ld, 9)
    keep = G.pinned_keep(rows, C, RATE, 5)
    y, x = filled((rows, ld)), filled((rows, ld))
    ops.act_fwd(dev(a), C, x, act="elu", y_act=y, rate=RATE, keep_in=dev(keep))
    yr, xr = G.act_fwd_ref(a, C, ld, "elu", RATE, keep)
    close("act_fwd grid-stride y_act", y, yr)
    close("act_fwd grid-stride x", x, xr)
    gx, gx2 = G.grads_like(rows, C, ld, 6), G.grads_like(rows, C, ld, 7)
    ga = filled((rows, ld))
    ops.act_bwd(dev(gx), C, ga, y_act=y, act="elu", rate=RATE, keep=dev(keep), gx2=dev(gx2))
    ref, scale = G.act_bwd_ref(gx, C, ld, y.cpu(), "elu", RATE, keep, gx2)
    close("act_bwd grid-stride ga", ga, ref, scale)
    assert float(ga[:, C:].abs().max()) == 0.0 and float(x[:, C:].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------------------- add
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("n", G.ADD_N)
def test_add(ops, n, bf16):
    """out = a + b; 2 100 000 elements loop.  bf16: the fp32 sum of two bf16 numbers is exact unless it rounds to the larger one anyway, so equality holds everywhere"""
    dt = BF if bf16 else F32
    a, b = G.add_inputs(n, n, bf16)
    out = filled((n + 1,), dt)
    ops.add(dev(a, dt), dev(b, dt), out[:n])
    assert float(out[n]) == 3.0
    if bf16:
        same_bf16("add bf16 n %d" % n, out[:n], G.add_ref(a, b))
    else:
        close("add f32 n %d" % n, out[:n], G.add_ref(a, b), torch.maximum(a.abs(), b.abs()).double())


# ------------------------------------------------------------------------------------------------------------------- Gumbel softmax
UNDERFLOW = 1e-35     # fp32 cannot hold y below 2^-126 ~ 1.2e-38 to full precision (logits over +-40: y underflows); the formulas multiply it by less than 1000


def _gumbel_case(ops, B, K, tau, ldl, ld_lp, scale=1.0):
    tag = "gumbel B %d K %d tau %.1f ld %d/%d%s" % (B, K, tau, ldl, ld_lp, " +-40" if scale != 1.0 else "")
    logits, u, gy = G.gumbel_inputs(B, K, ldl, B * K, scale)
    ld, ud = dev(logits), dev(u)
    y, y_lp, u_out = filled((B, K)), filled((B, ld_lp)), filled((B, K))
    ops.gumbel_softmax_fwd(ld, K, tau, y, y_lp, u=ud, u_out=u_out)
    ref = G.gumbel_fwd_ref(logits[:, :K], u, tau)
    close(tag + " y", y, ref, floor=UNDERFLOW)
    assert float((y.double().sum(dim=1) - 1.0).abs().max()) <= 1e-6
    assert torch.equal(y_lp[:, :K], y) and float(y_lp[:, K:].abs().max() if ld_lp > K else 0.0) == 0.0
    assert bits_equal(u_out.cpu(), G.clamp_u(u)), (tag, "u_out is not the clamped u")
    yb = filled((B, ld_lp), BF)
    y_again = filled((B, K))
    ops.gumbel_softmax_fwd(ld, K, tau, y_again, yb, u=ud)
    assert bits_equal(y_again, y) and bits_equal(yb[:, :K].contiguous(), y.to(BF)) and float(yb[:, K:].float().abs().max() if ld_lp > K else 0.0) == 0.0
    if scale != 1.0:
        p = torch.softmax(logits[:, :K].double(), dim=1)
        assert float(p.min()) < 1e-12                                            # log(p + 1e-8) on its floor
    # backward
    alpha_over_B = 3.0 / B
    gref, gscale, klref, klscale = G.gumbel_bwd_ref(gy, logits[:, :K], u, tau, alpha_over_B)
    gyd = dev(torch.cat([gy, torch.full((B, 1), 9.0)], dim=1))                    # ldg = K + 1
    g, kl = filled((B, ld_lp)), filled((B,))
    ops.gumbel_softmax_bwd(gyd, y, ld, K, tau, alpha_over_B, g, kl)
    close(tag + " g_logits", g[:, :K], gref, gscale, floor=UNDERFLOW)
    close(tag + " y_kl", kl, klref, klscale)
    assert float(g[:, K:].abs().max() if ld_lp > K else 0.0) == 0.0
    gb, klb = filled((B, ld_lp), BF), filled((B,))
    ops.gumbel_softmax_bwd(gyd, y, ld, K, tau, alpha_over_B, gb, klb)
    assert bits_equal(gb, g.to(BF)) and bits_equal(klb, kl)
    kl_eval = filled((B,))
    ops.gumbel_softmax_bwd(None, y, ld, K, tau, alpha_over_B, None, kl_eval)
    assert bits_equal(kl_eval, kl), (tag, "the evaluation call's y_kl differs from the training call's")


@pytest.mark.parametrize("tau", [0.5, 1.0])
@pytest.mark.parametrize("B,K", G.GUMBEL_SHAPES)
def test_gumbel_softmax(ops, B, K, tau):
    """forward and adjoint with a supplied u that holds 0, 2^-24, 1 - 2^-24 and 1 (the clamp is part of the contract); ld_logits = K + 3 for the odd K;
    ld_lp = 8 ceil(K / 8); fp32 and bf16 y_lp / g_logits"""
    _gumbel_case(ops, B, K, tau, K + 3 if K % 2 else K, (K + 7) // 8 * 8)


def test_gumbel_softmax_wide_pad_and_large_logits(ops):
    """K = 10 in a 128-wide y_lp (the second column of every lane is padding); logits over +-40: p underflows next to 1e-8, y underflows to 0"""
    _gumbel_case(ops, 5, 10, 1.0, 13, 128)
    _gumbel_case(ops, 9, 127, 0.5, 130, 128, scale=40.0)
    _gumbel_case(ops, 5, 10, 1.0, 10, 16, scale=40.0)


@pytest.mark.parametrize("B,K", [(7, 65), (6, 128), (5, 10)])
def test_gumbel_softmax_philox(ops, B, K):
    """u = NULL: u_out is the clamped mirror draw bit for bit, two calls agree, and rows [r0, B) of the batch equal a call on those rows at sample_offset + r0"""
    logits, _, _ = G.gumbel_inputs(B, K, K, B * K)
    ld = dev(logits)
    ld_lp = (K + 7) // 8 * 8
    outs = []
    for _ in range(2):
        y, y_lp, u_out = filled((B, K)), filled((B, ld_lp)), filled((B, K))
        ops.gumbel_softmax_fwd(ld, K, 0.5, y, y_lp, u_out=u_out, seed=SEED, step=STEP, sample_offset=OFFSET)
        outs.append((y, y_lp, u_out))
    assert all(bits_equal(p, q) for p, q in zip(*outs))
    y, y_lp, u_out = outs[0]
    mirror = G.gumbel_uniforms(B, K, SEED, STEP, OFFSET)
    assert bits_equal(u_out.cpu(), G.clamp_u(mirror)), "u_out is not the Philox mirror"
    close("gumbel Philox B %d K %d y" % (B, K), y, G.gumbel_fwd_ref(logits, mirror, 0.5), floor=UNDERFLOW)
    r0 = B // 2
    ys, us = filled((B - r0, K)), filled((B - r0, K))
    ops.gumbel_softmax_fwd(ld[r0:], K, 0.5, ys, filled((B - r0, ld_lp)), u_out=us, seed=SEED, step=STEP, sample_offset=OFFSET + r0)
    assert bits_equal(ys, y[r0:]) and bits_equal(us, u_out[r0:])
    u2 = filled((B, K))
    ops.gumbel_softmax_fwd(ld, K, 0.5, filled((B, K)), filled((B, ld_lp)), u_out=u2, seed=SEED, step=STEP + 1, sample_offset=OFFSET)
    assert not torch.equal(u2, u_out)


# ------------------------------------------------------------------------------------------------------------------- the heads
Z_COL = 3


def _head_fwd(ops, ins, lp_dtype, eps=True, **kw):
    a_m, a_s, a_pm, a_ps, e, _ = ins
    B, L = a_m.shape
    o = {k: filled((B, L)) for k in ("zm", "zs", "z", "pm", "ps", "eps_out")}
    o["zcat"], o["kl2"] = filled((B, Z_COL + L + 5), lp_dtype), filled((B,))
    ops.gm_head_fwd(dev(a_m), dev(a_s), dev(a_pm), dev(a_ps), o["zm"], o["zs"], o["z"], o["pm"], o["ps"], o["zcat"], Z_COL, o["kl2"],
                    eps=dev(e) if eps else None, eps_out=o["eps_out"], **kw)
    return o


def _pin_report(what, got, ref, B):
    """the worst relative error of each pinned row (the figure LAB_NOTES.md keeps before and after the softplus-adjoint fix)"""
    got, ref = got.detach().double().cpu(), ref.double()
    for v, r in sorted(G.pinned_rows(B, prior=not what.endswith("g_a_sig")).items()):
        print("%-58s row pinned at %+5.0f: worst rel %.3e" % (what, v, float(((got[r] - ref[r]).abs() / ref[r].abs()).max())))


@pytest.mark.parametrize("lp_bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,L", G.HEAD_SHAPES)
def test_gm_head_fwd_bwd(ops, B, L, lp_bf16):
    """The posterior / prior heads and their adjoint.  z_col = 3 and ldz = z_col + L + 5 in a sentinel-filled zcat; a_sig / a_prior_sig ~ N(0, 1.5) with whole rows pinned
    at -7, -9, -11, -14 (sigma 9e-4 .. 8e-7) and +12.  Backward: autograd of sum(dz z) + kl_scale sum(kl2), ld_dz = L + 3, fp32 and bf16 gradient outputs.
    On the library before the softplus adjoint was taken with expm1f, the g_a_sig / g_a_prior_sig rows pinned at -9 and below missed the 1e-4 bar (LAB_NOTES.md)."""
    dt = BF if lp_bf16 else F32
    tag = "gm_head B %d L %d" % (B, L)
    ins = G.head_inputs(B, L, B + L)
    a_m, a_s, a_pm, a_ps, eps, dz = ins
    o = _head_fwd(ops, ins, dt)
    r = G.gm_head_fwd_ref(a_m, a_s, a_pm, a_ps, eps)
    assert torch.equal(o["zm"].cpu(), a_m) and torch.equal(o["pm"].cpu(), a_pm) and torch.equal(o["eps_out"].cpu(), eps)
    close(tag + " z_sig", o["zs"], r["zs"])
    close(tag + " prior_sig", o["ps"], r["ps"])
    close(tag + " z", o["z"], r["z"], r["z_scale"])
    close(tag + " kl2", o["kl2"], r["kl2"], r["kl2_scale"])
    zc = o["zcat"]
    assert bits_equal(zc[:, Z_COL:Z_COL + L].contiguous(), o["z"].to(dt)), "z_lp is not the cast of z"
    assert bool((zc[:, :Z_COL] == 3.0).all()) and bool((zc[:, Z_COL + L:] == 3.0).all()), "columns outside [z_col, z_col + L) were written"
    # backward
    c = 40.0 / B
    dzd = dev(torch.cat([dz, torch.full((B, 3), 9.0)], dim=1))
    grads, scales = G.gm_head_bwd_ref(dz, a_m, a_s, a_pm, a_ps, eps, c)
    g = [filled((B, L), dt) for _ in range(4)]
    ops.gm_head_bwd(dzd, o["zm"], o["zs"], o["pm"], o["ps"], o["eps_out"], c, *g)
    names = ("g_a_mean", "g_a_sig", "g_a_prior_mean", "g_a_prior_sig")
    if lp_bf16:                                                              # the bf16 outputs are the rounded fp32 outputs, which the f32 case holds to the rule
        g32 = [filled((B, L)) for _ in range(4)]
        ops.gm_head_bwd(dzd, o["zm"], o["zs"], o["pm"], o["ps"], o["eps_out"], c, *g32)
        assert all(bits_equal(a, b.to(BF)) for a, b in zip(g, g32))
        g = g32
    for k in (1, 3):
        _pin_report(tag + " " + names[k], g[k], grads[k], B)
    for k in range(4):
        close(tag + " " + names[k], g[k], grads[k], scales[k])


def test_gm_head_bwd_grid_stride(ops):
    """B = 2100, L = 1024: the adjoint's loop takes a second trip; the whole result against autograd"""
    B, L = G.GRID_ROWS, G.GRID_LD
    ins = G.head_inputs(B, L, 17)
    a_m, a_s, a_pm, a_ps, eps, dz = ins
    o = _head_fwd(ops, ins, F32)
    c = 40.0 / B
    grads, scales = G.gm_head_bwd_ref(dz, a_m, a_s, a_pm, a_ps, eps, c)
    g = [filled((B, L)) for _ in range(4)]
    ops.gm_head_bwd(dev(dz), o["zm"], o["zs"], o["pm"], o["ps"], o["eps_out"], c, *g)
    for k, name in enumerate(("g_a_mean", "g_a_sig", "g_a_prior_mean", "g_a_prior_sig")):
        close("gm_head_bwd grid-stride " + name, g[k], grads[k], scales[k])


def test_gm_head_philox_eps(ops):
    """eps = NULL, B = 64, L = 128: eps_out against the Box-Muller mirror (Philox words bit for bit, the angle formed in fp32 as the kernel forms it, log / sqrt / cos in
    float64) within 1e-6 -- what logf, sqrtf, cosf and the final product round; reproducible; shard-invariant; mean and std within 0.05"""
    B, L = 64, 128
    ins = G.head_inputs(B, L, 5)
    kw = dict(seed=SEED, step=STEP, sample_offset=OFFSET)
    o1, o2 = _head_fwd(ops, ins, F32, eps=False, **kw), _head_fwd(ops, ins, F32, eps=False, **kw)
    assert all(bits_equal(o1[k], o2[k]) for k in o1)
    e = o1["eps_out"].double().cpu()
    err = float((e - G.head_eps(B, L, SEED, STEP, OFFSET)).abs().max())
    print("gm_head Philox eps: worst |eps_out - mirror| %.3e, mean %.4f, std %.4f" % (err, float(e.mean()), float(e.std())))
    assert err <= 1e-6
    assert abs(float(e.mean())) <= 0.05 and abs(float(e.std()) - 1.0) <= 0.05
    r = G.gm_head_fwd_ref(*ins[:4], e)
    close("gm_head Philox z", o1["z"], r["z"], r["z_scale"])
    r0 = 24
    os_ = _head_fwd(ops, tuple(t[r0:] for t in ins), F32, eps=False, **dict(kw, sample_offset=OFFSET + r0))
    assert bits_equal(os_["eps_out"], o1["eps_out"][r0:]) and bits_equal(os_["z"], o1["z"][r0:])
    o3 = _head_fwd(ops, ins, F32, eps=False, **dict(kw, step=STEP + 1))
    assert not torch.equal(o3["eps_out"], o1["eps_out"])


# ------------------------------------------------------------------------------------------------------------------- metrics
@pytest.mark.parametrize("B", G.METRICS_B)
def test_gm_metrics(ops, B):
    """the five batch means and the total, positive terms of magnitudes 1e3, 1e1, 1e3, 1e1, 1e-1.  rtol = (ceil(B / 256) + 8) 2^-24 * 2: the serial adds of a thread plus
    the 8 levels of the tree, times 2 for the division and the final combination -- derived, not measured.  Two launches are bit-equal."""
    terms = G.metrics_inputs(B, B)
    td = [dev(t) for t in terms]
    out = filled((8,))
    ops.gm_metrics(*td, 40.0, 3.0, out[:6])
    assert float(out[6]) == 3.0 and float(out[7]) == 3.0
    close("gm_metrics B %d" % B, out[:6], G.gm_metrics_ref(terms, 40.0, 3.0), rtol=G.gm_metrics_rtol(B), scale=torch.zeros(6, dtype=F64))
    again = filled((8,))
    ops.gm_metrics(*td, 40.0, 3.0, again[:6])
    assert bits_equal(out, again)
