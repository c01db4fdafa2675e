"""No GPU: self-checks of tests/gm_pointwise_ref.py, so that tests/test_gpu_gm_pointwise.py cannot pass because its reference is wrong -- the autograd
references against closed forms, the Philox mirrors against Random123's known answers, and every input generator of the GPU tests kept finite (and, for the
bf16 cases, away from the rounding ties) in the float64 reference."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gm_pointwise_ref as G  # noqa: E402
import tape_ref as T  # noqa: E402

F64 = torch.float64


@pytest.mark.parametrize("K", [2, 10, 128])
def test_gumbel_backward_autograd_is_the_kernels_closed_form(K):
    """autograd of sum(gy * y) + alpha_over_B * sum y_kl == (1 / tau) y (gy - <y, gy>) + alpha_over_B p (f - <p, f>), in float64"""
    for scale, tau in ((1.0, 0.5), (40.0, 1.0)):
        logits, u, gy = G.gumbel_inputs(5, K, K + 3, 10 + K, scale)
        g, sc, kl, _ = G.gumbel_bwd_ref(gy, logits[:, :K], u, tau, 0.37)
        y = G.gumbel_fwd_ref(logits[:, :K], u, tau)
        want = G.gumbel_bwd_closed_form(gy, y, logits[:, :K], tau, 0.37)
        assert float((g - want).abs().max()) <= 1e-12 * float(sc.max())
        assert bool((sc >= 0).all()) and bool(((g - want).abs() <= 1e-10 * sc + 1e-300).all())
        p = torch.softmax(logits[:, :K].double(), dim=1)
        assert torch.allclose(kl, (p * (torch.log(p + 1e-8) + math.log(K))).sum(dim=1), rtol=1e-13, atol=0)


def test_head_backward_autograd_has_a_true_sigmoid():
    """the sigma gradient of the heads, by hand with sigmoid(a) as softplus', equals the autograd reference -- on the pinned rows too"""
    a_m, a_s, a_pm, a_ps, eps, dz = G.head_inputs(7, 65, 3)
    c = 40.0 / 7
    (gm, gs, gm2, gs2), scales = G.gm_head_bwd_ref(dz, a_m, a_s, a_pm, a_ps, eps, c)
    m, m2, e, g = a_m.double(), a_pm.double(), eps.double(), dz.double()
    s, s2 = G.softplus(a_s.double()), G.softplus(a_ps.double())
    d = m - m2
    want = (g + c * d / s2 ** 2, (g * e + c * (s / s2 ** 2 - 1 / s)) * torch.sigmoid(a_s.double()), -c * d / s2 ** 2,
            c * (1 / s2 - (s * s + d * d) / s2 ** 3) * torch.sigmoid(a_ps.double()))
    for v, w, sc in zip((gm, gs, gm2, gs2), want, scales):                  # (both sides are cancelling float64 sums: judged by the scale)
        assert bool(((v - w).abs() <= 1e-13 * sc).all())
    for v, sc in zip((gm, gs, gm2, gs2), scales):
        assert bool((v.abs() <= 3.0 * sc * (1 + 1e-12)).all())            # at most three addends, each at most the scale


def test_act_backward_reference():
    """act_bwd_ref == (gx keep / (1 - rate) + gx2) * act'(pre) for the pre-activations themselves; act_inverse reproduces the activation"""
    for kind in (None, "relu", "elu"):
        a = G.act_inputs(7, 13, 16, 1).double()
        y, _ = G.act_fwd_ref(a, 13, 16, kind)
        assert torch.equal(G.act(G.act_inverse(y[:, :13], kind), kind)[a[:, :13] > 0], y[:, :13][a[:, :13] > 0])
        assert torch.allclose(G.act(G.act_inverse(y[:, :13], kind), kind), y[:, :13], rtol=1e-15, atol=0)
        keep = G.pinned_keep(7, 13, 0.3, 2)
        gx, gx2 = G.grads_like(7, 13, 16, 3), G.grads_like(7, 13, 16, 4)
        ga, sc = G.act_bwd_ref(gx, 13, 20, y, kind, 0.3, keep, gx2)
        d = {None: torch.ones(7, 13, dtype=F64), "relu": (a[:, :13] > 0).double(), "elu": torch.where(a[:, :13] > 0, 1.0, torch.exp(a[:, :13]))}[kind]
        want = (gx[:, :13].double() * keep.double() / (1 - G.rate64(0.3)) + gx2[:, :13].double()) * d
        assert torch.allclose(ga[:, :13], want, rtol=1e-9, atol=1e-300) and float(ga[:, 13:].abs().max()) == 0.0
        assert bool((ga.abs() <= 2.0 * sc * (1 + 1e-9)).all())


def test_metrics_reference_total_is_the_weighted_sum():
    for B in G.METRICS_B:
        t = G.metrics_inputs(B, B)
        out = G.gm_metrics_ref(t, 40.0, 3.0)
        m = [float(v.double().sum()) / B for v in t]
        assert all(abs(float(out[k]) - m[k]) <= 1e-13 * m[k] for k in range(5))
        assert abs(float(out[5]) - (m[0] + m[2] + 40.0 * (m[1] + m[3]) + 3.0 * m[4])) <= 1e-13 * float(out[5])
        assert 9 * 2.0 ** -23 <= G.gm_metrics_rtol(B) <= 12 * 2.0 ** -23


def test_philox_mirrors():
    """tape_ref.philox4x32_10 under the known answers of tests/test_tape_host.py::test_philox_mirror_known_answers, and the counter / key layout of philox_unit and
    head_eps spelled out on single draws"""
    z = T.philox4x32_10(np.zeros((1, 4), np.uint32), 0)[0]
    assert [int(v) for v in z] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    f = T.philox4x32_10(np.full((1, 4), 0xFFFFFFFF, np.uint32), 0xFFFFFFFFFFFFFFFF)[0]
    assert [int(v) for v in f] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    seed, step, sid, gs, col = 0x1234567890ABCDEF, (3 << 32) | 5, 9, (7 << 32) | 11, 300
    w = T.philox4x32_10(np.array([[col, 11, 7 ^ (0x676d0000 + sid), 5]], np.uint32), seed ^ 0x6d76616547)[0]
    u = G.philox_unit(seed, step, sid, gs, col)
    assert float(u) == ((int(w[0]) >> 8) + 1) / 2.0 ** 24 and 0.0 < float(u) <= 1.0
    w = T.philox4x32_10(np.array([[2, 11, 0x65707300, 5]], np.uint32), seed ^ 0xe9515eed)[0]
    u0, u1 = ((int(w[0]) >> 8) + 1) / 2.0 ** 24, ((int(w[1]) >> 8) + 1) / 2.0 ** 24
    e = G.head_eps(1, 3, seed, step, sample_offset=11)[0, 2]
    assert abs(float(e) - math.sqrt(-2 * math.log(u0)) * math.cos(2 * math.pi * u1)) <= 3e-6
    # shards: rows of a later offset are the rows of the whole draw
    assert torch.equal(G.gumbel_uniforms(3, 10, 5, 2, sample_offset=4), G.gumbel_uniforms(7, 10, 5, 2)[4:])
    assert torch.equal(G.dropout_keep(32, 8, 0.3, 5, 2, 1, sample_offset=1, rows_per_sample=16), G.dropout_keep(48, 8, 0.3, 5, 2, 1, rows_per_sample=16)[16:])
    assert torch.equal(G.head_eps(2, 65, 5, 2, sample_offset=3), G.head_eps(5, 65, 5, 2)[3:])


def test_bf16_rounding_helpers():
    x = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -40, -3.14159, 1e-3, 255.5, 0.0], dtype=F64)
    r = G.bf16_rne(x)
    assert r.tolist()[:4] == [1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7]                # ties to even; just above a tie goes up (float32 in between would not)
    assert torch.equal(r[4:], x[4:].float().bfloat16().double())
    assert float(G.tie_distance(x)[1]) == 0.0 and abs(float(G.tie_distance(x)[0]) - 2.0 ** -8) < 1e-18
    assert G.bf16_ulp(x)[:2].tolist() == [2.0 ** -7, 2.0 ** -7]


def _finite(*ts):
    return all(bool(torch.isfinite(t).all()) for t in ts)


def test_generators_stay_finite_in_the_reference():
    """every input set of tests/test_gpu_gm_pointwise.py through its float64 reference: finite values and finite, non-negative scales; sigma >= 5e-7 so that
    log sigma and 1 / sigma exist; the planted edge values are there"""
    for rows, C, lda, ldx, rps in G.ACT_SHAPES:
        for bf in (False, True):
            a = G.act_inputs(rows, C, lda, rows, bf)
            assert float(a[:, :C].min()) >= -12.0 and float(a[:, :C].max()) <= 6.0 and float(a[:, :C].min()) < -11.0 and float(a[:, :C].max()) > 5.0
            for kind in (None, "relu", "elu"):
                y, x = G.act_fwd_ref(a, C, ldx, kind, 0.3, G.pinned_keep(rows, C, 0.3, 5))
                assert _finite(y, x) and float(y[:, C:].abs().max() if ldx > C else 0.0) == 0.0
                ga, sc = G.act_bwd_ref(G.grads_like(rows, C, ldx, 6), C, ldx, y, kind, 0.3, G.pinned_keep(rows, C, 0.3, 5), G.grads_like(rows, C, ldx, 7))
                assert _finite(ga, sc) and bool((sc >= 0).all())
        y, _ = G.act_fwd_ref(G.act_inputs(rows, C, lda, rows), C, ldx, "elu")
        assert float(y[:, :C].min()) < -0.99999                                           # elu outputs near -1: act' = y + 1 is a cancelling difference
    for B, K in G.GUMBEL_SHAPES:
        for scale in (1.0, 40.0):
            logits, u, gy = G.gumbel_inputs(B, K, K + 3, B * K, scale)
            assert float(u.min()) == 0.0 and (B * K < 4 or float(u.max()) == 1.0)
            uc = G.clamp_u(u)
            assert float(uc.min()) == float(np.float32(1e-20)) and float(uc.max()) <= 1.0 - 2.0 ** -24
            for tau in (0.5, 1.0):
                y = G.gumbel_fwd_ref(logits[:, :K], u, tau)
                g, sc, kl, ksc = G.gumbel_bwd_ref(gy, logits[:, :K], u, tau, 0.6)
                assert _finite(y, g, sc, kl, ksc) and float((y.sum(dim=1) - 1).abs().max()) < 1e-12
    logits, _, _ = G.gumbel_inputs(9, 127, 130, 9 * 127, 40.0)
    p = torch.softmax(logits[:, :127].double(), dim=1)
    assert float(p.min()) < 1e-30 and float(p.float().min()) > 2.0 ** -126                # log(p + 1e-8) on its floor; p itself still a normal fp32 number
    for B, L in G.HEAD_SHAPES + ((G.GRID_ROWS, G.GRID_LD),):
        a_m, a_s, a_pm, a_ps, eps, dz = G.head_inputs(B, L, B + L)
        r = G.gm_head_fwd_ref(a_m, a_s, a_pm, a_ps, eps)
        assert _finite(*r.values()) and float(r["zs"].min()) >= 5e-7 and float(r["ps"].min()) >= 5e-7
        assert _finite(torch.log(r["zs"]), 1 / r["zs"], torch.log(r["ps"]), 1 / r["ps"])
        grads, scales = G.gm_head_bwd_ref(dz, a_m, a_s, a_pm, a_ps, eps, 40.0 / B)
        assert _finite(*grads) and _finite(*scales) and _finite(*(t.float() for t in grads))
        for v, k in G.pinned_rows(B).items():
            assert bool((a_s[k] == v).all()) and bool((a_ps[G.pinned_rows(B, prior=True)[v]] == v).all())
            assert B < 3 or k != G.pinned_rows(B, prior=True)[v]
    assert set(G.pinned_rows(5)) == set(G.PINS) and abs(float(G.softplus(torch.tensor(-14.0, dtype=F64))) - 8.3e-7) < 1e-8
    for B in G.METRICS_B:
        assert all(bool((t > 0).all()) for t in G.metrics_inputs(B, B))


def test_pinned_dropout_masks_leave_no_row_empty():
    """(no GPU test divides by a row norm today; the generator keeps the property so that one may)"""
    for rows, C, _, _, _ in G.ACT_SHAPES:
        k = G.pinned_keep(rows, C, 0.3, 5)
        assert float(k.sum(dim=1).min()) >= 1.0 and set(k.unique().tolist()) <= {0.0, 1.0}
        assert abs(float(k.mean()) - 0.7) < 0.1


@pytest.mark.parametrize("kind", [None, "relu", "elu"])
def test_bf16_cases_are_settled_away_from_the_ties(kind):
    """what settle_away_from_ties promises: no y_act, x or ga of a bf16 case within 8 fp32 ulps (of its largest addend) of a bf16 rounding tie"""
    rows, C, lda, ldx, _ = G.ACT_SHAPES[0]
    keep = G.pinned_keep(rows, C, 0.3, 5)
    for bf in (False, True):
        a = G.settled_act_inputs(rows, C, lda, 11, kind, 0.3, bf)
        assert (not bf) or torch.equal(a, G.as_bf16(a))
        y, x = G.act_fwd_ref(a, C, lda, kind, 0.3, torch.ones(rows, C))
        for r in (y, x):
            nz = r != 0
            assert bool((G.tie_distance(r)[nz] > G.TIE_BAND * r.abs()[nz]).all())
        yb = G.bf16_rne(y)
        gx, gx2 = G.settled_act_bwd_grads(G.grads_like(rows, C, lda, 6, True), G.grads_like(rows, C, lda, 7, True), C, yb, kind, 0.3, keep, True)
        assert torch.equal(gx, G.as_bf16(gx)) and torch.equal(gx2, G.as_bf16(gx2))
        ga, sc = G.act_bwd_ref(gx, C, lda, yb, kind, 0.3, keep, gx2)
        nz = ga != 0
        assert bool((G.tie_distance(ga)[nz] > G.TIE_BAND * sc[nz]).all())
