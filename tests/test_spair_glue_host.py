"""CPU: the float64 references of tests/spair_glue_ref.py -- by hand on tiny inputs and against oracle/spair_ref.py with torch autograd (two float64
statements of one formula: 1e-12) --, the conditions their case tables must meet (no sampling point of a random STN case within its coordinate bound of a
grid line, no noise-moved value whose fp32 sum falls on the other side of a clip gate), the MUTANTS (plausible wrong kernels applied to the reference,
rounded to fp32 and judged by the comparison the GPU test uses: each must be rejected on at least one case of the tables -- this list is what
tests/test_gpu_spair_glue.py can see), and the refusals of the four kernels' entry points, which return before anything is enqueued."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spair_glue_ref as R  # noqa: E402
from oracle import spair_model_ref as M  # noqa: E402
from oracle import spair_ref as O  # noqa: E402

AGREE = 1e-12


def T(a, grad=False):
    return torch.tensor(np.asarray(a), dtype=torch.float64, requires_grad=grad)


def rel(mine, theirs, scale=1.0, floor=1e-300):
    theirs = theirs.detach().numpy() if torch.is_tensor(theirs) else np.asarray(theirs)
    return float(np.abs(mine - theirs.reshape(mine.shape)).max() / max(float(np.abs(theirs).max()), floor)) / scale


# ---------------------------------------------------------------------------------------------------------------- the V arithmetic itself
def test_error_arithmetic_by_hand():
    u = R.U
    a, b = R.V(3.0, 2 * u), R.V(-4.0, u)
    assert (a + b).e == 3 * u + u * 1.0 and (a - b).e == 3 * u + u * 7.0
    assert (a * b).e == 3.0 * u + 4.0 * 2 * u + 2 * u * u + u * 12.0
    assert a.x2(0.5).v == 1.5 and a.x2(0.5).e == u
    q = a / b
    assert q.v == -0.75 and abs(q.e - ((2 * u + 0.75 * u) / (4.0 - u) + R.E_DIV * u * 0.75)) < 1e-22
    s = R.vsum(R.V([1.0, -2.0, 4.0], [u, 0, u]), -1, 5)
    assert s.v == 3.0 and s.e == 2 * u + 5 * u * 7.0
    assert R.vsigmoid(R.V(0.0)).e == 0.0 and R.vsigmoid(R.V(0.0)).v == 0.5              # the exact .5 of logit 0
    assert float(R.c32(1e-8).e) == u * 1e-8 and abs(R.A_MIN32 - 1e-8) <= u * 1e-8
    # judge: inside the widened interval, outside it, unwritten, and an error where nothing is allowed
    ref = (np.array([1.0, 1.0, 1.0, 0.0]), np.array([2.0, 2.0, 2.0, 0.0]), np.array([0.5, 0.5, 0.5, 0.0]))
    assert R.judge(np.array([0.6, 2.4, 1.5, 0.0]), ref)[0] == pytest.approx(0.8)
    assert R.judge(np.array([1.5, 3.0, 1.5, 0.0]), ref) == (2.0, 1)
    assert R.judge(np.array([1.5, 1.5, np.nan, 0.0]), ref) == (np.inf, 2)
    assert R.judge(np.array([1.5, 1.5, 1.5, 1e-30]), ref) == (np.inf, 3)


def test_small_reciprocals_are_exact():
    """m * fl(1 / m) == 1 in IEEE fp32 for m = 1 .. 16: what spair_glue_ref._pg relies on"""
    for m in range(1, 17):
        assert np.float32(m) * (np.float32(1.0) / np.float32(m)) == np.float32(1.0), m


# ---------------------------------------------------------------------------------------------------------------- STN
def test_stn_by_hand():
    """2 x 2 cells, z = 0 (sx = sy = .25, t = the bias), a 2 x 2 one-channel image, one output pixel (gx = gy = -1): cell 0 samples (0, 0) exactly, cell 3
    samples (.75, .75); forward form"""
    img = np.array([[1.0, 2.0], [4.0, 8.0]]).reshape(1, 2, 2, 1)
    z = np.zeros((1, 2, 2, 4))
    r = R._stn_core(img, z, 1, 1, False, np.ones((1, 4, 1, 1, 1)), True, None, (0, 0))
    out = r["out"].v.reshape(4)
    assert out[0] == 1.0 and out[3] == 0.0625 * 1 + 0.1875 * 2 + 0.1875 * 4 + 0.5625 * 8
    assert r["x"].reshape(4).tolist() == [0.0, 0.75, 0.0, 0.75] and r["y"].reshape(4).tolist() == [0.0, 0.0, 0.75, 0.75]
    assert r["cell"].bbox.v[0, 0].tolist() == [0.0, 0.0, 0.25, 0.25] and r["cell"].bbox.v[0, 3].tolist() == [0.75, 0.75, 1.0, 1.0]
    # g_img: the four cells' tap weights added per pixel; (0, 0): 1 + .25 + .25 + .0625
    assert r["g_img"].v.reshape(4)[0] == 1.5625 and r["g_img"].v.sum() == 4.0
    assert bool(r["fold"].reshape(4)[0]) and not bool(r["fold"].reshape(4)[3])           # cell 0 sits ON pixel (0, 0)
    # d out / d x of cell 3 = wy0 (I01 - I00) + wy1 (I11 - I10) = .25 + .75 * 4; times (W - 1)/2 = .5: the tx addend
    assert r["T"][2].v.reshape(4)[3] == 0.5 * (0.25 * 1 + 0.75 * 4)


STN_ORACLE = [c for c in R.stn_cases() if c[2] != "crafted" and not c[0][0].startswith("workload")] + \
             [c for c in R.stn_cases() if c[0][0].startswith("workload") and c[2] == "normal"]


@pytest.mark.parametrize("case", STN_ORACLE, ids=R.stn_case_id)
def test_stn_reference_agrees_with_the_oracle_and_its_autograd(case):
    img, z, g, res = R.stn_reference(case)
    (_, Hc, Wc, H, W, Cc, Ho, Wo, _), inverse, fam = case
    ri, rz = T(img, True), T(z, True)
    ref, rbox = O.stn_forward(ri, rz, Ho, Wo, inverse=inverse)
    (ref * T(g)).sum().backward()
    # coordinates of magnitude |sx| (W - 1) carry |sx| (W - 1) float64 roundings into weights of magnitude 1 (saturated inverse cases: sx -> 1e5)
    # -- and where every point is outside the image the oracle's w I - w I leaves 1e-16-sized noise around this file's exact zeros: the saturated family is
    # held to 1e-12 of max(|oracle|, 1), the normal family to 1e-12 of |oracle|
    scale = max(1.0, float(np.abs(res["cell"].sx.v).max()) * max(H, W))
    floor = 1.0 if fam == "saturated" else 1e-300
    assert not res["fold"].any()
    for name, theirs in (("out", ref), ("bbox", rbox), ("g_img", ri.grad), ("g_z", rz.grad)):
        lo, hi, _ = res[name]
        assert np.array_equal(lo, hi)
        assert rel(lo, theirs, scale, floor) <= AGREE, (name, rel(lo, theirs), scale)


@pytest.mark.parametrize("case", R.stn_cases(), ids=R.stn_case_id)
def test_stn_random_cases_have_no_fold_and_crafted_ones_do(case):
    img, z, g, res = R.stn_reference(case)
    (_, Hc, Wc, H, W, Cc, Ho, Wo, _), inverse, fam = case
    n = len(R.fold_pixels(case))
    assert n == int(res["fold"].sum())
    c = R.stn_c(res, W, H)
    print("%-40s fold pixels %d of %d   c = %.1f   largest m_x %.2e px" % (R.stn_case_id(case), n, res["fold"].size, c, float(res["mx"].max())))
    if fam != "crafted":
        assert n == 0
        return
    lo, hi, e = res["out"]
    if not inverse:
        assert n > 0                                         # z = 0: exact sampling points, some of them pixel centres
        x, y = res["x"], res["y"]
        # the pushed-out cell: gx = -1 lands exactly on the last column, everything else beyond it
        assert (x[:, -1] >= W - 1).all() and (x[:, -1] == W - 1).any()
        B = lo.shape[0]
        lo, hi = lo.reshape(B, Hc * Wc, Ho * Wo, Cc), hi.reshape(B, Hc * Wc, Ho * Wo, Cc)
        far = x[:, -1] - res["mx"][:, -1] > W - 1
        assert (far.any() or Wo == 1) and (lo[:, -1][far] == 0).all() and (hi[:, -1][far] == 0).all()


def test_crafted_cases_cover_the_three_edges():
    """over the crafted forward cases: a point exactly on an interior pixel centre, one exactly on the last column, and a cell wholly outside the image"""
    interior = last = outside = False
    for case in R.stn_cases():
        if case[2] != "crafted" or case[1]:
            continue
        res = R.stn_reference(case)[3]
        (_, Hc, Wc, H, W, Cc, Ho, Wo, _) = case[0]
        x, y = res["x"], res["y"]
        interior |= bool(((x == np.rint(x)) & (x > 0) & (x < W - 1) & (y >= 0) & (y < H - 1)).any())
        last |= bool((x == W - 1).any())
        outside |= bool((x[:, -1] >= W - 1).all())
        lo, hi, _ = res["g_z"]
        assert (lo <= hi).all() and (lo < hi).any()           # the two-sided rule is in use here
    assert interior and last and outside


def _rejected(outputs, ref, mutant):
    """is the mutant's result, rounded to fp32, refused by the GPU test's comparison on any output?"""
    worst = 0.0
    for name in outputs:
        if name not in mutant or name not in ref:
            continue
        m, r = mutant[name], ref[name]
        val = m[0] if isinstance(m, tuple) else m.v
        worst = max(worst, R.judge(R.f32(val), r if isinstance(r, tuple) else R.exact(r))[0])
    return worst


@pytest.mark.parametrize("mut", R.STN_MUTANTS)
def test_stn_mutants_are_rejected(mut):
    hit = []
    for case in R.stn_cases():
        (name, Hc, Wc, H, W, Cc, Ho, Wo, _), inverse, fam = case
        if name.startswith("workload") or name.startswith("lds") or name.startswith("atomics"):
            continue                                         # the small shapes must do
        img, z, g, res = R.stn_reference(case)
        m = R.stn(img, z, Ho, Wo, inverse, g, mut=mut)
        w = _rejected(("out", "g_img", "g_z"), res, m)
        if w > 1.0:
            hit.append((R.stn_case_id(case), w))
    print(mut, "rejected on", len(hit), "cases; e.g.", hit[:3])
    assert hit, mut


# ---------------------------------------------------------------------------------------------------------------- renderer
def test_render_by_hand():
    """one object, one pixel, one channel: alpha .5, rgb .25, z_pres 1, z_depth 0 (s = 1): t = w = .5, N = .5, T = .25, U = .125"""
    r = R.render(np.array([0.25, 0.5]).reshape(1, 1, 1, 1, 2), np.array([0.75]).reshape(1, 1, 1, 1), np.zeros((1, 1)), zp=np.ones((1, 1)),
                 g=np.ones((1, 1, 1, 1)))
    D = 0.5 + 1e-8
    A = 0.25 / D
    assert abs(float(r["out"].v.item()) - (A * (0.125 / D) + (1 - A) * 0.75)) < 1e-16
    assert abs(float(r["g_bg"].v.item()) - (1 - A)) < 1e-16
    # d out / d rgb = A w / D
    assert abs(float(r["g_obj"].v.reshape(2)[0]) - A * 0.5 / D) < 1e-16
    # gates: values ON a gate pass a gradient, a step outside passes none
    for v, on in ((0.0, True), (1.0, True), (-0.0, True), (R._nx(0, -1), False), (R._nx(1, 2), False)):
        q = R.render(np.array([v, 0.5]).reshape(1, 1, 1, 1, 2), np.array([0.75]).reshape(1, 1, 1, 1), np.zeros((1, 1)), zp=np.ones((1, 1)), g=np.ones((1, 1, 1, 1)))
        assert (float(q["g_obj"].v.reshape(2)[0]) != 0) == on, v
    for a, on in ((R.A_MIN32, True), (1.0, True), (R._nx(1e-8, 0), False), (R._nx(1, 2), False)):
        q = R.render(np.array([0.25, a]).reshape(1, 1, 1, 1, 2), np.array([0.75]).reshape(1, 1, 1, 1), np.zeros((1, 1)), zp=np.ones((1, 1)), g=np.ones((1, 1, 1, 1)))
        assert (float(q["g_obj"].v.reshape(2)[1]) != 0) == on, a
    # test time: logit 0 -> sigmoid exactly .5 -> rounds half to even: absent, and no alternative; +-1e-7: within the sigmoid's error of .5: either
    zpv, _, _, fold = R.render_scalars(np.zeros((1, 3)), None, np.array([[0.0, 1e-7, 30.0]]), False)
    assert zpv.v.tolist() == [[R.A_MIN32, R.A_MIN32, 1.0]] and fold.tolist() == [[False, True, False]]
    assert R.render_scalars(np.zeros((1, 3)), None, np.array([[0.0, 1e-7, 30.0]]), False, fold_up=True)[0].v.tolist() == [[R.A_MIN32, 1.0, 1.0]]


@pytest.mark.parametrize("mode", R.RENDER_MODES)
@pytest.mark.parametrize("shape", R.RENDER_SHAPES, ids=lambda s: s[0])
def test_render_reference_agrees_with_the_oracle_and_its_autograd(shape, mode):
    """with the oracle's float64 alpha floor (amin = 1e-8; the kernel and TensorFlow hold 1e-8f) and, at test time, logits that do not fold"""
    d, refs = R.render_reference(shape, mode)
    name, B, Bp, H, W, Cc = shape
    training = mode != "test"
    assert not R.render_gate_folds(d["obj"], d["noise"]).any()
    zl = np.where(np.abs(d["zl"]) < 1e-3, 0.75, d["zl"])
    o = [T(d["obj"], True), T(d["bg"], True), T(d["zd"].reshape(B, Bp, 1, 1), True), T(d["zp"].reshape(B, Bp, 1, 1), True)]
    ref = O.renderer(o[0], o[1], o[2], o[3], T(zl.reshape(B, Bp, 1, 1)), training=training, noise=None if d["noise"] is None else T(d["noise"]),
                     num_channel=Cc)
    mine = R.render(d["obj"], d["bg"], d["zd"], zp=d["zp"], zl=zl, training=training, noise=d["noise"], g=d["g"] if training else None, amin=1e-8)
    assert rel(mine["out"].v, ref) <= AGREE
    if training:
        (ref * T(d["g"])).sum().backward()
        # the all-absent image's N is 1e-8-sized next to the 1e-8 of D: its z_depth gradient is a difference of near-equal float64 numbers
        for k, t, tol in (("g_obj", o[0].grad, AGREE), ("g_bg", o[1].grad, AGREE), ("g_zp", o[3].grad, AGREE), ("g_zd", o[2].grad, 1e-8)):
            assert rel(mine[k].v, t) <= tol, (k, rel(mine[k].v, t))
    if mode == "test" and Bp >= 4:
        assert len(refs) == 4 and refs[0]["fold"].sum(-1).max() == 2     # +1e-7 and -1e-7 in one image: up / down in every combination
        assert all(not np.array_equal(refs[0]["out"].v, r["out"].v) for r in refs[1:])


@pytest.mark.parametrize("mut", R.RENDER_MUTANTS)
def test_render_mutants_are_rejected(mut):
    hit = []
    for shape in R.RENDER_SHAPES[:3]:
        for mode in ("train", "train_noise"):
            d, refs = R.render_reference(shape, mode)
            m = R.render(d["obj"], d["bg"], d["zd"], zp=d["zp"], training=True, noise=d["noise"], g=d["g"], mut=mut)
            w = _rejected(("out", "g_obj", "g_bg", "g_zp", "g_zd"), refs[0], m)
            if w > 1.0:
                hit.append((shape[0], mode, w))
    print(mut, "rejected on", hit)
    assert hit, mut


# ---------------------------------------------------------------------------------------------------------------- z_pres KL
def test_zpres_by_hand():
    """one cell: dist = (1, cpp) / (1 + cpp), p(z) = cpp / (1 + cpp)"""
    pp, Tt, y, q = 0.25, 0.5, 0.3, -0.7
    r = R.zpres_kl(np.array([[0.9]]), np.array([[q]]), np.array([[y]]), pp, Tt, 1.0)
    pz = 0.75 / 1.75
    p = np.log(pz + 1e-8) - np.log(1 - pz + 1e-8)
    lt = np.log(Tt + 1e-8)
    post = lt - y * Tt + q - 2 * np.log(1 + np.exp(-y * Tt + q) + 1e-8)
    prior = lt - y * Tt + p - 2 * np.log(1 + np.exp(-y * Tt + p) + 1e-8)
    assert abs(float(r["kl"].v[0]) - (post - prior)) < 1e-15
    eq = np.exp(-y * Tt + q)
    assert abs(float(r["g_logits"].v[0, 0]) - (1 - 2 * eq / (1 + eq + 1e-8))) < 1e-15


@pytest.mark.parametrize("case", R.zpres_cases(), ids=str)
def test_zpres_reference_agrees_with_the_oracle_and_its_autograd(case):
    B, n, prior, temp = case
    zp, lg, pre = R.zpres_inputs(case)
    r = R.zpres_kl(zp, lg, pre, prior, temp, 1.0 / B)
    pp, tt, gs = float(np.float32(prior)), float(np.float32(temp)), float(np.float32(1.0 / B))
    rows = range(B) if B <= 3 else [0, 1, B - 1]             # the oracle returns a batch mean: per image, one image at a time
    for b in rows:
        rl, rp = T(lg[b].reshape(1, n, 1, 1), True), T(pre[b].reshape(1, n, 1, 1), True)
        k = O.compute_z_pres_kl_yolo_air(T(zp[b].reshape(1, n, 1, 1)), rl, rp, pp, tt)
        (k * gs).backward()
        assert abs(float(r["kl"].v[b]) - float(k.detach())) <= AGREE * abs(float(k.detach()))
        assert rel(r["g_pre"].v[b], rp.grad) <= AGREE and rel(r["g_logits"].v[b], rl.grad) <= AGREE
    assert np.isfinite(r["kl"].e).all() and np.isfinite(r["g_pre"].e).all() and np.isfinite(r["g_logits"].e).all()


@pytest.mark.parametrize("mut", R.ZPRES_MUTANTS)
def test_zpres_mutants_are_rejected(mut):
    hit = []
    for case in R.zpres_cases():
        if case[0] > 3:
            continue
        zp, lg, pre = R.zpres_inputs(case)
        ref = R.zpres_kl(zp, lg, pre, case[2], case[3], 1.0 / case[0])
        m = R.zpres_kl(zp, lg, pre, case[2], case[3], 1.0 / case[0], mut=mut)
        w = _rejected(("kl", "g_pre", "g_logits"), ref, m)
        if w > 1.0:
            hit.append((case, w))
    print(mut, "rejected on", hit[:4])
    assert hit, mut


# ---------------------------------------------------------------------------------------------------------------- loss sums
def test_loss_by_hand():
    r = R.loss(0, np.array([[1.0, 0.0]]), np.array([[0.5, 0.5]]))
    assert abs(float(r["sums"][0][0]) + 2 * np.log(0.5 + 1e-8)) < 1e-15 and r["ga"] is None
    assert abs(float(r["gb"].v[0, 0]) + 1 / (0.5 + 1e-8)) < 1e-15 and abs(float(r["gb"].v[0, 1]) - 1 / (0.5 + 1e-8)) < 1e-15
    # a prediction above 1: log(1 - p + 1e-8) is NaN -> -100, and that term passes no gradient
    r = R.loss(0, np.array([[0.25]]), np.array([[1.25]]))
    assert abs(float(r["sums"][0][0]) - (-(0.25 * np.log(1.25 + 1e-8) + 0.75 * -100.0))) < 1e-13
    assert abs(float(r["gb"].v[0, 0]) + 0.25 / (1.25 + 1e-8)) < 1e-15
    r = R.loss(1, np.array([[2.0]]), np.array([[0.0]]))
    assert abs(float(r["sums"][0][0]) + 0.5 * (1 + np.log(1e-8) - 4.0 - 1e-8)) < 1e-14 and float(r["gb"].v[0, 0]) == 0.0 and float(r["ga"].v[0, 0]) == 2.0
    r = R.loss(2, np.array([[1.0]]), np.array([[2.0]]), 3.0, 0.5)
    want = np.log(0.5 + 1e-8) - np.log(2 + 1e-8) + (4 + 4) / (2 * 0.25) - 0.5
    assert abs(float(r["sums"][0][0]) - want) < 1e-14 and abs(float(r["ga"].v[0, 0]) - 2 * (-2.0) / 0.5) < 1e-14
    assert float(r["sums"][2][0]) == (1 / 256.0 + 10) * R.U * (abs(np.log(0.5 + 1e-8)) + 1 + abs(np.log(2 + 1e-8)) + 1 + 16 + 0.5)


@pytest.mark.parametrize("case", R.loss_cases(), ids=str)
def test_loss_reference_agrees_with_the_oracle_and_its_autograd(case):
    mode, n, B = case
    a, b = R.loss_inputs(case)
    pm, ps = R.LOSS_PRIOR
    r = R.loss(R.LOSS_MODES[mode], a, b, pm, ps)
    pm, ps = float(np.float32(pm)), float(np.float32(ps))
    ar, br = T(a, True), T(b, True)
    if mode == "xent":
        t = M.xent_loss(ar, br)
    elif mode == "kl":
        t = -0.5 * (1 + O.tf_safe_log(br * br) - ar * ar - torch.exp(O.tf_safe_log(br * br)))
    else:
        t = O.tf_safe_log(torch.full_like(br, ps)) - O.tf_safe_log(br) + (br * br + (ar - pm) ** 2) / (2 * ps * ps) - 0.5
    t = t.reshape(B, -1).sum(1)
    t.sum().backward()
    assert rel(r["sums"][0], t) <= AGREE
    assert rel(r["gb"].v, br.grad) <= AGREE
    if mode != "xent":
        assert rel(r["ga"].v, ar.grad) <= AGREE


@pytest.mark.parametrize("mut", R.LOSS_MUTANTS)
def test_loss_mutants_are_rejected(mut):
    hit = []
    for case in R.loss_cases():
        a, b = R.loss_inputs(case)
        ref = R.loss(R.LOSS_MODES[case[0]], a, b, *R.LOSS_PRIOR)
        m = R.loss(R.LOSS_MODES[case[0]], a, b, *R.LOSS_PRIOR, mut=mut)
        ref = {k: v for k, v in ref.items() if v is not None and k != "t"}
        m = {k: v for k, v in m.items() if v is not None and k != "t"}
        w = _rejected(("sums", "ga", "gb"), ref, m)
        if w > 1.0:
            hit.append((case, w))
    print(mut, "rejected on", hit[:4])
    assert hit, mut


# ---------------------------------------------------------------------------------------------------------------- refusals (no launch)
@pytest.fixture(scope="module")
def lib(lib_built):
    from split_vae_amd import _lib
    return _lib.load()


SENT = -777.0


class Bufs:
    """host buffers handed over as if they were device memory: a refusal never dereferences them, and must leave the outputs as they were"""

    def __init__(self):
        self.keep = []

    def __call__(self, n=64):
        a = np.full(n, SENT, np.float32)
        self.keep.append(a)
        return a.ctypes.data_as(C.c_void_p)

    def untouched(self):
        return all((a == np.float32(SENT)).all() for a in self.keep)


def test_stn_refusals(lib):
    from split_vae_amd import _lib
    BAD = _lib.STATUS_BADARG
    b = Bufs()
    img, zw, out, bbox, g, gi, gz = (b() for _ in range(7))
    ok = dict(B=1, Hc=2, Wc=2, H=2, W=2, C=1, Ho=1, Wo=1)
    fwd = lambda img=img, zw=zw, out=out, **kw: lib.sv_stn_sample_fwd(img, zw, out, bbox, *[{**ok, **kw}[k] for k in ok], 0, None)
    bwd = lambda img=img, zw=zw, g=g, gz=gz, **kw: lib.sv_stn_sample_bwd(img, zw, g, gi, gz, *[{**ok, **kw}[k] for k in ok], 1, None)
    for kw in (dict(img=None), dict(zw=None), dict(out=None)):
        assert fwd(**kw) == BAD, kw
    for kw in (dict(img=None), dict(zw=None), dict(g=None), dict(gz=None)):
        assert bwd(**kw) == BAD, kw
    for kw in (dict(B=0), dict(Hc=1), dict(Wc=1), dict(H=1), dict(W=1), dict(C=0), dict(Ho=0), dict(Wo=0)):
        assert fwd(**kw) == BAD and bwd(**kw) == BAD, kw
    assert b.untouched()
    assert lib.sv_stn_bwd_overwrites(32, 64, 4, 1) == 1 and lib.sv_stn_bwd_overwrites(41, 50, 4, 1) == 0 and lib.sv_stn_bwd_overwrites(4, 4, 4, 0) == 0


def test_render_refusals(lib):
    from split_vae_amd import _lib
    BAD = _lib.STATUS_BADARG
    b = Bufs()
    obj, bg, zd, zp, zl, nz, out, g, gobj, gbg, gzp, gzd, ws = (b() for _ in range(13))
    ok = dict(B=1, Bp=2, H=2, W=2, C=1)
    dims = lambda kw: [{**ok, **kw}[k] for k in ok]

    def fwd(training=1, **kw):
        p = dict(obj=obj, bg=bg, zd=zd, zp=zp, zl=zl, nz=None, out=out)
        p.update({k: v for k, v in kw.items() if k in p})
        return lib.sv_spair_render_fwd(p["obj"], p["bg"], p["zd"], p["zp"], p["zl"], p["nz"], p["out"], *dims(kw), training, None)

    def bwd(ws_floats=None, **kw):
        p = dict(obj=obj, bg=bg, zd=zd, zp=zp, g=g, gobj=gobj, gbg=gbg, gzp=gzp, gzd=gzd, ws=ws)
        p.update({k: v for k, v in kw.items() if k in p})
        a = [p["obj"], p["bg"], p["zd"], p["zp"], None, p["g"], p["gobj"], p["gbg"], p["gzp"], p["gzd"]] + dims(kw)
        if ws_floats is None:
            return lib.sv_spair_render_bwd(*a, None)
        return lib.sv_spair_render_bwd_ws(*a, p["ws"], ws_floats, None)

    for kw in (dict(obj=None), dict(bg=None), dict(zd=None), dict(out=None), dict(B=0), dict(Bp=0), dict(Bp=17), dict(C=0), dict(C=5), dict(H=0), dict(W=0)):
        assert fwd(**kw) == BAD, kw
    assert fwd(training=1, zp=None) == BAD                   # training without z_pres
    assert fwd(training=0, zl=None) == BAD                   # test time without logits
    assert fwd(training=0, nz=nz) == BAD                     # test time with noise
    need = lib.sv_spair_render_bwd_workspace_floats(1, 2, 2)
    assert need == 2 * 16 and lib.sv_spair_render_bwd_workspace_floats(3, 13, 23) == 3 * 2 * 32 and lib.sv_spair_render_bwd_workspace_floats(0, 2, 2) == 0
    for wsf in (None, need):
        for kw in (dict(obj=None), dict(bg=None), dict(zd=None), dict(zp=None), dict(g=None), dict(gobj=None), dict(gbg=None), dict(gzp=None), dict(gzd=None),
                   dict(B=0), dict(Bp=17), dict(C=5), dict(C=0), dict(H=0)):
            assert bwd(ws_floats=wsf, **kw) == BAD, (wsf, kw)
    assert bwd(ws_floats=need - 1) == BAD                    # a workspace one float short
    assert bwd(ws_floats=need, ws=None) == BAD
    assert b.untouched()


def test_zpres_and_loss_refusals(lib):
    from split_vae_amd import _lib
    BAD = _lib.STATUS_BADARG
    b = Bufs()
    zp, lg, pre, kl, gp, gl = (b() for _ in range(6))

    def kl_call(B=1, n=4, **kw):
        p = dict(zp=zp, lg=lg, pre=pre, kl=kl)
        p.update(kw)
        return lib.sv_spair_zpres_kl(p["zp"], p["lg"], p["pre"], p["kl"], gp, gl, B, n, 0.1, 1.0, 1.0, None)

    for kw in (dict(zp=None), dict(lg=None), dict(pre=None), dict(kl=None), dict(B=0), dict(n=0), dict(n=17)):
        assert kl_call(**kw) == BAD, kw
    assert lib.sv_spair_zpres_kl_dyn(zp, lg, pre, kl, gp, gl, 1, 17, 0.1, None, 1.0, 1.0, None) == BAD
    a, bb, sums, ga, gb = (b() for _ in range(5))

    def loss_call(mode=0, B=1, n=4, sig=1.0, **kw):
        p = dict(a=a, b=bb, sums=sums)
        p.update(kw)
        return lib.sv_spair_loss(mode, p["a"], p["b"], p["sums"], ga, gb, B, n, 0.0, sig, None)

    for kw in (dict(a=None), dict(b=None), dict(sums=None), dict(B=0), dict(n=0), dict(mode=3), dict(mode=-1), dict(mode=2, sig=0.0), dict(mode=2, sig=-1.0)):
        assert loss_call(**kw) == BAD, kw
    assert lib.sv_spair_loss_dyn(3, a, bb, sums, ga, gb, 1, 4, 0.0, None, 1.0, None) == BAD
    assert b.untouched()
