"""GPU: the four SPAIR glue kernels (csrc/stn.hip, csrc/spair_render.hip: renderer and sequential z_pres KL, csrc/spair_loss.hip) through their entry
points (include/splitvae.h), element by element against the float64 restatements of tests/spair_glue_ref.py: every element of every output must lie in
[lo - e, hi + e], `e` being the bound that file derives from the kernel's arithmetic (no fitted constant; lo = hi except where the device's floor or
rounding may legitimately fall either way -- the crafted STN family and the test-time logits of +-1e-7).  Every output buffer (and the renderer's workspace)
starts as NaN, so an element no thread writes fails; the one exception is g_img where the STN accumulates with global atomics, which starts as zero as its
contract says.  Fixed-order reductions are also run twice and compared bit for bit.  The case tables (tests/spair_glue_ref.py) are the smallest shapes that
reach each mechanism; tests/test_spair_glue_host.py shows, mutant by mutant, what this comparison can see.  Each check prints its worst error / bound
(pytest -s); LAB_NOTES.md section 13 records them."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spair_glue_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
NAN = float("nan")
WORST = {}          # (kernel, output) -> worst error / bound seen so far, printed with every check: the last line per output is LAB_NOTES.md's figure


@pytest.fixture(scope="module")
def lib(lib_built):
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from split_vae_amd import _lib
    return _lib.load()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32))).cuda()


def nans(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device="cuda")


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ratio(kernel, name, got, ref):
    """worst error / bound of one output, printed and remembered"""
    ref = ref if isinstance(ref, tuple) else R.exact(ref)
    g = got.detach().double().cpu().numpy()
    r, i = R.judge(g, ref)
    WORST[(kernel, name)] = max(WORST.get((kernel, name), 0.0), r)
    idx = tuple(int(v) for v in np.unravel_index(i, ref[0].shape)) if ref[0].ndim else ()
    msg = "%-9s %-9s worst error / bound %.4g at %s: got %.9g, reference [%.9g, %.9g] +- %.3g   (running worst %.4g)" % (
        kernel, name, r, idx, g.reshape(-1)[i], ref[0].reshape(-1)[i], ref[1].reshape(-1)[i], ref[2].reshape(-1)[i], WORST[(kernel, name)])
    print(msg)
    return r, msg


def check(kernel, name, got, ref):
    r, msg = ratio(kernel, name, got, ref)
    assert r <= 1.0, msg


def same_bits(what, a, b):
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), what


# ---------------------------------------------------------------------------------------------------------------- STN
@pytest.mark.parametrize("case", R.stn_cases(), ids=R.stn_case_id)
def test_stn_forward_and_backward(lib, case):
    (name, Hc, Wc, H, W, Cc, Ho, Wo, _), inverse, fam = case
    img, z, g, res = R.stn_reference(case)
    B, Bp, inv = z.shape[0], Hc * Wc, 1 if inverse else 0
    d_img, d_z, d_g = dev(img), dev(z), dev(g)
    out, bbox = nans(B, Bp, Ho, Wo, Cc), nans(B, Bp, 4)
    assert lib.sv_stn_sample_fwd(P(d_img), P(d_z), P(out), P(bbox), B, Hc, Wc, H, W, Cc, Ho, Wo, inv, stream()) == 0
    check("stn", "out", out, res["out"])
    check("stn", "bbox", bbox, res["bbox"])
    # the path the case is meant for
    over = lib.sv_stn_bwd_overwrites(H, W, Cc, inv)
    assert over == (1 if inverse and H * W * Cc <= 8192 else 0)
    if name == "lds_8192":
        assert H * W * Cc == 8192 and over == 1
    if name == "atomics_8200":
        assert H * W * Cc == 8200 and over == 0

    def bwd(need_img):
        g_img = None if not need_img else (nans(*img.shape) if over else torch.zeros(img.shape, dtype=torch.float32, device="cuda"))
        g_z = nans(B, Hc, Wc, 4)
        assert lib.sv_stn_sample_bwd(P(d_img), P(d_z), P(d_g), P(g_img), P(g_z), B, Hc, Wc, H, W, Cc, Ho, Wo, inv, stream()) == 0
        return g_img, g_z

    g_img, g_z = bwd(True)
    check("stn", "g_img", g_img, res["g_img"])
    check("stn", "g_z", g_z, res["g_z"])
    same_bits("g_z_where is reduced in a fixed order: run to run", g_z, bwd(True)[1])
    same_bits("need_img = False: the same g_z_where", g_z, bwd(False)[1])


# ---------------------------------------------------------------------------------------------------------------- renderer
RENDER_CASES = [(s, m) for s in R.RENDER_SHAPES for m in R.RENDER_MODES]


@pytest.mark.parametrize("shape,mode", RENDER_CASES, ids=lambda v: v[0] if isinstance(v, tuple) else v)
def test_renderer_forward(lib, shape, mode):
    name, B, Bp, H, W, Cc = shape
    d, refs = R.render_reference(shape, mode)
    training = mode != "test"
    t = {k: (None if v is None else dev(v)) for k, v in d.items()}
    out = nans(B, H, W, Cc)
    assert lib.sv_spair_render_fwd(P(t["obj"]), P(t["bg"]), P(t["zd"]), P(t["zp"]) if training else None, None if training else P(t["zl"]),
                                   P(t["noise"]), P(out), B, Bp, H, W, Cc, 1 if training else 0, stream()) == 0
    if len(refs) == 1:
        check("render", "out", out, refs[0]["out"])
        return
    # a test-time logit within the sigmoid's error of zero may round to present or absent: each IMAGE must match one of the alternative renderings as a whole
    g = out.double().cpu().numpy()
    for b in range(B):
        rs = [R.judge(g[b], tuple(t[b] for t in R.exact(r["out"])))[0] for r in refs]
        print("render    out(test) image %d: worst error / bound per alternative %s" % (b, ["%.4g" % v for v in rs]))
        assert min(rs) <= 1.0, (b, rs)
        WORST[("render", "out(test)")] = max(WORST.get(("render", "out(test)"), 0.0), min(rs))


@pytest.mark.parametrize("form", ["one_workgroup", "workspace"])
@pytest.mark.parametrize("shape,mode", [c for c in RENDER_CASES if c[1] != "test"], ids=lambda v: v[0] if isinstance(v, tuple) else v)
def test_renderer_backward(lib, shape, mode, form):
    """sv_spair_render_bwd (one workgroup walks the image) and sv_spair_render_bwd_ws (a workgroup per 256-pixel chunk, partial sums through a workspace)"""
    name, B, Bp, H, W, Cc = shape
    d, refs = R.render_reference(shape, mode)
    ref = refs[0]
    t = {k: (None if v is None else dev(v)) for k, v in d.items()}
    need = lib.sv_spair_render_bwd_workspace_floats(B, H, W)
    assert need == B * ((H * W + 255) // 256) * 32

    def run():
        o = dict(g_obj=nans(B, Bp, H, W, Cc + 1), g_bg=nans(B, H, W, Cc), g_zp=nans(B, Bp), g_zd=nans(B, Bp))
        a = [P(t["obj"]), P(t["bg"]), P(t["zd"]), P(t["zp"]), P(t["noise"]), P(t["g"]), P(o["g_obj"]), P(o["g_bg"]), P(o["g_zp"]), P(o["g_zd"]), B, Bp, H, W, Cc]
        if form == "workspace":
            ws = nans(need)
            assert lib.sv_spair_render_bwd_ws(*a, P(ws), need, stream()) == 0
        else:
            assert lib.sv_spair_render_bwd(*a, stream()) == 0
        return o

    o = run()
    for k in ("g_obj", "g_bg", "g_zp", "g_zd"):
        check("render", k, o[k], ref[k])
    again = run()
    for k in o:
        same_bits(k + ": fixed-order reductions, run to run", o[k], again[k])


# ---------------------------------------------------------------------------------------------------------------- z_pres KL
@pytest.mark.parametrize("case", R.zpres_cases(), ids=str)
def test_zpres_kl(lib, case):
    B, n, prior, temp = case
    zp, lg, pre = R.zpres_inputs(case)
    ref = R.zpres_kl(zp, lg, pre, prior, temp, 1.0 / B)
    t_zp, t_lg, t_pre = dev(zp), dev(lg), dev(pre)

    def run(prior_dev=None, grads=True, gscale=1.0 / B):
        kl, gp, gl = nans(B), nans(B, n) if grads else None, nans(B, n) if grads else None
        assert lib.sv_spair_zpres_kl_dyn(P(t_zp), P(t_lg), P(t_pre), P(kl), P(gp), P(gl), B, n, 0.0 if prior_dev is not None else prior, P(prior_dev), temp,
                                         gscale, stream()) == 0
        return kl, gp, gl

    kl, gp, gl = run()
    check("zpres_kl", "kl", kl, ref["kl"])                   # per image
    check("zpres_kl", "g_pre", gp, ref["g_pre"])
    check("zpres_kl", "g_logits", gl, ref["g_logits"])
    kl2, gp2, gl2 = run(prior_dev=dev([prior]))
    same_bits("device-scalar prior: kl", kl, kl2), same_bits("device-scalar prior: g_pre", gp, gp2), same_bits("device-scalar prior: g_logits", gl, gl2)
    same_bits("no gradient buffers: the same kl", kl, run(grads=False)[0])
    if B <= 3:
        r37 = R.zpres_kl(zp, lg, pre, prior, temp, 0.37)
        _, gp3, gl3 = run(gscale=0.37)
        check("zpres_kl", "g_pre", gp3, r37["g_pre"])
        check("zpres_kl", "g_logits", gl3, r37["g_logits"])


# ---------------------------------------------------------------------------------------------------------------- loss sums
@pytest.mark.parametrize("case", R.loss_cases(), ids=str)
def test_loss_sums(lib, case):
    mode, n, B = case
    a, b = R.loss_inputs(case)
    pm, ps = R.LOSS_PRIOR
    m = R.LOSS_MODES[mode]
    ref = R.loss(m, a, b, pm, ps)
    ta, tb = dev(a), dev(b)

    def run(pm_dev=None, grads=True):
        sums = nans(B)
        ga = nans(B, n) if grads and m != 0 else None
        gb = nans(B, n) if grads else None
        assert lib.sv_spair_loss_dyn(m, P(ta), P(tb), P(sums), P(ga), P(gb), B, n, 0.0 if pm_dev is not None else pm, P(pm_dev), ps, stream()) == 0
        return sums, ga, gb

    sums, ga, gb = run()
    check("loss", mode + " sums", sums, ref["sums"])
    check("loss", mode + " gb", gb, ref["gb"])
    if m != 0:
        check("loss", mode + " ga", ga, ref["ga"])
    same_bits("no gradient buffers: the same sums", sums, run(grads=False)[0])
    same_bits("run to run", sums, run()[0])
    if m == 2:
        s2, ga2, gb2 = run(pm_dev=dev([pm]))
        same_bits("device-scalar prior mean: sums", sums, s2), same_bits("device-scalar prior mean: ga", ga, ga2), same_bits("gb", gb, gb2)
