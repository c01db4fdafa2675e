"""SPLIT-SPAIR, first blocker: the conv backbone of spair.Encoder (spair/spair.py:382-388) -- 48 -> 24 ->
12 -> 4x4 cells with strides 2, 2, 3 and three 1x1 convs, the only non-power-of-two extents and the only stride 3 of the repo --
on the MFMA im2col kernels (divide-based row decode), at the reference's shape [32, 48, 48, 3] (batch 32 is hard-coded,
spair/trainer.py:346), against the fp64 oracle restatement: forward chain, and per layer the input and weight gradients."""
import math
import os
import sys

import numpy as np
import pytest
import torch

from oracle import spair_ref, torch_ref

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spair_glue_ref as G  # noqa: E402

pytestmark = pytest.mark.gpu
B = 32


@pytest.fixture(scope="module")
def ops(lib_built):
    assert torch.cuda.is_available()
    from split_vae_amd import ops as o
    return o


def _pad8(t):
    c = t.shape[-1]
    return torch.nn.functional.pad(t, (0, (c + 7) // 8 * 8 - c))


@pytest.mark.parametrize("dtype,rtol", [(torch.float32, 1e-4), (torch.bfloat16, 3e-2)])
def test_backbone_forward_chain(ops, dtype, rtol):
    rng = np.random.default_rng(0)
    x = torch.from_numpy((rng.integers(0, 256, (B, 48, 48, 3)) / 255.0).astype(np.float32))       # spair/data.py: canvases in [0,1]
    params = spair_ref.backbone_init(3)
    for i in range(1, len(params), 2):
        params[i] = (rng.standard_normal(params[i].shape) * 0.05).astype(np.float32)             # exercise the bias path
    # fp64 reference from the operands as the device sees them (bf16 path: weights and every activation rounded to bf16)
    rnd = (lambda t: t.to(dtype).double())
    h_ref, refs = rnd(x), []
    h = _pad8(x).to(dtype).cuda()
    H = 48
    for i, (name, k, s, ci, co) in enumerate(spair_ref.BACKBONE):
        w, b = torch.from_numpy(params[2 * i]), torch.from_numpy(params[2 * i + 1])
        conv = ops.Conv2D(B, H, H, ci, co, k, s, act="relu", dtype=dtype)
        conv.prep(w.cuda())
        h = conv.fwd(h.contiguous(), b.cuda())
        h_ref = rnd(torch_ref.conv2d_same(h_ref, rnd(w), b.double(), s, "relu"))
        H = (H + s - 1) // s
        assert tuple(h.shape) == (B, H, H, (co + 7) // 8 * 8)
        got = h[..., :co].double().cpu()
        torch.testing.assert_close(got, h_ref, rtol=rtol, atol=rtol * float(h_ref.abs().max()), msg=lambda m: name + ": " + m)
        if co % 8:
            assert float(h[..., co:].abs().max()) == 0.0                                          # pad channels stay zero
        h_ref = got if dtype == torch.bfloat16 else h_ref                                         # bf16: continue from the device's rounding
    assert H == 4


@pytest.mark.parametrize("layer", [l for l in spair_ref.BACKBONE if l[0] != "z3"], ids=lambda l: l[0])
def test_backbone_layer_gradients(ops, layer):
    """Input gradient (stride 3: nine parity classes with 1, 2 or 4 taps) and weight gradient, bf16 operands, fp64 reference."""
    name, k, s, ci, co = layer
    H = {"conv1": 48, "conv2": 24, "conv3": 12}.get(name, 4)
    rng = np.random.default_rng(sum(map(ord, name)))
    x = torch.from_numpy(rng.standard_normal((B, H, H, ci)).astype(np.float32)).bfloat16()
    w = torch.from_numpy(rng.uniform(-1, 1, (k, k, ci, co)).astype(np.float32)) * math.sqrt(6.0 / (k * k * (ci + co)))
    OH = (H + s - 1) // s
    dy = torch.from_numpy(rng.standard_normal((B, OH, OH, co)).astype(np.float32)).bfloat16()
    conv = ops.Conv2D(B, H, H, ci, co, k, s, act="relu", dtype=torch.bfloat16)
    conv.prep(w.cuda())
    xr = x.double().requires_grad_(True)
    wr = w.bfloat16().double().requires_grad_(True)
    br = torch.zeros(co, dtype=torch.float64, requires_grad=True)
    torch_ref.conv2d_same(xr, wr, br, s, None).backward(dy.double())
    dw, db = conv.wgrad(_pad8(x).cuda(), dy.cuda())
    torch.testing.assert_close(dw.double().cpu(), wr.grad, rtol=3e-2, atol=3e-2 * float(wr.grad.abs().max()))
    torch.testing.assert_close(db.double().cpu(), br.grad, rtol=3e-2, atol=3e-2 * float(br.grad.abs().max()))
    if name == "conv1":
        return                                                 # the canvas needs no gradient
    dx = conv.dgrad(dy.cuda())
    assert float((dx[..., :ci].double().cpu() - xr.grad).norm() / xr.grad.norm()) < 5e-3
    torch.testing.assert_close(dx[..., :ci].double().cpu(), xr.grad, rtol=3e-2, atol=1.5e-2 * float(xr.grad.abs().max()))


def test_unsupported_geometries_are_refused(ops):
    from split_vae_amd import _lib
    with pytest.raises(_lib.SplitVaeError):
        ops.Conv2D(4, 50, 50, 8, 8, 4, 3)                       # stride must divide the extent
    with pytest.raises(_lib.SplitVaeError):
        ops.Conv2D(4, 48, 48, 8, 8, 4, 4)                       # strides 1..3


# ------------------------------------------------------------------ spatial transformer (spair/utils.py:119-330)
# The STN, renderer, z_pres KL and loss kernels are compared element by element through their entry points in tests/test_gpu_spair_glue.py; the tests
# below run the workload's own shapes through the `ops` wrappers and are judged by the same comparison (spair_glue_ref.judge: every element within the
# bound derived from the kernel's arithmetic).
STN_CASES = [  # name, the case of spair_glue_ref's table
    ("glimpses", "workload_glimpse"),    # STN(H_img=32...) on the [.,48,48,3] canvas: one 32x32 glimpse per cell
    ("render", "workload_render"),       # the renderer's inverse STN: each object's rgb+alpha pasted on a 48x48 canvas
]
# What these tests asserted before the per-element bounds existed stays asserted next to them: a worst-case bound summed over a glimpse's pixels (g_img: hundreds
# of atomic adds per image pixel) is wider in the norm than the device's error, which these hold.  out: largest absolute error and error norm / reference
# norm; g_img, g_z_where: error norm / reference norm.
STN_NORMWISE = {"glimpses": dict(atol=2e-5, out=1e-5, g_img=1e-5, g_z=1e-3), "render": dict(atol=2e-3, out=2e-4, g_img=1e-3, g_z=2e-2)}


def _rel_norm(got, ref):
    ref = torch.as_tensor(ref, dtype=torch.float64).reshape(got.shape)
    return float((got.double().cpu() - ref).norm() / ref.norm())


def _within(what, got, ref):
    ref = ref if isinstance(ref, tuple) else G.exact(ref)
    r, i = G.judge(got.detach().double().cpu().numpy(), ref)
    print("%-28s worst error / bound %.4g" % (what, r))
    assert r <= 1.0, (what, r, "flat index %d" % i)


def _stn_case(table_id):
    return next(c for c in G.stn_cases() if c[0][0] == table_id and c[2] == "normal")


@pytest.mark.parametrize("case", STN_CASES, ids=lambda c: c[0])
def test_stn_forward_matches_oracle(ops, case):
    """Affine grid + 4-tap gather + obj_bbox_mask against the float64 restatement, both STN directions, per element."""
    c = _stn_case(case[1])
    img, z, g, res = G.stn_reference(c)
    Ho, Wo = c[0][6], c[0][7]
    out, bbox = ops.stn_sample(_dev(img), _dev(z), Ho, Wo, inverse=c[1])
    assert tuple(out.shape) == tuple(res["out"][0].shape)
    _within(case[0] + " out", out, res["out"])
    _within(case[0] + " bbox", bbox, res["bbox"])
    ref, rbox = torch.from_numpy(res["out"][0]), torch.from_numpy(res["bbox"][0])       # the random family has no fold: one reference value per element
    torch.testing.assert_close(out.double().cpu(), ref, rtol=0, atol=STN_NORMWISE[case[0]]["atol"])
    assert _rel_norm(out, ref) < STN_NORMWISE[case[0]]["out"]
    torch.testing.assert_close(bbox.double().cpu(), rbox.reshape(bbox.shape), rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("case", STN_CASES, ids=lambda c: c[0])
def test_stn_backward_matches_autograd_of_the_oracle(ops, case):
    """g_img (scatter of the four tap weights) and g_z_where (through the tap weights; floor / clip carry none) against the analytic float64
    backward (itself held to torch autograd of the oracle in tests/test_spair_glue_host.py), per element."""
    c = _stn_case(case[1])
    img, z, g, res = G.stn_reference(c)
    g_img, g_z = ops.stn_sample_bwd(_dev(img), _dev(z), _dev(g), inverse=c[1])
    _within(case[0] + " g_img", g_img, res["g_img"])
    _within(case[0] + " g_z_where", g_z, res["g_z"])
    ei, ez = _rel_norm(g_img, res["g_img"][0]), _rel_norm(g_z, res["g_z"][0])
    print("%s: error norm / reference norm g_img %.3g g_z_where %.3g" % (case[0], ei, ez))
    assert ei < STN_NORMWISE[case[0]]["g_img"], ei
    assert ez < STN_NORMWISE[case[0]]["g_z"], ez
    # run-to-run: g_z_where is reduced in a fixed order; and the same without g_img
    assert torch.equal(g_z, ops.stn_sample_bwd(_dev(img), _dev(z), _dev(g), inverse=c[1])[1])
    none, g_z3 = ops.stn_sample_bwd(_dev(img), _dev(z), _dev(g), inverse=c[1], need_img=False)
    assert none is None and torch.equal(g_z, g_z3)


# ------------------------------------------------------------------ Renderer (spair/spair.py:534-579)
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32))).cuda()


RENDER_SHAPE = next(s for s in G.RENDER_SHAPES if s[0] == "workload")


@pytest.mark.parametrize("mode", ["train", "train_noise", "test"])
def test_renderer_forward_matches_oracle(ops, mode):
    d, refs = G.render_reference(RENDER_SHAPE, mode)
    training = mode != "test"
    B, Bp = d["zd"].shape
    z4 = lambda a: _dev(a).reshape(B, 4, 4, 1)
    out = ops.spair_render(_dev(d["obj"]), _dev(d["bg"]), z4(d["zd"]), z_pres=z4(d["zp"]) if training else None,
                           z_pres_logits=None if training else z4(d["zl"]), training=training, noise=None if d["noise"] is None else _dev(d["noise"]))
    got = out.double().cpu().numpy()
    for b in range(B):                                     # test time: a logit of +-1e-7 may round either way, per image (spair_glue_ref.render_scalars)
        rs = [G.judge(got[b], tuple(t[b] for t in G.exact(r["out"])))[0] for r in refs]
        print("renderer %s image %d: worst error / bound %s" % (mode, b, ["%.4g" % v for v in rs]))
        assert min(rs) <= 1.0, (b, rs)


@pytest.mark.parametrize("with_noise", [False, True])
def test_renderer_backward_matches_autograd_of_the_oracle(ops, with_noise):
    d, refs = G.render_reference(RENDER_SHAPE, "train_noise" if with_noise else "train")
    B, Bp = d["zd"].shape
    z4 = lambda a: _dev(a).reshape(B, 4, 4, 1)
    args = (_dev(d["obj"]), _dev(d["bg"]), z4(d["zd"]), z4(d["zp"]), _dev(d["g"]))
    nz = None if d["noise"] is None else _dev(d["noise"])
    got = ops.spair_render_bwd(*args, noise=nz)
    for name, a in zip(("g_obj", "g_bg", "g_zp", "g_zd"), got):
        _within(name, a, refs[0][name])
        err = _rel_norm(a, refs[0][name].v)                # the z gradients sum 2304 signed pixel terms: their worst-case bound is wider than this in the norm
        print("%-28s error norm / reference norm %.3g" % (name, err))
        assert err < 1e-4, (name, err)
    again = ops.spair_render_bwd(*args, noise=nz)
    assert all(torch.equal(a, b) for a, b in zip(got, again))      # fixed-order reductions: run-to-run identical


# ------------------------------------------------------------------ z_pres KL and clipnorm Adam
@pytest.mark.parametrize("prior_prob,temp", [(0.1, 1.0), (0.5, 2.5), (0.01, 0.5)])
def test_zpres_kl_and_its_gradient(ops, prior_prob, temp):
    """compute_z_pres_kl_yolo_air (spair/trainer.py:45-94) on the device: per-image sums and the gradients, per element, against the float64
    restatement (the count prior sees thresholded samples only: no gradient to z_pres)."""
    rng = np.random.default_rng(int(prior_prob * 1000))
    Bs = 32
    pre = torch.from_numpy(rng.standard_normal((Bs, 4, 4, 1)).astype(np.float32) * 2)
    logits = torch.from_numpy(rng.standard_normal((Bs, 4, 4, 1)).astype(np.float32) * 2)
    zp = torch.sigmoid(pre)
    zp[0] = 0.9; zp[1] = 0.1                               # all on / all off: the count recursion's extremes
    kl, g_pre, g_log = ops.spair_zpres_kl(zp.cuda(), logits.cuda(), pre.cuda(), prior_prob, temp)
    ref = G.zpres_kl(zp.double().numpy().reshape(Bs, 16), logits.double().numpy().reshape(Bs, 16), pre.double().numpy().reshape(Bs, 16),
                     prior_prob, temp, 1.0 / Bs)
    _within("kl per image", kl, ref["kl"])
    _within("g_pre", g_pre, ref["g_pre"])
    _within("g_logits", g_log, ref["g_logits"])
    # the batch mean and the gradients against the oracle and its autograd, as tightly as before the per-element bounds (whose worst case through
    # safe_log(pz) - safe_log(1 - pz) is wider than the device's error)
    rp, rl = pre.double().requires_grad_(True), logits.double().requires_grad_(True)
    want = spair_ref.compute_z_pres_kl_yolo_air(zp.double(), rl, rp, prior_prob, temp)
    want.backward()
    want = want.detach()
    assert abs(float(kl.double().mean()) - float(want)) <= 1e-5 * abs(float(want)) + 1e-5
    torch.testing.assert_close(g_pre.double().cpu(), rp.grad, rtol=1e-4, atol=1e-7)
    torch.testing.assert_close(g_log.double().cpu(), rl.grad, rtol=1e-4, atol=1e-7)


def test_adam_with_clipnorm_matches_keras_formula(ops):
    """Adam(clipnorm=1.0) (spair/main.py:109): per-TENSOR tf.clip_by_norm, then the Keras update; three steps, tensors whose
    norm is above and below the threshold, a ragged table."""
    rng = np.random.default_rng(9)
    sizes = [7, 4096, 33, 100000, 1]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(off[-1])
    p = rng.standard_normal(n).astype(np.float32)
    m = np.zeros(n, np.float32); v = np.zeros(n, np.float32)
    P, M, V = (torch.from_numpy(a.copy()).cuda() for a in (p, m, v))
    OFF = torch.from_numpy(off).cuda()
    lr, b1, b2, eps, clip = 1e-3, 0.9, 0.999, 1e-7, 1.0
    p64, m64, v64 = p.astype(np.float64), m.astype(np.float64), v.astype(np.float64)
    for t in range(1, 4):
        g = rng.standard_normal(n).astype(np.float32) * np.repeat([0.01, 1.0, 0.2, 0.001, 5.0], sizes).astype(np.float32)
        ops.adam_step_clipnorm(P, torch.from_numpy(g).cuda(), M, V, OFF, clip, t, lr, b1, b2, eps)
        g64 = g.astype(np.float64)
        for a, b in zip(off[:-1], off[1:]):
            nrm = np.sqrt((g64[a:b] ** 2).sum())
            g64[a:b] *= clip / max(nrm, clip)
        m64 += (g64 - m64) * (1 - b1); v64 += (g64 * g64 - v64) * (1 - b2)
        alpha = lr * np.sqrt(1 - b2 ** t) / (1 - b1 ** t)
        p64 -= alpha * m64 / (np.sqrt(v64) + eps)
    np.testing.assert_allclose(P.cpu().numpy(), p64, rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(M.cpu().numpy(), m64, rtol=2e-5, atol=1e-8)


# ------------------------------------------------------------------ ImageEncoder / ImageDecoder geometry (spair/spair.py:113-160)
@pytest.mark.parametrize("dtype,rtol", [(torch.float32, 1e-4), (torch.bfloat16, 3e-2)])
@pytest.mark.parametrize("H,Cin,Cout", [(48, 3, 32), (24, 32, 64), (12, 64, 128), (32, 3, 32), (16, 32, 64)])
def test_odd_kernel_stride_2_layers(ops, H, Cin, Cout, dtype, rtol):
    """Conv2D(kernel_size=3, strides=2, padding='same') of SPAIR's ImageEncoder (48 -> 24 -> 12 -> 6; TF pads 0 before / 1 after)
    and the same layer on power-of-two extents: forward, input gradient (parity classes with 4 / 2 / 2 / 1 taps) and weight
    gradient against the fp64 reference."""
    rng = np.random.default_rng(H + Cin)
    Bs, k, s = 8, 3, 2
    x = torch.from_numpy(rng.standard_normal((Bs, H, H, Cin)).astype(np.float32)).to(dtype)
    w = torch.from_numpy(rng.uniform(-1, 1, (k, k, Cin, Cout)).astype(np.float32)) * math.sqrt(6.0 / (k * k * (Cin + Cout)))
    b = torch.from_numpy(rng.standard_normal((Cout,)).astype(np.float32)) * 0.1
    conv = ops.Conv2D(Bs, H, H, Cin, Cout, k, s, act="relu", dtype=dtype)
    conv.prep(w.cuda())
    xg = _pad8(x).cuda()
    y = conv.fwd(xg, b.cuda())
    wr, xr, br = w.to(dtype).double().requires_grad_(True), x.double().requires_grad_(True), b.double().requires_grad_(True)
    yr = torch_ref.conv2d_same(xr, wr, br, s, "relu")
    assert tuple(y.shape[1:3]) == tuple(yr.shape[1:3]) == (H // 2, H // 2)
    torch.testing.assert_close(y[..., :Cout].double().cpu(), yr.detach(), rtol=rtol, atol=rtol * float(yr.abs().max()))
    dy = torch.from_numpy(rng.standard_normal(tuple(yr.shape)).astype(np.float32)).to(dtype)
    pre = torch_ref.conv2d_same(xr, wr, br, s, None)
    pre.backward(dy.double())
    dyg = _pad8(dy).cuda()
    dw, db = conv.wgrad(xg, dyg)
    torch.testing.assert_close(dw.double().cpu(), wr.grad, rtol=rtol, atol=rtol * float(wr.grad.abs().max()))
    torch.testing.assert_close(db.double().cpu(), br.grad, rtol=rtol, atol=rtol * float(br.grad.abs().max()))
    # Cin = 3: the glimpse encoder's first layer (spair/spair.py:250) -- its input gradient reaches z_where through the STN
    dx = conv.dgrad(dyg)
    torch.testing.assert_close(dx[..., :Cin].double().cpu(), xr.grad, rtol=rtol, atol=rtol * float(xr.grad.abs().max()))
    assert float(dx[..., Cin:].abs().max()) == 0.0 if Cin % 8 else True


@pytest.mark.parametrize("mode", ["xent", "kl", "kl_prior"])
def test_loss_reductions_and_their_gradients(ops, mode):
    """sv_spair_loss: xent_loss / kl_divergence / kl_divergence_two_gauss (spair/trainer.py:13-24, :103-109) as per-image sums with
    gradients, against autograd of the fp64 restatement -- including predictions at exactly 0 and 1 (tf_safe_log's 1e-8)."""
    from oracle import spair_model_ref as R
    g = torch.Generator().manual_seed(4)
    B, shape = 5, (6, 7, 3)
    if mode == "xent":
        a = torch.rand(B, *shape, generator=g)
        b = torch.rand(B, *shape, generator=g)
        b.view(-1)[:4] = torch.tensor([0.0, 1.0, 1e-9, 1 - 1e-7])
        f = lambda x, y: R.xent_loss(x, y)
    elif mode == "kl":
        a = torch.randn(B, *shape, generator=g)
        b = torch.nn.functional.softplus(torch.randn(B, *shape, generator=g))
        f = lambda x, y: -0.5 * (1 + spair_ref.tf_safe_log(y * y) - x * x - torch.exp(spair_ref.tf_safe_log(y * y)))
    else:
        a = torch.randn(B, *shape, generator=g)
        b = torch.nn.functional.softplus(torch.randn(B, *shape, generator=g) - 1.0)
        pm, ps = float(np.float32(3.7)), 0.5                  # as the call rounds it
        f = lambda x, y: (spair_ref.tf_safe_log(torch.full_like(y, ps)) - spair_ref.tf_safe_log(y) + (y * y + (x - pm) ** 2) / (2 * ps * ps) - 0.5)
    ar, br = a.double().requires_grad_(True), b.double().requires_grad_(True)
    t = f(ar, br).reshape(B, -1).sum(dim=1)
    w = torch.rand(B, generator=g).double()
    wv = w.view(B, 1, 1, 1)
    (t * w).sum().backward()
    sums, ga, gb = ops.spair_loss(mode, a.cuda(), b.cuda(), *((pm, ps) if mode == "kl_prior" else ()))
    n = a[0].numel()
    ref = G.loss(G.LOSS_MODES[mode], a.double().numpy().reshape(B, n), b.double().numpy().reshape(B, n), *((pm, ps) if mode == "kl_prior" else ()))
    # the restatement the bounds belong to is the oracle's formula
    assert float((torch.from_numpy(ref["sums"][0]) - t.detach()).abs().max()) <= 1e-12 * float(t.detach().abs().max())
    assert float((torch.from_numpy(ref["gb"].v).reshape(b.shape) * wv - br.grad).abs().max()) <= 1e-12 * float(br.grad.abs().max())
    _within(mode + " sums", sums, ref["sums"])             # (n / 256 + 10) u sum|t|
    _within(mode + " gb", gb, ref["gb"])
    torch.testing.assert_close(sums.double().cpu(), t.detach(), rtol=2e-5, atol=1e-4)
    torch.testing.assert_close(gb.double().cpu() * wv, br.grad, rtol=2e-5, atol=1e-5 * float(br.grad.abs().max()))
    if mode == "xent":
        assert ga is None
    else:
        _within(mode + " ga", ga, ref["ga"])
        torch.testing.assert_close(ga.double().cpu() * wv, ar.grad, rtol=2e-5, atol=1e-5 * float(ar.grad.abs().max()))


def test_clipnorm_adam_over_separate_gradient_tensors(ops):
    """sv_adam_step_clipnorm_ptrs (gradient tensors as the autograd engine returns them, addresses by value) == the flat-buffer call,
    including tensors whose flat offset is not a multiple of 4 (a 1-element bias shifts everything behind it)."""
    g = torch.Generator().manual_seed(8)
    shapes = [(37, 64), (64,), (64, 1), (1,), (3, 3, 8, 32), (32,), (4099,), (5,)]
    grads = [torch.randn(s, generator=g).cuda() * (3.0 if i % 2 else 0.01) for i, s in enumerate(shapes)]
    offs = np.concatenate([[0], np.cumsum([int(np.prod(s)) for s in shapes])])
    off = torch.tensor(offs, dtype=torch.int64).cuda()
    n = int(offs[-1])
    res = []
    for mode in ("flat", "ptrs"):
        p = torch.linspace(-1, 1, n).cuda()
        m, v = torch.full((n,), 0.01).cuda(), torch.full((n,), 0.02).cuda()
        if mode == "flat":
            ops.adam_step_clipnorm(p, torch.cat([x.reshape(-1) for x in grads]), m, v, off, 1.0, 3, 1e-3)
        else:
            ops.adam_step_clipnorm_tensors(p, grads, m, v, off, 1.0, 3, 1e-3)
        res.append((p, m, v))
    for a, b in zip(*res):
        torch.testing.assert_close(a, b, rtol=1e-6, atol=1e-7)       # (both forms split a tensor's norm the same way: tests/test_gpu_pointwise.py holds them bit for bit)
