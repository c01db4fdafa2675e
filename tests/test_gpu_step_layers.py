"""GPU: one training step of the plan (PHASE_ALL without Adam), checked LAYER BY LAYER from the buffers the step itself stored.

Every stored tensor is compared with the float64 reference of ITS OWN layer applied to the inputs the step stored (tests/conv_ref.py for the
convs, the formulas of tests/pointwise_ref.py for Sampling + KL, the discretised logistic and the loss scalars), weights being the fp32 masters
rounded as the prepared image rounds them, and judged per element by `gauss_bound` (contractions) or by the pointwise rule of
tests/test_gpu_pointwise.py (|gpu - ref| <= 1e-4 |ref| + 1e-5 scale + the derived sum terms).  Because every layer is judged from its actual
inputs and every backward gate is taken from the stored activation, a ReLU unit that the step gates the other way than an end-to-end oracle
does not travel: no element is exempt and there is no fraction-of-elements allowance.  This is where the plan's own launch paths run -- twin
launches, the NLL fused into the head's epilogue, K-slice slabs, the input-gradient forms picked by the batch size.

Where a value is not stored the references are composed and their bounds added:
  * the head pre-activations and dL/dz may stay as K-slice slabs (lat_ws_*) that their consumers sum: z_mean / z_sig are judged from a3 through
    the dense contraction and the pointwise formula, ghead_* from g1_* through d1's input gradient and the adjoint of Sampling + KL;
    test_latent_buffers_with_the_slab_sums_unfused checks pre_* and gz_* themselves in a fresh process with the latent-fuse switch off;
  * with the loss fused into the head the per-image NLL sums exist only inside the loss scalars: `losses` is judged from out6_* and kl_*.
An input gradient of an upsample -> conv layer is judged in two stages (hi-res gradient gu*, then adjoint + gate) where the step stored gu*, and
as one fused layer where it did not."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_ref as R  # noqa: E402
import pointwise_ref as PW  # noqa: E402
from oracle import np_ref  # noqa: E402
from test_gpu_step import flat_params, make_inputs, unflat  # noqa: E402

pytestmark = pytest.mark.gpu

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
CONFIGS = [(32, 1, 5), (64, 8, 3)]                   # H, patch, B: odd batches, both geometries of the twin launches
BETA = 40.0
# S of gauss_bound: folds on top of the contraction (tests/test_gpu_conv_api.py derives both)
S_COMPOSITE, S_SPLIT = 32, 64
RULE_RTOL, RULE_ATOL = 1e-4, 1e-5                    # the pointwise rule of tests/test_gpu_pointwise.py


class Report:
    def __init__(self, tag):
        self.tag, self.lines, self.bad = tag, [], []

    def judge(self, name, got, ref, bound):
        got, ref = got.detach().to(F64).cpu(), ref.to(F64)
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        err = (got - ref).abs()
        r = err / bound.clamp_min(1e-300)
        ratio = float(r.max()) if bool(torch.isfinite(got).all()) else float("inf")
        line = "step_layers %s %-28s worst error / bound = %.3f" % (self.tag, name, ratio)
        print(line)
        self.lines.append(line)
        if not ratio <= 1.0:
            self.bad.append("%s (%d of %d elements over the bound, first at flat index %d)" % (line, int((r > 1).sum()), r.numel(), int(r.flatten().argmax())))

    def bits(self, name, got, want):
        same = got.dtype == want.dtype and got.shape == want.shape and bool((got.cpu() == want.cpu()).all())
        line = "step_layers %s %-28s bit for bit: %s" % (self.tag, name, "yes" if same else "NO")
        print(line)
        self.lines.append(line)
        if not same:
            self.bad.append(line)


def rule(ref, scale=None, floor=0.0, bf16=False):
    b = RULE_RTOL * ref.abs() + RULE_ATOL * (ref.abs() if scale is None else scale) + floor
    return b + 2.0 ** -8 * ref.abs() if bf16 else b


def contraction(ref, ab, n, S, bf16):
    return R.gauss_bound(ab, n, S=S, ref=ref, bf16_out=bf16)


def run_config(ops, dtype, H, patch, B, direct_latent=False):
    """one step; -> Report.  direct_latent: pre_* and gz_* hold the summed values (latent-fuse switch off): compare them too."""
    from split_vae_amd._lib import PHASE_ALL, PHASE_ADAM
    bf = dtype == BF16
    rep = Report("%s H%d B%d" % ("bf16" if bf else "f32", H, B))
    L = 128
    x, perm, eps = make_inputs(B, H, patch, seed=3)
    images = ops.scramble_gather(torch.from_numpy(x).cuda(), torch.from_numpy(perm).cuda(), patch)
    params_np = np_ref.glorot_init(H, H, seed=3)
    rng = np.random.default_rng(9)
    for i in range(1, len(params_np), 2):              # non-zero biases
        params_np[i] = (rng.standard_normal(params_np[i].shape) * 0.05).astype(np.float32)
    plan = ops.LGVaePlan(B, H, H, beta=BETA, dtype=dtype)
    P = flat_params(plan, params_np)
    G = torch.zeros_like(P)
    plan.step(PHASE_ALL & ~PHASE_ADAM, params=P, grads=G, images6=images, eps_x=torch.from_numpy(eps[0]).cuda(), eps_x_hat=torch.from_numpy(eps[1]).cuda(), t=1)
    torch.cuda.synchronize()
    grads = {name: g.double() for (name, _, _), g in zip(plan.param_table, unflat(plan, G))}
    par = {name: torch.from_numpy(p) for (name, _, _), p in zip(plan.param_table, params_np)}
    img = images.cpu()
    buf = lambda name, dt, shape: plan.buffer(name, dt, shape).cpu()
    act = lambda name, shape: buf(name, dtype, shape).double()
    wr = lambda name: R.rnd(par[name], dtype)                     # a prepared image: the master converted once
    F = (H // 8) * (H // 8) * 128
    h8 = H // 8
    ks = PW.f32(BETA / B)
    eps_t = [torch.from_numpy(eps[0]).double(), torch.from_numpy(eps[1]).double()]

    def conv_layer(name, xin, wname, s, relu, ups, out_f32=False, S=0):
        w, b = wr(wname + "/kernel"), par[wname + "/bias"].double()
        ref = R.conv(xin, w, b, s, "relu" if relu else None, ups, dtype if ups else None)
        # an upsample -> conv layer may run in a polyphase form (fp32: d4 per class, the head merged; bf16: the head), whose border terms are added and taken
        # out again: sum|terms| as conv_ref.ab_fwd_composite gives it, which is no less than the direct form's
        ab = R.ab_fwd_composite(xin.abs(), w.abs()) + b.abs() if ups else R.conv(xin.abs(), w.abs(), b.abs(), s, None, False)
        return ref, contraction(ref, ab, w.shape[0] * w.shape[1] * w.shape[2], S + (S_COMPOSITE if ups else 0), bf and not out_f32)

    def wgrad_layer(tag, pname, xin, dy, k, s, ups):
        # (the bf16 head's polyphase weight gradient starts at 512 images per launch -- run_wgrad_layers: here every bf16 layer stages its hi-res pixels;
        #  fp32 d4 / d5 take the polyphase forms, whose frame terms are in ab_wgrad_composite)
        dw, db = R.wgrad(xin, dy, k, k, s, ups, dtype)
        aw, ab_ = R.wgrad(xin.abs(), dy.abs(), k, k, s, ups)
        if ups and not bf:
            aw = R.ab_wgrad_composite(xin.abs(), dy.abs(), k, k)
        n = dy.shape[0] * dy.shape[1] * dy.shape[2]
        rep.judge("dW " + pname, grads[pname + "/kernel"], dw, contraction(dw, aw, n, S_SPLIT + (S_COMPOSITE if ups else 0), False))
        rep.judge("db " + pname, grads[pname + "/bias"], db, contraction(db, ab_, n, S_SPLIT, False))

    def dense_wgrad(pname_k, pname_b, xin, dy):
        dw, aw = xin.T @ dy, xin.abs().T @ dy.abs()
        rep.judge("dW " + pname_k, grads[pname_k], dw, contraction(dw, aw, dy.shape[0], S_SPLIT, False))
        db, ab_ = dy.sum(0), dy.abs().sum(0)
        rep.judge("db " + pname_b, grads[pname_b], db, contraction(db, ab_, dy.shape[0], S_SPLIT, False))

    z_st, dz_parts = [], {}
    nll_ref, nll_bound, kl_st = [], [], []
    for k, (sfx, enc, dec) in enumerate((("x", "encoder_x", "decoder_x"), ("xh", "encoder_x_hat", "decoder_x_hat"))):
        # ------------------------------------------------------------------ encoder forward
        in8 = buf("in8_" + sfx, dtype, (B, H, H, 8))
        want = torch.zeros(B, H, H, 8, dtype=dtype)
        want[..., :3] = img[..., 3 * k:3 * k + 3].to(dtype)
        rep.bits("in8_" + sfx, in8, want)
        x0 = in8.double()[..., :3]
        a1 = act("a1_" + sfx, (B, H // 2, H // 2, 32))
        a2 = act("a2_" + sfx, (B, H // 4, H // 4, 64))
        a3 = act("a3_" + sfx, (B, h8, h8, 128))
        rep.judge("a1_" + sfx, a1, *conv_layer("a1", x0, enc + "/e1", 2, True, False))
        rep.judge("a2_" + sfx, a2, *conv_layer("a2", a1, enc + "/e2", 2, True, False))
        rep.judge("a3_" + sfx, a3, *conv_layer("a3", a2, enc + "/e3", 2, True, False))
        a3f = a3.reshape(B, F)
        Wh = torch.cat([wr(enc + "/e4_mean/kernel"), wr(enc + "/e4_sd/kernel")], 1)                     # [F, 2L]
        bh = torch.cat([par[enc + "/e4_mean/bias"], par[enc + "/e4_sd/bias"]]).double()
        pre_ref = a3f @ Wh
        b_pre = contraction(pre_ref, a3f.abs() @ Wh.abs(), F, S_SPLIT, False)
        if direct_latent:
            rep.judge("pre_" + sfx, buf("pre_" + sfx, F32, (B, 2 * L)), pre_ref, b_pre)
        r = PW.reparam_fwd_ref(pre_ref, bh, eps_t[k])
        zm, zs, z = (buf(n_ + sfx, F32, (B, L)).double() for n_ in ("z_mean_", "z_sig_", "z_"))
        # composed: the dense contraction's bound travels through mu = pre + b (slope 1) and sigma = softplus(a) (slope sigmoid(a) <= 1)
        rep.judge("z_mean_" + sfx, zm, r["z_mean"], b_pre[:, :L] + rule(r["z_mean"], r["mean_scale"]))
        rep.judge("z_sig_" + sfx, zs, r["z_sig"], b_pre[:, L:] * torch.sigmoid(r["a_sig"]) + rule(r["z_sig"]))
        rep.bits("eps_" + sfx, buf("eps_" + sfx, F32, (B, L)), torch.from_numpy(eps[k]))
        # z and kl from the stored mean and sigma (the kernel's own fp32 values)
        z_ref = zm + zs * eps_t[k]
        rep.judge("z_" + sfx, z, z_ref, rule(z_ref, torch.maximum(zm.abs(), (zs * eps_t[k]).abs())))
        t = PW.kl_addends(zm, zs)
        kl_ref = t.sum(dim=0).sum(dim=1)
        kl = buf("kl_" + sfx, F32, (B,)).double()
        rep.judge("kl_" + sfx, kl, kl_ref, rule(kl_ref, t.abs().amax(dim=(0, 2)), PW.kl_sum_term(L, t.abs().sum(dim=(0, 2)))))
        z_st.append(z)
        kl_st.append(kl)
        enc_state = dict(x0=x0, a1=a1, a2=a2, a3=a3, a3f=a3f, Wh=Wh, zm=zm, zs=zs)
        dz_parts[k] = enc_state
    zcat = buf("zcat", dtype, (B, 2 * L))
    rep.bits("zcat", zcat, torch.cat(z_st, 1).to(F32).to(dtype))
    zc = zcat.double()

    dec_state = []
    for k, (sfx, dec) in enumerate((("x", "decoder_x"), ("xh", "decoder_x_hat"))):
        # ------------------------------------------------------------------ decoder forward
        zin = zc if k == 0 else zc[:, L:]
        W1, b1 = wr(dec + "/d1/kernel"), par[dec + "/d1/bias"].double()
        h1 = act("h1_" + sfx, (B, F))
        ref = (zin @ W1 + b1).clamp_min(0.0)
        rep.judge("h1_" + sfx, h1, ref, contraction(ref, zin.abs() @ W1.abs() + b1.abs(), zin.shape[1], 0, bf))
        h1v = h1.reshape(B, h8, h8, 128)
        h2 = act("h2_" + sfx, (B, h8, h8, 128))
        h3 = act("h3_" + sfx, (B, H // 4, H // 4, 64))
        h4 = act("h4_" + sfx, (B, H // 2, H // 2, 32))
        out6 = buf("out6_" + sfx, F32, (B, H, H, 6)).double()
        rep.judge("h2_" + sfx, h2, *conv_layer("h2", h1v, dec + "/d2", 1, True, False))
        rep.judge("h3_" + sfx, h3, *conv_layer("h3", h2, dec + "/d3", 1, True, True))
        rep.judge("h4_" + sfx, h4, *conv_layer("h4", h3, dec + "/d4", 1, True, True))
        o_ref, o_bound = conv_layer("out6", h4, dec + "/d5", 1, False, True, out_f32=True)
        if bf:                                         # the polyphase head: composite weights combined in fp32, converted once (conv_ref.poly_head_fwd)
            o_ref = R.poly_head_fwd(h4, par[dec + "/d5/kernel"], par[dec + "/d5/bias"].double(), dtype)
        rep.judge("out6_" + sfx, out6, o_ref, o_bound)
        # ------------------------------------------------------------------ loss and its gradient, from the stored out6
        d = PW.dll_ref(img, 3 * k, out6, grad_scale=1.0 / B)
        HW = H * H
        nll_ref.append(d["nll"])
        nll_bound.append(rule(d["nll"], d["nll_max"], PW.dll_sum_term(HW, d["nll_sumabs"])))
        nll = buf("nll_" + sfx, F32, (B,)).double()
        if float(nll.abs().max()) > 0:                 # (the fused head leaves per-tile partial sums instead: judged through `losses` below)
            rep.judge("nll_" + sfx, nll, d["nll"], nll_bound[-1])
        g5 = act("g5_" + sfx, (B, H, H, 8))
        rep.judge("g5_" + sfx, g5[..., :6], d["g"], rule(d["g"], d["g_scale"], d["g_floor"], bf))
        rep.bits("g5_" + sfx + " pad channels", g5[..., 6:], torch.zeros(B, H, H, 2, dtype=F64))
        # ------------------------------------------------------------------ decoder backward
        def lowres(tag, gy, wname, lo, gu_name, g_name, Hh):
            w = wr(wname + "/kernel")
            cin, cout = w.shape[2], w.shape[3]
            gy = gy[..., :cout]
            gu = act(gu_name + sfx, (B, Hh, Hh, cin))
            g_lo = act(g_name + sfx, tuple(lo.shape))
            n1 = w.shape[0] * w.shape[1] * cout
            hi_ref, hi_ab = R.dgrad(gy, w, 1, Hh, Hh), R.dgrad(gy.abs(), w.abs(), 1, Hh, Hh)
            if float(gu.abs().max()) > 0:              # two launches: the hi-res gradient went through memory
                rep.judge(gu_name + sfx, gu, hi_ref, contraction(hi_ref, hi_ab, n1, 0, bf))
                ref = R.gate(R.resize2x_adjoint(gu), lo)
                rep.judge(g_name + sfx, g_lo, ref, contraction(ref, R.resize2x_adjoint(gu.abs()), 16, 0, bf))
            else:                                      # one fused launch: conv-transpose, resize adjoint and gate
                ref = R.gate(R.resize2x_adjoint(hi_ref), lo)
                rep.judge(g_name + sfx + " (fused)", g_lo, ref, contraction(ref, R.ab_lowres_composite(gy.abs(), w.abs(), Hh, Hh), n1 + 16, S_COMPOSITE, bf))
            return g_lo
        g4 = lowres("d5", g5, dec + "/d5", h4, "gu4_", "g4_", H)
        g3 = lowres("d4", g4, dec + "/d4", h3, "gu3_", "g3_", H // 2)
        g2 = lowres("d3", g3, dec + "/d3", h2, "gu2_", "g2_", H // 4)
        w2 = wr(dec + "/d2/kernel")
        g1 = act("g1_" + sfx, (B, F))
        ref = R.gate(R.dgrad(g2, w2, 1, h8, h8), h1v)
        rep.judge("g1_" + sfx, g1.reshape(B, h8, h8, 128), ref, contraction(ref, R.dgrad(g2.abs(), w2.abs(), 1, h8, h8), 16 * 128, 0, bf))
        dz_ref, dz_ab = g1 @ W1.T, g1.abs() @ W1.abs().T
        b_dz = contraction(dz_ref, dz_ab, F, S_SPLIT, False)
        if direct_latent:
            rep.judge("gz_" + sfx, buf("gz_" + sfx, F32, (B, zin.shape[1])), dz_ref, b_dz)
        dec_state.append(dict(dz=dz_ref, b_dz=b_dz))
        # ------------------------------------------------------------------ decoder weight gradients
        wgrad_layer("d5", dec + "/d5", h4, g5[..., :6], 6, 1, True)
        wgrad_layer("d4", dec + "/d4", h3, g4, 6, 1, True)
        wgrad_layer("d3", dec + "/d3", h2, g3, 4, 1, True)
        wgrad_layer("d2", dec + "/d2", h1v, g2, 4, 1, False)
        dense_wgrad(dec + "/d1/kernel", dec + "/d1/bias", zin, g1)

    # ---------------------------------------------------------------------- the loss scalars: from out6 (NLL) and the stored kl
    losses = buf("losses", F32, (8,)).double()[:6]
    l_ref, l_scale = PW.finalize_ref(nll_ref[0], nll_ref[1], kl_st[0], kl_st[1], BETA)
    nb = [b_.sum() / B for b_ in nll_bound]
    composed = torch.stack([nb[0], torch.zeros(()).double(), nb[1], torch.zeros(()).double(), torch.zeros(()).double(), nb[0] + nb[1]])
    rep.judge("losses", losses, l_ref, rule(l_ref, l_scale, PW.finalize_sum_term(B, (nll_ref[0], kl_st[0], nll_ref[1], kl_st[1]), BETA)) + composed)

    for k, (sfx, enc) in enumerate((("x", "encoder_x"), ("xh", "encoder_x_hat"))):
        # ------------------------------------------------------------------ adjoint of Sampling + KL, from the stored mean / sigma / eps and dL/dz composed
        # from g1 through d1's input gradient: z_x takes decoder_x's first L columns, z_x-hat its last L plus decoder_x-hat's
        st = dz_parts[k]
        if k == 0:
            dz, b_dz = dec_state[0]["dz"][:, :L], dec_state[0]["b_dz"][:, :L]
        else:
            dz, b_dz = dec_state[0]["dz"][:, L:] + dec_state[1]["dz"], dec_state[0]["b_dz"][:, L:] + dec_state[1]["b_dz"]
        zm, zs, e = st["zm"], st["zs"], eps_t[k]
        sgm = -torch.expm1(-zs)                          # softplus'(a) = sigmoid(a) = 1 - exp(-softplus(a))
        g_mu = dz + ks * zm
        g_a = (dz * e + ks * (zs - 1.0 / zs)) * sgm
        ref = torch.cat([g_mu, g_a], 1)
        s_m = torch.maximum(dz.abs(), ks * zm.abs())
        s_s = torch.maximum(torch.maximum(dz.abs() * e.abs(), ks * zs), ks / zs) * sgm
        bound = torch.cat([b_dz, b_dz * e.abs() * sgm], 1) + rule(ref, torch.cat([s_m, s_s], 1), bf16=bf)
        gh = act("ghead_" + sfx, (B, 2 * L))
        rep.judge("ghead_" + sfx, gh, ref, bound)
        # ------------------------------------------------------------------ encoder backward
        a1, a2, a3, Wh = st["a1"], st["a2"], st["a3"], st["Wh"]
        ga3 = act("ga3_" + sfx, (B, h8, h8, 128))
        ref = R.gate((gh @ Wh.T).reshape(B, h8, h8, 128), a3)
        rep.judge("ga3_" + sfx, ga3, ref, contraction(ref, (gh.abs() @ Wh.abs().T).reshape(B, h8, h8, 128), 2 * L, 0, bf))
        w3, w2e = wr(enc + "/e3/kernel"), wr(enc + "/e2/kernel")
        ga2 = act("ga2_" + sfx, (B, H // 4, H // 4, 64))
        ref = R.gate(R.dgrad(ga3, w3, 2, H // 4, H // 4), a2)
        rep.judge("ga2_" + sfx, ga2, ref, contraction(ref, R.dgrad(ga3.abs(), w3.abs(), 2, H // 4, H // 4), 4 * 128, 0, bf))
        ga1 = act("ga1_" + sfx, (B, H // 2, H // 2, 32))
        ref = R.gate(R.dgrad(ga2, w2e, 2, H // 2, H // 2), a1)
        rep.judge("ga1_" + sfx, ga1, ref, contraction(ref, R.dgrad(ga2.abs(), w2e.abs(), 2, H // 2, H // 2), 9 * 64, 0, bf))
        # ------------------------------------------------------------------ encoder weight gradients
        wgrad_layer("e1", enc + "/e1", st["x0"], ga1, 6, 2, False)
        wgrad_layer("e2", enc + "/e2", a1, ga2, 6, 2, False)
        wgrad_layer("e3", enc + "/e3", a2, ga3, 4, 2, False)
        dense_wgrad(enc + "/e4_mean/kernel", enc + "/e4_mean/bias", st["a3f"], gh[:, :L])
        dense_wgrad(enc + "/e4_sd/kernel", enc + "/e4_sd/bias", st["a3f"], gh[:, L:])
    n_grads = sum(1 for l_ in rep.lines if " dW " in l_ or " db " in l_)
    assert n_grads == 40, n_grads
    return rep


@pytest.fixture(scope="module")
def ops(lib_built):
    assert torch.cuda.is_available()
    from split_vae_amd import ops as o
    return o


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("H,patch,B", CONFIGS)
def test_step_layer_by_layer_from_its_stored_buffers(ops, H, patch, B, dtype):
    rep = run_config(ops, dtype, H, patch, B)
    assert not rep.bad, "\n".join(rep.bad)


def child_main():
    """fresh process, SV_NO_LATENT_FUSE=1: the slab sums run in their own kernels, so pre_* and gz_* hold the head pre-activations and dL/dz"""
    import split_vae_amd
    split_vae_amd.configure_hw_queues()
    from split_vae_amd import ops as o
    bad = []
    for dtype in (BF16, F32):
        for H, patch, B in CONFIGS:
            bad += run_config(o, dtype, H, patch, B, direct_latent=True).bad
    print("STEP_LAYERS_CHILD bad=%d" % len(bad))
    for b in bad:
        print("BAD " + b)
    sys.exit(1 if bad else 0)


def test_latent_buffers_with_the_slab_sums_unfused(lib_built):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "import sys; sys.path[:0] = [%r, %r]\nimport test_gpu_step_layers as T\nT.child_main()\n" % (root, os.path.join(root, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SV_NO_LATENT_FUSE="1"), capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert "STEP_LAYERS_CHILD" in r.stdout, r.stderr[-3000:]
    assert " pre_x " in r.stdout and " gz_xh " in r.stdout
    assert r.returncode == 0, "\n".join(l for l in r.stdout.splitlines() if l.startswith("BAD ")) + r.stderr[-2000:]
