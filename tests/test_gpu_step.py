"""GPU parity of the whole SPLIT-VAE step (LGVae.call + train_step_lg_vae + Keras-Adam) through
the C ABI plan, against the oracle restatement on identical inputs / eps / perm / weights."""
import os

import numpy as np
import pytest
import torch

from oracle import np_ref, torch_ref

pytestmark = pytest.mark.gpu

NAMES10 = ["x_mean", "x_log_scale", "z_x", "z_mean_x", "z_sig_x", "z_x_hat", "x_hat_mean", "x_hat_log_scale",
           "z_mean_x_hat", "z_sig_x_hat"]
LOSS_KEYS = ["x_recon_loss", "x_kl_loss", "x_hat_recon_loss", "x_hat_kl_loss", "total_kl_loss", "total_loss"]


def make_inputs(B, H, patch, seed=0):
    rng = np.random.Generator(np.random.PCG64(seed))
    x = (rng.integers(0, 256, size=(B, H, H, 3)) / 255.0 * 2 - 1).astype(np.float32)
    G2 = (H // patch) ** 2
    perm = np.stack([np.random.Generator(np.random.PCG64(seed + 1 + b)).permutation(G2) for b in range(B)]).astype(np.int32)
    eps = np.random.Generator(np.random.PCG64(seed + 2)).standard_normal((2, B, 128)).astype(np.float32)
    return x, perm, eps


def flat_params(plan, params_np):
    flat = torch.zeros(plan.n_params, dtype=torch.float32)
    for (name, off, shape), p in zip(plan.param_table, params_np):
        assert tuple(p.shape) == tuple(shape), (name, p.shape, shape)
        flat[off:off + p.size] = torch.from_numpy(np.ascontiguousarray(p)).flatten()
    return flat.cuda()


def unflat(plan, flat):
    f = flat.cpu()
    return [f[off:off + int(np.prod(shape))].reshape(shape) for (_, off, shape) in plan.param_table]


def outputs10(plan, B, H, L=128):
    o = {}
    out6x = plan.buffer("out6_x", torch.float32, (B, H, H, 6))
    out6h = plan.buffer("out6_xh", torch.float32, (B, H, H, 6))
    o["x_mean"], o["x_log_scale"] = out6x[..., :3], out6x[..., 3:]
    o["x_hat_mean"], o["x_hat_log_scale"] = out6h[..., :3], out6h[..., 3:]
    for k, b in [("z_x", "z_x"), ("z_mean_x", "z_mean_x"), ("z_sig_x", "z_sig_x"), ("z_x_hat", "z_xh"),
                 ("z_mean_x_hat", "z_mean_xh"), ("z_sig_x_hat", "z_sig_xh")]:
        o[k] = plan.buffer(b, torch.float32, (B, L))
    return o


@pytest.fixture(scope="module")
def ops(lib_built):
    assert torch.cuda.is_available()
    from split_vae_amd import ops as o
    return o


@pytest.mark.parametrize("H,patch,beta,B", [(32, 1, 40.0, 4), (64, 8, 120.0, 3)])
def test_step_fp32_matches_oracle(ops, deterministic, H, patch, beta, B):
    """THE fp32 parity test (primary, SURVEY 8c's pin): fp32 MFMA path with fixed-order reductions against the fp64 oracle -- forward
    10-tuple and the ELBO terms at rtol 1e-4 / atol 1e-5, all 40 gradients within 2e-3 of each tensor's max |g| with NO element-fraction
    allowance, weights after 1..3 Adam steps."""
    _fp32_step_vs_oracle(ops, H, patch, beta, B, strict=True)


@pytest.mark.parametrize("H,patch,beta,B", [(32, 1, 40.0, 4), (64, 8, 120.0, 3)])
def test_step_fp32_default_summation_order_matches_oracle(ops, H, patch, beta, B):
    """The same comparison on the DEFAULT path (split-K / m-split fp32 atomics: the summation order changes from run to run), looser:
    atol 1e-4 on the outputs, and a ReLU unit within that noise of zero may take the other gate than the fp64 oracle (a few elements,
    small in norm -- nothing else passes)."""
    _fp32_step_vs_oracle(ops, H, patch, beta, B, strict=bool(os.environ.get("SV_TEST_STRICT")))


def _fp32_step_vs_oracle(ops, H, patch, beta, B, strict):
    x, perm, eps = make_inputs(B, H, patch)
    images = ops.scramble_gather(torch.from_numpy(x).cuda(), torch.from_numpy(perm).cuda(), patch)
    assert np.array_equal(images.cpu().numpy(), np_ref.scramble_batch(x, perm, patch).astype(np.float32))
    params_np = np_ref.glorot_init(H, H, seed=3)
    rng = np.random.default_rng(9)
    for i in range(1, len(params_np), 2):          # non-zero biases so bias paths are exercised
        params_np[i] = (rng.standard_normal(params_np[i].shape) * 0.05).astype(np.float32)
    ref = torch_ref.RefTrainer(params_np, beta, dtype=torch.float64)
    plan = ops.LGVaePlan(B, H, H, beta=beta, dtype=torch.float32)
    P = flat_params(plan, params_np)
    G = torch.zeros_like(P); M = torch.zeros_like(P); V = torch.zeros_like(P)
    ex, eh = torch.from_numpy(eps[0]).cuda(), torch.from_numpy(eps[1]).cuda()
    imgs_cpu = images.cpu().double()
    L = ops._lib  # noqa
    from split_vae_amd._lib import PHASE_ALL, PHASE_ADAM
    for t in range(1, 4):
        fwd_ref, loss_ref, g_ref = ref.grads(imgs_cpu, eps[0], eps[1])
        plan.step(PHASE_ALL & ~PHASE_ADAM, params=P, grads=G, images6=images, eps_x=ex, eps_x_hat=eh, t=t)
        torch.cuda.synchronize()
        got = outputs10(plan, B, H)
        for name, r in zip(NAMES10, fwd_ref):
            torch.testing.assert_close(got[name].cpu().double(), r.detach(), rtol=1e-4, atol=1e-5 if strict else 1e-4, msg=lambda m: name + ": " + m)
        losses = plan.buffer("losses", torch.float32, (8,)).cpu().double()
        for i, k in enumerate(LOSS_KEYS):
            assert abs(float(losses[i]) - float(loss_ref[k])) <= 1e-4 * abs(float(loss_ref[k])) + (1e-5 if strict else 1e-3), k
        for (name, off, shape), gr, gg in zip(plan.param_table, g_ref, unflat(plan, G)):
            tol = 2e-3 * float(gr.abs().max()) + 1e-7
            dlt = (gg.double() - gr).abs()
            err = float(dlt.max())
            if err > tol:
                assert not strict, "grad %s: err %g tol %g (strict: fixed-order reductions, no allowance)" % (name, err, tol)
                # a ReLU unit within fp32 summation-order noise of zero takes the other gate than the fp64 oracle (analysis in
                # tests/test_gpu_gm.py::test_gm_step_fp32_matches_oracle): a few elements, small in norm -- nothing else passes here
                frac, rel = float((dlt > tol).double().mean()), float(dlt.norm() / gr.norm().clamp_min(1e-30))
                assert frac <= 2e-3 and rel <= 5e-3, "grad %s: err %g tol %g (%.2e of the elements, relative L2 %.2e)" % (name, err, tol, frac, rel)
        P_before = P.clone()
        plan.step(PHASE_ADAM, params=P, grads=G, adam_m=M, adam_v=V, t=t)
        ref_before = [p.detach().clone() for p in ref.params]
        ref.t += 1
        torch_ref.keras_adam_(ref.params, g_ref, ref.m, ref.v, ref.t, ref.lr)
        # Adam normalises every coordinate to ~lr*sign(g): coordinates whose gradient is ~0 amplify
        # fp32 noise, so compare the UPDATES statistically (and the loss curve exactly, above).
        lr = ref.lr
        for (name, off, shape), pr, pb, pg, pgb in zip(plan.param_table, ref.params, ref_before, unflat(plan, P),
                                                       unflat(plan, P_before)):
            d_ref = (pr.detach() - pb).flatten()
            d_got = (pg.double() - pgb.double()).flatten()
            err = (d_got - d_ref).abs()
            assert float(err.max()) <= 2.0 * lr + 1e-9, name
            assert float((err > 0.05 * lr).double().mean()) < 5e-3, "param update %s step %d" % (name, t)
        # continue the oracle from the GPU weights so the next step's losses test the step, not drift
        with torch.no_grad():
            for pr, pg in zip(ref.params, unflat(plan, P)):
                pr.copy_(pg.double())


@pytest.mark.parametrize("B,Lg,Ll", [(32, 128, 128), (96, 128, 128), (32, 64, 64), (64, 256, 256)])
def test_step_fp32_latent_block_kernels_match_oracle(ops, deterministic, B, Lg, Ll):
    """The fp32 latent block on latent_gemm.hip (round 5; vae/model.py:41-42, :111-112 heads, :152, :160 d1 and their gradients, tape.gradient
    vae/trainer.py:137): nt_gemm_kernel<float> / nt_gemm_ring_kernel<float> (K-slice slabs summed inside Sampling + KL) and the whole-batch
    weight-gradient tile tn_wgrad_f32_kernel need batches of whole 32-row phases, which the 3- / 4-image strict tests above never reach.
    SVHN-32 shapes, one gradient evaluation against the fp64 oracle at the strict bounds (outputs rtol 1e-4 / atol 1e-5, every gradient within
    2e-3 of its tensor's max |g|; beyond that only what the default-order twin above allows: a ReLU unit within fp32 noise of zero taking the other
    gate than the fp64 oracle -- at 96 images one such unit shows in e1's kernel gradient, on the im2col launches (SV_NO_LATENT_GEMM_F32=1) as well).
    (64, 64): the heads take the kernels, d1's input gradient of decoder_x-hat (N = 64 < one column tile) does not -- the mixed state of the plan's
    slab bookkeeping; (256, 256): wider tiles, other split-K slice counts.  (The plan takes equal power-of-two latent widths only: check_desc.)"""
    H, patch, beta = 32, 1, 40.0
    rng0 = np.random.Generator(np.random.PCG64(5))
    x = (rng0.integers(0, 256, size=(B, H, H, 3)) / 255.0 * 2 - 1).astype(np.float32)
    perm = np.stack([np.random.Generator(np.random.PCG64(6 + b)).permutation((H // patch) ** 2) for b in range(B)]).astype(np.int32)
    eps_x = np.random.Generator(np.random.PCG64(7)).standard_normal((B, Lg)).astype(np.float32)
    eps_h = np.random.Generator(np.random.PCG64(8)).standard_normal((B, Ll)).astype(np.float32)
    images = ops.scramble_gather(torch.from_numpy(x).cuda(), torch.from_numpy(perm).cuda(), patch)
    params_np = np_ref.glorot_init(H, H, seed=3, global_latent=Lg, local_latent=Ll)
    rng = np.random.default_rng(9)
    for i in range(1, len(params_np), 2):
        params_np[i] = (rng.standard_normal(params_np[i].shape) * 0.05).astype(np.float32)
    ref = torch_ref.RefTrainer(params_np, beta, dtype=torch.float64)
    plan = ops.LGVaePlan(B, H, H, global_latent=Lg, local_latent=Ll, beta=beta, dtype=torch.float32)
    P = flat_params(plan, params_np)
    G = torch.zeros_like(P)
    from split_vae_amd._lib import PHASE_ALL, PHASE_ADAM
    fwd_ref, loss_ref, g_ref = ref.grads(images.cpu().double(), eps_x, eps_h)
    for _ in range(2):                                  # twice: the second call starts from the first one's host-side slab state
        plan.step(PHASE_ALL & ~PHASE_ADAM, params=P, grads=G, images6=images, eps_x=torch.from_numpy(eps_x).cuda(), eps_x_hat=torch.from_numpy(eps_h).cuda(), t=1)
        torch.cuda.synchronize()
        got = {"z_x": plan.buffer("z_x", torch.float32, (B, Lg)), "z_mean_x": plan.buffer("z_mean_x", torch.float32, (B, Lg)),
               "z_sig_x": plan.buffer("z_sig_x", torch.float32, (B, Lg)), "z_x_hat": plan.buffer("z_xh", torch.float32, (B, Ll)),
               "z_mean_x_hat": plan.buffer("z_mean_xh", torch.float32, (B, Ll)), "z_sig_x_hat": plan.buffer("z_sig_xh", torch.float32, (B, Ll))}
        for name, r in zip(NAMES10, fwd_ref):
            if name in got:
                torch.testing.assert_close(got[name].cpu().double(), r.detach(), rtol=1e-4, atol=1e-5, msg=lambda m: name + ": " + m)
        losses = plan.buffer("losses", torch.float32, (8,)).cpu().double()
        for i, k in enumerate(LOSS_KEYS):
            assert abs(float(losses[i]) - float(loss_ref[k])) <= 1e-4 * abs(float(loss_ref[k])) + 1e-5, k
        for (name, off, shape), gr, gg in zip(plan.param_table, g_ref, unflat(plan, G)):
            tol = 2e-3 * float(gr.abs().max()) + 1e-7
            dlt = (gg.double() - gr).abs()
            err = float(dlt.max())
            if err > tol:
                # (96 images: decoder_x-hat's d4 output has two units whose fp64 pre-activations are 1.2e-7 and -2.4e-8 -- images 2 and 14 -- and the fp32 step takes the
                #  other gate at both; scripts/f32_latent_probe.py prints them, scripts/f32_gateflip_probe.py shows the gradients they reach: 13 of e1's 3456 kernel
                #  elements leave the 2e-3 band, relative L2 2.6e-3)
                frac, rel = float((dlt > tol).double().mean()), float(dlt.norm() / gr.norm().clamp_min(1e-30))
                assert frac <= 1e-2 and rel <= 5e-3, "grad %s: err %g tol %g (%.2e of the elements, relative L2 %.2e)" % (name, err, tol, frac, rel)


def test_step_bf16_close_to_oracle(ops):
    """bf16 MFMA path (config 2's compute type): operands rounded to 8 significant bits, fp32
    accumulate, fp32 ELBO/KL/Adam.  Stated tolerance vs the fp64 oracle at B=8:
      reconstructions / latents: relative Frobenius error < 2e-2;  ELBO scalars: 1e-3 relative;
      every gradient tensor: cosine > 0.995 and relative Frobenius error < 0.12.
    The gradient bound is dominated by ReLU-mask flips (a pre-activation within bf16 noise of 0
    flips its mask: ~0.3 % of elements, each a 100 % error -> sqrt(0.003) ~ 6 % on tensors that
    are not averaged over many positions, e.g. d1/kernel at B=8); it shrinks with batch size."""
    B, H, patch, beta = 8, 64, 8, 120.0
    x, perm, eps = make_inputs(B, H, patch, seed=5)
    images = ops.scramble_gather(torch.from_numpy(x).cuda(), torch.from_numpy(perm).cuda(), patch)
    params_np = np_ref.glorot_init(H, H, seed=3)
    ref = torch_ref.RefTrainer(params_np, beta, dtype=torch.float64)
    fwd_ref, loss_ref, g_ref = ref.grads(images.cpu().double(), eps[0], eps[1])
    plan = ops.LGVaePlan(B, H, H, beta=beta, dtype=torch.bfloat16)
    P = flat_params(plan, params_np)
    G = torch.zeros_like(P)
    from split_vae_amd._lib import PHASE_ALL, PHASE_ADAM
    plan.step(PHASE_ALL & ~PHASE_ADAM, params=P, grads=G, images6=images, eps_x=torch.from_numpy(eps[0]).cuda(),
              eps_x_hat=torch.from_numpy(eps[1]).cuda())
    torch.cuda.synchronize()
    got = outputs10(plan, B, H)
    for name, r in zip(NAMES10, fwd_ref):
        e = got[name].cpu().double() - r.detach()
        assert float(e.norm() / r.norm()) < 2e-2, name
    losses = plan.buffer("losses", torch.float32, (8,)).cpu().double()
    for i, k in enumerate(LOSS_KEYS):
        assert abs(float(losses[i]) - float(loss_ref[k])) <= 1e-3 * abs(float(loss_ref[k])), k
    for (name, off, shape), gr, gg in zip(plan.param_table, g_ref, unflat(plan, G)):
        gg = gg.double()
        rel = float((gg - gr).norm() / gr.norm())
        cos = float((gg * gr).sum() / (gg.norm() * gr.norm() + 1e-30))
        assert cos > 0.995 and rel < 0.12, "grad %s: cosine %g relfro %g" % (name, cos, rel)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("H,patch,B", [(32, 1, 5), (64, 8, 3)])
def test_loss_fused_into_the_head_equals_the_separate_kernel(ops, H, patch, B, dtype):
    """A training step evaluates the discretised-logistic loss in the decoder head's epilogue (tile_conv.hip: nll_part); the
    same phases issued as two calls (forward, then loss + backward) run dlogistic_kernel on out6 instead.  Same element
    function on the same fp32 outputs: the gradient records g5 are bitwise equal, the per-image NLL sums differ by fp32
    summation order only, and so do the weight gradients (split-K atomics in the encoder).  Both precisions: the fp32 step (the reference's precision,
    vae/trainer.py:21-38 behind vae/model.py:169) takes the fused form since round 6, its gradient record in floats."""
    from split_vae_amd._lib import PHASE_ALL, PHASE_ADAM, PHASE_PREP, PHASE_FORWARD
    x, perm, eps = make_inputs(B, H, patch, seed=11)
    images = ops.scramble_gather(torch.from_numpy(x).cuda(), torch.from_numpy(perm).cuda(), patch)
    plan = ops.LGVaePlan(B, H, H, beta=40.0, dtype=dtype)
    P = flat_params(plan, np_ref.glorot_init(H, H, seed=3))
    ex, eh = torch.from_numpy(eps[0]).cuda(), torch.from_numpy(eps[1]).cuda()
    res = []
    for split in (False, True):
        G = torch.zeros_like(P)
        rest = PHASE_ALL & ~PHASE_ADAM
        if split:
            plan.step(PHASE_PREP | PHASE_FORWARD, params=P, images6=images, eps_x=ex, eps_x_hat=eh)
            rest &= ~(PHASE_PREP | PHASE_FORWARD)
        plan.step(rest, params=P, grads=G, images6=images, eps_x=ex, eps_x_hat=eh)
        torch.cuda.synchronize()
        res.append({"g5x": plan.buffer("g5_x", dtype, (B, H, H, 8)).clone(),
                    "g5h": plan.buffer("g5_xh", dtype, (B, H, H, 8)).clone(),
                    "o6x": plan.buffer("out6_x", torch.float32, (B, H, H, 6)).clone(),
                    "nll": plan.buffer("nll_x", torch.float32, (B,)).clone(),
                    "losses": plan.buffer("losses", torch.float32, (8,)).clone(), "G": G})
    a, b = res
    assert torch.equal(a["o6x"], b["o6x"])
    assert torch.equal(a["g5x"], b["g5x"]) and torch.equal(a["g5h"], b["g5h"])
    assert float(a["g5x"].float().abs().max()) > 0
    torch.testing.assert_close(a["nll"], b["nll"], rtol=1e-5, atol=0)
    torch.testing.assert_close(a["losses"][:6], b["losses"][:6], rtol=1e-5, atol=0)
    torch.testing.assert_close(a["G"], b["G"], rtol=1e-3, atol=1e-5 * float(b["G"].abs().max()))


def test_step_forward_reproducible(ops):
    """Same inputs/seed twice: the decoder outputs are bitwise equal and the scalars agree to
    fp32 round-off (the encoder head's split-K uses fp32 atomics, so the KL terms may differ in
    the last bits; everything downstream of the bf16 latents is atomic-free)."""
    B, H = 4, 32
    x, perm, eps = make_inputs(B, H, 1, seed=7)
    images = ops.scramble_gather(torch.from_numpy(x).cuda(), torch.from_numpy(perm).cuda(), 1)
    plan = ops.LGVaePlan(B, H, H, beta=40.0, dtype=torch.bfloat16)
    P = flat_params(plan, np_ref.glorot_init(H, H, seed=3))
    from split_vae_amd._lib import PHASE_PREP, PHASE_FORWARD, PHASE_LOSS
    outs = []
    for _ in range(2):
        plan.step(PHASE_PREP | PHASE_FORWARD | PHASE_LOSS, params=P, images6=images, seed=1, step=2)
        torch.cuda.synchronize()
        outs.append((plan.buffer("eps_x", torch.float32, (B, 128)).clone(),
                     plan.buffer("losses", torch.float32, (8,)).clone()))
    assert torch.equal(outs[0][0], outs[1][0])
    torch.testing.assert_close(outs[0][1][:6], outs[1][1][:6], rtol=1e-6, atol=0)


@pytest.mark.parametrize("H,L", [(128, 128), (32, 64)])
def test_other_geometries_match_oracle_losses(ops, H, L):
    """celeba128 (vae/data.py:18) and a non-default latent width: the bf16 step's loss terms against the fp64
    oracle, and a finite, non-zero gradient for every variable."""
    B, patch, beta = 2, 8, 120.0
    x, perm, _ = make_inputs(B, H, patch, seed=4)
    eps = np.random.Generator(np.random.PCG64(8)).standard_normal((2, B, L)).astype(np.float32)
    images = torch.from_numpy(np_ref.scramble_batch(x, perm, patch).astype(np.float32))
    params_np = np_ref.glorot_init(H, H, seed=3, global_latent=L, local_latent=L)
    ref = torch_ref.RefTrainer(params_np, beta, dtype=torch.float64)
    _, loss_ref = ref.forward_losses(images.double(), eps[0], eps[1])
    plan = ops.LGVaePlan(B, H, H, global_latent=L, local_latent=L, beta=beta, dtype=torch.bfloat16)
    P = flat_params(plan, params_np)
    G = torch.zeros_like(P)
    from split_vae_amd._lib import PHASE_ALL, PHASE_ADAM
    plan.step(PHASE_ALL & ~PHASE_ADAM, params=P, grads=G, images6=images.cuda(), eps_x=torch.from_numpy(eps[0]).cuda(),
              eps_x_hat=torch.from_numpy(eps[1]).cuda(), t=1)
    torch.cuda.synchronize()
    losses = plan.buffer("losses", torch.float32, (8,)).cpu()
    for i, k in enumerate(LOSS_KEYS):
        want = float(loss_ref[k])
        assert abs(float(losses[i]) - want) <= 5e-3 * abs(want) + 5e-2, (k, float(losses[i]), want)
    for name, off, shape in plan.param_table:
        g = G[off:off + int(np.prod(shape))]
        assert torch.isfinite(g).all() and float(g.abs().max()) > 0, name


@pytest.mark.gpu
def test_step_without_stored_reconstructions_is_the_same_step(lib_built):
    """SV_PHASE_NO_RECON: the training step with the loss fused into the head conv does not write out6_x / out6_xh; the five
    losses, gradients and updated variables are equal up to the step's own run-to-run atomics order."""
    import torch
    from split_vae_amd import data, trainer
    from split_vae_amd.augmentation import Augmentator
    from split_vae_amd.model import LGVae
    from split_vae_amd.optimizer import Adam
    B, H = 64, 64
    x = data.synthetic_images(B, H, H, seed=0, device="cuda")
    img = Augmentator("scramble", size=8, seed=1).augment(x)
    outs = []
    for keep in (True, False):
        m = LGVae(128, 128, image_shape=[-1, H, H, 3], dtype="bf16", device=torch.device("cuda"), seed=3)
        m.beta = 120.0
        opt = Adam(learning_rate=1e-4)
        plan = trainer.train_step(m, img, opt, keep_recon=keep)
        torch.cuda.synchronize()
        o6 = plan.buffer("out6_x", torch.float32, (B, H, H, 6)).clone()
        outs.append((trainer.last_losses(plan), m.grad_flat.clone(), m.flat.clone(), o6))
    (l0, g0, p0, o0), (l1, g1, p1, o1) = outs
    for k in l0:
        assert abs(l0[k] - l1[k]) <= 1e-5 * max(1.0, abs(l0[k])), k
    # (the split-K atomics of the heads / d1 reorder fp32 sums from run to run: equal up to that, not bitwise)
    assert float((g0 - g1).norm() / g0.norm()) < 1e-4 and float((p0 - p1).norm() / p0.norm()) < 1e-3   # (first Adam step = lr * sign-like: near-zero gradients flip)
    assert float(o0.abs().max()) > 0 and float(o1.abs().max()) == 0.0      # stored / never written (the workspace starts zeroed)


@pytest.mark.gpu
def test_stale_staged_inputs_are_not_trusted(lib_built):
    """The staged inputs live in the plan's shared in8_x / in8_xh: a test_step / second staged batch on the same plan, or an in-place
    edit of the batch, between augment(plan=) and train_step must make train_step fall back to its own split / pad pass."""
    import torch
    from split_vae_amd import data, trainer
    from split_vae_amd.augmentation import Augmentator
    from split_vae_amd.model import LGVae
    from split_vae_amd.optimizer import Adam
    B, H = 16, 32
    x = data.synthetic_images(B, H, H, seed=0, device="cuda")
    other = data.synthetic_images(B, H, H, seed=9, device="cuda")

    def run(disturb):
        m = LGVae(128, 128, image_shape=[-1, H, H, 3], dtype="bf16", device=torch.device("cuda"), seed=3)
        plan = m.plan(B)
        img = Augmentator("scramble", size=4, seed=1).augment(x, plan=plan if disturb else None)
        want = img.clone()
        if disturb == "test_step":
            trainer.test_step(m, Augmentator("scramble", size=4, seed=2).augment(other))     # overwrites in8_* with another batch
        elif disturb == "second_staging":
            Augmentator("scramble", size=4, seed=2).augment(other, plan=plan)                # a prefetched batch
        elif disturb == "in_place":
            img.mul_(0.5)
            want = img.clone()
        m._calls = 7                                                                         # same Philox step for every variant
        trainer.train_step(m, img, Adam(learning_rate=1e-4))
        torch.cuda.synchronize()
        return want, trainer.last_losses(plan)

    for disturb in ("test_step", "second_staging", "in_place"):
        img_d, got = run(disturb)
        m = LGVae(128, 128, image_shape=[-1, H, H, 3], dtype="bf16", device=torch.device("cuda"), seed=3)
        m._calls = 7
        trainer.train_step(m, img_d, Adam(learning_rate=1e-4))
        torch.cuda.synchronize()
        ref = trainer.last_losses(m.plan(B))
        for k in ref:
            assert abs(ref[k] - got[k]) <= 1e-5 * max(1.0, abs(ref[k])), (disturb, k, ref[k], got[k])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_staged_augmentation_fills_the_step_inputs(lib_built, dtype):
    """Augmentator.scramble(x, plan=plan): the scramble kernel also writes the plan's padded input tensors (in8_x / in8_xh) and
    train_step skips its split / pad pass (SV_PHASE_INPUTS_STAGED).  images6 bit-equal to the plain augmentation, the staged
    buffers bit-equal to what split_pad derives from it, the step's losses equal."""
    import torch
    from split_vae_amd import data, trainer
    from split_vae_amd.augmentation import Augmentator
    from split_vae_amd.model import LGVae
    from split_vae_amd.optimizer import Adam
    B, H = 16, 32
    x = data.synthetic_images(B, H, H, seed=0, device="cuda")
    res = []
    for staged in (False, True):
        m = LGVae(128, 128, image_shape=[-1, H, H, 3], dtype=dtype, device=torch.device("cuda"), seed=3)
        plan = m.plan(B)
        aug = Augmentator("scramble", size=4, seed=1)
        img = aug.augment(x, plan=plan if staged else None)
        assert (getattr(img, "_sv_staged_plan", None) is plan) == staged
        if staged:                                       # poison check: the step must not rewrite the buffers from images6
            in8 = plan.buffer("in8_xh", plan.dtype, (B, H, H, 8)).clone()
        trainer.train_step(m, img, Adam(learning_rate=1e-4))
        torch.cuda.synchronize()
        assert getattr(img, "_sv_staged_plan", None) is None
        res.append((img.clone(), plan.buffer("in8_x", plan.dtype, (B, H, H, 8)).clone(), plan.buffer("in8_xh", plan.dtype, (B, H, H, 8)).clone(),
                    trainer.last_losses(plan)))
        if staged:
            assert torch.equal(in8, res[-1][2])
    (i0, a0, b0, l0), (i1, a1, b1, l1) = res
    assert torch.equal(i0, i1) and torch.equal(a0, a1) and torch.equal(b0, b1)
    for k in l0:
        assert abs(l0[k] - l1[k]) <= 1e-5 * max(1.0, abs(l0[k])), k


def test_encoder_backward_without_the_decoders_sees_zero_dz(lib_built):
    """PHASE_BWD_ENC_HEADS | PHASE_BWD_ENC_CONVS right after a forward (no decoder backward: the KL terms' gradient only, vae/trainer.py:12-13)
    must not pick up the previous step's dz -- the slab path no longer zeroes those buffers every forward.  The head-bias
    gradient of encoder_x_hat is then d(beta * KL) / d(pre) summed over the batch, which has a closed form in z_mean / z_sig."""
    import torch
    from split_vae_amd import data, trainer
    from split_vae_amd._lib import PHASE_PREP, PHASE_FORWARD, PHASE_LOSS, PHASE_BWD_ENC_HEADS, PHASE_BWD_ENC_CONVS
    from split_vae_amd.augmentation import Augmentator
    from split_vae_amd.model import LGVae
    from split_vae_amd.optimizer import Adam
    B, H = 256, 64
    x = data.synthetic_images(B, H, H, seed=0, device="cuda")
    img = Augmentator("scramble", size=8, seed=1).augment(x)
    m = LGVae(128, 128, image_shape=[-1, H, H, 3], dtype="bf16", device=torch.device("cuda"), seed=3)
    m.beta = 120.0
    opt = Adam(learning_rate=1e-4)
    for _ in range(2):                                          # whole steps first: the slab path is active, dz slabs hold a real gradient
        plan = trainer.train_step(m, img, opt)
    plan.step(PHASE_PREP | PHASE_FORWARD | PHASE_LOSS, params=m.flat, grads=m.grad_flat, images6=img, seed=m.seed, step=7)
    plan.step(PHASE_BWD_ENC_HEADS | PHASE_BWD_ENC_CONVS, params=m.flat, grads=m.grad_flat, images6=img, seed=m.seed, step=7)
    torch.cuda.synchronize()
    zm = plan.buffer("z_mean_xh", torch.float32, (B, 128)).double()
    zs = plan.buffer("z_sig_xh", torch.float32, (B, 128)).double()
    ks = m.beta / B
    want_mean = (ks * zm).sum(0)                                # d KL / d mu = mu
    want_sd = (ks * (zs - 1.0 / zs) * (1.0 - torch.exp(-zs))).sum(0)     # d KL / d sigma * softplus'
    names = [n for n, _, _ in m.param_table]
    g = {n: t for n, t in zip(names, m.gradients)}
    gm, gs = g["encoder_x_hat/e4_mean/bias"].double(), g["encoder_x_hat/e4_sd/bias"].double()
    assert float((gm - want_mean).abs().max()) <= 2e-2 * float(want_mean.abs().max()) + 1e-6
    assert float((gs - want_sd).abs().max()) <= 2e-2 * float(want_sd.abs().max()) + 1e-6


@pytest.mark.gpu
def test_encoder_head_adjoint_at_small_sigma(lib_built):
    """reparam_kl_bwd_twin_kernel is reached only through the plan.  The phase sequence of the test above on an fp32 model, with encoder_x_hat's sigma-head bias
    at -8, -10, -12 and -14 on four 8-wide bands of latent dimensions (sigma 3e-4 .. 8e-7; the other 96 dimensions stay at the initial 0).  With dz = 0 the bias
    gradient is sum_b ks (sigma - 1 / sigma) softplus', softplus' = -expm1(-sigma), computed here in float64 from the plan's z_sig_xh.  Every band is held to
    1e-4 of ITS OWN maximum: taken as 1 - exp(-sigma), softplus' is 2 % off on the -12 band, which the maximum of the unpinned dimensions would hide."""
    import torch
    from split_vae_amd import data, trainer
    from split_vae_amd._lib import PHASE_PREP, PHASE_FORWARD, PHASE_LOSS, PHASE_BWD_ENC_HEADS, PHASE_BWD_ENC_CONVS
    from split_vae_amd.augmentation import Augmentator
    from split_vae_amd.model import LGVae
    from split_vae_amd.optimizer import Adam
    B, H, L = 8, 32, 128
    x = data.synthetic_images(B, H, H, seed=0, device="cuda")
    img = Augmentator("scramble", size=8, seed=1).augment(x)
    m = LGVae(L, L, image_shape=[-1, H, H, 3], dtype="f32", device=torch.device("cuda"), seed=3)
    m.beta = 120.0
    bands = {-8.0: slice(0, 8), -10.0: slice(8, 16), -12.0: slice(16, 24), -14.0: slice(24, 32), 0.0: slice(32, L)}
    off = {n: o for n, o, _ in m.param_table}["encoder_x_hat/e4_sd/bias"]
    for v, sl in bands.items():
        m.flat[off + sl.start:off + sl.stop] = v
    opt = Adam(learning_rate=1e-4)
    for _ in range(2):
        plan = trainer.train_step(m, img, opt)
    plan.step(PHASE_PREP | PHASE_FORWARD | PHASE_LOSS, params=m.flat, grads=m.grad_flat, images6=img, seed=m.seed, step=7)
    plan.step(PHASE_BWD_ENC_HEADS | PHASE_BWD_ENC_CONVS, params=m.flat, grads=m.grad_flat, images6=img, seed=m.seed, step=7)
    torch.cuda.synchronize()
    zs = plan.buffer("z_sig_xh", torch.float32, (B, L)).double()
    ks = m.beta / B
    want = (ks * (zs - 1.0 / zs) * -torch.expm1(-zs)).sum(0)
    got = {n: t for (n, _, _), t in zip(m.param_table, m.gradients)}["encoder_x_hat/e4_sd/bias"].double()
    assert float(zs[:, bands[-14.0]].max()) < 2e-6 and float(zs[:, bands[-8.0]].max()) < 1e-3 and float(zs.min()) >= 5e-7
    bad = []
    for v, sl in bands.items():
        err, top = float((got[sl] - want[sl]).abs().max()), float(want[sl].abs().max())
        print("e4_sd/bias gradient, band at %+.0f: worst |err| / max |want| %.3e" % (v, err / top))
        if not err <= 1e-4 * top:
            bad.append((v, err / top))
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("switches,bitwise", [({}, True), ({"SV_NO_LATENT_GEMM_F32": "1"}, False)], ids=["slabs", "accumulating"])
def test_second_backward_over_one_forward_recomputes_dz(lib_built, switches, bitwise):
    """LOSS, BWD_DECODERS, BWD_ENC_HEADS | BWD_ENC_CONVS twice over ONE forward (fp32, B = 8, 32 x 32, latents 128 / 128, after two warm-up steps; a fresh
    process per case, tests/second_backward_probe.py, so that the switches are read fresh): the second backward recomputes dL/dz of the decoders instead of adding
    to the first one's, whatever state the latent block's host state machine (csrc/plan_latent.h: DzState) is in.
    slabs: the default switches -- d1's input gradient is left as K-slice slabs (InSlabs; the re-zero of gz_* is issued and unused).  The fp32 step has no atomics
    there: the two gradient sets are bitwise equal (so they were in the parent commit of the state machine, 08c7130, measured with this probe).
    accumulating: SV_NO_LATENT_GEMM_F32=1, the im2col kernel's split-K atomics add into gz_* (InGz), where a missed re-zero doubles dz and moves the encoders'
    gradients by order 1.  The atomics reorder fp32 sums (parent and this commit: 4.2e-7 of a tensor's maximum at most), so every gradient tensor is held within 2e-3 of
    its own maximum, DESIGN section 2's gradient bar."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "second_backward_probe.py")], capture_output=True, text=True,
                       env=dict(os.environ, **switches), cwd=root, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("SECOND_BACKWARD ")][-1].split(" ", 1)[1])
    worst = max(res["per"].items(), key=lambda kv: kv[1][0] / max(kv[1][1], 1e-30))
    print("second backward:", switches, "bitwise", res["bitwise"], "worst", worst)
    assert res["finite"] and len(res["per"]) == 40
    for name, (diff, gmax) in res["per"].items():
        assert gmax > 0, name
        assert diff <= 2e-3 * gmax, (name, diff, gmax)
    if bitwise:
        assert res["bitwise"]
