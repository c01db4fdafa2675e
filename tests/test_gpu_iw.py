"""GPU tests of the importance-weighted log-likelihood: sv_iw_advance / sv_iw_finish (csrc/iw.hip) and split_vae_amd/iw.py against
the float64 twin of tests/iw_ref.py, and the flag's surface in main.py / evaluate.py."""
import numpy as np
import pytest
import torch

import iw_ref
from oracle import np_ref

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16


@pytest.fixture(scope="module")
def env(lib_built):
    assert torch.cuda.is_available()
    from split_vae_amd import _lib, iw, ops
    return ops, iw, _lib


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32).cpu().numpy()


def _images(B, H, patch=4, seed=0):
    rng = np.random.Generator(np.random.PCG64(seed))
    x = (rng.integers(0, 256, size=(B, H, H, 3)) / 255.0 * 2 - 1).astype(np.float32)
    perm = np.stack([np.random.Generator(np.random.PCG64(seed + 1 + b)).permutation((H // patch) ** 2) for b in range(B)]).astype(np.int32)
    return np_ref.scramble_batch(x, perm, patch).astype(np.float32)


def _model(H, dtype, params_np, L=128, seed=0):
    from split_vae_amd.model import LGVae
    m = LGVae(L, L, image_shape=(None, H, H, 3), dtype=dtype, seed=seed)
    m.set_weights(params_np)
    return m


def _glorot(H, L=128, bias_seed=9):
    params = np_ref.glorot_init(H, H, seed=3, global_latent=L, local_latent=L)
    rng = np.random.default_rng(bias_seed)
    for i in range(1, len(params), 2):              # non-zero biases, as tests/test_gpu_step.py
        params[i] = (rng.standard_normal(params[i].shape) * 0.05).astype(np.float32)
    return params


# ---------------------------------------------------------------- 1. draw, bit for bit
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("L", [128, 64])
def test_draw_writes_the_zcat_of_the_forward_bit_for_bit(env, dtype, L):
    """The plan's inference with pinned eps leaves z = mu + sig * eps in zcat; sv_iw_advance(DRAW) with the same eps on the plan's
    z_mean / z_sig writes the same bits, for sig from ~1e-6 to ~10.  r against the twin at rtol 1e-5 (a sum of <= 256 fp32 terms
    of order 1 to 1e7 with little cancellation, against float64: a few 1e-7 relative); the bf16 twin is fed the stored z~."""
    ops, iw, _lib = env
    B, H = 5, 32
    params = _glorot(H, L)
    for i in (9, 19):                                # e4_sd biases: softplus from ~1e-6 to ~10 across the dimensions
        params[i] = np.linspace(-14.0, 10.0, L).astype(np.float32)
    plan = ops.LGVaePlan(B, H, H, global_latent=L, local_latent=L, beta=1.0, dtype=dtype)
    P = torch.zeros(plan.n_params, dtype=F32)
    for (name, off, shape), p in zip(plan.param_table, params):
        P[off:off + p.size] = torch.from_numpy(np.ascontiguousarray(p)).flatten()
    P = P.cuda()
    eps = np.random.Generator(np.random.PCG64(11)).standard_normal((B, 2 * L)).astype(np.float32)
    ex, eh = torch.from_numpy(eps[:, :L].copy()).cuda(), torch.from_numpy(eps[:, L:].copy()).cuda()
    plan.step(_lib.PHASE_INFER, params=P, images6=torch.from_numpy(_images(B, H)).cuda(), eps_x=ex, eps_x_hat=eh)
    want = plan.buffer("zcat", dtype, (B, 2 * L)).clone()
    mu = [plan.buffer("z_mean_" + s, F32, (B, L)) for s in ("x", "xh")]
    sig = [plan.buffer("z_sig_" + s, F32, (B, L)) for s in ("x", "xh")]
    got = torch.full((B, 2 * L), 7.0, dtype=dtype, device="cuda")
    r = torch.full((B,), float("nan"), dtype=F32, device="cuda")
    ops.iw_advance(mu[0], sig[0], mu[1], sig[1], got, r, 0, _lib.IW_DRAW, eps=torch.from_numpy(eps).cuda())
    torch.cuda.synchronize()
    assert np.array_equal(_bits(got), _bits(want))
    mu_np, sig_np = (torch.cat(t, 1).cpu().numpy() for t in (mu, sig))
    assert sig_np.min() < 3e-6 and sig_np.max() > 9.0
    if dtype == F32:
        ref = iw_ref.latent_ratio(mu_np, sig_np, eps=eps)
    else:
        ref = iw_ref.latent_ratio(mu_np, sig_np, z_stored=got.float().cpu().numpy())
    print("r", r.cpu().numpy(), "twin", ref)
    np.testing.assert_allclose(r.cpu().numpy().astype(np.float64), ref, rtol=1e-5, atol=0)


# ---------------------------------------------------------------- 2. state
def test_state_and_finish_match_the_twin(env):
    """Synthetic nll_x, nll_xh, r for K = 6 at B = 5 (not a multiple of the 4 waves of a workgroup), log-weights up to 1e3 nats
    apart: the fp64 state and the accumulator at 1e-12 relative (a handful of fp64 exp / log roundings per update), the fp32
    outputs at 1e-6; the accumulator after two batches is the sum of both."""
    ops, iw, _lib = env
    B, K = 5, 6
    rng = np.random.default_rng(21)
    nx = (1.7e4 + 450 * rng.uniform(-1, 1, (K, B))).astype(np.float32)
    nh = (1.6e4 + 40 * rng.uniform(-1, 1, (K, B))).astype(np.float32)
    rr = (-300 + 10 * rng.uniform(-1, 1, (K, B))).astype(np.float32)
    spread = (-nx.astype(np.float64) - nh + rr).max(0) - (-nx.astype(np.float64) - nh + rr).min(0)
    assert spread.max() > 500 and spread.max() <= 1e3
    dummy = torch.ones((B, 8), dtype=F32, device="cuda")
    zcat = torch.zeros((B, 16), dtype=F32, device="cuda")
    acc = torch.zeros(4, dtype=torch.float64, device="cuda")
    acc_ref = np.zeros(4)
    for batch in range(2):
        n = B if batch == 0 else 3                   # the second batch: fewer images than waves in a workgroup
        state = torch.full((n, 5), float("nan"), dtype=torch.float64, device="cuda")
        st = iw_ref.state_init(n)
        for k in range(K):
            r = torch.from_numpy(rr[k, :n].copy()).cuda()
            ops.iw_advance(dummy[:n], dummy[:n], dummy[:n], dummy[:n], zcat[:n], r, k + 1, _lib.IW_ACCUMULATE,
                           nll_x=torch.from_numpy(nx[k, :n].copy()).cuda(), nll_xh=torch.from_numpy(nh[k, :n].copy()).cuda(), state=state)
            st = iw_ref.state_push(st, nx[k, :n], nh[k, :n], rr[k, :n])
            np.testing.assert_allclose(state.cpu().numpy(), st, rtol=1e-12, atol=0)
        out = ops.iw_finish(state, K, acc=acc)
        ref = iw_ref.finish(st, K)
        np.testing.assert_allclose(out.cpu().numpy().astype(np.float64), ref, rtol=1e-6, atol=0)
        acc_ref = iw_ref.acc_add(acc_ref, ref)
        np.testing.assert_allclose(acc.cpu().numpy(), acc_ref, rtol=1e-12, atol=0)
    assert acc.cpu().numpy()[3] == 8
    assert float(zcat.abs().max()) == 0.0            # accumulate-only calls draw nothing


def test_finish_sums_more_images_than_one_workgroup_has_threads(env):
    ops, iw, _lib = env
    B, K = 300, 2
    rng = np.random.default_rng(22)
    st = np.stack([-1.7e4 + rng.standard_normal(B), 1 + rng.uniform(0, 1, B), -1e4 + rng.standard_normal(B), 1 + rng.uniform(0, 1, B),
                   -3.4e4 + rng.standard_normal(B)], axis=1)
    acc = torch.zeros(4, dtype=torch.float64, device="cuda")
    out = ops.iw_finish(torch.from_numpy(st).cuda(), K, acc=acc)
    ref = iw_ref.finish(st, K)
    np.testing.assert_allclose(out.cpu().numpy().astype(np.float64), ref, rtol=1e-6, atol=0)
    np.testing.assert_allclose(acc.cpu().numpy(), iw_ref.acc_add(np.zeros(4), ref), rtol=1e-12, atol=0)


def test_entry_points_validate_arguments(env):
    ops, iw, _lib = env
    lib = _lib.load()
    t = torch.zeros((4, 8), dtype=F32, device="cuda")
    z = torch.zeros((4, 16), dtype=F32, device="cuda")
    r, st = torch.zeros(4, dtype=F32, device="cuda"), torch.zeros((4, 5), dtype=torch.float64, device="cuda")
    p = lambda a: None if a is None else a.data_ptr()   # noqa: E731

    def adv(zm=t, zc=z, rr=r, nx=r, state=st, B=4, Lg=8, Ll=8, k=1, dt=0, ldz=16, flags=3):
        return lib.sv_iw_advance(p(zm), p(t), p(t), p(t), None, p(zc), dt, ldz, p(rr), p(nx), p(r), p(state), B, Lg, Ll, k, 0, 0, flags, None)
    bad = _lib.STATUS_BADARG
    assert adv(flags=0) == bad and adv(flags=4) == bad and adv(flags=7) == bad and adv(dt=2) == bad
    assert adv(B=0) == bad and adv(Lg=0) == bad and adv(Ll=-1) == bad and adv(k=-1) == bad and adv(rr=None) == bad
    assert adv(zm=None, flags=2) == bad and adv(zc=None, flags=2) == bad and adv(ldz=15, flags=2) == bad
    assert adv(nx=None, flags=1) == bad and adv(state=None, flags=1) == bad and adv(k=0, flags=1) == bad
    assert adv(zm=None, zc=None, flags=1) == 0       # accumulate-only needs no latents
    out = torch.zeros((4, 3), dtype=F32, device="cuda")
    assert lib.sv_iw_finish(None, 1, p(out), None, 4, None) == bad and lib.sv_iw_finish(p(st), 1, None, None, 4, None) == bad
    assert lib.sv_iw_finish(p(st), 0, p(out), None, 4, None) == bad and lib.sv_iw_finish(p(st), 1, p(out), None, 0, None) == bad
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 3. closed form
@pytest.mark.parametrize("K", [1, 4])
def test_closed_form_with_a_standard_normal_posterior(env, K):
    """All weights and biases zero except the two e4_sd biases at ln(e - 1): mu = 0, sig = 1, z = eps, r = 0 (to the rounding of
    softplus), and the decoders give mean 0, log-scale 0 whatever z is.  So for any K and any draws L_joint = elbo = -(c_x + c_xh)
    and L_x = -c_x, c from the fp64 oracle's discretised-logistic loss.  Bound: rtol 1e-4 / atol 1e-5."""
    ops, iw, _lib = env
    B, H, L = 6, 32, 128
    params = [np.zeros_like(p) for p in np_ref.glorot_init(H, H, seed=3)]
    for i in (9, 19):
        params[i][:] = np.float32(np.log(np.e - 1.0))
    model = _model(H, "f32", params)
    images = _images(B, H, seed=5)
    Lj, Lx, el = (t.cpu().numpy().astype(np.float64) for t in iw.log_likelihood(model, torch.from_numpy(images).cuda(), K, seed=3))
    cx, ch = iw_ref.closed_form_nll(images)
    print("L_joint", Lj, "want", -(cx + ch))
    np.testing.assert_allclose(Lj, -(cx + ch), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(el, -(cx + ch), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(Lx, -cx, rtol=1e-4, atol=1e-5)


# ---------------------------------------------------------------- 4. end to end against the twin
def _end_to_end(env, H, B, K, dtype):
    ops, iw, _lib = env
    L = 128
    params = _glorot(H)
    model = _model(H, dtype, params)
    images = _images(B, H, patch=8 if H > 32 else 1, seed=2)
    eps = np.random.Generator(np.random.PCG64(13)).standard_normal((K, B, 2 * L)).astype(np.float32)
    eps_d = torch.from_numpy(eps).cuda()
    got = np.stack([t.cpu().numpy().astype(np.float64) for t in iw.log_likelihood(model, torch.from_numpy(images).cuda(), K, eps=eps_d)], axis=1)
    if model.dtype == F32:
        ref, _, _ = iw_ref.estimator(params, images, eps=eps)
    else:
        # the latents the bf16 plan stored: the plan's z_mean / z_sig still hold this batch's encoder outputs
        plan = model.plan(B)
        mu = [plan.buffer("z_mean_" + s, F32, (B, L)) for s in ("x", "xh")]
        sig = [plan.buffer("z_sig_" + s, F32, (B, L)) for s in ("x", "xh")]
        zs, r = torch.empty((K, B, 2 * L), dtype=BF16, device="cuda"), torch.empty(B, dtype=F32, device="cuda")
        for k in range(K):
            ops.iw_advance(mu[0], sig[0], mu[1], sig[1], zs[k], r, k, _lib.IW_DRAW, eps=eps_d[k])
        ref, _, _ = iw_ref.estimator(params, images, z_stored=zs.float().cpu().numpy())
    return got, ref


@pytest.mark.parametrize("H,B,K", [(32, 3, 4), (64, 2, 2)], ids=["svhn32", "celeba64"])
def test_end_to_end_fp32_matches_the_twin(env, deterministic, H, B, K):
    """Pinned eps, Glorot weights, fp32 plan with fixed-order reductions: per-image L_joint, L_x, elbo within rtol 1e-4 / atol 1e-5
    of the float64 estimator (L_K is 1-Lipschitz in the max-norm of the log-weights: the per-image bound on the ELBO terms of
    SURVEY 8c carries over)."""
    got, ref = _end_to_end(env, H, B, K, "f32")
    print("got", got, "twin", ref, "rel", np.abs(got - ref) / np.abs(ref))
    np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-5)


BF16_REL = 2 * 7.7e-6      # measured worst case on the MI355X: 7.64e-6 (L_x of one image: 0.15 of 19 164 nats), times two


def test_end_to_end_bf16_against_the_twin_on_the_stored_latents(env, deterministic):
    """bf16 plan, B = 3, K = 4: the twin decodes the stored z~ with its own float64 encoder outputs in the density ratio.  Bound:
    twice the measured worst relative error (as the other bf16 bounds of this suite).  Measured: L_joint 3.2e-6, L_x 7.6e-6, elbo
    8.0e-7 relative at worst over the three images."""
    got, ref = _end_to_end(env, 32, 3, 4, "bf16")
    rel = np.abs(got - ref) / np.abs(ref)
    print("got", got, "twin", ref, "rel", rel, "worst", rel.max())
    assert rel.max() <= BF16_REL


# ---------------------------------------------------------------- 5. consistency with test_step
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_one_sample_pass_leaves_the_nll_of_test_step(env, deterministic, dtype):
    """K = 1 with the eps a test_step call used: same kernels over the same latents, so the plan's nll_x / nll_xh are the same bits."""
    ops, iw, _lib = env
    from split_vae_amd import trainer
    B, H, L = 4, 32, 128
    model = _model(H, dtype, _glorot(H))
    images = torch.from_numpy(_images(B, H, seed=6)).cuda()
    eps = torch.from_numpy(np.random.Generator(np.random.PCG64(14)).standard_normal((B, 2 * L)).astype(np.float32)).cuda()
    trainer.test_step(model, images, eps=(eps[:, :L].contiguous(), eps[:, L:].contiguous()))
    plan = model.plan(B)
    want = [plan.buffer(n, F32, (B,)).clone() for n in ("nll_x", "nll_xh")]
    want_z = plan.buffer("zcat", model.dtype, (B, 2 * L)).clone()
    plan.buffer("nll_x", F32, (B,)).zero_()
    plan.buffer("nll_xh", F32, (B,)).zero_()
    Lj, Lx, el = iw.log_likelihood(model, images, 1, eps=eps[None].contiguous())
    assert np.array_equal(_bits(plan.buffer("zcat", model.dtype, (B, 2 * L))), _bits(want_z))
    for n, w in zip(("nll_x", "nll_xh"), want):
        assert float(w.abs().min()) > 0 and np.array_equal(_bits(plan.buffer(n, F32, (B,))), _bits(w)), n
    assert torch.equal(Lj, el)                       # K = 1: the bound is the single weight


# ---------------------------------------------------------------- 6. keying
def test_philox_draw_is_a_function_of_seed_image_and_sample(env):
    """zcat rows of image i for k = 0..2: the same bits in the batch [a, b, c] at sample_offset 0 and in the batch [c] at
    sample_offset 2; other images, samples and seeds draw other numbers."""
    ops, iw, _lib = env
    L = 40                                           # not a multiple of the wave: lanes 40..63 idle
    rng = np.random.default_rng(31)
    mu = [torch.from_numpy(rng.standard_normal((3, L)).astype(np.float32)).cuda() for _ in range(2)]
    sig = [torch.from_numpy(rng.uniform(0.1, 2.0, (3, L)).astype(np.float32)).cuda() for _ in range(2)]

    def draw(rows, off, k, seed=5, dtype=F32):
        z, r = torch.zeros((len(rows), 2 * L), dtype=dtype, device="cuda"), torch.zeros(len(rows), dtype=F32, device="cuda")
        ops.iw_advance(mu[0][rows].contiguous(), sig[0][rows].contiguous(), mu[1][rows].contiguous(), sig[1][rows].contiguous(), z, r, k,
                       _lib.IW_DRAW, seed=seed, sample_offset=off)
        return _bits(z), _bits(r)
    for dtype in (F32, BF16):
        seen = []
        for k in range(3):
            za, ra = draw([0, 1, 2], 0, k, dtype=dtype)
            zc, rc = draw([2], 2, k, dtype=dtype)
            assert np.array_equal(za[2:], zc) and np.array_equal(ra[2:], rc)
            assert np.array_equal(za, draw([0, 1, 2], 0, k, dtype=dtype)[0])
            seen.append(za)
        assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
        assert not np.array_equal(draw([2], 1, 0, dtype=dtype)[0], draw([2], 2, 0, dtype=dtype)[0])
        assert not np.array_equal(draw([2], 2, 0, seed=6, dtype=dtype)[0], draw([2], 2, 0, dtype=dtype)[0])
    # the draws are standard normal, and the global and local halves are different streams
    big = torch.zeros((64, 256), dtype=F32, device="cuda")
    one, zero = torch.ones((64, 128), dtype=F32, device="cuda"), torch.zeros((64, 128), dtype=F32, device="cuda")
    ops.iw_advance(zero, one, zero, one, big, torch.zeros(64, dtype=F32, device="cuda"), 0, _lib.IW_DRAW, seed=1)
    e = big.cpu().numpy().astype(np.float64)
    assert abs(e.mean()) < 0.03 and abs(e.std() - 1.0) < 0.03 and not np.array_equal(e[:, :128], e[:, 128:])


def test_state_does_not_depend_on_K_and_runs_repeat_bit_for_bit(env, deterministic, monkeypatch):
    ops, iw, _lib = env
    B, H = 3, 32
    model = _model(H, "f32", _glorot(H))
    images = torch.from_numpy(_images(B, H, seed=8)).cuda()
    states = []
    real = ops.iw_advance

    def spy(*a, **kw):
        real(*a, **kw)
        if a[7] & _lib.IW_ACCUMULATE:
            states[-1][a[6]] = kw["state"].clone()
    monkeypatch.setattr(ops, "iw_advance", spy)
    outs = []
    for K in (6, 3, 6):
        states.append({})
        outs.append(torch.stack(iw.log_likelihood(model, images, K, seed=4)).cpu().numpy())
    assert sorted(states[0]) == [1, 2, 3, 4, 5, 6] and sorted(states[1]) == [1, 2, 3]
    for k in (1, 2, 3):
        assert torch.equal(states[0][k], states[1][k])
    assert np.array_equal(outs[0].view(np.int32), outs[2].view(np.int32))
    assert all(torch.equal(states[0][k], states[2][k]) for k in states[0])
    assert (outs[0][1] >= outs[0][0]).all() and (outs[0][0] >= outs[0][2]).all()     # L_x >= L_joint >= elbo


# ---------------------------------------------------------------- 7. surface
def test_cli_prints_the_bound_and_evaluate_reproduces_it(env, deterministic, tmp_path, monkeypatch, capsys):
    from split_vae_amd import evaluate, main as svmain
    monkeypatch.chdir(tmp_path)
    argv = ["--synthetic", "-no_label", "--batch_size", "8", "--training_steps", "2", "--log_every", "2"]
    path = svmain.main(argv + ["--iw_samples", "3"])
    out = capsys.readouterr().out
    lines = [l for l in out.splitlines() if l.startswith("Test IW-3 bound: ")]
    assert len(lines) == 2 and "Training done!" in out, out
    for l in lines:
        joint, x, bpd = (float(l.split(key)[1].split()[0].rstrip(",;")) for key in ("joint ", ", x ", "bits/dim "))
        assert np.isfinite([joint, x, bpd]).all() and x >= joint and bpd > 0
        assert abs(bpd - iw_ref.bits_per_dim(x, 32, 32)) < 1e-4
    res = evaluate.main(argv + ["--iw_samples", "3", "--weights", path])
    again = [l for l in capsys.readouterr().out.splitlines() if l.startswith("Test IW-")]
    assert again == [lines[-1]] and res["n_images"] == 32
    svmain.main(argv)
    assert "Test IW-" not in capsys.readouterr().out


# ---------------------------------------------------------------- 8. no sync in the loop
def test_k_samples_cost_k_plus_one_advances_and_no_host_round_trip(env, monkeypatch):
    ops, iw, _lib = env
    B, H, K = 4, 32, 5
    model = _model(H, "f32", _glorot(H))
    images = torch.from_numpy(_images(B, H, seed=9)).cuda()
    iw.log_likelihood(model, images, 1)              # plan creation and first launches outside the count
    torch.cuda.synchronize()
    log = []
    real_adv, real_fin, real_step = ops.iw_advance, ops.iw_finish, ops.LGVaePlan.step
    real_sync, real_cpu, real_item, real_ssync = torch.cuda.synchronize, torch.Tensor.cpu, torch.Tensor.item, torch.cuda.Stream.synchronize
    monkeypatch.setattr(ops, "iw_advance", lambda *a, **kw: (log.append(("advance", a[7])), real_adv(*a, **kw))[1])
    monkeypatch.setattr(ops, "iw_finish", lambda *a, **kw: (log.append(("finish", 0)), real_fin(*a, **kw))[1])
    monkeypatch.setattr(ops.LGVaePlan, "step", lambda self, phases, **kw: (log.append(("step", phases)), real_step(self, phases, **kw))[1])
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **kw: (log.append(("sync", 0)), real_sync(*a, **kw))[1])
    monkeypatch.setattr(torch.cuda.Stream, "synchronize", lambda self: (log.append(("sync", 0)), real_ssync(self))[1])
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **kw: (log.append(("cpu", 0)), real_cpu(self, *a, **kw))[1])
    monkeypatch.setattr(torch.Tensor, "item", lambda self: (log.append(("item", 0)), real_item(self))[1])
    out = iw.log_likelihood(model, images, K)
    monkeypatch.undo()
    kinds = [k for k, _ in log]
    assert kinds.count("advance") == K + 1 and kinds.count("finish") == 1
    first, last = kinds.index("advance"), len(kinds) - 1 - kinds[::-1].index("advance")
    assert not {"sync", "cpu", "item"} & set(kinds[first:last + 1]), kinds
    D, A = _lib.IW_DRAW, _lib.IW_ACCUMULATE
    dec = _lib.PHASE_FWD_DECODERS | _lib.PHASE_LOSS
    want = [("step", _lib.PHASE_PREP | _lib.PHASE_FWD_ENCODERS), ("advance", D)]
    for k in range(1, K + 1):
        want += [("step", dec), ("advance", A | D if k < K else A)]
    assert log == want + [("finish", 0)]
    assert all(torch.isfinite(t).all() for t in out)
