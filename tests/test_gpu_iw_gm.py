"""GPU tests of the mixture models' importance-weighted bound: sv_iw_gm_advance / sv_iw_gm_tables (csrc/iw_gm.hip) and
split_vae_amd/iw.py's mixture_* functions against the float64 twin of tests/iw_gm_ref.py, and the surface of --gm_iw_samples.

The kernel cases feed the twin the z the kernel STORED (checked bit for bit against zm + zs * eps first): the bound of
iw_gm_ref.ratio_bound is on the kernel's arithmetic from exact inputs."""
import numpy as np
import pytest
import torch

import gmvae_ref
import iw_gm_ref as gr
import iw_ref
from oracle import gm_ref, np_ref

pytestmark = pytest.mark.gpu

F32, BF16, I32 = torch.float32, torch.bfloat16, torch.int32
H = 32
CASES = gr.case_inputs()
WORST = {}


@pytest.fixture(scope="module")
def env(lib_built):
    assert torch.cuda.is_available()
    from split_vae_amd import _lib, iw, ops
    return ops, iw, _lib


def _cu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32).cpu().numpy()


def _advance(env, d, dtype=F32, pad=3, pinned=True, k=0, seed=0, offset=0, flags=None, **kw):
    """One sv_iw_gm_advance on the arrays of a case: (zcat [B, Lc + pad] NaN-filled before, r, comp_out)."""
    ops, iw, _lib = env
    B, n, Lg = d["zm_all"].shape
    Ll = 0 if d["mu_l"] is None else d["mu_l"].shape[1]
    zcat = torch.full((B, Lg + Ll + pad), float("nan"), dtype=dtype, device="cuda")
    r = torch.full((B,), float("nan"), dtype=F32, device="cuda")
    comp_out = torch.full((B,), -7, dtype=I32, device="cuda")
    ops.iw_gm_advance(_cu(d["logits"]), _cu(d["zm_all"]), _cu(d["zs_all"]), _cu(d["pm"]), _cu(d["ps"]), _cu(d["mu_l"]), _cu(d["sig_l"]),
                      zcat, r, comp_out, k, _lib.IW_DRAW if flags is None else flags, eps=_cu(d["eps"]) if pinned else None,
                      comp=_cu(d["comp"]) if pinned else None, seed=seed, sample_offset=offset, **kw)
    torch.cuda.synchronize()
    return zcat, r, comp_out


def _args(d):
    return d["logits"], d["zm_all"], d["zs_all"], d["pm"], d["ps"], d["mu_l"], d["sig_l"]


def _check_r(name, d, z_stored, r):
    ref, bound = gr.ratio(z_stored, *_args(d)), gr.ratio_bound(z_stored, *_args(d))
    got = r.cpu().numpy().astype(np.float64)
    ratio = np.abs(got - ref) / bound
    WORST[name] = float(ratio.max())
    print(name, "worst err / bound %.4f" % ratio.max(), "worst so far %.4f (%s)" % max((v, k) for k, v in WORST.items()))
    assert np.isfinite(got).all() and (np.abs(got - ref) <= bound).all(), (name, got, ref, bound)


# ---------------------------------------------------------------- 1. pinned draw and r
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name,d", CASES, ids=[n for n, _ in CASES])
def test_pinned_draw_is_bit_exact_and_r_is_inside_the_bound(env, name, d, dtype):
    """zcat (NaN-filled, row pitch Lg + Ll + 3) receives zm_all[b, c] + zs_all[b, c] * eps (| mu_l + sig_l * eps) bit for bit at fp32 and
    its bf16 rounding at bf16; the padding columns stay NaN; comp_out == comp; r is within the derived bound of the twin at the stored
    z: the Gaussian shapes (every S from 2 to 64, Lg beyond the LDS copy of z) and the adversarial inputs."""
    B, n, Lg = d["zm_all"].shape
    Lc = d["eps"].shape[1]
    zcat, r, comp_out = _advance(env, d, dtype)
    want = torch.from_numpy(gr.draw(d["zm_all"], d["zs_all"], d["comp"], d["mu_l"], d["sig_l"], d["eps"], dtype=np.float32)).to(dtype)
    assert np.array_equal(_bits(zcat[:, :Lc]), _bits(want))
    assert bool(torch.isnan(zcat[:, Lc:]).all())
    assert np.array_equal(comp_out.cpu().numpy(), d["comp"])
    _check_r(name + ("-bf16" if dtype == BF16 else ""), d, zcat[:, :Lc].float().cpu().numpy(), r)


def test_out_of_range_pins_are_clamped(env):
    d = dict(gr.gaussian_case(3, 5, 8, 0, seed=60))
    d["comp"] = np.array([-4, 2, 99], np.int32)
    _, _, comp_out = _advance(env, d)
    assert comp_out.cpu().tolist() == [0, 2, 4]


# ---------------------------------------------------------------- 2. against sv_iw_advance
def test_one_standard_normal_component_agrees_with_sv_iw_advance(env):
    """n = 1, pm = 0, ps = 1: the same z bits, and r within the sum of both kernels' bounds around the twin at the stored z."""
    ops, iw, _lib = env
    d = gr.gaussian_case(5, 1, 40, 24, seed=61)
    d["pm"][:], d["ps"][:] = 0.0, 1.0
    zcat, r, _ = _advance(env, d, pad=0)
    mu_g, sg_g = _cu(d["zm_all"][:, 0]), _cu(d["zs_all"][:, 0])
    z2 = torch.zeros((5, 64), dtype=F32, device="cuda")
    r2 = torch.zeros(5, dtype=F32, device="cuda")
    ops.iw_advance(mu_g, sg_g, _cu(d["mu_l"]), _cu(d["sig_l"]), z2, r2, 0, _lib.IW_DRAW, eps=_cu(d["eps"]))
    torch.cuda.synchronize()
    assert np.array_equal(_bits(zcat), _bits(z2))
    mu, sig = np.concatenate([d["zm_all"][:, 0], d["mu_l"]], 1), np.concatenate([d["zs_all"][:, 0], d["sig_l"]], 1)
    bound = gr.ratio_bound(zcat.cpu().numpy(), *_args(d)) + gr.lgvae_ratio_bound(mu, sig, d["eps"])
    diff = np.abs(r.cpu().numpy().astype(np.float64) - r2.cpu().numpy().astype(np.float64))
    print("diff / bound", (diff / bound).max())
    assert (diff <= bound).all()


# ---------------------------------------------------------------- 3. relabelling the components
@pytest.mark.parametrize("n", [2, 30, 128])
def test_component_permutation_moves_r_by_no_more_than_the_bound(env, n):
    d = gr.gaussian_case(3, n, 24, 5, seed=62 + n)
    perm = np.random.default_rng(n).permutation(n)
    inv = np.argsort(perm).astype(np.int32)
    p = dict(d, logits=d["logits"][:, perm].copy(), zm_all=d["zm_all"][:, perm].copy(), zs_all=d["zs_all"][:, perm].copy(), pm=d["pm"][perm].copy(),
             ps=d["ps"][perm].copy(), comp=inv[d["comp"]])
    za, ra, _ = _advance(env, d)
    zb, rb, cb = _advance(env, p)
    assert np.array_equal(_bits(za[:, :29]), _bits(zb[:, :29])) and np.array_equal(cb.cpu().numpy(), p["comp"])
    bound = np.maximum(gr.ratio_bound(za[:, :29].cpu().numpy(), *_args(d)), gr.ratio_bound(za[:, :29].cpu().numpy(), *_args(p)))
    diff = np.abs(ra.cpu().numpy().astype(np.float64) - rb.cpu().numpy())
    print("diff / bound", (diff / bound).max())
    assert (diff <= bound).all()


# ---------------------------------------------------------------- 4. state and finish
@pytest.mark.parametrize("Ll", [5, 0], ids=["two-branch", "one-branch"])
def test_state_over_three_samples_matches_the_twin_through_finish(env, Ll):
    """Three samples of B = 5 images: the draw's r enters the next call's accumulation; the state is NaN-filled before k = 1; the
    one-branch form has no nll_xh (joint == x).  fp64 state at 1e-12 of the twin fed the kernel's own fp32 r."""
    ops, iw, _lib = env
    B, n, Lg, K = 5, 30, 8, 3
    rng = np.random.default_rng(70)
    nx = (1.7e4 + 450 * rng.uniform(-1, 1, (K, B))).astype(np.float32)
    nh = (1.6e4 + 40 * rng.uniform(-1, 1, (K, B))).astype(np.float32) if Ll else np.zeros((K, B), np.float32)
    state = torch.full((B, 5), float("nan"), dtype=torch.float64, device="cuda")
    st = iw_ref.state_init(B)
    d0 = gr.gaussian_case(B, n, Lg, Ll, seed=71)
    dev = [_cu(a) for a in _args(d0)]
    zcat = torch.zeros((B, Lg + Ll), dtype=F32, device="cuda")
    r, comp_out = torch.zeros(B, dtype=F32, device="cuda"), torch.zeros(B, dtype=I32, device="cuda")
    for k in range(K + 1):
        flags = (_lib.IW_ACCUMULATE if k > 0 else 0) | (_lib.IW_DRAW if k < K else 0)
        if k > 0:
            st = iw_ref.state_push(st, nx[k - 1], nh[k - 1], r.cpu().numpy())
        dk = gr.gaussian_case(B, n, Lg, Ll, seed=72 + k)
        before = zcat.clone()
        ops.iw_gm_advance(*dev, zcat, r, comp_out, k, flags, nll_x=_cu(nx[k - 1]) if k else None, nll_xh=_cu(nh[k - 1]) if k and Ll else None,
                          state=state, eps=_cu(dk["eps"]), comp=_cu(dk["comp"]))
        if k > 0:
            np.testing.assert_allclose(state.cpu().numpy(), st, rtol=1e-12, atol=0)
        if k == K:
            assert torch.equal(zcat, before)             # the accumulate-only call draws nothing
    out = ops.iw_finish(state, K).cpu().numpy().astype(np.float64)
    np.testing.assert_allclose(out, iw_ref.finish(st, K), rtol=1e-6, atol=0)
    if not Ll:
        assert np.array_equal(out[:, 0], out[:, 1])


# ---------------------------------------------------------------- 5. the Philox path
def test_philox_pick_is_the_inverse_cdf_of_the_host_uniform(env):
    """4 samples x 65 images: comp_out equals the inverse CDF of sv_iw_gm_uniform_host(seed, image, sample); an image at another batch
    position draws the same component and z; two runs are bit-equal; the components follow pi."""
    ops, iw, _lib = env
    B, n, Lg, Ll, seed, off = 65, 30, 8, 5, 11, 1000
    d = gr.gaussian_case(B, n, Lg, Ll, seed=80)
    sub = {k: (v[60:63].copy() if v is not None and v.shape[0] == B else v) for k, v in d.items()}
    for k in range(4):
        z, r, c = _advance(env, d, pinned=False, k=k, seed=seed, offset=off)
        want = [gr.pick(d["logits"][b], ops.iw_gm_uniform_host(seed, off + b, k)) for b in range(B)]
        assert c.cpu().tolist() == want
        z2, r2, c2 = _advance(env, d, pinned=False, k=k, seed=seed, offset=off)
        assert torch.equal(c, c2) and np.array_equal(_bits(z[:, :13]), _bits(z2[:, :13])) and np.array_equal(_bits(r), _bits(r2))
        zs, rs, cs = _advance(env, sub, pinned=False, k=k, seed=seed, offset=off + 60)
        assert torch.equal(cs, c[60:63]) and np.array_equal(_bits(zs[:, :13]), _bits(z[60:63, :13])) and np.array_equal(_bits(rs), _bits(r[60:63]))
        _check_r("philox-k%d" % k, dict(d, comp=c.cpu().numpy()), z[:, :13].cpu().numpy(), r)
        assert not np.array_equal(_bits(_advance(env, d, pinned=False, k=k, seed=seed + 1, offset=off)[0][:, :13]), _bits(z[:, :13]))
    one = dict(gr.gaussian_case(1, 4, 2, 0, seed=81))
    one["logits"] = np.log(np.array([[0.1, 0.2, 0.3, 0.4]], np.float32))
    big = {k: (np.repeat(v, 4000, axis=0) if v is not None and v.shape[0] == 1 else v) for k, v in one.items()}
    freq = np.bincount(_advance(env, big, pinned=False, seed=3)[2].cpu().numpy(), minlength=4) / 4000
    assert np.abs(freq - [0.1, 0.2, 0.3, 0.4]).max() < 0.03, freq


# ---------------------------------------------------------------- 6. arguments
def test_entry_points_validate_arguments(env):
    ops, iw, _lib = env
    lib = _lib.load()
    z = lambda *s, dt=F32: torch.zeros(s, dtype=dt, device="cuda")      # noqa: E731
    lg, tb, pr, ml, zc, r1, st, co = z(4, 3), z(4, 3, 8), z(3, 8), z(4, 6), z(4, 16), z(4), z(4, 5, dt=torch.float64), z(4, dt=I32)
    p = lambda a: None if a is None else a.data_ptr()   # noqa: E731

    def adv(logits=lg, zm=tb, pm=pr, mu_l=ml, comp_out=co, zcat=zc, rr=r1, nx=r1, nh=r1, state=st, B=4, n=3, Lg=8, Ll=6, k=1, dt=0, ldz=16, flags=3):
        return lib.sv_iw_gm_advance(p(logits), p(zm), p(tb), p(pm), p(pr), p(mu_l), p(ml), None, None, p(comp_out), p(zcat), dt, ldz, p(rr),
                                    p(nx), p(nh), p(state), B, n, Lg, Ll, k, 0, 0, flags, None)
    bad = _lib.STATUS_BADARG
    assert adv(flags=0) == bad and adv(flags=4) == bad and adv(flags=7) == bad and adv(dt=2) == bad
    assert adv(B=0) == bad and adv(Lg=0) == bad and adv(Ll=-1) == bad and adv(k=-1) == bad and adv(rr=None) == bad
    assert adv(n=0) == bad and adv(n=129) == bad
    assert adv(logits=None, flags=2) == bad and adv(zm=None, flags=2) == bad and adv(pm=None, flags=2) == bad and adv(zcat=None, flags=2) == bad
    assert adv(comp_out=None, flags=2) == bad and adv(mu_l=None, flags=2) == bad and adv(ldz=13, flags=2) == bad
    assert adv(nx=None, flags=1) == bad and adv(nh=None, flags=1) == bad and adv(state=None, flags=1) == bad and adv(k=0, flags=1) == bad
    assert adv(logits=None, zm=None, zcat=None, comp_out=None, flags=1) == 0          # accumulate-only needs no tables
    assert adv(mu_l=None, nh=None, Ll=0) == 0 and adv() == 0                            # one branch: the local inputs may be NULL
    he = z(4, 512)
    w = dict(w_ht=z(3, 512), b_ht=z(512), w_zm=z(512, 8), b_zm=z(8), w_zs=z(512, 8), b_zs=z(8), w_pm=z(3, 8), b_pm=z(8), w_ps=z(3, 8), b_ps=z(8))

    def tab(he_=he, dt=0, B=4, n=3, hid=512, L=8, out=tb, **over):
        a = [p(over.get(k, v)) if k not in over or over[k] is not None else None for k, v in w.items()]
        return lib.sv_iw_gm_tables(p(he_), dt, *a, p(out), p(tb), p(pr), p(pr), B, n, hid, L, None)
    assert tab() == 0 and tab(he_=None) == bad and tab(dt=2) == bad and tab(B=0) == bad and tab(n=0) == bad and tab(n=129) == bad
    assert tab(hid=0) == bad and tab(hid=1025) == bad and tab(L=0) == bad and tab(out=None) == bad and tab(w_zs=None) == bad
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 7. tables
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,n,L", [(3, 5, 16), (2, 30, 128), (1, 128, 200), (65, 9, 1)])
def test_tables_match_the_twin(env, dtype, B, n, L):
    """sv_iw_gm_tables against tables() in float64 from the same (stored) he, per element.  A pre-activation a = sum_h hh_h w_h + b
    is a chain of 512 fp32 products and sums over hh = he + elu(w_ht + b_ht) (u for the sum, 5u for expm1f and its argument):
    |da| <= (512 + 2 + 6) u (|hh| . |w| + |b|).  zm = a.  A sigma = softplus(a) = max(a, 0) + log1pf(__expf(-|a|)) moves by
    sigmoid(a) da and carries (|a| + 2) u of the fast exponential (its argument is scaled by log2 e in fp32) and 2 ulp of log1pf:
    32 u sigma for |a| <= 20.  Sigmas run from 1e-6 up."""
    ops, iw, _lib = env
    rng = np.random.default_rng(B + n + L)
    p = [None] * 24
    for i, shp in ((12, (n, 512)), (13, (512,)), (14, (n, L)), (15, (L,)), (16, (n, L)), (17, (L,)), (20, (512, L)), (21, (L,)), (22, (512, L)), (23, (L,))):
        p[i] = (rng.standard_normal(shp) * (0.05 if len(shp) == 2 and shp[0] == 512 else 1.0)).astype(np.float32)
    p[23] = np.linspace(-14.0, 5.0, L).astype(np.float32)
    he = torch.from_numpy(rng.standard_normal((B, 512)).astype(np.float32)).cuda().to(dtype)
    got = ops.iw_gm_tables(he, *[_cu(p[i]) for i in (12, 13, 20, 21, 22, 23, 14, 15, 16, 17)])
    he64 = he.float().cpu().numpy().astype(np.float64)
    ref = gr.tables(p, he64)
    u, q = 2.0 ** -24, [a.astype(np.float64) for a in (p[12], p[13], p[20], p[21], p[22], p[23], p[14], p[15], p[16], p[17])]
    hh = np.abs(he64[:, None, :] + gr.elu(q[0] + q[1])[None])
    da_m, da_s = 520 * u * (hh @ np.abs(q[2]) + np.abs(q[3])), 520 * u * (hh @ np.abs(q[4]) + np.abs(q[5]))
    sigm = lambda s: -np.expm1(-s)                     # noqa: E731  sigmoid(a) from sigma = softplus(a)
    bounds = (da_m, sigm(ref[1]) * da_s + 32 * u * ref[1], 2 * u * np.abs(ref[2]), sigm(ref[3]) * 2 * u * np.abs(q[8] + q[9]) + 32 * u * ref[3])
    assert ref[1].min() < 3e-6
    for g, w, b, nm in zip(got, ref, bounds, ("zm_all", "zs_all", "pm", "ps")):
        err = np.abs(g.cpu().numpy().astype(np.float64) - w)
        print(nm, "worst err / bound", (err / b).max())
        assert (err <= 1.01 * b).all(), nm


# ---------------------------------------------------------------- 8. the models
def _images(B, patch=4, seed=0):
    rng = np.random.Generator(np.random.PCG64(seed))
    x = (rng.integers(0, 256, size=(B, H, H, 3)) / 255.0 * 2 - 1).astype(np.float32)
    perm = np.stack([np.random.Generator(np.random.PCG64(seed + 1 + b)).permutation((H // patch) ** 2) for b in range(B)]).astype(np.int32)
    return np_ref.scramble_batch(x, perm, patch).astype(np.float32)


def _params(split, L, n, zero=False):
    if split:
        ps = gm_ref.gm_glorot_init(H, H, seed=3, global_latent=L, local_latent=L, y_size=n)
    else:
        ps = gmvae_ref.gmvae_glorot_init(H, H, seed=3, latent=L, y_size=n)
    if zero:
        return [np.zeros_like(p) for p in ps]
    rng = np.random.default_rng(9)
    for i in range(1, len(ps), 2):                    # non-zero biases
        ps[i] = (ps[i] + rng.standard_normal(ps[i].shape) * 0.05).astype(np.float32)
    return ps


def _model(split, L, n, dtype, params):
    from split_vae_amd.gm import LGGMVae
    from split_vae_amd.gmvae import GMVae
    m = LGGMVae(L, L, [-1, H, H, 3], n, 0.4, dtype=dtype, device="cuda", seed=1) if split else GMVae(L, [-1, H, H, 3], n, 0.4, dtype=dtype, device="cuda", seed=1)
    m.set_weights(params)
    return m


def _pins(K, B, n, Lc, seed=13):
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.standard_normal((K, B, Lc)).astype(np.float32), rng.integers(0, n, (K, B)).astype(np.int32)


@pytest.mark.parametrize("L,n", [(16, 5), (128, 30)], ids=["y5-l16", "defaults"])
@pytest.mark.parametrize("split", [True, False], ids=["lggmvae", "gmvae"])
def test_end_to_end_fp32_matches_the_twin(env, deterministic, split, L, n):
    """SVHN-32, Glorot weights, pinned eps and comp, B = 3, 3 samples: per-image joint, x and elbo within rtol 1e-4 / atol 1e-5 of
    the float64 estimator (L_K is 1-Lipschitz in the max-norm of the log-weights; the bound of test_gpu_iw's end-to-end test)."""
    ops, iw, _lib = env
    B, K = 3, 3
    params = _params(split, L, n)
    model = _model(split, L, n, "f32", params)
    calls = model._calls
    images = _images(B, seed=2)
    eps, comp = _pins(K, B, n, 2 * L if split else L)
    got = np.stack([t.cpu().numpy().astype(np.float64) for t in iw.mixture_log_likelihood(model, _cu(images), K, eps=_cu(eps), comp=_cu(comp))], axis=1)
    ref, _, _ = gr.estimator(params, images, split, eps=eps, comp=comp)
    print("got", got, "twin", ref, "rel", np.abs(got - ref) / np.abs(ref))
    np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-5)
    assert model._calls == calls
    if not split:
        assert np.array_equal(got[:, 0], got[:, 1])


@pytest.mark.parametrize("split", [True, False], ids=["lggmvae", "gmvae"])
def test_closed_form_when_every_posterior_component_is_its_prior_component(env, split):
    """All weights zero; the biases of z_sig and z_prior_sig both 0.3, of the local e4_sd ln(e - 1): every posterior component is
    N(0, softplus(0.3)) = its prior component, pi is uniform, q(z_l) = N(0, 1), and the decoders give mean 0, log-scale 0 whatever z
    is.  So r = 0 (to rounding) and for any draws L_joint = elbo = -(c_x + c_xh), L_x = -c_x (iw_ref.closed_form_nll)."""
    ops, iw, _lib = env
    B, K, L, n = 4, 3, 16, 5
    params = _params(split, L, n, zero=True)
    params[17][:], params[23][:] = 0.3, 0.3
    if split:
        params[33][:] = np.float32(np.log(np.e - 1.0))
    model = _model(split, L, n, "f32", params)
    images = _images(B, seed=5)
    Lj, Lx, el = (t.cpu().numpy().astype(np.float64) for t in iw.mixture_log_likelihood(model, _cu(images), K, seed=3))
    cx, ch = iw_ref.closed_form_nll(images)
    if not split:
        ch = 0.0
    np.testing.assert_allclose(Lj, -(cx + ch), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(el, -(cx + ch), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(Lx, -cx, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("split", [True, False], ids=["lggmvae", "gmvae"])
def test_one_sample_pass_leaves_the_nll_of_test_step(env, deterministic, monkeypatch, split, dtype):
    """The latents test_step left in zcat, put back behind the draw of a K = 1 evaluation: the decoder + loss pass is the same kernels
    over the same latents, so the plan's nll_x (and nll_xh) are the same bits."""
    ops, iw, _lib = env
    from split_vae_amd import gm, gmvae
    B, L, n = 4, 128, 30
    model = _model(split, L, n, dtype, _params(split, L, n))
    images = _cu(_images(B, seed=6))
    (gm.test_step_lg_gm_vae if split else gmvae.test_step_gm_vae)(model, images)
    plan = model.plan(B)
    names = ("nll_x", "nll_xh") if split else ("nll_x",)
    Lc = 2 * L if split else L
    want = [plan.buffer(nm, F32, (B,)).clone() for nm in names]
    want_z = plan.buffer("zcat", model.dtype, (B, Lc)).clone()
    for nm in names:
        plan.buffer(nm, F32, (B,)).zero_()
    real = ops.iw_gm_advance

    def spy(*a, **kw):
        real(*a, **kw)
        if a[11] & _lib.IW_DRAW:
            a[7].copy_(want_z)
    monkeypatch.setattr(ops, "iw_gm_advance", spy)
    iw.mixture_log_likelihood(model, images, 1)
    for nm, w in zip(names, want):
        assert float(w.abs().min()) > 0 and np.array_equal(_bits(plan.buffer(nm, F32, (B,))), _bits(w)), nm


BF16_REL = 2 * 2.3e-5      # measured worst case on the MI355X: 2.27e-5 (L_x of one GMVae image: 0.44 of 19 382 nats), times two


@pytest.mark.parametrize("split", [True, False], ids=["lggmvae", "gmvae"])
def test_end_to_end_bf16_against_the_twin_on_the_stored_latents(env, deterministic, monkeypatch, split):
    """bf16 plan, defaults (30, 128), B = 3, 3 samples: the twin decodes and scores the stored z~ with its own float64 tables (its he
    is the float64 encoder's, the device's is the bf16 encoder's: most of the distance).  Bound: twice the worst relative error
    measured on the MI355X (as the other bf16 bounds of this suite).  Measured: LGGMVae 1.65e-5 (L_x), 1.15e-5 (L_joint), 1.11e-5
    (elbo); GMVae 2.27e-5 (L_x = L_joint), 2.20e-5 (elbo) at worst over the three images."""
    ops, iw, _lib = env
    B, K, L, n = 3, 3, 128, 30
    params = _params(split, L, n)
    model = _model(split, L, n, "bf16", params)
    images = _images(B, seed=2)
    eps, comp = _pins(K, B, n, 2 * L if split else L)
    stored = []
    real = ops.iw_gm_advance

    def spy(*a, **kw):
        real(*a, **kw)
        if a[11] & _lib.IW_DRAW:
            stored.append(a[7].float().clone())
    monkeypatch.setattr(ops, "iw_gm_advance", spy)
    got = np.stack([t.cpu().numpy().astype(np.float64) for t in iw.mixture_log_likelihood(model, _cu(images), K, eps=_cu(eps), comp=_cu(comp))], axis=1)
    ref, _, _ = gr.estimator(params, images, split, z_stored=torch.stack(stored).cpu().numpy())
    rel = np.abs(got - ref) / np.abs(ref)
    print("got", got, "twin", ref, "rel", rel, "worst", rel.max())
    assert rel.max() <= BF16_REL


# ---------------------------------------------------------------- 9. surface
def test_cli_prints_the_mixture_bound_and_evaluate_reproduces_it(env, deterministic, tmp_path, monkeypatch, capsys):
    from split_vae_amd import evaluate, main as svmain
    monkeypatch.chdir(tmp_path)
    argv = ["--model", "lggmvae", "--gm_iw_samples", "2", "--synthetic", "-no_label"]
    path = svmain.main(argv + ["--training_steps", "2", "--log_every", "2"])
    out = capsys.readouterr().out
    lines = [l for l in out.splitlines() if l.startswith("Test IW-2 mixture bound: ")]
    assert len(lines) == 2 and "Training done!" in out, out
    for l in lines:
        joint, x, bpd = (float(l.split(key)[1].split()[0].rstrip(",;")) for key in ("joint ", ", x ", "bits/dim "))
        assert np.isfinite([joint, x, bpd]).all() and x >= joint and bpd > 0
        assert abs(bpd - iw_ref.bits_per_dim(x, 32, 32)) < 1e-4
    res = evaluate.main(argv + ["--weights", path])
    again = [l for l in capsys.readouterr().out.splitlines() if l.startswith("Test IW-")]
    assert again == [lines[-1]] and res["n_images"] > 0 and set(res) >= {"gm_iw_joint", "gm_iw_x", "gm_bits_per_dim_x"}


def test_k_samples_cost_k_plus_one_advances_and_no_host_round_trip(env, monkeypatch):
    ops, iw, _lib = env
    B, K, L, n = 4, 5, 128, 30
    model = _model(True, L, n, "f32", _params(True, L, n))
    images = _cu(_images(B, seed=9))
    iw.mixture_log_likelihood(model, images, 1)      # plan creation and first launches outside the count
    torch.cuda.synchronize()
    log = []
    real_adv, real_fin, real_tab, real_step = ops.iw_gm_advance, ops.iw_finish, ops.iw_gm_tables, ops.LGVaePlan.step
    real_sync, real_cpu, real_item, real_ssync = torch.cuda.synchronize, torch.Tensor.cpu, torch.Tensor.item, torch.cuda.Stream.synchronize
    monkeypatch.setattr(ops, "iw_gm_advance", lambda *a, **kw: (log.append(("advance", a[11])), real_adv(*a, **kw))[1])
    monkeypatch.setattr(ops, "iw_finish", lambda *a, **kw: (log.append(("finish", 0)), real_fin(*a, **kw))[1])
    monkeypatch.setattr(ops, "iw_gm_tables", lambda *a, **kw: (log.append(("tables", 0)), real_tab(*a, **kw))[1])
    monkeypatch.setattr(ops.LGVaePlan, "step", lambda self, phases, **kw: (log.append(("step", phases)), real_step(self, phases, **kw))[1])
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **kw: (log.append(("sync", 0)), real_sync(*a, **kw))[1])
    monkeypatch.setattr(torch.cuda.Stream, "synchronize", lambda self: (log.append(("sync", 0)), real_ssync(self))[1])
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **kw: (log.append(("cpu", 0)), real_cpu(self, *a, **kw))[1])
    monkeypatch.setattr(torch.Tensor, "item", lambda self: (log.append(("item", 0)), real_item(self))[1])
    out = iw.mixture_log_likelihood(model, images, K)
    monkeypatch.undo()
    D, A = _lib.IW_DRAW, _lib.IW_ACCUMULATE
    dec = _lib.PHASE_FWD_DECODERS | _lib.PHASE_LOSS
    want = [("step", _lib.PHASE_PREP | _lib.PHASE_FWD_ENCODERS), ("tables", 0), ("advance", D)]
    for k in range(1, K + 1):
        want += [("step", dec), ("advance", A | D if k < K else A)]
    assert log == want + [("finish", 0)], log
    assert all(torch.isfinite(t).all() for t in out)


def test_only_the_mixture_models_are_accepted(env):
    ops, iw, _lib = env
    from split_vae_amd.model import LGVae
    with pytest.raises(TypeError, match="LGGMVae and GMVae only"):
        iw.mixture_log_likelihood(LGVae(128, 128, image_shape=(None, H, H, 3), dtype="f32"), _cu(_images(2)), 1)
