"""CPU: the float64 restatements of tests/pointwise_ref.py against the oracle functions they restate (1e-12 relative where both are float64) and against closed forms;
the Philox mirrors; every condition the input generators promise to tests/test_gpu_pointwise.py; and the argument checks of the pointwise entry points, which answer
before any launch (no GPU)."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pointwise_ref as R  # noqa: E402
from oracle import np_ref, torch_ref  # noqa: E402

F64 = torch.float64


def rel_close(a, b, rtol=1e-12):
    a, b = a.to(F64), b.to(F64)
    assert a.shape == b.shape
    assert bool(((a - b).abs() <= rtol * b.abs()).all()), float(((a - b).abs() / b.abs().clamp_min(1e-300)).max())


# ------------------------------------------------------------------------------------------------------------------- dlogistic
@pytest.fixture(scope="module")
def dll_cases():
    return {s: R.dll_inputs(*s, seed=sum(s)) for s in R.DLL_SHAPES}


@pytest.mark.parametrize("shape", R.DLL_SHAPES)
def test_dll_restatement_is_the_oracle(dll_cases, shape):
    images6, out6, _ = dll_cases[shape]
    for net in (0, 1):
        x, o = images6[..., 3 * net:3 * net + 3].double(), out6[net].double().requires_grad_(True)
        want = torch_ref.discretised_logistic_loss(x, o[..., :3], o[..., 3:])
        gw, = torch.autograd.grad(want.sum(), o)
        r = R.dll_ref(images6, 3 * net, out6[net], grad_scale=1.0 / 3)
        # (torch_ref's softplus returns its argument above 20: exp(-20) = 2.1e-9 of a saturated pixel's term, and of the sigmoid in its gradient, is missing there, twice in the density branch)
        s = torch.exp(-o[..., 3:].detach()).repeat(1, 1, 1, 2) * (1.0 + 200.0 * torch.cat([torch.zeros_like(x), torch.ones_like(x)], dim=-1))
        assert bool(((r["terms"] - want.detach()).abs() <= 1e-12 * want.detach().abs() + 4.4e-9).all())
        assert bool(((r["g"] - gw * R.f32(1.0 / 3)).abs() <= 1e-12 * gw.abs() + 4.4e-9 * s).all())
        wn = np_ref.discretised_logistic_loss(x.numpy(), out6[net][..., :3].double().numpy(), out6[net][..., 3:].double().numpy())
        assert np.allclose(r["terms"].numpy(), wn, rtol=1e-9, atol=1e-10)                 # (its sigmoid goes through tanh: 1e-16 of a delta down to 1e-5)
        for k in ("nll", "g", "g_scale", "g_floor", "nll_sumabs"):
            assert bool(torch.isfinite(r[k]).all()), k
        # the scale is the largest |addend|: never below the result it belongs to (up to the rounding of a sum of three addends)
        assert bool((r["g"].abs() <= 3.0 * r["g_scale"] * (1 + 1e-9)).all())


@pytest.mark.parametrize("m,ls", R.SUMS_TO_ONE)
def test_dll_bins_sum_to_one(m, ls):
    x6, out6 = R.sums_to_one_inputs(m, ls)
    nll = R.dll_ref(x6, 0, out6, want_grad=False)["nll"]
    # (not 1e-12: the model's own bins do not tile exactly -- fp32 levels x +- 1 / 255 leave 1e-8 gaps, and a bin below 1e-5 is the density times the width)
    assert abs(float(torch.exp(-nll).sum()) - 1.0) < 1e-5


@pytest.mark.parametrize("shape", R.DLL_SHAPES)
def test_dll_generator_conditions(dll_cases, shape):
    """the share of each branch per family, nothing in the threshold band, and the kinds of wave the wave-uniform shortcuts of dll_elem distinguish"""
    images6, out6, fam = dll_cases[shape]
    B, H, W = shape
    HW = H * W
    for k in range(len(R.FAMILIES)):
        assert (fam == k).any(), ("every family tiles every image", R.FAMILIES[k])
    waves = R.dll_waves(HW)
    assert waves.max() + 1 == R.dll_parts(HW) * (((HW + R.dll_parts(HW) - 1) // R.dll_parts(HW) + 63) // 64)
    kinds = dict(no_lo=0, no_hi=0, small_d=0, mixed=0, big_d=0)
    for net in (0, 1):
        x, m, ls = images6[..., 3 * net:3 * net + 3].reshape(B, HW, 3), out6[net][..., :3].reshape(B, HW, 3), out6[net][..., 3:].reshape(B, HW, 3)
        delta, lo, hi = R.dll_delta(x, m, ls)
        open_ = ~lo & ~hi
        assert int((open_ & ((delta / R.DLL_THRESHOLD - 1.0).abs() < R.DLL_BAND)).sum()) == 0
        rare = open_ & ~(delta > R.DLL_THRESHOLD)
        share = {}
        for k, name in enumerate(R.FAMILIES):
            sel = torch.from_numpy(fam == k)
            n_open = int(open_[:, sel].sum())
            share[name] = float(rare[:, sel].sum()) / max(n_open, 1)
            if name.startswith("sat"):
                assert n_open == 0
                mm, xx = m[:, sel], x[:, sel]
                assert bool((mm < xx).any()) and bool((mm > xx).any())                 # m on both sides
        print(shape, net, {k: round(v, 3) for k, v in share.items()})
        assert share["near"] < 0.2 and share["calm"] < 0.2 and share["far"] > 0.9 and 0.1 < share["wide"] < 0.9
        r = (x - m).abs().double() * torch.exp(-ls.double())
        far = torch.from_numpy(fam == R.FAMILIES.index("far"))
        assert float(r[:, far].min()) > 14.9 and float(r[:, far].max()) < 200.1
        d32 = (torch.exp(-ls) * np.float32(2.0 / 255.0))
        for w in range(int(waves.max()) + 1):
            sel = torch.from_numpy(waves == w)
            for c in range(3):
                l, h, sd = lo[:, sel, c].any(dim=1), hi[:, sel, c].any(dim=1), (d32[:, sel, c] < 0.25).all(dim=1)
                kinds["no_lo"] += int((~l).sum()); kinds["no_hi"] += int((~h).sum()); kinds["small_d"] += int(sd.sum())
                kinds["mixed"] += int((l & h).sum()); kinds["big_d"] += int((~sd).sum())
    print(shape, kinds)
    assert kinds["mixed"] > 0 and kinds["big_d"] > 0
    if waves.max() + 1 >= 8:                                        # an image of one wave holds all six families in it: it is a mixed wave and nothing else
        assert min(kinds.values()) > 0, kinds


# ------------------------------------------------------------------------------------------------------------------- reparam / KL
@pytest.mark.parametrize("B,L", R.REPARAM_SHAPES)
def test_reparam_restatement(B, L):
    pre, bias, eps, dz, dz2 = R.reparam_inputs(B, L, B + L)
    r = R.reparam_fwd_ref(pre, bias, eps)
    mu = pre[:, :L].double() + bias[:L].double()
    sg = torch.nn.functional.softplus(pre[:, L:].double() + bias[L:].double(), threshold=1e9)
    kl = -0.5 * torch.sum(1 + torch.log(sg ** 2) - mu ** 2 - torch.exp(torch.log(sg ** 2)), dim=1)           # the formula of test_reparam_kl_fwd_bwd
    rel_close(r["z_mean"], mu); rel_close(r["z_sig"], sg); rel_close(r["kl"], kl, 1e-10)
    assert abs(float(torch_ref.kl_divergence(mu, sg)) - float(r["kl"].mean())) <= 1e-10 * abs(float(r["kl"].mean()))
    for k, v in enumerate(R.PINS[:B]):
        assert bool(((pre[k, L:].double() + bias[L:].double()) - v).abs().max() < 1e-5)
    g, scale = R.reparam_bwd_ref(dz, dz2, pre, bias, eps, R.f32(40.0 / B))
    assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(scale).all()) and bool((g.abs() <= 4 * scale).all())
    assert bool(torch.isfinite(R.kl_sum_term(L, r["kl_sumabs"])).all())


def test_kl_closed_forms():
    L = 16
    pre = torch.zeros(2, 2 * L, dtype=F64)
    pre[:, L:] = math.log(math.e - 1)
    pre[1, :L] = 0.5
    r = R.reparam_fwd_ref(pre, torch.zeros(2 * L, dtype=F64), torch.zeros(2, L, dtype=F64))
    assert abs(float(r["kl"][0])) < 1e-12 and abs(float(r["kl"][1]) - 0.5 * L * 0.25) < 1e-12


def test_box_muller_mirror_moments_and_stream():
    e0 = R.reparam_eps(512, 128, 11, 3).double()
    assert abs(float(e0.mean())) < 0.02 and abs(float(e0.std()) - 1.0) < 0.02 and abs(float((e0 ** 4).mean()) - 3.0) < 0.15
    e1 = R.reparam_eps(512, 128, 11, 3, stream_id=1)
    assert not torch.equal(e0, e1) and torch.equal(R.reparam_eps(512, 128, 11, 3, stream_id=0), R.head_eps(512, 128, 11, 3))
    assert torch.equal(R.reparam_eps(64, 128, 11, 3, sample_offset=128), e0[128:192])
    big = (1 << 32) + 5
    assert torch.equal(R.reparam_eps(4, 8, 11, 3, sample_offset=big + 2), R.reparam_eps(6, 8, 11, 3, sample_offset=big)[2:])
    assert not torch.equal(R.reparam_eps(4, 8, 11, 3, sample_offset=big), R.reparam_eps(4, 8, 11, 3, sample_offset=5))       # the high word is part of the counter


# ------------------------------------------------------------------------------------------------------------------- random_perm
@pytest.mark.parametrize("n", R.PERM_N)
def test_perm_mirror_is_a_permutation_and_shard_invariant(n):
    seed, step, off = 0xF234567890ABCDEF, (3 << 32) | 5, (1 << 32) + 5
    p = R.random_perm(3, n, seed, step, off)
    assert p.dtype == np.int32 and p.shape == (3, n)
    for row in p:
        assert np.array_equal(np.sort(row), np.arange(n))
    assert np.array_equal(R.random_perm(2, n, seed, step, off + 1), p[1:])
    if n > 2:
        assert not np.array_equal(R.random_perm(3, n, seed, step + 1, off), p) and not np.array_equal(R.random_perm(3, n, seed + 1, step, off), p)
        assert not np.array_equal(R.random_perm(3, n, seed, step, 5), p)


# ------------------------------------------------------------------------------------------------------------------- scramble
def test_scramble_oracles_agree():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((3, 8, 8, 3)).astype(np.float32)
    perm = R.random_perm(3, 16, 1, 2, 3)
    assert np.array_equal(np_ref.scramble_batch(x, perm, 2), torch_ref.scramble_batch(x, perm, 2).numpy())


# ------------------------------------------------------------------------------------------------------------------- Adam
@pytest.mark.parametrize("t", [1, 2, 1000])
def test_adam_restatement_is_keras_adam(t):
    p, m, v, grads = R.adam_inputs(1027, 7)
    # with constants that fp32 holds exactly the two must agree to rounding; the oracle takes them unrounded, so give it the rounded ones
    kw = dict(lr=R.f32(1e-4), beta1=R.f32(0.9), beta2=R.f32(0.999), eps=R.f32(1e-7))
    rp, rm, rv = [p.double().clone()], [m.double().clone()], [v.double().clone()]
    torch_ref.keras_adam_(rp, [grads[0].double()], rm, rv, t, **kw)
    (p1, m1, v1), scales = R.adam_ref(p, grads[0], m, v, t)
    # omb = 1.f - beta in fp32 differs from 1 - f32(beta) by one rounding (6e-8 relative): the restatement follows the kernel, the oracle Keras
    tol = 2e-7
    assert bool(((m1 - rm[0]).abs() <= tol * scales[1]).all()) and bool(((v1 - rv[0]).abs() <= tol * scales[2]).all())
    assert bool(((p1 - rp[0]).abs() <= 4e-7 * scales[0]).all())
    alpha = kw["lr"] * math.sqrt(1 - kw["beta2"] ** t) / (1 - kw["beta1"] ** t)
    assert abs(R.adam_alpha(1e-4, 0.9, 0.999, t) - alpha) <= 2.0 ** -24 * alpha
    # the generator: zeros, sqrt(v) << eps, a live state
    assert all(bool((g == 0).any()) for g in grads) and bool((v.sqrt() < 1e-9).any()) and bool((v > 0).all()) and bool((m != 0).all())
    assert float(min(g[g != 0].abs().min() for g in grads)) >= 0.99e-12


def test_adam_first_step_closed_form():
    g = torch.tensor([1., -1., 5., -5., 1e-2, -1e-2, 3., -3.])
    z = torch.zeros(8)
    (p1, _, _), _ = R.adam_ref(z, g, z, z, 1)
    assert bool(((p1 + R.f32(1e-4) * torch.sign(g).double()).abs() < 1e-4 * 1e-3).all())


def test_clip_generator_and_factor():
    p, m, v, g, off = R.clip_inputs(3)
    assert off[-1] == sum(R.CLIP_TABLE) and [b - a for a, b in zip(off[:-1], off[1:])] == list(R.CLIP_TABLE)
    assert any(o % 4 for o in off[1:-1]) and 0 in R.CLIP_TABLE and sum(n > 262144 for n in R.CLIP_TABLE) == 2
    sc, norms = R.clip_factor(g, off, R.CLIPNORM)
    assert norms[0] > 2 and norms[2] < 0.5 and 0 < norms[1] - 1 < 1e-3 and 0 < 1 - norms[4] < 1e-3 and norms[3] == 0
    assert abs(float(sc[0]) - 1 / norms[0]) < 1e-12 and float(sc[off[2]]) == 1.0 and float(sc[off[4]]) == 1.0
    sc_inf, _ = R.clip_factor(g, off, 1e38, 0.5)
    assert bool((sc_inf == 0.5).all())
    assert R.clip_norm_rtol(524291) < 2e-5


# ------------------------------------------------------------------------------------------------------------------- resize
@pytest.mark.parametrize("shape", R.UPS_F32[:5] + R.UPS_BF16)
def test_resize_restatement_is_the_oracle(shape):
    x, g_hi, mask = R.ups_inputs(shape, sum(shape))
    up, scale = R.upsample_ref(x)
    rel_close(up, torch_ref.resize_bilinear_2x(x.double()), 1e-12)
    assert np.allclose(up.numpy(), np_ref.resize_bilinear_2x(x.double().numpy()), rtol=1e-12, atol=1e-15)
    xr = x.double().clone().requires_grad_(True)
    torch_ref.resize_bilinear_2x(xr).backward(g_hi.double())
    gl, gscale = R.upsample_bwd_ref(g_hi)
    assert bool(((gl - xr.grad).abs() <= 1e-12 * gscale).all())
    glm, sm = R.upsample_bwd_ref(g_hi, mask)
    assert torch.equal(glm, gl * (mask.double() > 0)) and bool((sm[mask <= 0] == 0).all())
    assert bool((up.abs() <= 4 * scale).all()) and bool((gl.abs() <= 16 * gscale).all())
    # <fwd(x), g> == <x, bwd(g)>
    a, b = float((up * g_hi.double()).sum()), float((x.double() * gl).sum())
    assert abs(a - b) <= 1e-12 * float((up * g_hi.double()).abs().sum())
    # the mask generator holds all four kinds
    assert mask.numel() < 16 or bool((mask > 0).any()) and bool((mask < 0).any()) and bool(((mask == 0) & ~torch.signbit(mask)).any()) and bool(((mask == 0) & torch.signbit(mask)).any())


def test_resize_stencil_closed_form():
    v = torch.arange(8, dtype=F64) ** 2
    up = R.upsample_ref(v[None, :, None, None].expand(1, 8, 3, 4))[0][0, :, 0, 0]
    want = torch.tensor([0, .25, .75, 1.75, 3.25, 5.25, 7.75, 10.75, 14.25, 18.25, 22.75, 27.75, 33.25, 39.25, 45.75, 49.0], dtype=F64)
    assert torch.equal(up, want)


@pytest.mark.parametrize("shape", R.UPS_BF16)
def test_resize_bf16_inputs_are_settled(shape):
    x, g_hi, mask = R.ups_inputs(shape, sum(shape), bf16=True)
    for t in (x, g_hi, mask):
        assert torch.equal(t, R.as_bf16(t))
    for ref, scale in (R.upsample_ref(x), R.upsample_bwd_ref(g_hi)):
        d = R.tie_distance(ref)
        assert bool(((d > R.TIE_BAND * scale) | (d == 0) | (ref == 0)).all())
        assert bool((ref * 8192.0 == torch.round(ref * 8192.0)).all()) and float(ref.abs().max()) < 64.0          # multiples of 2^-13 below 2^6: exact in fp32
        assert int((d == 0).sum()) > 0                              # exact ties are there and count


# ------------------------------------------------------------------------------------------------------------------- finaliser
@pytest.mark.parametrize("B", R.FINALIZE_B)
def test_finalize_restatement(B):
    nx, nh, kx, kh = R.finalize_inputs(B, B)
    losses, scale = R.finalize_ref(nx, nh, kx, kh, 40.0)
    want = [nx.double().mean(), kx.double().mean(), nh.double().mean(), kh.double().mean()]
    want += [40.0 * (want[1] + want[3])]
    want += [want[0] + want[2] + want[4]]
    rel_close(losses, torch.stack(want), 1e-13)
    one, _ = R.finalize_ref(nx, None, None, None, 40.0)
    assert float(one[1]) == 0 and float(one[2]) == 0 and float(one[3]) == 0 and float(one[4]) == 0 and float(one[5]) == float(one[0])
    assert bool(torch.isfinite(scale).all()) and bool(torch.isfinite(R.finalize_sum_term(B, (nx, kx, nh, kh), 40.0)).all())
    part = np.arange(12, dtype=np.float32).reshape(3, 4)
    assert np.array_equal(R.rowsum_ref32(part), part.sum(axis=1))


# ------------------------------------------------------------------------------------------------------------------- argument checks (no launch)
def test_pointwise_entry_points_refuse_before_launching(lib_built):
    from split_vae_amd import _lib
    lib = _lib.load()
    BAD, UNS = _lib.STATUS_BADARG, _lib.STATUS_UNSUPPORTED
    buf = (C.c_float * 64)()                                        # host memory: never dereferenced, every call below answers before it launches
    a = (C.addressof(buf) + 15) // 16 * 16
    assert lib.sv_random_perm(a, 1, 4097, 0, 0, 0, None) == UNS
    assert lib.sv_random_perm(a, 0, 16, 0, 0, 0, None) == BAD and lib.sv_random_perm(a, 1, 0, 0, 0, 0, None) == BAD
    assert lib.sv_adam_step(a + 4, a, a, a, 16, 1e-4, .9, .999, 1e-7, 1, 1.0, None) == BAD        # a pointer one float off the 16-byte boundary
    assert lib.sv_adam_step(a, a, a, a + 4, 16, 1e-4, .9, .999, 1e-7, 1, 1.0, None) == BAD
    assert lib.sv_adam_step(a, a, a, a, 0, 1e-4, .9, .999, 1e-7, 1, 1.0, None) == BAD
    assert lib.sv_adam_step(a, a, a, a, 16, 1e-4, .9, .999, 1e-7, 0, 1.0, None) == BAD
    for dt, c in ((_lib.SV_F32, 6), (_lib.SV_BF16, 12)):
        assert lib.sv_upsample2x_fwd(a, a, dt, 1, 2, 2, c, None) == UNS
        assert lib.sv_upsample2x_bwd(a, None, a, dt, 1, 2, 2, c, None) == UNS
    assert lib.sv_upsample2x_fwd(a, a, 7, 1, 2, 2, 8, None) == BAD
    assert lib.sv_scramble_gather(a, a, a, 1, 8, 8, 3, None) == UNS and lib.sv_scramble_gather(a, a, a, 1, 8, 4, 2, None) == UNS
    for dt in (_lib.SV_F32, _lib.SV_BF16):                          # x8 / xh8 are stored as uint4: a pointer off the 16-byte boundary is refused
        assert lib.sv_scramble_gather_staged(a, a, a, a + 4, a, dt, 1, 8, 8, 4, None) == BAD and lib.sv_scramble_gather_staged(a, a, a, a, a + 8, dt, 1, 8, 8, 4, None) == BAD
    assert lib.sv_dlogistic_nll(a, 1, a, a, None, 0, 1.0, 1, 8, 8, a, None) == BAD
    # sv_dlogistic_nll_twin(images6, out6, zs_out, nll, zs_nll, grad, zs_grad, grad_dtype, grad_scale, B, H, W, partial_ws, zs_part, stream)
    ok = dict(images6=a, out6=a, zs_out=2 * 64 * 6, nll=a, zs_nll=2, grad=a, zs_grad=2 * 64 * 8, dt=_lib.SV_F32, B=2, H=8, W=8, ws=a, zs_part=2)

    def twin(**kw):
        q = dict(ok, **kw)
        return lib.sv_dlogistic_nll_twin(q["images6"], q["out6"], q["zs_out"], q["nll"], q["zs_nll"], q["grad"], q["zs_grad"], q["dt"], 1.0, q["B"], q["H"], q["W"],
                                         q["ws"], q["zs_part"], None)
    for kw in (dict(images6=None), dict(out6=None), dict(nll=None), dict(ws=None), dict(B=0), dict(H=0), dict(W=-1), dict(zs_out=2 * 64 * 6 - 2), dict(zs_out=2 * 64 * 6 + 1),
               dict(zs_nll=1), dict(zs_part=1), dict(zs_grad=2 * 64 * 8 - 4), dict(zs_grad=2 * 64 * 8 + 2), dict(dt=7), dict(grad=a + 4), dict(out6=a + 4),
               dict(dt=_lib.SV_BF16, zs_grad=2 * 64 * 8 + 4)):
        assert twin(**kw) == BAD, kw
    # sv_finalize_losses(nll_x, nll_xh, kl_x, kl_xh, part_x, part_xh, P, B, beta, losses, metric_acc, accumulate, stream)
    fin = lib.sv_finalize_losses
    assert fin(None, a, a, a, None, None, 0, 4, 1.0, a, a, 0, None) == BAD
    assert fin(a, a, a, a, None, None, 0, 4, 1.0, None, a, 0, None) == BAD
    assert fin(a, a, a, a, None, None, 0, 0, 1.0, a, a, 0, None) == BAD
    assert fin(a, a, a, a, None, None, 0, 4, 1.0, a, None, 1, None) == BAD             # accumulate without metric_acc
    assert fin(a, a, a, a, None, a, 4, 4, 1.0, a, a, 0, None) == BAD                   # part_xh without part_x
    assert fin(a, a, a, a, a, a, 0, 4, 1.0, a, a, 0, None) == BAD                      # partials without P
    assert fin(a, a, a, a, a, None, 4, 4, 1.0, a, a, 0, None) == BAD                   # nll_xh but no part_xh
    assert fin(a, None, a, a, a, a, 4, 4, 1.0, a, a, 0, None) == BAD                   # part_xh but no nll_xh
