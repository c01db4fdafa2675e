"""GPU tests of the per-dimension latent report: sv_latent_dims_prepare / _lse / _finish (csrc/latent_dims.hip) through their entry
points against the float64 twin of tests/latent_dims_ref.py, element by element inside the bound derived there; the extents written,
bit-reproducibility, the refusals, the estimator's identity against sv_latent_info_finish, split_vae_amd/latent_dims.py on the three
models and the flag's surface in main.py / evaluate.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import latent_dims_ref as ref
import latent_info_ref as iref

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
SENTINEL = -12345.678
WORST = {"lse": 0.0, "prepare": 0.0, "model": 0.0}        # worst device error / bound seen by this run (printed per test)


@pytest.fixture(scope="module")
def env(lib_built):
    assert torch.cuda.is_available()
    from split_vae_amd import _lib, latent_dims, ops
    return ops, latent_dims, _lib


def _dev(a, pad=0, off=0):
    """rows of `a` on the device, with `off` unused floats before and `pad` behind every row (a row pitch above the width; off not
    a multiple of 4: a base that is not 16-byte aligned)"""
    a = np.ascontiguousarray(a, np.float32)
    if not pad and not off:
        return torch.from_numpy(a).cuda()
    t = torch.full((a.shape[0], off + a.shape[1] + pad), 1e30, dtype=F32, device="cuda")  # the padding must never be read
    t[:, off:off + a.shape[1]] = torch.from_numpy(a).cuda()
    return t[:, off:off + a.shape[1]]


def _case(Nq, Nr, L, seed):
    c = iref.make_case(Nq, Nr, L, 0, seed=seed)
    c["lc"] = ref.prepare(c["mu"], c["sig"], np.zeros_like(c["mu"]))["lc"]
    return c


def _lse(ops, c, pad=0, off=0, poison=True):
    """sv_latent_dims_lse on a case -> lse [Nq,L] fp64 (NumPy); NaN-filled workspace, sentinel-filled output with guard bands and a
    row pitch of its own: nothing outside the stated extent is written, every stated element is."""
    Nq, L = c["z"].shape
    Nr = c["mu"].shape[0]
    G, ldl = 64, L + pad
    flat = torch.full((Nq * ldl + 2 * G,), SENTINEL, dtype=F64, device="cuda")
    out = flat[G:G + Nq * ldl].view(Nq, ldl)[:, :L]
    nbytes = ops.latent_dims_workspace_bytes(Nq, Nr, L)
    ws = torch.full((nbytes + 256,), 0xFF, dtype=torch.uint8, device="cuda")              # all-ones words: NaN
    ops.latent_dims_lse(_dev(c["z"], pad, off), _dev(c["mu"], pad, off), _dev(c["rsig"], pad, off), _dev(c["lc"], pad, off), lse=out,
                        workspace=ws[:nbytes] if poison else None)
    torch.cuda.synchronize()
    assert (flat[:G] == SENTINEL).all() and (flat[G + Nq * ldl:] == SENTINEL).all() and (ws[nbytes:] == 0xFF).all()
    if pad:
        assert (flat[G:G + Nq * ldl].view(Nq, ldl)[:, L:] == SENTINEL).all()
    got = out.cpu().numpy()
    assert (got != SENTINEL).all() and np.isfinite(got).all()
    return got


def _check(ops, c, pad=0, off=0):
    chunk = ops.latent_dims_chunk_rows()
    tw = ref.lse(c["z"], c["mu"], c["rsig"], c["lc"], chunk, device="cuda")
    got = _lse(ops, c, pad, off)
    err = np.abs(got - tw["lse"])
    ratio = err / tw["bound"]
    WORST["lse"] = max(WORST["lse"], float(ratio.max()))
    print("worst error / bound %.3g (error %.3g, bound %.3g); so far %.3g" % (ratio.max(), err.max(), tw["bound"].max(), WORST["lse"]))
    assert (ratio <= 1.0).all()
    return got, tw


# ---------------------------------------------------------------- 1. sv_latent_dims_lse against the twin
# one sweep per axis around the base case (Nq 65, Nr 2 chunks + 7, L 37): Nr as a multiple m of the chunk plus a remainder
BASE = dict(Nq=65, Nr=(2, 7), L=37, pad=0, off=0)
SWEEP = ([dict()] + [dict(Nq=v) for v in (1, 63, 64, 130)] + [dict(Nr=v) for v in ((0, 1), (1, -1), (1, 0), (1, 1))] +
         [dict(L=v) for v in (1, 3, 63, 64, 65, 128, 256, 512)] + [dict(pad=1), dict(pad=3), dict(pad=4, L=36), dict(pad=3, off=1, L=36)])


@pytest.mark.parametrize("case", SWEEP, ids=lambda c: "-".join("%s%s" % (k, v) for k, v in c.items()).replace(" ", "") or "base")
def test_lse_matches_the_twin_inside_the_bound(env, case):
    """sig log-uniform in [1e-2, 1]; every query has one dominant reference, a few comparable ones and a far-away tail
    (latent_info_ref.make_case).  |device - twin| <= bound for every element."""
    ops, _, _ = env
    p = dict(BASE, **case)
    chunk = ops.latent_dims_chunk_rows()
    Nr = p["Nr"][0] * chunk + p["Nr"][1]
    _check(ops, _case(p["Nq"], Nr, p["L"], seed=7), p["pad"], p["off"])


def test_all_references_equal(env):
    """Nr copies of one posterior: lse equals the single-reference score, the own-form lc - 1/2 ((z - mu) rsig)^2, within the bound."""
    ops, _, _ = env
    c = _case(33, 1, 37, seed=11)
    many = dict(c, **{k: np.repeat(c[k], 200, axis=0) for k in ("mu", "sig", "rsig", "lc")})
    got, tw = _check(ops, many)
    w = (c["z"].astype(np.float64) - c["mu"][0]) * c["rsig"][0].astype(np.float64)
    assert (np.abs(got - (c["lc"][0].astype(np.float64) - 0.5 * w * w)) <= tw["bound"]).all()


def test_a_far_away_tail_flushes_to_zero(env):
    """One reference at the query, more than a chunk of references 1e3 standard deviations away: their terms underflow."""
    ops, _, _ = env
    chunk = ops.latent_dims_chunk_rows()
    c = _case(5, chunk + 1, 12, seed=13)
    c["mu"][:] = 50.0
    c["sig"][:] = 0.05
    c["mu"][3] = 0.0
    c["z"] = (0.01 * np.arange(5 * 12).reshape(5, 12)).astype(np.float32)
    c["rsig"] = iref.draw(c["mu"], c["sig"], np.zeros_like(c["mu"]), 12)["rsig"]
    c["lc"] = ref.prepare(c["mu"], c["sig"], np.zeros_like(c["mu"]))["lc"]
    got, _ = _check(ops, c)
    e3 = c["lc"][3].astype(np.float64) - 0.5 * (c["z"].astype(np.float64) * c["rsig"][3]) ** 2
    assert np.allclose(got, e3 - np.log(chunk + 1), rtol=0, atol=1e-3)


# ---------------------------------------------------------------- 2. the same bits
def test_bit_identical_on_a_repeat_and_at_other_positions(env):
    ops, _, _ = env
    chunk = ops.latent_dims_chunk_rows()
    c = _case(130, chunk + 9, 70, seed=14)
    a = _lse(ops, c)
    assert np.array_equal(a, _lse(ops, c)) and np.array_equal(a, _lse(ops, c, poison=False))
    rng = np.random.default_rng(0)
    perm = rng.permutation(130)
    assert np.array_equal(_lse(ops, dict(c, z=c["z"][perm])), a[perm])                     # a permutation of the query rows
    assert np.array_equal(_lse(ops, dict(c, z=c["z"][37:101])), a[37:101])                 # a row slice
    cols = rng.permutation(70)
    sub = lambda idx: {k: c[k][:, idx] for k in ("z", "mu", "rsig", "lc")}                  # noqa: E731
    assert np.array_equal(_lse(ops, sub(cols)), a[:, cols])                                # a permutation of the columns
    assert np.array_equal(_lse(ops, sub(slice(5, 40))), a[:, 5:40])                        # a column slice
    assert np.array_equal(_lse(ops, c, pad=5), a) and np.array_equal(_lse(ops, c, pad=2, off=3), a)   # pitch and base alignment


# ---------------------------------------------------------------- 3. refusals leave the outputs alone
def test_refusals_return_their_status_and_write_nothing(env):
    ops, _, _lib = env
    lib = _lib.load()
    c = _case(9, 40, 24, seed=15)
    z, mu, rs, lc = _dev(c["z"]), _dev(c["mu"]), _dev(c["rsig"]), _dev(c["lc"])
    out = torch.full((9, 24), SENTINEL, dtype=F64, device="cuda")
    ws = torch.zeros((ops.latent_dims_workspace_bytes(9, 40, 24),), dtype=torch.uint8, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(z_=None, ldz=24, ldl=24, Nq=9, Nr=40, L=24, ws_bytes=None, lse=None, wsp=None):
        p = lambda t: C.c_void_p(t.data_ptr())                                            # noqa: E731
        return lib.sv_latent_dims_lse(C.c_void_p(z.data_ptr() + 2) if z_ == "misaligned" else None if z_ == "null" else p(z), ldz, p(mu), 24,
                                      p(rs), 24, p(lc), 24, Nq, Nr, L, C.c_void_p(out.data_ptr() + 4) if lse == "misaligned" else p(out), ldl,
                                      C.c_void_p(ws.data_ptr() + 8) if wsp == "misaligned" else p(ws),
                                      ws.numel() if ws_bytes is None else ws_bytes, st)
    U, B, W = _lib.STATUS_UNSUPPORTED, _lib.STATUS_BADARG, _lib.STATUS_WORKSPACE
    for want, kw in ((U, dict(L=0)), (U, dict(L=513)), (U, dict(Nq=0)), (U, dict(Nr=0)), (U, dict(ldz=23)), (U, dict(ldl=23)),
                     (B, dict(z_="null")), (B, dict(z_="misaligned")), (B, dict(lse="misaligned")), (B, dict(wsp="misaligned")),
                     (W, dict(ws_bytes=ws.numel() - 1)), (W, dict(ws_bytes=0))):
        assert call(**kw) == want, kw
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()
    with pytest.raises(_lib.SplitVaeError, match="SV_E_WORKSPACE"):
        ops.latent_dims_lse(z, mu, rs, lc, lse=out, workspace=ws[:-1])
    for bad in (lambda: ops.latent_dims_lse(z.double(), mu, rs, lc), lambda: ops.latent_dims_lse(z.cpu(), mu, rs, lc),
                lambda: ops.latent_dims_lse(z, mu[:, :20], rs, lc), lambda: ops.latent_dims_lse(z, mu, rs, lc[:8]),
                lambda: ops.latent_dims_lse(z, mu, rs, lc, lse=out.float()),
                lambda: ops.latent_dims_finish(out, out, z, out[:, 0]),                    # lse_block must be dense
                lambda: ops.latent_dims_prepare(mu, rs, out=(lc, out.float(), out[:3]))):
        with pytest.raises(ValueError):
            bad()
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()
    assert call() == 0                                            # and the accepted call writes all of it
    torch.cuda.synchronize()
    assert (out != SENTINEL).all()


# ---------------------------------------------------------------- 4. sv_latent_dims_prepare and sv_latent_dims_finish
@pytest.mark.parametrize("N,L,pad,off", [(70, 37, 0, 0), (5, 1, 3, 0), (300, 128, 0, 0), (257, 512, 1, 2)])
def test_prepare_with_pinned_eps_matches_the_twin(env, N, L, pad, off):
    """lc inside the error of logf (3 ulp) and its one rounding; own from the device's lc and the columns (mean, population variance,
    closed-form KL) at rtol 1e-12 of the fp64 sums; the padding behind the rows is neither read nor written."""
    ops, _, _ = env
    mu, sig = iref.make_refs(N, L, 0, seed=21)
    eps = np.random.default_rng(22).standard_normal((N, L)).astype(np.float32)
    lcfull = torch.full((N, off + L + pad), SENTINEL, dtype=F32, device="cuda")
    own = torch.full((N + 2, L), SENTINEL, dtype=F64, device="cuda")
    cols = torch.full((5, L), SENTINEL, dtype=F64, device="cuda")
    lc = lcfull[:, off:off + L]
    ops.latent_dims_prepare(_dev(mu, pad, off), _dev(sig, pad, off), eps=_dev(eps, pad, off), out=(lc, own[1:N + 1], cols[1:4]))
    torch.cuda.synchronize()
    assert (lcfull[:, :off] == SENTINEL).all() and (lcfull[:, off + L:] == SENTINEL).all()
    assert (own[0] == SENTINEL).all() and (own[N + 1] == SENTINEL).all() and (cols[0] == SENTINEL).all() and (cols[4] == SENTINEL).all()
    lcd = lc.cpu().numpy()
    p = ref.prepare(mu, sig, eps, lc=lcd)
    ratio = np.abs(lcd.astype(np.float64) - p["lc"].astype(np.float64)) / p["lcerr"]
    WORST["prepare"] = max(WORST["prepare"], float(ratio.max()))
    print("prepare: lc worst error / bound %.3g" % ratio.max())
    assert (ratio <= 1.0).all()
    assert np.allclose(own[1:N + 1].cpu().numpy(), p["own"], rtol=1e-12, atol=1e-12)
    got = cols[1:4].cpu().numpy()
    for k, name in enumerate(("mean", "var", "kl")):
        scale = {"mean": np.abs(mu.astype(np.float64)).mean(0), "var": p["var"], "kl": np.abs(p["kl"]) + np.abs(np.log(sig.astype(np.float64))).mean(0)}[name]
        assert (np.abs(got[k] - p[name]) <= 1e-12 * scale + 1e-300).all(), name


def test_free_running_prepare_draws_the_numbers_of_latent_info_draw(env):
    """eps = NULL: own_ij = lc_ij - 1/2 eps_ij^2 with the eps sv_latent_info_draw used for z = mu + sig * eps, per block."""
    ops, _, _ = env
    mu, sig = (_dev(a) for a in iref.make_refs(70, 37, 19, seed=23))
    z = ops.latent_info_draw(mu, sig, 37, seed=5)[0]
    for e, (a, b) in enumerate(((0, 37), (37, 56))):
        lc, own, _ = ops.latent_dims_prepare(mu[:, a:b], sig[:, a:b], block=e, seed=5)
        eps2 = 2.0 * (lc.double() - own)
        want = ((z[:, a:b].double() - mu[:, a:b].double()) / sig[:, a:b].double()) ** 2
        assert torch.allclose(eps2, want, rtol=1e-3, atol=1e-4)                            # z carries two fp32 roundings at sig >= 1e-2
        other = ops.latent_dims_prepare(mu[:, a:b], sig[:, a:b], block=1 - e, seed=5)[1]
        assert not torch.allclose(other, own, rtol=1e-3, atol=1e-4)
        part = ops.latent_dims_prepare(mu[33:, a:b], sig[33:, a:b], block=e, seed=5, sample_offset=33)[1]
        assert torch.equal(part, own[33:])


def test_finish_is_the_twins_report(env):
    ops, _, _ = env
    rng = np.random.default_rng(31)
    for N, L, pad in ((1, 3, 0), (300, 37, 3), (257, 512, 0)):
        lse, own, blk = rng.standard_normal((N, L)) * 5, rng.standard_normal((N, L)) * 5, rng.standard_normal(N) * 50
        z = rng.standard_normal((N, L)).astype(np.float32)
        lsed = torch.full((N, L + pad), SENTINEL, dtype=F64, device="cuda")
        lsed[:, :L] = torch.from_numpy(lse).cuda()
        flat = torch.full((3 * L + 2 + 16,), SENTINEL, dtype=F64, device="cuda")
        args = (lsed[:, :L], torch.from_numpy(own).cuda(), _dev(z, pad), torch.from_numpy(blk).cuda())
        out = ops.latent_dims_finish(*args, out=flat[8:8 + 3 * L + 2])
        torch.cuda.synchronize()
        assert (flat[:8] == SENTINEL).all() and (flat[8 + 3 * L + 2:] == SENTINEL).all()
        f = ref.finish(lse, own, z, blk)
        got = out.cpu().numpy()
        scale = np.abs(lse).mean(0) + np.abs(own).mean(0) + 1.0 + 0.5 * (z.astype(np.float64) ** 2).mean(0)
        for k, name in enumerate(("mi", "dwkl", "mlse")):
            assert (np.abs(got[k * L:(k + 1) * L] - f[name]) <= 1e-12 * scale).all(), name
        assert abs(got[3 * L] - f["tc"]) <= 1e-12 * (np.abs(blk).mean() + scale.sum())
        assert abs(got[3 * L + 1] - f["dwkl_sum"]) <= 1e-12 * scale.sum()
        assert torch.equal(out, ops.latent_dims_finish(*args))


def _blocks(ops, mu, sig, eps, Lg):
    """the three --latent_info calls and, per block, the three calls of this report on the same draws"""
    Lc = mu.shape[1]
    z, rsig, cst, own_b, prior_b = ops.latent_info_draw(mu, sig, Lg, eps=eps)
    lse_b = ops.latent_info_lse(z, mu, rsig, cst, Lg)
    info = ops.latent_info_finish(own_b, prior_b, lse_b, Lc - Lg).cpu().numpy()
    outs = []
    for e, (a, b) in enumerate(((0, Lg), (Lg, Lc))):
        if a == b:
            continue
        lc, own, cols = ops.latent_dims_prepare(mu[:, a:b], sig[:, a:b], eps=eps[:, a:b], block=e)
        lse = ops.latent_dims_lse(z[:, a:b], mu[:, a:b], rsig[:, a:b], lc)
        outs.append(dict(out=ops.latent_dims_finish(lse, own, z[:, a:b], lse_b[e]).cpu().numpy(), lse=lse, lc=lc, z=z[:, a:b], rsig=rsig[:, a:b],
                         cst=cst[:, e], lse_block=lse_b[e]))
    return info, outs


def test_kl_is_mi_plus_tc_plus_dimension_wise_kl_on_the_device(env):
    """The estimator's identity against sv_latent_info_finish on the same draws, to 1e-9 absolute, for both blocks."""
    ops, _, _ = env
    mu, sig = iref.make_refs(70, 37, 19, seed=33)
    eps = np.random.default_rng(34).standard_normal((70, 56)).astype(np.float32)
    info, outs = _blocks(ops, _dev(mu), _dev(sig), _dev(eps), 37)
    for e, (L, o) in enumerate(zip((37, 19), outs)):
        kl, mi, tc, dwkl = info[3 * e], info[3 * e + 1], o["out"][3 * L], o["out"][3 * L + 1]
        print("block %d: KL %.12g = MI %.12g + TC %.12g + dwKL %.12g (difference %.3g)" % (e, kl, mi, tc, dwkl, kl - mi - tc - dwkl))
        assert abs(kl - (mi + tc + dwkl)) <= 1e-9


def test_a_block_of_one_dimension_has_no_total_correlation(env):
    """L = 1: the block's log-sum-exp and the dimension's are the same quantity from two kernels: TC is zero within the sum of their
    bounds (the row constant and lc are the same bits there)."""
    ops, _, _ = env
    chunk = ops.latent_dims_chunk_rows()
    mu, sig = iref.make_refs(70, 1, 0, seed=35)
    eps = np.random.default_rng(36).standard_normal((70, 1)).astype(np.float32)
    _, (o,) = _blocks(ops, _dev(mu), _dev(sig), _dev(eps), 1)
    assert torch.equal(o["cst"], o["lc"][:, 0])
    z, rsig, lc = (o[k].cpu().numpy() for k in ("z", "rsig", "lc"))
    tw = ref.lse(z, mu, rsig, lc, chunk, device="cuda")
    acc = ((z.astype(np.float64) - mu.T.astype(np.float64)) * rsig.T.astype(np.float64)) ** 2       # [Nq, Nr]: the block's pair scores ARE the dimension's
    bb = iref.lse_bound(dict(e=[lc.T.astype(np.float64) - 0.5 * acc], acc=[acc]), 1, 0)[0]
    tol = (tw["bound"][:, 0] + bb).mean()
    print("L = 1: TC %.3g, tolerance %.3g" % (o["out"][3], tol))
    assert abs(o["out"][3]) <= tol


# ---------------------------------------------------------------- 5. the three models
H, LAT, B, N = 32, 128, 16, 48


def _make(kind):
    from split_vae_amd.gm import LGGMVae
    from split_vae_amd.gmvae import GMVae
    from split_vae_amd.model import LGVae
    shape = (None, H, H, 3)
    if kind == "lgvae":
        return LGVae(LAT, LAT, image_shape=shape, dtype="f32", seed=3)
    if kind == "lggmvae":
        return LGGMVae(LAT, LAT, shape, 10, 0.4, dtype="f32", seed=3)
    return GMVae(LAT, shape, 10, 0.4, dtype="f32", seed=3)


@pytest.mark.parametrize("kind", ["lgvae", "lggmvae", "gmvae"])
def test_evaluate_equals_the_twin_on_the_devices_own_posteriors(env, deterministic, kind):
    """SVHN-32 shapes, 48 images in batches of 16, pinned eps: latent_dims.evaluate equals the twin fed the read-back mu, sig and eps,
    within the means of the per-element bounds; the figures a model has no right to are None; model._calls stays."""
    ops, latent_dims, _ = env
    from split_vae_amd import latent_info
    model = _make(kind)
    rng = np.random.default_rng(41)
    batches = [torch.from_numpy(rng.uniform(-1, 1, (B, H, H, 6)).astype(np.float32)).cuda() for _ in range(4)]
    model._calls = 5
    mu, sig, Lg, Ll = latent_info.posteriors(model, batches, N)
    eps = torch.from_numpy(rng.standard_normal((N, Lg + Ll)).astype(np.float32)).cuda()
    res = latent_dims.evaluate(model, batches, N, eps=eps)
    assert model._calls == 5 and res["n_images"] == N and res["log_n"] == pytest.approx(np.log(N), abs=1e-12)
    assert Lg == LAT and Ll == (0 if kind == "gmvae" else LAT)
    mun, sign, epsn = mu.cpu().numpy(), sig.cpu().numpy(), eps.cpu().numpy()
    d = iref.draw(mun, sign, epsn, Lg)
    btw = iref.lse(d["z"], mun, sign, d["c"], Lg)
    bbound = iref.lse_bound(btw, Lg, Ll, cerr=d["cerr"])
    chunk = ops.latent_dims_chunk_rows()
    for e, (s, a, b) in enumerate((("g", 0, Lg), ("l", Lg, Lg + Ll))):
        if a == b:
            assert all(res[k + "_l"] is None for k in latent_dims.BLOCK_KEYS)
            continue
        p = ref.prepare(mun[:, a:b], sign[:, a:b], epsn[:, a:b])
        tw = ref.lse(d["z"][:, a:b], mun[:, a:b], d["rsig"][:, a:b], p["lc"], chunk, device="cuda")
        f = ref.finish(tw["lse"], p["own"], d["z"][:, a:b], btw["lse"][e])
        shift = p["lcerr"].max(0)                                        # every lc within lcerr of the twin's: lse moves by at most its maximum
        tol_lse = tw["bound"].mean(0) + shift
        gaussian = s == "l" or kind == "lgvae"
        assert res["dims_" + s] == b - a and res["active_" + s] == int((p["var"] > ref.ACTIVE).sum())
        assert np.allclose(res["var_" + s], p["var"], rtol=1e-12, atol=0)
        checks = [("mi", f["mi"], tol_lse + p["lcerr"].mean(0) + 1e-12), ("tc", f["tc"], bbound[e].mean() + tol_lse.sum())]
        if gaussian:
            assert np.allclose(res["kl_" + s], p["kl"], rtol=1e-11, atol=1e-12)
            checks += [("dwkl", f["dwkl"], tol_lse + 1e-12), ("dwkl_sum", f["dwkl_sum"], tol_lse.sum())]
            assert res["block_kl_" + s] == pytest.approx(res["block_mi_" + s] + res["tc_" + s] + res["dwkl_sum_" + s], abs=1e-9)
        else:
            assert all(res[k + "_" + s] is None for k in ("kl", "dwkl", "dwkl_sum", "block_kl"))
        for name, want, tol in checks:
            ratio = float(np.max(np.abs(np.asarray(res[name + "_" + s]) - want) / tol))
            WORST["model"] = max(WORST["model"], ratio)
            print("%s z_%s %s: worst error / bound %.3g" % (kind, s, name, ratio))
            assert ratio <= 1.0, (s, name)
        assert max(res["mi_" + s]) <= np.log(N) + tol_lse.max() + p["lcerr"].max()              # the estimator saturates at log N
    free = latent_dims.evaluate(model, batches, N)
    assert free == latent_dims.evaluate(model, batches, N) and free["mi_g"] != res["mi_g"]
    assert latent_dims.report_line(res).startswith("Test latent dimensions (48 images, log N = 3.8712): z_g active ")


# ---------------------------------------------------------------- 6. CLI
def _lines(out):
    return [l for l in out.splitlines() if l.startswith("Test latent dimensions (")]


CLI = ["--synthetic", "-no_label", "--batch_size", "8", "--training_steps", "1", "--log_every", "1", "--dtype", "f32"]


def test_cli_prints_the_line_and_fills_the_history(env, tmp_path, monkeypatch, capsys):
    """--latent_dims 32 --synthetic (32 test images): one line behind each evaluation's report, after the --latent_info line; the
    history carries the per-dimension lists; evaluate reproduces the line from the saved weights and returns the lists."""
    _, latent_dims, _ = env
    from split_vae_amd import evaluate, main as svmain
    monkeypatch.chdir(tmp_path)
    seen = []
    orig = latent_dims.report
    monkeypatch.setattr(latent_dims, "report", lambda m, t, config, step=None: (orig(m, t, config, step), seen.append(config))[0])
    path = svmain.main(CLI + ["--latent_dims", "32", "--latent_info", "32"])
    out = capsys.readouterr().out
    lines = _lines(out)
    assert len(lines) == out.count("Training step ") >= 1 and "clipped" not in out and "Training done!" in out
    assert all(l.startswith("Test latent dimensions (32 images, log N = 3.4657): z_g active ") and "; z_l active " in l and
               l.count("TC ") == 2 and l.count("dimension-wise KL ") == 2 and l.count("largest KL_j ") == 2 for l in lines), out
    assert out.index("Test latent information (") < out.index("Test latent dimensions (")
    hist = seen[-1].latent_dims_history
    assert len(hist) == len(lines) and hist[-1]["n_images"] == 32
    L = hist[-1]["dims_g"]
    assert all(len(hist[-1][k + "_" + s]) == L for k in ("var", "kl", "mi", "dwkl") for s in "gl")
    res = evaluate.main(CLI + ["--latent_dims", "32", "--weights", path])
    again = capsys.readouterr().out
    assert _lines(again) == [lines[-1]] and "Test latent information" not in again
    assert res["latent_dims_n_images"] == 32 and np.allclose(res["latent_dims_var_g"], hist[-1]["var_g"], rtol=1e-3, atol=1e-9) and len(res["latent_dims_mi_l"]) == L
    evaluate.main(CLI + ["--latent_dims", "500", "--latent_info", "32", "--weights", path])
    out2 = capsys.readouterr().out
    assert out2.count("Note: --latent_dims 500 clipped to the test set's 32 images") == 1 and len(_lines(out2)) == 1


def test_cli_gmvae_reports_z_g_without_the_prior_figures(env, tmp_path, monkeypatch, capsys):
    from split_vae_amd import main as svmain
    monkeypatch.chdir(tmp_path)
    svmain.main(CLI + ["--model", "gmvae", "--y_size", "10", "--latent_dims", "32"])
    lines = _lines(capsys.readouterr().out)
    assert len(lines) >= 1
    assert all(l.startswith("Test latent dimensions (32 images, log N = 3.4657): z_g active ") and "z_l" not in l and "KL" not in l and
               ", TC " in l for l in lines), lines
