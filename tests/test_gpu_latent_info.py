"""GPU tests of the aggregate-posterior information report: sv_latent_info_draw / _lse / _finish (csrc/latent_info.hip) through their
entry points against the float64 twin of tests/latent_info_ref.py, element by element inside the bound derived there; the extents
written, bit-reproducibility, the refusals, split_vae_amd/latent_info.py on the three models and the flag's surface in main.py /
evaluate.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import latent_info_ref as ref

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
SENTINEL = -12345.678
WORST = {"lse": 0.0, "draw": 0.0, "model": 0.0}           # worst device error / bound seen by this run (printed per test)


@pytest.fixture(scope="module")
def env(lib_built):
    assert torch.cuda.is_available()
    from split_vae_amd import _lib, latent_info, ops
    return ops, latent_info, _lib


def _dev(a, pad=0):
    """rows of `a` on the device, with `pad` unused floats behind every row (a row pitch above the width)"""
    a = np.ascontiguousarray(a, np.float32)
    if not pad:
        return torch.from_numpy(a).cuda()
    t = torch.full((a.shape[0], a.shape[1] + pad), 1e30, dtype=F32, device="cuda")       # the padding must never be read
    t[:, :a.shape[1]] = torch.from_numpy(a).cuda()
    return t[:, :a.shape[1]]


def _lse(ops, c, pad=0, poison=True):
    """sv_latent_info_lse on a case of ref.make_case -> lse [3,Nq] fp64 (NumPy); NaN-filled workspace, sentinel-filled output with
    guard bands: nothing outside the stated extent is written, every stated element is."""
    Nq, Nr = c["z"].shape[0], c["mu"].shape[0]
    G = 64
    flat = torch.full((3 * Nq + 2 * G,), SENTINEL, dtype=F64, device="cuda")
    out = flat[G:G + 3 * Nq].view(3, Nq)
    nbytes = ops.latent_info_workspace_bytes(Nq, Nr)
    ws = torch.full((nbytes + 256,), 0xFF, dtype=torch.uint8, device="cuda")              # all-ones words: NaN
    ops.latent_info_lse(_dev(c["z"], pad), _dev(c["mu"], pad), _dev(c["rsig"], pad), torch.from_numpy(c["cst"]).cuda(), c["Lg"],
                        lse=out, workspace=ws[:nbytes] if poison else None)
    torch.cuda.synchronize()
    assert (flat[:G] == SENTINEL).all() and (flat[G + 3 * Nq:] == SENTINEL).all() and (ws[nbytes:] == 0xFF).all()
    got = out.cpu().numpy()
    rows = 3 if c["Ll"] else 1
    assert (got[:rows] != SENTINEL).all() and np.isfinite(got[:rows]).all()
    assert (got[rows:] == SENTINEL).all()                                                  # Ll = 0: rows 1 and 2 are not written
    return got


def _check(ops, c, pad=0, what="lse"):
    chunk = ops.latent_info_chunk_rows()
    tw = ref.lse(c["z"], c["mu"], c["sig"], c["cst"], c["Lg"], chunk)
    bound = ref.lse_bound(tw, c["Lg"], c["Ll"], chunk)
    got = _lse(ops, c, pad)
    rows = 3 if c["Ll"] else 1
    ratio = np.abs(got[:rows] - tw["lse"][:rows]) / bound[:rows]
    WORST[what] = max(WORST[what], float(ratio.max()))
    print("worst error / bound %.3g (error %.3g, bound %.3g); so far %.3g" % (ratio.max(), np.abs(got[:rows] - tw["lse"][:rows]).max(),
                                                                              bound[:rows].max(), WORST[what]))
    assert (ratio <= 1.0).all()
    return got, tw, bound


# ---------------------------------------------------------------- 1. sv_latent_info_lse against the twin
# one sweep per axis around the base case (Nq 65, Nr 2 chunks + 7, Lg 37, Ll 19): Nr as a multiple m of the chunk plus a remainder
BASE = dict(Nq=65, Nr=(2, 7), Lg=37, Ll=19, pad=0)
SWEEP = ([dict()] + [dict(Nq=v) for v in (1, 63, 64, 130)] + [dict(Nr=v) for v in ((0, 1), (1, -1), (1, 0), (1, 1))] +
         [dict(Lg=v) for v in (1, 3, 128, 256)] + [dict(Ll=v) for v in (1, 3, 128, 256)] + [dict(Ll=0), dict(Ll=0, Lg=32), dict(Lg=32, Ll=32)] +
         [dict(pad=3), dict(pad=4, Lg=32, Ll=32), dict(pad=1, Lg=36, Ll=20)])


@pytest.mark.parametrize("case", SWEEP, ids=lambda c: "-".join("%s%s" % (k, v) for k, v in c.items()).replace(" ", "") or "base")
def test_lse_matches_the_twin_inside_the_bound(env, case):
    """sig log-uniform in [1e-2, 1]; every query has one dominant reference, a few comparable ones and a far-away tail
    (ref.make_case).  |device - twin| <= bound for every element of lse_g, lse_l and lse_gl."""
    ops, _, _ = env
    p = dict(BASE, **case)
    chunk = ops.latent_info_chunk_rows()
    Nr = p["Nr"][0] * chunk + p["Nr"][1]
    _check(ops, ref.make_case(p["Nq"], Nr, p["Lg"], p["Ll"], seed=7), p["pad"])


def test_all_references_equal(env):
    """Nr copies of one posterior: lse equals the single-reference score (log Nr - log Nr), to within the bound."""
    ops, _, _ = env
    c = ref.make_case(33, 1, 37, 19, seed=11)
    one = _check(ops, c)[0]
    many = dict(c, **{k: np.repeat(c[k], 200, axis=0) for k in ("mu", "sig", "rsig", "cst")})
    got, tw, bound = _check(ops, many)
    assert (np.abs(got - one) <= bound + ref.lse_bound(ref.lse(c["z"], c["mu"], c["sig"], c["cst"], 37), 37, 19)).all()


def test_queries_at_their_own_means(env):
    """z_i = mu_i with Nr = Nq: the own pair has a zero quadratic form, so lse_i >= c_i - log N; and the twin agrees."""
    ops, _, _ = env
    c = ref.make_case(70, 70, 37, 19, seed=12)
    c["z"] = c["mu"].copy()
    got, _, bound = _check(ops, c)
    cst = c["cst"].astype(np.float64)
    assert (got[0] >= cst[:, 0] - np.log(70) - bound[0]).all() and (got[1] >= cst[:, 1] - np.log(70) - bound[1]).all()
    assert (got[2] >= cst.sum(1) - np.log(70) - bound[2]).all()


def test_a_far_away_tail_flushes_to_zero(env):
    """One reference at the query, a chunk of references 1e3 standard deviations away: their terms underflow, lse = e - log Nr."""
    ops, _, _ = env
    chunk = ops.latent_info_chunk_rows()
    c = ref.make_case(5, chunk + 1, 8, 4, seed=13)
    c["mu"][:] = 50.0
    c["sig"][:] = 0.05
    c["mu"][3] = 0.0
    c["z"] = (0.01 * np.arange(5 * 12).reshape(5, 12)).astype(np.float32)
    d = ref.draw(c["mu"], c["sig"], np.zeros_like(c["mu"]), 8)
    c["rsig"], c["cst"] = d["rsig"], d["c"].astype(np.float32)
    got, tw, _ = _check(ops, c)
    assert np.allclose(got, np.stack([e[:, 3] for e in tw["e"]]) - np.log(chunk + 1), rtol=0, atol=1e-3)


# ---------------------------------------------------------------- 2. the same bits
def test_bit_identical_on_a_repeat_and_at_other_row_positions(env):
    ops, _, _ = env
    chunk = ops.latent_info_chunk_rows()
    c = ref.make_case(130, chunk + 9, 37, 19, seed=14)
    a = _lse(ops, c)
    assert np.array_equal(a, _lse(ops, c)) and np.array_equal(a, _lse(ops, c, poison=False))
    perm = np.random.default_rng(0).permutation(130)
    assert np.array_equal(_lse(ops, dict(c, z=c["z"][perm])), a[:, perm])
    assert np.array_equal(_lse(ops, dict(c, z=c["z"][37:101])), a[:, 37:101])
    assert np.array_equal(_lse(ops, c, pad=5), a)                                          # the row pitch does not matter either


# ---------------------------------------------------------------- 3. refusals leave the outputs alone
def test_refusals_return_their_status_and_write_nothing(env):
    ops, _, _lib = env
    lib = _lib.load()
    c = ref.make_case(9, 40, 16, 8, seed=15)
    z, mu, rs, cst = _dev(c["z"]), _dev(c["mu"]), _dev(c["rsig"]), torch.from_numpy(c["cst"]).cuda()
    out = torch.full((3, 9), SENTINEL, dtype=F64, device="cuda")
    ws = torch.zeros((ops.latent_info_workspace_bytes(9, 40),), dtype=torch.uint8, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(z_=None, ldz=24, Nq=9, Nr=40, Lg=16, Ll=8, ws_bytes=None, lse=None, wsp=None):
        p = lambda t: C.c_void_p(t.data_ptr())                                            # noqa: E731
        return lib.sv_latent_info_lse(C.c_void_p(z.data_ptr() + 2) if z_ == "misaligned" else None if z_ == "null" else p(z), ldz, p(mu), 24,
                                      p(rs), 24, p(cst), Nq, Nr, Lg, Ll, C.c_void_p(out.data_ptr() + 4) if lse == "misaligned" else p(out),
                                      C.c_void_p(ws.data_ptr() + 8) if wsp == "misaligned" else p(ws),
                                      ws.numel() if ws_bytes is None else ws_bytes, st)
    U, B, W = _lib.STATUS_UNSUPPORTED, _lib.STATUS_BADARG, _lib.STATUS_WORKSPACE
    for want, kw in ((U, dict(Lg=0)), (U, dict(Lg=513, Ll=0)), (U, dict(Ll=-1)), (U, dict(Ll=513)), (U, dict(Nq=0)), (U, dict(Nr=0)),
                     (U, dict(ldz=23)), (B, dict(z_="null")), (B, dict(z_="misaligned")), (B, dict(lse="misaligned")),
                     (B, dict(wsp="misaligned")), (W, dict(ws_bytes=ws.numel() - 1 if ws.numel() else 0)), (W, dict(ws_bytes=0))):
        assert call(**kw) == want, kw
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()
    with pytest.raises(_lib.SplitVaeError, match="SV_E_WORKSPACE"):
        ops.latent_info_lse(z, mu, rs, cst, 16, lse=out, workspace=ws[:-1])
    with pytest.raises(_lib.SplitVaeError, match="SV_E_UNSUPPORTED"):
        ops.latent_info_lse(z, mu, rs, cst, 0, lse=out)
    for bad in (lambda: ops.latent_info_lse(z.double(), mu, rs, cst, 16), lambda: ops.latent_info_lse(z.cpu(), mu, rs, cst, 16),
                lambda: ops.latent_info_lse(z, mu[:, :20], rs, cst, 16), lambda: ops.latent_info_lse(z, mu, rs, cst[:8], 16),
                lambda: ops.latent_info_lse(z, mu, rs, cst, 16, lse=out.float())):
        with pytest.raises(ValueError):
            bad()
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()
    assert call() == 0                                            # and the accepted call writes all of it
    torch.cuda.synchronize()
    assert (out != SENTINEL).all()


# ---------------------------------------------------------------- 4. sv_latent_info_draw and sv_latent_info_finish
def _draw_out(N, Lc, pad=0):
    z = torch.full((N, Lc + pad), SENTINEL, dtype=F32, device="cuda")
    rs = torch.full((N, Lc + pad), SENTINEL, dtype=F32, device="cuda")
    return (z[:, :Lc], rs[:, :Lc], torch.full((N, 2), SENTINEL, dtype=F32, device="cuda"),
            torch.full((N, 2), SENTINEL, dtype=F64, device="cuda"), torch.full((N, 2), SENTINEL, dtype=F64, device="cuda")), (z, rs)


@pytest.mark.parametrize("N,Lg,Ll,pad", [(70, 37, 19, 0), (5, 1, 0, 3), (130, 128, 128, 0), (3, 256, 3, 1)])
def test_draw_with_pinned_eps_matches_the_twin(env, N, Lg, Ll, pad):
    """z and 1 / sig bit for bit (fp32 multiply, add and correctly rounded divide); the row constants and the own term inside the
    error of logf (3 ulp each, summed in fp64) and the constant's one fp32 rounding; the prior term to fp64 rounding; the padding
    behind the rows is neither read nor written."""
    ops, _, _ = env
    mu, sig = ref.make_refs(N, Lg, Ll, seed=21)
    eps = np.random.default_rng(22).standard_normal((N, Lg + Ll)).astype(np.float32)
    out, (zfull, rfull) = _draw_out(N, Lg + Ll, pad)
    z, rs, cst, own, prior = ops.latent_info_draw(_dev(mu, pad), _dev(sig, pad), Lg, eps=_dev(eps, pad), out=out)
    torch.cuda.synchronize()
    d = ref.draw(mu, sig, eps, Lg)
    assert np.array_equal(z.cpu().numpy(), d["z"]) and np.array_equal(rs.cpu().numpy(), d["rsig"])
    if pad:
        assert (zfull[:, Lg + Ll:] == SENTINEL).all() and (rfull[:, Lg + Ll:] == SENTINEL).all()
    nb = 2 if Ll else 1
    ec = np.abs(cst.cpu().numpy().astype(np.float64) - d["c"])[:, :nb] / d["cerr"][:, :nb]
    eo = np.abs(own.cpu().numpy() - d["own"])[:, :nb] / d["cerr"][:, :nb]
    WORST["draw"] = max(WORST["draw"], float(ec.max()), float(eo.max()))
    print("draw: worst error / bound: cst %.3g, own %.3g" % (ec.max(), eo.max()))
    assert (ec <= 1.0).all() and (eo <= 1.0).all()
    assert np.allclose(prior.cpu().numpy(), d["prior"], rtol=1e-13, atol=1e-12)
    if not Ll:
        assert (cst[:, 1] == 0).all() and (own[:, 1] == 0).all() and (prior[:, 1] == 0).all()


def test_free_running_draws_do_not_depend_on_the_batch_split(env):
    ops, _, _ = env
    mu, sig = (_dev(a) for a in ref.make_refs(70, 37, 19, seed=23))
    whole = ops.latent_info_draw(mu, sig, 37, seed=5)
    a = ops.latent_info_draw(mu[:33], sig[:33], 37, seed=5)
    b = ops.latent_info_draw(mu[33:], sig[33:], 37, seed=5, sample_offset=33)
    for w, x, y in zip(whole, a, b):
        assert torch.equal(w, torch.cat([x, y]))
    again = ops.latent_info_draw(mu, sig, 37, seed=5)
    other = ops.latent_info_draw(mu, sig, 37, seed=6)
    assert torch.equal(again[0], whole[0]) and not torch.equal(other[0], whole[0])
    eps = ((whole[0] - mu) / sig).double()
    assert abs(float(eps.mean())) < 0.08 and abs(float(eps.std()) - 1.0) < 0.05       # 3920 standard normals
    g, l = eps[:, :19], eps[:, 37:]
    assert not torch.allclose(g, l, atol=1e-3)                                             # the blocks draw from streams of their own


def test_finish_is_the_twins_report(env):
    ops, _, _ = env
    rng = np.random.default_rng(31)
    for N, Ll in ((1, 3), (300, 3), (257, 0)):
        own, prior, lse = rng.standard_normal((N, 2)) * 50, rng.standard_normal((N, 2)) * 50, rng.standard_normal((3, N)) * 50
        flat = torch.full((24,), SENTINEL, dtype=F64, device="cuda")
        out = ops.latent_info_finish(torch.from_numpy(own).cuda(), torch.from_numpy(prior).cuda(), torch.from_numpy(lse).cuda(), Ll, out=flat[8:16])
        torch.cuda.synchronize()
        assert (flat[:8] == SENTINEL).all() and (flat[16:] == SENTINEL).all()
        want = ref.report(own, prior, lse, Ll)
        assert np.allclose(out.cpu().numpy(), want, rtol=1e-13, atol=1e-11)
        assert torch.equal(out, ops.latent_info_finish(torch.from_numpy(own).cuda(), torch.from_numpy(prior).cuda(), torch.from_numpy(lse).cuda(), Ll))


# ---------------------------------------------------------------- 5. the three models
H, LAT, B, N = 32, 128, 4, 12


def _make(kind):
    from split_vae_amd.gm import LGGMVae
    from split_vae_amd.gmvae import GMVae
    from split_vae_amd.model import LGVae
    shape = (None, H, H, 3)
    if kind == "lgvae-f32":
        return LGVae(LAT, LAT, image_shape=shape, dtype="f32", seed=3)
    if kind == "lgvae-bf16":
        return LGVae(LAT, LAT, image_shape=shape, dtype="bf16", seed=3)
    if kind == "lggmvae":
        return LGGMVae(LAT, LAT, shape, 10, 0.4, dtype="f32", seed=3)
    return GMVae(LAT, shape, 10, 0.4, dtype="f32", seed=3)


@pytest.mark.parametrize("kind", ["lgvae-f32", "lgvae-bf16", "lggmvae", "gmvae"])
def test_evaluate_equals_the_twin_on_the_devices_own_posteriors(env, deterministic, kind):
    """SVHN-32 shapes, batch 4, N = 12 over three batches: latent_info.evaluate equals the twin fed the read-back mu, sig and eps,
    within the mean of the per-element bounds; the figures a model has no right to are None; model._calls stays; a repeat without
    pinned eps gives the same figures."""
    _, latent_info, _ = env
    model = _make(kind)
    rng = np.random.default_rng(41)
    batches = [torch.from_numpy(rng.uniform(-1, 1, (B, H, H, 6)).astype(np.float32)).cuda() for _ in range(4)]
    model._calls = 5
    mu, sig, Lg, Ll = latent_info.posteriors(model, batches, N)
    assert model._calls == 5 and tuple(mu.shape) == (N, Lg + Ll) and Lg == LAT and Ll == (0 if kind == "gmvae" else LAT)
    assert (sig > 0).all() and torch.isfinite(mu).all()
    eps = torch.from_numpy(rng.standard_normal((N, Lg + Ll)).astype(np.float32)).cuda()
    res = latent_info.evaluate(model, batches, N, eps=eps)
    assert model._calls == 5 and res["n_images"] == N and res["log_n"] == pytest.approx(np.log(N), abs=1e-12)
    d = ref.draw(mu.cpu().numpy(), sig.cpu().numpy(), eps.cpu().numpy(), Lg)
    tw = ref.lse(d["z"], mu.cpu().numpy(), sig.cpu().numpy(), d["c"], Lg)
    bound = ref.lse_bound(tw, Lg, Ll, cerr=d["cerr"])
    want = ref.report(d["own"], d["prior"], tw["lse"], Ll)
    cerr = d["cerr"].mean(0)
    tol = dict(kl_g=cerr[0] + 1e-9, mi_g=bound[0].mean() + cerr[0], mkl_g=bound[0].mean() + 1e-9)
    names = dict(kl_g=0, mi_g=1, mkl_g=2)
    if Ll:
        tol.update(kl_l=cerr[1] + 1e-9, mi_l=bound[1].mean() + cerr[1], mkl_l=bound[1].mean() + 1e-9, overlap=bound.sum(0).mean())
        names.update(kl_l=3, mi_l=4, mkl_l=5, overlap=6)
    none = {"lgvae-f32": (), "lgvae-bf16": (), "lggmvae": ("kl_g", "mkl_g"), "gmvae": ("kl_g", "mkl_g", "kl_l", "mi_l", "mkl_l", "overlap")}[kind]
    for k in ("kl_g", "mi_g", "mkl_g", "kl_l", "mi_l", "mkl_l", "overlap"):
        if k in none:
            assert res[k] is None, k
            continue
        ratio = abs(res[k] - want[names[k]]) / tol[k]
        WORST["model"] = max(WORST["model"], ratio)
        print("%s %s: device %.9g twin %.9g error / bound %.3g" % (kind, k, res[k], want[names[k]], ratio))
        assert ratio <= 1.0, k
    if not none:
        assert res["kl_g"] == pytest.approx(res["mi_g"] + res["mkl_g"], abs=1e-9)
    assert res["mi_g"] <= np.log(N) + bound[0].mean() + cerr[0]          # the estimator saturates at log N
    free = latent_info.evaluate(model, batches, N)
    assert free == latent_info.evaluate(model, batches, N) and free != res
    assert latent_info.report_line(res).startswith("Test latent information (12 images, log N = 2.4849): z_g ")


# ---------------------------------------------------------------- 6. CLI
def _lines(out):
    return [l for l in out.splitlines() if l.startswith("Test latent information (")]


CLI = ["--synthetic", "-no_label", "--batch_size", "8", "--training_steps", "1", "--log_every", "1", "--dtype", "f32"]


def test_cli_prints_the_line_once_per_evaluation_and_evaluate_reproduces_it(env, tmp_path, monkeypatch, capsys):
    """--synthetic -no_label (32 test images): one line behind each evaluation's report, none without the flag, the same line from
    evaluate on the saved weights, the history on config-less evaluate's result; N above the test set is clipped with a note."""
    from split_vae_amd import evaluate, main as svmain
    monkeypatch.chdir(tmp_path)
    svmain.main(CLI)
    plain = capsys.readouterr().out
    assert not _lines(plain) and "Training done!" in plain
    path = svmain.main(CLI + ["--latent_info", "20"])
    out = capsys.readouterr().out
    lines = _lines(out)
    assert len(lines) == out.count("Training step ") >= 1 and "clipped" not in out and "Training done!" in out
    assert all(l.startswith("Test latent information (20 images, log N = 2.9957): z_g KL ") and "; z_l KL " in l and
               "; overlap I(z_g; z_l) " in l and l.count("MI ") == 2 and l.count("marginal KL ") == 2 for l in lines), out
    res = evaluate.main(CLI + ["--latent_info", "20", "--weights", path])
    again = capsys.readouterr().out
    assert _lines(again) == [lines[-1]] and "Test IW-" not in again and "Test k-NN" not in again
    assert res["latent_info_n_images"] == 20 and "%.4f" % res["latent_info_mi_g"] in lines[-1]
    both = evaluate.main(CLI + ["--latent_info", "500", "--iw_samples", "2", "--weights", path])
    out2 = capsys.readouterr().out
    assert out2.count("Note: --latent_info 500 clipped to the test set's 32 images") == 1 and len(_lines(out2)) == 1
    assert "(32 images, log N = 3.4657)" in _lines(out2)[0] and "Test IW-2 bound" in out2 and "iw_x" in both


def test_cli_gmvae_reports_the_mi_of_z_g_only(env, tmp_path, monkeypatch, capsys):
    from split_vae_amd import main as svmain
    monkeypatch.chdir(tmp_path)
    svmain.main(CLI + ["--model", "gmvae", "--y_size", "10", "--latent_info", "500"])
    out = capsys.readouterr().out
    lines = _lines(out)
    assert len(lines) >= 1 and out.count("clipped to the test set's 32 images") == 1 and "Training done!" in out
    assert all(l.startswith("Test latent information (32 images, log N = 3.4657): z_g MI ") and "z_l" not in l and "KL" not in l for l in lines), out
