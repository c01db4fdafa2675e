"""Host side of the per-dimension latent report (split_vae_amd/latent_dims.py, csrc/latent_dims.hip): the float64 twin
(tests/latent_dims_ref.py) against a brute-force logsumexp and on limit cases with known answers, the mutants of the twin against its
own bound on the inputs the GPU tests use, the kernel's fp32 arithmetic replayed inside half the bound, the entry points' refusals,
the flags and the report line.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import latent_dims_ref as ref
import latent_info_ref as iref

CHUNK = 4096


def _rand(N, L, seed, dyadic=False):
    e = np.random.default_rng(seed).standard_normal((N, L))
    return (np.round(e * 8) / 8 if dyadic else e).astype(np.float32)


def _report(mu, sig, eps):
    """the whole report of one block in the twin: (prepare, lse, finish, the block figures KL, MI of the --latent_info twin)"""
    L = mu.shape[1]
    d = iref.draw(mu, sig, eps, L)
    p = ref.prepare(mu, sig, eps)
    tw = ref.lse(d["z"], mu, d["rsig"], p["lc"], CHUNK)
    # the block's log-sum-exp from the SAME per-element constants and scale, so that the sums telescope
    w = (d["z"].astype(np.float64)[:, None] - mu.astype(np.float64)[None]) * d["rsig"].astype(np.float64)[None]
    e = (p["lc"].astype(np.float64)[None] - 0.5 * w * w).sum(2)
    lse_block = e.max(1) + np.log(np.exp(e - e.max(1)[:, None]).sum(1)) - np.log(mu.shape[0])
    f = ref.finish(tw["lse"], p["own"], d["z"], lse_block)
    prior = (-ref.HALF_LOG_2PI - 0.5 * d["z"].astype(np.float64) ** 2).sum(1)
    own = p["own"].sum(1)
    return p, tw, f, dict(kl=(own - prior).mean(), mi=(own - lse_block).mean())


# ---------------------------------------------------------------- the twin
def test_the_twin_is_the_brute_force_logsumexp():
    c = iref.make_case(23, 301, 11, 0, seed=3)
    lc = ref.prepare(c["mu"], c["sig"], np.zeros_like(c["mu"]))["lc"]
    tw = ref.lse(c["z"], c["mu"], c["rsig"], lc, CHUNK)
    bf = ref.brute_force(c["z"], c["mu"], c["sig"])
    # the twin takes the fp32 rsig and lc exactly; the definition has 1 / sig and the unrounded lc: a relative 2^-24 on w, an absolute one on lc
    w2 = (((c["z"].astype(np.float64)[:, None] - c["mu"][None]) / c["sig"][None].astype(np.float64)) ** 2).max(1)
    assert (np.abs(tw["lse"] - bf) <= 2 * ref.U * w2 + ref.U * 6.0).all()
    assert tw["lse"].shape == (23, 11) and (tw["bound"] > 0).all() and (tw["bound"] < 0.05).all()


def test_kl_is_mi_plus_tc_plus_dimension_wise_kl():
    mu, sig = iref.make_refs(60, 7, 0, 5)
    _, _, f, blk = _report(mu, sig, _rand(60, 7, 6))
    assert abs(blk["kl"] - (blk["mi"] + f["tc"] + f["dwkl_sum"])) < 1e-12


def test_identical_posteriors_carry_no_information():
    N, L = 40, 5
    mu = np.tile(np.arange(1, L + 1, dtype=np.float32), (N, 1))
    sig = np.full((N, L), 0.5, np.float32)                    # mu + 0.5 * eps and (z - mu) * 2 are exact for dyadic eps
    p, _, f, blk = _report(mu, sig, _rand(N, L, 2, dyadic=True))
    assert np.abs(f["mi"]).max() < 1e-12 and abs(f["tc"]) < 1e-12 and abs(blk["mi"]) < 1e-12
    assert (p["var"] == 0).all() and abs(blk["kl"] - f["dwkl_sum"]) < 1e-12        # the whole KL term is dimension-wise KL


def test_posteriors_equal_to_the_prior_are_inactive():
    N, L = 50, 4
    p = ref.prepare(np.zeros((N, L), np.float32), np.ones((N, L), np.float32), _rand(N, L, 1))
    assert (p["var"] == 0).all() and (p["kl"] == 0).all() and not (p["var"] > ref.ACTIVE).any()
    assert (p["lc"] == np.float32(-ref.HALF_LOG_2PI)).all()


def test_a_block_of_one_dimension_has_no_total_correlation():
    mu, sig = iref.make_refs(70, 1, 0, 8)
    _, _, f, blk = _report(mu, sig, _rand(70, 1, 9))
    assert abs(f["tc"]) < 1e-12 and abs(blk["mi"] - f["mi"][0]) < 1e-12


def test_separated_posteriors_saturate_at_log_n_and_are_active():
    N, L = 50, 3
    mu = (100.0 * np.arange(N)[:, None] * np.ones((1, L))).astype(np.float32)
    p, _, f, _ = _report(mu, np.full((N, L), 0.5, np.float32), _rand(N, L, 3, dyadic=True))
    assert np.abs(f["mi"] - np.log(N)).max() < 1e-9 and (p["var"] > ref.ACTIVE).all()


# ---------------------------------------------------------------- mutants and the fp32 replay on the GPU tests' base case
@pytest.fixture(scope="module")
def base():
    c = iref.make_case(65, 2 * CHUNK + 7, 37, 0, seed=7)
    c["lc"] = ref.prepare(c["mu"], c["sig"], np.zeros_like(c["mu"]))["lc"]
    c["tw"] = ref.lse(c["z"], c["mu"], c["rsig"], c["lc"], CHUNK)
    return c


def test_the_base_case_has_comparable_and_flushed_references(base):
    assert np.isfinite(base["tw"]["lse"]).all() and (base["tw"]["bound"] < 0.01).all()
    e = base["lc"][None, :, 0].astype(np.float64) - 0.5 * ((base["z"][:, None, 0].astype(np.float64) - base["mu"][None, :, 0]) * base["rsig"][None, :, 0]) ** 2
    gap = e.max(1)[:, None] - e
    assert ((gap < 3).sum(1) >= 2).all() and ((gap > 87).sum(1) > 0).any()


@pytest.mark.parametrize("mutant", ref.MUTANTS)
def test_every_mutant_of_the_twin_leaves_the_bound(base, mutant):
    got = ref.lse(base["z"], base["mu"], base["rsig"], base["lc"], CHUNK, mutant=mutant)["lse"]
    ratio = np.abs(got - base["tw"]["lse"]) / base["tw"]["bound"]
    print("%s: worst error / bound %.3g, elements outside %d of %d" % (mutant, ratio.max(), (ratio > 1).sum(), ratio.size))
    assert (ratio > 1.0).any()


@pytest.mark.parametrize("mutant", ref.PREPARE_MUTANTS)
def test_every_mutant_of_prepare_leaves_its_tolerance(base, mutant):
    eps = np.zeros_like(base["mu"])
    a, b = ref.prepare(base["mu"], base["sig"], eps), ref.prepare(base["mu"], base["sig"], eps, mutant=mutant)
    assert not all(np.allclose(a[k], b[k], rtol=1e-12, atol=0) for k in ("var", "kl"))


def test_there_are_at_least_ten_mutants():
    assert len(set(ref.MUTANTS)) >= 10


def test_the_fp32_replay_stays_inside_half_the_bound(base):
    got = ref.lse_fp32(base["z"], base["mu"], base["rsig"], base["lc"], CHUNK)
    ratio = np.abs(got - base["tw"]["lse"]) / base["tw"]["bound"]
    print("replay: worst error / bound %.3g" % ratio.max())
    assert (ratio <= 0.5).all()


# ---------------------------------------------------------------- refusals, through the built library without a GPU
def _bufs():
    return {k: (C.c_double * 64)() for k in ("mu", "sig", "eps", "z", "rsig", "lc", "lse", "own", "cols", "blk", "out", "ws")}


def _ptr(b, a, name):
    if name in a["null"]:
        return None
    return C.c_void_p(C.addressof(b[name]) + (2 if name in a["misalign"] else 0))


def _status(rc):
    from split_vae_amd import _lib
    return _lib.STATUS.get(rc, rc)


def _lse_call(lib, **kw):
    a = dict(Nq=9, Nr=40, L=24, ld=(24, 24, 24, 24, 24), null=(), misalign=(), short=0)
    a.update(kw)
    b = _bufs()
    n = C.c_int64(0)
    lib.sv_latent_dims_workspace_bytes(max(a["Nq"], 1), max(a["Nr"], 1), min(max(a["L"], 1), 512), C.byref(n))
    return _status(lib.sv_latent_dims_lse(_ptr(b, a, "z"), a["ld"][0], _ptr(b, a, "mu"), a["ld"][1], _ptr(b, a, "rsig"), a["ld"][2],
                                          _ptr(b, a, "lc"), a["ld"][3], a["Nq"], a["Nr"], a["L"], _ptr(b, a, "lse"), a["ld"][4],
                                          _ptr(b, a, "ws"), n.value - a["short"], None))


def _prepare_call(lib, **kw):
    a = dict(N=8, L=24, ld=(24, 24, 24, 24), block=0, offset=0, null=(), misalign=())
    a.update(kw)
    b = _bufs()
    return _status(lib.sv_latent_dims_prepare(_ptr(b, a, "mu"), a["ld"][0], _ptr(b, a, "sig"), a["ld"][1], _ptr(b, a, "eps"), a["ld"][2],
                                              _ptr(b, a, "lc"), a["ld"][3], _ptr(b, a, "own"), _ptr(b, a, "cols"), a["N"], a["L"], a["block"],
                                              5, a["offset"], None))


def _finish_call(lib, **kw):
    a = dict(N=8, L=24, ld=(24, 24), null=(), misalign=())
    a.update(kw)
    b = _bufs()
    return _status(lib.sv_latent_dims_finish(_ptr(b, a, "lse"), a["ld"][0], _ptr(b, a, "own"), _ptr(b, a, "z"), a["ld"][1], _ptr(b, a, "blk"),
                                             a["N"], a["L"], _ptr(b, a, "out"), None))


def test_entry_points_refuse_everything_outside_the_domain(lib_built):
    """Host addresses: every refusal is decided before anything is enqueued, so nothing is dereferenced."""
    from split_vae_amd import _lib
    lib = _lib.load()
    chunk = lib.sv_latent_dims_chunk_rows()
    assert chunk == CHUNK and chunk % 64 == 0
    for bad in (dict(L=0), dict(L=513), dict(L=-1), dict(Nq=0), dict(Nr=0), dict(Nq=-3)) + tuple(
            dict(ld=[24 - (i == k) for i in range(5)]) for k in range(5)):
        assert _lse_call(lib, **bad) == "SV_E_UNSUPPORTED", bad
    for name in ("z", "mu", "rsig", "lc", "lse", "ws"):
        assert _lse_call(lib, null=(name,)) == "SV_E_BADARG", name
        assert _lse_call(lib, misalign=(name,)) == "SV_E_BADARG", name
    assert _lse_call(lib, short=1) == "SV_E_WORKSPACE"
    assert _lse_call(lib, short=1, Nq=1, Nr=1, L=1, ld=(5, 1, 2, 3, 1)) == "SV_E_WORKSPACE"          # the domain's corners are accepted
    assert _lse_call(lib, short=1, Nq=130, Nr=2 * chunk + 7, L=512, ld=(512,) * 5) == "SV_E_WORKSPACE"
    for bad in (dict(L=0), dict(L=513), dict(N=0), dict(offset=-1), dict(block=2), dict(block=-1)) + tuple(
            dict(ld=[24 - (i == k) for i in range(4)]) for k in range(4)):
        assert _prepare_call(lib, **bad) == "SV_E_UNSUPPORTED", bad
    for name in ("mu", "sig", "lc", "own", "cols"):
        assert _prepare_call(lib, null=(name,)) == "SV_E_BADARG", name
    for name in ("mu", "sig", "eps", "lc", "own", "cols"):
        assert _prepare_call(lib, misalign=(name,)) == "SV_E_BADARG", name
    for bad in (dict(N=0), dict(L=0), dict(L=513), dict(ld=(23, 24)), dict(ld=(24, 23))):
        assert _finish_call(lib, **bad) == "SV_E_UNSUPPORTED", bad
    for name in ("lse", "own", "z", "blk", "out"):
        assert _finish_call(lib, null=(name,)) == "SV_E_BADARG", name
        assert _finish_call(lib, misalign=(name,)) == "SV_E_BADARG", name


def test_workspace_bytes(lib_built):
    from split_vae_amd import _lib
    lib = _lib.load()

    def ws(Nq, Nr, L):
        n = C.c_int64(-7)
        return lib.sv_latent_dims_workspace_bytes(Nq, Nr, L, C.byref(n)), n.value
    assert lib.sv_latent_dims_workspace_bytes(8, 40, 24, None) == _lib.STATUS_BADARG
    for bad in ((0, 40, 24), (8, 0, 24), (-1, 5, 24), (8, 40, 0), (8, 40, 513)):
        assert ws(*bad) == (_lib.STATUS_UNSUPPORTED, -7), bad
    sizes = [(1, 1, 1), (1, CHUNK, 37), (1, CHUNK + 1, 37), (65, CHUNK + 1, 37), (65, 2 * CHUNK + 7, 37), (26032, 26032, 256)]
    vals = [ws(*s) for s in sizes]
    assert all(rc == 0 for rc, _ in vals) and all(b[1] >= a[1] for a, b in zip(vals, vals[1:]))
    assert vals[4][1] >= 65 * 3 * 37 * 2 * 4 and vals[2][1] >= 2 * vals[1][1] - 256 and all(v % 256 == 0 for _, v in vals)
    assert ws(1 << 22, 1 << 22, 512)[1] > 1 << 35                # int64 arithmetic past 2^31 bytes


def test_header_and_binding_agree_on_the_new_entry_points(lib_built):
    import os
    import re
    from split_vae_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "splitvae.h")).read(), flags=re.S)
    lib = _lib.load()
    names = sorted(n for n in _lib.SYMBOLS if n.startswith("sv_latent_dims_"))
    assert names == ["sv_latent_dims_chunk_rows", "sv_latent_dims_finish", "sv_latent_dims_lse", "sv_latent_dims_prepare",
                     "sv_latent_dims_workspace_bytes"]
    for name in names:
        m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, src, flags=re.S)
        assert m, name
        params = [p for p in m.group(1).split(",") if p.strip() and p.strip() != "void"]
        assert len(params) == len(_lib.SYMBOLS[name][1]), name
        for p, ct in zip(params, _lib.SYMBOLS[name][1]):
            want = None if "*" in p else (C.c_int32 if "int32_t" in p else C.c_uint64 if "uint64_t" in p else C.c_int64 if "int64_t" in p
                                          else None)
            assert want is None or ct is want, (name, p)
            assert want is not None or ct in (C.c_void_p, C.POINTER(C.c_int64)), (name, p)
        assert hasattr(lib, name)


# ---------------------------------------------------------------- flags and the report line
def test_parser_has_the_flag_outside_the_reference_options():
    from split_vae_amd import main as svmain
    ap = svmain.build_parser()
    assert ap.parse_args([]).latent_dims == 0 and ap.parse_args(["--latent_dims", "500"]).latent_dims == 500
    assert "--latent_dims" not in [f for f, _, _ in svmain.REFERENCE_OPTIONS] and "--latent_dims" not in svmain.REFERENCE_SWITCHES
    assert "--latent_dims" in svmain.__doc__ and "0.01" in ap.format_help()


@pytest.mark.parametrize("entry", ["main", "evaluate"])
@pytest.mark.parametrize("flags,words", [(["--latent_dims", "1"], ("--latent_dims", "N >= 2")),
                                         (["--latent_dims", "-4"], ("--latent_dims", "N >= 2")),
                                         (["--latent_dims", "100", "--global_latent_dims", "600"], ("--latent_dims", "512")),
                                         (["--latent_dims", "100", "--local_latent_dims", "513"], ("--latent_dims", "512"))])
def test_bad_flags_are_refused_before_any_device_work(monkeypatch, capsys, entry, flags, words):
    import split_vae_amd
    import torch
    from split_vae_amd import _lib, data, evaluate, main as svmain

    def boom(*a, **k):
        raise AssertionError("device or data work before the refusal")
    monkeypatch.setattr(split_vae_amd, "configure_hw_queues", boom)
    monkeypatch.setattr(torch.cuda, "is_available", boom)
    monkeypatch.setattr(torch.cuda, "_lazy_init", boom)
    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setattr(data, "get_dataset", boom)
    with pytest.raises(SystemExit) as e:
        if entry == "main":
            svmain.main(flags + ["-no_label"])
        else:
            evaluate.main(flags + ["-no_label", "--weights", "nowhere.npz"])
    assert all(w in str(e.value) for w in words), str(e.value)
    assert "Config:" not in capsys.readouterr().out


def test_check_flags():
    from split_vae_amd import latent_dims
    latent_dims.check_flags(100, 128, 0)                          # gmvae: no local block
    latent_dims.check_flags(0, 9999, 9999)                        # off: nothing to check
    latent_dims.check_flags(2, 512, 512)
    for bad in ((100, 0, 0), (1, 8, 8), (-1, 8, 8), (100, 513, 0)):
        with pytest.raises(SystemExit):
            latent_dims.check_flags(*bad)


def test_evaluate_counts_the_flag_as_something_to_measure(monkeypatch):
    import split_vae_amd
    from split_vae_amd import evaluate

    class Reached(Exception):
        pass

    def reached(*a, **k):
        raise Reached()
    monkeypatch.setattr(split_vae_amd, "configure_hw_queues", reached)
    with pytest.raises(SystemExit) as e:
        evaluate.main(["--weights", "nowhere.npz"])
    assert str(e.value).startswith("nothing to measure: pass --iw_samples K") and str(e.value).endswith("--latent_dims N (test images of the "
                                                                                                        "per-dimension latent report, N >= 2)")
    with pytest.raises(Reached):
        evaluate.main(["--weights", "nowhere.npz", "--latent_dims", "50", "-no_label"])


def _res():
    g = dict(dims_g=4, active_g=3, var_g=[0.5, 0.001, 0.2, 0.3], kl_g=[1.5, 0.0, 2.25, 0.5], mi_g=[1.0, 0.0, 2.0, 0.4],
             dwkl_g=[0.5, 0.0, 0.25, 0.1], tc_g=0.75, dwkl_sum_g=0.85, block_kl_g=4.25, block_mi_g=2.65)
    l = dict(dims_l=2, active_l=0, var_l=[0.0, 0.0], kl_l=[0.001, 0.002], mi_l=[0.0, 0.0], dwkl_l=[0.001, 0.002], tc_l=0.0001,
             dwkl_sum_l=0.003, block_kl_l=0.003, block_mi_l=0.0)
    return dict(n_images=26032, log_n=10.16708, **g, **l)


def test_report_line():
    from split_vae_amd import latent_dims
    res = _res()
    assert latent_dims.report_line(res) == ("Test latent dimensions (26032 images, log N = 10.1671): z_g active 3/4 (largest KL_j 2.2500 at "
                                            "dim 2), TC 0.7500, dimension-wise KL 0.8500; z_l active 0/2 (largest KL_j 0.0020 at dim 1), "
                                            "TC 0.0001, dimension-wise KL 0.0030")
    gm = dict(res, kl_g=None, dwkl_g=None, dwkl_sum_g=None, block_kl_g=None)                        # lggmvae: the prior of z_g is a mixture
    assert latent_dims.report_line(gm).startswith("Test latent dimensions (26032 images, log N = 10.1671): z_g active 3/4, TC 0.7500; z_l active 0/2 (")
    one = dict(gm, **{k + "_l": None for k in latent_dims.BLOCK_KEYS})                              # gmvae
    assert latent_dims.report_line(one) == "Test latent dimensions (26032 images, log N = 10.1671): z_g active 3/4, TC 0.7500"
    assert latent_dims.CLIPPED.format(500, 27) == "Note: --latent_dims 500 clipped to the test set's 27 images"


def test_report_keeps_the_history_and_notes_the_clip_once(monkeypatch, capsys):
    from split_vae_amd import latent_dims
    from split_vae_amd.utils import dotdict
    monkeypatch.setattr(latent_dims, "evaluate", lambda model, batches, n: dict(_res(), n_images=27))
    config = dotdict(latent_dims=500)
    assert latent_dims.report(None, [], dotdict(latent_dims=0)) is None
    latent_dims.report(None, [], config, step=10)
    latent_dims.report(None, [], config, step=20)
    out = capsys.readouterr().out
    assert out.count("Note: --latent_dims 500 clipped to the test set's 27 images") == 1 and out.count("Test latent dimensions (27 images") == 2
    assert [h["step"] for h in config.latent_dims_history] == [10, 20]
    assert all(len(config.latent_dims_history[0][k + "_g"]) == 4 for k in ("var", "kl", "mi", "dwkl"))
