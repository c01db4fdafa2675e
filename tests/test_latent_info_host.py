"""Host side of the aggregate-posterior information report (split_vae_amd/latent_info.py, csrc/latent_info.hip): the float64 twin
(tests/latent_info_ref.py) on limit cases with known answers, the mutants of the twin against its own bound on the inputs the GPU
tests use, the kernel's fp32 arithmetic replayed inside the bound, the entry points' refusals, the flags and the report line.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import latent_info_ref as ref

CHUNK = 1024


def _report(mu, sig, eps, Lg):
    d = ref.draw(mu, sig, eps, Lg)
    tw = ref.lse(d["z"], mu, sig, d["c"], Lg)
    return ref.report(d["own"], d["prior"], tw["lse"], mu.shape[1] - Lg)


def _rand(N, Lc, seed, dyadic=False):
    """standard normal fp32; dyadic: rounded to eighths, so that mu + 0.5 * eps is exact in fp32 for integer mu below 2^13 and the
    sample's own pair score equals the closed-form own term to fp64 rounding"""
    rng = np.random.default_rng(seed)
    e = rng.standard_normal((N, Lc))
    return (np.round(e * 8) / 8 if dyadic else e).astype(np.float32)


# ---------------------------------------------------------------- limit cases
def test_identical_posteriors_carry_no_information():
    N, Lg, Ll = 40, 5, 3
    mu = np.tile(_rand(1, Lg + Ll, 0), (N, 1))
    sig = np.tile(np.exp(0.3 * _rand(1, Lg + Ll, 1)), (N, 1)).astype(np.float32)
    o = _report(mu, sig, _rand(N, Lg + Ll, 2), Lg)
    assert abs(o[1]) < 1e-9 and abs(o[4]) < 1e-9 and abs(o[6]) < 1e-9        # MI = 0, overlap = 0
    assert abs(o[2] - o[0]) < 1e-9 and abs(o[5] - o[3]) < 1e-9              # marginal KL = KL
    assert o[7] == np.log(N)


def test_separated_posteriors_saturate_at_log_n():
    N, Lg, Ll = 50, 4, 2
    mu = (100.0 * np.arange(N)[:, None] * np.ones((1, Lg + Ll))).astype(np.float32)
    sig = np.full((N, Lg + Ll), 0.5, np.float32)
    o = _report(mu, sig, _rand(N, Lg + Ll, 3, dyadic=True), Lg)
    assert abs(o[1] - np.log(N)) < 1e-9 and abs(o[4] - np.log(N)) < 1e-9
    assert abs(o[6] - np.log(N)) < 1e-9                                      # both separated: the documented saturation


def test_overlap_vanishes_when_one_block_is_constant():
    N, Lg, Ll = 50, 4, 3
    mu = (100.0 * np.arange(N)[:, None] * np.ones((1, Lg + Ll))).astype(np.float32)
    mu[:, Lg:] = 0.25
    sig = np.full((N, Lg + Ll), 0.5, np.float32)
    o = _report(mu, sig, _rand(N, Lg + Ll, 4, dyadic=True), Lg)
    assert abs(o[6]) < 1e-9 and abs(o[4]) < 1e-9 and abs(o[1] - np.log(N)) < 1e-9


def test_kl_is_mi_plus_marginal_kl():
    N, Lg, Ll = 60, 7, 5
    mu, sig = ref.make_refs(N, Lg, Ll, 5)
    o = _report(mu, sig, _rand(N, Lg + Ll, 6), Lg)
    assert abs(o[0] - (o[1] + o[2])) < 1e-9 * max(1.0, abs(o[0])) and abs(o[3] - (o[4] + o[5])) < 1e-9 * max(1.0, abs(o[3]))
    assert 0 < o[1] <= np.log(N) + 1e-9 and 0 < o[4] <= np.log(N) + 1e-9


def test_average_kl_matches_the_closed_form():
    """own_i - prior_i is a one-sample estimate of KL(q_i || N(0, I)): over 4000 draws of one image it meets the closed form."""
    L = 3
    mu = np.tile(np.array([[0.3, -1.0, 2.0]], np.float32), (4000, 1))
    sig = np.tile(np.array([[0.5, 1.5, 0.1]], np.float32), (4000, 1))
    d = ref.draw(mu, sig, _rand(4000, L, 7), L)
    kl = 0.5 * (sig[0].astype(np.float64) ** 2 + mu[0].astype(np.float64) ** 2 - 1.0).sum() - np.log(sig[0].astype(np.float64)).sum()
    assert abs((d["own"][:, 0] - d["prior"][:, 0]).mean() - kl) < 0.1


# ---------------------------------------------------------------- mutants and the fp32 replay, on the GPU tests' inputs
@pytest.fixture(scope="module")
def base():
    c = ref.make_case(65, 2 * CHUNK + 7, 37, 19)
    tw = ref.lse(c["z"], c["mu"], c["sig"], c["cst"], 37, CHUNK)
    return c, tw, ref.lse_bound(tw, 37, 19, CHUNK)


def test_the_base_case_has_dominant_comparable_and_flushed_references(base):
    c, tw, bound = base
    e = tw["e"][2]
    gap = e.max(1)[:, None] - e
    assert ((gap < 30).sum(1) >= 2).all() and ((gap < 30).sum(1) <= 8).all()     # the family: a few comparable references
    assert ((gap > 87).sum(1) > 2000).all()                                      # the far-away tail flushes
    assert np.isfinite(bound).all() and (bound > 0).all() and bound.max() < 2e-2


@pytest.mark.parametrize("mutant", ref.MUTANTS)
def test_every_mutant_of_the_twin_leaves_the_bound(base, mutant):
    c, tw, bound = base
    wrong = ref.lse(c["z"], c["mu"], c["sig"], c["cst"], 37, CHUNK, mutant=mutant)["lse"]
    worst = np.nanmax(np.abs(wrong - tw["lse"]) / bound)
    assert worst > 1.0, (mutant, worst)


def test_there_are_at_least_a_dozen_mutants():
    assert len(ref.MUTANTS) >= 12 and len(set(ref.MUTANTS)) == len(ref.MUTANTS)


def test_the_fp32_replay_stays_inside_the_bound(base):
    c, tw, bound = base
    got = ref.lse_fp32(c["z"], c["mu"], c["rsig"], c["cst"], 37, CHUNK)
    ratio = np.abs(got - tw["lse"]) / bound
    print("fp32 replay: worst error / bound %.3g" % ratio.max())
    assert (ratio <= 1.0).all() and ratio.max() > 1e-4           # inside, and the bound is not orders of magnitude loose


def test_the_fp32_replay_one_block(base):
    c = ref.make_case(7, 130, 3, 0, seed=3)
    tw = ref.lse(c["z"], c["mu"], c["sig"], c["cst"], 3, CHUNK)
    got = ref.lse_fp32(c["z"], c["mu"], c["rsig"], c["cst"], 3, CHUNK)
    assert (np.abs(got[0] - tw["lse"][0]) <= ref.lse_bound(tw, 3, 0, CHUNK)[0]).all()
    assert np.isnan(got[1:]).all() and np.isnan(tw["lse"][1:]).all()


# ---------------------------------------------------------------- entry-point validation (host code of the built library)
def _bufs():
    return {n: np.zeros(1 << 16, np.uint8) for n in ("mu", "sig", "eps", "z", "rsig", "cst", "own", "prior", "lse", "out", "ws")}


def _ptr(bufs, a, n):
    if n in a["null"]:
        return None
    addr = (bufs[n].ctypes.data + 63) // 64 * 64
    return C.c_void_p(addr + (4 if n in a["misalign"] and n in ("own", "prior", "lse", "out", "ws") else 1 if n in a["misalign"] else 0))


def _lse_call(lib, **kw):
    from split_vae_amd import _lib
    a = dict(Nq=8, Nr=40, Lg=16, Ll=8, ld=None, short=0, null=(), misalign=())
    a.update(kw)
    ldz, ldm, ldr = (a["Lg"] + a["Ll"],) * 3 if a["ld"] is None else a["ld"]
    nbytes = C.c_int64(1 << 16)
    lib.sv_latent_info_workspace_bytes(a["Nq"], a["Nr"], C.byref(nbytes))
    assert nbytes.value <= 1 << 16
    b = _bufs()
    rc = lib.sv_latent_info_lse(_ptr(b, a, "z"), ldz, _ptr(b, a, "mu"), ldm, _ptr(b, a, "rsig"), ldr, _ptr(b, a, "cst"), a["Nq"], a["Nr"],
                                a["Lg"], a["Ll"], _ptr(b, a, "lse"), _ptr(b, a, "ws"), nbytes.value - a["short"], None)
    return _lib.STATUS.get(rc, rc)


def _draw_call(lib, **kw):
    from split_vae_amd import _lib
    a = dict(N=8, Lg=16, Ll=8, ld=None, null=(), misalign=(), offset=0)
    a.update(kw)
    ld = [a["Lg"] + a["Ll"]] * 5 if a["ld"] is None else a["ld"]
    b = _bufs()
    rc = lib.sv_latent_info_draw(_ptr(b, a, "mu"), ld[0], _ptr(b, a, "sig"), ld[1], _ptr(b, a, "eps"), ld[2], _ptr(b, a, "z"), ld[3],
                                 _ptr(b, a, "rsig"), ld[4], _ptr(b, a, "cst"), _ptr(b, a, "own"), _ptr(b, a, "prior"), a["N"], a["Lg"],
                                 a["Ll"], 1, a["offset"], None)
    return _lib.STATUS.get(rc, rc)


def _finish_call(lib, **kw):
    from split_vae_amd import _lib
    a = dict(N=8, Ll=8, null=(), misalign=())
    a.update(kw)
    b = _bufs()
    rc = lib.sv_latent_info_finish(_ptr(b, a, "own"), _ptr(b, a, "prior"), _ptr(b, a, "lse"), a["N"], a["Ll"], _ptr(b, a, "out"), None)
    return _lib.STATUS.get(rc, rc)


def test_entry_points_refuse_everything_outside_the_domain(lib_built):
    """Host addresses: every refusal is decided before anything is enqueued, so nothing is dereferenced."""
    from split_vae_amd import _lib
    lib = _lib.load()
    chunk = lib.sv_latent_info_chunk_rows()
    assert chunk == CHUNK and chunk % 64 == 0
    for bad in (dict(Lg=0), dict(Lg=513), dict(Ll=-1), dict(Ll=513), dict(Nq=0), dict(Nr=0), dict(Nq=-3), dict(ld=(23, 24, 24)),
                dict(ld=(24, 23, 24)), dict(ld=(24, 24, 23))):
        assert _lse_call(lib, **bad) == "SV_E_UNSUPPORTED", bad
    for name in ("z", "mu", "rsig", "cst", "lse", "ws"):
        assert _lse_call(lib, null=(name,)) == "SV_E_BADARG", name
        assert _lse_call(lib, misalign=(name,)) == "SV_E_BADARG", name
    assert _lse_call(lib, short=1) == "SV_E_WORKSPACE"
    assert _lse_call(lib, short=1, Nq=1, Nr=1, Lg=1, Ll=0, ld=(5, 1, 2)) == "SV_E_WORKSPACE"         # the domain's corners are accepted
    assert _lse_call(lib, short=1, Nq=130, Nr=2 * chunk + 7, Lg=512, Ll=512) == "SV_E_WORKSPACE"
    for bad in (dict(Lg=0), dict(Lg=513), dict(Ll=-1), dict(Ll=513), dict(N=0), dict(offset=-1)) + tuple(
            dict(ld=[24 - (i == k) for i in range(5)]) for k in range(5)):
        assert _draw_call(lib, **bad) == "SV_E_UNSUPPORTED", bad
    for name in ("mu", "sig", "z", "rsig", "cst", "own", "prior"):
        assert _draw_call(lib, null=(name,)) == "SV_E_BADARG", name
    for name in ("mu", "sig", "eps", "z", "rsig", "cst", "own", "prior"):
        assert _draw_call(lib, misalign=(name,)) == "SV_E_BADARG", name
    for bad in (dict(N=0), dict(Ll=-1), dict(Ll=513)):
        assert _finish_call(lib, **bad) == "SV_E_UNSUPPORTED", bad
    for name in ("own", "prior", "lse", "out"):
        assert _finish_call(lib, null=(name,)) == "SV_E_BADARG", name
        assert _finish_call(lib, misalign=(name,)) == "SV_E_BADARG", name


def test_workspace_bytes(lib_built):
    from split_vae_amd import _lib
    lib = _lib.load()

    def ws(Nq, Nr):
        n = C.c_int64(-7)
        return lib.sv_latent_info_workspace_bytes(Nq, Nr, C.byref(n)), n.value
    assert lib.sv_latent_info_workspace_bytes(8, 40, None) == _lib.STATUS_BADARG
    for bad in ((0, 40), (8, 0), (-1, 5)):
        assert ws(*bad) == (_lib.STATUS_UNSUPPORTED, -7), bad
    sizes = [(1, 1), (1, CHUNK), (1, CHUNK + 1), (65, CHUNK + 1), (65, 2 * CHUNK + 7), (26032, 26032)]
    vals = [ws(*s) for s in sizes]
    assert all(rc == 0 for rc, _ in vals) and all(b[1] >= a[1] for a, b in zip(vals, vals[1:]))
    assert vals[4][1] >= 65 * 3 * 3 * 2 * 4 and vals[2][1] >= 2 * vals[0][1] - 256
    assert ws(1 << 22, 1 << 22)[1] > 1 << 35                     # int64 arithmetic past 2^31 bytes


def test_header_and_binding_agree_on_the_new_entry_points(lib_built):
    import os
    import re
    from split_vae_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "splitvae.h")).read(), flags=re.S)
    lib = _lib.load()
    names = sorted(n for n in _lib.SYMBOLS if n.startswith("sv_latent_info_"))
    assert names == ["sv_latent_info_chunk_rows", "sv_latent_info_draw", "sv_latent_info_finish", "sv_latent_info_lse",
                     "sv_latent_info_workspace_bytes"]
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
    assert _lib.LATENT_INFO_MAX_L == 512


# ---------------------------------------------------------------- flags and the report line
def test_parser_has_the_flag_outside_the_reference_options():
    from split_vae_amd import main as svmain
    ap = svmain.build_parser()
    assert ap.parse_args([]).latent_info == 0 and ap.parse_args(["--latent_info", "500"]).latent_info == 500
    assert "--latent_info" not in [f for f, _, _ in svmain.REFERENCE_OPTIONS] and "--latent_info" not in svmain.REFERENCE_SWITCHES


@pytest.mark.parametrize("entry", ["main", "evaluate"])
@pytest.mark.parametrize("flags,words", [(["--latent_info", "1"], ("--latent_info", "N >= 2")),
                                         (["--latent_info", "-4"], ("--latent_info", "N >= 2")),
                                         (["--latent_info", "100", "--global_latent_dims", "600"], ("--latent_info", "512")),
                                         (["--latent_info", "100", "--local_latent_dims", "513"], ("--latent_info", "512"))])
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


def test_gmvae_has_no_local_block_to_refuse():
    from split_vae_amd import latent_info
    latent_info.check_flags(100, 128, 0)
    latent_info.check_flags(0, 9999, 9999)                        # off: nothing to check
    with pytest.raises(SystemExit):
        latent_info.check_flags(100, 0, 0)


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
    assert str(e.value).startswith("nothing to measure: pass --iw_samples K") and "--latent_info N" in str(e.value)
    with pytest.raises(Reached):
        evaluate.main(["--weights", "nowhere.npz", "--latent_info", "50", "-no_label"])


def test_report_line():
    from split_vae_amd import latent_info
    res = dict(n_images=26032, log_n=10.16708, kl_g=61.25, mi_g=9.87654, mkl_g=51.37346, kl_l=20.5, mi_l=8.25, mkl_l=12.25, overlap=0.12345)
    assert latent_info.report_line(res) == ("Test latent information (26032 images, log N = 10.1671): z_g KL 61.2500, MI 9.8765, marginal KL "
                                            "51.3735; z_l KL 20.5000, MI 8.2500, marginal KL 12.2500; overlap I(z_g; z_l) 0.1235")
    gm = dict(res, kl_g=None, mkl_g=None)
    assert latent_info.report_line(gm).startswith("Test latent information (26032 images, log N = 10.1671): z_g MI 9.8765; z_l KL 20.5000")
    one = dict(gm, kl_l=None, mi_l=None, mkl_l=None, overlap=None)
    assert latent_info.report_line(one) == "Test latent information (26032 images, log N = 10.1671): z_g MI 9.8765"
    assert latent_info.CLIPPED.format(500, 27) == "Note: --latent_info 500 clipped to the test set's 27 images"
