"""Host side of the k-NN label probe (split_vae_amd/probe.py, csrc/knn.hip): the float64 twin (tests/knn_ref.py) on hand-worked
cases, the entry points' argument checks through the built library, the flags and their refusals, the report line.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import knn_ref


# ---------------------------------------------------------------- the twin, by hand
def test_twin_on_a_line_of_points():
    r = np.array([[0.0], [1.0], [2.0], [4.0], [8.0]])
    q = np.array([[2.9], [-1.0], [8.0]])
    idx, dist, pred, d = knn_ref.classify(q, r, np.array([0, 0, 1, 1, 2], np.uint8), 3, 3)
    assert idx.tolist() == [[2, 3, 1], [0, 1, 2], [4, 3, 2]]
    np.testing.assert_allclose(dist, [[0.81, 1.21, 3.61], [1.0, 4.0, 9.0], [0.0, 16.0, 36.0]], rtol=1e-12, atol=1e-12)
    assert pred.tolist() == [1, 0, 1]
    assert d.shape == (3, 5) and (d >= 0).all()
    np.testing.assert_allclose(knn_ref.boundary_gap(d, 3), [(8.41 - 3.61) / 8.41, (25.0 - 9.0) / 25.0, (49.0 - 36.0) / 49.0], rtol=1e-12)
    assert np.isinf(knn_ref.boundary_gap(d, 5)).all()


def test_twin_resolves_an_exact_tie_to_the_lower_index():
    r = np.array([[1.0, 0.0], [0.0, 1.0], [-1.0, 0.0], [0.0, -1.0], [3.0, 0.0]])      # four points at distance 1 from the origin
    idx, dist, pred, d = knn_ref.classify(np.zeros((1, 2)), r, np.array([3, 2, 1, 0, 0], np.uint8), 2, 4)
    assert idx.tolist() == [[0, 1]] and dist.tolist() == [[1.0, 1.0]]
    assert pred.tolist() == [2]                                  # one vote each for classes 3 and 2: the lower id
    assert knn_ref.boundary_gap(d, 2).tolist() == [0.0]          # the third is as near as the second: a tie at the boundary
    # the same references in another order: the SET changes with the indices, by the rule
    idx2, _, _, _ = knn_ref.classify(np.zeros((1, 2)), r[[3, 2, 1, 0, 4]], np.array([0, 1, 2, 3, 0], np.uint8), 2, 4)
    assert idx2.tolist() == [[0, 1]]


def test_twin_resolves_a_2_2_1_vote_to_the_lowest_class():
    r = np.arange(1.0, 6.0)[:, None]                             # distances 1, 4, 9, 16, 25 from the origin
    for classes, want in (([7, 3, 5, 7, 3], 3), ([5, 5, 2, 2, 9], 2), ([9, 1, 1, 9, 0], 1), ([4, 4, 4, 0, 0], 4)):
        _, _, pred, _ = knn_ref.classify(np.zeros((1, 1)), r, np.array(classes, np.uint8), 5, 10)
        assert pred.tolist() == [want], classes
    assert knn_ref.vote(np.array([[0, 1, 2]]), np.array([1, 0, 1], np.uint8), 2).tolist() == [1]


def test_twin_clamps_at_zero_and_orders_by_index_at_zero():
    v = np.full((3, 4), 0.1)
    idx, dist, _, _ = knn_ref.classify(v[:1], v, np.zeros(3, np.uint8), 3, 2)
    assert (dist >= 0).all() and idx.tolist() == [[0, 1, 2]]


# ---------------------------------------------------------------- entry-point validation (host code of the built library)
def _call(lib, **kw):
    """sv_knn_classify with host addresses: every refusal is decided before anything is enqueued, so nothing is dereferenced."""
    from split_vae_amd import _lib
    a = dict(Nq=8, Nr=40, L=16, k=5, n_class=10, ldq=None, ldr=None, short=0, null=(), misalign=())
    a.update(kw)
    ldq = a["L"] if a["ldq"] is None else a["ldq"]
    ldr = a["L"] if a["ldr"] is None else a["ldr"]
    nbytes = C.c_int64(1 << 20)
    lib.sv_knn_workspace_bytes(a["Nq"], a["Nr"], a["k"], C.byref(nbytes))
    bufs = {n: np.zeros(1 << 16, np.uint8) for n in ("q", "r", "r_class", "nn_index", "nn_dist", "pred", "q_class", "acc", "ws")}
    assert nbytes.value <= 1 << 20
    bufs["ws"] = np.zeros(1 << 20, np.uint8)

    def p(n):
        if n in a["null"]:
            return None
        addr = (bufs[n].ctypes.data + 63) // 64 * 64
        return C.c_void_p(addr + (1 if n in a["misalign"] else 0))
    rc = lib.sv_knn_classify(p("q"), ldq, p("r"), ldr, p("r_class"), a["Nq"], a["Nr"], a["L"], a["k"], a["n_class"], p("nn_index"),
                             p("nn_dist"), p("pred"), p("q_class"), p("acc"), p("ws"), nbytes.value - a["short"], None)
    return _lib.STATUS.get(rc, rc)


def test_entry_point_refuses_everything_outside_the_domain(lib_built):
    from split_vae_amd import _lib
    lib = _lib.load()
    chunk = lib.sv_knn_chunk_rows()
    assert chunk > 0 and chunk % 64 == 0
    for bad in (dict(k=0), dict(k=33), dict(k=6, Nr=5), dict(L=513), dict(L=0), dict(ldq=15), dict(ldr=15), dict(n_class=1),
                dict(n_class=65), dict(Nq=0), dict(k=-1)):
        assert _call(lib, **bad) == "SV_E_UNSUPPORTED", bad
    for name in ("q", "r", "r_class", "pred", "ws"):
        assert _call(lib, null=(name,)) == "SV_E_BADARG", name
    for name in ("q", "r", "pred", "nn_index", "nn_dist", "acc", "ws"):
        assert _call(lib, misalign=(name,)) == "SV_E_BADARG", name
    assert _call(lib, short=1) == "SV_E_WORKSPACE"
    assert _call(lib, short=1, k=32, Nr=2 * chunk + 7, L=512, n_class=64) == "SV_E_WORKSPACE"       # the domain's far corner is accepted
    assert _call(lib, short=1, k=1, Nr=1, Nq=1, L=1, n_class=2, ldq=9, ldr=4, null=("nn_index", "nn_dist", "q_class", "acc")) == "SV_E_WORKSPACE"


def test_workspace_bytes_is_monotone_and_refuses_the_same_sizes(lib_built):
    from split_vae_amd import _lib
    lib = _lib.load()
    chunk = lib.sv_knn_chunk_rows()

    def ws(Nq, Nr, k):
        n = C.c_int64(-7)
        rc = lib.sv_knn_workspace_bytes(Nq, Nr, k, C.byref(n))
        return rc, n.value
    assert lib.sv_knn_workspace_bytes(8, 40, 5, None) == _lib.STATUS_BADARG
    for bad in ((0, 40, 5), (8, 40, 0), (8, 40, 33), (8, 4, 5)):
        assert ws(*bad) == (_lib.STATUS_UNSUPPORTED, -7), bad
    base = ws(65, 2 * chunk + 7, 5)
    assert base[0] == 0 and base[1] >= (65 + 2 * chunk + 7) * 4 + 65 * 3 * 5 * 8
    sizes = [(1, 32, 1), (1, 32, 32), (64, 32, 32), (65, 33, 32), (65, chunk, 32), (65, chunk + 1, 32), (130, chunk + 1, 32),
             (130, 3 * chunk, 32), (26032, 73257, 32)]
    vals = [ws(*s) for s in sizes]
    assert all(rc == 0 for rc, _ in vals)
    assert all(b[1] >= a[1] for a, b in zip(vals, vals[1:])), vals
    assert vals[5][1] > vals[4][1]                               # one row past a chunk: one more list per query
    assert ws(1 << 20, 604388, 32)[1] > 1 << 35                     # sizes past 2^31 bytes are int64 arithmetic
    assert ws(2 ** 31 - 1, 2 ** 27, 32)[1] > 2 ** 40


# ---------------------------------------------------------------- CLI surface
def test_parser_has_the_probe_flags_outside_the_reference_options():
    from split_vae_amd import main as svmain
    ap = svmain.build_parser()
    d = ap.parse_args([])
    assert d.knn_probe == 0 and d.knn_refs == 20000
    a = ap.parse_args(["--knn_probe", "5", "--knn_refs", "300"])
    assert a.knn_probe == 5 and a.knn_refs == 300
    for flag in ("--knn_probe", "--knn_refs"):
        assert flag not in [f for f, _, _ in svmain.REFERENCE_OPTIONS] and flag not in svmain.REFERENCE_SWITCHES


@pytest.mark.parametrize("flags,words", [(["--knn_probe", "3", "-no_label"], ("-no_label",)),
                                         (["--knn_probe", "33"], ("--knn_probe", "32")),
                                         (["--knn_probe", "-1"], ("--knn_probe",)),
                                         (["--knn_probe", "5", "--knn_refs", "4"], ("--knn_refs", "5"))],
                         ids=["no_label", "k33", "negative", "few_refs"])
@pytest.mark.parametrize("model_name", ["lgvae", "gmvae"])
@pytest.mark.parametrize("entry", ["main", "evaluate"])
def test_probe_flags_are_refused_before_any_device_or_data_work(monkeypatch, capsys, entry, model_name, flags, words):
    import torch
    import split_vae_amd
    from split_vae_amd import _lib, data, evaluate, main as svmain

    def boom(*a, **k):
        raise AssertionError("device / data work before the refusal")
    monkeypatch.setattr(split_vae_amd, "configure_hw_queues", boom)
    monkeypatch.setattr(torch.cuda, "is_available", boom)
    monkeypatch.setattr(torch.cuda, "_lazy_init", boom)
    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setattr(data, "get_dataset", boom)
    argv = ["--model", model_name] + flags
    with pytest.raises(SystemExit) as e:
        if entry == "main":
            svmain.main(argv)
        else:
            evaluate.main(argv + ["--weights", "nowhere.npz"])
    msg = str(e.value)
    assert all(w in msg for w in words), msg
    assert "Config:" not in capsys.readouterr().out


def test_evaluate_wants_one_of_the_two_measurements(monkeypatch):
    import split_vae_amd
    from split_vae_amd import evaluate

    def boom(*a, **k):
        raise AssertionError("device work before the refusal")
    monkeypatch.setattr(split_vae_amd, "configure_hw_queues", boom)
    with pytest.raises(SystemExit) as e:
        evaluate.main(["--weights", "nowhere.npz"])
    assert "--iw_samples" in str(e.value) and "--knn_probe" in str(e.value)
    with pytest.raises(SystemExit) as e:                         # the mixture models' IW refusal still comes first
        evaluate.main(["--weights", "nowhere.npz", "--model", "gmvae", "--iw_samples", "2", "--knn_probe", "33"])
    assert "lgvae only" in str(e.value)


# ---------------------------------------------------------------- report line
def test_report_line():
    from split_vae_amd import probe
    res = dict(acc_g=0.12344, acc_l=0.5, n_ref=20000, n_test=26032, k=5)
    assert probe.report_line(res) == "Test k-NN probe (k=5, 20000 refs): z_g acc 0.1234, z_l acc 0.5000"
    assert probe.report_line(dict(res, acc_l=None, k=3, n_ref=40)) == "Test k-NN probe (k=3, 40 refs): z_g acc 0.1234"
    assert probe.SKIPPED == "Note: --knn_probe needs labels; skipped"


def test_python_constants_mirror_the_header():
    from split_vae_amd import _lib
    assert (_lib.KNN_MAX_K, _lib.KNN_MAX_L, _lib.KNN_MAX_CLASSES) == (32, 512, 64)
