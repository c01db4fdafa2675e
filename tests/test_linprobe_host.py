"""Host side of the linear label probe (split_vae_amd/linear_probe.py, csrc/linprobe.hip): the float64 twin (tests/linprobe_ref.py)
checked against itself -- monotone loss, finite differences, Boehning's bound --, its float32 emulation of the kernels' order
against the derived bounds, wrong kernels rejected by the comparison the device tests use, the margin cap of the predict cases,
the entry points' argument checks through the built library, the command line's refusals and the report line.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import linprobe_ref as lr


@pytest.fixture(scope="module")
def twin_results():
    return {c["name"]: lr.run_case(c) for c in lr.cases()}


@pytest.fixture(scope="module")
def case_bounds(twin_results):
    out = {}
    for c in lr.cases():
        if c["kind"] == "fit":
            P, B = lr.case_P(c)
            out[c["name"]] = lr.fit_bounds(c["x"], c["y"], c["C"], P, B, c["l2"], twin_results[c["name"]])
    return out


# ---------------------------------------------------------------- the twin against itself
def test_loss_is_monotone_on_the_device_tests_inputs(twin_results):
    seen = 0
    for c in lr.cases():
        if c["kind"] == "fit":
            loss = twin_results[c["name"]]["loss"]
            assert loss.shape == (c["T"] + 1,) and (np.diff(loss) <= 0).all(), c["name"]
            seen += 1
    assert seen == len(lr.GAUSS_CASES) * len(lr.GAUSS_T)


def _objective(x, y, C, W, l2):
    z = lr.design(x) @ W
    m = z.max(axis=1)
    lse = m + np.log(np.exp(z - m[:, None]).sum(axis=1))
    valid = y < C
    return float(np.where(valid, lse - z[np.arange(len(y)), np.where(valid, y, 0)], 0.0).sum() / len(y) + 0.5 * l2 * (W[:-1] ** 2).sum())


def test_gradient_against_finite_differences():
    """G of the twin = the central difference of the objective, at a W whose entries are fp32 numbers (W32 = W)"""
    x, y = lr.gauss(200, 7, 3, seed=2)
    y = y.copy()
    y[3] = 9
    rng = np.random.default_rng(0)
    W = rng.standard_normal((8, 3)).astype(np.float32).astype(np.float64)
    ev = lr.evaluate(x, y, 3, W, 1e-2)
    assert abs(ev["loss"] - _objective(x, y, 3, W, 1e-2)) <= 1e-12
    h = 1e-6
    for i in range(8):
        for c in range(3):
            d = np.zeros_like(W)
            d[i, c] = h
            fd = (_objective(x, y, 3, W + d, 1e-2) - _objective(x, y, 3, W - d, 1e-2)) / (2 * h)
            assert abs(fd - ev["G"][i, c]) <= 1e-8, (i, c)
    assert ev["gmax"] == np.abs(ev["G"]).max()


def test_boehning_bound_on_a_small_case():
    """The Hessian of the objective over all (L+1) C weights is at most B (x) I: the smallest eigenvalue of the difference is >= 0"""
    x, y = lr.gauss(120, 4, 3, seed=4)
    l2 = 1e-3
    a = lr.design(x)
    P, B = lr.make_P(lr.gram(x), 120, l2)
    assert np.allclose(P @ B, np.eye(5), atol=1e-10)
    rng = np.random.default_rng(1)
    for _ in range(3):
        W = rng.standard_normal((5, 3)).astype(np.float32).astype(np.float64)
        p = lr.evaluate(x, y, 3, W, l2)["p"]
        Hs = np.zeros((15, 15))                                    # index (c, f)
        for i in range(120):
            Hs += np.kron(np.diag(p[i]) - np.outer(p[i], p[i]), np.outer(a[i], a[i])) / 120
        d = np.full(5, l2)
        d[-1] = 0.0
        Hs += np.kron(np.eye(3), np.diag(d))
        assert np.linalg.eigvalsh(np.kron(np.eye(3), B) - Hs).min() >= -1e-12
    with pytest.raises(np.linalg.LinAlgError):
        lr.make_P(np.ones((3, 3)), 10, 0.0)


def test_fixed_orders_by_hand():
    assert lr.strided_sum(np.arange(600.0)) == 599 * 600 / 2
    big = np.zeros(512)
    big[0], big[256], big[1] = 2.0 ** 53, 1.0, 1.0                 # thread 0 sees 2^53 + 1 = 2^53, then + thread 1's 1: 2^53 again
    assert lr.strided_sum(big) == 2.0 ** 53
    assert lr.tile_sums(np.ones(130)).tolist() == [64.0, 64.0, 2.0]
    x, _ = lr.fold_trap()
    S = lr.gram(x)
    assert S[0, 1] == 2.0 ** 53 == S[1, 0] and lr.gram(x, bug="fold_reversed")[0, 1] == 2.0 ** 53 + 2
    W = np.array([[1.0, 2.0], [3.0, 4.0]])
    assert np.array_equal(lr.step(W, np.eye(2), np.ones((2, 2))), W - 1)


# ---------------------------------------------------------------- the kernels' order in float32
@pytest.mark.parametrize("name", [c["name"] for c in lr.cases() if c["kind"] in ("fit", "predict")])
def test_float32_emulation_stays_within_half_of_each_bound(twin_results, case_bounds, name):
    case = [c for c in lr.cases() if c["name"] == name][0]
    want = twin_results[name]
    em = lr.run_case(case, emulate=True)
    if case["kind"] == "fit":
        b = case_bounds[name]
        for n in ("W", "loss", "gmax", "G"):
            ratio = (np.abs(em[n] - want[n]) / b[n]).max()
            print("%s %s: emulated error / bound %.3g" % (name, n, ratio))
            assert ratio <= 0.5
    else:
        ex = lr.predict_excluded(case, want)
        assert np.array_equal(em["pred"][~ex], want["pred"][~ex])
        assert abs(em["loss"] - want["loss"]) <= 0.5 * lr.predict_loss_bound(case, want)


def test_float32_emulation_of_the_gram_chain():
    x, _ = lr.gauss(700, 21, 3)
    a = np.abs(lr.design(x))
    err = np.abs(lr.gram(x, emulate=True) - lr.gram(x))
    assert (err <= 0.5 * (lr.CHUNK + 1) * lr.U * (a.T @ a)).all() and err.max() > 0


def test_bounds_grow_at_most_linearly_in_T(twin_results, case_bounds):
    for name, N, L, Cc, l2 in lr.GAUSS_CASES:
        c = [c for c in lr.cases() if c["name"] == "%s-T50" % name][0]
        P, B = lr.case_P(c)
        betas = [lr.pass_bounds(c["x"], c["y"], c["C"], p, p["W"], P, B, l2)["beta"] for p in twin_results[c["name"]]["passes"]]
        assert abs(case_bounds[c["name"]]["EB"] - sum(betas[:-1])) <= 1e-12 * sum(betas) and case_bounds[c["name"]]["EB"] <= 50 * max(betas)


# ---------------------------------------------------------------- the margin cap
@pytest.mark.parametrize("name", [c["name"] for c in lr.cases() if c["kind"] == "predict"])
def test_predict_cases_exclude_at_most_one_percent(twin_results, name):
    case = [c for c in lr.cases() if c["name"] == name][0]
    share = lr.predict_excluded(case, twin_results[name]).mean()
    print(name, "excluded share", share)
    assert share <= lr.MARGIN_CAP


# ---------------------------------------------------------------- wrong kernels
def test_the_comparison_accepts_the_twin_itself(twin_results, case_bounds):
    for case in lr.cases():
        assert lr.compare(case, lr.run_case(case), twin_results[case["name"]], case_bounds.get(case["name"])) == []


@pytest.mark.parametrize("bug", lr.BUGS)
def test_a_wrong_kernel_is_rejected(twin_results, case_bounds, bug):
    """Each deliberately wrong kernel, applied to the twin, fails the comparison of tests/test_gpu_linprobe.py on at least one of
    the shared cases."""
    assert len(lr.BUGS) >= 10
    rejected = [c["name"] for c in lr.cases() if lr.compare(c, lr.run_case(c, bug), twin_results[c["name"]], case_bounds.get(c["name"]))]
    print(bug, "rejected on", rejected)
    assert rejected
    must = dict(fold_reversed="g-fold-trap", tie_high="p-ties", bias_regularised="f-600-35-8-w", no_max_shift="n-700-130-3-big",
                drop_last_col="n-700-130-3-predict", drop_chunk_last="g-700-33")
    if bug in must:
        assert must[bug] in rejected


# ---------------------------------------------------------------- entry-point validation (host code of the built library)
NAMES = ("x", "y", "P", "W", "loss", "gmax", "grad", "state", "S", "pred", "acc", "ws")


def _call(lib, fn="fit", **kw):
    """sv_linprobe_* with host addresses: every refusal is decided before anything is enqueued, so nothing is dereferenced."""
    from split_vae_amd import _lib
    a = dict(N=40, L=16, C=5, ldx=None, iters=4, resume=0, l2=1e-3, short=0, null=(), misalign=(), by=1)
    a.update(kw)
    ldx = a["L"] if a["ldx"] is None else a["ldx"]
    nbytes = C.c_int64(1 << 16)
    lib.sv_linprobe_workspace_bytes(a["N"], a["L"], a["C"] if fn != "gram" else 2, C.byref(nbytes))
    bufs = {n: np.zeros(1 << 10, np.uint8) for n in NAMES}

    def p(n):
        if n in a["null"]:
            return None
        return C.c_void_p((bufs[n].ctypes.data + 63) // 64 * 64 + (a["by"] if n in a["misalign"] else 0))
    if fn == "gram":
        rc = lib.sv_linprobe_gram(p("x"), ldx, a["N"], a["L"], p("S"), p("ws"), nbytes.value - a["short"], None)
    elif fn == "fit":
        rc = lib.sv_linprobe_fit(p("x"), ldx, p("y"), a["N"], a["L"], a["C"], p("P"), a["l2"], a["iters"], a["resume"], p("W"), p("loss"), p("gmax"),
                                 p("grad"), p("state"), p("ws"), nbytes.value - a["short"], None)
    else:
        rc = lib.sv_linprobe_predict(p("x"), ldx, a["N"], a["L"], a["C"], p("W"), p("pred"), p("y"), p("acc"), p("loss"), p("ws"),
                                     nbytes.value - a["short"], None)
    return _lib.STATUS.get(rc, rc)


def test_entry_points_refuse_everything_outside_the_domain(lib_built):
    from split_vae_amd import _lib
    lib = _lib.load()
    chunk = lib.sv_linprobe_chunk_rows()
    assert chunk == lr.CHUNK and chunk % 64 == 0
    domain = (dict(L=0), dict(L=513), dict(N=0), dict(N=1 << 24), dict(N=-1), dict(ldx=15), dict(L=-2))
    classes = (dict(C=1), dict(C=65), dict(C=-3))
    for fn in ("gram", "fit", "predict"):
        for bad in domain + (classes if fn != "gram" else ()):
            assert _call(lib, fn, **bad) == "SV_E_UNSUPPORTED", (fn, bad)
        assert _call(lib, fn, short=1) == "SV_E_WORKSPACE", fn
        assert _call(lib, fn, short=1, N=(1 << 24) - 1, L=512, C=64) == "SV_E_WORKSPACE", fn      # the domain's far corner is accepted
        assert _call(lib, fn, short=1, N=1, L=1, C=2, ldx=9) == "SV_E_WORKSPACE", fn               # and its near one
    for bad in (dict(iters=-1), dict(resume=2), dict(resume=-1), dict(l2=-1e-9), dict(l2=float("inf")), dict(l2=float("nan"))):
        assert _call(lib, "fit", **bad) == "SV_E_UNSUPPORTED", bad
    assert _call(lib, "fit", l2=0.0, iters=0, short=1) == "SV_E_WORKSPACE"
    for name in ("x", "S", "ws"):
        assert _call(lib, "gram", null=(name,)) == "SV_E_BADARG", name
        assert _call(lib, "gram", misalign=(name,)) == "SV_E_BADARG", name
    assert _call(lib, "gram", misalign=("S",), by=4) == "SV_E_BADARG"                               # fp64: 8 bytes
    for name in ("x", "y", "P", "W", "loss", "gmax", "state", "ws"):
        assert _call(lib, "fit", null=(name,)) == "SV_E_BADARG", name
    assert _call(lib, "fit", null=("grad",), short=1) == "SV_E_WORKSPACE"                           # grad may be NULL
    for name in ("x", "P", "W", "loss", "gmax", "grad", "state", "ws"):
        assert _call(lib, "fit", misalign=(name,)) == "SV_E_BADARG", name
    for name in ("P", "W", "loss", "gmax", "grad"):
        assert _call(lib, "fit", misalign=(name,), by=4) == "SV_E_BADARG", name
    assert _call(lib, "fit", misalign=("ws",), by=8) == "SV_E_BADARG"                               # workspace: 16 bytes
    for name in ("x", "W", "pred", "ws"):
        assert _call(lib, "predict", null=(name,)) == "SV_E_BADARG", name
    for name in ("x", "W", "pred", "acc", "loss", "ws"):
        assert _call(lib, "predict", misalign=(name,)) == "SV_E_BADARG", name
    assert _call(lib, "predict", misalign=("acc",), by=4) == "SV_E_BADARG"
    for ok in (("acc",), ("loss",), ("y", "loss"), ("y", "loss", "acc")):
        assert _call(lib, "predict", null=ok, short=1) == "SV_E_WORKSPACE", ok                      # optional pointers
    assert _call(lib, "predict", null=("y",)) == "SV_E_BADARG"                                      # a loss needs the classes
    # a bad argument is named before a bad size, a bad size before a short workspace
    assert _call(lib, "fit", null=("x",), C=99, short=1) == "SV_E_BADARG" and _call(lib, "fit", C=99, short=1) == "SV_E_UNSUPPORTED"


def test_workspace_bytes_are_monotone(lib_built):
    from split_vae_amd import _lib
    lib = _lib.load()

    def ws(*s):
        n = C.c_int64(-7)
        return lib.sv_linprobe_workspace_bytes(*s, C.byref(n)), n.value
    assert lib.sv_linprobe_workspace_bytes(40, 16, 5, None) == _lib.STATUS_BADARG
    for bad in ((0, 16, 5), (40, 0, 5), (40, 513, 5), (40, 16, 1), (40, 16, 65), (1 << 24, 16, 5)):
        assert ws(*bad) == (_lib.STATUS_UNSUPPORTED, -7), bad
    sizes = [(1, 1, 2), (64, 1, 2), (65, 1, 2), (65, 128, 2), (65, 128, 10), (65, 128, 17), (lr.CHUNK, 128, 17), (lr.CHUNK + 1, 128, 17),
             (20000, 128, 17), (73257, 256, 17), (73257, 512, 64), ((1 << 24) - 1, 512, 64)]
    vals = [ws(*s) for s in sizes]
    assert all(rc == 0 and n % 256 == 0 for rc, n in vals)
    assert all(b[1] >= a[1] for a, b in zip(vals, vals[1:])), vals
    assert vals[7][1] - vals[6][1] >= 129 * 144 * 4                             # one row past a chunk: one more slab of partials
    assert vals[-1][1] > 1 << 34                                                # int64 arithmetic
    assert vals[8][1] >= 20000 * 32 * 4 + 40 * 129 * 144 * 4
    assert ws(40, 16, 2)[1] <= ws(40, 16, 5)[1]                                 # the Gram pass asks with C = 2


def test_python_constants_mirror_the_header():
    from split_vae_amd import _lib
    assert (_lib.LINPROBE_MAX_L, _lib.LINPROBE_MAX_C, _lib.LINPROBE_MAX_N) == (512, 64, (1 << 24) - 1)


def test_step_matrix_refuses_a_singular_bound():
    from split_vae_amd import linear_probe as lp
    x, _ = lr.gauss(100, 6, 3)
    S = lr.gram(x)
    assert np.array_equal(lp.step_matrix(S, 100, 1e-3), lr.make_P(S, 100, 1e-3)[0])
    xc = x.copy()
    xc[:, 2] = 1.0                                                # a constant feature column: collinear with the bias
    with pytest.raises(ValueError, match="positive definite"):
        lp.step_matrix(lr.gram(xc), 100, 0.0)
    lp.step_matrix(lr.gram(xc), 100, 1e-3)


# ---------------------------------------------------------------- CLI surface
def test_the_frozen_parsers_do_not_know_the_report():
    import sys
    from split_vae_amd import main as svmain
    before = svmain.build_parser().format_help()
    sys.modules.pop("split_vae_amd.linear_probe", None)
    from split_vae_amd import evaluate, linear_probe, reports
    assert svmain.build_parser().format_help() == before           # importing the module changes nothing in main's parser
    for ap in (svmain.build_parser(), evaluate.build_parser()):
        assert not any(o.startswith("--probe_") for a in ap._actions for o in a.option_strings)
    assert not any("linear" in e.name or e.name.startswith("probe_") for e in reports.TABLE)
    ap = linear_probe.build_parser()
    assert svmain.build_parser().format_help() == before
    d = ap.parse_args(["--weights", "w.npz"])
    assert (d.probe_refs, d.probe_iters, d.probe_l2, d.knn_probe, d.global_latent_dims) == (20000, 100, 1e-3, 0, 128)
    assert linear_probe.build_parser() is not ap
    with pytest.raises(SystemExit):
        ap.parse_args([])                                         # --weights is required


@pytest.mark.parametrize("flags,words", [(["-no_label"], ("-no_label",)),
                                         (["--probe_refs", "0"], ("--probe_refs", "1 <= N")),
                                         (["--probe_refs", str(1 << 24)], ("--probe_refs", "16777215")),
                                         (["--probe_iters", "-1"], ("--probe_iters", "T >= 0")),
                                         (["--probe_l2", "-0.5"], ("--probe_l2", "-0.5")),
                                         (["--probe_l2", "inf"], ("--probe_l2",)),
                                         (["--probe_l2", "nan"], ("--probe_l2",)),
                                         (["--global_latent_dims", "513"], ("512 dimensions",)),
                                         (["--knn_probe", "5"], ("--knn_probe", "split_vae_amd.evaluate")),
                                         (["--latent_info", "100", "--iw_samples", "4"], ("--iw_samples, --latent_info", "split_vae_amd.evaluate")),
                                         (["--augmentation", "nope"], ("--augmentation",))],
                         ids=["no_label", "refs0", "many_refs", "negative_iters", "negative_l2", "inf_l2", "nan_l2", "wide_latent", "table_flag",
                              "two_table_flags", "augmentation"])
@pytest.mark.parametrize("model_name", ["lgvae", "gmvae"])
def test_cli_refuses_before_any_device_or_data_work(monkeypatch, capsys, model_name, flags, words):
    import torch
    import split_vae_amd
    from split_vae_amd import _lib, data, linear_probe

    def boom(*a, **k):
        raise AssertionError("device / data work before the refusal")
    monkeypatch.setattr(split_vae_amd, "configure_hw_queues", boom)
    monkeypatch.setattr(torch.cuda, "is_available", boom)
    monkeypatch.setattr(torch.cuda, "_lazy_init", boom)
    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setattr(data, "get_dataset", boom)
    with pytest.raises(SystemExit) as e:
        linear_probe.main(["--model", model_name, "--weights", "nowhere.npz"] + flags)
    msg = str(e.value)
    assert all(w in msg for w in words), msg
    assert capsys.readouterr().out == ""


def test_gmvae_ignores_the_local_width_it_does_not_have(monkeypatch):
    import split_vae_amd
    from split_vae_amd import linear_probe

    class Reached(Exception):
        pass

    def reached(*a, **k):
        raise Reached()
    monkeypatch.setattr(split_vae_amd, "configure_hw_queues", reached)
    with pytest.raises(Reached):                                  # every check passed: the next thing is the device
        linear_probe.main(["--model", "gmvae", "--weights", "nowhere.npz", "--local_latent_dims", "9999"])
    with pytest.raises(SystemExit):
        linear_probe.main(["--model", "lgvae", "--weights", "nowhere.npz", "--local_latent_dims", "9999"])


# ---------------------------------------------------------------- report line
def test_report_line():
    from split_vae_amd import linear_probe as lp
    res = dict(n_ref=20000, n_test=26032, iters=100, l2=1e-3, acc_g=0.61234, train_acc_g=0.7, loss_g=1.23456, test_loss_g=1.5, gmax_g=3.21e-4,
               acc_l=0.19, train_acc_l=0.2, loss_l=2.25, test_loss_l=2.3, gmax_l=1e-5)
    assert lp.report_line(res) == ("Test linear probe (20000 refs, 100 steps, l2 0.001): z_g acc 0.6123, train acc 0.7000, loss 1.2346 "
                                   "(|grad| 3.21e-04); z_l acc 0.1900, train acc 0.2000, loss 2.2500 (|grad| 1.00e-05)")
    gm = dict(res, acc_l=None, train_acc_l=None, loss_l=None, test_loss_l=None, gmax_l=None)
    assert lp.report_line(gm) == "Test linear probe (20000 refs, 100 steps, l2 0.001): z_g acc 0.6123, train acc 0.7000, loss 1.2346 (|grad| 3.21e-04)"
    assert lp.NO_LABELS.startswith("Note: ")
