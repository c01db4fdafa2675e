"""Host side of the k-means cluster report (split_vae_amd/cluster.py, csrc/kmeans.hip): the float64 twin (tests/kmeans_ref.py) on
hand-worked values and planted lattices, a float32 emulation of the kernel's order against the derived distance bound, wrong
kernels rejected by the comparison the device tests use, the entry points' argument checks through the built library, the command
line's refusals and the report line.  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

import kmeans_ref as kr


# ---------------------------------------------------------------- the twin, by hand
def test_nmi_and_accuracy_by_hand():
    from split_vae_amd import cluster
    from split_vae_amd.gmvae import accuracy_from_counts
    a = np.array([0, 0, 1, 1, 2, 2, 2])
    same = kr.contingency(a, np.array([2, 2, 0, 0, 1, 1, 1]), 3, 3)                 # the same partition, renamed
    assert abs(kr.nmi(same) - 1.0) <= 1e-15 and kr.accuracy(same) == 1.0
    product = np.outer([2, 3, 5], [1, 4])                                           # independent: the table is a product
    assert abs(kr.nmi(product)) <= 1e-15
    t = np.array([[2, 1, 0], [0, 1, 2]])
    # H(A) = ln 2, H(B) = ln 3; the cells of 2 carry (1/3) ln((1/3) / (1/6)) each, the cells of 1 carry 0: I = (2/3) ln 2
    want = 2.0 * (2.0 / 3.0) * math.log(2.0) / (math.log(2.0) + math.log(3.0))
    assert abs(kr.nmi(t) - want) <= 1e-15 and abs(want - 0.5158037429793889) <= 1e-12
    assert kr.accuracy(t) == accuracy_from_counts(t) == 4.0 / 6.0
    for table in (same, product, t, np.array([[5, 0], [0, 0]]), np.zeros((2, 2), int)):
        assert cluster.nmi(table) == kr.nmi(table)
    assert kr.nmi(np.array([[5, 0], [0, 0]])) == 1.0 and kr.nmi(np.zeros((2, 2), int)) == 0.0
    assert np.array_equal(kr.contingency([0, 1, 1], [2, 0, 0], 2, 3), [[0, 0, 1], [2, 0, 0]])


def test_twin_on_a_line_of_points():
    x = np.array([[0.0], [1.0], [2.0], [10.0], [11.0], [12.0]], np.float32)
    a, d, dm = kr.assign(x, np.array([[1.0], [11.0]], np.float32))
    assert a.tolist() == [0, 0, 0, 1, 1, 1] and d.tolist() == [1, 0, 1, 1, 0, 1]
    np.testing.assert_allclose(kr.assign_gap(dm), [1 - 1 / 121, 1.0, 1 - 1 / 81, 1 - 1 / 81, 1.0, 1 - 1 / 121])
    a, _, dm = kr.assign(np.array([[6.0]]), np.array([[1.0], [11.0], [1.0]]))        # an exact tie: the lower index
    assert a.tolist() == [0] and kr.assign_gap(dm).tolist() == [0.0]
    f = kr.fit(x, np.array([[0.0], [1.0]], np.float32), 10)
    assert f["assign"].tolist() == [0, 0, 0, 1, 1, 1] and f["centroids"].tolist() == [[1.0], [11.0]] and f["inertia"] == 4.0
    assert f["n_iter"] == 2 and f["counts"].tolist() == [3, 3]              # t = 0: [0,1,1,1,1,1]; t = 1: [0,0,0,1,1,1]; t = 2: unchanged
    assert kr.fit(x, np.array([[0.0], [1.0]], np.float32), 1)["n_iter"] == 1
    assert kr.fit(x, np.array([[5.0], [5.0]], np.float32), 0)["counts"].tolist() == [6, 0]      # two equal centroids: the lower index takes all
    empty = kr.fit(x, np.array([[5.0], [100.0]], np.float32), 4)                     # an empty cluster keeps its centroid
    assert empty["counts"].tolist() == [6, 0] and empty["centroids"].tolist() == [[6.0], [100.0]] and empty["n_iter"] == 1
    assert kr.best_restart([3.0, 1.0, 1.0]) == 1
    assert kr.pick_gap(np.array([4.0, 1.0, 2.0, np.inf])) == 0.5 and kr.pick_gap(np.array([np.inf, 3.0])) == np.inf


def test_race_is_the_d2_rule():
    """P(argmin_i -log(u_i) / m_i = i) = m_i / sum m: over 4000 races (the step index as the counter) the frequencies follow m"""
    m = np.array([1.0, 2.0, 0.0, 5.0])
    wins = np.zeros(4)
    for k in range(1, 4001):
        keys = kr.race_keys(m, 99, 0, k)
        assert np.isinf(keys[2])
        wins[keys.argmin()] += 1
    np.testing.assert_allclose(wins / 4000, m / m.sum(), atol=0.03)
    u = kr.unit_open(kr.philox_first_word(5 ^ kr.KM_KEY, np.arange(1000), 1, 2, kr.KM_TAG))
    assert 0 < u.min() and u.max() <= 1 and abs(u.mean() - 0.5) < 0.05
    assert 0 <= kr.first_centre(5, 3, 777) < 777


# ---------------------------------------------------------------- planted lattices
@pytest.fixture(scope="module")
def twin_results():
    return {c["name"]: kr.run_case(c) for c in kr.cases()}


@pytest.mark.parametrize("shape", kr.LATTICES, ids=str)
def test_planted_lattices_are_recovered(twin_results, shape):
    case = [c for c in kr.cases() if c["name"] == "lattice-%d-%d-%d" % shape][0]
    res = twin_results[case["name"]]
    assert (res["n_iter"] <= 2).all()
    assert res["pick_gap"] >= 1e-4
    b = res["best"]
    assert kr.accuracy(kr.contingency(res["assign"][b], case["labels"], shape[2], shape[2])) == 1.0
    assert res["inertia"][b] == res["inertia"].min() and b == int(np.flatnonzero(res["inertia"] == res["inertia"].min())[0])
    if shape == (777, 130, 64):                                   # restarts that end in a worse optimum: `best` does not choose them
        assert (res["inertia"] > 2 * res["inertia"][b]).any() and b > 0
    x = case["x"]
    assert np.array_equal(x, np.rint(x)) and np.abs(x).max() <= 66


def test_trap_set_is_what_it_says(twin_results):
    t0, t6 = twin_results["trap-T0"], twin_results["trap-T6"]
    assert (t0["n_iter"] == 0).all() and (t0["counts"][0][1] == 0)             # the twice-held centroid: the lower index takes every row
    assert t6["counts"][0][3] == 0 and (t6["centroids"][0][3] == 1000.0).all()   # the far centroid: empty in every pass, and it kept its place
    assert t6["n_iter"].max() == 6 and t6["n_iter"].min() < 6                  # one restart hits T, the others converge before it
    assert len(set(t0["inertia"].tolist())) == 3
    eq = twin_results["equal-rows"]["picks"]
    assert (eq[:, 1:] == 0).all() and (eq[:, 0] > 0).all()                     # every key +inf: row 0


# ---------------------------------------------------------------- the kernel's order in float32
@pytest.mark.parametrize("N,L,K,spread", [(300, 33, 7, 1.0), (200, 128, 10, 0.5), (100, 512, 16, 0.5)], ids=str)
def test_float32_emulation_stays_within_half_the_distance_bound(N, L, K, spread):
    rng = np.random.default_rng(L)
    centres = spread * rng.standard_normal((K, L))
    x = (centres[rng.integers(0, K, N)] + rng.standard_normal((N, L))).astype(np.float32)
    c = centres.astype(np.float32)
    err = np.abs(kr.distances_f32(x, c).astype(np.float64) - kr.distances(x, c))
    bound = kr.distance_bound(x, c)
    print("worst emulated error over bound: %.3f" % (err / bound).max())
    assert (err <= 0.5 * bound).all()
    assert (kr.distances_f32(x, x[:5]) >= 0).all()
    n32 = kr.norms_f32(x)
    assert np.abs(n32 - kr.norms(x)).max() <= (L / 64 + 7) * 2.0 ** -24 * kr.norms(x).max()


# ---------------------------------------------------------------- wrong kernels
def test_the_comparison_accepts_the_twin_itself(twin_results):
    for case in kr.cases():
        assert kr.compare(kr.run_case(case), twin_results[case["name"]], case["x"], exact=False) == []


@pytest.mark.parametrize("bug", kr.BUGS)
def test_a_wrong_kernel_is_rejected(twin_results, bug):
    """Each deliberately wrong kernel, applied to the twin, fails the comparison of tests/test_gpu_kmeans.py on at least one of the
    shared cases (the big lattice only where the bug needs a chunk boundary)."""
    assert len(kr.BUGS) >= 10
    rejected = []
    for case in kr.cases():
        if case["big"] and bug != "drop_chunk_last":
            continue
        if kr.compare(kr.run_case(case, bug), twin_results[case["name"]], case["x"], exact=False):
            rejected.append(case["name"])
    print(bug, "rejected on", rejected)
    assert rejected
    if bug == "drop_chunk_last":
        assert "lattice-4099-128-10" in rejected


# ---------------------------------------------------------------- entry-point validation (host code of the built library)
def _bufs():
    return {n: np.zeros(1 << 12, np.uint8) for n in ("x", "centroids", "picks", "assign", "counts", "inertia", "n_iter", "state", "best", "a", "b")}


def _call(lib, fn="iterate", **kw):
    """sv_kmeans_seed / _iterate with host addresses: every refusal is decided before anything is enqueued, so nothing is dereferenced."""
    from split_vae_amd import _lib
    a = dict(N=40, L=16, K=5, R=3, ldx=None, iters=4, resume=0, short=0, null=(), misalign=())
    a.update(kw)
    ldx = a["L"] if a["ldx"] is None else a["ldx"]
    nbytes = C.c_int64(1 << 16)
    lib.sv_kmeans_workspace_bytes(a["N"], a["L"], a["K"], a["R"], C.byref(nbytes))
    bufs = _bufs()
    bufs["ws"] = np.zeros(64, np.uint8)

    def p(n):
        if n in a["null"]:
            return None
        addr = (bufs[n].ctypes.data + 63) // 64 * 64
        return C.c_void_p(addr + (1 if n in a["misalign"] else 0) * (4 if n == "inertia" and a.get("inertia_by_4") else 1))
    if fn == "seed":
        rc = lib.sv_kmeans_seed(p("x"), ldx, a["N"], a["L"], a["K"], a["R"], 7, p("centroids"), p("picks"), p("ws"), nbytes.value - a["short"], None)
    else:
        rc = lib.sv_kmeans_iterate(p("x"), ldx, a["N"], a["L"], a["K"], a["R"], a["iters"], a["resume"], p("centroids"), p("assign"), p("counts"),
                                   p("inertia"), p("n_iter"), p("state"), p("ws"), nbytes.value - a["short"], None)
    return _lib.STATUS.get(rc, rc)


def test_entry_points_refuse_everything_outside_the_domain(lib_built):
    from split_vae_amd import _lib
    lib = _lib.load()
    chunk = lib.sv_kmeans_chunk_rows()
    assert chunk == kr.CHUNK and chunk % 64 == 0
    domain = (dict(L=0), dict(L=513), dict(K=1), dict(K=65), dict(R=0), dict(R=17), dict(N=4), dict(N=1 << 24), dict(ldx=15), dict(N=-1), dict(K=-3))
    for fn in ("seed", "iterate"):
        for bad in domain:
            assert _call(lib, fn, **bad) == "SV_E_UNSUPPORTED", (fn, bad)
        assert _call(lib, fn, short=1) == "SV_E_WORKSPACE", fn
        assert _call(lib, fn, short=1, N=(1 << 24) - 1, L=512, K=64, R=16) == "SV_E_WORKSPACE", fn      # the domain's far corner is accepted
        assert _call(lib, fn, short=1, N=2, L=1, K=2, R=1, ldx=9) == "SV_E_WORKSPACE", fn               # and its near one
    for bad in (dict(iters=-1), dict(resume=2), dict(resume=-1)):
        assert _call(lib, "iterate", **bad) == "SV_E_UNSUPPORTED", bad
    for name in ("x", "centroids", "ws"):
        assert _call(lib, "seed", null=(name,)) == "SV_E_BADARG", name
    assert _call(lib, "seed", null=("picks",), short=1) == "SV_E_WORKSPACE"                         # picks may be NULL
    for name in ("x", "centroids", "picks", "ws"):
        assert _call(lib, "seed", misalign=(name,)) == "SV_E_BADARG", name
    for name in ("x", "centroids", "assign", "counts", "inertia", "n_iter", "state", "ws"):
        assert _call(lib, "iterate", null=(name,)) == "SV_E_BADARG", name
        assert _call(lib, "iterate", misalign=(name,)) == "SV_E_BADARG", name
    assert _call(lib, "iterate", misalign=("inertia",), inertia_by_4=True) == "SV_E_BADARG"          # fp64: 8 bytes
    # a bad argument is named before a bad size, a bad size before a short workspace
    assert _call(lib, "iterate", null=("x",), K=99, short=1) == "SV_E_BADARG" and _call(lib, "iterate", K=99, short=1) == "SV_E_UNSUPPORTED"


def test_workspace_bytes_best_and_contingency_refusals(lib_built):
    from split_vae_amd import _lib
    lib = _lib.load()

    def ws(*s):
        n = C.c_int64(-7)
        return lib.sv_kmeans_workspace_bytes(*s, C.byref(n)), n.value
    assert lib.sv_kmeans_workspace_bytes(40, 16, 5, 3, None) == _lib.STATUS_BADARG
    for bad in ((4, 16, 5, 3), (40, 0, 5, 3), (40, 513, 5, 3), (40, 16, 1, 3), (40, 16, 65, 3), (40, 16, 5, 0), (40, 16, 5, 17), (1 << 24, 16, 5, 3)):
        assert ws(*bad) == (_lib.STATUS_UNSUPPORTED, -7), bad
    sizes = [(2, 1, 2, 1), (64, 1, 2, 1), (65, 1, 2, 1), (65, 128, 2, 1), (65, 128, 10, 1), (65, 128, 10, 8), (kr.CHUNK, 128, 10, 8),
             (kr.CHUNK + 1, 128, 10, 8), (26032, 128, 10, 8), (73257, 256, 30, 8), (73257, 512, 64, 16), ((1 << 24) - 1, 512, 64, 16)]
    vals = [ws(*s) for s in sizes]
    assert all(rc == 0 and n % 256 == 0 for rc, n in vals)
    assert all(b[1] >= a[1] for a, b in zip(vals, vals[1:])), vals
    assert vals[7][1] - vals[6][1] >= 8 * 10 * 128 * 8                         # one row past a chunk: one more slab of partial sums
    assert vals[-1][1] > 1 << 34                                                # int64 arithmetic
    assert vals[8][1] >= 26032 * 4 + 13 * 8 * 10 * 128 * 8
    b = _bufs()
    p = lambda n, o=0: C.c_void_p((b[n].ctypes.data + 63) // 64 * 64 + o)     # noqa: E731
    assert lib.sv_kmeans_best(None, 3, p("best"), None) == _lib.STATUS_BADARG and lib.sv_kmeans_best(p("inertia"), 3, None, None) == _lib.STATUS_BADARG
    assert lib.sv_kmeans_best(p("inertia", 4), 3, p("best"), None) == _lib.STATUS_BADARG and lib.sv_kmeans_best(p("inertia"), 3, p("best", 2), None) == _lib.STATUS_BADARG
    assert lib.sv_kmeans_best(p("inertia"), 0, p("best"), None) == _lib.STATUS_UNSUPPORTED and lib.sv_kmeans_best(p("inertia"), 17, p("best"), None) == _lib.STATUS_UNSUPPORTED
    for null in range(3):
        args = [p("a"), p("b"), 10, 3, 4, p("counts"), None]
        args[(0, 1, 5)[null]] = None
        assert lib.sv_contingency(*args) == _lib.STATUS_BADARG
    assert lib.sv_contingency(p("a", 2), p("b"), 10, 3, 4, p("counts"), None) == _lib.STATUS_BADARG
    for N, Ka, Kb in ((0, 3, 4), (10, 0, 4), (10, 65, 4), (10, 3, 0), (10, 3, 65)):
        assert lib.sv_contingency(p("a"), p("b"), N, Ka, Kb, p("counts"), None) == _lib.STATUS_UNSUPPORTED


def test_python_constants_mirror_the_header():
    from split_vae_amd import _lib
    assert (_lib.KMEANS_MAX_L, _lib.KMEANS_MAX_K, _lib.KMEANS_MAX_R, _lib.KMEANS_MAX_N) == (512, 64, 16, (1 << 24) - 1)


# ---------------------------------------------------------------- CLI surface
def test_the_frozen_parsers_do_not_know_the_report():
    from split_vae_amd import cluster, evaluate, main as svmain, reports
    for ap in (svmain.build_parser(), evaluate.build_parser()):
        assert not any(o.startswith("--cluster") for a in ap._actions for o in a.option_strings)
    assert "clusters" not in reports.BY_NAME and not any("cluster" in e.name for e in reports.TABLE)
    ap = cluster.build_parser()
    d = ap.parse_args(["--weights", "w.npz", "--clusters", "10"])
    assert (d.clusters, d.cluster_images, d.cluster_restarts, d.cluster_iters, d.knn_probe, d.global_latent_dims) == (10, None, 8, 100, 0, 128)
    assert cluster.build_parser() is not ap
    with pytest.raises(SystemExit):
        ap.parse_args(["--weights", "w.npz"])                     # --clusters is required


@pytest.mark.parametrize("flags,words", [(["--clusters", "1"], ("--clusters", "2 <= K <= 64")),
                                         (["--clusters", "65"], ("--clusters", "65")),
                                         (["--clusters", "10", "--cluster_images", "9"], ("--cluster_images", "K = 10")),
                                         (["--clusters", "10", "--cluster_images", str(1 << 24)], ("--cluster_images", "16777215")),
                                         (["--clusters", "10", "--cluster_restarts", "0"], ("--cluster_restarts", "1 <= R <= 16")),
                                         (["--clusters", "10", "--cluster_restarts", "17"], ("--cluster_restarts", "17")),
                                         (["--clusters", "10", "--cluster_iters", "-1"], ("--cluster_iters", "T >= 0")),
                                         (["--clusters", "10", "--global_latent_dims", "513"], ("512 dimensions",)),
                                         (["--clusters", "10", "--knn_probe", "5"], ("--knn_probe", "split_vae_amd.evaluate")),
                                         (["--clusters", "10", "--latent_info", "100", "--iw_samples", "4"], ("--iw_samples, --latent_info", "split_vae_amd.evaluate")),
                                         (["--clusters", "10", "--augmentation", "nope"], ("--augmentation",))],
                         ids=["k1", "k65", "few_images", "many_images", "r0", "r17", "negative_iters", "wide_latent", "table_flag", "two_table_flags",
                              "augmentation"])
@pytest.mark.parametrize("model_name", ["lgvae", "gmvae"])
def test_cli_refuses_before_any_device_or_data_work(monkeypatch, capsys, model_name, flags, words):
    import torch
    import split_vae_amd
    from split_vae_amd import _lib, cluster, data

    def boom(*a, **k):
        raise AssertionError("device / data work before the refusal")
    monkeypatch.setattr(split_vae_amd, "configure_hw_queues", boom)
    monkeypatch.setattr(torch.cuda, "is_available", boom)
    monkeypatch.setattr(torch.cuda, "_lazy_init", boom)
    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setattr(data, "get_dataset", boom)
    with pytest.raises(SystemExit) as e:
        cluster.main(["--model", model_name, "--weights", "nowhere.npz"] + flags)
    msg = str(e.value)
    assert all(w in msg for w in words), msg
    assert capsys.readouterr().out == ""


def test_gmvae_ignores_the_local_width_it_does_not_have(monkeypatch):
    import split_vae_amd
    from split_vae_amd import cluster

    class Reached(Exception):
        pass

    def reached(*a, **k):
        raise Reached()
    monkeypatch.setattr(split_vae_amd, "configure_hw_queues", reached)
    with pytest.raises(Reached):                                  # every check passed: the next thing is the device
        cluster.main(["--model", "gmvae", "--weights", "nowhere.npz", "--clusters", "10", "--local_latent_dims", "9999"])
    with pytest.raises(SystemExit):
        cluster.main(["--model", "lgvae", "--weights", "nowhere.npz", "--clusters", "10", "--local_latent_dims", "9999"])


# ---------------------------------------------------------------- report line
def test_report_line():
    from split_vae_amd import cluster
    res = dict(k=10, n_images=26032, restarts=8, labelled=True, acc_g=0.61234, nmi_g=0.5, inertia_g=12.34567, n_iter_g=37, empty_g=0,
               acc_l=0.19, nmi_l=0.01234, inertia_l=99.5, n_iter_l=50, empty_l=1, nmi_gl=0.0021)
    assert cluster.report_line(res) == ("Test k-means (10 clusters, 26032 images, 8 restarts): z_g acc 0.6123, NMI 0.5000, inertia/image 12.3457 "
                                        "(37 iterations, 0 empty); z_l acc 0.1900, NMI 0.0123, inertia/image 99.5000; "
                                        "NMI(z_g clusters; z_l clusters) 0.0021")
    bare = dict(res, labelled=False, acc_g=None, nmi_g=None, acc_l=None, nmi_l=None)
    assert cluster.report_line(bare) == ("Test k-means (10 clusters, 26032 images, 8 restarts): z_g inertia/image 12.3457 (37 iterations, 0 empty); "
                                         "z_l inertia/image 99.5000; NMI(z_g clusters; z_l clusters) 0.0021")
    gm = dict(res, acc_l=None, nmi_l=None, inertia_l=None, n_iter_l=None, empty_l=None, nmi_gl=None)
    assert cluster.report_line(gm) == "Test k-means (10 clusters, 26032 images, 8 restarts): z_g acc 0.6123, NMI 0.5000, inertia/image 12.3457 (37 iterations, 0 empty)"
    assert cluster.UNLABELLED.startswith("Note: ")
