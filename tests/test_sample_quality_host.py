"""CPU: the sample-quality report's float64 twins (tests/prdc_ref.py) against independent restatements, the mutants the GPU tests'
comparisons must reject, the condition of the Gaussian cases, the argument checks of sv_prdc_* that run before any launch, and the host
side of split_vae_amd.sample_quality (the Frechet distance against closed forms, the figures, flags, parser, refusals, the line).  No
device work."""
import ctypes as C

import numpy as np
import pytest

import prdc_ref as ref


@pytest.fixture(scope="module")
def lib(lib_built):
    from split_vae_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def chunk(lib):
    c = lib.sv_prdc_chunk_rows()
    assert c >= 64 and c % 64 == 0
    return c


@pytest.fixture(scope="module")
def count_cases(chunk):
    cases = []
    for n, (Nq, Nr, L, _, _, _) in enumerate(ref.count_shapes(chunk)):
        c = ref.count_case(Nq, Nr, L, 200 + n)
        c["want"] = ref.count(c["Q"], c["R"], c["rad"])
        cases.append(c)
    return cases


@pytest.fixture(scope="module")
def radius_cases(chunk):
    cases = []
    for n, (N, L, k, _, _) in enumerate(ref.radius_shapes(chunk)):
        X = ref.radius_case(N, L, 300 + n)
        cases.append(dict(X=X, k=k, want=ref.radius(X, k)))
    return cases


# ---------------------------------------------------------------- the twins
def test_count_twin_equals_the_loop_restatement_on_lattices_with_ties(count_cases):
    hits = ties = 0
    for c in count_cases:
        assert ref.counts_equal(c["want"], ref.count_by_loops(c["Q"], c["R"], c["rad"]))
        d = ref.distances(c["Q"], c["R"])
        assert np.abs(c["R"]).max() <= 4 and np.abs(c["Q"]).max() <= 12 and (c["Q"] == np.rint(c["Q"])).all() and (c["rad"] == np.rint(c["rad"])).all()
        assert d.max() < 2 ** 24                                           # every norm, dot product and distance is exact in fp32
        hits += int((d == c["rad"][None, :].astype(np.float64)).sum())
        ties += int(((d == d.min(axis=1, keepdims=True)).sum(axis=1) > 1).sum())
    assert hits > 1000 and ties > 100                                      # distances equal to a radius and tied minima are frequent
    spread = np.concatenate([c["want"][0] for c in count_cases])
    assert spread.min() == 0 and spread.max() > 1000 and len(np.unique(spread)) > 50


def test_radius_twin_equals_the_argsort_restatement_on_lattices_with_ties(radius_cases):
    zero = 0
    for c in radius_cases:
        assert ref.exact(c["want"], ref.radius_by_argsort(c["X"], c["k"]))
        assert ref.distances(c["X"], c["X"]).max() < 2 ** 24
        zero += int((c["want"] == 0).sum())
    assert zero > 100                                                      # duplicates: radii of exactly 0


def test_lattice_cases_hold_the_named_situations(count_cases, radius_cases, chunk):
    shapes = ref.count_shapes(chunk)
    assert [s[:3] for s in shapes] == [(1, 1, 1), (63, 2, 3), (64, 64, 31), (65, 65, 32), (130, chunk - 1, 33), (64, chunk, 128),
                                       (65, chunk + 1, 256), (130, 2 * chunk + 3, 33), (1, 65, 512)]
    assert any(s[3] for s in shapes) and any(s[4] for s in shapes) and any(s[5] for s in shapes)
    for c in count_cases[2:8]:
        d = ref.distances(c["Q"], c["R"])
        cnt, dmin, imin = c["want"]
        Nr = c["R"].shape[0]
        assert c["rad"][0] == 0 and d[0, 0] == 0 and (c["Q"][0] == c["R"][0]).all()      # radius 0, its duplicate a query: 0 <= 0 counts
        assert ref.count(c["Q"], c["R"], c["rad"], "lt")[0][0] < cnt[0]
        assert (d == c["rad"][None, :].astype(np.float64)).any()              # a distance exactly equal to a radius
        assert cnt[1] == 0                                                     # a query with count 0
        a, b = Nr // 3, Nr - 1
        assert dmin[2] == 0 and d[2, a] == 0 and d[2, b] == 0 and imin[2] <= a < b      # a tie of the minimum: the lowest index wins
    rs = ref.radius_shapes(chunk)
    assert {(s[0], s[2]) for s in rs} == {(N, k) for k in (1, 5, 31) for N in (k + 1, 64, 65, chunk + 1)}
    assert {s[1] for s in rs} == {3, 33, 256} and any(s[3] for s in rs) and any(s[4] for s in rs)
    for c, s in zip(radius_cases, rs):
        X, N = c["X"], s[0]
        if N >= 3:
            assert (X[0] == X[N // 2]).all() and (X[N - 1] == X[N // 2]).all()     # duplicates at a lower and at a higher index
            assert c["want"][N // 2] == 0 or c["k"] > 2
    assert any(s[0] == s[2] + 1 for s in rs)                                   # N = k + 1: every other row is a neighbour


@pytest.mark.parametrize("mutant", ref.COUNT_MUTANTS)
def test_count_mutants_are_rejected_by_the_lattice_comparison(count_cases, mutant):
    failed = [n for n, c in enumerate(count_cases) if not ref.counts_equal(ref.count(c["Q"], c["R"], c["rad"], mutant), c["want"])]
    assert len(failed) >= 3, (mutant, failed)


@pytest.mark.parametrize("mutant", ref.RADIUS_MUTANTS)
def test_radius_mutants_are_rejected_by_the_lattice_comparison(radius_cases, mutant):
    failed = [n for n, c in enumerate(radius_cases) if not ref.exact(ref.radius(c["X"], c["k"], mutant), c["want"])]
    assert len(failed) >= 3, (mutant, failed)


def test_at_least_ten_mutants():
    assert len(set(ref.COUNT_MUTANTS + ref.RADIUS_MUTANTS + ref.FIGURE_MUTANTS)) >= 10


@pytest.mark.parametrize("shape", ref.GAUSS_SHAPES)
def test_gaussian_cases_are_well_conditioned(shape):
    """on the twin alone: the bracket decides all but 2 % of the queries, and the share of queries inside some ball is neither 0 nor 1"""
    c = ref.gaussian_case(*shape)
    lo, hi = ref.count_bracket(c["Q"], c["R"], c["rad"])
    cnt = ref.count(c["Q"], c["R"], c["rad"])[0]
    share, positive = ref.undecided_share(lo, hi), float(np.mean(cnt > 0))
    print("gaussian %s: undecided share %.4f, positive share %.3f" % (shape, share, positive))
    assert share <= ref.UNDECIDED_CAP
    assert ref.POSITIVE_SHARE[0] < positive < ref.POSITIVE_SHARE[1]
    assert ((lo <= cnt) & (cnt <= hi)).all()
    for mutant in ("rad_of_query", "no_norm_r", "plain_vs_squared"):             # the bracket comparison rejects what can show on such data
        assert not ref.counts_in_bracket(ref.count(c["Q"], c["R"], c["rad"], mutant)[0], lo, hi, cnt), mutant


# ---------------------------------------------------------------- the Frechet distance and the figures
def _gram(X):
    A = np.concatenate([np.asarray(X, np.float64), np.ones((len(X), 1))], axis=1)
    return A.T @ A


def test_frechet_against_closed_forms():
    from split_vae_amd import sample_quality as sq
    rng = np.random.default_rng(5)
    X = rng.standard_normal((400, 8)) * rng.uniform(0.5, 2.0, size=8) + rng.standard_normal(8)
    mx, Cx = sq.moments(_gram(X), 400)
    m2, C2 = ref.moments(X)
    assert np.abs(mx - m2).max() <= 1e-12 and np.abs(Cx - C2).max() <= 1e-11      # divisor N
    tr = 2 * np.trace(Cx)
    assert abs(sq.frechet(mx, Cx, mx, Cx)) <= 1e-9 * tr                          # identical sets
    shift = rng.standard_normal(8)
    my, Cy = sq.moments(_gram(X + shift), 400)
    assert abs(sq.frechet(mx, Cx, my, Cy) - float(shift @ shift)) <= 1e-9 * tr    # a pure mean shift
    a, b = rng.uniform(0.1, 3.0, size=8), rng.uniform(0.1, 3.0, size=8)
    want = float(((np.sqrt(a) - np.sqrt(b)) ** 2).sum())
    assert abs(sq.frechet(mx, np.diag(a), mx, np.diag(b)) - want) <= 1e-9 * (a.sum() + b.sum())     # diagonal covariances
    Y = rng.standard_normal((300, 8)) @ rng.standard_normal((8, 8)) + 0.3
    my, Cy = sq.moments(_gram(Y), 300)
    got, twin = sq.frechet(mx, Cx, my, Cy), ref.frechet(mx, Cx, *ref.moments(Y))
    assert got > 0 and abs(got - twin) <= 1e-9 * (np.trace(Cx) + np.trace(Cy))
    assert abs(sq.frechet(my, Cy, mx, Cx) - got) <= 1e-9 * (np.trace(Cx) + np.trace(Cy))       # symmetric
    low = np.concatenate([X[:, :3], np.zeros((400, 5))], axis=1)                  # a collapsed block: rank 3, no NaN from a negative eigenvalue
    ml, Cl = sq.moments(_gram(low), 400)
    assert np.isfinite(sq.frechet(ml, Cl, mx, Cx)) and abs(sq.frechet(ml, Cl, ml, Cl)) <= 1e-6 * tr


def test_figure_arithmetic_and_its_mutants():
    from split_vae_amd import sample_quality as sq
    rng = np.random.default_rng(9)
    N, k = 57, 5
    cf, cr = rng.integers(0, 4, size=N) * rng.integers(0, 2, size=N), rng.integers(0, 3, size=N)
    dm, rx, ry = rng.uniform(0, 2, size=N), rng.uniform(0, 2, size=N), rng.uniform(0, 2, size=N)
    dm[:5] = rx[:5]                                                          # dmin == rad counts as covered
    got, want = sq.figures(cf, cr, dm, rx, k), ref.figures(cf, cr, dm, rx, ry, k)
    assert set(got) == set(want) == {"precision", "recall", "density", "coverage"}
    for key in want:
        assert abs(got[key] - want[key]) <= 1e-12, key
    assert want["coverage"] >= 5 / N and 0 < want["precision"] < 1 and want["precision"] != want["recall"]
    for mutant in ref.FIGURE_MUTANTS:
        bad = ref.figures(cf, cr, dm, rx, ry, k, mutant)
        assert any(abs(bad[key] - got[key]) > 1e-6 for key in got), mutant
    same = sq.figures(np.full(N, k), np.full(N, k), np.zeros(N), np.ones(N), k)
    assert same == dict(precision=1.0, recall=1.0, density=1.0, coverage=1.0)


# ---------------------------------------------------------------- the C ABI's argument checks (nothing is launched)
def test_entry_points_validate_arguments(lib):
    from split_vae_amd import _lib
    BAD, UNS, WS = _lib.STATUS_BADARG, _lib.STATUS_UNSUPPORTED, _lib.STATUS_WORKSPACE
    a = 1 << 20                                                            # a well aligned address nobody dereferences: every call below is refused
    n = C.c_int64(-1)
    wsb = lib.sv_prdc_workspace_bytes
    assert wsb(64, 64, 32, 5, None) == BAD
    assert wsb(0, 64, 32, 5, C.byref(n)) == BAD and wsb(64, 0, 32, 5, C.byref(n)) == BAD and wsb(64, 64, 0, 5, C.byref(n)) == BAD
    assert wsb(_lib.PRDC_MAX_NQ + 1, 64, 32, 5, C.byref(n)) == UNS and wsb(64, _lib.PRDC_MAX_NR + 1, 32, 5, C.byref(n)) == UNS
    assert wsb(64, 64, _lib.PRDC_MAX_L + 1, 5, C.byref(n)) == UNS and wsb(64, 64, 32, 0, C.byref(n)) == UNS
    assert wsb(64, 64, 32, _lib.PRDC_MAX_K + 1, C.byref(n)) == UNS and n.value == -1
    assert (_lib.PRDC_MAX_K, _lib.PRDC_MAX_L, _lib.PRDC_MAX_NQ, _lib.PRDC_MAX_NR) == (31, 512, 8 * 65536, 1 << 24)
    assert wsb(1, 1, 1, 1, C.byref(n)) == 0 and n.value > 0 and n.value % 256 == 0        # a count shape below k + 1 rows
    assert wsb(130, 5000, 33, 5, C.byref(n)) == 0 and n.value % 256 == 0
    count_bytes = n.value
    ok = [a, 33, a, 33, a, 130, 5000, 33, a, a, a, a, count_bytes, None]

    def count(**kw):
        names = ("q", "ldq", "r", "ldr", "rad", "Nq", "Nr", "L", "cnt", "dmin", "imin", "ws", "bytes", "stream")
        args = list(ok)
        for key, v in kw.items():
            args[names.index(key)] = v
        return lib.sv_prdc_count(*args)

    for key in ("q", "r", "rad", "cnt", "ws"):
        assert count(**{key: None}) == BAD, key
    for key in ("q", "r", "rad", "cnt", "dmin", "imin", "ws"):
        assert count(**{key: a + 2}) == BAD, key
    assert count(ws=a + 8) == BAD                                          # the workspace: 16 bytes
    assert count(Nq=0) == BAD and count(Nr=0) == BAD and count(L=0) == BAD and count(Nq=-1) == BAD
    assert count(ldq=32) == BAD and count(ldr=32) == BAD
    assert count(L=513, ldq=600, ldr=600) == UNS and count(Nq=_lib.PRDC_MAX_NQ + 1) == UNS and count(Nr=_lib.PRDC_MAX_NR + 1) == UNS
    assert count(bytes=count_bytes - 1) == WS
    assert count(dmin=None, imin=None, bytes=count_bytes - 1) == WS        # the minima are optional: the call gets as far as the size check

    assert wsb(300, 300, 33, 5, C.byref(n)) == 0
    both = n.value
    assert wsb(300, 301, 33, 5, C.byref(n)) == 0 and n.value < both        # Nq == Nr: the radius pass's lists are covered too
    okr = [a, 33, 300, 33, 5, a, a, both, None]

    def radius(**kw):
        names = ("x", "ldx", "N", "L", "k", "rad", "ws", "bytes", "stream")
        args = list(okr)
        for key, v in kw.items():
            args[names.index(key)] = v
        return lib.sv_prdc_radius(*args)

    for key in ("x", "rad", "ws"):
        assert radius(**{key: None}) == BAD, key
        assert radius(**{key: a + 2}) == BAD, key
    assert radius(ws=a + 8) == BAD and radius(N=0) == BAD and radius(L=0) == BAD and radius(ldx=32) == BAD
    assert radius(k=0) == UNS and radius(k=32) == UNS and radius(N=5) == UNS and radius(N=6, bytes=1) == WS
    assert radius(L=513, ldx=600) == UNS and radius(N=_lib.PRDC_MAX_NQ + 1) == UNS
    assert radius(bytes=both - 1) == WS and radius(k=31, N=32, bytes=1) == WS


# ---------------------------------------------------------------- flags, parser, refusals, the line
WEIGHTS = ["--weights", "nowhere.npz"]


@pytest.mark.parametrize("flags,words", [
    (["--sq_k", "0"], "--sq_k K"),
    (["--sq_k", "32"], "--sq_k K"),
    (["--sq_images", "5"], "--sq_images N"),
    (["--sq_images", "3", "--sq_k", "3"], "--sq_images N"),
    (["--sq_images", "65537"], "--sq_images N"),
    (["--sq_grid", "0"], "--sq_grid n"),
    (["--sq_grid", "33"], "--sq_grid n"),
    (["--augmentation", "blur"], "--augmentation blur"),
    (["--global_latent_dims", "300", "--local_latent_dims", "300"], "Lg + Ll <= 512"),
    (["--knn_probe", "5"], "runs the sample-quality report only: --knn_probe"),
    (["--recon_quality", "8"], "runs the sample-quality report only: --recon_quality"),
])
def test_refusals_print_their_message_before_any_device_work(monkeypatch, flags, words):
    import torch
    from split_vae_amd import data, sample_quality

    def never(*a, **k):
        raise AssertionError("data or device work before the flags were checked")
    monkeypatch.setattr(data, "get_dataset", never)
    monkeypatch.setattr(torch.cuda, "is_available", never)
    with pytest.raises(SystemExit) as e:
        sample_quality.main(WEIGHTS + flags)
    assert words in str(e.value)


def test_parser_has_the_flags_and_leaves_the_other_parsers_alone():
    from split_vae_amd import reports, sample_quality as sq
    from split_vae_amd.main import build_parser
    args = sq.build_parser().parse_args(WEIGHTS)
    assert (args.sq_images, args.sq_k, args.sq_out, args.sq_grid) == (None, 5, None, 10)
    assert not hasattr(build_parser().parse_args([]), "sq_k") and not hasattr(build_parser().parse_args([]), "weights")
    assert not any(e.name.startswith("sq") or e.name.startswith("sample") for e in reports.TABLE)
    sq.check_flags("lgvae", "scramble", None, 5, 10, 128, 128)
    sq.check_flags("lggmvae", "no_op", 65536, 31, 32, 256, 256)
    sq.check_flags("gmvae", "scramble", 6, 5, 1, 512, 128)                 # one block: z_l does not widen the feature space
    with pytest.raises(SystemExit):
        sq.check_flags("lgvae", "scramble", None, 5, 10, 512, 1)
    with pytest.raises(SystemExit):
        sq.check_flags("spair", "scramble", None, 5, 10, 128, 128)
    assert sq.PERM_STEP == 0x7371 << 40
    from split_vae_amd import swap
    assert sq.PERM_STEP != swap.PERM_STEP


def test_report_line_for_two_blocks_and_one():
    from split_vae_amd import sample_quality as sq
    res = dict(n_images=26032, k=5, sets=("prior", "g_drawn", "l_drawn", "recon"))
    for n, name in enumerate(res["sets"]):
        base = 0.125 * (n + 1)
        res.update({"precision_" + name: base, "recall_" + name: base + 0.0625, "density_" + name: base * 2, "coverage_" + name: base + 0.25,
                    "frechet_" + name: 10.0 / (n + 1)})
    line = sq.report_line(res)
    assert line == ("Test sample quality (26032 images, k=5): prior precision 0.1250, recall 0.1875, density 0.2500, coverage 0.3750, Frechet 10.0000; "
                    "z_g drawn (z_l kept): precision 0.2500, recall 0.3125, density 0.5000, coverage 0.5000, Frechet 5.0000; "
                    "z_l drawn (z_g kept): precision 0.3750, recall 0.4375, density 0.7500, coverage 0.6250, Frechet 3.3333; "
                    "reconstructions: precision 0.5000, recall 0.5625, density 1.0000, coverage 0.7500, Frechet 2.5000")
    res["sets"] = ("prior", "recon")                                          # gmvae
    one = sq.report_line(res)
    assert one == ("Test sample quality (26032 images, k=5): prior precision 0.1250, recall 0.1875, density 0.2500, coverage 0.3750, Frechet 10.0000; "
                   "reconstructions: precision 0.5000, recall 0.5625, density 1.0000, coverage 0.7500, Frechet 2.5000")
