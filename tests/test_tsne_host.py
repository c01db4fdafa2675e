"""CPU tests of the t-SNE report: the twin of tests/tsne_ref.py pinned by itself (the gradient against finite differences of its KL,
the beta search against the perplexity, the float32 restatement against the derived bounds, every wrong kernel rejected on the cases
the GPU tests use, the measured trajectory drift), and the host side of split_vae_amd/tsne.py (flags, parser, refusals, the
rasteriser, the .npz keys, argument checks of the C entry points).  No GPU."""
import ctypes as C

import numpy as np
import pytest

import tsne_ref as tr


@pytest.fixture(scope="module")
def step_P():
    x, _ = tr.clusters(tr.STEP_N, tr.STEP_L, seed=1)
    a = tr.affinities(x, tr.STEP_PERP)
    return a, a["P"], tr.p_const(a["P"])


# ---------------------------------------------------------------- the twin itself
def test_gradient_is_the_finite_difference_of_the_kl():
    x, _ = tr.clusters(40, 5, seed=2)
    P = tr.affinities(x, 8.0)["P"].astype(np.float64)
    P = P / P.sum()                                # the identity needs sum P = 1 exactly; the fp32 P sums to 1 within 2^-22
    pc = tr.p_const(P)
    Y = np.random.default_rng(0).standard_normal((40, 2))

    def kl(Y):
        s = tr.pair_sums(P, Y)
        return pc[1] + s["l"].sum() + np.log(s["z"].sum()) * pc[0]
    s = tr.pair_sums(P, Y)
    g = 4.0 * (s["A"] - s["R"] / s["z"].sum())
    fd, h = np.zeros_like(Y), 1e-6
    for i in range(40):
        for c in range(2):
            Yp, Ym = Y.copy(), Y.copy()
            Yp[i, c] += h
            Ym[i, c] -= h
            fd[i, c] = (kl(Yp) - kl(Ym)) / (2 * h)
    assert np.abs(fd - g).max() <= 1e-8 * max(1.0, np.abs(g).max())      # central differences at h = 1e-6: h^2 f''' + eps / h
    # and step()'s g is this g, its KL this KL
    st = dict(Y=Y.astype(np.float32), inc=np.zeros((40, 2), np.float32), gain=np.ones((40, 2), np.float32))
    r = tr.step(P, pc, st, 300)
    s32 = tr.pair_sums(P, st["Y"])
    assert np.allclose(r["g"], 4.0 * (s32["A"] - s32["R"] / s32["z"].sum()), rtol=1e-13, atol=0) and abs(r["KL"] - kl(st["Y"].astype(np.float64))) < 1e-12


@pytest.mark.parametrize("case", [c for c in tr.affinity_cases() if c[1].shape[0] <= 257], ids=lambda c: c[0])
def test_search_reaches_the_perplexity_on_every_row_with_a_root(case):
    _, x, perp, _, _ = case
    a = tr.affinities(x, perp)
    N = x.shape[0]
    assert a["has_root"].all() and np.abs(a["H"] - np.log(perp)).max() <= 1e-5
    P = a["P"].astype(np.float64)
    assert np.array_equal(a["P"], a["P"].T) and np.all(np.diag(P) == 0) and abs(P.sum() - 1.0) <= 2.0 ** -22
    assert np.all(np.abs(a["cond"].astype(np.float64).sum(axis=1) - 1.0) <= 2.0 ** -24 * 2 + N * 2.0 ** -149)


@pytest.mark.parametrize("case", tr.no_root_cases(), ids=lambda c: c[0])
def test_rows_without_a_root_end_at_the_clamp(case):
    name, x, perp = case
    a = tr.affinities(x, perp)
    stuck = ~a["has_root"]
    assert stuck.any() and np.all(a["beta"][stuck] == tr.BETA_MAX) and np.isfinite(a["P"]).all() and np.isfinite(a["H"]).all()
    assert (stuck.all() and np.all(a["cond"][~np.eye(17, dtype=bool)] == np.float32(1 / 16))) if name == "all_equal" else stuck[:13].all()
    if name == "duplicates":
        assert np.count_nonzero(a["cond"][0]) == 12 and np.all(a["cond"][0, 1:13] == np.float32(1 / 12))


def test_nan_and_inf_distances_count_as_the_largest():
    D = tr.distances_f32(tr.clusters(12, 3, seed=4)[0])
    D[0, 5], D[5, 0], D[3, 7] = np.nan, np.inf, np.inf
    a = tr.affinities(D, 3.0, is_D=True)
    assert np.isfinite(a["P"]).all() and np.isfinite(a["beta"]).all() and a["cond"][0, 5] == 0


def test_initial_map_is_reproducible_and_small():
    y, b = tr.init_map(500, 3)
    assert np.array_equal(y, tr.init_map(500, 3)[0]) and not np.array_equal(y[:100], tr.init_map(100, 4)[0])
    assert np.array_equal(y[:100], tr.init_map(100, 3)[0])       # keyed by (seed, row, component): a prefix of a longer map
    assert 8e-5 < y.std() < 1.2e-4 and abs(y.mean()) < 2e-5 and b.max() < 1e-9


# ---------------------------------------------------------------- the float32 restatement, the bounds, the wrong kernels
STEP_BUGS = ("drop4", "rep_w", "z_half", "kl_exag", "gain_inverted", "no_recentre", "momentum_late", "exag_late", "gain_no_floor")


@pytest.fixture(scope="module")
def step_results(step_P):
    _, P, pc = step_P
    eta = tr.auto_eta(tr.STEP_N, 12.0)
    out = {}
    for kind, t in tr.STEP_CASES:
        state = tr.step_states(tr.STEP_N, kind)
        want = tr.step(P, pc, state, t, eta=eta)
        out[(kind, t)] = (state, want, tr.step_bounds(want, state, pc, eta=eta), eta)
    return out


@pytest.mark.parametrize("kind,t", tr.STEP_CASES)
def test_float32_restatement_stays_within_half_of_every_bound(step_P, step_results, kind, t):
    _, P, pc = step_P
    state, want, b, eta = step_results[(kind, t)]
    assert b["g_gap"] >= 4.0
    em = tr.step(P, pc, state, t, eta=eta, emulate=True)
    bad, worst = tr.check_step(em, want, b, scale=0.5)
    assert bad == [], (bad, worst)


@pytest.mark.parametrize("bug", STEP_BUGS)
def test_every_wrong_iteration_breaks_a_bound(step_P, step_results, bug):
    _, P, pc = step_P
    broken = []
    for (kind, t), (state, want, b, eta) in step_results.items():
        got = tr.step(P, pc, state, t, eta=eta, bug=bug)
        if tr.check_step(got, want, b)[0]:
            broken.append((kind, t))
    assert broken, bug
    if bug in ("momentum_late", "exag_late"):
        assert all(t == 250 for _, t in broken)     # the iteration on the far side of the switch is the one that tells


@pytest.mark.parametrize("bug", ["self_kept", "sym_over_n", "entropy_bits"])
def test_every_wrong_affinity_breaks_a_bound(bug):
    broken = 0
    for _, x, perp, _, _ in tr.affinity_cases()[:5]:
        D = tr.distances_f32(x)
        N = x.shape[0]
        good = tr.affinities(D, perp, is_D=True)
        got = tr.affinities(D, perp, is_D=True, bug=bug)
        dd, off = tr._row_terms(D)
        h_err = np.abs(tr.entropy(dd, off, got["beta"])[0] - np.log(perp)).max()      # the GPU test's entropy check of the device's beta
        _, bj = tr.p_bounds(tr.conditional(D, got["beta"]), N)
        p_err = np.abs(got["P"].astype(np.float64) - tr.joint(tr.conditional(D, got["beta"]))) > bj
        broken += int(h_err > 1e-5 or p_err.any() or np.any(np.diag(got["P"]) != 0) or abs(got["P"].astype(np.float64).sum() - 1) > 2.0 ** -22)
        assert np.abs(good["H"] - np.log(perp)).max() <= 1e-5
    assert broken == 5, bug


def test_wrong_neighbour_scores_differ():
    rng = np.random.default_rng(5)
    a = rng.standard_normal((40, 3))
    a[:9] = a[0]
    lab = (np.arange(40) % 2).astype(np.uint8)
    nl, nm = tr.knn_lists(a, 5), tr.knn_lists(a[:, :2], 5)
    good = tr.neighbour_scores(nl, nm, lab, 2)
    assert tr.neighbour_scores(nl, nm, lab, 2, bug="self_in_lists") != good and tr.neighbour_scores(nl, nm, lab, 2, bug="vote_tie_high") != good
    assert tr.neighbour_scores(nl, nl, lab, 2)[0] == 40 * 4 and tr.neighbour_scores(nl, nm)[1:] == [0, 0]
    assert len(tr.BUGS) >= 10 and set(STEP_BUGS) | {"self_kept", "sym_over_n", "entropy_bits", "self_in_lists", "vote_tie_high"} == set(tr.BUGS)


@pytest.mark.parametrize("T,exag_iters,recorded", [(3, 250, dict(Y=2.5e-7, inc=2.4e-7, gain=4.8e-8, kl=1.5e-8)),
                                                   (20, 10, dict(Y=4.2e-4, inc=8.7e-5, gain=2.9e-7, kl=3.8e-6))])
def test_recorded_drift_is_the_measured_drift(T, exag_iters, recorded):
    """the figures written into tests/test_gpu_tsne.py are what the twin and its float32 restatement part by here (to the 10 % the figures were rounded to)"""
    x, _ = tr.clusters(tr.RUN_N, tr.RUN_L, seed=tr.RUN_SEED)
    P = tr.affinities(x, tr.RUN_PERP)["P"]
    pc = tr.p_const(P)
    eta = tr.auto_eta(tr.RUN_N, 12.0)
    a = tr.run(P, pc, tr.RUN_N, T, tr.RUN_SEED, exag_iters=exag_iters, eta=eta)
    b = tr.run(P, pc, tr.RUN_N, T, tr.RUN_SEED, exag_iters=exag_iters, eta=eta, emulate=True)
    for key, val in recorded.items():
        d = float(np.abs(np.asarray(a[key], np.float64) - np.asarray(b[key], np.float64)).max())
        assert 0.8 * val <= d <= 1.1 * val, (key, d, val)


def test_twin_separates_the_planted_clusters_with_room():
    """the premise of the GPU map test, on the twin: accuracy 1.0, well over half of the 5 latent neighbours kept, KL falling"""
    x, lab = tr.planted_map(tr.MAP_N, tr.MAP_L, seed=tr.MAP_SEED)
    P = tr.affinities(x, tr.MAP_PERP)["P"]
    r = tr.run(P, tr.p_const(P), tr.MAP_N, tr.MAP_T, tr.MAP_SEED, eta=tr.auto_eta(tr.MAP_N, 12.0))
    sc = tr.neighbour_scores(tr.knn_lists(x, 6), tr.knn_lists(r["Y"], 6), lab, 4)
    assert sc[1] == tr.MAP_N and sc[2] == tr.MAP_N and sc[0] / (5.0 * tr.MAP_N) > 0.7
    assert np.isfinite(r["kl"]).all() and r["kl"][-1] < r["kl"][250]


# ---------------------------------------------------------------- the host side of split_vae_amd/tsne.py
def test_flag_checks():
    from split_vae_amd import tsne
    from split_vae_amd._lib import TSNE_MAX_N
    ok = dict(images=1000, perplexity=30.0, iters=1000, exaggeration=12.0, exag_iters=250, lr=None, k=10)
    tsne.check_flags(**ok)
    tsne.check_flags(**dict(ok, images=None))
    for bad, word in ((dict(images=3), "--tsne_images"), (dict(images=TSNE_MAX_N + 1), "--tsne_images"), (dict(perplexity=1.0), "--perplexity"),
                      (dict(perplexity=999.0), "--perplexity"), (dict(iters=-1), "--tsne_iters"), (dict(exaggeration=0.5), "--tsne_exaggeration"),
                      (dict(exag_iters=-1), "--tsne_exag_iters"), (dict(lr=0.0), "--tsne_lr"), (dict(k=0), "--tsne_k"), (dict(k=32), "--tsne_k"),
                      (dict(images=8, perplexity=3.0, k=8), "--tsne_k"), (dict(canvas=8), "--tsne_canvas"), (dict(global_latent_dims=513), "512")):
        with pytest.raises(SystemExit, match=word):
            tsne.check_flags(**dict(ok, **bad))
    assert tsne.parse_lr("auto") is None and tsne.parse_lr("125.5") == 125.5 and tsne.auto_lr(10000, 12.0) == 10000 / 48.0 and tsne.auto_lr(100, 12.0) == 50.0
    with pytest.raises(SystemExit, match="--tsne_lr"):
        tsne.parse_lr("fast")


def test_parser_is_fresh_and_main_refuses_other_reports(tmp_path):
    from split_vae_amd import reports, tsne
    from split_vae_amd.main import build_parser
    ap = tsne.build_parser()
    args = ap.parse_args(["--weights", "w.npz"])
    assert (args.perplexity, args.tsne_iters, args.tsne_exaggeration, args.tsne_exag_iters, args.tsne_lr, args.tsne_k, args.tsne_out, args.tsne_images) == \
        (30.0, 1000, 12.0, 250, "auto", 10, None, None)
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--perplexity", "5"])          # main's parser does not know the flag
    with pytest.raises(SystemExit):
        ap.parse_args([])                                         # --weights is required
    entry = reports.TABLE[0]
    with pytest.raises(SystemExit, match="runs the t-SNE report only: --%s belongs to" % entry.name):
        tsne.main(["--weights", "w.npz", "--%s" % entry.name, "8"])
    with pytest.raises(SystemExit, match="--perplexity"):
        tsne.main(["--weights", "w.npz", "--perplexity", "0.5"])


def test_rasteriser_puts_a_point_in_its_pixel_and_draws_in_index_order():
    from split_vae_amd import tsne
    Y = np.array([[-1.0, -1.0], [1.0, 1.0], [1.0, -1.0], [0.0, 0.0], [0.0, 0.0]], np.float32)
    lab = np.array([0, 1, 2, 3, 4])
    px = tsne.pixel_of(Y, 101, margin=0.05)
    assert px.tolist() == [[5, 95], [95, 5], [95, 95], [50, 50], [50, 50]]          # y grows upwards; the box fills the canvas inside the margin
    img = tsne.rasterise(Y, lab, size=101, radius=2)
    assert img.shape == (101, 101, 3) and np.all(img[0, 0] == 1.0) and np.all(img[50, 60] == 1.0)
    for i in (0, 1, 2):
        assert np.allclose(img[px[i, 1], px[i, 0]], tsne.PALETTE[lab[i]])
        assert np.allclose(img[px[i, 1] + 2, px[i, 0]], tsne.PALETTE[lab[i]]) and np.all(img[px[i, 1] + 3, px[i, 0]] == 1.0)      # a disc of radius 2
    assert np.allclose(img[50, 50], tsne.PALETTE[4])                                # the later of two coincident points is on top
    assert np.allclose(tsne.rasterise(Y[::-1], lab[::-1], size=101)[50, 50], tsne.PALETTE[3])
    one = tsne.rasterise(Y, None, size=101)
    assert np.allclose(one[50, 50], tsne.ONE_COLOUR) and np.array_equal(tsne.rasterise(Y, lab, size=101), img)
    wide = tsne.pixel_of(np.array([[0, 0], [10, 1]], np.float32), 101, 0.05)        # one scale for both axes, centred
    assert wide.tolist() == [[5, 54], [95, 46]] or wide.tolist() == [[5, 55], [95, 45]]
    assert tsne.rasterise(np.zeros((3, 2), np.float32), None, size=32).shape == (32, 32, 3)      # a degenerate box does not divide by zero


def test_outputs_have_the_stated_files_and_keys(tmp_path):
    from split_vae_amd import tsne
    from split_vae_amd.visualizer import load_png
    rng = np.random.default_rng(0)
    res = dict(n_images=20, labels=(np.arange(20) % 3).astype(np.uint8), Y_g=rng.standard_normal((20, 2)).astype(np.float32), Y_l=None,
               kl_trace_g=np.arange(5.0), kl_trace_l=None, beta_g=np.ones(20), beta_l=None)
    paths = tsne.save_outputs(res, str(tmp_path / "o"), size=48)
    assert [p.rsplit("/", 1)[1] for p in paths] == ["tsne_z_g.png", "tsne.npz"] and load_png(paths[0]).shape == (48, 48, 3)
    doc = np.load(paths[1])
    assert sorted(doc.files) == ["Y_g", "Y_l", "beta_g", "beta_l", "kl_g", "kl_l", "labels"]
    assert np.array_equal(doc["Y_g"], res["Y_g"]) and doc["Y_l"].shape == (0, 2) and np.array_equal(doc["labels"], res["labels"])
    line = tsne.report_line(dict(n_images=20, perplexity=5.0, iters=7, k=3, labelled=True, kl_g=1.25, kept_g=0.5, map_acc_g=0.75, latent_acc_g=1.0, kl_l=None))
    assert line == "Test t-SNE map (20 images, perplexity 5, 7 iterations): z_g KL 1.2500, neighbours kept@3 0.5000, map k-NN acc 0.7500 (latent 1.0000)"


def test_entry_points_validate_arguments_without_a_gpu(lib_built):
    """the refusals that need no device memory: null pointers and sizes outside the accepted domain come back before any launch"""
    from split_vae_amd import _lib
    lib = _lib.load()
    BAD, UNS = _lib.STATUS_BADARG, _lib.STATUS_UNSUPPORTED
    n = C.c_int64()
    assert lib.sv_tsne_chunk_rows() == tr.CHUNK
    assert lib.sv_tsne_workspace_bytes(3, C.byref(n)) == UNS and lib.sv_tsne_workspace_bytes(_lib.TSNE_MAX_N + 1, C.byref(n)) == UNS
    assert lib.sv_tsne_workspace_bytes(100, None) == BAD and lib.sv_tsne_workspace_bytes(_lib.TSNE_MAX_N, C.byref(n)) == 0 and n.value % 256 == 0
    assert lib.sv_tsne_workspace_bytes(4, C.byref(n)) == 0 and n.value > 0
    assert lib.sv_tsne_affinities(None, 8, 64, 8, 5.0, 3, None, None, None, None, None, 0, None) == BAD
    assert lib.sv_tsne_init(64, 0, None, None, None, None, None) == BAD
    assert lib.sv_tsne_iterate(None, None, 64, 1, 12.0, 250, 50.0, None, None, None, None, None, 0, None, None, 0, None) == BAD
    assert lib.sv_tsne_neighbour_scores(None, None, None, 64, 5, 0, None, None) == BAD
    fake = C.c_void_p(4096)                                      # aligned, never dereferenced: the size checks come before any launch
    assert lib.sv_tsne_affinities(fake, 8, 3, 8, 1.5, 3, fake, fake, fake, fake, fake, 1 << 40, None) == UNS
    assert lib.sv_tsne_affinities(fake, 8, 64, 8, 1.0, 3, fake, fake, fake, fake, fake, 1 << 40, None) == UNS
    assert lib.sv_tsne_affinities(fake, 8, 64, 8, 63.0, 3, fake, fake, fake, fake, fake, 1 << 40, None) == UNS
    assert lib.sv_tsne_affinities(fake, 513, 64, 513, 5.0, 3, fake, fake, fake, fake, fake, 1 << 40, None) == UNS
    assert lib.sv_tsne_affinities(fake, 8, 64, 8, 5.0, 3, fake, fake, fake, fake, fake, 16, None) == _lib.STATUS_WORKSPACE
    assert lib.sv_tsne_affinities(C.c_void_p(4098), 8, 64, 8, 5.0, 3, fake, fake, fake, fake, fake, 1 << 40, None) == BAD
    assert lib.sv_tsne_iterate(fake, fake, 64, -1, 12.0, 250, 50.0, fake, fake, fake, fake, fake, 4, None, fake, 1 << 40, None) == UNS
    assert lib.sv_tsne_neighbour_scores(fake, fake, None, 64, 32, 0, fake, None) == UNS
