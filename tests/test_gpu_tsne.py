"""GPU tests of the exact t-SNE map: sv_tsne_affinities / sv_tsne_init / sv_tsne_iterate / sv_tsne_neighbour_scores (csrc/tsne.hip)
against the float64 twin of tests/tsne_ref.py -- distances bit for bit against sv_knn_classify, the beta search by the entropy it
reaches, P and single iterations by the derived per-element bounds, short runs by a multiple of the twin-vs-float32 drift, bits across
repeats / groupings / offsets, the neighbour scores exactly, a planted map, refusals, and split_vae_amd/tsne.py on the three models.

Trajectory tolerances (test 3).  The rounding drift of a trajectory cannot be derived; it is measured on the CPU as the largest
difference between the twin and its float32 restatement on the same case (tests/test_tsne_host.py recomputes it), and the device may
differ from the twin by DRIFT_FACTOR = 8 times that (v_rcp_f32 / v_log_f32 are not in the restatement):
    T = 3  (exaggerated throughout):        Y 2.5e-7   inc 2.4e-7   gain 4.8e-8   KL 1.5e-8
    T = 20 (the switch at iteration 10):    Y 4.2e-4   inc 8.7e-5   gain 2.9e-7   KL 3.8e-6
(measured with the switch at 250 and T = 20 the two CPU runs part by 0.17 in Y on a map of extent 12: the first exaggerated
iterations at this N overshoot, the gains' sign decisions part, and no tolerance means anything; hence the early switch.)"""
import ctypes as C

import numpy as np
import pytest
import torch

import tsne_ref as tr

pytestmark = pytest.mark.gpu

F32 = torch.float32
DRIFT_FACTOR = 8.0
DRIFT = {3: dict(exag_iters=250, Y=2.5e-7, inc=2.4e-7, gain=4.8e-8, kl=1.5e-8),
         20: dict(exag_iters=10, Y=4.2e-4, inc=8.7e-5, gain=2.9e-7, kl=3.8e-6)}
WORST = {"P": 0.0, "step": 0.0, "run": 0.0}       # worst device error over bound / tolerance seen by this run (printed per test)


@pytest.fixture(scope="module")
def env(lib_built):
    assert torch.cuda.is_available()
    from split_vae_amd import _lib, ops, tsne
    return ops, tsne, _lib


def _dev(a, pad=0, off=0):
    """rows of `a` on the device with `pad` unused floats behind every row and the first element `off` floats past a 256-byte boundary"""
    a = np.ascontiguousarray(a, np.float32)
    N, L = a.shape
    flat = torch.full((N * (L + pad) + off + 4,), 1e30, dtype=F32, device="cuda")       # the padding must never be read into a result
    t = flat[off:off + N * (L + pad)].view(N, L + pad)
    t[:, :L] = torch.from_numpy(a).cuda()
    return t[:, :L]


def _np(t):
    return t.cpu().numpy()


# ---------------------------------------------------------------- 1. affinities
@pytest.mark.parametrize("case", tr.affinity_cases(), ids=lambda c: c[0])
def test_affinities_match_the_twin(env, case):
    ops = env[0]
    _, x, perp, pad, off = case
    N, L = x.shape
    xd = _dev(x, pad, off)
    # distances: every row's k smallest, as sorted values, are sv_knn_classify's nn_dist bit for bit (k = min(32, N))
    D = _np(ops.tsne_affinities(xd, perp, stages=1)["P"])
    k = min(32, N)
    _, _, nn_d = ops.knn_classify(xd, xd, torch.zeros((N,), dtype=torch.uint8, device="cuda"), k, 2, want_neighbours=True)
    assert np.array_equal(np.sort(D, axis=1)[:, :k], _np(nn_d))
    # the conditional rows at the device's beta
    c2 = ops.tsne_affinities(xd, perp, stages=2)
    beta, H = _np(c2["beta"]), _np(c2["row_entropy"])
    tb, tH, has_root = tr.search_beta(D, perp)
    assert has_root.all()
    dd, offd = tr._row_terms(D)
    Hd = tr.entropy(dd, offd, beta)[0]
    print("max |H(device beta) - log perplexity| = %.3g; max rel beta difference to the twin's %.3g" %
          (np.abs(Hd - np.log(perp)).max(), np.abs(beta / tb - 1).max()))
    assert np.abs(Hd - np.log(perp)).max() <= 1e-5
    assert np.abs(H - Hd).max() <= 1e-9
    cond = tr.conditional(D, beta)
    bc, bj = tr.p_bounds(cond, N)
    got = _np(c2["P"]).astype(np.float64)
    assert np.all(np.abs(got - cond) <= bc) and np.all(np.diag(got) == 0)
    # the joint P
    a3 = ops.tsne_affinities(xd, perp)
    P = _np(a3["P"])
    assert np.array_equal(_np(a3["beta"]), beta)
    want = tr.joint(cond)
    err = np.abs(P.astype(np.float64) - want)
    WORST["P"] = max(WORST["P"], float((err / bj).max()))
    assert np.all(err <= bj)
    assert np.array_equal(P, P.T) and np.all(np.diag(P) == 0) and np.all(np.isfinite(P)) and P.min() >= 0
    assert abs(P.astype(np.float64).sum() - 1.0) <= 2.0 ** -22          # two fp32 roundings of relative 2^-24 per entry, twice
    pc = _np(a3["p_const"])
    wpc = tr.p_const(P)
    assert np.all(np.abs(pc - wpc) <= 1e-12 * np.maximum(1.0, np.abs(wpc)))
    print("worst device error over bound so far: %s" % WORST)


@pytest.mark.parametrize("case", tr.no_root_cases(), ids=lambda c: c[0])
def test_rows_without_a_root_end_at_the_clamp(env, case):
    """all rows equal; more exact duplicates of a row than the perplexity: beta = 2^60, the row the header defines, nothing NaN or inf"""
    ops = env[0]
    name, x, perp = case
    N = x.shape[0]
    xd = _dev(x)
    D = _np(ops.tsne_affinities(xd, perp, stages=1)["P"])
    c2 = ops.tsne_affinities(xd, perp, stages=2)
    beta, cond = _np(c2["beta"]), _np(c2["P"])
    tb, _, has_root = tr.search_beta(D, perp)
    stuck = ~has_root
    assert stuck.any() and np.array_equal(beta[stuck], tb[stuck]) and np.all(beta[stuck] == tr.BETA_MAX)
    want = tr.conditional(D, beta)
    bc, _ = tr.p_bounds(want, N)
    assert np.all(np.abs(cond.astype(np.float64) - want) <= bc) and np.all(np.isfinite(cond)) and np.all(np.diag(cond) == 0)
    if name == "all_equal":
        assert np.all(D == D[0, 1]) or np.all(D[~np.eye(N, dtype=bool)] == D[0, 1])
        assert np.all(cond[~np.eye(N, dtype=bool)] == np.float32(1.0 / (N - 1)))
    else:
        m = (D[0] == np.delete(D[0], 0).min()).sum() - (1 if D[0, 0] == np.delete(D[0], 0).min() else 0)
        assert m >= 12 and abs(float(cond[0].sum()) - 1.0) <= 1e-5 and np.count_nonzero(cond[0]) == m
    P = _np(ops.tsne_affinities(xd, perp)["P"])
    assert np.all(np.isfinite(P)) and np.array_equal(P, P.T) and abs(P.astype(np.float64).sum() - 1.0) <= 2.0 ** -22


def test_nothing_outside_the_stated_extents_is_written(env):
    """Sentinel-filled outputs with guard words on both sides and a NaN-filled workspace with a guard behind it: the results equal a
    plain run's, every output word inside the extents is written, no guard word changes."""
    ops, _, _lib = env
    lib = _lib.load()
    N, L, T, G = 130, 37, 4, 64
    x, _ = tr.clusters(N, L, seed=21)
    xd = _dev(x, pad=1, off=1)
    plain = ops.tsne_affinities(xd, 12.0)
    pst = ops.tsne_iterate(plain, ops.tsne_init(ops.tsne_state(N, T), 9), T, 12.0, 2, 50.0)
    nbytes = ops.tsne_workspace_bytes(N)

    def guarded(n, dt, fill):
        t = torch.full((n + 2 * G,), fill, dtype=dt, device="cuda")
        return t, t[G:G + n]
    bufs = dict(P=guarded(N * N, F32, -777.0), beta=guarded(N, torch.float64, -777.0), H=guarded(N, torch.float64, -777.0),
                pc=guarded(2, torch.float64, -777.0), Y=guarded(2 * N, F32, -777.0), inc=guarded(2 * N, F32, -777.0),
                gain=guarded(2 * N, F32, -777.0), state=guarded(4, torch.int32, -7), kl=guarded(T, torch.float64, -777.0),
                z=guarded(1, torch.float64, -777.0))
    wsf = torch.full((nbytes // 4 + 2 * G,), float("nan"), dtype=F32, device="cuda")
    ws = wsf[G:G + nbytes // 4]
    assert ws.data_ptr() % 16 == 0
    p = lambda name: C.c_void_p(bufs[name][1].data_ptr())      # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    wp = C.c_void_p(ws.data_ptr())
    assert lib.sv_tsne_affinities(C.c_void_p(xd.data_ptr()), xd.stride(0), N, L, 12.0, 3, p("P"), p("beta"), p("H"), p("pc"), wp, nbytes, st) == 0
    assert lib.sv_tsne_init(N, 9, p("Y"), p("inc"), p("gain"), p("state"), st) == 0
    assert lib.sv_tsne_iterate(p("P"), p("pc"), N, T, 12.0, 2, 50.0, p("Y"), p("inc"), p("gain"), p("state"), p("kl"), T, p("z"), wp, nbytes, st) == 0
    torch.cuda.synchronize()
    for name, (full, view) in bufs.items():
        fill = full[0].item()
        assert (full[:G] == fill).all() and (full[-G:] == fill).all(), name
        assert not (view == fill).any(), name
    assert torch.isnan(wsf[:G]).all() and torch.isnan(wsf[-G:]).all()
    for name, t in (("P", plain["P"]), ("beta", plain["beta"]), ("pc", plain["p_const"]), ("Y", pst["Y"]), ("inc", pst["inc"]), ("gain", pst["gain"]),
                    ("kl", pst["kl"])):
        assert torch.equal(bufs[name][1], t.reshape(-1)), name
    assert bufs["state"][1][0].item() == T
    assert float(xd.max()) < 1e29                                 # the input is untouched


# ---------------------------------------------------------------- 2. one iteration from a given state
@pytest.fixture(scope="module")
def step_P(env):
    ops = env[0]
    x, _ = tr.clusters(tr.STEP_N, tr.STEP_L, seed=1)
    aff = ops.tsne_affinities(_dev(x), tr.STEP_PERP)
    return aff, _np(aff["P"]), _np(aff["p_const"])


@pytest.mark.parametrize("kind,t", tr.STEP_CASES)
def test_one_iteration_from_a_given_state(env, step_P, kind, t):
    """tiny / spread / coincident states on each side of the exaggeration and momentum switch (249: exaggerated, 250: not)"""
    ops = env[0]
    aff, P, pc = step_P
    N = tr.STEP_N
    eta = tr.auto_eta(N, 12.0)
    state = tr.step_states(N, kind)
    want = tr.step(P, pc, state, t, eta=eta)
    b = tr.step_bounds(want, state, pc, eta=eta)
    print("%s t = %d: smallest |g| / bound(g) = %.3g" % (kind, t, b["g_gap"]))
    assert b["g_gap"] >= 4.0                                      # the premise: no sign decision of the gain rule is within rounding
    st = ops.tsne_state(N, 300, Y=torch.from_numpy(state["Y"]).cuda(), inc=torch.from_numpy(state["inc"]).cuda(),
                        gain=torch.from_numpy(state["gain"]).cuda(), counter=t)
    ops.tsne_iterate(aff, st, 1, 12.0, 250, eta)
    kl = _np(st["kl"])
    got = dict(Y=_np(st["Y"]), inc=_np(st["inc"]), gain=_np(st["gain"]), Z=_np(st["z"])[0], KL=kl[t])
    assert int(st["state"][0].item()) == t + 1 and np.isnan(np.delete(kl, t)).all()
    bad, worst = tr.check_step(got, want, b)
    WORST["step"] = max(WORST["step"], worst)
    print("worst device error over bound so far: %s" % WORST)
    assert bad == []


# ---------------------------------------------------------------- 3. short runs from sv_tsne_init
@pytest.fixture(scope="module")
def run_P(env):
    ops = env[0]
    x, _ = tr.clusters(tr.RUN_N, tr.RUN_L, seed=tr.RUN_SEED)
    aff = ops.tsne_affinities(_dev(x), tr.RUN_PERP)
    return aff, _np(aff["P"]), _np(aff["p_const"]), x


def test_initial_map_is_the_philox_stream(env):
    ops = env[0]
    for N, seed in ((4, 0), (257, 5), (1000, 2 ** 40 + 3)):
        st = ops.tsne_init(ops.tsne_state(N, 1), seed)
        want, bound = tr.init_map(N, seed)
        assert np.all(np.abs(_np(st["Y"]).astype(np.float64) - want) <= bound)
        assert (st["inc"] == 0).all() and (st["gain"] == 1).all() and (st["state"] == 0).all()
    a = _np(ops.tsne_init(ops.tsne_state(64, 1), 1)["Y"])
    assert not np.array_equal(a, _np(ops.tsne_init(ops.tsne_state(64, 1), 2)["Y"])) and 5e-5 < a.std() < 2e-4


@pytest.mark.parametrize("T", [3, 20])
def test_short_runs_stay_within_the_measured_drift(env, run_P, T):
    ops = env[0]
    aff, P, pc, _ = run_P
    N, d = tr.RUN_N, DRIFT[T]
    eta = tr.auto_eta(N, 12.0)
    st = ops.tsne_init(ops.tsne_state(N, T), tr.RUN_SEED)
    y0 = _np(st["Y"])
    ops.tsne_iterate(aff, st, T, 12.0, d["exag_iters"], eta)
    # the twin starts from the device's own initial map (pinned by test_initial_map_is_the_philox_stream): the run is what is compared
    want = tr.run(P, pc, N, T, tr.RUN_SEED, exag_iters=d["exag_iters"], eta=eta,
                  state=dict(Y=y0, inc=np.zeros((N, 2), np.float32), gain=np.ones((N, 2), np.float32)))
    for key, got in (("Y", st["Y"]), ("inc", st["inc"]), ("gain", st["gain"]), ("kl", st["kl"])):
        err = float(np.abs(_np(got).astype(np.float64) - want[key]).max())
        WORST["run"] = max(WORST["run"], err / (DRIFT_FACTOR * d[key]))
        print("T = %d %s: device - twin %.3g, tolerance %.3g" % (T, key, err, DRIFT_FACTOR * d[key]))
        assert err <= DRIFT_FACTOR * d[key], key
    print("worst device error over tolerance so far: %s" % WORST)


# ---------------------------------------------------------------- 4. bits
def test_same_inputs_same_bits(env, run_P):
    """a repeat, 12 iterations as one call against groups that straddle the switch at 5, and x at another offset and pitch"""
    ops = env[0]
    _, _, _, x = run_P
    N, T = tr.RUN_N, 12

    def go(groups, pad=0, off=0):
        aff = ops.tsne_affinities(_dev(x, pad, off), tr.RUN_PERP)
        st = ops.tsne_init(ops.tsne_state(N, T), 3)
        for g in groups:
            ops.tsne_iterate(aff, st, g, 12.0, 5, 50.0)
        return [aff["P"], aff["beta"], st["Y"], st["inc"], st["gain"], st["kl"], st["state"]]
    base = go([T])
    assert int(base[-1][0].item()) == T and torch.isfinite(base[5]).all()
    for other in (go([T]), go([4, 1, 0, 2, 5]), go([1] * T), go([T], pad=3, off=1), go([7, 5], pad=0, off=2)):
        for a, b in zip(base, other):
            assert torch.equal(a, b)


# ---------------------------------------------------------------- 5. neighbour scores
def _score_cases():
    rng = np.random.default_rng(5)
    out = []
    for N, k, n_class in ((4, 1, 2), (65, 5, 3), (300, 10, 10), (130, 31, 64)):
        a, b = rng.standard_normal((N, 3)), rng.standard_normal((N, 2))
        out.append((tr.knn_lists(a, k + 1), tr.knn_lists(b, k + 1), rng.integers(0, n_class, N).astype(np.uint8), n_class))
    # lists without self: 9 exact duplicates at k + 1 = 4 (the lowest indices fill the list), and vote ties: 2 classes at k = 4
    a = rng.standard_normal((40, 3))
    a[:9] = a[0]
    lab = (np.arange(40) % 2).astype(np.uint8)
    out.append((tr.knn_lists(a, 4), tr.knn_lists(rng.standard_normal((40, 2)), 4), lab, 2))
    out.append((tr.knn_lists(a, 5), tr.knn_lists(a[:, :2], 5), lab, 2))
    return out


@pytest.mark.parametrize("i", range(6))
def test_neighbour_scores_equal_the_twin(env, i):
    ops = env[0]
    nl, nm, lab, n_class = _score_cases()[i]
    N = nl.shape[0]
    if i >= 4:
        assert any(r not in nl[r] for r in range(N))              # the premise: a list without self
    dl, dm, dlab = (torch.from_numpy(v).cuda() for v in (nl, nm, lab))
    got = _np(ops.tsne_neighbour_scores(dl, dm, dlab, n_class)).tolist()
    assert got == tr.neighbour_scores(nl, nm, lab, n_class)
    start = torch.tensor([5, 6, 7], dtype=torch.int64, device="cuda")
    bare = _np(ops.tsne_neighbour_scores(dl, dm, None, 0, counts=start)).tolist()   # no labels: only the first counter moves; ADDED to
    assert bare == [5 + got[0], 6, 7]


# ---------------------------------------------------------------- 6. the map shows what it should
def test_planted_clusters_come_apart_in_the_map(env):
    """tsne_ref.planted_map: the twin and the float32 restatement reach accuracy 1.0 and keep 0.76 .. 0.80 of the neighbours on it"""
    ops, tsne, _ = env
    x, lab = tr.planted_map(tr.MAP_N, tr.MAP_L, seed=tr.MAP_SEED)
    xd = _dev(x)
    f = tsne.fit(xd, tr.MAP_PERP, tr.MAP_T, seed=tr.MAP_SEED)
    counts = _np(tsne.neighbour_counts(xd, f["Y"], 5, torch.from_numpy(lab).cuda(), 4))
    kl = f["kl_trace"]
    print("kept@5 %.4f, map acc %.4f, latent acc %.4f, KL %.4f -> %.4f -> %.4f" %
          (counts[0] / (5 * tr.MAP_N), counts[1] / tr.MAP_N, counts[2] / tr.MAP_N, kl[0], kl[250], kl[-1]))
    assert counts[1] == tr.MAP_N and counts[0] / (5.0 * tr.MAP_N) > 0.5
    assert np.isfinite(kl).all() and kl[-1] < kl[250]


# ---------------------------------------------------------------- 7. refusals
def test_refusals(env):
    ops, _, _lib = env
    lib = _lib.load()
    x = torch.zeros((64, 8), device="cuda")
    uns, bad = "SV_E_UNSUPPORTED", "SV_E_BADARG"
    for call, code in ((lambda: ops.tsne_affinities(x[:3], 1.5), uns), (lambda: ops.tsne_affinities(x, 1.0), uns),
                       (lambda: ops.tsne_affinities(x, 63.0), uns), (lambda: ops.tsne_affinities(torch.zeros((8, 513), device="cuda"), 2.0), uns),
                       (lambda: ops.tsne_affinities(x, 5.0, stages=4), uns), (lambda: ops.tsne_workspace_bytes(_lib.TSNE_MAX_N + 1), uns),
                       (lambda: ops.tsne_workspace_bytes(3), uns)):
        with pytest.raises(_lib.SplitVaeError, match=code):
            call()
    with pytest.raises(ValueError):
        ops.tsne_affinities(x.double(), 5.0)
    N = 64
    nb = ops.tsne_workspace_bytes(N)
    ws = torch.zeros((nb + 64,), dtype=torch.uint8, device="cuda")
    P = torch.zeros((N * N + 4,), device="cuda")
    d = torch.zeros((N + 4,), dtype=torch.float64, device="cuda")
    f = torch.zeros((2 * N + 4,), device="cuda")
    s = torch.zeros((8,), dtype=torch.int32, device="cuda")
    cnt = torch.zeros((4,), dtype=torch.int64, device="cuda")
    nn = torch.zeros((N * 4,), dtype=torch.int32, device="cuda")
    q = lambda t, o=0: C.c_void_p(t.data_ptr() + o)      # noqa: E731
    BAD, UNS, WS = _lib.STATUS_BADARG, _lib.STATUS_UNSUPPORTED, _lib.STATUS_WORKSPACE
    aff = lambda **k: lib.sv_tsne_affinities(k.get("x", q(x)), 8, k.get("N", N), k.get("L", 8), k.get("perp", 5.0), 3, k.get("P", q(P)), k.get("beta", q(d)),  # noqa: E731
                                             q(d), q(d), k.get("ws", q(ws)), k.get("nb", nb), None)
    assert aff(x=None) == BAD and aff(P=None) == BAD and aff(beta=None) == BAD and aff(ws=None) == BAD
    assert aff(x=q(x, 2)) == BAD and aff(P=q(P, 1)) == BAD and aff(beta=q(d, 4)) == BAD and aff(ws=q(ws, 8)) == BAD
    assert aff(N=3) == UNS and aff(perp=1.0) == UNS and aff(perp=float(N - 1)) == UNS and aff(L=513) == UNS and aff(L=9) == UNS
    assert aff(N=_lib.TSNE_MAX_N + 1) == UNS and aff(nb=nb - 1) == WS and aff(perp=float("nan")) == UNS
    it = lambda **k: lib.sv_tsne_iterate(k.get("P", q(P)), q(d), k.get("N", N), k.get("iters", 1), k.get("e", 12.0), 250, k.get("eta", 50.0), k.get("Y", q(f)),  # noqa: E731
                                         q(f), q(f), k.get("s", q(s)), k.get("kl", q(d)), 4, None, q(ws), k.get("nb", nb), None)
    assert it(P=None) == BAD and it(Y=None) == BAD and it(s=None) == BAD and it(kl=None) == BAD and it(Y=q(f, 2)) == BAD and it(kl=q(d, 4)) == BAD
    assert it(iters=-1) == UNS and it(N=3) == UNS and it(e=0.5) == UNS and it(eta=0.0) == UNS and it(nb=nb - 1) == WS
    assert lib.sv_tsne_init(N, 0, None, q(f), q(f), q(s), None) == BAD and lib.sv_tsne_init(3, 0, q(f), q(f), q(f), q(s), None) == UNS
    assert lib.sv_tsne_init(N, 0, q(f, 1), q(f), q(f), q(s), None) == BAD
    sc = lambda **k: lib.sv_tsne_neighbour_scores(k.get("a", q(nn)), q(nn), None, k.get("N", N), k.get("k", 3), 0, k.get("c", q(cnt)), None)      # noqa: E731
    assert sc(a=None) == BAD and sc(c=None) == BAD and sc(c=q(cnt, 4)) == BAD and sc(k=0) == UNS and sc(k=32) == UNS and sc(N=3) == UNS
    torch.cuda.synchronize()
    # no launch: every buffer is as it was
    assert not P.any() and not d.any() and not f.any() and not s.any() and not cnt.any()


# ---------------------------------------------------------------- 8. the report on the three models
H, LAT = 32, 128


def _family(n, seed):
    """n images6 [n,32,32,6] on two one-parameter families (tests/test_gpu_knn.py): the latent means lie along curves; the class follows x"""
    rng = np.random.default_rng(seed)
    a, b, c, e = (rng.uniform(-1, 1, (H, H, 3)) for _ in range(4))
    t, s = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    x = (1 - t)[:, None, None, None] * a + t[:, None, None, None] * b
    xh = (1 - s)[:, None, None, None] * c + s[:, None, None, None] * e
    return np.concatenate([x, xh], axis=-1).astype(np.float32), np.minimum((t * 10).astype(np.int64), 9)


def _batches(images, cls, B=16):
    onehot = np.eye(10, dtype=np.float32)[cls]
    return [(torch.from_numpy(images[o:o + B]).cuda(), torch.from_numpy(onehot[o:o + B]).cuda()) for o in range(0, len(images), B)]


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
def test_evaluate_on_the_three_models(env, deterministic, kind, tmp_path):
    """seeded weights, 128 labelled images, T = 50: the figures equal the twin's scores of the returned maps; the line; the files.  (Fixed-order
    reductions in the encoders: the labelled and the unlabelled call must see the same latent means to draw the same map.)"""
    from split_vae_amd.latent_info import posteriors
    from split_vae_amd.visualizer import load_png
    ops, tsne, _ = env
    model = _make(kind)
    images, cls = _family(144, 31)
    batches = _batches(images, cls)
    res = tsne.evaluate(model, batches, 128, perplexity=10.0, iters=50, k=5, seed=17)
    mu, _, Lg, Ll = posteriors(model, batches, 128)
    mu = _np(mu)
    assert (res["n_images"], res["iters"], res["k"], res["labelled"]) == (128, 50, 5, True) and np.array_equal(res["labels"], cls[:128])
    for s, z in (("g", mu[:, :Lg]), ("l", mu[:, Lg:])):
        if s == "l" and kind == "gmvae":
            assert Ll == 0 and all(res[k + "_l"] is None for k in ("kl", "kept", "map_acc", "latent_acc", "Y", "beta"))
            continue
        Y = res["Y_" + s]
        assert Y.shape == (128, 2) and np.isfinite(Y).all() and np.abs(Y.mean(axis=0)).max() < 1e-4 and res["kl_trace_" + s].shape == (50,)
        assert np.isfinite(res["kl_trace_" + s]).all() and res["kl_" + s] == res["kl_trace_" + s][-1] and res["beta_" + s].shape == (128,)
        # the scores of the device's own neighbour lists, recounted by the twin
        zd, Yd = torch.from_numpy(np.ascontiguousarray(z)).cuda(), torch.from_numpy(Y).cuda()
        dummy = torch.zeros((128,), dtype=torch.uint8, device="cuda")
        nl = _np(ops.knn_classify(zd, zd, dummy, 6, 2, want_neighbours=True)[1])
        nm = _np(ops.knn_classify(Yd, Yd, dummy, 6, 2, want_neighbours=True)[1])
        want = tr.neighbour_scores(nl, nm, cls[:128].astype(np.uint8), 10)
        assert (round(res["kept_" + s] * 5 * 128), round(res["map_acc_" + s] * 128), round(res["latent_acc_" + s] * 128)) == tuple(want)
    line = tsne.report_line(res)
    assert line.startswith("Test t-SNE map (128 images, perplexity 10, 50 iterations): z_g KL ") and ", neighbours kept@5 0." in line
    assert ", map k-NN acc " in line and " (latent " in line and ("; z_l KL " in line) == (kind != "gmvae")
    paths = tsne.save_outputs(res, str(tmp_path / "out"), size=96)
    assert [p.rsplit("/", 1)[1] for p in paths] == (["tsne_z_g.png", "tsne.npz"] if kind == "gmvae" else ["tsne_z_g.png", "tsne_z_l.png", "tsne.npz"])
    for p in paths[:-1]:
        img = load_png(p)
        assert img.shape == (96, 96, 3)
    doc = np.load(paths[-1])
    assert set(doc.files) == {"Y_g", "Y_l", "labels", "kl_g", "kl_l", "beta_g", "beta_l"}
    assert np.array_equal(doc["Y_g"], res["Y_g"]) and np.array_equal(doc["kl_g"], res["kl_trace_g"]) and np.array_equal(doc["labels"], cls[:128])
    assert doc["Y_l"].shape == ((0, 2) if kind == "gmvae" else (128, 2))
    bare = tsne.evaluate(model, [b[0] for b in batches], 128, perplexity=10.0, iters=50, k=5, seed=17)
    assert bare["labelled"] is False and bare["map_acc_g"] is None and bare["kept_g"] == res["kept_g"] and np.array_equal(bare["Y_g"], res["Y_g"])
    assert "acc" not in tsne.report_line(bare)


def test_cli_prints_the_line_and_writes_the_files(env, tmp_path, monkeypatch, capsys):
    """--synthetic -no_label (32 test images): one note, the label-free line, the three files"""
    from split_vae_amd import tsne
    from split_vae_amd.main import build_parser, make_model
    from split_vae_amd.utils import dotdict
    from split_vae_amd.visualizer import load_png
    monkeypatch.chdir(tmp_path)
    flags = ["--synthetic", "-no_label", "--batch_size", "8", "--dtype", "f32"]
    config = dotdict(vars(build_parser().parse_args(flags)))
    model, _ = make_model("lgvae", config, (None, 32, 32, 3))
    path = str(tmp_path / "w.npz")
    model.save_weights(path)
    capsys.readouterr()
    out_dir = str(tmp_path / "maps")
    res = tsne.main(flags + ["--weights", path, "--tsne_images", "30", "--perplexity", "5", "--tsne_iters", "20", "--tsne_k", "3", "--tsne_out", out_dir,
                             "--tsne_canvas", "64"])
    out = capsys.readouterr().out
    lines = [l for l in out.splitlines() if l.startswith("Test t-SNE map (")]
    assert out.count(tsne.UNLABELLED) == 1 and len(lines) == 1
    assert lines[0].startswith("Test t-SNE map (30 images, perplexity 5, 20 iterations): z_g KL ") and "acc" not in lines[0]
    assert "; z_l KL " in lines[0] and "neighbours kept@3 " in lines[0]
    assert res["tsne_n_images"] == 30 and res["tsne_map_acc_g"] is None and 0.0 <= res["tsne_kept_g"] <= 1.0
    assert load_png(out_dir + "/tsne_z_g.png").shape == (64, 64, 3) and load_png(out_dir + "/tsne_z_l.png").shape == (64, 64, 3)
    doc = np.load(out_dir + "/tsne.npz")
    assert doc["Y_g"].shape == (30, 2) and (doc["labels"] == -1).all() and doc["kl_l"].shape == (20,)
