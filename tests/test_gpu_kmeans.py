"""GPU tests of the k-means cluster report: sv_kmeans_seed / sv_kmeans_iterate / sv_kmeans_best / sv_contingency (csrc/kmeans.hip)
against the float64 twin of tests/kmeans_ref.py -- bit for bit on planted integer lattices, by the derived bounds and by invariants
on Gaussian data --, the edge shapes, the extents written, split_vae_amd/cluster.py on the three models and its command line."""
import ctypes as C

import numpy as np
import pytest
import torch

import kmeans_ref as kr

pytestmark = pytest.mark.gpu

F32 = torch.float32
WORST = {"centroid": 0.0, "inertia": 0.0}      # worst device error over bound seen by this run (printed per test)


@pytest.fixture(scope="module")
def env(lib_built):
    assert torch.cuda.is_available()
    from split_vae_amd import _lib, cluster, ops
    return ops, cluster, _lib


def _dev(a, pad=0, off=0):
    """rows of `a` on the device with `pad` unused floats behind every row and the first element `off` floats past a 256-byte boundary"""
    a = np.ascontiguousarray(a, np.float32)
    N, L = a.shape
    flat = torch.full((N * (L + pad) + off + 4,), 1e30, dtype=F32, device="cuda")       # the padding must never be read into a result
    t = flat[off:off + N * (L + pad)].view(N, L + pad)
    t[:, :L] = torch.from_numpy(a).cuda()
    return t[:, :L]


def _host(fit, extra=()):
    out = {k: fit[k].cpu().numpy() for k in ("centroids", "assign", "counts", "inertia", "n_iter")}
    out.update({k: v.cpu().numpy() for k, v in extra})
    return out


def device_fit(ops, x, c0, T, groups=None, pad=0, off=0):
    """sv_kmeans_iterate from given centroids, the iterations enqueued in `groups` (default: all at once) -> the twin's dict"""
    xd = x if torch.is_tensor(x) else _dev(x, pad, off)
    fit = ops.kmeans_state(xd, torch.from_numpy(np.ascontiguousarray(c0, np.float32)).cuda())
    groups = [T] if groups is None else groups
    assert sum(groups) == T
    for i, g in enumerate(groups):
        ops.kmeans_iterate(xd, fit, g, resume=i > 0)
    out = _host(fit)
    out["best"] = int(ops.kmeans_best(fit["inertia"]).item())
    return out


def device_kmeans(ops, x, K, R, T, seed, pad=0, off=0):
    xd = _dev(x, pad, off)
    cent, picks = ops.kmeans_seed(xd, K, R, seed=seed, want_picks=True)
    seeds = cent.cpu().numpy()
    out = device_fit(ops, xd, seeds, T)
    out["picks"] = picks.cpu().numpy()
    out["seeds"] = seeds
    return out


def run_on_device(ops, case, **kw):
    if case["kind"] == "kmeans":
        return device_kmeans(ops, case["x"], case["K"], case["R"], case["T"], case["seed"], **kw)
    if case["kind"] == "fit":
        return device_fit(ops, case["x"], case["c0"], case["T"], **kw)
    return dict(picks=ops.kmeans_seed(_dev(case["x"], **kw), case["K"], case["R"], seed=case["seed"], want_picks=True)[1].cpu().numpy())


# ---------------------------------------------------------------- 1. the shared cases, bit for bit
CASES = [c for c in kr.cases() if not c.get("host_only")]


@pytest.fixture(scope="module")
def twin_results():
    return {c["name"]: kr.run_case(c) for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_planted_sets_match_the_twin_bit_for_bit(env, twin_results, case):
    """The planted lattices (sums exact in fp64, gaps ~ 1), the trap set (exact ties, an empty cluster that keeps its centroid, T = 0
    and T hit before convergence) and the equal rows (every key +inf): picks, assignments, counts, n_iter, best and the centroids
    equal the twin's bit for bit, the inertia within the derived sum bound -- the comparison that rejects the wrong kernels of
    tests/test_kmeans_host.py."""
    ops = env[0]
    want = twin_results[case["name"]]
    if case["kind"] == "kmeans":
        assert want["pick_gap"] >= 1e-4 and want["assign_gap"] >= 1e-4
    got = run_on_device(ops, case)
    assert kr.compare(got, want, case["x"], exact=False) == []
    if "seeds" in got:
        assert np.array_equal(got["seeds"], case["x"][want["picks"]])            # a centre is a copy of its row
    if case["kind"] == "kmeans":
        b = got["best"]
        assert kr.accuracy(kr.contingency(got["assign"][b], case["labels"], case["K"], case["K"])) == 1.0


# ---------------------------------------------------------------- 2. edge shapes, bit for bit
def _planted_any(N, L, K, seed):
    for s in range(seed, seed + 50):
        try:
            return kr.planted(N, L, K, s)
        except AssertionError:
            continue
    raise AssertionError("no planted set with distinct centres")


def _shapes():
    chunk = kr.CHUNK
    base = dict(N=65, L=37, K=3, R=3, pad=0, off=0, T=20)
    sweep = ([dict(N=2, K=2), dict(N=63), dict(N=64), dict(N=chunk - 1), dict(N=chunk), dict(N=chunk + 1), dict(N=2 * chunk + 5), dict(N=10, K=10)] +
             [dict(L=v) for v in (1, 5, 31, 32, 33, 130, 512)] + [dict(K=2), dict(K=10), dict(K=17, R=3), dict(K=64, N=130)] +
             [dict(R=1), dict(R=16), dict(R=16, K=17, N=130), dict(R=16, K=64, N=130, L=5)] +
             [dict(pad=1), dict(off=1), dict(pad=1, off=1, L=32), dict(pad=3, off=3, L=130)] + [dict(T=0), dict(T=1)])
    return [dict(base, **s) for s in sweep]


@pytest.mark.parametrize("c", _shapes(), ids=lambda c: "N%d-L%d-K%d-R%d-p%d-o%d-T%d" % (c["N"], c["L"], c["K"], c["R"], c["pad"], c["off"], c["T"]))
def test_edge_shapes_match_the_twin_bit_for_bit(env, c):
    """One sweep per axis around (65, 37, 3, 3): N around the 64-row tile and the chunk of the segmented sum, N = K, L around the 16-
    and 32-wide K steps and at 512, K over the three column paddings, R up to the 1024-column corner, a row pitch of L + 1 and base
    pointers 4 and 12 bytes off the 16-byte grid, T = 0 and T = 1.  Planted integer data: everything equals the twin bit for bit."""
    ops = env[0]
    assert ops.kmeans_chunk_rows() == kr.CHUNK
    x, _ = _planted_any(c["N"], c["L"], c["K"], 100 + c["N"] + c["L"])
    want = kr.kmeans(x, c["K"], c["R"], c["T"], seed=11)
    assert want["pick_gap"] >= 1e-4 and want["assign_gap"] >= 1e-4      # the premise: no race and no row at a near-tie
    got = device_kmeans(ops, x, c["K"], c["R"], c["T"], 11, pad=c["pad"], off=c["off"])
    assert kr.compare(got, want, x, exact=False) == []


# ---------------------------------------------------------------- 3. Gaussian data: one step at the derived bounds
GAUSS = ((1500, 33, 7, 1.0), (4099, 128, 10, 0.5), (777, 130, 64, 0.3), (2500, 256, 30, 0.5), (1000, 512, 16, 0.5))


def _gauss(N, L, K, spread, seed=5):
    rng = np.random.default_rng(seed)
    centres = spread * rng.standard_normal((K, L))
    lab = rng.integers(0, K, N)
    x = (centres[lab] + rng.standard_normal((N, L))).astype(np.float32)
    c0 = np.stack([centres.astype(np.float32), x[rng.choice(N, K, replace=False)]])
    return x, c0


def _decided(x, c):
    """(twin assignment, mask of the rows the gap rule decides): the rows whose relative gap between the two nearest centroids is above
    4 times the derived relative error of those two distances"""
    a, _, dm = kr.assign(x, c)
    bound = kr.distance_bound(x, c)
    order = np.argsort(dm, axis=1, kind="stable")[:, :2]
    rows = np.arange(dm.shape[0])
    d1, d2 = dm[rows, order[:, 0]], dm[rows, order[:, 1]]
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(d2 > 0, (bound[rows, order[:, 0]] + bound[rows, order[:, 1]]) / d2, np.inf)
    return a, kr.assign_gap(dm) > 4.0 * rel


def _check_assign(x, cent, assign, what):
    """every restart's device assignment against the twin's on the decided rows; at most 2 % of the rows are left out"""
    for r in range(cent.shape[0]):
        a, ok = _decided(x, cent[r])
        left = 1.0 - ok.mean()
        print("%s restart %d: %.2f %% of the rows left to the gap rule" % (what, r, 100 * left))
        assert left <= 0.02
        assert np.array_equal(assign[r][ok], a[ok])
        # an undecided row still sits at one of its two nearest centroids
        dm = kr.distances(x[~ok], cent[r])
        if len(dm):
            assert (np.argsort(dm, axis=1)[:, :2] == assign[r][~ok][:, None]).any(axis=1).all()


def _check_inertia(x, cent, assign, inertia):
    for r in range(cent.shape[0]):
        want = ((x.astype(np.float64) - cent[r].astype(np.float64)[assign[r]]) ** 2).sum()
        tol = kr.inertia_bound(x, cent[r], assign[r])
        WORST["inertia"] = max(WORST["inertia"], abs(inertia[r] - want) / tol)
        assert abs(inertia[r] - want) <= tol


@pytest.mark.parametrize("N,L,K,spread", GAUSS, ids=lambda v: str(v))
def test_one_step_on_gaussian_data(env, N, L, K, spread):
    """sv_kmeans_iterate from given centroids (the true centres; K rows of the data).  The assign pass equals the twin's wherever the
    gap decides; the update is judged on its own, against the twin's fp64 sums over the DEVICE's assignment:
    |c - ref| <= 2^-24 |ref| + N 2^-53 sum |x| / count; counts and inertia belong to the returned assignment."""
    ops = env[0]
    x, c0 = _gauss(N, L, K, spread)
    xd = _dev(x)
    fit = ops.kmeans_state(xd, torch.from_numpy(c0.copy()).cuda())
    ops.kmeans_iterate(xd, fit, 0)
    p0 = _host(fit)
    assert np.array_equal(p0["centroids"], c0) and (p0["n_iter"] == 0).all()
    _check_assign(x, c0, p0["assign"], "pass 0")
    _check_inertia(x, c0, p0["assign"], p0["inertia"])
    ops.kmeans_iterate(xd, fit, 1, resume=True)
    p1 = _host(fit)
    x64 = x.astype(np.float64)
    for r in range(2):
        a0 = p0["assign"][r]
        assert np.array_equal(p0["counts"][r], np.bincount(a0, minlength=K))
        sums, cnt = kr.sums_counts(x, a0, K)
        absum = np.zeros((K, L))
        np.add.at(absum, a0, np.abs(x64))
        have = cnt > 0
        ref = sums[have] / cnt[have, None]
        tol = 2.0 ** -24 * np.abs(ref) + N * 2.0 ** -53 * absum[have] / cnt[have, None]
        err = np.abs(p1["centroids"][r][have].astype(np.float64) - ref)
        WORST["centroid"] = max(WORST["centroid"], float((err / np.maximum(tol, 1e-300)).max()))
        assert (err <= tol).all()
        assert np.array_equal(p1["centroids"][r][~have], c0[r][~have])
        assert np.array_equal(p1["counts"][r], np.bincount(p1["assign"][r], minlength=K))
    _check_assign(x, p1["centroids"], p1["assign"], "pass 1")
    _check_inertia(x, p1["centroids"], p1["assign"], p1["inertia"])
    assert (p1["n_iter"] == 1).all()
    print("worst device error over bound so far: %s" % WORST)


# ---------------------------------------------------------------- 4. fits on Gaussian data, by invariants
def _equal_fits(a, b):
    return all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in ("centroids", "assign", "counts", "inertia", "n_iter")) and a["best"] == b["best"]


@pytest.mark.parametrize("N,L,K,spread,T", [(1500, 33, 7, 1.0, 9), (4099, 128, 10, 0.5, 6)], ids=lambda v: str(v))
def test_fits_on_gaussian_data_hold_their_invariants(env, N, L, K, spread, T):
    ops = env[0]
    x, c0 = _gauss(N, L, K, spread, seed=9)
    c0 = np.concatenate([c0, x[None, 7:7 + K]])                   # R = 3
    xd = _dev(x)
    once = device_fit(ops, xd, c0, T)
    # the returned state belongs together
    _check_assign(x, once["centroids"], once["assign"], "fit")
    _check_inertia(x, once["centroids"], once["assign"], once["inertia"])
    for r in range(3):
        assert np.array_equal(once["counts"][r], np.bincount(once["assign"][r], minlength=K))
    assert ((once["n_iter"] >= 1) & (once["n_iter"] <= T)).all()
    assert once["best"] == int(np.argmin(once["inertia"]))
    # the same bits in groups of 1, in groups of 3 and in a second run
    assert _equal_fits(device_fit(ops, xd, c0, T, groups=[1] * T), once)
    assert _equal_fits(device_fit(ops, xd, c0, T, groups=[3] * (T // 3) + ([T % 3] if T % 3 else [])), once)
    assert _equal_fits(device_fit(ops, xd, c0, T), once)
    # the inertia of pass t + 1 is not above that of pass t, beyond the sum bound
    fit = ops.kmeans_state(xd, torch.from_numpy(c0.copy()).cuda())
    trace = []
    for t in range(T + 1):
        ops.kmeans_iterate(xd, fit, 0 if t == 0 else 1, resume=t > 0)
        h = _host(fit)
        trace.append((h["inertia"], [kr.inertia_bound(x, h["centroids"][r], h["assign"][r]) for r in range(3)]))
    for (i0, b0), (i1, b1) in zip(trace, trace[1:]):
        assert all(i1[r] <= i0[r] + b0[r] + b1[r] for r in range(3))
    assert any(trace[-1][0][r] < trace[0][0][r] for r in range(3))
    # a restart that converged before T kept riding along: n_iter froze, the bits stayed
    more = device_fit(ops, xd, c0, T + 4)
    for r in range(3):
        if once["n_iter"][r] < T:
            assert more["n_iter"][r] == once["n_iter"][r] and np.array_equal(more["centroids"][r], once["centroids"][r])
            assert np.array_equal(more["assign"][r], once["assign"][r]) and more["inertia"][r] == once["inertia"][r]
    # permuted rows, the same centroids: the assign pass permutes with them (d does not depend on where the row sits)
    perm = np.random.default_rng(3).permutation(N)
    p = device_fit(ops, x[perm], c0, 0)
    q = device_fit(ops, xd, c0, 0)
    assert np.array_equal(p["assign"], q["assign"][:, perm]) and np.array_equal(p["counts"], q["counts"])
    print("worst device error over bound so far: %s" % WORST)


# ---------------------------------------------------------------- 5. the extents written
def test_nothing_outside_the_stated_extents_is_written(env):
    """Sentinel-filled outputs with guard words on both sides and a NaN-filled workspace with a guard behind it: the results equal a
    plain run's, every output word inside the extents is written, no guard word changes."""
    ops, _, _lib = env
    lib = _lib.load()
    N, L, K, R, T, G = 130, 37, 5, 3, 4, 64
    x, _ = kr.planted(N, L, K, 21)
    xd = _dev(x, pad=1, off=1)
    plain = device_kmeans(ops, x, K, R, T, 13, pad=1, off=1)
    nbytes = ops.kmeans_workspace_bytes(N, L, K, R)

    def guarded(n, dt, fill):
        t = torch.full((n + 2 * G,), fill, dtype=dt, device="cuda")
        return t, t[G:G + n]
    bufs = dict(cent=guarded(R * K * L, F32, -777.0), picks=guarded(R * K, torch.int32, -7), assign=guarded(R * N, torch.int32, -7),
                counts=guarded(R * K, torch.int32, -7), inertia=guarded(R, torch.float64, -777.0), n_iter=guarded(R, torch.int32, -7),
                state=guarded(2 * R + 1, torch.int32, -7))
    wsf = torch.full((nbytes // 4 + 2 * G,), float("nan"), dtype=F32, device="cuda")
    ws = wsf[G:G + nbytes // 4]
    assert ws.data_ptr() % 16 == 0
    p = lambda name: C.c_void_p(bufs[name][1].data_ptr())      # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.sv_kmeans_seed(C.c_void_p(xd.data_ptr()), xd.stride(0), N, L, K, R, 13, p("cent"), p("picks"), C.c_void_p(ws.data_ptr()), nbytes, st) == 0
    assert lib.sv_kmeans_iterate(C.c_void_p(xd.data_ptr()), xd.stride(0), N, L, K, R, T, 0, p("cent"), p("assign"), p("counts"), p("inertia"),
                                 p("n_iter"), p("state"), C.c_void_p(ws.data_ptr()), nbytes, st) == 0
    torch.cuda.synchronize()
    for name, (full, view) in bufs.items():
        fill = full[0].item()
        assert (full[:G] == fill).all() and (full[-G:] == fill).all(), name
        assert not (view == fill).any(), name
    assert torch.isnan(wsf[:G]).all() and torch.isnan(wsf[-G:]).all()
    got = dict(centroids=bufs["cent"][1].view(R, K, L).cpu().numpy(), picks=bufs["picks"][1].view(R, K).cpu().numpy(),
               assign=bufs["assign"][1].view(R, N).cpu().numpy(), counts=bufs["counts"][1].view(R, K).cpu().numpy(),
               inertia=bufs["inertia"][1].cpu().numpy(), n_iter=bufs["n_iter"][1].cpu().numpy())
    for k, v in got.items():
        assert np.array_equal(v, plain[k]), k
    assert float(xd.max()) < 1e29                                 # the input is untouched


# ---------------------------------------------------------------- 6. sv_contingency
@pytest.mark.parametrize("N,Ka,Kb", [(5, 2, 2), (257, 3, 10), (100003, 64, 64), (70000, 30, 10)])
def test_contingency_equals_numpy(env, N, Ka, Kb):
    ops = env[0]
    rng = np.random.default_rng(N)
    a, b = rng.integers(0, Ka, N).astype(np.int32), rng.integers(0, Kb, N).astype(np.int32)
    start = rng.integers(0, 50, (Ka, Kb)).astype(np.int32)
    t = torch.from_numpy(start.copy()).cuda()
    ops.contingency(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), t)
    want = start.astype(np.int64) + kr.contingency(a, b, Ka, Kb)
    assert np.array_equal(t.cpu().numpy(), want)
    a[0], b[1] = Ka, -1                                           # labels outside their range are skipped
    t2 = torch.zeros((Ka, Kb), dtype=torch.int32, device="cuda")
    ops.contingency(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), t2)
    assert np.array_equal(t2.cpu().numpy(), kr.contingency(a[2:], b[2:], Ka, Kb))


def test_wrappers_refuse_what_the_kernels_cannot_read(env):
    ops, _, _lib = env
    x = torch.zeros((20, 8), device="cuda")
    for bad in (lambda: ops.kmeans_seed(x.double(), 3, 2), lambda: ops.kmeans_seed(x.t(), 3, 2), lambda: ops.kmeans_seed(x.cpu(), 3, 2),
                lambda: ops.kmeans_state(x, torch.zeros((2, 3, 9), device="cuda")),
                lambda: ops.contingency(torch.zeros(4, dtype=torch.int64, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda"),
                                        torch.zeros((2, 2), dtype=torch.int32, device="cuda"))):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(_lib.SplitVaeError, match="SV_E_UNSUPPORTED"):
        ops.kmeans_seed(x, 21, 2)                                 # K > N


# ---------------------------------------------------------------- 7. the report on the three models
H, LAT = 32, 128


def _family(n, seed):
    """n images6 [n,32,32,6] on two one-parameter families (tests/test_gpu_knn.py): the latent means lie along curves; the class
    follows x"""
    rng = np.random.default_rng(seed)
    a, b, c, e = (rng.uniform(-1, 1, (H, H, 3)) for _ in range(4))
    t, s = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    x = (1 - t)[:, None, None, None] * a + t[:, None, None, None] * b
    xh = (1 - s)[:, None, None, None] * c + s[:, None, None, None] * e
    return np.concatenate([x, xh], axis=-1).astype(np.float32), np.minimum((t * 10).astype(np.int64), 9)


def _batches(images, cls, B=8):
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
def test_evaluate_equals_the_twin_on_the_same_latent_means(env, deterministic, kind):
    """Random weights, 5 batches of 8 images with made-up labels, the first 36 images, K = 4, 3 restarts: the tables, accuracies,
    NMIs, iteration counts and empty clusters equal the twin's run on the latent means the report clustered; the inertia within the
    sum bound.  model._calls does not move; gmvae reports z_g only."""
    from split_vae_amd.gmvae import accuracy_from_counts
    from split_vae_amd.latent_info import posteriors
    _, cluster, _ = env
    model = _make(kind)
    images, cls = _family(40, 31)
    batches = _batches(images, cls)
    model._calls = 5
    res = cluster.evaluate(model, batches, 36, 4, restarts=3, iters=10, seed=17)
    assert model._calls == 5
    mu, _, Lg, Ll = posteriors(model, batches, 36)
    assert model._calls == 5
    mu = mu.cpu().numpy()
    assert (res["n_images"], res["k"], res["restarts"], res["labelled"]) == (36, 4, 3, True)
    best = {}
    for s, z in (("g", mu[:, :Lg]), ("l", mu[:, Lg:])):
        if s == "l" and kind == "gmvae":
            assert Ll == 0 and all(res[k + "_l"] is None for k in ("acc", "nmi", "inertia", "n_iter", "empty")) and res["nmi_gl"] is None
            assert "table_l" not in res and "table_gl" not in res
            continue
        want = kr.kmeans(z, 4, 3, 10, seed=17)
        gaps = [kr.assign_gap(kr.assign(z, want["centroids"][r])[2]).min() for r in range(3)]
        print("%s z_%s: pick gap %.3g, smallest assign gap %.3g, n_iter %s" % (kind, s, want["pick_gap"], min(gaps), want["n_iter"]))
        assert want["pick_gap"] >= 1e-4 and min(gaps) >= 1e-4      # the premise: no near-tie (if the models move one there, change _family's seed)
        b = want["best"]
        best[s] = want["assign"][b]
        table = kr.contingency(best[s], cls[:36], 4, 10)
        assert res["best_" + s] == b and np.array_equal(res["table_" + s], table)
        assert res["acc_" + s] == accuracy_from_counts(table, 36) == kr.accuracy(table)
        assert abs(res["nmi_" + s] - kr.nmi(table)) <= 1e-12
        assert res["n_iter_" + s] == want["n_iter"][b] and res["empty_" + s] == int((want["counts"][b] == 0).sum())
        assert abs(res["inertia_" + s] * 36 - want["inertia"][b]) <= kr.inertia_bound(z, want["centroids"][b], best[s])
    if kind != "gmvae":
        tgl = kr.contingency(best["g"], best["l"], 4, 4)
        assert np.array_equal(res["table_gl"], tgl) and abs(res["nmi_gl"] - kr.nmi(tgl)) <= 1e-12
    line = cluster.report_line(res)
    assert line.startswith("Test k-means (4 clusters, 36 images, 3 restarts): z_g acc 0.") and ("; z_l acc " in line) == (kind != "gmvae")
    # without labels: the label-free figures, the same clusters
    bare = cluster.evaluate(model, [b[0] for b in batches], 36, 4, restarts=3, iters=10, seed=17)
    assert bare["labelled"] is False and bare["acc_g"] is None and bare["nmi_g"] is None and bare["inertia_g"] == res["inertia_g"]
    assert bare["nmi_gl"] == res["nmi_gl"]


def test_kmeans_api_returns_one_consistent_fit(env):
    _, cluster, _ = env
    x, lab = kr.planted(300, 5, 3, 1)
    res = cluster.kmeans(_dev(x), 3, restarts=4, iters=20, seed=1)
    want = kr.kmeans(x, 3, 4, 20, seed=1)
    assert res["best"] == want["best"] and res["empty"] == 0 and np.array_equal(res["n_iter"], want["n_iter"])
    assert np.array_equal(res["assign"].cpu().numpy(), want["assign"]) and np.array_equal(res["centroids"].cpu().numpy(), want["centroids"])
    assert res["inertia"].dtype == np.float64 and res["counts"].is_cuda


def test_cli_prints_the_label_free_line_on_synthetic_data(env, tmp_path, monkeypatch, capsys):
    """--synthetic -no_label (32 test images): one note, the line without acc / NMI against labels, its figures in the returned dict."""
    from split_vae_amd import cluster
    from split_vae_amd.main import build_parser, make_model
    from split_vae_amd.utils import dotdict
    monkeypatch.chdir(tmp_path)
    flags = ["--synthetic", "-no_label", "--batch_size", "8", "--dtype", "f32"]
    config = dotdict(vars(build_parser().parse_args(flags)))
    model, _ = make_model("lgvae", config, (None, 32, 32, 3))
    path = str(tmp_path / "w.npz")
    model.save_weights(path)
    capsys.readouterr()
    res = cluster.main(flags + ["--weights", path, "--clusters", "4", "--cluster_images", "30", "--cluster_restarts", "2", "--cluster_iters", "5"])
    out = capsys.readouterr().out
    lines = [l for l in out.splitlines() if l.startswith("Test k-means (")]
    assert out.count(cluster.UNLABELLED) == 1 and len(lines) == 1
    assert lines[0].startswith("Test k-means (4 clusters, 30 images, 2 restarts): z_g inertia/image ") and "acc" not in lines[0]
    assert "; z_l inertia/image " in lines[0] and "; NMI(z_g clusters; z_l clusters) 0." in lines[0] or "clusters) 1.0000" in lines[0]
    assert {"kmeans_n_images", "kmeans_inertia_g", "kmeans_inertia_l", "kmeans_nmi_gl", "kmeans_n_iter_g", "kmeans_empty_g"} <= set(res)
    assert res["kmeans_n_images"] == 30 and res["kmeans_acc_g"] is None and 0.0 <= res["kmeans_nmi_gl"] <= 1.0
    assert "%.4f" % res["kmeans_inertia_g"] in lines[0]
