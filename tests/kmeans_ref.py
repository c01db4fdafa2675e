"""float64 NumPy twin of sv_kmeans_* / sv_contingency (include/splitvae.h): the race seeding of k-means++, the assignment under
the total order (d, centroid index), the fp64 update, the fit loop, the best restart, the contingency table, NMI and the
majority-class accuracy.  Every function takes `bug=` -- the name of one deliberately wrong kernel (BUGS) -- so the tests can show
that their comparisons reject each of them."""
import numpy as np

KM_KEY = 0x1a7e3c105fe5
KM_TAG = 0x6b6d0000
BUGS = ("tie_high", "no_clamp", "pad_wins", "drop_chunk_last", "count_off", "empty_zeroed", "inertia_updated", "key_no_log", "argmax_pick",
        "best_highest", "first_row_zero")
CHUNK = 1024                                      # sv_kmeans_chunk_rows(): only the drop_chunk_last bug looks at it


# ---------------------------------------------------------------- Philox4x32-10
def philox_first_word(seed, c0, c1, c2, c3):
    """The first output word of Philox4x32-10 at counter (c0, c1, c2, c3) under the 64-bit key `seed`; c0 may be an array."""
    m32 = np.uint64(0xFFFFFFFF)
    c = [np.atleast_1d(np.asarray(v, np.uint64)) & m32 for v in (c0, c1, c2, c3)]
    n = max(v.size for v in c)
    c = [np.broadcast_to(v, (n,)).copy() for v in c]
    a, b = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ a) & m32, p1 & m32, ((p0 >> np.uint64(32)) ^ c[3] ^ b) & m32, p0 & m32]
        a, b = (a + np.uint64(0x9E3779B9)) & m32, (b + np.uint64(0xBB67AE85)) & m32
    return c[0]


def unit_open(w):
    """(0, 1]: ((w >> 8) + 1) 2^-24, exact in fp32 and fp64"""
    return ((np.asarray(w, np.uint64) >> np.uint64(8)).astype(np.float64) + 1.0) / 16777216.0


# ---------------------------------------------------------------- distance, assignment
def norms(v):
    v = np.asarray(v, np.float64)
    return (v * v).sum(axis=1)


def distances(x, c, bug=None):
    """[N,K] float64: the squared distances the header's d approximates"""
    if bug == "no_clamp":                          # what a kernel without the clamp sees: the fp32 roundoff of equal rows, with its sign
        return distances_f32(x, c, clamp=False).astype(np.float64)
    x, c = np.asarray(x, np.float64), np.asarray(c, np.float64)
    out = np.empty((x.shape[0], c.shape[0]))
    step = max(1, (1 << 22) // max(1, c.shape[0] * x.shape[1]))
    for o in range(0, x.shape[0], step):           # the direct form: exact 0 for equal rows, no cancellation
        out[o:o + step] = ((x[o:o + step, None, :] - c[None, :, :]) ** 2).sum(axis=2)
    return out


def assign(x, c, bug=None):
    """(a [N] int32, d [N] float64 distance to the assigned centroid, dm [N,K] all distances)"""
    dm = distances(x, c, bug)
    K = dm.shape[1]
    if bug == "pad_wins":                          # a padded column (distance n(x) to a zero centroid) competes under index K
        pad = np.maximum(0.0, norms(x))[:, None]
        full = np.concatenate([dm, pad], axis=1)
        a = full.argmin(axis=1)
        a = np.where(a == K, K - 1, a)
    elif bug == "tie_high":
        a = K - 1 - dm[:, ::-1].argmin(axis=1)
    else:
        a = dm.argmin(axis=1)                      # the first minimum: ties to the lower index
    return a.astype(np.int32), dm[np.arange(dm.shape[0]), a], dm


def assign_gap(dm):
    """Per row the relative gap (d_2 - d_1) / d_2 between the nearest and the second-nearest centroid; 0 for an exact tie."""
    s = np.sort(np.asarray(dm, np.float64), axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(s[:, 1] > 0, (s[:, 1] - s[:, 0]) / s[:, 1], 0.0)


# ---------------------------------------------------------------- seeding
def first_centre(seed, r, N, bug=None):
    if bug == "first_row_zero":
        return 0
    w = int(philox_first_word(seed ^ KM_KEY, 0, r, 0, KM_TAG)[0])
    return (w * int(N)) >> 32


def race_keys(m, seed, r, k, bug=None):
    """key_i = -log(u_i) / m_i, +inf where m_i = 0"""
    u = unit_open(philox_first_word(seed ^ KM_KEY, np.arange(m.shape[0]), r, k, KM_TAG))
    e = u if bug == "key_no_log" else -np.log(u)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(m != 0, e / m, np.inf)


def pick_gap(keys):
    """The relative gap (key_2 - key_1) / key_2 between the smallest and the second-smallest race key (inf when only one is finite)."""
    s = np.sort(keys)
    if not np.isfinite(s[1]):
        return np.inf
    return (s[1] - s[0]) / s[1] if s[1] > 0 else 0.0


def seed_centres(x, K, R, seed, bug=None):
    """-> (picks [R,K] int32, centroids [R,K,L] float32, the smallest pick_gap over all races)"""
    x = np.asarray(x)
    N = x.shape[0]
    picks = np.zeros((R, K), np.int32)
    gap = np.inf
    for r in range(R):
        picks[r, 0] = first_centre(seed, r, N, bug)
        m = None
        for k in range(1, K):
            d = distances(x, x[picks[r, k - 1]][None, :], bug)[:, 0]
            m = d if m is None else np.minimum(m, d)
            keys = race_keys(m, seed, r, k, bug)
            finite = np.isfinite(keys)
            if not finite.any():
                picks[r, k] = 0
                continue
            if bug == "argmax_pick":
                picks[r, k] = int(np.where(finite, keys, -np.inf).argmax())
            else:
                picks[r, k] = int(keys.argmin())   # the first minimum: ties to the lower row
                gap = min(gap, pick_gap(keys))
    return picks, x[picks].astype(np.float32), gap


# ---------------------------------------------------------------- update, fit
def sums_counts(x, a, K, bug=None):
    """(sum [K,L] float64, count [K] int64) over the rows by cluster"""
    x = np.asarray(x, np.float64)
    keep = np.ones(x.shape[0], bool)
    if bug == "drop_chunk_last":
        keep[CHUNK - 1::CHUNK] = False
        keep[-1] = False
    s = np.zeros((K, x.shape[1]))
    np.add.at(s, a[keep], x[keep])
    n = np.bincount(a, minlength=K).astype(np.int64)
    if bug == "count_off":
        n = n + (n > 0)
    return s, n


def update(x, a, c, bug=None):
    K = c.shape[0]
    s, n = sums_counts(x, a, K, bug)
    out = np.array(c, np.float32, copy=True)
    have = n > 0
    out[have] = (s[have] / n[have, None]).astype(np.float32)
    if bug == "empty_zeroed":
        out[~have] = 0.0
    return out


def fit(x, c0, T, bug=None, history=None):
    """One restart from centroids c0 [K,L]: dict(centroids float32, assign, counts, inertia, n_iter, assign_gap: the smallest
    assign_gap of any row in any pass).  history: a list that receives every pass's inertia."""
    c = np.array(c0, np.float32, copy=True)
    prev, t, gap = None, 0, np.inf
    while True:
        a, d, dm = assign(x, c, bug)
        gap = min(gap, float(assign_gap(dm).min()))
        if bug != "no_clamp":                      # the reported distances in the direct form: they do not depend on where the centroid sits
            d = ((np.asarray(x, np.float64) - c.astype(np.float64)[a]) ** 2).sum(axis=1)
        if history is not None:
            history.append(float(d.sum()))
        if (t > 0 and np.array_equal(a, prev)) or t == T:
            break
        prev = a
        c = update(x, a, c, bug)
        t += 1
    inertia = float(d.sum())
    if bug == "inertia_updated":
        inertia = float(((np.asarray(x, np.float64) - update(x, a, c).astype(np.float64)[a]) ** 2).sum())
    return dict(centroids=c, assign=a, counts=np.bincount(a, minlength=c.shape[0]).astype(np.int32), inertia=inertia, n_iter=t, assign_gap=gap)


def best_restart(inertia, bug=None):
    inertia = np.asarray(inertia, np.float64)
    return int(inertia.argmax()) if bug == "best_highest" else int(inertia.argmin())


def kmeans(x, K, R, T, seed, bug=None):
    """The whole report's arithmetic: dict(picks, centroids [R,K,L], assign [R,N], counts [R,K], inertia [R], n_iter [R], best, pick_gap)"""
    picks, c0, gap = seed_centres(x, K, R, seed, bug)
    fits = [fit(x, c0[r], T, bug) for r in range(R)]
    out = {k: np.stack([f[k] for f in fits]) for k in ("centroids", "assign", "counts")}
    out.update(inertia=np.array([f["inertia"] for f in fits]), n_iter=np.array([f["n_iter"] for f in fits], np.int32), picks=picks,
               pick_gap=gap, assign_gap=min(f["assign_gap"] for f in fits))
    out["best"] = best_restart(out["inertia"], bug)
    return out


# ---------------------------------------------------------------- contingency, NMI, accuracy
def contingency(a, b, Ka, Kb):
    t = np.zeros((Ka, Kb), np.int64)
    np.add.at(t, (np.asarray(a), np.asarray(b)), 1)
    return t


def nmi(table):
    """2 I(A; B) / (H(A) + H(B)) of an integer contingency table, in float64; 1 when both partitions are trivial."""
    t = np.asarray(table, np.float64)
    n = t.sum()
    if n <= 0:
        return 0.0
    p = t / n
    pa, pb = p.sum(axis=1), p.sum(axis=0)
    ha = -(pa[pa > 0] * np.log(pa[pa > 0])).sum()
    hb = -(pb[pb > 0] * np.log(pb[pb > 0])).sum()
    if ha + hb <= 0:
        return 1.0
    nz = p > 0
    mi = (p[nz] * np.log(p[nz] / np.outer(pa, pb)[nz])).sum()
    return float(max(0.0, 2.0 * mi / (ha + hb)))


def accuracy(table):
    """sum_k max_c table[k][c] / N: every cluster gets its majority class"""
    t = np.asarray(table, np.int64)
    return float(t.max(axis=1).sum()) / int(t.sum()) if t.sum() else 0.0


# ---------------------------------------------------------------- the kernel's fp32 order, emulated
def norms_f32(v):
    """n(v) in sv_knn_classify's order: lane l sums j = l, l + 64, ... ascending (multiply, then add, fp32), then the xor butterfly"""
    v = np.asarray(v, np.float32)
    N, L = v.shape
    lanes = np.zeros((N, 64), np.float32)
    for j in range(L):
        lanes[:, j % 64] = (lanes[:, j % 64] + (v[:, j] * v[:, j]).astype(np.float32)).astype(np.float32)
    o = 32
    while o:
        lanes = (lanes + lanes[:, np.arange(64) ^ o]).astype(np.float32)
        o >>= 1
    return lanes[:, 0]


def distances_f32(x, c, clamp=True):
    """d in fp32 as the tile kernel forms it: the dot product as one fused multiply-add chain over j ascending, then
    (n(x) + n(c)) - 2 dot, clamped at 0"""
    x, c = np.asarray(x, np.float32), np.asarray(c, np.float32)
    acc = np.zeros((x.shape[0], c.shape[0]), np.float32)
    for j in range(x.shape[1]):
        acc = (acc.astype(np.float64) + x[:, j].astype(np.float64)[:, None] * c[:, j].astype(np.float64)[None, :]).astype(np.float32)
    d = ((norms_f32(x)[:, None] + norms_f32(c)[None, :]).astype(np.float32) - (np.float32(2.0) * acc).astype(np.float32)).astype(np.float32)
    return np.maximum(np.float32(0.0), d) if clamp else d


def distance_bound(x, c):
    """[N,K] the derived bound of |d_fp32 - d|: (L + 4) 2^-24 (n(x) + n(c) + 2 |x| |c|)"""
    nx, nc = norms(x), norms(c)
    return (np.asarray(x).shape[1] + 4) * 2.0 ** -24 * (nx[:, None] + nc[None, :] + 2.0 * np.sqrt(nx)[:, None] * np.sqrt(nc)[None, :])


def inertia_bound(x, c, a, exact=False):
    """The bound of |inertia_device - inertia_twin| for the assignment a: the rows' distance bounds (0 where the fp32 distances are
    exact, as on integer data) plus the rounding of N fp64 additions"""
    x = np.asarray(x, np.float64)
    ca = np.asarray(c, np.float64)[a]
    d = np.maximum(0.0, ((x - ca) ** 2).sum(axis=1))
    nx, nc = (x * x).sum(axis=1), (ca * ca).sum(axis=1)
    per_row = 0.0 if exact else ((x.shape[1] + 4) * 2.0 ** -24 * (nx + nc + 2.0 * np.sqrt(nx * nc))).sum()
    return per_row + x.shape[0] * 2.0 ** -53 * d.sum()


# ---------------------------------------------------------------- planted sets and the comparison the host and the device tests share
LATTICES = ((300, 5, 3), (1000, 33, 10), (4099, 128, 10), (777, 130, 64))
LATTICE_SEEDS = {(300, 5, 3): 1, (1000, 33, 10): 2, (4099, 128, 10): 3, (777, 130, 64): 4}


def planted(N, L, K, seed):
    """(x [N,L] float32 with integer entries, labels [N]): centres 16 U{-4..4}^L, offsets U{-2..2}; every cluster has a member"""
    rng = np.random.default_rng(seed)
    centres = 16 * rng.integers(-4, 5, (K, L))
    assert len({tuple(c) for c in centres}) == K
    lab = np.concatenate([np.arange(K), rng.integers(0, K, N - K)])
    rng.shuffle(lab)
    return (centres[lab] + rng.integers(-2, 3, (N, L))).astype(np.float32), lab


def fit_given(x, c0, T, bug=None):
    """R restarts from given centroids c0 [R,K,L]: kmeans()'s dict without the seeding entries"""
    fits = [fit(x, c0[r], T, bug) for r in range(c0.shape[0])]
    out = {k: np.stack([f[k] for f in fits]) for k in ("centroids", "assign", "counts")}
    out.update(inertia=np.array([f["inertia"] for f in fits]), n_iter=np.array([f["n_iter"] for f in fits], np.int32),
               assign_gap=min(f["assign_gap"] for f in fits))
    out["best"] = best_restart(out["inertia"], bug)
    return out


def compare(got, want, x, exact=True):
    """The names of the entries of `got` (a device result or a wrong twin) that do not match the twin's `want`: picks, assign, counts,
    n_iter, best and the centroids bit for bit, the inertia within inertia_bound."""
    bad = []
    for key in ("picks", "assign", "counts", "n_iter", "best"):
        if key in want and key in got and not np.array_equal(np.asarray(got[key]), np.asarray(want[key])):
            bad.append(key)
    if "centroids" in want and "centroids" in got:
        g, w = np.asarray(got["centroids"], np.float32), np.asarray(want["centroids"], np.float32)
        if g.shape != w.shape or not np.array_equal(g.view(np.uint32), w.view(np.uint32)):
            bad.append("centroids")
    if "inertia" in want and "inertia" in got:
        for r in range(len(want["inertia"])):
            tol = inertia_bound(x, want["centroids"][r], want["assign"][r], exact)
            if not abs(float(got["inertia"][r]) - float(want["inertia"][r])) <= tol:
                bad.append("inertia[%d]" % r)
    return bad


# ---------------------------------------------------------------- the cases both test files run
def trap_set():
    """The (300, 5, 3) lattice plus rows that expose wrong kernels: two zero rows (nearer to a zero-padded column than to any
    centroid), and start centroids [3, 4, 5] whose restart 0 holds one centroid twice (exact ties at t = 0) and one far away from
    every row (a cluster that stays empty and keeps its centroid)."""
    x, _ = planted(300, 5, 3, LATTICE_SEEDS[(300, 5, 3)])
    x = np.concatenate([x, np.zeros((2, 5), np.float32), x[:7]])
    c0 = np.stack([x[[3, 3, 50, 120]], x[[10, 60, 200, 250]], x[[5, 6, 7, 8]]]).astype(np.float32)
    c0[0, 3] = 1000.0
    return x, c0


def equal_rows(exact=True):
    """40 equal rows: every distance is 0, every race key +inf.  exact: small integers, whose fp32 arithmetic is exact in any order;
    otherwise 70 non-dyadic values whose fp32 expansion n + n - 2 dot comes out at -1.5e-5 (distances_f32): 0 only by the clamp."""
    v = np.arange(1, 8) if exact else np.random.default_rng(1).uniform(0.5, 1.5, 70)
    return np.tile(v.astype(np.float32), (40, 1))


def cases():
    out = []
    for shape in LATTICES:
        x, lab = planted(*shape, LATTICE_SEEDS[shape])
        out.append(dict(name="lattice-%d-%d-%d" % shape, kind="kmeans", x=x, labels=lab, K=shape[2], R=4, T=20, seed=LATTICE_SEEDS[shape],
                        big=shape[0] > 2000))
    x, c0 = trap_set()
    for T in (0, 6):
        out.append(dict(name="trap-T%d" % T, kind="fit", x=x, c0=c0, T=T, big=False))
    out.append(dict(name="equal-rows", kind="seed", x=equal_rows(), K=4, R=2, seed=7, big=False))
    out.append(dict(name="equal-rows-roundoff", kind="seed", x=equal_rows(False), K=4, R=2, seed=7, big=False, host_only=True))
    return out


def run_case(case, bug=None):
    if case["kind"] == "kmeans":
        return kmeans(case["x"], case["K"], case["R"], case["T"], case["seed"], bug)
    if case["kind"] == "fit":
        return fit_given(case["x"], case["c0"], case["T"], bug)
    return dict(picks=seed_centres(case["x"], case["K"], case["R"], case["seed"], bug)[0])
