"""Float64 twins of the sample-quality report (include/splitvae.h: sv_prdc_radius / sv_prdc_count; split_vae_amd/sample_quality.py), the
cases the GPU tests run and the comparisons they make.  tests/test_sample_quality_host.py applies mutants to the twins and checks that
the same comparisons on the same cases reject each of them; tests/test_gpu_sample_quality.py holds the device to the twins.

`mutant` names a deliberate mistake:
  count    'lt' (< in place of <=), 'rad_of_query' (the radius of the query's index, not of the reference column), 'no_norm_r' (the norm
           of r dropped from the distance), 'min_tie_high' (the highest index that attains the minimum), 'plain_vs_squared' (the radius
           square-rooted before the compare)
  radius   'self_counted' (self is a neighbour), 'k_plus_1' (the (k+1)-th), 'self_by_zero' (every zero-distance row dropped, not index i)
  figures  'coverage_fake_radius' (coverage against rad_Y), 'recall_precision_swapped', 'density_no_k' (no division by k)
"""
import numpy as np

from swap_ref import lattice_rows

COUNT_MUTANTS = ("lt", "rad_of_query", "no_norm_r", "min_tie_high", "plain_vs_squared")
RADIUS_MUTANTS = ("self_counted", "k_plus_1", "self_by_zero")
FIGURE_MUTANTS = ("coverage_fake_radius", "recall_precision_swapped", "density_no_k")


# ---------------------------------------------------------------- the twins
def distances(Q, R, mutant=None):
    """d [Nq, Nr] = max(0, (n(q) + n(r)) - 2 q . r) in float64 (swap_ref.distances)"""
    Q, R = np.asarray(Q, np.float64), np.asarray(R, np.float64)
    nq, nr = (Q * Q).sum(axis=1), (R * R).sum(axis=1)
    if mutant == "no_norm_r":
        nr = np.zeros_like(nr)
    return np.maximum(0.0, (nq[:, None] + nr[None, :]) - 2.0 * (Q @ R.T))


def radius(X, k, mutant=None):
    """rad [N]: the k-th smallest VALUE of {d(i, j) : j != i} (a sort of the values alone: the index order cannot matter to it)"""
    d = distances(X, X)
    N = d.shape[0]
    out = np.zeros(N, np.float64)
    for i in range(N):
        others = np.ones(N, bool)
        if mutant == "self_by_zero":
            others = d[i] != 0.0
        elif mutant != "self_counted":
            others[i] = False
        vals = np.sort(d[i][others])
        kk = k + 1 if mutant == "k_plus_1" else k
        out[i] = vals[min(kk, vals.size) - 1] if vals.size else 0.0      # (a mutant may run out of rows: its last one)
    return out


def radius_by_argsort(X, k):
    """The same radii restated: the stable (distance, index) order of the row with index i struck out, entry k - 1"""
    d = distances(X, X)
    out = np.zeros(d.shape[0], np.float64)
    for i in range(d.shape[0]):
        order = [j for j in np.argsort(d[i], kind="stable") if j != i]
        out[i] = d[i, order[k - 1]]
    return out


def count(Q, R, rad, mutant=None):
    """(cnt [Nq] int64, dmin [Nq] float64, imin [Nq] int64): cnt[q] = #{j : d(q, j) <= rad[j]}, the minimum and the lowest j attaining it"""
    d = distances(Q, R, mutant)
    rad = np.asarray(rad, np.float64)
    Nq, Nr = d.shape
    if mutant == "plain_vs_squared":
        rad = np.sqrt(rad)
    cnt, dmin, imin = np.zeros(Nq, np.int64), np.zeros(Nq, np.float64), np.zeros(Nq, np.int64)
    for q in range(Nq):
        r = np.full(Nr, rad[q % Nr]) if mutant == "rad_of_query" else rad
        cnt[q] = int((d[q] < r).sum() if mutant == "lt" else (d[q] <= r).sum())
        dmin[q] = d[q].min()
        at = np.nonzero(d[q] == dmin[q])[0]
        imin[q] = at[-1] if mutant == "min_tie_high" else at[0]
    return cnt, dmin, imin


def count_by_loops(Q, R, rad):
    """The same outputs restated element by element in Python"""
    d = distances(Q, R)
    out = []
    for q in range(d.shape[0]):
        c, best, where = 0, None, -1
        for j in range(d.shape[1]):
            c += 1 if d[q, j] <= float(rad[j]) else 0
            if best is None or d[q, j] < best:
                best, where = d[q, j], j
        out.append((c, best, where))
    return (np.array([o[0] for o in out], np.int64), np.array([o[1] for o in out], np.float64), np.array([o[2] for o in out], np.int64))


def figures(cnt_fake, cnt_real, dmin_real, rad_real, rad_fake, k, mutant=None):
    """precision, recall, density, coverage (sample_quality.py's definitions) in plain Python"""
    cf, cr = [int(v) for v in cnt_fake], [int(v) for v in cnt_real]
    M, N = float(len(cf)), float(len(cr))
    prec, rec = sum(v > 0 for v in cf) / M, sum(v > 0 for v in cr) / N
    if mutant == "recall_precision_swapped":
        prec, rec = rec, prec
    dens = sum(cf) / (M if mutant == "density_no_k" else k * M)
    r = rad_fake if mutant == "coverage_fake_radius" else rad_real
    cov = sum(float(dmin_real[i]) <= float(r[i]) for i in range(len(cr))) / N
    return dict(precision=prec, recall=rec, density=dens, coverage=cov)


def moments(X):
    X = np.asarray(X, np.float64)
    m = X.mean(axis=0)
    return m, (X - m).T @ (X - m) / X.shape[0]


def frechet(ma, Ca, mb, Cb):
    """|m_a - m_b|^2 + tr C_a + tr C_b - 2 tr (C_a C_b)^(1/2) through the eigenvalues of the product C_a C_b itself (they are those of
    C_a^(1/2) C_b C_a^(1/2)): another route than the report's two symmetric eigenproblems"""
    ma, mb, Ca, Cb = (np.asarray(v, np.float64) for v in (ma, mb, Ca, Cb))
    lam = np.linalg.eigvals(Ca @ Cb).real
    return float(((ma - mb) ** 2).sum() + np.trace(Ca) + np.trace(Cb) - 2.0 * np.sqrt(np.maximum(lam, 0.0)).sum())


# ---------------------------------------------------------------- the comparisons
def exact(got, want):
    """the lattice comparison: bit for bit (a float compares by value: every lattice figure is an integer below 2^24)"""
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and bool((got.astype(np.float64) == want.astype(np.float64)).all())


def counts_equal(got, want):
    return all(exact(g, w) for g, w in zip(got, want))


def pair_eps(Q, R):
    """eps [Nq, Nr]: swap_ref.rank_bracket's bound on the error of one device distance, 1.01 u ((K + 2)(n(q) + n(r)) + 2 (L + 5) sum_j
    |q_j r_j|), u = 2^-24, K = ceil(L / 64) + 6 (derived there from the operations as they run)"""
    Q, R = np.asarray(Q, np.float64), np.asarray(R, np.float64)
    L = Q.shape[1]
    nq, nr = (Q * Q).sum(axis=1), (R * R).sum(axis=1)
    K = -(-L // 64) + 6
    return 1.01 * 2.0 ** -24 * ((K + 2) * (nq[:, None] + nr[None, :]) + 2.0 * (L + 5) * (np.abs(Q) @ np.abs(R).T))


def count_bracket(Q, R, rad):
    """(lo, hi) [Nq]: lo = #{d <= rad - eps}, hi = #{d <= rad + eps}: the counts every fp32 evaluation of the tile may give"""
    d, eps, rad = distances(Q, R), pair_eps(Q, R), np.asarray(rad, np.float64)
    return (d <= rad[None, :] - eps).sum(axis=1), (d <= rad[None, :] + eps).sum(axis=1)


def counts_in_bracket(got, lo, hi, want):
    got = np.asarray(got, np.int64)
    decided = lo == hi
    return bool(((got >= lo) & (got <= hi)).all()) and bool((got[decided] == np.asarray(want)[decided]).all())


def undecided_share(lo, hi):
    return float(np.mean(hi > lo))


def within(got, want, tol):
    """an order statistic (a minimum, a k-th smallest) is 1-Lipschitz in the sup norm: |got - want| <= tol, tol = the row's max eps"""
    return bool((np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)) <= tol).all())


def nearest_ok(Q, R, imin, want_dmin):
    """d_twin(q, imin) <= dmin_twin + 2 max_j eps(q, j)"""
    d, eps = distances(Q, R), pair_eps(Q, R)
    imin = np.asarray(imin, np.int64)
    if ((imin < 0) | (imin >= d.shape[1])).any():
        return False
    return bool((d[np.arange(d.shape[0]), imin] <= np.asarray(want_dmin) + 2.0 * eps.max(axis=1)).all())


# ---------------------------------------------------------------- lattice cases
def count_shapes(c):
    """(Nq, Nr, L, pad_q, pad_r, off) with c = sv_prdc_chunk_rows(): the shapes the contract names"""
    return [(1, 1, 1, 0, 0, 0), (63, 2, 3, 5, 0, 0), (64, 64, 31, 0, 3, 1), (65, 65, 32, 0, 0, 0), (130, c - 1, 33, 7, 1, 3),
            (64, c, 128, 0, 0, 0), (65, c + 1, 256, 4, 4, 0), (130, 2 * c + 3, 33, 0, 0, 0), (1, 65, 512, 0, 0, 2)]


def count_case(Nq, Nr, L, seed):
    """dict(Q, R, rad): integer rows (every sum exact in fp32); rad[j] is the distance of a random query from reference j, so some
    distance equals a radius exactly.  With Nq, Nr >= 3: reference 0 has radius 0 and query 0 duplicates it (0 <= 0 counts); query 1 lies
    far outside the lattice (count 0); references a < b are duplicates and query 2 equals them (a two-way tie of the minimum, at least)."""
    rng = np.random.default_rng(seed)
    R, Q = lattice_rows(rng, Nr, L), lattice_rows(rng, Nq, L)
    if Nq >= 3 and Nr >= 3:
        Q[0] = R[0]
        Q[1] = 12.0 * np.where(np.arange(L) % 2, -1.0, 1.0)
        a, b = Nr // 3, Nr - 1
        R[b] = R[a]
        Q[2] = R[a]
    d = distances(Q, R)
    pick = rng.integers(0, Nq, size=Nr)
    if Nq >= 3 and Nr >= 3:
        pick[pick == 1] = 2                            # no radius reaches the far query
    rad = d[pick, np.arange(Nr)].astype(np.float32)
    if Nq >= 3 and Nr >= 3:
        rad[0] = 0.0
    return dict(Q=Q, R=R, rad=rad)


def radius_shapes(c):
    """(N, L, k, pad, off): N in {k + 1, 64, 65, c + 1} x k in {1, 5, 31}, L cycling through {3, 33, 256}"""
    out, Ls = [], (3, 33, 256)
    for k in (1, 5, 31):
        for n, N in enumerate((k + 1, 64, 65, c + 1)):
            out.append((N, Ls[(len(out)) % 3], k, (0, 3, 0, 5)[n], (0, 1, 0, 2)[n]))
    return out


def radius_case(N, L, seed):
    """X [N, L] integer rows; with N >= 3 row mid has a duplicate at row 0 and at row N - 1 (a lower and a higher index)"""
    rng = np.random.default_rng(seed)
    X = lattice_rows(rng, N, L)
    if N >= 3:
        X[0] = X[N // 2]
        X[N - 1] = X[N // 2]
    return X


# ---------------------------------------------------------------- Gaussian cases
GAUSS_SHAPES = [(130, 300, 32, 5), (65, 4099, 128, 5), (257, 2049, 256, 3), (130, 300, 33, 1), (64, 64, 7, 31)]      # (Nq, Nr, L, k)
GAUSS_SEED = 11
UNDECIDED_CAP = 0.02                               # swap's cap
POSITIVE_SHARE = (0.2, 0.9)                        # the share of queries with a positive count: strictly inside


def gaussian_case(Nq, Nr, L, k, seed=GAUSS_SEED):
    """Data on a 6-dimensional subspace embedded in L (isotropic noise in 128+ dimensions gives all-zero counts and tests nothing): ten
    cluster centres; the references fall into the first seven with noise 0.5, the queries into all ten with noise 0.7, and those three lie
    three times as far out, so a share of the queries lies where no reference ball reaches, however large k is.  rad: the float64 k-NN radii of the references cast to fp32 -- the one array
    both the device and the twin are fed."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((6, L)) / np.sqrt(L)
    centres = 4.0 * rng.standard_normal((10, 6))
    centres[7:] *= 3.0                             # the clusters without references lie outside the references' hull: k = 31 of 64 balls miss them
    R = ((centres[rng.integers(0, 7, size=Nr)] + 0.5 * rng.standard_normal((Nr, 6))) @ A).astype(np.float32)
    Q = ((centres[rng.integers(0, 10, size=Nq)] + 0.7 * rng.standard_normal((Nq, 6))) @ A).astype(np.float32)
    return dict(Q=Q, R=R, k=k, rad=radius(R, k).astype(np.float32))
