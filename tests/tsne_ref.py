"""float64 NumPy twin of sv_tsne_* (include/splitvae.h): the beta search and the conditional rows over given fp32 distances, the
joint P, the Philox initial map, the pair sums, KL, gradient and the delta-bar-delta update, the neighbour scores; a float32
emulation of the kernels' summation order (fp32 partials per (row, chunk), fp64 folds); the per-element bounds derived from the
arithmetic; and BUGS, the deliberately wrong kernels (every function takes `bug=`) the tests must reject.

Bounds, with u = 2^-24 (half an ulp of fp32).  A pair term is a product of rounded factors: dx = fl(y_i - y_j) (u), q = fl(fl(1 + dx^2)
+ dy^2) (4 u: positive terms), w = v_rcp_f32(q) (1 ulp = 2 u, so 6 u), P w (7 u), (P w) dx (9 u), w w (13 u), (w w) dx (15 u); a lane adds
16 terms and the butterfly 6 more: 22 u of the sum of the absolute terms.  The constants below round these up: C_A = 32, C_R = 40,
C_Z = 32 (units of u, times the sum of the absolute terms).  The log term P log2 q: v_log_f32 is good to 1 ulp of the result and sees q with
4 u, so its absolute error is at most 4 u / ln 2 + 2 u |log2 q|: C_L = 32 on sum |P log2 q| plus 8 u sum P.  The fp64 folds add 1e-15
relative.  Everything downstream (Z, KL, g, gain, inc, Y, the column means) propagates these by the formulas in step_bounds(), where every rounding of
the update itself (at most u of its result each) is counted twice: the float32 restatement must stay within half of each bound."""
import numpy as np

TS_KEY = 0x1a7e475e3a9
TS_TAG = 0x74730000
CHUNK = 1024                                      # sv_tsne_chunk_rows()
BETA_STEPS = 100
BETA_MIN, BETA_MAX = 2.0 ** -60, 2.0 ** 60
FLT_MAX = float(np.finfo(np.float32).max)
U = 2.0 ** -24
C_A, C_R, C_Z, C_L = 32.0, 40.0, 32.0, 32.0
BUGS = ("drop4", "rep_w", "z_half", "kl_exag", "gain_inverted", "no_recentre", "self_kept", "sym_over_n", "momentum_late", "exag_late",
        "self_in_lists", "vote_tie_high", "gain_no_floor", "entropy_bits")
DEFAULTS = dict(exag=12.0, exag_iters=250, eta=200.0)


# ---------------------------------------------------------------- Philox4x32-10 and the initial map
def philox4x32(seed, c0, c1, c2, c3):
    """The four output words of Philox4x32-10 at counter (c0, c1, c2, c3) under the 64-bit key `seed`; the counters may be arrays."""
    m32 = np.uint64(0xFFFFFFFF)
    c = [np.atleast_1d(np.asarray(v, np.uint64)) & m32 for v in (c0, c1, c2, c3)]
    n = max(v.size for v in c)
    c = [np.broadcast_to(v, (n,)).copy() for v in c]
    a, b = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ a) & m32, p1 & m32, ((p0 >> np.uint64(32)) ^ c[3] ^ b) & m32, p0 & m32]
        a, b = (a + np.uint64(0x9E3779B9)) & m32, (b + np.uint64(0xBB67AE85)) & m32
    return c


def unit_open(w):
    return ((np.asarray(w, np.uint64) >> np.uint64(8)).astype(np.float64) + 1.0) / 16777216.0


def init_map(N, seed):
    """(Y0 [N,2] float64, bound [N,2]): 1e-4 * sqrt(-2 log u1) cos(2 pi u2) of the counter (c, i, tag, 0).  The bound: the radius to 4 u
    (logf, sqrtf), the cosine's argument to 2 pi u (one fp32 product) and the cosine itself to 2 u, the two products to 2 u."""
    i = np.repeat(np.arange(N, dtype=np.uint64), 2)
    cc = np.tile(np.arange(2, dtype=np.uint64), N)
    w = philox4x32(seed ^ TS_KEY, cc, i, TS_TAG, 0)
    r = np.sqrt(-2.0 * np.log(unit_open(w[0])))
    y = 1e-4 * r * np.cos(2.0 * np.pi * unit_open(w[1]))
    bound = 1e-4 * (r * (2.0 * np.pi * U + 2.0 * U) + np.abs(r) * 6.0 * U) + 2.0 ** -149
    return y.reshape(N, 2), bound.reshape(N, 2) * 1.5


# ---------------------------------------------------------------- distances (an fp32 restatement for the CPU tests; the GPU tests take the device's)
def distances_f32(x):
    """sv_knn_classify's distance in fp32: norms, an fma chain over L in ascending order, max(0, (n_i + n_j) - 2 dot)"""
    x = np.asarray(x, np.float32)
    n = np.zeros(x.shape[0], np.float32)
    for j in range(x.shape[1]):
        n = n + x[:, j] * x[:, j]
    dot = np.zeros((x.shape[0], x.shape[0]), np.float32)
    for j in range(x.shape[1]):
        dot = (dot.astype(np.float64) + np.outer(x[:, j].astype(np.float64), x[:, j].astype(np.float64))).astype(np.float32)
    return np.maximum(np.float32(0), (n[:, None] + n[None, :]) - np.float32(2) * dot)


# ---------------------------------------------------------------- conditional rows and the joint P
def _row_terms(D, bug=None):
    D = np.asarray(D, np.float32).astype(np.float64)
    D = np.where(D <= FLT_MAX, D, FLT_MAX)        # NaN and +inf count as FLT_MAX
    N = D.shape[0]
    off = ~np.eye(N, dtype=bool)
    dmin = np.where(off, D, np.inf).min(axis=1)
    dd = D - dmin[:, None]
    if bug == "self_kept":
        dd[~off] = 0.0                             # the row itself stays in the sums, at the minimum
        off = np.ones_like(off)
    return dd, off


def entropy(dd, off, beta, bits=False):
    """(H [N], S [N], e [N,N]) of the rows at beta [N]"""
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.where(off, np.exp(-beta[:, None] * np.where(off, dd, 0.0)), 0.0)
        S = e.sum(axis=1)
        T = (e * np.where(off, dd, 0.0)).sum(axis=1)
        H = np.log(S) + beta * T / S
    return (H / np.log(2.0) if bits else H), S, e


def search_beta(D, perplexity, bug=None):
    """The header's search: 100 steps from beta = 1, doubling / halving while a side is unbounded, clamped.  -> (beta [N], H [N], has_root [N])"""
    dd, off = _row_terms(D, bug)
    N = dd.shape[0]
    target = np.log(perplexity)
    beta = np.ones(N)
    lo, hi = np.zeros(N), np.zeros(N)
    have_lo, have_hi = np.zeros(N, bool), np.zeros(N, bool)
    for _ in range(BETA_STEPS):
        H = entropy(dd, off, beta, bits=bug == "entropy_bits")[0]
        up = H > target
        lo = np.where(up, beta, lo); have_lo |= up
        hi = np.where(~up, beta, hi); have_hi |= ~up
        mid = 0.5 * (lo + hi)
        beta = np.where(up, np.where(have_hi, mid, beta * 2.0), np.where(have_lo, mid, beta * 0.5))
        beta = np.clip(beta, BETA_MIN, BETA_MAX)
    H = entropy(dd, off, beta)[0]
    m = (np.where(off, dd, 1.0) == 0.0).sum(axis=1)
    has_root = (m < perplexity) & (beta > BETA_MIN) & (beta < BETA_MAX)
    return beta, H, has_root


def conditional(D, beta, bug=None):
    """p(j|i) as the device stores it: float32 of e_j / S at the given beta; p(i|i) = 0 (unless the bug keeps it)"""
    dd, off = _row_terms(D, bug)
    _, S, e = entropy(dd, off, np.asarray(beta, np.float64))
    return (e / S[:, None]).astype(np.float32)


def joint(cond, bug=None):
    c = np.asarray(cond, np.float32).astype(np.float64)
    N = c.shape[0]
    P = ((c + c.T) / ((1.0 if bug == "sym_over_n" else 2.0) * N)).astype(np.float32)
    if bug != "self_kept":
        np.fill_diagonal(P, 0.0)
    return P


def p_bounds(cond, N):
    """(bound of a conditional entry, bound of a joint entry) given the twin's float32 conditional rows: the fp64 quotient is good to 1e-12
    relative (exp's argument to 2^-53 |arg|, |arg| < 750; N additions), so the fp32 rounding may land on the neighbouring value: one ulp
    (2^-23 relative) or one denormal step; the joint entry adds the two, divides and rounds once more."""
    c = np.asarray(cond, np.float64)
    bc = 2.0 ** -23 * c + 2.0 ** -149
    bj = (bc + bc.T) / (2.0 * N) + 2.0 ** -23 * (c + c.T) / (2.0 * N) + 2.0 ** -149
    return bc, bj


def p_const(P):
    P = np.asarray(P, np.float64)
    nz = P > 0
    return np.array([P.sum(), (P[nz] * np.log(P[nz])).sum()])


def affinities(x_or_D, perplexity, is_D=False, bug=None):
    D = np.asarray(x_or_D, np.float32) if is_D else distances_f32(x_or_D)
    beta, H, has_root = search_beta(D, perplexity, bug)
    cond = conditional(D, beta, bug)
    return dict(D=D, beta=beta, H=H, has_root=has_root, cond=cond, P=joint(cond, bug))


# ---------------------------------------------------------------- pair sums, gradient, update
def pair_sums(P, Y, bug=None):
    """float64: A [N,2], R [N,2], z [N], l [N] (natural log) and the sums of the absolute terms sA, sR, sL for the bounds"""
    P = np.asarray(P, np.float64)
    Y = np.asarray(Y, np.float64)
    dx = Y[:, None, :] - Y[None, :, :]
    q = 1.0 + (dx * dx).sum(axis=2)
    w = 1.0 / q
    np.fill_diagonal(w, 0.0)
    pw = P * w
    ww = w if bug == "rep_w" else w * w
    A = (pw[:, :, None] * dx).sum(axis=1)
    R = (ww[:, :, None] * dx).sum(axis=1)
    z = w.sum(axis=1)
    lq = np.where(P > 0, P * np.log(q), 0.0)
    return dict(A=A, R=R, z=z, l=lq.sum(axis=1), sA=(pw[:, :, None] * np.abs(dx)).sum(axis=1), sR=(ww[:, :, None] * np.abs(dx)).sum(axis=1),
                sL=np.abs(lq).sum(axis=1), sP=P.sum(axis=1))


def pair_sums_f32(P, Y):
    """The kernels' order in float32: lane l of 64 takes the columns l, l + 64, ... of a chunk of CHUNK columns, then the xor butterfly; the
    chunks in fp64 in chunk order.  (v_rcp_f32 and v_log_f32 are modelled by the correctly rounded values.)"""
    f = np.float32
    P = np.asarray(P, f)
    Y = np.asarray(Y, f)
    N = P.shape[0]
    nch = (N + CHUNK - 1) // CHUNK
    Np = nch * CHUNK
    Pp = np.zeros((N, Np), f); Pp[:, :N] = P
    Yp = np.zeros((Np, 2), f); Yp[:N] = Y
    valid = np.zeros((N, Np), bool); valid[:, :N] = True
    valid[np.arange(N), np.arange(N)] = False
    dx = Y[:, None, 0] - Yp[None, :, 0]
    dy = Y[:, None, 1] - Yp[None, :, 1]
    q = (f(1) + dx * dx) + dy * dy
    w = np.where(valid, (f(1) / q).astype(f), f(0))
    pw, ww = Pp * w, w * w
    terms = [pw * dx, pw * dy, ww * dx, ww * dy, w, np.where(Pp > 0, Pp * np.log2(q).astype(f), f(0))]
    out = np.zeros((6, N))
    lanes = np.arange(64)
    for k, t in enumerate(terms):
        t = t.reshape(N, nch, CHUNK // 64, 64)
        acc = np.zeros((N, nch, 64), f)
        for m in range(CHUNK // 64):
            acc = acc + t[:, :, m, :]
        for o in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[:, :, lanes ^ o]
        part = acc[:, :, 0].astype(np.float64)
        s = np.zeros(N)
        for c in range(nch):
            s = s + part[:, c]
        out[k] = s
    return dict(A=out[0:2].T.copy(), R=out[2:4].T.copy(), z=out[4], l=out[5] * np.log(2.0))


def _ordered_total(v):
    """rows in groups of 256: the group's rows in order, then the groups in order"""
    v = np.asarray(v, np.float64)
    tot = 0.0
    for o in range(0, v.shape[0], 256):
        s = 0.0
        for t in v[o:o + 256]:
            s += t
        tot += s
    return tot


def step(P, pc, state, t, exag=12.0, exag_iters=250, eta=200.0, bug=None, emulate=False):
    """One iteration from state = dict(Y, inc, gain) at counter t.  -> dict(Y, inc, gain, Z, KL, g, sums).  emulate: the float32 restatement."""
    f = np.float32
    Y, inc, gain = (np.asarray(state[k], f) for k in ("Y", "inc", "gain"))
    N = Y.shape[0]
    s = pair_sums_f32(P, Y) if emulate else pair_sums(P, Y, bug)
    Z = _ordered_total(s["z"]) if emulate else float(s["z"].sum())
    Lw = _ordered_total(s["l"]) if emulate else float(s["l"].sum())
    if bug == "z_half":
        Z *= 0.5
    early = t < exag_iters + (1 if bug == "exag_late" else 0)
    e = exag if early else 1.0
    mom = 0.5 if t < exag_iters + (1 if bug == "momentum_late" else 0) else 0.8
    if bug == "kl_exag":
        KL = e * pc[1] + e * pc[0] * np.log(e) + e * Lw + np.log(Z) * e * pc[0]
    else:
        KL = pc[1] + Lw + np.log(Z) * pc[0]
    g = (1.0 if bug == "drop4" else 4.0) * (e * s["A"] - s["R"] / Z)
    if emulate:
        g32 = g.astype(f)
        flip = (g32 > 0) != (inc > 0)
        ga = np.maximum(np.where(flip, gain + f(0.2), gain * f(0.8)), f(0.01))
        inn = f(mom) * inc - (f(eta) * ga) * g32
        yn = Y + inn
        m = np.array([_ordered_total(yn[:, 0]), _ordered_total(yn[:, 1])]) / N
        yn = yn - m.astype(f)[None, :]
        return dict(Y=yn, inc=inn, gain=ga, Z=Z, KL=KL, g=g, sums=s)
    g32 = g.astype(f).astype(np.float64)          # the header rounds g to fp32 before the update
    flip = (g32 > 0) != (inc > 0)
    if bug == "gain_inverted":
        flip = ~flip
    ga = np.where(flip, gain.astype(np.float64) + 0.2, gain.astype(np.float64) * 0.8)
    if bug != "gain_no_floor":
        ga = np.maximum(ga, 0.01)
    inn = mom * inc.astype(np.float64) - eta * ga * g32
    yn = Y.astype(np.float64) + inn
    mean = yn.mean(axis=0)
    if bug != "no_recentre":
        yn = yn - mean[None, :]
    return dict(Y=yn, inc=inn, gain=ga, Z=Z, KL=KL, g=g, sums=s, mean=mean, mom=mom, e=e)


def step_bounds(res, state, pc, eta=200.0):
    """Per-element bounds of one device iteration against the twin's `res` (see the module docstring).  Also `g_gap`: the smallest
    |g| / (bound of g) over the components with a non-zero bound -- above 2, no sign decision of the gain rule is within rounding."""
    s, Z, e, mom = res["sums"], res["Z"], res["e"], res["mom"]
    dA, dR, dz = C_A * U * s["sA"] + 1e-300, C_R * U * s["sR"] + 1e-300, C_Z * U * s["z"]
    dZ = dz.sum() + 1e-15 * Z
    dL = (C_L * U * s["sL"] + 8.0 * U * s["sP"]).sum() + 1e-15 * np.abs(s["l"]).sum()
    g = res["g"]
    dg = 4.0 * (e * dA + dR / Z + np.abs(s["R"]) * dZ / Z ** 2) + 2.0 * U * np.abs(g)
    nz = dg > 1e-290
    gap = float((np.abs(g[nz]) / dg[nz]).min()) if nz.any() else np.inf
    ga, inn = np.abs(res["gain"]), res["inc"]
    dgain = 4.0 * U * ga
    minc = mom * np.abs(np.asarray(state["inc"], np.float64))
    dinc = eta * ga * dg + eta * np.abs(g) * dgain + 8.0 * U * (minc + eta * ga * np.abs(g)) + 2.0 ** -149
    ypre = np.abs(np.asarray(state["Y"], np.float64) + inn)
    dpre = dinc + 2.0 * U * ypre
    dmean = dpre.mean(axis=0) + 2.0 * U * np.abs(res["mean"]) + 1e-15 * ypre.mean(axis=0)
    dY = dpre + dmean[None, :] + 2.0 * U * np.abs(res["Y"]) + 2.0 ** -149
    dKL = dL + dZ / Z * pc[0] + 1e-12 * (abs(pc[1]) + np.abs(s["l"]).sum() + abs(np.log(Z)) * pc[0])
    return dict(Y=dY, inc=dinc, gain=dgain, Z=dZ, KL=dKL, g=dg, g_gap=gap)


def check_step(got, res, b, scale=1.0):
    """[] when got (Y, inc, gain, Z, KL) lies within scale * the bounds of the twin's result, else what does not; `worst` error / bound"""
    bad, worst = [], 0.0
    for k in ("Y", "inc", "gain", "Z", "KL"):
        err = np.abs(np.asarray(got[k], np.float64) - np.asarray(res[k], np.float64))
        lim = scale * np.asarray(b[k], np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(err > 0, err / np.maximum(np.asarray(b[k], np.float64), 1e-300), 0.0)
        worst = max(worst, float(np.max(ratio)))
        if not np.all(err <= lim) or not np.all(np.isfinite(np.asarray(got[k], np.float64))):
            bad.append((k, float(np.max(ratio))))
    return bad, worst


def run(P, pc, N, T, seed, exag=12.0, exag_iters=250, eta=200.0, emulate=False, bug=None, state=None, t0=0):
    """T iterations from sv_tsne_init's state (or `state` at counter t0) -> dict(Y, inc, gain, kl [T])"""
    if state is None:
        y0 = init_map(N, seed)[0].astype(np.float32)
        state = dict(Y=y0, inc=np.zeros((N, 2), np.float32), gain=np.ones((N, 2), np.float32))
    kl = []
    for t in range(t0, t0 + T):
        r = step(P, pc, state, t, exag, exag_iters, eta, bug=bug, emulate=emulate)
        kl.append(r["KL"])
        state = dict(Y=r["Y"], inc=r["inc"], gain=r["gain"])
    return dict(state, kl=np.array(kl))


def auto_eta(N, exag):
    return max(N / exag / 4.0, 50.0)


# ---------------------------------------------------------------- neighbour lists and scores
def knn_lists(v, k1):
    """[N,k1] int32: the k1 nearest rows of v to each row under (d, index), d = the squared distance in float64 (self included)"""
    v = np.asarray(v, np.float64)
    d = ((v[:, None, :] - v[None, :, :]) ** 2).sum(axis=2)
    return np.argsort(d, axis=1, kind="stable")[:, :k1].astype(np.int32)


def neighbour_scores(nn_lat, nn_map, labels=None, n_class=0, bug=None):
    """[3] int: latent neighbours kept in the map, map k-NN hits, latent k-NN hits.  Self = the first entry with index i, else the last."""
    nn_lat, nn_map = np.asarray(nn_lat), np.asarray(nn_map)
    N, k1 = nn_lat.shape

    def others(row, i):
        row = [int(v) for v in row]
        if bug == "self_in_lists":
            return [v for v in row[:k1 - 1] if 0 <= v < N]
        pos = row.index(i) if i in row else k1 - 1
        return [v for p, v in enumerate(row) if p != pos and 0 <= v < N]

    def vote(idx):
        votes = np.bincount([int(labels[j]) for j in idx if labels[j] < n_class], minlength=n_class)[:n_class]
        if bug == "vote_tie_high":
            return int(n_class - 1 - votes[::-1].argmax())
        return int(votes.argmax())                 # the first maximum: ties to the lowest class id

    out = [0, 0, 0]
    for i in range(N):
        a, b = others(nn_lat[i], i), others(nn_map[i], i)
        out[0] += sum(1 for v in a if v in b)
        if labels is not None:
            out[1] += int(vote(b) == int(labels[i]))
            out[2] += int(vote(a) == int(labels[i]))
    return out


# ---------------------------------------------------------------- the shared cases
def clusters(N, L, n_clusters=4, sep=10.0, seed=0, scale=1.0):
    """Gaussian clusters, centres `sep` sigma apart along random directions -> (x [N,L] float32, labels [N] uint8)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    cen = rng.standard_normal((n_clusters, L))
    cen = cen / np.maximum(np.linalg.norm(cen, axis=1, keepdims=True), 1e-12) * sep * (np.arange(n_clusters)[:, None] + 1.0) / np.sqrt(2.0)
    lab = (np.arange(N) % n_clusters).astype(np.uint8)
    x = cen[lab] + rng.standard_normal((N, L))
    return (x * scale).astype(np.float32), lab


def planted_map(N=256, L=16, seed=0, minor=0.1):
    """Four Gaussian clusters whose centres lie 10 sigma apart (sigma = 1 along the first two axes, `minor` along the rest: a cluster is
    a thin 2-D sheet, so a 2-D map can keep its neighbours).  On seeds 0 .. 3 the twin and the float32 restatement both reach a
    leave-one-out 5-NN accuracy of 1.0 and keep 0.76 .. 0.80 of the 5 latent neighbours after 300 iterations (isotropic clusters keep
    0.41 .. 0.47 and leave one or two stragglers: the conditions of the map test cannot be relied on there)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    cen = rng.standard_normal((4, L))
    cen = cen / np.linalg.norm(cen, axis=1, keepdims=True) * 10.0 / np.sqrt(2.0)
    lab = (np.arange(N) % 4).astype(np.uint8)
    std = np.full(L, minor)
    std[:2] = 1.0
    return (cen[lab] + rng.standard_normal((N, L)) * std[None, :]).astype(np.float32), lab


def affinity_cases():
    """(name, x, perplexity, pad, off): the edge shapes of the GPU test; `chunk1` is N = sv_tsne_chunk_rows() + 1"""
    out = []
    for N, L, perp, pad, off in ((4, 1, 1.5, 0, 0), (5, 2, 2.0, 3, 1), (63, 3, 10.0, 0, 0), (64, 33, 15.0, 5, 3), (65, 128, 20.0, 0, 2),
                                 (257, 33, 30.0, 1, 0), (CHUNK + 1, 3, 30.0, 0, 1)):
        x, _ = clusters(N, L, n_clusters=min(4, N // 2), seed=N + L)
        out.append(("n%d_l%d" % (N, L), x, perp, pad, off))
    return out


def no_root_cases():
    """all rows equal; 12 exact duplicates of row 0 at perplexity 5 (more duplicates than the perplexity)"""
    eq = np.full((17, 5), 0.75, np.float32)
    x, _ = clusters(40, 4, seed=3)
    x[:13] = x[0]
    return [("all_equal", eq, 4.0), ("duplicates", x, 5.0)]


def step_states(N, kind, seed=0):
    """Y, inc, gain of the one-step cases: `tiny` (the 1e-4 scale of the initial map), `spread` (a developed map), `coincident`
    (pairs of rows share a position)"""
    rng = np.random.Generator(np.random.PCG64(1000 + seed))
    f = np.float32
    if kind == "tiny":
        Y = (1e-4 * rng.standard_normal((N, 2))).astype(f)
    else:
        Y = (8.0 * rng.standard_normal((N, 2))).astype(f)
    if kind == "coincident":
        Y[1::2] = Y[0::2][:Y[1::2].shape[0]]
    inc = (0.05 * np.abs(Y).mean() * rng.standard_normal((N, 2))).astype(f)
    gain = rng.choice(np.array([0.01, 0.0125, 0.5, 1.0, 1.2, 3.0], f), size=(N, 2)).astype(f)
    return dict(Y=Y, inc=inc, gain=gain)


STEP_CASES = [(kind, t) for kind in ("tiny", "spread", "coincident") for t in (249, 250)]
STEP_N, STEP_L, STEP_PERP = 300, 8, 20.0
RUN_N, RUN_L, RUN_PERP, RUN_SEED = 192, 8, 15.0, 5
MAP_N, MAP_L, MAP_PERP, MAP_T, MAP_SEED = 256, 16, 15.0, 300, 1
