"""float64 NumPy twin of sv_linprobe_* (include/splitvae.h): the Gram matrix, the logits from the fp32 rounding of W, softmax /
residual / loss, the chunk sums and the fp64 folds in the header's order, the gradient, the step, the fit loop and predict.
`emulate=True` emulates the fp32 roundings of the kernels (one rounding per multiply-add of a chain, per exp / log / division and per
addition) in the kernels' order.  Every function takes `bug=` -- the name of one deliberately wrong kernel (BUGS) -- so the tests
can show that their comparisons reject each of them.  fit_bounds() derives the error bounds the device tests use; the cases and the
comparison functions of tests/test_gpu_linprobe.py live here so that tests/test_linprobe_host.py can run them without a GPU."""
import numpy as np

CHUNK = 256                                       # sv_linprobe_chunk_rows()
TILE = 64
U = 2.0 ** -24                                    # unit roundoff of fp32
BUGS = ("drop_chunk_last", "transposed_fragment", "bias_regularised", "no_max_shift", "tie_high", "divisor_valid", "fold_reversed",
        "stale_w32", "sign", "drop_last_col")
f32, f64 = np.float32, np.float64


# ---------------------------------------------------------------- the fixed orders
def design(x):
    x = np.asarray(x, f64)
    return np.concatenate([x, np.ones((x.shape[0], 1))], axis=1)


def strided_sum(v):
    """thread u of 256 takes the elements u, u + 256, ... in ascending order, then the threads in ascending order (fp64)"""
    v = np.asarray(v, f64).reshape(-1)
    pad = np.zeros((-v.size) % 256)
    m = np.concatenate([v, pad]).reshape(-1, 256)
    part = np.zeros(256)
    with np.errstate(invalid="ignore"):            # a wrong kernel may hand over inf - inf
        for row in m:
            part = part + row
        tot = 0.0
        for p in part:
            tot = tot + p
    return float(tot)


def tile_sums(v):
    """fp64 sums of the 64-row tiles, rows in ascending order"""
    v = np.asarray(v, f64).reshape(-1)
    m = np.concatenate([v, np.zeros((-v.size) % TILE)]).reshape(-1, TILE)
    s = np.zeros(m.shape[0])
    with np.errstate(invalid="ignore"):
        for k in range(TILE):
            s = s + m[:, k]
    return s


def chunk_sums(a, m, emulate=False, bug=None):
    """[nchunks, Fa, Fm]: A^T M per chunk, the chunk's rows in ascending order; emulate: an fp32 accumulator, one rounding per row"""
    a, m = np.asarray(a, f64), np.asarray(m, f64)
    N = a.shape[0]
    nch = (N + CHUNK - 1) // CHUNK
    pad = nch * CHUNK - N
    ap = np.concatenate([a, np.zeros((pad, a.shape[1]))]).reshape(nch, CHUNK, -1)
    mp = np.concatenate([m, np.zeros((pad, m.shape[1]))]).reshape(nch, CHUNK, -1)
    rows = CHUNK - 1 if bug == "drop_chunk_last" else CHUNK
    if not emulate:
        return np.einsum("nkf,nkc->nfc", ap[:, :rows], mp[:, :rows])
    acc = np.zeros((nch, a.shape[1], m.shape[1]), f32)
    for k in range(rows):
        acc = (acc.astype(f64) + ap[:, k, :, None] * mp[:, k, None, :]).astype(f32)
    return acc.astype(f64)


def fold(parts, bug=None):
    """the chunks in ascending order, fp64"""
    order = range(parts.shape[0] - 1, -1, -1) if bug == "fold_reversed" else range(parts.shape[0])
    s = np.zeros(parts.shape[1:])
    for ch in order:
        s = s + parts[ch]
    return s


def gram(x, emulate=False, bug=None):
    """S = A^T A [(L+1),(L+1)], not divided by N: the upper triangle, mirrored"""
    a = design(np.asarray(x, f32))
    s = fold(chunk_sums(a, a, emulate, bug), bug)
    if bug == "transposed_fragment" and s.shape[0] > 16:       # the fragment (0, 1) written transposed
        k = min(16, s.shape[0] - 16)
        blk = s[:k, 16:16 + k].copy()
        s[:k, 16:16 + k] = blk.T
    return np.triu(s) + np.triu(s, 1).T


# ---------------------------------------------------------------- one pass
def logits(x, W, emulate=False, bug=None):
    """z = x . W32[:L] + W32[L], W32 the fp32 rounding of W; emulate: an fp32 accumulator over L in ascending order"""
    x = np.asarray(x, f32)
    w32 = np.asarray(W, f64).astype(f32)
    L = x.shape[1]
    Lu = L - 1 if (bug == "drop_last_col" and L % 4) else L
    if not emulate:
        return x[:, :Lu].astype(f64) @ w32[:Lu].astype(f64) + w32[L].astype(f64)
    z = np.zeros((x.shape[0], w32.shape[1]), f32)
    for l in range(Lu):
        z = (z.astype(f64) + x[:, l, None].astype(f64) * w32[l][None, :].astype(f64)).astype(f32)
    return (z + w32[L][None, :]).astype(f64)


def softmax_parts(z, y, C, emulate=False, bug=None):
    """(r [N,C], loss_i [N], p [N,C]) by the header's formulas; rows with y >= C: r = 0, loss = 0"""
    t = f32 if emulate or bug == "no_max_shift" else f64        # the overflow of the unshifted form is an fp32 matter
    z = np.asarray(z).astype(t)
    y = np.asarray(y).astype(np.int64)
    valid = y < C
    m = z.max(axis=1) if bug != "no_max_shift" else np.zeros(z.shape[0], t)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        e = np.exp((z - m[:, None]).astype(t).astype(f64)).astype(t)       # the correctly rounded function: the device's is within 1 ulp
        s = np.zeros(z.shape[0], t)
        for c in range(C):
            s = (s + e[:, c]).astype(t)
        p = (e / s[:, None]).astype(t)
        onehot = (np.arange(C)[None, :] == y[:, None]).astype(t)
        r = (onehot - p if bug == "sign" else p - onehot).astype(t)
        zy = z[np.arange(z.shape[0]), np.where(valid, y, 0)]
        loss = (np.log(s.astype(f64)).astype(t) - (zy - m).astype(t)).astype(t)
    r = np.where(valid[:, None], r, 0).astype(f64)
    loss = np.where(valid, loss, 0).astype(f64)
    return r, loss, p.astype(f64)


def evaluate(x, y, C, W, l2, emulate=False, bug=None, w_logits=None):
    """One pass against W -> dict(G, loss, gmax, r, p, z, loss_i).  w_logits: the W the logits are made from (the stale_w32 bug)."""
    x = np.asarray(x, f32)
    W = np.asarray(W, f64)
    N, L = x.shape
    z = logits(x, W if w_logits is None else w_logits, emulate, bug)
    r, loss_i, p = softmax_parts(z, y, C, emulate, bug)
    div = float(max(1, int((np.asarray(y) < C).sum()))) if bug == "divisor_valid" else float(N)
    s = fold(chunk_sums(design(x), r, emulate, bug), bug)
    if bug == "transposed_fragment":
        k = min(16, s.shape[0], C)
        s[:k, :k] = s[:k, :k].T.copy()
    G = s / div
    G[:L] = G[:L] + l2 * W[:L]
    reg = strided_sum((W[:L] * W[:L]).reshape(-1))
    if bug == "bias_regularised":
        G[L] = G[L] + l2 * W[L]
        reg = strided_sum((W * W).reshape(-1))
    loss = strided_sum(tile_sums(loss_i)) / div + (0.5 * l2) * reg
    return dict(G=G, loss=float(loss), gmax=float(np.abs(G).max()), r=r, p=p, z=z, loss_i=loss_i)


def step(W, P, G):
    """W - P G: per element the sum over j from 0 in ascending order (a product, then an addition), then one subtraction"""
    s = np.zeros_like(G)
    for j in range(P.shape[0]):
        s = s + P[:, j, None] * G[None, j, :]
    return W - s


def make_P(S, N, l2):
    """B = S / (2 N) + diag(l2 .. l2, 0); -> (P = B^-1, B); raises when B is not positive definite"""
    B = np.asarray(S, f64) / (2.0 * N)
    d = np.full(B.shape[0], float(l2))
    d[-1] = 0.0
    B = B + np.diag(d)
    np.linalg.cholesky(B)
    return np.linalg.inv(B), B


def fit(x, y, C, P, l2, T, W0=None, emulate=False, bug=None, keep=False):
    """-> dict(W, loss [T+1], gmax [T+1], G (of the last pass); keep: passes, the per-pass dicts with their W)"""
    x = np.asarray(x, f32)
    L = x.shape[1]
    W = np.zeros((L + 1, C)) if W0 is None else np.array(W0, f64)
    W_first = W.copy()
    loss, gmax, passes = [], [], []
    for t in range(T + 1):
        ev = evaluate(x, y, C, W, l2, emulate, bug, w_logits=W_first if bug == "stale_w32" else None)
        loss.append(ev["loss"])
        gmax.append(ev["gmax"])
        if keep:
            passes.append(dict(ev, W=W.copy()))
        if t == T:
            break
        W = step(W, P, ev["G"])
    return dict(W=W, loss=np.array(loss), gmax=np.array(gmax), G=ev["G"], passes=passes)


def predict(q, W, C, q_class=None, emulate=False, bug=None):
    """-> dict(pred int32 [Nq], hits, loss (mean cross-entropy; None without classes), z)"""
    z = logits(q, W, emulate, bug)
    zc = z.astype(f32) if emulate else z
    pred = (C - 1 - zc[:, ::-1].argmax(axis=1)) if bug == "tie_high" else zc.argmax(axis=1)
    out = dict(pred=pred.astype(np.int32), z=z, hits=None, loss=None)
    if q_class is not None:
        qc = np.asarray(q_class).astype(np.int64)
        out["hits"] = int(((pred == qc) & (qc < C)).sum())
        _, loss_i, _ = softmax_parts(z, qc, C, emulate, bug)
        div = float(max(1, int((qc < C).sum()))) if bug == "divisor_valid" else float(z.shape[0])
        out["loss"] = strided_sum(tile_sums(loss_i)) / div
    return out


# ---------------------------------------------------------------- derived bounds
def logit_bound(x, W):
    """Per row: |device z - twin z| <= (L + 4) u (|x| . |W32[:L]| + |W32[L]|), the maximum over the classes: L + 1 roundings of the fp32
    chain and of the bias addition, and 2 u |W| for two trajectories that round slightly different W (0 when they share W)."""
    x = np.abs(np.asarray(x, f64))
    w = np.abs(np.asarray(W, f64))
    L = x.shape[1]
    return (L + 4) * U * (x @ w[:L] + w[L][None, :]).max(axis=1)


def pass_bounds(x, y, C, ev, W, P, B, l2):
    """The rounding of one device pass against the twin's pass `ev` at the same W:
      dr   |r~ - r| <= p (exp(2 ez) - 1)                    the logits move by at most ez, softmax by that factor
                       + p u (2 D + C + 8) + u |r|           z - m, expf (1 ulp = 2 u), the sum of C terms, the division (2 u), twice
                                                             (numerator and denominator), D = max_c (m - z_c); the subtraction
      dG   |G~ - G| <= (sum_i |a_if| dr_ic + (CHUNK + 1) u sum_i |a_if| |r_ic|) / N        the fp32 chain over a chunk's rows
      beta = sqrt(sum_c dG_c^T |P| dG_c) >= || P dG ||_B                                   what one step adds in the B-norm
      dloss (arithmetic) <= mean_i (2 ez_i + u (2 C + 4 + 2 log C + 2 D_i + |loss_i|))"""
    x = np.asarray(x, f32)
    N = x.shape[0]
    a = np.abs(design(x))
    ez = logit_bound(x, W)
    z = ev["z"]
    D = z.max(axis=1) - z.min(axis=1)
    valid = (np.asarray(y) < C)[:, None]
    dr = np.where(valid, ev["p"] * np.expm1(2 * ez)[:, None] + ev["p"] * U * (2 * D[:, None] + C + 8) + U * np.abs(ev["r"]), 0.0)
    dG = (a.T @ dr + (CHUNK + 1) * U * (a.T @ np.abs(ev["r"]))) / N
    beta = float(np.sqrt(np.einsum("fc,fg,gc->", dG, np.abs(P), dG)))
    dloss = float((2 * ez + U * (2 * C + 4 + 2 * np.log(C) + 2 * D + np.abs(ev["loss_i"]))).mean())
    return dict(dG=dG, beta=beta, dloss=dloss)


def fit_bounds(x, y, C, P, B, l2, twin):
    """Bounds on the device's W_T, loss_t, gmax_t against a twin fit made with keep=True.  The exact step map W -> W - P grad f(W) is
    non-expansive in the B-norm (0 <= Hessian <= B in every class block), so with EB_t = sum_{s<t} beta_s (linear in t):
      |W~ - W|[i, c] <= sqrt(P_ii) EB_T;  |G~ - G|[f, c] <= dG + sqrt(B_ff) EB_t;
      |loss~ - loss| <= dloss + 2 max_i ||a_i||_P EB_t + sqrt(l2) ||W[:L]||_F EB_t
    and a floor of 1e-13 (1 + |value|) for the fp64 arithmetic both sides share."""
    x = np.asarray(x, f32)
    a = design(x)
    anorm = float(np.sqrt(np.einsum("if,fg,ig->i", a, P, a).max()))
    EB, out_loss, out_gmax = 0.0, [], []
    for ps in twin["passes"]:
        pb = pass_bounds(x, y, C, ps, ps["W"], P, B, l2)
        wn = float(np.sqrt((ps["W"][:-1] ** 2).sum()))
        out_loss.append(pb["dloss"] + (2 * anorm + np.sqrt(l2) * wn) * EB + 1e-13 * (1 + abs(ps["loss"])))
        dG = pb["dG"] + np.sqrt(np.diag(B))[:, None] * EB + 1e-13 * (1 + np.abs(ps["G"]))
        out_gmax.append(float(dG.max()))
        EB_here = EB
        EB += pb["beta"]
    W = twin["W"]
    return dict(W=np.sqrt(np.diag(P))[:, None] * EB_here + 1e-13 * (1 + np.abs(W)), loss=np.array(out_loss), gmax=np.array(out_gmax), G=dG, EB=EB_here)


# ---------------------------------------------------------------- the shared cases
def lattice(N, L, seed, amp=8):
    return np.random.default_rng(seed).integers(-amp, amp + 1, (N, L)).astype(f32)


def labels(N, C, seed, invalid=0):
    rng = np.random.default_rng(seed + 1000)
    y = rng.integers(0, C, N).astype(np.uint8)
    if invalid:
        y[rng.choice(N, min(invalid, N), replace=False)] = 200
    return y


def fold_trap(C=2):
    """three chunks whose fp64 fold depends on the order: 2^53, then two rows that carry 1 (x . 1 in S, x . r in G)"""
    x = np.zeros((2 * CHUNK + 1, 1), f32)
    x[0, 0], x[CHUNK, 0], x[2 * CHUNK, 0] = 2.0 ** 53, 1.0, 1.0
    return x, np.ones(x.shape[0], np.uint8)


def gauss(N, L, C, seed=7, spread=1.5):
    """Gaussian clusters: class centres spread / sqrt(L) apart per dimension, unit noise"""
    rng = np.random.default_rng(seed)
    centres = spread * rng.standard_normal((C, L)) / np.sqrt(L) * 3
    y = rng.integers(0, C, N).astype(np.uint8)
    x = (centres[y] + rng.standard_normal((N, L))).astype(f32)
    return x, y


GRAM_CASES = [("g-700-33", 700, 33, 1), ("g-1100-130", 1100, 130, 2), ("g-65-5", 65, 5, 3), ("g-513-16", CHUNK + 1, 16, 4)]
FIRST_CASES = [("f-1100-33-2", 1100, 33, 2, 5, False), ("f-700-130-4", 700, 130, 4, 7, False), ("f-1030-17-8", 2 * CHUNK + 6, 17, 8, 9, False),
               ("f-600-35-8-w", 600, 35, 8, 3, True)]
GAUSS_CASES = [("n-3000-32-10", 3000, 32, 10, 1e-3), ("n-700-130-3", 700, 130, 3, 1e-2)]
GAUSS_T = (1, 3, 50)


def cases():
    """The inputs the device tests and the wrong kernels share: dicts with kind in (gram, first, fit, predict)"""
    out = []
    for name, N, L, seed in GRAM_CASES:
        out.append(dict(name=name, kind="gram", x=lattice(N, L, seed)))
    out.append(dict(name="g-fold-trap", kind="gram", x=fold_trap()[0]))
    for name, N, L, C, invalid, w0 in FIRST_CASES:
        c = dict(name=name, kind="first", x=lattice(N, L, N + L), y=labels(N, C, N, invalid), C=C, l2=1e-3)
        if w0:                                     # equal columns: every logit of a row is the same integer, p = 1 / C still, and l2 W shows
            v = np.random.default_rng(L).integers(-2, 3, L + 1).astype(f64)
            v[L] = 3.0
            c["W0"] = np.repeat(v[:, None], C, axis=1)
        out.append(c)
    xt, yt = fold_trap()
    out.append(dict(name="f-fold-trap", kind="first", x=xt, y=yt, C=2, l2=0.0))
    for name, N, L, C, l2 in GAUSS_CASES:
        x, y = gauss(N, L, C)
        y = y.copy()
        y[5] = 77                                  # one row that takes no part
        for T in GAUSS_T:
            out.append(dict(name="%s-T%d" % (name, T), kind="fit", x=x, y=y, C=C, l2=l2, T=T))
        out.append(dict(name=name + "-predict", kind="predict", x=x, y=y, C=C, l2=l2, T=30))
        if L == 130:                               # logits of +-100 and more: expf overflows without the max shift
            out.append(dict(name=name + "-big", kind="predict", x=x, y=y, C=C, l2=l2, T=30, scale=60.0))
    out.append(dict(name="p-ties", kind="predict", x=lattice(130, 9, 3), y=labels(130, 5, 3), C=5, l2=1e-3, T=None))
    return out


_P_CACHE = {}


def case_P(case):
    """(P, B) of a fit / predict case from the twin's own Gram matrix"""
    key = case["name"].rsplit("-", 1)[0]
    if key not in _P_CACHE:
        _P_CACHE[key] = make_P(gram(case["x"]), case["x"].shape[0], case["l2"])
    return _P_CACHE[key]


def run_case(case, bug=None, emulate=False):
    """The twin's (or a wrong kernel's) outputs of a case, in the layout the device helpers of tests/test_gpu_linprobe.py return"""
    k = case["kind"]
    if k == "gram":
        return dict(S=gram(case["x"], emulate, bug))
    if k == "first":
        L = case["x"].shape[1]                    # every operation of these cases is exact but logf(C): the fp32 path is the reference
        ev = evaluate(case["x"], case["y"], case["C"], case.get("W0", np.zeros((L + 1, case["C"]))), case["l2"], True, bug)
        return dict(G=ev["G"], loss=np.array([ev["loss"]]), gmax=np.array([ev["gmax"]]))
    if k == "fit":
        P, _ = case_P(case)
        return fit(case["x"], case["y"], case["C"], P, case["l2"], case["T"], emulate=emulate, bug=bug, keep=bug is None and not emulate)
    W = predict_weights(case)
    pr = predict(case["x"], W, case["C"], case["y"], emulate, bug)
    return dict(pred=pr["pred"], hits=pr["hits"], loss=pr["loss"], z=pr["z"])


_W_CACHE = {}


def predict_weights(case):
    """the W a predict case classifies with: zeros (every logit ties), or the twin's fit after T steps"""
    if case["T"] is None:
        return np.zeros((case["x"].shape[1] + 1, case["C"]))
    if case["name"] not in _W_CACHE:
        P, _ = case_P(case)
        _W_CACHE[case["name"]] = case.get("scale", 1.0) * fit(case["x"], case["y"], case["C"], P, case["l2"], case["T"])["W"]
    return _W_CACHE[case["name"]]


MARGIN_CAP = 0.01                                 # at most 1 % of the rows of a predict case may sit below the margin


def predict_excluded(case, want):
    """rows whose top-2 logit margin in the twin is below twice the logit bound (either logit may be off by one bound); where the
    bound is 0 the logits are exact and a tie is the rule's to break"""
    W = predict_weights(case)
    z = np.sort(want["z"], axis=1)
    return (z[:, -1] - z[:, -2]) < 2 * logit_bound(case["x"], W)


def predict_loss_bound(case, want):
    W = predict_weights(case)
    x = case["x"]
    r, loss_i, p = softmax_parts(want["z"], case["y"], case["C"])
    D = want["z"].max(axis=1) - want["z"].min(axis=1)
    C = case["C"]
    return float((2 * logit_bound(x, W) + U * (2 * C + 4 + 2 * np.log(C) + 2 * D + np.abs(loss_i))).mean()) + 1e-13


def compare(case, got, want, bounds=None):
    """-> the list of what is wrong with `got` (empty: accepted).  gram / first: bit for bit.  fit: W, loss, gmax within `bounds`
    (fit_bounds) and the loss monotone up to its bound.  predict: pred equal outside the excluded rows, hits consistent, loss bounded."""
    bad = []
    k = case["kind"]

    def same(name):
        a, b = np.asarray(got[name], f64), np.asarray(want[name], f64)
        if a.shape != b.shape or not np.array_equal(a.view(np.int64), b.view(np.int64)):
            bad.append("%s differs in bits" % name)
    if k == "gram":
        same("S")
        if not np.array_equal(np.asarray(got["S"]), np.asarray(got["S"]).T):
            bad.append("S is not symmetric")
    elif k == "first":
        for n in ("G", "loss", "gmax"):
            same(n)
    elif k == "fit":
        for n in ("W", "loss", "gmax", "G"):
            a, b = np.asarray(got[n], f64), np.asarray(want[n], f64)
            if a.shape != b.shape or not np.isfinite(a).all():
                bad.append("%s: shape or non-finite" % n)
                continue
            ratio = float((np.abs(a - b) / bounds[n]).max())
            if ratio > 1.0:
                bad.append("%s off by %.3g of its bound" % (n, ratio))
        lo = np.asarray(got["loss"], f64)
        if lo.shape == bounds["loss"].shape and (lo[1:] > lo[:-1] + bounds["loss"][1:] + bounds["loss"][:-1]).any():
            bad.append("the loss rises")
    else:
        ex = predict_excluded(case, want)
        if ex.mean() > MARGIN_CAP:
            bad.append("%.3f of the rows excluded" % ex.mean())
        if not np.array_equal(np.asarray(got["pred"])[~ex], want["pred"][~ex]):
            bad.append("pred differs")
        qc = np.asarray(case["y"]).astype(np.int64)
        if got["hits"] != int(((np.asarray(got["pred"]) == qc) & (qc < case["C"])).sum()):
            bad.append("hits are not those of pred")
        if not (abs(got["loss"] - want["loss"]) <= predict_loss_bound(case, want)):
            bad.append("loss off")
    return bad
