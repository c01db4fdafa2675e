"""Float64 twins of the swap-consistency report (include/splitvae.h: sv_swap_pair / sv_swap_requantise / sv_swap_rank;
split_vae_amd/swap.py), the cases the GPU tests run and the comparisons they make.  tests/test_swap_host.py applies mutants to the
twins and checks that the same comparisons on the same cases reject each of them; tests/test_gpu_swap.py holds the device to the twins.

`mutant` names a deliberate mistake:
  rank        'le' (<= in place of <), 'tie_rev' (the tie rule reversed), 'count_target' (the target column counted), 'swap_targets',
              'no_norm_r' (the norm of r dropped from the distance)
  partner     'minus' (j = i - s)
  requantise  'trunc' (levels by truncation), 'no_clamp' (no clamp of the mean or of the level: the level wraps like a byte),
              'unscrambled' (channels 3..5 a copy of 0..2)
  pair        'l_from_ig' (the z_l columns taken from ig)
"""
from fractions import Fraction

import numpy as np

RANK_MUTANTS = ("le", "tie_rev", "count_target", "swap_targets", "no_norm_r")
REQUANT_MUTANTS = ("trunc", "no_clamp", "unscrambled")


# ---------------------------------------------------------------- ranks
def distances(Q, R, mutant=None):
    """d [Nq, Nr] = max(0, (n(q) + n(r)) - 2 q . r) in float64"""
    Q, R = np.asarray(Q, np.float64), np.asarray(R, np.float64)
    nq, nr = (Q * Q).sum(axis=1), (R * R).sum(axis=1)
    if mutant == "no_norm_r":
        nr = np.zeros_like(nr)
    return np.maximum(0.0, (nq[:, None] + nr[None, :]) - 2.0 * (Q @ R.T))


def rank(Q, R, t0, t1, mutant=None):
    """rank [Nq, 2] by the definition, brute force: #{r != t : d(q,r) < d(q,t) or (d(q,r) == d(q,t) and r < t)}"""
    d = distances(Q, R, mutant)
    if mutant == "swap_targets":
        t0, t1 = t1, t0
    Nq, Nr = d.shape
    out = np.zeros((Nq, 2), np.int64)
    col = np.arange(Nr)
    for s, t in enumerate((np.asarray(t0), np.asarray(t1))):
        for q in range(Nq):
            dt = d[q, t[q]]
            if mutant == "le":
                hit = d[q] <= dt
            elif mutant == "tie_rev":
                hit = (d[q] < dt) | ((d[q] == dt) & (col > t[q]))
            else:
                hit = (d[q] < dt) | ((d[q] == dt) & (col < t[q]))
            if mutant == "count_target":
                hit[t[q]] = True
            else:
                hit[t[q]] = False
            out[q, s] = int(hit.sum())
    return out


def rank_by_argsort(Q, R, t0, t1):
    """The same ranks restated: the position of the target in the stable (distance, index) order of the row"""
    d = distances(Q, R)
    out = np.zeros((d.shape[0], 2), np.int64)
    for s, t in enumerate((np.asarray(t0), np.asarray(t1))):
        for q in range(d.shape[0]):
            order = np.argsort(d[q], kind="stable")                  # equal distances keep ascending index
            out[q, s] = int(np.nonzero(order == t[q])[0][0])
    return out


def rank_bracket(Q, R, t0, t1):
    """(lo, hi) [Nq, 2]: the ranks every fp32 evaluation of the tile may give: lo counts the references certainly before the target, hi
    those possibly before it, with tol(q, r) = eps(q, r) + eps(q, t) and eps a bound on the error of one device distance.

    The contract's first bound is eps = (L + 4) 2^-23 (n(q) + n(r) + 2 |q| |r|): one rounding of 2^-23 per operation, every term at its
    Cauchy-Schwarz magnitude.  This is the tighter one it invites, from the operations as they run (u = 2^-24, the unit roundoff of
    round-to-nearest; gamma_m = m u / (1 - m u) <= 1.01 m u for m <= 600):
      norms    lane l squares and adds j = l, l + 64, ...: a term passes its product's rounding, at most ceil(L / 64) - 1 lane additions and
               the 6 of the butterfly: n^ = n (1 + theta), |theta| <= gamma_K, K = ceil(L / 64) + 6
      dot      a chain of L fused multiply-adds (the zero padding adds nothing); the four products of one MFMA are allowed a rounding of
               their own: |dot^ - dot| <= gamma_(L+4) S, S = sum_j |q_j r_j| <= |q| |r|
      epilogue s = fl(n^(q) + n^(r)), d^ = fl(s - 2 dot^) (the doubling is exact), max(0, .) moves d^ towards d >= 0: two more roundings,
               on at most n(q) + n(r) and n(q) + n(r) + 2 S
    so |d^ - d| <= 1.01 u ((K + 2) (n(q) + n(r)) + 2 (L + 5) S): never above the first bound, about a quarter of it on near pairs."""
    Q, R = np.asarray(Q, np.float64), np.asarray(R, np.float64)
    L = Q.shape[1]
    d = distances(Q, R)
    nq, nr = (Q * Q).sum(axis=1), (R * R).sum(axis=1)
    K = -(-L // 64) + 6
    eps = 1.01 * 2.0 ** -24 * ((K + 2) * (nq[:, None] + nr[None, :]) + 2.0 * (L + 5) * (np.abs(Q) @ np.abs(R).T))
    assert (eps <= (L + 4) * 2.0 ** -23 * (nq[:, None] + nr[None, :] + 2.0 * np.sqrt(nq)[:, None] * np.sqrt(nr)[None, :])).all()
    lo, hi = np.zeros((d.shape[0], 2), np.int64), np.zeros((d.shape[0], 2), np.int64)
    for s, t in enumerate((np.asarray(t0), np.asarray(t1))):
        for q in range(d.shape[0]):
            tol = eps[q] + eps[q, t[q]]
            a, b = d[q] < d[q, t[q]] - tol, d[q] <= d[q, t[q]] + tol
            a[t[q]] = b[t[q]] = False
            lo[q, s], hi[q, s] = int(a.sum()), int(b.sum())
    return lo, hi


def ranks_equal(got, want):
    """the lattice comparison: bit for bit"""
    got, want = np.asarray(got, np.int64), np.asarray(want, np.int64)
    return got.shape == want.shape and bool((got == want).all())


def ranks_in_bracket(got, lo, hi, want):
    """the Gaussian comparison: inside [lo, hi] everywhere, and the twin's rank wherever the bracket decides"""
    got = np.asarray(got, np.int64)
    decided = lo == hi
    return bool(((got >= lo) & (got <= hi)).all()) and bool((got[decided] == np.asarray(want)[decided]).all())


def undecided_share(lo, hi):
    return float(np.mean((hi > lo).any(axis=1)))


def lattice_rows(rng, n, L):
    """n rows of integers in [-4, 4] built from a 3-dimensional seed: row[j] = seed[j mod 3] * w[j], w fixed signs with a few zeros"""
    seed = rng.integers(-4, 5, size=(n, 3))
    w = np.array([1, -1, 1, 1, 0, -1, 1], np.int64)
    j = np.arange(L)
    return (seed[:, j % 3] * w[j % 7][None, :]).astype(np.float32)


def lattice_case(Nq, Nr, L, seed):
    """dict(Q, R, t0, t1): a target at row 0 and at row Nr - 1, t0 == t1 on some rows, references that duplicate a target at a lower and
    at a higher index, a query equal to its target"""
    rng = np.random.default_rng(seed)
    R = lattice_rows(rng, Nr, L)
    Q = lattice_rows(rng, Nq, L)
    t0 = rng.integers(0, Nr, size=Nq).astype(np.int32)
    t1 = rng.integers(0, Nr, size=Nq).astype(np.int32)
    t0[0], t1[0] = 0, Nr - 1
    if Nq > 2:
        t1[1] = t0[1]                                  # t0 == t1
        t0[2], t1[2] = Nr - 1, 0
        Q[2] = R[t0[2]]                                # a query equal to its target
    if Nr >= 3:
        mid = Nr // 2
        R[0] = R[mid]
        R[Nr - 1] = R[mid]                             # the target's duplicates at a lower and at a higher index
        t0[Nq - 1] = mid
        if Nq > 2:
            Q[2] = R[t0[2]]
    return dict(Q=Q, R=R, t0=t0, t1=t1)


def lattice_shapes(chunk):
    """(Nq, Nr, L, pad_q, pad_r, off): every Nq, Nr, L the report's contract names, padded pitches and an offset base pointer"""
    return [(1, 1, 1, 0, 0, 0), (63, 2, 3, 5, 0, 0), (64, 64, 31, 0, 3, 1), (65, 65, 32, 0, 0, 0), (130, chunk - 1, 33, 7, 1, 3),
            (64, chunk, 128, 0, 0, 0), (65, chunk + 1, 256, 4, 4, 0), (130, 2 * chunk + 3, 33, 0, 0, 0), (1, 65, 128, 0, 0, 2)]


GAUSS_SHAPES = [(130, 1000, 33), (257, 2100, 128), (200, 1500, 256), (65, 300, 7)]
GAUSS_SEED = 7
UNDECIDED_CAP = 0.02


def gaussian_case(Nq, Nr, L, seed=GAUSS_SEED):
    """references G [Nr,4] @ A [4,L] / 2 + 0.05 noise; queries r[t0] + 0.3 (g [Nq,4] @ A / 2); fp32 values.  t1 is one of the query's 32
    nearest references (a far target sits in the dense part of the distance distribution, where no fp32 evaluation decides its rank)."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((4, L))
    R = (rng.standard_normal((Nr, 4)) @ A / 2 + 0.05 * rng.standard_normal((Nr, L))).astype(np.float32)
    t0 = rng.integers(0, Nr, size=Nq).astype(np.int32)
    Q = (R[t0].astype(np.float64) + 0.3 * (rng.standard_normal((Nq, 4)) @ A / 2)).astype(np.float32)
    near = np.argsort(distances(Q, R), axis=1, kind="stable")[:, :32]
    t1 = near[np.arange(Nq), rng.integers(0, min(32, Nr), size=Nq)].astype(np.int32)
    return dict(Q=Q, R=R, t0=t0, t1=t1)


# ---------------------------------------------------------------- requantise
def make_lut():
    """data.ResidentDataset.make_lut restated: x / 255 * 2 - 1 in float64, rounded to fp32 once"""
    return (np.arange(256, dtype=np.float64) / 255.0 * 2 - 1).astype(np.float32)


def _round_f32(x):
    """a non-negative Fraction -> the nearest fp32 (ties to even), as a Fraction; normal range only"""
    if x == 0:
        return Fraction(0)
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1
    ulp = Fraction(2) ** (e - 23)
    return round(x / ulp) * ulp                        # Python rounds a Fraction half to even


def level(m, mutant=None):
    """The pixel level of one fp32 mean: v = min(max(m, -1), 1); rint(fma(v, 127.5, 127.5)) with the fma rounded once to fp32; clamp to 0 .. 255; NaN -> 0"""
    m = np.float32(m)
    if np.isnan(m):
        return 0
    if mutant == "no_clamp":
        if not np.isfinite(m):
            return 0
        v = Fraction(float(m))
    else:
        v = Fraction(float(min(max(m, np.float32(-1)), np.float32(1))))
    x = v * Fraction(255, 2) + Fraction(255, 2)
    y = -_round_f32(-x) if x < 0 else _round_f32(x)
    lv = int(y.numerator // y.denominator) if mutant == "trunc" else int(round(y))
    if mutant == "no_clamp":
        return lv & 255
    return min(max(lv, 0), 255)


def levels(means, mutant=None):
    """level() of every element of an fp32 array.  Where |v| >= 2^-20 the float64 expression v * 127.5 + 127.5 is exact (a 32-bit product
    whose lowest bit is at least 2^-44, under a sum below 2^8: 52 bits), so its rounding to fp32 is the fma's one rounding; the other
    elements take the rational path."""
    m = np.asarray(means, np.float32)
    flat = m.reshape(-1)
    out = np.zeros(flat.shape, np.int64)
    nan = np.isnan(flat)
    if mutant == "no_clamp":
        v = np.where(np.isfinite(flat), flat, np.float32(0))
    else:
        v = np.minimum(np.maximum(flat, np.float32(-1)), np.float32(1))
    fast = ~nan & (np.abs(v) >= np.float32(2.0 ** -20))
    with np.errstate(invalid="ignore", over="ignore"):
        y = (v[fast].astype(np.float64) * 127.5 + 127.5).astype(np.float32)
        lv = (np.trunc(y) if mutant == "trunc" else np.rint(y)).astype(np.float64)
        if mutant == "no_clamp":
            wrapped = np.mod(lv, 256.0)
            out[fast] = np.where(np.isfinite(wrapped), wrapped, 0.0).astype(np.int64)
        else:
            out[fast] = np.clip(lv, 0, 255).astype(np.int64)
    for n in np.nonzero(~nan & ~fast)[0]:
        out[n] = level(flat[n], mutant)
    return out.reshape(m.shape)


def scramble_source(H, patch, perm_b):
    """src [H*H]: the pixel index every destination pixel of the scrambled half copies (sv_scramble_gather's rule)"""
    G = H // patch
    y, x = np.divmod(np.arange(H * H), H)
    r, i, c, j = y // patch, y % patch, x // patch, x % patch
    p = np.asarray(perm_b)[r * G + c]
    return ((p // G) * patch + i) * H + (p % G) * patch + j


def requantise(out6, perm, patch, lut=None, mutant=None):
    """images6 [B,H,W,6]: channels 0..2 lut[level(mean)], channels 3..5 their patch scramble.  Channels 3..5 of out6 are not read."""
    lut = make_lut() if lut is None else lut
    out6 = np.asarray(out6, np.float32)
    B, H, W, _ = out6.shape
    x = lut[levels(np.ascontiguousarray(out6[..., :3]), mutant)]
    res = np.empty((B, H, W, 6), np.float32)
    res[..., :3] = x
    for b in range(B):
        src = np.arange(H * W) if mutant == "unscrambled" else scramble_source(H, patch, perm[b])
        res[b, ..., 3:] = x[b].reshape(H * W, 3)[src].reshape(H, W, 3)
    return res


def requantise_means(B, H, seed):
    """out6 [B,H,H,6] fp32 whose channels 0..2 walk through the edge values (means on levels, on half levels of both parities, one ulp
    either side of a half level, +-1, beyond +-1, +-0, NaN) and random values; channels 3..5 are NaN: they must not be read"""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    edge = []
    for l in (0, 1, 2, 3, 126, 127, 128, 200, 253, 254, 255):
        on = f32((l - 127.5) / 127.5)
        edge.append(on)
        if l < 255:
            half = f32((l + 0.5 - 127.5) / 127.5)      # level l + 1/2: l even and odd -> both parities
            edge += [half, np.nextafter(half, f32(2)), np.nextafter(half, f32(-2))]
    edge += [f32(1), f32(-1), f32(1.5), f32(-1.5), f32(3e38), f32(-3e38), f32(np.inf), f32(-np.inf), f32(0.0), f32(-0.0), f32(np.nan),
             np.nextafter(f32(1), f32(0)), np.nextafter(f32(-1), f32(0)), f32(1e-30), f32(-1e-30)]
    edge = np.array(edge, np.float32)
    n = B * H * H * 3
    vals = rng.uniform(-1.1, 1.1, size=n).astype(np.float32)
    # exact half levels in fp32 arithmetic: v = (k - 255) / 255 for odd k is not representable, so add the values whose fma lands on .5
    k = rng.integers(0, 255, size=n // 4)
    vals[:n // 4] = ((k + 0.5 - 127.5) / 127.5).astype(np.float32)
    vals[n // 4:n // 4 + edge.size] = edge[:max(0, min(edge.size, n - n // 4))]
    rng.shuffle(vals)
    out6 = np.full((B, H, H, 6), np.nan, np.float32)
    out6[..., :3] = vals.reshape(B, H, H, 3)
    return out6


def requantise_perms(B, H, patch, seed):
    """perm [B, G^2]: image 0 the identity, image 1 (if any) the reversal, the rest random"""
    rng = np.random.default_rng(seed)
    G2 = (H // patch) ** 2
    perm = np.stack([rng.permutation(G2) for _ in range(B)]).astype(np.int32)
    perm[0] = np.arange(G2)
    if B > 1:
        perm[1] = np.arange(G2)[::-1]
    return perm


REQUANT_SHAPES = [(B, H, p) for H in (8, 32) for p in (1, 4, H) for B in (1, 3)]


def bits_equal(a, b):
    """bit for bit, NaN payloads included"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool((a.view(np.uint32) == b.view(np.uint32)).all())


# ---------------------------------------------------------------- pair, partners, figures
def pair(mu, ig, il, Lg, mutant=None):
    mu = np.asarray(mu, np.float32)
    src_l = ig if mutant == "l_from_ig" else il
    return np.concatenate([mu[np.asarray(ig), :Lg], mu[np.asarray(src_l), Lg:]], axis=1)


def partner(n, s, mutant=None):
    i = np.arange(n)
    return (i - s) % n if mutant == "minus" else (i + s) % n


def figures(ranks, k):
    """ranks [P+1, N, 2] of one block (pass 0 unswapped; kept, leak) -> (kept@1, kept@k, MRR, leak@1, cycle@1) in float64"""
    r = np.asarray(ranks, np.int64)
    kept = [int(v) for v in r[1:, :, 0].reshape(-1)]
    leak = [int(v) for v in r[1:, :, 1].reshape(-1)]
    n = float(len(kept))
    return dict(kept1=sum(v == 0 for v in kept) / n, keptk=sum(v < k for v in kept) / n, mrr=float(np.sum([1.0 / (v + 1.0) for v in kept]) / n),
                leak1=sum(v == 0 for v in leak) / n, cycle1=sum(int(v) == 0 for v in r[0, :, 0]) / float(r.shape[1]))


def class_figures(pred, labels, shifts):
    pred, labels = np.asarray(pred), np.asarray(labels)
    n = len(labels)
    fg = fl = m = 0
    for p, s in enumerate(shifts):
        for i in range(n):
            j = (i + s) % n
            if labels[i] != labels[j]:
                m += 1
                fg += int(pred[p + 1][i] == labels[i])
                fl += int(pred[p + 1][i] == labels[j])
    return dict(follows_g=fg / m if m else None, follows_l=fl / m if m else None, unlike_pairs=m,
                unswapped_acc=sum(int(pred[0][i] == labels[i]) for i in range(n)) / float(n))


def philox4x32(key, ctr):
    k0, k1 = key
    c = list(ctr)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & 0xffffffff, (p0 >> 32) ^ c[3] ^ k1, p0 & 0xffffffff]
        k0, k1 = (k0 + 0x9E3779B9) & 0xffffffff, (k1 + 0xBB67AE85) & 0xffffffff
    return c


def shift_word(seed, p, attempt):
    """sv_swap_shift_word_host restated: key seed ^ 0x1a7e5a9c0de5, counter (attempt, p, 'sw' tag, 0), word 0"""
    s = (int(seed) ^ 0x1a7e5a9c0de5) & 0xffffffffffffffff
    return philox4x32((s & 0xffffffff, s >> 32), [attempt & 0xffffffff, p & 0xffffffff, 0x73770000, 0])[0]


def partner_shifts(seed, n, partners):
    out = []
    for p in range(1, partners + 1):
        attempt = 0
        while True:
            s = 1 + shift_word(seed, p, attempt) % (n - 1)
            attempt += 1
            if s not in out:
                break
        out.append(s)
    return out
