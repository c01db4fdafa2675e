"""float64 twin of the aggregate-posterior information report (include/splitvae.h: sv_latent_info_draw / _lse / _finish;
split_vae_amd/latent_info.py), a per-element error bound derived from the kernels' own arithmetic (csrc/latent_info.hip), the
kernel's fp32 arithmetic replayed operation by operation in NumPy, mutants of the twin, and the inputs the GPU tests use.

Definitions (block of width L, images j with posterior mean mu_j and standard deviation sig_j; fp32 inputs taken exactly):
    z_i = fl32(mu_i + fl32(sig_i * eps_i))                            the device's expression, reproduced bit for bit
    c_j = -sum_d log sig_jd - L/2 log 2 pi
    e_ij = c_j - 1/2 sum_d ((z_id - mu_jd) / sig_jd)^2                 e^gl = e^g + e^l
    own_i = c_i - 1/2 sum_d eps_id^2,  prior_i = -L/2 log 2 pi - 1/2 sum_d z_id^2
    lse[i] = logsumexp_j e_ij - log Nr
    KL = mean(own - prior), MI = mean(own - lse), marginal KL = mean(lse - prior), overlap = mean(lse_gl - lse_g - lse_l)

The bound, with u = 2^-24 (one fp32 rounding) and acc_ij = sum_d w_d^2, w_d = (z_d - mu_d) / sig_d:
    the device computes fl(fl(z - mu) * fl(1 / sig)) = w (1 + theta), |theta| <= 3 u, squares it inside a fused multiply-add
    (relative 6 u) and cumulates L non-negative terms, each passing through at most L roundings: |d acc| <= (L + 7) u acc;
    e = fl(c32 - acc / 2):  E_ij = (L + 7) u acc_ij / 2 + cerr_j + u |e_ij|, with cerr_j = 0 where cst is an input of the call
    and u |c_j| + 6 u sum_d |log sig_jd| where sv_latent_info_draw made it (logf within 3 ulp, summed in fp64, rounded once);
    e^gl = fl(e^g + e^l): E^gl = E^g + E^l + u |e^gl|;
    lse:  |d lse_i| <= log sum_j w_ij exp(E_ij)  (w = the softmax weights; exact, both signs, not first order)
          + the summation's own error: every partial passes through at most CHUNK / 64 pushes and 6 butterfly merges, each one
            v_exp_f32 (1 ulp = 2 u), an argument whose rounding (3 u |d|) matters only while s exp(-|d|) >= 1, i.e. |d| <= log CHUNK,
            and two roundings: (CHUNK / 64 + 6) (5 + 3 log CHUNK) u; the chunk merge is fp64;
          + the flushed tail: terms more than 87 nats below the row maximum may be dropped whole (v_exp_f32 flushes below 2^-126).
"""
import numpy as np

U = 2.0 ** -24
HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)
LOG2E32 = np.float32(1.44269504088896340736)
RT = 64                                  # references per pass of the tile kernel (one per lane)
F32, F64 = np.float32, np.float64


# ---------------------------------------------------------------- the twin
def draw(mu, sig, eps, Lg):
    """mu, sig, eps [N, Lg+Ll] fp32 -> dict(z, rsig (fp32, the device's bits), c [N,2], own [N,2], prior [N,2], cerr [N,2] fp64)."""
    mu, sig, eps = (np.asarray(a, F32) for a in (mu, sig, eps))
    z = (mu + (sig * eps).astype(F32)).astype(F32)
    rsig = (F32(1.0) / sig).astype(F32)
    N, Lc = mu.shape
    c, own, prior, cerr = (np.zeros((N, 2)) for _ in range(4))
    for e, (a, b) in enumerate(((0, Lg), (Lg, Lc))):
        L = b - a
        if L == 0:
            continue
        ls = np.log(sig[:, a:b].astype(F64))
        c[:, e] = -ls.sum(1) - L * HALF_LOG_2PI
        own[:, e] = c[:, e] - 0.5 * (eps[:, a:b].astype(F64) ** 2).sum(1)
        prior[:, e] = -L * HALF_LOG_2PI - 0.5 * (z[:, a:b].astype(F64) ** 2).sum(1)
        cerr[:, e] = U * np.abs(c[:, e]) + 6 * U * np.abs(ls).sum(1)
    return dict(z=z, rsig=rsig, c=c, own=own, prior=prior, cerr=cerr)


def quad(z, mu, sig, a, b, scale=None):
    """acc [Nq, Nr] fp64 = sum_{d in a..b-1} ((z_id - mu_jd) * scale_jd)^2, scale = 1 / sig"""
    z, mu = np.asarray(z, F64), np.asarray(mu, F64)
    scale = 1.0 / np.asarray(sig, F64) if scale is None else np.asarray(scale, F64)
    acc = np.zeros((z.shape[0], mu.shape[0]))
    for d in range(a, b):
        acc += ((z[:, d:d + 1] - mu[None, :, d]) * scale[None, :, d]) ** 2
    return acc


def _lse_rows(e):
    m = e.max(1)
    return m + np.log(np.exp(e - m[:, None]).sum(1))


def lse(z, mu, sig, cst, Lg, chunk=1024, mutant=None):
    """-> dict(lse [3,Nq] (rows 1, 2 NaN when Ll = 0), e, acc: lists per sum of [Nq,Nr]).  cst [Nr,2]: the row constants AS THE CALL
    RECEIVES THEM (fp32 values, taken exactly).  `mutant`: one of MUTANTS, a deliberately wrong twin."""
    z, mu, sig = (np.asarray(a, F32) for a in (z, mu, sig))
    cst = np.asarray(cst, F64)
    Nq, Lc = z.shape
    Nr = mu.shape[0]
    Ll = Lc - Lg
    ga, gb, la, lb = 0, Lg, Lg, Lc
    scale = None
    if mutant == "last_dim_g_dropped":
        gb -= 1
    if mutant == "last_dim_l_dropped":
        lb -= 1
    if mutant == "sig_for_rsig":
        scale = sig
    if mutant == "cst_without_log_sig":
        ls = np.log(sig.astype(F64))
        cst = cst + np.stack([ls[:, :Lg].sum(1), ls[:, Lg:].sum(1)], 1)
    if mutant == "cst_without_2pi":
        cst = cst + np.array([Lg, Ll]) * HALF_LOG_2PI
    half = 1.0 if mutant == "half_dropped" else 0.5
    acc_g = quad(z, mu, sig, ga, gb, scale)
    e_g = cst[None, :, 0] - half * acc_g
    es, accs = [e_g], [acc_g]
    if Ll:
        acc_l = quad(z, mu, sig, la, lb, scale)
        e_l = cst[None, :, 1] - half * acc_l
        es += [e_l, (e_g + e_g) if mutant == "joint_g_twice" else (e_g + e_l)]
        accs += [acc_l, acc_g + acc_l]
    keep = slice(None)
    if mutant == "last_partial_chunk_skipped" and Nr % chunk and Nr > chunk:
        keep = slice(0, Nr // chunk * chunk)
    if mutant == "first_reference_skipped" and Nr > 1:
        keep = slice(1, None)
    logn = 0.0 if mutant == "log_n_forgotten" else np.log(Nq if mutant == "log_nq" else Nr)
    out = np.full((3, Nq), np.nan)
    for t, e in enumerate(es):
        e = e[:, keep]
        if mutant == "max_not_updated":              # the chunk sums added without rescaling to a common maximum
            m0, tot = None, 0.0
            for c0 in range(0, e.shape[1], chunk):
                m = e[:, c0:c0 + chunk].max(1)
                tot = tot + np.exp(e[:, c0:c0 + chunk] - m[:, None]).sum(1)
                m0 = m if m0 is None else m0
            out[t] = m0 + np.log(tot) - logn
        else:
            out[t] = _lse_rows(e) - logn
    if Ll and mutant == "blocks_swapped":
        out[[0, 1]] = out[[1, 0]]
    if Ll and mutant == "joint_is_product":
        out[2] = out[0] + out[1]
    return dict(lse=out, e=es, acc=accs)


MUTANTS = ["last_dim_g_dropped", "last_dim_l_dropped", "sig_for_rsig", "log_n_forgotten", "last_partial_chunk_skipped", "blocks_swapped",
           "joint_is_product", "max_not_updated", "cst_without_log_sig", "cst_without_2pi", "half_dropped", "joint_g_twice",
           "first_reference_skipped", "log_nq"]


def report(own, prior, lse3, Ll):
    """-> [8] fp64: KL_g, MI_g, marginal KL_g, KL_l, MI_l, marginal KL_l, overlap, log N (entries 3 .. 6 are 0 when Ll = 0)"""
    N = own.shape[0]
    out = np.zeros(8)
    out[0], out[1], out[2] = (own[:, 0] - prior[:, 0]).mean(), (own[:, 0] - lse3[0]).mean(), (lse3[0] - prior[:, 0]).mean()
    if Ll:
        out[3], out[4], out[5] = (own[:, 1] - prior[:, 1]).mean(), (own[:, 1] - lse3[1]).mean(), (lse3[1] - prior[:, 1]).mean()
        out[6] = (lse3[2] - lse3[0] - lse3[1]).mean()
    out[7] = np.log(N)
    return out


# ---------------------------------------------------------------- the bound
def sum_error(chunk):
    return (chunk / RT + 6) * (5 + 3 * np.log(chunk)) * U


def lse_bound(tw, Lg, Ll, chunk=1024, cerr=None):
    """[3,Nq] per-element bound on |device lse - twin lse| for tw = lse(...) (rows 1, 2 NaN when Ll = 0); cerr [Nr,2]: the error of
    the row constants when sv_latent_info_draw made them (None: they were an input of the call)."""
    Nq, Nr = tw["e"][0].shape
    cerr = np.zeros((Nr, 2)) if cerr is None else cerr
    E = [0.5 * (Lg + 7) * U * tw["acc"][0] + cerr[None, :, 0] + U * np.abs(tw["e"][0])]
    if Ll:
        E.append(0.5 * (Ll + 7) * U * tw["acc"][1] + cerr[None, :, 1] + U * np.abs(tw["e"][1]))
        E.append(E[0] + E[1] + U * np.abs(tw["e"][2]))
    out = np.full((3, Nq), np.nan)
    for t, (e, Et) in enumerate(zip(tw["e"], E)):
        raw = _lse_rows(e)
        w = np.exp(e - raw[:, None])
        with np.errstate(over="ignore", invalid="ignore"):
            grow = np.where(w > 0, w * np.exp(np.minimum(Et, 700.0)), 0.0).sum(1)
        tail = np.where(e - e.max(1)[:, None] < -87.0, w, 0.0).sum(1)
        out[t] = np.log(grow) + sum_error(chunk) + tail + 1e-12
    return out


# ---------------------------------------------------------------- the kernel's fp32 arithmetic, operation by operation
def _f32(a):
    return np.asarray(a, F32)


def _exp2(x):
    with np.errstate(under="ignore"):
        return _f32(np.exp2(x.astype(F64)))


def _push(m, s, e, valid):
    with np.errstate(invalid="ignore", over="ignore"):
        d = _f32(e - m)
        x = _exp2(_f32(-np.abs(d) * LOG2E32))
        up = d > 0
        s2 = np.where(up, _f32(s.astype(F64) * x + 1.0), _f32(s + x))
        m2 = np.where(up, e, m)
    use = valid & (e > F32(-3.0e38))
    return np.where(use, m2, m), np.where(use, s2, s)


def _merge(m, s, m2, s2):
    with np.errstate(invalid="ignore", over="ignore"):
        mn = np.maximum(m, m2)
        a = np.where(m == mn, F32(1), _exp2(_f32(_f32(m - mn) * LOG2E32)))
        b = np.where(m2 == mn, F32(1), _exp2(_f32(_f32(m2 - mn) * LOG2E32)))
        return mn, _f32(_f32(s * a) + _f32(s2 * b))


def lse_fp32(z, mu, rsig, cst, Lg, chunk=1024):
    """The arithmetic of li_tile_kernel / li_merge_kernel replayed in NumPy: fp32 subtract, multiply, fused multiply-add (the
    product is exact in fp64), c - 0.5 acc, the per-lane streaming (max, sum), the xor butterfly, the fp64 chunk merge."""
    z, mu, rsig, cst = (_f32(a) for a in (z, mu, rsig, cst))
    Nq, Lc = z.shape
    Nr = mu.shape[0]
    Ll = Lc - Lg

    def score(a, b, col):
        acc = np.zeros((Nq, Nr), F32)
        for d in range(a, b):
            uu = _f32(_f32(z[:, d:d + 1] - mu[None, :, d]) * rsig[None, :, d])
            acc = _f32(uu.astype(F64) * uu.astype(F64) + acc.astype(F64))
        return _f32(cst[None, :, col] - _f32(F32(0.5) * acc))

    es = [score(0, Lg, 0)]
    if Ll:
        es.append(score(Lg, Lc, 1))
        es.append(_f32(es[0] + es[1]))
    out = np.full((3, Nq), np.nan)
    lanes = np.arange(RT)
    for t, e in enumerate(es):
        M, S = np.full(Nq, -np.inf), np.zeros(Nq)
        for c0 in range(0, Nr, chunk):
            c1 = min(Nr, c0 + chunk)
            m, s = np.full((Nq, RT), -np.inf, F32), np.zeros((Nq, RT), F32)
            for n0 in range(c0, c1, RT):
                idx = n0 + lanes
                valid = idx < c1
                ee = np.where(valid[None, :], e[:, np.minimum(idx, c1 - 1)], F32(0))
                m, s = _push(m, s, ee, valid[None, :])
            for o in (32, 16, 8, 4, 2, 1):
                m, s = _merge(m, s, m[:, lanes ^ o], s[:, lanes ^ o])
            m0, s0 = m[:, 0].astype(F64), s[:, 0].astype(F64)
            with np.errstate(invalid="ignore"):
                mn = np.maximum(M, m0)
                S = np.where(S > 0, S * np.exp(M - mn), 0.0) + np.where(s0 > 0, s0 * np.exp(m0 - mn), 0.0)
                M = np.where(s0 > 0, mn, M)
        out[t] = M + np.log(S) - np.log(Nr)
    return out


# ---------------------------------------------------------------- the inputs of the GPU tests
def make_refs(Nr, Lg, Ll, seed):
    """mu, sig [Nr, Lg+Ll] fp32: sig log-uniform in [1e-2, 1]; the rows come in families of about four around a common centre
    (means a quarter of a standard deviation apart, sig within a few per cent), the centres hundreds of standard deviations apart."""
    rng = np.random.default_rng(seed)
    Lc = Lg + Ll
    G = (Nr + 3) // 4
    cm = rng.standard_normal((G, Lc))
    cs = np.exp(rng.uniform(np.log(1e-2), 0.0, (G, Lc)))
    fam = np.arange(Nr) % G
    mu = cm[fam] + 0.25 * cs[fam] * rng.standard_normal((Nr, Lc))
    sig = np.clip(cs[fam] * np.exp(0.05 * rng.standard_normal((Nr, Lc))), 1e-2, 1.0)
    return mu.astype(F32), sig.astype(F32)


def make_case(Nq, Nr, Lg, Ll, seed=0):
    """dict(z [Nq,Lc], mu, sig, rsig [Nr,Lc] fp32, cst [Nr,2] fp32): every query is a sample of one reference's posterior, so it has
    one dominant reference, the three comparable ones of that reference's family, and a far-away tail whose terms flush to zero."""
    mu, sig = make_refs(Nr, Lg, Ll, seed)
    rng = np.random.default_rng(seed + 1000)
    src = (np.arange(Nq) * 7919) % Nr
    src[-1] = Nr - 1                                 # the first and the last reference each dominate a query
    z = (mu[src] + sig[src] * rng.standard_normal((Nq, Lg + Ll)).astype(F32)).astype(F32)
    d = draw(mu, sig, np.zeros_like(mu), Lg)
    return dict(z=z, mu=mu, sig=sig, rsig=d["rsig"], cst=d["c"].astype(F32), Lg=Lg, Ll=Ll)
