"""float64 twin of the mixture models' importance-weighted bound (include/splitvae.h: sv_iw_gm_advance / sv_iw_gm_tables;
split_vae_amd/iw.py: mixture_log_likelihood): tables from the parameters, the pick from a given uniform, the draw, both mixture
log-densities, the state and the finish (the shared pieces are tests/iw_ref.py's), and a per-element bound on the fp32 kernel's r.

The bound (ratio_bound) is derived from the kernel's arithmetic, one rounding u = 2^-24 per fp32 operation, in first order with a
factor 1.01 for the higher orders.  The inputs (stored z, tables, logits, mu_l, sig_l) are exact.  Per (component c, dimension d):
    a = z - m                      |da| <= u |a|
    t = a / s   (correctly rounded) |dt| <= 2u |t|
    h = t * t / 2                  |dh| <= 5u h            (2 x 2u from t, u of the product; the halving is exact)
    l = logf(s)                    |dl| <= 4u |l|          (the device's logf / expf within 2 ulp; 1 ulp is documented)
    e = h + l                      |de| <= u |e| + dh + dl
    g_c = -sum_d e                 a chain of ceil(Lg / S) subtractions per lane and log2(S) butterfly additions:
                                   |dg_c| <= sum_d de + (ceil(Lg / S) + log2 S) u sum_d |e|
    w_c = g_c + lw_c               |dw_c| <= dg_c + dlw_c + u |w_c|
with lw_c = -logf(n) (|dlw| <= 4u log n) for the prior mixture, and for the posterior mixture lw_c = x_c - logf(total), x_c =
logit_c - max, total = sum_j expf(x_j) cumulated in index order:
    |dlw_c| <= u |x_c| + [sum_j pi_j (u |x_j| + 4u) + n u + n 2^-126] + 4u log n + u |lw_c|
(a rounding of expf's argument is a relative error u |x| of its value; terms that underflow cost at most 2^-126 each of a total
>= 1).  The log-sum-exp LSE = M + logf(sum_c expf(w_c - M)), M the maximum of the computed w: with exact shares p_c,
    |dLSE| <= log sum_c p_c exp(dw_c + u |w_c - M| + 4u)  +  (8u + n 2^-126)  +  4u log n  +  u |LSE|
-- the error of each component enters weighted by its share; the form log sum p exp(d) is the exact worst case of which sum p d is
the first order, and it lets a component 1e3 sigma away carry an error of thousands of nats at a share of exp(-5e5); the sum of
<= 128 terms is two per lane and a 6-step butterfly (8u), logf(sum) has sum in [1, n].
The local ratio, per dimension: q = t^2 - z^2 (|dq| <= 5u t^2 + u z^2 + u |q|), e = q / 2 + logf(sig) (|de| <= dq / 2 + 4u |log
sig| + u |e|), summed by ceil(L / 256) + 9 additions.  r = (LSE_p - LSE_q) + loc adds u |LSE_p - LSE_q| + u |r|.
"""
import math

import numpy as np

import iw_ref

U = 2.0 ** -24
TINY = 2.0 ** -126
HO = 1.01

MUTANTS = ("no_log_pi", "no_log_n", "sigma_squared", "no_max", "short_loop", "pm_ps_swapped", "comp_plus_one", "local_sign",
           "no_log_sigma", "half_dropped", "pi_not_normalised", "local_dropped")


def softplus(x):
    return np.logaddexp(0.0, x)


def elu(x):
    return np.where(x > 0, x, np.expm1(np.minimum(x, 0.0)))


# ---------------------------------------------------------------- tables
def tables(gm_params, he):
    """(zm_all, zs_all [B,n,L], pm, ps [n,L]) float64 from the 24 arrays of the GM encoder (gm_ref.gm_param_shapes order) and he
    [B,512]."""
    p = [np.asarray(a, np.float64) for a in gm_params]
    he = np.asarray(he, np.float64)
    h_top = elu(p[12] + p[13])                                   # one-hot y: row c of the kernel plus the bias
    hh = he[:, None, :] + h_top[None]
    return hh @ p[20] + p[21], softplus(hh @ p[22] + p[23]), p[14] + p[15], softplus(p[16] + p[17])


def encoder_he_logits(gm_params, x):
    """(he [B,512], logits [B,n]) of Encoder.call_gmvae in test mode (no dropout) on oracle/gm_ref.py's float64 layers."""
    import torch
    import torch.nn.functional as F
    from oracle import gm_ref
    p = [torch.as_tensor(np.asarray(a)).double() for a in gm_params]
    h = torch.as_tensor(np.asarray(x)).double()
    for i, stride in ((0, 2), (2, 2), (4, 2)):
        h = gm_ref.conv_elu(h, p[i], p[i + 1], stride)
    h = h.reshape(h.shape[0], -1)
    yh = F.elu(F.elu(h @ p[6] + p[7]) @ p[8] + p[9])
    return F.elu(h @ p[18] + p[19]).numpy(), (yh @ p[10] + p[11]).numpy()


# ---------------------------------------------------------------- the pick and the draw
def pick(logits_row, u):
    """The kernel's inverse CDF in its own fp32 arithmetic: e = exp(logit - max), cumulated in index order; the first index whose
    cumulated mass is >= u * total, else the last."""
    l = np.asarray(logits_row, np.float32)
    e = np.exp((l - l.max()).astype(np.float32)).astype(np.float32)
    total = np.float32(0)
    for v in e:
        total = np.float32(total + v)
    thr, cum = np.float32(np.float32(u) * total), np.float32(0)
    for j, v in enumerate(e):
        cum = np.float32(cum + v)
        if cum >= thr:
            return j
    return len(e) - 1


def philox4x32(key, ctr):
    """Philox4x32-10 in Python integers: key (k0, k1), counter 4 x uint32 -> 4 x uint32."""
    k0, k1 = key
    c = list(ctr)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & 0xffffffff, (p0 >> 32) ^ c[3] ^ k1, p0 & 0xffffffff]
        k0, k1 = (k0 + 0x9E3779B9) & 0xffffffff, (k1 + 0xBB67AE85) & 0xffffffff
    return c


def pick_uniform(seed, image, sample):
    """sv_iw_gm_uniform_host restated: key seed ^ 0x1a7e17a11eed, counter (0, image lo, image hi ^ ('iw' tag | 2), sample)."""
    s = (int(seed) ^ 0x1a7e17a11eed) & 0xffffffffffffffff
    g = int(image) & 0xffffffffffffffff
    c = philox4x32((s & 0xffffffff, s >> 32), [0, g & 0xffffffff, (g >> 32) ^ (0x69770000 + 2), int(sample) & 0xffffffff])
    return float(np.float32(np.float32((c[0] >> 8) + 1.0) * np.float32(1.0 / 16777216.0)))


def draw(zm_all, zs_all, comp, mu_l, sig_l, eps, dtype=np.float64):
    """z [B, Lg + Ll] = (zm_all[b, c] + zs_all[b, c] eps_g | mu_l + sig_l eps_l) in `dtype`."""
    B, n, Lg = zm_all.shape
    idx = np.arange(B)
    c = np.asarray(comp)
    e = np.asarray(eps).astype(dtype)
    zg = zm_all[idx, c].astype(dtype) + zs_all[idx, c].astype(dtype) * e[:, :Lg]
    if mu_l is None:
        return zg
    return np.concatenate([zg, np.asarray(mu_l).astype(dtype) + np.asarray(sig_l).astype(dtype) * e[:, Lg:]], axis=1)


# ---------------------------------------------------------------- r
def _lse(w, dtype, no_max=False):
    if no_max:
        with np.errstate(divide="ignore", over="ignore"):
            return np.log(np.exp(w).astype(dtype).sum(axis=1, dtype=dtype)).astype(dtype)
    m = w.max(axis=1, keepdims=True)
    return (m[:, 0] + np.log(np.exp(w - m).astype(dtype).sum(axis=1, dtype=dtype))).astype(dtype)


def ratio(z, logits, zm_all, zs_all, pm, ps, mu_l=None, sig_l=None, mutant=None, dtype=np.float64):
    """r [B] at the stored latents z [B, Lg + Ll], in `dtype` arithmetic (float64: the twin; float32: a CPU stand-in for the kernel,
    other summation order).  `mutant`: one of MUTANTS (comp_plus_one acts in the draw, not here)."""
    assert mutant is None or mutant in MUTANTS
    c = lambda a: np.asarray(a).astype(dtype)          # noqa: E731
    z, logits, zm_all, zs_all, pm, ps = c(z), c(logits), c(zm_all), c(zs_all), c(pm), c(ps)
    B, n, Lg = zm_all.shape
    if mutant == "pm_ps_swapped":
        pm, ps = ps, pm
    zg = z[:, None, :Lg]
    half = dtype(1.0 if mutant == "half_dropped" else 0.5)

    def g(m, s):
        s_eff = s * s if mutant == "sigma_squared" else s
        t = (zg - m) / s_eff
        e = half * (t * t) + (0 if mutant == "no_log_sigma" else np.log(s_eff))
        return -e.sum(axis=2, dtype=dtype)
    x = logits - logits.max(axis=1, keepdims=True)
    log_pi = x if mutant == "pi_not_normalised" else x - np.log(np.exp(x).sum(axis=1, keepdims=True, dtype=dtype))
    wp = g(pm[None], ps[None]) - (0 if mutant == "no_log_n" else dtype(math.log(n)))
    wq = g(zm_all, zs_all) + (0 if mutant == "no_log_pi" else log_pi)
    if mutant == "short_loop" and n > 1:
        wp, wq = wp[:, :-1], wq[:, :-1]
    r = _lse(wp.astype(dtype), dtype, mutant == "no_max") - _lse(wq.astype(dtype), dtype, mutant == "no_max")
    if mu_l is not None and mutant != "local_dropped":
        mu, sg, zl = c(mu_l), c(sig_l), z[:, Lg:]
        t = (zl - mu) / sg
        loc = (dtype(0.5) * (t * t - zl * zl) + np.log(sg)).sum(axis=1, dtype=dtype)
        r = r - loc if mutant == "local_sign" else r + loc
    return r.astype(dtype)


def _lse_bound(w, dw, n):
    """Bound of one computed log-sum-exp: shares from the exact w [B,n], per-component error dw [B,n]."""
    m = w.max(axis=1, keepdims=True)
    lse = m[:, 0] + np.log(np.exp(w - m).sum(axis=1))
    d = dw + U * np.abs(w - m) + 4 * U
    a = (w - lse[:, None]) + d                                   # log p_c + d_c
    am = a.max(axis=1, keepdims=True)
    share = am[:, 0] + np.log(np.exp(a - am).sum(axis=1))        # log sum p exp(d) >= 0
    return share + 8 * U + n * TINY + 4 * U * math.log(max(n, 2)) + U * np.abs(lse), lse


def ratio_bound(z, logits, zm_all, zs_all, pm, ps, mu_l=None, sig_l=None):
    """Per-image bound [B] on |r_kernel - ratio(...)| (module docstring)."""
    c = lambda a: np.asarray(a).astype(np.float64)     # noqa: E731
    z, logits, zm_all, zs_all, pm, ps = c(z), c(logits), c(zm_all), c(zs_all), c(pm), c(ps)
    B, n, Lg = zm_all.shape
    np2 = 1
    while np2 < n:
        np2 *= 2
    S = min(64, 256 // np2)
    n_add = -(-Lg // S) + int(math.log2(S))
    zg = z[:, None, :Lg]

    def g(m, s):
        t = (zg - m) / s
        h, l = 0.5 * t * t, np.log(s)
        e = h + l
        de = U * np.abs(e) + 5 * U * h + 4 * U * np.abs(l)
        return -e.sum(axis=2), de.sum(axis=2) + n_add * U * np.abs(e).sum(axis=2)
    x = logits - logits.max(axis=1, keepdims=True)
    ex = np.exp(x)
    total = ex.sum(axis=1, keepdims=True)
    pi = ex / total
    lw_q = x - np.log(total)
    d_total = (pi * (U * np.abs(x) + 4 * U)).sum(axis=1, keepdims=True) + n * U + n * TINY
    dlw_q = U * np.abs(x) + d_total + 4 * U * math.log(max(n, 2)) + U * np.abs(lw_q)
    gp, dgp = g(pm[None], ps[None])
    gq, dgq = g(zm_all, zs_all)
    wp, wq = gp - math.log(n), gq + lw_q
    bp, lp = _lse_bound(wp, dgp + 4 * U * math.log(max(n, 2)) + U * np.abs(wp), n)
    bq, lq = _lse_bound(wq, dgq + dlw_q + U * np.abs(wq), n)
    r = lp - lq
    bound = bp + bq + U * np.abs(r)
    if mu_l is not None:
        mu, sg, zl = c(mu_l), c(sig_l), z[:, Lg:]
        t = (zl - mu) / sg
        q, l = t * t - zl * zl, np.log(sg)
        e = 0.5 * q + l
        de = 0.5 * (5 * U * t * t + U * zl * zl + U * np.abs(q)) + 4 * U * np.abs(l) + U * np.abs(e)
        bound = bound + de.sum(axis=1) + (-(-(z.shape[1]) // 256) + 9) * U * np.abs(e).sum(axis=1)
        r = r + e.sum(axis=1)
    return HO * (bound + U * np.abs(r))


def lgvae_ratio_bound(mu, sig, eps):
    """Bound [B] on |r of sv_iw_advance (fp32 plan) - iw_ref.latent_ratio at the STORED z|.  That kernel scores the eps it drew:
    e = (eps^2 - z^2) / 2 + logf(sig), z = fl(mu + fl(sig eps)), so |dz| <= u |sig eps| + u |z| and the twin's t = (z - mu) / sig
    differs from eps by dz / sig: |eps^2 - t^2| / 2 <= |eps| dz / sig (first order).  Its own arithmetic: u each for eps^2, z^2 and
    their difference, 4u |log sig|, u |e|, and ceil(L / 64) + 6 additions of the wave's sum."""
    c = lambda a: np.asarray(a).astype(np.float64)     # noqa: E731
    mu, sig, eps = c(mu), c(sig), c(eps)
    z = mu + sig * eps
    dz = U * np.abs(sig * eps) + U * np.abs(z)
    q, l = eps * eps - z * z, np.log(sig)
    e = 0.5 * q + l
    de = np.abs(eps) * dz / sig + 0.5 * (U * eps * eps + U * z * z + U * np.abs(q)) + 4 * U * np.abs(l) + U * np.abs(e)
    return HO * (de.sum(axis=1) + (-(-mu.shape[1] // 64) + 6) * U * np.abs(e).sum(axis=1))


# ---------------------------------------------------------------- the whole estimator on the fp64 oracle
def estimator(params_np, images6, split, eps=None, comp=None, z_stored=None):
    """(out3 [B,3], r [K,B], z [K,B,Lg+Ll]) float64.  params_np: the 54 arrays of LGGMVae (split) or the 34 of GMVae; images6
    [B,H,W,6]; comp [K,B]; eps [K,B,Lg+Ll] (the draw in float64) or z_stored [K,B,Lg+Ll] (the latents a plan stored, decoded and
    scored as they are)."""
    import torch
    from oracle import torch_ref as tr
    P = [np.asarray(p) for p in params_np]
    T = lambda a: torch.as_tensor(np.asarray(a)).double()      # noqa: E731
    img = T(images6)
    H, W = img.shape[1:3]
    x, xh = img[..., :3], img[..., 3:]
    he, logits = encoder_he_logits(P[:24], x.numpy())
    zm_all, zs_all, pm, ps = tables(P[:24], he)
    Lg = pm.shape[1]
    mu_l = sig_l = None
    if split:
        Ll = P[30].shape[1]
        _, mu_l, sig_l = tr.encoder_conv(xh, [T(p) for p in P[24:34]], torch.zeros((img.shape[0], Ll), dtype=torch.float64))
        mu_l, sig_l = mu_l.numpy(), sig_l.numpy()
        dec_x, dec_h = [T(p) for p in P[34:44]], [T(p) for p in P[44:54]]
    else:
        dec_x = [T(p) for p in P[24:34]]
    K = (eps if z_stored is None else z_stored).shape[0]
    st = iw_ref.state_init(img.shape[0])
    rs, zs = [], []
    for k in range(K):
        z = draw(zm_all, zs_all, comp[k], mu_l, sig_l, eps[k]) if z_stored is None else np.asarray(z_stored[k], np.float64)
        r = ratio(z, logits, zm_all, zs_all, pm, ps, mu_l, sig_l)
        xm, xls = tr.decoder(T(z), dec_x, H, W)
        nll_x = tr.discretised_logistic_loss(x, xm, xls).sum(dim=(1, 2, 3)).numpy()
        nll_h = np.zeros_like(nll_x)
        if split:
            hm, hls = tr.decoder(T(z[:, Lg:]), dec_h, H, W)
            nll_h = tr.discretised_logistic_loss(xh, hm, hls).sum(dim=(1, 2, 3)).numpy()
        st = iw_ref.state_push(st, nll_x, nll_h, r)
        rs.append(r)
        zs.append(z)
    return iw_ref.finish(st, K), np.stack(rs), np.stack(zs)


# ---------------------------------------------------------------- the inputs of the kernel cases (GPU and host tests share them)
def gaussian_case(B, n, Lg, Ll, seed):
    """Gaussian parameters: means ~ N(0, 1), sigmas in [0.3, 2], logits ~ 2 N(0, 1), eps ~ N(0, 1), comp uniform."""
    rng = np.random.default_rng(seed)
    f = np.float32
    d = dict(logits=(2 * rng.standard_normal((B, n))).astype(f), zm_all=rng.standard_normal((B, n, Lg)).astype(f),
             zs_all=rng.uniform(0.3, 2.0, (B, n, Lg)).astype(f), pm=rng.standard_normal((n, Lg)).astype(f),
             ps=rng.uniform(0.3, 2.0, (n, Lg)).astype(f), eps=rng.standard_normal((B, Lg + Ll)).astype(f),
             comp=rng.integers(0, n, B).astype(np.int32), mu_l=None, sig_l=None)
    if Ll:
        d["mu_l"], d["sig_l"] = rng.standard_normal((B, Ll)).astype(f), rng.uniform(0.3, 2.0, (B, Ll)).astype(f)
    return d


def adversarial_case(name, seed=0):
    """The adversarial inputs of the issue, each a change of a Gaussian case (B = 3, n = 30 unless said)."""
    f = np.float32
    d = gaussian_case(3, 30, 8, 5, 100 + seed)
    B, n, Lg = d["zm_all"].shape
    idx = np.arange(B)
    if name == "far_components":          # every component but the drawn one (and one prior component) 1e3 sigma away from z
        c = d["comp"]
        far = (1e3 * d["zs_all"] * np.sign(d["zm_all"] + 0.5)).astype(f)
        keep = d["zm_all"][idx, c].copy()
        d["zm_all"] = (d["zm_all"] + far).astype(f)
        d["zm_all"][idx, c] = keep
        d["pm"][1:] = (d["pm"][1:] + 1e3 * d["ps"][1:]).astype(f)
    elif name == "all_far":               # both mixtures hundreds of sigmas from z everywhere: exp underflows without the maximum
        d["pm"] = (d["pm"] + 300 * d["ps"]).astype(f)
        d["eps"][:, :Lg] = f(40.0)        # the drawn component itself 40 sigma out: g = -800 Lg
    elif name == "tiny_and_large_sigma":  # sigma = 8e-7 and sigma = 50 side by side
        d["zs_all"][:, ::2] = f(8e-7)
        d["zs_all"][:, 1::2] = f(50.0)
        d["ps"][::2] = f(8e-7)
        d["ps"][1::2] = f(50.0)
        d["sig_l"][:, 0], d["sig_l"][:, 1] = f(8e-7), f(50.0)
    elif name == "logit_spread":          # logits over +-80
        d["logits"] = np.linspace(-80, 80, B * n).reshape(B, n).astype(f)[:, ::-1].copy()
    elif name == "twin_components":       # two identical components, the drawn one among them
        c = d["comp"]
        o = (c + 1) % n
        for a in ("zm_all", "zs_all"):
            d[a][idx, o] = d[a][idx, c]
        d["logits"][idx, o] = d["logits"][idx, c]
        d["pm"][1], d["ps"][1] = d["pm"][0], d["ps"][0]
    elif name == "pi_on_last":            # pi concentrated on the last component
        d["logits"][:] = f(-30.0)
        d["logits"][:, -1] = f(30.0)
        d["comp"][:] = n - 1
    else:
        raise KeyError(name)
    return d


ADVERSARIAL = ("far_components", "all_far", "tiny_and_large_sigma", "logit_spread", "twin_components", "pi_on_last")
# the pinned-draw shapes: B in {1, 3, 65}, n in {1, 2, 30, 128}, Lg in {1, 8, 128, 200}, Ll in {0, 5, 128}, and one Lg beyond the
# dimensions the kernel keeps in LDS (2048)
SHAPES = [(1, 1, 1, 0), (3, 1, 8, 5), (3, 2, 1, 5), (65, 2, 8, 0), (3, 30, 128, 128), (65, 30, 8, 5), (1, 30, 200, 0), (3, 30, 200, 128),
          (3, 128, 8, 0), (1, 128, 128, 5), (65, 128, 1, 128), (3, 128, 200, 5), (1, 2, 2500, 5)]


def case_inputs():
    """[(id, dict)] of every r case: the Gaussian shapes and the adversarial ones."""
    out = [("gauss-B%d-n%d-Lg%d-Ll%d" % s, gaussian_case(*s, seed=i)) for i, s in enumerate(SHAPES)]
    return out + [(name, adversarial_case(name)) for name in ADVERSARIAL]
