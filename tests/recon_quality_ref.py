"""float64 twin of the label-free reconstruction quality report (include/splitvae.h: sv_recon_draw / sv_recon_quality /
sv_recon_finish; split_vae_amd/recon_quality.py), a per-image error bound derived from the kernel's own arithmetic
(csrc/recon_quality.hip), mutants of the twin, and the inputs the GPU tests use.

Definitions (fp32 inputs taken exactly; a = (x_a + 1) / 2, b = clip((x_b + 1) / 2, 0, 1), three channels from a channel offset):
    MSE_i  = mean over H*W*3 of (a - b)^2;   PSNR_i = 10 log10(1 / max(MSE_i, 1e-10))
    window = g g^T, g_k = exp(-(k - 5)^2 / (2 * 1.5^2)) / sum, k = 0..10 (sums to 1)
    per window and channel: mu_a, mu_b, var_a = E[a^2] - mu_a^2, var_b, cov = E[a b] - mu_a mu_b (E = the window's weighted mean)
    ssim   = (2 mu_a mu_b + C1)(2 cov + C2) / ((mu_a^2 + mu_b^2 + C1)(var_a + var_b + C2)),  C1 = 1e-4, C2 = 9e-4
    SSIM_i = mean over the (H-10) x (W-10) valid windows and the three channels

The bound.  The kernel converts every pixel to fp64 as it loads it; everything after that is fp64, u = 2^-53 per operation.  The
rescale (x + 1) * 0.5 of an fp32 x is then exact unless |x| < 2^-29 (absolute error u), and so is the clip.
    d = fl(a - b): |dd| <= u |d| + 2 u.  The squares are summed over at most 18 + 6 + 4 + tiles steps on the device and pairwise here:
        E_mse = (96 + tiles) u MSE + 4 u mean(|d| (|a| + |b| + 1))
    a window sum S_q = sum w_i w_j v_ij goes through a product, 11 vertical and 11 horizontal fused multiply-adds (24 roundings) on the
    device, 2 x 11 multiply-adds here, and the two sets of taps may differ by an ulp each: E_q = 160 u sum w |v|
        mu: E_a, E_b;   var_a: E_aa + 2 |mu_a| E_a + E_a^2 + 4 u (|S_aa| + mu_a^2), var_b likewise
        cov: E_ab + |mu_a| E_b + |mu_b| E_a + E_a E_b + 4 u (|S_ab| + |mu_a mu_b|)
        N1 = 2 mu_a mu_b + C1, D1 = mu_a^2 + mu_b^2 + C1, N2 = 2 cov + C2, D2 = var_a + var_b + C2, each with its propagated error and
        4 u of its own magnitude; ssim = N1 N2 / (D1 D2):
        E = (|N2| dN1 + |N1| dN2 + dN1 dN2 + |ssim| (D2 dD1 + D1 dD2 + dD1 dD2)) / (D1 D2 - that last bracket) + 8 u |ssim|
    E_ssim = mean over windows of E + (96 + tiles) u mean |ssim|
With plain fp32 sums the same derivation gives 22 * 2^-24 on var against C2 = 9e-4, 1.5e-3 relative, which is why the kernel does not
use them; with an fp32 rescale the pair (1.0, 1.0 - 1e-3) would carry 3.6e-4 relative on its MSE.
"""
import numpy as np

U = 2.0 ** -53
F32, F64 = np.float32, np.float64
C1, C2, MSE_FLOOR = 0.01 ** 2, 0.03 ** 2, 1e-10
WIN, SIGMA = 11, 1.5
TR, TC = 8, 75                            # the kernel's tile: output rows per band, output columns per tile
MEANS, KEEP_G, KEEP_L = 0, 1, 2
PARITY = 1e-4                             # the project's stated fp32 parity figure

MUTANTS = ("window_not_normalised", "sample_covariance", "same_padding", "no_clip", "sigma_1", "ten_taps", "c1_c2_swapped",
           "channels_3_5", "channel_mean_dropped", "psnr_of_mean_mse")


def window(n=WIN, sigma=SIGMA, normalise=True):
    k = np.arange(n, dtype=F64) - n // 2
    g = np.exp(-k * k / (2.0 * sigma * sigma))
    return g / g.sum() if normalise else g


def tiles(H, W):
    return -(-(H - 10) // TR) * -(-(W - 10) // TC)


def _planes(a, off_a, b, off_b, clip_b):
    a = (np.asarray(a)[..., off_a:off_a + 3].astype(F64) + 1.0) * 0.5
    b = (np.asarray(b)[..., off_b:off_b + 3].astype(F64) + 1.0) * 0.5
    return a, (np.clip(b, 0.0, 1.0) if clip_b else b)


def _filter(v, g, same):
    """the separable window over axes 1, 2 of v [B,H,W,3]: valid region, or zero-padded 'same'"""
    n = len(g)
    if same:
        lo, hi = (n - 1) // 2, n // 2
        v = np.pad(v, ((0, 0), (lo, hi), (lo, hi), (0, 0)))
    Ho, Wo = v.shape[1] - n + 1, v.shape[2] - n + 1
    t = sum(g[k] * v[:, k:k + Ho] for k in range(n))
    return sum(g[k] * t[:, :, k:k + Wo] for k in range(n))


def moments(a, b, g=None, same=False):
    g = window() if g is None else g
    return tuple(_filter(v, g, same) for v in (a, b, a * a, b * b, a * b))


def quality(a, b, off_a=0, off_b=0, clip_b=True, mutant=None):
    """a [B,H,W,Ca], b [B,H,W,Cb] fp32 -> per_image [B,2] fp64 = (MSE_i, SSIM_i).  mutant: one of MUTANTS (those of this stage)."""
    if mutant == "channels_3_5":
        off_a, off_b = off_a + 3, off_b + 3
    pa, pb = _planes(a, off_a, b, off_b, clip_b and mutant != "no_clip")
    B = pa.shape[0]
    mse = ((pa - pb) ** 2).reshape(B, -1).mean(1)
    g = window(10 if mutant == "ten_taps" else WIN, 1.0 if mutant == "sigma_1" else SIGMA, mutant != "window_not_normalised")
    ma, mb, saa, sbb, sab = moments(pa, pb, g, same=mutant == "same_padding")
    va, vb, cov = saa - ma * ma, sbb - mb * mb, sab - ma * mb
    if mutant == "sample_covariance":
        n = float(len(g) ** 2)
        va, vb, cov = (t * (n / (n - 1.0)) for t in (va, vb, cov))
    c1, c2 = (C2, C1) if mutant == "c1_c2_swapped" else (C1, C2)
    s = ((2.0 * ma * mb + c1) * (2.0 * cov + c2)) / ((ma * ma + mb * mb + c1) * (va + vb + c2))
    ssim = s.reshape(B, -1).mean(1)
    if mutant == "channel_mean_dropped":
        ssim = s.sum(-1).reshape(B, -1).mean(1)
    return np.stack([mse, ssim], axis=1)


def psnr(mse):
    return 10.0 * np.log10(1.0 / np.maximum(np.asarray(mse, F64), MSE_FLOOR))


def finish(per_image, acc=None, mutant=None):
    """acc [3] += (sum PSNR_i, sum SSIM_i, B), added in image order onto the accumulator."""
    acc = [0.0, 0.0, 0.0] if acc is None else [float(v) for v in acc]
    per_image = np.asarray(per_image, F64)
    p = psnr(per_image[:, 0])
    if mutant == "psnr_of_mean_mse":
        p = np.full(len(p), psnr(per_image[:, 0].mean()))
    for i in range(per_image.shape[0]):
        acc[0] += float(p[i])
        acc[1] += float(per_image[i, 1])
    acc[2] += float(per_image.shape[0])
    return np.array(acc, F64)


def bound(a, b, off_a=0, off_b=0, clip_b=True):
    """(E_mse [B], E_ssim [B]): what the kernel's per_image may differ from quality(...) by (the module docstring)."""
    pa, pb = _planes(a, off_a, b, off_b, clip_b)
    B, H, W = pa.shape[:3]
    nt = tiles(H, W)
    d = np.abs(pa - pb)
    mse = (d * d).reshape(B, -1).mean(1)
    e_mse = (96 + nt) * U * mse + 4 * U * (d * (np.abs(pa) + np.abs(pb) + 1.0)).reshape(B, -1).mean(1)
    ma, mb, saa, sbb, sab = moments(pa, pb)
    ea, eb, eaa, ebb, eab = (160 * U * t for t in moments(np.abs(pa), np.abs(pb)))
    va, vb, cov = saa - ma * ma, sbb - mb * mb, sab - ma * mb
    dva = eaa + 2 * np.abs(ma) * ea + ea * ea + 4 * U * (np.abs(saa) + ma * ma)
    dvb = ebb + 2 * np.abs(mb) * eb + eb * eb + 4 * U * (np.abs(sbb) + mb * mb)
    dcov = eab + np.abs(ma) * eb + np.abs(mb) * ea + ea * eb + 4 * U * (np.abs(sab) + np.abs(ma * mb))
    n1, d1, n2, d2 = 2 * ma * mb + C1, ma * ma + mb * mb + C1, 2 * cov + C2, va + vb + C2
    dn1 = 2 * (np.abs(ma) * eb + np.abs(mb) * ea + ea * eb) + 4 * U * (np.abs(n1) + C1)
    dd1 = 2 * np.abs(ma) * ea + 2 * np.abs(mb) * eb + ea * ea + eb * eb + 4 * U * d1
    dn2 = 2 * dcov + 4 * U * (np.abs(n2) + C2)
    dd2 = dva + dvb + 4 * U * (np.abs(va) + np.abs(vb) + C2)
    s = n1 * n2 / (d1 * d2)
    dden = d2 * dd1 + d1 * dd2 + dd1 * dd2
    e = (np.abs(n2) * dn1 + np.abs(n1) * dn2 + dn1 * dn2 + np.abs(s) * dden) / (d1 * d2 - dden) + 8 * U * np.abs(s)
    e_ssim = e.reshape(B, -1).mean(1) + (96 + nt) * U * np.abs(s).reshape(B, -1).mean(1)
    return e_mse, e_ssim


def agrees(got, want, e_mse, e_ssim):
    """THE comparison of the GPU tests and of the mutants: per image, inside the derived bound."""
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    return bool(np.all(np.isfinite(got))) and bool(np.all(np.abs(got[:, 0] - want[:, 0]) <= e_mse)) and \
        bool(np.all(np.abs(got[:, 1] - want[:, 1]) <= e_ssim))


def worst_ratio(got, want, e_mse, e_ssim):
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    return float(max(np.max(np.abs(got[:, 0] - want[:, 0]) / e_mse), np.max(np.abs(got[:, 1] - want[:, 1]) / e_ssim)))


# ---------------------------------------------------------------- sv_recon_draw
def bf16_round(x):
    """fp32 -> the nearest bf16 (ties to even), returned as fp32: what .to(torch.bfloat16) gives for finite values"""
    bits = np.ascontiguousarray(x, F32).view(np.uint32).astype(np.uint64)
    bits = (bits + 0x7fff + ((bits >> 16) & 1)) & 0xffff0000
    return bits.astype(np.uint32).view(F32)


def draw(mg, ml, mode, eps, comp=None, pm=None, ps=None, bf16=False):
    """zcat [B, Lg+Ll] fp32 (bf16-rounded when bf16) of pinned eps [B, Lg+Ll] / comp [B]; ml None: Ll = 0."""
    mg = np.asarray(mg, F32)
    B, Lg = mg.shape
    ml = np.zeros((B, 0), F32) if ml is None else np.asarray(ml, F32)
    eps = np.asarray(eps, F32)
    zg, zl = mg, ml
    if mode == KEEP_G:
        zl = eps[:, Lg:]
    elif mode == KEEP_L:
        zg = eps[:, :Lg]
        if pm is not None:
            c = np.clip(np.asarray(comp), 0, pm.shape[0] - 1)
            zg = (np.asarray(pm, F32)[c] + (np.asarray(ps, F32)[c] * zg).astype(F32)).astype(F32)     # the kernel's fp32 expression
    z = np.concatenate([zg, zl], axis=1).astype(F32)
    return bf16_round(z) if bf16 else z


# ---------------------------------------------------------------- the inputs of the GPU tests
SHAPES = ((3, 11, 11), (2, 12, 37), (5, 32, 32), (2, 64, 64), (1, 64, 64), (7, 32, 32),
          (1, 11, 100))                   # the last one: two column tiles (more than 75 output columns), beyond the issue's list
LAYOUTS = ((6, 0, 6, 0), (6, 3, 6, 3), (3, 0, 3, 0), (6, 0, 3, 0), (9, 3, 6, 0))     # (pitch_a, off_a, pitch_b, off_b)
KINDS = ("textured", "flat", "copies")


def _blur(v, sigma=2.0):
    g = window(9, sigma)
    return _filter(np.pad(v, ((0, 0), (4, 4), (4, 4), (0, 0)), mode="reflect"), g, False)


def images(kind, B, H, W, seed=0):
    """(x_a, x_b) [B,H,W,3] fp32 in the network's domain: the image in [-1,1] and a decoder mean that leaves it in places
    (textured, flat) or equals it (copies)."""
    rng = np.random.default_rng([seed, B, H, W, KINDS.index(kind)])
    if kind == "flat":                    # C2 decides the value: flat, close to 1 after the rescale, noise of 1e-3
        xa = 0.9 + 1e-3 * rng.standard_normal((B, H, W, 3))
        xb = xa + 1e-3 * rng.standard_normal((B, H, W, 3))
        xb[:, ::5, ::3] += 0.2            # some decoder values above 1 (the clip acts)
    else:
        t = _blur(rng.standard_normal((B, H, W, 3)))
        xa = np.clip(t / np.abs(t).max(), -1.0, 1.0)
        xb = xa if kind == "copies" else 1.3 * xa + 0.1 * _blur(rng.standard_normal((B, H, W, 3)), 1.0)
    return xa.astype(F32), xb.astype(F32)


def embed(x, pitch, off, fill=np.nan):
    """x [B,H,W,3] at channels off .. off+2 of a [B,H,W,pitch] buffer whose other channels hold `fill` (NaN: must not be read)"""
    out = np.full(x.shape[:3] + (pitch,), fill, F32)
    out[..., off:off + 3] = x
    return out
