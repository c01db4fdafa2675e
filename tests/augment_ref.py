"""fp64 numpy restatement of the reference's augmentations other than `scramble` (augmentation.py:33-38, :59-101), per image, NHWC.
The test oracle of split_vae_amd/csrc/augment.hip; no TensorFlow.  Line numbers are the reference's augmentation.py."""
import math

import numpy as np

MIX_SIZES = (1, 2, 4, 8)          # :41 np.random.choice([1,2,4,8])


def normal_prob(t, mean, std):
    """tfp.distributions.Normal(mean, std).prob(t) (:35-36)."""
    t = np.asarray(t, np.float64)
    return np.exp(-0.5 * ((t - mean) / std) ** 2) / (std * math.sqrt(2 * math.pi))


def gaussian_kernel(size, mean, std):
    """:33-38: vals = Normal(mean, std).prob(range(-size, size+1)); outer(vals, vals) / sum -> [2size+1, 2size+1]."""
    vals = normal_prob(np.arange(-size, size + 1), mean, std)
    k = np.einsum('i,j->ij', vals, vals)
    return k / k.sum()


def gaussian_taps(size, mean, std):
    """The 1-D factor w of gaussian_kernel: K = outer(w, w), w = vals / sum(vals)."""
    vals = normal_prob(np.arange(-size, size + 1), mean, std)
    return vals / vals.sum()


def symmetric_index(i, n):
    """tf.pad(..., 'SYMMETRIC') (:91-92, :28): mirror including the edge element, -1 -> 0, n -> n-1 (numpy mode='symmetric')."""
    return -i - 1 if i < 0 else (2 * n - 1 - i if i >= n else i)


def pad_symmetric(x, r):
    """x[H,W,C] -> [H+2r, W+2r, C], paddings [[r,r],[r,r],[0,0]] (:91, :28)."""
    return np.pad(np.asarray(x, np.float64), ((r, r), (r, r), (0, 0)), mode='symmetric')


def depthwise_valid(xp, k):
    """tf.nn.separable_conv2d(pad(x)[None], tile(k)[..., None, None], eye(3), padding='VALID') (:92, :98): a per-channel
    cross-correlation, out[y, x, c] = sum_{i,j} xp[y+i, x+j, c] k[i, j]; the pointwise eye(3) is the identity."""
    kh, kw = k.shape
    H, W = xp.shape[0] - kh + 1, xp.shape[1] - kw + 1
    out = np.zeros((H, W, xp.shape[2]), np.float64)
    for i in range(kh):
        for j in range(kw):
            out += k[i, j] * xp[i:i + H, j:j + W, :]
    return out


def gaussian_filter(x, size, mean, std):
    """The low-pass image of one [H,W,C] image: depthwise_valid(pad_symmetric(x, size), gaussian_kernel(size, mean, std))."""
    return depthwise_valid(pad_symmetric(x, size), gaussian_kernel(size, mean, std))


def gaussian_filter_separable(x, size, mean, std):
    """The same as a row pass then a column pass with the 1-D taps (what augment.hip runs)."""
    w = gaussian_taps(size, mean, std)
    xp = pad_symmetric(x, size)
    H, W = xp.shape[0] - 2 * size, xp.shape[1] - 2 * size
    rows = np.zeros((xp.shape[0], W, xp.shape[2]), np.float64)
    for j in range(2 * size + 1):
        rows += w[j] * xp[:, j:j + W, :]
    out = np.zeros((H, W, xp.shape[2]), np.float64)
    for i in range(2 * size + 1):
        out += w[i] * rows[i:i + H, :, :]
    return out


def gaussian_blur(x, radius, std):
    """:83-94 for one image with its draws pinned (radius = `size` of :87, std of :86, mean 0): concat([x, blur(x)], -1)."""
    x = np.asarray(x, np.float64)
    return np.concatenate([x, gaussian_filter(x, radius, 0.0, std)], axis=-1)


def gaussian_blur_batch(x, radius, std):
    return np.stack([gaussian_blur(x[b], int(radius[b]), float(std[b])) for b in range(x.shape[0])], 0)


def high_low_pass(x, size, mean=0.0, std=1.0):
    """:97-101 (kernel and paddings of :23-28): concat([x, x - low, low], -1)."""
    x = np.asarray(x, np.float64)
    low = gaussian_filter(x, size, mean, std)
    return np.concatenate([x, x - low, low], axis=-1)


def high_low_pass_batch(x, size, mean=0.0, std=1.0):
    return np.stack([high_low_pass(x[b], size, mean, std) for b in range(x.shape[0])], 0)


def scramble(x, perm, size):
    """:70-81 with the shuffle pinned: destination patch n (row-major over the (H/size) x (W/size) grid) takes source patch
    perm[n]."""
    H, W, C = x.shape
    G = W // size
    n = (H // size) * G
    patches = x.reshape(H // size, size, G, size, C).transpose(0, 2, 1, 3, 4).reshape(n, size, size, C)
    patches = patches[np.asarray(perm[:n])]
    aug = patches.reshape(H // size, G, size, size, C).transpose(0, 2, 1, 3, 4).reshape(H, W, C)
    return np.concatenate([x, aug], axis=-1)


def mix_scramble_batch(x, perm, sizes):
    """mix_scramble (:59-81) with a patch size per image (the per-image variant the commented-out :60-64 intended); perm[b]
    holds the permutation of image b's (H/sizes[b])^2 patches in its first entries."""
    return np.stack([scramble(x[b], perm[b], int(sizes[b])) for b in range(x.shape[0])], 0)


# ===================================================================================================================== kernel-level parity (tests/test_gpu_augment_kernels.py)
# What follows restates csrc/augment.hip kernel by kernel: the Gaussian filter with the scale and the sum of |addends| of every element and the bound they give, a
# float32 run of the kernel's own summation order with switchable defects, the Philox draws on tape_ref.philox4x32_10, the mixed-size permutation and gather, and
# the case tables of the GPU tests.  tests/test_augment_host.py holds all of it to hand-computable cases and asserts what every case promises.
import os  # noqa: E402
import sys  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pointwise_ref import FLT_MIN, ULP, random_perm  # noqa: E402
from tape_ref import philox4x32_10  # noqa: E402

F32_RTOL, ADDEND_ATOL = 1e-4, 1e-5                                 # the project's rule for an fp32 output (tests/pointwise_ref.py): 1e-4 |ref| + 1e-5 scale


def _window_reduce(a, w, size, op):
    """a [H + 2 size, W + 2 size, C] >= 0, w [2 size + 1] >= 0 -> [H, W, C]: op over (i, j) of w[i] w[j] a[y + i, x + j]; separable because nothing is negative"""
    H, W = a.shape[0] - 2 * size, a.shape[1] - 2 * size
    rows = None
    for j in range(2 * size + 1):
        t = w[j] * a[:, j:j + W, :]
        rows = t if rows is None else op(rows, t)
    out = None
    for i in range(2 * size + 1):
        t = w[i] * rows[i:i + H, :, :]
        out = t if out is None else op(out, t)
    return out


def gaussian_filter_with_scale(x, size, mean, std):
    """One [H, W, C] image -> (low, scale, sumabs), float64: low = gaussian_filter(x, size, mean, std) summed separably; per element
    sumabs = sum_{a,b} |w_a w_b x_pad| and scale = max_{a,b} |w_a w_b x_pad|, the largest |addend|."""
    w = gaussian_taps(size, float(mean), float(std))
    xp = pad_symmetric(x, size)
    low = _window_reduce(xp, w, size, np.add) if size else xp.copy()         # (signed: the sum of products is separable whatever the signs)
    ax = np.abs(xp)
    return low, _window_reduce(ax, w, size, np.maximum), _window_reduce(ax, w, size, np.add)


# ULP is 2^-24: what one correctly rounded fp32 operation adds, relative.  The three operations of gauss_taps that are not correctly rounded by contract, in units of
# it, at the accuracy the OpenCL C specification sets for single precision, which the ROCm device library is built to: x / y 2.5 ulp, exp 3 ulp, log 3 ulp.
DIV_HULP, EXPF_HULP, LOGF_HULP = 5, 6, 6
HALF_LOG_2PI = 0.91893853320467274178


def gauss_tap_hulp(r, mean, std):
    """The relative error of one fp32 tap w[k] = v[k] / s of gauss_taps, in units of ULP, at the outermost tap (the largest |z|), where it is largest.
      z = ((k - r) - mean) / std       the subtraction 1, the division DIV                                                  z (1 + dz),  dz = 1 + DIV
      q = 0.5 z z                      twice dz and the product's rounding; 0.5 is exact                                    an ABSOLUTE q (2 dz + 1) in the exponent
      log_norm = logf(std) + c         LOGF on |log std|, the rounding of the constant c = 0.9189, the add's on |log_norm|  absolute LOGF |log std| + c + |log_norm|
                                       (the same float for every tap of an image: most of it cancels in v / s; the bound does not lean on that)
      a = -q - log_norm                the argument-rounding term: one rounding of a number no larger than q + |log_norm|   absolute q + |log_norm|
      v = expf(a)                      an absolute error of the argument is a relative one of the result, plus EXPF
      s = sum v                        all v > 0: the weighted mean of their errors <= the largest, and 2r + 1 add roundings
      w = v / s                        DIV
    -> 2 rel(v) + (2r + 1) + DIV"""
    mean, std = float(mean), float(std)
    zmax = (r + abs(mean)) / std
    q = 0.5 * zmax * zmax
    ln = abs(math.log(std) + HALF_LOG_2PI)
    dz = 1 + DIV_HULP
    rel_v = q * (2 * dz + 1) + (LOGF_HULP * abs(math.log(std)) + HALF_LOG_2PI + ln) + (q + ln) + EXPF_HULP
    return 2.0 * rel_v + (2 * r + 1) + DIV_HULP


def gauss_chain_hulp(r):
    """The operation count of the two (2r + 1)-term chains `a += w[k] * p` (built with -ffp-contract=off: a product and an add each): 2 * 2 (2r + 1).  An addend
    passes through one product and at most 2r + 1 adds per pass, 2 (2r + 2) roundings in all, each at most ULP of a partial sum that no sum of |addends| falls short
    of: the count covers it for every r."""
    return 4 * (2 * r + 1)


def gauss_bound(ref, scale, sumabs, r, mean, std, xmax=0.0):
    """|gpu - ref| allowed per element: the project's rule 1e-4 |ref| + 1e-5 scale, plus the sum term (chain + tap) ULP sumabs.  Every one of the (2r+1)^2 addends
    w_a w_b x carries the roundings of the two chains (gauss_chain_hulp) and the relative errors of its taps: `tap` is what the taps put on an addend, and an addend
    has two of them, so it is twice gauss_tap_hulp, the figure of one tap.  No partial sum exceeds sumabs.  (r = 0: the one tap is v / v = 1 and the chains add it
    to zero, so the kernel is exact there; the term is not made smaller for it.)
    xmax: the largest |x| of the image, for the floor of taps below FLT_MIN (2^-126), which the GPU flushes to zero and float64 keeps: at most FLT_MIN / s
    absolute in w, 2r + 1 of them per pass, two passes, the other pass's taps summing to one: 2 (2r + 1) FLT_MIN / s xmax."""
    mean, std = float(mean), float(std)
    s = float(normal_prob(np.arange(-r, r + 1), mean, std).sum())
    floor = 2 * (2 * r + 1) * FLT_MIN / s * xmax
    return F32_RTOL * np.abs(ref) + ADDEND_ATOL * scale + (gauss_chain_hulp(r) + 2.0 * gauss_tap_hulp(r, mean, std)) * ULP * sumabs + floor


def clamp_radius(r, max_radius):
    """the documented clamp of sv_gauss_blur: a radius outside [0, max_radius] is clamped to it"""
    return min(max(int(r), 0), int(max_radius))


# --------------------------------------------------------------------------------------------------------------------- the kernel's own order, in float32
DEFECTS = ("reflect", "drop_last_tap", "unnormalised", "mean_sign", "column_unfiltered", "no_clamp")


def gauss_taps_f32(r, mean, std, normalise=True):
    """gauss_taps of augment.hip operation by operation in NumPy float32 (NumPy's exp and log are rounded at least as well as the device's)"""
    f = np.float32
    mean, std = f(mean), f(std)
    log_norm = f(np.log(std) + f(HALF_LOG_2PI))
    w = np.zeros(2 * r + 1, f)
    s = f(0)
    for k in range(2 * r + 1):
        z = f((f(k - r) - mean) / std)
        w[k] = np.exp(f(f(f(f(-0.5) * z) * z) - log_norm))
        s = f(s + w[k])
    return (w / s).astype(f) if normalise else w


def gauss_emulate_f32(x, r, mean, std, defect=None, max_radius=None):
    """One [H, W, 3] float32 image -> low [H, W, 3] float32 the way gauss_filter_kernel forms it: the radius clamped to [0, max_radius] (None: r as given), the taps
    of gauss_taps, the row pass over the mirrored rows, then the column pass, k ascending, a product and an add per step.
    defect: one wrong kernel of DEFECTS; each reads inside the mirrored image only (none models an out-of-range access):
      reflect            the mirror excludes the edge pixel (-1 -> 1, numpy 'reflect')
      drop_last_tap      both passes stop at k < 2r
      unnormalised       the taps are v, not v / s
      mean_sign          -mean: the taps reversed, a convolution where TensorFlow's conv is a cross-correlation
      column_unfiltered  the column pass reads the staged rows, not the row-filtered ones
      no_clamp           the radius is used as it comes (a negative one: no taps, a sum of nothing)"""
    assert defect is None or defect in DEFECTS, defect
    f = np.float32
    x = np.asarray(x, f)
    H, W, _ = x.shape
    if max_radius is not None and defect != "no_clamp":
        r = clamp_radius(r, max_radius)
    if r < 0:
        return np.zeros_like(x)
    w = gauss_taps_f32(r, -float(mean) if defect == "mean_sign" else mean, std, normalise=defect != "unnormalised")
    nk = 2 * r if defect == "drop_last_tap" else 2 * r + 1
    xs = np.pad(x, ((r, r), (r, r), (0, 0)), mode="reflect" if defect == "reflect" else "symmetric")
    hs = np.zeros((H + 2 * r, W, 3), f)
    for k in range(nk):
        hs = (hs + (w[k] * xs[:, k:k + W, :]).astype(f)).astype(f)
    src = xs[:, r:r + W, :] if defect == "column_unfiltered" else hs
    low = np.zeros((H, W, 3), f)
    for k in range(nk):
        low = (low + (w[k] * src[k:k + H, :, :]).astype(f)).astype(f)
    return low


# --------------------------------------------------------------------------------------------------------------------- Philox draws
BLUR_TAG, MIX_TAG = 0x626c757200000001, 0x6d69787300000002
M64 = 0xFFFFFFFFFFFFFFFF


def aug_draw(B, tag, seed, step, offset):
    """aug_draw of augment.hip for samples offset .. offset + B - 1: key seed ^ tag, counter (gs lo, gs hi, step lo, step hi) -> uint32 [B, 4]"""
    gs = (np.uint64(offset & M64) + np.arange(B, dtype=np.uint64))
    ctr = np.zeros((B, 4), dtype=np.uint32)
    ctr[:, 0] = (gs & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    ctr[:, 1] = (gs >> np.uint64(32)).astype(np.uint32)
    ctr[:, 2] = np.uint32(step & 0xFFFFFFFF)
    ctr[:, 3] = np.uint32((step >> 32) & 0xFFFFFFFF)
    return philox4x32_10(ctr, (seed ^ tag) & M64)


def blur_params(B, seed, step=0, offset=0):
    """blur_params_kernel -> (radius int32 [B], exact; std float64 [B] = 5 + 5 (c1 >> 8) / 2^24, the value the kernel rounds to fp32 in two steps or one)"""
    c = aug_draw(B, BLUR_TAG, seed, step, offset)
    return (3 + (c[:, 0] >> np.uint32(30))).astype(np.int32), 5.0 + 5.0 * (c[:, 1] >> np.uint32(8)).astype(np.float64) / 16777216.0


def mix_sizes(B, seed, step=0, offset=0):
    """mix_sizes_kernel / sv_mix_size_host -> int32 [B], exact: 1 << (c0 >> 30)"""
    c = aug_draw(B, MIX_TAG, seed, step, offset)
    return (1 << (c[:, 0] >> np.uint32(30)).astype(np.int64)).astype(np.int32)


# the s < 10 ? s : 9.99999905f branch of blur_params_kernel: a draw with c1 >> 8 == 2^24 - 1 gives 5 + 5 (1 - 2^-24), which fp32 rounds to 10.  Found by running
# aug_draw over samples 0 .. 2^27 - 1 of this seed and step (5 hits: 602308, 18118458, 77324059, 124939758, 126314834; this is the first).
STD_CLAMP_DRAW = dict(seed=0xF234567890ABCDEF, step=(3 << 32) | 5, sample=602308)
STD_BELOW_10 = np.float32(9.99999905)


def mix_valid(s, H, ld):
    """mix_valid of augment.hip: s | H and (H / s)^2 <= min(ld, 4096)"""
    if s <= 0 or s > H or H % s:
        return False
    g = H // s
    return g * g <= ld and g * g <= 4096


def random_perm_mixed(sizes, H, ld, seed, step=0, offset=0, prefill=-1):
    """random_perm_mixed_kernel -> int32 [B, ld]: row b holds pointwise_ref.random_perm of (H / sizes[b])^2 patches for sample offset + b in its first entries; what
    lies behind them, and the whole row of an invalid size, keeps the prefill"""
    out = np.full((len(sizes), ld), prefill, dtype=np.int32)
    for b, s in enumerate(sizes):
        if mix_valid(int(s), H, ld):
            n = (H // int(s)) ** 2
            out[b, :n] = random_perm(1, n, seed, step, offset + b)[0]
    return out


def mix_gather_ref(x, perm, sizes, ld):
    """scramble_mixed_kernel's documented semantics.  x [B, H, H, 3] float32, perm a flat int32 array read at pitch ld, sizes [B] -> [B, H, H, 6] float32 (copies only:
    bit for bit).  Destination patch n of image b takes source patch perm[b * ld + n]; a patch whose entry is outside [0, (H / s)^2), and every patch of an image
    whose size is invalid, is copied through.  Rows need not be permutations."""
    x = np.asarray(x, np.float32)
    B, H = x.shape[0], x.shape[1]
    perm = np.asarray(perm).reshape(-1)
    out = np.concatenate([x, x], axis=-1)
    for b in range(B):
        s = int(sizes[b])
        if not mix_valid(s, H, ld):
            continue
        G = H // s
        for n in range(G * G):
            p = int(perm[b * ld + n])
            if 0 <= p < G * G:
                r, c, pr, pc = n // G, n % G, p // G, p % G
                out[b, r * s:(r + 1) * s, c * s:(c + 1) * s, 3:] = x[b, pr * s:(pr + 1) * s, pc * s:(pc + 1) * s, :]
    return out


# --------------------------------------------------------------------------------------------------------------------- case tables
GAUSS_MAX_LDS = 64 * 1024


def gauss_band_rows(H, W, rmax):
    """gauss_band_rows of augment.hip: (br + 2 rmax) W 24 <= 65536, br tried from min(H, 16) and halved; 0: nothing fits"""
    br = min(H, 16)
    while br >= 1:
        if (br + 2 * rmax) * W * 3 * 4 * 2 <= GAUSS_MAX_LDS:
            return br
        br >>= 1
    return 0


def gauss_staging(W, x_offset_floats=0):
    """which staging loop gauss_filter_kernel takes: the float4 one iff a row is a whole number of float4 and x is 16-byte aligned (a torch allocation is; an
    offset of x_offset_floats floats into it moves it by 4 bytes each)"""
    return "vector" if (W * 3) % 4 == 0 and (x_offset_floats * 4) % 16 == 0 else "scalar"


class GaussCase:
    """One Gaussian-filter case.  call: 'blur' (radii, stds per image, max_radius; mean 0) or 'hlp' (size, mean, std for every image of a batch of B).  band_rows,
    bands, staging: what the header's formula gives, recorded here and asserted in tests/test_augment_host.py; x_offset: floats between the allocation and x."""

    def __init__(self, name, why, H, call, band_rows, bands, staging, radii=None, stds=None, max_radius=None, B=None, size=None, mean=0.0, std=1.0, x_offset=0):
        self.name, self.why, self.H, self.call, self.band_rows, self.bands, self.staging, self.x_offset = name, why, H, call, band_rows, bands, staging, x_offset
        if call == "blur":
            self.radii, self.stds, self.rmax, self.B, self.mean = list(radii), [float(np.float32(s)) for s in stds], max_radius, len(radii), 0.0
            assert len(self.stds) == self.B
        else:
            self.radii, self.stds, self.rmax, self.B, self.mean = [size] * B, [float(np.float32(std))] * B, size, B, float(np.float32(mean))

    def x(self):
        """the images, float32 [B, H, H, 3] in [-1, 1], seeded by the case"""
        return np.random.default_rng(1000 + GAUSS_CASES.index(self)).uniform(-1.0, 1.0, (self.B, self.H, self.H, 3)).astype(np.float32)

    def used_radii(self):
        return [clamp_radius(r, self.rmax) for r in self.radii]

    def __repr__(self):
        return self.name


GAUSS_CASES = [
    GaussCase("h8_double_mirror", "r = H: the halo mirrors at both ends on both axes; radius 0 beside it; one band", 8, "blur", 8, 1, "vector",
              radii=[0, 1, 3, 7, 8, 8], stds=[0.5, 1.0, 2.5, 5.0, 7.5, 9.99], max_radius=8),
    GaussCase("h6_scalar", "18 floats per row: the scalar staging loop", 6, "blur", 6, 1, "scalar", radii=[0, 2, 5, 6], stds=[5.0, 6.5, 8.0, 9.5], max_radius=6),
    GaussCase("h10_hlp_asym", "scalar staging, one 10-row band, asymmetric taps (mean -0.7)", 10, "hlp", 10, 1, "scalar", B=3, size=4, mean=-0.7, std=0.8),
    GaussCase("h21_halo_2h1", "16 + 5 row bands, scalar staging, a halo of 2H + 1 rows", 21, "blur", 16, 2, "scalar", radii=[21, 21], stds=[6.0, 9.0], max_radius=21),
    GaussCase("h24_bands_16_8", "16 + 8 row bands", 24, "blur", 16, 2, "vector", radii=[3, 4, 5, 6], stds=[5.0, 6.25, 7.5, 9.75], max_radius=6),
    GaussCase("h40_hlp_bands_16_16_8", "16 + 16 + 8 row bands, mean 0.5", 40, "hlp", 16, 3, "vector", B=2, size=8, mean=0.5, std=1.0),
    GaussCase("h64_hlp_underflow", "std 0.3 at size 8: the outer taps underflow in fp32", 64, "hlp", 16, 4, "vector", B=2, size=8, mean=0.0, std=0.3),
    GaussCase("h64_hlp_size20", "size 20: 2-row bands, 32 of them", 64, "hlp", 2, 32, "vector", B=2, size=20, mean=0.0, std=1.0),
    GaussCase("h128_bands_of_8", "H = 128 at r = 6: 8-row bands", 128, "blur", 8, 16, "vector", radii=[6, 6], stds=[5.5, 9.0], max_radius=6),
    GaussCase("h8_misaligned_x", "x one float into a larger buffer: scalar staging from a misaligned pointer", 8, "blur", 8, 1, "scalar",
              radii=[3, 8, 5], stds=[5.0, 7.0, 9.0], max_radius=8, x_offset=1),
    GaussCase("h16_clamp", "radii outside [0, max_radius]: must equal the reference at [0, 6, 6, 0]", 16, "blur", 16, 1, "vector",
              radii=[-3, 9, 6, 0], stds=[5.0, 6.0, 7.0, 8.0], max_radius=6),
]

_GAUSS_REF = {}


def gauss_case_reference(case):
    """-> (x float32 [B, H, H, 3], low float64 [B, H, H, 3], bound [B, H, H, 3]) of a case, at the clamped radii; computed once and shared (do not write to them)"""
    if case.name not in _GAUSS_REF:
        x = case.x()
        low, bound = np.zeros(x.shape), np.zeros(x.shape)
        for b, (r, sd) in enumerate(zip(case.used_radii(), case.stds)):
            low[b], scale, sumabs = gaussian_filter_with_scale(x[b], r, case.mean, sd)
            bound[b] = gauss_bound(low[b], scale, sumabs, r, case.mean, sd, xmax=float(np.abs(x[b]).max()))
        _GAUSS_REF[case.name] = (x, low, bound)
    return _GAUSS_REF[case.name]


SEED, STEP, OFFSET = 0xF234567890ABCDEF, (3 << 32) | 5, (1 << 32) + 5     # tests/test_gpu_pointwise.py: high seed bits, step high word set, offset above 2^32
DRAW_B = (1, 255, 256, 257, 1000)

# sv_random_perm_mixed: (name, H, sizes, ld, why).  ld None: the largest n of the row's valid sizes
PERM_CASES = [
    ("h8_all_sizes", 8, [8, 4, 2, 1, 3, 0, -2, 16], 64, "every valid size of H = 8 (n = 1, 4, 16, 64) and four invalid ones; ld = the largest n"),
    ("h8_wide_ld", 8, [8, 4, 2, 1, 3, 0, -2, 16], 71, "ld larger than the largest n: entries behind a row's n keep the prefill"),
    ("h8_ld16", 8, [8, 4, 2, 1], 16, "ld = 16 < 64: the size-1 row is invalid and unwritten"),
    ("h64_extremes", 64, [1, 8, 64], 4096, "n = 4096 (the largest the sort holds), 64, and 1 (npow2 = 1: the bitonic loops do nothing)"),
    ("h64_wide_ld", 64, [64, 1, 8], 4101, "the same with ld > 4096"),
    ("h128_s1_invalid", 128, [1, 2, 128], 16384, "H = 128, s = 1: 16384 patches > 4096, invalid whatever ld; s = 2 (n = 4096) and s = 128 (n = 1) beside it"),
]

# sv_scramble_gather_mixed: (name, H, sizes, ld, rows, why).  rows: per image 'perm' (a permutation), 'oob' (entries -1, G^2 and 2^30 among a permutation's),
# 'repeat' (entries drawn with repetition)
MIX_CASES = [
    ("h8_every_size", 8, [1, 2, 4, 8], 64, ["perm"] * 4, "H = 8, every valid size"),
    ("h16_every_size", 16, [1, 2, 4, 8, 16], 256, ["perm"] * 5, "H = 16, every valid size"),
    ("h8_invalid_sizes", 8, [3, 0, -2, 16, 4, 1], 16, ["perm"] * 6, "invalid sizes, and size 1 made invalid by ld = 16 < 64: copied through"),
    ("h16_out_of_range", 16, [1, 2, 4, 8, 16], 256, ["oob"] * 5, "entries -1, G^2 and 2^30: those patches are copied through, the others gathered"),
    ("h8_repeats", 8, [1, 2, 4], 64, ["repeat"] * 3, "rows that are no permutations"),
    ("h16_wide_ld", 16, [2, 1, 16, 4], 263, ["perm", "oob", "perm", "repeat"], "ld wider than the row: the pitch, not n, separates the rows"),
    ("h64_second_trip", 64, None, 4096, None, "B = 257 at H = 64: 1 052 672 pixels against the 1 048 576 of the capped grid, the last image the second trip's alone"),
]
MIX_GRID_PIXELS = 4096 * 256


def mix_case_inputs(name):
    """-> x float32 [B, H, H, 3], perm int32 flat [B * ld + 3] (three entries of slack behind the last row, never read), sizes int32 [B], ld"""
    k = [c[0] for c in MIX_CASES].index(name)
    _, H, sizes, ld, rows, _ = MIX_CASES[k]
    rng = np.random.default_rng(2000 + k)
    if sizes is None:                                               # the second-trip case: sizes drawn by the mirror, every row a permutation
        B = 257
        sizes = [int(s) * 2 for s in mix_sizes(B, 11, 0, 0)]        # 2, 4, 8, 16
        sizes[-1] = 2
        rows = ["perm"] * B
    B = len(sizes)
    x = rng.uniform(-1.0, 1.0, (B, H, H, 3)).astype(np.float32)
    perm = np.full(B * ld + 3, -1, dtype=np.int32)
    for b, (s, kind) in enumerate(zip(sizes, rows)):
        n = (H // s) ** 2 if (s > 0 and s <= H and H % s == 0) else 0
        n = min(n, ld) if n else min(ld, 16)                        # (an invalid size: a row of plausible entries, which a kernel that took it would follow)
        if kind == "repeat":
            row = rng.integers(0, max(n, 1), n)
        else:
            row = rng.permutation(n)
            if kind == "oob" and n >= 1:
                for j, v in zip(rng.permutation(n)[:3], (-1, n, 1 << 30)):
                    row[j] = v
        perm[b * ld:b * ld + n] = row
    return x, perm, np.asarray(sizes, np.int32), ld
