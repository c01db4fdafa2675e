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
