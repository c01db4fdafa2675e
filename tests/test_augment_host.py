"""CPU: the fp64 oracle of the blur / high-low-pass / mixed-scramble augmentations (tests/augment_ref.py) against hand-written
rules, the argument validation of their C-ABI entries (no device work), and the Augmentator / CLI surface that selects them."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_ref as ar  # noqa: E402


# ---------------------------------------------------------------- oracle KATs
def test_symmetric_padding_is_the_hand_written_index_rule():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((7, 7, 3))
    for r in range(0, 8):
        xp = ar.pad_symmetric(x, r)
        assert xp.shape == (7 + 2 * r, 7 + 2 * r, 3)
        for i in range(-r, 7 + r):
            for j in range(-r, 7 + r):
                assert np.array_equal(xp[i + r, j + r], x[ar.symmetric_index(i, 7), ar.symmetric_index(j, 7)])
    # the edge pixel itself is mirrored: -1 -> 0, H -> H-1 (numpy 'symmetric', not 'reflect')
    assert ar.symmetric_index(-1, 7) == 0 and ar.symmetric_index(7, 7) == 6 and ar.symmetric_index(-3, 7) == 2


@pytest.mark.parametrize("size,mean,std", [(0, 0.0, 1.0), (1, 0.0, 1.0), (3, 0.0, 5.0), (6, 0.0, 9.5), (4, 0.5, 1.0), (8, 0.0, 1.0)])
def test_separable_filter_equals_the_2d_kernel(size, mean, std):
    x = np.random.default_rng(size).standard_normal((16, 16, 3))
    w = ar.gaussian_taps(size, mean, std)
    assert np.allclose(np.outer(w, w), ar.gaussian_kernel(size, mean, std), rtol=0, atol=1e-15)
    assert np.abs(ar.gaussian_filter(x, size, mean, std) - ar.gaussian_filter_separable(x, size, mean, std)).max() < 1e-12


def test_delta_image_returns_the_kernel_cross_correlation_oriented():
    """tf.nn.separable_conv2d is a cross-correlation: a delta at (c, c) gives low[c - a, c - b] = K[a + r, b + r].  With mean 0.5
    the kernel is asymmetric, so a convolution (flipped taps) would fail this."""
    r, c, mean = 3, 8, 0.5
    x = np.zeros((17, 17, 3))
    x[c, c, :] = 1.0
    K = ar.gaussian_kernel(r, mean, 1.0)
    assert not np.allclose(K, K[::-1, ::-1])
    low = ar.gaussian_filter(x, r, mean, 1.0)
    for a in range(-r, r + 1):
        for b in range(-r, r + 1):
            assert abs(low[c - a, c - b, 1] - K[a + r, b + r]) < 1e-15
    assert abs(low.sum() / 3 - 1.0) < 1e-12


def test_constant_image_is_preserved_and_high_plus_low_is_x():
    x = np.full((12, 12, 3), 0.37)
    for r, std in ((3, 5.0), (6, 9.9), (0, 1.0)):
        assert np.abs(ar.gaussian_blur(x, r, std)[..., 3:] - 0.37).max() < 1e-14
    y = np.random.default_rng(1).standard_normal((12, 12, 3))
    out = ar.high_low_pass(y, 4, 0.5, 1.0)
    assert out.shape == (12, 12, 9)
    assert np.abs(out[..., 3:6] + out[..., 6:9] - y).max() < 1e-14 and np.array_equal(out[..., :3], y)


def test_mixed_scramble_oracle_is_a_per_image_scramble():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((3, 8, 8, 3))
    sizes = [1, 2, 8]
    perm = np.full((3, 64), -1)
    for b, s in enumerate(sizes):
        perm[b, :(8 // s) ** 2] = rng.permutation((8 // s) ** 2)
    out = ar.mix_scramble_batch(x, perm, sizes)
    assert np.array_equal(out[2, ..., 3:], x[2])                  # one 8x8 patch: identity
    # a patch size of 1 moves single pixels: destination pixel n is source pixel perm[n]
    assert np.array_equal(out[0, ..., 3:].reshape(64, 3), x[0].reshape(64, 3)[perm[0]])
    assert sorted(out[1, ..., 3:].reshape(-1).tolist()) == sorted(x[1].reshape(-1).tolist())


# ---------------------------------------------------------------- C-ABI validation (returns before any launch)
def test_augment_entry_points_validate_arguments(lib_built):
    from split_vae_amd import _lib
    lib = _lib.load()
    BAD, UNS = _lib.STATUS_BADARG, _lib.STATUS_UNSUPPORTED
    p = C.c_void_p(256)          # never dereferenced: every call below fails validation first
    assert lib.sv_gauss_blur(None, p, p, p, 2, 32, 32, 6, None) == BAD
    assert lib.sv_gauss_blur(p, p, p, p, 0, 32, 32, 6, None) == BAD
    assert lib.sv_gauss_blur(p, p, p, p, 2, 32, 32, -1, None) == BAD
    assert lib.sv_gauss_blur(p, p, p, p, 2, 32, 16, 6, None) == UNS            # non-square
    assert lib.sv_gauss_blur(p, p, p, p, 2, 4, 4, 6, None) == UNS              # radius > H
    assert lib.sv_gauss_blur_staged(p, p, p, p, p, p, 7, 2, 32, 32, 6, None) == BAD        # dtype
    assert lib.sv_gauss_blur_staged(p, p, p, p, None, p, 0, 2, 32, 32, 6, None) == BAD
    assert lib.sv_high_low_pass(p, p, 2, 32, 32, 4, 0.0, 0.0, None) == BAD    # std <= 0
    assert lib.sv_high_low_pass(p, p, 2, 32, 32, 33, 0.0, 1.0, None) == UNS   # size > H
    assert lib.sv_high_low_pass(p, p, 2, 32, 32, -1, 0.0, 1.0, None) == BAD
    assert lib.sv_high_low_pass(p, p, 2, 256, 256, 60, 0.0, 1.0, None) == UNS  # the staged rows do not fit the LDS
    assert lib.sv_high_low_pass_staged(p, p, p, p, 0, 2, 32, 24, 4, 0.0, 1.0, None) == UNS
    assert lib.sv_blur_params(None, p, 4, 0, 0, 0, None) == BAD
    assert lib.sv_blur_params(p, p, 0, 0, 0, 0, None) == BAD
    assert lib.sv_mix_sizes(None, 4, 0, 0, 0, None) == BAD
    assert lib.sv_random_perm_mixed(p, None, 4, 32, 1024, 0, 0, 0, None) == BAD
    assert lib.sv_random_perm_mixed(p, p, 4, 32, 0, 0, 0, 0, None) == BAD
    assert lib.sv_scramble_gather_mixed(p, p, p, 0, p, 2, 32, 32, None) == BAD
    assert lib.sv_scramble_gather_mixed(p, p, p, 1024, p, 2, 32, 16, None) == UNS
    assert lib.sv_scramble_gather_mixed_staged(p, p, p, 1024, p, p, p, 3, 2, 32, 32, None) == BAD


def test_host_size_draw_is_reproducible_and_covers_the_choices(lib_built):
    """sv_mix_size_host: np.random.choice([1, 2, 4, 8]) (augmentation.py:41) as a Philox draw -- no device needed."""
    from split_vae_amd import ops
    draws = [ops.mix_size_host(7, 0, i) for i in range(4000)]
    assert set(draws) == {1, 2, 4, 8}
    counts = np.bincount([int(np.log2(d)) for d in draws], minlength=4)
    assert counts.min() > 850 and counts.max() < 1150, counts
    assert draws == [ops.mix_size_host(7, 0, i) for i in range(4000)]
    assert draws != [ops.mix_size_host(8, 0, i) for i in range(4000)]


def test_staged_entry_points_refuse_misaligned_outputs_and_filters_a_batch_beyond_the_grid(lib_built):
    """x8 / xh8 are stored as uint4: a pointer off the 16-byte boundary is SV_E_BADARG.  The filter's grid is (bands, B): B > 65535 is SV_E_UNSUPPORTED.  Both are
    answered before any launch (the pointers are host memory and never dereferenced)."""
    from split_vae_amd import _lib
    lib = _lib.load()
    BAD, UNS = _lib.STATUS_BADARG, _lib.STATUS_UNSUPPORTED
    buf = (C.c_float * 64)()
    a = (C.addressof(buf) + 15) // 16 * 16
    for dt in (_lib.SV_F32, _lib.SV_BF16):
        for off in (2, 4, 8):
            for x8, xh8 in ((a + off, a), (a, a + off)):
                assert lib.sv_gauss_blur_staged(a, a, a, a, x8, xh8, dt, 2, 32, 32, 6, None) == BAD
                assert lib.sv_high_low_pass_staged(a, a, x8, xh8, dt, 2, 32, 32, 4, 0.0, 1.0, None) == BAD
                assert lib.sv_scramble_gather_mixed_staged(a, a, a, 1024, a, x8, xh8, dt, 2, 32, 32, None) == BAD
    p = C.c_void_p(256)
    assert lib.sv_gauss_blur(p, p, p, p, 65536, 32, 32, 6, None) == UNS
    assert lib.sv_gauss_blur_staged(p, p, p, p, p, p, 0, 65536, 32, 32, 6, None) == UNS
    assert lib.sv_high_low_pass(p, p, 65536, 32, 32, 4, 0.0, 1.0, None) == UNS
    assert lib.sv_high_low_pass_staged(p, p, p, p, 0, 1 << 20, 32, 32, 4, 0.0, 1.0, None) == UNS


# ---------------------------------------------------------------- the kernel-level restatements (tests/test_gpu_augment_kernels.py compares the kernels with them)
def test_filter_with_scale_is_the_existing_filter_and_its_scales_are_what_they_say():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((9, 9, 3))
    for size, mean, std in ((0, 0.0, 1.0), (1, 0.0, 1.0), (3, 0.5, 1.0), (9, 0.0, 5.0)):
        low, scale, sumabs = ar.gaussian_filter_with_scale(x, size, mean, std)
        assert np.abs(low - ar.gaussian_filter(x, size, mean, std)).max() < 1e-13
        lowa, _, sumabs_a = ar.gaussian_filter_with_scale(np.abs(x), size, mean, std)
        assert np.abs(sumabs - lowa).max() < 1e-13 and np.abs(sumabs_a - lowa).max() < 1e-13         # the sum of |addends| is the filter of |x|
        assert (scale <= sumabs + 1e-15).all() and (sumabs <= (2 * size + 1) ** 2 * scale + 1e-15).all() and (np.abs(low) <= sumabs + 1e-15).all()
    low, scale, sumabs = ar.gaussian_filter_with_scale(x, 0, 0.0, 1.0)
    assert np.array_equal(low, x) and np.array_equal(scale, np.abs(x)) and np.array_equal(sumabs, np.abs(x))
    # by hand: a delta of 2 at the centre of a 5 x 5 image, r = 1: one addend per output element, so scale = sumabs = |low| = 2 K
    d = np.zeros((5, 5, 3))
    d[2, 2] = 2.0
    low, scale, sumabs = ar.gaussian_filter_with_scale(d, 1, 0.0, 1.0)
    K = ar.gaussian_kernel(1, 0.0, 1.0)
    assert np.abs(low[1:4, 1:4, 0] - 2.0 * K[::-1, ::-1]).max() < 1e-15 and np.abs(scale - low).max() < 1e-15 and np.abs(sumabs - low).max() < 1e-15


def test_bound_terms_are_the_derivation():
    """the sum term by hand at r = 1, mean 0, std 1: chain 4 * 3 = 12; a tap: z = 1, q = 0.5, |log_norm| = c = 0.9189, dz = 6: rel(v) = 0.5 * 13 + (0 + c + c) + (0.5
    + c) + 6 = 15.757, tap = 2 * 15.757 + 3 + 5 = 39.51; an addend carries two taps"""
    c = ar.HALF_LOG_2PI
    assert ar.gauss_chain_hulp(1) == 12 and ar.gauss_chain_hulp(0) == 4 and ar.gauss_chain_hulp(21) == 4 * 43
    assert abs(ar.gauss_tap_hulp(1, 0.0, 1.0) - (2 * (6.5 + 2 * c + 0.5 + c + 6) + 3 + 5)) < 1e-12
    assert ar.gauss_tap_hulp(4, -0.7, 0.8) == ar.gauss_tap_hulp(4, 0.7, 0.8) > ar.gauss_tap_hulp(4, 0.0, 0.8)
    one = np.ones(1)
    b = ar.gauss_bound(2.0 * one, 0.5 * one, 3.0 * one, 1, 0.0, 1.0)
    assert abs(b[0] - (2e-4 + 0.5e-5 + (12 + 2 * ar.gauss_tap_hulp(1, 0.0, 1.0)) * 2.0 ** -24 * 3.0)) < 1e-18
    assert ar.gauss_bound(0 * one, 0 * one, 0 * one, 3, 0.0, 5.0)[0] == 0.0                          # nothing to add: an exact zero is wanted
    assert [ar.clamp_radius(r, 6) for r in (-3, 9, 6, 0)] == [0, 6, 6, 0]


def test_f32_taps_and_emulation_follow_the_float64_restatement():
    for r, mean, std in ((0, 0.0, 1.0), (3, 0.0, 5.0), (4, -0.7, 0.8), (8, 0.0, 0.3)):
        w32, w64 = ar.gauss_taps_f32(r, mean, std).astype(np.float64), ar.gaussian_taps(r, float(np.float32(mean)), float(np.float32(std)))
        s = ar.normal_prob(np.arange(-r, r + 1), float(np.float32(mean)), float(np.float32(std))).sum()
        assert (np.abs(w32 - w64) <= ar.gauss_tap_hulp(r, mean, std) * ar.ULP * w64 + ar.FLT_MIN / s).all()         # (the floor: a v below FLT_MIN, gauss_bound)
    assert ar.gauss_taps_f32(0, 0.3, 2.0)[0] == 1.0
    w = ar.gauss_taps_f32(8, 0.0, 0.3)
    assert w[0] == 0.0 and w[16] == 0.0 and 0 < w[4] < ar.FLT_MIN and w[8] > 0.99                                             # size 8 at std 0.3: the outer taps underflow
    x = np.random.default_rng(6).uniform(-1, 1, (7, 7, 3)).astype(np.float32)
    assert np.array_equal(ar.gauss_emulate_f32(x, 0, 0.0, 1.0), x)
    assert np.abs(ar.gauss_emulate_f32(x, 7, 0.5, 2.0) - ar.gaussian_filter(x, 7, 0.5, 2.0)).max() < 2e-6
    assert np.array_equal(ar.gauss_emulate_f32(x, 9, 0.0, 5.0, max_radius=6), ar.gauss_emulate_f32(x, 6, 0.0, 5.0))
    assert np.array_equal(ar.gauss_emulate_f32(x, -3, 0.0, 5.0, max_radius=6), x)
    assert not ar.gauss_emulate_f32(x, -3, 0.0, 5.0, max_radius=6, defect="no_clamp").any()


def test_philox_mirrors_against_the_library_and_by_hand(lib_built):
    """mix_sizes against sv_mix_size_host (the same aug_draw on the host: key, counter layout and the high words), blur_params' ranges, and the recorded draw that
    reaches the std clamp"""
    from split_vae_amd import _lib
    lib = _lib.load()
    for seed, step, off in ((ar.SEED, ar.STEP, ar.OFFSET), (7, 0, 0), (ar.SEED, 5, 3)):
        got = ar.mix_sizes(300, seed, step, off)
        assert got.tolist() == [lib.sv_mix_size_host(seed, step, off + b) for b in range(300)]
        assert set(got.tolist()) == {1, 2, 4, 8}
    assert ar.mix_sizes(300, ar.SEED, ar.STEP, ar.OFFSET).tolist() != ar.mix_sizes(300, ar.SEED, 5, ar.OFFSET).tolist()           # the step's high word is in the counter
    r, s = ar.blur_params(1000, ar.SEED, ar.STEP, ar.OFFSET)
    assert r.dtype == np.int32 and set(r.tolist()) == {3, 4, 5, 6} and s.dtype == np.float64 and (s >= 5).all() and (s < 10).all()
    c = ar.aug_draw(1000, ar.BLUR_TAG, ar.SEED, ar.STEP, ar.OFFSET)
    assert np.array_equal(r, 3 + (c[:, 0] >> 30)) and np.array_equal(s, 5 + 5 * (c[:, 1] >> 8) / 2.0 ** 24)
    assert np.array_equal(ar.blur_params(10, ar.SEED, ar.STEP, ar.OFFSET + 990)[1], s[990:])                                       # a shard draws the batch's rows
    d = ar.STD_CLAMP_DRAW
    c = ar.aug_draw(1, ar.BLUR_TAG, d["seed"], d["step"], d["sample"])
    assert int(c[0, 1]) >> 8 == (1 << 24) - 1
    u = np.float32(int(c[0, 1]) >> 8) * np.float32(1.0 / 16777216.0)
    assert np.float32(5) + np.float32(5) * u == np.float32(10) and ar.STD_BELOW_10 < 10 and np.nextafter(ar.STD_BELOW_10, np.float32(11)) == np.float32(10)


def test_mixed_permutation_and_gather_restatements():
    import pointwise_ref as R
    sizes = [8, 4, 2, 1, 3, 0, -2, 16]
    p = ar.random_perm_mixed(sizes, 8, 70, ar.SEED, ar.STEP, ar.OFFSET, prefill=-9)
    assert p.shape == (8, 70) and p.dtype == np.int32
    for b, s in enumerate(sizes):
        n = (8 // s) ** 2 if s in (8, 4, 2, 1) else 0
        assert np.array_equal(p[b, :n], R.random_perm(1, n, ar.SEED, ar.STEP, ar.OFFSET + b)[0]) if n else True
        assert sorted(p[b, :n].tolist()) == list(range(n)) and (p[b, n:] == -9).all()
    assert p[0, 0] == 0                                                                              # n = 1: the one patch
    assert (ar.random_perm_mixed([1, 2], 8, 16, 1, prefill=-9)[0] == -9).all()                       # 64 patches do not fit ld = 16
    assert (ar.random_perm_mixed([1], 128, 16384, 1, prefill=-9) == -9).all()                        # 16384 > 4096
    # the gather: permutations give mix_scramble_batch; by hand: one out-of-range entry copies that patch through, a repeated entry copies a patch twice
    rng = np.random.default_rng(8)
    x = rng.standard_normal((3, 8, 8, 3)).astype(np.float32)
    sz = [1, 2, 8]
    perm = np.full((3, 67), -1, np.int32)
    for b, s in enumerate(sz):
        perm[b, :(8 // s) ** 2] = rng.permutation((8 // s) ** 2)
    assert np.array_equal(ar.mix_gather_ref(x, perm, sz, 67), ar.mix_scramble_batch(x, perm, sz).astype(np.float32))
    q = np.array([3, 3, 4, -1], np.int32)                                                            # H = 4, s = 2: patches 0 and 1 take 3, patch 2 and 3 stay
    y = rng.standard_normal((1, 4, 4, 3)).astype(np.float32)
    out = ar.mix_gather_ref(y, q, [2], 4)
    assert np.array_equal(out[..., :3], y) and np.array_equal(out[0, :2, :2, 3:], y[0, 2:, 2:]) and np.array_equal(out[0, :2, 2:, 3:], y[0, 2:, 2:])
    assert np.array_equal(out[0, 2:, :, 3:], y[0, 2:, :])
    for bad in (3, 0, -2, 8):
        assert np.array_equal(ar.mix_gather_ref(y, np.zeros(16, np.int32), [bad], 16)[..., 3:], y)
    assert np.array_equal(ar.mix_gather_ref(y, np.zeros(16, np.int32), [1], 15)[..., 3:], y)         # 16 patches, ld = 15


def test_every_case_meets_the_conditions_its_name_promises():
    names = [c.name for c in ar.GAUSS_CASES]
    assert len(set(names)) == len(names) == 11
    for c in ar.GAUSS_CASES:
        H = c.H
        assert 2 <= c.B <= 6 and c.band_rows == ar.gauss_band_rows(H, H, c.rmax) and c.bands == -(-H // c.band_rows), c
        assert c.staging == ar.gauss_staging(H, c.x_offset) and (c.band_rows + 2 * c.rmax) * H * 24 <= 65536 and c.rmax <= H, c
        assert all(s > 0 for s in c.stds) and c.x().shape == (c.B, H, H, 3) and c.x().dtype == np.float32
    g = {c.name: c for c in ar.GAUSS_CASES}
    c = g["h8_double_mirror"]
    assert c.radii == [0, 1, 3, 7, 8, 8] and c.rmax == 8 == c.H and c.bands == 1 and min(c.stds) == 0.5 and abs(max(c.stds) - 9.99) < 1e-6
    assert g["h6_scalar"].staging == "scalar" and g["h6_scalar"].H * 3 == 18 and g["h6_scalar"].radii == [0, 2, 5, 6]
    c = g["h10_hlp_asym"]
    assert c.call == "hlp" and c.staging == "scalar" and (c.band_rows, c.bands) == (10, 1) and c.rmax == 4 and abs(c.mean + 0.7) < 1e-6 and abs(c.stds[0] - 0.8) < 1e-6
    w = ar.gaussian_taps(4, c.mean, c.stds[0])
    assert not np.allclose(w, w[::-1])
    c = g["h21_halo_2h1"]
    assert c.staging == "scalar" and (c.band_rows, c.bands) == (16, 2) and 21 % 16 == 5 and 21 in c.radii and 2 * c.rmax + 1 == 2 * c.H + 1
    assert (g["h24_bands_16_8"].band_rows, g["h24_bands_16_8"].bands, 24 % 16) == (16, 2, 8) and g["h24_bands_16_8"].radii == [3, 4, 5, 6]
    c = g["h40_hlp_bands_16_16_8"]
    assert c.call == "hlp" and (c.band_rows, c.bands, 40 - 32) == (16, 3, 8) and (c.rmax, c.mean, c.stds[0]) == (8, 0.5, 1.0)
    c = g["h64_hlp_underflow"]
    w = ar.gauss_taps_f32(c.rmax, c.mean, c.stds[0])
    assert c.call == "hlp" and c.H == 64 and c.rmax == 8 and abs(c.stds[0] - 0.3) < 1e-6 and w[0] == 0 and w[-1] == 0 and ar.gaussian_taps(8, 0.0, c.stds[0])[0] > 0
    c = g["h64_hlp_size20"]
    assert c.call == "hlp" and (c.H, c.rmax, c.band_rows, c.bands) == (64, 20, 2, 32)
    c = g["h128_bands_of_8"]
    assert (c.H, c.rmax, c.band_rows, c.bands) == (128, 6, 8, 16) and set(c.radii) == {6}
    c = g["h8_misaligned_x"]
    assert c.x_offset == 1 and c.staging == "scalar" and ar.gauss_staging(8, 0) == "vector" and ar.gauss_staging(8, 4) == "vector"
    c = g["h16_clamp"]
    assert c.radii == [-3, 9, 6, 0] and c.rmax == 6 and c.used_radii() == [0, 6, 6, 0]
    # permutation cases
    p = {c[0]: c for c in ar.PERM_CASES}
    valid = lambda c: [ar.mix_valid(s, c[1], c[3]) for s in c[2]]                                    # noqa: E731
    assert p["h8_all_sizes"][2] == [8, 4, 2, 1, 3, 0, -2, 16] and valid(p["h8_all_sizes"]) == [True] * 4 + [False] * 4 and p["h8_all_sizes"][3] == 64
    assert p["h8_wide_ld"][3] > 64 and valid(p["h8_wide_ld"]) == [True] * 4 + [False] * 4
    assert p["h8_ld16"][3] == 16 and valid(p["h8_ld16"]) == [True, True, True, False] and p["h8_ld16"][2][3] == 1
    assert p["h64_extremes"][2] == [1, 8, 64] and p["h64_extremes"][3] == 4096 == (64 // 1) ** 2 and valid(p["h64_extremes"]) == [True] * 3
    assert p["h64_wide_ld"][3] > 4096 and valid(p["h64_wide_ld"]) == [True] * 3
    assert p["h128_s1_invalid"][1:4] == (128, [1, 2, 128], 16384) and valid(p["h128_s1_invalid"]) == [False, True, True]
    # gather cases
    for name, H, sizes, ld, rows, _ in ar.MIX_CASES:
        x, perm, sz, ld2 = ar.mix_case_inputs(name)
        B = len(sz)
        assert ld2 == ld and x.shape == (B, H, H, 3) and perm.shape == (B * ld + 3,) and perm.dtype == np.int32 and sz.dtype == np.int32
        want = ar.mix_gather_ref(x, perm, sz, ld)
        ok = np.array([ar.mix_valid(int(s), H, ld) for s in sz])
        same = np.array([np.array_equal(want[b, ..., 3:], x[b]) for b in range(B)])
        if name in ("h8_every_size", "h16_every_size"):
            assert ok.all() and sorted(sz.tolist()) == [s for s in (1, 2, 4, 8, 16) if s <= H]
            assert not same[sz < H].any() and same[sz == H].all()                                   # every image with more than one patch is moved
        if name == "h8_invalid_sizes":
            assert sz.tolist() == [3, 0, -2, 16, 4, 1] and ok.tolist() == [False] * 4 + [True, False] and same.tolist() == [True] * 4 + [False, True]
        if name == "h16_out_of_range":
            for b, s in enumerate(sz.tolist()):
                n = (H // s) ** 2
                row = perm[b * ld:b * ld + n].tolist()
                assert row.count(-1) == 1 and (n < 3 or (row.count(n) == 1 and row.count(1 << 30) == 1))
        if name == "h8_repeats":
            assert all(len(set(perm[b * ld:b * ld + (H // int(s)) ** 2].tolist())) < (H // int(s)) ** 2 for b, s in enumerate(sz))
        if name == "h16_wide_ld":
            assert ld > H * H and ok.all()
        if name == "h64_second_trip":
            assert B == 257 and H == 64 and B * H * H > ar.MIX_GRID_PIXELS >= (B - 1) * H * H and ok.all() and not same[-1] and set(sz.tolist()) == {2, 4, 8, 16}


def _worst(case, defect=None):
    """the largest |emulation - float64 reference| / gauss_bound over a case"""
    x, low, bound = ar.gauss_case_reference(case)
    worst = 0.0
    for b, (r, sd) in enumerate(zip(case.radii, case.stds)):
        emu = ar.gauss_emulate_f32(x[b], r, case.mean, sd, defect=defect, max_radius=case.rmax).astype(np.float64)
        err = np.abs(emu - low[b])
        assert np.isfinite(emu).all() and ((bound[b] > 0) | (err == 0)).all()
        worst = max(worst, float((err / np.maximum(bound[b], 1e-300)).max()))
    return worst


@pytest.mark.parametrize("case", ar.GAUSS_CASES, ids=repr)
def test_emulation_stays_within_half_the_bound(case):
    """the float32 run of the kernel's own order, without a defect, against the float64 reference: the condition that the reference and the bound fit each other"""
    w = _worst(case)
    print("%-24s emulation: worst err / bound %.4f" % (case.name, w))
    assert w <= 0.5, (case.name, w)


@pytest.mark.parametrize("defect", ar.DEFECTS)
def test_each_defect_breaks_the_bound_on_some_case(defect):
    caught = {c.name: _worst(c, defect) for c in ar.GAUSS_CASES}
    print(defect, {k: round(v, 2) for k, v in caught.items()})
    assert max(caught.values()) > 1.0, (defect, caught)
    if defect == "mean_sign":                                       # only the asymmetric cases can see it
        assert all((v > 1.0) == (k in ("h10_hlp_asym", "h40_hlp_bands_16_16_8")) for k, v in caught.items()), caught
    if defect == "no_clamp":
        assert caught["h16_clamp"] > 1.0 and all(v <= 0.5 for k, v in caught.items() if k != "h16_clamp"), caught


# ---------------------------------------------------------------- Augmentator / CLI surface
def test_reference_augmentator_selects_every_reference_type():
    """augmentation.py:15-30: ReferenceAugmentator constructs for all five values of --augmentation (it does not exist without this
    feature); Augmentator keeps selecting scramble / no_op only, as before."""
    from split_vae_amd.augmentation import TYPES, Augmentator, ReferenceAugmentator
    assert TYPES == ('scramble', 'mix_scramble', 'blur', 'high_low_pass', 'no_op')
    a = ReferenceAugmentator("scramble", size=8)
    assert a.augment == a.scramble and a.size == 8 and a.channels == 6
    assert ReferenceAugmentator("no_op").augment("x") == "x"
    b = ReferenceAugmentator("blur")
    assert b.augment == b.blur and b.channels == 6
    h = ReferenceAugmentator("high_low_pass", size=4, mean=0.5)
    assert h.augment == h.high_low_pass and h.channels == 9 and (h.size, h.mean, h.std) == (4, 0.5, 1.0)
    m = ReferenceAugmentator("mix_scramble")
    assert m.augment == m.mix_scramble and not m.per_image
    assert ReferenceAugmentator("mix_scramble", per_image=True).per_image
    with pytest.raises(ValueError):
        ReferenceAugmentator("high_low_pass", size=2, std=0)
    with pytest.raises(ValueError):
        ReferenceAugmentator("nope")
    for t in ("mix_scramble", "blur", "high_low_pass"):
        with pytest.raises(NotImplementedError, match="ReferenceAugmentator"):
            Augmentator(t)
    assert isinstance(ReferenceAugmentator("blur"), Augmentator)


def test_mix_scramble_draws_one_size_per_pipeline(lib_built, capsys):
    from split_vae_amd.augmentation import ReferenceAugmentator as Augmentator
    sizes = set()
    for seed in range(12):
        tr, te = Augmentator("mix_scramble", seed=seed, pipeline=0), Augmentator("mix_scramble", seed=seed, pipeline=1)
        assert tr.mix_size in (1, 2, 4, 8) and te.mix_size in (1, 2, 4, 8)
        assert tr.mix_size == Augmentator("mix_scramble", seed=seed, pipeline=0).mix_size         # reproducible for a seed
        sizes |= {tr.mix_size, te.mix_size}
    assert len(sizes) >= 3
    out = capsys.readouterr().out
    assert "Patch size:" in out and "Window: [1, " in out                                        # printed like augmentation.py:66-68


def test_cli_accepts_every_augmentation():
    from split_vae_amd import main, spair_main
    for t in ("scramble", "mix_scramble", "blur", "high_low_pass", "no_op"):
        assert main.build_parser().parse_args(["--augmentation", t]).augmentation == t
        assert spair_main.build_parser().parse_args(["--augmentation", t]).augmentation == t
    a = main.build_parser().parse_args(["--augmentation", "mix_scramble", "--mix_per_image"])
    assert a.mix_per_image and not main.build_parser().parse_args([]).mix_per_image
    assert spair_main.build_parser().parse_args(["--mix_per_image"]).mix_per_image
    assert "--mix_per_image" not in [f for f, _, _ in main.REFERENCE_OPTIONS]
    for model in ("lgvae", "lggmvae", "gmvae"):
        for t in ("scramble", "mix_scramble", "blur", "no_op"):
            main.check_augmentation(t, model)
    main.check_augmentation("high_low_pass", "gmvae")
    for model in ("lgvae", "lggmvae", "lg_spair"):
        with pytest.raises(SystemExit, match="high_low_pass"):
            main.check_augmentation("high_low_pass", model)
    with pytest.raises(SystemExit):
        main.check_augmentation("sharpen", "lgvae")


def test_train_and_test_pipelines_get_their_own_mix_scramble():
    from split_vae_amd import main
    from split_vae_amd.utils import dotdict
    cfg = dotdict(augmentation="mix_scramble", patch_size=1, seed=3, mix_per_image=True)
    tr, te = main.make_augmentors(cfg)
    assert tr is not te and (tr.pipeline, te.pipeline) == (0, 1) and tr.per_image and te.per_image
    cfg.augmentation = "scramble"
    tr, te = main.make_augmentors(cfg)
    assert tr is te                                         # one shared permutation stream, as before
