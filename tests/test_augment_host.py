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
