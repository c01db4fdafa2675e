"""MI355X: the blur / high-low-pass / mixed-scramble augmentations (split_vae_amd/csrc/augment.hip) against the fp64 oracle
(tests/augment_ref.py), their staged outputs, their Philox draws, train steps on their batches, and the CLIs that select them."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_ref as ar  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ops(lib_built):
    assert torch.cuda.is_available()
    from split_vae_amd import ops as o
    from split_vae_amd import torch_ops  # noqa: F401  (registers the split_vae:: operators)
    return o


def _images(B, H, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return (rng.integers(0, 256, size=(B, H, H, 3)) / 255.0 * 2 - 1).astype(np.float32)


# ---------------------------------------------------------------- Gaussian filter
@pytest.mark.parametrize("H", [32, 64])
def test_blur_matches_the_fp64_oracle(ops, H):
    from split_vae_amd.augmentation import ReferenceAugmentator as Augmentator
    B = 8
    x = _images(B, H, 1)
    radius = np.array([3, 4, 5, 6, 6, 5, 4, 3], np.int32)            # every radius the reference draws
    std = np.array([5.0, 6.5, 9.99, 7.25, 5.0, 8.0, 9.5, 6.0], np.float32)
    got = Augmentator("blur", seed=0).augment(torch.from_numpy(x).cuda(), radius=torch.from_numpy(radius), std=torch.from_numpy(std))
    got = got.cpu().numpy()
    want = ar.gaussian_blur_batch(x.astype(np.float64), radius, std.astype(np.float64))
    assert got.shape == (B, H, H, 6) and got.dtype == np.float32
    assert np.array_equal(got[..., :3], x)
    assert np.abs(got - want).max() <= 1e-5
    # the same call twice: bit-identical (one summation order)
    again = torch.ops.split_vae.gauss_blur(torch.from_numpy(x).cuda(), torch.from_numpy(radius).cuda(), torch.from_numpy(std).cuda())
    assert np.array_equal(again.cpu().numpy(), got)


@pytest.mark.parametrize("size", [0, 1, 4, 8])
@pytest.mark.parametrize("mean", [0.0, 0.5])
def test_high_low_pass_matches_the_fp64_oracle(ops, size, mean):
    from split_vae_amd.augmentation import ReferenceAugmentator as Augmentator
    B, H = 4, 32
    x = _images(B, H, 2 + size)
    got = Augmentator("high_low_pass", size=size, mean=mean).augment(torch.from_numpy(x).cuda()).cpu().numpy()
    want = ar.high_low_pass_batch(x.astype(np.float64), size, mean, 1.0)
    assert got.shape == (B, H, H, 9)
    assert np.abs(got - want).max() <= 1e-5
    assert np.array_equal(got[..., :3], x)
    assert np.array_equal(got[..., 3:6], got[..., :3] - got[..., 6:9])          # x - low in fp32, bit for bit
    if size == 0:
        assert np.array_equal(got[..., 6:9], x)                                     # a one-tap kernel of weight 1


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("kind", ["blur", "high_low_pass", "mix"])
def test_staged_outputs_are_the_images_cast_and_zero_padded(ops, dtype, kind):
    B, H = 6, 32
    x = torch.from_numpy(_images(B, H, 5)).cuda()
    x8 = torch.full((B, H, H, 8), 7.0, dtype=dtype, device="cuda")
    xh8 = torch.full((B, H, H, 8), 7.0, dtype=dtype, device="cuda")
    if kind == "blur":
        r, s = ops.blur_params(B, seed=3)
        plain, staged = ops.gauss_blur(x, r, s), ops.gauss_blur(x, r, s, staged=(x8, xh8))
        lo, hi = plain[..., :3], plain[..., 3:6]
    elif kind == "high_low_pass":
        plain, staged = ops.high_low_pass(x, 4, 0.5, 1.0), ops.high_low_pass(x, 4, 0.5, 1.0, staged=(x8, xh8))
        lo, hi = plain[..., :3], plain[..., 3:6]
    else:
        sizes = ops.mix_sizes(B, seed=3)
        perm = ops.random_perm_mixed(sizes, H, seed=3)
        plain, staged = ops.scramble_gather_mixed(x, perm, sizes), ops.scramble_gather_mixed(x, perm, sizes, staged=(x8, xh8))
        lo, hi = plain[..., :3], plain[..., 3:6]
    torch.cuda.synchronize()
    assert torch.equal(plain, staged)
    assert torch.equal(x8[..., :3], lo.to(dtype)) and torch.equal(xh8[..., :3], hi.to(dtype))
    assert not x8[..., 3:].any() and not xh8[..., 3:].any()


# ---------------------------------------------------------------- mixed scramble
def test_mixed_gather_and_permutation_rows(ops):
    from split_vae_amd.augmentation import ReferenceAugmentator as Augmentator
    B, H = 8, 32
    x = _images(B, H, 6)
    sizes = torch.tensor([1, 2, 4, 8, 8, 4, 2, 1], dtype=torch.int32)
    aug = Augmentator("mix_scramble", seed=5, per_image=True)
    got = aug.augment(torch.from_numpy(x).cuda(), sizes=sizes).cpu().numpy()
    perm = ops.random_perm_mixed(sizes.cuda(), H, seed=5, step=0).cpu().numpy()      # the stream the call above drew from
    for b in range(B):
        n = (H // int(sizes[b])) ** 2
        assert sorted(perm[b, :n].tolist()) == list(range(n)), b                     # a permutation of that image's patches
        assert (perm[b, n:] == -1).all()
    assert np.array_equal(got, ar.mix_scramble_batch(x, perm, sizes.numpy()).astype(np.float32))
    # a row of one size is the sv_random_perm row of that size (same Philox keys)
    one = ops.random_perm_mixed(torch.full((4,), 4, dtype=torch.int32, device="cuda"), H, seed=9, step=2, sample_offset=3)
    assert torch.equal(one[:, :64], ops.random_perm(4, 64, 9, 2, 3))
    # explicit perm, drawn sizes
    sz = ops.mix_sizes(B, seed=1)
    p = ops.random_perm_mixed(sz, H, seed=2)
    got = torch.ops.split_vae.scramble_gather_mixed(torch.from_numpy(x).cuda(), p, sz).cpu().numpy()
    assert np.array_equal(got, ar.mix_scramble_batch(x, p.cpu().numpy(), sz.cpu().numpy()).astype(np.float32))


def test_faithful_mix_scramble_is_scramble_with_the_pipeline_size(ops):
    from split_vae_amd.augmentation import ReferenceAugmentator as Augmentator
    B, H = 4, 32
    x = torch.from_numpy(_images(B, H, 7)).cuda()
    m = Augmentator("mix_scramble", seed=4, pipeline=1)
    s = m.mix_size
    got = m.augment(x)
    want = Augmentator("scramble", size=s, seed=4).augment(x)
    assert torch.equal(got, want)


# ---------------------------------------------------------------- draws
def test_draws_are_uniform_reproducible_and_shardable(ops):
    n = 8192
    r, s = ops.blur_params(n, seed=11, step=3)
    r, s = r.cpu().numpy(), s.cpu().numpy()
    assert set(r.tolist()) == {3, 4, 5, 6}
    counts = np.bincount(r - 3, minlength=4)
    assert counts.min() > 0.2 * n and counts.max() < 0.3 * n, counts
    assert s.min() >= 5.0 and s.max() < 10.0 and 7.3 < s.mean() < 7.7
    assert np.histogram(s, bins=5, range=(5, 10))[0].min() > 0.15 * n
    r2, s2 = ops.blur_params(n, seed=11, step=3)
    assert np.array_equal(r, r2.cpu().numpy()) and np.array_equal(s, s2.cpu().numpy())
    r3, _ = ops.blur_params(n, seed=11, step=4)
    assert not np.array_equal(r, r3.cpu().numpy())
    rs, ss = ops.blur_params(100, seed=11, step=3, sample_offset=1000)              # a data-parallel shard
    assert np.array_equal(rs.cpu().numpy(), r[1000:1100]) and np.array_equal(ss.cpu().numpy(), s[1000:1100])
    z = ops.mix_sizes(n, seed=11, step=3).cpu().numpy()
    assert set(z.tolist()) == {1, 2, 4, 8}
    c = np.bincount(np.log2(z).astype(int), minlength=4)
    assert c.min() > 0.2 * n and c.max() < 0.3 * n, c
    assert np.array_equal(ops.mix_sizes(64, seed=11, step=3, sample_offset=500).cpu().numpy(), z[500:564])
    assert [ops.mix_size_host(11, 3, i) for i in range(16)] == z[:16].tolist()      # host and device draw the same
    sizes = torch.from_numpy(z[:32]).cuda()
    full = ops.random_perm_mixed(sizes, 32, seed=11, step=3)
    shard = ops.random_perm_mixed(sizes[8:16].contiguous(), 32, seed=11, step=3, sample_offset=8)
    assert torch.equal(full[8:16], shard)


def test_augmentator_draws_follow_the_global_sample_index(ops):
    from split_vae_amd.augmentation import ReferenceAugmentator as Augmentator
    B, H = 8, 32
    x = torch.from_numpy(_images(B, H, 8)).cuda()
    for t, kw in (("blur", {}), ("mix_scramble", {"per_image": True})):
        full = Augmentator(t, seed=2, **kw).augment(x)
        half = Augmentator(t, seed=2, **kw).augment(x[4:].contiguous(), sample_offset=4)
        assert torch.equal(full[4:], half), t


# ---------------------------------------------------------------- train steps
def _staged_vs_plain(make_model, step, aug_kw, B=16, H=32, steps=2, with_xh=True):
    from split_vae_amd import data
    from split_vae_amd.augmentation import ReferenceAugmentator as Augmentator
    from split_vae_amd.optimizer import Adam
    x = data.synthetic_images(B, H, H, seed=0, device="cuda")
    res = []
    for staged in (False, True):
        model = make_model()
        opt = Adam(learning_rate=1e-3)
        aug = Augmentator(seed=1, **aug_kw)
        out = []
        for _ in range(steps):
            img = aug.augment(x, plan=model.plan(B) if staged else None)
            assert (getattr(img, "_sv_staged_plan", None) is not None) == staged
            out.append(step(model, img, opt))
        torch.cuda.synchronize()
        res.append((np.stack(out), [t.detach().cpu().numpy() for t in model.trainable_variables]))
    (l0, p0), (l1, p1) = res
    assert np.array_equal(l0, l1)
    for a, b in zip(p0, p1):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("aug_kw", [dict(type="blur"), dict(type="mix_scramble", per_image=True)])
def test_lgvae_step_on_staged_batches_is_bit_identical(ops, deterministic, aug_kw):
    from split_vae_amd import trainer
    from split_vae_amd.model import LGVae

    def step(m, img, opt):
        plan = trainer.train_step(m, img, opt)
        return np.array([v for v in trainer.last_losses(plan).values()])
    _staged_vs_plain(lambda: LGVae(128, 128, image_shape=[-1, 32, 32, 3], dtype="f32", device=torch.device("cuda"), seed=3), step, aug_kw)


def test_lggmvae_step_on_staged_blur_is_bit_identical(ops, deterministic):
    from split_vae_amd import gm

    def make():
        m = gm.LGGMVae(128, 128, [-1, 32, 32, 3], 10, 0.4, dtype="f32", device="cuda", seed=4)
        m.beta, m.alpha = 40.0, 40.0
        return m
    from split_vae_amd import data
    from split_vae_amd.augmentation import ReferenceAugmentator as Augmentator
    from split_vae_amd.optimizer import Adam
    B, H = 16, 32
    x = data.synthetic_images(B, H, H, seed=0, device="cuda")
    r, s = ops.blur_params(B, seed=7)
    res = []
    for staged in (False, True):
        m = make()
        opt = Adam(learning_rate=1e-3)
        img = Augmentator("blur").augment(x, radius=r, std=s, plan=m.plan(B) if staged else None)
        assert (getattr(img, "_sv_staged_plan", None) is not None) == staged
        met = gm.train_step_lg_gm_vae(m, img, opt).cpu().numpy().astype(np.float64)
        torch.cuda.synchronize()
        res.append((met, m.flat.cpu().numpy().astype(np.float64), m.gm_flat.cpu().numpy().astype(np.float64)))
    # the staged step runs the two encoders on two streams (gm.py); with fixed-order reductions the order of the streams changes no bit
    for a, b in zip(res[0], res[1]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("aug_kw", [dict(type="blur"), dict(type="high_low_pass", size=2)])
def test_gmvae_step_on_staged_batches_is_bit_identical(ops, deterministic, aug_kw):
    from split_vae_amd.gmvae import GMVae, train_step_gm_vae

    def make():
        m = GMVae(128, [-1, 32, 32, 3], 10, 0.4, dtype="f32", device="cuda", seed=4)
        m.beta, m.alpha = 40.0, 40.0
        return m
    _staged_vs_plain(make, lambda m, img, opt: train_step_gm_vae(m, img, opt).cpu().numpy(), aug_kw)


def test_gmvae_high_low_pass_step_reads_only_channels_0_to_5(ops, deterministic):
    """GMVae reads x (channels 0-2) only: a 9-channel high_low_pass batch trains exactly like its first six channels."""
    from split_vae_amd import data
    from split_vae_amd.augmentation import ReferenceAugmentator as Augmentator
    from split_vae_amd.gmvae import GMVae, train_step_gm_vae
    from split_vae_amd.optimizer import Adam
    B, H = 8, 32
    img9 = Augmentator("high_low_pass", size=2).augment(data.synthetic_images(B, H, H, seed=0, device="cuda"))
    out = []
    for img in (img9, img9[..., :6].contiguous()):
        m = GMVae(128, [-1, H, H, 3], 10, 0.4, dtype="f32", device="cuda", seed=4)
        out.append((train_step_gm_vae(m, img, Adam(learning_rate=1e-3)).cpu().numpy(), m.flat.cpu().numpy()))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


def test_lgvae_step_on_a_blurred_batch_matches_the_oracle(ops, deterministic):
    """One fp32 LGVae step on a blurred batch against the fp64 oracle step on the oracle's blur of the same images: the loss
    terms at rtol 1e-4 and the updated weights within smoke()'s bound."""
    from oracle import torch_ref
    from split_vae_amd import trainer
    from split_vae_amd.augmentation import ReferenceAugmentator as Augmentator
    from split_vae_amd.model import LGVae
    from split_vae_amd.optimizer import Adam
    B, H, beta = 4, 32, 40.0
    x = _images(B, H, 9)
    radius, std = np.array([3, 4, 5, 6], np.int32), np.array([5.5, 9.0, 6.0, 7.5], np.float32)
    eps = np.random.Generator(np.random.PCG64(3)).standard_normal((2, B, 128)).astype(np.float32)
    want_img = ar.gaussian_blur_batch(x.astype(np.float64), radius, std.astype(np.float64))
    model = LGVae(128, 128, image_shape=[-1, H, H, 3], dtype="f32", seed=3)
    model.beta = beta
    images = Augmentator("blur").augment(torch.from_numpy(x).cuda(), radius=torch.from_numpy(radius), std=torch.from_numpy(std),
                                         plan=model.plan(B))
    ref = torch_ref.RefTrainer(model.get_weights(), beta, dtype=torch.float64)
    ref_losses, _ = ref.train_step(torch.from_numpy(want_img), eps[0], eps[1])
    plan = trainer.train_step(model, images, Adam(learning_rate=1e-4), eps=(torch.from_numpy(eps[0]).cuda(), torch.from_numpy(eps[1]).cuda()))
    torch.cuda.synchronize()
    got = trainer.last_losses(plan)
    for k, v in ref_losses.items():
        assert abs(got[k] - v) <= 1e-4 * abs(v) + 1e-5, (k, got[k], v)
    w_ref = torch.cat([p.detach().flatten() for p in ref.params])
    w_got = torch.cat([w.flatten() for w in model.trainable_variables]).cpu().double()
    assert float((w_ref - w_got).abs().max()) < 2.5e-4


# ---------------------------------------------------------------- CLIs
@pytest.mark.parametrize("args", [
    ["-m", "split_vae_amd.main", "--augmentation", "blur"],
    ["-m", "split_vae_amd.main", "--augmentation", "mix_scramble"],
    ["-m", "split_vae_amd.main", "--augmentation", "mix_scramble", "--mix_per_image"],
    ["-m", "split_vae_amd.main", "--model", "gmvae", "--augmentation", "high_low_pass", "--patch_size", "2"],
    ["-m", "split_vae_amd.spair_main", "--model", "lg_spair", "--augmentation", "blur", "--batch_size", "4", "--training_steps", "2",
     "--log_every", "1"],
], ids=["blur", "mix", "mix_per_image", "gmvae_hlp", "lg_spair_blur"])
def test_cli_runs_a_few_steps(lib_built, tmp_path, args):
    if args[1] == "split_vae_amd.main":
        args = args + ["--synthetic", "-no_label", "--batch_size", "8", "--training_steps", "2", "--log_every", "1"]
    else:
        args = args + ["--synthetic"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable] + args, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    if "mix_scramble" in args and "--mix_per_image" not in args:
        assert r.stdout.count("Patch size:") == 2                    # one draw for the train pipeline, one for the test pipeline


def test_cli_refuses_high_low_pass_for_the_split_models(lib_built, tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "split_vae_amd.main", "--augmentation", "high_low_pass", "--synthetic"], cwd=str(tmp_path),
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "high_low_pass" in r.stderr
