"""GPU: device-resident datasets -- sv_dataset_gather / sv_dataset_onehot / sv_dataset_gather_scramble against the host
pipeline they replace (data.normalise_u8, data.one_hot_svhn, ArrayDataset / StreamDataset) and against the two-kernel form
(sv_dataset_gather + sv_scramble_gather[_staged]).  Everything here is a copy or a table look-up: every comparison is bit for bit."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _u8_set(N, H, seed=0):
    """[N,H,H,3] uint8 holding every one of the 256 levels (image 0 carries them all)."""
    x = np.random.default_rng(seed).integers(0, 256, (N, H, H, 3), dtype=np.uint8)
    x[0].reshape(-1)[:256] = np.arange(256, dtype=np.uint8)
    return x


def _f32_set(N, H, seed=0):
    return (np.random.default_rng(seed).integers(0, 256, (N, H, H, 3)) / 255.0 * 2 - 1).astype(np.float32)


def _lut():
    import torch
    from split_vae_amd import data
    return torch.from_numpy(data.ResidentDataset.make_lut()).cuda()


def test_gather_uint8_is_the_host_normalisation(lib_built):
    import torch
    from split_vae_amd import data, ops
    src = _u8_set(37, 32)
    index = [36, 0, 17, 17, 3]                                   # both ends of the set and a duplicate
    assert len(np.unique(src[index])) == 256
    got = ops.dataset_gather(torch.from_numpy(src).cuda(), torch.tensor(index, dtype=torch.int32, device="cuda"), lut=_lut())
    assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy(), data.normalise_u8(src[index]))


def test_gather_fp32_copies(lib_built):
    import torch
    from split_vae_amd import ops
    src = _f32_set(9, 64)
    index = [8, 0, 4]
    got = ops.dataset_gather(torch.from_numpy(src).cuda(), torch.tensor(index, dtype=torch.int32, device="cuda"))
    assert np.array_equal(got.cpu().numpy(), src[index])


@pytest.mark.parametrize("H", [5, 6])
def test_gather_off_the_16_byte_grid(lib_built, H):
    """H = 5: 75 elements per image (no multiple of 4: the scalar loops, and an odd pixel count in the fused kernel); H = 6: 108
    elements (a multiple of 4, not of 16: 4-byte loads in the gather, byte staging in the fused kernel)."""
    import torch
    from split_vae_amd import data, ops
    rng = np.random.default_rng(H)
    index = torch.tensor([6, 0, 3], dtype=torch.int32, device="cuda")
    perm = torch.from_numpy(np.stack([rng.permutation(H * H) for _ in range(3)]).astype(np.int32)).cuda()
    for src in (rng.integers(0, 256, (7, H, H, 3), dtype=np.uint8), _f32_set(7, H)):
        lut = _lut() if src.dtype == np.uint8 else None
        dev = torch.from_numpy(src).cuda()
        x = ops.dataset_gather(dev, index, lut=lut)
        want = data.normalise_u8(src[[6, 0, 3]]) if src.dtype == np.uint8 else src[[6, 0, 3]]
        assert np.array_equal(x.cpu().numpy(), want)
        x8, xh8 = (torch.full((3, H, H, 8), 7.0, device="cuda") for _ in range(2))
        w8, wh8 = (torch.full((3, H, H, 8), 9.0, device="cuda") for _ in range(2))
        got = ops.dataset_gather_scramble(dev, index, perm, 1, lut=lut, staged=(x8, xh8))
        assert torch.equal(got, ops.scramble_gather(x, perm, 1, staged=(w8, wh8))) and torch.equal(x8, w8) and torch.equal(xh8, wh8)


def test_gather_beyond_2_31_bytes(lib_built):
    """Row 700 000 of a 32 x 32 uint8 set starts 2.15e9 bytes into the source: the row offset must be 64-bit arithmetic."""
    import torch
    from split_vae_amd import data, ops
    N = 700001
    src = torch.zeros((N, 32, 32, 3), dtype=torch.uint8, device="cuda")
    last = _u8_set(1, 32, seed=4)
    src[N - 1] = torch.from_numpy(last[0]).cuda()
    index = torch.tensor([N - 1, 0], dtype=torch.int32, device="cuda")
    perm = torch.from_numpy(np.stack([np.random.default_rng(b).permutation(64) for b in range(2)]).astype(np.int32)).cuda()
    lut = _lut()
    x = ops.dataset_gather(src, index, lut=lut)
    want = data.normalise_u8(np.concatenate([last, np.zeros_like(last)]))
    assert np.array_equal(x.cpu().numpy(), want)
    assert torch.equal(ops.dataset_gather_scramble(src, index, perm, 4, lut=lut), ops.scramble_gather(x, perm, 4))


def test_an_index_outside_the_set_is_clamped_not_followed(lib_built):
    """The host layer refuses such an index; the kernels clamp it all the same, so a stray one cannot read outside the set."""
    import torch
    from split_vae_amd import data, ops
    src = _u8_set(5, 32)
    index = torch.tensor([-3, 5, 1 << 30], dtype=torch.int32, device="cuda")
    got = ops.dataset_gather(torch.from_numpy(src).cuda(), index, lut=_lut())
    assert np.array_equal(got.cpu().numpy(), data.normalise_u8(src[[0, 4, 4]]))
    y = ops.dataset_onehot(torch.tensor([1, 2, 3, 4, 5], dtype=torch.uint8, device="cuda"), index, 10)
    assert y.argmax(1).tolist() == [0, 4, 4]


def test_onehot_follows_one_hot_svhn(lib_built):
    import torch
    from split_vae_amd import data, ops
    labels = np.array([1, 10, 5, 0, 11], np.uint8)               # 10 = digit 0 -> last index; 0 and 11 -> all-zero rows
    index = [4, 1, 3, 0, 2, 1]
    got = ops.dataset_onehot(torch.from_numpy(labels).cuda(), torch.tensor(index, dtype=torch.int32, device="cuda"), 10)
    want = data.one_hot_svhn(labels[index])
    assert want.sum(1).tolist() == [0, 1, 0, 1, 1, 1] and want[1, 9] == 1
    assert np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("kind,H,patch", [("u8", 32, 1), ("u8", 32, 4), ("u8", 32, 32), ("f32", 64, 8)])
def test_fused_scramble_equals_gather_then_scramble(lib_built, kind, H, patch, dtype):
    """images6, x8, xh8 of the fused kernel = sv_dataset_gather followed by sv_scramble_gather_staged on the same perm, and with
    x8 = xh8 = NULL images6 = sv_dataset_gather followed by sv_scramble_gather."""
    import torch
    from split_vae_amd import ops
    B, N = 4, 11
    tdt = torch.float32 if dtype == "f32" else torch.bfloat16
    src = torch.from_numpy(_u8_set(N, H) if kind == "u8" else _f32_set(N, H)).cuda()
    lut = _lut() if kind == "u8" else None
    rng = np.random.default_rng(patch)
    index = torch.tensor([10, 0, 6, 6], dtype=torch.int32, device="cuda")
    perm = torch.from_numpy(np.stack([rng.permutation((H // patch) ** 2) for _ in range(B)]).astype(np.int32)).cuda()
    x = ops.dataset_gather(src, index, lut=lut)
    want8, wanth8 = (torch.full((B, H, H, 8), 7.0, dtype=tdt, device="cuda") for _ in range(2))
    want = ops.scramble_gather(x, perm, patch, staged=(want8, wanth8))
    x8, xh8 = (torch.full((B, H, H, 8), 9.0, dtype=tdt, device="cuda") for _ in range(2))
    got = ops.dataset_gather_scramble(src, index, perm, patch, lut=lut, staged=(x8, xh8))
    assert torch.equal(got, want) and torch.equal(x8, want8) and torch.equal(xh8, wanth8)
    assert torch.equal(got[..., :3], x) and not (patch < H and torch.equal(got[..., 3:], x))
    plain = ops.dataset_gather_scramble(src, index, perm, patch, lut=lut)
    assert torch.equal(plain, ops.scramble_gather(x, perm, patch))


def _batches_equal(a, b):
    import torch
    if isinstance(a, tuple):
        return isinstance(b, tuple) and len(a) == len(b) and all(torch.equal(p, q) for p, q in zip(a, b))
    return torch.equal(a, b)


@pytest.mark.parametrize("labelled", [False, True], ids=["images", "labelled"])
@pytest.mark.parametrize("buffer", [8, 64])
def test_resident_dataset_yields_array_datasets_batches(lib_built, buffer, labelled):
    """N = 23, B = 4: repeat=False gives 4, 4, 4, 4, 4, 3; repeat=True for 13 batches crosses two epoch boundaries.  chunk_batches=2:
    the index upload is cut mid-epoch too."""
    from split_vae_amd import data
    N, B = 23, 4
    src = _u8_set(N, 32, seed=1)
    labels = np.random.default_rng(2).integers(0, 12, N).astype(np.uint8)
    y = data.one_hot_svhn(labels) if labelled else None
    for repeat, n_batches in ((False, 6), (True, 13)):
        host = data.ArrayDataset(data.normalise_u8(src), B, repeat, 5, "cuda", y=y, buffer_size=buffer)
        res = data.ResidentDataset(src, B, repeat, 5, "cuda", labels=labels if labelled else None, buffer_size=buffer, chunk_batches=2)
        assert res.labelled == host.labelled == labelled
        hb, rb = [], []
        for (h, r), _ in zip(zip(host, res), range(n_batches + 1)):
            hb.append(h)
            rb.append(r)
        assert len(hb) == len(rb) == (n_batches if not repeat else n_batches + 1)
        sizes = [(b[0] if labelled else b).shape[0] for b in rb]
        assert sizes == ([4, 4, 4, 4, 4, 3] if not repeat else [4] * (n_batches + 1))
        assert all(_batches_equal(h, r) for h, r in zip(hb, rb))
        if not repeat:
            assert len(list(res)) == len(list(host)) == 6                      # both end after the remainder


@pytest.mark.parametrize("buffer", [3, 64])
def test_resident_dataset_yields_stream_datasets_batches(lib_built, tmp_path, buffer):
    import torch
    from split_vae_amd import data, tfrecord as tfr
    imgs = _f32_set(7, 64, seed=3)
    path = str(tmp_path / "train_64x64.tfrec")
    tfr.write_celeba_tfrec(path, imgs)
    arr = tfr.read_celeba_tfrec_array(path, 64)
    assert np.array_equal(arr, imgs)
    for repeat, n_batches in ((False, 3), (True, 9)):
        host = data.StreamDataset(lambda: tfr.read_celeba_tfrec(path, 64), 3, repeat, buffer, 2, "cuda")
        res = data.ResidentDataset(arr, 3, repeat, 2, "cuda", buffer_size=buffer, stream_seeding=True)
        pairs = [p for p, _ in zip(zip(host, res), range(n_batches))]
        assert len(pairs) == n_batches and all(torch.equal(h, r) for h, r in pairs)
        if not repeat:
            assert [b.shape[0] for b in res] == [3, 3, 1]


def test_resident_dataset_that_does_not_fit_raises(lib_built, monkeypatch):
    import torch
    from split_vae_amd import data
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (1000, 2000))
    with pytest.raises(RuntimeError, match="3072"):
        data.ResidentDataset(_u8_set(2, 32), 2, False, device="cuda")


def test_step_equivalence_with_the_host_pipeline(lib_built, deterministic):
    """LGVae on SVHN-32, B = 4, fp32, three steps: ArrayDataset + Augmentator.scramble(plan=) against ResidentDataset +
    scramble_from(plan=), same seeds -> the losses after each step and the weights at the end are bit-equal, and both took the
    staged fast path (plan.in8_gen advanced once per batch, by the staging, not again by a split / pad pass)."""
    import torch
    from split_vae_amd import data, trainer
    from split_vae_amd.augmentation import Augmentator
    from split_vae_amd.model import LGVae
    from split_vae_amd.optimizer import Adam
    B, H, N = 4, 32, 23
    src = _u8_set(N, H, seed=6)
    runs = []
    for resident in (False, True):
        m = LGVae(128, 128, image_shape=[-1, H, H, 3], dtype="f32", device=torch.device("cuda"), seed=3)
        plan, opt, aug = m.plan(B), Adam(learning_rate=1e-4), Augmentator("scramble", size=4, seed=1)
        if resident:
            ds = data.ResidentDataset(src, B, True, 7, "cuda", buffer_size=8)
            batches = (aug.scramble_from(ds, i, plan=plan) for i in ds.index_batches())
        else:
            batches = (aug.scramble(x, plan=plan) for x in data.ArrayDataset(data.normalise_u8(src), B, True, 7, "cuda", buffer_size=8))
        losses, images = [], []
        for _, img in zip(range(3), batches):
            gen = plan.in8_gen
            assert img._sv_staged_plan is plan and img._sv_staged_gen == gen
            trainer.train_step(m, img, opt)
            torch.cuda.synchronize()
            assert plan.in8_gen == gen and img._sv_staged_plan is None     # consumed as staged: no split / pad pass bumped the generation
            losses.append(trainer.last_losses(plan))
            images.append(img.clone())
        assert plan.in8_gen == 3 and aug._step == 3
        runs.append((losses, images, m.flat.clone()))
    (l0, i0, w0), (l1, i1, w1) = runs
    assert all(torch.equal(a, b) for a, b in zip(i0, i1))
    assert l0 == l1, (l0, l1)
    assert torch.equal(w0, w1)


def test_a_batch_off_the_plans_size_is_not_staged(lib_built):
    """The last test batch: a batch whose size differs from the plan's takes the unstaged form, as with scramble(plan=)."""
    import torch
    from split_vae_amd import data
    from split_vae_amd.augmentation import Augmentator
    from split_vae_amd.model import LGVae
    src = _u8_set(9, 32)
    ds = data.ResidentDataset(src, 4, False, 0, "cuda")
    m = LGVae(128, 128, image_shape=[-1, 32, 32, 3], dtype="f32", device=torch.device("cuda"), seed=3)
    plan = m.plan(4)
    a, b = Augmentator("scramble", size=4, seed=2), Augmentator("scramble", size=4, seed=2)
    out = a.scramble_from(ds, [8, 1, 2], plan=plan)
    assert getattr(out, "_sv_staged_plan", None) is None and plan.in8_gen == 0
    assert torch.equal(out, b.scramble(torch.from_numpy(data.normalise_u8(src[[8, 1, 2]])).cuda()))
    with pytest.raises(ValueError):
        a.scramble_from(ds, [9, 0, 1])


@pytest.mark.parametrize("kind", ["mix_scramble", "blur", "no_op"])
def test_augment_from_serves_the_other_augmentations(lib_built, kind):
    import torch
    from split_vae_amd import data
    from split_vae_amd.augmentation import ReferenceAugmentator
    src = _u8_set(9, 32)
    ds = data.ResidentDataset(src, 4, False, 0, "cuda")
    a, b = ReferenceAugmentator(kind, size=4, seed=2), ReferenceAugmentator(kind, size=4, seed=2)
    x = torch.from_numpy(data.normalise_u8(src[[8, 1, 2, 2]])).cuda()
    for _ in range(2):                                          # twice: the draws advance alike
        assert torch.equal(a.augment_from(ds, [8, 1, 2, 2]), b.augment(x))
    assert a._step == b._step


def _write_svhn(root, n_train, n_extra, n_test, seed=0):
    import scipy.io
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, "SVHN"), exist_ok=True)
    for name, n in (("train", n_train), ("extra", n_extra), ("test", n_test)):
        X = rng.integers(0, 256, (32, 32, 3, n), dtype=np.uint8)
        X[:16, :16, 0, 0] = np.arange(256, dtype=np.uint8).reshape(16, 16)
        y = rng.integers(1, 11, (n, 1)).astype(np.uint8)
        scipy.io.savemat(os.path.join(root, "SVHN", name + "_32x32.mat"), {"X": X, "y": y})


def _loss_lines(out):
    keep = ("Training step", "Recon Loss", "Total KL", "Training done")
    return [l for l in out.splitlines() if any(k in l for k in keep)]


def _saved_arrays(path):
    from split_vae_amd import h5io
    if path.endswith(".npz"):
        z = np.load(path)
        return [z[k] for k in sorted(z.files)]
    return [a for _, ws in h5io.load_keras_weights(path) for _, a in ws]


CLI_ARGS = ["--beta", "40", "--patch_size", "1", "--batch_size", "12", "--training_steps", "3", "--log_every", "2", "--dtype", "f32"]


def test_cli_with_resident_data_trains_the_same_run(lib_built, deterministic, tmp_path, monkeypatch, capsys):
    """main() on tiny .mat files with and without --resident_data, fixed-order reductions (what SV_DETERMINISTIC=1 selects): the
    printed loss lines and the saved weights are identical."""
    from split_vae_amd import main as svmain
    _write_svhn(str(tmp_path / "data"), n_train=30, n_extra=9, n_test=27)
    monkeypatch.chdir(tmp_path)
    runs = []
    for i, flags in enumerate((["-no_label"], ["-no_label", "--resident_data"])):
        path = svmain.main(CLI_ARGS + flags)
        out = capsys.readouterr().out
        assert "Training step 0" in out and "Training step 2" in out and "Training done!" in out
        keep = str(tmp_path / ("run%d" % i)) + os.path.splitext(path)[1]
        os.replace(path, keep)                                  # (run names carry a timestamp of one-second resolution)
        runs.append((_loss_lines(out), _saved_arrays(keep)))
    assert len(runs[0][0]) >= 12 and runs[0][0] == runs[1][0]
    assert len(runs[0][1]) == len(runs[1][1]) == 40 and all(np.array_equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))


def test_cli_with_resident_data_and_labels(lib_built, tmp_path, monkeypatch, capsys):
    """The labelled form with the flag: (images, one-hot labels) tuples from the device, and the classifier note as without it."""
    from split_vae_amd import main as svmain
    _write_svhn(str(tmp_path / "data"), n_train=30, n_extra=9, n_test=27)
    monkeypatch.chdir(tmp_path)
    path = svmain.main(CLI_ARGS + ["--resident_data"])
    out = capsys.readouterr().out
    assert "classifier-based test metrics are not available" in out and "Training done!" in out and os.path.exists(path)
