"""MI355X: the Multi-Bird layout and canvas kernels (split_vae_amd/csrc/multibird.hip) against the host mirror and the NumPy
restatement of create_sample (tests/multibird_ref.py), their keying, and spair_main on --dataset."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multibird_ref as mr  # noqa: E402

pytestmark = pytest.mark.gpu
BGS = ("solid_fixed", "unseen_solid_fixed", "ckb_rot_6", "unseen_ckb_rot_6")
SEED = 11


@pytest.fixture(scope="module")
def env(lib_built):
    assert torch.cuda.is_available()
    from split_vae_amd import multibird as mb
    from split_vae_amd import ops
    bank = mb.procedural_bank(200, seed=4)
    return mb, ops, bank, torch.from_numpy(bank).cuda()


def _owner(L, bank):
    """[48,48]: the object whose mask is on top at each pixel, -1 for background (from the layout and the bank alone)."""
    owner = np.full((48, 48), -1)
    for k in range(L["count"]):
        r, c = L["row"][k], L["col"][k]
        owner[r:r + 14, c:c + 14][bank[L["sprite"][k]].max(-1) > 0] = k
    return owner


@pytest.mark.parametrize("bg", BGS)
def test_device_layouts_equal_the_host_mirror(env, bg):
    mb, ops, bank, dbank = env
    n = 1000
    got = mb.layouts_to_numpy(ops.multibird_layouts(n, mb.BACKGROUNDS[bg], bank.shape[0], SEED, 2, sample_offset=5))
    want = mb.layouts_host(mb.BACKGROUNDS[bg], bank.shape[0], SEED, 2, 5 + np.arange(n))
    assert got.tobytes() == want.tobytes()                          # bit for bit, the fp32 angle included
    assert want["count"].max() == 5 and want["max_tries"].max() > 64     # several wave rounds were needed somewhere


@pytest.mark.parametrize("bg", BGS)
def test_canvases_match_the_reference_restatement(env, bg):
    """Layouts pinned.  Solid backgrounds: exactly equal (every value is np.float32(v / 255.0)).  Rotated checkerboard: atol 1e-4, the
    project's fp32 bar and what the arithmetic gives (source coordinates are sums of three fp32 products of magnitude <= 192, about
    5e-5 absolute; the bilinear surface has slope <= 0.68 per pixel per axis); sprite pixels are exact there too."""
    mb, ops, bank, dbank = env
    n = 1000
    L = mb.layouts_host(mb.BACKGROUNDS[bg], bank.shape[0], SEED, 1, np.arange(n))
    x, count = ops.multibird_canvases(dbank, mb.BACKGROUNDS[bg], n, SEED, 1, layouts=mb.layouts_to_tensor(L))
    x, count = x.cpu().numpy(), count.cpu().numpy()
    want, wcount = mr.create_dataset(L, bank, bg)
    assert np.array_equal(count, wcount) and np.array_equal(count, L["count"].astype(np.float32))
    diff = np.abs(x.astype(np.float64) - want.astype(np.float64))
    print("multibird %s: largest difference to the restatement %.3e" % (bg, diff.max()))
    if "rot" not in bg:
        assert np.array_equal(x, want)
        return
    assert diff.max() <= 1e-4
    sprite_px = np.stack([_owner(L[i], bank) >= 0 for i in range(n)])
    assert sprite_px.sum() > 10000 and np.array_equal(x[sprite_px], want[sprite_px])


@pytest.mark.parametrize("bg", ("solid_fixed", "ckb_rot_6"))
def test_keying_and_forms(env, bg):
    mb, ops, bank, dbank = env
    b, ns = mb.BACKGROUNDS[bg], bank.shape[0]
    x, c = ops.multibird_canvases(dbank, b, 64, SEED, 0, sample_offset=100)
    lay = ops.multibird_layouts(64, b, ns, SEED, 0, sample_offset=100)
    xp, cp = ops.multibird_canvases(dbank, b, 64, SEED, 0, layouts=lay)
    assert torch.equal(x, xp) and torch.equal(c, cp)                           # unpinned = layouts, then pinned
    idx = (100 + torch.arange(64)).cuda()
    xi, ci = ops.multibird_canvases(dbank, b, 64, SEED, 0, index=idx, sample_offset=7)
    assert torch.equal(x, xi) and torch.equal(c, ci)                           # index = offset + arange
    assert torch.equal(ops.multibird_layouts(64, b, ns, SEED, 0, index=idx), lay)
    lo, hi = ops.multibird_canvases(dbank, b, 32, SEED, 0, sample_offset=100), ops.multibird_canvases(dbank, b, 32, SEED, 0, sample_offset=132)
    assert torch.equal(x[:32], lo[0]) and torch.equal(x[32:], hi[0]) and torch.equal(c, torch.cat([lo[1], hi[1]]))
    x2, c2 = ops.multibird_canvases(dbank, b, 64, SEED, 0, sample_offset=100)
    assert torch.equal(x, x2) and torch.equal(c, c2)                           # the same launch twice
    perm = torch.randperm(64, generator=torch.Generator().manual_seed(0)).cuda()
    xs, _ = ops.multibird_canvases(dbank, b, 64, SEED, 0, index=idx[perm])
    assert torch.equal(xs, x[perm])                                            # shuffled indices gather the same canvases
    for other in (dict(seed=SEED + 1, split=0), dict(seed=SEED, split=1)):
        xo, _ = ops.multibird_canvases(dbank, b, 64, other["seed"], other["split"], sample_offset=100)
        assert not torch.equal(xo, x)
    assert float(x.min()) >= 0.0 and float(x.max()) <= 1.0


def test_nothing_outside_the_outputs_is_written(env):
    mb, ops, bank, dbank = env
    B = 9
    xbuf = torch.full((B + 2, 48, 48, 3), -7.0, device="cuda")
    cbuf = torch.full((B + 8,), -7.0, device="cuda")
    ops.multibird_canvases(dbank, mb.BACKGROUNDS["ckb_rot_6"], B, SEED, 0, x=xbuf[1:B + 1], count=cbuf[4:B + 4])
    torch.cuda.synchronize()
    assert (xbuf[0] == -7).all() and (xbuf[B + 1] == -7).all() and (cbuf[:4] == -7).all() and (cbuf[B + 4:] == -7).all()
    assert (xbuf[1:B + 1] >= 0).all() and (cbuf[4:B + 4] >= 0).all()
    import ctypes as C
    from split_vae_amd import _lib
    lib = _lib.load()
    assert lib.sv_multibird_canvases(C.c_void_p(xbuf.data_ptr()), None, C.c_void_p(dbank.data_ptr()), bank.shape[0], None, None, 0, 1, 0, 0, 0,
                                     None) == 0                                # count NULL is allowed


@pytest.mark.parametrize("bg", ("solid_fixed", "ckb_rot_6"))
def test_visible_sprite_pixels_carry_the_sprite(env, bg):
    """From the layouts and the bank alone: count[b] is the layout's count and every mask pixel of a placed sprite that no later
    sprite's mask covers holds that sprite's value."""
    mb, ops, bank, dbank = env
    n = 256
    x, count = ops.multibird_canvases(dbank, mb.BACKGROUNDS[bg], n, SEED, 0)
    L = mb.layouts_to_numpy(ops.multibird_layouts(n, mb.BACKGROUNDS[bg], bank.shape[0], SEED, 0))
    x = x.cpu().numpy()
    assert np.array_equal(count.cpu().numpy(), L["count"].astype(np.float32))
    checked = 0
    for i in range(n):
        owner = _owner(L[i], bank)
        for k in range(L["count"][i]):
            r, c = L["row"][i][k], L["col"][i][k]
            vis = owner[r:r + 14, c:c + 14] == k
            assert np.array_equal(x[i, r:r + 14, c:c + 14][vis], np.float32(bank[L["sprite"][i][k]][vis] / 255.0))
            checked += int(vis.sum())
    assert checked > 10000


HARD = ("--model lg_spair --z_bg_beta 1 --patch_size 8 --latent_size 64 --bg_latent_size 64 --local_latent_size 64 -split_z_l "
        "--z_what_beta 0.5 -concat_z_what -dense_local -dense_bg")            # README.md:107 of the reference (Multi-Bird-Hard)


@pytest.mark.parametrize("argv", [HARD + " --dataset cub_ckb_rot_6", "--model spair --dataset cub_solid_fixed"], ids=["hard", "spair_solid"])
def test_cli_trains_on_the_dataset(env, argv, capsys, tmp_path, monkeypatch):
    """spair_main without --synthetic: 40 steps, logs (and both test sets) at steps 0 and 40.  `total` is the sum of the logged train terms."""
    from split_vae_amd import spair_main
    monkeypatch.chdir(tmp_path)
    hist = spair_main.main(argv.split() + ["--training_steps", "40", "--log_every", "40"])
    out = capsys.readouterr().out
    assert "Count accuracy0" in out and "Count accuracy1" in out and "Training done!" in out
    assert [h["step"] for h in hist] == [0, 40]
    for h in hist:
        assert 0.0 <= h["count_acc0"] <= 1.0 and 0.0 <= h["count_acc1"] <= 1.0
        assert all(np.isfinite(v) for v in h["train"].values())
        assert all(np.isfinite(v) for v in h["test0"].values()) and all(np.isfinite(v) for v in h["test1"].values())
    first, last = sum(hist[0]["train"].values()), sum(hist[-1]["train"].values())
    print("total: first step %.3f, mean of steps 1..40 %.3f" % (first, last))
    assert last < first
