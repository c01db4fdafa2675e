"""GPU: the augmentation kernels of csrc/augment.hip one by one through the C ABI (ctypes on raw pointers: offset pointers, any row pitch), against the float64
restatements and Philox mirrors of tests/augment_ref.py, at the shapes where their indexing can go wrong: the scalar staging loop (rows that are no whole float4s, a
misaligned x), a partial last band, band heights shrunk to fit the LDS, a halo wider than the image (r = H), radius 0 beside larger radii, the radius clamp, taps that
underflow, permutations of 1 and of 4096 patches, pitches wider and narrower than a row, invalid sizes, out-of-range and repeated permutation entries, and the second
grid-stride trip of the gather.

The low-pass channels are held element by element under augment_ref.gauss_bound: the project's rule 1e-4 |ref| + 1e-5 scale plus a sum term DERIVED beside its
definition (the two chains' operation count and the error of an fp32 tap), never fitted; tests/test_augment_host.py shows that a float32 run of the kernel's own order
stays within half of it and that six wrong kernels break it.  Everything else -- the x channels, x - low of the returned channels, the staged copies, a second launch,
draws, permutations, gathers -- is held bit for bit.

Every output buffer is a few elements longer than the kernel may write and pre-filled with a sentinel (3.0; -7 for index buffers): the tail must still hold it.  Every
compared figure is printed before it is asserted (pytest -s).  Measured on MI355X: LAB_NOTES.md, "Augmentation kernels: kernel-level parity"."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_ref as A  # noqa: E402
from test_gpu_gm_pointwise import bits_equal, close, dev, filled  # noqa: E402

pytestmark = pytest.mark.gpu

F64, F32, BF, I32 = torch.float64, torch.float32, torch.bfloat16, torch.int32
SENT, ISENT = 3.0, -7
SEED, STEP, OFFSET = A.SEED, A.STEP, A.OFFSET


@pytest.fixture(scope="module")
def lib(lib_built):
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from split_vae_amd import _lib
    return _lib.load()


def _p(t, off=0):
    """the address of element `off` of a device tensor"""
    return C.c_void_p(t.data_ptr() + off * t.element_size())


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dt(dtype):
    from split_vae_amd import _lib
    return _lib.SV_BF16 if dtype == BF else _lib.SV_F32


def ok(rc, what):
    torch.cuda.synchronize()
    assert rc == 0, (what, "status %d" % rc)


def untouched(what, t, sent=SENT):
    assert bool((t == sent).all()), (what, "the sentinel was overwritten", int((t != sent).sum()))


def ifilled(n):
    return torch.full((n,), ISENT, dtype=I32, device="cuda")


def check_staged(what, x8, xh8, got, n, nch, dt):
    """x8 / xh8 [n pixels, 8] of dtype dt against the fp32 images `got` [n, nch]: channels 0-2 the one rounding of channels 0-2 / 3-5, channels 3-7 exact zeros"""
    for name, t, lo in (("x8", x8, 0), ("xh8", xh8, 3)):
        v = t[:n * 8].view(n, 8)
        want = got[:, lo:lo + 3].to(dt).contiguous()
        same = bits_equal(v[:, :3].contiguous(), want)
        z = v[:, 3:].contiguous()
        nonzero = int((z.view(torch.int16 if dt == BF else torch.int32) != 0).sum())
        print("%-58s %s %s: channels 0-2 the rounding of the fp32 value: %s, nonzero pad words %d" % (what, name, "bf16" if dt == BF else "f32", same, nonzero))
        assert same and nonzero == 0, (what, name, dt)
        untouched(what + " " + name + " tail", t[n * 8:])


# ------------------------------------------------------------------------------------------------------------------- Gaussian filter
def _gauss_call(lib, c, xd, rad, std, out, staged=None):
    """one launch of the case's entry point; staged: (x8, xh8, dtype)"""
    B, H, x = c.B, c.H, _p(xd, c.x_offset)
    if c.call == "blur":
        if staged is None:
            return lib.sv_gauss_blur(x, _p(rad), _p(std), _p(out), B, H, H, c.rmax, _st())
        return lib.sv_gauss_blur_staged(x, _p(rad), _p(std), _p(out), _p(staged[0]), _p(staged[1]), _dt(staged[2]), B, H, H, c.rmax, _st())
    if staged is None:
        return lib.sv_high_low_pass(x, _p(out), B, H, H, c.rmax, c.mean, c.stds[0], _st())
    return lib.sv_high_low_pass_staged(x, _p(out), _p(staged[0]), _p(staged[1]), _dt(staged[2]), B, H, H, c.rmax, c.mean, c.stds[0], _st())


@pytest.mark.parametrize("c", A.GAUSS_CASES, ids=repr)
def test_gauss_filter_against_fp64(lib, c):
    """sv_gauss_blur / sv_high_low_pass and their _staged twins in both dtypes at one case of augment_ref.GAUSS_CASES (the table says what each is for)"""
    x, low, bound = A.gauss_case_reference(c)
    B, H = c.B, c.H
    n, nch = B * H * H, (6 if c.call == "blur" else 9)
    xd = filled((n * 3 + 8,))
    xd[c.x_offset:c.x_offset + n * 3] = torch.from_numpy(x).reshape(-1).cuda()
    assert (xd.data_ptr() + 4 * c.x_offset) % 16 == (4 * c.x_offset) % 16                # the allocation is 16-byte aligned: the offset alone decides the staging loop
    rad = torch.tensor(c.radii, dtype=I32).cuda()
    std = dev(torch.tensor(c.stds))
    out = filled((n * nch + 7,))
    ok(_gauss_call(lib, c, xd, rad, std, out), c.name)
    got = out[:n * nch].view(n, nch)
    g = got.cpu()
    xt = torch.from_numpy(x).reshape(n, 3)
    bad = int((g[:, :3].contiguous().view(I32) != xt.view(I32)).sum())
    print("%-58s channels 0-2: %d of %d words differ from x" % (c.name, bad, n * 3))
    assert bad == 0
    lo = nch - 3
    ref, bnd = torch.from_numpy(low).reshape(n, 3), torch.from_numpy(bound).reshape(n, 3)
    for b in range(B):                                              # per image: each has its own radius and std
        s = slice(b * H * H, (b + 1) * H * H)
        close("%s image %d r %d std %.4g low" % (c.name, b, c.used_radii()[b], c.stds[b]), g[s, lo:], ref[s], scale=torch.zeros_like(ref[s]), rtol=0.0, floor=bnd[s])
    sumterm = (bnd - A.F32_RTOL * ref.abs()).clamp_min(1e-300)      # (for the notes: what is left of the bound without the 1e-4 |ref|; not asserted)
    print("%-58s worst err / (bound - 1e-4 |ref|) %.4f" % (c.name, float(((g[:, lo:].to(F64) - ref).abs() / sumterm).max())))
    if nch == 9:
        high = (got[:, :3] - got[:, 6:]).contiguous()
        same = bits_equal(got[:, 3:6].contiguous(), high)
        print("%-58s channels 3-5 == x - low of the returned channels: %s" % (c.name, same))
        assert same
    untouched(c.name + " images tail", out[n * nch:])
    untouched(c.name + " x", torch.cat([xd[:c.x_offset], xd[c.x_offset + n * 3:]]))
    out2 = filled((n * nch + 7,))
    ok(_gauss_call(lib, c, xd, rad, std, out2), c.name)
    assert bits_equal(out2, out), (c.name, "a second launch differs")
    for dt in (F32, BF):
        o3, x8, xh8 = filled((n * nch + 7,)), filled((n * 8 + 16,), dt), filled((n * 8 + 16,), dt)
        ok(_gauss_call(lib, c, xd, rad, std, o3, staged=(x8, xh8, dt)), c.name + " staged")
        assert bits_equal(o3, out), (c.name, dt, "the staged call writes other images")
        check_staged(c.name, x8, xh8, got, n, nch, dt)


# ------------------------------------------------------------------------------------------------------------------- draws
@pytest.mark.parametrize("B", A.DRAW_B)
def test_draws_are_the_philox_mirror(lib, B):
    """sv_blur_params, sv_mix_sizes and sv_mix_size_host at B below, at and above one 256-thread block and at several: radii and sizes the mirror's exactly; std within
    one fp32 ulp of the mirror's float64 value (5 + 5 u rounds once or twice, as the compiler fuses it or not) and inside [5, 10)"""
    rad, std, siz = ifilled(B + 5), filled((B + 5,)), ifilled(B + 5)
    ok(lib.sv_blur_params(_p(rad), _p(std), B, SEED, STEP, OFFSET, _st()), "sv_blur_params")
    ok(lib.sv_mix_sizes(_p(siz), B, SEED, STEP, OFFSET, _st()), "sv_mix_sizes")
    r_ref, s_ref = A.blur_params(B, SEED, STEP, OFFSET)
    z_ref = A.mix_sizes(B, SEED, STEP, OFFSET)
    r, s, z = rad[:B].cpu().numpy(), std[:B].cpu().numpy(), siz[:B].cpu().numpy()
    ulps = np.abs(s.astype(np.float64) - s_ref) / np.spacing(s).astype(np.float64)
    host = np.array([lib.sv_mix_size_host(SEED, STEP, OFFSET + b) for b in range(B)], dtype=np.int32)
    print("draws B %4d: radii differing %d, sizes differing %d, host sizes differing %d, std worst %.3f ulp, range [%.7f, %.7f]"
          % (B, int((r != r_ref).sum()), int((z != z_ref).sum()), int((host != z).sum()), float(ulps.max()), float(s.min()), float(s.max())))
    assert np.array_equal(r, r_ref) and np.array_equal(z, z_ref) and np.array_equal(host, z)
    assert float(ulps.max()) <= 1.0 and bool((s >= 5).all()) and bool((s < 10).all())
    untouched("radius tail", rad[B:], ISENT)
    untouched("std tail", std[B:])
    untouched("sizes tail", siz[B:], ISENT)


def test_std_draw_that_rounds_to_ten_is_clamped_below_it(lib):
    """the recorded draw with c1 >> 8 == 2^24 - 1 (augment_ref.STD_CLAMP_DRAW): 5 + 5 (1 - 2^-24) is 10.f in fp32, and the kernel must answer the largest float
    below 10"""
    d = A.STD_CLAMP_DRAW
    rad, std = ifilled(4), filled((4,))
    ok(lib.sv_blur_params(_p(rad), _p(std), 1, d["seed"], d["step"], d["sample"], _st()), "sv_blur_params")
    got = std[:1].cpu().numpy()[0]
    print("std at the clamp draw: %.9g (the mirror's float64 value %.9f), radius %d" % (got, A.blur_params(1, d["seed"], d["step"], d["sample"])[1][0], int(rad[0])))
    assert got == A.STD_BELOW_10 and int(rad[0]) == int(A.blur_params(1, d["seed"], d["step"], d["sample"])[0][0])
    untouched("std tail", std[1:])
    untouched("radius tail", rad[1:], ISENT)


# ------------------------------------------------------------------------------------------------------------------- sv_random_perm_mixed
@pytest.mark.parametrize("name,H,sizes,ld,why", A.PERM_CASES, ids=[c[0] for c in A.PERM_CASES])
def test_random_perm_mixed_is_the_mirror(lib, name, H, sizes, ld, why):
    B = len(sizes)
    buf = ifilled(B * ld + 5)
    ok(lib.sv_random_perm_mixed(_p(buf), _p(torch.tensor(sizes, dtype=I32).cuda()), B, H, ld, SEED, STEP, OFFSET, _st()), name)
    want = A.random_perm_mixed(sizes, H, ld, SEED, STEP, OFFSET, prefill=ISENT)
    got = buf[:B * ld].view(B, ld).cpu().numpy()
    for b, s in enumerate(sizes):
        print("%-18s row %d size %3d valid %-5s: %d of %d entries differ from the mirror" % (name, b, s, A.mix_valid(s, H, ld), int((got[b] != want[b]).sum()), ld))
    assert np.array_equal(got, want), (name, why)
    untouched(name + " tail", buf[B * ld:], ISENT)
    buf2 = ifilled(B * ld + 5)
    ok(lib.sv_random_perm_mixed(_p(buf2), _p(torch.tensor(sizes, dtype=I32).cuda()), B, H, ld, SEED, STEP, OFFSET, _st()), name)
    assert torch.equal(buf, buf2)


# ------------------------------------------------------------------------------------------------------------------- sv_scramble_gather_mixed
@pytest.mark.parametrize("name", [c[0] for c in A.MIX_CASES])
def test_scramble_gather_mixed_against_the_restatement(lib, name):
    """bit for bit against augment_ref.mix_gather_ref; the staged twin in both dtypes writes the same images6 and the rounded, zero-padded copies"""
    x, perm, sizes, ld = A.mix_case_inputs(name)
    B, H = x.shape[0], x.shape[1]
    n = B * H * H
    want = torch.from_numpy(A.mix_gather_ref(x, perm, sizes, ld)).reshape(n, 6)
    xd, pd, sd = dev(torch.from_numpy(x)), torch.from_numpy(perm).cuda(), torch.from_numpy(sizes).cuda()
    out = filled((n * 6 + 7,))
    ok(lib.sv_scramble_gather_mixed(_p(xd), _p(pd), _p(sd), ld, _p(out), B, H, H, _st()), name)
    got = out[:n * 6].view(n, 6)
    diff = (got.cpu().view(I32) != want.view(I32)).view(B, -1).sum(dim=1)
    print("%-18s B %d H %d ld %d: %d of %d words differ (images that differ: %s)" % (name, B, H, ld, int(diff.sum()), n * 6, torch.nonzero(diff).flatten().tolist()[:8]))
    assert int(diff.sum()) == 0
    untouched(name + " images6 tail", out[n * 6:])
    for dt in (F32, BF):
        o2, x8, xh8 = filled((n * 6 + 7,)), filled((n * 8 + 16,), dt), filled((n * 8 + 16,), dt)
        ok(lib.sv_scramble_gather_mixed_staged(_p(xd), _p(pd), _p(sd), ld, _p(o2), _p(x8), _p(xh8), _dt(dt), B, H, H, _st()), name + " staged")
        assert bits_equal(o2, out), (name, dt, "the staged call writes other images6")
        check_staged(name, x8, xh8, got, n, 6, dt)
