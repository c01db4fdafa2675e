"""GPU: the SPLIT-VAE pointwise kernels of csrc/pointwise.hip and csrc/dlogistic.hip.h one by one through ops.*, against the float64 restatements and Philox mirrors of
tests/pointwise_ref.py, at the shapes where their indexing can go wrong: scalar tails, capped grids and their second grid-stride trip, sizes below one block, row
counts that are no multiple of the 4 waves of a block, lane loops at L < 64 and L % 64 != 0, unaligned tensor offsets, non-square images, one-pixel rows and columns.

The rule for an fp32 output, element by element (tests/test_gpu_gm_pointwise.py states it): |gpu - ref| <= 1e-4 |ref| + 1e-5 scale, scale the largest |addend| of the
element in the float64 reference.  Where the kernel's arithmetic needs more -- -log(delta) at delta -> 1, a per-image sum over 3 HW terms, a clip factor that rests on
a 256-part norm -- the floor or sum term is DERIVED beside its definition in pointwise_ref.py (chain length per thread, tree depth, partial count), never fitted.
Index bookkeeping (scramble, permutation, the Philox words) and everything that is the same arithmetic in the same order (twin launches against stand-alone ones,
flat against per-tensor Adam, bf16 outputs against the rounding of the fp32 output) is held bit for bit.

Every output buffer is a few elements longer than the kernel may write and pre-filled with a sentinel (3.0): what lies behind n, behind row B or behind the stated
workspace size must still hold it.  Every compared figure is printed before it is asserted (pytest -s).  Measured on MI355X: LAB_NOTES.md, "SPLIT-VAE pointwise kernels:
kernel-level parity"."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pointwise_ref as R  # noqa: E402
from oracle import np_ref  # noqa: E402
from test_gpu_gm_pointwise import bits_equal, close, dev, filled, same_bf16  # noqa: E402

pytestmark = pytest.mark.gpu

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
SEED, STEP = 0xF234567890ABCDEF, (3 << 32) | 5                    # a seed with high bits set; the step's high word must not reach the counter
OFFSET = (1 << 32) + 5                                            # a global sample index above 2^32: the high word of the counter
SENT = 3.0


@pytest.fixture(scope="module")
def ops(lib_built):
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from split_vae_amd import ops as o
    return o


def untouched(what, t):
    assert bool((t == SENT).all()), (what, "the sentinel was overwritten", int((t != SENT).sum()))


def refused(ops, status, fn, *a, **kw):
    from split_vae_amd._lib import SplitVaeError
    with pytest.raises(SplitVaeError, match=status):
        fn(*a, **kw)


# ------------------------------------------------------------------------------------------------------------------- a. scramble
@pytest.mark.parametrize("B,H,patch", [(3, 8, 8), (2, 8, 1), (5, 32, 4), (257, 64, 16)])
def test_scramble_and_staged(ops, B, H, patch):
    """bit for bit against np_ref.scramble_batch.  (257, 64, 16): 1 052 672 pixels against the 1 048 576 the capped grid covers -- the last image is written by the
    second grid-stride trip alone.  Staged, both dtypes: images6 the same, channels 0-2 of x8 / xh8 the fp32 value or its one bf16 rounding, 3-7 exact zeros."""
    rng = np.random.default_rng(B + H + patch)
    x = rng.standard_normal((B, H, H, 3)).astype(np.float32)
    perm = R.random_perm(B, (H // patch) ** 2, 7, 1)
    want = torch.from_numpy(np_ref.scramble_batch(x, perm, patch).astype(np.float32))
    xd, pd = torch.from_numpy(x).cuda(), torch.from_numpy(perm).cuda()
    n = B * H * H
    out = filled((n * 6 + 7,))
    ops.scramble_gather(xd, pd, patch, out=out)
    got = out[:n * 6].view(B, H, H, 6)
    bad = int((got.cpu().view(torch.int32) != want.view(torch.int32)).sum())
    print("scramble B %d H %d patch %d: %d of %d words differ" % (B, H, patch, bad, n * 6))
    assert bad == 0
    untouched("images6 tail", out[n * 6:])
    for dt in (F32, BF):
        o2, x8, xh8 = filled((n * 6 + 7,)), filled((n * 8 + 16,), dt), filled((n * 8 + 16,), dt)
        ops.scramble_gather(xd, pd, patch, staged=(x8, xh8), out=o2)
        assert bits_equal(o2, out), "the staged call writes other images6"
        for name, t, lo in (("x8", x8, 0), ("xh8", xh8, 3)):
            v = t[:n * 8].view(B, H, H, 8)
            assert bits_equal(v[..., :3].contiguous(), got[..., lo:lo + 3].to(dt).contiguous()), (name, dt)
            z = v[..., 3:].contiguous()
            assert int((z.view(torch.int16 if dt == BF else torch.int32) != 0).sum()) == 0, (name, dt, "pad channels are not exact zeros")
            untouched(name + " tail", t[n * 8:])


# ------------------------------------------------------------------------------------------------------------------- b. random_perm
@pytest.mark.parametrize("n", R.PERM_N)
def test_random_perm_is_the_mirror(ops, n):
    """bit for bit against the NumPy mirror: n = 1, powers of two and their neighbours (the ~0 padding keys of the bitonic sort), 4096 (the largest)"""
    buf = torch.full((3 * n + 5,), -7, dtype=torch.int32, device="cuda")
    ops.random_perm(3, n, SEED, STEP, OFFSET, out=buf)
    want = torch.from_numpy(R.random_perm(3, n, SEED, STEP, OFFSET))
    bad = int((buf[:3 * n].view(3, n).cpu() != want).sum())
    print("random_perm n %d: %d of %d entries differ from the mirror" % (n, bad, 3 * n))
    assert bad == 0 and bool((buf[3 * n:] == -7).all())
    if n > 2:                                                       # the step's low word and the seed are part of the key, and the mirror follows
        assert torch.equal(ops.random_perm(3, n, SEED, STEP + 1, OFFSET).cpu(), torch.from_numpy(R.random_perm(3, n, SEED, STEP + 1, OFFSET)))
        assert torch.equal(ops.random_perm(3, n, 5, STEP, 2).cpu(), torch.from_numpy(R.random_perm(3, n, 5, STEP, 2)))


def test_random_perm_limits_and_mixed_rows(ops):
    refused(ops, "SV_E_UNSUPPORTED", ops.random_perm, 3, 4097, SEED)
    sizes = torch.tensor([1, 2, 4, 8, 8, 1], dtype=torch.int32).cuda()
    perm = ops.random_perm_mixed(sizes, 32, SEED, STEP, OFFSET).cpu()
    assert perm.shape == (6, 1024)
    for b, s in enumerate(sizes.cpu().tolist()):
        n = (32 // s) ** 2
        assert torch.equal(perm[b, :n], torch.from_numpy(R.random_perm(1, n, SEED, STEP, OFFSET + b)[0])), (b, s)
        assert bool((perm[b, n:] == -1).all())


# ------------------------------------------------------------------------------------------------------------------- c. discretised logistic
_DLL = {}


def dll_case(shape):
    """inputs and float64 references of one shape, computed once and shared (never modified)"""
    if shape not in _DLL:
        images6, out6, _ = R.dll_inputs(*shape, seed=sum(shape))
        B = shape[0]
        refs = {(net, gs): R.dll_ref(images6, 3 * net, out6[net], gs) for net in (0, 1) for gs in (1.0 / B, 1.0)}
        _DLL[shape] = (images6, out6, refs, images6.cuda(), out6.cuda())
    return _DLL[shape]


def _dll_alone(ops, imd, od, net, B, H, W, gdt, gs):
    n, wsf = B * H * W * 8, ops.dlogistic_nll_workspace_floats(B, H, W)
    nll, ws = filled((B + 3,)), filled((wsf + 4,))
    grad = None if gdt is None else filled((n + 8,), gdt)
    ops.dlogistic_nll(imd, 3 * net, od[net], grad_scale=gs, nll=nll, grad=grad, ws=ws)
    untouched("nll behind B", nll[B:])
    untouched("workspace behind sv_dlogistic_nll_workspace_bytes", ws[wsf:])
    if grad is not None:
        untouched("grad tail", grad[n:])
    return nll, ws, grad


@pytest.mark.parametrize("gdt", [None, F32, BF], ids=["nograd", "f32", "bf16"])
@pytest.mark.parametrize("shape", R.DLL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_dlogistic(ops, shape, gdt):
    """ch_off 0 and 3 stand-alone, then both networks through the TWIN launch, which must give the same bits.  Per image: the NLL against float64 under the rule plus
    pointwise_ref.dll_sum_term; it is also the index-order fp32 sum of the P partials in the workspace.  Per element: d nll / d m and d nll / d log_scale times
    grad_scale (1 / B; fp32 also 1) under the rule plus the underflow floor; channels 6-7 zero; the bf16 gradient is the rounding of the fp32 call's own output."""
    B, H, W = shape
    HW, P = H * W, R.dll_parts(H * W)
    images6, out6, refs, imd, od = dll_case(shape)
    tag = "dlogistic %dx%dx%d P %d" % (B, H, W, P)
    wsf = ops.dlogistic_nll_workspace_floats(B, H, W)
    assert wsf == B * P
    gs = 1.0 / B
    alone = []
    for net in (0, 1):
        r = refs[(net, gs)]
        nll, ws, grad = _dll_alone(ops, imd, od, net, B, H, W, gdt, gs)
        alone.append((nll, ws, grad))
        close("%s ch_off %d nll" % (tag, 3 * net), nll[:B], r["nll"], r["nll_max"], floor=R.dll_sum_term(HW, r["nll_sumabs"]))
        assert np.array_equal(nll[:B].cpu().numpy(), R.rowsum_ref32(ws[:wsf].view(B, P).cpu().numpy())), "nll is not the index-order sum of its partials"
        if gdt is None:
            continue
        n32, _, g32 = (nll, ws, grad) if gdt == F32 else _dll_alone(ops, imd, od, net, B, H, W, F32, gs)
        if gdt == BF:
            assert bits_equal(n32, nll)
            gb, gf = grad[:B * HW * 8].float().cpu(), g32[:B * HW * 8].cpu()
            normal = (gf.abs() >= R.FLT_MIN) | (gf == 0)           # (an fp32 subnormal may reach bf16 as itself or as zero: the conversion may flush it)
            want = gf.to(BF).float()
            bad = int((gb[normal] != want[normal]).sum())
            print("%s ch_off %d bf16 grad: %d of %d differ from the rounded fp32 output, %d subnormal" % (tag, 3 * net, bad, gb.numel(), int((~normal).sum())))
            assert bad == 0 and bool((gb[~normal].abs() <= R.FLT_MIN).all())
            continue
        for scale_, g_ in ((gs, g32),) + (((1.0, _dll_alone(ops, imd, od, net, B, H, W, F32, 1.0)[2]),) if B > 1 else ()):
            rr = refs[(net, scale_)]
            g = g_[:B * HW * 8].view(B, H, W, 8)
            assert int((g[..., 6:].contiguous().view(torch.int32) != 0).sum()) == 0, "gradient channels 6-7 are not zero"
            close("%s ch_off %d grad_scale %.3g d/dm" % (tag, 3 * net, scale_), g[..., :3], rr["g"][..., :3], rr["g_scale"][..., :3], floor=rr["g_floor"][..., :3])
            close("%s ch_off %d grad_scale %.3g d/dls" % (tag, 3 * net, scale_), g[..., 3:6], rr["g"][..., 3:], rr["g_scale"][..., 3:], floor=rr["g_floor"][..., 3:])
            for name, m in (("rare", rr["rare"]), ("x<-.999", rr["lo"]), ("x>.999", rr["hi"])):
                e = ((g[..., :6].double().cpu() - rr["g"]).abs() / rr["g"].abs().clamp_min(1e-300))[m.repeat(1, 1, 1, 2) & (rr["g"].abs() > 1e-30)]
                print("    branch %-8s %7d elements, worst rel %.3e" % (name, int(m.sum()), float(e.max()) if e.numel() else 0.0))
    # the twin launch: same per-thread order, same tree -- the same bits
    n = B * HW * 8
    nll2, ws2 = filled((2, B + 3)), filled((2, wsf + 4))
    grad2 = None if gdt is None else filled((2, n + 8), gdt)
    ops.dlogistic_nll_twin(imd, od, nll2, ws2, grad=grad2, grad_scale=gs)
    for net in (0, 1):
        nll, ws, grad = alone[net]
        assert bits_equal(nll2[net].contiguous(), nll), (tag, "twin nll", net)
        assert bits_equal(ws2[net].contiguous(), ws), (tag, "twin partials", net)
        if grad is not None:
            bad = int((grad2[net].contiguous().view(torch.int16 if gdt == BF else torch.int32) != grad.view(torch.int16 if gdt == BF else torch.int32)).sum())
            print("%s twin net %d: %d gradient words differ from the stand-alone call" % (tag, net, bad))
            assert bad == 0


@pytest.mark.parametrize("m,ls", R.SUMS_TO_ONE)
def test_dlogistic_sums_to_one(ops, m, ls):
    """sum over the 256 bins of exp(-nll) == 1 for any (m, log_scale), as tests/test_gpu_kernels.py has it, also at log_scale -7 and 2"""
    x6, out6 = R.sums_to_one_inputs(m, ls)
    nll, _ = ops.dlogistic_nll(x6.cuda(), 0, out6.cuda())
    total = float(np.exp(-nll.cpu().double().numpy()).sum())
    print("dlogistic bins m %+.1f ls %+.1f: sum %.9f" % (m, ls, total))
    assert abs(total - 1.0) < 1e-4, (m, ls, total)


# ------------------------------------------------------------------------------------------------------------------- d. reparam / KL
def _reparam_fwd(ops, ins, B, L, dt, eps=True, **kw):
    pre, bias, e = ins[:3]
    rows = B + 2
    bufs = [filled((rows * L,)) for _ in range(3)] + [filled((rows * L,), dt), filled((rows,)), filled((rows * L,))]
    ops.reparam_kl_fwd(dev(pre), dev(bias), dev(e) if eps else None, z_dtype=dt, out=tuple(bufs), **kw)
    o = dict(zip(("z_mean", "z_sig", "z", "z_lp", "kl", "eps_out"), bufs))
    for k, t in o.items():
        w = B if k == "kl" else B * L
        untouched(k + " behind row B", t[w:])
        o[k] = t[:w] if k == "kl" else t[:w].view(B, L)
    return o


@pytest.mark.parametrize("lp_bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,L", R.REPARAM_SHAPES)
def test_reparam_kl_fwd_bwd(ops, B, L, lp_bf16):
    """Sampling + KL and the adjoint.  B is no multiple of the 4 waves of a block; L = 1, 10 (one partial lane trip), 64, 100 and 130 (a partial second / third trip), 256.
    Whole rows of the sigma pre-activation pinned at -7, -9, -11, -14 and +12."""
    dt = BF if lp_bf16 else F32
    tag = "reparam B %d L %d" % (B, L)
    ins = R.reparam_inputs(B, L, B + L)
    pre, bias, eps, dz, dz2 = ins
    o = _reparam_fwd(ops, ins, B, L, dt)
    r = R.reparam_fwd_ref(pre, bias, eps)
    close(tag + " z_mean", o["z_mean"], r["z_mean"], r["mean_scale"])
    close(tag + " z_sig", o["z_sig"], r["z_sig"])
    for k, v in enumerate(R.PINS[:B]):
        print("    row pinned at %+5.0f: z_sig worst rel %.3e" % (v, float(((o["z_sig"][k].double().cpu() - r["z_sig"][k]).abs() / r["z_sig"][k]).max())))
    close(tag + " z", o["z"], r["z"], r["z_scale"])
    close(tag + " kl", o["kl"], r["kl"], r["kl_scale"], floor=R.kl_sum_term(L, r["kl_sumabs"]))
    assert bits_equal(o["z_lp"].contiguous(), o["z"].to(dt).contiguous()), "z_lp is not the cast of z"
    assert torch.equal(o["eps_out"].cpu(), eps)
    # backward: fp32 under the rule, bf16 the rounding of the fp32 result; with the second addend and without
    ks = 40.0 / B
    zm, zs, eo = (o[k].contiguous() for k in ("z_mean", "z_sig", "eps_out"))
    for two in (True, False):
        g32 = filled((B * 2 * L + 6,))
        ops.reparam_kl_bwd(dev(dz), zm, zs, eo, ks, g_dtype=F32, dz2=dev(dz2) if two else None, out=g32)
        untouched("g_pre tail", g32[B * 2 * L:])
        if lp_bf16:
            gb = filled((B * 2 * L + 6,), BF)
            ops.reparam_kl_bwd(dev(dz), zm, zs, eo, ks, g_dtype=BF, dz2=dev(dz2) if two else None, out=gb)
            untouched("g_pre tail", gb[B * 2 * L:])
            assert bits_equal(gb[:B * 2 * L], g32[:B * 2 * L].to(BF)), "the bf16 gradient is not the rounding of the fp32 one"
        else:
            ref, scale = R.reparam_bwd_ref(dz, dz2 if two else None, pre, bias, eps, R.f32(ks))
            close("%s g_pre %s" % (tag, "dz + dz2" if two else "dz"), g32[:B * 2 * L].view(B, 2 * L), ref, scale)


@pytest.mark.parametrize("B,L", R.REPARAM_SHAPES)
def test_reparam_philox_draw(ops, B, L):
    """eps = NULL: eps_out against the Box-Muller mirror within 1e-6 (the bound tests/test_gpu_gm_pointwise.py holds gm_head_fwd's draw to: the same formula), for
    stream ids 0 and 1 and a sample offset above 2^32; a shard is bit for bit the rows of the full draw"""
    ins = R.reparam_inputs(B, L, B + L)
    full = {}
    for sid in (0, 1):
        o = _reparam_fwd(ops, ins, B, L, F32, eps=False, seed=SEED, step=STEP, stream_id=sid, sample_offset=OFFSET)
        e = o["eps_out"].double().cpu()
        err = float((e - R.reparam_eps(B, L, SEED, STEP, sid, OFFSET)).abs().max())
        print("reparam Philox B %d L %d stream %d: worst |eps_out - mirror| %.3e" % (B, L, sid, err))
        assert err <= 1e-6
        r = R.reparam_fwd_ref(ins[0], ins[1], e)
        close("reparam Philox z", o["z"], r["z"], r["z_scale"])
        full[sid] = o["eps_out"]
    assert B * L < 4 or not torch.equal(full[0], full[1])
    if B >= 2:
        r0 = B // 2
        sh = _reparam_fwd(ops, [ins[0][r0:], ins[1], None], B - r0, L, F32, eps=False, seed=SEED, step=STEP, stream_id=1, sample_offset=OFFSET + r0)
        assert bits_equal(sh["eps_out"].contiguous(), full[1][r0:].contiguous()), "a shard is not the rows of the full draw"


@pytest.mark.parametrize("lp_bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,L,L2", [(1, 1, 3), (5, 10, 64), (7, 100, 130), (9, 256, 100)])
def test_reparam_twin_entry_points_plain_tensors(ops, B, L, L2, lp_bf16):
    """sv_reparam_kl_*_twin on the S = 0 path: a different L per network, z_col > 0, ldz and ld_dz wider than L -- bit for bit the stand-alone calls, the columns
    around the two blocks of z_lp and the rows behind B untouched"""
    dt = BF if lp_bf16 else F32
    Ls = (L, L2)
    ins = [R.reparam_inputs(B, Ls[e], B + Ls[e] + e) for e in (0, 1)]
    alone = [_reparam_fwd(ops, ins[e], B, Ls[e], dt) for e in (0, 1)]
    cols = (3, 3 + L + 2)
    ldz = cols[1] + L2 + 4
    z_lp = filled((B + 1, ldz), dt)
    nets, keep = [], []
    for e in (0, 1):
        pre, bias, eps = (dev(t) for t in ins[e][:3])
        o = {k: filled((B + 1, Ls[e])) for k in ("eps_out", "z_mean", "z_sig", "z")}
        o["kl"] = filled((B + 1,))
        keep.append(o)
        nets.append(dict(o, pre=pre, bias_mean=bias[:Ls[e]], bias_sd=bias[Ls[e]:], eps=eps, L=Ls[e], z_col=cols[e]))
    ops.reparam_kl_fwd_twin(nets, z_lp, ldz, B)
    for e in (0, 1):
        for k in ("z_mean", "z_sig", "z", "eps_out", "kl"):
            assert bits_equal(keep[e][k][:B].contiguous(), alone[e][k].contiguous()), (e, k)
            untouched("%s row B" % k, keep[e][k][B:])
        assert bits_equal(z_lp[:B, cols[e]:cols[e] + Ls[e]].contiguous(), alone[e]["z_lp"].contiguous()), (e, "z_lp")
    mask = torch.ones(B + 1, ldz, dtype=torch.bool)
    for e in (0, 1):
        mask[:B, cols[e]:cols[e] + Ls[e]] = False
    untouched("z_lp around the blocks", z_lp[mask.cuda()])
    # backward: padded dz / dz2
    ks = 40.0 / B
    bw, want = [], []
    for e in (0, 1):
        Le = Ls[e]
        dz = dev(torch.cat([ins[e][3], torch.full((B, 3), 9.0)], dim=1))
        dz2 = dev(torch.cat([ins[e][4], torch.full((B, 5), 9.0)], dim=1))
        zm, zs, eo = (alone[e][k].contiguous() for k in ("z_mean", "z_sig", "eps_out"))
        g = filled((B + 1, 2 * Le), dt)
        bw.append(dict(dz=dz, ld_dz=Le + 3, dz2=dz2, ld_dz2=Le + 5, z_mean=zm, z_sig=zs, eps=eo, g_pre=g, L=Le))
        want.append(ops.reparam_kl_bwd(dz, zm, zs, eo, ks, g_dtype=dt, dz2=dz2))          # (the stand-alone call takes the padded pitches as well)
        plain = ops.reparam_kl_bwd(dev(ins[e][3]), zm, zs, eo, ks, g_dtype=dt, dz2=dev(ins[e][4]))
        assert bits_equal(want[e], plain), "ld_dz > L changes the stand-alone result"
    ops.reparam_kl_bwd_twin(bw, ks, dt, B)
    for e in (0, 1):
        assert bits_equal(bw[e]["g_pre"][:B].contiguous(), want[e]), (e, "g_pre")
        untouched("g_pre row B", bw[e]["g_pre"][B:])


# ------------------------------------------------------------------------------------------------------------------- e. Adam
@pytest.mark.parametrize("t0,gs", [(1, 1.0 / 64), (1000, 1.0)], ids=["t1_gs1/64", "t1000_gs1"])
@pytest.mark.parametrize("n", R.ADAM_N)
def test_adam_step_per_element(ops, n, t0, gs):
    """three consecutive steps from a live state; p, m, v per element against float64, the reference state re-synchronised to the device's after every step (a step's
    rounding is judged once).  n = 1 .. 7 and 1027: the scalar tail alone and behind a float4 body; 4 * 256 * 2048 + 4099: the 2048-block cap, a second grid-stride
    trip and a 3-element tail."""
    p, m, v, grads = R.adam_inputs(n, n % 1000 + t0)
    bufs = [filled((n + 5,)) for _ in range(4)]
    for b, s in zip(bufs[:3], (p, m, v)):
        b[:n] = s.cuda()
    pd, md, vd, gd = bufs
    for k in range(3):
        t = t0 + k
        gd[:n] = grads[k].cuda()
        state = [b[:n].cpu() for b in (pd, md, vd)]
        ops.adam_step(pd, gd, md, vd, t, grad_scale=gs, n=n)
        ref, scales = R.adam_ref(state[0], grads[k], state[1], state[2], t, grad_scale=gs)
        for name, b, r, s in zip("pmv", (pd, md, vd), ref, scales):
            close("adam n %d t %d grad_scale %.3g %s" % (n, t, gs, name), b[:n], r, s)
            untouched(name + " behind n", b[n:])
    zero = grads[0] == 0
    assert bool(zero.any()) or n < 7


def test_adam_step_refusals(ops):
    b = [filled((36,)) for _ in range(4)]
    refused(ops, "SV_E_BADARG", ops.adam_step, b[0][1:], b[1], b[2], b[3], 1, n=8)                  # one float off the 16-byte boundary
    refused(ops, "SV_E_BADARG", ops.adam_step, b[0], b[1][1:], b[2], b[3], 1, n=8)
    refused(ops, "SV_E_BADARG", ops.adam_step, b[0], b[1], b[2], b[3], 1, n=0)
    refused(ops, "SV_E_BADARG", ops.adam_step, b[0], b[1], b[2], b[3], 0, n=8)
    for t in b:
        untouched("a refused call wrote", t)


def test_adam_clipnorm_per_element_and_its_equalities(ops):
    """Keras clipnorm over the table [3, 262149, 1, 0, 1030, 524291]: unaligned offsets, an empty tensor, two tensors past one 262 144-element stride pass; norms 3 and
    0.2, and 1 +- 5e-4.  Per element against float64 (a clipped tensor's factor rests on a 256-part fp32 norm: pointwise_ref.clip_norm_rtol, carried to p, m, v by
    clip_floors).  Then the equalities, bit for bit: flat == per-tensor pointers; clipnorm 1e38 == sv_adam_step; alpha from device memory == alpha from (lr, t)."""
    p, m, v, g, off = R.clip_inputs(3)
    N, t, lr = off[-1], 3, 1e-4
    offd = torch.tensor(off, dtype=torch.int64).cuda()
    gd = dev(g)

    def state():
        return [dev(a).clone() for a in (p, m, v)]
    a = state()
    ops.adam_step_clipnorm(a[0], gd, a[1], a[2], offd, R.CLIPNORM, t, lr)
    sc, norms = R.clip_factor(g, off, R.CLIPNORM)
    print("clipnorm tensor norms", ["%.6f" % x for x in norms])
    E = torch.zeros(N, dtype=F64)
    for (lo, hi), nrm in zip(zip(off[:-1], off[1:]), norms):
        if nrm > 0.99 * R.CLIPNORM:                                 # (a norm within 1e-3 below clipnorm may land on either side in fp32: both are allowed the norm's error)
            E[lo:hi] = R.clip_norm_rtol(hi - lo)
    ref, scales = R.adam_ref(p, g, m, v, t, lr, sc=sc)
    floors = R.clip_floors(E, p, g, m, v, t, sc, lr)
    for name, got, r, s, f in zip("pmv", a, ref, scales, floors):
        close("adam clipnorm %s" % name, got, r, s, floor=f)
    # flat == per-tensor pointers (an empty tensor still needs an address)
    b = state()
    parts = [gd[lo:hi].clone() if hi > lo else torch.zeros(4, device="cuda") for lo, hi in zip(off[:-1], off[1:])]
    ops.adam_step_clipnorm_tensors(b[0], parts, b[1], b[2], offd, R.CLIPNORM, t, lr)
    assert all(bits_equal(x, y) for x, y in zip(a, b)), "flat and per-tensor clipnorm Adam differ"
    # alpha from device memory (the host's t is then not what sets the step size)
    c = state()
    alpha = torch.tensor([ops.adam_alpha(lr, 0.9, 0.999, t)], dtype=F32).cuda()
    ops.adam_step_clipnorm(c[0], gd, c[1], c[2], offd, R.CLIPNORM, t + 4, lr, alpha_dev=alpha)
    assert all(bits_equal(x, y) for x, y in zip(a, c)), "alpha_dev gives another step than (lr, t)"
    # no clipping == the plain step
    d, e = state(), state()
    ops.adam_step_clipnorm(d[0], gd, d[1], d[2], offd, 1e38, t, lr, grad_scale=0.5)
    ops.adam_step(e[0], gd, e[1], e[2], t, lr=lr, grad_scale=0.5)
    for name, x, y in zip("pmv", d, e):
        bad = int((x.view(torch.int32) != y.view(torch.int32)).sum())
        print("clipnorm 1e38 against sv_adam_step, %s: %d of %d words differ" % (name, bad, N))
        assert bad == 0


# ------------------------------------------------------------------------------------------------------------------- f. resize 2x
def _ups_run(ops, x, g_hi, mask, dt):
    B, H, W, C = x.shape
    n = x.numel()
    xd, gd, md = dev(x, dt), dev(g_hi, dt), dev(mask, dt)
    up = filled((4 * n + 8,), dt)
    ops.upsample2x_fwd(xd, out=up)
    untouched("resize output tail", up[4 * n:])
    outs = [up[:4 * n].view(B, 2 * H, 2 * W, C)]
    for mk in (None, md):
        lo = filled((n + 8,), dt)
        ops.upsample2x_bwd(gd, mk, out=lo)
        untouched("adjoint output tail", lo[n:])
        outs.append(lo[:n].view(B, H, W, C))
    return outs


@pytest.mark.parametrize("shape", R.UPS_F32, ids=lambda s: "x".join(map(str, s)))
def test_upsample2x_f32(ops, shape):
    """forward and adjoint per element: W != H, one-pixel rows and columns, C = one 16-byte piece, the per-output adjoint at H % 8 == 0 with too few threads for the
    rows kernel, and the rows kernel with two bands (16, 16, 64, 128) and with one band whose edges are both image edges (64, 8, 32, 128); no mask and a mask holding
    +x, -x, 0.0 and -0.0.  Then <fwd(x), g> == <x, bwd(g)> from the device outputs, in float64, to the sum of the two per-element bounds."""
    tag = "resize f32 " + "x".join(map(str, shape))
    x, g_hi, mask = R.ups_inputs(shape, sum(shape))
    up, lo, lom = _ups_run(ops, x, g_hi, mask, F32)
    ur, us = R.upsample_ref(x)
    close(tag + " fwd", up, ur, us)
    lr_, ls_ = R.upsample_bwd_ref(g_hi)
    close(tag + " adjoint", lo, lr_, ls_)
    lmr, lms = R.upsample_bwd_ref(g_hi, mask)
    close(tag + " adjoint, mask", lom, lmr, lms)
    closed = (mask <= 0)
    assert int((lom.cpu()[closed].view(torch.int32) & 0x7FFFFFFF != 0).sum()) == 0, "a closed mask element (-x, 0.0, -0.0) lets a gradient through"
    a = float((up.double().cpu() * g_hi.double()).sum())
    b = float((x.double() * lo.double().cpu()).sum())
    bound = float(((1e-4 * ur.abs() + 1e-5 * us) * g_hi.double().abs()).sum() + ((1e-4 * lr_.abs() + 1e-5 * ls_) * x.double().abs()).sum())
    print("%-58s <fwd x, g> %.9e  <x, bwd g> %.9e  |diff| / bound %.4f" % (tag, a, b, abs(a - b) / bound))
    assert abs(a - b) <= bound


@pytest.mark.parametrize("shape", R.UPS_BF16, ids=lambda s: "x".join(map(str, s)))
def test_upsample2x_bf16(ops, shape):
    """bf16 in and out: equality with the float64 result rounded once (pointwise_ref.ups_inputs says why that is the right question for these inputs)"""
    tag = "resize bf16 " + "x".join(map(str, shape))
    x, g_hi, mask = R.ups_inputs(shape, sum(shape), bf16=True)
    up, lo, lom = _ups_run(ops, x, g_hi, mask, BF)
    same_bf16(tag + " fwd", up, R.upsample_ref(x)[0])
    same_bf16(tag + " adjoint", lo, R.upsample_bwd_ref(g_hi)[0])
    same_bf16(tag + " adjoint, mask", lom, R.upsample_bwd_ref(g_hi, mask)[0])


def test_upsample2x_refuses_partial_pieces(ops):
    for dt, C in ((F32, 6), (BF, 12)):
        x = torch.zeros(1, 2, 2, C, dtype=dt, device="cuda")
        refused(ops, "SV_E_UNSUPPORTED", ops.upsample2x_fwd, x)
        refused(ops, "SV_E_UNSUPPORTED", ops.upsample2x_bwd, torch.zeros(1, 4, 4, C, dtype=dt, device="cuda"))


# ------------------------------------------------------------------------------------------------------------------- g. loss finaliser
def _fin_bufs(terms, B):
    out = []
    for t in terms:
        b = filled((B + 3,))
        b[:B] = t.cuda()
        out.append(b)
    return out


@pytest.mark.parametrize("B", R.FINALIZE_B)
def test_finalize_losses(ops, B):
    """the six losses per element (B = 1 .. 600: below a wave, 64 / 65, past the 256 threads, a third trip), accumulate twice and not at all, the one-branch form"""
    terms = R.finalize_inputs(B, B)
    nx, nh, kx, kh = _fin_bufs(terms, B)
    beta = 40.0
    ref, scale = R.finalize_ref(*terms, beta)
    floor = R.finalize_sum_term(B, (terms[0], terms[2], terms[1], terms[3]), beta)
    losses, acc = filled((9,)), filled((9,))
    ops.finalize_losses(nx, beta, losses, nll_xh=nh, kl_x=kx, kl_xh=kh, metric_acc=acc, accumulate=False, B=B)
    close("finalize B %d losses" % B, losses[:6], ref, scale, floor=floor)
    untouched("losses tail", losses[6:])
    untouched("metric_acc without accumulate", acc)
    for b, t in zip((nx, nh, kx, kh), terms):
        assert torch.equal(b[:B].cpu(), t) and bool((b[B:] == SENT).all())
    acc[:6] = 0.0
    l2 = filled((9,))
    for _ in range(2):
        ops.finalize_losses(nx, beta, l2, nll_xh=nh, kl_x=kx, kl_xh=kh, metric_acc=acc, accumulate=True, B=B)
    assert bits_equal(l2, losses)
    assert torch.equal(acc[:5], 2.0 * losses[:5]) and float(acc[5]) == 2.0
    untouched("metric_acc tail", acc[6:])
    # one branch: nll_xh, kl_x, kl_xh null
    l1 = filled((9,))
    ops.finalize_losses(nx, beta, l1, B=B)
    one, one_scale = R.finalize_ref(terms[0], None, None, None, beta)
    close("finalize B %d one branch" % B, l1[:6], one, one_scale, floor=R.finalize_sum_term(B, (terms[0], None, None, None), beta))
    assert [float(v) for v in l1[1:5]] == [0.0] * 4 and float(l1[5]) == float(l1[0]) and bits_equal(l1[:1], losses[:1])


@pytest.mark.parametrize("P", [1, 4, 16])
@pytest.mark.parametrize("B", [3, 257, 600])
def test_finalize_losses_from_partials(ops, B, P):
    """with partials: nll_x / nll_xh are WRITTEN as the index-order fp32 sums of their P partials, and the losses are those of the sums"""
    g = torch.Generator().manual_seed(B + P)
    px, ph = [(0.5 + torch.rand(B, P, generator=g)) * 5e3 / P for _ in range(2)]
    kx, kh = [(0.5 + torch.rand(B, generator=g)) * 30.0 for _ in range(2)]
    pxd, phd = filled((B * P + 4,)), filled((B * P + 4,))
    pxd[:B * P] = px.reshape(-1).cuda()
    phd[:B * P] = ph.reshape(-1).cuda()
    nx, nh = filled((B + 3,)), filled((B + 3,))
    kxd, khd = _fin_bufs((kx, kh), B)
    losses = filled((9,))
    ops.finalize_losses(nx, 40.0, losses, nll_xh=nh, kl_x=kxd, kl_xh=khd, part_x=pxd, part_xh=phd, P=P, B=B)
    sx, sh = torch.from_numpy(R.rowsum_ref32(px.numpy())), torch.from_numpy(R.rowsum_ref32(ph.numpy()))
    assert torch.equal(nx[:B].cpu(), sx) and torch.equal(nh[:B].cpu(), sh), "nll is not the index-order sum of its partials"
    untouched("nll_x behind B", nx[B:])
    untouched("nll_xh behind B", nh[B:])
    ref, scale = R.finalize_ref(sx, sh, kx, kh, 40.0)
    close("finalize B %d P %d from partials" % (B, P), losses[:6], ref, scale, floor=R.finalize_sum_term(B, (sx, kx, sh, kh), 40.0))
    # the one-branch form with partials: part_xh and nll_xh null
    n1, l1 = filled((B + 3,)), filled((9,))
    ops.finalize_losses(n1, 40.0, l1, part_x=pxd, P=P, B=B)
    assert bits_equal(n1, nx) and bits_equal(l1[:1], losses[:1]) and [float(v) for v in l1[1:5]] == [0.0] * 4


@pytest.mark.parametrize("shape", [(2, 32, 32), (2, 64, 64), (1, 128, 128)], ids=["P1", "P4", "P16"])
def test_finalize_losses_sums_the_dlogistic_partials_as_rowsum_does(ops, shape):
    """the partial workspace of a dlogistic call handed to the finaliser: its nll_x / nll_xh are bit for bit the nll rowsum_partials_kernel formed from the same partials"""
    B, H, W = shape
    P = R.dll_parts(H * W)
    images6, out6, refs, imd, od = dll_case(shape)
    nll = []
    ws = []
    for net in (0, 1):
        a, w, _ = _dll_alone(ops, imd, od, net, B, H, W, None, 1.0)
        nll.append(a)
        ws.append(w)
    nx, nh, losses = filled((B + 3,)), filled((B + 3,)), filled((9,))
    ops.finalize_losses(nx, 40.0, losses, nll_xh=nh, part_x=ws[0], part_xh=ws[1], P=P, B=B)
    assert bits_equal(nx, nll[0]) and bits_equal(nh, nll[1])
    ref, scale = R.finalize_ref(nll[0][:B].cpu(), nll[1][:B].cpu(), None, None, 40.0)
    close("finalize from dlogistic partials P %d" % P, losses[:6], ref, scale, floor=R.finalize_sum_term(B, (nll[0][:B].cpu(), None, nll[1][:B].cpu(), None), 40.0))
