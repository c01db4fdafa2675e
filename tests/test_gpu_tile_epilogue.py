"""GPU: the store phase of the fp32 LDS-tile convolution (tile_conv.hip: FAST STORE PATH and the general loop it falls back to), through the
public entry points and against fp64 at the bounds tests/test_gpu_conv_api.py applies to the same calls.

The fast path changes only WHERE a piece is written, so every output lies inside a larger NaN-filled allocation: nothing outside the tensor may
change, pad channels [C, r8(C)) come back exactly zero and the channels beyond r8(C) of a wide pitch stay untouched.

CASES names, per call, the store branch its tiles take.  `store_plan` mirrors the column-tile rule of tile_conv_plan_impl and the kernel's
branch condition on the CPU and is held against that table; the traced child process (SV_TRACE_DISPATCH) shows that the calls run the form the
table assumes -- at fp32 a `tile` / `merged` / `multi_class` / `per_class` / `polyc` / `lowres_polyd` line on power-of-two grids is the tile kernel
(the row-ring kernel is bf16 only, the im2col kernel has neither merged classes nor border terms).

What the planner cannot produce: a launch that mixes full and partial column tiles.  BN divides N for every N > 16 (N = 96 runs three full
32-column tiles), and N <= 16 is ONE 16-column tile, partial when r8(N) < 16 -- the two halves of that case are `n96` and `n4_partial_column`."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

import test_gpu_conv_api as api
from test_gpu_conv_api import F32_ATOL, F32_RTOL, case

GUARD = 4096            # elements of NaN in front of and behind every output

# (case, {call: branches}); calls: fwd, fwd_ws, dgrad, dgrad_masked, lowres_ws.  Branches: "fast" (full fp32 column tile, whole tile inside the batch),
# "general16" / "general8" (the general loop with 16- / 8-byte pieces).  16 x 16 output grids, 3 images, Cin 16 unless the branch needs otherwise.
CASES = [
    # BN = 32, 128-row tiles: 4 pieces per thread.  Pitch 40 > r8(32): 8 floats per pixel stay untouched
    (case("n32", 3, 16, 16, 16, 32, 3, 3, 1, "relu", "f32", ldy=40), {"fwd": {"fast"}}),
    # ... 256-row tiles from 300 workgroups per problem: 8 pieces per thread (4 distinct images)
    (case("n32_b300", 300, 16, 16, 16, 32, 3, 3, 1, "relu", "f32", P=4), {"fwd": {"fast"}}),
    # BN = 64 (a stride-2 forward keeps 64-column tiles): 128-row tiles, 8 pieces; with 8 input channels the 256-row tile fits twice per CU: 16 pieces
    (case("n64_s2", 3, 32, 32, 16, 64, 4, 4, 2, "relu", "f32"), {"fwd": {"fast"}, "dgrad": {"fast"}, "dgrad_masked": {"fast"}}),
    (case("n64_s2_c8", 3, 32, 32, 8, 64, 4, 4, 2, None, "f32"), {"fwd": {"fast"}}),
    # BN = 128 from 200 128 x 128 tiles per problem: 16 pieces per thread, two batches
    (case("n128_b100", 100, 16, 16, 16, 128, 3, 3, 1, "relu", "f32", P=4), {"fwd": {"fast"}}),
    # three column tiles in one launch (n0 = 0, 32, 64)
    (case("n96", 3, 16, 16, 16, 96, 3, 3, 1, None, "f32"), {"fwd": {"fast"}}),
    # one partial 16-column tile: 4 channels + 4 zero pad channels of 16-byte pieces on the general loop
    (case("n4_partial_column", 3, 16, 16, 16, 4, 3, 3, 1, "relu", "f32"), {"fwd": {"general16"}, "dgrad": {"fast"}, "dgrad_masked": {"fast"}}),
    # 8-byte pieces: the 6-channel fp32 head with ldy == Cout
    (case("c6_piece8", 3, 16, 16, 16, 6, 3, 3, 1, None, "f32", yf32=1), {"fwd": {"general8"}}),
    # masked stride-1 input gradient (N = Cin = 32; mask rows of 0, -0 and negatives: _mask_with_zeros)
    (case("dgrad_s1_c32", 3, 16, 16, 32, 16, 3, 3, 1, "relu", "f32"), {"dgrad": {"fast"}, "dgrad_masked": {"fast"}}),
    # stride-2 input gradients: merged parity classes (k 6: cls_n = Cin, N = 4 Cin = 64 / 128) and one problem per class (k 4: OS = 2, ooy / oox)
    (case("merged_c16", 3, 32, 32, 16, 32, 6, 6, 2, "relu", "f32"), {"dgrad": {"fast"}, "dgrad_masked": {"fast"}}),
    (case("merged_c32", 3, 32, 32, 32, 16, 6, 6, 2, "relu", "f32"), {"dgrad": {"fast"}, "dgrad_masked": {"fast"}}),
    (case("classes_c32", 3, 32, 32, 32, 16, 4, 4, 2, "relu", "f32"), {"dgrad": {"fast"}, "dgrad_masked": {"fast"}}),
    # per-class polyphase forward with the border-term epilogue (fix_nc), 8 x 8 low-res: 2 or 4 images per tile, so the last tile of 3 images
    # reaches past the batch and keeps the general loop beside the fast tiles
    (case("polyc_8x8", 3, 16, 16, 32, 32, 6, 6, 1, "relu", "f32", ups=1), {"fwd_ws": {"fast", "general16"}}),
    # polyphase input gradient at the low-res tensor (border terms + mask), 16 x 16 low-res
    (case("polyd_16x16", 3, 32, 32, 32, 32, 6, 6, 1, "relu", "f32", ups=1), {"lowres_ws": {"fast"}}),
]
FORMS = {"n32": {"fwd": "tile"}, "n32_b300": {"fwd": "tile"}, "n64_s2": {"fwd": "tile", "dgrad": "multi_class"},
         "n64_s2_c8": {"fwd": "tile"}, "n128_b100": {"fwd": "tile"}, "n96": {"fwd": "tile"}, "n4_partial_column": {"fwd": "tile", "dgrad": "per_class"},
         "c6_piece8": {"fwd": "tile"}, "dgrad_s1_c32": {"dgrad": "per_class"}, "merged_c16": {"dgrad": "merged"}, "merged_c32": {"dgrad": "merged"},
         "classes_c32": {"dgrad": "multi_class"}, "polyc_8x8": {"fwd_ws": "polyc"}, "polyd_16x16": {"lowres_ws": "lowres_polyd"}}


# ---------------------------------------------------------------- the plan's column-tile rule and the kernel's branch condition, on the CPU
def _column_tile(N, B, OY, OX, S, OS, cls):
    """BN of tile_conv_plan_impl at fp32 (SV_TC_SMALL_WGS 200, SV_TC_TINY_WGS 100, SV_TC_SMALL64_WGS 300, stride-1 forwards only)"""
    tiles = -(-B * OY * OX // 128)
    small = N % 128 == 0 and tiles * (N // 128) < 200 and not cls
    tiny = small and tiles * (N // 128) < 100
    tiny64 = N % 64 == 0 and N % 128 != 0 and tiles * (N // 64) < 300 and not cls and OS == 1 and S == 1
    if N % 128 == 0 and not small:
        return 128
    if N % 64 == 0 and not tiny and not tiny64:
        return 64
    if N % 32 == 0:
        return 32
    return 16 if N <= 16 else None


def store_plan(c, call):
    """-> the set of store branches the tiles of one call take"""
    r8 = api._r8
    B = c.B
    if call in ("fwd", "fwd_ws"):
        polyc = bool(c.ups)                                         # per-class polyphase: low-res grid, one problem per class
        OY, OX = (c.H // 2, c.W // 2) if polyc else (c.H // c.s, c.W // c.s)
        N, S, OS, cls, ldo, f32out = c.Cout, c.s, 2 if polyc else 1, False, (c.ldy or (c.Cout if c.yf32 else r8(c.Cout))), True
    else:
        merged = c.s == 2 and c.KH == 6
        OY, OX = (c.H // 2, c.W // 2) if (c.s == 2 or call == "lowres_ws") else (c.H, c.W)
        N, S, OS, cls, ldo = (4 * c.Cin if merged else c.Cin), (2 if call == "lowres_ws" else 1), (2 if c.s == 2 else 1), merged, (c.ldx or r8(c.Cin))
    BN = _column_tile(N, B, OY, OX, S, OS, cls)
    assert BN is not None and (1 << (OY.bit_length() - 1)) == OY and (1 << (OX.bit_length() - 1)) == OX, (c.name, call)
    nst = min(ldo, r8(N)) if (N & 7 and not cls) else N
    out = set()
    for n0 in range(0, N, BN):
        ncols = min(BN, nst - n0)
        if ncols * 4 % 16:
            out.add("general8")
        elif ncols < BN:
            out.add("general16")
        else:
            # a tile holds NB = rows / (OY * OX) images when the grid is smaller than the tile; the tile that reaches past the batch keeps the general
            # loop.  fp32 32-column launches below 300 workgroups run 128-row tiles, else either height (it changes nothing for 16 x 16 grids)
            for rows in ((128,) if BN == 32 and -(-B * OY * OX // 256) * (N // BN) < 300 else (128, 256)):
                nb = max(1, rows // (OY * OX))
                if B >= nb:
                    out.add("fast")
                if B % nb:
                    out.add("general16")
    return out


def test_cases_plan_onto_the_branches_they_name():
    for c, calls in CASES:
        for call, want in calls.items():
            assert store_plan(c, "dgrad" if call == "dgrad_masked" else call) == want, (c.name, call)
    named = set().union(*[b for _, calls in CASES for b in calls.values()])
    assert named == {"fast", "general16", "general8"}


# ---------------------------------------------------------------- calls into a guarded allocation
def _guarded(shape):
    n = 1
    for s in shape:
        n *= s
    full = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    return full, full[GUARD:GUARD + n].view(shape)


def _check(L, full, got, ref, C_, ld, what):
    """guards untouched, real channels against fp64, pad channels [C, r8(C)) zero, channels beyond r8(C) untouched"""
    nanbits = api._bits(torch.full((1,), float("nan"), dtype=torch.float32))[0].item()
    fb = api._bits(full)
    assert bool((fb[:GUARD] == nanbits).all()) and bool((fb[-GUARD:] == nanbits).all()), f"{L.c.name} {what}: wrote outside the tensor"
    g = got.double().cpu()
    scale = max(float(ref.abs().max()), 1e-6)
    torch.testing.assert_close(g[..., :C_], ref, rtol=F32_RTOL, atol=F32_ATOL * scale, msg=lambda m: f"{L.c.name} {what}: {m}")
    r8 = min(ld, api._r8(C_))
    assert bool((g[..., C_:r8] == 0).all()), f"{L.c.name} {what}: pad channels [{C_}, {r8}) not zero"
    assert bool((api._bits(got[..., r8:ld]) == nanbits).all()), f"{L.c.name} {what}: channels beyond r8(C) written"


def _mask_with_zeros(L):
    """the ReLU mask of the case with rows of +0, -0 and a denormal negative added (-> M: the CPU copy, device tensor)"""
    c = L.c
    M = (L.ML if c.ups else L.M).clone().float()
    M[:, 0] = 0.0
    M[:, 1] = -0.0
    M[:, 2] = -1e-40
    dev = torch.zeros(M.shape[:-1] + (L.ldx,), dtype=torch.float32)
    dev[..., :c.Cin] = M
    return M, dev[L.pidx].cuda()


def _launch(L, call, zeros=True):
    """one call into a guarded allocation -> (full allocation, output view, CPU copy of the mask or None)"""
    c, lib, d = L.c, L.lib, C.byref(L.d)
    p, st = api._p, api._st
    if call in ("fwd", "fwd_ws"):
        full, y = _guarded((c.B, L.OH, L.OW, L.ldy))
        n = lib.sv_conv2d_fwd_workspace_bytes(d) if call == "fwd_ws" else 0
        assert (n > 0) == (call == "fwd_ws")
        ws = torch.zeros((max(n, 1),), dtype=torch.uint8, device="cuda")
        assert lib.sv_conv2d_nhwc_fwd_ws(d, p(L.x), p(L.wf), p(L.b_dev), p(y), p(ws) if n else None, n, st()) == 0
        return full, y, None
    M, mask = _mask_with_zeros(L) if zeros else (None, L.mask_lo if c.ups else L.mask)
    if call in ("dgrad", "dgrad_masked"):
        full, dx = _guarded((c.B, c.H, c.W, L.ldx))
        masked = call == "dgrad_masked"
        assert lib.sv_conv2d_nhwc_dgrad(d, p(L.dy), p(L.wd), p(mask) if masked else None, p(dx), 0, st()) == 0
        return full, dx, M if masked else None
    assert call == "lowres_ws"
    full, dx = _guarded((c.B, L.hin, L.win, L.ldx))
    n = lib.sv_conv2d_dgrad_lowres_workspace_bytes(d)
    assert n > 0
    ws = torch.zeros((n,), dtype=torch.uint8, device="cuda")
    assert lib.sv_conv2d_nhwc_dgrad_lowres_ws(d, p(L.dy), p(L.wd), p(mask), p(dx), p(ws), n, st()) == 0
    return full, dx, M


def _reference(L, call, M):
    """-> (fp64 reference, real channels, pitch)"""
    c = L.c
    if call in ("fwd", "fwd_ws"):
        return api._ref_at(L, L.y_ref), c.Cout, L.ldy
    ref = (L.dxlo_ref if call == "lowres_ws" else L.dx_ref)[L.pidx]
    return (ref * (M[L.pidx].double() > 0) if M is not None else ref), c.Cin, L.ldx


@pytest.mark.gpu
@pytest.mark.parametrize("c,calls", CASES, ids=[c.name for c, _ in CASES])
def test_store_branches_against_fp64(lib_built, c, calls):
    L = api.Layer(c)
    for call in calls:
        full, got, M = _launch(L, call)
        ref, C_, ld = _reference(L, call, M)
        _check(L, full, got, ref, C_, ld, call)


# ---------------------------------------------------------------- the forms the table assumes
def trace_main():
    """child process (SV_TRACE_DISPATCH=1): every call of every case, each behind a marker line on stderr"""
    for c, calls in CASES:
        L = api.Layer(c, refs=False)
        for call in calls:
            sys.stderr.flush()
            os.write(2, f"call {c.name} {call}\n".encode())
            _launch(L, call, zeros=False)
            torch.cuda.synchronize()
    os.write(2, b"done\n")


@pytest.mark.gpu
def test_every_case_runs_the_form_its_branches_assume(lib_built):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "import sys; sys.path[:0] = [%r, %r]\nimport test_gpu_tile_epilogue as T\nT.trace_main()\n" % (root, os.path.join(root, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SV_TRACE_DISPATCH="1"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    got, key = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("call "):
            key = tuple(line.split()[1:3])
        elif line.startswith("sv_dispatch ") and key is not None:
            got.setdefault(key, []).append(line.split()[2])
    wrong = []
    for c, calls in CASES:
        for call in calls:
            want = FORMS[c.name]["dgrad" if call == "dgrad_masked" else call]
            if got.get((c.name, call)) != [want]:
                wrong.append(f"{c.name} {call}: expected {want}, took {got.get((c.name, call))}")
    assert not wrong, "\n".join(wrong)
