"""CPU: the C-ABI library builds for gfx950, loads, exports every symbol include/splitvae.h
declares, and validates arguments without touching a GPU (no compute calls here)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import np_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions():
    src = open(os.path.join(ROOT, "include", "splitvae.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(sv_[a-z0-9_]+)\s*\(", src)))


def test_header_and_binding_agree(lib_built):
    from split_vae_amd import _lib
    declared = header_functions()
    assert len(declared) >= 25
    assert sorted(_lib.SYMBOLS) == declared          # the ctypes table binds exactly the header's functions
    lib = _lib.load()
    for name in declared:
        assert hasattr(lib, name), name
    assert b"gfx950" in lib.sv_version()


def test_library_is_gfx950_code_object(lib_built):
    data = open(lib_built, "rb").read()
    assert b"gfx950" in data and b"tile_conv_kernel" in data and b"wgrad_tile_kernel" in data


def test_param_table_matches_reference_order(lib_built):
    from split_vae_amd import _lib, ops
    for H in (32, 64):
        desc = _lib.LGVaeDesc(8, H, H, 128, 128, _lib.SV_BF16, 40.0)
        table = ops.param_table(desc)
        want = np_ref.param_shapes(H, H)
        assert [n for n, _, _ in table] == [n for n, _ in want]
        assert [tuple(s) for _, _, s in table] == [tuple(s) for _, s in want]
        offs = [o for _, o, _ in table]
        assert offs == sorted(offs) and all(o % 4 == 0 for o in offs)      # 16-byte aligned tensors
        n = _lib.load().sv_lgvae_param_count(C.byref(desc))
        assert n >= sum(int(np.prod(s)) for _, s in want) and n % 4 == 0


def test_plan_geometry_without_gpu(lib_built):
    from split_vae_amd import _lib
    lib = _lib.load()
    desc = _lib.LGVaeDesc(512, 64, 64, 128, 128, _lib.SV_BF16, 120.0)
    h = C.c_void_p()
    assert lib.sv_lgvae_plan_create(C.byref(desc), C.byref(h)) == 0
    ws = lib.sv_lgvae_workspace_bytes(h)
    assert 1 << 30 < ws < 8 << 30           # ~1.6 GB of activations for B=512: fits 288 GB many times over
    off, nb = C.c_int64(), C.c_int64()
    assert lib.sv_lgvae_buffer(h, b"out6_x", C.byref(off), C.byref(nb)) == 0
    assert nb.value == 512 * 64 * 64 * 6 * 4 and off.value % 256 == 0
    assert lib.sv_lgvae_buffer(h, b"no_such_buffer", C.byref(off), C.byref(nb)) == _lib.STATUS_BADARG
    # stepping an unbound plan is refused, not undefined behaviour
    a = _lib.StepArgs()
    a.phases = _lib.PHASE_ALL
    assert lib.sv_lgvae_step(h, C.byref(a), None) == _lib.STATUS_STATE
    lib.sv_lgvae_plan_destroy(h)


def _layout_fixture():
    import json
    with open(os.path.join(ROOT, "tests", "golden", "plan_layout.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("kind,index", [("lgvae", i) for i in range(7)] + [("gm", i) for i in range(2)])
def test_workspace_layout_is_pinned(lib_built, kind, index):
    """The workspace layout of sv_lgvae_plan / sv_gm_encoder, buffer by buffer, against tests/golden/plan_layout.json (recorded by
    tests/golden/make_golden_plan_layout.py from the commit before the typed buffer tables): the workspace bytes, (offset, bytes) of every buffer
    name, and SV_E_BADARG for the names the mode lacks.  One buffer that moves, shrinks, appears or disappears fails here.  Host only."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden_plan_layout", os.path.join(ROOT, "tests", "golden", "make_golden_plan_layout.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    from split_vae_amd import _lib
    doc = _layout_fixture()
    assert re.fullmatch(r"[0-9a-f]{40}", doc["recorded_from_commit"])
    assert len(doc["lgvae"]) == len(gen.LGVAE_DESCS) == 7 and len(doc["gm"]) == len(gen.GM_DESCS) == 2
    want = doc[kind][index]
    descs, names, layout = (gen.LGVAE_DESCS, gen.LGVAE_NAMES, gen.lgvae_layout) if kind == "lgvae" else (gen.GM_DESCS, gen.GM_NAMES, gen.gm_layout)
    assert want["desc"] == list(descs[index]) and sorted(want["buffers"]) == sorted(names)
    got = layout(_lib.load(), descs[index])
    assert got["workspace_bytes"] == want["workspace_bytes"]
    for name in names:
        assert got["buffers"][name] == want["buffers"][name], name
    # nothing beside the fixture's buffers: they tile the workspace (256-byte granules) exactly
    present = [v for v in got["buffers"].values() if v != "absent"]
    assert sum((b + 255) // 256 * 256 for _, b in present) == got["workspace_bytes"]


def test_weight_image_sizes_are_pinned(lib_built):
    """sv_conv2d_wprep_elems (forward and input-gradient image) and the four conv workspace-size queries against tests/golden/wprep_elems.json
    (recorded by tests/golden/make_golden_wprep_elems.py from the commit before the weight-image layout table), entry by entry: every accepted
    descriptor of conv_domain_grid(), every case of tests/test_gpu_conv_api.py, the plan's nine layers at two shapes and both dtypes.  Host only."""
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("make_golden_wprep_elems", os.path.join(ROOT, "tests", "golden", "make_golden_wprep_elems.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    from split_vae_amd import _lib
    lib = _lib.load()
    with open(os.path.join(ROOT, "tests", "golden", "wprep_elems.json")) as f:
        doc = json.load(f)
    assert re.fullmatch(r"[0-9a-f]{40}", doc["recorded_from_commit"])
    # the grid: the same descriptors are accepted, and each answers what it answered
    want = gen.decode_grid(doc["grid"])
    descs = list(gen.grid_descs())
    assert len(want) == len(descs) and sum(w[0] != -1 for w in want) > 1000
    for i, d in enumerate(descs):
        got = gen.queries(lib, d)
        assert got == want[i], (i, d, got, want[i])
    # the named descriptors: the file's lists are the generator's lists, and every entry matches
    for key, descs in (("cases", gen.case_descs()), ("layers", gen.layer_descs())):
        descs = list(descs)
        assert [(e["name"], e["desc"]) for e in doc[key]] == [(n, d) for n, d in descs], key
        for e in doc[key]:
            assert gen.queries(lib, e["desc"]) == e["sizes"], (key, e["name"])
    assert len(doc["cases"]) >= 50 and len(doc["layers"]) == 36
    # the groups reach the forms the grid does not: polyphase images (forward workspace > 0) and the polyphase input gradient
    assert any(e["sizes"][2] > 0 for e in doc["cases"]) and any(e["sizes"][4] > 0 for e in doc["layers"])


@pytest.mark.parametrize("gl,ll,B", [(128, 128, 512), (64, 64, 64), (256, 256, 96), (128, 128, 70), (256, 128, 64)])
def test_latent_slab_workspace_covers_every_split(lib_built, gl, ll, B):
    """the K-slice slabs of the latent block (lat_ws_x / lat_ws_xh) are sized from the four launches' own (split, N) pairs; a slab
    set is [split][B][N] fp32 with split >= 1, so each buffer holds at least one slab of the widest problem.  (The plan accepts equal
    power-of-two latent sizes only -- sv_lgvae_plan_create refuses the last case -- so the over-run the advisor describes cannot be reached.)"""
    from split_vae_amd import _lib
    lib = _lib.load()
    desc = _lib.LGVaeDesc(B, 64, 64, gl, ll, _lib.SV_BF16, 120.0)
    h = C.c_void_p()
    rc = lib.sv_lgvae_plan_create(C.byref(desc), C.byref(h))
    if gl != ll:
        assert rc == _lib.STATUS_UNSUPPORTED
        return
    assert rc == 0
    off, nb = C.c_int64(), C.c_int64()
    for name in (b"lat_ws_x", b"lat_ws_xh"):
        assert lib.sv_lgvae_buffer(h, name, C.byref(off), C.byref(nb)) == 0
        assert nb.value >= B * max(2 * gl, 2 * ll, gl + ll) * 4 and off.value % 256 == 0
    lib.sv_lgvae_plan_destroy(h)


@pytest.mark.parametrize("bad", [dict(H=48), dict(H=64, W=32), dict(gl=100), dict(dtype=7), dict(B=0)])
def test_plan_rejects_unsupported(lib_built, bad):
    from split_vae_amd import _lib
    lib = _lib.load()
    H = bad.get("H", 64)
    desc = _lib.LGVaeDesc(bad.get("B", 8), H, bad.get("W", H), bad.get("gl", 128), 128, bad.get("dtype", 1), 1.0)
    h = C.c_void_p()
    assert lib.sv_lgvae_plan_create(C.byref(desc), C.byref(h)) < 0
    assert lib.sv_lgvae_param_count(C.byref(desc)) < 0


def test_kernel_entry_points_validate_arguments(lib_built):
    from split_vae_amd import _lib
    lib = _lib.load()
    assert lib.sv_scramble_gather(None, None, None, 1, 32, 32, 4, None) == _lib.STATUS_BADARG
    assert lib.sv_random_perm(None, 1, 16, 0, 0, 0, None) == _lib.STATUS_BADARG
    assert lib.sv_adam_step(None, None, None, None, 16, 1e-4, .9, .999, 1e-7, 1, 1.0, None) == _lib.STATUS_BADARG
    d = _lib.ConvDesc(4, 24, 24, 32, 32, 4, 4, 1, 0, 1, 32, 32, 0)       # 24: not a power of two -> im2col kernels (SPLIT-SPAIR backbone)
    assert lib.sv_conv2d_wprep_elems(C.byref(d), 0) == 32 * 16 * 32
    d = _lib.ConvDesc(4, 50, 50, 32, 32, 4, 4, 3, 0, 1, 32, 32, 0)       # a stride that does not divide the extent
    assert lib.sv_conv2d_wprep_elems(C.byref(d), 0) < 0
    d = _lib.ConvDesc(4, 48, 48, 32, 32, 4, 4, 4, 0, 1, 32, 32, 0)       # strides 1..3
    assert lib.sv_conv2d_wprep_elems(C.byref(d), 0) < 0
    d = _lib.ConvDesc(4, 32, 32, 32, 6, 6, 6, 1, 0, 1, 32, 6, 1)
    # bf16 head (Cout 6): the x-pixel-packed image, 16 columns (2 pixels x 8) x 6x7 taps x Cin
    assert lib.sv_conv2d_wprep_elems(C.byref(d), 0) == 16 * 42 * 32
    d32 = _lib.ConvDesc(4, 32, 32, 32, 6, 6, 6, 1, 0, 0, 32, 6, 1)           # fp32 (the reference's precision): the same x-packed image since round 4
    assert lib.sv_conv2d_wprep_elems(C.byref(d32), 0) == 16 * 42 * 32
    assert lib.sv_conv2d_wprep_elems(C.byref(d), 1) == 32 * 36 * 8        # dgrad contracts over Cout padded to 8
    assert lib.sv_dlogistic_nll_workspace_bytes(8, 64, 64) == 8 * 4 * 4
    # the two-network loss launch and the loss finaliser: null arguments are refused before any launch (the rest: tests/test_pointwise_host.py)
    assert lib.sv_dlogistic_nll_twin(None, None, 0, None, 0, None, 0, 0, 1.0, 1, 32, 32, None, 0, None) == _lib.STATUS_BADARG
    assert lib.sv_finalize_losses(None, None, None, None, None, None, 0, 4, 40.0, None, None, 0, None) == _lib.STATUS_BADARG


def test_missing_library_fails_loudly(tmp_path, monkeypatch):
    """The product path must not fall back to anything when the HIP extension is absent."""
    from split_vae_amd import _lib
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    monkeypatch.setattr(_lib, "_lib", None)
    with pytest.raises(_lib.SplitVaeError):
        _lib.load()


def test_tape_host_logic_without_gpu(lib_built):
    """sv_tape_*: recording, argument checks, workspace layout -- pure host code (also what scripts/asan_host.sh runs under ASan + UBSan)."""
    from split_vae_amd import _lib
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.sv_tape_create(C.byref(h), 0, _lib.SV_F32) == _lib.STATUS_BADARG
    assert lib.sv_tape_create(C.byref(h), 4, 7) == _lib.STATUS_BADARG
    assert lib.sv_tape_create(C.byref(h), 4, _lib.SV_F32) == 0
    x = lib.sv_tape_tensor(h, 64, 177, 180, 0)
    y = lib.sv_tape_tensor(h, 64, 64, 64, 1)
    z = lib.sv_tape_tensor(h, 64, 10, 12, 1)
    assert (x, y, z) == (0, 1, 2)
    assert lib.sv_tape_tensor(h, 64, 10, 8, 1) == _lib.STATUS_BADARG            # pitch below the width
    v = lib.sv_tape_view(h, y, 4, 1024, 1024)
    assert v == 3 and lib.sv_tape_view(h, y, 4, 2048, 2048) == _lib.STATUS_BADARG  # a view cannot outgrow its storage

    def node(kind, **kw):
        n = _lib.TapeNode()
        for f in ("x", "y", "t2", "t3", "t4", "t5", "t6"):
            setattr(n, f, -1)
        n.w_off = n.b_off = -1
        n.dyn_idx = n.loss_idx = -1
        n.rep, n.kind = 1, kind
        for k, val in kw.items():
            setattr(n, k, val)
        return lib.sv_tape_add(h, C.byref(n))

    assert node(_lib.TAPE_DENSE, x=x, y=y, w_off=0, b_off=177 * 64, act=_lib.SV_ACT_RELU) == 0
    assert node(_lib.TAPE_DENSE, x=x, y=y, w_off=-1) == _lib.STATUS_BADARG        # a Dense layer without a kernel
    assert node(_lib.TAPE_DENSE, x=y, y=z, w_off=12000, b_off=12640) == 0
    assert node(_lib.TAPE_UNARY, op=_lib.TAPE_SOFTPLUS, x=z, y=z, xo=1, yo=1, n=1) == 0
    assert node(_lib.TAPE_UNARY, op=_lib.TAPE_COPY, x=z, y=y, xo=0, yo=60, n=10) == _lib.STATUS_BADARG     # columns 60..69 of a 64-wide tensor
    assert node(_lib.TAPE_UNARY, op=99, x=z, y=z, n=1) == _lib.STATUS_BADARG
    assert node(_lib.TAPE_LOSS, loss_idx=0, mode=1, x=z, xo=0, t2=z, o2=1, R=16, n=1) == 0
    assert node(_lib.TAPE_LOSS, loss_idx=16, mode=1, x=z, t2=z, R=16, n=1) == _lib.STATUS_BADARG          # 16 loss slots
    assert node(_lib.TAPE_CONV, x=x, y=y, w_off=0, b_off=0, B=1, H=8, W=8, C=177, Cout=64, k=3, stride=1) != 0   # 177 channels: no conv geometry
    assert node(99) == _lib.STATUS_BADARG
    assert lib.sv_tape_workspace_bytes(h) == -1                                  # not finalized yet
    rep = (C.c_float * 16)(*([1.0] + [0.0] * 15))
    assert lib.sv_tape_set_report(h, rep, 1) == 0 and lib.sv_tape_set_report(h, rep, 17) == _lib.STATUS_BADARG
    assert lib.sv_tape_finalize(h) == 0 and lib.sv_tape_finalize(h) == _lib.STATUS_BADARG
    ws = lib.sv_tape_workspace_bytes(h)
    assert ws > 64 * (180 + 64 + 12) * 4 and ws % 256 == 0
    off, goff = C.c_int64(), C.c_int64()
    assert lib.sv_tape_tensor_info(h, x, C.byref(off), C.byref(goff)) == 0 and goff.value == -1 and off.value % 256 == 0
    assert lib.sv_tape_tensor_info(h, v, C.byref(off), C.byref(goff)) == 0 and goff.value >= 0
    assert lib.sv_tape_tensor_info(h, 9, None, None) == _lib.STATUS_BADARG
    assert lib.sv_tape_bind(h, None, ws, None) == _lib.STATUS_BADARG
    assert lib.sv_tape_run(h, None, None) == _lib.STATUS_BADARG
    lib.sv_tape_destroy(h)


def test_tape_with_conv_layers_reserves_the_weight_gradient_slabs(lib_built):
    """A tape that holds a Conv2D node reserves sv_conv2d_wgrad_workspace_bytes for the LDS-tile weight gradients' partial-sum slabs (one region,
    shared by its layers in stream order); a tape of Dense layers only does not.  Host logic: no GPU."""
    from split_vae_amd import _lib
    lib = _lib.load()

    def build(with_conv):
        h = C.c_void_p()
        assert lib.sv_tape_create(C.byref(h), 4, _lib.SV_F32) == 0
        x = lib.sv_tape_tensor(h, 4 * 16 * 16, 32, 32, 0)
        y = lib.sv_tape_tensor(h, 4 * 16 * 16, 32, 32, 1)
        n = _lib.TapeNode()
        for f in ("x", "y", "t2", "t3", "t4", "t5", "t6"):
            setattr(n, f, -1)
        n.dyn_idx = n.loss_idx = -1
        n.rep = 1
        n.x, n.y, n.w_off = x, y, 0
        if with_conv:
            n.kind, n.b_off = _lib.TAPE_CONV, 3 * 3 * 32 * 32
            n.B, n.H, n.W, n.C, n.Cout, n.k, n.stride = 4, 16, 16, 32, 32, 3, 1
        else:
            n.kind, n.b_off = _lib.TAPE_DENSE, 32 * 32
        assert lib.sv_tape_add(h, C.byref(n)) == 0
        assert lib.sv_tape_finalize(h) == 0
        ws = lib.sv_tape_workspace_bytes(h)
        lib.sv_tape_destroy(h)
        return ws

    d = _lib.ConvDesc()
    d.B, d.H, d.W, d.Cin, d.Cout, d.KH, d.KW, d.stride = 4, 16, 16, 32, 32, 3, 3, 1
    d.dtype, d.ldx, d.ldy = _lib.SV_F32, 32, 32
    slabs = lib.sv_conv2d_wgrad_workspace_bytes(C.byref(d))
    assert slabs > 0
    assert build(True) >= slabs and build(False) < slabs


def test_tape_lane_schedule_without_gpu(lib_built):
    """The step lists sv_tape_finalize builds and the cross-lane dependencies it derives from what the steps touch (csrc/tape.hip: build_steps, build_schedules), on a
    diamond: x -> A (lane 0) -> ya, x -> B (lane 1) -> yb, C (lane 0) = concat(ya, yb) -> z, loss on z.  Forward: C waits for B (read-after-write across lanes),
    nothing else crosses.  Backward (reverse order: loss, C, B, A): B (lane 1) waits for C's adjoint -- it wrote grad(yb) --; A is a lane-0 Dense whose input has a
    gradient, so its weight gradient is a step on lane 1 and its input gradient a step on lane 0, which waits for B: both ADD into grad(x), and conflicting
    accumulations keep the tape's order.  A's weight gradient reads grad(ya), last written by C on lane 0: lane 1 already waited for C (B did), so it waits for
    nothing.  Pure host code: no GPU."""
    import ctypes as C
    from split_vae_amd import _lib
    lib = _lib.load()
    if os.environ.get("SV_TAPE_LANES") == "0":
        pytest.skip("lanes are switched off in this environment")
    h = C.c_void_p()
    assert lib.sv_tape_create(C.byref(h), 4, _lib.SV_F32) == 0
    x = lib.sv_tape_tensor(h, 16, 32, 32, 1)
    ya = lib.sv_tape_tensor(h, 16, 8, 8, 1)
    yb = lib.sv_tape_tensor(h, 16, 8, 8, 1)
    z = lib.sv_tape_tensor(h, 16, 16, 16, 1)

    def node(tape, kind, **kw):
        n = _lib.TapeNode()
        for f in ("x", "y", "t2", "t3", "t4", "t5", "t6"):
            setattr(n, f, -1)
        n.w_off = n.b_off = -1
        n.dyn_idx = n.loss_idx = -1
        n.rep, n.kind = 1, kind
        for k, val in kw.items():
            setattr(n, k, val)
        assert lib.sv_tape_add(tape, C.byref(n)) == 0

    node(h, _lib.TAPE_DENSE, x=x, y=ya, w_off=0, b_off=256, lane=0)                      # node 0: A
    node(h, _lib.TAPE_DENSE, x=x, y=yb, w_off=512, b_off=768, lane=1)                    # node 1: B
    node(h, _lib.TAPE_UNARY, op=_lib.TAPE_COPY, x=ya, y=z, xo=0, yo=0, n=8, group=1)     # nodes 2, 3: C = one launch (a group)
    node(h, _lib.TAPE_UNARY, op=_lib.TAPE_COPY, x=yb, y=z, xo=0, yo=8, n=8, group=1)
    node(h, _lib.TAPE_LOSS, loss_idx=0, mode=1, x=z, xo=0, t2=z, o2=8, R=4, n=8)         # node 4
    bad = _lib.TapeNode()
    bad.kind, bad.x, bad.y, bad.lane = _lib.TAPE_UNARY, z, z, 9
    assert lib.sv_tape_add(h, C.byref(bad)) == _lib.STATUS_BADARG                     # lanes 0 .. 3
    one = _lib.TapeStep()
    assert lib.sv_tape_steps(h, 0) == _lib.STATUS_BADARG and lib.sv_tape_step_info(h, 0, 0, C.byref(one), None, 0) == _lib.STATUS_BADARG      # not finalized
    assert lib.sv_tape_finalize(h) == 0

    def steps(p):
        out = []
        for k in range(lib.sv_tape_steps(h, p)):
            s, w = _lib.TapeStep(), (C.c_int32 * 8)()
            assert lib.sv_tape_step_info(h, p, k, C.byref(s), w, 8) == 0
            out.append((s.first, s.last, s.part, s.lane, s.records, sorted(w[i] for i in range(s.n_waits))))
        return out

    ALL, WGRAD, DGRAD = _lib.TAPE_PART_ALL, _lib.TAPE_PART_WGRAD, _lib.TAPE_PART_DGRAD
    # forward: A, B, the group C as one step, the loss.  B waits for nothing (x is an input) and records; C (step 2) waits for B's event; nobody else waits or records
    assert steps(0) == [(0, 0, ALL, 0, 0, []), (1, 1, ALL, 1, 1, []), (2, 3, ALL, 0, 0, [1]), (4, 4, ALL, 0, 0, [])]
    # backward: loss, C (records: B waits for it), B (records), A's weight gradient on lane 1 (lane 1 waited for C already: nothing), A's input gradient, which waits for B
    assert steps(1) == [(4, 4, ALL, 0, 0, []), (2, 3, ALL, 0, 1, []), (1, 1, ALL, 1, 1, [1]), (0, 0, WGRAD, 1, 0, []), (0, 0, DGRAD, 0, 0, [2])]
    assert lib.sv_tape_steps(h, 2) == _lib.STATUS_BADARG and lib.sv_tape_step_info(h, 2, 0, C.byref(one), None, 0) == _lib.STATUS_BADARG
    assert lib.sv_tape_step_info(h, 0, 4, C.byref(one), None, 0) == _lib.STATUS_BADARG and lib.sv_tape_step_info(h, 1, 5, C.byref(one), None, 0) == _lib.STATUS_BADARG
    assert lib.sv_tape_step_info(h, 0, -1, C.byref(one), None, 0) == _lib.STATUS_BADARG
    lib.sv_tape_destroy(h)
    # every variable has one writer: a second layer on the same weights (or the same bias) is refused at finalize
    for second in (dict(w_off=0, b_off=768), dict(w_off=512, b_off=256)):
        h = C.c_void_p()
        assert lib.sv_tape_create(C.byref(h), 4, _lib.SV_F32) == 0
        x = lib.sv_tape_tensor(h, 16, 32, 32, 0)
        ya = lib.sv_tape_tensor(h, 16, 8, 8, 1)
        yb = lib.sv_tape_tensor(h, 16, 8, 8, 1)
        node(h, _lib.TAPE_DENSE, x=x, y=ya, w_off=0, b_off=256)
        node(h, _lib.TAPE_DENSE, x=x, y=yb, **second)
        assert lib.sv_tape_finalize(h) == _lib.STATUS_UNSUPPORTED
        lib.sv_tape_destroy(h)


def _conv_domain_rule(B, H, W, Cin, Cout, KH, KW, s, dtype, ldx, ldy, y_f32, ups):
    """include/splitvae.h's accepted domain of sv_conv_desc, as worded there: 0, SV_E_BADARG (-1) or SV_E_UNSUPPORTED (-2)"""
    if min(B, H, W, Cin, Cout, KH, KW) <= 0 or dtype not in (0, 1):
        return -1
    if s not in (1, 2, 3) or KH * KW > 81:
        return -2
    if s > 1 and (H % s or W % s):
        return -2
    if ldx < Cin or ldx % 8:
        return -1
    r8 = (Cin + 7) // 8 * 8
    if r8 & (r8 - 1):
        return -2
    if ldy < Cout or (not y_f32 and ldy % 8):
        return -1
    if ups and (s != 1 or H % 2 or W % 2):
        return -2
    OH, OW = -(-H // s), -(-W // s)
    if B * H * W * ldx >= 1 << 31 or B * OH * OW * ((Cout + 7) // 8 * 8) >= 1 << 31:
        return -2
    return 0


def conv_domain_grid():
    """the descriptors of test_conv_accepted_domain_matches_the_header, in a fixed order (tests/golden/make_golden_wprep_elems.py walks them too)"""
    import itertools
    grid = itertools.product((1, 3), ((16, 16), (16, 32), (12, 20), (24, 12), (15, 16), (1, 1)), (1, 3, 5, 12, 17, 30, 60), (1, 6, 10, 48),
                             ((3, 3), (3, 5), (6, 6), (9, 10)), (1, 2, 3, 4), (0, 1), (0, 8, 12), (0, 1), (0, 1))
    for B, (H, W), Cin, Cout, (KH, KW), s, dtype, ldx_over, y_f32, ups in grid:
        ldx = (Cin + 7) // 8 * 8 + ldx_over
        ldy = Cout if y_f32 else (Cout + 7) // 8 * 8
        yield B, H, W, Cin, Cout, KH, KW, s, dtype, ldx, ldy, y_f32, ups


def test_conv_accepted_domain_matches_the_header(lib_built):
    """host-only queries (no device work): a grid of descriptors through sv_conv2d_wprep_elems / the workspace-size queries, which answer
    -1 exactly for the descriptors the header's rule refuses, against a Python statement of that rule"""
    from split_vae_amd import _lib
    lib = _lib.load()
    n = 0
    for B, H, W, Cin, Cout, KH, KW, s, dtype, ldx, ldy, y_f32, ups in conv_domain_grid():
        d = _lib.ConvDesc(B, H, W, Cin, Cout, KH, KW, s, 0, dtype, ldx, ldy, y_f32, ups)
        ok = _conv_domain_rule(B, H, W, Cin, Cout, KH, KW, s, dtype, ldx, ldy, y_f32, ups) == 0
        got = [lib.sv_conv2d_wprep_elems(C.byref(d), 0), lib.sv_conv2d_wprep_elems(C.byref(d), 1), lib.sv_conv2d_fwd_workspace_bytes(C.byref(d)),
               lib.sv_conv2d_wgrad_workspace_bytes(C.byref(d)), lib.sv_conv2d_dgrad_lowres_workspace_bytes(C.byref(d)),
               lib.sv_conv2d_wgrad_poly_workspace_bytes(C.byref(d))]
        if ok:
            assert got[0] > 0 and got[1] > 0 and min(got[2:]) >= 0, (B, H, W, Cin, Cout, KH, KW, s, dtype, ldx, ldy, y_f32, ups, got)
        else:
            assert got == [-1] * 6, (B, H, W, Cin, Cout, KH, KW, s, dtype, ldx, ldy, y_f32, ups, got)
        n += ok
    assert n > 1000
    # malformed values the grid does not reach
    for kw in (dict(B=0), dict(Cin=0), dict(KH=0), dict(dtype=7), dict(ldy=4), dict(ldx=4)):
        f = dict(B=2, H=16, W=16, Cin=8, Cout=8, KH=3, KW=3, stride=1, act=0, dtype=1, ldx=8, ldy=8, y_f32=0, ups_in=0)
        f.update(kw)
        d = _lib.ConvDesc(*[f[k] for k in ("B", "H", "W", "Cin", "Cout", "KH", "KW", "stride", "act", "dtype", "ldx", "ldy", "y_f32", "ups_in")])
        assert lib.sv_conv2d_wprep_elems(C.byref(d), 0) == -1, kw
