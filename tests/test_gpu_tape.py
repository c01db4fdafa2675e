"""GPU: the tape executor (csrc/tape.hip) node by node, and the exact-fp32 Dense kernels it launches (dense_f32.hip), against torch fp64.

Every tape case is a hand-built graph of 2 to 12 nodes (tests/tape_ref.py: CASES) run TWICE with different inputs; the second run's activations, tensor
gradients, flat variable gradients and loss block are compared with the float64 twin that interprets the same node list on the CPU.  One rule for every
compared tensor: e = |gpu - ref64| / |ref64| <= max(floor, 3 * e32), e32 = the float32 twin's own error against ref64; floor = 2e-6 (the Dense figure below),
or, for graphs built on the STN / renderer / z_pres kernels, the norm of the per-element bounds of tests/spair_glue_ref.py over the norm of the reference (conv kernels: tests/test_gpu_spair.py).  The assembled step is
under the oracle in tests/test_gpu_spair_model.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tape_ref as T  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(lib_built):
    assert torch.cuda.is_available()
    from split_vae_amd import ops as o
    return o


@pytest.mark.parametrize("M,K,N", [(32, 6912, 1024), (32, 1024, 6912), (512, 177, 64), (512, 64, 1), (512, 68, 128), (32, 500, 4), (512, 4096, 128),
                                   (7, 13, 5), (65, 33, 129)])
def test_dense_f32_matches_fp64(ops, M, K, N):
    """tf.keras.layers.Dense forward / input gradient / weight + bias gradient for SPLIT-SPAIR's shapes (spair/spair.py:135-154, :185-202,
    :424-467) and ragged ones: exact-fp32 MFMA vs fp64, 2e-6 relative (split-K sums reorder fp32 adds)."""
    g = torch.Generator().manual_seed(M * 7 + K + N)
    x = torch.randn(M, K, generator=g)
    w = torch.randn(K, N, generator=g) / np.sqrt(K)
    b = torch.randn(N, generator=g)
    dy = torch.randn(M, N, generator=g)
    xd, wd, bd, dyd = x.cuda(), w.cuda(), b.cuda(), dy.cuda()
    rel = lambda a, r: float((a.double().cpu() - r).norm() / r.norm().clamp_min(1e-30))
    y = ops.dense_f32_fwd(xd, wd, bd)
    assert rel(y, x.double() @ w.double() + b.double()) < 2e-6
    yr = ops.dense_f32_fwd(xd, wd, bd, act="relu")
    assert rel(yr, torch.relu(x.double() @ w.double() + b.double())) < 2e-6
    dx = ops.dense_f32_dgrad(dyd, wd)
    assert rel(dx, dy.double() @ w.double().T) < 2e-6
    acc = torch.ones(M, K, device="cuda")
    ops.dense_f32_dgrad(dyd, wd, out=acc)
    assert rel(acc, 1.0 + dy.double() @ w.double().T) < 2e-6
    dw, db = ops.dense_f32_wgrad(xd, dyd)
    assert rel(dw, x.double().T @ dy.double()) < 2e-6
    assert rel(db, dy.double().sum(0)) < 2e-6
    # row pitches wider than the logical width (tape tensors are padded to 4 floats)
    xp = torch.zeros(M, K + 3, device="cuda"); xp[:, :K] = xd
    assert rel(ops.dense_f32_fwd(xp[:, :K], wd, bd), x.double() @ w.double() + b.double()) < 2e-6


# ------------------------------------------------------------------------------------------------------------------- node-level parity
def _err(a, b):
    a, b = a.double().cpu(), b.double()
    nb = float(b.norm())
    d = float((a - b).norm())
    return d / nb if nb > 0 else d                                            # a zero reference wants an exact zero


class Report:
    """every compared figure of a case: printed before anything is asserted (pytest -s, or the failure message)"""

    def __init__(self, name, g):
        self.name, self.g, self.rows, self.bad = name, g, [], []

    def check(self, what, tid, gpu, ref, r32):
        e, e32 = _err(gpu, ref), _err(r32, ref)
        floor = self.g.floors.get((what, tid), self.g.floor)
        bound = max(floor, 3.0 * e32)
        ok = bool(torch.isfinite(gpu).all()) and e <= bound
        self.rows.append("%-5s %-28s %-4s e %.3e  e32 %.3e  bound %.3e" % ("ok" if ok else "FAIL", self.name, "%s%s" % (what, "" if tid is None else tid), e, e32, bound))
        if not ok:
            self.bad.append(self.rows[-1])

    def finish(self):
        print("\n".join(self.rows))
        assert not self.bad, "\n" + "\n".join(self.bad)


def _compare(rep, g, dev, ref, r32, grads=True):
    for i, t in enumerate(g.tens):
        rep.check("act", i, dev.act(i), ref.act[i], r32.act[i])
        if grads and t["grad"]:
            rep.check("grad", i, dev.grad(i), ref.grad[i], r32.grad[i])
    if grads:
        rep.check("vars", None, dev.pgrads[:ref.pgrad.numel()], ref.pgrad, r32.pgrad)
        for off, shape, _ in g.params:                                        # (and layer by layer: a small layer's error does not hide in the flat norm)
            k = int(np.prod(shape))
            rep.check("var", off, dev.pgrads[off:off + k], ref.pgrad[off:off + k], r32.pgrad[off:off + k])
    rep.check("loss", None, dev.loss_out, ref.loss_out, r32.loss_out)
    for j in range(1 + 2 * T.MAX_LOSS):
        if float(ref.loss_out[j]) != 0.0:
            rep.check("loss", j, dev.loss_out[j:j + 1], ref.loss_out[j:j + 1], r32.loss_out[j:j + 1])


def _pads_are_zero(g, dev):
    """columns cols .. ld of every tensor the case allocated with ld > cols: "pad columns stay zero for ever" (the conv kernels read them)"""
    for i, t in enumerate(g.tens):
        if t["root"] == i and t["ld"] > t["cols"]:
            pad = dev.act(i, full=True)[:, t["cols"]:]
            assert float(pad.abs().max()) == 0.0, ("pad columns of tensor", i, float(pad.abs().max()))


@pytest.mark.parametrize("name", sorted(T.CASES))
def test_tape_case_matches_fp64_twin(lib_built, name):
    """One graph of tests/tape_ref.py: run on inputs 1, then on inputs 2 -- nothing may lean on sv_tape_bind's zero fill or on the previous step -- and compare the
    second run with the float64 twin (rule: the module docstring).  Then a forward-only run on inputs 3: the loss block is that of inputs 3, every gradient buffer
    and the variable gradients are left as the second run wrote them.  Pad columns are still exactly zero at the end.

    Measured on MI355X, worst e over all cases against its bound: see LAB_NOTES.md, "Tape executor: node-level parity"."""
    g = T.CASES[name]()
    dev = T.Device(g)
    runs = [g.make_inputs(s) for s in (1, 2, 3)]
    assert dev.run(*runs[0]) == 0
    assert dev.run(*runs[1]) == 0
    ref, r32 = (T.run_twin(g, runs[1][0], runs[1][1], dt) for dt in (torch.float64, torch.float32))
    rep = Report(name, g)
    _compare(rep, g, dev, ref, r32)
    _pads_are_zero(g, dev)
    before, pbefore = dev.grad_region(), dev.pgrads.clone()
    assert dev.run(*runs[2], backward=False) == 0
    ref, r32 = (T.run_twin(g, runs[2][0], runs[2][1], dt, backward=False) for dt in (torch.float64, torch.float32))
    _compare(rep, g, dev, ref, r32, grads=False)
    assert all(torch.equal(a, b) for a, b in zip(before, dev.grad_region())) and torch.equal(pbefore, dev.pgrads), "a forward-only run wrote a gradient"
    _pads_are_zero(g, dev)
    rep.finish()


def test_metrics_accumulate_over_two_runs(lib_built):
    """accumulate_metrics: the metric block holds the running sums of [total, reported] and the count, over the runs that ask for it only."""
    g = T.CASES["loss_modes_Rn64"]()
    dev = T.Device(g)
    outs = []
    for seed, acc in ((1, 1), (2, 0), (3, 1)):
        assert dev.run(*g.make_inputs(seed), accumulate=acc) == 0
        outs.append(dev.loss_out.double().cpu().clone())
    m = dev.metric.double().cpu()
    want = outs[0] + outs[2]
    nrep = len(g.report)
    assert torch.allclose(m[:1 + nrep], want[:1 + nrep], rtol=1e-6, atol=0) and float(m[1 + T.MAX_LOSS]) == 2.0
    assert float(m[1 + nrep:1 + T.MAX_LOSS].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------------------- lanes
def _snapshot(g, dev):
    out = [dev.act(i, full=True).clone() for i, t in enumerate(g.tens) if t["root"] == i]
    return out + dev.grad_region() + [dev.pgrads.clone(), dev.loss_out.clone()]


def test_lanes_compute_the_single_stream_tape_bit_for_bit(lib_built):
    """A fork of two Dense -> in-place-activation chains joined by a concat group, two LOSS nodes and a NOISE node (fixed-order kernels only), recorded with every
    node on lane 0 and with a seeded pseudo-random lane 0..3 per node (the default cap folds them onto one extra stream).  The single-lane tape is bit-identical
    over two runs; the lane run equals it bit for bit, activations and gradients: what csrc/tape.hip's header promises."""
    g0 = T.lanes_graph(None)
    ins, p = g0.make_inputs(4)
    d0 = T.Device(g0)
    kw = dict(pinned=0, seed=11, step=3)
    assert d0.run(ins, p, **kw) == 0
    a = _snapshot(g0, d0)
    assert d0.run(g0.make_inputs(5)[0], p, **kw) == 0                       # (other inputs in between)
    assert d0.run(ins, p, **kw) == 0
    b = _snapshot(g0, d0)
    assert all(torch.equal(x, y) for x, y in zip(a, b)), "the single-lane tape is not run-to-run identical"
    assert float(a[-2].abs().sum()) > 0
    for seed in (1, 2, 3):
        g1 = T.lanes_graph(seed)
        d1 = T.Device(g1)
        assert d1.run(g1.make_inputs(5)[0], p, **kw) == 0
        assert d1.run(ins, p, **kw) == 0
        c = _snapshot(g1, d1)
        bad = [k for k, (x, y) in enumerate(zip(a, c)) if not torch.equal(x, y)]
        assert not bad, ("lane assignment %d changes buffers" % seed, bad)


def test_conv_hand_off_computes_the_single_stream_tape_bit_for_bit(lib_built, deterministic):
    """The one PRE / WGRAD / DGRAD triple (T.conv_lanes_graph: a bf16 tape whose lane-0 ReLU conv hands its weight gradient to lane 1, where a second conv's weight
    gradient uses the same slab region), under fixed-order reductions.  The all-lane-0 recording is bit-identical over two runs; the two-lane recording equals it
    bit for bit in activations, gradient region, variable gradients and loss block."""
    g0 = T.conv_lanes_graph(False)
    ins, p = g0.make_inputs(4)
    d0 = T.Device(g0)
    assert [s[2] for s in d0.steps(1)] == [0] * 5                            # (loss, group, conv, conv, dense: whole adjoints)
    assert d0.run(ins, p) == 0
    a = _snapshot(g0, d0)
    assert d0.run(g0.make_inputs(5)[0], p) == 0                             # (other inputs in between)
    assert d0.run(ins, p) == 0
    b = _snapshot(g0, d0)
    assert all(torch.equal(x, y) for x, y in zip(a, b)), "the single-lane tape is not run-to-run identical"
    assert float(a[-2].abs().sum()) > 0
    g1 = T.conv_lanes_graph(True)
    d1 = T.Device(g1)
    assert [s[2:4] for s in d1.steps(1)][2:6] == [(0, 1), (1, 0), (2, 1), (3, 0)]      # conv on lane 1, then PRE / WGRAD (lane 1) / DGRAD of the lane-0 conv
    assert d1.run(g1.make_inputs(5)[0], p) == 0
    assert d1.run(ins, p) == 0
    c = _snapshot(g1, d1)
    bad = [k for k, (x, y) in enumerate(zip(a, c)) if not torch.equal(x, y)]
    assert not bad, ("the two-lane recording changes buffers", bad)


# ------------------------------------------------------------------------------------------------------------------- NOISE
def _noise_graph():
    g = T.Graph(2)
    u = g.tensor(7, 5, 8, grad=False)                                        # rows * cols = 35: a ragged tail, and pad columns
    nrm = g.tensor(7, 5, 8, grad=False)
    big = g.tensor(130, 4, 4, grad=False)                                    # more than one block of counters
    g.add(T.NOISE, y=u, op=1, p0=1.0, stream_id=4)
    g.add(T.NOISE, y=nrm, op=0, p0=0.01, stream_id=7)
    g.add(T.NOISE, y=big, op=0, p0=1.0, stream_id=4)
    g.add(T.NOISE, y=g.tensor(260, 4, 4, grad=False), op=1, p0=1.0, stream_id=9)
    return g


def test_noise_node_draws_match_the_philox_mirror(lib_built):
    """pinned_noise = 0.  Uniform draws bit for bit against a NumPy Philox4x32-10 mirror (counter {q, q >> 32, step, stream_id ^ (step >> 32) * 0x9E3779B9}, key =
    seed, value ((u >> 8) + 1) / 2^24); normal draws against Box-Muller in float64 from the same uniforms to 2e-5 * std absolute (|r| <= sqrt(2 * 24 * ln 2) ~ 5.8,
    ulp(2 pi) ~ 4.8e-7: about 3e-6 on the angle, plus a few ulp of the intrinsics; margin ~ x5), with the p0 scaling.  The ragged tail is written, the pad columns
    are not touched; (stream_id, step) key the draws; pinned_noise = 1 leaves the tensors alone."""
    g = _noise_graph()
    dev = T.Device(g)
    seed, step = 0x1234567890ABCDEF, (3 << 32) | 5
    p = torch.zeros(1)
    for i in range(4):
        dev.act(i, full=True).fill_(9.0)                                     # (sentinel, pad columns included)
    assert dev.run({}, p, backward=False, pinned=0, seed=seed, step=step) == 0
    got = [dev.act(i, full=True).cpu().clone() for i in range(4)]
    for i, (rows, cols) in ((0, (7, 5)), (3, (260, 4))):
        want, _ = T.noise_uniforms(rows * cols, seed, step, g.nodes[i]["stream_id"])
        assert np.array_equal(got[i][:, :cols].numpy().reshape(-1).view(np.uint32), want.view(np.uint32)), i
    for i, (rows, cols, std) in ((1, (7, 5, 0.01)), (2, (130, 4, 1.0))):
        want = T.noise_normals(rows * cols, seed, step, g.nodes[i]["stream_id"], std)
        err = np.abs(got[i][:, :cols].double().numpy().reshape(-1) - want).max()
        print("noise kind 0, std %g: max abs error %.3e (bound %.1e)" % (std, err, 2e-5 * std))
        assert err <= 2e-5 * std, (i, err)
    for i in (0, 1):
        assert bool((got[i][:, 5:] == 9.0).all()), "a NOISE node wrote pad columns"
    assert float(got[0][:, :5].min()) > 0.0 and float(got[0][:, :5].max()) <= 1.0
    # the same (seed, step) again: the same draws; another step, another stream: others
    assert dev.run({}, p, backward=False, pinned=0, seed=seed, step=step) == 0
    assert all(torch.equal(dev.act(i, full=True).cpu(), got[i]) for i in range(4))
    assert dev.run({}, p, backward=False, pinned=0, seed=seed, step=step + 1) == 0
    assert all(not torch.equal(dev.act(i).cpu(), got[i][:, :g.tens[i]["cols"]]) for i in range(4))
    assert not torch.equal(got[2][:7].reshape(-1)[:28] * 0.01, got[1][:, :5].reshape(-1)[:28])          # stream 4 against stream 7 at one step
    # pinned: the caller's values stay
    for i in range(4):
        dev.act(i, full=True).fill_(0.25)
    assert dev.run({}, p, backward=False, pinned=1, seed=seed, step=step) == 0
    assert all(bool((dev.act(i, full=True) == 0.25).all()) for i in range(4))
