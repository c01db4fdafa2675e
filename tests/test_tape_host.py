"""Host side of the tape executor (csrc/tape.hip), no GPU: the cross-lane schedule as a property over random tapes, and the CPU twin of tests/tape_ref.py
checked against the oracle functions it is built on (direct calls, torch.autograd.gradcheck) and over every case tests/test_gpu_tape.py runs on the device
(they record, and their float32 twin and float64 reference stay finite)."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import spair_model_ref as R
from oracle import spair_ref

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tape_ref as T  # noqa: E402


# ------------------------------------------------------------------------------------------------------------------- the schedule
def _random_tape(seed):
    """Dense, UNARY (in place, grouped and ungrouped), SAMPLE, LOSS and NOISE nodes over a pool of [8, c] tensors and their views, random fan-out and lanes"""
    rng = np.random.default_rng(seed)
    B, rows = 2, 8
    g = T.Graph(B)
    pick = lambda seq: seq[int(rng.integers(0, len(seq)))]
    lane = lambda: int(rng.integers(0, 4))
    pool = [g.tensor(rows, int(c), T.r4(int(c)), grad=bool(rng.integers(0, 4))) for c in rng.integers(4, 17, size=3)]
    same_rows = lambda r: [t for t in pool if g.tens[t]["rows"] == r]
    group = 0
    for _ in range(int(rng.integers(6, 22))):
        kind = pick(["dense", "dense", "unary", "inplace", "group", "sample", "loss", "noise", "view", "into"])
        x = pick(pool)
        tx = g.tens[x]
        if kind == "dense":
            pool.append(g.dense(x, int(rng.integers(2, 12)), bias=bool(rng.integers(0, 2)), act=int(rng.integers(0, 2)), grad=bool(rng.integers(0, 5)), lane=lane()))
        elif kind == "unary":
            n = int(rng.integers(1, tx["cols"] + 1))
            y = g.tensor(tx["rows"], n + 1, T.r4(n + 1), grad=bool(rng.integers(0, 5)))
            g.unary(int(rng.integers(0, 6)), x, y, n, xo=int(rng.integers(0, tx["cols"] - n + 1)), yo=int(rng.integers(0, 2)), p0=0.5, p1=0.9, lane=lane())
            pool.append(y)
        elif kind == "into":                      # out of place into columns of an EXISTING tensor (write after read / write after write)
            ys = [t for t in same_rows(tx["rows"]) if t != x]
            if not ys:
                continue
            y = pick(ys)
            n = int(rng.integers(1, min(tx["cols"], g.tens[y]["cols"]) + 1))
            g.unary(T.COPY, x, y, n, xo=0, yo=int(rng.integers(0, g.tens[y]["cols"] - n + 1)), lane=lane())
        elif kind == "inplace":
            n = int(rng.integers(1, tx["cols"] + 1))
            o = int(rng.integers(0, tx["cols"] - n + 1))
            g.unary(int(rng.integers(1, 6)), x, x, n, xo=o, yo=o, p0=0.5, p1=0.9, lane=lane())
        elif kind == "group":
            parts = int(rng.integers(2, 11))
            y = g.tensor(tx["rows"], 2 * parts, T.r4(2 * parts), grad=bool(rng.integers(0, 5)))
            group += 1
            ln = lane()
            srcs = same_rows(tx["rows"])
            for k in range(parts):
                s = pick(srcs)
                if bool(rng.integers(0, 6) == 0):
                    ln = lane()                    # a lane change cuts the group
                w = min(2, g.tens[s]["cols"])
                g.unary(T.COPY, s, y, w, xo=int(rng.integers(0, g.tens[s]["cols"] - w + 1)), yo=2 * k, group=group, lane=ln)
            pool.append(y)
        elif kind == "sample":
            c = same_rows(tx["rows"])
            m, s, e = pick(c), pick(c), pick(c)
            if not (g.tens[m]["grad"] and g.tens[s]["grad"]):
                continue                           # (the adjoint refuses a SAMPLE whose output has a gradient and whose mean / sig have none)
            n = int(rng.integers(1, min(g.tens[t]["cols"] for t in (m, s, e)) + 1))
            z = g.tensor(tx["rows"], n, T.r4(n))
            g.add(T.SAMPLE, x=m, t2=s, t3=e, y=z, n=n, lane=lane())
            pool.append(z)
        elif kind == "loss":
            if len(g.weights) >= T.MAX_LOSS or tx["rows"] % B:
                continue
            b = pick(same_rows(tx["rows"]))
            n = int(rng.integers(1, min(tx["cols"], g.tens[b]["cols"]) + 1))
            g.loss(int(rng.integers(0, 3)), x, 0, b, 0, n, 1.0, p1=0.5, lane=lane())
        elif kind == "noise":
            y = g.tensor(rows, 4, 4, grad=False)
            g.add(T.NOISE, y=y, op=int(rng.integers(0, 2)), p0=1.0, stream_id=len(g.nodes), lane=lane())
            pool.append(y)
        elif kind == "view":
            if tx["rows"] % 2 == 0 and tx["root"] == x:
                pool.append(g.view(x, tx["rows"] // 2, 2 * tx["ld"]))
    if not g.weights:
        g.loss(1, pool[0], 0, pool[0], 0, 1, 1.0)
    return g


def _units(g, lanes):
    """[first, last] node of every launch: consecutive UNARY nodes of one non-zero group and one lane, at most 8, are one launch (include/splitvae.h)"""
    u, i, N = [], 0, len(g.nodes)
    while i < N:
        n, e = g.nodes[i], i + 1
        if n["kind"] == T.UNARY and n["group"]:
            while e < N and e - i < T.MAX_PARTS and g.nodes[e]["kind"] == T.UNARY and g.nodes[e]["group"] == n["group"] and lanes[e] == lanes[i]:
                e += 1
        u.append((i, e - 1))
        i = e
    return u


ALL, PRE, WGRAD, DGRAD = range(4)


def _expected_steps(g, lanes, backward):
    """The step list (first, last, part, lane) as include/splitvae.h words it: forward, every unit is one ALL step on its lane.  Backward, the units in reverse; on a tape
    with more than one lane a lane-0 DENSE node (or a CONV node of a bf16 tape) whose input has a gradient is PRE on lane 0 (CONV only), WGRAD on lane 1, DGRAD on lane 0."""
    units = _units(g, lanes)
    if not backward:
        return [(a, b, ALL, lanes[a]) for a, b in units]
    out = []
    for a, b in reversed(units):
        n = g.nodes[a]
        layer = n["kind"] == T.DENSE or (n["kind"] == T.CONV and g.bf16)
        if not (layer and max(lanes) > 0 and lanes[a] == 0 and g.tens[n["x"]]["grad"]):
            out.append((a, b, ALL, lanes[a]))
            continue
        out += [(a, b, PRE, 0)] * (n["kind"] == T.CONV) + [(a, b, WGRAD, 1), (a, b, DGRAD, 0)]
    return out


def _access(g, i, part, lane, backward):
    """(reads, writes) of one node's part as resources ('A' | 'G', root tensor) / ('W', offset) / ('dY', node) / ('slab', lane), from the documented semantics of the
    node kinds: the forward pass reads input activations and writes outputs, LOSS / ZPRES add into their operands' gradients; the adjoint read-modify-writes the
    gradients it adds into, reads its output's gradient and writes its variables' gradients.  Of a DENSE / CONV adjoint, PRE gates G(y) in place and writes the bf16
    copy of dY, WGRAD reads both and writes the variables' gradients (CONV: through its lane's slab region), DGRAD reads both and adds into G(x); ALL is the three
    together.  Activations are only read backwards: never a conflict, left out."""
    tens, n = g.tens, g.nodes[i]
    A = lambda t: ("A", tens[t]["root"])
    G = lambda t: ("G", tens[t]["root"])
    hasg = lambda t: t >= 0 and tens[t]["grad"]
    k = n["kind"]
    rd, wr = set(), set()
    if not backward:
        ins = {T.DENSE: ["x"], T.CONV: ["x"], T.UNARY: ["x"], T.SAMPLE: ["x", "t2", "t3"], T.LOSS: ["x", "t2"], T.NOISE: []}[k]
        rd |= {A(n[f]) for f in ins}
        if k in (T.DENSE, T.CONV, T.UNARY, T.SAMPLE, T.NOISE):
            wr.add(A(n["y"]))
        if k == T.LOSS:
            wr |= {G(n[f]) for f in (["t2"] if n["mode"] == 0 else ["x", "t2"]) if hasg(n[f])}
        return rd, wr
    if k in (T.LOSS, T.NOISE) or not hasg(n["y"]):
        return rd, wr
    if k in (T.DENSE, T.CONV):
        dy = {G(n["y"])} | ({("dY", i)} if k == T.CONV and g.bf16 else set())
        if part in (ALL, PRE):
            wr |= dy
        else:
            rd |= dy
        if part in (ALL, WGRAD):
            wr.add(("W", n["w_off"]))
            if k == T.CONV:
                wr.add(("slab", lane))
        if part in (ALL, DGRAD) and hasg(n["x"]):
            wr.add(G(n["x"]))
    elif k == T.UNARY:
        if hasg(n["x"]):
            rd.add(G(n["y"]))
            wr.add(G(n["x"]))
    elif k == T.SAMPLE:
        rd.add(G(n["y"]))
        wr |= {G(n[f]) for f in ("x", "t2") if hasg(n[f])}
    return rd, wr


def _check_schedule(g, lanes, tag):
    """One tape: the library's step lists are the expected ones, waits point at earlier steps that record, and every pair of conflicting steps on different lanes has a
    happens-before path (wait edges plus same-lane issue order).  -> (cross-lane conflicts, those with a WGRAD step on one side)"""
    dev = T.Device(g, bind=False)
    crossed = with_wgrad = 0
    for p in (0, 1):
        steps = dev.steps(p)
        assert [s[:4] for s in steps] == _expected_steps(g, lanes, p == 1), (tag, p)
        before = []                                                      # step -> bit set of the steps that happen before it
        last_on_lane = {}
        acc = []
        for u, (a, b, part, ln, _, waits) in enumerate(steps):
            hb = 0
            if ln in last_on_lane:
                q = last_on_lane[ln]
                hb |= before[q] | (1 << q)
            for d in waits:
                assert 0 <= d < u, (tag, p, u, d, "waits for a step that is issued later")
                assert steps[d][4] == 1, (tag, p, d, "waited for, but no event is recorded behind it")
                hb |= before[d] | (1 << d)
            before.append(hb)
            last_on_lane[ln] = u
            rd, wr = set(), set()
            for i in range(a, b + 1):
                r_, w_ = _access(g, i, part, ln, p == 1)
                rd |= r_
                wr |= w_
            acc.append((rd, wr))
            for q in range(u):
                if steps[q][3] == ln:
                    continue
                qr, qw = acc[q]
                if (wr & (qr | qw)) or (rd & qw):
                    crossed += 1
                    with_wgrad += WGRAD in (part, steps[q][2])
                    assert (hb >> q) & 1, (tag, "backward" if p else "forward", "step", steps[u][:4], "is not ordered behind", steps[q][:4],
                                           sorted((wr & (qr | qw)) | (rd & qw)))
    return crossed, with_wgrad


@pytest.mark.parametrize("block", range(8))
def test_lane_schedule_orders_every_conflict(lib_built, block):
    """200 seeded random tapes (25 per block), each as recorded and with its lanes folded onto lanes 0 / 1 by the recording (the cap's own fold included).  The
    library's step lists equal the ones include/splitvae.h's wording gives -- the weight gradients handed to lane 1 are steps of their own --, and for every pair of
    steps on different lanes that touch one resource, one of them writing, the reported wait edges plus same-lane issue order contain a happens-before path from the
    earlier to the later, in both passes.  An event is recorded behind every step that is waited for, and waits point at steps issued earlier.
    Measured on the CPU (default cap 1): 4828 cross-lane conflicts over the 8 blocks, 85 of them with a WGRAD step (8 to 16 per block)."""
    if os.environ.get("SV_TAPE_LANES") == "0":
        pytest.skip("lanes are switched off in this environment")
    cap = int(os.environ.get("SV_TAPE_LANES", "1"))
    crossed = with_wgrad = 0
    for seed in range(block * 25, block * 25 + 25):
        g = _random_tape(seed)
        c, w = _check_schedule(g, [min(n["lane"], cap) for n in g.nodes], seed)          # lanes above the cap fold onto it
        crossed, with_wgrad = crossed + c, with_wgrad + w
        for n in g.nodes:                                                                  # kind "lanes folded by the cap": recorded 0 / 3, run as 0 / cap
            n["lane"] = 3 if n["lane"] >= 2 else 0
        c, w = _check_schedule(g, [min(n["lane"], cap) for n in g.nodes], (seed, "folded"))
        crossed, with_wgrad = crossed + c, with_wgrad + w
    print("cross-lane conflicts %d, with a WGRAD step %d" % (crossed, with_wgrad))
    assert crossed > 50, crossed                                             # the tapes do produce cross-lane conflicts
    assert with_wgrad > 0, with_wgrad                                        # ... and the handed-off weight gradients are among them


@pytest.mark.parametrize("name", sorted(T.CASES))
def test_single_lane_tape_has_plain_steps(lib_built, name):
    """Every graph of tests/test_gpu_tape.py, recorded on lane 0 alone: both passes report the units as SV_TAPE_PART_ALL steps on lane 0, with no waits and no
    records (a single-lane run records no event at all), the backward list being the forward one reversed."""
    g = T.CASES[name]()
    for n in g.nodes:
        n["lane"] = 0
    dev = T.Device(g, bind=False)
    fwd, bwd = dev.steps(0), dev.steps(1)
    assert fwd == [(a, b, ALL, 0, 0, []) for a, b in _units(g, [0] * len(g.nodes))]
    assert bwd == fwd[::-1]


def test_side_stream_failure_leaves_a_null_stream(lib_built):
    """sv_side_stream: an index outside 0 .. 2 is SV_E_BADARG with *stream NULL; index 0 gives either status 0 and a stream (a GPU) or a non-zero status and NULL
    (no GPU) -- never status 0 with the pointer left as it was."""
    import ctypes as C
    from split_vae_amd import _lib
    lib = _lib.load()
    for index in (-1, 3):
        h = C.c_void_p(0xdead)
        assert lib.sv_side_stream(index, C.byref(h)) == _lib.STATUS_BADARG and not h.value
    h = C.c_void_p(0xdead)
    rc = lib.sv_side_stream(0, C.byref(h))
    assert (rc == 0 and h.value not in (None, 0xdead)) or (rc != 0 and not h.value), (rc, h.value)
    assert lib.sv_side_stream(0, None) == _lib.STATUS_BADARG


# ------------------------------------------------------------------------------------------------------------------- the twin against the oracle
def _twin(name, seed=2, dtype=torch.float64):
    g = T.CASES[name]()
    ins, p = g.make_inputs(seed)
    return g, ins, p, T.run_twin(g, ins, p, dtype)


def test_twin_loss_nodes_are_the_oracle_functions():
    g, ins, p, r = _twin("loss_modes_Rn64")
    B, n = g.B, 4
    d = lambda t: ins[t].double()
    label, pred, m, sg = g.input_ids()
    means = r.loss_out[1 + T.MAX_LOSS:]
    img = lambda t: t.reshape(B, -1)
    assert torch.allclose(means[0], spair_ref.tf_mean_sum(img(R.xent_loss(d(label)[:, 1:1 + n], d(pred)[:, 2:2 + n]))), rtol=1e-12)
    assert torch.allclose(means[1], R.kl_divergence(img(d(m)[:, 1:1 + n]), img(d(sg)[:, 2:2 + n])), rtol=1e-12)
    full = lambda v: torch.full((B, 16 * n), v, dtype=torch.float64)
    assert torch.allclose(means[2], R.kl_divergence_two_gauss(img(d(m)[:, 1 + n:1 + 2 * n]), img(d(sg)[:, 1:1 + n]), full(3.7), full(0.5)), rtol=1e-12)
    assert torch.allclose(means[3], R.kl_divergence_two_gauss(img(d(m)[:, 1:1 + n]), img(d(sg)[:, 3:3 + n]), full(-1.3), full(0.8)), rtol=1e-12)
    w = torch.tensor(g.weights, dtype=torch.float64)
    assert torch.allclose(r.loss_out[0], (w * means[:5]).sum(), rtol=1e-12)
    rep = torch.tensor(g.report, dtype=torch.float64)
    assert torch.allclose(r.loss_out[1:5], rep @ means[:5], rtol=1e-12)


def test_twin_zpres_stn_render_nodes_are_the_oracle_functions():
    g, ins, p, r = _twin("zpres_node")
    logits, pre = (ins[i].double() for i in g.input_ids())
    sh = (g.B, 4, 4, 1)
    want = spair_ref.compute_z_pres_kl_yolo_air(torch.sigmoid(pre).reshape(sh), logits.reshape(sh), pre.reshape(sh), 0.1, 0.8)
    assert torch.allclose(r.loss_out[1 + T.MAX_LOSS], want, rtol=1e-9)
    g, ins, p, r = _twin("stn_glimpses_with_bbox")
    img, zw = (ins[i].double() for i in g.input_ids())
    out, bbox = spair_ref.stn_forward(img.reshape(2, 48, 48, 3), zw.reshape(2, 4, 4, 4), 32, 32, inverse=False)
    n = g.nodes[0]
    assert torch.equal(r.act[n["y"]], out.reshape(-1, 3)) and torch.equal(r.act[n["t3"]], bbox.reshape(-1, 4))
    g, ins, p, r = _twin("stn_inverse_with_bbox")
    obj, zw = (ins[i].double() for i in g.input_ids())
    out, bbox = spair_ref.stn_forward(obj.reshape(2, 16, 32, 32, 4), zw.reshape(2, 4, 4, 4), 48, 48, inverse=True)
    assert torch.equal(r.act[g.nodes[0]["y"]], out.reshape(-1, 4))
    for name, training in (("render_training_noise", True), ("render_test_time", False)):
        g, ins, p, r = _twin(name)
        n = g.nodes[0]
        v = lambda f, *s: ins[n[f]].double().reshape(*s)
        want = spair_ref.renderer(v("x", 2, 16, 48, 48, 4), v("t2", 2, 48, 48, 3), v("t3", 2, 4, 4, 1), v("t4", 2, 4, 4, 1), v("t5", 2, 4, 4, 1), training=training,
                                  noise=v("t6", 2, 16, 48, 48, 3) if training else None)
        assert torch.allclose(r.act[n["y"]], want.reshape(-1, 3), rtol=1e-12, atol=1e-14)


def test_twin_gradients_pass_gradcheck():
    """The float64 twin's autograd on one graph of the smooth nodes (Dense without ReLU, sigmoid / softplus / scale / copy, SAMPLE, LOGITNOISE, kl losses)."""
    B, rows = 2, 4
    g = T.Graph(B)
    x = g.tensor(rows, 5, 8)
    o = g.dense(x, 9)                                                         # [mean 0:3 | sig 3:6 | logits 6:9]
    g.unary(T.SOFTPLUS, o, o, 3, xo=3, yo=3, p0=-1.0)
    eps = g.tensor(rows, 3, 4, grad=False)
    z = g.tensor(rows, 3, 4)
    g.add(T.SAMPLE, x=o, xo=0, t2=o, o2=3, t3=eps, o3=0, y=z, yo=0, n=3)
    u = g.tensor(rows, 3, 4, grad=False, init=T.uniform(0.1, 0.9))
    pre = g.tensor(rows, 3, 4)
    g.add(T.LOGITNOISE, x=o, xo=6, t2=u, o2=0, y=pre, yo=0, n=3, p0=0.7)
    cat = g.tensor(rows * 2, 6, 8)
    g.unary(T.SIGMOID, pre, cat, 3, yo=3, rep=2, group=1)
    g.unary(T.SCALE, z, cat, 3, yo=0, rep=2, p0=0.6, group=1)
    g.kl(cat, 3, 0.8)
    g.loss(2, o, 0, o, 3, 3, 0.3, p0=0.4, p1=0.5)
    ins, p = g.make_inputs(5)

    def f(xv, pv):
        return T.run_twin(g, {**ins, x: xv}, pv, torch.float64, backward=False).total
    xv, pv = ins[x].double().requires_grad_(True), p.double().requires_grad_(True)
    assert torch.autograd.gradcheck(f, (xv, pv), eps=1e-6, atol=1e-7, rtol=1e-5)
    r = T.run_twin(g, ins, p, torch.float64)                                  # ... and the gradient buffers the twin reports are those
    gx, gp = torch.autograd.grad(f(xv, pv), (xv, pv))
    assert torch.allclose(r.grad[x], gx, rtol=1e-12, atol=1e-15) and torch.allclose(r.pgrad, gp, rtol=1e-12, atol=1e-15)


def rel(a, b):
    nb = float(b.double().norm())
    return float((a.double() - b.double()).norm()) / nb if nb > 0 else float(a.double().norm())


@pytest.mark.parametrize("name", sorted(T.CASES))
def test_gpu_cases_record_and_stay_finite(lib_built, name):
    """Every graph of tests/test_gpu_tape.py is accepted by sv_tape_add / sv_tape_finalize, and on the inputs of both of its runs the float64 reference and the
    float32 twin (losses, activations, gradients) are finite: a case whose float32 twin overflows would be a bad case, not a kernel finding."""
    g = T.CASES[name]()
    T.Device(g, bind=False)
    for seed in (1, 2):
        ins, p = g.make_inputs(seed)
        r64, r32 = T.run_twin(g, ins, p, torch.float64), T.run_twin(g, ins, p, torch.float32)
        for r in (r64, r32):
            assert bool(torch.isfinite(r.loss_out).all()) and bool(torch.isfinite(r.pgrad).all())
            assert all(bool(torch.isfinite(v).all()) for v in r.act.values())
            assert all(bool(torch.isfinite(v).all()) for v in r.grad.values() if v is not None)
        assert np.isfinite(rel(r32.loss_out, r64.loss_out)) and np.isfinite(rel(r32.pgrad, r64.pgrad))
        assert float(r64.pgrad.abs().sum()) + sum(float(v.abs().sum()) for v in r64.grad.values() if v is not None) > 0     # the adjoint has something to get wrong


def test_philox_mirror_known_answers():
    """Philox4x32-10 of Random123's known-answer file: zero counter and key; all-ones counter and key."""
    z = T.philox4x32_10(np.zeros((1, 4), np.uint32), 0)[0]
    assert [int(v) for v in z] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    f = T.philox4x32_10(np.full((1, 4), 0xFFFFFFFF, np.uint32), 0xFFFFFFFFFFFFFFFF)[0]
    assert [int(v) for v in f] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
