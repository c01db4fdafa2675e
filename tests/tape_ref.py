"""The tape executor (include/splitvae.h: sv_tape_*, csrc/tape.hip) under test: a graph description, a recorder that plays it into the
library through ctypes, and a CPU twin that interprets the SAME node list with torch -- generic in dtype, gradients from torch.autograd.

  Graph      tensors / views / nodes / variables as plain Python data (no library call): what a test case is made of
  Twin       run_twin(graph, ..., dtype): every node as torch ops over column slices, total = sum_i w_i * mean_b loss_i, gradients of every
             tensor and of the flat variables from torch.autograd.grad.  float64 = the reference, float32 = how far fp32 rounding alone moves
             each result.  STN / RENDER / ZPRES / the safe-log losses are the restatements of oracle/spair_ref.py and oracle/spair_model_ref.py,
             upsample / conv those of oracle/torch_ref.py; UNARY / SAMPLE / LOGITNOISE are the formulas of csrc/tape.hip's header.
  Device     sv_tape_create .. sv_tape_run on the graph (needs the library, and a GPU to run)
  CASES      the hand-built graphs tests/test_gpu_tape.py runs on the device and tests/test_tape_host.py sanity-checks on the CPU

What a gradient buffer holds after the adjoint: d total / d (the FIRST value an element took) -- in-place nodes multiply the gradient where it lies, and a
convolution's ReLU gates its output gradient in place (so a CONV output's gradient is that of the pre-activation; a DENSE layer gates on load, its output's
gradient is that of the activation).  The twin gets exactly these from zero-valued probes added to every value where it is first written.
"""
import ctypes as C
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import spair_model_ref as R
from oracle import spair_ref, torch_ref

DENSE, CONV, UNARY, SAMPLE, LOGITNOISE, UPSAMPLE, STN, RENDER, ZPRES, LOSS, NOISE = range(11)      # include/splitvae.h: SV_TAPE_*
COPY, RELU, SIGMOID, SOFTPLUS, CLAMP, SCALE = range(6)
ACT_NONE, ACT_RELU = 0, 1
MAX_LOSS, MAX_PARTS = 16, 8
PHASE_FORWARD, PHASE_BACKWARD = 1, 2
TENSOR_FIELDS = ("x", "y", "t2", "t3", "t4", "t5", "t6")
INT_FIELDS = ("xo", "yo", "o2", "o3", "n", "rep", "op", "act", "B", "H", "W", "C", "Cout", "k", "stride", "Ho", "Wo", "Hc", "Wc", "inverse", "training",
              "loss_idx", "dyn_idx", "mode", "R", "stream_id", "group", "lane")


def r4(v):
    return (v + 3) // 4 * 4


def r8(v):
    return (v + 7) // 8 * 8


def _granule(t):
    return (t["rows"] * t["ld"] + 63) // 64 * 64


class Graph:
    """A tape as data.  Tensor ids and node indices are the library's (both count from 0 in recording order)."""

    def __init__(self, B, bf16=False):
        self.B, self.bf16 = B, bf16
        self.tens, self.nodes, self.params = [], [], []
        self.n_params = 0
        self.init = {}                 # tensor id -> f(generator, rows, cols) -> float32 [rows, cols]: the inputs' distributions (default: N(0, 1))
        self.weights = []              # loss weights, one per loss index
        self.dyn = [0.0] * 8
        self.report = None             # [n_report][n_loss] or None
        self.floor = 2e-6              # the relative-error floor of the comparison (2e-6: the project's Dense figure)
        self.floors = {}               # (what, tensor id) -> a floor of its own.  STN / renderer / z_pres graphs: |bound| / |reference| (2-norms) of the per-element
                                       # bounds of tests/spair_glue_ref.py at the graph's shapes and input distributions, evaluated on the CPU and rounded up -- or the
                                       # figure that stood here before where that was already the smaller one
        self.pad_exempt = set()

    # ---- recording
    def tensor(self, rows, cols, ld=None, grad=True, init=None):
        i = len(self.tens)
        self.tens.append(dict(rows=rows, cols=cols, ld=cols if ld is None else ld, grad=bool(grad), root=i))
        if init is not None:
            self.init[i] = init
        return i

    def view(self, src, rows, cols, ld=None):
        s = self.tens[src]
        assert rows * (cols if ld is None else ld) <= _granule(self.tens[s["root"]])
        self.tens.append(dict(rows=rows, cols=cols, ld=cols if ld is None else ld, grad=s["grad"], root=s["root"]))
        return len(self.tens) - 1

    def param(self, *shape, scale=None):
        off = self.n_params
        self.params.append((off, tuple(shape), scale))
        self.n_params += int(np.prod(shape))
        return off

    def add(self, kind, **kw):
        n = dict(kind=kind, p0=0.0, p1=0.0, w_off=-1, b_off=-1)
        for f in TENSOR_FIELDS:
            n[f] = -1
        for f in INT_FIELDS:
            n[f] = 0
        n["rep"], n["dyn_idx"], n["loss_idx"] = 1, -1, -1
        for k, v in kw.items():
            assert k in n, k
            n[k] = v
        self.nodes.append(n)
        return len(self.nodes) - 1

    def unary(self, op, x, y, n, xo=0, yo=0, **kw):
        return self.add(UNARY, op=op, x=x, y=y, n=n, xo=xo, yo=yo, **kw)

    def dense(self, x, N, bias=True, act=ACT_NONE, grad=True, lane=0):
        K = self.tens[x]["cols"]
        y = self.tensor(self.tens[x]["rows"], N, r4(N), grad=grad)
        self.add(DENSE, x=x, y=y, w_off=self.param(K, N, scale=1.0 / math.sqrt(K)), b_off=self.param(N) if bias else -1, act=act, lane=lane)
        return y

    def loss(self, mode, a, ao, b, bo, n, weight, R=None, **kw):
        idx = len(self.weights)
        self.weights.append(float(weight))
        R = self.tens[a]["rows"] // self.B if R is None else R
        self.add(LOSS, loss_idx=idx, mode=mode, x=a, xo=ao, t2=b, o2=bo, R=R, n=n, **kw)
        return idx

    def kl(self, t, n, weight, c0=0, **kw):
        """kl_divergence with columns [c0, c0 + n) as the mean and the next n as sig: what most cases hang their outputs on."""
        return self.loss(1, t, c0, t, c0 + n, n, weight, **kw)

    # ---- structure
    def written_roots(self, with_noise=False):
        w = set()
        for n in self.nodes:
            if n["kind"] in (ZPRES, LOSS) or (n["kind"] == NOISE and not with_noise):
                continue
            if n["kind"] == UNARY and n["x"] == n["y"] and n["xo"] == n["yo"]:
                continue                      # in place: the tensor needs a value from somewhere else
            w.add(self.tens[n["y"]]["root"])
            if n["kind"] == STN and n["t3"] >= 0:
                w.add(self.tens[n["t3"]]["root"])
        return w

    def input_ids(self):
        """Root tensors no node writes, but for in-place UNARY nodes and (pinned) NOISE nodes: the caller fills them."""
        w = self.written_roots()
        return [i for i, t in enumerate(self.tens) if t["root"] == i and i not in w]

    def make_inputs(self, seed):
        """-> ({tensor id: float32 [rows, cols]}, flat float32 variables) for one run."""
        g = torch.Generator().manual_seed(seed)
        ins = {}
        for i in self.input_ids():
            t = self.tens[i]
            f = self.init.get(i)
            ins[i] = (f(g, t["rows"], t["cols"]) if f else torch.randn(t["rows"], t["cols"], generator=g)).to(torch.float32).contiguous()
        p = torch.zeros(max(self.n_params, 1))
        for off, shape, scale in self.params:
            k = int(np.prod(shape))
            p[off:off + k] = torch.randn(k, generator=g) * (scale if scale is not None else 0.3)
        return ins, p


# ------------------------------------------------------------------------------------------------------------------- the twin
class _ConvBf16(torch.autograd.Function):
    """conv_dtype bf16: the convolution takes x, W and (backwards) dY rounded to bf16 and accumulates exactly -- the operands as the device sees them."""

    @staticmethod
    def forward(ctx, x, w, b, stride):
        rnd = lambda t: t.to(torch.bfloat16).to(t.dtype)
        ctx.save_for_backward(rnd(x), rnd(w))
        ctx.stride = stride
        return torch_ref.conv2d_same(rnd(x), rnd(w), b, stride, None)

    @staticmethod
    def backward(ctx, dy):
        xr, wr = ctx.saved_tensors
        dyr = dy.to(torch.bfloat16).to(dy.dtype)
        with torch.enable_grad():
            xr, wr = xr.detach().requires_grad_(True), wr.detach().requires_grad_(True)
            y = torch_ref.conv2d_same(xr, wr, None, ctx.stride, None)
            gx, gw = torch.autograd.grad(y, [xr, wr], dyr)
        return gx, gw, dyr.sum(dim=(0, 1, 2)), None


def _unary(op, v, p0, p1):
    if op == RELU:
        return torch.relu(v)
    if op == SIGMOID:
        return torch.sigmoid(v)
    if op == SOFTPLUS:
        return F.softplus(v + p0)
    if op == CLAMP:
        return torch.clamp(v, p0, p1)
    if op == SCALE:
        return v * p0
    return v * 1.0


class TwinResult:
    pass


def run_twin(g, inputs, params, dtype=torch.float64, backward=True):
    """Interpret graph `g` on the CPU.  -> TwinResult with act[id] / grad[id] ([rows, cols]; grad None without a gradient), pgrad (flat), loss_out
    ([1 + 2 * 16]: total, reported, means) and sums ([n_loss][B], the per-image sums)."""
    B, tens = g.B, g.tens
    P = params.to(dtype)
    if not P.requires_grad:                        # (a caller that differentiates the twin itself -- gradcheck -- passes its own leaves)
        P = P.clone().requires_grad_(True)
    flat, leaves, probes = {}, {}, []
    for i, t in enumerate(tens):
        if t["root"] == i:
            flat[i] = torch.zeros(_granule(t), dtype=dtype)

    def mat(tid, buf=None):
        t = tens[tid]
        b = flat[t["root"]] if buf is None else buf
        return b[:t["rows"] * t["ld"]].view(t["rows"], t["ld"])

    def read(tid, c0=0, n=None):
        assert c0 >= 0 and c0 + (tens[tid]["cols"] if n is None else n) <= tens[tid]["ld"], ("columns outside the tensor", tid, c0, n)
        return mat(tid)[:, c0:c0 + (tens[tid]["cols"] if n is None else n)]

    def write(tid, c0, val):
        buf = flat[tens[tid]["root"]].clone()
        mat(tid, buf)[:, c0:c0 + val.shape[1]] = val
        flat[tens[tid]["root"]] = buf

    def probe(tid, c0, val):
        """the value as it is first written to tensor tid: cut from the graph when the tensor carries no gradient, else with a probe for its gradient"""
        if not tens[tid]["grad"]:
            return val.detach()
        p = torch.zeros_like(val, requires_grad=True)
        probes.append((tid, c0, p))
        return val + p

    for i in g.input_ids():
        leaf = inputs[i].to(dtype)
        if not leaf.requires_grad:
            leaf = leaf.clone()
            if tens[i]["grad"]:
                leaf.requires_grad_(True)
        if leaf.requires_grad:
            leaves[i] = leaf
        write(i, 0, leaf)

    n_loss = len(g.weights)
    sums = [torch.zeros(B, dtype=dtype) for _ in range(n_loss)]
    per_image = lambda t: t.reshape(B, -1).sum(dim=1)
    for n in g.nodes:
        k = n["kind"]
        if k == DENSE:
            K, N = tens[n["x"]]["cols"], tens[n["y"]]["cols"]
            y = read(n["x"]) @ P[n["w_off"]:n["w_off"] + K * N].view(K, N)
            if n["b_off"] >= 0:
                y = y + P[n["b_off"]:n["b_off"] + N]
            write(n["y"], 0, probe(n["y"], 0, torch.relu(y) if n["act"] == ACT_RELU else y))
        elif k == CONV:
            Bc, H, W, Ci, Co, kk, s = (n[f] for f in ("B", "H", "W", "C", "Cout", "k", "stride"))
            x = mat(n["x"]).view(Bc, H, W, tens[n["x"]]["ld"])[..., :Ci]
            w = P[n["w_off"]:n["w_off"] + kk * kk * Ci * Co].view(kk, kk, Ci, Co)
            b = P[n["b_off"]:n["b_off"] + Co]
            y = _ConvBf16.apply(x, w, b, s) if g.bf16 else torch_ref.conv2d_same(x, w, b, s, None)
            y = probe(n["y"], 0, y.reshape(-1, Co))
            write(n["y"], 0, torch.relu(y) if n["act"] == ACT_RELU else y)
        elif k == UNARY:
            src = read(n["x"], n["xo"], n["n"]).repeat_interleave(n["rep"], dim=0)
            val = _unary(n["op"], src, n["p0"], n["p1"])
            inplace = n["x"] == n["y"] and n["xo"] == n["yo"]
            if inplace:
                val = val if tens[n["y"]]["grad"] else val.detach()
            write(n["y"], n["yo"], val if inplace else probe(n["y"], n["yo"], val))
        elif k == SAMPLE:
            val = read(n["x"], n["xo"], n["n"]) + read(n["t2"], n["o2"], n["n"]) * read(n["t3"], n["o3"], n["n"])
            write(n["y"], n["yo"], probe(n["y"], n["yo"], val))
        elif k == LOGITNOISE:
            u = read(n["t2"], n["o2"], n["n"])
            val = (read(n["x"], n["xo"], n["n"]) + (torch.log(u + 1e-8) - torch.log(1.0 - u + 1e-8))) / n["p0"]
            write(n["y"], n["yo"], probe(n["y"], n["yo"], val))
        elif k == UPSAMPLE:
            ld = tens[n["x"]]["ld"]
            y = torch_ref.resize_bilinear_2x(mat(n["x"]).view(n["B"], n["H"], n["W"], ld))
            write(n["y"], 0, probe(n["y"], 0, y.reshape(-1, ld)[:, :tens[n["y"]]["cols"]]))
        elif k == STN:
            Bs, cells, Cc = n["B"], n["Hc"] * n["Wc"], n["C"]
            img = read(n["x"]).reshape((Bs, cells, n["H"], n["W"], Cc) if n["inverse"] else (Bs, n["H"], n["W"], Cc))
            z = read(n["t2"]).reshape(Bs, n["Hc"], n["Wc"], 4)
            out, bbox = spair_ref.stn_forward(img, z, n["Ho"], n["Wo"], inverse=bool(n["inverse"]))
            write(n["y"], 0, probe(n["y"], 0, out.reshape(-1, Cc)))
            if n["t3"] >= 0:
                write(n["t3"], 0, bbox.reshape(-1, 4).detach())
        elif k == RENDER:
            Bs, Rr, H, W, Cc = n["B"], n["R"], n["H"], n["W"], n["C"]
            noise = read(n["t6"]).reshape(Bs, Rr, H, W, Cc) if (n["training"] and n["t6"] >= 0) else None
            out = spair_ref.renderer(read(n["x"]).reshape(Bs, Rr, H, W, Cc + 1), read(n["t2"]).reshape(Bs, H, W, Cc), read(n["t3"]).reshape(Bs, Rr, 1, 1),
                                     read(n["t4"]).reshape(Bs, Rr, 1, 1), read(n["t5"]).reshape(Bs, Rr, 1, 1), training=bool(n["training"]), noise=noise,
                                     num_channel=Cc)
            out = out.reshape(-1, Cc)
            write(n["y"], 0, probe(n["y"], 0, out if n["training"] else out.detach()))      # the test-time renderer (rounded z_pres) has no adjoint
        elif k == ZPRES:
            sh = (B, n["R"], 1, 1)
            kl = spair_ref.compute_z_pres_kl_yolo_air(read(n["x"]).detach().reshape(sh), read(n["t2"]).reshape(sh), read(n["t3"]).reshape(sh),
                                                      g.dyn[n["dyn_idx"]], n["p0"])
            # the oracle returns the batch mean of the per-image sums; the per-image sums themselves, for the loss block:
            sums[n["loss_idx"]] = _zpres_per_image(read(n["x"]).detach().reshape(sh), read(n["t2"]).reshape(sh), read(n["t3"]).reshape(sh),
                                                   g.dyn[n["dyn_idx"]], n["p0"], kl)
        elif k == LOSS:
            rows = B * n["R"]
            assert rows <= min(tens[n["x"]]["rows"], tens[n["t2"]]["rows"])
            a = read(n["x"], n["xo"], n["n"])[:rows]
            b = read(n["t2"], n["o2"], n["n"])[:rows]
            if n["mode"] == 0:
                t = R.xent_loss(a.detach(), b)
            elif n["mode"] == 1:
                lv = spair_ref.tf_safe_log(b * b)
                t = -0.5 * (1 + lv - a * a - torch.exp(lv))                                   # the summand of R.kl_divergence
            else:
                m2 = g.dyn[n["dyn_idx"]] if n["dyn_idx"] >= 0 else n["p0"]
                s2 = torch.full_like(b, n["p1"])
                t = spair_ref.tf_safe_log(s2) - spair_ref.tf_safe_log(b) + (b * b + (a - m2) ** 2) / (2 * s2 * s2) - 0.5     # of R.kl_divergence_two_gauss
            sums[n["loss_idx"]] = per_image(t)
        elif k == NOISE:
            pass                                                                              # pinned: the tensor is an input
        else:
            raise ValueError(k)

    r = TwinResult()
    means = [s.mean() for s in sums]
    w = torch.tensor(g.weights, dtype=dtype)
    total = sum(w[i] * means[i] for i in range(n_loss)) if n_loss else torch.zeros((), dtype=dtype)
    out = torch.zeros(1 + 2 * MAX_LOSS, dtype=dtype)
    out[0] = total.detach()
    for j, row in enumerate(g.report or []):
        out[1 + j] = sum(float(row[i]) * means[i].detach() for i in range(n_loss))
    for i in range(n_loss):
        out[1 + MAX_LOSS + i] = means[i].detach()
    r.loss_out, r.sums, r.total = out, [s.detach() for s in sums], total
    r.act = {i: read(i).detach().clone() for i in range(len(tens))}
    r.flat = {i: f.detach() for i, f in flat.items()}
    r.grad, r.pgrad = {}, None
    if backward and n_loss and total.requires_grad:
        wrt = [P] + [leaves[i] for i in leaves] + [p for _, _, p in probes]
        gs = torch.autograd.grad(total, wrt, allow_unused=True)
        z = lambda v, like: torch.zeros_like(like) if v is None else v
        r.pgrad = z(gs[0], P).detach()
        gbuf = {i: torch.zeros(_granule(tens[i]), dtype=dtype) for i in flat}
        seen = {i: torch.zeros(_granule(tens[i]), dtype=torch.bool) for i in flat}

        def put(tid, c0, val):                    # first writer of an element wins
            root = tens[tid]["root"]
            gm, sm = mat(tid, gbuf[root]), mat(tid, seen[root])
            cur, new = gm[:, c0:c0 + val.shape[1]], sm[:, c0:c0 + val.shape[1]]
            gm[:, c0:c0 + val.shape[1]] = torch.where(new, cur, val)
            sm[:, c0:c0 + val.shape[1]] = True
        k = 1
        for i in leaves:
            put(i, 0, z(gs[k], leaves[i]))
            k += 1
        for tid, c0, p in probes:
            put(tid, c0, z(gs[k], p))
            k += 1
        for i, t in enumerate(tens):
            r.grad[i] = mat(i, gbuf[t["root"]])[:, :t["cols"]].clone() if t["grad"] else None
    return r


def _zpres_per_image(zp, logits, pre, prior_prob, temp, mean_kl):
    """compute_z_pres_kl_yolo_air per image: the oracle on one-image batches (its count recursion is per image); their mean is asserted to be the oracle's."""
    per = torch.stack([spair_ref.compute_z_pres_kl_yolo_air(zp[b:b + 1], logits[b:b + 1], pre[b:b + 1], prior_prob, temp) for b in range(zp.shape[0])])
    assert abs(float(per.detach().mean()) - float(mean_kl.detach())) <= 1e-5 * (1 + abs(float(mean_kl.detach())))
    return per


# ------------------------------------------------------------------------------------------------------------------- the device
class Device:
    """The graph recorded into the library: sv_tape_create / tensor / view / add / set_report / finalize / bind; run() = sv_tape_run."""

    def __init__(self, g, bind=True):
        from split_vae_amd import _lib
        self._lib, self.lib, self.g = _lib, _lib.load(), g
        self.h = C.c_void_p()
        assert self.lib.sv_tape_create(C.byref(self.h), g.B, _lib.SV_BF16 if g.bf16 else _lib.SV_F32) == 0
        for i, t in enumerate(g.tens):
            if t["root"] == i:
                got = self.lib.sv_tape_tensor(self.h, t["rows"], t["cols"], t["ld"], 1 if t["grad"] else 0)
            else:
                src = next(j for j in range(i) if g.tens[j]["root"] == t["root"])
                got = self.lib.sv_tape_view(self.h, src, t["rows"], t["cols"], t["ld"])
            assert got == i, (got, i)
        self.add_status = []
        for n in g.nodes:
            c = _lib.TapeNode()
            for k, v in n.items():
                setattr(c, k, v)
            self.add_status.append(self.lib.sv_tape_add(self.h, C.byref(c)))
        assert all(s == 0 for s in self.add_status), self.add_status
        if g.report is not None:
            m = [[0.0] * MAX_LOSS for _ in g.report]
            for j, row in enumerate(g.report):
                m[j][:len(row)] = [float(v) for v in row]
            arr = (C.c_float * (MAX_LOSS * len(m)))(*[v for row in m for v in row])
            assert self.lib.sv_tape_set_report(self.h, arr, len(m)) == 0
        assert self.lib.sv_tape_finalize(self.h) == 0
        self.ws = None
        if bind:
            self.bind()

    def __del__(self):
        try:
            if self.h:
                self.lib.sv_tape_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def steps(self, p):
        """the step list of pass p (sv_tape_steps / sv_tape_step_info): [(first, last, part, lane, records, [waits])]"""
        out = []
        for k in range(self.lib.sv_tape_steps(self.h, p)):
            s, w = self._lib.TapeStep(), (C.c_int32 * 64)()
            assert self.lib.sv_tape_step_info(self.h, p, k, C.byref(s), w, 64) == 0 and 0 <= s.n_waits <= 64
            out.append((s.first, s.last, s.part, s.lane, s.records, [w[i] for i in range(s.n_waits)]))
        return out

    def bind(self):
        from split_vae_amd.ops import _p, _stream
        nbytes = self.lib.sv_tape_workspace_bytes(self.h)
        self.ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
        assert self.lib.sv_tape_bind(self.h, _p(self.ws), nbytes, _stream()) == 0
        self.wsf = self.ws.view(torch.float32)
        oo, mo, nl = C.c_int64(), C.c_int64(), C.c_int32()
        assert self.lib.sv_tape_loss_info(self.h, C.byref(oo), C.byref(mo), C.byref(nl)) == 0
        self.loss_out = self.wsf[oo.value // 4: oo.value // 4 + 1 + 2 * MAX_LOSS]
        self.metric = self.wsf[mo.value // 4: mo.value // 4 + MAX_LOSS + 2]
        self.n_loss = nl.value
        self.pgrads = torch.full((max(self.g.n_params, 1),), 7.0, device="cuda")        # (stale on purpose: the adjoint zeroes them itself)
        self.grad_span = None

    def _view(self, tid, grad=False, full=False):
        t = self.g.tens[tid]
        off, goff = C.c_int64(), C.c_int64()
        assert self.lib.sv_tape_tensor_info(self.h, tid, C.byref(off), C.byref(goff)) == 0
        o = goff.value if grad else off.value
        if o < 0:
            return None
        return torch.as_strided(self.wsf, (t["rows"], t["ld"] if full else t["cols"]), (t["ld"], 1), o // 4)

    def act(self, tid, full=False):
        return self._view(tid, False, full)

    def grad(self, tid):
        return self._view(tid, True)

    def grad_region(self):
        """every gradient buffer of the tape, as one list of copies (what a forward-only run must leave alone)"""
        return [self._view(i, True, True).clone() for i, t in enumerate(self.g.tens) if t["root"] == i and t["grad"]]

    def run(self, inputs, params, backward=True, pinned=1, seed=1, step=0, accumulate=0):
        from split_vae_amd.ops import _p, _stream
        g = self.g
        for i, v in inputs.items():
            self.act(i).copy_(v.cuda())
        self.params = params.cuda().contiguous()
        a = self._lib.TapeRunArgs()
        a.params, a.grads = _p(self.params).value, _p(self.pgrads).value
        w = list(g.weights) or [0.0]
        wa = (C.c_float * len(w))(*w)
        a.loss_weights, a.n_weights = wa, len(g.weights)
        for i in range(8):
            a.dyn[i] = float(g.dyn[i])
        a.seed, a.step, a.pinned_noise = seed, step, pinned
        a.phases = PHASE_FORWARD | (PHASE_BACKWARD if backward else 0)
        a.accumulate_metrics = accumulate
        a.n_params = self.pgrads.numel()
        rc = self.lib.sv_tape_run(self.h, C.byref(a), _stream())
        torch.cuda.synchronize()
        return rc


# ------------------------------------------------------------------------------------------------------------------- input distributions
def uniform(lo, hi):
    return lambda g, r, c: torch.rand(r, c, generator=g) * (hi - lo) + lo


def positive(g, r, c):
    return F.softplus(torch.randn(r, c, generator=g)) + 0.05


def normal(std):
    return lambda g, r, c: torch.randn(r, c, generator=g) * std


def unit_draws(g, r, c):
    """uniform draws as the NOISE kernel makes them, (0, 1] on the 2^-24 grid, with values within 1e-6 of both ends"""
    u = (torch.randint(0, 1 << 24, (r, c), generator=g).double() + 1.0) / float(1 << 24)
    edge = torch.tensor([2.0 ** -24, 1.0 - 2.0 ** -24, 1.0, 0.5, 5.0 * 2.0 ** -24, 1.0 - 9.0 * 2.0 ** -24], dtype=torch.float64)
    k = min(6, u.numel() - 1)
    u.view(-1)[1:1 + k] = edge[:k]                      # (from flat index 1: column 0 of the 4-wide tensor is outside the node's block)
    return u.float()


def predictions(c0, hard):
    """xent predictions in (0, 1); in column c0: exact 0 and 1 (log(1e-8) on one side) and values outside [0, 1] (tf_safe_log's replacement branch: NaN -> -100,
    no gradient).  hard: also an exact 0 and an exact 1 under an arbitrary label (a slope of (1 - label) / 1e-8)."""
    def f(g, r, c):
        p = torch.rand(r, c, generator=g) * 0.96 + 0.02
        p[0, c0], p[1, c0], p[2, c0], p[3, c0] = 0.0, 1.0, -0.25, 1.5
        if hard:
            p[4, c0], p[5, c0] = 0.0, 1.0
        return p
    return f


def labels(c0):
    """labels in [0, 1]; rows 0 and 1 of column c0 agree with the exact-0 / exact-1 predictions there"""
    def f(g, r, c):
        l = torch.rand(r, c, generator=g)
        l[0, c0], l[1, c0] = 0.0, 1.0
        return l
    return f


# ------------------------------------------------------------------------------------------------------------------- the cases
CASES = {}


def case(name):
    def deco(f):
        CASES[name] = f
        return f
    return deco


def _tile_to_batch(g, t, B):
    """rows that are no multiple of the batch: tile them `B` times (rep) so that a loss node can own them image by image"""
    tt = g.tens[t]
    y = g.tensor(tt["rows"] * B, tt["cols"], tt["ld"])
    g.unary(COPY, t, y, tt["cols"], rep=B)
    return y


def _unary_ops(rows):
    def build():
        B = 2
        g = Graph(B)
        x = g.tensor(rows, 13, 16, init=normal(1.5))
        y = g.tensor(rows, 31, 32)
        ops = [(COPY, 0, 0), (RELU, 0, 0), (SIGMOID, 0, 0), (SOFTPLUS, -1.0, 0), (CLAMP, -0.5, 0.7), (SCALE, 1.7, 0)]
        for k, (op, p0, p1) in enumerate(ops):                                   # out of place, column blocks of 5 at odd offsets
            g.unary(op, x, y, 5, xo=k + 1, yo=1 + 5 * k, p0=p0, p1=p1)
        z = g.tensor(rows, 13, 16)
        g.unary(COPY, x, z, 13)
        for k, (op, p0, p1) in enumerate(ops):                                   # in place on a column block
            g.unary(op, z, z, 2, xo=1 + 2 * k, yo=1 + 2 * k, p0=p0, p1=p1)
        yt, zt = (y, z) if rows % B == 0 else (_tile_to_batch(g, y, B), _tile_to_batch(g, z, B))
        g.kl(yt, 15, 0.7, c0=1)
        g.kl(zt, 6, -1.3, c0=1)
        return g
    return build


for _r in (7, 65, 130):
    CASES["unary_ops_rows%d" % _r] = _unary_ops(_r)


def _unary_rep(rep, B, rows):
    def build():
        g = Graph(B)
        x = g.tensor(rows, 5, 8, init=normal(1.5))
        y = g.tensor(rows * rep, 11, 12)
        g.unary(COPY, x, y, 5, xo=0, yo=1, rep=rep)
        g.unary(SIGMOID, x, y, 4, xo=1, yo=7, rep=rep)
        g.unary(SOFTPLUS, y, y, 3, xo=2, yo=2, p0=-1.0)
        g.loss(1, y, 1, y, 6, 5, 0.9)
        return g
    return build


CASES["unary_rep1"] = _unary_rep(1, 2, 14)
CASES["unary_rep3"] = _unary_rep(3, 3, 7)
CASES["unary_rep16"] = _unary_rep(16, 2, 65)


@case("unary_softplus_small_sigma")
def _softplus_small_sigma():
    """SOFTPLUS (p0 = -1) on pre-activations in (-14, -7): sig from 9e-4 down to 8e-7, where its adjoint taken as 1 - exp(-sig) is a cancelling difference (6e-5 relative
    at -7, 13 % at -14; the float32 twin differentiates with a true sigmoid).  Out of place and in place, each next to a block at (-3, 5); the small block has a tensor
    of its own, so its gradient's relative error is not measured against the other block's norm."""
    B, rows = 2, 66
    g = Graph(B)
    small = g.tensor(rows, 8, 8, init=uniform(-13.0, -6.0))
    wide = g.tensor(rows, 8, 8, init=uniform(-2.0, 6.0))
    mu = g.tensor(rows, 8, 8)
    y = g.tensor(rows, 8, 8)
    g.unary(SOFTPLUS, small, y, 4, xo=0, yo=0, p0=-1.0)
    g.unary(SOFTPLUS, wide, y, 4, xo=0, yo=4, p0=-1.0)
    g.loss(1, mu, 0, y, 0, 8, 0.7)
    zs = g.tensor(rows, 5, 8)
    zw = g.tensor(rows, 5, 8)
    g.unary(COPY, small, zs, 5, xo=3)
    g.unary(COPY, wide, zw, 5, xo=3)
    g.unary(SOFTPLUS, zs, zs, 4, xo=1, yo=1, p0=-1.0)
    g.unary(SOFTPLUS, zw, zw, 4, xo=1, yo=1, p0=-1.0)
    g.loss(1, mu, 0, zs, 1, 4, -1.3)
    g.loss(1, mu, 4, zw, 1, 4, 0.9)
    return g


def _group(parts, rows, lanes=None, no_grad_part=None):
    """a concat group of `parts` column blocks (widths 1, 5, 13, ...) with mixed ops from `parts` sources into one tensor; 11 parts: the 8-part cut falls inside"""
    def build():
        B = 2
        g = Graph(B)
        widths = [(1, 5, 13)[k % 3] for k in range(parts)]
        ops = [(COPY, 0.0, 0.0), (SIGMOID, 0.0, 0.0), (SCALE, -0.6, 0.0), (SOFTPLUS, -1.0, 0.0), (CLAMP, -0.4, 0.9), (RELU, 0.0, 0.0)]
        total = sum(widths)
        tot2 = (total + 1) // 2 * 2
        y = g.tensor(rows, tot2, r4(tot2))
        srcs = [g.tensor(rows, w + 2, r4(w + 2), grad=(k != no_grad_part)) for k, w in enumerate(widths)]
        o = 0
        for k, w in enumerate(widths):
            op, p0, p1 = ops[k % 6]
            g.unary(op, srcs[k], y, w, xo=2 if w < 13 else 1, yo=o, p0=p0, p1=p1, group=3, lane=(lanes[k] if lanes else 0))
            o += w
        if tot2 > total:
            g.unary(COPY, srcs[0], y, 1, xo=0, yo=total)
        yt = y if rows % B == 0 else _tile_to_batch(g, y, B)
        g.kl(yt, tot2 // 2, 1.1)
        return g
    return build


CASES["group_2"] = _group(2, 65)
CASES["group_8_one_part_without_gradient"] = _group(8, 130, no_grad_part=3)
CASES["group_11_cut_inside"] = _group(11, 130)
CASES["group_interrupted_by_lane_change"] = _group(5, 130, lanes=[0, 0, 1, 1, 0])


@case("sample_logitnoise")
def _sample_logitnoise():
    B, rows = 3, 66
    g = Graph(B)
    o = g.tensor(rows, 13, 16)                                                   # [mean 0:5 | sig 5:10 | logits 10:13], as `o` in the model
    g.unary(SOFTPLUS, o, o, 5, xo=5, yo=5, p0=-1.0)
    eps = g.tensor(rows, 6, 8, grad=False)
    z = g.tensor(rows, 7, 8)
    g.add(SAMPLE, x=o, xo=0, t2=o, o2=5, t3=eps, o3=1, y=z, yo=2, n=5)
    u = g.tensor(rows, 4, 4, grad=False, init=unit_draws)
    pre = g.tensor(rows, 5, 8)
    g.add(LOGITNOISE, x=o, xo=10, t2=u, o2=1, y=pre, yo=1, n=3, p0=0.7)
    pres = g.tensor(rows, 3, 4)
    g.unary(SIGMOID, pre, pres, 3, xo=1)
    g.loss(1, z, 2, o, 5, 5, 0.8)
    g.loss(1, pre, 1, pres, 0, 3, 0.3)
    g.loss(1, o, 0, o, 5, 5, 1.7)
    return g


def _loss_modes(R, n):
    def build():
        B = 3
        g = Graph(B)
        rows = B * R
        label = g.tensor(rows, n + 1, r4(n + 1), grad=False, init=labels(1))
        pred = g.tensor(rows, n + 2, r4(n + 2), init=predictions(2, hard=(R * n == 3)))
        m = g.tensor(rows, 2 * n + 1, r4(2 * n + 1))
        sg = g.tensor(rows, n + 3, r4(n + 3), init=positive)
        g.loss(0, label, 1, pred, 2, n, 1.0)
        g.loss(1, m, 1, sg, 2, n, 0.5)
        g.loss(2, m, 1 + n, sg, 1, n, 0.25, p0=3.7, p1=0.5)                      # p0 as the prior's mean
        g.loss(2, m, 1, sg, 3, n, -0.6, p0=99.0, p1=0.8, dyn_idx=1)              # ... and through dyn[1]
        g.dyn[1] = -1.3
        down = g.tensor(rows, n, r4(n))                                          # two LOSS nodes on `sg` plus a downstream consumer of it
        g.unary(SOFTPLUS, sg, down, n, xo=2, p0=-1.0)
        g.loss(1, m, 1, down, 0, n, 0.35)
        g.report = [[1, 0, 0, 0, 0], [0, 1, 0.5, 0, 0], [0, 0, 0, 2, -1], [0.25, 0.25, 0.25, 0.25, 0.25]]
        return g
    return build


for _R, _n in ((3, 1), (16, 4), (60, 5)):
    CASES["loss_modes_Rn%d" % (_R * _n)] = _loss_modes(_R, _n)


def _two(order, first, second):
    """two consumers of one producer, in both tape orders"""
    for f in ((first, second) if order == 0 else (second, first)):
        f()


def _fan(kind, order):
    def build():
        B = 2
        g = Graph(B)
        if kind in ("dense_dense", "dense_loss"):
            src = g.tensor(14, 13, 16)
            x = g.tensor(14, 13, 16)
            g.unary(SCALE, src, x, 13, p0=0.8)                                    # x has a producer of its own: its gradient travels on
            a = lambda: g.kl(g.dense(x, 6, act=ACT_RELU), 3, 0.9)
            b = (lambda: g.kl(g.dense(x, 10), 5, -0.4)) if kind == "dense_dense" else (lambda: g.kl(x, 6, 0.6))
            _two(order, a, b)
        elif kind == "upsample_unary":
            x = g.tensor(B * 4 * 4, 8, 8)
            def a():
                y = g.tensor(B * 8 * 8, 8, 8)
                g.add(UPSAMPLE, x=x, y=y, B=B, H=4, W=4)
                g.kl(y, 4, 0.7)
            def b():
                z = g.tensor(B * 4 * 4, 6, 8)
                g.unary(SIGMOID, x, z, 6, xo=1)
                g.kl(z, 3, 1.2)
            _two(order, a, b)
        elif kind == "conv_unary":
            g.floor = 1e-4
            x = g.tensor(B * 8 * 8, 8, 8)
            def a():
                y = g.tensor(B * 8 * 8, 8, 8)
                g.add(CONV, x=x, y=y, w_off=g.param(3, 3, 8, 8, scale=0.2), b_off=g.param(8), B=B, H=8, W=8, C=8, Cout=8, k=3, stride=1, act=ACT_RELU)
                g.kl(y, 4, 0.7)
            def b():
                z = g.tensor(B * 8 * 8, 6, 8)
                g.unary(SIGMOID, x, z, 6, xo=1)
                g.kl(z, 3, 1.2)
            _two(order, a, b)
        elif kind in ("render_x_loss", "render_bg_unary"):
            g.floor = 1.5e-5                                                      # spair_glue_ref.render at these shapes: out 2.7e-6, g_obj 1.5e-5, g_bg 1.5e-6
            Rr, H, Cc = 4, 8, 3
            obj = g.tensor(B * Rr * H * H, Cc + 1, init=uniform(-0.2, 1.2))
            bg = g.tensor(B * H * H, Cc, init=uniform(0.0, 1.0))
            zd = g.tensor(B * Rr, 1, init=normal(2.0))
            zp = g.tensor(B * Rr, 1, init=uniform(0.05, 0.95))
            zl = g.tensor(B * Rr, 1, grad=False)
            g.floors[("grad", zd)] = g.floors[("grad", zp)] = 1e-4                # (sums over the image: the bounds' 2.5e-4 / 3.2e-4 are no tighter than this)
            def a():
                y = g.tensor(B * H * H, Cc)
                g.add(RENDER, x=obj, t2=bg, t3=zd, t4=zp, t5=zl, t6=-1, y=y, B=B, H=H, W=H, C=Cc, R=Rr, training=1)
                g.loss(1, y, 0, y, 1, 1, 0.9)
            def b():
                if kind == "render_x_loss":
                    g.kl(obj, 2, 0.02)                                            # a LOSS node adds into g_obj during the forward pass
                else:
                    z = g.tensor(B * H * H, Cc)
                    g.unary(SIGMOID, bg, z, Cc)
                    g.loss(1, z, 0, z, 1, 1, 0.8)
            _two(order, a, b)
        elif kind == "stn_inverse_unary":
            g.floor = 3e-5                                                        # spair_glue_ref.stn at these shapes: out 2.3e-5, g_obj 6.6e-5, g_z_where 2.7e-4
            Hc, S, Cc, Ho = 2, 4, 4, 8
            n = B * Hc * Hc
            obj = g.tensor(n * S * S, Cc, init=uniform(0.0, 1.0))
            zw = g.tensor(n, 4, init=normal(0.5))
            g.floors[("grad", obj)], g.floors[("grad", zw)] = 7e-5, 3e-4
            def a():
                full = g.tensor(n * Ho * Ho, Cc)
                g.add(STN, x=obj, t2=zw, y=full, B=B, H=S, W=S, C=Cc, Ho=Ho, Wo=Ho, Hc=Hc, Wc=Hc, inverse=1)
                g.kl(full, 2, 0.5)
            def b():
                z = g.tensor(n * S * S, 2, 4)
                g.unary(SIGMOID, obj, z, 2, xo=1)
                g.loss(1, z, 0, z, 1, 1, 0.8)
            _two(order, a, b)
        elif kind == "group_same_source":
            z = g.tensor(65, 5, 8)
            y = g.tensor(65 * 2, 12, 12)
            first, second = (dict(op=COPY, yo=0), dict(op=SIGMOID, yo=5)) if order == 0 else (dict(op=SIGMOID, yo=5), dict(op=COPY, yo=0))
            g.unary(x=z, y=y, n=5, xo=0, rep=2, group=1, **first)                 # a tile of z into two places: both adjoints add into grad(z)[:, 0:5]
            g.unary(x=z, y=y, n=5, xo=0, rep=2, group=1, **second)
            g.unary(COPY, z, y, 2, xo=3, yo=10, rep=2, group=1)                   # (and a third part that overlaps them partly)
            g.kl(y, 6, 1.0)
        else:
            raise ValueError(kind)
        return g
    return build


FAN_KINDS = ("dense_dense", "dense_loss", "upsample_unary", "conv_unary", "render_x_loss", "render_bg_unary", "stn_inverse_unary", "group_same_source")
for _k in FAN_KINDS:
    for _o in (0, 1):
        CASES["fan_%s_order%d" % (_k, _o)] = _fan(_k, _o)


@case("view_into_dense")
def _view_into_dense():
    B, n = 2, 6
    g = Graph(B)
    x = g.tensor(n * 4, 5, 8)
    a = g.dense(x, 8, act=ACT_RELU)                                               # [n * 4, 8]: rows of 8 floats, as a conv output's [n * s2 * s2, 64]
    v = g.view(a, n, 32)                                                          # -> [n, 4 * 8]
    g.kl(g.dense(v, 6), 3, 0.8)
    z = g.tensor(n * 4, 6, 8)
    g.unary(SIGMOID, a, z, 6, xo=2)                                               # a second adjoint reaches the gradient through the original shape
    g.kl(z, 3, -0.5)
    return g


def _dense(bias, relu, xgrad, M=14, K=13, N=10):
    def build():
        g = Graph(2)
        x = g.tensor(M, K, r4(K), grad=xgrad)
        y = g.dense(x, N, bias=bias, act=ACT_RELU if relu else ACT_NONE)
        g.kl(y, N // 2, 0.9)
        return g
    return build


for _b in (0, 1):
    for _r in (0, 1):
        for _x in (0, 1):
            CASES["dense_bias%d_relu%d_xgrad%d" % (_b, _r, _x)] = _dense(_b, _r, _x)
CASES["dense_ragged_65x33x129"] = _dense(1, 1, 1, 66, 33, 130)


@case("dense_split_k")
def _dense_split():
    """(32, 6912, 1024), the model's split-K layer, with bias and ReLU (applied after the split sums), then a second layer on top: the zero-at-start list"""
    g = Graph(2)
    x = g.tensor(32, 6912, init=uniform(0.0, 1.0))
    h = g.dense(x, 1024, act=ACT_RELU)
    y = g.dense(h, 6912, bias=False)                                              # (the dense image decoder's last layer)
    g.kl(y, 3456, 1e-3)
    g.kl(h, 512, 0.01)
    return g


def _conv(bf16, H, Ci, Co, k, s):
    def build():
        B = 2
        g = Graph(B, bf16=bf16)
        g.floor = 3e-2 if bf16 else 1e-4                                          # tests/test_gpu_spair.py: the conv kernels' own bounds
        x = g.tensor(B * H * H, Ci, r8(Ci))
        OH = (H + s - 1) // s
        y = g.tensor(B * OH * OH, Co, r8(Co))
        g.add(CONV, x=x, y=y, w_off=g.param(k, k, Ci, Co, scale=math.sqrt(2.0 / (k * k * Ci))), b_off=g.param(Co, scale=0.1), B=B, H=H, W=H, C=Ci, Cout=Co,
              k=k, stride=s, act=ACT_RELU)
        g.kl(y, Co // 2, 0.05)
        return g
    return build


CASES["conv_f32_obj_decoder_d2"] = _conv(False, 8, 32, 64, 3, 1)
CASES["conv_bf16_obj_decoder_d2"] = _conv(True, 8, 32, 64, 3, 1)
CASES["conv_f32_obj_encoder_conv1"] = _conv(False, 32, 3, 32, 3, 2)


@case("upsample_node")
def _upsample():
    B = 2
    g = Graph(B)
    # inputs in [0.5, 1.5]: the kl loss reads half of y as sig, and its slope 2 y / (y^2 + 1e-8) multiplies the forward pass's rounding by 1 / |y| -- with N(0, 1)
    # inputs the 22 of 16384 sig values below 1e-3 carried the whole error of the loss gradient (float32 twin 1.1e-5, 1.2e-7 without them; LAB_NOTES.md section 9)
    x = g.tensor(B * 8 * 8, 64, 64, init=uniform(0.5, 1.5))
    y = g.tensor(B * 16 * 16, 64, 64)
    g.add(UPSAMPLE, x=x, y=y, B=B, H=8, W=8)
    g.kl(y, 32, 0.1)
    return g


def _stn_glimpse(bbox):
    def build():
        B, Hc, H, Cc, S = 2, 4, 48, 3, 32
        g = Graph(B)
        g.floor = 1e-5                                                            # spair_glue_ref.stn at these shapes: out 2.2e-5, g_z_where 1.2e-3 -- no tighter
        img = g.tensor(B * H * H, Cc, grad=False, init=uniform(0.0, 1.0))         # than the 1e-5 / 1e-3 that stand
        zw = g.tensor(B * Hc * Hc, 4, init=normal(1.0))
        g.floors[("grad", zw)] = 1e-3
        gl = g.tensor(B * Hc * Hc * S * S, Cc)
        bb = g.tensor(B * Hc * Hc, 4, grad=False) if bbox else -1
        g.add(STN, x=img, t2=zw, y=gl, t3=bb, B=B, H=H, W=H, C=Cc, Ho=S, Wo=S, Hc=Hc, Wc=Hc, inverse=0)
        g.loss(1, gl, 0, gl, 1, 1, 0.01)
        g.kl(zw, 2, 0.3)
        return g
    return build


CASES["stn_glimpses_with_bbox"] = _stn_glimpse(True)
CASES["stn_glimpses_without_bbox"] = _stn_glimpse(False)


@case("stn_inverse_with_bbox")
def _stn_inverse():
    B, Hc, S, Cc, Ho = 2, 4, 32, 4, 48
    g = Graph(B)
    g.floor = 1.5e-4                                                              # spair_glue_ref.stn at these shapes: out 1.4e-4, g_obj 4.1e-4, g_z_where 4.4e-3
    n = B * Hc * Hc
    obj = g.tensor(n * S * S, Cc, init=uniform(0.0, 1.0))
    zw = g.tensor(n, 4, init=normal(0.5))
    g.floors[("grad", obj)], g.floors[("grad", zw)] = 5e-4, 5e-3
    full = g.tensor(n * Ho * Ho, Cc)
    bb = g.tensor(n, 4, grad=False)
    g.add(STN, x=obj, t2=zw, y=full, t3=bb, B=B, H=S, W=S, C=Cc, Ho=Ho, Wo=Ho, Hc=Hc, Wc=Hc, inverse=1)
    g.kl(full, 2, 0.01)
    return g


def _render(training, noise):
    def build():
        B, Rr, H, Cc = 2, 16, 48, 3
        g = Graph(B)
        g.floor = 2e-5                                                            # spair_glue_ref.render at these shapes: out 3.6e-6, g_obj 1.9e-5, g_bg 2.4e-6
        obj = g.tensor(B * Rr * H * H, Cc + 1, init=uniform(-0.2, 1.2))
        bg = g.tensor(B * H * H, Cc, init=uniform(0.0, 1.0))
        zd = g.tensor(B * Rr, 1, init=normal(2.0))
        zp = g.tensor(B * Rr, 1, init=uniform(0.05, 0.95))
        zl = g.tensor(B * Rr, 1, grad=False, init=normal(3.0))
        g.floors[("grad", zd)] = g.floors[("grad", zp)] = 1e-4                    # (sums over 2304 pixels: the bounds' 1.3e-3 / 1.6e-3 are no tighter than this)
        nz = g.tensor(B * Rr * H * H, Cc, grad=False, init=normal(0.01)) if noise else -1
        y = g.tensor(B * H * H, Cc)
        g.add(RENDER, x=obj, t2=bg, t3=zd, t4=zp, t5=zl, t6=nz, y=y, B=B, H=H, W=H, C=Cc, R=Rr, training=training)
        label = g.tensor(B * H * H, Cc, grad=False, init=uniform(0.0, 1.0))
        g.loss(0, label, 0, y, 0, Cc, 1.0)
        return g
    return build


CASES["render_training_noise"] = _render(1, True)
CASES["render_training_no_noise"] = _render(1, False)
CASES["render_test_time"] = _render(0, False)


@case("zpres_node")
def _zpres():
    B, Rr = 2, 16
    g = Graph(B)
    g.floor = 1e-4                                                                # spair_glue_ref.zpres_kl at these shapes: kl 4.3e-4, g_pre 3.9e-4: no tighter
    logits = g.tensor(B * Rr, 1, init=normal(2.0))
    g.floors[("grad", logits)] = 5e-6                                             # g_logits 3.4e-6
    pre = g.tensor(B * Rr, 1, init=normal(2.0))
    pres = g.tensor(B * Rr, 1)
    g.unary(SIGMOID, pre, pres, 1)
    g.weights.append(0.7)
    g.add(ZPRES, loss_idx=0, x=pres, t2=logits, t3=pre, R=Rr, p0=0.8, dyn_idx=0)
    g.dyn[0] = 0.1
    g.loss(1, logits, 0, pres, 0, 1, 0.2)
    return g


def lanes_graph(lanes):
    """A fork of two Dense -> in-place-activation chains joined by a concat group that feeds two LOSS nodes, plus a NOISE node: fixed-order kernels only (small K and
    N: no split-K; every Dense input has one writer).  lanes: None = everything on lane 0, else a seeded pseudo-random lane 0..3 per node."""
    g = Graph(2)
    rng = np.random.default_rng(lanes) if lanes is not None else None
    ln = lambda: int(rng.integers(0, 4)) if rng is not None else 0
    x = g.tensor(130, 13, 16, grad=False)
    eps = g.tensor(130, 5, 8, grad=False)
    g.add(NOISE, y=eps, op=0, p0=1.0, stream_id=3, lane=ln())
    chains = []
    for act in (SOFTPLUS, SIGMOID):
        h = g.dense(x, 24, act=ACT_RELU, lane=ln())
        y = g.dense(h, 10, lane=ln())
        g.unary(act, y, y, 5, xo=5, yo=5, p0=-1.0 if act == SOFTPLUS else 0.0, lane=ln())
        chains.append(y)
    z = g.tensor(130, 5, 8)
    g.add(SAMPLE, x=chains[0], xo=0, t2=chains[0], o2=5, t3=eps, o3=0, y=z, yo=0, n=5, lane=ln())
    cat = g.tensor(130, 15, 16)
    gl = ln()
    g.unary(COPY, z, cat, 5, yo=0, group=1, lane=gl)
    g.unary(COPY, chains[1], cat, 10, yo=5, group=1, lane=gl)
    g.weights = [0.7, 0.4]
    g.add(LOSS, loss_idx=0, mode=1, x=cat, xo=0, t2=cat, o2=10, R=65, n=5, lane=ln())
    g.add(LOSS, loss_idx=1, mode=2, x=chains[0], xo=0, t2=chains[0], o2=5, R=65, n=5, p0=0.3, p1=0.5, lane=ln())
    return g


def conv_lanes_graph(two_lanes):
    """The conv hand-off at bf16, B = 2 on 8 x 8 x 8 maps: Dense 8 -> 8 on lane 0 (so the convs' input has a gradient), a 3 x 3 ReLU conv on lane 0 -- with lanes its
    adjoint is the PRE / WGRAD / DGRAD triple --, a second 3 x 3 conv reading the same Dense output on lane 1 (both weight gradients then use lane 1's slab region), a
    COPY group joining the two and one kl loss over the join.  two_lanes False: the same nodes, all on lane 0."""
    B, H, C = 2, 8, 8
    g = Graph(B, bf16=True)
    x = g.tensor(B * H * H, C, C, grad=False)
    h = g.dense(x, C)
    ys = []
    for lane, act in ((0, ACT_RELU), (1 if two_lanes else 0, ACT_NONE)):
        y = g.tensor(B * H * H, C, C)
        g.add(CONV, x=h, y=y, w_off=g.param(3, 3, C, C, scale=math.sqrt(2.0 / (9 * C))), b_off=g.param(C, scale=0.1), B=B, H=H, W=H, C=C, Cout=C, k=3, stride=1,
              act=act, lane=lane)
        ys.append(y)
    cat = g.tensor(B * H * H, 2 * C, 2 * C)
    g.unary(COPY, ys[0], cat, C, yo=0, group=1)
    g.unary(COPY, ys[1], cat, C, yo=C, group=1)
    g.kl(cat, C, 0.05)
    return g


# ------------------------------------------------------------------------------------------------------------------- Philox mirror
def philox4x32_10(counter, key):
    """counter [n, 4] uint32, key = 64-bit seed -> [n, 4] uint32 (Salmon et al. 2011)"""
    c = [counter[:, i].astype(np.uint64) for i in range(4)]
    k0, k1 = np.uint64(key & 0xFFFFFFFF), np.uint64((key >> 32) & 0xFFFFFFFF)
    M0, M1, m32 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & m32, p1 >> np.uint64(32), p1 & m32
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return np.stack(c, axis=1).astype(np.uint32)


def noise_uniforms(total, seed, step, stream_id):
    """the `total` uniforms of one NOISE node in element order (float32, exact): counter {q, q >> 32, step, stream_id ^ (step >> 32) * 0x9E3779B9}, key = seed,
    value ((u >> 8) + 1) / 2^24"""
    nq = (total + 3) // 4
    q = np.arange(nq, dtype=np.uint64)
    ctr = np.zeros((nq, 4), dtype=np.uint32)
    ctr[:, 0] = (q & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    ctr[:, 1] = (q >> np.uint64(32)).astype(np.uint32)
    ctr[:, 2] = np.uint32(step & 0xFFFFFFFF)
    ctr[:, 3] = np.uint32((stream_id ^ (((step >> 32) * 0x9E3779B9) & 0xFFFFFFFF)) & 0xFFFFFFFF)
    r = philox4x32_10(ctr, seed)
    u = ((r >> np.uint32(8)).astype(np.float32) + np.float32(1.0)) * np.float32(1.0 / 16777216.0)
    return u.reshape(-1)[:total], u


def noise_normals(total, seed, step, stream_id, std):
    """Box-Muller in float64 from the same uniforms: (r0 cos a0, r0 sin a0, r1 cos a1, r1 sin a1) per counter"""
    _, u = noise_uniforms(total, seed, step, stream_id)
    u = u.astype(np.float64)
    r0, r1 = np.sqrt(-2.0 * np.log(u[:, 0])), np.sqrt(-2.0 * np.log(u[:, 2]))
    a0, a1 = 2.0 * np.pi * u[:, 1], 2.0 * np.pi * u[:, 3]
    v = np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1), r1 * np.sin(a1)], axis=1) * std
    return v.reshape(-1)[:total]
