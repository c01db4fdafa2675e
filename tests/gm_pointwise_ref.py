"""Float64 restatements (torch, CPU) of the SPLIT-GMVAE glue kernels of csrc/gm_pointwise.hip, one function per kernel, written from the formulas in
include/splitvae.h ("A9: SPLIT-GMVAE global encoder glue") and the model they replace (Encoder(type='gmvae').call_gmvae and the loss terms of
train_step_lg_gm_vae).  tests/test_gpu_gm_pointwise.py compares the kernels with them; tests/test_gm_pointwise_host.py checks them against closed forms.

  forward     plain float64 formulas
  backward    torch.autograd of the forward restatement -- never a hand-derived adjoint, so softplus' is a true sigmoid and elu' a true exp
  scale       next to most results: the largest |addend| of each element (of each sum: the largest |term|).  The GPU tests allow
              |gpu - ref| <= 1e-4 |ref| + 1e-5 scale: a cancelling sum is judged by its condition
  Philox      NumPy mirrors of philox_unit (dropout masks, Gumbel uniforms) and of gm_head_fwd's Box-Muller draw, on tape_ref.philox4x32_10
  bf16        bf16_rne: ONE round-to-nearest-even from float64 (torch's double -> bfloat16 goes through float32: two roundings), and the distance to the
              nearest rounding tie, with which the input generators keep results whose bf16 rounding fp32 arithmetic could flip out of the bf16 cases
  generators  the seeded inputs of the GPU tests (the host test checks that every one of them stays finite in the float64 reference)
"""
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from tape_ref import philox4x32_10  # noqa: E402

F64 = torch.float64
U_LO, U_HI = float(np.float32(1e-20)), 1.0 - 2.0 ** -24         # the kernel's documented clamp of u (fp32 constants 1e-20f, 0.99999994f)
PINS = (-7.0, -9.0, -11.0, -14.0, 12.0)                         # sigma pre-activations pinned on whole rows: sigma 9.1e-4, 1.2e-4, 1.7e-5, 8.3e-7; ~12
TIE_BAND = 8.0 * 2.0 ** -24                                     # see settle_away_from_ties


# ------------------------------------------------------------------------------------------------------------------- bf16
def bf16_rne(t):
    """float64 -> the nearest bf16 value (8 significant bits, ties to even), as float64.  Normal range only."""
    m, e = torch.frexp(t.to(F64))
    return torch.ldexp(torch.round(m * 256.0) / 256.0, e)         # torch.round: half to even


def bf16_ulp(t):
    _, e = torch.frexp(t.to(F64))
    return torch.ldexp(torch.ones_like(t, dtype=F64), e - 8)


def tie_distance(t):
    """|t - the nearest value halfway between two bf16 numbers|"""
    m, e = torch.frexp(t.to(F64))
    f = m * 256.0
    return torch.ldexp((f - torch.floor(f) - 0.5).abs() / 256.0, e)


def as_bf16(t):
    """values a bf16 tensor can hold, as float32 (the inputs 'the kernel actually reads')"""
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float32)


def settle_away_from_ties(x, results, is_bf16_input, exact_ties_ok=False, tries=40):
    """The bf16 cases expect EQUALITY with the once-rounded float64 result.  The kernels compute in fp32 and round that: where the float64 result lies within a few
    fp32 ulps of a bf16 tie the two roundings may differ by one bf16 ulp, which says nothing about the kernel.  Such elements are moved, here, in the generator:
    results(x) -> [(ref, scale), ...]; an element is kept only if every ref is further than TIE_BAND * scale from a tie (8 fp32 ulps of its largest addend: expm1f,
    the rounded 1 / (1 - rate) and two multiplications stay under 4).  Others get their input nudged by two bf16 ulps and are tried again.
    exact_ties_ok: a result exactly ON a tie stays (it has 9 significant bits, so a chain of exact or correctly rounded fp32 operations on bf16 inputs -- no rounded
    1 / (1 - rate) in it -- delivers it exactly, and both roundings then go to even)."""
    x = x.clone()
    for _ in range(tries):
        bad = None                                                  # (in the shape of the results: x may stack several inputs in front of it)
        for ref, scale in results(x):
            d = tie_distance(ref)
            b = (d <= TIE_BAND * scale) & (ref != 0) & ((d != 0) if exact_ties_ok else True)
            bad = b if bad is None else bad | b
        if not bool(bad.any()):
            return x
        nudged = x * 1.015625 + torch.sign(x) * 0.0009765625         # two bf16 ulps away from zero: never rounds back onto the old value
        x = torch.where(bad, as_bf16(nudged) if is_bf16_input else nudged, x)
    raise AssertionError("could not move every element away from the bf16 ties")


# ------------------------------------------------------------------------------------------------------------------- act / add
def act(a, kind):
    if kind == "relu":
        return torch.relu(a)
    if kind == "elu":
        return torch.where(a > 0, a, torch.expm1(torch.clamp(a, max=0.0)))
    assert kind is None
    return a * 1.0


def act_inverse(y, kind):
    """a pre-activation whose activation is exactly y (for relu's y == 0 and elu's y == -1: one with act' == 0)"""
    y = y.to(F64)
    if kind == "relu":
        return torch.where(y > 0, y, torch.full_like(y, -1.0))
    if kind == "elu":
        return torch.where(y > 0, y, torch.log1p(torch.clamp(y, max=0.0)))
    return y.clone()


def rate64(rate):
    return float(np.float32(rate))                                # the rate as the kernel receives it


def act_fwd_ref(a, C, ldx, kind, rate=0.0, keep=None):
    """a [rows, >= C] -> (y_act, x) [rows, ldx]: y_act = act(a), x = y_act * keep / (1 - rate); columns C.. are zero."""
    rows = a.shape[0]
    y = torch.zeros(rows, ldx, dtype=F64)
    x = torch.zeros(rows, ldx, dtype=F64)
    v = act(a[:, :C].to(F64), kind)
    y[:, :C] = v
    x[:, :C] = v * keep.to(F64) / (1.0 - rate64(rate)) if rate > 0 else v
    return y, x


def act_bwd_ref(gx, C, ldga, y_act=None, kind=None, rate=0.0, keep=None, gx2=None):
    """-> (ga [rows, ldga], scale).  gx is the gradient of the dropped-out activation, gx2 (optional) a second gradient of the activation itself; the kernel
    recovers act' from the stored activation y_act, the reference differentiates sum(gx * x) + sum(gx2 * y) through act_fwd_ref at the pre-activation that
    reproduces y_act exactly."""
    rows = gx.shape[0]
    a = (act_inverse(y_act[:, :C], kind) if y_act is not None else torch.zeros(rows, C, dtype=F64)).requires_grad_(True)
    y, x = act_fwd_ref(a, C, C, kind if y_act is not None else None, rate, keep)
    loss = (gx[:, :C].to(F64) * x).sum()
    if gx2 is not None:
        loss = loss + (gx2[:, :C].to(F64) * y).sum()
    g, = torch.autograd.grad(loss, a)
    d = torch.ones(rows, C, dtype=F64)
    if y_act is not None and kind is not None:                    # act' as a value, for the scale only
        yy = y_act[:, :C].to(F64)
        d = (yy > 0).to(F64) if kind == "relu" else torch.where(yy > 0, torch.ones_like(yy), yy + 1.0)
    s = gx[:, :C].to(F64).abs() * (keep.to(F64) / (1.0 - rate64(rate)) if rate > 0 else 1.0)
    if gx2 is not None:
        s = torch.maximum(s, gx2[:, :C].to(F64).abs())
    ga = torch.zeros(rows, ldga, dtype=F64)
    scale = torch.zeros(rows, ldga, dtype=F64)
    ga[:, :C] = g
    scale[:, :C] = s * d
    return ga, scale


def add_ref(a, b):
    return a.to(F64) + b.to(F64)


# ------------------------------------------------------------------------------------------------------------------- Philox
def philox_unit(seed, step, stream_id, gs, col):
    """philox_unit of gm_pointwise.hip: key = seed ^ 0x6d76616547, counter {col, gs, (gs >> 32) ^ (0x676d0000 + stream_id), step}, word 0 -> ((w >> 8) + 1) / 2^24
    in (0, 1].  gs (the GLOBAL sample index) and col broadcast; float32, exact."""
    gs, col = np.broadcast_arrays(np.asarray(gs, dtype=np.uint64), np.asarray(col, dtype=np.uint64))
    ctr = np.zeros((gs.size, 4), dtype=np.uint32)
    ctr[:, 0] = (col.reshape(-1) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    ctr[:, 1] = (gs.reshape(-1) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    ctr[:, 2] = (gs.reshape(-1) >> np.uint64(32)).astype(np.uint32) ^ np.uint32((0x676d0000 + stream_id) & 0xFFFFFFFF)
    ctr[:, 3] = np.uint32(step & 0xFFFFFFFF)
    w = philox4x32_10(ctr, (seed ^ 0x6d76616547) & 0xFFFFFFFFFFFFFFFF)[:, 0]
    return unit_open(w).reshape(gs.shape)


def unit_open(w):
    return ((w >> np.uint32(8)).astype(np.float32) + np.float32(1.0)) * np.float32(1.0 / 16777216.0)


def dropout_keep(rows, C, rate, seed, step, stream_id, sample_offset=0, rows_per_sample=1):
    """the mask act_fwd draws: row r belongs to sample sample_offset + r / rows_per_sample, its column index is (r % rows_per_sample) * C + c; keep = u > rate"""
    r = np.arange(rows, dtype=np.uint64)[:, None]
    c = np.arange(C, dtype=np.uint64)[None, :]
    u = philox_unit(seed, step, stream_id, np.uint64(sample_offset) + r // np.uint64(rows_per_sample), (r % np.uint64(rows_per_sample)) * np.uint64(C) + c)
    return torch.from_numpy((u > np.float32(rate)).astype(np.float32))


def gumbel_uniforms(B, K, seed, step, sample_offset=0):
    """the uniforms gumbel_softmax_fwd draws (stream id 7, column k of sample sample_offset + b), before the clamp"""
    b = np.arange(B, dtype=np.uint64)[:, None]
    k = np.arange(K, dtype=np.uint64)[None, :]
    return torch.from_numpy(philox_unit(seed, step, 7, np.uint64(sample_offset) + b, k))


def head_eps(B, L, seed, step, sample_offset=0, stream_id=0):
    """gm_head_fwd's draw: key = seed ^ 0xe9515eed, counter {j, gs, (gs >> 32) ^ 0x65707300, step}; eps = sqrt(-2 log u0) cos(2 pi u1), u0 / u1 from words 0 / 1.
    stream_id: sv_reparam_kl_fwd draws the same way with 0x65707300 + stream_id in the third word (pointwise_ref.reparam_eps).
    The angle is formed as the kernel forms it -- float32(2 pi) times u1, rounded to float32 (that difference alone is 4e-7 rad, times |r| up to 5.8); log, sqrt
    and cos are float64.  -> float64 [B, L]"""
    gs = (np.uint64(sample_offset) + np.arange(B, dtype=np.uint64))[:, None] + np.zeros((1, L), dtype=np.uint64)
    j = np.zeros((B, 1), dtype=np.uint64) + np.arange(L, dtype=np.uint64)[None, :]
    ctr = np.zeros((B * L, 4), dtype=np.uint32)
    ctr[:, 0] = j.reshape(-1).astype(np.uint32)
    ctr[:, 1] = (gs.reshape(-1) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    ctr[:, 2] = (gs.reshape(-1) >> np.uint64(32)).astype(np.uint32) ^ np.uint32((0x65707300 + stream_id) & 0xFFFFFFFF)
    ctr[:, 3] = np.uint32(step & 0xFFFFFFFF)
    w = philox4x32_10(ctr, (seed ^ 0xe9515eed) & 0xFFFFFFFFFFFFFFFF)
    u0, u1 = unit_open(w[:, 0]), unit_open(w[:, 1])
    angle = (np.float32(6.283185307179586) * u1).astype(np.float64)
    e = np.sqrt(-2.0 * np.log(u0.astype(np.float64))) * np.cos(angle)
    return torch.from_numpy(e.reshape(B, L))


# ------------------------------------------------------------------------------------------------------------------- Gumbel softmax
def clamp_u(u):
    """the kernel's clamp of u to [1e-20, 1 - 2^-24], in float32 as the kernel does it: part of the contract (u_out holds these values)"""
    return torch.clamp(u.to(torch.float32), U_LO, U_HI)


def gumbel_fwd_ref(logits, u, tau):
    """logits [B, K], u [B, K] -> y = softmax((logits - log(-log clamp(u))) / tau, axis 1)"""
    uc = clamp_u(u).to(F64)
    return torch.softmax((logits.to(F64) - torch.log(-torch.log(uc))) / tau, dim=1)


def y_kl_ref(logits):
    """per image: sum_k p (log(p + 1e-8) - log(1 / K)), p = softmax(logits); also the largest |term| of each sum"""
    K = logits.shape[1]
    p = torch.softmax(logits.to(F64), dim=1)
    t = p * (torch.log(p + 1e-8) - math.log(1.0 / K))
    return t.sum(dim=1), t.abs().max(dim=1).values


def gumbel_bwd_ref(gy, logits, u, tau, alpha_over_B):
    """-> (g_logits, scale, y_kl, y_kl_scale): autograd of sum(gy * y(logits)) + alpha_over_B * sum_b y_kl[b].
    scale: the addends of an element are y gy / tau, y <y, gy> / tau, alpha p f, alpha p <p, f> (f = d (p log(p + 1e-8) + p log K) / dp); the two inner products are
    sums themselves, taken at sum |term|."""
    l = logits.to(F64).clone().requires_grad_(True)
    y = gumbel_fwd_ref(l, u, tau)
    kl, kl_scale = y_kl_ref(l)
    g, = torch.autograd.grad((gy.to(F64) * y).sum() + alpha_over_B * kl.sum(), l)
    with torch.no_grad():
        K = l.shape[1]
        p = torch.softmax(l, dim=1)
        f = torch.log(p + 1e-8) + math.log(K) + p / (p + 1e-8)
        ygy = (y * gy.to(F64)).abs()
        s1 = torch.maximum(ygy, y * ygy.sum(dim=1, keepdim=True)) / tau
        s2 = abs(alpha_over_B) * torch.maximum(p * f.abs(), p * (p * f.abs()).sum(dim=1, keepdim=True))
    return g.detach(), torch.maximum(s1, s2), kl.detach(), kl_scale.detach()


def gumbel_bwd_closed_form(gy, y, logits, tau, alpha_over_B):
    """the formula in the kernel's comment: (1 / tau) y (gy - <y, gy>) + alpha_over_B p (f - <p, f>)"""
    K = logits.shape[1]
    p = torch.softmax(logits.to(F64), dim=1)
    f = torch.log(p + 1e-8) + math.log(K) + p / (p + 1e-8)
    y, gy = y.to(F64), gy.to(F64)
    return y * (gy - (y * gy).sum(dim=1, keepdim=True)) / tau + alpha_over_B * p * (f - (p * f).sum(dim=1, keepdim=True))


# ------------------------------------------------------------------------------------------------------------------- the heads
def softplus(a):
    return torch.nn.functional.softplus(a, beta=1.0, threshold=1e9)      # no linear shortcut above 20: the formula itself


def _kl2_terms(m, s, m2, s2):
    return torch.stack([torch.log(s2), -torch.log(s), (s * s + (m - m2) ** 2) / (2.0 * s2 * s2), torch.full_like(s, -0.5)])


def gm_head_fwd_ref(a_m, a_s, a_pm, a_ps, eps):
    """-> dict of zm, zs, z, pm, ps [B, L], kl2 [B] and z_scale, kl2_scale (the largest |addend| of z's elements / of kl2's row sums)"""
    m, m2, e = a_m.to(F64), a_pm.to(F64), eps.to(F64)
    s, s2 = softplus(a_s.to(F64)), softplus(a_ps.to(F64))
    t = _kl2_terms(m, s, m2, s2)
    return dict(zm=m, zs=s, z=m + s * e, pm=m2, ps=s2, kl2=t.sum(dim=0).sum(dim=1), z_scale=torch.maximum(m.abs(), (s * e).abs()),
                kl2_scale=t.abs().amax(dim=(0, 2)))


def gm_head_bwd_ref(dz, a_m, a_s, a_pm, a_ps, eps, kl_scale):
    """-> ((g_am, g_as, g_apm, g_aps), (their scales)): autograd of sum(dz * z) + kl_scale * sum_b kl2[b] with respect to the four pre-activations"""
    leaves = [t.to(F64).clone().requires_grad_(True) for t in (a_m, a_s, a_pm, a_ps)]
    r = gm_head_fwd_ref(*leaves, eps)
    grads = torch.autograd.grad((dz.to(F64) * r["z"]).sum() + kl_scale * r["kl2"].sum(), leaves)
    with torch.no_grad():
        m, s, m2, s2, e, g, c = r["zm"], r["zs"], r["pm"], r["ps"], eps.to(F64), dz.to(F64), abs(kl_scale)
        d, is2 = m - m2, 1.0 / (s2 * s2)
        sg, sg2 = torch.sigmoid(leaves[1]), torch.sigmoid(leaves[3])
        sc_m = torch.maximum(g.abs(), c * d.abs() * is2)
        sc_s = torch.maximum(torch.maximum((g * e).abs(), c * s * is2), c / s) * sg
        sc_m2 = c * d.abs() * is2
        sc_s2 = torch.maximum(c / s2, c * (s * s + d * d) * is2 / s2) * sg2
    return tuple(t.detach() for t in grads), (sc_m, sc_s, sc_m2, sc_s2)


# ------------------------------------------------------------------------------------------------------------------- metrics
def gm_metrics_ref(terms, beta, alpha):
    """five [B] per-image terms -> out[6]: their batch means and out[0] + out[2] + beta (out[1] + out[3]) + alpha out[4]"""
    m = [t.to(F64).mean() for t in terms]
    return torch.stack(m + [m[0] + m[2] + beta * (m[1] + m[3]) + alpha * m[4]])


def gm_metrics_rtol(B):
    """(ceil(B / 256) + 8) * 2^-24 * 2: the serial adds of one thread plus the 8 levels of the tree, times 2 for the division and the final combination"""
    return ((B + 255) // 256 + 8) * 2.0 ** -24 * 2.0


# ------------------------------------------------------------------------------------------------------------------- input generators
ACT_SHAPES = ((7, 13, 16, 24, 1), (130, 128, 128, 128, 1), (48, 128, 128, 136, 16))          # rows, C, lda, ldx, rows_per_sample
GUMBEL_SHAPES = ((1, 2), (5, 10), (4, 64), (7, 65), (9, 127), (6, 128))
HEAD_SHAPES = ((1, 1), (5, 64), (7, 65), (6, 128), (3, 200))
METRICS_B = (1, 255, 256, 257, 1000)
ADD_N = (1, 257, 2100000)
GRID_ROWS, GRID_LD = 2100, 1024                                 # 2 150 400 elements > 8192 blocks * 256: every grid-stride loop takes a second trip


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def act_inputs(rows, C, lda, seed, bf16=False):
    """pre-activations over [-12, 6] (elu's expm1 tail down to 1 - 6e-6 from -1), with both ends, 0 and values of either sign next to 0 planted; the pad columns
    of `a` hold 99 (nothing may read them into an output)"""
    a = torch.full((rows, lda), 99.0)
    a[:, :C] = torch.rand(rows, C, generator=_gen(seed)) * 18.0 - 12.0
    edge = torch.tensor([-12.0, 6.0, 0.0, -1e-4, 1e-4, -11.5, -0.5, 0.5])
    k = min(edge.numel(), C)
    a[rows // 2, :k] = edge[:k]
    return as_bf16(a) if bf16 else a


def settled_act_inputs(rows, C, lda, seed, kind, rate=0.0, bf16=False):
    """act_inputs whose act(a) and act(a) / (1 - rate) are both away from the bf16 ties, whatever the mask keeps (for the cases with a bf16 output)"""
    ones = torch.ones(rows, C)

    def results(a):
        y, x = act_fwd_ref(a, C, lda, kind, rate, ones)
        return [(y, y.abs()), (x, x.abs())]
    return settle_away_from_ties(act_inputs(rows, C, lda, seed, bf16), results, bf16)


def settled_act_bwd_grads(gx, gx2, C, y_act, kind, rate, keep, bf16):
    """(gx, gx2) whose ga is away from the bf16 ties, by the scale of ga's addends; gx2 (may be None) moves too: a dropped element's ga does not depend on gx"""
    if gx2 is None:
        return settle_away_from_ties(gx[None], lambda g: [act_bwd_ref(g[0], C, g.shape[2], y_act, kind, rate, keep, None)], bf16, rate == 0)[0], None
    g = settle_away_from_ties(torch.stack([gx, gx2]), lambda g: [act_bwd_ref(g[0], C, g.shape[2], y_act, kind, rate, keep, g[1])], bf16, rate == 0)
    return g[0], g[1]


def pinned_keep(rows, C, rate, seed):
    """a pinned 0 / 1 mask at `rate`; column 0 of every row is kept (no row is all-dropped)"""
    k = (torch.rand(rows, C, generator=_gen(seed)) > rate).to(torch.float32)
    k[:, 0] = 1.0
    return k


def grads_like(rows, C, ld, seed, bf16=False):
    g = torch.full((rows, ld), 77.0)
    g[:, :C] = torch.randn(rows, C, generator=_gen(seed))
    return as_bf16(g) if bf16 else g


def add_inputs(n, seed, bf16=False):
    g = _gen(seed)
    a, b = torch.randn(n, generator=g) * 3.0, torch.randn(n, generator=g) * 0.01
    return (as_bf16(a), as_bf16(b)) if bf16 else (a, b)


def gumbel_inputs(B, K, ldl, seed, scale=1.0):
    """logits [B, ldl] (pad columns 55) and u [B, K] on the 2^-24 grid with the values 0, 2^-24, 1 - 2^-24 and 1 planted; scale = 40: logits over +-40"""
    g = _gen(seed)
    logits = torch.full((B, ldl), 55.0)
    if scale == 1.0:
        logits[:, :K] = torch.randn(B, K, generator=g) * 1.5
    else:
        logits[:, :K] = (torch.rand(B, K, generator=g) * 2.0 - 1.0) * scale
    u = ((torch.randint(0, 1 << 24, (B, K), generator=g).double() + 1.0) / float(1 << 24)).float()
    edge = torch.tensor([0.0, 2.0 ** -24, 1.0 - 2.0 ** -24, 1.0])
    k = min(4, B * K)
    u.view(-1)[:k] = edge[:k]
    gy = torch.randn(B, K, generator=g)
    return logits, u, gy


def head_inputs(B, L, seed):
    """the four pre-activations, eps and dz.  a_sig / a_prior_sig ~ N(0, 1.5); rows 0.. of a_sig are pinned at PINS in order (as many as B holds), those of
    a_prior_sig at PINS rotated by two rows: both heads meet sigma from 9e-4 down to 8e-7 and sigma ~ 12, and (B >= 3) no row has the same pin in both heads, where
    sigma / sigma2^2 - 1 / sigma would cancel exactly and say nothing about the factor behind it"""
    g = _gen(seed)
    a_m, a_pm = torch.randn(B, L, generator=g), torch.randn(B, L, generator=g)
    a_s, a_ps = torch.randn(B, L, generator=g) * 1.5, torch.randn(B, L, generator=g) * 1.5
    for v, k in pinned_rows(B).items():
        a_s[k] = v
    for v, k in pinned_rows(B, prior=True).items():
        a_ps[k] = v
    eps, dz = torch.randn(B, L, generator=g), torch.randn(B, L, generator=g)
    return a_m, a_s, a_pm, a_ps, eps, dz


def pinned_rows(B, prior=False):
    """{pin value: row} of a_sig (prior: of a_prior_sig) as head_inputs lays them out"""
    n = min(B, len(PINS))
    return {v: (k + 2) % n if prior else k for k, v in enumerate(PINS[:n])}


def metrics_inputs(B, seed):
    """five positive per-image terms of magnitudes 1e3, 1e1, 1e3, 1e1, 1e-1"""
    g = _gen(seed)
    return [(0.5 + torch.rand(B, generator=g)) * m for m in (1e3, 1e1, 1e3, 1e1, 1e-1)]
