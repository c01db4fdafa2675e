"""Float64 restatements (torch / NumPy, CPU) of the SPLIT-VAE pointwise kernels of csrc/pointwise.hip and csrc/dlogistic.hip.h, one function per kernel, written
from the formulas of the model they replace as oracle/torch_ref.py and oracle/np_ref.py restate them.  tests/test_gpu_pointwise.py compares the kernels with them;
tests/test_pointwise_host.py holds them to the oracle and to closed forms, and asserts every condition the generators below promise.

  forward     plain float64 formulas
  backward    torch.autograd of the forward restatement -- never a hand-derived adjoint (a hand-written expression appears only where a SCALE needs a value)
  scale       next to each result: the largest |addend| of that element (of a sum: the largest |term|).  The GPU tests allow
              |gpu - ref| <= 1e-4 |ref| + 1e-5 scale (+ a floor or a sum term derived from the kernel's arithmetic where the text says so)
  constants   a constant that a call rounds to fp32 before the kernel sees it enters the restatement ROUNDED (f32()): Adam's beta1, beta2, 1.f - beta, lr, eps,
              grad_scale and alpha, the dlogistic grad_scale, and kl_scale.  1.f - 0.999f is 1.3e-5 off 0.001: no per-element bound should absorb that
  Philox      NumPy mirrors of random_perm_kernel's keys and of reparam's Box-Muller draw (gm_pointwise_ref.head_eps with the stream id), on tape_ref.philox4x32_10
  generators  the seeded inputs of the GPU tests, with the conditions the host test asserts
"""
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gm_pointwise_ref import PINS, TIE_BAND, as_bf16, bf16_rne, head_eps, settle_away_from_ties, tie_distance, unit_open  # noqa: E402,F401
from tape_ref import philox4x32_10  # noqa: E402

F64 = torch.float64
ULP = 2.0 ** -24                                                  # half an fp32 ulp relative: what one correctly rounded fp32 operation adds
FLT_MIN = 2.0 ** -126                                             # below it fp32 arithmetic on the GPU flushes to zero (the hardware exp does)


def f32(v):
    """a host constant as the kernel receives it"""
    return float(np.float32(v))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------------------------- random_perm
def random_perm(B, n, seed, step=0, sample_offset=0):
    """random_perm_kernel: key = seed ^ 0x5ca1ab1e5eed, counter {i, gs, (gs >> 32) ^ 0x7065726d, step}, gs = sample_offset + b; row b is the indices 0..n-1 ordered by
    (word0 << 32) | i (no ties: the index is the low word).  -> int32 [B, n]"""
    gs = (np.uint64(sample_offset) + np.arange(B, dtype=np.uint64))[:, None] + np.zeros((1, n), dtype=np.uint64)
    i = np.zeros((B, 1), dtype=np.uint64) + np.arange(n, dtype=np.uint64)[None, :]
    ctr = np.zeros((B * n, 4), dtype=np.uint32)
    ctr[:, 0] = i.reshape(-1).astype(np.uint32)
    ctr[:, 1] = (gs.reshape(-1) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    ctr[:, 2] = (gs.reshape(-1) >> np.uint64(32)).astype(np.uint32) ^ np.uint32(0x7065726d)
    ctr[:, 3] = np.uint32(step & 0xFFFFFFFF)
    w0 = philox4x32_10(ctr, (seed ^ 0x5ca1ab1e5eed) & 0xFFFFFFFFFFFFFFFF)[:, 0].astype(np.uint64).reshape(B, n)
    keys = (w0 << np.uint64(32)) | i
    return (np.sort(keys, axis=1) & np.uint64(0xFFFFFFFF)).astype(np.int32)


PERM_N = (1, 2, 36, 63, 64, 65, 1000, 4096)


# ------------------------------------------------------------------------------------------------------------------- reparam / KL
def reparam_eps(B, L, seed, step, stream_id=0, sample_offset=0):
    """sv_reparam_kl_fwd's draw: gm_pointwise_ref.head_eps with 0x65707300 + stream_id in the third counter word"""
    return head_eps(B, L, seed, step, sample_offset, stream_id)


def softplus(a):
    return torch.nn.functional.softplus(a, beta=1.0, threshold=1e9)


def kl_addends(mu, sg):
    """the four addends of -1/2 (1 + log sig^2 - mu^2 - sig^2), stacked in front"""
    return torch.stack([torch.full_like(sg, -0.5), -0.5 * torch.log(sg * sg), 0.5 * mu * mu, 0.5 * sg * sg])


def reparam_fwd_ref(pre, bias, eps):
    """pre [B, 2L] (no bias), bias [2L], eps [B, L] -> dict: z_mean, z_sig, z [B, L], kl [B]; z_scale = max(|mu|, |sig eps|); kl_scale = the largest |addend| of the row;
    kl_sumabs = the sum of all |addends| of the row (the sum term of kl_sum_term)"""
    L = pre.shape[1] // 2
    p, b, e = pre.to(F64), bias.to(F64), eps.to(F64)
    mu = p[:, :L] + b[:L]
    a = p[:, L:] + b[L:]
    sg = softplus(a)
    t = kl_addends(mu, sg)
    return dict(z_mean=mu, z_sig=sg, z=mu + sg * e, kl=t.sum(dim=0).sum(dim=1), z_scale=torch.maximum(mu.abs(), (sg * e).abs()),
                mean_scale=torch.maximum(p[:, :L].abs(), b[:L].abs().expand_as(mu)), kl_scale=t.abs().amax(dim=(0, 2)), kl_sumabs=t.abs().sum(dim=(0, 2)), a_sig=a)


def kl_sum_term(L, sumabs):
    """the KL row sum of reparam_kl_fwd_body: a lane adds ceil(L / 64) elements in a chain, wave_sum adds 6 shuffle levels; each element is itself 1 + lv - mu^2 -
    exp(lv): three adds of addends that each carry one rounding of their own (logf, the product, expf: budget 2 half-ulps each).  Every one of these ceil(L / 64) +
    6 + 3 + 2 roundings is at most 2^-24 of a partial sum, and no partial sum exceeds the sum of all |addends|."""
    return ((L + 63) // 64 + 6 + 3 + 2) * ULP * sumabs


def reparam_bwd_ref(dz, dz2, pre, bias, eps, kl_scale):
    """-> (g_pre [B, 2L], scale): autograd of sum((dz + dz2) * z) + kl_scale * sum_b kl[b] with respect to pre.  kl_scale: the fp32-rounded value.
    scale: the mean half's addends are dz, dz2, kl_scale mu; the sd half's are dz eps, dz2 eps, kl_scale sig, kl_scale / sig, each times softplus' = sigmoid(a)."""
    pt = pre.to(F64).clone().requires_grad_(True)
    r = reparam_fwd_ref(pt, bias, eps)
    g = dz.to(F64) if dz2 is None else dz.to(F64) + dz2.to(F64)
    grad, = torch.autograd.grad((g * r["z"]).sum() + kl_scale * r["kl"].sum(), pt)
    with torch.no_grad():
        c, e = abs(kl_scale), eps.to(F64).abs()
        ga = dz.to(F64).abs() if dz2 is None else torch.maximum(dz.to(F64).abs(), dz2.to(F64).abs())
        mu, sg = r["z_mean"], r["z_sig"]
        s_m = torch.maximum(ga, c * mu.abs())
        s_s = torch.maximum(torch.maximum(ga * e, c * sg), c / sg) * torch.sigmoid(r["a_sig"])
    return grad.detach(), torch.cat([s_m, s_s], dim=1)


REPARAM_SHAPES = ((1, 1), (5, 10), (6, 64), (7, 100), (3, 130), (9, 256))


def reparam_inputs(B, L, seed):
    """pre, bias, eps, dz, dz2.  The sigma pre-activations (bias included) of rows 0.. are pinned at PINS in order, as many as B holds."""
    g = _gen(seed)
    pre = torch.randn(B, 2 * L, generator=g) * 2.0
    bias = torch.randn(2 * L, generator=g) * 0.1
    for k, v in enumerate(PINS[:B]):
        pre[k, L:] = v - bias[L:]
    eps, dz, dz2 = torch.randn(B, L, generator=g), torch.randn(B, L, generator=g), torch.randn(B, L, generator=g)
    return pre, bias, eps, dz, dz2


# ------------------------------------------------------------------------------------------------------------------- discretised logistic
# HW 64 (fewer pixels than threads), P = 1, P = 2 (1040 pixels per block), P = 4, P = 16, and HW = 3149 = 3 * 1050 - 1: the one shape whose last block is cut short
# by the image's end (HW % P != 0), with a second image behind it
DLL_SHAPES = ((3, 8, 8), (2, 32, 32), (2, 40, 52), (2, 64, 64), (1, 128, 128), (2, 47, 67))
DLL_THRESHOLD, DLL_BAND = 1e-5, 1e-4
FAMILIES = ("calm", "near", "far", "sat_lo", "sat_hi", "wide")


def dll_parts(HW):
    return HW // 1024 if HW > 1024 else 1


def dll_waves(HW):
    """per pixel of an image: the index of the wave that handles it, counted as dlogistic_kernel assigns pixels -- block `part` takes pixels [part * ppb, (part + 1)
    * ppb), thread t of it the pixels p0 + t + 256 k: a wave is 64 consecutive pixels from the block's p0, per 256-pixel trip"""
    P = dll_parts(HW)
    ppb = (HW + P - 1) // P
    p = np.arange(HW)
    part, o = p // ppb, p % ppb
    return part * ((ppb + 63) // 64) + o // 64


def dll_delta(x, m, ls):
    """float64 cdf_delta and the two saturated-pixel masks"""
    x, m, ls = x.to(F64), m.to(F64), ls.to(F64)
    s = torch.exp(-ls)
    c = x - m
    return torch.sigmoid(s * (c + 1.0 / 255.0)) - torch.sigmoid(s * (c - 1.0 / 255.0)), x < -0.999, x > 0.999


def dll_elem_ref(x, m, ls):
    """vae/trainer.py:21-38 element by element: -log_prob [..], float64.  softplus is the formula itself, log(1 + exp(v)): torch's default returns v above 20, which
    drops exp(-20) = 2e-9 from a saturated pixel's term (oracle/np_ref.py has no such shortcut, oracle/torch_ref.py has).  log_cdf_plus = p - softplus(p) is written
    as the same number -softplus(-p): autograd differentiates the first to 1 - sigmoid(p), which at p = 30 keeps two digits of float64 (measured: 2e-3 off at
    exp(-p) = 1e-13, where the kernel's s (1 - sigmoid(p)) was right to 5e-6), the second to sigmoid(-p)"""
    sp = softplus
    x, m, ls = x.to(F64), m.to(F64), ls.to(F64)
    c = x - m
    s = torch.exp(-ls)
    p, q, mid = s * (c + 1.0 / 255.0), s * (c - 1.0 / 255.0), s * c
    delta = torch.sigmoid(p) - torch.sigmoid(q)
    log_pdf_mid = mid - ls - 2.0 * sp(mid)
    lp = torch.where(x < -0.999, -sp(-p), torch.where(x > 0.999, -sp(q), torch.where(delta > DLL_THRESHOLD, torch.log(torch.clamp(delta, min=1e-12)),
                                                                                      log_pdf_mid - math.log(127.5))))
    return -lp


def dll_ref(images6, ch_off, out6, grad_scale=1.0, want_grad=True):
    """images6, out6 [B, H, W, 6] -> dict
      nll [B]                 per-image sums
      nll_sumabs, nll_max     the sum and the largest of the |terms| of each image
      g [B, H, W, 6]          d(sum nll) / d(out6) * f32(grad_scale) by autograd (channels 0-2 d/dm, 3-5 d/dlog_scale)
      g_scale                 the largest |addend| of each gradient element, g_floor: see below
    The kernel forms d/dm as s (1 - sig(p) - sig(q)) [mid], s (1 - sig(p)) [x < -.999], -s sig(q) [x > .999], s (1 - 2 sig(mid)) [rare]; d/dls as -p (1 - sig p) +
    q sig q - d / expm1(d), p (1 - sig p), -q sig q, mid (1 - 2 sig mid) + 1: g_scale is the largest of those addends.
    g_floor: a factor exp(-|v|) below FLT_MIN is zero on the GPU; what is lost is at most FLT_MIN times the addend's other factors (s for d/dm; |p|, |q|, |mid| for
    d/dls), times grad_scale."""
    x = images6[..., ch_off:ch_off + 3].to(F64)
    o = out6.to(F64).clone().requires_grad_(want_grad)
    m, ls = o[..., :3], o[..., 3:]
    t = dll_elem_ref(x, m, ls)
    r = dict(nll=t.detach().sum(dim=(1, 2, 3)), nll_sumabs=t.detach().abs().sum(dim=(1, 2, 3)), nll_max=t.detach().abs().amax(dim=(1, 2, 3)), terms=t.detach())
    if not want_grad:
        return r
    gs = f32(grad_scale)
    g, = torch.autograd.grad(t.sum(), o)
    with torch.no_grad():
        m, ls = o[..., :3].detach(), o[..., 3:].detach()
        c, s = x - m, torch.exp(-ls)
        p, q, mid, d = s * (c + 1.0 / 255.0), s * (c - 1.0 / 255.0), s * c, s * (2.0 / 255.0)
        delta, lo, hi = dll_delta(x, m, ls)
        rare = ~lo & ~hi & ~(delta > DLL_THRESHOLD)
        spc, sq, sm = torch.sigmoid(-p), torch.sigmoid(q), torch.sigmoid(mid)
        dm_s = torch.where(lo, s * spc, torch.where(hi, s * sq, torch.where(rare, s * torch.maximum(sm, 1.0 - sm), s * torch.maximum(spc, sq))))
        dl_mid = torch.maximum(torch.maximum((p * spc).abs(), (q * sq).abs()), d / torch.expm1(d))
        dl_s = torch.where(lo, (p * spc).abs(), torch.where(hi, (q * sq).abs(), torch.where(rare, torch.clamp((mid * torch.maximum(sm, 1.0 - sm)).abs(), min=1.0), dl_mid)))
        big = torch.maximum(torch.maximum(p.abs(), q.abs()), torch.ones_like(p))
        r.update(g=g.detach() * gs, g_scale=torch.cat([dm_s, dl_s], dim=-1) * abs(gs), g_floor=torch.cat([s, big], dim=-1) * (FLT_MIN * abs(gs)),
                 rare=rare, lo=lo, hi=hi, delta=delta)
    return r


# -log(delta) on the main branch: delta = sig(p) (1 - sig(q)) (1 - exp(-d)) carries a RELATIVE error, which -log turns into an ABSOLUTE one however small the
# result (delta -> 1).  Budget in half-ulps: sig(p) = rcp(1 + e): 2 (hardware exp, damped by e / (1 + e) <= 1/2) + 1 (the add) + 2 (rcp) = 5; 1 - sig(q) = e * that:
# 4 + 5 + 1 = 10; 1 - exp(-d) at d >= 0.25: 4 * exp(-d) / (1 - exp(-d)) <= 14 + 1, the series below: less; two products: 2.  32 half-ulps of relative error.
DLL_ELEM_FLOOR = 32 * ULP + FLT_MIN


def dll_sum_term(HW, sumabs):
    """the per-image NLL of dlogistic_kernel + rowsum_partials_kernel: a thread adds ceil(ppb / 256) pixels in a chain, each (n0 + n1) + n2 (2 adds); wave_sum 6
    levels, the 4-wave tree 2, the P partials P adds in index order.  Each of these roundings is at most 2^-24 of a partial sum, none of which exceeds the sum of the
    |terms|; on top of it every one of the 3 HW terms may carry DLL_ELEM_FLOOR."""
    P = dll_parts(HW)
    ppb = (HW + P - 1) // P
    return ((ppb + 255) // 256 + 2 + 6 + 2 + P) * ULP * sumabs + 3 * HW * DLL_ELEM_FLOOR


def _levels(g, shape):
    return torch.randint(0, 256, shape, generator=g).to(torch.float32) / 255.0 * 2.0 - 1.0


def _family(name, n, g):
    """n pixels x 3 channels of one family -> x, m, ls float32 [n, 3]"""
    x = torch.randint(1, 255, (n, 3), generator=g).to(torch.float32) / 255.0 * 2.0 - 1.0        # interior levels: neither saturated branch
    if name == "calm":                                              # no x < -0.999 lane, no x > 0.999 lane, every d = 2 exp(-ls) / 255 < 0.25 (ls > -3.46)
        ls = torch.rand(n, 3, generator=g) * 4.4 - 3.4
        m = x + torch.randn(n, 3, generator=g) * 2.0 * torch.exp(ls)
    elif name == "near":                                            # m = x + t exp(ls), t ~ N(0, 2), ls ~ U(-7, 1); lanes 0 and 1 saturated: both kinds in one wave
        ls = torch.rand(n, 3, generator=g) * 8.0 - 7.0
        x[0::16] = -1.0
        x[1::16] = 1.0
        m = x + torch.randn(n, 3, generator=g) * 2.0 * torch.exp(ls)
    elif name == "far":                                             # |x - m| exp(-ls) in 15 .. 200: the delta <= 1e-5 branch
        ls = torch.rand(n, 3, generator=g) * 8.0 - 7.0
        r = (15.0 + torch.rand(n, 3, generator=g) * 185.0) * torch.where(torch.rand(n, 3, generator=g) < 0.5, -1.0, 1.0)
        m = x + r * torch.exp(ls)
    elif name in ("sat_lo", "sat_hi"):                              # x = -1 / x = +1 with m on both sides, near and far
        x = torch.full((n, 3), -1.0 if name == "sat_lo" else 1.0)
        ls = torch.rand(n, 3, generator=g) * 8.0 - 7.0
        m = x + torch.randn(n, 3, generator=g) * 8.0 * torch.exp(ls)
    else:                                                           # wide scales: d / 4 crosses 1e-5 at ls = 5.28
        assert name == "wide"
        ls = torch.rand(n, 3, generator=g) * 6.0 + 3.0
        m = torch.randn(n, 3, generator=g)
    return x, m.to(torch.float32), ls.to(torch.float32)


def dll_layout(HW):
    """the family of every pixel of an image.  An image of 8 waves or more gives whole waves to one family each, in turn, and every seventh and eighth wave to all six
    (chunks of 11 lanes); a smaller image (8 x 8: one wave) is tiled by the chunks alone -- every family is in every image either way."""
    w = dll_waves(HW)
    nw = int(w.max()) + 1
    lane = np.arange(HW) - np.searchsorted(w, np.arange(nw))[w]      # (wave indices rise with the pixel index: a wave is one run of pixels)
    chunk = np.minimum(lane // 11, 5)
    if nw < 8:
        return chunk, w
    k = w % 8
    return np.where(k < 6, k, chunk), w


def dll_inputs(B, H, W, seed):
    """images6 [B, H, W, 6] (x | x-hat: both triples filled, different draws), out6 [2, B, H, W, 6] (the x and the x-hat decoder heads), float32; and the family index of
    every pixel [HW].  No unsaturated element of either network has its float64 delta within DLL_BAND (relative) of the 1e-5 threshold: such elements get m nudged by
    1 % of exp(ls) until they have -- the two branches are different approximations there and differ far beyond rounding."""
    HW = H * W
    fam, _ = dll_layout(HW)
    g = _gen(seed)
    images6 = torch.empty(B, HW, 6)
    out6 = torch.empty(2, B, HW, 6)
    for net in range(2):
        for b in range(B):
            for k, name in enumerate(FAMILIES):
                idx = torch.from_numpy(np.flatnonzero(fam == k))
                if idx.numel() == 0:
                    continue
                x, m, ls = _family(name, idx.numel(), g)
                images6[b, idx, 3 * net:3 * net + 3] = x
                out6[net, b, idx, :3] = m
                out6[net, b, idx, 3:] = ls
    for net in range(2):
        x, m, ls = images6[..., 3 * net:3 * net + 3], out6[net, ..., :3], out6[net, ..., 3:]
        for _ in range(40):
            delta, lo, hi = dll_delta(x, m, ls)
            bad = ~lo & ~hi & ((delta / DLL_THRESHOLD - 1.0).abs() < DLL_BAND)
            if not bool(bad.any()):
                break
            m[bad] = (m[bad].double() + 0.01 * torch.exp(ls[bad].double())).float()
        else:
            raise AssertionError("could not move every element out of the threshold band")
    return images6.reshape(B, H, W, 6).contiguous(), out6.reshape(2, B, H, W, 6).contiguous(), fam


def sums_to_one_inputs(m, ls):
    """sum over the 256 bins of exp(-nll) == 1: B = 256 images, one per bin; one probed element per image, every other element parked at x = -1, m = -3, log_scale = -5
    where its nll is exactly 0 in fp32"""
    ks = torch.arange(256, dtype=torch.float32) / 255.0 * 2.0 - 1.0
    x6 = torch.full((256, 8, 8, 6), -1.0)
    out6 = torch.zeros(256, 8, 8, 6)
    out6[..., :3] = -3.0
    out6[..., 3:] = -5.0
    x6[:, 0, 0, 0] = ks
    out6[:, 0, 0, 0] = m
    out6[:, 0, 0, 3] = ls
    return x6, out6


SUMS_TO_ONE = ((0.1, -2.0), (-0.7, -5.0), (0.9, -1.0), (0.0, -3.5), (0.3, -6.0), (0.2, -7.0), (-0.4, 2.0))


# ------------------------------------------------------------------------------------------------------------------- Adam
def adam_alpha(lr, beta1, beta2, t):
    """sv_adam_alpha: float(lr sqrt(1 - beta2^t) / (1 - beta1^t)) in double from the fp32 arguments"""
    lr, b1, b2 = f32(lr), f32(beta1), f32(beta2)
    return f32(lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t))


def adam_ref(p, g, m, v, t, lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-7, grad_scale=1.0, sc=None):
    """One Keras-Adam step in float64 from the fp32 state (not in place) -> (p', m', v'), (their scales).  Constants as the kernel receives them: alpha =
    adam_alpha(), omb = 1.f - beta in fp32, eps and grad_scale rounded.  sc: the factor on g (default grad_scale; the clipnorm form passes its own).
    scales: m' = m + (gc - m) omb: max(|m|, |gc| omb); v' likewise with gc^2; p' = p - step: max(|p|, |step|)."""
    p, g, m, v = (a.to(F64) for a in (p, g, m, v))
    omb1 = float(np.float32(1.0) - np.float32(beta1))
    omb2 = float(np.float32(1.0) - np.float32(beta2))
    gc = g * (f32(grad_scale) if sc is None else sc)
    m1 = m + (gc - m) * omb1
    v1 = v + (gc * gc - v) * omb2
    step = adam_alpha(lr, beta1, beta2, t) * m1 / (torch.sqrt(v1) + f32(eps))
    return (p - step, m1, v1), (torch.maximum(p.abs(), step.abs()), torch.maximum(m.abs(), gc.abs() * omb1), torch.maximum(v.abs(), gc * gc * omb2))


def clip_factor(g, tensor_off, clipnorm, grad_scale=1.0):
    """per element: grad_scale * clipnorm / max(||g * grad_scale||_2 of its tensor, clipnorm) (tf.clip_by_norm); clipnorm >= 1e37: grad_scale.  Also the norms."""
    gs, cn = f32(grad_scale), f32(clipnorm)
    sc = torch.empty(g.numel(), dtype=F64)
    norms = []
    for lo, hi in zip(tensor_off[:-1], tensor_off[1:]):
        n = float(torch.sqrt(((g[lo:hi].to(F64) * gs) ** 2).sum()))
        norms.append(n)
        sc[lo:hi] = gs if cn >= 1e37 else gs * cn / max(n, cn)
    return sc, norms


def clip_norm_rtol(n):
    """the relative error of a tensor's clip factor: its sum of squares is a chain of ceil(n / 4 / 65536) float4 steps (3 adds and 4 squarings each: 4 roundings deep),
    6 shuffle levels, the 4-wave tree (2) and the 256 partials added in index order; all terms are positive, so each rounding is at most 2^-24 of the sum.  The square
    root halves it; sqrt, the product and the division add 3."""
    return (4 * ((n // 4 + 65535) // 65536) + 6 + 2 + 256) * ULP / 2 + 3 * ULP


def clip_floors(E, p, g, m, v, t, sc, lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-7):
    """what a relative error E (per element; clip_norm_rtol of its tensor where the norm clips, else 0) of the clip factor moves: gc by E |gc|, so m' by E |gc| omb1
    and v' by 2 E gc^2 omb2; the step alpha m' / (sqrt(v') + eps) by its derivative in m' times the first plus its derivative in v' times the second
    -> floors of (p', m', v')"""
    (_, m1, v1), _ = adam_ref(p, g, m, v, t, lr, beta1, beta2, eps, sc=sc)
    gc = g.to(F64) * sc
    omb1, omb2 = float(np.float32(1.0) - np.float32(beta1)), float(np.float32(1.0) - np.float32(beta2))
    fm, fv = E * gc.abs() * omb1, 2.0 * E * gc * gc * omb2
    den = torch.sqrt(v1) + f32(eps)
    a = adam_alpha(lr, beta1, beta2, t)
    fp = a / den * fm + a * m1.abs() / (den * den) * fv / (2.0 * torch.sqrt(v1).clamp_min(1e-300))
    return fp, fm, fv


ADAM_N = (1, 2, 3, 5, 7, 1027, 4 * 256 * 2048 + 4099)
CLIP_TABLE = (3, 262149, 1, 0, 1030, 524291)
CLIPNORM = 1.0


def adam_inputs(n, seed):
    """p, m, v (a state as a previous step leaves it: v >= 0, not zeros) and three gradients spanning 1e-10 .. 10 in magnitude, with exact zeros and, where v is
    tiny as well, sqrt(v) << eps"""
    g = _gen(seed)
    p = torch.randn(n, generator=g)
    m = torch.randn(n, generator=g) * 10.0 ** (torch.rand(n, generator=g) * 6.0 - 6.0)
    v = (m * m) * (0.05 + torch.rand(n, generator=g))
    grads = []
    for k in range(3):
        gk = torch.randn(n, generator=g) * 10.0 ** (torch.rand(n, generator=g) * 11.0 - 10.0)
        gk[k::7] = 0.0
        grads.append(gk)
    tiny = torch.arange(n) % 5 == 1                                  # a fifth of the elements: m, v and every g tiny: sqrt(v) ~ 1e-10 << eps = 1e-7
    m[tiny] *= 1e-9
    v[tiny] = (m[tiny] * m[tiny]) * 0.5
    for gk in grads:
        gk[tiny] *= 1e-9
        gk[(gk != 0) & (gk.abs() < 1e-12)] = 1e-12                   # (gc^2 (1 - beta2) stays a normal fp32 number down to grad_scale = 1 / 64)
    return p, m, v, grads


def clip_inputs(seed):
    """the flat state and a gradient over CLIP_TABLE whose tensor norms are 3 and 0.2 (above and below CLIPNORM), 1 +- 1e-3 / 2 (within 1e-3 on either side), and one
    element; -> p, m, v, g, offsets (python ints)"""
    off = [0]
    for n in CLIP_TABLE:
        off.append(off[-1] + n)
    p, m, v, grads = adam_inputs(off[-1], seed)
    g = torch.randn(off[-1], generator=_gen(seed + 1))
    targets = (3.0, 1.0005, 0.2, None, 0.9995, 0.2)
    for (lo, hi), want in zip(zip(off[:-1], off[1:]), targets):
        if hi > lo:
            g[lo:hi] *= want / float(torch.sqrt((g[lo:hi].double() ** 2).sum()))
    return p, m, v, g, off


# ------------------------------------------------------------------------------------------------------------------- resize 2x
def _taps(n):
    """tf.image.resize (bilinear, half-pixel centres) 2x along one axis of length n: out[2i] = .25 in[i-1] + .75 in[i], out[2i+1] = .75 in[i] + .25 in[i+1], neighbours
    clamped -> (index0, index1, weight of index1) per output position"""
    o = torch.arange(2 * n)
    i = o // 2
    odd = (o % 2) == 1
    i0 = torch.where(odd, i, torch.clamp(i - 1, min=0))
    i1 = torch.where(odd, torch.clamp(i + 1, max=n - 1), i)
    w1 = torch.where(odd, torch.tensor(0.25, dtype=F64), torch.tensor(0.75, dtype=F64))
    return i0, i1, w1


def upsample_ref(x):
    """x [B, H, W, C] -> (out [B, 2H, 2W, C] float64, scale = the largest |weight * x| of the four products)"""
    x = x.to(F64)
    B, H, W, C = x.shape
    y0, y1, wy = _taps(H)
    x0, x1, wx = _taps(W)
    out, scale = 0.0, None
    for ys, fy in ((y0, 1.0 - wy), (y1, wy)):
        for xs, fx in ((x0, 1.0 - wx), (x1, wx)):
            t = x[:, ys][:, :, xs] * (fy[None, :, None, None] * fx[None, None, :, None])
            out = out + t
            scale = t.detach().abs() if scale is None else torch.maximum(scale, t.detach().abs())
    return out, scale


def upsample_bwd_ref(g_hi, mask=None):
    """the adjoint by autograd of upsample_ref, times (mask > 0) -> (g_lo, scale = the largest |weight * g| over the 16 taps, zero where the mask closes)"""
    B, H2, W2, C = g_hi.shape
    x = torch.zeros(B, H2 // 2, W2 // 2, C, dtype=F64, requires_grad=True)
    g, = torch.autograd.grad((upsample_ref(x)[0] * g_hi.to(F64)).sum(), x)
    # the scale: every product w * |g| scattered with max instead of +
    H, W = H2 // 2, W2 // 2
    y0, y1, wy = _taps(H)
    x0, x1, wx = _taps(W)
    ga = g_hi.to(F64).abs()
    scale = torch.zeros(B, H, W, C, dtype=F64)
    for ys, fy in ((y0, 1.0 - wy), (y1, wy)):
        for xs, fx in ((x0, 1.0 - wx), (x1, wx)):
            t = ga * (fy[None, :, None, None] * fx[None, None, :, None])
            flat = (ys[:, None] * W + xs[None, :]).reshape(-1)
            s = scale.reshape(B, H * W, C)
            s.scatter_reduce_(1, flat[None, :, None].expand(B, -1, C), t.reshape(B, H2 * W2, C), reduce="amax")
    if mask is not None:
        open_ = (mask.to(F64) > 0).to(F64)
        return g * open_, scale * open_
    return g, scale


UPS_F32 = ((1, 1, 1, 4), (2, 1, 5, 4), (2, 3, 1, 8), (2, 5, 7, 12), (1, 8, 24, 4), (16, 16, 64, 128), (64, 8, 32, 128))
UPS_BF16 = ((2, 1, 5, 8), (2, 5, 7, 24), (3, 8, 8, 32))


def ups_mask(shape, seed):
    """a ReLU mask holding +x, -x, 0.0 and -0.0"""
    mask = torch.randn(shape, generator=_gen(seed))
    k = torch.arange(mask.numel()).reshape(shape) % 8
    mask = torch.where(k == 0, torch.zeros_like(mask), mask)
    return torch.where(k == 1, -torch.zeros_like(mask), mask)


def ups_inputs(shape, seed, bf16=False):
    """x [B, H, W, C], g_hi [B, 2H, 2W, C], mask.  bf16: values +-(1 + k / 128) 2^e, e in -2 .. 1: bf16 numbers whose exponents differ by 3 at the most, so every
    product with a weight n / 16 and every partial sum of the 4 (adjoint: 16) products is a multiple of 2^-13 below 2^6 -- exact in fp32 in whatever order the kernel
    adds them -- and the bf16 output must be the float64 result rounded once, ties included (both round them to even).  A result NEAR a tie without being on it cannot
    be decided this way: such outputs (none with these inputs; the host test asserts it) would have the input under them -- x[oy / 2, ox / 2], g_hi[2i, 2j] -- nudged
    by two bf16 ulps and everything tried again."""
    B, H, W, C = shape
    g = _gen(seed)
    x, g_hi = torch.randn(B, H, W, C, generator=g), torch.randn(B, 2 * H, 2 * W, C, generator=g)
    mask = ups_mask(shape, seed + 1)
    if not bf16:
        return x, g_hi, mask

    def grid(shp):
        k, e = torch.randint(0, 128, shp, generator=g), torch.randint(-2, 2, shp, generator=g)
        return torch.where(torch.rand(shp, generator=g) < 0.5, -1.0, 1.0) * (1.0 + k / 128.0) * torch.exp2(e.float())
    x, g_hi, mask = grid(x.shape), grid(g_hi.shape), as_bf16(mask)
    assert torch.equal(x, as_bf16(x)) and torch.equal(g_hi, as_bf16(g_hi))

    def nudge(t, bad):
        return torch.where(bad, as_bf16(t * 1.015625 + torch.sign(t) * 0.0009765625), t)
    for _ in range(40):
        ref, scale = upsample_ref(x)
        d = tie_distance(ref)
        bad = (d <= TIE_BAND * scale) & (ref != 0) & (d != 0)
        if not bool(bad.any()):
            break
        x = nudge(x, bad.view(B, H, 2, W, 2, C).any(dim=4).any(dim=2))
    else:
        raise AssertionError("could not move every resize output away from the bf16 ties")
    for _ in range(40):
        ref, scale = upsample_bwd_ref(g_hi)
        d = tie_distance(ref)
        bad = (d <= TIE_BAND * scale) & (ref != 0) & (d != 0)
        if not bool(bad.any()):
            break
        sel = torch.zeros(B, H, 2, W, 2, C, dtype=torch.bool)
        sel[:, :, 0, :, 0] = bad
        g_hi = nudge(g_hi, sel.view(B, 2 * H, 2 * W, C))
    else:
        raise AssertionError("could not move every adjoint output away from the bf16 ties")
    return x, g_hi, mask


# ------------------------------------------------------------------------------------------------------------------- loss finaliser
FINALIZE_B = (1, 3, 64, 65, 257, 600)


def finalize_ref(nll_x, nll_xh, kl_x, kl_xh, beta):
    """per-image terms [B] (None: zeros) -> (losses[6], scale[6]): batch means {x_recon, x_kl, x_hat_recon, x_hat_kl, beta (x_kl + x_hat_kl), x_recon + x_hat_recon +
    total_kl}; scale: the largest |term| / B of a mean, the largest |addend| of a combination"""
    B = nll_x.numel()
    z = torch.zeros(B, dtype=F64)
    t = [z if a is None else a.to(F64) for a in (nll_x, kl_x, nll_xh, kl_xh)]
    mean = [a.sum() / B for a in t]
    mx = [a.abs().max() / B for a in t]
    b = f32(beta)
    tk = b * (mean[1] + mean[3])
    losses = torch.stack(mean + [tk, mean[0] + mean[2] + tk])
    scale = torch.stack(mx + [abs(b) * torch.maximum(mean[1].abs(), mean[3].abs()), torch.maximum(torch.maximum(mean[0].abs(), mean[2].abs()), tk.abs())])
    return losses, scale


def finalize_sum_term(B, terms, beta):
    """finalize_losses_kernel: a thread adds ceil(B / 256) terms in a chain, wave_sum 6 levels, the tree 2, one division, and the combinations up to 3 more roundings:
    each at most 2^-24 of the sum of the |terms| of the means it touches.  -> [6]"""
    k = ((B + 255) // 256 + 6 + 2 + 1 + 3) * ULP
    z = torch.zeros(B, dtype=F64)
    a = [(z if t is None else t.to(F64)).abs().sum() / B for t in terms]          # nll_x, kl_x, nll_xh, kl_xh
    b = abs(f32(beta))
    return k * torch.stack([a[0], a[1], a[2], a[3], b * (a[1] + a[3]), a[0] + a[2] + b * (a[1] + a[3])])


def rowsum_ref32(part):
    """rowsum_partials_kernel / the finaliser's own sums: float32 adds in index order from 0.f -- bit for bit"""
    s = np.zeros(part.shape[0], dtype=np.float32)
    for i in range(part.shape[1]):
        s = (s + part[:, i].astype(np.float32)).astype(np.float32)
    return s


def finalize_inputs(B, seed):
    """per-image terms of the magnitudes a step sees: nll ~ 5e3, kl ~ 30"""
    g = _gen(seed)
    return [(0.5 + torch.rand(B, generator=g)) * s for s in (5e3, 5e3, 30.0, 30.0)]              # nll_x, nll_xh, kl_x, kl_xh
