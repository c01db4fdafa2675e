"""Plain float64 restatements of the convolution ABI (include/splitvae.h K3-K10), the two input families tests/test_gpu_conv_api.py runs on
and the `mut=` switches tests/test_conv_ref_host.py uses to show what the comparison can see.  CPU only: torch as an array library (the tap
loops below are written out; oracle/torch_ref.py and oracle/np_ref.py are what tests/test_conv_ref_host.py compares them with).

Layouts: activations NHWC, kernels HWIO.  TF SAME padding (the extra row / column at the bottom / right), the 2x bilinear resize with
half-pixel centres and edge clamp: hi-res row 2m = .25 x[m-1] + .75 x[m], row 2m+1 = .75 x[m] + .25 x[m+1], indices clamped.

Rounding points (read from the kernels): where a form rounds an intermediate to the activation dtype, the reference takes that point.
  * a fused resize stages its hi-res pixels in the activation dtype (tile_stage.hip.h blend2x2, row_conv.hip, upsample2x_fwd_kernel): the
    pixel is lerp(lerp(x00, x01, fx), lerp(x10, x11, fx), fy) with lerp(a, b, w) = fma(b - a, w, a) in fp32 (common.hip.h lerp2), then one
    conversion -- `resize2x_staged` restates exactly that, so the reference sees the operand the MFMA sees;
  * prepared weight images are the fp32 masters converted once (conv_api.hip prep_block: from_f32<T>); the composite images of the
    polyphase forms are combined in fp32 FIRST and converted once -- `poly_head_fwd` restates the bf16 head that way, with its border
    terms from the converted class sums and the staged edge lines (poly_fix.hip);
  * the input gradient of an ups_in layer at bf16 is rounded to bf16 at the hi-res tensor before the resize adjoint, by the row-ring
    kernel's fused epilogue and by dgrad + sv_upsample2x_bwd alike (common.hip.h adj2x_row_bf16) -- `dgrad_lowres(round_mid=...)`.
Every conversion is round to nearest even (common.hip.h: v_cvt_pk_bf16_f32), which is what torch's .to(bfloat16) does.

Integer family.  Operand entries are integers of small magnitude (`int_spec`), per-image scales the powers of two of Layer.SCALES, bias and
accumulator prefill multiples of 1/16.  The lemma (`conv_exact_property`): the bilinear coefficients are multiples of 1/16, so hi-res pixels
and composite polyphase weights are multiples of q_x / 16 with numerators below 2^8 -- exact in bf16; every product and every partial sum
of every form is a multiple of the unit q; while sum|terms| / q < 2^24 an fp32 accumulation is exact in ANY order, split or atomic fold; so
the float64 result, cast once to the output type, is bit for bit what a correct kernel returns.  For ups_in layers sum|terms| is taken over
the REPLICATE-padded resize of |x| and doubled: the polyphase forms add the border terms of the replicate-padded conv and subtract them
again (conv_geom.h svg_poly), and U |x| >= |U x| covers their composite products.

Gaussian family: `gauss_bound` of tests/latent_gemm_ref.py, unchanged; |a| . |b| is the same reference on absolute values."""
import math
import zlib

import torch

from latent_gemm_ref import gauss_bound  # noqa: F401  (re-exported: one bound for the latent GEMMs and the convs)

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
SCALES = (1.0, 2.0, 0.5, 4.0)          # per-image scales of batches that repeat P images (tests/test_gpu_conv_api.py Layer.SCALES)

MUTANTS = ("drop_border_tap", "swap_quarters_edge", "zero_pad_resize", "no_bias", "no_frame_corner", "gate_from_gradient")


def tdt(c):
    return F32 if c.dt == "f32" else BF16


def rnd(t, dtype):
    """float64 values of t converted once to dtype (round to nearest even)"""
    return t.to(F64).to(F32).to(dtype).to(F64) if dtype == BF16 else t.to(F64).to(F32).to(F64)


def same_pads(n, k, s):
    out = -(-n // s)
    pad = max((out - 1) * s + k - n, 0)
    return out, pad // 2, pad - pad // 2


# ---------------------------------------------------------------------------------------------------------------- the resize
def resize_matrix(n, mut=None):
    """[2n, n] float64: the 2x bilinear resize of one axis.  mut: swap_quarters_edge exchanges 1/4 and 3/4 on the first and the last hi-res
    row that blends two different low-res rows (rows 1 and 2n-2; rows 0 and 2n-1 are the clamped copies); zero_pad_resize reads zero where
    the clamp reads the edge row."""
    U = torch.zeros(2 * n, n, dtype=F64)
    for u in range(2 * n):
        m = u >> 1
        i0, i1, f = (m, m + 1, 0.25) if u & 1 else (m - 1, m, 0.75)         # f: weight of the second sample
        if mut == "swap_quarters_edge" and u in (1, 2 * n - 2):
            f = 1.0 - f
        for i, wgt in ((i0, 1.0 - f), (i1, f)):
            if 0 <= i < n:
                U[u, i] += wgt
            elif mut != "zero_pad_resize":
                U[u, min(max(i, 0), n - 1)] += wgt
    return U


def resize2x(x, mut=None):
    """[B, h, w, C] -> [B, 2h, 2w, C] in float64"""
    return torch.einsum("ui,vj,bijc->buvc", resize_matrix(x.shape[1], mut), resize_matrix(x.shape[2], mut), x.to(F64))


def resize2x_adjoint(g, mut=None):
    """[B, 2h, 2w, C] -> [B, h, w, C]: the transpose of resize2x"""
    return torch.einsum("ui,vj,buvc->bijc", resize_matrix(g.shape[1] // 2, mut), resize_matrix(g.shape[2] // 2, mut), g.to(F64))


def _lerp_f32(a, b, w):
    """fma(b - a, w, a) in fp32: the subtraction rounds to fp32, the fused multiply-add rounds once (evaluated in float64, where the product
    of a 24-bit and a 2-bit number and its sum with a are exact for operands within 2^26 of each other -- every tensor of the tests)"""
    d = (b.to(F32) - a.to(F32)).to(F64)
    return (d * w + a.to(F64)).to(F32)


def resize2x_staged(x, dtype):
    """the hi-res tensor as a fused resize stages it: fp32 lerps along x, then along y, one conversion to dtype.  x holds dtype values."""
    B, h, w, _ = x.shape

    def src(n):
        u = torch.arange(2 * n)
        m = u >> 1
        odd = (u & 1).bool()
        i0 = torch.where(odd, m, (m - 1).clamp_min(0))
        i1 = torch.where(odd, (m + 1).clamp_max(n - 1), m)
        f = torch.where(odd, torch.tensor(0.25, dtype=F64), torch.tensor(0.75, dtype=F64))
        return i0, i1, f
    y0, y1, fy = src(h)
    x0, x1, fx = src(w)
    xf = x.to(F32)
    fxv = fx.view(1, 1, -1, 1)
    top = _lerp_f32(xf[:, y0][:, :, x0], xf[:, y0][:, :, x1], fxv)
    bot = _lerp_f32(xf[:, y1][:, :, x0], xf[:, y1][:, :, x1], fxv)
    return rnd(_lerp_f32(top, bot, fy.view(1, -1, 1, 1)), dtype)


# ---------------------------------------------------------------------------------------------------------------- the conv and its gradients
def _pad_zero(x, KH, KW, s):
    B, H, W, C = x.shape
    oh, pt, pb = same_pads(H, KH, s)
    ow, pl, pr = same_pads(W, KW, s)
    xp = torch.zeros(B, H + pt + pb, W + pl + pr, C, dtype=F64)
    xp[:, pt:pt + H, pl:pl + W] = x
    return xp, oh, ow, pt, pl


def conv_hi(x, w, bias, s, act=None, mut=None):
    """SAME conv of the hi-res tensor x [B, H, W, Cin] with w [KH, KW, Cin, Cout] in float64.  mut: drop_border_tap leaves out, on output row
    0, the first kernel row that reads inside the image; no_bias."""
    KH, KW, _, Cout = w.shape
    xp, oh, ow, pt, pl = _pad_zero(x.to(F64), KH, KW, s)
    w = w.to(F64)
    out = torch.zeros(x.shape[0], oh, ow, Cout, dtype=F64)
    for i in range(KH):
        for j in range(KW):
            t = xp[:, i:i + (oh - 1) * s + 1:s, j:j + (ow - 1) * s + 1:s] @ w[i, j]
            if mut == "drop_border_tap" and i == pt and j == min(pl, KW - 1):
                t[:, 0] = 0.0
            out += t
    if bias is not None and mut != "no_bias":
        out = out + bias.to(F64)
    return out.clamp_min(0.0) if act == "relu" else out


def frame_corner(x_hi, w):
    """the top-left corner term of the polyphase frame: what the taps that leave the image in BOTH directions read from the replicate-padded
    hi-res tensor -- the form adds it with the replicate-padded conv and its border terms must take it out again"""
    KH, KW, _, Cout = w.shape
    B, H, W, _ = x_hi.shape
    xp, oh, ow, pt, pl = _pad_zero(torch.zeros_like(x_hi, dtype=F64), KH, KW, 1)
    xp[:, :pt, :pl] = x_hi[:, :1, :1].to(F64)
    out = torch.zeros(B, oh, ow, Cout, dtype=F64)
    for i in range(KH):
        for j in range(KW):
            out += xp[:, i:i + oh, j:j + ow] @ w[i, j].to(F64)
    return out


def conv(x, w, bias, s, act=None, ups=False, stage=None, mut=None):
    """the forward of a descriptor: x is the low-res tensor of an ups_in layer.  stage: the activation dtype a fused resize stages its hi-res
    pixels in (None: the exact float64 resize)."""
    if ups:
        if stage is not None and mut is None:
            x = resize2x_staged(x, stage)
        else:
            x = resize2x(x, mut)
    pre = conv_hi(x, w, bias, s, None, mut)
    if mut == "no_frame_corner" and ups:
        pre = pre + frame_corner(x, w)
    return pre.clamp_min(0.0) if act == "relu" else pre


def dgrad(dy, w, s, H, W, mut=None):
    """the gradient at the conv's input [B, H, W, Cin] (the hi-res tensor of an ups_in layer) in float64"""
    KH, KW, Cin, _ = w.shape
    oh, pt, pb = same_pads(H, KH, s)
    ow, pl, pr = same_pads(W, KW, s)
    dxp = torch.zeros(dy.shape[0], H + pt + pb, W + pl + pr, Cin, dtype=F64)
    dy, w = dy.to(F64), w.to(F64)
    for i in range(KH):
        for j in range(KW):
            t = dy @ w[i, j].T
            if mut == "drop_border_tap" and i == pt and j == min(pl, KW - 1):
                t[:, 0] = 0.0
            dxp[:, i:i + (oh - 1) * s + 1:s, j:j + (ow - 1) * s + 1:s] += t
    return dxp[:, pt:pt + H, pl:pl + W]


def gate(g, act_tensor, mut=None):
    """ReLU gate: elements whose stored activation is not > 0 become zero.  mut gate_from_gradient: the gradient's own sign instead."""
    return g * ((g if mut == "gate_from_gradient" else act_tensor.to(F64)) > 0)


def dgrad_lowres(dy, w, H, W, mask_lo=None, round_mid=None, mut=None):
    """the gradient at the low-res tensor of an ups_in layer: conv-transpose, resize adjoint, gate of the stored low-res activation.
    round_mid: the dtype the hi-res gradient is rounded to between the two stages (None: not rounded)."""
    g = dgrad(dy, w, 1, H, W, mut)
    if round_mid is not None:
        g = rnd(g, round_mid)
    g = resize2x_adjoint(g, mut)
    return g if mask_lo is None else gate(g, mask_lo, mut)


def wgrad(x, dy, KH, KW, s, ups=False, stage=None, count=None, mut=None):
    """(dW [KH, KW, Cin, Cout], dbias [Cout]) summed over the batch; count [B]: how often each image occurs.  x: the low-res tensor of an
    ups_in layer."""
    if ups:
        x = resize2x_staged(x, stage) if (stage is not None and mut is None) else resize2x(x, mut)
    xp, oh, ow, pt, pl = _pad_zero(x.to(F64), KH, KW, s)
    dy = dy.to(F64)
    if count is not None:
        dy = dy * count.to(F64).view(-1, 1, 1, 1)
    dw = torch.zeros(KH, KW, x.shape[-1], dy.shape[-1], dtype=F64)
    for i in range(KH):
        for j in range(KW):
            p = xp[:, i:i + (oh - 1) * s + 1:s, j:j + (ow - 1) * s + 1:s]
            if mut == "drop_border_tap" and i == pt and j == min(pl, KW - 1):
                p = p.clone()
                p[:, 0] = 0.0
            dw[i, j] = torch.einsum("bhwc,bhwo->co", p, dy)
    db = dy.sum((0, 1, 2))
    return dw, (torch.zeros_like(db) if mut == "no_bias" else db)


# ---------------------------------------------------------------------------------------------------------------- the polyphase head
def pcoef(p, k, t, pad):
    """blend coefficient of hi-res tap k of output parity p on the low-res offset t (conv_geom.h svg_pcoef, restated)"""
    h = p + k - pad
    m = h >> 1
    if h & 1:
        return 0.75 if t == m else 0.25 if t == m + 1 else 0.0
    return 0.25 if t == m - 1 else 0.75 if t == m else 0.0


def composite_weights(w, dtype=None):
    """W'[py, px][ty + 2, tx + 2] = sum_{ky, kx} cy cx w[ky, kx] of a 6 x 6 kernel, [2, 2, 5, 5, Cin, Cout] float64; dtype: converted once, AFTER
    the combination (conv_api.hip prep_block, SV_PREP_POLY_MAIN)"""
    K, pad = 6, 2
    w = w.to(F64)
    out = torch.zeros(2, 2, 5, 5, w.shape[2], w.shape[3], dtype=F64)
    for py in range(2):
        for px in range(2):
            for ty in range(-2, 3):
                for tx in range(-2, 3):
                    for ky in range(K):
                        cy = pcoef(py, ky, ty, pad)
                        for kx in range(K):
                            cx = pcoef(px, kx, tx, pad)
                            if cy and cx:
                                out[py, px, ty + 2, tx + 2] += cy * cx * w[ky, kx]
    return out if dtype is None else rnd(out, dtype)


_EXCL = ((0, (0, 1)), (1, (0,)), (-3, (5,)), (-2, (4, 5)), (-1, (3, 4, 5)))      # hi-res row / column (from the end when negative): taps that leave the image


def poly_head_fwd(x_lo, w, bias, dtype):
    """the polyphase head (conv_geom.h svg_poly: ups_in, 6 x 6) as its kernels compute it: composite weights over the edge-clamped low-res tensor,
    minus the border terms -- 1-D convs of the class sums (converted once) along the first / last staged hi-res row (replicate-extended) and column
    (zero outside).  x_lo holds dtype values, w the fp32 masters."""
    B, h, wd, Cin = x_lo.shape
    Cout = w.shape[3]
    Wc = composite_weights(w, dtype)
    xl = x_lo.to(F64)
    iy = (torch.arange(-2, h + 2)).clamp(0, h - 1)
    ix = (torch.arange(-2, wd + 2)).clamp(0, wd - 1)
    xc = xl[:, iy][:, :, ix]
    y = torch.zeros(B, 2 * h, 2 * wd, Cout, dtype=F64)
    for py in range(2):
        for px in range(2):
            acc = torch.zeros(B, h, wd, Cout, dtype=F64)
            for ty in range(5):
                for tx in range(5):
                    acc += xc[:, ty:ty + h, tx:tx + wd] @ Wc[py, px, ty, tx]
            y[:, py::2, px::2] = acc
    hi = resize2x_staged(x_lo, dtype)
    H2, W2 = 2 * h, 2 * wd
    w64 = w.to(F64)
    cxr = (torch.arange(-2, W2 + 3)).clamp(0, W2 - 1)
    for r, excl in _EXCL:
        line = hi[:, 0 if r >= 0 else H2 - 1][:, cxr]                       # [B, W2 + 5, Cin], replicate-extended
        for kx in range(6):
            fw = rnd(-sum(w64[ky, kx] for ky in excl), dtype)
            y[:, r] += line[:, kx:kx + W2] @ fw
    for cc, excl in _EXCL:
        col = torch.zeros(B, H2 + 5, Cin, dtype=F64)
        col[:, 2:2 + H2] = hi[:, :, 0 if cc >= 0 else W2 - 1]
        for ky in range(6):
            fw = rnd(-sum(w64[ky, kx] for kx in excl), dtype)
            y[:, :, cc] += col[:, ky:ky + H2] @ fw
    return y if bias is None else y + bias.to(F64)


# ---------------------------------------------------------------------------------------------------------------- input families
def int_spec(c):
    """(magnitude, density) of the integer family of a case: entries are integers in -m .. m, kept with probability `density` (else zero).
    -3 .. 3 where the property holds with it, -1 .. 1 for the 128- to 512-image cases; the 128-image polyphase head (2^19 hi-res positions per
    weight-gradient element at a unit of 1/32) takes sparse operands."""
    if c.B >= 128:
        return (1, 1.0 / 3) if c.ups else (1, 1.0)
    return 3, 1.0


def _ints(shape, g, mag, density):
    v = torch.randint(-mag, mag + 1, shape, generator=g).to(F32)
    if density < 1.0:
        v = v * (torch.rand(shape, generator=g) < density)
    return v


def geom(c):
    r8 = lambda v: (v + 7) // 8 * 8
    ldx = c.ldx or r8(c.Cin)
    ldy = c.ldy or (c.Cout if c.yf32 else r8(c.Cout))
    OH, OW = -(-c.H // c.s), -(-c.W // c.s)
    hin, win = (c.H // 2, c.W // 2) if c.ups else (c.H, c.W)
    return ldx, ldy, OH, OW, hin, win


def operands(c, family="gauss"):
    """dict of CPU tensors of one case: X [P, hin, win, Cin], DY [P, OH, OW, Cout], M (hi-res gate source), ML (low-res gate source) in the
    case's dtype, w (fp32 HWIO master), bias (fp32 | None), pidx / sidx [B] (image b = SCALES[sidx[b]] * X[pidx[b]]).  The Gaussian family draws
    what tests/test_gpu_conv_api.py always drew."""
    _, _, OH, OW, hin, win = geom(c)
    dt = tdt(c)
    P = c.P or c.B
    if family == "gauss":
        g = torch.Generator().manual_seed(zlib.crc32(c.name.encode()))
        X = torch.randn(P, hin, win, c.Cin, generator=g).to(dt)
        DY = torch.randn(P, OH, OW, c.Cout, generator=g).to(dt)
        M = torch.randn(P, c.H, c.W, c.Cin, generator=g).to(dt)
        ML = torch.randn(P, hin, win, c.Cin, generator=g).to(dt)
        fan = c.KH * c.KW * (c.Cin + c.Cout)
        w = ((torch.rand(c.KH, c.KW, c.Cin, c.Cout, generator=g) * 2 - 1) * math.sqrt(6.0 / fan)).contiguous()
        bias = (torch.randn(c.Cout, generator=g) * 0.1) if c.bias else None
    else:
        assert family == "int", family
        g = torch.Generator().manual_seed(zlib.crc32(("int " + c.name).encode()))
        mag, dens = int_spec(c)
        X = _ints((P, hin, win, c.Cin), g, mag, dens).to(dt)
        DY = _ints((P, OH, OW, c.Cout), g, mag, dens).to(dt)
        M = _ints((P, c.H, c.W, c.Cin), g, 3, 1.0).to(dt)
        ML = _ints((P, hin, win, c.Cin), g, 3, 1.0).to(dt)
        w = _ints((c.KH, c.KW, c.Cin, c.Cout), g, mag, 1.0).contiguous()
        bias = (_ints((c.Cout,), g, 3, 1.0) * 0.125) if c.bias else None
    pidx = torch.arange(c.B) % P
    sidx = (torch.arange(c.B) // P) % 4 if P < c.B else torch.zeros(c.B, dtype=torch.long)
    return dict(X=X, DY=DY, M=M, ML=ML, w=w, bias=bias, pidx=pidx, sidx=sidx)


def unique_images(ops):
    """(keys [(p, s)], uidx [B] -> key index, count [U], scale [U]) of a batch that repeats P images at power-of-two scales"""
    pairs = list(zip(ops["pidx"].tolist(), ops["sidx"].tolist()))
    keys = sorted(set(pairs))
    kidx = {k: i for i, k in enumerate(keys)}
    uidx = torch.tensor([kidx[k] for k in pairs])
    count = torch.bincount(uidx, minlength=len(keys)).to(F64)
    scale = torch.tensor([SCALES[s] for _, s in keys], dtype=F64)
    return keys, uidx, count, scale


def x_unique(ops):
    keys, _, _, scale = unique_images(ops)
    return torch.stack([ops["X"][p].to(F64) for p, _ in keys]) * scale.view(-1, 1, 1, 1)


CALLS = ("fwd", "dgrad", "lowres", "wgrad")        # every ABI call of a case is one of these four contractions (workspace variants, masks and the
#                                                   atomic accumulate change the order and the fold, which the property covers, not the terms)
PREFILL_UNIT = 1.0 / 16                            # accumulator prefill (Layer._pattern, + 1/16 on dbias) and the bias: multiples of 1/16 below 1


def _replicate_resize_abs(x):
    """U |x| replicate-padded by three hi-res pixels: an upper bound of what any form of an ups_in layer reads at any tap"""
    hi = resize2x(x.abs())
    iy = torch.arange(-3, hi.shape[1] + 3).clamp(0, hi.shape[1] - 1)
    ix = torch.arange(-3, hi.shape[2] + 3).clamp(0, hi.shape[2] - 1)
    return hi[:, iy][:, :, ix]


def _valid_abs_conv(xp, w):
    KH, KW = w.shape[:2]
    oh, ow = xp.shape[1] - 6, xp.shape[2] - 6
    _, pt, _ = same_pads(oh, KH, 1)
    _, pl, _ = same_pads(ow, KW, 1)
    out = torch.zeros(xp.shape[0], oh, ow, w.shape[3], dtype=F64)
    for i in range(KH):
        for j in range(KW):
            out += xp[:, 3 - pt + i:3 - pt + i + oh, 3 - pl + j:3 - pl + j + ow] @ w[i, j]
    return out


def ab_fwd_composite(xa_lo, wa):
    """sum|terms| of a polyphase forward per output element: its composite products add up to the conv over the REPLICATE-padded resize (U |x| covers
    them: the blend coefficients are non-negative), and the border terms take the part that leaves the image out again -- at most as much once more"""
    return 2.0 * _valid_abs_conv(_replicate_resize_abs(xa_lo), wa)


def ab_wgrad_composite(xa_lo, dya, KH, KW, count=None):
    """sum|terms| of a polyphase weight gradient (dW' projected, minus the frame terms): twice the gradient over the replicate-padded resize.  An element
    whose in-image products all vanish can still hold rounding from border products that cancel only in exact arithmetic: they are in here"""
    xp = _replicate_resize_abs(xa_lo)
    H, W = dya.shape[1], dya.shape[2]
    _, pt, _ = same_pads(H, KH, 1)
    _, pl, _ = same_pads(W, KW, 1)
    dyc = dya if count is None else dya * count.to(F64).view(-1, 1, 1, 1)
    dw = torch.zeros(KH, KW, xa_lo.shape[-1], dya.shape[-1], dtype=F64)
    for i in range(KH):
        for j in range(KW):
            dw[i, j] = torch.einsum("bhwc,bhwo->co", xp[:, 3 - pt + i:3 - pt + i + H, 3 - pl + j:3 - pl + j + W], dyc)
    return 2.0 * dw


def ab_lowres_composite(dya, wa, H, W):
    """sum|terms| of the polyphase input gradient (conv_geom.h svg_polyd): its main term is the gradient through an unpadded, unclamped resize -- the true
    terms A plus the pad terms E that the edge corrections remove -- and the corrections are -E plus the clamp folds (part of A): at most 3 A for E <= A"""
    return 3.0 * resize2x_adjoint(dgrad(dya, wa, 1, H, W))


def conv_exact_property(c, call, ops=None):
    """(q, worst): the unit every product and partial sum of `call` is a multiple of (a power of two) and the largest sum|terms| / q over all its
    output elements, bias and accumulator prefill included.  Asserts worst < 2^24: the lemma of the module docstring then makes the float64
    reference, cast once, the one right answer."""
    ops = ops or operands(c, "int")
    keys, uidx, count, scale = unique_images(ops)
    qx = float(min(SCALES[s] for _, s in keys)) * (1.0 / 16 if c.ups else 1.0)
    xa = x_unique(ops).abs()
    wa = ops["w"].to(F64).abs()
    dya = torch.stack([ops["DY"][p].to(F64) for p, _ in keys]).abs()
    if call == "fwd":
        q = min(qx, PREFILL_UNIT)
        m = ab_fwd_composite(xa, wa) if c.ups else conv_hi(xa, wa, None, c.s)
        if ops["bias"] is not None:
            m = m + ops["bias"].to(F64).abs()
    elif call == "dgrad":
        q = PREFILL_UNIT                                                    # (the atomic form adds onto the prefill)
        m = dgrad(dya, wa, c.s, c.H, c.W) + 0.5
    elif call == "lowres":
        assert c.ups
        q = 1.0 / 16
        m = ab_lowres_composite(dya, wa, c.H, c.W)
    else:
        assert call == "wgrad", call
        q = min(qx, PREFILL_UNIT)
        m = ab_wgrad_composite(xa, dya, c.KH, c.KW, count) if c.ups else wgrad(xa, dya, c.KH, c.KW, c.s, count=count)[0]
        m = torch.cat([m.flatten(), (dya * count.view(-1, 1, 1, 1)).sum((0, 1, 2))]) + 0.5
    lg = math.log2(q)
    assert lg == int(lg), q
    worst = float(m.max()) / q
    assert worst < 2.0 ** 24, f"{c.name} {call}: sum|terms| / q = {worst:.4g} >= 2^24 (q = {q})"
    return q, worst


def calls_of(c):
    return [k for k in CALLS if k != "lowres" or c.ups]


def references(c, ops, mut=None, absval=False, stage=False, round_mid=False):
    """every float64 reference of a case on its distinct images: y [U], dx [P] (at the conv's input), dxlo [P] (ups_in: at the low-res tensor, gated by
    ML), dw, db (summed over the batch).  Weights are the masters converted once to the case's dtype.  stage: the fused resize's hi-res pixels as staged
    (resize2x_staged); round_mid: the hi-res gradient rounded to the dtype before the adjoint.  absval: the same contractions on absolute values, without
    activation and gate -- the |a| . |b| of gauss_bound."""
    dt = tdt(c)
    keys, uidx, count, scale = unique_images(ops)
    ab = (lambda t: t.abs()) if absval else (lambda t: t)
    xu = ab(x_unique(ops))
    w = ab(rnd(ops["w"], dt))
    b = None if ops["bias"] is None else ab(ops["bias"].to(F64))
    DY = ab(ops["DY"].to(F64))
    st = dt if (stage and not absval) else None
    out = {}
    out["y"] = conv(xu, w, b, c.s, None if absval else c.act, bool(c.ups), st, mut)
    out["dx"] = dgrad(DY, w, c.s, c.H, c.W, mut)
    if c.ups:
        out["dxlo"] = dgrad_lowres(DY, w, c.H, c.W, None if absval else ops["ML"], dt if (round_mid and not absval) else None, mut)
    dyu = torch.stack([DY[p] for p, _ in keys])
    out["dw"], out["db"] = wgrad(xu, dyu, c.KH, c.KW, c.s, bool(c.ups), st, count, mut)
    return out
