"""Plain float64 restatements of the four SPAIR glue kernels (split_vae_amd/csrc/stn.hip, spair_render.hip: renderer and sequential z_pres KL,
spair_loss.hip), each with a per-element bound on what an fp32 evaluation of the same formula may differ by, plus the case tables and input families
of tests/test_gpu_spair_glue.py and the `mut=` switches tests/test_spair_glue_host.py uses to show what the comparison can see.  CPU only, numpy.

How the bounds are made.  Every quantity is a `V`: a float64 value `v` and an absolute error bound `e` of the device's fp32 value of the same
quantity.  Each arithmetic operator of V restates one fp32 operation of the kernel, written in the kernel's order, and adds to the propagated
operand errors ONE rounding, u |result| with u = 2^-24 (round to nearest): the number of roundings on a path is counted by the operators that
stand in the formula, so the formula IS the count.  Second-order terms (e_a e_b) are kept.  A reduction over terms whose order is a tree of
depth d (a thread's serial adds, six wave shuffles, the four waves) takes d u sum|t| (`vsum`); atomics of n addends in any order n u sum|t|.
Operations that are exact in fp32 (times 0.5, negation, a selection by 0 / 1) use `x2` and add nothing.  Device functions use the maxima below
(in units of u, relative to the result): the ROCm device-library's documentation is not part of this tree, so these are ASSUMED -- the OpenCL
full-profile limits, which that library is built to: divide 2.5 ulp, exp / log 3 ulp, tanh 5 ulp, pow 16 ulp (1 ulp <= 2 u relative).
No constant here is fitted to a device result.

The STN's coordinate term.  x = .5 (sx gx + tx + 1)(W - 1) is a V like everything else, so its bound m_x = x.e is the operation count of
sigmoid / tanh / the divides of the inverse form / lin() / the bias applied to this cell and pixel; `c` = m_x / (u (|sx gx| + |tx| + 1)(W - 1)/2)
is reported by `stn_c()` (LAB_NOTES.md section 13).  From there m travels through the float64 SLOPES of the bilinear form, which is exact for a
form that is bilinear inside a cell:  out: m_x |d out/dx| + m_y |d out/dy| + m_x m_y |Ia - Ib - Ic + Id|;  g_img, per target pixel:
sum |g| (m_x |w_y| + m_y |w_x| + m_x m_y);  d loss/dx of a pixel: m_y sum_k |g_k| |Ia - Ib - Ic + Id|_k (and the same in y), then through the
chain to z_where as a V (absolute values of every factor, the 1/ex^2 of the inverse form included).

Folds.  Where a grid line k in 0 .. W-1 lies within m_x of x (and the point is within reach of the image on the other axis), the device's floor may
land on either side: `fold` marks those pixels.  Random cases must have none (asserted on the CPU for every case).  Where there are some (the
crafted family) the reference is evaluated for both choices per axis and every output becomes an interval [lo, hi] widened by the bound; out and
g_img are continuous across an interior line (lo = hi there) but NOT across x = 0 and x = W - 1, where the reference's clipping drops the pixel.
The renderer's test-time round(sigmoid(logit)) and its clip gates under noise are decisions of the same kind: see `render`."""
import numpy as np

U = 2.0 ** -24
E_DIV, E_EXP, E_LOG, E_TANH, E_POW = 5.0, 6.0, 6.0, 10.0, 32.0          # assumed (see above), units of u
F32 = np.float32
A_MIN32 = float(F32(1e-8))                                               # the fp32 constant 1e-8f the clip gates compare with


def f32(a):
    """float64 array of fp32-representable values"""
    return np.asarray(a, dtype=F32).astype(np.float64)


class V:
    """value + absolute error bound of the device's fp32 value; an operator = one fp32 operation = one rounding"""
    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        v, e = np.broadcast_arrays(np.asarray(v, dtype=np.float64), np.asarray(e, dtype=np.float64))
        self.v, self.e = v.copy(), e.copy()

    def __add__(a, b):
        b = _l(b)
        v = a.v + b.v
        return V(v, a.e + b.e + U * np.abs(v))

    __radd__ = __add__

    def __sub__(a, b):
        b = _l(b)
        v = a.v - b.v
        return V(v, a.e + b.e + U * np.abs(v))

    def __rsub__(a, b):
        return _l(b) - a

    def __mul__(a, b):
        b = _l(b)
        v = a.v * b.v
        return V(v, np.abs(a.v) * b.e + np.abs(b.v) * a.e + a.e * b.e + U * np.abs(v))

    __rmul__ = __mul__

    def __truediv__(a, b):
        b = _l(b)
        den = np.abs(b.v) - b.e
        v = a.v / b.v
        with np.errstate(divide="ignore", invalid="ignore"):
            e = np.where(den > 0, (a.e + np.abs(v) * b.e) / den, np.inf) + E_DIV * U * np.abs(v)
        return V(v, e)

    def __rtruediv__(a, b):
        return _l(b) / a

    def __neg__(a):
        return V(-a.v, a.e)

    def __getitem__(a, i):
        return V(a.v[i], a.e[i])

    def x2(a, c):
        """an exact fp32 operation: a power of two, a sign, a 0 / 1 selector"""
        return V(a.v * c, a.e * np.abs(c))

    def reshape(a, *s):
        return V(a.v.reshape(*s), a.e.reshape(*s))

    @property
    def shape(a):
        return a.v.shape


def _l(x):
    return x if isinstance(x, V) else V(x)


def c32(c):
    """a literal the kernel holds in fp32 while this file holds it in float64 (1e-5f, 1e-8f): off by one rounding"""
    return V(c, U * abs(c))


def vwhere(c, a, b):
    a, b = _l(a), _l(b)
    return V(np.where(c, a.v, b.v), np.where(c, a.e, b.e))


def vexp(a, native=False):
    """expf; native: __expf = exp2(x log2e), whose argument product adds u |x| to the exponent"""
    v = np.exp(a.v)
    ea = a.e + (U * np.abs(a.v) if native else 0.0)
    return V(v, v * (np.expm1(ea) + E_EXP * U))


def vlog(a):
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.log(a.v)
        e = np.where(a.v > a.e, -np.log1p(-np.minimum(a.e / a.v, 1.0)), np.inf)
    return V(v, e + E_LOG * U * np.abs(v))


def vtanh(a):
    v = np.tanh(a.v)
    return V(v, a.e * (1 - v * v) + E_TANH * U * np.abs(v))


def vsigmoid(a):
    """sigmoid_f of csrc/common.hip.h: e = __expf(-|x|), s = 1 / (1 + e), x >= 0 ? s : e s.  x = 0: e = 1, 1 + 1 = 2, 1 / 2 -- all exact."""
    ex = vexp(V(-np.abs(a.v), a.e), native=True)
    s = 1.0 / (1.0 + ex)
    r = vwhere(a.v >= 0, s, ex * s)
    r.v = 1.0 / (1.0 + np.exp(-a.v))                        # the same number, as the oracle writes it
    return vwhere(a.v == 0, V(0.5), r)


def vsum(a, axis, depth):
    """a fixed-order fp32 reduction whose longest chain of adds is `depth`"""
    return V(a.v.sum(axis), a.e.sum(axis) + depth * U * np.abs(a.v).sum(axis))


def vstack(vs, axis=-1):
    return V(np.stack([x.v for x in vs], axis), np.stack([x.e for x in vs], axis))


# ================================================================================================================ comparison
def judge(got, ref):
    """got: device values (any float array); ref = (lo, hi, e).  -> (worst error / bound, flat index of it).  An element passes if it lies in
    [lo - e, hi + e]; a non-finite element, or an error where the bound is zero, is infinitely bad.  The ONE comparison of the GPU test and of the
    mutant test."""
    lo, hi, e = ref
    got = np.asarray(got, dtype=np.float64).reshape(lo.shape)
    over = np.maximum(np.maximum(lo - got, got - hi), 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(over == 0, 0.0, over / e)
    ratio = np.where(np.isfinite(got), ratio, np.inf)
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    i = int(np.argmax(ratio)) if ratio.size else 0
    return (float(ratio.reshape(-1)[i]) if ratio.size else 0.0), i


def exact(x):
    """(lo, hi, e) of a V without alternatives"""
    return x.v, x.v, x.e


# ================================================================================================================ STN
def _bias(i, n):
    """bias = (2 - r) i / (n - 1) - (1 - r/2), r = .5.  Value: rounded to fp32 from float64 as the oracle's table; device: 1.5f * i (exact) / (n - 1)
    (divide) - 0.75f (one rounding); + u for the table's own rounding"""
    i = np.asarray(i, dtype=np.float64)
    q = 1.5 * i / (n - 1)
    ref = f32(q - 0.75)
    return V(ref, U * (E_DIV * np.abs(q) + 2 * np.abs(ref)))


def _lin(i, n):
    """np.linspace(-1, 1, n)[i] rounded to fp32 (the oracle's grid); device: -1.f + 2.f * i / (n - 1): a divide and an add, + u for the table's rounding"""
    i = np.asarray(i)
    if n == 1:
        return V(np.full(i.shape, -1.0))
    tab = f32(np.linspace(-1.0, 1.0, n))
    g = np.where(i < n, tab[np.minimum(i, n - 1)], f32(-1.0 + 2.0 * i / (n - 1)))
    return V(g, U * (E_DIV * np.abs(g + 1) + 2 * np.abs(g)))


class _Cell:
    pass


def _stn_cell(z, Hc, Wc, inverse, mut):
    B = z.shape[0]
    Bp = Hc * Wc
    zz = z.reshape(B, Bp, 4)
    cell = np.arange(Bp)
    d = Hc if mut == "cell_hc" else Wc
    ci = cell // d
    cj = cell - ci * d
    by, bx = _bias(ci, Hc), _bias(cj, Wc)
    if mut == "bxby":
        bx, by = by, bx
    c = _Cell()
    c.s0, c.s1 = vsigmoid(V(zz[..., 0])), vsigmoid(V(zz[..., 1]))
    c.th2, c.th3 = vtanh(V(zz[..., 2])), vtanh(V(zz[..., 3]))
    c.sxr, c.syr = c.s0.x2(0.5), c.s1.x2(0.5)
    c.txr, c.tyr = c.th2.x2(0.5) + bx[None], c.th3.x2(0.5) + by[None]
    if inverse:
        eps = V(0.0) if mut == "no_eps" else c32(1e-5)
        c.ex, c.ey = c.sxr + eps, c.syr + eps
        c.tx, c.ty = (-c.txr) / c.ex, (-c.tyr) / c.ey
        c.sx, c.sy = 1.0 / c.ex, 1.0 / c.ey
    else:
        c.sx, c.sy, c.tx, c.ty = c.sxr, c.syr, c.txr, c.tyr
    bty, btx = (c.tyr + 1.0).x2(0.5), (c.txr + 1.0).x2(0.5)
    c.bbox = vstack([bty - c.syr.x2(0.5), btx - c.sxr.x2(0.5), bty + c.syr.x2(0.5), btx + c.sxr.x2(0.5)])
    return c


def _axis(xv, m, n, choice, mut_unclipped, drop):
    """one axis of stn_tap: -> (i0, i1 int, w0, w1 float64, fold mask, reach mask).  choice: which side the floor takes at a fold (0: x >= k)"""
    k = np.rint(xv)
    fold = (np.abs(xv - k) <= m) & (k >= 0) & (k <= n - 1) & (m > 0)
    x0 = np.where(fold, k - choice, np.floor(xv))
    x1 = x0 + 1
    x0c, x1c = np.clip(x0, 0, n - 1), np.clip(x1, 0, n - 1)
    if mut_unclipped:
        w0, w1 = x1 - xv, xv - x0
    else:
        w0, w1 = x1c - xv, xv - x0c
    if drop and not mut_unclipped:
        same = x0c == x1c
        w0, w1 = np.where(same, 0.0, w0), np.where(same, 0.0, w1)
    reach = (xv + m >= 0) & (xv - m <= n - 1)
    return x0c.astype(np.int64), x1c.astype(np.int64), w0, w1, fold, reach


def _stn_core(img, z, Ho, Wo, inverse, g, need_img, mut, choice):
    img, z = np.asarray(img, np.float64), np.asarray(z, np.float64)
    B, Hc, Wc, _ = z.shape
    Bp = Hc * Wc
    H, W, C = img.shape[-3:]
    P = Ho * Wo
    c = _stn_cell(z, Hc, Wc, inverse, mut)
    p = np.arange(P)
    dd = Ho if mut == "pix_ho" else Wo
    oy = p // dd
    ox = p - oy * dd
    gx, gy = _lin(ox, Wo), _lin(oy, Ho)
    col = lambda t: t.reshape(B, Bp, 1)
    x = ((col(c.sx) * gx.reshape(1, 1, P) + col(c.tx)) + 1.0).x2(0.5) * float(W - 1)
    y = ((col(c.sy) * gy.reshape(1, 1, P) + col(c.ty)) + 1.0).x2(0.5) * float(H - 1)
    mx, my = x.e, y.e
    x0, x1, wx0, wx1, fx, rx = _axis(x.v, mx, W, choice[0], mut == "unclipped", mut != "nodrop_x")
    y0, y1, wy0, wy1, fy, ry = _axis(y.v, my, H, choice[1], mut == "unclipped", True)
    r = dict(cell=c, mx=mx, my=my, x=x.v, y=y.v, fold=(fx & ry) | (fy & rx), fold_x=fx & ry, fold_y=fy & rx, gx=gx, gy=gy)
    live = np.ones(P, bool)
    if mut == "skip_last_wave" and P % 64:
        live = p < P // 64 * 64
    bi = np.arange(B).reshape(B, 1, 1)
    ki = np.arange(Bp).reshape(1, Bp, 1)
    if inverse:
        tap = lambda yy, xx: img[bi, ki, yy, xx]
    else:
        tap = lambda yy, xx: img[bi, yy, xx]
    Ia, Ib, Ic, Id = tap(y0, x0), tap(y1, x0), tap(y0, x1), tap(y1, x1)                  # [B,Bp,P,C]
    X = Ia - Ib - Ic + Id
    e4 = lambda a: a[..., None]
    Wx0, Wx1, Wy0, Wy1 = (V(w, U * np.abs(w)) for w in (wx0, wx1, wy0, wy1))             # x1 - x, x - x0: one subtraction each
    wa, wb, wc, wd = Wx0 * Wy0, Wx0 * Wy1, Wx1 * Wy0, Wx1 * Wy1
    v4 = lambda t: V(e4(t.v), e4(t.e))
    if mut == "nodrop_x":                                   # the cancellation w I - w I of the clipped corners, as fp32 would leave it
        q = lambda t: t.astype(F32)
        o32 = ((q(wx0 * wy0)[..., None] * q(Ia) + q(wx0 * wy1)[..., None] * q(Ib)) + q(wx1 * wy0)[..., None] * q(Ic)) + q(wx1 * wy1)[..., None] * q(Id)
        out = V(o32.astype(np.float64))
    else:
        out = ((v4(wa) * Ia + v4(wb) * Ib) + v4(wc) * Ic) + v4(wd) * Id                  # tf.add_n order
    dox = e4(wy0) * (Ic - Ia) + e4(wy1) * (Id - Ib)
    doy = e4(wx0) * (Ib - Ia) + e4(wx1) * (Id - Ic)
    out.e = out.e + e4(mx) * np.abs(dox) + e4(my) * np.abs(doy) + e4(mx * my) * np.abs(X)
    out.v = np.where(live[None, None, :, None], out.v, np.nan)
    r["out"] = out.reshape(B, Bp, Ho, Wo, C)
    if g is None:
        return r
    g = np.asarray(g, np.float64).reshape(B, Bp, P, C) * live[None, None, :, None]
    gV = V(g)
    dx = vsum(gV * (v4(Wy0) * V(Ic - Ia) + v4(Wy1) * V(Id - Ib)), -1, C)
    dy = vsum(gV * (v4(Wx0) * V(Ib - Ia) + v4(Wx1) * V(Id - Ic)), -1, C)
    gX = (np.abs(g) * np.abs(X)).sum(-1)
    dx.e = dx.e + my * gX
    dy.e = dy.e + mx * gX
    fw, fh = float(W - 1), float(H - 1)
    if mut == "hw_swap":
        fw, fh = fh, fw
    dxn, dyn = dx.x2(0.5) * fw, dy.x2(0.5) * fh
    r["T"] = [dxn * gx.reshape(1, 1, P), dyn * gy.reshape(1, 1, P), dxn, dyn]           # the addends of gsx, gsy, gtx, gty per pixel
    if need_img:
        gi_v, gi_e, gi_a, gi_n = (np.zeros(img.shape) for _ in range(4))
        flat = lambda yy, xx: ((bi * Bp + ki) * H + yy) * W + xx if inverse else ((bi + 0 * ki) * H + yy) * W + xx
        for w, dwx, dwy, yy, xx in ((wa, wy0, wx0, y0, x0), (wb, wy1, wx0, y1, x0), (wc, wy0, wx1, y0, x1), (wd, wy1, wx1, y1, x1)):
            t = gV * v4(w)
            te = t.e + np.abs(g) * e4(mx * np.abs(dwx) + my * np.abs(dwy) + mx * my)
            idx = np.broadcast_to(flat(yy, xx)[..., None] * C + np.arange(C), t.v.shape).reshape(-1)
            on = (np.broadcast_to(e4(w.v), t.v.shape) != 0).reshape(-1)
            for acc, val in ((gi_v, t.v), (gi_e, te), (gi_a, np.abs(t.v)), (gi_n, np.ones(t.v.shape))):
                np.add.at(acc.reshape(-1), idx[on], val.reshape(-1)[on])
        r["g_img"] = V(gi_v, gi_e + gi_n * U * gi_a)
    return r


def _stn_chain(S, c, inverse, mut):
    """(gsx', gsy', gtx', gty') of the transformed parameters -> g_z_where [B,Bp,4]: the kernel's last thread"""
    dsxr, dsyr, dtxr, dtyr = S
    if inverse:
        k = 1.01 if mut == "cross101" else 1.0
        ex2, ey2 = c.ex * c.ex, c.ey * c.ey
        # sx' = 1/ex, tx' = -txr/ex:  d/dsxr = -gsx'/ex^2 + txr gtx'/ex^2 (the cross term);  d/dtxr = -gtx'/ex
        dsxr, dtxr = (-S[0]) / ex2 + ((S[2] * c.txr) / ex2).x2(k), (-S[2]) / c.ex
        dsyr, dtyr = (-S[1]) / ey2 + ((S[3] * c.tyr) / ey2).x2(k), (-S[3]) / c.ey
    return vstack([dsxr.x2(0.5) * c.s0 * (1.0 - c.s0), dsyr.x2(0.5) * c.s1 * (1.0 - c.s1),
                   dtxr.x2(0.5) * (1.0 - c.th2 * c.th2), dtyr.x2(0.5) * (1.0 - c.th3 * c.th3)])


def stn(img, z, Ho, Wo, inverse, g=None, need_img=True, mut=None):
    """-> dict: out, bbox, g_img, g_z as (lo, hi, e); fold [B,Bp,P] bool; mx, my.  With folds every output is the hull of the floor choices."""
    base = _stn_core(img, z, Ho, Wo, inverse, g, need_img, mut, (0, 0))
    runs = [base]
    if base["fold"].any() and mut is None:
        runs += [_stn_core(img, z, Ho, Wo, inverse, g, need_img, mut, ch) for ch in ((1, 0), (0, 1), (1, 1))]
    hull = lambda vs: (np.min([t.v for t in vs], 0), np.max([t.v for t in vs], 0), np.max([t.e for t in vs], 0))
    res = dict(fold=base["fold"], fold_x=base["fold_x"], fold_y=base["fold_y"], mx=base["mx"], my=base["my"], x=base["x"], y=base["y"], cell=base["cell"])
    res["out"] = hull([r["out"] for r in runs])
    res["bbox"] = exact(base["cell"].bbox)
    if g is None:
        return res
    if need_img:
        res["g_img"] = hull([r["g_img"] for r in runs])
    P = Ho * Wo
    depth = (P + 255) // 256 + 8                              # a thread's pixels, six shuffles, (r0 + r1) + (r2 + r3)
    lo, hi = [], []
    for j in range(4):
        tl, th, te = hull([r["T"][j] for r in runs])         # per pixel: every pixel may fold on its own
        red = depth * U * np.maximum(np.abs(tl), np.abs(th)).sum(-1)
        lo.append(V(tl.sum(-1), te.sum(-1) + red))
        hi.append(V(th.sum(-1), te.sum(-1) + red))
    c = base["cell"]
    corners = []
    for a in (lo, hi):
        for b in (lo, hi):                                    # g_z[0] mixes S0 and S2 (g_z[1]: S1 and S3): their four corners
            corners.append(_stn_chain([a[0], a[1], b[2], b[3]], c, inverse, mut))
    B, Hc, Wc, _ = np.asarray(z).shape
    res["g_z"] = tuple(t.reshape(B, Hc, Wc, 4) for t in hull(corners))
    return res


def stn_c(res, W, H):
    """the largest m / (u (|s g| + |t| + 1)(n - 1)/2) of a case: the `c` of the coordinate term"""
    c = res["cell"]
    den_x = U * (np.abs(res["x"] * 2 / (W - 1) - 1 - c.tx.v[..., None]) + np.abs(c.tx.v[..., None]) + 1) * (W - 1) / 2
    den_y = U * (np.abs(res["y"] * 2 / (H - 1) - 1 - c.ty.v[..., None]) + np.abs(c.ty.v[..., None]) + 1) * (H - 1) / 2
    return float(max((res["mx"] / den_x).max(), (res["my"] / den_y).max()))


# ---- cases
STN_SHAPES = [  # id, Hc, Wc, H, W, C, Ho, Wo, directions (False: the glimpse form, True: the renderer's inverse form)
    ("tiny_distinct", 2, 3, 5, 7, 3, 3, 5, (False, True)),            # all extents distinct; 15 pixels < one wave
    ("second_round", 3, 2, 7, 5, 1, 17, 19, (False, True)),           # 323 = 256 + 67: a second round that ends inside its second wave
    ("one_row", 2, 2, 6, 6, 4, 1, 9, (False, True)),                  # lin(n = 1) in y
    ("one_col", 2, 2, 6, 6, 4, 9, 1, (False, True)),                  # lin(n = 1) in x
    ("lds_8192", 4, 4, 32, 64, 4, 12, 10, (True,)),                   # H W C == SV_STN_LDS_FLOATS: the last size on the LDS path
    ("atomics_8200", 3, 2, 41, 50, 4, 9, 11, (True,)),                # 8200 floats: the inverse form on global atomics
    ("workload_glimpse", 4, 4, 48, 48, 3, 32, 32, (False,)),
    ("workload_render", 4, 4, 32, 32, 4, 48, 48, (True,)),
]
STN_FAMILIES = ("normal", "saturated", "crafted")
STN_SEEDS = {("second_round", True, "saturated"): 5, ("lds_8192", True, "saturated"): 2}     # (id, inverse, family) -> seed, where seed 1 has a fold


def stn_cases():
    return [(s, inv, fam) for s in STN_SHAPES for inv in s[8] for fam in STN_FAMILIES]


def stn_case_id(c):
    return "%s-%s-%s" % (c[0][0], "inv" if c[1] else "fwd", c[2])


def stn_inputs(case):
    """-> (img, z_where, g) float64 arrays of fp32 values"""
    (name, Hc, Wc, H, W, C, Ho, Wo, _), inverse, fam = case
    B = 1 if name.startswith("workload") and fam != "normal" else 3
    seed = STN_SEEDS.get((name, inverse, fam), 1)
    rng = np.random.default_rng([seed, sum(map(ord, name)), int(inverse)])
    Bp = Hc * Wc
    img = f32(rng.uniform(0, 1, (B, Bp, H, W, C) if inverse else (B, H, W, C)))
    g = f32(rng.standard_normal((B, Bp, Ho, Wo, C)))
    z = rng.standard_normal((B, Hc, Wc, 4)) * 1.5
    if fam == "saturated":                                            # entries +-20: sigmoid -> 2e-9 / 1, tanh -> +-1.  Per cell and axis the scale, the
        pick = rng.integers(0, 3, (B, Hc, Wc, 2))                     # translation or neither (both at once puts whole rows ON grid lines: the crafted
        sat = np.concatenate([pick == 0, pick == 1], -1)              # family's business)
        z = np.where(sat, np.where(rng.uniform(size=z.shape) < 0.5, -20.0, 20.0), z)
    elif fam == "crafted":                                            # sx = sy = .25 and t = the cell's bias, all exact in fp32: points ON pixel centres
        z = np.zeros_like(z)                                          # (forward form); the last cell pushed out of the image: xn = 1 exactly at gx = -1
        z[:, -1, -1, 2] = 20.0
    return img, f32(z), g


_STN_MEMO = {}


def stn_reference(case):
    """the reference of a case, computed once and shared (never modified)"""
    key = stn_case_id(case)
    if key not in _STN_MEMO:
        img, z, g = stn_inputs(case)
        (name, Hc, Wc, H, W, C, Ho, Wo, _), inverse, fam = case
        _STN_MEMO[key] = (img, z, g, stn(img, z, Ho, Wo, inverse, g))
    return _STN_MEMO[key]


def fold_pixels(case):
    """-> [k, 3] int array of (image, cell, output pixel): the sampling points of a case within m_x (m_y) of a grid line and in reach of the image, where the
    device's floor may land on either side.  Empty for every random case at its seed (asserted on the CPU); the crafted family's are the on-pixel points."""
    return np.argwhere(stn_reference(case)[3]["fold"])


# "unclipped": weights from the corners BEFORE the clip.  The clip moves a corner only where both corners end on one pixel, which is where the drop applies, so
# with the drop in place this is the same function; the mutant is the kernel such an author would have written: no drop (nothing cancels), the border pixel
# replicated outwards instead of zeros.
STN_MUTANTS = ["bxby", "cell_hc", "pix_ho", "unclipped", "nodrop_x", "cross101", "no_eps", "hw_swap", "skip_last_wave"]


# ================================================================================================================ renderer
MAXBP = 16


def render_scalars(zd, zp, zl, training, fold_up=False, mut=None):
    """per object: (z_pres V, s V, ds V, fold mask).  Test time: max(rint(sigmoid(logit)), 1e-8f); a sigmoid within its own error of .5 (but not the exact
    .5 of logit 0, which rounds half to even: 0) may round either way: `fold`, resolved by fold_up (a bool, or one per object)."""
    fold = None
    if not training:
        sg = vsigmoid(V(zl))
        r = np.rint(sg.v)
        fold = (sg.v != 0.5) & (np.abs(sg.v - 0.5) <= sg.e)
        r = np.where(fold, np.where(np.broadcast_to(np.asarray(fold_up, bool), r.shape), 1.0, 0.0), r)
        zpv = V(np.where(r > 0, 1.0, A_MIN32))
    else:
        zpv = V(zp)
    sgd = vsigmoid(V(-np.asarray(zd, np.float64)))
    ds = (-sgd) * (1.0 - sgd)
    if mut == "ds_sign":
        ds = -ds
    return zpv, sgd + 0.5, ds, fold


def render_gate_folds(obj, noise):
    """elements whose fp32 sum rgb + noise falls on the other side of a clip gate than the float64 sum: must be empty for a case to be usable"""
    if noise is None:
        return np.zeros(0, bool)
    C = obj.shape[-1] - 1
    s64 = obj[..., :C] + noise
    s32 = (obj[..., :C].astype(F32) + noise.astype(F32)).astype(np.float64)
    inside = lambda s: (s >= 0) & (s <= 1)
    return inside(s64) != inside(s32)


def render(obj, bg, zd, zp=None, zl=None, training=True, noise=None, g=None, mut=None, fold_up=False, amin=A_MIN32):
    """obj [B,Bp,H,W,C+1], bg [B,H,W,C], z_* [B,Bp] -> dict of V: out [B,H,W,C]; with g: g_obj, g_bg, g_zp [B,Bp], g_zd [B,Bp].
    amin: the alpha floor (the kernel's and TensorFlow's 1e-8f; the float64 oracle has 1e-8)."""
    obj, bg = np.asarray(obj, np.float64), np.asarray(bg, np.float64)
    B, Bp, H, Wd, C1 = obj.shape
    C, HW = C1 - 1, H * Wd
    ob = obj.reshape(B, Bp, HW, C1)
    bgv = bg.reshape(B, HW, C)
    nz = None if noise is None else np.asarray(noise, np.float64).reshape(B, Bp, HW, C)
    f = lambda t: None if t is None else np.asarray(t, np.float64).reshape(B, Bp)
    zpv, s, ds, fold = render_scalars(f(zd), f(zp), f(zl), training, fold_up, mut)
    strict = mut == "gates_exclusive"
    inside = (lambda v, lo, hi: (v > lo) & (v < hi)) if strict else (lambda v, lo, hi: (v >= lo) & (v <= hi))
    ks = list(range(Bp))
    if mut == "bp_pad":
        ks += [k % Bp for k in range(Bp, MAXBP)]                     # the unused slots of the 16 read as objects again
    per = []
    N = T = V(np.zeros((B, HW)))
    Uc = V(np.zeros((B, HW, C)))
    k1 = lambda t, k: V(t.v[:, k, None], t.e[:, k, None])
    for k in ks:
        ar = ob[:, k, :, C]
        a = V(np.clip(ar, amin, 1.0))
        t = k1(zpv, k) * a
        w = t * k1(s, k)
        if nz is None:
            v = V(ob[:, k, :, :C])
        elif mut == "noise_after_clip":
            v = V(ob[:, k, :, :C])
        else:
            v = V(ob[:, k, :, :C]) + nz[:, k]
        i = V(np.clip(v.v, 0.0, 1.0), v.e)
        if nz is not None and mut == "noise_after_clip":
            i = i + nz[:, k]
        N = N + w
        T = T + t * w
        Uc = Uc + V(w.v[..., None], w.e[..., None]) * i
        per.append((ar, a, t, w, v, i))
    D = N + c32(1e-8)
    A = T / D
    c3 = lambda t: V(t.v[..., None], t.e[..., None])
    out = c3(A) * (Uc / c3(D)) + (1.0 - c3(A)) * bgv
    live = np.ones(HW, bool)
    if mut == "chunk_tail" and HW % 256:
        live = np.arange(HW) < HW // 256 * 256
    out.v = np.where(live[None, :, None], out.v, np.nan)
    res = dict(out=out.reshape(B, H, Wd, C), fold=fold)
    if g is None:
        return res
    gp = V(np.asarray(g, np.float64).reshape(B, HW, C))
    cn = Uc / c3(D)
    g_bg = gp * (1.0 - c3(A))
    dA = V(np.zeros((B, HW)))
    dD = V(np.zeros((B, HW)))
    dU = []
    for c in range(C):
        dA = dA + gp[..., c] * (cn[..., c] - bgv[..., c])
        dU.append(gp[..., c] * A / D)
        dD = dD - gp[..., c] * A * Uc[..., c] / (D * D)
    dT = dA / D
    dD = dD - dA * T / (D * D)
    g_obj_v, g_obj_e = np.zeros((B, Bp, HW, C1)), np.zeros((B, Bp, HW, C1))
    azp, azd = [], []
    depth = (HW + 255) // 256 + 8                                     # a thread's pixels (or the chunks, added in order), six shuffles, the four waves
    for k in range(Bp):
        ar, a, t, w, v, i = per[k]
        dw = dD if mut == "no_dT" else dD + dT * t
        for c in range(C):
            dw = dw + dU[c] * i[..., c]
            gq = vwhere(inside(v.v[..., c], 0.0, 1.0), dU[c] * w, V(0.0))
            g_obj_v[:, k, :, c], g_obj_e[:, k, :, c] = gq.v, gq.e
        dt = dT * w + dw * k1(s, k)
        gq = vwhere(inside(ar, amin, 1.0), dt * k1(zpv, k), V(0.0))
        g_obj_v[:, k, :, C], g_obj_e[:, k, :, C] = gq.v, gq.e
        lv = live[None, :]
        azp.append(vsum((dt * a).x2(lv), -1, depth))
        azd.append(vsum((dw * t * k1(ds, k)).x2(lv), -1, depth))
    g_obj_v = np.where(live[None, None, :, None], g_obj_v, np.nan)
    g_bg.v = np.where(live[None, :, None], g_bg.v, np.nan)
    res.update(g_obj=V(g_obj_v, g_obj_e).reshape(B, Bp, H, Wd, C1), g_bg=g_bg.reshape(B, H, Wd, C), g_zp=vstack(azp), g_zd=vstack(azd))
    return res


RENDER_SHAPES = [  # id, B, Bp, H, W, C
    ("one_object", 3, 1, 1, 5, 1),            # Bp = 1, C = 1, five pixels: one partial wave.  With one object the depth weight cancels out of the output, so
                                              # g_zd's true value is rounding-sized and its bound is 70 .. 370 times its norm: here g_zd is only held to "about
                                              # zero"; the other three shapes are the ones that check it
    ("tail_299", 3, 6, 13, 23, 3),            # 299 = 256 + 43: a second chunk that ends inside its first wave
    ("one_chunk", 3, 16, 16, 16, 4),          # exactly one chunk; C = 4
    ("workload", 1, 16, 48, 48, 3),
]
RENDER_MODES = ("train", "train_noise", "test")
RENDER_SEEDS = {}
_nx = lambda v, d: float(np.nextafter(F32(v), F32(d)))
GATE_RGB = [0.0, 1.0, -0.0, _nx(0, -1), _nx(0, 1), _nx(1, 0), _nx(1, 2)]
GATE_ALPHA = [A_MIN32, 1.0, _nx(1e-8, 0), _nx(1e-8, 1), _nx(1, 0), _nx(1, 2)]
TEST_LOGITS = [0.0, 1e-7, -1e-7, 30.0, -30.0]


def render_inputs(shape, mode):
    """-> dict(obj, bg, zd, zp, zl, noise | None, g).  The uniform [-0.2, 1.2] family with a planted block at the start of the image AND at its end (the last
    pixels: beyond the first chunk where there is one): rgb and alpha on, and one fp32 step either side of, every clip gate; with noise, values the noise moves
    exactly onto and across a gate (sums that are exact in fp32).  Image 0 of a batch of 3 is all-absent: every z_pres at 1e-8f."""
    name, B, Bp, H, W, C = shape
    rng = np.random.default_rng([RENDER_SEEDS.get((name, mode), 1), sum(map(ord, name))])
    HW = H * W
    obj = rng.uniform(-0.2, 1.2, (B, Bp, HW, C + 1))
    noise = rng.standard_normal((B, Bp, HW, C)) * 0.01 if mode == "train_noise" else None
    n = min(HW, 7)
    for at in (slice(0, n), slice(HW - n, HW)):
        for b in range(B):
            k = b % Bp
            for c in range(C):
                obj[b, k, at, c] = np.roll(GATE_RGB, c + b)[:n]
            obj[b, k, at, C] = np.roll(GATE_ALPHA + [0.5], b)[:n]
            if noise is not None:                                        # .5 + (-.5) = 0, .25 + .75 = 1, .5 - .75 < 0, .5 + .75 > 1, 0 + tiny, 1 - tiny, inside
                base = np.array([0.5, 0.25, 0.5, 0.5, 0.0, 1.0, 0.5])[:n]
                mv = np.array([-0.5, 0.75, -0.75, 0.75, _nx(0, 1), -2.0 ** -24, 0.125])[:n]
                if Bp > 1:                                               # the next object carries the noise-moved values, this one keeps its gate values
                    obj[b, (k + 1) % Bp, at, 0] = base
                    noise[b, (k + 1) % Bp, at, 0] = mv
                    noise[b, k, at, :] = 0.0
                else:
                    obj[b, k, at, 0] = base
                    noise[b, k, at, 0] = mv
    d = dict(obj=f32(obj).reshape(B, Bp, H, W, C + 1), bg=f32(rng.uniform(0, 1, (B, H, W, C))), zd=f32(rng.standard_normal((B, Bp)) * 2),
             zp=f32(rng.uniform(0.01, 0.99, (B, Bp))), zl=f32(rng.standard_normal((B, Bp)) * 3), g=f32(rng.standard_normal((B, H, W, C))),
             noise=None if noise is None else f32(noise).reshape(B, Bp, H, W, C))
    if B > 1:
        d["zp"][0] = A_MIN32
    lg = np.array(TEST_LOGITS)
    for b in range(B):
        m = min(Bp, len(lg))
        d["zl"][b, :m] = f32(np.roll(lg, b)[:m])
    if B > 1:
        d["zl"][0, min(Bp, len(lg)):] = -30.0
        d["zl"][0, :min(Bp, len(lg))] = f32(np.array([-30.0, -1e-7, 0.0, -30.0, -30.0])[:min(Bp, len(lg))])   # test mode's all-absent image
    return d


_RENDER_MEMO = {}


def render_reference(shape, mode):
    """(inputs, [reference dict per alternative]): test mode with n folding logits in an image has 2^n alternatives"""
    key = (shape[0], mode)
    if key not in _RENDER_MEMO:
        d = render_inputs(shape, mode)
        if mode == "test":
            fold = render_scalars(d["zd"], None, d["zl"], False)[3]
            rank = np.cumsum(fold, -1) - 1                              # the j-th folding object of its image
            refs = [render(d["obj"], d["bg"], d["zd"], zl=d["zl"], training=False, fold_up=fold & ((c >> np.maximum(rank, 0)) & 1 > 0))
                    for c in range(2 ** int(fold.sum(-1).max()))]      # every image's folds up / down in every combination
        else:
            refs = [render(d["obj"], d["bg"], d["zd"], zp=d["zp"], training=True, noise=d["noise"], g=d["g"])]
        _RENDER_MEMO[key] = (d, refs)
    return _RENDER_MEMO[key]


RENDER_MUTANTS = ["gates_exclusive", "ds_sign", "no_dT", "noise_after_clip", "chunk_tail", "bp_pad"]


# ================================================================================================================ z_pres KL
def _safe_log(a):
    """tf_safe_log: log(v + 1e-8f); the replacement branch (NaN / inf) is not reachable for 0 <= v <= 1"""
    return vlog(a + c32(1e-8))


def _pg(ks, so_far, inv, m, mut):
    """max(k - so_far, 0) * inv, inv = 1.f / m: the numerator is a small integer (exact).  m * fl(1 / m) == 1 exactly for every m <= 16 with a correctly rounded
    divide (hipcc's default; tests/test_spair_glue_host.py checks the arithmetic fact), so an entry the sample rules out (1 - pg) becomes an exact zero, as in
    the float64 recursion -- otherwise 6e-8 of its mass would survive and be renormalised upwards step after step."""
    num = np.maximum(ks[None] - so_far, 0.0)
    pg = V(num) * inv
    return pg if mut == "inv_n" else vwhere(num == m, V(1.0), pg)


def zpres_kl(zp, logits, pre, prior_prob, temp, gscale, mut=None):
    """zp, logits, pre [B,n] -> dict of V: kl [B], g_pre [B,n], g_logits [B,n].  prior_prob, temp, gscale: as passed (rounded to fp32 here, as the call does)"""
    zp, logits, pre = (np.asarray(t, np.float64) for t in (zp, logits, pre))
    B, n = zp.shape
    prior_prob, Tt, gscale = float(F32(prior_prob)), float(F32(temp)), float(F32(gscale))
    cpp = 1.0 - V(prior_prob)
    ks = np.arange(MAXBP + 1, dtype=np.float64)
    pw = V(cpp.v ** ks, cpp.v ** ks * (ks * cpp.e / cpp.v + np.where(ks > 0, E_POW * U, 0.0)))        # powf(cpp, k); powf(x, 0) = 1 exactly
    top = MAXBP if mut == "support_maxbp" else n
    on = ks <= top
    # The count distribution is carried PROJECTIVELY: device dist_k = c true_k (1 + d_k) with a factor c common to all k and |d_k| <= rho.  A common factor
    # (1 - cpp, the error of a computed norm) cancels in the next normalisation, so only what differs between entries adds up: per step the factor's own
    # relative error, the product and the divide -- linear growth.  (Propagating absolute errors through dist / sum(dist) instead doubles them every step: the
    # numerator's and the denominator's errors are the same errors.)  Against the true normalised value the device's entry is then within 2 rho + (17 + 5) u:
    # the weighted mean of the (1 + d_j), the 17 adds of the sum and the divide.  Entries that are exactly zero stay exactly zero.
    d0 = np.where(on, pw.v, 0.0)
    d0 = d0 / d0.sum()
    rho = np.full((B, 1), float(np.where(on, pw.e / pw.v, 0.0).max()) + (E_DIV + 1) * U)
    dv = np.broadcast_to(d0, (B, MAXBP + 1)).copy()
    assert (1.0 - cpp.v) * np.where(on, pw.v, 0.0).sum() > 2e-6          # the kernel's fmaxf(norm, 1e-6f) is not in play
    dev = lambda: V(dv, dv * (2 * rho + (MAXBP + 1 + E_DIV) * U))
    so_far = np.zeros((B, 1))
    total = V(np.zeros(B))
    lt = vlog(V(Tt) + c32(1e-8))
    gp, gl = [], []
    for i in range(n):
        inv = V(1.0) / (float(n) if mut == "inv_n" else float(n - i))
        pg = _pg(ks, so_far, inv, n - i, mut)
        pz = vsum(dev() * pg, -1, MAXBP + 1)
        p = _safe_log(pz) - _safe_log(1.0 - pz)
        y, q = V(pre[:, i]), V(logits[:, i])
        yT = y * Tt
        eq, ep = vexp(-yT + q), vexp(-yT + p)
        log_post = lt - yT + q - (vlog(1.0 + eq + c32(1e-8))).x2(2.0)
        log_prior = lt - yT + p - (vlog(1.0 + ep + c32(1e-8))).x2(2.0)
        total = total + (log_post - log_prior)
        rq, rp = eq / (1.0 + eq + c32(1e-8)), ep / (1.0 + ep + c32(1e-8))
        gp.append((V(gscale).x2(2.0) * Tt) * (rq - rp))
        gl.append(V(gscale) * (1.0 - rq.x2(2.0)))
        s = (zp[:, i] > 0.5).astype(np.float64)[:, None]
        if mut == "sofar_early":
            so_far = so_far + s
            pg = _pg(ks, so_far, inv, n - i, mut)
        f = vwhere(s > 0, pg, 1.0 - pg)                                 # s pg + (1 - s)(1 - pg) with s in {0, 1}: a selection
        dv = f.v * dv
        live = dv > 0
        rho = rho + np.where(live, f.e / np.where(f.v > 0, f.v, 1.0), 0.0).max(-1, keepdims=True) + (1 + E_DIV) * U
        nn = dv.sum(-1, keepdims=True)
        assert mut is not None or (nn > 2e-6).all()                    # fmaxf(nn, 1e-6f) not in play
        nn = np.maximum(nn, 1e-6)
        dv = dv / nn
        if mut != "sofar_early":
            so_far = so_far + s
    return dict(kl=total, g_pre=vstack(gp), g_logits=vstack(gl))


ZPRES_B = [1, 64, 65, 130]
ZPRES_N = [1, 6, 16]
ZPRES_PRIOR = [0.99 / 1000, 0.01, 0.5, 0.99]
ZPRES_TEMP = [0.5, 1.0, 2.5]


def zpres_cases():
    """(B, n, prior, temp): every B, n, prior and temperature of the tables at least once, B x n in full"""
    out = []
    for bi, B in enumerate(ZPRES_B):
        for ni, n in enumerate(ZPRES_N):
            j = bi * len(ZPRES_N) + ni
            out.append((B, n, ZPRES_PRIOR[j % 4], ZPRES_TEMP[j % 3]))
    out += [(3, 16, p, t) for p in ZPRES_PRIOR for t in ZPRES_TEMP if (3, 16, p, t) not in out]
    return out


def zpres_inputs(case):
    B, n, prior, temp = case
    rng = np.random.default_rng([B, n, int(prior * 1e5), int(temp * 10)])
    pre = f32(rng.standard_normal((B, n)) * 2)
    logits = f32(rng.standard_normal((B, n)) * 2)
    zp = f32(1.0 / (1.0 + np.exp(-pre)))
    zp[0] = f32(0.9)                                                    # all on
    if B > 1:
        zp[1] = f32(0.1)                                                # all off
    return zp, logits, pre


ZPRES_MUTANTS = ["inv_n", "support_maxbp", "sofar_early"]


# ================================================================================================================ loss sums
def _safe_log_ok(v):
    """(V log(v + 1e-8f) or -100, ok): ok as the fp32 kernel decides it -- log of the fp32 sum v + 1e-8f is NaN below zero and -inf at zero"""
    s32 = (np.asarray(v.v, F32) + F32(1e-8)).astype(np.float64)
    ok = s32 > 0
    a = v + c32(1e-8)
    l = vlog(V(np.where(ok, a.v, 1.0), np.where(ok, a.e, 0.0)))
    return vwhere(ok, l, V(-100.0)), ok


def loss(mode, a, b, m2=0.0, s2=1.0, mut=None):
    """a, b [B,n] -> dict: sums (lo, hi, e) with the bound (n/256 + 10) u sum|t| -- a thread's n/256 serial adds, six shuffles, the four waves: n/256 + 8
    adds deep, and two more roundings' worth for the evaluation of an addend, |t| being the magnitudes of an addend's OWN addends (a log counts |log| + 1:
    its argument v + 1e-8f is rounded, which moves the log by u) --, ga / gb V (None where the kernel writes none)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    B, n = a.shape
    x, y = V(a), V(b)
    m2, s2 = float(F32(m2)), float(F32(s2))
    gate = (lambda ok, t: t) if mut == "ok_ignored" else (lambda ok, t: vwhere(ok, t, V(0.0)))
    if mode == 0:
        l0, ok0 = _safe_log_ok(y)
        l1, ok1 = _safe_log_ok(1.0 - y)
        t = -(x * l0 + (1.0 - x) * l1)
        mag = np.abs(a) * (np.abs(l0.v) + 1) + np.abs(1 - a) * (np.abs(l1.v) + 1)
        da = None
        safe = lambda d, ok: V(np.where(ok, d.v, 1.0), np.where(ok, d.e, 0.0))
        db = -(gate(ok0, x / safe(y + c32(1e-8), ok0 | (mut == "ok_ignored"))) - gate(ok1, (1.0 - x) / safe(1.0 - y + c32(1e-8), ok1 | (mut == "ok_ignored"))))
    elif mode == 1:
        lv, ok0 = _safe_log_ok(y * y)
        ex = vexp(lv)
        t = (1.0 + lv - x * x - ex).x2(-0.5)
        mag = 0.5 * (1 + np.abs(lv.v) + 1 + a * a + ex.v)
        da = V(a)
        den = y * y + c32(1e-8)
        db = gate(ok0, ((y.x2(2.0) / den) - (y.x2(2.0) * ex / den)).x2(-0.5))
    else:
        l1, ok0 = _safe_log_ok(y)
        ls2 = vlog(V(s2) + c32(1e-8))
        inv2 = 1.0 / (V(s2).x2(2.0) * s2)
        d = x - m2
        t = ls2 - l1 + (y * y + d * d) * inv2 - 0.5
        mag = np.abs(ls2.v) + 1 + np.abs(l1.v) + 1 + (b * b + d.v * d.v) * inv2.v + 0.5
        da = d.x2(2.0) * inv2
        safe = V(np.where(ok0 | (mut == "ok_ignored"), (y + c32(1e-8)).v, 1.0), np.where(ok0, (y + c32(1e-8)).e, 0.0))
        db = -gate(ok0, 1.0 / safe) + y.x2(2.0) * inv2
    tv = t.v
    if mut == "first256":
        keep = np.arange(n) < 256
        tv = tv * keep
        if da is not None:
            da.v = np.where(keep, da.v, np.nan)
        db.v = np.where(keep, db.v, np.nan)
    sums = tv.sum(-1)
    return dict(sums=(sums, sums, (n / 256.0 + 10) * U * mag.sum(-1)), ga=da, gb=db, t=t)


LOSS_MODES = {"xent": 0, "kl": 1, "kl_prior": 2}
LOSS_N = [1, 255, 256, 257, 6912]
LOSS_B = [1, 5]
LOSS_PRIOR = (3.7, 0.5)
PLANTED_PRED = [0.0, 1.0, 1e-9, 1 - 1e-7, 1.25, -0.25]                  # tf_safe_log's 1e-8 at work; the last two: a NaN log, replaced and gated


def loss_cases():
    return [(m, n, B) for m in LOSS_MODES for n in LOSS_N for B in LOSS_B if B == 1 or n in (257, 6912)]


def loss_inputs(case):
    """xent: labels and predictions in (0, 1) with the planted predictions in the FIRST and the LAST elements of an image; kl / kl_prior: N(0, 1) means and
    softplus sigmas with one sigma = 0 first and last (kl_prior also a negative sigma: the gated log)"""
    mode, n, B = case
    rng = np.random.default_rng([LOSS_MODES[mode], n, B])
    if mode == "xent":
        a, b = rng.uniform(0, 1, (B, n)), rng.uniform(0.001, 0.999, (B, n))
        plant = PLANTED_PRED
    else:
        a = rng.standard_normal((B, n))
        b = np.log1p(np.exp(rng.standard_normal((B, n)) - (1.0 if mode == "kl_prior" else 0.0)))
        plant = [0.0] if mode == "kl" else [0.0, -0.25]
    k = min(len(plant), n)
    b[:, :k] = plant[:k]
    if n >= 2 * len(plant):
        b[:, n - k:] = plant[:k][::-1]
    return f32(a), f32(b)


LOSS_MUTANTS = ["first256", "ok_ignored"]
