"""GPU: the latent block's kernels (csrc/latent_gemm.hip and the S > 0 branches of the twin Sampling + KL kernels of csrc/pointwise.hip) one
by one through their direct entry points (include/splitvae.h: sv_latent_*, sv_reparam_kl_*_twin), element by element against the float64
restatements of tests/latent_gemm_ref.py, at the smallest shapes at which each of their paths is live (the case tables there).

Two input families per case (latent_gemm_ref.py says why each is needed):
  int     operands in -3 .. 3: every partial sum is an integer below 2^24, so the kernel's fp32 result must equal the reference BIT FOR BIT
          (a typed bf16 output: the reference rounded once to bf16, round to nearest even) -- one dropped product, one wrong row, one
          transposed fragment shows;
  gauss   standard normal operands, |got - ref64| <= latent_gemm_ref.gauss_bound per element -- a product that is not exact fp32 shows.
Every output buffer is larger than the kernel's output and pre-filled: rows >= M, columns N .. ldo-1, rows >= Kw_real of dW and
everything behind the last slab must keep their sentinel bits; slab buffers start as NaN, so an element of [S][M][N] that no workgroup
writes shows (the design has no zero fill); padding columns of the operands hold NaN, so a read outside the stated extents shows.
`form` assertions hold each case to the kernel it is meant for.  Every compared figure is printed before it is asserted (pytest -s).
Measured on MI355X: LAB_NOTES.md, "Latent-block GEMMs: kernel-level parity"."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import latent_gemm_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

F64, F32, BF16, I32, I16 = torch.float64, torch.float32, torch.bfloat16, torch.int32, torch.int16
DTYPES = [pytest.param(BF16, id="bf16"), pytest.param(F32, id="f32")]
FAMILIES = ["int", "gauss"]
NAN = float("nan")
SENTINEL = -777.0


@pytest.fixture(scope="module")
def ops(lib_built):
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from split_vae_amd import ops as o
    return o


def dev(t, dtype=F32):
    return t.to(dtype).cuda().contiguous()


def filled(shape, dtype=F32, value=SENTINEL):
    return torch.full(shape, value, dtype=dtype, device="cuda")


def bits(t):
    t = t.detach().contiguous()
    return t.view(I16 if t.dtype == BF16 else I32).cpu()


def same_bits(what, got, want):
    g, w = bits(got), bits(want.to(got.dtype))
    bad = int((g != w).sum())
    print("%-72s bit mismatches %d of %d" % (what, bad, g.numel()))
    assert g.shape == w.shape and bad == 0, (what, bad, "first at flat index %d" % int((g != w).flatten().nonzero()[0]) if bad else "")


def untouched(what, buf, before, keep):
    """the elements of `buf` selected by the boolean mask `keep` (same shape) still hold the bits of `before`"""
    k = keep.cpu()
    bad = int((bits(buf)[k] != bits(before)[k]).sum())
    print("%-72s sentinel elements overwritten %d of %d" % (what, bad, int(k.sum())))
    assert bad == 0, what


WORST = {}     # kernel -> worst err / bound of the Gaussian family (printed per check; LAB_NOTES.md records the maxima)


def check(what, kernel, family, got, ref, absprod, Kc, S=0):
    """got (device, fp32 or bf16) against the float64 reference `ref`: bitwise (int family) or within gauss_bound"""
    if family == "int":
        assert torch.equal(ref, ref.round()) and float(absprod.max()) < 2 ** 24
        want = (ref + 0.0).to(F32)                                   # exact: integers below 2^24 (+ 0.0: a zero is +0, as a sum that starts from +0.f)
        same_bits(what, got, want.to(got.dtype))                     # bf16: torch rounds to nearest even
        return
    g = got.detach().to(F64).cpu()
    assert bool(torch.isfinite(g).all()), what
    err = (g - ref).abs()
    bound = R.gauss_bound(absprod, Kc, S, ref=ref, bf16_out=got.dtype == BF16)
    ratio = float((err / bound.clamp_min(1e-300)).max())
    WORST[kernel] = max(WORST.get(kernel, 0.0), ratio)
    print("%-72s worst err / bound %.4f (K_c %d, S %d; running worst of %s: %.4f)" % (what, ratio, Kc, S, kernel, WORST[kernel]))
    assert bool((err <= bound).all()), (what, ratio, int((err / bound.clamp_min(1e-300)).argmax()))


def absprod_nt(A, W, bias=None):
    m = A.abs() @ W.abs().T
    return m if bias is None else m + bias.abs()[None, :]


def nt_kernel_name(form, dtype, bm):
    return "%s<%s,%d>" % ("nt_gemm_ring_kernel" if form else "nt_gemm_kernel", "bf16" if dtype == BF16 else "float", bm)


# ---------------------------------------------------------------------------------------------------------------- nt, typed output
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", R.NT_TYPED, ids=[c["id"] for c in R.NT_TYPED])
def test_nt_typed(ops, case, dtype, family):
    M, N, K = case["M"], case["N"], R.case_K(case, dtype)
    A, W, bias, mask = R.nt_typed_inputs(case, family, dtype)
    lda, ldo = K + case.get("lda_pad", 0), N + case.get("ldo_pad", 0)
    Ab = filled((M, lda), dtype, NAN)
    Ab[:, :K] = dev(A, dtype)
    Wd = dev(W, dtype)
    out = filled((M + 3, ldo), dtype)
    before = out.clone()
    prob = dict(A=Ab[:, :K], W=Wd, out=out, ldo=ldo, act=case.get("act"))
    if bias is not None:
        prob["bias"] = dev(bias)
    if mask is not None:
        mb = filled((M, ldo), dtype, NAN)
        mb[:, :N] = dev(mask, dtype)
        prob["mask"] = mb
    form, sk = ops.latent_nt_gemm([prob], dtype, bm=case["bm"])
    torch.cuda.synchronize()
    assert form == 0 and sk == [1]                                   # typed outputs: the one-slot kernel
    ref = R.nt(A, W, bias, case.get("act"), mask)
    check("nt typed %s" % case["id"], nt_kernel_name(0, dtype, case["bm"]), family, out[:M, :N], ref, absprod_nt(A, W, bias), K)
    keep = torch.ones(out.shape, dtype=torch.bool)
    keep[:M, :N] = False
    untouched("nt typed %s: rows >= M, columns N .. ldo-1" % case["id"], out, before, keep)


# ---------------------------------------------------------------------------------------------------------------- nt, K-slice slabs
def run_slabs(ops, probs_in, dtype, bm, family, tag, want_form, want_splitk=None):
    """One launch of 1 or 2 slab problems (dicts M, N, K, splitk, A, W as float64) into NaN-filled buffers; checks every slab element and
    that nothing else was written.  Returns the buffers and the (M, N, S, stride) of each problem."""
    probs, bufs, geo = [], [], []
    for q in probs_in:
        M, N = q["M"], q["N"]
        S_alloc = q["splitk"] if q["splitk"] else ops.latent_nt_pick_splitk(M, N, q["K"], len(probs_in))
        stride = M * N + 8                                           # a gap between the slabs: it must stay as it is
        buf = filled((S_alloc * stride + 64,), F32, NAN)
        probs.append(dict(A=dev(q["A"], dtype), W=dev(q["W"], dtype), out=buf, ldo=N, splitk=q["splitk"], out_f32=1, slab_stride=stride))
        bufs.append(buf)
        geo.append((M, N, S_alloc, stride))
    form, sk = ops.latent_nt_gemm(probs, dtype, bm=bm)
    torch.cuda.synchronize()
    print("%s: form %d, splitk %s" % (tag, form, sk))
    assert form == want_form, (tag, form)
    assert sk == [g[2] for g in geo] and (want_splitk is None or sk == want_splitk), (tag, sk)
    for i, (q, buf, (M, N, S, stride)) in enumerate(zip(probs_in, bufs, geo)):
        Kc = q["K"] // S
        ref = R.nt_slabs(q["A"], q["W"], S)
        got = torch.stack([buf[s * stride:s * stride + M * N].view(M, N) for s in range(S)])
        assert not bool(torch.isnan(got).any()), "%s problem %d: a slab element was never written" % (tag, i)
        ap = torch.stack([absprod_nt(q["A"][:, s * Kc:(s + 1) * Kc], q["W"][:, s * Kc:(s + 1) * Kc]) for s in range(S)])
        check("%s problem %d slabs [%d][%d][%d]" % (tag, i, S, M, N), nt_kernel_name(form, dtype, bm), family, got, ref, ap, Kc)
        keep = torch.ones(buf.shape, dtype=torch.bool)
        for s in range(S):
            keep[s * stride:s * stride + M * N] = False
        untouched("%s problem %d: gaps between the slabs and everything behind the last" % (tag, i), buf, filled(buf.shape, F32, NAN), keep)
    return bufs, geo


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nph,splitk", R.NT_SLABS)
def test_nt_slabs_ring_and_one_slot(ops, nph, splitk, dtype, family):
    """bm = 64: the ring kernel from two phases per slice on (nph = 2 is shorter than the three-slot ring, 4, 5 and 8 wrap it), the one-slot
    kernel at one; bm = 128: always the one-slot kernel.  Both contract K in the same order with the same MFMA per element (phases ascending,
    the four 16-B piece groups of a phase ascending), so their slabs must agree bit for bit in BOTH families."""
    M, N, K = R.NT_SLAB_M, R.NT_SLAB_N, nph * R.phase_depth(dtype) * splitk
    A, W = R.nt_slab_inputs(M, N, K, family, dtype)
    q = [dict(M=M, N=N, K=K, splitk=splitk, A=A, W=W)]
    b64, _ = run_slabs(ops, q, dtype, 64, family, "nt slabs nph %d splitk %d bm 64" % (nph, splitk), 0 if nph == 1 else 1)
    b128, _ = run_slabs(ops, q, dtype, 128, family, "nt slabs nph %d splitk %d bm 128" % (nph, splitk), 0)
    same_bits("nt slabs nph %d splitk %d: bm 64 (%s) == bm 128 (one slot)" % (nph, splitk, "one slot" if nph == 1 else "ring"), b64[0], b128[0])


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", R.NT_TWIN, ids=[c["id"] for c in R.NT_TWIN])
def test_nt_twin_launch_and_slab_reduce(ops, case, dtype, family):
    """Both problems of a launch (blockIdx.z ranges of different lengths, different N / M), then nt_slab_reduce_kernel over both (their
    slab counts and element counts differ): bitwise the float32 loop 0.f + s0 + s1 + ..., and within the bound of the whole contraction."""
    q = []
    for i, c in enumerate(case["probs"]):
        K = R.case_K(c, dtype)
        A, W = R.nt_slab_inputs(c["M"], c["N"], K, family, dtype, seed=31 + 2 * i)
        q.append(dict(M=c["M"], N=c["N"], K=K, splitk=c["splitk"], A=A, W=W))
    want_sk = [ops.latent_nt_pick_splitk(c["M"], c["N"], c["K"], 2) if c["splitk"] == 0 else c["splitk"] for c in q]
    bufs, geo = run_slabs(ops, q, dtype, 64, family, "nt twin %s" % case["id"], case["form"][0 if dtype == BF16 else 1], want_sk)
    outs, befores, rp = [], [], []
    for buf, (M, N, S, stride) in zip(bufs, geo):
        o = filled((M + 2, N), F32)
        outs.append(o)
        befores.append(o.clone())
        rp.append(dict(slabs=buf, out=o, S=S, M=M, ldo=N, slab_stride=stride))
    ops.latent_nt_slab_reduce(rp)
    torch.cuda.synchronize()
    for i, (c, buf, o, b4, (M, N, S, stride)) in enumerate(zip(q, bufs, outs, befores, geo)):
        slabs = torch.stack([buf[s * stride:s * stride + M * N].view(M, N) for s in range(S)]).cpu()
        same_bits("nt twin %s problem %d: slab reduce == float32 loop over %d slabs" % (case["id"], i, S), o[:M], R.slab_sum_f32(slabs))
        check("nt twin %s problem %d: reduced [%d][%d]" % (case["id"], i, M, N), "nt_slab_reduce_kernel", family, o[:M], R.nt(c["A"], c["W"]),
              absprod_nt(c["A"], c["W"]), c["K"] // S, S)
        keep = torch.zeros(o.shape, dtype=torch.bool)
        keep[M:] = True
        untouched("nt twin %s problem %d: reduce output rows >= M" % (case["id"], i), o, b4, keep)


@pytest.mark.parametrize("S", R.REDUCE_EXTRA_S)
def test_slab_reduce_one_and_seventeen_slabs(ops, S):
    M, ldo = 33, 128                                                 # 4224 floats: a last block that is partly idle
    stride = M * ldo + 4
    slabs = R.gauss((S, M, ldo), 41 + S).to(F32)
    buf = filled((S * stride + 16,), F32, NAN)
    for s in range(S):
        buf[s * stride:s * stride + M * ldo] = slabs[s].flatten().cuda()
    o = filled((M + 2, ldo), F32)
    b4 = o.clone()
    ops.latent_nt_slab_reduce([dict(slabs=buf, out=o, S=S, M=M, ldo=ldo, slab_stride=stride)])
    torch.cuda.synchronize()
    same_bits("slab reduce S = %d == float32 loop" % S, o[:M], R.slab_sum_f32(slabs))
    keep = torch.zeros(o.shape, dtype=torch.bool)
    keep[M:] = True
    untouched("slab reduce S = %d: output rows >= M" % S, o, b4, keep)


# ---------------------------------------------------------------------------------------------------------------- tn weight gradients
def tn_problem(c, family, dtype, seed=21):
    """device buffers of one weight-gradient problem (with their poison) + what is needed to judge it"""
    M, Kw, N, kr = c["M"], c["Kw"], c["N"], c.get("Kw_real", c["Kw"])
    X, dY = R.tn_inputs(M, Kw, N, family, dtype, seed)
    Xb = dev(X, dtype)
    if kr < Kw:
        Xb[:, kr:] = NAN                                             # the padding columns: no stored row may see them
    if c.get("col_half"):
        Yb = filled((M, 2 * N), dtype, NAN)                          # the heads' layout: this problem owns the second column half
        Yb[:, N:] = dev(dY, dtype)
        Yv = Yb[:, N:]
    else:
        Yv = dev(dY, dtype)
    dW, db = filled((Kw + 2, N), F32), (filled((N + 8,), F32) if c.get("dbias", True) else None)
    return dict(c=c, X=X, dY=dY, kr=kr, dW=dW, db=db, dW0=dW.clone(), db0=None if db is None else db.clone(),
                prob=dict(X=Xb, dY=Yv, dW=dW, dbias=db, Kw_real=kr))


def tn_check(tag, t, family, dtype):
    c, X, dY, kr, M, N = t["c"], t["X"], t["dY"], t["kr"], t["c"]["M"], t["c"]["N"]
    name = "tn_wgrad_kernel" if dtype == BF16 else "tn_wgrad_f32_kernel"
    dW_ref, db_ref = R.tn(X, dY, kr)
    check("%s dW [%d of %d][%d], M %d" % (tag, kr, c["Kw"], N, M), name, family, t["dW"][:kr], dW_ref, X[:, :kr].abs().T @ dY.abs(), M)
    keep = torch.zeros(t["dW"].shape, dtype=torch.bool)
    keep[kr:] = True
    untouched("%s dW rows >= Kw_real" % tag, t["dW"], t["dW0"], keep)
    if t["db"] is not None:
        check("%s dbias [%d]" % (tag, N), name + " (dbias)", family, t["db"][:N], db_ref, dY.abs().sum(0), M)
        keep = torch.zeros(t["db"].shape, dtype=torch.bool)
        keep[N:] = True
        untouched("%s dbias behind N" % tag, t["db"], t["db0"], keep)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", R.TN, ids=[c["id"] for c in R.TN])
def test_tn_wgrad(ops, case, dtype, family):
    t = tn_problem(case, family, dtype)
    ops.latent_tn_wgrad([t["prob"]], dtype)
    torch.cuda.synchronize()
    tn_check("tn %s" % case["id"], t, family, dtype)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_tn_wgrad_four_problems(ops, dtype, family):
    """One launch over four shapes: its grid is the largest problem's, the workgroups outside a smaller problem return before they write."""
    f = R.TN_FOUR
    ts = [tn_problem(dict(M=f["M"], Kw=kw, N=n, dbias=i != f["no_dbias"]), family, dtype, seed=51 + 2 * i) for i, (kw, n) in enumerate(f["shapes"])]
    ops.latent_tn_wgrad([t["prob"] for t in ts], dtype)
    torch.cuda.synchronize()
    for i, t in enumerate(ts):
        tn_check("tn four-problem launch, problem %d" % i, t, family, dtype)


# ---------------------------------------------------------------------------------------------------------------- twin Sampling + KL on slabs
def slab_buffer(slabs, stride):
    """float32 [S, B, C] slabs -> a NaN-filled device buffer holding them `stride` floats apart"""
    S, n = slabs.shape[0], slabs[0].numel()
    buf = filled((S * stride + 16,), F32, NAN)
    for s in range(S):
        buf[s * stride:s * stride + n] = slabs[s].flatten().cuda()
    return buf


@pytest.mark.parametrize("zdt", DTYPES)
@pytest.mark.parametrize("S", R.TWIN_FWD_S)
@pytest.mark.parametrize("L", R.TWIN_L, ids=["L128", "L64"])
@pytest.mark.parametrize("B", R.TWIN_B)
def test_reparam_kl_fwd_twin_on_slabs(ops, B, L, S, zdt):
    """reparam_kl_fwd_twin_kernel, S > 0: every output bit for bit what sv_reparam_kl_fwd gives on the float32 slice-order sum of the same
    slabs (that kernel is under float64 in tests/test_gpu_kernels.py: equality carries it over).  eps is given: the Philox path has its own test."""
    z_col = (8, 8 + L[0] + 8)
    ldz = z_col[1] + L[1] + 8
    z_lp = filled((B + 2, ldz), zdt)
    z_lp0 = z_lp.clone()
    nets, refs, outs = [], [], []
    for e in range(2):
        Le = L[e]
        stride = B * 2 * Le + 8
        slabs = (0.5 * R.gauss((S, B, 2 * Le), 61 + e)).to(F32)
        bias, eps = dev(R.gauss((2 * Le,), 63 + e)), dev(R.gauss((B, Le), 65 + e))
        o = {k: filled((B + 1, Le)) for k in ("eps_out", "z_mean", "z_sig", "z")}
        o["kl"] = filled((B + 3,))
        outs.append((o, {k: v.clone() for k, v in o.items()}))
        nets.append(dict(pre=slab_buffer(slabs, stride), bias_mean=bias[:Le], bias_sd=bias[Le:], eps=eps, L=Le, z_col=z_col[e], S=S, slab_stride=stride, **o))
        refs.append(ops.reparam_kl_fwd(dev(R.slab_sum_f32(slabs)), bias, eps, z_dtype=zdt, stream_id=e))
    ops.reparam_kl_fwd_twin(nets, z_lp, ldz, B)
    torch.cuda.synchronize()
    keep = torch.ones(z_lp.shape, dtype=torch.bool)
    for e in range(2):
        tag = "fwd twin B %d L %d S %d net %d" % (B, L[e], S, e)
        z_mean, z_sig, z, zl, kl, eps_out = refs[e]
        o, o0 = outs[e]
        for name, ref in (("z_mean", z_mean), ("z_sig", z_sig), ("z", z), ("eps_out", eps_out)):
            assert bool(torch.isfinite(ref).all())
            same_bits("%s %s" % (tag, name), o[name][:B], ref)
            same_bits("%s %s: the row behind B" % (tag, name), o[name][B:], o0[name][B:])
        same_bits("%s kl" % tag, o["kl"][:B], kl)
        same_bits("%s kl: behind B" % tag, o["kl"][B:], o0["kl"][B:])
        same_bits("%s z_lp columns [%d, %d)" % (tag, z_col[e], z_col[e] + L[e]), z_lp[:B, z_col[e]:z_col[e] + L[e]], zl)
        keep[:B, z_col[e]:z_col[e] + L[e]] = False
    untouched("fwd twin B %d: z_lp around the two networks' columns" % B, z_lp, z_lp0, keep)


@pytest.mark.parametrize("gdt", DTYPES)
@pytest.mark.parametrize("SS", R.TWIN_BWD_S, ids=["S2_S4", "S16_S1"])
@pytest.mark.parametrize("L", R.TWIN_L, ids=["L128", "L64"])
@pytest.mark.parametrize("B", R.TWIN_B)
def test_reparam_kl_bwd_twin_on_slabs(ops, B, L, SS, gdt):
    """reparam_kl_bwd_twin_kernel, S > 0, as the plan wires it: network 0 reads columns [0, Lg) of d1_x's input-gradient slabs (pitch Lg + Ll)
    and has no second addend, network 1 reads columns [Lg, Lg + Ll) of the same slabs plus d1_xh's slabs (their own count and stride).
    Bit for bit sv_reparam_kl_bwd on the separately pre-summed tensors."""
    S, S2 = SS
    Lg, Ll = L
    Lc = Lg + Ll
    kl_scale = 40.0 / B
    stride, stride2 = B * Lc + 8, B * Ll + 4
    sx = R.gauss((S, B, Lc), 71).to(F32)
    sxh = R.gauss((S2, B, Ll), 72).to(F32)
    bx, bxh = slab_buffer(sx, stride), slab_buffer(sxh, stride2)
    gz_x, gz_xh = dev(R.slab_sum_f32(sx)), dev(R.slab_sum_f32(sxh))
    nets, outs, refs = [], [], []
    for e, Le in enumerate(L):
        zm, eps = dev(R.gauss((B, Le), 73 + e)), dev(R.gauss((B, Le), 75 + e))
        zs = dev(torch.nn.functional.softplus(R.gauss((B, Le), 77 + e)))
        g = filled((B + 1, 2 * Le), gdt)
        outs.append((g, g.clone()))
        nets.append(dict(dz=bx if e == 0 else bx[Lg:], ld_dz=Lc, dz2=None if e == 0 else bxh, ld_dz2=0 if e == 0 else Ll, z_mean=zm, z_sig=zs, eps=eps,
                         g_pre=g, L=Le, S=S, stride=stride, S2=0 if e == 0 else S2, stride2=0 if e == 0 else stride2))
        dz = (gz_x[:, :Lg] if e == 0 else gz_x[:, Lg:]).contiguous()
        refs.append(ops.reparam_kl_bwd(dz, zm, zs, eps, kl_scale, g_dtype=gdt, dz2=None if e == 0 else gz_xh))
    ops.reparam_kl_bwd_twin(nets, kl_scale, gdt, B)
    torch.cuda.synchronize()
    for e in range(2):
        tag = "bwd twin B %d L %d (S, S2) %s net %d" % (B, L[e], SS, e)
        assert bool(torch.isfinite(refs[e].float()).all())
        same_bits("%s g_pre" % tag, outs[e][0][:B], refs[e])
        same_bits("%s g_pre: the row behind B" % tag, outs[e][0][B:], outs[e][1][B:])
