"""CPU: the references of tests/latent_gemm_ref.py on hand-worked cases, the exactness property of the integer input family for every case
of its tables, the refusals of the latent block's entry points (include/splitvae.h: checked before anything is enqueued, so no GPU is
touched), and the invariants of the plan's K-slice pick."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import latent_gemm_ref as R  # noqa: E402

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16


def t64(rows):
    return torch.tensor(rows, dtype=F64)


# ---------------------------------------------------------------------------------------------------------------- references, by hand
def test_nt_by_hand():
    A, W = t64([[1, 2], [3, -4]]), t64([[5, 6], [-7, 8]])           # out[m][n] = sum_k A[m][k] W[n][k]
    assert R.nt(A, W).tolist() == [[17, 9], [-9, -53]]
    assert R.nt(A, W, bias=t64([1, -10])).tolist() == [[18, -1], [-8, -63]]
    assert R.nt(A, W, bias=t64([1, -10]), act="relu").tolist() == [[18, 0], [0, 0]]
    # the gate is applied last, and a mask of exactly zero (or below) closes it
    assert R.nt(A, W, mask=t64([[0.5, 0.0], [-1.0, 2.0]])).tolist() == [[17, 0], [0, -53]]


def test_nt_slabs_by_hand():
    A, W = t64([[1, 2], [3, -4]]), t64([[5, 6], [-7, 8]])
    s = R.nt_slabs(A, W, 2)                                          # slice 0: column 0 of both, slice 1: column 1
    assert s.tolist() == [[[5, -7], [15, -21]], [[12, 16], [-24, -32]]]
    assert torch.equal(s.sum(0), R.nt(A, W)) and torch.equal(R.nt_slabs(A, W, 1)[0], R.nt(A, W))


def test_slab_sum_f32_is_a_float32_sum_in_slice_order():
    # 2^24 + 1 is a tie that rounds to even (2^24): adding 1 twice to 2^24 changes nothing, adding 2^24 to 1 + 1 gives 2^24 + 2 exactly
    big, one = float(1 << 24), 1.0
    a = torch.tensor([[big, one], [one, one], [one, big]], dtype=F32)
    got = R.slab_sum_f32(a)
    assert got.dtype == F32 and got.tolist() == [big, big + 2.0]
    assert R.slab_sum_f32(torch.tensor([[-0.0]], dtype=F32)).tolist() == [0.0] and \
        not torch.signbit(R.slab_sum_f32(torch.tensor([[-0.0]], dtype=F32)))[0]      # the sum starts from +0.f


def test_tn_by_hand():
    X, dY = t64([[1, 2], [3, -4]]), t64([[5, 6], [-7, 8]])           # dW[k][n] = sum_m X[m][k] dY[m][n]
    dW, db = R.tn(X, dY)
    assert dW.tolist() == [[-16, 30], [38, -20]] and db.tolist() == [-2, 14]
    dW1, db1 = R.tn(X, dY, 1)
    assert dW1.tolist() == [[-16, 30]] and db1.tolist() == [-2, 14]


def test_gauss_bound_by_hand():
    ap = t64([[2.0]])
    assert R.gauss_bound(ap, 6).tolist() == [[8 * 2.0 ** -23 * 2.0]]
    assert R.gauss_bound(ap, 6, S=4).tolist() == [[12 * 2.0 ** -23 * 2.0]]
    assert R.gauss_bound(ap, 6, ref=t64([[-3.0]]), bf16_out=True).tolist() == [[8 * 2.0 ** -23 * 2.0 + 3.0 * 2.0 ** -8]]


# ---------------------------------------------------------------------------------------------------------------- the integer family is exact
EXACT = float(1 << 24)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_integer_family_stays_below_2_24(dtype):
    """Every partial sum of every contraction of the tables, in any order, is an integer below 2^24 in magnitude: the sum of the |products|
    (plus |bias|) of an output element bounds them all.  Operands are integers in -3 .. 3: exact in bf16."""
    P = R.phase_depth(dtype)
    worst = 0.0
    for c in R.NT_TYPED:
        A, W, bias, _ = R.nt_typed_inputs(c, "int", dtype)
        for t in (A, W, bias):
            if t is not None:
                assert torch.equal(t, t.round()) and float(t.abs().max()) <= 3 and torch.equal(t.to(BF16).to(F64), t)
        worst = max(worst, R.int_magnitude_bound((A, W, bias)))
    for nph, sk in R.NT_SLABS:
        worst = max(worst, R.int_magnitude_bound(R.nt_slab_inputs(R.NT_SLAB_M, R.NT_SLAB_N, nph * P * sk, "int", dtype)))
    for c in R.NT_TWIN:
        for i, q in enumerate(c["probs"]):
            worst = max(worst, R.int_magnitude_bound(R.nt_slab_inputs(q["M"], q["N"], R.case_K(q, dtype), "int", dtype, seed=31 + 2 * i)))
    for c in R.TN + [dict(M=R.TN_FOUR["M"], Kw=kw, N=n) for kw, n in R.TN_FOUR["shapes"]]:
        X, dY = R.tn_inputs(c["M"], c["Kw"], c["N"], "int", dtype)
        worst = max(worst, R.int_magnitude_bound((X.T.contiguous(), dY.T.contiguous())), float(dY.abs().sum(0).max()))
    print("largest sum of |products| over the tables: %d (2^24 = %d)" % (worst, 1 << 24))
    assert 0 < worst < EXACT
    assert 9 * 8192 + 3 < EXACT                                      # the a-priori figure: K <= 8192 terms of at most 3 * 3, plus a bias


# ---------------------------------------------------------------------------------------------------------------- refusals (no launch)
@pytest.fixture(scope="module")
def lib(lib_built):
    from split_vae_amd import _lib
    return _lib.load()


def _nt(dtype=1, **kw):
    """a valid problem (fake, aligned device addresses: a refusal never dereferences them) with fields overridden"""
    from split_vae_amd import _lib
    f = dict(A=0x10000, lda=256, W=0x20000, ldw=256, out=0x30000, ldo=128, bias=0x40000, mask=None, M=33, N=128, K=256, act=0, splitk=1,
             out_f32=0, slab_stride=0)
    f.update(kw)
    g = _lib.LatentNtProb()
    for k, v in f.items():
        setattr(g, k, v)
    return g


def _call_nt(lib, probs, dtype=1, bm=64, n=None):
    from split_vae_amd import _lib
    arr = (_lib.LatentNtProb * 2)(*probs)
    form = C.c_int32(-7)
    rc = lib.sv_latent_nt_gemm(arr, len(probs) if n is None else n, dtype, bm, C.byref(form), None)
    assert form.value == -7                                          # a refused call reports no form
    return rc


def test_nt_gemm_bad_arguments(lib):
    from split_vae_amd import _lib
    BAD = _lib.STATUS_BADARG
    assert lib.sv_latent_nt_gemm(None, 1, 1, 64, None, None) == BAD
    assert _call_nt(lib, [_nt()], n=0) == BAD and _call_nt(lib, [_nt(), _nt()], n=3) == BAD
    assert _call_nt(lib, [_nt()], bm=32) == BAD and _call_nt(lib, [_nt()], bm=96) == BAD
    assert _call_nt(lib, [_nt()], dtype=2) == BAD
    for kw in (dict(A=None), dict(W=None), dict(out=None), dict(M=0), dict(lda=128), dict(ldw=248), dict(ldo=64), dict(splitk=-1), dict(act=2)):
        assert _call_nt(lib, [_nt(**kw)]) == BAD, kw
        assert _call_nt(lib, [_nt(), _nt(**kw)]) == BAD, kw          # the second problem is checked too


@pytest.mark.parametrize("dtype", [1, 0], ids=["bf16", "f32"])
def test_nt_gemm_unsupported(lib, dtype):
    from split_vae_amd import _lib
    UNS = _lib.STATUS_UNSUPPORTED
    pe, P = (8, 128) if dtype == 1 else (4, 64)                      # elements of a 16-byte piece, K per phase
    cases = [dict(N=64, ldo=64), dict(N=192, ldo=192), dict(K=32, lda=256, ldw=256), dict(K=224), dict(splitk=3),
             dict(K=3 * P, lda=3 * P, ldw=3 * P, splitk=2, out_f32=1, slab_stride=33 * 128),       # slices of one and a half phases
             # each misalignment svk_nt_gemm_supported names
             dict(lda=256 + pe // 2), dict(ldw=256 + pe // 2), dict(ldo=130), dict(A=0x10008), dict(W=0x20004), dict(out=0x30008), dict(bias=0x40004),
             dict(mask=0x50008),
             # splitk > 1 without out_f32: the slices would overwrite each other
             dict(splitk=2),
             # slab strides: no multiple of 4 floats; smaller than a slab
             dict(out_f32=1, splitk=2, slab_stride=33 * 128 + 2), dict(out_f32=1, splitk=2, slab_stride=33 * 128 - 4), dict(out_f32=1, splitk=1, slab_stride=0)]
    for kw in cases:
        assert _call_nt(lib, [_nt(**kw)], dtype=dtype) == UNS, kw
        assert _call_nt(lib, [_nt(out_f32=1, slab_stride=33 * 128), _nt(**kw)], dtype=dtype) == UNS, kw


def test_slab_reduce_refusals(lib):
    from split_vae_amd import _lib

    def call(n=1, **kw):
        f = dict(slabs=0x10000, out=0x20000, S=2, M=33, ldo=128, slab_stride=33 * 128)
        f.update(kw)
        arr = (_lib.LatentReduceProb * 2)()
        for g in arr:
            for k, v in f.items():
                setattr(g, k, v)
        return lib.sv_latent_nt_slab_reduce(arr, n, None)

    assert lib.sv_latent_nt_slab_reduce(None, 1, None) == _lib.STATUS_BADARG
    for kw in (dict(n=0), dict(n=3), dict(slabs=None), dict(out=None), dict(S=0), dict(M=0), dict(ldo=0)):
        assert call(**kw) == _lib.STATUS_BADARG, kw
    for kw in (dict(ldo=130), dict(slab_stride=33 * 128 + 2), dict(slabs=0x10004), dict(out=0x20008)):
        assert call(**kw) == _lib.STATUS_UNSUPPORTED, kw
        assert call(n=2, **kw) == _lib.STATUS_UNSUPPORTED, kw


def test_tn_wgrad_refusals(lib):
    from split_vae_amd import _lib

    def call(n=1, dtype=1, **kw):
        f = dict(X=0x10000, ldx=256, dY=0x20000, ldy=128, dW=0x30000, dbias=None, M=96, Kw=256, Kw_real=251, N=128)
        f.update(kw)
        arr = (_lib.LatentTnProb * 4)()
        for g in arr:
            for k, v in f.items():
                setattr(g, k, v)
        return lib.sv_latent_tn_wgrad(arr, n, dtype, None)

    assert lib.sv_latent_tn_wgrad(None, 1, 1, None) == _lib.STATUS_BADARG
    for kw in (dict(n=0), dict(n=5), dict(dtype=3), dict(X=None), dict(dY=None), dict(dW=None), dict(ldx=128), dict(ldy=64)):
        assert call(**kw) == _lib.STATUS_BADARG, kw
    for dtype in (1, 0):
        pe = 8 if dtype == 1 else 4
        for kw in (dict(M=48), dict(M=0), dict(M=16), dict(Kw=192, Kw_real=192), dict(N=64, ldy=64), dict(N=192, ldy=192), dict(Kw_real=0), dict(Kw_real=257),
                   dict(ldx=256 + pe // 2), dict(ldy=128 + pe // 2), dict(X=0x10008), dict(dY=0x20004)):
            assert call(dtype=dtype, **kw) == _lib.STATUS_UNSUPPORTED, (dtype, kw)
            assert call(n=4, dtype=dtype, **kw) == _lib.STATUS_UNSUPPORTED, (dtype, kw)


def test_twin_sampling_refusals(lib):
    from split_vae_amd import _lib
    BAD = _lib.STATUS_BADARG

    def fwd(which=1, z_lp=0x90000, z_dtype=1, ldz=256, B=5, **kw):
        arr = (_lib.ReparamTwinFwd * 2)()
        for e, g in enumerate(arr):
            f = dict(pre=0x10000, bias_mean=0x20000, bias_sd=0x30000, eps=0x40000, eps_out=None, z_mean=0x50000, z_sig=0x60000, z=0x70000, kl=0x80000,
                     L=128, z_col=128 * e, S=2, slab_stride=5 * 256)
            if e == which:
                f.update(kw)
            for k, v in f.items():
                setattr(g, k, v)
        return lib.sv_reparam_kl_fwd_twin(arr, z_lp, z_dtype, ldz, B, 0, 0, 0, None)

    assert lib.sv_reparam_kl_fwd_twin(None, 0x90000, 1, 256, 5, 0, 0, 0, None) == BAD
    assert fwd(z_lp=None) == BAD and fwd(z_dtype=2) == BAD and fwd(B=0) == BAD and fwd(ldz=255) == BAD
    for which in (0, 1):
        for kw in (dict(pre=None), dict(bias_mean=None), dict(bias_sd=None), dict(z_mean=None), dict(z_sig=None), dict(z=None), dict(kl=None), dict(L=0), dict(S=-1),
                   dict(z_col=-1), dict(z_col=136)):
            assert fwd(which=which, **kw) == BAD, (which, kw)

    def bwd(which=1, g_dtype=1, B=5, **kw):
        arr = (_lib.ReparamTwinBwd * 2)()
        for e, g in enumerate(arr):
            f = dict(dz=0x10000, dz2=0x20000 if e else None, z_mean=0x30000, z_sig=0x40000, eps=0x50000, g_pre=0x60000, ld_dz=256, ld_dz2=128, L=128, S=2, S2=4 * e,
                     stride=5 * 256, stride2=5 * 128)
            if e == which:
                f.update(kw)
            for k, v in f.items():
                setattr(g, k, v)
        return lib.sv_reparam_kl_bwd_twin(arr, 0.5, g_dtype, B, None)

    assert lib.sv_reparam_kl_bwd_twin(None, 0.5, 1, 5, None) == BAD
    assert bwd(g_dtype=2) == BAD and bwd(B=0) == BAD
    for which in (0, 1):
        for kw in (dict(dz=None), dict(z_mean=None), dict(z_sig=None), dict(eps=None), dict(g_pre=None), dict(L=0), dict(S=-1), dict(ld_dz=64)):
            assert bwd(which=which, **kw) == BAD, (which, kw)
    assert bwd(which=1, ld_dz2=64) == BAD and bwd(which=1, S2=0) == BAD


# ---------------------------------------------------------------------------------------------------------------- the plan's K-slice pick
def test_pick_splitk_invariants(lib):
    n = 0
    for M in (1, 8, 32, 33, 64, 70, 96, 128, 256, 500, 512, 2048):
        for N in (128, 256, 512, 1024):
            for K in (128, 256, 384, 512, 640, 896, 1024, 2048, 2176, 4096, 8192, 32768):
                for nprob in (1, 2):
                    s = lib.sv_latent_nt_pick_splitk(M, N, K, nprob)
                    assert 1 <= s <= K // 128 and K % s == 0 and (K // s) % 128 == 0, (M, N, K, nprob, s)
                    n += 1
    assert n == 12 * 4 * 12 * 2
    # a shape the kernels do not take: one slice
    assert lib.sv_latent_nt_pick_splitk(64, 64, 8192, 2) == 1 and lib.sv_latent_nt_pick_splitk(64, 128, 64, 2) == 1
    # the two launches the GPU test leaves to the plan's pick (tests/latent_gemm_ref.py: NT_TWIN "plan_pick")
    assert lib.sv_latent_nt_pick_splitk(32, 256, 2048, 2) == 16 and lib.sv_latent_nt_pick_splitk(64, 512, 8192, 2) == 32
