"""Plain float64 restatements of the latent block's kernels (split_vae_amd/csrc/latent_gemm.hip), the case tables of
tests/test_gpu_latent_gemm.py and the two input families those cases run on.  CPU only: torch as an array library.

Integer family: every operand entry is an integer in -3 .. 3 (bias too), so every product and every partial sum of a contraction is an
integer far below 2^24: fp32 accumulation is exact in ANY order, bf16 operands are exact, and the float64 result (exact as well: all values
are below 2^53) cast to float32 is the one right answer, bit for bit.  `int_magnitude_bound` is the property; tests/test_latent_gemm_host.py
checks it for every case of the tables, where the inputs are made.

Gaussian family: standard normal entries (rounded to bf16 first for the bf16 kernels: the reference sees what the kernel sees), judged per
element by `gauss_bound`."""
import torch

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16


def phase_depth(dtype):
    """K per LDS phase of the nt kernels: an LDS row is 256 bytes."""
    return 128 if dtype == BF16 else 64


# ---------------------------------------------------------------------------------------------------------------- references
def nt(A, W, bias=None, act=None, mask=None):
    """gate(act(A . W^T + bias)) in float64: A [M, K], W [N, K], bias [N], mask [M, N] (elements whose mask is not > 0 become zero)"""
    out = A.to(F64) @ W.to(F64).T
    if bias is not None:
        out = out + bias.to(F64)[None, :]
    if act == "relu":
        out = out.clamp_min(0.0)
    if mask is not None:
        out = torch.where(mask.to(F64) > 0, out, torch.zeros_like(out))
    return out


def nt_slabs(A, W, splitk):
    """[splitk][M][N] float64: slab s = the product over K slice s alone"""
    M, K = A.shape
    assert K % splitk == 0
    kc = K // splitk
    return torch.stack([A[:, s * kc:(s + 1) * kc].to(F64) @ W[:, s * kc:(s + 1) * kc].to(F64).T for s in range(splitk)])


def slab_sum_f32(slabs):
    """0.f + s0 + s1 + ... in float32, in slice order: what nt_slab_reduce_kernel and the twin kernels' S > 0 branches compute (IEEE adds:
    the same bits on any machine).  slabs: float32 [S, ...]."""
    assert slabs.dtype == F32
    acc = torch.zeros_like(slabs[0])
    for s in range(slabs.shape[0]):
        acc = acc + slabs[s]
    return acc


def tn(X, dY, Kw_real=None):
    """(dW [Kw_real, N], dbias [N]) = (X[:, :Kw_real]^T . dY, column sums of dY) in float64"""
    kr = X.shape[1] if Kw_real is None else Kw_real
    return X[:, :kr].to(F64).T @ dY.to(F64), dY.to(F64).sum(0)


def gauss_bound(absprod, Kc, S=0, ref=None, bf16_out=False):
    """The per-element bound of the Gaussian family: (Kc + S + 2) 2^-23 (|A| . |W|^T + |bias|), `absprod` being that last factor (float64),
    Kc the contraction length and S the number of slabs summed on top.  Derivation: a sum of n fp32 terms in any order is within
    (n - 1) u sum|t| of the exact sum to first order (u = 2^-24 for round to nearest); the products of an exact-fp32 MFMA carry one more
    rounding each, the bias add and the slab sums S + 1 more; 2^-23 instead of 2^-24 so that an accumulate that truncates instead of rounding
    still passes -- what must NOT pass is a reduced-precision product (tf32 / bf16x3: 2^-11 .. 2^-17 per product, against (Kc + 2) 2^-23 here).
    A typed bf16 output adds half a bf16 ulp of the result, 2^-8 |ref|, for its single rounding."""
    b = (Kc + S + 2) * 2.0 ** -23 * absprod
    if bf16_out:
        b = b + 2.0 ** -8 * ref.abs()
    return b


# ---------------------------------------------------------------------------------------------------------------- inputs
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def ints(shape, seed):
    """integers in -3 .. 3 as float64"""
    return torch.randint(-3, 4, shape, generator=_gen(seed)).to(F64)


def gauss(shape, seed, dtype=F32):
    """standard normal entries, rounded to the operand dtype, as float64"""
    return torch.randn(shape, generator=_gen(seed), dtype=F32).to(dtype).to(F64)


def operand(family, shape, seed, dtype):
    return ints(shape, seed) if family == "int" else gauss(shape, seed, dtype)


def relu_mask(shape, seed, dtype):
    """a post-ReLU Gaussian tensor: about half exact zeros (the ReLU gate of the `dgrad.head` form)"""
    return gauss(shape, seed, dtype).clamp_min(0.0)


def int_magnitude_bound(*contractions):
    """the largest sum of |products| (+ |bias|) any output element of the given (A, W[, bias]) contractions can reach, A [M, K], W [N, K]:
    an upper bound of every partial sum in every summation order"""
    worst = 0.0
    for c in contractions:
        A, W = c[0], c[1]
        m = A.abs().to(F64) @ W.abs().to(F64).T
        if len(c) > 2 and c[2] is not None:
            m = m + c[2].abs().to(F64)[None, :]
        worst = max(worst, float(m.max()))
    return worst


# ---------------------------------------------------------------------------------------------------------------- case tables
# K is given in phases: K = kp * phase_depth(dtype).  The smallest shapes at which each path of the kernels is live.
NT_TYPED = [   # out_f32 = 0, splitk = 1
    dict(id="m1_one_phase", M=1, N=128, kp=1, bm=64, bias=True, act="relu"),                      # one phase, 63 clamped rows
    dict(id="m33_pitches", M=33, N=256, kp=4, bm=64, bias=True, lda_pad=16, ldo_pad=4),           # one-slot multi-phase, M edge, pitches
    dict(id="m65_mask_bm128", M=65, N=128, kp=4, bm=128, mask=True),                              # the dgrad.head form
    dict(id="m130_two_tiles", M=130, N=256, kp=2, bm=128, bias=True),                             # two 128-row tiles, the second nearly empty
]
NT_SLAB_M, NT_SLAB_N = 33, 128
NT_SLABS = [(1, 8), (2, 4), (3, 2), (4, 2), (5, 1), (8, 1)]       # (phases per slice, slices): K = nph * P * splitk; bm = 64
# (the contraction of a slab is nph * P long: at most 512, the length the Gaussian bound is meant for, except bf16 at 5 and 8 phases -- 640 and
# 1024, which a ring that wraps needs; the bound's formula is the same there)
NT_TWIN = [    # two problems per launch; form: the kernel both must take (bf16, f32)
    dict(id="ring_n_and_split_differ", probs=[dict(M=40, N=256, kp=8, splitk=4), dict(M=40, N=128, kp=8, splitk=2)], form=(1, 1)),
    dict(id="one_phase_slices_force_one_slot", probs=[dict(M=40, N=128, kp=4, splitk=4), dict(M=70, N=128, kp=4, splitk=1)], form=(0, 0)),
    # splitk = 0: the plan's pick (16 and 32 slices: K / splitk = 128 and 256, one and two bf16 phases -> one-slot; two and four fp32 phases -> ring)
    dict(id="plan_pick", probs=[dict(M=32, N=256, K=2048, splitk=0), dict(M=64, N=512, K=8192, splitk=0)], form=(0, 1)),
]
REDUCE_EXTRA_S = [1, 17]       # 17: `#pragma unroll 4` leaves a remainder of one; also past the plan's fuse cap of 16
TN = [
    dict(id="minimum", M=32, Kw=128, N=128, dbias=True),
    dict(id="kw_real_251", M=96, Kw=256, Kw_real=251, N=128, dbias=True),         # unstored rows, NaN padding columns; bf16: a partial single phase
    dict(id="column_half", M=160, Kw=128, N=256, dbias=True, col_half=True),      # ldy = 2N, dY at column offset N; bf16: 2 phases, 32 valid rows in the last; f32: 5
    dict(id="no_dbias", M=256, Kw=128, N=128, dbias=False),                       # two full bf16 phases
    dict(id="three_phases", M=288, Kw=256, N=128, dbias=True),                    # bf16: 3 phases
]
TN_FOUR = dict(M=96, shapes=[(128, 128), (256, 128), (128, 256), (256, 256)], no_dbias=2)     # the grid is the largest problem's: the others return early
TWIN_B = [5, 33]
TWIN_L = [(128, 128), (64, 64)]          # 64: the kernels' j < L guards leave lanes idle
TWIN_FWD_S = [2, 16]
TWIN_BWD_S = [(2, 4), (16, 1)]


def case_K(c, dtype):
    return c["K"] if "K" in c else c["kp"] * phase_depth(dtype)


def nt_typed_inputs(c, family, dtype, seed=1):
    """(A [M, K], W [N, K], bias [N] | None, mask [M, N] | None) as float64"""
    K = case_K(c, dtype)
    A = operand(family, (c["M"], K), seed, dtype)
    W = operand(family, (c["N"], K), seed + 1, dtype)
    bias = operand(family, (c["N"],), seed + 2, F32) if c.get("bias") else None
    mask = relu_mask((c["M"], c["N"]), seed + 3, dtype) if c.get("mask") else None
    return A, W, bias, mask


def nt_slab_inputs(M, N, K, family, dtype, seed=11):
    return operand(family, (M, K), seed, dtype), operand(family, (N, K), seed + 1, dtype)


def tn_inputs(M, Kw, N, family, dtype, seed=21):
    return operand(family, (M, Kw), seed, dtype), operand(family, (M, N), seed + 1, dtype)
