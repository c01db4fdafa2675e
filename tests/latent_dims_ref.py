"""float64 twin of the per-dimension latent report (include/splitvae.h: sv_latent_dims_prepare / _lse / _finish;
split_vae_amd/latent_dims.py), a per-element error bound derived from the kernel's own arithmetic (csrc/latent_dims.hip), the
kernel's fp32 arithmetic replayed operation by operation in NumPy, and mutants of the twin.  The inputs of the GPU tests are those
of tests/latent_info_ref.py (make_case with one block).

Definitions (one block of width L, images n with posterior mean mu_n and standard deviation sig_n; fp32 inputs taken exactly):
    lc_nj   = -log sig_nj - 1/2 log 2 pi                      fp32; an INPUT of the log-sum-exp, as are z, mu and rsig
    e_inj   = lc_nj - 1/2 ((z_ij - mu_nj) * rsig_nj)^2
    lse_ij  = logsumexp_n e_inj - log Nr
    own_ij  = lc_ij - 1/2 eps_ij^2,  prior_ij = -1/2 log 2 pi - 1/2 z_ij^2
    mean_j, var_j (population) of mu_.j;  KL_j = mean_i [1/2 (mu_ij^2 + sig_ij^2 - 1) - log sig_ij]
    MI_j = mean_i (own_ij - lse_ij),  dwKL_j = mean_i (lse_ij - prior_ij),  TC = mean_i (lse_block_i - sum_j lse_ij),  dwKL = sum_j dwKL_j

The twin's heavy part (Nq x Nr x L scores) runs in torch float64 on a device of the caller's choice, 32 dimensions at a time: the
CPU tests run it on the host, the GPU tests on the card (plain IEEE fp64 there too; it shares no code with the kernel under test).

The bound on |device lse_ij - twin lse_ij|, with u = 2^-24 (one fp32 rounding) and a_inj = ((z_ij - mu_nj) rsig_nj)^2:
    the device computes fl(fl(z - mu) * rsig) = w (1 + theta), |theta| <= 2 u (rsig is an input), squares it (relative 5 u, taken as
    6 u for the second-order terms) and rounds lc - 0.5 * square once (0.5 * square is exact):
        E_inj = 3 u a_inj + u |e_inj|                                                   (lc taken exactly: no error of its own)
    lse:  |d lse_ij| <= log sum_n w_n exp(E_inj)   (w = the softmax weights; exact, both signs, not first order)
      + the summation's own error.  A lane pushes the n <= CHUNK rows of a chunk in ceil(n / 8) groups.  Every term is
        exp2(fl(fl(e - m) * log2e)): an argument error of 3 u |d| nats and v_exp_f32's 1 ulp = 2 u; since the sum is >= 1 relative to
        its maximum, sum_k p_k |d_k| <= log n for the weights p_k, so all the terms together move the sum by at most
        (2 + 3 log n) u relative.  Per group the running sum passes through one rescale (exact when the maximum stays; otherwise a
        rounding u and the same (2 + 3 |d|) u on a part whose weight is at most n exp(-|d|): at most (3 + 3 log n) u) and 8 additions
        (u each, all terms non-negative):
            sum_error(n) = [ceil(n / 8) (8 + 3 + 3 log n) + 2 + 3 log n] u        relative, so -log(1 - .) in the logarithm;
        the chunk merge is fp64;
      + the flushed tail: terms more than 87 nats below the row maximum may be dropped whole (v_exp_f32 flushes below 2^-126, and a
        rescaled sum below that flushes too).
"""
import numpy as np
import torch

U = 2.0 ** -24
HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)
LOG2E32 = np.float32(1.44269504088896340736)
GR = 8                                   # reference rows per pushed group of the tile kernel
F32, F64 = np.float32, np.float64
ACTIVE = 0.01


# ---------------------------------------------------------------- the twin
def prepare(mu, sig, eps, lc=None, mutant=None):
    """mu, sig, eps [N, L] fp32 -> dict(lc (fp32: the correctly rounded value), lcerr [N,L] (what the device's lc may differ from it by:
    logf within 3 ulp = 6 u |log sig|, and one rounding to fp32 on either side -- two values half an ulp from their exact ones can
    land a whole ulp = 2 u |lc| apart), own [N,L] fp64 (from `lc` when given: the device's own bits), mean, var, kl [L] fp64)."""
    mu, sig, eps = (np.asarray(a, F32).astype(F64) for a in (mu, sig, eps))
    ls = np.log(sig)
    lc64 = -ls - HALF_LOG_2PI
    lc32 = lc64.astype(F32)
    used = lc32 if lc is None else np.asarray(lc, F32)
    N = mu.shape[0]
    mean = mu.mean(0)
    var = ((mu - mean) ** 2).sum(0) / (N - 1 if mutant == "sample_variance" else N)
    kl = (0.5 * (mu ** 2 + sig ** 2 - 1.0) - (0.0 if mutant == "kl_without_log_sig" else ls)).mean(0)
    return dict(lc=lc32, lcerr=2 * U * np.abs(lc64) + 6 * U * np.abs(ls) + 1e-30, own=used.astype(F64) - 0.5 * eps ** 2, mean=mean, var=var, kl=kl)


def sum_error(n):
    x = (np.ceil(n / GR) * (GR + 3 + 3 * np.log(max(n, 2))) + 2 + 3 * np.log(max(n, 2))) * U
    return -np.log1p(-x)


def lse(z, mu, rsig, lc, chunk=4096, mutant=None, device="cpu", step=32):
    """-> dict(lse, bound [Nq, L] fp64 NumPy).  z [Nq,L]; mu, rsig, lc [Nr,L]: fp32 values taken exactly.  `mutant`: one of MUTANTS,
    a deliberately wrong twin (its bound is meaningless)."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, F32))).to(device).double()     # noqa: E731
    z, mu, rsig, lc = t(z), t(mu), t(rsig), t(lc)
    Nq, L = z.shape
    Nr = mu.shape[0]
    if mutant == "dimension_shifted":
        mu, rsig, lc = (torch.roll(a, 1, 1) for a in (mu, rsig, lc))
    if mutant == "columns_mixed" and L > 1:
        perm = torch.arange(L, device=lc.device) ^ 1
        perm[perm >= L] = L - 1
        lc = lc[:, perm]
    if mutant == "sig_for_rsig":
        rsig = 1.0 / rsig
    if mutant == "lc_without_2pi":
        lc = lc + HALF_LOG_2PI
    if mutant == "lc_sign":
        lc = -(lc + HALF_LOG_2PI) - HALF_LOG_2PI
    if mutant == "query_row_shifted" and Nq > 1:
        z = torch.roll(z, 1, 0)
    half = 1.0 if mutant == "half_dropped" else 0.5
    lo, hi = 0, Nr
    if mutant == "last_partial_chunk_skipped" and Nr % chunk and Nr > chunk:
        hi = Nr // chunk * chunk
    if mutant == "first_reference_skipped" and Nr > 1:
        lo = 1
    logn = 0.0 if mutant == "log_n_forgotten" else np.log(Nq if mutant == "log_nq" else Nr)
    serr = sum_error(min(Nr, chunk))
    out, bound = torch.empty_like(z), torch.empty_like(z)
    for a in range(0, L, step):
        b = min(L, a + step)
        w = (z[:, None, a:b] - mu[None, lo:hi, a:b]) * rsig[None, lo:hi, a:b]
        acc = w.abs() if mutant == "square_dropped" else w * w
        e = lc[None, lo:hi, a:b] - half * acc
        m = e.max(1, keepdim=True)[0]
        p = torch.exp(e - m)
        S = p.sum(1)
        if mutant == "max_not_updated":              # the groups' sums added without rescaling to a common maximum
            n = e.shape[1]
            pad = torch.full((Nq, (-n) % GR, b - a), -np.inf, dtype=e.dtype, device=e.device)
            eg = torch.cat([e, pad], 1).reshape(Nq, -1, GR, b - a)
            mg = eg.max(2, keepdim=True)[0]
            out[:, a:b] = mg[:, 0, 0] + torch.log(torch.exp(eg - mg).sum((1, 2))) - logn
        else:
            out[:, a:b] = m[:, 0] + torch.log(S) - logn
        E = 3 * U * acc + U * e.abs()
        grow = (p * torch.exp(E.clamp(max=700.0))).sum(1) / S
        tail = torch.where(e - m < -87.0, p, torch.zeros_like(p)).sum(1) / S
        bound[:, a:b] = torch.log(grow) + serr + tail + 1e-12
    return dict(lse=out.cpu().numpy(), bound=bound.cpu().numpy())


MUTANTS = ["dimension_shifted", "columns_mixed", "sig_for_rsig", "lc_without_2pi", "lc_sign", "query_row_shifted", "half_dropped",
           "last_partial_chunk_skipped", "first_reference_skipped", "log_n_forgotten", "log_nq", "square_dropped", "max_not_updated"]
PREPARE_MUTANTS = ["sample_variance", "kl_without_log_sig"]


def finish(lse_, own, z, lse_block):
    """-> dict(mi, dwkl, mlse [L], tc, dwkl_sum) fp64"""
    lse_, own, lse_block = (np.asarray(a, F64) for a in (lse_, own, lse_block))
    prior = -HALF_LOG_2PI - 0.5 * np.asarray(z, F32).astype(F64) ** 2
    dwkl = (lse_ - prior).mean(0)
    return dict(mi=(own - lse_).mean(0), dwkl=dwkl, mlse=lse_.mean(0), tc=(lse_block - lse_.sum(1)).mean(), dwkl_sum=dwkl.sum())


def brute_force(z, mu, sig):
    """lse [Nq, L] straight from the definition, with sig (not rsig, not lc) in fp64: the twin's check"""
    z, mu, sig = (np.asarray(a, F32).astype(F64) for a in (z, mu, sig))
    e = -np.log(sig)[None] - HALF_LOG_2PI - 0.5 * ((z[:, None] - mu[None]) / sig[None]) ** 2
    m = e.max(1)
    return m + np.log(np.exp(e - m[:, None]).sum(1)) - np.log(mu.shape[0])


# ---------------------------------------------------------------- the kernel's fp32 arithmetic, operation by operation
def _f32(a):
    return np.asarray(a, F32)


def _exp2(x):
    with np.errstate(under="ignore"):
        return _f32(np.exp2(x.astype(F64)))


def lse_fp32(z, mu, rsig, lc, chunk=4096):
    """The arithmetic of ld_tile_kernel / ld_merge_kernel replayed in NumPy: fp32 subtract, multiply, square, one rounding of
    lc - 0.5 * square; groups of 8 consecutive rows of a chunk: group maximum, the running maximum, one rescale of the running sum,
    then one exp2 per element added in row order; the fp64 chunk merge."""
    z, mu, rsig, lc = (_f32(a) for a in (z, mu, rsig, lc))
    Nq, L = z.shape
    Nr = mu.shape[0]
    M, S = np.full((Nq, L), -np.inf), np.zeros((Nq, L))
    ninf = F32(-np.inf)
    with np.errstate(invalid="ignore", over="ignore"):
        for c0 in range(0, Nr, chunk):
            c1 = min(Nr, c0 + chunk)
            m, s = np.full((Nq, L), ninf, F32), np.zeros((Nq, L), F32)
            for g0 in range(c0, c1, GR):
                es = []
                for n in range(g0, min(g0 + GR, c1)):
                    u = _f32(_f32(z - mu[n]) * rsig[n])
                    h = _f32(u * u)
                    es.append(_f32(lc[n].astype(F64) - 0.5 * h.astype(F64)))
                gm = es[0]
                for e in es[1:]:
                    gm = np.maximum(gm, e)
                mn = np.maximum(m, np.maximum(gm, F32(-3.0e38)))
                acc = _f32(s * _exp2(_f32(_f32(m - mn) * LOG2E32)))
                for e in es:
                    acc = _f32(acc + _exp2(_f32(_f32(e - mn) * LOG2E32)))
                m, s = mn, acc
            m0, s0 = m.astype(F64), s.astype(F64)
            mn = np.maximum(M, m0)
            S = np.where(S > 0, S * np.exp(M - mn), 0.0) + np.where(s0 > 0, s0 * np.exp(m0 - mn), 0.0)
            M = np.where(s0 > 0, mn, M)
        return M + np.log(S) - np.log(Nr)
