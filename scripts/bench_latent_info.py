"""Cost of the aggregate-posterior information report (split_vae_amd/latent_info.py, csrc/latent_info.hip) at SVHN scale, in ONE
process: N = 26 032 samples scored under N = 26 032 posteriors, latent widths Lg + Ll = 128 + 128 and 256 + 256.

Synthetic posteriors in the shape a trained split VAE leaves: sig log-uniform in [1e-2, 1], means ~ N(0, I).  Between hipEvent
pairs, after warm-up, alternating inside a round:

  kernel_ms  one latent_info.information call, box to box: sv_latent_info_draw, sv_latent_info_lse (tile + merge kernels) and
             sv_latent_info_finish; lse_ms: the sv_latent_info_lse call alone (workspace allocated outside)
  torch_ms   the only other implementation that exists: the same DIRECT form ((z - mu) * rsig)^2 as a chunked torch composition on
             the device (query chunks x reference chunks of `--torch-q` x `--torch-r` rows, a streamed logaddexp over the chunks)

Each figure is the median of `--rounds` blocks of `--calls` (kernel) / `--torch-calls` (torch) calls; `spread` = (max - min) /
median.  `pair_dims_per_s` = N N (Lg + Ll) over lse_ms.  `valu_peak_fraction` = 3 vector operations per pair-dimension (subtract,
multiply, fused multiply-add) over the fp32 vector peak counted in operations: 157.3 TFLOP/s is 78.65e12 fused multiply-adds per
second, so the fraction is 3 pair_dims_per_s / 78.65e12 -- a whole-call rate of sv_latent_info_lse, staging and the streaming
log-sum-exp included.  `max_abs_diff` = the largest |lse_kernel - lse_torch| over the three sums and all samples.

Per-kernel device times: run under `rocprofv3 --kernel-trace --stats` separately (`--kernel-only`: the kernel calls alone).

    python scripts/bench_latent_info.py [--rounds 5] [--calls 3] [--out profiles/latent_info_bench.json] [--kernel-only]
"""
import argparse
import json
import math
import os
import statistics
import sys

N, PEAK_FMA_PER_S = 26032, 157.3e12 / 2


def timed(fn, n=1):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def med(v):
    m = statistics.median(v)
    return dict(ms=round(m, 4), spread=round((max(v) - min(v)) / m, 4))


def posteriors(L, n=N):
    import torch
    gen = torch.Generator(device="cuda").manual_seed(L)
    mu = torch.randn((n, 2 * L), generator=gen, device="cuda")
    sig = torch.exp(torch.rand((n, 2 * L), generator=gen, device="cuda") * math.log(1e-2))
    return mu, sig


def torch_lse(z, mu, rsig, cst, Lg, qc, rc):
    """lse [3, Nq] fp64 by the direct form, chunk by chunk; fp32 scores, a streamed fp64 logaddexp over the reference chunks"""
    import torch
    Nq, Nr = z.shape[0], mu.shape[0]
    out = torch.empty((3, Nq), dtype=torch.float64, device=z.device)
    for q0 in range(0, Nq, qc):
        zq = z[q0:q0 + qc, None, :]
        run = None
        for r0 in range(0, Nr, rc):
            u = (zq - mu[None, r0:r0 + rc]) * rsig[None, r0:r0 + rc]
            u = u * u
            eg = cst[None, r0:r0 + rc, 0] - 0.5 * u[..., :Lg].sum(-1)
            el = cst[None, r0:r0 + rc, 1] - 0.5 * u[..., Lg:].sum(-1)
            part = torch.stack([torch.logsumexp(e.double(), dim=1) for e in (eg, el, eg + el)])
            run = part if run is None else torch.logaddexp(run, part)
        out[:, q0:q0 + qc] = run - math.log(Nr)
    return out


def shape_row(L, a):
    import torch
    from split_vae_amd import latent_info, ops
    mu, sig = posteriors(L)
    z, rsig, cst, own, prior = ops.latent_info_draw(mu, sig, L, seed=1)
    ws = torch.empty((ops.latent_info_workspace_bytes(N, N),), dtype=torch.uint8, device="cuda")
    lse = torch.empty((3, N), dtype=torch.float64, device="cuda")
    whole = lambda: latent_info.information(mu, sig, L, seed=1)                    # noqa: E731
    alone = lambda: ops.latent_info_lse(z, mu, rsig, cst, L, lse=lse, workspace=ws)  # noqa: E731
    theirs = lambda: torch_lse(z, mu, rsig, cst, L, a.torch_q, a.torch_r)            # noqa: E731
    timed(whole, 2), timed(alone, 2)
    if a.kernel_only:
        timed(whole, a.calls)
        return dict(N=N, Lg=L, Ll=L, kernel_only=True)
    timed(theirs, 1)
    tw, tl, tt = [], [], []
    for _ in range(a.rounds):
        tw.append(timed(whole, a.calls))
        tl.append(timed(alone, a.calls))
        tt.append(timed(theirs, a.torch_calls))
    row = dict(N=N, Lg=L, Ll=L, kernel=med(tw), lse_alone=med(tl), torch_direct_form=med(tt), workspace_mb=round(ws.numel() / 2 ** 20, 1),
               torch_chunks=[a.torch_q, a.torch_r])
    row["torch_over_kernel"] = round(row["torch_direct_form"]["ms"] / row["kernel"]["ms"], 2)
    pd = float(N) * N * 2 * L
    row["pair_dims"] = pd
    row["pair_dims_per_s"] = round(pd / (row["lse_alone"]["ms"] * 1e-3), 0)
    row["valu_peak_fraction"] = round(3.0 * row["pair_dims_per_s"] / PEAK_FMA_PER_S, 4)
    row["max_abs_diff"] = float((alone() - theirs()).abs().max())
    row["report"] = [round(v, 6) for v in whole().cpu().tolist()]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--torch-calls", type=int, default=1)
    ap.add_argument("--torch-q", type=int, default=256)
    ap.add_argument("--torch-r", type=int, default=1024)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import split_vae_amd
    split_vae_amd.configure_hw_queues()
    if not torch.cuda.is_available():
        raise SystemExit("bench_latent_info.py needs the GPU: no timing without one")
    rows = []
    for L in (128, 256):
        rows.append(shape_row(L, a))
        print(json.dumps(rows[-1]), flush=True)
    out = dict(device=torch.cuda.get_device_name(0), timing="hipEvent pairs; median over rounds of blocks of calls",
               fp32_vector_peak_tflops=157.3, rows=rows)
    if a.out and not a.kernel_only:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
