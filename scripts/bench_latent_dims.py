"""Cost of the per-dimension latent report (split_vae_amd/latent_dims.py, csrc/latent_dims.hip), in ONE process: sv_latent_dims_lse
alone at N = 4096, 10 000 and 26 032 images with latent widths 128 + 128 and 256 + 256 (one call per block), against

  torch_ms   the only other implementation that exists: the same definition as a chunked torch composition on the device (query
             chunks x reference chunks of `--torch-q` x `--torch-r` rows: [q, r, L] fp32 scores, logsumexp over r, a streamed fp64
             logaddexp over the reference chunks).  It materialises the scores and is bound by memory traffic: a factor to report,
             not a target.
  exp rate   the exponentials per second of the call (9 per 8 scores: one rescale per group of 8) as a fraction of what the card
             sustains on v_exp_f32 alone: `--exp-probe PATH` runs the built scripts/micro/exp_f32_rate.hip in a child process and
             takes its EXP_PER_S line (`--exp-per-s` gives the figure directly).

and the whole --latent_dims N pass (latent_dims.evaluate: encoders, the --latent_info calls it builds on, the three calls per block,
one read-back) against the --latent_info N pass (latent_info.evaluate) of the same SVHN-32 LGVae at the same N: what the flag adds to
an evaluation.

Synthetic posteriors in the shape a trained split VAE leaves: sig log-uniform in [1e-2, 1], means ~ N(0, I).  Every figure is the
median of `--rounds` hipEvent-timed blocks of `--calls` calls after a warm-up, the three sides alternating inside a round; `spread`
= (max - min) / median.  Per-kernel device times: run under `rocprofv3 --kernel-trace --stats` separately (`--kernel-only`).

    python scripts/bench_latent_dims.py [--rounds 5] [--calls 3] [--exp-probe build/exp_f32_rate] [--out profiles/latent_dims_bench.json]
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time

SIZES, WIDTHS, GROUP = (4096, 10000, 26032), (128, 256), 8


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


def posteriors(n, L):
    import torch
    gen = torch.Generator(device="cuda").manual_seed(L)
    mu = torch.randn((n, 2 * L), generator=gen, device="cuda")
    sig = torch.exp(torch.rand((n, 2 * L), generator=gen, device="cuda") * math.log(1e-2))
    return mu, sig


def torch_lse(z, mu, rsig, lc, qc, rc):
    """lse [Nq, L] fp64 of one block by the definition, chunk by chunk"""
    import torch
    Nq, Nr = z.shape[0], mu.shape[0]
    out = torch.empty(z.shape, dtype=torch.float64, device=z.device)
    for q0 in range(0, Nq, qc):
        zq = z[q0:q0 + qc, None, :]
        run = None
        for r0 in range(0, Nr, rc):
            u = (zq - mu[None, r0:r0 + rc]) * rsig[None, r0:r0 + rc]
            part = torch.logsumexp(lc[None, r0:r0 + rc] - 0.5 * u * u, dim=1).double()
            run = part if run is None else torch.logaddexp(run, part)
        out[q0:q0 + qc] = run - math.log(Nr)
    return out


def shape_row(n, L, a, exp_rate):
    import torch
    from split_vae_amd import ops
    mu, sig = posteriors(n, L)
    z, rsig = ops.latent_info_draw(mu, sig, L, seed=1)[:2]
    blocks = []
    for e, (c0, c1) in enumerate(((0, L), (L, 2 * L))):
        v = [t[:, c0:c1] for t in (z, mu, rsig)]
        lc = ops.latent_dims_prepare(mu[:, c0:c1], sig[:, c0:c1], block=e, seed=1)[0]
        blocks.append((v[0], v[1], v[2], lc, torch.empty((n, L), dtype=torch.float64, device="cuda")))
    ws = torch.empty((ops.latent_dims_workspace_bytes(n, n, L),), dtype=torch.uint8, device="cuda")
    ours = lambda: [ops.latent_dims_lse(zz, mm, rr, lc, lse=out, workspace=ws) for zz, mm, rr, lc, out in blocks]   # noqa: E731
    theirs = lambda: [torch_lse(zz, mm, rr, lc, a.torch_q, a.torch_r) for zz, mm, rr, lc, _ in blocks]            # noqa: E731
    timed(ours, 2)
    if not a.kernel_only:
        timed(theirs, 1)
    if a.kernel_only:
        timed(ours, a.calls)
        return dict(N=n, Lg=L, Ll=L, kernel_only=True)
    tk, tt = [], []
    for r in range(a.rounds):
        tk.append(timed(ours, a.calls))
        if r < a.torch_rounds:
            tt.append(timed(theirs, 1))
    row = dict(N=n, Lg=L, Ll=L, lse=med(tk), torch_composition=med(tt), workspace_mb=round(ws.numel() / 2 ** 20, 1),
               torch_chunks=[a.torch_q, a.torch_r])
    row["torch_over_kernel"] = round(row["torch_composition"]["ms"] / row["lse"]["ms"], 1)
    scores = float(n) * n * 2 * L
    row["scores_per_s"] = round(scores / (row["lse"]["ms"] * 1e-3), 0)
    row["exp_per_s"] = round(row["scores_per_s"] * (GROUP + 1) / GROUP, 0)
    if exp_rate:
        row["exp_rate_fraction"] = round(row["exp_per_s"] / exp_rate, 4)
    row["max_abs_diff"] = max(float((x - y).abs().max()) for x, y in zip(ours(), theirs()))
    return row


def pass_row(n, a):
    """latent_info.evaluate against latent_dims.evaluate on one SVHN-32 LGVae (128 + 128), the same N and batches: wall clock around
    the whole call, read-back included"""
    import torch
    from split_vae_amd import latent_dims, latent_info
    from split_vae_amd.model import LGVae
    model = LGVae(128, 128, image_shape=(None, 32, 32, 3), dtype="f32", seed=3)
    x = torch.rand((128, 32, 32, 6), device="cuda") * 2 - 1
    batches = [x + 0.01 * i for i in range(8)] * ((n + 1023) // 1024)

    def wall(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn(model, batches, n)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3
    wall(latent_info.evaluate), wall(latent_dims.evaluate)
    ti, td = [], []
    for _ in range(a.rounds):
        ti.append(wall(latent_info.evaluate))
        td.append(wall(latent_dims.evaluate))
    row = dict(N=n, model="lgvae 128+128, SVHN-32, batches of 128", latent_info_pass=med(ti), latent_dims_pass=med(td))
    row["dims_over_info"] = round(row["latent_dims_pass"]["ms"] / row["latent_info_pass"]["ms"], 2)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--torch-rounds", type=int, default=2)
    ap.add_argument("--torch-q", type=int, default=256)
    ap.add_argument("--torch-r", type=int, default=1024)
    ap.add_argument("--exp-probe", type=str, default=None)
    ap.add_argument("--exp-per-s", type=float, default=0.0)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    exp_rate, probe = a.exp_per_s, None
    if a.exp_probe:                                   # a child process of its own, before this one opens the device
        probe = subprocess.run([a.exp_probe], capture_output=True, text=True, timeout=120, check=True).stdout
        exp_rate = float([l for l in probe.splitlines() if l.startswith("EXP_PER_S")][-1].split()[1])
    import torch
    import split_vae_amd
    split_vae_amd.configure_hw_queues()
    if not torch.cuda.is_available():
        raise SystemExit("bench_latent_dims.py needs the GPU: no timing without one")
    rows, passes = [], []
    for n in SIZES:
        for L in WIDTHS:
            rows.append(shape_row(n, L, a, exp_rate))
            print(json.dumps(rows[-1]), flush=True)
    if not a.kernel_only:
        for n in SIZES:
            passes.append(pass_row(n, a))
            print(json.dumps(passes[-1]), flush=True)
    out = dict(device=torch.cuda.get_device_name(0), timing="hipEvent pairs; median over rounds of blocks of calls (passes: wall clock)",
               exp_probe_per_s=exp_rate, exp_probe_output=probe.splitlines() if probe else None, rows=rows, passes=passes)
    if a.out and not a.kernel_only:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
