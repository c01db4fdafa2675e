"""Cost of the exact t-SNE map (split_vae_amd/tsne.py, csrc/tsne.hip) at SVHN scale, in ONE process.

Per N in {10 000, 26 032}, L = 128: synthetic Gaussian clusters (10 centres ~ 3 N(0, I), points = centre + N(0, I)), perplexity 30.
Between hipEvent pairs, after warm-up, alternating inside a round:

  ours       ops.tsne_iterate, T iterations and 0, from a developed state (50 iterations in), box to box (workspace and state
             allocated outside); ops.tsne_affinities
  torch      the same definition as a user would compose it from dense ops: q = 1 + cdist(Y, Y)^2, w = 1 / q with a zero diagonal,
             Z = w.sum(), the forces as matrix products of (e P w - w^2 / Z) with Y, the gain rule, the update, the recentring --
             T iterations and 0

`iter_us` = (time(T) - time(0)) / T, the median over `--rounds` of blocks of `--calls` calls; `spread` = (max - min) / median of the
T-iteration calls.  `floor_us` = 4 N^2 B / 6.29 TB/s, the one pass over P every iteration needs (the achievable HBM rate of the
micro-architecture notes); `over_floor` = iter_us / floor_us.  `valu_us`: the pair pass issues about 26 vector instructions per pair
(two of them quarter-rate: v_rcp_f32, v_log_f32, counted four times) on 256 CUs x 4 SIMDs x 16 lanes at 2.4 GHz; the larger of
floor_us and valu_us names the bound.  `report_s`: tsne.evaluate of a seeded LGVae on N synthetic 32 x 32 images with made-up labels,
T = `--report_iters`, wall clock with one synchronisation.  Anything that did not run is "not measured".

    python scripts/bench_tsne.py [--rounds 3] [--calls 2] [--iters 10] [--report_n 10000] [--out profiles/tsne_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

HBM_TBS = 6.29
VALU_PER_PAIR = 26 + 2 * 3          # instructions per pair, the two transcendental ones at a quarter of the rate
LANE_RATE = 256 * 4 * 16 * 2.4e9    # lane-instructions per second


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


def torch_iterate(P, Y, inc, gain, T, t0, e0, exag_iters, eta):
    import torch
    N = Y.shape[0]
    for t in range(t0, t0 + T):
        e, mom = (e0, 0.5) if t < exag_iters else (1.0, 0.8)
        w = 1.0 / (1.0 + torch.cdist(Y, Y) ** 2)
        w.fill_diagonal_(0.0)
        Z = w.sum()
        m = (e * P - w / Z) * w
        g = 4.0 * (m.sum(dim=1, keepdim=True) * Y - m @ Y)
        gain = torch.where((g > 0) != (inc > 0), gain + 0.2, gain * 0.8).clamp_min(0.01)
        inc = mom * inc - eta * gain * g
        Y = Y + inc
        Y = Y - Y.mean(dim=0, keepdim=True)
    return Y, inc, gain


def row(N, L, a):
    import torch
    from split_vae_amd import ops
    gen = torch.Generator(device="cuda").manual_seed(N + L)
    centres = 3.0 * torch.randn((10, L), generator=gen, device="cuda")
    x = centres[torch.randint(0, 10, (N,), generator=gen, device="cuda")] + torch.randn((N, L), generator=gen, device="cuda")
    T, eta = a.iters, max(N / 48.0, 50.0)
    ws = torch.empty((ops.tsne_workspace_bytes(N),), dtype=torch.uint8, device="cuda")
    P = torch.empty((N, N), dtype=torch.float32, device="cuda")
    aff = ops.tsne_affinities(x, 30.0, P=P, workspace=ws)
    st = ops.tsne_init(ops.tsne_state(N, 50 + 1000 * T), 0)
    ops.tsne_iterate(aff, st, 50, 12.0, 250, eta, workspace=ws)              # a developed state: both paths start from it
    Y0, i0, g0 = st["Y"].clone(), st["inc"].clone(), st["gain"].clone()

    def ours(t):
        st["Y"].copy_(Y0); st["inc"].copy_(i0); st["gain"].copy_(g0); st["state"][0] = 50
        ops.tsne_iterate(aff, st, t, 12.0, 250, eta, workspace=ws)
    calls = {"ours_T": lambda: ours(T), "ours_0": lambda: ours(0), "torch_T": lambda: torch_iterate(P, Y0, i0, g0, T, 50, 12.0, 250, eta),
             "torch_0": lambda: torch_iterate(P, Y0, i0, g0, 0, 50, 12.0, 250, eta),
             "affinities": lambda: ops.tsne_affinities(x, 30.0, P=P, workspace=ws)}
    for fn in calls.values():
        timed(fn, 1)
    times = {k: [] for k in calls}
    for _ in range(a.rounds):
        for k, fn in calls.items():                                                # alternating inside a round
            times[k].append(timed(fn, a.calls if k != "affinities" else 1))
    m = {k: statistics.median(v) for k, v in times.items()}
    ours(T)
    Yt = torch_iterate(P, Y0, i0, g0, T, 50, 12.0, 250, eta)[0]
    iter_us = (m["ours_T"] - m["ours_0"]) / T * 1e3
    torch_us = (m["torch_T"] - m["torch_0"]) / T * 1e3
    floor_us = 4.0 * N * N / (HBM_TBS * 1e12) * 1e6
    valu_us = VALU_PER_PAIR * float(N) * N / LANE_RATE * 1e6
    return dict(N=N, L=L, iters=T, iter_us=round(iter_us, 1), torch_iter_us=round(torch_us, 1), torch_over_ours=round(torch_us / iter_us, 2),
                floor_us=round(floor_us, 1), over_floor=round(iter_us / floor_us, 3), valu_us=round(valu_us, 1),
                bound="HBM" if floor_us >= valu_us else "vector issue",
                spread=round((max(times["ours_T"]) - min(times["ours_T"])) / m["ours_T"], 4),
                torch_spread=round((max(times["torch_T"]) - min(times["torch_T"])) / m["torch_T"], 4),
                affinities_ms=round(m["affinities"], 2), workspace_mb=round(ws.numel() / 2 ** 20, 1), P_mb=round(4.0 * N * N / 2 ** 20, 1),
                max_dY=float((st["Y"] - Yt).abs().max()), Y_extent=float(Y0.abs().max()))


def report(a):
    import numpy as np
    import torch
    from split_vae_amd import tsne
    from split_vae_amd.model import LGVae
    N, B = a.report_n, 500
    model = LGVae(128, 128, image_shape=(None, 32, 32, 3), dtype="f32", seed=3)
    gen = torch.Generator(device="cuda").manual_seed(1)
    onehot = np.eye(10, dtype=np.float32)
    batches = []
    for o in range(0, N, B):
        cls = torch.randint(0, 10, (min(B, N - o),), generator=gen, device="cuda")
        batches.append((torch.rand((cls.numel(), 32, 32, 6), generator=gen, device="cuda") * 2 - 1, torch.from_numpy(onehot).cuda()[cls]))
    tsne.evaluate(model, batches[:2], 1000, iters=5)                                # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = tsne.evaluate(model, batches, N, iters=a.report_iters)
    torch.cuda.synchronize()
    return dict(model="LGVae 32 x 32, seeded weights, synthetic images", n_images=res["n_images"], iters=a.report_iters, blocks=2,
                report_s=round(time.perf_counter() - t0, 3), line=tsne.report_line(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--sizes", type=str, default="10000,26032")
    ap.add_argument("--report_n", type=int, default=10000)
    ap.add_argument("--report_iters", type=int, default=1000)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import split_vae_amd
    split_vae_amd.configure_hw_queues()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tsne.py needs the GPU: no timing without one")
    rows = []
    for N in [int(v) for v in a.sizes.split(",") if v]:
        rows.append(row(N, 128, a))
        print(json.dumps(rows[-1]), flush=True)
        torch.cuda.empty_cache()
    rep = report(a) if a.report_n > 0 else "not measured"
    print(json.dumps(rep), flush=True)
    out = dict(device=torch.cuda.get_device_name(0), timing="hipEvent pairs; median over rounds of blocks of calls; ours and torch alternate inside a round",
               hbm_achievable_tbs=HBM_TBS, rows=rows, report=rep)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
