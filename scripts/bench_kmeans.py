"""Cost of the k-means cluster report (split_vae_amd/cluster.py, csrc/kmeans.hip) at SVHN scale, in ONE process.

Part 1, per (N, L, K, R) in {26 032, 73 257} x {128, 256} x {10, 30} x {1, 8}: synthetic clustered latents (K centres ~ N(0, I),
points = centre + N(0, I)), the k-means++ seeds of sv_kmeans_seed as the start of both paths.  Between hipEvent pairs, after
warm-up, alternating inside a round:

  ours       ops.kmeans_iterate from the seeds, box to box (norms, assign, then per iteration segmented sum + update + assign;
             workspace and outputs allocated outside), once with T iterations and once with 0
  torch      the same definition as a user would compose it, per restart: d = (n(x) + n(c)) - 2 x c^T, argmin, index_add_ and
             bincount, the division, an empty cluster keeping its centroid -- T iterations and 0

`iter_us` = (time(T) - time(0)) / T, the median over `--rounds` of blocks of `--calls` calls; `spread` = (max - min) / median of the
T-iteration calls.  `bound_us` = max(N L 4 B / 6.29 TB/s, 2 N R K L / 157.3 TFLOP/s), the least time one iteration can take (x read
once at the achievable HBM rate; the distance GEMM at the fp32 matrix peak), `bound` says which, `share` = bound_us / iter_us.
`seed_ms` = one sv_kmeans_seed call.  `same_assign` = the fraction of (restart, row) pairs the two paths assign alike after T
iterations (they differ at near-ties: the composition's distances are in another order).

Part 2: the whole report of an LGVae (SVHN-32, latents 128 / 128) over 26 032 test images, K = 10, 8 restarts, at most 100
iterations: the encoding pass (latent_info.posteriors), the two fits and the tables, each timed separately.

    python scripts/bench_kmeans.py [--rounds 5] [--calls 3] [--iters 10] [--out profiles/kmeans_bench.json]
"""
import argparse
import itertools
import json
import os
import statistics
import sys

HBM_TBS, PEAK_TF = 6.29, 157.3


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


def torch_fit(x, c0, T):
    """R restarts, one after the other -> (assign [R,N], centroids [R,K,L])"""
    import torch
    K = c0.shape[1]
    xn = (x * x).sum(dim=1)
    outs_a, outs_c = [], []
    for r in range(c0.shape[0]):
        c = c0[r].clone()
        for t in range(T + 1):
            d = (xn[:, None] + (c * c).sum(dim=1)[None, :]) - 2.0 * (x @ c.t())
            a = d.argmin(dim=1)
            if t == T:
                break
            s = torch.zeros_like(c).index_add_(0, a, x)
            n = torch.bincount(a, minlength=K)
            c = torch.where(n[:, None] > 0, s / n.clamp(min=1)[:, None], c)
        outs_a.append(a)
        outs_c.append(c)
    return torch.stack(outs_a), torch.stack(outs_c)


def kernel_row(N, L, K, R, a):
    import torch
    from split_vae_amd import ops
    gen = torch.Generator(device="cuda").manual_seed(N + L + K + R)
    centres = torch.randn((K, L), generator=gen, device="cuda")
    x = centres[torch.randint(0, K, (N,), generator=gen, device="cuda")] + torch.randn((N, L), generator=gen, device="cuda")
    ws = torch.empty((ops.kmeans_workspace_bytes(N, L, K, R),), dtype=torch.uint8, device="cuda")
    seeds = ops.kmeans_seed(x, K, R, seed=1, workspace=ws)
    fit = ops.kmeans_state(x, seeds.clone())
    T = a.iters

    def ours(t):
        fit["centroids"].copy_(seeds)
        ops.kmeans_iterate(x, fit, t, workspace=ws)
    calls = {"ours_T": lambda: ours(T), "ours_0": lambda: ours(0), "torch_T": lambda: torch_fit(x, seeds, T), "torch_0": lambda: torch_fit(x, seeds, 0)}
    for fn in calls.values():
        timed(fn, 2)
    times = {k: [] for k in calls}
    for _ in range(a.rounds):
        for k, fn in calls.items():                                                # alternating inside a round
            times[k].append(timed(fn, a.calls))
    m = {k: statistics.median(v) for k, v in times.items()}
    ours(T)
    ta, _ = torch_fit(x, seeds, T)
    iter_us = (m["ours_T"] - m["ours_0"]) / T * 1e3
    torch_us = (m["torch_T"] - m["torch_0"]) / T * 1e3
    hbm_us, mfma_us = N * L * 4 / (HBM_TBS * 1e12) * 1e6, 2.0 * N * R * K * L / (PEAK_TF * 1e12) * 1e6
    return dict(N=N, L=L, K=K, R=R, iters=T, iter_us=round(iter_us, 2), torch_iter_us=round(torch_us, 2), torch_over_ours=round(torch_us / iter_us, 3),
                assign_pass_us=round(m["ours_0"] * 1e3, 2), torch_assign_pass_us=round(m["torch_0"] * 1e3, 2),
                spread=round((max(times["ours_T"]) - min(times["ours_T"])) / m["ours_T"], 4),
                torch_spread=round((max(times["torch_T"]) - min(times["torch_T"])) / m["torch_T"], 4),
                bound_us=round(max(hbm_us, mfma_us), 2), bound="hbm" if hbm_us >= mfma_us else "mfma", share=round(max(hbm_us, mfma_us) / iter_us, 4),
                seed_ms=round(timed(lambda: ops.kmeans_seed(x, K, R, seed=1, workspace=ws), 2), 3), workspace_mb=round(ws.numel() / 2 ** 20, 1),
                same_assign=round(float((fit["assign"].long() == ta).double().mean()), 5))


def report_row(a):
    import torch
    from split_vae_amd import cluster, data, ops
    from split_vae_amd.augmentation import Augmentator
    from split_vae_amd.latent_info import posteriors
    from split_vae_amd.model import LGVae
    B, H, N, K, R, T = a.batch, 32, 26032, 10, 8, 100
    model = LGVae(128, 128, image_shape=[-1, H, H, 3], dtype="f32", device="cuda", seed=3)
    aug = Augmentator("scramble", size=4, seed=1)
    pool = [aug.augment(data.synthetic_images(B, H, H, seed=s, device="cuda")) for s in range(8)]
    batches = [pool[i % len(pool)][:min(B, N - o)] for i, o in enumerate(range(0, N, B))]
    posteriors(model, batches[:4])                                                 # plans, code objects
    out = {}
    t_enc = timed(lambda: out.__setitem__("p", posteriors(model, batches, N)))
    mu, _, Lg, Ll = out["p"]
    cluster.kmeans(mu[:, :Lg], K, R, 2, seed=0)
    t_g = timed(lambda: out.__setitem__("g", cluster.kmeans(mu[:, :Lg], K, R, T, seed=0)))
    t_l = timed(lambda: out.__setitem__("l", cluster.kmeans(mu[:, Lg:], K, R, T, seed=0)))
    t_all = timed(lambda: out.__setitem__("res", cluster.evaluate(model, batches, N, K, R, T)))
    return dict(model="lgvae svhn-32 f32, latents 128/128, random weights", batch=B, n_images=N, k=K, restarts=R, max_iters=T, encode_ms=round(t_enc, 2),
                kmeans_z_g_ms=round(t_g, 2), kmeans_z_l_ms=round(t_l, 2), evaluate_ms=round(t_all, 2),
                n_iter_g=out["g"]["n_iter"].tolist(), n_iter_l=out["l"]["n_iter"].tolist(), line=cluster.report_line(out["res"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batch", type=int, default=64, help="encoder batch of the whole report (the CLI's default --batch_size)")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import split_vae_amd
    split_vae_amd.configure_hw_queues()
    if not torch.cuda.is_available():
        raise SystemExit("bench_kmeans.py needs the GPU: no timing without one")
    rows = []
    for N, L, K, R in itertools.product((26032, 73257), (128, 256), (10, 30), (1, 8)):
        rows.append(kernel_row(N, L, K, R, a))
        print(json.dumps(rows[-1]), flush=True)
    e2e = report_row(a)
    print(json.dumps(e2e), flush=True)
    out = dict(device=torch.cuda.get_device_name(0), timing="hipEvent pairs; median over rounds of blocks of calls; ours and torch alternate inside a round",
               hbm_achievable_tbs=HBM_TBS, fp32_matrix_peak_tf=PEAK_TF, rows=rows, report_end_to_end=e2e)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
