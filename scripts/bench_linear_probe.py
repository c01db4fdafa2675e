"""Cost of the linear label probe (split_vae_amd/linear_probe.py, csrc/linprobe.hip) at SVHN scale, in ONE process.

Per (N, L) in {20 000, 73 257} x {128, 256}, C = 10: synthetic Gaussian clusters (10 centres ~ N(0, I), points = centre +
N(0, I)), l2 = 1e-3, P = B^-1 from the device's own Gram matrix.  Between hipEvent pairs, after warm-up, alternating inside a round:

  ours       ops.linprobe_fit from W = 0, box to box (workspace and outputs allocated outside), once with T steps and once with 0;
             ops.linprobe_gram; ops.linprobe_predict with classes and loss
  torch      the same definition as a user would compose it: z = x @ w32 + b, softmax, r = p - onehot, G = [x 1]^T r / N + l2 W in
             fp32, the step W -= P @ G in float64 -- T steps and 0; A^T A in fp32; argmax of the logits

`iter_us` = (time(T) - time(0)) / T, the median over `--rounds` of blocks of `--calls` calls; `spread` = (max - min) / median of the
T-step calls.  `bound_us` = passes N L 4 B / 6.29 TB/s with passes = 2: the kernels read x once for the logits and once for A^T R
(the residuals, N x 16 fp32, go through memory beside them and are counted: 2 N 16 4 B); `share` = bound_us / iter_us.  A fit
iteration is four launches; where iter_us is near 4 launch latencies the shape is launch-bound and `share` says so.
`max_dW` = the largest difference of the two paths' W after T steps.

    python scripts/bench_linear_probe.py [--rounds 5] [--calls 3] [--iters 10] [--out profiles/linear_probe_bench.json]
"""
import argparse
import itertools
import json
import os
import statistics
import sys

HBM_TBS = 6.29
PASSES = 2


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


def torch_fit(x, onehot, P, l2, T):
    import torch
    N, L = x.shape
    W = torch.zeros((L + 1, onehot.shape[1]), dtype=torch.float64, device=x.device)
    for t in range(T + 1):
        w32 = W.float()
        z = x @ w32[:L] + w32[L]
        r = torch.softmax(z, dim=1) - onehot
        G = torch.cat([x.t() @ r, r.sum(dim=0, keepdim=True)]).double() / N
        G[:L] += l2 * W[:L]
        if t == T:
            break
        W = W - P @ G
    return W


def row(N, L, C, a):
    import torch
    from split_vae_amd import linear_probe, ops
    gen = torch.Generator(device="cuda").manual_seed(N + L)
    centres = torch.randn((C, L), generator=gen, device="cuda")
    y64 = torch.randint(0, C, (N,), generator=gen, device="cuda")
    x = centres[y64] + torch.randn((N, L), generator=gen, device="cuda")
    y = y64.to(torch.uint8)
    onehot = torch.nn.functional.one_hot(y64, C).float()
    l2, T = 1e-3, a.iters
    ws = torch.empty((ops.linprobe_workspace_bytes(N, L, C),), dtype=torch.uint8, device="cuda")
    S = ops.linprobe_gram(x, workspace=ws)
    P = torch.from_numpy(linear_probe.step_matrix(S.cpu().numpy(), N, l2)).cuda()
    fit = ops.linprobe_state(x, C, T)
    acc = torch.zeros((2,), dtype=torch.int64, device="cuda")

    def ours(t):
        fit["W"].zero_()
        ops.linprobe_fit(x, y, P, fit, t, l2, workspace=ws)
    a1 = torch.cat([x, torch.ones((N, 1), device="cuda")], dim=1)
    calls = {"ours_T": lambda: ours(T), "ours_0": lambda: ours(0), "torch_T": lambda: torch_fit(x, onehot, P, l2, T),
             "torch_0": lambda: torch_fit(x, onehot, P, l2, 0), "gram": lambda: ops.linprobe_gram(x, workspace=ws), "torch_gram": lambda: a1.t() @ a1,
             "predict": lambda: ops.linprobe_predict(x, fit["W"], q_class=y, acc=acc, want_loss=True, workspace=ws),
             "torch_predict": lambda: (x @ fit["W"][:L].float() + fit["W"][L].float()).argmax(dim=1)}
    for fn in calls.values():
        timed(fn, 2)
    times = {k: [] for k in calls}
    for _ in range(a.rounds):
        for k, fn in calls.items():                                                # alternating inside a round
            times[k].append(timed(fn, a.calls))
    m = {k: statistics.median(v) for k, v in times.items()}
    ours(T)
    Wt = torch_fit(x, onehot, P, l2, T)
    iter_us = (m["ours_T"] - m["ours_0"]) / T * 1e3
    torch_us = (m["torch_T"] - m["torch_0"]) / T * 1e3
    bound_us = (PASSES * N * L * 4 + 2 * N * 16 * 4) / (HBM_TBS * 1e12) * 1e6
    return dict(N=N, L=L, C=C, iters=T, iter_us=round(iter_us, 2), torch_iter_us=round(torch_us, 2), torch_over_ours=round(torch_us / iter_us, 3),
                pass_us=round(m["ours_0"] * 1e3, 2), torch_pass_us=round(m["torch_0"] * 1e3, 2),
                spread=round((max(times["ours_T"]) - min(times["ours_T"])) / m["ours_T"], 4),
                torch_spread=round((max(times["torch_T"]) - min(times["torch_T"])) / m["torch_T"], 4),
                passes_over_x=PASSES, bound_us=round(bound_us, 2), share=round(bound_us / iter_us, 4),
                gram_us=round(m["gram"] * 1e3, 2), torch_gram_us=round(m["torch_gram"] * 1e3, 2),
                predict_us=round(m["predict"] * 1e3, 2), torch_predict_us=round(m["torch_predict"] * 1e3, 2),
                workspace_mb=round(ws.numel() / 2 ** 20, 1), max_dW=float((fit["W"] - Wt).abs().max()),
                loss_first_last=[float(fit["loss"][0]), float(fit["loss"][T])])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import split_vae_amd
    split_vae_amd.configure_hw_queues()
    if not torch.cuda.is_available():
        raise SystemExit("bench_linear_probe.py needs the GPU: no timing without one")
    rows = []
    for N, L in itertools.product((20000, 73257), (128, 256)):
        rows.append(row(N, L, 10, a))
        print(json.dumps(rows[-1]), flush=True)
    out = dict(device=torch.cuda.get_device_name(0), timing="hipEvent pairs; median over rounds of blocks of calls; ours and torch alternate inside a round",
               hbm_achievable_tbs=HBM_TBS, rows=rows)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
