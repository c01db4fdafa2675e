"""Cost of the importance-weighted log-likelihood (split_vae_amd/iw.py) beside trainer.test_step, on the same batch, in ONE process.

Rows: SVHN-32 B = 64 and CelebA-64 B = 512, fp32 and bf16.  Per row, after warm-up, between hipEvent pairs:

  test_step_ms   one trainer.test_step (encoders + decoders + loss + the read-back of its five means), mean of `--steps` calls
  iw_total_ms    one iw.log_likelihood call at K = `--k-lo` and at K = `--k-hi` (encoders once, K sample passes, finish)
  iw_sample_ms   the marginal time per (batch, sample) of the K loop: (t(k-hi) - t(k-lo)) / (k-hi - k-lo), k-hi - k-lo >= 50:
                 one decoder + loss pass and one sv_iw_advance launch

Each figure is the median of `--rounds` rounds (test_step and the two K alternate inside a round); `spread` = (max - min) / median.

    python scripts/bench_iw.py [--steps 50] [--rounds 5] [--out profiles/iw_bench.json]

`--test-step-only --tree DIR` times test_step alone with split_vae_amd imported from another checkout (the parent commit, built,
in the same visit); `--parent-json FILE` embeds that run's rows so one file holds both.
"""
import argparse
import json
import os
import statistics
import sys

ROWS = (("svhn", 32, 64, 1, 40.0, "f32"), ("svhn", 32, 64, 1, 40.0, "bf16"), ("celeba64", 64, 512, 8, 120.0, "f32"),
        ("celeba64", 64, 512, 8, 120.0, "bf16"))


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
    return dict(ms=round(m, 5), spread=round((max(v) - min(v)) / m, 4))


def run_row(name, H, B, patch, beta, dtype, a):
    import torch
    from split_vae_amd import data, trainer
    from split_vae_amd.augmentation import Augmentator
    from split_vae_amd.model import LGVae
    model = LGVae(128, 128, image_shape=[-1, H, H, 3], dtype=dtype, device="cuda", seed=3)
    model.beta = beta
    images = Augmentator("scramble", size=patch, seed=1).augment(data.synthetic_images(B, H, H, seed=0, device="cuda"))
    row = dict(dataset=name, H=H, B=B, dtype=dtype, steps=a.steps, rounds=a.rounds)
    step = lambda: trainer.test_step(model, images)     # noqa: E731
    if a.test_step_only:
        timed(step, 5)
        row["test_step"] = med([timed(step, a.steps) for _ in range(a.rounds)])
        return row
    from split_vae_amd import iw
    lo = lambda: iw.log_likelihood(model, images, a.k_lo)    # noqa: E731
    hi = lambda: iw.log_likelihood(model, images, a.k_hi)    # noqa: E731
    timed(step, 5), timed(lo, 2), timed(hi, 1)
    ts, tl, th = [], [], []
    for _ in range(a.rounds):
        ts.append(timed(step, a.steps))
        tl.append(timed(lo))
        th.append(timed(hi))
    row["test_step"] = med(ts)
    row["iw_total_k%d" % a.k_lo], row["iw_total_k%d" % a.k_hi] = med(tl), med(th)
    row["iw_sample"] = med([(h - l) / (a.k_hi - a.k_lo) for h, l in zip(th, tl)])
    row["iw_sample_over_test_step"] = round(row["iw_sample"]["ms"] / row["test_step"]["ms"], 4)
    Lj, Lx, el = iw.log_likelihood(model, images, a.k_lo)
    row["check"] = dict(iw_joint=float(Lj.double().mean()), iw_x=float(Lx.double().mean()), elbo=float(el.double().mean()))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--k-lo", type=int, default=8)
    ap.add_argument("--k-hi", type=int, default=72)
    ap.add_argument("--test-step-only", action="store_true")
    ap.add_argument("--tree", type=str, default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--parent-json", type=str, default=None)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if a.k_hi - a.k_lo < 50:
        raise SystemExit("--k-hi - --k-lo must be at least 50 samples")
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch
    import split_vae_amd
    split_vae_amd.configure_hw_queues()
    if not torch.cuda.is_available():
        raise SystemExit("bench_iw.py needs the GPU: no timing without one")
    rows = []
    for r in ROWS:
        rows.append(run_row(*r, a))
        print(json.dumps(rows[-1]), flush=True)
    out = dict(tree=os.path.basename(os.path.abspath(a.tree)) if a.test_step_only else "this commit",
               device=torch.cuda.get_device_name(0), timing="hipEvent pairs, median over rounds", rows=rows)
    if a.parent_json:
        with open(a.parent_json) as f:
            out["parent_commit_test_step"] = json.load(f)["rows"]
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
