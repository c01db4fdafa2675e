"""The LGVae training loop fed three ways, in ONE process: what a real-data run costs beside the pre-staged synthetic loop.

  host      ArrayDataset (host index generator, NumPy gather, pageable .to(device)) -> Augmentator.augment -> train_step:
            the CLI's real-data path without --resident_data
  resident  ResidentDataset -> Augmentator.augment_from (sv_dataset_gather_scramble writes the step's staged inputs) -> train_step:
            the CLI's path with --resident_data
  synthetic one device batch -> Augmentator.augment(plan=) -> train_step: the loop bench.py times, the ceiling

Seeded arrays in the two real formats: SVHN uint8 32 x 32, N = 100 000 (above the 20 000-element shuffle buffer: fill and drain
phases), CelebA fp32 64 x 64, N = 20 000 (equal to the buffer: every epoch is drain only).  The variants alternate: `rounds`
rounds, each one window of `steps` steps per variant, warmed, synchronised on both sides.  A row reports images/s from the median
round and the spread (max - min) / median over the rounds of the same variant; `resident_faster` says whether the slowest
resident round beat the fastest host round.  Prints one JSON line per row and a last line holding them all.

    python scripts/bench_input.py [--steps 40] [--warmup 5] [--rounds 3] [--out profiles/input_pipeline_bench.json]

`--kernel-pair` instead launches, back to back on the same CelebA-64 B = 512 batch, the fused kernel and the existing
scramble_staged_kernel (both staged dtypes), for `rocprofv3 --kernel-trace --stats -- python scripts/bench_input.py --kernel-pair`;
`--summarise TRACE.csv` turns that run's kernel trace into the table of profiles/input_pipeline_kernel_stats.txt (bytes from the
shapes over the median duration, as a share of 8 TB/s).
"""
import argparse
import csv
import gc
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS = (("svhn", 32, 64, "f32"), ("celeba64", 64, 512, "f32"), ("celeba64", 64, 512, "bf16"), ("celeba64", 64, 64, "f32"))
SETS = {"svhn": dict(N=100000, H=32, kind="uint8", patch=1, beta=40.0), "celeba64": dict(N=20000, H=64, kind="float32", patch=8, beta=120.0)}
HBM_PEAK, COPY_MEASURED = 8.0e12, 6.29e12          # bytes/s: the data-sheet peak and the measured device copy


def make_set(name):
    import numpy as np
    s = SETS[name]
    u8 = np.random.default_rng(11).integers(0, 256, (s["N"], s["H"], s["H"], 3), dtype=np.uint8)
    if s["kind"] == "uint8":
        return u8
    out = np.empty(u8.shape, np.float32)
    for i in range(0, s["N"], 2000):                # (normalise_u8 works in float64: in pieces)
        out[i:i + 2000] = (u8[i:i + 2000] / 255.0 * 2 - 1).astype(np.float32)
    return out


def window(step, steps):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def run_row(name, raw, host_x, B, dtype, steps, warmup, rounds):
    import torch
    from split_vae_amd import data, trainer
    from split_vae_amd.augmentation import Augmentator
    from split_vae_amd.model import LGVae
    from split_vae_amd.optimizer import Adam
    s = SETS[name]
    H = s["H"]
    m = LGVae(128, 128, image_shape=[-1, H, H, 3], dtype=dtype, device="cuda", seed=3)
    m.beta = s["beta"]
    opt = Adam(learning_rate=1e-4)
    plan = m.plan(B)
    aug = Augmentator("scramble", size=s["patch"], seed=1)
    host = iter(data.ArrayDataset(host_x, B, True, 0, "cuda"))
    rds = data.ResidentDataset(raw, B, True, 0, "cuda")
    res = rds.index_batches()
    x = data.synthetic_images(B, H, H, seed=0, device="cuda")
    variants = {
        "host": lambda: trainer.train_step(m, aug.augment(next(host)), opt, keep_recon=False),
        "resident": lambda: trainer.train_step(m, aug.augment_from(rds, next(res), plan=plan), opt, keep_recon=False),
        "synthetic": lambda: trainer.train_step(m, aug.augment(x, plan=plan), opt, keep_recon=False),
    }
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    per = {k: [] for k in variants}
    gc.collect()
    gc.disable()
    try:
        for _ in range(rounds):
            for k, fn in variants.items():
                per[k].append(window(fn, steps))
    finally:
        gc.enable()
    row = {"dataset": name, "source": s["kind"], "N": s["N"], "H": H, "batch": B, "dtype": dtype, "patch": s["patch"], "steps": steps,
           "warmup": warmup, "rounds": rounds, "unit": "images/s"}
    for k, ts in per.items():
        med = statistics.median(ts)
        row[k] = round(B / med, 1)
        row[k + "_ms_per_step"] = round(1e3 * med, 4)
        row[k + "_rounds_ms"] = [round(1e3 * t, 4) for t in ts]
        row[k + "_spread"] = round((max(ts) - min(ts)) / med, 4)
    row["resident_over_host"] = round(row["resident"] / row["host"], 3)
    row["resident_over_synthetic"] = round(row["resident"] / row["synthetic"], 3)
    row["resident_faster"] = bool(max(per["resident"]) < min(per["host"]))
    print(json.dumps(row), flush=True)
    del m, plan, rds, host
    torch.cuda.empty_cache()
    return row


def pair_bytes(B, H, tsize):
    """Compulsory traffic of one fetch + scramble + staging pass, from the shapes: the batch read once (the scrambled half's second
    read of the same image is served by the caches), index / perm, images6 and the two padded 8-channel tensors written."""
    return B * H * H * 3 * 4 + B * H * H * 6 * 4 + 2 * B * H * H * 8 * tsize


def kernel_pair(reps):
    """Fused kernel, then the existing two (gather + scramble_staged_kernel), on the same batch, `reps` times per staged dtype."""
    import torch
    from split_vae_amd import data, ops
    B, H, patch = 512, 64, 8
    raw = make_set("celeba64")
    rds = data.ResidentDataset(raw, B, True, 0, "cuda")
    index = next(rds.index_batches())
    perm = ops.random_perm(B, (H // patch) ** 2, 1, 0, 0, "cuda")
    for tdt in (torch.float32, torch.bfloat16):
        staged = tuple(torch.empty((B, H, H, 8), dtype=tdt, device="cuda") for _ in range(2))
        for _ in range(reps):
            ops.dataset_gather_scramble(rds.data, index, perm, patch, staged=staged)
            x = ops.dataset_gather(rds.data, index)
            ops.scramble_gather(x, perm, patch, staged=staged)
        torch.cuda.synchronize()
    print(json.dumps({"batch": B, "H": H, "patch": patch, "reps": reps, "bytes_f32": pair_bytes(B, H, 4), "bytes_bf16": pair_bytes(B, H, 2)}))


def summarise(trace):
    """Kernel-trace CSV of the --kernel-pair run -> a table: per kernel the dispatch count, median / fastest / slowest duration, bytes over the median."""
    B, H = 512, 64
    rows = {}
    with open(trace, newline="") as f:
        for r in csv.DictReader(f):
            n = r["Kernel_Name"]
            if "scramble" in n or "dataset_gather" in n:
                rows.setdefault(n, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    print("# rocprofv3 --kernel-trace --stats -- python scripts/bench_input.py --kernel-pair ; python scripts/bench_input.py --summarise <kernel trace>")
    print("# CelebA-64 fp32, B = 512, patch 8 (MI355X).  bytes = batch read once + images6 + in8_x + in8_xh (from the shapes); share of the 8 TB/s peak;")
    print("# beside it the share of the measured 6.29 TB/s device copy.  spread = (max - min) / median over the repeated launches.")
    print("%-96s %5s %8s %8s %8s %7s %9s %7s %7s" % ("kernel", "calls", "med_us", "min_us", "max_us", "spread", "TB/s", "of_8.0", "of_6.29"))
    for n, d in sorted(rows.items(), key=lambda kv: -statistics.median(kv[1])):
        bf16 = "DF16b" in n or "bf16" in n.lower() or "_Accum" in n          # (some demanglers print __bf16 as `bool _Accum`)
        med = statistics.median(d)
        if "dataset_gather_f32" in n or "dataset_gather_u8" in n:
            nbytes = 2 * B * H * H * 3 * 4                       # the plain gather: a copy
        else:
            nbytes = pair_bytes(B, H, 2 if bf16 else 4)
        bw = nbytes / (med * 1e-6)
        print("%-96s %5d %8.2f %8.2f %8.2f %7.3f %9.3f %7.3f %7.3f" % (n[:96], len(d), med, min(d), max(d), (max(d) - min(d)) / med, bw / 1e12,
                                                                       bw / HBM_PEAK, bw / COPY_MEASURED))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--kernel-pair", action="store_true")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--summarise", type=str, default=None)
    a = ap.parse_args()
    if a.summarise:
        return summarise(a.summarise)
    import split_vae_amd
    split_vae_amd.configure_hw_queues()
    import torch
    assert torch.cuda.is_available(), "bench_input.py needs the MI355X"
    if a.kernel_pair:
        return kernel_pair(a.reps)
    from split_vae_amd import data
    rows, cache = [], {}
    for name, H, B, dtype in ROWS:
        if name not in cache:
            cache.clear()
            raw = make_set(name)
            cache[name] = (raw, data.normalise_u8(raw) if raw.dtype.name == "uint8" else raw)   # the host path holds fp32, as get_dataset does
        raw, host_x = cache[name]
        rows.append(run_row(name, raw, host_x, B, dtype, a.steps, a.warmup, a.rounds))
    line = json.dumps({"rows": rows, "note": "host = ArrayDataset -> augment -> train_step; resident = ResidentDataset -> augment_from(plan) -> train_step; "
                                             "synthetic = the pre-staged loop bench.py times; spread = (max - min) / median over the rounds of one variant"})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
