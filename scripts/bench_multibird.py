"""Multi-Bird canvas synthesis (csrc/multibird.hip) on the MI355X, in ONE process -> profiles/multibird_bench.json.

Rows:
- the canvas kernel alone per 32-canvas batch, per background (layouts drawn in the launch, a device index[32]), hipEvent-timed over
  `--calls` back-to-back launches after warm-up (the default fills well over a tenth of a second);
- steps per second of the SPLIT-SPAIR train loop with README.md:107's flags on `--dataset cub_ckb_rot_6` (TrainCanvases: shuffle-buffer
  indices, one launch per batch, the augmentor) against the `--synthetic` loop (synthetic_canvases per step: a Python loop of torch CPU
  ops and a host-to-device copy, exactly as spair_main.batches() runs it), alternated, `--repeats` repeats of `--steps` steps each.
  The two loops train on DIFFERENT images: only time is compared.  `not_slower` = the new loop's median is within the old loop's own
  repeat-to-repeat spread (max - min) of the old median, or faster.
Per-kernel device times: run under `rocprofv3 --kernel-trace --stats` separately (`--kernel-only`).

    python scripts/bench_multibird.py [--steps 200] [--repeats 3] [--calls 20000] [--out profiles/multibird_bench.json] [--kernel-only]
"""
import argparse
import gc
import itertools
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# README.md:107 (SPLIT-SPAIR on Multi-Bird-Hard)
HARD = dict(model="lg_spair", z_bg_beta=1.0, patch_size=8, latent_size=64, bg_latent_size=64, local_latent_size=64, split_z_l=True,
            z_what_beta=0.5, concat_z_what=True, dense_local=True, dense_bg=True)


def kernel_rows(calls, B=32):
    import torch
    from split_vae_amd import multibird as mb
    from split_vae_amd import ops
    bank = torch.from_numpy(mb.procedural_bank(256, 0)).cuda()
    idx = torch.randint(0, mb.N_TRAIN, (B,), generator=torch.Generator().manual_seed(0)).cuda()
    x = torch.empty((B, 48, 48, 3), device="cuda")
    c = torch.empty((B,), device="cuda")
    rows = []
    for name, bg in mb.BACKGROUNDS.items():
        def call():
            ops.multibird_canvases(bank, bg, B, 0, 0, index=idx, x=x, count=c)
        with ops.hold_stream():
            for _ in range(200):
                call()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(calls):
                call()
            e1.record()
            torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        rows.append({"row": "kernel_alone", "background": name, "batch": B, "calls": calls, "window_ms": round(ms, 2),
                     "us_per_batch": round(1e3 * ms / calls, 3), "bytes_written_per_batch": B * 48 * 48 * 3 * 4})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def loop_rows(steps, repeats, warmup=10):
    import torch
    from split_vae_amd import multibird as mb
    from split_vae_amd import spair, spair_main, spair_trainer
    from split_vae_amd.main import make_augmentors
    cfg = spair_main.default_config(dataset="cub_ckb_rot_6", **HARD)
    aug, _ = make_augmentors(cfg)
    model = spair.get_model(cfg, seed=0)
    opt = spair_trainer.ClipnormAdam(cfg.learning_rate, clipnorm=1.0)
    train_ds, _, _, _ = mb.get_cub_dataset(cfg.dataset, batch_size=cfg.batch_size, seed=cfg.seed, n_test=32)

    def new_source():
        for x in train_ds:
            yield aug.augment(x)

    def old_source():                              # spair_main.batches() under --synthetic
        for i in itertools.count():
            x, _ = spair_main.synthetic_canvases(cfg.batch_size, seed=cfg.seed + 1 + i)
            yield aug.augment(x)

    sources = {"dataset_cub_ckb_rot_6": new_source(), "synthetic": old_source()}
    k = [0]

    def run(name, n):
        src = sources[name]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            spair_trainer.train_step(model, next(src), opt, k[0], cfg)
            k[0] += 1
        torch.cuda.synchronize()
        return n / (time.perf_counter() - t0)

    for name in sources:
        run(name, warmup)
    per = {name: [] for name in sources}
    gc.collect()
    gc.disable()
    try:
        for _ in range(repeats):
            for name in sources:
                per[name].append(run(name, steps))
    finally:
        gc.enable()
    rows = []
    for name, v in per.items():
        rows.append({"row": "train_loop", "source": name, "batch": cfg.batch_size, "steps": steps, "steps_per_s": [round(s, 2) for s in v],
                     "median_steps_per_s": round(statistics.median(v), 2), "spread_steps_per_s": round(max(v) - min(v), 2),
                     "ms_per_step": round(1e3 / statistics.median(v), 4)})
        print(json.dumps(rows[-1]), flush=True)
    new, old = rows[0], rows[1]
    summary = {"row": "summary", "new_over_old_steps_per_s": round(new["median_steps_per_s"] / old["median_steps_per_s"], 4),
               "old_spread_steps_per_s": old["spread_steps_per_s"],
               "not_slower": new["median_steps_per_s"] >= old["median_steps_per_s"] - old["spread_steps_per_s"],
               "note": "the two loops train on different images: only time is compared"}
    print(json.dumps(summary), flush=True)
    return rows + [summary]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20000)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "multibird_bench.json"))
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args()
    import split_vae_amd
    split_vae_amd.configure_hw_queues()
    import torch
    assert torch.cuda.is_available(), "bench_multibird.py needs the MI355X"
    rows = kernel_rows(a.calls)
    if not a.kernel_only:
        rows += loop_rows(a.steps, a.repeats)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
