"""The LGVae CelebA-64 step (B=512, beta 120) under each augmentation, in ONE process, fp32 and bf16.

`scramble` (patch 8, the README command), `blur` and `mix_scramble --mix_per_image`, every one staged (Augmentator.augment(...,
plan=): the augmentation kernel writes the step's padded inputs).  The three alternate: `rounds` rounds, each timing `steps`
steps of every augmentation as 3 equal blocks (bench.py: timed_blocks); a row reports the median over its rounds' median blocks.
Beside the step, the augmentation call alone (its Philox draws + the kernel, staged), hipEvent-timed over `steps` back-to-back calls.
Per-kernel times: run this under `rocprofv3 --kernel-trace --stats` separately.  Prints one JSON line per (dtype, augmentation) and a
summary line with the ratios to `scramble`.

    python scripts/bench_augment.py [--steps 30] [--warmup 5] [--rounds 3] [--batch 512]
"""
import argparse
import gc
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

AUGS = (("scramble", dict(type="scramble", size=8)), ("blur", dict(type="blur")),
        ("mix_scramble_per_image", dict(type="mix_scramble", per_image=True)))


def aug_alone_ms(aug, x, plan, n):
    import torch
    for _ in range(3):
        aug.augment(x, plan=plan)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        aug.augment(x, plan=plan)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def run_dtype(dtype, B, steps, warmup, rounds):
    import torch
    from bench import timed_blocks
    from split_vae_amd import data, trainer
    from split_vae_amd.augmentation import ReferenceAugmentator as Augmentator
    from split_vae_amd.model import LGVae
    from split_vae_amd.optimizer import Adam
    H = 64
    x = data.synthetic_images(B, H, H, seed=0, device="cuda")
    m = LGVae(128, 128, image_shape=[-1, H, H, 3], dtype=dtype, device="cuda", seed=3)
    m.beta = 120.0
    opt = Adam(learning_rate=1e-4)
    plan = m.plan(B)
    augs = {name: Augmentator(seed=1, **kw) for name, kw in AUGS}

    def step(aug):
        trainer.train_step(m, aug.augment(x, plan=plan), opt, keep_recon=False)

    for name, _ in AUGS:
        for _ in range(warmup):
            step(augs[name])
    per = {name: [] for name, _ in AUGS}
    gc.collect()
    gc.disable()
    try:
        for _ in range(rounds):
            for name, _ in AUGS:
                t, _, _ = timed_blocks(lambda i: step(augs[name]), steps, blocks=3)
                per[name].append(1e3 * t)
    finally:
        gc.enable()
    rows = {}
    for name, _ in AUGS:
        rows[name] = {"dtype": dtype, "augmentation": name, "batch": B, "H": H, "staged": True,
                      "ms_per_step": round(statistics.median(per[name]), 4), "rounds_ms": [round(v, 4) for v in per[name]],
                      "augment_alone_ms": round(aug_alone_ms(augs[name], x, plan, steps), 4), "steps": steps, "warmup": warmup}
        print(json.dumps(rows[name]), flush=True)
    del m, plan
    torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=512)
    a = ap.parse_args()
    import split_vae_amd
    split_vae_amd.configure_hw_queues()
    import torch
    assert torch.cuda.is_available(), "bench_augment.py needs the MI355X"
    summary = {}
    for dtype in ("f32", "bf16"):
        rows = run_dtype(dtype, a.batch, a.steps, a.warmup, a.rounds)
        base = rows["scramble"]
        summary[dtype] = {name: {"step_over_scramble": round(r["ms_per_step"] / base["ms_per_step"], 4),
                                 "augment_over_scramble": round(r["augment_alone_ms"] / base["augment_alone_ms"], 4)}
                          for name, r in rows.items()}
    print(json.dumps({"summary": summary}))


if __name__ == "__main__":
    main()
