"""GMVae step against the LGGMVae step in ONE process (SVHN-32, y_size 30, tau 0.4, beta 40, alpha 40, patch 4), batch 64, fp32 and bf16.

The method of bench.py::gm_row: the augmentation stages the step's inputs (Augmentator.augment(..., plan=)), `warmup` steps, then
`steps` steps timed as 4 equal blocks (bench.py: timed_blocks), the median block reported.  Prints one JSON line per (model, dtype)
and a summary line with the ratio.

    python scripts/bench_gmvae.py [--steps 200] [--warmup 20] [--batch 64]
"""
import argparse
import gc
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def row(model_name, dtype, B, steps, warmup):
    import torch
    from bench import timed_blocks
    from split_vae_amd import data
    from split_vae_amd.augmentation import Augmentator
    from split_vae_amd.optimizer import Adam
    x = data.synthetic_images(B, 32, 32, seed=0, device="cuda")
    aug = Augmentator("scramble", size=4, seed=1)
    if model_name == "gmvae":
        from split_vae_amd.gmvae import GMVae, train_step_gm_vae as step
        m = GMVae(128, [-1, 32, 32, 3], 30, 0.4, dtype=dtype, device="cuda", seed=3)
    else:
        from split_vae_amd.gm import LGGMVae, train_step_lg_gm_vae as step
        m = LGGMVae(128, 128, [-1, 32, 32, 3], 30, 0.4, dtype=dtype, device="cuda", seed=3)
    m.beta, m.alpha = 40.0, 40.0
    opt = Adam(learning_rate=1e-4)
    plan = m.plan(B)
    for _ in range(warmup):
        step(m, aug.augment(x, plan=plan), opt)
    gc.collect()
    gc.disable()                                  # (as bench.py: no cyclic GC inside the timed window)
    try:
        t, blocks_ms, t_mean = timed_blocks(lambda i: step(m, aug.augment(x, plan=plan), opt), steps, blocks=4)
    finally:
        gc.enable()
    torch.cuda.synchronize()
    return {"model": model_name, "dtype": dtype, "batch": B, "ms_per_step": round(1e3 * t, 4), "blocks_ms": blocks_ms,
            "ms_per_step_mean": round(1e3 * t_mean, 4), "images_per_s": round(B / t, 1), "steps": steps, "warmup": warmup}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64)
    a = ap.parse_args()
    import split_vae_amd
    split_vae_amd.configure_hw_queues()
    import torch
    assert torch.cuda.is_available(), "bench_gmvae.py needs the MI355X"
    res = {}
    for dtype in ("f32", "bf16"):
        for name in ("gmvae", "lggmvae"):
            r = row(name, dtype, a.batch, a.steps, a.warmup)
            res[(name, dtype)] = r
            print(json.dumps(r), flush=True)
    print(json.dumps({"summary": {dt: {"gmvae_ms": res[("gmvae", dt)]["ms_per_step"], "lggmvae_ms": res[("lggmvae", dt)]["ms_per_step"],
                                       "gmvae_over_lggmvae": round(res[("gmvae", dt)]["ms_per_step"] / res[("lggmvae", dt)]["ms_per_step"], 4)}
                                  for dt in ("f32", "bf16")}}))


if __name__ == "__main__":
    main()
