"""SPLIT-SPAIR labelled evaluation at batch 32 with README.md:107's flags (Multi-Bird-Hard), in ONE process.

Rows:
- labelled `test_step` ms per batch on the native tape + sv_spair_count_metrics against the op-by-op forward (SV_SPAIR_AUTOGRAD=1, the
  labelled path before the native one existed).  The two alternate for `rounds` rounds; each round times `steps` batches as 3 equal
  blocks (bench.py: timed_blocks); a row reports the median over its rounds' median blocks;
- each new kernel alone (sv_spair_count_metrics on the batch's z_pres_logits, sv_draw_bounding_boxes on a 10-image 48x48x3 strip as
  reconstruction_bbox draws it), hipEvent-timed over `steps` back-to-back calls.
Per-kernel device times: run this under `rocprofv3 --kernel-trace --stats` separately.  Prints one JSON line per row and a summary.

    python scripts/bench_spair_eval.py [--steps 60] [--warmup 5] [--rounds 3] [--batch 32]
"""
import argparse
import gc
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# README.md:107 (SPLIT-SPAIR on Multi-Bird-Hard)
HARD = dict(model="lg_spair", z_bg_beta=1.0, patch_size=8, latent_size=64, bg_latent_size=64, local_latent_size=64, split_z_l=True,
            z_what_beta=0.5, concat_z_what=True, dense_local=True, dense_bg=True)


def alone_ms(fn, n):
    import torch
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    a = ap.parse_args()
    import split_vae_amd
    split_vae_amd.configure_hw_queues()
    import torch
    assert torch.cuda.is_available(), "bench_spair_eval.py needs the MI355X"
    from bench import timed_blocks
    from split_vae_amd import ops, spair, spair_main, spair_trainer
    from split_vae_amd.main import make_augmentors
    cfg = spair_main.default_config(**HARD)
    model = spair.get_model(cfg, seed=0)
    aug, _ = make_augmentors(cfg)
    x, labels = spair_main.synthetic_canvases(a.batch, seed=1)
    images = aug.augment(x)
    ca = spair_trainer.CountAccuracy()

    def step(native):
        if native:
            os.environ.pop("SV_SPAIR_AUTOGRAD", None)
        else:
            os.environ["SV_SPAIR_AUTOGRAD"] = "1"
        spair_trainer.test_step(model, images, cfg, labels=labels, count_acc=ca)

    forms = (("native", True), ("op_by_op", False))
    for _, nat in forms:
        for _ in range(a.warmup):
            step(nat)
    per = {name: [] for name, _ in forms}
    gc.collect()
    gc.disable()
    try:
        for _ in range(a.rounds):
            for name, nat in forms:
                t, _, _ = timed_blocks(lambda i: step(nat), a.steps, blocks=3)
                per[name].append(1e3 * t)
    finally:
        gc.enable()
        os.environ.pop("SV_SPAIR_AUTOGRAD", None)
    rows = {}
    for name, _ in forms:
        rows[name] = {"row": "test_step_labelled", "form": name, "batch": a.batch, "ms_per_batch": round(statistics.median(per[name]), 4),
                      "rounds_ms": [round(v, 4) for v in per[name]], "steps": a.steps, "warmup": a.warmup}
        print(json.dumps(rows[name]), flush=True)
    with torch.no_grad():
        o = model(images)
    logits = o[11]
    k_count = alone_ms(lambda: ops.spair_count_metrics(logits, labels, acc=ca.acc), a.steps)
    n = min(10, a.batch)
    strip = images[:n, ..., :3].contiguous()
    bbox, gate = o[17][:n].contiguous(), torch.round(torch.sigmoid(logits[:n])).reshape(n, -1).contiguous()
    white = torch.ones((1, 4), dtype=torch.float32, device=strip.device)
    out = torch.empty_like(strip)
    k_draw = alone_ms(lambda: ops.draw_bounding_boxes(strip, bbox, white, gate=gate, out=out), a.steps)
    kr = {"row": "kernels_alone", "sv_spair_count_metrics_ms": round(k_count, 5), "sv_draw_bounding_boxes_ms": round(k_draw, 5),
          "count_batch": a.batch, "draw_images": n, "calls": a.steps}
    print(json.dumps(kr), flush=True)
    print(json.dumps({"summary": {"op_by_op_over_native": round(rows["op_by_op"]["ms_per_batch"] / rows["native"]["ms_per_batch"], 3)}}))


if __name__ == "__main__":
    main()
