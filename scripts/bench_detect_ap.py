"""Cost of the detection average precision (split_vae_amd/detection.py, csrc/detect_ap.hip), in ONE process.

Part (a), the finish call at 16 000 records (a 1000-canvas test set) and 2^20 records (the accepted maximum): random records, a third
of them non-detections.  Between hipEvent pairs, after warm-up, alternating inside a round:

  finish_ms   one ops.detect_ap_finish call, box to box (chunk sort, merge rounds, the three scan passes, the final reduce; workspace
              and output allocated outside)
  torch_ms    what a user would otherwise write: torch.sort on the keys (sign bit flipped: they are unsigned), a gather of the masks,
              and per threshold cumsum, a division, a flipped cummax and a sum

`agree` = the largest relative difference between the two paths' AP_t; the integer outputs must be equal.  Each figure is the median
of `--rounds` blocks of `--calls` calls; `spread` = (max - min) / median.

Part (b), one full evaluation of a 1000-canvas Multi-Bird test set by an lg_spair model (batch 32: 32 labelled test_step calls, the
count accuracy read-back), with and without the detection report (one sv_detect_match per batch, one finish call and one read-back
per set), wall clock around a device synchronisation, alternating; the plain run is the evaluation as it was before the report
existed (test_step takes the same path when no detection state is passed).

    python scripts/bench_detect_ap.py [--rounds 7] [--calls 5] [--out profiles/detect_ap_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time


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


def torch_curve(keys, tps, G):
    """the same report from torch operators -> (ap [9], ap_un [9], tp [9], M) on the device"""
    import torch
    order = torch.sort(keys ^ (-2 ** 63)).indices
    k, m = keys[order], tps[order].to(torch.int64)
    det = (k >> 32) != -1                                             # the non-detection's high word, as a signed shift sees it
    M = det.sum()
    pos = torch.arange(1, k.numel() + 1, dtype=torch.float64, device=k.device)
    ap, ap_un, tp = [], [], []
    for t in range(9):
        hit = ((m >> t) & 1) * det
        p = torch.cumsum(hit, 0).to(torch.float64) / pos * det
        env = torch.flip(torch.cummax(torch.flip(p, [0]), 0).values, [0])
        ap.append((env * hit).sum() / G)
        ap_un.append((p * hit).sum() / G)
        tp.append(hit.sum())
    return torch.stack(ap), torch.stack(ap_un), torch.stack(tp), M


def finish_row(n, a):
    import torch
    from split_vae_amd import ops
    gen = torch.Generator(device="cuda").manual_seed(n)
    logits = torch.randn((n,), generator=gen, device="cuda") * 2.0 + 0.8
    ids = torch.randperm(n, generator=gen, device="cuda")
    u = logits.view(torch.int32).to(torch.int64)
    hi = torch.where(logits > 0, 0x7FFFFFFF - u, torch.full_like(u, 0xFFFFFFFF))
    keys = (hi << 32) | ids
    tps = torch.randint(0, 512, (n,), generator=gen, device="cuda").to(torch.int16) * (logits > 0)
    images = n // 16 + 1
    n_gt = torch.full((images,), 3, dtype=torch.int32, device="cuda")
    G = 3 * images
    ws = torch.empty((ops.detect_ap_workspace_bytes(n),), dtype=torch.uint8, device="cuda")
    out = torch.empty((ops.DETECT_AP_OUT,), dtype=torch.float64, device="cuda")
    ours = lambda: ops.detect_ap_finish(keys, tps, n_gt, workspace=ws, out=out)          # noqa: E731
    theirs = lambda: torch_curve(keys, tps, G)                                           # noqa: E731
    timed(ours, 3), timed(theirs, 3)
    to, tt = [], []
    for _ in range(a.rounds):
        to.append(timed(ours, a.calls))
        tt.append(timed(theirs, a.calls))
    o = ours().cpu()
    ap, ap_un, tp, M = (x.cpu() for x in theirs())
    ints = o.view(torch.int64)
    assert ints[18:27].tolist() == tp.tolist() and int(ints[27]) == int(M) and int(ints[28]) == G
    rel = float(((o[:18] - torch.cat([ap, ap_un])).abs() / torch.cat([ap, ap_un]).abs().clamp_min(1e-300)).max())
    row = dict(records=n, detections=int(M), boxes=G, finish=med(to), torch_sort_cumsum_cummax=med(tt),
               workspace_mb=round(ws.numel() / 2 ** 20, 2), agree=rel)
    row["torch_over_finish"] = round(row["torch_sort_cumsum_cummax"]["ms"] / row["finish"]["ms"], 3)
    return row


def evaluation_row(a):
    import torch
    from split_vae_amd import detection, multibird, spair, spair_main, spair_trainer
    from split_vae_amd.main import make_augmentors
    cfg = spair_main.default_config(model="lg_spair", latent_size=64, bg_latent_size=4, local_latent_size=4, patch_size=8, split_z_l=True,
                                    concat_z_what=True, dense_local=True, dense_bg=True)
    model = spair.get_model(cfg, seed=cfg.seed)
    _, tests, _, _ = multibird.get_cub_dataset("cub_solid_fixed", batch_size=cfg.batch_size, seed=cfg.seed)
    ds = tests[0]
    ds.augment = make_augmentors(cfg)[1].augment
    count_acc = spair_trainer.CountAccuracy(model.device)
    det = detection.DetectionAP(model.device, ds.boxes.shape[0], 16)

    def evaluate(with_report):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        seen = 0
        for imgs, labels in ds:
            B = imgs.shape[0]
            d = (det, ds.boxes[seen:seen + B], ds.n_boxes[seen:seen + B]) if with_report else None
            spair_trainer.test_step(model, imgs, cfg, labels, count_acc=count_acc, detection=d)
            seen += B
        acc = count_acc.result()
        count_acc.reset_states()
        res = None
        if with_report:
            res = det.result()
            det.reset_states()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, acc, res

    evaluate(True), evaluate(False)
    plain, full, res = [], [], None
    for _ in range(a.rounds):
        plain.append(evaluate(False)[0])
        ms, _, res = evaluate(True)
        full.append(ms)
    row = dict(model="lg_spair f32, latents 64/4/4", images=int(ds.boxes.shape[0]), batch=int(cfg.batch_size), plain=med(plain),
               with_detection_ap=med(full), mAP=res["mAP"], detections=res["detections"], boxes=res["boxes"])
    row["added_ms"] = round(row["with_detection_ap"]["ms"] - row["plain"]["ms"], 4)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import split_vae_amd
    split_vae_amd.configure_hw_queues()
    if not torch.cuda.is_available():
        raise SystemExit("bench_detect_ap.py needs the GPU: no timing without one")
    rows = []
    for n in (16000, 1 << 20):
        rows.append(finish_row(n, a))
        print(json.dumps(rows[-1]), flush=True)
    ev = evaluation_row(a)
    print(json.dumps(ev), flush=True)
    out = dict(device=torch.cuda.get_device_name(0), timing="finish: hipEvent pairs, median over rounds of blocks of calls; evaluation: wall "
               "clock between device synchronisations, median over rounds", finish=rows, evaluation=ev)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
