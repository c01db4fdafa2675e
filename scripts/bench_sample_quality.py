"""Cost of the sample-quality report (split_vae_amd/sample_quality.py, csrc/prdc.hip) at SVHN scale, in ONE process.

Part 1, per L in (256, 512): synthetic clustered features (ten centres ~ N(0, I), points = centre + N(0, I); the queries a second draw of
the same recipe), Nq = Nr = 26 032, k = 5.  Between hipEvent pairs, after warm-up, alternating inside a round:

  count_ms        one ops.prdc_count call, box to box (norms, count pass, fold; workspace allocated outside)
  radius_ms       one ops.prdc_radius call, box to box (sv_knn_classify's (k+1)-lists of the set against itself, then the pick)
  torch_count_ms  a chunked torch composition of the same definition: torch.cdist over query chunks of `--torch-chunk` rows, squared, the
                  compare against the per-column radii, the sum, the row minimum with its index
  torch_radius_ms the same chunks with the diagonal set to +inf and torch.kthvalue
  swap_rank_ms    one ops.swap_rank call at the same shape: the same tile and a comparable epilogue (two compares against per-ROW
                  thresholds), so count_ms / swap_rank_ms says what the per-column epilogue with its minimum costs

Each figure is the median of `--rounds` blocks of `--calls` calls; `spread` = (max - min) / median.  `tf` = 2 Nq Nr L FLOP over the time
and `mfma_peak_fraction` = tf / 157.3 (the fp32 matrix peak): whole-call rates.  `agree_*` = the fraction of outputs on which the device
and the torch path agree (torch's distances round differently, so near ties may differ).

Part 2: the whole report for an SVHN-32 LGVae (latents 128 / 128, random weights, synthetic images) by stage: encoding the test images,
per fake set the decode (draw, decoders, permutation, requantise) and the re-encoding, then the radii, the counts and the Gram sums.

    python scripts/bench_sample_quality.py [--rounds 5] [--calls 3] [--out profiles/sample_quality_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

N, K, PEAK_TF = 26032, 5, 157.3


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


def torch_count(q, r, rad, chunk):
    import torch
    cnt, dmin, imin = [], [], []
    for o in range(0, q.shape[0], chunk):
        d = torch.cdist(q[o:o + chunk], r).square_()
        cnt.append((d <= rad[None, :]).sum(dim=1))
        m = d.min(dim=1)
        dmin.append(m.values)
        imin.append(m.indices)
    return torch.cat(cnt), torch.cat(dmin), torch.cat(imin)


def torch_radius(x, k, chunk):
    import torch
    out = []
    for o in range(0, x.shape[0], chunk):
        d = torch.cdist(x[o:o + chunk], x).square_()
        n = d.shape[0]
        d[torch.arange(n, device=x.device), torch.arange(o, o + n, device=x.device)] = float("inf")
        out.append(torch.kthvalue(d, k, dim=1).values)
    return torch.cat(out)


def kernel_row(L, a):
    import torch
    from split_vae_amd import ops
    gen = torch.Generator(device="cuda").manual_seed(L)
    centres = torch.randn((10, L), generator=gen, device="cuda")
    draw = lambda: centres[torch.randint(0, 10, (N,), generator=gen, device="cuda")] + torch.randn((N, L), generator=gen, device="cuda")      # noqa: E731
    r, q = draw(), draw()
    ws = torch.empty((ops.prdc_workspace_bytes(N, N, L, K),), dtype=torch.uint8, device="cuda")
    rad = ops.prdc_radius(r, K, workspace=ws).clone()
    cnt, dmin, imin = (torch.empty((N,), dtype=dt, device="cuda") for dt in (torch.int32, torch.float32, torch.int32))
    radb = torch.empty((N,), dtype=torch.float32, device="cuda")
    t0 = torch.randint(0, N, (N,), generator=gen, device="cuda").to(torch.int32)
    t1 = torch.randint(0, N, (N,), generator=gen, device="cuda").to(torch.int32)
    wss = torch.empty((ops.swap_rank_workspace_bytes(N, N, L),), dtype=torch.uint8, device="cuda")
    rank = torch.empty((N, 2), dtype=torch.int32, device="cuda")
    fns = dict(prdc_count=lambda: ops.prdc_count(q, r, rad, cnt=cnt, dmin=dmin, imin=imin, workspace=ws),
               prdc_radius=lambda: ops.prdc_radius(r, K, rad=radb, workspace=ws),
               torch_count=lambda: torch_count(q, r, rad, a.torch_chunk),
               torch_radius=lambda: torch_radius(r, K, a.torch_chunk),
               swap_rank=lambda: ops.swap_rank(q, r, t0, t1, rank=rank, workspace=wss, check_range=False))
    for fn in fns.values():
        timed(fn, 2)
    times = {name: [] for name in fns}
    for _ in range(a.rounds):
        for name, fn in fns.items():
            times[name].append(timed(fn, a.calls))
    row = dict(Nq=N, Nr=N, L=L, k=K, torch_chunk=a.torch_chunk, workspace_mb=round(ws.numel() / 2 ** 20, 1))
    row.update({name: med(v) for name, v in times.items()})
    flop = 2.0 * N * N * L
    for name in ("prdc_count", "prdc_radius", "swap_rank"):
        row[name]["tf"] = round(flop / (row[name]["ms"] * 1e-3) / 1e12, 2)
        row[name]["mfma_peak_fraction"] = round(row[name]["tf"] / PEAK_TF, 4)
    row["torch_over_prdc_count"] = round(row["torch_count"]["ms"] / row["prdc_count"]["ms"], 3)
    row["torch_over_prdc_radius"] = round(row["torch_radius"]["ms"] / row["prdc_radius"]["ms"], 3)
    row["prdc_count_over_swap_rank"] = round(row["prdc_count"]["ms"] / row["swap_rank"]["ms"], 3)
    tc, td, ti = torch_count(q, r, rad, a.torch_chunk)
    fns["prdc_count"](), fns["prdc_radius"]()
    row["agree_cnt"] = round(float((cnt.long() == tc).double().mean()), 5)
    row["agree_imin"] = round(float((imin.long() == ti).double().mean()), 5)
    row["max_rel_dmin"] = float(((dmin - td).abs() / td.clamp_min(1e-30)).max())
    row["max_rel_radius"] = float(((radb - torch_radius(r, K, a.torch_chunk)).abs() / radb.clamp_min(1e-30)).max())
    row["positive_share"] = round(float((cnt > 0).double().mean()), 4)
    return row


def report_row(a):
    import torch
    from split_vae_amd import data, ops, sample_quality as sq
    from split_vae_amd.augmentation import Augmentator
    from split_vae_amd.latent_info import batch_posterior, posteriors
    from split_vae_amd.model import LGVae
    B, H, n = a.batch, 32, a.images
    model = LGVae(128, 128, image_shape=[-1, H, H, 3], dtype="f32", device="cuda", seed=3)
    aug = Augmentator("scramble", size=4, seed=1)
    pool = [aug.augment(data.synthetic_images(B, H, H, seed=s, device="cuda")) for s in range(8)]
    batches = [pool[i % len(pool)] for i in range((n + B - 1) // B)]
    posteriors(model, batches[:2])                                                  # plans, code objects
    out = {}
    t_enc = timed(lambda: out.__setitem__("mu", posteriors(model, batches, n, keyed=True)))
    X, _, Lg, Ll = out["mu"]
    cyc = sq._Samples(model, X, Lg, B, H, H, 4, model.seed)
    ev = lambda: torch.cuda.Event(enable_timing=True)                               # noqa: E731
    marks, Ys = [], {}
    for name in sq.set_names(model):
        Y = torch.empty((n, Lg + Ll), dtype=torch.float32, device="cuda")
        for o in range(0, n, B):
            idx = torch.arange(o, o + B, dtype=torch.int64, device="cuda").clamp_(max=n - 1)
            take = min(B, n - o)
            e0, e1, e2 = ev(), ev(), ev()
            e0.record()
            images6 = cyc.samples(name, X.index_select(0, idx), o)
            e1.record()
            mg, _, ml, _ = batch_posterior(model, images6, o)
            Y[o:o + take, :Lg] = mg[:take]
            Y[o:o + take, Lg:] = ml[:take]
            e2.record()
            marks.append((e0, e1, e2))
        Ys[name] = Y
    torch.cuda.synchronize()
    t_dec = sum(e0.elapsed_time(e1) for e0, e1, _ in marks)
    t_re = sum(e1.elapsed_time(e2) for _, e1, e2 in marks)
    ws = torch.empty((ops.prdc_workspace_bytes(n, n, Lg + Ll, K),), dtype=torch.uint8, device="cuda")
    rad_x = ops.prdc_radius(X, K, workspace=ws).clone()
    rads = {name: ops.prdc_radius(Y, K, workspace=ws).clone() for name, Y in Ys.items()}

    def radii():
        ops.prdc_radius(X, K, workspace=ws)
        for Y in Ys.values():
            ops.prdc_radius(Y, K, workspace=ws)

    def counts():
        for name, Y in Ys.items():
            ops.prdc_count(Y, X, rad_x, workspace=ws)
            ops.prdc_count(X, Y, rads[name], workspace=ws)

    def grams():
        ops.linprobe_gram(X)
        for Y in Ys.values():
            ops.linprobe_gram(Y)
    for fn in (radii, counts, grams):
        fn()
    t_rad, t_cnt, t_gram = timed(radii), timed(counts), timed(grams)
    t_all = timed(lambda: out.__setitem__("res", sq.evaluate(model, batches, n, K, patch=4)))
    res = out["res"]
    row = dict(model="lgvae svhn-32 f32, latents 128/128, random weights", batch=B, n_images=n, k=K, fake_sets=len(Ys),
               encode_ms=round(t_enc, 2), decode_ms=round(t_dec, 2), reencode_ms=round(t_re, 2), radii_ms=round(t_rad, 3),
               counts_ms=round(t_cnt, 3), gram_ms=round(t_gram, 3), evaluate_wall_ms=round(t_all, 2))
    for name in res["sets"]:
        row[name] = {key: round(res[key + "_" + name], 4) for key in sq.KEYS}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--torch-chunk", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=64, help="batch of the whole report (the CLI's default --batch_size)")
    ap.add_argument("--images", type=int, default=N, help="images of the whole report")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import split_vae_amd
    split_vae_amd.configure_hw_queues()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sample_quality.py needs the GPU: no timing without one")
    rows = []
    for L in (256, 512):
        rows.append(kernel_row(L, a))
        print(json.dumps(rows[-1]), flush=True)
    e2e = report_row(a)
    print(json.dumps(e2e), flush=True)
    out = dict(device=torch.cuda.get_device_name(0), timing="hipEvent pairs; median over rounds of blocks of calls",
               fp32_matrix_peak_tf=PEAK_TF, rows=rows, report_end_to_end=e2e)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
