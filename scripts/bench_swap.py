"""Cost of the swap-consistency report (split_vae_amd/swap.py, csrc/swap.hip) at SVHN scale, in ONE process.

Part 1, per L in (128, 256): synthetic clustered latents (references: ten centres ~ N(0, I), points = centre + N(0, I); query q = its
first target's row + 0.3 N(0, I)), Nq = Nr = 26 032, two random target lists.  Between hipEvent pairs, after warm-up, alternating
inside a round:

  rank_ms    one ops.swap_rank call, box to box (gather, norms, thresholds, count pass, fold; workspace allocated outside)
  torch_ms   a chunked torch composition of the same definition: torch.cdist over query chunks of `--torch-chunk` rows, squared, the
             compare against the gathered target distance with the index tie rule, the count

Each figure is the median of `--rounds` blocks of `--calls` calls; `spread` = (max - min) / median.  `tf` = 2 Nq Nr L FLOP over rank_ms
and `mfma_peak_fraction` = tf / 157.3 (the fp32 matrix peak): a whole-call rate.  `agree` = the fraction of (query, list) ranks on
which the two paths agree (torch's distances round differently, so near ties may differ).

Part 2: the two small kernels at B = 64, 32 x 32 (the report's batch).  Part 3: the whole report for an SVHN-32 LGVae (latents 128/128,
random weights, synthetic images, one partner plus the unswapped pass), split into encoding the originals, the hybrids' decode
(pair, decoders, permutation, requantise), their re-encoding, and the four rank calls per pass.

    python scripts/bench_swap.py [--rounds 5] [--calls 3] [--out profiles/swap_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

N, PEAK_TF = 26032, 157.3


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


def torch_rank(q, r, t0, t1, chunk):
    import torch
    col = torch.arange(r.shape[0], device=q.device)[None, :]
    out = []
    for o in range(0, q.shape[0], chunk):
        d = torch.cdist(q[o:o + chunk], r).square_()
        both = []
        for t in (t0, t1):
            tt = t[o:o + chunk].long()[:, None]
            dt = d.gather(1, tt)
            hit = (d < dt) | ((d == dt) & (col < tt))
            hit.scatter_(1, tt, False)
            both.append(hit.sum(dim=1))
        out.append(torch.stack(both, dim=1))
    return torch.cat(out)


def rank_row(L, a):
    import torch
    from split_vae_amd import ops
    gen = torch.Generator(device="cuda").manual_seed(L)
    centres = torch.randn((10, L), generator=gen, device="cuda")
    r = centres[torch.randint(0, 10, (N,), generator=gen, device="cuda")] + torch.randn((N, L), generator=gen, device="cuda")
    t0 = torch.randint(0, N, (N,), generator=gen, device="cuda").to(torch.int32)
    t1 = torch.randint(0, N, (N,), generator=gen, device="cuda").to(torch.int32)
    q = r[t0.long()] + 0.3 * torch.randn((N, L), generator=gen, device="cuda")
    ws = torch.empty((ops.swap_rank_workspace_bytes(N, N, L),), dtype=torch.uint8, device="cuda")
    rank = torch.empty((N, 2), dtype=torch.int32, device="cuda")
    ours = lambda: ops.swap_rank(q, r, t0, t1, rank=rank, workspace=ws, check_range=False)      # noqa: E731
    theirs = lambda: torch_rank(q, r, t0, t1, a.torch_chunk)                                   # noqa: E731
    timed(ours, 2), timed(theirs, 2)
    to, tt = [], []
    for _ in range(a.rounds):
        to.append(timed(ours, a.calls))
        tt.append(timed(theirs, a.calls))
    p_ours, p_theirs = ours().long(), theirs()
    row = dict(Nq=N, Nr=N, L=L, swap_rank=med(to), torch_cdist_count=med(tt), torch_chunk=a.torch_chunk, workspace_mb=round(ws.numel() / 2 ** 20, 1))
    row["torch_over_swap_rank"] = round(row["torch_cdist_count"]["ms"] / row["swap_rank"]["ms"], 3)
    row["tf"] = round(2.0 * N * N * L / (row["swap_rank"]["ms"] * 1e-3) / 1e12, 2)
    row["mfma_peak_fraction"] = round(row["tf"] / PEAK_TF, 4)
    row["agree"] = round(float((p_ours == p_theirs).double().mean()), 5)
    row["rank0_share_t0"] = round(float((p_ours[:, 0] == 0).double().mean()), 4)
    return row


def small_row(a):
    import torch
    from split_vae_amd import data, ops
    B, H, Lg = 64, 32, 128
    gen = torch.Generator(device="cuda").manual_seed(1)
    mu = torch.randn((N, 2 * Lg), generator=gen, device="cuda")
    ig = torch.randint(0, N, (B,), generator=gen, device="cuda").to(torch.int32)
    il = torch.randint(0, N, (B,), generator=gen, device="cuda").to(torch.int32)
    zcat = torch.empty((B, 2 * Lg), dtype=torch.float32, device="cuda")
    out6 = torch.randn((B, H, H, 6), generator=gen, device="cuda")
    lut = torch.from_numpy(data.ResidentDataset.make_lut()).cuda()
    perm = ops.random_perm(B, (H // 4) ** 2, 1)
    images6 = torch.empty((B, H, H, 6), dtype=torch.float32, device="cuda")
    pair = lambda: ops.swap_pair(mu, ig, il, Lg, zcat, check_range=False)                  # noqa: E731
    requ = lambda: ops.swap_requantise(out6, lut, perm, 4, out=images6)                    # noqa: E731
    timed(pair, 5), timed(requ, 5)
    tp, tr = [], []
    for _ in range(a.rounds):
        tp.append(timed(pair, 50))
        tr.append(timed(requ, 50))
    return dict(B=B, H=H, Lg=Lg, Ll=Lg, patch=4, swap_pair=med(tp), swap_requantise=med(tr),
                requantise_gb_s=round((B * H * H * (12 + 12 + 24)) / (statistics.median(tr) * 1e-3) / 1e9, 1))


def report_row(a):
    import torch
    from split_vae_amd import data, ops, swap
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
    t_enc = timed(lambda: out.__setitem__("mu", posteriors(model, batches, n)))
    mu, _, Lg, Ll = out["mu"]
    cyc = swap._Cycle(model, mu, Lg, B, H, H, 4, model.seed)
    shifts = swap.partner_shifts(model.seed, n, 1)
    Q = torch.empty((2, n, Lg + Ll), dtype=torch.float32, device="cuda")
    ev = lambda: torch.cuda.Event(enable_timing=True)                               # noqa: E731
    marks = []
    for pi, s in enumerate([0] + shifts):
        for o, take, ig, il, offset in cyc.batches(s, pi * n):
            e0, e1, e2 = ev(), ev(), ev()
            e0.record()
            images6 = cyc.hybrids(ig, il, offset)
            e1.record()
            mg, _, ml, _ = batch_posterior(model, images6, o)
            Q[pi, o:o + take, :Lg] = mg[:take]
            Q[pi, o:o + take, Lg:] = ml[:take]
            e2.record()
            marks.append((e0, e1, e2))
    torch.cuda.synchronize()
    t_dec = sum(e0.elapsed_time(e1) for e0, e1, _ in marks)
    t_re = sum(e1.elapsed_time(e2) for _, e1, e2 in marks)
    ar = torch.arange(n, device="cuda")
    ti = ar.to(torch.int32)
    ws = torch.empty((ops.swap_rank_workspace_bytes(n, n, max(Lg, Ll)),), dtype=torch.uint8, device="cuda")

    def ranks():
        for pi, s in enumerate([0] + shifts):
            tj = ((ar + s) % n).to(torch.int32)
            ops.swap_rank(Q[pi][:, :Lg], mu[:, :Lg], ti, tj, workspace=ws, check_range=False)
            ops.swap_rank(Q[pi][:, Lg:], mu[:, Lg:], tj, ti, workspace=ws, check_range=False)
    ranks()
    t_rank = timed(ranks)
    t_all = timed(lambda: out.__setitem__("res", swap.evaluate(model, batches, n, 1, 10, patch=4)))
    res = out["res"]
    return dict(model="lgvae svhn-32 f32, latents 128/128, random weights", batch=B, n_images=n, partners=1, encode_originals_ms=round(t_enc, 2),
                decode_hybrids_ms=round(t_dec, 2), reencode_hybrids_ms=round(t_re, 2), rank_ms=round(t_rank, 3),
                evaluate_wall_ms=round(t_all, 2), kept1_g=res["kept1_g"], kept1_l=res["kept1_l"], cycle1_g=res["cycle1_g"], cycle1_l=res["cycle1_l"])


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
        raise SystemExit("bench_swap.py needs the GPU: no timing without one")
    rows = []
    for L in (128, 256):
        rows.append(rank_row(L, a))
        print(json.dumps(rows[-1]), flush=True)
    small = small_row(a)
    print(json.dumps(small), flush=True)
    e2e = report_row(a)
    print(json.dumps(e2e), flush=True)
    out = dict(device=torch.cuda.get_device_name(0), timing="hipEvent pairs; median over rounds of blocks of calls",
               fp32_matrix_peak_tf=PEAK_TF, rows=rows, small_kernels=small, report_end_to_end=e2e)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
