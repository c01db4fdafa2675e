"""Cost of the k-NN label probe (split_vae_amd/probe.py, csrc/knn.hip) at SVHN scale, in ONE process.

Part 1, per L in (128, 256): synthetic clustered latents (ten class centres ~ N(0, I), points = centre + N(0, I)), Nq = 26 032
queries against Nr = 73 257 references, k = 5.  Between hipEvent pairs, after warm-up, alternating inside a round:

  knn_ms     one ops.knn_classify call, box to box (norm pre-pass, tile kernel, merge-and-vote; workspace allocated outside)
  torch_ms   what a user would otherwise write: torch.cdist over query chunks of `--torch-chunk` rows + topk + a one-hot vote

Each figure is the median of `--rounds` blocks of `--calls` calls; `spread` = (max - min) / median.  `tf` = 2 Nq Nr L FLOP over
knn_ms and `mfma_peak_fraction` = tf / 157.3 (the fp32 matrix peak): a whole-call rate, selection and merge included, not the
tile kernel's own.  `agree` = the fraction of queries on which the two paths predict the same class.

Part 2: one end-to-end probe of an LGVae (SVHN-32, latents 128) at those sizes -- encoding the references, encoding the test set
(probe.latent_means over synthetic batches of `--batch` images) and the two classify calls (z_g, z_l), each timed separately.

    python scripts/bench_knn.py [--rounds 5] [--calls 3] [--out profiles/knn_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

NQ, NR, K, PEAK_TF = 26032, 73257, 5, 157.3


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


def clustered(n, L, gen, centres):
    import torch
    cls = torch.randint(0, 10, (n,), generator=gen, device="cuda")
    return centres[cls] + torch.randn((n, L), generator=gen, device="cuda"), cls.to(torch.uint8)


def torch_knn(q, r, r_class, k, n_class, chunk):
    import torch
    pred = []
    for o in range(0, q.shape[0], chunk):
        d = torch.cdist(q[o:o + chunk], r)
        idx = d.topk(k, dim=1, largest=False).indices
        votes = torch.nn.functional.one_hot(r_class[idx].long(), n_class).sum(dim=1)
        pred.append(votes.argmax(dim=1))
    return torch.cat(pred)


def kernel_row(L, a):
    import torch
    from split_vae_amd import ops
    gen = torch.Generator(device="cuda").manual_seed(L)
    centres = torch.randn((10, L), generator=gen, device="cuda")
    r, rc = clustered(NR, L, gen, centres)
    q, qc = clustered(NQ, L, gen, centres)
    ws = torch.empty((ops.knn_workspace_bytes(NQ, NR, K),), dtype=torch.uint8, device="cuda")
    ours = lambda: ops.knn_classify(q, r, rc, K, 10, workspace=ws)                 # noqa: E731
    theirs = lambda: torch_knn(q, r, rc, K, 10, a.torch_chunk)                     # noqa: E731
    timed(ours, 2), timed(theirs, 2)
    to, tt = [], []
    for _ in range(a.rounds):
        to.append(timed(ours, a.calls))
        tt.append(timed(theirs, a.calls))
    p_ours, p_theirs = ours(), theirs()
    row = dict(Nq=NQ, Nr=NR, L=L, k=K, knn=med(to), torch_cdist_topk=med(tt), workspace_mb=round(ws.numel() / 2 ** 20, 1))
    row["torch_over_knn"] = round(row["torch_cdist_topk"]["ms"] / row["knn"]["ms"], 3)
    row["tf"] = round(2.0 * NQ * NR * L / (row["knn"]["ms"] * 1e-3) / 1e12, 2)
    row["mfma_peak_fraction"] = round(row["tf"] / PEAK_TF, 4)
    row["agree"] = round(float((p_ours.long() == p_theirs).double().mean()), 5)
    row["accuracy"] = round(float((p_ours.long() == qc.long()).double().mean()), 5)
    return row


def probe_row(a):
    import torch
    from split_vae_amd import data, ops, probe
    from split_vae_amd.augmentation import Augmentator
    from split_vae_amd.model import LGVae
    B, H = a.batch, 32
    model = LGVae(128, 128, image_shape=[-1, H, H, 3], dtype="f32", device="cuda", seed=3)
    aug = Augmentator("scramble", size=4, seed=1)
    pool = [aug.augment(data.synthetic_images(B, H, H, seed=s, device="cuda")) for s in range(8)]

    def batches(n):
        return [pool[i % len(pool)][:min(B, n - o)] for i, o in enumerate(range(0, n, B))]
    refs, tests = batches(NR), batches(NQ)
    probe.latent_means(model, tests[:4])                                           # plans, code objects
    out = {}
    t_ref = timed(lambda: out.__setitem__("r", probe.latent_means(model, refs)))
    t_test = timed(lambda: out.__setitem__("t", probe.latent_means(model, tests)))
    (rg, rl), (tg, tl) = out["r"], out["t"]
    gen = torch.Generator(device="cuda").manual_seed(1)
    rc = torch.randint(0, 10, (NR,), generator=gen, device="cuda").to(torch.uint8)
    tc = torch.randint(0, 10, (NQ,), generator=gen, device="cuda").to(torch.uint8)
    acc = torch.zeros((2, 2), dtype=torch.int64, device="cuda")
    ops.knn_classify(tg, rg, rc, K, 10)
    t_g = timed(lambda: ops.knn_classify(tg, rg, rc, K, 10, q_class=tc, acc=acc[0]))
    t_l = timed(lambda: ops.knn_classify(tl, rl, rc, K, 10, q_class=tc, acc=acc[1]))
    return dict(model="lgvae svhn-32 f32, latents 128/128", batch=B, n_ref=NR, n_test=NQ, k=K, encode_refs_ms=round(t_ref, 2),
                encode_tests_ms=round(t_test, 2), classify_z_g_ms=round(t_g, 3), classify_z_l_ms=round(t_l, 3),
                total_ms=round(t_ref + t_test + t_g + t_l, 2), counted=acc[:, 1].tolist())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--torch-chunk", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=64, help="encoder batch of the end-to-end probe (the CLI's default --batch_size)")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import split_vae_amd
    split_vae_amd.configure_hw_queues()
    if not torch.cuda.is_available():
        raise SystemExit("bench_knn.py needs the GPU: no timing without one")
    rows = []
    for L in (128, 256):
        rows.append(kernel_row(L, a))
        print(json.dumps(rows[-1]), flush=True)
    e2e = probe_row(a)
    print(json.dumps(e2e), flush=True)
    out = dict(device=torch.cuda.get_device_name(0), timing="hipEvent pairs; median over rounds of blocks of calls",
               fp32_matrix_peak_tf=PEAK_TF, rows=rows, probe_end_to_end=e2e)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
