"""k-nearest-neighbour label probe of the global and local latents: do the labels live in z_g and not in z_l?

No reference counterpart: Table 1's probe classifier (vae/trainer.py:81-97) needs a weights blob that is missing upstream
(.MISSING_LARGE_BLOBS:1).  This is the parameter-free stand-in: encode a labelled reference set and the labelled test set, classify
every test latent mean by the majority label of its k nearest reference latent means (sv_knn_classify, include/splitvae.h), and
report the accuracy separately for z_g (the encoder of x) and z_l (the encoder of the scrambled x_hat).  Deterministic; apart from
k it has no parameters.  lgvae and lggmvae report both latents, gmvae z_g only.
"""
import torch

from . import ops, reports
from ._lib import KNN_MAX_K
from .utils import images_of

REPORT = 'Test k-NN probe (k={}, {} refs): z_g acc {:.4f}'
REPORT_L = ', z_l acc {:.4f}'
SKIPPED = 'Note: --knn_probe needs labels; skipped'


def check_flags(knn_probe, knn_refs, no_label):
    """--knn_probe / --knn_refs, before any data or device work (main.py, evaluate.py)."""
    if knn_probe < 0 or knn_probe > KNN_MAX_K:
        raise SystemExit("--knn_probe K: 0 (off) or 1 <= K <= %d neighbours, got %d" % (KNN_MAX_K, knn_probe))
    if not knn_probe:
        return
    if no_label:
        raise SystemExit("--knn_probe classifies latents by the labels of their neighbours: it cannot run with -no_label")
    if knn_refs < knn_probe:
        raise SystemExit("--knn_refs %d: the probe needs at least K = %d reference images" % (knn_refs, knn_probe))


def _means(model, images):
    """(z_mean_x, z_mean_x_hat or None) of one batch, as views of buffers the next batch overwrites."""
    from .latent_info import batch_posterior
    mean_g, _, mean_l, _ = batch_posterior(model, images)
    return mean_g, mean_l


def latent_means(model, batches):
    """The encoders' means over `batches` ([B,H,W,6] device batches, or (images, labels) pairs) -> device tensors (z_g [N,Lg],
    z_l [N,Ll] or None for GMVae).  LGVae runs its encoders only.  LGGMVae / GMVae run the model's forward: their z_mean_x is
    computed behind the relaxed categorical sample y (vae/model.py:116-135), drawn at the model's current call counter -- every
    batch of one probe at the same counter.  Leaves model._calls alone."""
    zg, zl = [], []
    for batch in batches:
        images = images_of(batch)
        g, l = _means(model, images)
        zg.append(g.clone())
        if l is not None:
            zl.append(l.clone())
    if not zg:
        raise ValueError("latent_means: no batches")
    return torch.cat(zg), (torch.cat(zl) if zl else None)


def _class_ids(batches):
    """one-hot labels [B,C] of (images, labels) batches -> (uint8 class ids [N] on the device, C)"""
    ys = [b[1] for b in batches]
    return torch.cat([y.argmax(dim=1) for y in ys]).to(torch.uint8), int(ys[0].shape[1])


def knn_probe(model, ref_batches, test_batches, k):
    """dict(acc_g, acc_l (None for GMVae), n_ref, n_test, k): the accuracy of the k-NN classifier of the test latent means over
    the reference latent means.  Batches are (images6, one-hot labels) pairs.  The hits are counted on the device; one read-back."""
    ref_batches, test_batches = list(ref_batches), list(test_batches)
    rg, rl = latent_means(model, ref_batches)
    tg, tl = latent_means(model, test_batches)
    rc, n_class = _class_ids(ref_batches)
    tc, _ = _class_ids(test_batches)
    acc = torch.zeros((2, 2), dtype=torch.int64, device=rg.device)
    with ops.hold_stream():
        ops.knn_classify(tg, rg, rc, k, max(n_class, 2), q_class=tc, acc=acc[0])
        if rl is not None:
            ops.knn_classify(tl, rl, rc, k, max(n_class, 2), q_class=tc, acc=acc[1])
    a = acc.cpu().tolist()
    return dict(acc_g=a[0][0] / a[0][1], acc_l=(a[1][0] / a[1][1]) if rl is not None else None,
                n_ref=int(rg.shape[0]), n_test=int(tg.shape[0]), k=int(k), hits_g=a[0][0], hits_l=a[1][0] if rl is not None else None)


def reference_batches(train_ds, n, augmentor, batch_size):
    """The first `n` training images in file order (not shuffled) as (images6, one-hot labels) batches, from an ArrayDataset's
    x / y or from a ResidentDataset.  `augmentor` is an Augmentator of the probe's own: the draw counters of the training and test
    augmentors do not move."""
    if not getattr(train_ds, "labelled", False):
        raise ValueError("reference_batches needs a labelled training set")
    out = []
    if hasattr(train_ds, "gather"):                 # data.ResidentDataset
        n = min(int(n), train_ds.N)
        index = torch.arange(n, dtype=torch.int32, device=train_ds.device)
        for o in range(0, n, batch_size):
            idx = index[o:o + batch_size]
            out.append((augmentor.augment_from(train_ds, idx), train_ds.one_hot(idx)))
        return out
    n = min(int(n), train_ds.x.shape[0])
    for o in range(0, n, batch_size):
        x = torch.from_numpy(train_ds.x[o:min(o + batch_size, n)]).to(train_ds.device)
        y = torch.from_numpy(train_ds.y[o:min(o + batch_size, n)]).to(train_ds.device)
        out.append((x if augmentor.type == 'no_op' else augmentor.augment(x), y))
    return out


def report_line(res):
    line = REPORT.format(res["k"], res["n_ref"], res["acc_g"])
    return line + (REPORT_L.format(res["acc_l"]) if res.get("acc_l") is not None else '')


def report(model, test_batches, config, step=None):
    """--knn_probe K behind an evaluation's report (trainer.py, evaluate.py): prints the line, keeps dict(step, knn_acc_g, knn_acc_l) in
    config.knn_history and returns knn_probe's figures; None when the flag is off, the run has no labels or config.knn_ref_batches is empty."""
    return reports.run("knn_probe", model, test_batches, config, step)
