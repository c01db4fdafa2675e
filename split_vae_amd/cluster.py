"""k-means cluster report of the global and local latents: do the clusters of z_g line up with the classes, those of z_l not, and
are the two clusterings independent of each other?

No reference counterpart.  The paper's Table 2 reports the unsupervised cluster accuracy of the mixture models, whose y head names
a cluster per image (gmvae.cluster_accuracy).  The plain SPLIT-VAE has no such head; k-means on the latent means (sv_kmeans_*,
include/splitvae.h: k-means++ seeding, R restarts in one pass, the restart with the lowest inertia) gives it clusters, and the same
majority-class accuracy (gmvae.accuracy_from_counts) over the cluster / class table gives it a row on that axis.  The normalised
mutual information of the z_g clusters and the z_l clusters needs no labels.  lgvae and lggmvae report both latents, gmvae z_g only.

    python -m split_vae_amd.cluster --weights models/20260101-120000.h5 --dataset svhn --clusters 10
    python -m split_vae_amd.cluster --weights models/20260101-120000.h5 --dataset celeba64 -no_label --clusters 30 --cluster_images 10000

The command takes the flags of split_vae_amd.main plus --weights, --clusters, --cluster_images, --cluster_restarts, --cluster_iters.
It is an entry point of its own: reports.TABLE and the parsers of main / evaluate do not know it.
"""
import numpy as np
import torch

from . import ops
from ._lib import KMEANS_MAX_K, KMEANS_MAX_L, KMEANS_MAX_N, KMEANS_MAX_R

REPORT = 'Test k-means ({} clusters, {} images, {} restarts): z_g '
UNLABELLED = 'Note: no labels: the k-means report prints the label-free figures only'
CLIPPED = 'Note: --cluster_images {} clipped to the test set\'s {} images'
MAX_CLASSES = 64                                   # sv_contingency's table


def kmeans(x, k, restarts=8, iters=100, seed=0):
    """k-means of the rows of x [N,L] (fp32 device tensor; a row pitch above L is allowed): `restarts` fits from k-means++ seeds of
    (seed, r), at most `iters` updates each.  -> dict(centroids [R,k,L], assign [R,N] int32, counts [R,k] int32: device tensors;
    inertia [R], n_iter [R], best, empty (the number of empty clusters of the best restart): host values from one read-back)."""
    fit = kmeans_enqueue(x, k, restarts, iters, seed)
    return dict(fit, **_read(fit, _figures(fit)))


def kmeans_enqueue(x, k, restarts, iters, seed):
    """The device half of kmeans(): seeds, iterates, picks the best restart; nothing is read back.  Adds `best_dev` [1] int32 to the fit."""
    N, L = x.shape
    with ops.hold_stream():
        ws = torch.empty((ops.kmeans_workspace_bytes(N, L, k, restarts),), dtype=torch.uint8, device=x.device)
        cent = ops.kmeans_seed(x, k, restarts, seed=seed, workspace=ws)
        fit = ops.kmeans_iterate(x, ops.kmeans_state(x, cent), iters, workspace=ws)
        fit["best_dev"] = ops.kmeans_best(fit["inertia"])
    return fit


def _figures(fit):
    """[2R + 2] fp64 on the device: inertia, n_iter, best, empty clusters of the best restart"""
    best = fit["best_dev"].long()
    empty = (fit["counts"].index_select(0, best) == 0).sum().reshape(1)
    return torch.cat([fit["inertia"], fit["n_iter"].double(), best.double(), empty.double()])


def _read(fit, host):
    R = fit["inertia"].numel()
    host = host.cpu().numpy() if torch.is_tensor(host) else host
    return dict(inertia=host[:R].copy(), n_iter=host[R:2 * R].astype(np.int32), best=int(host[2 * R]), empty=int(host[2 * R + 1]))


def nmi(table):
    """2 I(A; B) / (H(A) + H(B)) (arithmetic-mean normalisation) of an integer contingency table, in float64; 1 when both partitions
    are trivial."""
    t = np.asarray(table, np.float64)
    n = t.sum()
    if n <= 0:
        return 0.0
    p = t / n
    pa, pb = p.sum(axis=1), p.sum(axis=0)
    ha = -(pa[pa > 0] * np.log(pa[pa > 0])).sum()
    hb = -(pb[pb > 0] * np.log(pb[pb > 0])).sum()
    if ha + hb <= 0:
        return 1.0
    nz = p > 0
    mi = (p[nz] * np.log(p[nz] / np.outer(pa, pb)[nz])).sum()
    return float(max(0.0, 2.0 * mi / (ha + hb)))


def _labels(batches, n):
    """int32 class ids [n] on the device and the number of classes when the batches are (images, one-hot labels) pairs, else (None, 0)"""
    ys, have = [], 0
    for b in batches:
        if have >= n:
            break
        if not isinstance(b, (tuple, list)) or len(b) < 2 or b[1] is None:
            return None, 0
        ys.append(b[1])
        have += b[1].shape[0]
    return torch.cat([y.argmax(dim=1) for y in ys])[:n].to(torch.int32).contiguous(), int(ys[0].shape[1])


def evaluate(model, test_batches, n, k, restarts=8, iters=100, seed=None):
    """The report over the latent means of the first `n` test images (all when there are fewer): one fit per latent block.
    -> dict(n_images, k, restarts, labelled; per block s in (g, l): acc_s, nmi_s (None without labels), inertia_s (per image), n_iter_s,
    empty_s; nmi_gl, the NMI of the two clusterings; tables: table_g / table_l [k, classes], table_gl [k, k] as int64 arrays).  The l
    entries are None for GMVae.  seed: model.seed.  One read-back."""
    from .gmvae import accuracy_from_counts
    from .latent_info import posteriors
    test_batches = list(test_batches)
    mu, _, Lg, Ll = posteriors(model, test_batches, int(n))
    N = int(mu.shape[0])
    if N < k:
        raise ValueError("cluster.evaluate: %d clusters need at least as many images, got %d" % (k, N))
    seed = model.seed if seed is None else seed
    cls, C = _labels(test_batches, N)
    if cls is not None and C > MAX_CLASSES:
        raise ValueError("cluster.evaluate: at most %d classes, got %d" % (MAX_CLASSES, C))
    blocks = [("g", mu[:, :Lg])] + ([("l", mu[:, Lg:])] if Ll else [])
    fits, parts, tables = {}, [], {}
    with ops.hold_stream():
        for s, z in blocks:
            fits[s] = kmeans_enqueue(z, k, restarts, iters, seed)
            fits[s]["best_assign"] = fits[s]["assign"].index_select(0, fits[s]["best_dev"].long()).reshape(-1).contiguous()
            parts.append(_figures(fits[s]))
            if cls is not None:
                tables["table_" + s] = ops.contingency(fits[s]["best_assign"], cls, torch.zeros((k, C), dtype=torch.int32, device=mu.device))
        if Ll:
            tables["table_gl"] = ops.contingency(fits["g"]["best_assign"], fits["l"]["best_assign"],
                                                 torch.zeros((k, k), dtype=torch.int32, device=mu.device))
        names = sorted(tables)
        host = torch.cat(parts + [tables[t].reshape(-1).double() for t in names]).cpu().numpy()      # the one read-back
    res = dict(n_images=N, k=int(k), restarts=int(restarts), labelled=cls is not None, acc_l=None, nmi_l=None, inertia_l=None,
               n_iter_l=None, empty_l=None, nmi_gl=None, acc_g=None, nmi_g=None)
    o = 0
    for s, _ in blocks:
        f = _read(fits[s], host[o:o + 2 * restarts + 2])
        o += 2 * restarts + 2
        res.update({"inertia_" + s: float(f["inertia"][f["best"]]) / N, "n_iter_" + s: int(f["n_iter"][f["best"]]), "empty_" + s: f["empty"],
                    "best_" + s: f["best"]})
    for t in names:
        shape = tuple(tables[t].shape)
        res[t] = np.rint(host[o:o + shape[0] * shape[1]]).astype(np.int64).reshape(shape)
        o += shape[0] * shape[1]
    for s, _ in blocks:
        if cls is not None:
            res["acc_" + s] = accuracy_from_counts(res["table_" + s], N)
            res["nmi_" + s] = nmi(res["table_" + s])
    if Ll:
        res["nmi_gl"] = nmi(res["table_gl"])
    return res


def _block(res, s, first):
    line = ''
    if res["labelled"]:
        line += 'acc {:.4f}, NMI {:.4f}, '.format(res["acc_" + s], res["nmi_" + s])
    line += 'inertia/image {:.4f}'.format(res["inertia_" + s])
    if first:
        line += ' ({} iterations, {} empty)'.format(res["n_iter_" + s], res["empty_" + s])
    return line


def report_line(res):
    line = REPORT.format(res["k"], res["n_images"], res["restarts"]) + _block(res, "g", True)
    if res.get("inertia_l") is not None:
        line += '; z_l ' + _block(res, "l", False) + '; NMI(z_g clusters; z_l clusters) {:.4f}'.format(res["nmi_gl"])
    return line


def check_flags(clusters, images, restarts, iters, global_latent_dims=1, local_latent_dims=0):
    """--clusters / --cluster_images / --cluster_restarts / --cluster_iters, before any data or device work."""
    if clusters < 2 or clusters > KMEANS_MAX_K:
        raise SystemExit("--clusters K: 2 <= K <= %d clusters, got %d" % (KMEANS_MAX_K, clusters))
    if images is not None and (images < clusters or images > KMEANS_MAX_N):
        raise SystemExit("--cluster_images N: at least K = %d and at most %d test images, got %d" % (clusters, KMEANS_MAX_N, images))
    if restarts < 1 or restarts > KMEANS_MAX_R:
        raise SystemExit("--cluster_restarts R: 1 <= R <= %d restarts, got %d" % (KMEANS_MAX_R, restarts))
    if iters < 0:
        raise SystemExit("--cluster_iters T: T >= 0 updates per restart, got %d" % iters)
    if not (1 <= global_latent_dims <= KMEANS_MAX_L and 0 <= local_latent_dims <= KMEANS_MAX_L):
        raise SystemExit("the k-means report covers latent blocks of at most %d dimensions" % KMEANS_MAX_L)


def build_parser():
    from .main import build_parser as build_main_parser
    ap = build_main_parser()                           # a fresh parser object: main's and evaluate's stay as they are
    ap.description = "k-means cluster report of the latent means of a saved weights file"
    ap.add_argument("--weights", type=str, required=True, help="file written by save_weights (.h5 / .hdf5 / .keras, else .npz)")
    ap.add_argument("--clusters", type=int, required=True, help="K: the number of clusters, 2 <= K <= %d" % KMEANS_MAX_K)
    ap.add_argument("--cluster_images", type=int, default=None, help="the report covers the first N test images (default: all)")
    ap.add_argument("--cluster_restarts", type=int, default=8, help="independent k-means++ restarts, 1 .. %d; the lowest inertia is reported" % KMEANS_MAX_R)
    ap.add_argument("--cluster_iters", type=int, default=100, help="at most T updates per restart")
    return ap


def main(argv=None):
    from . import reports
    args = build_parser().parse_args(argv)
    check_flags(args.clusters, args.cluster_images, args.cluster_restarts, args.cluster_iters, args.global_latent_dims,
                args.local_latent_dims if args.model != 'gmvae' else 0)               # before any data or device work
    if reports.any_on(args):
        on = [e.name for e in reports.TABLE if getattr(args, e.name) != 0]
        raise SystemExit("split_vae_amd.cluster runs the k-means report only: --%s belongs to python -m split_vae_amd.evaluate" % ", --".join(on))
    if args.model not in ('lgvae', 'lggmvae', 'gmvae'):
        raise SystemExit("--model %s: expected lgvae, lggmvae or gmvae" % args.model)
    from .main import check_augmentation, make_augmentors, make_model
    from .utils import dotdict
    config = dotdict(vars(args))
    check_augmentation(config.augmentation, args.model)
    from . import configure_hw_queues
    configure_hw_queues()                              # before the first HIP call (split_vae_amd/__init__.py)
    config.label = not config.no_label
    from . import data
    _, test_augmentor = make_augmentors(config)
    train_ds, test_ds, input_shape = data.get_dataset(config.dataset, config.batch_size, synthetic=config.synthetic,
                                                      data_dir=config.data_dir, get_label=config.label)
    if config.label and not train_ds.labelled:
        config.label = False
    if not config.label:
        print(UNLABELLED)
    if config.label:
        test_batches = [(test_augmentor.augment(x), y) for x, y in test_ds]      # the test batches of main(): the augmentor's first calls
    else:
        test_batches = [test_augmentor.augment(x) for x in test_ds]
    model, _ = make_model(args.model, config, input_shape)
    model.load_weights(args.weights)
    n = KMEANS_MAX_N if args.cluster_images is None else args.cluster_images
    res = evaluate(model, test_batches, n, args.clusters, args.cluster_restarts, args.cluster_iters)
    if res["n_images"] < n and args.cluster_images is not None:
        print(CLIPPED.format(n, res["n_images"]))
    print(report_line(res))
    return {("kmeans_" + key): val for key, val in res.items() if not key.startswith("table_")}


if __name__ == "__main__":
    main()
