"""Exact t-SNE map of the global and local latents: the 2-D picture of the latent means coloured by class -- digits separate in z_g
and do not in z_l -- with two numbers that state what it shows.

No reference counterpart.  The map is van der Maaten & Hinton's exact O(N^2) t-SNE (sv_tsne_*, include/splitvae.h: conditional
affinities by a fixed-length bisection on the perplexity, the symmetrised P, early exaggeration, the delta-bar-delta update), one fit
per latent block on the device.  The figures: the KL divergence the fit ends at; neighbours kept@k, the share of each image's k
nearest latent neighbours that are among its k nearest map neighbours; and the leave-one-out k-NN accuracy in the map beside the
same in the latent (labelled sets only).  lgvae and lggmvae report both latents, gmvae z_g only.

    python -m split_vae_amd.tsne --weights models/20260101-120000.h5 --dataset svhn --tsne_images 10000 --tsne_out maps
    python -m split_vae_amd.tsne --weights models/20260101-120000.h5 --dataset celeba64 -no_label --tsne_images 5000

The command takes the flags of split_vae_amd.main plus --weights, --tsne_images, --perplexity, --tsne_iters, --tsne_exaggeration,
--tsne_exag_iters, --tsne_lr, --tsne_k, --tsne_out, --tsne_canvas.  With --tsne_out DIR it writes tsne_z_g.png, tsne_z_l.png (a NumPy
rasteriser: white square canvas, one disc per image in a fixed palette indexed by class, drawn in index order) and tsne.npz (Y_g, Y_l,
labels, kl_g, kl_l, beta_g, beta_l).  It is an entry point of its own: reports.TABLE and the parsers of main / evaluate do not know it.
"""
import os

import numpy as np
import torch

from . import ops
from ._lib import TSNE_MAX_K, TSNE_MAX_L, TSNE_MAX_N, TSNE_MIN_N

REPORT = 'Test t-SNE map ({} images, perplexity {:g}, {} iterations): z_g '
UNLABELLED = 'Note: no labels: the t-SNE report prints the label-free figures only'
CLIPPED = 'Note: --tsne_images {} clipped to the test set\'s {} images'
MAX_CLASSES = 64                                   # sv_knn_classify's vote
PALETTE = np.array([[31, 119, 180], [255, 127, 14], [44, 160, 44], [214, 39, 40], [148, 103, 189], [140, 86, 75], [227, 119, 194],
                    [127, 127, 127], [188, 189, 34], [23, 190, 207]], np.float64) / 255.0      # indexed by class % 10
ONE_COLOUR = np.array([31, 119, 180], np.float64) / 255.0


def auto_lr(n, exaggeration):
    return max(n / exaggeration / 4.0, 50.0)


def fit_enqueue(x, perplexity, iters, seed, exaggeration=12.0, exag_iters=250, lr=None):
    """The device half of fit(): affinities, the initial map, `iters` iterations; nothing is read back."""
    N = x.shape[0]
    lr = auto_lr(N, exaggeration) if lr is None else lr
    with ops.hold_stream():
        ws = torch.empty((ops.tsne_workspace_bytes(N),), dtype=torch.uint8, device=x.device)
        aff = ops.tsne_affinities(x, perplexity, workspace=ws)
        st = ops.tsne_init(ops.tsne_state(N, iters, device=x.device), seed)
        ops.tsne_iterate(aff, st, iters, exaggeration, exag_iters, lr, workspace=ws)
    return dict(Y=st["Y"], inc=st["inc"], gain=st["gain"], state=st["state"], kl=st["kl"], beta=aff["beta"], row_entropy=aff["row_entropy"],
                P=aff["P"], p_const=aff["p_const"], lr=float(lr))


def fit(x, perplexity=30.0, iters=1000, seed=0, exaggeration=12.0, exag_iters=250, lr=None):
    """The t-SNE map of the rows of x [N,L] (fp32 device tensor; a row pitch above L is allowed) -> dict(Y [N,2], beta [N], kl [iters]
    (kl[t]: the KL divergence of the map iteration t started from), ...: device tensors; kl_trace: the same trace on the host)."""
    f = fit_enqueue(x, perplexity, iters, seed, exaggeration, exag_iters, lr)
    f["kl_trace"] = f["kl"].cpu().numpy()
    return f


def neighbour_counts(x, Y, k, cls=None, n_class=0):
    """[3] int64 on the device: sv_tsne_neighbour_scores of the (k + 1)-neighbour lists of the latent rows x and the map rows Y"""
    N = x.shape[0]
    dummy = torch.zeros((N,), dtype=torch.uint8, device=x.device) if cls is None else cls
    nc = max(2, int(n_class))
    with ops.hold_stream():
        ws = torch.empty((ops.knn_workspace_bytes(N, N, k + 1),), dtype=torch.uint8, device=x.device)
        _, nn_lat, _ = ops.knn_classify(x, x, dummy, k + 1, nc, want_neighbours=True, workspace=ws)
        _, nn_map, _ = ops.knn_classify(Y, Y, dummy, k + 1, nc, want_neighbours=True, workspace=ws)
        return ops.tsne_neighbour_scores(nn_lat, nn_map, cls, nc)


def _labels(batches, n):
    """uint8 class ids [n] on the device and the number of classes when the batches are (images, one-hot labels) pairs, else (None, 0)"""
    ys, have = [], 0
    for b in batches:
        if have >= n:
            break
        if not isinstance(b, (tuple, list)) or len(b) < 2 or b[1] is None:
            return None, 0
        ys.append(b[1])
        have += b[1].shape[0]
    return torch.cat([y.argmax(dim=1) for y in ys])[:n].to(torch.uint8).contiguous(), int(ys[0].shape[1])


def evaluate(model, test_batches, n, perplexity=30.0, iters=1000, exaggeration=12.0, exag_iters=250, lr=None, k=10, seed=None):
    """The report over the latent means of the first `n` test images (all when there are fewer): one fit per latent block.
    -> dict(n_images, perplexity, iters, k, labelled; per block s in (g, l): kl_s (the KL of the last map an iteration started from),
    kept_s (neighbours kept@k), map_acc_s, latent_acc_s (None without labels), Y_s [N,2], kl_trace_s [iters], beta_s [N]: host arrays;
    labels [N] uint8 or None).  The l entries are None for GMVae.  seed: model.seed.  One read-back of the figures per block and one
    of the coordinates."""
    from .latent_info import posteriors
    test_batches = list(test_batches)
    mu, _, Lg, Ll = posteriors(model, test_batches, int(n))
    N = int(mu.shape[0])
    if N < TSNE_MIN_N or not 1.0 < perplexity < N - 1 or k + 1 > N:
        raise ValueError("tsne.evaluate: %d images do not allow perplexity %g and k = %d" % (N, perplexity, k))
    seed = model.seed if seed is None else seed
    cls, C = _labels(test_batches, N)
    if cls is not None and C > MAX_CLASSES:
        raise ValueError("tsne.evaluate: at most %d classes, got %d" % (MAX_CLASSES, C))
    res = dict(n_images=N, perplexity=float(perplexity), iters=int(iters), k=int(k), labelled=cls is not None,
               labels=None if cls is None else cls.cpu().numpy())
    for s in ("g", "l"):
        res.update({key + s: None for key in ("kl_", "kept_", "map_acc_", "latent_acc_", "Y_", "kl_trace_", "beta_")})
    for s, z in [("g", mu[:, :Lg])] + ([("l", mu[:, Lg:])] if Ll else []):
        f = fit_enqueue(z, perplexity, iters, seed, exaggeration, exag_iters, lr)
        counts = neighbour_counts(z, f["Y"], k, cls, C)
        figs = torch.cat([f["kl"], counts.double()]).cpu().numpy()                  # the figures' read-back
        coords = torch.cat([f["Y"].reshape(-1).double(), f["beta"]]).cpu().numpy()   # the coordinates' read-back
        T = f["kl"].numel()
        trace, cnt = figs[:T][:iters], figs[T:]
        res.update({"kl_trace_" + s: trace, "kl_" + s: float(trace[-1]) if iters > 0 else float("nan"), "kept_" + s: float(cnt[0]) / (k * N),
                    "Y_" + s: coords[:2 * N].reshape(N, 2).astype(np.float32), "beta_" + s: coords[2 * N:].copy()})
        if cls is not None:
            res.update({"map_acc_" + s: float(cnt[1]) / N, "latent_acc_" + s: float(cnt[2]) / N})
    return res


def _block(res, s):
    line = 'KL {:.4f}, neighbours kept@{} {:.4f}'.format(res["kl_" + s], res["k"], res["kept_" + s])
    if res["labelled"]:
        line += ', map k-NN acc {:.4f} (latent {:.4f})'.format(res["map_acc_" + s], res["latent_acc_" + s])
    return line


def report_line(res):
    line = REPORT.format(res["n_images"], res["perplexity"], res["iters"]) + _block(res, "g")
    if res.get("kl_l") is not None:
        line += '; z_l ' + _block(res, "l")
    return line


# ---------------------------------------------------------------- the picture
def rasterise(Y, labels=None, size=512, radius=2, margin=0.05):
    """[size, size, 3] float canvas of the map Y [N,2]: white, the map's bounding box (one scale for both axes, centred) inside a margin of
    `margin` of the canvas on every side; point i is a disc of `radius` pixels around its pixel in PALETTE[labels[i] % 10] (ONE_COLOUR
    without labels); points are drawn in index order, so a later point covers an earlier one and the canvas is a function of (Y, labels)
    alone.  y grows upwards.  pixel_of(Y, size, margin) gives the centres."""
    canvas = np.ones((size, size, 3), np.float64)
    px = pixel_of(Y, size, margin)
    dy, dx = np.mgrid[-radius:radius + 1, -radius:radius + 1]
    disc = dx * dx + dy * dy <= radius * radius
    oy, ox = dy[disc], dx[disc]
    for i in range(px.shape[0]):
        colour = ONE_COLOUR if labels is None else PALETTE[int(labels[i]) % len(PALETTE)]
        r, c = px[i, 1] + oy, px[i, 0] + ox
        ok = (r >= 0) & (r < size) & (c >= 0) & (c < size)
        canvas[r[ok], c[ok]] = colour
    return canvas


def pixel_of(Y, size=512, margin=0.05):
    """[N,2] int (column, row) of every point's centre"""
    Y = np.asarray(Y, np.float64)
    lo, hi = Y.min(axis=0), Y.max(axis=0)
    span = float(max((hi - lo).max(), 1e-30))
    inner = (size - 1) * (1.0 - 2.0 * margin)
    u = (Y - 0.5 * (lo + hi)[None, :]) / span * inner + 0.5 * (size - 1)
    col = np.rint(u[:, 0]).astype(np.int64)
    row = np.rint((size - 1) - u[:, 1]).astype(np.int64)
    return np.stack([col, row], axis=1)


def save_outputs(res, out_dir, size=512):
    """tsne_z_g.png, tsne_z_l.png and tsne.npz under out_dir -> the paths written"""
    from .visualizer import save_png
    os.makedirs(out_dir, exist_ok=True)
    paths = []
    for s in ("g", "l"):
        if res.get("Y_" + s) is not None:
            path = os.path.join(out_dir, "tsne_z_%s.png" % s)
            save_png(path, rasterise(res["Y_" + s], res["labels"], size))
            paths.append(path)
    N = res["n_images"]
    empty2, empty1 = np.zeros((0, 2), np.float32), np.zeros((0,), np.float64)
    pick = lambda key, empty: empty if res.get(key) is None else res[key]      # noqa: E731
    path = os.path.join(out_dir, "tsne.npz")
    np.savez(path, Y_g=pick("Y_g", empty2), Y_l=pick("Y_l", empty2), labels=np.full((N,), -1, np.int32) if res["labels"] is None else res["labels"].astype(np.int32),
             kl_g=pick("kl_trace_g", empty1), kl_l=pick("kl_trace_l", empty1), beta_g=pick("beta_g", empty1), beta_l=pick("beta_l", empty1))
    return paths + [path]


# ---------------------------------------------------------------- the command line
def parse_lr(text):
    if text == "auto":
        return None
    try:
        return float(text)
    except ValueError:
        raise SystemExit("--tsne_lr: 'auto' or a positive number, got %r" % text)


def check_flags(images, perplexity, iters, exaggeration, exag_iters, lr, k, global_latent_dims=1, local_latent_dims=0, canvas=512):
    """--tsne_images / --perplexity / --tsne_iters / --tsne_exaggeration / --tsne_exag_iters / --tsne_lr / --tsne_k / --tsne_canvas, before
    any data or device work."""
    if images is not None and (images < TSNE_MIN_N or images > TSNE_MAX_N):
        raise SystemExit("--tsne_images N: at least %d and at most %d test images (P is N x N floats), got %d" % (TSNE_MIN_N, TSNE_MAX_N, images))
    if not perplexity > 1.0 or (images is not None and not perplexity < images - 1):
        raise SystemExit("--perplexity P: 1 < P < N - 1, got %g" % perplexity)
    if iters < 0:
        raise SystemExit("--tsne_iters T: T >= 0 iterations, got %d" % iters)
    if not 1.0 <= exaggeration <= 1e6:
        raise SystemExit("--tsne_exaggeration E: 1 <= E <= 1e6, got %g" % exaggeration)
    if exag_iters < 0:
        raise SystemExit("--tsne_exag_iters: >= 0 iterations, got %d" % exag_iters)
    if lr is not None and not 0.0 < lr <= 1e9:
        raise SystemExit("--tsne_lr: 'auto' or 0 < lr <= 1e9, got %g" % lr)
    if k < 1 or k > TSNE_MAX_K or (images is not None and k + 1 > images):
        raise SystemExit("--tsne_k K: 1 <= K <= %d neighbours (and K < N), got %d" % (TSNE_MAX_K, k))
    if canvas < 16 or canvas > 4096:
        raise SystemExit("--tsne_canvas: 16 .. 4096 pixels, got %d" % canvas)
    if not (1 <= global_latent_dims <= TSNE_MAX_L and 0 <= local_latent_dims <= TSNE_MAX_L):
        raise SystemExit("the t-SNE report covers latent blocks of at most %d dimensions" % TSNE_MAX_L)


def build_parser():
    from .main import build_parser as build_main_parser
    ap = build_main_parser()                           # a fresh parser object: main's and evaluate's stay as they are
    ap.description = "exact t-SNE map of the latent means of a saved weights file"
    ap.add_argument("--weights", type=str, required=True, help="file written by save_weights (.h5 / .hdf5 / .keras, else .npz)")
    ap.add_argument("--tsne_images", type=int, default=None, help="the map covers the first N test images (default: all, at most %d)" % TSNE_MAX_N)
    ap.add_argument("--perplexity", type=float, default=30.0, help="the perplexity of the conditional affinities, 1 < P < N - 1")
    ap.add_argument("--tsne_iters", type=int, default=1000, help="T: gradient iterations")
    ap.add_argument("--tsne_exaggeration", type=float, default=12.0, help="early exaggeration of P")
    ap.add_argument("--tsne_exag_iters", type=int, default=250, help="iterations under early exaggeration (momentum 0.5, then 0.8)")
    ap.add_argument("--tsne_lr", type=str, default="auto", help="learning rate; auto: max(N / exaggeration / 4, 50)")
    ap.add_argument("--tsne_k", type=int, default=10, help="k of the neighbour scores, 1 .. %d" % TSNE_MAX_K)
    ap.add_argument("--tsne_out", type=str, default=None, help="directory for tsne_z_g.png, tsne_z_l.png and tsne.npz")
    ap.add_argument("--tsne_canvas", type=int, default=512, help="side of the square PNG canvas in pixels")
    return ap


def main(argv=None):
    from . import reports
    args = build_parser().parse_args(argv)
    lr = parse_lr(args.tsne_lr)
    check_flags(args.tsne_images, args.perplexity, args.tsne_iters, args.tsne_exaggeration, args.tsne_exag_iters, lr, args.tsne_k,
                args.global_latent_dims, args.local_latent_dims if args.model != 'gmvae' else 0, args.tsne_canvas)      # before any data or device work
    if reports.any_on(args):
        on = [e.name for e in reports.TABLE if getattr(args, e.name) != 0]
        raise SystemExit("split_vae_amd.tsne runs the t-SNE report only: --%s belongs to python -m split_vae_amd.evaluate" % ", --".join(on))
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
    n = TSNE_MAX_N if args.tsne_images is None else args.tsne_images
    res = evaluate(model, test_batches, n, args.perplexity, args.tsne_iters, args.tsne_exaggeration, args.tsne_exag_iters, lr, args.tsne_k)
    if res["n_images"] < n and args.tsne_images is not None:
        print(CLIPPED.format(n, res["n_images"]))
    print(report_line(res))
    if args.tsne_out:
        res["files"] = save_outputs(res, args.tsne_out, args.tsne_canvas)
    return {("tsne_" + key): val for key, val in res.items()}


if __name__ == "__main__":
    main()
