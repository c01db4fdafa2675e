"""Linear label probe of the global and local latents: are the labels linearly decodable from z_g and not from z_l?

No reference counterpart.  The k-NN probe (probe.py) asks whether images of one class sit next to each other in a latent block; the
linear probe is the figure the representation-learning literature reports beside it: a softmax-regression classifier fitted on
the frozen latent means of a labelled reference set, and its accuracy on the test set, separately for z_g (the encoder of x) and
z_l (the encoder of the scrambled x_hat).  The fit is sv_linprobe_* (include/splitvae.h): Boehning's fixed-Hessian step
W <- W - B^-1 G with B = A^T A / (2 N) + diag(l2 .. l2, 0), A = [x 1] -- no step size, never an increase of the objective.  The
device computes the Gram matrix, the host inverts B once in float64, and all iterations then run on the device.  Convergence of
the weights is slow on nearly separable data with a small l2, so the report prints the final loss and the largest gradient entry
beside the accuracies.  lgvae and lggmvae report both latents, gmvae z_g only.

    python -m split_vae_amd.linear_probe --weights models/20260101-120000.h5 --dataset svhn
    python -m split_vae_amd.linear_probe --weights models/20260101-120000.h5 --probe_refs 73257 --probe_iters 200 --probe_l2 1e-4

The command takes the flags of split_vae_amd.main plus --weights, --probe_refs, --probe_iters, --probe_l2.  It is an entry point
of its own: reports.TABLE and the parsers of main / evaluate do not know it.
"""
import math

import numpy as np
import torch

from . import ops
from ._lib import LINPROBE_MAX_C, LINPROBE_MAX_L, LINPROBE_MAX_N

REPORT = 'Test linear probe ({} refs, {} steps, l2 {:g}): z_g '
BLOCK = 'acc {:.4f}, train acc {:.4f}, loss {:.4f} (|grad| {:.2e})'
NO_LABELS = 'Note: the linear probe needs labels; skipped'
CLIPPED = 'Note: --probe_refs {} clipped to the training set\'s {} images'


def step_matrix(S, n, l2):
    """P = B^-1 in float64 for B = S / (2 n) + diag(l2 .. l2, 0), S = A^T A the [(L+1),(L+1)] Gram matrix of A = [x 1].  Raises
    ValueError when B is not positive definite (a constant feature column with l2 = 0, say)."""
    S = np.asarray(S, np.float64)
    B = S / (2.0 * n)
    d = np.full(B.shape[0], float(l2))
    d[-1] = 0.0
    B = B + np.diag(d)
    try:
        pivots = np.diag(np.linalg.cholesky(B)) ** 2
        if pivots.min() <= 1e-12 * np.diag(B).max():                # positive only by its rounding
            raise np.linalg.LinAlgError("pivot")
        return np.linalg.inv(B)
    except np.linalg.LinAlgError:
        raise ValueError("linear_probe: A^T A / (2 N) + l2 I is not positive definite (a constant or duplicated feature column "
                         "with l2 = %g?): raise --probe_l2" % l2) from None


def fit(x, y, n_class, iters=100, l2=1e-3):
    """Softmax regression of the class ids y [N] uint8 on the rows of x [N,L] (fp32 device tensors) from W = 0: the Gram matrix on the
    device, one read-back, B^-1 on the host, `iters` steps on the device, one read-back of the trajectories.
    -> dict(W [(L+1),C] fp64 device tensor (row L is the bias), loss, gmax: float64 arrays [iters + 1], n, iters, l2)"""
    N, L = x.shape
    with ops.hold_stream():
        ws = torch.empty((ops.linprobe_workspace_bytes(N, L, n_class),), dtype=torch.uint8, device=x.device)
        S = ops.linprobe_gram(x, workspace=ws).cpu().numpy()                      # read-back 1
        P = torch.from_numpy(step_matrix(S, N, l2)).to(x.device)
        f = ops.linprobe_fit(x, y, P, ops.linprobe_state(x, n_class, iters), iters, l2, workspace=ws)
        traj = torch.stack([f["loss"], f["gmax"]]).cpu().numpy()                  # read-back 2
    return dict(W=f["W"], loss=traj[0], gmax=traj[1], n=int(N), iters=int(iters), l2=float(l2))


def evaluate(model, ref_batches, test_batches, iters=100, l2=1e-3):
    """The report: per latent block a fit on the reference latent means and its accuracy / mean cross-entropy on the test latent means.
    Batches are (images6, one-hot labels) pairs.  -> dict(per block s in (g, l): acc_s (test), train_acc_s, loss_s (the last loss of
    the fit, penalty included), test_loss_s, gmax_s; n_ref, n_test, iters, l2).  The l entries are None for GMVae."""
    from .probe import _class_ids, latent_means
    ref_batches, test_batches = list(ref_batches), list(test_batches)
    rg, rl = latent_means(model, ref_batches)
    tg, tl = latent_means(model, test_batches)
    rc, n_class = _class_ids(ref_batches)
    tc, _ = _class_ids(test_batches)
    n_class = max(n_class, 2)
    if n_class > LINPROBE_MAX_C:
        raise ValueError("linear_probe.evaluate: at most %d classes, got %d" % (LINPROBE_MAX_C, n_class))
    res = dict(n_ref=int(rg.shape[0]), n_test=int(tg.shape[0]), iters=int(iters), l2=float(l2))
    for s, r, t in (("g", rg, tg), ("l", rl, tl)):
        if r is None:
            res.update({k + s: None for k in ("acc_", "train_acc_", "loss_", "test_loss_", "gmax_")})
            continue
        f = fit(r, rc, n_class, iters, l2)
        acc = torch.zeros((2, 2), dtype=torch.int64, device=r.device)
        with ops.hold_stream():
            ops.linprobe_predict(r, f["W"], q_class=rc, acc=acc[0])
            pred, tloss = ops.linprobe_predict(t, f["W"], q_class=tc, acc=acc[1], want_loss=True)
            host = torch.cat([acc.reshape(-1).double(), tloss]).cpu().tolist()     # one read-back
        res.update({"acc_" + s: host[2] / host[3], "train_acc_" + s: host[0] / host[1], "loss_" + s: float(f["loss"][-1]),
                    "test_loss_" + s: host[4], "gmax_" + s: float(f["gmax"][-1]), "pred_" + s: pred, "hits_" + s: int(host[2])})
    return res


def report_line(res):
    line = REPORT.format(res["n_ref"], res["iters"], res["l2"]) + BLOCK.format(res["acc_g"], res["train_acc_g"], res["loss_g"], res["gmax_g"])
    if res.get("acc_l") is not None:
        line += '; z_l ' + BLOCK.format(res["acc_l"], res["train_acc_l"], res["loss_l"], res["gmax_l"])
    return line


def check_flags(refs, iters, l2, no_label, global_latent_dims=1, local_latent_dims=0):
    """--probe_refs / --probe_iters / --probe_l2, before any data or device work."""
    if no_label:
        raise SystemExit("split_vae_amd.linear_probe fits a classifier of the labels: it cannot run with -no_label")
    if refs < 1 or refs > LINPROBE_MAX_N:
        raise SystemExit("--probe_refs N: 1 <= N <= %d reference images, got %d" % (LINPROBE_MAX_N, refs))
    if iters < 0:
        raise SystemExit("--probe_iters T: T >= 0 steps, got %d" % iters)
    if not (l2 >= 0 and math.isfinite(l2)):
        raise SystemExit("--probe_l2: a finite penalty >= 0, got %r" % l2)
    if not (1 <= global_latent_dims <= LINPROBE_MAX_L and 0 <= local_latent_dims <= LINPROBE_MAX_L):
        raise SystemExit("the linear probe covers latent blocks of at most %d dimensions" % LINPROBE_MAX_L)


def build_parser():
    from .main import build_parser as build_main_parser
    ap = build_main_parser()                           # a fresh parser object: main's and evaluate's stay as they are
    ap.description = "linear label probe of the latent means of a saved weights file"
    ap.add_argument("--weights", type=str, required=True, help="file written by save_weights (.h5 / .hdf5 / .keras, else .npz)")
    ap.add_argument("--probe_refs", type=int, default=20000, help="the classifier is fitted on the first N training images in file order")
    ap.add_argument("--probe_iters", type=int, default=100, help="T: the number of fixed-Hessian steps of the fit")
    ap.add_argument("--probe_l2", type=float, default=1e-3, help="the l2 penalty on the weights (not on the bias)")
    return ap


def main(argv=None):
    from . import reports
    args = build_parser().parse_args(argv)
    check_flags(args.probe_refs, args.probe_iters, args.probe_l2, args.no_label, args.global_latent_dims,
                args.local_latent_dims if args.model != 'gmvae' else 0)               # before any data or device work
    if reports.any_on(args):
        on = [e.name for e in reports.TABLE if getattr(args, e.name) != 0]
        raise SystemExit("split_vae_amd.linear_probe runs the linear probe only: --%s belongs to python -m split_vae_amd.evaluate" % ", --".join(on))
    if args.model not in ('lgvae', 'lggmvae', 'gmvae'):
        raise SystemExit("--model %s: expected lgvae, lggmvae or gmvae" % args.model)
    from .main import check_augmentation, make_augmentors, make_model
    from .utils import dotdict
    config = dotdict(vars(args))
    check_augmentation(config.augmentation, args.model)
    from . import configure_hw_queues
    configure_hw_queues()                              # before the first HIP call (split_vae_amd/__init__.py)
    config.label = True
    from . import data, probe
    from .augmentation import ReferenceAugmentator
    _, test_augmentor = make_augmentors(config)
    train_ds, test_ds, input_shape = data.get_dataset(config.dataset, config.batch_size, synthetic=config.synthetic,
                                                      data_dir=config.data_dir, get_label=True)
    if not train_ds.labelled:
        print(NO_LABELS)
        return {}
    test_batches = [(test_augmentor.augment(x), y) for x, y in test_ds]          # the test batches of main(): the augmentor's first calls
    model, _ = make_model(args.model, config, input_shape)
    model.load_weights(args.weights)
    n_train = train_ds.N if hasattr(train_ds, "N") else train_ds.x.shape[0]
    n = int(args.probe_refs)
    if n > n_train:
        print(CLIPPED.format(n, n_train))
        n = n_train
    aug = ReferenceAugmentator(type=config.augmentation, size=config.patch_size, seed=config.seed,
                               per_image=bool(config.get("mix_per_image")), pipeline=1)
    res = evaluate(model, probe.reference_batches(train_ds, n, aug, config.batch_size), test_batches, args.probe_iters, args.probe_l2)
    print(report_line(res))
    return {("linprobe_" + key): val for key, val in res.items() if not key.startswith("pred_")}


if __name__ == "__main__":
    main()
