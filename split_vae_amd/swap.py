"""Swap-consistency report of the global and local latents: does decode(z_g of image A, z_l of image B) keep A's global content and
B's local content?

No reference counterpart.  The paper's Table 1 asks this with a classifier whose weights are missing upstream; the repository draws
the hybrid (visualizer.style_transfer_test) but puts no number on it.  This report answers with a cycle and no classifier: decode the
hybrid, turn the decode into the image it is (pixel levels, the data's own values), re-encode it, and rank all N test images by their
distance from the re-encoded latent block (sv_swap_pair / sv_swap_requantise / sv_swap_rank, include/splitvae.h).
In z_g space image A should come first and image B nowhere; in z_l space the roles reverse.  With labels the k-NN probe's references
give the class of the re-encoded z_g: it should follow A's label and not B's.

    python -m split_vae_amd.swap --weights models/20260101-120000.h5 --dataset svhn --swap_partners 2
    python -m split_vae_amd.swap --weights models/20260101-120000.h5 --dataset celeba64 -no_label --patch_size 8 --swap_out out/swap

Definitions:
  originals  mu [N, Lg+Ll]: the posterior means of the first N test images (latent_info.posteriors, keyed: the mixture models compute
             z_g's mean behind a relaxed categorical sample, and image i draws it as global sample i; every hybrid of image i's z_g is
             re-encoded under the same key, so neither the originals nor the cycle depend on the batch size)
  partners   for p = 1 .. P image i supplies z_g and image j = (i + s_p) mod N supplies z_l; the shifts s_p are distinct, in [1, N-1],
             drawn on the host from the Philox mirror keyed by (seed, a tag of this report's own, p) (sv_swap_shift_word_host)
  unswapped  a further pass with shift 0, the plain reconstruct-and-re-encode cycle, always runs: the ceiling of the swapped figures
  hybrid     zcat = [mu[i, :Lg] | mu[j, Lg:]]; the decoders; the mean requantised to pixel levels; its scramble by a permutation keyed by
             (seed, this report's step tag, the hybrid's global index = pass * N + i): it does not depend on the batch size
  ranks      rank of the source among the N originals by sv_knn_classify's distance from the re-encoded block (ties to the lower
             index, the source's own column excluded): kept = the block's own source, leak = the other one
  figures    kept@1 the share of hybrids with kept rank 0; kept@k with kept rank below k; MRR the mean of 1 / (kept rank + 1); leak@1
             the share whose nearest original is the OTHER source; cycle@1 = kept@1 of the unswapped pass.  Float64 on the host.
  classes    (labelled sets) the k-NN class of the re-encoded z_g among --swap_refs training latents; over the pairs whose two labels
             differ: the share that follows the z_g source's label, the share that follows the z_l source's, and the probe's accuracy on
             the unswapped pass

The command takes the flags of split_vae_amd.main plus --weights, --swap_images, --swap_partners, --swap_k, --swap_knn, --swap_refs,
--swap_out, --swap_grid.  It is an entry point of its own: reports.TABLE and the parsers of main / evaluate do not know it.
"""
import os

import numpy as np
import torch

from . import ops
from ._lib import KNN_MAX_K, PHASE_FWD_DECODERS, PHASE_PREP, SWAP_MAX_L
from .utils import images_of

REPORT = 'Test swap consistency ({} images, {} partners): '
BLOCK = 'kept@1 {:.4f}, kept@{} {:.4f}, MRR {:.4f}, leak@1 {:.4f} (cycle@1 {:.4f})'
CLASSES = '; class follows z_g source {:.4f}, z_l source {:.4f} ({} unlike pairs, k={}, {} refs; unswapped {:.4f})'
UNLABELLED = 'Note: no labels: the swap report prints the label-free figures only'
CLIPPED = 'Note: --swap_images {} clipped to the test set\'s {} images'
MAX_IMAGES = 65536                                 # the default of --swap_images: all test images, capped here
MAX_PARTNERS = 8
MAX_GRID = 32
MAX_CLASSES = 64                                   # sv_knn_classify's vote
PERM_STEP = 0x7377 << 40                           # 'sw': the `step` key of the hybrids' permutations (augmentation.py keeps 0, 1 << 40, 2 << 40)


def partner_shifts(seed, n, partners):
    """The P distinct shifts in [1, n-1]: partner p takes 1 + word(seed, p, attempt) mod (n - 1) at the first attempt that gives a
    shift no earlier partner has."""
    if not 1 <= partners <= min(MAX_PARTNERS, n - 1):
        raise ValueError("swap: 1 <= partners <= min(%d, N - 1 = %d), got %d" % (MAX_PARTNERS, n - 1, partners))
    out = []
    for p in range(1, partners + 1):
        for attempt in range(1 << 16):
            s = 1 + ops.swap_shift_word_host(seed, p, attempt) % (n - 1)
            if s not in out:
                break
        else:
            raise RuntimeError("swap: no free shift for partner %d" % p)
        out.append(int(s))
    return out


def _check_shifts(shifts, n):
    shifts = [int(s) for s in shifts]
    if not shifts or len(shifts) > MAX_PARTNERS or len(set(shifts)) != len(shifts) or min(shifts) < 1 or max(shifts) > n - 1:
        raise ValueError("swap: 1 .. %d distinct shifts in [1, N - 1 = %d], got %r" % (MAX_PARTNERS, n - 1, shifts))
    return shifts


def figures(ranks, k):
    """ranks [P+1, N, 2] integers of one block (pass 0 unswapped; [..., 0] kept, [..., 1] leak) -> dict(kept1, keptk, mrr, leak1, cycle1)."""
    r = np.asarray(ranks, np.int64)
    kept, leak = r[1:, :, 0].reshape(-1), r[1:, :, 1].reshape(-1)
    return dict(kept1=float(np.mean((kept == 0).astype(np.float64))), keptk=float(np.mean((kept < k).astype(np.float64))),
                mrr=float(np.mean(1.0 / (kept.astype(np.float64) + 1.0))), leak1=float(np.mean((leak == 0).astype(np.float64))),
                cycle1=float(np.mean((r[0, :, 0] == 0).astype(np.float64))))


def class_figures(pred, labels, shifts):
    """pred [P+1, N] class ids of the re-encoded z_g (pass 0 unswapped), labels [N] -> dict(follows_g, follows_l (None without an unlike
    pair), unlike_pairs, unswapped_acc)."""
    pred, labels = np.asarray(pred, np.int64), np.asarray(labels, np.int64)
    n = labels.shape[0]
    fg = fl = m = 0
    for p, s in enumerate(shifts):
        lj = labels[(np.arange(n) + s) % n]
        unlike = lj != labels
        m += int(unlike.sum())
        fg += int((pred[p + 1][unlike] == labels[unlike]).sum())
        fl += int((pred[p + 1][unlike] == lj[unlike]).sum())
    return dict(follows_g=fg / m if m else None, follows_l=fl / m if m else None, unlike_pairs=m,
                unswapped_acc=float(np.mean((pred[0] == labels).astype(np.float64))))


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


def reference_means(model, ref_batches, Lg):
    """z_g means [R, Lg] of the reference batches, reference r under the noise key of global sample r (the mixture models): they do not
    depend on the batch size either"""
    from .latent_info import posteriors
    return posteriors(model, ref_batches, None, keyed=True)[0][:, :Lg]


class _Cycle:
    """The buffers of one model and batch size: hybrids in, requantised six-channel batches and re-encoded means out."""

    def __init__(self, model, mu, Lg, B, H, W, patch, seed):
        from .data import ResidentDataset
        self.model, self.mu, self.Lg, self.B, self.patch, self.seed = model, mu, Lg, B, patch, seed
        dev, Lc = mu.device, int(mu.shape[1])
        self.N = int(mu.shape[0])
        self.plan = model.plan(B)
        self.zcat = self.plan.buffer("zcat", model.dtype, (B, Lc))
        self.out6 = self.plan.buffer("out6_x", torch.float32, (B, H, W, 6))
        self.images6 = torch.empty((B, H, W, 6), dtype=torch.float32, device=dev)
        self.perm = torch.empty((B, (H // patch) * (W // patch)), dtype=torch.int32, device=dev)
        self.lut = torch.from_numpy(ResidentDataset.make_lut()).to(dev)

    def hybrids(self, ig, il, offset):
        """ig, il [B] int32 device indices -> self.images6: decode([mu[ig, :Lg] | mu[il, Lg:]]) as the image it is, beside its scramble."""
        with ops.hold_stream():
            ops.swap_pair(self.mu, ig, il, self.Lg, self.zcat, check_range=False)
            self.plan.step(PHASE_PREP | PHASE_FWD_DECODERS, params=self.model.flat)
            ops.random_perm(self.B, self.perm.shape[1], self.seed, PERM_STEP, offset, out=self.perm)
            ops.swap_requantise(self.out6, self.lut, self.perm, self.patch, out=self.images6)
        return self.images6

    def batches(self, shift, offset):
        """(first row o, rows taken, ig, il) per batch of the pass with this shift; a short last batch repeats image N - 1"""
        for o in range(0, self.N, self.B):
            idx = torch.arange(o, o + self.B, dtype=torch.int64, device=self.mu.device).clamp_(max=self.N - 1)
            yield o, min(self.B, self.N - o), idx.to(torch.int32), ((idx + shift) % self.N).to(torch.int32), offset + o


def evaluate(model, test_batches, n, partners=1, k=10, seed=None, shifts=None, patch=1, knn=0, ref_batches=None, keep=False):
    """The report over the first `n` test images (all when there are fewer).  shifts pins the partners' shifts (tests); seed: model.seed.
    patch: the scramble's patch size (--patch_size).  knn > 0 with labelled test batches and ref_batches ((images6, one-hot) pairs, e.g.
    probe.reference_batches): the class figures.  keep: res["hybrids"] [P+1, N, H, W, 6] keeps every requantised batch (tests).
    -> dict(n_images, partners, k, shifts, labelled; per block s in (g, l): kept1_s, keptk_s, mrr_s, leak1_s, cycle1_s; ranks_g, ranks_l
    [P+1, N, 2] int64 arrays (pass 0 unswapped; kept, leak); labels [N] or None; follows_g, follows_l, unlike_pairs, unswapped_acc, knn,
    n_ref (None without labels); Q [P+1, N, Lg+Ll] and mu [N, Lg+Ll] device tensors).  One read-back.  Leaves model._calls alone."""
    from .gmvae import GMVae
    from .latent_info import batch_posterior, posteriors
    if isinstance(model, GMVae):
        raise ValueError("swap.evaluate: gmvae has one latent block; nothing to swap")
    if int(n) < 2:
        raise ValueError("swap.evaluate needs n >= 2 images, got %r" % (n,))
    test_batches = list(test_batches)
    mu, _, Lg, Ll = posteriors(model, test_batches, int(n), keyed=True)
    N, Lc = int(mu.shape[0]), Lg + Ll
    if N < 2 or not Ll:
        raise ValueError("swap.evaluate needs at least 2 test images and two latent blocks, got %d images, Ll = %d" % (N, Ll))
    seed = model.seed if seed is None else seed
    shifts = partner_shifts(seed, N, int(partners)) if shifts is None else _check_shifts(shifts, N)
    first = images_of(test_batches[0])
    B, H, W = (int(v) for v in first.shape[:3])
    dev = mu.device
    cyc = _Cycle(model, mu, Lg, B, H, W, int(patch), seed)
    passes = [0] + shifts
    Q = torch.empty((len(passes), N, Lc), dtype=torch.float32, device=dev)
    kept = torch.empty((len(passes), N, H, W, 6), dtype=torch.float32, device=dev) if keep else None
    for pi, s in enumerate(passes):
        for o, take, ig, il, offset in cyc.batches(s, pi * N):
            images6 = cyc.hybrids(ig, il, offset)
            mg, _, ml, _ = batch_posterior(model, images6, o)      # hybrid (pass, i) under the noise key of original i
            Q[pi, o:o + take, :Lg] = mg[:take]
            Q[pi, o:o + take, Lg:] = ml[:take]
            if keep:
                kept[pi, o:o + take] = images6[:take]
    ar = torch.arange(N, dtype=torch.int64, device=dev)
    ti = ar.to(torch.int32)
    ranks = torch.empty((len(passes), 2, N, 2), dtype=torch.int32, device=dev)
    cls, C = _labels(test_batches, N)
    labelled = bool(knn) and cls is not None and ref_batches is not None and len(ref_batches) > 0
    pred, n_ref = [], None
    with ops.hold_stream():
        ws = torch.empty((ops.swap_rank_workspace_bytes(N, N, max(Lg, Ll)),), dtype=torch.uint8, device=dev)
        for pi, s in enumerate(passes):
            tj = ((ar + s) % N).to(torch.int32)
            ops.swap_rank(Q[pi][:, :Lg], mu[:, :Lg], ti, tj, rank=ranks[pi, 0], workspace=ws, check_range=False)
            ops.swap_rank(Q[pi][:, Lg:], mu[:, Lg:], tj, ti, rank=ranks[pi, 1], workspace=ws, check_range=False)
    if labelled:
        from .probe import _class_ids
        if C > MAX_CLASSES:
            raise ValueError("swap.evaluate: at most %d classes, got %d" % (MAX_CLASSES, C))
        rg = reference_means(model, ref_batches, Lg)
        rc, _ = _class_ids(ref_batches)
        n_ref = int(rg.shape[0])
        with ops.hold_stream():
            pred = [ops.knn_classify(Q[pi][:, :Lg], rg, rc, int(knn), max(C, 2)) for pi in range(len(passes))]
    host = torch.cat([ranks.reshape(-1)] + pred + ([cls.to(torch.int32)] if cls is not None else [])).cpu().numpy()      # the one read-back
    nr = ranks.numel()
    hr = host[:nr].astype(np.int64).reshape(len(passes), 2, N, 2)
    res = dict(n_images=N, partners=len(shifts), k=int(k), shifts=list(shifts), labelled=labelled, ranks_g=hr[:, 0].copy(),
               ranks_l=hr[:, 1].copy(), labels=None, follows_g=None, follows_l=None, unlike_pairs=None, unswapped_acc=None,
               knn=int(knn) if labelled else None, n_ref=n_ref, Q=Q, mu=mu, Lg=Lg)
    for s in ("g", "l"):
        res.update({key + "_" + s: val for key, val in figures(res["ranks_" + s], int(k)).items()})
    if cls is not None:
        res["labels"] = host[nr + len(pred) * N:].astype(np.int64)
    if labelled:
        res.update(class_figures(host[nr:nr + len(pred) * N].reshape(len(passes), N), res["labels"], shifts))
    if keep:
        res["hybrids"] = kept
    return res


def grid_canvas(model, test_batches, mu, Lg, n, patch=1, seed=None):
    """The (n+1) x (n+1) tile canvas [(n+1) H, (n+1) W, 3] in [0, 1] of the first n images: the corner white, the top row the z_l
    sources, the left column the z_g sources, cell (i, j) the requantised decode([z_g of image i | z_l of image j])."""
    test_batches = list(test_batches)
    first = images_of(test_batches[0])
    B, H, W = (int(v) for v in first.shape[:3])
    N = int(mu.shape[0])
    n = min(int(n), N)
    xs = torch.cat([images_of(b)[..., :3] for b in test_batches[:(n + B - 1) // B]])[:n]
    cyc = _Cycle(model, mu, Lg, B, H, W, int(patch), model.seed if seed is None else seed)
    cells = torch.empty((n * n, H, W, 3), dtype=torch.float32, device=mu.device)
    ii = torch.arange(n * n, dtype=torch.int64, device=mu.device)
    for o in range(0, n * n, B):
        idx = ii[o:o + B]
        idx = torch.cat([idx, idx[-1:].expand(B - idx.numel())]) if idx.numel() < B else idx
        take = min(B, n * n - o)
        images6 = cyc.hybrids((idx // n).to(torch.int32), (idx % n).to(torch.int32), o)
        cells[o:o + take] = images6[:take, ..., :3]
    tiles = ((torch.cat([xs, cells]) + 1.0) * 0.5).cpu().numpy().astype(np.float64)
    canvas = np.ones(((n + 1) * H, (n + 1) * W, 3), np.float64)
    for a in range(n):
        canvas[0:H, (a + 1) * W:(a + 2) * W] = tiles[a]                  # top row: the z_l sources
        canvas[(a + 1) * H:(a + 2) * H, 0:W] = tiles[a]                  # left column: the z_g sources
        for b in range(n):
            canvas[(a + 1) * H:(a + 2) * H, (b + 1) * W:(b + 2) * W] = tiles[n + a * n + b]
    return canvas


def save_outputs(res, canvas, out_dir):
    """swap_grid.png and swap.npz under out_dir -> the paths written"""
    from .visualizer import save_png
    os.makedirs(out_dir, exist_ok=True)
    png = save_png(os.path.join(out_dir, "swap_grid.png"), canvas)
    N = res["n_images"]
    path = os.path.join(out_dir, "swap.npz")
    np.savez(path, ranks_g=res["ranks_g"].astype(np.int32), ranks_l=res["ranks_l"].astype(np.int32), shifts=np.asarray(res["shifts"], np.int32),
             labels=np.full((N,), -1, np.int32) if res["labels"] is None else res["labels"].astype(np.int32))
    return [png, path]


def _block(res, s):
    return BLOCK.format(res["kept1_" + s], res["k"], res["keptk_" + s], res["mrr_" + s], res["leak1_" + s], res["cycle1_" + s])


def report_line(res):
    line = REPORT.format(res["n_images"], res["partners"]) + 'z_g ' + _block(res, "g") + '; z_l ' + _block(res, "l")
    if res.get("labelled") and res.get("follows_g") is not None:
        line += CLASSES.format(res["follows_g"], res["follows_l"], res["unlike_pairs"], res["knn"], res["n_ref"], res["unswapped_acc"])
    return line


# ---------------------------------------------------------------- the command line
def check_flags(model, augmentation, images, partners, k, knn, refs, grid, global_latent_dims=1, local_latent_dims=1):
    """--model / --augmentation / --swap_images / --swap_partners / --swap_k / --swap_knn / --swap_refs / --swap_grid, before any data or
    device work."""
    if model == 'gmvae':
        raise SystemExit("--model gmvae has one latent block: the swap report needs z_g and z_l (lgvae, lggmvae)")
    if model not in ('lgvae', 'lggmvae'):
        raise SystemExit("--model %s: expected lgvae or lggmvae" % model)
    if augmentation not in ('scramble', 'no_op'):
        raise SystemExit("--augmentation %s: the x_hat half of a hybrid is a patch scramble; the swap report runs with scramble or no_op" % augmentation)
    if images is not None and (images < 2 or images > MAX_IMAGES):
        raise SystemExit("--swap_images N: at least 2 and at most %d test images, got %d" % (MAX_IMAGES, images))
    if partners < 1 or partners > MAX_PARTNERS or (images is not None and partners > images - 1):
        raise SystemExit("--swap_partners P: 1 <= P <= %d partners (and P < N), got %d" % (MAX_PARTNERS, partners))
    if k < 1:
        raise SystemExit("--swap_k K: K >= 1, got %d" % k)
    if knn < 0 or knn > KNN_MAX_K:
        raise SystemExit("--swap_knn K: 0 (off) or 1 <= K <= %d neighbours, got %d" % (KNN_MAX_K, knn))
    if knn and refs < knn:
        raise SystemExit("--swap_refs %d: the class figures need at least K = %d reference images" % (refs, knn))
    if grid < 1 or grid > MAX_GRID:
        raise SystemExit("--swap_grid n: 1 <= n <= %d images a side, got %d" % (MAX_GRID, grid))
    if not (1 <= global_latent_dims <= SWAP_MAX_L and 1 <= local_latent_dims <= SWAP_MAX_L):
        raise SystemExit("the swap report covers latent blocks of 1 .. %d dimensions" % SWAP_MAX_L)


def build_parser():
    from .main import build_parser as build_main_parser
    ap = build_main_parser()                           # a fresh parser object: main's and evaluate's stay as they are
    ap.description = "swap-consistency report of z_g and z_l of a saved weights file"
    ap.add_argument("--weights", type=str, required=True, help="file written by save_weights (.h5 / .hdf5 / .keras, else .npz)")
    ap.add_argument("--swap_images", type=int, default=None, help="the report covers the first N test images (default: all, at most %d)" % MAX_IMAGES)
    ap.add_argument("--swap_partners", type=int, default=1, help="P: z_l partners per image, 1 .. %d" % MAX_PARTNERS)
    ap.add_argument("--swap_k", type=int, default=10, help="k of kept@k")
    ap.add_argument("--swap_knn", type=int, default=5, help="neighbours of the class figures on labelled sets, 1 .. %d (0: off)" % KNN_MAX_K)
    ap.add_argument("--swap_refs", type=int, default=20000, help="training images the class figures take their references from")
    ap.add_argument("--swap_out", type=str, default=None, help="directory for swap_grid.png and swap.npz")
    ap.add_argument("--swap_grid", type=int, default=8, help="n: swap_grid.png shows the hybrids of the first n x n image pairs")
    return ap


def main(argv=None):
    from . import reports
    args = build_parser().parse_args(argv)
    check_flags(args.model, args.augmentation, args.swap_images, args.swap_partners, args.swap_k, args.swap_knn, args.swap_refs,
                args.swap_grid, args.global_latent_dims, args.local_latent_dims)      # before any data or device work
    if reports.any_on(args):
        on = [e.name for e in reports.TABLE if getattr(args, e.name) != 0]
        raise SystemExit("split_vae_amd.swap runs the swap report only: --%s belongs to python -m split_vae_amd.evaluate" % ", --".join(on))
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
    refs = None
    if config.label and args.swap_knn:
        from . import probe
        from .augmentation import ReferenceAugmentator
        aug = ReferenceAugmentator(type=config.augmentation, size=config.patch_size, seed=config.seed, pipeline=1)     # an augmentor of the report's own
        refs = probe.reference_batches(train_ds, args.swap_refs, aug, config.batch_size)
        if sum(int(b[1].shape[0]) for b in refs) < args.swap_knn:
            raise SystemExit("--swap_knn %d: the training set has fewer images" % args.swap_knn)
    n = MAX_IMAGES if args.swap_images is None else args.swap_images
    res = evaluate(model, test_batches, n, args.swap_partners, args.swap_k, patch=config.patch_size, knn=args.swap_knn if refs else 0,
                   ref_batches=refs)
    if res["n_images"] < n and args.swap_images is not None:
        print(CLIPPED.format(n, res["n_images"]))
    print(report_line(res))
    if args.swap_out:
        canvas = grid_canvas(model, test_batches, res["mu"], res["Lg"], args.swap_grid, patch=config.patch_size)
        res["files"] = save_outputs(res, canvas, args.swap_out)
    drop = ("ranks_g", "ranks_l", "labels", "Q", "mu", "Lg")
    return {("swap_" + key): val for key, val in res.items() if key not in drop}


if __name__ == "__main__":
    main()
