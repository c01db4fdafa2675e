"""Sample-quality report of prior draws: do decodes of latents drawn from the prior look, to the model's own encoders, like test images?

No reference counterpart.  The paper's Fig. 4 and Fig. 6 sample from the prior, and visualizer.generate* draws the pictures; this report
puts figures on them that need no Inception weights: the improved precision / recall of Kynkaanniemi et al. 2019, the density / coverage
of Naeem et al. 2020 and a Frechet distance of Gaussian fits, all in one feature space with one k-NN rule (sv_prdc_radius /
sv_prdc_count, include/splitvae.h).

    python -m split_vae_amd.sample_quality --weights models/20260101-120000.h5 --dataset svhn --beta 40
    python -m split_vae_amd.sample_quality --weights models/20260101-120000.h5 --dataset celeba64 -no_label --patch_size 8 --sq_out out/sq

Definitions:
  features   of an image: the encoders' posterior means [z_g | z_l] of the image "as the image it is" (gmvae: z_g alone).  THE FEATURE SPACE
             IS THE MODEL'S OWN ENCODER: the figures compare checkpoints of one architecture on one dataset, and a collapsed encoder
             flatters them (the `reconstructions` column and --latent_dims show when).  This is no FID.
  real set   X [N, Lg+Ll]: the posterior means of the first N test images (latent_info.posteriors, keyed by the global image index)
  fake sets  Y [N, Lg+Ll] each; fake i is keyed by the global image index i, so no figure depends on the batch size: a zcat, the decoders,
             the mean requantised to pixel levels beside its scramble (sv_swap_requantise; the permutation keyed by (seed, this report's
             step tag, i)), re-encoded under the noise key of image i (swap.py's cycle).  The zcat is
               prior    z_g and z_l both drawn          g_drawn  z_g drawn, z_l = image i's mean
               l_drawn  z_l drawn, z_g = image i's mean  recon    both means: the ceiling, like swap's cycle@1
             with sv_recon_draw's draws (KEEP_L draws z_g, KEEP_G draws z_l; the mixture models draw z_g from the uniform-y mixture
             prior); `prior` joins the drawn halves of those two calls in fp32 and rounds once to the plan's dtype.  gmvae: prior, recon.
  radii      rad_X, rad_Y: the squared distance to the k-th nearest OTHER row of the same set (self excluded by index)
  figures    precision = mean_j [cnt(Y->X, rad_X)[j] > 0]      density  = sum_j cnt(Y->X, rad_X)[j] / (k N)
             recall    = mean_i [cnt(X->Y, rad_Y)[i] > 0]      coverage = mean_i [dmin(X->Y)[i] <= rad_X[i]]
             Frechet   = |m_a - m_b|^2 + tr C_a + tr C_b - 2 sum sqrt(max(lambda, 0)), lambda the eigenvalues of C_a^(1/2) C_b C_a^(1/2),
             m and C (divisor N) from sv_linprobe_gram's fp64 sums.  Float64 on the host from four read-back vectors per fake set.

The command takes the flags of split_vae_amd.main plus --weights, --sq_images, --sq_k, --sq_out, --sq_grid.  It is an entry point of its own:
reports.TABLE and the parsers of main / evaluate do not know it.  No labels are needed.
"""
import os

import numpy as np
import torch

from . import ops
from ._lib import PHASE_FWD_DECODERS, PHASE_PREP, PRDC_MAX_K, PRDC_MAX_L, RECON_KEEP_G, RECON_KEEP_L, RECON_MEANS
from .swap import _Cycle
from .utils import images_of

REPORT = 'Test sample quality ({} images, k={}): '
FIGURES = 'precision {:.4f}, recall {:.4f}, density {:.4f}, coverage {:.4f}, Frechet {:.4f}'
TITLES = (("prior", "prior "), ("g_drawn", "z_g drawn (z_l kept): "), ("l_drawn", "z_l drawn (z_g kept): "), ("recon", "reconstructions: "))
ONE_BLOCK = ("prior", "recon")                     # gmvae
CLIPPED = 'Note: --sq_images {} clipped to the test set\'s {} images'
CAPPED = 'Note: the test set has {} images: CLIPPED to the first {} (the default of --sq_images)'
MAX_IMAGES = 65536                                 # the default of --sq_images: all test images, capped here
MAX_GRID = 32
PERM_STEP = 0x7371 << 40                           # 'sq': the `step` key of the samples' permutations (swap.py keeps 0x7377 << 40)
KEYS = ("precision", "recall", "density", "coverage", "frechet")


# ---------------------------------------------------------------- figures (float64, host)
def moments(S, n):
    """S [(L+1),(L+1)] = [x 1]^T [x 1] (sv_linprobe_gram) of n rows -> (m [L], C [L,L]) with divisor n"""
    S = np.asarray(S, np.float64)
    L = S.shape[0] - 1
    m = S[L, :L] / n
    return m, S[:L, :L] / n - np.outer(m, m)


def frechet(ma, Ca, mb, Cb):
    """|m_a - m_b|^2 + tr C_a + tr C_b - 2 tr (C_a^(1/2) C_b C_a^(1/2))^(1/2), every root through numpy.linalg.eigh with negative
    eigenvalues (rounding) taken as 0"""
    ma, mb, Ca, Cb = (np.asarray(v, np.float64) for v in (ma, mb, Ca, Cb))
    w, V = np.linalg.eigh((Ca + Ca.T) * 0.5)
    root = (V * np.sqrt(np.maximum(w, 0.0))) @ V.T
    M = root @ Cb @ root
    lam = np.linalg.eigh((M + M.T) * 0.5)[0]
    d = ma - mb
    return float(d @ d + np.trace(Ca) + np.trace(Cb) - 2.0 * np.sqrt(np.maximum(lam, 0.0)).sum())


def figures(cnt_fake, cnt_real, dmin_real, rad_real, k):
    """cnt_fake [N] = cnt(Y->X, rad_X), cnt_real [N] = cnt(X->Y, rad_Y), dmin_real [N] = dmin(X->Y), rad_real [N] = rad_X -> dict"""
    cf, cr = np.asarray(cnt_fake, np.int64), np.asarray(cnt_real, np.int64)
    dm, rx = np.asarray(dmin_real, np.float64), np.asarray(rad_real, np.float64)
    return dict(precision=float(np.mean((cf > 0).astype(np.float64))), density=float(cf.sum()) / (float(k) * cf.shape[0]),
                recall=float(np.mean((cr > 0).astype(np.float64))), coverage=float(np.mean((dm <= rx).astype(np.float64))))


# ---------------------------------------------------------------- the fake sets
def set_names(model):
    from .gmvae import GMVae
    return ONE_BLOCK if isinstance(model, GMVae) else tuple(name for name, _ in TITLES)


def draw_prior(model):
    """(pm, ps) of the mixture models' uniform-y prior of z_g (recon_quality.mixture_prior; gmvae's by the same encode_y), None for lgvae"""
    from .gmvae import GMVae
    from .recon_quality import mixture_prior
    if isinstance(model, GMVae):
        pm, ps = model.encode_y(torch.eye(model.y_size, dtype=torch.float32, device=model.device))
        return pm.float().contiguous(), ps.float().contiguous()
    return mixture_prior(model)


class _Samples(_Cycle):
    """swap's cycle with the zcat of a fake set in place of a hybrid's"""

    def __init__(self, model, mu, Lg, B, H, W, patch, seed):
        super().__init__(model, mu, Lg, B, H, W, patch, seed)
        Lc = int(mu.shape[1])
        self.prior = draw_prior(model)
        self.drawn_g = torch.empty((B, Lc), dtype=torch.float32, device=mu.device)      # fp32 scratch of `prior`
        self.drawn_l = torch.empty((B, Lc), dtype=torch.float32, device=mu.device)

    def fill(self, name, rows, o):
        """self.zcat of the fake set `name` for the images rows [B] (global index o + b draws)"""
        Lg = self.Lg
        mg = rows[:, :Lg]
        ml = rows[:, Lg:] if rows.shape[1] > Lg else None
        kw = dict(prior=self.prior, seed=self.seed, sample_offset=o)
        if name == "recon":
            ops.recon_draw(mg, ml, RECON_MEANS, self.zcat)
        elif name == "g_drawn":
            ops.recon_draw(mg, ml, RECON_KEEP_L, self.zcat, **kw)
        elif name == "l_drawn":
            ops.recon_draw(mg, ml, RECON_KEEP_G, self.zcat, **kw)
        elif ml is None:                           # prior, one block
            ops.recon_draw(mg, None, RECON_KEEP_L, self.zcat, **kw)
        else:                                      # prior: the drawn halves of the two calls, one rounding to the plan's dtype
            ops.recon_draw(mg, ml, RECON_KEEP_L, self.drawn_g, **kw)
            ops.recon_draw(mg, ml, RECON_KEEP_G, self.drawn_l, **kw)
            ops.recon_draw(self.drawn_g[:, :Lg], self.drawn_l[:, Lg:], RECON_MEANS, self.zcat)

    def samples(self, name, rows, o):
        """-> self.images6: the decode of the fake set's zcat as the image it is, beside its scramble"""
        with ops.hold_stream():
            self.fill(name, rows, o)
            self.plan.step(PHASE_PREP | PHASE_FWD_DECODERS, params=self.model.flat)
            ops.random_perm(self.B, self.perm.shape[1], self.seed, PERM_STEP, o, out=self.perm)
            ops.swap_requantise(self.out6, self.lut, self.perm, self.patch, out=self.images6)
        return self.images6


def fake_features(model, cyc, name, keep=None):
    """Y [N, Lc]: the re-encoded means of the fake set; keep [n,H,W,3]: receives the first n requantised samples"""
    from .latent_info import batch_posterior
    N, B, Lg, dev = cyc.N, cyc.B, cyc.Lg, cyc.mu.device
    Y = torch.empty((N, int(cyc.mu.shape[1])), dtype=torch.float32, device=dev)
    for o in range(0, N, B):
        idx = torch.arange(o, o + B, dtype=torch.int64, device=dev).clamp_(max=N - 1)     # a short last batch repeats image N - 1
        take = min(B, N - o)
        images6 = cyc.samples(name, cyc.mu.index_select(0, idx), o)
        mg, _, ml, _ = batch_posterior(model, images6, o)                                  # fake i under the noise key of image i
        Y[o:o + take, :Lg] = mg[:take]
        if ml is not None:
            Y[o:o + take, Lg:] = ml[:take]
        if keep is not None and o < keep.shape[0]:
            n = min(take, keep.shape[0] - o)
            keep[o:o + n] = images6[:n, ..., :3]
    return Y


def evaluate(model, test_batches, n, k=5, seed=None, patch=1, grid=0, keep=False):
    """The report over the first `n` test images (all when there are fewer).  seed: model.seed.  patch: the scramble's patch size
    (--patch_size).  grid > 0: res["samples"] [grid,H,W,3] keeps the first requantised prior samples.  keep: res["Y"] keeps the fake sets'
    features (tests).  -> dict(n_images, k, sets; per set s: precision_s, recall_s, density_s, coverage_s, frechet_s and the arrays
    cnt_fake_s, cnt_real_s, dmin_real_s, imin_fake_s [N]; rad_real [N]; X [N, Lc] device tensor, Lg).  One read-back per fake set.
    Leaves model._calls alone."""
    from .latent_info import posteriors
    k = int(k)
    if not 1 <= k <= PRDC_MAX_K:
        raise ValueError("sample_quality.evaluate: 1 <= k <= %d, got %d" % (PRDC_MAX_K, k))
    if int(n) < k + 1:
        raise ValueError("sample_quality.evaluate needs n >= k + 1 = %d images, got %r" % (k + 1, n))
    test_batches = list(test_batches)
    X, _, Lg, Ll = posteriors(model, test_batches, int(n), keyed=True)
    N, Lc = int(X.shape[0]), Lg + Ll
    if N < k + 1:
        raise ValueError("sample_quality.evaluate needs at least k + 1 = %d test images, got %d" % (k + 1, N))
    if Lc > PRDC_MAX_L:
        raise ValueError("sample_quality.evaluate: the feature space has Lg + Ll = %d dimensions, at most %d" % (Lc, PRDC_MAX_L))
    seed = model.seed if seed is None else seed
    first = images_of(test_batches[0])
    B, H, W = (int(v) for v in first.shape[:3])
    dev = X.device
    cyc = _Samples(model, X, Lg, B, H, W, int(patch), seed)
    ws = torch.empty((ops.prdc_workspace_bytes(N, N, Lc, k),), dtype=torch.uint8, device=dev)
    with ops.hold_stream():
        rad_x = ops.prdc_radius(X, k, workspace=ws)
        S_x = ops.linprobe_gram(X)
    sets = set_names(model)
    res = dict(n_images=N, k=k, sets=sets, X=X, Lg=Lg)
    m_x = C_x = None
    for name in sets:
        samples = torch.empty((min(int(grid), N), H, W, 3), dtype=torch.float32, device=dev) if grid and name == "prior" else None
        Y = fake_features(model, cyc, name, samples)
        with ops.hold_stream():
            rad_y = ops.prdc_radius(Y, k, workspace=ws)
            cnt_f, _, imin_f = ops.prdc_count(Y, X, rad_x, workspace=ws)
            cnt_r, dmin_r, _ = ops.prdc_count(X, Y, rad_y, workspace=ws)
            S_y = ops.linprobe_gram(Y)
        ints = torch.cat([cnt_f, cnt_r, imin_f]).cpu().numpy().astype(np.int64)
        flts = torch.cat([dmin_r, rad_x]).cpu().numpy()
        Sh = torch.stack([S_x, S_y]).cpu().numpy()
        if m_x is None:
            m_x, C_x = moments(Sh[0], N)
            res["rad_real"] = flts[N:].copy()
        fig = figures(ints[:N], ints[N:2 * N], flts[:N], res["rad_real"], k)
        fig["frechet"] = frechet(m_x, C_x, *moments(Sh[1], N))
        res.update({key + "_" + name: val for key, val in fig.items()})
        res.update({"cnt_fake_" + name: ints[:N].copy(), "cnt_real_" + name: ints[N:2 * N].copy(), "dmin_real_" + name: flts[:N].copy(),
                    "imin_fake_" + name: ints[2 * N:].copy()})
        if samples is not None:
            res["samples"] = samples
        if keep:
            res.setdefault("Y", {})[name] = Y
    return res


def nearest_canvas(res, test_batches):
    """[2 H, n W, 3] in [0, 1]: the first n requantised prior samples above the test images imin names (their nearest in feature space)"""
    samples = res["samples"]
    n, H, W, _ = samples.shape
    B = int(images_of(test_batches[0]).shape[0])
    near = res["imin_fake_prior"][:n]
    tiles = [images_of(test_batches[int(j) // B])[int(j) % B, ..., :3] for j in near]
    both = ((torch.cat([samples, torch.stack(tiles)]) + 1.0) * 0.5).cpu().numpy().astype(np.float64)
    canvas = np.ones((2 * H, n * W, 3), np.float64)
    for a in range(n):
        canvas[0:H, a * W:(a + 1) * W] = both[a]
        canvas[H:2 * H, a * W:(a + 1) * W] = both[n + a]
    return canvas


def save_outputs(res, canvas, out_dir):
    """sample_nearest.png and sample_quality.npz under out_dir -> the paths written"""
    from .visualizer import save_png
    os.makedirs(out_dir, exist_ok=True)
    png = save_png(os.path.join(out_dir, "sample_nearest.png"), canvas)
    doc = dict(k=np.int32(res["k"]), n_images=np.int32(res["n_images"]), rad_real=res["rad_real"].astype(np.float32))
    for name in res["sets"]:
        for key in KEYS:
            doc[key + "_" + name] = np.float64(res[key + "_" + name])
        for key in ("cnt_fake", "cnt_real", "imin_fake"):
            doc[key + "_" + name] = res[key + "_" + name].astype(np.int32)
        doc["dmin_real_" + name] = res["dmin_real_" + name].astype(np.float32)
    path = os.path.join(out_dir, "sample_quality.npz")
    np.savez(path, **doc)
    return [png, path]


def report_line(res):
    parts = [title + FIGURES.format(*(res[key + "_" + name] for key in ("precision", "recall", "density", "coverage", "frechet")))
             for name, title in TITLES if name in res["sets"]]
    return REPORT.format(res["n_images"], res["k"]) + "; ".join(parts)


# ---------------------------------------------------------------- the command line
def check_flags(model, augmentation, images, k, grid, global_latent_dims=1, local_latent_dims=0):
    """--model / --augmentation / --sq_images / --sq_k / --sq_grid, before any data or device work."""
    if model not in ('lgvae', 'lggmvae', 'gmvae'):
        raise SystemExit("--model %s: expected lgvae, lggmvae or gmvae" % model)
    if augmentation not in ('scramble', 'no_op'):
        raise SystemExit("--augmentation %s: the x_hat half of a sample is a patch scramble; the sample-quality report runs with scramble or no_op" % augmentation)
    if k < 1 or k > PRDC_MAX_K:
        raise SystemExit("--sq_k K: 1 <= K <= %d neighbours, got %d" % (PRDC_MAX_K, k))
    if images is not None and (images < k + 1 or images > MAX_IMAGES):
        raise SystemExit("--sq_images N: at least K + 1 = %d and at most %d test images, got %d" % (k + 1, MAX_IMAGES, images))
    if grid < 1 or grid > MAX_GRID:
        raise SystemExit("--sq_grid n: 1 <= n <= %d samples, got %d" % (MAX_GRID, grid))
    width = global_latent_dims + (0 if model == 'gmvae' else local_latent_dims)
    if global_latent_dims < 1 or local_latent_dims < 0 or width > PRDC_MAX_L:
        raise SystemExit("the sample-quality report covers a feature space of Lg + Ll <= %d dimensions, got %d" % (PRDC_MAX_L, width))


def build_parser():
    from .main import build_parser as build_main_parser
    ap = build_main_parser()                           # a fresh parser object: main's and evaluate's stay as they are
    ap.description = "sample-quality report (precision / recall, density / coverage, Frechet) of the prior draws of a saved weights file"
    ap.add_argument("--weights", type=str, required=True, help="file written by save_weights (.h5 / .hdf5 / .keras, else .npz)")
    ap.add_argument("--sq_images", type=int, default=None, help="the report covers the first N test images (default: all, at most %d)" % MAX_IMAGES)
    ap.add_argument("--sq_k", type=int, default=5, help="k of the k-NN balls, 1 .. %d" % PRDC_MAX_K)
    ap.add_argument("--sq_out", type=str, default=None, help="directory for sample_nearest.png and sample_quality.npz")
    ap.add_argument("--sq_grid", type=int, default=10, help="n: sample_nearest.png shows the first n prior samples above their nearest test images")
    return ap


def main(argv=None):
    from . import reports
    args = build_parser().parse_args(argv)
    check_flags(args.model, args.augmentation, args.sq_images, args.sq_k, args.sq_grid, args.global_latent_dims,
                args.local_latent_dims)                # before any data or device work
    if reports.any_on(args):
        on = [e.name for e in reports.TABLE if getattr(args, e.name) != 0]
        raise SystemExit("split_vae_amd.sample_quality runs the sample-quality report only: --%s belongs to python -m split_vae_amd.evaluate"
                         % ", --".join(on))
    from .main import check_augmentation, make_augmentors, make_model
    from .utils import dotdict
    config = dotdict(vars(args))
    check_augmentation(config.augmentation, args.model)
    from . import configure_hw_queues
    configure_hw_queues()                              # before the first HIP call (split_vae_amd/__init__.py)
    config.label = False                               # no labels anywhere: CelebA, --synthetic and -no_label all run
    from . import data
    _, test_augmentor = make_augmentors(config)
    _, test_ds, input_shape = data.get_dataset(config.dataset, config.batch_size, synthetic=config.synthetic, data_dir=config.data_dir,
                                               get_label=False)
    test_batches = [test_augmentor.augment(x) for x in test_ds]      # the test batches of main(): the augmentor's first calls
    model, _ = make_model(args.model, config, input_shape)
    model.load_weights(args.weights)
    n = MAX_IMAGES if args.sq_images is None else args.sq_images
    have = sum(int(images_of(b).shape[0]) for b in test_batches)
    if min(n, have) < args.sq_k + 1:
        raise SystemExit("--sq_k %d: the test set has %d images, the report needs K + 1" % (args.sq_k, have))
    res = evaluate(model, test_batches, n, args.sq_k, patch=config.patch_size, grid=args.sq_grid if args.sq_out else 0)
    if res["n_images"] < n and args.sq_images is not None:
        print(CLIPPED.format(n, res["n_images"]))
    elif args.sq_images is None and have > MAX_IMAGES:
        print(CAPPED.format(have, MAX_IMAGES))
    print(report_line(res))
    if args.sq_out:
        res["files"] = save_outputs(res, nearest_canvas(res, test_batches), args.sq_out)
    return {("sq_" + key): val for key, val in res.items() if not (torch.is_tensor(val) or isinstance(val, (np.ndarray, dict))) and key != "Lg"}


if __name__ == "__main__":
    main()
