"""Label-free reconstruction quality report: how close a decode is to its image, and how much of the image each latent block pins down.

The reference's labelled test step (vae/trainer.py:213-226) scores three decodes per test batch with a classifier whose weights are
missing upstream: the reconstruction, decode(z_x, random z_l) ("z_g kept") and decode(random z_g, z_x_hat) ("z_l kept"): the figures
behind Table 1.  The decodes need no classifier.  This report scores them in image space instead: the mean PSNR and the mean SSIM of
each against the original image x, over the first N test images.  It is the project's own stand-in for Table 1, as the k-NN probe is;
it needs no labels, so it also runs on CelebA and on synthetic data.

Definitions (include/splitvae.h: sv_recon_draw / sv_recon_quality / sv_recon_finish):
  images   the reference image is (x + 1) * 0.5 from channels 0..2 of the staged six-channel batch; the decode is
           clip((x_mean + 1) * 0.5, 0, 1) -- decode(rescale=True), vae/model.py:215 -- from channels 0..2 of the plan's out6_x; both are
           read in place; max_val = 1
  PSNR     per image 10 log10(1 / max(MSE_i, 1e-10)), MSE_i over H*W*3; the mean over images (the tf.image.psnr convention; the floor
           only keeps an exact copy finite)
  SSIM     the defaults of tf.image.ssim (Wang et al. 2004): 11 x 11 Gaussian window, sigma 1.5, normalised to sum 1; population
           moments; C1 = 0.01^2, C2 = 0.03^2; the valid region only, (H-10) x (W-10); per channel; per image the mean over windows and
           channels; the mean over images
  kept     blocks are the posterior MEANS (the reference keeps a posterior sample): the figures depend on the weights and the seed alone
  drawn    blocks come from a Philox stream keyed by (seed, global image index, a tag of this report's own) through the Box-Muller of
           sv_iw_advance: image i draws the same numbers whatever the batch size.  lgvae draws from N(0, I); lggmvae draws z_g from the
           uniform-y mixture prior: a component c uniformly, z_g = pm[c] + ps[c] * eps with (pm, ps) = encode_y(identity); gmvae has
           one block and reports the reconstruction only.
"""
import torch

from . import ops, reports
from ._lib import PHASE_FWD_DECODERS, PHASE_PREP, RECON_KEEP_G, RECON_KEEP_L, RECON_MEANS
from .latent_info import batch_posterior
from .utils import images_of

REPORT = 'Test reconstruction quality ({} images): '
FIGURES = 'PSNR {:.2f} dB, SSIM {:.4f}'
CLIPPED = 'Note: --recon_quality {} clipped to the test set\'s {} images'
HISTORY_KEYS = ("psnr", "ssim", "psnr_g", "ssim_g", "psnr_l", "ssim_l", "n_images")
VARIANTS = (("", RECON_MEANS), ("_g", RECON_KEEP_G), ("_l", RECON_KEEP_L))     # (key suffix, sv_recon_draw mode): _g = z_g kept


def check_flags(recon_quality):
    """--recon_quality, before any data or device work (main.py, evaluate.py)."""
    if recon_quality < 0:
        raise SystemExit("--recon_quality N: 0 (off) or N >= 1 test images, got %d" % recon_quality)


def mixture_prior(model):
    """(pm, ps) [y_size, Lg] fp32 of an LGGMVae: the prior mean and standard deviation of every component (encode_y of the identity);
    None for the other models (LGVae: N(0, I); GMVae: nothing is drawn)."""
    from .gm import LGGMVae
    if not isinstance(model, LGGMVae):
        return None
    pm, ps = model.encode_y(torch.eye(model.y_size, dtype=torch.float32, device=model.device))
    return pm.float().contiguous(), ps.float().contiguous()


def evaluate(model, test_batches, n, eps=None, seed=None, comp=None):
    """The report over the first `n` test images (all of them when there are fewer): dict(n_images, psnr, ssim, psnr_g, ssim_g, psnr_l,
    ssim_l), None where the model has no such figure (_g: z_g kept, z_l from its prior; _l: z_l kept).  eps [N, Lg+Ll] fp32 pins the
    normals and comp [N] int32 the mixture components; otherwise image i draws from (seed, i) (seed: model.seed).  Per batch the
    encoders run once; per variant sv_recon_draw, the decoders, sv_recon_quality on the batch and out6_x where they lie,
    sv_recon_finish onto a device accumulator.  One read-back.  Leaves model._calls alone."""
    from .gmvae import GMVae
    if int(n) < 1:
        raise ValueError("recon_quality.evaluate needs n >= 1 images, got %r" % (n,))
    n, seed = int(n), (model.seed if seed is None else seed)
    variants = VARIANTS[:1] if isinstance(model, GMVae) else VARIANTS
    prior = mixture_prior(model)
    acc = torch.zeros((len(variants), 3), dtype=torch.float64, device=model.device)
    have = 0
    for batch in test_batches:
        if have >= n:
            break
        images = images_of(batch)
        B, H, W = images.shape[:3]
        take = min(B, n - have)
        mg, _, ml, _ = batch_posterior(model, images)
        Lg, Ll = int(mg.shape[1]), (0 if ml is None else int(ml.shape[1]))
        plan = model.plan(B)
        zcat = plan.buffer("zcat", model.dtype, (B, Lg + Ll))
        out6 = plan.buffer("out6_x", torch.float32, (B, H, W, 6))
        per_image = torch.empty((B, 2), dtype=torch.float64, device=images.device)
        ws = torch.empty((ops.recon_quality_workspace_bytes(B, H, W),), dtype=torch.uint8, device=images.device)
        ep = None if eps is None else eps[have:have + B]
        cp = None if comp is None else comp[have:have + B]
        with ops.hold_stream():
            for v, (_, mode) in enumerate(variants):
                ops.recon_draw(mg, ml, mode, zcat, eps=ep, comp=cp, prior=prior, seed=seed, sample_offset=have)
                plan.step(PHASE_PREP | PHASE_FWD_DECODERS, params=model.flat)
                ops.recon_quality(images, out6, 0, 0, True, per_image=per_image, workspace=ws)
                ops.recon_finish(per_image, acc[v], take)
        have += take
    if not have:
        raise ValueError("recon_quality: no test batches")
    host = acc.cpu().tolist()
    res = dict(n_images=have, psnr=None, ssim=None, psnr_g=None, ssim_g=None, psnr_l=None, ssim_l=None)
    for (s, _), (sum_psnr, sum_ssim, count) in zip(variants, host):
        assert int(count) == have
        res["psnr" + s], res["ssim" + s] = sum_psnr / count, sum_ssim / count
    return res


def report_line(res):
    line = REPORT.format(res["n_images"]) + FIGURES.format(res["psnr"], res["ssim"])
    if res.get("psnr_g") is not None:
        line += '; z_g kept (z_l ~ prior): ' + FIGURES.format(res["psnr_g"], res["ssim_g"])
        line += '; z_l kept (z_g ~ prior): ' + FIGURES.format(res["psnr_l"], res["ssim_l"])
    return line


def report(model, test_batches, config, step=None):
    """--recon_quality N behind an evaluation's report (trainer.py, evaluate.py): prints the line, keeps the figures in
    config.recon_quality_history (one dict(step, ...) per evaluation) and returns them; None when the flag is off."""
    return reports.run("recon_quality", model, test_batches, config, step)
