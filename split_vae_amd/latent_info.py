"""Aggregate-posterior information report of the latents: how many nats about the image each latent block carries, and how much
of that the two blocks carry twice.

No reference counterpart.  Hoffman & Johnson's decomposition ("ELBO surgery") of the average KL term per block,

    KL = mean_i KL(q(z | x_i) || p(z)) = I(index; z) + KL(q(z) || p(z)),      q(z) = 1/N sum_j q(z | x_j),

estimated with one sample z_i per test image scored under every image's posterior (sv_latent_info_draw / _lse / _finish,
include/splitvae.h), and the mutual information of z_g and z_l under the aggregate posterior.  It needs no labels and no trained
probe.  Every MI-type figure saturates at log N (the known upward bias of the estimator): the report prints log N beside them.
lgvae reports everything; lggmvae the MI of both blocks and the overlap but KL / marginal KL for z_l only (the prior of z_g is a
mixture); gmvae the MI of z_g only.
"""
import torch

from . import ops, reports
from ._lib import LATENT_INFO_MAX_L, PHASE_FWD_ENCODERS, PHASE_PREP
from .model import LGVae
from .utils import images_of

REPORT = 'Test latent information ({} images, log N = {:.4f}): z_g '
CLIPPED = 'Note: --latent_info {} clipped to the test set\'s {} images'
HISTORY_KEYS = ("kl_g", "mi_g", "mkl_g", "kl_l", "mi_l", "mkl_l", "overlap", "log_n", "n_images")


def check_flags(latent_info, global_latent_dims=1, local_latent_dims=0):
    """--latent_info, before any data or device work (main.py, evaluate.py)."""
    if latent_info < 0 or latent_info == 1:
        raise SystemExit("--latent_info N: 0 (off) or N >= 2 test images, got %d" % latent_info)
    if latent_info and not (1 <= global_latent_dims <= LATENT_INFO_MAX_L and 0 <= local_latent_dims <= LATENT_INFO_MAX_L):
        raise SystemExit("--latent_info covers latent blocks of at most %d dimensions" % LATENT_INFO_MAX_L)


def batch_posterior(model, images, sample_offset=0):
    """(z_mean_x, z_sig_x, z_mean_x_hat or None, z_sig_x_hat or None) of one batch, as views of buffers the next batch overwrites:
    the encoder passes probe.latent_means reads its means from.  LGVae runs its encoders only; LGGMVae / GMVae run the model's forward
    (their z_mean_x is computed behind the relaxed categorical sample y, drawn at the model's current call counter).  That sample is
    keyed by the row's global sample index sample_offset + b: the default 0 keys a row by its place in the batch (every report so far);
    a caller that passes the batch's first global image index gets means that do not depend on how the images are batched.  LGVae's means
    depend on no noise."""
    from .gm import LGGMVae
    from .gmvae import GMVae, _images6
    B = images.shape[0]
    f32 = torch.float32
    if type(model) is LGVae:
        from .trainer import _check_images
        _check_images(model, images)
        plan = model.plan(B)
        Lg, Ll = model.global_latent_dims, model.local_latent_dims
        plan.step(PHASE_PREP | PHASE_FWD_ENCODERS, params=model.flat, images6=images, seed=model.seed)
        return (plan.buffer("z_mean_x", f32, (B, Lg)), plan.buffer("z_sig_x", f32, (B, Lg)),
                plan.buffer("z_mean_xh", f32, (B, Ll)), plan.buffer("z_sig_xh", f32, (B, Ll)))
    if not isinstance(model, (LGGMVae, GMVae)):
        raise TypeError("latent posteriors are read from LGVae, LGGMVae and GMVae models, got %s" % type(model).__name__)
    calls = model._calls
    try:
        out = model(_images6(images) if isinstance(model, GMVae) else images, copy=False, **({"sample_offset": int(sample_offset)} if sample_offset else {}))
    finally:
        model._calls = calls                       # a report between training steps does not move the training noise
    if isinstance(model, LGGMVae):
        return out[3], out[4], out[8], out[9]
    return out[3], out[4], None, None


def posteriors(model, batches, n=None, keyed=False):
    """The encoders' means and standard deviations of the first `n` images of `batches` ([B,H,W,6] device batches, or (images,
    labels) pairs; n None: all) -> (mu, sig [N, Lg+Ll] fp32 device tensors: columns 0 .. Lg-1 z_g, the rest z_l; Lg, Ll).  keyed: image i
    draws the mixture models' noise as global sample i (batch_posterior's sample_offset), whatever the batch size.  Leaves model._calls
    alone."""
    mus, sigs, have, Lg, Ll = [], [], 0, 0, 0
    for batch in batches:
        if n is not None and have >= n:
            break
        images = images_of(batch)
        mg, sg, ml, sl = batch_posterior(model, images, have if keyed else 0)
        Lg, Ll = int(mg.shape[1]), (0 if ml is None else int(ml.shape[1]))
        take = images.shape[0] if n is None else min(images.shape[0], n - have)
        mus.append(torch.cat([mg[:take]] + ([ml[:take]] if Ll else []), dim=1))
        sigs.append(torch.cat([sg[:take]] + ([sl[:take]] if Ll else []), dim=1))
        have += take
    if not mus:
        raise ValueError("latent_info: no test batches")
    return torch.cat(mus).contiguous(), torch.cat(sigs).contiguous(), Lg, Ll


def information(mu, sig, Lg, eps=None, seed=0):
    """out [8] fp64 on the device (sv_latent_info_finish) of N posteriors mu, sig [N, Lg+Ll]: three calls (four launches), nothing read back."""
    with ops.hold_stream():
        z, rsig, cst, own, prior = ops.latent_info_draw(mu, sig, Lg, eps=eps, seed=seed)
        lse = ops.latent_info_lse(z, mu, rsig, cst, Lg)
        return ops.latent_info_finish(own, prior, lse, mu.shape[1] - Lg)


def evaluate(model, test_batches, n, eps=None, seed=None):
    """The report over the first `n` test images (all of them when there are fewer): dict(n_images, log_n, kl_g, mi_g, mkl_g, kl_l,
    mi_l, mkl_l, overlap), None where the model has no such figure.  eps [N, Lg+Ll] fp32 pins the samples; otherwise image i draws
    from (seed, i) (seed: model.seed), so the same weights give the same figures.  One read-back."""
    if int(n) < 2:
        raise ValueError("latent_info.evaluate needs n >= 2 images, got %r" % (n,))
    mu, sig, Lg, Ll = posteriors(model, test_batches, int(n))
    N = int(mu.shape[0])
    if N < 2:
        raise ValueError("latent_info.evaluate needs at least 2 test images, got %d" % N)
    o = information(mu, sig, Lg, eps=eps, seed=model.seed if seed is None else seed).cpu().tolist()
    res = dict(n_images=N, log_n=o[7], kl_g=o[0], mi_g=o[1], mkl_g=o[2], kl_l=None, mi_l=None, mkl_l=None, overlap=None)
    if type(model) is not LGVae:                   # the mixture models: the prior of z_g is not N(0, I)
        res["kl_g"] = res["mkl_g"] = None
    if Ll:
        res.update(kl_l=o[3], mi_l=o[4], mkl_l=o[5], overlap=o[6])
    return res


def _block(res, s):
    if res["kl_" + s] is None:
        return 'MI {:.4f}'.format(res["mi_" + s])
    return 'KL {:.4f}, MI {:.4f}, marginal KL {:.4f}'.format(res["kl_" + s], res["mi_" + s], res["mkl_" + s])


def report_line(res):
    line = REPORT.format(res["n_images"], res["log_n"]) + _block(res, "g")
    if res.get("mi_l") is not None:
        line += '; z_l ' + _block(res, "l") + '; overlap I(z_g; z_l) {:.4f}'.format(res["overlap"])
    return line


def report(model, test_batches, config, step=None):
    """--latent_info N behind an evaluation's report (trainer.py, evaluate.py): prints the line, keeps the figures in
    config.latent_info_history (one dict(step, ...) per evaluation) and returns them; None when the flag is off."""
    return reports.run("latent_info", model, test_batches, config, step)
