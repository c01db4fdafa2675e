"""Per-dimension latent report: which dimensions of z_g and z_l carry anything, and how entangled they are inside a block.

No reference counterpart.  Two standard figures per latent block, from the encoders' posteriors of N test images:

    active units (Burda et al. 2016)       dimension j is active when the variance over the images of its posterior mean exceeds
                                           ACTIVE_THRESHOLD = 0.01
    KL = MI + TC + dimension-wise KL       Chen et al. 2018 ("Isolating sources of disentanglement"), with the aggregate posterior
                                           of dimension j, q_j(z_j) = 1/N sum_n q(z_j | x_n), scored by sv_latent_dims_lse

on the samples, and against the block log-sum-exp, of the --latent_info report (sv_latent_info_draw / _lse), so the block's KL and MI
there equal MI + TC + dwKL here term by term (include/splitvae.h).  Every MI-type figure saturates at log N.  lgvae reports everything
for both blocks; lggmvae active units, MI_j and TC for z_g (its prior is a mixture: no KL_j, no dimension-wise KL) and everything for
z_l; gmvae the z_g figures of lggmvae.
"""
import torch

from . import ops, reports
from ._lib import LATENT_INFO_MAX_L
from .latent_info import posteriors
from .model import LGVae

ACTIVE_THRESHOLD = 0.01
REPORT = 'Test latent dimensions ({} images, log N = {:.4f}): '
CLIPPED = 'Note: --latent_dims {} clipped to the test set\'s {} images'
BLOCK_KEYS = ("dims", "active", "var", "kl", "mi", "dwkl", "tc", "dwkl_sum", "block_kl", "block_mi")


def check_flags(latent_dims, global_latent_dims=1, local_latent_dims=0):
    """--latent_dims, before any data or device work (main.py, evaluate.py)."""
    if latent_dims < 0 or latent_dims == 1:
        raise SystemExit("--latent_dims N: 0 (off) or N >= 2 test images, got %d" % latent_dims)
    if latent_dims and not (1 <= global_latent_dims <= LATENT_INFO_MAX_L and 0 <= local_latent_dims <= LATENT_INFO_MAX_L):
        raise SystemExit("--latent_dims covers latent blocks of at most %d dimensions" % LATENT_INFO_MAX_L)


def dimensions(mu, sig, Lg, eps=None, seed=0):
    """One fp64 device vector of N posteriors mu, sig [N, Lg+Ll]: out [8] of sv_latent_info_finish, then per block (z_g, then z_l when
    Ll > 0) cols [3 L] = (mean_j, var_j, KL_j) and out [3 L + 2] of sv_latent_dims_finish.  Nothing is read back."""
    Lc = int(mu.shape[1])
    parts = []
    with ops.hold_stream():
        z, rsig, cst, own_b, prior_b = ops.latent_info_draw(mu, sig, Lg, eps=eps, seed=seed)
        lse_b = ops.latent_info_lse(z, mu, rsig, cst, Lg)
        parts.append(ops.latent_info_finish(own_b, prior_b, lse_b, Lc - Lg))
        for e, (a, b) in enumerate(((0, Lg), (Lg, Lc))):
            if b == a:
                continue
            lc, own, cols = ops.latent_dims_prepare(mu[:, a:b], sig[:, a:b], eps=None if eps is None else eps[:, a:b], block=e, seed=seed)
            lse = ops.latent_dims_lse(z[:, a:b], mu[:, a:b], rsig[:, a:b], lc)
            parts += [cols.reshape(-1), ops.latent_dims_finish(lse, own, z[:, a:b], lse_b[e])]
        return torch.cat(parts)


def evaluate(model, test_batches, n, eps=None, seed=None):
    """The report over the first `n` test images (all of them when there are fewer): dict(n_images, log_n, and per block s in g, l:
    dims_s, active_s, var_s, kl_s, mi_s, dwkl_s (lists over the dimensions), tc_s, dwkl_sum_s, block_kl_s, block_mi_s), None where the
    model has no such figure.  eps [N, Lg+Ll] fp32 pins the samples; otherwise image i draws from (seed, i) (seed: model.seed): the
    samples of latent_info.evaluate.  One read-back."""
    if int(n) < 2:
        raise ValueError("latent_dims.evaluate needs n >= 2 images, got %r" % (n,))
    mu, sig, Lg, Ll = posteriors(model, test_batches, int(n))
    N = int(mu.shape[0])
    if N < 2:
        raise ValueError("latent_dims.evaluate needs at least 2 test images, got %d" % N)
    o = dimensions(mu, sig, Lg, eps=eps, seed=model.seed if seed is None else seed).cpu().tolist()
    res = dict(n_images=N, log_n=o[7])
    at = 8
    for s, L, blk in (("g", Lg, 0), ("l", Ll, 3)):
        if not L:
            res.update({k + "_" + s: None for k in BLOCK_KEYS})
            continue
        var, kl = o[at + L:at + 2 * L], o[at + 2 * L:at + 3 * L]
        at += 3 * L
        mi, dwkl, tc, dwkl_sum = o[at:at + L], o[at + L:at + 2 * L], o[at + 3 * L], o[at + 3 * L + 1]
        at += 3 * L + 2
        gaussian_prior = s == "l" or type(model) is LGVae    # the mixture models: the prior of z_g is not N(0, I)
        res.update({"dims_" + s: L, "active_" + s: sum(v > ACTIVE_THRESHOLD for v in var), "var_" + s: var, "mi_" + s: mi, "tc_" + s: tc,
                    "kl_" + s: kl if gaussian_prior else None, "dwkl_" + s: dwkl if gaussian_prior else None,
                    "dwkl_sum_" + s: dwkl_sum if gaussian_prior else None, "block_kl_" + s: o[blk] if gaussian_prior else None,
                    "block_mi_" + s: o[blk + 1]})
    return res


def _block(res, s):
    out = 'z_{} active {}/{}'.format(s, res["active_" + s], res["dims_" + s])
    kl = res["kl_" + s]
    if kl is not None:
        d = max(range(len(kl)), key=kl.__getitem__)
        out += ' (largest KL_j {:.4f} at dim {})'.format(kl[d], d)
    out += ', TC {:.4f}'.format(res["tc_" + s])
    if res["dwkl_sum_" + s] is not None:
        out += ', dimension-wise KL {:.4f}'.format(res["dwkl_sum_" + s])
    return out


def report_line(res):
    line = REPORT.format(res["n_images"], res["log_n"]) + _block(res, "g")
    if res.get("dims_l"):
        line += '; ' + _block(res, "l")
    return line


def report(model, test_batches, config, step=None):
    """--latent_dims N behind an evaluation's report (trainer.py, evaluate.py): prints the line, keeps the figures in
    config.latent_dims_history (one dict(step, ...) per evaluation, the per-dimension lists included) and returns them; None when the
    flag is off."""
    return reports.run("latent_dims", model, test_batches, config, step)
