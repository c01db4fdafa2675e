"""Importance-weighted test log-likelihood of LGVae: the IW-K bound of Burda et al. in nats and bits per dimension.

No reference counterpart: test_step_lg_vae (vae/trainer.py:199-233) reports the single-sample ELBO pieces.  The estimator is
pinned in include/splitvae.h (sv_iw_advance).  Per test batch the encoders run once; each of the K samples is one decoder +
loss pass of the plan over latents that sv_iw_advance drew into `zcat`, and the same kernel folds the finished pass into a
per-image fp64 log-sum-exp on the device.  Everything is enqueued on one stream; nothing inside the K loop reads the device.
"""
import math

import torch

from . import ops
from ._lib import IW_ACCUMULATE, IW_DRAW, PHASE_FWD_DECODERS, PHASE_FWD_ENCODERS, PHASE_LOSS, PHASE_PREP
from .model import LGVae

REFUSAL = ("--iw_samples covers --model lgvae only: for lggmvae / gmvae the prior is the y-conditional mixture and q contains a "
           "relaxed categorical, which needs a different estimator")
REPORT = 'Test IW-{} bound: joint {:.4f}, x {:.4f} nats; x bits/dim {:.4f}'


def check_model_name(model_name, iw_samples):
    """--iw_samples against --model, before any data or device work (main.py, evaluate.py)."""
    if iw_samples < 0:
        raise SystemExit("--iw_samples must be >= 0")
    if iw_samples and model_name != 'lgvae':
        raise SystemExit("--model %s: %s." % (model_name, REFUSAL))


def bits_per_dim(mean_log_likelihood, H, W, channels=3):
    """Mean log p(x) in nats -> bits per dimension.  No offset: the discretised logistic is a probability mass over the 256 levels."""
    return -mean_log_likelihood / (H * W * channels * math.log(2.0))


def _check(model, images6, K):
    if type(model) is not LGVae:
        raise TypeError("%s (got %s)" % (REFUSAL, type(model).__name__))
    if int(K) < 1:
        raise ValueError("K must be >= 1, got %r" % (K,))
    from .trainer import _check_images
    _check_images(model, images6)


def log_likelihood(model, images6, K, eps=None, seed=None, sample_offset=0, acc=None, prep=True):
    """Per-image device tensors (L_joint, L_x, elbo) [B] fp32 of the K-sample bound for one batch images6 [B,H,W,6].
    eps [K,B,Lg+Ll] fp32 pins the latent noise; otherwise sample k of image sample_offset + b is a Philox draw keyed by (seed,
    image, k) (seed: model.seed), whatever batch the image sits in and whatever K is.  acc [4] fp64 (device) collects the batch's
    sums and count (sv_iw_finish); prep=False skips the weight preparation when this plan has run it since the last update.
    Leaves model._calls alone: an evaluation between training steps does not move the training noise."""
    _check(model, images6, K)
    K = int(K)
    B = images6.shape[0]
    Lg, Ll = model.global_latent_dims, model.local_latent_dims
    if eps is not None and (tuple(eps.shape) != (K, B, Lg + Ll) or eps.dtype != torch.float32 or not eps.is_cuda or not eps.is_contiguous()):
        raise ValueError("eps must be a contiguous [K=%d, B=%d, %d] fp32 device tensor" % (K, B, Lg + Ll))
    seed = model.seed if seed is None else seed
    plan = model.plan(B)
    f32 = torch.float32
    zm_x, zs_x = plan.buffer("z_mean_x", f32, (B, Lg)), plan.buffer("z_sig_x", f32, (B, Lg))
    zm_h, zs_h = plan.buffer("z_mean_xh", f32, (B, Ll)), plan.buffer("z_sig_xh", f32, (B, Ll))
    zcat = plan.buffer("zcat", model.dtype, (B, Lg + Ll))
    nll_x, nll_xh = plan.buffer("nll_x", f32, (B,)), plan.buffer("nll_xh", f32, (B,))
    state = torch.empty((B, 5), dtype=torch.float64, device=images6.device)
    r = torch.empty((B,), dtype=f32, device=images6.device)
    with ops.hold_stream():
        plan.step((PHASE_PREP if prep else 0) | PHASE_FWD_ENCODERS, params=model.flat, images6=images6, seed=model.seed)
        for k in range(K + 1):
            flags = (IW_ACCUMULATE if k > 0 else 0) | (IW_DRAW if k < K else 0)
            ops.iw_advance(zm_x, zs_x, zm_h, zs_h, zcat, r, k, flags, nll_x=nll_x, nll_xh=nll_xh, state=state,
                           eps=None if eps is None or k == K else eps[k], seed=seed, sample_offset=sample_offset)
            if k < K:
                plan.step(PHASE_FWD_DECODERS | PHASE_LOSS, params=model.flat, images6=images6)
        out = ops.iw_finish(state, K, acc=acc)
    return out[:, 0], out[:, 1], out[:, 2]


def evaluate(model, batches, K, seed=None):
    """Means over a test set: {iw_joint, iw_x, elbo (nats per image), bits_per_dim_x, n_images}.  `batches`: [B,H,W,6] device
    batches (or (images, labels) pairs).  The sums stay on the device until the one read-back at the end; the weight preparation
    runs once per plan, not per batch; image i of the set draws with sample_offset = i."""
    acc = torch.zeros((4,), dtype=torch.float64, device=model.device)
    prepped, offset = set(), 0
    for batch in batches:
        images6 = batch[0] if isinstance(batch, (tuple, list)) else batch
        B = images6.shape[0]
        log_likelihood(model, images6, K, seed=seed, sample_offset=offset, acc=acc, prep=B not in prepped)
        prepped.add(B)
        offset += B
    a = acc.cpu().tolist()
    n = int(a[3])
    if n == 0:
        raise ValueError("evaluate: no test batches")
    out = dict(iw_joint=a[0] / n, iw_x=a[1] / n, elbo=a[2] / n, n_images=n)
    out["bits_per_dim_x"] = bits_per_dim(out["iw_x"], model.H, model.W)
    return out


def report_line(K, res):
    return REPORT.format(int(K), res["iw_joint"], res["iw_x"], res["bits_per_dim_x"])
