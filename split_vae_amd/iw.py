"""Importance-weighted test log-likelihood of LGVae: the IW-K bound of Burda et al. in nats and bits per dimension.

No reference counterpart: test_step_lg_vae (vae/trainer.py:199-233) reports the single-sample ELBO pieces.  The estimator is
pinned in include/splitvae.h (sv_iw_advance).  Per test batch the encoders run once; each of the K samples is one decoder +
loss pass of the plan over latents that sv_iw_advance drew into `zcat`, and the same kernel folds the finished pass into a
per-image fp64 log-sum-exp on the device.  Everything is enqueued on one stream; nothing inside the K loop reads the device.
"""
import math

import torch

from . import ops, reports
from ._lib import IW_ACCUMULATE, IW_DRAW, PHASE_FWD_DECODERS, PHASE_FWD_ENCODERS, PHASE_LOSS, PHASE_PREP
from .model import LGVae
from .utils import images_of

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
        images6 = images_of(batch)
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


def report(model, test_batches, config, step=None):
    """--iw_samples K behind an evaluation's report (trainer.py, evaluate.py): prints the line and returns the figures (no history is
    kept); None when the flag is off or the model is not an LGVae."""
    return reports.run("iw_samples", model, test_batches, config, step)


# ---------------------------------------------------------------- the mixture models: LGGMVae and GMVae (sv_iw_gm_advance)
# The estimator is pinned in include/splitvae.h: y is marginalised on both sides, so a sample is a component pick c ~ Cat(pi_b), a
# draw from the posterior component c, and two n-component mixture log-densities.  Per batch the encoders run once (the GM encoder
# in test mode and, for LGGMVae, the plan's local encoder) and sv_iw_gm_tables builds the component tables once; then K decoder +
# loss passes with K + 1 launches of sv_iw_gm_advance between them, all on one stream.
MIXTURE_REPORT = 'Test IW-{} mixture bound: joint {:.4f}, x {:.4f} nats; x bits/dim {:.4f}'
MIXTURE_MODELS = ('lggmvae', 'gmvae')
MIXTURE_HISTORY_KEYS = ("gm_iw_joint", "gm_iw_x", "gm_bits_per_dim_x")


def check_mixture_model_name(model_name, gm_iw_samples):
    """--gm_iw_samples against --model, before any data or device work (main.py, evaluate.py)."""
    if gm_iw_samples < 0:
        raise SystemExit("--gm_iw_samples must be >= 0")
    if gm_iw_samples and model_name not in MIXTURE_MODELS:
        raise SystemExit("--model %s: --gm_iw_samples covers --model lggmvae / gmvae only (the mixture estimator); for lgvae use "
                         "--iw_samples." % model_name)


def _mixture_kind(model):
    from .gm import LGGMVae
    from .gmvae import GMVae
    if type(model) is LGGMVae:
        return True
    if type(model) is GMVae:
        return False
    raise TypeError("the mixture bound covers LGGMVae and GMVae only; LGVae has log_likelihood (got %s)" % type(model).__name__)


def _gm_params(model):
    """(kernel, bias) views into model.gm_flat of the five Dense layers the component tables need."""
    from .gm import GM_LAYERS
    views = model._gm_views(model.gm_flat)
    return {n: (views[2 * GM_LAYERS.index(n)], views[2 * GM_LAYERS.index(n) + 1]) for n in ("ht", "zm", "zs", "pm", "ps")}


def mixture_log_likelihood(model, images, K, eps=None, comp=None, seed=None, sample_offset=0, acc=None, prep=True):
    """Per-image device tensors (L_joint, L_x, elbo) [B] fp32 of the K-sample mixture bound of LGGMVae / GMVae for one batch
    [B,H,W,6] (GMVae also takes the 9-channel high_low_pass batch: it scores channels 0-2, as test_step_gm_vae does).  eps
    [K,B,Lg+Ll] fp32 and comp [K,B] int32 pin the noise and the components (Ll = 0 for GMVae); otherwise sample k of image
    sample_offset + b is keyed by (seed, image, k).  GMVae: L_joint == L_x.  `elbo` is the mean log-weight of this estimator, not
    the training loss.  acc, prep: as log_likelihood.  Leaves model._calls alone."""
    split = _mixture_kind(model)
    if int(K) < 1:
        raise ValueError("K must be >= 1, got %r" % (K,))
    K = int(K)
    if not split:
        from .gmvae import _images6
        images = _images6(images)
    elif torch.is_tensor(images) and images.dim() == 4 and images.shape[-1] == 9:
        raise ValueError("LGGMVae cannot score a high_low_pass batch (9 channels: x | x - low | low): its x_hat decoder has 3 channels")
    from .trainer import _check_images
    _check_images(model, images)
    B = images.shape[0]
    Lg, Ll = model.global_latent_dims, (model.local_latent_dims if split else 0)
    n = model.y_size
    f32, i32, dev = torch.float32, torch.int32, images.device
    if eps is not None and (tuple(eps.shape) != (K, B, Lg + Ll) or eps.dtype != f32 or not eps.is_cuda or not eps.is_contiguous()):
        raise ValueError("eps must be a contiguous [K=%d, B=%d, %d] fp32 device tensor" % (K, B, Lg + Ll))
    if comp is not None and (tuple(comp.shape) != (K, B) or comp.dtype != i32 or not comp.is_cuda or not comp.is_contiguous()):
        raise ValueError("comp must be a contiguous [K=%d, B=%d] int32 device tensor" % (K, B))
    seed = model.seed if seed is None else seed
    plan, enc = model.plan(B), model.encoder(B)
    zcat = plan.buffer("zcat", model.dtype, (B, Lg + Ll))
    nll_x = plan.buffer("nll_x", f32, (B,))
    zm_h = zs_h = nll_xh = None
    if split:
        zm_h, zs_h = plan.buffer("z_mean_xh", f32, (B, Ll)), plan.buffer("z_sig_xh", f32, (B, Ll))
        nll_xh = plan.buffer("nll_xh", f32, (B,))
    state = torch.empty((B, 5), dtype=torch.float64, device=dev)
    r = torch.empty((B,), dtype=f32, device=dev)
    comp_out = torch.empty((B,), dtype=i32, device=dev)
    P = _gm_params(model)
    images = images.contiguous()
    with ops.hold_stream():
        plan.step((PHASE_PREP if prep else 0) | PHASE_FWD_ENCODERS, params=model.flat, images6=images, seed=model.seed)
        if prep:
            enc.prep(model.gm_flat)
        enc.forward(model.gm_flat, plan.buffer("in8_x", model.dtype, (B, model.H, model.W, 8)), zcat, False, seed=model.seed)
        zm_all, zs_all, pm, ps = ops.iw_gm_tables(enc.buf["he"], *P["ht"], *P["zm"], *P["zs"], *P["pm"], *P["ps"])
        logits = enc.buf["logits"]
        for k in range(K + 1):
            flags = (IW_ACCUMULATE if k > 0 else 0) | (IW_DRAW if k < K else 0)
            ops.iw_gm_advance(logits, zm_all, zs_all, pm, ps, zm_h, zs_h, zcat, r, comp_out, k, flags, nll_x=nll_x, nll_xh=nll_xh,
                              state=state, eps=None if eps is None or k == K else eps[k],
                              comp=None if comp is None or k == K else comp[k], seed=seed, sample_offset=sample_offset)
            if k < K:
                plan.step(PHASE_FWD_DECODERS | PHASE_LOSS, params=model.flat, images6=images)
        out = ops.iw_finish(state, K, acc=acc)
    return out[:, 0], out[:, 1], out[:, 2]


def mixture_evaluate(model, batches, K, seed=None):
    """Means over a test set: {gm_iw_joint, gm_iw_x, gm_elbo (nats per image), gm_bits_per_dim_x, n_images}; as evaluate: one
    read-back per test set, the weight preparation once per plan, image i of the set draws with sample_offset = i."""
    _mixture_kind(model)
    acc = torch.zeros((4,), dtype=torch.float64, device=model.device)
    prepped, offset = set(), 0
    for batch in batches:
        images = images_of(batch)
        B = images.shape[0]
        mixture_log_likelihood(model, images, K, seed=seed, sample_offset=offset, acc=acc, prep=B not in prepped)
        prepped.add(B)
        offset += B
    a = acc.cpu().tolist()
    n = int(a[3])
    if n == 0:
        raise ValueError("mixture_evaluate: no test batches")
    out = dict(gm_iw_joint=a[0] / n, gm_iw_x=a[1] / n, gm_elbo=a[2] / n, n_images=n)
    out["gm_bits_per_dim_x"] = bits_per_dim(out["gm_iw_x"], model.H, model.W)
    return out


def mixture_report_line(K, res):
    return MIXTURE_REPORT.format(int(K), res["gm_iw_joint"], res["gm_iw_x"], res["gm_bits_per_dim_x"])


def mixture_report(model, test_batches, config, step=None):
    """--gm_iw_samples K behind an evaluation's report: prints the line, keeps dict(step, gm_iw_joint, gm_iw_x, gm_bits_per_dim_x) in
    config.gm_iw_history and returns the figures; None when the flag is off or the model is an LGVae."""
    return reports.run("gm_iw_samples", model, test_batches, config, step)
