"""float64 twin of the importance-weighted log-likelihood (include/splitvae.h: sv_iw_advance / sv_iw_finish; split_vae_amd/iw.py).

Two parts: the streaming log-sum-exp update and its finish in NumPy float64, and the whole estimator on the fp64 forward of
oracle/torch_ref.py (the oracle tests/test_gpu_step.py compares the step against), given the same weights and the same eps.
"""
import math

import numpy as np


# ---------------------------------------------------------------- streaming update and finish
def state_init(B):
    """[B,5] = (m_joint, s_joint, m_x, s_x, sum lw_joint) before any sample: m = -inf, s = 0."""
    st = np.zeros((B, 5), np.float64)
    st[:, 0] = st[:, 2] = -np.inf
    return st


def _push(m, s, lw):
    mn = np.maximum(m, lw)
    return mn, s * np.exp(m - mn) + np.exp(lw - mn)


def state_push(st, nll_x, nll_xh, r):
    """Fold one sample in: lw_joint = -nll_x - nll_xh + r, lw_x = -nll_x + r (float64, this order of operations)."""
    nx, nh, rr = (np.asarray(a).astype(np.float64) for a in (nll_x, nll_xh, r))
    lw_j, lw_x = -nx - nh + rr, -nx + rr
    out = np.empty_like(st)
    out[:, 0], out[:, 1] = _push(st[:, 0], st[:, 1], lw_j)
    out[:, 2], out[:, 3] = _push(st[:, 2], st[:, 3], lw_x)
    out[:, 4] = st[:, 4] + lw_j
    return out


def finish(st, K):
    """[B,3] float64 = (L_K joint, L_K x, elbo)."""
    logK = math.log(float(K))
    return np.stack([st[:, 0] + np.log(st[:, 1]) - logK, st[:, 2] + np.log(st[:, 3]) - logK, st[:, 4] / float(K)], axis=1)


def acc_add(acc, out3):
    """The device accumulator: (sum L_joint, sum L_x, sum elbo, count), the float64 values added in image index order."""
    acc = np.array(acc, np.float64)
    for row in out3:
        acc[:3] += row
    acc[3] += out3.shape[0]
    return acc


def stream_lse(lw):
    """L_K = logsumexp_k lw[k] - log K of a 1-D sequence through the streaming update, in the order given."""
    m, s = -np.inf, 0.0
    for v in np.asarray(lw, np.float64):
        m, s = _push(m, s, v)
    return float(m + np.log(s) - math.log(len(lw)))


def bits_per_dim(mean_ll, H, W, channels=3):
    return -mean_ll / (H * W * channels * math.log(2.0))


# ---------------------------------------------------------------- the latent log-ratio
def latent_ratio(mu, sig, eps=None, z_stored=None):
    """r = sum_j [log N(z_j; 0, 1) - log N(z_j; mu_j, sig_j)] = sum_j [(eps_j^2 - z_j^2) / 2 + log sig_j], float64, [B].
    eps: z = mu + sig * eps as drawn (the fp32 plan); z_stored: the value the decoder consumed, eps~ = (z~ - mu) / sig (bf16)."""
    mu, sig = np.asarray(mu).astype(np.float64), np.asarray(sig).astype(np.float64)
    if z_stored is not None:
        z = np.asarray(z_stored).astype(np.float64)
        e = (z - mu) / sig
    else:
        e = np.asarray(eps).astype(np.float64)
        z = mu + sig * e
    return (0.5 * (e * e - z * z) + np.log(sig)).sum(axis=1)


# ---------------------------------------------------------------- the whole estimator on the fp64 oracle
def estimator(params_np, images6, eps=None, z_stored=None):
    """(out3 [B,3], lw_joint [K,B], lw_x [K,B]) float64.  images6 [B,H,W,6]; eps [K,B,Lg+Ll] (z = mu + sig eps in float64) or
    z_stored [K,B,Lg+Ll] (the latents a bf16 plan stored, decoded as they are)."""
    import torch
    from oracle import torch_ref as tr
    P = [torch.as_tensor(np.asarray(p)).double() for p in params_np]
    img = torch.as_tensor(np.asarray(images6)).double()
    H, W = img.shape[1:3]
    x, xh = img[..., :3], img[..., 3:]
    Lg, Ll = P[6].shape[1], P[16].shape[1]
    zero_g, zero_l = torch.zeros((img.shape[0], Lg), dtype=torch.float64), torch.zeros((img.shape[0], Ll), dtype=torch.float64)
    _, mu_g, sg_g = tr.encoder_conv(x, P[0:10], zero_g)
    _, mu_l, sg_l = tr.encoder_conv(xh, P[10:20], zero_l)
    mu, sig = torch.cat([mu_g, mu_l], 1), torch.cat([sg_g, sg_l], 1)
    src = eps if z_stored is None else z_stored
    K = src.shape[0]
    st = state_init(img.shape[0])
    lws_j, lws_x = [], []
    for k in range(K):
        if z_stored is None:
            z = mu + sig * torch.as_tensor(np.asarray(eps[k])).double()
            r = latent_ratio(mu.numpy(), sig.numpy(), eps=eps[k])
        else:
            z = torch.as_tensor(np.asarray(z_stored[k])).double()
            r = latent_ratio(mu.numpy(), sig.numpy(), z_stored=z_stored[k])
        xm, xls = tr.decoder(z, P[20:30], H, W)
        hm, hls = tr.decoder(z[:, Lg:], P[30:40], H, W)
        nll_x = tr.discretised_logistic_loss(x, xm, xls).sum(dim=(1, 2, 3)).numpy()
        nll_h = tr.discretised_logistic_loss(xh, hm, hls).sum(dim=(1, 2, 3)).numpy()
        st = state_push(st, nll_x, nll_h, r)
        lws_j.append(-nll_x - nll_h + r)
        lws_x.append(-nll_x + r)
    return finish(st, K), np.stack(lws_j), np.stack(lws_x)


def closed_form_nll(images6):
    """Per-image (c_x, c_xh): the oracle's discretised-logistic loss at mean 0, log-scale 0."""
    import torch
    from oracle import torch_ref as tr
    img = torch.as_tensor(np.asarray(images6)).double()
    zero = torch.zeros_like(img[..., :3])
    return (tr.discretised_logistic_loss(img[..., :3], zero, zero).sum(dim=(1, 2, 3)).numpy(),
            tr.discretised_logistic_loss(img[..., 3:], zero, zero).sum(dim=(1, 2, 3)).numpy())
