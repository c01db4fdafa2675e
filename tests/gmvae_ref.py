"""fp64 restatement of GMVae.call + train_step_gm_vae + Keras Adam (vae/model.py:277-298, vae/trainer.py:176-198), composed from the
oracle's pieces: oracle.gm_ref.encoder_gmvae (the GMVAE encoder), torch_ref.decoder, torch_ref.discretised_logistic_loss,
gm_ref.kl_divergence_two_gauss, gm_ref.categorical_kl and torch_ref.keras_adam_.  A test helper (not collected: no test_ prefix); it
adds nothing to oracle/.

All randomness is an input: eps [B,L] (Sampling), u [B,K] (Gumbel uniforms), keep1 [B,1024] / keep5 [B,F] (dropout keep masks).
"""
import math

import numpy as np
import torch

from oracle import gm_ref, torch_ref

NAMES9 = ["x_mean", "x_log_scale", "z_x", "z_mean_x", "z_sig_x", "y", "y_logits", "z_prior_mean", "z_prior_sig"]
LOSS_KEYS = ["x_recon_loss", "x_kl_loss", "y_kl_loss", "total_loss"]


def gmvae_param_shapes(H, W, latent=128, y_size=30):
    """The 34 trainable variables of GMVae in layer-tracking order: encoder_x (gmvae, 24 arrays), then decoder_x over z_x alone
    (vae/model.py:285-286: Decoder(latent_dims=global_latent); d1 [latent, ((H//8)*W)//8*128])."""
    enc = gm_ref.gm_param_shapes(H, W, latent, latent, y_size)[:24]
    d1_out = ((H // 8) * W) // 8 * 128
    dec = []
    for name, shp in [("d1", (latent, d1_out)), ("d2", (4, 4, 128, 128)), ("d3", (4, 4, 128, 64)), ("d4", (6, 6, 64, 32)),
                      ("d5", (6, 6, 32, 6))]:
        dec.append(("decoder_x/" + name + "/kernel", shp))
        dec.append(("decoder_x/" + name + "/bias", (shp[-1],)))
    return enc + dec


def gmvae_glorot_init(H, W, seed=3, latent=128, y_size=30, dtype=np.float32):
    """Keras defaults: Glorot-uniform kernels, zero biases, z_prior_sig / z_sig biases 1 (vae/model.py:68,:78)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = []
    for name, shp in gmvae_param_shapes(H, W, latent, y_size):
        if name.endswith("kernel"):
            fan_in = int(np.prod(shp[:-1]))
            fan_out = int(np.prod(shp[:-2])) * shp[-1] if len(shp) == 4 else shp[-1]
            lim = math.sqrt(6.0 / (fan_in + fan_out))
            out.append(rng.uniform(-lim, lim, size=shp).astype(dtype))
        else:
            one = name in ("encoder_x/z_prior_sig/bias", "encoder_x/z_sig/bias")
            out.append((np.ones if one else np.zeros)(shp, dtype=dtype))
    return out


def gmvae_forward(images, params, eps, u, keep1, keep5, tau=0.4, dropout=True):
    """GMVae.call (vae/model.py:288-298): x = inputs[..., :3]; the 9-tuple."""
    H, W = images.shape[1:3]
    x = images[..., :3]
    z_x, z_mean_x, z_sig_x, y, y_logits, zpm, zps = gm_ref.encoder_gmvae(x, params[0:24], eps, u, keep1, keep5, tau, dropout)
    x_mean, x_log_scale = torch_ref.decoder(z_x, params[24:34], H, W)
    return x_mean, x_log_scale, z_x, z_mean_x, z_sig_x, y, y_logits, zpm, zps


def gmvae_losses(images, fwd, beta, alpha, y_size):
    """vae/trainer.py:180-190."""
    x_mean, x_log_scale, z_x, z_mean_x, z_sig_x, y, y_logits, zpm, zps = fwd
    x = images[..., :3]
    x_recon = torch_ref.discretised_logistic_loss(x, x_mean, x_log_scale).sum(dim=(1, 2, 3)).mean()
    x_kl = gm_ref.kl_divergence_two_gauss(z_mean_x, z_sig_x, zpm, zps)
    y_kl = gm_ref.categorical_kl(y_logits, y_size)
    total = x_recon + beta * x_kl + alpha * y_kl
    return dict(x_recon_loss=x_recon, x_kl_loss=x_kl, y_kl_loss=y_kl, total_loss=total)


class GMVaeRefTrainer:
    """Stateful restatement of train_step_gm_vae (vae/trainer.py:176-198) + Keras Adam."""

    def __init__(self, params, beta, alpha, y_size=30, tau=0.4, lr=1e-4, dtype=torch.float64, dropout=True):
        self.dropout = dropout
        self.params = [torch.as_tensor(p).to(dtype).clone().requires_grad_(True) for p in params]
        self.m = [torch.zeros_like(p) for p in self.params]
        self.v = [torch.zeros_like(p) for p in self.params]
        self.t = 0
        self.beta, self.alpha, self.y_size, self.tau, self.lr, self.dtype = float(beta), float(alpha), y_size, tau, lr, dtype

    def forward_losses(self, images, eps, u, keep1, keep5):
        c = lambda a: torch.as_tensor(a).to(self.dtype)
        images = c(images)
        fwd = gmvae_forward(images, self.params, c(eps), c(u), c(keep1), c(keep5), self.tau, self.dropout)
        return fwd, gmvae_losses(images, fwd, self.beta, self.alpha, self.y_size)

    def grads(self, *a):
        fwd, losses = self.forward_losses(*a)
        return fwd, losses, list(torch.autograd.grad(losses["total_loss"], self.params))

    def train_step(self, *a):
        fwd, losses, g = self.grads(*a)
        self.t += 1
        torch_ref.keras_adam_(self.params, g, self.m, self.v, self.t, self.lr)
        return {k: float(v.detach()) for k, v in losses.items()}, g


def linear_assignment_accuracy(labels, logits):
    """Literal restatement of vae/trainer.py:40-68 (linear_assignment) followed by tf.keras.metrics.CategoricalAccuracy: per cluster,
    tf.unique_with_counts of its members' classes (classes in order of first appearance), tf.argmax of the counts (the first maximum),
    then the majority class one-hot; accuracy = mean(argmax(labels) == argmax(prediction))."""
    labels, logits = np.asarray(labels), np.asarray(logits)
    lab = np.argmax(labels, axis=1)
    cluster = np.argmax(logits, axis=1)
    pred = np.zeros_like(lab)
    for i in range(logits.shape[1]):
        members = lab[cluster == i]
        if members.shape[0] == 0:
            continue
        uniq, first = [], {}
        counts = []
        for c in members:
            if c not in first:
                first[c] = len(uniq)
                uniq.append(c)
                counts.append(0)
            counts[first[c]] += 1
        maj = uniq[int(np.argmax(counts))]
        pred = np.where(cluster == i, maj, pred)
    onehot = np.eye(labels.shape[1])[pred]
    return float(np.mean(np.argmax(labels, axis=1) == np.argmax(onehot, axis=1)))
