"""GMVae: the GMVAE baseline of the reference's Table 2 (vae/model.py:277-320) and its steps train_step_gm_vae / test_step_gm_vae
(vae/trainer.py:176-198, :277-294), plus the unsupervised cluster accuracy of vae/trainer.py:40-68, :315-349.

GMVae = Encoder(type='gmvae') -> Decoder(latent_dims=global_latent): ONE branch, no local encoder, no second decoder, no x-hat term.
The encoder is the natively sequenced GMVAE encoder of the SPLIT-GMVAE model (gm.NativeGMEncoder, csrc/gm_encoder.hip); the decoder,
the discretised-logistic loss head and Adam of the decoder are the LGVae step plan built with `global_only` (csrc/lgvae_plan.hip:
decoder_x over z_x alone, d1 kernel [global_latent, (H/8)(W/8)128]).  torch only owns the buffers.

Trainable variables (34), Keras order: the 24 arrays of encoder_x (gm.gm_param_table), then the 10 of decoder_x.  The Keras variable
names are the reference's (`encoder_x/...`, `decoder_x/...`, model name gm_vae).  The inputs are the reference's [B,H,W,6] batches
(x | x_aug on the channel axis); the model reads channels 0-2 only (vae/model.py:289).
"""
import numpy as np
import torch

from . import ops
from ._lib import PHASE_ADAM, PHASE_BWD_DECODERS, PHASE_FWD_DECODERS, PHASE_FWD_ENCODERS, PHASE_INPUTS_STAGED, PHASE_LOSS, PHASE_PREP
from .gm import LGGMVae, gm_param_table
from .model import LGVae

GM_LOSS_KEYS = ["x_recon_loss", "x_kl_loss", "y_kl_loss", "total_loss"]
_METRIC_IDX = [0, 1, 4, 5]          # of sv_gm_metrics' six outputs (the x-hat terms are zero here)


def decoder_desc(H, W, latent, dtype):
    """The global-only plan descriptor of GMVae's decoder_x (batch 1: the parameter table does not depend on it)."""
    return ops.LGVaeDesc(1, H, W, latent, latent, ops.sv_dtype(dtype), 1.0, 1, 1)


def variable_table(H, W, latent, y_size, dtype=torch.float32):
    """[(Keras variable name, shape)] of GMVae's 34 trainable variables in the reference's order (host only: no device needed)."""
    return ([(n, shp) for n, _, shp in gm_param_table(H, W, latent, y_size)] +
            [(n, shp) for n, _, shp in ops.param_table(decoder_desc(H, W, latent, dtype))])


class GMVae:
    """vae/model.py:277-287: GMVae(global_latent_dims, image_shape, y_size, tau)."""

    KERAS_MODEL_NAME = "gm_vae"

    def __init__(self, global_latent_dims, image_shape, y_size, tau, variational=True, type='conv', dtype='bf16', device=None, seed=0,
                 dropout_in_training=False):
        if not variational:
            raise NotImplementedError('Determiistic LG-AE not implemented')   # vae/model.py:298
        if not torch.cuda.is_available():
            from ._lib import SplitVaeError
            raise SplitVaeError("split_vae_amd needs a HIP device (MI355X); there is no CPU path")
        self.global_latent_dims = global_latent_dims
        self.variational = variational
        self.image_shape = image_shape
        self.y_size, self.tau = y_size, tau
        self.H, self.W = int(image_shape[1]), int(image_shape[2])
        self.dtype = {"bf16": torch.bfloat16, "f32": torch.float32, "fp32": torch.float32}.get(dtype, dtype)
        self.device = torch.device(device or "cuda")
        self.seed = seed
        # False: tensorflow 2.0.0 (pinned) -- `training` never reaches encoder_x's Dropout layers; True: tensorflow >= 2.1
        # (the same switch as LGGMVae: GMVae.call drops `training` on the way to encoder_x too, vae/model.py:292)
        self.dropout_in_training = bool(dropout_in_training)
        self.beta, self.alpha = 1.0, 40.0                  # set by the trainer from config.beta / config.alpha (vae/main.py:19,:29)
        self._calls = 0
        self._plans, self._enc, self._enc_py = {}, {}, {}
        # decoder_x: the global-only plan's parameter table (10 arrays)
        self.param_table = ops.param_table(decoder_desc(self.H, self.W, global_latent_dims, self.dtype))
        self.n_params = self.param_table[-1][1] + (int(np.prod(self.param_table[-1][2])) + 3) // 4 * 4
        self.flat = torch.zeros(self.n_params, dtype=torch.float32, device=self.device)
        self.grad_flat = torch.zeros_like(self.flat)
        # encoder_x: the GMVAE encoder's 24 arrays (gm.gm_param_table)
        self.gm_table = gm_param_table(self.H, self.W, global_latent_dims, y_size)
        self.gm_n_params = self.gm_table[-1][1] + (int(np.prod(self.gm_table[-1][2])) + 3) // 4 * 4
        self.gm_flat = torch.zeros(self.gm_n_params, dtype=torch.float32, device=self.device)
        self.gm_grad_flat = torch.zeros_like(self.gm_flat)
        self._metrics_buf = torch.zeros(8, dtype=torch.float32, device=self.device)      # sv_gm_metrics writes [0:6]
        self._zeros = {}                                                                 # [B] zeros: the absent x-hat terms of sv_gm_metrics
        LGVae._init_glorot(self, seed)                     # Keras defaults of the decoder (glorot kernels, zero biases)
        LGGMVae._init_gm(self, seed + 1)                   # ... and of the encoder (z_prior_sig / z_sig biases 1)

    # ---------------------------------------------------------------- variables (34 arrays)
    def _views(self, flat):
        return [flat[off:off + int(np.prod(shape))].view(*shape) for (_, off, shape) in self.param_table]

    _gm_views = LGGMVae._gm_views

    @property
    def trainable_variables(self):
        return self._gm_views(self.gm_flat) + self._views(self.flat)

    @property
    def gradients(self):
        return self._gm_views(self.gm_grad_flat) + self._views(self.grad_flat)

    def keras_names(self):
        return [n + ":0" for n, _, _ in self.gm_table] + [n + ":0" for n, _, _ in self.param_table]

    def _keras_kind(self, name):
        if name.startswith("encoder_x/"):
            return LGGMVae._keras_kind(self, name)        # (its encoder_x branch does not reach LGVae's)
        return LGVae._keras_kind(self, name)

    keras_h5_layers = LGVae.keras_h5_layers
    save_weights = LGVae.save_weights
    load_weights = LGVae.load_weights
    summary = LGGMVae.summary

    def set_weights(self, arrays):
        assert len(arrays) == 34
        for v, a in zip(self.trainable_variables, arrays):
            v.copy_(torch.as_tensor(np.asarray(a), dtype=torch.float32).to(self.device).reshape(v.shape))

    def get_weights(self):
        return [v.detach().cpu().numpy().copy() for v in self.trainable_variables]

    # ---------------------------------------------------------------- plans
    def plan(self, B, beta=None):
        """The global-only step plan for batch B (decoder_x, its loss head, its Adam)."""
        beta = self.beta if beta is None else beta
        key = (int(B), float(beta))
        if key not in self._plans:
            self._plans[key] = ops.LGVaePlan(B, self.H, self.W, self.global_latent_dims, self.global_latent_dims, beta=beta,
                                             dtype=self.dtype, device=self.device, external_global_encoder=True, global_only=True)
        return self._plans[key]

    encoder = LGGMVae.encoder                              # the natively sequenced GMVAE encoder for batch B (one per B)
    _py_encoder = LGGMVae._py_encoder

    def _zero_terms(self, B):
        z = self._zeros.get(B)
        if z is None:
            z = self._zeros[B] = torch.zeros(B, dtype=torch.float32, device=self.device)
        return z

    def _forward(self, inputs, training, eps, noise, want_loss, plan_kw):
        """eps [B, L] pins the Sampling noise, noise = (u, keep1, keep5) the Gumbel uniforms / dropout masks (parity tests)."""
        B = inputs.shape[0]
        plan, enc = self.plan(B), self.encoder(B)
        u, k1, k5 = (None, None, None) if noise is None else noise
        kw = dict(params=self.flat, images6=inputs.contiguous(), seed=self.seed, step=self._calls)
        kw.update(plan_kw)
        # Augmentator.augment(..., plan=plan) left this batch's padded input in in8_x (still current: generation, version counter)
        staged = getattr(inputs, "_sv_staged_plan", None) is plan and inputs._sv_staged_gen == plan.in8_gen and inputs._sv_staged_version == inputs._version
        if getattr(inputs, "_sv_staged_plan", None) is plan:
            inputs._sv_staged_plan = None                     # one step per staging
        # the plan's encoder phase: the decoder's weight images, dz zeroed, in8_x filled (unless staged) -- no encoder of its own
        plan.step(PHASE_PREP | PHASE_FWD_ENCODERS | (PHASE_INPUTS_STAGED if staged else 0), **kw)
        enc.prep(self.gm_flat)
        enc.forward(self.gm_flat, plan.buffer("in8_x", self.dtype, (B, self.H, self.W, 8)),
                    plan.buffer("zcat", self.dtype, (B, self.global_latent_dims)), bool(training) and self.dropout_in_training, eps=eps, u=u,
                    keep1=k1, keep5=k5, seed=self.seed, step=self._calls, sample_offset=kw.get("sample_offset", 0))
        plan.step(PHASE_FWD_DECODERS | (PHASE_LOSS if want_loss else 0), **kw)
        return plan, enc, kw

    def __call__(self, inputs, training=False, eps=None, noise=None, copy=True, sample_offset=0):
        """vae/model.py:288-298 -> (x_mean, x_log_scale, z_x, z_mean_x, z_sig_x, y, y_logits, z_prior_mean, z_prior_sig).  sample_offset: row b
        draws its noise as global sample sample_offset + b (the train step's key); 0 keys a row by its place in the batch, as always."""
        B = inputs.shape[0]
        with ops.hold_stream():
            plan, enc, _ = self._forward(inputs, training, eps, noise, False, {"sample_offset": int(sample_offset)} if sample_offset else {})
        self._calls += 1
        o6 = plan.buffer("out6_x", torch.float32, (B, self.H, self.W, 6))
        b = enc.buf
        outs = (o6[..., :3], o6[..., 3:], b["z"], b["zm"], b["zs"], b["y"], b["logits"], b["pm"], b["ps"])
        return tuple(t.clone() for t in outs) if copy else outs

    call = __call__

    def encode(self, inputs, eps=None):
        """vae/model.py:300-304 -> z_x, sampled."""
        return self(inputs, eps=eps)[2]

    def decode(self, z_x, rescale=True):
        """vae/model.py:306-311: decoder_x(z_x); with rescale the mean is mapped to [0,1] (log_scale dropped)."""
        B = z_x.shape[0]
        plan = self.plan(B)
        plan.buffer("zcat", self.dtype, (B, self.global_latent_dims)).copy_(z_x.to(self.dtype))
        with ops.hold_stream():
            plan.step(PHASE_PREP | PHASE_FWD_DECODERS, params=self.flat)
        x_mean = plan.buffer("out6_x", torch.float32, (B, self.H, self.W, 6))[..., :3].clone()
        if rescale:
            return torch.clamp((x_mean + 1) * 0.5, 0., 1.)
        return x_mean

    encode_y = LGGMVae.encode_y                            # vae/model.py:313-315: prior mean / sig of a given y

    def get_y(self, x):
        """vae/model.py:317-319: (y, y_logits) of encoder_x for x [n,H,W,3] (a 6-channel batch uses its x half)."""
        x = x[..., :3]
        out = self(torch.cat([x, x], dim=-1).contiguous())
        return out[5], out[6]


def _check_images(model, images):
    from .trainer import _check_images as check
    check(model, images)


def _images6(images):
    """A 9-channel high_low_pass batch (x | x - low | low, augmentation.py:97-101) as the [B,H,W,6] batch the plan reads: GMVae
    reads channels 0-2 only (vae/model.py:289), so the first six channels carry everything it uses.  The staging marks of
    Augmentator.high_low_pass(..., plan=) move to the copy (its in8_x holds channels 0-2 of this batch).  Any other batch is
    returned as it is."""
    if not torch.is_tensor(images) or images.dim() != 4 or images.shape[-1] != 9:
        return images
    out = images[..., :6].contiguous()
    plan = getattr(images, "_sv_staged_plan", None)
    if plan is not None:
        if images._sv_staged_gen == plan.in8_gen and images._sv_staged_version == images._version:
            out._sv_staged_plan, out._sv_staged_gen, out._sv_staged_version = plan, plan.in8_gen, out._version
        images._sv_staged_plan = None                         # one step per staging
    return out


def _metrics(model, plan, enc, B):
    """x_recon, x_kl, y_kl and the total of vae/trainer.py:184-190 from the per-image terms, as a [4] fp32 device tensor."""
    z = model._zero_terms(B)
    out = model._metrics_buf
    ops.gm_metrics(plan.buffer("nll_x", torch.float32, (B,)), enc.buf["kl2"], z, z, enc.buf["ykl"], model.beta, model.alpha, out)
    return out[_METRIC_IDX].clone()


def train_step_gm_vae(model, images, optimizer, eps=None, noise=None, sample_offset=0):
    """train_step_gm_vae (vae/trainer.py:176-198): total = recon_x + beta * KL(q_x || p_y) + alpha * KL(softmax(y_logits) || uniform);
    gradients of the 34 variables; Adam; returns [x_recon, x_kl, y_kl, total] (GM_LOSS_KEYS) as a device tensor.  `images` [B,H,W,6] fp32
    (or the [B,H,W,9] of high_low_pass: its first six channels)."""
    if not isinstance(model, GMVae):
        raise TypeError("train_step_gm_vae needs a GMVae")
    images = _images6(images)
    _check_images(model, images)
    with ops.hold_stream():
        return _train_step_gm_vae(model, images, optimizer, eps, noise, sample_offset)


def _train_step_gm_vae(model, images, optimizer, eps, noise, sample_offset):
    B = images.shape[0]
    m, v = optimizer.slots(model.flat)
    gm_m, gm_v = optimizer.slots(model.gm_flat)
    lr = optimizer.lr()
    optimizer.iterations += 1
    t = optimizer.iterations
    kw = dict(grads=model.grad_flat, adam_m=m, adam_v=v, sample_offset=sample_offset, lr=lr, beta1=optimizer.beta_1,
              beta2=optimizer.beta_2, adam_eps=optimizer.epsilon, t=t, accumulate_metrics=False)
    plan, enc, kw = model._forward(images, True, eps, noise, True, kw)
    model._calls += 1
    plan.step(PHASE_BWD_DECODERS, **kw)
    model.gm_grad_flat.zero_()
    enc.backward(model.gm_flat, model.gm_grad_flat, plan.buffer("in8_x", model.dtype, (B, model.H, model.W, 8)),
                 plan.buffer("gz_x", torch.float32, (B, model.global_latent_dims)), model.beta, model.alpha)
    metrics = _metrics(model, plan, enc, B)
    plan.step(PHASE_ADAM, **kw)
    ops.adam_step(model.gm_flat, model.gm_grad_flat, gm_m, gm_v, t, lr, optimizer.beta_1, optimizer.beta_2, optimizer.epsilon)
    return metrics


def test_step_gm_vae(model, images, eps=None, noise=None):
    """test_step_gm_vae (vae/trainer.py:277-294): the same loss terms with training=False (no dropout), no update.  Returns the [4]
    metric tensor; the model's y_logits of this batch stay in `model.encoder(B).buf["logits"]` (cluster accuracy)."""
    images = _images6(images)
    _check_images(model, images)
    B = images.shape[0]
    with ops.hold_stream():
        plan, enc, _ = model._forward(images, False, eps, noise, True, {})
        model._calls += 1
        enc.y_kl_only()
        return _metrics(model, plan, enc, B)


test_step_gm_vae.__test__ = False   # not a pytest test


# ---------------------------------------------------------------- cluster accuracy (vae/trainer.py:40-68, :315-349)
def cluster_accuracy(labels, logits):
    """CategoricalAccuracy(labels, linear_assignment(labels, logits)) on the host: every cluster (argmax of a logits row, first index
    on ties) is mapped to the majority class of its members (argmax of the one-hot labels); empty clusters are skipped.  labels
    [N, C] one-hot, logits [N, K]; returns the fraction of rows whose cluster's class is their class."""
    labels, logits = np.asarray(labels), np.asarray(logits)
    n = labels.shape[0]
    if n == 0:
        return 0.0
    counts = np.zeros((logits.shape[1], labels.shape[1]), np.int64)
    np.add.at(counts, (np.argmax(logits, axis=1), np.argmax(labels, axis=1)), 1)
    return accuracy_from_counts(counts, n)


def accuracy_from_counts(counts, n=None):
    """sum_k max_c counts[k][c] / N: a tie between classes changes which class a cluster gets, not how many rows it gets right."""
    counts = np.asarray(counts, np.int64)
    n = int(counts.sum()) if n is None else int(n)
    return float(counts.max(axis=1).sum()) / n if n else 0.0


class ClusterAccuracy:
    """Device-side accumulation of the cluster / class counts over a test set (sv_cluster_confusion per batch), read back once."""

    def __init__(self, y_size, n_classes, device):
        self.counts = torch.zeros((y_size, n_classes), dtype=torch.int32, device=device)

    def update(self, y_logits, labels):
        ops.cluster_confusion(y_logits.contiguous(), labels.to(torch.float32).contiguous(), self.counts)

    def result(self):
        return accuracy_from_counts(self.counts.cpu().numpy())

    def reset_states(self):
        self.counts.zero_()
