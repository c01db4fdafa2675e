"""Host-side mirror of augmentation.py:12-104 (Augmentator) for the SPLIT-VAE path.  ReferenceAugmentator selects every
--augmentation value; Augmentator selects scramble / no_op, as it always has.

Every augmentation runs batched on the device, after batching, instead of per image inside tf.data (vae/main.py:57-61):
`scramble` in sv_scramble_gather, `mix_scramble` in the same gather (one size per pipeline) or sv_scramble_gather_mixed
(opt-in: one size per image), `blur` and `high_low_pass` in the Gaussian filter sv_gauss_blur / sv_high_low_pass.  The
reference's RNG is unseeded; every draw here comes from the counter-based Philox stream keyed by (seed, call index, global
sample index), and explicit parameters (perm=, radius= / std=, sizes=) pin the draws."""
import torch

from . import ops

TYPES = ('scramble', 'mix_scramble', 'blur', 'high_low_pass', 'no_op')     # the values of --augmentation (augmentation.py:15-30)
# Philox draw streams of one Augmentator (the `step` key): a call index per stream, so the streams never share a counter
_PERM, _BLUR, _MIX = 0, 1 << 40, 2 << 40


class Augmentator(object):
    """The SPLIT-VAE path's augmentor: its constructor selects `scramble` and `no_op` (every README command uses scramble) and
    raises NotImplementedError for the other three values, as it always has.  ReferenceAugmentator selects all five; the
    methods (blur, high_low_pass, mix_scramble) are the same on both."""
    SELECTS = ('scramble', 'no_op')

    def __init__(self, type, size=1, mean=0, std=1, seed=0, per_image=False, pipeline=0):
        """type: one of TYPES (those in SELECTS).  size: --patch_size (the scramble patch; the high_low_pass kernel radius, augmentation.py:25).
        mean / std: the high_low_pass kernel's Normal (the reference's callers leave 0 / 1).  per_image: mix_scramble draws a patch
        size per image (the intent of the commented-out augmentation.py:60-64) instead of one per pipeline (what the reference runs).
        pipeline: which mapped pipeline this is (0 train, 1 test): mix_scramble's one size is drawn per pipeline."""
        self.size = size
        self.mean, self.std = float(mean), float(std)
        self.seed = seed
        self.per_image = per_image
        self.pipeline = pipeline
        self.channels = 6
        self._step = 0
        self._mix_size = None
        if type in TYPES and type not in self.SELECTS:
            raise NotImplementedError("Augmentator(%r): Augmentator selects %s; ReferenceAugmentator selects every --augmentation value %s"
                                      % (type, ", ".join(self.SELECTS), TYPES))
        if type == 'scramble':
            self.augment = self.scramble
        elif type == 'mix_scramble':
            self.augment = self.mix_scramble
        elif type == 'blur':
            self.augment = self.blur
        elif type == 'high_low_pass':
            if size < 0 or not self.std > 0:
                raise ValueError("high_low_pass needs size >= 0 and std > 0 (augmentation.py:33-38)")
            self.augment = self.high_low_pass
            self.channels = 9
        elif type == 'no_op':
            self.augment = self.no_op
            self.channels = 3
        else:
            raise ValueError("unknown augmentation type %r" % (type,))
        self.type = type

    # ---------------------------------------------------------------- staging / bookkeeping
    @staticmethod
    def _staged_buffers(plan, single, B, H, W):
        if plan is not None and not single and (plan.desc.B, plan.desc.H, plan.desc.W) == (B, H, W):
            # the training plan's padded input buffers are written by the same kernel: train_step recognises the returned tensor
            # and skips its split / pad pass
            return (plan.buffer("in8_x", plan.dtype, (B, H, W, 8)), plan.buffer("in8_xh", plan.dtype, (B, H, W, 8)))
        return None

    @staticmethod
    def _mark_staged(out, plan):
        # valid for ONE train_step on this plan, and only while nothing else has written the plan's input buffers since
        # (another staged batch, a test_step / encode / visualizer call of the same batch size) and `out` is not edited in place:
        # trainer.train_step checks the generation and the tensor's version counter and falls back to its own split / pad pass
        plan.in8_gen += 1
        out._sv_staged_plan, out._sv_staged_gen, out._sv_staged_version = plan, plan.in8_gen, out._version

    def _draw_step(self, stream):
        step = stream + self._step
        self._step += 1
        return step

    def scramble(self, x, perm=None, sample_offset=0, plan=None):
        """x[B,H,W,3] (or [H,W,3]) fp32 on the device -> concat([x, x_aug], axis=-1).
        perm[B,(H/size)^2] int32 makes the shuffle explicit (the reference draws it from TF's
        unseeded RNG, augmentation.py:49); by default it comes from the counter-based Philox
        stream keyed by (seed, call index, global sample index)."""
        return self._scramble(x, self.size, perm, sample_offset, plan)

    def _scramble(self, x, size, perm, sample_offset, plan):
        single = x.dim() == 3
        if single:
            x = x[None]
            if perm is not None:
                perm = perm[None]
        B, H, W, C = x.shape
        if H != W or H % size:
            raise ValueError("scramble assumes square images and size | H (augmentation.py:44-46)")
        if perm is None:
            perm = ops.random_perm(B, (H // size) * (W // size), self.seed, self._step, sample_offset, x.device)
            self._step += 1
        staged = self._staged_buffers(plan, single, B, H, W)
        out = ops.scramble_gather(x.contiguous(), perm.to(torch.int32).contiguous(), size, staged=staged)
        if staged is not None:
            self._mark_staged(out, plan)
        return out[0] if single else out

    # ---------------------------------------------------------------- device-resident sets (data.ResidentDataset)
    def scramble_from(self, dataset, index, perm=None, sample_offset=0, plan=None):
        """scramble(dataset.gather(index), ...) in one kernel (sv_dataset_gather_scramble): index[B] int32 on the device (or a
        host list, checked and uploaded) names the batch's rows of the resident set; the batch itself never exists in memory.
        Same Philox draws in the same order as scramble(), same staging with plan=."""
        return self._scramble_from(dataset, index, self.size, perm, sample_offset, plan)

    def _scramble_from(self, dataset, index, size, perm, sample_offset, plan):
        if not torch.is_tensor(index):
            index = dataset.upload_index(index)
        B, H, W = index.shape[0], dataset.H, dataset.W
        if H != W or H % size:
            raise ValueError("scramble assumes square images and size | H (augmentation.py:44-46)")
        if perm is None:
            perm = ops.random_perm(B, (H // size) * (W // size), self.seed, self._step, sample_offset, index.device)
            self._step += 1
        staged = self._staged_buffers(plan, False, B, H, W)
        out = ops.dataset_gather_scramble(dataset.data, index, perm.to(torch.int32).contiguous(), size, lut=dataset.lut, staged=staged)
        if staged is not None:
            self._mark_staged(out, plan)
        return out

    def augment_from(self, dataset, index, plan=None):
        """augment(dataset.gather(index)) for the constructor's type: scramble and the one-size-per-pipeline mix_scramble fetch
        and scramble in one kernel; blur, high_low_pass, the per-image mix_scramble and no_op run on the gathered batch."""
        if self.type == 'scramble':
            return self._scramble_from(dataset, index, self.size, None, 0, plan)
        if self.type == 'mix_scramble' and not self.per_image:
            return self._scramble_from(dataset, index, self.mix_size, None, 0, plan)
        if not torch.is_tensor(index):
            index = dataset.upload_index(index)
        x = dataset.gather(index)
        return x if self.type == 'no_op' else self.augment(x, plan=plan)

    # ---------------------------------------------------------------- mix_scramble (augmentation.py:59-81)
    @property
    def mix_size(self):
        """The one patch size of this pipeline.  The reference draws it with np.random.choice when Dataset.map traces
        mix_scramble (augmentation.py:65), i.e. once per mapped pipeline, and prints it; here it is the Philox draw of
        (seed, pipeline), taken on the host at the first call."""
        if self._mix_size is None:
            self._mix_size = ops.mix_size_host(self.seed, _MIX + self.pipeline, 0)
            print('Patch size:', self._mix_size)
            print('Window:', [1, self._mix_size, self._mix_size, 1])
        return self._mix_size

    def mix_scramble(self, x, per_image=None, sizes=None, perm=None, sample_offset=0, plan=None):
        """x[B,H,W,3] (or [H,W,3]) fp32 -> concat([x, x_aug], axis=-1), x_aug scrambled in patches of a size from {1, 2, 4, 8}.
        per_image=False (default: the constructor's choice): one size for the pipeline (mix_size) and the plain scramble gather,
        perm as in scramble().  per_image=True: sizes[B] int32 (explicit, or drawn per image) and perm[B, ld] whose row b permutes
        (H/sizes[b])^2 patches (explicit, or drawn)."""
        per_image = self.per_image if per_image is None else per_image
        if not per_image:
            return self._scramble(x, self.mix_size, perm, sample_offset, plan)
        single = x.dim() == 3
        if single:
            x = x[None]
            perm = None if perm is None else perm[None]
            sizes = None if sizes is None else sizes.reshape(1)
        B, H, W, C = x.shape
        if H != W or H % max(ops.MIX_SIZES):
            raise ValueError("mix_scramble assumes square images whose side the patch sizes 1, 2, 4, 8 divide (augmentation.py:70-75)")
        if sizes is None:
            sizes = ops.mix_sizes(B, self.seed, self._draw_step(_MIX), sample_offset, x.device)
        else:
            s = sizes.detach().cpu()
            if s.shape != (B,) or not all(int(v) > 0 and H % int(v) == 0 for v in s):
                raise ValueError("sizes must be [B] positive divisors of H = %d" % H)
            sizes = sizes.to(device=x.device, dtype=torch.int32).contiguous()
        if perm is None:
            perm = ops.random_perm_mixed(sizes, H, self.seed, self._draw_step(_PERM), sample_offset)
        staged = self._staged_buffers(plan, single, B, H, W)
        out = ops.scramble_gather_mixed(x.contiguous(), perm.to(torch.int32).contiguous(), sizes, staged=staged)
        if staged is not None:
            self._mark_staged(out, plan)
        return out[0] if single else out

    # ---------------------------------------------------------------- gaussian_blur (augmentation.py:83-94)
    def blur(self, x, radius=None, std=None, sample_offset=0, plan=None):
        """x[B,H,W,3] (or [H,W,3]) fp32 -> concat([x, blur(x)], axis=-1).  Per image a radius r ~ U{3..6} and a std ~ U[5,10)
        (augmentation.py:86-87) from the Philox stream, or explicit radius[B] int32 / std[B] fp32 (both or neither)."""
        single = x.dim() == 3
        if single:
            x = x[None]
        B, H, W, C = x.shape
        if (radius is None) != (std is None):
            raise ValueError("pass radius and std together")
        max_radius = ops.BLUR_MAX_RADIUS
        if radius is None:
            radius, std = ops.blur_params(B, self.seed, self._draw_step(_BLUR), sample_offset, x.device)
        else:
            radius = torch.as_tensor(radius, dtype=torch.int32).reshape(B)
            std = torch.as_tensor(std, dtype=torch.float32).reshape(B)
            r = radius.cpu()
            if int(r.min()) < 0:
                raise ValueError("blur radius must be >= 0")
            max_radius = int(r.max())
            radius, std = radius.to(x.device).contiguous(), std.to(x.device).contiguous()
        if H != W or max_radius > H:
            raise ValueError("blur assumes square images and a radius <= H (SYMMETRIC padding, augmentation.py:91-92)")
        staged = self._staged_buffers(plan, single, B, H, W)
        out = ops.gauss_blur(x.contiguous(), radius, std, max_radius, staged=staged)
        if staged is not None:
            self._mark_staged(out, plan)
        return out[0] if single else out

    gaussian_blur = blur

    # ---------------------------------------------------------------- high_low_pass (augmentation.py:97-101)
    def high_low_pass(self, x, plan=None):
        """x[B,H,W,3] (or [H,W,3]) fp32 -> concat([x, x - low, low], axis=-1), low = x filtered by the fixed Gaussian of radius
        `size`, Normal(mean, std) (augmentation.py:23-28).  With plan= the plan's in8_x / in8_xh get channels 0-2 and 3-5."""
        single = x.dim() == 3
        if single:
            x = x[None]
        B, H, W, C = x.shape
        if H != W or self.size > H:
            raise ValueError("high_low_pass assumes square images and size <= H (SYMMETRIC padding, augmentation.py:28)")
        staged = self._staged_buffers(plan, single, B, H, W)
        out = ops.high_low_pass(x.contiguous(), self.size, self.mean, self.std, staged=staged)
        if staged is not None:
            self._mark_staged(out, plan)
        return out[0] if single else out

    def no_op(self, x):
        return x


class ReferenceAugmentator(Augmentator):
    """Augmentator (augmentation.py:12-30) selecting every value of --augmentation: scramble, mix_scramble, blur, high_low_pass,
    no_op.  The CLIs (main.make_augmentors) build this one."""
    SELECTS = TYPES
