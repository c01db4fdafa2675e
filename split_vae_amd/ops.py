"""Tensor-level wrappers over the C ABI (include/splitvae.h).

torch is plumbing only: it owns device memory and the HIP stream; every computation below is a
call into libsplitvae_hip.so with raw pointers.  All tensors must live on a HIP device.
"""
import ctypes as C

import torch

from . import _lib
from ._lib import SV_BF16, SV_F32, ConvDesc, LGVaeDesc, StepArgs, check

_TORCH_DT = {SV_BF16: torch.bfloat16, SV_F32: torch.float32}
_SV_DT = {torch.bfloat16: SV_BF16, torch.float32: SV_F32}


def sv_dtype(dt):
    if isinstance(dt, str):
        dt = {"bf16": torch.bfloat16, "bfloat16": torch.bfloat16, "f32": torch.float32, "fp32": torch.float32,
              "float32": torch.float32}[dt]
    if isinstance(dt, int):
        return dt
    return _SV_DT[dt]


_STREAM_HOLD = []      # hold_stream(): the stream handle of the enclosing step (torch's lookup is ~9 us, ~75 of them per GM step)


def _stream():
    if _STREAM_HOLD:
        return _STREAM_HOLD[-1]
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class hold_stream:
    """`with ops.hold_stream():` -- every op inside launches on the stream that was current at entry."""

    def __enter__(self):
        _STREAM_HOLD.append(C.c_void_p(torch.cuda.current_stream().cuda_stream))

    def __exit__(self, *exc):
        _STREAM_HOLD.pop()
        return False


def _p(t):
    if t is None:
        return None
    assert t.is_cuda, "split_vae_amd ops need device tensors (HIP); got a CPU tensor"
    assert t.is_contiguous()
    return C.c_void_p(t.data_ptr())


def _workspace(nbytes, workspace, device):
    """The caller's scratch tensor, or a fresh one of nbytes: a contiguous uint8 device tensor with any contents (the library checks its size)."""
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=device) if workspace is None else workspace
    if ws.dtype != torch.uint8 or not ws.is_cuda or not ws.is_contiguous():
        raise ValueError("workspace must be a contiguous uint8 device tensor")
    return ws


# ------------------------------------------------------------------ A1 scramble (augmentation.py:43-57)
def random_perm(B, n_patch, seed, step=0, sample_offset=0, device="cuda", out=None):
    """out: an int32 buffer of at least B * n_patch elements to write instead of a fresh one (the rest of it is not touched)"""
    perm = torch.empty((B, n_patch), dtype=torch.int32, device=device) if out is None else out
    check(_lib.load().sv_random_perm(_p(perm), B, n_patch, seed, step, sample_offset, _stream()), "sv_random_perm")
    return perm


def scramble_gather(x, perm, patch, staged=None, out=None):
    """x[B,H,W,3] fp32, perm[B,(H/patch)^2] int32 -> [B,H,W,6] = concat([x, x_aug], axis=-1).  out: a float32 buffer of at least
    B*H*W*6 elements to write instead of a fresh one."""
    B, H, W, Cc = x.shape
    assert Cc == 3 and x.dtype == torch.float32 and perm.dtype == torch.int32
    assert perm.shape == (B, (H // patch) * (W // patch))
    if out is None:
        out = torch.empty((B, H, W, 6), dtype=torch.float32, device=x.device)
    assert out.dtype == torch.float32 and out.numel() >= B * H * W * 6
    if staged is not None:                       # (x8, xh8): a plan's in8_x / in8_xh buffers, filled in the same pass
        x8, xh8 = staged
        assert x8.numel() >= B * H * W * 8 and xh8.numel() >= B * H * W * 8 and x8.dtype == xh8.dtype
        check(_lib.load().sv_scramble_gather_staged(_p(x), _p(perm), _p(out), _p(x8), _p(xh8), sv_dtype(x8.dtype), B, H, W, patch,
                                                    _stream()), "sv_scramble_gather_staged")
        return out
    check(_lib.load().sv_scramble_gather(_p(x), _p(perm), _p(out), B, H, W, patch, _stream()), "sv_scramble_gather")
    return out


# ------------------------------------------------------------------ A1b blur / high-low pass / mixed scramble (augmentation.py:33-41,59-101)
MIX_SIZES = (1, 2, 4, 8)           # augmentation.py:41
BLUR_MAX_RADIUS = 6                # augmentation.py:87: tf.random.uniform(int32, minval=3, maxval=7)


def _staged_args(staged, B, H, W):
    x8, xh8 = staged
    assert x8.shape == (B, H, W, 8) and xh8.shape == (B, H, W, 8) and x8.dtype == xh8.dtype
    return _p(x8), _p(xh8), sv_dtype(x8.dtype)


def blur_params(B, seed, step=0, sample_offset=0, device="cuda"):
    """(radius[B] int32, std[B] fp32) of gaussian_blur (augmentation.py:86-87) from the Philox stream."""
    radius = torch.empty((B,), dtype=torch.int32, device=device)
    std = torch.empty((B,), dtype=torch.float32, device=device)
    check(_lib.load().sv_blur_params(_p(radius), _p(std), B, seed, step, sample_offset, _stream()), "sv_blur_params")
    return radius, std


def gauss_blur(x, radius, std, max_radius=BLUR_MAX_RADIUS, staged=None):
    """x[B,H,W,3] fp32, radius[B] int32, std[B] fp32 -> [B,H,W,6] = concat([x, blur(x)], axis=-1) (augmentation.py:83-94)."""
    B, H, W, Cc = x.shape
    assert Cc == 3 and x.dtype == torch.float32 and radius.dtype == torch.int32 and std.dtype == torch.float32
    assert radius.shape == (B,) and std.shape == (B,)
    out = torch.empty((B, H, W, 6), dtype=torch.float32, device=x.device)
    if staged is not None:
        x8, xh8, dt = _staged_args(staged, B, H, W)
        check(_lib.load().sv_gauss_blur_staged(_p(x), _p(radius), _p(std), _p(out), x8, xh8, dt, B, H, W, max_radius, _stream()),
              "sv_gauss_blur_staged")
        return out
    check(_lib.load().sv_gauss_blur(_p(x), _p(radius), _p(std), _p(out), B, H, W, max_radius, _stream()), "sv_gauss_blur")
    return out


def high_low_pass(x, size, mean=0.0, std=1.0, staged=None):
    """x[B,H,W,3] fp32 -> [B,H,W,9] = concat([x, x - low, low], axis=-1), low the Gaussian of radius `size` (augmentation.py:97-101)."""
    B, H, W, Cc = x.shape
    assert Cc == 3 and x.dtype == torch.float32
    out = torch.empty((B, H, W, 9), dtype=torch.float32, device=x.device)
    if staged is not None:
        x8, xh8, dt = _staged_args(staged, B, H, W)
        check(_lib.load().sv_high_low_pass_staged(_p(x), _p(out), x8, xh8, dt, B, H, W, size, mean, std, _stream()),
              "sv_high_low_pass_staged")
        return out
    check(_lib.load().sv_high_low_pass(_p(x), _p(out), B, H, W, size, mean, std, _stream()), "sv_high_low_pass")
    return out


def mix_sizes(B, seed, step=0, sample_offset=0, device="cuda"):
    """sizes[B] int32 in {1, 2, 4, 8} (augmentation.py:40-41), one per image, from the Philox stream."""
    sizes = torch.empty((B,), dtype=torch.int32, device=device)
    check(_lib.load().sv_mix_sizes(_p(sizes), B, seed, step, sample_offset, _stream()), "sv_mix_sizes")
    return sizes


def mix_size_host(seed, step=0, sample=0):
    """The same draw on the host (no device): one patch size for a whole pipeline."""
    return int(_lib.load().sv_mix_size_host(seed, step, sample))


def random_perm_mixed(sizes, H, seed, step=0, sample_offset=0, ld=None):
    """perm[B, ld] int32: row b permutes the (H/sizes[b])^2 patches of image b (the rest of the row is -1); ld defaults to
    (H / min size)^2."""
    B = sizes.shape[0]
    if ld is None:
        ld = (H // min(MIX_SIZES)) ** 2
    perm = torch.full((B, ld), -1, dtype=torch.int32, device=sizes.device)
    check(_lib.load().sv_random_perm_mixed(_p(perm), _p(sizes), B, H, ld, seed, step, sample_offset, _stream()), "sv_random_perm_mixed")
    return perm


def scramble_gather_mixed(x, perm, sizes, staged=None):
    """x[B,H,W,3] fp32, perm[B,ld] int32 (row b: a permutation of (H/sizes[b])^2 patches), sizes[B] int32 -> [B,H,W,6]."""
    B, H, W, Cc = x.shape
    assert Cc == 3 and x.dtype == torch.float32 and perm.dtype == torch.int32 and sizes.dtype == torch.int32
    assert perm.dim() == 2 and perm.shape[0] == B and sizes.shape == (B,)
    ld = perm.shape[1]
    out = torch.empty((B, H, W, 6), dtype=torch.float32, device=x.device)
    if staged is not None:
        x8, xh8, dt = _staged_args(staged, B, H, W)
        check(_lib.load().sv_scramble_gather_mixed_staged(_p(x), _p(perm), _p(sizes), ld, _p(out), x8, xh8, dt, B, H, W, _stream()),
              "sv_scramble_gather_mixed_staged")
        return out
    check(_lib.load().sv_scramble_gather_mixed(_p(x), _p(perm), _p(sizes), ld, _p(out), B, H, W, _stream()), "sv_scramble_gather_mixed")
    return out


# ------------------------------------------------------------------ A1d device-resident datasets (vae/main.py:56-61 on the device)
_SRC_DT = {torch.uint8: _lib.SV_SRC_U8, torch.float32: _lib.SV_SRC_F32}


def _dataset_args(src, lut, index):
    N, H, W, Cc = src.shape
    assert Cc == 3 and src.dtype in _SRC_DT and index.dtype == torch.int32 and index.dim() == 1
    if src.dtype == torch.uint8:
        assert lut is not None and lut.dtype == torch.float32 and lut.shape == (256,)
    return N, H, W, index.shape[0], _SRC_DT[src.dtype]


def dataset_gather(src, index, lut=None):
    """src[N,H,W,3] uint8 or fp32 (the resident set), index[B] int32, lut[256] fp32 (uint8 sources: the value of each level)
    -> x[B,H,W,3] fp32 = value(src[index])."""
    N, H, W, B, sdt = _dataset_args(src, lut, index)
    x = torch.empty((B, H, W, 3), dtype=torch.float32, device=src.device)
    check(_lib.load().sv_dataset_gather(_p(src), sdt, _p(lut), _p(index), _p(x), N, B, H, W, _stream()), "sv_dataset_gather")
    return x


def dataset_gather_scramble(src, index, perm, patch, lut=None, staged=None):
    """dataset_gather followed by scramble_gather(..., staged=) in one kernel -> [B,H,W,6] = concat([x, x_aug], axis=-1)."""
    N, H, W, B, sdt = _dataset_args(src, lut, index)
    assert perm.dtype == torch.int32 and perm.shape == (B, (H // patch) * (W // patch))
    out = torch.empty((B, H, W, 6), dtype=torch.float32, device=src.device)
    x8, xh8, dt = (None, None, SV_F32) if staged is None else _staged_args(staged, B, H, W)
    check(_lib.load().sv_dataset_gather_scramble(_p(src), sdt, _p(lut), _p(index), _p(perm), _p(out), x8, xh8, dt, N, B, H, W, patch,
                                                 _stream()), "sv_dataset_gather_scramble")
    return out


def dataset_onehot(labels, index, depth=10):
    """labels[N] uint8 (resident), index[B] int32 -> [B,depth] fp32 = one_hot(labels[index] - 1) (data.one_hot_svhn)."""
    assert labels.dtype == torch.uint8 and labels.dim() == 1 and index.dtype == torch.int32 and index.dim() == 1
    B = index.shape[0]
    out = torch.empty((B, depth), dtype=torch.float32, device=labels.device)
    check(_lib.load().sv_dataset_onehot(_p(labels), _p(index), _p(out), labels.shape[0], B, depth, _stream()), "sv_dataset_onehot")
    return out


# ------------------------------------------------------------------ A1c Multi-Bird canvases (spair/data.py:39-174)
MULTIBIRD_LAYOUT_WORDS = C.sizeof(_lib.MultibirdLayout) // 4


def multibird_layout_host(bg, n_sprites, seed, split, sample, out=None):
    """The layout of canvas `sample` of `split` by the sequential host loop (no device) -> _lib.MultibirdLayout."""
    L = _lib.MultibirdLayout() if out is None else out
    check(_lib.load().sv_multibird_layout_host(C.addressof(L), bg, n_sprites, seed, split, sample), "sv_multibird_layout_host")
    return L


def _mb_index(index, B):
    if index is not None:
        assert index.dtype == torch.int64 and index.shape == (B,)
    return _p(index)


def multibird_layouts(B, bg, n_sprites, seed, split, sample_offset=0, index=None, device="cuda"):
    """int32 [B, 20]: sv_multibird_layout records (word 19 is the fp32 angle) of samples index[b] or sample_offset + b."""
    out = torch.empty((B, MULTIBIRD_LAYOUT_WORDS), dtype=torch.int32, device=device)
    check(_lib.load().sv_multibird_layouts(_p(out), _mb_index(index, B), bg, n_sprites, B, seed, split, sample_offset, _stream()),
          "sv_multibird_layouts")
    return out


def multibird_canvases(sprites, bg, B, seed, split, sample_offset=0, index=None, layouts=None, x=None, count=None):
    """sprites uint8 [n,14,14,3] on the device -> (x [B,48,48,3] fp32, count [B] fp32).  layouts (int32 [B,20]) pins the draws."""
    assert sprites.dtype == torch.uint8 and sprites.shape[1:] == (14, 14, 3)
    if x is None:
        x = torch.empty((B, 48, 48, 3), dtype=torch.float32, device=sprites.device)
    if count is None:
        count = torch.empty((B,), dtype=torch.float32, device=sprites.device)
    assert x.shape == (B, 48, 48, 3) and x.dtype == torch.float32 and count.shape == (B,) and count.dtype == torch.float32
    if layouts is not None:
        assert layouts.dtype == torch.int32 and layouts.shape == (B, MULTIBIRD_LAYOUT_WORDS)
    check(_lib.load().sv_multibird_canvases(_p(x), _p(count), _p(sprites), sprites.shape[0], _mb_index(index, B), _p(layouts), bg, B,
                                            seed, split, sample_offset, _stream()), "sv_multibird_canvases")
    return x, count


# ------------------------------------------------------------------ A6 discretised logistic (vae/trainer.py:21-38)
def dlogistic_nll(images6, ch_off, out6, grad_dtype=None, grad_scale=1.0, nll=None, grad=None, ws=None):
    """nll / grad / ws: buffers to write instead of fresh ones (at least B, B*H*W*8 and sv_dlogistic_nll_workspace_bytes / 4 elements)"""
    B, H, W, _ = images6.shape
    lib = _lib.load()
    if nll is None:
        nll = torch.empty((B,), dtype=torch.float32, device=images6.device)
    if ws is None:
        ws = torch.empty((lib.sv_dlogistic_nll_workspace_bytes(B, H, W) // 4,), dtype=torch.float32, device=images6.device)
    gdt = 0
    if grad is not None:
        gdt = sv_dtype(grad.dtype)
        assert grad.numel() >= B * H * W * 8
    elif grad_dtype is not None:
        gdt = sv_dtype(grad_dtype)
        grad = torch.empty((B, H, W, 8), dtype=_TORCH_DT[gdt], device=images6.device)
    check(lib.sv_dlogistic_nll(_p(images6), ch_off, _p(out6), _p(nll), _p(grad), gdt, grad_scale, B, H, W, _p(ws),
                               _stream()), "sv_dlogistic_nll")
    return nll, grad


def dlogistic_nll_twin(images6, out6, nll, ws, grad=None, grad_scale=1.0):
    """sv_dlogistic_nll_twin: the x and x-hat reconstructions in one launch.  out6 [2, B, H, W, 6], nll [2, >= B], ws [2, >= workspace floats]
    and grad [2, >= B*H*W*8] (or None) hold network e at index e of their first axis; its stride is what the call passes."""
    B, H, W, _ = images6.shape
    for t in (out6, nll, ws) + (() if grad is None else (grad,)):
        assert t.shape[0] == 2 and t[0].is_contiguous()
    check(_lib.load().sv_dlogistic_nll_twin(_p(images6), _pany(out6), out6.stride(0), _pany(nll), nll.stride(0), _pany(grad),
                                            0 if grad is None else grad.stride(0), 0 if grad is None else sv_dtype(grad.dtype), grad_scale,
                                            B, H, W, _pany(ws), ws.stride(0), _stream()), "sv_dlogistic_nll_twin")


def dlogistic_nll_workspace_floats(B, H, W):
    return _lib.load().sv_dlogistic_nll_workspace_bytes(B, H, W) // 4


def finalize_losses(nll_x, beta, losses, nll_xh=None, kl_x=None, kl_xh=None, part_x=None, part_xh=None, P=0, metric_acc=None, accumulate=False,
                    B=None):
    """sv_finalize_losses: per-image terms [B] -> losses[6] (and the running sums metric_acc[6]); with part_x [B, P] (part_xh) the per-image
    NLL sums are formed here from the partials and written to nll_x (nll_xh).  B defaults to nll_x.numel()."""
    B = nll_x.numel() if B is None else B
    check(_lib.load().sv_finalize_losses(_pany(nll_x), _pany(nll_xh), _pany(kl_x), _pany(kl_xh), _pany(part_x), _pany(part_xh), P, B,
                                         float(beta), _pany(losses), _pany(metric_acc), int(bool(accumulate)), _stream()), "sv_finalize_losses")


# ------------------------------------------------------------------ A4/A7 reparam + KL
def reparam_kl_fwd(pre, bias, eps=None, z_dtype=torch.bfloat16, seed=0, step=0, stream_id=0, sample_offset=0, out=None):
    """out: (z_mean, z_sig, z, z_lp, kl, eps_out) buffers to write instead of fresh ones: at least [B, L] ([B] for kl), z_lp in z_dtype"""
    B, L2 = pre.shape
    L = L2 // 2
    dev = pre.device
    if out is not None:
        z_mean, z_sig, z, z_lp, kl, eps_out = out
        assert z_lp.dtype == z_dtype and min(t.numel() for t in (z_mean, z_sig, z, z_lp, eps_out)) >= B * L and kl.numel() >= B
    else:
        z_mean = torch.empty((B, L), dtype=torch.float32, device=dev)
        z_sig = torch.empty_like(z_mean)
        z = torch.empty_like(z_mean)
        eps_out = torch.empty_like(z_mean)
        kl = torch.empty((B,), dtype=torch.float32, device=dev)
        z_lp = torch.empty((B, L), dtype=z_dtype, device=dev)
    check(_lib.load().sv_reparam_kl_fwd(_p(pre), _p(bias), _p(eps), _p(eps_out), _p(z_mean), _p(z_sig), _p(z),
                                        _p(z_lp), sv_dtype(z_dtype), L, 0, _p(kl), B, L, seed, step, stream_id,
                                        sample_offset, _stream()), "sv_reparam_kl_fwd")
    return z_mean, z_sig, z, z_lp, kl, eps_out


def reparam_kl_bwd(dz, z_mean, z_sig, eps, kl_scale, g_dtype=torch.bfloat16, dz2=None, out=None):
    """out: a g_dtype buffer of at least B * 2L elements to write instead of a fresh one"""
    B, L = z_mean.shape
    g = torch.empty((B, 2 * L), dtype=g_dtype, device=dz.device) if out is None else out
    assert g.dtype == g_dtype and g.numel() >= B * 2 * L
    check(_lib.load().sv_reparam_kl_bwd(_p(dz), dz.shape[1], _p(dz2), 0 if dz2 is None else dz2.shape[1],
                                        _p(z_mean), _p(z_sig), _p(eps), kl_scale, _p(g), sv_dtype(g_dtype), B, L,
                                        _stream()), "sv_reparam_kl_bwd")
    return g


# ------------------------------------------------------------------ K14 Keras Adam (vae/main.py:65)
def adam_step(p, g, m, v, t, lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-7, grad_scale=1.0, n=None):
    """n: the number of elements to update (default: all of p)"""
    check(_lib.load().sv_adam_step(_pany(p), _pany(g), _pany(m), _pany(v), p.numel() if n is None else n, lr, beta1, beta2, eps, t, grad_scale,
                                   _stream()), "sv_adam_step")


# ------------------------------------------------------------------ K10a bilinear 2x (vae/model.py:163-167)
def upsample2x_fwd(x, out=None):
    B, H, W, Cc = x.shape
    if out is None:
        out = torch.empty((B, 2 * H, 2 * W, Cc), dtype=x.dtype, device=x.device)
    assert out.dtype == x.dtype and out.numel() >= 4 * x.numel()
    check(_lib.load().sv_upsample2x_fwd(_p(x), _p(out), sv_dtype(x.dtype), B, H, W, Cc, _stream()), "sv_upsample2x_fwd")
    return out


def upsample2x_bwd(g_hi, y_lo_mask=None, out=None):
    B, H2, W2, Cc = g_hi.shape
    if out is None:
        out = torch.empty((B, H2 // 2, W2 // 2, Cc), dtype=g_hi.dtype, device=g_hi.device)
    assert out.dtype == g_hi.dtype and out.numel() * 4 >= g_hi.numel()
    check(_lib.load().sv_upsample2x_bwd(_p(g_hi), _p(y_lo_mask), _p(out), sv_dtype(g_hi.dtype), B, H2 // 2, W2 // 2,
                                        Cc, _stream()), "sv_upsample2x_bwd")
    return out


# ------------------------------------------------------------------ SPLIT-SPAIR spatial transformer (spair/utils.py:119-330)
def stn_sample(img, z_where, Ho, Wo, inverse=False):
    """STN.call: img [B,H,W,C] (inverse: [B,B',H,W,C]) fp32, z_where [B,Hc,Wc,4] -> (out [B,B',Ho,Wo,C], obj_bbox_mask [B,B',4])."""
    B, Hc, Wc, _ = z_where.shape
    H, W, Cc = img.shape[-3:]
    assert img.dtype == torch.float32 and z_where.dtype == torch.float32
    assert tuple(img.shape[:-3]) == ((B, Hc * Wc) if inverse else (B,))
    out = torch.empty((B, Hc * Wc, Ho, Wo, Cc), dtype=torch.float32, device=img.device)
    bbox = torch.empty((B, Hc * Wc, 4), dtype=torch.float32, device=img.device)
    check(_lib.load().sv_stn_sample_fwd(_p(img.contiguous()), _p(z_where.contiguous()), _p(out), _p(bbox), B, Hc, Wc, H, W, Cc, Ho, Wo,
                                        1 if inverse else 0, _stream()), "sv_stn_sample_fwd")
    return out, bbox


def stn_sample_bwd(img, z_where, g_out, inverse=False, need_img=True):
    """-> (g_img like img | None, g_z_where like z_where) for the upstream gradient g_out [B,B',Ho,Wo,C]."""
    B, Hc, Wc, _ = z_where.shape
    H, W, Cc = img.shape[-3:]
    Ho, Wo = g_out.shape[2:4]
    lib = _lib.load()
    g_img = None
    if need_img:
        g_img = torch.empty_like(img) if lib.sv_stn_bwd_overwrites(H, W, Cc, 1 if inverse else 0) else torch.zeros_like(img)
    g_z = torch.empty_like(z_where)
    check(_lib.load().sv_stn_sample_bwd(_p(img.contiguous()), _p(z_where.contiguous()), _p(g_out.contiguous()), _p(g_img), _p(g_z), B, Hc,
                                        Wc, H, W, Cc, Ho, Wo, 1 if inverse else 0, _stream()), "sv_stn_sample_bwd")
    return g_img, g_z


def spair_render(obj, bg, z_depth, z_pres=None, z_pres_logits=None, training=False, noise=None):
    """Renderer.call (spair/spair.py:534-579): obj [B,B',H,W,C+1], bg [B,H,W,C], z_* [B,Hc,Wc,1] -> canvas [B,H,W,C]."""
    B, Bp, H, W, C1 = obj.shape
    out = torch.empty((B, H, W, C1 - 1), dtype=torch.float32, device=obj.device)
    f = lambda t: None if t is None else t.reshape(B, Bp).contiguous()
    check(_lib.load().sv_spair_render_fwd(_p(obj.contiguous()), _p(bg.contiguous()), _p(f(z_depth)), _p(f(z_pres)), _p(f(z_pres_logits)),
                                          _p(None if noise is None else noise.contiguous()), _p(out), B, Bp, H, W, C1 - 1,
                                          1 if training else 0, _stream()), "sv_spair_render_fwd")
    return out


def spair_render_bwd(obj, bg, z_depth, z_pres, g_out, noise=None):
    """-> (g_obj, g_bg, g_z_pres [B,B'], g_z_depth [B,B']) of the training-form renderer."""
    B, Bp, H, W, C1 = obj.shape
    g_obj, g_bg = torch.empty_like(obj), torch.empty_like(bg)
    g_zp = torch.empty((B, Bp), dtype=torch.float32, device=obj.device)
    g_zd = torch.empty_like(g_zp)
    f = lambda t: t.reshape(B, Bp).contiguous()
    lib = _lib.load()
    n = lib.sv_spair_render_bwd_workspace_floats(B, H, W)
    ws = torch.empty((n,), dtype=torch.float32, device=obj.device)
    check(lib.sv_spair_render_bwd_ws(_p(obj.contiguous()), _p(bg.contiguous()), _p(f(z_depth)), _p(f(z_pres)),
                                     _p(None if noise is None else noise.contiguous()), _p(g_out.contiguous()), _p(g_obj), _p(g_bg),
                                     _p(g_zp), _p(g_zd), B, Bp, H, W, C1 - 1, _p(ws), n, _stream()), "sv_spair_render_bwd_ws")
    return g_obj, g_bg, g_zp, g_zd


def _dev_scalar(v):
    """(python float, device pointer | None): a scalar given as a 1-element fp32 device tensor is read by the kernel at run
    time (hipGraph replays see its current value)."""
    if torch.is_tensor(v):
        assert v.dtype == torch.float32 and v.numel() == 1 and v.is_cuda
        return 0.0, v
    return float(v), None


def spair_zpres_kl(z_pres, z_pres_logits, z_pres_pre_sigmoid, prior_prob, temperature, grad_scale=None):
    """compute_z_pres_kl_yolo_air (spair/trainer.py:45-94): inputs [B,H,W,1] -> (kl [B] per-image sums, g_pre_sigmoid, g_logits)
    with the gradients of mean_b(kl_b) (grad_scale = 1/B) unless grad_scale is given."""
    B = z_pres.shape[0]
    n = z_pres[0].numel()
    f = lambda t: t.reshape(B, n).contiguous()
    kl = torch.empty((B,), dtype=torch.float32, device=z_pres.device)
    g_pre, g_log = torch.empty((B, n), dtype=torch.float32, device=z_pres.device), torch.empty((B, n), dtype=torch.float32, device=z_pres.device)
    pp, pp_dev = _dev_scalar(prior_prob)
    check(_lib.load().sv_spair_zpres_kl_dyn(_p(f(z_pres)), _p(f(z_pres_logits)), _p(f(z_pres_pre_sigmoid)), _p(kl), _p(g_pre), _p(g_log), B, n,
                                            pp, _p(pp_dev), float(temperature), 1.0 / B if grad_scale is None else float(grad_scale),
                                            _stream()), "sv_spair_zpres_kl")
    return kl, g_pre.reshape(z_pres.shape), g_log.reshape(z_pres.shape)


def adam_step_clipnorm_tensors(p, grads, m, v, tensor_off, clipnorm, t, lr, beta1=0.9, beta2=0.999, eps=1e-7, grad_scale=1.0, alpha_dev=None):
    """adam_step_clipnorm over a LIST of gradient tensors (one per variable, contiguous fp32, in tensor_off order): their
    addresses go to the kernels by value -- no flat copy."""
    nt = tensor_off.numel() - 1
    assert len(grads) == nt and nt <= 128
    arr = (C.c_void_p * nt)(*[g.data_ptr() for g in grads])
    ws = torch.empty((256 * nt,), dtype=torch.float32, device=p.device)
    check(_lib.load().sv_adam_step_clipnorm_ptrs(_p(p), arr, _p(m), _p(v), _p(tensor_off), nt, _p(ws), float(clipnorm), float(lr),
                                                 float(beta1), float(beta2), float(eps), int(t), _p(alpha_dev), float(grad_scale),
                                                 _stream()), "sv_adam_step_clipnorm_ptrs")


SPAIR_LOSS_MODES = {"xent": 0, "kl": 1, "kl_prior": 2}


def spair_loss(mode, a, b, prior_mean=0.0, prior_sig=1.0, grads=True):
    """Per-image loss sums of spair/trainer.py (xent_loss / kl_divergence / kl_divergence_two_gauss vs a constant prior) over
    a, b [B, ...] fp32 -> (sums [B], ga | None, gb | None) with the per-element derivatives (xent: gb only)."""
    B = a.shape[0]
    n = a[0].numel()
    a2, b2 = a.reshape(B, n).contiguous(), b.reshape(B, n).contiguous()
    sums = torch.empty((B,), dtype=torch.float32, device=a.device)
    ga = torch.empty_like(a2) if grads and mode != "xent" else None
    gb = torch.empty_like(b2) if grads else None
    pm, pm_dev = _dev_scalar(prior_mean)
    check(_lib.load().sv_spair_loss_dyn(SPAIR_LOSS_MODES[mode], _p(a2), _p(b2), _p(sums), _p(ga), _p(gb), B, n, pm, _p(pm_dev),
                                        float(prior_sig), _stream()), "sv_spair_loss")
    return sums, (None if ga is None else ga.reshape(a.shape)), (None if gb is None else gb.reshape(b.shape))


# ------------------------------------------------------------------ SPAIR evaluation (spair/trainer.py:294-301, spair/visualizer.py:107-111)
def draw_bounding_boxes(images, boxes, colors, gate=None, out=None):
    """tf.image.draw_bounding_boxes: images [B,H,W,C] fp32 (C in 1, 3, 4), boxes [B,NB,4] = (ymin, xmin, ymax, xmax) in [0,1],
    colors [NC,ldc] fp32 with ldc >= C, gate [B,NB] (optional: the boxes are multiplied by it) -> out [B,H,W,C]: a new tensor, or
    `out` (which may be `images` itself)."""
    B, H, W, Cc = images.shape
    NB = boxes.shape[1]
    assert images.dtype == boxes.dtype == colors.dtype == torch.float32 and colors.dim() == 2
    assert tuple(boxes.shape) == (B, NB, 4) and (gate is None or (gate.dtype == torch.float32 and gate.numel() == B * NB))
    if out is None:
        out = torch.empty_like(images)
    assert out.shape == images.shape and out.dtype == torch.float32
    check(_lib.load().sv_draw_bounding_boxes(_p(images), _p(boxes), _p(gate), _p(colors), _p(out), B, H, W, Cc, NB, colors.shape[0],
                                             colors.shape[1], _stream()), "sv_draw_bounding_boxes")
    return out


def spair_count_metrics(z_pres_logits, labels, acc=None, want_pred=False):
    """The count metrics of test_step: z_pres_logits [B, ...] (an image's cells contiguous, images at any row pitch), labels [B] ->
    (metrics [2] = (MAE, MAPE) of the batch, pred [B] | None).  acc: int32 [2] device counters (matches, images seen) to add to."""
    B = z_pres_logits.shape[0]
    lg = z_pres_logits.reshape(B, -1)
    if lg.stride(1) != 1 or lg.data_ptr() % 4:
        lg = lg.contiguous()
    assert lg.dtype == torch.float32 and lg.is_cuda
    lab = labels.reshape(-1).to(device=lg.device, dtype=torch.float32).contiguous()
    assert lab.numel() == B and (acc is None or (acc.dtype == torch.int32 and acc.numel() == 2))
    metrics = torch.empty((2,), dtype=torch.float32, device=lg.device)
    pred = torch.empty((B,), dtype=torch.float32, device=lg.device) if want_pred else None
    check(_lib.load().sv_spair_count_metrics(C.c_void_p(lg.data_ptr()), lg.stride(0), _p(lab), _p(pred), _p(metrics), _p(acc), B,
                                             lg.shape[1], _stream()), "sv_spair_count_metrics")
    return metrics, pred


# ------------------------------------------------------------------ detection average precision (csrc/detect_ap.hip)
DETECT_AP_THRESHOLDS = 9           # IoU 0.1 .. 0.9
DETECT_AP_MAX_CELLS, DETECT_AP_MAX_RECORDS, DETECT_AP_OUT = 64, 1 << 20, 29
DETECT_NONDET = 0xFFFFFFFF         # high word of a non-detection's key


def _np_ptr(a):
    return C.c_void_p(a.ctypes.data)


def sprite_extents_host(bank):
    """uint8 [n,14,14,3] NumPy bank -> int32 [n,4] (r0, c0, r1, c1), -1 for an empty sprite (sv_sprite_extents_host; no device)."""
    import numpy as np
    bank = np.ascontiguousarray(bank, np.uint8)
    assert bank.ndim == 4 and bank.shape[1:] == (14, 14, 3)
    out = np.empty((bank.shape[0], 4), np.int32)
    check(_lib.load().sv_sprite_extents_host(_np_ptr(bank), bank.shape[0], _np_ptr(out)), "sv_sprite_extents_host")
    return out


def sprite_extents(bank):
    """uint8 [n,14,14,3] device bank -> int32 [n,4] on its device (sv_sprite_extents)."""
    assert bank.dtype == torch.uint8 and bank.dim() == 4 and tuple(bank.shape[1:]) == (14, 14, 3)
    out = torch.empty((bank.shape[0], 4), dtype=torch.int32, device=bank.device)
    check(_lib.load().sv_sprite_extents(_p(bank), bank.shape[0], _p(out), _stream()), "sv_sprite_extents")
    return out


def multibird_gt_boxes_host(layouts, extents):
    """layouts: structured array / int32 [B,20] NumPy, extents int32 [n,4] -> (boxes [B,5,4] fp32, n_gt [B] int32); no device."""
    import numpy as np
    lay = np.ascontiguousarray(layouts).view("<i4").reshape(-1, MULTIBIRD_LAYOUT_WORDS)
    ext = np.ascontiguousarray(extents, np.int32)
    B = lay.shape[0]
    boxes, n_gt = np.empty((B, 5, 4), np.float32), np.empty((B,), np.int32)
    check(_lib.load().sv_multibird_gt_boxes_host(_np_ptr(lay), _np_ptr(ext), ext.shape[0], _np_ptr(boxes), _np_ptr(n_gt), B),
          "sv_multibird_gt_boxes_host")
    return boxes, n_gt


def multibird_gt_boxes(layouts, extents):
    """layouts int32 [B,20] (ops.multibird_layouts), extents int32 [n,4] (ops.sprite_extents) -> (boxes [B,5,4] fp32, n_gt [B] int32)."""
    assert layouts.dtype == torch.int32 and layouts.dim() == 2 and layouts.shape[1] == MULTIBIRD_LAYOUT_WORDS
    assert extents.dtype == torch.int32 and extents.dim() == 2 and extents.shape[1] == 4
    B = layouts.shape[0]
    boxes = torch.empty((B, 5, 4), dtype=torch.float32, device=layouts.device)
    n_gt = torch.empty((B,), dtype=torch.int32, device=layouts.device)
    check(_lib.load().sv_multibird_gt_boxes(_p(layouts), _p(extents), extents.shape[0], _p(boxes), _p(n_gt), B, _stream()),
          "sv_multibird_gt_boxes")
    return boxes, n_gt


def detect_match_host(bbox, logits, gt_boxes, n_gt, image_offset=0, rec_key=None, rec_tp=None):
    """sv_detect_match_host over NumPy arrays: bbox [B,cells,4] fp32, logits [B,cells] fp32, gt_boxes [B,5,4] fp32, n_gt [B] int32 ->
    (rec_key uint64, rec_tp uint16); given arrays are written at the records of image_offset .. image_offset + B - 1.  No device."""
    import numpy as np
    bbox, logits = np.ascontiguousarray(bbox, np.float32), np.ascontiguousarray(logits, np.float32)
    gt_boxes, n_gt = np.ascontiguousarray(gt_boxes, np.float32), np.ascontiguousarray(n_gt, np.int32)
    B, cells = logits.shape
    assert bbox.shape == (B, cells, 4) and gt_boxes.shape == (B, 5, 4) and n_gt.shape == (B,)
    n = (image_offset + B) * cells
    if rec_key is None:
        rec_key, rec_tp = np.zeros((n,), np.uint64), np.zeros((n,), np.uint16)
    assert rec_key.dtype == np.uint64 and rec_tp.dtype == np.uint16 and rec_key.size >= n and rec_tp.size >= n
    assert rec_key.flags.c_contiguous and rec_tp.flags.c_contiguous
    check(_lib.load().sv_detect_match_host(_np_ptr(bbox), cells * 4, _np_ptr(logits), cells, cells, _np_ptr(gt_boxes), _np_ptr(n_gt), B,
                                           image_offset, _np_ptr(rec_key), _np_ptr(rec_tp)), "sv_detect_match_host")
    return rec_key, rec_tp


def detect_match(bbox, logits, gt_boxes, n_gt, rec_key, rec_tp, image_offset=0):
    """sv_detect_match: bbox [B,cells,4] and logits [B,cells(,...)] fp32 (an image's cells contiguous, images at any row pitch: the
    tape's outputs are read in place), gt_boxes [B,5,4] fp32, n_gt [B] int32 -> the records of images image_offset .. + B - 1 of
    rec_key (int64: the key's bits) and rec_tp (int16)."""
    B = bbox.shape[0]
    lg = logits.reshape(B, -1)
    cells = lg.shape[1]
    if lg.stride(1) != 1 or lg.data_ptr() % 4:
        lg = lg.contiguous()
    bb = bbox.reshape(B, cells, 4)
    if bb.stride(2) != 1 or bb.stride(1) != 4 or bb.data_ptr() % 4:
        bb = bb.contiguous()
    assert bb.dtype == torch.float32 and lg.dtype == torch.float32 and bb.is_cuda and lg.is_cuda
    assert gt_boxes.dtype == torch.float32 and tuple(gt_boxes.shape) == (B, 5, 4) and n_gt.dtype == torch.int32 and n_gt.numel() == B
    assert rec_key.dtype == torch.int64 and rec_tp.dtype == torch.int16 and rec_key.dim() == 1 and rec_tp.dim() == 1
    assert image_offset >= 0 and (image_offset + B) * cells <= min(rec_key.numel(), rec_tp.numel()), "record arrays too small"
    ldb = bb.stride(0) if B > 1 else cells * 4
    ldl = lg.stride(0) if B > 1 else cells
    check(_lib.load().sv_detect_match(C.c_void_p(bb.data_ptr()), ldb, C.c_void_p(lg.data_ptr()), ldl, cells, _p(gt_boxes), _p(n_gt), B,
                                      int(image_offset), _p(rec_key), _p(rec_tp), _stream()), "sv_detect_match")
    return rec_key, rec_tp


def detect_ap_chunk_records():
    return int(_lib.load().sv_detect_ap_chunk_records())


def detect_ap_workspace_bytes(n_records):
    n = C.c_int64()
    check(_lib.load().sv_detect_ap_workspace_bytes(int(n_records), C.byref(n)), "sv_detect_ap_workspace_bytes")
    return int(n.value)


def detect_ap_finish(rec_key, rec_tp, n_gt, n_records=None, workspace=None, out=None):
    """sv_detect_ap_finish over the first n_records records (default: all) -> out [29] fp64 on the device: AP_t [0:9], AP'_t [9:18],
    then int64 bits (out.view(torch.int64)) TP_t(M) [18:27], M [27], G [28].  workspace: uint8, at least detect_ap_workspace_bytes."""
    assert rec_key.dtype == torch.int64 and rec_tp.dtype == torch.int16 and n_gt.dtype == torch.int32
    n = int(rec_key.numel() if n_records is None else n_records)
    assert 1 <= n <= min(rec_key.numel(), rec_tp.numel())
    workspace = _workspace(detect_ap_workspace_bytes(n), workspace, rec_key.device)
    if out is None:
        out = torch.empty((DETECT_AP_OUT,), dtype=torch.float64, device=rec_key.device)
    assert out.dtype == torch.float64 and out.numel() == DETECT_AP_OUT
    check(_lib.load().sv_detect_ap_finish(_p(rec_key), _p(rec_tp), n, _p(n_gt), n_gt.numel(), _p(workspace), workspace.numel(), _p(out),
                                          _stream()), "sv_detect_ap_finish")
    return out


def adam_alpha(lr, beta1, beta2, t):
    """Keras Adam's bias-corrected step size of iteration t (what sv_adam_step* computes from lr and t)."""
    return float(_lib.load().sv_adam_alpha(float(lr), float(beta1), float(beta2), int(t)))


def adam_step_clipnorm(p, g, m, v, tensor_off, clipnorm, t, lr, beta1=0.9, beta2=0.999, eps=1e-7, grad_scale=1.0, alpha_dev=None):
    """Keras Adam(clipnorm=...) over flat buffers; tensor_off: int64 device tensor of n_tensors+1 offsets.  alpha_dev: a
    1-element device tensor holding adam_alpha(lr, beta1, beta2, t) -- read at run time instead of (lr, t) (hipGraph replay)."""
    nt = tensor_off.numel() - 1
    ws = torch.empty((256 * nt,), dtype=torch.float32, device=p.device)
    check(_lib.load().sv_adam_step_clipnorm_dyn(_p(p), _p(g), _p(m), _p(v), _p(tensor_off), nt, _p(ws), float(clipnorm), float(lr),
                                                float(beta1), float(beta2), float(eps), int(t), _p(alpha_dev), float(grad_scale),
                                                _stream()), "sv_adam_step_clipnorm")


# ------------------------------------------------------------------ K3-K10 conv (vae/model.py:36-38,:153-156)
class Conv2D:
    """One Conv2D(padding='same') layer instance on the MFMA path (forward, dgrad, wgrad)."""

    def __init__(self, B, H, W, Cin, Cout, k, stride, act=None, dtype=torch.bfloat16, y_f32=False, ups_in=False):
        r8 = lambda v: (v + 7) // 8 * 8
        self.dtype = dtype
        self.desc = ConvDesc(B, H, W, Cin, Cout, k, k, stride, 1 if act == "relu" else 0, sv_dtype(dtype),
                             r8(Cin), Cout if y_f32 else r8(Cout), 1 if y_f32 else 0, 1 if ups_in else 0)
        self.OH, self.OW = (H + stride - 1) // stride, (W + stride - 1) // stride
        lib = _lib.load()
        nf = lib.sv_conv2d_wprep_elems(C.byref(self.desc), 0)
        nd = lib.sv_conv2d_wprep_elems(C.byref(self.desc), 1)
        if nf < 0 or nd < 0:
            raise _lib.SplitVaeError("unsupported conv geometry")
        self.nf, self.nd = nf, nd
        self.w_fwd = self.w_dgrad = None

    def prep(self, w_hwio, fwd=True, dgrad=True):
        """The kernels' weight images from the Keras HWIO kernel (either may be skipped: a forward-only or gradient-only call)."""
        dev = w_hwio.device
        if fwd:
            self.w_fwd = torch.empty((self.nf,), dtype=self.dtype, device=dev)
        if dgrad:
            self.w_dgrad = torch.empty((self.nd,), dtype=self.dtype, device=dev)
        check(_lib.load().sv_conv2d_prep_weights(C.byref(self.desc), _p(w_hwio), _p(self.w_fwd if fwd else None),
                                                 _p(self.w_dgrad if dgrad else None), _stream()), "sv_conv2d_prep_weights")

    def fwd(self, x, bias, out=None, workspace=True):
        d = self.desc
        y = out if out is not None else torch.empty((d.B, self.OH, self.OW, d.ldy),
                                                    dtype=torch.float32 if d.y_f32 else self.dtype, device=x.device)
        lib = _lib.load()
        if workspace:                                   # polyphase head: border terms through a workspace (else atomics)
            n = lib.sv_conv2d_fwd_workspace_bytes(C.byref(d))
            if n > 0 and (getattr(self, "_fws", None) is None or self._fws.numel() < n or self._fws.device != x.device):
                self._fws = torch.empty((n,), dtype=torch.uint8, device=x.device)
            ws = self._fws if n > 0 else None
            check(lib.sv_conv2d_nhwc_fwd_ws(C.byref(d), _p(x), _p(self.w_fwd), _p(bias), _p(y), _p(ws), n if n > 0 else 0,
                                            _stream()), "sv_conv2d_nhwc_fwd_ws")
        else:
            check(lib.sv_conv2d_nhwc_fwd(C.byref(d), _p(x), _p(self.w_fwd), _p(bias), _p(y), _stream()), "sv_conv2d_nhwc_fwd")
        return y

    def dgrad(self, dy, relu_mask=None, f32_atomic=False, out=None):
        """out (f32_atomic only): an fp32 [B,H,W,ldx] tensor the partial sums are ADDED to (several layers
        feeding one activation accumulate into the same buffer)."""
        d = self.desc
        if out is not None:
            assert f32_atomic and out.dtype == torch.float32
            dx = out
        elif f32_atomic:
            dx = torch.zeros((d.B, d.H, d.W, d.ldx), dtype=torch.float32, device=dy.device)
        else:
            dx = torch.zeros((d.B, d.H, d.W, d.ldx), dtype=self.dtype, device=dy.device)
        check(_lib.load().sv_conv2d_nhwc_dgrad(C.byref(d), _p(dy), _p(self.w_dgrad), _p(relu_mask), _p(dx),
                                               1 if f32_atomic else 0, _stream()), "sv_conv2d_nhwc_dgrad")
        return dx

    def dgrad_lowres(self, dy, relu_mask_lo=None):
        """ups_in layers: the gradient at the LOW-RES input [B,H/2,W/2,ldx] in one launch (conv-transpose, resize adjoint, ReLU
        mask); None when the geometry has no fused kernel (then: upsample2x_bwd(dgrad(dy), mask))."""
        d = self.desc
        dx = torch.empty((d.B, d.H // 2, d.W // 2, d.ldx), dtype=self.dtype, device=dy.device)
        lib = _lib.load()
        n = lib.sv_conv2d_dgrad_lowres_workspace_bytes(C.byref(d))          # > 0: the polyphase form (fp32 d4 / d5), edge terms through a workspace
        if n > 0:
            if getattr(self, "_dws", None) is None or self._dws.numel() < n or self._dws.device != dy.device:
                self._dws = torch.empty((n,), dtype=torch.uint8, device=dy.device)
            rc = lib.sv_conv2d_nhwc_dgrad_lowres_ws(C.byref(d), _p(dy), _p(self.w_dgrad), _p(relu_mask_lo), _p(dx), _p(self._dws), n, _stream())
        else:
            rc = lib.sv_conv2d_nhwc_dgrad_lowres(C.byref(d), _p(dy), _p(self.w_dgrad), _p(relu_mask_lo), _p(dx), _stream())
        if rc == _lib.STATUS_UNSUPPORTED:
            return None
        check(rc, "sv_conv2d_nhwc_dgrad_lowres")
        return dx

    def wgrad(self, x, dy, workspace=False, dw=None, db=None):
        """dw / db: zeroed fp32 views to accumulate into (e.g. slices of a flat gradient buffer)."""
        d = self.desc
        if dw is None and db is None:                    # one zero fill for both accumulators
            n = d.KH * d.KW * d.Cin * d.Cout
            n4 = (n + 3) // 4 * 4
            z = torch.zeros((n4 + d.Cout,), dtype=torch.float32, device=x.device)
            dw, db = z[:n].view(d.KH, d.KW, d.Cin, d.Cout), z[n4:]
        if dw is None:
            dw = torch.zeros((d.KH, d.KW, d.Cin, d.Cout), dtype=torch.float32, device=x.device)
        if db is None:
            db = torch.zeros((d.Cout,), dtype=torch.float32, device=x.device)
        if workspace:
            n = _lib.load().sv_conv2d_wgrad_workspace_bytes(C.byref(d))
            if getattr(self, "_ws", None) is None or self._ws.numel() < n:
                self._ws = torch.empty((n,), dtype=torch.uint8, device=x.device)
            check(_lib.load().sv_conv2d_nhwc_wgrad_ws(C.byref(d), _p(x), _p(dy), _p(dw), _p(db), _p(self._ws), n, _stream()),
                  "sv_conv2d_nhwc_wgrad_ws")
        else:
            check(_lib.load().sv_conv2d_nhwc_wgrad(C.byref(d), _p(x), _p(dy), _p(dw), _p(db), _stream()),
                  "sv_conv2d_nhwc_wgrad")
        return dw, db

    def wgrad_poly(self, x_lo, dy, dw=None, db=None):
        """Polyphase weight gradient of the decoder head (sv_conv2d_nhwc_wgrad_poly); None when the layer has no such form."""
        d = self.desc
        lib = _lib.load()
        n = lib.sv_conv2d_wgrad_poly_workspace_bytes(C.byref(d))
        if n <= 0:
            return None
        if getattr(self, "_pws", None) is None or self._pws.numel() < n or self._pws.device != x_lo.device:
            self._pws = torch.zeros((n,), dtype=torch.uint8, device=x_lo.device)
        if dw is None:
            dw = torch.zeros((d.KH, d.KW, d.Cin, d.Cout), dtype=torch.float32, device=x_lo.device)
        if db is None:
            db = torch.zeros((d.Cout,), dtype=torch.float32, device=x_lo.device)
        check(lib.sv_conv2d_nhwc_wgrad_poly(C.byref(d), _p(x_lo), _p(dy), _p(dw), _p(db), _p(self._pws), n, _stream()),
              "sv_conv2d_nhwc_wgrad_poly")
        return dw, db


# ------------------------------------------------------------------ the whole-step plan
class LGVaePlan:
    """Native launch plan for LGVae.call / train_step_lg_vae (vae/model.py:189-200, vae/trainer.py:120-144)."""

    def __init__(self, B, H, W, global_latent=128, local_latent=128, beta=40.0, dtype=torch.bfloat16, device="cuda",
                 external_global_encoder=False, global_only=False):
        lib = _lib.load()
        self.lib = lib
        self.device = torch.device(device)
        self.dtype = dtype
        # global_only: GMVae's one branch (include/splitvae.h) -- decoder_x over the caller's z_x, no x-hat network
        self.desc = LGVaeDesc(B, H, W, global_latent, local_latent, sv_dtype(dtype), float(beta),
                              1 if external_global_encoder else 0, 1 if global_only else 0)
        h = C.c_void_p()
        check(lib.sv_lgvae_plan_create(C.byref(self.desc), C.byref(h)), "sv_lgvae_plan_create")
        self.handle = h
        self.n_params = lib.sv_lgvae_param_count(C.byref(self.desc))
        self.param_table = param_table(self.desc)
        nbytes = lib.sv_lgvae_workspace_bytes(h)
        self.workspace = torch.zeros((nbytes,), dtype=torch.uint8, device=self.device)
        check(lib.sv_lgvae_plan_bind(h, _p(self.workspace), nbytes, _stream()), "sv_lgvae_plan_bind")
        # generation of the shared input buffers in8_x / in8_xh: bumped by every writer (a staged augmentation, the split / pad
        # pass of any step that runs the encoders' forward); a staged batch is only valid while its generation is the current one
        self.in8_gen = 0
        self.graph_on = False
        self._views = {}

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self.lib.sv_lgvae_plan_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    def buffer(self, name, dtype, shape):
        """A named buffer of the plan's workspace as a tensor view (memoised: the same view object for the same request -- a step asks for half a dozen of
        them, ~25 us of ctypes + view arithmetic each, and the launch-bound steps are host-bound by now)."""
        key = (name, dtype, tuple(shape))
        v = self._views.get(key)
        if v is None:
            off, nb = C.c_int64(), C.c_int64()
            check(self.lib.sv_lgvae_buffer(self.handle, name.encode(), C.byref(off), C.byref(nb)), "sv_lgvae_buffer " + name)
            v = self._views[key] = self.workspace[off.value: off.value + nb.value].view(dtype).view(*shape)
        return v

    def step(self, phases, params=None, grads=None, adam_m=None, adam_v=None, images6=None, eps_x=None,
             eps_x_hat=None, seed=0, step=0, sample_offset=0, lr=1e-4, beta1=0.9, beta2=0.999, adam_eps=1e-7, t=1,
             grad_scale=1.0, accumulate_metrics=False):
        a = StepArgs()
        for name, tns in (("params", params), ("grads", grads), ("adam_m", adam_m), ("adam_v", adam_v),
                          ("images6", images6), ("eps_x", eps_x), ("eps_x_hat", eps_x_hat)):
            setattr(a, name, None if tns is None else _p(tns).value)
        a.seed, a.step, a.sample_offset = seed, step, sample_offset
        a.lr, a.beta1, a.beta2, a.adam_eps, a.t = lr, beta1, beta2, adam_eps, t
        a.grad_scale, a.phases, a.accumulate_metrics = grad_scale, phases, 1 if accumulate_metrics else 0
        if (phases & _lib.PHASE_FWD_ENCODERS) and not (phases & _lib.PHASE_INPUTS_STAGED):
            self.in8_gen += 1                                  # this step's split / pad pass overwrites in8_x / in8_xh
        check(self.lib.sv_lgvae_step(self.handle, C.byref(a), _stream()), "sv_lgvae_step")

    def bucket_wait(self, bucket, stream):
        """Make `stream` (a torch.cuda.Stream) wait for gradient bucket 0 (decoders) / 1 (encoder heads) / 2 (encoder convs) / 3 (1 and 2) of the last
        step that carried PHASE_BUCKET_EVENTS (sv_lgvae_bucket_wait)."""
        check(self.lib.sv_lgvae_bucket_wait(self.handle, int(bucket), C.c_void_p(stream.cuda_stream)), "sv_lgvae_bucket_wait")

    def debug(self, key, value):
        """Test hooks of this plan (include/splitvae.h: sv_lgvae_plan_debug)."""
        check(self.lib.sv_lgvae_plan_debug(self.handle, key.encode(), int(value)), "sv_lgvae_plan_debug")

    def graph_enable(self, on=True):
        """hipGraph replay of `step` (include/splitvae.h: sv_lgvae_graph_enable); effective on a non-default stream."""
        check(self.lib.sv_lgvae_graph_enable(self.handle, 1 if on else 0), "sv_lgvae_graph_enable")
        self.graph_on = bool(on)

    def graph_count(self):
        return int(self.lib.sv_lgvae_graph_count(self.handle))

    def profile_enable(self, on=True):
        check(self.lib.sv_lgvae_profile_enable(self.handle, 1 if on else 0), "sv_lgvae_profile_enable")

    def profile_filter(self, name=None):
        check(self.lib.sv_lgvae_profile_filter(self.handle, (name or "").encode()), "sv_lgvae_profile_filter")

    def profile_read(self, max_entries=128):
        names = ((C.c_char * 64) * max_entries)()
        ms = (C.c_double * max_entries)()
        n_l = (C.c_int32 * max_entries)()
        fl = (C.c_double * max_entries)()
        by = (C.c_double * max_entries)()
        n = self.lib.sv_lgvae_profile_read(self.handle, max_entries, names, ms, n_l, fl, by)
        if n < 0:
            check(n, "sv_lgvae_profile_read")
        iss = (C.c_double * max_entries)()
        ni = self.lib.sv_lgvae_profile_read_issued(self.handle, max_entries, iss)
        if ni < 0:
            check(ni, "sv_lgvae_profile_read_issued")
        # flops: the direct form's count; issued: what the scope's algorithm really multiplies (polyphase forms: fewer)
        return [dict(name=names[i].value.decode(), total_ms=ms[i], launches=n_l[i], flops=fl[i], bytes=by[i], issued=iss[i] if i < ni else fl[i])
                for i in range(n)]


def param_table(desc):
    """[(name, offset, shape)] of the 40 variables in Keras creation order (the 10 of decoder_x for a global_only desc)."""
    lib = _lib.load()
    out = []
    for i in range(10 if desc.global_only else 40):
        off, nd = C.c_int64(), C.c_int32()
        shp = (C.c_int64 * 4)()
        name = C.create_string_buffer(96)
        check(lib.sv_lgvae_param_info(C.byref(desc), i, C.byref(off), C.byref(nd), C.byref(shp), name), "sv_lgvae_param_info")
        out.append((name.value.decode(), off.value, tuple(shp[k] for k in range(nd.value))))
    return out


# ------------------------------------------------------------------ IW: importance-weighted log-likelihood (include/splitvae.h)
def iw_advance(z_mean_x, z_sig_x, z_mean_xh, z_sig_xh, zcat, r, k, flags, nll_x=None, nll_xh=None, state=None, eps=None, seed=0,
               sample_offset=0):
    """sv_iw_advance between two decoder passes: fold sample k - 1 into state [B,5] fp64 (IW_ACCUMULATE) and / or draw sample k
    into zcat [B,Lg+Ll] (the plan's dtype) and r [B] (IW_DRAW).  eps [B,Lg+Ll] pins the draw."""
    B, Lg = z_mean_x.shape
    Ll = z_mean_xh.shape[1]
    assert r.dtype == torch.float32 and (state is None or (state.dtype == torch.float64 and tuple(state.shape) == (B, 5)))
    assert eps is None or (eps.dtype == torch.float32 and tuple(eps.shape) == (B, Lg + Ll))
    check(_lib.load().sv_iw_advance(_p(z_mean_x), _p(z_sig_x), _p(z_mean_xh), _p(z_sig_xh), _p(eps), _p(zcat), sv_dtype(zcat.dtype),
                                    zcat.shape[1], _p(r), _p(nll_x), _p(nll_xh), _p(state), B, Lg, Ll, int(k), int(seed),
                                    int(sample_offset), int(flags), _stream()), "sv_iw_advance")


def iw_finish(state, K, out3=None, acc=None):
    """sv_iw_finish: out3 [B,3] fp32 = per-image (L_joint, L_x, elbo); acc [4] fp64 += their sums and the image count."""
    B = state.shape[0]
    if out3 is None:
        out3 = torch.empty((B, 3), dtype=torch.float32, device=state.device)
    assert state.dtype == torch.float64 and out3.dtype == torch.float32 and (acc is None or (acc.dtype == torch.float64 and acc.numel() >= 4))
    check(_lib.load().sv_iw_finish(_p(state), int(K), _p(out3), _p(acc), B, _stream()), "sv_iw_finish")
    return out3


def iw_gm_advance(logits, zm_all, zs_all, pm, ps, z_mean_xh, z_sig_xh, zcat, r, comp_out, k, flags, nll_x=None, nll_xh=None,
                  state=None, eps=None, comp=None, seed=0, sample_offset=0):
    """sv_iw_gm_advance, the mixture models' sv_iw_advance: logits [B,n], zm_all / zs_all [B,n,Lg], pm / ps [n,Lg] fp32; z_mean_xh /
    z_sig_xh [B,Ll] or None (one branch, Ll = 0); eps [B,Lg+Ll] fp32 and comp [B] int32 pin the draw; comp_out [B] int32 receives
    the component drawn."""
    B, n, Lg = zm_all.shape
    Ll = 0 if z_mean_xh is None else z_mean_xh.shape[1]
    i32 = torch.int32
    assert tuple(logits.shape) == (B, n) and tuple(zs_all.shape) == (B, n, Lg) and tuple(pm.shape) == (n, Lg) and tuple(ps.shape) == (n, Lg)
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in (logits, zm_all, zs_all, pm, ps, r))
    assert z_mean_xh is None or (tuple(z_mean_xh.shape) == tuple(z_sig_xh.shape) == (B, Ll) and z_mean_xh.is_contiguous() and z_sig_xh.is_contiguous())
    assert state is None or (state.dtype == torch.float64 and tuple(state.shape) == (B, 5))
    assert eps is None or (eps.dtype == torch.float32 and tuple(eps.shape) == (B, Lg + Ll) and eps.is_contiguous())
    assert comp_out.dtype == i32 and comp_out.numel() == B and (comp is None or (comp.dtype == i32 and comp.numel() == B))
    assert zcat.shape[0] == B and zcat.stride(1) == 1 and r.numel() == B
    check(_lib.load().sv_iw_gm_advance(_p(logits), _p(zm_all), _p(zs_all), _p(pm), _p(ps), _p(z_mean_xh), _p(z_sig_xh), _p(eps), _p(comp),
                                       _p(comp_out), _p(zcat), sv_dtype(zcat.dtype), zcat.stride(0), _p(r), _p(nll_x), _p(nll_xh),
                                       _p(state), B, n, Lg, Ll, int(k), int(seed), int(sample_offset), int(flags), _stream()),
          "sv_iw_gm_advance")


def iw_gm_uniform_host(seed, image, sample):
    """sv_iw_gm_uniform_host: the uniform in (0, 1] behind the component pick of (seed, global image index, sample).  No device."""
    return float(_lib.load().sv_iw_gm_uniform_host(int(seed), int(image), int(sample)))


def iw_gm_tables(he, w_ht, b_ht, w_zm, b_zm, w_zs, b_zs, w_pm, b_pm, w_ps, b_ps, out=None):
    """sv_iw_gm_tables: (zm_all, zs_all [B,n,L], pm, ps [n,L]) fp32 from the GM encoder's he [B,hidden] and the Keras kernels / biases
    of h_top_dense, z_mean, z_sig, z_prior_mean, z_prior_sig (views of the flat parameter buffer)."""
    B, hidden = he.shape
    n, L = w_pm.shape
    f32 = torch.float32
    assert he.is_contiguous() and tuple(w_ht.shape) == (n, hidden) and tuple(w_zm.shape) == tuple(w_zs.shape) == (hidden, L) and tuple(w_ps.shape) == (n, L)
    assert b_ht.numel() == hidden and b_zm.numel() == b_zs.numel() == b_pm.numel() == b_ps.numel() == L
    assert all(t.dtype == f32 and t.is_contiguous() for t in (w_ht, b_ht, w_zm, b_zm, w_zs, b_zs, w_pm, b_pm, w_ps, b_ps))
    if out is None:
        e = lambda *s: torch.empty(s, dtype=f32, device=he.device)      # noqa: E731
        out = (e(B, n, L), e(B, n, L), e(n, L), e(n, L))
    zm_all, zs_all, pm, ps = out
    assert tuple(zm_all.shape) == tuple(zs_all.shape) == (B, n, L) and tuple(pm.shape) == tuple(ps.shape) == (n, L)
    assert all(t.dtype == f32 and t.is_contiguous() for t in out)
    check(_lib.load().sv_iw_gm_tables(_p(he), sv_dtype(he.dtype), _p(w_ht), _p(b_ht), _p(w_zm), _p(b_zm), _p(w_zs), _p(b_zs), _p(w_pm),
                                      _p(b_pm), _p(w_ps), _p(b_ps), _p(zm_all), _p(zs_all), _p(pm), _p(ps), B, n, hidden, L, _stream()),
          "sv_iw_gm_tables")
    return out


# ------------------------------------------------------------------ k-NN label probe of the latents (include/splitvae.h)
def knn_chunk_rows():
    return int(_lib.load().sv_knn_chunk_rows())


def knn_workspace_bytes(Nq, Nr, k):
    n = C.c_int64()
    check(_lib.load().sv_knn_workspace_bytes(int(Nq), int(Nr), int(k), C.byref(n)), "sv_knn_workspace_bytes")
    return n.value


def _rows_f32(t, name):
    if not torch.is_tensor(t) or t.dim() != 2 or t.dtype != torch.float32 or not t.is_cuda or t.stride(1) != 1 or t.stride(0) < t.shape[1]:
        raise ValueError("%s must be a 2-D fp32 device tensor with contiguous rows (a row pitch >= its width is allowed)" % name)
    return C.c_void_p(t.data_ptr()), int(t.stride(0))


def _classes_u8(t, n, name):
    if not torch.is_tensor(t) or t.dtype != torch.uint8 or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != (n,):
        raise ValueError("%s must be a contiguous uint8 device tensor of %d class ids" % (name, n))
    return C.c_void_p(t.data_ptr())


def knn_classify(q, r, r_class, k, n_class, q_class=None, acc=None, want_neighbours=False, workspace=None):
    """sv_knn_classify: pred [Nq] int32 = the majority class among the k references of r [Nr,L] nearest to each row of q [Nq,L]
    (squared Euclidean distance, ties to the lower index / class).  q_class [Nq] uint8 and acc [2] int64 (device): acc += (hits,
    Nq).  want_neighbours: returns (pred, nn_index [Nq,k] int32, nn_dist [Nq,k] fp32).  workspace: a uint8 device tensor of at
    least knn_workspace_bytes(Nq, Nr, k) bytes with any contents (default: allocated here)."""
    qp, ldq = _rows_f32(q, "q")
    rp, ldr = _rows_f32(r, "r")
    Nq, L = q.shape
    Nr = r.shape[0]
    if r.shape[1] != L or r.device != q.device:
        raise ValueError("q [%d,%d] and r [%d,%d] must have one width and one device" % (Nq, L, Nr, r.shape[1]))
    rc = _classes_u8(r_class, Nr, "r_class")
    qc = None if q_class is None else _classes_u8(q_class, Nq, "q_class")
    if acc is not None and (acc.dtype != torch.int64 or not acc.is_cuda or not acc.is_contiguous() or acc.numel() < 2):
        raise ValueError("acc must be a contiguous int64 device tensor of >= 2 elements")
    pred = torch.empty((Nq,), dtype=torch.int32, device=q.device)
    nn_i = torch.empty((Nq, int(k)), dtype=torch.int32, device=q.device) if want_neighbours else None
    nn_d = torch.empty((Nq, int(k)), dtype=torch.float32, device=q.device) if want_neighbours else None
    ws = _workspace(knn_workspace_bytes(Nq, Nr, k), workspace, q.device)
    check(_lib.load().sv_knn_classify(qp, ldq, rp, ldr, rc, Nq, Nr, L, int(k), int(n_class), _p(nn_i), _p(nn_d), _p(pred), qc, _p(acc),
                                      _p(ws), ws.numel(), _stream()), "sv_knn_classify")
    return (pred, nn_i, nn_d) if want_neighbours else pred


# ------------------------------------------------------------------ k-means cluster report of the latents (include/splitvae.h)
def kmeans_chunk_rows():
    return int(_lib.load().sv_kmeans_chunk_rows())


def kmeans_workspace_bytes(N, L, K, R):
    n = C.c_int64()
    check(_lib.load().sv_kmeans_workspace_bytes(int(N), int(L), int(K), int(R), C.byref(n)), "sv_kmeans_workspace_bytes")
    return n.value


def kmeans_seed(x, K, R, seed=0, want_picks=False, workspace=None):
    """sv_kmeans_seed: the k-means++ centres of R restarts of x [N,L] -> centroids [R,K,L] fp32 (and picks [R,K] int32, their rows)."""
    xp, ldx = _rows_f32(x, "x")
    N, L = x.shape
    cent = torch.empty((int(R), int(K), L), dtype=torch.float32, device=x.device)
    picks = torch.empty((int(R), int(K)), dtype=torch.int32, device=x.device) if want_picks else None
    ws = _workspace(kmeans_workspace_bytes(N, L, K, R), workspace, x.device)
    check(_lib.load().sv_kmeans_seed(xp, ldx, N, L, int(K), int(R), int(seed) & (2 ** 64 - 1), _p(cent), _p(picks), _p(ws), ws.numel(),
                                     _stream()), "sv_kmeans_seed")
    return (cent, picks) if want_picks else cent


def kmeans_state(x, centroids):
    """The in-out buffers of a fit of x [N,L] from centroids [R,K,L]: dict(centroids (the tensor given: written in place), assign [R,N]
    int32, counts [R,K] int32, inertia [R] fp64, n_iter [R] int32, state [2R + 1] int32), for kmeans_iterate."""
    R, K, L = centroids.shape
    if centroids.dtype != torch.float32 or not centroids.is_cuda or not centroids.is_contiguous() or L != x.shape[1]:
        raise ValueError("centroids must be a contiguous [R,K,%d] fp32 device tensor" % x.shape[1])
    e = lambda shape, dt: torch.empty(shape, dtype=dt, device=x.device)      # noqa: E731
    return dict(centroids=centroids, assign=e((R, x.shape[0]), torch.int32), counts=e((R, K), torch.int32), inertia=e((R,), torch.float64),
                n_iter=e((R,), torch.int32), state=e((2 * R + 1,), torch.int32))


def kmeans_iterate(x, fit, iters, resume=False, workspace=None):
    """sv_kmeans_iterate on the buffers of kmeans_state: resume False starts the fit at fit["centroids"] (one assign pass, then `iters`
    update + assign steps), True continues it by `iters` more.  Nothing is read back."""
    xp, ldx = _rows_f32(x, "x")
    N, L = x.shape
    R, K, _ = fit["centroids"].shape
    ws = _workspace(kmeans_workspace_bytes(N, L, K, R), workspace, x.device)
    check(_lib.load().sv_kmeans_iterate(xp, ldx, N, L, K, R, int(iters), int(bool(resume)), _p(fit["centroids"]), _p(fit["assign"]),
                                        _p(fit["counts"]), _p(fit["inertia"]), _p(fit["n_iter"]), _p(fit["state"]), _p(ws), ws.numel(),
                                        _stream()), "sv_kmeans_iterate")
    return fit


def kmeans_best(inertia, out=None):
    best = torch.empty((1,), dtype=torch.int32, device=inertia.device) if out is None else out
    check(_lib.load().sv_kmeans_best(_p(inertia), inertia.numel(), _p(best), _stream()), "sv_kmeans_best")
    return best


def contingency(a, b, counts):
    """counts [Ka,Kb] int32 (accumulated into) += the pairs (a_i, b_i) of two int32 label vectors (sv_contingency)."""
    if a.dtype != torch.int32 or b.dtype != torch.int32 or counts.dtype != torch.int32 or a.numel() != b.numel() or counts.dim() != 2:
        raise ValueError("contingency takes two int32 label vectors of one length and an int32 [Ka,Kb] table")
    check(_lib.load().sv_contingency(_p(a), _p(b), a.numel(), counts.shape[0], counts.shape[1], _p(counts), _stream()), "sv_contingency")
    return counts


# ------------------------------------------------------------------ linear label probe of the latents (include/splitvae.h)
def linprobe_chunk_rows():
    return int(_lib.load().sv_linprobe_chunk_rows())


def linprobe_workspace_bytes(N, L, n_class):
    n = C.c_int64()
    check(_lib.load().sv_linprobe_workspace_bytes(int(N), int(L), int(n_class), C.byref(n)), "sv_linprobe_workspace_bytes")
    return n.value


def _f64(t, shape, name):
    if not torch.is_tensor(t) or t.dtype != torch.float64 or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
        raise ValueError("%s must be a contiguous fp64 device tensor of shape %s" % (name, tuple(shape)))
    return t


def linprobe_gram(x, workspace=None):
    """sv_linprobe_gram: S [(L+1),(L+1)] fp64 = A^T A of A = [x 1], x [N,L] fp32 (not divided by N; symmetric bit for bit)."""
    xp, ldx = _rows_f32(x, "x")
    N, L = x.shape
    S = torch.empty((L + 1, L + 1), dtype=torch.float64, device=x.device)
    ws = _workspace(linprobe_workspace_bytes(N, L, 2), workspace, x.device)
    check(_lib.load().sv_linprobe_gram(xp, ldx, N, L, _p(S), _p(ws), ws.numel(), _stream()), "sv_linprobe_gram")
    return S


def linprobe_state(x, n_class, total_iters, W=None):
    """The in-out buffers of a fit of x [N,L] over `total_iters` steps in all: dict(W [(L+1),C] fp64 (zeros, or the tensor given: written
    in place), loss / gmax [total_iters + 1] fp64, grad [(L+1),C] fp64, state [1] int32), for linprobe_fit."""
    L = x.shape[1]
    e = lambda shape, dt: torch.empty(shape, dtype=dt, device=x.device)      # noqa: E731
    W = torch.zeros((L + 1, int(n_class)), dtype=torch.float64, device=x.device) if W is None else _f64(W, (L + 1, int(n_class)), "W")
    return dict(W=W, loss=e((int(total_iters) + 1,), torch.float64), gmax=e((int(total_iters) + 1,), torch.float64),
                grad=e((L + 1, int(n_class)), torch.float64), state=e((1,), torch.int32))


def linprobe_fit(x, y, P, fit, iters, l2, resume=False, workspace=None):
    """sv_linprobe_fit on the buffers of linprobe_state: resume False starts at fit["W"] and the trajectory index 0 and makes `iters`
    steps W <- W - P G, True continues by `iters` more.  y [N] uint8 class ids, P [(L+1),(L+1)] fp64.  Nothing is read back."""
    xp, ldx = _rows_f32(x, "x")
    N, L = x.shape
    n_class = fit["W"].shape[1]
    yp = _classes_u8(y, N, "y")
    _f64(P, (L + 1, L + 1), "P")
    _f64(fit["W"], (L + 1, n_class), "W")
    ws = _workspace(linprobe_workspace_bytes(N, L, n_class), workspace, x.device)
    check(_lib.load().sv_linprobe_fit(xp, ldx, yp, N, L, n_class, _p(P), float(l2), int(iters), int(bool(resume)), _p(fit["W"]),
                                      _p(fit["loss"]), _p(fit["gmax"]), _p(fit["grad"]), _p(fit["state"]), _p(ws), ws.numel(), _stream()),
          "sv_linprobe_fit")
    return fit


def linprobe_predict(q, W, q_class=None, acc=None, want_loss=False, workspace=None):
    """sv_linprobe_predict: pred [Nq] int32 = the first maximum of the logits of q [Nq,L] under W [(L+1),C] fp64.  q_class [Nq] uint8
    and acc [2] int64 (device): acc += (hits, Nq), without q_class the count only.  want_loss (needs q_class): returns (pred, loss
    [1] fp64, the mean cross-entropy)."""
    qp, ldq = _rows_f32(q, "q")
    Nq, L = q.shape
    n_class = W.shape[1] if torch.is_tensor(W) and W.dim() == 2 else 0
    _f64(W, (L + 1, n_class), "W")
    qc = None if q_class is None else _classes_u8(q_class, Nq, "q_class")
    if acc is not None and (acc.dtype != torch.int64 or not acc.is_cuda or not acc.is_contiguous() or acc.numel() < 2):
        raise ValueError("acc must be a contiguous int64 device tensor of >= 2 elements")
    pred = torch.empty((Nq,), dtype=torch.int32, device=q.device)
    loss = torch.empty((1,), dtype=torch.float64, device=q.device) if want_loss else None
    ws = _workspace(linprobe_workspace_bytes(Nq, L, n_class), workspace, q.device)
    check(_lib.load().sv_linprobe_predict(qp, ldq, Nq, L, n_class, _p(W), _p(pred), qc, _p(acc), _p(loss), _p(ws), ws.numel(), _stream()),
          "sv_linprobe_predict")
    return (pred, loss) if want_loss else pred


# ------------------------------------------------------------------ exact t-SNE map of the latents (include/splitvae.h)
def tsne_chunk_rows():
    return int(_lib.load().sv_tsne_chunk_rows())


def tsne_workspace_bytes(N):
    n = C.c_int64()
    check(_lib.load().sv_tsne_workspace_bytes(int(N), C.byref(n)), "sv_tsne_workspace_bytes")
    return n.value


def tsne_affinities(x, perplexity, stages=3, P=None, workspace=None):
    """sv_tsne_affinities of x [N,L] -> dict(P [N,N] fp32, beta [N] fp64, row_entropy [N] fp64, p_const [2] fp64 (sum P, sum P log P)).
    stages 1 / 2 stop behind the distances / the conditional rows (P holds those).  P: an [N,N] fp32 buffer to fill instead of a fresh one."""
    xp, ldx = _rows_f32(x, "x")
    N, L = x.shape
    if P is None:
        P = torch.empty((N, N), dtype=torch.float32, device=x.device)
    if P.dtype != torch.float32 or not P.is_cuda or not P.is_contiguous() or tuple(P.shape) != (N, N):
        raise ValueError("P must be a contiguous [%d,%d] fp32 device tensor" % (N, N))
    e = lambda n: torch.empty((n,), dtype=torch.float64, device=x.device)      # noqa: E731
    out = dict(P=P, beta=e(N), row_entropy=e(N), p_const=e(2))
    ws = _workspace(tsne_workspace_bytes(N), workspace, x.device)
    check(_lib.load().sv_tsne_affinities(xp, ldx, N, L, float(perplexity), int(stages), _p(P), _p(out["beta"]), _p(out["row_entropy"]),
                                         _p(out["p_const"]), _p(ws), ws.numel(), _stream()), "sv_tsne_affinities")
    return out


def tsne_state(N, total_iters, device="cuda", Y=None, inc=None, gain=None, counter=0):
    """The in-out buffers of a run: dict(Y, inc, gain [N,2] fp32, state [4] int32, kl [total_iters] fp64 (NaN until written), z [1] fp64).
    Without Y this is storage only (tsne_init fills it); with Y (and optionally inc, gain, counter) it is a caller's state."""
    def take(t, fill):
        if t is None:
            return torch.full((N, 2), fill, dtype=torch.float32, device=device)
        if t.dtype != torch.float32 or not t.is_cuda or tuple(t.shape) != (N, 2):
            raise ValueError("Y, inc and gain must be [%d,2] fp32 device tensors" % N)
        return t.contiguous()
    state = torch.zeros((4,), dtype=torch.int32, device=device)
    state[0] = int(counter)
    return dict(Y=take(Y, 0.0), inc=take(inc, 0.0), gain=take(gain, 1.0), state=state,
                kl=torch.full((max(int(total_iters), 1),), float("nan"), dtype=torch.float64, device=device),
                z=torch.zeros((1,), dtype=torch.float64, device=device))


def tsne_init(st, seed=0):
    """sv_tsne_init on the buffers of tsne_state: the Philox initial map, inc = 0, gain = 1, counter = 0."""
    N = st["Y"].shape[0]
    check(_lib.load().sv_tsne_init(N, int(seed) & (2 ** 64 - 1), _p(st["Y"]), _p(st["inc"]), _p(st["gain"]), _p(st["state"]), _stream()), "sv_tsne_init")
    return st


def tsne_iterate(aff, st, iters, exaggeration=12.0, exag_iters=250, eta=200.0, workspace=None):
    """sv_tsne_iterate: `iters` more iterations of the run in `st` against aff["P"]; nothing is read back."""
    P = aff["P"]
    N = P.shape[0]
    ws = _workspace(tsne_workspace_bytes(N), workspace, P.device)
    check(_lib.load().sv_tsne_iterate(_p(P), _p(aff["p_const"]), N, int(iters), float(exaggeration), int(exag_iters), float(eta), _p(st["Y"]),
                                      _p(st["inc"]), _p(st["gain"]), _p(st["state"]), _p(st["kl"]), st["kl"].numel(), _p(st["z"]), _p(ws),
                                      ws.numel(), _stream()), "sv_tsne_iterate")
    return st


def tsne_neighbour_scores(nn_latent, nn_map, labels=None, n_class=0, counts=None):
    """sv_tsne_neighbour_scores: counts [3] int64 += (latent neighbours kept in the map, map k-NN hits, latent k-NN hits) from the two
    [N,k+1] int32 neighbour lists of knn_classify(x, x, ..., k + 1, want_neighbours=True); labels [N] uint8 or None."""
    N, k1 = nn_latent.shape
    for t in (nn_latent, nn_map):
        if t.dtype != torch.int32 or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != (N, k1):
            raise ValueError("the neighbour lists must be contiguous [N,k+1] int32 device tensors of one shape")
    lab = None if labels is None else _classes_u8(labels, N, "labels")
    if counts is None:
        counts = torch.zeros((3,), dtype=torch.int64, device=nn_latent.device)
    check(_lib.load().sv_tsne_neighbour_scores(_p(nn_latent), _p(nn_map), lab, N, k1 - 1, int(n_class), _p(counts), _stream()),
          "sv_tsne_neighbour_scores")
    return counts


# ------------------------------------------------------------------ swap-consistency report of the latents (include/splitvae.h)
def swap_chunk_rows():
    return int(_lib.load().sv_swap_chunk_rows())


def swap_rank_workspace_bytes(Nq, Nr, L):
    n = C.c_int64()
    check(_lib.load().sv_swap_rank_workspace_bytes(int(Nq), int(Nr), int(L), C.byref(n)), "sv_swap_rank_workspace_bytes")
    return n.value


def swap_shift_word_host(seed, p, attempt=0):
    """The 32-bit Philox word of (seed, partner p, attempt) the report's partner shifts come from; host only."""
    return int(_lib.load().sv_swap_shift_word_host(int(seed) & (2 ** 64 - 1), int(p), int(attempt)))


def _index_i32(t, n, name, limit=None):
    """A contiguous int32 device tensor [n]; with `limit`, one host read checks every entry against [0, limit)."""
    if not torch.is_tensor(t) or t.dtype != torch.int32 or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != (n,):
        raise ValueError("%s must be a contiguous int32 device tensor of %d indices" % (name, n))
    if limit is not None and n:
        lo, hi = torch.stack([t.min(), t.max()]).tolist()
        if lo < 0 or hi >= limit:
            raise ValueError("%s: an index outside [0, %d): min %d, max %d" % (name, limit, lo, hi))
    return C.c_void_p(t.data_ptr())


def swap_pair(mu, ig, il, Lg, zcat, check_range=True):
    """sv_swap_pair: zcat [B, Lg+Ll] (fp32 or bf16, contiguous) <- [mu[ig, :Lg] | mu[il, Lg:]] of mu [N, Lg+Ll] fp32 (a row pitch above
    the width is allowed); ig, il [B] int32 device tensors in [0, N) (check_range: checked here with one read-back)."""
    mp, ldmu = _rows_f32(mu, "mu")
    N, Lc = mu.shape
    B = int(ig.shape[0]) if torch.is_tensor(ig) and ig.dim() == 1 else -1
    if not 0 < int(Lg) < Lc:
        raise ValueError("swap_pair needs two latent blocks: 0 < Lg < %d, got %r" % (Lc, Lg))
    if B < 1:
        raise ValueError("ig must be a contiguous int32 device tensor of B >= 1 indices")
    lim = N if check_range else None
    gp, lp = _index_i32(ig, B, "ig", lim), _index_i32(il, B, "il", lim)
    if (not torch.is_tensor(zcat) or zcat.dtype not in _SV_DT or not zcat.is_cuda or not zcat.is_contiguous()
            or tuple(zcat.shape) != (B, Lc)):
        raise ValueError("zcat must be a contiguous [%d,%d] fp32 or bf16 device tensor" % (B, Lc))
    check(_lib.load().sv_swap_pair(mp, ldmu, gp, lp, _p(zcat), sv_dtype(zcat.dtype), N, B, int(Lg), Lc - int(Lg), _stream()), "sv_swap_pair")
    return zcat


def swap_requantise(out6, lut, perm, patch, out=None):
    """sv_swap_requantise: out6 [B,H,W,6] fp32 (channels 0..2 read) -> images6 [B,H,W,6] fp32: the decode's mean as pixel levels
    through lut [256] fp32 in channels 0..2, its patch scramble by perm [B,(H/patch)^2] int32 in channels 3..5."""
    if not torch.is_tensor(out6) or out6.dim() != 4 or out6.shape[3] != 6 or out6.dtype != torch.float32 or not out6.is_cuda or not out6.is_contiguous():
        raise ValueError("out6 must be a contiguous [B,H,W,6] fp32 device tensor")
    B, H, W, _ = out6.shape
    if not torch.is_tensor(lut) or lut.dtype != torch.float32 or not lut.is_cuda or not lut.is_contiguous() or tuple(lut.shape) != (256,):
        raise ValueError("lut must be a contiguous [256] fp32 device tensor")
    if H != W or patch < 1 or H % patch:
        raise ValueError("swap_requantise assumes square images and patch | H, got %dx%d, patch %r" % (H, W, patch))
    G2 = (H // patch) * (W // patch)
    if not torch.is_tensor(perm) or perm.dtype != torch.int32 or not perm.is_cuda or not perm.is_contiguous() or tuple(perm.shape) != (B, G2):
        raise ValueError("perm must be a contiguous [%d,%d] int32 device tensor" % (B, G2))
    if out is None:
        out = torch.empty((B, H, W, 6), dtype=torch.float32, device=out6.device)
    if out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous() or tuple(out.shape) != (B, H, W, 6) or out.data_ptr() == out6.data_ptr():
        raise ValueError("out must be a contiguous [%d,%d,%d,6] fp32 device tensor other than out6" % (B, H, W))
    check(_lib.load().sv_swap_requantise(_p(out6), _p(lut), _p(perm), _p(out), B, H, W, int(patch), _stream()), "sv_swap_requantise")
    return out


def swap_rank(q, r, t0, t1, rank=None, workspace=None, check_range=True):
    """sv_swap_rank: rank [Nq,2] int32 = per query row of q [Nq,L] the number of rows of r [Nr,L] that come before row t0[q] / t1[q]
    of r under the order (squared distance of sv_knn_classify, index).  t0, t1 [Nq] int32 device tensors in [0, Nr) (check_range:
    checked here with one read-back).  workspace: a uint8 device tensor of at least swap_rank_workspace_bytes(Nq, Nr, L) bytes."""
    qp, ldq = _rows_f32(q, "q")
    rp, ldr = _rows_f32(r, "r")
    Nq, L = q.shape
    Nr = r.shape[0]
    if r.shape[1] != L or r.device != q.device:
        raise ValueError("q [%d,%d] and r [%d,%d] must have one width and one device" % (Nq, L, Nr, r.shape[1]))
    lim = Nr if check_range else None
    p0, p1 = _index_i32(t0, Nq, "t0", lim), _index_i32(t1, Nq, "t1", lim)
    if rank is None:
        rank = torch.empty((Nq, 2), dtype=torch.int32, device=q.device)
    if rank.dtype != torch.int32 or not rank.is_cuda or not rank.is_contiguous() or tuple(rank.shape) != (Nq, 2):
        raise ValueError("rank must be a contiguous [%d,2] int32 device tensor" % Nq)
    ws = _workspace(swap_rank_workspace_bytes(Nq, Nr, L), workspace, q.device)
    check(_lib.load().sv_swap_rank(qp, ldq, rp, ldr, p0, p1, Nq, Nr, L, _p(rank), _p(ws), ws.numel(), _stream()), "sv_swap_rank")
    return rank


# ------------------------------------------------------------------ sample-quality report of prior draws (include/splitvae.h)
def prdc_chunk_rows():
    return int(_lib.load().sv_prdc_chunk_rows())


def prdc_workspace_bytes(Nq, Nr, L, k):
    n = C.c_int64()
    check(_lib.load().sv_prdc_workspace_bytes(int(Nq), int(Nr), int(L), int(k), C.byref(n)), "sv_prdc_workspace_bytes")
    return n.value


def _vec(t, n, dtype, name):
    if not torch.is_tensor(t) or t.dtype != dtype or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != (n,):
        raise ValueError("%s must be a contiguous %s device tensor of %d elements" % (name, str(dtype).replace("torch.", ""), n))
    return t


def prdc_radius(x, k, rad=None, workspace=None):
    """sv_prdc_radius: rad [N] fp32 = per row i of x [N,L] the k-th smallest squared distance (sv_knn_classify's, ties to the lower
    index) to the OTHER rows: self is excluded by index, a duplicate at another index is a neighbour at distance 0.  1 <= k <= 31,
    N >= k + 1.  workspace: a uint8 device tensor of at least prdc_workspace_bytes(N, N, L, k) bytes."""
    xp, ldx = _rows_f32(x, "x")
    N, L = x.shape
    if not 1 <= int(k) <= _lib.PRDC_MAX_K or N < int(k) + 1:
        raise ValueError("prdc_radius needs 1 <= k <= %d and N >= k + 1, got k = %r, N = %d" % (_lib.PRDC_MAX_K, k, N))
    rad = torch.empty((N,), dtype=torch.float32, device=x.device) if rad is None else _vec(rad, N, torch.float32, "rad")
    ws = _workspace(prdc_workspace_bytes(N, N, L, k), workspace, x.device)
    check(_lib.load().sv_prdc_radius(xp, ldx, N, L, int(k), _p(rad), _p(ws), ws.numel(), _stream()), "sv_prdc_radius")
    return rad


def prdc_count(q, r, rad, cnt=None, dmin=None, imin=None, want_min=True, workspace=None):
    """sv_prdc_count: per query row of q [Nq,L] against r [Nr,L] with the references' radii rad [Nr] fp32: cnt [Nq] int32 =
    #{j : d(q,j) <= rad[j]}, dmin [Nq] fp32 = min_j d(q,j), imin [Nq] int32 = the lowest j that attains it (d sv_knn_classify's squared
    distance).  -> (cnt, dmin, imin), or cnt alone with want_min False.  workspace: a uint8 device tensor of at least
    prdc_workspace_bytes(Nq, Nr, L, 1) bytes."""
    qp, ldq = _rows_f32(q, "q")
    rp, ldr = _rows_f32(r, "r")
    Nq, L = q.shape
    Nr = r.shape[0]
    if r.shape[1] != L or r.device != q.device:
        raise ValueError("q [%d,%d] and r [%d,%d] must have one width and one device" % (Nq, L, Nr, r.shape[1]))
    _vec(rad, Nr, torch.float32, "rad")
    e = lambda dt: torch.empty((Nq,), dtype=dt, device=q.device)      # noqa: E731
    cnt = e(torch.int32) if cnt is None else _vec(cnt, Nq, torch.int32, "cnt")
    if want_min:
        dmin = e(torch.float32) if dmin is None else _vec(dmin, Nq, torch.float32, "dmin")
        imin = e(torch.int32) if imin is None else _vec(imin, Nq, torch.int32, "imin")
    elif dmin is not None or imin is not None:
        raise ValueError("prdc_count: dmin / imin given with want_min False")
    ws = _workspace(prdc_workspace_bytes(Nq, Nr, L, 1), workspace, q.device)
    check(_lib.load().sv_prdc_count(qp, ldq, rp, ldr, _p(rad), Nq, Nr, L, _p(cnt), _p(dmin), _p(imin), _p(ws), ws.numel(), _stream()),
          "sv_prdc_count")
    return (cnt, dmin, imin) if want_min else cnt


# ------------------------------------------------------------------ aggregate-posterior information report (include/splitvae.h)
def latent_info_chunk_rows():
    return int(_lib.load().sv_latent_info_chunk_rows())


def latent_info_workspace_bytes(Nq, Nr):
    n = C.c_int64()
    check(_lib.load().sv_latent_info_workspace_bytes(int(Nq), int(Nr), C.byref(n)), "sv_latent_info_workspace_bytes")
    return n.value


def _same_rows(t, name, N, Lc, device):
    p, ld = _rows_f32(t, name)
    if tuple(t.shape) != (N, Lc) or t.device != device:
        raise ValueError("%s must be [%d,%d] on %s, got %s" % (name, N, Lc, device, tuple(t.shape)))
    return p, ld


def latent_info_draw(mu, sig, Lg, eps=None, seed=0, sample_offset=0, out=None):
    """sv_latent_info_draw: mu, sig [N, Lg+Ll] fp32 (columns 0 .. Lg-1: z_g, the rest: z_l) -> (z, rsig [N, Lg+Ll] fp32, cst [N,2]
    fp32, own [N,2], prior [N,2] fp64).  eps [N, Lg+Ll] pins the draw; otherwise image sample_offset + b draws from (seed, image,
    block).  out: that 5-tuple, to write into (z and rsig may have a row pitch above their width)."""
    mp, ldm = _rows_f32(mu, "mu")
    N, Lc = mu.shape
    dev = mu.device
    sp, lds = _same_rows(sig, "sig", N, Lc, dev)
    ep, lde = (None, 0) if eps is None else _same_rows(eps, "eps", N, Lc, dev)
    if out is None:
        f32, f64 = torch.float32, torch.float64
        out = (torch.empty((N, Lc), dtype=f32, device=dev), torch.empty((N, Lc), dtype=f32, device=dev),
               torch.empty((N, 2), dtype=f32, device=dev), torch.empty((N, 2), dtype=f64, device=dev), torch.empty((N, 2), dtype=f64, device=dev))
    z, rsig, cst, own, prior = out
    zp, ldz = _same_rows(z, "z", N, Lc, dev)
    rp, ldr = _same_rows(rsig, "rsig", N, Lc, dev)
    for t, dt, name in ((cst, torch.float32, "cst"), (own, torch.float64, "own"), (prior, torch.float64, "prior")):
        if t.dtype != dt or tuple(t.shape) != (N, 2) or not t.is_contiguous() or t.device != dev:
            raise ValueError("%s must be a contiguous [%d,2] %s device tensor" % (name, N, dt))
    check(_lib.load().sv_latent_info_draw(mp, ldm, sp, lds, ep, lde, zp, ldz, rp, ldr, _p(cst), _p(own), _p(prior), N, int(Lg), Lc - int(Lg),
                                          int(seed), int(sample_offset), _stream()), "sv_latent_info_draw")
    return out


def latent_info_lse(z, mu, rsig, cst, Lg, lse=None, workspace=None):
    """sv_latent_info_lse: lse [3, Nq] fp64 = (lse_g, lse_l, lse_gl) of the queries z [Nq, Lg+Ll] under the references mu, rsig
    [Nr, Lg+Ll], cst [Nr,2] (rows 1 and 2 are not written when Ll = 0).  workspace: a uint8 device tensor of at least
    latent_info_workspace_bytes(Nq, Nr) bytes with any contents (default: allocated here)."""
    zp, ldz = _rows_f32(z, "z")
    Nq, Lc = z.shape
    Nr = mu.shape[0]
    dev = z.device
    mp, ldm = _same_rows(mu, "mu", Nr, Lc, dev)
    rp, ldr = _same_rows(rsig, "rsig", Nr, Lc, dev)
    if cst.dtype != torch.float32 or tuple(cst.shape) != (Nr, 2) or not cst.is_contiguous() or cst.device != dev:
        raise ValueError("cst must be a contiguous [%d,2] fp32 device tensor" % Nr)
    if lse is None:
        lse = torch.empty((3, Nq), dtype=torch.float64, device=dev)
    if lse.dtype != torch.float64 or tuple(lse.shape) != (3, Nq) or not lse.is_contiguous() or lse.device != dev:
        raise ValueError("lse must be a contiguous [3,%d] fp64 device tensor" % Nq)
    ws = _workspace(latent_info_workspace_bytes(Nq, Nr), workspace, dev)
    check(_lib.load().sv_latent_info_lse(zp, ldz, mp, ldm, rp, ldr, _p(cst), Nq, Nr, int(Lg), Lc - int(Lg), _p(lse), _p(ws), ws.numel(),
                                         _stream()), "sv_latent_info_lse")
    return lse


def latent_info_finish(own, prior, lse, Ll, out=None):
    """sv_latent_info_finish: out [8] fp64 = (KL_g, MI_g, marginal KL_g, KL_l, MI_l, marginal KL_l, overlap, log N)."""
    N = own.shape[0]
    f64 = torch.float64
    if out is None:
        out = torch.empty((8,), dtype=f64, device=own.device)
    if not all(t.dtype == f64 and t.is_contiguous() and t.is_cuda for t in (own, prior, lse, out)) or tuple(own.shape) != (N, 2) or \
            tuple(prior.shape) != (N, 2) or tuple(lse.shape) != (3, N) or out.numel() < 8:
        raise ValueError("own, prior [N,2], lse [3,N] and out [8] must be contiguous fp64 device tensors")
    check(_lib.load().sv_latent_info_finish(_p(own), _p(prior), _p(lse), N, int(Ll), _p(out), _stream()), "sv_latent_info_finish")
    return out


# ------------------------------------------------------------------ per-dimension latent report (include/splitvae.h)
def latent_dims_chunk_rows():
    return int(_lib.load().sv_latent_dims_chunk_rows())


def latent_dims_workspace_bytes(Nq, Nr, L):
    n = C.c_int64()
    check(_lib.load().sv_latent_dims_workspace_bytes(int(Nq), int(Nr), int(L), C.byref(n)), "sv_latent_dims_workspace_bytes")
    return n.value


def _dense_f64(t, name, shape, device):
    if not torch.is_tensor(t) or t.dtype != torch.float64 or tuple(t.shape) != tuple(shape) or not t.is_contiguous() or t.device != device:
        raise ValueError("%s must be a contiguous %s fp64 tensor on %s" % (name, list(shape), device))
    return _p(t)


def _rows_f64(t, name, shape, device):
    if not torch.is_tensor(t) or t.dim() != 2 or t.dtype != torch.float64 or tuple(t.shape) != tuple(shape) or t.device != device or \
            t.stride(1) != 1 or t.stride(0) < t.shape[1]:
        raise ValueError("%s must be a %s fp64 tensor on %s with contiguous rows (a row pitch >= its width is allowed)" %
                         (name, list(shape), device))
    return C.c_void_p(t.data_ptr()), int(t.stride(0))


def latent_dims_prepare(mu, sig, eps=None, block=0, seed=0, sample_offset=0, out=None):
    """sv_latent_dims_prepare: mu, sig [N, L] fp32 of ONE block (column views of wider arrays are fine) -> (lc [N,L] fp32, own [N,L]
    fp64, cols [3,L] fp64 = mean_j, var_j, KL_j).  eps [N,L] pins the draw; otherwise the numbers ops.latent_info_draw drew for
    (seed, sample_offset + i, block).  out: that 3-tuple, to write into (lc may have a row pitch above its width)."""
    mp, ldm = _rows_f32(mu, "mu")
    N, L = mu.shape
    dev = mu.device
    sp, lds = _same_rows(sig, "sig", N, L, dev)
    ep, lde = (None, 0) if eps is None else _same_rows(eps, "eps", N, L, dev)
    if out is None:
        out = (torch.empty((N, L), dtype=torch.float32, device=dev), torch.empty((N, L), dtype=torch.float64, device=dev),
               torch.empty((3, L), dtype=torch.float64, device=dev))
    lc, own, cols = out
    cp, ldc = _same_rows(lc, "lc", N, L, dev)
    op, kp = _dense_f64(own, "own", (N, L), dev), _dense_f64(cols, "cols", (3, L), dev)
    check(_lib.load().sv_latent_dims_prepare(mp, ldm, sp, lds, ep, lde, cp, ldc, op, kp, N, L, int(block), int(seed), int(sample_offset),
                                             _stream()), "sv_latent_dims_prepare")
    return out


def latent_dims_lse(z, mu, rsig, lc, lse=None, workspace=None):
    """sv_latent_dims_lse: lse [Nq, L] fp64, lse_ij = logsumexp_n log q(z_ij | x_n) - log Nr of the queries z [Nq, L] under the
    references mu, rsig, lc [Nr, L] (fp32; each may have a row pitch above L).  workspace: a uint8 device tensor of at least
    latent_dims_workspace_bytes(Nq, Nr, L) bytes with any contents (default: allocated here)."""
    zp, ldz = _rows_f32(z, "z")
    Nq, L = z.shape
    Nr = mu.shape[0]
    dev = z.device
    mp, ldm = _same_rows(mu, "mu", Nr, L, dev)
    rp, ldr = _same_rows(rsig, "rsig", Nr, L, dev)
    cp, ldc = _same_rows(lc, "lc", Nr, L, dev)
    if lse is None:
        lse = torch.empty((Nq, L), dtype=torch.float64, device=dev)
    lp, ldl = _rows_f64(lse, "lse", (Nq, L), dev)
    ws = _workspace(latent_dims_workspace_bytes(Nq, Nr, L), workspace, dev)
    check(_lib.load().sv_latent_dims_lse(zp, ldz, mp, ldm, rp, ldr, cp, ldc, Nq, Nr, L, lp, ldl, _p(ws), ws.numel(), _stream()),
          "sv_latent_dims_lse")
    return lse


def latent_dims_finish(lse, own, z, lse_block, out=None):
    """sv_latent_dims_finish: out [3 L + 2] fp64 = (MI_j [L], dwKL_j [L], mean_i lse_ij [L], TC, dwKL) of lse [N,L] (latent_dims_lse
    with Nq = Nr = N), own [N,L] (latent_dims_prepare), the samples z [N,L] fp32 and lse_block [N] fp64: the block's row of
    ops.latent_info_lse on the same z."""
    zp, ldz = _rows_f32(z, "z")
    N, L = z.shape
    dev = z.device
    lp, ldl = _rows_f64(lse, "lse", (N, L), dev)
    op, bp = _dense_f64(own, "own", (N, L), dev), _dense_f64(lse_block, "lse_block", (N,), dev)
    if out is None:
        out = torch.empty((3 * L + 2,), dtype=torch.float64, device=dev)
    qp = _dense_f64(out, "out", (3 * L + 2,), dev)
    check(_lib.load().sv_latent_dims_finish(lp, ldl, op, zp, ldz, bp, N, L, qp, _stream()), "sv_latent_dims_finish")
    return out


# ------------------------------------------------------------------ label-free reconstruction quality (include/splitvae.h)
def recon_window():
    """The 11 fp64 taps of the SSIM window (sigma 1.5, normalised to sum 1) as the kernel uses them."""
    w = (C.c_double * 11)()
    _lib.load().sv_recon_window(w)
    return list(w)


def recon_quality_workspace_bytes(B, H, W):
    n = C.c_int64()
    check(_lib.load().sv_recon_quality_workspace_bytes(int(B), int(H), int(W), C.byref(n)), "sv_recon_quality_workspace_bytes")
    return n.value


def recon_draw(z_mean_x, z_mean_xh, mode, zcat, eps=None, comp=None, prior=None, seed=0, sample_offset=0):
    """sv_recon_draw: zcat [B, Lg+Ll] (fp32 or bf16; a row pitch above its width is allowed) = [z_g | z_l] from the posterior means
    z_mean_x [B,Lg], z_mean_xh [B,Ll] (None: Ll = 0).  mode: _lib.RECON_MEANS | RECON_KEEP_G (z_l ~ N(0, I)) | RECON_KEEP_L (z_g ~ its
    prior: N(0, I), or with prior = (pm, ps) [n, Lg] the uniform mixture over their rows).  eps [B, Lg+Ll] pins the normals, comp [B]
    int32 the components; otherwise image sample_offset + b draws from (seed, image, mode, block)."""
    gp, ldg = _rows_f32(z_mean_x, "z_mean_x")
    B, Lg = z_mean_x.shape
    dev = z_mean_x.device
    lp, ldl, Ll = None, 0, 0
    if z_mean_xh is not None:
        Ll = int(z_mean_xh.shape[1])
        lp, ldl = _same_rows(z_mean_xh, "z_mean_xh", B, Ll, dev)
    Lc = Lg + Ll
    ep, lde = (None, 0) if eps is None else _same_rows(eps, "eps", B, Lc, dev)
    if not torch.is_tensor(zcat) or zcat.dtype not in _SV_DT or tuple(zcat.shape) != (B, Lc) or zcat.device != dev or zcat.stride(1) != 1 or \
            zcat.stride(0) < Lc:
        raise ValueError("zcat must be a [%d,%d] fp32 / bf16 device tensor with contiguous rows" % (B, Lc))
    if comp is not None and (comp.dtype != torch.int32 or tuple(comp.shape) != (B,) or not comp.is_contiguous() or comp.device != dev):
        raise ValueError("comp must be a contiguous [%d] int32 device tensor" % B)
    pmp, psp, n = None, None, 0
    if prior is not None:
        pm, ps = prior
        n = int(pm.shape[0])
        for t, name in ((pm, "pm"), (ps, "ps")):
            if t.dtype != torch.float32 or tuple(t.shape) != (n, Lg) or not t.is_contiguous() or t.device != dev:
                raise ValueError("%s must be a contiguous [n,%d] fp32 device tensor" % (name, Lg))
        pmp, psp = _p(pm), _p(ps)
    check(_lib.load().sv_recon_draw(gp, ldg, lp, ldl, int(mode), ep, lde, _p(comp), pmp, psp, n, C.c_void_p(zcat.data_ptr()),
                                    int(zcat.stride(0)), sv_dtype(zcat.dtype), B, Lg, Ll, int(seed), int(sample_offset), _stream()),
          "sv_recon_draw")
    return zcat


def _nhwc_f32(t, name, off):
    if not torch.is_tensor(t) or t.dim() != 4 or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
        raise ValueError("%s must be a contiguous [B,H,W,C] fp32 device tensor" % name)
    if not 0 <= int(off) <= t.shape[3] - 3:
        raise ValueError("%s: channels %d .. %d of %d" % (name, off, off + 2, t.shape[3]))
    return _p(t), int(t.shape[3])


def recon_quality(a, b, off_a=0, off_b=0, clip_b=True, per_image=None, workspace=None):
    """sv_recon_quality: per_image [B,2] fp64 = (MSE_i, SSIM_i) of channels off_a .. off_a+2 of a [B,H,W,Ca] (the image in [-1,1])
    against channels off_b .. off_b+2 of b [B,H,W,Cb] (the decoder mean), both rescaled by (x + 1) / 2 and b clipped to [0,1] when
    clip_b; both are read in place.  workspace: a uint8 device tensor of at least recon_quality_workspace_bytes(B, H, W) bytes with any
    contents (default: allocated here)."""
    ap, pa = _nhwc_f32(a, "a", off_a)
    bp, pb = _nhwc_f32(b, "b", off_b)
    B, H, W = a.shape[:3]
    if tuple(b.shape[:3]) != (B, H, W) or b.device != a.device:
        raise ValueError("a %s and b %s must share B, H, W and the device" % (tuple(a.shape), tuple(b.shape)))
    if per_image is None:
        per_image = torch.empty((B, 2), dtype=torch.float64, device=a.device)
    if per_image.dtype != torch.float64 or tuple(per_image.shape) != (B, 2) or not per_image.is_contiguous() or per_image.device != a.device:
        raise ValueError("per_image must be a contiguous [%d,2] fp64 device tensor" % B)
    ws = _workspace(recon_quality_workspace_bytes(B, H, W), workspace, a.device)
    check(_lib.load().sv_recon_quality(ap, pa, int(off_a), bp, pb, int(off_b), int(bool(clip_b)), B, H, W, _p(per_image), _p(ws), ws.numel(),
                                       _stream()), "sv_recon_quality")
    return per_image


def recon_finish(per_image, acc, n=None):
    """sv_recon_finish: acc [3] fp64 += (sum PSNR_i, sum SSIM_i, n) over the first n rows of per_image [B,2] (default: all)."""
    f64 = torch.float64
    if per_image.dtype != f64 or per_image.dim() != 2 or per_image.shape[1] != 2 or not per_image.is_contiguous() or not per_image.is_cuda:
        raise ValueError("per_image must be a contiguous [B,2] fp64 device tensor")
    n = per_image.shape[0] if n is None else int(n)
    if not 1 <= n <= per_image.shape[0]:
        raise ValueError("recon_finish: n = %d of %d images" % (n, per_image.shape[0]))
    if acc.dtype != f64 or acc.numel() != 3 or not acc.is_contiguous() or acc.device != per_image.device:
        raise ValueError("acc must be a contiguous [3] fp64 device tensor")
    check(_lib.load().sv_recon_finish(_p(per_image), n, _p(acc), _stream()), "sv_recon_finish")
    return acc


# ------------------------------------------------------------------ A9 SPLIT-GMVAE glue (vae/model.py:48-79,:116-135)
ACT ={None: _lib.SV_ACT_NONE, "relu": _lib.SV_ACT_RELU, "elu": _lib.SV_ACT_ELU}


def act_fwd(a, C_, x, act=None, y_act=None, rate=0.0, keep_in=None, keep_out=None, seed=0, step=0, stream_id=0,
            sample_offset=0, rows_per_sample=1):
    """x[r, :C] = dropout(act(a[r, :C])), padding columns of x zeroed; a, x 2-D views [rows, ld]."""
    rows = a.shape[0]
    check(_lib.load().sv_act_fwd(_p(a), sv_dtype(a.dtype), a.shape[1], _p(y_act), _p(x), sv_dtype(x.dtype), x.shape[1], rows, C_,
                                 ACT[act], float(rate), _p(keep_in), _p(keep_out), seed, step, stream_id, sample_offset,
                                 rows_per_sample, _stream()), "sv_act_fwd")
    return x


def act_bwd(gx, C_, ga, y_act=None, act=None, rate=0.0, keep=None, gx2=None):
    rows = gx.shape[0]
    check(_lib.load().sv_act_bwd(_p(gx), sv_dtype(gx.dtype), gx.shape[1], _p(gx2), sv_dtype(gx2.dtype) if gx2 is not None else 0,
                                 gx2.shape[1] if gx2 is not None else 0, _p(y_act),
                                 sv_dtype(y_act.dtype) if y_act is not None else 0, y_act.shape[1] if y_act is not None else 0,
                                 ACT[act], float(rate), _p(keep), _p(ga), sv_dtype(ga.dtype), ga.shape[1], rows, C_, _stream()),
          "sv_act_bwd")
    return ga


def add(a, b, out):
    check(_lib.load().sv_add(_p(a), _p(b), _p(out), sv_dtype(out.dtype), out.numel(), _stream()), "sv_add")
    return out


def gm_metrics(nll_x, kl_x, nll_xh, kl_xh, y_kl, beta, alpha, out6):
    """vae/trainer.py:157-173: the five batch means + total (include/splitvae.h: sv_gm_metrics)."""
    check(_lib.load().sv_gm_metrics(_p(nll_x), _p(kl_x), _p(nll_xh), _p(kl_xh), _p(y_kl), nll_x.numel(), float(beta), float(alpha),
                                    _p(out6), _stream()), "sv_gm_metrics")
    return out6


def cluster_confusion(logits, labels_onehot, counts):
    """counts[K, C] (int32, accumulated into) += the (argmax logits, argmax label) pairs of the rows (include/splitvae.h:
    sv_cluster_confusion).  logits [B, >=K] / labels_onehot [B, >=C] fp32 rows."""
    B = logits.shape[0]
    K, C_ = counts.shape
    assert labels_onehot.shape[0] == B and counts.dtype == torch.int32
    check(_lib.load().sv_cluster_confusion(_p(logits), logits.shape[1], _p(labels_onehot), labels_onehot.shape[1], B, K, C_, _p(counts),
                                           _stream()), "sv_cluster_confusion")
    return counts


def gumbel_softmax_fwd(logits, K, tau, y, y_lp, u=None, u_out=None, seed=0, step=0, sample_offset=0):
    B = logits.shape[0]
    check(_lib.load().sv_gumbel_softmax_fwd(_p(logits), logits.shape[1], _p(u), _p(u_out), float(tau), _p(y), _p(y_lp),
                                            sv_dtype(y_lp.dtype), y_lp.shape[1], B, K, seed, step, sample_offset, _stream()),
          "sv_gumbel_softmax_fwd")


def gumbel_softmax_bwd(gy, y, logits, K, tau, alpha_over_B, g_logits, y_kl):
    B = logits.shape[0]
    check(_lib.load().sv_gumbel_softmax_bwd(_p(gy), gy.shape[1] if gy is not None else 0, _p(y), _p(logits), logits.shape[1],
                                            float(tau), float(alpha_over_B), _p(g_logits),
                                            sv_dtype(g_logits.dtype) if g_logits is not None else 0,
                                            g_logits.shape[1] if g_logits is not None else 0, _p(y_kl), B, K, _stream()),
          "sv_gumbel_softmax_bwd")


def gm_head_fwd(a_m, a_s, a_pm, a_ps, zm, zs, z, pm, ps, zcat, z_col, kl2, eps=None, eps_out=None, seed=0, step=0,
                sample_offset=0):
    B, L = a_m.shape
    check(_lib.load().sv_gm_head_fwd(_p(a_m), _p(a_s), _p(a_pm), _p(a_ps), _p(eps), _p(eps_out), _p(zm), _p(zs), _p(z), _p(pm),
                                     _p(ps), _p(zcat), sv_dtype(zcat.dtype), zcat.shape[1], z_col, _p(kl2), B, L, seed, step,
                                     sample_offset, _stream()), "sv_gm_head_fwd")


def gm_head_bwd(dz, zm, zs, pm, ps, eps, kl_scale, g_am, g_as, g_apm, g_aps):
    B, L = zm.shape
    check(_lib.load().sv_gm_head_bwd(_p(dz), dz.shape[1], _p(zm), _p(zs), _p(pm), _p(ps), _p(eps), float(kl_scale), _p(g_am),
                                     _p(g_as), _p(g_apm), _p(g_aps), sv_dtype(g_am.dtype), B, L, _stream()), "sv_gm_head_bwd")


# ---------------------------------------------------------------- SPLIT-SPAIR Dense layers (dense_f32.hip)
def _pr(t):
    """Pointer of a 2-D tensor whose rows are contiguous (any row pitch)."""
    assert t.is_cuda and t.dim() == 2 and t.stride(1) == 1 and t.dtype == torch.float32
    return C.c_void_p(t.data_ptr())


def dense_f32_fwd(x, w, bias=None, act=None):
    """y = act(x . w + bias) for x [M, K] fp32 (row pitch = x.stride(0)), w [K, N] (Keras Dense kernel): exact-fp32 MFMA."""
    M, K = x.shape
    N = w.shape[1]
    y = torch.empty((M, N), dtype=torch.float32, device=x.device)
    check(_lib.load().sv_dense_f32_fwd(_pr(x), x.stride(0), _p(w), _p(bias), _p(y), N, M, K, N, 1 if act == "relu" else 0, _stream()),
          "sv_dense_f32_fwd")
    return y


def dense_f32_dgrad(dy, w, out=None):
    """dx = dy . w^T; out: an fp32 [M, K] tensor the product is ADDED to (atomics, K split over workgroups)."""
    M, N = dy.shape
    K = w.shape[0]
    dx = out if out is not None else torch.empty((M, K), dtype=torch.float32, device=dy.device)
    check(_lib.load().sv_dense_f32_dgrad(_pr(dy), dy.stride(0), _p(w), _pr(dx), dx.stride(0), M, K, N, 1 if out is not None else 0, _stream()),
          "sv_dense_f32_dgrad")
    return dx


def dense_f32_wgrad(x, dy):
    """(dw [K, N], dbias [N]) = (x^T . dy, column sums of dy)."""
    M, K = x.shape
    N = dy.shape[1]
    dw = torch.zeros((K, N), dtype=torch.float32, device=x.device)
    db = torch.zeros((N,), dtype=torch.float32, device=x.device)
    check(_lib.load().sv_dense_f32_wgrad(_pr(x), x.stride(0), _pr(dy), dy.stride(0), _p(dw), _p(db), M, K, N, _stream()), "sv_dense_f32_wgrad")
    return dw, db


# ---------------------------------------------------------------- the latent block's kernels, one by one (latent_gemm.hip)
def _pany(t):
    """Pointer of a device tensor or view (the caller states the pitches)."""
    if t is None:
        return None
    assert t.is_cuda
    return t.data_ptr()


def latent_nt_pick_splitk(M, N, K, nprob):
    return int(_lib.load().sv_latent_nt_pick_splitk(M, N, K, nprob))


def latent_nt_gemm(probs, dtype, bm=64):
    """sv_latent_nt_gemm over 1 or 2 problems, each a dict: A [M, K] and W [N, K] (2-D views, last dimension contiguous, the row stride is
    the pitch), out (tensor or view: its data pointer), ldo, and optionally bias, mask, act ("relu"), splitk (0: the plan's pick), out_f32,
    slab_stride.  Returns (form, [splitk that ran per problem]); form 0 = the one-slot kernel, 1 = the ring."""
    arr = (_lib.LatentNtProb * len(probs))()
    for g, q in zip(arr, probs):
        A, W = q["A"], q["W"]
        assert A.dim() == 2 and W.dim() == 2 and A.stride(1) == 1 and W.stride(1) == 1 and A.shape[1] == W.shape[1]
        g.A, g.lda, g.W, g.ldw = _pany(A), A.stride(0), _pany(W), W.stride(0)
        g.out, g.ldo, g.bias, g.mask = _pany(q["out"]), q["ldo"], _pany(q.get("bias")), _pany(q.get("mask"))
        g.M, g.N, g.K = A.shape[0], W.shape[0], A.shape[1]
        g.act = 1 if q.get("act") == "relu" else 0
        g.splitk, g.out_f32, g.slab_stride = q.get("splitk", 1), int(bool(q.get("out_f32"))), q.get("slab_stride", 0)
    form = C.c_int32(-1)
    check(_lib.load().sv_latent_nt_gemm(arr, len(probs), sv_dtype(dtype), bm, C.byref(form), _stream()), "sv_latent_nt_gemm")
    return form.value, [g.splitk for g in arr]


def latent_nt_slab_reduce(probs):
    """sv_latent_nt_slab_reduce over 1 or 2 problems, each a dict: slabs, out (fp32 tensors or views), S, M, ldo, slab_stride."""
    arr = (_lib.LatentReduceProb * len(probs))()
    for g, q in zip(arr, probs):
        g.slabs, g.out, g.S, g.M, g.ldo, g.slab_stride = _pany(q["slabs"]), _pany(q["out"]), q["S"], q["M"], q["ldo"], q["slab_stride"]
    check(_lib.load().sv_latent_nt_slab_reduce(arr, len(probs), _stream()), "sv_latent_nt_slab_reduce")


def latent_tn_wgrad(probs, dtype):
    """sv_latent_tn_wgrad over 1 .. 4 problems, each a dict: X [M, Kw] and dY [M, N] (2-D views, the row stride is the pitch), dW (fp32, row
    pitch N), dbias (fp32 or None), Kw_real (default Kw)."""
    arr = (_lib.LatentTnProb * len(probs))()
    for g, q in zip(arr, probs):
        X, dY = q["X"], q["dY"]
        assert X.dim() == 2 and dY.dim() == 2 and X.stride(1) == 1 and dY.stride(1) == 1 and X.shape[0] == dY.shape[0]
        g.X, g.ldx, g.dY, g.ldy, g.dW, g.dbias = _pany(X), X.stride(0), _pany(dY), dY.stride(0), _pany(q["dW"]), _pany(q.get("dbias"))
        g.M, g.Kw, g.Kw_real, g.N = X.shape[0], X.shape[1], q.get("Kw_real", X.shape[1]), dY.shape[1]
    check(_lib.load().sv_latent_tn_wgrad(arr, len(probs), sv_dtype(dtype), _stream()), "sv_latent_tn_wgrad")


def reparam_kl_fwd_twin(nets, z_lp, ldz, B, seed=0, step=0, sample_offset=0):
    """sv_reparam_kl_fwd_twin: nets = two dicts with pre, bias_mean, bias_sd, eps, eps_out, z_mean, z_sig, z, kl, L, z_col and, for K-slice
    slabs, S and slab_stride; z_lp the shared [B, ldz] decoder input (bf16 or fp32)."""
    arr = (_lib.ReparamTwinFwd * 2)()
    for g, q in zip(arr, nets):
        for k in ("pre", "bias_mean", "bias_sd", "eps", "eps_out", "z_mean", "z_sig", "z", "kl"):
            setattr(g, k, _pany(q.get(k)))
        g.L, g.z_col, g.S, g.slab_stride = q["L"], q["z_col"], q.get("S", 0), q.get("slab_stride", 0)
    check(_lib.load().sv_reparam_kl_fwd_twin(arr, _pany(z_lp), sv_dtype(z_lp.dtype), ldz, B, seed, step, sample_offset, _stream()),
          "sv_reparam_kl_fwd_twin")


def reparam_kl_bwd_twin(nets, kl_scale, g_dtype, B):
    """sv_reparam_kl_bwd_twin: nets = two dicts with dz, ld_dz, dz2 (or None), ld_dz2, z_mean, z_sig, eps, g_pre, L and, for slabs, S, stride,
    S2, stride2."""
    arr = (_lib.ReparamTwinBwd * 2)()
    for g, q in zip(arr, nets):
        for k in ("dz", "dz2", "z_mean", "z_sig", "eps", "g_pre"):
            setattr(g, k, _pany(q.get(k)))
        g.ld_dz, g.ld_dz2, g.L = q["ld_dz"], q.get("ld_dz2", 0), q["L"]
        g.S, g.S2, g.stride, g.stride2 = q.get("S", 0), q.get("S2", 0), q.get("stride", 0), q.get("stride2", 0)
    check(_lib.load().sv_reparam_kl_bwd_twin(arr, float(kl_scale), sv_dtype(g_dtype), B, _stream()), "sv_reparam_kl_bwd_twin")
