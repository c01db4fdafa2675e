"""CLI mirror of spair/main.py:19-50 (same flag names and defaults) for SPAIR / SPLIT-SPAIR.

    python -m split_vae_amd.spair_main --dataset cub_solid_fixed --z_bg_beta 10 --patch_size 8 --latent_size 64 --bg_latent_size 4 \\
        --local_latent_size 4 --model lg_spair -split_z_l -concat_z_what -dense_local -dense_bg --training_steps 200 --synthetic

--dataset cub_solid_fixed | cub_ckb_rot_6: the Multi-Bird canvases of spair/data.py, synthesised on the device (multibird.py,
csrc/multibird.hip) with the reference's two test sets (seen / unseen colours).  The CUB sprite blobs are not in the reference's
repository (spair/data.py:14-15): they are read from --data_dir when present, a procedural stand-in bank is used otherwise.
--synthetic: 48x48x3 canvases in [0,1] with 0-5 soft-edged blobs on a solid background and the blob count as the label.
Extra flags (not in the reference): --synthetic, --data_dir, --seed, --log_every, --graph, --dtype, -viz, --detection_ap.
"""
import argparse

import torch

from .utils import dotdict

REFERENCE_SWITCHES = ["-no_label", "-allow_growth", "-split_z_l", "-dense_bg", "-dense_local", "-concat_bg", "-concat_z_what",
                      "-concat_backbone"]
REFERENCE_OPTIONS = [
    ("--learning_rate", float, 1e-4), ("--beta", float, 0.5), ("--dataset", str, "cub_solid_fixed"), ("--channel", int, 3),
    ("--training_steps", int, 100000), ("--batch_size", int, 32), ("--runs", int, 1), ("--tau", float, 0.8), ("--object_size", int, 32),
    ("--latent_size", int, 128), ("--anneal_until", float, 1.0), ("--z_pres_anneal_step", float, 10000.0), ("--prior_z_zoom", float, 0.0),
    ("--prior_z_zoom_start", float, 10.0), ("--reconstruction_weight", float, 1.0), ("--bg_latent_size", int, 4),
    ("--local_latent_size", int, 64), ("--z_bg_beta", float, 10.0), ("--z_l_beta", float, 0.1), ("--z_what_beta", float, 0.1),
    ("--model", str, "spair"), ("--patch_size", int, 4), ("--augmentation", str, "scramble"),
]


def build_parser():
    ap = argparse.ArgumentParser(description="SPAIR / SPLIT-SPAIR training on MI355X (flags of the reference's spair/main.py)")
    for sw in REFERENCE_SWITCHES:
        ap.add_argument(sw, action="store_true")
    for flag, ty, default in REFERENCE_OPTIONS:
        ap.add_argument(flag, type=ty, nargs="?", default=default)
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--data_dir", type=str, default="data",
                    help="where the Multi-Bird sprite banks (cub_{train,test}_seg_14x14_pad_20_masked.npy) or multi_cub/*.tfrec are looked for; "
                         "without them the canvases use a procedural stand-in bank (split_vae_amd/multibird.py)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--log_every", type=int, default=1000)
    ap.add_argument("--dtype", type=str, default="f32", choices=["f32", "bf16"],
                    help="bf16: the spatial convolutions on the bf16 MFMA kernels (fp32 accumulation / master weights); f32 = the reference's precision")
    ap.add_argument("--save_weights", action="store_true", help="write models/<time>.h5 (Keras HDF5 weights) at the end, as spair/trainer.py:424 does")
    ap.add_argument("--clipnorm_semantics", type=str, default="tf2.0", choices=["tf2.0", "tf2.4"],
                    help="Adam(clipnorm=1.0) in a tape.gradient -> apply_gradients loop (spair/main.py:109, spair/trainer.py:226-227): the pinned "
                         "tensorflow_gpu==2.0.0 does not clip in apply_gradients (default); TF >= 2.4 clips every gradient tensor with tf.clip_by_norm")
    ap.add_argument("--graph", action="store_true", help="capture the train step into a hipGraph and replay it (spair_trainer.GraphedTrainStep)")
    ap.add_argument("--mix_per_image", action="store_true",
                    help="--augmentation mix_scramble: a patch size per image instead of one per pipeline (see split_vae_amd/main.py)")
    ap.add_argument("-viz", action="store_true",
                    help="write the reference's figures (train_recon_it_<step>.png, spair/visualizer.py's test figures) under "
                         "output/<RUN_NAME>/ at every log step (spair_visualizer.py)")
    ap.add_argument("--detection_ap", action="store_true",
                    help="report the detection average precision (AP@IoU 0.1 .. 0.9, precision / recall at 0.5) of every test set after "
                         "its count accuracy (split_vae_amd/detection.py); needs the kernel-rendered Multi-Bird canvases, whose "
                         "ground-truth boxes are known")
    return ap


def default_config(**kw):
    c = dotdict(vars(build_parser().parse_args([])))
    c.image_size, c.test_size = [48, 48, 3], [48, 48, 3]
    c.update(kw)
    c.label = not c.no_label
    return c


def synthetic_canvases(B, seed=0, device="cuda", size=48):
    """[B,size,size,3] in [0,1] + the object count per canvas."""
    g = torch.Generator().manual_seed(seed)
    ys = torch.arange(size).view(1, size, 1).float()
    xs = torch.arange(size).view(1, 1, size).float()
    bg = torch.rand(B, 1, 1, 3, generator=g) * 0.5
    img = bg.expand(B, size, size, 3).clone()
    count = torch.randint(0, 6, (B,), generator=g)
    for k in range(5):
        on = (count > k).float().view(B, 1, 1, 1)
        cy, cx = torch.rand(B, 1, 1, generator=g) * size, torch.rand(B, 1, 1, generator=g) * size
        r = 3.0 + torch.rand(B, 1, 1, generator=g) * 5.0
        col = 0.5 + 0.5 * torch.rand(B, 1, 1, 3, generator=g)
        a = torch.sigmoid((r - torch.sqrt((ys - cy) ** 2 + (xs - cx) ** 2)) * 1.5).unsqueeze(-1) * on
        img = img * (1 - a) + col * a
    return img.clamp(0, 1).to(device), count.float().to(device)


def main(argv=None):
    args = build_parser().parse_args(argv)
    from . import configure_hw_queues
    configure_hw_queues()                            # before the first HIP call (split_vae_amd/__init__.py)
    config = dotdict(vars(args))
    config.label = not config.no_label
    print('Config:', config)
    from .main import check_augmentation, make_augmentors
    check_augmentation(config.augmentation, config.model)
    from . import spair, spair_trainer
    config.image_size, config.test_size = [48, 48, config.channel], [48, 48, config.channel]
    augmentor, test_augmentor = make_augmentors(config)
    lg = config.model == 'lg_spair'

    if config.synthetic:
        def batches():
            i = 0
            while True:
                x, _ = synthetic_canvases(config.batch_size, seed=config.seed + 1 + i)
                yield augmentor.augment(x) if lg else x                     # spair/main.py:71-72
                i += 1

        tx, ty = synthetic_canvases(config.batch_size, seed=config.seed + 10 ** 6)
        test_batches = [[(test_augmentor.augment(tx) if lg else tx, ty) if config.label else (test_augmentor.augment(tx) if lg else tx)]]
    else:                                                                   # spair/main.py:71-93 on the device generator
        from . import multibird
        train_ds, test_batches, _, _ = multibird.get_cub_dataset(config.dataset, channel=config.channel, batch_size=config.batch_size,
                                                                  data_dir=config.data_dir, seed=config.seed)

        def batches():
            for x in train_ds:
                yield augmentor.augment(x) if lg else x

        for t in test_batches:
            t.augment, t.label = (test_augmentor.augment if lg else None), bool(config.label)
    if config.detection_ap and not all(getattr(t, "boxes", None) is not None for t in test_batches):
        from . import detection
        print(detection.UNAVAILABLE)                                        # synthetic canvases / TFRecord test sets: no boxes
        config.detection_ap = False
    history = None
    for _ in range(args.runs):
        print('Creating model...')
        model = spair.get_model(config, seed=config.seed)
        print(type(model))
        model.summary()
        optimizer = spair_trainer.ClipnormAdam(config.learning_rate, clipnorm=1.0,         # spair/main.py:109
                                               clip_in_apply=(config.clipnorm_semantics == "tf2.4"))
        print('Training SPAIR')
        history = spair_trainer.train_spair(model, optimizer, config.dataset, batches(), test_batches, config)
    return history


if __name__ == "__main__":
    main()
