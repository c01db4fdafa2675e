"""CLI mirror of vae/main.py:15-31 (same flag names and defaults) for the SPLIT-VAE path.

    python -m split_vae_amd.main --beta 120 --patch_size 8 --dataset celeba64 -no_label --synthetic
    python -m split_vae_amd.main --model gmvae --beta 40 --patch_size 4       (GMVAE baseline, Table 2)

Extra flags (not in the reference): --synthetic, --dtype, --seed, --log_every, --data_dir, --gm_dropout, --mix_per_image,
--resident_data, --iw_samples, --gm_iw_samples, --knn_probe, --knn_refs, --latent_info, --recon_quality, --latent_dims.
"""
import argparse

from . import reports
from .utils import dotdict


# (flag, type, default) of vae/main.py:15-31 -- same names and defaults; the test suite checks the table
# against the reference's list (tests/test_host_logic.py::test_cli_flags_match_reference)
REFERENCE_SWITCHES = ["-viz", "-no_label", "-allow_growth"]
REFERENCE_OPTIONS = [
    ("--global_latent_dims", int, 128), ("--local_latent_dims", int, 128), ("--learning_rate", float, 1e-4),
    ("--beta", float, 40), ("--dataset", str, "svhn"), ("--training_steps", int, 1000000), ("--batch_size", int, 64),
    ("--patch_size", int, 1), ("--augmentation", str, "scramble"), ("--model", str, "lgvae"), ("--y_size", int, 30),
    ("--tau", float, 0.4), ("--alpha", float, 40),
]


def build_parser():
    ap = argparse.ArgumentParser(description="SPLIT-VAE / SPLIT-GMVAE training on MI355X (flags of the reference's vae/main.py)")
    for sw in REFERENCE_SWITCHES:
        ap.add_argument(sw, action="store_true")
    for flag, ty, default in REFERENCE_OPTIONS:
        ap.add_argument(flag, type=ty, nargs="?", default=default)
    # additions (not in the reference)
    ap.add_argument("--synthetic", action="store_true", help="synthetic batches in the reference data domain")
    ap.add_argument("--dtype", type=str, default="f32", choices=["bf16", "f32"],
                    help="f32 (default) = the reference's precision (vae/model.py:12: fp32 end to end; exact-fp32 MFMA); bf16 = opt-in throughput "
                         "mode: bf16 MFMA operands, fp32 accumulation / ELBO / Adam / master weights (BASELINE.json configs[1])")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--log_every", type=int, default=10000)
    ap.add_argument("--gm_dropout", type=str, default="tf2.0", choices=["tf2.0", "tf2.1"],
                    help="lggmvae: whether encoder_x's Dropout layers fire in training (tf2.0 = pinned tensorflow 2.0.0: no; "
                         "tf2.1 = call-context propagation of `training`: yes); see split_vae_amd/gm.py")
    ap.add_argument("--data_dir", type=str, default="data", help="holds SVHN/*.mat and celeba/*.tfrec (vae/data.py:24,:103)")
    ap.add_argument("--mix_per_image", action="store_true",
                    help="--augmentation mix_scramble: draw a patch size per image (the intent of augmentation.py:60-64) instead of one "
                         "per pipeline (what the reference runs: np.random.choice when Dataset.map traces mix_scramble)")
    ap.add_argument("--resident_data", action="store_true",
                    help="hold the on-disk dataset in device memory (SVHN as uint8, CelebA as fp32) and fetch, scramble and stage each "
                         "batch in one kernel from a host-side index list; same batches, same permutations, same losses")
    reports.add_arguments(ap)                        # the evaluation reports: --iw_samples ... --latent_dims (reports.py)
    return ap


def check_augmentation(augmentation, model_name):
    """--augmentation (augmentation.py:15-30) against --model, before any data or device work.  high_low_pass makes a 9-channel
    batch (x | x - low | low): the split models then reconstruct a 6-channel x_hat with a 3-channel decoder mean and the reference
    fails inside its loss; only the global-only GMVae (channels 0-2, vae/model.py:289) trains with it."""
    from .augmentation import TYPES
    if augmentation not in TYPES:
        raise SystemExit("--augmentation %s: expected one of %s (augmentation.py:15-30)" % (augmentation, ", ".join(TYPES)))
    if augmentation == 'high_low_pass' and model_name in ('lgvae', 'lggmvae', 'lg_spair'):
        raise SystemExit("--augmentation high_low_pass gives 9-channel inputs (x | x - low | low); --model %s splits them into x and a "
                         "6-channel x_hat its 3-channel decoder cannot reconstruct (the reference fails there too). "
                         "Use --model gmvae, or another augmentation." % model_name)


def make_augmentors(config):
    """(train, test) augmentors (vae/main.py:54-61).  mix_scramble draws its one patch size per mapped pipeline, so the test
    pipeline gets an Augmentator of its own; every other type shares one, as before."""
    from .augmentation import ReferenceAugmentator
    kw = dict(type=config.augmentation, size=config.patch_size, seed=config.seed, per_image=bool(config.get("mix_per_image")))
    train = ReferenceAugmentator(pipeline=0, **kw)
    test = ReferenceAugmentator(pipeline=1, **kw) if config.augmentation == 'mix_scramble' else train
    return train, test


def make_probe_references(train_ds, config):
    """--knn_probe: the reference batches, from the training set as data.get_dataset returned it (before main wraps it), through an
    augmentor of the probe's own (the test pipeline's settings)."""
    from . import probe
    from .augmentation import ReferenceAugmentator
    n_train = train_ds.N if hasattr(train_ds, "N") else train_ds.x.shape[0]
    n = int(config.knn_refs)
    if n > n_train:
        print('Note: --knn_refs %d clipped to the training set\'s %d images' % (n, n_train))
        n = n_train
    if n < int(config.knn_probe):
        raise SystemExit("--knn_probe %d: the training set has only %d images" % (config.knn_probe, n))
    aug = ReferenceAugmentator(type=config.augmentation, size=config.patch_size, seed=config.seed,
                               per_image=bool(config.get("mix_per_image")), pipeline=1)
    return probe.reference_batches(train_ds, n, aug, config.batch_size)


def make_model(model_name, config, input_shape):
    """vae/main.py:63-73: the model and optimizer `--model` selects -> (model, optimizer)."""
    from .model import LGVae
    from .optimizer import Adam, ExponentialDecay
    if model_name == 'lgvae':
        model = LGVae(global_latent_dims=config.global_latent_dims, local_latent_dims=config.local_latent_dims,
                      image_shape=input_shape, dtype=config.dtype, seed=config.seed)
        optimizer = Adam(learning_rate=config.learning_rate)
    elif model_name == 'lggmvae':                                       # vae/main.py:66-69
        from .gm import LGGMVae
        lr_schedule = ExponentialDecay(config.learning_rate, decay_steps=1000000, decay_rate=0.4, staircase=True)
        optimizer = Adam(learning_rate=lr_schedule)
        model = LGGMVae(global_latent_dims=config.global_latent_dims, local_latent_dims=config.local_latent_dims,
                        image_shape=input_shape, y_size=config.y_size, tau=config.tau, dtype=config.dtype, seed=config.seed,
                        dropout_in_training=config.gm_dropout == "tf2.1")
    elif model_name == 'gmvae':                                         # vae/main.py:70-73
        from .gmvae import GMVae
        lr_schedule = ExponentialDecay(config.learning_rate, decay_steps=1000000, decay_rate=0.4, staircase=True)
        optimizer = Adam(learning_rate=lr_schedule)
        model = GMVae(global_latent_dims=config.global_latent_dims, image_shape=input_shape, y_size=config.y_size, tau=config.tau,
                      dtype=config.dtype, seed=config.seed, dropout_in_training=config.gm_dropout == "tf2.1")
    else:
        raise ValueError("--model %s: expected lgvae, lggmvae or gmvae (vae/main.py:27)" % model_name)
    return model, optimizer


def main(argv=None):
    args = build_parser().parse_args(argv)
    reports.check_all(args)                          # before any data or device work
    from . import configure_hw_queues
    configure_hw_queues()                            # before the first HIP call (split_vae_amd/__init__.py)
    config = dotdict(vars(args))
    config.label = not config.no_label
    print('Config:', config)
    check_augmentation(config.augmentation, args.model)
    from . import data, trainer

    augmentor, test_augmentor = make_augmentors(config)
    resident = bool(config.get("resident_data"))
    train_ds, test_ds, input_shape = data.get_dataset(config.dataset, config.batch_size, synthetic=config.synthetic,
                                                      data_dir=config.data_dir, get_label=config.label,
                                                      resident=resident)
    if config.label and not train_ds.labelled:
        # only the SVHN files carry labels (vae/data.py:54-62); the reference's labelled pipeline (vae/main.py:56-58)
        # cannot run on CelebA either, its README passes -no_label there
        print('Note: dataset %r serves no labels; continuing as with -no_label' % config.dataset)
        config.label = False
    if config.label:
        # vae/trainer.py:81-97 trains / loads the SVHN probe classifier here; its weights blob is missing upstream
        # (.MISSING_LARGE_BLOBS:1), so the labels ride along unused and the classifier metrics are not reported
        print('Note: classifier-based test metrics are not available (svhn_classifier_weights.h5 is not in the reference repo)')
    if config.knn_probe:
        config.knn_ref_batches = None
        if not config.label:
            from . import probe
            print(probe.SKIPPED)
            config.knn_probe = 0
        else:
            config.knn_ref_batches = make_probe_references(train_ds, config)
    if resident:
        # the test batches first, as below: the augmentor's Philox call indices, hence every permutation, match a run without the flag
        test_batches = [(test_augmentor.augment_from(test_ds, i), test_ds.one_hot(i)) if config.label else test_augmentor.augment_from(test_ds, i)
                        for i in test_ds.index_batches()]
    elif config.label:
        train_ds = ((augmentor.augment(x), y) for x, y in train_ds)     # vae/main.py:57-58
        test_batches = [(test_augmentor.augment(x), y) for x, y in test_ds]
    else:
        train_ds = (augmentor.augment(x) for x in train_ds)             # vae/main.py:60-61
        test_batches = [test_augmentor.augment(x) for x in test_ds]
    model, optimizer = make_model(args.model, config, input_shape)
    if resident:
        # the fetch writes the training plan's padded inputs itself (the plan of this batch size, looked up per batch: the trainer sets beta first)
        rds, B = train_ds, config.batch_size
        if config.label:
            train_ds = ((augmentor.augment_from(rds, i, plan=model.plan(B)), rds.one_hot(i)) for i in rds.index_batches())
        else:
            train_ds = (augmentor.augment_from(rds, i, plan=model.plan(B)) for i in rds.index_batches())
    model.summary()
    print('Training local-global autoencoder')
    return trainer.train_local_global_autoencoder(model, optimizer, config.dataset, train_ds, test_batches, config=config)


if __name__ == "__main__":
    main()
