"""Measure a saved SPLIT-VAE (LGVae) without training: the importance-weighted test log-likelihood of split_vae_amd/iw.py.

    python -m split_vae_amd.evaluate --weights models/20260101-120000.h5 --dataset svhn --iw_samples 64 -no_label

Takes the flags of split_vae_amd.main (the model's latent widths, --dataset, --batch_size, --dtype, --data_dir, --synthetic,
--seed, --patch_size / --augmentation for the x_hat half of the test batches) plus --weights; builds the model, loads the .h5 /
.npz file, runs iw.evaluate over the test set and prints the line the training loop prints with --iw_samples.
"""
from .main import build_parser, check_augmentation, make_augmentors, make_model
from .utils import dotdict


def main(argv=None):
    ap = build_parser()
    ap.description = "Importance-weighted test log-likelihood of a saved SPLIT-VAE (LGVae) weights file"
    ap.add_argument("--weights", type=str, required=True, help="file written by save_weights (.h5 / .hdf5 / .keras, else .npz)")
    args = ap.parse_args(argv)
    from . import iw
    if args.iw_samples <= 0:
        raise SystemExit("--iw_samples K: the number of importance samples per image (K >= 1)")
    iw.check_model_name(args.model, args.iw_samples)     # before any data or device work
    from . import configure_hw_queues
    configure_hw_queues()                                # before the first HIP call (split_vae_amd/__init__.py)
    config = dotdict(vars(args))
    config.label = False
    check_augmentation(config.augmentation, args.model)
    from . import data
    _, test_augmentor = make_augmentors(config)
    _, test_ds, input_shape = data.get_dataset(config.dataset, config.batch_size, synthetic=config.synthetic, data_dir=config.data_dir,
                                               get_label=False)
    test_batches = (test_augmentor.augment(x) for x in test_ds)      # the test batches of main(): the augmentor's first calls
    model, _ = make_model(args.model, config, input_shape)
    model.load_weights(args.weights)
    res = iw.evaluate(model, test_batches, config.iw_samples)
    print(iw.report_line(config.iw_samples, res))
    return res


if __name__ == "__main__":
    main()
