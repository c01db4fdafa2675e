"""Measure a saved model without training: any of the evaluation reports of split_vae_amd/reports.py, in its order --
--iw_samples (the importance-weighted test log-likelihood of LGVae) or --gm_iw_samples (the mixture bound of LGGMVae / GMVae),
--knn_probe (the k-NN label probe of the latents), --latent_info (the aggregate-posterior information report), --recon_quality
(PSNR / SSIM of the decodes) and --latent_dims (the per-dimension latent report); the last three cover every model and need no labels.

    python -m split_vae_amd.evaluate --weights models/20260101-120000.h5 --dataset svhn --iw_samples 64 -no_label
    python -m split_vae_amd.evaluate --weights models/20260101-120000.h5 --dataset svhn --knn_probe 5
    python -m split_vae_amd.evaluate --weights models/20260101-120000.h5 --dataset celeba64 -no_label --latent_info 10000
    python -m split_vae_amd.evaluate --weights models/20260101-120000.h5 --dataset celeba64 -no_label --recon_quality 10000
    python -m split_vae_amd.evaluate --weights models/20260101-120000.h5 --dataset celeba64 -no_label --latent_dims 10000

Takes the flags of split_vae_amd.main (the model's latent widths, --dataset, --batch_size, --dtype, --data_dir, --synthetic,
--seed, --patch_size / --augmentation for the x_hat half of the test batches) plus --weights; builds the model, loads the .h5 /
.npz file, runs the reports over the test set and prints the lines the training loop prints with the same flags.  The probe loads
the labels and the training split (its first --knn_refs images are the references).
"""
from . import reports
from .main import build_parser as build_main_parser, check_augmentation, make_augmentors, make_model, make_probe_references
from .utils import dotdict

NOTHING = ("nothing to measure: pass --iw_samples K (importance samples per image, K >= 1) and / or --knn_probe K "
           "(neighbours of the latent label probe, 1 <= K <= 32) and / or --latent_info N (test images of the "
           "information report, N >= 2) and / or --recon_quality N (test images of the reconstruction quality report, N >= 1) "
           "and / or --latent_dims N (test images of the per-dimension latent report, N >= 2)")


def build_parser():
    ap = build_main_parser()
    ap.description = "Importance-weighted test log-likelihood, k-NN latent label probe, latent information and reconstruction quality reports of a saved weights file"
    ap.add_argument("--weights", type=str, required=True, help="file written by save_weights (.h5 / .hdf5 / .keras, else .npz)")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    reports.check_all(args, nothing_on=NOTHING)          # before any data or device work
    from . import configure_hw_queues
    configure_hw_queues()                                # before the first HIP call (split_vae_amd/__init__.py)
    config = dotdict(vars(args))
    config.label = bool(args.knn_probe)
    check_augmentation(config.augmentation, args.model)
    from . import data
    _, test_augmentor = make_augmentors(config)
    train_ds, test_ds, input_shape = data.get_dataset(config.dataset, config.batch_size, synthetic=config.synthetic,
                                                      data_dir=config.data_dir, get_label=config.label)
    if config.label and not train_ds.labelled:
        from . import probe
        print(probe.SKIPPED)
        config.label, config.knn_probe = False, 0
    if config.label:
        test_batches = [(test_augmentor.augment(x), y) for x, y in test_ds]      # the test batches of main(): the augmentor's first calls
    else:
        test_batches = [test_augmentor.augment(x) for x in test_ds]
    model, _ = make_model(args.model, config, input_shape)
    model.load_weights(args.weights)
    if config.knn_probe:
        config.knn_ref_batches = make_probe_references(train_ds, config)
    return reports.results_dict(reports.run_all(model, test_batches, config))


if __name__ == "__main__":
    main()
