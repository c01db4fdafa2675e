"""Measure a saved model without training: the importance-weighted test log-likelihood of split_vae_amd/iw.py (--iw_samples:
LGVae; --gm_iw_samples: the mixture bound of LGGMVae / GMVae), the k-NN label probe of the latents of split_vae_amd/probe.py and /
or the aggregate-posterior information report of split_vae_amd/latent_info.py (--latent_info; every model, no labels needed) and /
or the reconstruction quality report of split_vae_amd/recon_quality.py (--recon_quality; every model, no labels needed) and / or
the per-dimension latent report of split_vae_amd/latent_dims.py (--latent_dims; every model, no labels needed).

    python -m split_vae_amd.evaluate --weights models/20260101-120000.h5 --dataset svhn --iw_samples 64 -no_label
    python -m split_vae_amd.evaluate --weights models/20260101-120000.h5 --dataset svhn --knn_probe 5
    python -m split_vae_amd.evaluate --weights models/20260101-120000.h5 --dataset celeba64 -no_label --latent_info 10000
    python -m split_vae_amd.evaluate --weights models/20260101-120000.h5 --dataset celeba64 -no_label --recon_quality 10000
    python -m split_vae_amd.evaluate --weights models/20260101-120000.h5 --dataset celeba64 -no_label --latent_dims 10000

Takes the flags of split_vae_amd.main (the model's latent widths, --dataset, --batch_size, --dtype, --data_dir, --synthetic,
--seed, --patch_size / --augmentation for the x_hat half of the test batches) plus --weights; builds the model, loads the .h5 /
.npz file, runs iw.evaluate and / or probe.knn_probe over the test set and prints the lines the training loop prints with
--iw_samples / --knn_probe.  The probe loads the labels and the training split (its first --knn_refs images are the references).
"""
from .main import build_parser, check_augmentation, make_augmentors, make_model, make_probe_references
from .utils import dotdict


def main(argv=None):
    ap = build_parser()
    ap.description = "Importance-weighted test log-likelihood, k-NN latent label probe, latent information and reconstruction quality reports of a saved weights file"
    ap.add_argument("--weights", type=str, required=True, help="file written by save_weights (.h5 / .hdf5 / .keras, else .npz)")
    args = ap.parse_args(argv)
    from . import iw, latent_dims, latent_info, probe, recon_quality
    iw.check_model_name(args.model, args.iw_samples)     # before any data or device work
    iw.check_mixture_model_name(args.model, args.gm_iw_samples)
    if args.iw_samples <= 0 and args.gm_iw_samples <= 0 and args.knn_probe == 0 and args.latent_info == 0 and \
            args.recon_quality == 0 and args.latent_dims == 0:
        raise SystemExit("nothing to measure: pass --iw_samples K (importance samples per image, K >= 1) and / or --knn_probe K "
                         "(neighbours of the latent label probe, 1 <= K <= 32) and / or --latent_info N (test images of the "
                         "information report, N >= 2) and / or --recon_quality N (test images of the reconstruction quality report, N >= 1) "
                         "and / or --latent_dims N (test images of the per-dimension latent report, N >= 2)")
    probe.check_flags(args.knn_probe, args.knn_refs, args.no_label)
    latent_info.check_flags(args.latent_info, args.global_latent_dims, args.local_latent_dims if args.model != 'gmvae' else 0)
    recon_quality.check_flags(args.recon_quality)
    latent_dims.check_flags(args.latent_dims, args.global_latent_dims, args.local_latent_dims if args.model != 'gmvae' else 0)
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
        print(probe.SKIPPED)
        config.label, config.knn_probe = False, 0
    if config.label:
        test_batches = [(test_augmentor.augment(x), y) for x, y in test_ds]      # the test batches of main(): the augmentor's first calls
    else:
        keep = config.latent_info or config.recon_quality or config.latent_dims       # reports that walk the test batches after another one has
        test_batches = [test_augmentor.augment(x) for x in test_ds] if keep else (test_augmentor.augment(x) for x in test_ds)
    model, _ = make_model(args.model, config, input_shape)
    model.load_weights(args.weights)
    res = {}
    if config.iw_samples > 0:
        res = iw.evaluate(model, test_batches, config.iw_samples)
        print(iw.report_line(config.iw_samples, res))
    if config.gm_iw_samples > 0:
        res = iw.mixture_evaluate(model, test_batches, config.gm_iw_samples)
        print(iw.mixture_report_line(config.gm_iw_samples, res))
    if config.knn_probe:
        refs = make_probe_references(train_ds, config)
        pr = probe.knn_probe(model, refs, test_batches, config.knn_probe)
        print(probe.report_line(pr))
        res = dict(res, knn_acc_g=pr["acc_g"], knn_acc_l=pr["acc_l"])
    li = latent_info.report(model, test_batches, config)
    if li is not None:
        res = dict(res, **{"latent_info_" + k: li[k] for k in latent_info.HISTORY_KEYS})
    rq = recon_quality.report(model, test_batches, config)
    if rq is not None:
        res = dict(res, **{"recon_quality_" + k: rq[k] for k in recon_quality.HISTORY_KEYS})
    ld = latent_dims.report(model, test_batches, config)
    if ld is not None:
        res = dict(res, **{"latent_dims_" + k: v for k, v in ld.items()})
    return res


if __name__ == "__main__":
    main()
