"""The evaluation reports behind a test-set evaluation: one table for their flags, their pre-device checks, the training loops
(trainer.py) and the saved-model CLI (evaluate.py).  A report's arithmetic, its printed line and its constants live in its module
(iw.py, probe.py, latent_info.py, recon_quality.py, latent_dims.py); an entry here says how the module is driven.  A new report is
one module and one entry.

The modules are looked up when a report runs, not when this file is imported: importing it costs nothing, and a test that replaces
`module.evaluate` or `module.report` is honoured.
"""
import importlib


class Report:
    """One row of TABLE.  `name` is the flag (without the dashes), the config key and the key of run_all's result.
      arguments  ((flag, default, help), ...) for argparse: the flag itself first
      check      (module, args): the pre-device check of the parsed flags; raises SystemExit
      models     --model names the report covers (None: all).  A restricted report's check is a model check: check_all runs those first
      needs      (config) -> bool: what else the run needs (the probe: labels and reference batches)
      measure    (module, model, test_batches, config, n) -> res, n the flag's value
      line       (module, n, res) -> the printed line
      clipped    the report covers the first n test images: a shorter test set is noted once per run with module.CLIPPED
      history    config attribute that collects one dict(row(module, res), step=step) per run (None: no history)
      result     (module, res) -> the report's share of the dict evaluate.main returns
      report     the module's function run_all calls: (model, test_batches, config, step)"""

    def __init__(self, name, module, arguments, check, measure, line, result, models=None, needs=None, clipped=False, history=None,
                 row=None, report="report"):
        self.name, self.module, self.arguments, self.check, self.measure, self.line, self.result = name, module, arguments, check, measure, line, result
        self.models, self.needs, self.clipped, self.history, self.row, self.report = models, needs, clipped, history, row, report


def _first_n(name, help, check, result_keys):
    """A label-free report over the first N test images: module.evaluate(model, test_batches, N), module.report_line(res), the whole
    result kept in config.<name>_history."""
    return Report(name, name, (("--" + name, 0, help),), check,
                  measure=lambda m, model, batches, config, n: m.evaluate(model, batches, n),
                  line=lambda m, n, res: m.report_line(res), clipped=True, history=name + "_history", row=lambda m, res: res,
                  result=lambda m, res: {name + "_" + k: res[k] for k in result_keys(m, res)})


def _local_dims(args):
    return args.local_latent_dims if args.model != 'gmvae' else 0


def _knn_figures(m, res):
    return dict(knn_acc_g=res["acc_g"], knn_acc_l=res["acc_l"])


TABLE = (           # in print order
    Report("iw_samples", "iw",
           (("--iw_samples", 0,
             "K > 0: after the report of every evaluation, the K-sample importance-weighted bound of the test log-likelihood "
             "(joint and x-only, nats) and the bits per dimension of x (split_vae_amd/iw.py); --model lgvae only"),),
           check=lambda m, a: m.check_model_name(a.model, a.iw_samples), models=('lgvae',),
           measure=lambda m, model, batches, config, k: m.evaluate(model, batches, k),
           line=lambda m, k, res: m.report_line(k, res), result=lambda m, res: res),
    Report("gm_iw_samples", "iw",
           (("--gm_iw_samples", 0,
             "K > 0: after the report of every evaluation, the K-sample importance-weighted bound of the mixture models' "
             "test log-likelihood, y marginalised (split_vae_amd/iw.py: mixture_evaluate); --model lggmvae / gmvae only"),),
           check=lambda m, a: m.check_mixture_model_name(a.model, a.gm_iw_samples), models=('lggmvae', 'gmvae'),
           measure=lambda m, model, batches, config, k: m.mixture_evaluate(model, batches, k),
           line=lambda m, k, res: m.mixture_report_line(k, res), history="gm_iw_history",
           row=lambda m, res: {key: res[key] for key in m.MIXTURE_HISTORY_KEYS}, result=lambda m, res: res, report="mixture_report"),
    Report("knn_probe", "probe",
           (("--knn_probe", 0,
             "K > 0: after the report of every evaluation, the accuracy of a K-nearest-neighbour classifier of the test "
             "set's latent means over --knn_refs training images, for z_g and z_l separately (split_vae_amd/probe.py); "
             "needs labels; K <= 32"),
            ("--knn_refs", 20000, "--knn_probe: the number of reference images, the first N of the training set in file order")),
           check=lambda m, a: m.check_flags(a.knn_probe, a.knn_refs, a.no_label),
           needs=lambda config: config.label and config.get("knn_ref_batches"),
           measure=lambda m, model, batches, config, k: m.knn_probe(model, config.knn_ref_batches, batches, k),
           line=lambda m, k, res: m.report_line(res), history="knn_history", row=_knn_figures, result=_knn_figures),
    _first_n("latent_info",
             "N >= 2: after the report of every evaluation, the aggregate-posterior information report over the first N "
             "test images: per latent block the KL term split into index-code mutual information and marginal KL, and the "
             "mutual information of z_g and z_l (split_vae_amd/latent_info.py); needs no labels",
             check=lambda m, a: m.check_flags(a.latent_info, a.global_latent_dims, _local_dims(a)),
             result_keys=lambda m, res: m.HISTORY_KEYS),
    _first_n("recon_quality",
             "N >= 1: after the report of every evaluation, the mean PSNR and SSIM against the original image, over the first "
             "N test images, of the reconstruction and of the decodes with z_l, then z_g, drawn from its prior "
             "(split_vae_amd/recon_quality.py); needs no labels",
             check=lambda m, a: m.check_flags(a.recon_quality), result_keys=lambda m, res: m.HISTORY_KEYS),
    _first_n("latent_dims",
             "N >= 2: after the report of every evaluation, the per-dimension latent report over the first N test images: "
             "active units per block (Burda et al. 2016: variance of the posterior mean over the images above 0.01), the "
             "largest per-dimension KL, the total correlation and the dimension-wise KL of Chen et al. 2018's "
             "decomposition (split_vae_amd/latent_dims.py); needs no labels",
             check=lambda m, a: m.check_flags(a.latent_dims, a.global_latent_dims, _local_dims(a)),
             result_keys=lambda m, res: res),
)
BY_NAME = {e.name: e for e in TABLE}


def _module(entry):
    return importlib.import_module("." + entry.module, __package__)


def model_name(model):
    """The --model name of a model object (the training loops pick their step functions by the same classes)."""
    from .gm import LGGMVae
    from .gmvae import GMVae
    return 'lggmvae' if isinstance(model, LGGMVae) else 'gmvae' if isinstance(model, GMVae) else 'lgvae'


def add_arguments(parser):
    for entry in TABLE:
        for flag, default, help in entry.arguments:
            parser.add_argument(flag, type=int, default=default, help=help)


def any_on(args):
    return any(getattr(args, entry.name) != 0 for entry in TABLE)


def check_all(args, nothing_on=None):
    """Every report's check of the parsed flags, before any data or device work: the model checks, then -- with `nothing_on`, a
    message -- SystemExit(nothing_on) when no report is switched on, then the other checks; each group in table order."""
    for entry in TABLE:
        if entry.models:
            entry.check(_module(entry), args)
    if nothing_on is not None and not any_on(args):
        raise SystemExit(nothing_on)
    for entry in TABLE:
        if not entry.models:
            entry.check(_module(entry), args)


def _on(entry, model, config):
    if int(config.get(entry.name) or 0) <= 0:
        return False
    if entry.models and model_name(model) not in entry.models:
        return False
    return entry.needs is None or bool(entry.needs(config))


def run(name, model, test_batches, config, step=None):
    """Report `name` behind an evaluation's report: measures, prints the line (and once per run the clipped note), appends to the
    entry's history and returns the figures; None when the report is off or does not cover this run."""
    entry = BY_NAME[name]
    if not _on(entry, model, config):
        return None
    m, n = _module(entry), int(config.get(name))
    res = entry.measure(m, model, test_batches, config, n)
    if entry.clipped and res["n_images"] < n and not config.get(name + "_clipped"):
        print(m.CLIPPED.format(n, res["n_images"]))
        setattr(config, name + "_clipped", True)
    print(entry.line(m, n, res))
    if entry.history:
        if config.get(entry.history) is None:
            setattr(config, entry.history, [])
        config.get(entry.history).append(dict(entry.row(m, res), step=step))
    return res


def run_all(model, test_batches, config, step=None):
    """Every report that is on, in table order, through its module's report function -> {name: figures}."""
    out = {}
    for entry in TABLE:
        if _on(entry, model, config):
            out[entry.name] = getattr(_module(entry), entry.report)(model, test_batches, config, step)
    return out


def results_dict(results):
    """run_all's results as the flat dict evaluate.main returns."""
    out = {}
    for entry in TABLE:
        if results.get(entry.name) is not None:
            out.update(entry.result(_module(entry), results[entry.name]))
    return out
