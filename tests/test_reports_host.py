"""The table of evaluation reports (split_vae_amd/reports.py): flags and help text, check order, the loops' run_all, the shared
runner and the dict evaluate.main returns.  CPU only: models, data and every module's arithmetic are stubs."""
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ORDER = ["iw_samples", "gm_iw_samples", "knn_probe", "latent_info", "recon_quality", "latent_dims"]
FIRST_N = ORDER[3:]
# module attribute behind each entry: (module, its report function, the function that measures)
HOOKS = {"iw_samples": ("iw", "report", "evaluate"), "gm_iw_samples": ("iw", "mixture_report", "mixture_evaluate"),
         "knn_probe": ("probe", "report", "knn_probe"), "latent_info": ("latent_info", "report", "evaluate"),
         "recon_quality": ("recon_quality", "report", "evaluate"), "latent_dims": ("latent_dims", "report", "evaluate")}
IW = dict(iw_joint=-2000.5, iw_x=-1900.25, elbo=-2100.0, n_images=27, bits_per_dim_x=0.8924)
GM_IW = dict(gm_iw_joint=-2000.5, gm_iw_x=-1900.25, gm_elbo=-2100.0, n_images=27, gm_bits_per_dim_x=0.8924)
KNN = dict(acc_g=0.75, acc_l=0.125, n_ref=39, n_test=27, k=3, hits_g=20, hits_l=3)
LATENT_INFO = dict(n_images=27, log_n=3.2958, kl_g=5.0, mi_g=3.0, mkl_g=2.0, kl_l=4.0, mi_l=2.5, mkl_l=1.5, overlap=0.25)
RECON = dict(n_images=27, psnr=20.5, ssim=0.75, psnr_g=15.25, ssim_g=0.5, psnr_l=12.0, ssim_l=0.25)
_G = dict(dims_g=2, active_g=1, var_g=[0.5, 0.001], kl_g=[1.5, 0.0], mi_g=[1.0, 0.0], dwkl_g=[0.5, 0.0], tc_g=0.75, dwkl_sum_g=0.5,
          block_kl_g=2.25, block_mi_g=1.0)
LATENT_DIMS = dict(n_images=27, log_n=3.2958, **_G, **{k[:-2] + "_l": v for k, v in _G.items()})
CANNED = {"iw_samples": IW, "gm_iw_samples": GM_IW, "knn_probe": KNN, "latent_info": LATENT_INFO, "recon_quality": RECON,
          "latent_dims": LATENT_DIMS}


def _module(name):
    import importlib
    return importlib.import_module("split_vae_amd." + HOOKS[name][0])


def _stub(kind):
    """An instance of the model class without its constructor: run_all reads nothing but the class."""
    from split_vae_amd.gm import LGGMVae
    from split_vae_amd.gmvae import GMVae
    from split_vae_amd.model import LGVae
    return object.__new__({"lgvae": LGVae, "lggmvae": LGGMVae, "gmvae": GMVae}[kind])


def _all_on(**over):
    from split_vae_amd.utils import dotdict
    return dotdict(dict(iw_samples=2, gm_iw_samples=2, knn_probe=3, latent_info=500, recon_quality=500, latent_dims=500, label=True,
                        knn_ref_batches=[("refs", "labels")]), **over)


def _can_measures(monkeypatch, seen):
    """every module's measuring function -> a recorder that returns the canned figures"""
    for name in ORDER:
        def measure(*a, _name=name, **k):
            seen.append((_name,) + tuple(a[1:]))
            return dict(CANNED[_name])
        monkeypatch.setattr(_module(name), HOOKS[name][2], measure)


# ---------------------------------------------------------------- flags and help text
def test_table_order_and_flags():
    from split_vae_amd import main as svmain, reports
    assert [e.name for e in reports.TABLE] == ORDER
    flags = [f for e in reports.TABLE for f, _, _ in e.arguments]
    assert flags == ["--iw_samples", "--gm_iw_samples", "--knn_probe", "--knn_refs", "--latent_info", "--recon_quality", "--latent_dims"]
    args = svmain.build_parser().parse_args([])
    assert all(getattr(args, n) == 0 for n in ORDER) and args.knn_refs == 20000 and not reports.any_on(args)


@pytest.mark.parametrize("entry,fixture", [("main", "cli_help.txt"), ("evaluate", "cli_help_evaluate.txt")])
def test_help_text_is_the_parents(monkeypatch, entry, fixture):
    """tests/golden/cli_help*.txt: format_help() of the two parsers before the table existed (COLUMNS=120, prog set as here)"""
    from split_vae_amd import evaluate, main as svmain
    monkeypatch.setenv("COLUMNS", "120")
    ap = (svmain if entry == "main" else evaluate).build_parser()
    ap.prog = "split_vae_amd." + entry
    with open(os.path.join(GOLDEN, fixture)) as f:
        assert ap.format_help() == f.read()


# ---------------------------------------------------------------- check_all: today's first message
BAD_PAIRS = [
    (["--iw_samples", "-1", "--gm_iw_samples", "-1"], "--iw_samples must be >= 0"),
    (["--gm_iw_samples", "-1", "--knn_probe", "99"], "--gm_iw_samples must be >= 0"),
    (["--knn_probe", "99", "--latent_info", "1"], "--knn_probe K: 0 (off) or 1 <= K <= 32 neighbours, got 99"),
    (["--latent_info", "1", "--recon_quality", "-3"], "--latent_info N: 0 (off) or N >= 2 test images, got 1"),
    (["--recon_quality", "-3", "--latent_dims", "1"], "--recon_quality N: 0 (off) or N >= 1 test images, got -3"),
]


@pytest.mark.parametrize("entry", ["check_all", "main", "evaluate"])
@pytest.mark.parametrize("flags,message", BAD_PAIRS)
def test_two_bad_flags_raise_the_first_ones_message(monkeypatch, entry, flags, message):
    import split_vae_amd
    from split_vae_amd import data, evaluate, main as svmain, reports

    def boom(*a, **k):
        raise AssertionError("device or data work before the refusal")
    monkeypatch.setattr(split_vae_amd, "configure_hw_queues", boom)
    monkeypatch.setattr(data, "get_dataset", boom)
    with pytest.raises(SystemExit) as e:
        if entry == "check_all":
            reports.check_all(svmain.build_parser().parse_args(flags))
        elif entry == "main":
            svmain.main(flags)
        else:
            evaluate.main(flags + ["--weights", "nowhere.npz"])
    assert str(e.value) == message


def test_model_restrictions_come_before_nothing_to_measure_and_that_before_the_rest():
    from split_vae_amd import evaluate, main as svmain, reports
    parse = svmain.build_parser().parse_args
    with pytest.raises(SystemExit) as e:
        reports.check_all(parse(["--model", "gmvae", "--iw_samples", "2", "--knn_probe", "99"]), nothing_on=evaluate.NOTHING)
    assert str(e.value).startswith("--model gmvae: --iw_samples covers --model lgvae only")
    with pytest.raises(SystemExit) as e:
        reports.check_all(parse(["--knn_refs", "0"]), nothing_on=evaluate.NOTHING)
    assert str(e.value) == evaluate.NOTHING and all("--" + n in evaluate.NOTHING for n in ORDER if n != "gm_iw_samples")
    reports.check_all(parse(["--knn_refs", "0"]))                                  # the training CLI: nothing on is fine
    with pytest.raises(SystemExit) as e:
        reports.check_all(parse(["--knn_probe", "-1"]), nothing_on=evaluate.NOTHING)   # a bad value counts as on: its own message
    assert str(e.value).startswith("--knn_probe K: 0 (off)")
    with pytest.raises(SystemExit) as e:                                            # the local block is not checked for gmvae
        reports.check_all(parse(["--latent_dims", "100", "--local_latent_dims", "513"]))
    assert str(e.value) == "--latent_dims covers latent blocks of at most 512 dimensions"
    reports.check_all(parse(["--latent_dims", "100", "--latent_info", "100", "--local_latent_dims", "513", "--model", "gmvae"]))


# ---------------------------------------------------------------- run_all
def _record_reports(monkeypatch, called):
    def boom(*a, **k):
        raise AssertionError("a module measured although its report function was replaced")
    for name in ORDER:
        monkeypatch.setattr(_module(name), HOOKS[name][2], boom)
        monkeypatch.setattr(_module(name), HOOKS[name][1], lambda m, t, config, step=None, _name=name: called.append((_name, step)) or _name)


@pytest.mark.parametrize("kind,iw", [("lgvae", "iw_samples"), ("lggmvae", "gm_iw_samples"), ("gmvae", "gm_iw_samples")])
def test_run_all_calls_the_modules_report_functions_in_table_order(monkeypatch, kind, iw):
    from split_vae_amd import reports
    from split_vae_amd.utils import dotdict
    called = []
    _record_reports(monkeypatch, called)
    model, label_free = _stub(kind), [iw] + FIRST_N
    out = reports.run_all(model, ["batch"], _all_on(), 7)
    assert [c[0] for c in called] == [iw, "knn_probe"] + FIRST_N and all(c[1] == 7 for c in called)
    assert list(out) == [c[0] for c in called] and out["latent_dims"] == "latent_dims"
    for config in (_all_on(label=False), _all_on(knn_ref_batches=None), _all_on(knn_ref_batches=[]), _all_on(knn_probe=0)):
        del called[:]
        reports.run_all(model, ["batch"], config, 0)
        assert [c[0] for c in called] == label_free                               # the probe needs labels and reference batches
    del called[:]
    assert reports.run_all(model, ["batch"], dotdict(label=True, knn_ref_batches=[("refs", "labels")]), 0) == {}
    assert reports.run_all(model, ["batch"], dotdict({n: 0 for n in ORDER}, label=True), 0) == {} and not called
    reports.run_all(model, ["batch"], dotdict(latent_info=16, recon_quality=None), None)
    assert called == [("latent_info", None)]


@pytest.mark.parametrize("kind", ["lgvae", "gmvae"])
def test_run_all_prints_in_table_order_and_keeps_each_reports_history(monkeypatch, capsys, kind):
    from split_vae_amd import iw, reports
    seen, config, model = [], _all_on(), _stub(kind)
    _can_measures(monkeypatch, seen)
    for step in (0, 5):
        reports.run_all(model, ["batch"], config, step)
    out = capsys.readouterr().out.splitlines()
    first = "Test IW-2 bound: " if kind == "lgvae" else "Test IW-2 mixture bound: "
    starts = [first, "Note: --latent_info 500 clipped", "Note: --recon_quality 500 clipped", "Note: --latent_dims 500 clipped"]
    per_run = [first, "Test k-NN probe (k=3, 39 refs): z_g acc 0.7500, z_l acc 0.1250", "Test latent information (27 images",
               "Test reconstruction quality (27 images): PSNR 20.50 dB", "Test latent dimensions (27 images"]
    want = [per_run[0], per_run[1], starts[1], per_run[2], starts[2], per_run[3], starts[3], per_run[4]] + per_run
    assert len(out) == len(want) and all(l.startswith(w) for l, w in zip(out, want)), out
    # what each measuring function was handed: (test batches, n), the probe its reference batches first
    assert seen[:5] == [("iw_samples" if kind == "lgvae" else "gm_iw_samples", ["batch"], 2), ("knn_probe", [("refs", "labels")], ["batch"], 3),
                        ("latent_info", ["batch"], 500), ("recon_quality", ["batch"], 500), ("latent_dims", ["batch"], 500)]
    assert config.get("iw_samples_history") is None and config.get("iw_history") is None      # --iw_samples keeps none
    if kind == "lgvae":
        assert config.get("gm_iw_history") is None
    else:
        assert config.gm_iw_history == [dict(step=s, **{k: GM_IW[k] for k in iw.MIXTURE_HISTORY_KEYS}) for s in (0, 5)]
    assert config.knn_history == [dict(step=s, knn_acc_g=0.75, knn_acc_l=0.125) for s in (0, 5)]
    assert config.latent_info_history == [dict(LATENT_INFO, step=s) for s in (0, 5)]
    assert config.recon_quality_history == [dict(RECON, step=s) for s in (0, 5)]
    assert config.latent_dims_history == [dict(LATENT_DIMS, step=s) for s in (0, 5)]


# ---------------------------------------------------------------- the shared runner of the first-N reports
@pytest.mark.parametrize("name", FIRST_N)
def test_first_n_runner_notes_the_clip_once_and_appends_one_history_dict_per_call(monkeypatch, capsys, name):
    from split_vae_amd import reports
    from split_vae_amd.utils import dotdict
    module, seen = _module(name), []
    monkeypatch.setattr(module, "evaluate", lambda model, batches, n: seen.append(n) or dict(CANNED[name]))
    assert module.report(None, [], dotdict({name: 0})) is None and reports.run(name, None, [], dotdict()) is None and not seen
    config = dotdict({name: 500})
    assert module.report(None, [], config, step=10) == CANNED[name]
    assert reports.run(name, None, [], config, 20) == CANNED[name]
    out = capsys.readouterr().out
    assert out.count(module.CLIPPED.format(500, 27)) == 1 and out.count("clipped") == 1
    assert out.count(module.report_line(CANNED[name])) == 2 and len(out.splitlines()) == 3
    assert config[name + "_history"] == [dict(CANNED[name], step=10), dict(CANNED[name], step=20)] and seen == [500, 500]
    exact = dotdict({name: 27})
    module.report(None, [], exact)
    assert "clipped" not in capsys.readouterr().out and exact[name + "_history"] == [dict(CANNED[name], step=None)]


# ---------------------------------------------------------------- evaluate.main's dict
def _evaluate(monkeypatch, argv):
    import split_vae_amd
    from split_vae_amd import data, evaluate

    class Augmentor:
        def augment(self, x):
            return x

    class Train:
        labelled = True
    model = _stub(argv[argv.index("--model") + 1] if "--model" in argv else "lgvae")
    model.load_weights = lambda path: None
    monkeypatch.setattr(split_vae_amd, "configure_hw_queues", lambda: None)
    monkeypatch.setattr(data, "get_dataset", lambda *a, get_label=False, **k: (Train(), [("x", "y")] if get_label else ["x"], [-1, 32, 32, 3]))
    monkeypatch.setattr(evaluate, "make_augmentors", lambda config: (None, Augmentor()))
    monkeypatch.setattr(evaluate, "make_model", lambda name, config, shape: (model, None))
    monkeypatch.setattr(evaluate, "make_probe_references", lambda train_ds, config: [("refs", "labels")])
    return evaluate.main(argv + ["--synthetic", "--weights", "nowhere.npz"])


def test_evaluate_returns_todays_keys_for_each_report(monkeypatch, capsys):
    from split_vae_amd import latent_info, recon_quality
    seen = []
    _can_measures(monkeypatch, seen)
    want = {"iw_samples": set(IW), "gm_iw_samples": set(GM_IW), "knn_probe": {"knn_acc_g", "knn_acc_l"},
            "latent_info": {"latent_info_" + k for k in latent_info.HISTORY_KEYS},
            "recon_quality": {"recon_quality_" + k for k in recon_quality.HISTORY_KEYS},
            "latent_dims": {"latent_dims_" + k for k in LATENT_DIMS}}
    assert len(want["latent_info"]) == 9 and len(want["recon_quality"]) == 7 and len(want["latent_dims"]) == 22
    for name in ORDER:
        argv = ["--" + name, "3"] + ([] if name == "knn_probe" else ["-no_label"]) + (["--model", "gmvae"] if name == "gm_iw_samples" else [])
        res = _evaluate(monkeypatch, argv)
        assert set(res) == want[name], name
        batches = seen[-1][-2]
        assert batches == ([("x", "y")] if name == "knn_probe" else ["x"]) and isinstance(batches, list)
    res = _evaluate(monkeypatch, ["--iw_samples", "2", "--knn_probe", "3", "--latent_info", "27", "--recon_quality", "27", "--latent_dims", "27"])
    assert set(res) == set().union(*(want[n] for n in ORDER if n != "gm_iw_samples"))
    assert res["iw_x"] == IW["iw_x"] and res["knn_acc_l"] == 0.125 and res["latent_info_overlap"] == 0.25 and res["recon_quality_ssim_l"] == 0.25
    assert res["latent_dims_var_g"] == [0.5, 0.001] and res["latent_dims_n_images"] == 27
    lines = [l.split(" (")[0].split(":")[0] for l in capsys.readouterr().out.splitlines()[-5:]]
    assert lines == ["Test IW-2 bound", "Test k-NN probe", "Test latent information", "Test reconstruction quality", "Test latent dimensions"]
