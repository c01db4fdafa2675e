"""Host side of the label-free reconstruction quality report (split_vae_amd/recon_quality.py, csrc/recon_quality.hip): the float64
twin (tests/recon_quality_ref.py) on cases with known answers, the mutants of the twin against its own bound on the inputs the GPU
tests use, the size of that bound (the check that the kernel's arithmetic is adequate), the entry points' refusals, the flag and
the report line.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import recon_quality_ref as ref


def _const(v, B=2, H=13, W=17):
    """a constant IMAGE value v in [0,1] as the network-domain input 2 v - 1"""
    return np.full((B, H, W, 3), 2.0 * v - 1.0, np.float32)


# ---------------------------------------------------------------- known answers
def test_window_sums_to_one_and_is_symmetric():
    g = ref.window()
    assert len(g) == 11 and abs(g.sum() - 1.0) < 1e-15 and np.array_equal(g, g[::-1]) and g.argmax() == 5
    assert abs(np.outer(g, g).sum() - 1.0) < 1e-15
    assert abs(g[4] / g[5] - np.exp(-1.0 / 4.5)) < 1e-15


def test_constant_images_have_the_closed_form_ssim():
    a, b = 0.75, 0.25
    pi = ref.quality(_const(a), _const(b))
    assert np.allclose(pi[:, 1], (2 * a * b + ref.C1) / (a * a + b * b + ref.C1), rtol=0, atol=1e-12)
    assert np.allclose(pi[:, 0], (a - b) ** 2, rtol=1e-12)


def test_identical_images_give_ssim_one_and_100_db():
    xa, _ = ref.images("textured", 3, 16, 19, seed=3)
    pi = ref.quality(xa, xa)
    assert np.array_equal(pi[:, 0], np.zeros(3)) and np.allclose(pi[:, 1], 1.0, rtol=0, atol=1e-12)
    acc = ref.finish(pi)
    assert acc[0] == 300.0 and abs(acc[1] - 3.0) < 1e-11 and acc[2] == 3.0


def test_one_11_by_11_image_is_a_single_window():
    xa, xb = ref.images("textured", 1, 11, 11, seed=4)
    pa, pb = (xa.astype(np.float64) + 1) / 2, np.clip((xb.astype(np.float64) + 1) / 2, 0, 1)
    w = np.outer(ref.window(), ref.window())[None, :, :, None]
    ma, mb = (w * pa).sum((1, 2)), (w * pb).sum((1, 2))
    va, vb, cov = (w * pa * pa).sum((1, 2)) - ma * ma, (w * pb * pb).sum((1, 2)) - mb * mb, (w * pa * pb).sum((1, 2)) - ma * mb
    s = (2 * ma * mb + ref.C1) * (2 * cov + ref.C2) / ((ma * ma + mb * mb + ref.C1) * (va + vb + ref.C2))
    assert abs(ref.quality(xa, xb)[0, 1] - s.mean()) < 1e-13


def test_psnr_of_a_known_mse():
    assert np.allclose(ref.psnr([1e-2, 1e-3, 0.0, 1e-12, 1.0]), [20.0, 30.0, 100.0, 100.0, 0.0], rtol=0, atol=1e-12)
    acc = ref.finish(np.array([[1e-2, 0.5], [1e-4, 0.25]]), acc=[1.0, 2.0, 3.0])
    assert np.allclose(acc, [61.0, 2.75, 5.0], rtol=1e-14)


def test_agrees_with_an_installed_ssim_if_there_is_one():
    try:
        from skimage.metrics import structural_similarity
    except Exception:
        pytest.skip("no scikit-image on this machine (tf.image.ssim neither): nothing to compare with")
    xa, xb = ref.images("textured", 1, 32, 32, seed=5)
    pa, pb = (xa[0].astype(np.float64) + 1) / 2, np.clip((xb[0].astype(np.float64) + 1) / 2, 0, 1)
    _, full = structural_similarity(pa, pb, gaussian_weights=True, sigma=1.5, use_sample_covariance=False, data_range=1.0,
                                    channel_axis=-1, full=True)
    assert abs(full[5:-5, 5:-5].mean() - ref.quality(xa, xb)[0, 1]) < 1e-6        # skimage truncates its window at 3.5 sigma: 11 taps


# ---------------------------------------------------------------- the bound: the chosen arithmetic is adequate
def _gpu_inputs():
    for (B, H, W) in ref.SHAPES:
        for kind in ref.KINDS:
            yield kind, ref.images(kind, B, H, W)


def test_the_bound_is_inside_the_parity_figure_on_the_worst_case_and_on_every_gpu_input():
    one, near = np.full((2, 32, 32, 3), 1.0, np.float32), np.full((2, 32, 32, 3), 1.0 - 1e-3, np.float32)
    cases = [("worst", (one, near)), ("worst swapped", (near, one))] + list(_gpu_inputs())
    for name, (xa, xb) in cases:
        for clip in (True, False):
            pi = ref.quality(xa, xb, clip_b=clip)
            e_mse, e_ssim = ref.bound(xa, xb, clip_b=clip)
            assert np.all(e_ssim <= ref.PARITY), (name, clip, e_ssim.max())
            assert np.all(e_mse <= ref.PARITY * pi[:, 0] + 1e-30), (name, clip)       # copies: MSE = 0 and the bound is 0 too
            assert np.all(e_mse >= 0) and np.all(e_ssim > 0)


def test_the_twin_does_not_depend_on_the_buffer_layout():
    xa, xb = ref.images("textured", 2, 12, 37)
    want = ref.quality(xa, xb)
    for pa, oa, pb, ob in ref.LAYOUTS:
        got = ref.quality(ref.embed(xa, pa, oa), ref.embed(xb, pb, ob), oa, ob)
        assert np.array_equal(got, want), (pa, oa, pb, ob)


# ---------------------------------------------------------------- mutants
def _rejected(mutant):
    """True when the GPU tests' comparison tells the mutant from the twin on at least one of their inputs"""
    if mutant == "psnr_of_mean_mse":
        xa, xb = ref.images("textured", 5, 32, 32)
        xb[0] = xa[0] + np.float32(0.01) * (xb[0] - xa[0])              # images of very different MSE
        pi = ref.quality(xa, xb)
        return not np.allclose(ref.finish(pi, mutant=mutant), ref.finish(pi), rtol=1e-12, atol=0)
    for kind, (xa, xb) in _gpu_inputs():
        rng = np.random.default_rng(7)
        a6 = ref.embed(xa, 6, 0, 0.0)
        b6 = ref.embed(xb, 6, 0, 0.0)
        a6[..., 3:], b6[..., 3:] = rng.uniform(-1, 1, xa.shape), rng.uniform(-1, 1, xb.shape)    # channels_3_5 reads these
        want = ref.quality(a6, b6)
        if not ref.agrees(ref.quality(a6, b6, mutant=mutant), want, *ref.bound(a6, b6)):
            return True
    return False


@pytest.mark.parametrize("mutant", ref.MUTANTS)
def test_the_comparison_rejects_the_mutant(mutant):
    assert _rejected(mutant), mutant


def test_there_are_at_least_the_ten_mutants_and_the_twin_passes_its_own_comparison():
    assert len(set(ref.MUTANTS)) >= 10
    for kind, (xa, xb) in _gpu_inputs():
        assert ref.agrees(ref.quality(xa, xb), ref.quality(xa, xb), *ref.bound(xa, xb))
    with_nan = ref.embed(ref.images("flat", 1, 11, 11)[0], 6, 0)
    assert not ref.agrees(ref.quality(with_nan, with_nan, 3, 3), np.ones((1, 2)), np.ones(1), np.ones(1))     # a NaN never agrees


def test_the_no_clip_mutant_needs_values_outside_the_range():
    xa, xb = ref.images("flat", 2, 16, 16)
    assert (xb > 1).any()
    assert not np.array_equal(ref.quality(xa, xb), ref.quality(xa, xb, mutant="no_clip"))
    assert np.array_equal(ref.quality(xa, xa), ref.quality(xa, xa, mutant="no_clip"))


# ---------------------------------------------------------------- the draw's twin
def test_draw_twin_blocks():
    rng = np.random.default_rng(0)
    mg, ml, eps = (rng.standard_normal(s).astype(np.float32) for s in ((4, 5), (4, 3), (4, 8)))
    pm, ps = rng.standard_normal((6, 5)).astype(np.float32), rng.uniform(0.5, 2, (6, 5)).astype(np.float32)
    assert np.array_equal(ref.draw(mg, ml, ref.MEANS, eps), np.concatenate([mg, ml], 1))
    assert np.array_equal(ref.draw(mg, ml, ref.KEEP_G, eps), np.concatenate([mg, eps[:, 5:]], 1))
    assert np.array_equal(ref.draw(mg, ml, ref.KEEP_L, eps), np.concatenate([eps[:, :5], ml], 1))
    comp = np.array([0, 5, 9, -2])
    z = ref.draw(mg, ml, ref.KEEP_L, eps, comp, pm, ps)
    assert np.allclose(z[1, :5], pm[5] + ps[5] * eps[1, :5], rtol=1e-6) and np.array_equal(z[:, 5:], ml)       # comp is clamped to 0 .. n-1
    assert np.allclose(z[2, :5], pm[5] + ps[5] * eps[2, :5], rtol=1e-6) and np.allclose(z[3, :5], pm[0] + ps[0] * eps[3, :5], rtol=1e-6)
    assert ref.draw(mg, None, ref.KEEP_L, eps[:, :5]).shape == (4, 5)


def test_bf16_rounding_is_to_nearest_even():
    import torch
    x = np.concatenate([np.random.default_rng(1).standard_normal(4096).astype(np.float32) * 3,
                        np.array([1.00390625, 1.01171875, 0.0, -0.0, 1e-30, 65504.0], np.float32)])      # two exact ties
    assert np.array_equal(ref.bf16_round(x), torch.from_numpy(x).to(torch.bfloat16).float().numpy())


# ---------------------------------------------------------------- entry-point validation (host code of the built library)
def _buf():
    b = np.zeros(1 << 16, np.uint8)
    return b, (b.ctypes.data + 63) // 64 * 64


def _q_call(lib, **kw):
    from split_vae_amd import _lib
    a = dict(B=2, H=12, W=13, pa=6, oa=0, pb=6, ob=0, null=(), misalign=(), short=0)
    a.update(kw)
    keep = [_buf() for _ in range(4)]
    p = {n: None if n in a["null"] else C.c_void_p(k[1] + (2 if n in a["misalign"] else 0)) for n, k in zip(("a", "b", "per_image", "ws"), keep)}
    nbytes = C.c_int64(1 << 12)
    lib.sv_recon_quality_workspace_bytes(a["B"], a["H"], a["W"], C.byref(nbytes))
    rc = lib.sv_recon_quality(p["a"], a["pa"], a["oa"], p["b"], a["pb"], a["ob"], 1, a["B"], a["H"], a["W"], p["per_image"], p["ws"],
                              nbytes.value - a["short"], None)
    return _lib.STATUS.get(rc, rc)


def _d_call(lib, **kw):
    from split_vae_amd import _lib
    a = dict(B=4, Lg=16, Ll=8, ld=(16, 8, 24, 24), mode=1, dtype=0, n=0, null=("comp", "pm", "ps"), misalign=(), offset=0)
    a.update(kw)
    names = ("mg", "ml", "eps", "comp", "pm", "ps", "zcat")
    keep = [_buf() for _ in names]
    p = {n: None if n in a["null"] else C.c_void_p(k[1] + (1 if n in a["misalign"] else 0)) for n, k in zip(names, keep)}
    rc = lib.sv_recon_draw(p["mg"], a["ld"][0], p["ml"], a["ld"][1], a["mode"], p["eps"], a["ld"][2], p["comp"], p["pm"], p["ps"], a["n"],
                           p["zcat"], a["ld"][3], a["dtype"], a["B"], a["Lg"], a["Ll"], 1, a["offset"], None)
    return _lib.STATUS.get(rc, rc)


def test_entry_points_refuse_everything_outside_the_domain(lib_built):
    """Host addresses: every refusal is decided before anything is enqueued, so nothing is dereferenced."""
    from split_vae_amd import _lib
    lib = _lib.load()
    for bad in (dict(H=10), dict(W=10), dict(B=0), dict(B=-1), dict(pa=2), dict(pa=5, oa=3), dict(pb=5, ob=3), dict(oa=-1), dict(ob=-1),
                dict(pa=4097), dict(H=16385)):
        assert _q_call(lib, **bad) == "SV_E_UNSUPPORTED", bad
    for name in ("a", "b", "per_image", "ws"):
        assert _q_call(lib, null=(name,)) == "SV_E_BADARG", name
        assert _q_call(lib, misalign=(name,)) == "SV_E_BADARG", name
    assert _q_call(lib, short=1) == "SV_E_WORKSPACE"
    assert _q_call(lib, short=1, B=1, H=11, W=11, pa=3, pb=3) == "SV_E_WORKSPACE"                # the domain's corners are accepted
    assert _q_call(lib, short=1, B=7, H=64, W=200, pa=9, oa=6, pb=4096, ob=4093) == "SV_E_WORKSPACE"
    for bad in (dict(Lg=0), dict(Lg=513), dict(Ll=-1), dict(Ll=513), dict(B=0), dict(offset=-1), dict(mode=3), dict(mode=-1), dict(dtype=2),
                dict(ld=(15, 8, 24, 24)), dict(ld=(16, 7, 24, 24)), dict(ld=(16, 8, 23, 24)), dict(ld=(16, 8, 24, 23)),
                dict(null=("comp",), n=0), dict(null=("comp",), n=4097)):
        assert _d_call(lib, **bad) == "SV_E_UNSUPPORTED", bad
    for null in (("mg", "comp", "pm", "ps"), ("ml", "comp", "pm", "ps"), ("zcat", "comp", "pm", "ps"), ("comp", "pm"), ("comp", "ps")):
        assert _d_call(lib, null=null, n=5) == "SV_E_BADARG", null
    for name in ("mg", "ml", "eps", "zcat"):
        assert _d_call(lib, misalign=(name,)) == "SV_E_BADARG", name
    acc, per = _buf(), _buf()
    assert lib.sv_recon_finish(C.c_void_p(per[1]), 0, C.c_void_p(acc[1]), None) == _lib.STATUS_UNSUPPORTED
    assert lib.sv_recon_finish(None, 4, C.c_void_p(acc[1]), None) == _lib.STATUS_BADARG
    assert lib.sv_recon_finish(C.c_void_p(per[1]), 4, None, None) == _lib.STATUS_BADARG
    assert lib.sv_recon_finish(C.c_void_p(per[1] + 4), 4, C.c_void_p(acc[1]), None) == _lib.STATUS_BADARG
    assert lib.sv_recon_finish(C.c_void_p(per[1]), 4, C.c_void_p(acc[1] + 4), None) == _lib.STATUS_BADARG


def test_workspace_bytes_and_the_window(lib_built):
    from split_vae_amd import _lib, ops
    lib = _lib.load()

    def ws(B, H, W):
        n = C.c_int64(-7)
        return lib.sv_recon_quality_workspace_bytes(B, H, W, C.byref(n)), n.value
    assert lib.sv_recon_quality_workspace_bytes(2, 32, 32, None) == _lib.STATUS_BADARG
    for bad in ((0, 32, 32), (2, 10, 32), (2, 32, 10)):
        assert ws(*bad) == (_lib.STATUS_UNSUPPORTED, -7), bad
    for B, H, W in ref.SHAPES + ((512, 64, 64),):
        rc, n = ws(B, H, W)
        assert rc == 0 and n >= B * ref.tiles(H, W) * 16 and n % 256 == 0, (B, H, W)
    assert ref.tiles(32, 32) == 3 and ref.tiles(64, 64) == 7 and ref.tiles(11, 100) == 2
    assert np.allclose(ops.recon_window(), ref.window(), rtol=4e-16, atol=0)


def test_header_and_binding_agree_on_the_new_entry_points(lib_built):
    import os
    import re
    from split_vae_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "splitvae.h")).read(), flags=re.S)
    lib = _lib.load()
    names = sorted(n for n in _lib.SYMBOLS if n.startswith("sv_recon_"))
    assert names == ["sv_recon_draw", "sv_recon_finish", "sv_recon_quality", "sv_recon_quality_workspace_bytes", "sv_recon_window"]
    for name in names:
        m = re.search(r"\b(?:int|void)\s+%s\s*\((.*?)\)\s*;" % name, src, flags=re.S)
        assert m, name
        params = [p for p in m.group(1).split(",") if p.strip() and p.strip() != "void"]
        assert len(params) == len(_lib.SYMBOLS[name][1]), name
        for p, ct in zip(params, _lib.SYMBOLS[name][1]):
            want = None if "*" in p else (C.c_int32 if "int32_t" in p else C.c_uint64 if "uint64_t" in p else C.c_int64 if "int64_t" in p
                                          else None)
            assert want is None or ct is want, (name, p)
            assert want is not None or ct in (C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_double)), (name, p)
        assert hasattr(lib, name)
    assert (_lib.RECON_MEANS, _lib.RECON_KEEP_G, _lib.RECON_KEEP_L) == (ref.MEANS, ref.KEEP_G, ref.KEEP_L) == (0, 1, 2)
    assert re.search(r"SV_RECON_MEANS = 0, SV_RECON_KEEP_G = 1, SV_RECON_KEEP_L = 2", src)


# ---------------------------------------------------------------- the flag and the report line
def test_parser_has_the_flag_outside_the_reference_options():
    from split_vae_amd import main as svmain
    ap = svmain.build_parser()
    assert ap.parse_args([]).recon_quality == 0 and ap.parse_args(["--recon_quality", "500"]).recon_quality == 500
    assert "--recon_quality" not in [f for f, _, _ in svmain.REFERENCE_OPTIONS] and "--recon_quality" not in svmain.REFERENCE_SWITCHES


@pytest.mark.parametrize("entry", ["main", "evaluate"])
def test_a_negative_count_is_refused_before_any_device_work(monkeypatch, capsys, entry):
    import split_vae_amd
    import torch
    from split_vae_amd import _lib, data, evaluate, main as svmain

    def boom(*a, **k):
        raise AssertionError("device or data work before the refusal")
    monkeypatch.setattr(split_vae_amd, "configure_hw_queues", boom)
    monkeypatch.setattr(torch.cuda, "is_available", boom)
    monkeypatch.setattr(torch.cuda, "_lazy_init", boom)
    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setattr(data, "get_dataset", boom)
    with pytest.raises(SystemExit) as e:
        if entry == "main":
            svmain.main(["--recon_quality", "-3", "-no_label"])
        else:
            evaluate.main(["--recon_quality", "-3", "-no_label", "--weights", "nowhere.npz"])
    assert "--recon_quality" in str(e.value) and "-3" in str(e.value)
    assert "Config:" not in capsys.readouterr().out


def test_evaluate_accepts_the_flag_alone(monkeypatch):
    import split_vae_amd
    from split_vae_amd import evaluate

    class Reached(Exception):
        pass

    def reached(*a, **k):
        raise Reached()
    monkeypatch.setattr(split_vae_amd, "configure_hw_queues", reached)
    with pytest.raises(SystemExit) as e:
        evaluate.main(["--weights", "nowhere.npz"])
    assert "--recon_quality N" in str(e.value)
    for model in ("lgvae", "lggmvae", "gmvae"):
        with pytest.raises(Reached):
            evaluate.main(["--weights", "nowhere.npz", "--recon_quality", "50", "-no_label", "--model", model])


def test_report_line_for_the_three_models():
    from split_vae_amd import recon_quality
    res = dict(n_images=26032, psnr=21.23456, ssim=0.712345, psnr_g=17.5, ssim_g=0.51236, psnr_l=9.87654, ssim_l=0.1)
    assert recon_quality.report_line(res) == ("Test reconstruction quality (26032 images): PSNR 21.23 dB, SSIM 0.7123; z_g kept (z_l ~ prior): "
                                              "PSNR 17.50 dB, SSIM 0.5124; z_l kept (z_g ~ prior): PSNR 9.88 dB, SSIM 0.1000")
    assert recon_quality.report_line(dict(res, n_images=7)) == recon_quality.report_line(res).replace("26032", "7")     # lggmvae: the same parts
    one = dict(res, psnr_g=None, ssim_g=None, psnr_l=None, ssim_l=None)
    assert recon_quality.report_line(one) == "Test reconstruction quality (26032 images): PSNR 21.23 dB, SSIM 0.7123"
    assert recon_quality.CLIPPED.format(500, 27) == "Note: --recon_quality 500 clipped to the test set's 27 images"
    assert set(recon_quality.HISTORY_KEYS) == set(res)


def test_report_clips_with_one_note_and_keeps_a_history(monkeypatch, capsys):
    from split_vae_amd import recon_quality
    from split_vae_amd.utils import dotdict
    res = dict(n_images=27, psnr=20.0, ssim=0.5, psnr_g=None, ssim_g=None, psnr_l=None, ssim_l=None)
    seen = []
    monkeypatch.setattr(recon_quality, "evaluate", lambda model, batches, n: seen.append(n) or dict(res))
    config = dotdict(recon_quality=500)
    assert recon_quality.report(None, [], config, step=0) == res and recon_quality.report(None, [], config, step=10) == res
    out = capsys.readouterr().out
    assert out.count("Note: --recon_quality 500 clipped to the test set's 27 images") == 1
    assert out.count("Test reconstruction quality (27 images): PSNR 20.00 dB, SSIM 0.5000") == 2
    assert seen == [500, 500] and [h["step"] for h in config.recon_quality_history] == [0, 10]
    assert recon_quality.report(None, [], dotdict(recon_quality=0)) is None and len(seen) == 2
    with pytest.raises(SystemExit):
        recon_quality.check_flags(-1)
    recon_quality.check_flags(0), recon_quality.check_flags(1)
