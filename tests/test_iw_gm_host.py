"""Host side of the mixture models' importance-weighted bound: the float64 twin of tests/iw_gm_ref.py in its degenerate cases, the
derived bound against mutants of the twin on the inputs the GPU cases use, and the CLI surface of --gm_iw_samples.  No GPU."""
import numpy as np
import pytest

import iw_gm_ref as gr
import iw_ref


def _z32(d, comp=None):
    return gr.draw(d["zm_all"], d["zs_all"], d["comp"] if comp is None else comp, d["mu_l"], d["sig_l"], d["eps"], dtype=np.float32)


def _args(d):
    return d["logits"], d["zm_all"], d["zs_all"], d["pm"], d["ps"], d["mu_l"], d["sig_l"]


CASES = gr.case_inputs()


# ---------------------------------------------------------------- degenerate cases
def test_one_standard_normal_component_is_the_latent_ratio_of_lgvae():
    """n = 1, pm = 0, ps = 1: r = log N(z; 0, 1) - log q(z) over all Lg + Ll dimensions, iw_ref.latent_ratio at the same z."""
    d = gr.gaussian_case(4, 1, 24, 9, seed=50)
    d["pm"][:], d["ps"][:] = 0.0, 1.0
    z = gr.draw(d["zm_all"], d["zs_all"], d["comp"], d["mu_l"], d["sig_l"], d["eps"])
    mu = np.concatenate([d["zm_all"][:, 0], d["mu_l"]], axis=1)
    sig = np.concatenate([d["zs_all"][:, 0], d["sig_l"]], axis=1)
    np.testing.assert_allclose(gr.ratio(z, *_args(d)), iw_ref.latent_ratio(mu, sig, z_stored=z), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(gr.ratio(z, *_args(d)), iw_ref.latent_ratio(mu, sig, eps=d["eps"]), rtol=1e-9, atol=1e-9)


def test_posterior_equal_to_prior_with_uniform_pi_gives_zero_exactly():
    d = gr.gaussian_case(3, 30, 16, 0, seed=51)
    d["zm_all"][:], d["zs_all"][:], d["logits"][:] = d["pm"][None], d["ps"][None], 0.75
    z = _z32(d)
    assert np.array_equal(gr.ratio(z, *_args(d)), np.zeros(3))
    assert np.array_equal(gr.ratio(z, *_args(d), dtype=np.float32), np.zeros(3, np.float32))


def test_ratio_is_the_ratio_of_the_two_mixture_densities():
    """Against the densities written out with their 2 pi constants and no log-sum-exp trick (moderate values)."""
    d = gr.gaussian_case(3, 5, 4, 3, seed=52)
    z = gr.draw(d["zm_all"], d["zs_all"], d["comp"], d["mu_l"], d["sig_l"], d["eps"])
    N = lambda v, m, s: np.exp(-0.5 * ((v - m) / s) ** 2) / (s * np.sqrt(2 * np.pi))      # noqa: E731
    pi = np.exp(d["logits"].astype(np.float64))
    pi /= pi.sum(1, keepdims=True)
    zg, zl = z[:, None, :4], z[:, 4:]
    p = (N(zg, d["pm"][None].astype(np.float64), d["ps"][None].astype(np.float64)).prod(2) / 5).sum(1) * N(zl, 0.0, 1.0).prod(1)
    q = (pi * N(zg, d["zm_all"].astype(np.float64), d["zs_all"].astype(np.float64)).prod(2)).sum(1) * N(zl, d["mu_l"].astype(np.float64), d["sig_l"].astype(np.float64)).prod(1)
    np.testing.assert_allclose(gr.ratio(z, *_args(d)), np.log(p / q), rtol=1e-10, atol=1e-10)


# ---------------------------------------------------------------- the bound: fp32 twin inside, mutants outside
@pytest.mark.parametrize("name,d", CASES, ids=[n for n, _ in CASES])
def test_fp32_twin_stays_inside_the_bound(name, d):
    z = _z32(d)
    ref = gr.ratio(z, *_args(d))
    got = gr.ratio(z, *_args(d), dtype=np.float32).astype(np.float64)
    bound = gr.ratio_bound(z, *_args(d))
    assert np.isfinite(ref).all() and np.isfinite(got).all() and np.isfinite(bound).all()
    print(name, "worst err / bound", (np.abs(got - ref) / bound).max(), "bound / |r|", (bound / np.maximum(np.abs(ref), 1e-30)).max())
    assert (np.abs(got - ref) <= bound).all()


@pytest.mark.parametrize("mutant", gr.MUTANTS)
def test_bound_rejects_the_mutant(mutant):
    """Each mutant of the twin leaves the bound on at least one image of the inputs the GPU cases use (a mutant that cannot act on a
    case -- no local latent, one component -- is not asked to fail there)."""
    rejected = []
    for name, d in CASES:
        n = d["zm_all"].shape[1]
        z = _z32(d)
        ref, bound = gr.ratio(z, *_args(d)), gr.ratio_bound(z, *_args(d))
        if mutant == "comp_plus_one":
            zmut = _z32(d, comp=(d["comp"] + 1) % n)
            with np.errstate(all="ignore"):
                got = gr.ratio(zmut, *_args(d))
        else:
            with np.errstate(all="ignore"):
                got = gr.ratio(z, *_args(d), mutant=mutant, dtype=np.float32 if mutant == "no_max" else np.float64).astype(np.float64)
        if not (np.abs(got - ref) <= bound).all():
            rejected.append(name)
    print(mutant, "rejected on", len(rejected), "of", len(CASES), rejected)
    assert rejected, mutant


def test_there_are_at_least_ten_mutants_and_the_issues_eight_are_among_them():
    assert len(gr.MUTANTS) >= 10
    assert {"no_log_pi", "no_log_n", "sigma_squared", "no_max", "short_loop", "pm_ps_swapped", "comp_plus_one", "local_sign"} <= set(gr.MUTANTS)


def test_component_permutation_leaves_the_twin_unchanged():
    d = gr.gaussian_case(3, 30, 8, 5, seed=53)
    z = _z32(d)
    perm = np.random.default_rng(1).permutation(30)
    got = gr.ratio(z, d["logits"][:, perm], d["zm_all"][:, perm], d["zs_all"][:, perm], d["pm"][perm], d["ps"][perm], d["mu_l"], d["sig_l"])
    np.testing.assert_allclose(got, gr.ratio(z, *_args(d)), rtol=1e-13, atol=1e-12)


def test_pick_is_the_inverse_cdf():
    logits = np.log(np.array([0.1, 0.2, 0.3, 0.4], np.float32))
    assert [gr.pick(logits, u) for u in (1e-7, 0.05, 0.11, 0.29, 0.31, 0.59, 0.61, 1.0)] == [0, 0, 1, 1, 2, 2, 3, 3]
    assert gr.pick(np.array([-30, -30, 30], np.float32), 0.5) == 2 and gr.pick(np.zeros(1, np.float32), 1.0) == 0
    counts = np.bincount([gr.pick(logits, (i + 0.5) / 2000) for i in range(2000)], minlength=4) / 2000
    assert np.abs(counts - [0.1, 0.2, 0.3, 0.4]).max() < 2e-3


# ---------------------------------------------------------------- the surface
def test_uniform_host_matches_a_numpy_philox(lib_built):
    from split_vae_amd import ops
    seen = []
    for seed, image, sample in [(0, 0, 0), (5, 1, 0), (5, 0, 1), (5, 64, 3), (2 ** 40 + 7, 2 ** 33 + 5, 1023), (2 ** 64 - 1, 123456789, 7)]:
        u = ops.iw_gm_uniform_host(seed, image, sample)
        assert u == gr.pick_uniform(seed, image, sample) and 0.0 < u <= 1.0
        seen.append(u)
    assert len(set(seen)) == len(seen)
    us = np.array([ops.iw_gm_uniform_host(3, i, k) for i in range(500) for k in range(4)])
    assert abs(us.mean() - 0.5) < 0.03 and abs(us.std() - 12 ** -0.5) < 0.02


def test_philox_restatement_known_answer():
    """Philox4x32-10 known answers (Random123 kat_vectors)."""
    assert gr.philox4x32((0, 0), [0, 0, 0, 0]) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert gr.philox4x32((0xffffffff, 0xffffffff), [0xffffffff] * 4) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]


def test_parser_has_gm_iw_samples_and_the_report_line():
    from split_vae_amd import iw, main as svmain
    ap = svmain.build_parser()
    assert ap.parse_args([]).gm_iw_samples == 0
    assert ap.parse_args(["--gm_iw_samples", "16"]).gm_iw_samples == 16
    assert "--gm_iw_samples" not in [f for f, _, _ in svmain.REFERENCE_OPTIONS] and "--gm_iw_samples" not in svmain.REFERENCE_SWITCHES
    line = iw.mixture_report_line(3, dict(gm_iw_joint=-2.5, gm_iw_x=-1.25, gm_bits_per_dim_x=0.5))
    assert line == "Test IW-3 mixture bound: joint -2.5000, x -1.2500 nats; x bits/dim 0.5000"
    assert iw.MIXTURE_HISTORY_KEYS == ("gm_iw_joint", "gm_iw_x", "gm_bits_per_dim_x")


@pytest.mark.parametrize("argv,needle", [(["--model", "lgvae", "--gm_iw_samples", "2"], "--iw_samples"),
                                         (["--model", "lggmvae", "--gm_iw_samples", "-1"], ">= 0"),
                                         (["--model", "gmvae", "--gm_iw_samples", "-3"], ">= 0")])
@pytest.mark.parametrize("entry", ["main", "evaluate"])
def test_gm_iw_samples_refusals_come_before_any_device_work(monkeypatch, capsys, argv, needle, entry):
    import torch
    import split_vae_amd
    from split_vae_amd import _lib, data, evaluate, main as svmain

    def boom(*a, **k):
        raise AssertionError("device / data work before the refusal")
    monkeypatch.setattr(split_vae_amd, "configure_hw_queues", boom)
    monkeypatch.setattr(torch.cuda, "is_available", boom)
    monkeypatch.setattr(torch.cuda, "_lazy_init", boom)
    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setattr(data, "get_dataset", boom)
    argv = argv + ["--synthetic", "-no_label"]
    with pytest.raises(SystemExit) as e:
        if entry == "main":
            svmain.main(argv)
        else:
            evaluate.main(argv + ["--weights", "nowhere.npz"])
    assert "--gm_iw_samples" in str(e.value) and needle in str(e.value)
    assert "Config:" not in capsys.readouterr().out


def test_evaluate_keeps_its_nothing_to_measure_text():
    from split_vae_amd import evaluate
    with pytest.raises(SystemExit) as e:
        evaluate.main(["--model", "lggmvae", "--synthetic", "-no_label", "--weights", "nowhere.npz"])
    assert str(e.value).startswith("nothing to measure: pass --iw_samples K")
