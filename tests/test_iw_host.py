"""Host side of the importance-weighted log-likelihood (split_vae_amd/iw.py): the float64 streaming twin (tests/iw_ref.py) against
numpy.logaddexp.reduce, the bounds of L_K, the bits/dim conversion and the CLI surface.  No GPU."""
import math

import numpy as np
import pytest

import iw_ref


def _lk(lw):
    lw = np.asarray(lw, np.float64)
    return float(np.logaddexp.reduce(lw) - math.log(len(lw)))


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


def test_streaming_k1_returns_the_weight_itself():
    for v in (-17234.56789, 0.0, 3.25, -1e-3):
        assert iw_ref.stream_lse([v]) == v
    st = iw_ref.state_push(iw_ref.state_init(2), [100.0, 7.5], [50.0, 2.5], [-3.0, 1.0])
    assert np.array_equal(st[:, 0], [-153.0, -9.0]) and np.array_equal(st[:, 1], [1.0, 1.0])
    assert np.array_equal(st[:, 2], [-103.0, -6.5]) and np.array_equal(st[:, 3], [1.0, 1.0])
    assert np.array_equal(iw_ref.finish(st, 1), [[-153.0, -103.0, -153.0], [-9.0, -6.5, -9.0]])


def test_streaming_matches_logaddexp():
    rng = np.random.default_rng(0)
    cases = [np.array([-2.0e4, -1.0e4]), np.array([-1.0e4, -2.0e4, -1.5e4]),          # weights 1e4 nats apart
             np.full(7, -12345.678), np.full(64, 0.25),                              # all equal
             -1.7e4 + 30.0 * rng.standard_normal(64), 1e3 * rng.standard_normal(33)]
    for lw in cases:
        assert _rel(iw_ref.stream_lse(lw), _lk(lw)) <= 1e-12, lw
    assert iw_ref.stream_lse(np.full(7, -12345.678)) == pytest.approx(-12345.678, rel=1e-15)


def test_streaming_state_stays_finite_up_to_64_samples():
    rng = np.random.default_rng(1)
    for K in (1, 2, 3, 17, 64):
        B = 4
        st = iw_ref.state_init(B)
        for k in range(K):
            st = iw_ref.state_push(st, 1.7e4 + 1e3 * rng.standard_normal(B), 1.6e4 + 1e3 * rng.standard_normal(B), -300 + 50 * rng.standard_normal(B))
            assert np.isfinite(st).all() and (st[:, 1] >= 1.0).all() and (st[:, 3] >= 1.0).all()
        assert np.isfinite(iw_ref.finish(st, K)).all()


def test_streaming_is_order_independent():
    rng = np.random.default_rng(2)
    for scale in (1.0, 30.0, 1e3):
        lw = -1.7e4 + scale * rng.standard_normal(48)
        want = iw_ref.stream_lse(lw)
        for _ in range(8):
            assert _rel(iw_ref.stream_lse(rng.permutation(lw)), want) <= 1e-12
        assert _rel(iw_ref.stream_lse(np.sort(lw)), want) <= 1e-12 and _rel(iw_ref.stream_lse(np.sort(lw)[::-1]), want) <= 1e-12


def test_bound_lies_between_the_mean_and_the_max_weight():
    rng = np.random.default_rng(3)
    for K in (1, 2, 5, 64):
        for scale in (1e-3, 1.0, 100.0):
            lw = -1.7e4 + scale * rng.standard_normal(K)
            L = iw_ref.stream_lse(lw)
            slack = 1e-12 * abs(L)
            assert lw.mean() - slack <= L <= lw.max() + slack


def test_state_twin_against_direct_formulas():
    rng = np.random.default_rng(4)
    K, B = 6, 5
    nx, nh, r = 1.7e4 + 400 * rng.standard_normal((K, B)), 1.6e4 + 100 * rng.standard_normal((K, B)), -300 + 60 * rng.standard_normal((K, B))
    st = iw_ref.state_init(B)
    for k in range(K):
        st = iw_ref.state_push(st, nx[k], nh[k], r[k])
    out = iw_ref.finish(st, K)
    lw_j, lw_x = -nx - nh + r, -nx + r
    for b in range(B):
        assert _rel(out[b, 0], _lk(lw_j[:, b])) <= 1e-12 and _rel(out[b, 1], _lk(lw_x[:, b])) <= 1e-12
        assert _rel(out[b, 2], lw_j[:, b].mean()) <= 1e-12
    acc = iw_ref.acc_add(iw_ref.acc_add(np.zeros(4), out), out[:3])
    assert acc[3] == 8 and np.allclose(acc[:3], out.sum(0) + out[:3].sum(0), rtol=1e-13, atol=0)


def test_latent_ratio_is_the_density_ratio():
    rng = np.random.default_rng(5)
    mu, sig, eps = rng.standard_normal((3, 40)), np.exp(rng.uniform(-13, 2.3, (3, 40))), rng.standard_normal((3, 40))
    z = mu + sig * eps
    log_p = -0.5 * z * z - 0.5 * math.log(2 * math.pi)
    log_q = -0.5 * ((z - mu) / sig) ** 2 - np.log(sig) - 0.5 * math.log(2 * math.pi)
    want = (log_p - log_q).sum(1)
    np.testing.assert_allclose(iw_ref.latent_ratio(mu, sig, eps=eps), want, rtol=1e-7)
    np.testing.assert_allclose(iw_ref.latent_ratio(mu, sig, z_stored=z), want, rtol=1e-7)


def test_bits_per_dim_conversion():
    from split_vae_amd import iw
    # one bit per sub-pixel: log p(x) = -(H W 3) ln 2
    assert iw.bits_per_dim(-32 * 32 * 3 * math.log(2.0), 32, 32) == pytest.approx(1.0, rel=1e-15)
    # the uniform distribution over the 256 levels: 8 bits per dimension, no offset
    assert iw.bits_per_dim(64 * 64 * 3 * math.log(1.0 / 256.0), 64, 64) == pytest.approx(8.0, rel=1e-15)
    assert iw.bits_per_dim(-17000.0, 32, 32) == pytest.approx(17000.0 / (3072 * math.log(2.0)), rel=1e-15)
    assert iw.bits_per_dim(-17000.0, 32, 32) == pytest.approx(iw_ref.bits_per_dim(-17000.0, 32, 32), rel=1e-15)
    line = iw.report_line(3, dict(iw_joint=-2.5, iw_x=-1.25, bits_per_dim_x=0.5))
    assert line == "Test IW-3 bound: joint -2.5000, x -1.2500 nats; x bits/dim 0.5000"


def test_parser_has_iw_samples_outside_the_reference_options():
    from split_vae_amd import main as svmain
    ap = svmain.build_parser()
    assert ap.parse_args([]).iw_samples == 0
    assert ap.parse_args(["--iw_samples", "64"]).iw_samples == 64
    assert "--iw_samples" not in [f for f, _, _ in svmain.REFERENCE_OPTIONS]
    assert "--iw_samples" not in svmain.REFERENCE_SWITCHES


@pytest.mark.parametrize("model_name", ["lggmvae", "gmvae"])
@pytest.mark.parametrize("entry", ["main", "evaluate"])
def test_iw_samples_is_refused_for_the_mixture_models_before_any_device_work(monkeypatch, capsys, model_name, entry):
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
    argv = ["--model", model_name, "--iw_samples", "2", "--synthetic", "-no_label"]
    with pytest.raises(SystemExit) as e:
        if entry == "main":
            svmain.main(argv)
        else:
            evaluate.main(argv + ["--weights", "nowhere.npz"])
    msg = str(e.value)
    assert "--model %s" % model_name in msg and "lgvae only" in msg and "different estimator" in msg
    assert "Config:" not in capsys.readouterr().out
