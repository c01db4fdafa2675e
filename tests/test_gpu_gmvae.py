"""GPU tests of GMVae (vae/model.py:277-298) + train_step_gm_vae / test_step_gm_vae (vae/trainer.py:176-198, :277-294) against the fp64
restatement (tests/gmvae_ref.py) on identical inputs, weights and random draws; the cluster-count kernel against numpy; the CLI loop."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import np_ref, torch_ref

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gmvae_ref  # noqa: E402

pytestmark = pytest.mark.gpu

H, PATCH, BETA, ALPHA, K, TAU = 32, 4, 40.0, 40.0, 30, 0.4


@pytest.fixture(scope="module")
def ops(lib_built):
    assert torch.cuda.is_available()
    from split_vae_amd import ops as o
    return o


def _inputs(B, seed=0):
    rng = np.random.Generator(np.random.PCG64(seed))
    x = (rng.integers(0, 256, size=(B, H, H, 3)) / 255.0 * 2 - 1).astype(np.float32)
    perm = np.stack([rng.permutation((H // PATCH) ** 2) for _ in range(B)]).astype(np.int32)
    images = np_ref.scramble_batch(x, perm, PATCH).astype(np.float32)
    F_ = (H // 8) ** 2 * 128
    noise = dict(eps=rng.standard_normal((B, 128)).astype(np.float32), u=rng.uniform(0.02, 0.98, (B, K)).astype(np.float32),
                 keep1=(rng.uniform(size=(B, 1024)) > 0.2).astype(np.float32), keep5=(rng.uniform(size=(B, F_)) > 0.2).astype(np.float32))
    return images, noise


def _params(seed=3):
    ps = gmvae_ref.gmvae_glorot_init(H, H, seed=seed, y_size=K)
    rng = np.random.default_rng(9)
    for i, (n, _) in enumerate(gmvae_ref.gmvae_param_shapes(H, H, y_size=K)):
        if n.endswith("bias"):
            ps[i] = (ps[i] + rng.standard_normal(ps[i].shape) * 0.05).astype(np.float32)    # exercise the bias paths
    return ps


def _model(dtype="f32", seed=1, dropout=False):
    from split_vae_amd.gmvae import GMVae
    m = GMVae(128, [-1, H, H, 3], K, TAU, dtype=dtype, device="cuda", seed=seed, dropout_in_training=dropout)
    m.beta, m.alpha = BETA, ALPHA
    return m


def test_gmvae_variables_and_trainer_dispatch(ops):
    from split_vae_amd import trainer
    from split_vae_amd.optimizer import Adam
    m = _model()
    want = gmvae_ref.gmvae_param_shapes(H, H, y_size=K)
    assert m.keras_names() == [n + ":0" for n, _ in want]
    assert [tuple(v.shape) for v in m.trainable_variables] == [tuple(s) for _, s in want]
    b = dict(zip(m.keras_names(), m.get_weights()))
    assert np.all(b["encoder_x/z_sig/bias:0"] == 1) and np.all(b["decoder_x/d1/bias:0"] == 0)
    img = torch.zeros((4, H, H, 6), device="cuda")
    with pytest.raises(TypeError, match="train_step_gm_vae"):
        trainer.train_step(m, img, Adam())
    with pytest.raises(Exception):
        m.plan(4).graph_enable(True)                     # global-only plans have no capture path


@pytest.mark.parametrize("dropout", [False, True], ids=["tf2.0-no-dropout", "tf2.1-dropout"])
@pytest.mark.parametrize("order", ["deterministic", "default"])
def test_gmvae_step_fp32_matches_restatement(ops, request, dropout, order):
    """One fp32 step against the fp64 restatement: the 9-tuple, the four metrics, all 34 gradients and the Adam update; then a
    3-step loss curve.  Tolerances of tests/test_gpu_gm.py (the default order's split-K atomics: its one-ReLU-gate allowance)."""
    if order == "deterministic":
        request.getfixturevalue("deterministic")
    strict = order == "deterministic"
    from split_vae_amd.gmvae import GM_LOSS_KEYS, train_step_gm_vae
    from split_vae_amd.optimizer import Adam
    B = 4
    images, nz = _inputs(B)
    params = _params()
    ref = gmvae_ref.GMVaeRefTrainer(params, BETA, ALPHA, y_size=K, tau=TAU, dtype=torch.float64, dropout=dropout)
    model = _model(dropout=dropout)
    model.set_weights(params)
    opt = Adam(learning_rate=1e-4)
    cu = lambda a: torch.from_numpy(a).cuda()
    img, eps, noise = cu(images), cu(nz["eps"]), (cu(nz["u"]), cu(nz["keep1"]), cu(nz["keep5"]))
    args = (images, nz["eps"], nz["u"], nz["keep1"], nz["keep5"])

    fwd_ref, _, _ = ref.grads(*args)
    out = model(img, training=True, eps=eps, noise=noise)
    assert len(out) == 9
    for name, got, want in zip(gmvae_ref.NAMES9, out, fwd_ref):
        want = want.detach()
        torch.testing.assert_close(got.double().cpu(), want, rtol=1e-4 if strict else 2e-4,
                                   atol=(1e-5 if strict else 2e-4) * max(1.0, float(want.abs().max())), msg=lambda m: name + ": " + m)

    curve_got, curve_ref = [], []
    for t in range(1, 4):
        fwd_ref, loss_ref, g_ref = ref.grads(*args)
        metrics = train_step_gm_vae(model, img, opt, eps=eps, noise=noise).cpu().double()
        curve_got.append(float(metrics[3]))
        curve_ref.append(float(loss_ref["total_loss"].detach()))
        for i, k in enumerate(GM_LOSS_KEYS):
            want = float(loss_ref[k].detach())
            assert abs(float(metrics[i]) - want) <= 2e-4 * abs(want) + 1e-5, (t, k, float(metrics[i]), want)
        for name, got, want in zip(model.keras_names(), model.gradients, g_ref):
            scale = float(want.abs().max())
            got = got.double().cpu()
            try:
                torch.testing.assert_close(got, want, rtol=2e-3, atol=2e-3 * scale + 1e-9, msg=lambda m: "step %d grad %s: %s" % (t, name, m))
            except AssertionError:
                if strict:
                    raise
                # a decoder ReLU unit within fp32 summation-order noise of zero (tests/test_gpu_gm.py): its gate may fall the other way
                bad = ((got - want).abs() > 2e-3 * scale + 2e-3 * want.abs()).double().mean()
                rel = float((got - want).norm() / want.norm().clamp_min(1e-30))
                assert float(bad) <= 2e-3 and rel <= 5e-3, "step %d grad %s: %.2e off, relative L2 %.2e" % (t, name, float(bad), rel)
        before = [p.detach().clone() for p in ref.params]
        ref.t += 1
        torch_ref.keras_adam_(ref.params, g_ref, ref.m, ref.v, ref.t, ref.lr)
        upd_ref = torch.cat([(a.detach() - b).flatten() for a, b in zip(ref.params, before)])
        upd_got = torch.cat([(torch.as_tensor(w).double() - b).flatten() for w, b in zip(model.get_weights(), before)])
        agree = float((torch.sign(upd_ref) == torch.sign(upd_got)).double().mean())
        assert agree > 0.995, agree
        assert float((upd_ref - upd_got).abs().max()) <= 2.1e-4
        with torch.no_grad():
            for p, w in zip(ref.params, model.get_weights()):
                p.copy_(torch.as_tensor(w).double())
    assert np.allclose(curve_got, curve_ref, rtol=2e-4), (curve_got, curve_ref)
    assert curve_got[-1] < curve_got[0], curve_got


def test_gmvae_bf16_close_to_fp32_and_eval_mode(ops):
    """bf16 contractions: the step's metrics near the fp32 step's; evaluation (training=False) applies no dropout and matches the
    restatement without dropout."""
    from split_vae_amd.gmvae import GM_LOSS_KEYS, test_step_gm_vae, train_step_gm_vae
    from split_vae_amd.optimizer import Adam
    B = 8
    images, nz = _inputs(B, seed=5)
    params = _params()
    cu = lambda a: torch.from_numpy(a).cuda()
    eps, noise = cu(nz["eps"]), (cu(nz["u"]), None, None)
    ref = gmvae_ref.GMVaeRefTrainer(params, BETA, ALPHA, y_size=K, tau=TAU, dtype=torch.float64, dropout=False)
    _, loss_ref = ref.forward_losses(images, nz["eps"], nz["u"], nz["keep1"], nz["keep5"])
    res = {}
    for dtype in ("f32", "bf16"):
        m = _model(dtype, dropout=True)
        m.set_weights(params)
        ev = test_step_gm_vae(m, cu(images), eps=eps, noise=noise).cpu()
        tol = 2e-4 if dtype == "f32" else 2e-2
        for i, k in enumerate(GM_LOSS_KEYS):
            want = float(loss_ref[k].detach())
            assert abs(float(ev[i]) - want) <= tol * abs(want) + tol, (dtype, k, float(ev[i]), want)
        res[dtype] = train_step_gm_vae(m, cu(images), Adam(learning_rate=1e-4), eps=eps).cpu().double().numpy()
        assert m(cu(images))[0].shape == (B, H, H, 3)
    assert np.allclose(res["bf16"], res["f32"], rtol=2e-2, atol=2e-2), res


def test_gmvae_training_descends_with_device_rng(ops):
    from split_vae_amd.gmvae import train_step_gm_vae
    from split_vae_amd.optimizer import Adam
    B = 16
    images, _ = _inputs(B, seed=7)
    img = torch.from_numpy(images).cuda()
    for dtype, dropout in (("bf16", True), ("f32", False)):
        model = _model(dtype, seed=4, dropout=dropout)
        opt = Adam(learning_rate=1e-3)
        tot = [float(train_step_gm_vae(model, img, opt)[3]) for _ in range(15)]
        assert all(np.isfinite(tot)) and min(tot[-3:]) < tot[0], (dtype, tot)


def test_gmvae_staged_step_is_bit_identical(ops, deterministic):
    """Inputs staged by the augmentation (Augmentator.augment(..., plan=model.plan(B))): the step skips its split / pad pass and is
    otherwise the same launch sequence -- three steps bit-identical to the un-staged ones."""
    from split_vae_amd import data
    from split_vae_amd.augmentation import Augmentator
    from split_vae_amd.gmvae import train_step_gm_vae
    from split_vae_amd.optimizer import Adam
    B = 32
    x = data.synthetic_images(B, H, H, seed=0, device="cuda")
    res = []
    for staged in (False, True):
        model = _model("f32", seed=4)
        opt = Adam(learning_rate=1e-3)
        aug = Augmentator("scramble", size=PATCH, seed=1)
        ms = []
        for _ in range(3):
            img = aug.augment(x, plan=model.plan(B) if staged else None)
            assert (getattr(img, "_sv_staged_plan", None) is not None) == staged
            ms.append(train_step_gm_vae(model, img, opt).cpu().numpy())
        torch.cuda.synchronize()
        res.append((np.stack(ms), model.flat.cpu().numpy(), model.gm_flat.cpu().numpy()))
    for a, b in zip(res[0], res[1]):
        assert np.array_equal(a, b)


def test_gmvae_weights_round_trip(ops, tmp_path, deterministic):
    from split_vae_amd import h5io
    m = _model("f32", seed=2)
    img = torch.from_numpy(_inputs(4, seed=3)[0]).cuda()
    eps = torch.zeros((4, 128), device="cuda")
    noise = (torch.full((4, K), 0.5, device="cuda"), None, None)
    path = m.save_weights(str(tmp_path / ("w.h5" if h5io.available() else "w")))
    if h5io.available():
        layers = h5io.load_keras_weights(path)
        assert [w for _, ws in layers for w, _ in ws][0].startswith("gm_vae/encoder/")
        assert sum(len(ws) for _, ws in layers) == 34
    m2 = _model("f32", seed=9)
    m2.load_weights(path)
    for a, b in zip(m.get_weights(), m2.get_weights()):
        assert np.array_equal(a, b)
    o1, o2 = m(img, eps=eps, noise=noise), m2(img, eps=eps, noise=noise)
    for a, b in zip(o1, o2):
        torch.testing.assert_close(a, b, rtol=1e-6, atol=1e-6)
    y, logits = m.get_y(img[..., :3])                    # (y_logits precede the Gumbel noise and do not depend on it)
    torch.testing.assert_close(logits, o1[6], rtol=1e-6, atol=1e-6)
    z = m.encode(img, eps=eps)
    assert z.shape == (4, 128) and bool(torch.isfinite(z).all())
    rec = m.decode(z)
    assert rec.shape == (4, H, H, 3) and float(rec.min()) >= 0 and float(rec.max()) <= 1
    pm, ps = m.encode_y(torch.eye(K, device="cuda")[:3])
    assert pm.shape == (3, 128) and bool((ps > 0).all())


def test_cluster_confusion_matches_numpy(ops):
    from split_vae_amd.gmvae import ClusterAccuracy, accuracy_from_counts, cluster_accuracy
    rng = np.random.default_rng(1)
    Kc, Cc = 30, 10
    acc = ClusterAccuracy(Kc, Cc, "cuda")
    labs, logs = [], []
    for B in (64, 1, 300, 17):
        lab = np.eye(Cc, dtype=np.float32)[rng.integers(0, Cc, B)]
        lg = np.round(rng.standard_normal((B, Kc)) * 0.7).astype(np.float32)      # many ties inside rows: the first index wins
        lg[0] = 0.0                                                              # an all-equal row -> cluster 0
        acc.update(torch.from_numpy(lg).cuda(), torch.from_numpy(lab).cuda())
        labs.append(lab)
        logs.append(lg)
    L, G = np.concatenate(labs), np.concatenate(logs)
    want = np.zeros((Kc, Cc), np.int64)
    np.add.at(want, (np.argmax(G, axis=1), np.argmax(L, axis=1)), 1)
    got = acc.counts.cpu().numpy()
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert acc.result() == accuracy_from_counts(want) == pytest.approx(cluster_accuracy(L, G))
    assert acc.result() == pytest.approx(gmvae_ref.linear_assignment_accuracy(L, G))
    # a row pitch wider than K (a view of a padded buffer)
    acc.reset_states()
    wide = torch.zeros((5, 40), device="cuda")
    wide[:, 3] = 1.0
    acc.update(wide[:, :Kc].contiguous(), torch.from_numpy(labs[0][:5]).cuda())
    assert int(acc.counts[3].sum()) == 5 and int(acc.counts.sum()) == 5


def test_lgvae_step_unchanged_by_a_gmvae_in_the_process(ops, deterministic):
    """The two-branch plan does not change: an LGVae step is bit-identical before and after a GMVae (and its global-only plan) has been
    created and trained in the same process."""
    from split_vae_amd import trainer
    from split_vae_amd.gmvae import train_step_gm_vae
    from split_vae_amd.model import LGVae
    from split_vae_amd.optimizer import Adam
    B = 8
    images, nz = _inputs(B, seed=11)
    img = torch.from_numpy(images).cuda()
    eps = (torch.from_numpy(nz["eps"]).cuda(), torch.from_numpy(nz["eps"][::-1].copy()).cuda())

    def lgvae_step():
        m = LGVae(128, 128, [-1, H, H, 3], dtype="f32", seed=5)
        m.beta = BETA
        plan = trainer.train_step(m, img, Adam(learning_rate=1e-4), eps=eps)
        torch.cuda.synchronize()
        return plan.buffer("losses", torch.float32, (8,)).cpu().numpy(), m.flat.cpu().numpy()

    before = lgvae_step()
    g = _model("f32")
    train_step_gm_vae(g, img, Adam(learning_rate=1e-4))
    torch.cuda.synchronize()
    after = lgvae_step()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


@pytest.mark.parametrize("model_name", ["gmvae", "lggmvae"])
def test_main_runs_gm_models_on_svhn_files(tmp_path, monkeypatch, capsys, lib_built, model_name):
    """main() end to end on tiny SVHN .mat files: with labels the cluster accuracy is reported, without labels it is not; weights
    are saved either way."""
    from split_vae_amd import main as svmain
    from test_host_logic import _write_svhn
    _write_svhn(str(tmp_path / "data"), n_train=30, n_extra=9, n_test=27)
    monkeypatch.chdir(tmp_path)
    for flags in ([], ["-no_label"]):
        path = svmain.main(["--model", model_name, "--beta", "40", "--patch_size", "4", "--batch_size", "12", "--training_steps", "2",
                            "--log_every", "2", "--dtype", "f32"] + flags)
        out = capsys.readouterr().out
        assert "Training step 0" in out and "Training step 2" in out and "Training done!" in out
        assert ("Classifier cluster acc" in out) == (not flags), out
        assert os.path.exists(path)
        if not flags:
            accs = [float(l.split(":")[1]) for l in out.splitlines() if "Classifier cluster acc" in l]
            assert len(accs) == 2 and all(0.0 <= a <= 1.0 for a in accs)
    if model_name == "gmvae":
        assert not os.path.exists(str(tmp_path / "output"))              # no image grids for GMVae (vae/trainer.py:386)
