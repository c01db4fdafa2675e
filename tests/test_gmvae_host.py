"""GMVae (vae/model.py:277-298) on the host: the variable table, the global-only plan's parameter table and workspace, the host
cluster accuracy against a literal restatement of linear_assignment + CategoricalAccuracy (vae/trainer.py:40-68, :315-349), the fp64
restatement against its golden fixture, and the CLI selection.  No GPU needed."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gmvae_ref  # noqa: E402

H, K = 32, 30
G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gmvae_svhn32_b2.npz"))

# vae/model.py:277-287: encoder_x = Encoder(type='gmvae') (its variables, vae/model.py:48-79), decoder_x = Decoder(global_latent)
REFERENCE_NAMES = (["encoder_x/h_block/conv2d", "encoder_x/h_block/conv2d_1", "encoder_x/h_block/conv2d_2", "encoder_x/y_block/dense",
                    "encoder_x/y_block/dense_1", "encoder_x/y_dense", "encoder_x/h_top_dense", "encoder_x/z_prior_mean", "encoder_x/z_prior_sig",
                    "encoder_x/e1", "encoder_x/z_mean", "encoder_x/z_sig"] + ["decoder_x/d%d" % i for i in range(1, 6)])


def _desc(B=4, global_only=1, external=1, dtype=0, gl=128, ll=128):
    from split_vae_amd import _lib
    return _lib.LGVaeDesc(B, H, H, gl, ll, dtype, 40.0, external, global_only)


def test_gmvae_variables_match_reference_order(lib_built):
    from split_vae_amd import gmvae
    table = gmvae.variable_table(H, H, 128, K)
    assert len(table) == 34
    assert [n for n, _ in table] == [n + s for n in REFERENCE_NAMES for s in ("/kernel", "/bias")]
    assert [tuple(s) for _, s in table] == [tuple(s) for _, s in gmvae_ref.gmvae_param_shapes(H, H, 128, K)]
    assert tuple(table[24][1]) == (128, (H // 8) * (H // 8) * 128)         # d1 over z_x alone: the geometry of decoder_x_hat
    assert tuple(table[14][1]) == (K, 128) and tuple(table[10][1]) == (128, K)


def test_global_only_plan_tables_and_workspace(lib_built):
    from split_vae_amd import _lib, ops
    lib = _lib.load()
    d = _desc()
    table = ops.param_table(d)
    D1 = (H // 8) * (H // 8) * 128
    assert [n for n, _, _ in table] == ["decoder_x/d%d/%s" % (i, k) for i in range(1, 6) for k in ("kernel", "bias")]
    assert table[0][2] == (128, D1)
    want = table[-1][1] + (int(np.prod(table[-1][2])) + 3) // 4 * 4
    assert lib.sv_lgvae_param_count(C.byref(d)) == want == sum((int(np.prod(s)) + 3) // 4 * 4 for _, _, s in table)
    assert lib.sv_lgvae_param_info(C.byref(d), 10, None, None, None, None) == _lib.STATUS_BADARG      # 10 arrays only
    for dtype in (_lib.SV_F32, _lib.SV_BF16):
        for B in (2, 64):
            ws = []
            for go in (1, 0):
                h = C.c_void_p()
                assert lib.sv_lgvae_plan_create(C.byref(_desc(B, go, 1, dtype)), C.byref(h)) == 0
                ws.append(lib.sv_lgvae_workspace_bytes(h))
                off, nb = C.c_int64(), C.c_int64()
                assert lib.sv_lgvae_buffer(h, b"gz_x", C.byref(off), C.byref(nb)) == 0
                assert nb.value == B * (128 if go else 256) * 4                      # dz pitch: decoder_x's input width
                rc = lib.sv_lgvae_buffer(h, b"out6_xh", C.byref(off), C.byref(nb))
                assert (rc == _lib.STATUS_BADARG) == bool(go)                         # no x-hat network
                lib.sv_lgvae_plan_destroy(h)
            assert 0 < ws[0] < ws[1], ws
    # global_only without the caller's encoder is refused; local_latent is ignored in the mode
    h = C.c_void_p()
    assert lib.sv_lgvae_plan_create(C.byref(_desc(external=0)), C.byref(h)) == _lib.STATUS_BADARG
    assert lib.sv_lgvae_param_count(C.byref(_desc(external=0))) < 0
    assert lib.sv_lgvae_param_count(C.byref(_desc(ll=0))) == want
    # the two-branch descriptor is unchanged by the new field (positional construction leaves it 0)
    two = _lib.LGVaeDesc(4, H, H, 128, 128, 0, 40.0)
    assert two.global_only == 0 and lib.sv_lgvae_param_count(C.byref(two)) > want and len(ops.param_table(two)) == 40


def _onehot(idx, C_):
    return np.eye(C_, dtype=np.float32)[idx]


def test_cluster_accuracy_matches_linear_assignment():
    from split_vae_amd.gmvae import accuracy_from_counts, cluster_accuracy
    rng = np.random.default_rng(0)
    for K_, C_, N in ((30, 10, 200), (10, 10, 57), (4, 10, 40), (12, 3, 31), (30, 10, 7)):     # K != C both ways, empty clusters
        for trial in range(6):
            lab = _onehot(rng.integers(0, C_, N), C_)
            logits = rng.standard_normal((N, K_)).astype(np.float32)
            if trial % 2:
                logits = np.round(logits)                                 # ties inside rows: the first index wins (tf.argmax)
            want = gmvae_ref.linear_assignment_accuracy(lab, logits)
            assert cluster_accuracy(lab, logits) == pytest.approx(want, abs=1e-12), (K_, C_, N, trial)
    # a tied majority: cluster 0 holds two of class 1 and two of class 2 -- either class is right for half of them
    lab = _onehot(np.array([1, 2, 2, 1, 0]), 3)
    logits = _onehot(np.array([0, 0, 0, 0, 1]), 2)
    assert cluster_accuracy(lab, logits) == gmvae_ref.linear_assignment_accuracy(lab, logits) == pytest.approx(3 / 5)
    # only some clusters used: the empty ones contribute nothing
    counts = np.zeros((5, 3), np.int64)
    counts[1] = [3, 1, 0]
    counts[4] = [0, 2, 2]
    assert accuracy_from_counts(counts) == pytest.approx(5 / 8)
    assert cluster_accuracy(np.zeros((0, 3)), np.zeros((0, 4))) == 0.0


def test_restatement_reproduces_golden():
    names = [n for n, _ in gmvae_ref.gmvae_param_shapes(H, H, y_size=int(G["y_size"]))]
    params = gmvae_ref.gmvae_glorot_init(H, H, seed=int(G["weight_seed"]), y_size=int(G["y_size"]))
    rngb = np.random.Generator(np.random.PCG64(97))
    for i, n in enumerate(names):
        if n.endswith("bias"):
            params[i] = (params[i] + rngb.standard_normal(params[i].shape) * 0.05).astype(np.float32)
    assert abs(sum(float(np.abs(p.astype(np.float64)).sum()) for p in params) - float(G["weight_checksum"])) < 1e-6
    from oracle import np_ref
    images = np_ref.scramble_batch(G["x"], G["perm"], int(G["patch"])).astype(np.float32)
    assert np.array_equal(images, G["images"])
    ref = gmvae_ref.GMVaeRefTrainer(params, float(G["beta"]), float(G["alpha"]), y_size=int(G["y_size"]), tau=float(G["tau"]))
    args = (images, G["eps_x"], G["u"], G["keep1"], G["keep5"])
    fwd, losses, grads = ref.grads(*args)
    for n, t in zip(gmvae_ref.NAMES9, fwd):
        assert np.abs(t.detach().numpy() - G["fwd_" + n]).max() < 1e-6 * max(1.0, float(np.abs(G["fwd_" + n]).max())), n
    for k in gmvae_ref.LOSS_KEYS:
        assert abs(float(losses[k].detach()) - float(G["loss_" + k])) < 1e-8 * abs(float(G["loss_" + k])) + 1e-12, k
    l = {k: float(v.detach()) for k, v in losses.items()}
    assert abs(l["total_loss"] - (l["x_recon_loss"] + 40 * l["x_kl_loss"] + 40 * l["y_kl_loss"])) < 1e-9 * abs(l["total_loss"])
    for i, g in enumerate(grads):
        gn = g.numpy().ravel()
        assert abs(np.linalg.norm(gn) - float(G["grad_norm_%02d" % i])) <= 1e-8 * float(G["grad_norm_%02d" % i]) + 1e-15, i
        idx = np.unique(np.linspace(0, gn.size - 1, min(48, gn.size)).astype(np.int64))
        assert np.allclose(gn[idx], G["grad_samp_%02d" % i], rtol=1e-8, atol=1e-15), i
    for step in (1, 2):
        l, _ = ref.train_step(*args)
        assert abs(l["total_loss"] - float(G["step%d_total_loss" % step])) < 1e-8 * abs(float(G["step%d_total_loss" % step])), step


def test_cli_gmvae_builds_a_gmvae(monkeypatch):
    """vae/main.py:70-73: --model gmvae -> GMVae(global_latent_dims, image_shape, y_size, tau) with ExponentialDecay(lr, 1e6, 0.4,
    staircase=True) Adam.  The constructor is recorded, not run (it needs the device)."""
    from split_vae_amd import gmvae
    from split_vae_amd.main import build_parser, make_model
    from split_vae_amd.optimizer import ExponentialDecay
    from split_vae_amd.utils import dotdict
    seen = {}

    class Rec:
        def __init__(self, **kw):
            seen.update(kw)
    monkeypatch.setattr(gmvae, "GMVae", Rec)
    a = build_parser().parse_args(["--model", "gmvae", "--patch_size", "4", "--y_size", "20", "--tau", "0.5", "--gm_dropout", "tf2.1"])
    assert a.model == "gmvae"
    model, opt = make_model(a.model, dotdict(vars(a)), [-1, 32, 32, 3])
    assert isinstance(model, Rec)
    assert seen == dict(global_latent_dims=128, image_shape=[-1, 32, 32, 3], y_size=20, tau=0.5, dtype="f32", seed=0, dropout_in_training=True)
    sch = opt.learning_rate
    assert isinstance(sch, ExponentialDecay)
    assert (sch.initial_learning_rate, sch.decay_steps, sch.decay_rate, sch.staircase) == (1e-4, 1000000, 0.4, True)
    with pytest.raises(ValueError):
        make_model("vae", dotdict(vars(a)), [-1, 32, 32, 3])
