"""The SPAIR evaluation kernels (spair_eval.hip) against their numpy restatements (tests/spair_eval_ref.py), the native labelled
test_step against the op-by-op one, the figures of spair_visualizer.py pixel by pixel, and the -viz / count-accuracy surface of
spair_main."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spair_eval_ref as er  # noqa: E402

pytestmark = pytest.mark.gpu


def _edge_boxes(NB):
    """Edge cases first, then random boxes over [-0.3, 1.3]: inverted, outside on every side, zero, exact pixel hits, degenerate lines."""
    fixed = [[0.6, 0.2, 0.4, 0.6], [0.2, 0.6, 0.4, 0.2], [1.2, 0.2, 1.5, 0.6], [-0.9, 0.2, -0.2, 0.6], [0.2, 1.3, 0.6, 1.6],
             [0.2, -0.8, 0.6, -0.3], [0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 1.0, 1.0], [-0.05, -0.05, 1.05, 1.05], [0.5, 0.1, 0.5, 0.9],
             [0.1, 0.5, 0.9, 0.5], [-0.15, 0.3, 0.4, 1.2], [0.25, 0.25, 0.75, 0.75]]
    return np.array(fixed[:NB], np.float32)


def _case(B, H, W, Cc, NB, seed):
    rng = np.random.default_rng(seed)
    img = rng.random((B, H, W, Cc), dtype=np.float32)
    boxes = rng.uniform(-0.3, 1.3, (B, NB, 4)).astype(np.float32)
    e = _edge_boxes(NB)
    boxes[0, :len(e)] = e
    return img, boxes


@pytest.mark.parametrize("Cc", [1, 3, 4])
@pytest.mark.parametrize("gated", [False, True])
def test_draw_bounding_boxes_bit_exact(lib_built, Cc, gated):
    from split_vae_amd import ops
    B, H, W, NB = 3, 13, 21, 16
    img, boxes = _case(B, H, W, Cc, NB, seed=Cc * 10 + gated)
    rng = np.random.default_rng(7)
    colors = rng.random((3, 5), dtype=np.float32)               # 3 colours, row pitch 5 >= C
    gate = None
    if gated:
        gate = rng.integers(0, 2, (B, NB)).astype(np.float32)
        gate[1, ::3] = rng.random(gate[1, ::3].shape, dtype=np.float32)      # fractional gates scale the boxes
    want = er.draw_bounding_boxes(img, boxes, colors, gate=gate)
    dimg, dbox, dcol = torch.from_numpy(img).cuda(), torch.from_numpy(boxes).cuda(), torch.from_numpy(colors).cuda()
    dgate = None if gate is None else torch.from_numpy(gate).cuda()
    out = ops.draw_bounding_boxes(dimg, dbox, dcol, gate=dgate)             # out of place
    assert np.array_equal(out.cpu().numpy(), want)
    assert np.array_equal(dimg.cpu().numpy(), img)                          # the input is untouched
    ops.draw_bounding_boxes(dimg, dbox, dcol, gate=dgate, out=dimg)         # in place
    assert np.array_equal(dimg.cpu().numpy(), want)


def test_draw_bounding_boxes_torch_op_and_origin_dot(lib_built):
    import split_vae_amd.torch_ops  # noqa: F401
    img = torch.zeros(2, 8, 12, 3).cuda()
    boxes = torch.tensor([[[0.25, 0.25, 0.75, 0.75]], [[0.25, 0.25, 0.75, 0.75]]]).cuda()
    gate = torch.tensor([[0.0], [1.0]]).cuda()
    out = torch.ops.split_vae.draw_bounding_boxes(img, boxes, torch.ones(1, 4).cuda(), gate).cpu().numpy()
    drawn0 = np.argwhere(out[0].any(-1))
    assert drawn0.tolist() == [[0, 0]]                                      # the gated-off box's dot (spair/visualizer.py:109)
    assert np.array_equal(out, er.draw_bounding_boxes(img.cpu().numpy(), boxes.cpu().numpy(), np.ones((1, 4), np.float32),
                                                      gate.cpu().numpy()))
    with pytest.raises(NotImplementedError):
        torch.ops.split_vae.draw_bounding_boxes(img.cpu(), boxes.cpu(), torch.ones(1, 4), None)


def test_refused_calls_leave_buffers_untouched(lib_built):
    from split_vae_amd import _lib
    lib = _lib.load()
    p = lambda t: C.c_void_p(t.data_ptr())
    img = torch.rand(1, 8, 8, 4).cuda()
    boxes = torch.tensor([[[0.1, 0.1, 0.9, 0.9]]]).cuda()
    out = torch.full_like(img, float("nan"))
    cols = torch.ones(2, 4).cuda()
    img0, out0 = img.clone(), out.clone()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.sv_draw_bounding_boxes(p(img), p(boxes), None, p(cols), p(out), 1, 8, 8, 4, 1, 2, 3, st) == _lib.STATUS_BADARG
    assert lib.sv_draw_bounding_boxes(p(img), p(boxes), None, p(cols), p(out), 1, 8, 8, 2, 1, 2, 4, st) == _lib.STATUS_BADARG
    assert lib.sv_draw_bounding_boxes(p(img), p(boxes), None, p(cols), p(img), 1, 8, 8, 4, 0, 2, 4, st) == _lib.STATUS_BADARG
    lg = torch.zeros(2, 16).cuda()
    lab = torch.zeros(2).cuda()
    met = torch.full((2,), 7.0).cuda()
    pred = torch.full((2,), 7.0).cuda()
    acc = torch.tensor([3, 4], dtype=torch.int32).cuda()
    assert lib.sv_spair_count_metrics(p(lg), 15, p(lab), p(pred), p(met), p(acc), 2, 16, st) == _lib.STATUS_BADARG
    assert lib.sv_spair_count_metrics(p(lg), 16, None, p(pred), p(met), p(acc), 2, 16, st) == _lib.STATUS_BADARG
    torch.cuda.synchronize()
    assert torch.equal(img, img0) and torch.equal(out.isnan(), out0.isnan())
    assert met.tolist() == [7.0, 7.0] and pred.tolist() == [7.0, 7.0] and acc.tolist() == [3, 4]


@pytest.mark.parametrize("B", [1, 37, 300])
def test_count_metrics_exact_and_accumulating(lib_built, B):
    from split_vae_amd import ops
    rng = np.random.default_rng(B)
    base = rng.normal(0.0, 3.0, (B, 20)).astype(np.float32)
    base[np.abs(base) < 1e-3] = 0.5
    base[0, 3] = 0.0                                           # not counted
    base[:, 16:] = np.nan                                      # the row pitch's tail is never read
    lg = base[:, :16]
    labels = rng.integers(0, 8, B).astype(np.float32)
    labels[0] = 0.0
    pred_ref, mae_ref, mape_ref, hits = er.count_metrics(lg, labels)
    dlg = torch.from_numpy(base).cuda()[:, :16]                # a [B,16] view at row pitch 20
    dlab = torch.from_numpy(labels).cuda()
    acc = torch.zeros(2, dtype=torch.int32).cuda()
    runs = []
    for _ in range(3):
        metrics, pred = ops.spair_count_metrics(dlg, dlab, acc=acc, want_pred=True)
        runs.append((metrics.cpu().numpy().copy(), pred.cpu().numpy().copy()))
    for metrics, pred in runs:
        assert np.array_equal(pred, pred_ref)
        assert metrics[0] == pytest.approx(mae_ref, rel=1e-6, abs=0)
        assert metrics[1] == pytest.approx(mape_ref, rel=1e-6, abs=0)
        assert metrics.tobytes() == runs[0][0].tobytes()        # same inputs, same bits
    assert acc.tolist() == [3 * hits, 3 * B]


def test_count_accuracy_object(lib_built):
    from split_vae_amd import spair_trainer
    ca = spair_trainer.CountAccuracy()
    assert ca.result() == 0.0                                  # un-updated: 0.0, as Keras' Accuracy
    lg = torch.full((3, 4, 4, 1), -5.0)
    lg[0, 0, :2] = 5.0
    lg[2, 1, 1] = 5.0
    ca.update(torch.tensor([2.0, 0.0, 3.0]).cuda(), lg.cuda())
    ca.update(torch.tensor([2.0]).cuda(), lg[:1].cuda())
    assert ca.acc.tolist() == [3, 4] and ca.result() == np.float32(0.75)
    ca.reset_states()
    assert ca.acc.tolist() == [0, 0]


CONFIGS = {
    "spair": dict(model="spair"),
    "bg_spair": dict(model="bg_spair", latent_size=64, bg_latent_size=4),
    "lg_spair": dict(model="lg_spair", latent_size=64, bg_latent_size=4, local_latent_size=4, patch_size=8, z_bg_beta=10.0,
                     split_z_l=True, concat_z_what=True, dense_local=True, dense_bg=True),
}


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


@pytest.mark.parametrize("name", list(CONFIGS))
def test_native_labelled_test_step_matches_op_by_op(lib_built, name, monkeypatch):
    from oracle import spair_model_ref as R
    from split_vae_amd import spair, spair_trainer
    from split_vae_amd.utils import dotdict
    cfg = dotdict(R.default_config(**CONFIGS[name]))
    B = 8
    chans = 6 if cfg.model == "lg_spair" else 3
    model = spair.get_model(cfg)
    model.set_weights({k: v.numpy() for k, v in R.init_params(cfg, seed=2).items()})
    # powers of two and a power-of-two batch: every |label - pred| / label and every sum of them is exact in fp32, so the kernel's
    # summation order and torch's give the same MAE / MAPE bits
    labels = torch.tensor([1.0, 2.0, 4.0, 8.0, 16.0, 1.0, 2.0, 4.0]).cuda()
    for seed in range(8):                                      # a batch whose logits keep clear of 0 (the count rounds sigmoid)
        images = torch.rand(B, 48, 48, chans, generator=torch.Generator().manual_seed(seed)).cuda()
        noise = {k: v.float().cuda() for k, v in R.draw_noise(cfg, B, seed=seed + 100).items()}
        monkeypatch.setenv("SV_SPAIR_AUTOGRAD", "1")
        ca_ref = spair_trainer.CountAccuracy()
        ref_out, ref_losses = spair_trainer.test_step(model, images, cfg, labels=labels, noise=noise, count_acc=ca_ref)
        ref_out = [t.clone() for t in ref_out]
        ref_losses = [float(l) for l in ref_losses]
        if float(ref_out[11].abs().min()) >= 1e-3:
            break
    assert float(ref_out[11].abs().min()) >= 1e-3
    monkeypatch.delenv("SV_SPAIR_AUTOGRAD")
    ca = spair_trainer.CountAccuracy()
    out, losses = spair_trainer.test_step(model, images, cfg, labels=labels, noise=noise, count_acc=ca)
    # the loss means (6 for 'spair', 9 for bg_spair / lg_spair: test_step :262-285), then MAE and MAPE
    assert len(out) == len(ref_out) and len(losses) == len(ref_losses) == (8 if name == "spair" else 11)
    for i, (a, b) in enumerate(zip(out, ref_out)):
        assert tuple(a.shape) == tuple(b.shape), i
        assert _rel(a, b) < 2e-4, (i, _rel(a, b))
    assert float(out[11].abs().min()) >= 1e-3
    for i in range(len(losses) - 2):
        assert abs(float(losses[i]) - ref_losses[i]) <= 2e-4 * max(abs(ref_losses[i]), 1e-6), (i, float(losses[i]), ref_losses[i])
    assert float(losses[-2]) == ref_losses[-2] and float(losses[-1]) == ref_losses[-1]    # MAE, MAPE
    assert ca.acc.tolist() == ca_ref.acc.tolist() and ca.acc.tolist()[1] == B


# ---------------------------------------------------------------- figures
def _q(a):
    """save_png's quantisation."""
    return np.clip(np.rint(np.asarray(a, np.float64) * 255.0), 0, 255).astype(np.uint8)


def _strip(x):
    return np.concatenate(list(x), axis=1)


def _cells(x):
    return np.concatenate([xi.reshape((-1,) + xi.shape[2:]) for xi in x], axis=1)


def _grey3(x):
    return np.repeat(x, 3, axis=-1)


def _panels_equal(path, panels):
    from split_vae_amd.visualizer import load_png
    got = load_png(path)
    widths = [p.shape[1] for p in panels]
    assert got.shape == (panels[0].shape[0], sum(widths) + 4 * (len(panels) - 1), 3), got.shape
    x = 0
    for i, p in enumerate(panels):
        assert np.array_equal(got[:, x:x + p.shape[1]], _q(p)), i
        x += p.shape[1]
        if i + 1 < len(panels):
            assert np.all(got[:, x:x + 4] == 255)
            x += 4


def _recon_ref(img, x_recon, z_pres, z_depth, full):
    """spair/visualizer.py:14-81 written out with numpy."""
    n, cells, H, W, _ = full.shape
    rgb, alpha = full[..., :3], full[..., 3:4]
    zp = z_pres.reshape(n, cells, 1, 1, 1)
    zd = z_depth.reshape(n, cells, 1, 1, 1).astype(np.float32)
    head = np.concatenate([_strip(img[..., :3]), _strip(x_recon)], axis=0)
    w = rgb * alpha * zp * (1.0 / (1.0 + np.exp(zd))).astype(np.float32)
    p3 = np.zeros_like(rgb)
    p3[..., 0] = np.broadcast_to(zp[..., 0], rgb.shape[:-1])
    return [np.concatenate([head, _cells(b)], axis=0) for b in (rgb, w, p3)]


@pytest.mark.parametrize("name", ["spair", "lg_spair"])
def test_figures_equal_numpy_canvases(lib_built, name, tmp_path):
    from oracle import spair_model_ref as R
    from split_vae_amd import spair, spair_trainer
    from split_vae_amd import spair_visualizer as V
    from split_vae_amd.utils import dotdict
    cfg = dotdict(R.default_config(**CONFIGS[name]))
    chans = 6 if cfg.model == "lg_spair" else 3
    B, n = 12, 10
    model = spair.get_model(cfg, seed=3)
    images = torch.rand(B, 48, 48, chans, generator=torch.Generator().manual_seed(4)).cuda()
    labels = torch.arange(B, dtype=torch.float32).cuda() % 6
    ds = [(images, labels)]
    with torch.no_grad():
        o = model(images[:n].contiguous())
    npo = [t.detach().float().cpu().numpy() for t in o]
    img = images[:n].cpu().numpy()
    pres = torch.round(torch.sigmoid(o[11])).reshape(n, -1).cpu().numpy()      # tf.round(tf.sigmoid(z_pres_logits))
    out_dir = str(tmp_path) + "/"
    tag = "_it_7_0"
    # x_reconstrcution_test
    V.reconstruction_test(model, ds, filename=tag, filepath=out_dir, label=True, outputs=o)
    _panels_equal(out_dir + "x_reconstrcution_test" + tag + ".png", _recon_ref(img, npo[0], pres, npo[7], npo[16]))
    # x_reconstrcution_bbox: input | input with boxes | x_recon with boxes
    white = np.ones((1, 4), np.float32)
    V.reconstruction_bbox(model, ds, filename=tag, filepath=out_dir, label=True, outputs=o)
    rows = np.concatenate([_strip(img[..., :3]), _strip(er.draw_bounding_boxes(img[..., :3], npo[17], white, pres)),
                           _strip(er.draw_bounding_boxes(npo[0], npo[17], white, pres))], axis=0)
    _panels_equal(out_dir + "x_reconstrcution_bbox" + tag + ".png", [rows])
    # glimpses
    V.glimpses_reconstruction_test(model, ds, filename=tag, filepath=out_dir, label=True, outputs=o)
    S = cfg.object_size
    panels = [_cells(npo[13]), _cells(npo[14]), _grey3(_cells(npo[15]))]
    assert panels[0].shape == (16 * S, n * S, 3)
    _panels_equal(out_dir + "glimpses" + tag + ".png", panels)
    if name == "lg_spair":
        V.x_hat_reconstruction_test(model, ds, filename=tag, filepath=out_dir, label=True, outputs=o)
        _panels_equal(out_dir + "x_hat_reconstrcution_test" + tag + ".png",
                      [np.concatenate([_strip(npo[21]), _strip(img[..., 3:])], axis=0)])
    # train_recon_it_<step>: from a train step's own outputs (its sampled z_pres), the full batch sliced to n
    opt = spair_trainer.ClipnormAdam(1e-4)
    res, _ = spair_trainer.train_step(model, images, opt, 0, cfg)
    r = [res[i].detach().float().cpu().numpy()[:n] for i in (0, 7, 10, 16)]
    V.train_reconstruction(images, res, step=3, filepath=out_dir)
    _panels_equal(out_dir + "train_recon_it_3.png", _recon_ref(img, r[0], r[2], r[1], r[3]))
    # the sizes of the reference's canvases: (cells + 2) * H x n * W per panel
    from split_vae_amd.visualizer import load_png
    assert load_png(out_dir + "train_recon_it_3.png").shape == (18 * 48, 3 * n * 48 + 8, 3)


def _run_main(argv, tmp_path, monkeypatch, capsys):
    from split_vae_amd import spair_main
    monkeypatch.chdir(tmp_path)
    hist = spair_main.main(argv)
    return hist, capsys.readouterr().out


def test_cli_viz_writes_figures_and_count_accuracy(lib_built, tmp_path, monkeypatch, capsys):
    argv = ["--synthetic", "--batch_size", "12", "--training_steps", "4", "--log_every", "2", "--model", "lg_spair", "--latent_size", "64",
            "--bg_latent_size", "4", "--local_latent_size", "4", "--patch_size", "8", "-split_z_l", "-concat_z_what", "-dense_local",
            "-dense_bg"]
    from split_vae_amd.spair_trainer import TEST_METRIC_NAMES
    (tmp_path / "viz").mkdir()
    hist, out = _run_main(argv + ["-viz"], tmp_path / "viz", monkeypatch, capsys)
    assert "Count accuracy0: " in out
    assert [h["step"] for h in hist] == [0, 2, 4]
    for h in hist:
        assert 0.0 <= h["count_acc0"] <= 1.0
        assert set(h["test0"]) == {nm + "0" for nm in TEST_METRIC_NAMES}
    runs = os.listdir(tmp_path / "viz" / "output")
    assert len(runs) == 1
    files = set(os.listdir(tmp_path / "viz" / "output" / runs[0]))
    want = set()
    for s in (0, 2, 4):
        want |= {"train_recon_it_%d.png" % s, "x_reconstrcution_test_it_%d_0.png" % s, "x_reconstrcution_bbox_it_%d_0.png" % s,
                 "glimpses_it_%d_0.png" % s, "x_hat_reconstrcution_test_it_%d_0.png" % s}
    assert files == want
    # without -viz: nothing under output/
    (tmp_path / "plain").mkdir()
    hist, out = _run_main(["--synthetic", "--batch_size", "8", "--training_steps", "2", "--log_every", "2"], tmp_path / "plain",
                          monkeypatch, capsys)
    assert "Count accuracy0: " in out and 0.0 <= hist[-1]["count_acc0"] <= 1.0
    assert not os.path.exists(tmp_path / "plain" / "output")


def test_cli_unlabelled_count_accuracy_is_zero(lib_built, tmp_path, monkeypatch, capsys):
    hist, out = _run_main(["--synthetic", "--batch_size", "8", "--training_steps", "0", "--log_every", "1", "-no_label"], tmp_path,
                          monkeypatch, capsys)
    assert "Count accuracy0: 0.0" in out and hist[0]["count_acc0"] == 0.0
    assert "MAE test0" not in hist[0]["test0"]
