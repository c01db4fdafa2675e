"""GPU: the detection average precision kernels (csrc/detect_ap.hip) -- sv_detect_match, sv_sprite_extents and sv_multibird_gt_boxes bit
for bit against their host mirrors (which tests/test_detect_ap_host.py pins against the NumPy twin on the same cases), sv_detect_ap_finish
against the twin's float64 curve, and DetectionAP end to end through test_step and spair_main."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detect_ap_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

CHUNK = 4096
KEY_FILL, TP_FILL = 0x5555555555555555, 0x7777


def _i64(keys):
    return torch.from_numpy(np.asarray(keys, np.uint64).view(np.int64).copy()).cuda()


def _i16(tps):
    return torch.from_numpy(np.asarray(tps, np.uint16).view(np.int16).copy()).cuda()


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _u16(t):
    return t.cpu().numpy().view(np.uint16)


# ---------------------------------------------------------------------------------------------- matching
def _tile(case, B):
    """the case's images repeated up to B images"""
    n = len(case["n_gt"])
    idx = np.arange(B) % n
    return {k: np.ascontiguousarray(v[idx]) for k, v in case.items()}


@pytest.mark.parametrize("cells", [1, 16, 17, 64])
@pytest.mark.parametrize("B,offset,pitched", [(1, 0, False), (3, 2, True), (65, 0, True), (65, 7, False)])
def test_match_equals_host_mirror(lib_built, cells, B, offset, pitched):
    from split_vae_amd import ops
    for case in (ref.lattice_case(cells), ref.random_case(cells)[0]):
        case = _tile(case, B)
        n_rec = (offset + B + 2) * cells
        hk, ht = np.full(n_rec, KEY_FILL, np.uint64), np.full(n_rec, TP_FILL, np.uint16)
        ops.detect_match_host(case["bbox"], case["logits"], case["gt"], case["n_gt"], image_offset=offset, rec_key=hk, rec_tp=ht)
        ldb, ldl = (cells * 4 + 12, cells + 5) if pitched else (cells * 4, cells)
        bb = torch.full((B, ldb), float("nan")).cuda()
        lg = torch.full((B, ldl), 9.0).cuda()                         # what lies between the rows would be a detection
        bb[:, :cells * 4] = torch.from_numpy(case["bbox"].reshape(B, -1)).cuda()
        lg[:, :cells] = torch.from_numpy(case["logits"]).cuda()
        rk = torch.full((n_rec,), KEY_FILL, dtype=torch.int64).cuda()
        rt = torch.full((n_rec,), TP_FILL, dtype=torch.int16).cuda()
        ops.detect_match(bb[:, :cells * 4].view(B, cells, 4), lg[:, :cells], torch.from_numpy(case["gt"]).cuda(),
                         torch.from_numpy(case["n_gt"]).cuda(), rk, rt, image_offset=offset)
        gk, gt = _u64(rk), _u16(rt)
        assert np.array_equal(gk, hk) and np.array_equal(gt, ht)      # the B images' records, and the fill everywhere else
        lo, hi = offset * cells, (offset + B) * cells
        assert (gk[:lo] == KEY_FILL).all() and (gk[hi:] == KEY_FILL).all() and (gt[:lo] == TP_FILL).all() and (gt[hi:] == TP_FILL).all()
        assert (gk[lo:hi] & np.uint64(0xFFFFFFFF)).tolist() == list(range(lo, hi))


def test_match_equals_twin_directly(lib_built):
    """one lattice case against the twin itself, and the twin's mutants rejected by the device's records"""
    from split_vae_amd import ops
    case = ref.lattice_case(16)
    rk, rt = torch.zeros(12 * 16, dtype=torch.int64).cuda(), torch.zeros(12 * 16, dtype=torch.int16).cuda()
    ops.detect_match(*(torch.from_numpy(case[k]).cuda() for k in ("bbox", "logits", "gt", "n_gt")), rk, rt)
    tk, tt = ref.match(case["bbox"], case["logits"], case["gt"], case["n_gt"])
    assert np.array_equal(_u64(rk), tk) and np.array_equal(_u16(rt), tt)
    for mutant in ("strict_threshold", "tie_high_box", "reuse_boxes", "ascending", "sigmoid_keys"):
        mk, mt = ref.match(case["bbox"], case["logits"], case["gt"], case["n_gt"], mutant=mutant)
        assert not (np.array_equal(_u64(rk), mk) and np.array_equal(_u16(rt), mt)), mutant


def test_extents_and_gt_boxes_equal_host_mirror(lib_built):
    from split_vae_amd import detection, multibird, ops
    from test_detect_ap_host import _hand_bank
    bank = _hand_bank()
    ext = ops.sprite_extents(torch.from_numpy(bank).cuda())
    assert np.array_equal(ext.cpu().numpy(), ops.sprite_extents_host(bank))
    for bg, split, seed, n in (("solid_fixed", 1, 5, 300), ("unseen_ckb_rot_6", 2, 0, 1000)):
        lay = ops.multibird_layouts(n, multibird.BACKGROUNDS[bg], len(bank), seed, split)
        lay[7, 11:16] = len(bank) + 2                                 # pinned ids outside the bank
        lay[8, 0] = 9                                                 # a count beyond 5 is clamped
        boxes, n_gt = ops.multibird_gt_boxes(lay, ext)
        hb, hn = ops.multibird_gt_boxes_host(multibird.layouts_to_numpy(lay), ext.cpu().numpy())
        assert np.array_equal(boxes.cpu().numpy(), hb) and np.array_equal(n_gt.cpu().numpy(), hn)
        assert hn[7] == 0 and set(hn.tolist()) == set(range(6))
    b2, n2 = detection.ground_truth(torch.from_numpy(bank).cuda(), multibird.BACKGROUNDS["solid_fixed"], len(bank), 64, 5, 1)
    h2 = ops.multibird_gt_boxes_host(multibird.layouts_host(multibird.BACKGROUNDS["solid_fixed"], len(bank), 5, 1, range(64)), ext.cpu().numpy())
    assert np.array_equal(b2.cpu().numpy(), h2[0]) and np.array_equal(n2.cpu().numpy(), h2[1])


# ---------------------------------------------------------------------------------------------- the curve
def _finish(keys, tps, G, check_twice=True):
    """sv_detect_ap_finish on a NaN-filled workspace -> (ap, ap_un, tp, M, G); two calls give the same bits"""
    from split_vae_amd import ops
    n = len(keys)
    rk, rt = _i64(keys), _i16(tps)
    images = max(1, (G + 4) // 5)
    n_gt = np.full(images, 5, np.int32)
    n_gt[-1] = G - 5 * (images - 1)
    n_gt = torch.from_numpy(n_gt).cuda()
    nbytes = ops.detect_ap_workspace_bytes(n)
    assert nbytes % 8 == 0
    outs = []
    for _ in range(2 if check_twice else 1):
        ws = torch.full((nbytes // 8,), float("nan"), dtype=torch.float64).cuda().view(torch.uint8)
        out = torch.full((ops.DETECT_AP_OUT,), float("nan"), dtype=torch.float64).cuda()
        ops.detect_ap_finish(rk, rt, n_gt, workspace=ws, out=out)
        outs.append(out.cpu().numpy().copy())
    assert np.array_equal(_u64(rk), np.asarray(keys, np.uint64)) and np.array_equal(_u16(rt), np.asarray(tps, np.uint16))   # inputs untouched
    if check_twice:
        assert outs[0].tobytes() == outs[1].tobytes()
    o = outs[0]
    ints = o.view(np.int64)
    return o[:9], o[9:18], ints[18:27], int(ints[27]), int(ints[28])


def _check_finish(keys, tps, G, mutants=False):
    ap, ap_un, tp, M, Gd = _finish(keys, tps, G)
    want = ref.curve(keys, tps, G)
    assert M == want["M"] and Gd == G and tp.tolist() == want["tp"].tolist()
    tol = len(keys) * 2.0 ** -52                     # the fp64 summation bound: both sides divide the same integers
    for t in range(9):
        print("n %d t %d AP %.17g twin %.17g AP' %.17g twin %.17g" % (len(keys), t + 1, ap[t], want["ap"][t], ap_un[t], want["ap_un"][t]))
        assert abs(ap[t] - want["ap"][t]) <= tol * abs(want["ap"][t])
        assert abs(ap_un[t] - want["ap_un"][t]) <= tol * abs(want["ap_un"][t])
    if mutants:
        flat = ref.curve(keys, tps, G, mutant="no_interpolation")
        assert any(abs(ap[t] - flat["ap"][t]) > tol * abs(flat["ap"][t]) for t in range(9))
    return want


@pytest.mark.parametrize("n", [1, 2, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 7, 5 * CHUNK + 1, 16000])
def test_finish_equals_twin_across_chunk_boundaries(lib_built, n):
    from split_vae_amd import ops
    assert ops.detect_ap_chunk_records() == CHUNK
    keys, tps, G = ref.random_records(n, seed=1)
    want = _check_finish(keys, tps, G, mutants=n >= CHUNK)
    if n >= CHUNK:
        assert 0 < want["M"] < n and 0 < want["ap"][4] < 1


@pytest.mark.parametrize("kind", ["all_tp", "all_fp", "sorted", "reversed"])
@pytest.mark.parametrize("n", [CHUNK + 1, 3 * CHUNK + 7])
def test_finish_on_structured_records(lib_built, kind, n):
    keys, tps, G = ref.random_records(n, seed=2, kind=kind)
    want = _check_finish(keys, tps, G)
    assert want["M"] == n
    if kind == "all_tp":
        assert want["tp"].tolist() == [n] * 9
    if kind == "all_fp":
        assert not want["ap"].any()


def test_finish_degenerate_sets(lib_built):
    # no detection at all; detections but no boxes; one true positive alone
    keys = np.array([(ref.NONDET << 32) | i for i in range(40)], np.uint64)
    ap, ap_un, tp, M, G = _finish(keys, np.zeros(40, np.uint16), 3)
    assert M == 0 and G == 3 and not ap.any() and not ap_un.any() and not tp.any()
    keys, tps, _ = ref.random_records(100, seed=3, kind="all_tp")
    ap, ap_un, tp, M, G = _finish(keys, tps, 0)
    assert M == 100 and G == 0 and not ap.any() and not ap_un.any() and tp.tolist() == [100] * 9
    ap, ap_un, tp, M, G = _finish(np.array([ref.record_key(2.0, 0)], np.uint64), np.array([0x1FF], np.uint16), 1)
    assert ap.tolist() == [1.0] * 9 and ap_un.tolist() == [1.0] * 9 and (M, G) == (1, 1)


def test_finish_at_the_largest_size(lib_built):
    n = 1 << 20
    keys, tps, G = ref.random_records(n, seed=4)
    ap, ap_un, tp, M, Gd = _finish(keys, tps, G, check_twice=False)
    want = ref.curve(keys, tps, G)
    assert M == want["M"] and Gd == G and tp.tolist() == want["tp"].tolist()
    tol = n * 2.0 ** -52
    assert (np.abs(ap - want["ap"]) <= tol * np.abs(want["ap"])).all() and (np.abs(ap_un - want["ap_un"]) <= tol * np.abs(want["ap_un"])).all()


def test_by_hand_through_the_object_and_torch_ops(lib_built):
    """the hand-worked image of the host tests (AP@0.5 = 2/3, AP'@0.5 = 7/12, AP@0.6 = 1/4) through DetectionAP and the torch ops"""
    import split_vae_amd.torch_ops  # noqa: F401
    from split_vae_amd import detection
    from test_detect_ap_host import _case
    case = _case([(0, 0, 8, 8), (0, 16, 8, 24)], [((0, 0, 8, 8), 2.0), ((20, 20, 28, 28), 3.0), ((0, 16, 8, 20), 1.0)])
    dev = {k: torch.from_numpy(v).cuda() for k, v in case.items()}
    det = detection.DetectionAP("cuda", 4, 3)
    assert det.result() is None
    for _ in range(2):                                               # reset_states gives the same answer again
        det.update(dev["bbox"], dev["logits"], dev["gt"], dev["n_gt"])
        res = det.result()
        assert res["detections"] == 3 and res["boxes"] == 2 and res["images"] == 1 and res["tp"] == [2] * 5 + [1] * 4
        assert res["ap"][4] == pytest.approx(2 / 3, rel=1e-15) and res["ap_uninterpolated"][4] == pytest.approx(7 / 12, rel=1e-15)
        assert res["ap"][5] == pytest.approx(1 / 4, rel=1e-15) and res["precision50"] == pytest.approx(2 / 3) and res["recall50"] == 1.0
        det.reset_states()
    with pytest.raises(ValueError):
        det.update(dev["bbox"].repeat(5, 1, 1), dev["logits"].repeat(5, 1), dev["gt"].repeat(5, 1, 1), dev["n_gt"].repeat(5))
    rk, rt = torch.zeros(3, dtype=torch.int64).cuda(), torch.zeros(3, dtype=torch.int16).cuda()
    torch.ops.split_vae.detect_match(dev["bbox"], dev["logits"], dev["gt"], dev["n_gt"], rk, rt)
    out = torch.ops.split_vae.detect_ap_finish(rk, rt, dev["n_gt"])
    assert out[4].item() == res["ap"][4] and out.view(torch.int64)[27:].tolist() == [3, 2]
    with pytest.raises(NotImplementedError):
        torch.ops.split_vae.detect_match(*(torch.from_numpy(case[k]) for k in ("bbox", "logits", "gt", "n_gt")), rk.cpu(), rt.cpu())
    with pytest.raises(NotImplementedError):
        torch.ops.split_vae.detect_ap_finish(rk.cpu(), rt.cpu(), dev["n_gt"].cpu())


# ---------------------------------------------------------------------------------------------- end to end
CONFIGS = {
    "spair": dict(model="spair"),
    "lg_spair": dict(model="lg_spair", latent_size=64, bg_latent_size=4, local_latent_size=4, patch_size=8, z_bg_beta=10.0,
                     split_z_l=True, concat_z_what=True, dense_local=True, dense_bg=True),
}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_detection_ap_through_test_step(lib_built, name, monkeypatch):
    """64 kernel-rendered canvases through the labelled test_step, native and op by op: the records equal the twin's on the pass's own
    obj_bbox_mask and logits copied to the host, and the report equals the twin's curve."""
    from oracle import spair_model_ref as R
    from split_vae_amd import detection, multibird, spair, spair_trainer
    from split_vae_amd.utils import dotdict
    cfg = dotdict(R.default_config(**CONFIGS[name]))
    model = spair.get_model(cfg)
    model.set_weights({k: v.numpy() for k, v in R.init_params(cfg, seed=2).items()})
    _, tests, _, _ = multibird.get_cub_dataset("cub_solid_fixed", batch_size=32, seed=3, n_test=64)
    ds = tests[0]
    assert tuple(ds.boxes.shape) == (64, 5, 4) and ds.n_boxes.dtype == torch.int32 and ds.n_boxes.tolist() == [int(v) for v in ds.y.tolist()]

    class Recording(detection.DetectionAP):
        def update(self, bbox, logits, gt_boxes, n_gt):
            self.fed.append(tuple(t.detach().reshape(s).cpu().numpy().copy() for t, s in
                                  ((bbox, (-1, 16, 4)), (logits, (-1, 16)), (gt_boxes, (-1, 5, 4)), (n_gt, (-1,)))))
            super().update(bbox, logits, gt_boxes, n_gt)

    for autograd in (False, True):
        if autograd:
            monkeypatch.setenv("SV_SPAIR_AUTOGRAD", "1")
        det = Recording("cuda", 64, 16)
        det.fed = []
        seen = 0
        for b, (x, y) in enumerate(ds):                              # two batches of 32
            images = torch.cat([x, x.flip(1)], dim=-1) if cfg.model == "lg_spair" else x
            noise = {k: v.float().cuda() for k, v in R.draw_noise(cfg, x.shape[0], seed=50 + b).items()}
            B = x.shape[0]
            spair_trainer.test_step(model, images, cfg, labels=y, noise=noise,
                                    detection=(det, ds.boxes[seen:seen + B], ds.n_boxes[seen:seen + B]))
            seen += B
        assert seen == det.seen == 64
        bbox, logits, gt, n_gt = (np.concatenate([f[i] for f in det.fed]) for i in range(4))
        assert np.array_equal(gt, ds.boxes.cpu().numpy()) and np.array_equal(n_gt, ds.n_boxes.cpu().numpy())
        tk, tt = ref.match(bbox, logits, gt, n_gt)
        assert np.array_equal(_u64(det.rec_key), tk) and np.array_equal(_u16(det.rec_tp), tt)
        res, want = det.result(), ref.evaluate(bbox, logits, gt, n_gt)
        assert res["detections"] == want["M"] and res["boxes"] == want["G"] == int(n_gt.sum()) and res["tp"] == want["tp"].tolist()
        assert res["detections"] > 0                                  # an untrained model still switches cells on
        tol = 1024 * 2.0 ** -52
        assert all(abs(a - w) <= tol * abs(w) for a, w in zip(res["ap"] + res["ap_uninterpolated"], list(want["ap"]) + list(want["ap_un"])))
        assert res["mAP"] == pytest.approx(want["mAP"], rel=1e-12, abs=0) and res["recall50"] == pytest.approx(want["recall50"])


def test_cli_prints_the_report_only_with_the_flag(lib_built, tmp_path, monkeypatch, capsys):
    from split_vae_amd import detection, spair_main
    monkeypatch.chdir(tmp_path)
    argv = ["--dataset", "cub_solid_fixed", "--training_steps", "0", "--log_every", "1", "--data_dir", str(tmp_path / "none")]
    hist = spair_main.main(argv + ["--detection_ap"])
    out = capsys.readouterr().out
    for k in ("0", "1"):
        line = [l for l in out.splitlines() if l.startswith("Detection AP" + k + ": mean ")]
        assert len(line) == 1 and "(IoU 0.1 .. 0.9), AP@0.5 " in line[0] and line[0].endswith(" boxes)")
        assert 0.0 <= hist[0]["det_ap" + k] <= 1.0 and 0.0 <= hist[0]["det_ap50_" + k] <= 1.0 and hist[0]["det_boxes" + k] > 1000
        assert out.index("Count accuracy" + k) < out.index("Detection AP" + k)
    plain = spair_main.main(argv)
    out = capsys.readouterr().out
    assert "Detection AP" not in out and detection.UNAVAILABLE not in out and "Count accuracy1" in out
    assert not any(k.startswith("det_") for k in plain[0]) and set(plain[0]) == {k for k in hist[0] if not k.startswith("det_")}
    spair_main.main(["--synthetic", "--batch_size", "8", "--training_steps", "0", "--log_every", "1", "--detection_ap"])
    out = capsys.readouterr().out
    assert out.count(detection.UNAVAILABLE) == 1 and "Detection AP0" not in out and "Count accuracy0" in out
