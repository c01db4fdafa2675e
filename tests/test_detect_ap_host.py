"""CPU: the detection average precision without a device -- hand-worked cases, the host mirrors
(sv_detect_match_host, sv_sprite_extents_host, sv_multibird_gt_boxes_host: the per-image functions the kernels run) against the
NumPy twin bit for bit, the ground-truth boxes against rendered canvases, the twin's mutants, and the CLI surface."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detect_ap_ref as ref        # noqa: E402
import multibird_ref               # noqa: E402

U = 1.0 / 64.0


def _case(gt, dets, cells=None):
    """one image: gt boxes and (box, logit) detections in 1/64 units; unused cells get logit -1"""
    cells = cells or max(len(dets), 1)
    bbox, logits = np.zeros((1, cells, 4), np.float32), np.full((1, cells), -1.0, np.float32)
    g = np.zeros((1, 5, 4), np.float32)
    g[0, :len(gt)] = np.asarray(gt, np.float64).reshape(-1, 4) * U
    for j, (box, lg) in enumerate(dets):
        bbox[0, j], logits[0, j] = np.asarray(box, np.float64) * U, lg
    return dict(bbox=bbox, logits=logits, gt=g, n_gt=np.array([len(gt)], np.int32))


def _host(case, image_offset=0):
    from split_vae_amd import ops
    keys, tps = ops.detect_match_host(case["bbox"], case["logits"], case["gt"], case["n_gt"], image_offset=image_offset)
    n = case["logits"].size
    return keys[image_offset * case["logits"].shape[1]:][:n], tps[image_offset * case["logits"].shape[1]:][:n]


def _both(case):
    """host mirror == twin on the case; -> (keys, tps)"""
    keys, tps = _host(case)
    rk, rt = ref.match(case["bbox"], case["logits"], case["gt"], case["n_gt"])
    assert np.array_equal(keys, rk) and np.array_equal(tps, rt)
    return keys, tps


# ---------------------------------------------------------------------------------------------- hand-worked cases
def test_two_boxes_three_detections_by_hand(lib_built):
    """Boxes A = (0,0,8,8), B = (0,16,8,24).  Detections in confidence order: a miss (logit 3), A exactly (logit 2), the left half of B
    (logit 1, IoU exactly 0.5).  IoU 0.5: FP, TP, TP -> p = 0, 1/2, 2/3; interpolated AP = (2/3 + 2/3) / 2 = 2/3, uninterpolated
    (1/2 + 2/3) / 2 = 7/12.  IoU 0.6: FP, TP, FP -> p = 0, 1/2, 1/3; AP = AP' = (1/2) / 2 = 1/4."""
    case = _case([(0, 0, 8, 8), (0, 16, 8, 24)], [((0, 0, 8, 8), 2.0), ((20, 20, 28, 28), 3.0), ((0, 16, 8, 20), 1.0)])
    keys, tps = _both(case)
    assert tps.tolist() == [0x1FF, 0, 0x01F]
    assert np.argsort(keys).tolist() == [1, 0, 2]
    res = ref.evaluate(**case)
    assert res["M"] == 3 and res["G"] == 2 and res["tp"].tolist() == [2] * 5 + [1] * 4
    assert res["ap"][4] == pytest.approx(2 / 3, rel=1e-15) and res["ap_un"][4] == pytest.approx(7 / 12, rel=1e-15)
    assert res["ap"][5] == pytest.approx(1 / 4, rel=1e-15) and res["ap_un"][5] == pytest.approx(1 / 4, rel=1e-15)
    assert res["precision50"] == pytest.approx(2 / 3) and res["recall50"] == 1.0
    assert res["mAP"] == pytest.approx((5 * (2 / 3) + 4 * (1 / 4)) / 9, rel=1e-15)
    # the uninterpolated sum reported as the interpolated one is another number
    assert ref.evaluate(**case, mutant="no_interpolation")["ap"][4] == pytest.approx(7 / 12, rel=1e-15)


def test_no_boxes_no_detections_all_false_positives(lib_built):
    # G = 0: detections exist, nothing to match
    case = _case([], [((0, 0, 8, 8), 1.0), ((0, 0, 4, 4), 2.0)])
    _, tps = _both(case)
    res = ref.evaluate(**case)
    assert tps.tolist() == [0, 0] and res["M"] == 2 and res["G"] == 0 and not res["ap"].any() and not res["ap_un"].any()
    assert res["precision50"] == 0.0 and res["recall50"] == 0.0
    # M = 0: no logit above 0 (0.0, -0.0 and NaN are no detections)
    case = _case([(0, 0, 8, 8)], [((0, 0, 8, 8), 0.0), ((0, 0, 8, 8), -0.0), ((0, 0, 8, 8), np.nan), ((0, 0, 8, 8), -3.0)])
    keys, tps = _both(case)
    res = ref.evaluate(**case)
    assert (keys >> np.uint64(32)).tolist() == [ref.NONDET] * 4 and (keys & np.uint64(0xFFFFFFFF)).tolist() == [0, 1, 2, 3]
    assert not tps.any() and res["M"] == 0 and res["G"] == 1 and not res["ap"].any() and res["precision50"] == 0.0
    # every detection a false positive: disjoint, touching an edge, inverted, zero area, a non-finite coordinate
    case = _case([(0, 0, 8, 8)], [((20, 20, 28, 28), 5.0), ((8, 0, 16, 8), 4.0), ((8, 8, 0, 0), 3.0), ((0, 0, 0, 8), 2.0),
                                  ((0, 0, np.inf, 8), 1.0)])
    _, tps = _both(case)
    res = ref.evaluate(**case)
    assert not tps.any() and res["M"] == 5 and res["G"] == 1 and not res["ap"].any() and res["tp"].tolist() == [0] * 9


def test_duplicate_and_second_best_by_hand(lib_built):
    # two identical detections of one box: the lower id takes it, the second is a false positive at every threshold
    case = _case([(0, 0, 8, 8)], [((0, 0, 8, 8), 2.0), ((0, 0, 8, 8), 2.0)])
    _, tps = _both(case)
    assert tps.tolist() == [0x1FF, 0]
    assert ref.evaluate(**case)["ap"].tolist() == [1.0] * 9
    # boxes A = (0,0,8,8), B = (0,4,8,12).  d0 = A exactly takes A.  d1 = (0,1,8,9): IoU 56/72 = 0.78 with A (taken), 40/88 = 0.45 with
    # B: it takes B up to IoU 0.4 and is a false positive from 0.5 on (A would have passed up to 0.7)
    case = _case([(0, 0, 8, 8), (0, 4, 8, 12)], [((0, 0, 8, 8), 3.0), ((0, 1, 8, 9), 2.0)])
    _, tps = _both(case)
    assert tps.tolist() == [0x1FF, 0x00F]


def test_threshold_ties_are_inclusive(lib_built):
    """a 10 x t detection nested in a 10 x 10 box has IoU exactly t / 10: it passes thresholds 1 .. t"""
    for t in range(1, 10):
        _, tps = _both(_case([(0, 0, 10, 10)], [((0, 0, 10, t), 1.0)]))
        assert tps.tolist() == [(1 << t) - 1], t
    inter, union, iou = ref.iou_terms(np.array([0, 0, 2, 2]) * U, np.array([0, 0, 2, 10]) * U)
    assert inter == np.float32(4 / 4096) and union == np.float32(20 / 4096) and ref.passes(inter, union, 2) and not ref.passes(inter, union, 3)


# ---------------------------------------------------------------------------------------------- host mirror against the twin
@pytest.mark.parametrize("cells", [1, 16, 17, 64])
def test_match_host_equals_twin_on_the_lattice(lib_built, cells):
    case = ref.lattice_case(cells)
    keys, tps = _both(case)
    assert set(case["n_gt"].tolist()) == set(range(6))
    if cells >= 16:
        assert tps.any() and (tps == 0).any() and ((keys >> np.uint64(32)) == ref.NONDET).any()
        # image 0: nine detections with IoU == t / 10 exactly compete for one box in the order t = 1 .. 9: at threshold t the first
        # that passes is detection t, so each owns exactly its own tie
        assert tps[:9].tolist() == [1 << (t - 1) for t in range(1, 10)]
    # a non-zero image offset moves the ids and nothing else
    k2, t2 = _host(case, image_offset=3)
    assert np.array_equal(t2, tps) and np.array_equal(k2 - keys, np.full(keys.shape, 3 * cells, np.uint64))


@pytest.mark.parametrize("cells", [1, 16, 17, 64])
def test_match_host_equals_twin_on_random_boxes(lib_built, cells):
    case, redraws = ref.random_case(cells)
    assert redraws < len(case["n_gt"]) / 10          # the generator cannot quietly empty the set
    keys, tps = _both(case)
    if cells >= 16:
        assert tps.any() and len(set(tps.tolist())) > 4


def test_match_host_rejects_bad_arguments(lib_built):
    from split_vae_amd import _lib
    lib = _lib.load()
    a = np.zeros(64 * 4 * 2, np.float32)
    n = np.zeros(2, np.int32)
    k, t = np.zeros(130, np.uint64), np.zeros(130, np.uint16)
    p = lambda x: x.ctypes.data                      # noqa: E731
    f = lib.sv_detect_match_host
    assert f(p(a), 64, p(a), 16, 16, p(a), p(n), 2, 0, p(k), p(t)) == 0
    assert f(None, 64, p(a), 16, 16, p(a), p(n), 2, 0, p(k), p(t)) == _lib.STATUS_BADARG
    assert f(p(a), 63, p(a), 16, 16, p(a), p(n), 2, 0, p(k), p(t)) == _lib.STATUS_BADARG       # pitch below the row
    assert f(p(a), 64, p(a), 15, 16, p(a), p(n), 2, 0, p(k), p(t)) == _lib.STATUS_BADARG
    assert f(p(a), 64, p(a), 16, 16, p(a), p(n), 0, 0, p(k), p(t)) == _lib.STATUS_BADARG
    assert f(p(a), 64, p(a), 16, 16, p(a), p(n), 2, -1, p(k), p(t)) == _lib.STATUS_BADARG
    assert f(p(a), 260, p(a), 65, 65, p(a), p(n), 1, 0, p(k), p(t)) == _lib.STATUS_UNSUPPORTED
    assert k[:32].all() and not k[32:].any() and not t.any()      # the one valid call wrote its 32 records; the refused ones nothing
    nb = _lib.C.c_int64()
    assert lib.sv_detect_ap_workspace_bytes(0, _lib.C.byref(nb)) == _lib.STATUS_UNSUPPORTED
    assert lib.sv_detect_ap_workspace_bytes((1 << 20) + 1, _lib.C.byref(nb)) == _lib.STATUS_UNSUPPORTED
    assert lib.sv_detect_ap_workspace_bytes(1 << 20, _lib.C.byref(nb)) == 0 and nb.value >= (1 << 20) * 20
    assert lib.sv_detect_ap_finish(None, None, 1, None, 1, None, 0, None, None) == _lib.STATUS_BADARG
    assert lib.sv_sprite_extents(None, 1, None, None) == _lib.STATUS_BADARG
    assert lib.sv_multibird_gt_boxes(None, None, 1, None, None, 1, None) == _lib.STATUS_BADARG
    assert lib.sv_detect_ap_chunk_records() == 4096


# ---------------------------------------------------------------------------------------------- extents and ground truth
def _hand_bank():
    from split_vae_amd import multibird
    hand = np.zeros((7, 14, 14, 3), np.uint8)
    for i, (r, c) in enumerate([(0, 0), (0, 13), (13, 0), (13, 13)]):
        hand[1 + i, r, c, i % 3] = 1                 # one pixel in each corner, one channel lit
    hand[5] = 200                                    # full
    hand[6, 3:9, 5:6, 2] = 7                         # a one-column bar
    return np.concatenate([hand, multibird.procedural_bank(40, seed=3, test=True)])


def test_sprite_extents_host_equals_twin(lib_built):
    from split_vae_amd import ops
    bank = _hand_bank()
    got = ops.sprite_extents_host(bank)
    assert np.array_equal(got, ref.sprite_extents(bank))
    assert got[:7].tolist() == [[-1] * 4, [0, 0, 0, 0], [0, 13, 0, 13], [13, 0, 13, 0], [13, 13, 13, 13], [0, 0, 13, 13], [3, 5, 8, 5]]
    assert (got[7:, 0] >= 0).all() and (got[7:, 2] > got[7:, 0]).all()


def test_gt_boxes_host_equals_twin_and_counts_real_boxes_only(lib_built):
    from split_vae_amd import multibird, ops
    bank = _hand_bank()
    ext = ops.sprite_extents_host(bank)
    lay = multibird.layouts_host(multibird.BACKGROUNDS["solid_fixed"], len(bank), 5, multibird.SPLIT_TEST, range(300))
    lay["sprite"][7, :] = len(bank) + 2              # pinned ids outside the bank
    boxes, n_gt = ops.multibird_gt_boxes_host(lay, ext)
    rb, rn = ref.gt_boxes(lay, ext)
    assert np.array_equal(boxes, rb) and np.array_equal(n_gt, rn)
    # sprite 0 is empty: G counted from `count` is another number
    assert int(n_gt.sum()) < int(lay["count"].sum()) and n_gt[7] == 0 and set(n_gt.tolist()) == set(range(6))
    assert not boxes[n_gt == 0].any()
    # a wrong + 1 in the extent moves the far edges
    mb, _ = ref.gt_boxes(lay, ext, mutant="extent_plus_one")
    assert not np.array_equal(boxes, mb)
    k = int(np.nonzero(n_gt == lay["count"])[0][-1])
    L = lay[k]
    e = ext[L["sprite"][0]]
    assert boxes[k, 0].tolist() == [np.float32(L["row"][0] + e[0]) / np.float32(48), np.float32(L["col"][0] + e[1]) / np.float32(48),
                                    np.float32(L["row"][0] + e[2] + 1) / np.float32(48), np.float32(L["col"][0] + e[3] + 1) / np.float32(48)]


@pytest.mark.parametrize("seed,split", [(0, 1), (11, 2)])
def test_gt_boxes_enclose_the_rendered_sprites(lib_built, seed, split):
    """On a solid background, for every sprite no other sprite's 14 x 14 footprint touches: (i) every pixel of its footprint that
    differs from the background lies inside its box, (ii) each of the box's four border rows / columns holds such a pixel."""
    from split_vae_amd import multibird, ops
    bank = multibird.procedural_bank(64, seed=seed, test=True)
    ext = ops.sprite_extents_host(bank)
    lay = multibird.layouts_host(multibird.BACKGROUNDS["solid_fixed"], len(bank), seed, split, range(40))
    boxes, n_gt = ops.multibird_gt_boxes_host(lay, ext)
    assert np.array_equal(n_gt, lay["count"])        # the procedural bank has no empty sprite
    checked = 0
    for i, L in enumerate(lay):
        canvas = multibird_ref.create_sample(L, bank, "solid_fixed")
        bgc = np.asarray(multibird_ref.TRAIN_COLORS[int(L["colour"][0])], np.float32) / np.float32(255.)
        for k in range(int(L["count"])):
            r, c = int(L["row"][k]), int(L["col"][k])
            if any(abs(r - int(L["row"][j])) < 14 and abs(c - int(L["col"][j])) < 14 for j in range(int(L["count"])) if j != k):
                continue
            diff = (canvas[r:r + 14, c:c + 14] != bgc).any(axis=-1)
            y0, x0, y1, x1 = (int(v) for v in np.rint(boxes[i, k].astype(np.float64) * 48))
            inside = np.zeros((14, 14), bool)
            inside[y0 - r:y1 - r, x0 - c:x1 - c] = True
            assert not (diff & ~inside).any()
            assert diff[y0 - r].any() and diff[y1 - 1 - r].any() and diff[:, x0 - c].any() and diff[:, x1 - 1 - c].any()
            checked += 1
    assert checked >= 20


# ---------------------------------------------------------------------------------------------- mutants
@pytest.mark.parametrize("mutant", ["strict_threshold", "tie_high_box", "reuse_boxes", "ascending", "sigmoid_keys"])
def test_matching_mutants_are_rejected(lib_built, mutant):
    """each mistake in the twin's matching or keys breaks the bit-for-bit comparison on the lattice inputs the twin passes on"""
    case = ref.lattice_case(16)
    keys, tps = _both(case)
    mk, mt = ref.match(case["bbox"], case["logits"], case["gt"], case["n_gt"], mutant=mutant)
    assert not (np.array_equal(keys, mk) and np.array_equal(tps, mt))
    if mutant in ("strict_threshold", "tie_high_box", "reuse_boxes"):
        assert np.array_equal(keys, mk) and not np.array_equal(tps, mt)      # the masks alone give it away


def test_curve_mutants_are_rejected(lib_built):
    case = ref.lattice_case(16)
    keys, tps = _both(case)
    G = int(case["n_gt"].sum())
    good, flat = ref.curve(keys, tps, G), ref.curve(keys, tps, G, mutant="no_interpolation")
    assert np.array_equal(good["ap_un"], flat["ap_un"]) and (good["ap"] > flat["ap"]).any() and (good["ap"] >= flat["ap"]).all()
    more = ref.evaluate(**case, counts=case["n_gt"] + 1, mutant="g_from_count")
    assert more["G"] != G and (more["ap"] < good["ap"]).any()
    # the order matters: ascending keys give another curve from the same masks
    mk, _ = ref.match(case["bbox"], case["logits"], case["gt"], case["n_gt"], mutant="ascending")
    det = (keys >> np.uint64(32)) != ref.NONDET
    assert not np.array_equal(np.argsort(keys[det]), np.argsort(mk[det]))


# ---------------------------------------------------------------------------------------------- surface
def test_parser_flag_and_notes(lib_built, capsys):
    from split_vae_amd import detection, spair_main, spair_trainer
    ap = spair_main.build_parser()
    assert ap.parse_args([]).detection_ap is False and ap.parse_args(["--detection_ap"]).detection_ap is True
    with pytest.raises(SystemExit):
        ap.parse_args(["--detection_ap", "3"])       # a switch: it takes no value
    assert "unrecognized arguments" in capsys.readouterr().err
    assert spair_main.default_config().detection_ap is False
    lines = []
    log = lambda *a: lines.append(" ".join(str(x) for x in a))      # noqa: E731
    cfg = spair_main.default_config()
    assert spair_trainer._detection_state(cfg, [], {}, 0, "cpu", log) is None and not lines           # off: inert
    cfg = spair_main.default_config(detection_ap=True)
    for num in (0, 1):                                               # a test set without boxes: one note, skipped
        assert spair_trainer._detection_state(cfg, [("images", "labels")], {}, num, "cpu", log) is None
    assert lines == [detection.UNAVAILABLE]
    res = dict(mAP=0.5, ap50=0.25, precision50=0.75, recall50=0.125, detections=7, boxes=9)
    assert detection.report_line(res, 1) == ("Detection AP1: mean 0.5000 (IoU 0.1 .. 0.9), AP@0.5 0.2500, precision@0.5 0.7500, "
                                             "recall@0.5 0.1250 (7 detections, 9 boxes)")
    assert detection.history_entries(res, 0)["det_ap0"] == 0.5 and detection.history_entries(res, 0)["det_ap50_0"] == 0.25


def test_labelled_batches_yield_the_same_with_box_attributes(lib_built):
    import torch
    from split_vae_amd import multibird
    x, y = torch.arange(5 * 2 * 2 * 3, dtype=torch.float32).reshape(5, 2, 2, 3), torch.arange(5, dtype=torch.float32)
    plain, boxed = multibird.LabelledBatches(x, y, 2), multibird.LabelledBatches(x, y, 2)
    boxed.boxes, boxed.n_boxes = torch.zeros(5, 5, 4), torch.zeros(5, dtype=torch.int32)
    a, b = list(plain), list(boxed)
    assert len(a) == len(b) == 3 and all(len(p) == 2 and torch.equal(p[0], q[0]) and torch.equal(p[1], q[1]) for p, q in zip(a, b))
    assert not hasattr(plain, "boxes")
