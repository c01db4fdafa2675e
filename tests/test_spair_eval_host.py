"""CPU: the numpy restatements of the SPAIR evaluation kernels (tests/spair_eval_ref.py) on hand-worked cases, the argument checks of
sv_draw_bounding_boxes / sv_spair_count_metrics (refused before any device work), and the -viz switch of spair_main."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spair_eval_ref as er  # noqa: E402

WHITE = np.ones((1, 4), np.float32)


def _outline(H, W, r0, c0, r1, c1):
    """The hand-drawn outline of a box fully inside an H x W image: a boolean mask."""
    m = np.zeros((H, W), bool)
    m[r0, c0:c1 + 1] = m[r1, c0:c1 + 1] = True
    m[r0:r1 + 1, c0] = m[r0:r1 + 1, c1] = True
    return m


def _drawn(out, img):
    return np.any(out != img, axis=-1)[0]


def test_five_by_five_box():
    img = np.zeros((1, 11, 11, 3), np.float32)
    out = er.draw_bounding_boxes(img, [[[0.2, 0.2, 0.6, 0.6]]], WHITE)        # 0.2 * 10 = 2, 0.6 * 10 = 6: rows / cols 2..6
    want = _outline(11, 11, 2, 2, 6, 6)
    assert want.sum() == 16
    assert np.array_equal(_drawn(out, img), want)
    assert np.all(out[0][want] == 1.0)


def test_non_square_image_uses_h_for_rows_and_w_for_columns():
    img = np.zeros((1, 6, 11, 1), np.float32)
    out = er.draw_bounding_boxes(img, [[[0.2, 0.3, 0.8, 0.5]]], WHITE)        # rows 0.2*5 = 1, 0.8*5 = 4; cols 0.3*10 = 3, 5
    assert np.array_equal(_drawn(out, img), _outline(6, 11, 1, 3, 4, 5))


def test_negative_coordinates_truncate_toward_zero():
    img = np.zeros((1, 11, 11, 3), np.float32)
    # ymin * 10 = -0.5 -> 0 (not floor -1): the top edge lies inside the image and is drawn on row 0
    out = er.draw_bounding_boxes(img, [[[-0.05, 0.2, 0.4, 0.6]]], WHITE)
    assert np.array_equal(_drawn(out, img), _outline(11, 11, 0, 2, 4, 6))
    # ymin * 10 = -1.5 -> -1: no top edge, the sides start at the clamped row 0
    out = er.draw_bounding_boxes(img, [[[-0.15, 0.2, 0.4, 0.6]]], WHITE)
    want = np.zeros((11, 11), bool)
    want[4, 2:7] = True
    want[0:5, 2] = want[0:5, 6] = True
    assert np.array_equal(_drawn(out, img), want)
    # xmax * 10 = 12 -> beyond the right edge: no right side, top and bottom run to the last column
    out = er.draw_bounding_boxes(img, [[[0.2, 0.5, 0.6, 1.2]]], WHITE)
    want = np.zeros((11, 11), bool)
    want[2, 5:] = want[6, 5:] = True
    want[2:7, 5] = True
    assert np.array_equal(_drawn(out, img), want)
    assert er.tf_trunc_i64(np.float32(-0.999)) == 0 and er.tf_trunc_i64(np.float32(-1.0)) == -1
    assert er.tf_trunc_i64(np.float32("nan")) == er.INT64_MIN


def test_inverted_and_outside_boxes_are_skipped():
    img = np.full((1, 9, 9, 3), 0.25, np.float32)
    boxes = [[[0.6, 0.2, 0.4, 0.6],            # ymin > ymax
              [0.2, 0.6, 0.4, 0.2],            # xmin > xmax
              [1.2, 0.2, 1.5, 0.6],            # below the image: r0 >= H
              [-0.9, 0.2, -0.2, 0.6],          # above: r1 < 0
              [0.2, 1.3, 0.6, 1.6],            # right of it
              [0.2, -0.8, 0.6, -0.3]]]         # left of it
    out = er.draw_bounding_boxes(img, boxes, WHITE)
    assert np.array_equal(out, img)


def test_gated_off_box_draws_the_origin_dot():
    img = np.zeros((1, 8, 8, 3), np.float32)
    out = er.draw_bounding_boxes(img, [[[0.25, 0.25, 0.75, 0.75]]], WHITE, gate=[[0.0]])
    want = np.zeros((8, 8), bool)
    want[0, 0] = True                          # (0,0,0,0): r0 = r1 = c0 = c1 = 0, all four edges on pixel (0, 0)
    assert np.array_equal(_drawn(out, img), want)
    out = er.draw_bounding_boxes(img, [[[0.25, 0.25, 0.75, 0.75]]], WHITE, gate=[[1.0]])
    assert np.array_equal(_drawn(out, img), _outline(8, 8, 1, 1, 5, 5))       # 0.75 * 7 = 5.25 -> 5


def test_last_box_wins_with_a_three_colour_table():
    colors = np.array([[1, 0, 0, 9], [0, 1, 0, 9], [0, 0, 1, 9]], np.float32)
    img = np.zeros((1, 11, 11, 4), np.float32)
    boxes = [[[0.2, 0.2, 0.6, 0.6],            # colour 0
              [0.2, 0.2, 0.6, 0.6],            # colour 1, the same outline: overwrites box 0
              [0.6, 0.2, 0.8, 0.8],            # colour 2: its top edge (row 6) overlaps box 1's bottom edge
              [0.0, 0.0, 0.2, 0.2]]]           # colour 3 % 3 = 0: crosses box 1 at (2, 2)
    out = er.draw_bounding_boxes(img, boxes, colors)
    assert np.array_equal(out[0, 2, 4], [0, 1, 0, 9])          # box 1's top edge
    assert np.array_equal(out[0, 6, 4], [0, 0, 1, 9])          # box 2 over box 1
    assert np.array_equal(out[0, 2, 2], [1, 0, 0, 9])          # box 3 over box 1 (colour index 0)
    assert np.array_equal(out[0, 0, 1], [1, 0, 0, 9])
    assert np.array_equal(out[0, 4, 2], [0, 1, 0, 9])
    assert np.array_equal(out[0, 5, 5], [0, 0, 0, 0])          # inside every box: untouched
    # only the first C components of a colour are written
    out3 = er.draw_bounding_boxes(np.zeros((1, 11, 11, 3), np.float32), boxes, colors)
    assert np.array_equal(out3[0, 2, 2], [1, 0, 0])


def test_count_of_a_zero_logit_is_zero():
    lg = np.array([[0.0, 0.0, 1e-3, -1e-3, 10.0, -10.0]], np.float32)
    pred, mae, mape, hits = er.count_metrics(lg, [2.0])
    assert pred[0] == 2.0                                      # sigmoid(0) = 0.5 rounds to even: 0
    assert mae == 0.0 and mape == 0.0 and hits == 1


def test_mae_mape_and_matches_by_hand():
    lg = np.full((3, 16), -5.0, np.float32)
    lg[0, :3] = 5.0                 # 3 objects
    lg[1, :1] = 5.0                 # 1 object
    # image 2: none
    pred, mae, mape, hits = er.count_metrics(lg, [3.0, 2.0, 0.0])
    assert pred.tolist() == [3.0, 1.0, 0.0]
    assert mae == pytest.approx(1.0 / 3.0)
    assert mape == pytest.approx(100.0 * (0.0 + 0.5 + 0.0) / 3.0)
    assert hits == 2


def test_mape_with_label_zero_divides_by_epsilon():
    lg = np.full((1, 4), 5.0, np.float32)                      # 4 objects
    _, mae, mape, hits = er.count_metrics(lg, [0.0])
    assert mae == 4.0 and hits == 0
    assert mape == pytest.approx(100.0 * 4.0 / 1e-7, rel=1e-12)


def test_entry_points_refuse_bad_arguments_before_any_device_work(lib_built):
    from split_vae_amd import _lib
    lib = _lib.load()
    bad = _lib.STATUS_BADARG
    p = 256                                    # never dereferenced: every call below is refused by its argument checks
    # images, boxes, gate, colors, out, B, H, W, C, NB, NC, ldc, stream
    assert lib.sv_draw_bounding_boxes(None, p, None, p, p, 1, 8, 8, 3, 1, 1, 4, None) == bad
    assert lib.sv_draw_bounding_boxes(p, None, None, p, p, 1, 8, 8, 3, 1, 1, 4, None) == bad
    assert lib.sv_draw_bounding_boxes(p, p, None, None, p, 1, 8, 8, 3, 1, 1, 4, None) == bad
    assert lib.sv_draw_bounding_boxes(p, p, None, p, None, 1, 8, 8, 3, 1, 1, 4, None) == bad
    for B, H, W, NB, NC in [(0, 8, 8, 1, 1), (1, 0, 8, 1, 1), (1, 8, -1, 1, 1), (1, 8, 8, 0, 1), (1, 8, 8, 1, 0)]:
        assert lib.sv_draw_bounding_boxes(p, p, None, p, p, B, H, W, 3, NB, NC, 4, None) == bad
    for Cc in (0, 2, 5):
        assert lib.sv_draw_bounding_boxes(p, p, None, p, p, 1, 8, 8, Cc, 1, 1, 8, None) == bad
    assert lib.sv_draw_bounding_boxes(p, p, None, p, p, 1, 8, 8, 4, 1, 1, 3, None) == bad      # colour table narrower than C
    # z_pres_logits, ld, labels, pred, metrics, acc, B, ncell, stream
    assert lib.sv_spair_count_metrics(None, 16, p, None, p, None, 1, 16, None) == bad
    assert lib.sv_spair_count_metrics(p, 16, None, None, p, None, 1, 16, None) == bad
    assert lib.sv_spair_count_metrics(p, 16, p, None, None, None, 1, 16, None) == bad
    assert lib.sv_spair_count_metrics(p, 16, p, None, p, None, 0, 16, None) == bad
    assert lib.sv_spair_count_metrics(p, 16, p, None, p, None, 1, 0, None) == bad
    assert lib.sv_spair_count_metrics(p, 15, p, None, p, None, 1, 16, None) == bad           # row pitch below ncell


def test_viz_switch_parses_and_is_off_by_default():
    from split_vae_amd import spair_main
    assert spair_main.build_parser().parse_args(["-viz", "--synthetic"]).viz is True
    assert spair_main.build_parser().parse_args([]).viz is False
    assert spair_main.default_config().viz is False


def test_spair_visualizer_layout_helpers():
    from split_vae_amd import spair_visualizer as sv
    a, b = np.zeros((5, 7, 3), np.float32), np.full((5, 2, 3), 0.5, np.float32)
    c = sv._side_by_side([a, b])
    assert c.shape == (5, 7 + sv.GUTTER + 2, 3) and np.all(c[:, 7:7 + sv.GUTTER] == 1.0)
    x = np.arange(2 * 3 * 4 * 5 * 1, dtype=np.float32).reshape(2, 3, 4, 5, 1)
    cells = sv._cells(x, 2)
    assert cells.shape == (12, 10, 1)
    assert np.array_equal(cells[:, 5:10], x[1].reshape(12, 5, 1))
