"""CPU: the Multi-Bird layout draws on the host (sv_multibird_layout_host), the NumPy restatement of create_sample
(tests/multibird_ref.py) against hand-written rules, the procedural sprite bank, the tf.train.Example codec and the TFRecord
round trip of the dataset.  No device work."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multibird_ref as mr  # noqa: E402

N_SPRITES = 256


@pytest.fixture(scope="module")
def mb(lib_built):
    from split_vae_amd import multibird
    return multibird


def _pairs_ok(L):
    for a in range(L["count"]):
        for b in range(a):
            ix = max(0, 14 - abs(int(L["row"][a]) - int(L["row"][b])))
            iy = max(0, 14 - abs(int(L["col"][a]) - int(L["col"][b])))
            if ix * iy >= 30:
                return False
    return True


def test_layouts_of_the_whole_dataset(mb):
    """All 102 000 canvases of cub_ckb_rot_6 at seed 0 (100 000 train + 2 x 1 000 test): the rules of spair/data.py:59-135,166 and
    the 4096-try cap, which must not bind."""
    sets = [(mb.SPLIT_TRAIN, "ckb_rot_6", mb.N_TRAIN), (mb.SPLIT_TEST, "ckb_rot_6", mb.N_TEST),
            (mb.SPLIT_TEST_UNSEEN, "unseen_ckb_rot_6", mb.N_TEST)]
    counts, worst = [], 0
    for split, bg, n in sets:
        L = mb.layouts_host(mb.BACKGROUNDS[bg], N_SPRITES, 0, split, np.arange(n))
        counts.append(L["count"])
        assert L["count"].min() >= 0 and L["count"].max() <= 5
        placed = np.arange(5)[None, :] < L["count"][:, None]
        for f, hi in (("row", 33), ("col", 33), ("sprite", N_SPRITES - 1)):
            assert (L[f][placed] >= 0).all() and (L[f][placed] <= hi).all() and (L[f][~placed] == -1).all()
        assert all(_pairs_ok(r) for r in L[L["count"] >= 2])
        assert (L["max_tries"] < 4096).all()                 # the cap never bound: no count was reduced
        worst = max(worst, int(L["max_tries"].max()))
        ncol = len(mb.COLOURS[bg])
        assert (L["colour"] >= 0).all() and (L["colour"] < ncol).all() and (L["colour"][:, 0] != L["colour"][:, 1]).all()
        assert len(set(map(tuple, L["colour"]))) == ncol * (ncol - 1)          # every ordered pair occurs
        h = np.float32(np.pi / 2)
        assert L["angle"].dtype == np.float32 and (L["angle"] >= -h).all() and (L["angle"] < h).all()
        assert L["angle"].min() < -1.5 and L["angle"].max() > 1.5
    c = np.concatenate(counts)
    n = c.shape[0]
    assert n == 102000
    sigma = np.sqrt(n * (1 / 6) * (5 / 6))
    hist = np.bincount(c, minlength=6)
    print("count histogram", hist.tolist(), "largest max_tries", worst)
    assert (np.abs(hist - n / 6) <= 5 * sigma).all(), hist


def test_solid_layouts_use_their_tables(mb):
    for bg in ("solid_fixed", "unseen_solid_fixed"):
        L = mb.layouts_host(mb.BACKGROUNDS[bg], 7, 3, 1, np.arange(2000))
        ncol = len(mb.COLOURS[bg])
        assert (L["colour"][:, 0] == L["colour"][:, 1]).all() and set(L["colour"][:, 0].tolist()) == set(range(ncol))
        assert (L["angle"] == 0).all() and L["sprite"].max() == 6


def test_layout_is_a_function_of_its_key(mb):
    bg = mb.BACKGROUNDS["ckb_rot_6"]
    s = np.arange(64)
    a = mb.layouts_host(bg, N_SPRITES, 5, 0, s)
    assert a.tobytes() == mb.layouts_host(bg, N_SPRITES, 5, 0, s).tobytes()
    assert a[7:9].tobytes() == mb.layouts_host(bg, N_SPRITES, 5, 0, [7, 8]).tobytes()          # addressable sample by sample
    for other in (mb.layouts_host(bg, N_SPRITES, 5, 0, s + 64), mb.layouts_host(bg, N_SPRITES, 5, 1, s),
                  mb.layouts_host(bg, N_SPRITES, 6, 0, s)):
        assert (other["angle"] != a["angle"]).mean() > 0.95
    big = mb.layouts_host(bg, N_SPRITES, 5, 0, [2 ** 40 + 3])
    assert big.tobytes() != mb.layouts_host(bg, N_SPRITES, 5, 0, [3]).tobytes()                 # the high word of the index is keyed


def test_entry_points_validate_arguments(lib_built):
    from split_vae_amd import _lib
    lib = _lib.load()
    L = _lib.MultibirdLayout()
    p = C.c_void_p(C.addressof(L))
    assert lib.sv_multibird_layout_host(None, 0, 4, 0, 0, 0) == _lib.STATUS_BADARG
    assert lib.sv_multibird_layout_host(p, 0, 0, 0, 0, 0) == _lib.STATUS_BADARG
    assert lib.sv_multibird_layout_host(p, 4, 4, 0, 0, 0) == _lib.STATUS_UNSUPPORTED
    assert lib.sv_multibird_layout_host(p, -1, 4, 0, 0, 0) == _lib.STATUS_UNSUPPORTED
    assert lib.sv_multibird_layout_host(p, 0, (1 << 20) + 1, 0, 0, 0) == _lib.STATUS_UNSUPPORTED
    assert lib.sv_multibird_layout_host(p, 3, 4, 0, 0, 0) == 0
    assert lib.sv_multibird_layouts(None, None, 0, 4, 8, 0, 0, 0, None) == _lib.STATUS_BADARG
    assert lib.sv_multibird_layouts(p, None, 0, 4, 0, 0, 0, 0, None) == _lib.STATUS_BADARG
    assert lib.sv_multibird_layouts(p, None, 9, 4, 8, 0, 0, 0, None) == _lib.STATUS_UNSUPPORTED
    assert lib.sv_multibird_canvases(None, None, p, 4, None, None, 0, 8, 0, 0, 0, None) == _lib.STATUS_BADARG
    assert lib.sv_multibird_canvases(p, None, None, 4, None, None, 0, 8, 0, 0, 0, None) == _lib.STATUS_BADARG
    assert lib.sv_multibird_canvases(p, None, p, 4, None, None, 0, 0, 0, 0, 0, None) == _lib.STATUS_BADARG
    assert lib.sv_multibird_canvases(C.c_void_p(C.addressof(L) + 4), None, p, 4, None, None, 0, 8, 0, 0, 0, None) == _lib.STATUS_BADARG
    assert C.sizeof(_lib.MultibirdLayout) == 80


def test_five_branch_intersection_is_the_max_form():
    """calculateIntersection (:18-29) for two 14-wide boxes at every offset pair equals max(0, 14 - |d|); the rule `> 0.15` is
    ix * iy >= 30."""
    for a in range(34):
        for b in range(34):
            assert mr.calculate_intersection(a, a + 14, b, b + 14) == max(0, 14 - abs(a - b))
    for ix in range(15):
        for iy in range(15):
            assert (ix * iy / 14 ** 2 > 0.15) == (ix * iy >= 30)
    assert mr.calculate_overlap(0, 0, [(9, 8)]) and not mr.calculate_overlap(0, 0, [(9, 9)])    # 5 * 6 = 30, 5 * 5 = 25


def test_fp32_division_gives_the_float64_quotient_rounded():
    v = np.arange(256)
    assert np.array_equal(np.float32(v / 255.0), np.float32(v) / np.float32(255))


def test_reference_rotation_rules():
    cols = [mr.TRAIN_COLORS_TRIAD[0], mr.TRAIN_COLORS_TRIAD[3]]
    board = mr.checkerboard(cols)
    assert board.dtype == np.float32 and np.array_equal(board[0, 0], np.float32(np.array(cols[0]) / 255.))
    assert np.array_equal(board[5, 6], board[6, 5]) and np.array_equal(board[5, 6], np.float32(np.array(cols[1]) / 255.))
    rot0, ok = mr.rotate_bilinear(board, 0.0)
    assert ok[:-1, :-1].all() and np.array_equal(rot0[:-1, :-1], board[:-1, :-1].astype(np.float64))
    assert np.array_equal(mr.background("ckb_rot_6", (0, 3), 0.0), board[72:120, 72:120])       # angle 0: the unrotated crop, exactly
    for ang in (0.3, 1.1, -0.7, 1.3):
        full, _ = mr.rotate_bilinear(board, ang)
        part, okp = mr.rotate_bilinear(board, ang, region=(72, 120))
        assert okp.all() and np.array_equal(mr.central_crop_quarter(full), part)
        a, b = mr.background("ckb_rot_6", (0, 3), ang), mr.background("ckb_rot_6", (0, 3), -ang)
        assert np.abs(a - b.transpose(1, 0, 2)).max() < 1e-6 and np.abs(a - b).max() > 0.1    # mirror images about the diagonal
        assert a.min() >= min(min(c) for c in cols) / 255. - 1e-6 and a.max() <= 1.0


def test_reference_paste_rules(mb):
    bank = np.zeros((2, 14, 14, 3), np.uint8)
    bank[0, 2:9, 3:11] = (0, 7, 255)
    bank[0, 4, 4] = 0                                                    # a hole: all channels 0 leaves the background
    bank[1, :, :] = (200, 1, 0)
    L = np.zeros(1, mb.LAYOUT_DTYPE)[0]
    L["colour"] = (2, 2)
    blank = mr.create_sample(L, bank, "solid_fixed")
    want = np.float32(np.array(mr.TRAIN_COLORS[2]) / 255.)
    assert blank.dtype == np.float32 and (blank == want).all()           # count 0 on solid_fixed: constant
    L["count"], L["row"][:2], L["col"][:2], L["sprite"][:2] = 2, (5, 10), (20, 22), (0, 1)
    x = mr.create_sample(L, bank, "solid_fixed")
    assert np.array_equal(x[5 + 4, 20 + 4], want) and np.array_equal(x[5 + 2, 20 + 3], np.float32(np.array([0, 7, 255]) / 255.0))
    assert np.array_equal(x[10, 22], np.float32(np.array([200, 1, 0]) / 255.0))                # the later sprite is on top
    assert np.array_equal(x[4], blank[4]) and np.array_equal(x[:, 36:], blank[:, 36:])       # rows index axis 0 (rand_x, :152)


def test_procedural_bank(mb):
    a, b = mb.procedural_bank(64, seed=0), mb.procedural_bank(64, seed=0)
    t, s1 = mb.procedural_bank(64, seed=0, test=True), mb.procedural_bank(64, seed=1)
    assert a.shape == (64, 14, 14, 3) and a.dtype == np.uint8 and np.array_equal(a, b)
    assert not np.array_equal(a, t) and not np.array_equal(a, s1)
    mask = a.max(-1) > 0
    area = mask.reshape(64, -1).sum(1)
    assert area.min() >= 20 and area.max() <= 150                        # a bird, not a full tile and not a speck
    assert (a[~mask] == 0).all() and len({tuple(x[m].mean(0).round()) for x, m in zip(a, mask)}) > 32      # hues differ
    tr, te, stand_in = mb.load_banks(os.path.join(os.path.dirname(__file__), "no_such_dir"), seed=0, n=16)
    assert stand_in and tr.shape == te.shape == (16, 14, 14, 3) and not np.array_equal(tr, te)


def test_example_codec_round_trip():
    from split_vae_amd import tfrecord
    img = np.random.default_rng(0).random((4, 4, 3)).astype(np.float32)
    for label in (0, 5, 300, -2):
        rec = tfrecord.encode_example({"image": tfrecord.serialize_tensor(img), "label": label})
        ex = tfrecord.parse_example(rec)
        assert sorted(ex) == ["image", "label"] and ex["label"] == [label]
        assert np.array_equal(tfrecord.parse_tensor(ex["image"][0]), img)
    # the wire bytes of a known message: Example{features{feature{key:"label" value{int64_list{value:[5]}}}}}
    assert tfrecord.encode_example({"label": 5}) == bytes.fromhex("0a100a0e0a056c6162656c12051a030a0105")
    assert tfrecord.parse_example(bytes.fromhex("0a0f0a0d0a056c6162656c12041a020805")) == {"label": [5]}   # unpacked form
    assert tfrecord.parse_example(tfrecord.encode_example({"w": 0.5}))["w"] == [0.5]


def test_tfrec_round_trip_and_dataset_names(mb, tmp_path):
    def renderer(bank, bg, n, seed, split):
        name = [k for k, v in mb.BACKGROUNDS.items() if v == bg][0]
        return mr.create_dataset(mb.layouts_host(bg, bank.shape[0], seed, split, np.arange(n)), bank, name)

    d = str(tmp_path)
    paths = mb.write_cub_tfrec("cub_ckb_rot_6", n_train=5, n_test=3, data_dir=d, seed=2, renderer=renderer)
    assert [os.path.basename(p) for p in paths] == ["train_cub_ckb_rot_6.tfrec", "test_cub_ckb_rot_6.tfrec", "test_unseen_cub_ckb_rot_6.tfrec"]
    train, tests, shape, tshape = mb.get_cub_dataset("cub_ckb_rot_6", batch_size=2, data_dir=d, device="cpu")
    assert shape == [-1, 48, 48, 3] == tshape and len(tests) == 2
    tr_bank, te_bank, _ = mb.load_banks(d, 2)
    want, _ = renderer(tr_bank, mb.BACKGROUNDS["ckb_rot_6"], 5, 2, mb.SPLIT_TRAIN)
    assert np.array_equal(train.x, want)
    for t, (split, bg) in zip(tests, ((mb.SPLIT_TEST, "ckb_rot_6"), (mb.SPLIT_TEST_UNSEEN, "unseen_ckb_rot_6"))):
        wx, wy = renderer(te_bank, mb.BACKGROUNDS[bg], 3, 2, split)
        got = list(t)
        assert [g[0].shape[0] for g in got] == [2, 1]                    # the last batch keeps the remainder
        assert np.array_equal(np.concatenate([g[0].numpy() for g in got]), wx)
        assert np.array_equal(np.concatenate([g[1].numpy() for g in got]), wy)
    with pytest.raises(NotImplementedError, match="Undefined dataset"):
        mb.get_cub_dataset("cub_16x16_ckb", data_dir=d, device="cpu")
    with pytest.raises(NotImplementedError):
        mb.write_cub_tfrec("svhn", data_dir=d, renderer=renderer)


def test_train_index_stream_is_the_shuffle_buffer(mb):
    import itertools
    src = mb.TrainCanvases(None, 0, 4, n=50, shuffle_seed=1, buffer_size=20)
    idx = list(itertools.islice(src.indices(), 120))
    assert sorted(idx[:50]) == list(range(50)) and sorted(idx[50:100]) == list(range(50)) and idx[:50] != idx[50:100]
    assert max(idx[:10]) < 30                                            # the first ten come from a 20-element buffer


def test_cli_flags(mb):
    from split_vae_amd import spair_main
    a = spair_main.build_parser().parse_args(["--dataset", "cub_ckb_rot_6"])
    assert a.data_dir == "data" and not a.synthetic and a.dataset == "cub_ckb_rot_6"
    assert spair_main.build_parser().parse_args(["--data_dir", "/x"]).data_dir == "/x"
