"""Multi-Bird data source of SPLIT-SPAIR (spair/data.py of the reference) on the device.

The reference synthesises 100 000 + 2 x 1 000 canvases on the CPU (MultiCUB.create_dataset, :39-174) and stores them as
TFRecord files.  Here canvas i of a split is a pure function of (seed, split, i), rendered by one kernel launch per batch
(csrc/multibird.hip, sv_multibird_canvases): nothing is stored and nothing is copied per step but the batch's indices.

Sprite bank.  The reference pastes data/cub_{train,test}_seg_14x14_pad_20_masked.npy (:13-16, uint8-valued [N,14,14,3], zero
outside the bird), which are not in its repository.  They are loaded when they exist under --data_dir; otherwise
`procedural_bank` draws a STAND-IN bank (ellipse body, head disc, tail wedge, a hue per sprite, hard mask), so counts,
layouts and backgrounds are the reference's but the birds are not CUB crops.
"""
import colorsys
import os

import numpy as np
import torch

from . import _lib, tfrecord
from .data import SHUFFLE_BUFFER, ArrayDataset, _shuffled_indices

BACKGROUNDS = {"solid_fixed": _lib.SV_MB_SOLID_FIXED, "unseen_solid_fixed": _lib.SV_MB_UNSEEN_SOLID_FIXED,
               "ckb_rot_6": _lib.SV_MB_CKB_ROT_6, "unseen_ckb_rot_6": _lib.SV_MB_UNSEEN_CKB_ROT_6}
# spair/data.py:52-57 (train_colors, test_colors, train_colors_triad, test_colors_triad), in the order of csrc/multibird.hip
COLOURS = {
    "solid_fixed": [(100, 209, 72), (209, 72, 100), (209, 127, 72), (72, 129, 209), (84, 184, 209), (209, 109, 84), (184, 209, 84),
                    (109, 84, 209)],
    "unseen_solid_fixed": [(222, 222, 102), (100, 100, 219), (219, 100, 219), (100, 219, 100)],
    "ckb_rot_6": [(195, 135, 255), (193, 255, 135), (255, 165, 135), (81, 197, 255), (255, 229, 81), (255, 81, 139)],
    "unseen_ckb_rot_6": [(255, 125, 227), (125, 255, 184), (255, 205, 125)],
}
DATASETS = ("cub_solid_fixed", "cub_ckb_rot_6")            # create_cub_tfrec :232
SPLIT_TRAIN, SPLIT_TEST, SPLIT_TEST_UNSEEN = 0, 1, 2
N_TRAIN, N_TEST = 100000, 1000                             # :239-247
LAYOUT_DTYPE = np.dtype([("count", "<i4"), ("row", "<i4", (5,)), ("col", "<i4", (5,)), ("sprite", "<i4", (5,)),
                         ("colour", "<i4", (2,)), ("max_tries", "<i4"), ("angle", "<f4")])
assert LAYOUT_DTYPE.itemsize == 80


def layouts_host(bg, n_sprites, seed, split, samples):
    """Structured array (LAYOUT_DTYPE) of sv_multibird_layout_host over `samples` (no device)."""
    import ctypes as C
    samples = np.asarray(samples, np.int64).reshape(-1)
    out = np.zeros(samples.shape[0], LAYOUT_DTYPE)
    f = _lib.load().sv_multibird_layout_host
    base = out.ctypes.data
    for i, s in enumerate(samples.tolist()):
        _lib.check(f(C.c_void_p(base + 80 * i), bg, n_sprites, seed, split, s), "sv_multibird_layout_host")
    return out


def layouts_to_numpy(t):
    """int32 [B,20] device layouts (ops.multibird_layouts) -> structured array."""
    return np.ascontiguousarray(t.cpu().numpy()).view(LAYOUT_DTYPE).reshape(-1)


def layouts_to_tensor(a, device="cuda"):
    return torch.from_numpy(np.ascontiguousarray(a).view("<i4").reshape(-1, 20).copy()).to(device)


def procedural_bank(n=256, seed=0, test=False):
    """Stand-in sprite bank, uint8 [n,14,14,3]: an ellipse body, a head disc and a tail wedge under a hard mask, a hue per
    sprite; every masked pixel has a non-zero channel, everything outside is 0.  Deterministic in (seed, test)."""
    rng = np.random.default_rng([int(seed), int(bool(test)), 0x6D62])
    yy, xx = np.mgrid[0:14, 0:14].astype(np.float64) + 0.5
    out = np.zeros((n, 14, 14, 3), np.uint8)
    for i in range(n):
        th = rng.uniform(-0.6, 0.6)
        a, b = rng.uniform(3.2, 4.6), rng.uniform(2.0, 3.0)
        cy, cx = 7 + rng.uniform(-0.7, 0.7), 7 + rng.uniform(-0.7, 0.7)
        face = 1.0 if rng.integers(2) else -1.0
        u = (xx - cx) * np.cos(th) + (yy - cy) * np.sin(th)
        v = -(xx - cx) * np.sin(th) + (yy - cy) * np.cos(th)
        body = (u / a) ** 2 + (v / b) ** 2 <= 1.0
        head = (u - face * a * 0.85) ** 2 + (v + b * 0.6) ** 2 <= rng.uniform(1.3, 1.9) ** 2
        s = -face * u - a * 0.6
        tail = (s >= 0) & (s <= rng.uniform(2.0, 3.5)) & (np.abs(v) <= 0.4 + 0.45 * s)
        hue, sat = rng.uniform(), rng.uniform(0.45, 0.95)
        shade = rng.uniform(0.75, 1.0, size=(14, 14, 1))
        img = np.zeros((14, 14, 3))
        for mask, dh, val in ((tail, 0.08, 0.6), (body, 0.0, 0.9), (head, 0.5, 1.0)):     # head drawn last: on top
            img[mask] = colorsys.hsv_to_rgb((hue + dh) % 1.0, sat, val)
        out[i] = np.where((body | head | tail)[..., None], np.clip(np.rint(img * shade * 255.0), 40, 255), 0).astype(np.uint8)
        out[i][(body | head | tail) & (out[i].max(-1) == 0)] = 40
    return out


def load_banks(data_dir="data", seed=0, n=256):
    """(train bank, test bank, stand_in): the reference's .npy files under data_dir when both exist, else procedural banks."""
    paths = [os.path.join(data_dir, "cub_%s_seg_14x14_pad_20_masked.npy" % s) for s in ("train", "test")]
    if all(os.path.exists(p) for p in paths):
        banks = [np.ascontiguousarray(np.clip(np.load(p), 0, 255).astype(np.uint8)) for p in paths]
        for p, b in zip(paths, banks):
            if b.ndim != 4 or b.shape[1:] != (14, 14, 3) or b.shape[0] == 0:
                raise ValueError("%s: expected [N,14,14,3], got %s" % (p, b.shape))
        return banks[0], banks[1], False
    return procedural_bank(n, seed, False), procedural_bank(n, seed, True), True


class TrainCanvases:
    """cache().shuffle(20000).repeat().batch(B) (spair/main.py:78,87) over n virtual canvases: the shuffle buffer runs on
    indices, each batch is one kernel launch over a device index[B].  Indices are uploaded `chunk` batches at a time."""

    def __init__(self, bank, bg, batch_size, n=N_TRAIN, seed=0, split=SPLIT_TRAIN, shuffle_seed=0, buffer_size=SHUFFLE_BUFFER, chunk=64):
        self.bank, self.bg, self.bs, self.n, self.seed, self.split = bank, bg, batch_size, n, seed, split
        self.shuffle_seed, self.buffer_size, self.chunk = shuffle_seed, buffer_size, chunk
        self.labelled = False

    def indices(self):
        epoch = 0
        while True:
            yield from _shuffled_indices(self.n, self.buffer_size, np.random.default_rng([self.shuffle_seed, epoch]))
            epoch += 1

    def __iter__(self):
        from . import ops
        it = self.indices()
        while True:
            idx = torch.tensor([next(it) for _ in range(self.bs * self.chunk)], dtype=torch.int64).to(self.bank.device)
            for c in range(self.chunk):
                yield ops.multibird_canvases(self.bank, self.bg, self.bs, self.seed, self.split, index=idx[c * self.bs:(c + 1) * self.bs])[0]


class LabelledBatches:
    """A finite test set resident on the device as batches of (images, counts); the last batch keeps the remainder
    (Dataset.batch without drop_remainder).  `augment` is applied per batch at every pass, as Dataset.map does."""

    def __init__(self, x, y, batch_size, augment=None, label=True):
        self.x, self.y, self.bs, self.augment, self.label = x, y, batch_size, augment, label
        self.labelled = label

    def __iter__(self):
        for i in range(0, self.x.shape[0], self.bs):
            xb = self.x[i:i + self.bs]
            if self.augment is not None:
                xb = self.augment(xb)
            yield (xb, self.y[i:i + self.bs]) if self.label else xb


def render(bank, bg, n, seed, split):
    """All n canvases of a split in one launch -> (x [n,48,48,3], count [n]) on the bank's device."""
    from . import ops
    return ops.multibird_canvases(bank, bg, n, seed, split)


def _tfrec_paths(name, data_dir):
    return [os.path.join(data_dir, "multi_cub", "%s_%s.tfrec" % (s, name)) for s in ("train", "test", "test_unseen")]


def _check_name(name):
    if name not in DATASETS:
        print(name)
        raise NotImplementedError('Undefined dataset')                  # spair/data.py:232-234


def get_cub_dataset(name, size=48, channel=3, batch_size=32, data_dir="data", seed=0, device="cuda", n_train=N_TRAIN, n_test=N_TEST):
    """spair/data.py:258-278 -> (train, [test, test_unseen], [-1,size,size,channel] twice).  train iterates [B,48,48,3] batches
    forever; the test sets are LabelledBatches of (images, counts).  The reference's TFRecord files under
    data_dir/multi_cub/ are read when all three exist; otherwise the canvases come from the kernel."""
    _check_name(name)
    if size != 48 or channel != 3:
        raise NotImplementedError("Multi-Bird canvases are 48 x 48 x 3 (spair/data.py:239-247)")
    shape = [-1, size, size, channel]
    paths = _tfrec_paths(name, data_dir)
    if all(os.path.exists(p) for p in paths):
        train = ArrayDataset(tfrecord.read_celeba_tfrec_array(paths[0], size), batch_size, True, seed, device)
        tests = []
        for p in paths[1:]:
            x, y = read_labelled_tfrec(p, size, channel)
            tests.append(LabelledBatches(torch.from_numpy(x).to(device), torch.from_numpy(y).to(device), batch_size))
        return train, tests, shape, shape
    from . import detection
    bg = name[4:]
    train_bank, test_bank, _ = load_banks(data_dir, seed)
    train_bank, test_bank = torch.from_numpy(train_bank).to(device), torch.from_numpy(test_bank).to(device)
    train = TrainCanvases(train_bank, BACKGROUNDS[bg], batch_size, n_train, seed, SPLIT_TRAIN, shuffle_seed=seed)
    tests = []
    for split, b in ((SPLIT_TEST, bg), (SPLIT_TEST_UNSEEN, "unseen_" + bg)):              # :239,247: the test sprite bank for both
        x, y = render(test_bank, BACKGROUNDS[b], n_test, seed, split)
        tests.append(LabelledBatches(x, y, batch_size))
        # the canvases' ground-truth boxes (detection.py): attributes only, iteration yields what it always did
        tests[-1].boxes, tests[-1].n_boxes = detection.ground_truth(test_bank, BACKGROUNDS[b], test_bank.shape[0], n_test, seed, split)
    return train, tests, shape, shape


def read_labelled_tfrec(path, size=48, channel=3):
    """parse_48_with_label (spair/data.py:217-227) over a whole file -> (images [N,size,size,channel] fp32, labels [N] fp32)."""
    xs, ys = [], []
    for rec in tfrecord.read_records(path):
        ex = tfrecord.parse_example(rec)
        xs.append(tfrecord.parse_tensor(ex["image"][0]).reshape(size, size, channel))
        ys.append(ex["label"][0])
    x = np.stack(xs) if xs else np.zeros((0, size, size, channel), np.float32)
    return x, np.asarray(ys, np.float32)


def write_cub_tfrec(name, n_train=N_TRAIN, n_test=N_TEST, data_dir="data", seed=0, device="cuda", renderer=None):
    """create_cub_tfrec (spair/data.py:229-255): the three files of `name` from the generator, in the reference's formats --
    train records are serialize_tensor(image), test records a tf.train.Example {image: bytes_list, label: int64_list}.
    renderer(bank, bg, n, seed, split) -> (x, count) replaces the kernel (the host tests pass their NumPy restatement)."""
    _check_name(name)
    bg = name[4:]
    train_bank, test_bank, _ = load_banks(data_dir, seed)
    if renderer is None:
        def renderer(bank, b, n, seed_, split):
            x, y = render(torch.from_numpy(bank).to(device), b, n, seed_, split)
            return x.cpu().numpy(), y.cpu().numpy()
    os.makedirs(os.path.join(data_dir, "multi_cub"), exist_ok=True)
    paths = _tfrec_paths(name, data_dir)
    x, _ = renderer(train_bank, BACKGROUNDS[bg], n_train, seed, SPLIT_TRAIN)
    tfrecord.write_records(paths[0], (tfrecord.serialize_tensor(im) for im in x))
    for p, split, b in ((paths[1], SPLIT_TEST, bg), (paths[2], SPLIT_TEST_UNSEEN, "unseen_" + bg)):
        x, y = renderer(test_bank, BACKGROUNDS[b], n_test, seed, split)
        tfrecord.write_records(p, (tfrecord.encode_example({"image": tfrecord.serialize_tensor(im), "label": int(c)})
                                   for im, c in zip(x, y)))
    return paths
