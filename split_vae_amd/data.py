"""Input side of the SPLIT-VAE path.  The metric runs on synthetic batches in the reference's data
domain (vae/data.py:52: x/255*2-1, fp32 NHWC); the on-disk formats of vae/data.py are
read without TensorFlow: SVHN .mat here, the CelebA TFRecord-of-serialize_tensor files in tfrecord.py,
both behind the pipeline of vae/main.py:56-61,

    train: dataset.shuffle(20000).repeat().map(augment).batch(B)     (batches never partial, they span epochs)
    test : dataset.shuffle(20000).map(augment).batch(B)              (the last batch keeps the remainder)

with (image, label) tuples when `get_label` (vae/main.py:56-58, vae/data.py:54-62) and bare images otherwise.
The augmentation itself (the patch scramble) runs batched on the device, after batching.
ResidentDataset keeps a whole on-disk set in device memory instead and serves the same batches in the same order: the host
sends index lists (ShuffleIndexStream), a kernel fetches them (csrc/dataset.hip)."""
import os

import numpy as np
import torch

SHAPES = {"svhn": [-1, 32, 32, 3], "svhn_no_extra": [-1, 32, 32, 3], "celeba64": [-1, 64, 64, 3],
          "celeba128": [-1, 128, 128, 3]}
SHUFFLE_BUFFER = 20000                      # vae/main.py:57-61


def synthetic_images(n, H, W, seed=0, device="cuda", sample_offset=0):
    """n images uniform over the 256 quantised levels {-1 + 2k/255}; sample i depends only on
    (seed, sample_offset + i) so shards of a global batch are slices of the single-process batch."""
    out = torch.empty((n, H, W, 3), dtype=torch.float32)
    for i in range(n):
        rng = np.random.Generator(np.random.PCG64([seed, sample_offset + i]))
        out[i] = torch.from_numpy((rng.integers(0, 256, size=(H, W, 3)) / 255.0 * 2 - 1).astype(np.float32))
    return out.to(device)


class SyntheticDataset:
    """Infinite (train) or finite (test) iterator of [B,H,W,3] device batches."""

    def __init__(self, H, W, batch_size, n_batches=None, seed=0, device="cuda", pool=4):
        self.pool = [synthetic_images(batch_size, H, W, seed + 1000 * k, device) for k in range(pool)]
        self.n_batches = n_batches
        self.labelled = False

    def __iter__(self):
        i = 0
        while self.n_batches is None or i < self.n_batches:
            yield self.pool[i % len(self.pool)]
            i += 1


def normalise_u8(x):
    """vae/data.py:52-53: (x / 255.0 * 2 - 1).astype(np.float32) -- the division, scale and shift run in float64
    (NumPy promotes uint8 / float) and only the result is rounded to fp32.  Doing the arithmetic in fp32 instead
    differs in the last bit on 128 of the 256 pixel levels."""
    return (np.asarray(x) / 255.0 * 2 - 1).astype(np.float32)


def one_hot_svhn(y, depth=10):
    """vae/data.py:55-57: tf.squeeze(tf.one_hot(y - 1, 10)); SVHN stores digit 0 as label 10, so "0" is the LAST
    index.  (tf.one_hot gives an all-zero row for an index outside [0, depth).)"""
    idx = np.asarray(y).reshape(-1).astype(np.int64) - 1
    out = np.zeros((idx.shape[0], depth), np.float32)
    ok = (idx >= 0) & (idx < depth)
    out[np.nonzero(ok)[0], idx[ok]] = 1.0
    return out


def load_svhn_mat(path):
    """vae/data.py:44-53: scipy.io.loadmat(...)['X'] is [32,32,3,N] uint8 -> [N,32,32,3] fp32 in [-1,1];
    returns (x, y) with y the raw [N] labels in 1..10."""
    import scipy.io
    m = scipy.io.loadmat(path)
    x = normalise_u8(np.transpose(m["X"], (3, 0, 1, 2)))
    return x, m["y"].reshape(-1)


def load_svhn_mat_u8(path):
    """The same file as stored: (x [N,32,32,3] uint8 pixel levels, y [N] uint8 labels in 1..10) -- what a ResidentDataset keeps
    on the device (a quarter of the fp32 bytes; sv_dataset_gather normalises through normalise_u8's table)."""
    import scipy.io
    m = scipy.io.loadmat(path)
    return np.ascontiguousarray(np.transpose(m["X"], (3, 0, 1, 2)), dtype=np.uint8), m["y"].reshape(-1).astype(np.uint8)


def _shuffled_indices(n, buffer_size, rng):
    """Index stream of tf.data's shuffle(buffer_size) over elements 0..n-1: keep `buffer_size` candidates, emit a
    uniformly random one and replace it by the next input, drain randomly at the end (same algorithm as
    tfrecord.shuffle_buffer, on indices so that an array source is gathered once per batch)."""
    buf = list(range(min(n, buffer_size)))
    for nxt in range(len(buf), n):
        j = int(rng.integers(len(buf)))
        out, buf[j] = buf[j], nxt
        yield out
    while buf:
        j = int(rng.integers(len(buf)))
        buf[j], buf[-1] = buf[-1], buf[j]
        yield buf.pop()


class ArrayDataset:
    """shuffle(buffer).repeat()?.batch(B) over in-memory arrays (vae/main.py:56-61).  With labels the batches are
    (x[B,H,W,3], y[B,10]) tuples; repeat=True never yields a partial batch (the batch spans the epoch boundary, as
    .repeat().batch() does), repeat=False ends with the remainder (Dataset.batch keeps it)."""

    def __init__(self, x, batch_size, repeat, shuffle_seed=0, device="cuda", y=None, buffer_size=SHUFFLE_BUFFER):
        self.x, self.y, self.bs, self.repeat, self.seed, self.device = x, y, batch_size, repeat, shuffle_seed, device
        self.buffer_size = buffer_size
        self.labelled = y is not None

    def _emit(self, idx):
        idx = np.asarray(idx)
        xb = torch.from_numpy(self.x[idx]).to(self.device)
        if self.y is None:
            return xb
        return xb, torch.from_numpy(self.y[idx]).to(self.device)

    def __iter__(self):
        n = self.x.shape[0]
        epoch, pend = 0, []
        while True:
            rng = np.random.default_rng([self.seed, epoch])
            for i in _shuffled_indices(n, self.buffer_size, rng):
                pend.append(i)
                if len(pend) == self.bs:
                    yield self._emit(pend)
                    pend = []
            if not self.repeat:
                if pend:
                    yield self._emit(pend)
                return
            if n == 0:
                return
            epoch += 1


class StreamDataset:
    """shuffle(buffer).repeat()?.batch(B) over a re-iterable source of single images (vae/main.py:59-61; the
    CelebA TFRecord files carry no labels, vae/data.py:102-134)."""

    def __init__(self, make_iter, batch_size, repeat, buffer_size=SHUFFLE_BUFFER, seed=0, device="cuda"):
        self.make_iter, self.bs, self.repeat, self.buffer_size, self.seed, self.device = make_iter, batch_size, repeat, buffer_size, seed, device
        self.labelled = False

    def __iter__(self):
        from .tfrecord import shuffle_buffer
        epoch, batch = 0, []
        while True:
            seen = 0
            for x in shuffle_buffer(self.make_iter(), self.buffer_size, self.seed + epoch):
                seen += 1
                batch.append(x)
                if len(batch) == self.bs:
                    yield torch.from_numpy(np.stack(batch)).to(self.device)
                    batch = []
            if not self.repeat:
                if batch:
                    yield torch.from_numpy(np.stack(batch)).to(self.device)      # Dataset.batch keeps the remainder
                return
            if seen == 0:
                return
            epoch += 1                      # .repeat().batch(): a batch may span the epoch boundary


def shuffled_index_array(n, buffer_size, rng):
    """list(_shuffled_indices(n, buffer_size, rng)) -- equally the order tfrecord.shuffle_buffer(range(n), buffer_size, seed)
    emits when rng = default_rng(seed) -- as one int64 array, from two vectorised draws instead of n scalar ones.
    Fill phase (m = min(n, buffer) slots, k = n - m emissions): one rng.integers(m, size=k); the element emitted at time t is
    what was last written into slot j[t] -- m + t' for the latest t' < t with j[t'] == j[t], else j[t] itself.  Drain: one
    rng.integers(0, [m, m-1, ..., 1]) and the generator's swap-and-pop over the m survivors.  The Generator consumes its bit
    stream the same way for the array draws as for the scalar ones (tests/test_resident_host.py pins that)."""
    m = min(n, buffer_size)
    k = n - m
    out = np.empty(n, np.int64)
    if m <= 0:
        return out[:0]
    buf = np.arange(m, dtype=np.int64)
    if k:
        j = rng.integers(m, size=k)
        order = np.argsort(j, kind="stable")               # emissions grouped by slot, in time order inside a group
        js = j[order]
        same = js[1:] == js[:-1]
        val = js.copy()
        val[1:][same] = m + order[:-1][same]
        out[:k][order] = val
        last = np.concatenate([~same, [True]])
        buf[js[last]] = m + order[last]
    jd = rng.integers(0, np.arange(m, 0, -1))
    b = buf.tolist()
    tail = []
    for jj in jd.tolist():
        v = b[jj]
        b[jj] = b[-1]
        b.pop()
        tail.append(v)
    out[k:] = tail
    return out


class ShuffleIndexStream:
    """The index order of shuffle(buffer_size).repeat()? over n elements, served in chunks: `take(k)` returns the next k indices
    (fewer only when a non-repeating stream ends).  Element for element the order of ArrayDataset (epoch e drawn from
    default_rng([seed, e])) or, with stream_seeding, of StreamDataset (default_rng(seed + e), tfrecord.shuffle_buffer)."""

    def __init__(self, n, buffer_size=SHUFFLE_BUFFER, seed=0, repeat=False, stream_seeding=False):
        self.n, self.buffer_size, self.seed, self.repeat, self.stream_seeding = int(n), buffer_size, seed, repeat, stream_seeding
        self.epoch = 0
        self._cur, self._pos = None, 0

    def _next_epoch(self):
        rng = np.random.default_rng(self.seed + self.epoch if self.stream_seeding else [self.seed, self.epoch])
        self._cur, self._pos = shuffled_index_array(self.n, self.buffer_size, rng), 0
        self.epoch += 1

    def take(self, k):
        parts, need = [], int(k)
        while need > 0:
            if self._cur is None or self._pos >= len(self._cur):
                if self.n <= 0 or (self._cur is not None and not self.repeat):
                    break
                self._next_epoch()
            part = self._cur[self._pos:self._pos + need]
            self._pos += len(part)
            need -= len(part)
            parts.append(part)
        return np.concatenate(parts) if parts else np.empty(0, np.int64)


class ResidentDataset:
    """shuffle(buffer).repeat()?.batch(B) (vae/main.py:56-61) over a set that lives in device memory: x [N,H,W,3] uint8 (SVHN's
    pixel levels, normalised through `lut` by the fetch kernel) or float32 (the CelebA files' images), labels [N] uint8 (SVHN's
    1..10) or None.  The host's part per batch is an int32 index list, uploaded `chunk_batches` batches at a time; the fetch is
    sv_dataset_gather (+ sv_dataset_onehot), or, through Augmentator.scramble_from, the fused gather + scramble + staging.
    Iterating yields exactly ArrayDataset's batches for the same arguments (StreamDataset's with stream_seeding): repeat=True
    never yields a partial batch, repeat=False ends with the remainder.  A set that does not fit in free device memory raises."""

    def __init__(self, x, batch_size, repeat, shuffle_seed=0, device="cuda", labels=None, buffer_size=SHUFFLE_BUFFER,
                 stream_seeding=False, chunk_batches=64):
        x = np.ascontiguousarray(x)
        if x.ndim != 4 or x.shape[3] != 3 or x.dtype not in (np.uint8, np.float32):
            raise ValueError("ResidentDataset holds [N,H,W,3] uint8 or float32 images, got %s %s" % (x.dtype, x.shape))
        self.N, self.H, self.W = int(x.shape[0]), int(x.shape[1]), int(x.shape[2])
        self.bs, self.repeat, self.seed, self.device = batch_size, repeat, shuffle_seed, torch.device(device)
        self.buffer_size, self.stream_seeding, self.chunk_batches = buffer_size, stream_seeding, max(1, int(chunk_batches))
        self.labelled = labels is not None
        if self.labelled:
            labels = np.ascontiguousarray(np.asarray(labels).reshape(-1), dtype=np.uint8)
            if labels.shape[0] != self.N:
                raise ValueError("%d labels for %d images" % (labels.shape[0], self.N))
        need = x.nbytes + (labels.nbytes if self.labelled else 0)
        if self.device.type == "cuda":
            free, total = torch.cuda.mem_get_info(self.device)
            if need > free:
                raise RuntimeError("resident dataset needs %d bytes of device memory (%d images of %d bytes), %d of %d are free"
                                   % (need, self.N, x.nbytes // max(self.N, 1), free, total))
        self.data = torch.from_numpy(x).to(self.device)
        self.labels = torch.from_numpy(labels).to(self.device) if self.labelled else None
        self.lut = torch.from_numpy(self.make_lut()).to(self.device) if x.dtype == np.uint8 else None

    @staticmethod
    def make_lut():
        """lut[v] = the normalised value of pixel level v: vae/data.py:52's float64 arithmetic, rounded to fp32 once."""
        return normalise_u8(np.arange(256, dtype=np.uint8))

    def upload_index(self, index):
        """A host index list -> int32 device tensor; an index outside [0, N) raises ValueError here, on the host, before any upload."""
        idx = np.asarray(index).reshape(-1)
        if idx.size and (int(idx.min()) < 0 or int(idx.max()) >= self.N):
            raise ValueError("dataset index outside [0, %d): min %d, max %d" % (self.N, int(idx.min()), int(idx.max())))
        return torch.from_numpy(idx.astype(np.int32)).to(self.device)

    def index_batches(self):
        """The batches' index lists as int32 device tensors, in iteration order."""
        stream = ShuffleIndexStream(self.N, self.buffer_size, self.seed, self.repeat, self.stream_seeding)
        while True:
            chunk = stream.take(self.bs * self.chunk_batches)
            if chunk.size == 0:
                return
            dev = self.upload_index(chunk)
            for off in range(0, chunk.size, self.bs):
                yield dev[off:off + self.bs]

    def gather(self, index):
        """index: int32 device tensor [B] (index_batches, upload_index) -> x[B,H,W,3] fp32."""
        from . import ops
        return ops.dataset_gather(self.data, index, lut=self.lut)

    def one_hot(self, index, depth=10):
        from . import ops
        return ops.dataset_onehot(self.labels, index, depth)

    def __iter__(self):
        for idx in self.index_batches():
            yield (self.gather(idx), self.one_hot(idx)) if self.labelled else self.gather(idx)


def get_dataset(dataset="svhn", batch_size=64, synthetic=False, data_dir="data", device="cuda", test_batches=4,
                get_label=False, resident=False):
    """vae/data.py:11-21 + the pipeline of vae/main.py:55-61 -> (train_iterable, test_iterable, input_shape).
    Each iterable has `.labelled`: True when its batches are (images, one-hot labels) tuples -- only the SVHN files
    carry labels (vae/data.py:54-62; get_celeba_tfrec ignores get_label).
    resident=True: the on-disk sets are held in device memory (ResidentDataset: SVHN as uint8, CelebA as fp32) and serve the
    same batches in the same order."""
    if dataset not in SHAPES:
        raise NotImplementedError('Dataset doesn\'t exit')          # vae/data.py:21
    shape = SHAPES[dataset]
    H, W = shape[1], shape[2]
    if synthetic and resident:
        raise ValueError("resident=True serves the on-disk datasets; synthetic batches already live on the device")
    if synthetic:
        return (SyntheticDataset(H, W, batch_size, None, 0, device), SyntheticDataset(H, W, batch_size, test_batches, 77, device), shape)
    if dataset.startswith("svhn"):                                     # vae/data.py:23-75
        root = os.path.join(data_dir, "SVHN")
        tr, te, ex = (os.path.join(root, f + "_32x32.mat") for f in ("train", "test", "extra"))
        extra = dataset == "svhn"                                      # 'svhn_no_extra' leaves extra_32x32.mat out (:15-16)
        need = [tr, te] + ([ex] if extra else [])
        missing = [f for f in need if not os.path.exists(f)]
        if missing:
            raise FileNotFoundError("SVHN files %s not found (the reference would download them, vae/data.py:34-42; "
                                    "no network here); pass --synthetic%s" %
                                    (missing, " or --dataset svhn_no_extra" if missing == [ex] else ""))
        if resident:
            xtr, ytr = load_svhn_mat_u8(tr)
            xte, yte = load_svhn_mat_u8(te)
            if extra:
                xex, yex = load_svhn_mat_u8(ex)
                xtr, ytr = np.concatenate([xtr, xex]), np.concatenate([ytr, yex])
            return (ResidentDataset(xtr, batch_size, True, 0, device, labels=ytr if get_label else None),
                    ResidentDataset(xte, batch_size, False, 1, device, labels=yte if get_label else None), shape)
        xtr, ytr = load_svhn_mat(tr)
        xte, yte = load_svhn_mat(te)
        if extra:
            xex, yex = load_svhn_mat(ex)
            xtr, ytr = np.concatenate([xtr, xex]), np.concatenate([ytr, yex])
        ltr, lte = (one_hot_svhn(ytr), one_hot_svhn(yte)) if get_label else (None, None)
        return (ArrayDataset(xtr, batch_size, True, 0, device, y=ltr), ArrayDataset(xte, batch_size, False, 1, device, y=lte), shape)
    from .tfrecord import read_celeba_tfrec                            # vae/data.py:102-131
    tr = os.path.join(data_dir, "celeba", "train_%dx%d.tfrec" % (H, W))
    te = os.path.join(data_dir, "celeba", "test_%dx%d.tfrec" % (H, W))
    if not (os.path.exists(tr) and os.path.exists(te)):
        raise FileNotFoundError("dataset files for %r not found under %r (no network here); pass --synthetic" % (dataset, data_dir))
    if resident:
        from .tfrecord import read_celeba_tfrec_array
        return (ResidentDataset(read_celeba_tfrec_array(tr, H), batch_size, True, 0, device, stream_seeding=True),
                ResidentDataset(read_celeba_tfrec_array(te, H), batch_size, False, 1, device, stream_seeding=True), shape)
    return (StreamDataset(lambda: read_celeba_tfrec(tr, H), batch_size, True, SHUFFLE_BUFFER, 0, device),
            StreamDataset(lambda: read_celeba_tfrec(te, H), batch_size, False, SHUFFLE_BUFFER, 1, device), shape)
