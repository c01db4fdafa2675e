"""CPU: the host side of the device-resident datasets (data.ShuffleIndexStream, data.ResidentDataset's table and index check,
the argument checks of the three sv_dataset_* entries, the --resident_data flag).  No device work anywhere."""
import ctypes as C

import numpy as np
import pytest

CASES = [(0, 8), (7, 3), (8, 8), (5, 8), (1000, 64)]          # (n, buffer): empty, drain-only, n == buffer, n < buffer, fill + drain


@pytest.mark.parametrize("n,buffer", CASES)
@pytest.mark.parametrize("seed", [0, 5])
def test_shuffle_index_stream_equals_the_generators(n, buffer, seed):
    """Three epochs, element for element: ArrayDataset's order (_shuffled_indices, default_rng([seed, epoch])) and StreamDataset's
    (tfrecord.shuffle_buffer(range(n), buffer, seed + epoch)), consumed in chunks of 1, 5 or all at once."""
    from split_vae_amd import data
    from split_vae_amd.tfrecord import shuffle_buffer
    want_array = [i for e in range(3) for i in data._shuffled_indices(n, buffer, np.random.default_rng([seed, e]))]
    want_stream = [i for e in range(3) for i in shuffle_buffer(range(n), buffer, seed + e)]
    assert sorted(want_array) == sorted(list(range(n)) * 3)
    for stream_seeding, want in ((False, want_array), (True, want_stream)):
        for chunk in (1, 5, 3 * n):
            s = data.ShuffleIndexStream(n, buffer, seed, repeat=True, stream_seeding=stream_seeding)
            got = []
            while len(got) < 3 * n:
                part = s.take(chunk)
                assert part.dtype == np.int64 and len(part) == chunk          # a repeating stream never runs short
                got += part.tolist()
            assert got[:3 * n] == want, (stream_seeding, chunk)
        one = data.ShuffleIndexStream(n, buffer, seed, repeat=False, stream_seeding=stream_seeding)
        assert one.take(n + 9).tolist() == want[:n] and one.take(4).size == 0          # no repeat: the epoch, then nothing


def test_lut_is_the_float64_normalisation():
    from split_vae_amd import data
    lut = data.ResidentDataset.make_lut()
    want = data.normalise_u8(np.arange(256, dtype=np.uint8))
    assert lut.dtype == np.float32 and lut.shape == (256,) and lut.tobytes() == want.tobytes()
    assert lut.tobytes() == (np.arange(256) / 255.0 * 2 - 1).astype(np.float32).tobytes()


def _aligned(nbytes, off=0):
    """A host buffer and a 16-byte aligned address inside it (+ off): the entries only look at the pointer's value."""
    buf = (C.c_uint8 * (nbytes + 32))()
    a = (C.addressof(buf) + 15) & ~15
    return buf, C.c_void_p(a + off)


def test_dataset_entries_validate_arguments(lib_built):
    """SV_E_BADARG for null pointers, B <= 0 and a misaligned source; SV_E_UNSUPPORTED from the scramble entry for H != W or a
    patch that does not divide H.  Every call returns before anything is launched."""
    from split_vae_amd import _lib
    lib = _lib.load()
    BAD, UNS = _lib.STATUS_BADARG, _lib.STATUS_UNSUPPORTED
    keep, p = _aligned(64)
    _, odd = _aligned(64, 4)
    U8, F32 = _lib.SV_SRC_U8, _lib.SV_SRC_F32
    # gather(src, src_dtype, lut, index, x, N, B, H, W, stream)
    assert lib.sv_dataset_gather(None, U8, p, p, p, 9, 2, 32, 32, None) == BAD
    assert lib.sv_dataset_gather(p, U8, None, p, p, 9, 2, 32, 32, None) == BAD           # a uint8 source needs the table
    assert lib.sv_dataset_gather(p, U8, p, None, p, 9, 2, 32, 32, None) == BAD
    assert lib.sv_dataset_gather(p, U8, p, p, None, 9, 2, 32, 32, None) == BAD
    assert lib.sv_dataset_gather(p, F32, None, p, p, 9, 0, 32, 32, None) == BAD
    assert lib.sv_dataset_gather(p, F32, None, p, p, 9, -1, 32, 32, None) == BAD
    assert lib.sv_dataset_gather(p, F32, None, p, p, 0, 2, 32, 32, None) == BAD
    assert lib.sv_dataset_gather(p, 7, p, p, p, 9, 2, 32, 32, None) == BAD
    assert lib.sv_dataset_gather(odd, U8, p, p, p, 9, 2, 32, 32, None) == BAD
    assert lib.sv_dataset_gather(odd, F32, None, p, p, 9, 2, 32, 32, None) == BAD
    # gather_scramble(src, src_dtype, lut, index, perm, images6, x8, xh8, dtype, N, B, H, W, patch, stream)
    assert lib.sv_dataset_gather_scramble(None, U8, p, p, p, p, p, p, 0, 9, 2, 32, 32, 4, None) == BAD
    assert lib.sv_dataset_gather_scramble(p, U8, p, p, None, p, p, p, 0, 9, 2, 32, 32, 4, None) == BAD
    assert lib.sv_dataset_gather_scramble(p, U8, p, p, p, None, p, p, 0, 9, 2, 32, 32, 4, None) == BAD
    assert lib.sv_dataset_gather_scramble(p, U8, p, p, p, p, p, None, 0, 9, 2, 32, 32, 4, None) == BAD   # x8 without xh8
    assert lib.sv_dataset_gather_scramble(p, U8, p, p, p, p, p, p, 7, 9, 2, 32, 32, 4, None) == BAD
    assert lib.sv_dataset_gather_scramble(p, U8, p, p, p, p, p, p, 0, 9, 0, 32, 32, 4, None) == BAD
    assert lib.sv_dataset_gather_scramble(p, U8, p, p, p, p, p, p, 0, 9, 2, 32, 32, 0, None) == BAD
    assert lib.sv_dataset_gather_scramble(odd, F32, None, p, p, p, p, p, 1, 9, 2, 32, 32, 4, None) == BAD
    assert lib.sv_dataset_gather_scramble(p, F32, None, p, p, p, p, p, 1, 9, 2, 32, 64, 4, None) == UNS
    assert lib.sv_dataset_gather_scramble(p, U8, p, p, p, p, None, None, 0, 9, 2, 32, 32, 5, None) == UNS
    assert lib.sv_dataset_gather_scramble(p, U8, p, p, p, p, None, None, 0, 9, 2, 32, 32, 64, None) == UNS
    # onehot(labels, index, out, N, B, depth, stream)
    assert lib.sv_dataset_onehot(None, p, p, 9, 2, 10, None) == BAD
    assert lib.sv_dataset_onehot(p, None, p, 9, 2, 10, None) == BAD
    assert lib.sv_dataset_onehot(p, p, None, 9, 2, 10, None) == BAD
    assert lib.sv_dataset_onehot(p, p, p, 9, 0, 10, None) == BAD
    assert lib.sv_dataset_onehot(p, p, p, 9, 2, 0, None) == BAD
    del keep


def test_resident_dataset_refuses_an_index_outside_the_set():
    """The check runs on the host, before any upload (device="cpu": the set is only held, nothing is fetched)."""
    from split_vae_amd import data
    N = 11
    ds = data.ResidentDataset(np.zeros((N, 32, 32, 3), np.uint8), 4, False, device="cpu")
    assert ds.upload_index([0, N - 1, 3]).tolist() == [0, N - 1, 3]
    for bad in ([0, N], [-1, 2], np.array([5, 2 ** 31 + 1])):
        with pytest.raises(ValueError):
            ds.upload_index(bad)
    with pytest.raises(ValueError):
        data.ResidentDataset(np.zeros((N, 32, 32, 3), np.float64), 4, False, device="cpu")
    with pytest.raises(ValueError):
        data.ResidentDataset(np.zeros((N, 32, 32, 3), np.uint8), 4, False, device="cpu", labels=np.ones(N - 1, np.uint8))


def test_cli_knows_resident_data():
    from split_vae_amd.main import build_parser
    ap = build_parser()
    assert ap.parse_args([]).resident_data is False
    assert ap.parse_args(["--resident_data"]).resident_data is True
