"""GPU tests of the k-NN label probe: sv_knn_classify (csrc/knn.hip) against the float64 twin of tests/knn_ref.py -- exactly on
integer lattices, at the fp32 bound on Gaussian latents --, its invariances, the accumulator, split_vae_amd/probe.py on the three
models and the flags' surface in main.py / evaluate.py."""
import os

import numpy as np
import pytest
import torch

import knn_ref

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16


@pytest.fixture(scope="module")
def env(lib_built):
    assert torch.cuda.is_available()
    from split_vae_amd import _lib, ops, probe
    return ops, probe, _lib


def _dev(a, pad=0):
    """rows of `a` on the device, with `pad` unused floats behind every row (a row pitch above the width)"""
    a = np.ascontiguousarray(a, np.float32)
    if not pad:
        return torch.from_numpy(a).cuda()
    t = torch.full((a.shape[0], a.shape[1] + pad), 1e30, dtype=F32, device="cuda")       # the padding must never be read
    t[:, :a.shape[1]] = torch.from_numpy(a).cuda()
    return t[:, :a.shape[1]]


def _run(ops, q, r, rc, k, n_class, pad=0, **kw):
    pred, idx, dist = ops.knn_classify(_dev(q, pad), _dev(r, pad), torch.from_numpy(np.asarray(rc, np.uint8)).cuda(), k, n_class,
                                       want_neighbours=True, **kw)
    return idx.cpu().numpy(), dist.cpu().numpy(), pred.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ---------------------------------------------------------------- 1. exact on a lattice
# one sweep per axis around the base case (Nq 65, Nr 2 chunk + 7, L 37, k 5): Nr as a multiple m of the chunk plus a remainder
BASE = dict(Nq=65, Nr=(2, 7), L=37, k=5, pad=0, n_class=10, lo=-4, hi=4)
LATTICE = ([dict(Nq=v) for v in (1, 63, 64, 130)] + [dict(Nr=v) for v in ((0, 5), (0, 63), (0, 65), (1, 1))] +
           [dict(k=1), dict(k=32), dict(k=32, Nr=(0, 32))] + [dict(L=v) for v in (1, 3, 16, 128, 256)] +
           [dict(pad=3), dict(pad=3, L=16), dict(pad=1, L=128)] + [dict(n_class=2), dict(n_class=64)] +
           [dict(), dict(L=16, lo=-1, hi=1), dict(L=16, lo=-1, hi=1, Nq=130, k=32)])


@pytest.mark.parametrize("case", LATTICE, ids=lambda c: "-".join("%s%s" % (k, v) for k, v in c.items()).replace(" ", "") or "base")
def test_lattice_latents_match_the_twin_exactly(env, case):
    """Integer latents in [-4, 4] (and {-1, 0, 1}, where equal distances are the rule): every norm, dot product and distance is
    exactly representable in fp32 (max 2 * 256 * 64 < 2^24), so nn_index, nn_dist and pred equal the float64 twin EXACTLY, the
    index tie-break across tile and chunk boundaries included."""
    ops, _, _ = env
    c = dict(BASE, **case)
    chunk = ops.knn_chunk_rows()
    Nr = c["Nr"][0] * chunk + c["Nr"][1]
    rng = np.random.default_rng(1234 + c["Nq"] + 3 * Nr + 5 * c["L"] + 7 * c["k"])
    q = rng.integers(c["lo"], c["hi"] + 1, (c["Nq"], c["L"])).astype(np.float32)
    r = rng.integers(c["lo"], c["hi"] + 1, (Nr, c["L"])).astype(np.float32)
    rc = rng.integers(0, c["n_class"], Nr).astype(np.uint8)
    idx, dist, pred = _run(ops, q, r, rc, c["k"], c["n_class"], pad=c["pad"])
    widx, wdist, wpred, d = knn_ref.classify(q, r, rc, c["k"], c["n_class"])
    if c["hi"] == 1 and Nr > 64:                                # the tie case is one: equal distances inside the neighbour lists
        assert (np.diff(wdist, axis=1) == 0).mean() > 0.2
    assert np.array_equal(wdist.astype(np.float32).astype(np.float64), wdist)         # (the premise: exactly representable)
    assert np.array_equal(idx, widx)
    assert np.array_equal(dist.astype(np.float64), wdist)
    assert np.array_equal(pred, wpred)


# ---------------------------------------------------------------- 2. Gaussian latents against fp64
def _gaussian(Nr, Nq, L, seed):
    """Ten class centres ~ N(0, I), point i = centre (i mod 10) + N(0, I); the queries are drawn before the references.  (The
    draw order is part of the data: with this one the float64 twin ALONE, on the CPU, puts at most 1 query of a case under the
    1e-4 boundary gap over the twelve (case, seed) pairs below; other orders of the same draws give up to 3.)"""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((10, L))
    qc, rc = np.arange(Nq) % 10, np.arange(Nr) % 10
    q = (centres[qc] + rng.standard_normal((Nq, L))).astype(np.float32)
    r = (centres[rc] + rng.standard_normal((Nr, L))).astype(np.float32)
    return q, r, rc.astype(np.uint8), qc.astype(np.uint8)


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("Nr,Nq,L,k", [(600, 96, 128, 5), (333, 70, 16, 5), (1000, 130, 37, 10), (600, 96, 128, 1)])
def test_gaussian_latents_against_float64(env, Nr, Nq, L, k, seed):
    """Ten class centres ~ N(0, I), points = centre + N(0, I).  nn_dist against the twin's float64 distances at rtol 1e-5 (numpy's
    fp32 evaluation of the same formula reaches 1.7e-6; the margin is for the MFMA's summation order); the neighbour sets and pred
    equal the twin's for every query whose float64 relative gap at the k | k+1 boundary is >= 1e-4 (ten times the distance
    tolerance), and at most 2 queries per case fall under that gap."""
    ops, _, _ = env
    q, r, rc, _ = _gaussian(Nr, Nq, L, seed)
    idx, dist, pred = _run(ops, q, r, rc, k, 10)
    widx, wdist, wpred, d = knn_ref.classify(q, r, rc, k, 10)
    rel = np.abs(dist.astype(np.float64) - wdist) / wdist
    print("max relative distance error %.3g" % rel.max())
    np.testing.assert_allclose(dist.astype(np.float64), wdist, rtol=1e-5, atol=0)
    assert (np.diff(dist, axis=1) >= 0).all()
    keep = knn_ref.boundary_gap(d, k) >= 1e-4
    print("queries under the gap: %d of %d" % ((~keep).sum(), Nq))
    assert (~keep).sum() <= 2
    assert np.array_equal(np.sort(idx[keep], axis=1), np.sort(widx[keep], axis=1))
    assert np.array_equal(pred[keep], wpred[keep])
    assert (idx >= 0).all() and (idx < Nr).all() and all(len(set(row)) == k for row in idx.tolist())


# ---------------------------------------------------------------- 3. invariances that need no twin
@pytest.fixture(scope="module")
def cloud(env):
    ops = env[0]
    Nr = ops.knn_chunk_rows() + 100                              # two chunks
    q, r, rc, qc = _gaussian(Nr, 130, 37, 5)
    return q, r, rc, qc, _run(ops, q, r, rc, 5, 10)


def test_permuting_the_references_permutes_the_indices_only(env, cloud):
    ops = env[0]
    q, r, rc, _, (idx, dist, pred) = cloud
    perm = np.random.default_rng(9).permutation(r.shape[0])
    idx2, dist2, pred2 = _run(ops, q, r[perm], rc[perm], 5, 10)
    assert np.array_equal(_bits(dist2), _bits(dist))
    assert np.array_equal(perm[idx2], idx)                       # (tie-free: continuous data)
    assert np.array_equal(pred2, pred)


def test_a_subset_of_the_queries_gives_the_same_rows(env, cloud):
    ops = env[0]
    q, r, rc, _, (idx, dist, pred) = cloud
    idx2, dist2, pred2 = _run(ops, q[:65], r, rc, 5, 10)
    assert np.array_equal(idx2, idx[:65]) and np.array_equal(_bits(dist2), _bits(dist[:65])) and np.array_equal(pred2, pred[:65])
    idx3, dist3, pred3 = _run(ops, q[64:66], r[:70], rc[:70], 5, 10)    # another position in the tile, fewer references
    idx4, dist4, pred4 = _run(ops, q, r[:70], rc[:70], 5, 10)
    assert np.array_equal(idx3, idx4[64:66]) and np.array_equal(_bits(dist3), _bits(dist4[64:66])) and np.array_equal(pred3, pred4[64:66])


def test_two_runs_and_any_workspace_contents_give_the_same_bits(env, cloud):
    ops = env[0]
    q, r, rc, _, (idx, dist, pred) = cloud
    nbytes = ops.knn_workspace_bytes(q.shape[0], r.shape[0], 5)
    for fill in (None, 0x00, 0xFF):
        ws = None if fill is None else torch.full((nbytes,), fill, dtype=torch.uint8, device="cuda")
        idx2, dist2, pred2 = _run(ops, q, r, rc, 5, 10, workspace=ws)
        assert np.array_equal(idx2, idx) and np.array_equal(_bits(dist2), _bits(dist)) and np.array_equal(pred2, pred), fill


def test_a_query_equal_to_a_reference_finds_it_first(env, cloud):
    ops = env[0]
    _, r, rc, _, _ = cloud
    chunk = ops.knn_chunk_rows()
    rows = np.array([0, 63, 64, chunk - 1, chunk, r.shape[0] - 1])
    q = r[rows]
    idx, dist, pred = _run(ops, q, r, rc, 5, 10)
    assert np.array_equal(idx[:, 0], rows)
    assert (dist[:, 0] >= 0).all() and (dist[:, 0] <= 1e-5 * 2 * knn_ref.norms(q)).all()


# ---------------------------------------------------------------- 4. accumulator
def test_accumulator_adds_hits_and_counts(env, cloud):
    ops = env[0]
    q, r, rc, qc, (_, _, pred) = cloud
    dq, dr = _dev(q), _dev(r)
    drc, dqc = torch.from_numpy(rc).cuda(), torch.from_numpy(qc).cuda()
    one = torch.zeros(2, dtype=torch.int64, device="cuda")
    p1 = ops.knn_classify(dq, dr, drc, 5, 10, q_class=dqc, acc=one)
    assert np.array_equal(p1.cpu().numpy(), pred)
    hits = int((pred == qc).sum())
    assert one.tolist() == [hits, 130] and 0.5 < hits / 130                       # (clustered data: the probe finds the classes)
    assert one[0].item() / one[1].item() == float(np.mean(pred == qc))
    both = torch.tensor([1000, 7], dtype=torch.int64, device="cuda")               # ADDED to: not overwritten
    ops.knn_classify(dq[:70], dr, drc, 5, 10, q_class=dqc[:70], acc=both)
    ops.knn_classify(dq[70:], dr, drc, 5, 10, q_class=dqc[70:], acc=both)
    assert both.tolist() == [1000 + hits, 7 + 130]
    count_only = torch.zeros(2, dtype=torch.int64, device="cuda")
    ops.knn_classify(dq, dr, drc, 5, 10, acc=count_only)                           # no query classes: only the count moves
    assert count_only.tolist() == [0, 130]


def test_wrapper_refuses_what_the_kernel_cannot_read(env):
    ops = env[0]
    q, r = torch.zeros((4, 8), device="cuda"), torch.zeros((9, 8), device="cuda")
    rc = torch.zeros(9, dtype=torch.uint8, device="cuda")
    for bad in (lambda: ops.knn_classify(q.double(), r, rc, 3, 10), lambda: ops.knn_classify(q.cpu(), r, rc, 3, 10),
                lambda: ops.knn_classify(q.t(), r, rc, 3, 10), lambda: ops.knn_classify(q, r[:, :4], rc, 3, 10),
                lambda: ops.knn_classify(q, r, rc.int(), 3, 10), lambda: ops.knn_classify(q, r, rc[:8], 3, 10)):
        with pytest.raises(ValueError):
            bad()
    from split_vae_amd._lib import SplitVaeError
    with pytest.raises(SplitVaeError, match="SV_E_UNSUPPORTED"):
        ops.knn_classify(q, r, rc, 10, 10)                       # k > Nr


# ---------------------------------------------------------------- 5. / 6. the probe on the three models
H, LAT, NREF, NTEST = 32, 128, 150, 70


def _family(n, seed):
    """n images6 [n,32,32,6] on two one-parameter families -- x = (1 - t) a + t b, x_hat = (1 - s) c + s e -- and the class
    floor(10 t): the latent means lie along a curve, so a query's distances to the references are spread out and the k | k+1
    boundary is not a near-tie; the label follows x, not x_hat."""
    rng = np.random.default_rng(seed)
    a, b, c, e = (rng.uniform(-1, 1, (H, H, 3)) for _ in range(4))
    t, s = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    x = (1 - t)[:, None, None, None] * a + t[:, None, None, None] * b
    xh = (1 - s)[:, None, None, None] * c + s[:, None, None, None] * e
    cls = np.minimum((t * 10).astype(np.int64), 9)
    return np.concatenate([x, xh], axis=-1).astype(np.float32), cls


def _batches(images, cls, B=8):
    onehot = np.eye(10, dtype=np.float32)[cls]
    return [(torch.from_numpy(images[o:o + B]).cuda(), torch.from_numpy(onehot[o:o + B]).cuda()) for o in range(0, len(images), B)]


def _make(kind):
    from split_vae_amd.gm import LGGMVae
    from split_vae_amd.gmvae import GMVae
    from split_vae_amd.model import LGVae
    shape = (None, H, H, 3)
    if kind == "lgvae-f32":
        return LGVae(LAT, LAT, image_shape=shape, dtype="f32", seed=3)
    if kind == "lgvae-bf16":
        return LGVae(LAT, LAT, image_shape=shape, dtype="bf16", seed=3)
    if kind == "lggmvae":
        return LGGMVae(LAT, LAT, shape, 10, 0.4, dtype="f32", seed=3)
    return GMVae(LAT, shape, 10, 0.4, dtype="f32", seed=3)


MODELS = ["lgvae-f32", "lgvae-bf16", "lggmvae", "gmvae"]


@pytest.mark.parametrize("kind", MODELS)
def test_latent_means_are_the_models_own_means(env, deterministic, kind):
    """probe.latent_means over batches of 8, 8 and 4 images equals z_mean_x / z_mean_x_hat of the model's forward bit for bit, and
    leaves model._calls where it was.  (The mixture models' z_mean_x is computed behind the relaxed categorical sample y, which
    is drawn at the model's call counter: the forward it is compared with runs at the same counter.)"""
    _, probe, _ = env
    model = _make(kind)
    images, cls = _family(20, 11)
    batches = _batches(images, cls)
    assert [b[0].shape[0] for b in batches] == [8, 8, 4]
    model._calls = 5
    zg, zl = probe.latent_means(model, batches)
    assert model._calls == 5
    outs = []
    for b in batches:
        model._calls = 5
        outs.append(model(b[0]))
    assert zg.dtype == F32 and tuple(zg.shape) == (20, LAT) and torch.equal(zg, torch.cat([o[3] for o in outs]))
    if kind == "gmvae":
        assert zl is None
    else:
        assert zl.dtype == F32 and tuple(zl.shape) == (20, LAT) and torch.equal(zl, torch.cat([o[8] for o in outs]))
        assert not torch.equal(zl, zg)
    assert torch.isfinite(zg).all() and zg.std() > 0
    model._calls = 5
    zg2, _ = probe.latent_means(model, [b[0] for b in batches])          # bare image batches too
    assert torch.equal(zg2, zg)


@pytest.mark.parametrize("kind", MODELS)
def test_knn_probe_equals_the_twin_on_the_same_means(env, deterministic, kind):
    """150 references, 70 queries, k = 5, random weights: hits and count equal the twin's over the means the probe classified.
    The images lie on one-parameter families (_family), so no query sits at a near-tie of the k | k+1 boundary -- asserted; if a
    change of the models moves one there, change the seeds of _family below."""
    _, probe, _ = env
    model = _make(kind)
    images, cls = _family(NREF + NTEST, 21)                      # ONE pair of families: the queries lie on the references' curve
    ri, rcls, ti, tcls = images[:NREF], cls[:NREF], images[NREF:], cls[NREF:]
    refs, tests = _batches(ri, rcls), _batches(ti, tcls)
    calls = model._calls
    res = probe.knn_probe(model, refs, tests, 5)
    assert model._calls == calls
    assert (res["n_ref"], res["n_test"], res["k"]) == (NREF, NTEST, 5)
    rg, rl = probe.latent_means(model, refs)
    tg, tl = probe.latent_means(model, tests)
    for name, tq, rr in (("g", tg, rg), ("l", tl, rl)):
        if rr is None:
            assert kind == "gmvae" and res["acc_l"] is None and res["hits_l"] is None
            continue
        _, _, wpred, d = knn_ref.classify(tq.cpu().numpy(), rr.cpu().numpy(), rcls.astype(np.uint8), 5, 10)
        gap = knn_ref.boundary_gap(d, 5)
        print("%s z_%s: smallest boundary gap %.3g" % (kind, name, gap.min()))
        assert (gap >= 1e-4).all()
        hits = int((wpred == tcls).sum())
        assert res["hits_" + name] == hits and res["acc_" + name] == hits / NTEST
    assert res["acc_g"] > 0.3                                    # the label follows x: z_g finds it (chance: 0.1)


# ---------------------------------------------------------------- 7. CLI
def _write_svhn(root, n_train, n_extra, n_test, seed=0):
    import scipy.io
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, "SVHN"), exist_ok=True)
    for name, n in (("train", n_train), ("extra", n_extra), ("test", n_test)):
        X = rng.integers(0, 256, (32, 32, 3, n), dtype=np.uint8)
        y = rng.integers(1, 11, (n, 1)).astype(np.uint8)
        scipy.io.savemat(os.path.join(root, "SVHN", name + "_32x32.mat"), {"X": X, "y": y})


def _loss_lines(out):
    keep = ("Training step", "Recon Loss", "Total KL", "KLD loss", "KL loss", "Training done")
    return [l for l in out.splitlines() if any(k in l for k in keep)]


def _probe_lines(out):
    return [l for l in out.splitlines() if l.startswith("Test k-NN probe")]


CLI = ["--beta", "40", "--patch_size", "4", "--batch_size", "12", "--training_steps", "2", "--log_every", "1", "--dtype", "f32"]
PROBE = ["--knn_probe", "3", "--knn_refs", "40"]
NOTE = "classifier-based test metrics are not available"


def test_cli_prints_the_probe_line_and_evaluate_reproduces_it(env, deterministic, tmp_path, monkeypatch, capsys):
    """main on tiny .mat files: the probe line behind each of the three reports, the same on both input paths; every loss line as
    in the run without the flag; --knn_refs above the 39 training images is clipped with a note; evaluate --knn_probe on the saved
    weights prints the run's last line."""
    from split_vae_amd import evaluate, main as svmain
    _write_svhn(str(tmp_path / "data"), n_train=30, n_extra=9, n_test=27)
    monkeypatch.chdir(tmp_path)
    svmain.main(CLI)
    plain = capsys.readouterr().out
    assert not _probe_lines(plain) and "--knn_refs" not in plain and NOTE in plain
    path = svmain.main(CLI + PROBE)
    out = capsys.readouterr().out
    lines = _probe_lines(out)
    assert len(lines) == 3 and all(l.startswith("Test k-NN probe (k=3, 39 refs): z_g acc 0.") and ", z_l acc 0." in l for l in lines), out
    assert "--knn_refs 40 clipped" in out and NOTE in out and "Training done!" in out
    assert len(_loss_lines(plain)) >= 15 and _loss_lines(out) == _loss_lines(plain)
    keep = str(tmp_path / "kept") + os.path.splitext(path)[1]
    os.replace(path, keep)
    svmain.main(CLI + PROBE + ["--resident_data"])
    res_out = capsys.readouterr().out
    assert _probe_lines(res_out) == lines and _loss_lines(res_out) == _loss_lines(plain)
    res = evaluate.main(CLI + PROBE + ["--weights", keep])
    again = capsys.readouterr().out
    assert _probe_lines(again) == [lines[-1]] and "Test IW-" not in again
    assert "%.4f" % res["knn_acc_g"] in lines[-1]


def test_cli_gmvae_reports_z_g_only(env, deterministic, tmp_path, monkeypatch, capsys):
    from split_vae_amd import main as svmain
    _write_svhn(str(tmp_path / "data"), n_train=30, n_extra=9, n_test=27)
    monkeypatch.chdir(tmp_path)
    svmain.main(CLI[:-6] + ["--training_steps", "1", "--log_every", "1", "--dtype", "f32", "--model", "gmvae", "--y_size", "10"] + PROBE)
    out = capsys.readouterr().out
    lines = _probe_lines(out)
    assert len(lines) == 2 and all(l.startswith("Test k-NN probe (k=3, 39 refs): z_g acc 0.") and "z_l" not in l for l in lines), out
    assert "Classifier cluster acc" in out and "Training done!" in out


def test_cli_without_labels_skips_the_probe_and_trains(env, tmp_path, monkeypatch, capsys):
    from split_vae_amd import main as svmain
    monkeypatch.chdir(tmp_path)
    svmain.main(["--synthetic", "--batch_size", "8", "--training_steps", "1", "--log_every", "1"] + PROBE)
    out = capsys.readouterr().out
    assert out.count("Note: --knn_probe needs labels; skipped") == 1 and not _probe_lines(out) and "Training done!" in out
