"""GPU tests of the linear label probe: sv_linprobe_gram / sv_linprobe_fit / sv_linprobe_predict (csrc/linprobe.hip) against the
float64 twin of tests/linprobe_ref.py -- bit for bit on integer lattices, by the derived bounds on Gaussian clusters --, the
repeatability and resume rules, the edge shapes with the extents written, split_vae_amd/linear_probe.py on two models and its
command line."""
import numpy as np
import pytest
import torch

import linprobe_ref as lr

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
SENT = -7.25e30                                 # what every output holds before a call
WORST = {}                                      # worst device error over bound seen by this run (printed per test)


@pytest.fixture(scope="module")
def env(lib_built):
    assert torch.cuda.is_available()
    from split_vae_amd import _lib, linear_probe, ops
    assert ops.linprobe_chunk_rows() == lr.CHUNK
    return ops, linear_probe, _lib


def _dev(a, pad=0):
    """rows of `a` on the device with `pad` NaN floats behind every row: the padding must never be read into a result"""
    a = np.ascontiguousarray(a, np.float32)
    N, L = a.shape
    flat = torch.full((N * (L + pad) + 4,), float("nan"), dtype=F32, device="cuda")
    t = flat[:N * (L + pad)].view(N, L + pad)
    t[:, :L] = torch.from_numpy(a).cuda()
    return t[:, :L]


def _workspace(ops, N, L, C):
    """a workspace full of 0xff bytes: NaN as fp32 and as fp64"""
    return torch.full((ops.linprobe_workspace_bytes(N, L, C),), 255, dtype=torch.uint8, device="cuda")


def _guarded(shape, dtype):
    """(a sentinel-filled buffer with two guard elements on either side, its inner view)"""
    n = int(np.prod(shape))
    big = torch.full((n + 4,), SENT if dtype.is_floating_point else -77, dtype=dtype, device="cuda")
    return big, big[2:2 + n].view(*shape)


def _guards_intact(big):
    v = big.cpu().numpy()
    s = SENT if big.dtype.is_floating_point else -77
    return v[0] == s and v[1] == s and v[-1] == s and v[-2] == s


def device_gram(ops, x, pad=0):
    xd = x if torch.is_tensor(x) else _dev(x, pad)
    return ops.linprobe_gram(xd, workspace=_workspace(ops, xd.shape[0], xd.shape[1], 2)).cpu().numpy()


def device_fit(ops, x, y, C, P, l2, T, W0=None, groups=None, pad=0):
    """sv_linprobe_fit from W0 (zeros), the steps enqueued in `groups` (default: all at once) -> the twin's dict; every output sits
    between guard elements and starts as the sentinel"""
    xd = x if torch.is_tensor(x) else _dev(x, pad)
    N, L = xd.shape
    yd = torch.from_numpy(np.ascontiguousarray(y, np.uint8)).cuda()
    Pd = torch.from_numpy(np.ascontiguousarray(P, np.float64)).cuda()
    bufs = {n: _guarded(s, d) for n, s, d in (("W", (L + 1, C), F64), ("loss", (T + 1,), F64), ("gmax", (T + 1,), F64), ("grad", (L + 1, C), F64),
                                              ("state", (1,), torch.int32))}
    fit = {n: b[1] for n, b in bufs.items()}
    fit["W"].copy_(torch.from_numpy(np.zeros((L + 1, C)) if W0 is None else np.ascontiguousarray(W0, np.float64)).cuda())
    ws = _workspace(ops, N, L, C)
    groups = [T] if groups is None else groups
    assert sum(groups) == T
    for i, g in enumerate(groups):
        ops.linprobe_fit(xd, yd, Pd, fit, g, l2, resume=i > 0, workspace=ws)
    out = dict(W=fit["W"].cpu().numpy(), loss=fit["loss"].cpu().numpy(), gmax=fit["gmax"].cpu().numpy(), G=fit["grad"].cpu().numpy(),
               state=int(fit["state"].item()))
    assert all(_guards_intact(b[0]) for b in bufs.values())
    assert out["state"] == T + 1
    return out


def device_predict(ops, q, W, C, q_class, start=(5, 7), pad=0):
    qd = q if torch.is_tensor(q) else _dev(q, pad)
    Wd = torch.from_numpy(np.ascontiguousarray(W, np.float64)).cuda()
    qc = None if q_class is None else torch.from_numpy(np.ascontiguousarray(q_class, np.uint8)).cuda()
    acc_big, acc = _guarded((2,), torch.int64)
    acc.copy_(torch.tensor(start, dtype=torch.int64))
    ws = _workspace(ops, qd.shape[0], qd.shape[1], C)
    if qc is None:
        pred, loss = ops.linprobe_predict(qd, Wd, acc=acc, workspace=ws), None
    else:
        pred, loss = ops.linprobe_predict(qd, Wd, q_class=qc, acc=acc, want_loss=True, workspace=ws)
    a = acc.cpu().numpy()
    assert a[1] == start[1] + qd.shape[0]                         # acc is added to
    v = acc_big.cpu().numpy()
    assert v[0] == v[1] == v[-1] == v[-2]
    return dict(pred=pred.cpu().numpy(), hits=int(a[0] - start[0]), loss=None if loss is None else float(loss.item()))


def run_on_device(ops, case):
    k = case["kind"]
    if k == "gram":
        return dict(S=device_gram(ops, case["x"]))
    if k == "first":
        return device_fit(ops, case["x"], case["y"], case["C"], np.eye(case["x"].shape[1] + 1), case["l2"], 0, W0=case.get("W0"))
    if k == "fit":
        return device_fit(ops, case["x"], case["y"], case["C"], lr.case_P(case)[0], case["l2"], case["T"])
    return device_predict(ops, case["x"], lr.predict_weights(case), case["C"], case["y"])


def _note(name, got, want, bounds):
    for n in ("W", "loss", "gmax", "G"):
        r = float((np.abs(np.asarray(got[n]) - np.asarray(want[n])) / bounds[n]).max())
        WORST[n] = max(WORST.get(n, 0.0), r)
        print("%s %s: worst error %.3g, error / bound %.3g (run worst %.3g)" % (name, n, np.abs(np.asarray(got[n]) - np.asarray(want[n])).max(), r, WORST[n]))


# ---------------------------------------------------------------- 1. the shared cases
CASES = lr.cases()


@pytest.fixture(scope="module")
def twin_results():
    return {c["name"]: lr.run_case(c) for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_shared_cases_match_the_twin(env, twin_results, case):
    """gram: integer lattices with |x| <= 8 (every fp32 partial sum is exact) and the fold trap (2^53 + 1 + 1 over three chunks: the
    fp64 fold shows its order) -- S equals the twin's bits and its own transpose.  first: integer x against W = 0 (or equal
    columns), C in {2, 4, 8}, so p = 1 / C is exact: G, loss_0, gmax_0 bit for bit.  fit: Gaussian clusters, W / loss / gmax / G after
    T in {1, 3, 50} steps within the derived bounds, the loss monotone up to them.  predict: the argmax outside the margin, the
    hits, the loss.  The comparison is the one that rejects the wrong kernels of tests/test_linprobe_host.py."""
    ops = env[0]
    want = twin_results[case["name"]]
    bounds = None
    if case["kind"] == "fit":
        P, B = lr.case_P(case)
        bounds = lr.fit_bounds(case["x"], case["y"], case["C"], P, B, case["l2"], want)
        assert bounds["EB"] <= (case["T"] + 1) * max(lr.pass_bounds(case["x"], case["y"], case["C"], p, p["W"], P, B, case["l2"])["beta"]
                                                      for p in want["passes"])        # at most linear in T
    got = run_on_device(ops, case)
    if bounds is not None:
        _note(case["name"], got, want, bounds)
    if case["kind"] == "predict":
        print("%s: %d rows excluded, loss error %.3g of bound %.3g" % (case["name"], lr.predict_excluded(case, want).sum(),
                                                                       abs(got["loss"] - want["loss"]), lr.predict_loss_bound(case, want)))
    assert lr.compare(case, got, want, bounds) == []


def test_gram_of_gaussian_rows_is_within_the_chain_bound(env):
    """|S~ - S| <= (CHUNK + 1) u |A|^T |A|: one rounding per row of a chunk's fp32 chain; symmetric bit for bit on any data"""
    ops = env[0]
    x, _ = lr.gauss(1500, 37, 4)
    got = device_gram(ops, x, pad=3)
    a = np.abs(lr.design(x))
    err = np.abs(got - lr.gram(x))
    bound = (lr.CHUNK + 1) * lr.U * (a.T @ a)
    print("gram: worst error / bound %.3g" % (err / bound).max())
    assert (err <= bound).all() and np.array_equal(got, got.T)


# ---------------------------------------------------------------- 2. repeatability, resume, row order
def _gauss_case():
    return [c for c in CASES if c["name"] == "n-700-130-3-T3"][0]


def test_same_call_same_bits_and_resume_gives_the_bits_of_one_call(env):
    ops = env[0]
    c = _gauss_case()
    P = lr.case_P(c)[0]
    a = device_fit(ops, c["x"], c["y"], c["C"], P, c["l2"], 5)
    b = device_fit(ops, c["x"], c["y"], c["C"], P, c["l2"], 5)
    s = device_fit(ops, c["x"], c["y"], c["C"], P, c["l2"], 5, groups=[2, 3])
    z = device_fit(ops, c["x"], c["y"], c["C"], P, c["l2"], 5, groups=[0, 2, 0, 3])
    for other in (b, s, z):
        for n in ("W", "loss", "gmax", "G"):
            assert np.array_equal(a[n].view(np.int64), other[n].view(np.int64)), n
    g1, g2 = device_gram(ops, c["x"]), device_gram(ops, c["x"])
    assert np.array_equal(g1.view(np.int64), g2.view(np.int64))


def test_rows_permuted_inside_a_chunk(env):
    """What a permutation of the rows inside one chunk leaves alone.  On any data: a row's logits do not depend on where the row
    sits, so pred follows its row exactly.  On lattice data against W = 0, where every fp32 partial sum of a chunk is exact and
    every loss_i is the same fp32 number (sums of up to 64 and of N copies of it are exact in fp64): S, G, loss_0 and gmax_0 keep
    their bits.  Nothing more is promised: on general data the fp32 chain of a chunk follows the row order."""
    ops = env[0]
    first = [c for c in CASES if c["name"] == "f-1100-33-2"][0]
    x, y, C = first["x"], first["y"].copy(), first["C"]
    y[y >= C] = 0                                                 # every row valid: every loss_i equal
    rng = np.random.default_rng(3)
    perm = np.arange(x.shape[0])
    perm[:lr.CHUNK] = rng.permutation(lr.CHUNK)
    perm[lr.CHUNK:2 * lr.CHUNK] = lr.CHUNK + rng.permutation(lr.CHUNK)
    eye = np.eye(x.shape[1] + 1)
    a, b = device_fit(ops, x, y, C, eye, 0.0, 0), device_fit(ops, x[perm], y[perm], C, eye, 0.0, 0)
    for n in ("G", "loss", "gmax"):
        assert np.array_equal(a[n].view(np.int64), b[n].view(np.int64)), n
    assert np.array_equal(device_gram(ops, x).view(np.int64), device_gram(ops, x[perm]).view(np.int64))
    c = [c for c in CASES if c["name"] == "n-700-130-3-predict"][0]
    W = lr.predict_weights(c)
    perm = np.arange(700)
    perm[:lr.CHUNK] = rng.permutation(lr.CHUNK)
    p0 = device_predict(ops, c["x"], W, c["C"], c["y"])
    p1 = device_predict(ops, c["x"][perm], W, c["C"], c["y"][perm])
    assert np.array_equal(p0["pred"][perm], p1["pred"]) and p0["hits"] == p1["hits"]


def test_predict_without_classes_adds_only_the_count(env):
    ops = env[0]
    c = [c for c in CASES if c["name"] == "p-ties"][0]
    W = lr.predict_weights(c)
    with_classes = device_predict(ops, c["x"], W, c["C"], c["y"])
    bare = device_predict(ops, c["x"], W, c["C"], None)           # asserts the count inside
    assert bare["hits"] == 0 and bare["loss"] is None and np.array_equal(bare["pred"], with_classes["pred"])
    assert (with_classes["pred"] == 0).all()                      # every logit ties: the lower class


# ---------------------------------------------------------------- 3. edge shapes
def _shapes():
    ch = lr.CHUNK
    base = dict(N=65, L=5, C=3, pad=0)
    sweep = ([dict(N=v) for v in (1, 2, 63, 64, ch - 1, ch, ch + 1, 2 * ch + 3)] + [dict(L=v) for v in (1, 3, 4, 16, 17, 128, 512)] +
             [dict(C=v) for v in (2, 10, 63, 64)] + [dict(pad=3), dict(pad=1, L=16), dict(pad=5, L=17, N=ch + 1)] +
             [dict(N=2 * ch + 3, L=17, C=10), dict(N=ch + 1, L=128, C=64), dict(N=64, L=512, C=63), dict(N=1, L=1, C=2), dict(N=63, L=4, C=64),
              dict(N=ch, L=16, C=2, pad=4), dict(N=2, L=3, C=10, pad=1)])
    return [dict(base, **s) for s in [{}] + sweep]


@pytest.mark.parametrize("c", _shapes(), ids=lambda c: "N%d-L%d-C%d-p%d" % (c["N"], c["L"], c["C"], c["pad"]))
def test_edge_shapes(env, c):
    """One sweep per axis around (65, 5, 3): N around the 64-row tile and the chunk, L around the 4-wide MFMA step, the 16-wide
    K step and the 16-feature fragment and at 512, C over the four fragment counts, row pitches above L with NaN in the padding,
    one row of a class >= C, a workspace full of NaN, outputs full of a sentinel between guard elements.  Integer lattice rows:
    S bit for bit; a fit of two steps from W = 0 within the derived bounds (loss_0 and gmax_0 bit for bit where C is a power of
    two); predict on the fitted W."""
    ops = env[0]
    N, L, C = c["N"], c["L"], c["C"]
    x = lr.lattice(N, L, 11 + N + L)
    y = lr.labels(N, C, N + C, invalid=1 if N >= 3 else 0)
    xd = _dev(x, c["pad"])
    S = device_gram(ops, xd)
    assert np.array_equal(S.view(np.int64), lr.gram(x).view(np.int64))
    l2 = 1e-2
    P, B = lr.make_P(lr.gram(x), N, l2)
    want = lr.fit(x, y, C, P, l2, 2, keep=True)
    bounds = lr.fit_bounds(x, y, C, P, B, l2, want)
    got = device_fit(ops, xd, y, C, P, l2, 2)
    case = dict(kind="fit", x=x, y=y, C=C)
    _note("edge", got, want, bounds)
    assert lr.compare(case, got, want, bounds) == []
    if C & (C - 1) == 0:
        exact = lr.evaluate(x, y, C, np.zeros((L + 1, C)), l2, emulate=True)
        assert got["loss"][0] == exact["loss"] and got["gmax"][0] == exact["gmax"]
    pcase = dict(kind="predict", x=x, y=y, C=C, T=None)
    W = got["W"]
    pwant = lr.predict(x, W, C, y)
    pgot = device_predict(ops, xd, W, C, y)
    margin = np.sort(pwant["z"], axis=1)
    keep = (margin[:, -1] - margin[:, -2]) >= 2 * lr.logit_bound(x, W)
    assert np.array_equal(pgot["pred"][keep], pwant["pred"][keep])
    qc = y.astype(np.int64)
    assert pgot["hits"] == int(((pgot["pred"] == qc) & (qc < C)).sum())
    _, loss_i, _ = lr.softmax_parts(pwant["z"], y, C)
    D = pwant["z"].max(axis=1) - pwant["z"].min(axis=1)
    lb = float((2 * lr.logit_bound(x, W) + lr.U * (2 * C + 4 + 2 * np.log(C) + 2 * D + np.abs(loss_i))).mean()) + 1e-13
    assert abs(pgot["loss"] - pwant["loss"]) <= lb
    assert not torch.isnan(xd).any()                              # the input is untouched (its padding is not part of the view)


def test_wrappers_refuse_what_the_kernels_cannot_read(env):
    ops, _, _lib = env
    x = torch.zeros((20, 8), device="cuda")
    y = torch.zeros((20,), dtype=torch.uint8, device="cuda")
    P = torch.eye(9, dtype=F64, device="cuda")
    for bad in (lambda: ops.linprobe_gram(x.double()), lambda: ops.linprobe_gram(x.t()), lambda: ops.linprobe_gram(x.cpu()),
                lambda: ops.linprobe_fit(x, y.int(), P, ops.linprobe_state(x, 3, 2), 2, 1e-3),
                lambda: ops.linprobe_fit(x, y, P.float(), ops.linprobe_state(x, 3, 2), 2, 1e-3),
                lambda: ops.linprobe_fit(x, y, P[:8, :8].contiguous(), ops.linprobe_state(x, 3, 2), 2, 1e-3),
                lambda: ops.linprobe_predict(x, torch.zeros((8, 3), dtype=F64, device="cuda")),
                lambda: ops.linprobe_predict(x, torch.zeros((9, 3), dtype=F64, device="cuda"), acc=torch.zeros(2, dtype=torch.int32, device="cuda"))):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(_lib.SplitVaeError, match="SV_E_UNSUPPORTED"):
        ops.linprobe_fit(x, y, P, ops.linprobe_state(x, 65, 2), 2, 1e-3)      # C > 64
    with pytest.raises(_lib.SplitVaeError, match="SV_E_UNSUPPORTED"):
        ops.linprobe_fit(x, y, P, ops.linprobe_state(x, 3, 2), 2, float("inf"))


# ---------------------------------------------------------------- 4. the report on two models
H, LAT, NCLS = 32, 128, 4


def _labelled_images(n, seed):
    """images6 [n,32,32,6] whose class sets a visible global feature (the mean colour of x) on top of a shared texture; x_hat is noise"""
    rng = np.random.default_rng(seed)
    cls = rng.integers(0, NCLS, n)
    tone = np.linspace(-0.8, 0.8, NCLS)[cls]
    x = 0.15 * rng.uniform(-1, 1, (n, H, H, 3)) + tone[:, None, None, None]
    xh = rng.uniform(-1, 1, (n, H, H, 3))
    return np.concatenate([x, xh], axis=-1).astype(np.float32), cls


def _batches(images, cls, B=8):
    onehot = np.eye(NCLS, dtype=np.float32)[cls]
    return [(torch.from_numpy(images[o:o + B]).cuda(), torch.from_numpy(onehot[o:o + B]).cuda()) for o in range(0, len(images), B)]


def _make(kind):
    from split_vae_amd.gmvae import GMVae
    from split_vae_amd.model import LGVae
    shape = (None, H, H, 3)
    return LGVae(LAT, LAT, image_shape=shape, dtype="f32", seed=3) if kind == "lgvae" else GMVae(LAT, shape, 10, 0.4, dtype="f32", seed=3)


@pytest.mark.parametrize("kind", ["lgvae", "gmvae"])
def test_evaluate_on_a_tiny_model(env, deterministic, kind):
    """Random weights, 48 labelled reference images and 24 test images of 4 classes that set the mean colour: the keys and Nones as
    specified, acc_g the recomputation from pred, the report's fit the twin's fit on the same latent means within its bounds."""
    from split_vae_amd.probe import latent_means
    ops, lp, _ = env
    model = _make(kind)
    ri, rc = _labelled_images(48, 5)
    ti, tc = _labelled_images(24, 6)
    refs, tests = _batches(ri, rc), _batches(ti, tc)
    res = lp.evaluate(model, refs, tests, iters=20, l2=1e-2)
    assert (res["n_ref"], res["n_test"], res["iters"], res["l2"]) == (48, 24, 20, 1e-2)
    keys = ["acc_", "train_acc_", "loss_", "test_loss_", "gmax_"]
    assert all(isinstance(res[k + "g"], float) for k in keys)
    if kind == "gmvae":
        assert all(res[k + "l"] is None for k in keys)
    else:
        assert all(isinstance(res[k + "l"], float) for k in keys) and 0.0 <= res["acc_l"] <= 1.0
    pred = res["pred_g"].cpu().numpy()
    assert res["acc_g"] == float((pred == tc).sum()) / 24 == res["hits_g"] / 24
    zg = latent_means(model, refs)[0].cpu().numpy()
    P, B = lr.make_P(lr.gram(zg), 48, 1e-2)
    want = lr.fit(zg, rc.astype(np.uint8), NCLS, P, 1e-2, 20, keep=True)
    bounds = lr.fit_bounds(zg, rc.astype(np.uint8), NCLS, P, B, 1e-2, want)
    assert abs(res["loss_g"] - want["loss"][-1]) <= bounds["loss"][-1] and abs(res["gmax_g"] - want["gmax"][-1]) <= bounds["gmax"][-1]
    assert want["loss"][-1] < want["loss"][0]
    line = lp.report_line(res)
    assert line.startswith("Test linear probe (48 refs, 20 steps, l2 0.01): z_g acc ") and ("; z_l acc " in line) == (kind != "gmvae")
    assert "%.4f" % res["acc_g"] in line and "train acc %.4f" % res["train_acc_g"] in line


def test_fit_refuses_a_singular_bound(env):
    ops, lp, _ = env
    x = torch.ones((40, 3), device="cuda")                        # constant columns, l2 = 0: B is singular
    y = torch.zeros((40,), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="positive definite"):
        lp.fit(x, y, 2, iters=3, l2=0.0)
    f = lp.fit(x, y, 2, iters=3, l2=1e-2)
    assert f["loss"].shape == (4,) and (np.diff(f["loss"]) <= 0).all() and f["W"].shape == (4, 2)


def test_cli_prints_the_note_on_synthetic_data(env, tmp_path, monkeypatch, capsys):
    """--synthetic has no labels: one note, no fit on the device, an empty result."""
    ops, lp, _ = env
    from split_vae_amd.main import build_parser, make_model
    from split_vae_amd.utils import dotdict
    monkeypatch.chdir(tmp_path)
    flags = ["--synthetic", "--batch_size", "8", "--dtype", "f32"]
    config = dotdict(vars(build_parser().parse_args(flags)))
    model, _ = make_model("lgvae", config, (None, 32, 32, 3))
    path = str(tmp_path / "w.npz")
    model.save_weights(path)
    capsys.readouterr()

    def boom(*a, **k):
        raise AssertionError("a device fit without labels")
    for name in ("linprobe_gram", "linprobe_fit", "linprobe_predict"):
        monkeypatch.setattr(ops, name, boom)
    res = lp.main(flags + ["--weights", path, "--probe_refs", "16", "--probe_iters", "3"])
    out = capsys.readouterr().out
    assert res == {} and out.count(lp.NO_LABELS) == 1 and "Test linear probe" not in out
