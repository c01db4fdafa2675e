"""GPU: the sample-quality report (sv_prdc_radius / sv_prdc_count, split_vae_amd/sample_quality.py) against the float64 twins of
tests/prdc_ref.py: counts, minima and radii bit for bit on integer lattices and inside derived brackets on Gaussian data, the wrappers'
refusals, and sample_quality.evaluate against a composition of existing pieces on three models."""
import numpy as np
import pytest
import torch

import prdc_ref as ref
import swap_ref

pytestmark = pytest.mark.gpu

F32, I32 = torch.float32, torch.int32
SENTINEL = -77777
WORST = {"rad": 0.0, "dmin": 0.0}                  # worst device error / bound over the Gaussian cases (printed)


@pytest.fixture(scope="module")
def env(lib_built):
    assert torch.cuda.is_available()
    from split_vae_amd import _lib, ops, sample_quality
    return ops, sample_quality, _lib


def _strided(a, pad, off):
    """the rows of a [N, L] in a NaN-filled buffer with row pitch L + pad that starts `off` floats behind the allocation"""
    N, L = a.shape
    buf = torch.full((off + N * (L + pad),), float("nan"), dtype=F32, device="cuda")
    view = buf[off:].view(N, L + pad)[:, :L]
    view.copy_(torch.from_numpy(np.ascontiguousarray(a, np.float32)))
    assert view.stride(0) == L + pad and view.data_ptr() == buf.data_ptr() + 4 * off
    return view


def _guarded(n, dtype):
    """[n + 2] sentinels: the output is the middle"""
    return torch.full((n + 2,), SENTINEL, dtype=dtype, device="cuda")


def _count(ops, Q, R, rad, pads=(0, 0, 0)):
    """sv_prdc_count on a case: sentinel-filled outputs with a guard either side, a workspace of NaN bit patterns with a guard behind it,
    the call twice (the same bits), and once without the minima (the same counts)"""
    pq, pr, off = pads
    q, r = _strided(Q, pq, off), _strided(R, pr, off)
    Nq, L = Q.shape
    Nr = R.shape[0]
    radd = torch.from_numpy(np.ascontiguousarray(rad, np.float32)).cuda()
    c, d, i = _guarded(Nq, I32), _guarded(Nq, F32), _guarded(Nq, I32)
    nbytes = ops.prdc_workspace_bytes(Nq, Nr, L, 1)
    ws = torch.full((nbytes + 256,), 0xFF, dtype=torch.uint8, device="cuda")
    out = ops.prdc_count(q, r, radd, cnt=c[1:Nq + 1], dmin=d[1:Nq + 1], imin=i[1:Nq + 1], workspace=ws[:nbytes])
    first = [t.clone() for t in out]
    torch.cuda.synchronize()
    for g in (c, d, i):
        assert g[0] == SENTINEL and g[Nq + 1] == SENTINEL
    assert (ws[nbytes:] == 0xFF).all()
    ops.prdc_count(q, r, radd, cnt=c[1:Nq + 1], dmin=d[1:Nq + 1], imin=i[1:Nq + 1], workspace=ws[:nbytes])      # the workspace now holds partials
    assert all(torch.equal(a.view(I32), b.view(I32)) for a, b in zip(first, out))
    assert torch.equal(ops.prdc_count(q, r, radd, want_min=False), first[0])
    return tuple(t.cpu().numpy() for t in first)


def _radius(ops, X, k, pad=0, off=0):
    x = _strided(X, pad, off)
    N, L = X.shape
    g = _guarded(N, F32)
    nbytes = ops.prdc_workspace_bytes(N, N, L, k)
    ws = torch.full((nbytes + 256,), 0xFF, dtype=torch.uint8, device="cuda")
    out = ops.prdc_radius(x, k, rad=g[1:N + 1], workspace=ws[:nbytes])
    first = out.clone()
    torch.cuda.synchronize()
    assert g[0] == SENTINEL and g[N + 1] == SENTINEL and (ws[nbytes:] == 0xFF).all()
    ops.prdc_radius(x, k, rad=g[1:N + 1], workspace=ws[:nbytes])
    assert torch.equal(first.view(I32), out.view(I32))
    return first.cpu().numpy()


# ---------------------------------------------------------------- 1. integer lattices: bit for bit
@pytest.mark.parametrize("index", range(9))
def test_counts_on_integer_lattices_bit_for_bit(env, index):
    ops = env[0]
    shapes = ref.count_shapes(ops.prdc_chunk_rows())
    assert len(shapes) == 9
    Nq, Nr, L, pq, pr, off = shapes[index]
    c = ref.count_case(Nq, Nr, L, 200 + index)
    want = ref.count(c["Q"], c["R"], c["rad"])
    got = _count(ops, c["Q"], c["R"], c["rad"], (pq, pr, off))
    print("lattice Nq %d Nr %d L %d: counts %d .. %d, differing cnt %d dmin %d imin %d" %
          ((Nq, Nr, L, want[0].min(), want[0].max()) + tuple(int((g.astype(np.float64) != w).sum()) for g, w in zip(got, want))))
    assert got[0].dtype == np.int32 and got[1].dtype == np.float32 and got[2].dtype == np.int32
    assert ref.counts_equal(got, want)


@pytest.mark.parametrize("index", range(12))
def test_radii_on_integer_lattices_bit_for_bit(env, index):
    ops = env[0]
    shapes = ref.radius_shapes(ops.prdc_chunk_rows())
    assert len(shapes) == 12
    N, L, k, pad, off = shapes[index]
    X = ref.radius_case(N, L, 300 + index)
    want = ref.radius(X, k)
    got = _radius(ops, X, k, pad, off)
    print("lattice N %d L %d k %d: radii %g .. %g, zeros %d, differing %d" % (N, L, k, want.min(), want.max(), int((want == 0).sum()), int((got != want).sum())))
    assert got.dtype == np.float32 and ref.exact(got, want)


def test_fake_equal_to_real_on_a_lattice_gives_ones(env):
    """Y = X: every row lies in its own ball (d = 0 <= rad), so precision = recall = coverage = 1, whatever the ties"""
    ops, sq, _ = env
    X = ref.radius_case(200, 33, 77)
    x = torch.from_numpy(np.ascontiguousarray(X)).cuda()
    rad = ops.prdc_radius(x, 5)
    cnt, dmin, imin = ops.prdc_count(x, x, rad)
    fig = sq.figures(cnt.cpu().numpy(), cnt.cpu().numpy(), dmin.cpu().numpy(), rad.cpu().numpy(), 5)
    assert fig["precision"] == fig["recall"] == fig["coverage"] == 1.0 and fig["density"] >= 1.0
    assert (dmin == 0).all() and (imin.cpu().numpy() <= np.arange(200)).all()
    want = ref.count(X, X, rad.cpu().numpy())
    assert ref.counts_equal((cnt.cpu().numpy(), dmin.cpu().numpy(), imin.cpu().numpy()), want)


# ---------------------------------------------------------------- 2. Gaussian data: inside the derived brackets
@pytest.mark.parametrize("shape", ref.GAUSS_SHAPES)
def test_gaussian_data_inside_the_derived_brackets(env, shape):
    """cnt inside [lo, hi] and equal to the twin wherever lo == hi (the same fp32 radii on both sides); dmin and the radii within the
    row's largest per-pair bound of the twin (an order statistic is 1-Lipschitz in the sup norm); imin names a row within twice that of
    the minimum"""
    ops = env[0]
    c = ref.gaussian_case(*shape)
    Q, R, rad, k = c["Q"], c["R"], c["rad"], c["k"]
    lo, hi = ref.count_bracket(Q, R, rad)
    want = ref.count(Q, R, rad)
    cnt, dmin, imin = _count(ops, Q, R, rad)
    eps_q = ref.pair_eps(Q, R).max(axis=1)
    WORST["dmin"] = max(WORST["dmin"], float((np.abs(dmin - want[1]) / eps_q).max()))
    print("gaussian %s: undecided %.4f, positive share %.3f, outside the bracket %d, off the twin %d, worst |dmin - twin| / bound %.3f" %
          (shape, ref.undecided_share(lo, hi), float(np.mean(want[0] > 0)), int(((cnt < lo) | (cnt > hi)).sum()), int((cnt != want[0]).sum()),
           float((np.abs(dmin - want[1]) / eps_q).max())))
    assert ref.undecided_share(lo, hi) <= ref.UNDECIDED_CAP
    assert ref.counts_in_bracket(cnt, lo, hi, want[0])
    assert ref.within(dmin, want[1], eps_q)
    assert ref.nearest_ok(Q, R, imin, want[1])
    got_rad = _radius(ops, R, k)
    eps_r = ref.pair_eps(R, R).max(axis=1)
    twin_rad = ref.radius(R, k)
    WORST["rad"] = max(WORST["rad"], float((np.abs(got_rad - twin_rad) / eps_r).max()))
    print("gaussian %s: worst |rad - twin| / bound %.3f (so far: rad %.3f, dmin %.3f)" %
          (shape, float((np.abs(got_rad - twin_rad) / eps_r).max()), WORST["rad"], WORST["dmin"]))
    assert ref.within(got_rad, twin_rad, eps_r)


# ---------------------------------------------------------------- 3. the wrappers refuse what the kernels cannot read
def test_wrappers_refuse(env):
    ops = env[0]
    q, r = torch.zeros((4, 8), dtype=F32, device="cuda"), torch.zeros((6, 8), dtype=F32, device="cuda")
    rad = torch.zeros((6,), dtype=F32, device="cuda")
    cnt, dmin, imin = ops.prdc_count(q, r, rad)
    assert cnt.tolist() == [6] * 4 and dmin.tolist() == [0.0] * 4 and imin.tolist() == [0] * 4      # 0 <= 0 counts, the lowest index wins
    assert ops.prdc_radius(r, 5).tolist() == [0.0] * 6
    narrow = torch.as_strided(torch.zeros((64,), dtype=F32, device="cuda"), (4, 8), (4, 1))        # a pitch below L
    i4 = torch.zeros((4,), dtype=I32, device="cuda")
    for bad in (lambda: ops.prdc_count(q.double(), r, rad), lambda: ops.prdc_count(q.cpu(), r, rad), lambda: ops.prdc_count(q, r[:, :7], rad),
                lambda: ops.prdc_count(narrow, r, rad), lambda: ops.prdc_count(q, narrow, rad[:4]), lambda: ops.prdc_count(q, r, rad[:5]),
                lambda: ops.prdc_count(q, r, rad.double()), lambda: ops.prdc_count(q, r, rad.cpu()), lambda: ops.prdc_count(q, r, rad, cnt=i4.long()),
                lambda: ops.prdc_count(q, r, rad, cnt=i4[:3]), lambda: ops.prdc_count(q, r, rad, dmin=i4), lambda: ops.prdc_count(q, r, rad, imin=i4.float()),
                lambda: ops.prdc_count(q, r, rad, dmin=torch.zeros(4, device="cuda"), want_min=False),
                lambda: ops.prdc_count(q, r, rad, workspace=torch.zeros((8,), dtype=F32, device="cuda")),
                lambda: ops.prdc_radius(r, 0), lambda: ops.prdc_radius(r, 32), lambda: ops.prdc_radius(r, 6), lambda: ops.prdc_radius(r.double(), 2),
                lambda: ops.prdc_radius(narrow, 2), lambda: ops.prdc_radius(r, 2, rad=rad[:5]), lambda: ops.prdc_radius(r, 2, rad=rad.double())):
        with pytest.raises(ValueError):
            bad()
    from split_vae_amd._lib import SplitVaeError
    small = torch.zeros((16,), dtype=torch.uint8, device="cuda")
    with pytest.raises(SplitVaeError):
        ops.prdc_count(q, r, rad, workspace=small)                         # SV_E_WORKSPACE
    with pytest.raises(SplitVaeError):
        ops.prdc_radius(r, 2, workspace=small)
    with pytest.raises(SplitVaeError):
        ops.prdc_workspace_bytes(4, 6, 513, 1)


# ---------------------------------------------------------------- 4. end to end
H, LAT, Y_SIZE, N_IMG, PATCH, K = 32, 64, 10, 40, 4, 3


def _make(kind):
    from split_vae_amd.gm import LGGMVae
    from split_vae_amd.gmvae import GMVae
    from split_vae_amd.model import LGVae
    shape = (None, H, H, 3)
    if kind == "lgvae":
        return LGVae(LAT, LAT, image_shape=shape, dtype="f32", seed=3)
    if kind == "gmvae":
        return GMVae(LAT, shape, Y_SIZE, 0.4, dtype="f32", seed=3)
    return LGGMVae(LAT, LAT, shape, Y_SIZE, 0.4, dtype="f32", seed=3)


def _images(ops, n=N_IMG, seed=41):
    """n images in the data's own domain (smooth blobs) beside their patch scramble: [n,H,H,6]"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:H] / float(H)
    x = np.zeros((n, H, H, 3))
    for i in range(n):
        for c in range(3):
            a, b, p, q = rng.uniform(-3, 3, 4)
            x[i, ..., c] = np.sin(a * 2 * np.pi * yy + p) * np.cos(b * 2 * np.pi * xx + q)
    lv = np.clip(np.rint(x * 127.5 + 127.5), 0, 255).astype(np.int64)
    x3 = torch.from_numpy(swap_ref.make_lut()[lv]).cuda()
    perm = ops.random_perm(n, (H // PATCH) ** 2, 5, 0, 0)
    return ops.scramble_gather(x3, perm, PATCH)


def _composition(ops, sq, model, batches, name):
    """the fake set's features from existing pieces: recon_draw, the plan's decoder phase, swap_requantise, batch_posterior"""
    from split_vae_amd._lib import PHASE_FWD_DECODERS, PHASE_PREP, RECON_KEEP_G, RECON_KEEP_L, RECON_MEANS
    from split_vae_amd.data import ResidentDataset
    from split_vae_amd.latent_info import batch_posterior, posteriors
    X, _, Lg, Ll = posteriors(model, batches, N_IMG, keyed=True)
    Lc = Lg + Ll
    B = batches[0].shape[0]
    plan = model.plan(B)
    zcat = plan.buffer("zcat", model.dtype, (B, Lc))
    lut = torch.from_numpy(ResidentDataset.make_lut()).cuda()
    prior = sq.draw_prior(model)
    Yf = torch.empty((N_IMG, Lc), dtype=F32, device="cuda")
    for o in range(0, N_IMG, B):
        idx = torch.arange(o, o + B, device="cuda").clamp_(max=N_IMG - 1)
        take = min(B, N_IMG - o)
        rows = X.index_select(0, idx)
        mg, ml = rows[:, :Lg].contiguous(), (rows[:, Lg:].contiguous() if Ll else None)
        kw = dict(prior=prior, seed=model.seed, sample_offset=o)
        if name == "recon":
            ops.recon_draw(mg, ml, RECON_MEANS, zcat)
        elif name == "g_drawn" or not Ll:
            ops.recon_draw(mg, ml, RECON_KEEP_L, zcat, **kw)
        elif name == "l_drawn":
            ops.recon_draw(mg, ml, RECON_KEEP_G, zcat, **kw)
        else:
            a, b = torch.empty((B, Lc), dtype=F32, device="cuda"), torch.empty((B, Lc), dtype=F32, device="cuda")
            ops.recon_draw(mg, ml, RECON_KEEP_L, a, **kw)
            ops.recon_draw(mg, ml, RECON_KEEP_G, b, **kw)
            zcat.copy_(torch.cat([a[:, :Lg], b[:, Lg:]], dim=1))
        plan.step(PHASE_PREP | PHASE_FWD_DECODERS, params=model.flat)
        perm = ops.random_perm(B, (H // PATCH) ** 2, model.seed, sq.PERM_STEP, o)
        images6 = ops.swap_requantise(plan.buffer("out6_x", F32, (B, H, H, 6)), lut, perm, PATCH)
        mg2, _, ml2, _ = batch_posterior(model, images6, o)
        Yf[o:o + take] = torch.cat([mg2[:take]] + ([ml2[:take]] if Ll else []), dim=1)
    return X, Yf


@pytest.mark.parametrize("kind", ["lgvae", "lggmvae", "gmvae"])
def test_evaluate_equals_a_composition_of_existing_pieces(env, deterministic, kind):
    ops, sq, _ = env
    model = _make(kind)
    x = _images(ops)
    batches = [x[o:o + 8].contiguous() for o in range(0, N_IMG, 8)]
    calls = getattr(model, "_calls", None)
    res = sq.evaluate(model, batches, N_IMG, k=K, patch=PATCH, keep=True, grid=4)
    assert getattr(model, "_calls", None) == calls
    assert res["n_images"] == N_IMG and res["k"] == K
    assert res["sets"] == (("prior", "recon") if kind == "gmvae" else ("prior", "g_drawn", "l_drawn", "recon"))
    assert res["samples"].shape == (4, H, H, 3) and set(np.unique(res["samples"].cpu().numpy()).tolist()) <= set(swap_ref.make_lut().tolist())
    for name in res["sets"]:
        X, Yf = _composition(ops, sq, model, batches, name)
        assert torch.equal(res["X"].view(I32), X.view(I32))
        assert torch.equal(res["Y"][name].view(I32), Yf.view(I32))               # the re-encoded features, bit for bit
        rad_x, rad_y = ops.prdc_radius(X, K), ops.prdc_radius(Yf, K)
        cf, _, imf = ops.prdc_count(Yf, X, rad_x)
        cr, dr, _ = ops.prdc_count(X, Yf, rad_y)
        cf, imf, cr, dr, rx, ry = (t.cpu().numpy() for t in (cf, imf, cr, dr, rad_x, rad_y))
        assert np.array_equal(res["rad_real"], rx) and np.array_equal(res["cnt_fake_" + name], cf) and np.array_equal(res["cnt_real_" + name], cr)
        assert np.array_equal(res["dmin_real_" + name], dr) and np.array_equal(res["imin_fake_" + name], imf)
        Xh, Yh = X.cpu().numpy(), Yf.cpu().numpy()
        lo, hi = ref.count_bracket(Yh, Xh, rx)                                   # the new ops against the twin on the model's own features
        assert ref.counts_in_bracket(cf, lo, hi, ref.count(Yh, Xh, rx)[0])
        assert ref.within(rx, ref.radius(Xh, K), ref.pair_eps(Xh, Xh).max(axis=1))
        want = ref.figures(cf, cr, dr, rx, ry, K)
        for key, val in want.items():
            assert abs(res[key + "_" + name] - val) <= 1e-12, (key, name)
        # the Frechet distance: sv_linprobe_gram's sums and the twin's route through the eigenvalues of C_a C_b.  N - 1 < L: the
        # covariances are singular, and a zero eigenvalue comes back as +- L u |C_a| |C_b|, its root as sqrt(L u) sqrt(|C_a| |C_b|)
        Sx, Sy = ops.linprobe_gram(X).cpu().numpy(), ops.linprobe_gram(Yf).cpu().numpy()
        (ma, Ca), (mb, Cb) = sq.moments(Sx, N_IMG), sq.moments(Sy, N_IMG)
        twin = ref.frechet(ma, Ca, mb, Cb)
        L = Xh.shape[1]
        tol = 2 * L * np.sqrt(L * 2.0 ** -52) * np.sqrt(np.trace(Ca) * np.trace(Cb)) + 1e-9 * (np.trace(Ca) + np.trace(Cb))
        print("%s %s: %s, Frechet %.6g (twin %.6g, tolerance %.3g)" % (kind, name, {k_: round(v, 4) for k_, v in want.items()}, res["frechet_" + name], twin, tol))
        assert abs(res["frechet_" + name] - twin) <= tol
        # the moments against float64: a chunk's sums are fp32 chains of c = min(N, chunk rows) products (gamma_(c+1) of the sum of
        # magnitudes, at most the largest second moment by Cauchy-Schwarz); C = S / N - m m^T carries the sum's error and twice the mean's
        m64, C64 = ref.moments(Xh)
        g = 1.01 * (min(N_IMG, ops.linprobe_chunk_rows()) + 1) * 2.0 ** -24
        s2 = float((Xh.astype(np.float64) ** 2).mean(axis=0).max())
        assert np.abs(ma - m64).max() <= g * np.sqrt(s2) and np.abs(Ca - C64).max() <= 3 * g * s2
    line = sq.report_line(res)
    assert line.startswith("Test sample quality (40 images, k=3): prior precision ") and "; reconstructions: precision " in line
    assert ("z_g drawn (z_l kept): " in line) == (kind != "gmvae")


@pytest.mark.parametrize("kind", ["lgvae", "lggmvae", "gmvae"])
def test_the_same_figures_at_batch_size_5(env, deterministic, kind):
    """N = 40 in batches of 8 and of 5: fake i and image i are keyed by the global index i, so the figures do not move"""
    ops, sq, _ = env
    model = _make(kind)
    x = _images(ops)
    res = sq.evaluate(model, [x[o:o + 8].contiguous() for o in range(0, N_IMG, 8)], N_IMG, k=K, patch=PATCH)
    five = sq.evaluate(model, [x[o:o + 5].contiguous() for o in range(0, N_IMG, 5)], N_IMG, k=K, patch=PATCH)
    for name in res["sets"]:
        for key in sq.KEYS:
            print("%s %s_%s: batch 8 %.9g, batch 5 %.9g" % (kind, key, name, res[key + "_" + name], five[key + "_" + name]))
    for name in res["sets"]:
        for key in sq.KEYS:
            a, b = res[key + "_" + name], five[key + "_" + name]
            assert abs(a - b) <= (1e-12 if key != "frechet" else 1e-9 * max(abs(a), 1.0)), (key, name)


def test_a_short_last_batch_and_fewer_images_than_asked(env, deterministic):
    ops, sq, _ = env
    model = _make("lgvae")
    x = _images(ops, 21)
    res = sq.evaluate(model, [x[o:o + 8].contiguous() for o in range(0, 24, 8) if o < 21], 1000, k=K, patch=PATCH)
    assert res["n_images"] == 21 and res["cnt_fake_prior"].shape == (21,) and res["imin_fake_recon"].max() < 21
    with pytest.raises(ValueError):
        sq.evaluate(model, [x[:8].contiguous()], 3, k=K)
    with pytest.raises(ValueError):
        sq.evaluate(model, [x[:8].contiguous()], 8, k=32)


@pytest.mark.parametrize("kind", ["lgvae", "lggmvae", "gmvae"])
def test_cli_prints_the_line_and_writes_the_files(env, tmp_path, monkeypatch, capsys, kind):
    """--synthetic -no_label (32 test images): the line, the nearest-neighbour strip and the .npz"""
    from split_vae_amd import data, sample_quality as sq
    from split_vae_amd.main import build_parser, make_model
    from split_vae_amd.utils import dotdict, images_of
    from split_vae_amd.visualizer import load_png
    monkeypatch.chdir(tmp_path)
    flags = ["--synthetic", "-no_label", "--batch_size", "8", "--dtype", "f32", "--patch_size", "4", "--model", kind]
    config = dotdict(vars(build_parser().parse_args(flags)))
    config.label = False
    model, _ = make_model(kind, config, (None, 32, 32, 3))
    path = str(tmp_path / "w.npz")
    model.save_weights(path)
    capsys.readouterr()
    out_dir = str(tmp_path / "sq")
    res = sq.main(flags + ["--weights", path, "--sq_images", "30", "--sq_k", "3", "--sq_out", out_dir, "--sq_grid", "4"])
    out = capsys.readouterr().out
    lines = [l for l in out.splitlines() if l.startswith("Test sample quality (")]
    assert len(lines) == 1 and lines[0].startswith("Test sample quality (30 images, k=3): prior precision ")
    assert "; reconstructions: precision " in lines[0] and ("; z_l drawn (z_g kept): precision " in lines[0]) == (kind != "gmvae")
    assert res["sq_n_images"] == 30 and res["sq_k"] == 3 and not any(torch.is_tensor(v) or isinstance(v, np.ndarray) for v in res.values())
    for name in res["sq_sets"]:
        for key in ("precision", "recall", "coverage"):
            assert 0.0 <= res["sq_%s_%s" % (key, name)] <= 1.0
        assert res["sq_density_" + name] >= 0.0 and res["sq_frechet_" + name] >= -1e-6
    doc = np.load(out_dir + "/sample_quality.npz")
    want = {"k", "n_images", "rad_real"} | {"%s_%s" % (key, name) for name in res["sq_sets"]
                                            for key in sq.KEYS + ("cnt_fake", "cnt_real", "dmin_real", "imin_fake")}
    assert set(doc.files) == want and doc["rad_real"].shape == (30,) and doc["imin_fake_prior"].shape == (30,)
    assert doc["imin_fake_prior"].min() >= 0 and doc["imin_fake_prior"].max() < 30 and float(doc["precision_prior"]) == res["sq_precision_prior"]
    png = load_png(out_dir + "/sample_nearest.png").astype(np.float64) / 255.0
    assert png.shape == (2 * 32, 4 * 32, 3)
    _, test_ds, _ = data.get_dataset("svhn", 8, synthetic=True, data_dir=config.data_dir, get_label=False)
    x = torch.cat([images_of(b)[..., :3] for b in test_ds])[:30].cpu().numpy().astype(np.float64)
    for a in range(4):
        tile = (x[int(doc["imin_fake_prior"][a])] + 1.0) * 0.5
        assert np.abs(png[32:, a * 32:(a + 1) * 32] - tile).max() <= 1.0 / 255 + 1e-9       # beneath each sample: the test image imin names
