"""GPU: the swap-consistency report (sv_swap_pair / sv_swap_requantise / sv_swap_rank, split_vae_amd/swap.py) against the float64
twins of tests/swap_ref.py: ranks bit for bit on integer lattices and inside a derived bracket on Gaussian data, the requantiser and
the pair gather bit for bit, the wrappers' refusals, and swap.evaluate against a composition of existing pieces on two models."""
import numpy as np
import pytest
import torch

import swap_ref as ref

pytestmark = pytest.mark.gpu

F32, I32 = torch.float32, torch.int32
SENTINEL = -77777
WORST = {"undecided": 0.0}


@pytest.fixture(scope="module")
def env(lib_built):
    assert torch.cuda.is_available()
    from split_vae_amd import _lib, ops, swap
    return ops, swap, _lib


def _strided(a, pad, off):
    """the rows of a [N, L] in a NaN-filled buffer with row pitch L + pad that starts `off` floats behind the allocation"""
    N, L = a.shape
    buf = torch.full((off + N * (L + pad),), float("nan"), dtype=F32, device="cuda")
    view = buf[off:].view(N, L + pad)[:, :L]
    view.copy_(torch.from_numpy(a))
    assert view.stride(0) == L + pad and view.data_ptr() == buf.data_ptr() + 4 * off
    return view


def _rank(ops, c, pads=(0, 0, 0)):
    """sv_swap_rank on a case: a sentinel-filled rank with a guard row either side, a workspace of NaN bit patterns with a guard behind it,
    and the call twice: the same bits"""
    pq, pr, off = pads
    Q, R = _strided(c["Q"], pq, off), _strided(c["R"], pr, off)
    Nq, L = c["Q"].shape
    t0, t1 = torch.from_numpy(c["t0"]).cuda(), torch.from_numpy(c["t1"]).cuda()
    flat = torch.full((Nq + 2, 2), SENTINEL, dtype=I32, device="cuda")
    nbytes = ops.swap_rank_workspace_bytes(Nq, c["R"].shape[0], L)
    ws = torch.full((nbytes + 256,), 0xFF, dtype=torch.uint8, device="cuda")
    out = ops.swap_rank(Q, R, t0, t1, rank=flat[1:Nq + 1], workspace=ws[:nbytes])
    first = out.clone()
    torch.cuda.synchronize()
    assert (flat[0] == SENTINEL).all() and (flat[Nq + 1] == SENTINEL).all() and (ws[nbytes:] == 0xFF).all()
    ops.swap_rank(Q, R, t0, t1, rank=flat[1:Nq + 1], workspace=ws[:nbytes])              # the workspace now holds the first call's partials
    assert torch.equal(first, out)
    return first.cpu().numpy()


# ---------------------------------------------------------------- 1. ranks on integer lattices
@pytest.mark.parametrize("index", range(9))
def test_ranks_on_integer_lattices_bit_for_bit(env, index):
    ops = env[0]
    shapes = ref.lattice_shapes(ops.swap_chunk_rows())
    assert len(shapes) == 9
    Nq, Nr, L, pq, pr, off = shapes[index]
    c = ref.lattice_case(Nq, Nr, L, 100 + index)
    want = ref.rank(c["Q"], c["R"], c["t0"], c["t1"])
    got = _rank(ops, c, (pq, pr, off))
    print("lattice Nq %d Nr %d L %d: ranks %d .. %d, differing %d" % (Nq, Nr, L, want.min(), want.max(), int((got != want).sum())))
    assert ref.ranks_equal(got, want)


# ---------------------------------------------------------------- 2. ranks on Gaussian data
@pytest.mark.parametrize("shape", ref.GAUSS_SHAPES)
def test_ranks_on_gaussian_data_inside_the_derived_bracket(env, shape):
    """lo <= rank <= hi for every query, the twin's rank wherever lo == hi; the bracket decides all but 2 % of the queries"""
    c = ref.gaussian_case(*shape)
    lo, hi = ref.rank_bracket(c["Q"], c["R"], c["t0"], c["t1"])
    want = ref.rank(c["Q"], c["R"], c["t0"], c["t1"])
    share = ref.undecided_share(lo, hi)
    got = _rank(env[0], c)
    WORST["undecided"] = max(WORST["undecided"], share)
    print("gaussian %s: undecided share %.4f, outside the bracket %d, off the twin where decided %d, off the twin at all %d" %
          (shape, share, int(((got < lo) | (got > hi)).sum()), int((got != want)[lo == hi].sum()), int((got != want).sum())))
    assert share <= ref.UNDECIDED_CAP
    assert ref.ranks_in_bracket(got, lo, hi, want)


# ---------------------------------------------------------------- 3. sv_swap_requantise
@pytest.mark.parametrize("B,H,patch", ref.REQUANT_SHAPES)
def test_requantise_bit_for_bit(env, B, H, patch):
    ops = env[0]
    n = ref.REQUANT_SHAPES.index((B, H, patch))
    out6, perm = ref.requantise_means(B, H, 50 + n), ref.requantise_perms(B, H, patch, 60 + n)
    assert np.isnan(out6[..., 3:]).all()                                                  # the log-scale channels must not be read
    want = ref.requantise(out6, perm, patch)
    flat = torch.full((B + 2, H, H, 6), float(SENTINEL), dtype=F32, device="cuda")
    lut = torch.from_numpy(ref.make_lut()).cuda()
    got = ops.swap_requantise(torch.from_numpy(out6).cuda(), lut, torch.from_numpy(perm).cuda(), patch, out=flat[1:B + 1])
    torch.cuda.synchronize()
    assert (flat[0] == SENTINEL).all() and (flat[B + 1] == SENTINEL).all()
    got = got.cpu().numpy()
    print("requantise B %d H %d patch %d: differing words %d" % (B, H, patch, int((got.view(np.uint32) != want.view(np.uint32)).sum())))
    assert ref.bits_equal(got, want)


# ---------------------------------------------------------------- 4. sv_swap_pair
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("N,B,Lg,Ll,pad", [(9, 4, 4, 3, 0), (40, 33, 128, 128, 5), (3, 1, 1, 7, 2), (300, 257, 32, 64, 0)])
def test_pair_bit_for_bit(env, dtype, N, B, Lg, Ll, pad):
    ops = env[0]
    rng = np.random.default_rng(N + B)
    mu = rng.standard_normal((N, Lg + Ll)).astype(np.float32)
    ig, il = rng.integers(0, N, size=B).astype(np.int32), rng.integers(0, N, size=B).astype(np.int32)
    il[0] = ig[0]                                                                          # ig == il: the image's own latents
    want = torch.from_numpy(ref.pair(mu, ig, il, Lg)).to(dtype)
    flat = torch.full((B + 2, Lg + Ll), float(SENTINEL), dtype=dtype, device="cuda")
    got = ops.swap_pair(_strided(mu, pad, 0), torch.from_numpy(ig).cuda(), torch.from_numpy(il).cuda(), Lg, flat[1:B + 1])
    torch.cuda.synchronize()
    assert (flat[0] == SENTINEL).all() and (flat[B + 1] == SENTINEL).all()
    as_int = torch.int32 if dtype == torch.float32 else torch.int16
    assert torch.equal(got.cpu().view(as_int), want.view(as_int))
    if B > 1:                                                                              # (B = 1 is the ig == il row alone)
        assert not torch.equal(torch.from_numpy(ref.pair(mu, ig, il, Lg, mutant="l_from_ig")).to(dtype).view(as_int), want.view(as_int))


# ---------------------------------------------------------------- 5. the wrappers refuse what the kernels cannot read
def test_wrappers_refuse(env):
    ops = env[0]
    q, r = torch.zeros((4, 8), dtype=F32, device="cuda"), torch.zeros((6, 8), dtype=F32, device="cuda")
    t = torch.zeros((4,), dtype=I32, device="cuda")
    ok = ops.swap_rank(q, r, t, t)
    assert ok.shape == (4, 2) and ok.dtype == I32 and int(ok.abs().sum()) == 0            # all distances tie, the target is row 0
    narrow = torch.as_strided(torch.zeros((64,), dtype=F32, device="cuda"), (4, 8), (4, 1))        # a pitch below L
    for bad in (lambda: ops.swap_rank(q.double(), r, t, t), lambda: ops.swap_rank(q.cpu(), r, t, t), lambda: ops.swap_rank(q, r[:, :7], t, t),
                lambda: ops.swap_rank(narrow, r, t, t), lambda: ops.swap_rank(q, narrow, t, t), lambda: ops.swap_rank(q, r, t.long(), t),
                lambda: ops.swap_rank(q, r, t, t.cpu()), lambda: ops.swap_rank(q, r, t[:3], t), lambda: ops.swap_rank(q, r, t + 6, t),
                lambda: ops.swap_rank(q, r, t, t - 1), lambda: ops.swap_rank(q, r, t, t, rank=torch.zeros((4, 2), dtype=torch.int64, device="cuda")),
                lambda: ops.swap_rank(q, r, t, t, workspace=torch.zeros((8,), dtype=F32, device="cuda"))):
        with pytest.raises(ValueError):
            bad()
    from split_vae_amd._lib import SplitVaeError
    with pytest.raises(SplitVaeError):
        ops.swap_rank(q, r, t, t, workspace=torch.zeros((16,), dtype=torch.uint8, device="cuda"))        # SV_E_WORKSPACE
    z = torch.zeros((4, 8), dtype=F32, device="cuda")
    for bad in (lambda: ops.swap_pair(r, t + 6, t, 4, z), lambda: ops.swap_pair(r, t, t - 1, 4, z), lambda: ops.swap_pair(r, t, t, 8, z),
                lambda: ops.swap_pair(r, t, t, 0, z), lambda: ops.swap_pair(r.cpu(), t, t, 4, z), lambda: ops.swap_pair(r, t, t, 4, z.double()),
                lambda: ops.swap_pair(r, t, t, 4, z[:, :7]), lambda: ops.swap_pair(r, t.long(), t, 4, z), lambda: ops.swap_pair(narrow, t, t, 4, z)):
        with pytest.raises(ValueError):
            bad()
    out6 = torch.zeros((2, 8, 8, 6), dtype=F32, device="cuda")
    lut = torch.from_numpy(ref.make_lut()).cuda()
    perm = torch.zeros((2, 4), dtype=I32, device="cuda")
    for bad in (lambda: ops.swap_requantise(out6.double(), lut, perm, 4), lambda: ops.swap_requantise(out6.cpu(), lut, perm, 4),
                lambda: ops.swap_requantise(out6, lut[:255], perm, 4), lambda: ops.swap_requantise(out6, lut, perm, 3),
                lambda: ops.swap_requantise(out6, lut, perm, 2), lambda: ops.swap_requantise(out6, lut, perm.long(), 4),
                lambda: ops.swap_requantise(out6[:, :, :4], lut, perm, 4), lambda: ops.swap_requantise(out6, lut, perm, 4, out=out6)):
        with pytest.raises(ValueError):
            bad()


# ---------------------------------------------------------------- 6. end to end
H, LAT, Y, N_IMG, PATCH = 32, 128, 10, 20, 4
SHIFTS = [3, 7]


def _make(kind):
    from split_vae_amd.gm import LGGMVae
    from split_vae_amd.model import LGVae
    shape = (None, H, H, 3)
    if kind == "lgvae":
        return LGVae(LAT, LAT, image_shape=shape, dtype="f32", seed=3)
    return LGGMVae(LAT, LAT, shape, Y, 0.4, dtype="f32", seed=3)


def _images(ops, n=24, seed=41):
    """n images in the data's own domain (smooth blobs, so that the encoders see structure) beside their patch scramble: [n,H,H,6]"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:H] / float(H)
    x = np.zeros((n, H, H, 3))
    for i in range(n):
        for c in range(3):
            a, b, p, q = rng.uniform(-3, 3, 4)
            x[i, ..., c] = np.sin(a * 2 * np.pi * yy + p) * np.cos(b * 2 * np.pi * xx + q)
    lv = np.clip(np.rint(x * 127.5 + 127.5), 0, 255).astype(np.int64)
    x3 = torch.from_numpy(ref.make_lut()[lv]).cuda()
    perm = ops.random_perm(n, (H // PATCH) ** 2, 5, 0, 0)
    return ops.scramble_gather(x3, perm, PATCH)


def _composition(ops, swap, model, batches, shifts):
    """swap.evaluate's hybrids and re-encoded means from existing pieces: index_select, the decode through the plan, the twin's requantiser on
    the device's out6, ops.scramble_gather with the same permutations, batch_posterior"""
    from split_vae_amd._lib import PHASE_FWD_DECODERS, PHASE_PREP
    from split_vae_amd.latent_info import batch_posterior, posteriors
    mu = posteriors(model, batches, N_IMG, keyed=True)[0]
    B = batches[0].shape[0]
    plan = model.plan(B)
    lut = ref.make_lut()
    hyb = torch.empty((len(shifts) + 1, N_IMG, H, H, 6), dtype=F32, device="cuda")
    Q = torch.empty((len(shifts) + 1, N_IMG, 2 * LAT), dtype=F32, device="cuda")
    for pi, s in enumerate([0] + shifts):
        for o in range(0, N_IMG, B):
            idx = torch.arange(o, o + B, device="cuda").clamp_(max=N_IMG - 1)
            take = min(B, N_IMG - o)
            plan.buffer("zcat", model.dtype, (B, 2 * LAT)).copy_(torch.cat([mu.index_select(0, idx)[:, :LAT], mu.index_select(0, (idx + s) % N_IMG)[:, LAT:]], dim=1))
            plan.step(PHASE_PREP | PHASE_FWD_DECODERS, params=model.flat)
            out6 = plan.buffer("out6_x", F32, (B, H, H, 6)).cpu().numpy()
            x3 = torch.from_numpy(lut[ref.levels(np.ascontiguousarray(out6[..., :3]))]).cuda()
            perm = ops.random_perm(B, (H // PATCH) ** 2, model.seed, swap.PERM_STEP, pi * N_IMG + o)
            images6 = ops.scramble_gather(x3, perm, PATCH)
            mg, _, ml, _ = batch_posterior(model, images6, o)
            hyb[pi, o:o + take] = images6[:take]
            Q[pi, o:o + take] = torch.cat([mg[:take], ml[:take]], dim=1)
    return mu, hyb, Q


@pytest.mark.parametrize("kind", ["lgvae", "lggmvae"])
def test_evaluate_equals_a_composition_of_existing_pieces(env, deterministic, kind):
    ops, swap, _ = env
    model = _make(kind)
    x = _images(ops)
    batches = [x[o:o + 8].contiguous() for o in range(0, 24, 8)]
    calls = getattr(model, "_calls", None)
    res = swap.evaluate(model, batches, N_IMG, k=3, shifts=SHIFTS, patch=PATCH, keep=True)
    assert getattr(model, "_calls", None) == calls
    mu, hyb, Q = _composition(ops, swap, model, batches, SHIFTS)
    assert res["n_images"] == N_IMG and res["shifts"] == SHIFTS and res["partners"] == 2 and not res["labelled"]
    assert torch.equal(res["mu"].view(I32), mu.view(I32))
    assert torch.equal(res["hybrids"].view(I32), hyb.view(I32))                          # the hybrid images, bit for bit
    assert torch.equal(res["Q"].view(I32), Q.view(I32))                                  # the re-encoded means, bit for bit
    levels = set(np.unique(res["hybrids"].cpu().numpy()).tolist())
    assert levels <= set(ref.make_lut().tolist()) and len(levels) > 4                    # the hybrids lie in the data's own domain
    Qh, muh = Q.cpu().numpy(), mu.cpu().numpy()
    i = np.arange(N_IMG)
    for pi, s in enumerate([0] + SHIFTS):
        j = ref.partner(N_IMG, s)
        for blk, cols, (t0, t1) in (("g", slice(0, LAT), (i, j)), ("l", slice(LAT, 2 * LAT), (j, i))):
            lo, hi = ref.rank_bracket(Qh[pi][:, cols], muh[:, cols], t0, t1)
            want = ref.rank(Qh[pi][:, cols], muh[:, cols], t0, t1)
            got = res["ranks_" + blk][pi]
            print("%s pass %d z_%s: kept ranks %s, undecided %d" % (kind, pi, blk, got[:, 0].tolist(), int((hi > lo).sum())))
            assert ref.ranks_in_bracket(got, lo, hi, want)
    for blk in ("g", "l"):
        want = ref.figures(res["ranks_" + blk], 3)
        for key, val in want.items():
            assert abs(res[key + "_" + blk] - val) <= 1e-12, (key, blk)
    line = swap.report_line(res)
    assert line.startswith("Test swap consistency (20 images, 2 partners): z_g kept@1 ") and "kept@3 " in line and "class follows" not in line


@pytest.mark.parametrize("kind", ["lgvae", "lggmvae"])
def test_the_same_figures_at_batch_size_5(env, deterministic, kind):
    """N = 20 in batches of 8 (a short last batch) and in batches of 5: the same figures.  lggmvae computes z_g's mean behind a relaxed
    categorical sample; the report keys that sample by the image's global index (batch_posterior's sample_offset), not by its row in the
    batch -- with the row key the figures moved with the batch size (z_g kept@1 0.15 against 0.10, MRR 0.4110 against 0.3354)."""
    ops, swap, _ = env
    model = _make(kind)
    x = _images(ops)
    res = swap.evaluate(model, [x[o:o + 8].contiguous() for o in range(0, 24, 8)], N_IMG, k=3, shifts=SHIFTS, patch=PATCH)
    five = swap.evaluate(model, [x[o:o + 5].contiguous() for o in range(0, 20, 5)], N_IMG, k=3, shifts=SHIFTS, patch=PATCH)
    for blk in ("g", "l"):
        for key in ("kept1", "keptk", "mrr", "leak1", "cycle1"):
            print("%s %s_%s: batch 8 %.6f, batch 5 %.6f" % (kind, key, blk, res[key + "_" + blk], five[key + "_" + blk]))
    for blk in ("g", "l"):
        for key in ("kept1", "keptk", "mrr", "leak1", "cycle1"):
            assert abs(res[key + "_" + blk] - five[key + "_" + blk]) <= 1e-12, (key, blk)


def test_class_figures_on_a_labelled_set(env, deterministic):
    """(images, one-hot) batches and references: the class figures are the twin's on sv_knn_classify's predictions of the re-encoded z_g"""
    ops, swap, _ = env
    model = _make("lgvae")
    x = _images(ops)
    cls = torch.arange(24, device="cuda") % 3
    onehot = torch.nn.functional.one_hot(cls, 10).to(F32)
    batches = [(x[o:o + 8].contiguous(), onehot[o:o + 8].contiguous()) for o in range(0, 24, 8)]
    res = swap.evaluate(model, batches, N_IMG, k=3, shifts=SHIFTS, patch=PATCH, knn=3, ref_batches=batches)
    assert res["labelled"] and res["knn"] == 3 and res["n_ref"] == 24 and res["labels"].tolist() == (np.arange(N_IMG) % 3).tolist()
    from split_vae_amd.latent_info import posteriors
    rg = posteriors(model, batches, None, keyed=True)[0][:, :LAT]
    pred = np.stack([ops.knn_classify(res["Q"][pi][:, :LAT], rg, cls.to(torch.uint8), 3, 10).cpu().numpy() for pi in range(3)])
    want = ref.class_figures(pred, res["labels"], SHIFTS)
    assert res["unlike_pairs"] == want["unlike_pairs"] > 0
    for key in ("follows_g", "follows_l", "unswapped_acc"):
        assert abs(res[key] - want[key]) <= 1e-12, key
    assert "; class follows z_g source " in swap.report_line(res) and "(%d unlike pairs, k=3, 24 refs; unswapped " % want["unlike_pairs"] in swap.report_line(res)
    bare = swap.evaluate(model, [b[0] for b in batches], N_IMG, k=3, shifts=SHIFTS, patch=PATCH, knn=3, ref_batches=batches)
    assert not bare["labelled"] and bare["labels"] is None and np.array_equal(bare["ranks_g"], res["ranks_g"])


def test_cli_prints_the_line_and_writes_the_files(env, tmp_path, monkeypatch, capsys):
    """--synthetic -no_label (32 test images): one note, the label-free line, the grid and the .npz"""
    from split_vae_amd import data, swap
    from split_vae_amd.main import build_parser, make_model
    from split_vae_amd.utils import dotdict, images_of
    from split_vae_amd.visualizer import load_png
    monkeypatch.chdir(tmp_path)
    flags = ["--synthetic", "-no_label", "--batch_size", "8", "--dtype", "f32", "--patch_size", "4"]
    config = dotdict(vars(build_parser().parse_args(flags)))
    model, _ = make_model("lgvae", config, (None, 32, 32, 3))
    path = str(tmp_path / "w.npz")
    model.save_weights(path)
    capsys.readouterr()
    out_dir = str(tmp_path / "swap")
    res = swap.main(flags + ["--weights", path, "--swap_images", "30", "--swap_partners", "2", "--swap_k", "5", "--swap_out", out_dir, "--swap_grid", "3"])
    out = capsys.readouterr().out
    lines = [l for l in out.splitlines() if l.startswith("Test swap consistency (")]
    assert out.count(swap.UNLABELLED) == 1 and len(lines) == 1
    assert lines[0].startswith("Test swap consistency (30 images, 2 partners): z_g kept@1 ") and "; z_l kept@1 " in lines[0]
    assert "kept@5 " in lines[0] and "class follows" not in lines[0]
    assert res["swap_n_images"] == 30 and res["swap_follows_g"] is None and 0.0 <= res["swap_kept1_g"] <= res["swap_keptk_g"] <= 1.0
    assert len(res["swap_shifts"]) == 2 and not any(torch.is_tensor(v) or isinstance(v, np.ndarray) for v in res.values())
    png = load_png(out_dir + "/swap_grid.png").astype(np.float64) / 255.0
    assert png.shape == (4 * 32, 4 * 32, 3) and (png[:32, :32] == 1.0).all()            # (n+1) x (n+1) tiles, the corner white
    _, test_ds, _ = data.get_dataset("svhn", 8, synthetic=True, data_dir=config.data_dir, get_label=False)
    x = torch.cat([images_of(b)[..., :3] for b in test_ds])[:3].cpu().numpy().astype(np.float64)
    for a in range(3):
        tile = (x[a] + 1.0) * 0.5
        assert np.abs(png[(a + 1) * 32:(a + 2) * 32, :32] - tile).max() <= 1.0 / 255 + 1e-9       # the left column: the z_g sources
        assert np.abs(png[:32, (a + 1) * 32:(a + 2) * 32] - tile).max() <= 1.0 / 255 + 1e-9       # the top row: the z_l sources
    doc = np.load(out_dir + "/swap.npz")
    assert sorted(doc.files) == ["labels", "ranks_g", "ranks_l", "shifts"]
    assert doc["ranks_g"].shape == (3, 30, 2) and doc["ranks_l"].shape == (3, 30, 2) and doc["shifts"].tolist() == res["swap_shifts"]
    assert (doc["labels"] == -1).all() and doc["ranks_g"].min() >= 0 and doc["ranks_g"].max() < 30
