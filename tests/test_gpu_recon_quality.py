"""GPU tests of the label-free reconstruction quality report: sv_recon_draw / sv_recon_quality / sv_recon_finish
(csrc/recon_quality.hip) through their entry points against the float64 twin of tests/recon_quality_ref.py, image by image inside the
bound derived there; the extents written and read, bit-reproducibility, the refusals, and split_vae_amd/recon_quality.py on the three
models against the twin applied to what the models' own decode() returns."""
import ctypes as C

import numpy as np
import pytest
import torch

import recon_quality_ref as ref

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
SENTINEL = -12345.678
WORST = {"quality": 0.0}                  # worst device error / bound seen by this run (printed per test)


@pytest.fixture(scope="module")
def env(lib_built):
    assert torch.cuda.is_available()
    from split_vae_amd import _lib, ops, recon_quality
    return ops, recon_quality, _lib


def _quality(ops, xa, xb, layout, clip):
    """sv_recon_quality on xa, xb [B,H,W,3] embedded in NaN-poisoned buffers of the layout -> per_image [B,2] (NumPy); NaN-filled
    workspace and output, a sentinel row before and after the output: nothing outside the stated extent is written or read."""
    pa, oa, pb, ob = layout
    B, H, W = xa.shape[:3]
    a, b = torch.from_numpy(ref.embed(xa, pa, oa)).cuda(), torch.from_numpy(ref.embed(xb, pb, ob)).cuda()
    flat = torch.full((B + 2, 2), SENTINEL, dtype=F64, device="cuda")
    out = flat[1:B + 1]
    out.fill_(float("nan"))
    nbytes = ops.recon_quality_workspace_bytes(B, H, W)
    ws = torch.full((nbytes + 256,), 0xFF, dtype=torch.uint8, device="cuda")              # all-ones words: NaN
    ops.recon_quality(a, b, oa, ob, clip, per_image=out, workspace=ws[:nbytes])
    torch.cuda.synchronize()
    assert (flat[0] == SENTINEL).all() and (flat[B + 1] == SENTINEL).all() and (ws[nbytes:] == 0xFF).all()
    first = out.clone()
    ops.recon_quality(a, b, oa, ob, clip, per_image=out, workspace=ws[:nbytes])          # the workspace now holds the first call's pairs
    assert torch.equal(first, out)                                                        # the same call twice: the same bits
    return first.cpu().numpy()


def _check(ops, kind, shape, layout, clip):
    xa, xb = ref.images(kind, *shape)
    got = _quality(ops, xa, xb, layout, clip)
    want = ref.quality(xa, xb, clip_b=clip)
    e_mse, e_ssim = ref.bound(xa, xb, clip_b=clip)
    if kind == "copies" and clip:
        assert (got[:, 0] == 0).all() and np.abs(got[:, 1] - 1).max() <= e_ssim.max()
    ratio = max(np.max(np.abs(got[:, 1] - want[:, 1]) / e_ssim), np.max(np.abs(got[:, 0] - want[:, 0]) / np.maximum(e_mse, 1e-300)))
    WORST["quality"] = max(WORST["quality"], float(ratio))
    print("%s %s %s clip %d: worst error / bound %.3g (SSIM error %.3g of %.3g, MSE error %.3g of %.3g); so far %.3g" % (
        kind, shape, layout, clip, ratio, np.abs(got[:, 1] - want[:, 1]).max(), e_ssim.max(), np.abs(got[:, 0] - want[:, 0]).max(),
        e_mse.max(), WORST["quality"]))
    assert ref.agrees(got, want, e_mse, e_ssim)
    return got


# ---------------------------------------------------------------- 1. sv_recon_quality against the twin
@pytest.mark.parametrize("kind", ref.KINDS)
@pytest.mark.parametrize("shape", ref.SHAPES)
def test_quality_matches_the_twin_inside_the_bound(env, shape, kind):
    ops = env[0]
    i = ref.SHAPES.index(shape) + ref.KINDS.index(kind)
    for clip in (True, False):
        _check(ops, kind, shape, ref.LAYOUTS[(i + clip) % len(ref.LAYOUTS)], clip)


@pytest.mark.parametrize("layout", ref.LAYOUTS)
def test_quality_reads_every_layout_in_place(env, layout):
    ops = env[0]
    got = [_check(ops, "textured", shape, layout, True) for shape in ((2, 12, 37), (5, 32, 32))]
    want = [_check(ops, "textured", shape, ref.LAYOUTS[2], True) for shape in ((2, 12, 37), (5, 32, 32))]
    assert all(np.array_equal(g, w) for g, w in zip(got, want))                          # the layout does not change a bit


def test_quality_of_an_image_does_not_depend_on_its_batch(env):
    ops = env[0]
    xa, xb = ref.images("textured", 7, 32, 32)
    whole = _quality(ops, xa, xb, ref.LAYOUTS[0], True)
    part = _quality(ops, xa[3:5], xb[3:5], ref.LAYOUTS[0], True)
    assert np.array_equal(whole[3:5], part)


def test_the_clip_flag_acts_on_b_only(env):
    ops = env[0]
    xa, xb = ref.images("flat", 2, 32, 32)
    assert (xb > 1).any()
    on, off = _check(ops, "flat", (2, 32, 32), ref.LAYOUTS[0], True), _check(ops, "flat", (2, 32, 32), ref.LAYOUTS[0], False)
    assert (on[:, 0] < off[:, 0]).all()
    swapped = _quality(ops, xb, xa, ref.LAYOUTS[0], True)                                 # a is never clipped: the unclipped figures
    assert np.allclose(swapped[:, 0], off[:, 0], rtol=1e-12)


# ---------------------------------------------------------------- 2. refusals
def test_refusals_enqueue_nothing(env):
    ops, _, _lib = env
    lib = _lib.load()
    a = torch.zeros((2, 12, 13, 6), dtype=F32, device="cuda")
    out = torch.full((2, 2), SENTINEL, dtype=F64, device="cuda")
    ws = torch.zeros((ops.recon_quality_workspace_bytes(2, 12, 13),), dtype=torch.uint8, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())

    def call(a_=a, b_=a, pa=6, oa=0, pb=6, ob=0, B=2, H=12, W=13, out_=out, ws_=ws, nbytes=None):
        return lib.sv_recon_quality(None if a_ is None else p(a_), pa, oa, None if b_ is None else p(b_), pb, ob, 1, B, H, W,
                                    None if out_ is None else p(out_), None if ws_ is None else p(ws_), ws.numel() if nbytes is None else nbytes, None)
    assert call() == 0
    torch.cuda.synchronize()
    assert (out != SENTINEL).all()
    out.fill_(SENTINEL)
    for kw in (dict(H=10), dict(W=10), dict(B=0), dict(pa=2), dict(pa=5, oa=3), dict(pb=5, ob=3), dict(ob=-1)):
        assert call(**kw) == _lib.STATUS_UNSUPPORTED, kw
    for kw in (dict(a_=None), dict(b_=None), dict(out_=None), dict(ws_=None)):
        assert call(**kw) == _lib.STATUS_BADARG, kw
    assert call(nbytes=ws.numel() - 1) == _lib.STATUS_WORKSPACE
    acc = torch.full((3,), SENTINEL, dtype=F64, device="cuda")
    assert lib.sv_recon_finish(p(out), 0, p(acc), None) == _lib.STATUS_UNSUPPORTED
    assert lib.sv_recon_finish(None, 2, p(acc), None) == _lib.STATUS_BADARG
    mg, z = torch.zeros((2, 8), dtype=F32, device="cuda"), torch.full((2, 8), SENTINEL, dtype=F32, device="cuda")
    assert lib.sv_recon_draw(p(mg), 8, None, 0, 3, None, 0, None, None, None, 0, p(z), 8, 0, 2, 8, 0, 1, 0, None) == _lib.STATUS_UNSUPPORTED
    assert lib.sv_recon_draw(p(mg), 8, None, 0, 1, None, 0, None, None, None, 0, p(z), 7, 0, 2, 8, 0, 1, 0, None) == _lib.STATUS_UNSUPPORTED
    assert lib.sv_recon_draw(None, 8, None, 0, 1, None, 0, None, None, None, 0, p(z), 8, 0, 2, 8, 0, 1, 0, None) == _lib.STATUS_BADARG
    assert lib.sv_recon_draw(p(mg), 8, None, 4, 1, None, 0, None, None, None, 0, p(z), 12, 0, 2, 8, 4, 1, 0, None) == _lib.STATUS_BADARG
    torch.cuda.synchronize()
    assert (out == SENTINEL).all() and (acc == SENTINEL).all() and (z == SENTINEL).all()
    for bad in (lambda: ops.recon_quality(a.double(), a), lambda: ops.recon_quality(a.cpu(), a), lambda: ops.recon_quality(a, a[:1]),
                lambda: ops.recon_quality(a, a, off_a=4), lambda: ops.recon_quality(a, a, per_image=out.float()),
                lambda: ops.recon_quality(a[..., :3], a), lambda: ops.recon_finish(out, acc[:2]), lambda: ops.recon_finish(out, acc, 3),
                lambda: ops.recon_draw(mg, None, 1, z[:, :7])):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(_lib.SplitVaeError):
        ops.recon_quality(a, a, workspace=ws[:-1])


# ---------------------------------------------------------------- 3. sv_recon_draw
def _draw_inputs(B=8, Lg=37, Ll=21, n=10, seed=0):
    rng = np.random.default_rng(seed)
    mg, ml = rng.standard_normal((B, Lg)).astype(np.float32), rng.standard_normal((B, Ll)).astype(np.float32)
    eps = rng.standard_normal((B, Lg + Ll)).astype(np.float32)
    pm, ps = rng.standard_normal((n, Lg)).astype(np.float32), rng.uniform(0.3, 2.0, (n, Lg)).astype(np.float32)
    comp = rng.integers(0, n, B).astype(np.int32)
    return mg, ml, eps, pm, ps, comp


def _zcat(B, Lc, dtype, pad=5):
    full = torch.full((B, Lc + pad), SENTINEL, dtype=dtype, device="cuda")
    return full, full[:, :Lc]


@pytest.mark.parametrize("dtype", [F32, torch.bfloat16])
def test_draw_pinned_is_bit_exact(env, dtype):
    ops, _, _lib = env
    mg, ml, eps, pm, ps, comp = _draw_inputs()
    cu = lambda a: torch.from_numpy(a).cuda()
    B, Lc = eps.shape
    for mode in (ref.MEANS, ref.KEEP_G, ref.KEEP_L):
        for prior in (None, (cu(pm), cu(ps))):
            full, z = _zcat(B, Lc, dtype)
            ops.recon_draw(cu(mg), cu(ml), mode, z, eps=cu(eps), comp=cu(comp) if prior else None, prior=prior)
            want = ref.draw(mg, ml, mode, eps, comp, pm if prior else None, ps if prior else None, bf16=dtype is torch.bfloat16)
            assert np.array_equal(z.float().cpu().numpy(), want), (mode, prior is not None)
            assert torch.equal(z, torch.from_numpy(ref.draw(mg, ml, mode, eps, comp, pm if prior else None, ps if prior else None)).cuda().to(dtype))
            assert (full[:, Lc:] == SENTINEL).all()                                       # the columns past Lg + Ll are untouched
    # the kept blocks are the means (or their bf16 rounding), the drawn ones eps
    full, z = _zcat(B, Lc, dtype)
    ops.recon_draw(cu(mg), cu(ml), ref.KEEP_G, z, eps=cu(eps))
    assert torch.equal(z[:, :37], cu(mg).to(dtype)) and torch.equal(z[:, 37:], cu(eps)[:, 37:].to(dtype))
    # Ll = 0: the one-branch model
    full, z = _zcat(B, 37, dtype)
    ops.recon_draw(cu(mg), None, ref.MEANS, z)
    assert torch.equal(z, cu(mg).to(dtype)) and (full[:, 37:] == SENTINEL).all()
    ops.recon_draw(cu(mg), None, ref.KEEP_L, z, eps=cu(eps[:, :37].copy()), comp=cu(comp), prior=(cu(pm), cu(ps)))
    assert np.array_equal(z.float().cpu().numpy(), ref.draw(mg, None, ref.KEEP_L, eps[:, :37], comp, pm, ps, bf16=dtype is torch.bfloat16))


def test_draw_unpinned_is_a_function_of_seed_image_and_mode(env):
    ops, _, _lib = env
    mg, ml, eps, pm, ps, comp = _draw_inputs(Lg=32, Ll=32)
    cu = lambda a: torch.from_numpy(a).cuda()
    g, l, prior = cu(mg), cu(ml), (cu(pm[:, :32].copy()), cu(ps[:, :32].copy()))

    def draw(mode, rows=slice(0, 8), offset=0, seed=5, prior=None):
        z = torch.empty((rows.stop - rows.start, 64), dtype=F32, device="cuda")
        return ops.recon_draw(g[rows], l[rows], mode, z, prior=prior, seed=seed, sample_offset=offset)
    for mode, pr in ((ref.KEEP_G, None), (ref.KEEP_L, None), (ref.KEEP_L, prior)):
        whole = draw(mode, prior=pr)
        assert torch.equal(whole[5:8], draw(mode, slice(5, 8), 5, prior=pr))              # image 5: row 5 of 8, or row 0 at offset 5
        assert torch.equal(whole, draw(mode, prior=pr))
        other = draw(mode, seed=6, prior=pr)
        drawn = slice(32, 64) if mode == ref.KEEP_G else slice(0, 32)
        kept = slice(0, 32) if mode == ref.KEEP_G else slice(32, 64)
        assert not (whole[:, drawn] == other[:, drawn]).any() and torch.equal(whole[:, kept], other[:, kept])
        assert torch.isfinite(whole).all()
    zl, zg = draw(ref.KEEP_G)[:, 32:], draw(ref.KEEP_L)[:, :32]
    assert not (zl == zg).any()                                                           # the modes' tags give different streams
    assert abs(float(zl.mean())) < 0.25 and 0.75 < float(zl.std()) < 1.25                # 256 standard normals
    assert torch.equal(draw(ref.MEANS), torch.cat([g, l], 1))
    # the mixture: every row is pm[c] + ps[c] * eps for ONE component c of its own, and the components vary
    big = torch.empty((64, 64), dtype=F32, device="cuda")
    ops.recon_draw(g.repeat(8, 1), l.repeat(8, 1), ref.KEEP_L, big, prior=prior, seed=5)
    e = ((big[:, None, :32] - prior[0][None]) / prior[1][None])                          # [64, n, 32]: eps under every component
    plain = torch.empty((64, 64), dtype=F32, device="cuda")
    ops.recon_draw(g.repeat(8, 1), l.repeat(8, 1), ref.KEEP_L, plain, seed=5)
    hit = ((e - plain[:, None, :32]).abs().amax(2) < 1e-4)
    assert (hit.sum(1) == 1).all() and len(set(hit.float().argmax(1).tolist())) >= 4


# ---------------------------------------------------------------- 4. sv_recon_finish
def test_finish_accumulates_in_order_and_honours_the_floor(env):
    ops = env[0]
    rng = np.random.default_rng(2)
    per = np.stack([10.0 ** rng.uniform(-6, 0, 300), rng.uniform(-0.2, 1.0, 300)], axis=1)
    per[3, 0], per[4, 0], per[5, 0] = 0.0, 1e-12, 1e-10                                  # at and under the floor: 100 dB
    flat = torch.full((9,), SENTINEL, dtype=F64, device="cuda")
    acc = flat[3:6]
    acc.zero_()
    d = torch.from_numpy(per).cuda()
    ops.recon_finish(d[:260], acc)
    first = acc.cpu().numpy()
    assert np.allclose(first, ref.finish(per[:260]), rtol=1e-12, atol=0) and first[2] == 260
    ops.recon_finish(d[260:].contiguous(), acc, 33)                                       # the first 33 of the 40 rows
    second = acc.cpu().numpy()
    assert np.allclose(second, ref.finish(per[260:293], first), rtol=1e-12, atol=0) and second[2] == 293
    assert (flat[:3] == SENTINEL).all() and (flat[6:] == SENTINEL).all()
    one = torch.zeros(3, dtype=F64, device="cuda")
    ops.recon_finish(d[3:6].contiguous(), one)
    assert np.allclose(one.cpu().numpy(), [300.0, per[3, 1] + per[4, 1] + per[5, 1], 3.0], rtol=1e-12, atol=0)
    assert not np.allclose(ref.finish(per, mutant="psnr_of_mean_mse"), ref.finish(per), rtol=1e-12, atol=0)


# ---------------------------------------------------------------- 5. the three models
H, LAT, Y = 32, 128, 10
SIZES = (4, 4, 2)
PSNR_TOL = 10.0 * np.log10(1.0 + 1e-4)                    # the MSE at rtol 1e-4, carried to every PSNR_i and so to their mean
SSIM_TOL = 1e-4


def _make(kind):
    from split_vae_amd.gm import LGGMVae
    from split_vae_amd.gmvae import GMVae
    from split_vae_amd.model import LGVae
    shape = (None, H, H, 3)
    if kind.startswith("lgvae"):
        return LGVae(LAT, LAT, image_shape=shape, dtype=kind.split("-")[1], seed=3)
    if kind.startswith("lggmvae"):
        return LGGMVae(LAT, LAT, shape, Y, 0.4, dtype=kind.split("-")[1], seed=3)
    return GMVae(LAT, shape, Y, 0.4, dtype=kind.split("-")[1], seed=3)


def _batches(seed=41):
    rng = np.random.default_rng(seed)
    t = ref._blur(rng.standard_normal((sum(SIZES), H, H, 6)))
    x = np.clip(t / np.abs(t).max(), -1, 1).astype(np.float32)
    cuts = np.cumsum((0,) + SIZES)
    return [torch.from_numpy(x[a:b]).cuda() for a, b in zip(cuts[:-1], cuts[1:])], x


def _twin_of_the_models_decode(model, kind, batches, x, eps, comp, n):
    """The figures from model.decode(...) of the same latents: dict like recon_quality.evaluate's"""
    from split_vae_amd import latent_info, recon_quality
    mu = latent_info.posteriors(model, batches, None)[0].cpu().numpy()
    one = kind.startswith("gmvae")
    mg, ml = (mu, None) if one else (mu[:, :LAT], mu[:, LAT:])
    prior = recon_quality.mixture_prior(model)
    pm, ps = (None, None) if prior is None else (prior[0].cpu().numpy(), prior[1].cpu().numpy())
    res = dict(n_images=n)
    for s, mode in (("", ref.MEANS),) if one else (("", ref.MEANS), ("_g", ref.KEEP_G), ("_l", ref.KEEP_L)):
        z = torch.from_numpy(ref.draw(mg, ml, mode, eps, comp, pm, ps)).cuda()
        per, at = [], 0
        for B in SIZES:
            zb = z[at:at + B]
            y = model.decode(zb) if one else model.decode(zb[:, :LAT].contiguous(), zb[:, LAT:].contiguous())[0]
            per.append(ref.quality(x[at:at + B], 2.0 * y.cpu().numpy().astype(np.float64) - 1.0))
            at += B
        acc = ref.finish(np.concatenate(per)[:n])
        res["psnr" + s], res["ssim" + s] = acc[0] / n, acc[1] / n
    return res


@pytest.mark.parametrize("kind", ["lgvae-f32", "lgvae-bf16", "lggmvae-f32", "lggmvae-bf16", "gmvae-f32", "gmvae-bf16"])
def test_evaluate_equals_the_twin_on_the_models_own_decode(env, deterministic, kind):
    """SVHN-32 shapes, random weights, 10 images in batches of 4 + 4 + 2, pinned eps and components: recon_quality.evaluate agrees
    with the twin applied to what model.decode returns for the same latents and to (x + 1) / 2; model._calls stays; N = 6 counts
    six images; a repeat without pinned eps gives the same figures."""
    _, recon_quality, _ = env
    model = _make(kind)
    batches, x = _batches()
    N = sum(SIZES)
    rng = np.random.default_rng(43)
    Lc = LAT if kind.startswith("gmvae") else 2 * LAT
    eps, comp = rng.standard_normal((N, Lc)).astype(np.float32), rng.integers(0, Y, N).astype(np.int32)
    model._calls = 5
    kw = dict(eps=torch.from_numpy(eps).cuda(), comp=torch.from_numpy(comp).cuda())
    for n in (N, 6):
        res = recon_quality.evaluate(model, batches, n, **kw)
        assert model._calls == 5 and res["n_images"] == n
        want = _twin_of_the_models_decode(model, kind, batches, x, eps, comp, n)
        for k in recon_quality.HISTORY_KEYS:
            if k not in want:
                assert res[k] is None and kind.startswith("gmvae"), k
                continue
            print("%s N %d %s: device %.9g twin %.9g" % (kind, n, k, res[k], want[k]))
            assert abs(res[k] - want[k]) <= (PSNR_TOL if k.startswith("psnr") else SSIM_TOL if k.startswith("ssim") else 0), (k, res[k], want[k])
    assert recon_quality.evaluate(model, batches, 500, **kw)["n_images"] == N            # clipped to what there is
    free = recon_quality.evaluate(model, batches, N)
    assert free == recon_quality.evaluate(model, batches, N) and model._calls == 5
    if not kind.startswith("gmvae"):
        assert free["psnr_g"] != recon_quality.evaluate(model, batches, N, seed=99)["psnr_g"]     # the draws follow the seed
        assert recon_quality.evaluate(model, batches, N, seed=99)["psnr"] == free["psnr"]         # the reconstruction draws nothing
    line = recon_quality.report_line(res)
    assert line.startswith("Test reconstruction quality (6 images): PSNR ") and ("z_g kept" in line) == (not kind.startswith("gmvae"))


@pytest.mark.parametrize("kind", ["lgvae-f32", "lggmvae-f32", "gmvae-f32"])
def test_a_report_between_training_steps_leaves_the_training_alone(env, deterministic, kind):
    from split_vae_amd import trainer
    from split_vae_amd.gm import train_step_lg_gm_vae
    from split_vae_amd.gmvae import train_step_gm_vae
    from split_vae_amd.optimizer import Adam
    _, recon_quality, _ = env
    step = {"lgvae-f32": trainer.train_step, "lggmvae-f32": train_step_lg_gm_vae, "gmvae-f32": train_step_gm_vae}[kind]
    batches, _ = _batches(7)
    flats = []
    for with_report in (True, False):
        model, opt = _make(kind), Adam(learning_rate=1e-3)
        step(model, batches[0], opt)
        if with_report:
            recon_quality.evaluate(model, batches, 10)
        step(model, batches[1], opt)
        torch.cuda.synchronize()
        flats.append([model.flat.clone()] + ([model.gm_flat.clone()] if hasattr(model, "gm_flat") else []))
    assert all(torch.equal(a, b) for a, b in zip(*flats))


# ---------------------------------------------------------------- 6. CLI
def _lines(out):
    return [l for l in out.splitlines() if l.startswith("Test reconstruction quality (")]


CLI = ["--synthetic", "-no_label", "--batch_size", "8", "--training_steps", "1", "--log_every", "1", "--dtype", "f32"]


def test_cli_prints_the_line_once_per_evaluation_and_evaluate_reproduces_it(env, tmp_path, monkeypatch, capsys):
    """--synthetic -no_label (32 test images): one line behind each evaluation's report, the same line from evaluate on the saved
    weights with the flag alone, the figures on evaluate's result; N above the test set is clipped with one note."""
    from split_vae_amd import evaluate, main as svmain
    monkeypatch.chdir(tmp_path)
    path = svmain.main(CLI + ["--recon_quality", "20"])
    out = capsys.readouterr().out
    lines = _lines(out)
    assert len(lines) == out.count("Training step ") >= 1 and "clipped" not in out and "Training done!" in out
    assert all(l.startswith("Test reconstruction quality (20 images): PSNR ") and "; z_g kept (z_l ~ prior): PSNR " in l and
               "; z_l kept (z_g ~ prior): PSNR " in l and l.count(" dB, SSIM ") == 3 for l in lines), out
    res = evaluate.main(CLI + ["--recon_quality", "20", "--weights", path])
    again = capsys.readouterr().out
    assert _lines(again) == [lines[-1]] and "Test IW-" not in again and "Test latent information" not in again
    assert res["recon_quality_n_images"] == 20 and "PSNR %.2f dB" % res["recon_quality_psnr"] in lines[-1]
    evaluate.main(CLI + ["--recon_quality", "500", "--latent_info", "16", "--weights", path])
    out2 = capsys.readouterr().out
    assert out2.count("Note: --recon_quality 500 clipped to the test set's 32 images") == 1 and len(_lines(out2)) == 1
    assert "(32 images)" in _lines(out2)[0] and "Test latent information (16 images" in out2


@pytest.mark.parametrize("model,parts", [("gmvae", 1), ("lggmvae", 3)])
def test_cli_mixture_models(env, tmp_path, monkeypatch, capsys, model, parts):
    from split_vae_amd import main as svmain
    monkeypatch.chdir(tmp_path)
    svmain.main(CLI + ["--model", model, "--y_size", "10", "--recon_quality", "500"])
    out = capsys.readouterr().out
    lines = _lines(out)
    assert len(lines) >= 1 and out.count("clipped to the test set's 32 images") == 1 and "Training done!" in out
    assert all(l.count(" dB, SSIM ") == parts for l in lines)
