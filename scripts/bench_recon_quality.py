"""Cost of the label-free reconstruction quality report (split_vae_amd/recon_quality.py, csrc/recon_quality.hip), in ONE process.

1. sv_recon_quality alone, at CelebA-64 B = 512 and SVHN-32 B = 64: the image from channels 0..2 of a six-channel batch against
   channels 0..2 of a six-channel decoder output, both read in place (pitch 6).  Between hipEvent pairs, after warm-up:

     kernel_ms  one ops.recon_quality call (the tile kernel and the per-image kernel; output and workspace allocated outside).  The
                call rotates over `--sets` pairs of buffers so that a timed call does not find its input in the 256 MB Infinity
                Cache (512 x 64 x 64 x 6 floats are 50 MB per buffer); `bytes` = 2 B H W 24: the strided reads pull whole 24-byte
                pixels; `hbm_fraction` = bytes / kernel_ms over 6.3e12 B/s, the achievable HBM rate of the guide (8e12 B/s is the spec)
     torch_ms   the same definition as a torch composition on the device, fp32: slice, rescale, clamp, five depthwise conv2d passes
                with the 11 x 11 window (a, b, a^2, b^2, a b), the SSIM map, the means
     max_abs_diff of the two per-image (MSE, SSIM) results

2. The whole report per evaluation of an SVHN-32 LGVae (`--dtype`, 128 + 128 latents, batch 64, `--batches` batches): the encoders
   once per batch, then per variant sv_recon_draw, the decoders, sv_recon_quality, sv_recon_finish; host clock around the call (it ends
   in its one read-back).  `test_step_ms`: one trainer.test_step pass over the same batches in the same process (`--test-step-only`
   prints that alone: run from a checkout of the parent commit, its figure is folded in with `--merge parent=FILE`).
   `new_kernels_ms`: the three variants' draw + quality + finish calls alone on one batch, between hipEvent pairs, times the
   number of batches; `new_kernels_share` = that over report_ms.

Each figure is the median of `--rounds` blocks of `--calls` calls; `spread` = (max - min) / median.  SV_LIB_NAME selects another
build of the library (an A/B build of a kernel variant): `lib` records which one ran; `--kernel-only` then times part 1 without torch.

    python scripts/bench_recon_quality.py [--rounds 5] [--calls 20] [--out profiles/recon_quality_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

HBM_ACHIEVABLE, HBM_SPEC = 6.3e12, 8.0e12
SHAPES = (("celeba64", 512, 64), ("svhn32", 64, 32))


def timed(fn, n=1):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def wall(fn):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def med(v):
    m = statistics.median(v)
    return dict(ms=round(m, 4), spread=round((max(v) - min(v)) / m, 4))


def window2d():
    import torch
    from split_vae_amd import ops
    g = torch.tensor(ops.recon_window(), dtype=torch.float32, device="cuda")
    return torch.outer(g, g)[None, None].repeat(3, 1, 1, 1)


def torch_quality(a6, b6, win):
    """per_image [B,2] of the same definition as a torch composition, fp32"""
    import torch
    import torch.nn.functional as F
    a = ((a6[..., :3] + 1) * 0.5).permute(0, 3, 1, 2)
    b = torch.clamp((b6[..., :3] + 1) * 0.5, 0., 1.).permute(0, 3, 1, 2)
    mse = ((a - b) ** 2).flatten(1).mean(1)
    ma, mb, saa, sbb, sab = (F.conv2d(v, win, groups=3) for v in (a, b, a * a, b * b, a * b))
    va, vb, cov = saa - ma * ma, sbb - mb * mb, sab - ma * mb
    s = ((2 * ma * mb + 1e-4) * (2 * cov + 9e-4)) / ((ma * ma + mb * mb + 1e-4) * (va + vb + 9e-4))
    return torch.stack([mse, s.flatten(1).mean(1)], dim=1)


def kernel_row(name, B, H, a):
    import torch
    from split_vae_amd import ops
    gen = torch.Generator(device="cuda").manual_seed(B + H)
    sets = max(1, a.sets if B * H * H * 24 > (8 << 20) else 1)
    bufs = []
    for _ in range(sets):
        x = torch.rand((B, H, H, 6), generator=gen, device="cuda") * 2 - 1
        bufs.append((x, (x + 0.3 * torch.randn((B, H, H, 6), generator=gen, device="cuda")).contiguous()))
    per = torch.empty((B, 2), dtype=torch.float64, device="cuda")
    ws = torch.empty((ops.recon_quality_workspace_bytes(B, H, H),), dtype=torch.uint8, device="cuda")
    turn = [0]

    def ours():
        x, y = bufs[turn[0] % sets]
        turn[0] += 1
        ops.recon_quality(x, y, per_image=per, workspace=ws)
    timed(ours, 2 * sets)
    nbytes = 2 * B * H * H * 24
    row = dict(shape=name, B=B, H=H, W=H, bytes=nbytes, buffer_sets=sets)
    if a.kernel_only:
        tk = [timed(ours, a.calls) for _ in range(a.rounds)]
        row["kernel"] = med(tk)
    else:
        win = window2d()
        turn_t = [0]

        def theirs():
            x, y = bufs[turn_t[0] % sets]
            turn_t[0] += 1
            return torch_quality(x, y, win)
        timed(theirs, 2)
        tk, tt = [], []
        for _ in range(a.rounds):
            tk.append(timed(ours, a.calls))
            tt.append(timed(theirs, a.torch_calls))
        row["kernel"], row["torch"] = med(tk), med(tt)
        row["torch_over_kernel"] = round(row["torch"]["ms"] / row["kernel"]["ms"], 2)
        ops.recon_quality(bufs[0][0], bufs[0][1], per_image=per, workspace=ws)
        row["max_abs_diff"] = float((per - torch_quality(bufs[0][0], bufs[0][1], win).double()).abs().max())
    rate = nbytes / (row["kernel"]["ms"] * 1e-3)
    row["bytes_per_s"] = round(rate, 0)
    row["hbm_fraction"], row["hbm_fraction_of_spec"] = round(rate / HBM_ACHIEVABLE, 4), round(rate / HBM_SPEC, 4)
    return row


def make_model(a):
    import torch
    from split_vae_amd.model import LGVae
    model = LGVae(128, 128, image_shape=(None, 32, 32, 3), dtype=a.dtype, seed=1)
    gen = torch.Generator(device="cuda").manual_seed(7)
    batches = [torch.rand((64, 32, 32, 6), generator=gen, device="cuda") * 2 - 1 for _ in range(a.batches)]
    return model, batches


def test_step_pass(model, batches):
    from split_vae_amd import trainer
    for x in batches:
        trainer.test_step(model, x)


def test_step_row(a):
    model, batches = make_model(a)
    wall(lambda: test_step_pass(model, batches))
    return dict(model="lgvae", dtype=a.dtype, batch=64, batches=a.batches, test_step=med([wall(lambda: test_step_pass(model, batches))
                                                                                         for _ in range(a.rounds)]))


def report_row(a):
    import torch
    from split_vae_amd import latent_info, ops, recon_quality
    from split_vae_amd._lib import RECON_KEEP_G, RECON_KEEP_L, RECON_MEANS
    model, batches = make_model(a)
    n = 64 * a.batches
    whole = lambda: recon_quality.evaluate(model, batches, n)                     # noqa: E731
    wall(whole), wall(lambda: test_step_pass(model, batches))
    tr, ts = [], []
    for _ in range(a.rounds):
        tr.append(wall(whole))
        ts.append(wall(lambda: test_step_pass(model, batches)))
    # the new kernels alone, on one batch: three variants of draw + quality + finish
    mg, _, ml, _ = latent_info.batch_posterior(model, batches[0])
    plan = model.plan(64)
    zcat, out6 = plan.buffer("zcat", model.dtype, (64, 256)), plan.buffer("out6_x", torch.float32, (64, 32, 32, 6))
    per = torch.empty((64, 2), dtype=torch.float64, device="cuda")
    ws = torch.empty((ops.recon_quality_workspace_bytes(64, 32, 32),), dtype=torch.uint8, device="cuda")
    acc = torch.zeros((3, 3), dtype=torch.float64, device="cuda")

    def new_kernels():
        with ops.hold_stream():
            for v, mode in enumerate((RECON_MEANS, RECON_KEEP_G, RECON_KEEP_L)):
                ops.recon_draw(mg, ml, mode, zcat, seed=1)
                ops.recon_quality(batches[0], out6, per_image=per, workspace=ws)
                ops.recon_finish(per, acc[v])
    timed(new_kernels, 3)
    tn = [timed(new_kernels, a.calls) * a.batches for _ in range(a.rounds)]
    row = dict(model="lgvae", dtype=a.dtype, batch=64, batches=a.batches, images=n, report=med(tr), test_step=med(ts), new_kernels=med(tn),
               figures=recon_quality.evaluate(model, batches, n))
    row["report_over_test_step"] = round(row["report"]["ms"] / row["test_step"]["ms"], 2)
    row["new_kernels_share"] = round(row["new_kernels"]["ms"] / row["report"]["ms"], 4)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--torch-calls", type=int, default=3)
    ap.add_argument("--sets", type=int, default=8)
    ap.add_argument("--batches", type=int, default=64)
    ap.add_argument("--dtype", type=str, default="f32", choices=["f32", "bf16"])
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--test-step-only", action="store_true")
    ap.add_argument("--merge", action="append", default=[], help="name=FILE: fold the JSON of another run in under `name`")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import split_vae_amd
    from split_vae_amd import _lib
    split_vae_amd.configure_hw_queues()
    if not torch.cuda.is_available():
        raise SystemExit("bench_recon_quality.py needs the GPU: no timing without one")
    out = dict(device=torch.cuda.get_device_name(0), lib=os.path.basename(_lib.LIB_PATH),
               timing="hipEvent pairs (kernel, torch, new_kernels) / host clock around a synchronised call (report, test_step); "
                      "median over rounds of blocks of calls", hbm_bytes_per_s=dict(achievable=HBM_ACHIEVABLE, spec=HBM_SPEC))
    if a.test_step_only:
        out["test_step_pass"] = test_step_row(a)
    else:
        out["kernel_rows"] = []
        for name, B, H in SHAPES:
            out["kernel_rows"].append(kernel_row(name, B, H, a))
            print(json.dumps(out["kernel_rows"][-1]), flush=True)
        if not a.kernel_only:
            out["report"] = report_row(a)
    for m in a.merge:
        name, path = m.split("=", 1)
        with open(path) as f:
            out[name] = json.load(f)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
