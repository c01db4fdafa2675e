"""Cost of the mixture models' importance-weighted bound (split_vae_amd/iw.py: mixture_log_likelihood) beside their test steps, on the
same batch, in ONE process, and of sv_iw_gm_advance alone beside sv_iw_advance alone.

Rows: SVHN-32 B = 64, fp32 and bf16, LGGMVae and GMVae.  Per row, after warm-up, between hipEvent pairs:

  test_step_ms   one gm.test_step_lg_gm_vae / gmvae.test_step_gm_vae (both encoders, decoders, loss, the metric launch), mean of
                 `--steps` calls
  iw_total_ms    one mixture_log_likelihood call at K = `--k-lo` and at K = `--k-hi` (encoders and tables once, K sample passes, finish)
  iw_sample_ms   the marginal time per (batch, sample): (t(k-hi) - t(k-lo)) / (k-hi - k-lo), k-hi - k-lo >= 50: one decoder + loss
                 pass and one sv_iw_gm_advance launch
  decoder_pass_ms  the plan's FWD_DECODERS | LOSS pass alone, mean of `--steps` back-to-back calls
  tables_ms      sv_iw_gm_tables alone (once per batch)

Kernel rows (Lg = Ll = 128, 30 components, B = 64, fp32 and bf16 zcat): `--steps` back-to-back draw + accumulate launches of
sv_iw_gm_advance and of sv_iw_advance on the same stream: the mean time of one launch in a dependent chain.

Each figure is the median of `--rounds` rounds; `spread` = (max - min) / median.

    python scripts/bench_iw_gm.py [--steps 50] [--rounds 5] [--out profiles/iw_gm_bench.json]

`--test-step-only --tree DIR` times the test steps alone with split_vae_amd imported from another checkout (the parent commit,
built, in the same visit); `--parent-json FILE` embeds that run's rows so one file holds both.
"""
import argparse
import json
import os
import statistics
import sys

ROWS = (("lggmvae", "f32"), ("lggmvae", "bf16"), ("gmvae", "f32"), ("gmvae", "bf16"))
H, B, PATCH, BETA, N_COMP, TAU, L = 32, 64, 4, 40.0, 30, 0.4, 128


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


def med(v):
    m = statistics.median(v)
    return dict(ms=round(m, 5), spread=round((max(v) - min(v)) / m, 4))


def run_row(name, dtype, a):
    from split_vae_amd import data, gm, gmvae
    from split_vae_amd.augmentation import Augmentator
    if name == "lggmvae":
        model = gm.LGGMVae(L, L, [-1, H, H, 3], N_COMP, TAU, dtype=dtype, device="cuda", seed=3)
        step = lambda: gm.test_step_lg_gm_vae(model, images)     # noqa: E731
    else:
        model = gmvae.GMVae(L, [-1, H, H, 3], N_COMP, TAU, dtype=dtype, device="cuda", seed=3)
        step = lambda: gmvae.test_step_gm_vae(model, images)     # noqa: E731
    model.beta = BETA
    images = Augmentator("scramble", size=PATCH, seed=1).augment(data.synthetic_images(B, H, H, seed=0, device="cuda"))
    row = dict(model=name, dataset="svhn", H=H, B=B, dtype=dtype, steps=a.steps, rounds=a.rounds)
    if a.test_step_only:
        timed(step, 5)
        row["test_step"] = med([timed(step, a.steps) for _ in range(a.rounds)])
        return row
    from split_vae_amd import _lib, iw, ops
    lo = lambda: iw.mixture_log_likelihood(model, images, a.k_lo)    # noqa: E731
    hi = lambda: iw.mixture_log_likelihood(model, images, a.k_hi)    # noqa: E731
    plan, enc = model.plan(B), model.encoder(B)
    dec = lambda: plan.step(_lib.PHASE_FWD_DECODERS | _lib.PHASE_LOSS, params=model.flat, images6=images)     # noqa: E731
    P = iw._gm_params(model)
    tab_out = ops.iw_gm_tables(enc.buf["he"], *P["ht"], *P["zm"], *P["zs"], *P["pm"], *P["ps"])
    tab = lambda: ops.iw_gm_tables(enc.buf["he"], *P["ht"], *P["zm"], *P["zs"], *P["pm"], *P["ps"], out=tab_out)    # noqa: E731
    timed(step, 5), timed(lo, 2), timed(hi, 1), timed(dec, 5), timed(tab, 5)
    ts, tl, th, td, tt = [], [], [], [], []
    for _ in range(a.rounds):
        ts.append(timed(step, a.steps))
        tl.append(timed(lo))
        th.append(timed(hi))
        td.append(timed(dec, a.steps))
        tt.append(timed(tab, a.steps))
    row["test_step"] = med(ts)
    row["iw_total_k%d" % a.k_lo], row["iw_total_k%d" % a.k_hi] = med(tl), med(th)
    row["iw_sample"] = med([(h - l) / (a.k_hi - a.k_lo) for h, l in zip(th, tl)])
    row["decoder_pass"], row["tables"] = med(td), med(tt)
    row["iw_sample_over_test_step"] = round(row["iw_sample"]["ms"] / row["test_step"]["ms"], 4)
    Lj, Lx, el = iw.mixture_log_likelihood(model, images, a.k_lo)
    row["check"] = dict(gm_iw_joint=float(Lj.double().mean()), gm_iw_x=float(Lx.double().mean()), gm_elbo=float(el.double().mean()))
    return row


def run_kernels(dtype, a):
    """sv_iw_gm_advance and sv_iw_advance alone: draw + accumulate launches back to back."""
    import torch
    from split_vae_amd import _lib, ops
    f32 = torch.float32
    g = torch.Generator(device="cuda").manual_seed(0)
    rn = lambda *s: torch.randn(s, dtype=f32, device="cuda", generator=g)             # noqa: E731
    sg = lambda *s: torch.rand(s, dtype=f32, device="cuda", generator=g) * 1.5 + 0.3   # noqa: E731
    logits, zm_all, zs_all, pm, ps = rn(B, N_COMP), rn(B, N_COMP, L), sg(B, N_COMP, L), rn(N_COMP, L), sg(N_COMP, L)
    mu_g, sg_g, mu_l, sg_l = rn(B, L), sg(B, L), rn(B, L), sg(B, L)
    zcat = torch.zeros((B, 2 * L), dtype={"f32": f32, "bf16": torch.bfloat16}[dtype], device="cuda")
    r, comp_out = torch.zeros(B, dtype=f32, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
    nll = torch.full((B,), 1.7e4, dtype=f32, device="cuda")
    state = torch.zeros((B, 5), dtype=torch.float64, device="cuda")
    fl = _lib.IW_ACCUMULATE | _lib.IW_DRAW
    new = lambda: ops.iw_gm_advance(logits, zm_all, zs_all, pm, ps, mu_l, sg_l, zcat, r, comp_out, 1, fl, nll_x=nll, nll_xh=nll, state=state)   # noqa: E731
    old = lambda: ops.iw_advance(mu_g, sg_g, mu_l, sg_l, zcat, r, 1, fl, nll_x=nll, nll_xh=nll, state=state)                                  # noqa: E731
    timed(new, 10), timed(old, 10)
    tn, to = [], []
    for _ in range(a.rounds):
        tn.append(timed(new, a.steps))
        to.append(timed(old, a.steps))
    return dict(kernels="sv_iw_gm_advance vs sv_iw_advance", B=B, Lg=L, Ll=L, components=N_COMP, zcat=dtype, sv_iw_gm_advance=med(tn),
                sv_iw_advance=med(to), ratio=round(statistics.median(tn) / statistics.median(to), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--k-lo", type=int, default=8)
    ap.add_argument("--k-hi", type=int, default=72)
    ap.add_argument("--test-step-only", action="store_true")
    ap.add_argument("--tree", type=str, default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--parent-json", type=str, default=None)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if a.k_hi - a.k_lo < 50:
        raise SystemExit("--k-hi - --k-lo must be at least 50 samples")
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch
    import split_vae_amd
    split_vae_amd.configure_hw_queues()
    if not torch.cuda.is_available():
        raise SystemExit("bench_iw_gm.py needs the GPU: no timing without one")
    rows = []
    for r in ROWS:
        rows.append(run_row(*r, a))
        print(json.dumps(rows[-1]), flush=True)
    out = dict(tree=os.path.basename(os.path.abspath(a.tree)) if a.test_step_only else "this commit",
               device=torch.cuda.get_device_name(0), timing="hipEvent pairs, median over rounds", rows=rows)
    if not a.test_step_only:
        out["kernel_rows"] = [run_kernels(dt, a) for dt in ("f32", "bf16")]
    if a.parent_json:
        with open(a.parent_json) as f:
            out["parent_commit_test_step"] = json.load(f)["rows"]
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
