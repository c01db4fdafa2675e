"""hipGraph replay of the step (include/splitvae.h: sv_lgvae_graph_enable) against the eager launches: same batch,
same weights, same Philox streams -> the same losses, draws and weights, step after step (the per-step scalars --
seed, step, sample offset, Adam's bias-corrected rate -- reach the captured kernels through the device record)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H, PATCH, BETA = 32, 4, 40.0


@pytest.fixture(scope="module")
def ops(lib_built):
    assert torch.cuda.is_available()
    from split_vae_amd import ops as o
    return o


def _setup(B, dtype):
    from split_vae_amd import data
    from split_vae_amd.augmentation import Augmentator
    from split_vae_amd.model import LGVae
    from split_vae_amd.optimizer import Adam
    model = LGVae(128, 128, image_shape=[-1, H, H, 3], dtype=dtype, device=torch.device("cuda"), seed=11)
    model.beta = BETA
    x = data.synthetic_images(B, H, H, seed=0, device="cuda")
    images = Augmentator("scramble", size=PATCH, seed=1).augment(x)
    return model, Adam(learning_rate=1e-3), images


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_replayed_steps_equal_eager_steps(ops, dtype, monkeypatch):
    from split_vae_amd import trainer
    monkeypatch.setenv("SV_GRAPH", "1")                              # LGVae.plan() enables replay on its plans
    B, steps = 16, 6
    eager, opt_e, images = _setup(B, dtype)
    twin, opt_t, _ = _setup(B, dtype)             # a second eager run: the run-to-run noise floor (fp32 atomics reorder sums)
    graph, opt_g, _ = _setup(B, dtype)
    assert torch.equal(eager.flat, graph.flat)
    side = torch.cuda.Stream()
    hist = []
    for t in range(steps):
        pe = trainer.train_step(eager, images, opt_e)                 # legacy default stream: never captured
        le = pe.buffer("losses", torch.float32, (8,)).clone()
        eps_e = pe.buffer("eps_x", torch.float32, (B, 128)).clone()
        trainer.train_step(twin, images, opt_t)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            pg = trainer.train_step(graph, images, opt_g)
            lg = pg.buffer("losses", torch.float32, (8,)).clone()
            eps_g = pg.buffer("eps_x", torch.float32, (B, 128)).clone()
        side.synchronize()
        assert torch.equal(eps_e, eps_g), t                           # the replay drew THIS step's noise
        hist.append(eps_g)
        rt = 2e-4 if dtype == "f32" else 3e-3           # bf16: the two trajectories drift apart step by step (see below)
        torch.testing.assert_close(lg[:6], le[:6], rtol=rt, atol=rt)
        # Run-to-run noise floor: the split-K atomics of the heads reorder fp32 sums, a last-bit change of z can flip a
        # bf16 rounding or a ReLU mask downstream, and Adam normalises every element (an element whose gradient is
        # noise moves by +-lr either way).  Two eager runs differ the same way (scripts/dbg_graph.py); a wrong
        # per-step scalar (stale Adam rate, stale seed) would move EVERY element, which is what this guards.
        d, d0 = (graph.flat - eager.flat).abs(), (twin.flat - eager.flat).abs()
        assert float(d.max()) <= 2.1e-3 * (t + 1), (t, float(d.max()))
        frac, frac0 = float((d > 1e-5).float().mean()), float((d0 > 1e-5).float().mean())
        # (two eager runs share one launch schedule and are often bit-identical; the replay runs the weight gradients on
        # the main stream, another valid order of the same atomics, and bf16 + Adam's sign-like update amplify it: 2-14 %
        # of the elements were seen to sit more than 1e-5 apart by the third step (scripts/dbg_e3race.py: the gradients of
        # the two schedules agree to 1e-5 relative, like two runs of one schedule); a stale scalar gives ~100 %)
        assert frac <= 3 * frac0 + (2e-2 if dtype == "f32" else 0.3), (t, frac, frac0)
    assert pe.graph_count() == 0 and pg.graph_count() == 1            # eager / eager, capture, then replays
    assert not torch.equal(hist[2], hist[3])                          # consecutive replays draw different noise
    assert np.isfinite(float(lg[5]))


def test_split_phase_replay_matches_one_call(ops):
    """The data-parallel trainer issues the step as four phase groups (all-reduces in between): each group is its own
    graph; the sequence equals the single PHASE_ALL call."""
    from split_vae_amd._lib import (PHASE_ALL, PHASE_PREP, PHASE_FORWARD, PHASE_LOSS, PHASE_BWD_DECODERS, PHASE_BWD_ENC_HEADS,
                                    PHASE_BWD_ENC_CONVS, PHASE_ADAM)
    B = 8
    ref, _, images = _setup(B, "f32")
    P0 = ref.flat.clone()
    side = torch.cuda.Stream()
    groups = [PHASE_PREP | PHASE_FORWARD | PHASE_LOSS | PHASE_BWD_DECODERS, PHASE_BWD_ENC_HEADS, PHASE_BWD_ENC_CONVS, PHASE_ADAM]

    def run(split, use_graph, steps=5):
        plan = ops.LGVaePlan(B, H, H, beta=BETA, dtype=torch.float32)
        plan.graph_enable(use_graph)
        P, G, M, V = P0.clone(), torch.zeros_like(P0), torch.zeros_like(P0), torch.zeros_like(P0)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for t in range(1, steps + 1):
                kw = dict(params=P, grads=G, adam_m=M, adam_v=V, images6=images, seed=3, step=t, lr=1e-3, t=t)
                for ph in (groups if split else [PHASE_ALL]):
                    plan.step(ph, **kw)
        side.synchronize()
        return P, plan.graph_count()

    Pa, na = run(False, False)
    Pb, nb = run(True, True)
    Pc, nc = run(False, True)
    assert (na, nb, nc) == (0, 4, 1)
    for Px in (Pb, Pc):
        d = (Px - Pa).abs()
        assert float(d.max()) <= 1.1e-2 and float((d > 1e-5).float().mean()) < 2e-2, (float(d.max()), float((d > 1e-5).float().mean()))


def test_replay_sees_a_changed_learning_rate(ops):
    """lr and t are per-step values of a captured step (ExponentialDecay in vae/main.py:66-69 changes lr between steps)."""
    from split_vae_amd._lib import PHASE_ALL
    B = 4
    ref, _, images = _setup(B, "f32")
    side = torch.cuda.Stream()
    out = {}
    for use_graph in (False, True):
        plan = ops.LGVaePlan(B, H, H, beta=BETA, dtype=torch.float32)
        plan.graph_enable(use_graph)
        P, G, M, V = ref.flat.clone(), torch.zeros_like(ref.flat), torch.zeros_like(ref.flat), torch.zeros_like(ref.flat)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for t, lr in enumerate([1e-3, 1e-3, 1e-3, 4e-4, 1.6e-4], start=1):
                plan.step(PHASE_ALL, params=P, grads=G, adam_m=M, adam_v=V, images6=images, seed=3, step=t, lr=lr, t=t)
        side.synchronize()
        out[use_graph] = P
    d = (out[True] - out[False]).abs()
    assert float(d.max()) <= 1.1e-2 and float((d > 1e-5).float().mean()) < 2e-2, (float(d.max()), float((d > 1e-5).float().mean()))


def test_replay_restores_the_host_flags_the_phases_leave_behind(ops):
    """a replayed graph must leave the plan's host-side state (the latent block's DzState of csrc/plan_latent.h -- zeroed, stale,
    in gz_*, in slabs -- and nll_fused) as the captured phases left it -- it selects which buffer the next phase's reparam_kl_bwd reads.  Scenario: whole
    training steps (the slab path is live, the dz slabs hold a real gradient: InSlabs), then a REPLAYED forward-only call (Stale) followed by an EAGER encoder
    backward without the decoders' (the KL terms' gradient only, vae/trainer.py:12-13).  With the state of before the replay that backward reads the heads' forward slabs as dz.
    The encoder_x_hat head-bias gradients have a closed form in z_mean / z_sig."""
    from split_vae_amd import data
    from split_vae_amd._lib import PHASE_ALL, PHASE_PREP, PHASE_FORWARD, PHASE_LOSS, PHASE_BWD_ENC_HEADS, PHASE_BWD_ENC_CONVS
    from split_vae_amd.augmentation import Augmentator
    from split_vae_amd.model import LGVae
    B, Hc, beta = 256, 64, 120.0
    x = data.synthetic_images(B, Hc, Hc, seed=0, device="cuda")
    img = Augmentator("scramble", size=8, seed=1).augment(x)
    m = LGVae(128, 128, image_shape=[-1, Hc, Hc, 3], dtype="bf16", device=torch.device("cuda"), seed=3)
    plan = ops.LGVaePlan(B, Hc, Hc, beta=beta, dtype=torch.bfloat16)
    plan.graph_enable(True)
    P, G, M, V = m.flat.clone(), torch.zeros_like(m.flat), torch.zeros_like(m.flat), torch.zeros_like(m.flat)
    fwd = PHASE_PREP | PHASE_FORWARD | PHASE_LOSS
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for t in range(1, 4):                                     # eager, capture, replay: whole steps
            plan.step(PHASE_ALL, params=P, grads=G, adam_m=M, adam_v=V, images6=img, seed=3, step=t, lr=1e-4, t=t)
        for t in range(4, 7):                                     # forward-only: eager, capture, REPLAY -- each followed by the KL-only backward
            plan.step(PHASE_ALL, params=P, grads=G, adam_m=M, adam_v=V, images6=img, seed=3, step=t, lr=1e-4, t=t)
            plan.step(fwd, params=P, grads=G, images6=img, seed=3, step=100 + t)
            G.zero_()
            plan.step(PHASE_BWD_ENC_HEADS | PHASE_BWD_ENC_CONVS, params=P, grads=G, images6=img, seed=3, step=100 + t)
            side.synchronize()
            zm = plan.buffer("z_mean_xh", torch.float32, (B, 128)).double()
            zs = plan.buffer("z_sig_xh", torch.float32, (B, 128)).double()
            ks = beta / B
            want_mean = (ks * zm).sum(0)
            want_sd = (ks * (zs - 1.0 / zs) * (1.0 - torch.exp(-zs))).sum(0)
            g = {n: G[o:o + int(np.prod(sh))].view(*sh) for n, o, sh in m.param_table}
            gm, gs = g["encoder_x_hat/e4_mean/bias"].double(), g["encoder_x_hat/e4_sd/bias"].double()
            assert float((gm - want_mean).abs().max()) <= 2e-2 * float(want_mean.abs().max()) + 1e-6, t
            assert float((gs - want_sd).abs().max()) <= 2e-2 * float(want_sd.abs().max()) + 1e-6, t
    assert plan.graph_count() >= 2


def test_capture_that_forks_to_the_side_streams_replays_the_same_step(lib_built):
    """SV_GRAPH_SIDE=1 (opt-in): the captured step forks to the weight-gradient side streams -- every fork / join on its own event, only the streams the call
    used joined back.  Round 3's capture (one re-recorded fork event, every stream joined) replayed corrupt gradients on ROCm 7.2; this form must replay the
    eager step BIT FOR BIT (the bf16 step is bit-reproducible): equal parameter hashes after 30 steps, in fresh processes.  (It is not the default: the replay of a
    multi-stream graph is 2.5x slower than the eager launches on this runtime, profiles/r06_graph_side.txt.)"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = {}
    for mode in ("eager", "graph_side", "early_side"):
        r = subprocess.run([sys.executable, os.path.join(root, "scripts", "r06_graph_side.py"), mode, "bf16", "16", "30"], capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
        assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
        line = [ln for ln in r.stdout.splitlines() if ln.startswith(mode)][-1].split()
        out[mode] = (line[line.index("params") + 1], int(line[line.index("ms/step") + 1].split("=")[1]))
    assert out["eager"][0] == out["graph_side"][0], out
    assert out["eager"][1] == 0 and out["graph_side"][1] == 1, out           # eager: no graph; replay: one captured graph
    # SV_EARLY_SIDE=1 (opt-in too: no gain measured): the decoders' weight images and the gradient zero fill on side stream 0 beside the encoders' forward
    assert out["eager"][0] == out["early_side"][0] and out["early_side"][1] == 0, out
