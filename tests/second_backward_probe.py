"""Probe of tests/test_gpu_step.py::test_second_backward_over_one_forward_recomputes_dz: two warm-up training steps on one plan (the latent block's launch
forms are latched), then forward + loss, the decoders' backward and the encoders' backward as separate phase calls, then loss and both backward phases AGAIN
over the same forward.  The second backward must recompute dL/dz, not add to the first one's.  Prints one JSON line: whether the two gradient sets are bitwise
equal, and per parameter tensor max |g2 - g1| / max |g1|.  usage: python tests/second_backward_probe.py  (switches in the environment, read fresh)"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import split_vae_amd                                                 # noqa: E402
split_vae_amd.configure_hw_queues()                                  # the library's queue setting, before the first HIP call
from split_vae_amd import data, trainer                              # noqa: E402
from split_vae_amd._lib import (PHASE_PREP, PHASE_FORWARD, PHASE_LOSS, PHASE_BWD_DECODERS, PHASE_BWD_ENC_HEADS,   # noqa: E402
                                PHASE_BWD_ENC_CONVS)
from split_vae_amd.augmentation import Augmentator                   # noqa: E402
from split_vae_amd.model import LGVae                                # noqa: E402
from split_vae_amd.optimizer import Adam                             # noqa: E402


def main():
    B, H = 8, 32
    x = data.synthetic_images(B, H, H, seed=0, device="cuda")
    img = Augmentator("scramble", size=4, seed=1).augment(x)
    m = LGVae(128, 128, image_shape=[-1, H, H, 3], dtype="f32", device=torch.device("cuda"), seed=3)
    m.beta = 40.0
    opt = Adam(learning_rate=1e-4)
    for _ in range(2):
        plan = trainer.train_step(m, img, opt)
    kw = dict(params=m.flat, grads=m.grad_flat, images6=img, seed=m.seed, step=7)

    def backward(first):
        plan.step((PHASE_PREP | PHASE_FORWARD | PHASE_LOSS) if first else PHASE_LOSS, **kw)
        plan.step(PHASE_BWD_DECODERS, **kw)
        plan.step(PHASE_BWD_ENC_HEADS | PHASE_BWD_ENC_CONVS, **kw)
        torch.cuda.synchronize()
        return m.grad_flat.clone()

    g1, g2 = backward(True), backward(False)
    per = {}
    for name, off, shape in m.param_table:
        n = 1
        for s in shape:
            n *= int(s)
        a, b = g1[off:off + n].double(), g2[off:off + n].double()
        per[name] = [float((b - a).abs().max()), float(a.abs().max())]
    print("SECOND_BACKWARD " + json.dumps({"bitwise": bool(torch.equal(g1, g2)), "finite": bool(torch.isfinite(g1).all() and torch.isfinite(g2).all()),
                                           "per": per}))


if __name__ == "__main__":
    main()
