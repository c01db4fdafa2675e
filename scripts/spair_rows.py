"""One run of bench.py's SPLIT-SPAIR rows on the tree given as argv[1] (its own bench.py and library); prints one JSON line."""
import json
import os
import sys

root = os.path.abspath(sys.argv[1])
os.chdir(root)
sys.path.insert(0, root)
import bench  # noqa: E402  (configures the hardware queues on import, as the benchmark does)
import split_vae_amd  # noqa: E402
assert os.path.abspath(os.path.dirname(split_vae_amd.__file__)) == os.path.join(root, "split_vae_amd"), split_vae_amd.__file__
import torch  # noqa: E402
dev = torch.device("cuda:0")
out = {"tree": sys.argv[2]}
for name, which in (("lg_spair_b32", "hard"), ("lg_spair_easy_b32", "easy")):
    r = bench.spair_row(dev, which)
    for dt in ("f32", "bf16"):
        out["%s_%s" % (name, dt)] = {"ms": r[dt]["ms_per_step"], "blocks": r[dt]["blocks_ms"]}
print(json.dumps(out), flush=True)
