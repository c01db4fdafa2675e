"""Generates tests/golden/wprep_elems.json: the sizes of the prepared conv weight images and of the conv workspaces, descriptor by descriptor.

For each descriptor: sv_conv2d_wprep_elems(d, 0), sv_conv2d_wprep_elems(d, 1) and the four workspace-size queries (forward, weight gradient,
low-res input gradient, polyphase weight gradient).  Host-only.  Three groups:
  grid   every descriptor of tests/test_abi.py's conv_domain_grid(), in grid order.  The 17 280 accepted ones take only a few dozen distinct
         answers, so the file keeps one letter per descriptor ("." = refused: every query answers -1): "sizes" lists the distinct answers,
         "blocks" the distinct strings of GRID_BLOCK consecutive descriptors, "index" which block each stretch of the grid is;
  cases  every descriptor of tests/test_gpu_conv_api.py's CASES;
  layers the nine layer descriptors of the LGVAE plan (e1, e2, e3, head, d1 .. d5 of the x network) at (B, H) = (2, 32) and (64, 64), both
         dtypes, ups_in as the plan sets it.
The last two groups reach the space-to-depth, x-packed and polyphase images; the grid reaches none of them.
tests/test_abi.py::test_weight_image_sizes_are_pinned compares the built library with the file, entry by entry.

The file records the commit it was taken from (the commit BEFORE the weight-image layout table replaced the hand-written sums); regenerate it
only when a change of an image's size is intended.

Run from the repo root:  python tests/golden/make_golden_wprep_elems.py [COMMIT]     (COMMIT: what the loaded library was built from; default HEAD)
"""
import ctypes as C
import importlib.util
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from split_vae_amd import _lib  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "wprep_elems.json")
LAYER_SHAPES = [(2, 32), (64, 64)]     # (B, H = W)
LATENT = 128


def _test_module(name):
    spec = importlib.util.spec_from_file_location("_golden_" + name, os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def queries(lib, d):
    """d: the 14 fields of sv_conv_desc"""
    cd = _lib.ConvDesc(*d)
    return [lib.sv_conv2d_wprep_elems(C.byref(cd), 0), lib.sv_conv2d_wprep_elems(C.byref(cd), 1), lib.sv_conv2d_fwd_workspace_bytes(C.byref(cd)),
            lib.sv_conv2d_wgrad_workspace_bytes(C.byref(cd)), lib.sv_conv2d_dgrad_lowres_workspace_bytes(C.byref(cd)),
            lib.sv_conv2d_wgrad_poly_workspace_bytes(C.byref(cd))]


def grid_descs():
    for B, H, W, Cin, Cout, KH, KW, s, dtype, ldx, ldy, y_f32, ups in _test_module("test_abi").conv_domain_grid():
        yield [B, H, W, Cin, Cout, KH, KW, s, 0, dtype, ldx, ldy, y_f32, ups]


def case_descs():
    mod = _test_module("test_gpu_conv_api")
    for c in mod.CASES:
        d = mod._desc(c)
        yield c.name, [getattr(d, f) for f, _ in _lib.ConvDesc._fields_]


def layer_descs():
    """csrc/lgvae_plan.hip: build_layers (the x network; the three resizes are fused into d3 / d4 / d5 from H = 16 up)"""
    relu, none = 1, 0
    for B, H in LAYER_SHAPES:
        F, L = (H // 8) * (H // 8) * 128, LATENT
        for dtype in ("f32", "bf16"):
            dt = _lib.SV_F32 if dtype == "f32" else _lib.SV_BF16
            ups = 1 if H >= 16 else 0
            for name, h, cin, cout, k, s, act, ldx, ldy, yf32, u in (
                    ("e1", H, 3, 32, 6, 2, relu, 8, 32, 0, 0), ("e2", H // 2, 32, 64, 6, 2, relu, 32, 64, 0, 0),
                    ("e3", H // 4, 64, 128, 4, 2, relu, 64, 128, 0, 0), ("head", 1, F, 2 * L, 1, 1, none, F, 2 * L, 1, 0),
                    ("d1", 1, 2 * L, F, 1, 1, relu, 2 * L, F, 0, 0), ("d2", H // 8, 128, 128, 4, 1, relu, 128, 128, 0, 0),
                    ("d3", H // 4, 128, 64, 4, 1, relu, 128, 64, 0, ups), ("d4", H // 2, 64, 32, 6, 1, relu, 64, 32, 0, ups),
                    ("d5", H, 32, 6, 6, 1, none, 32, 6, 1, ups)):
                yield "%s_b%d_h%d_%s" % (name, B, H, dtype), [B, h, h, cin, cout, k, k, s, act, dt, ldx, ldy, yf32, u]


GRID_BLOCK = 384     # descriptors per block: the grid's inner loops (kernel size, stride, dtype, ldx, y_f32, ups_in) of one (B, H x W, Cin, Cout)
LETTERS = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"


def decode_grid(g):
    """the file's grid record -> per descriptor of the grid, in order: its six answers"""
    codes = "".join(g["blocks"][i] for i in g["index"])
    return [[-1] * 6 if c == "." else g["sizes"][LETTERS.index(c)] for c in codes]


def record(lib):
    answers = [queries(lib, d) for d in grid_descs()]
    sizes = sorted({tuple(q) for q in answers if q[0] != -1})
    assert len(sizes) <= len(LETTERS) and all(q == [-1] * 6 for q in answers if q[0] == -1) and len(answers) % GRID_BLOCK == 0
    codes = "".join("." if q[0] == -1 else LETTERS[sizes.index(tuple(q))] for q in answers)
    blocks, index = [], []
    for i in range(0, len(codes), GRID_BLOCK):
        b = codes[i:i + GRID_BLOCK]
        if b not in blocks:
            blocks.append(b)
        index.append(blocks.index(b))
    named = lambda it: [{"name": n, "desc": d, "sizes": queries(lib, d)} for n, d in it]
    return {"grid": {"sizes": [list(v) for v in sizes], "blocks": blocks, "index": index}, "cases": named(case_descs()), "layers": named(layer_descs())}


if __name__ == "__main__":
    commit = sys.argv[1] if len(sys.argv) > 1 else subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
    doc = record(_lib.load())
    lines = lambda v: ",\n".join("   " + json.dumps(e) for e in v)
    with open(OUT, "w") as f:
        f.write("{\n")
        f.write(' "recorded_from_commit": %s,\n' % json.dumps(commit))
        for key in ("cases", "layers"):
            f.write(' "%s": [\n%s\n ],\n' % (key, lines(doc[key])))
        g = doc["grid"]
        f.write(' "grid": {\n  "sizes": [\n%s\n  ],\n  "blocks": [\n%s\n  ],\n  "index": %s\n }\n}\n' % (lines(g["sizes"]), lines(g["blocks"]), json.dumps(g["index"])))
    print(OUT, sum(c != "." for b in g["index"] for c in g["blocks"][b]), len(doc["cases"]), len(doc["layers"]))
