"""Generates tests/golden/plan_layout.json: the workspace layout of sv_lgvae_plan and sv_gm_encoder, buffer by buffer.

For each descriptor below: the workspace bytes and (offset, bytes) of every buffer name the library creates in any mode,
"absent" where the mode lacks the buffer (sv_*_buffer answers SV_E_BADARG).  Host-only: sv_lgvae_plan_create and
sv_gm_encoder_create need no device.  tests/test_abi.py::test_workspace_layout_is_pinned compares the built library with
the file, so a buffer that moves, shrinks, appears or disappears fails there.

The file records the commit it was taken from (the commit BEFORE the typed buffer tables replaced the string-keyed
maps); regenerate it only when a layout change is intended.

Run from the repo root:  python tests/golden/make_golden_plan_layout.py
"""
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from split_vae_amd import _lib  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "plan_layout.json")

# (B, H, Lg = Ll, dtype, external_global_encoder, global_only)
LGVAE_DESCS = [(2, 32, 128, "f32", 0, 0), (2, 32, 128, "bf16", 0, 0), (64, 64, 128, "f32", 0, 0), (512, 64, 128, "bf16", 0, 0),
               (70, 32, 64, "bf16", 0, 0), (64, 32, 128, "f32", 1, 0), (64, 32, 128, "bf16", 1, 1)]
# (B, H, latent, y_size, tau, dtype)
GM_DESCS = [(64, 32, 128, 30, 0.4, "f32"), (64, 32, 128, 30, 0.4, "bf16")]

# every name build_buffers (csrc/lgvae_plan.hip) can create
_TWIN = ["polyfix_", "polycfix_", "polyd_", "polycw2_", "polycw3_", "polycw4_", "polyw_", "lat_ws_", "in8_", "a1_", "a2_", "a3_", "pre_", "gz_",
         "z_mean_", "z_sig_", "z_", "eps_", "kl_", "ghead_", "ga3_", "ga2_", "ga1_", "h1_", "h2_", "u2_", "h3_", "u3_", "h4_", "u4_", "out6_",
         "nll_", "nllpart_", "g5_", "gu4_", "g4_", "gu3_", "g3_", "gu2_", "g2_", "g1_"]
LGVAE_NAMES = ["jobs", "warena", "wgrad_ws", "dyn", "losses", "metric_acc", "zcat"] + [k + s for k in _TWIN for s in ("x", "xh")]
# every name sv_gm_encoder_create (csrc/gm_encoder.hip) adds
GM_NAMES = ["jobs", "warena", "h1", "h2", "h3", "a1", "yh1a", "yh1", "keep1", "a2", "yh2", "logits", "y", "y_lp", "u", "a_pm", "a_ps", "a_t",
            "h_top", "h5", "keep5", "a_e", "he", "hh", "a_m", "a_s", "zm", "zs", "z", "pm", "ps", "eps", "kl2", "ykl", "g_am", "g_as", "g_apm",
            "g_aps", "g_ae", "g_at", "g_logits", "g_a2", "g_a1", "g_c3", "g_h2", "g_c2", "g_h1d", "g_c1", "g_hh", "g_h5", "g_y", "g_yh2",
            "g_yh1", "g_h1", "acc_end", "wgrad_ws"]
DTYPES = {"f32": _lib.SV_F32, "bf16": _lib.SV_BF16}


def _buffers(lookup, handle, names):
    out = {}
    off, nb = C.c_int64(), C.c_int64()
    for n in names:
        rc = lookup(handle, n.encode(), C.byref(off), C.byref(nb))
        assert rc in (0, _lib.STATUS_BADARG), (n, rc)
        out[n] = [off.value, nb.value] if rc == 0 else "absent"
    return out


def lgvae_layout(lib, desc):
    B, H, L, dtype, ext, go = desc
    d = _lib.LGVaeDesc(B, H, H, L, L, DTYPES[dtype], 40.0, ext, go)
    h = C.c_void_p()
    assert lib.sv_lgvae_plan_create(C.byref(d), C.byref(h)) == 0, desc
    rec = {"desc": list(desc), "workspace_bytes": lib.sv_lgvae_workspace_bytes(h), "buffers": _buffers(lib.sv_lgvae_buffer, h, LGVAE_NAMES)}
    lib.sv_lgvae_plan_destroy(h)
    return rec


def gm_layout(lib, desc):
    B, H, L, K, tau, dtype = desc
    d = _lib.GmDesc(B, H, H, L, K, tau, DTYPES[dtype])
    h = C.c_void_p()
    assert lib.sv_gm_encoder_create(C.byref(d), C.byref(h)) == 0, desc
    rec = {"desc": list(desc), "workspace_bytes": lib.sv_gm_encoder_workspace_bytes(h), "buffers": _buffers(lib.sv_gm_encoder_buffer, h, GM_NAMES)}
    lib.sv_gm_encoder_destroy(h)
    return rec


def layouts(lib):
    return {"lgvae": [lgvae_layout(lib, d) for d in LGVAE_DESCS], "gm": [gm_layout(lib, d) for d in GM_DESCS]}


if __name__ == "__main__":
    commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
    doc = {"recorded_from_commit": commit}
    doc.update(layouts(_lib.load()))
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(OUT)
