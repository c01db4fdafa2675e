"""The library's environment switches are a closed, documented list (csrc/knobs.h; LAB_NOTES.md section 7).

csrc/knobs.h is the only file of the library that reads the environment.  It holds the runtime switches of the shipped library; every other
knob is an SV_TUNE_* macro that the default build compiles to its default (the name is not in the binary) and a -DSV_DEBUG_KNOBS build reads
from the environment.  These tests hold the sources, the documentation and the built library to that.  None needs a GPU."""
import glob
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "split_vae_amd", "csrc")
NAME = r"SV_[A-Z0-9_]+"


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _csrc_files():
    return sorted(f for f in glob.glob(os.path.join(CSRC, "*")) if f.endswith((".hip", ".h")))


def _shipped():
    """Names the default build reads: the getenv literals of knobs.h (the SV_TUNE_* macros pass their argument on, no literal)."""
    return set(re.findall(r'getenv\("(%s)"\)' % NAME, _read(os.path.join(CSRC, "knobs.h"))))


def _debug_tier():
    """Names behind the SV_TUNE_* macros, collected from every source of the library."""
    names = set()
    for f in _csrc_files():
        names |= set(re.findall(r'SV_TUNE_(?:FLAG|INT|STR)\(\s*"(%s)"' % NAME, _read(f)))
    return names


def _lab_notes_section(title):
    """Backticked SV_* names in the first column of the table under the LAB_NOTES.md heading that starts with `title`."""
    text = _read(os.path.join(ROOT, "LAB_NOTES.md"))
    m = re.search(r"^### %s[^\n]*\n(.*?)(?=^#{2,3} )" % re.escape(title), text, re.S | re.M)
    assert m, "LAB_NOTES.md has no section '### %s'" % title
    names = set()
    for line in m.group(1).splitlines():
        if line.startswith("|") and not line.startswith("|---"):
            names |= set(re.findall(r"`(%s)[`=]" % NAME, line.split("|")[1]))
    return names


def test_getenv_lives_in_one_file():
    users = [os.path.basename(f) for f in _csrc_files() if re.search(r"\bgetenv\b", _read(f))]
    assert users == ["knobs.h"], users


def test_shipped_switches_match_the_documented_list():
    shipped, debug = _shipped(), _debug_tier()
    assert len(shipped) == 23, sorted(shipped)
    assert not shipped & debug, sorted(shipped & debug)
    assert shipped == _lab_notes_section("7.1"), sorted(shipped ^ _lab_notes_section("7.1"))
    assert debug == _lab_notes_section("7.2"), sorted(debug ^ _lab_notes_section("7.2"))
    removed = _lab_notes_section("7.3")
    assert removed and not removed & (shipped | debug), sorted(removed & (shipped | debug))
    # the removed names are gone from the sources altogether, comments included
    for f in _csrc_files() + [os.path.join(ROOT, "include", "splitvae.h")]:
        left = removed & set(re.findall(NAME, _read(f)))
        assert not left, (os.path.basename(f), sorted(left))


def _python_files():
    files = [os.path.join(ROOT, "bench.py"), os.path.join(ROOT, "__graft_entry__.py")]
    for d in ("tests", "split_vae_amd", "scripts"):
        files += glob.glob(os.path.join(ROOT, d, "*.py"))
    return sorted(files)


def test_every_switch_python_sets_is_shipped_or_python_layer():
    """What tests/, bench.py and split_vae_amd/*.py put into an environment (monkeypatch.setenv, os.environ[...] = , env dicts, NAME=value in
    a command) reaches either the shipped library or Python code that reads it: never a knob the default build has compiled away."""
    shipped = _shipped()
    python_layer = set()
    for f in _python_files():
        python_layer |= set(re.findall(r'(?:environ\.get|getenv|environ\.pop)\(\s*["\'](%s)["\']' % NAME, _read(f)))
        python_layer |= set(re.findall(r'["\'](%s)["\']\s+(?:not\s+)?in\s+os\.environ' % NAME, _read(f)))
        python_layer |= set(re.findall(r'environ\[["\'](%s)["\']\](?!\s*=[^=])' % NAME, _read(f)))
    set_sites = [r'setenv\(\s*["\'](%s)["\']', r'delenv\(\s*["\'](%s)["\']', r'\[["\'](%s)["\']\]\s*=[^=]', r'["\'](%s)["\']\s*:',
                 r'\b(%s)=', r'setdefault\(\s*["\'](%s)["\']']
    this = os.path.abspath(__file__)
    for f in _python_files():
        if os.path.dirname(f).endswith("scripts") or os.path.abspath(f) == this:
            continue
        text = _read(f)
        for pat in set_sites:
            for name in re.findall(pat % NAME, text):
                assert name in shipped or name in python_layer, "%s sets %s: neither a shipped switch nor read by Python" % (os.path.relpath(f, ROOT), name)
    assert not python_layer & _debug_tier() - {"SV_NO_FUSED_UPSAMPLE"}, sorted(python_layer & _debug_tier())
    # (scripts/bench_layers.py reads SV_NO_FUSED_UPSAMPLE itself to pick the layer form it benchmarks: a Python-layer reading of the same name)


def _has(blob, name):
    return re.search(re.escape(name.encode()) + rb"(?![A-Z0-9_])", blob) is not None


def test_default_library_holds_the_shipped_names_only(lib_built):
    with open(lib_built, "rb") as f:
        blob = f.read()
    missing = sorted(n for n in _shipped() if not _has(blob, n))
    assert not missing, missing
    leaked = sorted(n for n in _debug_tier() | _lab_notes_section("7.3") if _has(blob, n))
    assert not leaked, leaked


def test_debug_knobs_build_compiles():
    """SV_EXTRA_FLAGS=-DSV_DEBUG_KNOBS builds a second library beside the shipped one, and that one does read the tuning knobs."""
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        import pytest
        pytest.skip("no hipcc")
    env = dict(os.environ, SV_EXTRA_FLAGS="-DSV_DEBUG_KNOBS -O2", SV_OBJ_TAG="_dbgknobs", SV_LIB_NAME="libsplitvae_hip_dbgknobs.so")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "split_vae_amd", "build.py")], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lib = os.path.join(ROOT, "split_vae_amd", "libsplitvae_hip_dbgknobs.so")
    with open(lib, "rb") as f:
        blob = f.read()
    missing = sorted(n for n in _shipped() | _debug_tier() if not _has(blob, n))
    assert not missing, missing
