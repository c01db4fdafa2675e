"""Are the kernels of two trees the same kernels?  Compiles every csrc/*.hip of each tree to gfx950 assembly with the build's own flags
(split_vae_amd/build.py FLAGS + -S --cuda-device-only, what scripts/mfma_hazard_scan.py reads) and compares, per kernel symbol, the instruction
text from its label to its function end and its .amdhsa_kernel resource block (VGPR / AGPR / SGPR / LDS / scratch).  Comments and the function
index inside local labels (.LBB<fn>_<bb>) are not compared: both renumber when another kernel of the file goes away.
Usage: python scripts/kernel_asm_diff.py OLD_TREE NEW_TREE [WORK_DIR]     (a tree = a checkout, e.g. `git worktree add /tmp/old HEAD^`)
Prints kernels compared / identical / differing / removed / added with the names; exit status 1 when a kernel differs.
A differing kernel is classed further: RENAMED = same resource block and the same opcode sequence (only registers, immediates' homes or
label targets differ); RESCHEDULED = same resource block and the same opcodes the same number of times, in another order; DIFFERS = anything
else ("(resources)" when the resource block changed)."""
import glob, os, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor

FLAGS = ["--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-ffp-contract=off", "-w", "-S", "--cuda-device-only"]


def assemble(tree, out):
    os.makedirs(out, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    srcs = sorted(glob.glob(os.path.join(tree, "split_vae_amd", "csrc", "*.hip")))
    with ThreadPoolExecutor(max_workers=6) as ex:
        list(ex.map(lambda s: subprocess.run([hipcc] + FLAGS + [s, "-o", os.path.join(out, os.path.basename(s) + ".s")], check=True), srcs))


def kernels(out):
    """symbol -> (file, instruction text, resource block)"""
    found = {}
    for f in sorted(glob.glob(os.path.join(out, "*.s"))):
        lines = open(f).read().split("\n")
        res = {}
        for i, l in enumerate(lines):
            if l.strip().startswith(".amdhsa_kernel "):
                j = i
                while not lines[j].strip().startswith(".end_amdhsa_kernel"): j += 1
                res[l.split()[1]] = "\n".join(x.strip() for x in lines[i + 1:j])
        i = 0
        while i < len(lines):
            m = re.match(r"^([A-Za-z_][\w$.]*):", lines[i])
            if m and m.group(1) in res:
                j = i + 1
                while not lines[j].startswith(".Lfunc_end"): j += 1
                text = "\n".join(re.sub(r"\s*;.*$", "", re.sub(r"BB\d+_", "BB_", x)).rstrip() for x in lines[i + 1:j])
                found[m.group(1)] = (os.path.basename(f), text, res[m.group(1)])
                i = j
            i += 1
    return found


def opcodes(text):
    """the opcode of every instruction line of a kernel's text, in order (labels and directives dropped)"""
    return [l.split()[0] for l in text.split("\n") if l.startswith("\t") and l.split() and not l.split()[0].startswith(".")]


def classify(old, new):
    if old[2] != new[2]:
        return "DIFFERS"
    a, b = opcodes(old[1]), opcodes(new[1])
    return "RENAMED" if a == b else "RESCHEDULED" if sorted(a) == sorted(b) else "DIFFERS"


if __name__ == "__main__":
    work = sys.argv[3] if len(sys.argv) > 3 else tempfile.mkdtemp(prefix="kernel_asm_diff_")
    both = []
    for k, tree in enumerate(sys.argv[1:3]):
        assemble(tree, os.path.join(work, "old" if k == 0 else "new"))
        both.append(kernels(os.path.join(work, "old" if k == 0 else "new")))
    old, new = both
    same = [n for n in new if n in old and old[n][1:] == new[n][1:]]
    differ = [n for n in new if n in old and old[n][1:] != new[n][1:]]
    removed, added = [n for n in old if n not in new], [n for n in new if n not in old]
    print("kernels: old %d, new %d; compared %d: identical %d, differing %d; removed %d, added %d" %
          (len(old), len(new), len(same) + len(differ), len(same), len(differ), len(removed), len(added)))
    kind = {n: classify(old[n], new[n]) for n in differ}
    print("differing: renamed %d, rescheduled %d, other %d" % tuple(sum(k == t for k in kind.values()) for t in ("RENAMED", "RESCHEDULED", "DIFFERS")))
    for n in differ:
        print(kind[n], new[n][0], n, "%d -> %d instructions" % (len(opcodes(old[n][1])), len(opcodes(new[n][1]))),
              "(resources)" if old[n][2] != new[n][2] else "")
    for tag, names, src in (("REMOVED", removed, old), ("ADDED", added, new)):
        for n in names:
            print(tag, src[n][0], n)
    sys.exit(1 if differ else 0)
