"""Are the kernels of two trees the same kernels?  Compiles every csrc/*.hip of each tree to gfx950 assembly with the build's own flags
(split_vae_amd/build.py FLAGS + -S --cuda-device-only, what scripts/mfma_hazard_scan.py reads) and compares, per kernel symbol, the instruction
text from its label to its function end and its .amdhsa_kernel resource block (VGPR / AGPR / SGPR / LDS / scratch).  Comments and the function
index inside local labels (.LBB<fn>_<bb>) are not compared: both renumber when another kernel of the file goes away.
Usage: python scripts/kernel_asm_diff.py OLD_TREE NEW_TREE [WORK_DIR]     (a tree = a checkout, e.g. `git worktree add /tmp/old HEAD^`)
Prints kernels compared / identical / differing / removed / added with the names; exit status 1 when a kernel differs."""
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
    for tag, names, src in (("DIFFERS", differ, new), ("REMOVED", removed, old), ("ADDED", added, new)):
        for n in names:
            print(tag, src[n][0], n, ("(resources)" if tag == "DIFFERS" and old[n][2] != new[n][2] else ""))
    sys.exit(1 if differ else 0)
