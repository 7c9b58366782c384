"""Compare the gfx950 device code of two source trees kernel by kernel (host only, no GPU).

    python scripts/kernel_isa_diff.py OLD_TREE NEW_TREE

Every .hip of each tree's ptt_amd/build.py is compiled with the flags that build gives it (PTT_HIP_FLAGS etc. are read from
the environment as usual) plus --cuda-device-only -S. A kernel's text runs from its `_Z...:` label to `.Lfunc_end`, comments
stripped, `.LBB<n>_` label numbers normalised; its descriptor is the `.amdhsa_` lines (register counts, LDS and scratch
size). Text is compared for equality, nothing else. Kernels that were renamed on purpose: --rename OLD_SYMBOL=NEW_SYMBOL.
Exit status 1 unless every kernel of OLD_TREE is SAME with an equal descriptor and NEW_TREE adds none.
"""
import collections
import importlib.util
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor


def kernels(tree):
    """{symbol: (source file, instruction text, descriptor text)} of every kernel of the tree."""
    spec = importlib.util.spec_from_file_location("_build_" + str(abs(hash(tree))), os.path.join(tree, "ptt_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)

    def compile_one(src):
        cmd = [b._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-S", "-o", "-",
               os.path.join(b.CSRC, src)] + b.EXTRA_FLAGS.get(src, []) + b.COMMON_FLAGS
        return src, subprocess.run(cmd, check=True, stdout=subprocess.PIPE, universal_newlines=True).stdout

    out = {}
    with ThreadPoolExecutor(max_workers=len(b.HIP_SOURCES)) as pool:
        for src, asm in pool.map(compile_one, [s for s in b.HIP_SOURCES if os.path.exists(os.path.join(b.CSRC, s))]):
            asm = re.sub(r"[ \t]*;.*", "", asm)
            asm = re.sub(r"\.LBB\d+_", ".LBB_", asm)
            for sym, desc in re.findall(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)^\s*\.end_amdhsa_kernel", asm, re.M | re.S):
                body = re.search(r"^%s:\n(.*?)^\.Lfunc_end" % re.escape(sym), asm, re.M | re.S).group(1)
                lines = [ln.strip() for ln in body.splitlines() if ln.strip()]
                key = sym if sym not in out else sym + "@" + src
                out[key] = (src, "\n".join(lines), "\n".join(ln.strip() for ln in desc.splitlines() if ".amdhsa_" in ln))
    return out


def main(argv):
    renames = dict(a.split("=", 1) for i, a in enumerate(argv) if i and argv[i - 1] == "--rename")
    trees = [a for i, a in enumerate(argv) if a != "--rename" and not (i and argv[i - 1] == "--rename")]
    if len(trees) != 2:
        sys.exit(__doc__)
    old, new = kernels(trees[0]), kernels(trees[1])
    per_file = collections.defaultdict(collections.Counter)
    bad = 0
    for sym in sorted(old):
        src, text, desc = old[sym]
        nsym = renames.get(sym, sym)
        if nsym not in new:
            verdict = "ONLY IN OLD"
        else:
            verdict = ("SAME" if new[nsym][1].replace(nsym, sym) == text else "DIFF") + \
                      (", descriptor equal" if new[nsym][2].replace(nsym, sym) == desc else ", descriptor DIFFERS")
        per_file[src][verdict] += 1
        bad += verdict != "SAME, descriptor equal"
        print("%-28s %-18s %s%s" % (verdict, src, sym, " -> " + new[nsym][0] if nsym in new and new[nsym][0] != src else ""))
    added = sorted(set(new) - {renames.get(s, s) for s in old})
    for sym in added:
        print("%-28s %-18s %s" % ("ONLY IN NEW", new[sym][0], sym))
    print("\nsummary (by the old tree's files):")
    for src in sorted(per_file):
        print("  %-18s %3d kernels: %s" % (src, sum(per_file[src].values()),
                                          "; ".join("%d %s" % (n, v) for v, n in sorted(per_file[src].items()))))
    print("  added in the new tree: %d" % len(added))
    return 1 if bad or added else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
