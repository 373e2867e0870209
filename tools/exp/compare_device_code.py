#!/usr/bin/env python3
"""Do the gfx950 kernels of csrc/*.hip differ between a git revision and the working tree?  Compiles every file device-only
to assembly in both states (the flags of tests/test_kernel_codegen.py), strips debug directives, comments and the function
ordinal in local labels, and compares per mangled name: the set of symbols, every body, and every kernel's resources
(VGPRs + AGPRs, SGPRs, LDS, scratch).  Exit status 1 when anything differs.
usage: python tools/exp/compare_device_code.py <git rev> [file under graph_kmer_index_amd/csrc ...]"""
import glob, os, re, subprocess, sys, tempfile

rev = sys.argv[1]
root = subprocess.run(["git", "rev-parse", "--show-toplevel"], capture_output=True, text=True, check=True).stdout.strip()
csrc = os.path.join(root, "graph_kmer_index_amd", "csrc")
names = sys.argv[2:] or sorted(os.path.basename(p) for p in glob.glob(os.path.join(csrc, "*.hip")))
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-function", "--cuda-device-only", "-S"]


def asm_of(tree, name):
    out = os.path.join(tree, name + ".s")
    subprocess.run(["/opt/rocm/bin/hipcc"] + FLAGS + [os.path.join(tree, "graph_kmer_index_amd", "csrc", name), "-o", out],
                   check=True, stderr=subprocess.DEVNULL)
    return open(out).read()


def funcs(txt):
    res = {}
    for m in re.finditer(r"\n(_Z\w+):[^\n]*\n(.*?)\n\.Lfunc_end\d+:", txt, re.S):
        lines = []
        for l in m.group(2).split("\n"):
            if re.match(r"\s*\.(loc|file|cfi)", l) or re.match(r"\s*;", l):
                continue
            l = l.split(";")[0].rstrip()
            l = re.sub(r"\.LBB\d+_", ".LBB_", l)       # block labels carry the function's index in the file
            l = re.sub(r"\.L(tmp|func_begin|func_end|JTI)\d+(_\d+)?", r".L\1", l)
            if l:
                lines.append(l)
        res[m.group(1)] = lines
    return res


def resources(txt):
    res = {}
    for blk in re.split(r"\n  - \.agpr_count:", txt)[1:]:
        blk = ".agpr_count:" + blk
        get = lambda key: re.search(r"\.%s:\s*(\S+)" % key, blk).group(1)
        res[get("name")] = tuple(int(get(k)) for k in ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size",
                                                        "private_segment_fixed_size"))
    return res


old_tree = tempfile.mkdtemp(prefix="gki_cmp_old_")
new_tree = tempfile.mkdtemp(prefix="gki_cmp_new_")
for tree, src in ((old_tree, ["git", "archive", rev, "graph_kmer_index_amd/csrc", "include"]),
                  (new_tree, ["tar", "-c", "--exclude=*.o", "--exclude=*_obj", "graph_kmer_index_amd/csrc", "include"])):
    tar = subprocess.run(src, cwd=root, capture_output=True, check=True).stdout
    subprocess.run(["tar", "-x", "-C", tree], input=tar, check=True)

n_diff = n_funcs = n_kernels = 0
for name in names:
    old, new = asm_of(old_tree, name), asm_of(new_tree, name)
    A, B, RA, RB = funcs(old), funcs(new), resources(old), resources(new)
    diffs = ["symbol only in %s: %s" % (rev if n in A else "the working tree", n) for n in sorted(set(A) ^ set(B))]
    diffs += ["kernel only in %s: %s" % (rev if n in RA else "the working tree", n) for n in sorted(set(RA) ^ set(RB))]
    diffs += ["body differs (%d -> %d lines): %s" % (len(A[n]), len(B[n]), n) for n in sorted(set(A) & set(B)) if A[n] != B[n]]
    diffs += ["resources differ (%s -> %s): %s" % (RA[n], RB[n], n) for n in sorted(set(RA) & set(RB)) if RA[n] != RB[n]]
    print("%-24s %3d functions, %3d kernels, %d differences" % (name, len(B), len(RB), len(diffs)))
    for d in diffs:
        print("    " + d)
    n_diff += len(diffs); n_funcs += len(B); n_kernels += len(RB)
print("%d files, %d functions, %d kernels compared with %s: %d differences" % (len(names), n_funcs, n_kernels, rev, n_diff))
sys.exit(1 if n_diff else 0)
