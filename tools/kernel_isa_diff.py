"""Which kernels' machine code differs between two builds: the device assembly build.sh keeps (build/*-hip-amdgcn-amd-amdhsa-gfx950.s),
normalised as tools/device_code_hash.sh does (comments and blank lines dropped, the compilation unit's id replaced by a constant), cut at the
labels of the functions and hashed per function.  A function's number within its unit, which its local labels carry (.LBB<number>_<block>) and
which moves when kernels are added in front of it, is replaced by a constant too.  A change meant for some kernels must leave every other one as it was.
  python tools/kernel_isa_diff.py <build directory of the parent> [build directory, default: build]"""
import hashlib
import os
import re
import sys

UNITS = ("rtx_api", "rtx_sort")


def functions(path):
    out, cur = {}, None
    names = set(re.findall(r"^\s*\.type\s+(\w+),@function", open(path).read(), re.M))
    for ln in open(path):
        ln = re.sub(r"[ \t]*;.*$", "", ln.rstrip("\n"))
        ln = re.sub(r"__hip_cuid_[0-9a-f]*", "__hip_cuid_X", ln)
        ln = re.sub(r"\.LBB\d+_", ".LBBn_", ln)
        if not ln.strip():
            continue
        m = re.match(r"^(_Z\w+):$", ln)
        if m and m.group(1) in names:
            cur = m.group(1)
            out[cur] = []
            continue
        if ln.startswith(".Lfunc_end"):
            cur = None
            continue
        if cur:
            out[cur].append(ln)
    return {k: hashlib.sha256("\n".join(v).encode()).hexdigest() for k, v in out.items()}


def main():
    old = sys.argv[1]
    new = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "build")
    for unit in UNITS:
        a, b = (functions(os.path.join(d, unit + "-hip-amdgcn-amd-amdhsa-gfx950.s")) for d in (old, new))
        differ = sorted(k for k in a if k in b and a[k] != b[k])
        print("%s: %d kernels, %d identical, %d differ, %d only in the first, %d only in the second" % (
            unit, len(set(a) | set(b)), sum(1 for k in a if k in b and a[k] == b[k]), len(differ), len(set(a) - set(b)), len(set(b) - set(a))))
        for k in differ:
            print("  differs  ", k)
        for k in sorted(set(a) ^ set(b)):
            print("  only in the %s" % ("first " if k in a else "second"), k)


if __name__ == "__main__":
    main()
