"""Writes tests/golden/powf_domain.json: one SHA-256 per sub-domain of tests/util_device_math.powf_subdomains() over the outputs of THIS machine's
libm powf (it must be glibc 2.35 on a CPU with FMA: the variant oracle/rt_oracle.cpp restates), NaNs canonicalised to 0x7fc00000, little-endian
uint32.  tests/test_oracle_powf.py recomputes the same digests from the oracle's powf.

    python tools/make_golden_powf.py
"""
import ctypes
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "powf_domain.json")


def libc_version():
    libc = ctypes.CDLL(None)
    libc.gnu_get_libc_version.restype = ctypes.c_char_p
    return libc.gnu_get_libc_version().decode()


def digest(values):
    from tests import util_device_math as DM
    return hashlib.sha256(DM.canonical(values).astype("<u4").tobytes()).hexdigest()


def main():
    from oracle import oracle as O
    from tests import util_device_math as DM
    ver = libc_version()
    if ver != "2.35" and "--any-libc" not in sys.argv:
        sys.exit("this machine's glibc is %s, not 2.35: its powf is not the one the oracle restates" % ver)
    cpu = open("/proc/cpuinfo").read()
    if " fma " not in cpu.replace("\n", " "):
        sys.exit("this CPU has no FMA: glibc would run its other powf variant")
    doc = {"source": "libm powf, glibc %s, x86-64 FMA variant" % ver, "nan": "canonicalised to 0x7fc00000", "elements": 0, "sha256": {}}
    for name, x, y in DM.powf_subdomains():
        doc["sha256"][name] = digest(O.libm_powf_n(x, y))
        doc["elements"] += int(x.size)
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote %s: %d sub-domains, %d elements" % (OUT, len(doc["sha256"]), doc["elements"]))


if __name__ == "__main__":
    main()
