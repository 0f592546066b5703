"""Writes tests/golden/analytic_margins.json: one SHA-256 per (scene form, ray family, output) of tests/util_analytic.py over the records of
the REAL reference (oracle/_ref/libref_harness.so; the build container only) -- the hit records and colours of every ray family, pass 1 and
the SSAA frame (first row and column zeroed) -- float32 bits, little-endian, NaNs canonicalised to 0x7fc00000.
tests/test_analytic_margins_cpu.py recomputes the same digests from the oracle.  One process per form: the reference keeps process-global
option flags.  Results only; no text of the reference.

    python tools/make_golden_analytic.py
"""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "analytic_margins.json")

CHILD = r"""
import json, sys
sys.path.insert(0, %r)
from oracle import oracle as O
from tools import ref_harness as R
from tests import util_analytic as UA
form, work = sys.argv[1], sys.argv[2]
fams = UA.families(form, O, work)
print(json.dumps({"digests": UA.digests(UA.results(R.RefScene, form, work, fams)), "rays": sum(len(f.rays) for f in fams.values())}))
"""


def main():
    from tools import ref_harness as R
    from tests import util_analytic as UA
    if not R.available():
        sys.exit("oracle/_ref is not built: the reference is not on this machine")
    doc = {"source": "the reference's Render::trace / castRay / pass 1 / SSAA through oracle/ref_harness.cpp", "nan": "canonicalised to 0x7fc00000",
           "frame": "%d x %d" % (UA.W, UA.H), "rays": {}, "sha256": {}}
    with tempfile.TemporaryDirectory() as work:
        for form in UA.FORMS:
            out = subprocess.run([sys.executable, "-c", CHILD % ROOT, form, work], cwd=ROOT, capture_output=True, text=True)
            if out.returncode != 0:
                sys.exit("%s: the reference refused the form or failed:\n%s" % (form, out.stderr[-2000:]))
            got = json.loads(out.stdout.strip().split("\n")[-1])
            doc["sha256"][form] = got["digests"]
            doc["rays"][form] = got["rays"]
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d forms, %d digests, %d rays" % (OUT, len(doc["sha256"]), sum(len(v) for v in doc["sha256"].values()), sum(doc["rays"].values())))


if __name__ == "__main__":
    main()
