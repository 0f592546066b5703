"""The host flatten's records (rendering_amd/csrc/rtx_flat_records.h through flattenMesh, rtx_flatten.hip) against digests of what the flatten
produced before its formulas were written once for host and device: a SHA-256 per output array of mesh_flatten_probe -- wide nodes, box records,
plane records, root record -- for every raw form of tests/util_adversarial.py at each of its penalties, the meshes of three bundled scenes and three
hand-made trees that reach the branches the builder cannot (an irregular box, a box outside its parent's, coordinates of 2^40 and beyond with an
infinite one, an empty leaf and a zero-edge triangle among them).

tests/golden/flatten_digest.json was written by `python tests/test_flatten_records_cpu.py <file>` run against the library of the commit BEFORE the
formulas moved into the header (that commit's tree first on sys.path), never by the code this test checks; it is regenerated only when a change
means to alter the records."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "flatten_digest.json")
SCENES = ("cfg2_smooth_4k", "cfg2_smooth_25k", "cfg4_textured_256")
ARRAYS = ("wide", "box", "plane", "root")


def hand_trees():
    """{name: bvh}: seven nodes -- the root, two inner nodes, four leaves --, one reference per triangle in leaf order."""
    def tree(bounds, leaf_tris):
        counts = [len(t) for t in leaf_tris]
        begin = np.concatenate([[0], np.cumsum(counts)])
        tris = np.zeros((begin[-1], 30), np.float32)
        tris[:, 0:9] = np.concatenate([np.asarray(t, np.float32).reshape(-1, 9) for t in leaf_tris])
        return dict(bounds=np.asarray(bounds, np.float32), skip=np.array([7, 4, 0, 0, 7, 0, 0], np.int32),
                    leaf_begin=np.array([0, 0, begin[0], begin[1], 0, begin[2], begin[3]], np.int32),
                    leaf_count=np.array([-1, -1, counts[0], counts[1], -1, counts[2], counts[3]], np.int32),
                    refs=np.arange(begin[-1], dtype=np.uint32), tris=tris)

    unit = [[0, 0, 0, 1, 1, 1]] * 7
    small = [[[0.1 + 0.2 * k, 0.1, 0.1, 0.3 + 0.2 * k, 0.1, 0.2, 0.1 + 0.2 * k, 0.4, 0.3]] for k in range(4)]
    irregular = [list(b) for b in unit]
    irregular[3][3] = 1e30                                      # (|b| < 1e30 fails: no wide tree at all)
    loose = [list(b) for b in unit]
    loose[5][0] = -0.5                                          # (node 5 is not inside node 4)
    big, inf = 2.0 ** 40, np.inf
    huge = [[[big, 0, 0, 2 * big, 1, 0, big, 0, 3], [-2 * big, 5, 5, -big, 6, 5, -big, 5, 7]],      # coordinates of 2^40 and 2^41
            [[1, 2, 3, inf, 2, 3, 1, 4, 3]],                                                        # a corner at infinity: never pruned
            [],                                                                                     # an empty leaf
            [[0.5, 0.5, 0.5, 0.75, 0.5, 0.5, 0.5, 0.75, 0.5], [0.25, 0.25, 0.25, 0.25, 0.25, 0.25, 0.5, 0.25, 0.25]]]      # the second: e1 = 0
    return {"irregular": tree(irregular, small), "not_nested": tree(loose, small), "huge": tree([[-4 * big] * 3 + [4 * big] * 3] * 7, huge)}


def cases(ra):
    """(case name, bvh) of everything the golden file covers"""
    from tests import util_adversarial as A
    for name in A.RAW_NAMES:
        t, lo, hi, pens = A.raw_form(name)
        for pen in pens:
            b = ra.bvh_build_host(t, lo, hi, pen)
            b["tris"] = t
            yield "raw/%s/penalty%d" % (name, pen), b
    for name in SCENES:
        s = ra.Scene("scenes/%s.scene" % name, 64, 64)
        for i in range(s.n_objects):
            b = s.bvh(i)
            if b is not None:
                yield "scene/%s/object%d" % (name, i), b
        s.close()
    for name, b in hand_trees().items():
        yield "hand/" + name, b


def digests(ra):
    out = {}
    for case, b in cases(ra):
        flat = ra.mesh_flatten_probe(b)
        out[case] = {k: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest() for k, a in zip(ARRAYS, flat)}
        out[case]["n_wide"] = len(flat[0])
    return out


@pytest.fixture(scope="module")
def computed(ra):
    return digests(ra)


def test_the_golden_file_covers_the_branches(computed):
    golden = json.load(open(GOLDEN))
    assert sorted(golden) == sorted(computed)
    assert golden["hand/irregular"]["n_wide"] == 0 and golden["hand/not_nested"]["n_wide"] == 0 and golden["hand/huge"]["n_wide"] == 1
    assert sum(1 for c in golden if c.startswith("scene/")) >= len(SCENES)


def test_flatten_records_match_the_digests(computed):
    golden = json.load(open(GOLDEN))
    differ = [(case, k) for case in golden for k in golden[case] if computed[case][k] != golden[case][k]]
    assert not differ, "records differ from tests/golden/flatten_digest.json: %s" % differ[:12]


if __name__ == "__main__":
    # (the tree whose library is to be recorded comes first on sys.path; see the docstring)
    import rendering_amd as RA
    from rendering_amd import assets
    assets.ensure()
    RA.load()
    json.dump(digests(RA), open(sys.argv[1], "w"), indent=1, sort_keys=True)
    print("wrote", sys.argv[1], "from", RA.__file__)
