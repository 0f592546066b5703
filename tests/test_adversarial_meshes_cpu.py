"""The adversarial meshes of tests/util_adversarial.py, without a GPU: every family has the property it was made for -- on the host builder
and the host flatten, the raw forms through bvh_build_host + mesh_flatten_probe, the scene forms through Scene(path).bvh() so that the
loader's placement is part of what is checked --, every scene the GPU tests load keeps to the builder's domain, the aimed rays of the GPU
tests meet something for at least a quarter of their number in the oracle, and on every scene form the oracle, against which everything on
the GPU side is judged, is bit-identical to the real reference (where oracle/_ref is built; one scene per child process, as in
tests/test_oracle_vs_reference.py).

Every coordinate is finite with |x| <= 2^10: the reference's split search (objects.cpp:676-689) ends only below a width of 0.1 in absolute
units, so it does not return for non-finite coordinates or for coordinates whose ulp reaches 0.1, and nothing here asks what happens
beyond.  For the same reason three branches of the flatten are out of reach of the builder and stay with rtx_mesh_flatten_probe on
hand-made trees (tests/test_host_cpu.py): the "irregular box" branch (|b| >= 1e30), the "not nested" branch and the vmax >= 2^40 branch."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import util_adversarial as A
from tests.test_gpu_margins import ray_families
from tests.util_move import edit_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref", "libref_harness.so")


def leaves(b):
    """[(node, the triangles its references name)] of every leaf"""
    return [(i, b["refs"][b["leaf_begin"][i]:b["leaf_begin"][i] + b["leaf_count"][i]]) for i in np.nonzero(b["leaf_count"] >= 0)[0]]


def assert_property(name, b, flat, tris9, raw):
    wide, box, plane, root = flat
    lk = A.links(wide)
    level, parent = A.wide_levels(wide)
    counts = b["leaf_count"]
    if name == "one":
        assert b["n_nodes"] == 1 and counts[0] == 1 and len(wide) == 1 and (lk[0] != 0).sum() == 1 and lk[0, 0] == ~1
    elif name in ("two", "seven", "nine"):
        assert 3 <= b["n_nodes"] <= 9, b["n_nodes"]
        assert 2 <= (lk[0] != 0).sum() <= 7 and (lk[0] < 0).any(), lk[0]
    elif name.startswith("stack_"):
        k = int(name[6:])
        assert (counts == k).sum() == 1, counts
        if raw:
            assert b["n_nodes"] == 1
    elif name == "slivers":
        assert b["n_refs"] >= 2.5 * len(tris9) and counts.max() > 128, (b["n_refs"], len(tris9), counts.max())
    elif name == "flat":
        assert (b["bounds"][:, 1] == b["bounds"][:, 4]).all(), "a node box with an extent in y"
    elif name == "degenerate":
        ze = A.zero_edge(tris9)
        kinds = [(ze[r].all(), ze[r].any()) for _, r in leaves(b) if len(r)]
        assert any(every for every, _ in kinds), "no leaf of zero-edge triangles only"
        assert any(some and not every for every, some in kinds), "no leaf that mixes zero-edge triangles with others"
    elif name == "tiny":
        used = lk != 0
        spoiled = used & np.isneginf(plane[:, :, 3])
        first = np.ascontiguousarray(wide[:, :, 7]).view(np.int32)
        n_soup = len(tris9) - 8
        holds = np.zeros_like(used)          # the leaf slots that reference one of the eight tiny triangles
        for w, k in zip(*np.nonzero(lk < 0)):
            holds[w, k] = (b["refs"][first[w, k]:first[w, k] + ~lk[w, k]] >= n_soup).any()
        assert holds.any() and np.array_equal(spoiled & (lk < 0), holds), "the leaf slots without a plane bound are not the ones with a tiny triangle"
        for w, k in zip(*np.nonzero(spoiled)):
            assert parent[w] is None or spoiled[parent[w]], "wide node %d slot %d has no plane bound, the slot above it has one" % (w, k)
        assert (spoiled & (level > 1)[:, None]).any() and (used & ~spoiled).any()
        assert np.isposinf(plane[:, :, 7][spoiled]).all()
    elif name == "deep_edge":
        assert len(wide) == A.DEEP_WIDE[name]
        assert 28 <= b["max_depth"] <= 30 and len(wide) > 0 and level.max() == 10, (b["max_depth"], len(wide), level.max() if len(wide) else 0)
    elif name == "deep_over":
        assert b["max_depth"] >= 31 and len(wide) == 0 == A.DEEP_WIDE[name], (b["max_depth"], len(wide))
    else:
        assert name.startswith("soup_")


def in_domain(t, lo, hi):
    return bool(np.isfinite(t).all() and np.isfinite(lo).all() and np.isfinite(hi).all() and max(np.abs(t).max(), np.abs(lo).max(), np.abs(hi).max()) <= A.COORD_MAX)


@pytest.mark.parametrize("name", A.RAW_NAMES)
def test_raw_forms_have_their_property(ra, name):
    t, lo, hi, pens = A.raw_form(name)
    assert t.dtype == np.float32 and t.shape[1] == 9 and len(t) <= 1110 and in_domain(t, lo, hi)
    for pen in pens:
        b = ra.bvh_build_host(t, lo, hi, pen)
        b["tris"] = t
        flat = ra.mesh_flatten_probe(b)
        assert_property(name, b, flat, t, raw=True)
        print(name, "raw, penalty", pen, A.sizes(b, flat))


def scene_states(name, tmp_path, cull=1, pen=1):
    """[(tag, path)]: the scene with the family's mesh added, then after each of its moves"""
    base, keys, text = A.scene_form(name, tmp_path, cull, pen)
    out = []
    for tag, mv in [("add", None)] + A.moves(name):
        if mv:
            text = edit_scene(text, 1, **mv)
        p = tmp_path / ("%s_%s.scene" % (name, tag))
        p.write_text(text)
        out.append((tag, str(p)))
    return out


@pytest.mark.parametrize("name", A.SCENE_NAMES)
def test_scene_forms_have_their_property(ra, tmp_path, name):
    """... after the loader's placement, and every state the GPU tests load stays in the builder's domain; a deep family keeps its depth
    when only its pos moves."""
    for pen in A.SCENE_FAMILIES[name][3]:
        for tag, path in scene_states(name, tmp_path, 1, pen):
            s = ra.Scene(path, A.W, A.H)
            b = s.bvh(1)
            s.close()
            t = b["tris"][:, 0:9]
            assert len(t) == len(A.scene_triangles(name)) <= 1110
            assert in_domain(t, b["bounds"][0, 0:3], b["bounds"][0, 3:6]), "%s %s leaves the builder's domain" % (name, tag)
            flat = ra.mesh_flatten_probe(b)
            if tag == "add" or (tag == "shift" and name in A.DEEP):
                assert_property(name, b, flat, t, raw=False)
            if tag == "add" and name not in ("one", "flat") and not name.startswith("stack_"):
                assert t.tobytes() == A.raw_form(name)[0].tobytes(), "the placement is not exact"
            print(name, tag, "penalty", pen, A.sizes(b, flat))


@pytest.mark.parametrize("name,cull,pen", A.CASES)
def test_aimed_rays_meet_something_for_a_quarter_of_their_number(ra, oracle, tmp_path, name, cull, pen):
    """A condition on the inputs of the GPU tests, not on any code under test: the oracle alone."""
    tag, path = scene_states(name, tmp_path, cull, pen)[0]
    o = oracle.OracleScene(path, A.W, A.H)
    rays = A.aimed_rays(ray_families, o.bvh(1)["tris"][:, 0:9], A.ray_seed(name))
    assert 64 <= len(rays) <= 10048 and len(rays) % 64 == 0
    h, _ = o.probe(rays)
    tree = o.bvh(1)
    o.close()
    hits, on_mesh = int((h[:, 0] > 0).sum()), int(((h[:, 0] > 0) & (h[:, 1] == 1)).sum())
    print(name, "cull", cull, "penalty", pen, "rays", len(rays), "hits", hits, "on the mesh", on_mesh)
    assert 4 * hits >= len(rays), "%d of %d rays hit" % (hits, len(rays))
    assert 10 * on_mesh >= len(rays), "%d of %d rays hit the mesh" % (on_mesh, len(rays))
    if name.startswith("stack_"):          # (the tie the GPU tests look at is there: the oracle keeps the first of equal t, in leaf order)
        on_stack, first = A.stack_hits(name, tree, h)
        assert on_stack.sum() > len(rays) // 50 and (h[on_stack, 2] == first).all()


CHILD = r"""
import sys, numpy as np
sys.path.insert(0, %r)
from tools import ref_harness as R
from oracle import oracle as O
from tests import util_adversarial as A
from tests.test_gpu_margins import ray_families
path, name = sys.argv[1], sys.argv[2]
r = R.RefScene(path, A.W, A.H); o = O.OracleScene(path, A.W, A.H)
b = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
fr = r.pass1(); fo = o.pass1()
assert np.array_equal(b(fr), b(fo)), 'pass1'
f2r = r.ssaa(fr); f2o = o.ssaa(fo)
d = (b(f2r) != b(f2o)).any(-1); d[0, :] = False; d[:, 0] = False
assert not d.any(), 'ssaa'
for i in range(r.n_objects):
    x, y = r.bvh(i), o.bvh(i)
    assert (x is None) == (y is None)
    if x is not None:
        for k in x:
            if isinstance(x[k], np.ndarray): assert x[k].tobytes() == y[k].tobytes(), k
            else: assert x[k] == y[k], k
rays = A.aimed_rays(ray_families, o.bvh(1)['tris'][:, 0:9], A.ray_seed(name))
hr, cr = r.probe(rays); ho, co = o.probe(rays)
assert np.array_equal(b(hr), b(ho)), 'probe: hit records'
assert np.array_equal(b(cr), b(co)), 'probe: colours'
print('OK')
"""


@pytest.mark.skipif(not os.path.exists(REF), reason="oracle/_ref not built")
@pytest.mark.parametrize("name,cull,pen", A.CASES)
def test_oracle_bit_identical_to_reference_on_scene_forms(tmp_path, name, cull, pen):
    """Pass 1, the frame after SSAA away from the reference's uninitialised first row and column, the tree, the aimed rays."""
    for tag, path in scene_states(name, tmp_path, cull, pen):
        out = subprocess.run([sys.executable, "-c", CHILD % ROOT, path, name], cwd=ROOT, capture_output=True, text=True)
        assert out.returncode == 0 and "OK" in out.stdout, "%s %s: %s" % (name, tag, out.stdout[-2000:] + out.stderr[-2000:])
