"""Scene.move_object without a GPU: moving an object of a loaded scene gives, bit for bit, the triangles, the acceleration structure and
the object records of a fresh load of the scene file with that object's [object] block edited (the reference's only way to move it).
Vertices are placed again by the loader's own code; the host structure is built again as the loader builds it."""
import os
import re

import numpy as np
import pytest

from tests.util_move import edit_scene, same_structure, write_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (object index, keys) per step; every scene comes back to its first placement at the end
MOVES = {
    "cfg2_smooth_4k": [
        (1, dict(pos=(0.3, -0.2, -3.5))),
        (1, dict(size=(1.2, 2.5, 1.7), rot=(10, -35, 5))),
        (0, dict(pos=(0, -1.7, 0.2), normal=(0.1, 0.9, 0.05))),
        (1, dict(pos=(0, 0, -3), size=(2, 2, 2), rot=(0, 0, 0))),
        (0, dict(pos=(0, -1.5, 0), normal=(0, 1, 0))),
    ],
    "cfg4_textured_256": [
        (0, dict(pos=(0.2, 0.1, -0.8))),
        (0, dict(rot=(30, 60, -20), size=(1.5, 2.5, 2))),
        (0, dict(pos=(-0.1, 0, -0.6), rot=(0, 100, 0), size=(2, 2, 2))),
    ],
    "mixed_materials": [
        (0, dict(pos=(0.5, -1.0, -4.2), size=(6, 2, 9))),          # the flat quad: its pinned axis follows pos
        (1, dict(rot=(-40, 10, 70), pos=(-1.0, 0.2, -4.4))),
        (2, dict(rot=(15, 80, -5), size=(1.2, 1.9, 1.4))),
        (3, dict(pos=(0.4, 1.2, -5.5), radius=0.85)),
        (4, dict(pos=(0, 0, -8), normal=(0.2, -0.1, 1.3))),
        (0, dict(pos=(0, -1.2, -4), size=(8, 1, 8))),
        (1, dict(pos=(-1.2, 0, -4), rot=(20, 30, 10))),
        (2, dict(rot=(0, 45, 0), size=(1.8, 1.8, 1.8))),
        (3, dict(pos=(0, 1.6, -5), radius=0.6)),
        (4, dict(pos=(0, 0, -9), normal=(0, 0, 1))),
    ],
}


def mesh_objects(g):
    return [i for i in range(g.n_objects) if g.bvh(i) is not None]


def assert_same(g, f, what):
    assert np.array_equal(g.digest().view(np.uint32), f.digest().view(np.uint32)), "%s: object records differ" % what
    for i in mesh_objects(f):
        k = same_structure(g.bvh(i), f.bvh(i))
        assert k is None, "%s: object %d, %s differs from a fresh load" % (what, i, k)


@pytest.mark.parametrize("name", sorted(MOVES))
def test_move_object_equals_a_fresh_load_of_the_edited_file(ra, tmp_path, name):
    text = open(os.path.join(ROOT, "scenes", name + ".scene")).read()
    g = ra.Scene("scenes/%s.scene" % name, 64, 48)
    first = {i: g.bvh(i) for i in mesh_objects(g)}
    first_digest = g.digest()
    for step, (idx, keys) in enumerate(MOVES[name]):
        g.move_object(idx, **keys)
        text = edit_scene(text, idx, **keys)
        f = ra.Scene(write_scene(tmp_path, text, "%s_%d" % (name, step)), 64, 48)
        assert_same(g, f, "%s step %d" % (name, step))
        f.close()
    # back where every object started: the first load's triangles and structures again
    assert np.array_equal(g.digest().view(np.uint32), first_digest.view(np.uint32))
    for i, b in first.items():
        assert same_structure(g.bvh(i), b) is None
    g.close()


def test_random_placements_of_meshes_equal_fresh_loads(ra, tmp_path):
    rng = np.random.default_rng(7)
    text = open(os.path.join(ROOT, "scenes", "mixed_materials.scene")).read()
    g = ra.Scene("scenes/mixed_materials.scene", 64, 48)
    for step in range(6):
        idx = int(rng.integers(0, 3))
        keys = dict(pos=rng.uniform(-2, 2, 3) + np.float32([0, 0, -5]), rot=rng.uniform(-180, 180, 3), size=rng.uniform(0.2, 3, 3))
        keys = {k: np.float32(v) for k, v in keys.items() if rng.random() < 0.8} or dict(pos=np.float32([0, 0, -5]))
        g.move_object(idx, **keys)
        text = edit_scene(text, idx, **keys)
        f = ra.Scene(write_scene(tmp_path, text, "rand_%d" % step), 64, 48)
        assert_same(g, f, "random step %d (object %d, %s)" % (step, idx, sorted(keys)))
        f.close()
    g.close()


def test_keys_that_do_not_fit_the_type_raise(ra):
    g = ra.Scene("scenes/mixed_materials.scene", 64, 48)
    before = g.digest()
    with pytest.raises(ValueError):
        g.move_object(0, radius=1.0)           # mesh
    with pytest.raises(ValueError):
        g.move_object(0, normal=(0, 1, 0))
    with pytest.raises(ValueError):
        g.move_object(3, rot=(0, 10, 0))       # sphere
    with pytest.raises(ValueError):
        g.move_object(3, size=(1, 1, 1))
    with pytest.raises(ValueError):
        g.move_object(4, radius=2.0)           # plane
    with pytest.raises(ValueError):
        g.move_object(4, rot=(1, 2, 3))
    with pytest.raises(ValueError):
        g.move_object(5, pos=(0, 0, 0))        # no such object
    with pytest.raises(ValueError):
        g.move_object(3, pos=(0, 0))           # three values
    assert np.array_equal(g.digest().view(np.uint32), before.view(np.uint32))
    # the host entry point refuses them as well (NULL = unchanged)
    r = np.ones(1, np.float32)
    assert g.host.rah_object_move(g.h, 0, None, None, None, r.ctypes.data, None) != 0
    assert b"radius" in g.host.rah_last_error()
    assert g.host.rah_object_move(g.h, 99, None, None, None, None, None) != 0
    assert np.array_equal(g.digest().view(np.uint32), before.view(np.uint32))
    g.close()


def test_edit_symbols_are_exported_and_declared(ra):
    hdr = open(os.path.join(ROOT, "include", "rtx_scene_edit.h")).read()
    declared = set(re.findall(r"\b(rtx_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(ra.RTX_EDIT_SYMBOLS)
    assert not set(ra.RTX_EDIT_SYMBOLS) & set(ra.RTX_SYMBOLS)
    rtx, _ = ra.load()
    for s in ra.RTX_EDIT_SYMBOLS:
        assert hasattr(rtx, s), s
    _, missing = ra.exported_symbols()
    assert not missing
