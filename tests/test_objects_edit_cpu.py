"""Scene.add_object / remove_object without a GPU: editing the object list of a loaded scene gives, bit for bit, the object records, the
serialised description and the acceleration structures of a fresh load of the scene file with an [object] block written or deleted (the
reference's only way to add or remove an object).  The keys go through the code the .scene parser applies them with (objects.h,
applyObjectKeys)."""
import os
import re

import numpy as np
import pytest

from tests.util_lights import serialized
from tests.util_move import same_structure
from tests.util_objects import BUMPY, LONG_PLANE, TORUS_GLASS, TORUS_MAPS, apply_step, mesh_objects, write_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every scene comes back to its first objects at the end
STEPS = {
    "cfg1_simple_shapes": [
        ("add", "sphere", None, dict(pos=(0.8, -0.5, -3), radius=0.7, color=(0.9, 0.6, 0.2))),
        ("add", "plane", None, LONG_PLANE),
        ("add", "mesh", None, BUMPY),
        ("add", "mesh", 0, TORUS_MAPS),
        ("add", "sphere", 3, {}),                                           # (every key absent: the loader's defaults)
        ("remove", 3), ("remove", 8), ("remove", 0), ("remove", 6), ("remove", 5),
    ],
    "cfg2_smooth_4k": [
        ("add", "sphere", None, dict(pos=(1.2, -0.8, -2.5), radius=0.6, color=(1, 1, 1), material="reflective")),
        ("remove", 2),
        ("add", "mesh", None, TORUS_GLASS),
        ("remove", 1),
        ("add", "mesh", 0, BUMPY),
        ("remove", 0), ("remove", 1),
        ("add", "mesh", None, dict(pos=(0, 0, -3), size=(2, 2, 2), color=(1, 1, 1), name="scenes/assets/bumpy_4k.obj")),
    ],
    "mixed_materials": [
        ("remove", 1),
        ("add", "mesh", 1, dict(pos=(-1.2, 0, -4), size=(1.6, 1.6, 1.6), rot=(20, 30, 10), color=(1, 1, 1), material="transparent,1.3",
                                name="scenes/assets/bumpy_4k.obj")),
        ("remove", 3), ("remove", 3),
        ("add", "sphere", None, dict(pos=(0, 1.6, -5), color=(0.9, 0.2, 0.2), radius=0.6, material="phong,0.3,0.5,0.6,20.0")),
        ("add", "plane", None, dict(pos=(0, 0, -9), normal=(0, 0, 1), color=(0.5, 0.6, 0.5))),
    ],
}
# the steps after which a scene holds its first objects again (the last one always)
BACK = {"mixed_materials": (1,)}


def digest_bits(s):
    return s.digest().view(np.uint32)


def assert_same_host_state(ra, g, f, text, what):
    assert g.n_objects == f.n_objects, what
    assert np.array_equal(digest_bits(g), digest_bits(f)), "%s: the records differ from a fresh load's" % what
    assert serialized(ra, g) == serialized(ra, f), "%s: the serialised description differs from a fresh load's" % what
    for i in mesh_objects(text):
        k = same_structure(g.bvh(i), f.bvh(i))
        assert k is None, "%s: %s of object %d's acceleration structure differs from a fresh load's" % (what, k, i)
    assert [g.bvh(i) is None for i in range(g.n_objects)] == [i not in mesh_objects(text) for i in range(g.n_objects)], what


@pytest.mark.parametrize("name", sorted(STEPS))
def test_object_edits_equal_a_fresh_load_of_the_edited_file(ra, tmp_path, name):
    text = open(os.path.join(ROOT, "scenes", name + ".scene")).read()
    g = ra.Scene("scenes/%s.scene" % name, 64, 48)
    first_digest, first_desc = g.digest(), serialized(ra, g)
    first_bvh = {i: g.bvh(i) for i in mesh_objects(text)}
    for k, step in enumerate(STEPS[name]):
        text = apply_step(g, text, step)
        f = ra.Scene(write_scene(tmp_path, text, "%s_%d" % (name, k)), 64, 48)
        what = "%s step %d %r" % (name, k, step[:3])
        assert_same_host_state(ra, g, f, text, what)
        f.close()
        if k in BACK.get(name, ()) or k == len(STEPS[name]) - 1:
            assert np.array_equal(digest_bits(g), first_digest.view(np.uint32)), "%s: not the first objects again" % what
            assert serialized(ra, g) == first_desc, what
            for i, b in first_bvh.items():
                assert same_structure(g.bvh(i), b) is None, what
    g.close()


def test_refused_keys_and_indices_leave_the_scene_as_it_was(ra):
    g = ra.Scene("scenes/mixed_materials.scene", 64, 48)          # objects: mesh, mesh, mesh, sphere, plane
    before, desc = g.digest(), serialized(ra, g)
    for kind, at, keys in [("cone", None, {}), ("sphere", None, dict(normal=(0, 1, 0))), ("sphere", None, dict(size=(1, 1, 1))),
                           ("sphere", None, dict(name="scenes/assets/quad.obj")), ("plane", None, dict(radius=1.0)), ("plane", None, dict(rot=(0, 1, 0))),
                           ("mesh", None, dict(radius=1.0, name="scenes/assets/quad.obj")), ("mesh", None, dict(normal=(0, 1, 0))),
                           ("sphere", None, dict(pos=(1, 2))), ("sphere", None, dict(radius=(1, 2))), ("plane", None, dict(normal=(0, 1, 0, 0))),
                           ("sphere", None, dict(material="glass")), ("sphere", None, dict(material="transparent")),
                           ("sphere", None, dict(material="phong,0.3,0.5")), ("sphere", None, dict(material="reflective,1")),
                           ("sphere", None, dict(material="transparent,x")), ("sphere", None, dict(material=2)), ("mesh", None, dict(name=3)),
                           ("sphere", 6, {}), ("sphere", -1, {}), ("sphere", None, dict(position=(0, 1, 0)))]:
        with pytest.raises(ValueError):
            g.add_object(kind, at, **keys)
    for index in (5, -1, 99):
        with pytest.raises(ValueError):
            g.remove_object(index)
    # files that cannot be loaded, a mesh without a file
    for keys in (dict(name="scenes/assets/no_such.obj"), {}, dict(name="scenes/assets/quad.obj", diffuse_map="scenes/assets/no_such.bmp")):
        with pytest.raises(ra.RtxError):
            g.add_object("mesh", None, **keys)
    assert g.n_objects == 5
    assert np.array_equal(digest_bits(g), before.view(np.uint32)) and serialized(ra, g) == desc
    # the host entry points refuse them as well (NULL = absent)
    host = g.host
    v = np.ones(3, np.float32)
    p = v.ctypes.data
    none = [None] * 11
    args = lambda **kw: [kw.get(k) for k in ra._OBJECT_ARGS]
    assert host.rah_object_add(g.h, 1, -1, None, *args(normal=p)) < 0 and b"normal" in host.rah_last_error()
    assert host.rah_object_add(g.h, 2, -1, None, *args(radius=p)) < 0 and b"radius" in host.rah_last_error()
    assert host.rah_object_add(g.h, 1, -1, None, *args(name=b"scenes/assets/quad.obj")) < 0 and b"name" in host.rah_last_error()
    assert host.rah_object_add(g.h, 3, -1, None, *args(radius=p)) < 0 and b"radius" in host.rah_last_error()
    assert host.rah_object_add(g.h, 0, -1, None, *none) < 0 and host.rah_object_add(g.h, 4, -1, None, *none) < 0
    assert host.rah_object_add(g.h, 1, 6, None, *none) < 0
    assert host.rah_object_add(g.h, 3, -1, None, *none) < 0
    assert host.rah_object_remove(g.h, 5) != 0 and host.rah_object_remove(g.h, -1) != 0
    g._dims()
    assert g.n_objects == 5
    assert np.array_equal(digest_bits(g), before.view(np.uint32)) and serialized(ra, g) == desc
    g.close()


def test_every_object_removed_and_one_added(ra, tmp_path):
    name = "cfg1_simple_shapes"
    g = ra.Scene("scenes/%s.scene" % name, 64, 48)
    text = open(os.path.join(ROOT, "scenes", name + ".scene")).read()
    for k in range(5):
        text = apply_step(g, text, ("remove", (k * 2) % (5 - k)))
    assert g.n_objects == 0 and len(g.digest()) == 12 * g.n_lights
    f = ra.Scene(write_scene(tmp_path, text, "empty"), 64, 48)
    assert_same_host_state(ra, g, f, text, "no object left")
    f.close()
    text = apply_step(g, text, ("add", "mesh", None, BUMPY))
    f = ra.Scene(write_scene(tmp_path, text, "one"), 64, 48)
    assert_same_host_state(ra, g, f, text, "a mesh as the only object")
    f.close(); g.close()


def test_object_edit_symbols_are_declared_where_they_belong(ra):
    edit = open(os.path.join(ROOT, "include", "rtx_scene_edit.h")).read()
    debug = open(os.path.join(ROOT, "include", "rtx_debug.h")).read()
    boundary = open(os.path.join(ROOT, "include", "rtx.h")).read()
    decl = lambda hdr: set(re.findall(r"\b(rtx_[a-z0-9_]+)\s*\(", hdr))
    assert decl(edit) == set(ra.RTX_EDIT_SYMBOLS) and "rtx_scene_set_objects" in ra.RTX_EDIT_SYMBOLS
    assert "rtx_scene_objects_read" in decl(debug) and "rtx_scene_objects_read" in ra.RTX_SYMBOLS
    for s in ("rtx_scene_set_objects", "rtx_scene_objects_read"):
        assert s not in decl(boundary)
    assert len(decl(boundary)) <= 32
    for t in ("rtx_mesh_build", "rtx_mesh_source"):
        assert re.search(r"typedef struct %s\b" % t, edit), t
    rtx, host = ra.load()
    for s in ("rtx_scene_set_objects", "rtx_scene_objects_read"):
        assert hasattr(rtx, s), s
    for s in ("rah_object_add", "rah_object_remove"):
        assert hasattr(host, s), s
    _, missing = ra.exported_symbols()
    assert not missing
    for m in ("add_object", "remove_object", "device_objects"):
        assert callable(getattr(ra.Scene, m)), m
