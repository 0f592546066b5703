"""Scene.set_light / add_light / remove_light without a GPU: editing the lights of a loaded scene gives, bit for bit, the light records and
area-light sample points of a fresh load of the scene file with its [light] blocks rewritten, appended or deleted (the reference's only way
to change a light).  The keys go through the code the .scene parser applies them with (lights.h, applyLightKeys)."""
import os
import re

import numpy as np
import pytest

from tests.util_lights import apply_step, serialized, write_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every scene comes back to its first lights at the end
STEPS = {
    "area_light": [
        ("set", 0, dict(pos=(0.4, 2.8, -2.6))),
        ("set", 0, dict(samples=1)),
        ("set", 0, dict(samples=5, i=(1.2, 0.1, 0), j=(0, 0.2, 1.1))),
        ("set", 1, dict(samples=2, color=(0.2, 0.9, 0.3), intensity=0.7)),
        ("set", 2, dict(position=(1.5, 2.5, -0.5), intensity=0.55)),
        ("remove", 1),
        ("add", "area", dict(pos=(-3, 1, -1), i=(0, 0.8, 0), j=(0, 0, 0.8), samples=1, color=(0.4, 0.5, 1), intensity=1.5)),
        ("add", "distant", dict(direction=(0.1, -1, 0.2))),                 # (colour and intensity: the loader's defaults)
        ("add", "area", {}),                                                # (every key absent: one sample at the origin)
        ("remove", 4), ("remove", 3),
        # back: the point light to the end again, the first area light as it was
        ("remove", 1),
        ("add", "point", dict(position=(2, 2, 0), color=(1, 0.6, 0.4), intensity=0.4)),
        ("set", 0, dict(pos=(0, 3, -3), i=(1.5, 0, 0), j=(0, 0, 1.5), samples=3)),
    ],
    "cfg1_simple_shapes": [
        ("set", 0, dict(position=(-0.5, 1.5, -2.5))),
        ("set", 1, dict(direction=(0.3, -1, -0.2), color=(1, 0.9, 0.7), intensity=0.35)),
        ("add", "point", dict(position=(2, 1, -3), color=(0.3, 0.4, 1), intensity=0.6)),
        ("remove", 0),
        ("remove", 0), ("remove", 0),                                       # no light left
        ("add", "point", dict(position=(-1, 1, -1.5), color=(1, 1, 0.8), intensity=0.5)),
        ("add", "distant", dict(direction=(0, -1, 0), color=(1, 1, 1), intensity=0.2)),
    ],
    "cfg2_smooth_4k": [
        ("set", 0, dict(position=(0.5, 2.2, -1.4))),
        ("set", 1, dict(color=(0.2, 0.8, 0.4), intensity=0.6)),
        ("remove", 2),
        ("add", "distant", dict(direction=(-0.3, -1, -0.4), color=(0, 0, 1), intensity=0.9)),
        ("add", "area", dict(pos=(0, 2.5, -2), i=(1, 0, 0), j=(0, 0, 1), samples=3, color=(1, 1, 1), intensity=0.5)),
        ("remove", 3), ("remove", 2),
        ("add", "point", dict(position=(-1, -1, -1), color=(0, 0, 1), intensity=0.9)),
        ("set", 1, dict(color=(0, 1, 0), intensity=0.9)),
        ("set", 0, dict(position=(0, 2, -1))),
    ],
}


def digest_bits(s):
    return s.digest().view(np.uint32)


@pytest.mark.parametrize("name", sorted(STEPS))
def test_light_edits_equal_a_fresh_load_of_the_edited_file(ra, tmp_path, name):
    text = open(os.path.join(ROOT, "scenes", name + ".scene")).read()
    g = ra.Scene("scenes/%s.scene" % name, 64, 48)
    first_digest, first_desc = g.digest(), serialized(ra, g)
    for k, step in enumerate(STEPS[name]):
        text = apply_step(g, text, step)
        f = ra.Scene(write_scene(tmp_path, text, "%s_%d" % (name, k)), 64, 48)
        what = "%s step %d %r" % (name, k, step[:2])
        assert g.n_lights == f.n_lights, what
        assert [g.light_type(i) for i in range(g.n_lights)] == [f.light_type(i) for i in range(f.n_lights)], what
        assert np.array_equal(digest_bits(g), digest_bits(f)), "%s: the records differ from a fresh load's" % what
        assert serialized(ra, g) == serialized(ra, f), "%s: the serialised description differs from a fresh load's" % what
        f.close()
    assert np.array_equal(digest_bits(g), first_digest.view(np.uint32))
    assert serialized(ra, g) == first_desc
    g.close()


def test_refused_keys_and_indices_leave_the_scene_as_it_was(ra):
    g = ra.Scene("scenes/area_light.scene", 64, 48)          # lights: area, area, point
    before, desc = g.digest(), serialized(ra, g)
    for index, keys in [(2, dict(direction=(0, -1, 0))), (2, dict(pos=(0, 1, 0))), (2, dict(samples=2)), (0, dict(position=(0, 1, 0))),
                        (0, dict(direction=(0, 1, 0))), (0, dict(radius=1.0)), (2, dict(position=(0, 1))), (2, dict(intensity=(1, 2))),
                        (0, dict(samples=(2, 3))), (0, dict(samples=2.5)), (3, dict(color=(1, 1, 1))), (-1, dict(color=(1, 1, 1))),
                        (0, dict(color=(1, 1, 1), i=(1, 0)))]:
        with pytest.raises(ValueError):
            g.set_light(index, **keys)
    for kind, keys in [("spot", {}), ("point", dict(direction=(0, -1, 0))), ("distant", dict(position=(0, 1, 0))), ("area", dict(position=(0, 1, 0))),
                       ("point", dict(position=(1, 2, 3, 4)))]:
        with pytest.raises(ValueError):
            g.add_light(kind, **keys)
    for index in (3, -1, 99):
        with pytest.raises(ValueError):
            g.remove_light(index)
        with pytest.raises(ValueError):
            g.light_type(index)
    assert g.n_lights == 3
    assert np.array_equal(digest_bits(g), before.view(np.uint32)) and serialized(ra, g) == desc
    # the host entry points refuse them as well (NULL = unchanged)
    host = g.host
    v = np.ones(3, np.float32); n = np.array([2], np.int32)
    p, q = v.ctypes.data, n.ctypes.data
    assert [host.rah_light_type(g.h, i) for i in (0, 1, 2, 3, -1)] == [3, 3, 2, -1, -1]
    assert host.rah_light_set(g.h, 2, None, None, p, None, None, None, None, None) != 0 and b"direction" in host.rah_last_error()
    assert host.rah_light_set(g.h, 2, p, None, None, p, None, None, None, q) != 0 and b"samples" in host.rah_last_error()       # (the colour is not taken either)
    assert host.rah_light_set(g.h, 0, None, None, None, p, None, None, None, None) != 0 and b"position" in host.rah_last_error()
    assert host.rah_light_set(g.h, 3, p, None, None, None, None, None, None, None) != 0
    assert host.rah_light_set(g.h, -1, p, None, None, None, None, None, None, None) != 0
    assert host.rah_light_add(g.h, 2, None, None, None, None, p, None, None, None) < 0 and b"pos" in host.rah_last_error()
    assert host.rah_light_add(g.h, 0, None, None, None, None, None, None, None, None) < 0
    assert host.rah_light_add(g.h, 4, None, None, None, None, None, None, None, None) < 0
    assert host.rah_light_remove(g.h, 3) != 0 and host.rah_light_remove(g.h, -1) != 0
    g._dims()
    assert g.n_lights == 3
    assert np.array_equal(digest_bits(g), before.view(np.uint32)) and serialized(ra, g) == desc
    g.close()


def test_an_area_light_gets_its_points_again_only_when_they_change(ra):
    """The host's setPoints latch: the points follow pos / i / j / samples, and a colour edit leaves them alone."""
    g = ra.Scene("scenes/area_light.scene", 64, 48)
    n0 = g.digest().reshape(-1)[-12 * 3 + 11]                  # light 0's n_points in the digest (12 floats per light, the last one)
    assert n0 == 9
    g.set_light(0, samples=4)
    assert g.digest().reshape(-1)[-12 * 3 + 11] == 16
    g.set_light(0, color=(0.5, 0.5, 0.5))
    assert g.digest().reshape(-1)[-12 * 3 + 11] == 16
    g.set_light(0, samples=0)                                  # (samples <= 1: the light's own position, lights.cpp)
    assert g.digest().reshape(-1)[-12 * 3 + 11] == 1
    g.close()


def test_light_edit_symbols_are_declared_where_they_belong(ra):
    edit = open(os.path.join(ROOT, "include", "rtx_scene_edit.h")).read()
    debug = open(os.path.join(ROOT, "include", "rtx_debug.h")).read()
    boundary = open(os.path.join(ROOT, "include", "rtx.h")).read()
    decl = lambda hdr: set(re.findall(r"\b(rtx_[a-z0-9_]+)\s*\(", hdr))
    assert "rtx_scene_set_lights" in decl(edit) and "rtx_scene_set_lights" in ra.RTX_EDIT_SYMBOLS
    for s in ("rtx_scene_lights_read", "rtx_scene_mesh_prune_copy_read"):
        assert s in decl(debug) and s in ra.RTX_SYMBOLS
    for s in ("rtx_scene_set_lights", "rtx_scene_lights_read", "rtx_scene_mesh_prune_copy_read"):
        assert s not in decl(boundary)
    assert len(decl(boundary)) <= 32
    rtx, host = ra.load()
    for s in ("rtx_scene_set_lights", "rtx_scene_lights_read", "rtx_scene_mesh_prune_copy_read"):
        assert hasattr(rtx, s), s
    for s in ("rah_light_type", "rah_light_set", "rah_light_add", "rah_light_remove"):
        assert hasattr(host, s), s
    _, missing = ra.exported_symbols()
    assert not missing
