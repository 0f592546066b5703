"""The lights of a live GPU scene changed, added and removed between frames (Scene.set_light / add_light / remove_light ->
rtx_scene_set_lights, include/rtx_scene_edit.h): every state must render, bit for bit, what a fresh scene of the scene file
with the edited [light] blocks renders -- and the oracle's frame of that file -- in both frame modes and in three launches; the kernel
variant, the scene's bytes, the light records and EVERY copy of every mesh's prune blocks (a stale source copy carries a bound certified for
the old light position: it can drop a shadow hit without any other sign) must equal the fresh scene's; the other entry points must agree
with a fresh scene; refused arguments must leave the scene as it was; replaced lights must be freed."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests.util_lights import add_light, apply_step, remove_light, replace_light, set_light, write_scene
from tests.util_move import edit_scene
from tests.util_rays import probe_rays

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTX_ERR_ARG = -1


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def frame(g, w, h, mode=-1, stream=None):
    fb = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
    mask = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
    g.set_frame_mode(mode)
    g.render_frame(fb, mask, stream=stream)
    torch.cuda.synchronize()
    assert g.frame_status() == 0
    return fb.cpu().numpy(), mask.cpu().numpy()


def stages(g, w, h):
    """render_pass1 + sobel + render_ssaa"""
    fb = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
    mask = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
    g.render_pass1(fb)
    g.sobel(fb, mask)
    g.render_ssaa(mask, fb)
    torch.cuda.synchronize()
    return fb.cpu().numpy(), mask.cpu().numpy()


def n_meshes(g):
    return sum(1 for i in range(g.n_objects) if g.host.rah_object_type(g.h, i) == 3)


def readbacks(g):
    recs, pts = g.device_lights()
    return dict(variant=g.kernel_variant(), bytes=g.scene_bytes(), lights=recs.tobytes(), n_lights=len(recs), points=bits(pts).tobytes(),
                copies=[g.device_prune_copies(m) for m in range(n_meshes(g))])


def assert_readbacks(got, want, what):
    assert got["variant"] == want["variant"], "%s: kernel variant %r, a fresh scene's %r" % (what, got["variant"], want["variant"])
    assert got["bytes"] == want["bytes"], "%s: scene_bytes %d, a fresh scene's %d" % (what, got["bytes"], want["bytes"])
    assert got["n_lights"] == want["n_lights"] and got["lights"] == want["lights"], "%s: the device's light records differ from a fresh scene's" % what
    assert got["points"] == want["points"], "%s: the device's area-light points differ from a fresh scene's" % what
    assert len(got["copies"]) == len(want["copies"])
    for m, (a, b) in enumerate(zip(got["copies"], want["copies"])):
        assert a.shape == b.shape, "%s: mesh %d holds %d copies of its prune blocks, a fresh scene's %d" % (what, m, a.shape[0], b.shape[0])
        for c in range(a.shape[0]):
            assert np.array_equal(bits(a[c]), bits(b[c])), "%s: copy %d of mesh %d's prune blocks differs from a fresh scene's" % (what, c, m)


def state(g, w, h):
    return dict(frames=[frame(g, w, h, m) for m in (0, 1)], stages=stages(g, w, h), read=readbacks(g))


def assert_state(got, want, what):
    for mode in (0, 1):
        (a, am), (b, bm) = got["frames"][mode], want["frames"][mode]
        assert np.array_equal(bits(a), bits(b)), "%s mode %d: %d pixels differ from a fresh scene's" % (what, mode, int((bits(a) != bits(b)).any(-1).sum()))
        assert np.array_equal(am, bm), "%s mode %d: the SSAA mask differs from a fresh scene's" % (what, mode)
    (a, am), (b, bm) = got["stages"], want["stages"]
    assert np.array_equal(bits(a), bits(b)) and np.array_equal(am, bm), "%s: pass 1 + sobel + ssaa differ from a fresh scene's" % what
    assert_readbacks(got["read"], want["read"], what)


def assert_fresh(ra, g, path, w, h, what, oracle=None, prepare=None):
    """The live scene g against a fresh Scene of the file at `path` (and the oracle's frame of it)."""
    f = ra.Scene(path, w, h)
    if prepare:
        prepare(f)
    f.gpu()
    f.set_knob("verify_lists", 1)
    got = state(g, w, h)
    assert_state(got, state(f, w, h), what)
    f.close()
    if oracle is not None:
        o = oracle.OracleScene(path, w, h)
        ref = o.ssaa(o.pass1())
        for mode in (0, 1):
            d = (bits(got["frames"][mode][0]) != bits(ref)).any(-1)
            d[0, :] = False; d[:, 0] = False          # (the reference's uninitialised mask border)
            assert not d.any(), "%s mode %d: %d pixels differ from the oracle" % (what, mode, int(d.sum()))
    return got


def extra_point(k):
    """the k-th point light the sequences add (spread round the meshes of the scenes)"""
    a = 0.9 * k + 0.3
    return dict(position=(2.2 * np.cos(a), 1.0 + 0.35 * k, -3.0 + 2.2 * np.sin(a)), color=(0.3 + 0.1 * (k % 3), 0.5, 0.9 - 0.1 * (k % 4)), intensity=0.15 + 0.05 * k)


AREA = dict(pos=(0.5, 2.5, -2.0), i=(1.0, 0, 0.2), j=(0, 0.1, 1.0), samples=3, color=(1, 0.9, 0.8), intensity=0.6)

# name -> (scene, width, height, steps, {step: RTX_VARIANT_PLAIN expected after it})
SEQUENCES = {
    # PLAIN, three point lights: moved, recoloured, a point light turned into a distant one (removed, the new one at the end), point lights
    # added up to 9 (kMaxSrcLights = 6 copies and the estimate's 8 lights are crossed), removed down to 2 (from the front, the middle and
    # the end: every light behind a removed one is at another index), all removed, one added
    "4k_points": ("cfg2_smooth_4k", 140, 100,
                  [("set", 0, dict(position=(0.6, 2.3, -1.5))),
                   ("set", 1, dict(color=(0.2, 0.9, 0.5), intensity=0.55)),
                   ("remove", 2), ("add", "distant", dict(direction=(-0.3, -1, -0.4), color=(0, 0, 1), intensity=0.9))] +
                  [("add", "point", extra_point(k)) for k in range(6)] +
                  [("remove", 0), ("remove", 3), ("remove", 6), ("remove", 1), ("remove", 1), ("remove", 3), ("remove", 0)] +
                  [("remove", 1), ("remove", 0), ("add", "point", extra_point(7))],
                  {0: True, 9: True, 18: True, 19: True}),
    # an area light added (the PLAIN family no longer holds), its samples, edges and position changed, removed (PLAIN again)
    "4k_area": ("cfg2_smooth_4k", 140, 100,
                [("add", "area", AREA), ("set", 3, dict(samples=1)), ("set", 3, dict(samples=5)),
                 ("set", 3, dict(i=(0.6, 0.2, 0), j=(0.1, 0, 0.7), pos=(-0.4, 2.2, -2.4))), ("remove", 3)],
                {0: False, 1: False, 2: False, 3: False, 4: True}),
    # every material, two area lights and a point light: each moved, then two swapped in the order (castRay sums in light order)
    "area_light": ("area_light", 160, 120,
                   [("set", 0, dict(pos=(0.5, 2.7, -2.5))), ("set", 1, dict(pos=(-2.5, 1.4, -1.5))), ("set", 2, dict(position=(1.6, 2.4, -0.6))),
                    ("remove", 1), ("add", "area", dict(pos=(-2.5, 1.4, -1.5), i=(0, 0.8, 0), j=(0, 0, 0.8), samples=1, color=(0.4, 0.5, 1), intensity=1.5))],
                   {0: False, 4: False}),
    "mixed_materials": ("mixed_materials", 160, 120,
                        [("set", 0, dict(position=(1.2, 2.6, -1.0))), ("set", 1, dict(direction=(0.3, -1, -0.5))),
                         ("remove", 0), ("add", "point", dict(position=(1.2, 2.6, -1.0), color=(1, 0.9, 0.8), intensity=0.8))],
                        {0: False}),
    # no mesh: spheres and planes only
    "analytic": ("cfg1_simple_shapes", 160, 120,
                 [("set", 0, dict(position=(-0.4, 1.6, -2.2))), ("set", 1, dict(direction=(0.2, -1, -0.1))), ("add", "point", extra_point(2)),
                  ("add", "area", AREA)],
                 {}),
}


@pytest.mark.parametrize("case", sorted(SEQUENCES))
def test_light_edits_equal_fresh_scenes_and_the_oracle(ra, oracle, tmp_path, case):
    name, w, h, steps, plain = SEQUENCES[case]
    text = open(os.path.join(ROOT, "scenes", name + ".scene")).read()
    g = ra.Scene("scenes/%s.scene" % name, w, h)
    g.gpu()
    g.set_knob("verify_lists", 1)
    frame(g, w, h)
    for k, step in enumerate(steps):
        text = apply_step(g, text, step)
        what = "%s step %d %r" % (case, k, step[:2])
        got = assert_fresh(ra, g, write_scene(tmp_path, text, "%s_%d" % (case, k)), w, h, what, oracle)
        if k in plain:
            assert got["read"]["variant"]["plain"] == plain[k], "%s: RTX_VARIANT_PLAIN is %r" % (what, got["read"]["variant"]["plain"])
    g.close()


class Light(C.Structure):
    _fields_ = [("type", C.c_int32), ("color", C.c_float * 3), ("intensity", C.c_float), ("dir", C.c_float * 3), ("pos", C.c_float * 3),
                ("n_points", C.c_uint32), ("points", C.c_void_p)]


def light_array(g):
    """The device's lights as an array of rtx_light for rtx_scene_set_lights (the scenes used with it have no area light)."""
    recs, _ = g.device_lights()
    arr = (Light * max(len(recs), 1))()
    for i, r in enumerate(recs):
        assert r["type"] != 3
        arr[i].type = int(r["type"]); arr[i].color[:] = r["color"].tolist(); arr[i].intensity = float(r["intensity"])
        arr[i].dir[:] = r["dir"].tolist(); arr[i].pos[:] = r["pos"].tolist(); arr[i].n_points = int(r["n_points"])
    return arr, len(recs)


def test_a_type_changed_in_place_through_the_c_abi(ra, oracle, tmp_path):
    """Light 1 of three point lights becomes a distant light at its index (one rtx_scene_set_lights): its source copy holds copy 0's
    content again, light 2 keeps its copy; and back."""
    name, w, h = "cfg2_smooth_4k", 140, 100
    text = open(os.path.join(ROOT, "scenes", name + ".scene")).read()
    g = ra.Scene("scenes/%s.scene" % name, w, h)
    start = state(g, w, h)
    arr, n = light_array(g)
    keep = Light.from_buffer_copy(arr[1])
    arr[1].type = 1
    arr[1].dir[:] = (0.25, -1.0, 0.5)
    arr[1].pos[:] = (0, 0, 0)
    assert g.rtx.rtx_scene_set_lights(g.gpu(), n, arr) == 0
    there = replace_light(text, 1, "distant", direction=(0.25, -1.0, 0.5), color=tuple(keep.color), intensity=keep.intensity)
    got = assert_fresh(ra, g, write_scene(tmp_path, there, "inplace"), w, h, "point -> distant in place", oracle)
    c = got["read"]["copies"][0]
    assert np.array_equal(bits(c[3]), bits(c[0])), "the copy of a light that is no point light must hold copy 0's content"
    assert not np.array_equal(bits(c[2]), bits(c[0])) and not np.array_equal(bits(c[4]), bits(c[0])), "the point lights' copies were not built"
    arr[1] = keep
    assert g.rtx.rtx_scene_set_lights(g.gpu(), n, arr) == 0
    assert_state(state(g, w, h), start, "back to a point light in place")
    g.close()


def test_a_sequence_that_returns_to_the_start(ra):
    name, w, h = "cfg2_smooth_25k", 224, 160
    g = ra.Scene("scenes/%s.scene" % name, w, h)
    start = state(g, w, h)
    g.set_light(0, position=(0.6, 2.3, -1.5), color=(0.5, 0.5, 0))
    assert g.add_light("area", **AREA) == 3
    frame(g, w, h)
    g.set_light(3, samples=2)
    for k in range(4):
        g.add_light("point", **extra_point(k))          # (8 lights: more than have a source copy)
    state(g, w, h)
    for index in (7, 3, 3, 3, 3):
        g.remove_light(index)
    g.set_light(0, position=(0, 2, -1), color=(1, 0, 0))
    assert g.n_lights == 3
    assert_state(state(g, w, h), start, "back at the first lights")
    g.close()


def test_light_edits_interleaved_with_moves_and_views(ra, tmp_path):
    name, w, h = "cfg2_smooth_25k", 224, 160
    text = open(os.path.join(ROOT, "scenes", name + ".scene")).read()
    g = ra.Scene("scenes/%s.scene" % name, w, h)
    frame(g, w, h)
    # a light edit, then a mesh moved
    g.set_light(1, position=(1.4, -0.6, -1.6))
    g.add_light("point", **extra_point(1))
    text = add_light(set_light(text, 1, position=(1.4, -0.6, -1.6)), "point", **extra_point(1))
    move = dict(pos=(0.3, 0.1, -3.3), rot=(10, 30, 0))
    g.move_object(1, **move)
    text = edit_scene(text, 1, **move)
    assert_fresh(ra, g, write_scene(tmp_path, text, "light_move"), w, h, "light edit, then move_object")
    # a mesh moved, then a light edit (the new mesh's copies are laid out for the lights of the moment)
    move = dict(pos=(-0.2, 0.0, -3.1), size=(1.7, 2.1, 1.9))
    g.move_object(1, **move)
    text = edit_scene(text, 1, **move)
    g.remove_light(0)
    g.set_light(0, position=(0.9, -0.4, -1.2))
    text = set_light(remove_light(text, 0), 0, position=(0.9, -0.4, -1.2))
    assert_fresh(ra, g, write_scene(tmp_path, text, "move_light"), w, h, "move_object, then light edit")
    # a light edit, a new view, the earlier view again
    pos, rot = g.camera_pose()
    g.set_light(2, position=(-1.3, 0.8, -1.9))
    text = set_light(text, 2, position=(-1.3, 0.8, -1.9))
    path = write_scene(tmp_path, text, "views")
    there = (np.float32([0.8, 0.5, 0.6]), np.float32([-6, 14, 2]))
    g.set_camera(*there)
    assert_fresh(ra, g, path, w, h, "light edit, then a new view", prepare=lambda f: f.set_camera(*there))
    g.set_camera(pos, rot)
    assert_fresh(ra, g, path, w, h, "light edit, a new view, the earlier view again")
    g.close()


def test_other_entry_points_after_a_light_edit(ra, tmp_path):
    name, w, h = "mixed_materials", 160, 160
    text = open(os.path.join(ROOT, "scenes", name + ".scene")).read()
    g = ra.Scene("scenes/%s.scene" % name, w, h)
    frame(g, w, h)
    rays = torch.from_numpy(probe_rays(4096)).cuda()
    occluded_before = g.occluded(rays).cpu().numpy()
    for step in [("set", 0, dict(position=(1.3, 2.4, -0.8), intensity=0.7)), ("add", "point", extra_point(3)), ("add", "area", AREA)]:
        text = apply_step(g, text, step)
    f = ra.Scene(write_scene(tmp_path, text, "entry"), w, h)
    hg, cg = g.trace_rays(rays)
    hf, cf = f.trace_rays(rays)
    torch.cuda.synchronize()
    assert np.array_equal(bits(hg.cpu().numpy()), bits(hf.cpu().numpy())), "trace_rays: the hits differ from a fresh scene's"
    assert np.array_equal(bits(cg.cpu().numpy()), bits(cf.cpu().numpy())), "trace_rays: the colours differ from a fresh scene's"
    host_rays = probe_rays(256)
    for a, b, what in zip(g.cast_rays(host_rays), f.cast_rays(host_rays), ("hits", "colours")):
        assert np.array_equal(bits(a), bits(b)), "cast_rays: the %s differ from a fresh scene's" % what
    assert np.array_equal(g.occluded(rays).cpu().numpy(), occluded_before), "occluded: changed by a light edit"
    assert np.array_equal(f.occluded(rays).cpu().numpy(), occluded_before)
    # the instrumented pass 1 and its counters
    p1 = []
    for s in (g, f):
        s.counters_enable(True); s.counters_reset()
        fb = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
        s.render_pass1(fb)
        torch.cuda.synchronize()
        p1.append((fb.cpu().numpy(), s.counters(), s.moot_rays))
        s.counters_enable(False)
    assert np.array_equal(bits(p1[0][0]), bits(p1[1][0]))
    assert np.array_equal(p1[0][1], p1[1][1]) and p1[0][2] == p1[1][2], "counters %r moot %d, a fresh scene's %r moot %d" % (p1[0][1], p1[0][2], p1[1][1], p1[1][2])
    assert p1[0][1][0] > 0
    # a frame under row ownership, two parts
    for part in (0, 1):
        own = []
        for s in (g, f):
            s.set_row_ownership(64, 2, part, True)
            own.append([frame(s, w, h, m) for m in (0, 1)])
            s.set_row_ownership(0, 1, 0, False)
        for m in (0, 1):
            assert np.array_equal(bits(own[0][m][0]), bits(own[1][m][0])) and np.array_equal(own[0][m][1], own[1][m][1]), "part %d of 2, mode %d" % (part, m)
    # the showNormals view
    views = []
    for s in (g, f):
        s.set_flag("showNormals", 1)
        views.append(frame(s, w, h))
        s.set_flag("showNormals", 0)
    assert np.array_equal(bits(views[0][0]), bits(views[1][0])) and np.array_equal(views[0][1], views[1][1])
    for m in (0, 1):
        a, b = frame(g, w, h, m), frame(f, w, h, m)
        assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1])
    f.close(); g.close()


def test_renders_on_a_non_blocking_stream_around_a_light_edit(ra, tmp_path):
    name, w, h = "cfg2_smooth_4k", 140, 100
    text = open(os.path.join(ROOT, "scenes", name + ".scene")).read()
    before = ra.Scene("scenes/%s.scene" % name, w, h)
    want0 = frame(before, w, h, 0)
    before.close()
    g = ra.Scene("scenes/%s.scene" % name, w, h)
    st = torch.cuda.Stream()
    fbs = []
    with torch.cuda.stream(st):
        for k in range(2):
            fb = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda"); mask = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
            g.render_frame(fb, mask, stream=st)
            fbs.append((fb, mask))
            if k == 0:
                g.set_light(2, position=(-0.4, 1.5, -1.2), intensity=0.5)        # (waits for the frame queued before it)
    st.synchronize()
    f = ra.Scene(write_scene(tmp_path, set_light(text, 2, position=(-0.4, 1.5, -1.2), intensity=0.5), "stream"), w, h)
    want1 = frame(f, w, h, 0)
    f.close()
    for k, ((fb, mask), (wf, wm)) in enumerate(zip(fbs, (want0, want1))):
        assert np.array_equal(bits(fb.cpu().numpy()), bits(wf)) and np.array_equal(mask.cpu().numpy(), wm), "the frame queued %s the edit" % ("before", "after")[k]
    g.close()


def test_refused_lights_leave_the_scene_as_it_was(ra):
    name, w, h = "cfg2_smooth_4k", 140, 100
    g = ra.Scene("scenes/%s.scene" % name, w, h)
    want = state(g, w, h)
    rtx, sc = g.rtx, g.gpu()
    arr, n = light_array(g)
    assert rtx.rtx_scene_set_lights(sc, 2, None) == RTX_ERR_ARG                  # NULL lights with a count
    arr[1].type = 0
    assert rtx.rtx_scene_set_lights(sc, n, arr) == RTX_ERR_ARG                   # no RTX_LIGHT_*
    arr[1].type = 4
    assert rtx.rtx_scene_set_lights(sc, n, arr) == RTX_ERR_ARG
    pts = np.zeros((4, 3), np.float32)
    arr[1].type = 3; arr[1].n_points = 4; arr[1].points = None
    assert rtx.rtx_scene_set_lights(sc, n, arr) == RTX_ERR_ARG                   # an area light without points
    arr[1].n_points = 0; arr[1].points = pts.ctypes.data
    assert rtx.rtx_scene_set_lights(sc, n, arr) == RTX_ERR_ARG
    assert rtx.rtx_scene_set_lights(None, n, arr) == RTX_ERR_ARG
    assert g.n_lights == 3
    assert_state(state(g, w, h), want, "after refused calls")
    g.close()


def test_replaced_lights_are_freed(ra):
    """Two light sets in turn, 50 times: three point lights; five lights, one of them an area light (another number of copies of the
    prune blocks, another kernel family, sample points)."""
    name, w, h = "cfg2_smooth_4k", 140, 100
    g = ra.Scene("scenes/%s.scene" % name, w, h)
    frame(g, w, h)
    a, na = light_array(g)
    pts = np.ascontiguousarray(np.random.default_rng(5).uniform(-1, 1, (9, 3)) + [0, 2.5, -2], np.float32)
    b = (Light * 5)()
    for i in range(3):
        b[i] = Light.from_buffer_copy(a[i])
    b[3].type = 3; b[3].color[:] = (1, 1, 1); b[3].intensity = 0.5; b[3].pos[:] = (0, 2.5, -2); b[3].n_points = 9; b[3].points = pts.ctypes.data
    b[4].type = 2; b[4].color[:] = (0.5, 0.5, 1); b[4].intensity = 0.3; b[4].pos[:] = (1.5, 1.0, -2.0)
    sizes, live = [], {}
    for k in range(1, 51):
        arr, n = (b, 5) if k % 2 else (a, na)
        assert g.rtx.rtx_scene_set_lights(g.gpu(), n, arr) == 0
        if k in (1, 2, 49, 50):
            frame(g, w, h)
        sizes.append(g.scene_bytes())
        live[k] = ra.live_device_memory()
    assert live[50] == live[2], "device memory after the 50th alternation %r, after the 2nd %r" % (live[50], live[2])
    assert live[49] == live[3]
    assert len(set(sizes)) == 2 and sizes[0::2] == [sizes[0]] * 25 and sizes[1::2] == [sizes[1]] * 25, "scene_bytes: %r" % sorted(set(sizes))
    assert sizes[0] > sizes[1]
    g.close()
