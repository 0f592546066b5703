"""Objects of a live GPU scene added and removed between frames (Scene.add_object / remove_object -> rtx_scene_set_objects,
include/rtx_scene_edit.h): every state must render, bit for bit, what a fresh scene of the scene file with the [object]
block written or deleted renders -- and the oracle's frame of that file -- in both frame modes and in three launches; the kernel variant,
the scene's bytes, the object records, the flattened tree and EVERY copy of every mesh's prune blocks (a stale source copy carries a bound
certified for the old longest plane normal: it can drop a shadow hit without any other sign) must equal the fresh scene's; the other entry
points must agree with a fresh scene; refused arguments must leave the scene as it was; removed meshes must be freed."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests.test_gpu_lights_edit import bits, frame, stages
from tests.util_lights import add_light, remove_light, set_light
from tests.util_move import edit_scene, same_structure
from tests.util_objects import BUMPY, LONG_PLANE, TORUS_GLASS, TORUS_MAPS, add_object, apply_step, write_scene
from tests.util_rays import probe_rays

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTX_ERR_ARG = -1


def readbacks(g):
    recs, nm = g.device_objects()
    return dict(variant=g.kernel_variant(), bytes=g.scene_bytes(), objects=recs.tobytes(), n_objects=len(recs), n_meshes=nm,
                flat=[g.device_mesh_flat(m) for m in range(nm)], copies=[g.device_prune_copies(m) for m in range(nm)])


def assert_readbacks(got, want, what):
    assert got["variant"] == want["variant"], "%s: kernel variant %r, a fresh scene's %r" % (what, got["variant"], want["variant"])
    assert got["bytes"] == want["bytes"], "%s: scene_bytes %d, a fresh scene's %d" % (what, got["bytes"], want["bytes"])
    assert (got["n_objects"], got["n_meshes"]) == (want["n_objects"], want["n_meshes"]), "%s: %d objects and %d meshes, a fresh scene's %d and %d" % (
        what, got["n_objects"], got["n_meshes"], want["n_objects"], want["n_meshes"])
    assert got["objects"] == want["objects"], "%s: the device's object records differ from a fresh scene's" % what
    for m, (a, b) in enumerate(zip(got["flat"], want["flat"])):
        for part, x, y in zip(("wide nodes", "box records", "plane records", "root record"), a, b):
            assert x.shape == y.shape and np.array_equal(bits(x), bits(y)), "%s: the %s of mesh %d differ from a fresh scene's" % (what, part, m)
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


SPHERE = dict(pos=(0.8, -0.5, -3), radius=0.7, color=(0.9, 0.6, 0.2))
MIRROR = dict(pos=(1.2, -0.8, -2.5), radius=0.6, color=(1, 1, 1), material="reflective")
MIDDLE = dict(pos=(-1.2, 0, -4), size=(1.6, 1.6, 1.6), rot=(20, 30, 10), color=(1, 1, 1), material="transparent,1.3", name="scenes/assets/bumpy_4k.obj")

# name -> (scene, width, height, steps, {step: flag expected after it}, the flag, steps after which the state is the first one again)
SEQUENCES = {
    # no mesh at first: a sphere, a plane with a long normal (srcNmax grows), a mesh (the mesh kernels), a textured mesh in front of
    # everything (every mesh index shifts; tangents), both removed again, every object removed down to none, a sphere added
    "analytic": ("cfg1_simple_shapes", 160, 120,
                 [("add", "sphere", None, SPHERE), ("add", "plane", None, LONG_PLANE), ("add", "mesh", None, BUMPY), ("add", "mesh", 0, TORUS_MAPS),
                  ("remove", 8), ("remove", 0)] + [("remove", (2 * k) % (7 - k)) for k in range(7)] + [("add", "sphere", None, SPHERE)],
                 dict([(0, True), (1, True), (2, False), (3, False), (4, False), (5, True)] + [(6 + k, True) for k in range(8)]), "analytic", ()),
    # PLAIN: a mirror ball added (the PLAIN family no longer holds) and removed, a glass mesh added, the first mesh removed (the new one
    # becomes mesh 0), a mesh inserted in front
    "plain": ("cfg2_smooth_4k", 140, 100,
              [("add", "sphere", None, MIRROR), ("remove", 2), ("add", "mesh", None, TORUS_GLASS), ("remove", 1), ("add", "mesh", 0, BUMPY)],
              {0: False, 1: True, 2: False, 3: False, 4: False}, "plain", (1,)),
    # three meshes: the middle one removed (mesh 2 is carried over as mesh 1) and added again at its index, the sphere and the plane removed
    "three_meshes": ("mixed_materials", 160, 120,
                     [("remove", 1), ("add", "mesh", 1, MIDDLE), ("remove", 3), ("remove", 3)],
                     {0: False, 1: False, 3: False}, "plain", (1,)),
}


@pytest.mark.parametrize("case", sorted(SEQUENCES))
def test_object_edits_equal_fresh_scenes_and_the_oracle(ra, oracle, tmp_path, case):
    name, w, h, steps, flags, flag, back = SEQUENCES[case]
    text = open(os.path.join(ROOT, "scenes", name + ".scene")).read()
    g = ra.Scene("scenes/%s.scene" % name, w, h)
    g.gpu()
    g.set_knob("verify_lists", 1)
    start = state(g, w, h)
    for k, step in enumerate(steps):
        text = apply_step(g, text, step)
        what = "%s step %d %r" % (case, k, step[:3])
        got = assert_fresh(ra, g, write_scene(tmp_path, text, "%s_%d" % (case, k)), w, h, what, oracle)
        if k in flags:
            assert got["read"]["variant"][flag] == flags[k], "%s: the variant's %s is %r" % (what, flag, got["read"]["variant"][flag])
        if k in back:
            assert_state(got, start, "%s: the first state again" % what)
    g.close()


def test_the_order_of_the_objects_matters(ra, oracle, tmp_path):
    """A blue twin of the green sphere, inserted before it and appended: Render::trace keeps the first of two equal hits."""
    name, w, h = "cfg1_simple_shapes", 160, 120
    text = open(os.path.join(ROOT, "scenes", name + ".scene")).read()
    twin = dict(pos=(-0.5, 2, -6), radius=0.5, color=(0, 0, 1))
    frames = []
    for at in (4, None):
        g = ra.Scene("scenes/%s.scene" % name, w, h)
        frame(g, w, h)
        edited = apply_step(g, text, ("add", "sphere", at, twin))
        got = assert_fresh(ra, g, write_scene(tmp_path, edited, "twin_%s" % at), w, h, "a twin sphere at %s" % at, oracle)
        frames.append(got["frames"][0][0])
        g.close()
    assert (bits(frames[0]) != bits(frames[1])).any(-1).sum() >= 1, "the twin's place in the object order changed no pixel"


# ---- through the C ABI directly -----------------------------------------------------------------------------------------------------

class Flat:
    """The flattened description of a host Scene (rah_flatten), alive until close()."""

    def __init__(self, ra, scene):
        self.host = scene.host
        self.flat = C.c_void_p(self.host.rah_flatten(scene.h))
        assert self.flat
        self.desc = C.cast(self.host.rah_flat_desc(self.flat), C.POINTER(ra.RtxSceneDesc)).contents

    def close(self):
        self.host.rah_flat_free(self.flat)


def source(ra, keep=-1, mesh=None, build=None):
    s = ra.RtxMeshSource()
    s.keep = keep
    if mesh is not None:
        s.mesh = C.pointer(mesh)
    if build is not None:
        s.build = C.pointer(build)
    return s


def sources(ra, *items):
    arr = (ra.RtxMeshSource * max(len(items), 1))()
    for i, s in enumerate(items):
        arr[i] = s
    return arr


def device_triangles(ra, mesh, stream=None):
    """(rtx_mesh_build without the root box, what keeps its arrays alive) of an rtx_mesh's triangles.  With a stream the copies are only queued
    on it, from pinned memory: the caller hands that stream to rtx_scene_set_objects, which has to wait for it."""
    def host(ptr, per):
        return torch.from_numpy(np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_float)), (mesh.n_tris * per,)).copy())
    src = [host(mesh.tri_pos, 9), host(mesh.tri_nrm, 9), host(mesh.tri_tb, 6)]
    if stream is None:
        t = [x.cuda() for x in src]
        torch.cuda.synchronize()
    else:
        src = [x.pin_memory() for x in src]
        with torch.cuda.stream(stream):
            t = [x.to("cuda", non_blocking=True) for x in src]
    b = ra.RtxMeshBuild()
    b.tri_pos_dev, b.tri_nrm_dev, b.tri_tb_dev = (x.data_ptr() for x in t)
    return b, (src, t)


def test_a_new_mesh_in_host_form_and_in_device_form(ra, tmp_path):
    name, w, h = "cfg1_simple_shapes", 160, 120
    text = add_object(open(os.path.join(ROOT, "scenes", name + ".scene")).read(), "mesh", 2, **TORUS_MAPS)
    f = ra.Scene(write_scene(tmp_path, text, "abi"), w, h)
    want = state(f, w, h)
    flat = Flat(ra, f)
    d = flat.desc
    assert d.n_meshes == 1 and d.n_objects == 6
    root = f.bvh(2)["bounds"][0]
    # (the third form: the triangles are still on their way, queued on a non-blocking stream that the call is given to wait for)
    for form in ("host", "device", "device, triangles queued on a stream"):
        g = ra.Scene("scenes/%s.scene" % name, w, h)
        frame(g, w, h)
        build, keep, st = None, None, None
        if form != "host":
            st = torch.cuda.Stream() if "stream" in form else None
            build, keep = device_triangles(ra, d.meshes[0], st)
            build.root_lo[:] = root[0:3].tolist(); build.root_hi[:] = root[3:6].tolist()
            build.ac_penalty = 1
        rc = g.rtx.rtx_scene_set_objects(g.gpu(), d.n_objects, d.objects, 1, sources(ra, source(ra, -1, d.meshes[0], build)), st.cuda_stream if st else None)
        assert rc == 0, g.rtx.rtx_last_error()
        assert_state(state(g, w, h), want, "a new mesh in %s form" % form)
        # ... and away again: the scene as it was loaded
        n = g.n_objects
        objs = (ra.RtxObject * 6)(*[d.objects[i] for i in (0, 1, 3, 4, 5)])
        assert g.rtx.rtx_scene_set_objects(g.gpu(), n, objs, 0, None, None) == 0
        first = ra.Scene("scenes/%s.scene" % name, w, h)
        assert_state(state(g, w, h), state(first, w, h), "the new mesh in %s form removed" % form)
        first.close(); g.close()
    flat.close(); f.close()


def test_two_meshes_swapped_with_keep_only(ra, tmp_path):
    name, w, h = "mixed_materials", 160, 120
    lines = open(os.path.join(ROOT, "scenes", name + ".scene")).read().split("\n")
    at = [i for i, l in enumerate(lines) if l.strip() == "[object]"]
    swapped = "\n".join(lines[:at[1]] + lines[at[2]:at[3]] + lines[at[1]:at[2]] + lines[at[3]:])
    f = ra.Scene(write_scene(tmp_path, swapped, "swapped"), w, h)
    want = state(f, w, h)
    flat = Flat(ra, f)
    g = ra.Scene("scenes/%s.scene" % name, w, h)
    frame(g, w, h)
    d = flat.desc
    assert [d.objects[i].mesh for i in range(5)] == [0, 1, 2, -1, -1]
    assert g.rtx.rtx_scene_set_objects(g.gpu(), d.n_objects, d.objects, 3, sources(ra, source(ra, 0), source(ra, 2), source(ra, 1)), None) == 0
    assert_state(state(g, w, h), want, "meshes 1 and 2 swapped")
    flat.close(); f.close(); g.close()


def test_refused_arguments_leave_the_scene_as_it_was(ra):
    name, w, h = "cfg2_smooth_4k", 140, 100
    g = ra.Scene("scenes/%s.scene" % name, w, h)
    want = state(g, w, h)
    rtx, sc = g.rtx, g.gpu()
    flat = Flat(ra, g)
    d = flat.desc
    objs = lambda: (ra.RtxObject * 3)(d.objects[0], d.objects[1], d.objects[1])
    kept = sources(ra, source(ra, 0))
    call = lambda n, o, nm, m: rtx.rtx_scene_set_objects(sc, n, o, nm, m, None)
    assert call(2, None, 1, kept) == RTX_ERR_ARG                                  # NULL arrays with a count
    assert call(2, objs(), 1, None) == RTX_ERR_ARG
    assert rtx.rtx_scene_set_objects(None, 2, objs(), 1, kept, None) == RTX_ERR_ARG
    for field, values in (("type", (0, 4)), ("material", (-1, 4)), ("mesh", (-1, 1, 7))):      # the checks of rtx_scene_create
        for v in values:
            o = objs()
            setattr(o[1], field, v)
            assert call(2, o, 1, kept) == RTX_ERR_ARG, (field, v)
    for keep in (1, 5, -2):                                                       # keep out of range
        assert call(2, objs(), 1, sources(ra, source(ra, keep, d.meshes[0]))) == RTX_ERR_ARG, keep
    o = objs()
    o[2].mesh = 1
    assert call(3, o, 2, sources(ra, source(ra, 0), source(ra, 0))) == RTX_ERR_ARG          # one old mesh kept twice
    # a new mesh with missing arrays: no description; host form without a tree, without triangles; device form without triangles
    mesh = lambda: ra._RtxMesh.from_buffer_copy(d.meshes[0])
    assert call(2, objs(), 1, sources(ra, source(ra, -1))) == RTX_ERR_ARG
    for field in ("node_bounds", "node_skip", "leaf_begin", "leaf_count", "refs", "tri_pos", "tri_nrm", "tri_uv"):
        m = mesh()
        setattr(m, field, None)
        assert call(2, objs(), 1, sources(ra, source(ra, -1, m))) == RTX_ERR_ARG, field
    build, keep = device_triangles(ra, d.meshes[0])
    for field in ("tri_pos_dev", "tri_nrm_dev"):
        b = ra.RtxMeshBuild.from_buffer_copy(build)
        setattr(b, field, None)
        assert call(2, objs(), 1, sources(ra, source(ra, -1, mesh(), b))) == RTX_ERR_ARG, field
    m = mesh()
    m.tri_uv = None
    assert call(2, objs(), 1, sources(ra, source(ra, -1, m, build))) == RTX_ERR_ARG
    m = mesh()
    m.n_tris = 0                                                                  # (no triangles: nothing to build a tree from)
    assert call(2, objs(), 1, sources(ra, source(ra, -1, m, build))) == RTX_ERR_ARG
    # a normal map without tangents, in either form
    px = np.zeros((4, 4, 3), np.float32)
    m = mesh()
    m.normal_w, m.normal_h, m.normal_map, m.tri_tb = 4, 4, px.ctypes.data, None
    assert call(2, objs(), 1, sources(ra, source(ra, -1, m))) == RTX_ERR_ARG
    m.tri_tb = d.meshes[0].tri_tb
    b = ra.RtxMeshBuild.from_buffer_copy(build)
    b.tri_tb_dev = None
    assert call(2, objs(), 1, sources(ra, source(ra, -1, m, b))) == RTX_ERR_ARG
    assert g.n_objects == 2
    assert_state(state(g, w, h), want, "after refused calls")
    flat.close(); g.close()


# ---- the other entry points, other edits, streams, memory ------------------------------------------------------------------------------

def test_other_entry_points_after_an_object_edit(ra, tmp_path):
    name, w, h = "mixed_materials", 160, 160
    text = open(os.path.join(ROOT, "scenes", name + ".scene")).read()
    g = ra.Scene("scenes/%s.scene" % name, w, h)
    frame(g, w, h)
    rays = torch.from_numpy(probe_rays(4096)).cuda()
    g.trace_rays(rays); g.occluded(rays)          # (the ray kernels of the first variant have been asked for)
    dirs = torch.from_numpy(ra.sphere_directions(8)).cuda()

    def queries(s, points=None):
        """The surface, light and scatter queries at the probe rays, and the point queries at `points` (None: at this scene's own hits)."""
        surf = s.surface_rays(rays, hits=True, position=True, normal=True, albedo=True, specular=True)
        if points is None:
            points = torch.cat([surf["position"], surf["normal"]], 1).contiguous()
        out = dict(surface_rays=surf, light_rays=s.light_rays(rays, hits=True, per_light=True), scatter_rays=s.scatter_rays(rays, hits=True),
                   light_points=s.light_points(points, per_light=True), ao_points=s.ao_points(points, dirs, counts=True))
        torch.cuda.synchronize()
        return {call: {ch: t.cpu().numpy() for ch, t in chans.items()} for call, chans in out.items()}, points

    queries(g)                                    # (... and those of the surface, light, scatter and point queries)
    for step in [("remove", 1), ("add", "sphere", None, MIRROR), ("add", "mesh", 0, BUMPY), ("remove", 4)]:
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
    tmax = torch.from_numpy(np.linspace(0.5, 9.0, 4096).astype(np.float32)).cuda()
    for t in (None, tmax):
        assert np.array_equal(g.occluded(rays, t).cpu().numpy(), f.occluded(rays, t).cpu().numpy()), "occluded: differs from a fresh scene's"
    assert g.occluded(rays).cpu().numpy().any()
    # the queries whose kernels were asked for before the edits: every channel, the point queries at the fresh scene's hits for both
    qf, points = queries(f)
    qg, _ = queries(g, points)
    assert (qf["surface_rays"]["hits"][:, 1] >= 0).any() and qf["ao_points"]["counts"].any() and qf["light_points"]["light_open"].any()
    for call in ("surface_rays", "light_rays", "scatter_rays", "light_points", "ao_points"):
        assert list(qg[call]) == list(qf[call])
        for ch in qf[call]:
            a, b = qg[call][ch], qf[call][ch]
            assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a) if a.dtype == np.float32 else a, bits(b) if b.dtype == np.float32 else b), (
                "%s: the channel %s differs from a fresh scene's" % (call, ch))
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
    # the showNormals view, the showAC heat map
    views = []
    for s in (g, f):
        s.set_flag("showNormals", 1)
        views.append(frame(s, w, h))
        s.set_flag("showNormals", 0)
    assert np.array_equal(bits(views[0][0]), bits(views[1][0])) and np.array_equal(views[0][1], views[1][1])
    heat = []
    for s in (g, f):
        fb = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda"); counts = torch.zeros((h, w), dtype=torch.int32, device="cuda")
        s.render_ac(fb, counts)
        torch.cuda.synchronize()
        heat.append((fb.cpu().numpy(), counts.cpu().numpy()))
    assert np.array_equal(bits(heat[0][0]), bits(heat[1][0])) and np.array_equal(heat[0][1], heat[1][1]), "render_ac differs from a fresh scene's"
    assert heat[0][1].max() > 0
    for m in (0, 1):
        a, b = frame(g, w, h, m), frame(f, w, h, m)
        assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1])
    # the host's trees follow the device's (a mesh added to a live scene is built there)
    for i in (0, 1, 2):
        assert same_structure(g.bvh(i), f.bvh(i)) is None, "bvh(%d) differs from a fresh load's" % i
    f.close(); g.close()


def test_object_edits_interleaved_with_moves_lights_and_views(ra, tmp_path):
    name, w, h = "cfg2_smooth_25k", 224, 160
    text = open(os.path.join(ROOT, "scenes", name + ".scene")).read()
    g = ra.Scene("scenes/%s.scene" % name, w, h)
    frame(g, w, h)
    point = dict(position=(1.6, 1.2, -1.8), color=(0.4, 0.5, 0.9), intensity=0.3)
    # an object edit, then the kept and the new mesh moved, a light moved and one added (four source copies instead of three)
    text = apply_step(g, text, ("add", "mesh", 0, BUMPY))
    move = dict(pos=(0.3, 0.1, -3.3), rot=(10, 30, 0))
    g.move_object(2, **move)
    g.move_object(0, pos=(1.1, -0.3, -3.0))
    g.set_light(1, position=(1.4, -0.6, -1.6))
    g.add_light("point", **point)
    text = add_light(set_light(edit_scene(edit_scene(text, 2, **move), 0, pos=(1.1, -0.3, -3.0)), 1, position=(1.4, -0.6, -1.6)), "point", **point)
    assert_fresh(ra, g, write_scene(tmp_path, text, "edit_first"), w, h, "add_object, then moves and light edits")
    # a mesh moved and the lights edited, then object edits (the kept mesh's copies are laid out for the lights of the moment)
    move = dict(pos=(-0.2, 0.0, -3.1), size=(1.7, 2.1, 1.9))
    g.move_object(2, **move)
    g.remove_light(0)
    text = remove_light(edit_scene(text, 2, **move), 0)
    text = apply_step(g, text, ("remove", 0))
    text = apply_step(g, text, ("add", "plane", None, LONG_PLANE))
    assert_fresh(ra, g, write_scene(tmp_path, text, "edit_last"), w, h, "moves and light edits, then object edits")
    # an object edit, a new view, the earlier view again
    pos, rot = g.camera_pose()
    text = apply_step(g, text, ("add", "sphere", 1, SPHERE))
    path = write_scene(tmp_path, text, "views")
    there = (np.float32([0.8, 0.5, 0.6]), np.float32([-6, 14, 2]))
    g.set_camera(*there)
    assert_fresh(ra, g, path, w, h, "object edit, then a new view", prepare=lambda f: f.set_camera(*there))
    g.set_camera(pos, rot)
    assert_fresh(ra, g, path, w, h, "object edit, a new view, the earlier view again")
    # a new view first, then the edit
    g.set_camera(*there)
    frame(g, w, h)
    text = apply_step(g, text, ("remove", 1))
    assert_fresh(ra, g, write_scene(tmp_path, text, "view_first"), w, h, "a new view, then an object edit", prepare=lambda f: f.set_camera(*there))
    g.close()


def test_renders_on_a_non_blocking_stream_around_an_object_edit(ra, tmp_path):
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
                g.add_object("mesh", 0, **TORUS_GLASS)        # (waits for the frame queued before it)
    st.synchronize()
    f = ra.Scene(write_scene(tmp_path, add_object(text, "mesh", 0, **TORUS_GLASS), "stream"), w, h)
    want1 = frame(f, w, h, 0)
    f.close()
    for k, ((fb, mask), (wf, wm)) in enumerate(zip(fbs, (want0, want1))):
        assert np.array_equal(bits(fb.cpu().numpy()), bits(wf)) and np.array_equal(mask.cpu().numpy(), wm), "the frame queued %s the edit" % ("before", "after")[k]
    g.close()


def test_removed_meshes_are_freed(ra, tmp_path):
    """A textured mesh added and removed again, 30 times."""
    name, w, h = "cfg2_smooth_4k", 140, 100
    text = open(os.path.join(ROOT, "scenes", name + ".scene")).read()
    fresh = []
    for t, tag in ((add_object(text, "mesh", None, **TORUS_MAPS), "with"), (text, "without")):
        f = ra.Scene(write_scene(tmp_path, t, "freed_" + tag), w, h)
        fresh.append(f.scene_bytes())
        f.close()
    g = ra.Scene("scenes/%s.scene" % name, w, h)
    frame(g, w, h)
    sizes, live = [], {}
    for k in range(1, 31):
        assert g.add_object("mesh", **TORUS_MAPS) == 2
        sizes.append(g.scene_bytes())
        if k in (1, 2, 30):
            frame(g, w, h)
        g.remove_object(2)
        sizes.append(g.scene_bytes())
        if k in (1, 2, 30):
            frame(g, w, h)
        live[k] = ra.live_device_memory()
    assert live[30] == live[2], "device memory after the 30th round %r, after the 2nd %r" % (live[30], live[2])
    assert sizes[0::2] == [fresh[0]] * 30 and sizes[1::2] == [fresh[1]] * 30, "scene_bytes: %r, fresh scenes' %r" % (sorted(set(sizes)), fresh)
    assert fresh[0] > fresh[1]
    g.close()
