"""The device build (rtx_bvh.hip), the device flatten (rtx_flatten.hip) and the mesh walks (rtx_kernels.hip) on the adversarial meshes of
tests/util_adversarial.py -- a root that is a leaf, trees of a few nodes, leaves of 63 .. 200 coincident triangles, slivers referenced
many times over, boxes without extent, zero-edge and collinear triangles, plane records without a bound, a tree of exactly ten wide levels
and one of eleven (no wide tree: the product kernels walk it in the binary form).  tests/test_adversarial_meshes_cpu.py asserts, without a
GPU, that every family has that property, and that the oracle equals the reference on every scene form.
  (a) rtx_bvh_build against the host builder, in both of its modes, on every raw form;
  (b) a mesh added to a live scene and moved (the device form: build and flatten on the device) against fresh scenes and the oracle;
  (c) rays aimed at the triangles through every ray query, against the oracle;
  (d) raw triangles handed to rtx_scene_update_mesh through the C ABI against the host builder and the host flatten.  No frame is compared
      in (d): no scene file describes those triangles.
Everything is compared bit for bit.  Every coordinate is finite with |x| <= 2^10, the domain of the reference's builder."""
import ctypes as C

import numpy as np
import pytest

from tests import util_adversarial as A
from tests import util_occlusion as OC
from tests import util_surface as SU
from tests.test_gpu_margins import ray_families
from tests.test_gpu_move_objects import check_structures
from tests.test_gpu_objects_edit import assert_fresh
from tests.util_move import edit_scene
from tests.util_objects import add_object, write_scene

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

W, H = A.W, A.H
TREE = ("bounds", "skip", "leaf_begin", "leaf_count", "refs")
FLAT = ("wide nodes", "box records", "plane records", "root record")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_tree(got, want):
    """the first array of TREE that differs, or None"""
    for k in TREE:
        if got[k].shape != want[k].shape or got[k].tobytes() != want[k].tobytes():
            return k
    return None


# ---- (a) the builder ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", A.RAW_NAMES)
def test_device_build_equals_host_build(ra, name):
    t, lo, hi, pens = A.raw_form(name)
    for pen in pens:
        want = ra.bvh_build_host(t, lo, hi, pen)
        try:
            for mode in (0, 1):
                ra.bvh_build_mode(mode)
                got = ra.bvh_build(t, lo, hi, pen)
                what = "%s penalty %d, %s" % (name, pen, ("the persistent launches", "level by level")[mode])
                assert same_tree(got, want) is None, "%s: %s differs from the host builder's" % (what, same_tree(got, want))
                assert got["max_depth"] == want["max_depth"], "%s: %d levels, the host builder's %d" % (what, got["max_depth"], want["max_depth"])
                assert got["queued"] == (mode == 0), "%s: queued is %r" % (what, got["queued"])
        finally:
            ra.bvh_build_mode(0)


# ---- (b) live edits -----------------------------------------------------------------------------------------------------------------------

def live_scene(ra, tmp_path, name, cull, pen):
    """(a live GPU scene of the family's base scene with its mesh added by add_object, the scene text of that state)"""
    base, keys, text = A.scene_form(name, tmp_path, cull, pen)
    g = ra.Scene(write_scene(tmp_path, base, "base"), W, H)
    g.gpu()
    g.set_knob("verify_lists", 1)
    assert g.add_object("mesh", **keys) == 1
    return g, text


def assert_structures(ra, g, path, what):
    f = ra.Scene(path, W, H)
    check_structures(ra, g, f)
    assert same_tree(g.device_mesh(0), f.bvh(1)) is None, what
    f.close()


@pytest.mark.parametrize("name,cull,pen", A.CASES)
def test_added_and_moved_mesh_equals_fresh_scenes_and_the_oracle(ra, oracle, tmp_path, name, cull, pen):
    g, text = live_scene(ra, tmp_path, name, cull, pen)
    states = [("add", None)] + A.moves(name)
    for tag, mv in states:
        if mv:
            g.move_object(1, **mv)
            text = edit_scene(text, 1, **mv)
        what = "%s cull %d penalty %d, %s" % (name, cull, pen, tag)
        path = write_scene(tmp_path, text, tag)
        assert_fresh(ra, g, path, W, H, what, oracle)
        assert_structures(ra, g, path, what)
        if name in A.DEEP and tag in ("add", "shift"):
            n = len(g.device_mesh_flat(0)[0])
            assert n == A.DEEP_WIDE[name], "%s: %d wide nodes on the device, %d expected" % (what, n, A.DEEP_WIDE[name])
            assert not g.kernel_variant()["stats"]      # (the product kernels, not the instrumented ones)
    g.close()


# ---- (c) aimed rays ---------------------------------------------------------------------------------------------------------------------

def differing(rays, got, want, what):
    bad = (bits(got) != bits(want)).reshape(len(rays), -1).any(1)
    assert not bad.any(), "%s: %d of %d rays differ, first %d: ray %s oracle %s gpu %s" % (
        what, int(bad.sum()), len(rays), int(np.argmax(bad)), rays[np.argmax(bad)], want[np.argmax(bad)], got[np.argmax(bad)])


@pytest.mark.parametrize("name,cull,pen", A.CASES)
def test_aimed_rays_through_every_query(ra, oracle, tmp_path, name, cull, pen):
    g, text = live_scene(ra, tmp_path, name, cull, pen)
    path = write_scene(tmp_path, text, "rays")
    tree = g.bvh(1)
    rays = A.aimed_rays(ray_families, tree["tris"][:, 0:9], A.ray_seed(name))
    o = oracle.OracleScene(path, W, H)
    exp = SU.expected(o, text, rays)
    rh, rc = o.probe(rays)
    o.close()
    what = "%s cull %d penalty %d" % (name, cull, pen)
    hit, tnear = rh[:, 0] > 0, rh[:, 3].astype(np.float32)
    assert 4 * int(hit.sum()) >= len(rays)
    gh, gc = g.cast_rays(rays)
    differing(rays, gh, rh, what + ", cast_rays hits"); differing(rays, gc, rc, what + ", cast_rays colours")
    dev = torch.from_numpy(rays).cuda()
    for reorder in (0, 1):
        g.set_knob("trace_reorder", reorder)
        th, tc = g.trace_rays(dev)
        torch.cuda.synchronize()
        differing(rays, th.cpu().numpy(), rh, "%s, trace_rays hits (trace_reorder %d)" % (what, reorder))
        differing(rays, tc.cpu().numpy(), rc, "%s, trace_rays colours (trace_reorder %d)" % (what, reorder))
        for label, tmax in (("none", None), ("mix", OC.tmax_mix(hit, tnear))):
            got = g.occluded(dev, None if tmax is None else torch.from_numpy(tmax).cuda())
            torch.cuda.synchronize()
            want = OC.expected(hit, tnear, np.float32(np.inf) if tmax is None else tmax)
            bad = got.cpu().numpy() != want
            assert not bad.any(), "%s, occluded with ranges %s (trace_reorder %d): %d of %d rays differ, first %d: ray %s oracle %s" % (
                what, label, reorder, int(bad.sum()), len(rays), int(np.argmax(bad)), rays[np.argmax(bad)], rh[np.argmax(bad)])
        out = g.surface_rays(dev, hits=True, position=True, normal=True, albedo=True, specular=True)
        torch.cuda.synchronize()
        bad = SU.mismatches({c: t.cpu().numpy() for c, t in out.items()}, exp)
        assert not bad, "%s, surface_rays (trace_reorder %d): rays that differ from the expectation, per channel: %s" % (what, reorder, bad)
    if name.startswith("stack_"):
        # k coincident triangles are an exact tie of t in every lane: the reference keeps the first in leaf order
        on_stack, first = A.stack_hits(name, tree, gh)
        assert on_stack.sum() > len(rays) // 50, "%s: %d rays hit the stack" % (what, int(on_stack.sum()))
        assert (gh[on_stack, 2] == first).all(), "%s: a hit on the stack names another triangle than the leaf's first, %d" % (what, first)
    g.close()


# ---- (d) raw triangles through the C ABI --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["tiny", "stack_129", "slivers", "deep_edge", "deep_over"])
def test_raw_triangles_through_update_mesh(ra, tmp_path, name):
    """rtx_scene_update_mesh on a scene whose mesh has as many triangles: the device's tree, wide nodes, records and copy 0 of its prune
    blocks against the host builder and the host flatten of the same triangles and box."""
    t, lo, hi, pens = A.raw_form(name)
    n = len(t)
    stand_in = np.concatenate([A.pins(), [A.corner((0.125 + 0.75 * (i % 32) / 32, 0.125 + 0.75 * (i // 32) / 36, 0.5), 0.015625) for i in range(n - 2)]])
    obj = tmp_path / "stand_in.obj"
    obj.write_text(A.obj_text(stand_in))
    base = A.base_scene("two")
    g = ra.Scene(write_scene(tmp_path, add_object(base, "mesh", None, **A.mesh_keys("two", obj)), "stand_in"), W, H)
    assert g.bvh(1)["n_tris"] == n
    sc = g.gpu()
    pos = torch.from_numpy(t).cuda()
    nrm = torch.from_numpy(np.tile(np.float32([0, 0, 1]), (n, 3))).contiguous().cuda()
    tb = torch.from_numpy(np.ascontiguousarray(g.bvh(1)["tris"][:, 24:30])).cuda()      # (the stand-in's tangents: the walk does not read them)
    torch.cuda.synchronize()
    lo = np.ascontiguousarray(lo, np.float32); hi = np.ascontiguousarray(hi, np.float32)
    for pen in pens:
        rc = g.rtx.rtx_scene_update_mesh(sc, 0, C.c_void_p(pos.data_ptr()), C.c_void_p(nrm.data_ptr()), C.c_void_p(tb.data_ptr()), lo.ctypes.data, hi.ctypes.data, pen, None)
        assert rc == 0, g.rtx.rtx_last_error()
        want = ra.bvh_build_host(t, lo, hi, pen)
        what = "%s penalty %d" % (name, pen)
        assert same_tree(g.device_mesh(0), want) is None, "%s: the device's %s differs from the host builder's" % (what, same_tree(g.device_mesh(0), want))
        want["tris"] = t
        flat = ra.mesh_flatten_probe(want)
        got = g.device_mesh_flat(0)
        for a, b, part in zip(got, flat, FLAT):
            assert a.shape == b.shape and np.array_equal(bits(a), bits(b)), "%s: the device's %s differ from the host flatten" % (what, part)
        copies = g.device_prune_copies(0)
        S = flat[0].shape[1]
        if len(flat[0]):
            assert copies.shape[0] >= 1 and copies.shape[1] == len(flat[0])
            assert np.array_equal(bits(copies[0][:, 0:S]), bits(flat[1])), "%s: copy 0's box records differ from the host flatten" % what
            assert np.array_equal(bits(copies[0][:, S:2 * S]), bits(flat[2])), "%s: copy 0's plane records differ from the host flatten" % what
        else:
            assert copies.shape[0] == 0 and copies.shape[1] == 0, "%s: prune blocks without a wide tree" % what
    g.close()


@pytest.mark.parametrize("name", ["two", "stack_129", "tiny"])
def test_updated_mesh_has_a_created_scenes_estimate_and_prune_copies(ra, tmp_path, name):
    """The two outputs of the flatten that (d) does not read -- the leaf boxes of the cost estimate and the slots' reference ranges, which
    the source copies of the prune blocks are built from: a scene created from the family's raw triangles written as an OBJ (the host
    flatten) against a stand-in scene whose mesh rtx_scene_update_mesh replaces with the created scene's placed triangles and root box (the
    device flatten), under one new view: cost_grid() and every copy of the prune blocks."""
    obj = tmp_path / "raw.obj"
    obj.write_text(A.obj_text(A.raw_form(name)[0]))
    base = A.base_scene("two")
    f = ra.Scene(write_scene(tmp_path, add_object(base, "mesh", None, **A.mesh_keys("two", obj)), "created"), W, H)
    tree = f.bvh(1)
    t = np.ascontiguousarray(tree["tris"][:, 0:9], np.float32)
    n = len(t)
    lo = np.ascontiguousarray(tree["bounds"][0, 0:3], np.float32); hi = np.ascontiguousarray(tree["bounds"][0, 3:6], np.float32)
    stand_in = np.array(A.pins() + [A.corner((0.125 + 0.75 * (i % 32) / 32, 0.125 + 0.75 * (i // 32) / 36, 0.5), 0.015625) for i in range(n - 2)])
    obj = tmp_path / "stand_in.obj"
    obj.write_text(A.obj_text(stand_in))
    g = ra.Scene(write_scene(tmp_path, add_object(base, "mesh", None, **A.mesh_keys("two", obj)), "stand_in"), W, H)
    assert g.bvh(1)["n_tris"] == n
    sc = g.gpu()
    pos = torch.from_numpy(t).cuda()
    nrm = torch.from_numpy(np.tile(np.float32([0, 0, 1]), (n, 3))).contiguous().cuda()
    tb = torch.from_numpy(np.ascontiguousarray(g.bvh(1)["tris"][:, 24:30])).cuda()
    torch.cuda.synchronize()
    rc = g.rtx.rtx_scene_update_mesh(sc, 0, C.c_void_p(pos.data_ptr()), C.c_void_p(nrm.data_ptr()), C.c_void_p(tb.data_ptr()), lo.ctypes.data, hi.ctypes.data, 1, None)
    assert rc == 0, g.rtx.rtx_last_error()
    assert same_tree(g.device_mesh(0), tree) is None
    cam, rot = g.camera_pose()
    there = (cam + np.float32([0.125, 0.0625, 0]), rot + np.float32([0, 5, 0]))
    for s in (g, f):
        s.set_camera(*there)
    got, want = g.device_prune_copies(0), f.device_prune_copies(0)
    assert got.shape == want.shape and got.shape[0] >= 2, "%s: %r copies of the prune blocks, the created scene's %r" % (name, got.shape, want.shape)
    for c in range(got.shape[0]):
        assert np.array_equal(bits(got[c]), bits(want[c])), "%s: copy %d of the prune blocks differs from the created scene's" % (name, c)
    for a, b, part in zip(g.cost_grid(), f.cost_grid(), ("references", "leaves")):
        assert a.shape == b.shape and np.array_equal(a, b), "%s: the cost estimate's %s differ from the created scene's" % (name, part)
    assert g.cost_grid()[1].sum() > 0
    g.close(); f.close()
