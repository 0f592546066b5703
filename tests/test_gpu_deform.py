"""Meshes of a live GPU scene deformed between frames (Scene.set_vertices -> rtx_scene_deform_mesh, include/rtx_deform.h): the device
kernels give the bytes of the shared formulas on the CPU; every deformed state renders, bit for bit, what a fresh scene of the rewritten OBJ
file renders -- and the oracle's frame of it -- in both frame modes; the structures the device built equal the fresh scene's; inputs
produced on another stream are waited for; the other entry points and the other edits agree with fresh scenes; refusals leave the scene
as it was; nothing leaks."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests.test_gpu_move_objects import check_structures, frame
from tests.util_deform import bits, bulge, deformed_scene, mesh_name, probe_cases, rewrite_obj, scale, set_mesh_name, twist
from tests.util_move import edit_scene, same_structure
from tests.util_objects import BUMPY, add_object, remove_object
from tests.util_rays import probe_rays

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same_frames(a, b):
    return np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1])


def test_the_device_kernels_give_the_cpu_formulas_bytes(ra, tmp_path):
    seen_nan = seen_unplaced = seen_ragged = False
    for label, topo, stored, V, N, pose in probe_cases(ra, tmp_path):
        cpu = ra.place_probe(topo, stored, V, N, pose, device=-1)
        dev = ra.place_probe(topo, stored, V, N, pose, device=0)
        for k in ("pos", "nrm", "tb", "root_lo", "root_hi", "obj_hi"):
            assert np.array_equal(bits(cpu[k]), bits(dev[k])), "%s: %s differs between the device and the CPU" % (label, k)
        # (the sign of a zero minimum is the one thing a parallel reduction does not reproduce; it reaches no triangle)
        assert np.array_equal(cpu["obj_lo"], dev["obj_lo"]), "%s: obj_lo" % label
        assert cpu["bad_input"] == dev["bad_input"] and cpu["bad_placed"] == dev["bad_placed"], label
        for k in ("pos", "nrm", "tb"):
            m = np.isnan(dev[k])
            assert (bits(dev[k])[m] == 0xFFC00000).all(), "%s: a NaN of %s is not stored as 0xFFC00000" % (label, k)
            seen_nan |= bool(m.any())
        seen_unplaced |= topo["placed_pos"] < V.shape[0]
        seen_ragged |= topo["corner_pos"].shape[0] % 64 != 0 and topo["corner_pos"].shape[0] > 256
    assert seen_nan and seen_unplaced and seen_ragged


# scene -> (width, height, [(object, deformations in a row)])
SEQUENCES = {
    "mixed_materials": (200, 152, (0, 1, 2)),
    "cfg4_textured_256": (160, 160, (0,)),
    "cfg2_smooth_25k": (224, 160, (1,)),
}


def deformations(P0):
    flat = bool((P0[:, 1] == 0).all())
    a = scale(P0, (1.25, 1.0 if flat else 0.75, 1.1))
    return [a, bulge(twist(a, 0.6), 0.12, 3.0)]


@pytest.mark.parametrize("name", sorted(SEQUENCES))
def test_deformations_equal_fresh_scenes_and_the_oracle(ra, oracle, tmp_path, name):
    w, h, objs = SEQUENCES[name]
    text0 = open(os.path.join(ROOT, "scenes", name + ".scene")).read()
    g = ra.Scene("scenes/%s.scene" % name, w, h)
    g.gpu()
    g.set_knob("verify_lists", 1)
    start = [frame(g, w, h, m) for m in (0, 1)]
    first = {idx: g.mesh_vertices(idx)[0] for idx in objs}
    text = text0
    for idx in objs:
        for step, V in enumerate(deformations(first[idx])):
            g.set_vertices(idx, torch.from_numpy(V).cuda())
            tag = "%s_%d_%d" % (name, idx, step)
            f, p = deformed_scene(ra, tmp_path, text, idx, V, None, tag, w, h)
            ff, fm = frame(f, w, h, 0)
            o = oracle.OracleScene(p, w, h)
            ref = o.ssaa(o.pass1())
            for mode in (0, 1):
                got, gm = frame(g, w, h, mode)
                assert np.array_equal(bits(got), bits(ff)) and np.array_equal(gm, fm), "%s mode %d: differs from a fresh scene" % (tag, mode)
                d = (bits(got) != bits(ref)).any(-1)
                d[0, :] = False; d[:, 0] = False          # (the reference's uninitialised mask border)
                assert not d.any(), "%s mode %d: %d pixels differ from the oracle" % (tag, mode, int(d.sum()))
            check_structures(ra, g, f)
            mi = [i for i in range(g.n_objects) if g.bvh(i) is not None].index(idx)
            assert np.array_equal(bits(g.device_prune_copies(mi)), bits(f.device_prune_copies(mi))), "%s: the prune copies differ" % tag
            f.close()
        # (the next object is deformed in a scene whose earlier ones keep their last shape: the text reads their rewritten files)
        obj = rewrite_obj(os.path.join(ROOT, mesh_name(text0, idx)), tmp_path / ("kept_%s_%d.obj" % (name, idx)), deformations(first[idx])[-1])
        text = set_mesh_name(text, idx, obj)
    # every mesh back to its first vertices: the first frames again
    for idx in objs:
        g.set_vertices(idx, first[idx])
    for m, s in zip((0, 1), start):
        assert same_frames(frame(g, w, h, m), s), "mode %d: the first frame does not come back" % m
    g.close()


def test_inputs_produced_on_another_stream_are_waited_for(ra, tmp_path):
    name, w, h, idx = "cfg2_smooth_25k", 224, 160, 1
    text = open(os.path.join(ROOT, "scenes", name + ".scene")).read()
    g = ra.Scene("scenes/%s.scene" % name, w, h)
    frame(g, w, h, 0)
    P0, N0 = g.mesh_vertices(idx)
    st = torch.cuda.Stream()
    base = torch.from_numpy(P0).cuda()
    nbase = torch.from_numpy(N0).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        # a long chain of small launches in front of the final values: a call that did not wait would read an earlier state
        V = base.clone()
        for _ in range(200):
            V = V * 1.0009765625
        V = V * torch.tensor([1.0, 0.75, 1.0], device="cuda")
        N = nbase * 2.0
        g.set_vertices(idx, V, N, stream=st)
    Vh, Nh = V.cpu().numpy(), N.cpu().numpy()
    got = frame(g, w, h, 0)
    f, _ = deformed_scene(ra, tmp_path, text, idx, Vh, Nh, "stream", w, h)
    want = frame(f, w, h, 0)
    assert same_frames(got, want), "the frame after a deformation from a stream differs from a fresh scene's"
    assert same_structure(g.bvh(idx), f.bvh(idx)) is None
    # the same from numpy
    g2 = ra.Scene("scenes/%s.scene" % name, w, h)
    frame(g2, w, h, 0)
    g2.set_vertices(idx, Vh, Nh)
    assert same_frames(frame(g2, w, h, 0), want)
    # ... and from CPU tensors
    g2.set_vertices(idx, torch.from_numpy(P0))
    g2.set_vertices(idx, torch.from_numpy(Vh), torch.from_numpy(Nh))
    assert same_frames(frame(g2, w, h, 0), want)
    t = g.deform_times()
    assert t["total"] > 0 and t["rebuild"] > 0 and t["kernels"] >= 0
    f.close(); g2.close(); g.close()


def test_other_entry_points_after_a_deformation(ra, tmp_path):
    name, w, h, idx = "mixed_materials", 160, 120, 1
    text = open(os.path.join(ROOT, "scenes", name + ".scene")).read()
    g = ra.Scene("scenes/%s.scene" % name, w, h)
    frame(g, w, h)
    rays = torch.from_numpy(probe_rays(4096)).cuda()
    g.trace_rays(rays); g.occluded(rays)
    P0, _ = g.mesh_vertices(idx)
    V = bulge(twist(P0, 0.7), 0.1, 2.0)
    g.set_vertices(idx, torch.from_numpy(V).cuda())
    f, _ = deformed_scene(ra, tmp_path, text, idx, V, None, "entry", w, h)
    cpu = lambda t: t.cpu().numpy()
    same = lambda a, b: np.array_equal(bits(cpu(a)), bits(cpu(b))) if a.dtype == torch.float32 else np.array_equal(cpu(a), cpu(b))
    hg, cg = g.trace_rays(rays)
    hf, cf = f.trace_rays(rays)
    assert same(hg, hf) and same(cg, cf), "trace_rays differs from a fresh scene's"
    assert (cpu(hg)[:, 0] != 0).any()
    assert same(g.occluded(rays), f.occluded(rays)), "occluded differs from a fresh scene's"
    a, b = g.surface_rays(rays, hits=True, position=True, normal=True, albedo=True, specular=True), f.surface_rays(rays, hits=True, position=True, normal=True, albedo=True, specular=True)
    for k in a:
        assert same(a[k], b[k]), "surface_rays: %s differs from a fresh scene's" % k
    a, b = g.light_rays(rays, hits=True, per_light=True), f.light_rays(rays, hits=True, per_light=True)
    for k in a:
        assert same(a[k], b[k]), "light_rays: %s differs from a fresh scene's" % k
    aov = []
    for s in (g, f):
        bufs = dict(depth=torch.zeros((h, w), dtype=torch.float32, device="cuda"), object_id=torch.zeros((h, w), dtype=torch.int32, device="cuda"),
                    triangle_id=torch.zeros((h, w), dtype=torch.int32, device="cuda"), uv=torch.zeros((h, w, 2), dtype=torch.float32, device="cuda"),
                    normal=torch.zeros((h, w, 3), dtype=torch.float32, device="cuda"), albedo=torch.zeros((h, w, 3), dtype=torch.float32, device="cuda"))
        s.render_aov(**bufs)
        torch.cuda.synchronize()
        aov.append(bufs)
    for k in aov[0]:
        assert same(aov[0][k], aov[1][k]), "render_aov: %s differs from a fresh scene's" % k
    f.close(); g.close()


def test_deformations_between_other_edits(ra, tmp_path):
    name, w, h = "mixed_materials", 128, 96
    text = open(os.path.join(ROOT, "scenes", name + ".scene")).read()
    g = ra.Scene("scenes/%s.scene" % name, w, h)
    frame(g, w, h)

    def check(text, idx, V, tag):
        f, _ = deformed_scene(ra, tmp_path, text, idx, V, None, tag, w, h)
        for mode in (0, 1):
            assert same_frames(frame(g, w, h, mode), frame(f, w, h, mode)), "%s mode %d: differs from a fresh scene" % (tag, mode)
        check_structures(ra, g, f)
        f.close()

    # deform, move, deform
    P2, _ = g.mesh_vertices(2)
    V = scale(P2, (1.2, 0.8, 1.0))
    g.set_vertices(2, torch.from_numpy(V).cuda())
    keys = dict(pos=(1.1, 0.3, -4.2), rot=(30, 10, -15))
    g.move_object(2, **keys)
    text = edit_scene(text, 2, **keys)
    check(text, 2, V, "moved")
    V = twist(V, 0.9)
    g.set_vertices(2, torch.from_numpy(V).cuda())
    check(text, 2, V, "moved_deformed")
    # a light edited between deformations
    g.set_light(0, position=(1.0, 2.5, -1.0))
    lines = text.split("\n")
    at = next(i for i, l in enumerate(lines) if l.startswith("position=2,3,0"))
    lines[at] = "position=1,2.5,-1"
    text = "\n".join(lines)
    V = bulge(V, 0.1, 2.0)
    g.set_vertices(2, torch.from_numpy(V).cuda())
    check(text, 2, V, "light")
    # the quad removed: the torus moves up to object 1 / mesh 1, and its topology follows it
    obj = rewrite_obj(os.path.join(ROOT, "scenes", "assets", "torus_1536.obj"), tmp_path / "torus_kept.obj", V)
    text = remove_object(set_mesh_name(text, 2, obj), 0)
    g.remove_object(0)
    V = scale(V, (0.9, 1.1, 1.05))
    g.set_vertices(1, torch.from_numpy(V).cuda())
    check(text, 1, V, "moved_up")
    text = set_mesh_name(text, 1, rewrite_obj(os.path.join(ROOT, "scenes", "assets", "torus_1536.obj"), tmp_path / "torus_kept_2.obj", V))
    # a mesh added to the live scene, then deformed
    at = g.add_object("mesh", None, **BUMPY)
    text = add_object(text, "mesh", None, **BUMPY)
    PB, _ = g.mesh_vertices(at)
    VB = bulge(PB, 0.08, 4.0)
    g.set_vertices(at, torch.from_numpy(VB).cuda())
    check(text, at, VB, "added")
    g.close()


ERR_ARG = -1      # RTX_ERR_ARG


def test_refusals_leave_the_live_scene_as_it_was(ra):
    name, w, h = "mixed_materials", 96, 72
    g = ra.Scene("scenes/%s.scene" % name, w, h)
    want = frame(g, w, h, 0)
    rtx, sc = g.rtx, g.gpu()
    P1, N1 = g.mesh_vertices(1)
    dev = torch.from_numpy(P1).cuda()
    pose = ra.MeshPose()
    pose.pos[:] = (0, 0, -4); pose.size[:] = (1, 1, 1); pose.rot_matrix[:] = [float(x) for x in np.eye(4).reshape(-1)]
    pose.bias = 1e-4; pose.ac_penalty = 1
    p = C.c_void_p(dev.data_ptr())
    # a mesh without topology
    assert rtx.rtx_scene_deform_mesh(sc, 1, p, P1.shape[0], None, 0, C.byref(pose), None, None, None) == ERR_ARG
    assert b"topology" in rtx.rtx_last_error()
    # the same vertices again: the same scene, and the topology is on the device from here on
    g.set_vertices(1, dev)
    assert same_frames(frame(g, w, h, 0), want)
    for bad in (np.nan, np.inf):
        V = P1.copy(); V[11, 2] = bad
        # (the library's own check, on the device: the wrapper's host copy is not in the way of a direct call)
        vd = torch.from_numpy(V).cuda()
        assert rtx.rtx_scene_deform_mesh(sc, 1, C.c_void_p(vd.data_ptr()), P1.shape[0], None, 0, C.byref(pose), None, None, None) == ERR_ARG
        assert b"finite" in rtx.rtx_last_error()
        nd = N1.copy(); nd[5, 1] = bad
        nd = torch.from_numpy(nd).cuda()
        assert rtx.rtx_scene_deform_mesh(sc, 1, p, P1.shape[0], C.c_void_p(nd.data_ptr()), N1.shape[0], C.byref(pose), None, None, None) == ERR_ARG
        with pytest.raises(ra.RtxError):
            g.set_vertices(1, torch.from_numpy(V).cuda())
        N = N1.copy(); N[0, 0] = bad
        with pytest.raises(ra.RtxError):
            g.set_vertices(1, dev, torch.from_numpy(N).cuda())
    P0, _ = g.mesh_vertices(0)
    V = P0.copy(); V[:, 1] = 1      # a flat axis away from zero
    with pytest.raises(ra.RtxError):
        g.set_vertices(0, torch.from_numpy(V).cuda())
    with pytest.raises(ValueError):
        g.set_vertices(1, dev[:-1])
    with pytest.raises(ValueError):
        g.set_vertices(1, dev.double())
    with pytest.raises(ValueError):
        g.set_vertices(3, dev)
    # wrong counts, a NULL pose, a bad mesh index, NULL vertices
    assert rtx.rtx_scene_deform_mesh(sc, 1, p, P1.shape[0] - 1, None, 0, C.byref(pose), None, None, None) == ERR_ARG
    assert rtx.rtx_scene_deform_mesh(sc, 1, p, P1.shape[0], p, N1.shape[0] + 1, C.byref(pose), None, None, None) == ERR_ARG
    assert rtx.rtx_scene_deform_mesh(sc, 1, p, P1.shape[0], None, 0, None, None, None, None) == ERR_ARG
    assert rtx.rtx_scene_deform_mesh(sc, 9, p, P1.shape[0], None, 0, C.byref(pose), None, None, None) == ERR_ARG
    assert rtx.rtx_scene_deform_mesh(sc, 1, None, P1.shape[0], None, 0, C.byref(pose), None, None, None) == ERR_ARG
    topo = ra.MeshTopology()
    topo.n_tris = 7
    assert rtx.rtx_scene_set_mesh_topology(sc, 1, C.byref(topo)) == ERR_ARG
    assert same_frames(frame(g, w, h, 0), want), "a refused call changed the frame"
    for i in (0, 1):
        assert np.array_equal(bits(g.mesh_vertices(i)[0]), bits((P0, P1)[i]))
    g.close()


def test_deformations_leak_nothing_and_count_as_a_fresh_scene(ra, tmp_path):
    name, w, h, idx = "mixed_materials", 96, 72, 2
    live0 = ra.live_device_memory()
    f = ra.Scene("scenes/%s.scene" % name, w, h)
    frame(f, w, h, 0)
    fresh_bytes = f.scene_bytes()
    f.close()
    assert ra.live_device_memory() == live0
    g = ra.Scene("scenes/%s.scene" % name, w, h)
    frame(g, w, h, 0)
    P0, N0 = g.mesh_vertices(idx)
    text = open(os.path.join(ROOT, "scenes", name + ".scene")).read()
    # three shapes in turn (another shape is another tree, of another size): the first and the tenth deformation are the first load's shape
    shapes = [P0, scale(P0, (1.1, 0.9, 1.0)), bulge(P0, 0.1, 3.0)]
    # (the scene's scratch buffers grow to the largest tree they have seen and stay: every shape once before anything is counted)
    for V in shapes[::-1]:
        g.set_vertices(idx, torch.from_numpy(V).cuda())
    live = []
    for k in range(10):
        V = shapes[k % 3]
        g.set_vertices(idx, torch.from_numpy(V).cuda(), torch.from_numpy(N0).cuda() if k % 3 == 0 else None)
        frame(g, w, h, 0)
        live.append(ra.live_device_memory())
        if k % 3 == 0:
            want = fresh_bytes
        elif k < 3:
            f, _ = deformed_scene(ra, tmp_path, text, idx, V, None, "bytes_%d" % k, w, h)
            frame(f, w, h, 0)
            want = f.scene_bytes()
            f.close()
        else:
            continue
        assert g.scene_bytes() == want, "scene_bytes after deformation %d: %d, a fresh scene's %d" % (k, g.scene_bytes(), want)
    assert live[9] == live[0], "live device memory after the tenth deformation is not what it was after the first: %r" % (live,)
    assert live[4] == live[1] and live[5] == live[2], "live device memory grows with deformations: %r" % (live,)
    g.close()
    assert ra.live_device_memory() == live0, "device memory is left behind after close()"
