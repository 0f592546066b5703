#!/usr/bin/env python
"""Times deforming a mesh of a live GPU scene (include/rtx_deform.h) on the 250 000-triangle meshes of
scenes/cfg2_smooth_250k.scene and scenes/r6_knot_250k.scene; writes one JSON object to --out, stamped with tools/srchash.py.  The method of
tools/move_time.py: host wall clock around synchronised calls, medians of --reps warm runs (each after a warm-up); --rounds rounds, of which
the middle and the range [min, max] are kept:
  set_vertices      Scene.set_vertices end to end from a device tensor (two shapes alternated), with its stages (Scene.deform_times): the
                    placement and assembly kernels with their read-backs, the rebuild (rtx_scene_update_mesh), the host's copy of the vertices
  move_object       Scene.move_object of the same mesh end to end, with its stages (Scene.move_times)
  update_mesh       rtx_scene_update_mesh alone, from device triangles
  frames            a warm frame, the first frame after a deformation, the first frame after a new view

    python tools/deform_time.py [--size 1024] [--reps 7] [--rounds 3] [--out profiles/deform_time.json]
    python tools/deform_time.py --only-move --package DIR      (move_object alone with the package of another build, e.g. the parent commit's)
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCENES = [("cfg2_smooth_250k", "bumpy_250k.obj"), ("r6_knot_250k", "knot_250k.obj")]
PLACEMENTS = [dict(pos=(0.2, -0.1, -3.2), rot=(10, 25, 0), size=(1.8, 2.2, 2.0)), dict(pos=(0, 0, -3), rot=(0, 0, 0), size=(2, 2, 2))]


def med(xs):
    return float(np.median(xs))


def spread(rounds):
    """{key: [middle, min, max]} of a list of flat dicts"""
    return {k: [med([r[k] for r in rounds]), float(min(r[k] for r in rounds)), float(max(r[k] for r in rounds))] for k in rounds[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only-move", action="store_true")
    ap.add_argument("--package", default=ROOT, help="the directory that holds the rendering_amd package to time")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deform_time.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package))
    sys.path.insert(1, ROOT)
    import torch
    import rendering_amd as RA
    from rendering_amd import assets
    from tools.srchash import source_hash
    os.chdir(ROOT)
    rtx, host = RA.load()
    sync = torch.cuda.synchronize
    w = h = a.size
    fb = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
    mask = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
    result = dict(device=torch.cuda.get_device_name(0), size=[w, h], reps=a.reps, rounds=a.rounds, package=os.path.relpath(os.path.abspath(a.package), ROOT),
                  source_hash=source_hash(), columns=["middle", "min", "max"], scenes={})

    def frame_ms(g):
        sync(); t0 = time.perf_counter(); g.render_frame(fb, mask); sync()
        return (time.perf_counter() - t0) * 1e3

    for name, obj in SCENES:
        if not os.path.exists(os.path.join(ROOT, "scenes", "assets", obj)):      # (another build's package would write beside itself)
            assets.ensure([obj])
        g = RA.Scene("scenes/%s.scene" % name, w, h, cwd=ROOT)
        for _ in range(3):
            g.render_frame(fb, mask)
        sync()
        mesh_obj = 1
        rounds = []
        n_tris = int(g.bvh(mesh_obj)["n_tris"])
        if not a.only_move:
            P0, _ = g.mesh_vertices(mesh_obj)
            base = torch.from_numpy(P0).cuda()
            # (two shapes of about the same tree: how long the rebuild takes depends on the shape, and move_object is timed on the file's own)
            shapes = [base * torch.tensor([1.0, 0.9, 1.05], device="cuda"), base.clone()]
            # the triangles of two placements on the device, for rtx_scene_update_mesh alone
            dev = []
            for k in range(2):
                g.move_object(mesh_obj, **PLACEMENTS[k])
                b = g.bvh(mesh_obj)
                t = b["tris"]
                dev.append((torch.from_numpy(np.ascontiguousarray(t[:, 0:9])).cuda(), torch.from_numpy(np.ascontiguousarray(t[:, 9:18])).cuda(),
                            torch.from_numpy(np.ascontiguousarray(t[:, 24:30])).cuda(), b["bounds"][0].copy()))
            sync()
        for _ in range(a.rounds):
            r = {}
            # (b) Scene.move_object end to end, alternating two placements, with its stages
            e2e, stages = [], []
            for k in range(a.reps + 1):
                sync(); t0 = time.perf_counter()
                g.move_object(mesh_obj, **PLACEMENTS[k % 2]); sync()
                t = (time.perf_counter() - t0) * 1e3
                if k:
                    e2e.append(t); stages.append(g.move_times())
            r["move_object_ms"] = med(e2e)
            for s in ("place", "upload", "set_object", "update_mesh"):
                r["move_object_%s_ms" % s] = med([x[s] for x in stages])
            if a.only_move:
                rounds.append(r)
                continue
            # (a) Scene.set_vertices end to end from a device tensor, two shapes alternated, with its stages
            e2e, stages = [], []
            for k in range(a.reps + 1):
                sync(); t0 = time.perf_counter()
                g.set_vertices(mesh_obj, shapes[k % 2]); sync()
                t = (time.perf_counter() - t0) * 1e3
                if k:
                    e2e.append(t); stages.append(g.deform_times())
            r["set_vertices_ms"] = med(e2e)
            for s in ("kernels", "rebuild", "mirror"):
                r["set_vertices_%s_ms" % s] = med([x[s] for x in stages])
            for j in (0, 1):      # (run k deforms to shape k % 2; e2e[k - 1] is its time)
                r["set_vertices_shape%d_ms" % j] = med([t for k, t in enumerate(e2e, 1) if k % 2 == j])
            # (c) rtx_scene_update_mesh alone
            times, split = [], []
            for k in range(a.reps + 1):
                pos, nrm, tb, root = dev[k % 2]
                lo = np.ascontiguousarray(root[0:3], np.float32); hi = np.ascontiguousarray(root[3:6], np.float32)
                sync(); t0 = time.perf_counter()
                rc = rtx.rtx_scene_update_mesh(g.gpu(), 0, C.c_void_p(pos.data_ptr()), C.c_void_p(nrm.data_ptr()), C.c_void_p(tb.data_ptr()),
                                               lo.ctypes.data, hi.ctypes.data, 1, None)
                sync()
                t = (time.perf_counter() - t0) * 1e3
                assert rc == 0, rtx.rtx_last_error()
                if k:
                    times.append(t); split.append(g.edit_times())
            r["update_mesh_ms"] = med(times)
            r["update_mesh_call_ms"] = med([s["total"] for s in split])
            r["set_vertices_minus_update_mesh_ms"] = r["set_vertices_ms"] - r["update_mesh_ms"]
            # the device holds the triangles of a placement now and the host those of a shape: one deformation brings them together
            g.set_vertices(mesh_obj, shapes[1])
            # frames: warm, the first after a deformation, the first after a new view
            for _ in range(3):
                g.render_frame(fb, mask)
            warm, after_deform, after_view = [], [], []
            pos0, rot0 = g.camera_pose()
            for k in range(a.reps):
                warm.append(frame_ms(g))
                g.set_vertices(mesh_obj, shapes[k % 2]); sync()
                after_deform.append(frame_ms(g))
                g.set_camera(pos0 + np.float32([0.01 * (k % 2), 0, 0]), rot0)
                after_view.append(frame_ms(g))
            r["frame_warm_ms"] = med(warm); r["frame_after_deformation_ms"] = med(after_deform); r["frame_after_new_view_ms"] = med(after_view)
            g.set_vertices(mesh_obj, shapes[1])      # (the next round moves the file's own shape again)
            rounds.append(r)
        out = spread(rounds)
        out["n_tris"] = n_tris
        result["scenes"][name] = out
        print(json.dumps({name: out}), flush=True)
        g.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
