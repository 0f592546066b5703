#!/usr/bin/env python
"""Times moving a mesh of a live GPU scene (include/rtx_scene_edit.h) on the 250 000-triangle meshes of
scenes/cfg2_smooth_250k.scene and scenes/r6_knot_250k.scene; writes one JSON object to --out.  Medians of --reps warm runs (each after a
warm-up), host wall clock around synchronised calls:
  update_mesh       rtx_scene_update_mesh from device triangles (two placements uploaded once, alternated), until the device is idle;
                    split into the device build, read-back + flatten + upload, the view's preparation (rtx_scene_edit_times)
  move_object       Scene.move_object end to end, and its stages timed on their own (Scene.move_times): host placement by the loader's
                    code, upload of the triangles, rtx_scene_set_object, rtx_scene_update_mesh
  frames            a warm frame, the first frame after a move, the first frame after a new view (rtx_render_frame)
  scene_create      rtx_scene_create of the same description (flattenScene + upload + preparation), for comparison

    python tools/move_time.py [--size 1024] [--reps 7] [--out profiles/move_objects_time.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENES = [("cfg2_smooth_250k", "bumpy_250k.obj"), ("r6_knot_250k", "knot_250k.obj")]
PLACEMENTS = [dict(pos=(0.2, -0.1, -3.2), rot=(10, 25, 0), size=(1.8, 2.2, 2.0)), dict(pos=(0, 0, -3), rot=(0, 0, 0), size=(2, 2, 2))]


def med(xs):
    return float(np.median(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "move_objects_time.json"))
    a = ap.parse_args()
    import torch
    import rendering_amd as RA
    from rendering_amd import assets
    os.chdir(ROOT)
    assets.ensure()
    rtx, host = RA.load()
    sync = torch.cuda.synchronize
    w = h = a.size
    fb = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
    mask = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
    result = dict(device=torch.cuda.get_device_name(0), size=[w, h], reps=a.reps, scenes={})

    def frame_ms(g):
        sync(); t0 = time.perf_counter(); g.render_frame(fb, mask); sync()
        return (time.perf_counter() - t0) * 1e3

    for name, obj in SCENES:
        assets.ensure([obj])
        g = RA.Scene("scenes/%s.scene" % name, w, h)
        for _ in range(3):
            g.render_frame(fb, mask)
        sync()
        mesh_obj = 1
        n_tris = g.bvh(mesh_obj)["n_tris"]
        r = dict(n_tris=int(n_tris))
        # (a) Scene.move_object end to end, alternating two placements, with its stages
        e2e, stages = [], []
        for k in range(a.reps + 1):
            sync(); t0 = time.perf_counter()
            g.move_object(mesh_obj, **PLACEMENTS[k % 2]); sync()
            t = (time.perf_counter() - t0) * 1e3
            if k:
                e2e.append(t); stages.append(g.move_times())
        r["move_object_ms"] = med(e2e)
        r["move_object_stages_ms"] = {k: med([s[k] for s in stages]) for k in ("place", "upload", "set_object", "update_mesh")}
        # (b) rtx_scene_update_mesh alone, from device triangles of the two placements
        dev = []
        for k in range(2):
            g.move_object(mesh_obj, **PLACEMENTS[k])
            t = g.bvh(mesh_obj)["tris"]
            dev.append((torch.from_numpy(np.ascontiguousarray(t[:, 0:9])).cuda(), torch.from_numpy(np.ascontiguousarray(t[:, 9:18])).cuda(),
                        torch.from_numpy(np.ascontiguousarray(t[:, 24:30])).cuda(), g.bvh(mesh_obj)["bounds"][0].copy()))
        sync()
        pen = 1      # (options::acPenalty of both scenes)
        times, split = [], []
        for k in range(a.reps + 1):
            pos, nrm, tb, root = dev[k % 2]
            lo = np.ascontiguousarray(root[0:3], np.float32); hi = np.ascontiguousarray(root[3:6], np.float32)
            sync(); t0 = time.perf_counter()
            rc = rtx.rtx_scene_update_mesh(g.gpu(), 0, C.c_void_p(pos.data_ptr()), C.c_void_p(nrm.data_ptr()), C.c_void_p(tb.data_ptr()),
                                           lo.ctypes.data, hi.ctypes.data, pen, None)
            sync()
            t = (time.perf_counter() - t0) * 1e3
            assert rc == 0, rtx.rtx_last_error()
            if k:
                times.append(t); split.append(g.edit_times())
        r["update_mesh_ms"] = med(times)
        r["update_mesh_split_ms"] = {k: med([s[k] for s in split]) for k in ("build", "flatten", "prepare")}
        r["update_mesh_split_ms"]["preparation_on_device"] = med([t - s["total"] for t, s in zip(times, split)])
        # (c) frames: warm, first after a move, first after a new view
        g.move_object(mesh_obj, **PLACEMENTS[1])
        for _ in range(3):
            g.render_frame(fb, mask)
        warm, after_move, after_view = [], [], []
        pos0, rot0 = g.camera_pose()
        for k in range(a.reps):
            warm.append(frame_ms(g))
            g.move_object(mesh_obj, **PLACEMENTS[k % 2]); sync()
            after_move.append(frame_ms(g))
            g.set_camera(pos0 + np.float32([0.01 * (k % 2), 0, 0]), rot0)
            after_view.append(frame_ms(g))
        r["frame_warm_ms"] = med(warm); r["frame_after_move_ms"] = med(after_move); r["frame_after_new_view_ms"] = med(after_view)
        # (d) rtx_scene_create of the same description
        creates = []
        for k in range(a.reps + 1):
            sync(); t0 = time.perf_counter()
            f = host.rah_flatten(g.h)
            out = C.c_void_p()
            rc = rtx.rtx_scene_create(C.c_void_p(host.rah_flat_desc(f)), 0, C.byref(out))
            sync()
            t = (time.perf_counter() - t0) * 1e3
            host.rah_flat_free(f)
            assert rc == 0, rtx.rtx_last_error()
            rtx.rtx_scene_destroy(out)
            if k:
                creates.append(t)
        r["scene_create_ms"] = med(creates)
        r["create_over_update"] = r["scene_create_ms"] / r["update_mesh_ms"]
        result["scenes"][name] = r
        print(json.dumps({name: r}), flush=True)
        g.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
