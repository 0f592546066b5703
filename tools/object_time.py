#!/usr/bin/env python
"""Times adding and removing objects of a live GPU scene (rtx_scene_set_objects, include/rtx_scene_edit.h) on
scenes/cfg2_smooth_250k.scene; writes one JSON object to --out.  Medians of --reps warm runs (each after a warm-up), host wall clock
around synchronised calls, all in one process.  Per edit -- a sphere appended / removed again, bumpy_4k added in the device form / removed
again, a second 250 000-triangle mesh added in the device form (and removed again, to repeat it):
  set_objects       rtx_scene_set_objects, until the device is idle (the new mesh's triangles are in device memory before the clock starts)
  scene             Scene.add_object / remove_object end to end (the OBJ read and placed, the triangles uploaded, then the call)
  scene_create      rtx_scene_create of the resulting description, for comparison
  first_frame       the first frame after the edit (rtx_render_frame), beside a warm frame and the first frame of a new view
Every one of these edits keeps the 250 000-triangle mesh, so each must cost less than rtx_scene_create of the description it produces
(an add: the description with the object; a remove: the scene as loaded; exit status 1 otherwise): if it does not, something of a kept
mesh is uploaded or built again.

    python tools/object_time.py [--size 4096] [--reps 7] [--out profiles/object_edit_time.json]
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

SCENE, OBJ = "cfg2_smooth_250k", "bumpy_250k.obj"
EDITS = [
    ("sphere", "sphere", dict(pos=(1.4, -0.6, -2.4), radius=0.5, color=(0.9, 0.6, 0.2))),
    ("bumpy_4k", "mesh", dict(pos=(1.5, -0.4, -2.6), size=(1.0, 1.0, 1.0), rot=(10, 25, 0), color=(0.9, 0.8, 0.6), name="scenes/assets/bumpy_4k.obj")),
    ("second_250k", "mesh", dict(pos=(-1.6, -0.3, -3.4), size=(1.4, 1.4, 1.4), rot=(0, 40, 0), color=(0.7, 0.8, 1.0), name="scenes/assets/" + OBJ)),
]


def med(xs):
    return float(np.median(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "object_edit_time.json"))
    a = ap.parse_args()
    import torch
    import rendering_amd as RA
    from rendering_amd import assets
    os.chdir(ROOT)
    assets.ensure([OBJ, "bumpy_4k.obj"])
    rtx, host = RA.load()
    sync = torch.cuda.synchronize
    w = h = a.size
    fb = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
    mask = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
    r = dict(device=torch.cuda.get_device_name(0), scene=SCENE, size=[w, h], reps=a.reps)

    def frame_ms(g):
        sync(); t0 = time.perf_counter(); g.render_frame(fb, mask); sync()
        return (time.perf_counter() - t0) * 1e3

    def timed(f):
        sync(); t0 = time.perf_counter(); rc = f(); sync()
        return (time.perf_counter() - t0) * 1e3, rc

    g = RA.Scene("scenes/%s.scene" % SCENE, w, h)
    for _ in range(3):
        g.render_frame(fb, mask)
    sync()
    n0 = g.n_objects
    first = host.rah_flatten(g.h)
    first_desc = C.cast(host.rah_flat_desc(first), C.POINTER(RA.RtxSceneDesc)).contents
    # rtx_scene_create of the scene as loaded: the description every removal below produces
    creates = []
    for k in range(a.reps + 1):
        out = C.c_void_p()
        t, rc = timed(lambda: rtx.rtx_scene_create(C.byref(first_desc), 0, C.byref(out)))
        assert rc == 0, rtx.rtx_last_error()
        rtx.rtx_scene_destroy(out)
        if k:
            creates.append(t)
    r["scene_create_ms"] = med(creates)
    ok = True
    for tag, kind, keys in EDITS:
        # the edited description from a host scene of its own: the object records, the new mesh's uv and maps, its placed triangles
        e = RA.Scene("scenes/%s.scene" % SCENE, w, h)
        assert e.add_object(kind, **keys) == n0
        flat = host.rah_flatten(e.h)
        d = C.cast(host.rah_flat_desc(flat), C.POINTER(RA.RtxSceneDesc)).contents
        srcs = (RA.RtxMeshSource * d.n_meshes)()
        srcs[0].keep = 0
        keep = []
        if kind == "mesh":
            m = d.meshes[1]
            up = lambda ptr, per: torch.from_numpy(np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_float)), (m.n_tris * per,)).copy()).cuda()
            keep = [up(m.tri_pos, 9), up(m.tri_nrm, 9), up(m.tri_tb, 6)]
            build = RA.RtxMeshBuild()
            build.tri_pos_dev, build.tri_nrm_dev, build.tri_tb_dev = (t.data_ptr() for t in keep)
            root = e.bvh(n0)["bounds"][0]
            build.root_lo[:] = root[0:3].tolist(); build.root_hi[:] = root[3:6].tolist()
            build.ac_penalty = 1
            srcs[1].keep = -1; srcs[1].mesh = C.pointer(m); srcs[1].build = C.pointer(build)
            r[tag + "_triangles"] = int(m.n_tris)
        back = (RA.RtxMeshSource * 1)()
        back[0].keep = 0

        def add():
            return rtx.rtx_scene_set_objects(g.gpu(), d.n_objects, d.objects, d.n_meshes, srcs, None)

        def remove():
            return rtx.rtx_scene_set_objects(g.gpu(), first_desc.n_objects, first_desc.objects, 1, back, None)

        # (a) rtx_scene_set_objects: the object added, removed again; the first frame after each
        adds, removes, frames_add, frames_remove = [], [], [], []
        for k in range(a.reps + 1):
            t, rc = timed(add)
            assert rc == 0, rtx.rtx_last_error()
            f1 = frame_ms(g)
            frame_ms(g); frame_ms(g)
            t2, rc = timed(remove)
            assert rc == 0, rtx.rtx_last_error()
            f2 = frame_ms(g)
            frame_ms(g); frame_ms(g)
            if k:
                adds.append(t); removes.append(t2); frames_add.append(f1); frames_remove.append(f2)
        r[tag + "_set_objects_add_ms"] = med(adds); r[tag + "_set_objects_remove_ms"] = med(removes)
        r[tag + "_first_frame_after_add_ms"] = med(frames_add); r[tag + "_first_frame_after_remove_ms"] = med(frames_remove)
        # (b) Scene.add_object / remove_object end to end
        adds, removes = [], []
        for k in range(a.reps + 1):
            t, _ = timed(lambda: g.add_object(kind, **keys))
            t2, _ = timed(lambda: g.remove_object(n0))
            if k:
                adds.append(t); removes.append(t2)
        r[tag + "_add_object_ms"] = med(adds); r[tag + "_remove_object_ms"] = med(removes)
        # (c) rtx_scene_create of the description with the object
        creates = []
        for k in range(a.reps + 1):
            out = C.c_void_p()
            t, rc = timed(lambda: rtx.rtx_scene_create(C.byref(d), 0, C.byref(out)))
            assert rc == 0, rtx.rtx_last_error()
            rtx.rtx_scene_destroy(out)
            if k:
                creates.append(t)
        r[tag + "_scene_create_ms"] = med(creates)
        host.rah_flat_free(flat)
        e.close()
        del keep
        # each edit against rtx_scene_create of the description it produces: with the object after an add, the scene as loaded after a remove
        for what, create in (("add", r[tag + "_scene_create_ms"]), ("remove", r["scene_create_ms"])):
            ms = r["%s_set_objects_%s_ms" % (tag, what)]
            if not ms < create:
                print("FAIL: %s %s: rtx_scene_set_objects (%.2f ms) costs no less than rtx_scene_create of the same description (%.2f ms)" % (tag, what, ms, create))
                ok = False
    # (d) a warm frame and the first frame of a new view, for comparison with the first frames after the edits
    for _ in range(3):
        g.render_frame(fb, mask)
    warm, after_view = [], []
    pos0, rot0 = g.camera_pose()
    for k in range(a.reps):
        warm.append(frame_ms(g))
        g.set_camera(pos0 + np.float32([0.01 * (1 + k), 0, 0]), rot0)
        after_view.append(frame_ms(g))
        frame_ms(g)
    r["frame_warm_ms"] = med(warm); r["frame_new_view_ms"] = med(after_view)
    host.rah_flat_free(first)
    g.close()
    print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(r, fh, indent=1)
    print("wrote", a.out)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
