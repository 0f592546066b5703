#!/usr/bin/env python
"""Times changing the lights of a live GPU scene (rtx_scene_set_lights, include/rtx_scene_edit.h) on
scenes/cfg2_smooth_250k.scene; writes one JSON object to --out.  Medians of --reps warm runs (each after a warm-up), host wall clock
around synchronised calls, all in one process:
  set_lights_move   rtx_scene_set_lights with one of the three point lights at another position (two positions alternated), until the
                    device is idle
  set_lights_add    the same call with a fourth point light appended (alternated with the call that removes it again: the meshes' prune
                    blocks are laid out for another number of copies both ways; the removal is reported beside it)
  set_light         Scene.set_light end to end (the host's records, then the call)
  frames            a warm frame, the first frame after a light edit, the first frame of a new view (rtx_render_frame)
  scene_create      rtx_scene_create of the same description (and with the host's flattenScene before it), for comparison
The edit must cost less than the rtx_scene_create measured beside it (exit status 1 otherwise): if it does not, something is rebuilt
that does not depend on the lights.

    python tools/light_time.py [--size 4096] [--reps 7] [--out profiles/light_edit_time.json]
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
POSITIONS = [(0.4, 2.2, -1.3), (0.0, 2.0, -1.0)]      # light 0, the second is the scene file's
EXTRA = dict(position=(1.5, 1.2, -1.8), color=(0.6, 0.6, 1.0), intensity=0.4)


def med(xs):
    return float(np.median(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "light_edit_time.json"))
    a = ap.parse_args()
    import torch
    import rendering_amd as RA
    from rendering_amd import assets
    os.chdir(ROOT)
    assets.ensure([OBJ])
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
    recs, _ = g.device_lights()
    r["n_lights"] = int(len(recs))

    def lights(position0, extra):
        arr = (RA.RtxLight * (len(recs) + 1))()
        for i, rec in enumerate(recs):
            arr[i].type = int(rec["type"]); arr[i].color[:] = rec["color"].tolist(); arr[i].intensity = float(rec["intensity"])
            arr[i].dir[:] = rec["dir"].tolist(); arr[i].pos[:] = rec["pos"].tolist()
        arr[0].pos[:] = position0
        k = len(recs)
        arr[k].type = 2; arr[k].color[:] = EXTRA["color"]; arr[k].intensity = EXTRA["intensity"]; arr[k].pos[:] = EXTRA["position"]
        return arr, len(recs) + (1 if extra else 0)

    def set_lights(arr, n):
        t, rc = timed(lambda: rtx.rtx_scene_set_lights(g.gpu(), n, arr))
        assert rc == 0, rtx.rtx_last_error()
        return t

    # (a) rtx_scene_set_lights: one point light moved
    moved = [lights(p, False) for p in POSITIONS]
    ts = [set_lights(*moved[k % 2]) for k in range(a.reps + 1)][1:]
    r["set_lights_move_ms"] = med(ts)
    # (b) ... a point light added / removed again
    both = [lights(POSITIONS[1], True), lights(POSITIONS[1], False)]
    ts = [set_lights(*both[k % 2]) for k in range(2 * a.reps + 2)][2:]
    r["set_lights_add_ms"] = med(ts[0::2]); r["set_lights_remove_ms"] = med(ts[1::2])
    # (c) Scene.set_light end to end
    ts = [timed(lambda: g.set_light(0, position=POSITIONS[k % 2]))[0] for k in range(a.reps + 1)][1:]
    r["set_light_ms"] = med(ts)
    # (d) frames: warm, the first after a light edit, the first of a new view
    for _ in range(3):
        g.render_frame(fb, mask)
    warm, after_edit, after_view = [], [], []
    pos0, rot0 = g.camera_pose()
    for k in range(a.reps):
        warm.append(frame_ms(g))
        g.set_light(0, position=POSITIONS[k % 2]); sync()
        after_edit.append(frame_ms(g))
        g.set_camera(pos0 + np.float32([0.01 * (1 + k), 0, 0]), rot0)
        after_view.append(frame_ms(g))
        frame_ms(g)
    r["frame_warm_ms"] = med(warm); r["frame_after_light_edit_ms"] = med(after_edit); r["frame_new_view_ms"] = med(after_view)
    # (e) rtx_scene_create of the same description
    creates, with_flatten = [], []
    for k in range(a.reps + 1):
        sync(); t0 = time.perf_counter()
        f = host.rah_flatten(g.h)
        out = C.c_void_p()
        t1 = time.perf_counter()
        rc = rtx.rtx_scene_create(C.c_void_p(host.rah_flat_desc(f)), 0, C.byref(out))
        sync()
        t2 = time.perf_counter()
        host.rah_flat_free(f)
        assert rc == 0, rtx.rtx_last_error()
        rtx.rtx_scene_destroy(out)
        if k:
            creates.append((t2 - t1) * 1e3); with_flatten.append((t2 - t0) * 1e3)
    r["scene_create_ms"] = med(creates); r["flatten_and_scene_create_ms"] = med(with_flatten)
    r["create_over_set_lights_move"] = r["scene_create_ms"] / r["set_lights_move_ms"]
    g.close()
    print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(r, fh, indent=1)
    print("wrote", a.out)
    slowest = max(r["set_lights_move_ms"], r["set_lights_add_ms"], r["set_lights_remove_ms"], r["set_light_ms"])
    if not slowest < r["scene_create_ms"]:
        print("FAIL: a light edit (%.2f ms) costs no less than rtx_scene_create (%.2f ms)" % (slowest, r["scene_create_ms"]))
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
