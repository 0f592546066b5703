#!/usr/bin/env python
"""Times rtx_texel_points and rtx_dilate_texels (include/rtx_bake.h); writes one JSON object to --out, stamped with
tools/srchash.py.  The method of the other timing tools: buffers allocated once, warm-up calls, then an event pair around each of --reps calls
on one stream; the middle and the range [min, max] are kept.  A call is everything the entry point queues (the owner words' reset, the bin
kernel, the scan, the chunk kernel, the write kernel), so its time is the sum of its kernels and the gaps between them; the kernels one by one
come from a profiler run of one workload (--only NAME under rocprofv3 --kernel-trace --stats, then --kernel-stats NAME=CSV adds them here).

Workloads (mesh, map):
  cfg2_250k_{1024,64}   the mesh of scenes/cfg2_smooth_250k.scene as it is: its OBJ file has no texture coordinates, so every triangle's
                        layout is the point (0, 0) and nothing is covered -- what is left is the cost of looking at 250 000 triangles
  torus250k_{1024,64}   torus_obj(500, 250): 250 000 triangles whose layout tiles [0, 1]^2 (at 64^2 most triangles contain no centre)
  quad_4096             two triangles that span all of a 4096^2 map (the chunk path alone)
  dilate_1024           rtx_dilate_texels, 2 passes, 3 channels, on the sparse layout of tests/util_texel_points.charts_obj at 1024^2
Every row has the bytes the call must write (full: w * h * 36), the time that takes at the HBM rate of the guide (6.3 TB/s achievable) and
its share of the measured time.

--restatement times the numpy restatement (tests/util_texel_points.texel_points_ref) of torus250k at 1024^2 on the host instead: the only
alternative there was; it needs no GPU and adds its row to the same file.

    python tools/texel_points_time.py [--reps 9] [--only NAME] [--out profiles/texel_points_time.json]
    python tools/texel_points_time.py --restatement
    python tools/texel_points_time.py --kernel-stats torus250k_1024=DIR/x_kernel_stats.csv
"""
import argparse
import csv
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 6.3e12


def spread(xs):
    return [float(np.median(xs)), float(min(xs)), float(max(xs))]


def scenes(d):
    from rendering_amd import assets
    from tests import util_texel_points as U
    assets.ensure(["bumpy_250k.obj"])
    return {"cfg2": ("scenes/cfg2_smooth_250k.scene", 1),
            "torus250k": (U.write_mesh_scene(d, "torus250k", assets.torus_obj(500, 250)), 0),
            "quad": (U.write_mesh_scene(d, "quad", U.quad_obj()), 0),
            "charts": (U.write_mesh_scene(d, "charts", U.charts_obj()), 0)}


WORKLOADS = [("cfg2_250k_1024", "cfg2", 1024), ("cfg2_250k_64", "cfg2", 64), ("torus250k_1024", "torus250k", 1024), ("torus250k_64", "torus250k", 64),
             ("quad_4096", "quad", 4096)]


def merge(path, update):
    from tools.srchash import source_hash
    d = {}
    if os.path.exists(path):
        d = json.load(open(path))
        if d.get("source_hash") != source_hash():
            d = {}
    d.setdefault("source_hash", source_hash())
    for k, v in update.items():
        if isinstance(v, dict):
            d.setdefault(k, {}).update(v)
        else:
            d[k] = v
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(d, fh, indent=1)
    print("wrote", path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--only", default=None)
    ap.add_argument("--restatement", action="store_true")
    ap.add_argument("--kernel-stats", default=None, metavar="NAME=CSV")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "texel_points_time.json"))
    a = ap.parse_args()
    os.chdir(ROOT)
    if a.kernel_stats:
        name, path = a.kernel_stats.split("=", 1)
        rows = {}
        for r in csv.DictReader(open(path)):
            # (the call's own kernels, the scan's and the owner words' reset; the fill also serves torch in the same run)
            if not any(s in r["Name"] for s in ("rtxbake::", "rocprim", "fillBufferAligned")):
                continue
            rows[r["Name"].split("(")[0].split("<")[0]] = dict(calls=int(r["Calls"]), average_us=float(r["AverageNs"]) / 1e3, min_us=float(r["MinNs"]) / 1e3,
                                                 max_us=float(r["MaxNs"]) / 1e3)
        merge(a.out, {"kernels": {name: rows}})
        return
    import rendering_amd as RA
    from tests import util_texel_points as U
    RA.load()
    d = tempfile.mkdtemp(prefix="texel_points_time_")
    sc = scenes(d)
    if a.restatement:
        from oracle import oracle as O
        g = RA.Scene(sc["torus250k"][0], 64, 48, cwd=ROOT)
        tris = U.triangles(g, sc["torus250k"][1])
        g.close()
        t0 = time.perf_counter()
        r = U.texel_points_ref(*tris, 1024, 1024, O.normalize_n)
        sec = time.perf_counter() - t0
        merge(a.out, {"host_restatement": dict(workload="torus250k_1024", seconds=sec, covered=int((r["tri"] >= 0).sum()), what="numpy, one core")})
        return

    import torch
    rtx, _ = RA.load()
    sync = torch.cuda.synchronize
    stream = torch.cuda.current_stream()
    st = C.c_void_p(stream.cuda_stream)

    def timed(call, before=None):
        for _ in range(3):
            if before:
                before()
            call()
        sync()
        ms = []
        for _ in range(a.reps):
            if before:
                before()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream); call(); e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return ms

    def row(ms, nbytes):
        floor_ms = nbytes / HBM_BYTES_PER_S * 1e3
        m = spread(ms)
        return dict(ms=m, bytes_written=int(nbytes), hbm_floor_ms=floor_ms, floor_over_measured=floor_ms / m[0])

    result = {}
    live = {}
    for name, key, size in WORKLOADS:
        if a.only and a.only != name:
            continue
        if key not in live:
            live[key] = RA.Scene(sc[key][0], 64, 48, cwd=ROOT)
        g, obj = live[key], sc[key][1]
        mesh = sum(1 for i in range(obj) if g.host.rah_object_type(g.h, i) == 3)
        n = size * size
        P = torch.empty((n, 6), dtype=torch.float32, device="cuda")
        T = torch.empty((size, size), dtype=torch.int32, device="cuda")
        B = torch.empty((size, size, 2), dtype=torch.float32, device="cuda")
        full, tri_only = RA.TexelBuffers(P.data_ptr(), T.data_ptr(), B.data_ptr()), RA.TexelBuffers(None, T.data_ptr(), None)
        sp = g.gpu()

        def call(buf):
            assert rtx.rtx_texel_points(sp, mesh, size, size, C.byref(buf), st) == 0, rtx.rtx_last_error()

        out = dict(n_tris=int(g.bvh(obj)["n_tris"]), size=[size, size], full=row(timed(lambda: call(full)), n * 36),
                   tri_only=row(timed(lambda: call(tri_only)), n * 4))
        sync()
        out["covered"] = int((T >= 0).sum())
        result[name] = out
        print(json.dumps({name: out}), flush=True)
        del P, T, B
    if not a.only or a.only == "dilate_1024":
        g = RA.Scene(sc["charts"][0], 64, 48, cwd=ROOT)
        size, ch, passes = 1024, 3, 2
        tri0 = g.texel_points(0, size, size, points=False)["tri"]
        img = torch.rand((size, size, ch), dtype=torch.float32, device="cuda")
        tri = tri0.clone()
        sp = g.gpu()
        ms = timed(lambda: rtx.rtx_dilate_texels(sp, size, size, ch, C.c_void_p(img.data_ptr()), C.c_void_p(tri.data_ptr()), passes, st),
                   before=lambda: tri.copy_(tri0))
        sync()
        filled = int((tri == -2).sum())
        # per pass every texel's tri is read and written; a filled texel's channels are read and written once
        nbytes = passes * size * size * 4 + filled * ch * 4
        out = row(ms, nbytes)
        out.update(size=[size, size], channels=ch, passes=passes, uncovered=int((tri0 == -1).sum()), filled=filled)
        result["dilate_1024"] = out
        print(json.dumps({"dilate_1024": out}), flush=True)
        g.close()
    for g in live.values():
        g.close()
    merge(a.out, {"device": torch.cuda.get_device_name(0), "reps": a.reps, "columns": ["middle", "min", "max"],
                  "hbm_bytes_per_s": HBM_BYTES_PER_S, "workloads": result})


if __name__ == "__main__":
    main()
