#!/usr/bin/env python
"""Times a batch of views in one call (rtx_render_views, Scene.render_views) on the GPU against the loop a caller had before it: per view
set_camera / resize, render_pass1 and, with SSAA, sobel + render_ssaa (one JSON line per row, all of them also written to --out, stamped with
the kernel sources' hash, tools/srchash.py).  Rows, on cfg2_smooth_250k and mixed_materials, each without and with SSAA:
    256 views of 64^2, 64 views of 128^2 (a ring of cameras turning about the scene's own), the 6 faces of cube_cameras at 512^2, 1 view of 1024^2.
Both ways are timed alternately in one process, from a host clock around work that ends in a synchronise, after every shape has been warmed:
--runs runs of --reps repetitions each; per way the median of a run, then the middle value and the range of the runs' medians.  The verdict of
the 256- and 64-view rows: the batch's median is below the loop's by more than the sum of the two ranges.  Also per batch row the primary rays
per second (pixels of pass 1 / time without SSAA), to set against the headline's.

    python tools/views_time.py [--runs 3] [--reps 10] [--out profiles/views_time.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENES = ("cfg2_smooth_250k", "mixed_materials")
ROWS = (("256x64", 256, 64, "ring", True), ("64x128", 64, 128, "ring", True), ("cube6x512", 6, 512, "cube", False), ("1x1024", 1, 1024, "ring", False))


def cameras(RA, s, kind, n):
    pos, rot = s.camera_pose()
    if kind == "cube":
        return RA.cube_cameras(pos)
    # a ring: the scene's camera turned about its vertical axis, 120 degrees in all
    return [(tuple(float(x) for x in pos), (float(rot[0]), float(rot[1]) + (120.0 * k / n - 60.0 if n > 1 else 0.0), float(rot[2]))) for k in range(n)]


def measure(a):
    import torch
    import rendering_amd as RA
    from rendering_amd import assets
    from tools.srchash import source_hash
    assets.ensure(); assets.ensure(["bumpy_250k.obj"])
    dev = "cuda:0"
    rows = []
    for name in SCENES:
        path = "scenes/%s.scene" % name
        for label, n, size, kind, judged in ROWS:
            for ssaa in (False, True):
                batch_scene = RA.Scene(path, size, size)
                loop_scene = RA.Scene(path, size, size)
                loop_scene.gpu(); loop_scene.set_frame_mode(0)
                cams = cameras(RA, batch_scene, kind, n)
                fov = cams[0][2] if len(cams[0]) == 3 else None
                fbs = torch.zeros((n, size, size, 3), dtype=torch.float32, device=dev)
                masks = torch.zeros((n, size, size), dtype=torch.uint8, device=dev)
                fbs_loop = torch.zeros_like(fbs); masks_loop = torch.zeros_like(masks)

                def batch():
                    batch_scene.render_views(cams, fbs, masks if ssaa else None, ssaa=ssaa)
                    torch.cuda.synchronize()

                def loop():
                    for k, cam in enumerate(cams):
                        loop_scene.set_camera(cam[0], cam[1])
                        loop_scene.render_pass1(fbs_loop[k])
                        if ssaa:
                            loop_scene.sobel(fbs_loop[k], masks_loop[k])
                            loop_scene.render_ssaa(masks_loop[k], fbs_loop[k])
                    torch.cuda.synchronize()

                # (the one-view path has no call for the fov: the cube row's loop renders the scene's own fov -- reported, not judged)
                for _ in range(2):
                    batch(); loop()
                same = None
                if fov is None:
                    same = bool(torch.equal(fbs.view(torch.int32), fbs_loop.view(torch.int32)) and (not ssaa or torch.equal(masks, masks_loop)))
                med = dict(batch=[], loop=[])
                for _ in range(a.runs):
                    t = dict(batch=[], loop=[])
                    for _ in range(a.reps):
                        for way, f in (("loop", loop), ("batch", batch)):
                            t0 = time.perf_counter(); f(); t[way].append((time.perf_counter() - t0) * 1e3)
                    for way in t:
                        med[way].append(sorted(t[way])[len(t[way]) // 2])
                row = dict(scene=name, row=label, views=n, size=size, ssaa=ssaa, same_bits_as_loop=same)
                for way in ("batch", "loop"):
                    v = sorted(med[way])
                    row[way + "_ms"] = dict(runs=med[way], median=v[len(v) // 2], range=v[-1] - v[0])
                b, l = row["batch_ms"], row["loop_ms"]
                row["speedup"] = l["median"] / b["median"]
                if judged:
                    row["batch_below_loop_by_more_than_both_ranges"] = bool(b["median"] < l["median"] - (b["range"] + l["range"]))
                if not ssaa:
                    row["primary_rays_per_s"] = n * (size - 1) * (size - 1) / (b["median"] * 1e-3)
                else:
                    row["flagged_pixels"] = int(masks.sum().item())
                print(json.dumps(row), flush=True)
                rows.append(row)
                batch_scene.close(); loop_scene.close()
                del fbs, masks, fbs_loop, masks_loop
                torch.cuda.empty_cache()
    return dict(sources=source_hash(), runs=a.runs, reps=a.reps, rows=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = measure(a)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            json.dump(out, fo, indent=1)


if __name__ == "__main__":
    main()
