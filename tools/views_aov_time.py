#!/usr/bin/env python
"""Times the first-hit buffers of a batch of views in one call (rtx_render_views_aov, Scene.render_views_aov) on the GPU against the loop a
caller had before it: per view set_camera + render_aov (one JSON line per row, all of them also written to --out, stamped with the kernel
sources' hash, tools/srchash.py).  Rows, on cfg2_smooth_250k and mixed_materials:
    256 views of 64^2, 64 views of 128^2 (a ring of cameras turning about the scene's own), the 6 directions of cube_cameras at 512^2 (with
    the scene's own fov: the one-view path has no call for another, and every row is first checked against the loop bit for bit), 1 view of
    1024^2.
Each in three forms:
    geometry  depth, object_id, triangle_id, uv from the call and from the loop (no surface fetch in either)
    all       the call's eight channels against the loop's six
    rays      the `rays` channel alone; no loop has it, so only the call is timed (its bits are checked against the form `all`)
Both ways are timed alternately in one process, from a host clock around work that ends in a synchronise, after every shape has been warmed:
--runs runs of --reps repetitions each; per way the median of a run, then the middle value and the range of the runs' medians.  The verdict of
the 256- and 64-view rows: the batch's median is below the loop's by more than the sum of the two ranges.  The one-view row records by how
much the one-view call, which walks with the camera's copies of the prune records, wins.

    python tools/views_aov_time.py [--runs 3] [--reps 10] [--out profiles/views_aov_time.json]
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
TAIL = {"depth": (), "object_id": (), "triangle_id": (), "uv": (2,), "normal": (3,), "albedo": (3,), "position": (3,), "rays": (6,)}
LOOP_ALL = ("depth", "object_id", "triangle_id", "uv", "normal", "albedo")
FORMS = (("geometry", LOOP_ALL[:4], LOOP_ALL[:4]), ("all", tuple(TAIL), LOOP_ALL), ("rays", ("rays",), ()))


def cameras(RA, s, kind, n):
    pos, rot = s.camera_pose()
    if kind == "cube":
        return [(p, r) for p, r, _ in RA.cube_cameras(pos)]
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

    def tensors(n, size, names):
        return {c: torch.zeros((n, size, size) + TAIL[c], dtype=torch.int32 if c.endswith("_id") else torch.float32, device=dev) for c in names}

    for name in SCENES:
        path = "scenes/%s.scene" % name
        for label, n, size, kind, judged in ROWS:
            rays_of_all = None
            for form, names, loop_names in FORMS:
                batch_scene = RA.Scene(path, size, size)
                loop_scene = RA.Scene(path, size, size)
                loop_scene.gpu()
                cams = cameras(RA, batch_scene, kind, n)
                out = tensors(n, size, names)
                out_loop = tensors(n, size, loop_names)

                def batch():
                    batch_scene.render_views_aov(cams, **out)
                    torch.cuda.synchronize()

                def loop():
                    for k, cam in enumerate(cams):
                        loop_scene.set_camera(cam[0], cam[1])
                        loop_scene.render_aov(**{c: t[k] for c, t in out_loop.items()})
                    torch.cuda.synchronize()

                ways = (("loop", loop), ("batch", batch)) if loop_names else (("batch", batch),)
                for _ in range(2):
                    for _, f in ways:
                        f()
                if loop_names:
                    same = all(torch.equal(out[c].view(torch.int32), out_loop[c].view(torch.int32)) for c in loop_names)
                else:
                    same = bool(torch.equal(out["rays"].view(torch.int32), rays_of_all.view(torch.int32)))
                assert same, "%s %s %s: the batch's bits are not the loop's" % (name, label, form)
                if form == "all":
                    rays_of_all = out["rays"].clone()
                med = {way: [] for way, _ in ways}
                for _ in range(a.runs):
                    t = {way: [] for way, _ in ways}
                    for _ in range(a.reps):
                        for way, f in ways:
                            t0 = time.perf_counter(); f(); t[way].append((time.perf_counter() - t0) * 1e3)
                    for way in t:
                        med[way].append(sorted(t[way])[len(t[way]) // 2])
                row = dict(scene=name, row=label, views=n, size=size, form=form, channels=list(names), same_bits_as_loop=bool(same))
                for way in med:
                    v = sorted(med[way])
                    row[way + "_ms"] = dict(runs=med[way], median=v[len(v) // 2], range=v[-1] - v[0])
                b = row["batch_ms"]
                if loop_names:
                    l = row["loop_ms"]
                    row["speedup"] = l["median"] / b["median"]
                    if judged:
                        row["batch_below_loop_by_more_than_both_ranges"] = bool(b["median"] < l["median"] - (b["range"] + l["range"]))
                row["primary_rays_per_s"] = n * (size - 1) * (size - 1) / (b["median"] * 1e-3)
                print(json.dumps(row), flush=True)
                rows.append(row)
                batch_scene.close(); loop_scene.close()
                del out, out_loop
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
