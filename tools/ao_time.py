#!/usr/bin/env python
"""Times the ambient occlusion of a frame (rtx_render_ao, Scene.render_ao) on the GPU against the route a caller had before it (one JSON
line per scene, all of them also written to --out, stamped with the kernel sources' hash, tools/srchash.py).  Per scene, with
sphere_directions(16) and the radii +inf and 0.5:
  (a) render_ao (ao and counts) at 1024^2 and at 4096^2;
  (b) at 1024^2, where its ray buffer fits: occluded() on the same traced rays {P + N bias, d_k}, already built from render_aov's depth and
      normal -- its time alone, not render_aov, not the construction of the rays, not the reduction; the range as a prebuilt tensor
      (None for +inf).  The rays in direction-major and in pixel-major order, each with trace_reorder 0 and 1; the best of the four is the
      yardstick.
HIP events around each call after a warm-up call; median and minimum of --reps warm launches.

    python tools/ao_time.py [--reps 10] [--sizes 1024,4096] [--out run1.json]
    python tools/ao_time.py --merge run1.json run2.json run3.json --out profiles/ao_time.json

--sizes: the frame sizes of (a); (b) is measured when 1024 is among them.  --merge puts runs of the tool together: per figure the medians of the runs, their middle value and their range (the run-to-run spread), and
per scene and radius whether (a) at 1024^2 is below the best (b) by more than (b)'s spread.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENES = ("cfg2_smooth_250k", "r6_knot_250k")
RADII = (("inf", float("inf")), ("0.5", 0.5))
ORDERS = ("direction_major", "pixel_major")
BIAS = 0.0001          # Options::bias, which no scene file sets
N_DIRS = 16


def measure(a):
    import torch
    import rendering_amd as RA
    from rendering_amd import assets
    from tools.srchash import source_hash
    from tools.trace_rays_time import camera_rays, timed
    assets.ensure(); assets.ensure(["bumpy_250k.obj", "knot_250k.obj"])
    dev = "cuda:0"
    dirs = torch.from_numpy(RA.sphere_directions(N_DIRS)).to(dev)
    rows = []
    for name in SCENES:
        row = dict(scene=name, n_dirs=N_DIRS)
        for size in a.sizes:
            W = H = size
            s = RA.Scene("scenes/%s.scene" % name, W, H)
            ao = torch.zeros((H, W), dtype=torch.float32, device=dev)
            counts = torch.zeros((H, W), dtype=torch.int32, device=dev)
            for label, radius in RADII:
                key = "ao_%d_r%s" % (size, label)
                row[key + "_ms"], row[key + "_min_ms"] = timed(lambda: s.render_ao(dirs, radius, ao=ao, counts=counts), a.reps)
                torch.cuda.synchronize()
                row["traced_%d" % size] = int((counts >> 16).sum().item())
                row["open_%d_r%s" % (size, label)] = int((counts & 0xFFFF).sum().item())
            if size == 1024:
                # the caller's route: first hits, rays, occluded(); only occluded() is timed
                depth = torch.zeros((H, W), dtype=torch.float32, device=dev)
                normal = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
                obj = torch.full((H, W), -1, dtype=torch.int32, device=dev)
                s.render_aov(depth=depth, normal=normal, object_id=obj)
                cam = camera_rays(s, W, H)
                hit = (obj >= 0).view(-1)
                N = normal.view(-1, 3)
                O = cam[:, 0:3] + cam[:, 3:6] * depth.view(-1, 1) + N * BIAS
                traced = hit[:, None] & ((N @ dirs.t()) > 0)
                for order in ORDERS:
                    if order == "pixel_major":
                        pix, k = torch.nonzero(traced, as_tuple=True)
                    else:
                        k, pix = torch.nonzero(traced.t(), as_tuple=True)
                    rays = torch.cat([O[pix], dirs[k]], 1).contiguous()
                    row["rays_1024"] = int(rays.shape[0])
                    for label, radius in RADII:
                        tmax = None if radius == float("inf") else torch.full((rays.shape[0],), radius, dtype=torch.float32, device=dev)
                        for reorder in (0, 1):
                            s.set_knob("trace_reorder", reorder)
                            key = "occluded_%s_reorder%d_r%s" % (order, reorder, label)
                            row[key + "_ms"], row[key + "_min_ms"] = timed(lambda: s.occluded(rays, tmax), a.reps)
                        s.set_knob("trace_reorder", -1)
                        # (camera_rays restates the camera-ray arithmetic in torch, not bit for bit: a sanity figure only --
                        # tests/test_gpu_ao.py compares the two routes on identical rays, exactly)
                        row["open_by_occluded_r%s" % label] = int((s.occluded(rays, tmax) == 0).sum().item())
                    del rays, pix, k
                del cam, O, traced, N, depth, normal, obj
            s.close()
            del ao, counts
            torch.cuda.empty_cache()
        for label, _ in RADII if 1024 in a.sizes else ():
            row["occluded_best_r%s_ms" % label] = min(row["occluded_%s_reorder%d_r%s_ms" % (o, r, label)] for o in ORDERS for r in (0, 1))
        print(json.dumps(row), flush=True)
        rows.append(row)
    return dict(sources=source_hash(), reps=a.reps, rows=rows)


def merge(paths):
    runs = [json.load(open(p)) for p in paths]
    assert len({r["sources"] for r in runs}) == 1, "the runs are of different kernel sources"
    out = dict(sources=runs[0]["sources"], reps=runs[0]["reps"], runs=len(runs), rows=[])
    for i, first in enumerate(runs[0]["rows"]):
        row = {k: v for k, v in first.items() if not k.endswith("_ms")}
        for k in first:
            if k.endswith("_ms") and not k.endswith("_min_ms"):
                vals = sorted(r["rows"][i][k] for r in runs)
                row[k] = dict(runs=[r["rows"][i][k] for r in runs], median=vals[len(vals) // 2], range=vals[-1] - vals[0])
        for label, _ in RADII:
            # the yardstick: the order and setting that is best by its middle value; its spread: the range of its medians over the runs
            keys = ["occluded_%s_reorder%d_r%s_ms" % (o, r, label) for o in ORDERS for r in (0, 1)]
            best = min(keys, key=lambda k: row[k]["median"])
            worst_ao = max(row["ao_1024_r%s_ms" % label]["runs"])
            row["verdict_r%s" % label] = dict(yardstick=best, yardstick_ms=row[best]["median"], yardstick_spread_ms=row[best]["range"],
                                              ao_1024_ms=row["ao_1024_r%s_ms" % label]["median"], ao_1024_worst_run_ms=worst_ao,
                                              below_by_more_than_the_spread=bool(worst_ao < min(row[best]["runs"]) - row[best]["range"]))
        out["rows"].append(row)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sizes", type=lambda t: [int(x) for x in t.split(",")], default=[1024, 4096])
    ap.add_argument("--out", default=None)
    ap.add_argument("--merge", nargs="+", default=None)
    a = ap.parse_args()
    out = merge(a.merge) if a.merge else measure(a)
    if a.merge:
        for row in out["rows"]:
            print(json.dumps({k: v for k, v in row.items() if k.startswith("verdict") or k == "scene"}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            json.dump(out, fo, indent=1)


if __name__ == "__main__":
    main()
