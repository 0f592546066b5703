#!/usr/bin/env python
"""Times rtx_surface_rays (Scene.surface_rays) on the GPU against the routes a caller had before it (one JSON line per scene and ray set,
all of them also written to --out, stamped with the kernel sources' hash, tools/srchash.py).  Per scene two ray sets:
  camera   the camera rays of a 2048^2 view, in pixel order (coherent, 4.2 M);
  bounce   tools/ao_time.py's traced rays of a 1024^2 view with sphere_directions(16), pixel-major, compacted (incoherent, about 5 M);
each with the knob trace_reorder at its default (-1), at 0 (as given) and at 1 (always grouped by key), and per setting the rows
  (a) surface_rays, all five channels;
  (b) surface_rays, hits + normal;
  (c) surface_rays, normal + albedo;
  (d) trace_rays, hits only                          -- existing code: the yardstick of the walk alone;
  (e) trace_rays, hits + colours under showNormals   -- existing code: the only earlier route to anything like a normal; it writes the same
                                                        44 bytes per ray as (b).
HIP events around each call after a warm-up call; median and minimum of --reps warm launches, one process.

    python tools/surface_time.py [--reps 10] [--out run1.json]
    python tools/surface_time.py --merge run1.json run2.json run3.json --out profiles/surface_time.json

--merge puts runs of the tool together: per figure the medians of the runs, their middle value and their range (the run-to-run spread);
per scene, ray set and setting whether (b) is no slower than (e) beyond (e)'s spread, and (a) - (d), the price of the surface data.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENES = ("cfg2_smooth_250k", "r6_knot_250k")
REORDER = (("default", -1), ("as_given", 0), ("grouped", 1))
ROWS = ("a_all_five", "b_hits_normal", "c_normal_albedo", "d_trace_hits", "e_trace_show_normals")
BIAS = 0.0001          # Options::bias, which no scene file sets
N_DIRS = 16


def bounce_rays(s, W, H, dirs):
    """tools/ao_time.py's traced rays of the frame: {P + N bias, d_k} for N . d_k > 0, pixel-major"""
    import torch
    from tools.trace_rays_time import camera_rays
    dev = "cuda:0"
    depth = torch.zeros((H, W), dtype=torch.float32, device=dev)
    normal = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
    obj = torch.full((H, W), -1, dtype=torch.int32, device=dev)
    s.render_aov(depth=depth, normal=normal, object_id=obj)
    cam = camera_rays(s, W, H)
    N = normal.view(-1, 3)
    O = cam[:, 0:3] + cam[:, 3:6] * depth.view(-1, 1) + N * BIAS
    traced = (obj >= 0).view(-1)[:, None] & ((N @ dirs.t()) > 0)
    pix, k = torch.nonzero(traced, as_tuple=True)
    return torch.cat([O[pix], dirs[k]], 1).contiguous()


def measure(a):
    import torch
    import rendering_amd as RA
    from rendering_amd import assets
    from tools.srchash import source_hash
    from tools.trace_rays_time import camera_rays, timed
    assets.ensure(); assets.ensure(["bumpy_250k.obj", "knot_250k.obj"])
    dirs = torch.from_numpy(RA.sphere_directions(N_DIRS)).to("cuda:0")
    rows = []
    for name in SCENES:
        s = RA.Scene("scenes/%s.scene" % name, 1024, 1024)
        sets = [("bounce", bounce_rays(s, 1024, 1024, dirs))]
        s.resize(2048, 2048)
        sets.insert(0, ("camera", camera_rays(s, 2048, 2048)))
        for set_name, rays in sets:
            row = dict(scene=name, rays=set_name, n=int(rays.shape[0]))
            out = s.surface_rays(rays, hits=True)
            row["hit_share"] = float((out["hits"][:, 0] > 0).float().mean().item())
            del out
            for label, reorder in REORDER:
                s.set_knob("trace_reorder", reorder)
                calls = {
                    "a_all_five": lambda: s.surface_rays(rays, hits=True, position=True, normal=True, albedo=True, specular=True),
                    "b_hits_normal": lambda: s.surface_rays(rays, hits=True, normal=True, albedo=False),
                    "c_normal_albedo": lambda: s.surface_rays(rays),
                    "d_trace_hits": lambda: s.trace_rays(rays, hits=True, colours=False),
                    "e_trace_show_normals": lambda: s.trace_rays(rays, hits=True, colours=True),
                }
                for r in ROWS:
                    if r == "e_trace_show_normals":
                        s.set_flag("showNormals", 1)
                    key = "%s_%s" % (r, label)
                    row[key + "_ms"], row[key + "_min_ms"] = timed(calls[r], a.reps)
                    if r == "e_trace_show_normals":
                        s.set_flag("showNormals", 0)
            s.set_knob("trace_reorder", -1)
            print(json.dumps(row), flush=True)
            rows.append(row)
        del sets, rays
        s.close()
        torch.cuda.empty_cache()
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
        for label, _ in REORDER:
            fig = {r: row["%s_%s_ms" % (r, label)] for r in ROWS}
            b, e = fig["b_hits_normal"], fig["e_trace_show_normals"]
            row["verdict_" + label] = dict(b_ms=b["median"], b_spread_ms=b["range"], e_ms=e["median"], e_spread_ms=e["range"],
                                           b_no_slower_than_e_beyond_the_spread=bool(b["median"] <= e["median"] + max(b["range"], e["range"])),
                                           price_of_surface_a_minus_d_ms=fig["a_all_five"]["median"] - fig["d_trace_hits"]["median"])
        out["rows"].append(row)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--merge", nargs="+", default=None)
    a = ap.parse_args()
    out = merge(a.merge) if a.merge else measure(a)
    if a.merge:
        for row in out["rows"]:
            print(json.dumps({k: v for k, v in row.items() if k.startswith("verdict") or k in ("scene", "rays")}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            json.dump(out, fo, indent=1)


if __name__ == "__main__":
    main()
