#!/usr/bin/env python
"""Times the direct light of a frame (rtx_render_light, Scene.render_light) on the GPU against the route a caller had before it (one JSON
line per scene and size, all of them also written to --out, stamped with the kernel sources' hash, tools/srchash.py).  Scenes
cfg2_smooth_250k (three point lights) and area_light (two area lights of 9 and 1 samples, one point light), at 1024^2 and 4096^2:
  (a) render_light, the two sums only;
  (b) render_light with all five buffers;
  (c) light_rays on the view's camera rays, which are built once beforehand and not timed -- the two sums only, and with per_light --,
      and the bytes of its ray buffer.
HIP events around each call after a warm-up call; median and minimum of --reps warm launches.

    python tools/render_light_time.py [--reps 10] [--sizes 1024,4096] [--form plain] [--out run1.json]
    python tools/render_light_time.py --merge run1.json run2.json run3.json [--other parked1.json parked2.json parked3.json] --out profiles/render_light_time.json

--form: a label for the register form of the kernel the library was built with (RTX_LIGHT_FRAME_PARK, rtx_render_light.hip).  --merge puts
runs of the tool together: per figure the medians of the runs, their middle value and their range (the run-to-run spread), and per scene
and size whether (a) is below (c) by more than the two spreads.  --other: runs with the library of the other form, of which (a) and (b)
are reported next to the first form's.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENES = ("cfg2_smooth_250k", "area_light")


def measure(a):
    import torch
    import rendering_amd as RA
    from rendering_amd import assets
    from tools.srchash import source_hash
    from tools.trace_rays_time import camera_rays, timed
    assets.ensure(); assets.ensure(["bumpy_250k.obj"])
    dev = "cuda:0"
    rows = []
    for name in SCENES:
        for size in a.sizes:
            W = H = size
            s = RA.Scene("scenes/%s.scene" % name, W, H)
            L = s.n_lights
            row = dict(scene=name, size=size, n_lights=L)
            z = lambda shape, dt=torch.float32: torch.zeros(shape, dtype=dt, device=dev)
            sums = dict(diffuse=z((H, W, 3)), specular=z((H, W, 3)))
            row["a_sums_ms"], row["a_sums_min_ms"] = timed(lambda: s.render_light(**sums), a.reps)
            per = dict(light_diffuse=z((L, H, W, 3)), light_specular=z((L, H, W, 3)), light_open=z((L, H, W), torch.int32))
            row["b_all_ms"], row["b_all_min_ms"] = timed(lambda: s.render_light(**sums, **per), a.reps)
            torch.cuda.synchronize()
            row["open_pairs"] = int((per["light_open"] > 0).sum().item())
            frame = (sums["diffuse"].clone(), sums["specular"].clone())
            del per
            cam = camera_rays(s, W, H)
            row["c_ray_buffer_bytes"] = int(cam.numel() * 4)
            row["c_sums_ms"], row["c_sums_min_ms"] = timed(lambda: s.light_rays(cam), a.reps)
            row["c_per_light_ms"], row["c_per_light_min_ms"] = timed(lambda: s.light_rays(cam, per_light=True), a.reps)
            out = s.light_rays(cam)
            torch.cuda.synchronize()
            # (camera_rays restates the camera-ray arithmetic in torch, not bit for bit: a sanity figure only --
            # tests/test_gpu_render_light.py compares the two routes on identical rays, exactly)
            row["c_max_abs_difference"] = float(max((out["diffuse"].view(H, W, 3)[:-1, :-1] - frame[0][:-1, :-1]).abs().max().item(),
                                                    (out["specular"].view(H, W, 3)[:-1, :-1] - frame[1][:-1, :-1]).abs().max().item()))
            s.close()
            del cam, out, frame, sums
            torch.cuda.empty_cache()
            print(json.dumps(row), flush=True)
            rows.append(row)
    return dict(sources=source_hash(), form=a.form, reps=a.reps, rows=rows)


def spread(runs, i, k):
    vals = [r["rows"][i][k] for r in runs]
    return dict(runs=vals, median=sorted(vals)[len(vals) // 2], range=max(vals) - min(vals))


def merge(paths, other):
    runs = [json.load(open(p)) for p in paths]
    others = [json.load(open(p)) for p in other]
    assert len({r["sources"] for r in runs + others}) == 1, "the runs are of different kernel sources"
    assert len({r["form"] for r in runs}) == 1 and len({r["form"] for r in others}) <= 1
    out = dict(sources=runs[0]["sources"], form=runs[0]["form"], reps=runs[0]["reps"], runs=len(runs), rows=[])
    for i, first in enumerate(runs[0]["rows"]):
        row = {k: v for k, v in first.items() if not k.endswith("_ms")}
        for k in first:
            if k.endswith("_ms") and not k.endswith("_min_ms"):
                row[k] = spread(runs, i, k)
        if others:
            for k in ("a_sums_ms", "b_all_ms"):
                row["%s_%s" % (others[0]["form"], k)] = spread(others, i, k)
        a_, c_ = row["a_sums_ms"], row["c_sums_ms"]
        row["a_below_c_by_more_than_the_two_spreads"] = bool(c_["median"] - a_["median"] > a_["range"] + c_["range"])
        b_, c_ = row["b_all_ms"], row["c_per_light_ms"]
        row["b_below_c_per_light_by_more_than_the_two_spreads"] = bool(c_["median"] - b_["median"] > b_["range"] + c_["range"])
        out["rows"].append(row)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sizes", type=lambda t: [int(x) for x in t.split(",")], default=[1024, 4096])
    ap.add_argument("--form", default="plain")
    ap.add_argument("--out", default=None)
    ap.add_argument("--merge", nargs="+", default=None)
    ap.add_argument("--other", nargs="+", default=[])
    a = ap.parse_args()
    out = merge(a.merge, a.other) if a.merge else measure(a)
    if a.merge:
        for row in out["rows"]:
            print(json.dumps({k: (v["median"] if isinstance(v, dict) else v) for k, v in row.items()}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            json.dump(out, fo, indent=1)


if __name__ == "__main__":
    main()
