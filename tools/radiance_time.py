#!/usr/bin/env python
"""Times radiance gathered over directions at caller-supplied surface points (rtx_radiance_points, Scene.radiance_points) on the GPU
against the route a caller had before it (one JSON line per scene, all of them also written to --out, stamped with the kernel sources'
hash, tools/srchash.py).  Scenes cfg2_smooth_250k and mixed_materials; points: the first hits of the size^2 camera rays ({P, N} from
surface_rays), for every size of --sizes; directions: sphere_directions(16), cosine-weighted with seeded weights.  Per scene:
  (a) radiance_points (the sums), and (a') the same with the points grouped by key whatever their number (knob trace_reorder = 1);
  (b) the composed route on the older calls: the rays {P + N * bias, d_k} of every (point, direction) with N . d_k > 0 built in torch,
      trace_rays(colours=True), and the weighted sum in torch (index_add_ over the traced rays, whose order of additions is not the
      contract's: the figures of (b) are not bit for bit those of (a)); with the peak of the bytes torch allocates meanwhile;
  (c) ao_points on the same points and directions: the floor of what the walks of the first rays alone cost.
HIP events around each call after a warm-up call, the median of --reps warm launches; the figures are measured in turn, --runs times over
(alternated: a drift of the device shows as a spread within every figure, not as a difference between them).  Reported per figure: the
runs' medians, their middle value and their range, and whether the worst run of (a) is below the best run of (b).

    python tools/radiance_time.py [--reps 5] [--runs 3] [--sizes 1024] [--out profiles/radiance_time.json]
    python tools/radiance_time.py --add-resources build/hipcc.log [--out profiles/radiance_time.json]

The second form needs no GPU: it adds to the file the compiler's resource lines (build.sh keeps them in build/hipcc.log) of every instance
of rtxPointRadianceKernel and of rtxRayColourKernel, whose recursion it shares -- VGPRs, SGPRs, scratch bytes per lane, waves per SIMD,
spilled registers, LDS bytes per block."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENES = ["cfg2_smooth_250k", "mixed_materials"]
BIAS = 0.0001          # Options::bias, which no scene file sets
N_DIRS = 16


def composed(s, points, dirs, weights):
    """(b): the contract of include/rtx_radiance.h on the caller's side.  Returns (sums, number of traced rays)."""
    import torch
    P, N = points[:, 0:3], points[:, 3:6]
    c = N @ dirs.t()
    pt, kk = (c > 0).nonzero(as_tuple=True)
    rays = torch.cat([(P + N * BIAS)[pt], dirs[kk]], 1).contiguous()
    _, col = s.trace_rays(rays, hits=False, colours=True)
    total = torch.zeros_like(P)
    total.index_add_(0, pt, col * (weights[kk] * c[pt, kk])[:, None])
    return total, int(rays.shape[0])


def regrouped(s, fn):
    """(a'): fn() with the batch grouped by key however small it is"""
    s.set_knob("trace_reorder", 1)
    try:
        return fn()
    finally:
        s.set_knob("trace_reorder", -1)


def measure(a):
    import numpy as np
    import torch
    import rendering_amd as RA
    from rendering_amd import assets
    from tools.srchash import source_hash
    from tools.trace_rays_time import camera_rays, timed
    assets.ensure(); assets.ensure(["bumpy_250k.obj"])
    dev = "cuda:0"
    dirs = torch.from_numpy(RA.sphere_directions(N_DIRS)).to(dev)
    weights = torch.from_numpy(np.random.default_rng(16).uniform(0.5, 1.5, N_DIRS).astype(np.float32)).to(dev)
    rows = []
    for scene, size in [(scene, size) for size in a.sizes for scene in SCENES]:
        W = H = size
        s = RA.Scene("scenes/%s.scene" % scene, W, H)
        cam = camera_rays(s, W, H)
        first = s.surface_rays(cam, hits=True, position=True, normal=True, albedo=False)
        hit = first["hits"][:, 0] > 0
        points = torch.cat([first["position"], first["normal"]], 1)[hit].contiguous()
        del cam, first
        n = int(points.shape[0])
        v = s.kernel_variant()
        row = dict(scene=scene, size=size, n=n, n_dirs=N_DIRS, variant=sorted(k for k, on in v.items() if on))
        figures = {
            "a_radiance_points": lambda: s.radiance_points(points, dirs, weights, cosine=True),
            "a_regrouped": lambda: regrouped(s, lambda: s.radiance_points(points, dirs, weights, cosine=True)),
            "b_composed": lambda: composed(s, points, dirs, weights),
            "c_ao_points": lambda: s.ao_points(points, dirs, counts=True),
        }
        runs = {key: [] for key in figures}
        for _ in range(a.runs):
            for key, fn in figures.items():
                runs[key].append(timed(fn, a.reps)[0])
        for key, vals in runs.items():
            row[key + "_ms"] = dict(runs=vals, median=sorted(vals)[len(vals) // 2], range=max(vals) - min(vals))
        # the bytes torch allocates at the peak of one composed call, and of one call of (a): its output
        for key in ("a_radiance_points", "b_composed"):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            out = figures[key]()
            torch.cuda.synchronize()
            row[key + "_peak_bytes"] = int(torch.cuda.max_memory_allocated() - base)
            del out
        total, n_rays = composed(s, points, dirs, weights)
        mine = s.radiance_points(points, dirs, weights, cosine=True, counts=True)
        torch.cuda.synchronize()
        # (sanity figures only: the composed route adds in another order -- tests/test_gpu_radiance.py compares exactly)
        row["traced_rays"] = [n_rays, int(mine["counts"].sum().item())]
        row["composed_max_abs_difference"] = float((total - mine["sum"]).abs().max().item())
        row["sum_max"] = float(mine["sum"].abs().max().item())
        aa, bb = row["a_radiance_points_ms"], row["b_composed_ms"]
        row["a_below_b_in_every_run"] = bool(max(aa["runs"]) < min(bb["runs"]))
        print(json.dumps(row), flush=True)
        rows.append(row)
        s.close()
    return dict(sources=source_hash(), reps=a.reps, runs=a.runs, rows=rows)


def resources(log):
    """kernel name -> its resource figures, for the two kernel families, from the remarks of -Rpass-analysis=kernel-resource-usage"""
    import re
    keys = {"TotalSGPRs": "sgprs", "VGPRs": "vgprs", "ScratchSize [bytes/lane]": "scratch_bytes_per_lane", "Occupancy [waves/SIMD]": "waves_per_simd",
            "SGPRs Spill": "sgprs_spilled", "VGPRs Spill": "vgprs_spilled", "LDS Size [bytes/block]": "lds_bytes_per_block"}
    out, cur = {}, None
    for ln in open(log):
        m = re.search(r"remark: \S+ +(.+?): (\S+) \[-Rpass-analysis", ln)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = m.group(2) if re.match(r"_Z\d+rtx(PointRadiance|RayColour)Kernel", m.group(2)) else None
            if cur:
                out[cur] = {}
        elif cur and m.group(1) in keys:
            out[cur][keys[m.group(1)]] = int(m.group(2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--sizes", type=lambda v: [int(x) for x in v.split(",")], default=[1024])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "radiance_time.json"))
    ap.add_argument("--add-resources", default=None)
    a = ap.parse_args()
    if a.add_resources:
        out = json.load(open(a.out))
        out["resources"] = resources(a.add_resources)
        assert len(out["resources"]) == 18, "nine instances of each kernel family are expected, got %d" % len(out["resources"])
    else:
        out = measure(a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        json.dump(out, fo, indent=1)


if __name__ == "__main__":
    main()
