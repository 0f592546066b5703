#!/usr/bin/env python
"""Times surface points projected into cameras with visibility (rtx_project_points, Scene.project_points) on the GPU against the route a
caller had before it (one JSON line per case, all of them also written to --out, stamped with the kernel sources' hash, tools/srchash.py).
Scene cfg2_smooth_250k; the points are the first hits of the size^2 camera rays ({P, N} from surface_rays).  Cases: K = 1, another camera;
K = 6, the cube cameras at a point beside the mesh; each with and without visibility.  Per case:
  (a) project_points on a camera table made beforehand (pixel and flags);
  (c) the composed route on the older calls: per camera the camera restated in torch from the table's fields (the difference, a 3 x 3
      product, the divisions, the frame test), and with visibility an n x 6 ray buffer {O, -L}, an n-float range buffer (NaN for the pairs
      outside the frame, which occluded() then does not walk) and occluded().  Its kernels are the parent's: this pull request changes none
      of them.  Its pixels are torch's fp32, not the contract's: the largest deviation from (a) over the pairs inside the frame is reported.
HIP events around each call after a warm-up call, the median of --reps warm launches; the figures are measured in turn, --runs times over
(alternated: a drift of the device shows as a spread within every figure, not as a difference between them).  Reported per figure: the
runs' medians, their middle value and their range, and whether the worst run of (a) is below the best run of (c) by more than the two
ranges together (DESIGN.md 3.20's rule).

    python tools/project_time.py [--reps 10] [--runs 3] [--size 1024] [--out profiles/project_time.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENE = "cfg2_smooth_250k"
BIAS = 0.0001          # Options::bias, which no scene file sets
OTHER = ((3.0, 1.0, -0.5), (14.0, -50.0, 0.0))
CUBE_AT = (1.5, 1.0, -1.0)


def composed(s, points, table, visibility):
    """(c).  Returns (pixel (K, n, 2), inside (K, n), open (K, n) or None, bytes of ray and range buffers allocated)."""
    import torch
    P, N = points[:, 0:3], points[:, 3:6]
    O = P + N * BIAS
    pixels, insides, opens = [], [], []
    nbytes = 0
    for R in table:
        C, scale, aspect, width, height = R[0:3], R[3], R[4], R[5], R[6]
        M = R[8:24].view(4, 4)[:3, :3]
        c = P - C
        sc = c @ M.t()
        inz = -sc[:, 2]
        px = (sc[:, 0] / inz / (scale * aspect) + 1) * (width * 0.5) - 1
        py = (1 - sc[:, 1] / inz / scale) * (height * 0.5) - 1
        inside = (sc[:, 2] < 0) & (px >= -0.5) & (px < width - 1.5) & (py >= -0.5) & (py < height - 1.5)
        pixels.append(torch.stack([px, py], 1)); insides.append(inside)
        if visibility:
            dist = torch.linalg.norm(c, dim=1)
            rays = torch.cat([O, -c / dist[:, None]], 1).contiguous()
            tmax = torch.where(inside, dist, torch.full_like(dist, float("nan")))
            nbytes += rays.numel() * 4 + tmax.numel() * 4
            opens.append(inside & (s.occluded(rays, tmax) == 0))
    return torch.stack(pixels), torch.stack(insides), torch.stack(opens) if visibility else None, nbytes


def measure(a):
    import torch
    import rendering_amd as RA
    from rendering_amd import assets
    from tools.srchash import source_hash
    from tools.trace_rays_time import camera_rays, timed
    assets.ensure(); assets.ensure(["bumpy_250k.obj"])
    W = H = a.size
    s = RA.Scene("scenes/%s.scene" % SCENE, W, H)
    cam = camera_rays(s, W, H)
    first = s.surface_rays(cam, hits=True, position=True, normal=True, albedo=False)
    hit = first["hits"][:, 0] > 0
    points = torch.cat([first["position"], first["normal"]], 1)[hit].contiguous()
    del first, cam
    n = int(points.shape[0])
    rows = []
    for name, cams in (("K1_other_camera", [OTHER]), ("K6_cube_cameras", RA.cube_cameras(CUBE_AT))):
        table = s.camera_table(cams)
        for vis in (True, False):
            row = dict(scene=SCENE, size=a.size, case=name, n=n, n_cams=len(cams), visibility=vis)
            figures = {
                "a_project_points": lambda: s.project_points(points, table, visibility=vis),
                "c_composed": lambda: composed(s, points, table, vis),
            }
            runs = {key: [] for key in figures}
            for _ in range(a.runs):
                for key, fn in figures.items():
                    runs[key].append(timed(fn, a.reps)[0])
            for key, vals in runs.items():
                row[key + "_ms"] = dict(runs=vals, median=sorted(vals)[len(vals) // 2], range=max(vals) - min(vals))
            mine = s.project_points(points, table, visibility=vis)
            pixel, inside, is_open, nbytes = composed(s, points, table, vis)
            torch.cuda.synchronize()
            fl = mine["flags"]
            both = ((fl & RA.PROJ_INSIDE) != 0) & inside
            row["pairs"] = n * len(cams)
            row["pairs_inside"] = int(((fl & RA.PROJ_INSIDE) != 0).sum().item())
            row["pairs_open"] = int(((fl & RA.PROJ_OPEN) != 0).sum().item())
            row["composed_inside_differs"] = int((((fl & RA.PROJ_INSIDE) != 0) != inside).sum().item())
            row["composed_open_differs"] = int((((fl & RA.PROJ_OPEN) != 0) != is_open).sum().item()) if vis else None
            row["composed_max_pixel_deviation"] = float((pixel - mine["pixel"])[both].abs().max().item()) if bool(both.any()) else 0.0
            row["composed_ray_and_range_buffer_bytes"] = int(nbytes)
            aa, cc = row["a_project_points_ms"], row["c_composed_ms"]
            row["a_below_c_by_more_than_both_spreads"] = bool(max(aa["runs"]) < min(cc["runs"]) - (aa["range"] + cc["range"]))
            print(json.dumps(row), flush=True)
            rows.append(row)
    s.close()
    return dict(sources=source_hash(), reps=a.reps, runs=a.runs, rows=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "project_time.json"))
    a = ap.parse_args()
    out = measure(a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        json.dump(out, fo, indent=1)


if __name__ == "__main__":
    main()
