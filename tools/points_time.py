#!/usr/bin/env python
"""Times direct light and ambient occlusion at caller-supplied surface points (rtx_light_points / rtx_ao_points, Scene.light_points /
Scene.ao_points) on the GPU against the routes a caller had before them (one JSON line per point set, all of them also written to --out,
stamped with the kernel sources' hash, tools/srchash.py).  Scene cfg2_smooth_250k; point sets: the first hits of the size^2 camera rays
({P, N} from surface_rays, V the ray's direction, ns the hit object's), and the triangle corners of the mesh with their vertex normals
(Scene.bvh(i)["tris"] of a fresh scene: 30 floats per triangle, corners a b c, then normals n_a n_b n_c; V = -N, ns = 5).  Per point set:
  (a) light_points, the two sums only;
  (b) light_points with per_light (sums, each light's terms, light_open);
  (c) the composed route on the older calls: per light illuminate restated in torch, an n x 6 ray buffer and an n-float range buffer,
      occluded(), and the Phong arithmetic in torch (its pow is not the reference's: the figures of (c) are not bit for bit those of (a));
  (d) light_rays on the rays that produced the points (camera set only);
  ao_points with 16 directions (counts and ao), against occluded() on the same traced rays built beforehand (the buffer is not timed),
      and against render_ao of the frame (camera set only).
HIP events around each call after a warm-up call, the median of --reps warm launches; the figures are measured in turn, --runs times over
(alternated: a drift of the device shows as a spread within every figure, not as a difference between them).  Reported per figure: the
runs' medians, their middle value and their range, and whether the worst run of (a) is below the best run of (c) by more than the two
ranges together.

    python tools/points_time.py [--reps 10] [--runs 3] [--size 1024] [--out profiles/points_time.json]
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENE = "cfg2_smooth_250k"
BIAS = 0.0001          # Options::bias, which no scene file sets
N_DIRS = 16


def composed(s, points, view, lights):
    """(c): the two sums of the contract of include/rtx_points.h on the caller's side, point and distant lights.  Returns (diffuse,
    specular, bytes of shadow-ray and range buffers allocated)."""
    import torch
    P, N = points[:, 0:3], points[:, 3:6]
    nd, ns = -view[:, 0:3], view[:, 3]
    O = P + N * BIAS
    diffuse = torch.zeros_like(P); specular = torch.zeros_like(P)
    nbytes = 0
    for kind, color, intensity, direction, pos in lights:
        if kind == 1:
            L = direction.expand_as(P)
            I = (color * intensity).expand_as(P)
            dist = torch.full((P.shape[0],), torch.finfo(torch.float32).max, dtype=torch.float32, device=P.device)
        else:
            Lv = P - pos
            l2 = (Lv * Lv).sum(1)
            att = (float(intensity) / (4 * math.pi * l2.double() / 1000)).float().clamp(max=1.0)
            I = color[None, :] * att[:, None]
            dist = l2.sqrt()
            L = Lv / dist[:, None]
        shadow = torch.cat([O, -L], 1).contiguous()
        nbytes += shadow.numel() * 4 + dist.numel() * 4
        vis = (s.occluded(shadow, dist) == 0).float()[:, None]
        m = (N * -L).sum(1).clamp(min=0)[:, None]
        R = L - N * (2 * (L * N).sum(1))[:, None]
        sd = (R * nd).sum(1).clamp(min=0)
        diffuse = diffuse + vis * I * m
        specular = specular + vis * I * torch.pow(sd, ns)[:, None]
    return diffuse, specular, nbytes


def measure(a):
    import numpy as np
    import torch
    import rendering_amd as RA
    from rendering_amd import assets
    from tools.srchash import source_hash
    from tools.trace_rays_time import camera_rays, timed
    assets.ensure(); assets.ensure(["bumpy_250k.obj"])
    dev = "cuda:0"
    W = H = a.size
    s = RA.Scene("scenes/%s.scene" % SCENE, W, H)
    # the triangle corners of the meshes, read before the scene is uploaded
    corners = []
    for k in range(s.n_objects):
        b = s.bvh(k)              # (None: not a mesh)
        if b is not None and b["n_tris"]:
            tr = b["tris"]
            corners.append(np.concatenate([tr[:, 0:9].reshape(-1, 3), tr[:, 9:18].reshape(-1, 3)], 1))
    corners = np.ascontiguousarray(np.concatenate(corners), np.float32)
    recs, _ = s.device_lights()
    assert all(r["type"] in (1, 2) for r in recs), "the composed route restates point and distant lights only"
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(dev)
    lights = [(int(r["type"]), t(r["color"]), float(r["intensity"]), t(r["dir"]), t(r["pos"])) for r in recs]
    objs, _ = s.device_objects()
    n_specular = t(objs["n_specular"])
    cam = camera_rays(s, W, H)
    first = s.surface_rays(cam, hits=True, position=True, normal=True, albedo=False)
    hit = first["hits"][:, 0] > 0
    cam_hit = cam[hit].contiguous()
    cam_points = torch.cat([first["position"], first["normal"]], 1)[hit].contiguous()
    cam_view = torch.cat([cam[:, 3:6], n_specular[first["hits"][:, 1].clamp(min=0).long()][:, None]], 1)[hit].contiguous()
    tri_points = t(corners)
    tri_view = torch.cat([-tri_points[:, 3:6], torch.full((tri_points.shape[0], 1), 5.0, device=dev)], 1).contiguous()
    dirs = torch.from_numpy(RA.sphere_directions(N_DIRS)).to(dev)
    ao_img = torch.zeros((H, W), dtype=torch.float32, device=dev)
    counts_img = torch.zeros((H, W), dtype=torch.int32, device=dev)
    rows = []
    for name, points, view, rays in (("camera_hits", cam_points, cam_view, cam_hit), ("triangle_corners", tri_points, tri_view, None)):
        n = int(points.shape[0])
        row = dict(scene=SCENE, size=a.size, points=name, n=n, n_lights=len(lights), n_dirs=N_DIRS)
        # the AO rays of the older route, built beforehand: {O, d_k} for every (point, direction) with N . d_k > 0
        traced = (points[:, 3:6] @ dirs.t()) > 0
        pt, kk = traced.nonzero(as_tuple=True)
        ao_rays = torch.cat([(points[:, 0:3] + points[:, 3:6] * BIAS)[pt], dirs[kk]], 1).contiguous()
        row["ao_traced_rays"] = int(ao_rays.shape[0])
        figures = {
            "a_sums": lambda: s.light_points(points, view),
            "b_per_light": lambda: s.light_points(points, view, per_light=True),
            "c_composed": lambda: composed(s, points, view, lights),
            "ao_points": lambda: s.ao_points(points, dirs, counts=True),
            "ao_occluded_prebuilt": lambda: s.occluded(ao_rays),
        }
        if rays is not None:
            figures["d_light_rays"] = lambda: s.light_rays(rays)
            figures["ao_render_ao"] = lambda: s.render_ao(dirs, ao=ao_img, counts=counts_img)
        runs = {key: [] for key in figures}
        for _ in range(a.runs):
            for key, fn in figures.items():
                runs[key].append(timed(fn, a.reps)[0])
        for key, vals in runs.items():
            row[key + "_ms"] = dict(runs=vals, median=sorted(vals)[len(vals) // 2], range=max(vals) - min(vals))
        d, sp, nbytes = composed(s, points, view, lights)
        mine = s.light_points(points, view)
        torch.cuda.synchronize()
        # (a sanity figure only: the composed route's pow and normalisation are torch's -- tests/test_gpu_points.py compares exactly)
        row["composed_max_abs_difference"] = float(max((d - mine["diffuse"]).abs().max().item(), (sp - mine["specular"]).abs().max().item()))
        row["composed_ray_buffer_bytes"] = int(nbytes)
        # ... and of the AO: open rays of the older route against ao_points' counts
        occ = s.occluded(ao_rays)
        counts = s.ao_points(points, dirs, ao=False, counts=True)["counts"]
        torch.cuda.synchronize()
        row["ao_open_rays"] = [int((occ == 0).sum().item()), int((counts & 0xFFFF).sum().item())]
        aa, cc = row["a_sums_ms"], row["c_composed_ms"]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "points_time.json"))
    a = ap.parse_args()
    out = measure(a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        json.dump(out, fo, indent=1)


if __name__ == "__main__":
    main()
