#!/usr/bin/env python
"""Times the direct light at the hits of caller-supplied rays (rtx_light_rays, Scene.light_rays) on the GPU against the route a caller
had before it (one JSON line per ray set, all of them also written to --out, stamped with the kernel sources' hash, tools/srchash.py).
Scene cfg2_smooth_250k at 1024^2; ray sets: the camera rays, and one bounce ray per first hit (the first of sphere_directions(12) on the
side of the normal, from P + N bias).  Per ray set:
  (a) light_rays, the two sums only;
  (b) light_rays with per_light (sums, each light's terms, light_open);
  (c) the composed route: surface_rays (hits, position, normal), then per light illuminate restated in torch, an n x 6 ray buffer and an
      n-float range buffer, occluded(), and the Phong arithmetic in torch (its pow is not the reference's: the figures of (c) are not bit
      for bit those of (a)); everything between the rays and the two sums is timed;
  trace_rays with colours only, for orientation.
HIP events around each call after a warm-up call, the median of --reps warm launches; the four are measured in turn, --runs times over
(alternated: a drift of the device shows as a spread within every figure, not as a difference between them).  Reported per figure: the
runs' medians, their middle value and their range, the bytes of ray and range buffers (c) allocates, and whether the worst run of (a) is
below the best run of (c) by more than (c)'s range.

    python tools/light_rays_time.py [--reps 10] [--runs 3] [--size 1024] [--out profiles/light_rays_time.json]
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


def composed(s, rays, lights, n_specular):
    """(c): the two sums of the contract of include/rtx_light.h on the caller's side, point and distant lights.  Returns (diffuse,
    specular, bytes of shadow-ray and range buffers allocated)."""
    import torch
    out = s.surface_rays(rays, hits=True, position=True, normal=True, albedo=False)
    hits, P, N = out["hits"], out["position"], out["normal"]
    hit = hits[:, 0] > 0
    ns = n_specular[hits[:, 1].clamp(min=0).long()]
    O = P + N * BIAS
    nd = -rays[:, 3:6]
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
        vis = ((s.occluded(shadow, dist) == 0) & hit).float()[:, None]
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
    recs, _ = s.device_lights()
    assert all(r["type"] in (1, 2) for r in recs), "the composed route restates point and distant lights only"
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(dev)
    lights = [(int(r["type"]), t(r["color"]), float(r["intensity"]), t(r["dir"]), t(r["pos"])) for r in recs]
    objs, _ = s.device_objects()
    n_specular = t(objs["n_specular"])
    cam = camera_rays(s, W, H)
    first = s.surface_rays(cam, hits=True, position=True, normal=True, albedo=False)
    hit = first["hits"][:, 0] > 0
    dirs = torch.from_numpy(RA.sphere_directions(12)).to(dev)
    k = ((first["normal"] @ dirs.t()) > 0).float().argmax(1)
    bounce = torch.cat([first["position"] + first["normal"] * BIAS, dirs[k]], 1)[hit].contiguous()
    rows = []
    for name, rays in (("camera", cam), ("bounce", bounce)):
        n = int(rays.shape[0])
        row = dict(scene=SCENE, size=a.size, rays=name, n=n, n_lights=len(lights))
        figures = {
            "a_sums": lambda: s.light_rays(rays),
            "b_per_light": lambda: s.light_rays(rays, per_light=True),
            "c_composed": lambda: composed(s, rays, lights, n_specular),
            "trace_colours": lambda: s.trace_rays(rays, hits=False),
        }
        runs = {key: [] for key in figures}
        for _ in range(a.runs):
            for key, fn in figures.items():
                runs[key].append(timed(fn, a.reps)[0])
        for key, vals in runs.items():
            row[key + "_ms"] = dict(runs=vals, median=sorted(vals)[len(vals) // 2], range=max(vals) - min(vals))
        d, sp, nbytes = composed(s, rays, lights, n_specular)
        mine = s.light_rays(rays)
        torch.cuda.synchronize()
        # (a sanity figure only: the composed route's pow and normalisation are torch's -- tests/test_gpu_light_rays.py compares exactly)
        row["composed_max_abs_difference"] = float(max((d - mine["diffuse"]).abs().max().item(), (sp - mine["specular"]).abs().max().item()))
        row["composed_ray_buffer_bytes"] = int(nbytes)
        row["hit_share"] = float((s.light_rays(rays, diffuse=False, specular=False, hits=True)["hits"][:, 0] > 0).float().mean().item())
        c = row["c_composed_ms"]
        row["a_below_c_by_more_than_the_spread"] = bool(max(row["a_sums_ms"]["runs"]) < min(c["runs"]) - c["range"])
        print(json.dumps(row), flush=True)
        rows.append(row)
    s.close()
    return dict(sources=source_hash(), reps=a.reps, runs=a.runs, rows=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "light_rays_time.json"))
    a = ap.parse_args()
    out = measure(a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        json.dump(out, fo, indent=1)


if __name__ == "__main__":
    main()
