#!/usr/bin/env python
"""Times rtx_scatter_rays (Scene.scatter_rays) and Scene.cast_tree on the GPU against the routes a caller had before them (one JSON line per
scene and ray set, all of them also written to --out, stamped with the kernel sources' hash, tools/srchash.py).
Scenes cfg3_reflective_refractive (spheres) and mixed_materials (meshes) at 1024^2; ray sets: the camera rays, and their first-level children
(scatter_rays' reflection and refraction rays, compacted in parent order).  Per ray set:
  (a) scatter_rays, the five scatter channels: one walk, one light loop;
  (b) the route it replaces: surface_rays (hits, position, normal, albedo, specular) + light_rays (diffuse, specular) -- two walks --, then
      local, the child rays, the weights and the kinds built in torch (its fresnel, refract and normalisation are torch's: the figures of
      (b) are not bit for bit those of (a));
  (c) cast_tree to the scene's max_ray_depth against trace_rays with colours only, the fused recursion (cast_tree synchronises with the host
      once per level; both are timed with events around the whole call).
HIP events around each call after a warm-up call, the median of --reps warm launches; the figures are measured in turn, --runs times over
(alternated: a drift of the device shows as a spread within every figure, not as a difference between them).  Reported per figure: the
runs' medians, their middle value and their range; whether the worst run of (a) is below the best run of (b) by more than the larger of the
two ranges; the ratio (c) cast_tree / trace_rays.

    python tools/scatter_time.py [--reps 10] [--runs 3] [--size 1024] [--out profiles/scatter_time.json]
                                 [--light-rays PARENT.json THIS.json [--keep]]

--light-rays: two outputs of tools/light_rays_time.py, of the parent's build and of this one (rtxRayLightKernel shares its light loop with
rtxRayScatterKernel): both are written into --out with, per figure of rtx_light_rays, whether this build's median lies within the parent's
own run-to-run range of the parent's median (--keep: --out's own figures stay as they are).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENES = ("cfg3_reflective_refractive", "mixed_materials")
BIAS = 0.0001          # Options::bias, which no scene file sets


def composed(s, rays, consts):
    """(b): the channels of include/rtx_scatter.h on the caller's side.  Returns (local, reflect, refract, weight, kinds)."""
    import torch
    material, ambient, kd, iors = consts
    out = s.surface_rays(rays, hits=True, position=True, normal=True, albedo=True, specular=True)
    light = s.light_rays(rays)
    hits, P, N, albedo, ks = out["hits"], out["position"], out["normal"], out["albedo"], out["specular"]
    D, S = light["diffuse"], light["specular"]
    hit = hits[:, 0] > 0
    obj = hits[:, 1].clamp(min=0).long()
    mat = torch.where(hit, material[obj], torch.full_like(obj, -1))
    d = rays[:, 3:6]
    B = N * BIAS
    dn = (d * N).sum(1)
    R = d - N * (2 * dn)[:, None]
    # fresnel and refract (scene.cpp:677-722)
    ior = iors[obj]
    cosi = dn.clamp(-1, 1)
    inside = cosi > 0
    one = torch.ones_like(ior)
    n1, n2 = torch.where(inside, ior, one), torch.where(inside, one, ior)
    ac = cosi.abs()
    sint = n1 / n2 * (1 - cosi * cosi).clamp(min=0).sqrt()
    cost = (1 - sint * sint).clamp(min=0).sqrt()
    rs = (n2 * ac - n1 * cost) / (n2 * ac + n1 * cost)
    rp = (n1 * ac - n2 * cost) / (n1 * ac + n2 * cost)
    kr = torch.where(sint >= 1, one, (rs * rs + rp * rp) / 2)
    eta = n1 / n2
    k = 1 - eta * eta * (1 - ac * ac)
    T = d * eta[:, None] + torch.where(inside[:, None], -N, N) * (eta * ac - k.clamp(min=0).sqrt())[:, None]
    norm = lambda v: v / v.norm(dim=1, keepdim=True)
    mirror, glass = mat == 1, mat == 2
    both = glass & (kr < 1)
    outside = (dn < 0)[:, None]
    zero3 = torch.zeros_like(P)
    local = torch.where((mat == 0)[:, None], albedo * D, albedo)
    local = torch.where((mat == 3)[:, None], albedo * ambient[obj][:, None] + D * kd[obj][:, None] + S * ks[:, None], local)
    local = torch.where(mirror[:, None], S, local)
    local = torch.where(glass[:, None], S * kr[:, None], local)
    fo = torch.where(mirror[:, None] | (glass[:, None] & outside), P + B, P - B)
    reflect = torch.where((mirror | glass)[:, None], torch.cat([fo, torch.where(mirror[:, None], R, norm(R))], 1), torch.cat([zero3, zero3], 1))
    refract = torch.where(both[:, None], torch.cat([torch.where(outside, P - B, P + B), norm(T)], 1), torch.cat([zero3, zero3], 1))
    zero = torch.zeros_like(kr)
    weight = torch.stack([torch.where(mirror, torch.full_like(kr, 0.8), torch.where(glass, kr, zero)), torch.where(both, 1 - kr, zero)], 1)
    kinds = (mirror | glass).to(torch.uint8) + 2 * both.to(torch.uint8)
    return local, reflect, refract, weight, kinds


def first_children(s, rays):
    import torch
    out = s.scatter_rays(rays, local=False, weight=False)
    m = rays.shape[0]
    both = torch.stack([out["refract"], out["reflect"]], 1).reshape(2 * m, 6)
    exists = torch.stack([(out["kinds"] & 2) != 0, (out["kinds"] & 1) != 0], 1).reshape(2 * m)
    return both[exists].contiguous()


def measure(a):
    import numpy as np
    import torch
    import rendering_amd as RA
    from rendering_amd import assets
    from tools.srchash import source_hash
    from tools.trace_rays_time import camera_rays, timed
    assets.ensure()
    dev = "cuda:0"
    W = H = a.size
    rows = []
    for scene in SCENES:
        s = RA.Scene("scenes/%s.scene" % scene, W, H)
        objs, _ = s.device_objects()
        t = lambda v, dt: torch.from_numpy(np.ascontiguousarray(v)).to(dev).to(dt)
        consts = (t(objs["material"], torch.int64), t(objs["ambient"], torch.float32), t(objs["diffuse"], torch.float32), t(objs["ior"], torch.float32))
        cam = camera_rays(s, W, H)
        for name, rays in (("camera", cam), ("children", first_children(s, cam))):
            n = int(rays.shape[0])
            row = dict(scene=scene, size=a.size, rays=name, n=n, n_lights=s.n_lights, max_ray_depth=s.max_ray_depth)
            figures = {
                "a_scatter": lambda: s.scatter_rays(rays),
                "b_composed": lambda: composed(s, rays, consts),
                "c_cast_tree": lambda: s.cast_tree(rays),
                "trace_colours": lambda: s.trace_rays(rays, hits=False),
            }
            runs = {key: [] for key in figures}
            for _ in range(a.runs):
                for key, fn in figures.items():
                    runs[key].append(timed(fn, a.reps)[0])
            for key, vals in runs.items():
                row[key + "_ms"] = dict(runs=vals, median=sorted(vals)[len(vals) // 2], range=max(vals) - min(vals))
            mine = s.scatter_rays(rays)
            theirs = composed(s, rays, consts)
            _, levels = s.cast_tree(rays)
            torch.cuda.synchronize()
            # (sanity figures only: tests/test_gpu_scatter.py compares exactly)
            row["composed_kinds_differ"] = int((mine["kinds"] != theirs[4]).sum().item())
            row["composed_local_max_abs_difference"] = float((mine["local"] - theirs[0]).abs().max().item())
            row["kinds"] = [int((mine["kinds"] == k).sum().item()) for k in (0, 1, 3)]
            row["cast_tree_levels"] = [int(lv["rays"].shape[0]) for lv in levels]
            fa, fb = row["a_scatter_ms"], row["b_composed_ms"]
            row["a_below_b_by_more_than_the_spread"] = bool(max(fa["runs"]) < min(fb["runs"]) - max(fa["range"], fb["range"]))
            row["b_over_a"] = fb["median"] / fa["median"]
            row["cast_tree_over_trace_rays"] = row["c_cast_tree_ms"]["median"] / row["trace_colours_ms"]["median"]
            print(json.dumps(row), flush=True)
            rows.append(row)
        s.close()
        torch.cuda.empty_cache()
    return dict(sources=source_hash(), reps=a.reps, runs=a.runs, rows=rows)


def light_rays_verdict(parent_path, this_path):
    """Both outputs of tools/light_rays_time.py and, per ray set and figure of rtx_light_rays, this build's median against the parent's own range."""
    parent, this = json.load(open(parent_path)), json.load(open(this_path))
    verdict = []
    for p, t in zip(parent["rows"], this["rows"]):
        assert (p["rays"], p["n"]) == (t["rays"], t["n"])
        for key in ("a_sums_ms", "b_per_light_ms"):
            verdict.append(dict(rays=p["rays"], figure=key, parent_median=p[key]["median"], parent_range=p[key]["range"], this_median=t[key]["median"],
                                this_range=t[key]["range"], within_the_parents_range=bool(abs(t[key]["median"] - p[key]["median"]) <= p[key]["range"])))
    return dict(parent=parent, this=this, verdict=verdict)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scatter_time.json"))
    ap.add_argument("--light-rays", nargs=2, default=None, metavar=("PARENT.json", "THIS.json"))
    ap.add_argument("--keep", action="store_true", help="measure nothing: add --light-rays to the figures --out already holds")
    a = ap.parse_args()
    out = json.load(open(a.out)) if a.keep else measure(a)
    if a.light_rays:
        out["light_rays_time"] = light_rays_verdict(*a.light_rays)
        for v in out["light_rays_time"]["verdict"]:
            print(json.dumps(v), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        json.dump(out, fo, indent=1)


if __name__ == "__main__":
    main()
