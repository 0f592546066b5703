#!/usr/bin/env python
"""Times rtx_occluded_rays (Scene.occluded) on the GPU on scenes/cfg2_smooth_250k.scene next to its yardstick, rtx_trace_rays with
hits only, on the same rays in the same process (one JSON line per workload, all of them written to --out, stamped with the kernel
sources' hash).  Workloads, as tools/trace_rays_time.py builds them:
  (a) the size^2 camera rays of the view, in pixel order;   (b) the same rays under a seeded permutation;
  (c) the hit points of (a), each with a seeded uniform direction, the whole ray;
  (d) 4M rays drawn like tests/util_rays.probe_rays, and their first 1M / 262k / 64k;
  (e) (c)'s origins aimed at the scene's point lights in turn, the range the light's distance: true shadow rays;
  (f) (c) with the range 0.5: ambient occlusion.
Per workload, for both calls: the rays as handed over (knob trace_reorder = 0), always grouped by key (1) and the default rule (-1);
for occluded also the objects in scene order (knob occluded_scene_order = 1) under the default rule.  The scene lists its plane before
its mesh, so (c), (e) and (f) are timed once more in a copy of the scene with the two blocks swapped (written to output/): there the
scene order sends every ray through the mesh first.  HIP events around each call after a warm-up call; median and minimum of --reps.

    python tools/occluded_rays_time.py [--size 4096] [--reps 5] [--out profiles/occluded_rays_time.json]
    python tools/occluded_rays_time.py --merge run1.json run2.json run3.json --out profiles/occluded_rays_time.json
--merge: the first run's rows plus, per workload, the medians of the yardstick in every run and their range (the run-to-run spread
a difference between the two calls has to exceed to mean anything).
"""
import argparse
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.trace_rays_time import SCENE, camera_rays, probe_like, timed      # noqa: E402

COLUMNS = (("as_given", 0), ("grouped", 1), ("default", -1))


def point_lights(path):
    text = open(os.path.join(ROOT, path)).read()
    out = []
    for b in re.split(r"(?m)^(?=\[)", text):
        if b.startswith("[light]") and re.search(r"(?m)^type\s*=\s*point", b):
            out.append([float(v) for v in re.search(r"(?m)^position\s*=\s*(\S+)", b).group(1).split(",")])
    return out


def mesh_first_copy(path):
    """The scene with its [object] blocks in reverse order (the mesh before the plane), written to output/."""
    blocks = re.split(r"(?m)^(?=\[)", open(os.path.join(ROOT, path)).read())
    idx = [i for i, b in enumerate(blocks) if b.startswith("[object]")]
    objs = [blocks[i] for i in idx][::-1]
    for i, b in zip(idx, objs):
        blocks[i] = b
    out = os.path.join("output", os.path.basename(path).replace(".scene", "_mesh_first.scene"))
    os.makedirs(os.path.join(ROOT, "output"), exist_ok=True)
    with open(os.path.join(ROOT, out), "w") as f:
        f.write("".join(blocks))
    return out


def measure(s, rays, tmax, reps, yardstick=True):
    row = {}
    for label, reorder in COLUMNS:
        s.set_knob("trace_reorder", reorder)
        row["occluded_%s_ms" % label], row["occluded_%s_min_ms" % label] = timed(lambda: s.occluded(rays, tmax), reps)
        if yardstick:
            row["hits_%s_ms" % label], row["hits_%s_min_ms" % label] = timed(lambda: s.trace_rays(rays, hits=True, colours=False), reps)
    s.set_knob("occluded_scene_order", 1)
    row["occluded_scene_order_default_ms"], row["occluded_scene_order_default_min_ms"] = timed(lambda: s.occluded(rays, tmax), reps)
    s.set_knob("occluded_scene_order", 0)
    if yardstick:
        row["ratio_hits_over_occluded_default"] = row["hits_default_ms"] / row["occluded_default_ms"]
    return row


def merge(paths, out):
    runs = [json.load(open(p)) for p in paths]
    res = runs[0]
    for row in res["rows"]:
        meds = [r2["hits_default_ms"] for run in runs for r2 in run["rows"] if r2["workload"] == row["workload"] and "hits_default_ms" in r2]
        occ = [r2["occluded_default_ms"] for run in runs for r2 in run["rows"] if r2["workload"] == row["workload"]]
        if meds:
            row["hits_default_ms_runs"] = meds
            row["hits_default_ms_range"] = max(meds) - min(meds)
        row["occluded_default_ms_runs"] = occ
    res["runs"] = len(runs)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    for row in res["rows"]:
        print(json.dumps(row))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--probe-rays", type=int, default=4 << 20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--merge", nargs="+", default=None)
    a = ap.parse_args()
    if a.merge:
        return merge(a.merge, a.out)
    import torch
    import rendering_amd as RA
    from rendering_amd import assets
    from tools.srchash import source_hash
    assets.ensure(); assets.ensure(["bumpy_250k.obj"])
    W = H = a.size
    path = "scenes/%s.scene" % SCENE
    s = RA.Scene(path, W, H)
    cam = camera_rays(s, W, H)
    gen = torch.Generator(device="cuda:0"); gen.manual_seed(1234)
    perm = torch.randperm(cam.shape[0], device="cuda:0", generator=gen)
    h, _ = s.trace_rays(cam, hits=True, colours=False)
    hit = h[:, 0] > 0
    sec = torch.empty((int(hit.sum().item()), 6), dtype=torch.float32, device="cuda:0")
    sec[:, 0:3] = cam[hit, 0:3] + cam[hit, 3:6] * h[hit, 3:4]
    u = torch.randn((sec.shape[0], 3), device="cuda:0", generator=gen)
    sec[:, 3:6] = u / torch.linalg.norm(u, dim=1, keepdim=True)
    lights = torch.tensor(point_lights(path), dtype=torch.float32, device="cuda:0")
    to = lights[torch.arange(sec.shape[0], device="cuda:0") % lights.shape[0]] - sec[:, 0:3]
    dist = torch.linalg.norm(to, dim=1)
    shadow = torch.cat([sec[:, 0:3], to / dist[:, None]], 1).contiguous()
    probe = torch.from_numpy(probe_like(a.probe_rays, 77)).cuda()
    ao = torch.full((sec.shape[0],), 0.5, dtype=torch.float32, device="cuda:0")
    workloads = [("a_camera_pixel_order", cam, None), ("b_camera_permuted", cam[perm].contiguous(), None), ("c_surface_uniform", sec, None),
                 ("d_probe_like", probe, None)]
    for n in (1 << 20, 262144, 65536):
        workloads.append(("d_probe_like_%d" % n, probe[:n].contiguous(), None))
    workloads += [("e_shadow_rays_to_point_lights", shadow, dist.contiguous()), ("f_ambient_occlusion_0.5", sec, ao)]
    del h, hit, u, to
    torch.cuda.synchronize()
    rows = []
    stamp = dict(scene=SCENE, width=W, height=H, sources=source_hash())
    for wname, rays, tmax in workloads:
        row = dict(workload=wname, n=int(rays.shape[0]))
        reps = a.reps if rays.shape[0] >= (1 << 20) else 4 * a.reps      # (short calls: more of them)
        row["occluded_share"] = float(s.occluded(rays, tmax).float().mean().item())
        row.update(measure(s, rays, tmax, reps))
        print(json.dumps(row), flush=True)
        rows.append(row)
    s.close()
    # the same scene with the mesh listed before the plane: what the analytic-objects-first order is for
    s2 = RA.Scene(mesh_first_copy(path), W, H)
    for wname, rays, tmax in workloads:
        if wname[0] not in "cef":
            continue
        row = dict(workload=wname + "_mesh_listed_first", n=int(rays.shape[0]))
        row.update(measure(s2, rays, tmax, a.reps, yardstick=False))
        print(json.dumps(row), flush=True)
        rows.append(row)
    s2.close()
    out = dict(stamp, rows=rows)
    print(json.dumps(stamp), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
