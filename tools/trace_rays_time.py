#!/usr/bin/env python
"""Times rtx_trace_rays (Scene.trace_rays) on the GPU on scenes/cfg2_smooth_250k.scene (one JSON line per measurement, all of them
also written to --out, stamped with the kernel sources' hash, tools/srchash.py).  Workloads:
  (a) the size^2 camera rays of the view, in pixel order (the rays of pass 1: Camera::getRay of every pixel centre);
  (b) the same rays under a seeded permutation;
  (c) incoherent secondary rays: the hit points of (a), each with a seeded uniform direction;
  (d) 4M rays drawn like tests/util_rays.probe_rays (seeded numpy), and prefixes of them of 4k .. 1M rays (where grouping starts to pay).
Per workload the three output modes (colours, hits, both), each with the rays as handed over (knob trace_reorder = 0), always grouped by
key (1), the key's interleave starting with the direction or with the origin (knob trace_key_origin_first), and with the defaults
(trace_reorder = -1: by the number of rays and the coherence of the caller's order; origin first).  HIP events around each call
after a warm-up call; median and minimum of --reps.  pass 1 of the same view is timed for comparison with (a).

    python tools/trace_rays_time.py [--size 4096] [--reps 5] [--out profiles/trace_rays_time.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENE = "cfg2_smooth_250k"
MODES = {"colours": (False, True), "hits": (True, False), "both": (True, True)}


def timed(fn, reps):
    import torch
    fn(); torch.cuda.synchronize()       # warm
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms))


def camera_rays(s, W, H):
    """(a): pass 1's primary ray of every pixel (x + 0.5 twice: renderWorker and getPixels), row by row -- rtx_kernels.hip primaryRay."""
    import torch
    scale, aspect, m, pos = s.camera()
    dev = "cuda:0"
    y, x = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    xp = (2 * (x + 0.5 + 0.5) / W - 1) * float(scale) * float(aspect)
    yp = -(2 * (y + 0.5 + 0.5) / H - 1) * float(scale)
    d = torch.stack([xp, yp, -torch.ones_like(xp)], -1).reshape(-1, 3)
    d = d / torch.linalg.norm(d, dim=1, keepdim=True)
    M = torch.from_numpy(m.reshape(4, 4)).to(dev)
    r = d @ M[:3, :3] + M[3, :3]
    rays = torch.empty((W * H, 6), dtype=torch.float32, device=dev)
    rays[:, 0:3] = torch.from_numpy(pos).to(dev)
    rays[:, 3:6] = r
    return rays.contiguous()


def probe_like(n, seed):
    """(d): tests/util_rays.probe_rays' distribution, drawn with a seeded numpy generator (its PCG32 loop is too slow for millions)."""
    rng = np.random.default_rng(seed)
    u = rng.random((n, 6))
    rays = np.zeros((n, 6), np.float32)
    rays[:, 0:3] = (u[:, 0:3] - 0.5).astype(np.float32)
    tgt = (u[:, 3:6] - 0.5) * np.array([6.0, 4.0, 4.0]) + np.array([0.0, 0.0, -4.0])
    d = tgt - rays[:, 0:3]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays[:, 3:6] = d.astype(np.float32)
    k = n // 4
    rays[:k:4, 3] = 0.0
    rays[1:k:4, 4] = 0.0
    rays[2:k:4, 3:6] = np.array([0.0, 0.0, -1.0], np.float32)
    rays[3:k:4, 4] = np.float32(1e-7)
    return rays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--probe-rays", type=int, default=4 << 20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import rendering_amd as RA
    from rendering_amd import assets
    from tools.srchash import source_hash
    assets.ensure(); assets.ensure(["bumpy_250k.obj"])
    W = H = a.size
    s = RA.Scene("scenes/%s.scene" % SCENE, W, H)
    fb = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0")
    p1_med, p1_min = timed(lambda: s.render_pass1(fb), a.reps)
    cam = camera_rays(s, W, H)
    gen = torch.Generator(device="cuda:0"); gen.manual_seed(1234)
    perm = torch.randperm(cam.shape[0], device="cuda:0", generator=gen)
    h, _ = s.trace_rays(cam, hits=True, colours=False)
    hit = h[:, 0] > 0
    sec = torch.empty((int(hit.sum().item()), 6), dtype=torch.float32, device="cuda:0")
    sec[:, 0:3] = cam[hit, 0:3] + cam[hit, 3:6] * h[hit, 3:4]
    u = torch.randn((sec.shape[0], 3), device="cuda:0", generator=gen)
    sec[:, 3:6] = u / torch.linalg.norm(u, dim=1, keepdim=True)
    probe = torch.from_numpy(probe_like(a.probe_rays, 77)).cuda()
    workloads = [("a_camera_pixel_order", cam), ("b_camera_permuted", cam[perm].contiguous()), ("c_secondary_uniform", sec.contiguous()),
                 ("d_probe_like", probe)]
    for n in (4096, 16384, 65536, 262144, 1 << 20):
        workloads.append(("d_probe_like_%d" % n, probe[:n].contiguous()))
    del h, hit, u
    torch.cuda.synchronize()
    rows = []
    stamp = dict(scene=SCENE, width=W, height=H, sources=source_hash(), pass1_ms=p1_med, pass1_min_ms=p1_min)
    for wname, rays in workloads:
        row = dict(workload=wname, n=int(rays.shape[0]))
        reps = a.reps if rays.shape[0] >= (1 << 20) else 4 * a.reps      # (short calls: more of them)
        for mname, (hits, colours) in MODES.items():
            if wname.startswith("d_probe_like_") and mname == "both":
                continue
            for label, reorder, origin_first in (("as_given", 0, 0), ("grouped_dir_first", 1, 0), ("grouped_origin_first", 1, 1)):
                s.set_knob("trace_reorder", reorder)
                s.set_knob("trace_key_origin_first", origin_first)
                med, mn = timed(lambda: s.trace_rays(rays, hits=hits, colours=colours), reps)
                row["%s_%s_ms" % (mname, label)] = med
                row["%s_%s_min_ms" % (mname, label)] = mn
        # the defaults (trace_reorder -1: grouped from kReorderMin rays on, unless the rays already come in coherent groups;
        # trace_key_origin_first 1), every output mode
        s.set_knob("trace_reorder", -1); s.set_knob("trace_key_origin_first", 1)
        for mname, (hits, colours) in MODES.items():
            med, mn = timed(lambda: s.trace_rays(rays, hits=hits, colours=colours), reps)
            row["%s_default_ms" % mname] = med
            row["%s_default_min_ms" % mname] = mn
        row["grays_per_s_both_default"] = row["n"] / (row["both_default_ms"] * 1e-3) / 1e9
        print(json.dumps(row), flush=True)
        rows.append(row)
    s.close()
    out = dict(stamp, rows=rows)
    print(json.dumps(stamp), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
