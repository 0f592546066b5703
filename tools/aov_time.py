#!/usr/bin/env python
"""Times the first-hit buffers of a frame (rtx_render_aov, Scene.render_aov) on the GPU against the other routes to the same data (one
JSON line per scene, all of them also written to --out, stamped with the kernel sources' hash, tools/srchash.py).  Per scene, 4096^2 by
default:
  (a) render_aov with depth + ids + uv only (no surface fetch);
  (b) render_aov with all six channels;
  (c) trace_rays(hits only) on tools/trace_rays_time.py's camera_rays of the same view, under the default knobs and with trace_reorder = 0
      -- what a caller without render_aov has to do for the data of (a), the ray buffer already built;
  (d) rtx_render_pass1 of the same view.
HIP events around each call after a warm-up call; median and minimum of --reps warm launches.

    python tools/aov_time.py [--size 4096] [--reps 10] [--out profiles/aov_time.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENES = ("cfg2_smooth_250k", "r6_knot_250k")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import rendering_amd as RA
    from rendering_amd import assets
    from tools.srchash import source_hash
    from tools.trace_rays_time import camera_rays, timed
    assets.ensure(); assets.ensure(["bumpy_250k.obj", "knot_250k.obj"])
    W = H = a.size
    rows = []
    for name in SCENES:
        s = RA.Scene("scenes/%s.scene" % name, W, H)
        dev = "cuda:0"
        f = lambda *tail: torch.zeros((H, W) + tail, dtype=torch.float32, device=dev)
        i = lambda: torch.zeros((H, W), dtype=torch.int32, device=dev)
        geo = dict(depth=f(), object_id=i(), triangle_id=i(), uv=f(2))
        surf = dict(normal=f(3), albedo=f(3))
        fb = f(3)
        row = dict(scene=name, width=W, height=H)
        row["pass1_ms"], row["pass1_min_ms"] = timed(lambda: s.render_pass1(fb), a.reps)
        row["aov_geometry_ms"], row["aov_geometry_min_ms"] = timed(lambda: s.render_aov(**geo), a.reps)
        row["aov_all_ms"], row["aov_all_min_ms"] = timed(lambda: s.render_aov(**geo, **surf), a.reps)
        row["hit_share"] = float((geo["object_id"][: H - 1, : W - 1] >= 0).float().mean().item())
        del surf, fb
        cam = camera_rays(s, W, H)
        for label, reorder in (("default", -1), ("as_given", 0)):
            s.set_knob("trace_reorder", reorder)
            row["trace_hits_%s_ms" % label], row["trace_hits_%s_min_ms" % label] = timed(lambda: s.trace_rays(cam, hits=True, colours=False), a.reps)
        s.set_knob("trace_reorder", -1)
        # (camera_rays restates the camera-ray arithmetic in torch, not bit for bit: the share of pass 1's pixels whose ids agree is a sanity
        # figure only -- tests/test_gpu_aov.py compares the two routes on identical rays, exactly)
        h, _ = s.trace_rays(cam, hits=True, colours=False)
        h = h.view(H, W, 8)[: H - 1, : W - 1]
        row["ids_agree_share"] = float(((h[..., 1].to(torch.int32) == geo["object_id"][: H - 1, : W - 1])
                                        & (h[..., 2].to(torch.int32) == geo["triangle_id"][: H - 1, : W - 1])).float().mean().item())
        row["trace_hits_best_ms"] = min(row["trace_hits_default_ms"], row["trace_hits_as_given_ms"])
        row["aov_geometry_faster_than_trace_hits"] = row["aov_geometry_ms"] < row["trace_hits_best_ms"]
        print(json.dumps(row), flush=True)
        rows.append(row)
        del cam, h, geo
        s.close()
        torch.cuda.empty_cache()
    out = dict(sources=source_hash(), reps=a.reps, rows=rows)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            json.dump(out, fo, indent=1)


if __name__ == "__main__":
    main()
