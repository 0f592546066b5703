#!/usr/bin/env python
"""Times the two debug views on the GPU (one JSON line per measurement, also written to --out):
  * the showAC heat map (rtx_render_ac: count + normalise) against pass 1 of the same view (rtx_render_pass1), 4096^2 by default;
  * the showNormals frame (rtx_render_frame with RTX_FLAG_SHOW_NORMALS: three launches) against the ordinary frame;
  * the reference's serial heat map (oracle/_ref/render_ref, its own "Total time" timer) at a small size on this host, scaled by pixels.

    python tools/debug_view_time.py [--size 4096] [--reps 10] [--out profiles/debug_views_time.json]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps):
    import torch
    fn(); torch.cuda.synchronize()       # warm
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms))


def reference_serial(name, w, h):
    """Wall time of the reference's heat-map loop (its Timer "Total time" around Scene::render) at w x h, in ms."""
    from tests.ac_heatmap import scene_copy
    exe = os.path.join(ROOT, "oracle", "_ref", "render_ref")
    if not os.path.exists(exe):
        return None
    with tempfile.TemporaryDirectory() as tmp:
        path = scene_copy(name, tmp, dict(showAC=1, width=w, height=h, image_name=os.path.join(tmp, "heat")))
        r = subprocess.run([exe, path], cwd=ROOT, capture_output=True, text=True, timeout=900)
    m = re.search(r"Total time\s+(\d+) ms", r.stdout)
    return float(m.group(1)) if m else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--ref-size", type=int, default=512)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import rendering_amd as RA
    from rendering_amd import assets
    assets.ensure(); assets.ensure(["bumpy_250k.obj", "knot_250k.obj"])
    rows = []
    W = H = a.size
    for name in ("cfg2_smooth_250k", "r6_knot_250k"):
        s = RA.Scene("scenes/%s.scene" % name, W, H)
        fb = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0")
        mask = torch.zeros((H, W), dtype=torch.uint8, device="cuda:0")
        counts = torch.zeros((H, W), dtype=torch.int32, device="cuda:0")
        ac_med, ac_min = timed(lambda: s.render_ac(fb, counts), a.reps)
        p1_med, p1_min = timed(lambda: s.render_pass1(fb), a.reps)
        fr_med, fr_min = timed(lambda: s.render_frame(fb, mask), a.reps)
        s.set_flag("showNormals", 1)
        nf_med, nf_min = timed(lambda: s.render_frame(fb, mask), a.reps)
        s.set_flag("showNormals", 0)
        mx = int(counts.max().item())
        rw, rh = a.ref_size, a.ref_size * H // W
        t0 = time.time()
        ref_ms = reference_serial(name, rw, rh)
        row = dict(scene=name, width=W, height=H, heatmap_ms=ac_med, heatmap_min_ms=ac_min, ac_max=mx, pass1_ms=p1_med, pass1_min_ms=p1_min,
                   frame_ms=fr_med, normals_frame_ms=nf_med, normals_frame_min_ms=nf_min,
                   ref_serial_ms=ref_ms, ref_size=[rw, rh], ref_serial_scaled_ms=(ref_ms * (W * H) / (rw * rh)) if ref_ms is not None else None,
                   ref_wall_s=round(time.time() - t0, 2))
        print(json.dumps(row), flush=True)
        rows.append(row)
        s.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
