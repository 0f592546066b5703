#!/usr/bin/env python
"""Times replacing texture maps and skybox faces of a live GPU scene (include/rtx_texture.h) on scenes/cfg4_textured_1024.scene:
its three 1024 x 1024 maps and a skybox of 2048 x 1024 faces given to it here.  Writes one JSON object to --out, stamped with tools/srchash.py.
Per target (diffuse, normal, specular, sky face):
  write_rgb8 / write_stored   rtx_scene_write_texels over the whole map from a device tensor, per call: HIP events around --batch calls queued back
                              to back on one stream, the median of --reps such windows after a warm-up window; the bytes a call reads and
                              writes (computed from the shapes) and the achieved GB/s beside the HBM figures of the hardware notes
  torch_then_stored           the same result by the loader's arithmetic written in torch (fp32 steps, fp64 rsqrt for the normals) followed by
                              a STORED write, timed the same way -- not bit-exact for normal maps, a comparison of cost only
  set_texture_ms              Scene.set_texture / set_skybox end to end from device tensors: host wall clock around the synchronised call
  reload_ms                   the only route without this API: the image written as a BMP, the scene file loaded again and uploaded (host wall
                              clock to the end of Scene.gpu()); with --package DIR measured on another build's package, e.g. the parent commit's

    python tools/texture_edit_probe.py [--reps 9] [--batch 50] [--out profiles/texture_edit_time.json]
    python tools/texture_edit_probe.py --only-reload --package DIR --out FILE
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE = "scenes/cfg4_textured_1024.scene"
HBM_SPEC_GBS, HBM_COPY_GBS = 8000.0, 6290.0      # MI355X: HBM3E peak by specification; measured with a float4 copy


def med(xs):
    return float(np.median(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--only-reload", action="store_true")
    ap.add_argument("--package", default=ROOT, help="the directory that holds the rendering_amd package to time")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "texture_edit_time.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package))
    sys.path.insert(1, ROOT)
    import torch
    import rendering_amd as RA
    from rendering_amd import assets
    from tools.srchash import source_hash
    os.chdir(ROOT)
    assets.ensure()
    sync = torch.cuda.synchronize
    result = dict(device=torch.cuda.get_device_name(0), scene=SCENE, reps=a.reps, batch=a.batch, package=os.path.relpath(os.path.abspath(a.package), ROOT),
                  source_hash=source_hash(), hbm_gbs=dict(specification=HBM_SPEC_GBS, float4_copy=HBM_COPY_GBS), targets={})
    rng = np.random.default_rng(7)
    sizes = {"diffuse": (1024, 1024), "normal": (1024, 1024), "specular": (1024, 1024), "sky": (2048, 1024)}

    # the route without the API: a BMP written, the scene file loaded again and uploaded
    text = open(os.path.join(ROOT, SCENE)).read()
    with tempfile.TemporaryDirectory(dir=os.path.join(ROOT, "output") if os.path.isdir(os.path.join(ROOT, "output")) else None) as d:
        reload_ms = []
        for k in range(4):
            img = rng.integers(0, 256, (1024, 1024, 3), dtype=np.uint8)
            sync(); t0 = time.perf_counter()
            bmp = os.path.join(d, "d%d.bmp" % k)
            with open(bmp, "wb") as f:
                f.write(assets.bmp24(img))
            path = os.path.join(d, "s%d.scene" % k)
            with open(path, "w") as f:
                f.write(text.replace("scenes/assets/diffuse_1024.bmp", bmp))
            g = RA.Scene(path, 256, 256, cwd=ROOT)
            g.gpu(); sync()
            t = (time.perf_counter() - t0) * 1e3
            g.close()
            if k:
                reload_ms.append(t)
        assert "diffuse_1024.bmp" in text
    result["reload_ms"] = dict(median=med(reload_ms), min=min(reload_ms), max=max(reload_ms), what="one 1024 x 1024 diffuse map: BMP written, scene file loaded, uploaded")
    print(json.dumps({"reload_ms": result["reload_ms"]}), flush=True)

    if not a.only_reload:
        g = RA.Scene(SCENE, 256, 256, cwd=ROOT)
        g.gpu()
        st = torch.cuda.Stream()

        def window(call):
            """per-call microseconds: events around --batch calls on `st`, the median of --reps windows after one warm-up window"""
            times = []
            for k in range(a.reps + 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                sync()
                with torch.cuda.stream(st):
                    e0.record(st)
                    for _ in range(a.batch):
                        call()
                    e1.record(st)
                st.synchronize()
                if k:
                    times.append(e0.elapsed_time(e1) * 1e3 / a.batch)
            return dict(median_us=med(times), min_us=min(times), max_us=max(times))

        def torch_decode(kind, rgb):
            c = rgb.to(torch.float32) / 256
            if kind in ("diffuse", "sky"):
                return c
            if kind == "specular":
                return ((c[..., 0] + c[..., 1]) + c[..., 2]) / 3
            v = torch.stack([c[..., 0] * 2 - 1, -(c[..., 1] * 2 - 1), c[..., 2]], -1)
            l2 = (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]
            f = torch.where(l2 > 0, (1 / torch.sqrt(l2.double())).float(), torch.ones_like(l2))
            return v * f[..., None]

        for kind, (w, h) in sizes.items():
            ch = 1 if kind == "specular" else 3
            rgb = torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).cuda()
            if kind == "sky":
                wall = []
                for k in range(4):
                    sync(); t0 = time.perf_counter()
                    g.set_skybox([rgb] * 6); sync()
                    wall.append((time.perf_counter() - t0) * 1e3)
                write = lambda img: g.write_skybox(2, img, stream=st)
                read = lambda: g.skybox_face(2)
            else:
                wall = []
                for k in range(4):
                    sync(); t0 = time.perf_counter()
                    g.set_texture(0, kind, rgb); sync()
                    wall.append((time.perf_counter() - t0) * 1e3)
                write = lambda img, kind=kind: g.write_texture(0, kind, img, stream=st)
                read = lambda kind=kind: g.texture(0, kind)
            stored = read().clone()
            sync()
            r = dict(size=[w, h], set_texture_ms=dict(median=med(wall[1:]), first=wall[0], what="six faces" if kind == "sky" else "one map"))
            for fmt, src, nbytes in (("write_rgb8", rgb, w * h * (3 + 4 * ch)), ("write_stored", stored, w * h * 8 * ch)):
                t = window(lambda: write(src))
                t.update(bytes=nbytes, gbs=nbytes / t["median_us"] / 1e3)
                t.update(share_of_hbm_specification=t["gbs"] / HBM_SPEC_GBS, share_of_float4_copy=t["gbs"] / HBM_COPY_GBS)
                r[fmt] = t
            r["torch_then_stored"] = window(lambda: write(torch_decode(kind, rgb)))
            want = torch_decode(kind, rgb)
            write(rgb); st.synchronize()
            r["torch_decode_equals_kernel"] = bool((read().view(torch.int32) == want.view(torch.int32)).all())
            result["targets"][kind] = r
            print(json.dumps({kind: r}), flush=True)
        g.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
