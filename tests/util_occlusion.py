"""Expected values for Scene.occluded (rtx_occluded_rays) from the oracle's camera-ray probe: a shadow ray's trace skips the Transparent
objects and keeps the order of the others (scene.cpp:731-754), so it is the probe's trace in the scene S' = S without its transparent
[object] blocks, compared with the range:  occluded = hit' and tNear' < tmax, in float32."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLT_MAX = np.finfo(np.float32).max
_TRANSPARENT = re.compile(r"^\s*material\s*=\s*transparent\b", re.I | re.M)


def opaque_scene(path, tmp_path):
    """Writes S' for the scene file `path` into tmp_path and returns (its path, the number of [object] blocks left out).  A block is
    left out by its material= key (comments may say "transparent" too)."""
    text = open(os.path.join(ROOT, path) if not os.path.isabs(path) else path).read()
    blocks = re.split(r"(?m)^(?=\[)", text)
    kept, dropped = [], 0
    for b in blocks:
        if b.startswith("[object]") and _TRANSPARENT.search(b):
            dropped += 1
        else:
            kept.append(b)
    out = os.path.join(str(tmp_path), "opaque_" + os.path.basename(path))
    with open(out, "w") as f:
        f.write("".join(kept))
    return out, dropped


def opaque_probe(oracle, path, tmp_path, rays, culling=None, size=64):
    """(hit', tNear') of the rays in S', float32; culling: None = as the scene says, else useBackfaceCulling forced to it."""
    p, _ = opaque_scene(path, tmp_path)
    o = oracle.OracleScene(p, size, size)
    if culling is not None:
        oracle.lib().orc_set_flag(o.h, b"useBackfaceCulling", int(culling))
    h, _ = o.probe(rays, colours=False)
    o.close()
    return h[:, 0] > 0, h[:, 3].astype(np.float32)


def expected(hit, tnear, tmax):
    """The contract: some opaque object at tNear < tmax (strict float32 <; NaN compares false)."""
    tmax = np.broadcast_to(np.asarray(tmax, np.float32), tnear.shape)
    with np.errstate(invalid="ignore"):
        return (hit & (tnear < tmax)).astype(np.uint8)


def tmax_mix(hit, tnear, seed=0x5EED):
    """The seeded mix of ranges: for a ray that hits, one of 0.5 t, 1.5 t, +inf, t, nextafter(t, +inf), nextafter(t, 0) drawn uniformly
    (half of them occluded, the last three pin the strict < at the nearest blocker and one ulp to either side); for a ray that misses a
    uniform value in [0.1, 20]."""
    rng = np.random.default_rng(seed)
    n = len(tnear)
    pick = rng.integers(0, 6, n)
    miss = rng.uniform(0.1, 20.0, n).astype(np.float32)
    t = tnear.astype(np.float32)
    inf = np.float32(np.inf)
    with np.errstate(over="ignore"):      # (a miss's tNear is FLT_MAX; its row of the table is not used)
        table = np.stack([np.float32(0.5) * t, np.float32(1.5) * t, np.full(n, inf, np.float32), t,
                          np.nextafter(t, inf), np.nextafter(t, np.float32(0))]).astype(np.float32)
    return np.where(hit, table[pick, np.arange(n)], miss).astype(np.float32)
