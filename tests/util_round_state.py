"""Scenes for the state that the PLAIN pass-1 and colour kernels keep, fetch again or derive again around a mesh walk (traceWave and castRayPlainWave in
rendering_amd/csrc/rtx_kernels.hip): the object's record and flag word, the lane sets of a trace, the light's record, the tile loop's scalars.  Small
frames of the family of tests/util_shading.py -- its tori and maps, every object Diffuse, point and distant lights only -- with what makes each case the
case it is named after asserted on the oracle's own rays and hits (expectations): no case is vacuous.  Used by tests/test_gpu_round_state.py."""
import os

import numpy as np

from tests import util_plain_rounds as PR
from tests import util_shading as U

f32 = np.float32
MAX_W, MAX_H = 72, 56
SRC_COPIES = 6          # point lights with a source copy of the prune records (kMaxSrcLights, rendering_amd/csrc/rtx_device.h)
POP_MANY = 4            # tiles per atomic in the cheap half of a queue (RTX_POP_MANY, rendering_amd/csrc/rtx_tuning.h)

A = U.mesh("A", d=(64, 24, 11), s=(12, 52, 13))
B = U.mesh("B", d=(8, 124, 14))
C = U.mesh("C", d=(36, 36, 15))
D = U.mesh("D", s=(4, 52, 16))
SPHERE = "[object]\ntype=sphere\npos=0.3,0.1,-3.0\ncolor=0.9,0.6,0.3\nradius=0.55\n\n"
FLOOR = "[object]\ntype=plane\npos=0,-2.6,0\nnormal=0,1,0\ncolor=0.8,0.9,0.7\n\n"
BELOW = "[light]\ntype=point\nposition=0.5,-9,-4\ncolor=1,1,0.8\nintensity=0.9\n\n"


def point(x, y, z, k):
    return "[light]\ntype=point\nposition=%g,%g,%g\ncolor=%g,%g,%g\nintensity=%g\n\n" % (x, y, z, 0.4 + 0.07 * k, 1 - 0.06 * k, 0.5 + 0.05 * k, 0.3 + 0.05 * k)


# nine lights: eight point lights (more than SRC_COPIES: those from index SRC_COPIES on walk with copy 0), a distant light between them, and one under the floor
MANY = (point(2, 3, 0, 0) + point(-3, 1.5, -1, 1) + point(0, 4, -3, 2) + U.DISTANT + point(3, -1, -1, 3) + point(-2, 3, 1, 4) +
        point(1, 2, -1, 5) + BELOW + point(-1, 3, -2, 6))

# name -> dict(w, h, fov, rot, lights, objects: list of mesh dicts / object text in scene order)
CASES = {
    "objects": dict(w=72, h=56, fov=75, rot=(-5, 8, 3), lights=U.POINT + BELOW, objects=[A, FLOOR, SPHERE, C]),
    "irregular": dict(w=71, h=55, fov=75, rot=(0, 0, 0), lights=U.POINT + U.DISTANT, objects=[A, B, C, D]),
    "wide": dict(w=16, h=16, fov=120, rot=(-5, 8, 3), lights=U.POINT + U.DISTANT, objects=[A, B, C, D]),
    "lights": dict(w=72, h=56, fov=75, rot=(-5, 8, 3), lights=MANY, objects=[FLOOR, A, C]),
    "tiles": dict(w=71, h=55, fov=75, rot=(-5, 8, 3), lights=U.POINT + U.DISTANT, objects=[A, B, FLOOR, D]),
}


def scene_text(name, dst, cull):
    c = CASES[name]
    s = "[options]\nwidth=%d\nheight=%d\nfov=%d\nposition=0.1,0.2,0.5\nrotation=%s\nmax_ray_depth=3\nac_penalty=2\nbackground_color=0.2,0.3,0.4\nimage_name=output/shading\n" % (
        c["w"], c["h"], c["fov"], ",".join("%g" % x for x in c["rot"]))
    s += "skyboxes=%s\nuseBackfaceCulling=%d\n\n" % (",".join(os.path.join(dst, "k%d.bmp" % k) for k in range(6)), int(cull))
    s += c["lights"]
    for ob in c["objects"]:
        s += ob if isinstance(ob, str) else U.object_text(ob, dst)
    return s + "[end]\n"


def write_scene(name, dst, cull):
    """Writes the scene (the family's images must be in dst: util_shading.write_images) and returns its path."""
    path = os.path.join(str(dst), "rs_%s%d.scene" % (name[:5], cull))
    with open(path, "w") as f:
        f.write(scene_text(name, str(dst), cull))
    return path


def point_lights(name):
    """[(index among the lights, position)] of the case's point lights."""
    out = []
    for i, blk in enumerate(CASES[name]["lights"].split("[light]\n")[1:]):
        if blk.startswith("type=point"):
            out.append((i, np.array([float(x) for x in blk.split("position=")[1].split("\n")[0].split(",")])))
    return out


def tiles(mask):
    """An [h, w] mask as [tile row, 8, tile column, 8] over the whole 8 x 8 tiles of the frame."""
    h, w = mask.shape
    return mask[:h // 8 * 8, :w // 8 * 8].reshape(h // 8, 8, w // 8, 8)


def expectations(name, o, rays, hits):
    """rays / hits: the frame's primary rays and the oracle's hit records for them ([hit, object, triangle, t, u, v, 0, 0])."""
    c = CASES[name]
    w, h = o.width, o.height
    assert (w, h) == (c["w"], c["h"]) and w <= MAX_W and h <= MAX_H
    hit = hits[:, 0] > 0
    obj = hits[:, 1].astype(int)
    is_mesh = np.array([not isinstance(ob, str) for ob in c["objects"]])
    assert o.n_objects == len(c["objects"]) and (hit & is_mesh[np.clip(obj, 0, len(is_mesh) - 1)]).any(), "%s: no ray hits a mesh" % name
    if name == "objects":
        assert [isinstance(ob, str) for ob in c["objects"]] == [False, True, True, False]      # a plane and a sphere between two meshes, in scene order
        nearest = set(obj[hit])
        assert nearest == set(range(4)), "objects: nearest hits only of %s" % sorted(nearest)
        # who stands between a point light and a point that is seen: the first hit of the ray from the light to that point, when it is nearer than the point
        casts = set()
        P = rays[hit, 0:3].astype(np.float64) + rays[hit, 3:6].astype(np.float64) * hits[hit, 3:4].astype(np.float64)
        for _, lp in point_lights(name):
            v = P - lp
            dist = np.linalg.norm(v, axis=1)
            sh, _ = o.probe(np.concatenate([np.tile(lp, (len(P), 1)), v / dist[:, None]], 1).astype(f32), colours=False)
            blocked = (sh[:, 0] > 0) & (sh[:, 3] < dist * (1 - 1e-3))
            casts |= set(sh[blocked, 1].astype(int))
        assert casts == set(range(4)), "objects: shadows cast only by %s" % sorted(casts)
    if name == "irregular":
        assert w % 2 == 1 and h % 2 == 1 and c["rot"] == (0, 0, 0)
        zero = (rays[:, 3:6] == 0).any(1).reshape(h, w)
        assert zero.any() and (zero & hit.reshape(h, w) & is_mesh[np.clip(obj, 0, 3)].reshape(h, w)).any(), "irregular: no ray with a zero component hits a mesh"
        t = tiles(zero)
        mixed = t.any((1, 3)) & ~t.all((1, 3)) & tiles(hit.reshape(h, w)).any((1, 3))
        assert mixed.any(), "irregular: no tile holds rays with and without a zero direction component"
    if name == "wide":
        # a tile of 8 x 8 pixels spans half of a 120-degree view: the box of its directions, carried to the distance of the nearest hit, is wider than a torus
        d = rays[:, 3:6].reshape(h, w, 3)
        for ty in range(h // 8):
            for tx in range(w // 8):
                dd = d[ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8].reshape(-1, 3)
                assert ((dd.max(0) - dd.min(0)) / 2).max() > 0.4
        assert hit.any() and float(hits[hit, 3].min()) * 0.4 > 1.0
    if name == "lights":
        pl = point_lights(name)
        assert len(pl) > SRC_COPIES and o.n_lights == 9 and sum(1 for i, _ in pl if i >= SRC_COPIES) >= 2
        assert 0 < min(i for i in range(9) if i not in [k for k, _ in pl]) < SRC_COPIES      # the distant light stands between point lights
        # the light under the floor: every ray from the floor to it is moot, and a tile of pure floor has a round with nothing to trace
        floor = (hit & (obj == 0)).reshape(h, w)
        assert tiles(floor).all((1, 3)).sum() >= 2, "lights: no tile of pure floor"
    if name == "tiles":
        n_tiles = ((w + 7) // 8) * ((h + 7) // 8)
        assert n_tiles % POP_MANY != 0 and n_tiles // 2 > POP_MANY
        sky, some = PR.tiles_hit(o)
        assert sky + some > 0 and some > 0
