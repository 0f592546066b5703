"""Scenes for the rounds of the PLAIN kernels (every object Diffuse, every light a point or a distant light: castRayPlainWave and
castRayWave<.., PLAIN = true> in rendering_amd/csrc/rtx_kernels.hip), built from the family of tests/util_shading.py: its "plain" / "plain_nosky" scenes with the list of lights,
the camera or the recursion depth replaced.  Shared by tests/test_gpu_plain_rounds.py (GPU against the oracle) and tests/test_plain_rounds_cpu.py
(the oracle against the reference on the same scenes)."""
import os

import numpy as np

from tests import util_shading as U

f32 = np.float32
W, H = U.W, U.H

POINT2 = "[light]\ntype=point\nposition=-3,1.5,-1\ncolor=0.5,1,0.6\nintensity=0.6\n\n"
DISTANT2 = "[light]\ntype=distant\ndirection=0.5,-0.6,-0.7\ncolor=1,0.5,0.4\nintensity=0.25\n\n"
# under the floor (y = -4) and shining upwards: the floor's normal points away from both, so every shadow ray from the floor to them is moot
# (max(0, N . -L) = +0), and a tile of floor has rounds in which no lane has a ray to trace
POINT_BELOW = "[light]\ntype=point\nposition=0.5,-9,-4\ncolor=1,1,0.8\nintensity=0.9\n\n"
DISTANT_UP = "[light]\ntype=distant\ndirection=0,1,0\ncolor=0.7,0.7,1\nintensity=0.4\n\n"
FLOOR = "[object]\ntype=plane\npos=0,-4,0\nnormal=0,1,0\ncolor=0.8,0.9,0.7\n\n"
# the camera turned to the right: the tori fill the left of the frame, the right is sky
AWAY = "-5,-38,3"

# name -> (scene of the family, lights (None: the family's point + distant), options appended, objects prepended)
SCENES = {
    "no_lights": ("plain", "", {}, ""),
    "mixed_lights": ("plain", U.DISTANT + U.POINT + POINT2 + DISTANT2, {}, ""),
    "light_below": ("plain", POINT_BELOW + DISTANT_UP + U.POINT, {}, FLOOR),
    "only_below": ("plain_nosky", POINT_BELOW + DISTANT_UP, {}, FLOOR),
    "sky_tiles": ("plain", None, {"rotation": AWAY}, ""),
    "bg_tiles": ("plain_nosky", U.POINT + POINT2, {"rotation": AWAY}, ""),
    "depth_zero": ("plain", None, {"max_ray_depth": 0}, ""),
    "depth_negative": ("plain", None, {"max_ray_depth": -1}, ""),
}


def scene_text(name, dst, cull):
    base, lights, extra, objects = SCENES[name]
    extra = dict(extra, useBackfaceCulling=int(cull))
    s = U.scene_text(base, dst, extra=extra)
    family = U.FAMILY[base]["lights"]
    assert s.count(family) == 1
    if lights is not None:
        s = s.replace(family, lights)
    if objects:
        first = s.index("[object]")
        s = s[:first] + objects + s[first:]
    return s


def write_scene(name, dst, cull):
    """Writes the scene (the family's images must be in dst: util_shading.write_images) and returns its path."""
    path = os.path.join(str(dst), "%s%d.scene" % (name[:6], cull))
    with open(path, "w") as f:
        f.write(scene_text(name, str(dst), cull))
    return path


def tiles_hit(o):
    """(tiles whose pixels all hit nothing, tiles with a hit) of the 8x8 tiles of an OracleScene's frame, from its primary rays."""
    hits, _ = o.probe(U.primary_rays(o), colours=False)
    hit = (hits[:, 0] > 0).reshape(o.height, o.width)
    t = hit[:o.height // 8 * 8, :o.width // 8 * 8].reshape(o.height // 8, 8, o.width // 8, 8)
    return int((~t.any((1, 3))).sum()), int(t.any((1, 3)).sum())


def expectations(name, o, frame):
    """What makes the case the case it is named after, asserted on the oracle's own frame: no case is vacuous."""
    sky, some = tiles_hit(o)
    assert some > 0, "%s: no tile sees an object" % name
    if name in ("sky_tiles", "bg_tiles"):
        assert sky >= 8, "%s: only %d tiles of pure sky" % (name, sky)
    if name == "bg_tiles":
        bg = np.array([0.2, 0.3, 0.4], f32)
        t = (frame[:H // 8 * 8 - 8, :W // 8 * 8 - 8] == bg).all(-1).reshape(H // 8 - 1, 8, W // 8 - 1, 8)
        assert t.all((1, 3)).any()
    if name in ("no_lights", "only_below"):
        # no_lights: objColor * (0, 0, 0).  only_below: every light is under the floor -- the floor is moot for all of them, everything
        # above it is in its shadow.  Either way every ray that hits is +0
        hits, col = o.probe(U.primary_rays(o))
        hit = hits[:, 0] > 0
        assert hit.any() and (col[hit] == 0).all() and (frame == 0).all(-1).sum() > hit.sum() // 2
    if name in ("light_below", "only_below"):
        # a tile of pure floor (object 0): all its lanes hit and all are moot for the two lights under the floor, so the wave has whole rounds with nothing to trace
        hits, _ = o.probe(U.primary_rays(o), colours=False)
        floor = ((hits[:, 0] > 0) & (hits[:, 1] == 0)).reshape(o.height, o.width)
        t = floor[:o.height // 8 * 8, :o.width // 8 * 8].reshape(o.height // 8, 8, o.width // 8, 8)
        assert int(t.all((1, 3)).sum()) >= 8, "%s: only %d tiles of pure floor" % (name, int(t.all((1, 3)).sum()))
    if name == "depth_negative":
        hits, _ = o.probe(U.primary_rays(o), colours=False)
        assert (hits[:, 0] > 0).any() and len(np.unique(frame[:-1, :-1].reshape(-1, 3), axis=0)) > 1
