"""What rtx_render_light / Scene.render_light must write (include/rtx_render_light.h): the frames, buffers and comparisons that
tests/test_gpu_render_light.py and tests/test_render_light_cpu.py share.  The contract's identity is "the bits of rtx_light_rays for the
pixel's primary ray", so the expectation of a frame is Scene.light_rays of tests/util_aov.primary_rays, transposed to planes -- existing
code, pinned to the oracle by tests/test_gpu_light_rays.py, and not the code under test."""
import numpy as np

from tests import util_aov as U

f32 = np.float32
SCENES = ["cfg1_simple_shapes", "cfg2_smooth_4k", "cfg3_reflective_refractive", "area_light", "mixed_materials", "cfg4_textured_256", "coincident"]
# 48x32: whole tiles; 36x48 and 33x17: partly valid edge tiles, and the W-1 / H-1 rule cuts inside a tile.  What the oracle shows of
# each frame -- misses, pairs lit, shadowed while facing, facing away -- is asserted and printed by tests/test_render_light_cpu.py.
SIZES = [(48, 32), (36, 48), (33, 17)]
CHANNELS = ("diffuse", "specular", "light_diffuse", "light_specular", "light_open")
SUMS = ("diffuse", "specular")
PER_LIGHT = ("light_diffuse", "light_specular", "light_open")
GUARD = 96                    # untouched elements before and after every buffer
FILL = {c: 7.25 for c in CHANNELS[:4]}
FILL["light_open"] = 0x0BADF00D


def shape_of(c, L, w, h):
    return {"diffuse": (h, w, 3), "specular": (h, w, 3), "light_diffuse": (L, h, w, 3), "light_specular": (L, h, w, 3), "light_open": (L, h, w)}[c]


def planes(out, w, h):
    """Scene.light_rays' channels of a frame's primary rays (numpy, ray-major) as render_light's planes (light-major)."""
    L = out["light_open"].shape[1]
    return dict(diffuse=out["diffuse"].reshape(h, w, 3), specular=out["specular"].reshape(h, w, 3),
                light_diffuse=np.ascontiguousarray(out["light_diffuse"].transpose(1, 0, 2)).reshape(L, h, w, 3),
                light_specular=np.ascontiguousarray(out["light_specular"].transpose(1, 0, 2)).reshape(L, h, w, 3),
                light_open=np.ascontiguousarray(out["light_open"].T).reshape(L, h, w))


def pixels(c, a):
    """a channel as (planes, h, w, ...), a view"""
    return a if c in PER_LIGHT else a[None]


def differ(got, want, mask, names=CHANNELS):
    """{name: number of (plane, pixel) entries of `mask` whose bits differ}: empty = equal."""
    bad = {}
    for c in names:
        assert got[c].shape == want[c].shape, (c, got[c].shape, want[c].shape)
        d = pixels(c, U.bits(got[c]) != U.bits(np.ascontiguousarray(want[c])))
        d = d.any(-1) if d.ndim == 4 else d
        if d[:, mask].any():
            bad[c] = int(d[:, mask].sum())
    return bad


def touched(got, mask):
    """names of the buffers with a changed element outside `mask`"""
    out = []
    for c, a in got.items():
        same = pixels(c, a == a.dtype.type(FILL[c]))
        if not same[:, ~mask].all():
            out.append(c)
    return out
