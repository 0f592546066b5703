"""rtx_render_light / Scene.render_light without a GPU: the extension header and its symbol list, the binding's structure, the argument
checks, and the frames of the GPU tests (tests/test_gpu_render_light.py) shown to be non-trivial with the oracle alone: in every frame
some pixel misses, and of its (pixel, light) pairs some are lit, some shadowed while facing the light, some turned away from it.

The classes take the normal decoded from the showNormals colour (tests/util_ao.decoded_normals), which is within an ulp or two of hitNormal:
good enough to show that a class is not empty, not for the bit-exact expectations of the GPU tests."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import util_ao as AO
from tests import util_aov as U
from tests import util_light as UL
from tests import util_occlusion as OC
from tests import util_render_light as RL

ROOT = U.ROOT
f32 = np.float32


def test_render_light_header_and_symbol_list(ra):
    hdr = open(os.path.join(ROOT, "include", "rtx_render_light.h")).read()
    declared = re.findall(r"\b(rtx_[a-z0-9_]+)\s*\(", hdr)
    assert declared == list(ra.RTX_RENDER_LIGHT_SYMBOLS) == ["rtx_render_light"]
    others = [n for n in dir(ra) if re.fullmatch(r"RTX_[A-Z_]*SYMBOLS", n) and n != "RTX_RENDER_LIGHT_SYMBOLS"]
    assert len(others) >= 11
    for n in others:
        assert not set(declared) & set(getattr(ra, n)), n
    rtx, _ = ra.load()
    assert hasattr(rtx, "rtx_render_light")
    listed, missing = ra.exported_symbols()
    assert not missing and listed == list(ra.RTX_SYMBOLS)
    # rtx_light.h keeps its declarations; rtx.h does not include the new header
    assert "rtx_render_light" not in open(os.path.join(ROOT, "include", "rtx_light.h")).read()
    assert "rtx_render_light" not in open(os.path.join(ROOT, "include", "rtx.h")).read()
    # the structure of the binding is the header's: the number of lights, then five pointers in its order
    body = re.search(r"typedef struct rtx_frame_light_buffers \{(.*?)\} rtx_frame_light_buffers;", hdr, re.S).group(1)
    fields = re.findall(r"(uint32_t|float\*|uint32_t\*)\s+(\w+);", body)
    assert [n for _, n in fields] == [n for n, _ in ra.FrameLightBuffers._fields_] and len(fields) == 6
    assert fields[0] == ("uint32_t", "n_lights") and all(t.endswith("*") for t, _ in fields[1:])
    assert ra.FrameLightBuffers._fields_[0][1] is C.c_uint32 and all(t is C.c_void_p for _, t in ra.FrameLightBuffers._fields_[1:])


def test_c_entry_refuses_null_arguments(ra):
    rtx, _ = ra.load()
    assert rtx.rtx_render_light(None, 0, 8, None, None) == -1      # RTX_ERR_ARG
    assert b"NULL" in rtx.rtx_last_error()
    bufs = ra.FrameLightBuffers(3, None, None, None, None, None)
    assert rtx.rtx_render_light(None, 0, 8, C.byref(bufs), None) == -1


def test_bad_arguments_are_refused_before_the_gpu(ra):
    torch = pytest.importorskip("torch")
    s = ra.Scene("scenes/cfg1_simple_shapes.scene", 32, 24)
    L = s.n_lights
    assert L >= 1
    z = lambda shape, dt=torch.float32: torch.zeros(shape, dtype=dt)
    cases = [
        (dict(), "render_light: nothing to compute"),
        (dict(diffuse=np.zeros((24, 32, 3), f32)), "render_light: diffuse must be a torch tensor"),
        (dict(diffuse=z((24, 32, 3), torch.float64)), "render_light: diffuse must be float32"),
        (dict(specular=z((32, 24, 3))), r"render_light: specular must have shape \(24, 32, 3\)"),
        (dict(specular=z((24, 32))), r"render_light: specular must have shape \(24, 32, 3\)"),
        (dict(diffuse=z((24, 32, 6))[:, :, ::2]), "render_light: diffuse must be contiguous"),
        (dict(light_diffuse=z((24, 32, L, 3))), r"render_light: light_diffuse must have shape \(%d, 24, 32, 3\)" % L),
        (dict(light_diffuse=z((L + 1, 24, 32, 3))), r"render_light: light_diffuse must have shape \(%d, 24, 32, 3\)" % L),
        (dict(light_specular=z((L, 24, 32, 3), torch.float16)), "render_light: light_specular must be float32"),
        (dict(light_open=z((L, 24, 32))), "render_light: light_open must be int32"),
        (dict(light_open=z((L, 24, 32), torch.uint8)), "render_light: light_open must be int32"),
        (dict(light_open=z((L, 24, 32, 1), torch.int32)), r"render_light: light_open must have shape \(%d, 24, 32\)" % L),
        (dict(light_open=z((L, 24, 64), torch.int32)[:, :, ::2]), "render_light: light_open must be contiguous"),
        (dict(diffuse=z((24, 32, 3))), "render_light: diffuse must be on cuda:0"),
        (dict(diffuse=None, light_open=z((L, 24, 32), torch.int32)), "render_light: light_open must be on cuda:0"),
    ]
    for kw, what in cases:
        with pytest.raises(ValueError, match=what):
            s.render_light(**kw)
    assert s._gpu is None              # (the scene was never flattened and uploaded: no GPU call was made)
    s.close()


# Every frame of the GPU tests' equality with light_rays, culling on: a miss, and pairs of all three classes -- but for what a scene cannot
# show at any of the three sizes (tests/test_light_rays_cpu.py leaves the same three scenes out of its shares): in mixed_materials no
# pixel misses (its floor fills the view), in cfg3_reflective_refractive no pair is shadowed while facing its one light, in
# cfg4_textured_256 no pair that faces a light is open.  Those frames still carry the other three classes, and every size has every class
# in the four other scenes.  What the oracle gives per frame is printed by the test.
ABSENT = {"mixed_materials": "misses", "cfg3_reflective_refractive": "shadowed", "cfg4_textured_256": "lit"}


@pytest.mark.parametrize("w,h", RL.SIZES)
@pytest.mark.parametrize("name", RL.SCENES)
def test_the_frames_are_not_trivial(oracle, tmp_path, name, w, h):
    path = "scenes/%s.scene" % name
    text = open(os.path.join(ROOT, path)).read()
    exp = U.expected_of(path, w, h, 1)
    mask = U.written_mask(w, h)
    o = oracle.OracleScene(path, w, h)
    rays = U.primary_rays(o)
    hit = (exp["hit"] & mask).reshape(-1)
    hits = np.zeros((len(rays), 8), f32)
    hits[:, 0] = hit
    hits[:, 3] = exp["depth"].reshape(-1)
    lights = UL.lights_of_text(text)
    plan = UL.Plan(o, lights, rays, hits, AO.decoded_normals(exp))
    o.close()
    hit2, t2 = OC.opaque_probe(oracle, path, tmp_path, plan.shadow_rays, culling=1)
    occluded = OC.expected(hit2, t2, plan.shadow_tmax)
    m = len(plan.idx)
    lit = shadowed = away = 0
    at = 0
    for I, L, dist in plan.lights:
        S_ = L.shape[1]
        occ = occluded[at:at + m * S_].reshape(S_, m).T != 0
        at += m * S_
        facing = UL.max0(UL.dot(np.broadcast_to(plan.N[:, None, :], L.shape), -L)) > 0
        lit += int((facing & ~occ).any(1).sum()); shadowed += int((facing & occ).any(1).sum()); away += int((~facing).all(1).sum())
    misses = int((~exp["hit"] & mask).sum())
    print("%s %dx%d: %d written pixels, %d misses, %d lights; pairs lit %d, shadowed while facing %d, facing away %d" % (
        name, w, h, mask.sum(), misses, len(plan.lights), lit, shadowed, away))
    counts = dict(misses=misses, lit=lit, shadowed=shadowed, away=away)
    for k, v in counts.items():
        assert v >= 1 or ABSENT.get(name) == k, "%s %dx%d: no %s" % (name, w, h, k)
