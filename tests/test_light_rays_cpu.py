"""rtx_light_rays / Scene.light_rays without a GPU: the extension header and its symbol list, the argument checks, tests/util_light's
restatement of the contract pinned to the oracle where the exact normal is known without a GPU (planes and spheres), and the inputs of the
GPU tests (tests/test_gpu_light_rays.py) shown to be non-trivial with the oracle alone: the rays hit Diffuse and Phong objects, and their
(hit, light) pairs are lit, shadowed while facing the light, and turned away from it in fair shares."""
import os
import re

import numpy as np
import pytest

from tests import util_aov as U
from tests import util_light as UL
from tests import util_occlusion as OC
from tests import util_shading as S
from tests import util_surface as SU

ROOT = U.ROOT
f32 = np.float32
MATERIALS = {"": 0, "diffuse": 0, "reflective": 1, "transparent": 2, "phong": 3}


@pytest.fixture(scope="module")
def family(tmp_path_factory):
    d = S.short_dir(tmp_path_factory)
    return d, S.write_family(d)


def path_of(name, family):
    return family[1][name] if name in S.FAMILY else "scenes/%s.scene" % name


def text_of(path):
    return open(path if os.path.isabs(path) else os.path.join(ROOT, path)).read()


def material_of(block):
    return MATERIALS[block.get("material", "").split(",")[0]]


def test_light_header_and_symbol_list(ra):
    hdr = open(os.path.join(ROOT, "include", "rtx_light.h")).read()
    declared = set(re.findall(r"\b(rtx_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(ra.RTX_LIGHT_SYMBOLS) and len(ra.RTX_LIGHT_SYMBOLS) == len(declared)
    for other in (ra.RTX_SYMBOLS, ra.RTX_EDIT_SYMBOLS, ra.RTX_QUERY_SYMBOLS, ra.RTX_AOV_SYMBOLS, ra.RTX_AO_SYMBOLS, ra.RTX_SURFACE_SYMBOLS):
        assert not declared & set(other)
    rtx, _ = ra.load()
    for s in declared:
        assert hasattr(rtx, s), s
    listed, missing = ra.exported_symbols()
    assert not missing and listed == list(ra.RTX_SYMBOLS)
    # the structure of the binding is the header's: the number of lights, then six pointers in its order
    body = re.search(r"typedef struct rtx_light_buffers \{(.*?)\} rtx_light_buffers;", hdr, re.S).group(1)
    fields = re.findall(r"(uint32_t|float\*|uint32_t\*)\s+(\w+);", body)
    assert [n for _, n in fields] == [n for n, _ in ra.LightBuffers._fields_] and len(fields) == 7
    assert fields[0] == ("uint32_t", "n_lights") and all(t.endswith("*") for t, _ in fields[1:])
    assert ra.LightBuffers._fields_[0][1] is __import__("ctypes").c_uint32


def test_c_entry_refuses_a_null_scene(ra):
    rtx, _ = ra.load()
    assert rtx.rtx_light_rays(None, 4, None, None, None) == -1      # RTX_ERR_ARG
    assert b"NULL" in rtx.rtx_last_error()


def test_bad_arguments_are_refused_before_the_gpu(ra):
    torch = pytest.importorskip("torch")
    s = ra.Scene("scenes/cfg1_simple_shapes.scene", 32, 24)
    z = lambda shape, dt=torch.float32: torch.zeros(shape, dtype=dt)
    cases = [
        (dict(rays=z((4, 6)), diffuse=False, specular=False), "light_rays: nothing to compute"),
        (dict(rays=np.zeros((4, 6), np.float32)), "light_rays: rays must be a torch tensor"),
        (dict(rays=z((4, 6), torch.float64)), "light_rays: rays must be float32"),
        (dict(rays=z((6, 4))), r"light_rays: rays must have shape \(n, 6\)"),
        (dict(rays=z((24,)), per_light=True), r"light_rays: rays must have shape \(n, 6\)"),
        (dict(rays=z((4, 12))[:, ::2]), "light_rays: rays must be contiguous"),
        (dict(rays=z((4, 6)), hits=True), "light_rays: rays must be on cuda:0"),
    ]
    for kw, what in cases:
        with pytest.raises(ValueError, match=what):
            s.light_rays(**kw)
    assert s._gpu is None              # (the scene was never flattened and uploaded: no GPU call was made)
    s.close()


def analytic_case(oracle, path, w, h):
    """The camera rays of a scene file that hit a Diffuse or Phong plane or sphere, with what the oracle alone knows of them: hit records,
    colours, the exact N (the plane's stored normal, normalize(P - centre) of a sphere), and the objects' constants per ray."""
    vec = lambda s: np.array([float(x) for x in s.split(",")], f32)
    blocks = SU.object_blocks(text_of(path))
    o = oracle.OracleScene(path, w, h)
    rays = U.primary_rays(o)
    hits, col = o.probe(rays)
    obj = hits[:, 1].astype(np.int32)
    ok = np.zeros(len(rays), bool)
    for k, b in enumerate(blocks):
        if b["type"] in ("plane", "sphere") and material_of(b) in (0, 3):
            ok |= obj == k
    rays, hits, col, obj = rays[ok], hits[ok], col[ok], obj[ok]
    P = rays[:, 0:3] + rays[:, 3:6] * hits[:, 3:4]
    N = np.zeros((len(rays), 3), f32)
    const = {c: np.zeros(len(rays), f32) for c in ("ambient", "kd", "ks", "ns")}
    albedo = np.zeros((len(rays), 3), f32)
    material = np.zeros(len(rays), np.int32)
    for k, b in enumerate(blocks):
        sel = np.nonzero(obj == k)[0]
        if not len(sel):
            continue
        if b["type"] == "plane":
            N[sel] = vec(b["normal"])
            assert np.array_equal(oracle.normalize(vec(b["normal"])), vec(b["normal"]))
        else:
            for j in sel:
                N[j] = oracle.normalize(P[j] - vec(b["pos"]))
        albedo[sel] = vec(b["color"])
        material[sel] = material_of(b)
        m = b.get("material", "").split(",")
        ka, kd, ks, ns = (f32(float(x)) for x in m[1:5]) if m[0] == "phong" else (f32(0.1), f32(0.1), f32(1.0), UL.DEFAULT_N_SPECULAR)
        const["ambient"][sel], const["kd"][sel], const["ks"][sel], const["ns"][sel] = ka, kd, ks, ns
    return o, blocks, rays, hits, col, obj, N, albedo, material, const


# tests/util_light itself: on the hits whose N the oracle's own functions give exactly, the sums it restates make the colours the oracle
# returns, bit for bit (Diffuse: scene.cpp:808, Phong: scene.cpp:852).  What matched when this was written: cfg1_simple_shapes 48x32 --
# 686 Diffuse plane, 18 Diffuse sphere and 177 Phong sphere hits; area_light 48x36 -- 487 plane and 223 Phong sphere hits.
@pytest.mark.parametrize("name,w,h", [("cfg1_simple_shapes", 48, 32), ("area_light", 48, 36)])
def test_the_expectation_gives_the_oracles_colours(oracle, tmp_path, name, w, h):
    path = "scenes/%s.scene" % name
    o, blocks, rays, hits, col, obj, N, albedo, material, const = analytic_case(oracle, path, w, h)
    plan = UL.Plan(o, UL.lights_of_text(text_of(path)), rays, hits, N)
    o.close()
    assert plan.hit.all() and len(plan.shadow_rays) >= len(rays)
    hit2, t2 = OC.opaque_probe(oracle, path, tmp_path, plan.shadow_rays)
    got = plan.reduce(OC.expected(hit2, t2, plan.shadow_tmax), const["ns"])
    is_dp, want = UL.colour_identities(col, albedo, const["ks"], got["diffuse"], got["specular"], material, const["ambient"], const["kd"])
    assert is_dp.all()
    bad = (U.bits(want) != U.bits(col)).any(-1)
    kinds = {(blocks[k]["type"], material_of(blocks[k])): int((obj == k).sum()) for k in np.unique(obj)}
    print("%s %dx%d: %d hits by (type, material) %s, %d differ; shadow rays %d, open %.3f" % (
        name, w, h, len(rays), kinds, bad.sum(), len(plan.shadow_rays), (got["light_open"] > 0).mean()))
    assert len(rays) >= 700 and (material == 3).sum() >= 150 and (material == 0).sum() >= 400
    assert not bad.any(), "%d of %d hits: the restated sums do not make the oracle's colour" % (bad.sum(), len(rays))
    # ... and both answers of the visibility occur, so do partly open area lights
    assert 0.05 < (got["light_open"] == 0).mean() < 0.95
    if name == "area_light":
        assert ((got["light_open"][:, 0] > 0) & (got["light_open"][:, 0] < 9)).any()


def test_lights_of_text_reads_the_area_lights():
    """lights_of_text on scenes/area_light.scene: types, sample counts, and the grid's centre and single sample at the light's position
    (the points themselves are compared with the device's on the GPU: tests/test_gpu_light_rays.py)"""
    recs, pts = UL.lights_of_text(text_of("scenes/area_light.scene"))
    assert list(recs["type"]) == [3, 3, 2] and list(recs["n_points"]) == [9, 1, 0] and pts.shape == (10, 3)
    assert np.array_equal(pts[9], recs[1]["pos"]) and np.array_equal(pts[4], recs[0]["pos"])


def rays_ab(oracle, path, w, h, cull):
    o = oracle.OracleScene(path, w, h)
    cam = U.primary_rays(o)
    o.close()
    return cam, SU.oracle_bounce_rays(oracle, path, w, h, cull)


# (A): on every scene but cfg3_reflective_refractive (mirrors and glass in front of everything) at least 0.10 of the camera rays hit a
# Diffuse or Phong object -- the hits the colour identities speak about
@pytest.mark.parametrize("name", [n for n in SU.SCENES if n != "cfg3_reflective_refractive"])
def test_camera_rays_hit_diffuse_and_phong_objects(family, name):
    path = path_of(name, family)
    w, h = SU.size_of(name)
    blocks = SU.object_blocks(text_of(path))
    exp = U.expected_of(path, w, h, 1)
    obj = exp["object_id"].reshape(-1)
    dp = np.array([material_of(b) in (0, 3) for b in blocks] + [False])
    share = dp[obj].mean()                       # (a miss is -1: the last entry)
    print("%s %dx%d: share of camera rays on Diffuse / Phong objects %.3f" % (name, w, h, share))
    assert share >= 0.10


# The (hit ray, non-area light) pairs of (A) and (B) with culling on, pooled: lit at least 0.30, shadowed while facing the light at least
# 0.015, facing away at least 0.04 -- every branch of the per-light terms is taken by many pairs.  (N decoded from the showNormals colour:
# an ulp or two from hitNormal, good enough for shares.)
@pytest.mark.parametrize("name", UL.SHARED_OUT)
def test_pairs_are_lit_shadowed_and_turned_away(oracle, family, tmp_path, name):
    path = path_of(name, family)
    w, h = SU.size_of(name)
    cam, bounce = rays_ab(oracle, path, w, h, 1)
    rays = np.concatenate([cam, bounce])
    exp = SU.expected_of(path, w, h, 1, rays)
    N = ((exp["normal_colour"] - f32(0.5)) * f32(2)).astype(f32)
    lights = UL.lights_of_text(text_of(path))
    o = oracle.OracleScene(path, w, h)
    plan = UL.Plan(o, lights, rays, exp["hits"], N)
    o.close()
    hit2, t2 = OC.opaque_probe(oracle, path, tmp_path, plan.shadow_rays, culling=1)
    occluded = OC.expected(hit2, t2, plan.shadow_tmax)
    m = len(plan.idx)
    lit = shadowed = away = total = 0
    at = 0
    for li, (I, L, dist) in enumerate(plan.lights):
        S_ = L.shape[1]
        occ = occluded[at:at + m * S_]
        at += m * S_
        if lights[0][li]["type"] == UL.AREA:
            continue
        facing = UL.max0(UL.dot(plan.N, -L[:, 0])) > 0
        lit += int((facing & (occ == 0)).sum()); shadowed += int((facing & (occ != 0)).sum()); away += int((~facing).sum()); total += m
    assert total >= 300               # (the smallest share asked for below is then several pairs)
    print("%s %dx%d: %d pairs, lit %.3f, shadowed while facing %.3f, facing away %.3f" % (name, w, h, total, lit / total, shadowed / total, away / total))
    assert lit / total >= 0.30 and shadowed / total >= 0.015 and away / total >= 0.04
