"""rtx_light_points / rtx_ao_points (Scene.light_points, Scene.ao_points; include/rtx_points.h) without a GPU: the extension header against
the symbol list, the argument checks, and tests/util_points' restatement of the two contracts pinned to the oracle alone where the exact
normal is known without a GPU (planes and spheres): fed with {P, N, V, ns} of the oracle's own hits and the oracle's visibility, its sums
make the colour the oracle's castRay returns for every Diffuse and Phong hit, bit for bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import util_ao as AO
from tests import util_aov as U
from tests import util_light as UL
from tests import util_occlusion as OC
from tests import util_points as UP
from tests.test_light_rays_cpu import analytic_case, text_of

ROOT = U.ROOT
f32 = np.float32
CASES = [("cfg1_simple_shapes", 48, 32), ("area_light", 48, 36)]


def test_points_header_and_symbol_list(ra):
    hdr = open(os.path.join(ROOT, "include", "rtx_points.h")).read()
    declared = re.findall(r"^int\s+(rtx_[a-z0-9_]+)\s*\(", hdr, re.M)
    assert declared == list(ra.RTX_POINTS_SYMBOLS) == ["rtx_light_points", "rtx_ao_points"]
    assert '#include "rtx_light.h"' in hdr and '#include "rtx_ao.h"' in hdr
    for other in (ra.RTX_SYMBOLS, ra.RTX_EDIT_SYMBOLS, ra.RTX_QUERY_SYMBOLS, ra.RTX_AOV_SYMBOLS, ra.RTX_AO_SYMBOLS, ra.RTX_SURFACE_SYMBOLS,
                  ra.RTX_LIGHT_SYMBOLS, ra.RTX_DEFORM_SYMBOLS, ra.RTX_VIEWS_SYMBOLS, ra.RTX_SCATTER_SYMBOLS):
        assert not set(declared) & set(other)
    rtx, _ = ra.load()
    for s in declared:
        assert hasattr(rtx, s), s
    listed, missing = ra.exported_symbols()
    assert not missing and listed == list(ra.RTX_SYMBOLS)


def test_c_entries_refuse_a_null_scene(ra):
    rtx, _ = ra.load()
    bufs, par = ra.LightBuffers(), ra.AoParams()
    assert rtx.rtx_light_points(None, 4, None, None, None, None) == -1      # RTX_ERR_ARG
    assert b"NULL" in rtx.rtx_last_error()
    assert rtx.rtx_light_points(None, 4, None, None, C.byref(bufs), None) == -1
    assert b"NULL" in rtx.rtx_last_error()
    assert rtx.rtx_ao_points(None, 4, None, None, None, None, None) == -1
    assert b"NULL" in rtx.rtx_last_error()
    assert rtx.rtx_ao_points(None, 4, None, C.byref(par), None, None, None) == -1
    assert b"NULL" in rtx.rtx_last_error()


def test_bad_arguments_are_refused_before_the_gpu(ra):
    torch = pytest.importorskip("torch")
    s = ra.Scene("scenes/cfg1_simple_shapes.scene", 32, 24)
    z = lambda shape, dt=torch.float32: torch.zeros(shape, dtype=dt)
    for who, fn, extra in (
            ("light_points", s.light_points, [
                (dict(points=z((4, 6)), diffuse=False), "light_points: nothing to compute"),
                (dict(points=z((4, 6)), specular=True), "light_points: specular needs a view"),
                (dict(points=z((24,)), per_light=True), r"light_points: points must have shape \(n, 6\)")]),
            ("ao_points", s.ao_points, [
                (dict(points=z((4, 6)), ao=False), "ao_points: nothing to compute"),
                (dict(points=z((24,)), counts=True), r"ao_points: points must have shape \(n, 6\)")])):
        more = dict(dirs=z((3, 3))) if who == "ao_points" else {}
        cases = extra + [
            (dict(points=np.zeros((4, 6), np.float32)), "%s: points must be a torch tensor" % who),
            (dict(points=z((4, 6), torch.float64)), "%s: points must be float32" % who),
            (dict(points=z((6, 4))), r"%s: points must have shape \(n, 6\)" % who),
            (dict(points=z((4, 12))[:, ::2]), "%s: points must be contiguous" % who),
            (dict(points=z((4, 6))), "%s: points must be on cuda:0" % who),
        ]
        for kw, what in cases:
            with pytest.raises(ValueError, match=what):
                fn(**dict(more, **kw))
    assert s._gpu is None                  # (the scene was never flattened and uploaded: no GPU call was made)
    s.close()


_case = {}


def case_of(oracle, name, w, h):
    """analytic_case of tests/test_light_rays_cpu.py as points: {P, N} and {V, ns} of the oracle's Diffuse and Phong hits on planes and
    spheres, computed once per scene and shared read-only"""
    if name not in _case:
        path = "scenes/%s.scene" % name
        o, blocks, rays, hits, col, obj, N, albedo, material, const = analytic_case(oracle, path, w, h)
        with np.errstate(all="ignore"):
            P = (rays[:, 0:3] + rays[:, 3:6] * hits[:, 3:4]).astype(f32)      # castRay's hit point (scene.cpp:763)
        points = np.ascontiguousarray(np.concatenate([P, N], 1), f32)
        view = np.ascontiguousarray(np.concatenate([rays[:, 3:6], const["ns"][:, None]], 1), f32)
        plan = UP.PointPlan(o, UL.lights_of_text(text_of(path)), points, view)
        o.close()
        for a in (points, view, rays, hits, col):
            a.setflags(write=False)
        _case[name] = dict(path=path, points=points, view=view, plan=plan, rays=rays, hits=hits, col=col, N=N, albedo=albedo,
                           material=material, const=const)
    return _case[name]


# tests/util_points itself: what matched when this was written -- cfg1_simple_shapes 48x32: 881 points, 1762 pairs, lit 0.766, shadowed
# while facing 0.163, turned away 0.071; area_light 48x36: 710 points, 2130 pairs, lit 0.846, shadowed 0.085, turned away 0.070.
@pytest.mark.parametrize("name,w,h", CASES)
def test_the_restated_sums_make_the_oracles_colours(oracle, tmp_path, name, w, h):
    c = case_of(oracle, name, w, h)
    plan = c["plan"]
    n = len(c["points"])
    assert plan.n == n and len(plan.shadow_rays) >= n
    hit2, t2 = OC.opaque_probe(oracle, c["path"], tmp_path, plan.shadow_rays)
    occluded = OC.expected(hit2, t2, plan.shadow_tmax)
    got = plan.reduce(occluded)
    const = c["const"]
    is_dp, want = UL.colour_identities(c["col"], c["albedo"], const["ks"], got["diffuse"], got["specular"], c["material"],
                                       const["ambient"], const["kd"])
    assert is_dp.all()
    bad = (U.bits(want) != U.bits(c["col"])).any(-1)
    lit, shadowed, away, total = plan.classes(occluded)
    print("%s %dx%d: %d points, %d differ; %d pairs, lit %.3f, shadowed while facing %.3f, turned away %.3f" % (
        name, w, h, n, bad.sum(), total, lit / total, shadowed / total, away / total))
    assert n >= 700 and (c["material"] == 3).sum() >= 150 and (c["material"] == 0).sum() >= 400
    assert min(lit, shadowed, away) >= 0.02 * total
    assert not bad.any(), "%d of %d points: the restated sums do not make the oracle's colour" % (bad.sum(), n)
    # without a view the diffuse channels are the same and nothing specular is asked of the plan
    o = oracle.OracleScene(c["path"], w, h)
    blind = UP.PointPlan(o, UL.lights_of_text(text_of(c["path"])), c["points"], None)
    o.close()
    assert np.array_equal(U.bits(blind.shadow_rays), U.bits(plan.shadow_rays))
    assert not UP.same(blind.reduce(occluded), got, ("diffuse", "light_diffuse", "light_open"))


@pytest.mark.parametrize("name,w,h", CASES)
def test_the_restated_ao_is_util_aos(oracle, tmp_path, name, w, h):
    c = case_of(oracle, name, w, h)
    n = len(c["points"])
    traced, pt, k, rays = UP.ao_traced_rays(c["points"], AO.DIRS19)
    # the frame's restatement on the rays that made the points: the same traced rays, bit for bit
    traced_f, pix, k_f, rays_f = AO.traced_rays(c["rays"], c["hits"][:, 3], c["N"], np.ones(n, bool), AO.DIRS19)
    assert np.array_equal(traced, traced_f) and np.array_equal(pt, pix) and np.array_equal(k, k_f)
    assert np.array_equal(U.bits(rays), U.bits(rays_f))
    # the zero and the NaN direction are never traced; the axes meet the planes' normals at c == 0, which is not traced either
    assert not traced[:, 16].any() and not traced[:, 17].any()
    flat = (c["N"] == f32([0, 1, 0])).all(1)
    assert flat.sum() >= 100 and not traced[flat][:, [12, 14, 15]].any() and traced[flat][:, 13].all()
    hit2, t2 = OC.opaque_probe(oracle, c["path"], tmp_path, rays)
    some = False
    for radius in (np.inf, 1.5):
        occluded = OC.expected(hit2, t2, f32(radius))
        counts, ao = UP.ao_reduce(traced, pt, occluded)
        counts_f, ao_f = AO.reduce(traced_f, pix, occluded, (n,))
        assert counts.shape == (n,) and np.array_equal(counts, counts_f) and np.array_equal(U.bits(ao), U.bits(ao_f))
        assert ((counts >> 16) == traced.sum(1)).all() and ((counts & 0xFFFF) <= (counts >> 16)).all()
        some = some or (0 < (counts & 0xFFFF).sum() < (counts >> 16).sum())
    assert some, "every traced ray has the same answer"
