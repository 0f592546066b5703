"""The device's powf and shading vector helpers (powfRef, reflectDir, refractDir, fresnelKr, normalized in rendering_amd/csrc/rtx_math.h, through
rendering_amd.math_probe(0, ...) and vec_probe(0..3, ...)) against the CPU oracle's array calls over the whole domains of tests/util_device_math.py, under
that module's comparison rule: equal bits, or both NaN.  tests/test_oracle_powf.py pins the oracle's powf to glibc 2.35 on the same inputs and
tests/test_device_math_cpu.py shows that the inputs reach every branch.

The second half sends the same exponents through the API: as a scene's n_specular (every loader takes 0, 0.5, -1.5, 300.25 and 1e4: none was dropped) and as the
ns of Scene.light_points' view records.

Measured on an MI355X, seconds per test: the grid 0.47 (35 launches of 524 288), each sweep of 2^23 mantissas 0.12, powf in y under 0.01, the vector helpers 0.06,
each of the ten scenes 0.14 - 0.20, light_points 0.30; test_gpu_parity.py::test_device_math_matches_host over all of its elements 0.03.  No difference was found.
"""
import numpy as np
import pytest

from tests import util_device_math as DM

pytestmark = pytest.mark.gpu


def test_powf_grid(ra, oracle):
    """every exponent of x, both signs, 1024 mantissas, one launch per y of the list"""
    x = DM.grid_x()
    for y in DM.Y_LIST:
        msg = DM.first_difference(x, y, ra.math_probe(0, x, y), oracle.powf_n(x, y))
        assert msg is None, msg


@pytest.mark.parametrize("exponent,y", DM.SWEEPS)
def test_powf_every_mantissa(ra, oracle, exponent, y):
    x = DM.sweep_x(exponent)
    msg = DM.first_difference(x, y, ra.math_probe(0, x, np.float32(y)), oracle.powf_n(x, y))
    assert msg is None, msg


def test_powf_in_y(ra, oracle):
    """every exponent of y, both signs, 64 mantissas, for nine x"""
    y = DM.ydomain_y()
    for x0 in DM.YDOMAIN_X:
        x = np.full(y.shape, x0, np.float32)
        msg = DM.first_difference(x, y, ra.math_probe(0, x, y), oracle.powf_n(x, y))
        assert msg is None, msg


def test_vector_helpers(ra, oracle):
    """reflect; refract and fresnel at every ior of the list and on the critical-angle fans at their own; normalize"""
    for label, op, d, n, ior in DM.vector_cases():
        got = ra.vec_probe(op, d, n, float(ior))
        if op == 2:
            assert not got[:, 1:].any()
        msg = DM.first_vector_difference(label, d, n, got, DM.oracle_vec(oracle, op, d, n, ior))
        assert msg is None, msg


# ---- the same exponents through the API ----------------------------------------------------------------------------------------------------------
# powf's y reaches the device as a scene's n_specular and as the ns of Scene.light_points' view records.  tests/test_device_math_cpu.py shows on the
# oracle that these inputs let powf's value reach the output, and, where the reference is built, that the oracle's frames of the scenes are its own.
@pytest.fixture(scope="module")
def api_scenes(tmp_path_factory):
    return DM.write_api_scenes(tmp_path_factory.mktemp("dm"))


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, np.float32, order="C")).cuda()


def host(out):
    import torch
    torch.cuda.synchronize()
    return {c: t.cpu().numpy() for c, t in out.items()}


@pytest.mark.parametrize("ns", DM.N_SPECULAR)
@pytest.mark.parametrize("kind", DM.API_KINDS)
def test_exponents_through_frames_and_rays(ra, oracle, api_scenes, kind, ns):
    """pass 1, trace_rays of the primary rays and 2048 probe rays, and light_rays(per_light=True) of a 40 x 32 scene whose Phong objects have n_specular
    `ns`, under a point light, one of intensity 0, a distant and an area light.  With ns = -1.5 most pixels are inf or NaN, on both sides."""
    from tests import util_ao as AO
    from tests import util_light as UL
    path = api_scenes[kind, ns]
    o = oracle.OracleScene(path, DM.API_W, DM.API_H)
    g = ra.Scene(path, DM.API_W, DM.API_H)
    objs, _ = g.device_objects()
    assert DM.same(objs["n_specular"], np.full(len(objs), np.float32(ns))).all()
    want, got = o.pass1(), g.render_host(ssaa=False)
    bad = ~DM.same(got, want).all(-1)
    assert not bad.any(), "pass 1: %d pixels differ, first at %s" % (bad.sum(), np.argwhere(bad)[0])
    rays = DM.api_rays(o)
    rh, rc = o.probe(rays)
    hits, colours = g.trace_rays(dev(rays))
    s = host(g.surface_rays(dev(rays), hits=True, normal=True, albedo=False))
    hits, colours = hits.cpu().numpy(), colours.cpu().numpy()
    assert np.array_equal(DM.bits(hits), DM.bits(rh)), "trace_rays: hit records"
    bad = ~DM.same(colours, rc).all(-1)
    assert not bad.any(), "trace_rays: %d colours differ, first at ray %d: %r, the oracle %r" % (bad.sum(), np.argmax(bad), colours[np.argmax(bad)], rc[np.argmax(bad)])
    # light_rays against tests/util_light's restatement: the exact N from surface_rays, visibility from Scene.occluded (neither is the code under test)
    import torch
    plan = UL.Plan(o, g.device_lights(), rays, s["hits"], s["normal"], bias=AO.BIAS)
    occ = g.occluded(dev(plan.shadow_rays), dev(plan.shadow_tmax))
    torch.cuda.synchronize()
    obj = s["hits"][:, 1].astype(np.int32)
    exp = plan.reduce(occ.cpu().numpy(), np.where(obj >= 0, objs["n_specular"][np.maximum(obj, 0)], np.float32(0)).astype(np.float32))
    exp["hits"] = rh
    lr = host(g.light_rays(dev(rays), hits=True, per_light=True))
    bad = DM.same_channels(lr, exp, UL.CHANNELS)
    assert not bad, "light_rays: rays whose channels differ from the expectation: %s" % bad
    o.close()
    g.close()


def test_exponents_through_light_points(ra, oracle, api_scenes, tmp_path):
    """Scene.light_points on the mesh scene at 4096 points whose ns cycle through the whole y list of the grid, with V placed against the point light's R
    so that x is <= 0, 2^-k, next to 1, above 1, +inf and a denormal; 64 points at the point light and 64 at 1e-20 from it (a flushed squared length
    would leave L unnormalised).  Expectation: tests/util_points.PointPlan with the oracle's visibility."""
    from tests import util_occlusion as OC
    from tests import util_points as UP
    path = api_scenes["mesh", "0.5"]
    points, view = DM.light_point_inputs(oracle, path)
    g = ra.Scene(path, DM.API_W, DM.API_H)
    plan = DM.light_points_plan(oracle, path, g.device_lights(), points, view)
    hit, t = OC.opaque_probe(oracle, path, tmp_path, plan.shadow_rays)
    exp = plan.reduce(OC.expected(hit, t, plan.shadow_tmax))
    got = host(g.light_points(dev(points), dev(view), per_light=True))
    bad = DM.same_channels(got, exp, UP.CHANNELS)
    assert not bad, "light_points: points whose channels differ from the expectation: %s" % bad
    sums = host(g.light_points(dev(points), dev(view), per_light=False))
    assert not DM.same_channels(sums, exp, UP.SUMS)
    g.close()
