"""What the domains of tests/util_device_math.py reach, shown on the CPU oracle alone -- so that tests/test_gpu_device_math.py, which holds the device to
the oracle on them, is a test of every branch of powf and of the shading vector helpers and not of a comfortable sample.

  census       the oracle's powf on the grid lands at least 1000 times in every class of result: +-0, +-denormal, +-normal, +-inf, NaN, exactly 1 from
               x != 1 and y != 0, the 2^-149 of the "may underflow" branch (-150 < y log2 x < -149), a finite non-zero result from a denormal x.
  flushing     at least 10 000 grid inputs change their result when x and the result are flushed to zero: a build that flushes float32 denormals fails.
  fans         on every critical-angle fan on the side where total internal reflection exists, the oracle's fresnel reaches 1 and its refract the zero
               vector strictly inside the fan; on at least one fan at different j (two roundings of one condition: the zone in which scatter_rays'
               two rays need not both exist); on the other side of the surface neither happens.
  reference    where oracle/_ref is built, the oracle's reflect, refract, fresnel and normalize equal the reference's over the whole vector domain.

  api          the scenes and light_points inputs of the GPU module's second half: the restated attenuation gives the oracle's min(1, x) for x = +inf and NaN;
               for every exponent at least a quarter of its points carry powf's value into the output (measured 0.778 - 0.855); at least 100 of the (x, ns)
               pairs change under flushing (207); where oracle/_ref is built, the oracle's pass 1 of the ten scenes is the reference's.

Measured on the grid (18 350 080 inputs): +0 4 667 877, -0 516 430, +denormal 91 456, -denormal 24 523, +normal 4 308 317, -normal 747 059, +inf 4 775 872,
-inf 539 835, NaN 2 678 711, exactly 1 522 257, may-underflow 2^-149 4 363, denormal x 14 835; sensitive to flushing 130 900.  Fans whose two conditions turn one
direction apart at step 2^-22: ior 1.05 leaving the object (axis-aligned and rotated), ior 0.7 entering it.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import util_device_math as DM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref", "libref_harness.so")
f32 = np.float32


def census(oracle):
    x = DM.grid_x()
    xb = DM.bits(x)
    count = dict.fromkeys(["+0", "-0", "+denormal", "-denormal", "+normal", "-normal", "+inf", "-inf", "nan", "one", "may_underflow", "denormal_x"], 0)
    with np.errstate(all="ignore"):
        log2x = np.log2(np.abs(x.astype(np.float64)))
    x_denormal = ((xb & 0x7f800000) == 0) & ((xb & 0x007fffff) != 0)
    for y in DM.Y_LIST:
        r = oracle.powf_n(x, y)
        b = DM.bits(r)
        mag, neg = b & np.uint32(0x7fffffff), (b >> np.uint32(31)) != 0
        for sign, m in (("+", ~neg), ("-", neg)):
            count[sign + "0"] += int((m & (mag == 0)).sum())
            count[sign + "denormal"] += int((m & (mag != 0) & (mag < 0x00800000)).sum())
            count[sign + "normal"] += int((m & (mag >= 0x00800000) & (mag < 0x7f800000)).sum())
            count[sign + "inf"] += int((m & (mag == 0x7f800000)).sum())
        count["nan"] += int((mag > 0x7f800000).sum())
        finite_nonzero = (mag != 0) & (mag < 0x7f800000)
        if y != 0 and not np.isnan(y):
            count["one"] += int(((b == 0x3f800000) & (x != 1)).sum())
        with np.errstate(all="ignore"):
            ylogx = np.float64(y) * log2x
            count["may_underflow"] += int(((mag == 1) & (ylogx > -150) & (ylogx < -149)).sum())
        count["denormal_x"] += int((x_denormal & finite_nonzero).sum())
    return count


def test_census_of_the_grid(oracle):
    count = census(oracle)
    print("census of the oracle's powf on the grid:", count)
    short = {k: v for k, v in count.items() if v < 1000}
    assert not short, "classes of result the grid reaches fewer than 1000 times: %s" % short


def test_grid_is_sensitive_to_denormal_flushing(oracle):
    x = DM.grid_x()
    n = sum(DM.flush_sensitive(oracle.powf_n, x, y) for y in DM.Y_LIST)
    print("grid inputs whose result changes under flushing:", n)
    assert n >= 10000


def test_domains_are_what_the_module_says():
    x = DM.grid_x()
    assert x.size == 256 * 1024 * 2 and np.unique(DM.bits(x)).size == x.size
    m = set((DM.bits(x)[:1024] & 0x7fffff).tolist())
    assert {0, 1, 0x400000, 0x7FFFFF} <= m and len(m) == 1024
    nan = np.isnan(x)
    assert nan.sum() == 2 * 1023 and (DM.bits(x[nan]) & DM.QNAN_BIT != 0).all()         # (quiet ones only)
    yy = DM.ydomain_y()
    assert yy.size == 256 * 64 * 2 and (DM.bits(yy[np.isnan(yy)]) & DM.QNAN_BIT != 0).all()
    assert DM.Y_LIST.size == 35 and np.isnan(DM.Y_LIST[-1]) and np.signbit(DM.Y_LIST[1]) and DM.Y_LIST[1] == 0
    assert [DM.sweep_x(e).size for e, _ in DM.SWEEPS] == [1 << 23] * 7
    d, n = DM.vector_domain()
    # unit pairs, d = n, d = -n, perpendicular; axes; d . n = +-2^-k twice; n or d scaled; special components; zero vectors
    assert d.shape == n.shape and d.shape[0] == 4 * 4096 + 18 + 2 * 80 + 2 * len(DM.SCALES) * 4096 + 6 * len(DM.SPECIALS) * 64 + 12
    assert len(DM.fans()) == len(DM.FAN_IORS) * 4 and all(f["d"].shape == (2 * DM.FAN_HALF + 1, 3) for f in DM.fans())
    v = DM.normalize_domain()
    with np.errstate(all="ignore"):
        l2 = ((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]).astype(f32)
    nz = (v != 0).any(1)
    tiny = DM.bits(l2) & np.uint32(0x7f800000) == 0
    assert (np.isinf(l2) & np.isfinite(v).all(1)).sum() >= 512, "squared lengths that overflow"
    assert (tiny & (l2 != 0)).sum() >= 512, "squared lengths that are denormals"
    assert (nz & (l2 == 0)).sum() >= 512, "squared lengths that underflow to zero"


def turning_points(oracle, fan):
    """(first j at which fresnel is 1, first j at which refract is the zero vector, whether both stay so from there on); None where it never happens"""
    kr = oracle.fresnel_n(fan["d"], fan["n"], fan["ior"])
    t = oracle.refract_n(fan["d"], fan["n"], fan["ior"])
    total = kr == 1
    gone = (DM.bits(t) == 0).all(1)
    j = lambda m: int(np.argmax(m)) - DM.FAN_HALF if m.any() else None
    return j(total), j(gone), total, gone


def test_fans_cross_the_critical_angle(oracle):
    apart = []
    for f in DM.fans():
        jk, jt, total, gone = turning_points(oracle, f)
        label = "ior %g side %+d %s" % (f["ior"], f["side"], "rotated" if f["rotated"] else "axis")
        if not f["turns"]:
            assert jk is None and jt is None, "%s: total reflection on the side that has none" % label
            continue
        assert jk is not None and -DM.FAN_HALF < jk < DM.FAN_HALF, "%s: fresnel reaches 1 at j = %s" % (label, jk)
        assert jt is not None and -DM.FAN_HALF < jt < DM.FAN_HALF, "%s: refract gives the zero vector at j = %s" % (label, jt)
        assert not total[0] and not gone[0] and total[-1] and gone[-1], label
        if (total != gone).any():
            apart.append((label, jk, jt, int((total != gone).sum())))
    print("fans on which fresnel = 1 and refract = 0 disagree at step 2^%d (label, j of fresnel, j of refract, directions):" % int(np.log2(DM.FAN_STEP)), apart)
    assert apart, "no fan on which the two conditions turn at different directions: halve util_device_math.FAN_STEP"


def test_batch_vector_calls_are_the_scalar_calls(oracle):
    d, n = DM.vector_domain()
    pick = np.arange(0, d.shape[0], 97)
    for ior in DM.IORS:
        kr = oracle.fresnel_n(d[pick], n[pick], ior)
        t = oracle.refract_n(d[pick], n[pick], ior)
        for k, i in enumerate(pick):
            assert DM.same(kr[k], oracle.fresnel(d[i], n[i], float(ior))).all()
            assert DM.same(t[k], oracle.refract(d[i], n[i], float(ior))).all()
    r = oracle.reflect_n(d[pick], n[pick]); v = oracle.normalize_n(d[pick])
    for k, i in enumerate(pick):
        assert DM.same(r[k], oracle.reflect(d[i], n[i])).all() and DM.same(v[k], oracle.normalize(d[i])).all()


VEC_CHILD = r"""
import ctypes as C, sys, numpy as np
sys.path.insert(0, %r)
from tools import ref_harness as R
from oracle import oracle as O
from tests import util_device_math as DM
lib = R.lib()
lib.ref_reflect.argtypes = [C.c_void_p] * 3
lib.ref_normalize.argtypes = [C.c_void_p] * 2


def reference(op, d, n, ior):
    # the harness's scalar calls on element i of the arrays (addresses: one ctypes call per element and nothing else)
    d = np.ascontiguousarray(d, np.float32).reshape(-1, 3)
    out = np.zeros_like(d)
    pd, po = d.ctypes.data, out.ctypes.data
    if op == 3:
        f = lib.ref_normalize
        for at in range(0, 12 * len(d), 12):
            f(pd + at, po + at)
        return out
    n = np.ascontiguousarray(n, np.float32).reshape(-1, 3)
    pn, ior = n.ctypes.data, float(ior)
    if op == 0:
        f = lib.ref_reflect
        for at in range(0, 12 * len(d), 12):
            f(pd + at, pn + at, po + at)
    elif op == 1:
        f = lib.ref_refract
        for at in range(0, 12 * len(d), 12):
            f(pd + at, pn + at, ior, po + at)
    else:
        f = lib.ref_fresnel
        out[:, 0] = [f(pd + at, pn + at, ior) for at in range(0, 12 * len(d), 12)]
    return out


calls = 0
for label, op, d, n, ior in DM.vector_cases():
    want = reference(op, d, n, ior); got = DM.oracle_vec(O, op, d, n, ior)
    msg = DM.first_vector_difference(label, d, n, got, want)
    assert msg is None, msg + ' (first result: the oracle, second: the reference)'
    calls += 1
print('OK', calls)
"""


@pytest.mark.skipif(not os.path.exists(REF), reason="oracle/_ref is not built here")
def test_oracle_vector_helpers_equal_the_reference_on_the_whole_domain():
    out = subprocess.run([sys.executable, "-c", VEC_CHILD % ROOT], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


# ---- the same exponents through the API (tests/test_gpu_device_math.py, second half) ------------------------------------------------------------
@pytest.fixture(scope="module")
def api_scenes(tmp_path_factory):
    return DM.write_api_scenes(tmp_path_factory.mktemp("dm"))


def test_restated_attenuation_is_the_oracles_at_the_ends(oracle, api_scenes):
    """tests/util_light.attenuation (float64 in numpy, what util_points.PointPlan gives an area light) against the oracle's fmin(1, (float)(intensity /
    (4 pi l2 / 1000))) of the two point lights where the quotient is +inf (l2 = 0, a denormal), NaN (0 / 0: the light of intensity 0 at l2 = 0; a NaN or
    infinite P), 0 (l2 = +inf) and in between: min(1, x) = x < 1 ? x : 1 gives 1 for +inf and for NaN"""
    from tests import util_light as UL
    path = api_scenes["mesh", "0.5"]
    o = oracle.OracleScene(path, DM.API_W, DM.API_H)
    text = open(path).read()
    blocks = UL.light_blocks(text)
    for li in (0, 1):
        pos = np.array([float(v) for v in blocks[li]["position"].split(",")], f32)
        intensity = f32(blocks[li]["intensity"])
        color = np.array([float(v) for v in blocks[li]["color"].split(",")], f32)
        off = np.array([[0, 0, 0], [1e-20, 0, 0], [0, 1e-23, 0], [1e-10, 0, 0], [0.05, 0, 0], [1, 2, 3], [1e19, 1e19, 0], [1e20, 0, 0],
                        [np.inf, 0, 0], [np.nan, 0, 0], [3e38, 3e38, 3e38]], f32)
        P = (pos + off).astype(f32)
        with np.errstate(all="ignore"):
            d0 = (P - pos).astype(f32)
            att = UL.attenuation(intensity, UL.dot(d0, d0))
            want = (color[None, :] * att[:, None]).astype(f32)
        got = o.illuminate(li, P)[:, 3:6]
        assert DM.same(got, want).all(), (li, got, want)
        if li == 0:
            assert (att[:3] == 1).all() and att[8] == 0 and att[9] == 1
        else:
            assert (att[:4] == 1).all() and (att[4:9] == 0).all()         # (the small offsets round onto this light: 0 / 0 = NaN -> 1; else 0 / l2 = 0)
    o.close()


_points = {}


def light_points_case(oracle, api_scenes, tmp_path_factory):
    if not _points:
        from tests import util_light as UL
        from tests import util_occlusion as OC
        path = api_scenes["mesh", "0.5"]
        points, view = DM.light_point_inputs(oracle, path)
        plan = DM.light_points_plan(oracle, path, UL.lights_of_text(open(path).read()), points, view)
        hit, t = OC.opaque_probe(oracle, path, tmp_path_factory.mktemp("opaque"), plan.shadow_rays)
        occ = OC.expected(hit, t, plan.shadow_tmax)
        _points.update(points=points, view=view, plan=plan, occ=occ, inputs=DM.specular_inputs(oracle, plan, occ))
    return _points


def test_light_point_inputs_let_powf_reach_the_output(oracle, api_scenes, tmp_path_factory):
    """for every exponent of the list, at least a quarter of its points have, for some light, an open shadow ray and x > 0: there powf's value is in the
    output.  And the inputs are what the builder says: points at the light and 1e-20 from it, x <= 0, tiny, next to 1, above 1, +inf and denormal."""
    c = light_points_case(oracle, api_scenes, tmp_path_factory)
    points, view = c["points"], c["view"]
    assert points.shape == (DM.N_POINTS, 6) and view.shape == (DM.N_POINTS, 4)
    ns = view[:, 3]
    reach = np.zeros(DM.N_POINTS, bool)
    for x, opened in c["inputs"]:
        reach |= opened & (x > 0)
    share = []
    for k in range(len(DM.Y_LIST)):
        mine = np.arange(DM.N_POINTS) % len(DM.Y_LIST) == k
        assert DM.same(ns[mine], np.full(mine.sum(), DM.Y_LIST[k], f32)).all()
        share.append(float(reach[mine].mean()))
    print("share of points per exponent at which powf's value reaches the output: min %.3f, max %.3f" % (min(share), max(share)))
    assert min(share) >= 0.25, share
    light = np.array(DM.POINT_LIGHT, f32)
    with np.errstate(all="ignore"):
        d0 = points[:, 0:3] - light
        l2 = ((d0[:, 0] * d0[:, 0] + d0[:, 1] * d0[:, 1]) + d0[:, 2] * d0[:, 2]).astype(f32)
    assert (l2 == 0).sum() == DM.N_AT_LIGHT
    assert ((l2 != 0) & (DM.bits(l2) < 0x00800000)).sum() == DM.N_AT_LIGHT
    x0 = c["inputs"][0][0]
    xs = np.concatenate([x for x, _ in c["inputs"]])
    assert (x0 == 0).sum() >= 400 and ((x0 > 0) & (x0 < 2.0 ** -20)).sum() >= 300 and ((x0 > 1 - 2.0 ** -19) & (x0 <= 1)).sum() >= 300
    assert (xs > 1).sum() >= 100 and np.isinf(xs).sum() >= 20 and ((xs != 0) & (DM.bits(xs) < 0x00800000)).sum() >= 100


def test_light_point_inputs_are_sensitive_to_denormal_flushing(oracle, api_scenes, tmp_path_factory):
    c = light_points_case(oracle, api_scenes, tmp_path_factory)
    ns = c["view"][:, 3]
    n = sum(DM.flush_sensitive(oracle.powf_n, x, ns) for x, _ in c["inputs"])
    print("light_points inputs (x, ns) whose powf changes under flushing:", n)
    assert n >= 100


API_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, %r)
from tools import ref_harness as R
from oracle import oracle as O
from tests import util_device_math as DM
for path in sys.argv[1:]:
    r = R.RefScene(path, DM.API_W, DM.API_H); o = O.OracleScene(path, DM.API_W, DM.API_H)
    fr = r.pass1(); fo = o.pass1()
    assert DM.same(fr, fo).all(), ('pass1', path, int((~DM.same(fr, fo)).any(-1).sum()))
    o.close()
print('OK')
"""


@pytest.mark.skipif(not os.path.exists(REF), reason="oracle/_ref is not built here")
def test_oracle_pass1_of_the_api_scenes_equals_the_reference(api_scenes):
    """every exponent of util_device_math.N_SPECULAR is taken by the reference's loader, and its frames -- NaN and inf pixels included -- are the oracle's"""
    out = subprocess.run([sys.executable, "-c", API_CHILD % ROOT] + list(api_scenes.values()), cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
