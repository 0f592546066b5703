"""The input domains on which the device's powf and shading vector helpers (powfRef, reflectDir, refractDir, fresnelKr, normalized in
rendering_amd/csrc/rtx_math.h) are held to the CPU oracle, built once from fixed seeds and shared by tests/test_oracle_powf.py,
tests/test_device_math_cpu.py (what the domains reach, on the oracle alone) and tests/test_gpu_device_math.py (the device).

Comparison rule (same()): two float32 results are equal when their bits are equal, or when both are NaN of any payload and sign -- x86 and
the GPU write different default NaNs.  The signs of zeros must match.

powf
  grid      for every y of Y_LIST: x = all 256 exponents x 1024 mantissas x both signs (grid_x(), 524 288 values; the mantissas hold 0, 1,
            0x400000, 0x7FFFFF and one seeded value from each of the remaining 8192-wide strata); signalling-NaN patterns made quiet.
  sweeps    SWEEPS: all 2^23 mantissas of x at exponents 126 and 127 for y = 5, 64, 0.5, and at exponent 100 for y = 3.7.
  in y      for every x of YDOMAIN_X: y = all 256 exponents x 64 mantissas x both signs, quiet NaNs only (ydomain_y(), 32 768 values).
vectors     vector_domain(): pairs (d, n) -- seeded unit pairs, d = +-n, d perpendicular to n, d . n = +-2^-k, the unit pairs with n or d
            scaled, components replaced by special values -- and the critical-angle FANS, each with its own ior; every pair is also
            evaluated at every ior of IORS.  normalize_domain(): those vectors plus lengths whose square overflows, is a denormal or zero.
"""
import functools

import numpy as np

f32 = np.float32
u32 = np.uint32
QNAN_BIT = u32(0x00400000)


def bits(a):
    return np.ascontiguousarray(a, f32).view(u32)


def word(v):
    """the bit pattern of one float32 as an int"""
    return int(np.asarray(v, f32).reshape(1).view(u32)[0])


def same(a, b):
    """elementwise: the comparison rule of this module's docstring"""
    a = np.ascontiguousarray(a, f32); b = np.ascontiguousarray(b, f32)
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


def first_difference(x, y, got, want):
    """None, or a message naming the first (x, y) whose results differ under same(), all four numbers in hex"""
    x = np.ascontiguousarray(x, f32); y = np.ascontiguousarray(np.broadcast_to(np.asarray(y, f32), x.shape))
    bad = np.nonzero(~same(got, want).reshape(-1))[0]
    if bad.size == 0:
        return None
    k = int(bad[0])
    h = lambda a: "0x%08x" % int(bits(a).reshape(-1)[k])
    return "%d of %d differ; first at index %d: powf(x = %s, y = %s) gives %s, the oracle %s" % (bad.size, x.size, k, h(x), h(y), h(got), h(want))


def canonical(a):
    """bits with every NaN replaced by 0x7fc00000: what the digests of tests/golden/powf_domain.json are taken over"""
    a = np.ascontiguousarray(a, f32)
    return np.where(np.isnan(a), u32(0x7fc00000), bits(a)).astype(u32)


def quieted(b):
    """uint32 float patterns with every signalling NaN made quiet (bit 22 set)"""
    b = np.asarray(b, u32)
    nan = ((b & u32(0x7f800000)) == u32(0x7f800000)) & ((b & u32(0x007fffff)) != 0)
    return np.where(nan, b | QNAN_BIT, b).astype(u32)


def _y_list():
    ys = [0.0, -0.0, 1, 2, 3, 5, 10, 20, 64, 128, 149, 150, 255, 256, 1000, 1e4, 1e10,
          0.5, 3.7, 0.999, 1 + 2.0 ** -23, 1e-3, 1e-40, -1e-40,
          -0.5, -1, -2, -3, -1e10,
          2.0 ** 24, 2.0 ** 24 + 1, 2.0 ** 25,            # (2^24 + 1 as float32 is 2^24 again: every float from there on is an even integer)
          np.inf, -np.inf, np.nan]
    return np.array(ys, np.float64).astype(f32)


Y_LIST = _y_list()
SWEEPS = [(126, 5.0), (127, 5.0), (126, 64.0), (127, 64.0), (126, 0.5), (127, 0.5), (100, 3.7)]
YDOMAIN_X = np.array([0.0, 1e-40, 1e-20, 0.5, 1 - 2.0 ** -24, 1 + 2.0 ** -23, 2.0, 1e20, np.inf], np.float64).astype(f32)


def _mantissas(count, seed):
    """`count` 23-bit mantissas: 0, 1, 0x400000, 0x7FFFFF and one seeded value from each of the other equal strata (a multiplicative hash, not numpy's
    generator: the digests of tests/golden/powf_domain.json are taken over these very inputs)"""
    width = (1 << 23) // count
    k = np.arange(count, dtype=np.uint64)
    offset = (((k + np.uint64(seed)) * np.uint64(2654435761)) >> np.uint64(7)) % np.uint64(width)
    m = (k * np.uint64(width) + offset).astype(u32)
    m[0] = 0; m[1] = 1; m[count // 2] = 0x400000; m[count - 1] = 0x7FFFFF
    return m


def _all_exponents(count, seed):
    """float patterns: 256 exponents x `count` mantissas x both signs, signalling NaNs made quiet"""
    m = _mantissas(count, seed)
    e = (np.arange(256, dtype=u32) << u32(23))[:, None]
    pos = (e | m[None, :]).reshape(-1)
    return quieted(np.concatenate([pos, pos | u32(0x80000000)]))


@functools.lru_cache(None)
def grid_x():
    return _all_exponents(1024, 20350).view(f32)


@functools.lru_cache(None)
def ydomain_y():
    return _all_exponents(64, 20351).view(f32)


def sweep_x(exponent):
    return (u32(exponent << 23) | np.arange(1 << 23, dtype=u32)).view(f32)


def powf_subdomains():
    """[(name, x, y)]: every sub-domain of the powf comparison, y a scalar or an array of x's shape.  The names key tests/golden/powf_domain.json."""
    for k, y in enumerate(Y_LIST):
        yield "grid y[%02d]=0x%08x" % (k, word(y)), grid_x(), y
    for e, y in SWEEPS:
        yield "sweep e=%d y=%g" % (e, y), sweep_x(e), f32(y)
    for x in YDOMAIN_X:
        yield "in y, x=0x%08x" % word(x), np.full(ydomain_y().shape, x, f32), ydomain_y()


def signalling_nans():
    """the 8192 inputs on which the oracle's powf differs from glibc's, (x, y): 4096 signalling-NaN patterns of x (both signs) against y = +-0"""
    rng = np.random.default_rng(20352)
    m = np.unique(np.concatenate([[1, 0x3FFFFF, 0x200000], rng.integers(1, 0x400000, 4096)]).astype(u32))[:2048]
    x = np.concatenate([u32(0x7f800000) | m, u32(0xff800000) | m]).view(f32)
    return np.concatenate([x, x]), np.concatenate([np.zeros(x.size, f32), -np.zeros(x.size, f32)])


def flushed(a):
    """denormals replaced by zeros of their sign"""
    b = bits(a)
    return np.where((b & u32(0x7f800000)) == 0, b & u32(0x80000000), b).astype(u32).view(f32)


def flush_sensitive(powf_n, x, y):
    """how many inputs give another result (under same()) once x and the result are flushed to zero: what a build that flushes float32 denormals
    would get wrong.  powf_n: the oracle's array call."""
    return int((~same(flushed(powf_n(flushed(x), y)), powf_n(x, y))).sum())


# ------------------------------------------------------------------------------------------------
# vectors
# ------------------------------------------------------------------------------------------------
IORS = np.array([1.0, 1 + 2.0 ** -23, 1 - 2.0 ** -23, 1.4, 0.7, 2.5, 0.0, -1.0, 1e-30, 1e30, np.inf, np.nan], np.float64).astype(f32)
FAN_IORS = (1.05, 1.33, 1.5, 1.8, 2.5, 0.7, 0.4)
FAN_HALF = 256
FAN_STEP = 2.0 ** -22      # (the step at which the oracle's fresnel and refract turn at different j on some fan: tests/test_device_math_cpu.py)
SCALES = (0.0, 2.0 ** -10, 0.5, 2.0, 2.0 ** 10)
SPECIALS = np.array([0.0, -0.0, 1e-40, np.inf, -np.inf, np.nan], np.float64).astype(f32)


def _unit(v):
    return v / np.sqrt((v * v).sum(-1, keepdims=True))


def _rotation(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def critical_angle(ior):
    """the angle of incidence at which total internal reflection begins: asin of the ratio of the thinner to the denser index"""
    return float(np.arcsin(min(ior, 1 / ior)))


def fan(ior, side, rot=None, step=FAN_STEP, half=FAN_HALF):
    """(d, n) float32 (2 half + 1, 3): n = (0, 1, 0), d = (sin t, side cos t, 0) at t = critical angle + j step, j = -half ... half, computed in
    float64, rotated by `rot` (3 x 3) if given, then rounded"""
    t = critical_angle(ior) + np.arange(-half, half + 1, dtype=np.float64) * step
    d = np.stack([np.sin(t), side * np.cos(t), np.zeros_like(t)], 1)
    n = np.broadcast_to(np.array([0.0, 1.0, 0.0]), d.shape)
    if rot is not None:
        d = d @ rot.T; n = n @ rot.T
    return np.ascontiguousarray(d.astype(f32)), np.ascontiguousarray(n.astype(f32))


def total_reflection_side(ior):
    """the sign of d . n at which a ray meets the denser-to-thinner boundary, where total internal reflection exists: for ior > 1 the ray leaves the
    object (d . n > 0), for ior < 1 it enters it"""
    return 1 if ior > 1 else -1


@functools.lru_cache(None)
def fans(step=FAN_STEP):
    """[dict(ior, side, rotated, turns, d, n)]: per ior of FAN_IORS both sides of the surface, axis-aligned and under one seeded rotation.  turns: whether
    this is the side on which total internal reflection exists"""
    rng = np.random.default_rng(20353)
    out = []
    for ior in FAN_IORS:
        rot = _rotation(rng)
        for side in (1, -1):
            for r in (None, rot):
                d, n = fan(ior, side, r, step)
                out.append(dict(ior=f32(ior), side=side, rotated=r is not None, turns=side == total_reflection_side(ior), d=d, n=n))
    return out


@functools.lru_cache(None)
def unit_pairs(count=4096):
    rng = np.random.default_rng(20354)
    d = _unit(rng.standard_normal((count, 3))).astype(f32)
    n = _unit(rng.standard_normal((count, 3))).astype(f32)
    return d, n


@functools.lru_cache(None)
def vector_domain():
    """(d, n) float32 (m, 3): every pair but the fans' (module docstring), in a fixed order"""
    rng = np.random.default_rng(20355)
    ud, un = unit_pairs()
    D, N = [ud], [un]
    # d = +-n; d perpendicular to n (as near as float32 gets, and exactly on the axes)
    perp = _unit(np.cross(un.astype(np.float64), ud.astype(np.float64))).astype(f32)
    D += [un, -un, perp]; N += [un, un, un]
    ax = np.eye(3, dtype=f32)
    for i in range(3):
        for j in range(3):
            for s in (1, -1):
                D.append(ax[i:i + 1] * f32(s)); N.append(ax[j:j + 1])
    # d . n = +-2^-k exactly (n an axis), and the same pairs under a rotation
    k = np.arange(1, 41, dtype=np.float64)
    c = np.concatenate([2.0 ** -k, -2.0 ** -k])
    d = np.stack([np.sqrt(1 - c * c), c, np.zeros_like(c)], 1)
    n = np.broadcast_to(np.array([0.0, 1.0, 0.0]), d.shape)
    rot = _rotation(rng)
    D += [d.astype(f32), (d @ rot.T).astype(f32)]; N += [n.astype(f32), (n @ rot.T).astype(f32)]
    # the unit pairs with n scaled, and with d scaled
    for s in SCALES:
        D += [ud, ud * f32(s)]; N += [un * f32(s), un]
    # components replaced in turn by special values (the first 64 pairs)
    for comp in range(6):
        for v in SPECIALS:
            both = np.concatenate([ud[:64], un[:64]], 1).copy()
            both[:, comp] = v
            D.append(both[:, 0:3]); N.append(both[:, 3:6])
    # zero vectors
    z = np.zeros((4, 3), f32); z[1] = -z[1]
    D += [z, ud[:4], z]; N += [un[:4], z, z]
    return np.ascontiguousarray(np.concatenate(D), f32), np.ascontiguousarray(np.concatenate(N), f32)


@functools.lru_cache(None)
def normalize_domain():
    """float32 (m, 3): the vectors of vector_domain() and of the fans; vectors whose squared length overflows (components near 1e20), is a denormal (1e-20)
    or zero (1e-23); single-component vectors at every exponent"""
    rng = np.random.default_rng(20356)
    d, n = vector_domain()
    V = [d, n] + [f["d"] for f in fans()]
    u = unit_pairs()[0][:512]
    for s in (1e20, 1e-20, 1e-23, 3e38, 1.5e-19, 1e-45):
        V.append(u * f32(s))
    e = 2.0 ** np.arange(-149, 128, dtype=np.float64)
    mag = np.concatenate([e, e * (1 + rng.random(e.size)), [0.0, np.inf, np.nan]]).astype(f32)
    for axis in range(3):
        for s in (1, -1):
            v = np.zeros((mag.size, 3), f32)
            v[:, axis] = mag * f32(s)
            V.append(v)
    return np.ascontiguousarray(np.concatenate(V), f32)


VEC_OPS = ("reflect", "refract", "fresnel", "normalize")


def oracle_vec(O, op, d, n=None, ior=1.0):
    """the oracle's array call of vec_probe's op (0 reflect, 1 refract, 2 fresnel, 3 normalize) in vec_probe's output layout: fresnel in column 0"""
    if op == 0:
        return O.reflect_n(d, n)
    if op == 1:
        return O.refract_n(d, n, ior)
    if op == 2:
        out = np.zeros(np.asarray(d).reshape(-1, 3).shape, f32)
        out[:, 0] = O.fresnel_n(d, n, ior)
        return out
    return O.normalize_n(d)


def vector_cases():
    """[(label, op, d, n, ior)]: every call of the vector comparison -- reflect once, refract and fresnel at every ior of IORS on vector_domain() and at each
    fan's own ior (and at IORS) on the fans, normalize on normalize_domain()"""
    d, n = vector_domain()
    fs = fans()
    fd = np.concatenate([f["d"] for f in fs]); fn = np.concatenate([f["n"] for f in fs])
    out = [("reflect", 0, np.concatenate([d, fd]), np.concatenate([n, fn]), f32(1))]
    for op in (1, 2):
        for ior in IORS:
            out.append(("%s ior=%r" % (VEC_OPS[op], float(ior)), op, np.concatenate([d, fd]), np.concatenate([n, fn]), ior))
        for ior in FAN_IORS:
            mine = [f for f in fs if f["ior"] == f32(ior)]
            out.append(("%s fans of ior=%r" % (VEC_OPS[op], ior), op, np.concatenate([f["d"] for f in mine]), np.concatenate([f["n"] for f in mine]), f32(ior)))
    out.append(("normalize", 3, normalize_domain(), None, f32(1)))
    return out


def first_vector_difference(label, d, n, got, want):
    ok = same(got, want).all(1)
    if ok.all():
        return None
    k = int(np.nonzero(~ok)[0][0])
    hx = lambda v: "(" + ", ".join("0x%08x" % int(b) for b in bits(v)) + ")"
    return "%s: %d of %d differ; first at index %d: d = %s, n = %s gives %s, the oracle %s" % (
        label, int((~ok).sum()), len(ok), k, hx(d[k]), hx(n[k]) if n is not None else "-", hx(got[k]), hx(want[k]))


# ------------------------------------------------------------------------------------------------
# the same exponents through the API: two small scenes per n_specular, and points for Scene.light_points
# ------------------------------------------------------------------------------------------------
API_W, API_H = 40, 32
N_SPECULAR = ("0", "0.5", "-1.5", "300.25", "10000")      # (as written into the scene file; every loader takes all five)
API_KINDS = ("analytic", "mesh")
POINT_LIGHT = (0.0, 0.0, 0.0)       # (at the origin, where a point 1e-20 away is still another float: at 0.5 it would round onto the light)
N_POINTS = 4096
N_AT_LIGHT = 64

_API_LIGHTS = """[light]
type=point
position=%g,%g,%g
color=1,0.9,0.8
intensity=0.9

[light]
type=point
position=-1,1.5,-1
color=1,1,1
intensity=0

[light]
type=distant
direction=0.3,-1,-0.2
color=0.6,0.7,1
intensity=0.4

[light]
type=area
pos=-1.5,2,-2
i=1,0,0
j=0,0,1
samples=2
color=1,1,1
intensity=2.0

""" % POINT_LIGHT


def api_scene_text(kind, ns):
    """A Phong sphere on a Phong plane ("analytic"), or the Phong mesh bumpy_4k.obj on that plane ("mesh"), both with exponent `ns` (text), under a point
    light, a point light of intensity 0, a distant light and an area light of 2 x 2 samples: the general shading kernels, whose every term has a powf"""
    head = "[options]\nwidth=%d\nheight=%d\nfov=60\nimage_name=output/device_math_%s\n\n" % (API_W, API_H, kind)
    plane = "[object]\ntype=plane\npos=0,-1.5,0\nnormal=0,1,0\ncolor=0.9,0.9,0.9\nmaterial=phong,0.1,0.6,0.5,%s\n\n" % ns
    if kind == "analytic":
        body = "[object]\ntype=sphere\npos=0,0,-3\nradius=1\ncolor=0.9,0.4,0.3\nmaterial=phong,0.2,0.5,0.7,%s\n\n" % ns
    else:
        body = "[object]\ntype=mesh\npos=0,0,-3\nsize=2,2,2\ncolor=0.4,0.8,0.5\nmaterial=phong,0.2,0.5,0.7,%s\nname=scenes/assets/bumpy_4k.obj\n\n" % ns
    return head + _API_LIGHTS + plane + body + "[end]\n"


def write_api_scenes(dst):
    """{(kind, ns): path} of the ten scene files, written into dst"""
    import os
    out = {}
    for kind in API_KINDS:
        for k, ns in enumerate(N_SPECULAR):
            out[kind, ns] = os.path.join(str(dst), "dm_%s_%d.scene" % (kind, k))
            with open(out[kind, ns], "w") as f:
                f.write(api_scene_text(kind, ns))
    return out


def api_rays(o):
    """the primary rays of the frame, then 2048 seeded probe rays"""
    from tests import util_aov as U
    from tests.util_rays import probe_rays
    return np.ascontiguousarray(np.concatenate([U.primary_rays(o), probe_rays(2048)]), f32)


def light_point_inputs(O, mesh_scene_path):
    """(points (4096, 6) {P, N}, view (4096, 4) {V, ns}) for Scene.light_points on the mesh scene, from the oracle alone.
    P, N   the first hits of a 96 x 72 grid of camera rays, cycled, with N the unit vector from the mesh's centre (the plane's: its normal) -- any N is
           "as stored"; the last 128: 64 points exactly at the point light (squared distance 0) and 64 at 1e-20 from it (squared distance a denormal).
    ns     Y_LIST, cycled per point.
    V      per block of 35 points one of eight kinds, placed against R = reflect(L, N) of the point light so that x = R . -V is: <= 0; 0 up to rounding;
           2^-k, k cycling through 1 ... 40 (three kinds); within 2^-20 of 1 (two kinds); and (one eighth) 0.9 scaled by 2^10, 2^-10, 1e20, 3e38 (the
           dot product overflows: x = +inf), 1e-39 and 2^-130 (x a denormal)."""
    from tests import util_aov as U
    rng = np.random.default_rng(20357)
    o = O.OracleScene(mesh_scene_path, 96, 72)
    rays = U.primary_rays(o)
    hits, _ = o.probe(rays, colours=False)
    o.close()
    hit = np.nonzero(hits[:, 0] > 0)[0]
    n_hit = N_POINTS - 2 * N_AT_LIGHT
    pick = hit[(np.arange(n_hit) * 7919) % len(hit)]
    with np.errstate(all="ignore"):
        P = (rays[pick, 0:3] + rays[pick, 3:6] * hits[pick, 3:4]).astype(f32)
    on_mesh = hits[pick, 1] == 1
    N = np.where(on_mesh[:, None], _unit(P.astype(np.float64) - np.array([0.0, 0.0, -3.0])), np.array([0.0, 1.0, 0.0])).astype(f32)
    light = np.array(POINT_LIGHT, f32)
    u = _unit(rng.standard_normal((2 * N_AT_LIGHT, 3)))
    P = np.concatenate([P, np.broadcast_to(light, (N_AT_LIGHT, 3)), (light + 1e-20 * u[N_AT_LIGHT:]).astype(f32)]).astype(f32)
    N = np.concatenate([N, u.astype(f32)])
    i = np.arange(N_POINTS)
    ns = Y_LIST[i % len(Y_LIST)]
    kind, sub = (i // len(Y_LIST)) % 8, i // (8 * len(Y_LIST))
    # R of the point light, from the oracle's own normalize and reflect
    R = O.reflect_n(O.normalize_n(P - light), N).astype(np.float64)
    bad = ~(np.abs(np.sqrt((R * R).sum(1)) - 1) < 0.5)           # (at the light L is 0 and so is R: V against any unit vector)
    assert bad.sum() == N_AT_LIGHT
    R[bad] = u[:N_AT_LIGHT]
    R = _unit(R)
    T = _unit(np.cross(R, rng.standard_normal((N_POINTS, 3))))
    k = 1 + (sub * 3 + kind) % 40
    c = np.select([kind == 0, kind == 1, (kind >= 2) & (kind <= 4), (kind == 5) | (kind == 6)],
                  [-0.5, 0.0, 2.0 ** -k, 1 - rng.random(N_POINTS) * 2.0 ** -20], 0.9)
    V = -(c[:, None] * R + np.sqrt(1 - c * c)[:, None] * T)
    scale = np.where(kind == 7, np.array([2.0 ** 10, 2.0 ** -10, 1e20, 3e38, 1e-39, 2.0 ** -130])[sub % 6], 1.0)
    V = (V.astype(f32) * scale.astype(f32)[:, None]).astype(f32)
    return (np.ascontiguousarray(np.concatenate([P, N], 1), f32), np.ascontiguousarray(np.concatenate([V, ns[:, None]], 1), f32))


def same_channels(got, want, channels):
    """{channel: number of rows that differ under same()} over the channels that differ; integer channels compare exactly"""
    out = {}
    for c in channels:
        a, b = np.asarray(got[c]), np.asarray(want[c])
        assert a.shape == b.shape, (c, a.shape, b.shape)
        ok = same(a, b) if a.dtype == f32 else (a == b)
        if not ok.all():
            out[c] = int((~ok).reshape(len(a), -1).any(1).sum())
    return out


def light_points_plan(O, path, lights, points, view):
    """tests/util_points.PointPlan of the points in the scene file `path`; lights: (records, points) as Scene.device_lights() or util_light.lights_of_text()"""
    from tests import util_points as UP
    o = O.OracleScene(path, API_W, API_H)
    plan = UP.PointPlan(o, lights, points, view)
    o.close()
    return plan


def specular_inputs(O, plan, occluded):
    """per light (x (n,), open (n,) bool): powf's first argument at every point -- max0(R . -V) of a point or distant light, the mean of it over the open
    samples of an area light -- and whether a shadow ray of the light arrives (tests/util_light.Plan.reduce's own steps)"""
    from tests import util_light as UL
    occluded = np.asarray(occluded).reshape(-1)
    n, at, out = plan.n, 0, []
    with np.errstate(all="ignore"):
        for li, (I, L, dist) in enumerate(plan.lights):
            S = L.shape[1]
            opened = occluded[at:at + n * S].reshape(S, n).T == 0
            at += n * S
            Nb = np.ascontiguousarray(np.broadcast_to(plan.N[:, None, :], L.shape))
            R = O.reflect_n(np.ascontiguousarray(L), Nb).reshape(L.shape)
            sd = UL.max0(UL.dot(R, -np.broadcast_to(plan.dir[:, None, :], L.shape)))
            if plan.recs[li]["type"] == UL.AREA:
                ssum = np.zeros(n, f32)
                for k in range(S):
                    ssum = (ssum + opened[:, k].astype(f32) * sd[:, k]).astype(f32)
                out.append(((ssum / f32(S)).astype(f32), opened.any(1)))
            else:
                out.append((sd[:, 0], opened[:, 0]))
    return out
