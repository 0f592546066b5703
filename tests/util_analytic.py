"""Scenes and rays aimed at the margins of the analytic branch of the walk (rtx_kernels.hip traceWave: Sphere::intersectObject /
Plane::intersectObject, objects.cpp:774-786, 807-814; Render::trace, scene.cpp:724-756), where the mesh side has tests/test_gpu_margins.py:
  d2 = L.L - tca tca cancels, sqrtf and the division are correctly rounded, fabs(denom) < 1e-8 is compared in double, t0 < 0 picks the
  second root, t0 >= 0 accepts -0, and between objects the strict t0 < tNear lets the first object in scene order win.

Scene forms (FORMS; small .scene texts written to a directory, 48 x 32, a point and a distant light, a background that is not black):
  spheres, materials, with_mesh_cull / with_mesh_nocull, planes, extremes, and the ties -- two coincident spheres, a sphere tangent to a
  plane, two coincident planes, a lattice quad lying in a plane -- each in BOTH object orders (tie_*_ab / tie_*_ba).
Ray families (families(); waves of 64 = a base ray, its ulp neighbours, small component-wise relative jitter):
  limb, inside_on, through_centre (spheres); denom, on_plane, far (planes); sheet (the mesh of with_mesh, from both sides: what culling
  changes); tie.
restate() is the analytic branch and the closest-hit search in numpy float32, with the deliberate mistakes of MISTAKES; a mesh's share of the
search is an input (the oracle's record of the scene with nothing but its mesh).  Seeded numpy only; the yardstick is the CPU oracle."""
import os

import numpy as np


f32 = np.float32
W, H = 48, 32
FLT_MAX = np.finfo(f32).max
BIAS = f32(1e-4)                              # Options::bias, which no scene key sets
EPS = 1e-8                                    # objects.cpp:810, a double
EPS_F32 = f32(1e-8)                           # what a float comparison would use: one ulp below the smallest float that is >= 1e-8
CAM = (0.0, 0.0, 0.0)
LIGHT_POS = (1.0, 2.0, -1.0)
LIGHT_DIR = (0.3, -1.0, -0.4)
PHONG = "phong,0.4,0.1,0.7,10.0"

FORMS = ["spheres", "materials", "with_mesh_cull", "with_mesh_nocull", "planes", "extremes",
         "tie_spheres_ab", "tie_spheres_ba", "tie_tangent_ab", "tie_tangent_ba", "tie_planes_ab", "tie_planes_ba", "tie_quad_ab", "tie_quad_ba"]
TIE_PAIRS = [("tie_spheres_ab", "tie_spheres_ba"), ("tie_tangent_ab", "tie_tangent_ba"), ("tie_planes_ab", "tie_planes_ba"),
             ("tie_quad_ab", "tie_quad_ba")]
FAMILIES = ["limb", "inside_on", "through_centre", "denom", "on_plane", "far", "sheet", "tie", "tie_near"]
MISTAKES = ["d2_one_rounding", "d2_ge_r2", "t0_le_0", "plane_t_gt_0", "eps_in_float", "last_tie_wins", "analytic_before_meshes"]


def lattice_obj(n=16, bump=0.0):
    """(n+1)^2 vertices on the lattice k / 8 (exact in fp32), two triangles per cell; bump: z = +-bump in a checker pattern."""
    s = []
    for j in range(n + 1):
        for i in range(n + 1):
            s.append("v %.6f %.6f %.6f" % (i / 8.0, j / 8.0, bump * (1 if (i + j) % 2 else -1)))
    for j in range(n):
        for i in range(n):
            a = j * (n + 1) + i + 1; b = a + 1; c = a + n + 2; d = a + n + 1
            s.append("f %d %d %d" % (a, b, c)); s.append("f %d %d %d" % (a, c, d))
    return "\n".join(s) + "\n"


def fmt(v):
    """float32 values as text that parses back to the same float32"""
    return ",".join("%.9g" % x for x in np.asarray(v, f32).reshape(-1))


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_bits(a, b):
    """per element: the bits are equal or both are NaN; signs of zero count"""
    a = np.ascontiguousarray(a, f32); b = np.ascontiguousarray(b, f32)
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


def canonical(a):
    """the uint32 bits with every NaN as 0x7fc00000: what the digests of tests/golden/analytic_margins.json are taken over"""
    a = np.ascontiguousarray(a, f32)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), bits(a)).astype("<u4")


# ---- the scene forms ----------------------------------------------------------------------------------------------------------------------
def sphere(pos, r, color, material=""):
    return dict(type="sphere", pos=tuple(float(x) for x in pos), r=float(r), color=color, material=material)


def plane(pos, normal, color, material=""):
    return dict(type="plane", pos=tuple(float(x) for x in pos), normal=tuple(float(x) for x in normal), color=color, material=material)


def mesh(pos, size, color, n=16):
    return dict(type="mesh", pos=tuple(float(x) for x in pos), size=tuple(float(x) for x in size), color=color, material="", n=n)


THREE = [((0.5, 0.25, -3.0), 1.0, "1,0.5,0.25"), ((-1.5, 0.5, -4.0), 0.5, "0.25,1,0.5"), ((-30.0, 130.0, -300.0), 25.0, "0.5,0.25,1")]
GROUND = ((0.0, -1.5, 0.0), (0.0, 1.0, 0.0), "1,1,1")
SHEET = ((-0.75, -0.5, -2.0), (0.5, 0.5, 0.0), "1,1,0.5")      # the flat lattice sheet of tests/test_gpu_margins.py, scaled small
QUAD = ((0.0, 0.0, -3.0), (2.0, 2.0, 0.0), "1,0.25,0.25")      # ... and at z = -3 exactly, in the plane it ties with


def objects_of(form):
    """The objects of a form in scene order."""
    if form == "spheres":
        return [plane(*GROUND)] + [sphere(*s) for s in THREE]
    if form == "materials":
        return [plane(*GROUND, material=PHONG)] + [sphere(*s, material=m) for s, m in zip(THREE, (PHONG, "reflective", "transparent,1.4"))]
    if form.startswith("with_mesh"):
        return [plane(*GROUND)] + [sphere(*s) for s in THREE[:2]] + [mesh(*SHEET)] + [sphere(*THREE[2])]
    if form == "planes":
        # every plane is parallel to z (a tunnel): a ray along z is nearly parallel to all of them, so the one it is aimed at can be the
        # nearest.  Stored normals of length 1e-3, 1 and 1e4, axis-aligned and tilted (rotated about z), kept as stored.
        return [plane((0, -1.5, 0), (0, 1, 0), "1,1,1"), plane((0, 6, 0), (0, -1e-3, 0), "1,0.5,0.5"),
                plane((-5, 0, 0), (8e3, 6e3, 0), "0.5,1,0.5"), plane((5, 0, 0), (-0.8e-3, 0.6e-3, 0), "0.5,0.5,1"),
                plane((0, -4, 0), (0.28, 0.96, 0), "1,1,0.5"), plane((9, 0, 0), (-1e4, 0, 0), "0.5,1,1")]
    if form == "extremes":
        # radius 0, 1e-3, 1e19 (r2 = 1e38, finite), 1e20 (r2 = inf; the camera is inside it), a sphere around the camera, a plane through
        # the camera position
        return [sphere((0, 0.5, -3), 0.0, "1,0,0"), sphere((-0.5, 0.25, -2), 1e-3, "0,1,0"), sphere((0, 2.25e18, -1.18e19), 1e19, "0.5,0.25,1"),
                sphere((0, 0, 1.2e19), 1e20, "1,0,1"), sphere((0.25, 0, -1), 6.0, "1,0.5,0.25"), plane(CAM, (0, 1, 0), "1,1,1")]
    kind, order = form[4:-3], form[-2:]
    pair = {"spheres": [sphere((0.5, 0.25, -3), 1.0, "1,0,0"), sphere((0.5, 0.25, -3), 1.0, "0,0,1")],
            "tangent": [sphere((0, 0, -4), 1.0, "1,0,0"), plane((0, -1, 0), (0, 1, 0), "0,0,1")],
            "planes": [plane((0, -1.5, 0), (0, 1, 0), "1,0,0"), plane((0, -1.5, 0), (0, 1, 0), "0,0,1")],
            "quad": [mesh(*QUAD, n=4), plane((0, 0, -3), (0, 0, 1), "0,0,1")]}[kind]
    return pair if order == "ab" else pair[::-1]


def cull_of(form):
    return 0 if form == "with_mesh_nocull" else 1


def object_text(o, work):
    s = "[object]\ntype=%s\npos=%s\n" % (o["type"], fmt(o["pos"]))
    if o["type"] == "sphere":
        s += "radius=%s\n" % fmt(o["r"])
    elif o["type"] == "plane":
        s += "normal=%s\n" % fmt(o["normal"])
    else:
        path = os.path.join(str(work), "lattice%d.obj" % o["n"])
        if not os.path.exists(path):
            with open(path, "w") as f:
                f.write(lattice_obj(o["n"], 0.0))
        s += "size=%s\nrot=0,0,0\n" % fmt(o["size"])
    s += "color=%s\n" % o["color"]
    if o["material"]:
        s += "material=%s\n" % o["material"]
    if o["type"] == "mesh":
        s += "name=%s\n" % path
    return s + "\n"


def scene_text(form, work, cam=CAM, keep=None, only=None):
    """keep: None = every object, else a predicate over the object dicts (the form without its spheres and planes, or with only them);
    only: the indices of the objects to keep"""
    head = ("[options]\nwidth=%d\nheight=%d\nfov=60\nposition=%s\nuseBackfaceCulling=%d\nbackground_color=0.2,0.3,0.5\n"
            "image_name=output/analytic_margins\n\n"
            "[light]\ntype=point\nposition=%s\ncolor=1,0.8,0.6\nintensity=0.9\n\n[light]\ntype=distant\ndirection=%s\ncolor=0.4,0.6,1\nintensity=0.5\n\n"
            ) % (W, H, fmt(cam), cull_of(form), fmt(LIGHT_POS), fmt(LIGHT_DIR))
    return head + "".join(object_text(o, work) for k, o in enumerate(objects_of(form)) if (keep is None or keep(o)) and (only is None or k in only)) + "[end]\n"


def write_scene(form, work, cam=CAM, keep=None, tag="", only=None):
    path = os.path.join(str(work), "%s%s.scene" % (form, tag))
    with open(path, "w") as f:
        f.write(scene_text(form, work, cam, keep, only))
    return path


def is_mesh(o):
    return o["type"] == "mesh"


def cameras(form):
    """The camera positions of the frames of a form: its own, and where the form has such an object inside a sphere, at a sphere's centre
    and on a plane."""
    objs = objects_of(form)
    out = [("own", CAM)]
    sph = [o for o in objs if o["type"] == "sphere" and 0.1 <= o["r"] <= 100]
    if sph:
        c, r = np.array(sph[0]["pos"]), sph[0]["r"]
        out += [("inside", tuple(c + r * np.array([0.25, -0.125, 0.5]))), ("centre", tuple(c))]
    pl = [o for o in objs if o["type"] == "plane" and o["pos"] != CAM]
    if pl:
        c = np.array(pl[0]["pos"])
        n = np.array(pl[0]["normal"])
        a = np.array([0.0, 0.0, 1.0]) if n[2] == 0 else np.array([1.0, 0.0, 0.0])
        out.append(("on_plane", tuple(c + 0.5 * a)))
    return out


# ---- waves ----------------------------------------------------------------------------------------------------------------------------------
def waves(base_o, base_d, rng, rel=2.0 ** -20, fixed_origin=None):
    """Every base ray becomes a wave of 64, as waves() of tests/test_gpu_margins.py builds them: lane 0 the ray itself, lanes 1 .. 15 its ulp
    neighbours in one component of the origin or the direction, lanes 16 .. 63 relative jitter.  The jitter here is relative to each COMPONENT
    (a component that is 0, or 1e-12 on purpose, stays so): these rays are aimed to within ulps, and jitter relative to the largest component
    would move all of them off their margin.  fixed_origin: the base rays whose jittered lanes keep the origin (an origin found by search)."""
    base_o = np.asarray(base_o, np.float64); base_d = np.asarray(base_d, np.float64)
    n = len(base_o)
    with np.errstate(over="ignore"):
        o = np.repeat(base_o[:, None, :], 64, 1).astype(f32); d = np.repeat(base_d[:, None, :], 64, 1).astype(f32)
        jo = 1 + rng.uniform(-1, 1, (n, 64, 3)) * rel; jd = 1 + rng.uniform(-1, 1, (n, 64, 3)) * rel
        jo[:, :16] = 1; jd[:, :16] = 1
        if fixed_origin is not None:
            jo[np.asarray(fixed_origin, bool)] = 1
        o = (o * jo).astype(f32); d = (d * jd).astype(f32)
    for k in range(1, 16):
        which = o if k % 2 else d
        comp = (k // 2) % 3
        which[:, k, comp] = np.nextafter(which[:, k, comp], f32(np.inf if k < 8 else -np.inf))
    return np.concatenate([o, d], 2).reshape(-1, 6)


def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def random_units(rng, n):
    return unit(rng.normal(size=(n, 3)))


def perpendicular(a, rng):
    """random unit vectors perpendicular to the unit vectors a"""
    p = np.cross(a, random_units(rng, len(a)))
    return unit(p)


# ---- a sphere's families --------------------------------------------------------------------------------------------------------------------
def limb_base(c, r, cam, rng, per_j=2):
    """Rays whose exact d2 is r2 (1 + j' 2^-22), j' within 1 of j = -8 .. 8: sin(angle to the centre) = sqrt(r2 (1 + j 2^-22)) / |L|.  Origins within 0.5 of
    the camera and 50 units from it (above the ground, in front), alternately; every second ray reversed, so that the sphere is behind it (tca < 0)."""
    c = np.asarray(c, f32).astype(np.float64)
    r2 = float(radius2(r))
    O, D = [], []
    k = 0
    for j in range(-8, 9):
        for _ in range(per_j):
            near = (k // 2) % 2 == 0
            o = np.asarray(cam, np.float64) + (rng.uniform(-0.5, 0.5, 3) if near else 50.0 * np.abs(random_units(rng, 1)[0]) * [1, 1, -1])
            o = o.astype(f32).astype(np.float64)
            L = c - o
            ln = np.linalg.norm(L)
            k += 1
            if not ln > np.sqrt(r2 * (1 + 9 * 2.0 ** -22)):
                continue                      # (the origin is inside the sphere: inside_on's)
            Lh = L / ln
            p = perpendicular(Lh[None, :], rng)[0]
            # within a step of j, the first direction whose float32 d2 IS r2 where there is one (a sphere so far away that L does not feel
            # the origin has few such directions: tca tca must round to one particular float)
            jj = j + np.concatenate([[0.0], np.linspace(-1, 1, 65)])
            s = np.sqrt(r2 * (1 + jj * 2.0 ** -22)) / ln
            cand = (np.sqrt(1 - s * s)[:, None] * Lh + s[:, None] * p) * (1 if k % 2 else -1)
            _, _, det = sphere_test(np.repeat(o[None, :], len(cand), 0).astype(f32), cand.astype(f32), c.astype(f32), radius2(r), detail=True)
            O.append(o); D.append(cand[np.argmax(det["exact"])])
    return np.array(O).reshape(-1, 3), np.array(D).reshape(-1, 3)


def restated_sphere_hit_point(o, d, c, r):
    """(t, P, N) of rays that meet the sphere from outside, float32 throughout (a construction, not an expectation)"""
    _, t = sphere_test(o.astype(f32), d.astype(f32), np.asarray(c, f32), radius2(r))
    with np.errstate(all="ignore"):
        P = (o.astype(f32) + d.astype(f32) * t[:, None]).astype(f32)
        N = P - np.asarray(c, f32)
        N = (N / np.sqrt((N * N).sum(1, dtype=f32))[:, None]).astype(f32)
    return t, P, N


def inside_on_base(c, r, cam, rng, n=3):
    """(origins, directions, sub-family) -- 'centre': origins at the centre; 'inside': strictly inside; 'surface': on the surface (c + r u
    rounded to float32) with directions on both sides of the tangent plane, down to 2^-22 of it; 'surface_exact': the same where L.L == r2; 'bias': P + N bias of an earlier hit, towards
    the lights and along the mirror direction, as the recursion makes them."""
    c = np.asarray(c, np.float64)
    O, D, S = [], [], []
    u = random_units(rng, n)
    O.append(np.repeat(c[None, :], n, 0)); D.append(random_units(rng, n)); S += ["centre"] * n
    O.append(c + r * u * rng.uniform(0.05, 0.9, (n, 1))); D.append(random_units(rng, n)); S += ["inside"] * n
    m = 3 * n
    u = random_units(rng, m)
    tang = perpendicular(u, rng)
    eta = np.where(np.arange(m) % 3 == 0, rng.uniform(-1, 1, m), np.sign(rng.uniform(-1, 1, m)) * 2.0 ** -rng.integers(4, 23, m))
    eta[::7] = 0.0
    O.append(c + r * u); D.append(unit(tang + u * eta[:, None])); S += ["surface"] * m
    # ... and surface origins whose float32 L.L is r2 exactly (found by search): any direction then has thc = |tca| and a root that is 0
    u = random_units(rng, 4096)
    c32 = np.asarray(c, f32)
    o = (c + r * u).astype(f32)
    L = (c32 - o).astype(f32)
    at = np.nonzero(dot(L, L) == radius2(r))[0][:2 * n]
    if len(at):
        d = unit(perpendicular(u[at], rng) + u[at] * rng.uniform(-1, 1, (len(at), 1)))
        O.append(o[at].astype(np.float64)); D.append(d); S += ["surface_exact"] * len(at)
    # earlier hits: rays from around the camera into the cone of the sphere
    L = c - np.asarray(cam, np.float64)
    ln = np.linalg.norm(L)
    if ln > r > 0:
        k = 2 * n
        o = np.asarray(cam, np.float64) + rng.uniform(-0.25, 0.25, (k, 3))
        aim = c + r * rng.uniform(0.0, 0.999, (k, 1)) * perpendicular(np.repeat((L / ln)[None, :], k, 0), rng)
        d = unit(aim - o)
        t, P, N = restated_sphere_hit_point(o, d, c, r)
        ok = np.isfinite(t) & (t > 0) & (t < FLT_MAX)
        P, N, d = P[ok].astype(np.float64), N[ok].astype(np.float64), d[ok]
        B = (P.astype(f32) + N.astype(f32) * BIAS).astype(np.float64)
        to_light = unit(np.asarray(LIGHT_POS) - P)
        mirror = d - 2 * (d * N).sum(1, keepdims=True) * N
        for dirs in (to_light, np.repeat(unit(-np.asarray(LIGHT_DIR))[None, :], len(P), 0), mirror):
            O.append(B); D.append(dirs); S += ["bias"] * len(P)
    return np.concatenate(O), np.concatenate(D), np.array(S)


def through_centre_base(c, r, cam, rng, n=4):
    """Rays through the centre: d2 comes out 0, denormal or negative.  From around the camera and from far away, forwards and backwards, and
    from 1e-20 .. 1e-3 off the centre where float32 can say so (a coordinate of the centre that is 0)."""
    c = np.asarray(c, np.float64)
    O, D = [], []
    for k in range(n):
        o = np.asarray(cam, np.float64) + (rng.uniform(-0.5, 0.5, 3) if k % 2 == 0 else 50.0 * random_units(rng, 1)[0])
        o = o.astype(f32).astype(np.float64)
        if np.linalg.norm(c - o) > 0:
            O.append(o); D.append(unit(c - o) * (1 if k % 4 < 2 else -1))
    for k, off in enumerate((1e-20, 1e-20, 3e-19, 1e-12, 1e-6, 1e-3)):
        e = np.zeros(3); e[k % 3] = off
        dirs = (random_units(rng, 1)[0], np.roll(np.array([1.0, 0.0, 0.0]), k % 3), -e / off)
        for d in dirs:
            O.append(c + e); D.append(d)
    return np.array(O), np.array(D)


# ---- a plane's families ---------------------------------------------------------------------------------------------------------------------
def plane_frame(n):
    """(unit normal, a coordinate axis in the plane, the components the normal lives in)"""
    n = np.asarray(n, np.float64)
    live = [k for k in range(3) if n[k] != 0]
    free = [k for k in range(3) if n[k] == 0]
    assert free, "the planes of these forms are parallel to a coordinate axis"
    axis = np.zeros(3); axis[free[-1]] = 1.0
    return n / np.linalg.norm(n), axis, live


def aimed_denominator(n, axis, live, tau, rng):
    """a direction along `axis` whose float32 d.n is tau to within an ulp or two: the normal's components are set, nothing cancels"""
    n32 = np.asarray(n, f32).astype(np.float64)
    d = axis.copy()
    if len(live) == 1:
        d[live[0]] = tau / n32[live[0]]
    else:
        a, b = live
        d[a] = rng.uniform(0.2, 0.8) * tau / n32[a]
        d[b] = (tau - float(f32(d[a])) * n32[a]) / n32[b]
    return d


def denom_base(c, n, rng, per=1):
    """d.n either side of +-1e-8: within a few ulp (j = -6 .. 6; the waves' ulp neighbours and jitter fill the gaps), at 0.5 x and 2 x, and +-0 exactly.  The origin is 2^-7 from the plane on the
    side the ray comes from or on the other (t < 0), far from every other plane of the form."""
    c = np.asarray(c, np.float64)
    nh, axis, live = plane_frame(n)
    taus = [s * EPS * m * (1 + j * 2.0 ** -23) for s in (1, -1) for m, js in ((1.0, (-6, -3, -2, -1, 0, 1, 2, 3, 6)), (0.5, (0,)), (2.0, (0,))) for j in js]
    O, D = [], []
    for tau in taus * per:
        for side in (1, -1):
            d = aimed_denominator(n, axis, live, tau, rng)
            h = -np.sign(tau) * side * 2.0 ** -7
            O.append(c + rng.uniform(-2, 2) * axis + h * nh); D.append(d)
    for z in (0.0, -0.0):
        for sgn in (1, -1):
            d = axis * sgn
            for k in live:
                d[k] = z
            O.append(c + 2.0 ** -7 * nh); D.append(d)
    return np.array(O), np.array(D)


def on_plane_base(c, n, rng, per=2):
    """Origins exactly on the plane (the numerator is +0 or -0), one ulp above and one below, with directions towards the plane, away from it
    and along it."""
    c32 = np.asarray(c, f32)
    nh, axis, live = plane_frame(n)
    O, D = [], []
    for _ in range(per):
        for step in (0, 1, -1):
            o = c32 + (axis * rng.choice([-1.0, 1.0]) * rng.integers(1, 64) / 16.0).astype(f32)
            if step:
                k = live[0]
                o[k] = np.nextafter(o[k], f32(np.inf * step * np.sign(nh[k])))
            tang = axis * rng.choice([-1.0, 1.0])
            for d in (unit(tang - nh * rng.uniform(0.05, 2)), unit(tang + nh * rng.uniform(0.05, 2)), tang, -nh, nh):
                O.append(o.astype(np.float64)); D.append(d)
    return np.array(O), np.array(D)


def far_base(c, n, rng):
    """Grazing hits whose t runs through 1e6 .. 1e30 (the horizon): height h over the plane, slope h / t, the slope large enough for the
    denominator to pass the 1e-8."""
    c = np.asarray(c, np.float64)
    nh, axis, live = plane_frame(n)
    ln = np.linalg.norm(np.asarray(n, np.float64))
    O, D = [], []
    for e in range(6, 31, 2):
        t = 10.0 ** e * rng.uniform(1, 9)
        h = max(1.0, t * 4e-8 / ln)
        d = axis * rng.choice([-1.0, 1.0]) - nh * (h / t)
        O.append(c + h * nh + rng.uniform(-3, 3) * axis); D.append(d)
    return np.array(O), np.array(D)


# ---- ties -------------------------------------------------------------------------------------------------------------------------------------
PYTH = [(3, 4, 5), (4, 3, 5), (5, 12, 13), (12, 5, 13), (8, 15, 17), (15, 8, 17), (7, 24, 25), (24, 7, 25), (0, 1, 1), (1, 0, 1)]


def tie_candidates(kind, rng):
    """Rays through both objects of a tie.  Coincident spheres and planes tie on every ray (the same arithmetic twice); the tangent point and
    the quad tie only where both formulas round alike: rays on dyadic and Pythagorean values, kept where restate() finds the tie."""
    O, D = [], []
    if kind == "spheres":
        c = np.array([0.5, 0.25, -3.0])
        o = np.concatenate([rng.uniform(-0.5, 0.5, (40, 3)), c + 50.0 * random_units(rng, 24)])
        aim = c + rng.uniform(0, 0.98, (64, 1)) * random_units(rng, 64)
        return o, unit(aim - o)
    if kind == "planes":
        o = np.concatenate([rng.uniform(-0.5, 0.5, (32, 3)), rng.uniform(-0.5, 0.5, (32, 3)) + [0, -3, 0]])
        d = random_units(rng, 64)
        d[:, 1] = np.where(np.arange(64) < 32, -np.abs(d[:, 1]), np.abs(d[:, 1]))
        return o, d
    if kind == "tangent":
        # from below the plane up through the tangent point T = (0, -1, -4): the plane answers on both faces
        T = np.array([0.0, -1.0, -4.0])
        for a, b, h in PYTH:
            for ca, sa, hh in PYTH:
                for s in (1.0, 2.0, 4.0, 0.5, 5.0, 13.0, 17.0, 25.0, 8.0, 3.0):
                    d = np.array([a * ca / (h * hh), b / h, a * sa / (h * hh)])
                    if b:
                        O.append(T - s * d); D.append(d)
        return np.array(O), np.array(D)
    # quad: straight at the lattice sheet in z = -3 from dyadic points, the direction a power of two long
    for k in range(256):
        x, y = rng.integers(-60, 61, 2) / 64.0
        z = float(rng.integers(0, 5)) / 4.0
        s = 2.0 ** rng.integers(-2, 3)
        O.append([x, y, z]); D.append([0.0, 0.0, -s])
    return np.array(O), np.array(D)


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
def radius2(r):
    """Sphere's r2 as the loaders keep it: r * r in float32 (inf for r = 1e20)"""
    with np.errstate(over="ignore"):
        return f32(r) * f32(r)


def dot(a, b):
    with np.errstate(all="ignore"):
        return ((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]).astype(f32)


def sphere_test(o, d, c, r2, mistake=None, detail=False):
    """Sphere::intersectObject (objects.cpp:774-786) over arrays, float32: (returns true, t0)"""
    with np.errstate(all="ignore"):
        L = (c - o).astype(f32)
        tca = dot(L, d)
        ll = dot(L, L)
        if mistake == "d2_one_rounding":          # what a contracted build does: fma(-tca, tca, L.L)
            d2 = (ll.astype(np.float64) - tca.astype(np.float64) * tca.astype(np.float64)).astype(f32)
        else:
            d2 = (ll - (tca * tca).astype(f32)).astype(f32)
        out = (d2 >= r2) if mistake == "d2_ge_r2" else (d2 > r2)
        thc = np.sqrt((r2 - d2).astype(f32)).astype(f32)
        t0 = (tca - thc).astype(f32); t1 = (tca + thc).astype(f32)
        second = (t0 <= 0) if mistake == "t0_le_0" else (t0 < 0)
        t = np.where(second, t1, t0).astype(f32)
        ok = ~out & ~(t < 0)
    if detail:
        return ok, t, dict(d2=d2, second=second & ~out, exact=(d2 == r2))
    return ok, t


def plane_test(o, d, c, n, mistake=None, detail=False):
    """Plane::intersectObject (objects.cpp:807-814) over arrays: (returns true, t0)"""
    with np.errstate(all="ignore"):
        denom = dot(d, n)
        small = (np.abs(denom) < EPS_F32) if mistake == "eps_in_float" else (np.abs(denom.astype(np.float64)) < EPS)
        t = (dot((c - o).astype(f32), n) / denom).astype(f32)
        ok = ~small & ((t > 0) if mistake == "plane_t_gt_0" else (t >= 0))
    if detail:
        return ok, t, dict(denom=denom, rejected=small, float_differs=(np.abs(denom) < EPS_F32) != (np.abs(denom.astype(np.float64)) < EPS))
    return ok, t


def restate(form, rays, mesh_records=None, mistake=None):
    """Render::trace (scene.cpp:724-756) of a form over arrays: (hit, object, tNear) per ray, tNear FLT_MAX at a miss.  mesh_records: the
    oracle's probe records of the form with nothing but its mesh (the mesh's share of the search: hit and tNear), needed where it has one."""
    rays = np.ascontiguousarray(rays, f32)
    o, d = rays[:, 0:3], rays[:, 3:6]
    objs = objects_of(form)
    order = list(range(len(objs)))
    if mistake == "analytic_before_meshes":
        order = [k for k in order if not is_mesh(objs[k])] + [k for k in order if is_mesh(objs[k])]
    obj = np.full(len(rays), -1, np.int32)
    tn = np.full(len(rays), FLT_MAX, f32)
    for k in order:
        b = objs[k]
        if b["type"] == "sphere":
            ok, t = sphere_test(o, d, np.asarray(b["pos"], f32), radius2(b["r"]), mistake)
        elif b["type"] == "plane":
            ok, t = plane_test(o, d, np.asarray(b["pos"], f32), np.asarray(b["normal"], f32), mistake)
        else:
            ok, t = mesh_records[:, 0] > 0, mesh_records[:, 3].astype(f32)
        with np.errstate(invalid="ignore"):
            take = ok & ((t <= tn) if mistake == "last_tie_wins" else (t < tn))
        obj[take] = k; tn[take] = t[take]
    return obj >= 0, obj, tn


def differs(a, b):
    """per ray: the restated records (hit, object, tNear) differ"""
    return (a[0] != b[0]) | (a[1] != b[1]) | ~same_bits(a[2], b[2])


# ---- the families of a form -----------------------------------------------------------------------------------------------------------------
class Family:
    """rays n x 6 float32; target: per ray the object it is aimed at; sub: per ray the sub-family (inside_on) or ''"""

    def __init__(self, rays, target, sub=None):
        self.rays = np.ascontiguousarray(rays, f32)
        self.target = np.asarray(target, np.int32)
        self.sub = np.asarray(sub if sub is not None else [""] * len(rays))
        assert len(self.rays) % 64 == 0 and len(self.target) == len(self.rays) == len(self.sub)
        for a in (self.rays, self.target, self.sub):
            a.setflags(write=False)


def _join(parts):
    return Family(np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts]))


_families = {}


def mesh_records(oracle, form, work, rays):
    """The oracle's probe records of `rays` in the form with nothing but its mesh: the mesh's share of restate()'s search."""
    o = oracle.OracleScene(write_scene(form, work, keep=is_mesh, tag="_mesh_only"), W, H)
    h, _ = o.probe(rays, colours=False)
    o.close()
    return h


def placed_triangles(oracle, form, work):
    """the form's mesh as the loader places it: n x 9 (a, b, c)"""
    o = oracle.OracleScene(write_scene(form, work, keep=is_mesh, tag="_mesh_only"), W, H)
    tris = o.bvh(0)["tris"][:, 0:9].astype(np.float64)
    o.close()
    return tris


def sheet_base(tris, rng, n=32):
    """Rays at vertices, edge midpoints and inner points of the sheet's triangles, alternately from its front and from its back: the back
    ones are what useBackfaceCulling decides, and what lies behind the sheet answers in its place."""
    T = tris[rng.choice(len(tris), n, replace=False)]
    A, B, C = T[:, 0:3], T[:, 3:6], T[:, 6:9]
    nrm = unit(np.cross(B - A, C - A))
    w = rng.dirichlet((1, 1, 1), n)
    w[0::4] = (1, 0, 0); w[1::4] = (0.5, 0.5, 0)
    P = w[:, 0:1] * A + w[:, 1:2] * B + w[:, 2:3] * C
    side = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)[:, None]
    d = unit(-side * nrm + perpendicular(nrm, rng) * rng.uniform(0, 0.5, (n, 1)))
    return P - d * rng.uniform(0.5, 1.5, (n, 1)), d


def has_mesh(form):
    return any(is_mesh(b) for b in objects_of(form))


def families(form, oracle=None, work=None):
    """{family: Family} of a form, in the order of FAMILIES, seeded by the form's place in FORMS (both orders of a tie get the same rays, and so
    do with_mesh_cull and with_mesh_nocull);
    computed once.  About 20 000 rays on the forms with three spheres; every family is whole waves of 64.  The quad's ties are kept by the
    mesh's own records and the sheet's rays aim at its placed triangles, so those forms need the oracle and a directory to write to."""
    if form in _families:
        return _families[form]
    ab = form[:-3] + "_ab" if form.startswith("tie_") else "with_mesh_cull" if form == "with_mesh_nocull" else form
    rng = np.random.default_rng(0xA7A1 + FORMS.index(ab))
    objs = objects_of(form)
    out = {}
    if not form.startswith("tie_"):
        sph = [(k, b) for k, b in enumerate(objs) if b["type"] == "sphere"]
        pls = [(k, b) for k, b in enumerate(objs) if b["type"] == "plane"]
        fam = {f: [] for f in FAMILIES[:7]}
        for k, b in sph:
            c, r = b["pos"], b["r"]
            if r > 0:
                o, d = limb_base(c, r, CAM, rng, per_j=4 if form == "extremes" else 2)
                if len(o):
                    fam["limb"].append((waves(o, d, rng, 2.0 ** -23), np.full(64 * len(o), k), np.full(64 * len(o), "")))
            if 0 < r < 1e18:
                o, d, s = inside_on_base(c, r, CAM, rng)
                fam["inside_on"].append((waves(o, d, rng, 2.0 ** -23, s == "surface_exact"), np.full(64 * len(o), k), np.repeat(s, 64)))
            if r < 1e18:
                o, d = through_centre_base(c, r, CAM, rng)
                fam["through_centre"].append((waves(o, d, rng, 2.0 ** -23), np.full(64 * len(o), k), np.full(64 * len(o), "")))
        for k, b in pls:
            c, n = b["pos"], b["normal"]
            o, d = denom_base(c, n, rng)
            fam["denom"].append((waves(o, d, rng, 2.0 ** -22), np.full(64 * len(o), k), np.full(64 * len(o), "")))
            o, d = on_plane_base(c, n, rng)
            fam["on_plane"].append((waves(o, d, rng, 2.0 ** -21), np.full(64 * len(o), k), np.full(64 * len(o), "")))
            o, d = far_base(c, n, rng)
            fam["far"].append((waves(o, d, rng, 2.0 ** -20), np.full(64 * len(o), k), np.full(64 * len(o), "")))
        if has_mesh(form):
            o, d = sheet_base(placed_triangles(oracle, form, work), rng)
            k = [is_mesh(b) for b in objs].index(True)
            fam["sheet"].append((waves(o, d, rng, 2.0 ** -20), np.full(64 * len(o), k), np.full(64 * len(o), "")))
        out = {f: _join(p) for f, p in fam.items() if p}
    else:
        kind = form[4:-3]
        o, d = tie_candidates(kind, rng)
        if kind in ("spheres", "planes"):
            exact = waves(o, d, rng, 2.0 ** -20)                 # (the same arithmetic twice: every ray ties)
        else:
            cand = np.concatenate([o, d], 1).astype(f32)
            exact, _ = keep_exact_ties(ab, cand, mesh_records(oracle, ab, work, cand) if kind == "quad" else None)
        out["tie"] = Family(exact, np.zeros(len(exact)))
        near = waves(o[:32], d[:32], rng, 2.0 ** -22)
        out["tie_near"] = Family(near, np.zeros(len(near)))
    _families[form] = out
    return out


def keep_exact_ties(form, rays, mesh_recs, n_waves=8):
    """The tie candidates on which restate() finds the two objects at the same tNear (first wins and last wins name different objects),
    repeated to n_waves whole waves; also their number."""
    a = restate(form, rays, mesh_recs)
    b = restate(form, rays, mesh_recs, "last_tie_wins")
    tie = a[0] & (a[1] != b[1])
    kept = rays[tie]
    assert len(kept) >= 16, "%s: only %d of %d candidates tie" % (form, len(kept), len(rays))
    reps = -(-64 * n_waves // len(kept))
    return np.ascontiguousarray(np.tile(kept, (reps, 1))[:64 * n_waves], f32), int(tie.sum())


# ---- results of a form and their digests ------------------------------------------------------------------------------------------------------
def results(scene_class, form, work, fams):
    """Everything the CPU module compares of one form, from an OracleScene or a tools.ref_harness.RefScene (the same methods):
    {(family, "hits"): n x 8, (family, "colours"): n x 3, ("frame", "pass1"), ("frame", "ssaa")}.  The SSAA frame's first row and column
    are zeroed: the reference's Sobel reads its border from an uninitialised buffer (tests/test_oracle_vs_reference.py)."""
    s = scene_class(write_scene(form, work), W, H)
    out = {}
    for name, fam in fams.items():
        out[(name, "hits")], out[(name, "colours")] = s.probe(fam.rays)
    p1 = s.pass1()
    out[("frame", "pass1")] = p1
    f2 = s.ssaa(p1).copy()
    f2[0, :] = 0; f2[:, 0] = 0
    out[("frame", "ssaa")] = f2
    if hasattr(s, "close"):
        s.close()
    return out


def digests(res):
    """{"family/output": SHA-256 of canonical()} of results()"""
    import hashlib
    return {"%s/%s" % k: hashlib.sha256(canonical(v).tobytes()).hexdigest() for k, v in res.items()}
