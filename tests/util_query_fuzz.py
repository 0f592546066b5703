"""Seeded random scenes for the ray, point and frame queries (tests/test_query_fuzz_cpu.py, tests/test_gpu_query_fuzz.py): a generator of its
own -- tests/test_gpu_fuzz.make_scene and tests/util_shading.make_shading_scene are pinned to the reference seed by seed and aim their
cameras past most meshes --, the seeded ray and point sets of a seed, and the expectation of every query composed from the helpers the suite
already pins to the CPU oracle (tests/util_*.py).  No arithmetic of a contract is written again here.

A scene is a cluster of objects around CENTRE, which is also where tests/util_rays.probe_rays aims, and a camera on an orbit around the
cluster that looks at it.  The expectation takes the shading normals N of the rays as an input: exact from Scene.surface_rays on the GPU
(after that call has passed), decoded from the showNormals colours on the CPU, where shares and sensitivities are all that is asked."""
import functools
import math
import os
import random
import re

import numpy as np

from tests import util_ao as AO
from tests import util_aov as U
from tests import util_light as UL
from tests import util_occlusion as OC
from tests import util_points as UP
from tests import util_radiance as UR
from tests import util_render_light as RL
from tests import util_scatter as SC
from tests import util_shading as S
from tests import util_surface as SU
from tests import util_views_aov as VA
from tests.util_rays import probe_rays

f32 = np.float32
SEEDS = list(range(16))
CENTRE = (0.0, 0.0, -4.0)
MESHES = ["bumpy_4k.obj", "torus_1536.obj", "torus_uvwild.obj", "quad.obj", "coincident_4k.obj"]
MAPPED = ("torus_1536.obj", "torus_uvwild.obj")          # the assets with texture coordinates
# what a seed is there for, whatever else it draws
NO_MESH = (5, 12)                 # the analytic kernels
PLAIN = (2, 7, 10, 15)            # meshes, default materials only, no area light
NO_LIGHT = 9
N_LIGHTS = {1: 3, 6: 3, 3: 4, 13: 4}
GLASS_AT_ORIGIN = (4, 12)         # a glass sphere around the origins of probe_rays: rays that leave glass, total internal reflection
N_BOUNCE = 4096                   # (B) is subsampled to this many rays: what a seed costs is the expectation's per-element oracle calls
N_PROBE = 2048
N_FREE = 512
VIEW_SIZES = [s for s in VA.SIZES if s[0] <= 64 and s[1] <= 48 and min(s) >= 2]
CALLS = ["trace_rays", "occluded", "surface_rays", "light_rays", "scatter_rays", "sky", "cast_tree", "light_points", "ao_points",
         "radiance_points", "render_aov", "render_ao", "render_light", "render_views", "render_views_aov"]
# the calls whose inputs or expectation take surface_rays' N or position
AFTER_SURFACE = ("light_rays", "scatter_rays", "light_points", "ao_points", "radiance_points", "render_ao", "render_light")


# ---- the generator ------------------------------------------------------------------------------------------------------------------------------
def make_query_scene(seed, dst):
    """Writes the maps and skybox faces of seed `seed` into dst and returns (scene text, width, height)."""
    from rendering_amd import assets
    dst = str(dst)
    assert S.fits(dst), "file names under %s would be longer than %d characters" % (dst, S.NAME_LIMIT)
    r = random.Random(0x9F2 + seed)
    u = r.uniform
    v3 = lambda lo, hi: ",".join("%.3f" % u(lo, hi) for _ in range(3))
    around = lambda sx, sy, sz: "%.3f,%.3f,%.3f" % (CENTRE[0] + u(-sx, sx), CENTRE[1] + u(-sy, sy), CENTRE[2] + u(-sz, sz))
    plain, analytic = seed in PLAIN, seed in NO_MESH
    while True:
        w, h = r.randrange(40, 49), r.randrange(32, 41)
        if w % 8 or h % 8:
            break
    # the camera: on an orbit around the cluster, looking at it, rolled
    az = math.radians(u(35, 75) * r.choice((-1, 1)) if seed in GLASS_AT_ORIGIN else u(-75, 75))
    el = math.radians(u(6, 14) if MESHES[seed % len(MESHES)] == "quad.obj" else u(-8, 14))          # (a quad lies flat: seen from above)
    dist = u(2.8, 4.0)
    tgt = [c + u(-0.3, 0.3) for c in CENTRE]
    pos = (tgt[0] + dist * math.cos(el) * math.sin(az), tgt[1] + dist * math.sin(el), tgt[2] + dist * math.cos(el) * math.cos(az))
    fwd = [(t - p) / dist for t, p in zip(tgt, pos)]
    # (the camera matrix is Rz Ry Rx of the rotation, the view direction its third row negated: (sin y, -cos y sin x, -cos y cos x))
    rot = (math.degrees(math.atan2(-fwd[1], -fwd[2])), math.degrees(math.asin(max(-1.0, min(1.0, fwd[0])))), u(-20, 20))

    # (the materials are dealt in turn, the seeds start at different ones: over the seeds every material is met by many rays)
    deck = [1, 2, 3, 0] * 4
    deck = deck[seed % 4:] + deck[:seed % 4]

    def material():
        if plain:
            return ""
        k = deck.pop(0)
        return ["", "material=reflective\n", "material=transparent,%.2f\n" % u(1.05, 1.8),
                "material=phong,%.2f,%.2f,%.2f,%.1f\n" % (u(0, 0.5), u(0, 1), u(0, 1), r.choice([1, 2, 5, 10, 20, 64]))][k]

    s = "[options]\nwidth=%d\nheight=%d\nfov=%.1f\nposition=%.4f,%.4f,%.4f\nrotation=%.4f,%.4f,%.4f\nmax_ray_depth=%d\nac_penalty=%d\nuseBackfaceCulling=%d\nbackground_color=%s\nimage_name=output/qfuzz\n" % (
        (w, h, u(38, 72)) + pos + rot + (r.randrange(7), r.randrange(1, 6), r.randrange(2), v3(0, 0.6)))
    if r.random() < 0.45:
        kw, kh = r.choice([(8, 20), (44, 12), (96, 40), (12, 28), (4, 64)])
        names = []
        for k in range(6):
            names.append(os.path.join(dst, "q%d_k%d.bmp" % (seed, k)))
            with open(names[-1], "wb") as f:
                f.write(assets.bmp24(S.colour_image(kw, kh, 20 + 40 * k)))
        s += "skyboxes=%s\n" % ",".join(names)
    s += "\n"
    n_lights = 0 if seed == NO_LIGHT else N_LIGHTS.get(seed, r.randrange(1, 3))
    for _ in range(n_lights):
        t = r.choice(["point", "distant"] if plain else ["point", "distant", "area", "area"])
        at = "%.3f,%.3f,%.3f" % (CENTRE[0] + u(-3, 3), CENTRE[1] + u(0.0, 2.5), CENTRE[2] + u(-2, 3))
        if t == "point":
            s += "[light]\ntype=point\nposition=%s\ncolor=%s\nintensity=%.2f\n\n" % (at, v3(0.3, 1), u(0.3, 2))
        elif t == "distant":
            s += "[light]\ntype=distant\ndirection=%.3f,%.3f,%.3f\ncolor=%s\nintensity=%.2f\n\n" % (u(-1, 1), u(-1, -0.2), u(-1, 1), v3(0.3, 1), u(0.2, 1))
        else:
            s += "[light]\ntype=area\npos=%s\ni=%s\nj=%s\nsamples=%d\ncolor=%s\nintensity=%.2f\n\n" % (at, v3(-1, 1), v3(-1, 1), r.randrange(1, 4), v3(0.3, 1), u(0.5, 3))
    objects = []
    floor = analytic or r.random() < 0.75          # (without one, two more spheres: the rays still meet something)
    n_mesh = 0 if analytic else r.randrange(2, 4)
    for k in range(n_mesh):
        obj = MESHES[seed % len(MESHES)] if k == 0 else r.choice(MESHES)
        # (the first mesh where the camera looks, large; a quad lies flat: below the camera's height)
        at = around(0.5, 0.4, 0.5) if k == 0 else around(1.3, 0.8, 0.8)
        size = v3(3.0, 4.2) if k == 0 else v3(2.4, 3.6)
        if obj == "quad.obj":
            at, size = "%.3f,%.3f,%.3f" % (CENTRE[0] + u(-0.5, 0.5), CENTRE[1] + u(-1.3, -0.7), CENTRE[2] + u(-0.5, 0.5)), "%.3f,1,%.3f" % (u(2.5, 4), u(2.5, 4))
        b = "[object]\ntype=mesh\npos=%s\nsize=%s\nrot=%s\ncolor=%s\n%sname=scenes/assets/%s\n" % (at, size, v3(-80, 80), v3(0.4, 1), material(), obj)
        kinds = r.choice([("d", "n", "s"), ("d",), ("n",), ("s",), ("d", "s"), ("d", "n"), ()]) if obj in MAPPED else ()
        for kind, key in (("d", "diffuse_map"), ("n", "normal_map"), ("s", "specular_map")):
            if kind not in kinds:
                continue
            mw = r.choice([4, 8, 12, 20, 36, 64, 100])
            mh = r.choice([x for x in ([3, 5, 9, 17, 33, 60] if kind == "s" else [3, 5, 24, 52, 77, 124]) if x != mw and (kind != "s" or mw * x <= 700)])
            name = os.path.join(dst, "q%d_%d%s.bmp" % (seed, k, kind))
            with open(name, "wb") as f:
                f.write(assets.bmp24(S.IMAGE[kind](mw, mh, 10 + 5 * k)))
            b += "%s=%s\n" % (key, name)
        objects.append(b + "\n")
    for _ in range(r.randrange(3, 6) if analytic else r.randrange(0, 3) + (0 if floor else 2)):
        objects.append("[object]\ntype=sphere\npos=%s\ncolor=%s\nradius=%.2f\n%s\n" % (
            (around(1.8, 1.0, 1.2), v3(0.1, 1), u(0.4, 1.0), material()) if analytic else (around(2.0, 1.0, 1.4), v3(0.1, 1), u(0.3, 0.7), material())))
    if seed in GLASS_AT_ORIGIN:
        objects.append("[object]\ntype=sphere\npos=%s\ncolor=%s\nradius=%.2f\nmaterial=transparent,%.2f\n\n" % (v3(-0.03, 0.03), v3(0.5, 1), u(0.95, 1.1), u(1.35, 1.6)))
    if floor:
        objects.append("[object]\ntype=plane\npos=0,%.3f,0\nnormal=0,1,0\ncolor=%s\n%s\n" % (u(-1.9, -1.5), v3(0.4, 1), material()))
    r.shuffle(objects)
    return s + "".join(objects) + "[end]\n", w, h


def option(text, key):
    return re.search(r"(?m)^%s=(.*)$" % key, text).group(1)


def family_of_text(text):
    """the kernel family that serves a scene file: "analytic" (no mesh), "plain" (every object Diffuse, no area light) or "general" """
    blocks = U.object_blocks(text)
    if not any(b["type"] == "mesh" for b in blocks):
        return "analytic"
    plain = all(SC.material_of(b) == SC.DIFFUSE for b in blocks) and all(b["type"] != "area" for b in UL.light_blocks(text))
    return "plain" if plain else "general"


def view_text(text, w, h, pos, rot, cull=None):
    """the scene text with width, height, position and rotation (and the culling flag) rewritten"""
    vec = lambda v: ",".join("%r" % float(x) for x in v)
    for key, val in (("width", "%d" % w), ("height", "%d" % h), ("position", vec(pos)), ("rotation", vec(rot))) + (
            (("useBackfaceCulling", "%d" % cull),) if cull is not None else ()):
        text, n = re.subn(r"(?m)^%s=.*$" % key, "%s=%s" % (key, val), text, count=1)
        assert n == 1, key
    return text


def order_of(seed):
    """CALLS shuffled by the seed, surface_rays before the first call that takes its N"""
    r = random.Random(0x0DE2 + seed)
    order = list(CALLS)
    r.shuffle(order)
    order.remove("surface_rays")
    first = min(order.index(c) for c in AFTER_SURFACE)
    order.insert(r.randrange(0, first + 1), "surface_rays")
    return order


@functools.lru_cache(maxsize=None)
def _probe_rays():
    rays = probe_rays(N_PROBE)
    rays.setflags(write=False)
    return rays


def unit(v):
    return (v / np.sqrt((v.astype(np.float64) ** 2).sum(1))[:, None]).astype(f32)


# ---- a seed: scene, ray and point sets, expectations ------------------------------------------------------------------------------------------
class Case:
    """Seed `seed` written into dst: text, path, w, h; pool = (A) the view's primary rays, (B) bounce rays from their first hits,
    (D) probe_rays, one array (the answers of a ray do not depend on its batch); everything else a test draws for the seed."""

    def __init__(self, oracle, seed, dst):
        self.O, self.seed, self.dst = oracle, seed, str(dst)
        self.text, self.w, self.h = make_query_scene(seed, self.dst)
        self.path = os.path.join(self.dst, "q%d.scene" % seed)
        with open(self.path, "w") as f:
            f.write(self.text)
        self.blocks, self.const, self.lights = U.object_blocks(self.text), SC.constants_of(U.object_blocks(self.text)), UL.lights_of_text(self.text)
        self.cull = int(option(self.text, "useBackfaceCulling"))
        self.family = family_of_text(self.text)
        self.pose = (tuple(float(x) for x in option(self.text, "position").split(",")), tuple(float(x) for x in option(self.text, "rotation").split(",")))
        o = self.oracle()
        self.cam = U.primary_rays(o)
        o.close()
        rng = np.random.default_rng(0x9F2 + seed)
        bounce = SU.oracle_bounce_rays(oracle, self.path, self.w, self.h, None)
        if len(bounce) > N_BOUNCE:
            bounce = bounce[np.sort(rng.choice(len(bounce), N_BOUNCE, replace=False))]
        self.n_cam, self.n_bounce = len(self.cam), len(bounce)
        self.pool = np.ascontiguousarray(np.concatenate([self.cam, bounce, _probe_rays()]), f32)
        self.pool.setflags(write=False)
        a = int(rng.integers(0, self.h // 2))
        self.rows = (a, int(rng.integers(a + 1, self.h + 1)))
        self.dirs = S.sphere_directions(int(rng.choice([1, 7, 16])))
        self.weights = rng.uniform(0.05, 2.0, len(self.dirs)).astype(f32)
        self.radius = float(rng.choice([np.inf, 0.75, 2.5]))
        box = np.array([2.5, 1.8, 2.0])
        self.free = np.concatenate([(np.array(CENTRE) + rng.uniform(-box, box, (N_FREE, 3))).astype(f32), unit(rng.normal(size=(N_FREE, 3)))], 1).astype(f32)
        self.free_view = np.concatenate([unit(rng.normal(size=(N_FREE, 3))), rng.choice(f32([1, 2, 5, 10, 20, 64]), N_FREE)[:, None]], 1).astype(f32)
        # four further views, and the state the scene is moved to and back from in the middle of the sequence
        self.views = []
        for k in range(4):
            vw, vh = VIEW_SIZES[int(rng.integers(0, len(VIEW_SIZES)))]
            self.views.append((vw, vh) + self.moved(rng.uniform(-0.4, 0.4, 3), rng.uniform(-12, 12, 3)))
        while True:
            dw, dh = int(rng.integers(17, 57)), int(rng.integers(17, 49))
            if (dw, dh) != (self.w, self.h):
                break
        self.detour = (dw, dh) + self.moved(rng.uniform(-0.5, 0.5, 3), rng.uniform(-15, 15, 3))
        self.order = order_of(seed)
        self._memo = {}

    def moved(self, dpos, drot):
        """(pos, rot) offset from the scene's own, as float32 values"""
        return (tuple(float(f32(a + b)) for a, b in zip(self.pose[0], dpos)), tuple(float(f32(a + b)) for a, b in zip(self.pose[1], drot)))

    def oracle(self, cull=None, path=None, size=None):
        w, h = size or (self.w, self.h)
        o = self.O.OracleScene(path or self.path, w, h)
        if cull is not None:
            self.O.lib().orc_set_flag(o.h, b"useBackfaceCulling", int(cull))
        return o

    def memo(self, key, fn):
        if key not in self._memo:
            self._memo[key] = fn()
        return self._memo[key]

    # -- trace_rays, occluded, surface_rays, sky
    def probe(self, cull=None):
        """(hits, colours) of the pool"""
        def fn():
            o = self.oracle(cull)
            out = o.probe(self.pool)
            o.close()
            return out
        return self.memo(("probe", cull), fn)

    def opaque(self, rays, cull=None, transparent_blocks=False):
        """(hit', tNear') of shadow rays: the oracle's probe without the Transparent objects (fault: with them)"""
        if not len(rays):
            return np.zeros(0, bool), np.zeros(0, f32)
        if transparent_blocks:
            o = self.oracle(cull)
            h, _ = o.probe(rays, colours=False)
            o.close()
            return h[:, 0] > 0, h[:, 3].astype(f32)
        return OC.opaque_probe(self.O, self.path, self.dst, rays, culling=cull)

    def occlusion(self, le=False, **fault):
        """(tmax of the seeded mix, expected with it, expected with tmax=None); le: the fault `<=` for `<`"""
        hit0, t0 = self.memo("opaque_pool", lambda: self.opaque(self.pool))
        hit, t = self.opaque(self.pool, **fault) if fault else (hit0, t0)
        tmax = OC.tmax_mix(hit0, t0, seed=0x5EED + self.seed)
        with np.errstate(invalid="ignore"):
            mixed = (hit & (t <= tmax)).astype(np.uint8) if le else OC.expected(hit, t, tmax)
        return tmax, mixed, OC.expected(hit, t, f32(np.inf))

    def surface(self, rays=None, cull=None):
        return SU.expected_of(self.path, self.w, self.h, cull, self.pool if rays is None else rays)

    def decoded_normals(self, rays=None):
        """N decoded from the showNormals colours, 0 at a miss: within an ulp or two of hitNormal, for statistics and sensitivities only"""
        e = self.surface(rays)
        return np.where(e["hit"][:, None], (e["normal_colour"] - f32(0.5)) * f32(2), f32(0)).astype(f32)

    def sky(self):
        def fn():
            o = self.oracle()
            out = o.skybox(self.pool[:, 3:6])
            o.close()
            return out
        return self.memo("sky", fn)

    # -- light_rays, render_light, scatter_rays
    def n_specular(self, hits):
        obj = hits[:, 1].astype(np.int32)
        return np.where(obj >= 0, self.const["n_specular"][np.maximum(obj, 0)], f32(0)).astype(f32)

    def light(self, rays, hits, N, bias=UL.BIAS, reverse=False, **fault):
        """util_light's channels of `rays` (+ "hits"), and the plan; faults: bias, reverse (the sums in reverse order of the lights),
        transparent_blocks / cull (of the shadow rays' probe)"""
        o = self.oracle()
        plan = UL.Plan(o, self.lights, rays, hits, N, bias=bias)
        o.close()
        hit2, t2 = self.opaque(plan.shadow_rays, **fault)
        occ = OC.expected(hit2, t2, plan.shadow_tmax)
        e = plan.reduce(occ, self.n_specular(hits))
        if reverse:
            e["diffuse"], e["specular"] = UL.in_order_sum(e["light_diffuse"][:, ::-1]), UL.in_order_sum(e["light_specular"][:, ::-1])
        e["hits"] = hits
        return e, plan, occ

    def pool_light(self, N):
        return self.memo(("light", N.tobytes()), lambda: self.light(self.pool, self.probe()[0], N))

    def frame_light(self, N):
        """render_light's planes of the frame: light_rays of the primary rays, transposed"""
        e = self.pool_light(N)[0]
        return RL.planes({c: e[c][:self.n_cam] for c in RL.CHANNELS}, self.w, self.h)

    def scatter(self, N):
        def fn():
            s, e = self.surface(), self.pool_light(N)[0]
            out = SC.restate(self.pool, s["hits"], N, s["albedo"], s["specular"], e["diffuse"], e["specular"], self.const)
            out["hits"] = s["hits"]
            return out
        return self.memo(("scatter", N.tobytes()), fn)

    def material(self):
        """per ray of the pool, -1 at a miss"""
        obj = self.probe()[0][:, 1].astype(np.int32)
        return np.where(obj >= 0, self.const["material"][np.maximum(obj, 0)], -1)

    # -- the point calls
    def points(self, position, normal):
        """({P, N} (n, 6), {V, ns} (n, 4), number at first hits): the first hits of (A) -- position and normal of the pool's rays, as
        surface_rays gives them --, then the free points"""
        hits = self.probe()[0][:self.n_cam]
        hit = hits[:, 0] > 0
        first = np.concatenate([position[:self.n_cam][hit], normal[:self.n_cam][hit]], 1)
        view = np.concatenate([self.cam[hit, 3:6], self.n_specular(hits)[hit, None]], 1)
        return (np.ascontiguousarray(np.concatenate([first, self.free]), f32), np.ascontiguousarray(np.concatenate([view, self.free_view]), f32),
                int(hit.sum()))

    def free_light(self):
        def fn():
            o = self.oracle()
            plan = UP.PointPlan(o, self.lights, self.free, self.free_view)
            o.close()
            hit2, t2 = self.opaque(plan.shadow_rays)
            return plan.reduce(OC.expected(hit2, t2, plan.shadow_tmax))
        return self.memo("free_light", fn)

    def point_light(self, N):
        """light_points' channels: at the first hits light_rays' of the primary rays that hit, then util_points.PointPlan's at the free points"""
        e, free = self.pool_light(N)[0], self.free_light()
        hit = self.probe()[0][:self.n_cam, 0] > 0
        return {c: np.concatenate([e[c][:self.n_cam][hit], free[c]]) for c in UP.CHANNELS}

    def point_ao(self, points):
        traced, pt, k, rays = UP.ao_traced_rays(points, self.dirs)
        hit, t = self.opaque(rays)
        return UP.ao_reduce(traced, pt, OC.expected(hit, t, f32(self.radius)))

    def frame_ao(self, N):
        """render_ao's (counts, ao) of the frame, from the primary rays, the oracle's tNear and the normals N of the pool"""
        hits = self.probe()[0][:self.n_cam]
        hit = (hits[:, 0] > 0) & U.written_mask(self.w, self.h, self.rows).ravel()
        traced, pix, k, rays = AO.traced_rays(self.cam, hits[:, 3], N[:self.n_cam], hit, self.dirs)
        h2, t2 = self.opaque(rays)
        return AO.reduce(traced, pix, OC.expected(h2, t2, f32(self.radius)), (self.h, self.w))

    def radiance_colours(self, points):
        rays, traced = UR.rays(points, self.dirs)
        o = self.oracle()
        _, col = o.probe(rays)
        o.close()
        return col.reshape(len(points), len(self.dirs), 3)

    def radiance(self, points, cosine, col=None):
        col = self.radiance_colours(points) if col is None else col
        return UR.reduce(col, points[:, 3:6], self.dirs, self.weights, cosine)

    # -- frames and views
    def frame_aov(self):
        return U.expected_of(self.path, self.w, self.h)

    def view_path(self, k, w, h, pos, rot, cull=None):
        path = os.path.join(self.dst, "q%d_%s.scene" % (self.seed, k))
        with open(path, "w") as f:
            f.write(view_text(self.text, w, h, pos, rot, cull))
        return path

    def view(self, k):
        """what view k of the batch calls must hold: pass1, ssaa, mask, aov (util_aov.expected_of), rays, position"""
        def fn():
            w, h, pos, rot = self.views[k]
            path = self.view_path("v%d" % k, w, h, pos, rot)
            o = self.oracle(path=path, size=(w, h))
            p1 = o.pass1()
            out = dict(pass1=p1, ssaa=o.ssaa(p1), mask=inner_mask(o.sobel(p1)), rays=U.primary_rays(o), aov=U.expected_of(path, w, h))
            o.close()
            out["position"] = SU.expected_of(path, w, h, None, out["rays"])["position"]
            return out
        return self.memo(("view", k), fn)

    def detour_frame(self):
        """(the finished frame, its mask) of the state the sequence visits in its middle: the other culling value, another camera and size"""
        w, h, pos, rot = self.detour
        o = self.oracle(path=self.view_path("d", w, h, pos, rot, 1 - self.cull), size=(w, h))
        p1 = o.pass1()
        out = o.ssaa(p1), inner_mask(o.sobel(p1))
        o.close()
        return out


def inner_mask(sobel):
    """the oracle's Sobel mask as flags, its border 0 by definition (tests/test_gpu_shading_data.reference)"""
    mask = sobel != 0
    mask[0, :] = False; mask[-1, :] = False; mask[:, 0] = False; mask[:, -1] = False
    return mask


def texels(o, text, exp):
    """{"d" / "n" / "s": distinct texels of the maps of that kind that the hits of SU.expected()'s `exp` fetch}, summed over the objects"""
    out = {"d": 0, "n": 0, "s": 0}
    for k, b in enumerate(U.object_blocks(text)):
        sel = np.nonzero(exp["object_id"] == k)[0]
        for kind, key in (("d", "diffuse_map"), ("n", "normal_map"), ("s", "specular_map")):
            if key in b and len(sel):
                mw, mh, _ = U.load_bmp(b[key])
                tx, ty = S.tex_coords(o.bvh(k)["tris"], exp["triangle_id"][sel], exp["hits"][sel, 4], exp["hits"][sel, 5])
                out[kind] += len(np.unique(S.map_index((mw, mh), tx, ty)))
    return out
