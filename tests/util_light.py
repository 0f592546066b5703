"""What rtx_light_rays / Scene.light_rays must write (include/rtx_light.h), restated in numpy float32 in the order of the contract, from
what is already pinned to the CPU oracle:
  illuminate     OracleScene.illuminate for point and distant lights; for an area light the sample points as the scene holds them
                 (Scene.device_lights(), or lights_of_text's restatement of the grid for a scene file) and the attenuation in float64, cast;
  normalize, reflect, powf   the oracle's (oracle.normalize, oracle.reflect, oracle.powf), one call per element;
  visibility     answers to the shadow rays {O, -L} with tmax = dist, which the caller gets from tests/util_occlusion (the oracle) or from
                 Scene.occluded -- neither is the code under test.
The exact N of every hit is an input: Scene.surface_rays on the GPU, the stored normal of a plane / oracle.normalize(P - centre) of a sphere
without one.  Ray sets, scenes and sizes are tests/util_surface's."""
import numpy as np

from tests import util_ao as AO
from tests import util_surface as SU
from tests.util_aov import bits

f32 = np.float32
FLT_MAX = np.finfo(f32).max
BIAS = AO.BIAS
SCENES = SU.SCENES
size_of = SU.size_of
# the scenes whose (hit, light) pairs are lit, shadowed and turned away in fair shares (tests/test_light_rays_cpu.py shows it on the oracle)
SHARED_OUT = ["cfg1_simple_shapes", "coincident", "cfg2_smooth_4k", "area_light", "plain", "plain_nrm", "uvwild", "mixed_nrm"]
CHANNELS = ("hits", "diffuse", "specular", "light_diffuse", "light_specular", "light_open")
LIGHT_DTYPE = [("type", np.int32), ("color", f32, 3), ("intensity", f32), ("dir", f32, 3), ("pos", f32, 3), ("n_points", np.uint32)]
DISTANT, POINT, AREA = 1, 2, 3
# Object::nSpecular (objects.h), what a material= line without an exponent leaves
DEFAULT_N_SPECULAR = f32(5.0)


def light_blocks(text):
    """[{key: value text}] of the [light] blocks of a scene file, in file order"""
    out, cur = [], None
    for ln in text.split("\n"):
        s = ln.strip()
        if s.startswith("["):
            cur = {} if s == "[light]" else None
            if cur is not None:
                out.append(cur)
        elif cur is not None and "=" in s and not s.startswith("#"):
            k, v = s.split("=", 1)
            cur[k.strip()] = v.strip()
    return out


def lights_of_text(text):
    """(records, points) in the layout of Scene.device_lights() for a scene file's text, as far as the expectation reads them: the type of
    every light, and of an area light colour, intensity, pos and the sample grid of lights.cpp:46-63 in float32."""
    vec = lambda s: np.array([float(x) for x in s.split(",")], f32)
    blocks = light_blocks(text)
    recs = np.zeros(len(blocks), LIGHT_DTYPE)
    pts = []
    for k, b in enumerate(blocks):
        recs[k]["type"] = {"distant": DISTANT, "point": POINT, "area": AREA}[b["type"]]
        if b["type"] != "area":
            continue
        pos, i, j, s = vec(b["pos"]), vec(b["i"]), vec(b["j"]), int(b["samples"])
        recs[k]["color"], recs[k]["intensity"], recs[k]["pos"] = vec(b["color"]), f32(b["intensity"]), pos
        corner = pos - i / f32(2.0) - j / f32(2.0)
        mine = [corner + i * (f32(a) / f32(s - 1)) + j * (f32(c) / f32(s - 1)) for a in range(s) for c in range(s)] if s > 1 else [pos]
        recs[k]["n_points"] = len(mine)
        pts += mine
    return recs, np.array(pts, f32).reshape(-1, 3)


def n_specular_of(block):
    m = block.get("material", "").split(",")
    return f32(float(m[4])) if m[0] == "phong" else DEFAULT_N_SPECULAR


def max0(x):
    """std::max(0.f, x): NaN and -0 give +0"""
    with np.errstate(invalid="ignore"):
        return np.where(f32(0) < x, x, f32(0)).astype(f32)


def dot(a, b):
    """summed x, y, z in float32"""
    with np.errstate(all="ignore"):
        return ((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]).astype(f32)


def attenuation(intensity, l2):
    """fmin(1.0f, (float)(intensity / (4 pi l2 / 1000))) with the quotient in double (lights.cpp:35; scene.cpp:796, 832)"""
    with np.errstate(all="ignore"):
        x = (np.float64(f32(intensity)) / (4 * np.pi * np.asarray(l2, f32).astype(np.float64) / 1000)).astype(f32)
        return np.where(x < f32(1), x, f32(1)).astype(f32)


def _rows(fn, *arrs):
    from oracle import oracle as O
    out = np.zeros(arrs[0].shape, f32)
    flat = [a.reshape(-1, 3) for a in arrs]
    o = out.reshape(-1, 3)
    f = getattr(O, fn)
    for k in range(len(o)):
        o[k] = f(*[a[k] for a in flat])
    return out


def powf(x, y):
    from oracle import oracle as O
    x = np.asarray(x, f32); y = np.broadcast_to(np.asarray(y, f32), x.shape)
    out = np.zeros(x.shape, f32)
    for k in np.ndindex(x.shape):
        out[k] = O.powf(float(x[k]), float(y[k]))
    return out


class Plan:
    """Steps 1 and 2 of the contract up to the visibility, for the rays that hit.  o: an OracleScene of the same scene (its illuminate);
    lights: (records, points) as Scene.device_lights(); rays n x 6, hits n x 8 (rtx_trace_rays' records), N n x 3.
    shadow_rays / shadow_tmax: every shadow ray of the contract, light by light (all hits of light 0, sample 0; then sample 1; ...)."""

    def __init__(self, o, lights, rays, hits, N, bias=BIAS):
        recs, pts = lights
        assert o is None or o.n_lights == len(recs)
        rays = np.ascontiguousarray(rays, f32); hits = np.asarray(hits, f32); N = np.asarray(N, f32)
        self.n, self.recs = len(rays), recs
        self.hit = hits[:, 0] > 0
        self.idx = np.nonzero(self.hit)[0]
        m = len(self.idx)
        with np.errstate(all="ignore"):
            self.P = (rays[:, 0:3] + rays[:, 3:6] * hits[:, 3:4])[self.idx]
            self.N = N[self.idx]
            self.O = self.P + self.N * f32(bias)
        self.dir = rays[self.idx, 3:6]
        assert self.P.dtype == f32 and self.O.dtype == f32
        self.lights = []              # per light: (I (m, 3), L (m, S, 3), dist (m, S))
        first = 0
        for li, r in enumerate(recs):
            if r["type"] == AREA:
                S = int(r["n_points"])
                p = pts[first:first + S]
                first += S
                d0 = self.P - r["pos"]
                I = r["color"][None, :] * attenuation(r["intensity"], dot(d0, d0))[:, None]
                Ld = (self.P[:, None, :] - p[None, :, :]).astype(f32)
                with np.errstate(all="ignore"):
                    dist = np.sqrt(dot(Ld, Ld).astype(np.float64)).astype(f32)      # geometry.h:99-102
                L = _rows("normalize", Ld)
            else:
                out = o.illuminate(li, self.P) if m else np.zeros((0, 8), f32)
                L, I, dist = out[:, None, 0:3].copy(), out[:, 3:6].copy(), out[:, 6:7].copy()
                if r["type"] == DISTANT:
                    assert (dist == FLT_MAX).all()
            self.lights.append((I.astype(f32), L.astype(f32), dist.astype(f32)))
        ray_parts, tmax_parts = [], []
        for I, L, dist in self.lights:
            for k in range(L.shape[1]):
                ray_parts.append(np.concatenate([self.O, -L[:, k]], 1))
                tmax_parts.append(dist[:, k])
        self.shadow_rays = np.ascontiguousarray(np.concatenate(ray_parts) if ray_parts else np.zeros((0, 6), f32), f32)
        self.shadow_tmax = np.ascontiguousarray(np.concatenate(tmax_parts) if tmax_parts else np.zeros(0, f32), f32)

    def reduce(self, occluded, ns):
        """Steps 2 to 4 from one byte per shadow ray (1: occluded) and ns (n,), the hit objects' n_specular: the five light channels over
        all n rays."""
        L_ = len(self.recs)
        m = len(self.idx)
        occluded = np.asarray(occluded).reshape(-1)
        assert len(occluded) == len(self.shadow_rays)
        ns = np.asarray(ns, f32)[self.idx]
        ld = np.zeros((self.n, L_, 3), f32); ls = np.zeros((self.n, L_, 3), f32); lo = np.zeros((self.n, L_), np.int32)
        at = 0
        with np.errstate(all="ignore"):
            for li, (I, L, dist) in enumerate(self.lights):
                S = L.shape[1]
                opened = (occluded[at:at + m * S].reshape(S, m).T == 0)
                at += m * S
                Nb = np.broadcast_to(self.N[:, None, :], L.shape)
                md = max0(dot(Nb, -L))
                R = _rows("reflect", np.ascontiguousarray(L), np.ascontiguousarray(Nb))
                sd = max0(dot(R, -np.broadcast_to(self.dir[:, None, :], L.shape)))
                if self.recs[li]["type"] == AREA:
                    dsum = np.zeros(m, f32); ssum = np.zeros(m, f32)
                    for k in range(S):
                        vis = opened[:, k].astype(f32)
                        dsum = (dsum + vis * md[:, k]).astype(f32)
                        ssum = (ssum + vis * sd[:, k]).astype(f32)
                    D = (dsum / f32(S))[:, None] * I
                    Sp = powf(ssum / f32(S), ns)[:, None] * I
                else:
                    D = np.where(opened[:, 0:1], I * md[:, 0:1], f32(0))
                    Sp = np.where(opened[:, 0:1], I * powf(sd[:, 0], ns)[:, None], f32(0))
                ld[self.idx, li] = D.astype(f32); ls[self.idx, li] = Sp.astype(f32); lo[self.idx, li] = opened.sum(1)
            diffuse, specular = in_order_sum(ld), in_order_sum(ls)
        return dict(light_diffuse=ld, light_specular=ls, light_open=lo, diffuse=diffuse, specular=specular)


def in_order_sum(per_light):
    """(((+0) + t_0) + t_1) + ... over axis 1, in float32"""
    acc = np.zeros((per_light.shape[0], 3), f32)
    with np.errstate(all="ignore"):
        for li in range(per_light.shape[1]):
            acc = (acc + per_light[:, li]).astype(f32)
    return acc


def same(a, b, channels):
    """names of the channels whose bits differ between two results, over every ray"""
    return [c for c in channels if a[c].shape != b[c].shape or not np.array_equal(bits(a[c]), bits(b[c]))]


def colour_identities(colour, albedo, ks, diffuse, specular, material, ambient, kd):
    """The two identities of the contract's step 3, per ray: (is Diffuse or Phong, the colour castRay returns from the sums) --
    albedo * diffuse (scene.cpp:808) or (albedo * ambient + diffuse * kd) + specular * ks (scene.cpp:852), float32."""
    with np.errstate(all="ignore"):
        d = (albedo * diffuse).astype(f32)
        p = ((albedo * ambient[:, None] + diffuse * kd[:, None]) + specular * ks[:, None]).astype(f32)
    return (material == 0) | (material == 3), np.where((material == 0)[:, None], d, p)
