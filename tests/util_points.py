"""What rtx_light_points / Scene.light_points and rtx_ao_points / Scene.ao_points must write (include/rtx_points.h), restated in numpy
float32 from the pieces tests/util_light.py and tests/util_ao.py already pin to the CPU oracle: OracleScene.illuminate, oracle.normalize /
reflect / powf, the float64 attenuation, max0, dot and in_order_sum.

PointPlan differs from util_light.Plan only in taking P as given -- it is not recomputed from a ray, so a -0 component of P stays -0 --
and in taking castRay's dir and the exponent from the caller's view record; Plan.reduce then runs unchanged.  Visibility is an input:
the answers to shadow_rays / shadow_tmax (light) or to the traced rays (AO), from tests/util_occlusion (the oracle) or Scene.occluded --
neither is the code under test."""
import numpy as np

from tests import util_ao as AO
from tests import util_light as UL

f32 = np.float32
BIAS = AO.BIAS
SUMS = ("diffuse", "specular")
PER_LIGHT = ("light_diffuse", "light_specular", "light_open")
CHANNELS = SUMS + PER_LIGHT


class PointPlan(UL.Plan):
    """Steps 2 of the light contract up to the visibility for n points: points n x 6 {P, N}; view n x 4 {V, ns} or None (no specular:
    dir is 0 and the specular channels of reduce() mean nothing).  Every point counts as a hit.  Attributes as util_light.Plan's."""

    def __init__(self, o, lights, points, view=None, bias=BIAS):
        recs, pts = lights
        assert o is None or o.n_lights == len(recs)
        points = np.ascontiguousarray(points, f32)
        self.n, self.recs = len(points), recs
        self.hit = np.ones(self.n, bool)
        self.idx = np.arange(self.n)
        m = self.n
        self.P = points[:, 0:3].copy()                       # (as given)
        self.N = points[:, 3:6].copy()
        with np.errstate(all="ignore"):
            self.O = self.P + self.N * f32(bias)
        self.dir = np.ascontiguousarray(view[:, 0:3], f32) if view is not None else np.zeros((m, 3), f32)
        self.ns = np.ascontiguousarray(view[:, 3], f32) if view is not None else np.zeros(m, f32)
        assert self.P.dtype == f32 and self.O.dtype == f32
        self.lights = []              # per light: (I (m, 3), L (m, S, 3), dist (m, S))
        first = 0
        for li, r in enumerate(recs):
            if r["type"] == UL.AREA:
                S = int(r["n_points"])
                p = pts[first:first + S]
                first += S
                with np.errstate(all="ignore"):
                    d0 = self.P - r["pos"]
                    I = r["color"][None, :] * UL.attenuation(r["intensity"], UL.dot(d0, d0))[:, None]
                    Ld = (self.P[:, None, :] - p[None, :, :]).astype(f32)
                    dist = np.sqrt(UL.dot(Ld, Ld).astype(np.float64)).astype(f32)      # geometry.h:99-102
                L = UL._rows("normalize", Ld)
            else:
                out = o.illuminate(li, self.P) if m else np.zeros((0, 8), f32)
                L, I, dist = out[:, None, 0:3].copy(), out[:, 3:6].copy(), out[:, 6:7].copy()
            self.lights.append((I.astype(f32), L.astype(f32), dist.astype(f32)))
        ray_parts, tmax_parts = [], []
        for I, L, dist in self.lights:
            for k in range(L.shape[1]):
                ray_parts.append(np.concatenate([self.O, -L[:, k]], 1))
                tmax_parts.append(dist[:, k])
        self.shadow_rays = np.ascontiguousarray(np.concatenate(ray_parts) if ray_parts else np.zeros((0, 6), f32), f32)
        self.shadow_tmax = np.ascontiguousarray(np.concatenate(tmax_parts) if tmax_parts else np.zeros(0, f32), f32)

    def reduce(self, occluded, ns=None):
        """The five light channels over all n points from one byte per shadow ray (1: occluded); ns: the view's, unless given."""
        return UL.Plan.reduce(self, occluded, self.ns if ns is None else ns)

    def classes(self, occluded):
        """(lit, shadowed while facing the light, turned away, total) over the (point, light) pairs: a pair faces the light when some
        sample has max0(N . -L) > 0, is lit when such a sample is open, shadowed when none of them is"""
        occluded = np.asarray(occluded).reshape(-1)
        lit = shadowed = away = total = 0
        at = 0
        for I, L, dist in self.lights:
            S = L.shape[1]
            occ = occluded[at:at + self.n * S].reshape(S, self.n).T
            at += self.n * S
            facing = UL.max0(UL.dot(np.broadcast_to(self.N[:, None, :], L.shape), -L)) > 0
            some = (facing & (occ == 0)).any(1)
            lit += int(some.sum()); shadowed += int((facing.any(1) & ~some).sum()); away += int((~facing.any(1)).sum())
            total += self.n
        return lit, shadowed, away, total


def ao_traced_rays(points, dirs, bias=BIAS):
    """Step 2 of rtx_render_ao's contract per point: (traced [n, K] bool, pt, k, out) -- out[j] = {O[pt[j]], dirs[k[j]]}, the traced rays
    in point-major order (util_ao.traced_rays with P as given and every point a hit)."""
    points = np.ascontiguousarray(points, f32); dirs = np.asarray(dirs, f32)
    P, N = points[:, 0:3], points[:, 3:6]
    with np.errstate(all="ignore"):
        O = P + N * f32(bias)
        c = (N[:, 0:1] * dirs[None, :, 0] + N[:, 1:2] * dirs[None, :, 1]) + N[:, 2:3] * dirs[None, :, 2]
        traced = c > 0
    assert O.dtype == f32 and c.dtype == f32
    pt, k = np.nonzero(traced)
    return traced, pt, k, np.ascontiguousarray(np.concatenate([O[pt], dirs[k]], 1).astype(f32))


def ao_reduce(traced, pt, occluded):
    """Step 3: (counts uint32 (n,), ao float32 (n,)) from one byte per traced ray -- util_ao.reduce"""
    return AO.reduce(traced, pt, occluded, (traced.shape[0],))


def same(a, b, channels):
    return UL.same(a, b, channels)
