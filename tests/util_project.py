"""What rtx_project_points / Scene.project_points must write (include/rtx_project.h), restated in numpy operation by operation on np.float32.
dist and L come from the pieces tests/util_points.PointPlan already uses for an area light's sample -- sqrt of the float64 of the fp32 dot
product (geometry.h:99-102), and the oracle's normalize (its array form) --; dot products are util_light.dot's (summed x, y, z).
Visibility is an input: the answers to shadow_rays / shadow_tmax, from tests/util_occlusion (the oracle) or Scene.occluded -- neither is the
code under test."""
import numpy as np

from tests import util_ao as AO
from tests import util_light as UL

f32 = np.float32
BIAS = AO.BIAS
FRONT, INSIDE, FACING, OPEN = 1, 2, 4, 8
CAMERA_FLOATS = 24
CHANNELS = ("pixel", "depth", "flags")

# The second camera of cfg1_simple_shapes (chosen by tests/test_project_cpu.py with the oracle's occlusion answers) and the camera with
# another fov for a non-square frame; the scenes' own camera is ((0, 0, 0), (0, 0, 0)) at the scene's fov.
SECOND_CAMERA = ((-5.0, 1.0, -3.0), (-10.0, 70.0, 0.0))
WIDE_CAMERA = ((-1.5, 2.5, 1.0), (-25.0, -20.0, 5.0), 65.0)
WIDE_SIZE = (57, 31)


def record(scale, aspect, m, pos, w, h):
    """One record of cameras_dev from the camera fields (OracleScene.camera() or Scene.camera(), and the size)"""
    r = np.zeros(CAMERA_FLOATS, f32)
    r[0:3] = pos
    r[3:7] = (scale, aspect, w, h)
    r[8:24] = np.asarray(m, f32).reshape(16)
    return r


def bits(a):
    """The bits of a float32 array, every NaN as one pattern: 0 / 0 is 0xFFC00000 on the host and 0x7FC00000 on the device, and the contract
    says NaN, not which"""
    a = np.ascontiguousarray(a)
    if a.dtype != np.float32:
        return a
    b = a.view(np.uint32).copy()
    b[np.isnan(a)] = 0x7FC00000
    return b


class Plan:
    """Steps 1 to 5 of the contract up to the visibility for n points {P, N} and K camera records: pixel (K, n, 2), depth (K, n), geo (K, n)
    uint8 = FRONT | INSIDE | FACING, walk (K, n) bool = the pairs whose shadow ray is cast, and those rays camera-major: shadow_rays
    (m, 6) = {O, -L}, shadow_tmax (m,) = dist."""

    def __init__(self, points, table, bias=BIAS):
        from oracle import oracle as O
        points = np.ascontiguousarray(points, f32).reshape(-1, 6)
        table = np.ascontiguousarray(table, f32).reshape(-1, CAMERA_FLOATS)
        n, K = len(points), len(table)
        self.n, self.K = n, K
        P, N = points[:, 0:3], points[:, 3:6]
        self.pixel = np.zeros((K, n, 2), f32)
        self.depth = np.zeros((K, n), f32)
        self.geo = np.zeros((K, n), np.uint8)
        self.walk = np.zeros((K, n), bool)
        rays, tmax = [], []
        with np.errstate(all="ignore"):
            Oo = (P + N * f32(bias)).astype(f32)
            for k in range(K):
                R = table[k]
                C, scale, aspect, width, height, M = R[0:3], R[3], R[4], R[5], R[6], R[8:24]
                c = (P - C[None, :]).astype(f32)
                dist = np.sqrt(UL.dot(c, c).astype(np.float64)).astype(f32)          # geometry.h:99-102
                L = O.normalize_n(c) if n else np.zeros((0, 3), f32)
                sx = (c[:, 0] * M[0] + c[:, 1] * M[1]) + c[:, 2] * M[2]
                sy = (c[:, 0] * M[4] + c[:, 1] * M[5]) + c[:, 2] * M[6]
                sz = (c[:, 0] * M[8] + c[:, 1] * M[9]) + c[:, 2] * M[10]
                inz = -sz
                xp, yp = sx / inz, sy / inz
                ax = scale * aspect
                px = (xp / ax + f32(1)) * (width * f32(0.5)) - f32(1)
                py = (f32(1) - yp / scale) * (height * f32(0.5)) - f32(1)
                assert px.dtype == f32 and py.dtype == f32 and dist.dtype == f32 and type(ax) is f32
                front = sz < 0
                inside = front & (px >= f32(-0.5)) & (px < width - f32(1.5)) & (py >= f32(-0.5)) & (py < height - f32(1.5))
                nL = -L
                facing = UL.dot(N, nL) > 0
                self.pixel[k, :, 0], self.pixel[k, :, 1], self.depth[k] = px, py, dist
                self.geo[k] = front * FRONT + inside * INSIDE + facing * FACING
                self.walk[k] = inside & ~np.isnan(dist)
                sel = self.walk[k]
                rays.append(np.concatenate([Oo[sel], nL[sel]], 1))
                tmax.append(dist[sel])
        self.shadow_rays = np.ascontiguousarray(np.concatenate(rays) if rays else np.zeros((0, 6), f32), f32)
        self.shadow_tmax = np.ascontiguousarray(np.concatenate(tmax) if tmax else np.zeros(0, f32), f32)

    def flags(self, occluded=None):
        """(K, n) uint8: the geometric flags, and OPEN from one byte per shadow ray (1: occluded); None: with_visibility = 0"""
        fl = self.geo.copy()
        if occluded is not None:
            occluded = np.asarray(occluded).reshape(-1)
            assert len(occluded) == int(self.walk.sum())
            fl[self.walk] |= np.where(occluded == 0, OPEN, 0).astype(np.uint8)
        return fl

    def expected(self, occluded=None):
        return {"pixel": self.pixel, "depth": self.depth, "flags": self.flags(occluded)}

    def nearest(self):
        """floor(p + 0.5) of every pair as float32 (K, n, 2): not an integer type, so that inf and NaN stay what they are"""
        with np.errstate(all="ignore"):
            return np.floor(self.pixel + f32(0.5))

    def shares(self, occluded):
        """(open, blocked) as shares of the pairs that are FRONT && INSIDE, and the share of all pairs that fail FRONT or INSIDE"""
        occluded = np.asarray(occluded).reshape(-1)
        inside = (self.geo & INSIDE) != 0
        m = max(int(self.walk.sum()), 1)
        return float((occluded == 0).sum()) / m, float((occluded != 0).sum()) / m, float((~inside).sum()) / inside.size


def differing(got, exp, channels=CHANNELS):
    """channel -> number of pairs whose bits differ"""
    out = {}
    for c in channels:
        a, b = bits(got[c]), bits(exp[c])
        assert a.shape == b.shape, (c, a.shape, b.shape)
        d = a != b
        if d.any():
            out[c] = int(d.reshape(d.shape[0], d.shape[1], -1).any(-1).sum())
    return out


def special_points(table, seed=0x9807):
    """Points of the special classes, for every camera record of `table`: behind the camera, at the camera's position (c == 0), and with
    sz == 0 exactly (on the plane through the camera across its axis: P = C + a * right + b * up with small integers a and b, exact in fp32
    for the cameras used here only when the products are -- so the caller checks that the class is present, not this function).  Normals:
    towards the camera, away from it, zero."""
    rng = np.random.default_rng(seed)
    out = []
    for R in np.asarray(table, f32).reshape(-1, CAMERA_FLOATS):
        C, M = R[0:3], R[8:24].reshape(4, 4)
        right, up, back = M[0, 0:3], M[1, 0:3], M[2, 0:3]
        for j in range(8):
            behind = (C + back * f32(0.5 + j) + right * f32(rng.uniform(-1, 1))).astype(f32)
            out.append(np.concatenate([behind, -back]))
            out.append(np.concatenate([C, (up, -up, np.zeros(3, f32), back)[j % 4]]))
        # sz == 0: along the world axis the camera's axis has no component of, if there is one; else a = 1, b = 0 (sz is then the dot
        # product of two rows of the matrix: zero only as far as the matrix is orthogonal in fp32)
        for axis in range(3):
            e = np.zeros(3, f32); e[axis] = 1
            if back[axis] == 0:
                out.append(np.concatenate([(C + e * f32(2)).astype(f32), -e]))
                out.append(np.concatenate([(C - e * f32(0.75)).astype(f32), e]))
        out.append(np.concatenate([(C + right).astype(f32), -right]))
    return np.ascontiguousarray(np.array(out, f32))
