"""include/rtx_bake.h restated in numpy, operation by operation (np.float32 / np.float64 scalars and arrays: no operation is fused), and the
meshes the texel-point tests run on.  texel_points_ref is what rtx_texel_points must give bit for bit; dilate_ref what rtx_dilate_texels must.
A triangle is only looked at on the texels whose centre lies in its UV bounding box: the contract's own condition, which also keeps the
250k-triangle mesh within reach of a Python loop (tools/texel_points_time.py times it)."""
import os

import numpy as np

from tests.util_deform import SCENE

f32, f64 = np.float32, np.float64
NEIGHBOURS = ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (1, -1), (-1, 1), (1, 1))      # (di, dj), the header's order


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def centres(n):
    """cx of texels 0 .. n-1: ((float)i + 0.5f) / (float)n."""
    return ((np.arange(n, dtype=np.int64).astype(f32) + f32(0.5)) / f32(n)).astype(f32)


def _edge_raw(px, py, qx, qy, cx, cy):
    return (f64(qx) - f64(px)) * (cy.astype(f64) - f64(py)) - (f64(qy) - f64(py)) * (cx.astype(f64) - f64(px))


def edge(px, py, qx, qy, cx, cy):
    """E(p, q, c) in canonical form; cx, cy: float32 arrays of one shape."""
    if px > qx or (px == qx and py > qy):
        return -_edge_raw(qx, qy, px, py, cx, cy)
    return _edge_raw(px, py, qx, qy, cx, cy)


def weights(uv6, cx, cy):
    """(w_a, w_b, w_c, D) of a triangle with UV corners uv6 = (ax, ay, bx, by, cx, cy) at the centres."""
    ax, ay, bx, by, qx, qy = (f32(v) for v in uv6)
    wa = edge(bx, by, qx, qy, cx, cy)
    wb = edge(qx, qy, ax, ay, cx, cy)
    wc = edge(ax, ay, bx, by, cx, cy)
    return wa, wb, wc, (wa + wb) + wc


def covers(wa, wb, wc, D):
    with np.errstate(invalid="ignore"):
        return ((D > 0) & (wa >= 0) & (wb >= 0) & (wc >= 0)) | ((D < 0) & (wa <= 0) & (wb <= 0) & (wc <= 0))


def texel_points_ref(tri_pos, tri_nrm, tri_uv, w, h, normalize=None):
    """dict(points (h*w, 6), tri (h, w) int32, bary (h, w, 2)) of a w x h map over the triangles (T, 9), (T, 9), (T, 6), float32.
    normalize: Vec3::normalize over (n, 3) float32 -- oracle.normalize_n; None leaves N = M (the tests of the restatement's own properties)."""
    tri_pos, tri_nrm, tri_uv = (np.ascontiguousarray(a, f32) for a in (tri_pos, tri_nrm, tri_uv))
    T = tri_uv.shape[0]
    cxs, cys = centres(w), centres(h)
    tri = np.full((h, w), -1, np.int32)
    wb_o, wc_o, D_o = (np.zeros((h, w), f64) for _ in range(3))
    for t in range(T):
        uv = tri_uv[t]
        if np.isnan(uv).any():
            continue                                   # (some edge function is NaN at every centre: covers nothing)
        xs, ys = uv[0::2], uv[1::2]
        # the centres inside the bounding box, fp32 comparisons, closed (the centres are sorted)
        i0, i1 = np.searchsorted(cxs, xs.min(), "left"), np.searchsorted(cxs, xs.max(), "right")
        j0, j1 = np.searchsorted(cys, ys.min(), "left"), np.searchsorted(cys, ys.max(), "right")
        if i0 >= i1 or j0 >= j1:
            continue
        cx, cy = np.meshgrid(cxs[i0:i1], cys[j0:j1])
        with np.errstate(invalid="ignore", over="ignore"):
            wa, wb, wc, D = weights(uv, cx, cy)
        take = covers(wa, wb, wc, D) & (tri[j0:j1, i0:i1] == -1)      # (t ascends: the lowest index owns)
        if take.any():
            tri[j0:j1, i0:i1][take] = t
            wb_o[j0:j1, i0:i1][take] = wb[take]; wc_o[j0:j1, i0:i1][take] = wc[take]; D_o[j0:j1, i0:i1][take] = D[take]
    own = tri >= 0
    bu, bv = np.zeros((h, w), f32), np.zeros((h, w), f32)
    bu[own] = (wb_o[own] / D_o[own]).astype(f32)
    bv[own] = (wc_o[own] / D_o[own]).astype(f32)
    points = np.zeros((h, w, 6), f32)
    if own.any():
        t = tri[own]
        u, v = bu[own][:, None], bv[own][:, None]
        k = (f32(1.0) - u) - v
        A, B, Cc = tri_pos[t, 0:3], tri_pos[t, 3:6], tri_pos[t, 6:9]
        na, nb, nc = tri_nrm[t, 0:3], tri_nrm[t, 3:6], tri_nrm[t, 6:9]
        with np.errstate(invalid="ignore", over="ignore"):
            P = (B * u + Cc * v) + A * k
            M = ((nb * u + nc * v) + na * k) / f32(3)
        N = M if normalize is None else normalize(np.ascontiguousarray(M, f32)).reshape(-1, 3)
        points[own] = np.concatenate([P, N], 1).astype(f32)
    return dict(points=points.reshape(h * w, 6), tri=tri, bary=np.stack([bu, bv], 2))


def tex_coord(tri_uv, tri, bary):
    """objects.cpp:125's texCoord in fp32 at (bu, bv) for the covered texels: (t_b * u + t_c * v) + t_a * (1 - u - v) per component; rows in
    the order of np.nonzero(tri >= 0)."""
    own = tri >= 0
    t = tri[own]
    u, v = bary[own][:, 0:1].astype(f32), bary[own][:, 1:2].astype(f32)
    k = (f32(1.0) - u) - v
    ta, tb, tc = tri_uv[t, 0:2], tri_uv[t, 2:4], tri_uv[t, 4:6]
    return ((tb * u + tc * v) + ta * k).astype(f32)


def dilate_ref(image, tri, passes):
    """rtx_dilate_texels: (image, tri) after `passes` passes; image (h, w, C) or (h, w) float32, tri (h, w) int32; copies."""
    image, tri = np.array(image, f32, copy=True), np.array(tri, np.int32, copy=True)
    h, w = tri.shape
    for _ in range(passes):
        t0, im0 = tri.copy(), image.copy()      # the state at the start of the pass
        for j in range(h):
            for i in range(w):
                if t0[j, i] != -1:
                    continue
                for di, dj in NEIGHBOURS:
                    ni, nj = i + di, j + dj
                    if 0 <= ni < w and 0 <= nj < h and t0[nj, ni] != -1:
                        image[j, i] = im0[nj, ni]
                        tri[j, i] = -2
                        break
    return image, tri


# ---- meshes ---------------------------------------------------------------------------------------------------------------------------
def quad_obj(lo=0.0, hi=1.0):
    """Two triangles over the square, texture coordinates (lo, lo) (hi, lo) (hi, hi) (lo, hi)."""
    return ("v -1 -1 0\nv 1 -1 0.25\nv 1 1 0\nv -1 1 0.5\nvn 0 0 1\nvn 0.2 0 1\nvn 0 0.2 1\nvn -0.2 0.1 1\n"
            "vt %g %g\nvt %g %g\nvt %g %g\nvt %g %g\nf 1/1/1 2/2/2 3/3/3\nf 1/1/1 3/3/3 4/4/4\n" % (lo, lo, hi, lo, hi, hi, lo, hi))


# One mesh for the ownership rules.  Its faces, by index:
#   0, 1  two charts that overlap (the triangles of the lower-left square's two diagonals): the lower index owns the overlap
#   2     a mirrored chart (D < 0)
#   3     a triangle whose three corners share one texture coordinate (every edge function is 0: D == 0)
#   4     a collinear one on dyadic coordinates
#   5     wholly outside [0, 1)
#   6     a NaN texture coordinate
#   7     a small chart of its own in the upper left
CHART_VT = [(0.0625, 0.0625), (0.4375, 0.0625), (0.0625, 0.4375), (0.4375, 0.4375),         # 1-4
            (0.5625, 0.0625), (0.5625, 0.4375), (0.9375, 0.0625),                              # 5-7
            (0.7, 0.7),                                                                          # 8
            (0.625, 0.625), (0.75, 0.75), (0.875, 0.875),                                        # 9-11
            (1.25, 1.25), (1.75, 1.25), (1.25, 1.75),                                            # 12-14
            (float("nan"), 0.3),                                                                 # 15
            (0.125, 0.625), (0.375, 0.6875), (0.1875, 0.9375)]                                   # 16-18
CHART_FACES = [(1, 2, 3), (1, 2, 4), (5, 6, 7), (8, 8, 8), (9, 10, 11), (12, 13, 14), (15, 2, 3), (16, 17, 18)]
CHART_OVERLAP = (0, 1)
CHART_NEVER = (3, 5, 6)


def charts_obj(reverse=False):
    rng = np.random.RandomState(7)
    lines = []
    nv = 3 * len(CHART_FACES)
    V = rng.uniform(-1, 1, (nv, 3))
    N = rng.uniform(-1, 1, (nv, 3)) + np.array([0, 0, 2.0])
    lines += ["v %.6f %.6f %.6f" % tuple(p) for p in V]
    lines += ["vn %.6f %.6f %.6f" % tuple(p) for p in N]
    lines += ["vt %s %s" % (("nan" if x != x else "%.9g" % x), "%.9g" % y) for x, y in CHART_VT]
    faces = ["f " + " ".join("%d/%d/%d" % (3 * f + k + 1, vt[k], 3 * f + k + 1) for k in range(3)) for f, vt in enumerate(CHART_FACES)]
    lines += faces[::-1] if reverse else faces
    return "\n".join(lines) + "\n"


def write_mesh_scene(d, name, obj, size="2,1.5,1", rot="20,30,10"):
    """The scene file of one mesh (tests/util_deform.SCENE: a point light and the mesh) whose OBJ file holds `obj` (text or bytes); its path."""
    p = os.path.join(str(d), name + ".obj")
    with open(p, "wb") as f:
        f.write(obj if isinstance(obj, bytes) else obj.encode())
    s = os.path.join(str(d), name + ".scene")
    with open(s, "w") as f:
        f.write(SCENE % (size, rot, p))
    return s


def triangles(scene, index=0):
    """(tri_pos, tri_nrm, tri_uv) of mesh `index` as the host holds them (what is uploaded): (T, 9), (T, 9), (T, 6) float32."""
    t = scene.bvh(index)["tris"]
    return (np.ascontiguousarray(t[:, 0:9]), np.ascontiguousarray(t[:, 9:18]), np.ascontiguousarray(t[:, 18:24]))
