"""What rtx_render_aov / Scene.render_aov must write, from the CPU oracle alone: pass 1's primary rays (tests/ac_heatmap.rays with the first
0.5 added here, the second by the function), their hit records and miss colours (OracleScene.probe), N / 2 + 0.5 from the probe under
showNormals, and the albedo from the scene file's colours and -- for a mesh with a diffuse map -- the texel that tests/util_shading's
restated index arithmetic selects from the loaded image."""
import functools
import os
import struct

import numpy as np

from tests import ac_heatmap as A
from tests.util_shading import map_index, tex_coords

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHANNELS = ("depth", "object_id", "triangle_id", "uv", "normal", "albedo")
GEOMETRY = ("depth", "object_id", "triangle_id", "uv")
FLT_MAX_BITS = 0x7F7FFFFF
# the sizes of the GPU tests: none a multiple of 8 in both directions (partial tiles), wide, tall and odd
SIZES = [(40, 24), (24, 40), (33, 17)]
REPO_SCENES = ["cfg1_simple_shapes", "cfg3_reflective_refractive", "mixed_materials", "coincident", "cfg2_smooth_4k", "cfg4_textured_256",
               "area_light"]
# of tests/util_shading.FAMILY: a NORMAL_MAPPED scene, wild texture coordinates, non-square maps with the skybox on (every one has both)
FAMILY_SCENES = ["plain_nrm", "uvwild", "plain"]


def size_of(name):
    """Every scene at one of SIZES, spread by position in the lists."""
    names = REPO_SCENES + FAMILY_SCENES
    return SIZES[names.index(name) % len(SIZES)]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def primary_rays(o):
    """pass 1's ray of every pixel, row-major (renderWorker scene.cpp:444-468: x + 0.5 and getPixels' own 0.5): n x 6 float32"""
    scale, aspect, m, pos = o.camera()
    ys, xs = np.mgrid[0:o.height, 0:o.width]
    org, d = A.rays(scale, aspect, m, pos, o.width, o.height, xs.ravel().astype(f32) + f32(0.5), ys.ravel().astype(f32) + f32(0.5))
    return np.concatenate([org, d], 1).astype(f32)


def object_blocks(text):
    """[{key: value text}] of the [object] blocks of a scene file, in file order"""
    out, cur = [], None
    for ln in text.split("\n"):
        s = ln.strip()
        if s.startswith("["):
            cur = {} if s == "[object]" else None
            if cur is not None:
                out.append(cur)
        elif cur is not None and "=" in s and not s.startswith("#"):
            k, v = s.split("=", 1)
            cur[k.strip()] = v.strip()
    return out


def load_bmp(path):
    """A 24-bpp bottom-up BMP as the loaders keep it: (width, height, float32 [h * w, 3] RGB / 256, rows in file order)."""
    raw = open(path if os.path.isabs(path) else os.path.join(ROOT, path), "rb").read()
    off, = struct.unpack_from("<I", raw, 10)
    w, h, _, bpp = struct.unpack_from("<iiHH", raw, 18)
    assert raw[:2] == b"BM" and bpp == 24 and h > 0 and w % 4 == 0, path
    px = np.frombuffer(raw, np.uint8, w * h * 3, off).reshape(h * w, 3)[:, ::-1]
    return w, h, px.astype(f32) / f32(256)


def expected(o, text):
    """The six channels of OracleScene o (loaded from a scene file with this text) as arrays of the frame's shape, under o's current culling
    flag; also `hit`, `normal_colour` (the showNormals colours, what normal / 2 + 0.5 is compared with) and `shaded` (the ordinary colours)."""
    from oracle import oracle as O
    W, H = o.width, o.height
    rays = primary_rays(o)
    hits, col = o.probe(rays)
    O.lib().orc_set_flag(o.h, b"showNormals", 1)
    hits_n, ncol = o.probe(rays)
    O.lib().orc_set_flag(o.h, b"showNormals", 0)
    assert np.array_equal(bits(hits), bits(hits_n))
    hit = hits[:, 0] > 0
    obj = hits[:, 1].astype(np.int32)
    tri = hits[:, 2].astype(np.int32)
    assert np.array_equal(obj >= 0, hit)
    albedo = col.copy()                    # a miss: getSkybox(dir), what castRay returns for it
    blocks = object_blocks(text)
    assert len(blocks) == o.n_objects
    for k, b in enumerate(blocks):
        sel = np.nonzero(obj == k)[0]
        if not len(sel):
            continue
        if "diffuse_map" in b:
            mw, mh, img = load_bmp(b["diffuse_map"])
            tx, ty = tex_coords(o.bvh(k)["tris"], tri[sel], hits[sel, 4], hits[sel, 5])
            albedo[sel] = img[map_index((mw, mh), tx, ty)]
        else:
            albedo[sel] = np.array([float(x) for x in b["color"].split(",")], f32)
    return dict(depth=hits[:, 3].reshape(H, W).copy(), object_id=obj.reshape(H, W), triangle_id=tri.reshape(H, W),
                uv=hits[:, 4:6].reshape(H, W, 2).copy(), normal_colour=ncol.reshape(H, W, 3), albedo=albedo.reshape(H, W, 3),
                hit=hit.reshape(H, W), shaded=col.reshape(H, W, 3))


def vertex_normal_colour(o, exp):
    """N / 2 + 0.5 of the interpolated vertex normal alone (objects.cpp:132-134, no normal map) at the mesh pixels of `exp`, and their mask."""
    H, W = exp["hit"].shape
    out = np.zeros((H, W, 3), f32)
    mesh = exp["triangle_id"] >= 0
    for k in np.unique(exp["object_id"][mesh]):
        sel = mesh & (exp["object_id"] == k)
        t = o.bvh(int(k))["tris"][exp["triangle_id"][sel]]
        u, v = exp["uv"][sel][:, 0:1], exp["uv"][sel][:, 1:2]
        n = (t[:, 12:15] * u + t[:, 15:18] * v + t[:, 9:12] * (f32(1) - u - v)) / f32(3)
        out[sel] = A._normalize(n.astype(f32)) / f32(2) + f32(0.5)
    return out, mesh


@functools.lru_cache(maxsize=None)
def _cached(path, w, h, cull):
    from oracle import oracle as O
    o = O.OracleScene(path, w, h)
    if cull is not None:
        O.lib().orc_set_flag(o.h, b"useBackfaceCulling", int(cull))
    e = expected(o, open(path if os.path.isabs(path) else os.path.join(ROOT, path)).read())
    o.close()
    for v in e.values():
        v.setflags(write=False)
    return e


def expected_of(path, w, h, cull=None):
    """expected() of a scene file, computed once per (file, size, culling) and shared read-only among the tests."""
    return _cached(str(path), int(w), int(h), cull)


def written_mask(w, h, rows=None, band=0, parts=1, part=0):
    """The pixels a call writes: x < w-1, y < h-1, y in rows, and of the bands of `band` rows those that part `part` of `parts` owns."""
    y = np.arange(h)
    ok = y < h - 1
    if rows is not None:
        ok &= (y >= rows[0]) & (y < rows[1])
    if band:
        ok &= (y // band) % parts == part
    m = np.zeros((h, w), bool)
    m[ok, : w - 1] = True
    return m


def mismatches(got, exp, mask, channels=CHANNELS):
    """{channel: number of pixels of `mask` whose bits differ from the expectation}: empty = equal.  got: channel -> numpy array of the frame.
    The normal is compared as normal / 2 + 0.5 in float32 with the showNormals colours at hits and as (0, 0, 0) at misses."""
    bad = {}
    for c in channels:
        g = got[c]
        if c == "normal":
            enc = g / f32(2) + f32(0.5)
            d = np.where(exp["hit"][..., None], bits(enc) != bits(exp["normal_colour"]), bits(g) != 0).any(-1)
        else:
            d = bits(g) != bits(exp[c])
            d = d.any(-1) if d.ndim == 3 else d
        if d[mask].any():
            bad[c] = int(d[mask].sum())
    return bad
