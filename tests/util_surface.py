"""What rtx_surface_rays / Scene.surface_rays must write for any n x 6 ray array, from what is already pinned to the CPU oracle:
  hits      OracleScene.probe's records;
  normal    the oracle exposes hitNormal only as N / 2 + 0.5: the probe under showNormals gives the colour every ray's normal / 2 + 0.5
            must equal (the exact bits of N come from render_aov of another view, tests/test_gpu_surface.py);
  albedo    the probe's colour at a miss (getSkybox(dir)); at a hit tests/util_aov.expected's construction on these hit records -- the
            scene file's colour, or the texel of the loaded diffuse map at tests/util_shading's restated index;
  specular  the same construction: ((R + G) + B) / 3.0f of the loaded texel of a specular map (loadSpecularMap), else the ks of
            material=phong,ka,kd,ks,n, else the loader's default 1.0; 0 at a miss;
  position  rays[:, :3] + rays[:, 3:] * tNear in numpy float32, a product then a sum; 0 at a miss.
Also the ray sets of the tests: (A) the view's camera rays, (B) bounce rays leaving the first hits in twelve directions, (C) another
camera's rays, (D) tests/util_rays.probe_rays."""
import hashlib
import os

import numpy as np

from tests import util_ao as AO
from tests import util_aov as U
from tests import util_rays
from tests.util_aov import load_bmp, object_blocks
from tests.util_shading import map_index, tex_coords

f32 = np.float32
ROOT = U.ROOT
CHANNELS = ("hits", "position", "normal", "albedo", "specular")
TAIL = {"hits": (8,), "position": (3,), "normal": (3,), "albedo": (3,), "specular": ()}
DEFAULT_SPECULAR = f32(1.0)          # Object::specular (objects.h)
SCENES = U.REPO_SCENES + U.FAMILY_SCENES + ["mixed_nrm"]
# the family scenes whose meshes carry normal maps (and specular maps): (A) and (B) must reach them
MAPPED = ["plain_nrm", "uvwild", "mixed_nrm"]
# another pose per scene for (C): (position offset, rotation offset in degrees) from the scene's own camera
OTHER_POSE = (f32([0.9, 0.5, -0.4]), f32([-7, 14, 5]))


def size_of(name):
    """tests/util_aov.size_of, but 40x24 for mixed_nrm, which that list does not hold, and for uvwild, whose 33x17 there reaches too few
    texels of its specular maps (tests/test_surface_cpu.py)."""
    return (40, 24) if name in ("mixed_nrm", "uvwild") else U.size_of(name)


def probe_rays():
    """(D): zero and tiny direction components included"""
    return util_rays.probe_rays(4096)


def bounce_rays(rays, depth, normal, hit):
    """(B): from the first hits of a frame (its primary rays, tNear, N and hit mask, row-major) in sphere_directions(12), as rtx_render_ao
    would trace them"""
    return AO.traced_rays(rays, depth, normal, hit, AO.DIRS19[:12])[3]


def oracle_bounce_rays(oracle, path, w, h, cull):
    """(B) from the oracle alone: N decoded from the showNormals colour (an ulp or two from hitNormal: the rays are rays all the same)"""
    exp = U.expected_of(path, w, h, cull)
    o = oracle.OracleScene(path, w, h)
    rays = U.primary_rays(o)
    o.close()
    return bounce_rays(rays, exp["depth"], AO.decoded_normals(exp), exp["hit"] & U.written_mask(w, h))


def specular_of(block):
    m = block.get("material", "").split(",")
    return f32(float(m[3])) if m[0] == "phong" else DEFAULT_SPECULAR


def expected(o, text, rays):
    """The five channels of `rays` in OracleScene o (loaded from a scene file with this text) under o's current culling flag; also `hit`,
    `normal_colour` (the showNormals colours at hits), `object_id`, `triangle_id`, and per object with a map the texel indices the hits
    fetched: `spec_texels` / `normal_hits` {object: ...}."""
    from oracle import oracle as O
    rays = np.ascontiguousarray(rays, f32)
    hits, col = o.probe(rays)
    O.lib().orc_set_flag(o.h, b"showNormals", 1)
    hits_n, ncol = o.probe(rays)
    O.lib().orc_set_flag(o.h, b"showNormals", 0)
    assert np.array_equal(U.bits(hits), U.bits(hits_n))
    hit = hits[:, 0] > 0
    obj = hits[:, 1].astype(np.int32)
    tri = hits[:, 2].astype(np.int32)
    assert np.array_equal(obj >= 0, hit)
    albedo = col.copy()                    # a miss: getSkybox(dir), what castRay returns for it
    specular = np.zeros(len(rays), f32)
    blocks = object_blocks(text)
    assert len(blocks) == o.n_objects
    spec_texels, normal_hits = {}, {}
    for k, b in enumerate(blocks):
        sel = np.nonzero(obj == k)[0]
        if "normal_map" in b:
            normal_hits[k] = len(sel)
        if "specular_map" in b:
            spec_texels[k] = 0
        if not len(sel):
            continue
        if "diffuse_map" not in b:
            albedo[sel] = np.array([float(x) for x in b["color"].split(",")], f32)
        specular[sel] = specular_of(b)
        if "diffuse_map" in b or "specular_map" in b:
            tx, ty = tex_coords(o.bvh(k)["tris"], tri[sel], hits[sel, 4], hits[sel, 5])
        if "diffuse_map" in b:
            mw, mh, img = load_bmp(b["diffuse_map"])
            albedo[sel] = img[map_index((mw, mh), tx, ty)]
        if "specular_map" in b:
            mw, mh, img = load_bmp(b["specular_map"])
            at = map_index((mw, mh), tx, ty)
            specular[sel] = (((img[:, 0] + img[:, 1]) + img[:, 2]) / f32(3.0))[at]
            spec_texels[k] = len(np.unique(at))
    with np.errstate(all="ignore"):
        position = rays[:, 0:3] + rays[:, 3:6] * hits[:, 3:4]
    position[~hit] = 0
    assert position.dtype == f32 and specular.dtype == f32 and albedo.dtype == f32
    return dict(hits=hits, position=position, normal_colour=ncol, albedo=albedo, specular=specular, hit=hit, object_id=obj, triangle_id=tri,
                spec_texels=spec_texels, normal_hits=normal_hits)


_cache = {}


def expected_of(path, w, h, cull, rays):
    """expected() of a scene file for these rays, computed once per (file, size, culling, rays) and shared read-only among the tests."""
    from oracle import oracle as O
    rays = np.ascontiguousarray(rays, f32)
    key = (str(path), int(w), int(h), cull, hashlib.sha1(rays.tobytes()).hexdigest())
    if key not in _cache:
        o = O.OracleScene(str(path), int(w), int(h))
        if cull is not None:
            O.lib().orc_set_flag(o.h, b"useBackfaceCulling", int(cull))
        e = expected(o, open(path if os.path.isabs(path) else os.path.join(ROOT, path)).read(), rays)
        o.close()
        for v in e.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[key] = e
    return _cache[key]


def mismatches(got, exp, channels=None):
    """{channel: number of rays whose bits differ from the expectation}: empty = equal, over every ray.  got: channel -> numpy array.
    The normal is compared as normal / 2 + 0.5 in float32 with the showNormals colours at hits and as (0, 0, 0) at misses."""
    bad = {}
    for c in channels or [c for c in CHANNELS if c in got]:
        g = got[c]
        assert g.dtype == f32 and g.shape == (len(exp["hit"]),) + TAIL[c], c
        if c == "normal":
            enc = g / f32(2) + f32(0.5)
            d = np.where(exp["hit"][:, None], U.bits(enc) != U.bits(exp["normal_colour"]), U.bits(g) != 0).any(-1)
        else:
            d = U.bits(g) != U.bits(exp[c])
            d = d.any(-1) if d.ndim == 2 else d
        if d.any():
            bad[c] = int(d.sum())
    return bad


def same(a, b, channels=CHANNELS):
    """names of the channels whose bits differ between two results, over every ray"""
    return [c for c in channels if not np.array_equal(U.bits(a[c]), U.bits(b[c]))]
