"""rtx_scatter_rays / rtx_sky_rays (Scene.scatter_rays, Scene.sky, Scene.cast_tree) without a GPU: the extension header against the symbol
list and the ctypes structure, the argument checks, tests/util_scatter's restatement of the contract pinned to the oracle one level of
castRay at a time where the exact normal is known without a GPU (planes and spheres), and the inputs of the GPU tests
(tests/test_gpu_scatter.py) shown with the oracle alone to reach every class of hit their scene is there for."""
import os
import re

import numpy as np
import pytest

from tests import util_aov as U
from tests import util_light as UL
from tests import util_occlusion as OC
from tests import util_scatter as SC
from tests import util_shading as S
from tests import util_surface as SU
from tests.ac_heatmap import scene_copy

ROOT = U.ROOT
f32 = np.float32


@pytest.fixture(scope="module")
def family(tmp_path_factory):
    d = S.short_dir(tmp_path_factory)
    return d, S.write_family(d)


def path_of(name, family):
    return family[1][name] if name in S.FAMILY else "scenes/%s.scene" % name


def text_of(path):
    return open(path if os.path.isabs(path) else os.path.join(ROOT, path)).read()


def at_depth(name, family, tmp_path, depth):
    """the scene file of `name` with max_ray_depth = depth"""
    if name in S.FAMILY:
        path = os.path.join(family[0], "%s_d%d.scene" % (name, depth))
        with open(path, "w") as f:
            f.write(S.scene_text(name, family[0], extra={"max_ray_depth": depth}))
        return path
    return scene_copy(name, str(tmp_path), dict(max_ray_depth=depth))


def test_scatter_header_and_symbol_list(ra):
    import ctypes as C
    hdr = open(os.path.join(ROOT, "include", "rtx_scatter.h")).read()
    declared = re.findall(r"^int\s+(rtx_[a-z0-9_]+)\s*\(", hdr, re.M)
    assert declared == list(ra.RTX_SCATTER_SYMBOLS) == ["rtx_scatter_rays", "rtx_sky_rays"]
    for other in (ra.RTX_SYMBOLS, ra.RTX_EDIT_SYMBOLS, ra.RTX_QUERY_SYMBOLS, ra.RTX_AOV_SYMBOLS, ra.RTX_AO_SYMBOLS, ra.RTX_SURFACE_SYMBOLS,
                  ra.RTX_LIGHT_SYMBOLS, ra.RTX_DEFORM_SYMBOLS, ra.RTX_VIEWS_SYMBOLS):
        assert not set(declared) & set(other)
    rtx, _ = ra.load()
    for s in declared:
        assert hasattr(rtx, s), s
    listed, missing = ra.exported_symbols()
    assert not missing and listed == list(ra.RTX_SYMBOLS)
    # the structure of the binding is the header's: six pointers in its order, which is the order of the channels
    body = re.search(r"typedef struct rtx_scatter_buffers \{(.*?)\} rtx_scatter_buffers;", hdr, re.S).group(1)
    fields = re.findall(r"(float\*|uint8_t\*)\s+(\w+);", body)
    assert [n for _, n in fields] == [n for n, _ in ra.ScatterBuffers._fields_] == [c + "_dev" for c in SC.CHANNELS] and len(fields) == 6
    assert [t for t, _ in fields] == ["float*"] * 5 + ["uint8_t*"]
    assert all(t is C.c_void_p for _, t in ra.ScatterBuffers._fields_) and C.sizeof(ra.ScatterBuffers) == 6 * C.sizeof(C.c_void_p)
    assert tuple(ra.Scene.SCATTER_CHANNELS) == SC.CHANNELS
    # the header states the identities the tests check
    for line in ("castRay = C(reflect) * 0.8f + local", "castRay = (((+0) + C(refract) * weight[1]) + C(reflect) * weight[0]) + local",
                 "castRay = local"):
        assert line in hdr, line


def test_c_entries_refuse_null_arguments(ra):
    import ctypes as C
    rtx, _ = ra.load()
    bufs = ra.ScatterBuffers()
    assert rtx.rtx_scatter_rays(None, 4, None, None, None) == -1      # RTX_ERR_ARG
    assert b"NULL" in rtx.rtx_last_error()
    assert rtx.rtx_scatter_rays(None, 4, None, C.byref(bufs), None) == -1
    assert b"NULL" in rtx.rtx_last_error()
    assert rtx.rtx_sky_rays(None, 4, None, None, None) == -1
    assert b"NULL" in rtx.rtx_last_error()


def test_bad_arguments_are_refused_before_the_gpu(ra):
    torch = pytest.importorskip("torch")
    s = ra.Scene("scenes/cfg1_simple_shapes.scene", 32, 24)
    z = lambda shape, dt=torch.float32: torch.zeros(shape, dtype=dt)
    off = dict(local=False, reflect=False, refract=False, weight=False, kinds=False)
    for who, fn, extra in (("scatter_rays", s.scatter_rays, [(dict(rays=z((4, 6)), **off), "scatter_rays: nothing to compute"),
                                                           (dict(rays=z((24,)), hits=True, **off), r"scatter_rays: rays must have shape \(n, 6\)")]),
                           ("sky", s.sky, []),
                           ("cast_tree", s.cast_tree, [(dict(rays=z((4, 6)), depth=-1), "cast_tree: rays must be on cuda:0"),
                                                       (dict(rays=z((6, 4)), stream=7), r"cast_tree: rays must have shape \(n, 6\)")])):
        cases = extra + [
            (dict(rays=np.zeros((4, 6), np.float32)), "%s: rays must be a torch tensor" % who),
            (dict(rays=z((4, 6), torch.float64)), "%s: rays must be float32" % who),
            (dict(rays=z((6, 4))), r"%s: rays must have shape \(n, 6\)" % who),
            (dict(rays=z((4, 12))[:, ::2]), "%s: rays must be contiguous" % who),
            (dict(rays=z((4, 6))), "%s: rays must be on cuda:0" % who),
        ]
        for kw, what in cases:
            with pytest.raises(ValueError, match=what):
                fn(**kw)
    assert s.max_ray_depth == 10           # (Options::maxRayDepth: the file sets none)
    assert s._gpu is None                  # (the scene was never flattened and uploaded: no GPU call was made)
    s.close()


def file_depth(text):
    m = re.search(r"^max_ray_depth\s*=\s*(-?\d+)", text, re.M)
    return int(m.group(1)) if m else 10


def exact_case(oracle, path, tmp_path, rays):
    """Of `rays` in the scene file `path`, those that miss or whose first hit is a plane or a sphere, with everything the restatement reads
    from the oracle and the file's text alone: hit records, the exact N (the plane's stored normal, normalize(P - centre) of a sphere),
    albedo (the sky colour at a miss), ks, the sums D and S of tests/util_light, the objects' constants.  Returns (rays, hits, N, material
    per ray, restated channels)."""
    vec = lambda s: np.array([float(x) for x in s.split(",")], f32)
    text = text_of(path)
    blocks = SU.object_blocks(text)
    const = SC.constants_of(blocks)
    o = oracle.OracleScene(path, 8, 8)
    hits, _ = o.probe(rays, colours=False)
    obj = hits[:, 1].astype(np.int32)
    ok = obj < 0
    for k, b in enumerate(blocks):
        if b["type"] in ("plane", "sphere"):
            ok |= obj == k
    rays, hits, obj = np.ascontiguousarray(rays[ok]), hits[ok], obj[ok]
    n = len(rays)
    P = rays[:, 0:3] + rays[:, 3:6] * hits[:, 3:4]
    N = np.zeros((n, 3), f32); albedo = o.skybox(rays[:, 3:6]); ks = np.zeros(n, f32)
    for k, b in enumerate(blocks):
        sel = np.nonzero(obj == k)[0]
        if not len(sel):
            continue
        if b["type"] == "plane":
            N[sel] = vec(b["normal"])
            assert np.array_equal(oracle.normalize(vec(b["normal"])), vec(b["normal"]))
        else:
            for j in sel:
                N[j] = oracle.normalize(P[j] - vec(b["pos"]))
        albedo[sel] = vec(b["color"])
        ks[sel] = SU.specular_of(b)
    plan = UL.Plan(o, UL.lights_of_text(text), rays, hits, N)
    o.close()
    hit2, t2 = OC.opaque_probe(oracle, path, tmp_path, plan.shadow_rays) if len(plan.shadow_rays) else (np.zeros(0, bool), np.zeros(0, f32))
    sums = plan.reduce(OC.expected(hit2, t2, plan.shadow_tmax), const["n_specular"][np.maximum(obj, 0)])
    res = SC.restate(rays, hits, N, albedo, ks, sums["diffuse"], sums["specular"], const)
    material = np.where(obj >= 0, const["material"][np.maximum(obj, 0)], -1)
    return rays, hits, N, material, res


def probe_colours(oracle, path, rays):
    o = oracle.OracleScene(path, 8, 8)
    _, col = o.probe(rays)
    o.close()
    return col


# tests/util_scatter itself, one level of castRay at a time: the oracle's colour of every ray in the scene at max_ray_depth = M is
# compose() of the restated channels and the oracle's colours of the restated children in the same scene at M - 1 -- for M the file's depth
# (the children recurse), 1 (the grandchildren are sky) and 0 (the children are sky) -- bit for bit over every ray.  Through the Diffuse and
# Phong hits this pins `local` to tests/util_light's sums, through the Reflective and Transparent ones the children, the weights and S.
# What matched when this was written is printed per scene: the classes of hits and their numbers.
@pytest.mark.parametrize("name", SC.EXACT_N)
def test_the_restatement_composes_the_oracles_colours(oracle, family, tmp_path, name):
    path = path_of(name, family)
    w, h = SC.size_of(name)
    o = oracle.OracleScene(path, w, h)
    cam = U.primary_rays(o)
    o.close()
    rays, hits, N, material, res = exact_case(oracle, path, tmp_path, np.concatenate([cam, SC.inside_rays(name)]))
    counts = SC.class_counts(rays, res, hits, N, material)
    kid_rays, parent, is_refract = SC.children(res)
    print("%s %dx%d + %d inside rays: %d rays on planes, spheres and sky, %s, %d children" % (name, w, h, SC.N_INSIDE, len(rays), counts, len(kid_rays)))
    for c in SC.CLAIMS[name]:
        assert counts[c] >= SC.MIN_CLASS, "%s: %d rays of class %s" % (name, counts[c], c)
    M0 = file_depth(text_of(path))
    for M in (M0, 1, 0):
        want = probe_colours(oracle, at_depth(name, family, tmp_path, M), rays)
        kids = probe_colours(oracle, at_depth(name, family, tmp_path, M - 1), kid_rays)
        if M == 0:            # the children are beyond the depth: getSkybox of their directions
            o = oracle.OracleScene(path, 8, 8)
            assert np.array_equal(U.bits(kids), U.bits(o.skybox(kid_rays[:, 3:6])))
            o.close()
        c_reflect, c_refract = SC.spread(kids, parent, is_refract, len(rays))
        got = SC.compose(res["kinds"], res["weight"], res["local"], c_reflect, c_refract)
        bad = (U.bits(got) != U.bits(want)).any(-1)
        assert not bad.any(), "%s, max_ray_depth %d: %d of %d rays whose composed colour is not the oracle's (materials %s)" % (
            name, M, bad.sum(), len(rays), np.unique(material[bad]))


def oracle_channels(path, w, h, cull, rays, const):
    """the restated channels of `rays` from the oracle alone, good enough to classify and to build children: N decoded from the showNormals
    colours (an ulp or two from hitNormal), no light"""
    exp = SU.expected_of(path, w, h, cull, rays)
    N = ((exp["normal_colour"] - f32(0.5)) * f32(2)).astype(f32)
    N[~exp["hit"]] = 0
    z = np.zeros((len(rays), 3), f32)
    res = SC.restate(rays, exp["hits"], N, z, np.zeros(len(rays), f32), z, z, const)
    obj = exp["object_id"]
    material = np.where(obj >= 0, const["material"][np.maximum(obj, 0)], -1)
    return exp["hits"], N, material, res


def oracle_ray_sets(oracle, name, path, cull):
    """[(what, rays, hits, N, material, res)] of the ray sets the GPU tests use on this scene: the camera rays and the rays inside the
    glass sphere where there is one, else the camera rays, their children and their grandchildren"""
    w, h = SC.size_of(name)
    const = SC.constants_of(SU.object_blocks(text_of(path)))
    o = oracle.OracleScene(path, w, h)
    cam = U.primary_rays(o)
    o.close()
    out = []
    if name in SC.GLASS_SPHERE:
        for what, rays in (("camera", cam), ("inside", SC.inside_rays(name))):
            out.append((what, rays) + oracle_channels(path, w, h, cull, rays, const))
    else:
        rays = cam
        for what in ("camera", "children", "grandchildren"):
            out.append((what, rays) + oracle_channels(path, w, h, cull, rays, const))
            rays = SC.children(out[-1][5])[0]
    return out


# The inputs of tests/test_gpu_scatter.py are not vacuous: over the ray sets of a scene together, every class the scene is there for
# (tests/util_scatter.CLAIMS) has at least MIN_CLASS rays, under either culling flag.
@pytest.mark.parametrize("cull", [1, 0])
@pytest.mark.parametrize("name", SC.SCENES)
def test_ray_sets_reach_every_class(oracle, family, name, cull):
    path = path_of(name, family)
    total = {}
    for what, rays, hits, N, material, res in oracle_ray_sets(oracle, name, path, cull):
        counts = SC.class_counts(rays, res, hits, N, material)
        print("%s cull %d, %s (%d rays): %s" % (name, cull, what, len(rays), counts))
        for c, k in counts.items():
            total[c] = total.get(c, 0) + k
    for c in SC.claims(name, cull):
        assert total[c] >= SC.MIN_CLASS, "%s cull %d: %d rays of class %s" % (name, cull, total[c], c)
