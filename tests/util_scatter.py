"""What rtx_scatter_rays / Scene.scatter_rays must write (include/rtx_scatter.h), restated in numpy float32 in the order of the contract, from
what other tests already pin: the hit records, the exact N, albedo and ks (tests/util_surface; Scene.surface_rays on the GPU), the sums D
and S over the lights (tests/util_light; Scene.light_rays on the GPU) and the objects' constants from the scene file's text
(Scene.device_objects() on the GPU).  reflect, refract, fresnel and normalize are the oracle's, one call per ray: no expression of them is
written again here.  compose() is the contract's three identities.  Also the scenes, sizes and ray sets of the tests."""
import functools

import numpy as np

from tests import util_light as UL
from tests.util_aov import bits

f32 = np.float32
BIAS = UL.BIAS
CHANNELS = ("hits", "local", "reflect", "refract", "weight", "kinds")
SCATTER = CHANNELS[1:]
TAIL = {"hits": (8,), "local": (3,), "reflect": (6,), "refract": (6,), "weight": (2,), "kinds": ()}
DIFFUSE, REFLECTIVE, TRANSPARENT, PHONG = 0, 1, 2, 3
MATERIALS = {"": DIFFUSE, "diffuse": DIFFUSE, "reflective": REFLECTIVE, "transparent": TRANSPARENT, "phong": PHONG}
MIRROR_WEIGHT = f32(0.8)              # scene.cpp:858
# Object's defaults (objects.h): what a material= line that does not set them leaves
DEFAULT_IOR, DEFAULT_AMBIENT, DEFAULT_KD = f32(1.0), f32(0.1), f32(0.1)

# the scenes of the GPU tests: repository scenes, then scenes of tests/util_shading.FAMILY
REPO = ["cfg1_simple_shapes", "cfg3_reflective_refractive", "area_light", "mixed_materials"]
FAMILY = ["mixed", "mixed_nrm", "uvwild", "analytic"]
SCENES = REPO + FAMILY
# where every object is a plane or a sphere but for area_light's one mesh: N is known exactly without a GPU (tests/test_scatter_cpu.py)
EXACT_N = ["cfg1_simple_shapes", "cfg3_reflective_refractive", "area_light", "analytic"]
# the glass sphere the inside rays start in: (centre, the cube's half-width -- inside the sphere, whose radius is at least 1.73 times it)
GLASS_SPHERE = {"cfg1_simple_shapes": ((-1.0, 0.75, -2.0), 0.16), "cfg3_reflective_refractive": ((-1.75, 0.75, -4.0), 0.8),
                "area_light": ((0.2, -0.4, -2.2), 0.24), "analytic": ((1.1, 0.9, -4.0), 0.44)}
# (about one such ray in a hundred is totally reflected at ior 1.33, two at 1.4: enough of them for MIN_CLASS several times over at 1.4)
N_INSIDE = 3072
# the classes a scene is there for, each with at least MIN_CLASS rays among all its ray sets together (tests/test_scatter_cpu.py shows it on
# the oracle): miss, dp (Diffuse or Phong hits), mirror, glass_out / glass_in (Transparent from outside / inside with both children),
# tir (Transparent, total internal reflection)
MIN_CLASS = 16
CLAIMS = {
    "cfg1_simple_shapes": ("miss", "dp", "mirror", "glass_out", "glass_in", "tir"),
    "cfg3_reflective_refractive": ("miss", "mirror", "glass_out", "glass_in", "tir"),
    "area_light": ("miss", "dp", "mirror", "glass_out", "glass_in", "tir"),
    "analytic": ("miss", "dp", "mirror", "glass_out", "glass_in", "tir"),
    "mixed_materials": ("miss", "dp", "glass_out", "glass_in"),          # (its mirror, the torus, is met by a handful of these rays only)
    "mixed": ("miss", "dp", "mirror", "glass_out", "glass_in"),
    "mixed_nrm": ("miss", "dp", "mirror", "glass_out", "glass_in"),
    "uvwild": ("miss", "dp", "mirror"),
}


def claims(name, cull):
    """CLAIMS[name] under a culling flag: with culling on no ray meets a glass mesh from inside (the spheres are not culled)"""
    return tuple(c for c in CLAIMS[name] if not (cull and c == "glass_in" and name not in GLASS_SPHERE))


def size_of(name):
    return (40, 24) if name in ("mixed", "mixed_nrm", "uvwild") else (48, 32)


def material_of(block):
    return MATERIALS[block.get("material", "").split(",")[0]]


def constants_of(blocks):
    """Per object of a scene file's [object] blocks: material, ambient, kd, ior, n_specular as the loader leaves them (numpy arrays)."""
    n = len(blocks)
    out = dict(material=np.zeros(n, np.int32), ambient=np.full(n, DEFAULT_AMBIENT, f32), diffuse=np.full(n, DEFAULT_KD, f32),
               ior=np.full(n, DEFAULT_IOR, f32), n_specular=np.full(n, UL.DEFAULT_N_SPECULAR, f32))
    for k, b in enumerate(blocks):
        m = b.get("material", "").split(",")
        out["material"][k] = material_of(b)
        if m[0] == "phong":
            out["ambient"][k], out["diffuse"][k], out["n_specular"][k] = f32(float(m[1])), f32(float(m[2])), f32(float(m[4]))
        if m[0] == "transparent":
            out["ior"][k] = f32(float(m[1]))
    return out


@functools.lru_cache(maxsize=None)
def _inside_rays(centre, half, n):
    rng = np.random.default_rng(0x5CA7)
    org = np.array(centre, np.float64) + rng.uniform(-half, half, (n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([org, d], 1).astype(f32)


def inside_rays(name, n=N_INSIDE):
    """n seeded rays that start inside the scene's glass sphere: origins uniform in a cube around its centre, directions uniform"""
    centre, half = GLASS_SPHERE[name]
    return _inside_rays(tuple(centre), half, n).copy()


def restate(rays, hits, N, albedo, ks, D, S, const, bias=BIAS):
    """The five scatter channels of the contract's step 3.  rays n x 6; hits n x 8 (rtx_trace_rays' records); N, albedo (at a miss the sky
    colour of the direction), D, S n x 3; ks n; const: per object (indexed by hits[:, 1]) material, ambient, diffuse, ior."""
    from oracle import oracle as O
    rays = np.ascontiguousarray(rays, f32); hits = np.asarray(hits, f32)
    N = np.asarray(N, f32); albedo = np.asarray(albedo, f32); D = np.asarray(D, f32); S = np.asarray(S, f32); ks = np.asarray(ks, f32)
    n = len(rays)
    hit = hits[:, 0] > 0
    obj = np.maximum(hits[:, 1].astype(np.int32), 0)
    mat = np.where(hit, const["material"][obj], -1)
    o, d = rays[:, 0:3], rays[:, 3:6]
    with np.errstate(all="ignore"):
        P = (o + d * hits[:, 3:4]).astype(f32)
        B = (N * f32(bias)).astype(f32)
        _, dp = UL.colour_identities(None, albedo, ks, D, S, mat, const["ambient"][obj], const["diffuse"][obj])
    local = albedo.copy()                                  # a miss: getSkybox(d)
    sel = (mat == DIFFUSE) | (mat == PHONG)
    local[sel] = dp[sel]
    reflect = np.zeros((n, 6), f32); refract = np.zeros((n, 6), f32); weight = np.zeros((n, 2), f32); kinds = np.zeros(n, np.uint8)
    with np.errstate(all="ignore"):
        for j in np.nonzero(mat == REFLECTIVE)[0]:
            local[j] = S[j]
            reflect[j, 0:3] = P[j] + B[j]
            reflect[j, 3:6] = O.reflect(d[j], N[j])
            weight[j, 0] = MIRROR_WEIGHT
            kinds[j] = 1
        for j in np.nonzero(mat == TRANSPARENT)[0]:
            ior = float(const["ior"][obj[j]])
            kr = f32(O.fresnel(d[j], N[j], ior))
            outside = UL.dot(d[j], N[j]) < 0
            local[j] = S[j] * kr
            reflect[j, 0:3] = P[j] + B[j] if outside else P[j] - B[j]
            reflect[j, 3:6] = O.normalize(O.reflect(d[j], N[j]))
            weight[j, 0] = kr
            kinds[j] = 1
            if kr < 1:
                refract[j, 0:3] = P[j] - B[j] if outside else P[j] + B[j]
                refract[j, 3:6] = O.normalize(O.refract(d[j], N[j], ior))
                weight[j, 1] = f32(1) - kr
                kinds[j] = 3
    return dict(local=local, reflect=reflect, refract=refract, weight=weight, kinds=kinds)


def compose(kinds, weight, local, c_reflect, c_refract):
    """castRay's colour from the channels of a ray and the colours of its children (rows of rays without that child are not read): the three
    identities of include/rtx_scatter.h, as written there.  A mirror is told from glass in total internal reflection -- both have kinds
    1 -- by the weight the contract gives it."""
    kinds = np.asarray(kinds); weight = np.asarray(weight, f32); local = np.asarray(local, f32)
    out = local.copy()                                     # kinds == 0: local itself
    mirror = (kinds == 1) & (bits(weight[:, 0]) == bits(MIRROR_WEIGHT)) & (bits(weight[:, 1]) == 0)
    with np.errstate(all="ignore"):
        m = (c_reflect * MIRROR_WEIGHT + local).astype(f32)
        acc = np.zeros(local.shape, f32)
        acc = np.where(((kinds & 2) != 0)[:, None], (acc + c_refract * weight[:, 1:2]).astype(f32), acc)
        g = ((acc + c_reflect * weight[:, 0:1]).astype(f32) + local).astype(f32)
    out = np.where(((kinds & 1) != 0)[:, None], g, out)
    return np.where(mirror[:, None], m, out).astype(f32)


def children(res):
    """(rays of the children m x 6, parent index m, is the refraction ray m): per parent the refraction ray, then the reflection ray"""
    n = len(res["kinds"])
    both = np.stack([res["refract"], res["reflect"]], 1).reshape(2 * n, 6)
    exists = np.stack([(res["kinds"] & 2) != 0, (res["kinds"] & 1) != 0], 1).reshape(2 * n)
    at = np.nonzero(exists)[0]
    return np.ascontiguousarray(both[at], f32), at // 2, (at % 2) == 0


def spread(colours, parent, is_refract, n):
    """(c_reflect, c_refract) n x 3 from the colours of children()'s rays; +0 where there is no such child"""
    c_reflect = np.zeros((n, 3), f32); c_refract = np.zeros((n, 3), f32)
    c_refract[parent[is_refract]] = colours[is_refract]
    c_reflect[parent[~is_refract]] = colours[~is_refract]
    return c_reflect, c_refract


def class_counts(rays, res, hits, N, material):
    """{class: number of rays} of the classes of CLAIMS, from the restated channels `res` and per-ray material (-1: a miss)"""
    hit = np.asarray(hits)[:, 0] > 0
    with np.errstate(all="ignore"):
        outside = UL.dot(np.asarray(rays, f32)[:, 3:6], np.asarray(N, f32)) < 0
    glass = material == TRANSPARENT
    return dict(miss=int((~hit).sum()), dp=int(((material == DIFFUSE) | (material == PHONG)).sum()), mirror=int((material == REFLECTIVE).sum()),
                glass_out=int((glass & outside & (res["kinds"] == 3)).sum()), glass_in=int((glass & ~outside & (res["kinds"] == 3)).sum()),
                tir=int((glass & (res["kinds"] == 1)).sum()))


def same(a, b, channels=CHANNELS):
    """names of the channels whose bits differ between two results, over every ray"""
    return [c for c in channels if a[c].shape != b[c].shape or not np.array_equal(bits(a[c]), bits(b[c]))]
