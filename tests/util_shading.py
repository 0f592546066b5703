"""The scene family that pins the SHADING DATA path -- texture, normal and specular maps and the skybox -- at the sizes where an index can go
wrong: maps that are not square, not powers of two, as narrow as 4 texels, the three maps of a mesh all different, skybox faces 96 x 40.
Deterministic, no random state: scene files and images are written by write_family() into a directory of the caller's.

Every texel of every image is unique within its map (and the salt in the blue channel tells the maps and faces apart), so a wrong index is a
wrong value wherever the index differs.  Also here: the ray sets of the tests (sky_directions, sky_rays, shading_rays, mirror_rays) and a numpy
restatement of the four index computations (texel, the three map fetches, toPixel and the face table of the sky lookup) with the faults
the tests must be able to see as switches -- tests/test_shading_data_cpu.py proves the restatement against the oracle and then counts, per
fault, the rays whose fetched value changes."""
import functools
import os

import numpy as np

from tests.util_rays import _pcg32, probe_rays

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 128, 96
SKY_W, SKY_H = 96, 40
NAME_LIMIT = 63         # a skybox file name longer than this is cut by every loader (scene.cpp:191 copies 64 bytes, unterminated)


# ---- images -------------------------------------------------------------------------------------------------------------------------
def colour_image(w, h, salt):
    """uint8 [h, w, 3], row 0 = top: R = 255 - x, G = 255 - y, B = salt.  Unique texels for w, h <= 256."""
    assert w <= 256 and h <= 256 and w % 4 == 0
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return np.stack([255 - x, 255 - y, np.full_like(x, salt)], -1).astype(np.uint8)


def normal_image(w, h, salt):
    """A smooth tilt around +z (R, G centred on 128, B = 200 + salt): unique texels, every texel a normal within ~35 degrees of the surface's."""
    assert w <= 128 and h <= 128 and w % 4 == 0 and salt < 56
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return np.stack([128 - w // 2 + x, 128 - h // 2 + y, np.full_like(x, 200 + salt)], -1).astype(np.uint8)


def specular_image(w, h, salt):
    """The loaders keep (R + G + B) / 3 of a specular texel, so the SUM is what has to be unique: sum = 12 + salt + (y * w + x), spread over
    the three channels."""
    assert w * h + 12 + salt <= 765 and w % 4 == 0
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    s = 12 + salt + y * w + x
    r = np.minimum(s, 255); g = np.minimum(s - r, 255); b = s - r - g
    return np.stack([r, g, b], -1).astype(np.uint8)


IMAGE = {"d": colour_image, "n": normal_image, "s": specular_image}


def loaded(img):
    """An image as the loaders keep it: rows in file order (bottom-up), float32 channel / 256."""
    return (img[::-1].astype(f32) / f32(256)).reshape(-1, 3)


def sky_image(k):
    return colour_image(SKY_W, SKY_H, 20 + 40 * k)


# ---- scenes -------------------------------------------------------------------------------------------------------------------------
POINT = "[light]\ntype=point\nposition=2,3,0\ncolor=1,0.9,0.8\nintensity=0.8\n\n"
DISTANT = "[light]\ntype=distant\ndirection=-0.4,-1,-0.3\ncolor=0.6,0.7,1\nintensity=0.3\n\n"
AREA = "[light]\ntype=area\npos=-1,3,-1\ni=1,0,0\nj=0,0,1\nsamples=2\ncolor=1,1,0.9\nintensity=1.5\n\n"
PHONG = "phong,0.3,0.5,0.6,20.0"
# four tori turned to face the camera, their silhouettes meeting in the middle of the frame: (pos, size, rot)
PLACE = {"A": ((-1.5, 1.0, -4.0), 3.6, (70, 10, 0)), "B": ((1.5, 1.0, -4.5), 3.8, (65, 0, -25)),
         "C": ((1.7, -1.1, -4.0), 3.2, (75, 0, 20)), "D": ((-1.1, -1.1, -3.5), 2.7, (60, 0, 20))}


def mesh(slot, material="", obj="torus_1536.obj", **maps):
    """maps: d / n / s = (width, height, salt)"""
    return dict(slot=slot, material=material, obj=obj, maps=maps)


# name -> dict(cam=(pos, rot), depth, lights, sky (bool: useSkybox), meshes | text of the [object] blocks)
FAMILY = {
    # PLAIN: everything Diffuse, point + distant light.  diffuse + specular; diffuse only (W < H); a square map; specular only
    "plain": dict(cam=((0.1, 0.2, 0.5), (-5, 8, 3)), depth=3, lights=POINT + DISTANT, sky=True, meshes=[
        mesh("A", d=(64, 24, 11), s=(12, 52, 13)), mesh("B", d=(8, 124, 14)), mesh("C", d=(36, 36, 15)), mesh("D", s=(4, 52, 16))]),
    # its Phong twin (the specular maps now show), the camera pitched up and rolled: the top face is in the frame
    "phong": dict(cam=((0.1, -0.3, 0.5), (22, -9, -14)), depth=3, lights=POINT + DISTANT, sky=True, meshes=[
        mesh("A", PHONG, d=(64, 24, 11), s=(12, 52, 13)), mesh("B", PHONG, d=(8, 124, 14)), mesh("C", PHONG, d=(36, 36, 15)),
        mesh("D", PHONG, s=(4, 52, 16))]),
    # the same two with normal maps: all three maps in three sizes; normal only (W > H); diffuse only; diffuse + specular
    "plain_nrm": dict(cam=((0.1, 0.2, 0.5), (-5, 8, 3)), depth=3, lights=POINT + DISTANT, sky=True, meshes=[
        mesh("A", d=(64, 24, 11), n=(20, 36, 12), s=(12, 52, 13)), mesh("B", n=(100, 28, 17)), mesh("C", d=(36, 36, 15)),
        mesh("D", d=(4, 100, 18), s=(36, 20, 19))]),
    "phong_nrm": dict(cam=((0.1, 0.2, 0.5), (-5, 8, 3)), depth=3, lights=POINT + DISTANT, sky=True, meshes=[
        mesh("A", PHONG, d=(64, 24, 11), n=(20, 36, 12), s=(12, 52, 13)), mesh("B", PHONG, n=(100, 28, 17)), mesh("C", PHONG, d=(36, 36, 15)),
        mesh("D", PHONG, d=(4, 100, 18), s=(36, 20, 19))]),
    # every material, an area light, recursion: the maps of A, C and D are fetched from inside the mirror B and through the glass D
    "mixed": dict(cam=((-0.2, 0.3, 0.8), (-15, -12, 6)), depth=4, lights=POINT + AREA, sky=True, meshes=[
        mesh("A", d=(64, 24, 11), s=(12, 52, 13)), mesh("B", "reflective", d=(8, 124, 14)), mesh("C", PHONG, d=(28, 100, 21), s=(36, 20, 19)),
        mesh("D", "transparent,1.3", d=(4, 100, 18))]),
    "mixed_nrm": dict(cam=((-0.2, 0.3, 0.8), (-15, -12, 6)), depth=4, lights=POINT + AREA, sky=True, meshes=[
        mesh("A", d=(64, 24, 11), n=(20, 36, 12), s=(12, 52, 13)), mesh("B", "reflective", n=(100, 28, 17)),
        mesh("C", PHONG, d=(28, 100, 21), n=(52, 44, 22), s=(36, 20, 19)), mesh("D", "transparent,1.3", n=(20, 36, 12))]),
    # "plain" with the skybox loaded by name and switched off again
    "plain_nosky": dict(cam=((0.1, 0.2, 0.5), (-5, 8, 3)), depth=3, lights=POINT + DISTANT, sky=False, meshes=[
        mesh("A", d=(64, 24, 11), s=(12, 52, 13)), mesh("B", d=(8, 124, 14)), mesh("C", d=(36, 36, 15)), mesh("D", s=(4, 52, 16))]),
    # texture coordinates in [-0.75, 1.75] x [-0.3, 1.2]: the oracle's definition of the clamps (the reference reads out of bounds)
    "uvwild": dict(cam=((0.1, 0.2, 0.5), (-5, 8, 3)), depth=3, lights=POINT + DISTANT, sky=True, meshes=[
        mesh("A", PHONG, "torus_uvwild.obj", d=(64, 24, 11), n=(20, 36, 12), s=(12, 52, 13)), mesh("B", "reflective", "torus_uvwild.obj", n=(100, 28, 17)),
        mesh("C", "", "torus_uvwild.obj", d=(8, 124, 14)), mesh("D", PHONG, "torus_uvwild.obj", s=(4, 52, 16))]),
    # no mesh: the analytic kernels with non-square faces, the camera turned about all three axes
    "analytic": dict(cam=((0.0, 0.3, 0.5), (18, 25, -12)), depth=4, lights=POINT + DISTANT, sky=True, text=(
        "[object]\ntype=sphere\npos=-0.9,0.3,-3.5\ncolor=1,1,1\nradius=1.0\nmaterial=reflective\n\n"
        "[object]\ntype=sphere\npos=1.1,0.9,-4\ncolor=0.9,0.6,0.3\nradius=0.8\nmaterial=transparent,1.4\n\n"
        "[object]\ntype=plane\npos=0,-1.5,0\nnormal=0,1,0\ncolor=0.7,0.8,0.7\n\n")),
}
NORMAL_MAPPED = [n for n, s in FAMILY.items() if any("n" in m["maps"] for m in s.get("meshes", []))]
UV_WILD = ["uvwild"]
# what can be pinned to the reference bit for bit: uv inside [0,1] and no normal map
REFERENCE_EXACT = [n for n in FAMILY if n not in NORMAL_MAPPED and n not in UV_WILD]


def map_name(kind, spec):
    return "%s%dx%d_%d.bmp" % (kind, spec[0], spec[1], spec[2])


def object_text(m, dst, place=None):
    pos, size, rot = place or PLACE[m["slot"]]
    s = "[object]\ntype=mesh\npos=%s\nsize=%s\nrot=%s\ncolor=0.9,0.8,0.7\n" % (
        ",".join("%g" % x for x in pos), ",".join(["%g" % size] * 3), ",".join("%g" % x for x in rot))
    if m["material"]:
        s += "material=%s\n" % m["material"]
    s += "name=scenes/assets/%s\n" % m["obj"]
    for kind, key in (("d", "diffuse_map"), ("n", "normal_map"), ("s", "specular_map")):
        if kind in m["maps"]:
            s += "%s=%s\n" % (key, os.path.join(dst, map_name(kind, m["maps"][kind])))
    return s + "\n"


def scene_text(name, dst, extra=None, places=None):
    """The text of scene `name` with its images under dst; extra: options appended (they win); places: {slot: (pos, size, rot)} overrides."""
    sp = FAMILY[name]
    pos, rot = sp["cam"]
    s = "[options]\nwidth=%d\nheight=%d\nfov=75\nposition=%s\nrotation=%s\nmax_ray_depth=%d\nac_penalty=2\nbackground_color=0.2,0.3,0.4\nimage_name=output/shading\n" % (
        W, H, ",".join("%g" % x for x in pos), ",".join("%g" % x for x in rot), sp["depth"])
    s += "skyboxes=%s\n" % ",".join(os.path.join(dst, "k%d.bmp" % k) for k in range(6))
    if not sp["sky"]:
        s += "useSkybox=0\n"
    for kv in (extra or {}).items():
        s += "%s=%s\n" % kv
    s += "\n" + sp["lights"]
    if "text" in sp:
        s += sp["text"]
    else:
        for m in sp["meshes"]:
            s += object_text(m, dst, (places or {}).get(m["slot"]))
    return s + "[end]\n"


def write_images(dst):
    dst = str(dst)
    assert fits(dst), "skybox file names under %s would be longer than %d characters" % (dst, NAME_LIMIT)
    from rendering_amd import assets
    assets.ensure(["torus_1536.obj", "torus_uvwild.obj"])
    for k in range(6):
        with open(os.path.join(dst, "k%d.bmp" % k), "wb") as f:
            f.write(assets.bmp24(sky_image(k)))
    for sp in FAMILY.values():
        for m in sp.get("meshes", []):
            for kind, spec in m["maps"].items():
                with open(os.path.join(dst, map_name(kind, spec)), "wb") as f:
                    f.write(assets.bmp24(IMAGE[kind](*spec)))


def write_family(dst):
    """Writes every image and scene of the family into dst; returns {name: path of the scene file}."""
    dst = str(dst)
    write_images(dst)
    out = {}
    for name in FAMILY:
        out[name] = os.path.join(dst, name + ".scene")
        with open(out[name], "w") as f:
            f.write(scene_text(name, dst))
    return out


NAME_ROOM = 16          # the longest file name written here ("r31_k5.bmp", "d64x24_11.bmp": maps have no limit) fits in it


def fits(d):
    return len(os.path.join(d, "x" * NAME_ROOM)) <= NAME_LIMIT


def short_dir(tmp_path_factory):
    """A fresh directory whose skybox file names fit NAME_LIMIT wherever the temporary directories of this user and machine happen to be:
    pytest's, else one straight under the system's temporary directory, under /tmp or /dev/shm, else one under the repository's output/ named
    relative to the repository root (every loader here is given that root as its working directory).  What is made outside pytest's
    directory is removed when the process ends."""
    import atexit
    import shutil
    import tempfile
    d = str(tmp_path_factory.mktemp("sh"))
    if fits(d):
        return d
    for parent in (None, "/tmp", "/dev/shm"):
        if parent is not None and not (os.path.isdir(parent) and os.access(parent, os.W_OK)):
            continue
        d = tempfile.mkdtemp(prefix="sh", dir=parent)
        atexit.register(shutil.rmtree, d, True)
        if fits(d):
            return d
    os.makedirs(os.path.join(ROOT, "output"), exist_ok=True)
    d = tempfile.mkdtemp(prefix="sh", dir=os.path.join(ROOT, "output"))
    atexit.register(shutil.rmtree, d, True)
    d = os.path.relpath(d, ROOT)
    assert fits(d) and os.path.samefile(os.getcwd(), ROOT), "no directory short enough for skybox file names (%s)" % d
    return d


# ---- rays ---------------------------------------------------------------------------------------------------------------------------
def _ulp(x, up):
    return np.nextafter(f32(x), f32(np.inf) if up else f32(-np.inf))


def sky_directions():
    """n x 3 float32 directions for the sky lookup, none zero or non-finite: the 26 sign patterns of {-1,0,1}^3 as they are and normalised (axes
    included), axes with -0.0 in the other components, for each pair of axes two equal largest components and their neighbours one ulp to either
    side (every sign), and for each face and each of its two image axes the projected coordinate at +-1 (toPixel's clamp at the last texel, the
    first texel) and one ulp inside."""
    d = []
    for x in (-1, 0, 1):
        for y in (-1, 0, 1):
            for z in (-1, 0, 1):
                if (x, y, z) != (0, 0, 0):
                    v = np.array([x, y, z], f32)
                    d += [v, v / f32(np.sqrt(f32(x * x + y * y + z * z)))]
    for ax in range(3):
        for sgn in (1, -1):
            v = np.array([-0.0, -0.0, -0.0], f32); v[ax] = sgn
            d.append(v)
            v = np.array([0.0, -0.0, 0.0], f32) if ax != 1 else np.array([-0.0, 0.0, 0.0], f32); v[ax] = sgn
            d.append(v)
    big, small = f32(0.7), f32(0.3)
    for a, b in ((0, 2), (0, 1), (1, 2)):
        c = 3 - a - b
        for sa in (1, -1):
            for sb in (1, -1):
                for va in (big, _ulp(big, True), _ulp(big, False)):
                    v = np.zeros(3, f32); v[a] = sa * va; v[b] = sb * big; v[c] = small
                    d.append(v)
    one = f32(1)
    for m in range(3):
        for sm in (1, -1):
            for o in range(3):
                if o == m:
                    continue
                t = 3 - m - o
                for val in (one, -one, _ulp(one, False), -_ulp(one, False)):
                    v = np.zeros(3, f32); v[m] = sm; v[o] = val; v[t] = f32(-0.25)
                    d.append(v)
    d = np.stack(d).astype(f32)
    assert np.isfinite(d).all() and (np.abs(d).max(1) > 0).all()
    return d


SKY_ORIGIN = (40.0, 30.0, 20.0)        # outside every object of every scene of the family, the tori far off every special direction


def sky_rays(origin=SKY_ORIGIN):
    d = sky_directions()
    return np.concatenate([np.tile(np.array([origin], f32), (len(d), 1)), d], 1).astype(f32)


def sphere_directions(n):
    """n directions spread evenly over the sphere (a Fibonacci lattice), float32, normalised in float64."""
    i = np.arange(n, dtype=np.float64) + 0.5
    z = 1 - 2 * i / n
    phi = i * np.pi * (3 - np.sqrt(5.0))
    r = np.sqrt(1 - z * z)
    return np.stack([r * np.cos(phi), z, r * np.sin(phi)], 1).astype(f32)


@functools.lru_cache(maxsize=None)
def _shading_rays(n):
    rays = probe_rays(n).copy()
    k = len(rays[1::3])
    rays[1::3, 3:6] = sphere_directions(k)
    return rays


def shading_rays(n=2048):
    """probe_rays(n) re-aimed: every third ray keeps its origin near the camera and takes a direction of a lattice over the whole sphere,
    so that all six faces are met.  (Generated once per n: the generator is a Python loop.)"""
    return _shading_rays(n).copy()


@functools.lru_cache(maxsize=None)
def _mirror_rays(slot, n):
    pos, size, _ = PLACE[slot]
    u = (_pcg32(n * 2, seed=0xB0B).astype(np.float64) / 2**32).reshape(n, 2)
    tgt = np.array(pos) + np.stack([(u[:, 0] - 0.5) * size, (u[:, 1] - 0.5) * size, np.zeros(n)], 1)
    org = np.array(pos) + np.array([0.3, 0.2, 3.0])
    dirs = tgt - org
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    return np.concatenate([np.tile(org, (n, 1)), dirs], 1).astype(f32)


def mirror_rays(slot="B", n=512):
    """Rays from a point in front of the reflective torus (slot B of the mixed scenes) aimed at a square around it: the sky arrives through one
    bounce."""
    return _mirror_rays(slot, n).copy()


def primary_rays(o):
    """The primary rays of an OracleScene's frame, one per pixel centre (tests/ac_heatmap.rays).  They say WHERE a frame looks: every value
    compared by the tests is computed from the very ray that was cast."""
    from tests import ac_heatmap as A
    scale, aspect, m, pos = o.camera()
    org, d = A.rays(scale, aspect, m, pos, o.width, o.height)
    return np.concatenate([org, d], 1).astype(f32)


# ---- the index arithmetic, restated -----------------------------------------------------------------------------------------------------
def texel(dim, coord):
    """objects.cpp:144-147 with the oracle's definition outside [0, dim): (int)(dim * coord) in float32, negative or NaN -> 0, too large -> dim - 1."""
    f = f32(dim) * np.asarray(coord, f32)
    with np.errstate(invalid="ignore"):
        return np.where(f >= f32(dim), dim - 1, np.where(~(f >= 0), 0, np.trunc(np.where(np.isfinite(f), f, 0)))).astype(np.int64)


def tex_coords(tris, tri, u, v):
    """Mesh::getSurfaceData's texture coordinate (objects.cpp:121-131) of hits (triangle index, u, v), float32 in the reference's order."""
    t = tris[tri]
    ta, tb, tc = t[:, 18:20], t[:, 20:22], t[:, 22:24]
    u = u.astype(f32); v = v.astype(f32)
    w = f32(1) - u - v
    return (tb[:, 0] * u + tc[:, 0] * v) + ta[:, 0] * w, (tb[:, 1] * u + tc[:, 1] * v) + ta[:, 1] * w


def map_index(size, tx, ty, fault=None, other=None):
    """Flat index of the texel a map of size (w, h) returns for (tx, ty).  fault: None, "wh" (width and height exchanged in the texel computation),
    "stride" (the row stride taken from the height), "other" (another map's size, `other`, used throughout).  A faulty index may lie outside
    the map; since texels are unique the fetched value changes exactly where the index does."""
    w, h = other if fault == "other" else size
    if fault == "wh":
        return texel(w, ty) * w + texel(h, tx)
    if fault == "stride":
        return texel(h, ty) * h + texel(w, tx)
    return texel(h, ty) * w + texel(w, tx)


def to_pixel(v, mx):
    """scene.cpp:387-392: (int)((v + 1) / 2 * mx), clamped at mx - 1."""
    val = np.trunc((np.asarray(v, f32) + f32(1)) / f32(2) * f32(mx)).astype(np.int64)
    return np.minimum(val, mx - 1)


def sky_index(d, w=SKY_W, h=SKY_H, fault=None):
    """(face, flat index) the sky lookup returns for directions d [n, 3] (scene.cpp:394-441): the largest |component| chooses the face, z before
    x before y on ties.  fault: None, "wh" (face 1 indexed with width and height exchanged), "ij" (row and column exchanged on the top face),
    "faces" (faces 4 and 5 exchanged), "tie" (x before z on ties)."""
    d = np.asarray(d, f32).reshape(-1, 3)
    ax, ay, az = np.abs(d[:, 0]), np.abs(d[:, 1]), np.abs(d[:, 2])
    mx = np.maximum(ax, np.maximum(ay, az))
    isz, isx = mx == az, mx == ax
    if fault == "tie":
        isz = isz & ~isx
    else:
        isx = isx & ~isz
    isy = ~(isz | isx)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = np.where(isz, f32(1) / az, np.where(isx, f32(1) / ax, f32(1) / ay)).astype(f32)
    a = d * inv[:, None]
    neg = np.where(isz, d[:, 2] < 0, np.where(isx, d[:, 0] < 0, d[:, 1] < 0))
    face = np.where(isz, np.where(neg, 1, 3), np.where(isx, np.where(neg, 0, 2), np.where(neg, 5, 4)))
    row = np.where(isy, a[:, 2], a[:, 1])
    col = np.where(isz, np.where(neg, a[:, 0], -a[:, 0]), np.where(isx, np.where(neg, -a[:, 2], a[:, 2]), a[:, 0]))
    i, j = to_pixel(row, h), to_pixel(col, w)
    if fault == "wh":
        i1, j1 = to_pixel(row, w), to_pixel(col, h)
        i, j = np.where(face == 1, i1, i), np.where(face == 1, j1, j)
    if fault == "ij":
        i, j = np.where(face == 4, j, i), np.where(face == 4, i, j)
    if fault == "faces":
        face = np.where(face == 4, 5, np.where(face == 5, 4, face))
    return face, i * w + j


def sky_colour(d, faces=None, fault=None):
    """The colour the sky lookup returns: float32 [n, 3]; a faulty index outside the face gives NaN."""
    faces = faces if faces is not None else [loaded(sky_image(k)) for k in range(6)]
    face, idx = sky_index(d, fault=fault)
    table = np.stack(faces)
    ok = (idx >= 0) & (idx < table.shape[1])
    out = table[face, np.where(ok, idx, 0)]
    out[~ok] = np.nan
    return out


# ---- what a scene computes: the same calls on the reference's harness and on the oracle -----------------------------------------------------
MIRROR_SCENES = ("mixed", "mixed_nrm", "uvwild")
GOLDEN_RAYS = 2048


def results(s, name):
    """Everything the goldens keep of scene `name`, from s = tools.ref_harness.RefScene or oracle.OracleScene (same methods)."""
    out = {}
    out["pass1"] = s.pass1()
    out["ssaa"] = s.ssaa(out["pass1"])            # row 0 / column 0: the reference's uninitialised Sobel border, masked by same_results
    out["probe_hits"], out["probe_colours"] = s.probe(shading_rays(GOLDEN_RAYS))
    out["sky_ray_hits"], out["sky_ray_colours"] = s.probe(sky_rays())
    out["sky_colours"] = s.skybox(sky_directions())
    if name in MIRROR_SCENES:
        out["mirror_hits"], out["mirror_colours"] = s.probe(mirror_rays())
    return out


def differences(got, want, ulp=0):
    """{key: number of pixels / rays that differ by more than ulp} over the keys of `want` that are results; empty = equal."""
    from tests.util_ulp import ulp_diff
    bad = {}
    for k in ("pass1", "ssaa", "probe_hits", "probe_colours", "sky_ray_hits", "sky_ray_colours", "sky_colours", "mirror_hits", "mirror_colours"):
        if k not in want:
            continue
        d = ulp_diff(got[k], want[k]) > ulp
        if k == "ssaa":
            d[0, :] = False; d[:, 0] = False
        if d.any():
            bad[k] = int(d.sum())
    return bad


def pack(res):
    """results() as stored: the 4-sample frame as the pixels where it differs from pass 1, the hit records as their columns in use."""
    out = dict(res)
    p1, ss = out["pass1"], out.pop("ssaa")
    idx = np.nonzero((p1.view(np.uint32) != ss.view(np.uint32)).any(-1).ravel())[0].astype(np.int32)
    out["ssaa_index"] = idx; out["ssaa_value"] = ss.reshape(-1, 3)[idx]
    for k in [k for k in out if k.endswith("_hits")]:
        out[k] = out[k][:, :6].copy()
    return out


def unpack(g):
    out = {k: g[k] for k in g.files if k not in ("ssaa_index", "ssaa_value", "assets_md5")}
    ss = out["pass1"].copy()
    ss.reshape(-1, 3)[g["ssaa_index"]] = g["ssaa_value"]
    out["ssaa"] = ss
    for k in [k for k in out if k.endswith("_hits")]:
        out[k] = np.concatenate([out[k], np.zeros((len(out[k]), 2), f32)], 1)
    return out


def golden_file(name, kind="shading"):
    return os.path.join(ROOT, "tests", "golden", "%s__%s.npz" % (kind, name))


# ---- random scenes with maps and skyboxes ---------------------------------------------------------------------------------------------------
RANDOM_SEEDS = list(range(32))


def random_has_normal_map(seed):
    """Seeds 0, 1 mod 4 carry no normal map and only meshes with uv inside [0,1]: those are pinned to the reference as well."""
    return seed % 4 >= 2


def make_shading_scene(seed, w, h, dst):
    """A random scene in the manner of tests/test_gpu_fuzz.make_scene (a generator of its own: that one's seeds are pinned to the reference as they
    are) whose meshes carry a random subset of maps of random non-square sizes; the skybox is on in the odd seeds.  Writes its images into dst
    and returns the scene text."""
    import random
    from rendering_amd import assets
    r = random.Random(0x5AD1 + seed)
    v3 = lambda lo, hi: ",".join("%.3f" % r.uniform(lo, hi) for _ in range(3))
    nrm = random_has_normal_map(seed)

    def material():
        k = r.randrange(5)
        return ["", "material=reflective\n", "material=transparent,%.2f\n" % r.uniform(1.05, 1.8)][k] if k < 3 else \
            "material=phong,%.2f,%.2f,%.2f,%.1f\n" % (r.uniform(0, 0.5), r.uniform(0, 1), r.uniform(0, 1), r.choice([1, 2, 5, 10, 20, 64]))

    s = "[options]\nwidth=%d\nheight=%d\nfov=%d\nposition=%s\nrotation=%s\nmax_ray_depth=%d\nac_penalty=%d\nuseBackfaceCulling=%d\nbackground_color=%s\nimage_name=output/fuzz\n" % (
        w, h, r.choice([60, 75, 90]), v3(-0.4, 0.4), v3(-14, 14), r.randrange(1, 5), r.choice([1, 2, 3]), r.randrange(2), v3(0, 0.6))
    if seed % 2:
        kw, kh = r.choice([(8, 20), (44, 12), (96, 40), (12, 12), (4, 64)])
        names = []
        for k in range(6):
            names.append(os.path.join(dst, "r%d_k%d.bmp" % (seed, k)))
            assert len(names[-1]) <= NAME_LIMIT, names[-1]
            with open(names[-1], "wb") as f:
                f.write(assets.bmp24(colour_image(kw, kh, 20 + 40 * k)))
        s += "skyboxes=%s\n" % ",".join(names)
    s += "\n"
    for _ in range(r.randrange(1, 3)):
        t = r.choice(["point", "distant", "area"])
        if t == "point":
            s += "[light]\ntype=point\nposition=%s\ncolor=%s\nintensity=%.2f\n\n" % (v3(-3, 3), v3(0.3, 1), r.uniform(0.3, 2))
        elif t == "distant":
            s += "[light]\ntype=distant\ndirection=%s\ncolor=%s\nintensity=%.2f\n\n" % (v3(-1, 1), v3(0.3, 1), r.uniform(0.2, 1))
        else:
            s += "[light]\ntype=area\npos=%s\ni=%s\nj=%s\nsamples=%d\ncolor=%s\nintensity=%.2f\n\n" % (v3(-3, 3), v3(-1, 1), v3(-1, 1), r.randrange(1, 3), v3(0.3, 1), r.uniform(0.5, 3))
    n_mesh = r.randrange(2, 4)
    for k in range(n_mesh + r.randrange(0, 2)):
        if k >= n_mesh:
            s += "[object]\ntype=sphere\npos=%.3f,%.3f,%.3f\ncolor=%s\nradius=%.2f\n%s\n" % (r.uniform(-2, 2), r.uniform(-1.5, 1.5), r.uniform(-6, -3), v3(0.1, 1), r.uniform(0.3, 1.0), material())
            continue
        obj = r.choice(["torus_1536.obj", "torus_uvwild.obj"]) if nrm else "torus_1536.obj"
        s += "[object]\ntype=mesh\npos=%.3f,%.3f,%.3f\nsize=%s\nrot=%s\ncolor=%s\n%sname=scenes/assets/%s\n" % (
            r.uniform(-1.6, 1.6), r.uniform(-1.1, 1.1), r.uniform(-4.6, -3.0), v3(2.0, 3.6), v3(-80, 80), v3(0.4, 1), material(), obj)
        kinds = r.choice([("d", "n", "s"), ("d",), ("n",), ("s",), ("d", "s"), ("d", "n")])
        for kind, key in (("d", "diffuse_map"), ("n", "normal_map"), ("s", "specular_map")):
            if kind not in kinds or (kind == "n" and not nrm):
                continue
            mw = r.choice([4, 8, 12, 20, 36, 64, 100])
            mh = r.choice([x for x in ([3, 5, 9, 17, 33, 60] if kind == "s" else [3, 5, 24, 52, 77, 124]) if x != mw and (kind != "s" or mw * x <= 700)])
            name = os.path.join(dst, "r%d_%d%s.bmp" % (seed, k, kind))
            with open(name, "wb") as f:
                f.write(assets.bmp24(IMAGE[kind](mw, mh, 10 + 5 * k)))
            s += "%s=%s\n" % (key, name)
        s += "\n"
    return s + "[end]\n"


def random_size(seed):
    """Half the frame of the family's scenes: what a seed costs is the oracle's CPU render of it, and a mesh is still hundreds of pixels."""
    return 64 + 8 * (seed % 3), 48 + 4 * (seed % 5)
