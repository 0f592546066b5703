"""What the texture-edit tests share (tests/test_texture_edit_cpu.py, tests/test_gpu_texture_edit.py): the numpy restatement of the loaders'
texel arithmetic, and for every scene of tests/util_shading.py's family a second set of images -- set B: every map and the skybox at another
size, non-square, other salts -- with the scene files that name them.  Expected values never come from the code under test: a map's
expected texels are the restatement's or the host decode's of the image, a frame's those of a fresh Scene loaded from a file whose BMP files hold
the new images."""
import os

import numpy as np

from tests import util_shading as S

f32 = np.float32
KINDS = {"d": "diffuse", "n": "normal", "s": "specular"}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def restated(kind, rgb8):
    """The loaders' arithmetic in float32 steps, in their order (objects.cpp:395-446, scene.cpp:292-311): uint8 (..., 3) -> float32 (..., 3), (...) for
    "specular".  The normalisation goes through the reference's fp64 factor."""
    c = np.asarray(rgb8, np.uint8).astype(f32) / f32(256)
    if kind in ("diffuse", "sky"):
        return c
    if kind == "specular":
        return ((c[..., 0] + c[..., 1]) + c[..., 2]) / f32(3)
    assert kind == "normal"
    x = c[..., 0] * f32(2) - f32(1)
    y = -(c[..., 1] * f32(2) - f32(1))      # (g == 128: -(+0) = -0)
    z = c[..., 2]
    l2 = (x * x + y * y) + z * z
    with np.errstate(divide="ignore"):
        f = np.where(l2 > 0, f32(1.0) / np.sqrt(l2.astype(np.float64)), 1.0).astype(f32)
    v = np.stack([x, y, z], -1)
    return np.where((l2 > 0)[..., None], v * f[..., None], v).astype(f32)


def all_triples(chunk, chunks=16):
    """Chunk `chunk` of the 2^24 byte triples, uint8 (1024, 1024, 3): r the high byte, b the low one."""
    n = (1 << 24) // chunks
    assert n == 1024 * 1024
    i = np.arange(chunk * n, (chunk + 1) * n, dtype=np.uint32)
    return np.stack([(i >> 16) & 255, (i >> 8) & 255, i & 255], -1).astype(np.uint8).reshape(1024, 1024, 3)


# ---- set B --------------------------------------------------------------------------------------------------------------------------
def spec_b(kind, spec):
    """The size and salt of set B's image for a map of set A: another size, non-square, within what the image generators take."""
    w, h, salt = spec
    if kind == "s":
        return (w + 4, h // 2 + 4, salt + 3)
    return (w + 4, h + 3, salt + 1)


SKY_B = (S.SKY_W + 8, S.SKY_H - 7)


def sky_image_b(k):
    return S.colour_image(SKY_B[0], SKY_B[1], 25 + 40 * k)


def image_b(kind, spec):
    """Set B's image (uint8 [h, w, 3], row 0 = top, as a BMP is written) for the map `spec` of set A."""
    return S.IMAGE[kind](*spec_b(kind, spec))


def family_b(name):
    """Scene `name` of the family with every map replaced by set B's."""
    sp = dict(S.FAMILY[name])
    if "meshes" in sp:
        sp["meshes"] = [dict(m, maps={k: spec_b(k, v) for k, v in m["maps"].items()}) for m in sp["meshes"]]
    return sp


def scene_text(sp, dst, sky_prefix="k", places=None, extra=None):
    """util_shading.scene_text for a scene given as its dict (family_b, or one with maps added or removed); sky_prefix: the skybox files' names."""
    pos, rot = sp["cam"]
    s = "[options]\nwidth=%d\nheight=%d\nfov=75\nposition=%s\nrotation=%s\nmax_ray_depth=%d\nac_penalty=2\nbackground_color=0.2,0.3,0.4\nimage_name=output/shading\n" % (
        S.W, S.H, ",".join("%g" % x for x in pos), ",".join("%g" % x for x in rot), sp["depth"])
    s += "skyboxes=%s\n" % ",".join(os.path.join(dst, "%s%d.bmp" % (sky_prefix, k)) for k in range(6))
    if not sp["sky"]:
        s += "useSkybox=0\n"
    for kv in (extra or {}).items():
        s += "%s=%s\n" % kv
    s += "\n" + sp["lights"]
    if "text" in sp:
        s += sp["text"]
    else:
        for m in sp["meshes"]:
            s += S.object_text(m, dst, (places or {}).get(m["slot"]))
    return s + "[end]\n"


def write_family_b(dst):
    """Set B's images under dst (beside set A's: util_shading.write_family) and the family's scene files naming them: {name: path}."""
    from rendering_amd import assets
    dst = str(dst)
    for k in range(6):
        with open(os.path.join(dst, "q%d.bmp" % k), "wb") as f:
            f.write(assets.bmp24(sky_image_b(k)))
    out = {}
    for name in S.FAMILY:
        sp = family_b(name)
        for m in sp.get("meshes", []):
            for kind, spec in m["maps"].items():
                with open(os.path.join(dst, S.map_name(kind, spec)), "wb") as f:
                    f.write(assets.bmp24(S.IMAGE[kind](*spec)))
        out[name] = os.path.join(dst, name + "_b.scene")
        with open(out[name], "w") as f:
            f.write(scene_text(sp, dst, "q"))
    return out


def write_scene(dst, file_name, sp, sky_prefix="k", places=None, extra=None):
    path = os.path.join(str(dst), file_name)
    with open(path, "w") as f:
        f.write(scene_text(sp, str(dst), sky_prefix, places, extra))
    return path


def maps_of(name):
    """[(object index, kind letter, set A's spec)] of scene `name`."""
    return [(i, k, spec) for i, m in enumerate(S.FAMILY[name].get("meshes", [])) for k, spec in sorted(m["maps"].items())]


def load_bmp(ra, path):
    """rah_load_bmp: the bytes the loaders decode, uint8 [h, w, 3] in file order (row 0 = the first stored row)."""
    import ctypes as C
    _, host = ra.load()
    w, h = C.c_int(0), C.c_int(0)
    need = host.rah_load_bmp(str(path).encode(), C.byref(w), C.byref(h), None, 0)
    assert need > 0, path
    out = np.zeros(need, np.uint8)
    assert host.rah_load_bmp(str(path).encode(), C.byref(w), C.byref(h), out.ctypes.data_as(C.c_void_p), need) == need
    return out.reshape(h.value, w.value, 3)
