"""Replacing texture maps and skybox without a GPU (include/rtx_texture.h): the host decode over all 2^24 byte triples against a
numpy restatement of the loaders' arithmetic, the loaders pinned to that decode, the edits on a scene that lives on the host alone, the
refusals, and the binding of rtx_texels.  Everything on bits."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import util_shading as S
from tests import util_texture_edit as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
bits = T.bits


@pytest.fixture(scope="module")
def family(tmp_path_factory):
    d = S.short_dir(tmp_path_factory)
    return d, S.write_family(d)


# ---- the decode -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["diffuse", "normal", "specular", "sky"])
def test_decode_texels_over_all_byte_triples(ra, kind):
    for chunk in range(16):
        rgb = T.all_triples(chunk)
        got, want = ra.decode_texels(kind, rgb), T.restated(kind, rgb)
        assert got.shape == want.shape and got.dtype == np.float32
        bad = bits(got) != bits(want)
        assert not bad.any(), "%s: %d texels of chunk %d differ, first %s" % (kind, int(bad.sum()), chunk, rgb.reshape(-1, 3)[np.argmax(bad.reshape(len(rgb) ** 2, -1).any(1))])


def test_decode_keeps_the_sign_of_zero_and_the_zero_vector(ra):
    rgb = np.array([[10, 128, 200], [128, 128, 0], [128, 128, 1]], np.uint8)
    n = ra.decode_texels("normal", rgb)
    assert np.signbit(n[0, 1]) and n[0, 1] == 0, n[0]
    assert np.array_equal(bits(n[1]), bits(np.array([0.0, -0.0, 0.0], np.float32))), n[1]
    assert np.array_equal(bits(n[2]), bits(np.array([0.0, -0.0, 1.0], np.float32))), n[2]
    assert np.array_equal(bits(n), bits(T.restated("normal", rgb)))


def test_the_loaders_store_what_decode_texels_gives(ra, family):
    """One non-square image per kind, written as a BMP and loaded through a scene file: the host scene's maps and skybox faces are the decode
    of the bytes the BMP loader returns."""
    name = "plain_nrm"      # object 0: all three maps in three sizes; the skybox on
    g = ra.Scene(family[1][name], S.W, S.H)
    for kind, spec in S.FAMILY[name]["meshes"][0]["maps"].items():
        raw = T.load_bmp(ra, os.path.join(family[0], S.map_name(kind, spec)))
        assert raw.shape[:2] == (spec[1], spec[0]) and spec[0] != spec[1]
        assert np.array_equal(raw, S.IMAGE[kind](*spec)[::-1])
        got = g.texture(0, T.KINDS[kind])
        assert isinstance(got, np.ndarray) and not g.has_gpu()
        assert np.array_equal(bits(got), bits(ra.decode_texels(T.KINDS[kind], raw))), kind
    for k in range(6):
        raw = T.load_bmp(ra, os.path.join(family[0], "k%d.bmp" % k))
        assert np.array_equal(bits(g.skybox_face(k)), bits(ra.decode_texels("sky", raw))), k
    assert g.texture(1, "diffuse") is None and g.texture(1, "normal") is not None
    g.close()


# ---- host-only edits ------------------------------------------------------------------------------------------------------------------
def canary(h, w, ch):
    """Stored texels no decode gives: negative, all different."""
    a = -(np.arange(h * w * ch, dtype=np.float32) + np.float32(1.5))
    return a.reshape((h, w, 3) if ch == 3 else (h, w))


@pytest.mark.parametrize("kind", ["d", "n", "s"])
def test_host_only_set_and_write(ra, family, kind):
    name = T.KINDS[kind]
    g = ra.Scene(family[1]["plain_nrm"], S.W, S.H)
    img = S.IMAGE[kind](20, 7, 5)                         # [7, 20, 3]
    g.set_texture(2, name, img)                           # (object 2 had a diffuse map only: the others appear)
    assert np.array_equal(bits(g.texture(2, name)), bits(ra.decode_texels(name, img)))
    g.set_texture(2, name, img, top_down=True)
    assert np.array_equal(bits(g.texture(2, name)), bits(ra.decode_texels(name, img[::-1])))
    stored = T.restated(name, img[:, ::-1])
    g.set_texture(2, name, stored)
    assert np.array_equal(bits(g.texture(2, name)), bits(stored))
    # a rectangle into a canary map of 13 x 7, from a source whose pitch exceeds its row
    can = canary(7, 13, 1 if kind == "s" else 3)
    g.set_texture(2, name, can)
    rect = S.IMAGE[kind](8, 3, 9)[:, :5]                  # [3, 5, 3]: a view of an [3, 8, 3] image
    for top_down in (False, True):
        want = can.copy()
        g.set_texture(2, name, can)
        g.write_texture(2, name, rect, x0=3, y0=2, top_down=top_down)
        want[2:5, 3:8] = ra.decode_texels(name, rect[::-1] if top_down else rect)
        assert np.array_equal(bits(g.texture(2, name)), bits(want)), top_down
    g.write_texture(2, name, want[1:2, 12:13].copy() * np.float32(2), x0=0, y0=6)
    want[6, 0] = want[1, 12] * np.float32(2)
    assert np.array_equal(bits(g.texture(2, name)), bits(want))
    g.set_texture(2, name, None)
    assert g.texture(2, name) is None
    assert not g.has_gpu()
    g.close()


def test_host_only_skybox(ra, family):
    g = ra.Scene(family[1]["plain_nosky"], S.W, S.H)
    assert g.skybox_face(0) is None
    faces = [T.sky_image_b(k) for k in range(6)]
    g.set_skybox(faces, top_down=True)
    for k in range(6):
        assert np.array_equal(bits(g.skybox_face(k)), bits(ra.decode_texels("sky", faces[k][::-1])))
    rect = S.colour_image(4, 2, 77)
    before = g.skybox_face(4)
    g.write_skybox(4, rect, x0=9, y0=1)
    before[1:3, 9:13] = ra.decode_texels("sky", rect)
    assert np.array_equal(bits(g.skybox_face(4)), bits(before))
    assert np.array_equal(bits(g.skybox_face(3)), bits(ra.decode_texels("sky", faces[3][::-1])))
    g.set_skybox(None)
    assert g.skybox_face(0) is None
    g.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def snapshot(g, n_objects):
    out = []
    for i in range(n_objects):
        for kind in ("diffuse", "normal", "specular"):
            t = g.texture(i, kind)
            out.append(None if t is None else bits(t).copy())
    for k in range(6):
        t = g.skybox_face(k)
        out.append(None if t is None else bits(t).copy())
    return out


def same(a, b):
    return len(a) == len(b) and all((x is None and y is None) or (x is not None and y is not None and np.array_equal(x, y)) for x, y in zip(a, b))


def test_refusals_leave_the_scene_as_it_was(ra, family, tmp_path):
    g = ra.Scene(family[1]["plain_nrm"], S.W, S.H)
    before = snapshot(g, 4)
    img = S.colour_image(8, 5, 3)
    for bad in (lambda: g.set_texture(4, "diffuse", img), lambda: g.set_texture(-1, "diffuse", img), lambda: g.set_texture(0, "sky", img),
                lambda: g.set_texture(0, "diffuse", img.astype(np.int32)), lambda: g.set_texture(0, "diffuse", img.astype(np.float64)),
                lambda: g.set_texture(0, "diffuse", img[:, :, :2]), lambda: g.set_texture(0, "diffuse", img[:, :, 0].astype(np.float32)),
                lambda: g.set_texture(0, "specular", np.zeros((5, 8, 3), np.float32)), lambda: g.set_texture(0, "diffuse", [[1, 2, 3]]),
                lambda: g.write_texture(0, "diffuse", None), lambda: g.write_texture(0, "diffuse", img, x0=-1),
                lambda: g.set_skybox([img] * 5), lambda: g.set_skybox([img] * 5 + [S.colour_image(8, 6, 3)]),
                lambda: g.set_skybox([img] * 5 + [np.zeros((5, 8, 3), np.float32)]), lambda: g.write_skybox(6, img), lambda: g.skybox_face(6),
                lambda: g.texture(0, "sky")):
        with pytest.raises(ValueError):
            bad()
    for bad in (lambda: g.set_texture(0, "diffuse", np.zeros((0, 8, 3), np.uint8)), lambda: g.set_texture(0, "diffuse", np.zeros((5, 0, 3), np.uint8)),
                lambda: g.write_texture(1, "diffuse", img),                        # (object 1 has no diffuse map)
                lambda: g.write_texture(0, "diffuse", img, x0=64 - 7),             # (a 64 x 24 map)
                lambda: g.write_texture(0, "diffuse", img, y0=24 - 4), lambda: g.write_texture(0, "diffuse", img, x0=64),
                lambda: g.write_texture(0, "diffuse", S.colour_image(68, 5, 3)),
                lambda: g.write_skybox(0, img, x0=S.SKY_W - 7), lambda: g.set_skybox(None)):      # (useSkybox is on)
        with pytest.raises(ra.RtxError):
            bad()
    assert same(snapshot(g, 4), before)
    g.close()
    # an object that is no mesh; a normal map for a mesh whose OBJ has no texture coordinates
    g = ra.Scene(family[1]["analytic"], S.W, S.H)
    with pytest.raises(ValueError):
        g.set_texture(0, "diffuse", img)
    with pytest.raises(ValueError):
        g.texture(0, "diffuse")
    g.close()
    path = tmp_path / "nouv.scene"
    path.write_text("[options]\nwidth=32\nheight=24\nfov=60\nposition=0,0,0\nrotation=0,0,0\nmax_ray_depth=2\nimage_name=output/nouv\n\n"
                    "[light]\ntype=point\nposition=2,3,0\ncolor=1,1,1\nintensity=1\n\n"
                    "[object]\ntype=mesh\npos=0,0,-4\nsize=2,2,2\nrot=0,0,0\ncolor=0.9,0.8,0.7\nname=scenes/assets/bumpy_4k.obj\n\n[end]\n")
    g = ra.Scene(str(path), 32, 24)
    with pytest.raises(ra.RtxError, match="tangents"):
        g.set_texture(0, "normal", S.normal_image(8, 5, 3))
    assert g.texture(0, "normal") is None
    g.set_texture(0, "diffuse", img)
    assert np.array_equal(bits(g.texture(0, "diffuse")), bits(ra.decode_texels("diffuse", img)))
    g.close()


# ---- the binding ----------------------------------------------------------------------------------------------------------------------
def test_rtx_texels_matches_the_header(ra):
    text = open(os.path.join(ROOT, "include", "rtx_texture.h")).read()
    body = re.search(r"typedef struct rtx_texels \{(.*?)\} rtx_texels;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "const void*": C.c_void_p, "int64_t": C.c_int64}
    fields = []
    for decl in [d.strip() for d in body.split(";") if d.strip()]:
        m = re.match(r"(const void\*|u?int(?:32|64)_t)\s+(.*)$", decl)
        assert m, decl
        fields += [(n.strip(), ctype[m.group(1)]) for n in m.group(2).split(",")]
    assert fields == list(ra.RtxTexels._fields_)
    assert C.sizeof(ra.RtxTexels) == 32 and ra.RtxTexels.data_dev.offset == 16 and ra.RtxTexels.row_pitch.offset == 24
    enums = dict((n, int(v)) for n, v in re.findall(r"(RTX_TEX(?:ELS)?_[A-Z0-9]+)\s*=\s*(\d+)", text))
    assert {k: enums["RTX_TEX_" + k.upper()] for k in ra.TEXTURE_KINDS} == ra.TEXTURE_KINDS
    assert (enums["RTX_TEXELS_STORED"], enums["RTX_TEXELS_RGB8"]) == (ra.TEXELS_STORED, ra.TEXELS_RGB8)
    declared = set(re.findall(r"\b(rtx_[a-z0-9_]+)\s*\(", text))
    assert declared == set(ra.RTX_TEXTURE_SYMBOLS)


def test_exported_symbols(ra):
    listed, missing = ra.exported_symbols()
    assert missing == [] and listed == list(ra.RTX_SYMBOLS)
    assert not set(ra.RTX_TEXTURE_SYMBOLS) & set(ra.RTX_SYMBOLS)
    rtx, host = ra.load()
    for s in ra.RTX_TEXTURE_SYMBOLS:
        assert hasattr(rtx, s), s
    for s in ("rah_decode_texels", "rah_mesh_set_map", "rah_scene_set_sky", "rah_write_texels", "rah_texture"):
        assert hasattr(host, s), s
