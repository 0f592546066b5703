"""rtx_render_views / Scene.render_views without a GPU: the extension header, its symbol lists and the ctypes structure; the refusals that need no
device; the map from a batch's work items to views and tiles (rtx_views_plan_probe: the functions the kernels use, csrc/rtx_views_plan.h); and
rah_view_target against scenes loaded from rewritten scene files."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the sizes the issue names: a tile and less, no multiples of 8, a wide and a tall view
MIXED = [(7, 5), (1, 1), (2, 2), (41, 27), (200, 8), (8, 200), (64, 64), (9, 8), (8, 9), (1, 40), (40, 1)]


def decl(text):
    return set(re.findall(r"\b(rtx_[a-z0-9_]+)\s*\(", text))


def test_header_symbol_lists_and_structure(ra):
    hdr = open(os.path.join(ROOT, "include", "rtx_views.h")).read()
    assert decl(hdr) == set(ra.RTX_VIEWS_SYMBOLS) == {"rtx_render_views"}
    debug = open(os.path.join(ROOT, "include", "rtx_debug.h")).read()
    assert "rtx_views_plan_probe" in decl(debug) and "rtx_views_plan_probe" in ra.RTX_SYMBOLS
    for other in (ra.RTX_SYMBOLS, ra.RTX_EDIT_SYMBOLS, ra.RTX_QUERY_SYMBOLS, ra.RTX_AOV_SYMBOLS, ra.RTX_AO_SYMBOLS, ra.RTX_SURFACE_SYMBOLS, ra.RTX_LIGHT_SYMBOLS,
                  ra.RTX_DEFORM_SYMBOLS):
        assert not set(ra.RTX_VIEWS_SYMBOLS) & set(other)
    rtx, host = ra.load()
    assert hasattr(rtx, "rtx_render_views") and hasattr(rtx, "rtx_views_plan_probe") and hasattr(host, "rah_view_target")
    listed, missing = ra.exported_symbols()
    assert not missing and listed == list(ra.RTX_SYMBOLS)
    # the structure's fields, in the header's order and with its types
    body = re.search(r"typedef struct rtx_view_target \{(.*?)\} rtx_view_target;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if not stmt:
            continue
        m = re.match(r"(uint32_t|float\*|uint8_t\*|float)\s*(.*)", stmt)
        ctype = {"uint32_t": C.c_uint32, "float": C.c_float, "float*": C.c_void_p, "uint8_t*": C.c_void_p}[m.group(1)]
        for name in m.group(2).split(","):
            a = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", name)
            fields.append((a.group(1), ctype * int(a.group(2)) if a.group(2) else ctype))
    assert fields == list(ra.ViewTarget._fields_)
    assert C.sizeof(ra.ViewTarget) == 8 + 12 + 64 + 8 + 4 + 16      # (4 bytes of padding before the pointers)
    limits = {k: int(v) for k, v in re.findall(r"#define (RTX_VIEWS_MAX_\w+)\s+(\d+)u", hdr)}
    assert limits["RTX_VIEWS_MAX_VIEWS"] >= 4096 and limits["RTX_VIEWS_MAX_SIDE"] >= 8192


def test_refusals_that_need_no_device(ra):
    rtx, _ = ra.load()
    t = (ra.ViewTarget * 1)()
    assert rtx.rtx_render_views(None, 1, t, 0, None) == -1      # RTX_ERR_ARG
    assert b"scene is NULL" in rtx.rtx_last_error()
    assert rtx.rtx_render_views(None, 0, None, 1, None) == -1
    # the sizes and counts of a batch are checked by one function for the call and for its probe
    n = C.c_size_t(0)
    probe = lambda sizes: rtx.rtx_views_plan_probe(len(sizes) // 2, np.asarray(sizes, np.uint32).ctypes.data_as(C.c_void_p), None, 0, C.byref(n))
    for sizes, what in (([8, 0], b"zero width or height"), ([0, 8], b"zero width or height"), ([16, 16, 4, 0], b"view 1 has a zero"),
                        ([32769, 8], b"RTX_VIEWS_MAX_SIDE"), ([8, 32769], b"RTX_VIEWS_MAX_SIDE"), ([8, 8] * 65537, b"RTX_VIEWS_MAX_VIEWS"),
                        ([8192, 8192] * 4 + [1, 1], b"RTX_VIEWS_MAX_TILES")):
        assert probe(sizes) == -1 and what in rtx.rtx_last_error(), sizes[:6]
    assert probe([8192, 8192] * 4) == 0 and n.value == 4 * 1024 * 1024      # (the limit itself is legal)
    assert probe([32768, 8]) == 0 and n.value == 4096
    assert probe([8, 8] * 4096) == 0 and n.value == 4096
    assert rtx.rtx_views_plan_probe(1, None, None, 0, C.byref(n)) == -1 and rtx.rtx_views_plan_probe(0, None, None, 0, None) == -1
    assert rtx.rtx_views_plan_probe(0, None, None, 0, C.byref(n)) == 0 and n.value == 0


def test_wrapper_refuses_bad_arguments_before_the_gpu(ra):
    torch = pytest.importorskip("torch")
    s = ra.Scene("scenes/cfg1_simple_shapes.scene", 32, 24)
    cam = ((0, 0, 0), (0, 0, 0))
    z = lambda shape, dt=torch.float32: torch.zeros(shape, dtype=dt)
    cases = [
        (dict(cameras=[cam], fbs=[np.zeros((8, 8, 3), np.float32)]), r"fbs\[0\] must be a torch tensor"),
        (dict(cameras=[cam], fbs=[z((8, 8, 3), torch.float64)]), r"fbs\[0\] must be float32"),
        (dict(cameras=[cam], fbs=[z((8, 8))]), r"fbs\[0\] must have shape \(H, W, 3\)"),
        (dict(cameras=[cam, cam], fbs=[z((8, 8, 3))]), "2 cameras but 1 framebuffers"),
        (dict(cameras=[cam], fbs=z((8, 8, 3))), r"fbs must have shape \(N, H, W, 3\)"),
        (dict(cameras=[cam], fbs=[z((8, 8, 3))], ssaa=True), "ssaa needs masks"),
        (dict(cameras=[cam], fbs=[z((8, 8, 3))], masks=[]), "1 cameras but 0 masks"),
        (dict(cameras=[((0, 0, 0),)], fbs=[z((8, 8, 3))]), r"camera 0 must be \(pos, rot\)"),
        (dict(cameras=[cam], fbs=[z((8, 8, 3))]), r"fbs\[0\] must be on cuda:0"),
    ]
    for kw, what in cases:
        with pytest.raises(ValueError, match=what):
            s.render_views(**kw)
    assert s._gpu is None              # (the scene was never flattened and uploaded: no GPU call was made)
    s.close()


def check_plan(ra, sizes):
    items = ra.views_plan_probe(sizes)
    want = sum(((w + 7) // 8) * ((h + 7) // 8) for w, h in sizes)
    assert items.shape == (want, 3)
    v, tx, ty = items[:, 0].astype(np.int64), items[:, 1].astype(np.int64), items[:, 2].astype(np.int64)
    assert (v >= 0).all() and (v < len(sizes)).all() and (np.diff(v) >= 0).all()
    W = np.asarray([s[0] for s in sizes], np.int64)[v]; H = np.asarray([s[1] for s in sizes], np.int64)[v]
    # no item lies outside its view: the tile has a pixel of it
    assert (tx * 8 < W).all() and (ty * 8 < H).all()
    # every tile of every view exactly once
    key = (v << 40) | (ty << 20) | tx
    assert len(np.unique(key)) == want
    counts = np.bincount(v, minlength=len(sizes))
    assert counts.tolist() == [((w + 7) // 8) * ((h + 7) // 8) for w, h in sizes]
    return items


def test_plan_covers_every_tile_of_every_view_once(ra):
    items = check_plan(ra, MIXED)
    # view 3 is 41 x 27: six tiles across, four down, row by row after the items of the views before it
    first = 1 + 1 + 1
    assert items[first:first + 24].tolist() == [[3, t % 6, t // 6] for t in range(24)]
    for one in MIXED + [(8, 8), (16, 8), (1023, 3)]:
        check_plan(ra, [one])
    rng = np.random.default_rng(7)
    many = [(int(w), int(h)) for w, h in rng.integers(1, 70, size=(700, 2))]
    check_plan(ra, many)
    check_plan(ra, [(24, 16)] * 300)
    check_plan(ra, MIXED * 40)
    assert ra.views_plan_probe([]).shape == (0, 3)


def rewritten(src, pos, rot, fov):
    lines = src.split("\n")
    i = lines.index("[options]")
    j = next(k for k in range(i + 1, len(lines)) if lines[k].startswith("["))      # (lights have a position= of their own)
    keep = [l for l in lines[i + 1:j] if not l.startswith(("position=", "rotation=") + (("fov=",) if fov is not None else ()))]
    lines[i + 1:j] = keep + ["position=%r,%r,%r" % pos, "rotation=%r,%r,%r" % rot] + (["fov=%r" % fov] if fov is not None else [])
    return "\n".join(lines)


@pytest.mark.parametrize("name", ["cfg1_simple_shapes", "mixed_materials"])
def test_view_target_equals_a_scene_loaded_with_that_camera(ra, tmp_path, name):
    src = open(os.path.join(ROOT, "scenes", name + ".scene")).read()
    s = ra.Scene("scenes/%s.scene" % name, 48, 32)
    before = [np.array(a, copy=True) for a in s.camera()] + [s.width, s.height] + [np.array(a) for a in s.camera_pose()]
    cases = [((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), None, 48, 32), ((0.15, 0.1, 0.2), (-4.0, 9.0, 2.0), None, 41, 27), ((-0.3, 0.25, 0.4), (3.0, -14.0, -1.0), 35.0, 200, 8),
             ((0.0, 0.6, -0.5), (-25.0, 0.0, 0.0), 90.0, 8, 200), ((1.5, -2.0, 3.0), (90.0, 45.0, 180.0), 117.5, 7, 5), ((0.1, 0.2, 0.3), (0.0, 90.0, 0.0), 60.0, 1, 1)]
    for k, (pos, rot, fov, w, h) in enumerate(cases):
        t = s.view_target(pos, rot, fov, w, h)
        p = tmp_path / ("%s_%d.scene" % (name, k))
        p.write_text(rewritten(src, pos, rot, fov))
        f = ra.Scene(str(p), w, h)
        scale, aspect, m, cp = f.camera()
        f.close()
        bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
        assert (t.width, t.height) == (w, h)
        assert np.array_equal(bits(np.float32(t.scale)), bits(scale)) and np.array_equal(bits(np.float32(t.aspect)), bits(aspect)), (k, t.scale, scale)
        assert np.array_equal(bits(np.asarray(t.cam_matrix[:])), bits(m)) and np.array_equal(bits(np.asarray(t.cam_pos[:])), bits(cp))
        assert t.fb_dev is None and t.mask_dev is None
    after = [np.array(a, copy=True) for a in s.camera()] + [s.width, s.height] + [np.array(a) for a in s.camera_pose()]
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    with pytest.raises(ValueError, match="must be > 0"):
        s.view_target((0, 0, 0), (0, 0, 0), None, 0, 4)
    s.close()


def test_cube_cameras_look_along_the_six_axes(ra):
    s = ra.Scene("scenes/cfg1_simple_shapes.scene", 16, 16)
    cams = ra.cube_cameras((0.5, 1.0, -2.0))
    assert len(cams) == 6
    want = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    for (pos, rot, fov), axis in zip(cams, want):
        assert pos == (0.5, 1.0, -2.0) and fov == 90.0
        t = s.view_target(pos, rot, fov, 16, 16)
        m = np.asarray(t.cam_matrix[:], np.float32)
        # the view direction: (0, 0, -1) through the camera's matrix, as primaryRay applies it (row vector x matrix)
        d = -m[8:11]
        assert np.allclose(d, axis, atol=1e-6), (rot, d)
        assert abs(t.scale - 1.0) < 1e-6 and t.aspect == 1.0      # 90 degrees on a square face: the faces meet at their edges
    s.close()
