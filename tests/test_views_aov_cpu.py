"""rtx_render_views_aov / Scene.render_views_aov without a GPU: the extension header, its symbol list and the ctypes structure, that
include/rtx_views.h and ViewTarget are what they were, and the refusals that need no device -- the C entry's and every one of the wrapper's,
raised before the scene is uploaded."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTYPES = {"uint32_t": C.c_uint32, "float": C.c_float, "float*": C.c_void_p, "int32_t*": C.c_void_p, "uint8_t*": C.c_void_p}


def decl(text):
    return re.findall(r"\b(rtx_[a-z0-9_]+)\s*\(", text)


def struct_fields(hdr, name):
    """[(field, ctypes type)] of `typedef struct name { ... } name;` in the header's order (tests/test_render_views_cpu.py's parse)"""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if not stmt:
            continue
        m = re.match(r"(uint32_t|int32_t\*|uint8_t\*|float\*|float)\s*(.*)", stmt)
        ctype = CTYPES[m.group(1)]
        for field in m.group(2).split(","):
            a = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", field)
            fields.append((a.group(1), ctype * int(a.group(2)) if a.group(2) else ctype))
    return fields


def test_header_symbol_list_and_structure(ra):
    hdr = open(os.path.join(ROOT, "include", "rtx_views_aov.h")).read()
    assert decl(hdr) == list(ra.RTX_VIEWS_AOV_SYMBOLS) == ["rtx_render_views_aov"]
    lists = [k for k in dir(ra) if re.fullmatch(r"RTX_\w*SYMBOLS", k)]
    assert "RTX_VIEWS_SYMBOLS" in lists and "RTX_SYMBOLS" in lists and len(lists) >= 14
    for k in lists:
        if k != "RTX_VIEWS_AOV_SYMBOLS":
            assert not set(ra.RTX_VIEWS_AOV_SYMBOLS) & set(getattr(ra, k)), k
    rtx, _ = ra.load()
    listed, missing = ra.exported_symbols()
    assert not missing and listed == list(ra.RTX_SYMBOLS)
    assert hasattr(rtx, "rtx_render_views_aov")
    # exported_symbols looks for the new entry point: a library without it is reported
    src = open(os.path.join(ROOT, "rendering_amd", "__init__.py")).read()
    assert "RTX_VIEWS_AOV_SYMBOLS" in re.search(r"def exported_symbols\(\):.*?return", src, re.S).group(0)
    fields = struct_fields(hdr, "rtx_view_aov_target")
    assert fields == list(ra.ViewAovTarget._fields_)
    assert [f for f, _ in fields[6:]] == ["depth_dev", "object_dev", "triangle_dev", "uv_dev", "normal_dev", "albedo_dev", "position_dev", "rays_dev"]
    assert C.sizeof(ra.ViewAovTarget) == 8 + 12 + 64 + 8 + 4 + 8 * 8      # (4 bytes of padding before the pointers)
    # the size and camera fields lie as ViewTarget's do: rah_view_target fills either
    for (f, _), (g, _) in zip(ra.ViewTarget._fields_[:6], ra.ViewAovTarget._fields_[:6]):
        assert f == g and getattr(ra.ViewTarget, f).offset == getattr(ra.ViewAovTarget, g).offset
    # the limits are rtx_views.h's, not defined again
    assert "#define RTX_VIEWS_MAX" not in hdr and '#include "rtx_views.h"' in hdr


def test_the_other_batch_header_is_unchanged(ra):
    hdr = open(os.path.join(ROOT, "include", "rtx_views.h")).read()
    assert decl(hdr) == ["rtx_render_views"] == list(ra.RTX_VIEWS_SYMBOLS)
    assert struct_fields(hdr, "rtx_view_target") == list(ra.ViewTarget._fields_)
    assert [f for f, _ in ra.ViewTarget._fields_] == ["width", "height", "cam_pos", "cam_matrix", "scale", "aspect", "fb_dev", "mask_dev"]
    assert C.sizeof(ra.ViewTarget) == 8 + 12 + 64 + 8 + 4 + 16
    assert dict(re.findall(r"#define (RTX_VIEWS_MAX_\w+)\s+(\d+)u", hdr)) == {"RTX_VIEWS_MAX_VIEWS": "65536", "RTX_VIEWS_MAX_SIDE": "32768", "RTX_VIEWS_MAX_TILES": "4194304"}


def test_refusals_that_need_no_device(ra):
    rtx, _ = ra.load()
    t = (ra.ViewAovTarget * 1)()
    assert rtx.rtx_render_views_aov(None, 1, t, None) == -1      # RTX_ERR_ARG
    assert b"scene is NULL" in rtx.rtx_last_error()
    assert rtx.rtx_render_views_aov(None, 0, None, None) == -1
    assert b"scene is NULL" in rtx.rtx_last_error()
    # (NULL views with a scene: tests/test_gpu_views_aov.py -- a scene needs a device)
    # the shared size check names its caller: the probe's messages are still the other call's
    n = C.c_size_t(0)
    assert rtx.rtx_views_plan_probe(1, np.asarray([8, 0], np.uint32).ctypes.data_as(C.c_void_p), None, 0, C.byref(n)) == -1
    assert rtx.rtx_last_error().startswith(b"rtx_render_views: view 0 has a zero width or height")


def test_wrapper_refuses_bad_arguments_before_the_gpu(ra):
    torch = pytest.importorskip("torch")
    s = ra.Scene("scenes/cfg1_simple_shapes.scene", 32, 24)
    cam = ((0, 0, 0), (0, 0, 0))
    z = lambda shape, dt=torch.float32: torch.zeros(shape, dtype=dt)
    cases = [
        # not a tensor
        (dict(cameras=[cam], depth=[np.zeros((8, 8), np.float32)]), r"depth\[0\] must be a torch tensor"),
        (dict(cameras=[cam], depth=np.zeros((1, 8, 8), np.float32)), r"depth must be a torch tensor or a list of torch tensors, got ndarray"),
        (dict(cameras=[cam], rays=7), r"rays must be a torch tensor or a list"),
        # dtype
        (dict(cameras=[cam], depth=[z((8, 8), torch.float64)]), r"depth\[0\] must be float32"),
        (dict(cameras=[cam], object_id=[z((8, 8))]), r"object_id\[0\] must be int32"),
        (dict(cameras=[cam], triangle_id=z((1, 8, 8), torch.int64)), r"triangle_id must be int32"),
        # shape
        (dict(cameras=[cam], uv=[z((8, 8, 3))]), r"uv\[0\] must have shape \(H, W, 2\)"),
        (dict(cameras=[cam], normal=[z((8, 8))]), r"normal\[0\] must have shape \(H, W, 3\)"),
        (dict(cameras=[cam], albedo=[z((8, 8, 2))]), r"albedo\[0\] must have shape \(H, W, 3\)"),
        (dict(cameras=[cam], position=[z((8, 8, 4))]), r"position\[0\] must have shape \(H, W, 3\)"),
        (dict(cameras=[cam], rays=[z((8, 8, 3))]), r"rays\[0\] must have shape \(H, W, 6\)"),
        (dict(cameras=[cam], rays=z((8, 8, 6))), r"rays must have shape \(N, H, W, 6\)"),
        (dict(cameras=[cam], depth=[z((8, 8)).t()[:, ::2]]), r"depth\[0\] must be contiguous"),
        (dict(cameras=[cam], depth=[z((0, 8))]), r"depth\[0\] is empty"),
        # one form for all channels
        (dict(cameras=[cam], depth=z((1, 8, 8)), rays=[z((8, 8, 6))]), "must all be one tensor or all be lists"),
        # lists of different lengths / another number of views than cameras
        (dict(cameras=[cam, cam], depth=[z((8, 8)), z((8, 8))], rays=[z((8, 8, 6))]), "2 cameras but 1 tensors in rays"),
        (dict(cameras=[cam, cam], depth=[z((8, 8))]), "2 cameras but 1 tensors in depth"),
        (dict(cameras=[cam, cam], depth=z((3, 8, 8))), "2 cameras but 3 views in depth"),
        # the channels of one view disagree in size
        (dict(cameras=[cam, cam], depth=[z((8, 8)), z((5, 7))], uv=[z((8, 8, 2)), z((7, 5, 2))]), r"uv\[1\] must have shape \(5, 7, 2\)"),
        (dict(cameras=[cam], depth=z((1, 8, 8)), normal=z((1, 8, 9, 3))), r"normal must have shape \(1, 8, 8, 3\)"),
        (dict(cameras=[cam, cam], depth=z((2, 8, 8)), object_id=z((1, 8, 8), torch.int32)), r"object_id must have shape \(2, 8, 8\)"),
        # no channel
        (dict(cameras=[cam]), "nothing to compute"),
        # a bad camera tuple
        (dict(cameras=[((0, 0, 0),)], depth=[z((8, 8))]), r"camera 0 must be \(pos, rot\)"),
        (dict(cameras=[cam, (0, 0, 0, 0)], depth=z((2, 8, 8))), r"camera 1 must be \(pos, rot\)"),
        # device
        (dict(cameras=[cam], depth=[z((8, 8))]), r"depth\[0\] must be on cuda:0"),
        (dict(cameras=[cam], rays=z((1, 8, 8, 6))), r"rays must be on cuda:0"),
    ]
    for kw, what in cases:
        with pytest.raises(ValueError, match=what):
            s.render_views_aov(**kw)
    assert s._gpu is None              # (the scene was never flattened and uploaded: no GPU call was made)
    s.close()
