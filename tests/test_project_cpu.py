"""rtx_project_points (Scene.camera_table, project_points, bake_view; include/rtx_project.h) without a GPU: the header against the symbol
list and the binding, the refusals, and tests/util_project's restatement of the contract pinned to the oracle alone -- the oracle's own
primary rays, taken to their hits and projected back into the oracle's camera, land in the pixel they left from -- and the choice of the
second camera the GPU tests project into, with the oracle's occlusion answers."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import util_aov as U
from tests import util_occlusion as OC
from tests import util_project as UPJ
from tests.test_light_rays_cpu import analytic_case

ROOT = U.ROOT
f32 = np.float32


def test_project_header_and_symbol_list(ra):
    hdr = open(os.path.join(ROOT, "include", "rtx_project.h")).read()
    declared = re.findall(r"^int\s+(rtx_[a-z0-9_]+)\s*\(", hdr, re.M)
    assert declared == list(ra.RTX_PROJECT_SYMBOLS) == ["rtx_project_points"]
    assert '#include "rtx_points.h"' in hdr
    others = [n for n in dir(ra) if re.fullmatch(r"RTX_[A-Z_]*SYMBOLS", n) and n != "RTX_PROJECT_SYMBOLS"]
    assert len(others) >= 16
    for other in others:
        assert not set(declared) & set(getattr(ra, other)), other
    rtx, _ = ra.load()
    for s in declared:
        assert hasattr(rtx, s), s
    listed, missing = ra.exported_symbols()
    assert not missing and listed == list(ra.RTX_SYMBOLS)
    src = open(os.path.join(ROOT, "rendering_amd", "__init__.py")).read()
    assert "RTX_PROJECT_SYMBOLS" in re.search(r"def exported_symbols\(\):.*?return", src, re.S).group(0)
    # the constants and the structure of the binding are the header's
    defines = dict(re.findall(r"^#define\s+(RTX_PROJ\w+)\s+(\d+)u?\b", hdr, re.M))
    assert defines == {"RTX_PROJECT_CAMERA_FLOATS": "24", "RTX_PROJ_FRONT": "1", "RTX_PROJ_INSIDE": "2", "RTX_PROJ_FACING": "4", "RTX_PROJ_OPEN": "8"}
    assert (ra.PROJECT_CAMERA_FLOATS, ra.PROJ_FRONT, ra.PROJ_INSIDE, ra.PROJ_FACING, ra.PROJ_OPEN) == (24, 1, 2, 4, 8)
    assert (UPJ.CAMERA_FLOATS, UPJ.FRONT, UPJ.INSIDE, UPJ.FACING, UPJ.OPEN) == (24, 1, 2, 4, 8)
    body = re.search(r"typedef struct rtx_project_buffers \{(.*?)\} rtx_project_buffers;", hdr, re.S).group(1)
    fields = re.findall(r"(float\*|uint8_t\*)\s+(\w+);", body)
    assert fields == [("float*", "pixel_dev"), ("float*", "depth_dev"), ("uint8_t*", "flags_dev")]
    assert [n for n, _ in ra.ProjectBuffers._fields_] == [n for _, n in fields]
    assert [t for _, t in ra.ProjectBuffers._fields_] == [C.c_void_p] * 3
    for name in ("camera_table", "project_points", "bake_view"):
        assert callable(getattr(ra.Scene, name))


def test_c_entry_refuses_a_null_scene(ra):
    rtx, _ = ra.load()
    buf = ra.ProjectBuffers()
    assert rtx.rtx_project_points(None, 4, None, 1, None, 1, C.byref(buf), None) == -1      # RTX_ERR_ARG
    assert b"NULL" in rtx.rtx_last_error()
    assert rtx.rtx_project_points(None, 0, None, 0, None, 0, None, None) == -1
    assert b"NULL" in rtx.rtx_last_error()


def test_wrapper_refusals_before_the_gpu(ra):
    torch = pytest.importorskip("torch")
    s = ra.Scene("scenes/cfg1_simple_shapes.scene", 32, 24)
    z = lambda shape, dt=torch.float32: torch.zeros(shape, dtype=dt)
    cams = [((0, 0, 0), (0, 0, 0))]
    cases = [
        (dict(points=z((4, 6)), cameras=cams, pixel=False, flags=False), "project_points: nothing to compute"),
        (dict(points=np.zeros((4, 6), np.float32), cameras=cams), "project_points: points must be a torch tensor"),
        (dict(points=z((4, 6), torch.float64), cameras=cams), "project_points: points must be float32"),
        (dict(points=z((6, 4)), cameras=cams), r"project_points: points must have shape \(n, 6\)"),
        (dict(points=z((4, 12))[:, ::2], cameras=cams), "project_points: points must be contiguous"),
        (dict(points=z((4, 6)), cameras=cams), "project_points: points must be on cuda:0"),
    ]
    for kw, what in cases:
        with pytest.raises(ValueError, match=what):
            s.project_points(**kw)
    for bad, what in (([], "1 .. 256 cameras, got 0"), (cams * 257, "1 .. 256 cameras, got 257"), ([((0, 0, 0),)], r"camera 0 must be \(pos, rot\)")):
        with pytest.raises(ValueError, match="camera_table: " + what):
            s._camera_records(bad)
    with pytest.raises(ValueError, match="camera_table: width and height must be positive"):
        s._camera_records(cams, 0, 4)
    with pytest.raises(ValueError, match="bake_view: image must be a torch tensor"):
        s.bake_view(0, cams[0], np.zeros((4, 4, 3), np.float32))
    with pytest.raises(ValueError, match=r"bake_view: image must have shape \(H, W, 3\)"):
        s.bake_view(0, cams[0], z((4, 4)))
    assert s._gpu is None                  # (the scene was never flattened and uploaded: no GPU call was made)
    s.close()


def test_camera_records_are_the_view_targets_fields(ra, oracle):
    """Field by field, on the host: a record is view_target's camera at the size asked for; the scene's own pose at the scene's size is
    the oracle's camera."""
    path = "scenes/cfg1_simple_shapes.scene"
    s = ra.Scene(path, 48, 32)
    cams = [((0, 0, 0), (0, 0, 0)), UPJ.SECOND_CAMERA, UPJ.WIDE_CAMERA] + ra.cube_cameras((0.5, 1.0, -2.0))
    for size in ((None, None), UPJ.WIDE_SIZE):
        rec = s._camera_records(cams, *size)
        assert rec.shape == (len(cams), 24) and rec.dtype == f32
        for r, cam in zip(rec, cams):
            t = s.view_target(cam[0], cam[1], cam[2] if len(cam) == 3 else None, *size)
            want = UPJ.record(f32(t.scale), f32(t.aspect), np.array(t.cam_matrix, f32), np.array(t.cam_pos, f32), t.width, t.height)
            assert np.array_equal(U.bits(r), U.bits(want)) and r[7] == 0
            assert (r[5], r[6]) == ((48, 32) if size[0] is None else size)
    o = oracle.OracleScene(path, 48, 32)
    own = UPJ.record(*o.camera(), 48, 32)
    o.close()
    assert np.array_equal(U.bits(s._camera_records(cams[:1])[0]), U.bits(own))
    assert (s.width, s.height) == (48, 32)
    s.close()


# tests/util_project itself.  What was met when this was written (recorded, not asserted) -- the largest |px - x|, |py - y| over the hit
# pixels: cfg1_simple_shapes 48x32 3.81e-06, 1.91e-06 (1053 pixels); cfg2_smooth_4k 48x32 3.81e-06, 9.54e-07 (853 pixels).
@pytest.mark.parametrize("name", ["cfg1_simple_shapes", "cfg2_smooth_4k"])
def test_the_oracles_hits_project_into_their_own_pixels(oracle, name):
    w, h = 48, 32
    o = oracle.OracleScene("scenes/%s.scene" % name, w, h)
    rays = U.primary_rays(o)
    hits, _ = o.probe(rays, colours=False)
    rec = UPJ.record(*o.camera(), w, h)
    o.close()
    # the pixels pass 1 renders (x < w - 1, y < h - 1) whose ray hits
    sel = (hits[:, 0] > 0) & U.written_mask(w, h).reshape(-1)
    assert sel.sum() >= 0.5 * w * h
    P = (rays[sel, 0:3] + rays[sel, 3:6] * hits[sel, 3:4]).astype(f32)                  # castRay's hit point (scene.cpp:763)
    plan = UPJ.Plan(np.concatenate([P, np.zeros_like(P)], 1), rec[None, :])
    ys, xs = np.divmod(np.nonzero(sel)[0], w)
    both = UPJ.FRONT | UPJ.INSIDE
    assert ((plan.geo[0] & both) == both).all()
    near = plan.nearest()[0]
    assert np.array_equal(near[:, 0], xs.astype(f32)) and np.array_equal(near[:, 1], ys.astype(f32))
    print("%s %dx%d: %d hit pixels, largest |px - x| %.3g, |py - y| %.3g" % (
        name, w, h, sel.sum(), np.abs(plan.pixel[0, :, 0] - xs).max(), np.abs(plan.pixel[0, :, 1] - ys).max()))
    assert plan.walk.all() and not (plan.geo & UPJ.FACING).any()                        # (a zero normal never faces)


def second_camera_case(ra, oracle, tmp_path):
    """cfg1_simple_shapes at 48x32: {P, N} of the oracle's hits on planes and spheres with their exact normals (tests/test_points_cpu.py),
    projected into the scene's own camera and the second camera, with the oracle's occlusion answers"""
    path, w, h = "scenes/cfg1_simple_shapes.scene", 48, 32
    o, blocks, rays, hits, col, obj, N, albedo, material, const = analytic_case(oracle, path, w, h)
    o.close()
    with np.errstate(all="ignore"):
        P = (rays[:, 0:3] + rays[:, 3:6] * hits[:, 3:4]).astype(f32)
    s = ra.Scene(path, w, h)
    table = s._camera_records([((0, 0, 0), (0, 0, 0)), UPJ.SECOND_CAMERA])
    s.close()
    plan = UPJ.Plan(np.concatenate([P, N], 1), table)
    hit2, t2 = OC.opaque_probe(oracle, path, tmp_path, plan.shadow_rays)
    return plan, OC.expected(hit2, t2, plan.shadow_tmax)


# What was met when this was written: 881 points; second camera -- FRONT && INSIDE 0.564 of the pairs, of those open 0.302, blocked 0.698;
# own camera -- every pair FRONT, and INSIDE and open but for the pixels of the last row and column.
def test_the_second_camera_has_every_class(ra, oracle, tmp_path):
    plan, occluded = second_camera_case(ra, oracle, tmp_path)
    n = plan.n
    assert n >= 700
    own, second = plan.walk[0], plan.walk[1]
    # the scene's own camera sees what its rays hit: every pair is FRONT, INSIDE unless its pixel is in the last row or column (which pass 1
    # does not render), and open (the shadow ray runs back along the primary ray)
    near = plan.nearest()[0]
    assert ((plan.geo[0] & UPJ.FRONT) != 0).all() and own.sum() >= 0.9 * n
    assert ((near[~own, 0] == 47) | (near[~own, 1] == 31)).all() and (near[own, 0] < 47).all() and (near[own, 1] < 31).all()
    n_own = int(own.sum())
    assert not occluded[:n_own].any()
    occ2 = occluded[n_own:]
    inside = float(second.sum()) / n
    open_, blocked = float((occ2 == 0).sum()) / max(len(occ2), 1), float((occ2 != 0).sum()) / max(len(occ2), 1)
    print("second camera: %d points, FRONT && INSIDE %.3f; of those open %.3f, blocked %.3f" % (n, inside, open_, blocked))
    assert open_ >= 0.02 and blocked >= 0.02 and 1 - inside >= 0.02
    fl = plan.flags(occluded)
    assert ((fl & UPJ.OPEN) != 0).sum() == (occluded == 0).sum() and not (fl[~plan.walk] & UPJ.OPEN).any()
    assert not (plan.flags(None) & UPJ.OPEN).any() and np.array_equal(plan.flags(None), fl & ~np.uint8(UPJ.OPEN))
    # facing: both answers occur for the second camera
    facing = (fl[1] & UPJ.FACING) != 0
    assert facing.any() and not facing.all()


def test_special_points_have_their_classes(ra):
    s = ra.Scene("scenes/cfg1_simple_shapes.scene", 48, 32)
    table = s._camera_records([((0, 0, 0), (0, 0, 0)), UPJ.SECOND_CAMERA] + ra.cube_cameras((0.5, 1.0, -2.0)))
    s.close()
    pts = UPJ.special_points(table)
    plan = UPJ.Plan(pts, table)
    behind = (plan.geo & UPJ.FRONT) == 0
    at_camera = plan.depth == 0
    with np.errstate(all="ignore"):
        unbounded = ~np.isfinite(plan.pixel).all(-1) & (plan.depth > 0)
    assert behind.any(1).all() and at_camera.any(1).all() and unbounded.any()
    # c == 0: L = 0, sz = 0, the pixel is NaN, nothing but the buffers' own values; never FRONT, INSIDE or FACING
    assert np.isnan(plan.pixel[at_camera]).all() and not plan.geo[at_camera].any()
    assert not plan.walk[behind].any() and not plan.walk[unbounded].any()
