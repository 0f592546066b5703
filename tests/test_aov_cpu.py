"""rtx_render_aov / Scene.render_aov without a GPU: the extension header and its symbol list, the argument checks, the construction of the
expected channels (tests/util_aov.py) proved against the oracle's own pass 1, and the inputs of the GPU tests (tests/test_gpu_aov.py) shown
to be non-trivial: hits and misses, several objects, normal maps that turn the normal, a diffuse map with many texels in view."""
import os
import re

import numpy as np
import pytest

from tests import util_aov as U
from tests import util_shading as S

ROOT = U.ROOT


@pytest.fixture(scope="module")
def family(tmp_path_factory):
    d = S.short_dir(tmp_path_factory)
    return d, S.write_family(d)


def path_of(name, family):
    return family[1][name] if name in S.FAMILY else "scenes/%s.scene" % name


def test_aov_header_and_symbol_list(ra):
    hdr = open(os.path.join(ROOT, "include", "rtx_aov.h")).read()
    declared = set(re.findall(r"\b(rtx_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(ra.RTX_AOV_SYMBOLS) and len(ra.RTX_AOV_SYMBOLS) == len(declared)
    assert not declared & set(ra.RTX_SYMBOLS) and not declared & set(ra.RTX_EDIT_SYMBOLS) and not declared & set(ra.RTX_QUERY_SYMBOLS)
    rtx, _ = ra.load()
    for s in declared:
        assert hasattr(rtx, s), s
    listed, missing = ra.exported_symbols()
    assert not missing and listed == list(ra.RTX_SYMBOLS)


def test_c_entry_refuses_a_null_scene(ra):
    rtx, _ = ra.load()
    assert rtx.rtx_render_aov(None, 0, 8, None, None) == -1      # RTX_ERR_ARG
    assert b"NULL" in rtx.rtx_last_error()


def test_bad_buffers_are_refused_before_the_gpu(ra):
    torch = pytest.importorskip("torch")
    s = ra.Scene("scenes/cfg1_simple_shapes.scene", 32, 24)
    z = lambda shape, dt=torch.float32: torch.zeros(shape, dtype=dt)
    cases = [
        (dict(), "at least one buffer"),
        (dict(depth=np.zeros((24, 32), np.float32)), "depth must be a torch tensor"),
        (dict(depth=z((24, 32), torch.float64)), "depth must be float32"),
        (dict(object_id=z((24, 32))), "object_id must be int32"),
        (dict(triangle_id=z((24, 32), torch.int64)), "triangle_id must be int32"),
        (dict(depth=z((32, 24))), r"depth must have shape \(24, 32\)"),
        (dict(uv=z((24, 32, 3))), r"uv must have shape \(24, 32, 2\)"),
        (dict(normal=z((24, 32))), r"normal must have shape \(24, 32, 3\)"),
        (dict(albedo=z((24 * 32, 3))), r"albedo must have shape \(24, 32, 3\)"),
        (dict(depth=z((32, 24)).t()), "depth must be contiguous"),
        (dict(normal=z((24, 32, 6))[..., ::2]), "normal must be contiguous"),
        (dict(depth=z((24, 32))), "depth must be on cuda:0"),
        (dict(depth=None, albedo=z((24, 32, 3))), "albedo must be on cuda:0"),
    ]
    for kw, what in cases:
        with pytest.raises(ValueError, match=what):
            s.render_aov(**kw)
    assert s._gpu is None              # (the scene was never flattened and uploaded: no GPU call was made)
    s.close()


@pytest.mark.parametrize("name,size,share", [("cfg4_textured_256", (40, 24), 0.44), ("mixed_materials", (24, 40), 1.00),
                                             ("cfg3_reflective_refractive", (33, 17), 0.43)])
def test_primary_rays_reproduce_pass1(oracle, name, size, share):
    w, h = size
    o = oracle.OracleScene("scenes/%s.scene" % name, w, h)
    e = U.expected(o, open(os.path.join(ROOT, "scenes", name + ".scene")).read())
    p1 = o.pass1()
    m = U.written_mask(w, h)
    assert np.array_equal(U.bits(e["shaded"])[m], U.bits(p1)[m])
    assert round(float(e["hit"].mean()), 2) == share
    miss = ~e["hit"]
    if miss.any():
        assert (U.bits(e["depth"])[miss] == U.FLT_MAX_BITS).all() and (e["object_id"][miss] == -1).all() and (e["triangle_id"][miss] == -1).all()
        assert (e["uv"][miss] == -1).all()
    assert (U.bits(e["normal_colour"]) != U.bits(e["shaded"])).any()
    o.close()


@pytest.mark.parametrize("cull", [1, 0])
@pytest.mark.parametrize("name", U.REPO_SCENES + U.FAMILY_SCENES)
def test_inputs_of_the_gpu_tests_are_not_trivial(oracle, family, name, cull):
    w, h = U.size_of(name)
    path = path_of(name, family)
    e = U.expected_of(path, w, h, cull)
    m = U.written_mask(w, h)
    hit = e["hit"][m]
    ids = np.unique(e["object_id"][m])
    if (name, cull) == ("cfg4_textured_256", 0):
        # its one object surrounds the camera: without culling every ray meets the inside of the torus.  With culling (the scene's own
        # setting, the other case of this test) it has both hits and misses.
        assert hit.all() and ids.tolist() == [0]
    elif name == "mixed_materials":
        assert hit.all() and len(ids) >= 2
    else:
        assert hit.any() and not hit.all() and len(ids) >= 2          # (ids of the channel: -1 counts)
    print("%s %dx%d cull %d: %.2f hit, objects %s" % (name, w, h, cull, hit.mean(), ids.tolist()))
    if name in S.NORMAL_MAPPED:
        o = oracle.OracleScene(path, w, h)
        oracle.lib().orc_set_flag(o.h, b"useBackfaceCulling", cull)
        plain, mesh = U.vertex_normal_colour(o, e)
        o.close()
        turned = (np.abs(plain - e["normal_colour"]) > 1e-3).any(-1) & mesh & m
        assert turned.sum() > 0.01 * (mesh & m).sum()
    if name == "cfg4_textured_256":
        texels = np.unique(U.bits(e["albedo"])[m & e["hit"]], axis=0)
        assert len(texels) > 16
