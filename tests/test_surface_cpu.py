"""rtx_surface_rays / Scene.surface_rays without a GPU: the extension header and its symbol list, the argument checks, and the inputs of
the GPU tests (tests/test_gpu_surface.py) shown to be non-trivial with the oracle alone: the bounce rays hit and miss in fair shares and
reach the meshes, the probe rays hit and miss, and on the family scenes the rays reach the normal-mapped meshes and many texels of every
specular map."""
import os
import re

import numpy as np
import pytest

from tests import util_aov as U
from tests import util_shading as S
from tests import util_surface as SU

ROOT = U.ROOT
f32 = np.float32


@pytest.fixture(scope="module")
def family(tmp_path_factory):
    d = S.short_dir(tmp_path_factory)
    return d, S.write_family(d)


def path_of(name, family):
    return family[1][name] if name in S.FAMILY else "scenes/%s.scene" % name


def test_surface_header_and_symbol_list(ra):
    hdr = open(os.path.join(ROOT, "include", "rtx_surface.h")).read()
    declared = set(re.findall(r"\b(rtx_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(ra.RTX_SURFACE_SYMBOLS) and len(ra.RTX_SURFACE_SYMBOLS) == len(declared)
    for other in (ra.RTX_SYMBOLS, ra.RTX_EDIT_SYMBOLS, ra.RTX_QUERY_SYMBOLS, ra.RTX_AOV_SYMBOLS, ra.RTX_AO_SYMBOLS):
        assert not declared & set(other)
    rtx, _ = ra.load()
    for s in declared:
        assert hasattr(rtx, s), s
    listed, missing = ra.exported_symbols()
    assert not missing and listed == list(ra.RTX_SYMBOLS)
    # the structure of the binding is the header's: five pointers in its order
    fields = re.findall(r"float\*\s+(\w+_dev);", hdr)
    assert fields == [n for n, _ in ra.SurfaceBuffers._fields_] and len(fields) == 5


def test_c_entry_refuses_a_null_scene(ra):
    rtx, _ = ra.load()
    assert rtx.rtx_surface_rays(None, 4, None, None, None) == -1      # RTX_ERR_ARG
    assert b"NULL" in rtx.rtx_last_error()


def test_bad_arguments_are_refused_before_the_gpu(ra):
    torch = pytest.importorskip("torch")
    s = ra.Scene("scenes/cfg1_simple_shapes.scene", 32, 24)
    z = lambda shape, dt=torch.float32: torch.zeros(shape, dtype=dt)
    cases = [
        (dict(rays=z((4, 6)), normal=False, albedo=False), "surface_rays: nothing to compute"),
        (dict(rays=np.zeros((4, 6), np.float32)), "surface_rays: rays must be a torch tensor"),
        (dict(rays=z((4, 6), torch.float64)), "surface_rays: rays must be float32"),
        (dict(rays=z((6, 4))), r"surface_rays: rays must have shape \(n, 6\)"),
        (dict(rays=z((24,))), r"surface_rays: rays must have shape \(n, 6\)"),
        (dict(rays=z((4, 12))[:, ::2]), "surface_rays: rays must be contiguous"),
        (dict(rays=z((4, 6))), "surface_rays: rays must be on cuda:0"),
    ]
    for kw, what in cases:
        with pytest.raises(ValueError, match=what):
            s.surface_rays(**kw)
    assert s._gpu is None              # (the scene was never flattened and uploaded: no GPU call was made)
    s.close()


def mesh_objects(path):
    text = open(path if os.path.isabs(path) else os.path.join(ROOT, path)).read()
    return [k for k, b in enumerate(SU.object_blocks(text)) if b.get("type") == "mesh"]


# (B): more than 1 000 rays per scene, hit share within [0.10, 0.60], at least 40 mesh hits where there is a mesh.  What the oracle gives
# (culling on / off): coincident 0.241 / 0.250, cfg2_smooth_4k 0.457, cfg4_textured_256 0.369 / 0.396, area_light 0.413 / 0.414,
# cfg3_reflective_refractive 0.130, cfg1_simple_shapes 0.279, mixed_materials 0.149 / 0.156, the family scenes 0.16 - 0.30.
@pytest.mark.parametrize("cull", [1, 0])
@pytest.mark.parametrize("name", SU.SCENES)
def test_bounce_rays_hit_and_miss(oracle, family, name, cull):
    path = path_of(name, family)
    w, h = SU.size_of(name)
    rays = SU.oracle_bounce_rays(oracle, path, w, h, cull)
    exp = SU.expected_of(path, w, h, cull, rays)
    share = exp["hit"].mean()
    meshes = mesh_objects(path)
    on_mesh = int(np.isin(exp["object_id"], meshes).sum())
    print("%s %dx%d cull %d: %d bounce rays, hit share %.3f, %d mesh hits" % (name, w, h, cull, len(rays), share, on_mesh))
    assert len(rays) > 1000
    assert 0.10 <= share <= 0.60
    if meshes:
        assert on_mesh >= 40


# (D): hit share at least 0.4; at least 0.3 misses on every scene but mixed_materials, which has none
@pytest.mark.parametrize("cull", [1, 0])
@pytest.mark.parametrize("name", SU.SCENES)
def test_probe_rays_hit_and_miss(family, name, cull):
    path = path_of(name, family)
    w, h = SU.size_of(name)
    exp = SU.expected_of(path, w, h, cull, SU.probe_rays())
    share = exp["hit"].mean()
    print("%s cull %d: probe rays' hit share %.3f" % (name, cull, share))
    assert share >= 0.4
    if name == "mixed_materials":
        assert share == 1.0
    else:
        assert 1 - share >= 0.3


# the family scenes with normal maps: (A) and (B) each reach at least 30 hits on a normal-mapped mesh and at least 30 distinct texels of
# every specular map of the scene
@pytest.mark.parametrize("cull", [1, 0])
@pytest.mark.parametrize("name", SU.MAPPED)
def test_rays_reach_the_maps(oracle, family, name, cull):
    path = path_of(name, family)
    w, h = SU.size_of(name)
    o = oracle.OracleScene(path, w, h)
    cam = U.primary_rays(o)
    o.close()
    for what, rays in (("A", cam), ("B", SU.oracle_bounce_rays(oracle, path, w, h, cull))):
        exp = SU.expected_of(path, w, h, cull, rays)
        print("%s %dx%d cull %d (%s): hits per normal-mapped mesh %s, texels per specular map %s" % (
            name, w, h, cull, what, exp["normal_hits"], exp["spec_texels"]))
        assert exp["normal_hits"] and max(exp["normal_hits"].values()) >= 30
        assert exp["spec_texels"] and min(exp["spec_texels"].values()) >= 30
        # the maps decide values: the specular channel is neither constant nor the objects' default at those hits
        sel = np.isin(exp["object_id"], list(exp["spec_texels"]))
        assert len(np.unique(exp["specular"][sel])) >= 30
