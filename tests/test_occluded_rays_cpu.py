"""rtx_occluded_rays / Scene.occluded without a GPU: the extension header and its symbol list, the argument checks, and the inputs of
the GPU tests (tests/test_gpu_occluded_rays.py) checked against the oracle alone -- the scene without its transparent objects differs
where it must, and the expected bits are neither all 0 nor all 1."""
import os
import re

import numpy as np
import pytest

from tests.util_occlusion import ROOT, expected, opaque_probe, opaque_scene, tmax_mix
from tests.util_rays import probe_rays

WITH_GLASS = ["mixed_materials", "cfg1_simple_shapes", "cfg3_reflective_refractive", "area_light"]
WITHOUT = ["coincident", "cfg2_smooth_4k", "cfg4_textured_256"]


def test_query_header_and_symbol_list(ra):
    hdr = open(os.path.join(ROOT, "include", "rtx_query.h")).read()
    declared = set(re.findall(r"\b(rtx_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(ra.RTX_QUERY_SYMBOLS) and len(ra.RTX_QUERY_SYMBOLS) == len(declared)
    assert not declared & set(ra.RTX_SYMBOLS) and not declared & set(ra.RTX_EDIT_SYMBOLS)
    rtx, _ = ra.load()
    for s in declared:
        assert hasattr(rtx, s), s
    listed, missing = ra.exported_symbols()
    assert not missing and listed == list(ra.RTX_SYMBOLS)


def test_c_entry_refuses_a_null_scene(ra):
    rtx, _ = ra.load()
    assert rtx.rtx_occluded_rays(None, 4, None, None, None, None) == -1      # RTX_ERR_ARG
    assert b"NULL" in rtx.rtx_last_error()


def test_bad_arguments_are_refused_before_the_gpu(ra):
    torch = pytest.importorskip("torch")
    s = ra.Scene("scenes/cfg1_simple_shapes.scene", 32, 32)
    for rays, what in (([[0.0] * 6], "torch tensor"), (torch.zeros((4, 6), dtype=torch.float64), "float32"),
                       (torch.zeros((4, 5), dtype=torch.float32), r"shape \(n, 6\)"), (torch.zeros((6, 8), dtype=torch.float32).t(), "contiguous"),
                       (torch.zeros((4, 6), dtype=torch.float32), "cuda:0")):
        with pytest.raises(ValueError, match=what):
            s.occluded(rays)
    assert s._gpu is None
    s.close()


@pytest.mark.parametrize("name", WITH_GLASS + WITHOUT)
def test_opaque_scene_drops_exactly_the_transparent_objects(oracle, tmp_path, name):
    path = "scenes/%s.scene" % name
    p, dropped = opaque_scene(path, tmp_path)
    a, b = oracle.OracleScene(path, 64, 64), oracle.OracleScene(p, 64, 64)
    assert dropped == (1 if name in WITH_GLASS else 0)
    assert b.n_objects == a.n_objects - dropped and b.n_lights == a.n_lights
    rays = probe_rays(4096)
    ha, hb = a.probe(rays)[0], b.probe(rays)[0]
    # the object index shifts behind the dropped block: compare what does not (hit, t)
    differ = (ha[:, 0] != hb[:, 0]) | (ha[:, 3].view(np.uint32) != hb[:, 3].view(np.uint32))
    print("%s: %.1f %% of the rays have another nearest hit without the transparent objects" % (name, 100.0 * differ.mean()))
    if name in WITH_GLASS:
        assert differ.mean() > 0.01      # "transparent objects do not occlude" is a statement the GPU test can fail
    else:
        assert open(p).read() == open(os.path.join(ROOT, path)).read() and not differ.any()
    a.close(); b.close()


@pytest.mark.parametrize("name", WITH_GLASS + WITHOUT)
def test_expected_bits_are_not_trivial(oracle, tmp_path, name):
    rays = probe_rays(4096)
    hit, t = opaque_probe(oracle, "scenes/%s.scene" % name, tmp_path, rays)
    share = expected(hit, t, tmax_mix(hit, t)).mean()
    print("%s: %.2f of the rays occluded under the seeded mix of ranges (%.2f hit something)" % (name, share, hit.mean()))
    assert 0.05 <= share <= 0.95
    # the edge ranges: nothing is below 0, -1 or NaN; +inf and FLT_MAX are the whole ray
    for v in (0.0, -1.0, np.nan):
        assert not expected(hit, t, np.float32(v)).any()
    assert np.array_equal(expected(hit, t, np.float32(np.inf)), hit.astype(np.uint8))
