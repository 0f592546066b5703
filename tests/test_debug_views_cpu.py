"""The two debug views of the reference (showNormals, showAC) without a GPU: the per-scene flags of the host, our numpy restatement
of the heat map (tests/ac_heatmap.py) against the committed goldens (tests/golden/debug_*.npz, tools/make_golden_debug_views.py),
and -- where oracle/_ref is built -- the goldens against a fresh run of the reference."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import ac_heatmap as A
from tools.make_golden_debug_views import HEATMAP, NORMALS, key, load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_BIN = os.path.join(ROOT, "oracle", "_ref", "render_ref")


@pytest.fixture(scope="module")
def gold():
    return load()


def test_show_normals_is_a_view_flag_per_scene(ra, tmp_path):
    s = ra.Scene(A.scene_copy("cfg2_smooth_4k", str(tmp_path), {"showNormals": 1}), 64, 48)
    t = ra.Scene("scenes/cfg2_smooth_4k.scene", 64, 48)
    assert s.view_flags() & 4
    assert not t.view_flags() & 4                     # loading another scene does not change the first one's flags
    assert s.view_flags() & 4
    s.set_flag("showNormals", 0)
    assert not s.view_flags() & 4
    t.set_flag("showNormals", 1)
    assert t.view_flags() & 4 and not s.view_flags() & 4
    assert t.view_flags() & 3 == s.view_flags() & 3   # culling / skybox bits untouched
    s.set_flag("showAC", 1)                           # (the heat map is not a flag of the view: Scene::render picks rtx_render_ac)
    assert not s.view_flags() & 4


@pytest.mark.parametrize("name,w,h,extra", HEATMAP, ids=[key("ac", n, e) for n, w, h, e in HEATMAP])
def test_restated_heatmap_equals_golden_bmp(ra, gold, tmp_path, name, w, h, extra):
    from rendering_amd import assets
    if "250k" in name:
        assets.ensure(["bumpy_250k.obj"])
    s = ra.Scene(A.scene_copy(name, str(tmp_path), dict(extra, showAC=1)), w, h)
    c = A.counts(s)
    if name == "cfg1_simple_shapes":
        assert c.max() == 0                           # no mesh: 0 / 0 = NaN in every pixel
    bmp = A.quantize_bmp(A.frame(c, w, h), w, h)
    k = key("ac", name, extra)
    assert bmp == gold[k + "__bmp"].tobytes()
    assert hashlib.md5(bmp).hexdigest() == str(gold[k + "__md5"])


def test_ac_penalty_changes_the_heatmap(gold):
    a = key("ac", "cfg2_smooth_250k", {"ac_penalty": 1}); b = key("ac", "cfg2_smooth_250k", {"ac_penalty": 10})
    assert str(gold[a + "__md5"]) != str(gold[b + "__md5"])


def test_restated_count_walk_on_a_tiny_tree():
    """recCountAC by hand: root (passes) -> left leaf (passes), right inner (fails: its children are never tested)."""
    bvh = dict(bounds=np.array([[-1, -1, -2, 1, 1, 0], [-1, -1, -2, 1, 1, 0], [5, 5, -2, 6, 6, 0], [5, 5, -2, 6, 6, 0], [-1, -1, -2, 1, 1, 0]], np.float32),
               skip=np.array([5, 2, 5, 4, 5], np.int32), leaf_count=np.array([-1, 1, -1, 1, 1], np.int32))
    o = np.array([[0, 0, 0], [0, 0, 5]], np.float32)
    d = np.array([[0, 0, -1], [1, 0, 0]], np.float32)      # (zero components: 1 / 0 = inf in the slab products, as in the reference)
    assert list(A.count_mesh(bvh, o, d)) == [2, 0]


needs_ref = pytest.mark.skipif(not os.path.exists(REF_BIN), reason="oracle/_ref (the reference build) is not present")


@needs_ref
@pytest.mark.parametrize("name,w,h,extra", [e for e in HEATMAP if "250k" not in e[0]], ids=[key("ac", n, e) for n, w, h, e in HEATMAP if "250k" not in n])
def test_heatmap_golden_equals_fresh_reference(gold, tmp_path, name, w, h, extra):
    from tools.make_golden_debug_views import heatmap_run
    bmp = heatmap_run(name, w, h, extra, str(tmp_path))
    assert hashlib.md5(bmp).hexdigest() == str(gold[key("ac", name, extra) + "__md5"])


@needs_ref
# (not the normal-map scene: the reference normalises its normal map in place at every sample, so its own runs differ -- tests/test_gpu_debug_views.py)
@pytest.mark.parametrize("name,w,h,extra", [NORMALS[1], NORMALS[5], NORMALS[7]], ids=["cfg2", "area_light", "mixed_culling_off"])
def test_normals_golden_equals_fresh_reference(gold, tmp_path, name, w, h, extra):
    f = str(tmp_path / "n.npz")
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_golden_debug_views.py"), "--normals", name, str(w), str(h), repr(extra), f],
                   cwd=ROOT, check=True)
    g = np.load(f)
    k = key("normals", name, extra)
    assert np.array_equal(g["pass1"].view(np.uint32), gold[k + "__pass1"].view(np.uint32))
    assert np.array_equal(g["probe_colours"].view(np.uint32), gold[k + "__probe_colours"].view(np.uint32))
    d = (g["ssaa"].view(np.uint32) != gold[k + "__ssaa"].view(np.uint32)).any(-1)
    d[0, :] = False; d[:, 0] = False                  # uninitialised Sobel border in the reference
    assert not d.any()
