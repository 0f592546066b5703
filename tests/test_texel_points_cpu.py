"""rtx_texel_points and rtx_dilate_texels (Scene.texel_points, dilate_texels, bake_light; include/rtx_bake.h) without a GPU: the header against
the symbol list and the binding, and the properties of tests/util_texel_points' restatement that the GPU tests rely on, on the restatement
alone.

The tie condition.  torus_obj writes its texture coordinates with six decimals, so only grids of dyadic steps are exact: at 8 x 6 over
torus_obj(8, 6) the rows j = 0, 1, 3, 4 have v = 0.166667 ... and their centres lie beside the diagonals, not on them (24 of the 48 texels are
owned by the odd triangle).  The exact ties are therefore checked on torus_obj(8, 4) at 8 x 4, where every coordinate and every centre is a
dyadic fraction; 8 x 6 stays among the sizes that must be covered and round-trip."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from rendering_amd import assets
from tests import util_texel_points as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def test_bake_header_and_symbol_list(ra):
    hdr = open(os.path.join(ROOT, "include", "rtx_bake.h")).read()
    declared = re.findall(r"^int\s+(rtx_[a-z0-9_]+)\s*\(", hdr, re.M)
    assert declared == list(ra.RTX_BAKE_SYMBOLS) == ["rtx_texel_points", "rtx_dilate_texels"]
    others = [n for n in dir(ra) if re.fullmatch(r"RTX_[A-Z_]*SYMBOLS", n) and n != "RTX_BAKE_SYMBOLS"]
    assert len(others) >= 15
    for other in others:
        assert not set(declared) & set(getattr(ra, other)), other
    rtx, _ = ra.load()
    for s in declared:
        assert hasattr(rtx, s), s
    listed, missing = ra.exported_symbols()
    assert not missing and listed == list(ra.RTX_SYMBOLS)
    src = open(os.path.join(ROOT, "rendering_amd", "__init__.py")).read()
    assert "RTX_BAKE_SYMBOLS" in re.search(r"def exported_symbols\(\):.*?return", src, re.S).group(0)
    # the structure of the binding is the header's
    body = re.search(r"typedef struct rtx_texel_buffers \{(.*?)\} rtx_texel_buffers;", hdr, re.S).group(1)
    fields = re.findall(r"(float\*|int32_t\*)\s+(\w+);", body)
    assert fields == [("float*", "points_dev"), ("int32_t*", "tri_dev"), ("float*", "bary_dev")]
    assert [n for n, _ in ra.TexelBuffers._fields_] == [n for _, n in fields]
    assert [t for _, t in ra.TexelBuffers._fields_] == [C.c_void_p] * 3
    for name in ("texel_points", "dilate_texels", "bake_light"):
        assert callable(getattr(ra.Scene, name))


def test_c_entries_refuse_a_null_scene(ra):
    rtx, _ = ra.load()
    buf = ra.TexelBuffers()
    assert rtx.rtx_texel_points(None, 0, 4, 4, C.byref(buf), None) == -1      # RTX_ERR_ARG
    assert b"NULL" in rtx.rtx_last_error()
    assert rtx.rtx_texel_points(None, 0, 4, 4, None, None) == -1
    assert rtx.rtx_dilate_texels(None, 4, 4, 3, None, None, 1, None) == -1
    assert b"NULL" in rtx.rtx_last_error()


def test_wrapper_refusals_before_the_gpu(ra, tmp_path):
    torch = pytest.importorskip("torch")
    s = ra.Scene(U.write_mesh_scene(tmp_path, "quad", U.quad_obj()), 32, 24)
    with pytest.raises(ValueError, match="texel_points: nothing to compute"):
        s.texel_points(0, 8, 8, points=False, tri=False)
    with pytest.raises(ValueError, match="no diffuse map, and no size is given"):
        s.texel_points(0)
    with pytest.raises(ValueError, match="width and height go together"):
        s.texel_points(0, 8)
    with pytest.raises(ValueError, match="must be positive"):
        s.texel_points(0, 0, 8)
    with pytest.raises(ValueError, match="must be positive"):
        s.texel_points(0, 1 << 16, 1 << 16)
    with pytest.raises(ValueError, match="out of range"):
        s.texel_points(3, 8, 8)
    with pytest.raises(ValueError, match="dilate_texels: tri must be int32"):
        s.dilate_texels(torch.zeros((4, 4, 3)), torch.zeros((4, 4)))
    s.close()


# ---- the restatement's own properties ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def toruses(ra, tmp_path_factory):
    d = tmp_path_factory.mktemp("texel_cpu")
    out = {}
    for nu, nv in ((8, 6), (8, 4), (64, 48)):
        s = ra.Scene(U.write_mesh_scene(d, "torus_%d_%d" % (nu, nv), assets.torus_obj(nu, nv)), 32, 24)
        out[nu, nv] = U.triangles(s)
        s.close()
    return out


@pytest.mark.parametrize("mesh,w,h", [((8, 6), 16, 12), ((8, 6), 37, 21), ((8, 6), 8, 6), ((8, 6), 1, 1), ((8, 4), 8, 4), ((64, 48), 16, 16)])
def test_every_texel_of_a_tiling_layout_is_covered_and_round_trips(toruses, mesh, w, h):
    tri_pos, tri_nrm, tri_uv = toruses[mesh]
    r = U.texel_points_ref(tri_pos, tri_nrm, tri_uv, w, h)
    assert (r["tri"] >= 0).all(), "uncovered texels: %s" % np.argwhere(r["tri"] < 0)[:4]
    assert r["tri"].max() < tri_uv.shape[0]
    # the sampler's rule reads the texel the point was made for: (int)(W * texCoord.x) == i, (int)(H * texCoord.y) == j
    tc = U.tex_coord(tri_uv, r["tri"], r["bary"])
    jj, ii = np.nonzero(r["tri"] >= 0)
    assert np.array_equal((f32(w) * tc[:, 0]).astype(np.int32), ii) and np.array_equal((f32(h) * tc[:, 1]).astype(np.int32), jj)


def test_exact_ties_go_to_the_lower_index(toruses):
    tri_pos, tri_nrm, tri_uv = toruses[8, 4]
    w, h = 8, 4
    cx, cy = np.meshgrid(U.centres(w), U.centres(h))
    n_cover = np.zeros((h, w), int)
    lowest = np.full((h, w), 1 << 30)
    for t in range(tri_uv.shape[0]):
        c = U.covers(*U.weights(tri_uv[t], cx, cy))
        n_cover += c
        lowest = np.where(c, np.minimum(lowest, t), lowest)
    assert (n_cover == 2).all(), "every centre lies on its quad's diagonal: both triangles cover it"
    r = U.texel_points_ref(tri_pos, tri_nrm, tri_uv, w, h)
    assert np.array_equal(r["tri"], lowest) and (r["tri"] % 2 == 0).all()
    # on the diagonal one barycentric weight is exactly zero: the point lies on the shared edge
    k = (f32(1) - r["bary"][..., 0]) - r["bary"][..., 1]
    assert ((r["bary"][..., 0] == 0) | (r["bary"][..., 1] == 0) | (k == 0)).all()


def test_shared_edges_are_watertight_in_magnitude():
    """Two triangles that share an edge evaluate it to the same magnitude with opposite signs, whatever the corners' order."""
    rng = np.random.RandomState(3)
    cx, cy = np.meshgrid(U.centres(37), U.centres(21))
    for _ in range(50):
        p, q = rng.uniform(-0.2, 1.2, 2).astype(f32), rng.uniform(-0.2, 1.2, 2).astype(f32)
        a, b = U.edge(p[0], p[1], q[0], q[1], cx, cy), U.edge(q[0], q[1], p[0], p[1], cx, cy)
        assert np.array_equal(a, -b)


def test_uncovered_texels_are_minus_one_and_zero(ra, tmp_path):
    s = ra.Scene(U.write_mesh_scene(tmp_path, "charts", U.charts_obj()), 32, 24)
    tri_pos, tri_nrm, tri_uv = U.triangles(s)
    s.close()
    assert np.isnan(tri_uv[6, 0]) and tri_uv.shape == (8, 6)
    r = U.texel_points_ref(tri_pos, tri_nrm, tri_uv, 37, 21)
    none = r["tri"] < 0
    assert none.any() and not U.bits(r["points"].reshape(21, 37, 6)[none]).any() and not U.bits(r["bary"][none]).any()
    assert not np.isin(r["tri"], U.CHART_NEVER).any()
    assert set(np.unique(r["tri"])) >= {-1, 0, 1, 2, 7}


# ---- the dilation's restatement ---------------------------------------------------------------------------------------------------------
def test_dilation_grows_by_the_stated_neighbourhood():
    w, h = 7, 5
    tri = np.full((h, w), -1, np.int32)
    tri[2, 3] = 5
    img = np.zeros((h, w, 3), f32)
    img[2, 3] = (1, 2, 3)
    for passes in (0, 1, 2, 3):
        out, t = U.dilate_ref(img, tri, passes)
        jj, ii = np.mgrid[0:h, 0:w]
        reach = np.maximum(abs(jj - 2), abs(ii - 3))      # (eight neighbours: the Chebyshev distance)
        assert np.array_equal(t == -2, (reach >= 1) & (reach <= passes)) and t[2, 3] == 5 and np.array_equal(t == -1, reach > passes)
        assert (out[reach <= passes] == (1, 2, 3)).all() and not out[reach > passes].any()


def test_dilation_takes_the_first_neighbour_in_the_fixed_order():
    w, h = 5, 5
    base = np.full((h, w), -1, np.int32)
    # every pair of neighbours of the centre texel: the earlier one in the order wins
    for a in range(8):
        for b in range(a + 1, 8):
            tri, img = base.copy(), np.zeros((h, w), f32)
            for k in (a, b):
                di, dj = U.NEIGHBOURS[k]
                tri[2 + dj, 2 + di] = k
                img[2 + dj, 2 + di] = 10 + k
            out, t = U.dilate_ref(img, tri, 1)
            assert out[2, 2] == 10 + a and t[2, 2] == -2


def test_dilation_reads_nothing_written_in_the_same_pass():
    w, h = 6, 1
    tri = np.array([[0, -1, -1, -1, -1, -1]], np.int32)
    img = np.array([[7, 0, 0, 0, 0, 0]], f32)
    out, t = U.dilate_ref(img, tri, 1)
    assert list(out[0]) == [7, 7, 0, 0, 0, 0] and list(t[0]) == [0, -2, -1, -1, -1, -1]
    out, t = U.dilate_ref(img, tri, 3)
    assert list(out[0]) == [7, 7, 7, 7, 0, 0] and list(t[0]) == [0, -2, -2, -2, -1, -1]
