"""Scene.set_vertices without a GPU: new vertices (and raw normals) for a mesh of a loaded scene give, bit for bit, the triangles, the
acceleration structure and the object records of a fresh load of the scene whose mesh reads the OBJ file rewritten with those v / vn lines.
The functions the device kernels run (rendering_amd/csrc/rtx_place.h) are pinned to the loader's Mesh::place through rtx_place_probe on
the CPU: every fit branch, the loader's quirks, the NaN a zero uv determinant creates."""
import os
import re

import numpy as np
import pytest

from tests.util_deform import bits, bulge, deformed_scene, quirk_scene, scale, twist
from tests.util_move import edit_scene, same_structure

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# scene -> the mesh objects deformed
MESHES = {"mixed_materials": (0, 1, 2), "cfg4_textured_256": (0,)}
MOVE = dict(pos=(0.2, -0.4, -3.8), rot=(25, -40, 10), size=(1.4, 2.2, 1.7))


def assert_same(g, f, idx, what):
    assert np.array_equal(bits(g.digest()), bits(f.digest())), "%s: object records differ" % what
    k = same_structure(g.bvh(idx), f.bvh(idx))
    assert k is None, "%s: object %d, %s differs from a fresh load" % (what, idx, k)


def steps_for(P0, flat):
    """Deformations in a row; the flat quad keeps its flat axis at 0 for the first two (range = FLT_MIN) and leaves it with the third."""
    a = scale(P0, (1.3, 1.0 if flat else 0.7, 1.1))
    b = twist(a, 0.8)
    c = bulge(b, 0.15, 3.0)
    return [a, b, c]


@pytest.mark.parametrize("name,idx", [(n, i) for n in sorted(MESHES) for i in MESHES[n]])
def test_set_vertices_equals_a_fresh_load_of_the_rewritten_obj(ra, tmp_path, name, idx):
    text = open(os.path.join(ROOT, "scenes", name + ".scene")).read()
    g = ra.Scene("scenes/%s.scene" % name, 64, 48)
    first, first_digest = g.bvh(idx), g.digest()
    P0, N0 = g.mesh_vertices(idx)
    assert P0.shape[0] > 0 and P0.dtype == np.float32
    flat = bool((P0[:, 1] == 0).all())
    pose0 = {k: g.mesh_pose(idx)[k] for k in ("pos", "rot", "size")}
    steps = steps_for(P0, flat)
    for step, V in enumerate(steps):
        g.set_vertices(idx, V)
        if step == 1:      # a move between two deformations: the rewritten OBJ with the edited block
            g.move_object(idx, **MOVE)
            text = edit_scene(text, idx, **MOVE)
        f, _ = deformed_scene(ra, tmp_path, text, idx, V, None, "%s_%d_%d" % (name, idx, step))
        assert_same(g, f, idx, "%s object %d step %d" % (name, idx, step))
        Pg, Ng = g.mesh_vertices(idx)
        assert np.array_equal(bits(Pg), bits(V)) and np.array_equal(bits(Ng), bits(N0))
        f.close()
    # back to the first vertices and the first placement: the first load's structures again
    g.move_object(idx, **pose0)
    g.set_vertices(idx, P0)
    assert np.array_equal(bits(g.digest()), bits(first_digest))
    assert same_structure(g.bvh(idx), first) is None
    g.close()


@pytest.mark.parametrize("name,idx", [("mixed_materials", 1), ("cfg4_textured_256", 0)])
def test_raw_normals_are_normalised_as_the_loader_does(ra, tmp_path, name, idx):
    text = open(os.path.join(ROOT, "scenes", name + ".scene")).read()
    g = ra.Scene("scenes/%s.scene" % name, 64, 48)
    P0, N0 = g.mesh_vertices(idx)
    raw = (twist(N0, 0.5) * np.float32(3)).astype(np.float32)
    raw[7] = 0      # a zero vector stays zero
    V = bulge(P0, 0.1, 2.0)
    g.set_vertices(idx, V, raw)
    f, _ = deformed_scene(ra, tmp_path, text, idx, V, raw, "%s_nrm" % name)
    assert_same(g, f, idx, "%s with normals" % name)
    assert np.array_equal(bits(g.mesh_vertices(idx)[1]), bits(f.mesh_vertices(idx)[1]))
    assert not g.mesh_vertices(idx)[1][7].any()
    f.close()
    # normals = None keeps them: only the vertices change
    V2 = scale(V, (0.9, 1.2, 1.0))
    g.set_vertices(idx, V2)
    f, _ = deformed_scene(ra, tmp_path, text, idx, V2, raw, "%s_nrm_kept" % name)
    assert_same(g, f, idx, "%s, normals kept" % name)
    f.close()
    g.close()


def probe_equals_bvh(ra, g, idx, V, N, f, what, device=-1):
    """rtx_place_probe on g's topology, stored normals and pose with the vertices V (raw normals N) against the fresh load f"""
    r = ra.place_probe(g.mesh_topology(idx), g.mesh_vertices(idx)[1], V, N, g.mesh_pose(idx), device=device)
    b = f.bvh(idx)
    assert not r["bad_input"] and not r["bad_placed"]
    for key, cols in (("pos", slice(0, 9)), ("nrm", slice(9, 18)), ("tb", slice(24, 30))):
        assert np.array_equal(bits(r[key]), bits(b["tris"][:, cols])), "%s: %s differs from Mesh::place" % (what, key)
    assert np.array_equal(bits(r["root_lo"]), bits(b["bounds"][0, 0:3])) and np.array_equal(bits(r["root_hi"]), bits(b["bounds"][0, 3:6])), what
    return r


# sizes that make each of x, y, z the tightest stretch of the torus (its y range is the smallest)
FIT_SIZES = {0: (0.5, 5.0, 5.0), 1: (5.0, 0.2, 5.0), 2: (5.0, 5.0, 0.5)}


@pytest.mark.parametrize("axis", sorted(FIT_SIZES))
def test_the_shared_formulas_equal_mesh_place_in_every_fit_branch(ra, tmp_path, axis):
    name, idx = "cfg4_textured_256", 0
    text = open(os.path.join(ROOT, "scenes", name + ".scene")).read()
    g = ra.Scene("scenes/%s.scene" % name, 64, 48)
    P0, N0 = g.mesh_vertices(idx)
    V = bulge(twist(P0, 0.4), 0.1, 2.5)
    keys = dict(size=FIT_SIZES[axis], rot=(12, 100, -33))
    rng = V.max(0) - V.min(0)
    assert int(np.argmin(np.float32(FIT_SIZES[axis]) / rng)) == axis, "the sizes do not take the branch of axis %d" % axis
    g.move_object(idx, **keys)
    text = edit_scene(text, idx, **keys)
    raw = (N0 * np.float32(2)).astype(np.float32)
    for N, tag in ((None, "kept"), (raw, "raw")):
        f, _ = deformed_scene(ra, tmp_path, text, idx, V, N, "fit_%d_%s" % (axis, tag))
        probe_equals_bvh(ra, g, idx, V, N, f, "fit branch %d, normals %s" % (axis, tag))
        f.close()
    g.close()


@pytest.mark.parametrize("name,idx", [("mixed_materials", 0), ("mixed_materials", 1)])
def test_the_shared_formulas_on_the_flat_quad_and_the_rotated_mesh(ra, tmp_path, name, idx):
    text = open(os.path.join(ROOT, "scenes", name + ".scene")).read()
    g = ra.Scene("scenes/%s.scene" % name, 64, 48)
    P0, _ = g.mesh_vertices(idx)
    V = twist(scale(P0, (1.2, 1.0, 0.8)), 0.6)
    f, _ = deformed_scene(ra, tmp_path, text, idx, V, None, "probe_%d" % idx)
    r = probe_equals_bvh(ra, g, idx, V, None, f, "%s object %d" % (name, idx))
    if idx == 0:      # the flat axis: lo = 0, hi = FLT_MIN
        assert r["obj_lo"][1] == 0 and bits(r["obj_hi"])[1] == 0x00800000
    f.close(); g.close()


def quirk(ra, tmp_path, name, V=None, N=None, **kw):
    text, obj = quirk_scene(tmp_path, name, **kw)
    p = tmp_path / ("%s.scene" % name)
    p.write_text(text)
    g = ra.Scene(str(p), 64, 48)
    return g, text


def test_vertices_and_normals_after_the_first_face_stay_unplaced(ra, tmp_path):
    g, text = quirk(ra, tmp_path, "late")
    topo = g.mesh_topology(0)
    assert topo["placed_pos"] == 3 and topo["placed_nrm"] == 3 and g.mesh_vertices(0)[0].shape[0] == 4
    P0, N0 = g.mesh_vertices(0)
    V = (P0 + np.float32([[0.1, 0, 0], [0, 0.2, 0], [0, 0, 0.3], [0.5, -0.25, 0.125]])).astype(np.float32)
    N = np.float32([[0, 0, 2], [0, 3, 0], [1, 0, 0], [0, 5, 5]])[::-1].copy()
    for nn, tag in ((None, "v"), (N, "vn")):
        g.set_vertices(0, V, nn)
        f, _ = deformed_scene(ra, tmp_path, text, 0, V, nn, "late_" + tag)
        assert_same(g, f, 0, "late " + tag)
        tris = f.bvh(0)["tris"]
        # the vertex and the normal declared late are used as given: triangle 1's corner c is vertex 3, its normal normalised only
        assert np.array_equal(bits(tris[1, 6:9]), bits(V[3]))
        if nn is not None:
            assert np.array_equal(bits(tris[1, 15:18]), bits(f.mesh_vertices(0)[1][3]))
        f.close()
    # ... and the shared formulas agree (fresh state: the probe takes the stored normals of a scene that was not given any)
    g2, _ = quirk(ra, tmp_path, "late")
    f, _ = deformed_scene(ra, tmp_path, text, 0, V, N, "late_probe")
    probe_equals_bvh(ra, g2, 0, V, N, f, "late")
    f.close(); g2.close(); g.close()


def test_a_rotated_minus_zero_becomes_plus_zero_as_in_the_loaders_mult_vec_matrix(ra, tmp_path):
    """Unrotated, a normal's -0 components come out of the three products as -0; the loader's multVecMatrix adds the matrix's fourth row
    (+0) and stores +0."""
    g, text = quirk(ra, tmp_path, "late", rot="0,0,0")
    P0, _ = g.mesh_vertices(0)
    nz = -0.0
    N = np.float32([[-1, nz, -1], [nz, -2, nz], [nz, nz, -3], [nz, 5, 5]])
    assert np.signbit(N[0, 1]) and np.signbit(N[2, 0])
    f, _ = deformed_scene(ra, tmp_path, text, 0, P0, N, "minus_zero")
    r = probe_equals_bvh(ra, g, 0, P0, N, f, "minus zero")
    rotated = r["nrm"][0].reshape(3, 3)      # triangle 0 has the three rotated normals
    assert (rotated == 0).sum() == 5 and not np.signbit(rotated[rotated == 0]).any()
    # ... while the one read after the first face is not rotated and keeps its sign
    assert np.signbit(r["nrm"][1, 6]) and r["nrm"][1, 6] == 0
    g.set_vertices(0, P0, N)
    assert_same(g, f, 0, "minus zero")
    f.close(); g.close()


def test_a_mesh_wholly_at_negative_coordinates_keeps_the_loaders_upper_bound(ra, tmp_path):
    g, text = quirk(ra, tmp_path, "negative")
    P0, _ = g.mesh_vertices(0)
    V = scale(P0, (1.1, 0.9, 1.3))
    assert (V < 0).all()
    g.set_vertices(0, V)
    f, _ = deformed_scene(ra, tmp_path, text, 0, V, None, "negative")
    assert_same(g, f, 0, "negative")
    r = probe_equals_bvh(ra, g, 0, V, None, f, "negative")
    assert (bits(r["obj_hi"]) == 0x00800000).all(), "objHi must stay FLT_MIN, the smallest positive float"
    f.close(); g.close()


def test_the_sign_of_a_zero_minimum_reaches_no_triangle(ra, tmp_path):
    g, text = quirk(ra, tmp_path, "zeros")
    P0, _ = g.mesh_vertices(0)
    nz = np.float32(-0.0)
    results = []
    for order, tag in (((0.0, nz), "pm"), ((nz, 0.0), "mp")):
        V = P0.copy()
        V[0, 0], V[2, 0] = order      # the two vertices at the x minimum
        V[0, 2], V[2, 2] = order      # ... and at the z minimum
        V[0, 1], V[1, 1] = order[::-1]
        assert np.signbit(V[0, 0]) != np.signbit(V[2, 0])
        g.set_vertices(0, V)
        f, _ = deformed_scene(ra, tmp_path, text, 0, V, None, "zeros_" + tag)
        assert_same(g, f, 0, "zeros " + tag)
        r = probe_equals_bvh(ra, g, 0, V, None, f, "zeros " + tag)
        results.append((g.bvh(0)["tris"].copy(), r))
        f.close()
    assert np.array_equal(bits(results[0][0][:, 0:18]), bits(results[1][0][:, 0:18])), "the placed triangles depend on the sign of a zero"
    assert np.array_equal(bits(results[0][1]["pos"]), bits(results[1][1]["pos"]))
    g.close()


def test_a_zero_uv_determinant_gives_the_loaders_nan(ra, tmp_path):
    g, text = quirk(ra, tmp_path, "uvdet")
    P0, _ = g.mesh_vertices(0)
    V = bulge(P0, 0.2, 1.5)
    g.set_vertices(0, V)
    f, _ = deformed_scene(ra, tmp_path, text, 0, V, None, "uvdet")
    assert_same(g, f, 0, "uvdet")
    r = probe_equals_bvh(ra, g, 0, V, None, f, "uvdet")
    tb = bits(r["tb"])
    nan = np.isnan(r["tb"])
    assert nan[0].all() and nan[1, 0:3].all() and not nan[2].any(), "the test's triangles: all NaN, a NaN tangent, a finite frame"
    assert (tb[nan] == 0xFFC00000).all(), "a NaN the arithmetic creates is stored as x86 writes it"
    f.close(); g.close()


def test_refusals_leave_the_scene_as_it_was(ra, tmp_path):
    g = ra.Scene("scenes/mixed_materials.scene", 64, 48)
    digest = g.digest()
    before = {i: g.bvh(i) for i in (0, 1, 2)}
    P1, N1 = g.mesh_vertices(1)
    with pytest.raises(ValueError):
        g.set_vertices(1, P1[:-1])                                  # a wrong row count
    with pytest.raises(ValueError):
        g.set_vertices(1, P1, N1[:-1])
    with pytest.raises(ValueError):
        g.set_vertices(1, P1.astype(np.float64))                    # float64
    with pytest.raises(ValueError):
        g.set_vertices(1, P1.reshape(-1))                           # no (n, 3)
    with pytest.raises(ValueError):
        g.set_vertices(3, P1)                                       # a sphere
    with pytest.raises(ValueError):
        g.set_vertices(9, P1)                                       # no such object
    for bad in (np.nan, np.inf, -np.inf):
        V = P1.copy(); V[5, 1] = bad
        with pytest.raises(ra.RtxError):
            g.set_vertices(1, V)
        N = N1.copy(); N[3, 0] = bad
        with pytest.raises(ra.RtxError):
            g.set_vertices(1, bulge(P1), N)
    # a flat axis away from zero: the loader's own 0 / 0, which the rotation spreads over the vertex
    P0, _ = g.mesh_vertices(0)
    V = P0.copy(); V[:, 1] = 1
    with pytest.raises(ra.RtxError):
        g.set_vertices(0, V)
    # the host entry point refuses a wrong count as well
    assert g.host.rah_mesh_set_vertices(g.h, 1, P1.ctypes.data, P1.shape[0] - 1, None, 0, 0, None) != 0
    assert b"vertices" in g.host.rah_last_error()
    assert np.array_equal(bits(g.digest()), bits(digest))
    for i, b in before.items():
        assert same_structure(g.bvh(i), b) is None, "object %d changed by a refused call" % i
        assert np.array_equal(bits(g.mesh_vertices(i)[0]), bits({0: P0, 1: P1}.get(i, g.mesh_vertices(i)[0])))
    # the probe reports both kinds
    r = ra.place_probe(g.mesh_topology(0), g.mesh_vertices(0)[1], V, None, g.mesh_pose(0))
    assert r["bad_placed"] and not r["bad_input"] and np.isnan(r["pos"]).any()
    V = P1.copy(); V[0, 0] = np.nan
    r = ra.place_probe(g.mesh_topology(1), N1, V, None, g.mesh_pose(1))
    assert r["bad_input"] and not r["pos"].any()
    g.close()


def test_deform_symbols_are_declared_where_they_belong(ra):
    hdr = open(os.path.join(ROOT, "include", "rtx_deform.h")).read()
    decl = lambda text: set(re.findall(r"\b(rtx_[a-z0-9_]+)\s*\(", text))
    declared = decl(hdr)
    assert declared == set(ra.RTX_DEFORM_SYMBOLS) and len(ra.RTX_DEFORM_SYMBOLS) == len(declared) == 2
    for other in (ra.RTX_SYMBOLS, ra.RTX_EDIT_SYMBOLS, ra.RTX_QUERY_SYMBOLS, ra.RTX_AOV_SYMBOLS, ra.RTX_AO_SYMBOLS, ra.RTX_SURFACE_SYMBOLS, ra.RTX_LIGHT_SYMBOLS):
        assert not declared & set(other)
    rtx, host = ra.load()
    for s in declared:
        assert hasattr(rtx, s), s
    listed, missing = ra.exported_symbols()
    assert not missing and listed == list(ra.RTX_SYMBOLS)
    assert "rtx_place_probe" in decl(open(os.path.join(ROOT, "include", "rtx_debug.h")).read()) and "rtx_place_probe" in ra.RTX_SYMBOLS
    for other in ("rtx.h", "rtx_scene_edit.h"):
        assert not declared & decl(open(os.path.join(ROOT, "include", other)).read())
    for s in ("rah_mesh_counts", "rah_mesh_vertices", "rah_mesh_topology", "rah_mesh_set_vertices"):
        assert hasattr(host, s), s
    # the structures of the binding are the header's
    body = re.search(r"typedef struct rtx_mesh_topology \{(.*?)\} rtx_mesh_topology;", hdr, re.S).group(1)
    names = re.findall(r"(\w+)\s*(?:,|;)", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == [n for n, _ in ra.MeshTopology._fields_]
    body = re.search(r"typedef struct rtx_mesh_pose \{(.*?)\} rtx_mesh_pose;", hdr, re.S).group(1)
    names = re.findall(r"(\w+)(?:\[\d+\])?\s*;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == [n for n, _ in ra.MeshPose._fields_]
