"""GPU: rtx_bvh_build must reproduce the host builder -- which the CPU suite pins to the real
reference's BVH digests (tests/test_host_cpu.py, tests/golden) -- bit for bit: topology, bounds, reference order."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEYS = ("bounds", "skip", "leaf_begin", "leaf_count", "refs")


def _mesh_objects(g):
    return [i for i in range(g.n_objects) if g.bvh(i) is not None]


def _same(a, b):
    for k in KEYS:
        assert a[k].shape == b[k].shape, (k, a[k].shape, b[k].shape)
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    assert a["max_depth"] == b["max_depth"] and a["n_nodes"] == b["n_nodes"] and a["n_refs"] == b["n_refs"]


@pytest.mark.parametrize("name", ["cfg2_smooth_4k", "cfg2_smooth_25k", "cfg4_textured_256", "mixed_materials", "legacy_smooth_4k",
                                  "cfg2_smooth_250k"])
def test_device_build_equals_host_build(ra, name):
    """Same scene loaded twice: acceleration structures from the host builder and from the device builder."""
    path = "scenes/%s.scene" % name
    if name == "cfg2_smooth_250k":
        from rendering_amd import assets
        assets.ensure(["bumpy_250k.obj"])      # (the default asset set leaves the 250k mesh out)
    try:
        ra.set_ac_build("host")
        gh = ra.Scene(path, 64, 64)
        ra.set_ac_build("device")
        gd = ra.Scene(path, 64, 64)
    finally:
        ra.set_ac_build("auto")
    objs = _mesh_objects(gh)
    assert objs and objs == _mesh_objects(gd)
    for oi in objs:
        h, d = gh.bvh(oi), gd.bvh(oi)
        assert not h["built_on_device"] and d["built_on_device"] and d["build_ms"] > 0
        _same(h, d)


def test_default_loader_picks_the_faster_builder(ra):
    """The loader's default: the device builder from 50 000 triangles on (where it is the faster one), the host builder
    for small meshes -- the same structure either way (the digest test pins the 250k one to the reference)."""
    from rendering_amd import assets
    assets.ensure(["bumpy_250k.obj"])
    ra.set_ac_build("auto")
    g = ra.Scene("scenes/cfg2_smooth_4k.scene", 64, 64)
    assert not any(g.bvh(oi)["built_on_device"] for oi in _mesh_objects(g))
    g = ra.Scene("scenes/cfg2_smooth_250k.scene", 64, 64)
    assert all(g.bvh(oi)["built_on_device"] for oi in _mesh_objects(g))


@pytest.mark.parametrize("penalty", [1, 2, 3, 7, 1000000])
def test_penalty_sweep_against_host_builder(ra, tmp_path, penalty):
    """Leaf rule n <= depth * acPenalty (objects.cpp:477) across penalties, via temporary scene files."""
    src = open("scenes/cfg2_smooth_4k.scene").read().replace("fov=60", "fov=60\nac_penalty=%d" % penalty)
    p = tmp_path / "p.scene"
    p.write_text(src)
    try:
        ra.set_ac_build("host")
        gh = ra.Scene(str(p), 64, 64)
    finally:
        ra.set_ac_build("auto")
    for oi in _mesh_objects(gh):
        h = gh.bvh(oi)
        d = ra.bvh_build(h["tris"][:, :9], h["bounds"][0, :3], h["bounds"][0, 3:], penalty)
        _same(h, d)


def test_edge_cases(ra):
    lo, hi = np.array([-1, -1, -1], np.float32), np.array([1, 1, 1], np.float32)
    # no triangles: a single empty leaf (objects.cpp:477 with n = 0)
    d = ra.bvh_build(np.zeros((0, 9), np.float32), lo, hi, 1)
    assert d["n_nodes"] == 1 and d["n_refs"] == 0 and d["max_depth"] == 1
    assert d["leaf_begin"][0] == 0 and d["leaf_count"][0] == 0 and d["skip"][0] == 1
    assert np.array_equal(d["bounds"][0], np.concatenate([lo, hi]))
    # one triangle: leaf at the root (1 <= 1 * 1)
    d = ra.bvh_build(np.array([[0, 0, 0, 1, 0, 0, 0, 1, 0]], np.float32), lo, hi, 1)
    assert d["n_nodes"] == 1 and list(d["refs"]) == [0]
    # identical triangles cannot be separated: the 1.5x duplication rule stops the recursion (objects.cpp:498)
    tri = np.tile(np.array([[0, 0, 0, 0.5, 0, 0, 0, 0.5, 0]], np.float32), (64, 1))
    d = ra.bvh_build(tri, lo, hi, 1)
    leaves = d["leaf_count"] >= 0
    assert d["n_refs"] >= 64 and set(d["refs"]) == set(range(64))
    assert d["skip"][0] == d["n_nodes"] and (d["leaf_count"][leaves].sum() == d["n_refs"])
    # determinism
    d2 = ra.bvh_build(tri, lo, hi, 1)
    _same(d, d2)


def test_error_paths(ra):
    lo, hi = np.zeros(3, np.float32), np.ones(3, np.float32)
    with pytest.raises(ra.RtxError):
        ra.bvh_build(np.zeros((1, 9), np.float32), lo, np.array([np.inf, 1, 1], np.float32), 1)
    with pytest.raises(ra.RtxError):
        ra.bvh_build(np.zeros((1, 9), np.float32), lo, hi, 1, device=99)


def test_persistent_build_equals_the_level_by_level_build(ra):
    """rtx_bvh_build runs as two persistent launches over a queue of nodes (round 5: 740 launches -> 7); the level-by-level build of rounds 1-4 is its
    fallback.  Both must give the reference's structure: compared with each other here, with the host builder / the reference's digests elsewhere."""
    s = ra.Scene("scenes/cfg2_smooth_25k.scene", 64, 64)
    h = s.bvh(1)
    s.close()
    q = ra.bvh_build(h["tris"][:, :9], h["bounds"][0, :3], h["bounds"][0, 3:], 1)
    assert q["queued"] and q["launches"] <= 20, (q["queued"], q["launches"])
    ra.bvh_build_mode(1)
    try:
        l = ra.bvh_build(h["tris"][:, :9], h["bounds"][0, :3], h["bounds"][0, 3:], 1)
    finally:
        ra.bvh_build_mode(0)
    assert not l["queued"] and l["launches"] > 100
    for k in ("bounds", "skip", "leaf_begin", "leaf_count", "refs"):
        assert q[k].tobytes() == l[k].tobytes() == h[k].tobytes(), k
    assert q["max_depth"] == l["max_depth"] == h["max_depth"]


def test_persistent_build_gives_up_cleanly_when_its_pools_run_out(ra):
    """Pools far too small (rtx_bvh_build_mode(2)): the persistent launches report it instead of writing out of bounds or waiting for ever, and rtx_bvh_build
    delivers the structure through the level-by-level path."""
    s = ra.Scene("scenes/cfg2_smooth_25k.scene", 64, 64)
    h = s.bvh(1)
    s.close()
    ra.bvh_build_mode(2)
    try:
        d = ra.bvh_build(h["tris"][:, :9], h["bounds"][0, :3], h["bounds"][0, 3:], 1)
    finally:
        ra.bvh_build_mode(0)
    assert not d["queued"]
    for k in ("bounds", "skip", "leaf_begin", "leaf_count", "refs"):
        assert d[k].tobytes() == h[k].tobytes(), k
    again = ra.bvh_build(h["tris"][:, :9], h["bounds"][0, :3], h["bounds"][0, 3:], 1)
    assert again["queued"] and again["refs"].tobytes() == h["refs"].tobytes()
