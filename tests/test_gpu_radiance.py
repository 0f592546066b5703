"""rtx_radiance_points / Scene.radiance_points (include/rtx_radiance.h): radiance gathered over directions at surface points the caller
supplies.  Every comparison is bit for bit: the expectation is the composition on the same scene object -- the rays {P + N * bias, d_k}
of tests/util_radiance through Scene.trace_rays(colours=True), which tests/test_gpu_trace_rays.py holds against the oracle, then
tests/util_radiance's restatement of the weighted sum, which tests/test_radiance_cpu.py pins to the oracle."""
import ctypes as C

import numpy as np
import pytest

from tests import util_ao as AO
from tests import util_aov as U
from tests import util_radiance as UR

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

f32 = np.float32
GUARD = 96                    # untouched elements before and after every buffer
FILL = 7.25
FILL_BITS = int(np.array(FILL, f32).view(np.uint32))
N_FREE = 512
K_MIN = 1 << 20               # kReorderMin (rtx_query.hip): batches are regrouped from this many points on


def dev(a, dtype=f32):
    return torch.from_numpy(np.array(a, dtype, order="C")).cuda()


def unit(v):
    with np.errstate(all="ignore"):
        return (v / np.sqrt((v.astype(np.float64) ** 2).sum(1))[:, None]).astype(f32)


def point_pool(g, n_free=N_FREE, seed=0x2AD1):
    """{P, N} at the first hits of the camera rays (surface_rays' position and normal), then n_free seeded free points: inside the box of
    those hits (so some are inside the meshes) or 1e3 to 1e6 outside it, with normals of every kind -- random unit vectors, which make
    neighbouring lanes trace different subsets of the directions, zero, NaN, of length 3, axis-aligned with -0 components."""
    cam = dev(U.primary_rays(g))
    s = g.surface_rays(cam, hits=True, position=True, normal=True, albedo=False)
    torch.cuda.synchronize()
    hit = s["hits"][:, 0].cpu().numpy() > 0
    at = np.concatenate([s["position"].cpu().numpy()[hit], s["normal"].cpu().numpy()[hit]], 1).astype(f32)
    lo, hi = np.clip(at[:, 0:3].min(0), -20, 20), np.clip(at[:, 0:3].max(0), -20, 20)
    rng = np.random.default_rng(seed)
    P = rng.uniform(lo - 0.5, hi + 0.5, (n_free, 3)).astype(f32)
    N = unit(rng.normal(size=(n_free, 3)).astype(f32))
    kind = np.arange(n_free) % 16
    far = kind == 10
    P[far] = (unit(rng.normal(size=(far.sum(), 3)).astype(f32)) * f32([1e3, 1e6])[np.arange(far.sum()) % 2][:, None]).astype(f32)
    N[kind == 11] = 0
    N[kind == 12] *= f32(3)
    N[kind == 13, rng.integers(0, 3)] = np.nan
    axes = np.array([[-0.0, 1, -0.0], [1, -0.0, -0.0], [-0.0, -0.0, -1], [-0.0, -1, 0.0]], f32)
    N[kind == 14] = axes[rng.integers(0, 4, (kind == 14).sum())]
    free = np.concatenate([P, N], 1).astype(f32)
    return np.ascontiguousarray(np.concatenate([at, free])), int(hit.sum())


def colours_of(g, points, dirs):
    """Step 2 by composition: the colours (n, K, 3) Scene.trace_rays gives all n x K rays of tests/util_radiance"""
    rays, traced = UR.rays(points, dirs)
    n, K = traced.shape
    if n == 0:
        return np.zeros((0, K, 3), f32)
    _, col = g.trace_rays(dev(rays), hits=False, colours=True)
    torch.cuda.synchronize()
    return col.cpu().numpy().reshape(n, K, 3)


def expected(g, points, dirs, weights=None, cosine=False, col=None):
    col = colours_of(g, points, dirs) if col is None else col
    return UR.reduce(col, np.asarray(points, f32)[:, 3:6], dirs, weights, cosine)


def radiance(g, points, dirs, weights=None, cosine=False):
    out = g.radiance_points(dev(points), dev(dirs), None if weights is None else dev(weights), cosine=cosine, total=True, counts=True)
    torch.cuda.synchronize()
    assert set(out) == {"sum", "counts"} and out["sum"].dtype == torch.float32 and out["counts"].dtype == torch.int32
    assert tuple(out["sum"].shape) == (len(points), 3) and tuple(out["counts"].shape) == (len(points),)
    return out["sum"].cpu().numpy(), out["counts"].cpu().numpy().view(np.uint32)


def assert_same(got, want, what):
    bad = np.nonzero((UR.bits(got[0]) != UR.bits(want[0])).any(1))[0]
    assert bad.size == 0, "%s: the sums of %d of %d points differ, first %s" % (what, len(bad), len(want[0]), bad[:5])
    bad = np.nonzero(got[1] != want[1])[0]
    assert bad.size == 0, "%s: the counts of %d of %d points differ, first %s" % (what, len(bad), len(want[1]), bad[:5])


def weight_sets(K, seed=0x3E1):
    """seeded positive weights, and the same with a zero, a negative and a NaN entry"""
    w = np.random.default_rng(seed).uniform(0.05, 2.0, K).astype(f32)
    odd = w.copy()
    odd[0 % K], odd[min(2, K - 1)], odd[min(5, K - 1)] = f32(0), f32(-0.75), f32(np.nan)
    return w, odd


def family_of(g):
    """the kernel family the scene's launches take: "analytic" (no mesh kernel), "plain" or "general" """
    v = g.kernel_variant()
    return "analytic" if v["analytic"] else ("plain" if v["plain"] else "general")


def with_skybox(name, tmp_path):
    """scenes/<name>.scene with the six skybox faces of cfg3_reflective_refractive among its options, written into tmp_path (asset paths
    stay relative to the repository root)"""
    faces = [ln for ln in open("scenes/cfg3_reflective_refractive.scene").read().splitlines() if ln.startswith("skyboxes=")]
    assert len(faces) == 1
    text = open("scenes/%s.scene" % name).read()
    assert text.count("[options]\n") == 1 and "skyboxes=" not in text
    path = str(tmp_path / "sky.scene")
    with open(path, "w") as f:
        f.write(text.replace("[options]\n", "[options]\n" + faces[0] + "\n"))
    return path


# ---- 1. the scenes -------------------------------------------------------------------------------------------------------------------------
# (name, width, height, culling, skybox -- the flag, on a copy of the scene with skybox faces --, the kernel family that must serve it -- None: whichever does)
SCENES = [("cfg1_simple_shapes", 48, 32, None, None, "analytic"), ("cfg2_smooth_4k", 48, 32, 1, None, "plain"),
          ("cfg2_smooth_4k", 48, 32, 0, None, "plain"), ("mixed_materials", 48, 32, 1, None, "general"),
          ("mixed_materials", 64, 48, 0, None, "general"), ("cfg3_reflective_refractive", 48, 32, None, None, "analytic"),
          ("area_light", 48, 32, 1, None, None),
          ("area_light", 48, 32, 0, None, None), ("cfg4_textured_256", 48, 32, 1, 1, None), ("cfg4_textured_256", 48, 32, 0, 1, None)]


@pytest.mark.parametrize("name,w,h,cull,sky,family", SCENES)
def test_radiance_is_the_composition(ra, tmp_path, name, w, h, cull, sky, family):
    g = ra.Scene("scenes/%s.scene" % name if sky is None else with_skybox(name, tmp_path), w, h)
    if cull is not None:
        g.set_flag("useBackfaceCulling", cull)
    if sky is not None:
        g.set_flag("useSkybox", sky)
    v = family_of(g)
    assert family is None or v == family          # (the PLAIN and the general families are both exercised, and the walk-free kernel)
    points, n_hits = point_pool(g)
    n = len(points)
    assert n_hits >= 0.10 * w * h
    some_nan = False
    for dirs in (AO.DIRS19, ra.sphere_directions(16)):
        K = len(dirs)
        col = colours_of(g, points, dirs)
        traced = UR.cosines(points[:, 3:6], dirs) > 0
        # neighbouring lanes of one wave trace different subsets of the directions
        free = traced[n_hits:n_hits + 64]
        assert len({r.tobytes() for r in free}) >= 16
        w_pos, w_odd = weight_sets(K)
        for weights in (None, w_pos, w_odd):
            for cosine in (False, True):
                want = expected(g, points, dirs, weights, cosine, col)
                got = radiance(g, points, dirs, weights, cosine)
                assert_same(got, want, "%s cull %s, %d directions, weights %s, cosine %s" % (
                    name, cull, K, "none" if weights is None else ("odd" if weights is w_odd else "positive"), cosine))
                some_nan = some_nan or bool(np.isnan(got[0]).any())
        assert (got[1] == traced.sum(1)).all() and (got[1] > 0).any() and (got[1] == 0).any()
        dead = ~traced.any(1)
        assert dead.sum() >= N_FREE // 16 and not UR.bits(got[0][dead]).any()
    assert some_nan, "the NaN weight reached no sum"
    print("%s %dx%d cull %s: %d points (%d at hits), the %s family" % (name, w, h, cull, n, n_hits, v))
    g.close()


def test_sky_texels_enter_the_sums(ra, tmp_path):
    g = ra.Scene(with_skybox("cfg4_textured_256", tmp_path), 48, 32)
    points, _ = point_pool(g)
    dirs = ra.sphere_directions(16)
    sums = {}
    for sky in (0, 1):
        g.set_flag("useSkybox", sky)
        sums[sky] = radiance(g, points, dirs)
        assert_same(sums[sky], expected(g, points, dirs), "skybox %d" % sky)
    assert (UR.bits(sums[0][0]) != UR.bits(sums[1][0])).any() and np.array_equal(sums[0][1], sums[1][1])
    g.close()


# ---- 2. batch shapes, order, slices ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed(ra):
    """mixed_materials with its pool and the colours of all its rays under DIRS19, computed once and shared read-only"""
    g = ra.Scene("scenes/mixed_materials.scene", 48, 32)
    points, n_hits = point_pool(g)
    if len(points) % 256 == 0:
        points = points[:-1]          # (the last group of the whole pool is short)
    col = colours_of(g, points, AO.DIRS19)
    w_pos, _ = weight_sets(len(AO.DIRS19))
    want = UR.reduce(col, points[:, 3:6], AO.DIRS19, w_pos, True)
    for a in (points, col, w_pos) + want:
        a.setflags(write=False)
    yield g, points, col, w_pos, want
    g.close()


@pytest.mark.parametrize("reorder", [-1, 1])
def test_batch_sizes_and_order(mixed, reorder):
    g, points, col, w, want = mixed
    n = len(points)
    assert n % 256 != 0 and n > 512
    g.set_knob("trace_reorder", reorder)          # (1: the sort runs on every batch, however small)
    try:
        assert_same(radiance(g, points, AO.DIRS19, w, True), want, "the whole pool, reorder %d" % reorder)
        rng = np.random.default_rng(17)
        perm = rng.permutation(n)
        assert_same(radiance(g, points[perm], AO.DIRS19, w, True), (want[0][perm], want[1][perm]), "a shuffled batch, reorder %d" % reorder)
        for m in (1, 63, 64, 65, 257):
            first = int(rng.integers(0, n - m))
            sl = slice(first, first + m)
            assert_same(radiance(g, points[sl], AO.DIRS19, w, True), (want[0][sl], want[1][sl]), "n = %d, reorder %d" % (m, reorder))
        out = g.radiance_points(dev(points[:0]), dev(AO.DIRS19), counts=True)
        assert tuple(out["sum"].shape) == (0, 3) and tuple(out["counts"].shape) == (0,)
    finally:
        g.set_knob("trace_reorder", -1)


def test_an_unaligned_slice_of_a_larger_tensor(mixed):
    g, points, col, w, want = mixed
    flat = torch.full((len(points) * 6 + 7,), float("nan"), dtype=torch.float32, device="cuda")
    for off in (1, 3):
        t = flat[off:off + len(points) * 6].view(-1, 6)
        t.copy_(dev(points))
        assert t.data_ptr() % 16 != 0 and t.is_contiguous()
        out = g.radiance_points(t[5:-3], dev(AO.DIRS19), dev(w), cosine=True, counts=True)
        torch.cuda.synchronize()
        got = out["sum"].cpu().numpy(), out["counts"].cpu().numpy().view(np.uint32)
        assert_same(got, (want[0][5:-3], want[1][5:-3]), "slice at offset %d" % off)


def test_every_normal_faces_away(mixed):
    g, points, col, w, want = mixed
    away = points[:300].copy()
    away[:, 3:6] = f32([0, -1, 0])
    dirs = np.array([[0, 1, 0], [0.6, 0.8, 0], [0, 0, 1], [1, 0, 0], [0, 0, 0], [np.nan, 1, 0]], f32)     # c <= 0 or NaN for every one
    total, counts = radiance(g, away, dirs, None, True)
    assert not counts.any() and not UR.bits(total).any()          # (+0, not -0)


@pytest.mark.parametrize("K", [1, 256])
def test_one_and_256_directions(ra, mixed, K):
    g, points, col, w, want = mixed
    pts = points[::7]
    dirs = ra.sphere_directions(256)[3:4] if K == 1 else ra.sphere_directions(256)
    assert len(dirs) == K
    wts = np.random.default_rng(K).uniform(0.0, 1.0, K).astype(f32)
    assert_same(radiance(g, pts, dirs, wts, True), expected(g, pts, dirs, wts, True), "%d directions" % K)


# ---- 3. only what is asked for is written (the C entry, directly) -----------------------------------------------------------------------
class Buffers:
    """sum (n x 3) and counts (n), each in the middle of a larger pre-filled allocation"""

    def __init__(self, n):
        self.n = n
        self.flat = {c: torch.full((n * k + 2 * GUARD,), FILL, dtype=torch.float32, device="cuda") for c, k in (("sum", 3), ("counts", 1))}
        self.ptr = {c: t.data_ptr() + 4 * GUARD for c, t in self.flat.items()}

    def read(self):
        torch.cuda.synchronize()
        out = {}
        for c, t in self.flat.items():
            f = t.cpu().numpy().view(np.uint32)
            assert (f[:GUARD] == FILL_BITS).all() and (f[-GUARD:] == FILL_BITS).all(), "%s: written outside the buffer" % c
            out[c] = f[GUARD:len(f) - GUARD]
        return out["sum"].reshape(self.n, 3), out["counts"]

    def untouched(self, names=("sum", "counts")):
        total, counts = self.read()
        return all((a == FILL_BITS).all() for a, c in ((total, "sum"), (counts, "counts")) if c in names)


def stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def call(ra, g, tp, td, tw, bufs, names=("sum", "counts"), n=None, n_dirs=None, cosine=1, par=True, dirs=True):
    rtx, _ = ra.load()
    p = ra.RadianceParams(td.shape[0] if n_dirs is None else n_dirs, td.data_ptr() if dirs else None, tw.data_ptr() if tw is not None else None, cosine)
    return rtx.rtx_radiance_points(g.gpu(), tp.shape[0] if n is None else n, C.c_void_p(tp.data_ptr()) if tp is not None else None,
                                   C.byref(p) if par else None, C.c_void_p(bufs.ptr["sum"]) if "sum" in names else None,
                                   C.c_void_p(bufs.ptr["counts"]) if "counts" in names else None, stream_ptr())


def test_only_what_was_asked_for_is_written(ra, mixed):
    g, points, col, w, want = mixed
    pts = points[:-1]                  # (a short last group)
    n = len(pts)
    tp, td, tw = dev(pts), dev(AO.DIRS19), dev(w)
    b = Buffers(n)
    assert call(ra, g, tp, td, tw, b) == 0
    total, counts = b.read()
    assert np.array_equal(total, UR.bits(want[0][:-1])) and np.array_equal(counts, want[1][:-1])
    for names in (("sum",), ("counts",)):
        b = Buffers(n)
        assert call(ra, g, tp, td, tw, b, names) == 0
        total, counts = b.read()
        if "sum" in names:
            assert np.array_equal(total, UR.bits(want[0][:-1])) and b.untouched(("counts",))
        else:
            assert np.array_equal(counts, want[1][:-1]) and b.untouched(("sum",))
    # fewer points than the buffers hold: the bytes beyond n stay
    b = Buffers(n)
    assert call(ra, g, tp, td, tw, b, n=100) == 0
    total, counts = b.read()
    assert np.array_equal(total[:100], UR.bits(want[0][:100])) and np.array_equal(counts[:100], want[1][:100])
    assert (total[100:] == FILL_BITS).all() and (counts[100:] == FILL_BITS).all()
    assert set(g.radiance_points(tp, td)) == {"sum"} and set(g.radiance_points(tp, td, total=False, counts=True)) == {"counts"}
    torch.cuda.synchronize()


def test_refusals_leave_the_buffers_untouched(ra, mixed):
    g, points, col, w, want = mixed
    rtx, _ = ra.load()
    pts = points[:200]
    tp, td, tw = dev(pts), dev(AO.DIRS19), dev(w)
    b = Buffers(len(pts))
    refused = [
        ("params", lambda: call(ra, g, tp, td, tw, b, par=False)),
        ("output", lambda: call(ra, g, tp, td, tw, b, names=())),
        ("dirs_dev", lambda: call(ra, g, tp, td, tw, b, dirs=False)),
        ("n_dirs", lambda: call(ra, g, tp, td, tw, b, n_dirs=0)),
        ("n_dirs", lambda: call(ra, g, tp, td, tw, b, n_dirs=257)),
        ("cosine", lambda: call(ra, g, tp, td, tw, b, cosine=2)),
        ("cosine", lambda: call(ra, g, tp, td, tw, b, cosine=-1)),
        ("points", lambda: call(ra, g, None, td, tw, b, n=len(pts))),
        ("too many", lambda: call(ra, g, tp, td, tw, b, n=0xFFFFFFC1)),
    ]
    for what, fn in refused:
        assert fn() == -1, what                 # RTX_ERR_ARG
        assert what.encode() in rtx.rtx_last_error(), (what, rtx.rtx_last_error())
    assert call(ra, g, None, td, tw, b, n=0) == 0      # n == 0: nothing to do
    assert b.untouched()
    # RTX_FLAG_SHOW_NORMALS: a debug view has no radiance
    g.set_flag("showNormals", 1)
    try:
        assert call(ra, g, tp, td, tw, b) == -4 and b"SHOW_NORMALS" in rtx.rtx_last_error()      # RTX_ERR_UNSUPPORTED
        with pytest.raises(ra.RtxError, match="SHOW_NORMALS"):
            g.radiance_points(tp, td)
        assert b.untouched()
    finally:
        g.set_flag("showNormals", 0)
    with pytest.raises(ValueError, match="radiance_points: nothing to compute"):
        g.radiance_points(tp, td, total=False)
    with pytest.raises(ValueError, match=r"radiance_points: weights must have shape \(19,\)"):
        g.radiance_points(tp, td, tw[:18])
    with pytest.raises(ValueError, match="radiance_points: weights must be float32"):
        g.radiance_points(tp, td, tw.double())
    with pytest.raises(ValueError, match="radiance_points: weights must be contiguous"):
        g.radiance_points(tp, td, torch.zeros(38, device="cuda")[::2])
    with pytest.raises(ValueError, match="radiance_points: weights must be on cuda:0"):
        g.radiance_points(tp, td, tw.cpu())
    with pytest.raises(ValueError, match=r"radiance_points: 1 \.\. 256 directions"):
        g.radiance_points(tp, torch.zeros((257, 3), device="cuda"))
    # ... and the call works afterwards
    assert call(ra, g, tp, td, tw, b) == 0
    total, counts = b.read()
    assert np.array_equal(total, UR.bits(want[0][:200])) and np.array_equal(counts, want[1][:200])


def test_a_second_call_allocates_nothing(ra, mixed):
    g, points, col, w, want = mixed
    tp, td, tw = dev(points), dev(AO.DIRS19), dev(w)
    g.radiance_points(tp, td, tw, cosine=True, counts=True)
    torch.cuda.synchronize()
    before = ra.live_device_memory()
    out = g.radiance_points(tp, td, tw, cosine=True, counts=True)
    torch.cuda.synchronize()
    assert ra.live_device_memory() == before
    assert_same((out["sum"].cpu().numpy(), out["counts"].cpu().numpy().view(np.uint32)), want, "the second call")


# ---- 4. regrouping --------------------------------------------------------------------------------------------------------------------------
def test_a_batch_just_above_the_regrouping_threshold(ra):
    g = ra.Scene("scenes/cfg1_simple_shapes.scene", 48, 32)
    pool, _ = point_pool(g, n_free=2048)
    n = K_MIN + 77
    rng = np.random.default_rng(0xB16)
    points = pool[rng.integers(0, len(pool), n)].copy()
    points[:, 0:3] += rng.uniform(-0.25, 0.25, (n, 3)).astype(f32)
    dirs = np.array([[0.3, 0.9, 0.2], [-0.5, 0.2, 0.8]], f32)
    w = f32([0.75, 1.5])
    out = g.radiance_points(dev(points), dev(dirs), dev(w), cosine=True, counts=True)
    torch.cuda.synchronize()
    idx = np.unique(np.concatenate([np.arange(128), np.arange(n - 128, n), rng.choice(n, 4096, replace=False)]))
    got = out["sum"].cpu().numpy()[idx], out["counts"].cpu().numpy().view(np.uint32)[idx]
    assert_same(got, expected(g, points[idx], dirs, w, True), "%d points" % n)
    assert (got[1] > 0).any() and (got[1] < 2).any()
    g.close()


# ---- 5. scene state -------------------------------------------------------------------------------------------------------------------------
AREA = dict(pos=(0.5, 2.5, -2.0), i=(1.0, 0, 0.2), j=(0, 0.1, 1.0), samples=3, color=(1, 0.9, 0.8), intensity=0.6)


def test_after_scene_edits(ra):
    g = ra.Scene("scenes/cfg2_smooth_4k.scene", 48, 32)
    points, _ = point_pool(g)
    dirs = ra.sphere_directions(16)
    w, _ = weight_sets(16)

    def check(what):
        got = radiance(g, points, dirs, w, True)
        assert_same(got, expected(g, points, dirs, w, True), what)
        return got

    assert family_of(g) == "plain"
    first = check("as loaded")
    g.set_camera((0.3, 0.4, 0.5), (-5.0, 10.0, 0.0))
    check("set_camera")
    g.set_flag("useBackfaceCulling", 0)
    check("culling off")
    g.set_flag("useBackfaceCulling", 1)
    g.set_light(1, position=(1.5, 0.5, -1.5), intensity=0.9)
    lit = check("set_light")
    assert (UR.bits(lit[0]) != UR.bits(first[0])).any()
    g.add_light("area", **AREA)
    assert family_of(g) == "general"          # (an area light: the PLAIN family no longer serves)
    area = check("an area light added")
    assert (UR.bits(area[0]) != UR.bits(lit[0])).any()
    g.close()


def test_after_move_object(ra):
    g = ra.Scene("scenes/mixed_materials.scene", 48, 32)
    points, _ = point_pool(g)
    w, _ = weight_sets(19)
    before = radiance(g, points, AO.DIRS19, w, False)
    for k, (index, keys) in enumerate([(3, dict(pos=(0.4, 1.2, -5.5), radius=0.85)), (1, dict(rot=(-40, 10, 70), pos=(-0.9, 0.2, -4.4)))]):
        g.move_object(index, **keys)
        got = radiance(g, points, AO.DIRS19, w, False)
        assert_same(got, expected(g, points, AO.DIRS19, w, False), "move %d" % k)
        assert (UR.bits(got[0]) != UR.bits(before[0])).any()
        before = got
    g.close()
