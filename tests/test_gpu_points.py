"""rtx_light_points / Scene.light_points and rtx_ao_points / Scene.ao_points (include/rtx_points.h): direct light and ambient occlusion at
surface points the caller supplies.  Every comparison is bit for bit over every point:
  1. at the hits of rays, with {P, N} from surface_rays, V the ray's direction and ns the hit object's, light_points is light_rays;
  2. on free points in space, with normals of every kind, every channel is tests/util_points' restatement (pinned to the oracle by
     tests/test_points_cpu.py) with the visibility from Scene.occluded -- which walks with source class 0, so the source copies of the
     point lights are checked too;
  3. the same far away from the mesh, where a source copy must not serve;
  4. ao_points at the camera's hits is render_ao, and on the free points the restatement;
  5. across batches, orders and sizes;  6. only what is asked for is written;  7. scene edits, flags, counters, streams, refusals."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import util_ao as AO
from tests import util_aov as U
from tests import util_light as UL
from tests import util_lights as LE
from tests import util_points as UP
from tests import util_shading as S
from tests import util_surface as SU
from tests.ac_heatmap import scene_copy

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = U.ROOT
f32 = np.float32
GUARD = 96                    # untouched elements before and after every buffer
FILL = 7.25
CH = UP.CHANNELS
FREE_SCENES = ["cfg2_smooth_4k", "area_light", "mixed_nrm"]
N_FREE = 4096
RADIUS = 1.5                  # the finite AO range: some rays blocked further away than this are open under it


@pytest.fixture(scope="module")
def family(tmp_path_factory):
    d = S.short_dir(tmp_path_factory)
    return d, S.write_family(d)


def path_of(name, family):
    return family[1][name] if name in S.FAMILY else "scenes/%s.scene" % name


def dev(a, dtype=f32):
    return torch.from_numpy(np.array(a, dtype, order="C")).cuda()      # (a copy: the shared cases are read-only)


def host(out):
    torch.cuda.synchronize()
    return {c: t.cpu().numpy() for c, t in out.items()}


def light_points(g, points, view, per_light=True, stream=None):
    """channel -> numpy array of Scene.light_points for numpy arrays"""
    out = host(g.light_points(dev(points), None if view is None else dev(view), per_light=per_light, stream=stream))
    want = ("diffuse",) + (("specular",) if view is not None else ()) + \
           ((("light_diffuse", "light_open") + (("light_specular",) if view is not None else ())) if per_light else ())
    assert set(out) == set(want)
    return out


def ao_points(g, points, dirs, radius):
    out = host(g.ao_points(dev(points), dev(dirs), radius, ao=True, counts=True))
    assert set(out) == {"ao", "counts"} and out["counts"].dtype == np.int32 and out["ao"].dtype == f32
    return out["counts"].view(np.uint32), out["ao"]


def surface(g, rays):
    return host(g.surface_rays(dev(rays), hits=True, position=True, normal=True, albedo=False))


def points_at_hits(g, rays):
    """(hit mask, points {P, N}, view {V, ns}) at the hits of `rays`: surface_rays' position and normal, the ray's direction, the hit
    object's n_specular"""
    s = surface(g, rays)
    objs, _ = g.device_objects()
    hit = s["hits"][:, 0] > 0
    obj = s["hits"][hit, 1].astype(np.int32)
    points = np.concatenate([s["position"][hit], s["normal"][hit]], 1).astype(f32)
    view = np.concatenate([rays[hit, 3:6], objs["n_specular"][obj].astype(f32)[:, None]], 1).astype(f32)
    return hit, points, view


def identity_with_light_rays(g, rays, what):
    """1.: light_points at the hits of `rays` equals light_rays there, all five channels.  Returns the number of hits compared."""
    hit, points, view = points_at_hits(g, rays)
    if not hit.any():
        return 0
    got = light_points(g, points, view)
    lr = host(g.light_rays(dev(rays), per_light=True))
    bad = UP.same(got, {c: lr[c][hit] for c in CH}, CH)
    assert not bad, "%s: light_points differs from light_rays at the hits in %s" % (what, {
        c: int((U.bits(got[c]) != U.bits(lr[c][hit])).reshape(len(points), -1).any(1).sum()) for c in bad})
    # ... and the sums alone, where the pairs that cannot matter are not walked
    sums = light_points(g, points, view, per_light=False)
    assert not UP.same(sums, got, UP.SUMS), "%s: the sums of a call without per-light buffers" % what
    return int(hit.sum())


def first_hit_rays(g):
    """(A) and (B) of Scene g"""
    cam, depth, normal, hit = AO.first_hits(g)
    return cam, SU.bounce_rays(cam, depth, normal, hit)


# ---- 1. identity with light_rays ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cull", [1, 0])
@pytest.mark.parametrize("name", UL.SCENES)
def test_light_points_at_hits_is_light_rays(ra, family, name, cull):
    w, h = UL.size_of(name)
    g = ra.Scene(path_of(name, family), w, h)
    g.set_flag("useBackfaceCulling", cull)
    cam, bounce = first_hit_rays(g)
    for what, rays in (("A", cam), ("B", bounce), ("D", SU.probe_rays())):
        n = identity_with_light_rays(g, rays, "%s cull %d (%s)" % (name, cull, what))
        print("%s %dx%d cull %d (%s): %d hits of %d rays compared" % (name, w, h, cull, what, n, len(rays)))
        if what == "A":
            assert n >= 0.10 * len(rays)
    g.close()


# ---- 2. the restatement on free points -------------------------------------------------------------------------------------------------------
def unit(v):
    with np.errstate(all="ignore"):
        return (v / np.sqrt((v.astype(np.float64) ** 2).sum(1))[:, None]).astype(f32)


def free_points(g, n=N_FREE, seed=0x901E75):
    """n seeded points inside the box of the camera's first hits (clipped to +-20 per axis: planes run to the horizon) with normals of
    every kind -- unit, zero, of length 3 (longer than any source copy was built for), with a NaN component, axis-aligned with -0
    components -- and a view record per point: a unit direction and ns drawn from {0, 1, 5, 50}.  Some P carry a -0 component too."""
    cam = U.primary_rays(g)
    s = surface(g, cam)
    pos = s["position"][s["hits"][:, 0] > 0]
    lo, hi = np.clip(pos.min(0), -20, 20), np.clip(pos.max(0), -20, 20)
    rng = np.random.default_rng(seed)
    P = rng.uniform(lo - 0.5, hi + 0.5, (n, 3)).astype(f32)
    N = unit(rng.normal(size=(n, 3)).astype(f32))
    kind = np.arange(n) % 16
    N[kind == 11] = 0
    N[kind == 12] *= f32(3)
    N[kind == 13, rng.integers(0, 3)] = np.nan
    axes = np.array([[-0.0, 1, -0.0], [1, -0.0, -0.0], [-0.0, -0.0, -1], [-0.0, -1, 0.0]], f32)
    N[kind == 14] = axes[rng.integers(0, 4, (kind == 14).sum())]
    P[kind == 15, 0] = f32(-0.0)
    V = unit(rng.normal(size=(n, 3)).astype(f32))
    ns = np.array([0, 1, 5, 50], f32)[rng.integers(0, 4, n)]
    return np.ascontiguousarray(np.concatenate([P, N], 1), f32), np.ascontiguousarray(np.concatenate([V, ns[:, None]], 1), f32)


def restated(g, path, points, view):
    """tests/util_points' five channels for `points` in Scene g, whose lights are those of the scene file `path`: the lights as the
    device holds them, illuminate from the oracle, visibility from Scene.occluded (source class 0)."""
    from oracle import oracle as O
    o = O.OracleScene(path, g.width, g.height)
    plan = UP.PointPlan(o, g.device_lights(), points, view, bias=AO.BIAS)
    o.close()
    occ = g.occluded(dev(plan.shadow_rays), dev(plan.shadow_tmax)) if len(plan.shadow_rays) else torch.zeros(0, dtype=torch.uint8)
    torch.cuda.synchronize()
    occ = occ.cpu().numpy()
    return plan.reduce(occ), plan, occ


_free = {}


def free_case(ra, family, name):
    """The free points of a scene with their restated channels, computed once and shared read-only"""
    if name not in _free:
        w, h = UL.size_of(name)
        path = path_of(name, family)
        g = ra.Scene(path, w, h)
        points, view = free_points(g)
        exp, plan, occ = restated(g, path, points, view)
        g.close()
        for a in [points, view] + list(exp.values()):
            a.setflags(write=False)
        _free[name] = dict(path=path, size=(w, h), points=points, view=view, exp=exp, classes=plan.classes(occ))
    return _free[name]


def differing(got, exp, n, channels):
    return {c: int((U.bits(got[c]) != U.bits(exp[c])).reshape(n, -1).any(1).sum()) for c in UP.same(got, exp, channels)}


@pytest.mark.parametrize("name", FREE_SCENES)
def test_free_points_equal_the_restatement(ra, family, name):
    c = free_case(ra, family, name)
    g = ra.Scene(c["path"], *c["size"])
    n = len(c["points"])
    got = light_points(g, c["points"], c["view"])
    lit, shadowed, away, total = c["classes"]
    print("%s: %d free points, %d pairs: lit %.3f, shadowed while facing %.3f, turned away %.3f" % (
        name, n, total, lit / total, shadowed / total, away / total))
    assert min(lit, shadowed, away) > 0
    bad = differing(got, c["exp"], n, CH)
    assert not bad, "%s: points whose channels differ from the restatement: %s" % (name, bad)
    assert np.array_equal(U.bits(UL.in_order_sum(got["light_diffuse"])), U.bits(got["diffuse"]))
    assert np.array_equal(U.bits(UL.in_order_sum(got["light_specular"])), U.bits(got["specular"]))
    # the sums alone (pairs that cannot matter are not walked); without a view the diffuse channels are the same
    assert not UP.same(light_points(g, c["points"], c["view"], per_light=False), c["exp"], UP.SUMS)
    blind = light_points(g, c["points"], None)
    assert not differing(blind, c["exp"], n, ("diffuse", "light_diffuse", "light_open"))
    g.close()


# ---- 3. far points: the guard of the source copies ------------------------------------------------------------------------------------------
def test_far_points_equal_the_restatement(ra):
    name = "cfg2_smooth_4k"             # three point lights, each with a source copy of the mesh's prune records
    path = "scenes/%s.scene" % name
    g = ra.Scene(path, *UL.size_of(name))
    rng = np.random.default_rng(0xFA2)
    out = unit(rng.normal(size=(256, 3)).astype(f32))
    dist = np.array([1e3, 1e6, 1e30], f32)[np.arange(256) % 3]
    P = (f32([0, 0, -3]) + out * dist[:, None]).astype(f32)                 # the mesh sits at (0, 0, -3)
    N = np.where((np.arange(256) % 2 == 0)[:, None], -out, unit(rng.normal(size=(256, 3)).astype(f32))).astype(f32)
    points = np.ascontiguousarray(np.concatenate([P, N], 1), f32)
    view = np.ascontiguousarray(np.concatenate([out, np.full((256, 1), 5, f32)], 1), f32)
    exp, plan, occ = restated(g, path, points, view)
    got = light_points(g, points, view)
    print("far points: %d of %d shadow rays occluded; open pairs %d of %d" % (occ.sum(), len(occ), (got["light_open"] > 0).sum(), got["light_open"].size))
    assert occ.any() and not occ.all()
    bad = differing(got, exp, 256, CH)
    assert not bad, "far points whose channels differ from the restatement: %s" % bad
    g.close()


# ---- 4. ambient occlusion ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cull", [1, 0])
@pytest.mark.parametrize("name", ["cfg1_simple_shapes", "cfg2_smooth_4k", "mixed_materials", "mixed_nrm"])
def test_ao_points_at_the_camera_hits_is_render_ao(ra, family, name, cull):
    w, h = UL.size_of(name)
    g = ra.Scene(path_of(name, family), w, h)
    g.set_flag("useBackfaceCulling", cull)
    cam = U.primary_rays(g)
    s = surface(g, cam)
    hit = (s["hits"][:, 0] > 0) & U.written_mask(w, h).reshape(-1)
    points = np.concatenate([s["position"][hit], s["normal"][hit]], 1).astype(f32)
    dirs = dev(AO.DIRS19)
    seen = {}
    for radius in (float("inf"), RADIUS):
        ao = torch.full((h, w), FILL, dtype=torch.float32, device="cuda")
        counts = torch.full((h, w), -3, dtype=torch.int32, device="cuda")
        g.render_ao(dirs, radius, ao=ao, counts=counts)
        torch.cuda.synchronize()
        got_c, got_a = ao_points(g, points, AO.DIRS19, radius)
        want_c = counts.cpu().numpy().reshape(-1)[hit].view(np.uint32)
        want_a = ao.cpu().numpy().reshape(-1)[hit]
        assert np.array_equal(got_c, want_c), "%s cull %d radius %s: %d counts differ" % (name, cull, radius, (got_c != want_c).sum())
        assert np.array_equal(U.bits(got_a), U.bits(want_a))
        seen[radius] = got_c
    changed = (seen[float("inf")] != seen[RADIUS]).sum()
    print("%s cull %d: %d points, %d whose counts change with the radius" % (name, cull, hit.sum(), changed))
    assert hit.sum() >= 0.10 * len(cam) and changed > 0
    g.close()


@pytest.mark.parametrize("name", FREE_SCENES)
def test_ao_of_free_points_equals_the_restatement(ra, family, name):
    c = free_case(ra, family, name)
    g = ra.Scene(c["path"], *c["size"])
    points = c["points"]
    traced, pt, k, rays = UP.ao_traced_rays(points, AO.DIRS19)
    for radius in (float("inf"), RADIUS):
        occ = g.occluded(dev(rays), radius)
        torch.cuda.synchronize()
        want_c, want_a = UP.ao_reduce(traced, pt, occ.cpu().numpy())
        got_c, got_a = ao_points(g, points, AO.DIRS19, radius)
        assert np.array_equal(got_c, want_c), "%s radius %s: %d counts differ" % (name, radius, (got_c != want_c).sum())
        assert np.array_equal(U.bits(got_a), U.bits(want_a))
    zero = ~points[:, 3:6].any(1)
    assert zero.sum() >= 100 and (got_c[zero] == 0).all() and (got_a[zero] == f32(1.0)).all()
    assert ((got_c & 0xFFFF) < (got_c >> 16)).any() and (got_c & 0xFFFF).any()
    only = g.ao_points(dev(points), dev(AO.DIRS19), counts=True, ao=False)
    assert set(only) == {"counts"}
    assert set(g.ao_points(dev(points), dev(AO.DIRS19))) == {"ao"}
    torch.cuda.synchronize()
    g.close()


# ---- 5. batches and order ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reorder", [0, 1])
@pytest.mark.parametrize("name", ["cfg2_smooth_4k", "area_light"])
def test_points_are_independent_of_their_batch(ra, family, name, reorder):
    c = free_case(ra, family, name)
    g = ra.Scene(c["path"], *c["size"])
    hit, at_p, at_v = points_at_hits(g, np.concatenate(first_hit_rays(g)))
    pool, view = np.concatenate([c["points"], at_p]), np.concatenate([c["view"], at_v])
    n = len(pool)

    def both(sl):
        out = light_points(g, pool[sl], view[sl])
        out["counts"], out["ao"] = ao_points(g, pool[sl], AO.DIRS19, RADIUS)
        return out

    all_ch = CH + ("counts", "ao")
    want = both(slice(None))                   # (the default: no grouping at these sizes)
    assert not differing({k: want[k][:N_FREE] for k in CH}, c["exp"], N_FREE, CH)
    g.set_knob("trace_reorder", reorder)       # (1: the sort runs on every batch, however small)
    rng = np.random.default_rng(11)
    perm = rng.permutation(n)
    assert not UP.same(both(perm), {k: want[k][perm] for k in all_ch}, all_ch), "a shuffled batch, reorder %d" % reorder
    half = n // 2 + 7
    a, b = both(slice(0, half)), both(slice(half, n))
    assert not UP.same({k: np.concatenate([a[k], b[k]]) for k in all_ch}, want, all_ch), "the batch split in two, reorder %d" % reorder
    for m in (1, 63, 64, 65):
        first = int(rng.integers(0, n - m))
        sl = slice(first, first + m)
        bad = UP.same(both(sl), {k: want[k][sl] for k in all_ch}, all_ch)
        assert not bad, "n = %d, reorder %d: %s" % (m, reorder, bad)
    out = g.light_points(dev(pool[:0]), dev(view[:0]), per_light=True)
    L = g.n_lights
    assert [tuple(out[k].shape) for k in CH] == [(0, 3), (0, 3), (0, L, 3), (0, L, 3), (0, L)] and out["light_open"].dtype == torch.int32
    assert g.ao_points(dev(pool[:0]), dev(AO.DIRS19), counts=True)["counts"].shape == (0,)
    g.close()


# ---- 6. only what is asked for is written (the C entries, directly) ------------------------------------------------------------------------
def tail_of(c, L):
    return {"hits": (8,), "diffuse": (3,), "specular": (3,), "light_diffuse": (L, 3), "light_specular": (L, 3), "light_open": (L,),
            "ao": (), "counts": ()}[c]


class Buffers:
    """The channels of n points and L lights (and the hit records no call may write), each in the middle of a larger pre-filled
    allocation; light_open and counts are read as the integers of their bits."""
    ALL = ("hits",) + CH + ("ao", "counts")

    def __init__(self, n, L):
        self.n, self.L = n, L
        self.flat, self.ptr = {}, {}
        for c in self.ALL:
            size = n * int(np.prod(tail_of(c, L), dtype=np.int64))
            self.flat[c] = torch.full((size + 2 * GUARD,), FILL, dtype=torch.float32, device="cuda")
            self.ptr[c] = self.flat[c].data_ptr() + 4 * GUARD

    def struct(self, ra, names, n_lights=None):
        return ra.LightBuffers(self.L if n_lights is None else n_lights, *[self.ptr[c] if c in names else None for c in ("hits",) + CH])

    def read(self):
        torch.cuda.synchronize()
        out = {}
        for c in self.ALL:
            f = self.flat[c].cpu().numpy()
            assert (f[:GUARD] == f32(FILL)).all() and (f[-GUARD:] == f32(FILL)).all(), "%s: written outside the buffer" % c
            a = f[GUARD:len(f) - GUARD].reshape((self.n,) + tail_of(c, self.L))
            out[c] = a.view(np.int32) if c == "light_open" else (a.view(np.uint32) if c == "counts" else a)
        return out

    def all_untouched(self):
        return all(untouched(a) for a in self.read().values())


def untouched(a):
    return (np.ascontiguousarray(a).view(np.uint32) == np.array(FILL, f32).view(np.uint32)).all()


def stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def call_light(ra, g, tp, tv, bufs, names, n_lights=None, n=None):
    rtx, _ = ra.load()
    s = bufs.struct(ra, names, n_lights)
    return rtx.rtx_light_points(g.gpu(), tp.shape[0] if n is None else n, C.c_void_p(tp.data_ptr()) if tp is not None else None,
                                C.c_void_p(tv.data_ptr()) if tv is not None else None, C.byref(s), stream_ptr())


def call_ao(ra, g, tp, td, bufs, names, n_dirs=None, radius=RADIUS, n=None):
    rtx, _ = ra.load()
    par = ra.AoParams(td.shape[0] if n_dirs is None else n_dirs, td.data_ptr(), radius)
    return rtx.rtx_ao_points(g.gpu(), tp.shape[0] if n is None else n, C.c_void_p(tp.data_ptr()) if tp is not None else None, C.byref(par),
                             C.c_void_p(bufs.ptr["ao"]) if "ao" in names else None, C.c_void_p(bufs.ptr["counts"]) if "counts" in names else None,
                             stream_ptr())


@pytest.mark.parametrize("name", ["area_light", "cfg2_smooth_4k"])
def test_only_what_was_asked_for_is_written(ra, family, name):
    c = free_case(ra, family, name)
    g = ra.Scene(c["path"], *c["size"])
    points, view = c["points"][:-1], c["view"][:-1]
    n = len(points)
    tp, tv, td = dev(points), dev(view), dev(AO.DIRS19)
    b = Buffers(n, g.n_lights)
    assert call_light(ra, g, tp, tv, b, CH) == 0 and call_ao(ra, g, tp, td, b, ("ao", "counts")) == 0
    full = b.read()
    assert untouched(full["hits"])
    assert not differing(full, {k: v[:-1] for k, v in c["exp"].items()}, n, CH)
    for names in [(k,) for k in CH] + [UP.SUMS, ("diffuse", "light_open"), ("specular", "light_diffuse")]:
        b = Buffers(n, g.n_lights)
        assert call_light(ra, g, tp, tv, b, names) == 0
        got = b.read()
        for k in Buffers.ALL:
            if k in names:
                assert np.array_equal(U.bits(got[k]), U.bits(full[k])), "%s of a call for %s differs from the five-channel call" % (k, names)
            else:
                assert untouched(got[k]), "%s was written by a call for %s" % (k, names)
    # without a view: the diffuse channels are the same, and no specular buffer is written
    b = Buffers(n, g.n_lights)
    assert call_light(ra, g, tp, None, b, ("diffuse", "light_diffuse", "light_open")) == 0
    got = b.read()
    assert all(np.array_equal(U.bits(got[k]), U.bits(full[k])) for k in ("diffuse", "light_diffuse", "light_open"))
    assert all(untouched(got[k]) for k in ("hits", "specular", "light_specular", "ao", "counts"))
    assert set(g.light_points(tp)) == {"diffuse"} and set(g.light_points(tp, tv, diffuse=False)) == {"specular"}
    assert set(g.light_points(tp, tv, specular=False, per_light=True)) == {"diffuse", "light_diffuse", "light_open"}
    for names in (("ao",), ("counts",)):
        b = Buffers(n, g.n_lights)
        assert call_ao(ra, g, tp, td, b, names) == 0
        got = b.read()
        for k in Buffers.ALL:
            if k in names:
                assert np.array_equal(U.bits(got[k]), U.bits(full[k]))
            else:
                assert untouched(got[k]), "%s was written by a call for %s" % (k, names)
    torch.cuda.synchronize()
    g.close()


# ---- 7. scene state and refusals --------------------------------------------------------------------------------------------------------------
def state_rays(g):
    return np.concatenate(first_hit_rays(g) + (SU.probe_rays()[:1024],))


def test_edited_lights(ra, family):
    """set_light, add_light up to seven point lights (one more than have a source copy), remove_light down to none: after every step
    light_points at the hits is light_rays (which tests/test_gpu_light_rays.py holds against a fresh scene and the restatement)"""
    c = free_case(ra, family, "cfg2_smooth_4k")
    g = ra.Scene(c["path"], *c["size"])
    rays = state_rays(g)
    assert identity_with_light_rays(g, rays, "as loaded") > 500
    g.set_light(1, position=(1.5, 0.5, -1.5), intensity=0.9)
    identity_with_light_rays(g, rays, "set_light")
    spots = [(2.5, 1.5, -3), (-2.5, 1.0, -2), (0.3, 3.0, -4.5), (-0.8, 0.5, -0.5)]
    for k, pos in enumerate(spots):
        g.add_light("point", position=pos, color=(0.9 - 0.1 * k, 0.3 + 0.1 * k, 0.5), intensity=0.4 + 0.2 * k)
    assert g.n_lights == 7
    identity_with_light_rays(g, rays, "seven point lights")
    points, view = c["points"], c["view"]
    seven = light_points(g, points, view)
    assert seven["light_open"].shape == (N_FREE, 7)
    for li in range(7):
        col = seven["light_open"][:, li]
        assert col.any() and not col.all(), "light %d is open for every point or for none" % li
    # a per-light buffer sized for another number of lights is refused and stays untouched; the sums need no count
    tp, tv = dev(points), dev(view)
    b = Buffers(N_FREE, 3)
    rtx, _ = ra.load()
    assert call_light(ra, g, tp, tv, b, CH) == -1 and b"n_lights" in rtx.rtx_last_error()
    assert b.all_untouched()
    assert call_light(ra, g, tp, tv, b, UP.SUMS) == 0
    assert not UP.same(b.read(), seven, UP.SUMS)
    while g.n_lights:
        g.remove_light(g.n_lights - 1)
        if g.n_lights in (6, 2):
            identity_with_light_rays(g, rays, "%d lights" % g.n_lights)
    # no lights: the sums are +0, and per-light buffers are refused whatever n_lights says
    dark = light_points(g, points, view)
    assert not dark["diffuse"].view(np.uint32).any() and not dark["specular"].view(np.uint32).any()
    assert dark["light_diffuse"].shape == (N_FREE, 0, 3) and dark["light_open"].shape == (N_FREE, 0)
    b = Buffers(N_FREE, 1)
    for nl in (0, 1):
        assert call_light(ra, g, tp, tv, b, CH, n_lights=nl) == -1
    assert b.all_untouched()
    g.close()


def test_after_move_object(ra):
    name = "mixed_materials"
    g = ra.Scene("scenes/%s.scene" % name, 40, 24)
    identity_with_light_rays(g, SU.probe_rays()[:500], "before")
    for k, (index, keys) in enumerate([(3, dict(pos=(0.4, 1.2, -5.5), radius=0.85)), (1, dict(rot=(-40, 10, 70), pos=(-0.9, 0.2, -4.4)))]):
        g.move_object(index, **keys)
        assert identity_with_light_rays(g, state_rays(g), "move %d" % k) > 500
    g.close()


def test_flags_depth_and_counters_change_nothing(ra, family, tmp_path):
    name = "cfg2_smooth_4k"
    c = free_case(ra, family, name)
    g = ra.Scene(c["path"], *c["size"])
    points, view, exp = c["points"], c["view"], c["exp"]
    want_c, want_a = ao_points(g, points, AO.DIRS19, RADIUS)

    def check(s, what):
        assert not differing(light_points(s, points, view), exp, N_FREE, CH), what
        got_c, got_a = ao_points(s, points, AO.DIRS19, RADIUS)
        assert np.array_equal(got_c, want_c) and np.array_equal(U.bits(got_a), U.bits(want_a)), what

    g.set_flag("showNormals", 1)
    check(g, "showNormals")
    g.set_flag("showNormals", 0)
    f = ra.Scene(scene_copy(name, str(tmp_path), dict(max_ray_depth=0)), *c["size"])
    check(f, "max_ray_depth = 0")
    f.close()
    g.counters_enable(True)
    g.counters_reset()
    check(g, "counters enabled")
    assert not g.counters().any()
    g.counters_enable(False)
    g.close()


@pytest.mark.parametrize("as_current", [False, True])
def test_points_written_on_another_stream(ra, family, as_current):
    c = free_case(ra, family, "cfg2_smooth_4k")
    g = ra.Scene(c["path"], *c["size"])
    want_c, want_a = ao_points(g, c["points"], AO.DIRS19, RADIUS)
    src_p, src_v, dirs = dev(c["points"]), dev(c["view"]), dev(AO.DIRS19)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    for _ in range(2):
        with torch.cuda.stream(st):
            tp = torch.full_like(src_p, float("nan"))       # (written on st: a call that did not wait for the copy would read NaNs)
            tp.copy_(src_p)
            tv = torch.full_like(src_v, float("nan"))
            tv.copy_(src_v)
            kw = {} if as_current else dict(stream=st)
            out = g.light_points(tp, tv, per_light=True, **kw)
            occ = g.ao_points(tp, dirs, RADIUS, counts=True, **kw)
        st.synchronize()
        assert not differing({k: v.cpu().numpy() for k, v in out.items()}, c["exp"], N_FREE, CH), "stream, as current %s" % as_current
        assert np.array_equal(occ["counts"].cpu().numpy().view(np.uint32), want_c) and np.array_equal(U.bits(occ["ao"].cpu().numpy()), U.bits(want_a))
    g.close()


def test_refusals_leave_the_buffers_untouched(ra, family):
    c = free_case(ra, family, "cfg2_smooth_4k")
    g = ra.Scene(c["path"], *c["size"])
    rtx, _ = ra.load()
    points, view = c["points"][:1000], c["view"][:1000]
    tp, tv, td = dev(points), dev(view), dev(AO.DIRS19)
    with pytest.raises(ValueError, match="light_points: nothing to compute"):
        g.light_points(tp, tv, diffuse=False, specular=False)
    with pytest.raises(ValueError, match="light_points: specular needs a view"):
        g.light_points(tp, specular=True)
    with pytest.raises(ValueError, match=r"light_points: view must have shape \(1000, 4\)"):
        g.light_points(tp, tv[:999])
    b = Buffers(len(points), g.n_lights)
    L = g.n_lights
    refused = [
        ("no output", lambda: call_light(ra, g, tp, tv, b, ())),
        ("hits_dev set", lambda: call_light(ra, g, tp, tv, b, ("hits",) + CH)),
        ("hits_dev alone", lambda: call_light(ra, g, tp, tv, b, ("hits",))),
        ("specular without a view", lambda: call_light(ra, g, tp, None, b, ("diffuse", "specular"))),
        ("light_specular without a view", lambda: call_light(ra, g, tp, None, b, ("light_specular",))),
        ("one light too many", lambda: call_light(ra, g, tp, tv, b, CH, n_lights=L + 1)),
        ("one light too few", lambda: call_light(ra, g, tp, tv, b, ("light_open",), n_lights=L - 1)),
        ("n = 0xFFFFFFC1", lambda: call_light(ra, g, tp, tv, b, CH, n=0xFFFFFFC1)),
        ("NULL points", lambda: call_light(ra, g, None, tv, b, CH, n=len(points))),
        ("NULL out", lambda: rtx.rtx_light_points(g.gpu(), len(points), C.c_void_p(tp.data_ptr()), C.c_void_p(tv.data_ptr()), None, stream_ptr())),
        ("ao: no output", lambda: call_ao(ra, g, tp, td, b, ())),
        ("ao: n_dirs 0", lambda: call_ao(ra, g, tp, td, b, ("ao", "counts"), n_dirs=0)),
        ("ao: n_dirs 257", lambda: call_ao(ra, g, tp, td, b, ("ao", "counts"), n_dirs=257)),
        ("ao: radius 0", lambda: call_ao(ra, g, tp, td, b, ("ao", "counts"), radius=0.0)),
        ("ao: radius NaN", lambda: call_ao(ra, g, tp, td, b, ("ao", "counts"), radius=float("nan"))),
        ("ao: radius < 0", lambda: call_ao(ra, g, tp, td, b, ("ao", "counts"), radius=-1.0)),
        ("ao: n = 0xFFFFFFC1", lambda: call_ao(ra, g, tp, td, b, ("ao", "counts"), n=0xFFFFFFC1)),
        ("ao: NULL points", lambda: call_ao(ra, g, None, td, b, ("ao", "counts"), n=len(points))),
        ("ao: NULL params", lambda: rtx.rtx_ao_points(g.gpu(), len(points), C.c_void_p(tp.data_ptr()), None, C.c_void_p(b.ptr["ao"]), None, stream_ptr())),
        ("ao: NULL dirs", lambda: rtx.rtx_ao_points(g.gpu(), len(points), C.c_void_p(tp.data_ptr()), C.byref(ra.AoParams(19, None, 1.0)),
                                                    C.c_void_p(b.ptr["ao"]), None, stream_ptr())),
    ]
    for what, fn in refused:
        assert fn() == -1, what                 # RTX_ERR_ARG
        assert rtx.rtx_last_error(), what
    assert call_light(ra, g, None, tv, b, CH, n=0) == 0 and call_ao(ra, g, None, td, b, ("ao",), n=0) == 0      # n == 0: nothing to do
    assert b.all_untouched()
    # ... and the calls work afterwards; the sums ignore n_lights
    assert call_light(ra, g, tp, tv, b, UP.SUMS, n_lights=99) == 0 and call_ao(ra, g, tp, td, b, ("counts",)) == 0
    got = b.read()
    assert not differing(got, {k: v[:1000] for k, v in c["exp"].items()}, 1000, UP.SUMS)
    assert all(untouched(got[k]) for k in ("hits", "ao") + UP.PER_LIGHT) and not untouched(got["counts"])
    g.close()
