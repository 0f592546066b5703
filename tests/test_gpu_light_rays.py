"""rtx_light_rays / Scene.light_rays (include/rtx_light.h): castRay's sums over the lights at the hits of caller-supplied rays, each
light's terms and the number of its shadow rays that arrive.  Every comparison is bit for bit over every ray:
  the colour identities -- trace_rays' colour of a Diffuse hit is albedo * diffuse, of a Phong hit (albedo * ambient + diffuse * kd) +
      specular * ks, with albedo, ks and hits from surface_rays and the object constants from device_objects();
  the per-light channels against tests/util_light's restatement (pinned to the oracle by tests/test_light_rays_cpu.py) with the exact N
      from surface_rays and the visibility from Scene.occluded -- neither is the code under test;
  across batches, orders and sizes; only what is asked for is written; scene edits, flags, counters, streams, refusals.

Ray sets: (A) the view's camera rays, (B) bounce rays from their hits, (D) seeded probe rays (tests/util_surface.py)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import util_ao as AO
from tests import util_aov as U
from tests import util_light as UL
from tests import util_lights as LE
from tests import util_shading as S
from tests import util_surface as SU
from tests.ac_heatmap import scene_copy

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = U.ROOT
f32 = np.float32
GUARD = 96                    # untouched elements before and after every buffer
FILL = 7.25
CH = UL.CHANNELS
SUMS = ("diffuse", "specular")
PER_LIGHT = ("light_diffuse", "light_specular", "light_open")


@pytest.fixture(scope="module")
def family(tmp_path_factory):
    d = S.short_dir(tmp_path_factory)
    return d, S.write_family(d)


def path_of(name, family):
    return family[1][name] if name in S.FAMILY else "scenes/%s.scene" % name


def dev(a, dtype=f32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def light(g, rays, hits=True, per_light=True, stream=None):
    """channel -> numpy array of Scene.light_rays for a numpy ray array"""
    out = g.light_rays(dev(rays), hits=hits, per_light=per_light, stream=stream)
    torch.cuda.synchronize()
    assert set(out) == set(SUMS + (("hits",) if hits else ()) + (PER_LIGHT if per_light else ()))
    return {c: t.cpu().numpy() for c, t in out.items()}


def first_hit_rays(g):
    """(A) and (B) of Scene g"""
    cam, depth, normal, hit = AO.first_hits(g)
    return cam, SU.bounce_rays(cam, depth, normal, hit)


def surface(g, rays):
    out = g.surface_rays(dev(rays), hits=True, normal=True, albedo=True, specular=True)
    torch.cuda.synchronize()
    return {c: t.cpu().numpy() for c, t in out.items()}


def expectation(g, path, rays):
    """tests/util_light's channels of `rays` in Scene g, whose lights and objects are those of the scene file `path`: hits and the exact N
    from surface_rays, the lights and n_specular as the device holds them, illuminate from the oracle, visibility from Scene.occluded."""
    from oracle import oracle as O
    s = surface(g, rays)
    objs, _ = g.device_objects()
    o = O.OracleScene(path, g.width, g.height)
    plan = UL.Plan(o, g.device_lights(), rays, s["hits"], s["normal"], bias=AO.BIAS)
    o.close()
    occ = g.occluded(dev(plan.shadow_rays), dev(plan.shadow_tmax)) if len(plan.shadow_rays) else torch.zeros(0, dtype=torch.uint8)
    torch.cuda.synchronize()
    obj = s["hits"][:, 1].astype(np.int32)
    ns = np.where(obj >= 0, objs["n_specular"][np.maximum(obj, 0)], f32(0)).astype(f32)
    e = plan.reduce(occ.cpu().numpy(), ns)
    e["hits"] = s["hits"]
    return e


# ---- 1. the colour identities -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cull", [1, 0])
@pytest.mark.parametrize("name", UL.SCENES)
def test_sums_make_the_colours_of_diffuse_and_phong_hits(ra, family, name, cull):
    w, h = UL.size_of(name)
    g = ra.Scene(path_of(name, family), w, h)
    g.set_flag("useBackfaceCulling", cull)
    objs, _ = g.device_objects()
    cam, bounce = first_hit_rays(g)
    for what, rays in (("A", cam), ("B", bounce), ("D", SU.probe_rays())):
        got = light(g, rays, per_light=False)
        s = surface(g, rays)
        _, colours = g.trace_rays(dev(rays), hits=False)
        torch.cuda.synchronize()
        colours = colours.cpu().numpy()
        assert np.array_equal(U.bits(got["hits"]), U.bits(s["hits"]))
        obj = s["hits"][:, 1].astype(np.int32)
        rec = objs[np.maximum(obj, 0)]
        material = np.where(obj >= 0, rec["material"], -1)
        is_dp, want = UL.colour_identities(colours, s["albedo"], s["specular"], got["diffuse"], got["specular"], material,
                                           rec["ambient"], rec["diffuse"])
        bad = is_dp & (U.bits(want) != U.bits(colours)).any(-1)
        print("%s %dx%d cull %d (%s): %d Diffuse and %d Phong hits of %d rays, %d differ" % (
            name, w, h, cull, what, (material == 0).sum(), (material == 3).sum(), len(rays), bad.sum()))
        if what == "A" and name != "cfg3_reflective_refractive":
            assert is_dp.mean() >= 0.10
        assert not bad.any(), "%s cull %d (%s): %d of %d Diffuse / Phong hits whose sums do not make trace_rays' colour" % (
            name, cull, what, bad.sum(), is_dp.sum())
        miss = obj < 0
        assert not got["diffuse"][miss].view(np.uint32).any() and not got["specular"][miss].view(np.uint32).any()
    g.close()


# ---- 2. the per-light channels against the restated contract ------------------------------------------------------------------------------
@pytest.mark.parametrize("cull", [1, 0])
@pytest.mark.parametrize("name", UL.SCENES)
def test_per_light_channels_equal_the_expectation(ra, family, name, cull):
    w, h = UL.size_of(name)
    path = path_of(name, family)
    g = ra.Scene(path, w, h)
    g.set_flag("useBackfaceCulling", cull)
    cam, bounce = first_hit_rays(g)
    for what, rays in (("A", cam), ("B", bounce), ("D", SU.probe_rays())):
        got = light(g, rays)
        exp = expectation(g, path, rays)
        bad = UL.same(got, exp, CH)
        assert not bad, "%s %dx%d cull %d (%s): channels that differ from the expectation: %s" % (name, w, h, cull, what, {
            c: int((U.bits(got[c]) != U.bits(exp[c])).reshape(len(rays), -1).any(1).sum()) for c in bad})
        # the sums are the in-order sums of the per-light terms
        assert np.array_equal(U.bits(UL.in_order_sum(got["light_diffuse"])), U.bits(got["diffuse"]))
        assert np.array_equal(U.bits(UL.in_order_sum(got["light_specular"])), U.bits(got["specular"]))
        miss = got["hits"][:, 0] == 0
        assert not got["light_open"][miss].any()
        if what == "A" and name in UL.SHARED_OUT:
            assert got["light_open"].any() and (got["light_open"][~miss] == 0).any()
    g.close()


# ---- 3. batches and order --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reorder", [0, 1])
@pytest.mark.parametrize("name", ["cfg2_smooth_4k", "area_light", "cfg1_simple_shapes"])
def test_rays_are_independent_of_their_batch(ra, name, reorder):
    w, h = UL.size_of(name)
    g = ra.Scene("scenes/%s.scene" % name, w, h)
    cam, bounce = first_hit_rays(g)
    pool = np.concatenate([cam, bounce, SU.probe_rays()[:1500]])
    want = light(g, pool)                      # (the default: no grouping at these sizes)
    g.set_knob("trace_reorder", reorder)       # (1: the sort runs on every batch, however small)
    rng = np.random.default_rng(11)
    perm = rng.permutation(len(pool))
    got = light(g, pool[perm])
    assert not UL.same(got, {c: want[c][perm] for c in CH}, CH), "a shuffled batch, reorder %d" % reorder
    half = len(pool) // 2 + 7
    a, b = light(g, pool[:half]), light(g, pool[half:])
    assert not UL.same({c: np.concatenate([a[c], b[c]]) for c in CH}, want, CH), "the batch split in two, reorder %d" % reorder
    for n in (1, 63, 64, 65):
        first = int(rng.integers(0, len(cam) - n))
        sl = slice(first, first + n)
        bad = UL.same(light(g, pool[sl]), {c: want[c][sl] for c in CH}, CH)
        assert not bad, "n = %d, reorder %d: %s" % (n, reorder, bad)
    out = g.light_rays(dev(pool[:0]), hits=True, per_light=True)
    L = g.n_lights
    assert [tuple(out[c].shape) for c in CH] == [(0, 8), (0, 3), (0, 3), (0, L, 3), (0, L, 3), (0, L)]
    assert out["light_open"].dtype == torch.int32
    g.close()


# ---- 4. only what is asked for is written (the C entry, directly) ------------------------------------------------------------------------
def tail_of(c, L):
    return {"hits": (8,), "diffuse": (3,), "specular": (3,), "light_diffuse": (L, 3), "light_specular": (L, 3), "light_open": (L,)}[c]


class Buffers:
    """The six channels of n rays and L lights, each in the middle of a larger pre-filled allocation (light_open: int32 of FILL's bits)."""

    def __init__(self, n, L):
        self.n, self.L = n, L
        self.flat, self.ptr = {}, {}
        for c in CH:
            size = n * int(np.prod(tail_of(c, L), dtype=np.int64))
            self.flat[c] = torch.full((size + 2 * GUARD,), FILL, dtype=torch.float32, device="cuda")
            self.ptr[c] = self.flat[c].data_ptr() + 4 * GUARD

    def struct(self, ra, names, n_lights=None):
        return ra.LightBuffers(self.L if n_lights is None else n_lights, *[self.ptr[c] if c in names else None for c in CH])

    def read(self):
        """channel -> numpy array (n, ...), after checking the guards; light_open as int32"""
        torch.cuda.synchronize()
        out = {}
        for c in CH:
            f = self.flat[c].cpu().numpy()
            assert (f[:GUARD] == f32(FILL)).all() and (f[-GUARD:] == f32(FILL)).all(), "%s: written outside the buffer" % c
            a = f[GUARD:len(f) - GUARD].reshape((self.n,) + tail_of(c, self.L))
            out[c] = a.view(np.int32) if c == "light_open" else a
        return out


def untouched(a):
    return (np.ascontiguousarray(a).view(np.uint32) == np.array(FILL, f32).view(np.uint32)).all()


def call(ra, g, t, bufs, names, n_lights=None):
    rtx, _ = ra.load()
    s = bufs.struct(ra, names, n_lights)
    return rtx.rtx_light_rays(g.gpu(), t.shape[0], C.c_void_p(t.data_ptr()), C.byref(s), C.c_void_p(torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize("name", ["area_light", "cfg1_simple_shapes"])
def test_only_what_was_asked_for_is_written(ra, name):
    w, h = UL.size_of(name)
    g = ra.Scene("scenes/%s.scene" % name, w, h)
    cam, bounce = first_hit_rays(g)
    rays = np.concatenate([cam, bounce])[:-1]
    t = dev(rays)
    n = len(rays)
    b = Buffers(n, g.n_lights)
    assert call(ra, g, t, b, CH) == 0
    full = b.read()
    assert not UL.same(full, light(g, rays), CH)
    for names in [(c,) for c in CH] + [SUMS, ("hits", "light_open"), ("diffuse", "light_specular")]:
        b = Buffers(n, g.n_lights)
        assert call(ra, g, t, b, names) == 0
        got = b.read()
        for c in CH:
            if c in names:
                assert np.array_equal(U.bits(got[c]), U.bits(full[c])), "%s of a call for %s differs from the six-channel call" % (c, names)
            else:
                assert untouched(got[c]), "%s was written by a call for %s" % (c, names)
    # hits alone is trace_rays' hits; the dict holds exactly what is asked for
    traced, _ = g.trace_rays(t, colours=False)
    torch.cuda.synchronize()
    assert np.array_equal(U.bits(full["hits"]), U.bits(traced.cpu().numpy()))
    only = g.light_rays(t, diffuse=False, specular=False, hits=True)
    assert set(only) == {"hits"} and torch.equal(only["hits"], traced)
    assert set(g.light_rays(t, specular=False)) == {"diffuse"}
    assert set(g.light_rays(t, diffuse=False, specular=False, per_light=True)) == set(PER_LIGHT)
    torch.cuda.synchronize()
    g.close()


# ---- 5. scene state ---------------------------------------------------------------------------------------------------------------------------
def check_against_fresh(ra, g, path, what, expect=True):
    """g's results for (A), (B) and (D) equal those of a scene loaded from `path`, and the expectation."""
    f = ra.Scene(path, g.width, g.height)
    cam, bounce = first_hit_rays(f)
    rays = np.concatenate([cam, bounce, SU.probe_rays()[:1024]])
    got, want = light(g, rays), light(f, rays)
    bad = UL.same(got, want, CH)
    assert not bad, "%s: differs from a fresh scene in %s" % (what, bad)
    if expect:
        assert not UL.same(got, expectation(f, path, rays), CH), "%s: differs from the expectation" % what
    f.close()
    return got


def test_edited_lights_equal_a_fresh_scene(ra, tmp_path):
    name = "area_light"
    w, h = UL.size_of(name)
    text = open(os.path.join(ROOT, "scenes", name + ".scene")).read()
    g = ra.Scene("scenes/%s.scene" % name, w, h)
    rays = SU.probe_rays()[:1000]
    t = dev(rays)
    light(g, rays)
    steps = [("set", 2, dict(position=(-1.5, 2.5, -1.0), intensity=0.9)),
             ("set", 0, dict(samples=2, i=(1.0, 0, 0.2))),
             ("add", "point", dict(position=(0.5, 3.0, -6.0), color=(0.3, 0.9, 0.5), intensity=1.1)),
             ("add", "distant", dict(direction=(0.3, -1.0, -0.2), color=(0.8, 0.8, 0.7), intensity=0.6)),
             ("remove", 1)]
    for k, step in enumerate(steps):
        before = g.n_lights
        text = LE.apply_step(g, text, step)
        if g.n_lights != before:
            # a per-light buffer sized for the old number of lights is refused and stays untouched; the sums need no count
            b = Buffers(len(rays), before)
            assert call(ra, g, t, b, CH) == -1
            rtx, _ = ra.load()
            assert b"n_lights" in rtx.rtx_last_error()
            assert all(untouched(a) for a in b.read().values())
            assert call(ra, g, t, b, ("hits",) + SUMS) == 0
        check_against_fresh(ra, g, LE.write_scene(tmp_path, text, "step%d" % k), "step %d %s" % (k, step[0]))
    g.close()


def test_seven_point_lights(ra, tmp_path):
    """more point lights than have a source copy of the prune records (six): lights 6 and up walk with the general class"""
    name = "cfg2_smooth_4k"
    w, h = UL.size_of(name)
    text = open(os.path.join(ROOT, "scenes", name + ".scene")).read()
    for k in range(LE.n_lights(text) - 1, -1, -1):
        text = LE.remove_light(text, k)
    # around and above the mesh at (0, 0, -3), all above the plane y = -1.5: each is shadowed by the mesh for some hits and open for others
    spots = [(0, 2, -1), (1, -1, -1), (-1, -1, -1), (2.5, 1.5, -3), (-2.5, 1.0, -2), (0.3, 3.0, -4.5), (-0.8, 0.5, -0.5)]
    for k, pos in enumerate(spots):
        text = LE.add_light(text, "point", position=pos, color=(0.9 - 0.1 * k, 0.3 + 0.1 * k, 0.5), intensity=0.4 + 0.2 * k)
    path = LE.write_scene(tmp_path, text, "seven")
    g = ra.Scene(path, w, h)
    assert g.n_lights == 7
    got = check_against_fresh(ra, g, path, "seven point lights")
    hit = got["hits"][:, 0] > 0
    for li in range(7):
        col = got["light_open"][hit, li]
        assert col.any() and not col.all(), "light %d is open for every hit or for none" % li
    g.close()


def test_a_scene_without_lights(ra, tmp_path):
    name = "cfg1_simple_shapes"
    text = open(os.path.join(ROOT, "scenes", name + ".scene")).read()
    for k in range(LE.n_lights(text) - 1, -1, -1):
        text = LE.remove_light(text, k)
    path = LE.write_scene(tmp_path, text, "dark")
    g = ra.Scene(path, 40, 24)
    rays = np.concatenate(first_hit_rays(g))
    got = light(g, rays)
    assert (got["hits"][:, 0] > 0).any()
    assert not got["diffuse"].view(np.uint32).any() and not got["specular"].view(np.uint32).any()
    assert got["light_diffuse"].shape == (len(rays), 0, 3) and got["light_open"].shape == (len(rays), 0)
    # per-light pointers on a scene without lights are refused, whatever n_lights says
    b = Buffers(len(rays), 1)
    t = dev(rays)
    for nl in (0, 1):
        assert call(ra, g, t, b, CH, n_lights=nl) == -1
    assert all(untouched(a) for a in b.read().values())
    # ... and the lights of the live scene removed one by one end in the same state
    live = ra.Scene("scenes/%s.scene" % name, 40, 24)
    light(live, rays)
    while live.n_lights:
        live.remove_light(0)
    assert not UL.same(light(live, rays), got, CH)
    live.close()
    g.close()


@pytest.mark.parametrize("samples", [1, 3])
def test_area_light_samples(ra, tmp_path, samples):
    name = "area_light"
    w, h = UL.size_of(name)
    text = LE.set_light(open(os.path.join(ROOT, "scenes", name + ".scene")).read(), 0, samples=samples)
    path = LE.write_scene(tmp_path, text, "samples%d" % samples)
    g = ra.Scene(path, w, h)
    recs, pts = g.device_lights()
    mine = UL.lights_of_text(text)
    assert np.array_equal(U.bits(pts), U.bits(mine[1])) and list(recs["n_points"]) == list(mine[0]["n_points"]) == [samples * samples, 1, 0]
    got = check_against_fresh(ra, g, path, "samples = %d" % samples)
    hit = got["hits"][:, 0] > 0
    assert got["light_open"][hit, 0].max() == samples * samples
    if samples > 1:
        partly = (got["light_open"][:, 0] > 0) & (got["light_open"][:, 0] < samples * samples)
        assert partly.sum() >= 10, "no hit sees the area light partly"
    g.close()


def test_after_move_object(ra, tmp_path):
    from tests.util_move import edit_scene, write_scene
    name = "mixed_materials"
    w, h = 40, 24
    text = open(os.path.join(ROOT, "scenes", name + ".scene")).read()
    g = ra.Scene("scenes/%s.scene" % name, w, h)
    light(g, SU.probe_rays()[:500])
    for k, (index, keys) in enumerate([(3, dict(pos=(0.4, 1.2, -5.5), radius=0.85)), (1, dict(rot=(-40, 10, 70), pos=(-0.9, 0.2, -4.4)))]):
        g.move_object(index, **keys)
        text = edit_scene(text, index, **keys)
        check_against_fresh(ra, g, write_scene(tmp_path, text, "light_move%d" % k), "move %d" % k)
    g.close()


def test_flags_and_depth_change_nothing(ra, tmp_path):
    name = "cfg4_textured_256"
    w, h = UL.size_of(name)
    g = ra.Scene("scenes/%s.scene" % name, w, h)
    rays = np.concatenate(first_hit_rays(g) + (SU.probe_rays()[:1024],))
    want = light(g, rays)
    g.set_flag("showNormals", 1)
    assert not UL.same(light(g, rays), want, CH), "showNormals changes a channel"
    g.set_flag("showNormals", 0)
    for depth in (0, -1):
        f = ra.Scene(scene_copy(name, str(tmp_path), dict(max_ray_depth=depth)), w, h)
        assert not UL.same(light(f, rays), want, CH), "max_ray_depth = %d" % depth
        f.close()
    g.close()


def test_counters_are_neither_collected_nor_refused(ra):
    g = ra.Scene("scenes/cfg2_smooth_4k.scene", 64, 64)
    rays = SU.probe_rays()
    want = light(g, rays)
    g.counters_enable(True)
    g.counters_reset()
    assert not UL.same(light(g, rays), want, CH), "counters enabled"
    c = g.counters()
    assert not c.any(), c
    g.counters_enable(False)
    g.close()


@pytest.mark.parametrize("as_current", [False, True])
def test_rays_written_on_another_stream(ra, as_current):
    name = "cfg2_smooth_4k"
    w, h = UL.size_of(name)
    g = ra.Scene("scenes/%s.scene" % name, w, h)
    rays = np.concatenate([SU.probe_rays()] * 4)
    want = light(g, rays)
    src = dev(rays)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    for _ in range(2):
        with torch.cuda.stream(st):
            t = torch.full_like(src, float("nan"))       # (written on st: a call that did not wait for the copy would trace NaNs)
            t.copy_(src)
            out = g.light_rays(t, hits=True, per_light=True) if as_current else g.light_rays(t, hits=True, per_light=True, stream=st)
        st.synchronize()
        assert not UL.same({c: v.cpu().numpy() for c, v in out.items()}, want, CH), "stream, as current %s" % as_current
    g.close()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_buffers_untouched(ra):
    g = ra.Scene("scenes/cfg1_simple_shapes.scene", 40, 24)
    rtx, _ = ra.load()
    rays = SU.probe_rays()[:1000]
    t = dev(rays)
    with pytest.raises(ValueError, match="light_rays: nothing to compute"):
        g.light_rays(t, diffuse=False, specular=False)
    b = Buffers(len(rays), g.n_lights)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    # the all-NULL struct, a NULL struct, NULL rays, too many rays, another number of lights
    assert call(ra, g, t, b, ()) == -1
    assert b"NULL" in rtx.rtx_last_error()
    assert rtx.rtx_light_rays(g.gpu(), len(rays), C.c_void_p(t.data_ptr()), None, st) == -1
    s = b.struct(ra, CH)
    assert rtx.rtx_light_rays(g.gpu(), len(rays), None, C.byref(s), st) == -1
    assert rtx.rtx_light_rays(g.gpu(), 0xFFFFFFC1, C.c_void_p(t.data_ptr()), C.byref(s), st) == -1
    assert call(ra, g, t, b, CH, n_lights=g.n_lights + 1) == -1
    assert call(ra, g, t, b, ("light_open",), n_lights=g.n_lights - 1) == -1
    assert rtx.rtx_light_rays(g.gpu(), 0, None, C.byref(s), st) == 0          # n == 0: nothing to do
    assert all(untouched(a) for a in b.read().values())
    # ... and the call works afterwards; the sums ignore n_lights
    assert call(ra, g, t, b, ("hits",) + SUMS, n_lights=99) == 0
    got = b.read()
    want = light(g, rays)
    assert not UL.same(got, want, ("hits",) + SUMS) and all(untouched(got[c]) for c in PER_LIGHT)
    g.close()
