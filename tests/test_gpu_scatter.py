"""rtx_scatter_rays / rtx_sky_rays (include/rtx_scatter.h; Scene.scatter_rays, Scene.sky, Scene.cast_tree): the part of castRay's colour at
the hits of caller-supplied rays that needs no further ray, the reflection and refraction rays, their factors and which of them exist.
Every comparison is bit for bit over every ray:
  every channel against tests/util_scatter's restatement (pinned to the oracle by tests/test_scatter_cpu.py), fed with surface_rays' and
      light_rays' outputs for the same rays and the object constants of device_objects() -- none of them is the code under test;
  hits against trace_rays' records, local against trace_rays' colours where there is no child;
  one level of castRay: trace_rays' colours of the parents are compose() of trace_rays' colours of the children in a scene of the same
      file one level shallower; cast_tree against trace_rays, sky against the oracle;
  across batches, orders and sizes; only what is asked for is written; flags, depth, scene edits, streams, counters, refusals.

Ray sets (tests/util_scatter.py): the view's camera rays; rays that start inside the scene's glass sphere; on the scenes without one the
children and grandchildren of the camera rays, built by the restatement."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import util_aov as U
from tests import util_deform as DF
from tests import util_lights as LE
from tests import util_scatter as SC
from tests import util_shading as S
from tests import util_surface as SU
from tests.ac_heatmap import scene_copy

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = U.ROOT
f32 = np.float32
GUARD = 96                    # untouched elements before and after every buffer
FILL = 7.25
FILL_BYTE = 0xA5
CH = SC.CHANNELS


@pytest.fixture(scope="module")
def family(tmp_path_factory):
    d = S.short_dir(tmp_path_factory)
    return d, S.write_family(d)


def path_of(name, family):
    return family[1][name] if name in S.FAMILY else "scenes/%s.scene" % name


def text_of(path):
    return open(path if os.path.isabs(path) else os.path.join(ROOT, path)).read()


def at_depth(name, family, tmp_path, depth):
    """the scene file of `name` with max_ray_depth = depth"""
    if name in S.FAMILY:
        path = os.path.join(family[0], "%s_gd%d.scene" % (name, depth))
        with open(path, "w") as f:
            f.write(S.scene_text(name, family[0], extra={"max_ray_depth": depth}))
        return path
    return scene_copy(name, str(tmp_path), dict(max_ray_depth=depth))


def dev(a, dtype=f32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def scatter(g, rays, stream=None, **kw):
    """channel -> numpy array of Scene.scatter_rays for a numpy ray array (all six channels unless told otherwise)"""
    kw.setdefault("hits", True)
    out = g.scatter_rays(dev(rays), stream=stream, **kw)
    torch.cuda.synchronize()
    return {c: t.cpu().numpy() for c, t in out.items()}


def colours(g, rays):
    _, c = g.trace_rays(dev(rays), hits=False)
    torch.cuda.synchronize()
    return c.cpu().numpy()


def sky(g, rays):
    c = g.sky(dev(rays))
    torch.cuda.synchronize()
    return c.cpu().numpy()


def constants(g):
    objs, _ = g.device_objects()
    return {k: np.ascontiguousarray(objs[k]) for k in ("material", "ambient", "diffuse", "ior")}


def expectation(g, rays):
    """tests/util_scatter's channels of `rays` in Scene g from surface_rays, light_rays and device_objects(); also "normal" and "material"
    (per ray, -1 at a miss) for the classes"""
    t = dev(rays)
    s = g.surface_rays(t, hits=True, normal=True, albedo=True, specular=True)
    l = g.light_rays(t)
    torch.cuda.synchronize()
    s = {c: v.cpu().numpy() for c, v in s.items()}
    l = {c: v.cpu().numpy() for c, v in l.items()}
    const = constants(g)
    e = SC.restate(rays, s["hits"], s["normal"], s["albedo"], s["specular"], l["diffuse"], l["specular"], const)
    e["hits"] = s["hits"]
    obj = s["hits"][:, 1].astype(np.int32)
    e["normal"] = s["normal"]
    e["material"] = np.where(obj >= 0, const["material"][np.maximum(obj, 0)], -1)
    return e


def ray_sets(g, name):
    """[(what, rays, expectation)] of the scene's ray sets"""
    cam = U.primary_rays(g)
    if name in SC.GLASS_SPHERE:
        return [(what, rays, expectation(g, rays)) for what, rays in (("camera", cam), ("inside", SC.inside_rays(name)))]
    out, rays = [], cam
    for what in ("camera", "children", "grandchildren"):
        out.append((what, rays, expectation(g, rays)))
        rays = SC.children(out[-1][2])[0]
    return out


def pool_of(g, name):
    """the scene's ray sets in one array"""
    return np.concatenate([rays for _, rays, _ in ray_sets(g, name)])


# ---- 1. every channel against the restated contract ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("cull", [1, 0])
@pytest.mark.parametrize("name", SC.SCENES)
def test_channels_equal_the_expectation(ra, family, name, cull):
    w, h = SC.size_of(name)
    g = ra.Scene(path_of(name, family), w, h)
    g.set_flag("useBackfaceCulling", cull)
    total = {}
    for what, rays, exp in ray_sets(g, name):
        got = scatter(g, rays)
        assert got["kinds"].dtype == np.uint8 and all(got[c].shape == (len(rays),) + SC.TAIL[c] for c in CH)
        bad = SC.same(got, exp, CH)
        assert not bad, "%s %dx%d cull %d (%s): channels that differ from the expectation: %s" % (name, w, h, cull, what, {
            c: int((U.bits(got[c]) != U.bits(exp[c])).reshape(len(rays), -1).any(1).sum()) for c in bad})
        hits, col = g.trace_rays(dev(rays))
        torch.cuda.synchronize()
        assert np.array_equal(U.bits(got["hits"]), U.bits(hits.cpu().numpy())), "hits are not trace_rays' records"
        leaf = got["kinds"] == 0
        assert np.array_equal(U.bits(got["local"][leaf]), U.bits(col.cpu().numpy()[leaf])), "local is not trace_rays' colour where kinds == 0"
        # what does not exist is +0
        assert not got["reflect"][(got["kinds"] & 1) == 0].view(np.uint32).any() and not got["refract"][(got["kinds"] & 2) == 0].view(np.uint32).any()
        assert not got["weight"][leaf].view(np.uint32).any() and not got["weight"][(got["kinds"] & 2) == 0, 1].view(np.uint32).any()
        counts = SC.class_counts(rays, got, got["hits"], exp["normal"], exp["material"])
        print("%s %dx%d cull %d (%s): %d rays, %s" % (name, w, h, cull, what, len(rays), counts))
        for c, k in counts.items():
            total[c] = total.get(c, 0) + k
    for c in SC.claims(name, cull):
        assert total[c] >= SC.MIN_CLASS, "%s cull %d: %d rays of class %s" % (name, cull, total[c], c)
    g.close()


# ---- 2. one level of castRay ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", ["file", 1, 0])
@pytest.mark.parametrize("name", SC.SCENES)
def test_one_level_composes_trace_rays_colours(ra, family, tmp_path, name, level):
    w, h = SC.size_of(name)
    g0 = ra.Scene(path_of(name, family), w, h)
    M = g0.max_ray_depth if level == "file" else level
    g0.close()
    g = ra.Scene(at_depth(name, family, tmp_path, M), w, h)
    shallow = ra.Scene(at_depth(name, family, tmp_path, M - 1), w, h)
    assert (g.max_ray_depth, shallow.max_ray_depth) == (M, M - 1)
    rays = pool_of(g, name)
    got = scatter(g, rays)
    kid_rays, parent, is_refract = SC.children(got)
    assert len(kid_rays) >= SC.MIN_CLASS
    kids = colours(shallow, kid_rays)
    if M == 0:                # the children are beyond the depth
        assert np.array_equal(U.bits(kids), U.bits(sky(g, kid_rays))) and np.array_equal(U.bits(kids), U.bits(sky(shallow, kid_rays)))
    c_reflect, c_refract = SC.spread(kids, parent, is_refract, len(rays))
    want = colours(g, rays)
    mine = SC.compose(got["kinds"], got["weight"], got["local"], c_reflect, c_refract)
    bad = (U.bits(mine) != U.bits(want)).any(-1)
    print("%s, max_ray_depth %d: %d rays, %d children, %d differ" % (name, M, len(rays), len(kid_rays), bad.sum()))
    assert not bad.any(), "%s, max_ray_depth %d: %d of %d rays whose composed colour is not trace_rays' (kinds %s)" % (
        name, M, bad.sum(), len(rays), np.unique(got["kinds"][bad]))
    g.close(); shallow.close()


# ---- 3. cast_tree ---------------------------------------------------------------------------------------------------------------------------
def check_levels(levels, n, depth):
    assert 1 <= len(levels) <= depth + 2
    assert levels[0]["parent"] is None and levels[0]["rays"].shape == (n, 6)
    for k, lv in enumerate(levels):
        m = lv["rays"].shape[0]
        assert lv["kind"].dtype == torch.uint8 and lv["kind"].shape == (m,) and lv["weight"].shape == (m, 2)
        assert lv["local"].shape == (m, 3) and lv["colour"].shape == (m, 3)
        if k:
            above = levels[k - 1]
            p = lv["parent"].cpu().numpy()
            assert p.shape == (m,) and (np.diff(p) >= 0).all() and p.min() >= 0 and p.max() < above["rays"].shape[0]
            # every parent has as many children as its kind says, the refraction ray first
            kind = above["kind"].cpu().numpy()
            assert np.array_equal(np.bincount(p, minlength=len(kind)), (kind & 1) + ((kind >> 1) & 1))
        if k > depth:
            assert not lv["kind"].any()


@pytest.mark.parametrize("name", SC.SCENES)
def test_cast_tree_equals_trace_rays(ra, family, tmp_path, name):
    w, h = SC.size_of(name)
    g = ra.Scene(path_of(name, family), w, h)
    rays = pool_of(g, name)
    t = dev(rays)
    want = colours(g, rays)
    col, levels = g.cast_tree(t)
    torch.cuda.synchronize()
    bad = (U.bits(col.cpu().numpy()) != U.bits(want)).any(-1)
    print("%s: %d rays, max_ray_depth %d, levels of %s rays, %d differ" % (name, len(rays), g.max_ray_depth, [lv["rays"].shape[0] for lv in levels], bad.sum()))
    assert not bad.any(), "%s: %d of %d colours of cast_tree are not trace_rays'" % (name, bad.sum(), len(rays))
    check_levels(levels, len(rays), g.max_ray_depth)
    assert len(levels) >= 3
    # beyond the depth everything is sky; a depth of the caller's is the scene's with that max_ray_depth
    col, levels = g.cast_tree(t, depth=-1)
    assert len(levels) == 1 and np.array_equal(U.bits(col.cpu().numpy()), U.bits(sky(g, rays)))
    col, levels = g.cast_tree(t, depth=1)
    check_levels(levels, len(rays), 1)
    f = ra.Scene(at_depth(name, family, tmp_path, 1), w, h)
    assert np.array_equal(U.bits(col.cpu().numpy()), U.bits(colours(f, rays))), "depth=1 is not the scene at max_ray_depth 1"
    f.close()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        t2 = t.clone()
    st.synchronize()
    col, _ = g.cast_tree(t2, stream=st)
    st.synchronize()
    assert np.array_equal(U.bits(col.cpu().numpy()), U.bits(want))
    with pytest.raises(ValueError, match="cast_tree: stream must be"):
        g.cast_tree(t, stream=st.cuda_stream)
    g.close()


# ---- 4. sky ---------------------------------------------------------------------------------------------------------------------------------
def test_sky(ra, family):
    from oracle import oracle as O
    name = "analytic"                          # (the skybox of the family: non-square faces)
    path = path_of(name, family)
    w, h = SC.size_of(name)
    g = ra.Scene(path, w, h)
    # on rays that miss: surface_rays' albedo
    rays = np.concatenate([U.primary_rays(g), S.sky_rays()])
    s = g.surface_rays(dev(rays), hits=True, normal=False, albedo=True)
    torch.cuda.synchronize()
    miss = s["hits"].cpu().numpy()[:, 0] == 0
    assert miss.sum() >= 300 and (~miss).sum() >= 300
    got = sky(g, rays)
    assert np.array_equal(U.bits(got[miss]), U.bits(s["albedo"].cpu().numpy()[miss]))
    # on rays that hit: the special directions of the lookup, each through the centre of the mirror sphere
    d = S.sky_directions()
    centre = np.array([-0.9, 0.3, -3.5], f32)
    aimed = np.concatenate([centre[None, :] - d * (f32(3) / np.sqrt((d.astype(np.float64) ** 2).sum(1)))[:, None].astype(f32), d], 1).astype(f32)
    hits, _ = g.trace_rays(dev(aimed), colours=False)
    torch.cuda.synchronize()
    assert (hits.cpu().numpy()[:, 0] > 0).all()
    o = O.OracleScene(path, w, h)
    want = o.skybox(d)
    everywhere = o.skybox(rays[:, 3:6])
    o.close()
    assert len(np.unique(want, axis=0)) >= 6           # (at least a texel of every face)
    assert np.array_equal(U.bits(sky(g, aimed)), U.bits(want))
    assert np.array_equal(U.bits(got), U.bits(everywhere))
    # without the skybox: the background colour, whatever the direction
    g.set_flag("useSkybox", 0)
    bg = np.tile(np.array([[0.2, 0.3, 0.4]], f32), (len(aimed), 1))
    assert np.array_equal(U.bits(sky(g, aimed)), U.bits(bg))
    assert tuple(g.sky(dev(aimed[:0])).shape) == (0, 3)
    g.close()


# ---- 5. batches and order -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reorder", [0, 1])
@pytest.mark.parametrize("name", ["cfg3_reflective_refractive", "mixed_materials", "area_light"])
def test_rays_are_independent_of_their_batch(ra, name, reorder):
    w, h = SC.size_of(name)
    g = ra.Scene("scenes/%s.scene" % name, w, h)
    pool = np.concatenate([pool_of(g, name), SU.probe_rays()[:1000]])
    want = scatter(g, pool)                    # (the default: no grouping at these sizes)
    assert len(np.unique(want["kinds"])) == 3
    g.set_knob("trace_reorder", reorder)       # (1: the sort runs on every batch, however small)
    rng = np.random.default_rng(23)
    perm = rng.permutation(len(pool))
    got = scatter(g, pool[perm])
    assert not SC.same(got, {c: want[c][perm] for c in CH}, CH), "a shuffled batch, reorder %d" % reorder
    # growing, then shrinking batches (the scene's ray scratch grows and stays)
    for n in (1, 63, 64, 65, 700, len(pool), 1500, 65, 64, 63, 1):
        first = int(rng.integers(0, len(pool) - n + 1))
        sl = slice(first, first + n)
        bad = SC.same(scatter(g, pool[sl]), {c: want[c][sl] for c in CH}, CH)
        assert not bad, "n = %d, reorder %d: %s" % (n, reorder, bad)
    out = g.scatter_rays(dev(pool[:0]), hits=True)
    assert [tuple(out[c].shape) for c in CH] == [(0,) + SC.TAIL[c] for c in CH] and out["kinds"].dtype == torch.uint8
    g.close()


# ---- 6. only what is asked for is written (the C entry, directly) --------------------------------------------------------------------------
class Buffers:
    """The six channels of n rays, each in the middle of a larger pre-filled allocation (kinds: bytes)."""

    def __init__(self, n):
        self.n = n
        self.flat, self.ptr = {}, {}
        for c in CH:
            size = n * int(np.prod(SC.TAIL[c], dtype=np.int64))
            if c == "kinds":
                self.flat[c] = torch.full((size + 2 * GUARD,), FILL_BYTE, dtype=torch.uint8, device="cuda")
                self.ptr[c] = self.flat[c].data_ptr() + GUARD
            else:
                self.flat[c] = torch.full((size + 2 * GUARD,), FILL, dtype=torch.float32, device="cuda")
                self.ptr[c] = self.flat[c].data_ptr() + 4 * GUARD

    def struct(self, ra, names):
        return ra.ScatterBuffers(*[self.ptr[c] if c in names else None for c in CH])

    def read(self):
        """channel -> numpy array (n, ...), after checking the guards"""
        torch.cuda.synchronize()
        out = {}
        for c in CH:
            f = self.flat[c].cpu().numpy()
            fill = FILL_BYTE if c == "kinds" else f32(FILL)
            assert (f[:GUARD] == fill).all() and (f[-GUARD:] == fill).all(), "%s: written outside the buffer" % c
            out[c] = f[GUARD:len(f) - GUARD].reshape((self.n,) + SC.TAIL[c])
        return out


def untouched(c, a):
    return (a == FILL_BYTE).all() if c == "kinds" else (np.ascontiguousarray(a).view(np.uint32) == np.array(FILL, f32).view(np.uint32)).all()


def call(ra, g, t, bufs, names):
    rtx, _ = ra.load()
    s = bufs.struct(ra, names)
    return rtx.rtx_scatter_rays(g.gpu(), t.shape[0], C.c_void_p(t.data_ptr()), C.byref(s), C.c_void_p(torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize("name", ["area_light", "mixed"])
def test_only_what_was_asked_for_is_written(ra, family, name):
    w, h = SC.size_of(name)
    g = ra.Scene(path_of(name, family), w, h)
    rays = pool_of(g, name)[:-1]
    t = dev(rays)
    n = len(rays)
    b = Buffers(n)
    assert call(ra, g, t, b, CH) == 0
    full = b.read()
    assert not SC.same(full, scatter(g, rays), CH)
    assert len(np.unique(full["kinds"])) == 3
    for names in [(c,) for c in CH] + [("reflect", "refract", "weight", "kinds"), ("hits", "local"), ("local", "kinds"), ("refract", "weight")]:
        b = Buffers(n)
        assert call(ra, g, t, b, names) == 0
        got = b.read()
        for c in CH:
            if c in names:
                assert np.array_equal(U.bits(got[c]), U.bits(full[c])), "%s of a call for %s differs from the six-channel call" % (c, names)
            else:
                assert untouched(c, got[c]), "%s was written by a call for %s" % (c, names)
    # hits alone is trace_rays' hits; the dict holds exactly what is asked for; local=False gives the same children
    traced, _ = g.trace_rays(t, colours=False)
    only = g.scatter_rays(t, local=False, reflect=False, refract=False, weight=False, kinds=False, hits=True)
    assert set(only) == {"hits"} and torch.equal(only["hits"], traced)
    assert set(g.scatter_rays(t)) == set(SC.SCATTER)
    kids = g.scatter_rays(t, local=False)
    torch.cuda.synchronize()
    assert set(kids) == set(SC.SCATTER) - {"local"}
    assert not SC.same({c: v.cpu().numpy() for c, v in kids.items()}, full, tuple(kids))
    g.close()


# ---- 7. scene state -------------------------------------------------------------------------------------------------------------------------
def test_flags_and_depth_change_nothing(ra, family, tmp_path):
    name = "mixed"
    w, h = SC.size_of(name)
    g = ra.Scene(path_of(name, family), w, h)
    rays = np.concatenate([pool_of(g, name), SU.probe_rays()[:1024]])
    want = scatter(g, rays)
    assert len(np.unique(want["kinds"])) == 3 and (want["hits"][:, 0] == 0).sum() >= 100
    g.set_flag("showNormals", 1)
    assert not SC.same(scatter(g, rays), want, CH), "showNormals changes a channel"
    g.set_flag("showNormals", 0)
    for depth in (-1, 0, 7):
        f = ra.Scene(at_depth(name, family, tmp_path, depth), w, h)
        assert f.max_ray_depth == depth
        assert not SC.same(scatter(f, rays), want, CH), "max_ray_depth = %d" % depth
        f.close()
    # the skybox flag: only the sky colour follows it, as surface_rays' albedo at a miss does
    g.set_flag("useSkybox", 0)
    got = scatter(g, rays)
    assert not SC.same(got, want, tuple(c for c in CH if c != "local"))
    miss = want["hits"][:, 0] == 0
    assert np.array_equal(U.bits(got["local"][~miss]), U.bits(want["local"][~miss]))
    assert np.array_equal(U.bits(got["local"][miss]), U.bits(np.tile(np.array([[0.2, 0.3, 0.4]], f32), (miss.sum(), 1))))
    assert (U.bits(want["local"][miss]) != U.bits(got["local"][miss])).any()
    g.close()


def check_against_fresh(ra, g, path, what, name="mixed_materials"):
    """g's results equal those of a scene loaded from `path`, and the expectation there"""
    f = ra.Scene(path, g.width, g.height)
    rays = np.concatenate([pool_of(f, name), SU.probe_rays()[:1024]])
    got, want = scatter(g, rays), scatter(f, rays)
    bad = SC.same(got, want, CH)
    assert not bad, "%s: differs from a fresh scene in %s" % (what, bad)
    assert not SC.same(got, expectation(f, rays), CH), "%s: differs from the expectation" % what
    f.close()
    return got


def test_edited_scenes_equal_a_fresh_scene(ra, tmp_path):
    from tests.util_move import edit_scene, write_scene
    name = "mixed_materials"
    w, h = SC.size_of(name)
    text = text_of("scenes/%s.scene" % name)
    g = ra.Scene("scenes/%s.scene" % name, w, h)
    scatter(g, SU.probe_rays()[:1024])
    # lights: set, add, remove
    for k, step in enumerate([("set", 0, dict(position=(-1.5, 2.5, -1.0), intensity=0.9)),
                              ("add", "point", dict(position=(0.5, 3.0, -6.0), color=(0.3, 0.9, 0.5), intensity=1.1)), ("remove", 1)]):
        text = LE.apply_step(g, text, step)
        check_against_fresh(ra, g, LE.write_scene(tmp_path, text, "sc_light%d" % k), "light step %d %s" % (k, step[0]))
    # objects: the Phong sphere, then the glass mesh
    for k, (index, keys) in enumerate([(3, dict(pos=(0.4, 1.2, -5.5), radius=0.85)), (1, dict(rot=(-40, 10, 70), pos=(-0.9, 0.2, -4.4)))]):
        g.move_object(index, **keys)
        text = edit_scene(text, index, **keys)
        check_against_fresh(ra, g, write_scene(tmp_path, text, "sc_move%d" % k), "move %d" % k)
    # vertices: the mirror torus
    P, _ = g.mesh_vertices(2)
    V = DF.bulge(P)
    g.set_vertices(2, torch.from_numpy(V).cuda())
    f, path = DF.deformed_scene(ra, tmp_path, text, 2, V, None, "sc_bulge", w, h)
    f.close()
    check_against_fresh(ra, g, path, "set_vertices")
    g.close()


def test_a_scene_without_lights(ra, tmp_path):
    name = "cfg1_simple_shapes"
    text = text_of("scenes/%s.scene" % name)
    for k in range(LE.n_lights(text) - 1, -1, -1):
        text = LE.remove_light(text, k)
    path = LE.write_scene(tmp_path, text, "sc_dark")
    w, h = SC.size_of(name)
    g = ra.Scene(path, w, h)
    assert g.n_lights == 0
    rays = pool_of(g, name)
    got = scatter(g, rays)
    exp = expectation(g, rays)
    assert not SC.same(got, exp, CH)
    mirror, glass = exp["material"] == SC.REFLECTIVE, exp["material"] == SC.TRANSPARENT
    assert mirror.sum() >= SC.MIN_CLASS and glass.sum() >= SC.MIN_CLASS
    assert not got["local"][mirror].view(np.uint32).any() and not got["local"][glass].view(np.uint32).any()
    # ... and the lights of the live scene removed one by one end in the same state
    live = ra.Scene("scenes/%s.scene" % name, w, h)
    lit = scatter(live, rays)
    assert lit["local"][mirror].any()
    while live.n_lights:
        live.remove_light(0)
    assert not SC.same(scatter(live, rays), got, CH)
    live.close()
    g.close()


@pytest.mark.parametrize("as_current", [False, True])
def test_rays_written_on_another_stream(ra, as_current):
    name = "mixed_materials"
    w, h = SC.size_of(name)
    g = ra.Scene("scenes/%s.scene" % name, w, h)
    rays = np.concatenate([pool_of(g, name), SU.probe_rays()] * 3)
    want = scatter(g, rays)
    src = dev(rays)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    for _ in range(2):
        with torch.cuda.stream(st):
            t = torch.full_like(src, float("nan"))       # (written on st: a call that did not wait for the copy would trace NaNs)
            t.copy_(src)
            out = g.scatter_rays(t, hits=True) if as_current else g.scatter_rays(t, hits=True, stream=st)
            c = g.sky(t) if as_current else g.sky(t, stream=st)
        st.synchronize()
        assert not SC.same({k: v.cpu().numpy() for k, v in out.items()}, want, CH), "stream, as current %s" % as_current
        assert np.array_equal(U.bits(c.cpu().numpy()), U.bits(sky(g, rays)))
    g.close()


def test_counters_are_neither_collected_nor_refused(ra):
    name = "mixed_materials"
    w, h = SC.size_of(name)
    g = ra.Scene("scenes/%s.scene" % name, w, h)
    rays = SU.probe_rays()
    want = scatter(g, rays)
    sk = sky(g, rays)
    g.counters_enable(True)
    g.counters_reset()
    assert not SC.same(scatter(g, rays), want, CH), "counters enabled"
    assert np.array_equal(U.bits(sky(g, rays)), U.bits(sk))
    c = g.counters()
    assert not c.any(), c
    g.counters_enable(False)
    g.close()


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_buffers_untouched(ra):
    g = ra.Scene("scenes/cfg1_simple_shapes.scene", 40, 24)
    rtx, _ = ra.load()
    rays = SU.probe_rays()[:1000]
    t = dev(rays)
    with pytest.raises(ValueError, match="scatter_rays: nothing to compute"):
        g.scatter_rays(t, local=False, reflect=False, refract=False, weight=False, kinds=False)
    b = Buffers(len(rays))
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    # the all-NULL struct, a NULL struct, NULL rays, too many rays
    assert call(ra, g, t, b, ()) == -1
    assert b"NULL" in rtx.rtx_last_error()
    assert rtx.rtx_scatter_rays(g.gpu(), len(rays), C.c_void_p(t.data_ptr()), None, st) == -1
    s = b.struct(ra, CH)
    assert rtx.rtx_scatter_rays(g.gpu(), len(rays), None, C.byref(s), st) == -1
    assert rtx.rtx_scatter_rays(g.gpu(), 0xFFFFFFC1, C.c_void_p(t.data_ptr()), C.byref(s), st) == -1
    assert rtx.rtx_scatter_rays(g.gpu(), 0, None, C.byref(s), st) == 0          # n == 0: nothing to do
    # rtx_sky_rays: NULL rays, NULL colours, too many rays
    out = C.c_void_p(b.ptr["local"])
    assert rtx.rtx_sky_rays(g.gpu(), len(rays), None, out, st) == -1
    assert rtx.rtx_sky_rays(g.gpu(), len(rays), C.c_void_p(t.data_ptr()), None, st) == -1
    assert rtx.rtx_sky_rays(g.gpu(), 0xFFFFFFC1, C.c_void_p(t.data_ptr()), out, st) == -1
    assert rtx.rtx_sky_rays(g.gpu(), 0, None, None, st) == 0
    got = b.read()
    assert all(untouched(c, got[c]) for c in CH)
    # ... and the calls work afterwards
    assert call(ra, g, t, b, CH) == 0
    assert not SC.same(b.read(), scatter(g, rays), CH)
    assert rtx.rtx_sky_rays(g.gpu(), len(rays), C.c_void_p(t.data_ptr()), out, st) == 0
    assert np.array_equal(U.bits(b.read()["local"]), U.bits(sky(g, rays)))
    g.close()
