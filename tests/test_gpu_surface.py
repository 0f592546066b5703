"""rtx_surface_rays / Scene.surface_rays (include/rtx_surface.h): hit record, hit point, shading normal, albedo and specular coefficient of
caller-supplied rays.  Every comparison is bit for bit over every ray: against the oracle-derived expectation of tests/util_surface.py,
against render_aov of the same and of another view (the exact bits of N for rays that do not start at the camera), against the library's
own other routes (trace_rays with and without showNormals), across batches, orders and sizes; only what is asked for is written; the
surroundings (frames, edits, streams, ownership, counters, refusals); and one composed use: surface_rays -> rays built in torch ->
occluded, which must count what render_ao counts.

Ray sets: (A) the view's camera rays, (B) bounce rays from their hits, (C) another camera's rays, (D) seeded probe rays."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import util_ao as AO
from tests import util_aov as U
from tests import util_shading as S
from tests import util_surface as SU
from tests.util_move import edit_scene
from tests.util_objects import apply_step, write_scene

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = U.ROOT
f32 = np.float32
GUARD = 96                    # untouched elements before and after every buffer
FILL = 7.25
CH = SU.CHANNELS
ALL = dict(hits=True, position=True, normal=True, albedo=True, specular=True)
AOV_TAIL = {"depth": ((), torch.float32), "object_id": ((), torch.int32), "triangle_id": ((), torch.int32), "uv": ((2,), torch.float32),
            "normal": ((3,), torch.float32), "albedo": ((3,), torch.float32)}


@pytest.fixture(scope="module")
def family(tmp_path_factory):
    d = S.short_dir(tmp_path_factory)
    return d, S.write_family(d)


def path_of(name, family):
    return family[1][name] if name in S.FAMILY else "scenes/%s.scene" % name


def dev(rays):
    return torch.from_numpy(np.ascontiguousarray(rays, f32)).cuda()


def surface(g, rays, channels=CH, stream=None):
    """channel -> numpy array of Scene.surface_rays for a numpy ray array"""
    out = g.surface_rays(dev(rays), stream=stream, **{c: c in channels for c in CH})
    torch.cuda.synchronize()
    assert set(out) == set(channels)
    return {c: t.cpu().numpy() for c, t in out.items()}


def aov(g):
    """the six channels of render_aov of g's current view, flat over the pixels row-major (unwritten pixels: zeros)"""
    w, h = g.width, g.height
    b = {c: torch.zeros((h, w) + tail, dtype=dt, device="cuda") for c, (tail, dt) in AOV_TAIL.items()}
    g.render_aov(**b)
    torch.cuda.synchronize()
    return {c: t.cpu().numpy().reshape((w * h,) + AOV_TAIL[c][0]) for c, t in b.items()}


def differs_from_aov(got, frame, mask):
    """names of render_aov's channels that a surface_rays result of the view's primary rays does not equal on the written pixels"""
    m = mask.reshape(-1)
    hits = got["hits"]
    mine = dict(depth=hits[:, 3], object_id=hits[:, 1].astype(np.int32), triangle_id=hits[:, 2].astype(np.int32), uv=hits[:, 4:6],
                normal=got["normal"], albedo=got["albedo"])
    return [c for c in AOV_TAIL if not np.array_equal(U.bits(np.ascontiguousarray(mine[c][m])), U.bits(np.ascontiguousarray(frame[c][m])))]


def first_hit_rays(g):
    """(A) and (B) of Scene g"""
    cam, depth, normal, hit = AO.first_hits(g)
    return cam, SU.bounce_rays(cam, depth, normal, hit)


def other_view(g):
    """(C): the primary rays and render_aov's frame of another pose; the camera is moved back."""
    pos, rot = g.camera_pose()
    g.set_camera(pos + SU.OTHER_POSE[0], rot + SU.OTHER_POSE[1])
    rays, frame = U.primary_rays(g), aov(g)
    g.set_camera(pos, rot)
    return rays, frame


# ---- 1. all five channels against the oracle-derived expectation ------------------------------------------------------------------------
@pytest.mark.parametrize("cull", [1, 0])
@pytest.mark.parametrize("name", SU.SCENES)
def test_channels_equal_the_expectation(ra, family, name, cull):
    w, h = SU.size_of(name)
    path = path_of(name, family)
    g = ra.Scene(path, w, h)
    g.set_flag("useBackfaceCulling", cull)
    cam, bounce = first_hit_rays(g)
    assert len(bounce) > 1000
    for what, rays in (("A", cam), ("B", bounce), ("D", SU.probe_rays())):
        got = surface(g, rays)
        exp = SU.expected_of(path, w, h, cull, rays)
        bad = SU.mismatches(got, exp)
        assert not bad, "%s %dx%d cull %d (%s): rays that differ from the expectation, per channel: %s" % (name, w, h, cull, what, bad)
        if what == "A":
            bad = differs_from_aov(got, aov(g), U.written_mask(w, h))
            assert not bad, "%s %dx%d cull %d: camera rays differ from render_aov in %s" % (name, w, h, cull, bad)
    g.close()


# ---- 2. another camera's rays under this view: the exact N, the general source class against the camera's copies --------------------------
@pytest.mark.parametrize("cull", [1, 0])
@pytest.mark.parametrize("name", ["cfg1_simple_shapes", "cfg2_smooth_4k", "plain_nrm", "coincident"])
def test_another_cameras_rays_equal_its_render_aov(ra, family, name, cull):
    w, h = SU.size_of(name)
    path = path_of(name, family)
    g = ra.Scene(path, w, h)
    g.set_flag("useBackfaceCulling", cull)
    here = aov(g)
    rays, there = other_view(g)
    assert not np.array_equal(rays, U.primary_rays(g))
    got = surface(g, rays)
    mask = U.written_mask(w, h)
    m = mask.reshape(-1)
    hit = got["hits"][:, 0] > 0
    assert hit.mean() >= 0.2, "too few of the other camera's rays hit"
    assert (hit[m] != (here["object_id"][m] >= 0)).any(), "the other view's hit mask is this view's"
    bad = differs_from_aov(got, there, mask)
    assert not bad, "%s cull %d: differs from the other view's render_aov in %s" % (name, cull, bad)
    assert not SU.mismatches(got, SU.expected_of(path, w, h, cull, rays))
    # ... and the view is the original one again
    assert not differs_from_aov(surface(g, U.primary_rays(g)), here, mask)
    g.close()


# ---- 3. the library's other routes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cfg4_textured_256", "mixed_materials", "plain_nrm", "cfg3_reflective_refractive"])
def test_library_routes_agree(ra, family, name):
    w, h = SU.size_of(name)
    g = ra.Scene(path_of(name, family), w, h)
    cam, bounce = first_hit_rays(g)
    rays = np.concatenate([cam, bounce, SU.probe_rays()])
    t = dev(rays)
    five = surface(g, rays)
    traced, _ = g.trace_rays(t, hits=True, colours=False)
    torch.cuda.synchronize()
    assert np.array_equal(U.bits(five["hits"]), U.bits(traced.cpu().numpy()))
    assert not SU.same(surface(g, rays, ("hits",)), five, ("hits",))
    g.set_flag("showNormals", 1)
    assert not SU.same(surface(g, rays), five), "showNormals changes a channel"
    hn, cn = g.trace_rays(t)
    torch.cuda.synchronize()
    g.set_flag("showNormals", 0)
    hn, cn = hn.cpu().numpy(), cn.cpu().numpy()
    assert np.array_equal(U.bits(hn), U.bits(five["hits"]))
    hit = five["hits"][:, 0] > 0
    assert hit.any() and not hit.all() or name == "mixed_materials"
    want = np.where(hit[:, None], five["normal"] / f32(2) + f32(0.5), five["albedo"]).astype(f32)
    assert np.array_equal(U.bits(cn), U.bits(want)), "trace_rays' showNormals colours are not normal / 2 + 0.5 | albedo"
    g.close()


# ---- 4. every ray is independent of its batch ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reorder", [0, 1])
@pytest.mark.parametrize("name", ["cfg2_smooth_4k", "plain_nrm", "cfg1_simple_shapes"])
def test_rays_are_independent_of_their_batch(ra, family, name, reorder):
    w, h = SU.size_of(name)
    g = ra.Scene(path_of(name, family), w, h)
    cam, bounce = first_hit_rays(g)
    sets = [cam, bounce, other_view(g)[0]]
    separate = [surface(g, r) for r in sets]              # (the default: no grouping at these sizes)
    rays = np.concatenate(sets)
    want = {c: np.concatenate([s[c] for s in separate]) for c in CH}
    n = len(rays) - (1 if len(rays) % 64 == 0 else 0)
    perm = np.random.default_rng(2024).permutation(len(rays))[:n]
    assert n % 64 != 0 and n > 64
    g.set_knob("trace_reorder", reorder)
    got = surface(g, rays[perm])
    bad = SU.same(got, {c: want[c][perm] for c in CH})
    assert not bad, "%s reorder %d: rays of a permuted batch differ from their separate calls in %s" % (name, reorder, bad)
    g.close()


@pytest.mark.parametrize("reorder", [-1, 1])
def test_small_and_changing_batch_sizes(ra, reorder):
    name = "cfg4_textured_256"
    w, h = SU.size_of(name)
    g = ra.Scene("scenes/%s.scene" % name, w, h)
    cam, bounce = first_hit_rays(g)
    pool = np.concatenate([cam, bounce, SU.probe_rays()])
    pool = pool[np.random.default_rng(7).permutation(len(pool))]
    want = surface(g, pool)
    g.set_knob("trace_reorder", reorder)                  # (1: the sort's scratch grows and is reused)
    rng = np.random.default_rng(9)
    for n in (1, 63, 64, 65, 700, 129, len(pool), 3000, 2, 4097):
        first = int(rng.integers(0, len(pool) - n + 1))
        sl = slice(first, first + n)
        got = surface(g, pool[sl])
        bad = SU.same(got, {c: want[c][sl] for c in CH})
        assert not bad, "n = %d, reorder %d: %s" % (n, reorder, bad)
    out = g.surface_rays(dev(pool[:0]), **ALL)
    assert [tuple(out[c].shape) for c in CH] == [(0, 8), (0, 3), (0, 3), (0, 3), (0,)]
    g.close()


# ---- 5. only what is asked for is written (the C entry, directly) ------------------------------------------------------------------------
class Buffers:
    """The five channels of n rays, each in the middle of a larger pre-filled allocation."""

    def __init__(self, n):
        self.n = n
        self.flat, self.ptr = {}, {}
        for c in CH:
            size = n * int(np.prod(SU.TAIL[c], dtype=np.int64))
            self.flat[c] = torch.full((size + 2 * GUARD,), FILL, dtype=torch.float32, device="cuda")
            self.ptr[c] = self.flat[c].data_ptr() + 4 * GUARD

    def struct(self, ra, names):
        return ra.SurfaceBuffers(*[self.ptr[c] if c in names else None for c in CH])

    def read(self):
        """channel -> numpy array (n, ...), after checking the guards"""
        torch.cuda.synchronize()
        out = {}
        for c in CH:
            f = self.flat[c].cpu().numpy()
            assert (f[:GUARD] == f32(FILL)).all() and (f[-GUARD:] == f32(FILL)).all(), "%s: written outside the buffer" % c
            out[c] = f[GUARD:-GUARD].reshape((self.n,) + SU.TAIL[c])
        return out


def call(ra, g, t, bufs, names):
    rtx, _ = ra.load()
    s = bufs.struct(ra, names)
    return rtx.rtx_surface_rays(g.gpu(), t.shape[0], C.c_void_p(t.data_ptr()), C.byref(s), C.c_void_p(torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize("name", ["cfg4_textured_256", "cfg1_simple_shapes"])
def test_only_what_was_asked_for_is_written(ra, name):
    w, h = SU.size_of(name)
    g = ra.Scene("scenes/%s.scene" % name, w, h)
    cam, bounce = first_hit_rays(g)
    rays = np.concatenate([cam, bounce])[:-1]
    t = dev(rays)
    n = len(rays)
    b = Buffers(n)
    assert call(ra, g, t, b, CH) == 0
    full = b.read()
    assert not SU.same(full, surface(g, rays))
    for c in CH:
        assert not (full[c].reshape(n, -1) == f32(FILL)).all(1).any(), "%s: a ray was not written" % c
    for names in [(c,) for c in CH] + [("hits", "normal"), ("normal", "albedo")]:
        b = Buffers(n)
        assert call(ra, g, t, b, names) == 0
        got = b.read()
        for c in CH:
            if c in names:
                assert np.array_equal(U.bits(got[c]), U.bits(full[c])), "%s of a call for %s differs from the five-channel call" % (c, names)
            else:
                assert (got[c] == f32(FILL)).all(), "%s was written by a call for %s" % (c, names)
    g.close()


# ---- 6. surroundings ------------------------------------------------------------------------------------------------------------------------
def test_ordinary_frames_are_undisturbed(ra):
    w, h = 96, 72
    g = ra.Scene("scenes/cfg2_smooth_4k.scene", w, h)

    def frame():
        fb = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
        mask = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
        g.render_frame(fb, mask)
        torch.cuda.synchronize()
        assert g.frame_status() == 0
        return fb.cpu().numpy(), mask.cpu().numpy()

    for _ in range(3):                # (the frame mode settles on its measurements)
        before = frame()
    mode = g.frame_mode()
    costs = g.tile_cost()
    rays = SU.probe_rays()
    got = surface(g, rays)
    assert g.frame_mode() == mode and np.array_equal(costs, g.tile_cost())
    after = frame()
    assert np.array_equal(U.bits(before[0]), U.bits(after[0])) and np.array_equal(before[1], after[1])
    assert not SU.mismatches(got, SU.expected_of("scenes/cfg2_smooth_4k.scene", w, h, None, rays))
    g.close()


def test_edited_scene_equals_a_fresh_one(ra, tmp_path):
    name = "mixed_materials"
    w, h = 40, 24
    text = open(os.path.join(ROOT, "scenes", name + ".scene")).read()
    g = ra.Scene("scenes/%s.scene" % name, w, h)
    surface(g, SU.probe_rays())
    steps = [("move", 3, dict(pos=(0.4, 1.2, -5.5), radius=0.85)),                      # a sphere
             ("move", 1, dict(rot=(-40, 10, 70), pos=(-0.9, 0.2, -4.4))),               # a mesh
             ("add", "sphere", None, dict(pos=(-0.6, -0.3, -2.5), color=(0.2, 0.9, 0.4), radius=0.4)),
             ("remove", 0),
             ("light",),
             ("resize", 33, 17)]
    for k, step in enumerate(steps):
        if step[0] == "move":
            g.move_object(step[1], **step[2])
            text = edit_scene(text, step[1], **step[2])
        elif step[0] == "resize":
            w, h = step[1], step[2]
            g.resize(w, h)
        elif step[0] == "light":
            # (no channel depends on a light: the edit must change nothing, and must not leave the scene in another state)
            g.set_light(0, intensity=0.37)
        else:
            text = apply_step(g, text, step)
        p = write_scene(tmp_path, text, "surface_%d" % k)
        f = ra.Scene(p, w, h)
        rays = np.concatenate([first_hit_rays(f)[1], U.primary_rays(f), SU.probe_rays()])
        got, want = surface(g, rays), surface(f, rays)
        bad = SU.same(got, want)
        assert not bad, "step %d %s: differs from a fresh scene in %s" % (k, step[0], bad)
        assert not SU.mismatches(got, SU.expected_of(p, w, h, None, rays)), "step %d %s: differs from the expectation" % (k, step[0])
        f.close()
    g.close()


@pytest.mark.parametrize("as_current", [False, True])
def test_rays_written_on_another_stream(ra, as_current):
    name = "cfg2_smooth_4k"
    w, h = SU.size_of(name)
    g = ra.Scene("scenes/%s.scene" % name, w, h)
    rays = np.concatenate([SU.probe_rays()] * 8)
    want = surface(g, rays)
    src = dev(rays)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    for _ in range(3):
        with torch.cuda.stream(st):
            t = torch.full_like(src, float("nan"))       # (written on st: a call that did not wait for the copy would trace NaNs)
            t.copy_(src)
            out = g.surface_rays(t, **ALL) if as_current else g.surface_rays(t, stream=st, **ALL)
        st.synchronize()
        assert not SU.same({c: v.cpu().numpy() for c, v in out.items()}, want), "stream, as current %s" % as_current
    g.close()


def test_row_ownership_is_ignored(ra):
    g = ra.Scene("scenes/mixed_materials.scene", 64, 64)
    rays = SU.probe_rays()
    want = surface(g, rays)
    for part in (0, 1):
        g.set_row_ownership(16, 2, part)
        assert not SU.same(surface(g, rays), want), "row ownership part %d of 2" % part
    g.set_row_ownership(0, 1, 0)
    g.close()


def test_counters_are_neither_collected_nor_refused(ra):
    g = ra.Scene("scenes/cfg2_smooth_4k.scene", 64, 64)
    rays = SU.probe_rays()
    want = surface(g, rays)
    g.counters_enable(True)
    g.counters_reset()
    assert not SU.same(surface(g, rays), want), "counters enabled"
    c = g.counters()
    assert not c.any(), c
    g.counters_enable(False)
    g.close()


def test_refusals_leave_the_buffers_untouched(ra):
    g = ra.Scene("scenes/cfg1_simple_shapes.scene", 40, 24)
    rtx, _ = ra.load()
    rays = SU.probe_rays()[:1000]
    t = dev(rays)
    with pytest.raises(ValueError, match="surface_rays: nothing to compute"):
        g.surface_rays(t, normal=False, albedo=False)
    b = Buffers(len(rays))
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    # the all-NULL struct, a NULL struct, NULL rays
    assert call(ra, g, t, b, ()) == -1
    assert b"NULL" in rtx.rtx_last_error()
    assert rtx.rtx_surface_rays(g.gpu(), len(rays), C.c_void_p(t.data_ptr()), None, st) == -1
    s = b.struct(ra, CH)
    assert rtx.rtx_surface_rays(g.gpu(), len(rays), None, C.byref(s), st) == -1
    assert rtx.rtx_surface_rays(g.gpu(), 0xFFFFFFC1, C.c_void_p(t.data_ptr()), C.byref(s), st) == -1
    assert rtx.rtx_surface_rays(g.gpu(), 0, None, C.byref(s), st) == 0          # n == 0: nothing to do
    for c, a in b.read().items():
        assert (a == f32(FILL)).all(), c
    # ... and the call works afterwards
    assert call(ra, g, t, b, CH) == 0
    assert not SU.mismatches(b.read(), SU.expected_of("scenes/cfg1_simple_shapes.scene", 40, 24, None, rays))
    g.close()


# ---- 7. composed: surface_rays -> rays built in torch -> occluded, which counts what render_ao counts ------------------------------------
@pytest.mark.parametrize("name", ["cfg4_textured_256", "mixed_materials"])
def test_composed_ambient_occlusion_equals_render_ao(ra, name):
    w, h = SU.size_of(name)
    g = ra.Scene("scenes/%s.scene" % name, w, h)
    counts = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    g.render_ao(dev(AO.DIRS19), float("inf"), counts=counts)
    torch.cuda.synchronize()
    # the contract of include/rtx_ao.h, steps 1 to 3, on the caller's side
    s = g.surface_rays(dev(U.primary_rays(g)), hits=True, position=True, normal=True, albedo=False)
    N, dirs = s["normal"], dev(AO.DIRS19)
    O = s["position"] + N * float(AO.BIAS)
    c = (N[:, 0:1] * dirs[None, :, 0] + N[:, 1:2] * dirs[None, :, 1]) + N[:, 2:3] * dirs[None, :, 2]
    written = torch.from_numpy(U.written_mask(w, h).reshape(-1)).cuda()
    traced = (s["hits"][:, 0:1] > 0) & written[:, None] & (c > 0)
    pix, k = torch.nonzero(traced, as_tuple=True)
    assert len(pix) > 1000
    rays = torch.cat([O[pix], dirs[k]], 1).contiguous()
    occluded = g.occluded(rays)
    nopen = torch.zeros(w * h, dtype=torch.int64, device="cuda").index_add_(0, pix, (occluded == 0).to(torch.int64))
    mine = (nopen | (traced.sum(1) << 16)).to(torch.int32).cpu().numpy().reshape(h, w)
    torch.cuda.synchronize()
    mask = U.written_mask(w, h)
    want = counts.cpu().numpy()
    assert (want[mask] >> 16).max() > 0 and len(np.unique(want[mask] & 0xFFFF)) > 3
    assert np.array_equal(mine[mask], want[mask]), "%d pixels count differently" % (mine[mask] != want[mask]).sum()
    g.close()
