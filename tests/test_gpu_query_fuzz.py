"""The ray, point and frame queries on the sixteen seeded random scenes of tests/util_query_fuzz.py, one test and one live Scene per seed:
occluded, trace_rays, surface_rays, light_rays, scatter_rays / sky / cast_tree, light_points, ao_points, radiance_points, render_aov,
render_ao, render_light, render_views and render_views_aov, in an order shuffled by the seed (surface_rays before the calls that take its
N), each compared bit for bit over every ray, point or pixel with the expectation composed from the CPU oracle.  The visibility of every
shadow and occlusion ray is the oracle's, never Scene.occluded's.  tests/test_query_fuzz_cpu.py shows that these inputs can tell right from
wrong.

Odd seeds force the grouping path (trace_reorder = 1), seeds divisible by three put every call on one non-default stream with inputs produced
on it.  In the middle of the sequence the scene is moved to another camera, culling value and size, renders a frame there (compared with the
oracle's), and is set back: every call made before is made again and returns the same bits.  Frame calls take seed-drawn rows and write
into buffers with guard elements; nothing outside the written pixels may change.

Measured on an MI355X, the whole test of a seed with its expectation (whose per-element oracle calls on the host dominate), seconds for
seeds 0 to 15: 1.5, 0.6, 0.9, 0.8, 1.0, 0.4, 1.2, 0.4, 0.3, 0.7, 0.5, 0.6, 0.5, 0.9, 1.0, 0.4 -- the module in 14 s; (B) therefore keeps the
4096 rays it may have.  Every seed passed when the module was written: no comparison failed, so at no seed was one of the faults of
tests/test_query_fuzz_cpu.py the only thing between a pass and a silent error."""
import time

import numpy as np
import pytest

from tests import util_aov as U
from tests import util_light as UL
from tests import util_points as UP
from tests import util_query_fuzz as Q
from tests import util_render_light as RL
from tests import util_scatter as SC
from tests import util_shading as S
from tests import util_surface as SU
from tests import util_views_aov as VA

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

f32 = np.float32
GUARD = RL.GUARD              # untouched elements before and after every buffer (128 for bytes: the buffer keeps its alignment)
FILL_F, FILL_I, FILL_B = VA.FILL_F, VA.FILL_I, 7
assert RL.FILL["diffuse"] == FILL_F and RL.FILL["light_open"] == FILL_I


@pytest.fixture(scope="module")
def qdir(tmp_path_factory):
    return S.short_dir(tmp_path_factory)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


class Buf:
    """A tensor of `shape` in the middle of a larger allocation filled with the sentinel (zero=True: the tensor itself zeroed)"""

    def __init__(self, run, shape, dtype, zero=False):
        self.fill = {torch.float32: FILL_F, torch.int32: FILL_I, torch.uint8: FILL_B}[dtype]
        self.guard = 128 if dtype == torch.uint8 else GUARD
        self.shape, n = tuple(shape), int(np.prod(shape))
        with run.on():
            self.flat = torch.full((n + 2 * self.guard,), self.fill, dtype=dtype, device="cuda")
            self.t = self.flat[self.guard:self.guard + n].view(self.shape)
            if zero:
                self.t.zero_()

    def read(self, what):
        f = self.flat.cpu().numpy()
        assert (f[:self.guard] == self.fill).all() and (f[len(f) - self.guard:] == self.fill).all(), "%s: written outside the buffer" % what
        return f[self.guard:len(f) - self.guard].reshape(self.shape).copy()


class Run:
    """One seed's scene and sequence: call(name) makes a call and returns its outputs as numpy arrays, check(name, got, where) compares
    them with the expectation."""

    def __init__(self, case, g, stream):
        self.case, self.g, self.stream = case, g, stream
        self.rays = self.dev(case.pool)
        self.N = self.position = None

    def on(self):
        return torch.cuda.stream(self.stream)

    def dev(self, a, dtype=f32):
        with self.on():
            return torch.from_numpy(np.array(a, dtype, order="C")).cuda()

    def sync(self):
        torch.cuda.synchronize()

    def host(self, out):
        self.sync()
        return {k: v.cpu().numpy() for k, v in out.items() if v is not None}

    def points(self):
        return self.case.points(self.position, self.N)

    # -- the calls
    def call(self, name):
        c, g, st = self.case, self.g, self.stream
        if name == "trace_rays":
            h, col = g.trace_rays(self.rays, stream=st)
            return self.host(dict(hits=h, colours=col))
        if name == "occluded":
            tmax = self.dev(c.occlusion()[0])
            return self.host(dict(mixed=g.occluded(self.rays, tmax, stream=st), whole=g.occluded(self.rays, None, stream=st)))
        if name == "surface_rays":
            return self.host(g.surface_rays(self.rays, hits=True, position=True, normal=True, albedo=True, specular=True, stream=st))
        if name == "light_rays":
            return self.host(g.light_rays(self.rays, hits=True, per_light=True, stream=st))
        if name == "scatter_rays":
            return self.host(g.scatter_rays(self.rays, hits=True, stream=st))
        if name == "sky":
            return self.host(dict(sky=g.sky(self.rays, stream=st)))
        if name == "cast_tree":
            return self.host(dict(colours=g.cast_tree(self.rays, stream=st)[0]))
        if name == "light_points":
            pts, view, _ = self.points()
            return self.host(g.light_points(self.dev(pts), self.dev(view), per_light=True, stream=st))
        if name == "ao_points":
            pts, _, _ = self.points()
            return self.host(g.ao_points(self.dev(pts), self.dev(c.dirs), c.radius, ao=True, counts=True, stream=st))
        if name == "radiance_points":
            pts, _, _ = self.points()
            tp, td, tw = self.dev(pts), self.dev(c.dirs), self.dev(c.weights)
            out = {}
            for cosine in (False, True):
                r = g.radiance_points(tp, td, tw, cosine=cosine, counts=True, stream=st)
                out.update({"sum%d" % cosine: r["sum"], "counts%d" % cosine: r["counts"]})
            return self.host(out)
        if name == "render_aov":
            bufs = {ch: Buf(self, (c.h, c.w) + VA.TAIL[ch], torch.int32 if VA.integer(ch) else torch.float32) for ch in U.CHANNELS}
            g.render_aov(rows=c.rows, stream=st, **{ch: b.t for ch, b in bufs.items()})
            return self.read(bufs, name)
        if name == "render_ao":
            bufs = dict(ao=Buf(self, (c.h, c.w), torch.float32), counts=Buf(self, (c.h, c.w), torch.int32))
            g.render_ao(self.dev(c.dirs), c.radius, ao=bufs["ao"].t, counts=bufs["counts"].t, rows=c.rows, stream=st)
            return self.read(bufs, name)
        if name == "render_light":
            L = len(c.lights[0])
            bufs = {ch: Buf(self, RL.shape_of(ch, L, c.w, c.h), torch.int32 if ch == "light_open" else torch.float32) for ch in RL.CHANNELS}
            g.render_light(rows=c.rows, stream=st, **{ch: b.t for ch, b in bufs.items()})
            return self.read(bufs, name)
        cams = [(pos, rot) for _, _, pos, rot in c.views]
        if name == "render_views":
            p1 = [Buf(self, (h, w, 3), torch.float32) for w, h, _, _ in c.views]
            g.render_views(cams, [b.t for b in p1], stream=st)
            fb = [Buf(self, (h, w, 3), torch.float32, zero=True) for w, h, _, _ in c.views]
            mask = [Buf(self, (h, w), torch.uint8) for w, h, _, _ in c.views]
            g.render_views(cams, [b.t for b in fb], [b.t for b in mask], ssaa=True, stream=st)
            bufs = {}
            for i in range(len(cams)):
                bufs.update({"pass1_%d" % i: p1[i], "ssaa_%d" % i: fb[i], "mask_%d" % i: mask[i]})
            return self.read(bufs, name)
        assert name == "render_views_aov"
        bufs = {ch: [Buf(self, (h, w) + VA.TAIL[ch], torch.int32 if VA.integer(ch) else torch.float32) for w, h, _, _ in c.views] for ch in VA.CHANNELS}
        g.render_views_aov(cams, stream=st, **{ch: [b.t for b in bs] for ch, bs in bufs.items()})
        # the batch's own rays through trace_rays: their hit records are the geometry channels, their colours pass 1 of the view
        traced = {}
        for i, b in enumerate(bufs["rays"]):
            h, col = g.trace_rays(b.t.reshape(-1, 6), stream=st)
            traced.update({"traced_hits_%d" % i: h, "traced_colours_%d" % i: col})
        out = self.read({"%s_%d" % (ch, i): b for ch, bs in bufs.items() for i, b in enumerate(bs)}, name)
        out.update(self.host(traced))
        return out

    def read(self, bufs, what):
        self.sync()
        return {k: b.read("%s, %s" % (what, k)) for k, b in bufs.items()}

    # -- the comparisons
    def check(self, name, got, where):
        c = self.case
        n = len(c.pool)

        def equal(a, want, what):
            want = np.ascontiguousarray(want)
            assert a.shape == want.shape, "%s, %s: shape %s, expected %s" % (where, what, a.shape, want.shape)
            d = U.bits(a) != U.bits(want)
            d = d.reshape(len(d), -1).any(1) if d.ndim > 1 else d
            assert not d.any(), "%s, %s: %d of %d differ from the expectation, first at %s" % (where, what, d.sum(), len(d), np.nonzero(d)[0][:5])

        if name == "trace_rays":
            hits, col = c.probe()
            equal(got["hits"], hits, "hits"); equal(got["colours"], col, "colours")
        elif name == "occluded":
            _, mixed, whole = c.occlusion()
            equal(got["mixed"], mixed, "a range per ray"); equal(got["whole"], whole, "tmax=None")
        elif name == "surface_rays":
            bad = SU.mismatches(got, c.surface())
            assert not bad, "%s: rays whose channels differ from the expectation: %s" % (where, bad)
            self.N, self.position = got["normal"], got["position"]
        elif name == "light_rays":
            exp = c.pool_light(self.N)[0]
            assert got["light_open"].shape == (n, len(c.lights[0]))
            for ch in UL.CHANNELS:
                equal(got[ch], exp[ch], ch)
        elif name == "scatter_rays":
            exp = c.scatter(self.N)
            assert got["kinds"].dtype == np.uint8
            for ch in SC.CHANNELS:
                equal(got[ch], exp[ch], ch)
        elif name == "sky":
            equal(got["sky"], c.sky(), "sky")
            miss = c.probe()[0][:, 0] == 0
            equal(got["sky"][miss], c.probe()[1][miss], "sky at the rays that miss")
        elif name == "cast_tree":
            equal(got["colours"], c.probe()[1], "colours")
        elif name == "light_points":
            exp = c.point_light(self.N)
            for ch in UP.CHANNELS:
                equal(got[ch], exp[ch], ch)
        elif name == "ao_points":
            counts, ao = c.point_ao(self.points()[0])
            equal(got["counts"].view(np.uint32), counts, "counts"); equal(got["ao"], ao, "ao")
        elif name == "radiance_points":
            pts = self.points()[0]
            col = c.memo(("radiance_colours", pts.tobytes()), lambda: c.radiance_colours(pts))
            for cosine in (False, True):
                total, counts = c.radiance(pts, cosine, col)
                equal(got["sum%d" % cosine], total, "sum, cosine %s" % cosine)
                equal(got["counts%d" % cosine].view(np.uint32), counts, "counts, cosine %s" % cosine)
        elif name == "render_aov":
            mask = U.written_mask(c.w, c.h, c.rows)
            bad = U.mismatches(got, c.frame_aov(), mask)
            assert not bad, "%s, rows %s: pixels that differ from the expectation: %s" % (where, c.rows, bad)
            for ch in U.CHANNELS:
                assert VA.touched(got[ch], ch, mask) == 0, "%s, rows %s: %s was written outside the rows" % (where, c.rows, ch)
        elif name == "render_ao":
            mask = U.written_mask(c.w, c.h, c.rows)
            counts, ao = c.frame_ao(self.N)
            equal(got["counts"].view(np.uint32)[mask], counts[mask], "counts, rows %s" % (c.rows,)); equal(got["ao"][mask], ao[mask], "ao, rows %s" % (c.rows,))
            assert (got["ao"][~mask] == f32(FILL_F)).all() and (got["counts"][~mask] == FILL_I).all(), "%s: written outside the rows %s" % (where, c.rows)
        elif name == "render_light":
            mask = U.written_mask(c.w, c.h, c.rows)
            bad = RL.differ(got, c.frame_light(self.N), mask)
            assert not bad, "%s, rows %s: (plane, pixel) entries that differ from the expectation: %s" % (where, c.rows, bad)
            assert not RL.touched(got, mask), "%s, rows %s: written outside the rows: %s" % (where, c.rows, RL.touched(got, mask))
        elif name == "render_views":
            for i, (w, h, _, _) in enumerate(c.views):
                v, mask = c.view(i), U.written_mask(w, h)
                what = "view %d (%d x %d)" % (i, w, h)
                equal(got["pass1_%d" % i][mask], v["pass1"][mask], what + " pass 1")
                assert (got["pass1_%d" % i][~mask] == f32(FILL_F)).all(), "%s, %s: pass 1 wrote outside its pixels" % (where, what)
                inner = np.ones((h, w), bool)
                inner[0, :] = False; inner[:, 0] = False          # (the reference's uninitialised mask border)
                equal(got["ssaa_%d" % i][inner], v["ssaa"][inner], what + " with the 4-sample pass")
                equal(got["mask_%d" % i] != 0, v["mask"], what + " mask")
        else:
            for i, (w, h, _, _) in enumerate(c.views):
                v, mask = c.view(i), U.written_mask(w, h)
                what = "view %d (%d x %d)" % (i, w, h)
                mine = {ch: got["%s_%d" % (ch, i)] for ch in VA.CHANNELS}
                bad = U.mismatches(mine, v["aov"], mask)
                assert not bad, "%s, %s: pixels that differ from the expectation: %s" % (where, what, bad)
                equal(mine["position"][mask], v["position"].reshape(h, w, 3)[mask], what + " position")
                equal(mine["rays"][mask], v["rays"].reshape(h, w, 6)[mask], what + " rays")
                for ch in VA.CHANNELS:
                    assert VA.touched(mine[ch], ch, mask) == 0, "%s, %s: %s was written outside its pixels" % (where, what, ch)
                hits = got["traced_hits_%d" % i].reshape(h, w, 8)
                equal(hits[..., 3][mask], mine["depth"][mask], what + " trace_rays(rays) tNear")
                equal(hits[..., 1].astype(np.int32)[mask], mine["object_id"][mask], what + " trace_rays(rays) object")
                equal(hits[..., 2].astype(np.int32)[mask], mine["triangle_id"][mask], what + " trace_rays(rays) triangle")
                equal(hits[..., 4:6][mask], mine["uv"][mask], what + " trace_rays(rays) uv")
                equal(got["traced_colours_%d" % i].reshape(h, w, 3)[mask], v["pass1"][mask], what + " trace_rays(rays) colours")


def detour(run, where):
    """Another camera, the other culling value, another size; one frame there, against the oracle; then everything back."""
    c, g = run.case, run.g
    w, h, pos, rot = c.detour
    before = (g.camera_pose(), g.kernel_variant(), [a.copy() for a in g.camera()])
    g.set_camera(pos, rot)
    g.set_flag("useBackfaceCulling", 1 - c.cull)
    g.resize(w, h)
    with run.on():
        fb = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda"); mask = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
    g.render_frame(fb, mask, stream=run.stream)
    run.sync()
    assert g.frame_status() == 0
    assert g.kernel_variant()["cull"] == bool(1 - c.cull)
    frame, flags = c.detour_frame()
    d = (U.bits(fb.cpu().numpy()) != U.bits(frame)).any(-1)
    assert not d.any(), "%s: %d pixels of the frame at %d x %d differ from the oracle" % (where, d.sum(), w, h)
    assert np.array_equal(mask.cpu().numpy() != 0, flags), "%s: the mask of the frame at %d x %d differs from the oracle's" % (where, w, h)
    g.resize(c.w, c.h)
    g.set_flag("useBackfaceCulling", c.cull)
    g.set_camera(*before[0])
    assert g.kernel_variant() == before[1] and all(np.array_equal(a, b) for a, b in zip(before[2], g.camera())), "%s: the first state did not come back" % where


@pytest.mark.parametrize("seed", Q.SEEDS)
def test_queries_on_a_random_scene(ra, oracle, qdir, seed):
    t0 = time.time()
    c = Q.Case(oracle, seed, qdir)
    live = ra.live_device_memory()
    g = ra.Scene(c.path, c.w, c.h)
    try:
        g.gpu()
        v = g.kernel_variant()
        assert ("analytic" if v["analytic"] else "plain" if v["plain"] else "general") == c.family and v["cull"] == bool(c.cull)
        recs, pts = g.device_lights()
        assert list(recs["type"]) == list(c.lights[0]["type"]) and list(recs["n_points"]) == list(c.lights[0]["n_points"])
        assert np.array_equal(U.bits(pts), U.bits(c.lights[1])), "seed %d: the area lights' sample points are not the scene file's" % seed
        assert all(np.array_equal(a, b) for a, b in zip(g.camera_pose(), (f32(c.pose[0]), f32(c.pose[1]))))
        if seed % 2:
            g.set_knob("trace_reorder", 1)           # the grouping path, which batches of this size do not take by themselves
        run = Run(c, g, torch.cuda.Stream() if seed % 3 == 0 else None)
        first = {}
        mid = len(c.order) // 2
        for at, name in enumerate(c.order):
            if at == mid:
                detour(run, "seed %d, the detour before call %d" % (seed, at))
                for k, earlier in enumerate(c.order[:mid]):
                    again = run.call(earlier)
                    diff = [key for key in first[earlier] if not same_bits(again[key], first[earlier][key])]
                    assert not diff, "seed %d, %s (call %d of %s) made again after the detour: %s changed" % (seed, earlier, k, c.order, diff)
            first[name] = run.call(name)
            run.check(name, first[name], "seed %d, %s (call %d of %s)" % (seed, name, at, c.order))
        run.sync()
    finally:
        g.close()
    assert ra.live_device_memory() == live, "seed %d: device memory is still held after close()" % seed
    print("seed %d (%d x %d, %s, %d lights, %d rays): %.1f s" % (seed, c.w, c.h, c.family, len(c.lights[0]), len(c.pool), time.time() - t0))
