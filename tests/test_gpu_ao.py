"""rtx_render_ao / Scene.render_ao: ambient occlusion of a frame in one launch (include/rtx_ao.h), every bit of `counts` and `ao` over every
written pixel against the expectation of tests/util_ao.py -- the traced rays answered by the CPU oracle (yardstick (i)) and by
Scene.occluded (yardstick (ii)) --; the strict range; what is not asked for or not owned stays untouched; the ordinary frames are not
disturbed; edited scenes, other streams, flags and refusals."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import util_ao as AO
from tests import util_aov as U
from tests import util_lights as L
from tests import util_shading as S
from tests.util_move import edit_scene
from tests.util_objects import apply_step, write_scene

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = U.ROOT
f32 = np.float32
GUARD = 96                    # untouched elements before and after every buffer
FILL = {"ao": 7.25, "counts": 0x0BADF00D}
DTYPE = {"ao": torch.float32, "counts": torch.int32}
BOTH = ("ao", "counts")
RADII = (float("inf"), 1.0, 0.25)


@pytest.fixture(scope="module")
def family(tmp_path_factory):
    d = S.short_dir(tmp_path_factory)
    return d, S.write_family(d)


def path_of(name, family):
    return family[1][name] if name in S.FAMILY else "scenes/%s.scene" % name


class Buffers:
    """`names` of a w x h frame, each in the middle of a larger pre-filled allocation."""

    def __init__(self, w, h, names=BOTH):
        self.w, self.h, self.names = w, h, tuple(names)
        self.flat, self.view = {}, {}
        for c in self.names:
            self.flat[c] = torch.full((w * h + 2 * GUARD,), FILL[c], dtype=DTYPE[c], device="cuda")
            self.view[c] = self.flat[c][GUARD:GUARD + w * h].view(h, w)
            assert self.view[c].is_contiguous()

    def read(self):
        """name -> numpy frame, after checking the guards"""
        torch.cuda.synchronize()
        out = {}
        for c in self.names:
            f = self.flat[c].cpu().numpy()
            fill = f.dtype.type(FILL[c])
            assert (f[:GUARD] == fill).all() and (f[-GUARD:] == fill).all(), "%s: written outside the buffer" % c
            out[c] = f[GUARD:-GUARD].reshape(self.h, self.w)
        return out


def untouched(got, mask):
    """names of the buffers with a changed element outside `mask`"""
    return [c for c, a in got.items() if not (a == a.dtype.type(FILL[c]))[~mask].all()]


def dirs_t(dirs):
    return torch.from_numpy(np.ascontiguousarray(dirs, f32)).cuda()


def render(g, dirs, radius=float("inf"), names=BOTH, rows=None, stream=None):
    b = Buffers(g.width, g.height, names)
    g.render_ao(dirs if isinstance(dirs, torch.Tensor) else dirs_t(dirs), radius, rows=rows, stream=stream, **b.view)
    return b.read()


def differ(got, want, mask, names=BOTH):
    """{name: number of pixels of `mask` whose bits differ}: empty = equal.  want: (counts, ao) of util_ao or a dict like got."""
    if isinstance(want, tuple):
        want = {"counts": want[0], "ao": want[1]}
    bad = {}
    for c in names:
        d = U.bits(got[c]).view(np.uint32) != U.bits(np.ascontiguousarray(want[c])).view(np.uint32)
        if d[mask].any():
            bad[c] = int(d[mask].sum())
    return bad


# ---- 1. every bit against the oracle's answers and against Scene.occluded's -----------------------------------------------------------
@pytest.mark.parametrize("cull", [1, 0])
@pytest.mark.parametrize("name", U.REPO_SCENES + U.FAMILY_SCENES)
def test_counts_and_ao_equal_both_yardsticks(ra, oracle, family, tmp_path, name, cull):
    w, h = U.size_of(name)
    path = path_of(name, family)
    g = ra.Scene(path, w, h)
    g.set_flag("useBackfaceCulling", cull)
    e = AO.Expectation(g, AO.DIRS19)
    mask = U.written_mask(w, h)
    for radius in RADII:
        what = "%s %dx%d cull %d radius %g" % (name, w, h, cull, radius)
        by_oracle = e.by_oracle(oracle, path, tmp_path, cull, radius)
        by_occluded = e.by_occluded(radius)
        got = render(g, AO.DIRS19, radius)
        ntr = by_oracle[0] >> 16
        print("%s: %d traced rays, %d open, ao mean %.3f" % (what, ntr.sum(), (by_oracle[0] & 0xFFFF).sum(), by_oracle[1][mask].mean()))
        # (i) == (ii) first, so that a failure says which side moved
        assert np.array_equal(by_oracle[0], by_occluded[0]) and np.array_equal(U.bits(by_oracle[1]), U.bits(by_occluded[1])), \
            "%s: Scene.occluded and the oracle disagree on the traced rays" % what
        bad = differ(got, by_oracle, mask)
        assert not bad, "%s: pixels that differ from the oracle's answers: %s" % (what, bad)
        bad = differ(got, by_occluded, mask)
        assert not bad, "%s: pixels that differ from Scene.occluded's answers: %s" % (what, bad)
        assert not untouched(got, mask)
    g.close()


# ---- 2. the strict range --------------------------------------------------------------------------------------------------------------
def test_the_range_is_strict(ra, oracle, tmp_path):
    """A traced ray's own tNear' as the radius leaves it open (tNear' < radius is false); one ulp more closes it."""
    name = "cfg2_smooth_4k"
    path = "scenes/%s.scene" % name
    w, h = 24, 40
    g = ra.Scene(path, w, h)
    dirs = ra.sphere_directions(12)
    e = AO.Expectation(g, dirs)
    hit, t = e.probe(oracle, path, tmp_path, None)
    blocked = np.flatnonzero(hit & (t < 1e3) & (t > 1e-3))
    assert len(blocked) > 100
    # three rays of three different pixels, spread over the blocked ones
    picks = []
    for j in blocked[[len(blocked) // 7, len(blocked) // 2, len(blocked) * 6 // 7]]:
        assert e.pix[j] not in [e.pix[q] for q in picks]
        picks.append(int(j))
    for j in picks:
        y, x = divmod(int(e.pix[j]), w)
        rows = (y, y + 1)
        mask = U.written_mask(w, h, rows)
        assert mask[y, x]
        opened = []
        for radius in (t[j], np.nextafter(t[j], f32(np.inf))):
            want = e.by_oracle(oracle, path, tmp_path, None, radius)
            got = render(g, dirs, float(radius), rows=rows)
            assert not differ(got, want, mask), "pixel (%d, %d), radius %r" % (x, y, radius)
            assert not untouched(got, mask)
            opened.append((int(got["counts"][y, x]) & 0xFFFF, int(want[0][y, x]) & 0xFFFF))
        # the picked ray, and whatever else of the pixel has the very same tNear', is open at its own tNear' and closed one ulp above
        same_t = int(((e.pix == e.pix[j]) & hit & (t == t[j])).sum())
        assert same_t >= 1 and opened[0][1] - opened[1][1] == same_t
        assert opened[0][0] - opened[1][0] == same_t
    g.close()


# ---- 3. the outputs are independent, and only the asked pixels are written ----------------------------------------------------------------
@pytest.mark.parametrize("name,rows", [("cfg4_textured_256", (3, 13)), ("mixed_materials", (9, 17)), ("cfg1_simple_shapes", (0, 24))])
def test_only_what_was_asked_for_is_written(ra, name, rows):
    w, h = U.size_of(name)
    g = ra.Scene("scenes/%s.scene" % name, w, h)
    full = render(g, AO.DIRS19, 1.0)
    whole = U.written_mask(w, h)
    assert not untouched(full, whole)
    mask = U.written_mask(w, h, rows)
    assert mask.sum() < whole.sum() or rows == (0, h)
    for names in (("ao",), ("counts",), BOTH):
        got = render(g, AO.DIRS19, 1.0, names, rows)
        assert set(got) == set(names)
        assert not untouched(got, mask), "%s: written outside rows %s" % (names, rows)
        assert not differ(got, full, mask, names), "%s alone differs from the two-output call" % (names,)
    # rows past the frame are cut, an empty range does nothing
    got = render(g, AO.DIRS19, 1.0, BOTH, (h - 3, h + 100))
    assert not untouched(got, U.written_mask(w, h, (h - 3, h))) and not differ(got, full, U.written_mask(w, h, (h - 3, h)))
    for empty in ((5, 5), (7, 2), (h - 1, h), (h, h + 8)):
        assert not untouched(render(g, AO.DIRS19, 1.0, BOTH, empty), np.zeros((h, w), bool))
    g.close()


# ---- 4. the number of directions --------------------------------------------------------------------------------------------------------
def test_one_direction_and_256(ra, oracle, tmp_path):
    name = "cfg2_smooth_4k"
    path = "scenes/%s.scene" % name
    w, h = 33, 17
    g = ra.Scene(path, w, h)
    mask = U.written_mask(w, h)
    for dirs in (np.array([[0.3, 1, 0.2]], f32), ra.sphere_directions(256)):
        e = AO.Expectation(g, dirs)
        want = e.by_oracle(oracle, path, tmp_path, None, np.inf)
        got = render(g, dirs)
        assert not differ(got, want, mask), "%d directions" % len(dirs)
        assert not differ(got, e.by_occluded(np.inf), mask), "%d directions" % len(dirs)
        traced, opened = got["counts"].view(np.uint32)[mask] >> 16, got["counts"].view(np.uint32)[mask] & 0xFFFF
        if len(dirs) == 256:
            # (a byte-wide accumulator would fail here)
            assert traced.max() > 127 and opened.max() > 127 and traced.max() <= 256
        else:
            assert traced.max() == 1 and set(np.unique(got["ao"][mask])) == {f32(0), f32(1)}
    g.close()


# ---- 5. the order of the directions -----------------------------------------------------------------------------------------------------
def test_direction_order(ra):
    name = "cfg1_simple_shapes"
    w, h = U.size_of(name)
    g = ra.Scene("scenes/%s.scene" % name, w, h)
    mask = U.written_mask(w, h)
    obj = torch.full((h, w), -1, dtype=torch.int32, device="cuda")
    g.render_aov(object_id=obj)
    torch.cuda.synchronize()
    plane = (obj.cpu().numpy() == 0) & mask                 # object 0: the plane with normal (0, 1, 0)
    assert plane.sum() > 50
    # no direction with c > 0 on the plane: c == 0, c < 0, zero, NaN
    below = np.array([[1, 0, 0], [0, 0, 1], [0, -1, 0], [0, 0, 0], [np.nan, 0, 0], [2, -3, 1], [0, np.nan, 0]], f32)
    got = render(g, below)
    assert (got["counts"][plane] == 0).all() and (U.bits(got["ao"])[plane] == U.bits(np.array([1], f32))[0]).all()
    assert (got["counts"][mask & ~plane] != 0).any()
    full = render(g, AO.DIRS19, 1.0)
    for seed in (1, 2):
        perm = np.random.default_rng(seed).permutation(len(AO.DIRS19))
        assert not differ(render(g, AO.DIRS19[perm], 1.0), full, mask), "a permutation of the directions changes the result"
    g.close()


# ---- 6. row ownership -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("halo", [True, False])
def test_row_ownership(ra, halo):
    name = "cfg2_smooth_4k"
    w, h = 24, 40
    g = ra.Scene("scenes/%s.scene" % name, w, h)
    full = render(g, AO.DIRS19, 1.0)
    union = {c: a.copy() for c, a in render(g, AO.DIRS19, 1.0, BOTH, (0, 0)).items()}      # (all pattern)
    for part in range(3):
        g.set_row_ownership(8, 3, part, halo)
        got = render(g, AO.DIRS19, 1.0)
        mask = U.written_mask(w, h, band=8, parts=3, part=part)
        assert mask.any()
        assert not untouched(got, mask), "part %d wrote rows it does not own" % part
        assert not differ(got, full, mask)
        for c in BOTH:
            union[c][mask] = got[c][mask]
    g.set_row_ownership(0, 1, 0)
    whole = U.written_mask(w, h)
    assert not differ(union, full, whole) and not untouched(union, whole)
    g.close()


# ---- 7. the ordinary frame is undisturbed -----------------------------------------------------------------------------------------------
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
    got = render(g, ra.sphere_directions(12), 1.0)
    assert g.frame_mode() == mode and np.array_equal(costs, g.tile_cost())
    after = frame()
    assert np.array_equal(U.bits(before[0]), U.bits(after[0])) and np.array_equal(before[1], after[1])
    e = AO.Expectation(g, ra.sphere_directions(12))
    assert not differ(got, e.by_occluded(1.0), U.written_mask(w, h))
    g.close()


# ---- 8. live scene ----------------------------------------------------------------------------------------------------------------------
def test_edited_scene_equals_a_fresh_one(ra, tmp_path):
    name = "mixed_materials"
    w, h = 40, 24
    text = open(os.path.join(ROOT, "scenes", name + ".scene")).read()
    g = ra.Scene("scenes/%s.scene" % name, w, h)
    render(g, AO.DIRS19, 1.0)
    steps = [("move", 3, dict(pos=(0.4, 1.2, -5.5), radius=0.85)),                      # a sphere
             ("move", 1, dict(rot=(-40, 10, 70), pos=(-0.9, 0.2, -4.4))),               # a mesh
             ("add", "sphere", None, dict(pos=(-0.6, -0.3, -2.5), color=(0.2, 0.9, 0.4), radius=0.4)),
             ("remove", 0),
             ("light", 0, dict(position=(-1.5, 2.0, -1.0), intensity=0.5)),
             ("resize", 33, 17)]
    for k, step in enumerate(steps):
        if step[0] == "move":
            g.move_object(step[1], **step[2])
            text = edit_scene(text, step[1], **step[2])
        elif step[0] == "light":
            text = L.apply_step(g, text, ("set", step[1], step[2]))
        elif step[0] == "resize":
            w, h = step[1], step[2]
            g.resize(w, h)
        else:
            text = apply_step(g, text, step)
        f = ra.Scene(write_scene(tmp_path, text, "ao_%d" % k), w, h)
        mask = U.written_mask(w, h)
        for radius in (float("inf"), 0.5):
            got, want = render(g, AO.DIRS19, radius), render(f, AO.DIRS19, radius)
            assert not differ(got, want, mask), "step %d %s: differs from a fresh scene" % (k, step[0])
            assert not untouched(got, mask)
        assert not differ(got, AO.Expectation(g, AO.DIRS19).by_occluded(0.5), mask), "step %d %s: differs from Scene.occluded" % (k, step[0])
        f.close()
    g.close()


# ---- 9. another stream ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("as_current", [False, True])
def test_another_stream_gives_the_same_bits(ra, as_current):
    name = "cfg2_smooth_4k"
    w, h = 64, 64
    g = ra.Scene("scenes/%s.scene" % name, w, h)
    mask = U.written_mask(w, h)
    want = render(g, AO.DIRS19, 1.0)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    for _ in range(3):
        with torch.cuda.stream(st):
            b = Buffers(w, h)         # (filled on st: a call that did not wait for the fill would be overwritten by it)
            d = dirs_t(AO.DIRS19)
            if as_current:
                g.render_ao(d, 1.0, **b.view)
            else:
                g.render_ao(d, 1.0, stream=st, **b.view)
        st.synchronize()
        got = b.read()
        assert not differ(got, want, mask) and not untouched(got, mask)
    g.close()


# ---- 10. flags and refusals -------------------------------------------------------------------------------------------------------------
def test_show_normals_and_ray_depth_change_nothing(ra, tmp_path):
    from tests.ac_heatmap import scene_copy
    name = "cfg3_reflective_refractive"
    w, h = U.size_of(name)
    g = ra.Scene("scenes/%s.scene" % name, w, h)
    full = render(g, AO.DIRS19, 1.0)
    mask = U.written_mask(w, h)
    for flag in ("showNormals", "useSkybox"):
        g.set_flag(flag, 1)
        assert not differ(render(g, AO.DIRS19, 1.0), full, mask), flag
        g.set_flag(flag, 0)
    g.close()
    for depth in (0, 1):
        f = ra.Scene(scene_copy(name, str(tmp_path), dict(max_ray_depth=depth)), w, h)
        assert not differ(render(f, AO.DIRS19, 1.0), full, mask), "max_ray_depth = %d" % depth
        f.close()


def test_refusals_leave_the_buffers_untouched(ra):
    w, h = 40, 24
    g = ra.Scene("scenes/cfg1_simple_shapes.scene", w, h)
    rtx, _ = ra.load()
    b = Buffers(w, h)
    none = np.zeros((h, w), bool)
    d = dirs_t(AO.DIRS19)
    big = torch.zeros((300, 3), dtype=torch.float32, device="cuda")
    g.counters_enable(True)
    with pytest.raises(ra.RtxError):
        g.render_ao(d, **b.view)
    par = ra.AoParams(19, d.data_ptr(), 1.0)
    ao, counts = C.c_void_p(b.view["ao"].data_ptr()), C.c_void_p(b.view["counts"].data_ptr())
    assert rtx.rtx_render_ao(g.gpu(), 0, h, C.byref(par), ao, counts, None) == -4       # RTX_ERR_UNSUPPORTED
    g.counters_enable(False)
    assert not untouched(b.read(), none)
    # RTX_ERR_ARG
    P = ra.AoParams
    cases = [(None, C.byref(par), ao, counts, "a NULL scene"), (g.gpu(), None, ao, counts, "NULL params"),
             (g.gpu(), C.byref(par), None, None, "both outputs NULL"),
             (g.gpu(), C.byref(P(19, None, 1.0)), ao, counts, "NULL dirs_dev"),
             (g.gpu(), C.byref(P(0, d.data_ptr(), 1.0)), ao, counts, "n_dirs 0"),
             (g.gpu(), C.byref(P(257, big.data_ptr(), 1.0)), ao, counts, "n_dirs 257"),
             (g.gpu(), C.byref(P(19, d.data_ptr(), float("nan"))), ao, counts, "radius NaN"),
             (g.gpu(), C.byref(P(19, d.data_ptr(), 0.0)), ao, counts, "radius 0"),
             (g.gpu(), C.byref(P(19, d.data_ptr(), -1.0)), ao, counts, "radius -1"),
             (g.gpu(), C.byref(P(19, d.data_ptr(), float("-inf"))), ao, counts, "radius -inf")]
    for scene, params, a, c, what in cases:
        assert rtx.rtx_render_ao(scene, 0, h, params, a, c, None) == -1, what
        assert rtx.rtx_last_error(), what
    for radius in (float("nan"), 0.0, -2.0):
        with pytest.raises(ra.RtxError):
            g.render_ao(d, radius, **b.view)
    with pytest.raises(ra.RtxError):
        g.render_ao(big, **b.view)
    assert not untouched(b.read(), none)
    # the Python checks, in render_aov's wording
    z = lambda shape, dt=torch.float32, dev="cuda": torch.zeros(shape, dtype=dt, device=dev)
    bad = [(dict(ao=z((h, w), torch.float64)), "ao must be float32"), (dict(counts=z((h, w))), "counts must be int32"),
           (dict(counts=z((h, w), torch.uint8)), "counts must be int32"),
           (dict(ao=z((w, h))), r"ao must have shape \(24, 40\)"), (dict(counts=z((h, w, 1), torch.int32)), r"counts must have shape \(24, 40\)"),
           (dict(ao=z((w, h)).t()), "ao must be contiguous"), (dict(counts=z((h, 2 * w), torch.int32)[:, ::2]), "counts must be contiguous"),
           (dict(ao=z((h, w), dev="cpu")), "ao must be on cuda:0"), (dict(counts=z((h, w), torch.int32, "cpu")), "counts must be on cuda:0"),
           (dict(ao=np.zeros((h, w), f32)), "ao must be a torch tensor"), (dict(), "at least one buffer")]
    for kw, what in bad:
        with pytest.raises(ValueError, match=what):
            g.render_ao(d, **kw)
    with pytest.raises(ValueError, match="dirs must be on cuda:0"):
        g.render_ao(d.cpu(), **b.view)
    with pytest.raises(ValueError, match=r"dirs must have shape \(K, 3\)"):
        g.render_ao(z((19, 4)), **b.view)
    assert not untouched(b.read(), none)
    # ... and the call works afterwards
    g.render_ao(d, 1.0, **b.view)
    got = b.read()
    assert not untouched(got, U.written_mask(w, h))
    assert not differ(got, AO.Expectation(g, AO.DIRS19).by_occluded(1.0), U.written_mask(w, h))
    g.close()
