"""rtx_render_aov / Scene.render_aov: the first-hit buffers of a frame -- depth, object id, triangle id, uv, normal, albedo -- against the CPU
oracle (tests/util_aov.py), bit for bit over every written pixel; what is not asked for or not owned stays untouched; the ordinary frames
are not disturbed; edited scenes, other streams, and the library's own other route to the same data (trace_rays, hits only)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import util_aov as U
from tests import util_shading as S
from tests.util_move import edit_scene
from tests.util_objects import apply_step, write_scene

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = U.ROOT
GUARD = 96                    # untouched elements before and after every buffer
FILL_F, FILL_I = 7.25, 0x0BADF00D
TAIL = {"depth": (), "object_id": (), "triangle_id": (), "uv": (2,), "normal": (3,), "albedo": (3,)}


@pytest.fixture(scope="module")
def family(tmp_path_factory):
    d = S.short_dir(tmp_path_factory)
    return d, S.write_family(d)


def path_of(name, family):
    return family[1][name] if name in S.FAMILY else "scenes/%s.scene" % name


class Buffers:
    """The channels `names` of a w x h frame, each in the middle of a larger pre-filled allocation."""

    def __init__(self, w, h, names=U.CHANNELS):
        self.w, self.h, self.names = w, h, tuple(names)
        self.flat, self.view = {}, {}
        for c in self.names:
            shape = (h, w) + TAIL[c]
            n = int(np.prod(shape))
            integer = c.endswith("_id")
            self.flat[c] = torch.full((n + 2 * GUARD,), FILL_I if integer else FILL_F, dtype=torch.int32 if integer else torch.float32, device="cuda")
            self.view[c] = self.flat[c][GUARD:GUARD + n].view(shape)
            assert self.view[c].is_contiguous()

    def read(self):
        """channel -> numpy frame, after checking the guards"""
        torch.cuda.synchronize()
        out = {}
        for c in self.names:
            f = self.flat[c].cpu().numpy()
            fill = f.dtype.type(FILL_I if c.endswith("_id") else FILL_F)
            assert (f[:GUARD] == fill).all() and (f[-GUARD:] == fill).all(), "%s: written outside the buffer" % c
            out[c] = f[GUARD:-GUARD].reshape((self.h, self.w) + TAIL[c])
        return out


def untouched(got, mask):
    """names of the channels with a changed element outside `mask`"""
    bad = []
    for c, a in got.items():
        fill = a.dtype.type(FILL_I if c.endswith("_id") else FILL_F)
        keep = a == fill
        keep = keep.all(-1) if keep.ndim == 3 else keep
        if not keep[~mask].all():
            bad.append(c)
    return bad


def render(g, names=U.CHANNELS, rows=None, stream=None):
    b = Buffers(g.width, g.height, names)
    g.render_aov(rows=rows, stream=stream, **b.view)
    return b.read()


def same(a, b, mask, names):
    """names of the channels whose bits differ between two results inside `mask`"""
    bad = []
    for c in names:
        d = U.bits(a[c]) != U.bits(b[c])
        d = d.any(-1) if d.ndim == 3 else d
        if d[mask].any():
            bad.append(c)
    return bad


# ---- 1. every channel against the oracle ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cull", [1, 0])
@pytest.mark.parametrize("name", U.REPO_SCENES + U.FAMILY_SCENES)
def test_channels_equal_the_oracle(ra, family, name, cull):
    w, h = U.size_of(name)
    path = path_of(name, family)
    exp = U.expected_of(path, w, h, cull)
    g = ra.Scene(path, w, h)
    g.set_flag("useBackfaceCulling", cull)
    got = render(g)
    mask = U.written_mask(w, h)
    bad = U.mismatches(got, exp, mask)
    assert not bad, "%s %dx%d cull %d: pixels that differ from the oracle, per channel: %s" % (name, w, h, cull, bad)
    assert not untouched(got, mask)
    g.close()


# ---- 2. only what was asked for is written --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,rows", [("cfg4_textured_256", (3, 13)), ("mixed_materials", (9, 17)), ("cfg1_simple_shapes", (0, 24))])
def test_only_what_was_asked_for_is_written(ra, name, rows):
    w, h = U.size_of(name)
    g = ra.Scene("scenes/%s.scene" % name, w, h)
    full = render(g)
    whole = U.written_mask(w, h)
    assert not untouched(full, whole)
    assert not U.mismatches(full, U.expected_of("scenes/%s.scene" % name, w, h), whole)
    mask = U.written_mask(w, h, rows)
    assert mask.sum() < whole.sum() or rows == (0, h)
    for names in [(c,) for c in U.CHANNELS] + [U.GEOMETRY, U.CHANNELS]:
        got = render(g, names, rows)
        assert set(got) == set(names)
        assert not untouched(got, mask), "%s: written outside rows %s" % (names, rows)
        assert not same(got, full, mask, names), "%s alone differs from the six-channel call" % (names,)
    # rows past the frame are cut, an empty range does nothing
    got = render(g, U.CHANNELS, (h - 3, h + 100))
    assert not untouched(got, U.written_mask(w, h, (h - 3, h))) and not same(got, full, U.written_mask(w, h, (h - 3, h)), U.CHANNELS)
    for empty in ((5, 5), (7, 2), (h - 1, h), (h, h + 8)):
        assert not untouched(render(g, U.CHANNELS, empty), np.zeros((h, w), bool))
    g.close()


# ---- 3. row ownership -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("halo", [True, False])
def test_row_ownership(ra, halo):
    name = "cfg2_smooth_4k"
    w, h = 24, 40
    g = ra.Scene("scenes/%s.scene" % name, w, h)
    full = render(g)
    union = {c: a.copy() for c, a in render(g, U.CHANNELS, (0, 0)).items()}      # (all pattern)
    for part in range(3):
        g.set_row_ownership(8, 3, part, halo)
        got = render(g)
        mask = U.written_mask(w, h, band=8, parts=3, part=part)
        assert mask.any()
        assert not untouched(got, mask), "part %d wrote rows it does not own" % part
        assert not same(got, full, mask, U.CHANNELS)
        for c in U.CHANNELS:
            union[c][mask] = got[c][mask]
    g.set_row_ownership(0, 1, 0)
    whole = U.written_mask(w, h)
    assert not same(union, full, whole, U.CHANNELS) and not untouched(union, whole)
    g.close()


# ---- 4. flags and refusals ------------------------------------------------------------------------------------------------------------
def test_show_normals_and_ray_depth_change_nothing(ra, tmp_path):
    from tests.ac_heatmap import scene_copy
    name = "cfg3_reflective_refractive"
    w, h = U.size_of(name)
    g = ra.Scene("scenes/%s.scene" % name, w, h)
    full = render(g)
    mask = U.written_mask(w, h)
    g.set_flag("showNormals", 1)
    assert not same(render(g), full, mask, U.CHANNELS)
    assert not U.mismatches(render(g), U.expected_of("scenes/%s.scene" % name, w, h), mask)
    g.set_flag("showNormals", 0)
    g.close()
    for depth in (0, 1):
        f = ra.Scene(scene_copy(name, str(tmp_path), dict(max_ray_depth=depth)), w, h)
        assert not same(render(f), full, mask, U.CHANNELS), "max_ray_depth = %d" % depth
        f.close()


def test_refusals_leave_the_buffers_untouched(ra):
    g = ra.Scene("scenes/cfg1_simple_shapes.scene", 40, 24)
    rtx, _ = ra.load()
    b = Buffers(40, 24)
    none = np.zeros((24, 40), bool)
    g.counters_enable(True)
    with pytest.raises(ra.RtxError):
        g.render_aov(**b.view)
    assert not untouched(b.read(), none)
    g.counters_enable(False)
    # the all-NULL struct, a NULL struct
    empty = ra.AovBuffers()
    assert rtx.rtx_render_aov(g.gpu(), 0, 24, C.byref(empty), None) == -1
    assert b"NULL" in rtx.rtx_last_error()
    assert rtx.rtx_render_aov(g.gpu(), 0, 24, None, None) == -1
    # ... and the call works afterwards
    g.render_aov(**b.view)
    assert not U.mismatches(b.read(), U.expected_of("scenes/cfg1_simple_shapes.scene", 40, 24), U.written_mask(40, 24))
    g.close()


# ---- 5. the ordinary frame is undisturbed -----------------------------------------------------------------------------------------------
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
    got = render(g)
    assert g.frame_mode() == mode and np.array_equal(costs, g.tile_cost())
    after = frame()
    assert np.array_equal(U.bits(before[0]), U.bits(after[0])) and np.array_equal(before[1], after[1])
    assert not U.mismatches(got, U.expected_of("scenes/cfg2_smooth_4k.scene", w, h), U.written_mask(w, h))
    g.close()


# ---- 6. live scene ----------------------------------------------------------------------------------------------------------------------
def test_edited_scene_equals_a_fresh_one(ra, tmp_path):
    name = "mixed_materials"
    w, h = 40, 24
    text = open(os.path.join(ROOT, "scenes", name + ".scene")).read()
    g = ra.Scene("scenes/%s.scene" % name, w, h)
    render(g)
    steps = [("move", 3, dict(pos=(0.4, 1.2, -5.5), radius=0.85)),                      # a sphere
             ("move", 1, dict(rot=(-40, 10, 70), pos=(-0.9, 0.2, -4.4))),               # a mesh
             ("add", "sphere", None, dict(pos=(-0.6, -0.3, -2.5), color=(0.2, 0.9, 0.4), radius=0.4)),
             ("remove", 0),
             ("resize", 33, 17)]
    for k, step in enumerate(steps):
        if step[0] == "move":
            g.move_object(step[1], **step[2])
            text = edit_scene(text, step[1], **step[2])
        elif step[0] == "resize":
            w, h = step[1], step[2]
            g.resize(w, h)
        else:
            text = apply_step(g, text, step)
        p = write_scene(tmp_path, text, "aov_%d" % k)
        f = ra.Scene(p, w, h)
        got, want = render(g), render(f)
        mask = U.written_mask(w, h)
        assert not same(got, want, mask, U.CHANNELS), "step %d %s: differs from a fresh scene" % (k, step[0])
        assert not untouched(got, mask)
        assert not U.mismatches(got, U.expected_of(p, w, h), mask), "step %d %s: differs from the oracle" % (k, step[0])
        f.close()
    g.close()


# ---- 7. another stream ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("as_current", [False, True])
def test_buffers_written_on_another_stream(ra, as_current):
    name = "cfg2_smooth_4k"
    w, h = 64, 64
    g = ra.Scene("scenes/%s.scene" % name, w, h)
    exp = U.expected_of("scenes/%s.scene" % name, w, h)
    mask = U.written_mask(w, h)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    for _ in range(3):
        with torch.cuda.stream(st):
            b = Buffers(w, h)         # (filled on st: a call that did not wait for the fill would be overwritten by it)
            if as_current:
                g.render_aov(**b.view)
            else:
                g.render_aov(stream=st, **b.view)
        st.synchronize()
        got = b.read()
        assert not U.mismatches(got, exp, mask) and not untouched(got, mask)
    g.close()


# ---- 8. the library's other route -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,size", [("cfg2_smooth_4k", (64, 64)), ("cfg4_textured_256", (40, 24)), ("cfg1_simple_shapes", (33, 17))])
def test_trace_rays_gives_the_same_geometry(ra, name, size):
    """trace_rays walks these rays without the camera's copies of the prune records, render_aov with them."""
    w, h = size
    g = ra.Scene("scenes/%s.scene" % name, w, h)
    got = render(g, U.GEOMETRY)
    rays = torch.from_numpy(U.primary_rays(g)).cuda()
    hits, _ = g.trace_rays(rays, hits=True, colours=False)
    torch.cuda.synchronize()
    hits = hits.cpu().numpy()
    want = dict(depth=hits[:, 3].reshape(h, w), object_id=hits[:, 1].astype(np.int32).reshape(h, w),
                triangle_id=hits[:, 2].astype(np.int32).reshape(h, w), uv=hits[:, 4:6].reshape(h, w, 2))
    assert not same(got, want, U.written_mask(w, h), U.GEOMETRY)
    g.close()
