"""rtx_render_views_aov / Scene.render_views_aov on the device: every view of a batch against resize + set_camera + render_aov on a second
scene of the same file, the closure of the `rays` channel on the ray queries (trace_rays, surface_rays, render_views), the oracle at fovs of
the views' own, channel subsets, batches of many times the resident waves, and what the call must leave alone -- every byte outside the
written pixels, the scene's own view, its tile costs and timings.  Every expectation is bit equality."""
import os

import numpy as np
import pytest
import torch

from tests import util_aov as U
from tests import util_shading as S
from tests import util_views_aov as V

pytestmark = pytest.mark.gpu

ROOT = U.ROOT
SIZES, POSES = V.SIZES, V.POSES


@pytest.fixture(scope="module")
def family(tmp_path_factory):
    return S.write_family(S.short_dir(tmp_path_factory))


def path_of(name, family):
    return family[name] if name in S.FAMILY else "scenes/%s.scene" % name


# ---- 1. every view equals the one-view call, 2. closure on the ray queries --------------------------------------------------------------
@pytest.mark.parametrize("name,cull", [("cfg1_simple_shapes", 1), ("cfg2_smooth_4k", 1), ("cfg2_smooth_4k", 0), ("cfg4_textured_256", 1), ("cfg4_textured_256", 0),
                                       ("mixed_materials", 1), ("mixed_materials", 0), ("plain_nrm", 1), ("plain_nrm", 0), ("mixed", 1), ("mixed", 0)])
def test_every_view_equals_the_one_view_call(ra, family, name, cull):
    """(`plain_nrm`: a normal map; `mixed`: the shading family's scene with every material, maps and the skybox flag on.)"""
    path = path_of(name, family)
    g = ra.Scene(path, 24, 16)
    g.set_flag("useBackfaceCulling", cull)
    kv = g.kernel_variant()
    assert kv["analytic"] == (name == "cfg1_simple_shapes") and (kv["analytic"] or kv["cull"] == bool(cull)) and not kv["stats"]
    if name == "mixed":
        assert g.view_flags() & 2, "the skybox flag is not on"
    cams = V.cams_of(g)
    setup = lambda f: f.set_flag("useBackfaceCulling", cull)
    want = V.loop(ra, path, cams, SIZES, setup=setup)
    assert sum(int((w["object_id"] >= 0).sum()) for w in want if w) > 500, "the batch hits too little to test the surface channels"
    got, bufs = V.batch(g, cams, SIZES, keep=True)
    V.compare(got, want, SIZES, U.CHANNELS, "%s cull %d" % (name, cull))
    # the two views of one pose and size got the same buffers
    assert all(np.array_equal(U.bits(got[6][c]), U.bits(got[7][c])) for c in V.CHANNELS)
    # trace_rays / surface_rays on the batch's rays give the batch's channels, and render_views' colours
    V.closure(g, got, bufs["rays"], SIZES, cams, label="%s cull %d" % (name, cull))
    # one tensor per channel for the whole batch
    n = 5
    got4 = V.batch_whole(g, cams[:n], 40, 24)
    V.compare(got4, V.loop(ra, path, cams[:n], [(40, 24)] * n, setup=setup), [(40, 24)] * n, U.CHANNELS, "%s cull %d (N, H, W, c)" % (name, cull))
    g.close()


# ---- 3. against the oracle, with a fov of the view's own --------------------------------------------------------------------------------
def rewritten(src, pos, rot, fov):
    lines = src.split("\n")
    i = lines.index("[options]")
    j = next(k for k in range(i + 1, len(lines)) if lines[k].startswith("["))      # (lights have a position= of their own)
    keep = [l for l in lines[i + 1:j] if not l.startswith(("position=", "rotation=", "fov="))]
    lines[i + 1:j] = keep + ["position=%r,%r,%r" % pos, "rotation=%r,%r,%r" % rot, "fov=%r" % fov]
    return "\n".join(lines)


def test_against_the_oracle_at_fovs_of_the_views_own(ra, oracle, tmp_path):
    name = "mixed_materials"
    src = open(os.path.join(ROOT, "scenes", name + ".scene")).read()
    views = [((0.3, 0.4, 1.0), (-8.0, 12.0, 3.0), 35.0, 41, 27), ((0.1, 0.5, 0.8), (-12.0, -6.0, 0.0), 90.0, 8, 200), ((-0.2, 0.6, 1.5), (-10.0, 4.0, -2.0), 117.5, 33, 17)]
    g = ra.Scene("scenes/%s.scene" % name, 32, 32)
    sizes = [(w, h) for _, _, _, w, h in views]
    got = V.batch(g, [(p, r, f) for p, r, f, _, _ in views], sizes)
    for k, (pos, rot, fov, w, h) in enumerate(views):
        p = tmp_path / ("v%d.scene" % k)
        p.write_text(rewritten(src, pos, rot, fov))
        exp = U.expected_of(str(p), w, h)
        mask = U.written_mask(w, h)
        assert exp["hit"][mask].any()
        bad = U.mismatches(got[k], exp, mask)
        assert not bad, "view %d (fov %g, %d x %d): pixels that differ from the oracle, per channel: %s" % (k, fov, w, h, bad)
        o = oracle.OracleScene(str(p), w, h)
        rays = U.primary_rays(o).reshape(h, w, 6)
        o.close()
        n = V.differing(got[k]["rays"], rays, mask)
        assert n == 0, "view %d (fov %g): %d rays differ from the oracle's primary rays" % (k, fov, n)
        for c in V.CHANNELS:
            assert V.touched(got[k][c], c, mask) == 0
    g.close()


# ---- 4. subsets ---------------------------------------------------------------------------------------------------------------------------
def test_subsets_give_the_same_bits(ra):
    g = ra.Scene("scenes/cfg4_textured_256.scene", 24, 16)
    cams = V.cams_of(g)
    full = V.batch(g, cams, SIZES)
    for names in [(c,) for c in V.CHANNELS] + [V.GEOMETRY, V.CHANNELS]:
        got = V.batch(g, cams, SIZES, names)
        for i, (w, h) in enumerate(SIZES):
            mask = U.written_mask(w, h)
            assert set(got[i]) == set(names)
            for c in names:
                assert V.differing(got[i][c], full[i][c], mask) == 0, "%s alone / in %s: view %d differs from the call with all eight" % (c, names, i)
                assert V.touched(got[i][c], c, mask) == 0
    g.close()


# ---- 5. many items ------------------------------------------------------------------------------------------------------------------------
def test_a_batch_of_many_times_the_waves(ra):
    """300 views of 72 x 56 = 18 900 items, several times the waves the device holds at once (tests/test_gpu_render_views.py's cameras)."""
    path = "scenes/cfg2_smooth_4k.scene"
    n, vw, vh = 300, 72, 56
    g = ra.Scene(path, 24, 16)
    base = g.camera_pose()
    cams = [(tuple(float(x) for x in base[0] + np.float32([0.002 * k, 0.001 * k, 0.0])), tuple(float(x) for x in base[1] + np.float32([0.0, 0.3 * k - 40.0, 0.0])))
            for k in range(n)]
    names = ("depth", "object_id", "rays")
    got = V.batch_whole(g, cams, vw, vh, names)
    want = V.loop(ra, path, cams, [(vw, vh)] * n, ("depth", "object_id"))
    V.compare(got, want, [(vw, vh)] * n, ("depth", "object_id"), "300 views")
    org = np.stack([np.asarray(g.view_target(p, r, None, vw, vh).cam_pos[:], np.float32) for p, r in cams])
    rays = np.stack([v["rays"] for v in got])
    assert np.array_equal(U.bits(rays[:, :vh - 1, :vw - 1, :3]), U.bits(np.broadcast_to(org[:, None, None, :], (n, vh - 1, vw - 1, 3))))
    g.close()


def test_a_long_irregular_batch_closes_on_trace_rays(ra):
    """700 views of seeded random sizes in 1 .. 69: the item-to-view search runs over a long, irregular prefix array.  Checked by the
    closure on trace_rays -- one call over the rays of all views -- instead of 700 one-view calls."""
    g = ra.Scene("scenes/cfg2_smooth_4k.scene", 24, 16)
    rng = np.random.default_rng(7)
    sizes = [(int(w), int(h)) for w, h in rng.integers(1, 70, size=(700, 2))]
    base = g.camera_pose()
    cams = [(tuple(float(x) for x in base[0] + np.float32([0.001 * k, 0.0, 0.0005 * k])), tuple(float(x) for x in base[1] + np.float32([0.02 * (k % 50) - 5.0, 0.1 * k - 35.0, 0.0])))
            for k in range(len(sizes))]
    px = np.cumsum([0] + [w * h for w, h in sizes])
    flat = {c: V.new((int(px[-1]),), c) for c in V.GEOMETRY}
    views = {c: [flat[c][int(px[i]):int(px[i + 1])].view((h, w) + V.TAIL[c]) for i, (w, h) in enumerate(sizes)] for c in V.GEOMETRY}
    g.render_views_aov(cams, **views)
    hits, _ = g.trace_rays(flat["rays"], hits=True, colours=False)      # (an unwritten ray is the sentinel's, and is not looked at)
    torch.cuda.synchronize()
    hits = hits.cpu().numpy()
    host = {c: flat[c].cpu().numpy() for c in V.GEOMETRY}
    written = np.concatenate([U.written_mask(w, h).ravel() for w, h in sizes])
    assert written.sum() > 500000
    want = dict(depth=hits[:, 3], object_id=hits[:, 1].astype(np.int32), triangle_id=hits[:, 2].astype(np.int32), uv=np.ascontiguousarray(hits[:, 4:6]))
    for c, wv in want.items():
        d = U.bits(host[c]) != U.bits(wv)
        d = d.any(-1) if d.ndim == 2 else d
        assert not d[written].any(), "%s: %d pixels differ from trace_rays on the batch's rays" % (c, int(d[written].sum()))
    assert (want["object_id"][written] >= 0).sum() > 10000
    for c in V.GEOMETRY:
        keep = host[c] == V.fill_of(c)
        keep = keep.all(-1) if keep.ndim == 2 else keep
        assert keep[~written].all(), "%s: %d pixels outside the written ones were touched" % (c, int((~keep[~written]).sum()))
    # the origin of every written ray is its view's camera
    view_of = np.repeat(np.arange(len(sizes)), np.diff(px))
    org = np.stack([np.asarray(g.view_target(p, r, None, w, h).cam_pos[:], np.float32) for (p, r), (w, h) in zip(cams, sizes)])
    assert np.array_equal(U.bits(host["rays"][written, :3]), U.bits(org[view_of[written]]))
    g.close()


# ---- 6. guards ------------------------------------------------------------------------------------------------------------------------------
def test_unwritten_bytes_keep_their_sentinel(ra):
    """All channels of all views in slices of ONE tensor with guard runs of an odd length between them, everything filled with a sentinel."""
    g = ra.Scene("scenes/mixed_materials.scene", 24, 16)
    guard = 97
    width = {c: int(np.prod(V.TAIL[c], dtype=np.int64)) for c in V.CHANNELS}
    total = sum(w * h * width[c] + guard for w, h in SIZES for c in V.CHANNELS) + guard
    big = torch.full((total,), V.FILL_F, dtype=torch.float32, device="cuda")
    sent = np.float32(V.FILL_F).view(np.uint32)
    views, spans, at = {c: [] for c in V.CHANNELS}, [], guard
    for w, h in SIZES:
        for c in V.CHANNELS:
            n = w * h * width[c]
            s = big[at:at + n]
            views[c].append((s.view(torch.int32) if V.integer(c) else s).view((h, w) + V.TAIL[c]))
            spans.append((at, n, w, h, c))
            at += n + guard
    cams = V.cams_of(g)
    g.render_views_aov(cams, **views)
    torch.cuda.synchronize()
    got = big.cpu().numpy().view(np.uint32)
    inside = np.zeros(total, bool)
    for a, n, w, h, c in spans:
        inside[a:a + n] = True
        v = got[a:a + n].reshape(h, w, width[c])
        mask = U.written_mask(w, h)
        assert (v[~mask] == sent).all(), "%s of a %d x %d view: a pixel outside the written ones was touched" % (c, w, h)
        if c in ("depth", "rays"):      # (no depth and no direction is the sentinel: every written pixel shows)
            assert (v[mask] != sent).any(-1).all(), "%s of a %d x %d view: a pixel was not written" % (c, w, h)
    assert (got[~inside] == sent).all(), "%d words outside the views' buffers were written" % int((got[~inside] != sent).sum())
    g.close()


# ---- 7. the scene is left as it was -----------------------------------------------------------------------------------------------------------
def test_the_scene_is_left_as_it_was(ra):
    w, h = 160, 120
    g = ra.Scene("scenes/cfg2_smooth_4k.scene", w, h)
    g.set_frame_mode(0)
    fb = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda"); mask = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
    for _ in range(2):
        fb.zero_()
        g.render_frame(fb, mask)
    torch.cuda.synchronize()
    before = (fb.cpu().numpy(), mask.cpu().numpy())
    cost, mode, ms = g.tile_cost(), g.frame_mode(), g.last_kernel_ms(0)
    cam = g.camera()
    cams = [(p, r) for p, r in POSES[:6]]
    bufs = {c: [V.new((vh, vw), c) for vw, vh in SIZES[:6]] for c in V.CHANNELS}
    g.render_views_aov(cams, **bufs)
    torch.cuda.synchronize()
    live = ra.live_device_memory()
    g.render_views_aov(cams, **bufs)
    torch.cuda.synchronize()
    assert ra.live_device_memory() == live, "a second call with the same batch allocated"
    assert np.array_equal(g.tile_cost(), cost) and g.frame_mode() == mode and g.last_kernel_ms(0) == ms
    assert all(np.array_equal(a, b) for a, b in zip(cam, g.camera())) and (g.width, g.height) == (w, h)
    fb.zero_(); mask.zero_()
    g.render_frame(fb, mask)
    torch.cuda.synchronize()
    assert g.frame_status() == 0
    assert np.array_equal(U.bits(fb.cpu().numpy()), U.bits(before[0])) and np.array_equal(mask.cpu().numpy(), before[1])
    g.close()


# ---- 8. after edits -------------------------------------------------------------------------------------------------------------------------
def test_edited_scene_equals_the_loop_on_a_scene_with_the_same_edits(ra):
    path = "scenes/mixed_materials.scene"
    g = ra.Scene(path, 24, 16)
    cams, sizes = V.cams_of(g)[2:9], SIZES[2:9]
    first = V.batch(g, cams, sizes)
    move = dict(rot=(-40, 10, 70), pos=(-0.9, 0.2, -4.4))      # (object 1: a mesh)

    def edits(f):
        f.gpu()
        f.move_object(1, **move)
        f.set_light(0, intensity=0.5)

    edits(g)
    got = V.batch(g, cams, sizes)
    want = V.loop(ra, path, cams, sizes, setup=edits)
    V.compare(got, want, sizes, U.CHANNELS, "after move_object and set_light")
    assert any(V.differing(a["depth"], b["depth"], U.written_mask(w, h)) for a, b, (w, h) in zip(first, got, sizes)), "the move changed no depth"
    # the culling flag of the current view is the batch's
    flip = 0 if g.kernel_variant()["cull"] else 1

    def flipped(f):
        edits(f)
        f.set_flag("useBackfaceCulling", flip)

    g.set_flag("useBackfaceCulling", flip)
    got2 = V.batch(g, cams, sizes)
    assert g.kernel_variant()["cull"] == bool(flip)
    V.compare(got2, V.loop(ra, path, cams, sizes, setup=flipped), sizes, U.CHANNELS, "culling flipped")
    g.close()


# ---- 9. refusals on a live scene ------------------------------------------------------------------------------------------------------------
def test_refusals_on_a_live_scene(ra):
    rtx, _ = ra.load()
    g = ra.Scene("scenes/cfg2_smooth_4k.scene", 24, 16)
    cams, sizes = [POSES[1], POSES[2]], [(24, 16), (9, 9)]
    want = V.batch(g, cams, sizes)

    def sentinel(bufs):
        torch.cuda.synchronize()
        return all((t == (V.FILL_I if V.integer(c) else V.FILL_F)).all().item() for c, ts in bufs.items() for t in ts)

    def refused(code, what):
        bufs = {c: [V.new((h, w), c) for w, h in sizes] for c in V.CHANNELS}
        with pytest.raises(ra.RtxError, match=what) as e:
            g.render_views_aov(cams, **bufs)
        assert "(%d)" % code in str(e.value)
        assert sentinel(bufs), "a refused call touched a buffer"

    g.counters_enable(True)
    refused(-4, "rtx_render_views_aov collects no statistics")
    g.counters_enable(False)
    g.set_row_ownership(8, 2, 1)
    refused(-1, "rtx_render_views_aov: the rows are shared among devices.*deal out views")
    g.set_row_ownership(0, 1, 0)
    # RTX_FLAG_SHOW_NORMALS changes no channel
    g.set_flag("showNormals", 1)
    shown = V.batch(g, cams, sizes)
    g.set_flag("showNormals", 0)
    for i, (w, h) in enumerate(sizes):
        for c in V.CHANNELS:
            assert V.differing(shown[i][c], want[i][c], np.ones((h, w), bool)) == 0, "showNormals changed %s" % c
    # the C entry's own argument checks, on the live scene
    bufs = {c: [V.new((h, w), c) for w, h in sizes] for c in V.CHANNELS}
    fields = [f for f, _ in ra.ViewAovTarget._fields_[6:]]
    t = (ra.ViewAovTarget * 2)()
    for i, (cam, (w, h)) in enumerate(zip(cams, sizes)):
        g._fill_view_target(t[i], cam[0], cam[1], None, w, h)
        for f, c in zip(fields, V.CHANNELS):
            setattr(t[i], f, bufs[c][i].data_ptr())
    sp = g.gpu()
    err = lambda: rtx.rtx_last_error()
    assert rtx.rtx_render_views_aov(sp, 2, None, None) == -1 and b"rtx_render_views_aov: views is NULL" in err()
    assert rtx.rtx_render_views_aov(sp, 0, None, None) == 0
    t[1].width = 0
    assert rtx.rtx_render_views_aov(sp, 2, t, None) == -1 and b"rtx_render_views_aov: view 1 has a zero width or height" in err()
    t[1].width = 9; t[1].height = 0
    assert rtx.rtx_render_views_aov(sp, 2, t, None) == -1 and b"rtx_render_views_aov: view 1 has a zero width or height" in err()
    t[1].height = 40000
    assert rtx.rtx_render_views_aov(sp, 2, t, None) == -1 and b"rtx_render_views_aov: view 1 is larger than RTX_VIEWS_MAX_SIDE" in err()
    t[1].height = 9
    many = (ra.ViewAovTarget * 65537)(*([t[0]] * 65537))
    assert rtx.rtx_render_views_aov(sp, 65537, many, None) == -1 and b"rtx_render_views_aov: more than RTX_VIEWS_MAX_VIEWS" in err()
    big = (ra.ViewAovTarget * 5)(*([t[0]] * 5))
    for k in range(4):
        big[k].width = big[k].height = 8192
    assert rtx.rtx_render_views_aov(sp, 5, big, None) == -1 and b"rtx_render_views_aov: more than RTX_VIEWS_MAX_TILES" in err()
    # a channel in some views and not in others, either way round; no channel at all
    keep = t[1].uv_dev
    t[1].uv_dev = None
    assert rtx.rtx_render_views_aov(sp, 2, t, None) == -1 and b"view 1 has no uv_dev but view 0 has one" in err()
    t[1].uv_dev = keep
    keep = t[0].rays_dev
    t[0].rays_dev = None
    assert rtx.rtx_render_views_aov(sp, 2, t, None) == -1 and b"view 1 has a rays_dev but view 0 has none" in err()
    t[0].rays_dev = keep
    none = (ra.ViewAovTarget * 2)()
    for i, (cam, (w, h)) in enumerate(zip(cams, sizes)):
        g._fill_view_target(none[i], cam[0], cam[1], None, w, h)
    assert rtx.rtx_render_views_aov(sp, 2, none, None) == -1 and b"rtx_render_views_aov: no output" in err()
    assert sentinel(bufs), "a refused call touched a buffer"
    # ... and the scene still renders a batch
    assert rtx.rtx_render_views_aov(sp, 2, t, None) == 0
    torch.cuda.synchronize()
    for i, (w, h) in enumerate(sizes):
        for c in V.CHANNELS:
            assert V.differing(bufs[c][i].cpu().numpy(), want[i][c], np.ones((h, w), bool)) == 0
    g.close()
