"""rtx_render_light / Scene.render_light: the direct light of a frame in one launch (include/rtx_render_light.h).  Every comparison is bit
for bit over every written pixel, in buffers that are pre-filled and sit between guard areas:
  the stated identity -- all five outputs equal Scene.light_rays(primary rays, per_light=True) transposed to planes, and on two scenes the
      numpy restatement of the contract (tests/util_light.py) with the exact N and depth from render_aov;
  composition -- render_pass1's colour at Diffuse and Phong first hits is made of the two sums, render_aov's albedo and the object's constants;
  each output alone and every combination of wantD / wantS / wantOpen; lights of every kind and edited lights; rows and row ownership;
  edited scenes; the ordinary frame is not disturbed; streams, flags, refusals."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import util_ao as AO
from tests import util_aov as U
from tests import util_light as UL
from tests import util_lights as LE
from tests import util_render_light as RL
from tests.ac_heatmap import scene_copy
from tests.util_move import edit_scene
from tests.util_objects import apply_step, write_scene

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = U.ROOT
f32 = np.float32
CH, SUMS, PER_LIGHT, GUARD, FILL = RL.CHANNELS, RL.SUMS, RL.PER_LIGHT, RL.GUARD, RL.FILL
differ, touched = RL.differ, RL.touched


def dev(a, dtype=f32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def text_of(name):
    return open(os.path.join(ROOT, "scenes", name + ".scene")).read()


class Buffers:
    """`names` of a w x h frame of L lights, each in the middle of a larger pre-filled allocation."""

    def __init__(self, w, h, L, names=CH):
        self.names = tuple(names)
        self.flat, self.view = {}, {}
        for c in self.names:
            shape = RL.shape_of(c, L, w, h)
            n = int(np.prod(shape, dtype=np.int64))
            self.flat[c] = torch.full((n + 2 * GUARD,), FILL[c], dtype=torch.int32 if c == "light_open" else torch.float32, device="cuda")
            self.view[c] = self.flat[c][GUARD:GUARD + n].view(shape)
            assert self.view[c].is_contiguous()

    def struct(self, ra, names, n_lights):
        ptr = lambda c: self.flat[c].data_ptr() + 4 * GUARD
        return ra.FrameLightBuffers(n_lights, *[ptr(c) if c in names else None for c in CH])

    def read(self):
        """name -> numpy array of the channel's shape, after checking the guards"""
        torch.cuda.synchronize()
        out = {}
        for c in self.names:
            f = self.flat[c].cpu().numpy()
            fill = f.dtype.type(FILL[c])
            assert (f[:GUARD] == fill).all() and (f[-GUARD:] == fill).all(), "%s: written outside the buffer" % c
            out[c] = f[GUARD:len(f) - GUARD].reshape(tuple(self.view[c].shape))
        return out


def render(g, names=CH, rows=None, stream=None):
    b = Buffers(g.width, g.height, g.n_lights, names)
    g.render_light(rows=rows, stream=stream, **b.view)
    return b.read()


def call(ra, g, b, names, n_lights=None, rows=None):
    """the C entry, directly"""
    rtx, _ = ra.load()
    s = b.struct(ra, names, g.n_lights if n_lights is None else n_lights)
    r0, r1 = rows if rows is not None else (0, g.height)
    return rtx.rtx_render_light(g.gpu(), r0, r1, C.byref(s), C.c_void_p(torch.cuda.current_stream().cuda_stream))


def by_light_rays(g, hits=False):
    """The expectation: Scene.light_rays of the frame's primary rays, as planes; with hits also the rays' hit mask (h, w)."""
    rays = U.primary_rays(g)
    out = g.light_rays(dev(rays), hits=True, per_light=True)
    torch.cuda.synchronize()
    out = {c: t.cpu().numpy() for c, t in out.items()}
    want = RL.planes(out, g.width, g.height)
    return (want, (out["hits"][:, 0] > 0).reshape(g.height, g.width)) if hits else want


def check_frame(g, what, names=CH):
    """g's frame equals light_rays of its primary rays on the written pixels and is untouched elsewhere; returns (got, hit mask)."""
    w, h = g.width, g.height
    mask = U.written_mask(w, h)
    got = render(g, names)
    want, hit = by_light_rays(g, hits=True)
    bad = differ(got, want, mask, names)
    assert not bad, "%s: entries that differ from light_rays of the primary rays: %s" % (what, bad)
    assert not touched(got, mask), "%s: written outside the pixels of pass 1" % what
    return got, hit


# ---- 1. the stated identity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cull", [1, 0])
@pytest.mark.parametrize("w,h", RL.SIZES)
@pytest.mark.parametrize("name", RL.SCENES)
def test_frame_equals_light_rays_of_the_primary_rays(ra, name, w, h, cull):
    g = ra.Scene("scenes/%s.scene" % name, w, h)
    g.set_flag("useBackfaceCulling", cull)
    got, hit = check_frame(g, "%s %dx%d cull %d" % (name, w, h, cull))
    mask = U.written_mask(w, h)
    miss = mask & ~hit
    # (with culling on every frame but mixed_materials', whose floor fills the view, has misses: tests/test_render_light_cpu.py)
    assert (mask & hit).any() and (miss.any() or name == "mixed_materials" or not cull)
    # a miss writes zeros, and light_open = 0
    for c in SUMS:
        assert not U.bits(got[c])[miss].any(), c
    for c in PER_LIGHT:
        assert not U.bits(got[c])[:, miss].any(), c
    # the sums are the in-order sums of the planes
    for s, p in (("diffuse", "light_diffuse"), ("specular", "light_specular")):
        per = got[p][:, mask].transpose(1, 0, 2)
        assert np.array_equal(U.bits(UL.in_order_sum(per)), U.bits(got[s][mask])), s
    g.close()


@pytest.mark.parametrize("name,w,h", [("cfg1_simple_shapes", 33, 17), ("area_light", 36, 48)])
def test_frame_equals_the_restated_contract(ra, oracle, name, w, h):
    """tests/util_light's numpy restatement with P and N from render_aov, illuminate from the oracle and visibility from Scene.occluded"""
    path = "scenes/%s.scene" % name
    g = ra.Scene(path, w, h)
    got = render(g)
    rays, depth, normal, hit = AO.first_hits(g)
    obj = torch.full((h, w), -1, dtype=torch.int32, device="cuda")
    g.render_aov(object_id=obj)
    torch.cuda.synchronize()
    obj = obj.cpu().numpy().reshape(-1)
    hits = np.zeros((len(rays), 8), f32)
    hits[:, 0] = hit; hits[:, 1] = obj; hits[:, 3] = depth
    o = oracle.OracleScene(path, w, h)
    plan = UL.Plan(o, g.device_lights(), rays, hits, normal, bias=AO.BIAS)
    o.close()
    occ = g.occluded(dev(plan.shadow_rays), dev(plan.shadow_tmax))
    torch.cuda.synchronize()
    objs, _ = g.device_objects()
    ns = np.where(obj >= 0, objs["n_specular"][np.maximum(obj, 0)], f32(0)).astype(f32)
    want = RL.planes(plan.reduce(occ.cpu().numpy(), ns), w, h)
    mask = U.written_mask(w, h)
    bad = differ(got, want, mask)
    assert not bad, "%s %dx%d: entries that differ from the restated contract: %s" % (name, w, h, bad)
    assert (got["light_open"][:, mask] > 0).any() and (got["light_open"][:, mask & hit.reshape(h, w)] == 0).any()
    g.close()


# ---- 2. composition ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,w,h", [("cfg1_simple_shapes", 48, 32), ("area_light", 36, 48), ("mixed_materials", 33, 17), ("cfg4_textured_256", 48, 32)])
def test_the_sums_compose_pass_1_at_diffuse_and_phong_hits(ra, name, w, h):
    g = ra.Scene("scenes/%s.scene" % name, w, h)
    got = render(g, SUMS)
    fb = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
    albedo = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
    obj = torch.full((h, w), -1, dtype=torch.int32, device="cuda")
    g.render_pass1(fb)
    g.render_aov(albedo=albedo, object_id=obj)
    ks = g.surface_rays(dev(U.primary_rays(g)), hits=False, position=False, normal=False, albedo=False, specular=True)["specular"]
    torch.cuda.synchronize()
    mask = U.written_mask(w, h).reshape(-1)
    obj = obj.cpu().numpy().reshape(-1)
    objs, _ = g.device_objects()
    rec = objs[np.maximum(obj, 0)]
    material = np.where((obj >= 0) & mask, rec["material"], -1)
    colour = fb.cpu().numpy().reshape(-1, 3)
    is_dp, want = UL.colour_identities(colour, albedo.cpu().numpy().reshape(-1, 3), ks.cpu().numpy().reshape(-1), got["diffuse"].reshape(-1, 3),
                                       got["specular"].reshape(-1, 3), material, rec["ambient"], rec["diffuse"])
    bad = is_dp & (U.bits(want) != U.bits(colour)).any(-1)
    print("%s %dx%d: %d Diffuse and %d Phong first hits, %d differ" % (name, w, h, (material == 0).sum(), (material == 3).sum(), bad.sum()))
    assert is_dp.sum() >= 50 and ((material == 3).sum() >= 20 or name in ("cfg4_textured_256", "mixed_materials"))
    assert not bad.any(), "%s: %d of %d Diffuse / Phong pixels whose sums do not make pass 1's colour" % (name, bad.sum(), is_dp.sum())
    g.close()


# ---- 3. each output alone; wantD / wantS / wantOpen ---------------------------------------------------------------------------------------
SUBSETS = [(c,) for c in CH] + [SUMS, ("diffuse", "light_open"), ("light_specular", "light_open"), ("light_diffuse", "specular"),
                                ("light_diffuse", "light_specular")]


@pytest.mark.parametrize("name,w,h,rows", [("area_light", 33, 17, (3, 13)), ("cfg1_simple_shapes", 36, 48, None), ("cfg2_smooth_4k", 33, 17, (8, 100))])
def test_only_what_was_asked_for_is_written(ra, name, w, h, rows):
    g = ra.Scene("scenes/%s.scene" % name, w, h)
    full = render(g)
    whole = U.written_mask(w, h)
    assert not touched(full, whole)
    mask = U.written_mask(w, h, rows)
    for names in SUBSETS:
        # through the C entry, with every other pointer NULL; the buffers of the channels not asked for stay as they were
        b = Buffers(w, h, g.n_lights)
        assert call(ra, g, b, names, rows=rows) == 0
        got = b.read()
        assert not touched(got, mask), "%s: written outside rows %s" % (names, rows)
        assert not differ(got, full, mask, names), "%s differs from the five-output call" % (names,)
        assert not touched({c: got[c] for c in CH if c not in names}, np.zeros((h, w), bool)), "a call for %s wrote another buffer" % (names,)
        # ... and through the wrapper
        assert not differ(render(g, names, rows), full, mask, names)
    g.close()


# ---- 4. lights --------------------------------------------------------------------------------------------------------------------------
def without_lights(text):
    for k in range(LE.n_lights(text) - 1, -1, -1):
        text = LE.remove_light(text, k)
    return text


def test_a_scene_without_lights(ra, tmp_path):
    w, h = 33, 17
    path = LE.write_scene(tmp_path, without_lights(text_of("cfg1_simple_shapes")), "dark")
    g = ra.Scene(path, w, h)
    assert g.n_lights == 0
    mask = U.written_mask(w, h)
    got = render(g)                       # (the per-light tensors are empty: the library takes no pointer for them)
    assert got["light_open"].shape == (0, h, w)
    for c in SUMS:
        assert not U.bits(got[c])[mask].any(), "%s is not +0 at every written pixel" % c
    assert not touched(got, mask)
    # per-light pointers on a scene without lights are refused, whatever n_lights says
    b = Buffers(w, h, 1)
    for nl in (0, 1):
        assert call(ra, g, b, CH, n_lights=nl) == -1
        assert call(ra, g, b, ("light_open",), n_lights=nl) == -1
    assert not touched(b.read(), np.zeros((h, w), bool))
    with pytest.raises(ra.RtxError):
        g.render_light(light_open=torch.zeros((0, h, w), dtype=torch.int32, device="cuda"))
    # ... and the lights of the live scene removed one by one end in the same state
    live = ra.Scene("scenes/cfg1_simple_shapes.scene", w, h)
    render(live)
    while live.n_lights:
        live.remove_light(0)
    assert not differ(render(live), got, mask)
    live.close(); g.close()


def test_one_distant_light(ra, tmp_path):
    w, h = 36, 48
    text = LE.add_light(without_lights(text_of("cfg2_smooth_4k")), "distant", direction=(0.3, -1.0, -0.2), color=(0.8, 0.8, 0.7), intensity=0.6)
    g = ra.Scene(LE.write_scene(tmp_path, text, "distant"), w, h)
    assert g.n_lights == 1
    got, hit = check_frame(g, "one distant light")
    col = got["light_open"][0][U.written_mask(w, h) & hit]
    assert col.any() and not col.all()
    g.close()


def test_seven_point_lights(ra, tmp_path):
    """more point lights than have a source copy of the prune records (six): lights 6 and up walk with the general class"""
    w, h = 48, 32
    text = without_lights(text_of("cfg2_smooth_4k"))
    spots = [(0, 2, -1), (1, -1, -1), (-1, -1, -1), (2.5, 1.5, -3), (-2.5, 1.0, -2), (0.3, 3.0, -4.5), (-0.8, 0.5, -0.5)]
    for k, pos in enumerate(spots):
        text = LE.add_light(text, "point", position=pos, color=(0.9 - 0.1 * k, 0.3 + 0.1 * k, 0.5), intensity=0.4 + 0.2 * k)
    g = ra.Scene(LE.write_scene(tmp_path, text, "seven"), w, h)
    assert g.n_lights == 7
    got, hit = check_frame(g, "seven point lights")
    for li in range(7):
        col = got["light_open"][li][U.written_mask(w, h) & hit]
        assert col.any() and not col.all(), "light %d is open for every hit or for none" % li
    g.close()


@pytest.mark.parametrize("samples", [1, 3])
def test_area_light_samples(ra, tmp_path, samples):
    w, h = 36, 48
    text = LE.set_light(text_of("area_light"), 0, samples=samples)
    g = ra.Scene(LE.write_scene(tmp_path, text, "samples%d" % samples), w, h)
    recs, _ = g.device_lights()
    assert list(recs["n_points"]) == [samples * samples, 1, 0]
    got, hit = check_frame(g, "samples = %d" % samples)
    mine = got["light_open"][0][U.written_mask(w, h) & hit]
    assert mine.max() == samples * samples
    if samples > 1:
        assert ((mine > 0) & (mine < samples * samples)).sum() >= 10, "no pixel sees the area light partly"
    g.close()


def test_edited_lights_equal_a_fresh_scene(ra, tmp_path):
    name, w, h = "area_light", 33, 17
    text = text_of(name)
    g = ra.Scene("scenes/%s.scene" % name, w, h)
    mask = U.written_mask(w, h)
    none = np.zeros((h, w), bool)
    render(g)
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
            b = Buffers(w, h, before)
            assert call(ra, g, b, CH, n_lights=before) == -1
            rtx, _ = ra.load()
            assert b"n_lights" in rtx.rtx_last_error()
            assert not touched(b.read(), none)
            assert call(ra, g, b, SUMS, n_lights=before) == 0
            assert not touched(b.read(), mask)
            with pytest.raises(ValueError, match="light_open must have shape"):
                g.render_light(light_open=b.view["light_open"])
        got, _ = check_frame(g, "step %d %s" % (k, step[0]))
        f = ra.Scene(LE.write_scene(tmp_path, text, "step%d" % k), w, h)
        assert not differ(got, render(f), mask), "step %d %s: differs from a fresh scene" % (k, step[0])
        f.close()
    g.close()


# ---- 5. rows and ownership --------------------------------------------------------------------------------------------------------------
def test_row_ranges(ra):
    name, w, h = "mixed_materials", 36, 48
    g = ra.Scene("scenes/%s.scene" % name, w, h)
    full = render(g)
    for rows in ((0, h), (5, 6), (7, 29), (h - 3, h + 100), (40, 0xFFFFFFFF)):
        mask = U.written_mask(w, h, (rows[0], min(rows[1], h)))
        got = render(g, rows=rows)
        assert mask.any() and not touched(got, mask) and not differ(got, full, mask), rows
    for empty in ((5, 5), (7, 2), (h - 1, h), (h, h + 8), (0, 0)):
        assert not touched(render(g, rows=empty), np.zeros((h, w), bool)), empty
    g.close()


@pytest.mark.parametrize("halo", [True, False])
def test_row_ownership(ra, halo):
    name, w, h = "cfg2_smooth_4k", 33, 41
    g = ra.Scene("scenes/%s.scene" % name, w, h)
    full = render(g)
    union = render(g, rows=(0, 0))            # (all pattern)
    seen = np.zeros((h, w), int)
    for part in range(3):
        g.set_row_ownership(8, 3, part, halo)
        got = render(g)
        mask = U.written_mask(w, h, band=8, parts=3, part=part)
        assert mask.any()
        assert not touched(got, mask), "part %d wrote rows it does not own" % part
        assert not differ(got, full, mask)
        seen += mask
        for c in CH:
            RL.pixels(c, union[c])[:, mask] = RL.pixels(c, got[c])[:, mask]
    g.set_row_ownership(0, 1, 0)
    whole = U.written_mask(w, h)
    assert np.array_equal(seen > 0, whole) and seen.max() == 1             # (the parts' pixels are disjoint and their union is the frame)
    assert not differ(union, full, whole) and not touched(union, whole)
    g.close()


# ---- 6. state around a call -------------------------------------------------------------------------------------------------------------
def test_edited_scene_equals_a_fresh_one(ra, tmp_path):
    name = "mixed_materials"
    w, h = 36, 48
    text = text_of(name)
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
        f = ra.Scene(write_scene(tmp_path, text, "light_%d" % k), w, h)
        got, _ = check_frame(g, "step %d %s" % (k, step[0]))
        assert not differ(got, render(f), U.written_mask(w, h)), "step %d %s: differs from a fresh scene" % (k, step[0])
        f.close()
    g.close()


def test_after_set_vertices(ra, tmp_path):
    from tests.util_deform import bulge, deformed_scene, twist
    name, w, h, idx = "mixed_materials", 36, 48, 1
    g = ra.Scene("scenes/%s.scene" % name, w, h)
    before = render(g)
    P0, _ = g.mesh_vertices(idx)
    V = bulge(twist(P0, 0.7), 0.1, 2.0)
    g.set_vertices(idx, torch.from_numpy(V).cuda())
    f, _ = deformed_scene(ra, tmp_path, text_of(name), idx, V, None, "render_light", w, h)
    mask = U.written_mask(w, h)
    got, _ = check_frame(g, "after set_vertices")
    assert not differ(got, render(f), mask), "differs from a fresh scene of the deformed mesh"
    assert differ(got, before, mask), "the deformation changes nothing in the frame"
    f.close(); g.close()


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
    assert not differ(got, by_light_rays(g), U.written_mask(w, h))
    g.close()


# ---- 7. streams and flags ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("as_current", [False, True])
def test_another_stream_gives_the_same_bits(ra, as_current):
    name, w, h = "cfg2_smooth_4k", 48, 32
    g = ra.Scene("scenes/%s.scene" % name, w, h)
    mask = U.written_mask(w, h)
    want = render(g)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    for _ in range(3):
        with torch.cuda.stream(st):
            b = Buffers(w, h, g.n_lights)         # (filled on st: a call that did not wait for the fill would be overwritten by it)
            if as_current:
                g.render_light(**b.view)
            else:
                g.render_light(stream=st, **b.view)
        st.synchronize()
        got = b.read()
        assert not differ(got, want, mask) and not touched(got, mask)
    g.close()


def test_flags_and_ray_depth_change_nothing(ra, tmp_path):
    name, w, h = "cfg3_reflective_refractive", 36, 48
    g = ra.Scene("scenes/%s.scene" % name, w, h)
    full = render(g)
    mask = U.written_mask(w, h)
    for flag in ("showNormals", "useSkybox"):
        g.set_flag(flag, 1)
        assert not differ(render(g), full, mask), flag
        g.set_flag(flag, 0)
    g.close()
    for depth in (0, -1):
        f = ra.Scene(scene_copy(name, str(tmp_path), dict(max_ray_depth=depth)), w, h)
        assert not differ(render(f), full, mask), "max_ray_depth = %d" % depth
        f.close()


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_buffers_untouched(ra):
    w, h = 33, 17
    g = ra.Scene("scenes/cfg1_simple_shapes.scene", w, h)
    rtx, _ = ra.load()
    L = g.n_lights
    b = Buffers(w, h, L)
    none = np.zeros((h, w), bool)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    s = b.struct(ra, CH, L)
    # counters enabled: RTX_ERR_UNSUPPORTED
    g.counters_enable(True)
    with pytest.raises(ra.RtxError):
        g.render_light(**b.view)
    assert rtx.rtx_render_light(g.gpu(), 0, h, C.byref(s), st) == -4
    g.counters_enable(False)
    assert not touched(b.read(), none)
    # RTX_ERR_ARG: a NULL scene, a NULL struct, the all-NULL struct, another number of lights for every per-light pointer
    assert rtx.rtx_render_light(None, 0, h, C.byref(s), st) == -1
    assert rtx.rtx_render_light(g.gpu(), 0, h, None, st) == -1
    assert b"NULL" in rtx.rtx_last_error()
    assert call(ra, g, b, ()) == -1
    assert b"NULL" in rtx.rtx_last_error()
    for names in (CH,) + tuple((c,) for c in PER_LIGHT):
        for nl in (L + 1, L - 1, 0):
            assert call(ra, g, b, names, n_lights=nl) == -1, (names, nl)
            assert b"n_lights" in rtx.rtx_last_error()
    assert not touched(b.read(), none)
    with pytest.raises(ValueError, match="render_light: nothing to compute"):
        g.render_light()
    with pytest.raises(ValueError, match="diffuse must be on cuda:0"):
        g.render_light(diffuse=torch.zeros((h, w, 3)))
    # ... and the call works afterwards; the sums ignore n_lights
    assert call(ra, g, b, SUMS, n_lights=99) == 0
    got = b.read()
    mask = U.written_mask(w, h)
    assert not differ(got, by_light_rays(g), mask, SUMS) and not touched(got, mask)
    assert not touched({c: got[c] for c in PER_LIGHT}, none)
    g.close()
