"""rtx_project_points / Scene.camera_table, project_points, bake_view (include/rtx_project.h): surface points projected into cameras, with
visibility.  Every comparison is bit for bit over every (camera, point) pair:
  1. pixel, depth and the geometric flags are tests/util_project's restatement (pinned to the oracle by tests/test_project_cpu.py), and OPEN
     is Scene.occluded({O, -L}, dist) == 0 on exactly the pairs FRONT && INSIDE && dist == dist, under both culling flags;
  2. the round trip on the device: the hit points of a camera project into the pixels they were seen through, and into the objects
     another camera sees at the pixels where they are OPEN;
  3. across batches, orders and tables;  4. only what is asked for is written;  5. scene edits, flags, counters, streams, refusals;
  6. camera_table is view_target;  7. bake_view."""
import ctypes as C

import numpy as np
import pytest

from tests import util_aov as U
from tests import util_project as UPJ
from tests import util_texel_points as UT
from tests.ac_heatmap import scene_copy
from tests.test_gpu_points import free_points, surface

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

f32 = np.float32
GUARD = 96                    # untouched elements before and after every buffer
FILL = 7.25
W, H = 48, 32
SCENES = ["cfg1_simple_shapes", "cfg2_smooth_4k", "mixed_materials", "area_light"]
CH = UPJ.CHANNELS


def dev(a, dtype=f32):
    return torch.from_numpy(np.array(a, dtype, order="C")).cuda()      # (a copy: the shared cases are read-only)


def host(out):
    torch.cuda.synchronize()
    return {c: t.cpu().numpy() for c, t in out.items()}


def own_camera(g):
    pos, rot = g.camera_pose()
    return (tuple(float(x) for x in pos), tuple(float(x) for x in rot))


def cameras_of(ra, g, centre):
    """The camera sequences of a scene: its own, the second camera, the six of a cube at `centre` -- at the scene's size -- and one with
    another fov at a non-square size of its own; and their table (K, 24) as numpy"""
    cams = [own_camera(g), UPJ.SECOND_CAMERA] + ra.cube_cameras(centre)
    table = np.concatenate([g._camera_records(cams), g._camera_records([UPJ.WIDE_CAMERA], *UPJ.WIDE_SIZE)])
    return cams, np.ascontiguousarray(table, f32)


def project(g, points, table, **kw):
    kw.setdefault("depth", True)
    return host(g.project_points(dev(points), table if isinstance(table, list) else dev(table), **kw))


def occluded(g, plan):
    if not len(plan.shadow_rays):
        return np.zeros(0, np.uint8)
    occ = g.occluded(dev(plan.shadow_rays), dev(plan.shadow_tmax))
    torch.cuda.synchronize()
    return occ.cpu().numpy()


_case = {}


def case(ra, name):
    """The points, cameras and restated channels of a scene, computed once and shared read-only: the first hits of the camera rays with
    their shading normals, 4096 free points with normals of every kind, and the special points of every camera (behind it, at its
    position, with sz == 0)"""
    if name not in _case:
        path = "scenes/%s.scene" % name
        g = ra.Scene(path, W, H)
        s = surface(g, U.primary_rays(g))
        hit = s["hits"][:, 0] > 0
        at_hits = np.concatenate([s["position"][hit], s["normal"][hit]], 1).astype(f32)
        cams, table = cameras_of(ra, g, at_hits[:, 0:3].mean(0) + f32([0, 0.5, 0]))
        points = np.ascontiguousarray(np.concatenate([at_hits, free_points(g)[0], UPJ.special_points(table)]), f32)
        plan = UPJ.Plan(points, table)
        occ = {}
        for cull in (1, 0):
            g.set_flag("useBackfaceCulling", cull)
            occ[cull] = occluded(g, plan)
        g.close()
        for a in (points, table, plan.pixel, plan.depth, plan.geo, plan.walk):
            a.setflags(write=False)
        _case[name] = dict(path=path, cams=cams, table=table, points=points, plan=plan, occ=occ, n_hits=int(hit.sum()))
    return _case[name]


def scene_of(ra, c, cull=None):
    g = ra.Scene(c["path"], W, H)
    if cull is not None:
        g.set_flag("useBackfaceCulling", cull)
    return g


def default_cull(g):
    return g.view_flags() & 1


# ---- 1. the restatement, and OPEN against Scene.occluded ------------------------------------------------------------------------------------
@pytest.mark.parametrize("cull", [1, 0])
@pytest.mark.parametrize("name", SCENES)
def test_every_pair_equals_the_restatement(ra, name, cull):
    c = case(ra, name)
    plan, occ = c["plan"], c["occ"][cull]
    g = scene_of(ra, c, cull)
    got = project(g, c["points"], c["table"])
    exp = plan.expected(occ)
    assert got["pixel"].shape == (plan.K, plan.n, 2) and got["depth"].shape == (plan.K, plan.n) and got["flags"].dtype == np.uint8
    bad = UPJ.differing(got, exp)
    assert not bad, "%s cull %d: pairs that differ from the restatement: %s of %d" % (name, cull, bad, plan.K * plan.n)
    # OPEN only where a shadow ray is cast, and both answers there; every class of pair is present
    is_open = (got["flags"] & UPJ.OPEN) != 0
    assert not is_open[~plan.walk].any() and is_open[plan.walk].any() and not is_open[plan.walk].all()
    geo = got["flags"] & 7
    front, inside, facing = (geo & 1) != 0, (geo & 2) != 0, (geo & 4) != 0
    assert (front & ~inside).any() and (~front).any() and inside.any() and facing.any() and (~facing).any() and not (inside & ~front).any()
    with np.errstate(all="ignore"):
        assert np.isnan(got["pixel"]).any() and np.isinf(got["pixel"]).any() and (got["depth"] == 0).any()
    open_, blocked, out = plan.shares(occ)
    print("%s cull %d: %d points x %d cameras; of the pairs FRONT && INSIDE open %.3f, blocked %.3f; outside %.3f" % (
        name, cull, plan.n, plan.K, open_, blocked, out))
    # the second camera's classes, as tests/test_project_cpu.py chose it (there on the oracle's answers)
    if name == "cfg1_simple_shapes":
        k = 1
        w2 = plan.walk[k, :c["n_hits"]]
        o2 = is_open[k, :c["n_hits"]][w2]
        assert o2.mean() >= 0.02 and (~o2).mean() >= 0.02 and (~w2).mean() >= 0.02
    # without visibility nothing is walked: OPEN is never set and everything else is the same
    blind = project(g, c["points"], c["table"], visibility=False)
    assert not UPJ.differing(blind, plan.expected(None)), "with_visibility = 0"
    g.close()


def test_transparent_objects_do_not_block(ra):
    """mixed_materials: of the shadow rays towards the cameras, some meet a Transparent object first, nearer than the camera, and are OPEN"""
    name = "mixed_materials"
    c = case(ra, name)
    plan = c["plan"]
    g = scene_of(ra, c)
    blocks = U.object_blocks(open(c["path"]).read())
    transparent = [k for k, b in enumerate(blocks) if b.get("material", "").startswith("transparent")]
    assert transparent
    first = surface(g, plan.shadow_rays)["hits"]
    through = (first[:, 0] > 0) & np.isin(first[:, 1].astype(np.int32), transparent) & (first[:, 3] < plan.shadow_tmax)
    fl = project(g, c["points"], c["table"])["flags"]
    is_open = ((fl & UPJ.OPEN) != 0)[plan.walk]
    print("%s: %d shadow rays, %d meet a transparent object first, %d of those are open" % (name, len(first), through.sum(), (through & is_open).sum()))
    assert (through & is_open).sum() >= 20
    g.close()


# ---- 2. the round trip on the device ---------------------------------------------------------------------------------------------------------
def aov_of(g, cams, w, h):
    n = len(cams)
    pos = torch.zeros((n, h, w, 3), dtype=torch.float32, device="cuda")
    nrm = torch.zeros((n, h, w, 3), dtype=torch.float32, device="cuda")
    obj = torch.full((n, h, w), -1, dtype=torch.int32, device="cuda")
    g.render_views_aov(cams, position=pos, normal=nrm, object_id=obj)
    return pos, nrm, obj


@pytest.mark.parametrize("name", SCENES)
def test_round_trip_through_the_cameras(ra, name):
    c = case(ra, name)
    g = scene_of(ra, c)
    w, h = 64, 48
    cams = [own_camera(g), UPJ.SECOND_CAMERA]
    pos, nrm, obj = aov_of(g, cams, w, h)
    ys, xs = torch.meshgrid(torch.arange(h, device="cuda"), torch.arange(w, device="cuda"), indexing="ij")
    both = UPJ.FRONT | UPJ.INSIDE
    seen_other = 0
    # (a Transparent object blocks no shadow ray: a point seen through one is OPEN, and the camera's first hit at its pixel is that object)
    blocks = U.object_blocks(open(c["path"]).read())
    transparent = torch.tensor([k for k, blk in enumerate(blocks) if blk.get("material", "").startswith("transparent")] or [-2], dtype=torch.int32, device="cuda")
    for a in (0, 1):
        hit = (obj[a] >= 0).reshape(-1)
        points = torch.cat([pos[a].reshape(-1, 3), nrm[a].reshape(-1, 3)], 1)[hit].contiguous()
        out = g.project_points(points, cams, w, h)
        near = torch.floor(out["pixel"] + 0.5)
        fl = out["flags"]
        # into the same camera: every hit pixel maps to itself by the nearest-pixel rule, and is FRONT and INSIDE
        assert bool(((fl[a] & both) == both).all()), "%s camera %d: a hit pixel is not FRONT && INSIDE in its own camera" % (name, a)
        assert torch.equal(near[a, :, 0], xs.reshape(-1)[hit].float()) and torch.equal(near[a, :, 1], ys.reshape(-1)[hit].float())
        # into the other camera: where OPEN, that camera's first hit at the nearest pixel lies within the same object (or a Transparent one in front of it)
        b = 1 - a
        is_open = (fl[b] & UPJ.OPEN) != 0
        px, py = near[b, is_open, 0].long(), near[b, is_open, 1].long()
        assert bool((px >= 0).all() and (px < w - 1).all() and (py >= 0).all() and (py < h - 1).all())
        same = (obj[b][py, px] == obj[a].reshape(-1)[hit][is_open]) | torch.isin(obj[b][py, px], transparent)
        seen_other += int(is_open.sum())
        # The exceptions, each of them geometry the id buffer cannot show, each counted and bounded so that growth in one shows up:
        # (i) a point within half a pixel of a silhouette, or on a feature thinner than a pixel, falls into a pixel whose centre ray passes its
        # object; the object is then within two pixels in the other camera's id buffer (compared by id, not by coordinates).  The smallest
        # objects of these 64x48 views are about 6 pixels in radius, and the half-pixel rim of such a disc is 1 - (5.5 / 6)^2 = 16 % of it:
        # at most 20 % of the open points.
        own_id = obj[a].reshape(-1)[hit][is_open]
        n_obj = int(obj.max()) + 1
        present = torch.stack([torch.nn.functional.max_pool2d((obj[b] == k).float()[None, None], 5, 1, 2)[0, 0] > 0 for k in range(n_obj)])
        edge = present[own_id.long(), py, px] & ~same
        # (ii) a surface that camera b meets at grazing incidence or from behind has no pixel of its own there -- a flat mesh seen edge-on
        # covers none, a one-sided surface seen from behind under back-face culling is not drawn -- yet is hidden by nothing.  cos < 0.05
        # (under 3 degrees off the surface; NaN is not excused), computed here from the positions: at most 5 % of the open points.
        cpos = torch.tensor(cams[b][0], dtype=torch.float32, device="cuda")
        cvec = points[is_open, 0:3] - cpos
        dist = cvec.norm(dim=1)
        nvec = points[is_open, 3:6]
        cosv = -(nvec * cvec).sum(1) / (nvec.norm(dim=1) * dist)
        grazing = (cosv < 0.05) & ~same & ~edge
        wrong = ~(same | edge | grazing)
        # (iii) a part of a rotated mesh outside its clipped root box (objects.cpp:328-330) is met only by rays that cross the box: another
        # camera draws it, this one neither draws it nor is blocked by it.  Only where the renderer's own trace along the exact line from the
        # camera to P meets NOTHING before P -- a miss, or a first hit no nearer than P (within 1e-4 of the distance, the scale of the bias),
        # or a Transparent one.  An opaque object met before P is a blocker, and the pair fails.  At most 2 % of the open points.
        unseen = torch.zeros_like(wrong)
        if bool(wrong.any()):
            line = cvec[wrong] / dist[wrong][:, None]
            first = g.surface_rays(torch.cat([cpos.expand_as(line), line], 1).contiguous(), hits=True, position=False, normal=False, albedo=False)["hits"]
            nothing = (first[:, 0] <= 0) | (first[:, 3] >= dist[wrong] * (1 - 1e-4)) | torch.isin(first[:, 1].int(), transparent)
            unseen[wrong.clone()] = nothing
            wrong = wrong & ~unseen
        n_open = int(is_open.sum())
        print("%s, camera %d into %d: %d open points; %d in their object's pixels or behind a transparent one, %d within two pixels, %d grazing or from behind, "
              "%d with nothing before them on the camera's own line" % (name, a, b, n_open, int(same.sum()), int(edge.sum()), int(grazing.sum()), int(unseen.sum())))
        pairs = torch.stack([own_id[wrong], obj[b][py, px][wrong], px[wrong].int(), py[wrong].int()], 1).cpu().numpy()
        assert not bool(wrong.any()), "%s, camera %d into %d: %d open points land inside another object: (own, seen, x, y) %s" % (
            name, a, b, len(pairs), pairs[:12].tolist())
        assert int(edge.sum()) <= 0.20 * n_open and int(grazing.sum()) <= 0.05 * n_open and int(unseen.sum()) <= 0.02 * n_open
    torch.cuda.synchronize()
    assert seen_other > 50
    g.close()


# ---- 3. batches, orders and tables ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reorder", [0, 1])
def test_pairs_are_independent_of_batch_and_table(ra, reorder):
    c = case(ra, "cfg2_smooth_4k")
    g = scene_of(ra, c)
    pool, table = c["points"], c["table"]
    n, K = len(pool), len(table)
    want = project(g, pool, table)                   # (the default: no grouping at these sizes)
    assert not UPJ.differing(want, c["plan"].expected(c["occ"][default_cull(g)]))
    g.set_knob("trace_reorder", reorder)             # (1: the sort runs on every batch, however small)
    rng = np.random.default_rng(23)
    perm = rng.permutation(n)
    assert not UPJ.differing(project(g, pool[perm], table), {k: want[k][:, perm] for k in CH}), "a shuffled batch, reorder %d" % reorder
    half = n // 2 + 7
    a, b = project(g, pool[:half], table), project(g, pool[half:], table)
    assert not UPJ.differing({k: np.concatenate([a[k], b[k]], 1) for k in CH}, want), "the batch split in two, reorder %d" % reorder
    for m in (1, 63, 64, 65):
        first = int(rng.integers(0, n - m))
        bad = UPJ.differing(project(g, pool[first:first + m], table), {k: want[k][:, first:first + m] for k in CH})
        assert not bad, "n = %d, reorder %d: %s" % (m, reorder, bad)
    # the table: one camera, two, six, and 256 records in another order -- a pair's result is its camera's and its point's alone
    for ks in ([3], [8, 0], [2, 3, 4, 5, 6, 7]):
        assert not UPJ.differing(project(g, pool, table[ks]), {k: want[k][ks] for k in CH}), "cameras %s, reorder %d" % (ks, reorder)
    ks = rng.integers(0, K, 256)
    sub = slice(0, 515)
    assert not UPJ.differing(project(g, pool[sub], table[ks]), {k: want[k][ks][:, sub] for k in CH}), "256 cameras, reorder %d" % reorder
    # a slice of a larger table that starts at a record of its own (4-byte aligned, not 32)
    big = dev(np.concatenate([np.full(1, FILL, f32), table.reshape(-1)]))
    out = host(g.project_points(dev(pool), big[1:].view(K, 24), depth=True))
    assert not UPJ.differing(out, want), "an unaligned table"
    empty = g.project_points(dev(pool[:0]), dev(table), depth=True)
    assert [tuple(empty[k].shape) for k in CH] == [(K, 0, 2), (K, 0), (K, 0)] and empty["flags"].dtype == torch.uint8
    g.close()


# ---- 4. only what is asked for is written (the C entry, directly) --------------------------------------------------------------------------
class Buffers:
    """The three channels of K cameras and n points, each in the middle of a larger pre-filled allocation"""
    TAIL = {"pixel": 2, "depth": 1, "flags": 1}

    def __init__(self, K, n):
        self.K, self.n = K, n
        self.flat, self.ptr = {}, {}
        for c in CH:
            size = K * n * self.TAIL[c] + 2 * GUARD
            if c == "flags":
                self.flat[c] = torch.full((size,), 0xA5, dtype=torch.uint8, device="cuda")
                self.ptr[c] = self.flat[c].data_ptr() + GUARD
            else:
                self.flat[c] = torch.full((size,), FILL, dtype=torch.float32, device="cuda")
                self.ptr[c] = self.flat[c].data_ptr() + 4 * GUARD

    def struct(self, ra, names):
        return ra.ProjectBuffers(*[self.ptr[c] if c in names else None for c in CH])

    def read(self):
        torch.cuda.synchronize()
        out = {}
        for c in CH:
            f = self.flat[c].cpu().numpy()
            fill = np.uint8(0xA5) if c == "flags" else f32(FILL)
            assert (f[:GUARD] == fill).all() and (f[-GUARD:] == fill).all(), "%s: written outside the buffer" % c
            out[c] = f[GUARD:len(f) - GUARD].reshape((self.K, self.n) + ((2,) if c == "pixel" else ()))
        return out


def untouched(a):
    return (a == (np.uint8(0xA5) if a.dtype == np.uint8 else f32(FILL))).all()


def stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def call(ra, g, tp, tc, b, names, vis=1, n=None, K=None):
    rtx, _ = ra.load()
    s = b.struct(ra, names)
    return rtx.rtx_project_points(g.gpu(), tp.shape[0] if n is None else n, C.c_void_p(tp.data_ptr()) if tp is not None else None,
                                  tc.shape[0] if K is None else K, C.c_void_p(tc.data_ptr()) if tc is not None else None, vis, C.byref(s),
                                  stream_ptr())


def test_only_what_was_asked_for_is_written(ra):
    c = case(ra, "area_light")
    g = scene_of(ra, c)
    points, table = c["points"][:-1], c["table"]
    n, K = len(points), len(table)
    exp = c["plan"].expected(c["occ"][default_cull(g)])
    exp = {k: v[:, :-1] for k, v in exp.items()}
    tp, tc = dev(points), dev(table)
    b = Buffers(K, n)
    assert call(ra, g, tp, tc, b, CH) == 0
    full = b.read()
    assert not UPJ.differing(full, exp)
    for names in [(k,) for k in CH] + [("pixel", "flags"), ("depth", "flags")]:
        for vis in (1, 0):
            b = Buffers(K, n)
            assert call(ra, g, tp, tc, b, names, vis=vis) == 0
            got = b.read()
            for k in CH:
                if k not in names:
                    assert untouched(got[k]), "%s was written by a call for %s" % (k, names)
                elif k == "flags" and not vis:
                    assert np.array_equal(got[k], full[k] & ~np.uint8(UPJ.OPEN)) and (full[k] & UPJ.OPEN).any()
                else:
                    assert np.array_equal(UPJ.bits(got[k]), UPJ.bits(full[k])), "%s of a call for %s differs from the three-channel call" % (k, names)
    assert set(g.project_points(tp, tc)) == {"pixel", "flags"} and set(g.project_points(tp, tc, pixel=False, depth=True, flags=False)) == {"depth"}
    torch.cuda.synchronize()
    g.close()


# ---- 5. scene state and refusals ---------------------------------------------------------------------------------------------------------------
def check_against_occluded(g, points, table, what):
    """project_points on Scene g as it is now: the restatement, with the visibility from g.occluded"""
    plan = UPJ.Plan(points, table)
    occ = occluded(g, plan)
    bad = UPJ.differing(project(g, points, table), plan.expected(occ))
    assert not bad, "%s: %s" % (what, bad)
    return occ


def test_after_scene_edits(ra):
    c = case(ra, "mixed_materials")
    g = scene_of(ra, c)
    points, table = c["points"][::3], c["table"][[0, 1, 8]]
    before = check_against_occluded(g, points, table, "as loaded")
    g.move_object(3, pos=(0.4, 1.2, -5.5), radius=0.85)
    g.move_object(1, rot=(-40, 10, 70), pos=(-0.9, 0.2, -4.4))
    moved = check_against_occluded(g, points, table, "move_object")
    assert not np.array_equal(before, moved)
    v, nrm = g.mesh_vertices(2)                    # (the reflective mesh: object 1, the transparent one, blocks nothing)
    g.set_vertices(2, dev(v * (f32(1) + f32(0.8) * (v[:, 1:2] > np.median(v[:, 1])))))      # (the upper half 1.8 times as wide)
    deformed = check_against_occluded(g, points, table, "set_vertices")
    print("answers that change: %d with the moves, %d with the deformation, of %d" % ((before != moved).sum(), (moved != deformed).sum(), len(moved)))
    g.set_light(0, position=(1.5, 0.5, -1.5), intensity=0.9)
    assert np.array_equal(check_against_occluded(g, points, table, "set_light"), deformed)      # (a light changes nothing)
    g.close()


def test_flags_depth_and_counters_change_nothing(ra, tmp_path):
    name = "cfg2_smooth_4k"
    c = case(ra, name)
    g = scene_of(ra, c)
    exp = c["plan"].expected(c["occ"][default_cull(g)])
    g.set_flag("showNormals", 1)
    assert not UPJ.differing(project(g, c["points"], c["table"]), exp), "showNormals"
    g.set_flag("showNormals", 0)
    f = ra.Scene(scene_copy(name, str(tmp_path), dict(max_ray_depth=0)), W, H)
    assert not UPJ.differing(project(f, c["points"], c["table"]), exp), "max_ray_depth = 0"
    f.close()
    g.counters_enable(True)
    g.counters_reset()
    assert not UPJ.differing(project(g, c["points"], c["table"]), exp), "counters enabled"
    assert not g.counters().any()
    g.counters_enable(False)
    # row ownership is ignored
    g.set_row_ownership(8, 2, 1)
    assert not UPJ.differing(project(g, c["points"], c["table"]), exp), "row ownership"
    g.close()


@pytest.mark.parametrize("as_current", [False, True])
def test_written_on_another_stream(ra, as_current):
    c = case(ra, "cfg2_smooth_4k")
    g = scene_of(ra, c)
    exp = c["plan"].expected(c["occ"][default_cull(g)])
    src_p, src_c = dev(c["points"]), dev(c["table"])
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    for cams in (None, c["cams"]):
        with torch.cuda.stream(st):
            tp = torch.full_like(src_p, float("nan"))       # (written on st: a call that did not wait for the copy would read NaNs)
            tp.copy_(src_p)
            tc = torch.full_like(src_c, float("nan"))
            tc.copy_(src_c)
            kw = {} if as_current else dict(stream=st)
            out = g.project_points(tp, tc if cams is None else cams, depth=True, **kw)
        st.synchronize()
        got = {k: v.cpu().numpy() for k, v in out.items()}
        want = exp if cams is None else {k: v[:len(cams)] for k, v in exp.items()}
        assert not UPJ.differing(got, want), "stream, as current %s, %s" % (as_current, "a table" if cams is None else "a camera sequence")
    g.close()


def test_refusals_leave_the_buffers_untouched(ra):
    c = case(ra, "cfg2_smooth_4k")
    g = scene_of(ra, c)
    rtx, _ = ra.load()
    points, table = c["points"][:1000], c["table"]
    n, K = len(points), len(table)
    tp, tc = dev(points), dev(table)
    with pytest.raises(ValueError, match="project_points: nothing to compute"):
        g.project_points(tp, tc, pixel=False, flags=False)
    with pytest.raises(ValueError, match=r"project_points: cameras must have shape \(K, 24\)"):
        g.project_points(tp, tc[:, :23].contiguous())
    with pytest.raises(ValueError, match="project_points: a camera table has its sizes in it"):
        g.project_points(tp, tc, 48, 32)
    with pytest.raises(ValueError, match="project_points: 1 .. 256 cameras, got 0"):
        g.project_points(tp, tc[:0])
    b = Buffers(K, n)
    null_out = lambda: rtx.rtx_project_points(g.gpu(), n, C.c_void_p(tp.data_ptr()), K, C.c_void_p(tc.data_ptr()), 1, None, stream_ptr())
    refused = [
        ("no output", lambda: call(ra, g, tp, tc, b, ())),
        ("NULL out", null_out),
        ("NULL points", lambda: call(ra, g, None, tc, b, CH, n=n)),
        ("NULL cameras", lambda: call(ra, g, tp, None, b, CH, K=K)),
        ("n_cams 0", lambda: call(ra, g, tp, tc, b, CH, K=0)),
        ("n_cams 257", lambda: call(ra, g, tp, tc, b, CH, K=257)),
        ("n = 0xFFFFFFC1", lambda: call(ra, g, tp, tc, b, CH, n=0xFFFFFFC1)),
    ]
    for what, fn in refused:
        assert fn() == -1, what                 # RTX_ERR_ARG
        assert rtx.rtx_last_error(), what
    assert call(ra, g, None, tc, b, CH, n=0) == 0      # n == 0: nothing to do
    assert all(untouched(a) for a in b.read().values())
    # ... and the call works afterwards
    assert call(ra, g, tp, tc, b, ("depth", "flags")) == 0
    got = b.read()
    exp = c["plan"].expected(c["occ"][default_cull(g)])
    assert untouched(got["pixel"]) and not UPJ.differing(got, {k: v[:, :n] for k, v in exp.items()}, ("depth", "flags"))
    g.close()


# ---- 6. camera_table -----------------------------------------------------------------------------------------------------------------------------
def test_camera_table_is_view_target(ra):
    c = case(ra, "mixed_materials")
    g = scene_of(ra, c)
    cams = c["cams"] + [UPJ.WIDE_CAMERA]
    for size in ((None, None), UPJ.WIDE_SIZE):
        t = g.camera_table(cams, *size)
        assert t.dtype == torch.float32 and tuple(t.shape) == (len(cams), 24) and t.device.type == "cuda"
        tab = t.cpu().numpy()
        for r, cam in zip(tab, cams):
            v = g.view_target(cam[0], cam[1], cam[2] if len(cam) == 3 else None, *size)
            assert np.array_equal(UPJ.bits(r[0:3]), UPJ.bits(np.array(v.cam_pos, f32))) and np.array_equal(UPJ.bits(r[8:24]), UPJ.bits(np.array(v.cam_matrix, f32)))
            assert np.array_equal(UPJ.bits(r[3:5]), UPJ.bits(np.array([v.scale, v.aspect], f32))) and (r[5], r[6], r[7]) == (v.width, v.height, 0)
    # the scene's own pose at the scene's size is the view the renderer uses
    own = UPJ.record(*g.camera(), W, H)
    assert np.array_equal(UPJ.bits(g.camera_table([own_camera(g)]).cpu().numpy()[0]), UPJ.bits(own))
    # a table tensor and the camera sequence give the same bits
    pts = dev(c["points"][:777])
    a = host(g.project_points(pts, cams[:8], depth=True))
    b = host(g.project_points(pts, g.camera_table(cams[:8]), depth=True))
    assert not UPJ.differing(a, b) and not UPJ.differing(a, {k: v[:8, :777] for k, v in c["plan"].expected(c["occ"][default_cull(g)]).items()})
    assert (g.width, g.height) == (W, H) and own_camera(g) == c["cams"][0]
    g.close()


# ---- 7. bake_view ---------------------------------------------------------------------------------------------------------------------------------
def test_bake_view_of_a_quad_facing_the_camera(ra, tmp_path):
    g = ra.Scene(UT.write_mesh_scene(tmp_path, "quad", UT.quad_obj(), size="2,1.5,1", rot="0,0,0"), 64, 48)
    cam = own_camera(g)
    iw, ih, tw, th = 64, 48, 24, 20
    xs, ys = np.meshgrid(np.arange(iw, dtype=f32), np.arange(ih, dtype=f32))
    image = dev(np.stack([xs, ys, np.ones_like(xs)], -1))

    def bake(margin):
        texels, seen = g.bake_view(0, cam, image, tw, th, margin=margin)
        torch.cuda.synchronize()
        return texels.cpu().numpy(), seen.cpu().numpy()

    t = g.texel_points(0, tw, th)
    pr = host(g.project_points(t["points"], [cam], iw, ih))
    tri = t["tri"].cpu().numpy()
    near = np.floor(pr["pixel"][0] + f32(0.5)).reshape(th, tw, 2)
    # (the nearest pixels are the restatement's, not only the call's own)
    plan = UPJ.Plan(t["points"].cpu().numpy(), g._camera_records([cam], iw, ih))
    assert np.array_equal(near, plan.nearest()[0].reshape(th, tw, 2)) and np.array_equal(pr["flags"][0] & 7, plan.geo[0])
    want = UPJ.INSIDE | UPJ.FACING | UPJ.OPEN | UPJ.FRONT
    texels, seen = bake(0)
    assert seen.dtype == bool and seen.shape == (th, tw) and texels.shape == (th, tw, 3)
    assert np.array_equal(seen, ((pr["flags"][0] & want) == want).reshape(th, tw) & (tri >= 0))
    assert (tri >= 0).all() and seen.all(), "the whole quad faces the camera and nothing is in the way"
    assert np.array_equal(texels[..., 0:2], near) and (texels[..., 2] == 1).all()
    assert (near[..., 0] >= 0).all() and (near[..., 0] < iw - 1).all() and len(np.unique(near.reshape(-1, 2), axis=0)) > 50
    # on another stream, as a torch stream and as a raw handle (where the host waits around torch's gather): the same bits
    other = torch.cuda.Stream()
    for st in (other, other.cuda_stream):
        tex_s, seen_s = g.bake_view(0, cam, image, tw, th, margin=2, stream=st)
        other.synchronize()
        tex_0, seen_0 = g.bake_view(0, cam, image, tw, th, margin=2)
        torch.cuda.synchronize()
        assert torch.equal(tex_s, tex_0) and torch.equal(seen_s, seen_0), "bake_view on %s" % type(st).__name__
    # a sphere between the camera and the quad: the texels in its shadow are unseen and 0 before the margin, the others as before
    g.add_object("sphere", pos=(0.05, 0.1, -1.5), radius=0.2)
    shadowed, seen2 = bake(0)
    assert (~seen2).sum() >= 10 and seen2.sum() >= 0.5 * tw * th and not shadowed[~seen2].any()
    assert np.array_equal(shadowed[seen2], texels[seen2])
    # (the shadow lies in the middle of the quad: no texel of the map's border is in it)
    assert seen2[0].all() and seen2[-1].all() and seen2[:, 0].all() and seen2[:, -1].all()
    g.close()
    # the margin: a layout that leaves a border uncovered -- 0 before the margin, filled by dilate_texels' rule after it
    g2 = ra.Scene(UT.write_mesh_scene(tmp_path, "inner", UT.quad_obj(0.25, 0.75), size="2,1.5,1", rot="0,0,0"), 64, 48)
    tri3 = g2.texel_points(0, tw, th)["tri"].cpu().numpy()
    out = {}
    for margin in (0, 2):
        tex, seen3 = g2.bake_view(0, cam, image, tw, th, margin=margin)
        torch.cuda.synchronize()
        out[margin] = tex.cpu().numpy()
        assert np.array_equal(seen3.cpu().numpy(), tri3 >= 0)
    assert (tri3 < 0).any() and not out[0][tri3 < 0].any() and (out[0][tri3 >= 0][:, 2] == 1).all()
    want2, _ = UT.dilate_ref(out[0], tri3, 2)
    assert np.array_equal(UPJ.bits(out[2]), UPJ.bits(want2)) and not np.array_equal(out[2], out[0])
    g2.close()
