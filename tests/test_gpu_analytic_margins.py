"""The rays of tests/util_analytic.py -- aimed at the limb of spheres, at origins in and on them, at |d.n| around 1e-8, at origins on planes,
at the horizon and at exact ties between two objects -- through every entry point that carries the analytic branch of traceWave
(rtx_kernels.hip; Sphere::intersectObject / Plane::intersectObject, objects.cpp:774-786, 807-814), on every scene form, against the CPU
oracle bit for bit: two results are equal when their bits are equal or both are NaN; signs of zero count.
tests/test_analytic_margins_cpu.py holds the oracle itself to the reference on the same rays and shows that they sit at their margins.

  cast_rays; trace_rays with trace_reorder 0 and 1 in its three output modes; occluded with the ranges of tests/test_gpu_margins.py in both
  object orders; surface_rays; light_rays(per_light) and scatter_rays against the restatements of their own modules, all on every ray of
  every family; frames -- pass 1, the
  frame in one launch cold and warm and in three, the SSAA mask, render_aov -- from the form's camera and from inside a sphere, a sphere's
  centre and a point on a plane.  Every case asserts the kernel variant it runs on; CASES names every (form, BOXES) pair."""
import numpy as np
import pytest

from tests import util_analytic as UA
from tests import util_aov as U
from tests import util_light as UL
from tests import util_occlusion as OC
from tests import util_scatter as SC
from tests import util_surface as SU
from tests.test_gpu_margins import occlusion_ranges

pytestmark = pytest.mark.gpu
f32 = np.float32

# (form, prune_boxes forced to): the forms without a mesh launch the ANALYTIC kernels, which have no box test
MESH_FORMS = ["with_mesh_cull", "with_mesh_nocull", "tie_quad_ab", "tie_quad_ba"]
CASES = [(form, boxes) for form in UA.FORMS for boxes in ((0, 1) if form in MESH_FORMS else (None,))]


def case_id(case):
    return case[0] if case[1] is None else "%s-boxes%d" % case


def variant_of(form, boxes):
    """(analytic, plain, cull, boxes) the launch must report"""
    return (form not in MESH_FORMS, form != "materials", bool(UA.cull_of(form)), bool(boxes))


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return str(tmp_path_factory.mktemp("gpu_analytic_margins"))


_oracle = {}


def reference(oracle, form, work):
    """Once per form: the scene file, all its families as one ray array (whole waves), the oracle's records and colours."""
    if form not in _oracle:
        fams = UA.families(form, oracle, work)
        rays = np.ascontiguousarray(np.concatenate([f.rays for f in fams.values()]), f32)
        path = UA.write_scene(form, work)
        o = oracle.OracleScene(path, UA.W, UA.H)
        hits, col = o.probe(rays)
        o.close()
        for a in (rays, hits, col):
            a.setflags(write=False)
        _oracle[form] = dict(path=path, rays=rays, hits=hits, colours=col,
                             family=np.concatenate([[name] * len(f.rays) for name, f in fams.items()]))
    return _oracle[form]


def scene(ra, form, boxes, path):
    g = ra.Scene(path, UA.W, UA.H)
    if boxes is not None:
        g.set_knob("prune_boxes", boxes)
    v = g.kernel_variant()
    assert (v["analytic"], v["plain"], v["cull"], v["boxes"], v["stats"]) == variant_of(form, boxes) + (False,), (form, boxes, v)
    return g


def first_bad(bad, ref, *shown):
    k = int(np.argmax(bad))
    return "%d of %d rays differ, first %d (%s): ray %s %s" % (int(bad.sum()), len(bad), k, ref["family"][k], ref["rays"][k], [a[k] for a in shown])


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, copy=True, order="C")).cuda()      # (the cached arrays are read-only)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_records_and_colours(ra, oracle, work, case):
    """cast_rays, and trace_rays grouped and ungrouped in its three output modes."""
    import torch
    form, boxes = case
    ref = reference(oracle, form, work)
    g = scene(ra, form, boxes, ref["path"])
    gh, gc = g.cast_rays(ref["rays"])
    bad = ~UA.same_bits(gh, ref["hits"]).all(1) | ~UA.same_bits(gc, ref["colours"]).all(1)
    assert not bad.any(), "cast_rays: " + first_bad(bad, ref, ref["hits"], gh, ref["colours"], gc)
    rays = dev(ref["rays"])
    for reorder in (0, 1):
        g.set_knob("trace_reorder", reorder)
        for hits, colours in ((True, True), (True, False), (False, True)):
            h, c = g.trace_rays(rays, hits=hits, colours=colours)
            torch.cuda.synchronize()
            assert (h is None) == (not hits) and (c is None) == (not colours)
            bad = np.zeros(len(ref["rays"]), bool)
            if hits:
                bad |= ~UA.same_bits(h.cpu().numpy(), ref["hits"]).all(1)
            if colours:
                bad |= ~UA.same_bits(c.cpu().numpy(), ref["colours"]).all(1)
            assert not bad.any(), "trace_rays, trace_reorder %d, hits %d colours %d: %s" % (reorder, hits, colours, first_bad(bad, ref, ref["hits"], ref["colours"]))
    assert g.kernel_variant()["analytic"] == variant_of(form, boxes)[0]
    g.close()


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_occlusion_queries(ra, oracle, work, tmp_path, case):
    """occluded: spheres and planes first (the default) and in scene order, under every kind of range.  The expectation is the oracle's
    nearest hit among the objects that are not Transparent (materials: the form without its glass sphere)."""
    import torch
    form, boxes = case
    ref = reference(oracle, form, work)
    if form == "materials":
        opaque, dropped = OC.opaque_scene(ref["path"], tmp_path)
        assert dropped == 1
        o = oracle.OracleScene(opaque, UA.W, UA.H)
        h, _ = o.probe(ref["rays"], colours=False)
        o.close()
        hit, tnear = h[:, 0] > 0, h[:, 3].astype(f32)
    else:
        hit, tnear = ref["hits"][:, 0] > 0, ref["hits"][:, 3].astype(f32)
    g = scene(ra, form, boxes, ref["path"])
    rays = dev(ref["rays"])
    for order in (0, 1):
        g.set_knob("occluded_scene_order", order)
        for label, tmax in occlusion_ranges(hit, tnear):
            got = g.occluded(rays, dev(tmax) if isinstance(tmax, np.ndarray) else tmax)
            torch.cuda.synchronize()
            bad = got.cpu().numpy() != OC.expected(hit, tnear, f32(np.inf) if tmax is None else tmax)
            assert not bad.any(), "occluded_scene_order %d, ranges %s: %s" % (order, label, first_bad(
                bad, ref, ref["hits"], np.broadcast_to(np.asarray(np.inf if tmax is None else tmax, f32), tnear.shape)))
    g.close()


def surface_mismatches(got, exp):
    """tests/util_surface.mismatches under the NaN rule (a position can be inf - inf)"""
    bad = {}
    for c in SU.CHANNELS:
        if c == "normal":
            enc = got[c] / f32(2) + f32(0.5)
            d = np.where(exp["hit"][:, None], ~UA.same_bits(enc, exp["normal_colour"]), UA.bits(got[c]) != 0).any(-1)
        else:
            d = ~UA.same_bits(got[c], exp[c])
            d = d.any(-1) if d.ndim == 2 else d
        if d.any():
            bad[c] = (int(d.sum()), int(np.argmax(d)))
    return bad


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_surface_data(ra, oracle, work, case):
    """surface_rays: records, position, normal (as N / 2 + 0.5 against the oracle's showNormals colours), albedo and specular."""
    import torch
    form, boxes = case
    ref = reference(oracle, form, work)
    exp = SU.expected_of(ref["path"], UA.W, UA.H, None, ref["rays"])
    assert UA.same_bits(exp["hits"], ref["hits"]).all()
    g = scene(ra, form, boxes, ref["path"])
    got = g.surface_rays(dev(ref["rays"]), hits=True, position=True, normal=True, albedo=True, specular=True)
    torch.cuda.synchronize()
    got = {c: v.cpu().numpy() for c, v in got.items()}
    bad = surface_mismatches(got, exp)
    assert not bad, "%s: {channel: (rays that differ, the first)} %s; ray %s" % (form, bad, ref["rays"][next(iter(bad.values()))[1]])
    g.close()


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_direct_light_and_scatter(ra, oracle, work, case):
    """light_rays(per_light) against tests/util_light's restatement and scatter_rays against tests/util_scatter's, on every ray of every
    family: the limb rays on the glass and mirror spheres of `materials` among them.  N and the records come from surface_rays, which
    test_surface_data holds to the oracle on these very rays; the visibility of the shadow rays comes from occluded, which
    tests/test_gpu_occluded.py and test_occlusion_queries above hold to it."""
    import torch
    form, boxes = case
    ref = reference(oracle, form, work)
    pick = np.ones(len(ref["rays"]), bool)
    rays = ref["rays"]
    g = scene(ra, form, boxes, ref["path"])
    t = dev(rays)
    s = {c: v.cpu().numpy() for c, v in g.surface_rays(t, hits=True, normal=True, albedo=True, specular=True).items()}
    assert UA.same_bits(s["hits"], ref["hits"][pick]).all()
    objs, _ = g.device_objects()
    o = oracle.OracleScene(ref["path"], UA.W, UA.H)
    plan = UL.Plan(o, g.device_lights(), rays, s["hits"], s["normal"], bias=UL.BIAS)
    o.close()
    occ = g.occluded(dev(plan.shadow_rays), dev(plan.shadow_tmax))
    torch.cuda.synchronize()
    obj = s["hits"][:, 1].astype(np.int32)
    ns = np.where(obj >= 0, objs["n_specular"][np.maximum(obj, 0)], f32(0)).astype(f32)
    want = plan.reduce(occ.cpu().numpy(), ns)
    got = {c: v.cpu().numpy() for c, v in g.light_rays(t, hits=True, per_light=True).items()}
    bad = [c for c in UL.CHANNELS if c != "hits" and not (UA.same_bits(got[c], want[c]).all() if got[c].dtype == f32 else np.array_equal(got[c], want[c]))]
    assert not bad and UA.same_bits(got["hits"], s["hits"]).all(), "light_rays: %s differ" % bad
    const = {k: np.ascontiguousarray(objs[k]) for k in ("material", "ambient", "diffuse", "ior")}
    want = SC.restate(rays, s["hits"], s["normal"], s["albedo"], s["specular"], got["diffuse"], got["specular"], const)
    sc = {c: v.cpu().numpy() for c, v in g.scatter_rays(t, hits=True).items()}
    bad = [c for c in SC.SCATTER if not (UA.same_bits(sc[c], want[c]).all() if sc[c].dtype == f32 else np.array_equal(sc[c], want[c]))]
    assert not bad and UA.same_bits(sc["hits"], s["hits"]).all(), "scatter_rays: %s differ" % bad
    if form == "materials":
        limb = ref["family"][pick] == "limb"
        mat = np.where(obj >= 0, const["material"][np.maximum(obj, 0)], -1)
        assert (limb & (mat == SC.REFLECTIVE)).sum() >= 16 and (limb & (mat == SC.TRANSPARENT)).sum() >= 16
        assert (sc["kinds"] == 3).sum() >= 16 and (sc["kinds"] == 1).sum() >= 16
    g.close()


FRAME_CASES = [(form, boxes, cam) for form, boxes in CASES for cam, _ in UA.cameras(form)]


@pytest.mark.parametrize("case", FRAME_CASES, ids=lambda c: "%s-%s" % (case_id(c[:2]), c[2]))
def test_frames(ra, oracle, work, case):
    """Pass 1, the frame in one launch cold and warm and in three launches, the SSAA mask and render_aov, from the form's own camera and
    from inside a sphere, at a sphere's centre and on a plane."""
    import torch
    form, boxes, cam = case
    key = ("frame", form, cam)
    if key not in _oracle:
        path = UA.write_scene(form, work, cam=dict(UA.cameras(form))[cam], tag="_cam_" + cam)
        o = oracle.OracleScene(path, UA.W, UA.H)
        p1 = o.pass1()
        mask = o.sobel(p1)
        mask[0, :] = 0; mask[-1, :] = 0; mask[:, 0] = 0; mask[:, -1] = 0       # (border = 0 by definition)
        _oracle[key] = (path, p1, o.ssaa(p1), mask, U.expected(o, open(path).read()))
        o.close()
    path, p1, ref, ref_mask, aov = _oracle[key]
    g = scene(ra, form, boxes, path)
    W, H = UA.W, UA.H
    fb = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    g.render_pass1(fb)
    torch.cuda.synchronize()
    nd = int((~UA.same_bits(fb.cpu().numpy(), p1)).any(-1).sum())
    assert nd == 0, "pass 1: %d pixels differ" % nd
    for mode in (1, 1, 0):          # one launch cold, then warm (slow tiles split), three launches
        fb = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
        mask = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
        g.set_frame_mode(mode)
        g.render_frame(fb, mask)
        assert g.frame_status() == 0 and g.frame_mode()[0] == mode
        nd = int((~UA.same_bits(fb.cpu().numpy(), ref)).any(-1).sum())
        assert nd == 0, "%s: %d pixels differ" % ("one launch" if mode else "three launches", nd)
        assert np.array_equal(mask.cpu().numpy() != 0, ref_mask != 0), "%s: the SSAA mask differs" % ("one launch" if mode else "three launches")
    bufs = dict(depth=torch.zeros((H, W), dtype=torch.float32, device="cuda"), object_id=torch.zeros((H, W), dtype=torch.int32, device="cuda"),
                triangle_id=torch.zeros((H, W), dtype=torch.int32, device="cuda"), uv=torch.zeros((H, W, 2), dtype=torch.float32, device="cuda"),
                normal=torch.zeros((H, W, 3), dtype=torch.float32, device="cuda"), albedo=torch.zeros((H, W, 3), dtype=torch.float32, device="cuda"))
    g.render_aov(**bufs)
    torch.cuda.synchronize()
    bad = U.mismatches({c: v.cpu().numpy() for c, v in bufs.items()}, aov, U.written_mask(W, H))
    assert not bad, "render_aov: {channel: pixels that differ} %s" % bad
    assert g.kernel_variant()["analytic"] == variant_of(form, boxes)[0]
    g.close()


def test_case_list_is_complete():
    """Every form; every mesh form with the box test of the prune records forced on and off; every variant the analytic branch is compiled
    into that a scene of spheres, planes and one Diffuse mesh can choose: ANALYTIC with and without PLAIN, and MESH PLAIN with BOXES and CULL
    each way.  Every form with every camera it has."""
    assert {f for f, _ in CASES} == set(UA.FORMS) and len(UA.FORMS) == 14
    for form in UA.FORMS:
        assert {b for f, b in CASES if f == form} == ({0, 1} if UA.has_mesh(form) else {None})
    seen = {variant_of(f, b) for f, b in CASES}
    assert {(True, True, True, False), (True, False, True, False)} <= seen
    assert {(False, True, c, b) for c in (True, False) for b in (True, False)} <= seen
    assert {(f, b) for f, b, _ in FRAME_CASES} == set(CASES)      # (every ray test is parametrised over CASES itself)
    for form in UA.FORMS:
        want = {"own"} | ({"inside", "centre"} if any(o["type"] == "sphere" and 0.1 <= o["r"] <= 100 for o in UA.objects_of(form)) else set()) \
            | ({"on_plane"} if any(o["type"] == "plane" and o["pos"] != UA.CAM for o in UA.objects_of(form)) else set())
        assert {c for f, _, c in FRAME_CASES if f == form} == want, form
