"""The source copies of the prune records (rtx_source.hip sourceP / rtxSourceRefKernel / rtxSourceSlotKernel, rtx_api.hip buildSources, selected
in traceWave through srcSel, consumed in pruneEval8 as Pn = ainf <= kSrcAinfMax ? P : Pgen) with the source where they are closest to
being wrong: tests/util_sources.py puts the camera and a point light in and just off the plane of a triangle of a fine sheet, under long
plane normals, either side of the 32-unit fallback and at large coordinates.  The mesh chooses the kernels with the box test (BOXES) by
itself.  Frames, first-hit buffers and ambient occlusion are compared with the CPU oracle bit for bit; the copies themselves are read
back and compared with the host's sourceP of the placed triangles (util_sources.check_records).  tests/test_source_margins_cpu.py keeps
the case list complete and every case decisive."""
import numpy as np
import pytest

from tests import util_ao as AO
from tests import util_aov as U
from tests import util_sources as S

pytestmark = pytest.mark.gpu
f32 = np.float32
bits = S.bits


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return str(tmp_path_factory.mktemp("sources"))


def check_variant(g, d, what):
    """No knob: the mesh chooses BOXES by itself; PLAIN follows from the material, CULL from the scene."""
    v = g.kernel_variant()
    assert v["boxes"], "%s: the sheet no longer chooses the kernels with the box test by itself: %r" % (what, v)
    assert (v["plain"], v["cull"], v["analytic"], v["stats"]) == (d["material"] == "diffuse", bool(d["cull"]), False, False), (what, v)
    return v


def check_frames(g, oracle, path, what):
    """Pass 1, the post-SSAA frame and the SSAA mask against the oracle: the frame in one launch twice (cold, then warm: slow tiles split),
    then in three launches."""
    import torch
    p1, ref, ref_mask = S.reference(oracle, path)
    for mode, label in ((1, "one launch, cold"), (1, "one launch, warm"), (0, "three launches")):
        fb = torch.zeros((S.H, S.W, 3), dtype=torch.float32, device="cuda")
        mask = torch.zeros((S.H, S.W), dtype=torch.uint8, device="cuda")
        g.set_frame_mode(mode)
        g.render_frame(fb, mask)
        assert g.frame_status() == 0 and g.frame_mode()[0] == mode
        got = fb.cpu().numpy()
        nd = int((bits(ref) != bits(got)).any(-1).sum())
        assert nd == 0, "%s, %s: %d pixels of the frame differ from the oracle's" % (what, label, nd)
        assert np.array_equal(mask.cpu().numpy() != 0, ref_mask != 0), "%s, %s: the SSAA mask differs" % (what, label)
        fb.zero_()
        g.render_pass1(fb)
        torch.cuda.synchronize()
        nd = int((bits(p1) != bits(fb.cpu().numpy())).any(-1).sum())
        assert nd == 0, "%s, after %s: %d pixels of pass 1 differ from the oracle's" % (what, label, nd)


def check_copies(ra, g, d, case, what):
    shares = S.check_records(ra, g.device_prune_copies(0), g.device_mesh_flat(0)[0], g.device_mesh(0)["refs"], d, case, what)
    print("%s: certified share of the non-empty slots: camera %.3f, light %.3f" % (what, shares[0], shares[1]))


def check_aov(g, path, what):
    import torch
    exp = U.expected_of(path, S.W, S.H)
    depth = torch.full((S.H, S.W), -7.0, dtype=torch.float32, device="cuda")
    tri = torch.full((S.H, S.W), -7, dtype=torch.int32, device="cuda")
    obj = torch.full((S.H, S.W), -7, dtype=torch.int32, device="cuda")
    g.render_aov(depth=depth, triangle_id=tri, object_id=obj)
    torch.cuda.synchronize()
    got = dict(depth=depth.cpu().numpy(), triangle_id=tri.cpu().numpy(), object_id=obj.cpu().numpy())
    bad = U.mismatches(got, exp, U.written_mask(S.W, S.H), ("depth", "triangle_id", "object_id"))
    assert not bad, "%s: first-hit buffers differ from the oracle's: %s" % (what, bad)
    assert (exp["object_id"] == 1).sum() >= S.DECISIVE_FLOOR, "%s: the camera hardly sees the sheet" % what


@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_source_placements_against_the_oracle(ra, oracle, work, case):
    what = S.case_id(case)
    path, d = S.write_case(oracle, work, case)
    g = ra.Scene(path, S.W, S.H)
    v = check_variant(g, d, what)
    check_copies(ra, g, d, case, what)
    check_frames(g, oracle, path, what)
    if case[0] == "camera":
        check_aov(g, path, what)
    check_copies(ra, g, d, case, what + ", after the frames")
    assert g.kernel_variant() == v
    g.close()


@pytest.mark.parametrize("cull", S.CULLS)
def test_ambient_occlusion_from_a_camera_in_the_plane(ra, oracle, work, tmp_path, cull):
    """render_ao walks its first hits with the camera's copy: 16 sphere_directions and a finite radius from the camera in the plane of
    triangle k, against the render_aov + oracle yardstick of tests/util_ao.py."""
    import torch
    case = ("camera", "near", 0.0, "diffuse", cull)
    what = S.case_id(case)
    path, d = S.write_case(oracle, work, case)
    g = ra.Scene(path, S.W, S.H)
    check_variant(g, d, what)
    dirs = ra.sphere_directions(16)
    radius = 0.25
    e = AO.Expectation(g, dirs)
    want_counts, want_ao = e.by_oracle(oracle, path, tmp_path, None, radius)
    ao = torch.full((S.H, S.W), -7.0, dtype=torch.float32, device="cuda")
    counts = torch.full((S.H, S.W), -7, dtype=torch.int32, device="cuda")
    g.render_ao(torch.from_numpy(dirs).cuda(), radius, ao=ao, counts=counts)
    torch.cuda.synchronize()
    mask = U.written_mask(S.W, S.H)
    got_counts, got_ao = counts.cpu().numpy().view(np.uint32), ao.cpu().numpy()
    traced, opened = want_counts >> 16, want_counts & 0xFFFF
    print("%s: %d traced rays, %d open" % (what, int(traced[mask].sum()), int(opened[mask].sum())))
    assert traced[mask].sum() > 1000 and 0 < opened[mask].sum() < traced[mask].sum(), "%s: the radius no longer splits the rays" % what
    assert np.array_equal(got_counts[mask], want_counts[mask]), "%s: %d pixels' counts differ from the oracle's" % (
        what, int((got_counts != want_counts)[mask].sum()))
    assert np.array_equal(bits(got_ao)[mask], bits(want_ao)[mask]), "%s: ao differs from the oracle's" % what
    g.close()


@pytest.mark.parametrize("material", S.MATERIALS)
def test_live_edits_move_the_sources_onto_the_sheet_and_back(ra, oracle, work, material):
    """From a generic placement to the light on triangle k (set_light) and the camera in its plane (set_camera), and back: after each step
    the frames equal the oracle's of the corresponding scene file and the prune-record copies those of a fresh scene of that file -- a
    copy left over from the earlier source fails here."""
    generic = ("light", "normal", 1.0, material, 1)             # light 0.3 over k, the camera of the light cases, plane normal 0,1,0
    d0 = S.placement(oracle, work, generic)
    s = d0["sheet"]
    on_sheet = dict(light=np.asarray(s.c, f32), cam=np.asarray(s.c + 0.9 * s.tz, f32))
    steps = [("generic", d0["light"], d0["cam"], generic),
             ("light on k", on_sheet["light"], d0["cam"], ("light", "on", 0.0, material, 1)),
             ("light on k, camera in its plane", on_sheet["light"], on_sheet["cam"], None),
             ("generic again", d0["light"], d0["cam"], generic)]
    g = None
    for n, (label, light, cam, case) in enumerate(steps):
        d = dict(d0, light=light, cam=cam)
        path = "%s/live_%s_%d.scene" % (work, material, n)
        with open(path, "w") as f:
            f.write(S.scene_text(s.mesh, cam, light, 1, material))
        if g is None:
            g = ra.Scene(path, S.W, S.H)
            rot = g.camera_pose()[1]
        else:
            g.set_light(0, position=light)
            g.set_camera(cam, rot)
        what = "live %s, step %d (%s)" % (material, n, label)
        check_variant(g, d, what)
        check_frames(g, oracle, path, what)
        fresh = ra.Scene(path, S.W, S.H)
        want = fresh.device_prune_copies(0)
        got = g.device_prune_copies(0)
        fresh.close()
        assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), "%s: %d prune records differ from a fresh scene's" % (
            what, int((bits(got) != bits(want)).any(-1).sum()))
        if case is not None:
            S.check_records(ra, got, g.device_mesh_flat(0)[0], g.device_mesh(0)["refs"], d, case, what)
    g.close()
