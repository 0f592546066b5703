"""CPU: the case list of tests/util_sources.py is what tests/test_gpu_source_margins.py needs it to be -- no case is vacuous, none is missing,
and every placement puts the source where it is meant to: by the oracle's frames and the host's sourceP (rtx_source_p_probe) alone.

decisive(): the pixels whose pass-1 bits differ between the oracle's frame of a case and of the same scene without its mesh; at least 50
for every case.  Measured (128 x 96, the same for the Diffuse and the Phong mesh unless two values are given):

    placement                          culling 1        culling 0
    camera near, H = 0 / 1e-6             843             1295
    camera near, H = 1e-3                 852             1291
    camera near, H = 0.05                1081             1449
    camera near at 1e3, H = 1e-3          852             1291
    camera far, D = 30                    124              124
    camera far, D = 33                     57               57
    light on k, H = 0                    1635             5969
    light on k, H = 1e-4                 1656             5969
    light on k, H = 1e-3                 1841             5969
    light on k, H = 0.05                 1818             5001
    light on k at 1e3, H = 1e-3          1841             5969
    plane normal 1e-3                  461 / 462       1439 / 1440
    plane normal 100                      461             1383
    plane normal 1e4                      461              461
    ground at -40                         463             2391
    light 40 above                        461              461

(Under culling the shadow rays from the ground see the sheet's back, which they skip: 461 is the sheet as the camera of the light cases
sees it.)"""
import numpy as np
import pytest

from tests import util_sources as S


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return str(tmp_path_factory.mktemp("sources"))


@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_every_case_has_decisive_pixels(oracle, work, case):
    path, _ = S.write_case(oracle, work, case)
    n = S.decisive(oracle, path)
    print("%s: %d decisive pixels" % (S.case_id(case), n))
    assert n >= S.DECISIVE_FLOOR, "%s: only %d pixels can show a lost hit of the mesh" % (S.case_id(case), n)


def test_case_list_is_complete():
    """Every placement under either culling, every light placement with either material -- so no selection of tests can shrink it unnoticed."""
    assert {(n, p) for n, p in S.CAMERA_PLACEMENTS} == {("near", 0.0), ("near", 1e-6), ("near", 1e-3), ("near", 0.05), ("far", 30.0), ("far", 33.0),
                                                        ("near@1e3", 1e-3)}
    assert {(n, p) for n, p in S.LIGHT_PLACEMENTS} == {("on", 0.0), ("on", 1e-4), ("on", 1e-3), ("on", 0.05), ("normal", 1e-3), ("normal", 100.0),
                                                       ("normal", 1e4), ("ground-40", 0.3), ("above", 40.0), ("on@1e3", 1e-3)}
    assert len(set(S.CASES)) == len(S.CASES) == 2 * len(S.CAMERA_PLACEMENTS) + 4 * len(S.LIGHT_PLACEMENTS)
    for n, p in S.CAMERA_PLACEMENTS:
        assert {c[4] for c in S.CASES if c[:3] == ("camera", n, p)} == {0, 1}
    for n, p in S.LIGHT_PLACEMENTS:
        assert {(c[3], c[4]) for c in S.CASES if c[:3] == ("light", n, p)} == {(m, c) for m in ("diffuse", "phong") for c in (0, 1)}


def test_the_sheet_is_what_the_placements_assume(oracle, work):
    """The placed box, the normals' side, and a Pgen under the 1 / 216 below which the launch picks the box test by itself -- shared by all
    triangles up to the rounding of the placement (what lets a slot without a certificate be recognised by P >= 0.999 Pgen)."""
    for shifted in (False, True):
        s = S.sheet(oracle, work, shifted)
        assert len(s.tris) == 2048
        assert np.allclose(s.lo - s.shift, [-0.5, -0.50390625, -3.5], atol=1e-4) and np.allclose(s.hi - s.shift, [0.5, -0.49609375, -2.5], atol=1e-4)
        t = s.tris.astype(np.float64)
        n = np.cross(t[:, 3:6] - t[:, 0:3], t[:, 6:9] - t[:, 0:3])
        assert (n[:, 1] > 0).all() or (n[:, 1] < 0).all()
        pg = s.pgen()
        assert pg.max() < 1.0 / 216 and pg.min() > 0.9995 * pg.max()
        assert abs(np.dot(s.n, s.tz)) < 1e-12 and s.tz[2] > 0.9 and s.n[1] > 0.9
        # k near the front-centre: the near cameras stand in front of the sheet, over its middle
        assert abs(s.c[0] - s.shift[0]) < 0.05 and s.hi[2] - s.c[2] < 0.1


def p_of(ra, oracle, work, case, source):
    d = S.placement(oracle, work, case)
    s = d["sheet"]
    if source == "camera":
        return s, S.host_p(ra, s, d["cam"], 0.0, True)
    return s, S.host_p(ra, s, d["light"], S.light_sigma_floor(d["plane_l"]), False)


def test_sources_in_the_plane_of_triangle_k_have_no_certificate_for_it(ra, oracle, work):
    """The camera at H = 0 (as close to k's plane as float32 coordinates come); the light at H = 0 and at H = 1e-4 = bias, where
    H - sigma <= 0."""
    for case, source in ((("camera", "near", 0.0, "diffuse", 1), "camera"), (("light", "on", 0.0, "diffuse", 1), "light"),
                         (("light", "on", 1e-4, "diffuse", 1), "light")):
        s, p = p_of(ra, oracle, work, case, source)
        pg = s.pgen()
        assert not S.certified(p, pg)[s.k], S.case_id(case)
        assert p[s.k] >= np.float32(pg[s.k])
        # ... while the sheet's other triangles mostly keep theirs: the copy is still in use
        assert S.certified(p, pg).mean() > 0.9, S.case_id(case)


def test_sources_off_the_plane_certify_triangle_k(ra, oracle, work):
    for case, source in ((("camera", "near", 0.05, "diffuse", 1), "camera"), (("light", "on", 0.05, "diffuse", 1), "light")):
        s, p = p_of(ra, oracle, work, case, source)
        assert S.certified(p, s.pgen())[s.k], S.case_id(case)
        assert p[s.k] < 0.05 * s.pgen()[s.k]


def test_sources_away_from_the_sheet_certify_most_of_it(ra, oracle, work):
    """As test_source_p_never_exceeds_pgen_and_needs_height has it for random triangles: P under 0.05 Pgen for more than 0.9 of the
    triangles -- the generic source of every case (the light of the camera cases, the camera of the light cases) and the placements that
    stand off the sheet; under plane normals of 1e4 (sigma = 1 over a height of 0.3) nothing is certified."""
    seen = set()
    for case in S.CASES:
        kind, name, par, _, _ = case
        if (kind, name, par) in seen:
            continue
        seen.add((kind, name, par))
        cam_state, light_state = S.copy_states(case)
        for source, state in (("camera", cam_state), ("light", light_state)):
            s, p = p_of(ra, oracle, work, case, source)
            pg = s.pgen()
            assert (p > 0).all() and (p <= pg * (1 + 1e-5) + 1e-36).all()
            if state == "most":
                assert (p < 0.05 * pg).mean() > 0.9, (S.case_id(case), source)
            elif state == "none":
                assert not S.certified(p, pg).any(), (S.case_id(case), source)
            elif state == "k":
                assert not S.certified(p, pg)[s.k], (S.case_id(case), source)
    assert S.copy_states(("light", "normal", 1e4, "diffuse", 1))[1] == "none" and S.copy_states(("camera", "near", 0.0, "diffuse", 0))[0] == "k"


def test_far_cameras_stand_either_side_of_the_fallback(oracle, work):
    """|camera - vertex|_inf of every vertex of the sheet is under kSrcAinfMax = 32 at D = 30 and over it at D = 33: pruneEval8 takes P for
    every record of the one and Pgen for every record of the other."""
    for par, side in ((30.0, -1), (33.0, 1)):
        d = S.placement(oracle, work, ("camera", "far", par, "diffuse", 1))
        a = np.abs(d["sheet"].tris.reshape(-1, 3).astype(np.float64) - d["cam"].astype(np.float64)).max(1)
        assert ((a - S.K_SRC_AINF_MAX) * side > 0.25).all(), (par, a.min(), a.max())


def test_record_check_on_the_host(ra, oracle, work):
    """tests/util_sources.check_records -- the check of the GPU tests -- on copies made by the host alone (mesh_flatten_probe's records with
    every slot's P the max of the host's sourceP below it): it passes them, and fails once one slot's P is lowered or one subtree's maximum
    is left out."""
    for case in (("camera", "near", 0.0, "diffuse", 1), ("light", "on", 1e-4, "phong", 0), ("light", "normal", 1e4, "diffuse", 0),
                 ("light", "normal", 100.0, "diffuse", 1), ("camera", "far", 33.0, "diffuse", 0)):
        path, d = S.write_case(oracle, work, case)
        g = ra.Scene(path, S.W, S.H)
        bvh = g.bvh(1)
        g.close()
        assert np.array_equal(S.bits(bvh["tris"][:, 0:9]), S.bits(d["sheet"].tris)), "the two loaders place the sheet differently"
        copies, wide, refs = S.host_copies(ra, bvh, d)
        shares = S.check_records(ra, copies, wide, refs, d, case, S.case_id(case))
        print("%s: certified share of the non-empty slots: camera %.3f, light %.3f" % (S.case_id(case), shares[0], shares[1]))
        box = copies[:, :, :copies.shape[2] // 2, :]
        w, k = [tuple(x) for x in np.argwhere((box[0][..., 4] >= 0) & (box[1][..., 3] < box[1][..., 7]))][0]
        bad = copies.copy()
        bad[1, w, k, 3] = np.nextafter(bad[1, w, k, 3], np.float32(0))
        with pytest.raises(AssertionError, match="below the host's max"):
            S.check_records(ra, bad, wide, refs, d, case)
        bad = copies.copy()
        bad[1, 0, 0, 7] *= 2
        with pytest.raises(AssertionError, match="differs from copy 0"):
            S.check_records(ra, bad, wide, refs, d, case)
