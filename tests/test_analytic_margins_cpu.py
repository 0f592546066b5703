"""The rays of tests/util_analytic.py on the CPU: the oracle against the real reference, the digests of the reference's records, the numpy
restatement against the oracle, and that the families ARE at the margins they are aimed at (conditions, not tolerances).

Two results are equal when their bits are equal or both are NaN; signs of zero count.

  1. Where oracle/_ref exists the oracle equals the reference on every form: the hit records and colours of every family, pass 1 and the
     SSAA frame.  Everywhere, the oracle's digests equal tests/golden/analytic_margins.json (tools/make_golden_analytic.py: the reference's).
     Every form loads in the reference's loader, the oracle's and the host loader; none was dropped.
  2. restate() equals the oracle's records on every family of every form (0 of 195 000 rays differ), so its per-object verdicts are the
     oracle's.  Measured on them (the floors asserted are in the tests):
       limb       per sphere with r >= 0.1: the test says hit for 25-34 % and miss for the rest (every second ray has the sphere behind it);
                  d2 == r2 exactly for 14.7-29.3 % (r = 1e19: 7.8 % -- |c| absorbs the origin, so tca tca must round to one particular float;
                  r = 1e-3: 0 %, exempt: its d2 quantum is as large as r2; r = 1e20 has no limb rays and so no share: r2 = inf, no d2 exceeds
                  it, and the construction needs |L| > r -- its rays are the other families', which all pass it with the camera inside)
       inside_on  of the surface origins 47-78 % take t0 < 0 -> t1; 549-621 rays per form are accepted at t == +-0 (extremes: 277)
       denom      per plane 55-60 % rejected, 40-45 % pass; 132-256 rays per plane get another verdict from a float comparison with 1e-8f
       on_plane   per plane 100-256 accepted hits at t = -0 and 112-256 at t = +0
       far        accepted t from 1.5e6 to 8e30 (extremes is left out of this range check, not of the comparisons: the sphere around its
                  camera and the two giant ones answer many of these rays first)
       sheet      with_mesh_cull and with_mesh_nocull share their rays; culling changes 47 % of the records of the rays aimed at the sheet
       tie        exchanging the two objects names the other object on 100 % of the tie rays of every tie scene, with equal t bits
                  (79 distinct rays through the tangent point and 255 at the quad tie exactly; coincident spheres and planes tie always)
       frames     pass 1 differs from the form without its spheres and planes in 310-1457 of 1536 pixels
  3. Each deliberate mistake, applied to restate() only, changes the records of (largest share over the families):
       d2 with one rounding 72 % (tie_spheres tie; limb 15-32 %) | d2 >= r2 12.7 % (spheres limb) | t0 <= 0 4.6 % (materials inside_on) |
       t0 > 0 for planes 26.7 % (extremes on_plane) | threshold in float 3.1 % (with_mesh_cull denom) | last of equal t wins 100 % (tie) |
       spheres and planes before meshes 100 % (tie_quad_ab tie: the quad is first in scene order)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import util_analytic as UA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref", "libref_harness.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "analytic_margins.json")
f32 = np.float32

CHILD = r"""
import sys, numpy as np
sys.path.insert(0, %r)
from oracle import oracle as O
from tools import ref_harness as R
from tests import util_analytic as UA
form, work = sys.argv[1], sys.argv[2]
fams = UA.families(form, O, work)
ref = UA.results(R.RefScene, form, work, fams)
orc = UA.results(O.OracleScene, form, work, fams)
assert sorted(ref) == sorted(orc)
bad = {"%%s/%%s" %% k: int((~UA.same_bits(ref[k], orc[k])).sum()) for k in ref if not UA.same_bits(ref[k], orc[k]).all()}
assert not bad, bad
print('OK', sum(len(f.rays) for f in fams.values()))
"""


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return str(tmp_path_factory.mktemp("analytic_margins"))


_results = {}


def oracle_results(oracle, form, work):
    """results() of the oracle, once per form; read-only"""
    if form not in _results:
        r = UA.results(oracle.OracleScene, form, work, UA.families(form, oracle, work))
        for v in r.values():
            v.setflags(write=False)
        _results[form] = r
    return _results[form]


def records_of(res, family):
    h = res[(family, "hits")]
    return h[:, 0] > 0, h[:, 1].astype(np.int32), h[:, 3]


_mesh_records, _restated = {}, {}


def restated(oracle, form, work, family, mistake=None):
    """restate() of a family, once per (form, family, mistake); the mesh's records once per (form, family)"""
    key = (form, family, mistake)
    if key not in _restated:
        rays = UA.families(form, oracle, work)[family].rays
        if UA.has_mesh(form) and key[:2] not in _mesh_records:
            _mesh_records[key[:2]] = UA.mesh_records(oracle, form, work, rays)
        _restated[key] = UA.restate(form, rays, _mesh_records.get(key[:2]), mistake)
    return _restated[key]


# ---- 1. the oracle, the reference and the loaders ---------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(REF), reason="oracle/_ref not built (the reference is not on this machine)")
@pytest.mark.parametrize("form", UA.FORMS)
def test_oracle_equals_the_reference(form, work):
    # one form per process: the reference keeps process-global option flags
    out = subprocess.run([sys.executable, "-c", CHILD % ROOT, form, work], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


@pytest.mark.parametrize("form", UA.FORMS)
def test_oracle_equals_the_digests_of_the_reference(oracle, form, work):
    gold = json.load(open(GOLDEN))
    assert sorted(gold["sha256"]) == sorted(UA.FORMS)
    got = UA.digests(oracle_results(oracle, form, work))
    assert sorted(got) == sorted(gold["sha256"][form])
    bad = [k for k in got if got[k] != gold["sha256"][form][k]]
    assert not bad, "%s: the oracle's %s differ from the reference's records" % (form, bad)
    assert gold["rays"][form] == sum(len(f.rays) for f in UA.families(form, oracle, work).values())


@pytest.mark.parametrize("form", UA.FORMS)
def test_every_loader_takes_the_form(ra, oracle, form, work):
    """The oracle's loader and the host loader hold the form's objects as the form lists them (the reference's: the digests)."""
    objs = UA.objects_of(form)
    path = UA.write_scene(form, work)
    o = oracle.OracleScene(path)
    g = ra.Scene(path)
    assert (o.width, o.height, o.n_objects, o.n_lights) == (UA.W, UA.H, len(objs), 2) == (g.width, g.height, g.n_objects, g.n_lights)
    held = set(UA.bits(g.digest()).tolist())
    for b in objs:
        want = list(b["pos"]) + ([UA.radius2(b["r"])] if b["type"] == "sphere" else list(b["normal"]) if b["type"] == "plane" else [])
        missing = [x for x in want if int(f32(x).view(np.uint32)) not in held]
        assert not missing, "%s: the host loader does not hold %s of %s" % (form, missing, b)
    o.close(); g.close()


# ---- 2. the restatement is the oracle's, and the families are decisive -------------------------------------------------------------------
@pytest.mark.parametrize("form", UA.FORMS)
def test_restatement_equals_the_oracle_and_families_are_decisive(oracle, form, work):
    res = oracle_results(oracle, form, work)
    fams = UA.families(form, oracle, work)
    objs = UA.objects_of(form)
    total = sum(len(f.rays) for f in fams.values())
    assert 2500 <= total <= 36000 and (form.startswith("tie_") or total >= 20000), total
    for name, fam in fams.items():
        bad = UA.differs(restated(oracle, form, work, name), records_of(res, name))
        assert not bad.any(), "%s %s: restate() differs from the oracle on %d rays, first %s" % (form, name, bad.sum(), fam.rays[np.argmax(bad)])
    report = []
    for name in ("limb", "inside_on", "denom", "on_plane"):
        if name not in fams:
            continue
        fam = fams[name]
        hit, obj, tn = records_of(res, name)
        zeros = 0
        for k in np.unique(fam.target):
            sel = fam.target == k
            o, d, b = fam.rays[sel, 0:3], fam.rays[sel, 3:6], objs[k]
            if b["type"] == "sphere":
                ok, t, det = UA.sphere_test(o, d, np.asarray(b["pos"], f32), UA.radius2(b["r"]), detail=True)
                if name == "limb" and b["r"] >= 0.1:
                    report.append(("limb", k, b["r"], ok.mean(), det["exact"].mean()))
                    assert ok.mean() >= 0.2 and (~ok).mean() >= 0.2, (form, b, ok.mean())
                    assert det["exact"].mean() >= 0.05, (form, b, det["exact"].mean())
                if name == "inside_on":
                    surf = np.char.startswith(fam.sub[sel], "surface")
                    assert surf.sum() >= 512
                    report.append(("surface", k, b["r"], det["second"][surf].mean()))
                    assert det["second"][surf].mean() >= 0.25, (form, b, det["second"][surf].mean())
                    zeros += int((ok & (t == 0) & (obj[sel] == k) & UA.same_bits(tn[sel], t)).sum())
            else:
                ok, t, det = UA.plane_test(o, d, np.asarray(b["pos"], f32), np.asarray(b["normal"], f32), detail=True)
                if name == "denom":
                    report.append(("denom", k, b["normal"], det["rejected"].mean(), int(det["float_differs"].sum())))
                    assert det["rejected"].mean() >= 0.25 and (~det["rejected"]).mean() >= 0.25, (form, b)
                    assert det["float_differs"].sum() >= 100, (form, b, det["float_differs"].sum())
                if name == "on_plane":
                    mine = hit[sel] & (obj[sel] == k)
                    neg, pos = int((mine & (UA.bits(tn[sel]) == 0x80000000)).sum()), int((mine & (UA.bits(tn[sel]) == 0)).sum())
                    report.append(("on_plane", k, neg, pos))
                    assert neg >= 50 and pos >= 50, (form, b, neg, pos)
        if name == "inside_on":
            report.append(("t == +-0", zeros))
            assert zeros >= 100, (form, zeros)            # (accepted, and the record's nearest hit)
    if "far" in fams and form != "extremes":      # (in extremes the sphere around the camera and the two giant ones take many of these rays)
        hit, obj, tn = records_of(res, "far")
        planes = np.array([b["type"] == "plane" for b in objs])
        t = tn[hit & planes[np.maximum(obj, 0)]]
        report.append(("far", float(t.min()), float(t.max())))
        filled = sum(bool(((t >= 10.0 ** e) & (t < 10.0 ** (e + 2))).any()) for e in range(8, 30, 2))
        assert t.min() < 1e9 and t.max() > 1e30 and filled >= 8, (t.min(), t.max(), filled)      # (of 11 windows of two decades)
    print(form, total, report)


@pytest.mark.parametrize("ab,ba", UA.TIE_PAIRS)
def test_exchanging_the_objects_of_a_tie_names_the_other_object(oracle, ab, ba, work):
    """The strict t0 < tNear: the first object in scene order wins a tie.  With the two objects exchanged the record's index stays (the first)
    and therefore names the OTHER object, at the same t."""
    fa, fb = UA.families(ab, oracle, work)["tie"], UA.families(ba, oracle, work)["tie"]
    assert np.array_equal(UA.bits(fa.rays), UA.bits(fb.rays)) and len(fa.rays) >= 512
    ha, ia, ta = records_of(oracle_results(oracle, ab, work), "tie")
    hb, ib, tb = records_of(oracle_results(oracle, ba, work), "tie")
    other = ha & hb & (ia == 0) & (ib == 0)              # object 0 of ab is object 1 of ba
    assert other.mean() >= 0.9, (ab, other.mean())
    assert UA.same_bits(ta[other], tb[other]).all()
    # ... and the CPU check of the tie itself: alone, either object is met at these bits
    objs = UA.objects_of(ab)
    for k in (0, 1):
        o = oracle.OracleScene(UA.write_scene(ab, work, only=(k,), tag="_only%d" % k), UA.W, UA.H)
        h, _ = o.probe(fa.rays, colours=False)
        o.close()
        assert ((h[:, 0] > 0) & UA.same_bits(h[:, 3], ta))[other].all(), (ab, k)
    assert len(objs) == 2


def test_culling_decides_records_of_the_mesh_forms(oracle, work):
    """with_mesh_cull and with_mesh_nocull take the same rays, and the flag can be told on them: of the sheet family, aimed at the mesh from
    both sides, at least a fifth of the records differ (measured: 47 %; the rays from behind pass the culled sheet), and no record differs on
    a ray that neither form's mesh answers."""
    fa, fb = UA.families("with_mesh_cull", oracle, work), UA.families("with_mesh_nocull", oracle, work)
    assert list(fa) == list(fb) and all(np.array_equal(UA.bits(fa[k].rays), UA.bits(fb[k].rays)) for k in fa)
    ra, rb = oracle_results(oracle, "with_mesh_cull", work), oracle_results(oracle, "with_mesh_nocull", work)
    mesh = [UA.is_mesh(b) for b in UA.objects_of("with_mesh_cull")].index(True)
    for name in fa:
        a, b = records_of(ra, name), records_of(rb, name)
        d = UA.differs(a, b)
        assert not (d & (a[1] != mesh) & (b[1] != mesh)).any(), name
        if name == "sheet":
            print("sheet", d.mean(), (a[1] == mesh).mean(), (b[1] == mesh).mean())
            assert d.mean() >= 0.2 and (a[1] == mesh).mean() >= 0.2, (d.mean(), (a[1] == mesh).mean())


@pytest.mark.parametrize("form", UA.FORMS)
def test_the_frame_shows_the_spheres_and_planes(oracle, form, work):
    """Pass 1 of every form differs from the same form without its spheres and planes in at least 50 pixels."""
    o = oracle.OracleScene(UA.write_scene(form, work, keep=UA.is_mesh, tag="_no_analytic"), UA.W, UA.H)
    bare = o.pass1()
    o.close()
    n = int((~UA.same_bits(bare, oracle_results(oracle, form, work)[("frame", "pass1")])).any(-1).sum())
    print(form, n)
    assert n >= 50, (form, n)


# ---- 3. the inputs can tell right from wrong -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mistake", UA.MISTAKES)
def test_a_deliberate_mistake_changes_the_records(oracle, mistake, work):
    """Each mistake, made in restate() only, changes the records of at least 1 % of some family."""
    best = (0.0, "", "")
    for form in UA.FORMS:
        for name in UA.families(form, oracle, work):
            share = float(UA.differs(restated(oracle, form, work, name), restated(oracle, form, work, name, mistake)).mean())
            best = max(best, (share, form, name))
    print(mistake, best)
    assert best[0] >= 0.01, (mistake, best)
