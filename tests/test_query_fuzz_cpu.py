"""The inputs of tests/test_gpu_query_fuzz.py can tell right from wrong: conditions on the sixteen seeds of tests/util_query_fuzz.py, checked
on the CPU oracle alone.  The generator was tuned until the oracle met them; the numbers stay.  N is decoded from the showNormals colours
here (an ulp or two from hitNormal): good for shares and for "does a fault change the expected bits", which is all that is asked."""
import numpy as np
import pytest

from tests import util_aov as U
from tests import util_light as UL
from tests import util_occlusion as OC
from tests import util_points as UP
from tests import util_query_fuzz as Q
from tests import util_radiance as UR
from tests import util_scatter as SC
from tests import util_shading as S
from tests import util_surface as SU

f32 = np.float32


@pytest.fixture(scope="module")
def cases(oracle, tmp_path_factory):
    """seed -> Case, made when first asked for and shared read-only"""
    d = S.short_dir(tmp_path_factory)
    made = {}

    def get(seed):
        if seed not in made:
            made[seed] = Q.Case(oracle, seed, d)
        return made[seed]
    get.dir = d
    return get


def differ(a, b):
    return a.shape != b.shape or not np.array_equal(U.bits(a), U.bits(b))


def mesh_seeds(cases):
    return [s for s in Q.SEEDS if cases(s).family != "analytic"]


# ---- the generator ------------------------------------------------------------------------------------------------------------------------------
def test_the_same_seed_gives_the_same_scene_and_rays(oracle, cases):
    for seed in (0, 5, 13):
        a = cases(seed)
        b = Q.Case(oracle, seed, cases.dir)
        assert a.text == b.text and (a.w, a.h) == (b.w, b.h)
        for name in ("pool", "free", "free_view", "dirs", "weights"):
            assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), name
        assert (a.rows, a.radius, a.views, a.detour, a.order) == (b.rows, b.radius, b.views, b.detour, b.order)
    assert len({cases(s).text for s in Q.SEEDS}) == len(Q.SEEDS)


def test_what_the_seeds_hold(cases):
    types, meshes, materials, maps, sky, n_lights, light_types, samples, cull, depth, penalty, first = (set() for _ in range(12))
    for seed in Q.SEEDS:
        c = cases(seed)
        assert c.w <= 48 and c.h <= 40 and (c.w % 8 or c.h % 8)
        blocks = c.blocks
        first.add(blocks[0]["type"])
        for b in blocks:
            types.add(b["type"])
            materials.add(SC.material_of(b))
            if b["type"] == "mesh":
                meshes.add(b["name"].split("/")[-1])
                for key in ("diffuse_map", "normal_map", "specular_map"):
                    if key in b:
                        mw, mh, _ = U.load_bmp(b[key])
                        assert mw != mh
                        maps.add(key)
        lights = UL.light_blocks(c.text)
        n_lights.add(len(lights))
        for l in lights:
            light_types.add(l["type"])
            if l["type"] == "area":
                samples.add(int(l["samples"]))
        sky.add("skyboxes=" in c.text)
        cull.add(c.cull); depth.add(int(Q.option(c.text, "max_ray_depth"))); penalty.add(int(Q.option(c.text, "ac_penalty")))
        assert 0 <= int(Q.option(c.text, "max_ray_depth")) <= 6 and 1 <= int(Q.option(c.text, "ac_penalty")) <= 5
    assert types == {"sphere", "plane", "mesh"} and first == types          # (any kind of object comes first somewhere)
    assert meshes == set(Q.MESHES) and materials == {0, 1, 2, 3} and maps == {"diffuse_map", "normal_map", "specular_map"}
    assert sky == {True, False} and n_lights >= {0, 4} and n_lights <= {0, 1, 2, 3, 4} and light_types == {"point", "distant", "area"}
    assert samples == {1, 2, 3} and cull == {0, 1} and len(depth) >= 4 and len(penalty) >= 3
    assert len(UL.light_blocks(cases(Q.NO_LIGHT).text)) == 0


def test_orders(cases):
    orders = [cases(s).order for s in Q.SEEDS]
    for order in orders:
        assert sorted(order) == sorted(Q.CALLS)
        assert all(order.index("surface_rays") < order.index(c) for c in Q.AFTER_SURFACE)
    assert len({tuple(o) for o in orders}) == len(orders)
    # (surface_rays can only come early; every other call is met at many positions)
    assert len({o.index("surface_rays") for o in orders}) >= 3
    assert all(len({o.index(c) for o in orders}) >= 6 for c in Q.CALLS if c != "surface_rays")


# ---- the primary rays meet the scene ------------------------------------------------------------------------------------------------------
def test_hit_and_mesh_shares(cases):
    meshy = 0
    for seed in Q.SEEDS:
        c = cases(seed)
        e = c.frame_aov()
        hit, mesh = e["hit"].mean(), (e["triangle_id"] >= 0).mean()
        print("seed %d (%d x %d, %s): %.3f of the pixels hit, %.3f a mesh" % (seed, c.w, c.h, c.family, hit, mesh))
        assert 0.25 <= hit <= 0.97, "seed %d: %.3f of the primary rays hit" % (seed, hit)
        meshy += mesh >= 0.15
    assert meshy >= 12


def test_kernel_families(cases):
    fam = [cases(s).family for s in Q.SEEDS]
    assert fam.count("analytic") >= 2 and fam.count("plain") >= 3 and fam.count("general") >= 6
    assert all(cases(s).family == "analytic" for s in Q.NO_MESH) and all(cases(s).family == "plain" for s in Q.PLAIN)
    assert {cases(s).cull for s in mesh_seeds(cases)} == {0, 1}
    assert {cases(s).cull for s in Q.SEEDS if cases(s).family == "plain"} == {0, 1}


def test_materials_and_texels(cases):
    first = np.zeros(4, np.int64)
    tex = {"d": 0, "n": 0, "s": 0}
    for seed in Q.SEEDS:
        c = cases(seed)
        mat = c.material()[:c.n_cam]
        first += np.array([(mat == k).sum() for k in range(4)])
        o = c.oracle()
        t = Q.texels(o, c.text, c.surface())
        o.close()
        for k in tex:
            tex[k] += t[k]
    print("first hits by material (Diffuse, Reflective, Transparent, Phong): %s; distinct texels fetched: %s" % (first, tex))
    assert (first >= 2000).all() and all(v >= 200 for v in tex.values())


def test_light_classes(cases):
    """(hit, light, sample) triples of (A) and (B): lit, shadowed while facing the light, turned away (N . -L <= 0)"""
    lit = shadowed = away = 0
    for seed in Q.SEEDS:
        c = cases(seed)
        e, plan, occ = c.pool_light(c.decoded_normals())
        mine = plan.idx < c.n_cam + c.n_bounce
        m, at = len(plan.idx), 0
        for I, L, dist in plan.lights:
            n_s = L.shape[1]
            blocked = occ[at:at + m * n_s].reshape(n_s, m).T[mine] != 0
            at += m * n_s
            facing = UL.max0(UL.dot(np.broadcast_to(plan.N[:, None, :], L.shape), -L))[mine] > 0
            lit += int((facing & ~blocked).sum()); shadowed += int((facing & blocked).sum()); away += int((~facing).sum())
    total = lit + shadowed + away
    print("%d triples: lit %.3f, shadowed %.3f, turned away %.3f" % (total, lit / total, shadowed / total, away / total))
    assert min(lit, shadowed, away) >= 0.10 * total


def test_scatter_classes(cases):
    total = {}
    for seed in Q.SEEDS:
        c = cases(seed)
        N = c.decoded_normals()
        for k, v in SC.class_counts(c.pool, c.scatter(N), c.probe()[0], N, c.material()).items():
            total[k] = total.get(k, 0) + v
    print(total)
    assert set(total) == {"miss", "dp", "mirror", "glass_out", "glass_in", "tir"} and all(v >= SC.MIN_CLASS for v in total.values())


# ---- the expectation is sensitive: a fault changes its bits ----------------------------------------------------------------------------------
def cam_light(c, **fault):
    N = c.decoded_normals()
    return c.light(c.cam, c.probe()[0][:c.n_cam], N[:c.n_cam], **fault)[0]


def light_changes(c, **fault):
    want = c.pool_light(c.decoded_normals())[0]
    got = cam_light(c, **fault)
    return any(differ(got[k], want[k][:c.n_cam]) for k in UL.CHANNELS[1:])


def cpu_points(c):
    return c.points(c.surface()["position"], c.decoded_normals())[0]


def radiance_changes(c, what):
    pts = cpu_points(c)
    col = c.memo("cpu_radiance_colours", lambda: c.radiance_colours(pts))
    want = c.radiance(pts, True, col)
    if what == "cosine":
        got = c.radiance(pts, False, col)
    else:
        got = UR.reduce(col[:, ::-1], pts[:, 3:6], c.dirs[::-1], c.weights[::-1], True)
    return differ(got[0], want[0])


def map_changes(c, monkeypatch):
    # (a faulty index may lie outside the map: it is kept inside, where it still fetches another texel than the right index)
    wrong = lambda size, tx, ty: np.clip(S.map_index(size, tx, ty, fault="wh"), 0, size[0] * size[1] - 1)
    with monkeypatch.context() as m:
        m.setattr(SU, "map_index", wrong)
        o = c.oracle()
        got = SU.expected(o, c.text, c.pool)
        o.close()
    want = c.surface()
    return differ(got["albedo"], want["albedo"]) or differ(got["specular"], want["specular"])


FAULTS = {
    "<= for < at tmax": lambda c, mp: differ(c.occlusion(le=True)[1], c.occlusion()[1]),
    "transparent objects block": lambda c, mp: differ(c.occlusion(transparent_blocks=True)[2], c.occlusion()[2]) or light_changes(c, transparent_blocks=True),
    "bias 0 in the shadow origin": lambda c, mp: light_changes(c, bias=f32(0)),
    "the light sum in reverse order": lambda c, mp: len(c.lights[0]) >= 3 and light_changes(c, reverse=True),
    "the other culling value": lambda c, mp: differ(c.probe(cull=1 - c.cull)[0], c.probe()[0]),
    "map_index with W and H exchanged": lambda c, mp: map_changes(c, mp),
    "cosine dropped in reduce": lambda c, mp: radiance_changes(c, "cosine"),
    "directions reversed in reduce": lambda c, mp: radiance_changes(c, "reversed"),
}


@pytest.mark.parametrize("fault", list(FAULTS))
def test_a_fault_changes_the_expected_bits(cases, monkeypatch, fault):
    seen = [seed for seed in Q.SEEDS if FAULTS[fault](cases(seed), monkeypatch)]
    print("%s: the expectation of seeds %s changes" % (fault, seen))
    assert len(seen) >= 3, "the seeds are blind to \"%s\": only %s see it" % (fault, seen)


# ---- the compositions agree with one another ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 12])
def test_point_calls_at_the_first_hits_are_the_ray_and_frame_calls(cases, seed):
    """light_points at the first hits is light_rays of the primary rays (util_points.PointPlan against util_light.Plan), ao_points there is
    render_ao's pixel, and sky is the probe's colour of a ray that misses"""
    c = cases(seed)
    N = c.decoded_normals()
    pts, view, n_first = c.points(c.surface()["position"], N)
    assert n_first >= 300 and len(pts) == n_first + Q.N_FREE
    o = c.oracle()
    plan = UP.PointPlan(o, c.lights, pts[:n_first], view[:n_first])
    o.close()
    hit2, t2 = c.opaque(plan.shadow_rays)
    got = plan.reduce(OC.expected(hit2, t2, plan.shadow_tmax))
    want = c.point_light(N)
    for k in UP.CHANNELS:
        assert not differ(got[k], want[k][:n_first]), k
    counts, ao = c.point_ao(pts)
    fc, fa = c.frame_ao(N)
    hit = (c.probe()[0][:c.n_cam, 0] > 0).reshape(c.h, c.w)
    mask = U.written_mask(c.w, c.h, c.rows)
    at = np.cumsum(hit.ravel()) - 1                      # (pixel -> its index among the first hits)
    sel = (hit & mask).ravel()
    assert sel.sum() >= 50
    assert np.array_equal(fc.ravel()[sel], counts[at[sel]]) and np.array_equal(U.bits(fa.ravel()[sel]), U.bits(ao[at[sel]]))
    miss = c.probe()[0][:, 0] == 0
    assert miss.sum() >= 100 and np.array_equal(U.bits(c.sky()[miss]), U.bits(c.probe()[1][miss]))
