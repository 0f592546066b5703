"""GPU: rtx_texel_points and rtx_dilate_texels (include/rtx_bake.h) against tests/util_texel_points' numpy restatement, bit
for bit: `tri` exactly, every float as its uint32 view.  The sizes are the smallest that take every path: boxes a lane walks (at most 64
texels), boxes cut into 8 x 8 chunks, both in one mesh, maps that are no multiple of anything, one texel, ties on every texel.  The
restatement's own properties are tests/test_texel_points_cpu.py's.  Nothing here has a tolerance."""
import ctypes as C

import numpy as np
import pytest

from rendering_amd import assets
from tests import util_texel_points as U
from tests.util_deform import bulge

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
bits = U.bits
ERR_ARG = -1


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    d = tmp_path_factory.mktemp("texel_gpu")
    objs = dict(torus86=assets.torus_obj(8, 6), torus84=assets.torus_obj(8, 4), torus6448=assets.torus_obj(64, 48), quad=U.quad_obj(),
                quad_wide=U.quad_obj(-0.5, 1.5), charts=U.charts_obj(), charts_rev=U.charts_obj(reverse=True))
    return {k: U.write_mesh_scene(d, k, v) for k, v in objs.items()}


_refs = {}


def ref(oracle, g, key, w, h):
    """The restatement for scene `key` at w x h, computed once and shared (never modified)."""
    if (key, w, h) not in _refs:
        _refs[key, w, h] = U.texel_points_ref(*U.triangles(g), w, h, oracle.normalize_n)
    return _refs[key, w, h]


def host(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def assert_same(got, want, what):
    assert np.array_equal(got["tri"], want["tri"]), "%s: tri differs at %s" % (what, np.argwhere(got["tri"] != want["tri"])[:4])
    for k in ("points", "bary"):
        bad = bits(got[k]) != bits(want[k])
        assert got[k].shape == want[k].shape and not bad.any(), "%s: %s differs in %d values, first at %s" % (what, k, int(bad.sum()), np.argwhere(bad)[0])


CASES = [("torus86", 37, 21), ("torus86", 16, 12), ("torus86", 8, 6), ("torus86", 1, 1), ("torus84", 8, 4),      # non-multiples, one texel, ties
         ("quad", 1024, 512), ("quad", 65, 63), ("quad_wide", 65, 63), ("quad_wide", 1024, 512),                # the chunk path
         ("torus6448", 16, 16),                                                                                 # the small-box path
         ("charts", 37, 21), ("charts", 64, 64), ("charts", 9, 5)]                                              # both in one mesh


@pytest.mark.parametrize("key,w,h", CASES)
def test_texel_points_equal_the_restatement(ra, oracle, scenes, key, w, h):
    g = ra.Scene(scenes[key], 32, 24)
    want = ref(oracle, g, key, w, h)
    got = host(g.texel_points(0, w, h, bary=True))
    assert got["points"].shape == (h * w, 6) and got["tri"].shape == (h, w) and got["bary"].shape == (h, w, 2)
    assert_same(got, want, "%s %dx%d" % (key, w, h))
    if key.startswith("torus") or key == "quad":
        assert (got["tri"] >= 0).all()
    g.close()


def test_ownership_rules(ra, oracle, scenes):
    w, h = 37, 21
    g = ra.Scene(scenes["charts"], 32, 24)
    tri_uv = U.triangles(g)[2]
    got = host(g.texel_points(0, w, h, bary=True))
    g.close()
    tri = got["tri"]
    cx, cy = np.meshgrid(U.centres(w), U.centres(h))
    cov = [U.covers(*U.weights(tri_uv[t], cx, cy)) if not np.isnan(tri_uv[t]).any() else np.zeros((h, w), bool) for t in range(8)]
    # the overlap of charts 0 and 1 is owned by 0, the rest of 1 by 1; the mirrored chart, whose D is negative, owns all it covers
    both = cov[0] & cov[1]
    assert both.any() and (tri[both] == 0).all() and (tri[cov[1] & ~cov[0]] == 1).all() and (cov[1] & ~cov[0]).any()
    assert (U.weights(tri_uv[2], cx, cy)[3] < 0).all() and cov[2].any() and (tri[cov[2]] == 2).all()
    # the degenerate triangle, the one outside the map and the one with a NaN coordinate own nothing; nor does the collinear one (D == 0 here)
    assert not np.isin(tri, U.CHART_NEVER + (4,)).any() and not cov[3].any() and not cov[4].any() and not cov[5].any()
    assert (tri[cov[7]] == 7).all() and cov[7].any()
    none = ~np.any(cov, axis=0)
    assert none.any() and (tri[none] == -1).all() and (tri[~none] >= 0).all()
    assert not bits(got["points"].reshape(h, w, 6)[none]).any() and not bits(got["bary"][none]).any()
    # the faces listed in reverse order: triangle t is 7 - t, and outside the overlap every texel has the same point
    r = ra.Scene(scenes["charts_rev"], 32, 24)
    rev = host(r.texel_points(0, w, h))
    r.close()
    once = ~both
    assert np.array_equal(np.where(rev["tri"] >= 0, 7 - rev["tri"], -1)[once], tri[once]) and (rev["tri"][both] == 7 - 1).all()
    assert np.array_equal(bits(rev["points"].reshape(h, w, 6)[once]), bits(got["points"].reshape(h, w, 6)[once]))


def test_each_output_alone_canaries_and_repeats(ra, oracle, scenes):
    w, h = 37, 21
    g = ra.Scene(scenes["charts"], 32, 24)
    full = host(g.texel_points(0, w, h, bary=True))
    again = host(g.texel_points(0, w, h, bary=True))
    assert_same(again, full, "a second call")
    for k in ("points", "tri", "bary"):
        one = host(g.texel_points(0, w, h, points=k == "points", tri=k == "tri", bary=k == "bary"))
        assert list(one) == [k] and np.array_equal(one[k].view(np.uint32), full[k].view(np.uint32)), k
    # canaries behind each buffer, through the C entry itself; the buffers start at odd word offsets (no 8- or 16-byte alignment)
    rtx, _ = ra.load()
    n, pad = w * h, 67
    P = torch.full((1 + n * 6 + pad,), 7.5, dtype=torch.float32, device="cuda")
    T = torch.full((1 + n + pad,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    B = torch.full((1 + n * 2 + pad,), -3.25, dtype=torch.float32, device="cuda")
    buf = ra.TexelBuffers(P.data_ptr() + 4, T.data_ptr() + 4, B.data_ptr() + 4)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert rtx.rtx_texel_points(g.gpu(), 0, w, h, C.byref(buf), st) == 0
    torch.cuda.synchronize()
    P, T, B = P.cpu().numpy(), T.cpu().numpy(), B.cpu().numpy()
    assert P[0] == 7.5 and (P[1 + n * 6:] == 7.5).all() and T[0] == 0x5a5a5a5a and (T[1 + n:] == 0x5a5a5a5a).all()
    assert B[0] == -3.25 and (B[1 + n * 2:] == -3.25).all()
    assert np.array_equal(bits(P[1:1 + n * 6]), bits(full["points"]).ravel()) and np.array_equal(T[1:1 + n], full["tri"].ravel())
    assert np.array_equal(bits(B[1:1 + n * 2]), bits(full["bary"]).ravel())
    g.close()


def test_points_follow_a_deformation(ra, oracle, scenes):
    w, h = 37, 21
    g = ra.Scene(scenes["torus86"], 32, 24)
    before = host(g.texel_points(0, w, h, bary=True))
    P0, _ = g.mesh_vertices(0)
    g.set_vertices(0, torch.from_numpy(bulge(P0, 0.2, 2.0)).cuda())
    want = U.texel_points_ref(*U.triangles(g), w, h, oracle.normalize_n)
    got = host(g.texel_points(0, w, h, bary=True))
    assert_same(got, want, "after set_vertices")
    assert np.array_equal(got["tri"], before["tri"]) and np.array_equal(bits(got["bary"]), bits(before["bary"]))
    assert (bits(got["points"][:, :3]) != bits(before["points"][:, :3])).any()
    g.close()


def test_points_follow_the_object_list(ra, oracle, scenes):
    """rtx_scene_set_objects: a kept mesh's triangles move with it to its new index, a new mesh brings its own, a removed one leaves."""
    w, h = 16, 12
    g = ra.Scene(scenes["torus86"], 32, 24)
    first = host(g.texel_points(0, w, h, bary=True))
    new = dict(pos=(1.2, 0.2, -2.6), size=(1.5, 1.2, 1.0), rot=(60, 0, 20), color=(1, 1, 1), name=scenes["charts"].replace(".scene", ".obj"))
    assert g.add_object("mesh", 0, **new) == 0          # (before the torus, which is object and mesh 1 now)
    assert_same(host(g.texel_points(1, w, h, bary=True)), first, "the kept mesh at its new index")
    for idx in (0, 1):
        want = U.texel_points_ref(*U.triangles(g, idx), w, h, oracle.normalize_n)
        assert_same(host(g.texel_points(idx, w, h, bary=True)), want, "object %d after add_object" % idx)
    g.set_vertices(1, torch.from_numpy(bulge(g.mesh_vertices(1)[0], 0.1, 3.0)).cuda())
    for idx in (0, 1):
        want = U.texel_points_ref(*U.triangles(g, idx), w, h, oracle.normalize_n)
        assert_same(host(g.texel_points(idx, w, h, bary=True)), want, "object %d after the other's deformation" % idx)
    g.remove_object(0)
    want = U.texel_points_ref(*U.triangles(g, 0), w, h, oracle.normalize_n)
    assert_same(host(g.texel_points(0, w, h, bary=True)), want, "after remove_object")
    g.close()


def test_the_chain_back_into_the_map(ra, oracle, scenes):
    w, h = 37, 21
    g = ra.Scene(scenes["charts"], 32, 24)
    want = ref(oracle, g, "charts", w, h)
    t = g.texel_points(0, w, h)
    lit = g.light_points(t["points"], diffuse=True)["diffuse"]
    lit_ref = g.light_points(torch.from_numpy(want["points"]).cuda(), diffuse=True)["diffuse"]
    torch.cuda.synchronize()
    assert np.array_equal(bits(lit.cpu().numpy()), bits(lit_ref.cpu().numpy()))
    covered = want["tri"].ravel() >= 0
    assert lit.cpu().numpy()[covered].any() and not bits(lit.cpu().numpy()[~covered]).any()      # (a zero normal yields +0 light)
    for margin in (0, 2):
        image, tri = g.bake_light(0, w, h, margin=margin)
        hand = g.dilate_texels(lit.reshape(h, w, 3).clone(), t["tri"].clone(), margin)
        hand_tri = U.dilate_ref(np.zeros((h, w), np.float32), want["tri"], margin)[1]
        torch.cuda.synchronize()
        assert image.shape == (h, w, 3) and np.array_equal(bits(image.cpu().numpy()), bits(hand.cpu().numpy()))
        assert np.array_equal(tri.cpu().numpy(), hand_tri)
    g.set_texture(0, "diffuse", image)
    back = g.texture(0, "diffuse")
    assert back.is_cuda and np.array_equal(bits(back.cpu().numpy()), bits(image.cpu().numpy()))
    # the size now defaults to the map's
    assert g.texel_points(0, points=False)["tri"].shape == (h, w)
    fb = torch.zeros((24, 32, 3), dtype=torch.float32, device="cuda")
    g.render_pass1(fb)
    torch.cuda.synchronize()
    assert np.isfinite(fb.cpu().numpy()).all()
    g.close()


@pytest.mark.parametrize("channels", [1, 3])
def test_dilation_equals_the_restatement(ra, oracle, scenes, channels):
    w, h = 37, 21
    g = ra.Scene(scenes["charts"], 32, 24)
    tri0 = ref(oracle, g, "charts", w, h)["tri"]
    rng = np.random.RandomState(11)
    img0 = rng.uniform(-4, 4, (h, w, channels)).astype(np.float32)
    img0.view(np.uint32)[0, 0, 0] = 0x7fc12345      # (a copy keeps a NaN's payload)
    if channels == 1:
        img0 = img0[..., 0]
    for passes in (0, 1, 3):
        want_img, want_tri = U.dilate_ref(img0, tri0, passes)
        img, tri = torch.from_numpy(img0).cuda(), torch.from_numpy(tri0).cuda()
        assert g.dilate_texels(img, tri, passes) is img
        torch.cuda.synchronize()
        assert np.array_equal(tri.cpu().numpy(), want_tri) and np.array_equal(bits(img.cpu().numpy()), bits(want_img)), "passes %d" % passes
        assert ((want_tri == -2).sum() > 0) == (passes > 0)
    g.close()


def test_refusals_leave_the_buffers_alone(ra, scenes):
    rtx, _ = ra.load()
    g = ra.Scene(scenes["quad"], 32, 24)
    sc = g.gpu()
    P = torch.full((16 * 6,), 7.5, dtype=torch.float32, device="cuda")
    T = torch.full((16,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    B = torch.full((16 * 2,), -3.25, dtype=torch.float32, device="cuda")
    buf = ra.TexelBuffers(P.data_ptr(), T.data_ptr(), B.data_ptr())
    none = ra.TexelBuffers(None, None, None)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert rtx.rtx_texel_points(None, 0, 4, 4, C.byref(buf), st) == ERR_ARG
    assert rtx.rtx_texel_points(sc, 0, 4, 4, None, st) == ERR_ARG
    assert rtx.rtx_texel_points(sc, 0, 4, 4, C.byref(none), st) == ERR_ARG
    assert rtx.rtx_texel_points(sc, 1, 4, 4, C.byref(buf), st) == ERR_ARG
    assert rtx.rtx_texel_points(sc, 0, 0, 4, C.byref(buf), st) == ERR_ARG
    assert rtx.rtx_texel_points(sc, 0, 4, 0, C.byref(buf), st) == ERR_ARG
    assert rtx.rtx_texel_points(sc, 0, 1 << 16, 1 << 15, C.byref(buf), st) == ERR_ARG
    img, tri = P, T
    assert rtx.rtx_dilate_texels(None, 4, 4, 3, img.data_ptr(), tri.data_ptr(), 1, st) == ERR_ARG
    assert rtx.rtx_dilate_texels(sc, 4, 4, 3, None, tri.data_ptr(), 1, st) == ERR_ARG
    assert rtx.rtx_dilate_texels(sc, 4, 4, 3, img.data_ptr(), None, 1, st) == ERR_ARG
    assert rtx.rtx_dilate_texels(sc, 4, 4, 0, img.data_ptr(), tri.data_ptr(), 1, st) == ERR_ARG
    assert rtx.rtx_dilate_texels(sc, 4, 4, 5, img.data_ptr(), tri.data_ptr(), 1, st) == ERR_ARG
    assert rtx.rtx_dilate_texels(sc, 0, 4, 3, img.data_ptr(), tri.data_ptr(), 1, st) == ERR_ARG
    assert rtx.rtx_dilate_texels(sc, 4, 0, 3, img.data_ptr(), tri.data_ptr(), 1, st) == ERR_ARG
    # passes == 0 does nothing, and succeeds
    assert rtx.rtx_dilate_texels(sc, 4, 4, 3, img.data_ptr(), tri.data_ptr(), 0, st) == 0
    torch.cuda.synchronize()
    assert (P.cpu().numpy() == 7.5).all() and (T.cpu().numpy() == 0x5a5a5a5a).all() and (B.cpu().numpy() == -3.25).all()
    before = g.scene_bytes()
    g.texel_points(0, 8, 8)
    assert g.scene_bytes() == before, "the scratch is not scene data"
    g.close()
