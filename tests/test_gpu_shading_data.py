"""GPU: the shading DATA path -- texture, normal and specular maps, the skybox -- through every mesh kernel, on the scene family of
tests/util_shading.py: maps that are not square, not powers of two, as narrow as 4 texels, the three maps of a mesh in three sizes, two to four
textured tori per scene (Diffuse = the PLAIN kernels, Phong, reflective, transparent), 96 x 40 skybox faces.  Everything bit for bit against the
oracle, which tests/test_shading_data_cpu.py pins to the real reference on the same scenes; that file also shows that these inputs can see an
exchanged width / height, a wrong row stride, another map's size, exchanged sky faces and the tie order of the sky lookup."""
import os

import numpy as np
import pytest

from tests import util_shading as S
from tests.util_move import edit_scene
from tests.util_occlusion import expected, opaque_probe, tmax_mix

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
W, H = S.W, S.H


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def family(tmp_path_factory):
    d = S.short_dir(tmp_path_factory)
    return d, S.write_family(d)


def variant_path(family, name, **extra):
    """The family's scene `name` with extra options (they win over the file's), written beside it."""
    if not extra:
        return family[1][name]
    path = os.path.join(family[0], "%s__%s.scene" % (name, "_".join("%s%s" % kv for kv in sorted(extra.items()))))
    if not os.path.exists(path):
        with open(path, "w") as f:
            f.write(S.scene_text(name, family[0], extra))
    return path


def ray_sets(name):
    sets = {"shading": S.shading_rays(2048), "sky": S.sky_rays()}
    if name in S.MIRROR_SCENES:
        sets["mirror"] = S.mirror_rays()
    return sets


_oracle = {}


def reference(oracle, path, name):
    """The oracle's pass 1, frame, mask and ray records of a scene file (once per file)."""
    if path not in _oracle:
        o = oracle.OracleScene(path, W, H)
        p1 = o.pass1()
        sobel = o.sobel(p1)
        mask = sobel.copy()
        mask[0, :] = 0; mask[-1, :] = 0; mask[:, 0] = 0; mask[:, -1] = 0       # (border = 0 by definition)
        _oracle[path] = dict(pass1=p1, frame=o.ssaa(p1, sobel), mask=mask, rays={k: (r,) + o.probe(r) for k, r in ray_sets(name).items()})
        o.close()
    return _oracle[path]


def assert_frame(got, want, what):
    nd = int((bits(got) != bits(want)).any(-1).sum())
    assert nd == 0, "%s: %d pixels differ from the oracle, first at %s" % (what, nd, np.argwhere((bits(got) != bits(want)).any(-1))[0])


def assert_rays(rays, gh, gc, rh, rc, what):
    bad = np.zeros(len(rays), bool)
    if gh is not None:
        bad |= (bits(rh) != bits(gh)).any(1)
    if gc is not None:
        bad |= (bits(rc) != bits(gc)).any(1)
    i = int(np.argmax(bad))
    assert not bad.any(), "%s: %d of %d rays differ, first %d: ray %s oracle %s %s gpu %s %s" % (
        what, int(bad.sum()), len(rays), i, rays[i], rh[i], rc[i], None if gh is None else gh[i], None if gc is None else gc[i])


def check_frames(g, ref, what):
    """The frame in one launch (cold, then warm: slow tiles split) and in three, with the mask."""
    for mode in (1, 1, 0):
        fb = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
        mask = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
        g.set_frame_mode(mode)
        g.render_frame(fb, mask)
        assert g.frame_status() == 0 and g.frame_mode()[0] == mode
        label = "%s in %s" % (what, "one launch" if mode else "three launches")
        assert_frame(fb.cpu().numpy(), ref["frame"], label)
        assert np.array_equal(mask.cpu().numpy() != 0, ref["mask"] != 0), label + ": mask differs"


def check_trace(g, ref, what, outputs=((True, True),)):
    for key, (rays, rh, rc) in ref["rays"].items():
        t = torch.from_numpy(rays).cuda()
        for hits, colours in outputs:
            gh, gc = g.trace_rays(t, hits=hits, colours=colours)
            torch.cuda.synchronize()
            assert (gh is None) == (not hits) and (gc is None) == (not colours)
            assert_rays(rays, None if gh is None else gh.cpu().numpy(), None if gc is None else gc.cpu().numpy(), rh, rc, "%s, %s rays" % (what, key))


# ---- frames -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(S.FAMILY))
def test_frames(ra, oracle, family, name):
    path = family[1][name]
    ref = reference(oracle, path, name)
    g = ra.Scene(path, W, H)
    assert bool(g.view_flags() & 2) == S.FAMILY[name]["sky"]
    assert_frame(g.render_host(ssaa=False), ref["pass1"], name + " pass 1")
    assert_frame(g.render_host(ssaa=True), ref["frame"], name + " with the 4-sample pass")
    check_frames(g, ref, name)
    g.close()


# ---- the variant matrix with shading data ---------------------------------------------------------------------------------------------------
# (PLAIN, BOXES, CULL) as in tests/test_gpu_margins.py, on the PLAIN scene with all three maps and on its Phong twin: pass 1, the 4-sample pass,
# the single-launch frame and the colour kernel per (PLAIN, BOXES, CULL), the hit kernel per (BOXES, CULL).
MATRIX = [(plain, boxes, cull) for plain in (1, 0) for boxes in (0, 1) for cull in (1, 0)]


@pytest.mark.parametrize("plain,boxes,cull", MATRIX)
def test_variant_matrix_with_shading_data(ra, oracle, family, plain, boxes, cull):
    name = "plain_nrm" if plain else "phong_nrm"
    path = family[1][name] if cull else variant_path(family, name, useBackfaceCulling=0)       # (culling is on unless the file says otherwise)
    ref = reference(oracle, path, name)
    g = ra.Scene(path, W, H)
    g.set_knob("prune_boxes", boxes)
    g.set_knob("trace_reorder", 0)
    v = g.kernel_variant()
    assert (v["plain"], v["boxes"], v["cull"], v["analytic"], v["stats"]) == (bool(plain), bool(boxes), bool(cull), False, False), v
    check_trace(g, ref, "%s boxes %d cull %d" % (name, boxes, cull))
    check_frames(g, ref, "%s boxes %d cull %d" % (name, boxes, cull))
    assert g.kernel_variant() == v
    g.close()


def test_variant_matrix_is_complete():
    assert set(MATRIX) == {(p, b, c) for p in (0, 1) for b in (0, 1) for c in (0, 1)} and len(MATRIX) == 8


def test_analytic_variant_with_a_non_square_skybox(ra, oracle, family):
    path = family[1]["analytic"]
    ref = reference(oracle, path, "analytic")
    g = ra.Scene(path, W, H)
    v = g.kernel_variant()
    assert v["analytic"] and not v["stats"], v
    check_trace(g, ref, "analytic", outputs=((True, True), (True, False), (False, True)))
    check_frames(g, ref, "analytic")
    g.close()


# ---- rays -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(S.FAMILY))
def test_rays(ra, oracle, family, tmp_path, name):
    """cast_rays and trace_rays (in ray order and reordered; hits only, colours only, both) on the re-aimed probe rays, on sky_directions() from
    outside every object and -- where there is a mirror -- from in front of it; occluded() on the same rays equals its CPU reference: maps and
    skybox change no occlusion answer."""
    path = family[1][name]
    ref = reference(oracle, path, name)
    g = ra.Scene(path, W, H)
    for key, (rays, rh, rc) in ref["rays"].items():
        gh, gc = g.cast_rays(rays)
        assert_rays(rays, gh, gc, rh, rc, "%s cast_rays, %s rays" % (name, key))
    for reorder in (0, 1):
        g.set_knob("trace_reorder", reorder)
        check_trace(g, ref, "%s reorder %d" % (name, reorder), outputs=((True, True), (True, False), (False, True)))
    if "meshes" in S.FAMILY[name]:                  # (no plane in the way: the sky directions reach the sky, or the background)
        assert (ref["rays"]["sky"][1][:, 0] == 0).mean() > 0.9
    for key, (rays, rh, rc) in ref["rays"].items():
        hit, t = opaque_probe(oracle, path, tmp_path, rays, size=48)
        t_dev = torch.from_numpy(rays).cuda()
        for tmax in (None, tmax_mix(hit, t)):
            got = g.occluded(t_dev, None if tmax is None else torch.from_numpy(tmax).cuda())
            torch.cuda.synchronize()
            want = expected(hit, t, np.float32(np.inf) if tmax is None else tmax)
            assert np.array_equal(got.cpu().numpy(), want), "%s occluded, %s rays: %d differ" % (name, key, int((got.cpu().numpy() != want).sum()))
    g.close()


# ---- flags ----------------------------------------------------------------------------------------------------------------------------------
def test_skybox_flag_on_a_live_scene(ra, oracle, family):
    on, off = reference(oracle, family[1]["plain"], "plain"), reference(oracle, family[1]["plain_nosky"], "plain_nosky")
    assert not np.array_equal(bits(on["frame"]), bits(off["frame"]))
    g = ra.Scene(family[1]["plain"], W, H)
    check_frames(g, on, "skybox as loaded")
    for value, ref in ((0, off), (1, on), (0, off), (1, on)):
        g.set_flag("useSkybox", value)
        assert bool(g.view_flags() & 2) == bool(value)
        check_frames(g, ref, "useSkybox set to %d" % value)
        check_trace(g, ref, "useSkybox set to %d" % value)
    g.close()


@pytest.mark.parametrize("name", S.NORMAL_MAPPED)
def test_normals_view_equals_the_oracles(ra, oracle, family, name):
    """showNormals where normal maps of three sizes show (uv-wild included): the oracle's view (scene.cpp:771-772 after Mesh::getSurfaceData) bit
    for bit -- set in the file, and switched on and off on a live scene."""
    path = variant_path(family, name, showNormals=1)
    ref, plain = reference(oracle, path, name), reference(oracle, family[1][name], name)
    assert not np.array_equal(bits(ref["frame"]), bits(plain["frame"]))
    g = ra.Scene(path, W, H)
    assert g.view_flags() & 4
    assert_frame(g.render_host(ssaa=False), ref["pass1"], name + " normals pass 1")
    assert_frame(g.render_host(ssaa=True), ref["frame"], name + " normals frame")
    check_trace(g, ref, name + " normals")
    for key, (rays, rh, rc) in ref["rays"].items():
        assert_rays(rays, None, g.cast_rays(rays)[1], rh, rc, "%s normals cast_rays, %s rays" % (name, key))
    g.close()
    g = ra.Scene(family[1][name], W, H)
    for value, want in ((1, ref), (0, plain), (1, ref)):
        g.set_flag("showNormals", value)
        fb = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
        mask = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
        g.render_frame(fb, mask)
        assert g.frame_status() == 0
        assert_frame(fb.cpu().numpy(), want["frame"], "%s showNormals set to %d" % (name, value))
    g.close()


# ---- edits ----------------------------------------------------------------------------------------------------------------------------------
MOVES = [(0, dict(pos=(-1.2, 0.7, -3.6), rot=(40, 30, 10))), (2, dict(size=(2.2, 3.4, 2.8))), (0, dict(size=(2.5, 2.5, 3.5), rot=(75, -20, 5)))]


def test_moves_keep_the_maps(ra, oracle, family):
    """move_object of textured meshes (A: all three maps in three sizes, twice; C: a diffuse map) with the skybox on: every state equals a fresh
    load of the edited file and the oracle, in both frame modes -- the moved mesh keeps its six map fields (rtx_edit.hip), the others theirs."""
    name = "phong_nrm"
    text = open(family[1][name]).read()
    g = ra.Scene(family[1][name], W, H)
    g.gpu()
    for step, (idx, keys) in enumerate(MOVES):
        g.move_object(idx, **keys)
        text = edit_scene(text, idx, **keys)
        p = os.path.join(family[0], "%s_moved%d.scene" % (name, step))
        with open(p, "w") as f:
            f.write(text)
        ref = reference(oracle, p, name)
        what = "%s step %d" % (name, step)
        check_frames(g, ref, what)
        check_trace(g, ref, what)
        f = ra.Scene(p, W, H)
        check_frames(f, ref, what + " (fresh load)")
        f.close()
    g.close()


# ---- random scenes --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", S.RANDOM_SEEDS)
def test_random_scene_with_maps_bit_exact(ra, oracle, family, seed):
    """tests/test_gpu_fuzz.py's check on scenes whose meshes carry random subsets of maps of random non-square sizes, the skybox on in the odd
    seeds (util_shading.make_shading_scene; the seeds without normal maps are pinned to the reference by tests/test_shading_data_cpu.py)."""
    w, h = S.random_size(seed)
    path = os.path.join(family[0], "random%d.scene" % seed)
    with open(path, "w") as f:
        f.write(S.make_shading_scene(seed, w, h, family[0]))
    o = oracle.OracleScene(path, w, h)
    g = ra.Scene(path, w, h)
    ref1 = o.pass1()
    got1 = g.render_host(ssaa=False)
    assert np.array_equal(bits(ref1), bits(got1)), "seed %d: pass 1 differs in %d pixels" % (seed, int((bits(ref1) != bits(got1)).any(-1).sum()))
    assert np.array_equal(bits(o.ssaa(ref1)), bits(g.render_host(ssaa=True))), "seed %d: post-SSAA frame differs" % seed
    rays = S.shading_rays(512)                       # (two thirds of them are probe_rays(512))
    rh, rc = o.probe(rays)
    gh, gc = g.cast_rays(rays)
    assert_rays(rays, gh, gc, rh, rc, "seed %d" % seed)
    o.close()
    g.close()
