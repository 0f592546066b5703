"""Adversarial inputs for the two places where the HIP path decides NOT to run the reference's arithmetic: the bundle filter
(rtx_kernels.hip, bundleRejects1/2: error-budget margins, K = 64 u) and the prune records of the wide walk (pruneAlive /
planeAlive: 36 u dmax ainf P / 1e-8 around a slot's true box, the filter's first stage over a slot's normal box).  Every
ray family below is aimed AT a margin; the per-ray records (object, t, triangle, u, v, colour) must equal the oracle's
bit for bit (objects.cpp:59-95, 534-631).  Rays come in groups of 64 = one wave = one narrow bundle, as in a frame.
VERDICT r2, item 4."""
import os

import numpy as np
import pytest

from tests import util_occlusion as OC
from tests.util_analytic import lattice_obj      # (util_sources and the tests below take it from here)

pytestmark = pytest.mark.gpu
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def scene_text(mesh, pos=(0, 0, -3), size=(2, 2, 2), rot=(0, 0, 0), cull=1, cam=(0, 0, 0), w=96, h=72, penalty=1, plane_y=-1.5, material=""):
    return ("[options]\nwidth=%d\nheight=%d\nfov=60\nposition=%s\nuseBackfaceCulling=%d\nac_penalty=%d\nimage_name=output/margins\n\n"
            "[light]\ntype=point\nposition=%s\ncolor=1,0.8,0.6\nintensity=0.9\n\n[light]\ntype=distant\ndirection=0.3,-1,-0.4\ncolor=0.4,0.6,1\nintensity=0.5\n\n"
            "[object]\ntype=plane\npos=%s\nnormal=0,1,0\ncolor=1,1,1\n\n"
            "[object]\ntype=mesh\npos=%s\nsize=%s\nrot=%s\ncolor=1,1,1\n%sname=%s\n\n[end]\n") % (
        w, h, ",".join("%r" % float(x) for x in cam), cull, penalty,
        ",".join("%r" % float(x) for x in (cam[0] + 1, cam[1] + 2, cam[2] - 1)),
        ",".join("%r" % float(x) for x in (cam[0], cam[1] + plane_y * max(size), cam[2])),
        ",".join("%r" % float(x) for x in pos), ",".join("%r" % float(x) for x in size), ",".join("%r" % float(x) for x in rot), material, mesh)


def waves(base_o, base_d, rng, rel=2.0 ** -12):
    """Every base ray becomes a wave of 64: itself, ulp neighbours, and small relative perturbations of origin and direction."""
    n = len(base_o)
    o = np.repeat(base_o[:, None, :], 64, 1).astype(f32); d = np.repeat(base_d[:, None, :], 64, 1).astype(f32)
    scale_o = np.maximum(np.abs(base_o).max(1), 1e-30)[:, None, None]; scale_d = np.maximum(np.abs(base_d).max(1), 1e-30)[:, None, None]
    jo = rng.uniform(-1, 1, (n, 64, 3)) * rel * scale_o; jd = rng.uniform(-1, 1, (n, 64, 3)) * rel * scale_d
    jo[:, :16] = 0; jd[:, :16] = 0                   # lanes 0..15: the base ray and its ulp neighbours
    o = (o + jo.astype(f32)).astype(f32); d = (d + jd.astype(f32)).astype(f32)
    for k in range(1, 16):
        which = o if k % 2 else d
        comp = (k // 2) % 3
        step = 1 if k < 8 else -1
        which[:, k, comp] = np.nextafter(which[:, k, comp], f32(np.inf if step > 0 else -np.inf))
    return np.concatenate([o, d], 2).reshape(-1, 6)


def ray_families(tris, rng, n_tri=48):
    """Rays aimed at the margins of the triangles `tris` (n x 9: a, b, c as uploaded)."""
    T = tris[rng.choice(len(tris), min(n_tri, len(tris)), replace=False)].astype(np.float64)
    A, B, C = T[:, 0:3], T[:, 3:6], T[:, 6:9]
    e1, e2 = B - A, C - A
    nrm = np.cross(e1, e2); area2 = np.linalg.norm(nrm, axis=1); ok = area2 > 0
    A, B, C, e1, e2, nrm, area2 = A[ok], B[ok], C[ok], e1[ok], e2[ok], nrm[ok], area2[ok]
    nh = nrm / area2[:, None]
    size = np.maximum(np.linalg.norm(e1, axis=1), np.linalg.norm(e2, axis=1))[:, None]
    O, D = [], []

    def add(o, d):
        O.append(np.asarray(o, np.float64)); D.append(np.asarray(d, np.float64))

    # 1. through vertices, edge midpoints and the centroid: u = 0, v = 0, u + v = 1 exactly (in exact arithmetic)
    for P in (A, B, C, 0.5 * (A + B), 0.5 * (B + C), 0.5 * (A + C), (A + B + C) / 3):
        for d in ((0.25, 0.5, -1.0), (-0.5, 0.125, -1.0)):
            dd = np.broadcast_to(np.array(d), P.shape)
            add(P - 2.0 * dd, dd)
        add(P + 2.0 * size * nh, -nh)                # along the (reversed) face normal: front face when culling is on
    # 2. |det| straddling 1e-8 (objects.cpp:75-79): det = dir . (e2 x e1) = -dir . nrm
    tang = e1 / np.linalg.norm(e1, axis=1)[:, None]
    for j in (-40, -6, -2, -1, 0, 1, 2, 6, 40):
        alpha = 1e-8 * (1.0 + j * 2.0 ** -23) / area2
        d = tang - nh * alpha[:, None]               # det = alpha |nrm|
        P = (A + B + C) / 3
        add(P - d * (0.5 * size), d)
        add(P - d * (4.0 * size) + nh * 1e-6 * size, d)
    # 3. grazing: nearly in the plane of the triangle, starting on / just off the plane, near and far
    for dl in (2.0 ** -6, 2.0 ** -10, 2.0 ** -14, 2.0 ** -18, 2.0 ** -22, -2.0 ** -14, -2.0 ** -22):
        for s in (0.05, 2.0, 40.0):
            for eps in (0.0, 2.0 ** -20, -2.0 ** -20):
                d = tang * np.cos(dl) - nh * np.sin(dl)
                add((A + B + C) / 3 - d * (s * size) + nh * (eps * size), d)
    o = np.concatenate(O).astype(f32); d = np.concatenate(D).astype(f32)
    # 4. magnitudes either side of the filter's "tame" limits (|dir| < 2^20, |orig| < 2^40), and tiny directions
    k = len(A)
    extra_o, extra_d = [], []
    for sc in (2.0 ** 19, 2.0 ** 21, 2.0 ** -30):
        extra_o.append(o[:k]); extra_d.append((d[:k].astype(np.float64) * sc).astype(f32))
    for far in (2.0 ** 39, 2.0 ** 41):
        dn = d[:k].astype(np.float64); dn /= np.linalg.norm(dn, axis=1)[:, None]
        extra_o.append((o[:k] - dn * far).astype(f32)); extra_d.append(dn.astype(f32))
    # 5. zero, negative-zero and denormal direction components
    for comp, val in ((0, 0.0), (1, -0.0), (0, 1e-40), (1, -1e-42), (2, 1e-39)):
        dz = d[k:3 * k].copy(); dz[:, comp] = f32(val)
        extra_o.append(o[k:3 * k]); extra_d.append(dz)
    o = np.concatenate([o] + extra_o); d = np.concatenate([d] + extra_d)
    return waves(o, d, rng)


def check(ra, oracle, path, w, h, obj_idx, seed, frames=True, n_tri=48, boxes=None):
    o = oracle.OracleScene(path, w, h)
    g = ra.Scene(path, w, h)
    if boxes is not None:
        g.set_knob("prune_boxes", boxes)
        assert g.kernel_variant()["boxes"] == bool(boxes), "prune_boxes = %d did not take" % boxes
    tris = g.bvh(obj_idx)["tris"][:, 0:9]
    rays = ray_families(tris, np.random.default_rng(seed), n_tri)
    rh, rc = o.probe(rays)
    gh, gc = g.cast_rays(rays)
    bad = (bits(rh) != bits(gh)).any(1) | (bits(rc) != bits(gc)).any(1)
    assert not bad.any(), "%s: %d of %d rays differ, first %d: ray %s oracle %s gpu %s" % (
        path, int(bad.sum()), len(rays), int(np.argmax(bad)), rays[np.argmax(bad)], rh[np.argmax(bad)], gh[np.argmax(bad)])
    hits = int((rh[:, 0] >= 0).sum())
    if frames:
        ref = o.ssaa(o.pass1())
        got = g.render_host(ssaa=True)
        assert np.array_equal(bits(ref), bits(got)), "%s: frame differs in %d pixels" % (path, int((bits(ref) != bits(got)).any(-1).sum()))
    o.close(); g.close()
    return len(rays), hits


@pytest.mark.parametrize("cull", [1, 0])
@pytest.mark.parametrize("bump", [0.0, 0.0625])
def test_lattice_edges_vertices_det_and_grazing(ra, oracle, tmp_path, cull, bump):
    """A lattice mesh (vertices on multiples of 1/8): rays through shared vertices and edges, |det| either side of 1e-8,
    rays in the plane of a flat sheet of coplanar triangles (every one of them a candidate for a garbage hit)."""
    obj = tmp_path / "lattice.obj"
    obj.write_text(lattice_obj(16, bump))
    path = tmp_path / "lattice.scene"
    path.write_text(scene_text(str(obj), pos=(0, 0, -3), size=(2, 2, 2) if bump else (2, 2, 0), rot=(0, 0, 0) if bump == 0 else (20, 30, 0), cull=cull))
    n, hits = check(ra, oracle, str(path), 96, 72, 1, 11 + cull)
    assert hits > n // 50


@pytest.mark.parametrize("cull", [1, 0])
@pytest.mark.parametrize("scale,shift", [(1.0, 0.0), (1e-4, 0.0), (1e4, 0.0), (1.0, 1e3), (1.0, 1e5), (1e-4, 1e3)])
def test_scaled_and_translated_mesh(ra, oracle, tmp_path, cull, scale, shift):
    """The 4k mesh scaled by 1e-4 / 1e+4 and translated by 1e3 / 1e5 (camera moved along): the error scales of the filter
    (ainf, s1 s2) and of the prune records (P, vmax) move by orders of magnitude.  (A mesh out at 2^20, where fp32 steps are
    wider than the 0.1 of the reference's split search, objects.cpp:676-689, is no test case: the reference's builder never
    returns there.  The filter's 2^20 / 2^40 limits are met by ray family 4 instead.)"""
    from rendering_amd import assets
    mesh = assets.ensure(["bumpy_4k.obj"])["bumpy_4k.obj"]
    cam = (shift, -shift * 0.5, shift * 0.25)
    pos = (cam[0], cam[1], cam[2] - 3 * scale)
    path = tmp_path / "scaled.scene"
    path.write_text(scene_text(mesh, pos=pos, size=(2 * scale,) * 3, rot=(10, 25, 5), cull=cull, cam=cam))
    check(ra, oracle, str(path), 96, 72, 1, 23)


@pytest.mark.parametrize("name,n_tri", [("bumpy_25k.obj", 32), ("bumpy_250k.obj", 12)])
def test_fine_meshes_where_the_box_records_prune(ra, oracle, tmp_path, name, n_tri):
    """Meshes of small triangles (P = |e1|_1 |e2|_1 ~ 5e-4 .. 5e-3): the inflated true boxes are tight enough to prune, so
    the grazing and det ~ 1e-8 families test the 36 u dmax ainf P / 1e-8 bound where it matters."""
    from rendering_amd import assets
    mesh = assets.ensure([name])[name]
    for cull in (1, 0):
        path = tmp_path / ("fine%d.scene" % cull)
        path.write_text(scene_text(mesh, pos=(0, 0, -3), size=(2, 2, 2), rot=(0, 0, 0), cull=cull, w=128, h=96))
        n, hits = check(ra, oracle, str(path), 128, 96, 1, 31 + cull, frames=(name != "bumpy_250k.obj" or cull == 1), n_tri=n_tri)
        assert hits > n // 50


@pytest.mark.parametrize("name,size,boxes", [("bumpy_4k.obj", 2, 1), ("bumpy_25k.obj", 1, 0)], ids=["bumpy_4k.obj-1", "bumpy_25k.obj-0"])
def test_either_kernel_variant_on_either_kind_of_mesh(ra, oracle, tmp_path, name, size, boxes):
    """The launch picks the kernels with the box test of the prune records (BOXES) only for scenes with small triangles (the whole
    mesh's P < 1/216: the 25k mesh at size 1, not at size 2); the knob forces the other variant: the box test on a mesh of large
    triangles (its margin is then larger than the mesh: it must simply never prune), and a fine mesh through the kernels without it."""
    from rendering_amd import assets
    mesh = assets.ensure([name])[name]
    path = tmp_path / "variant.scene"
    path.write_text(scene_text(mesh, pos=(0, 0, -3), size=(size,) * 3, rot=(15, 40, 0), cull=1, w=128, h=96))
    g = ra.Scene(str(path), 128, 96)
    assert g.kernel_variant()["boxes"] == (not boxes), "%s: the meshes no longer choose the other variant by themselves" % name
    g.close()
    n, hits = check(ra, oracle, str(path), 128, 96, 1, 47, n_tri=24, boxes=boxes)
    assert hits > n // 50


def test_environment_knobs_need_the_gate(ra, tmp_path, monkeypatch):
    """The product ignores RTX_* variables unless RTX_ALLOW_ENV_KNOBS=1: a scene created under RTX_PRUNE_BOXES=1 keeps the variant its
    meshes choose, and takes the forced one only through the gate.  (Tests force knobs with set_knob: an environment knob without the gate
    forces nothing.)"""
    from rendering_amd import assets
    mesh = assets.ensure(["bumpy_4k.obj"])["bumpy_4k.obj"]
    path = tmp_path / "gate.scene"
    path.write_text(scene_text(mesh, pos=(0, 0, -3), size=(2, 2, 2), rot=(15, 40, 0), cull=1, w=64, h=48))
    monkeypatch.delenv("RTX_ALLOW_ENV_KNOBS", raising=False)
    monkeypatch.setenv("RTX_PRUNE_BOXES", "1")
    g = ra.Scene(str(path), 64, 48)
    assert not g.kernel_variant()["boxes"], "RTX_PRUNE_BOXES took effect without RTX_ALLOW_ENV_KNOBS"
    g.close()
    monkeypatch.setenv("RTX_ALLOW_ENV_KNOBS", "1")
    g = ra.Scene(str(path), 64, 48)
    assert g.kernel_variant()["boxes"], "RTX_PRUNE_BOXES=1 did not take with RTX_ALLOW_ENV_KNOBS=1"
    g.close()


# The variant matrix: the ray families of the margins through the kernels the product launches for frames and rtx_trace_rays -- compile-time
# variants per (PLAIN, BOXES, CULL) for pass 1, SSAA, the single-launch frame and the colour kernel, per (BOXES, CULL) for the hit kernel
# (rtx_scene.h variantOf; rtx_api.hip pass1Kernel, ssaaKernel, frameKernel, rayHitKernel, rayColourKernel).  PLAIN follows from the material (Diffuse everywhere, or a Phong mesh),
# BOXES is forced with the knob, CULL is the scene's.  Every case asserts the bits it expects, and the list below names every combination
# on every scene, so no selection of tests can shrink the matrix unnoticed.
PHONG = "material=phong,0.4,0.1,0.7,10.0\n"
MATRIX_SCENES = ["lattice_flat", "lattice_bumped", "mesh_1e-4", "mesh_at_1e5"]
MATRIX = [(scene, plain, boxes, cull) for scene in MATRIX_SCENES for plain in (1, 0) for boxes in (0, 1) for cull in (1, 0)]
_matrix_oracle = {}


def matrix_scene(tmp_path, scene, plain, cull):
    material = "" if plain else PHONG
    if scene.startswith("lattice"):
        bump = 0.0625 if scene == "lattice_bumped" else 0.0
        obj = tmp_path / "lattice.obj"
        obj.write_text(lattice_obj(16, bump))
        text = scene_text(str(obj), pos=(0, 0, -3), size=(2, 2, 2) if bump else (2, 2, 0), rot=(20, 30, 0) if bump else (0, 0, 0), cull=cull,
                          w=128, h=96, material=material)
    else:
        from rendering_amd import assets
        mesh = assets.ensure(["bumpy_4k.obj"])["bumpy_4k.obj"]
        scale, shift = {"mesh_1e-4": (1e-4, 0.0), "mesh_at_1e5": (1.0, 1e5)}[scene]
        cam = (shift, -shift * 0.5, shift * 0.25)
        text = scene_text(mesh, pos=(cam[0], cam[1], cam[2] - 3 * scale), size=(2 * scale,) * 3, rot=(10, 25, 5), cull=cull, cam=cam,
                          w=128, h=96, material=material)
    path = tmp_path / "matrix.scene"
    path.write_text(text)
    return str(path)


def matrix_reference(oracle, ra, path, key):
    """The oracle's rays, probe records, frame and mask of a matrix scene (the same for either BOXES: computed once)."""
    if key not in _matrix_oracle:
        o = oracle.OracleScene(path, 128, 96)
        g = ra.Scene(path, 128, 96)
        tris = g.bvh(1)["tris"][:, 0:9]
        g.close()
        rays = ray_families(tris, np.random.default_rng(61), 16)
        rh, rc = o.probe(rays)
        p1 = o.pass1()
        mask = o.sobel(p1)
        mask[0, :] = 0; mask[-1, :] = 0; mask[:, 0] = 0; mask[:, -1] = 0       # (border = 0 by definition)
        _matrix_oracle[key] = (rays, rh, rc, o.ssaa(p1), mask)
        o.close()
    return _matrix_oracle[key]


def occlusion_ranges(hit, tnear):
    """The ranges the margin rays are asked with as occlusion queries: none (the whole ray), +inf, every ray's own nearest hit and its
    neighbours (util_occlusion.tmax_mix: t, nextafter(t, +-), 0.5 t, 1.5 t, +inf), and FLT_MAX, +inf, NaN, 0 and 1e-30 in turn within every
    wave -- a lane with an unbounded range then shares its bundle's largest range with lanes that can see nothing."""
    n = len(tnear)
    turn = np.array([OC.FLT_MAX, np.inf, np.nan, 0.0, 1e-30], f32)[(np.arange(n) % 64) % 5]
    mix = OC.tmax_mix(hit, tnear)
    assert (hit & (mix == tnear)).sum() > 10 and (hit & (mix < tnear)).sum() > 10 and (hit & (mix > tnear)).sum() > 10
    return [("none", None), ("+inf", float("inf")), ("mix", mix), ("FLT_MAX / +inf / NaN / 0 / 1e-30 in turn", np.ascontiguousarray(turn))]


@pytest.mark.parametrize("scene,plain,boxes,cull", MATRIX)
def test_variant_matrix_rays_and_frames(ra, oracle, tmp_path, scene, plain, boxes, cull):
    """The margin rays through rtx_trace_rays (trace_reorder 0: a wave of 64 stays the bundle it was built as) and frames in one and in
    three launches, on the variant (PLAIN, BOXES, CULL) the case names, against the oracle bit for bit."""
    import torch
    path = matrix_scene(tmp_path, scene, plain, cull)
    rays, rh, rc, ref, ref_mask = matrix_reference(oracle, ra, path, (scene, plain, cull))
    g = ra.Scene(path, 128, 96)
    g.set_knob("prune_boxes", boxes)
    g.set_knob("trace_reorder", 0)
    v = g.kernel_variant()
    assert (v["plain"], v["boxes"], v["cull"], v["analytic"], v["stats"]) == (bool(plain), bool(boxes), bool(cull), False, False), v
    gh, gc = g.trace_rays(torch.from_numpy(rays).cuda())
    torch.cuda.synchronize()
    gh, gc = gh.cpu().numpy(), gc.cpu().numpy()
    bad = (bits(rh) != bits(gh)).any(1) | (bits(rc) != bits(gc)).any(1)
    assert not bad.any(), "%d of %d rays differ, first %d: ray %s oracle %s %s gpu %s %s" % (
        int(bad.sum()), len(rays), int(np.argmax(bad)), rays[np.argmax(bad)], rh[np.argmax(bad)], rc[np.argmax(bad)], gh[np.argmax(bad)], gc[np.argmax(bad)])
    assert (rh[:, 0] >= 0).sum() > len(rays) // 50
    # the same rays as occlusion queries (rtxRayOccludedKernel: the one entry point with a range per ray, walked in shadow mode under the
    # wave's largest range): no object here is Transparent, so the oracle's records above say what is occluded
    hit, tnear = rh[:, 0] > 0, rh[:, 3].astype(f32)
    assert hit.sum() > len(rays) // 50
    rays_dev = torch.from_numpy(rays).cuda()
    for label, tmax in occlusion_ranges(hit, tnear):
        arg = torch.from_numpy(tmax).cuda() if isinstance(tmax, np.ndarray) else tmax
        got = g.occluded(rays_dev, arg)
        torch.cuda.synchronize()
        want = OC.expected(hit, tnear, f32(np.inf) if tmax is None else tmax)
        bad = got.cpu().numpy() != want
        assert not bad.any(), "occluded, ranges %s: %d of %d rays differ, first %d: ray %s oracle %s range %r" % (
            label, int(bad.sum()), len(rays), int(np.argmax(bad)), rays[np.argmax(bad)], rh[np.argmax(bad)],
            np.broadcast_to(np.asarray(np.inf if tmax is None else tmax, f32), tnear.shape)[np.argmax(bad)])
    for mode in (1, 0, 1):          # one launch (cold, then warm: slow tiles split), three launches
        fb = torch.zeros((96, 128, 3), dtype=torch.float32, device="cuda")
        mask = torch.zeros((96, 128), dtype=torch.uint8, device="cuda")
        g.set_frame_mode(mode)
        g.render_frame(fb, mask)
        assert g.frame_status() == 0 and g.frame_mode()[0] == mode
        got = fb.cpu().numpy()
        nd = int((bits(ref) != bits(got)).any(-1).sum())
        assert nd == 0, "%s in %s: %d pixels differ" % (scene, "one launch" if mode else "three launches", nd)
        assert np.array_equal(mask.cpu().numpy() != 0, ref_mask != 0), "%s in %s: mask differs" % (scene, "one launch" if mode else "three launches")
    assert g.kernel_variant() == v
    g.close()


def test_variant_matrix_is_complete():
    """Every (PLAIN, BOXES, CULL) on every matrix scene -- so every (BOXES, CULL) of the hit kernel too."""
    for scene in MATRIX_SCENES:
        assert {(p, b, c) for s, p, b, c in MATRIX if s == scene} == {(p, b, c) for p in (0, 1) for b in (0, 1) for c in (0, 1)}
