"""Scenes that put the SOURCE of a walk -- the camera of the primary rays, a point light of the shadow rays -- where the source copies of the
prune records (rtx_source.hip sourceP, rtx_api.hip buildSources, rtx_kernels.hip pruneEval8: Pn = ainf <= kSrcAinfMax ? P : Pgen) are
closest to being wrong: in and just off the plane of a triangle (H - sigma around 0), under long plane normals (sigma = bias |N|),
either side of the 32-unit fallback, at large coordinates.  The mesh is a fine sheet, fine enough for the launch to pick the kernels with
the box test (BOXES) by itself.  Every placement is derived from the placed triangles; the yardstick is the CPU oracle alone.

The sheet: lattice_obj(32, 1 / 64), 2048 triangles, rot 90,0,0, size 1,1,1 at 0,-0.5,-3: the box [-0.5, 0.5] x [-0.504, -0.496] x
[-3.5, -2.5], every normal with n.y > 0, the largest Pgen = |e1|_1 |e2|_1 = 0.00244 < 1 / 216.  Object 0 is the ground plane, object 1
the mesh."""
import functools
import os
import re

import numpy as np

from tests.test_gpu_margins import PHONG, lattice_obj

f32 = np.float32
W, H = 128, 96
BIAS = 1e-4                                   # Options::bias, which no scene key sets
K_SRC_AINF_MAX = 32.0                         # rtx_device.h kSrcAinfMax
SHIFT = np.array([1e3, -500.0, 250.0])        # the translation of test_scaled_and_translated_mesh at shift = 1e3
MESH_POS = np.array([0.0, -0.5, -3.0])
LIGHT_CAM = np.array([0.0, 0.5, -1.2])        # the camera of the light placements
GENERIC_LIGHT = np.array([0.5, 1.5, -2.0])    # the light of the camera placements
DECISIVE_FLOOR = 50

# ---- the case list ------------------------------------------------------------------------------------------------------------------------
# camera placements: (name, parameter); light placements likewise.  "@1e3": the whole scene translated by SHIFT.
CAMERA_PLACEMENTS = [("near", 0.0), ("near", 1e-6), ("near", 1e-3), ("near", 0.05), ("far", 30.0), ("far", 33.0), ("near@1e3", 1e-3)]
LIGHT_PLACEMENTS = [("on", 0.0), ("on", 1e-4), ("on", 1e-3), ("on", 0.05), ("normal", 1e-3), ("normal", 100.0), ("normal", 1e4),
                    ("ground-40", 0.3), ("above", 40.0), ("on@1e3", 1e-3)]
CULLS = (1, 0)
MATERIALS = ("diffuse", "phong")              # a Diffuse mesh: the PLAIN kernels with the wave-uniform light loop; a Phong mesh: the others
CAMERA_CASES = [("camera", name, par, "diffuse", cull) for name, par in CAMERA_PLACEMENTS for cull in CULLS]
LIGHT_CASES = [("light", name, par, mat, cull) for name, par in LIGHT_PLACEMENTS for mat in MATERIALS for cull in CULLS]
CASES = CAMERA_CASES + LIGHT_CASES


def case_id(case):
    return "%s-%s-%g-%s-cull%d" % case


def fmt(v):
    """float32 values as text that parses back to the same float32"""
    return ",".join("%.9g" % x for x in np.asarray(v, f32).reshape(-1))


def scene_text(mesh, cam, light, cull, material="diffuse", fov=60.0, plane_y=-1.5, plane_l=1.0, shift=(0, 0, 0), with_mesh=True):
    """Ground plane (normal 0,L,0: planes keep theirs un-normalised), the sheet, one point light."""
    shift = np.asarray(shift, np.float64)
    text = ("[options]\nwidth=%d\nheight=%d\nfov=%s\nposition=%s\nuseBackfaceCulling=%d\nac_penalty=1\nimage_name=output/sources\n\n"
            "[light]\ntype=point\nposition=%s\ncolor=1,0.8,0.6\nintensity=0.9\n\n"
            "[object]\ntype=plane\npos=%s\nnormal=0,%s,0\ncolor=1,1,1\n\n") % (
        W, H, fmt(fov), fmt(cam), cull, fmt(light), fmt(np.array([0.0, plane_y, 0.0]) + shift), fmt(plane_l))
    if with_mesh:
        text += "[object]\ntype=mesh\npos=%s\nsize=1,1,1\nrot=90,0,0\ncolor=1,1,1\n%sname=%s\n\n" % (
            fmt(MESH_POS + shift), PHONG if material == "phong" else "", mesh)
    return text + "[end]\n"


def without_mesh(text):
    """The scene text without its mesh block."""
    blocks = re.split(r"(?m)^(?=\[)", text)
    kept = [b for b in blocks if not (b.startswith("[object]") and re.search(r"(?m)^type=mesh\s*$", b))]
    assert len(kept) == len(blocks) - 1
    return "".join(kept)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Sheet:
    """The placed sheet of one translation: its triangles as the oracle's loader places them, the triangle k near its front-centre
    (front: towards +z, where the cameras stand), k's centroid c, unit normal n (n.y > 0) and the in-plane direction tz closest to +z."""

    def __init__(self, oracle, work, shift):
        self.shift = np.asarray(shift, np.float64)
        self.mesh = os.path.join(work, "sheet.obj")
        if not os.path.exists(self.mesh):
            with open(self.mesh, "w") as f:
                f.write(lattice_obj(32, 1.0 / 64))
        path = os.path.join(work, "sheet_base_%g.scene" % self.shift[0])
        with open(path, "w") as f:
            f.write(scene_text(self.mesh, LIGHT_CAM + self.shift, GENERIC_LIGHT + self.shift, 1, shift=self.shift))
        o = oracle.OracleScene(path, W, H)
        self.tris = o.bvh(1)["tris"][:, 0:9].copy()
        o.close()
        t = self.tris.astype(np.float64)
        a, b, c = t[:, 0:3], t[:, 3:6], t[:, 6:9]
        self.lo, self.hi = t.reshape(-1, 3).min(0), t.reshape(-1, 3).max(0)
        cen = (a + b + c) / 3
        target = np.array([0.5 * (self.lo[0] + self.hi[0]), 0.5 * (self.lo[1] + self.hi[1]), self.hi[2] - 1.0 / 16])
        self.k = int(np.argmin(np.abs(cen - target).sum(1)))
        self.c = cen[self.k]
        n = np.cross(b[self.k] - a[self.k], c[self.k] - a[self.k])
        n /= np.linalg.norm(n)
        self.n = n if n[1] > 0 else -n
        tz = np.array([0.0, 0.0, 1.0]) - self.n[2] * self.n
        self.tz = tz / np.linalg.norm(tz)
        self.tris.setflags(write=False)

    def v0e1e2(self):
        """(v0, e1, e2) of every triangle as the exact test sees them: the float32 differences b - a, c - a."""
        t = self.tris
        return t[:, 0:3], (t[:, 3:6] - t[:, 0:3]).astype(f32), (t[:, 6:9] - t[:, 0:3]).astype(f32)

    def pgen(self):
        _, e1, e2 = self.v0e1e2()
        return np.abs(e1.astype(np.float64)).sum(1) * np.abs(e2.astype(np.float64)).sum(1)


_sheets = {}


def sheet(oracle, work, shifted=False):
    key = (str(work), bool(shifted))
    if key not in _sheets:
        _sheets[key] = Sheet(oracle, str(work), SHIFT if shifted else np.zeros(3))
    return _sheets[key]


def placement(oracle, work, case):
    """dict of one case: cam, light (float32, as the scene file holds them), fov, plane_y, plane_l, shift, the Sheet, and `text`."""
    kind, name, par, material, cull = case
    s = sheet(oracle, work, name.endswith("@1e3"))
    d = dict(cam=LIGHT_CAM + s.shift, light=GENERIC_LIGHT + s.shift, fov=60.0, plane_y=-1.5, plane_l=1.0, shift=s.shift, sheet=s, cull=cull,
             material=material)
    base = name.split("@")[0]
    if kind == "camera":
        if base == "near":          # in, or just off, the plane of triangle k, looking along the sheet
            d["cam"] = s.c + 0.9 * s.tz + par * s.n
        else:                       # far: either side of kSrcAinfMax from the sheet, through a narrow lens
            assert base == "far"
            d["cam"] = MESH_POS + np.array([0.0, 0.5, par]) + s.shift
            d["fov"] = 3.0
    else:
        if base == "on":
            d["light"] = s.c + par * s.n
        elif base == "normal":
            d["light"] = s.c + 0.3 * s.n
            d["plane_l"] = par
        elif base == "ground-40":
            d["light"] = s.c + par * s.n
            d["plane_y"] = -40.0
        else:
            assert base == "above"
            d["light"] = s.c + np.array([0.0, par, 0.0])
    d["cam"] = np.asarray(d["cam"], f32); d["light"] = np.asarray(d["light"], f32)
    d["text"] = scene_text(s.mesh, d["cam"], d["light"], cull, material, d["fov"], d["plane_y"], d["plane_l"], s.shift)
    return d


def write_case(oracle, work, case):
    """(path of the case's scene file under `work`, its placement)"""
    d = placement(oracle, work, case)
    path = os.path.join(str(work), "src_%s.scene" % case_id(case).replace("@", "_at_"))
    with open(path, "w") as f:
        f.write(d["text"])
    return path, d


def decisive(oracle, path):
    """The number of pixels whose pass-1 bits differ between the oracle's frame of the scene and of the same scene without its mesh block:
    the pixels a lost hit of the mesh -- primary or shadow -- can show in."""
    with open(path) as f:
        text = f.read()
    bare = path[:-len(".scene")] + "_nomesh.scene"
    with open(bare, "w") as f:
        f.write(without_mesh(text))
    frames = []
    for p in (path, bare):
        o = oracle.OracleScene(p, W, H)
        frames.append(o.pass1())
        o.close()
    return int((bits(frames[0]) != bits(frames[1])).any(-1).sum())


@functools.lru_cache(maxsize=None)
def reference(oracle, path):
    """(pass 1, post-SSAA frame, SSAA mask) of a scene file by the oracle, computed once and shared read-only."""
    o = oracle.OracleScene(path, W, H)
    p1 = o.pass1()
    mask = o.sobel(p1)
    mask[0, :] = 0; mask[-1, :] = 0; mask[:, 0] = 0; mask[:, -1] = 0       # (border = 0 by definition)
    out = (p1, o.ssaa(p1), mask)
    o.close()
    for a in out:
        a.setflags(write=False)
    return out


# ---- the host's P of a source over the placed triangles -----------------------------------------------------------------------------------
def light_sigma_floor(plane_l):
    """bias |N|max: a lower bound of the sigma buildSources gives a light's copy (its rounding part only adds to it)."""
    return BIAS * max(1.0, float(plane_l))


def host_p(ra, s, S, sigma, cam):
    """source_p_probe of every placed triangle for the source S (as the scene file holds it: float32)."""
    v0, e1, e2 = s.v0e1e2()
    return ra.source_p_probe(v0, e1, e2, np.asarray(S, f32).astype(np.float64), sigma, cam)


def certified(p, pgen):
    """P below the unconditional Pgen (sourceP returns Pgen rounded up where the certificate fails)."""
    return p < pgen.astype(f32)


# ---- the references below every slot of the device's wide nodes ---------------------------------------------------------------------------
def slot_triangles(wide, refs):
    """wide: [n, S, 8] float32 of device_mesh_flat (rtx_device.h Node: link / first as bit patterns in [..., 6:8]); refs: the triangle of
    every leaf reference.  Returns {(wide node, slot): sorted array of the triangles below it} for the non-empty slots."""
    link = np.ascontiguousarray(wide[..., 6]).view(np.int32)
    first = np.ascontiguousarray(wide[..., 7]).view(np.int32)
    n, S = link.shape
    below = {}

    def node(w, depth=0):
        assert depth < 64
        if w not in below:
            parts = [slot(w, k, depth) for k in range(S) if link[w, k] != 0]
            below[w] = np.unique(np.concatenate(parts)) if parts else np.zeros(0, np.int64)
        return below[w]

    def slot(w, k, depth):
        l = int(link[w, k])
        if l < 0:
            cnt, b = ~l, int(first[w, k])
            assert 0 <= b and b + cnt <= len(refs)
            return np.asarray(refs[b:b + cnt], np.int64)
        assert 0 < l <= n
        return node(l - 1, depth + 1)

    out = {}
    for w in range(n):
        for k in range(S):
            if link[w, k] != 0:
                out[(w, k)] = np.unique(slot(w, k, 0))
    return out


# ---- the record check ---------------------------------------------------------------------------------------------------------------------
# What a placement says about the certificates of a copy: "k" -- no slot above triangle k is certified (the source lies in k's plane, or
# within sigma of it); "none" -- no slot is (sigma above every height); "most" -- more than half of the non-empty slots are.
def copy_states(case):
    """{copy: (source, sigma floor, cam, state or None)} of a case: copy 1 the camera's, copy 2 the light's."""
    kind, name, par, _, _ = case
    base = name.split("@")[0]
    cam_state, light_state = "most", "most"
    if kind == "camera":
        if base == "near":
            cam_state = "k" if par == 0.0 else ("most" if par >= 0.05 else None)
    else:
        if base == "on":
            light_state = "k" if par <= 1e-4 else ("most" if par >= 0.05 else None)
        elif base == "normal" and par >= 1e4:
            light_state = "none"
    return cam_state, light_state


def check_records(ra, copies, wide, refs, d, case, what=""):
    """The checks of a device's prune-record copies (Scene.device_prune_copies: float32 (copies, n_wide, 2 S, 8)) against the host's sourceP
    of the placed triangles: P <= Pgen, copy 0 generic, every non-empty slot's P at least the plain float32 max of rtx_source_p_probe over
    the triangles below it (sigma: 0 for the camera, bias |N|max for the light -- a lower bound of the device's, and sourceP grows with
    sigma), and the certificate state the placement is there for."""
    s = d["sheet"]
    S8 = copies.shape[2] // 2
    assert copies.shape[0] == 3 and copies.shape[1] == wide.shape[0] and wide.shape[1] == S8, (copies.shape, wide.shape)
    box = copies[:, :, :S8, :]
    P, Pgen, h0 = box[..., 3], box[..., 7], box[..., 4]
    assert np.array_equal(bits(box[1:, ..., [0, 1, 2, 4, 5, 6, 7]]), bits(np.broadcast_to(box[0][..., [0, 1, 2, 4, 5, 6, 7]], box[1:, ..., :7].shape))), \
        "%s: a source copy differs from copy 0 in more than P" % what
    assert np.array_equal(bits(copies[1:, :, S8:, :]), bits(np.broadcast_to(copies[0, :, S8:, :], copies[1:, :, S8:, :].shape))), \
        "%s: a source copy's plane records differ from copy 0's" % what
    nonempty = h0[0] >= 0
    assert (P <= Pgen).all(), "%s: %d records with P > Pgen" % (what, int((~(P <= Pgen)).sum()))
    assert np.array_equal(bits(P[0]), bits(Pgen[0])), "%s: copy 0 is not generic" % what
    below = slot_triangles(wide, np.asarray(refs))
    assert len(np.unique(np.concatenate(list(below.values())))) == len(s.tris), "%s: the slots do not cover the mesh" % what
    slots = [tuple(x) for x in np.argwhere(nonempty)]
    assert slots and all(sl in below and len(below[sl]) for sl in slots), "%s: a non-empty record over a slot without references" % what
    pgen_tri = s.pgen()
    states = copy_states(case)
    sources = ((d["cam"], 0.0, True), (d["light"], light_sigma_floor(d["plane_l"]), False))
    shares = []
    for copy, (src, sigma, cam) in zip((1, 2), sources):
        hp = host_p(ra, s, src, sigma, cam)
        assert (hp == hp).all()
        want = np.array([hp[below[sl]].max() for sl in slots], f32)
        got = np.array([P[copy][sl] for sl in slots], f32)
        pg = np.array([Pgen[copy][sl] for sl in slots], f32)
        low = got < want
        assert not low.any(), "%s: copy %d: %d of %d slots hold a P below the host's max over their triangles, first %r: %r < %r" % (
            what, copy, int(low.sum()), len(slots), slots[int(np.argmax(low))], got[int(np.argmax(low))], want[int(np.argmax(low))])
        generic = got >= pg * f32(0.999)           # (the sheet's triangles share one Pgen up to the rounding of their placement)
        share = 1.0 - generic.mean()
        shares.append(share)
        state = states[copy - 1]
        if state == "k":
            above = np.array([s.k in below[sl] for sl in slots])
            assert above.sum() >= 2 and generic[above].all(), "%s: copy %d certifies %d of the %d slots above triangle k" % (
                what, copy, int((~generic[above]).sum()), int(above.sum()))
            assert not certified(hp, pgen_tri)[s.k]
        elif state == "none":
            assert generic.all(), "%s: copy %d certifies %d slots under a sigma above every height" % (what, copy, int((~generic).sum()))
        elif state == "most":
            assert share > 0.5, "%s: copy %d certifies only %.3f of its non-empty slots" % (what, copy, share)
    return shares


def host_copies(ra, bvh, d):
    """What buildSources must leave at the least, from the host alone: (copies, wide, refs) with every slot's P the max of the host's
    sourceP over the triangles below it, capped by Pgen (the emulation the CPU tests run check_records on)."""
    wide, box, plane, _ = ra.mesh_flatten_probe(bvh)
    block = np.concatenate([box, plane], 1)
    copies = np.stack([block, block, block]).copy()
    below = slot_triangles(wide, bvh["refs"])
    s = d["sheet"]
    S8 = box.shape[1]
    for copy, (src, sigma, cam) in zip((1, 2), ((d["cam"], 0.0, True), (d["light"], light_sigma_floor(d["plane_l"]), False))):
        hp = host_p(ra, s, src, sigma, cam)
        for (w, k), tris in below.items():
            if copies[copy, w, k, 4] >= 0 and len(tris):
                copies[copy, w, k, 3] = min(hp[tris].max(), copies[copy, w, k, 7])
    return copies, wide, bvh["refs"]
