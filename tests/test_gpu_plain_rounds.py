"""The rounds of the PLAIN kernels (rendering_amd/csrc/rtx_kernels.hip): pass 1 and the colour kernel of rtx_trace_rays trace the primary ray and loop
over the lights on a scalar index (castRayPlainWave), SSAA and the one-launch frame run the per-lane castRay state machine (castRayWave).
Scenes of the family of tests/util_shading.py (tests/util_plain_rounds.py): no lights at all;
distant and point lights mixed; lights below a floor, so that every ray to them is moot and whole rounds have nothing to trace; views with tiles
of pure sky (skybox and background colour); recursion depth 0 and negative -- each with culling on and off and with and without the box test of
the prune records, as rays (the colour kernel of rtx_trace_rays: rays that do not start at the camera as far as the kernel knows) and as frames in
one launch and in three; the SSAA layouts of 16, 4 and 1 pixels per item; row bands with halo strips.  Everything bit for bit against the oracle,
and every case asserts through rtx_kernel_variant that a PLAIN kernel ran.  tests/test_plain_rounds_cpu.py pins the oracle to the reference on
the same scenes."""
import numpy as np
import pytest

from tests import util_plain_rounds as PR
from tests import util_shading as U

pytestmark = pytest.mark.gpu

W, H = PR.W, PR.H


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def images(tmp_path_factory):
    d = U.short_dir(tmp_path_factory)
    U.write_images(d)
    return d


_oracle = {}


def reference(oracle, images, name, cull, w=W, h=H):
    """path, and the oracle's rays, probe records, pass 1, frame and mask of the case (the same for either BOXES: computed once)."""
    key = (name, cull, w, h)
    if key not in _oracle:
        path = PR.write_scene(name, images, cull)
        o = oracle.OracleScene(path, w, h)
        p1 = o.pass1()
        if (w, h) == (W, H):
            PR.expectations(name, o, p1)
        rays = U.primary_rays(o)
        rh, rc = o.probe(rays)
        mask = o.sobel(p1)
        mask[0, :] = 0; mask[-1, :] = 0; mask[:, 0] = 0; mask[:, -1] = 0       # (border = 0 by definition)
        _oracle[key] = (path, rays, rh, rc, p1, o.ssaa(p1), mask)
        o.close()
    return _oracle[key]


def plain_scene(ra, path, w, h, cull, boxes=None):
    g = ra.Scene(path, w, h)
    if boxes is not None:
        g.set_knob("prune_boxes", boxes)
    v = g.kernel_variant()
    assert v["plain"] and not v["analytic"] and not v["stats"] and v["cull"] == bool(cull), v
    if boxes is not None:
        assert v["boxes"] == bool(boxes), v
    return g, v


@pytest.mark.parametrize("boxes", [1, 0])
@pytest.mark.parametrize("cull", [1, 0])
@pytest.mark.parametrize("name", sorted(PR.SCENES))
def test_rays_and_frames(ra, oracle, images, name, cull, boxes):
    """The frame's own primary rays through rtx_trace_rays, pass 1 alone, and the frame in one launch (cold, then warm: slow tiles split) and
    in three launches."""
    import torch
    path, rays, rh, rc, p1, ref, ref_mask = reference(oracle, images, name, cull)
    g, v = plain_scene(ra, path, W, H, cull, boxes)
    for reorder in (0, 1):
        g.set_knob("trace_reorder", reorder)
        gh, gc = g.trace_rays(torch.from_numpy(rays).cuda())
        torch.cuda.synchronize()
        gh, gc = gh.cpu().numpy(), gc.cpu().numpy()
        bad = (bits(rh) != bits(gh)).any(1) | (bits(rc) != bits(gc)).any(1)
        assert not bad.any(), "%s, trace_reorder %d: %d of %d rays differ, first %d: ray %s oracle %s %s gpu %s %s" % (
            name, reorder, int(bad.sum()), len(rays), int(np.argmax(bad)), rays[np.argmax(bad)], rh[np.argmax(bad)], rc[np.argmax(bad)],
            gh[np.argmax(bad)], gc[np.argmax(bad)])
    fb = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    g.render_pass1(fb)
    torch.cuda.synchronize()
    nd = int((bits(p1) != bits(fb.cpu().numpy())).any(-1).sum())
    assert nd == 0, "%s, pass 1: %d pixels differ" % (name, nd)
    for mode in (1, 1, 0):
        fb = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
        mask = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
        g.set_frame_mode(mode)
        g.render_frame(fb, mask)
        assert g.frame_status() == 0 and g.frame_mode()[0] == mode
        nd = int((bits(ref) != bits(fb.cpu().numpy())).any(-1).sum())
        assert nd == 0, "%s in %s: %d pixels differ" % (name, "one launch" if mode else "three launches", nd)
        assert np.array_equal(mask.cpu().numpy() != 0, ref_mask != 0), "%s in %s: mask differs" % (name, "one launch" if mode else "three launches")
    assert g.kernel_variant() == v
    g.close()


# (pixels per SSAA work item -> the knobs that force the layout: tests/test_gpu_parity.py)
LAYOUTS = {16: [("ssaa_local_below", 0)],
           4: [("ssaa_local_below", 4000000000), ("ssaa_sparse_below", 0), ("ssaa_heavy_ticks", 1), ("ssaa_spread_slots", 1048576)],
           1: [("ssaa_local_below", 4000000000), ("ssaa_sparse_below", 4000000000), ("ssaa_heavy_ticks", 1)]}


@pytest.mark.parametrize("per_item", [16, 4, 1])
@pytest.mark.parametrize("cull", [1, 0])
@pytest.mark.parametrize("name", ["mixed_lights", "light_below", "sky_tiles"])
def test_ssaa_layouts(ra, oracle, images, name, cull, per_item):
    """The SSAA launch with work items of 16, 4 and 1 pixels (every tile classified as very slow for the latter two), on a cold and a warm frame."""
    import torch
    from tests.util_ssaa import check_list
    path, rays, rh, rc, p1, ref, ref_mask = reference(oracle, images, name, cull)
    g, v = plain_scene(ra, path, W, H, cull)
    for k, val in LAYOUTS[per_item]:
        g.set_knob(k, val)
    for it in range(2):
        fb = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
        mask = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
        g.render_pass1(fb)
        g.sobel(fb, mask)
        g.render_ssaa(mask, fb)
        torch.cuda.synchronize()
        nd = int((bits(ref) != bits(fb.cpu().numpy())).any(-1).sum())
        assert nd == 0, "%s, %d pixels per item, frame %d: %d pixels differ" % (name, per_item, it, nd)
        lst = g.ssaa_list()
        m = mask.cpu().numpy()
        assert lst["flagged"] == int((m[:-1, :-1] != 0).sum()) > 0
        assert lst["local"] == (per_item != 16) and (per_item == 16 or lst["sparse"] == (per_item == 1))
        wd, nf, want, spread, per = check_list(lst, g.tile_cost(), m)
        if per_item != 16:
            assert (per[nf > 0] == per_item).all() and want.any() and np.array_equal(spread, want)
    assert g.kernel_variant() == v
    g.close()


@pytest.mark.parametrize("mode", [0, 1], ids=["three_launches", "one_launch"])
@pytest.mark.parametrize("cull", [1, 0])
@pytest.mark.parametrize("name", ["mixed_lights", "light_below"])
def test_row_bands_with_halo_strips(ra, oracle, images, name, cull, mode):
    """A frame of 200 rows sharded into bands of 64 rows over 2 and 3 parts, the halo rows rendered as 64 x 1 strips (three launches: and, with the
    limit forced to 0, expanded back into tiles): the owned rows of every part are the oracle's."""
    import torch
    from rendering_amd import parallel
    w, h = 136, 200
    path, rays, rh, rc, p1, ref, ref_mask = reference(oracle, images, name, cull, w, h)
    g, v = plain_scene(ra, path, w, h, cull)
    g.set_frame_mode(mode)
    for limit in (None, 0):
        if limit is not None:
            g.set_knob("strip_limit", limit)
        for parts in (2, 3):
            acc = np.zeros((h, w, 3), np.float32)
            for part in range(parts):
                g.set_row_ownership(64, parts, part, True)
                for it in range(2):
                    fb = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
                    mask = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
                    g.render_frame(fb, mask)
                    assert g.frame_status() == 0 and g.frame_mode()[0] == mode
                rows = np.asarray(parallel.owned_rows(h, 64, parts, part))
                acc[rows] = fb.cpu().numpy()[rows]
                assert np.array_equal(mask.cpu().numpy()[rows] != 0, ref_mask[rows] != 0), "%s: mask, part %d of %d" % (name, part, parts)
            nd = int((bits(ref) != bits(acc)).any(-1).sum())
            assert nd == 0, "%s, %d parts, strip limit %s: %d pixels differ" % (name, parts, limit, nd)
    g.set_row_ownership(0, 1, 0, False)
    assert g.kernel_variant() == v
    g.close()
