"""State around a mesh walk of the PLAIN pass-1 and colour kernels (traceWave / castRayPlainWave, rendering_amd/csrc/rtx_kernels.hip).  What a wave needs again
after a walk is partly kept and partly fetched or derived again -- the object's record and flag word, the lane sets of a trace, the light's record, the
tile loop's scalars -- and a value that comes back wrong or stale shows as a wrong pixel.  So every case is compared with the oracle bit for bit: the frame's
own primary rays through rtx_trace_rays (the colour kernel), pass 1 alone, and the frame in three launches, with culling on and off and with and without the
box test of the prune records.  Frames of at most 72 x 56 pixels (tests/util_round_state.py, which asserts on the oracle what makes each case its case):

  objects    two meshes with a plane and a sphere between them in scene order; each of the four is the nearest hit of some pixel and casts a shadow on one
  irregular  a frame odd in both dimensions under an unrotated camera: rays with a zero direction component (walked apart, in the binary form) share
             8 x 8 tiles with rays that have none
  wide       16 x 16 pixels at a 120-degree field of view: the rays of a tile fan out over 60 degrees, so the split rule halves the bundles (up to
             RTX_MAX_SPLITS times).  A product build cannot count splits.  Checked once with a diagnostic build (-DRTX_DBG=1) of the same sources: one pass 1 of
             this frame makes 86 wide walks with culling and 92 without (with and without the box records alike), where 4 tiles x 3 rounds (the primary trace
             and two lights) x 4 meshes = 48 is the most there can be without a split (profiles/round_state_ab.txt).  What is asserted here is the geometry the
             rule looks at: every tile's direction box, at the distance of the nearest hit, is wider than a torus
  lights     nine lights: eight point lights (six have a source copy of the prune records), a distant light between them, one under the floor so that
             tiles of pure floor have a round with nothing to trace
  tiles      63 tiles (no multiple of RTX_POP_MANY: the cheap half's batches end unevenly), rendered whole, as a rows=(y0, y1) range and as row bands
             with halo strips"""
import numpy as np
import pytest

from tests import util_round_state as RS
from tests import util_shading as U

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def images(tmp_path_factory):
    d = U.short_dir(tmp_path_factory)
    U.write_images(d)
    return d


_oracle = {}


def reference(oracle, images, name, cull):
    """path, and the oracle's rays, probe records and colours, pass 1, frame and mask of the case (the same for either BOXES: computed once)."""
    key = (name, cull)
    if key not in _oracle:
        path = RS.write_scene(name, images, cull)
        c = RS.CASES[name]
        o = oracle.OracleScene(path, c["w"], c["h"])
        rays = U.primary_rays(o)
        rh, rc = o.probe(rays)
        RS.expectations(name, o, rays, rh)
        p1 = o.pass1()
        mask = o.sobel(p1)
        mask[0, :] = 0; mask[-1, :] = 0; mask[:, 0] = 0; mask[:, -1] = 0       # (border = 0 by definition)
        rows = (13, 42)
        _oracle[key] = (path, rays, rh, rc, p1, o.ssaa(p1), mask, rows, o.pass1(rows) if name == "tiles" else None)
        o.close()
    return _oracle[key]


def plain_scene(ra, path, w, h, cull, boxes):
    g = ra.Scene(path, w, h)
    g.set_knob("prune_boxes", boxes)
    v = g.kernel_variant()
    assert v["plain"] and not v["analytic"] and not v["stats"] and v["cull"] == bool(cull) and v["boxes"] == bool(boxes), v
    return g, v


@pytest.mark.parametrize("boxes", [1, 0])
@pytest.mark.parametrize("cull", [1, 0])
@pytest.mark.parametrize("name", sorted(RS.CASES))
def test_round_state(ra, oracle, images, name, cull, boxes):
    import torch
    path, rays, rh, rc, p1, ref, ref_mask, rows, p1_rows = reference(oracle, images, name, cull)
    w, h = RS.CASES[name]["w"], RS.CASES[name]["h"]
    g, v = plain_scene(ra, path, w, h, cull, boxes)
    gh, gc = g.trace_rays(torch.from_numpy(rays).cuda())
    torch.cuda.synchronize()
    gh, gc = gh.cpu().numpy(), gc.cpu().numpy()
    bad = (bits(rh) != bits(gh)).any(1) | (bits(rc) != bits(gc)).any(1)
    assert not bad.any(), "%s: %d of %d rays differ, first %d: oracle %s %s gpu %s %s" % (
        name, int(bad.sum()), len(rays), int(np.argmax(bad)), rh[np.argmax(bad)], rc[np.argmax(bad)], gh[np.argmax(bad)], gc[np.argmax(bad)])

    def frame(**kw):
        fb = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
        mask = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
        g.render_frame(fb, mask, **kw)
        assert g.frame_status() == 0 and g.frame_mode()[0] == 0
        return fb.cpu().numpy(), mask.cpu().numpy()

    for it in range(2):                     # (the second pass 1 knows the tile costs of the first: the queues are ordered by them)
        fb = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
        g.render_pass1(fb)
        torch.cuda.synchronize()
        nd = int((bits(p1) != bits(fb.cpu().numpy())).any(-1).sum())
        assert nd == 0, "%s, pass 1, frame %d: %d pixels differ" % (name, it, nd)
    g.set_frame_mode(0)
    got, mask = frame()
    nd = int((bits(ref) != bits(got)).any(-1).sum())
    assert nd == 0, "%s in three launches: %d pixels differ" % (name, nd)
    assert np.array_equal(mask != 0, ref_mask != 0), "%s in three launches: mask differs" % name
    if name == "tiles":
        from rendering_amd import parallel
        fb = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
        g.render_pass1(fb, rows=rows)
        torch.cuda.synchronize()
        got = fb.cpu().numpy()
        assert (got[:rows[0]] == 0).all() and (got[rows[1]:] == 0).all()
        nd = int((bits(p1_rows) != bits(got)).any(-1).sum())
        assert nd == 0, "tiles, pass 1 of rows %s: %d pixels differ" % (rows, nd)
        # bands of 16 rows dealt to 2 and 3 parts, the halo rows either side of a band rendered as 64 x 1 strips
        for parts in (2, 3):
            acc = np.zeros((h, w, 3), np.float32)
            for part in range(parts):
                g.set_row_ownership(16, parts, part, True)
                got, mask = frame()
                own = np.asarray(parallel.owned_rows(h, 16, parts, part))
                acc[own] = got[own]
                assert np.array_equal(mask[own] != 0, ref_mask[own] != 0), "tiles: mask, part %d of %d" % (part, parts)
            nd = int((bits(ref) != bits(acc)).any(-1).sum())
            assert nd == 0, "tiles, %d parts: %d pixels differ" % (parts, nd)
        g.set_row_ownership(0, 1, 0, False)
    assert g.kernel_variant() == v
    g.close()
