"""rtx_render_frame (pass 1 + Sobel + SSAA as one call; one launch with per-tile dependencies, or three launches):
the framebuffer and the mask must equal, bit for bit, what rtx_render_pass1 ; rtx_sobel ; rtx_render_ssaa produce --
in either mode, on cold and warm frames (warm frames split their slowest tiles), on row ranges and on row bands of a
sharded frame -- and the CPU oracle on bands.  Through the C ABI, device-resident buffers."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SPLIT, FUSED, AUTO = 0, 1, -1


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def stages(torch, g, rows=None, parts=1, part=0):
    H, W = g.height, g.width
    fb = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    mask = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
    g.set_row_ownership(64 if parts > 1 else 0, parts, part, True)
    g.render_pass1(fb, rows=rows)
    g.sobel(fb, mask, rows=rows)
    g.render_ssaa(mask, fb, rows=rows)
    torch.cuda.synchronize()
    return fb, mask


def frame(torch, g, mode, rows=None, parts=1, part=0, mask_fill=0):
    H, W = g.height, g.width
    fb = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    mask = torch.full((H, W), mask_fill, dtype=torch.uint8, device="cuda")
    g.set_row_ownership(64 if parts > 1 else 0, parts, part, True)
    g.set_frame_mode(mode)
    g.render_frame(fb, mask, rows=rows)
    assert g.frame_status() == 0
    if mode != AUTO:
        assert g.frame_mode()[0] == mode
    return fb, mask


def same(torch, a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


CASES = [("scenes/cfg1_simple_shapes.scene", 96, 64), ("scenes/cfg1_simple_shapes.scene", 257, 131), ("scenes/cfg2_smooth_4k.scene", 200, 120),
         ("scenes/cfg3_reflective_refractive.scene", 160, 90), ("scenes/cfg4_textured_256.scene", 128, 128), ("scenes/mixed_materials.scene", 120, 72),
         ("scenes/area_light.scene", 64, 48), ("scenes/uv_out_of_range.scene", 96, 96)]


@pytest.mark.parametrize("path,W,H", CASES)
def test_frame_equals_three_stages(ra, torch_cuda, path, W, H):
    torch = torch_cuda
    g = ra.Scene(path, W, H)
    ref_fb, ref_mask = stages(torch, g)
    for mode in (FUSED, SPLIT):
        for it in range(4):              # cold frame, then warm ones (tile costs known: slow tiles are split, SSAA items shrink)
            fb, mask = frame(torch, g, mode, mask_fill=9 if it == 0 else 0)
            assert same(torch, ref_fb, fb), "%s mode %d frame %d: framebuffer differs" % (path, mode, it)
            assert torch.equal(ref_mask, mask), "%s mode %d frame %d: mask differs" % (path, mode, it)
    g.set_frame_mode(AUTO)


def test_frame_everything_split(ra, torch_cuda):
    """Every tile rendered as sixteen 2x2 parts and every flagged pixel as its own SSAA item (limits forced to the floor): the limits read
    back follow rtxTileOrderKernel's rule from the previous frame's tile costs, and some tile really is over them."""
    torch = torch_cuda
    g = ra.Scene("scenes/cfg2_smooth_4k.scene", 136, 104)
    g.set_knob("split_percent", 1)
    ref_fb, ref_mask = stages(torch, g)
    over = 0
    for it in range(3):
        prev = g.tile_cost().astype(np.int64)      # (what the frame's limits are derived from: the costs of the frame before)
        fb, mask = frame(torch, g, FUSED)
        assert same(torch, ref_fb, fb) and torch.equal(ref_mask, mask)
        lst = g.ssaa_list()
        assert lst["cost_sum"] == int(prev.sum()) > 0 and lst["frame_waves"] > 0
        split4 = max(2000, min(0x0fffffff, lst["cost_sum"] // lst["frame_waves"] * 1 // 100))
        assert (lst["split4"], lst["split16"]) == (split4, 4 * split4), "frame %d: limits %s" % (it, (lst["split4"], lst["split16"]))
        over += int((prev > split4).sum())
    assert over > 0, "no tile was over the split limit: the split path never ran"
    g.set_knob("split_percent", 0)      # and never
    fb, mask = frame(torch, g, FUSED)
    assert same(torch, ref_fb, fb) and torch.equal(ref_mask, mask)
    lst = g.ssaa_list()
    assert (lst["split4"], lst["split16"]) == (0xffffffff, 0xffffffff)


def test_frame_row_ranges_and_bands(ra, torch_cuda):
    """Row ranges (the other rows keep what they held) and the row bands of a sharded frame, one launch against three."""
    torch = torch_cuda
    g = ra.Scene("scenes/cfg2_smooth_4k.scene", 160, 200)
    g.set_knob("verify_lists", 1)      # (every list the calls below cause is also compared with the host's construction)
    for rows in ((0, 200), (0, 64), (37, 150), (192, 200), (199, 200)):
        ref_fb, ref_mask = stages(torch, g, rows=rows)
        for it in range(2):
            fb, mask = frame(torch, g, FUSED, rows=rows)
            assert same(torch, ref_fb, fb), "rows %s" % (rows,)
            assert torch.equal(ref_mask[rows[0]:rows[1]], mask[rows[0]:rows[1]]), "mask rows %s" % (rows,)
    for parts in (2, 3):
        for part in range(parts):
            ref_fb, ref_mask = stages(torch, g, parts=parts, part=part)
            for it in range(2):
                fb, mask = frame(torch, g, FUSED, parts=parts, part=part)
                assert same(torch, ref_fb, fb), "part %d of %d" % (part, parts)
                assert torch.equal(ref_mask, mask), "mask, part %d of %d" % (part, parts)
    g.set_row_ownership(0, 1, 0, False)
    g.set_frame_mode(AUTO)


def test_frame_mode_is_measured(ra, torch_cuda):
    """Left to itself the call tries both ways on warm frames, reports what it measured and settles on the faster."""
    torch = torch_cuda
    g = ra.Scene("scenes/cfg2_smooth_4k.scene", 320, 200)
    ref_fb, ref_mask = stages(torch, g)
    seen = set()
    for it in range(10):
        fb, mask = frame(torch, g, AUTO)
        torch.cuda.synchronize()
        seen.add(g.frame_mode()[0])
        assert same(torch, ref_fb, fb) and torch.equal(ref_mask, mask)
    mode, split_ms, fused_ms = g.frame_mode()
    assert seen == {0, 1}
    assert split_ms > 0 and fused_ms > 0
    assert mode == (1 if fused_ms <= split_ms else 0)


def test_frame_statistics_need_the_stages(ra, torch_cuda):
    torch = torch_cuda
    g = ra.Scene("scenes/cfg1_simple_shapes.scene", 64, 64)
    fb = torch.zeros((64, 64, 3), dtype=torch.float32, device="cuda"); mask = torch.zeros((64, 64), dtype=torch.uint8, device="cuda")
    g.counters_enable(True)
    with pytest.raises(ra.RtxError):
        g.render_frame(fb, mask)
    g.counters_enable(False)
    g.render_frame(fb, mask)
    assert g.frame_status() == 0


def test_frame_1080p_against_oracle_bands(ra, oracle, torch_cuda):
    """250k-triangle scene at 1920x1080 in one launch (warm: the pole tiles are split) against the CPU oracle's bands."""
    from rendering_amd import assets
    torch = torch_cuda
    assets.ensure(["bumpy_250k.obj"])
    g = ra.Scene("scenes/cfg2_smooth_250k.scene", 1920, 1080)
    ref_fb, ref_mask = stages(torch, g)
    for it in range(3):
        fb, mask = frame(torch, g, FUSED)
        assert same(torch, ref_fb, fb) and torch.equal(ref_mask, mask), "frame %d" % it
    o = oracle.OracleScene("scenes/cfg2_smooth_250k.scene", 1920, 1080)
    p1 = torch.zeros_like(fb); g.render_pass1(p1); torch.cuda.synchronize()
    p1 = p1.cpu().numpy(); got = fb.cpu().numpy(); gm = mask.cpu().numpy()
    bands = [(204, 212), (536, 544), (864, 872)]
    band_mask = np.zeros_like(gm)
    for y0, y1 in bands:
        band_mask[y0:y1] = gm[y0:y1]
    assert band_mask.any()
    ref = o.ssaa(p1, band_mask)
    for y0, y1 in bands:
        assert np.array_equal(np.ascontiguousarray(ref[y0:y1], np.float32).view(np.uint32), np.ascontiguousarray(got[y0:y1], np.float32).view(np.uint32)), "rows %d..%d" % (y0, y1)


def test_halo_strips_and_their_expansion(ra, torch_cuda, monkeypatch):
    """Three-launch path of a sharded frame: halo rows rendered as 64x1 strips (cold frame), as strips ordered by cost
    (warm frame), and -- with the limit forced to 0 -- expanded back into tiles: always the pixels of the unsharded frame."""
    from rendering_amd import parallel
    torch = torch_cuda
    W, H = 200, 330
    g = ra.Scene("scenes/cfg2_smooth_4k.scene", W, H)
    g.set_knob("verify_lists", 1)      # (every list the calls below cause is also compared with the host's construction)
    g.set_frame_mode(SPLIT)
    full, full_mask = stages(torch, g)
    for limit in (None, "0"):
        if limit is not None:
            g.set_knob("strip_limit", int(limit))
        for parts in (2, 3):
            acc = torch.zeros_like(full)
            for part in range(parts):
                for it in range(3):
                    fb, mask = frame(torch, g, SPLIT, parts=parts, part=part)
                rows = torch.as_tensor(parallel.owned_rows(H, 64, parts, part), device="cuda")
                acc.index_copy_(0, rows, fb.index_select(0, rows))
                assert torch.equal(mask.index_select(0, rows), full_mask.index_select(0, rows)), "mask, part %d of %d" % (part, parts)
            assert same(torch, full, acc), "%d parts, strip limit %s" % (parts, limit)
    g.set_row_ownership(0, 1, 0, False)
    g.set_frame_mode(AUTO)
