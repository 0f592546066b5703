"""rtx_sobel, rtx_render_ssaa and rtx_quantize_bgr8 on inputs the renderer never produces (tests/util_image_stage.py), against the
CPU oracle -- which tests/test_image_stage_cpu.py holds to a plain numpy restatement and to the real reference on the same inputs.

Sobel: probes within 4 ulp of the threshold, edges on the columns and rows where a wave's 62 columns and 8 rows end, inf / NaN / huge /
denormal pixels, row ranges and row ownership.  SSAA: masks that fill tiles, sit on the pad-to-16 edges and on the borders and hold
bytes other than 1, through every layout of the flagged-pixel list, on a canary framebuffer: a pixel that is not re-rendered keeps its
bits.  Quantiser: every fp32 within 3 ulp of a byte boundary in every position of a thread's four pixels.  Every output buffer starts
as 0xA5 (or canaries): what a call must not write is still that afterwards."""
import numpy as np
import pytest

from tests import util_image_stage as U
from tests.util_ssaa import check_list

pytestmark = pytest.mark.gpu

CFG1 = "scenes/cfg1_simple_shapes.scene"
CFG2 = "scenes/cfg2_smooth_4k.scene"
BIG = 4000000000


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def filled(shape, dtype=None):
    import torch
    return torch.full(shape, U.CANARY, dtype=dtype or torch.uint8, device="cuda")


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


# ------------------------------------------------------------------------------------------------
# Sobel
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sobel_cases(oracle):
    """[(name, image, the oracle's mask)], computed once."""
    return [(name, img, oracle.OracleScene(CFG1, img.shape[1], img.shape[0]).sobel(img)) for name, img in U.sobel_images()]


def ranged(cases):
    """The two sizes that are also computed in parts: the 256 x 256 probes and 187 x 35 (four wave columns, five groups of rows)."""
    return [c for c in cases if c[0] == "probe" or c[0].endswith("_187x35")]


def test_sobel_every_image_byte_for_byte(ra, sobel_cases):
    """Every image through rtx_sobel into a mask of 0xA5: the oracle's bytes, the borders (0) included."""
    scenes = {}
    for name, img, ref in sobel_cases:
        H, W, _ = img.shape
        g = scenes.get((W, H)) or scenes.setdefault((W, H), ra.Scene(CFG1, W, H))
        mask = filled((H, W))
        g.sobel(dev(img), mask)
        got = host(mask)
        bad = np.argwhere(got != ref)
        assert bad.size == 0, "%s: %d mask bytes differ, first (y, x) = %s: %d, oracle %d" % (
            name, len(bad), bad[0], got[tuple(bad[0])], ref[tuple(bad[0])])


def test_sobel_row_ranges(ra, sobel_cases):
    """Row ranges that start and end inside a wave's 8 rows: the rows in range hold the oracle's bytes, every other row is untouched."""
    for name, img, ref in ranged(sobel_cases):
        H, W, _ = img.shape
        g = ra.Scene(CFG1, W, H)
        fb = dev(img)
        for r0, r1 in ((0, H), (1, 2), (7, 9), (8, 16), (5, H), (H - 1, H)):
            mask = filled((H, W))
            g.sobel(fb, mask, rows=(r0, r1))
            got = host(mask)
            assert np.array_equal(got[r0:r1], ref[r0:r1]), "%s rows %d..%d: %d bytes differ" % (name, r0, r1, int((got[r0:r1] != ref[r0:r1]).sum()))
            assert (got[:r0] == U.CANARY).all() and (got[r1:] == U.CANARY).all(), "%s rows %d..%d: a row outside was written" % (name, r0, r1)


@pytest.mark.parametrize("parts", [2, 3])
def test_sobel_row_ownership(ra, sobel_cases, parts):
    """Bands of 64 rows dealt to 2 and 3 parts: the rows a part owns hold the oracle's bytes (the neighbours across a band's edge
    are read from the framebuffer, which holds every row here)."""
    from rendering_amd.parallel import owned_rows
    for name, img, ref in ranged(sobel_cases):
        H, W, _ = img.shape
        g = ra.Scene(CFG1, W, H)
        fb = dev(img)
        seen = np.zeros(H, int)
        for part in range(parts):
            g.set_row_ownership(64, parts, part, halo=True)
            mask = filled((H, W))
            g.sobel(fb, mask)
            got = host(mask)
            rows = owned_rows(H, 64, parts, part)
            seen[rows] += 1
            assert np.array_equal(got[rows], ref[rows]), "%s part %d of %d: %d bytes differ" % (name, part, parts, int((got[rows] != ref[rows]).sum()))
        assert (seen == 1).all()


# ------------------------------------------------------------------------------------------------
# SSAA list
# ------------------------------------------------------------------------------------------------
SSAA_SIZES = [(CFG2, 136, 104), (CFG2, 61, 43), (CFG1, 9, 9), (CFG1, 8, 8), (CFG1, 2, 2)]
LAYOUTS = ["packed", "local", "sparse"]
_expected = {}


def expected(oracle, path, W, H, name, mask, fb):
    """oracle.ssaa(fb, mask) of the whole frame, computed once per scene, size and mask and never modified."""
    key = (path, W, H, name)
    if key not in _expected:
        o = _expected.get((path, W, H)) or _expected.setdefault((path, W, H), oracle.OracleScene(path, W, H))
        full = o.ssaa(fb, mask)
        full.setflags(write=False)
        _expected[key] = full
    return _expected[key]


class View:
    """One scene at one size with its canary framebuffer.  warm: pass 1 has run (into a buffer of its own), so the list is built from
    real tile costs; otherwise rtx_render_ssaa is the first call the view ever sees."""

    def __init__(self, ra, oracle, path, W, H, warm):
        import torch
        self.path, self.W, self.H, self.warm, self.oracle = path, W, H, warm, oracle
        self.g = ra.Scene(path, W, H)
        self.fb0 = U.canary_fb(W, H)
        self.fb0_dev = dev(self.fb0)
        self.calls = 0
        self.default_heavy = None
        if warm:
            first = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
            self.g.render_pass1(first)
            torch.cuda.synchronize()

    def run(self, layout, name, mask, rows=None, heavy=None, spread_slots=None):
        """rtx_render_ssaa with the layout forced, then every check of this module on the framebuffer and on the list.
        The layout of a view is decided once and kept for 16 frames; the limits are varied by one per call (far from any count
        of flagged pixels) so that every call decides anew and reports its own count."""
        g, W, H = self.g, self.W, self.H
        rows = rows or (0, H)
        self.calls += 1
        if layout == "packed":
            knobs = [("ssaa_local_below", 0), ("ssaa_sparse_below", self.calls)]
        else:
            knobs = [("ssaa_local_below", BIG - self.calls), ("ssaa_sparse_below", BIG if layout == "sparse" else 0)]
        if heavy is not None:
            knobs.append(("ssaa_heavy_ticks", heavy))
        elif self.default_heavy is not None:
            knobs.append(("ssaa_heavy_ticks", self.default_heavy))
        if spread_slots is not None:
            knobs.append(("ssaa_spread_slots", spread_slots))
        for k, v in knobs:
            g.set_knob(k, v)
        fb = self.fb0_dev.clone()
        g.render_ssaa(dev(mask), fb, rows=rows)
        got = host(fb)
        what = "%s %dx%d %s %s rows %s heavy %s%s" % (self.path, W, H, layout, name, rows, heavy, " warm" if self.warm else " cold")
        want = U.ssaa_expected(None, self.fb0, mask, rows, full=expected(self.oracle, self.path, W, H, name, mask, self.fb0))
        bad = np.argwhere((got.view(np.int32) != want.view(np.int32)).any(-1))
        assert bad.size == 0, "%s: %d pixels differ, first (y, x) = %s" % (what, len(bad), bad[0])
        flagged = U.ssaa_flagged(mask, rows)
        lst = g.ssaa_list()
        if heavy is None and self.default_heavy is None:
            self.default_heavy = lst["heavy_ticks"]
        cost = g.tile_cost()
        assert lst["local"] == (layout != "packed") and (layout == "packed" or lst["sparse"] == (layout == "sparse")), what
        assert lst["flagged"] == int(flagged.sum()), "%s: the list counts %d flagged pixels, the mask has %d" % (what, lst["flagged"], int(flagged.sum()))
        if heavy is not None:
            assert lst["heavy_ticks"] == heavy
        if spread_slots is not None:
            assert lst["spread_slots"] == spread_slots
        wd, nf, _, _, _ = check_list(lst, cost, flagged)
        assert int(nf.sum()) == int(flagged.sum()) and (wd >= nf).all(), what
        return lst, cost, wd, nf


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("path,W,H", SSAA_SIZES)
def test_ssaa_every_mask_every_layout(ra, oracle, path, W, H, layout):
    """Every mask of ssaa_masks through one layout of the list, on a view that never ran pass 1 (its tile costs are the estimate made
    when the view was set, not measurements), and after pass 1 with the default
    threshold for a slow tile and with a threshold of one tick (every tile slow: 4 pixels or one pixel per wave).  The framebuffer is
    ssaa_expected bit for bit -- unflagged pixels, the last row and the last column keep their canaries --, the list passes check_list
    and counts exactly the flagged pixels x < W-1, y < H-1."""
    masks = U.ssaa_masks(W, H, seed=W * 1000 + H)
    cold, warm = View(ra, oracle, path, W, H, False), View(ra, oracle, path, W, H, True)
    estimate = None
    for name, mask in masks.items():
        lst, cost, _, _ = cold.run(layout, name, mask)
        # (no pass 1 has measured a tile: the list is built from the first-frame estimate of the view, the same for every call)
        estimate = cost if estimate is None else estimate
        assert np.array_equal(cost, estimate)
        warm.run(layout, name, mask)
        lst, cost, wd, nf = warm.run(layout, name, mask, heavy=1)
        if layout != "packed" and nf.any():
            assert (cost.ravel()[nf > 0] > lst["very"]).all()
            per = 1 if layout == "sparse" else lst["spread_px"]
            assert np.array_equal(wd, (nf + per - 1) // per * 16), "%s: every tile is very slow and the budget covers all" % name
    assert cold.default_heavy == warm.default_heavy and cold.default_heavy > 1


@pytest.mark.parametrize("layout", LAYOUTS)
def test_ssaa_row_ranges(ra, oracle, layout):
    """Row ranges that cut tiles (3..21, the single row 8, the last row alone: nothing to do) on the dense masks and the pad-to-16
    ones: rows outside the range keep their canaries, and the list holds the range's pixels only."""
    for path, W, H in SSAA_SIZES[:2]:
        masks = U.ssaa_masks(W, H, seed=W * 1000 + H)
        warm = View(ra, oracle, path, W, H, True)
        for name in U.DENSE_MASKS + ("tile_15", "tile_16", "bernoulli_1_4", "row_0", "last_row", "tile_bit_63"):
            for rows in ((0, H), (3, 21), (8, 9), (H - 1, H)):
                warm.run(layout, name, masks[name], rows=rows)
                warm.run(layout, name, masks[name], rows=rows, heavy=1)


@pytest.mark.parametrize("spread_slots", [1048576, 4096, 0])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_ssaa_dense_masks_and_the_slot_budget(ra, oracle, layout, spread_slots):
    """The dense masks with every tile classified very slow, so that every tile asks for 4x or 16x its slots, under a full, a partly
    and a fully exhausted slot budget: the list never overruns its budget (check_list) and the frame is unchanged."""
    path, W, H = SSAA_SIZES[0]
    masks = U.ssaa_masks(W, H, seed=W * 1000 + H)
    warm = View(ra, oracle, path, W, H, True)
    for name in U.DENSE_MASKS:
        lst, cost, wd, nf = warm.run(layout, name, masks[name], heavy=1, spread_slots=spread_slots)
        extra = int((wd - (nf + 15) // 16 * 16).sum()) if layout != "packed" else 0
        assert extra <= spread_slots
        if layout != "packed" and spread_slots == 4096:
            assert 0 < extra, "%s: no tile got spread slots" % name
        if spread_slots == 0 and layout != "packed":
            assert np.array_equal(wd, (nf + 15) // 16 * 16)


# ------------------------------------------------------------------------------------------------
# Quantiser
# ------------------------------------------------------------------------------------------------
def quantize(ra, oracle, fb, ownership=None):
    H, W, _ = fb.shape
    g = ra.Scene(CFG1, W, H)
    if ownership:
        g.set_row_ownership(*ownership)
    out = filled((H * W * 3,))
    g.quantize(dev(fb), out)
    return host(out), np.frombuffer(oracle.encode_bmp(fb)[54:], np.uint8)


def test_quantize_every_byte_boundary(ra, oracle):
    """The table: every fp32 within 3 ulp of k / 255, the zeros, denormals, 1 -+ ulp, values outside [0, 1], infinities and NaNs of
    both signs, each in every channel and in each of a thread's four pixels."""
    table = U.quant_table()
    got, ref = quantize(ra, oracle, table)
    bad = np.nonzero(got != ref)[0]
    if bad.size:
        y, x, ch = np.unravel_index(bad[0], table.shape)
        v = table[::-1, :, ::-1][y, x, ch]
        raise AssertionError("%d bytes differ; first: %r (0x%08x) -> %d, oracle %d" % (bad.size, v, U.bits(v), got[bad[0]], ref[bad[0]]))


@pytest.mark.parametrize("W,H", U.QUANT_SIZES + [(4, 2)])
def test_quantize_random_frames(ra, oracle, W, H):
    """Random frames (no canaries: half of the floats are table values) at sizes of one thread, of a few and of rows that end inside a
    block.  A view of height 1 does not exist on the device (rtx_scene_set_view refuses a dimension below 2, and the call takes its
    size from the view), so 4 x 1 is held to that refusal and 4 x 2 is the smallest frame converted; the oracle's 4 x 1 is pinned to
    the restatement in tests/test_image_stage_cpu.py."""
    fb = U.quant_frame(W, H, seed=W * 100 + H)
    if min(W, H) < 2:
        with pytest.raises(ra.RtxError, match="width/height must be >= 2"):
            quantize(ra, oracle, fb)
        return
    got, ref = quantize(ra, oracle, fb)
    assert np.array_equal(got, ref), "%d bytes differ" % int((got != ref).sum())


def test_quantize_row_ownership(ra, oracle):
    """64 x 9, bands of 4 rows, 2 parts: the image rows a part owns are converted (row y is stored at H-1-y), the others still 0xA5."""
    from rendering_amd.parallel import owned_rows
    W, H = 64, 9
    fb = U.quant_frame(W, H, seed=7)
    for part in range(2):
        got, ref = quantize(ra, oracle, fb, ownership=(4, 2, part, True))
        got, ref = got.reshape(H, W * 3), ref.reshape(H, W * 3)
        mine = np.zeros(H, bool)
        mine[H - 1 - owned_rows(H, 4, 2, part)] = True
        assert mine.any() and not mine.all()
        assert np.array_equal(got[mine], ref[mine]) and (got[~mine] == U.CANARY).all()


@pytest.mark.parametrize("W", [61, 62, 63])
def test_quantize_refuses_widths_that_are_no_multiple_of_four(ra, W):
    H = 5
    g = ra.Scene(CFG1, W, H)
    out = filled((H * W * 3 + 16,))
    with pytest.raises(ra.RtxError):
        g.quantize(dev(U.quant_frame(W, H, seed=W)), out)
    assert (host(out) == U.CANARY).all()
