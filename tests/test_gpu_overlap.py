"""Frames of a sequence overlapped on two streams, as a caller rendering a camera path does (bench.py --pipelined): pass 1 + Sobel of
frame k + 1 on stream A beside the SSAA launch of frame k on stream B, two framebuffers, events between them.  Every frame must equal the
serial frame bit for bit (framebuffer and mask).  The SSAA work list of frame k is built while pass 1 of frame k + 1 rewrites the tile
costs it is ordered by (rtxSsaaCountKernel / rtxSsaaScatterKernel): the heavy threshold is put at the median cost of the tiles with
flagged pixels, so that many of them cross it from one frame to the next."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FRAMES = 24

CASES = [("scenes/cfg2_smooth_250k.scene", 4096, 4096, 1), ("scenes/cfg2_smooth_250k.scene", 4096, 4096, 0),
         ("scenes/r6_ref_bunny.scene", 4096, 4096, None)]


@pytest.mark.parametrize("path,W,H,cull", CASES)
def test_overlapped_frames_equal_the_serial_frame(ra, path, W, H, cull):
    import torch
    g = ra.Scene(path, W, H)
    if cull is not None:
        g.set_flag("useBackfaceCulling", cull)
    assert g.kernel_variant()["cull"] == bool(cull if cull is not None else g.view_flags() & 1)
    fb = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    mask = torch.zeros((H, W), dtype=torch.uint8, device="cuda")

    def serial():
        g.render_pass1(fb)
        g.sobel(fb, mask)
        g.render_ssaa(mask, fb)
        torch.cuda.synchronize()

    for _ in range(2):          # (warm: measured tile costs)
        serial()
    cost = g.tile_cost()
    tx = cost.shape[1]
    flagged = np.zeros(cost.size, bool)
    ys, xs = np.nonzero(mask.cpu().numpy())
    flagged[(ys // 8) * tx + xs // 8] = True
    heavy = int(np.median(cost.ravel()[flagged]))
    g.set_knob("ssaa_heavy_ticks", heavy)
    serial()                    # the reference, with the knob set (no knob changes a pixel)
    ref_fb, ref_mask = fb.clone(), mask.clone()
    ref_i = ref_fb.view(torch.int32)

    fbs = [fb, torch.zeros_like(fb)]
    masks = [mask, torch.zeros_like(mask)]
    sA, sB = torch.cuda.Stream(), torch.cuda.Stream()
    free = [None, None]
    diff = torch.zeros((FRAMES, 2), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    for k in range(FRAMES):
        i = k & 1
        if free[i] is not None:
            sA.wait_event(free[i])          # frame k - 2 has left this framebuffer (and been compared)
        g.render_pass1(fbs[i], stream=sA)
        g.sobel(fbs[i], masks[i], stream=sA)
        e = torch.cuda.Event()
        e.record(sA)
        sB.wait_event(e)
        g.render_ssaa(masks[i], fbs[i], stream=sB)
        with torch.cuda.stream(sB):
            diff[k, 0] = (fbs[i].view(torch.int32) != ref_i).any(-1).sum()
            diff[k, 1] = (masks[i] != ref_mask).sum()
        free[i] = torch.cuda.Event()
        free[i].record(sB)
    torch.cuda.synchronize()
    d = diff.cpu().numpy()
    lst = g.ssaa_list()
    g.close()
    bad = np.nonzero(d.any(1))[0]
    assert len(bad) == 0, "%s (culling %s, heavy threshold %d ticks): %d of %d overlapped frames differ from the serial frame; pixels per frame %s, mask pixels %s" % (
        path, cull, heavy, len(bad), FRAMES, d[:, 0].tolist(), d[:, 1].tolist())
    assert lst["heavy_ticks"] == heavy
