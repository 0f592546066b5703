"""rtx_render_views / Scene.render_views on the device: every view of a batch against the three launches of the one-view path on a second scene
of the same file (bit for bit, framebuffer and mask), against the oracle, and what the call must leave alone -- the scene's own view, its tile
costs and timings, the last row and column of every view, and every byte outside the views' buffers."""
import os

import numpy as np
import pytest
import torch

from tests import util_shading as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (width, height): a tile and less, views without a rendered pixel, no multiples of 8, a wide and a tall view, several tiles each way;
# the two 64 x 48 views also share their pose
SIZES = [(7, 5), (1, 1), (2, 2), (41, 27), (200, 8), (8, 200), (64, 48), (64, 48), (33, 17), (96, 64), (1, 40)]
POSES = [((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)), ((0.15, 0.1, 0.2), (-4.0, 9.0, 2.0)), ((-0.3, 0.25, 0.4), (3.0, -14.0, -1.0)), ((0.0, 0.6, -0.5), (-25.0, 0.0, 0.0)),
         ((0.1, 0.0, 0.3), (0.0, 35.0, 0.0)), ((-0.2, 0.1, 0.1), (10.0, -30.0, 5.0)), ((0.05, 0.2, 0.6), (-6.0, 4.0, 0.0)), ((0.05, 0.2, 0.6), (-6.0, 4.0, 0.0)),
         ((0.3, 0.3, 0.0), (-12.0, 20.0, -8.0)), ((0.0, 0.1, 0.8), (2.0, -3.0, 1.0)), ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def family(tmp_path_factory):
    return S.write_family(S.short_dir(tmp_path_factory))


def path_of(name, family):
    return family[name] if name in S.FAMILY else "scenes/%s.scene" % name


def loop(ra, path, cams, sizes):
    """The yardstick: every view through resize + set_camera + render_pass1 + sobel + render_ssaa on a scene of its own.  Per view the framebuffer
    after pass 1, the final one and the mask.  (The one-view calls take no view under 2 x 2: such a view has no pixel to render and no interior.)"""
    g = ra.Scene(path, 16, 16)
    g.gpu()
    g.set_frame_mode(0)
    out = []
    for (pos, rot), (w, h) in zip(cams, sizes):
        fb = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
        mask = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
        if w < 2 or h < 2:
            out.append((fb.cpu().numpy(), fb.cpu().numpy(), mask.cpu().numpy()))
            continue
        g.resize(w, h)
        g.set_camera(pos, rot)
        g.render_pass1(fb)
        p1 = fb.cpu().numpy()
        g.sobel(fb, mask)
        g.render_ssaa(mask, fb)
        out.append((p1, fb.cpu().numpy(), mask.cpu().numpy()))
    g.close()
    return out


def batch(g, cams, sizes, ssaa, fill=0.0):
    fbs = [torch.full((h, w, 3), fill, dtype=torch.float32, device="cuda") for w, h in sizes]
    masks = [torch.full((h, w), 7, dtype=torch.uint8, device="cuda") for w, h in sizes]      # (a sentinel: with SSAA every byte is written)
    g.render_views(cams, fbs, masks if ssaa else None, ssaa=ssaa)
    torch.cuda.synchronize()
    return [f.cpu().numpy() for f in fbs], [m.cpu().numpy() for m in masks]


def compare(got_fb, got_mask, want, ssaa, label):
    for i, (p1, full, mask) in enumerate(want):
        ref = full if ssaa else p1
        nd = int((bits(got_fb[i]) != bits(ref)).any(-1).sum())
        assert nd == 0, "%s view %d (%s): %d pixels differ from the one-view calls" % (label, i, ref.shape, nd)
        if ssaa:
            assert np.array_equal(got_mask[i], mask), "%s view %d: %d mask bytes differ" % (label, i, int((got_mask[i] != mask).sum()))


@pytest.mark.parametrize("name", ["cfg1_simple_shapes", "cfg2_smooth_4k", "mixed_materials", "area_light", "cfg4_textured_256", "mixed"])
def test_every_view_equals_the_three_launches(ra, family, name):
    """(`mixed`: the shading family's scene with every material, maps and the skybox flag on.)"""
    path = path_of(name, family)
    g = ra.Scene(path, 24, 16)
    base = g.camera_pose()
    cams = [(tuple(float(x) for x in base[0] + np.float32(p)), tuple(float(x) for x in base[1] + np.float32(r))) for p, r in POSES]
    want = loop(ra, path, cams, SIZES)
    assert sum(int(m.sum()) for _, _, m in want) > 50, "the batch flags too few pixels to test the 4-sample pass"
    assert any((bits(p1) != bits(full)).any() for p1, full, _ in want)
    for ssaa in (False, True):
        fbs, masks = batch(g, cams, SIZES, ssaa)
        compare(fbs, masks, want, ssaa, "%s ssaa=%d" % (name, ssaa))
    # the two views of one pose and size got the same picture
    assert np.array_equal(bits(fbs[6]), bits(fbs[7])) and np.array_equal(masks[6], masks[7])
    # one tensor for the whole batch
    n = 5
    fb4 = torch.zeros((n, 24, 40, 3), dtype=torch.float32, device="cuda"); m3 = torch.zeros((n, 24, 40), dtype=torch.uint8, device="cuda")
    g.render_views(cams[:n], fb4, m3, ssaa=True)
    torch.cuda.synchronize()
    want4 = loop(ra, path, cams[:n], [(40, 24)] * n)
    compare(list(fb4.cpu().numpy()), list(m3.cpu().numpy()), want4, True, "%s (N, H, W, 3)" % name)
    g.close()


def test_a_batch_of_many_times_the_waves(ra):
    """300 views of 72 x 56 = 18 900 items, three times the waves of a full pass-1 grid (at most six blocks of four on each of 256 CUs): every
    wave pops the queue several times, and so do the waves of the 4-sample pass."""
    path = "scenes/cfg2_smooth_4k.scene"
    n, vw, vh = 300, 72, 56
    g = ra.Scene(path, 24, 16)
    base = g.camera_pose()
    cams = [(tuple(float(x) for x in base[0] + np.float32([0.002 * k, 0.001 * k, 0.0])), tuple(float(x) for x in base[1] + np.float32([0.0, 0.3 * k - 40.0, 0.0])))
            for k in range(n)]
    sizes = [(vw, vh)] * n
    want = loop(ra, path, cams, sizes)
    fb = torch.zeros((n, vh, vw, 3), dtype=torch.float32, device="cuda"); mask = torch.zeros((n, vh, vw), dtype=torch.uint8, device="cuda")
    g.render_views(cams, fb, mask, ssaa=True)
    torch.cuda.synchronize()
    compare(list(fb.cpu().numpy()), list(mask.cpu().numpy()), want, True, "300 views")
    g.close()


def rewritten(src, pos, rot, fov):
    lines = src.split("\n")
    i = lines.index("[options]")
    j = next(k for k in range(i + 1, len(lines)) if lines[k].startswith("["))
    keep = [l for l in lines[i + 1:j] if not l.startswith(("position=", "rotation=") + (("fov=",) if fov is not None else ()))]
    lines[i + 1:j] = keep + ["position=%r,%r,%r" % pos, "rotation=%r,%r,%r" % rot] + (["fov=%r" % fov] if fov is not None else [])
    return "\n".join(lines)


def test_against_the_oracle(ra, oracle, tmp_path):
    src = open("scenes/mixed_materials.scene").read()
    views = [((0.3, 0.4, 1.0), (-8.0, 12.0, 3.0), None, 120, 88), ((0.1, 0.5, 0.8), (-12.0, -6.0, 0.0), 95.0, 97, 61)]
    g = ra.Scene("scenes/mixed_materials.scene", 32, 32)
    fbs = [torch.zeros((h, w, 3), dtype=torch.float32, device="cuda") for _, _, _, w, h in views]
    masks = [torch.zeros((h, w), dtype=torch.uint8, device="cuda") for _, _, _, w, h in views]
    g.render_views([(p, r, f) for p, r, f, _, _ in views], fbs, masks, ssaa=True)
    torch.cuda.synchronize()
    for k, (pos, rot, fov, w, h) in enumerate(views):
        p = tmp_path / ("v%d.scene" % k)
        p.write_text(rewritten(src, pos, rot, fov))
        o = oracle.OracleScene(str(p), w, h)
        ref = o.ssaa(o.pass1())
        o.close()
        d = (bits(fbs[k].cpu().numpy()) != bits(ref)).any(-1)
        d[0, :] = False; d[:, 0] = False          # (the reference's uninitialised mask border)
        assert not d.any(), "view %d: %d pixels differ from the oracle" % (k, int(d.sum()))
    g.close()


def test_the_scene_is_left_as_it_was(ra):
    w, h = 160, 120
    g = ra.Scene("scenes/cfg2_smooth_4k.scene", w, h)
    g.set_frame_mode(0)
    fb = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda"); mask = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
    for _ in range(2):
        fb.zero_()
        g.render_frame(fb, mask)
    torch.cuda.synchronize()
    before = (fb.cpu().numpy(), mask.cpu().numpy())
    cost, mode, ms = g.tile_cost(), g.frame_mode(), g.last_kernel_ms(0)
    cam = g.camera()
    cams = [(p, r) for p, r in POSES[:6]]
    batch(g, cams, SIZES[:6], True)
    assert np.array_equal(g.tile_cost(), cost) and g.frame_mode() == mode and g.last_kernel_ms(0) == ms
    assert all(np.array_equal(a, b) for a, b in zip(cam, g.camera()))
    fb.zero_(); mask.zero_()
    g.render_frame(fb, mask)
    torch.cuda.synchronize()
    assert g.frame_status() == 0
    assert np.array_equal(bits(fb.cpu().numpy()), bits(before[0])) and np.array_equal(mask.cpu().numpy(), before[1])
    g.close()


def test_unwritten_bytes_keep_their_sentinel(ra):
    """Pass 1 only, into slices of ONE tensor with guard rows between them, everything filled with a sentinel."""
    g = ra.Scene("scenes/cfg2_smooth_4k.scene", 24, 16)
    sent = np.float32(-123.25)
    guard = 97
    total = sum(w * h * 3 + guard for w, h in SIZES) + guard
    big = torch.full((total,), float(sent), dtype=torch.float32, device="cuda")
    fbs, spans, at = [], [], guard
    for w, h in SIZES:
        fbs.append(big[at:at + w * h * 3].view(h, w, 3)); spans.append((at, at + w * h * 3)); at += w * h * 3 + guard
    base = g.camera_pose()
    cams = [(tuple(float(x) for x in base[0] + np.float32(p)), tuple(float(x) for x in base[1] + np.float32(r))) for p, r in POSES]
    g.render_views(cams, fbs)
    torch.cuda.synchronize()
    got = big.cpu().numpy()
    inside = np.zeros(total, bool)
    for (a, b), (w, h) in zip(spans, SIZES):
        inside[a:b] = True
        v = got[a:b].reshape(h, w, 3)
        assert (v[h - 1] == sent).all() and (v[:, w - 1] == sent).all(), "the last row / column of a %d x %d view was written" % (w, h)
        if w > 1 and h > 1:
            assert (v[:h - 1, :w - 1] != sent).all(), "a pixel of a %d x %d view was not rendered" % (w, h)
    assert (got[~inside] == sent).all(), "%d floats outside the views' buffers were written" % int((got[~inside] != sent).sum())
    g.close()


def test_refusals_on_a_live_scene(ra):
    rtx, _ = ra.load()
    g = ra.Scene("scenes/cfg2_smooth_4k.scene", 24, 16)
    cams, sizes = [POSES[1], POSES[2]], [(24, 16), (9, 9)]

    def refused(code, what, ssaa=True, **kw):
        fbs = [torch.full((h, w, 3), 5.0, dtype=torch.float32, device="cuda") for w, h in sizes]
        masks = [torch.full((h, w), 7, dtype=torch.uint8, device="cuda") for w, h in sizes]
        with pytest.raises(ra.RtxError, match=what) as e:
            g.render_views(cams, fbs, masks, ssaa=ssaa)
        assert "(%d)" % code in str(e.value)
        torch.cuda.synchronize()
        assert all((f == 5.0).all().item() for f in fbs) and all((m == 7).all().item() for m in masks), "a refused call touched a buffer"

    g.counters_enable(True)
    refused(-4, "statistics")
    g.counters_enable(False)
    g.set_flag("showNormals", 1)
    refused(-4, "normals view")
    g.set_flag("showNormals", 0)
    g.set_row_ownership(8, 2, 1)
    refused(-1, "deal out views")
    g.set_row_ownership(0, 1, 0)
    # the C entry's own argument checks, on the live scene
    t = (ra.ViewTarget * 2)()
    for i, (cam, (w, h)) in enumerate(zip(cams, sizes)):
        t[i] = g.view_target(cam[0], cam[1], None, w, h)
    fb = torch.full((16, 24, 3), 5.0, dtype=torch.float32, device="cuda"); mask = torch.full((16, 24), 7, dtype=torch.uint8, device="cuda")
    fb2 = torch.full((9, 9, 3), 5.0, dtype=torch.float32, device="cuda")
    t[0].fb_dev = fb.data_ptr(); t[0].mask_dev = mask.data_ptr(); t[1].fb_dev = fb2.data_ptr()
    sp = g.gpu()
    assert rtx.rtx_render_views(sp, 2, t, 1, None) == -1 and b"mask_dev is NULL" in rtx.rtx_last_error()
    t[1].fb_dev = None
    assert rtx.rtx_render_views(sp, 2, t, 0, None) == -1 and b"fb_dev is NULL" in rtx.rtx_last_error()
    t[1].fb_dev = fb2.data_ptr(); t[1].width = 0
    assert rtx.rtx_render_views(sp, 2, t, 0, None) == -1 and b"zero width" in rtx.rtx_last_error()
    t[1].width = 40000
    assert rtx.rtx_render_views(sp, 2, t, 0, None) == -1 and b"MAX_SIDE" in rtx.rtx_last_error()
    assert rtx.rtx_render_views(sp, 2, None, 0, None) == -1 and b"views is NULL" in rtx.rtx_last_error()
    assert rtx.rtx_render_views(sp, 0, None, 1, None) == 0
    torch.cuda.synchronize()
    assert (fb == 5.0).all().item() and (fb2 == 5.0).all().item() and (mask == 7).all().item()
    # ... and the scene still renders a batch
    t[1].width = 9
    assert rtx.rtx_render_views(sp, 2, t, 0, None) == 0
    torch.cuda.synchronize()
    assert (fb[:15, :23] != 5.0).all().item()
    g.close()
