"""GPU: the two debug views of the reference on the HIP path -- showNormals (RTX_FLAG_SHOW_NORMALS) and the showAC heat map
(rtx_render_ac) -- against the committed goldens of the real reference (tests/golden/debug_*.npz) and our numpy restatement
of countAC (tests/ac_heatmap.py).  Reads only the repository."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

from tests import ac_heatmap as A
from tests.util_rays import probe_rays
from tests.util_ulp import NORMAL_MAP_ULP, bits, ulp_diff
from tools.make_golden_debug_views import HEATMAP, NORMALS, key, load

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "rendering_amd", "render_amd")


@pytest.fixture(scope="module")
def gold():
    from rendering_amd import assets
    g = load()
    assets.ensure(); assets.ensure(["bumpy_250k.obj"])
    for item in str(g["assets_md5"]).split(";"):
        n, md5 = item.split("=")
        assert assets.md5(n) == md5, "generated asset %s differs from the one the goldens were made with" % n
    return g


# NORMAL_MAP_ULP: where a normal map shows, the view is pinned to within the reference's own walk (tests/util_ulp.py); every other scene bit for bit.


def border_masked_diff(got, want, ulp=0):
    d = ulp_diff(got, want) > ulp
    d[0, :] = False; d[:, 0] = False                  # uninitialised Sobel border in the reference
    return int(d.sum())


def same(got, want, ulp=0):
    return bool((ulp_diff(got, want) <= ulp).all())


@pytest.mark.parametrize("name,w,h,extra", NORMALS, ids=[key("normals", n, e) for n, w, h, e in NORMALS])
def test_normals_view_matches_reference(ra, gold, tmp_path, name, w, h, extra):
    import torch
    k = key("normals", name, extra)
    ulp = NORMAL_MAP_ULP if name.startswith("cfg4") else 0
    s = ra.Scene(A.scene_copy(name, str(tmp_path), dict(extra, showNormals=1)), w, h)
    assert s.view_flags() & 4
    fb1 = s.render_host(ssaa=False)
    assert same(fb1, gold[k + "__pass1"], ulp)
    if ulp:
        assert (ulp_diff(fb1, gold[k + "__pass1"]) > 0).mean() < 0.1      # (fraction of pixels)
    assert border_masked_diff(s.render_host(ssaa=True), gold[k + "__ssaa"], ulp) == 0
    fb = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
    mask = torch.zeros((h, w), dtype=torch.uint8, device="cuda:0")
    for _ in range(2):
        fb.zero_()
        s.render_frame(fb, mask)
        assert s.frame_status() == 0
        assert border_masked_diff(fb.cpu().numpy(), gold[k + "__ssaa"], ulp) == 0
    _, col = s.cast_rays(probe_rays(1024))
    assert same(col, gold[k + "__probe_colours"], ulp)


@pytest.mark.parametrize("name,w,h,extra", HEATMAP, ids=[key("ac", n, e) for n, w, h, e in HEATMAP])
def test_heatmap_matches_reference(ra, gold, tmp_path, name, w, h, extra):
    import torch
    k = key("ac", name, extra)
    s = ra.Scene(A.scene_copy(name, str(tmp_path), dict(extra, showAC=1)), w, h)
    fb = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
    counts = torch.full((h, w), -1, dtype=torch.int32, device="cuda:0")
    s.render_ac(fb, counts)
    torch.cuda.synchronize()
    c = counts.cpu().numpy().view(np.uint32)
    want = A.counts(s).reshape(h, w)
    assert np.array_equal(c, want)
    f = fb.cpu().numpy()
    ref = A.frame(want, w, h)
    assert np.array_equal(np.isnan(f), np.isnan(ref))
    ok = ~np.isnan(ref)
    assert np.array_equal(bits(f)[ok], bits(ref)[ok])
    if name == "cfg1_simple_shapes":
        assert np.isnan(f).all()
    out = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda:0")
    s.quantize(fb, out)
    torch.cuda.synchronize()
    bmp = gold[k + "__bmp"].tobytes()[:54] + out.cpu().numpy().tobytes()
    assert hashlib.md5(bmp).hexdigest() == str(gold[k + "__md5"])
    fb2 = torch.zeros_like(fb)
    s.render_ac(fb2)                                  # no counts buffer: the scene's own
    torch.cuda.synchronize()
    assert torch.equal(fb2.view(torch.int32), fb.view(torch.int32))


def test_heatmap_4096_sample_matches_restatement(ra, gold):
    import torch
    W = H = 4096
    s = ra.Scene("scenes/cfg2_smooth_250k.scene", W, H)
    fb = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0")
    counts = torch.zeros((H, W), dtype=torch.int32, device="cuda:0")
    s.render_ac(fb, counts)
    torch.cuda.synchronize()
    c = counts.cpu().numpy().view(np.uint32)
    rng = np.random.default_rng(4096)
    ys, xs = rng.integers(0, H, 10000), rng.integers(0, W, 10000)
    ys[:4] = [0, H - 1, 0, H - 1]; xs[:4] = [0, 0, W - 1, W - 1]          # the last row and column are part of the heat map
    assert np.array_equal(c[ys, xs], A.counts(s, xs, ys))
    mx = int(c.max())
    assert mx > 0
    f = fb[ys, xs, 0].cpu().numpy()
    assert np.array_equal(bits(f), bits(c[ys, xs].astype(np.float32) / np.float32(mx)))


def test_cli_writes_the_reference_images(ra, gold, tmp_path):
    for name, w, h, extra in (HEATMAP[1], HEATMAP[4]):
        img = str(tmp_path / ("ac_" + name))
        path = A.scene_copy(name, str(tmp_path), dict(extra, showAC=1, width=w, height=h, image_name=img))
        r = subprocess.run([CLI, path], cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert hashlib.md5(open(img + ".bmp", "rb").read()).hexdigest() == str(gold[key("ac", name, extra) + "__md5"])
    for name, w, h, extra in (NORMALS[1], NORMALS[7]):
        img = str(tmp_path / ("n_" + name))
        path = A.scene_copy(name, str(tmp_path), dict(extra, showNormals=1, width=w, height=h, image_name=img))
        r = subprocess.run([CLI, path], cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        got = np.frombuffer(open(img + ".bmp", "rb").read()[54:], np.uint8).reshape(h, w, 3)[::-1]
        want = np.frombuffer(A.quantize_bmp(gold[key("normals", name, extra) + "__ssaa"], w, h)[54:], np.uint8).reshape(h, w, 3)[::-1]
        d = (got != want).any(-1)
        d[0, :] = False; d[:, 0] = False
        assert not d.any()


def test_cli_refuses_sharded_heatmap(ra, tmp_path):
    path = A.scene_copy("cfg2_smooth_4k", str(tmp_path), dict(showAC=1, width=64, height=48, image_name=str(tmp_path / "x")))
    r = subprocess.run([CLI, "--gpus", "2", path], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    if ra.device_count() >= 2:
        assert "showAC" in r.stderr
    assert not os.path.exists(str(tmp_path / "x.bmp"))


def test_render_ac_refusals_leave_the_buffers_alone(ra):
    import torch
    w, h = 64, 48
    s = ra.Scene("scenes/cfg2_smooth_4k.scene", w, h)
    fb = torch.full((h, w, 3), 7.0, dtype=torch.float32, device="cuda:0")
    counts = torch.full((h, w), 7, dtype=torch.int32, device="cuda:0")
    s.set_row_ownership(16, 2, 0)
    with pytest.raises(ra.RtxError):
        s.render_ac(fb, counts)
    s.set_row_ownership(0, 1, 0)
    s.counters_enable(True)
    with pytest.raises(ra.RtxError):
        s.render_ac(fb, counts)
    s.counters_enable(False)
    torch.cuda.synchronize()
    assert bool((fb == 7.0).all()) and bool((counts == 7).all())
    s.render_ac(fb, counts)
    torch.cuda.synchronize()
    assert not bool((counts == 7).all())


def test_debug_views_leave_the_ordinary_frame_alone(ra):
    import torch
    w, h = 160, 120
    s = ra.Scene("scenes/cfg2_smooth_4k.scene", w, h)
    fb = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
    mask = torch.zeros((h, w), dtype=torch.uint8, device="cuda:0")

    def ordinary():
        frames = []
        for _ in range(3):
            fb.zero_()
            s.render_frame(fb, mask)
            assert s.frame_status() == 0
            frames.append(fb.cpu().numpy().copy())
        fb.zero_()
        s.render_pass1(fb)
        torch.cuda.synchronize()
        return frames + [fb.cpu().numpy().copy()]

    before = ordinary()
    s.set_flag("showNormals", 1)
    fb.zero_()
    s.render_frame(fb, mask)
    s.frame_status()
    normals = fb.cpu().numpy().copy()
    s.set_flag("showNormals", 0)
    s.render_ac(fb)
    torch.cuda.synchronize()
    after = ordinary()
    for a, b in zip(before, after):
        assert np.array_equal(bits(a), bits(b))
    assert not np.array_equal(bits(normals), bits(before[0]))
