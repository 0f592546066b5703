"""The inputs and numpy references of tests/util_image_stage.py against the CPU oracle, against the real reference where oracle/_ref
exists, and against the reference's recorded verdicts (tests/golden/image_stage.npz, tools/make_golden_image_stage.py) everywhere.
tests/test_gpu_image_stage.py then holds rtx_sobel, rtx_render_ssaa and rtx_quantize_bgr8 to the oracle on the same inputs."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import util_image_stage as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref", "libref_harness.so")
GOLD = os.path.join(ROOT, "tests", "golden", "image_stage.npz")
SCENE = "scenes/cfg1_simple_shapes.scene"
needs_ref = pytest.mark.skipif(not os.path.exists(REF), reason="oracle/_ref not built (no /root/reference here)")


@pytest.fixture(scope="module")
def images():
    return U.sobel_images()


@pytest.fixture(scope="module")
def oracle_masks(oracle, images):
    return {name: oracle.OracleScene(SCENE, img.shape[1], img.shape[0]).sobel(img) for name, img in images}


def test_sobel_images_have_the_sizes_and_features_asked_for(images):
    d = dict(images)
    assert len(d) == len(images) == 2 + 4 * len(U.STRUCTURE_SIZES)
    assert d["probe"].shape == (256, 256, 3) and d["special"].shape == (64, 64, 3)
    for W, H in U.STRUCTURE_SIZES:
        for kind in ("vsteps", "hsteps", "checker", "ramp"):
            assert d["%s_%dx%d" % (kind, W, H)].shape == (H, W, 3)
    v = d["vsteps_187x35"][0, :, 0]
    assert set(np.nonzero(v[1:] != v[:-1])[0] + 1) == {1, 61, 62, 63, 123, 124, 125, 185}
    h = d["hsteps_187x35"][:, 0, 0]
    assert set(np.nonzero(h[1:] != h[:-1])[0] + 1) == {1, 7, 8, 9, 15, 16, 31, 32, 33}       # (H-2 = 33)
    h = d["hsteps_65x41"][:, 0, 0]
    assert set(np.nonzero(h[1:] != h[:-1])[0] + 1) == {1, 7, 8, 9, 15, 16, 31, 32, 33, 39}
    val = U.sobel_f64(d["ramp_187x35"])[1:-1, 1:-1]
    assert (val > 0.6).any() and (val < 0.4).any()
    sp = d["special"]
    for v in U.SPECIAL_VALUES:
        want = U.bits(np.float32(v))
        assert v == "nan" or (U.bits(sp) == want).sum() >= 3, v
    assert np.isnan(sp).sum() == 3 and np.isinf(sp).sum() == 6 + 2 * 20


def test_sobel_restatement_equals_the_oracle(images, oracle_masks):
    """sobel_f32 -- one fp32 rounding per operation, in the order of scene.cpp:554-567, zero-weight terms included -- gives the oracle's
    mask byte for byte on every image, the borders (0) included."""
    for name, img in images:
        mine, ref = U.sobel_f32(img), oracle_masks[name]
        assert mine.shape == ref.shape and np.array_equal(mine, ref), "%s: %d bytes differ" % (name, int((mine != ref).sum()))
        assert not ref[0].any() and not ref[-1].any() and not ref[:, 0].any() and not ref[:, -1].any(), name
        assert set(np.unique(ref)) <= {0, 1}


def test_sobel_special_values(oracle_masks):
    """What the special image is for: an infinity at the centre or at an edge neighbour meets a zero weight and clears the flag (NaN);
    at a corner it reaches both gradients and sets it; two infinities that meet in one gradient clear it again."""
    m = oracle_masks["special"][U.probe_centres(16)].ravel()
    vals = list(U.SPECIAL_VALUES)
    for v in ("+inf", "-inf"):
        i = 3 * vals.index(v)
        assert list(m[i:i + 3]) == [0, 0, 1], v
    assert list(m[3 * vals.index("nan"):3 * vals.index("nan") + 3]) == [0, 0, 0]
    for i in (vals.index("1e38"), vals.index("-1e38")):
        assert m[3 * i + 1] == 1 and m[3 * i + 2] == 1          # 2 * 1e38 and the squared length overflow to inf: flagged
    pairs = m[24:44].reshape(5, 4)                               # (inf, inf), (inf, -inf), (-inf, -inf), (inf, -inf in another channel)
    # corners of one side share the sign of their weight in one gradient and differ in the other: some gradient cancels whatever the
    # signs; diagonal corners have both weights opposite: only equal signs cancel
    assert pairs.tolist() == [[0, 0, 0, 1]] * 3 + [[0, 1, 0, 1]] * 2


def test_sobel_float64_check(images, oracle_masks):
    """Wherever val, evaluated in float64, is further than 1e-4 * 0.5 from the threshold, the oracle's flag is val64 > 0.5.  The band
    is about 100 times the fp32 bound of the expression (some 25 roundings of 2^-24 each, relative to values of at most 8).  The
    special image is left out: overflow to inf in fp32 is no rounding error."""
    outside = 0
    for name, img in images:
        if name == "special":
            continue
        val = U.sobel_f64(img)
        far = np.abs(val - 0.5) > 1e-4 * 0.5
        far[0] = far[-1] = False
        far[:, 0] = far[:, -1] = False
        assert np.array_equal(oracle_masks[name][far] != 0, val[far] > 0.5), name
        outside += int(far.sum())
    assert outside > 20000


def test_sobel_inputs_discriminate(images, oracle_masks):
    """Conditions on the INPUTS, met by the restatement alone (seed 1): of the 4096 probes 1713 are flagged and 2383 are not (each at
    least 25 %), 410 have val == 0.5f exactly (the strict >), and the mutants of the restatement disagree with it on 30 (fma in the
    final sum), 166 (s > 0.25f without the square root), 57 (no sqrt-then-square round trip) and 322 (float64 throughout) probes."""
    img = dict(images)["probe"]
    c = U.probe_centres()
    ref = U.sobel_f32(img)[c]
    assert ref.size == 4096
    assert min(int(ref.sum()), int((ref == 0).sum())) >= 1024
    with np.errstate(all="ignore"):
        x, y = U._gradients(img, np.float32)
        lx, ly = np.sqrt(U._len2(x)), np.sqrt(U._len2(y))
        val = np.sqrt(lx * lx + ly * ly)[::4, ::4]              # (the centres are the interior's (0, 0), (0, 4), ...)
    assert val.shape == ref.shape and np.array_equal(val > np.float32(0.5), ref != 0)
    exact = int((val == np.float32(0.5)).sum())
    counts = {k: int((f(img)[c] != ref).sum()) for k, f in U.MUTANTS.items()}
    print("flagged %d of %d, exactly 0.5f: %d, mutants: %r" % (int(ref.sum()), ref.size, exact, counts))
    assert exact >= 100
    assert sorted(counts) == ["float64", "fma", "no_round_trip", "no_sqrt"]
    for k, n in counts.items():
        assert n >= 8, "mutant %s differs on %d probes only" % (k, n)
    # every probe's val is within the few ulp asked for (so the float64 check above says nothing about them)
    assert (np.abs(U.sobel_f64(img)[c] - 0.5) < 16 * 2.0 ** -24).all()


def test_canaries():
    fb = U.canary_fb(136, 104)
    assert np.unique(U.bits(fb)).size == fb.size and U.is_canary(fb).all()
    assert np.isnan(fb).sum() == fb.size // 2 and (fb[~np.isnan(fb)] < 0).all()


def test_ssaa_masks():
    for W, H in ((136, 104), (61, 43), (9, 9), (8, 8), (2, 2)):
        m = U.ssaa_masks(W, H, 5)
        assert len(m) == 20 and all(a.shape == (H, W) and a.dtype == np.uint8 for a in m.values())
        assert not m["empty"].any() and (m["all_1"] == 1).all() and (m["all_255"] == 255).all()
        assert m["px_w1_h1"][H - 1, W - 1] == 1 and m["px_w1_h1"].sum() == 1 and m["px_0_0"][0, 0] == 1
        assert m["row_0"][0].all() and not m["row_0"][1:].any() and m["last_column"][:, -1].all() and not m["last_column"][:, :-1].any()
        full = (slice(0, H // 8 * 8), slice(0, W // 8 * 8))
        if H >= 8 and W >= 8:
            for n in (15, 16, 17):
                t = m["tile_%d" % n][full]
                assert (t.reshape(H // 8, 8, W // 8, 8).sum((1, 3)) == n).all()
            assert (m["tile_bit_63"][full].reshape(H // 8, 8, W // 8, 8)[:, 7, :, 7] == 1).all() and m["tile_bit_63"][full].sum() == (H // 8) * (W // 8)
        assert set(U.DENSE_MASKS) <= set(m)
    big = U.ssaa_masks(136, 104, 5)
    for name, p in (("bernoulli_1_64", 1 / 64), ("bernoulli_1_4", 1 / 4), ("bernoulli_63_64", 63 / 64)):
        assert abs((big[name] != 0).mean() - p) < 0.02 and set(np.unique(big[name])) == {0, 1, 2, 128, 255}


def test_ssaa_expected_keeps_unflagged_bits(oracle):
    """ssaa_expected on a canary framebuffer: exactly the flagged pixels x < W-1, y < H-1 inside the rows hold rendered values, every
    other float still has its canary bits -- and the oracle takes any nonzero byte as a flag."""
    W, H = 61, 43
    o = oracle.OracleScene("scenes/cfg2_smooth_4k.scene", W, H)
    fb = U.canary_fb(W, H)
    masks = U.ssaa_masks(W, H, 5)
    for name, rows in (("bernoulli_1_4", (0, H)), ("all_255", (3, 21)), ("last_row", (0, H)), ("column_0", (8, 9))):
        exp = U.ssaa_expected(o, fb, masks[name], rows)
        changed = (U.bits(exp) != U.bits(fb)).any(-1)
        assert np.array_equal(changed, U.ssaa_flagged(masks[name], rows)), name
        assert not U.is_canary(exp[changed]).any() and np.array_equal(U.bits(exp)[~changed], U.bits(fb)[~changed])
    one = U.ssaa_expected(o, fb, (masks["bernoulli_1_4"] != 0).astype(np.uint8))
    assert np.array_equal(U.bits(one), U.bits(U.ssaa_expected(o, fb, masks["bernoulli_1_4"])))


def test_quant_table_covers_every_boundary_in_every_slot():
    t = U.quant_table()
    v = U.quant_values()
    assert t.shape[1:] == (U.QUANT_WIDTH, 3) and t.shape[0] % 12 == 0
    flat = U.bits(t).ravel()
    slot = np.arange(flat.size) % 12                    # which of its thread's 12 floats: pixel = slot // 3, channel = slot % 3
    for s in range(12):
        assert set(U.bits(v).tolist()) <= set(flat[slot == s].tolist()), s
    k = np.arange(256)
    exact = (k / 255.0).astype(np.float32)
    assert set(U.bits(exact).tolist()) <= set(U.bits(v).tolist())
    # the boundaries bite: around every k / 255 the byte changes within the 7 values, and truncation differs from rounding somewhere
    b = U.quant_f32(v.reshape(1, -1, 1).repeat(3, 2))[::3]
    near = b[:7 * 256].reshape(256, 7)
    assert (near.max(1) - near.min(1) >= 1)[1:].all()
    assert (np.isnan(v)).sum() == 4 and b[np.isnan(v)].tolist() == [255] * 4
    assert b[U.bits(v) == 0x80000000].tolist() == [0] and b[np.isposinf(v)].tolist() == [255] and b[np.isneginf(v)].tolist() == [0]


def test_quant_restatement_equals_the_oracle(oracle):
    """quant_f32 -- clamp with the comparison order of std::min / std::max, one fp32 product, truncation, BGR, bottom-up -- gives the
    oracle's BMP body on the table and on random frames of every size the GPU test uses."""
    t = U.quant_table()
    assert U.quant_f32(t).tobytes() == oracle.encode_bmp(t)[54:]
    for W, H in U.QUANT_SIZES:
        fb = U.quant_frame(W, H, seed=W * 100 + H)
        assert U.quant_f32(fb).tobytes() == oracle.encode_bmp(fb)[54:], (W, H)


def test_oracle_matches_reference_golden_image_stage(oracle, images, oracle_masks):
    """The oracle against the real reference's recorded verdicts: its Sobel flags over 1 <= x < W-1, 1 <= y < H-1 on every image, and
    the file its saveImage wrote for the quantiser table.  Runs everywhere, so a machine without the reference is still held to it."""
    g = np.load(GOLD)
    assert sorted(g.files) == sorted(["mask__" + name for name, _ in images] + ["quant_bmp"])
    for name, img in images:
        assert np.array_equal(np.packbits(oracle_masks[name][1:-1, 1:-1] != 0), g["mask__" + name]), name
    assert oracle.encode_bmp(U.quant_table()) == g["quant_bmp"].tobytes()


SOBEL_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, %r)
from oracle import oracle as O
from tests import util_image_stage as U
from tools import make_golden_image_stage as G
W, H = int(sys.argv[1]), int(sys.argv[2])
ref = G.reference_masks(W, H)          # (asserts that the canaries are negative or NaN and that the scene renders neither)
assert ref
o = O.OracleScene(G.SCENE, W, H)
for name, img in U.sobel_images():
    if name in ref:
        m = o.sobel(img)
        assert np.array_equal(m, o.sobel(-img)), name
        assert np.array_equal(m[1:-1, 1:-1] != 0, ref[name]), (name, int(((m[1:-1, 1:-1] != 0) != ref[name]).sum()))
print('OK', len(ref))
"""

QUANT_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, %r)
from oracle import oracle as O
from tests import util_image_stage as U
from tools import make_golden_image_stage as G
assert G.reference_quant_bmp().tobytes() == O.encode_bmp(U.quant_table())
print('OK')
"""


@needs_ref
@pytest.mark.parametrize("W,H", [(256, 256), (64, 64)] + U.STRUCTURE_SIZES)
def test_reference_launch_ssaa_flags_what_the_oracle_flags(W, H):
    """The real reference's launchSSAA on the probe, special and structure images (negated: every float negative or NaN, the mask is
    the same -- tools/make_golden_image_stage.py): over 1 <= x < W-1, 1 <= y < H-1 the pixels whose bits changed are the oracle's
    mask.  Row 0 and column 0 are left out: the reference's border flags are uninitialised memory.  One process per frame size."""
    out = subprocess.run([sys.executable, "-c", SOBEL_CHILD % ROOT, str(W), str(H)], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


@needs_ref
def test_reference_save_image_writes_the_oracles_bytes():
    out = subprocess.run([sys.executable, "-c", QUANT_CHILD % ROOT], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
