"""Synthetic inputs and plain numpy references for the three calls that take a buffer of the caller's: rtx_sobel (any framebuffer),
rtx_render_ssaa (any mask) and rtx_quantize_bgr8 (any framebuffer).  No torch; everything is generated from seeds.

Sobel (scene.cpp:554-567): probes whose `val` lies within 4 ulp of the 0.5 threshold, small images with edges on the columns and rows
where the wave layout of rtxSobelKernel changes, and a probe image with inf / NaN / huge / denormal entries.  sobel_f32 restates the
reference's arithmetic with one fp32 rounding per operation; MUTANTS are four near misses of it that only show the probes discriminate.
SSAA: named masks for the flagged-pixel list (full tiles, the pad-to-16 edges, borders, bytes other than 1).
Quantiser (util.cpp:46-58): every fp32 within 3 ulp of k/255 and the special values, under every position of a thread's 12 floats.
"""
import numpy as np

CANARY = 0xA5                     # every mask / image byte outside what a call may write
SOBEL_OP = ((-1.0, 0.0, 1.0), (-2.0, 0.0, 2.0), (-1.0, 0.0, 1.0))
PROBE_SEED, PROBE_SIDE = 1, 64    # 256 x 256, 4096 probes
SPECIAL_SEED = 2
STRUCTURE_SIZES = [(3, 3), (4, 3), (62, 9), (63, 8), (64, 33), (65, 41), (126, 16), (187, 35)]       # (W, H)
STEP_COLUMNS = (1, 61, 62, 63, 123, 124, 125)       # and W-2
STEP_ROWS = (1, 7, 8, 9, 15, 16, 31, 32, 33)        # and H-2
QUANT_SIZES = [(4, 1), (8, 3), (60, 12), (64, 9), (68, 2)]      # (W, H)
QUANT_WIDTH = 60


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------
# Sobel: the reference's arithmetic in numpy
# ------------------------------------------------------------------------------------------------
def _gradients(fb, dtype):
    """(x, y) of scene.cpp:556-563 for every interior pixel, (H-2, W-2, 3) each: 9 products and 9 additions per gradient in the
    reference's order, the terms with a zero weight included (inf * 0 = NaN reaches the sum), each rounded to `dtype`."""
    fb = np.asarray(fb, np.float32).astype(dtype)
    H, W, _ = fb.shape
    x = np.zeros((H - 2, W - 2, 3), dtype)
    y = np.zeros((H - 2, W - 2, 3), dtype)
    for a in range(3):
        for b in range(3):
            p = fb[a:a + H - 2, b:b + W - 2]
            x = x + p * dtype(SOBEL_OP[a][b])
            y = y + p * dtype(SOBEL_OP[b][a])
    return x, y


def _len2(v):
    return v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2]      # left to right (geometry.h:84-87)


def _mask(flag, shape):
    m = np.zeros(shape[:2], np.uint8)
    m[1:-1, 1:-1] = flag
    return m


def sobel_f32(fb):
    """The mask of Scene::launchSSAA (scene.cpp:554-567), borders 0: every operation rounded once to fp32.  Vec3f::length is
    (float)sqrt((double)len2), which is the correctly rounded fp32 square root; powf(l, 2) is l * l."""
    with np.errstate(all="ignore"):
        x, y = _gradients(fb, np.float32)
        lx, ly = np.sqrt(_len2(x)), np.sqrt(_len2(y))
        val = np.sqrt(lx * lx + ly * ly)
        return _mask(val > np.float32(0.5), np.shape(fb))


def sobel_f64(fb):
    """`val` of the same expression evaluated in float64 from the fp32 pixels, (H, W) with borders 0."""
    with np.errstate(all="ignore"):
        x, y = _gradients(fb, np.float64)
        lx, ly = np.sqrt(_len2(x)), np.sqrt(_len2(y))
        val = np.zeros(np.shape(fb)[:2], np.float64)
        val[1:-1, 1:-1] = np.sqrt(lx * lx + ly * ly)
        return val


def _mutant_fma(fb):
    """fma(lx, lx, ly * ly) in the final sum: lx * lx enters unrounded (it is exact in float64)."""
    with np.errstate(all="ignore"):
        x, y = _gradients(fb, np.float32)
        lx, ly = np.sqrt(_len2(x)), np.sqrt(_len2(y))
        s = (lx.astype(np.float64) * lx.astype(np.float64) + (ly * ly).astype(np.float64)).astype(np.float32)
        return _mask(np.sqrt(s) > np.float32(0.5), np.shape(fb))


def _mutant_no_sqrt(fb):
    """s > 0.25f in place of sqrtf(s) > 0.5f."""
    with np.errstate(all="ignore"):
        x, y = _gradients(fb, np.float32)
        lx, ly = np.sqrt(_len2(x)), np.sqrt(_len2(y))
        return _mask(lx * lx + ly * ly > np.float32(0.25), np.shape(fb))


def _mutant_no_round_trip(fb):
    """sqrt(len2(x) + len2(y)): the lengths are not taken and squared again."""
    with np.errstate(all="ignore"):
        x, y = _gradients(fb, np.float32)
        return _mask(np.sqrt(_len2(x) + _len2(y)) > np.float32(0.5), np.shape(fb))


def _mutant_f64(fb):
    return (sobel_f64(fb) > 0.5).astype(np.uint8)


MUTANTS = {"fma": _mutant_fma, "no_sqrt": _mutant_no_sqrt, "no_round_trip": _mutant_no_round_trip, "float64": _mutant_f64}


# ------------------------------------------------------------------------------------------------
# Sobel: inputs
# ------------------------------------------------------------------------------------------------
def sobel_probe_image(seed=PROBE_SEED, n_side=PROBE_SIDE):
    """n_side x n_side cells of 4 x 4 pixels, (4 n_side, 4 n_side, 3) fp32.  Each cell holds an independent random 3 x 3 x 3 patch in
    [0, 1) in its upper left 3 x 3 pixels (the rest is 0), scaled in float64 so that the cell's centre pixel (4 i + 1, 4 j + 1) has
    val = 0.5, then multiplied by 1 + k 2^-23 with k drawn from -4 .. 4 and rounded to fp32: val lands within a few ulp of the
    threshold, on either side and on it."""
    rng = np.random.default_rng(seed)
    patch = rng.random((n_side, n_side, 3, 3, 3))                      # cell row, cell column, a, b, channel
    k = rng.integers(-4, 5, (n_side, n_side))
    op = np.array(SOBEL_OP)
    gx = np.einsum("ijabc,ab->ijc", patch, op)
    gy = np.einsum("ijabc,ba->ijc", patch, op)
    val = np.sqrt((gx * gx).sum(-1) + (gy * gy).sum(-1))
    patch = patch * (0.5 / val)[:, :, None, None, None] * (1.0 + k * 2.0 ** -23)[:, :, None, None, None]
    cells = np.zeros((n_side, n_side, 4, 4, 3))
    cells[:, :, :3, :3] = patch
    return np.ascontiguousarray(cells.transpose(0, 2, 1, 3, 4).reshape(4 * n_side, 4 * n_side, 3).astype(np.float32))


def probe_centres(n_side=PROBE_SIDE):
    """(rows, columns) index of the centre pixels of sobel_probe_image, for img[probe_centres()]."""
    c = 4 * np.arange(n_side) + 1
    return np.ix_(c, c)


def _steps(n, at):
    """0 / 1 along an axis of n entries, toggling at every index of `at` that lies inside: a step of height 1 at each."""
    v = np.zeros(n)
    for s in sorted(set(a for a in at if 0 < a < n)):
        v[s:] = 1 - v[s:]
    return v


def sobel_structure_images():
    """[(name, (H, W, 3) fp32)]: for every size of STRUCTURE_SIZES, vertical steps of height 1.0 at the columns where one wave of
    rtxSobelKernel ends and the next begins (61 / 62 / 63, 123 / 124 / 125) and next to the borders, horizontal steps at the rows
    where its 8-row groups and 32-row blocks end, a checkerboard of 2 x 2 squares, and a ramp whose val crosses 0.5 inside the image
    (val = sqrt((x / W)^2 + (y / H)^2) up to rounding)."""
    out = []
    amp = np.array([1.0, 0.5, 0.25])
    for W, H in STRUCTURE_SIZES:
        xs, ys = np.arange(W), np.arange(H)
        v = np.broadcast_to(_steps(W, STEP_COLUMNS + (W - 2,))[None, :, None], (H, W, 3))
        h = np.broadcast_to(_steps(H, STEP_ROWS + (H - 2,))[:, None, None], (H, W, 3))
        checker = (((xs[None, :] // 2 + ys[:, None] // 2) % 2)[:, :, None] * amp)
        ramp = np.zeros((H, W, 3))
        ramp[:, :, 0] = (xs[None, :] ** 2) / (16.0 * W)
        ramp[:, :, 1] = (ys[:, None] ** 2) / (16.0 * H)
        for name, img in (("vsteps", v), ("hsteps", h), ("checker", checker), ("ramp", ramp)):
            out.append(("%s_%dx%d" % (name, W, H), np.ascontiguousarray(img, np.float32)))
    return out


SPECIAL_VALUES = ("+inf", "-inf", "nan", "-0.0", "1e38", "-1e38", "1e-45", "3e-39")
_CENTRE, _EDGES, _CORNERS = (1, 1), ((0, 1), (1, 0), (1, 2), (2, 1)), ((0, 0), (0, 2), (2, 0), (2, 2))


def sobel_special_image():
    """The probe layout at 64 x 64 (16 x 16 cells).  In the first 24 cells the centre pixel, an edge neighbour or a corner neighbour of
    the cell's centre holds one of SPECIAL_VALUES in one channel.  An inf at the centre or at an edge neighbour meets a zero weight
    (NaN: no flag); at a corner both gradients are infinite (flag).  The next cells put two infinities at two corners of one channel:
    corners of one side cancel to NaN in x or in y whatever their signs, diagonal corners only with equal signs; in different channels
    they never meet."""
    img = sobel_probe_image(SPECIAL_SEED, 16)
    vals = [np.float32(v) for v in SPECIAL_VALUES]
    cell = 0

    def put(pos, ch, v):
        cy, cx = divmod(cell, 16)
        img[4 * cy + pos[0], 4 * cx + pos[1], ch] = v

    for i, v in enumerate(vals):
        for kind in range(3):
            pos = (_CENTRE, _EDGES[(i + kind) % 4], _CORNERS[(i + kind) % 4])[kind]
            put(pos, cell % 3, v)
            cell += 1
    inf = np.float32(np.inf)
    for (p, q) in (((0, 0), (0, 2)), ((0, 0), (2, 0)), ((0, 2), (2, 2)), ((0, 0), (2, 2)), ((0, 2), (2, 0))):
        for sp, sq, chq in ((inf, inf, 0), (inf, -inf, 0), (-inf, -inf, 0), (inf, -inf, 1)):
            put(p, 0, sp)
            put(q, chq, sq)
            cell += 1
    assert cell <= 256
    return img


def sobel_images():
    """Every Sobel input of this module: [(name, image)]."""
    return [("probe", sobel_probe_image()), ("special", sobel_special_image())] + sobel_structure_images()


# ------------------------------------------------------------------------------------------------
# Canaries
# ------------------------------------------------------------------------------------------------
def canary_fb(W, H):
    """(H, W, 3) fp32 in which every float is a different bit pattern that no render produces: negative finite values at the even
    indices, quiet NaNs with a payload (of both signs) at the odd ones."""
    i = np.arange(H * W * 3, dtype=np.uint32)
    assert i.size < 1 << 21
    neg = np.uint32(0xBF000000) + i
    nan = np.uint32(0x7FC00000) | ((i & np.uint32(2)) << np.uint32(30)) | (i + np.uint32(1))
    return np.where(i % 2 == 0, neg, nan).astype(np.uint32).view(np.float32).reshape(H, W, 3)


def is_canary(a):
    """True where a float is negative (sign bit set) or NaN -- what canary_fb holds and a render never writes."""
    a = np.asarray(a, np.float32)
    return np.signbit(a) | np.isnan(a)


# ------------------------------------------------------------------------------------------------
# SSAA masks
# ------------------------------------------------------------------------------------------------
DENSE_MASKS = ("all_1", "all_255", "checker", "bernoulli_63_64", "tile_17")


def ssaa_masks(W, H, seed=0):
    """{name: (H, W) uint8}.  The list kernels take the flagged pixels x < W-1, y < H-1 of 8 x 8 tiles: masks that fill a tile's 64-bit
    bitmap, sit on the pad-to-16 edges (15, 16, 17 pixels in every tile that lies inside the frame), flag the first row and column
    (re-rendered) and the last ones (never visited), and hold bytes other than 1."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H, 0:W]
    m = {}

    def new(name):
        m[name] = np.zeros((H, W), np.uint8)
        return m[name]

    new("empty")
    new("all_1")[:] = 1
    new("all_255")[:] = 255
    for name, (x, y) in (("px_0_0", (0, 0)), ("px_w2_h2", (W - 2, H - 2)), ("px_w1_0", (W - 1, 0)), ("px_0_h1", (0, H - 1)),
                         ("px_w1_h1", (W - 1, H - 1))):
        if 0 <= x and 0 <= y:
            new(name)[y, x] = 1
    new("row_0")[0, :] = 1
    new("column_0")[:, 0] = 1
    new("last_row")[H - 1, :] = 1
    new("last_column")[:, W - 1] = 1
    new("checker")[:] = (xs + ys) % 2
    new("tile_bit_63")[:] = (xs % 8 == 7) & (ys % 8 == 7)
    order = rng.permutation(64)                         # in-tile positions; the first n of them are flagged in every tile
    rank = np.empty(64, np.int64)
    rank[order] = np.arange(64)
    for n in (15, 16, 17):
        new("tile_%d" % n)[:] = rank[(ys % 8) * 8 + xs % 8] < n
    values = np.array([1, 2, 128, 255], np.uint8)
    for name, p in (("bernoulli_1_64", 1 / 64), ("bernoulli_1_4", 1 / 4), ("bernoulli_63_64", 63 / 64)):
        new(name)[:] = np.where(rng.random((H, W)) < p, values[rng.integers(0, 4, (H, W))], 0)
    return m


def ssaa_flagged(mask, rows):
    """The pixels rtx_render_ssaa re-renders: mask != 0, x < W-1, y < H-1, y inside rows (scene.cpp:369-372, 523-525)."""
    H, W = mask.shape
    f = np.asarray(mask) != 0
    f[H - 1:, :] = False
    f[:, W - 1:] = False
    f[:rows[0]] = False
    f[rows[1]:] = False
    return f


def ssaa_expected(oracle_scene, fb, mask, rows=None, full=None):
    """oracle.ssaa(fb, mask) inside rows, fb's own bits elsewhere.  full: oracle_scene.ssaa(fb, mask) where the caller has it already."""
    H = fb.shape[0]
    r0, r1 = rows if rows is not None else (0, H)
    if full is None:
        full = oracle_scene.ssaa(fb, mask)
    out = np.array(fb, np.float32, copy=True)
    out.view(np.uint32)[r0:r1] = full.view(np.uint32)[r0:r1]
    return out


# ------------------------------------------------------------------------------------------------
# Quantiser
# ------------------------------------------------------------------------------------------------
def quant_values():
    """Every fp32 within 3 ulp of float32(k / 255), k = 0 .. 255 -- the 256 places where v * 255 crosses an integer, so that a rounding
    convert, a product kept unrounded or a saturating convert would give another byte -- and the special values."""
    v = []
    for k in range(256):
        c = np.float32(k / 255.0)
        lo = hi = c
        v.append(c)
        for _ in range(3):
            lo = np.nextafter(lo, np.float32(-np.inf), dtype=np.float32)
            hi = np.nextafter(hi, np.float32(np.inf), dtype=np.float32)
            v += [lo, hi]
    one = np.float32(1)
    v += [np.float32(x) for x in (0.0, -0.0, 1e-45, -1e-45, np.nextafter(one, np.float32(0)), 1.0, np.nextafter(one, np.float32(2)),
                                  2.0, -1.0, 1e38, -1e38, np.inf, -np.inf)]
    out = np.array(v, np.float32)
    nans = np.array([0x7FC00000, 0xFFC00000, 0x7FC12345, 0xFFC54321], np.uint32).view(np.float32)
    return np.concatenate([out, nans])


def quant_table():
    """(H, 60, 3) fp32: quant_values, padded with 0.5 to whole rows, repeated under the 12 cyclic shifts of the flat array: a thread of
    rtxQuantizeKernel converts 12 consecutive floats (4 pixels), so every value meets every channel and each of the four pixels."""
    v = quant_values()
    per_row = QUANT_WIDTH * 3
    n = -(-v.size // per_row) * per_row
    flat = np.full(n, 0.5, np.float32)
    flat.view(np.uint32)[:v.size] = v.view(np.uint32)
    u = flat.view(np.uint32)
    table = np.concatenate([np.roll(u, s) for s in range(12)])
    return table.view(np.float32).reshape(-1, QUANT_WIDTH, 3)


def quant_frame(W, H, seed):
    """A random frame for the quantiser: values over [-0.25, 1.25), with exact k / 255 and special values sprinkled in."""
    rng = np.random.default_rng(seed)
    fb = (rng.random((H, W, 3)) * 1.5 - 0.25).astype(np.float32)
    v = quant_values()
    pick = rng.random((H, W, 3)) < 0.5
    fb.view(np.uint32)[pick] = v.view(np.uint32)[rng.integers(0, v.size, int(pick.sum()))]
    return fb


def quant_f32(fb):
    """saveImage's bytes (util.cpp:46-58), (H * W * 3,) uint8: std::max(0, std::min(1, v)) with the comparisons of <algorithm> --
    min(1, v) = v < 1 ? v : 1 and max(0, m) = 0 < m ? m : 0, so NaN gives 1 and -0 gives +0 --, times 255 rounded to fp32, truncated;
    B, G, R; image rows bottom-up."""
    v = np.asarray(fb, np.float32)
    with np.errstate(invalid="ignore"):
        m = np.where(v < np.float32(1), v, np.float32(1))
        c = np.where(np.float32(0) < m, m, np.float32(0))
        p = c * np.float32(255)
    return np.ascontiguousarray(np.trunc(p).astype(np.uint8)[::-1, :, ::-1]).ravel()
