"""CPU: the pure parts of the frame calls (csrc/rtx_frame_plan.h) through their host-only probes -- the one-launch-or-three policy of
rtx_render_frame (rtx_frame_mode_probe) and the pass-1 tile lists (rtx_tile_list_probe: TileGrid, stripsFit, planTileList, expectedTileList).
What is expected is written down here, in Python and numpy, from the rules; nothing of it is read from the library."""
import itertools

import numpy as np
import pytest

from rendering_amd import parallel


def mode_rule(forced, has_list, gave_up, listed, rule_tiles, warm, samples, ms, seen):
    """(mode, reprobe, probing): the first rule that applies decides the mode."""
    probing = forced < 0 and has_list and listed <= rule_tiles and (not warm or samples[0] < 2 or samples[1] < 2 or (seen & 63) >= 62)
    if forced >= 0:
        return forced, False, probing
    if not has_list or gave_up:
        return 0, False, probing
    if listed > rule_tiles:
        return 0, False, probing
    if not warm:
        return 1, False, probing
    if samples[0] < 2 or samples[1] < 2:
        return seen & 1, False, probing
    t0, t1 = np.float32(ms[0]), np.float32(ms[1])
    best = 1 if t1 <= t0 else 0
    lo, hi = min(t0, t1), max(t0, t1)
    if ((seen & 63) == 63 and hi <= np.float32(1.2) * lo) or (seen & 1023) == 1023:
        return best ^ 1, True, probing
    if (seen & 63) == 62:
        return best, True, probing
    return best, False, probing


def test_frame_mode_policy(ra):
    checked, seen_modes = 0, set()
    for rule_tiles in (8192, 65536):
        for forced, has_list, gave_up, dl, warm, n0, n1, ms, seen in itertools.product(
                (-1, 0, 1), (0, 1), (0, 1), (-1, 0, 1), (0, 1), range(4), range(4), ((1, 1), (1, 1.19), (1.19, 1), (1, 1.25), (1.25, 1)),
                (0, 1, 61, 62, 63, 64, 126, 127, 1022, 1023, 1087, 2047)):
            args = (forced, has_list, gave_up, rule_tiles + dl, rule_tiles, warm, (n0, n1), ms, seen)
            want = mode_rule(*args)
            got = ra.frame_mode_probe(*args)
            assert got == (int(want[0]), bool(want[1]), bool(want[2])), (args, got, want)
            checked += 1
            seen_modes.add(got)
    assert checked == 2 * 3 * 2 * 2 * 3 * 2 * 16 * 5 * 12
    assert seen_modes == set(itertools.product((0, 1), (False, True), (False, True))) - {(0, True, False), (1, True, False)}      # (a re-probe is always bracketed)


def rendered_rows(H, own):
    """rendered[y] for y <= H: owned, or with the halo next to an owned row"""
    band, parts, part, halo = own
    y = np.arange(H + 2)
    o = np.ones(H + 2, bool) if band == 0 else (y // band) % parts == part
    assert band == 0 or np.array_equal(y[:H][o[:H]], parallel.owned_rows(H, band, parts, part))
    r = o.copy()
    if halo:
        r[1:] |= o[:-1]
        r[:-1] |= o[1:]
    return o, r


def expected_list(W, H, own, rows, strips, rect):
    """The list by its rules: per queue the entries inside the rectangle, then the others, each in row-then-column order."""
    band, parts, part, _ = own
    row_end = min(rows[1], H)
    last = min(row_end, H - 1)
    tiles_x, n_strips, row0 = (W - 1 + 7) // 8, -(-(W - 1) // 64), rows[0] // 8
    o, r = rendered_rows(H, own)
    queues = [([], []) for _ in range(8)]
    listed = 0
    for ty in range(row0, (H + 7) // 8):
        live = [y for y in range(max(ty * 8, rows[0]), min(ty * 8 + 8, last)) if r[y]]
        if not live or rows[0] >= row_end:
            continue
        t = ty - row0
        q = (t // 8) & 7
        if band:
            y = live[-1]
            b = y // band if o[y] else ((y - 1) // band if y > 0 and o[y - 1] else (y + 1) // band)
            q = ((b // parts) * max(band // 64, 1) + (y % band) // 64) & 7
        in_y = rect[2] <= ty < rect[3]
        if strips and len(live) == 1:
            for sx in range(n_strips):
                inside = in_y and min(sx * 8 + 8, tiles_x) > rect[0] and sx * 8 < rect[1]
                queues[q][0 if inside else 1].append(0x10000000 | sx << 16 | live[0])
            listed += n_strips
        else:
            for tx in range(tiles_x):
                queues[q][0 if in_y and rect[0] <= tx < rect[1] else 1].append(ty << 16 | tx)
            listed += tiles_x
    return queues, listed


def check_list(ra, W, H, own, rows, strips, rect, strips_fit=True):
    got = ra.tile_list_probe(W, H, own, rows, strips, rect)
    queues, listed = expected_list(W, H, own, rows, strips and strips_fit, rect)
    what = (W, H, own, rows, strips, rect)
    base, count = got[0:8].astype(np.int64), got[8:16].astype(np.int64)
    assert base[0] == 16 and np.array_equal(base[1:], base[:-1] + count[:-1]), what      # contiguous from word 16
    assert len(got) == 16 + count.sum() == 16 + listed, what
    entries = got[16:].tolist()
    assert len(set(entries)) == len(entries), what                                            # nothing twice
    assert sorted(entries) == sorted(e for q in queues for c in q for e in c), what            # exactly the rows' tiles / strips
    for x in range(8):
        assert got[base[x]:base[x] + count[x]].tolist() == queues[x][0] + queues[x][1], (what, x)      # queue, class, row-then-column order
    return got


SIZES = [(17, 9), (17, 10), (65, 24), (66, 24), (200, 330), (160, 200)]
OWNERSHIPS = [(b, n, p, h) for (b, n, p) in ((0, 1, 0), (64, 2, 0), (64, 2, 1), (64, 3, 2), (8, 2, 1)) for h in (0, 1)]


@pytest.mark.parametrize("W,H", SIZES)
def test_tile_lists(ra, W, H):
    tiles_x, tiles_y_full = (W - 1 + 7) // 8, (H + 7) // 8
    rects = [(tiles_x, 0, tiles_y_full, 0), (0, tiles_x, 0, tiles_y_full),
             (tiles_x // 3, 2 * tiles_x // 3, tiles_y_full // 3, max(2 * tiles_y_full // 3, tiles_y_full // 3 + 1))]
    ranges = [(0, H), (H - 1, H), (H - 2, H)] + ([(37, 150)] if H >= 150 else [])
    strips_listed = tiles_listed = 0
    for own, rows, strips, rect in itertools.product(OWNERSHIPS, ranges, (False, True), rects):
        got = check_list(ra, W, H, own, rows, strips, rect)
        strips_listed += int((got[16:] & 0x10000000 != 0).sum())
        tiles_listed += int((got[16:] & 0x10000000 == 0).sum())
        if rows == (H - 1, H):
            assert len(got) == 16      # (row H-1 is never rendered)
    assert tiles_listed > 0
    # single live rows: the last tile row of H = 10 (row 8 alone) without ownership, the halo rows of the bands, the range (H - 2, H)
    assert strips_listed > 0


def test_tile_list_of_a_frame_too_tall_for_strips(ra):
    """2 x 32770: a strip entry has 15 bits for its row -- stripsFit turns the strips off and the halo rows are listed as tiles."""
    W, H = 2, 32770
    for own in ((0, 1, 0, 0), (64, 2, 0, 1)):
        got = check_list(ra, W, H, own, (0, H), True, (0, 1, 0, (H + 7) // 8), strips_fit=False)
        assert not (got[16:] & 0xffff).any()      # (tiles of column 0 all: a strip would carry its pixel row here; tile rows from 4096 set bit 28)
    got = check_list(ra, W, 32768, (64, 2, 0, 1), (0, 32768), True, (0, 1, 0, 4096))      # (the tallest frame that fits)
    assert (got[16:] & 0x10000000).any()
