"""The SSAA flagged-pixel list as rtxSsaaCountKernel builds it, derived on the host from the mask and the pass-1 tile costs,
and checked against what the device built (Scene.ssaa_list: the scan offsets of the last render_ssaa)."""
import numpy as np


def flagged_per_tile(mask, tiles_x, tiles):
    """Flagged pixels of every 8x8 tile (ty * tiles_x + tx), counted as the list kernels count them: x < W-1, y < H-1 only."""
    m = np.asarray(mask) != 0
    H, W = m.shape
    m = m.copy()
    m[H - 1, :] = False
    m[:, W - 1] = False
    ty = tiles // tiles_x
    pad = np.zeros((ty * 8, tiles_x * 8), bool)
    pad[:H, :W] = m
    return pad.reshape(ty, 8, tiles_x, 8).sum((1, 3)).ravel().astype(np.int64)


def widths(lst):
    """(slots of every tile in the heavy half, in the normal half) of the list's scan."""
    scan = lst["scan"].astype(np.int64)
    T = lst["tiles"]
    return np.diff(scan[:T + 1]), np.diff(scan[T:2 * T + 1])


def pad16(n):
    return (n + 15) // 16 * 16


def check_list(lst, cost, mask):
    """Every tile's slots against the rule of rtxSsaaCountKernel, for the layout the device chose (lst["local"], lst["sparse"]).
    Which tiles got their spread slots within the budget depends on atomic order: only the total and the alternatives are fixed.
    Returns (per-tile slots, per-tile nf, bool: the tile wanted spread slots, bool: it got them, pixels per wave asked for)."""
    T, tx = lst["tiles"], lst["tiles_x"]
    cost = np.asarray(cost, np.int64).ravel()
    assert lst["scan"] is not None and cost.size == T, (cost.size, T)
    nf = flagged_per_tile(mask, tx, T)
    heavy = cost > lst["heavy_ticks"]
    wh, wn = widths(lst)
    assert (wh[~heavy] == 0).all() and (wn[heavy] == 0).all(), "a tile has slots in the wrong half of the list"
    w = wh + wn
    assert int(lst["scan"][2 * T]) == int(w.sum())
    if not lst["local"]:
        assert np.array_equal(w, nf), "packed list: %d tiles are not nf wide" % int((w != nf).sum())
        z = np.zeros(T, bool)
        return w, nf, z, z, np.full(T, 16)
    very = cost > lst["very"] * lst["heavy_ticks"]
    per = np.full(T, 16)
    if lst["sparse"]:
        per[heavy] = lst["spread_px"]
        per[very] = 1
    else:
        per[very] = lst["spread_px"]
    packed = pad16(nf)
    spread = (nf + per - 1) // per * 16
    want = (per < 16) & (spread > packed)
    got = want & (w == spread)
    assert (w % 16 == 0).all(), "tile-local list: a tile's slots are not whole waves"
    assert np.array_equal(w[~want], packed[~want]), "tiles that ask for no spread slots are not packed"
    assert np.array_equal(w[want & ~got], packed[want & ~got]), "a tile is neither spread nor packed"
    extra = int((w - packed).sum())
    assert extra <= lst["spread_slots"], "%d extra slots handed out, budget %d" % (extra, lst["spread_slots"])
    if int((spread - packed)[want].sum()) <= lst["spread_slots"]:
        assert got.sum() == want.sum(), "the budget covers every tile, but %d of %d are packed" % (int(want.sum() - got.sum()), int(want.sum()))
    return w, nf, want, got, per
