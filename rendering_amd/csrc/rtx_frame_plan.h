// The pure parts of the frame calls of rtx_api.hip: what a call renders of the view (TileGrid), the per-row plan of a tile list and the list it
// stands for (planTileList, expectedTileList), and the one-launch-or-three policy of rtx_render_frame (decideFrameMode).  Plain C++: no HIP call,
// no rtx_scene, no globals -- so that they can be checked without a GPU (rtx_frame_mode_probe, rtx_tile_list_probe: tests/test_frame_plan_cpu.py).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "rtx_device.h"

namespace rtxplan {

// What a call renders of a W x H view in the rows [rowBegin, rowEnd): the 8x8 tiles of pass 1's pixels (the last row and the last column of the
// view are never rendered).  The size limits stay with the calls: they differ by call.
struct TileGrid {
	uint32_t rowBegin, rowEnd, lastRow;      // rowEnd clamped to the view; lastRow exclusive: row H-1 is never rendered
	uint32_t tilesX, tileRow0, tilesY;
	uint32_t tilesXFull, tilesYFull;         // tiles per row and tile rows of the whole frame (tileCost indexing)
	size_t nTiles;
	TileGrid(uint32_t W, uint32_t H, uint32_t rowBegin_, uint32_t rowEnd_)
		: rowBegin(rowBegin_), rowEnd(rowEnd_ > H ? H : rowEnd_), lastRow(rowEnd < H - 1 ? rowEnd : H - 1), tilesX((W - 1 + 7) / 8), tileRow0(rowBegin / 8),
		  tilesY(lastRow > rowBegin ? (lastRow + 7) / 8 - tileRow0 : 0u), tilesXFull((W + 7) / 8), tilesYFull((H + 7) / 8), nTiles((size_t)tilesX * tilesY) {}
	bool noRows() const { return rowBegin >= rowEnd; }
	bool noRenderedRow() const { return lastRow <= rowBegin; }
	// (tilesXFull is ensureWork's to set, tilesYFull the single launch's: no other kernel reads it)
	void writeTo(rtxd::Params& p) const { p.rowBegin = rowBegin; p.rowEnd = rowEnd; p.tilesX = tilesX; p.tileRow0 = tileRow0; p.tilesY = tilesY; p.nTiles = (uint32_t)nTiles; }
};

// multi-GPU row ownership (rtxd::Params): with halo, the rows next to an owned one are rendered as well
struct RowOwnership {
	uint32_t bandH, nParts, part, halo;
	bool owned(uint32_t y) const { return bandH == 0 || (y / bandH) % nParts == part; }
	bool rendered(uint32_t y) const { return owned(y) || (halo && ((y > 0 && owned(y - 1)) || owned(y + 1))); }
};

// A strip entry is 0x10000000 | strip << 16 | y: it needs y < 2^15, strip < 2^12, and plain entries (ty << 16 | tx) that never
// set bit 28, i.e. tile rows below 4096.  Larger frames are listed as tiles only and the kernels are told so (Params::stripBit).
inline bool stripsFit(uint32_t width, uint32_t height) { return height <= 32768u && width <= 262144u; }

// The plan of a tile list: per tile row what it is listed as, its queue and class bases (rtx_kernels.hip, rtxTileListKernel).  O(rows) here, the entries are written
// on the device -- a new view used to cost the host a loop over every tile (262 144 at 4096^2) and a synchronous 1-MB copy.
struct TilePlan {
	std::vector<uint32_t> words;          // the list's header of 16, then four words per tile row
	std::vector<uint8_t> rowQueue;        // per tile row: its queue
	size_t listWords;                     // header + entries of the list
	uint32_t nStrips, in0, in1, sIn0, sIn1;      // 64 x 1 strips per pixel row; the columns inside the meshes' tile rectangle: tiles, strips
};

// The plan of the list of the rows [rowBegin, lastRow) of a view `width` wide: only tile rows with a row this launch renders are listed.  strips
// (already combined with stripsFit): a tile row with a single rendered row is listed as strips.  rect: the tile rectangle [tx0, tx1) x [ty0, ty1)
// that can see a mesh (meshTileRect) -- its tiles go first in their queue.  (The plan does not depend on the view's height.)
inline TilePlan planTileList(uint32_t width, const RowOwnership& own, uint32_t rowBegin, uint32_t lastRow, uint32_t tilesX, uint32_t tileRow0, uint32_t tilesY,
                             bool strips, const uint32_t rect[4])
{
	TilePlan pl;
	const uint32_t W1 = width - 1;                               // (the last column is never rendered)
	const uint32_t nStrips = pl.nStrips = (W1 + 63) / 64;
	pl.in0 = std::min(rect[0], tilesX); pl.in1 = std::min(rect[1], tilesX);
	uint32_t sIn0 = nStrips, sIn1 = 0;                            // strips sx with min(sx * 8 + 8, tilesX) > rect[0] && sx * 8 < rect[1]: a contiguous range
	for (uint32_t sx = 0; sx < nStrips; sx++) {
		const uint32_t tx0 = sx * 8, tx1 = std::min(tx0 + 8, tilesX);
		if (tx1 > rect[0] && tx0 < rect[1]) { sIn0 = std::min(sIn0, sx); sIn1 = std::max(sIn1, sx + 1); }
	}
	pl.sIn0 = sIn0; pl.sIn1 = sIn1;
	std::vector<uint32_t>& plan = pl.words;
	plan.assign(16 + 4 * (size_t)tilesY, 0u);
	pl.rowQueue.assign(tilesY, 0);
	uint32_t cnt[8][2] = {};
	for (uint32_t t = 0; t < tilesY; t++) {
		const uint32_t ty = tileRow0 + t;
		uint32_t live = 0, only = 0;
		for (uint32_t y = std::max(ty * 8, rowBegin); y < std::min(ty * 8 + 8, lastRow); y++) if (own.rendered(y)) { live++; only = y; }
		if (!live) continue;
		// queue = XCD: bands of 8 tile rows are dealt round the eight queues.  When the rows are shared among devices it is
		// the bands of THIS device that are dealt round (band p, p + nParts, ... of the frame would otherwise all land in
		// queue p % 8 for 8 devices, and every wave of the chip would pop from one address); a halo row goes with the band
		// it serves.
		uint32_t xq = (t / 8) & 7u;
		if (own.bandH) {
			uint32_t b = only / own.bandH;
			if (!own.owned(only)) b = (only > 0 && own.owned(only - 1)) ? (only - 1) / own.bandH : (only + 1) / own.bandH;
			xq = ((b / own.nParts) * (own.bandH / 64 ? own.bandH / 64 : 1) + (only % own.bandH) / 64) & 7u;
		}
		const bool inY = ty >= rect[2] && ty < rect[3];
		const bool strip = strips && live == 1;
		const uint32_t n = strip ? nStrips : tilesX;
		const uint32_t nIn = !inY ? 0u : (strip ? (sIn1 > sIn0 ? sIn1 - sIn0 : 0u) : (pl.in1 > pl.in0 ? pl.in1 - pl.in0 : 0u));
		plan[16 + 4 * t] = (strip ? 2u : 1u) | (inY ? 0x100u : 0u);
		plan[17 + 4 * t] = strip ? only : ty;
		plan[18 + 4 * t] = cnt[xq][0]; plan[19 + 4 * t] = cnt[xq][1];      // (relative to the class: made absolute below)
		cnt[xq][0] += nIn; cnt[xq][1] += n - nIn;
		pl.rowQueue[t] = (uint8_t)xq;
	}
	uint32_t qBase[8], total = 16;
	for (int x = 0; x < 8; x++) { qBase[x] = total; plan[x] = total; plan[8 + x] = cnt[x][0] + cnt[x][1]; total += cnt[x][0] + cnt[x][1]; }
	for (uint32_t t = 0; t < tilesY; t++) {
		if (!plan[16 + 4 * t]) continue;
		const uint32_t x = pl.rowQueue[t];
		plan[18 + 4 * t] += qBase[x]; plan[19 + 4 * t] += qBase[x] + cnt[x][0];
	}
	pl.listWords = total;
	return pl;
}

// (tests: the straightforward construction on the host -- one entry after the other, the way rounds 1-4 built the list -- of the list a plan
// stands for: the header of 16, then the eight queues)
inline std::vector<uint32_t> expectedTileList(uint32_t width, uint32_t tilesX, uint32_t tilesY, const uint32_t rect[4], const TilePlan& pl)
{
	const uint32_t W1 = width - 1;
	std::vector<uint32_t> q[8][2];
	for (uint32_t t = 0; t < tilesY; t++) {
		const uint32_t kind = pl.words[16 + 4 * t];
		if (!kind) continue;
		const uint32_t xq = pl.rowQueue[t], val = pl.words[17 + 4 * t];
		const bool inY = (kind & 0x100u) != 0;
		if ((kind & 0xffu) == 2u)
			for (uint32_t sx = 0; sx * 64 < W1; sx++) {
				const uint32_t tx0 = sx * 8, tx1 = std::min(tx0 + 8, tilesX);
				q[xq][(inY && tx1 > rect[0] && tx0 < rect[1]) ? 0 : 1].push_back(0x10000000u | sx << 16 | val);
			}
		else for (uint32_t tx = 0; tx < tilesX; tx++) q[xq][(inY && tx >= rect[0] && tx < rect[1]) ? 0 : 1].push_back(val << 16 | tx);
	}
	std::vector<uint32_t> want(16);
	for (int x = 0; x < 8; x++) {
		want[x] = (uint32_t)want.size();
		want[8 + x] = (uint32_t)(q[x][0].size() + q[x][1].size());
		want.insert(want.end(), q[x][0].begin(), q[x][0].end());
		want.insert(want.end(), q[x][1].begin(), q[x][1].end());
	}
	return want;
}

// One launch or three for a frame (rtx_render_frame): mode 0 three launches, 1 one; reprobe: the frame's time REPLACES what was known of its
// way; probing: the frame is bracketed by its own pair of events.
struct FrameModeChoice { int mode; bool reprobe, probing; };

// forced: -1 measure, 0 / 1 the caller's choice.  hasList: the call renders some row (it has a tile list, whose entry keeps what follows);
// listed: its tiles; warm: the tile costs of the view are known; frameSamples / frameMs: the frames measured either way and the best
// time of each; framesSeen: the frames of this view so far.
inline FrameModeChoice decideFrameMode(int forced, bool hasList, bool fusedGaveUp, uint32_t listed, uint32_t ruleTiles, bool warm,
                                       const uint32_t frameSamples[2], const float frameMs[2], uint32_t framesSeen)
{
	FrameModeChoice c = { 0, false, false };
	if (forced >= 0) { c.mode = forced; return c; }
	if (!hasList) return c;
	// By rule, not by measurement, where the single launch has never won: frames of more than 65 536 listed tiles
	// (8 192 without meshes) are throughput-bound over cheap tiles -- 4096^2: 4.5 ms in one launch against 4.0 in three, 8192^2 18.1
	// against 15.2 -- and probing there cost the headline two slow frames at the start and one in every 64.
	if (listed > ruleTiles) return c;
	// The frame is bracketed by its own pair of events only while the choice is being made or re-examined (the frame that
	// tries the other way every 64 frames and the one before it): an event costs the queue ~5 us.
	// no measured costs yet: by size -- the single launch where the frame is bounded by its slowest tiles; without meshes (cheap,
	// even tiles: cfg3 at 1080p 2.0 ms in one launch, 1.1 in three) only for small frames
	if (!warm) { c.mode = 1; c.probing = true; }
	// not measured twice each yet: in turn
	else if (frameSamples[0] < 2 || frameSamples[1] < 2) { c.mode = (int)(framesSeen & 1u); c.probing = true; }
	else {
		c.mode = frameMs[1] <= frameMs[0] ? 1 : 0;
		// (the other way is tried again every 64 frames -- every 1024 when it lost by more than a fifth)
		const float lo = std::min(frameMs[0], frameMs[1]), hi = std::max(frameMs[0], frameMs[1]);
		if (((framesSeen & 63u) == 63u && hi <= 1.2f * lo) || (framesSeen & 1023u) == 1023u) { c.mode ^= 1; c.reprobe = true; }
		else if ((framesSeen & 63u) == 62u) c.reprobe = true;      // (the frame before: the current way's time is refreshed as well)
		c.probing = (framesSeen & 63u) >= 62u;
	}
	// the single launch once ended with an error for this view: three launches from then on (bracketed as it would have been)
	if (fusedGaveUp) { c.mode = 0; c.reprobe = false; }
	return c;
}

} // namespace rtxplan
