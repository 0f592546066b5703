// The work items of rtx_render_views (include/rtx_views.h): the 8x8 tiles of every view of a batch, numbered view after view
// and row by row inside a view, and the record a kernel reads of a view.  Plain C++ that the host and the kernels both compile (rtx_views.hip,
// rtx_views_api.hip), so that the map from an item to its view and tile exists once and can be checked without a GPU (rtx_views_plan_probe:
// tests/test_render_views_cpu.py).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RTX_VIEWS_HD __host__ __device__ __forceinline__
#else
#define RTX_VIEWS_HD inline
#endif

namespace rtxviews {

// The limits of a batch (include/rtx_views.h states them): an SSAA list entry is item << 6 | pixel of the tile, a queue head counts items.
constexpr uint32_t kMaxViews = 65536u, kMaxSide = 32768u, kMaxItems = 1u << 22;

// What the kernels read of view v: the camera fields under the names of rtxd::View (one primaryRay for both), the buffers, and where the
// view's items start.  128 bytes = two s_load_dwordx16 when a wave is at one view.
struct ViewRec {
	uint32_t width, height;
	float scale, aspect;
	float camPos[3];
	uint32_t firstItem;      // the view's tiles are the items [firstItem, firstItem + tilesX * tilesY)
	float camM[16];
	float* fb;
	uint8_t* mask;
	uint32_t tilesX, pad[3];
};
static_assert(sizeof(ViewRec) == 128, "view record = two 64-byte lines");

// 8x8 tiles that cover w pixels in one dimension / a w x h view (every pixel, the last row and column included: the mask covers them)
RTX_VIEWS_HD uint32_t tilesAcross(uint32_t w) { return (w + 7u) / 8u; }
RTX_VIEWS_HD uint64_t tilesOf(uint32_t w, uint32_t h) { return (uint64_t)tilesAcross(w) * tilesAcross(h); }

// The view of an item: the last v with first(v) <= item, where first(v) is the number of items of the views before v (first(0) = 0 <= item <
// first(nViews); every view has at least one tile, so first is strictly increasing).  `first` is a callable, so that a kernel can read
// the array through the scalar unit.
template <typename First>
RTX_VIEWS_HD uint32_t viewOfItem(First&& first, uint32_t nViews, uint32_t item)
{
	uint32_t lo = 0, hi = nViews;      // first(lo) <= item < first(hi)
	while (hi - lo > 1u) {
		const uint32_t mid = lo + (hi - lo) / 2u;
		if (first(mid) <= item) lo = mid; else hi = mid;
	}
	return lo;
}

// ... and its tile inside the view: tile (tx, ty) covers the pixels [8 tx, 8 tx + 8) x [8 ty, 8 ty + 8)
struct Tile { uint32_t tx, ty; };
RTX_VIEWS_HD Tile tileOfItem(uint32_t item, uint32_t firstItem, uint32_t tilesX)
{
	const uint32_t t = item - firstItem;
	Tile r;
	r.ty = t / tilesX; r.tx = t - r.ty * tilesX;
	return r;
}

} // namespace rtxviews
