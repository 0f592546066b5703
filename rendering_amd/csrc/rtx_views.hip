// Many views of a scene in one call (rtx_render_views, include/rtx_views.h): pass 1, the Sobel mask and the 4-sample
// pass of every view of a batch in one launch each, for batches of views too small to fill the device one at a time.
//
// A work item is one 8x8 tile of one view (rtx_views_plan.h: the views' tiles numbered view after view).  The camera is the item's, read from
// the view's record (rtxviews::ViewRec) instead of the argument block; everything castRayWave reads again from the argument block --
// bias, depth, background, flags -- is the scene's current view's and so the same for every view of the batch.  The rays are cast with
// CAM = false, as rtxRayColourKernel casts a caller's rays: no ray is taken to start at the scene's camera, so the walks use the prune
// records any ray may use (copy 0), never the camera's copies -- which would be another camera's.  A pixel's colour does not depend on
// that (the records only drop what the reference is certain to reject), so every view gets the bits of rtx_render_pass1 / rtx_sobel /
// rtx_render_ssaa (tests/test_gpu_render_views.py).
//   1. rtxViewsPass1Kernel: persistent waves pop items off one queue head; recursion frames: the pass-1 area (the grid is at most blocksPass1).
//   2. rtxViewsMaskKernel: one wave per item, sobelFlag on the item's 64 pixels; the flagged pixels of the tile go into the batch's list
//      as one run (one atomic per tile), item << 6 | pixel of the tile.
//   3. rtxViewsSsaaKernel: persistent waves pop 16 consecutive list entries x 4 sub-samples, rtxSsaaKernel's item; a wave may hold pixels
//      of several tiles and views, so the view's record is per-lane data there.  Recursion frames: the SSAA area.
// No wave waits for another.
#pragma clang fp contract(off)

#include "rtx_views_plan.h"

using rtxviews::ViewRec;

// What the kernels of a batch read besides the scene: nViews records, the first item of every view (first[nViews] = nItems), the view
// of every item (written by the mask kernel for the SSAA kernel's lanes), the list of flagged pixels, and the heads -- [0] pass 1's queue,
// [16] the list's length, [32] the SSAA queue (64 bytes apart, zero before the first launch).
struct ViewsArgs {
	const ViewRec* views; const uint32_t* first; uint32_t nViews, nItems;
	uint32_t* itemView; uint32_t* list; uint32_t* heads;
};
// One kernel argument, so that the argument block still starts with Params (freshParams) and the batch's part can be read afresh the same way.
struct ViewsKernArgs { Params P; ViewsArgs A; };

namespace {

__device__ __forceinline__ const ViewsArgs& freshViewsArgs(const ViewsKernArgs& K) { return ((const ViewsKernArgs&)freshParams(K.P)).A; }

// The record of an item's view, through the scalar unit (item is wave-uniform).
__device__ __forceinline__ const ViewRec* viewOfItemUni(const ViewsArgs& A, uint32_t item)
{
	const uint32_t* first = uni(A.first);
	const uint32_t v = rtxviews::viewOfItem([&](uint32_t i) { return sload1(first + i); }, uni(A.nViews), item);
	return uni(A.views) + uni(v);
}

// The pixel of lane ln in tile `item` of the view R
__device__ __forceinline__ void pixelOfItem(const ViewRec& R, uint32_t item, uint32_t ln, uint32_t& x, uint32_t& y)
{
	const rtxviews::Tile t = rtxviews::tileOfItem(item, R.firstItem, R.tilesX);
	x = t.tx * 8 + (ln & 7); y = t.ty * 8 + (ln >> 3);
}

} // namespace

template <bool MESH, bool BOXES, int CULLK, bool PLAIN>
__global__ void __launch_bounds__(256, MESH ? (PLAIN ? RTX_WAVES_PLAIN : RTX_WAVES) : RTX_WAVES_ANALYTIC) rtxViewsPass1Kernel(const ViewsKernArgs K)
{
	if (!PLAIN) fillPowTab();
	const uint32_t gl = blockIdx.x * blockDim.x + threadIdx.x;
	Counts cnt = {};
	for (;;) {
		const ViewsArgs& A = freshViewsArgs(K);
		const uint32_t item = nextWork(A.heads);
		if (item >= A.nItems) break;
		V3 c;
		{
			const ViewRec& R = *viewOfItemUni(A, item);
			uint32_t x, y;
			pixelOfItem(R, item, laneNow(), x, y);
			// (the last column and row are never rendered, scene.cpp:369-372: a view one pixel wide or high renders nothing)
			const bool valid = x < R.width - 1 && y < R.height - 1;
			if (ballot(valid) == 0) continue;
			V3 o, d;
			viewRay(R, (float)x + 0.5f, (float)y + 0.5f, o, d);
			if constexpr (PLAIN) c = castRayPlainWave<false, false, BOXES, false, CULLK>(K.P, valid, o, d, gl, cnt);
			else c = castRayWave<false, MESH, false, BOXES, false, CULLK, PLAIN>(K.P, valid, o, d, gl, cnt);
		}
		// where the pixel goes is derived from the item again, as rtxPass1Kernel does, instead of being kept across the rays
		uint32_t itemWas = item;
		asm volatile("" : "+s"(itemWas));
		const ViewRec& R = *viewOfItemUni(freshViewsArgs(K), itemWas);
		uint32_t x, y;
		pixelOfItem(R, itemWas, laneNow(), x, y);
		if (x < R.width - 1 && y < R.height - 1) {
			float* px = R.fb + ((size_t)y * R.width + x) * 3;
			px[0] = c.x; px[1] = c.y; px[2] = c.z;
		}
	}
}
RTX_QUERY_INSTANCES(rtxViewsPass1Kernel, (const ViewsKernArgs), false)
RTX_MESH_INSTANCES(rtxViewsPass1Kernel, (const ViewsKernArgs), true)

// The mask of every pixel of the item's tile (borders 0, as rtxSobelKernel defines them) from the view's pass-1 framebuffer, and the tile's
// flagged pixels appended to the list.  A flagged pixel is an interior one, so it is one the 4-sample pass visits (x < W - 1, y < H - 1).
// The nine pixels are read per lane: the tiles are small and their rows are in the caches.
__global__ void __launch_bounds__(256) rtxViewsMaskKernel(const ViewsArgs A)
{
	const uint32_t item = uni(blockIdx.x * 4 + (threadIdx.x >> 6)), lane = __lane_id();
	if (item >= A.nItems) return;
	const ViewRec* Rp = viewOfItemUni(A, item);
	const ViewRec& R = *Rp;
	const uint32_t W = R.width, H = R.height;
	uint32_t x, y;
	pixelOfItem(R, item, lane, x, y);
	const bool inView = x < W && y < H;
	bool flag = false;
	if (inView && x >= 1 && x + 1 < W && y >= 1 && y + 1 < H) {
		const float* fb = R.fb;
		flag = sobelFlag([&](int a, int b) { return load3(fb + ((size_t)(y - 1 + a) * W + (x - 1 + b)) * 3); });
	}
	if (inView) R.mask[(size_t)y * W + x] = flag ? 1 : 0;
	if (lane == 0) A.itemView[item] = (uint32_t)(Rp - A.views);
	const uint64_t m = ballot(flag);
	if (m == 0) return;
	uint32_t base = 0;
	if (lane == 0) base = atomicAdd(A.heads + 16, (uint32_t)__popcll(m));
	base = __builtin_amdgcn_readfirstlane(base);
	if (flag) A.list[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = item << 6 | lane;
}

// rtxSsaaKernel's item over the batch's list: 16 pixels x 4 sub-samples, the offsets in the reference's order, 0 + c0 + c1 + c2 + c3, / 4.
template <bool MESH, bool BOXES, int CULLK, bool PLAIN>
__global__ void __launch_bounds__(256, MESH ? RTX_WAVES_SSAA : RTX_WAVES_ANALYTIC) rtxViewsSsaaKernel(const ViewsKernArgs K)
{
	if (!PLAIN) fillPowTab();
	const uint32_t gl = blockIdx.x * blockDim.x + threadIdx.x;
	Counts cnt = {};
	for (;;) {
		const ViewsArgs& A = freshViewsArgs(K);
		const uint32_t work = nextWork(A.heads + 32);
		const uint32_t total = sload1(A.heads + 16);
		if ((uint64_t)work * 16 >= total) break;
		// The pixel of a lane and its view's record (per lane: a wave may hold several views), from the work item alone
		auto place = [&](const ViewsArgs& Aa, uint32_t w, uint32_t ln, bool& valid, const ViewRec*& R, uint32_t& x, uint32_t& y) {
			const uint32_t n = sload1(Aa.heads + 16), g = w * 16 + (ln >> 2);
			valid = g < n;
			const uint32_t e = Aa.list[valid ? g : w * 16];
			R = Aa.views + Aa.itemView[e >> 6];
			pixelOfItem(*R, e >> 6, e & 63u, x, y);
		};
		V3 c;
		{
			const uint32_t ln = laneNow(), sub = ln & 3;
			bool valid; const ViewRec* R; uint32_t x, y;
			place(A, work, ln, valid, R, x, y);
			// offsets in the reference's order: (.25,.25) (.25,.75) (.75,.25) (.75,.75)  (scene.cpp:527-534)
			const float fx = (float)x + ((sub & 2) ? 0.75f : 0.25f), fy = (float)y + ((sub & 1) ? 0.75f : 0.25f);
			V3 o, d;
			viewRay(*R, fx, fy, o, d);
			c = castRayWave<false, MESH, true, BOXES, false, CULLK, PLAIN>(K.P, valid, o, d, gl, cnt);
		}
		// color = 0; color += c0; += c1; += c2; += c3; fb = color / 4
		const uint32_t ln = laneNow();
		const int base = (int)(ln & ~3u);
		V3 sum = mk(0, 0, 0);
		for (int k = 0; k < 4; ++k)
			sum = sum + mk(__shfl(c.x, base + k), __shfl(c.y, base + k), __shfl(c.z, base + k));
		uint32_t workWas = work;
		asm volatile("" : "+s"(workWas));
		bool valid; const ViewRec* R; uint32_t x, y;
		place(freshViewsArgs(K), workWas, ln, valid, R, x, y);
		if (valid && (ln & 3) == 0) {
			float* px = R->fb + ((size_t)y * R->width + x) * 3;
			px[0] = sum.x / 4; px[1] = sum.y / 4; px[2] = sum.z / 4;
		}
	}
}
RTX_QUERY_INSTANCES(rtxViewsSsaaKernel, (const ViewsKernArgs), false)
RTX_MESH_INSTANCES(rtxViewsSsaaKernel, (const ViewsKernArgs), true)
