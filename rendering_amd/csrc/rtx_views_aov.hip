// First-hit buffers and primary rays of many views in one call (rtx_render_views_aov, include/rtx_views_aov.h):
// for every pixel of pass 1 of every view of a batch the channels of rtxAovKernel (rtx_aov.hip), the hit point and the ray itself.
//
// rtxAovKernel's plain grid over rtx_render_views' work items: one wave per 8x8 tile of one view (rtx_views_plan.h: the views' tiles
// numbered view after view), ceil(nItems / 4) blocks, no queue head and nothing to clear.  The camera is the item's, read from the view's
// record (rtxviews::ViewRec, found through the scalar unit as rtxViewsPass1Kernel finds it); the culling flag and what a miss's albedo is
// made of are the scene's current view's, in the argument block.  traceWave runs in its trace-only form with source class 0: the camera's
// copies of the prune records (class 1) belong to the scene's current camera, not to a view of the batch.  The hit is the
// same bits; the walk visits more slots.  No state machine, no park area, no recursion frames -- so the grid is not bounded by the blocks
// the device holds at once.
// SURFACE = false: only the hit record and the ray are written; surfaceAtHit of rtx_rays.hip (shadePrimary and its fetches: uv, normals,
// tangents, maps) is not compiled in.  SURFACE = true: its hit point, normal and albedo are written as well.
#pragma clang fp contract(off)

// The eight channel pointers of a view, in rtx_view_aov_target's order: 64 bytes, one s_load_dwordx16.  The table of these records sits
// beside the table of the ViewRecs (whose fb and mask are NULL here), staged and copied with it.
struct ViewAovRec { float* depth; int32_t* object; int32_t* triangle; float* uv; float* normal; float* albedo; float* position; float* rays; };
static_assert(sizeof(ViewAovRec) == 64, "channel record = one 64-byte line");

// Which channels the batch has (bit k: channel k of ViewAovRec; the same for every view, so wave-uniform and part of the argument block)
enum : uint32_t { VA_DEPTH = 1, VA_OBJECT = 2, VA_TRIANGLE = 4, VA_UV = 8, VA_NORMAL = 16, VA_ALBEDO = 32, VA_POSITION = 64, VA_RAYS = 128 };

// One kernel argument that starts with Params, as ViewsKernArgs does (freshParams): the views' records, their channel records, the first
// item of every view (first[nViews] = nItems).
struct ViewsAovKernArgs {
	Params P;
	const ViewRec* views; const ViewAovRec* chans; const uint32_t* first; uint32_t nViews, nItems, present;
};

namespace {

__device__ __forceinline__ const ViewsAovKernArgs& freshViewsAovArgs(const ViewsAovKernArgs& K) { return (const ViewsAovKernArgs&)freshParams(K.P); }

// The view of an item, through the scalar unit (item is wave-uniform)
__device__ __forceinline__ uint32_t viewIndexUni(const ViewsAovKernArgs& K, uint32_t item)
{
	const uint32_t* first = uni(K.first);
	return uni(rtxviews::viewOfItem([&](uint32_t i) { return sload1(first + i); }, uni(K.nViews), item));
}

// channel pointer k of a record read with one scalar load (said to be global memory: put together from two words it would be a flat address)
template <typename T> __device__ __forceinline__ T* chanPtr(const u32x16& c, int k)
{
	return (T*)(RTX_AS1 T*)(uintptr_t)(((uint64_t)c[2 * k + 1] << 32) | c[2 * k]);
}

} // namespace

template <bool MESH, bool BOXES, int CULLK, bool SURFACE>
__global__ void __launch_bounds__(256) rtxViewsAovKernel(const ViewsAovKernArgs K)
{
	const uint32_t item = uni(blockIdx.x * 4 + (threadIdx.x >> 6));
	if (item >= K.nItems) return;
	V3 o, d;
	Hit h;
	{
		const ViewRec& R = *(uni(K.views) + viewIndexUni(K, item));
		uint32_t x, y;
		pixelOfItem(R, item, laneNow(), x, y);
		// (the last column and row are never rendered: a view one pixel wide or high gets nothing)
		const bool valid = x < R.width - 1 && y < R.height - 1;
		if (ballot(valid) == 0) return;
		viewRay(R, (float)x + 0.5f, (float)y + 0.5f, o, d);
		Counts cnt = {};
		traceWave<false, MESH, false, BOXES, CULLK>(K.P, valid, false, o, d, kFltMax, h, cnt, 0u);
	}
	// where the pixel goes is derived from the item again, as rtxViewsPass1Kernel does, instead of being kept across the walk
	uint32_t itemWas = item;
	asm volatile("" : "+s"(itemWas));
	const ViewsAovKernArgs& F = freshViewsAovArgs(K);
	const uint32_t v = viewIndexUni(F, itemWas);
	const ViewRec& R = *(uni(F.views) + v);
	uint32_t x, y;
	pixelOfItem(R, itemWas, laneNow(), x, y);
	if (!(x < R.width - 1 && y < R.height - 1)) return;
	const u32x16 c = sload16(uni(F.chans) + v);
	const uint32_t present = uni(F.present);
	// The stores of one channel stay together: a tile row's eight lanes write 32 (depth, ids), 64 (uv), 96 (normal, albedo, position) or
	// 192 (rays) consecutive bytes, eight such runs per instruction.
	const size_t i = (size_t)y * R.width + x;
	const bool hit = h.obj >= 0;
	if (present & VA_DEPTH) chanPtr<float>(c, 0)[i] = h.t;      // (a miss keeps the range it started with: FLT_MAX)
	if (present & VA_OBJECT) chanPtr<int32_t>(c, 1)[i] = hit ? h.obj : -1;
	if (present & VA_TRIANGLE) {
		// rtx_cast_rays' record: the triangle of a mesh only (a sphere's or a plane's h.tri is whatever an earlier mesh left)
		const bool mesh = hit && K.P.objects[hit ? h.obj : 0].type == 3;
		chanPtr<int32_t>(c, 2)[i] = mesh ? (int32_t)h.tri : -1;
	}
	if (present & VA_UV) { float* p = chanPtr<float>(c, 3) + i * 2; p[0] = hit ? h.u : -1.f; p[1] = hit ? h.v : -1.f; }
	if (present & VA_RAYS) { float* p = chanPtr<float>(c, 7) + i * 6; store3(p, o); store3(p + 3, d); }
	if (SURFACE) {
		V3 p, n, a;
		float ks;
		surfaceAtHit(K.P, h, o, d, p, n, a, ks);
		if (present & VA_NORMAL) store3(chanPtr<float>(c, 4) + i * 3, n);
		if (present & VA_ALBEDO) store3(chanPtr<float>(c, 5) + i * 3, a);
		if (present & VA_POSITION) store3(chanPtr<float>(c, 6) + i * 3, p);
	}
}
// (each with and without the surface fetch)
RTX_QUERY_INSTANCES(rtxViewsAovKernel, (const ViewsAovKernArgs), false)
RTX_QUERY_INSTANCES(rtxViewsAovKernel, (const ViewsAovKernArgs), true)
