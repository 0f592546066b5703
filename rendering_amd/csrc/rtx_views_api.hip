// The host half of the view batches (include/rtx_views.h, include/rtx_views_aov.h): checkViewSizes, the staging of the view records,
// rtx_views_plan_probe, rtx_render_views and rtx_render_views_aov.  Part of rtx_api.hip: uses rtx_views_plan.h, the kernels of rtx_views.hip and
// rtx_views_aov.hip, the selectors of rtx_query.hip and the launch bookkeeping of rtx_api.hip (ensureWork, renderOn).  Opens and closes its own
// extern "C" and namespace blocks.
extern "C" {

namespace {

// What the batch calls and the plan's probe refuse of a batch's sizes; *items = the batch's tiles.  who: the call's name.
int checkViewSizes(const char* who, uint32_t n, const uint32_t* w, const uint32_t* h, size_t stride, uint64_t* items)
{
	const std::string name = who;
	if (n > rtxviews::kMaxViews) return fail(RTX_ERR_ARG, name + ": more than RTX_VIEWS_MAX_VIEWS views");
	uint64_t total = 0;
	for (uint32_t i = 0; i < n; i++) {
		const uint32_t W = *(const uint32_t*)((const char*)w + i * stride), H = *(const uint32_t*)((const char*)h + i * stride);
		if (W == 0 || H == 0) return fail(RTX_ERR_ARG, name + ": view " + std::to_string(i) + " has a zero width or height");
		if (W > rtxviews::kMaxSide || H > rtxviews::kMaxSide) return fail(RTX_ERR_ARG, name + ": view " + std::to_string(i) + " is larger than RTX_VIEWS_MAX_SIDE");
		total += rtxviews::tilesOf(W, H);
	}
	if (total > rtxviews::kMaxItems) return fail(RTX_ERR_ARG, name + ": more than RTX_VIEWS_MAX_TILES tiles in all");
	*items = total;
	return RTX_OK;
}

// The record of view t of a batch (rtx_view_target or rtx_view_aov_target: their size and camera fields are the same) whose items start at
// `at`: the camera and size as the kernels read them, no buffers.  Returns the first item of the next view.
extern "C++" template <typename Target> uint32_t fillViewRec(ViewRec& r, const Target& t, uint32_t at)
{
	r.width = t.width; r.height = t.height; r.scale = t.scale; r.aspect = t.aspect;
	memcpy(r.camPos, t.cam_pos, 12); memcpy(r.camM, t.cam_matrix, 64);
	r.firstItem = at;
	r.fb = nullptr; r.mask = nullptr;
	r.tilesX = rtxviews::tilesAcross(t.width); r.pad[0] = r.pad[1] = r.pad[2] = 0;
	return at + (uint32_t)rtxviews::tilesOf(t.width, t.height);
}

// The staging buffer of the batch calls with `bytes` in it and free to be filled: the previous call's copy out of it has been made (the
// only wait besides the growth of a table).  The calls on one scene never overlap, so rtx_render_views and rtx_render_views_aov share it.
int viewsStageFor(rtx_scene* s, size_t bytes)
{
	if (s->viewsStagePending) { HIPCHK(hipEventSynchronize(s->viewsStaged)); s->viewsStagePending = false; }
	HIPCHK(s->viewsStage.reserve(bytes));
	return RTX_OK;
}

// ... and its copy into the device's table, queued on st with the event the next call waits for
int viewsStageCopy(rtx_scene* s, size_t bytes, hipStream_t st)
{
	HIPCHK(hipMemcpyAsync(s->viewsTable.get(), s->viewsStage.host(), bytes, hipMemcpyHostToDevice, st));
	HIPCHK(s->viewsStaged.create(hipEventDisableTiming));
	HIPCHK(hipEventRecord(s->viewsStaged, st));
	s->viewsStagePending = true;
	return RTX_OK;
}

} // namespace

int rtx_views_plan_probe(uint32_t n_views, const uint32_t* sizes2, uint32_t* items3_out, size_t cap_items, size_t* n_items)
{
	if (!n_items || (n_views && !sizes2)) return fail(RTX_ERR_ARG, "rtx_views_plan_probe: NULL argument");
	uint64_t items = 0;
	if (int rc = checkViewSizes("rtx_render_views", n_views, sizes2, sizes2 + 1, 8, &items)) return rc;
	*n_items = (size_t)items;
	if (!items3_out || cap_items < items) return RTX_OK;
	// the table as rtx_render_views lays it out, read as the kernels read it
	std::vector<uint32_t> first(n_views + 1, 0u);
	for (uint32_t v = 0; v < n_views; v++) first[v + 1] = first[v] + (uint32_t)rtxviews::tilesOf(sizes2[2 * v], sizes2[2 * v + 1]);
	for (uint32_t item = 0; item < (uint32_t)items; item++) {
		const uint32_t v = rtxviews::viewOfItem([&](uint32_t i) { return first[i]; }, n_views, item);
		const rtxviews::Tile t = rtxviews::tileOfItem(item, first[v], rtxviews::tilesAcross(sizes2[2 * v]));
		items3_out[3 * (size_t)item] = v; items3_out[3 * (size_t)item + 1] = t.tx; items3_out[3 * (size_t)item + 2] = t.ty;
	}
	return RTX_OK;
}

int rtx_render_views(rtx_scene* s, uint32_t n_views, const rtx_view_target* views, int with_ssaa, void* stream)
{
	RoctxRange range("Render views (rtx_render_views)");
	if (!s) return fail(RTX_ERR_ARG, "scene is NULL");
	if (n_views == 0) return RTX_OK;
	if (!views) return fail(RTX_ERR_ARG, "rtx_render_views: views is NULL");
	uint64_t items64 = 0;
	if (int rc = checkViewSizes("rtx_render_views", n_views, &views[0].width, &views[0].height, sizeof(rtx_view_target), &items64)) return rc;
	for (uint32_t i = 0; i < n_views; i++) {
		if (!views[i].fb_dev) return fail(RTX_ERR_ARG, "rtx_render_views: view " + std::to_string(i) + " has no framebuffer (fb_dev is NULL)");
		if (with_ssaa && !views[i].mask_dev) return fail(RTX_ERR_ARG, "rtx_render_views: view " + std::to_string(i) + " has no mask (mask_dev is NULL) and SSAA is asked for");
	}
	if (s->params.bandH && s->params.nParts > 1) return fail(RTX_ERR_ARG, "rtx_render_views: the rows are shared among devices (rtx_set_row_ownership); deal out views, not rows");
	if (s->stats) return fail(RTX_ERR_UNSUPPORTED, "rtx_render_views collects no statistics (rtx_counters_enable)");
	if (showNormals(s)) return fail(RTX_ERR_UNSUPPORTED, "rtx_render_views does not render the normals view (RTX_FLAG_SHOW_NORMALS)");
	const uint32_t nItems = (uint32_t)items64;
	// (sizes the recursion frames for the current view's depth; the tile lists, tile costs and events are neither used nor touched from here on)
	int rc = ensureWork(s);
	if (rc) return rc;
	hipStream_t st = (hipStream_t)stream;
	if ((rc = renderOn(s, st))) return rc;
	// the batch's scratch: only a larger batch than any before allocates (which waits for the device)
	const size_t recBytes = (size_t)n_views * sizeof(ViewRec), tableBytes = recBytes + ((size_t)n_views + 1) * sizeof(uint32_t);
	HIPCHK(s->viewsTable.reserve(tableBytes));
	HIPCHK(s->viewsWork.reserve(64));
	if (with_ssaa) { HIPCHK(s->viewsItemView.reserve(nItems)); HIPCHK(s->viewsList.reserve((size_t)nItems * 64)); }
	// the staging buffer is free again once the previous call's copy out of it has been made
	if ((rc = viewsStageFor(s, tableBytes))) return rc;
	ViewRec* recs = (ViewRec*)s->viewsStage.host();
	uint32_t* first = (uint32_t*)(s->viewsStage.host() + recBytes);
	uint32_t at = 0;
	for (uint32_t i = 0; i < n_views; i++) {
		first[i] = at;
		at = fillViewRec(recs[i], views[i], at);
		recs[i].fb = views[i].fb_dev; recs[i].mask = views[i].mask_dev;
	}
	first[n_views] = at;
	if ((rc = viewsStageCopy(s, tableBytes, st))) return rc;
	HIPCHK(hipMemsetAsync(s->viewsWork.get(), 0, 64 * sizeof(uint32_t), st));
	ViewsKernArgs k;
	k.P = s->params;
	k.A.views = (const ViewRec*)s->viewsTable.get(); k.A.first = (const uint32_t*)(s->viewsTable.get() + recBytes);
	k.A.nViews = n_views; k.A.nItems = nItems;
	k.A.itemView = s->viewsItemView; k.A.list = s->viewsList; k.A.heads = s->viewsWork;
	const Variant v = variantOf(s);
	// (the recursion frames of the pass-1 area hold blocksPass1 blocks)
	const uint32_t itemBlocks = (nItems + 3) / 4;
	hipLaunchKernelGGL(viewsPass1Kernel(v), dim3(std::min<uint32_t>((uint32_t)s->blocksPass1, itemBlocks)), dim3(256), 0, st, k);
	HIPCHK(hipGetLastError());
	if (!with_ssaa) return RTX_OK;
	hipLaunchKernelGGL(rtxViewsMaskKernel, dim3(itemBlocks), dim3(256), 0, st, k.A);
	HIPCHK(hipGetLastError());
	// (the list's length is the device's to know: at most four SSAA items per tile, and a wave that finds the queue empty ends at once)
	k.P.frames = s->frames + s->framesArea;
	hipLaunchKernelGGL(viewsSsaaKernel(v), dim3(std::min<uint32_t>((uint32_t)s->blocksSsaa, nItems)), dim3(256), 0, st, k);
	HIPCHK(hipGetLastError());
	return RTX_OK;
}

int rtx_render_views_aov(rtx_scene* s, uint32_t n_views, const rtx_view_aov_target* views, void* stream)
{
	RoctxRange range("First-hit buffers of views (rtx_render_views_aov)");
	const char* who = "rtx_render_views_aov";
	if (!s) return fail(RTX_ERR_ARG, "scene is NULL");
	if (n_views == 0) return RTX_OK;
	if (!views) return fail(RTX_ERR_ARG, "rtx_render_views_aov: views is NULL");
	uint64_t items64 = 0;
	if (int rc = checkViewSizes(who, n_views, &views[0].width, &views[0].height, sizeof(rtx_view_aov_target), &items64)) return rc;
	// one channel set for the batch: view 0's, in ViewAovRec's order
	static const char* const kChannel[8] = { "depth_dev", "object_dev", "triangle_dev", "uv_dev", "normal_dev", "albedo_dev", "position_dev", "rays_dev" };
	auto channels = [](const rtx_view_aov_target& t) {
		const ViewAovRec c = { t.depth_dev, t.object_dev, t.triangle_dev, t.uv_dev, t.normal_dev, t.albedo_dev, t.position_dev, t.rays_dev };
		return c;
	};
	auto presentOf = [](const ViewAovRec& c) {
		const void* const p[8] = { c.depth, c.object, c.triangle, c.uv, c.normal, c.albedo, c.position, c.rays };
		uint32_t m = 0;
		for (int k = 0; k < 8; k++) if (p[k]) m |= 1u << k;
		return m;
	};
	const uint32_t present = presentOf(channels(views[0]));
	if (!present) return fail(RTX_ERR_ARG, "rtx_render_views_aov: no output (all eight channels of view 0 are NULL)");
	for (uint32_t i = 1; i < n_views; i++) {
		const uint32_t differ = presentOf(channels(views[i])) ^ present;
		if (!differ) continue;
		const int k = __builtin_ctz(differ);
		return fail(RTX_ERR_ARG, std::string(who) + ": view " + std::to_string(i) + ((present >> k & 1u) ? " has no " : " has a ") + kChannel[k] + " but view 0 " +
		            ((present >> k & 1u) ? "has one" : "has none") + " (a channel is given in every view of a batch or in none)");
	}
	if (s->params.bandH && s->params.nParts > 1) return fail(RTX_ERR_ARG, "rtx_render_views_aov: the rows are shared among devices (rtx_set_row_ownership); deal out views, not rows");
	if (s->stats) return fail(RTX_ERR_UNSUPPORTED, "rtx_render_views_aov collects no statistics (rtx_counters_enable)");
	const uint32_t nItems = (uint32_t)items64;
	// (no recursion frames, no tile lists, no events: nothing of the scene's frame state is used or touched from here on)
	HIPCHK(hipSetDevice(s->device));
	hipStream_t st = (hipStream_t)stream;
	int rc = renderOn(s, st);
	if (rc) return rc;
	// the batch's table -- the views' records, their channel records, the first item of every view: only a batch of more views than any
	// before allocates (which waits for the device)
	const size_t recBytes = (size_t)n_views * sizeof(ViewRec), chanBytes = (size_t)n_views * sizeof(ViewAovRec);
	const size_t tableBytes = recBytes + chanBytes + ((size_t)n_views + 1) * sizeof(uint32_t);
	HIPCHK(s->viewsTable.reserve(tableBytes));
	if ((rc = viewsStageFor(s, tableBytes))) return rc;
	ViewRec* recs = (ViewRec*)s->viewsStage.host();
	ViewAovRec* chans = (ViewAovRec*)(s->viewsStage.host() + recBytes);
	uint32_t* first = (uint32_t*)(s->viewsStage.host() + recBytes + chanBytes);
	uint32_t at = 0;
	for (uint32_t i = 0; i < n_views; i++) {
		first[i] = at;
		at = fillViewRec(recs[i], views[i], at);
		chans[i] = channels(views[i]);
	}
	first[n_views] = at;
	if ((rc = viewsStageCopy(s, tableBytes, st))) return rc;
	ViewsAovKernArgs k;
	k.P = s->params;
	k.views = (const ViewRec*)s->viewsTable.get(); k.chans = (const ViewAovRec*)(s->viewsTable.get() + recBytes);
	k.first = (const uint32_t*)(s->viewsTable.get() + recBytes + chanBytes);
	k.nViews = n_views; k.nItems = nItems; k.present = present;
	// one wave per item
	const bool surface = (present & (VA_NORMAL | VA_ALBEDO | VA_POSITION)) != 0;
	hipLaunchKernelGGL(viewsAovKernel(variantOf(s), surface), dim3((nItems + 3) / 4), dim3(256), 0, st, k);
	HIPCHK(hipGetLastError());
	return RTX_OK;
}

} // extern "C"
