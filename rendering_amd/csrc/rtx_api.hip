// C-ABI implementation (include/rtx.h): one-time flatten+upload of the scene into HBM and the launches of
// the gfx950 kernels in rtx_kernels.hip.  No CPU fallback exists: without a HIP device every entry point
// fails with RTX_ERR_NO_DEVICE / RTX_ERR_DEVICE.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <dlfcn.h>
#include <algorithm>
#include <array>
#include <functional>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/rtx.h"
#include "../../include/rtx_debug.h"
#include "../../include/rtx_scene_edit.h"
#include "../../include/rtx_query.h"
#include "../../include/rtx_aov.h"
#include "../../include/rtx_ao.h"
#include "../../include/rtx_surface.h"
#include "../../include/rtx_light.h"
#include "../../include/rtx_scatter.h"
#include "../../include/rtx_points.h"
#include "../../include/rtx_project.h"
#include "../../include/rtx_render_light.h"
#include "../../include/rtx_radiance.h"
#include "../../include/rtx_views.h"
#include "../../include/rtx_views_aov.h"
#include "rtx_device.h"
#include "rtx_frame_plan.h"
#include "rtx_own.h"

using namespace rtxd;
using rtxown::DevArray; using rtxown::DevBag; using rtxown::Event; using rtxown::PinnedArray;

// single translation unit: the kernels are compiled together with their launch code
#include "rtx_kernels.hip"
#include "rtx_source.hip"
#include "rtx_rays.hip"
#include "rtx_views.hip"
#include "rtx_aov.hip"
#include "rtx_ao.hip"
#include "rtx_surface.hip"
#include "rtx_light.hip"
#include "rtx_scatter.hip"
#include "rtx_points.hip"
#include "rtx_project.hip"
#include "rtx_render_light.hip"
#include "rtx_radiance.hip"
#include "rtx_views_aov.hip"
#undef RTX_QUERY_INSTANCES
#undef RTX_MESH_INSTANCES
#undef RTX_WALK_RANGE
#undef RTX_ANY_HIT
#undef RTX_AO_DIRECTIONS
#undef RTX_TILE_PIXEL
// ... and the macros of the kernel layers (rtx_wave.h, rtx_math.h, rtx_kernels.hip): no host code below uses one
#undef F
#undef RTX_AS4
#undef RTX_AS1
#undef RTX_EPS8
#undef RTX_AGENT
#undef RTX_FRAME_QUEUES
#undef RTX_LEAF_BATCH_MAX
#undef RTX_T0
#undef RTX_ACC
#undef RTX_DBG_ONLY
#undef RTX_TRACE_ONLY

// rtx_sort.hip
hipError_t rtxSortRayKeys(void* temp, size_t* tempBytes, const uint32_t* keysIn, uint32_t* keysOut, uint32_t* order, uint32_t n, int endBit,
                          hipStream_t st);

#include "rtx_host.h"       // gErr, fail, HIPCHK, the roctx ranges, dispatchVariant
#include "rtx_scene.h"      // Knobs, rtx_scene, Variant, variantOf

namespace {

// The product ignores RTX_* environment variables: a stray RTX_NO_PRUNE / RTX_FRAME_MODE in a caller's environment must not change what
// is launched.  RTX_ALLOW_ENV_KNOBS=1 (the A/B tools under tools/) lets them through; tests use rtx_set_knob (include/rtx_debug.h).
void readKnobs(Knobs& k)
{
	const char* allow = ::getenv("RTX_ALLOW_ENV_KNOBS");
	if (!(allow && allow[0] == '1')) return;
	auto getenv = [](const char* name) { return ::getenv(name); };
	auto num = [](const char* name, long long dflt) { const char* e = ::getenv(name); return e ? strtoll(e, nullptr, 10) : dflt; };
	k.pass1BlocksPerCU = (int)num("RTX_PASS1_BLOCKS_PER_CU", 0); k.ssaaBlocksPerCU = (int)num("RTX_SSAA_BLOCKS_PER_CU", 0); k.frameBlocksPerCU = (int)num("RTX_FRAME_BLOCKS_PER_CU", 0);
	k.prune = !getenv("RTX_NO_PRUNE");
	k.sources = !getenv("RTX_NO_SRC");
	k.pruneBoxes = (int)num("RTX_PRUNE_BOXES", -1);
	k.estimate = !getenv("RTX_NO_COST_ESTIMATE");
	k.estimateShadows = !getenv("RTX_NO_SHADOW_ESTIMATE");
	if (const char* e = getenv("RTX_COST_COEFFS")) sscanf(e, "%f,%f,%f", &k.costPerRef, &k.costPerLeaf, &k.costBase);
	if (const char* e = getenv("RTX_FAT_FACTOR")) k.fatFactor = strtof(e, nullptr);
	k.stripLimit = (uint32_t)num("RTX_STRIP_LIMIT", k.stripLimit);
	k.heavyTicks = (uint32_t)num("RTX_SSAA_HEAVY_TICKS", k.heavyTicks);
	k.spreadSlots = (uint32_t)std::min<long long>(num("RTX_SSAA_SPREAD_SLOTS", k.spreadSlots), 1ll << 20);
	k.splitPercent = (uint32_t)num("RTX_SPLIT_PERCENT", k.splitPercent);
	k.localBelow = num("RTX_SSAA_LOCAL_BELOW", -1);
	k.sparseBelow = num("RTX_SSAA_SPARSE_BELOW", -1);
	if (const char* e = getenv("RTX_FRAME_MODE")) k.frameMode = !strcmp(e, "split") ? 0 : (!strcmp(e, "fused") ? 1 : -1);
	k.frameQueueCap = (uint32_t)num("RTX_FRAME_QUEUE_CAP", 0);
	k.debugItems = getenv("RTX_DEBUG_ITEMS") != nullptr;
	if (const char* e = getenv("RTX_DBG_TILE")) { unsigned tx = 0, ty = 0; if (sscanf(e, "%u,%u", &tx, &ty) == 2) k.dbgTile = ((ty << 16) | tx) + 1; }
}

// The kernel variant with the box test of the prune records (rtx_scene_create's rule over the current records; again after an
// edit, rtx_edit.hip, and after the knob prune_boxes).
void chooseBoxPrune(rtx_scene* s)
{
	s->boxPrune = false;
	for (const Object& d : s->objectRecs) {
		if (d.type != RTX_OBJ_MESH) continue;
		if (d.pruneBoxes && s->knobs.pruneBoxes != 0) s->boxPrune = true;
		if (s->knobs.pruneBoxes > 0 && d.prune) s->boxPrune = true;
	}
}

int setView(rtx_scene* s, const rtx_view* v)
{
	if (v->width < 2 || v->height < 2) return fail(RTX_ERR_ARG, "view: width/height must be >= 2");
	View& d = s->params.view;
	d.width = v->width; d.height = v->height; d.bias = v->bias; d.maxDepth = v->max_ray_depth;
	memcpy(d.bg, v->background, 12);
	d.flags = v->flags;
	memcpy(d.camPos, v->cam_pos, 12);
	memcpy(d.camM, v->cam_matrix, 64);
	d.scale = v->scale; d.aspect = v->aspect;
	if ((d.flags & RTX_FLAG_SKYBOX) && !s->params.sky) return fail(RTX_ERR_ARG, "view: skybox flag without skybox faces");
	if (d.maxDepth < 0) d.maxDepth = -1;
	return RTX_OK;
}

constexpr size_t kMaxTimedLaunches = 4096;
constexpr uint32_t kSsaaSpreadSlots = 1u << 20;
constexpr size_t kFrameCtlBytes = 256 * 64;      // the frame kernel's control block (FC_* in rtx_kernels.hip), every word on its own line

// The kernel of each frame family for a variant; the third flag of dispatchVariant is PLAIN.  (The query families, whose template
// parameters come in another order, have their selectors in rtx_query.hip.)
typedef void (*FrameKernel)(const Params);
FrameKernel pass1Kernel(const Variant& v)
{
	if (v.stats) return rtxPass1Kernel<true>;
	if (v.analytic) return rtxPass1Kernel<false, false>;
	return dispatchVariant(v.boxes, v.cull, v.plain, [](auto b, auto c, auto pl) -> FrameKernel { return rtxPass1Kernel<false, true, decltype(b)::value, decltype(c)::value, decltype(pl)::value>; });
}
FrameKernel ssaaKernel(const Variant& v)
{
	if (v.stats) return rtxSsaaKernel<true>;
	if (v.analytic) return rtxSsaaKernel<false, false>;
	return dispatchVariant(v.boxes, v.cull, v.plain, [](auto b, auto c, auto pl) -> FrameKernel { return rtxSsaaKernel<false, true, decltype(b)::value, decltype(c)::value, decltype(pl)::value>; });
}
FrameKernel frameKernel(const Variant& v)      // (rtx_render_frame has no instrumented variant)
{
	if (v.analytic) return rtxFrameKernel<false>;
	return dispatchVariant(v.boxes, v.cull, v.plain, [](auto b, auto c, auto pl) -> FrameKernel { return rtxFrameKernel<true, decltype(b)::value, decltype(c)::value, decltype(pl)::value>; });
}

// Blocks of `kernel` (256 threads) a CU holds at once, as the runtime answers.
int askBlocksPerCU(int& perCU, const void* kernel)
{
	HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, kernel, 256, 0));
	perCU = std::max(perCU, 1);
	return RTX_OK;
}

// ... and of the whole device, at most `knobPerCU` per CU when that knob is set
int residentBlocks(const rtx_scene* s, FrameKernel kernel, int knobPerCU, int* blocks)
{
	int b;
	const int rc = askBlocksPerCU(b, (const void*)kernel);
	if (rc) return rc;
	if (knobPerCU >= 1 && knobPerCU < b) b = knobPerCU;
	*blocks = b * s->numCUs;
	return RTX_OK;
}

// The grids of the persistent launches.  The occupancy is asked of the mesh kernels with the box test and culling, whatever variant the
// scene launches: PLAIN counts for pass 1 only (a PLAIN scene's pass-1 kernels may hold more blocks per CU than the general ones:
// RTX_WAVES_PLAIN), a scene without meshes for the frame kernel only.  Again when the kernel family changes (rtx_scene_set_lights).
int askResidentBlocks(rtx_scene* s)
{
	Variant v = { false, false, true, true, s->plain };
	int rc;
	if ((rc = residentBlocks(s, pass1Kernel(v), s->knobs.pass1BlocksPerCU, &s->blocksPass1))) return rc;
	v.plain = false;
	if ((rc = residentBlocks(s, ssaaKernel(v), s->knobs.ssaaBlocksPerCU, &s->blocksSsaa))) return rc;
	v.analytic = s->analytic;
	return residentBlocks(s, frameKernel(v), s->knobs.frameBlocksPerCU, &s->blocksFrame);
}

int ensureWork(rtx_scene* s)
{
	HIPCHK(hipSetDevice(s->device));
	if (!s->work) {
		HIPCHK(s->work.reserve(256));
		HIPCHK(hipMemset(s->work, 0, 256 * sizeof(uint32_t)));
		HIPCHK(s->orderWork.reserve(8 * 32 * 32));      // rtxTileOrderKernel: entries per (queue, block, class)
		HIPCHK(s->counters.reserve(16));
		HIPCHK(hipMemset(s->counters, 0, 16 * sizeof(unsigned long long)));
		const int rc = askResidentBlocks(s);
		if (rc) return rc;
	}
	const int blocks = std::max(s->blocksFrame, s->blocksPass1 > s->blocksSsaa ? s->blocksPass1 : s->blocksSsaa);
	const uint32_t totalLanes = (uint32_t)blocks * 256u;
	const int slots = s->params.view.maxDepth + 2;
	// two areas: pass-1 launches use the first, SSAA launches the second (the two may run concurrently on two streams)
	const size_t area = (size_t)(slots < 1 ? 1 : slots) * kFrameFields * sizeof(float) * totalLanes;
	const size_t need = 2 * area;
	s->framesArea = area / sizeof(float);
	HIPCHK(s->frames.reserve(need / sizeof(float)));
	const uint32_t txFull = (s->params.view.width + 7) / 8, tyFull = (s->params.view.height + 7) / 8;
	const size_t tiles = (size_t)txFull * tyFull;
	if (tiles > s->tileCap) {
		s->tileCap = 0;      // (until both are in place)
		HIPCHK(s->tileCost.reserve(2 * tiles));      // pass-1 cost of every tile; its slowest SSAA item (rtxSsaaKernel)
		HIPCHK(s->items.reserve(tiles * 2 + 1 + tiles / 256 + 1024));
		HIPCHK(hipMemset(s->tileCost, 0, 2 * tiles * sizeof(uint32_t)));
		s->tileCap = tiles;
	}
	// every tile's pixels padded to whole waves, plus kSsaaSpreadSlots for the tiles that get 4-pixel waves (a slot budget
	// enforced on the device by rtxSsaaCountKernel: a tile over the budget is packed normally)
	const size_t pixels = tiles * 64 + kSsaaSpreadSlots;
	HIPCHK(s->ssaaPixels.reserve(pixels));
	s->params.tileCost = s->tileCost;
	s->params.tilesXFull = txFull;
	s->params.frames = s->frames;
	s->params.totalLanes = totalLanes;
	s->params.workCounter = s->work;
	s->params.counters = s->counters;
	return RTX_OK;
}

int prepareView(rtx_scene* s);

// Order of the null-stream preparation work against the caller's render stream (see rtx_scene::lastRenderStream).
int prepBegin(rtx_scene* s)
{
	for (auto& rs : s->renderStreams) {
		if (!rs.active) continue;
		HIPCHK(rs.done.create(hipEventDisableTiming));
		// (a stream the caller has destroyed since is reported as an invalid handle: nothing of it can still be running)
		if (hipEventRecord(rs.done, rs.st) == hipSuccess) HIPCHK(hipStreamWaitEvent(nullptr, rs.done, 0));
		else (void)hipGetLastError();
		rs.active = false;
	}
	return RTX_OK;
}
int prepEnd(rtx_scene* s)
{
	HIPCHK(s->evPrepDone.create(hipEventDisableTiming));
	HIPCHK(hipEventRecord(s->evPrepDone, nullptr));
	s->prepRecorded = true; s->prepSeenBy = nullptr;
	for (auto& rs : s->renderStreams) rs.prepSeen = false;
	return RTX_OK;
}
// every entry point that launches on the caller's stream calls this first
int renderOn(rtx_scene* s, hipStream_t st)
{
	s->lastRenderStream = st; s->rendered = true;
	if (st == nullptr) return RTX_OK;      // (the legacy null stream orders itself against the preparation)
	rtx_scene::RenderStream* rs = nullptr;
	for (auto& r : s->renderStreams) if (r.st == st) { rs = &r; break; }
	if (!rs) {
		// (a handful of streams per scene; the oldest idle entry is recycled beyond 8 -- its stream has been waited for by the last preparation)
		if (s->renderStreams.size() >= 8) { for (auto& r : s->renderStreams) if (!r.active) { rs = &r; break; } }
		if (!rs) { s->renderStreams.emplace_back(); rs = &s->renderStreams.back(); }
		rs->st = st; rs->active = false; rs->prepSeen = false;
	}
	if (s->prepRecorded && !rs->prepSeen) { HIPCHK(hipStreamWaitEvent(st, s->evPrepDone, 0)); rs->prepSeen = true; s->prepSeenBy = st; }
	rs->active = true;
	return RTX_OK;
}

// The source copies of every mesh's prune records (rtx_source.hip): copy 1 for the camera of the current view, copy 2 + l for point
// light l.  The camera's is rebuilt when the camera moved, the lights' when the bias changed (a shadow ray starts bias along the
// shading normal off the surface, so it passes the light at that distance: sigma).  Part of setting the view, like the tile lists.
int buildSources(rtx_scene* s)
{
	if (s->srcMeshes.empty() || !s->knobs.sources) return RTX_OK;
	const View& v = s->params.view;
	const bool camSame = s->srcCamBuilt && !memcmp(s->srcBuiltCam, v.camPos, 12);
	const bool lightsSame = s->srcLightsBuilt && s->srcBuiltBias == v.bias;
	if (camSame && lightsSame) return RTX_OK;
	bool any = false;
	for (const auto& sm : s->srcMeshes) any = any || sm.base;
	if (!any) return RTX_OK;
	// (a launch may still be reading the copies: the null stream is ordered behind it -- prepBegin)
	const uint32_t nLights = std::min<uint32_t>((uint32_t)s->srcLightPos.size(), kMaxSrcLights);
	bool failed = false;      // (a copy that could not be reset must not be marked as built: it may hold an older camera's P)
	for (const auto& sm : s->srcMeshes) {
		if (!sm.base) continue;
		auto build = [&](uint32_t copy, const float* S, double sigma, bool cam) {
			PruneBlock* dst = sm.base + (size_t)copy * sm.nWide;
			// (back to copy 0 first: a slot the kernel leaves alone must not keep the P of an earlier camera)
			if (hipMemcpyAsync(dst, sm.base, (size_t)sm.nWide * sizeof(PruneBlock), hipMemcpyDeviceToDevice, nullptr) != hipSuccess) { failed = true; return; }
			if (!(sigma >= 0.0) || !std::isfinite(sigma) || !std::isfinite((double)S[0] + S[1] + S[2])) return;      // no certificate: the copy stays generic
			hipLaunchKernelGGL(rtxsrc::rtxSourceRefKernel, dim3((sm.nRefs + 255) / 256), dim3(256), 0, nullptr, sm.refA, sm.refB, sm.refC, sm.nRefs,
			                   (double)S[0], (double)S[1], (double)S[2], sigma, cam ? 1 : 0, sm.refP, sm.blockP);
			hipLaunchKernelGGL(rtxsrc::rtxSourceSlotKernel, dim3(sm.nWide * (kWideSlots / 4)), dim3(256), 0, nullptr, sm.slotRange, sm.nWide, (const float*)sm.refP, (const float*)sm.blockP, dst);
		};
		if (!camSame) build(1, v.camPos, 0.0, true);
		if (!lightsSame)
			for (uint32_t l = 0; l < nLights; l++) {
				if (!s->srcLightIsPoint[l]) continue;      // (its copy stays generic; the kernels never select it)
				if (s->srcBuiltBias == v.bias && l < s->srcLightFresh.size() && s->srcLightFresh[l]) continue;      // (a light rtx_scene_set_lights left where it was)
				// the line of a shadow ray -- orig = P + N bias, dir = -normalize(P - pos), both rounded (scene.cpp:787, lights.cpp:32-38) -- passes
				// pos within |N| bias (1 + 2 u) + sqrt(3) u (3.01 |P|_inf + 2.01 |pos|_inf); |P|_inf <= vmax + kSrcAinfMax + |N| bias for the
				// origins pruneAlive lets the copy serve.  Twice the rounding part for good measure.
				const float* lp = s->srcLightPos[l].data();
				const double nb = (double)s->srcNmax * std::fabs((double)v.bias);
				const double lpm = std::max(std::fabs((double)lp[0]), std::max(std::fabs((double)lp[1]), std::fabs((double)lp[2])));
				const double sigma = nb * 1.001 + 4.0 * 0x1p-24 * (3.01 * ((double)sm.vmax + kSrcAinfMax + nb) + 2.01 * lpm);
				build(2 + l, lp, sigma, false);
			}
	}
	HIPCHK(hipGetLastError());
	s->srcLightFresh.clear();
	if (failed) { s->srcCamBuilt = false; s->srcLightsBuilt = false; return fail(RTX_ERR_DEVICE, "buildSources: a source copy of the prune records could not be reset"); }
	memcpy(s->srcBuiltCam, v.camPos, 12); s->srcCamBuilt = true;
	s->srcBuiltBias = v.bias; s->srcLightsBuilt = true;
	return RTX_OK;
}

// First-frame cost estimate of the current view into tileCost (rtx_kernels.hip, rtxCostSplatKernel).  Part of loading the
// scene / setting the view, like the upload: the reference's "Render scene" timer starts after its loader too.
int estimateCosts(rtx_scene* s)
{
	s->costsUsable = false;
	if (!s->knobs.estimate || s->meshLeaves.empty() || !s->tileCost) return RTX_OK;
	const View& v = s->params.view;
	const uint32_t txFull = (v.width + 7) / 8, tyFull = (v.height + 7) / 8;
	const uint32_t gridW = (txFull + 1) / 2, gridH = (tyFull + 1) / 2;
	const size_t cells = (size_t)gridW * gridH;
	HIPCHK(s->costGrid.reserve(2 * cells));
	HIPCHK(hipMemsetAsync(s->costGrid, 0, 2 * cells * sizeof(uint32_t), nullptr));
	// the camera's splat and the leaves' shadows on the planes, per point / distant light (rtxCostSplatKernel): one launch per set of leaves
	SplatSources src;
	memset(&src, 0, sizeof(src));
	if (s->knobs.estimateShadows)
		for (size_t l = 0; l < s->estLights.size() && l < 8; l++)
			for (size_t q = 0; q < s->estPlanes.size() && q < 4 && src.n < 16; q++) {
				const auto& L = s->estLights[l]; const auto& P = s->estPlanes[q];
				// (kind 1 distant, 2 point; an area light: 2 + 4 n_points -- the weight of its shadow in the estimate)
				src.kind[src.n] = L[3] > 2.5f ? 2 : (int32_t)L[3]; src.weight[src.n] = L[3] > 2.5f ? (uint32_t)((L[3] - 2.0f) / 4.0f) : 1u;
				memcpy(src.l[src.n], L.data(), 12); memcpy(src.p[src.n], P.data(), 24);
				src.n++;
			}
	for (const auto& m : s->meshLeaves)
		if (m.n) hipLaunchKernelGGL(rtxCostSplatKernel, dim3((m.n + 255) / 256, 1 + src.n), dim3(256), 0, nullptr, m.boxes, m.n, v, gridW, gridH, s->costGrid, src);
	const uint32_t tiles = txFull * tyFull;
	FarPlanes far;
	memset(&far, 0, sizeof(far));
	if (s->knobs.estimateShadows) {      // (the horizon of a plane: rtxCostFillKernel)
		for (size_t q = 0; q < s->estPlanes.size() && q < 4; q++) memcpy(far.p[far.n++], s->estPlanes[q].data(), 24);
		far.farDist = 1500.0f; far.farTicks = 200000u;      // (8192^2 headline scene, by tile row below the horizon: ~3 000 units 0.43 ms mean / 1.5 ms max, 1 000 units and nearer 0.06 ms like any floor tile)
	}
	hipLaunchKernelGGL(rtxCostFillKernel, dim3((tiles + 255) / 256), dim3(256), 0, nullptr, (const uint32_t*)s->costGrid, gridW, txFull, tyFull, s->tileCost,
	                   s->knobs.costPerRef, s->knobs.costPerLeaf, s->knobs.costBase, v, far);
	HIPCHK(hipGetLastError());
	s->costsUsable = true;
	return RTX_OK;
}

// Records an event on `st`; events come in (start, stop) pairs per launch.
int stamp(rtx_scene* s, int which, hipStream_t st)
{
	if ((s->evUsed[which] & 1) == 0 && s->evUsed[which] >= 2 && (!s->evCollect || s->evUsed[which] >= 2 * kMaxTimedLaunches))
		s->evUsed[which] -= 2;          // start of a launch: recycle the previous pair
	if (s->evUsed[which] == s->evPool[which].size()) {
		Event e;
		HIPCHK(e.create());
		s->evPool[which].push_back(std::move(e));
	}
	HIPCHK(hipEventRecord(s->evPool[which][s->evUsed[which]++], st));
	return RTX_OK;
}

} // namespace

// device-side acceleration-structure build (uses fail / HIPCHK above)
#include "rtx_bvh.hip"

// the flatten of a mesh on the host and on the device (uses the scene's internals above and the tree of rtx_bvh.hip)
#include "rtx_flatten.hip"

// loading a scene: checks, uploads, rtx_scene_create / destroy / set_view (uses the view preparation above and uploadMeshGeometry of rtx_flatten.hip)
#include "rtx_upload.hip"

extern "C" {

namespace {

// Tile rectangle [tx0, tx1) x [ty0, ty1) that can see the root box of some mesh through the camera (conservative; the
// whole frame when a box reaches behind the camera).  Inverse of primaryRay(): dir = normalize(xp, yp, -1) . M3 with an
// orthonormal M3 (rMatrix, scene.cpp:22-49), so camera-space s = (P - camPos) . M3^T.
void meshTileRect(const rtx_scene* s, uint32_t tilesX, uint32_t tilesYFull, uint32_t r[4])
{
	const View& v = s->params.view;
	r[0] = tilesX; r[1] = 0; r[2] = tilesYFull; r[3] = 0;
	const float* M = v.camM;
	for (size_t m = 0; m + 6 <= s->meshBounds.size(); m += 6) {
		const float* b = &s->meshBounds[m];
		double x0 = 1e300, x1 = -1e300, y0 = 1e300, y1 = -1e300;
		bool behind = false;
		for (int c = 0; c < 8; c++) {
			const double P[3] = { b[(c & 1) ? 3 : 0] - v.camPos[0], b[(c & 2) ? 4 : 1] - v.camPos[1], b[(c & 4) ? 5 : 2] - v.camPos[2] };
			const double sx = P[0] * M[0] + P[1] * M[1] + P[2] * M[2], sy = P[0] * M[4] + P[1] * M[5] + P[2] * M[6], sz = P[0] * M[8] + P[1] * M[9] + P[2] * M[10];
			if (!(sz < -1e-6)) { behind = true; break; }
			const double xp = sx / -sz, yp = sy / -sz;
			const double px = (xp / ((double)v.scale * v.aspect) + 1) * 0.5 * v.width - 1.0, py = (-yp / (double)v.scale + 1) * 0.5 * v.height - 1.0;
			x0 = std::min(x0, px); x1 = std::max(x1, px); y0 = std::min(y0, py); y1 = std::max(y1, py);
		}
		if (behind || !(x0 <= x1) || !std::isfinite(x0 + x1 + y0 + y1)) { r[0] = 0; r[1] = tilesX; r[2] = 0; r[3] = tilesYFull; return; }
		auto lo = [](double p) { const double t = std::floor(p / 8.0) - 1; return t < 0 ? 0u : (uint32_t)std::min(t, 65535.0); };
		auto hi = [](double p, uint32_t cap) { const double t = std::floor(p / 8.0) + 2; return t < 0 ? 0u : (uint32_t)std::min<double>(t, cap); };
		r[0] = std::min(r[0], lo(x0)); r[1] = std::max(r[1], hi(x1, tilesX)); r[2] = std::min(r[2], lo(y0)); r[3] = std::max(r[3], hi(y1, tilesYFull));
	}
}

using rtxplan::TileGrid; using rtxplan::TilePlan; using rtxplan::stripsFit;

// The steps of buildTileList, in its order.  The key: what a list is built for (view, row range, row ownership).
void tileListKey(const Params& p, uint32_t rowBegin, uint32_t lastRow, uint32_t tilesX, bool strips, std::vector<uint32_t>& key)
{
	key = { rowBegin, lastRow, tilesX, p.bandH, p.nParts, p.part, p.halo, p.view.width, p.view.height, strips ? 1u : 0u };
	for (int i = 0; i < 16; i++) { uint32_t w; memcpy(&w, &p.view.camM[i], 4); key.push_back(w); }
	for (int i = 0; i < 3; i++) { uint32_t w; memcpy(&w, &p.view.camPos[i], 4); key.push_back(w); }
	{ uint32_t w; memcpy(&w, &p.view.scale, 4); key.push_back(w); memcpy(&w, &p.view.aspect, 4); key.push_back(w); }
}

// The cached list with this key (*out; none: nullptr), ordered in front of what `st` is given next.
int findTileList(rtx_scene* s, const std::vector<uint32_t>& key, hipStream_t st, rtx_scene::TileQueues** out)
{
	*out = nullptr;
	for (auto& q : s->tileQueues)
		if (q.list && q.key == key) {
			// (written on another stream -- the null stream of prepareView is covered by evPrepDone, a caller's second render stream is not: ADVICE r5)
			if (q.builtEv && q.builtOn != st && q.builtOn != nullptr && st != nullptr) HIPCHK(hipStreamWaitEvent(st, q.builtEv, 0));
			q.lastUse = ++s->tileUse; *out = &q; return RTX_OK;
		}
	return RTX_OK;
}

// new entry (the least recently used one is recycled once there are 16; callers keep pointers to entries across calls
// that may add one: the vector never reallocates)
rtx_scene::TileQueues* recycleTileList(rtx_scene* s)
{
	if (s->tileQueues.capacity() < 16) s->tileQueues.reserve(16);
	if (s->tileQueues.size() < 16) s->tileQueues.emplace_back();
	rtx_scene::TileQueues* e = &s->tileQueues[0];
	for (auto& q : s->tileQueues) { if (!q.list) { e = &q; break; } if (q.lastUse < e->lastUse) e = &q; }
	e->forget();
	return e;
}

// Room for a list of listWords in entry e's part of the slab, and for its ordered copy.
int ensureListSlabs(rtx_scene* s, rtx_scene::TileQueues* e, size_t listWords)
{
	const Params& p = s->params;
	// (every list of this view fits 16 + the frame's tiles: a strip row has fewer entries than a tile row.  Sized for that at once, so that the
	// second list of a frame -- tiles after strips, an owned band after the whole frame -- never grows the slab under a `tq` the caller holds: ADVICE r5)
	const size_t frameWords = 16 + (size_t)((p.view.width + 7) / 8) * ((p.view.height + 7) / 8);
	if (std::max(listWords, frameWords) > s->listStride) {
		HIPCHK(hipDeviceSynchronize());      // (growing: an earlier launch may still be reading the buffer that is freed)
		s->listStride = 0;
		for (auto& q : s->tileQueues) { q.list = nullptr; q.key.clear(); q.costValid = false; }      // every cached list lived in the old slab
		const size_t stride = (std::max(listWords, frameWords) + 4095) & ~(size_t)4095;
		HIPCHK(s->listSlab.reserve(16 * stride));
		s->listStride = stride;
	}
	e->list = s->listSlab + (size_t)(e - s->tileQueues.data()) * s->listStride;
	// the ordered copy, where every tile may be listed in sixteen parts: ONE buffer per scene, shared by the cached lists (the
	// launch that consumes it follows the ordering kernels on the same stream)
	if (16 * std::max(listWords, frameWords) > s->orderedList.capacity()) {
		HIPCHK(hipDeviceSynchronize());
		HIPCHK(s->orderedList.reserve(16 * std::max(listWords, frameWords)));
	}
	return RTX_OK;
}

// The plan goes through a ring of pinned host buffers the kernel reads directly; a slot is taken again eight lists later (its event says whether the
// kernel that read it has run: it has, unless eight views were set without the device getting a turn).  The list that is recycled may still be read
// by an earlier launch: the kernel runs on the stream `st` the CALLER renders on (every render entry point passes its own; prepareView the null stream,
// ordered by prepBegin / prepEnd), behind that launch.
int launchTileList(rtx_scene* s, rtx_scene::TileQueues* e, const TilePlan& pl, uint32_t tilesX, uint32_t tilesY, hipStream_t st)
{
	if (!s->planRing[0].host) {
		// all eight slots in one pinned allocation, on first use (rtx_scene_create: not on the path of a new view), each good for 2 048 tile rows
		const size_t each = 16 + 4 * 2048;
		HIPCHK(s->planRingBase.reserve(8 * each));
		for (int k = 0; k < 8; k++) {
			s->planRing[k].host = s->planRingBase.host() + k * each; s->planRing[k].dev = s->planRingBase.dev() + k * each; s->planRing[k].capWords = each;
			HIPCHK(s->planRing[k].done.create(hipEventDisableTiming));
		}
	}
	rtx_scene::PlanSlot& slot = s->planRing[s->planNext++ & 7u];
	if (slot.used) HIPCHK(hipEventSynchronize(slot.done));
	if (pl.words.size() > slot.capWords) {
		// (its part of the common allocation is simply left behind)
		slot.host = slot.dev = nullptr; slot.capWords = 0;
		const size_t want = std::max<size_t>(pl.words.size(), 16 + 4 * 1100);
		HIPCHK(slot.own.reserve(want));
		slot.host = slot.own.host(); slot.dev = slot.own.dev(); slot.capWords = want;
	}
	HIPCHK(slot.done.create(hipEventDisableTiming));
	memcpy(slot.host, pl.words.data(), pl.words.size() * sizeof(uint32_t));
	const uint32_t cols = std::max(std::max(tilesX, pl.nStrips), 16u);
	hipLaunchKernelGGL(rtxTileListKernel, dim3((cols + 255) / 256, std::max(tilesY, 1u)), dim3(256), 0, st, (const uint32_t*)slot.dev, tilesX, pl.nStrips, pl.in0, pl.in1, pl.sIn0, pl.sIn1, e->list);
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(slot.done, st));
	slot.used = true;
	HIPCHK(e->builtEv.create(hipEventDisableTiming));
	HIPCHK(hipEventRecord(e->builtEv, st));
	e->builtOn = st;
	return RTX_OK;
}

// knob verify_lists: what the device wrote against the host's construction (rtx_frame_plan.h, expectedTileList)
int verifyTileList(rtx_scene* s, const rtx_scene::TileQueues* e, const TilePlan& pl, uint32_t tilesX, uint32_t tilesY, const uint32_t rect[4], hipStream_t st)
{
	const std::vector<uint32_t> want = rtxplan::expectedTileList(s->params.view.width, tilesX, tilesY, rect, pl);
	std::vector<uint32_t> got(pl.listWords);
	HIPCHK(hipStreamSynchronize(st));
	HIPCHK(hipMemcpy(got.data(), e->list, pl.listWords * sizeof(uint32_t), hipMemcpyDeviceToHost));
	if (want != got) return fail(RTX_ERR_DEVICE, "buildTileList: the list written on the device differs from the host's construction");
	return RTX_OK;
}

// The eight per-XCD queues of one pass-1 launch.  Only tiles with a row this launch renders are listed.
// strips (the three-launch path): a tile row of which this launch renders a single pixel row -- the halo row of a band
// that belongs to another device -- is listed as 64 x 1 pixel strips (0x10000000 | strip << 16 | y) instead of 8 x 8
// tiles with one live row each: a wave's time goes into walking its bundle whatever the number of live lanes, and the
// halo rows are a quarter of the tile rows of a 64-row band.
int buildTileList(rtx_scene* s, uint32_t rowBegin, uint32_t lastRow, uint32_t tilesX, uint32_t tileRow0, uint32_t tilesY, rtx_scene::TileQueues** out, bool strips, hipStream_t st)
{
	const Params& p = s->params;
	if (!stripsFit(p.view.width, p.view.height)) strips = false;
	std::vector<uint32_t> key;
	tileListKey(p, rowBegin, lastRow, tilesX, strips, key);
	int rc = findTileList(s, key, st, out);
	if (rc || *out) return rc;
	rtx_scene::TileQueues* e = recycleTileList(s);
	uint32_t rect[4];
	meshTileRect(s, tilesX, (p.view.height + 7) / 8, rect);
	const TilePlan plan = rtxplan::planTileList(p.view.width, { p.bandH, p.nParts, p.part, p.halo }, rowBegin, lastRow, tilesX, tileRow0, tilesY, strips, rect);
	if ((rc = ensureListSlabs(s, e, plan.listWords))) return rc;
	if ((rc = launchTileList(s, e, plan, tilesX, tilesY, st))) return rc;
	if (s->verifyLists && (rc = verifyTileList(s, e, plan, tilesX, tilesY, rect, st))) return rc;
	e->listed = (uint32_t)(plan.listWords - 16);
	e->needValid = false;      // (computed on the device when the single launch first uses this list: renderFrameFused)
	e->key = key;
	e->lastUse = ++s->tileUse;
	*out = e;
	return RTX_OK;
}

// Buffers of the single-launch frame (renderFrameFused): dependency counters, flags, the 64 SSAA item queues, the control block.
int ensureFrameBuffers(rtx_scene* s, size_t tiles, size_t* perQueueOut)
{
	// (the three grow together; each keeps its own capacity, so a call that fails half-way leaves nothing behind that a later one would not see)
	if (tiles > s->tileClass.capacity() || 4 * tiles > s->tileDeps.capacity() || tiles > s->tileFlags.capacity()) {
		HIPCHK(hipDeviceSynchronize());
		HIPCHK(s->tileClass.reserve(tiles));
		HIPCHK(s->tileDeps.reserve(4 * tiles));      // pass-1 count, Sobel count, quarter costs, quarter count
		HIPCHK(s->tileFlags.reserve(tiles));
	}
	// 64 queues; in all up to 4 items per tile (16 flagged pixels each) plus the budget of extra items for tiles that get
	// 4-pixel items.  The items are dealt round the queues, so each holds about 1/64 of them: twice that, and some.
	const size_t perQueue = s->knobs.frameQueueCap ? s->knobs.frameQueueCap : 2 * ((4 * tiles + kSsaaSpreadSlots / 16) / 64) + 256;
	if (tiles >= (1u << 24)) return fail(RTX_ERR_ARG, "frame too large for rtx_render_frame");
	if (64 * perQueue != s->ssaaQueue.capacity()) {      // (exactly the size the kernel is told: a smaller frame shrinks it)
		HIPCHK(hipDeviceSynchronize());
		s->ssaaQueue.reset();
		HIPCHK(s->ssaaQueue.reserve(64 * perQueue));
		HIPCHK(hipMemset(s->ssaaQueue, 0, 64 * perQueue * sizeof(unsigned long long)));
	}
	if (!s->frameCtl) {
		HIPCHK(s->frameCtl.reserve(kFrameCtlBytes / sizeof(unsigned long long)));
		HIPCHK(hipMemset(s->frameCtl, 0, kFrameCtlBytes));      // (rtxFrameClearKernel keeps an error word it finds)
	}
	*perQueueOut = perQueue;
	return RTX_OK;
}

// Everything a first frame would otherwise do on the host before its first launch, done when the scene is created / the view
// set (scene loading: outside the reference's "Render scene" timer as well): the cost estimate, the tile lists of the whole
// frame for either way of rendering it, the buffers of the single launch.
int prepareView(rtx_scene* s)
{
	int rc = buildSources(s);
	if (rc) return rc;
	if ((rc = estimateCosts(s))) return rc;
	const View& v = s->params.view;
	if (v.width > 0xffffu || v.height > 0xffffu || s->params.bandH) return RTX_OK;
	const TileGrid g(v.width, v.height, 0, v.height);
	if (g.noRenderedRow()) return RTX_OK;
	rtx_scene::TileQueues* tq = nullptr;
	if ((rc = buildTileList(s, 0, g.lastRow, g.tilesX, 0, g.tilesY, &tq, true, nullptr))) return rc;
	// the list and the buffers of the single launch: only where rtx_render_frame may take it (frames of more tiles render in three launches by rule)
	const uint32_t ruleTiles = s->analytic ? s->knobs.frameRuleTilesAnalytic : s->knobs.frameRuleTiles;
	if (tq->listed > ruleTiles && s->knobs.frameMode != 1 && s->frameModeForced != 1) return RTX_OK;
	if ((rc = buildTileList(s, 0, g.lastRow, g.tilesX, 0, g.tilesY, &tq, false, nullptr))) return rc;
	const size_t tiles = (size_t)g.tilesXFull * g.tilesYFull;
	size_t perQueue = 0;
	if (tiles < (1u << 24) && (rc = ensureFrameBuffers(s, tiles, &perQueue))) return rc;
	return RTX_OK;
}

} // namespace


namespace {

// RTX_FLAG_SHOW_NORMALS: the view's pass 1 / 4-sample pass through rtxNormalsKernel.  Plain grids over the pixels: the tile lists, the
// tile costs and the frame-mode measurements of the ordinary frames are neither used nor touched.
bool showNormals(const rtx_scene* s) { return (s->params.view.flags & RTX_FLAG_SHOW_NORMALS) != 0; }

// The plain grid over the 8x8 tiles of pass 1's pixels in the rows [rowBegin, rowEnd) (clamped to the view), one wave per tile: p's TileGrid;
// the launch takes (nTiles + 3) / 4 blocks.  Neither the tile lists nor the tile costs are read or written.
// false: the call ends here with rc -- no such pixel (RTX_OK), or a frame too large.
bool plainTileGrid(const rtx_scene* s, uint32_t rowBegin, uint32_t rowEnd, Params& p, int& rc)
{
	const TileGrid g(s->params.view.width, s->params.view.height, rowBegin, rowEnd);
	rc = RTX_OK;
	if (g.noRows() || g.noRenderedRow()) return false;
	if (g.nTiles >= (1u << 30)) { rc = fail(RTX_ERR_ARG, "frame too large"); return false; }
	g.writeTo(p);
	return true;
}

int normalsPass1(rtx_scene* s, uint32_t rowBegin, uint32_t rowEnd, float* fb_dev, hipStream_t st)
{
	if (s->stats) return fail(RTX_ERR_UNSUPPORTED, "the debug views collect no statistics (rtx_counters_enable)");
	Params p = s->params;
	p.fb = fb_dev;
	int rc;
	if (!plainTileGrid(s, rowBegin, rowEnd, p, rc)) return rc;
	if ((rc = stamp(s, 0, st))) return rc;
	hipLaunchKernelGGL(rtxNormalsKernel, dim3((p.nTiles + 3) / 4), dim3(256), 0, st, p, 0);
	HIPCHK(hipGetLastError());
	return stamp(s, 0, st);
}

int normalsSsaa(rtx_scene* s, const uint8_t* mask_dev, uint32_t rowBegin, uint32_t rowEnd, float* fb_dev, hipStream_t st)
{
	if (s->stats) return fail(RTX_ERR_UNSUPPORTED, "the debug views collect no statistics (rtx_counters_enable)");
	const uint32_t W = s->params.view.width;
	Params p = s->params;
	p.fb = fb_dev;
	p.ssaaMask = mask_dev;
	p.rowBegin = rowBegin; p.rowEnd = rowEnd;      // (clamped by rtx_render_ssaa's TileGrid)
	const size_t waves = ((size_t)(rowEnd - rowBegin) * W + 15) / 16;
	if (waves >= (1ull << 32)) return fail(RTX_ERR_ARG, "frame too large");
	int rc = stamp(s, 2, st);
	if (rc) return rc;
	hipLaunchKernelGGL(rtxNormalsKernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, p, 1);
	HIPCHK(hipGetLastError());
	return stamp(s, 2, st);
}

// The tile list of the next launch in the order of rtxTileOrderKernel, into s->orderedList: the count of the cost classes (only where the queues
// are long), then the placement.  What differs between the callers: pass 1 orders its strips and has the queue heads zeroed, the single
// launch splits slow tiles (classes, cost sum, waves, limits); the defaults are the kernel's.
struct TileOrderArgs {
	const uint8_t* classes = nullptr; const unsigned long long* costSum = nullptr; uint32_t nWaves = 1, splitPercent = 0, splitFloor = 0; uint32_t* thresholds = nullptr;
	uint32_t tilesX = 0, stripLimit = 0xffffffffu; uint32_t* heads = nullptr; uint32_t stripBit = 0;
};
void orderTiles(rtx_scene* s, const rtx_scene::TileQueues* tq, const TileOrderArgs& a, hipStream_t st)
{
	const unsigned pieces = tq->listed > 16384u ? 32u : 1u;      // (short queues: one block each, one launch)
	if (pieces > 1) hipLaunchKernelGGL(rtxTileOrderKernel<false>, dim3(pieces, 8), dim3(256), 0, st, s->orderWork, tq->list, s->tileCost, s->params.tilesXFull, s->orderedList, a.classes,
	                   a.costSum, a.nWaves, a.splitPercent, a.splitFloor, a.thresholds, a.tilesX, a.stripLimit, (uint32_t*)nullptr, a.stripBit);
	hipLaunchKernelGGL(rtxTileOrderKernel<true>, dim3(pieces, 8), dim3(256), 0, st, s->orderWork, tq->list, s->tileCost, s->params.tilesXFull, s->orderedList, a.classes,
	                   a.costSum, a.nWaves, a.splitPercent, a.splitFloor, a.thresholds, a.tilesX, a.stripLimit, a.heads, a.stripBit);      // (also zeroes the queue heads it is given)
}

// (the open event pair of `which` is dropped with the launch that failed)
void dropOpenStamp(rtx_scene* s, int which) { if (s->evUsed[which] & 1) s->evUsed[which]--; }

} // namespace

int rtx_render_pass1(rtx_scene* s, uint32_t rowBegin, uint32_t rowEnd, float* fb_dev, void* stream)
{
	RoctxRange range("Render scene (rtx_render_pass1)");
	if (!s || !fb_dev) return fail(RTX_ERR_ARG, "scene/fb is NULL");
	const TileGrid g(s->params.view.width, s->params.view.height, rowBegin, rowEnd);
	if (g.noRows()) return RTX_OK;
	int rc = ensureWork(s);
	if (rc) return rc;
	hipStream_t st = (hipStream_t)stream;
	if (int ro = renderOn(s, st)) return ro;
	if (showNormals(s)) return normalsPass1(s, rowBegin, g.rowEnd, fb_dev, st);
	if (g.noRenderedRow()) return RTX_OK;
	Params p = s->params;
	p.fb = fb_dev;
	g.writeTo(p);
#if RTX_DBG
	p.pad3 = s->knobs.dbgTile;
#endif
	p.workCounter = s->work + 128;            // eight per-XCD queue heads, 64 bytes apart
	if (p.view.width > 0x7fff8u || p.view.height > 0x7fff8u) return fail(RTX_ERR_ARG, "frame too large");
	rtx_scene::TileQueues* tq = nullptr;
	if ((rc = buildTileList(s, rowBegin, g.lastRow, g.tilesX, g.tileRow0, g.tilesY, &tq, true, st))) return rc;
	p.tileList = tq->list;
	p.stripBit = stripsFit(p.view.width, p.view.height) ? 0x10000000u : 0u;
	if (tq->costValid || s->costsUsable) {
		// the previous launch rendered exactly these tiles from this view (or their costs are estimated: estimateCosts): start with the expensive ones
		// (a strip of a halo row that took more than 1 ms is listed as its tiles again: rtxTileOrderKernel)
		TileOrderArgs a;
		a.tilesX = g.tilesX; a.stripLimit = s->knobs.stripLimit; a.heads = s->work + 128; a.stripBit = p.stripBit;
		orderTiles(s, tq, a, st);
		p.tileList = s->orderedList;
	}
	else HIPCHK(hipMemsetAsync(s->work + 128, 0, 128 * sizeof(uint32_t), st));
	tq->costValid = true;
	uint32_t blocks = (uint32_t)s->blocksPass1;
	const uint32_t wavesNeeded = (p.nTiles + 3) / 4;
	if (blocks > wavesNeeded) blocks = wavesNeeded ? wavesNeeded : 1;
	if ((rc = stamp(s, 0, st))) return rc;
	hipLaunchKernelGGL(pass1Kernel(variantOf(s)), dim3(blocks), dim3(256), 0, st, p);
	HIPCHK(hipGetLastError());
	if ((rc = stamp(s, 0, st))) return rc;
	return RTX_OK;
}

// The frame in one launch (rtxFrameKernel).
static int renderFrameFused(rtx_scene* s, uint32_t rowBegin, uint32_t rowEnd, float* fb_dev, uint8_t* mask_dev, void* stream, bool costsKnown)
{
	RoctxRange range("one launch (rtxFrameKernel)");
	const uint32_t W = s->params.view.width;
	const TileGrid g(W, s->params.view.height, rowBegin, rowEnd);
	if (g.noRows()) return RTX_OK;
	rowEnd = g.rowEnd;
	int rc = ensureWork(s);
	if (rc) return rc;
	hipStream_t st = (hipStream_t)stream;
	Params p = s->params;
	p.fb = fb_dev;
	p.maskOut = mask_dev;
	g.writeTo(p);
	if (p.view.width > 0xffffu || p.view.height > 0xffffu) return fail(RTX_ERR_ARG, "frame too large");
	// the mask of the rows is defined everywhere: 0 where no tile computes it (rows of other parts, the last row / column)
	const size_t maskBytes = (size_t)(rowEnd - rowBegin) * W;
	const bool maskInClear = maskBytes <= (4u << 20);      // (a small frame: cleared by rtxFrameClearKernel below)
	if (!maskInClear || g.noRenderedRow()) HIPCHK(hipMemsetAsync(mask_dev + (size_t)rowBegin * W, 0, maskBytes, st));
	if (g.noRenderedRow()) return RTX_OK;
	p.tilesYFull = g.tilesYFull;
	p.workCounter = s->work + 128;            // eight per-XCD queue heads, 64 bytes apart
	rtx_scene::TileQueues* tq = nullptr;
	if ((rc = buildTileList(s, rowBegin, g.lastRow, g.tilesX, g.tileRow0, g.tilesY, &tq, false, st))) return rc;
	const size_t tiles = (size_t)p.tilesXFull * p.tilesYFull;
	size_t perQueue = 0;
	if ((rc = ensureFrameBuffers(s, tiles, &perQueue))) return rc;
	if (!tq->needValid) {
		// once per tile list, on the device: the listed tiles around every tile and the expected values of the completion counters
		// (the 16 cached lists share one allocation: per entry `needStride` bytes of neighbour counts, then 66 counters)
		if (tiles > s->needStride) {
			HIPCHK(hipDeviceSynchronize());
			s->needStride = 0;
			for (auto& q : s->tileQueues) { q.need = nullptr; q.countExpect = nullptr; q.needValid = false; }
			const size_t stride = (tiles + 4095) & ~(size_t)4095;
			HIPCHK(s->needSlab.reserve(16 * (stride + 512)));
			s->needStride = stride;
		}
		{
			const size_t idx = (size_t)(tq - s->tileQueues.data());
			tq->need = s->needSlab + idx * (s->needStride + 512);
			tq->countExpect = (uint32_t*)(tq->need + s->needStride);
		}
		HIPCHK(hipMemsetAsync(s->tileClass, 0, tiles, st));      // (scratch here: the marks; the classes are written later)
		HIPCHK(hipMemsetAsync(tq->countExpect, 0, 66 * sizeof(uint32_t), st));
		hipLaunchKernelGGL(rtxTileMarkKernel, dim3(64, 8), dim3(256), 0, st, (const uint32_t*)tq->list, p.tilesXFull, s->tileClass);
		hipLaunchKernelGGL(rtxTileNeedKernel, dim3((unsigned)((tiles + 255) / 256)), dim3(256), 0, st, (const uint8_t*)s->tileClass, p.tilesXFull, p.tilesYFull,
		                   tq->need, tq->countExpect, tq->countExpect + 65);
		HIPCHK(hipGetLastError());
		tq->needValid = true;
	}
	if (++s->epoch == 0) s->epoch = 1;
	p.tileReady = s->tileDeps; p.tileSobel = s->tileDeps + tiles;
	p.tileNeed = tq->need; p.tileFlags = s->tileFlags;
	p.ssaaQueue = s->ssaaQueue; p.frameCtl = s->frameCtl;
	p.listedTiles = tq->listed; p.epoch = s->epoch; p.queueCap = (uint32_t)perQueue;
	p.countExpect = tq->countExpect;
	p.heavyTicks = s->knobs.heavyTicks;
	p.veryBudget = s->knobs.spreadSlots / 16;
	{
		const size_t most = std::max<size_t>(4 * tiles, maskInClear ? maskBytes : 0);
		hipLaunchKernelGGL(rtxFrameClearKernel, dim3((unsigned)std::min<size_t>((most + 255) / 256, 2048)), dim3(256), 0, st, s->work, s->tileDeps, 4 * tiles,
		                   (uint32_t*)s->frameCtl.get(), (uint32_t)(kFrameCtlBytes / 4), (uint32_t)FC_ERROR, maskInClear ? mask_dev + (size_t)rowBegin * W : nullptr, maskInClear ? maskBytes : 0);
	}
	p.tileList = tq->list;
	p.splitLimits = s->work + 18;
	const bool ordered = tq->costValid || costsKnown || s->costsUsable;      // (the costs of this view may come from frames rendered in three launches)
	if (!ordered) HIPCHK(hipMemsetAsync(s->work + 18, 0xff, 2 * sizeof(uint32_t), st));      // no costs yet: nothing is split
	if (ordered) {
		// the previous launch rendered exactly these tiles from this view: start with the ones that were expensive
		hipLaunchKernelGGL(rtxTileClassKernel, dim3((unsigned)((tiles + 255) / 256)), dim3(256), 0, st, s->tileCost, p.tilesXFull, p.tilesYFull, s->tileClass, (unsigned long long*)(s->work + 16));
		TileOrderArgs a;
		a.classes = s->tileClass; a.costSum = (const unsigned long long*)(s->work + 16); a.nWaves = (uint32_t)s->blocksFrame * 4u;
		a.splitPercent = s->knobs.splitPercent; a.splitFloor = 2000u;            // floor: 20 us (100 MHz)
		a.thresholds = s->work + 18;
		orderTiles(s, tq, a, st);
		p.tileList = s->orderedList;
	}
	tq->costValid = true;
	uint32_t blocks = (uint32_t)s->blocksFrame;
	const uint32_t wavesNeeded = p.nTiles;       // (blocks: quarters of slow tiles and SSAA items want waves too)
	if (blocks > wavesNeeded) blocks = wavesNeeded ? wavesNeeded : 1;
	if ((rc = stamp(s, 4, st))) return rc;
	hipLaunchKernelGGL(frameKernel(variantOf(s)), dim3(blocks), dim3(256), 0, st, p);
	HIPCHK(hipGetLastError());
	if ((rc = stamp(s, 4, st))) return rc;
	return RTX_OK;
}

// The frame in three launches.  The mask of the rows is defined everywhere, as in the single launch: rtx_sobel leaves the rows
// of other parts alone, so under row ownership they are zeroed first.
static int renderFrameSplit(rtx_scene* s, uint32_t rowBegin, uint32_t rowEnd, float* fb_dev, uint8_t* mask_dev, void* stream)
{
	const uint32_t W = s->params.view.width;
	const TileGrid g(W, s->params.view.height, rowBegin, rowEnd);
	if (g.noRows()) return RTX_OK;
	rowEnd = g.rowEnd;
	if (s->params.bandH) HIPCHK(hipMemsetAsync(mask_dev + (size_t)rowBegin * W, 0, (size_t)(rowEnd - rowBegin) * W, (hipStream_t)stream));
	int rc = rtx_render_pass1(s, rowBegin, rowEnd, fb_dev, stream);
	if (!rc) rc = rtx_sobel(s, fb_dev, rowBegin, rowEnd, mask_dev, stream);
	if (!rc) rc = rtx_render_ssaa(s, mask_dev, rowBegin, rowEnd, fb_dev, stream);
	return rc;
}

// finished frames: take their durations
static void collectFrameProbes(rtx_scene* s)
{
	for (auto& pr : s->probes) {
		if (!pr.pending || hipEventQuery(pr.b) != hipSuccess) continue;
		pr.pending = false;
		float ms = 0;
		if (hipEventElapsedTime(&ms, pr.a, pr.b) != hipSuccess) continue;
		if (pr.queue < s->tileQueues.size() && s->tileQueues[pr.queue].generation == pr.generation && pr.mode >= 0)
		{
			// (the best of the samples: the first frame of either way carries one-off work -- buffers, the first ordered list)
			rtx_scene::TileQueues& q = s->tileQueues[pr.queue];
			// a re-probe REPLACES what was known (a view's costs shift during a sequence: an old loss must not pin the choice for ever)
			q.frameMs[pr.mode] = (q.frameSamples[pr.mode] && !pr.refresh) ? std::min(q.frameMs[pr.mode], ms) : ms;
			q.frameSamples[pr.mode]++;
		}
	}
	(void)hipGetLastError();
}

// One launch or three?  The single launch overlaps the stages and splits the slowest tiles -- it wins when the frame is
// bounded by its slowest tiles (small and medium frames, a shard of a large one), by up to 3x; its per-tile bookkeeping
// (a dozen device-scope round trips of ~5 us) loses to three plain launches when the frame is throughput-bound and its
// tiles are cheap.  Which case a view is in is measured, not guessed: the frames are bracketed by events that later
// calls read back without waiting; both ways are tried on warm frames, the faster one is kept and the other one is
// tried again every 64 frames (rtx_frame_plan.h, decideFrameMode).  The pixels are the same either way.
int rtx_render_frame(rtx_scene* s, uint32_t rowBegin, uint32_t rowEnd, float* fb_dev, uint8_t* mask_dev, void* stream)
{
	RoctxRange range("Render scene + MSAA (rtx_render_frame)");
	if (!s || !fb_dev || !mask_dev) return fail(RTX_ERR_ARG, "scene/fb/mask is NULL");
	if (s->stats) return fail(RTX_ERR_UNSUPPORTED, "rtx_render_frame has no instrumented variant: use rtx_render_pass1 / rtx_sobel / rtx_render_ssaa for statistics");
	const TileGrid g(s->params.view.width, s->params.view.height, rowBegin, rowEnd);
	if (g.noRows()) return RTX_OK;
	rowEnd = g.rowEnd;
	int rc = ensureWork(s);
	if (rc) return rc;
	hipStream_t st = (hipStream_t)stream;
	if (int ro = renderOn(s, st)) return ro;
	if (showNormals(s)) {
		// the debug view in three launches, outside the measurements and tile lists of the ordinary frames
		s->lastFused.valid = false;
		if ((rc = stamp(s, 3, st))) return rc;
		if ((rc = renderFrameSplit(s, rowBegin, rowEnd, fb_dev, mask_dev, stream))) { dropOpenStamp(s, 3); return rc; }
		if ((rc = stamp(s, 3, st))) return rc;
		s->lastFrameMode = 0;
		return RTX_OK;
	}
	rtx_scene::TileQueues* tq = nullptr;
	// (the list of the three-launch path: its entry also keeps what was measured for this view)
	if (!g.noRenderedRow() && (rc = buildTileList(s, rowBegin, g.lastRow, g.tilesX, g.tileRow0, g.tilesY, &tq, true, st))) return rc;
	collectFrameProbes(s);
	const int forced = s->frameModeForced >= 0 ? s->frameModeForced : s->knobs.frameMode;
	const uint32_t ruleTiles = s->analytic ? s->knobs.frameRuleTilesAnalytic : s->knobs.frameRuleTiles;
	const bool warm = tq && tq->costValid;
	const uint32_t noSamples[2] = { 0, 0 }; const float noMs[2] = { -1.f, -1.f };      // (no row is rendered: no list, nothing measured)
	const rtxplan::FrameModeChoice c = tq ? rtxplan::decideFrameMode(forced, true, tq->fusedGaveUp, tq->listed, ruleTiles, warm, tq->frameSamples, tq->frameMs, tq->framesSeen)
	                                      : rtxplan::decideFrameMode(forced, false, false, 0u, ruleTiles, false, noSamples, noMs, 0u);
	rtx_scene::FrameProbe* pr = nullptr;
	if (c.probing) {
		pr = &s->probes[s->probeNext++ & 7u];
		HIPCHK(pr->a.create()); HIPCHK(pr->b.create());
		pr->pending = false;
		HIPCHK(hipEventRecord(pr->a, st));
	}
	if ((rc = stamp(s, 3, st))) return rc;
	if (c.mode == 1) {
		rc = renderFrameFused(s, rowBegin, rowEnd, fb_dev, mask_dev, stream, warm);
		// what rtx_frame_status needs to render the frame again should the single launch have given up
		s->lastFused = { true, rowBegin, rowEnd, fb_dev, mask_dev, stream, tq ? (size_t)(tq - s->tileQueues.data()) : ~(size_t)0, tq ? tq->generation : 0u,
		                 s->viewSerial, s->params.bandH, s->params.nParts, s->params.part, s->params.halo };
	}
	else { s->lastFused.valid = false; rc = renderFrameSplit(s, rowBegin, rowEnd, fb_dev, mask_dev, stream); }
	if (rc) { dropOpenStamp(s, 3); return rc; }
	if ((rc = stamp(s, 3, st))) return rc;
	if (pr) {
		HIPCHK(hipEventRecord(pr->b, st));
		// (a cold frame is not a sample: it is slower either way)
		pr->mode = warm ? c.mode : -1; pr->queue = (size_t)(tq - s->tileQueues.data()); pr->generation = tq->generation; pr->pending = true; pr->refresh = c.reprobe;
	}
	if (tq) tq->framesSeen++;
	if (tq) tq->costValid = true;      // (either way the tile costs of this view are now known)
	s->lastFrameMode = c.mode;
	s->lastFrameQueue = tq ? (size_t)(tq - s->tileQueues.data()) : ~(size_t)0;
	return RTX_OK;
}

int rtx_set_knob(rtx_scene* s, const char* name, double value)
{
	if (!s || !name) return fail(RTX_ERR_ARG, "scene/name is NULL");
	Knobs& k = s->knobs;
	const std::string n = name;
	if (n == "strip_limit") k.stripLimit = (uint32_t)value;
	else if (n == "ssaa_heavy_ticks") k.heavyTicks = (uint32_t)value;
	else if (n == "ssaa_spread_slots") k.spreadSlots = (uint32_t)std::min(value, (double)kSsaaSpreadSlots);
	else if (n == "split_percent") k.splitPercent = (uint32_t)value;
	else if (n == "ssaa_local_below") k.localBelow = (long long)value;
	else if (n == "ssaa_sparse_below") k.sparseBelow = (long long)value;
	else if (n == "frame_queue_cap") k.frameQueueCap = (uint32_t)value;
	else if (n == "verify_lists") s->verifyLists = value != 0;
	else if (n == "frame_rule_tiles") k.frameRuleTiles = value >= 4294967295.0 ? 0xffffffffu : (uint32_t)value;
	else if (n == "frame_rule_tiles_analytic") k.frameRuleTilesAnalytic = value >= 4294967295.0 ? 0xffffffffu : (uint32_t)value;
	else if (n == "debug_items") k.debugItems = value != 0;
	else if (n == "trace_reorder") k.traceReorder = value < 0 ? -1 : (value != 0 ? 1 : 0);
	else if (n == "trace_key_origin_first") k.traceOriginFirst = value != 0 ? 1 : 0;
	else if (n == "occluded_scene_order") k.occludedSceneOrder = value != 0 ? 1 : 0;
	else if (n == "prune_boxes") {
		// (taken by the next launch; launches already queued keep the variant they were launched with)
		k.pruneBoxes = value < 0 ? -1 : (value != 0 ? 1 : 0);
		chooseBoxPrune(s);
	}
	else return fail(RTX_ERR_ARG, "unknown knob: " + n);
	return RTX_OK;
}

int rtx_kernel_variant(rtx_scene* s, uint32_t* bits)
{
	if (!s || !bits) return fail(RTX_ERR_ARG, "scene/bits is NULL");
	// the very value the kernel of every family is chosen by at launch (pass1Kernel ... rayOccludedKernel)
	const Variant v = variantOf(s);
	*bits = (v.boxes ? RTX_VARIANT_BOXES : 0u) | (v.plain ? RTX_VARIANT_PLAIN : 0u) | (v.analytic ? RTX_VARIANT_ANALYTIC : 0u) |
	        (v.stats ? RTX_VARIANT_STATS : 0u) | (v.cull ? RTX_VARIANT_CULL : 0u);
	return RTX_OK;
}

int rtx_ssaa_list_read(rtx_scene* s, uint32_t* info, uint32_t* scan, size_t n)
{
	if (!s || !info) return fail(RTX_ERR_ARG, "scene/info is NULL");
	HIPCHK(hipSetDevice(s->device));
	HIPCHK(hipDeviceSynchronize());
	memset(info, 0, 16 * sizeof(uint32_t));
	uint32_t w[20] = { 0 };
	if (s->work) HIPCHK(hipMemcpy(w, s->work, sizeof(w), hipMemcpyDeviceToHost));
	info[0] = w[8]; info[1] = w[9]; info[2] = w[11];      // mode[0] local, mode[1] flagged pixels, mode[3] sparse
	info[3] = s->ssaaListTiles; info[4] = s->params.tilesXFull; info[5] = s->ssaaListHeavy; info[6] = s->ssaaListSpread;
	info[7] = RTX_SSAA_VERY; info[8] = RTX_SSAA_SPREAD_PX;
	info[9] = w[18]; info[10] = w[19]; info[11] = w[16]; info[12] = w[17];      // split limits; the cost sum they were derived from
	info[13] = (uint32_t)s->blocksFrame * 4u;
	if (!scan) return RTX_OK;
	if (!s->ssaaListTiles || !s->items) return fail(RTX_ERR_ARG, "no SSAA list has been built");
	if (n != 2 * (size_t)s->ssaaListTiles + 1) return fail(RTX_ERR_ARG, "n must be 2 tiles + 1 of the last list");
	HIPCHK(hipMemcpy(scan, s->items, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
	return RTX_OK;
}

int rtx_set_frame_mode(rtx_scene* s, int mode)
{
	if (!s || mode < -1 || mode > 1) return fail(RTX_ERR_ARG, "scene is NULL or mode not in -1 (measure), 0 (three launches), 1 (one launch)");
	s->frameModeForced = mode;
	return RTX_OK;
}

int rtx_frame_mode(rtx_scene* s, int* mode, float* split_ms, float* fused_ms)
{
	if (!s || !mode) return fail(RTX_ERR_ARG, "scene/mode is NULL");
	*mode = s->lastFrameMode;
	const rtx_scene::TileQueues* best = s->lastFrameQueue < s->tileQueues.size() && s->tileQueues[s->lastFrameQueue].list ? &s->tileQueues[s->lastFrameQueue] : nullptr;
	if (split_ms) *split_ms = best ? best->frameMs[0] : -1.f;
	if (fused_ms) *fused_ms = best ? best->frameMs[1] : -1.f;
	return RTX_OK;
}

int rtx_frame_status(rtx_scene* s, uint32_t* status)
{
	if (!s || !status) return fail(RTX_ERR_ARG, "scene/status is NULL");
	*status = 0;
	if (!s->frameCtl && !RTX_DBG) return RTX_OK;
	HIPCHK(hipSetDevice(s->device));
	HIPCHK(hipDeviceSynchronize());
#if RTX_DBG
	if (const char* path = getenv("RTX_DBG_TIMELINE")) {      // work items of the frame launches since the last dump: start, duration, kind << 32 | item
		std::vector<unsigned long long> tl(3 * 8192 * 160), keep;
		HIPCHK(hipMemcpyFromSymbol(tl.data(), HIP_SYMBOL(gDbgTimeline), tl.size() * 8));
		for (size_t e = 0; e < tl.size() / 3; e++) if (tl[3 * e]) { keep.push_back(tl[3 * e]); keep.push_back(tl[3 * e + 1]); keep.push_back(tl[3 * e + 2] | (unsigned long long)(e / 160) << 48); }
		std::fill(tl.begin(), tl.end(), 0ull);
		HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(gDbgTimeline), tl.data(), tl.size() * 8));
		if (FILE* f = fopen(path, "wb")) { fwrite(keep.data(), 8, keep.size(), f); fclose(f); }
	}
	if (!s->frameCtl) return RTX_OK;
#endif
	// the error word of the last frame, or the one an earlier frame left since the last call (kept by rtxFrameClearKernel)
	uint32_t err = 0, earlier = 0;
	HIPCHK(hipMemcpy(&err, (const uint32_t*)s->frameCtl.get() + FC_ERROR, sizeof(err), hipMemcpyDeviceToHost));
	HIPCHK(hipMemcpy(&earlier, s->work + 24, sizeof(earlier), hipMemcpyDeviceToHost));
	if (earlier) HIPCHK(hipMemset(s->work + 24, 0, sizeof(uint32_t)));
	const bool lastFrameFailed = err != 0;
	if (!err) err = earlier;
	*status = err;
	if (!err) return RTX_OK;
	// The single launch gave up (1: queue entry never written, 2: work never completed, 3: SSAA queue overflow): its frame is
	// incomplete.  The reference's Scene::render cannot deliver a partial frame (scene.cpp:595-606), so the frame is rendered
	// again here, in three launches, into the same buffers, and the view stays with three launches.  status = the error | 0x100.
	HIPCHK(hipMemset((uint32_t*)s->frameCtl.get() + FC_ERROR, 0, sizeof(uint32_t)));
	const rtx_scene::LastFused lf = s->lastFused;
	s->lastFused.valid = false;
	if (lf.queue < s->tileQueues.size() && s->tileQueues[lf.queue].generation == lf.generation) s->tileQueues[lf.queue].fusedGaveUp = true;
	// Only the LAST frame can be rendered again, and only into what it was rendered with: an error left by an earlier frame, or a
	// view / row ownership that changed since, means a frame the caller may already have consumed is incomplete.
	const Params& pp = s->params;
	if (!lf.valid || !lastFrameFailed || lf.viewSerial != s->viewSerial || lf.bandH != pp.bandH || lf.nParts != pp.nParts || lf.part != pp.part || lf.halo != pp.halo)
		return fail(RTX_ERR_DEVICE, "rtx_render_frame: the frame kernel gave up on a frame that cannot be rendered again (an earlier frame, or the view / row ownership changed since)");
	int rc = renderFrameSplit(s, lf.rowBegin, lf.rowEnd, lf.fb, lf.mask, lf.stream);
	if (rc) return rc;
	HIPCHK(hipStreamSynchronize((hipStream_t)lf.stream));
	s->framesRecovered++;
	*status = err | 0x100u;
	return RTX_OK;
}

int rtx_sobel(rtx_scene* s, const float* fb_dev, uint32_t rowBegin, uint32_t rowEnd, uint8_t* mask_dev, void* stream)
{
	RoctxRange range("Sobel filter (rtx_sobel)");
	if (!s || !fb_dev || !mask_dev) return fail(RTX_ERR_ARG, "scene/fb/mask is NULL");
	const uint32_t W = s->params.view.width, H = s->params.view.height;
	const TileGrid g(W, H, rowBegin, rowEnd);
	if (g.noRows()) return RTX_OK;
	rowEnd = g.rowEnd;
	int rc = ensureWork(s);
	if (rc) return rc;
	hipStream_t st = (hipStream_t)stream;
	if (int ro = renderOn(s, st)) return ro;
	if ((rc = stamp(s, 1, st))) return rc;
	dim3 grid((W + 61) / 62, (rowEnd - rowBegin + 4 * kSobelRows - 1) / (4 * kSobelRows));      // (a wave: 62 columns x kSobelRows rows)
	hipLaunchKernelGGL(rtxSobelKernel, grid, dim3(256), 0, st, fb_dev, mask_dev, W, H, rowBegin, rowEnd,
	                   s->params.bandH, s->params.nParts, s->params.part);
	HIPCHK(hipGetLastError());
	if ((rc = stamp(s, 1, st))) return rc;
	return RTX_OK;
}

// The SSAA launch of frame k may overlap pass 1 of frame k + 1 on another stream (bench.py --pipelined): pass 1 then rewrites
// tileCost while the list is built from it.  Each tile's cost is read once, by rtxSsaaCountKernel; the scatter takes the tile's
// half and layout from the scan, so the list stays consistent and the frame the serial one (tests/test_gpu_overlap.py).  The
// second area of `frames`, the SSAA queue head (work[1]) and the list (items, ssaaPixels) are this stage's own.
int rtx_render_ssaa(rtx_scene* s, const uint8_t* mask_dev, uint32_t rowBegin, uint32_t rowEnd, float* fb_dev, void* stream)
{
	RoctxRange range("MSAA (rtx_render_ssaa)");
	if (!s || !fb_dev || !mask_dev) return fail(RTX_ERR_ARG, "scene/fb/mask is NULL");
	const uint32_t W = s->params.view.width, H = s->params.view.height;
	const TileGrid g(W, H, rowBegin, rowEnd);
	if (g.noRows()) return RTX_OK;
	rowEnd = g.rowEnd;
	int rc = ensureWork(s);
	if (rc) return rc;
	hipStream_t st = (hipStream_t)stream;
	if (int ro = renderOn(s, st)) return ro;
	if (showNormals(s)) return normalsSsaa(s, mask_dev, rowBegin, rowEnd, fb_dev, st);
	// (work[1], the queue head, and work[10], the slot budget used, are zeroed by rtxSsaaScatterKernel; [8], [9]: the layout
	// decision and its count, see below)
	if ((uint32_t)s->tileCap < s->params.tilesXFull * g.tilesYFull || W > 0xffffu || H > 0xffffu) return fail(RTX_ERR_ARG, "frame too large for the SSAA pixel list");
	if ((rc = stamp(s, 2, st))) return rc;
	Params p = s->params;
	p.fb = fb_dev;
	p.workCounter = s->work + 1;
	p.ssaaMask = mask_dev;
	p.rowBegin = rowBegin; p.rowEnd = rowEnd;
	p.nTiles = p.tilesXFull * g.tilesYFull;
	p.ssaaScan = s->items;
	p.frames = s->frames + s->framesArea;
	p.ssaaPixels = s->ssaaPixels;
	// flagged pixels -> one packed list; tiles on which pass 1 spent more than 0.25 ms go first (wall clock = 100 MHz)
	const uint32_t heavyTicks = s->knobs.heavyTicks, spreadSlots = s->knobs.spreadSlots;
	const uint32_t scanN = 2 * p.nTiles + 1;
	// tile-local waves (see rtxSsaaCountKernel) below eight full rounds of waves' worth of flagged pixels -- measured:
	// 250k scene 4096^2 (88 k flagged) 1.00 against 1.54 ms packed, 8192^2 (350 k) 1.29 against 1.75; the glass-and-
	// mirror scene at 1080p (746 k flagged, no slow tiles) 0.82 against 0.68 packed
	uint32_t localBelow = (uint32_t)s->blocksSsaa * 4u * 16u * 8u;      // (about 650 000 flagged pixels)
	if (s->knobs.localBelow >= 0) localBelow = (uint32_t)std::min<long long>(s->knobs.localBelow, 0xffffffffll);   // test knob: 0 = always packed
	uint32_t* mode = s->work + 8;             // [0] local mode, [1] flagged pixels, [2] extra slots handed to 4-pixel tiles
	uint32_t launches = 0;
	// The layout (tile-local or packed) follows from the number of flagged pixels: a count, a scan and a copy before the
	// real count.  It only changes when the view does, so it is decided on the first frame of a view (and again every 16th)
	// and kept in between -- five small launches less per frame.
	const uint64_t key = (((((((uint64_t)s->viewSerial * 0x9e3779b97f4a7c15ull + W) * 31 + H) * 31 + rowBegin) * 31 + rowEnd) * 31 + p.bandH * 64 + p.nParts * 8 + p.part) * 31 + localBelow) * 31 + (uint64_t)(s->knobs.sparseBelow + 1);
	const bool decideNow = key != s->ssaaLayoutKey || (s->ssaaLayoutAge++ & 15u) == 15u;
	if (decideNow) {
		hipLaunchKernelGGL(rtxSsaaCountKernel, dim3((scanN + 255) / 256), dim3(256), 0, st, p, s->items, mode, heavyTicks, 0u, 0u, 0u);
		if ((rc = scanExclusive(s->items, scanN, s->items + scanN, st, launches))) return rc;
		HIPCHK(hipMemcpyAsync(mode + 1, s->items + 2 * (size_t)p.nTiles, sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
		s->ssaaLayoutKey = key; s->ssaaLayoutAge = 0;
	}
	// "sparse" (rtxSsaaCountKernel): fewer 16-pixel items than half the waves of the launch
	uint32_t sparseBelow = (uint32_t)s->blocksSsaa * 4u * 16u / 2u;
	if (s->knobs.sparseBelow >= 0) sparseBelow = (uint32_t)std::min<long long>(s->knobs.sparseBelow, 0xffffffffll);
	hipLaunchKernelGGL(rtxSsaaCountKernel, dim3((scanN + 255) / 256), dim3(256), 0, st, p, s->items, mode, heavyTicks, decideNow ? 1u : 2u, localBelow, spreadSlots, sparseBelow);
	if ((rc = scanExclusive(s->items, scanN, s->items + scanN, st, launches))) return rc;
	hipLaunchKernelGGL(rtxSsaaScatterKernel, dim3((p.nTiles + 255) / 256), dim3(256), 0, st, p, s->items, mode, s->ssaaPixels);
	HIPCHK(hipGetLastError());
	s->ssaaListTiles = p.nTiles; s->ssaaListHeavy = heavyTicks; s->ssaaListSpread = spreadSlots;
	hipLaunchKernelGGL(ssaaKernel(variantOf(s)), dim3(s->blocksSsaa), dim3(256), 0, st, p);
	HIPCHK(hipGetLastError());
	if ((rc = stamp(s, 2, st))) return rc;
	return RTX_OK;
}

int rtx_quantize_bgr8(rtx_scene* s, const float* fb_dev, uint8_t* bgr_dev, void* stream)
{
	if (!s || !fb_dev || !bgr_dev) return fail(RTX_ERR_ARG, "scene/fb/out is NULL");
	const uint32_t W = s->params.view.width, H = s->params.view.height;
	if (W % 4) return fail(RTX_ERR_UNSUPPORTED, "saveImage is only defined for width % 4 == 0 (util.cpp:28-29)");
	HIPCHK(hipSetDevice(s->device));
	if (((uintptr_t)fb_dev & 15u) || ((uintptr_t)bgr_dev & 3u)) return fail(RTX_ERR_ARG, "rtx_quantize_bgr8: fb must be 16-byte aligned, the image 4-byte aligned");
	const size_t n = (size_t)(W / 4) * H;
	if (int ro = renderOn(s, (hipStream_t)stream)) return ro;
	hipLaunchKernelGGL(rtxQuantizeKernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, fb_dev, bgr_dev, W, H,
	                   s->params.bandH, s->params.nParts, s->params.part);
	HIPCHK(hipGetLastError());
	return RTX_OK;
}

int rtx_render_frame_host(rtx_scene* s, int with_ssaa, float* fb_host)
{
	if (!s || !fb_host) return fail(RTX_ERR_ARG, "scene/fb is NULL");
	HIPCHK(hipSetDevice(s->device));
	const uint32_t W = s->params.view.width, H = s->params.view.height;
	const size_t bytes = (size_t)W * H * 3 * sizeof(float);
	DevArray<float> fb; DevArray<uint8_t> mask;
	HIPCHK(fb.reserve((size_t)W * H * 3));
	HIPCHK(hipMemset(fb, 0, bytes));                 // new Vec3f[H*W] is zero-initialised (scene.cpp:599)
	int rc = rtx_render_pass1(s, 0, H, fb, nullptr);
	if (rc) return rc;
	if (with_ssaa) {
		HIPCHK(mask.reserve((size_t)W * H));
		if ((rc = rtx_sobel(s, fb, 0, H, mask, nullptr))) return rc;
		if ((rc = rtx_render_ssaa(s, mask, 0, H, fb, nullptr))) return rc;
	}
	HIPCHK(hipMemcpy(fb_host, fb, bytes, hipMemcpyDeviceToHost));
	return RTX_OK;
}

int rtx_render_ac(rtx_scene* s, float* fb_dev, uint32_t* counts_dev, void* stream)
{
	RoctxRange range("Render AC heat map (rtx_render_ac)");
	if (!s || !fb_dev) return fail(RTX_ERR_ARG, "scene/fb is NULL");
	if (s->params.bandH != 0 && s->params.nParts > 1) return fail(RTX_ERR_ARG, "rtx_render_ac: the heat map is normalised by the maximum of the whole frame -- not under row ownership with more than one part");
	if (s->stats) return fail(RTX_ERR_ARG, "rtx_render_ac: the debug views collect no statistics (rtx_counters_enable)");
	int rc = ensureWork(s);
	if (rc) return rc;
	const uint32_t W = s->params.view.width, H = s->params.view.height;
	const size_t px = (size_t)W * H;
	const size_t waves = (size_t)((W + 7) / 8) * ((H + 7) / 8);
	if (waves >= (1ull << 32)) return fail(RTX_ERR_ARG, "frame too large");
	HIPCHK(s->acMax.reserve(1));
	uint32_t* counts = counts_dev;
	if (!counts) {
		if (s->acCounts.capacity() < px) {
			HIPCHK(hipDeviceSynchronize());
			HIPCHK(s->acCounts.reserve(px));
		}
		counts = s->acCounts;
	}
	hipStream_t st = (hipStream_t)stream;
	if (int ro = renderOn(s, st)) return ro;
	HIPCHK(hipMemsetAsync(s->acMax, 0, sizeof(uint32_t), st));
	hipLaunchKernelGGL(rtxAcCountKernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, s->params, counts, s->acMax);
	HIPCHK(hipGetLastError());
	hipLaunchKernelGGL(rtxAcNormalizeKernel, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, st, (const uint32_t*)counts, (const uint32_t*)s->acMax, fb_dev, px);
	HIPCHK(hipGetLastError());
	return RTX_OK;
}

int rtx_counters_enable(rtx_scene* s, int enable)
{
	if (!s) return fail(RTX_ERR_ARG, "scene is NULL");
	s->stats = enable != 0;
	return RTX_OK;
}

int rtx_counters_reset(rtx_scene* s)
{
	if (!s) return fail(RTX_ERR_ARG, "scene is NULL");
	int rc = ensureWork(s);
	if (rc) return rc;
	HIPCHK(hipDeviceSynchronize());
	HIPCHK(hipMemset(s->counters, 0, 16 * sizeof(unsigned long long)));
	return RTX_OK;
}

int rtx_counters_read(rtx_scene* s, rtx_counters* out)
{
	if (!s || !out) return fail(RTX_ERR_ARG, "scene/out is NULL");
	int rc = ensureWork(s);
	if (rc) return rc;
	HIPCHK(hipDeviceSynchronize());
	unsigned long long c[16];
	HIPCHK(hipMemcpy(c, s->counters, sizeof(c), hipMemcpyDeviceToHost));
	out->rays = c[0]; out->box_tests = c[1]; out->tri_tests = c[2]; out->moot_rays = c[15];
	if (s->knobs.debugItems) fprintf(stderr, "[rtx] slowest work item %.3f ms, sum of items %.3f ms (100 MHz wall clock)\n", c[3] * 1e-5, c[4] * 1e-5);
	if (s->knobs.debugItems) fprintf(stderr, "[rtx] wave-level: node visits %llu, reached leaves %llu, filter passes (64 references) %llu, of which rejected whole by stage 1 %llu, by stage 2 %llu; survivors tested exactly %llu; slots pruned by their records %llu, per-ray slot tests %llu, evaluations of prune records %llu\n", c[5], c[10], c[12], c[13], c[7], c[6], c[11], c[8], c[9]);
#if RTX_DBG || RTX_WAVE_TRACE
	if (s->knobs.debugItems) {
		std::vector<unsigned long long> w(3 * 16384);
		HIPCHK(hipMemcpyFromSymbol(w.data(), HIP_SYMBOL(gDbgWave), w.size() * 8));
		unsigned long long t0 = ~0ull, t1 = 0; double busy = 0; int n = 0;
		for (int i = 0; i < 16384; i++) if (w[3 * i]) { t0 = std::min(t0, w[3 * i]); t1 = std::max(t1, w[3 * i + 1]); busy += (double)w[3 * i + 2]; n++; }
		if (n) {
			int hist[10] = { 0 }; double idleEnd = 0, idleStart = 0;
			for (int i = 0; i < 16384; i++) if (w[3 * i]) { int b = (int)(10.0 * (double)(w[3 * i + 1] - t0) / (double)(t1 - t0 + 1)); hist[b < 0 ? 0 : b > 9 ? 9 : b]++; idleEnd += (double)(t1 - w[3 * i + 1]); idleStart += (double)(w[3 * i] - t0); }
			fprintf(stderr, "[rtx] pass-1 waves %d: span %.3f ms, mean busy %.3f ms, mean idle before first tile %.3f ms, after last tile %.3f ms; waves ending in each tenth of the span:", n, (t1 - t0) * 1e-5, busy / n * 1e-5, idleStart / n * 1e-5, idleEnd / n * 1e-5);
			for (int b = 0; b < 10; b++) fprintf(stderr, " %d", hist[b]);
			fprintf(stderr, "\n");
			// the end of the launch in twentieths of a millisecond before its last wave's last tile: how many waves are still busy
			fprintf(stderr, "[rtx] waves still rendering x ms before the end:");
			for (int k = 12; k >= 0; k--) { int m = 0; const double at = (double)t1 - k * 5000.0; for (int i = 0; i < 16384; i++) if (w[3 * i] && (double)w[3 * i + 1] > at) m++; fprintf(stderr, " %.2f:%d", k * 0.05, m); }
			fprintf(stderr, "\n");
		}
	}
#endif
#if RTX_DBG
	if (s->knobs.debugItems) {
		unsigned long long h[64];
		HIPCHK(hipMemcpyFromSymbol(h, HIP_SYMBOL(gDbgHist), sizeof(h)));
		{ unsigned long long z[8] = {}; HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(gDbgHist), z, sizeof(z), 8 * sizeof(unsigned long long))); }
		static const char* names[10] = { "depth limit sky", "next light", "lights done: mirror", "lights done: transparent", "return: mirror", "return: transparent 1", "return: transparent 2", "consume: miss", "consume: shade", "consume: shadow" };
		for (int k = 0; k < 10; k++) if (h[17 + 2 * k]) fprintf(stderr, "[rtx]   %-26s %8llu wave-level executions, %7.0f cycles each\n", names[k], h[17 + 2 * k], (double)h[16 + 2 * k] / (double)h[17 + 2 * k]);
		{ unsigned long long z[32] = {}; HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(gDbgHist), z, sizeof(z), 16 * sizeof(unsigned long long))); }
		if (h[32] + h[33] + h[34]) fprintf(stderr, "[rtx] walk cycles (waves whose walk ended early inside the reference passes are not counted for that batch): nodes %llu, reference passes without the exact tests %llu, exact tests %llu\n", h[32], h[33], h[34]);
		{ unsigned long long z[3] = {}; HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(gDbgHist), z, sizeof(z), 32 * sizeof(unsigned long long))); }
		if (h[40]) fprintf(stderr, "[rtx] wide walks %llu, of shadow bundles %llu: their node visits %llu, leaves %llu, filter passes %llu, exact tests %llu (these six: since the last print)\n", h[40], h[41], h[42], h[43], h[44], h[45]);
		{ unsigned long long z[6] = {}; HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(gDbgHist), z, sizeof(z), 40 * sizeof(unsigned long long))); }
		if (h[15]) fprintf(stderr, "[rtx] work items %llu: slowest = %llu trace rounds, %llu cycles in Render::trace + %llu in the castRay state machine; "
		                   "all items: %llu rounds, %.0f + %.0f cycles per round\n", h[15], h[9], h[10], h[11], h[12], (double)h[13] / (double)h[12], (double)h[14] / (double)h[12]);
	}
#endif
#if RTX_DBG >= 2
	if (s->knobs.debugItems) {
		unsigned long long h[64];
		HIPCHK(hipMemcpyFromSymbol(h, HIP_SYMBOL(gDbgHist), sizeof(h)));
		{ unsigned long long z[64] = {}; HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(gDbgHist), z, sizeof(z))); }
		if (h[0]) fprintf(stderr, "[rtx] certificates (one sampled lane per evaluation): %llu, back-facing %.1f%%, facing %.1f%% (behind %.1f%%, miss %.1f%%, neither %.1f%%), uncertain %.1f%%; skipped %.1f%%\n",
		                  h[0], 100.0 * h[1] / h[0], 100.0 * h[2] / h[0], 100.0 * h[4] / h[0], 100.0 * h[5] / h[0], 100.0 * h[6] / h[0], 100.0 * (h[0] - h[1] - h[2]) / h[0], 100.0 * h[7] / h[0]);
		for (int b = 0; b < 12; b++)
			if (h[16 + b]) fprintf(stderr, "[rtx]   leaves of %4d..%4d refs: unskipped wave visits %10llu, chunk headers %10llu, triangle iterations %10llu\n", 1 << b, (2 << b) - 1, h[16 + b], h[32 + b], h[48 + b]);
	}
#endif
	return RTX_OK;
}

int rtx_last_kernel_ms(rtx_scene* s, int which, float* ms)
{
	if (!s || !ms || which < 0 || which > 4) return fail(RTX_ERR_ARG, "bad argument");
	const size_t n = s->evUsed[which];
	if (n < 2) return fail(RTX_ERR_ARG, "no such launch recorded yet");
	HIPCHK(hipSetDevice(s->device));
	HIPCHK(hipEventSynchronize(s->evPool[which][n - 1]));
	HIPCHK(hipEventElapsedTime(ms, s->evPool[which][n - 2], s->evPool[which][n - 1]));
	return RTX_OK;
}

int rtx_kernel_time_reset(rtx_scene* s)
{
	if (!s) return fail(RTX_ERR_ARG, "scene is NULL");
	for (int i = 0; i < 5; i++) s->evUsed[i] = 0;
	s->evCollect = true;
	return RTX_OK;
}

int rtx_kernel_time_stats(rtx_scene* s, int which, uint32_t* launches, double* total_ms)
{
	if (!s || !launches || !total_ms || which < 0 || which > 4) return fail(RTX_ERR_ARG, "bad argument");
	HIPCHK(hipSetDevice(s->device));
	*launches = 0; *total_ms = 0;
	for (size_t i = 0; i + 1 < s->evUsed[which]; i += 2) {
		float ms = 0;
		HIPCHK(hipEventSynchronize(s->evPool[which][i + 1]));
		HIPCHK(hipEventElapsedTime(&ms, s->evPool[which][i], s->evPool[which][i + 1]));
		*total_ms += ms; (*launches)++;
	}
	return RTX_OK;
}

int rtx_scene_bytes(rtx_scene* s, size_t* bytes)
{
	if (!s || !bytes) return fail(RTX_ERR_ARG, "scene/bytes is NULL");
	*bytes = s->owned.bytes() + s->lightsOwned.bytes() + s->recordsOwned.bytes();
	for (const DevBag& m : s->meshOwned) *bytes += m.bytes();
	for (const DevBag& m : s->meshFixed) *bytes += m.bytes();
	return RTX_OK;
}

int rtx_live_device_memory(size_t* allocations, size_t* bytes)
{
	if (allocations) *allocations = rtxown::gLiveAllocations.load();
	if (bytes) *bytes = rtxown::gLiveBytes.load();
	return RTX_OK;
}

int rtx_tile_cost_read(rtx_scene* s, uint32_t* out, size_t n)
{
	if (!s || !out) return fail(RTX_ERR_ARG, "scene/out is NULL");
	HIPCHK(hipSetDevice(s->device));
	const size_t tiles = (size_t)((s->params.view.width + 7) / 8) * ((s->params.view.height + 7) / 8);
	if (n != tiles && n != 2 * tiles) return fail(RTX_ERR_ARG, "n must be ceil(width/8) * ceil(height/8), or twice that");
	if (!s->tileCost || s->tileCap < tiles) return fail(RTX_ERR_ARG, "no pass 1 has run at this size");
	HIPCHK(hipDeviceSynchronize());
	HIPCHK(hipMemcpy(out, s->tileCost, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
	return RTX_OK;
}

int rtx_cost_grid_read(rtx_scene* s, uint32_t* out, size_t n, uint32_t* grid_w, uint32_t* grid_h)
{
	if (!s || !grid_w || !grid_h) return fail(RTX_ERR_ARG, "scene/grid_w/grid_h is NULL");
	const View& v = s->params.view;
	*grid_w = ((v.width + 7) / 8 + 1) / 2; *grid_h = ((v.height + 7) / 8 + 1) / 2;
	if (!out) return RTX_OK;
	if (!s->costsUsable || !s->costGrid) return fail(RTX_ERR_ARG, "no cost estimate for this view");
	const size_t cells = (size_t)*grid_w * *grid_h;
	HIPCHK(hipSetDevice(s->device));
	HIPCHK(hipDeviceSynchronize());
	HIPCHK(hipMemcpy(out, s->costGrid, std::min(n, 2 * cells) * sizeof(uint32_t), hipMemcpyDeviceToHost));
	return RTX_OK;
}

// Host only: P_S of triangles (v0, e1, e2: 9 floats each) for the source S, sigma (rtx_source.hip, sourceP) -- the very function the
// device kernels run, for the CPU tests of the bound.
int rtx_source_p_probe(const float* tris9, uint32_t n, const double* S3, double sigma, int cam, float* out)
{
	if (!tris9 || !S3 || !out) return fail(RTX_ERR_ARG, "rtx_source_p_probe: NULL argument");
	for (uint32_t i = 0; i < n; i++) out[i] = rtxsrc::sourceP(tris9 + (size_t)i * 9, tris9 + (size_t)i * 9 + 3, tris9 + (size_t)i * 9 + 6, S3, sigma, cam != 0);
	return RTX_OK;
}

int rtx_wide_node_slots(void) { return kWideSlots; }

// Host only: the description as ONE canonical byte string -- every scalar and the contents of every array rtx_scene_create would read,
// in declaration order, no pointers, no padding.  Two producers of descriptions (this repo's host, rendering_amd/host/src/scene.cpp flattenScene,
// and the binding a maintainer adds to the reference, oracle/ref_binding.cpp = INTEGRATION.md) are compared through it byte for byte.
int rtx_desc_serialize(const rtx_scene_desc* d, void* out, size_t cap, size_t* need)
{
	if (!d || !need) return fail(RTX_ERR_ARG, "desc/need is NULL");
	size_t at = 0;
	auto put = [&](const void* src, size_t bytes) {
		if (out && src && at + bytes <= cap) memcpy((char*)out + at, src, bytes);
		at += bytes;
	};
	auto put32 = [&](uint32_t v) { put(&v, 4); };
	auto arr = [&](const void* p, size_t n, size_t elem) {      // presence, element count, contents
		put32(p ? 1u : 0u);
		const unsigned long long cnt = p ? n : 0;
		put(&cnt, 8);
		if (p) put(p, n * elem);
	};
	put("RTXD0001", 8);
	static_assert(sizeof(rtx_view) == 4 * 29, "rtx_view has no padding");
	put(&d->view, sizeof(rtx_view));
	put32(d->n_objects);
	static_assert(sizeof(rtx_object) == 4 * 18, "rtx_object has no padding");
	if (d->n_objects && !d->objects) return fail(RTX_ERR_ARG, "objects is NULL");
	put(d->objects, (size_t)d->n_objects * sizeof(rtx_object));
	put32(d->n_meshes);
	if (d->n_meshes && !d->meshes) return fail(RTX_ERR_ARG, "meshes is NULL");
	for (uint32_t i = 0; i < d->n_meshes; i++) {
		const rtx_mesh& m = d->meshes[i];
		put32(m.n_nodes); put32(m.n_refs); put32(m.n_tris);
		arr(m.node_bounds, (size_t)m.n_nodes * 6, 4); arr(m.node_skip, m.n_nodes, 4); arr(m.leaf_begin, m.n_nodes, 4); arr(m.leaf_count, m.n_nodes, 4);
		arr(m.refs, m.n_refs, 4);
		arr(m.tri_pos, (size_t)m.n_tris * 9, 4); arr(m.tri_nrm, (size_t)m.n_tris * 9, 4); arr(m.tri_uv, (size_t)m.n_tris * 6, 4);
		// (tangent / bitangent are read only with a normal map: rtx_scene_create uploads them only then)
		arr(m.normal_map ? m.tri_tb : nullptr, (size_t)m.n_tris * 6, 4);
		put32(m.diffuse_map ? m.diffuse_w : 0u); put32(m.diffuse_map ? m.diffuse_h : 0u); arr(m.diffuse_map, (size_t)m.diffuse_w * m.diffuse_h * 3, 4);
		put32(m.normal_map ? m.normal_w : 0u); put32(m.normal_map ? m.normal_h : 0u); arr(m.normal_map, (size_t)m.normal_w * m.normal_h * 3, 4);
		put32(m.specular_map ? m.specular_w : 0u); put32(m.specular_map ? m.specular_h : 0u); arr(m.specular_map, (size_t)m.specular_w * m.specular_h, 4);
	}
	put32(d->n_lights);
	if (d->n_lights && !d->lights) return fail(RTX_ERR_ARG, "lights is NULL");
	for (uint32_t i = 0; i < d->n_lights; i++) {
		const rtx_light& l = d->lights[i];
		put32((uint32_t)l.type); put(l.color, 12); put(&l.intensity, 4); put(l.dir, 12); put(l.pos, 12);
		arr(l.type == RTX_LIGHT_AREA ? l.points : nullptr, (size_t)l.n_points * 3, 4);
	}
	const bool sky = d->sky_w && d->sky_h && d->sky[0];
	put32(sky ? d->sky_w : 0u); put32(sky ? d->sky_h : 0u);
	for (int k = 0; k < 6; k++) arr(sky ? d->sky[k] : nullptr, (size_t)d->sky_w * d->sky_h * 3, 4);
	*need = at;
	return RTX_OK;
}

int rtx_mesh_flatten_probe(const rtx_mesh* m, uint32_t* n_wide, void* wide_out, void* prune_out, uint32_t cap_wide, float* root_rec8)
{
	if (!m || !n_wide) return fail(RTX_ERR_ARG, "mesh/n_wide is NULL");
	FlatMesh flat;
	int rc = flattenMesh(*m, true, flat);
	if (rc) return rc;
	*n_wide = (uint32_t)flat.wide.size();
	if (root_rec8) memcpy(root_rec8, &flat.rootRec, sizeof(PruneRec));
	if (flat.prune.size() != flat.wide.size() && !flat.wide.empty()) return fail(RTX_ERR_DEVICE, "prune blocks missing");
	const size_t n = std::min<size_t>(cap_wide, flat.wide.size());
	if (wide_out && n) memcpy(wide_out, flat.wide.data(), n * sizeof(WideNode));
	if (prune_out && n) memcpy(prune_out, flat.prune.data(), n * sizeof(PruneBlock));
	return RTX_OK;
}

// Host only: the policy of rtx_render_frame (rtx_frame_plan.h, decideFrameMode) for the CPU tests.
int rtx_frame_mode_probe(int forced, int has_list, int fused_gave_up, uint32_t listed, uint32_t rule_tiles, int warm, const uint32_t* frame_samples2,
                         const float* frame_ms2, uint32_t frames_seen, int* mode, int* reprobe, int* probing)
{
	if (!frame_samples2 || !frame_ms2 || !mode || !reprobe || !probing) return fail(RTX_ERR_ARG, "rtx_frame_mode_probe: NULL argument");
	const rtxplan::FrameModeChoice c = rtxplan::decideFrameMode(forced, has_list != 0, fused_gave_up != 0, listed, rule_tiles, warm != 0, frame_samples2, frame_ms2, frames_seen);
	*mode = c.mode; *reprobe = c.reprobe ? 1 : 0; *probing = c.probing ? 1 : 0;
	return RTX_OK;
}

// Host only: the tile list buildTileList would have the device write (TileGrid, stripsFit, planTileList, expectedTileList) for the CPU tests.
int rtx_tile_list_probe(uint32_t width, uint32_t height, uint32_t band_height, uint32_t n_parts, uint32_t part, int halo, uint32_t rowBegin, uint32_t rowEnd,
                        int strips, const uint32_t* rect4, uint32_t* out, size_t cap, size_t* need)
{
	if (!rect4 || !need) return fail(RTX_ERR_ARG, "rtx_tile_list_probe: rect/need is NULL");
	if (width < 2 || height < 2) return fail(RTX_ERR_ARG, "view: width/height must be >= 2");
	if (band_height != 0 && (n_parts == 0 || part >= n_parts)) return fail(RTX_ERR_ARG, "bad ownership");
	const TileGrid g(width, height, rowBegin, rowEnd);
	// (no rendered row: no tile row, eight empty queues)
	const TilePlan plan = rtxplan::planTileList(width, { band_height, n_parts ? n_parts : 1, part, halo ? 1u : 0u }, rowBegin, g.lastRow, g.tilesX, g.tileRow0, g.tilesY,
	                                            strips != 0 && rtxplan::stripsFit(width, height), rect4);
	const std::vector<uint32_t> list = rtxplan::expectedTileList(width, g.tilesX, g.tilesY, rect4, plan);
	// (the header the device copies from the plan is the construction's)
	if (list.size() != plan.listWords || !std::equal(plan.words.begin(), plan.words.begin() + 16, list.begin()))
		return fail(RTX_ERR_ARG, "rtx_tile_list_probe: the plan's header differs from the host's construction");
	*need = list.size();
	if (out && cap >= list.size()) memcpy(out, list.data(), list.size() * sizeof(uint32_t));
	return RTX_OK;
}

int rtx_set_row_ownership(rtx_scene* s, uint32_t band_height, uint32_t n_parts, uint32_t part, int halo)
{
	if (!s) return fail(RTX_ERR_ARG, "scene is NULL");
	if (band_height != 0 && (n_parts == 0 || part >= n_parts)) return fail(RTX_ERR_ARG, "bad ownership");
	s->params.bandH = band_height; s->params.nParts = n_parts ? n_parts : 1; s->params.part = part; s->params.halo = halo ? 1u : 0u;
	s->lastFused.valid = false;      // (rtx_frame_status renders a failed frame again only under the ownership it was rendered with)
	return RTX_OK;
}

int rtx_cast_rays(rtx_scene* s, uint32_t n, const float* rays, float* hits, float* colours)
{
	if (!s || !rays || !hits || !colours) return fail(RTX_ERR_ARG, "NULL argument");
	if (n == 0) return RTX_OK;
	int rc = ensureWork(s);
	if (rc) return rc;
	DevArray<float> dr, dh, dc;
	HIPCHK(dr.reserve((size_t)n * 6)); HIPCHK(dh.reserve((size_t)n * 8)); HIPCHK(dc.reserve((size_t)n * 3));
	HIPCHK(hipMemcpy(dr, rays, (size_t)n * 24, hipMemcpyHostToDevice));
	HIPCHK(hipMemset(s->work + 3, 0, sizeof(uint32_t)));
	Params p = s->params;
	p.workCounter = s->work + 3;
	p.probeRays = dr; p.probeHits = dh; p.probeColours = dc; p.nProbe = n;
	uint32_t blocks = (uint32_t)s->blocksPass1;
	const uint32_t need = ((n + 63) / 64 + 3) / 4;
	if (blocks > need) blocks = need;
	if (showNormals(s)) hipLaunchKernelGGL(rtxNormalsKernel, dim3(need), dim3(256), 0, nullptr, p, 2);
	else hipLaunchKernelGGL(rtxProbeKernel, dim3(blocks), dim3(256), 0, nullptr, p);
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpy(hits, dh, (size_t)n * 32, hipMemcpyDeviceToHost));
	HIPCHK(hipMemcpy(colours, dc, (size_t)n * 12, hipMemcpyDeviceToHost));
	return RTX_OK;
}

} // extern "C"

// the ray, point and first-hit queries of a loaded scene: their kernel selectors, shared host steps and entry points (uses the scene's internals above)
#include "rtx_query.hip"

// the host half of the view batches (uses the selectors of rtx_query.hip and ensureWork / renderOn above)
#include "rtx_views_api.hip"

// the math probes of include/rtx_debug.h (uses fail / HIPCHK above)
#include "rtx_probes.hip"

// multi-GPU: RCCL communicator + frame gather (uses fail / HIPCHK above)
#include "rtx_comm.hip"

// editing a live scene (include/rtx_scene_edit.h; uses the scene's internals above and the device build of rtx_bvh.hip)
#include "rtx_edit.hip"

// deforming a mesh of a live scene from vertices on the device (include/rtx_deform.h; its kernels come after every other one)
#include "rtx_deform.hip"

// replacing maps and skybox of a live scene from device memory (include/rtx_texture.h; its kernels come last)
#include "rtx_texture.hip"

// texel points of a mesh's UV layout and the margin fill (include/rtx_bake.h; its kernels come last)
#include "rtx_bake.hip"
