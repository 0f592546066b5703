// The scene behind the C ABI's handle: its knobs, everything it owns on the device and remembers between calls, and the variant of its launches.
// Part of rtx_api.hip's translation unit (after the `using` lines there).
#pragma once
#include <array>
#include <cstdint>
#include <memory>
#include <utility>
#include <vector>

#include "rtx_device.h"
#include "rtx_own.h"
#include "rtx_host.h"

// Experiment / test knobs.  Their environment variables are read ONCE, by rtx_scene_create (never on the per-frame path);
// rtx_set_knob changes one of a live scene.
struct Knobs {
	int pass1BlocksPerCU = 0, ssaaBlocksPerCU = 0, frameBlocksPerCU = 0;   // RTX_*_BLOCKS_PER_CU: 0 = what the occupancy allows
	bool prune = true;                   // RTX_NO_PRUNE: no prune records (rtxd::PruneBlock)
	bool sources = true;                 // RTX_NO_SRC: no source copies of the prune records (every walk uses copy 0)
	int pruneBoxes = -1;                 // RTX_PRUNE_BOXES=0|1: the kernels without / with the box test whatever the triangle sizes (-1: by the meshes)
	bool estimate = true;                // RTX_NO_COST_ESTIMATE: no first-frame cost estimate
	bool estimateShadows = true;         // RTX_NO_SHADOW_ESTIMATE / knob estimate_shadows: the leaves' shadows on the planes are not part of it
	float costPerRef = 2.0f, costPerLeaf = 95.0f, costBase = 6100.0f;   // estimate = base + perRef refs + perLeaf leaves (100 MHz ticks per tile; tools/cost_fit.py on the final round-4 kernels: profiles/r04_cost_fit.txt)
	float fatFactor = 3.0f;              // RTX_FAT_FACTOR: bundle width, in mean triangle edges, above which a bundle is split; 0 = never
	uint32_t stripLimit = 100000u;       // RTX_STRIP_LIMIT: a halo strip slower than this (100 MHz ticks) is listed as tiles again
	uint32_t heavyTicks = 18000u;        // RTX_SSAA_HEAVY_TICKS: tiles above go first in the SSAA list (x RTX_SSAA_VERY: 4-pixel waves).  0.25 ms until pass 1 got a quarter faster in round 4: headline SSAA 0.506 (25 000) / 0.475 (20 000) / 0.478 (15 000) / 0.642 (10 000) ms
	uint32_t spreadSlots = 1u << 20;     // RTX_SSAA_SPREAD_SLOTS: slot budget of the 4-pixel SSAA waves
	uint32_t splitPercent = 100;         // RTX_SPLIT_PERCENT: frame kernel, tile split limit in % of the even share; 0 = never
	long long localBelow = -1;           // RTX_SSAA_LOCAL_BELOW: tile-local SSAA list below this many flagged pixels; -1 = by device size
	long long sparseBelow = -1;          // RTX_SSAA_SPARSE_BELOW: one-step-finer SSAA items below this many flagged pixels (rtxSsaaCountKernel); -1 = by device size, 0 = never
	int frameMode = -1;                  // RTX_FRAME_MODE=split|fused
	uint32_t frameRuleTiles = 65536u, frameRuleTilesAnalytic = 8192u;   // knobs frame_rule_tiles / frame_rule_tiles_analytic: frames with more listed tiles take three launches
	                                     // without probing (measured on one MI355X: rtx_render_frame); 0xffffffff = always measure
	uint32_t frameQueueCap = 0;          // RTX_FRAME_QUEUE_CAP: entries per SSAA item queue of the frame kernel; 0 = sized from the frame
	bool debugItems = false;             // RTX_DEBUG_ITEMS: rtx_counters_read prints the wave-level counters
	int traceReorder = -1;               // knob trace_reorder: rtx_trace_rays groups the rays by key always (1), never (0), by their number and coherence (-1)
	int traceOriginFirst = 1;            // knob trace_key_origin_first: the key's interleave starts with the origin's bits (1) or the direction's (0)
	int occludedSceneOrder = 0;          // knob occluded_scene_order: rtx_occluded_rays asks the objects in scene order (1) instead of spheres and planes first (0)
	uint32_t dbgTile = 0;               // RTX_DBG_TILE=tx,ty (RTX_DBG builds): only this tile
};

struct rtx_scene_mesh_deform;      // rtx_deform.hip

struct rtx_scene {
	int device = 0;
	int numCUs = 0;
	Knobs knobs;
	// device allocations that live as long as the scene.  Their counted bytes, with the meshes', are the scene data resident in HBM
	// (rtx_scene_bytes: nodes, leaf references, shading arrays, maps, skybox)
	DevBag owned;
	// the six skybox faces among them (their table is params.sky): what rtx_scene_set_sky replaces and rtx_scene_write_texels writes (rtx_texture.hip)
	const float* skyFaces[6] = { nullptr, nullptr, nullptr, nullptr, nullptr, nullptr };
	// the light records and the area lights' sample points: a bag of their own, replaced as a whole by rtx_scene_set_lights (rtx_edit.hip);
	// the records as uploaded (points: device pointers)
	DevBag lightsOwned;
	std::vector<Light> lightRecs;
	// the records as uploaded, kept for the edits (rtx_scene_set_object, rtx_scene_update_mesh: rtx_edit.hip): per mesh its device record and the
	// allocations of its geometry, normals and tangents (replaced as a whole by rtx_scene_update_mesh); per object its record and its description
	std::vector<Mesh> meshRecs;
	std::vector<DevBag> meshOwned;
	// per mesh what rtx_scene_update_mesh keeps: its uv and maps (freed with the mesh by rtx_scene_set_objects); and the Mesh[] and Object[]
	// arrays behind params.meshes / params.objects with the spheres' entry of meshLeaves, replaced as a whole by rtx_scene_set_objects
	std::vector<DevBag> meshFixed;
	DevBag recordsOwned;
	std::vector<Object> objectRecs;
	std::vector<rtx_object> objectDescs;
	DevArray<float> sphereLeafDev;     // the spheres' entry of meshLeaves once an edit has rebuilt it
	DevArray<char> flatScratch;        // rtx_scene_update_mesh: the device flatten's scratch (rtx_flatten.hip)
	// per mesh what rtx_scene_deform_mesh needs (include/rtx_deform.h): its topology in device memory and the scratch of its kernels; empty until
	// rtx_scene_set_mesh_topology, moved with a kept mesh by rtx_scene_set_objects, not counted in rtx_scene_bytes
	std::vector<std::shared_ptr<rtx_scene_mesh_deform>> meshDeform;
	// per mesh its triangles' positions (n_tris x 9, as given to rtx_scene_create, rtx_scene_update_mesh or rtx_scene_set_objects): the walk reads
	// the leaf references' (v0, e1, e2), from which b and c cannot be had again bit for bit; rtx_texel_points interpolates these (include/rtx_bake.h).
	// Moved with a kept mesh by rtx_scene_set_objects, not counted in rtx_scene_bytes
	std::vector<DevArray<float>> meshTriPos;
	// rtx_texel_points / rtx_dilate_texels: the owner (second copy of tri) of every texel, the large triangles' chunk counts and their scan's scratch.
	// Lazily sized, they only grow
	DevArray<uint32_t> texelOwner; DevArray<unsigned long long> texelChunks; DevArray<char> texelScanTemp;
	float editMs[4] = { 0, 0, 0, 0 };  // the last rtx_scene_update_mesh: build, read-back + flatten + upload, sources + estimate queued, whole call (host wall ms)
	Params params;                // template of the kernel argument block
	bool stats = false;
	bool analytic = true;         // no object is a triangle mesh: the ray kernels without the walk are launched
	bool boxPrune = false;        // some mesh has triangles small enough for the box test of the prune records: the kernels with it are launched
	bool plain = true;            // every object is Diffuse and every light a point / distant light: the mesh kernels without recursion, powf and area-light sums are launched (PLAIN)
	// lazily sized work buffers
	DevArray<float> frames; size_t framesArea = 0;
	DevArray<uint32_t> tileCost, items; size_t tileCap = 0;   // per-tile pass-1 cost, SSAA scan array (2 tiles + 1, then scan scratch), both good for tileCap tiles
	DevArray<uint32_t> ssaaPixels;                            // SSAA flagged-pixel list (<= W * H entries)
	DevArray<uint32_t> work;      // 256 words: [1] SSAA queue head, [3] probe queue head, [8] SSAA list mode, [9] flagged pixels, [128 + 16 q] pass-1 queue head of XCD q
	DevArray<unsigned long long> counters;
	DevArray<uint32_t> orderWork;
	int blocksPass1 = 0, blocksSsaa = 0, blocksFrame = 0;
	// rtx_render_frame: dependency counters (ready, sobel), flags, SSAA item queue, control words
	DevArray<uint32_t> tileDeps; DevArray<unsigned long long> tileFlags; DevArray<uint8_t> tileClass;
	DevArray<unsigned long long> ssaaQueue;
	DevArray<unsigned long long> frameCtl;
	uint32_t epoch = 0;
	// pass-1 tile queues (buildTileList): rebuilt when the view, the row range or the row ownership changes
	std::vector<float> meshBounds;        // 6 floats per mesh: the root box
	struct TileQueues {
		std::vector<uint32_t> key;        // what the list was built for (view, row range, row ownership)
		uint32_t* list = nullptr;         // the queues in geometric order (ordered by cost: rtx_scene::orderedList); this entry's part of listSlab
		uint8_t* need = nullptr; uint32_t listed = 0;      // (need, countExpect: this entry's part of needSlab)
		uint32_t* countExpect = nullptr; bool needValid = false;          // listed tiles by index % 64 (the frame kernel's completion counters)   // rtx_render_frame: listed tiles in each tile's 3x3 neighbourhood
		bool costValid = false;           // tileCost holds the costs of a launch with this key
		uint64_t lastUse = 0;
		// rtx_render_frame: measured duration of the frame in either mode (0: three launches, 1: one launch), -1 = not yet
		float frameMs[2] = { -1.f, -1.f };
		uint32_t frameSamples[2] = { 0, 0 };
		uint32_t framesSeen = 0, generation = 0;
		bool fusedGaveUp = false;         // the single launch once ended with an error for this view: three launches from then on
		hipStream_t builtOn = nullptr; Event builtEv;      // the stream rtxTileListKernel wrote the list on, and its completion
		// the entry is about to hold another list, or its view's geometry has changed: what was measured on it no longer applies
		void forget() { key.clear(); costValid = false; forgetMeasurements(); }
		// ... or the kernel family has changed (rtx_scene_set_lights): only the frame-mode measurements go
		void forgetMeasurements() { frameMs[0] = frameMs[1] = -1.f; frameSamples[0] = frameSamples[1] = 0; framesSeen = 0; generation++; fusedGaveUp = false; }
	};
	// the last frame rendered in one launch (rtx_frame_status renders it again in three if the launch gave up)
	// (only while nothing it depends on has changed: the view and the row ownership it was rendered with are part of it, and
	// rtx_scene_set_view / rtx_set_row_ownership / a later frame in three launches drop it -- ADVICE r3)
	struct LastFused { bool valid = false; uint32_t rowBegin = 0, rowEnd = 0; float* fb = nullptr; uint8_t* mask = nullptr; void* stream = nullptr; size_t queue = ~(size_t)0; uint32_t generation = 0;
	                   uint64_t viewSerial = 0; uint32_t bandH = 0, nParts = 0, part = 0, halo = 0; };
	LastFused lastFused;
	uint32_t framesRecovered = 0;
	// rtx_render_ac: per-pixel counts when the caller passes none, and the frame's maximum
	DevArray<uint32_t> acCounts, acMax;
	// rtx_trace_rays: sort keys (in, out) and the order of up to rayCap rays, the sort's scratch, queue heads + key box (rtxRayInitKernel)
	DevArray<uint32_t> rayKeys, rayOrder; size_t rayCap = 0;      // (rayKeys: 2 rayCap keys, rayOrder: rayCap)
	DevArray<char> raySortTemp;
	DevArray<uint32_t> rayWork;
	// blocks per CU of every ray or point kernel launched so far (blocksPerCU, rtx_query.hip): a handful of entries, keyed by the kernel itself
	std::vector<std::pair<const void*, int>> kernelBlocksPerCU;
	// rtx_render_views (rtx_views.hip): the view table of a batch (records, then the first item of every view) on the device and in the pinned
	// buffer it is copied from -- viewsStaged: that copy, which the next call waits for before it fills the buffer again --, the heads, and
	// with SSAA the view of every item and the list of flagged pixels.  They only grow.
	DevArray<char> viewsTable; PinnedArray<char> viewsStage; Event viewsStaged; bool viewsStagePending = false;
	DevArray<uint32_t> viewsWork, viewsItemView, viewsList;
	// first-frame cost estimate (estimateCosts): the leaf arrays of the meshes, the cell grid, whether tileCost holds usable
	// numbers (estimated or measured) for EVERY tile of the current view
	struct MeshLeaves { const float* boxes; uint32_t n; };      // 8 floats per non-empty leaf: true box lo, hi, reference count, -
	std::vector<MeshLeaves> meshLeaves;
	DevArray<uint32_t> costGrid;
	DevArray<uint8_t> needSlab; size_t needStride = 0;           // rtx_render_frame in one launch: neighbour counts + completion counters of the cached lists
	DevArray<uint32_t> listSlab; size_t listStride = 0;          // the buffers of the 16 cached tile lists: ONE allocation (a hipMalloc per new view cost the host 3 ms)
	DevArray<uint32_t> orderedList;                              // the tile list of the next launch in the order of rtxTileOrderKernel
	bool costsUsable = false;
	// source copies of the prune records (rtxd::PruneRec, rtx_source.hip): per mesh the copies' base, the reference arrays and the
	// slots' reference ranges; the point lights that have a copy; what the copies were last built for
	// (pruneAlloc / pruneWide: the allocation of copy 0 and the source copies, whether or not the copies are used -- rtx_scene_set_lights lays it out again)
	struct SrcMesh { PruneBlock* pruneAlloc = nullptr; uint32_t pruneWide = 0; PruneBlock* base = nullptr; uint32_t nWide = 0, nRefs = 0; const RefA* refA = nullptr; const RefB* refB = nullptr; const RefC* refC = nullptr;
	                 const uint32_t* slotRange = nullptr; float* refP = nullptr; float* blockP = nullptr; float vmax = 0; uint32_t meshIndex = 0; };
	std::vector<SrcMesh> srcMeshes;
	std::vector<std::array<float, 4>> estLights;        // first-frame estimate: point lights (x, y, z, 2) and distant lights (direction, 1)
	std::vector<std::array<float, 6>> estPlanes;        // ... and the planes they cast the meshes' shadows on (position, normal)
	std::vector<std::array<float, 3>> srcLightPos;      // [l]: position of light l (point lights only count below nSrcLights)
	std::vector<uint8_t> srcLightIsPoint;
	float srcNmax = 1.0f;                 // the longest shading normal a shadow ray's origin is offset along (planes keep theirs un-normalised)
	float srcBuiltBias = -1.0f; bool srcLightsBuilt = false;
	std::vector<uint8_t> srcLightFresh;   // after rtx_scene_set_lights, until the next buildSources: [l] != 0 -- light l's copy is still the one built for its position and srcBuiltBias
	float srcBuiltCam[3] = { 0, 0, 0 }; bool srcCamBuilt = false;
	// rtx_render_frame: event pairs around the last few frames, read back (without waiting) by later calls
	// Preparing a view (source copies of the prune records, the cost estimate, the tile lists) is queued on the NULL stream and never waits for the
	// device (ADVICE r3 A5 / VERDICT r4 item 2).  The legacy null stream orders itself against the caller's blocking streams; for a non-blocking render
	// stream the two events below carry the order both ways: the preparation waits for the last render call, the next render call for the preparation.
	hipStream_t lastRenderStream = nullptr; bool rendered = false;
	Event evPrepDone; bool prepRecorded = false; hipStream_t prepSeenBy = nullptr;
	// every distinct non-null stream a render call was made on since the last preparation (pass 1 on A with the quantiser on B, two frames in flight:
	// ADVICE r5): the preparation waits for each of them, and each waits for the preparation (prepSeen)
	struct RenderStream { hipStream_t st = nullptr; Event done; bool active = false, prepSeen = false; };
	std::vector<RenderStream> renderStreams;
	// tile-list plans travel through a ring of pinned host buffers read by rtxTileListKernel (no staging copy, no synchronisation)
	// (a slot is an eighth of planRingBase until a plan outgrows it: from then on it is the slot's own allocation)
	struct PlanSlot { uint32_t* host = nullptr; uint32_t* dev = nullptr; size_t capWords = 0; PinnedArray<uint32_t> own; Event done; bool used = false; };
	PinnedArray<uint32_t> planRingBase;
	PlanSlot planRing[8]; unsigned planNext = 0;
	bool verifyLists = false;             // knob verify_lists: every list built on the device is read back and compared with the host's construction (tests)
	struct FrameProbe { Event a, b; int mode = -1; size_t queue = 0; uint32_t generation = 0; bool pending = false, refresh = false; };
	FrameProbe probes[8];
	unsigned probeNext = 0;
	int lastFrameMode = -1, frameModeForced = -1;
	uint64_t viewSerial = 1, ssaaLayoutKey = 0;      // (the SSAA list layout is decided per view: ssaaStage)
	uint32_t ssaaLayoutAge = 0;
	uint32_t ssaaListTiles = 0, ssaaListHeavy = 0, ssaaListSpread = 0;      // the last rtx_render_ssaa's list: tiles, heavyTicks, spreadSlots (rtx_ssaa_list_read)
	size_t lastFrameQueue = ~(size_t)0;      // the view of the last rtx_render_frame (index into tileQueues)
	std::vector<TileQueues> tileQueues;   // a few entries: a frame may be rendered in several row ranges
	uint64_t tileUse = 0;
	// HIP-event pairs around every launch of {pass 1, sobel, ssaa} since the last rtx_kernel_time_reset
	// By default only the most recent pair is kept (rtx_last_kernel_ms); rtx_kernel_time_reset starts accumulating
	// pairs for rtx_kernel_time_stats, up to kMaxTimedLaunches per kernel (later launches overwrite the last pair).
	std::vector<Event> evPool[5];      // pass 1, sobel, ssaa, whole frame (rtx_render_frame), its single kernel
	size_t evUsed[5] = { 0, 0, 0, 0, 0 };
	bool evCollect = false;
};

namespace {

// The variant of a launch: constants of the scene and the view, so that no kernel carries another's code.  The mesh kernels exist per
// (box test of the prune records, culling mode, PLAIN); scenes without meshes and the instrumented launches have one kernel each.
struct Variant { bool analytic, stats, boxes, cull, plain; };
Variant variantOf(const rtx_scene* s)
{
	return { s->analytic, s->stats, s->boxPrune, (s->params.view.flags & RTX_FLAG_BACKFACE_CULL) != 0, s->plain };
}

} // namespace
