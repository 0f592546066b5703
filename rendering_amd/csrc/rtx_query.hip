// The queries of a loaded scene (include/rtx_query.h, rtx_surface.h, rtx_light.h, rtx_scatter.h, rtx_points.h, rtx_aov.h, rtx_ao.h,
// rtx_render_light.h, rtx_radiance.h, rtx_project.h): which kernel a call launches, the host steps the calls share, and the entry points.  Included by rtx_api.hip after
// its launch bookkeeping (ensureWork, renderOn, plainTileGrid), as rtx_edit.hip is.
#include "rtx_scene.h"      // (Variant, dispatchVariant, fail / HIPCHK)

namespace {

// The kernel of a query family for a variant, the form written once: a scene without meshes has the family's walk-free kernel
// f(false, true, -1, third), a mesh scene f(true, boxes, cull, third).  third: the family's own flag, false for a family without one.
template <typename F> auto selectKernel(const Variant& v, bool third, F&& f)
{
	const std::false_type no; const std::true_type yes; const std::integral_constant<int, -1> none;
	if (v.analytic) return third ? f(no, yes, none, yes) : f(no, yes, none, no);
	return dispatchVariant(v.boxes, v.cull, third, [&](auto b, auto c, auto t) { return f(std::true_type(), b, c, t); });
}
// NAME PARAMS: the selector (PARAMS names the Variant v); THIRD: its third flag; ARGS: the kernels' argument list; then the kernel with
// M, B, C, T -- MESH, BOXES, CULLK and the third flag -- as template arguments.
#define RTX_SELECTOR(NAME, PARAMS, THIRD, ARGS, ...)                                                                          \
typedef void (*NAME##Fn) ARGS;                                                                                                \
NAME##Fn NAME PARAMS                                                                                                          \
{                                                                                                                             \
	return selectKernel(v, THIRD, [](auto m, auto b, auto c, auto t) -> NAME##Fn {                                            \
		[[maybe_unused]] constexpr bool M = decltype(m)::value, B = decltype(b)::value, T = decltype(t)::value;               \
		[[maybe_unused]] constexpr int C = decltype(c)::value;                                                                \
		return __VA_ARGS__;                                                                                                   \
	});                                                                                                                       \
}
RTX_SELECTOR(rayHitKernel, (const Variant& v), false, (const Params, const uint32_t*, float*), rtxRayHitKernel<M, B, C>)
RTX_SELECTOR(raySurfaceKernel, (const Variant& v), false, (const Params, const uint32_t*, const rtx_surface_buffers), rtxRaySurfaceKernel<M, B, C>)
RTX_SELECTOR(rayLightKernel, (const Variant& v), false, (const Params, const uint32_t*, const rtx_light_buffers), rtxRayLightKernel<M, B, C>)
RTX_SELECTOR(rayScatterKernel, (const Variant& v), false, (const Params, const uint32_t*, const rtx_scatter_buffers), rtxRayScatterKernel<M, B, C>)
RTX_SELECTOR(pointLightKernel, (const Variant& v), false, (const Params, const uint32_t*, const float*, const rtx_light_buffers), rtxPointLightKernel<M, B, C>)
RTX_SELECTOR(pointAoKernel, (const Variant& v), false, (const Params, const uint32_t*, const AoArgs), rtxPointAoKernel<M, B, C>)
RTX_SELECTOR(pointProjectKernel, (const Variant& v), false, (const Params, const uint32_t*, const ProjectArgs), rtxPointProjectKernel<M, B, C>)
RTX_SELECTOR(aoKernel, (const Variant& v), false, (const Params, const AoArgs), rtxAoKernel<M, B, C>)
RTX_SELECTOR(lightFrameKernel, (const Variant& v), false, (const Params, const rtx_frame_light_buffers), rtxLightFrameKernel<M, B, C>)
// (PLAIN exists for mesh scenes only: M && T)
RTX_SELECTOR(rayColourKernel, (const Variant& v), v.plain, (const Params, const uint32_t*, float*), rtxRayColourKernel<M, B, C, M && T>)
RTX_SELECTOR(pointRadianceKernel, (const Variant& v), v.plain, (const Params, const uint32_t*, const RadianceArgs), rtxPointRadianceKernel<M, B, C, M && T>)
// rtx_render_views' pass-1 and SSAA kernels: the instances of rtxRayColourKernel
RTX_SELECTOR(viewsPass1Kernel, (const Variant& v), v.plain, (const ViewsKernArgs), rtxViewsPass1Kernel<M, B, C, M && T>)
RTX_SELECTOR(viewsSsaaKernel, (const Variant& v), v.plain, (const ViewsKernArgs), rtxViewsSsaaKernel<M, B, C, M && T>)
// (surface: the normal or the albedo is asked for -- only then is shadePrimary part of the kernel)
RTX_SELECTOR(aovKernel, (const Variant& v, bool surface), surface, (const Params, const rtx_aov_buffers), rtxAovKernel<M, B, C, T>)
// (rtx_render_views_aov: surface -- the normal, the albedo or the hit point is asked for)
RTX_SELECTOR(viewsAovKernel, (const Variant& v, bool surface), surface, (const ViewsAovKernArgs), rtxViewsAovKernel<M, B, C, T>)
#undef RTX_SELECTOR
// (sceneOrder: knob occluded_scene_order -- the objects in scene order instead of spheres and planes first; scenes without meshes have one
// kernel, whose ORDER is true whatever the knob says)
typedef void (*OccludedKernel)(const Params, const uint32_t*, const float*, uint8_t*);
OccludedKernel rayOccludedKernel(const Variant& v, bool sceneOrder)
{
	if (v.analytic) return rtxRayOccludedKernel<false, true, -1, true>;
	return dispatchVariant(v.boxes, v.cull, sceneOrder, [](auto b, auto c, auto ord) -> OccludedKernel { return rtxRayOccludedKernel<true, decltype(b)::value, decltype(c)::value, decltype(ord)::value>; });
}

// Blocks of `kernel` (256 threads) a CU holds at once: asked of the runtime once per kernel and kept by the scene under the kernel's
// address, so that no edit that changes the kernel family has an answer to forget.
int blocksPerCU(rtx_scene* s, const void* kernel, int* perCU)
{
	for (const auto& e : s->kernelBlocksPerCU) if (e.first == kernel) { *perCU = e.second; return RTX_OK; }
	int n = 0;
	if (int rc = askBlocksPerCU(n, kernel)) return rc;
	s->kernelBlocksPerCU.emplace_back(kernel, n);
	*perCU = n;
	return RTX_OK;
}

// A batch of caller-supplied rays on its way to the kernels of rtx_rays.hip (startRays): the argument block of the launches, the rays' order,
// the stream and the number of 64-ray groups.
struct RayCall { Params p; const uint32_t* order; hipStream_t st; uint32_t waves; };

// A launch of persistent waves for such a batch: as many blocks as the device holds of `kernel` at once, at most one wave per group.
template <typename... KArgs, typename... Args>
int launchRays(rtx_scene* s, void (*kernel)(KArgs...), const RayCall& c, Args... args)
{
	int perCU;
	if (int rc = blocksPerCU(s, (const void*)kernel, &perCU)) return rc;
	const uint32_t blocks = std::min<uint32_t>((uint32_t)(perCU * s->numCUs), (c.waves + 3) / 4);
	hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, c.st, c.p, c.order, args...);
	HIPCHK(hipGetLastError());
	return RTX_OK;
}

// Every ray and point query groups its batch by key from this many on, unless the rays already come in coherent groups (rtxRayKeyKernel).
// Measured on one MI355X for rtx_trace_rays (profiles/trace_rays_time.json) and rtx_occluded_rays (profiles/occluded_rays_time.json;
// DESIGN.md 3.8).  rtx_surface_rays' times follow rtx_trace_rays' hits-only times within 0.1 ms at every setting of the knob
// (profiles/surface_time.json); the first half of rtx_light_rays and of rtx_scatter_rays (profiles/
// scatter_time.json) is rtx_surface_rays'; rtx_light_points and rtx_ao_points group {P, N} in the place of origin and
// direction.
constexpr uint32_t kReorderMin = 1u << 20;

// The scratch of rtx_trace_rays for n rays: only a larger n than ever before allocates (the old buffers are freed first -- hipFree waits
// for the device, so no launch of an earlier call still reads them).  (The sort's scratch is asked for every call -- a host computation --
// in case a smaller n ever needed more.)
int ensureRayScratch(rtx_scene* s, uint32_t n, bool reorder, hipStream_t st)
{
	HIPCHK(s->rayWork.reserve(64));
	if (!reorder) return RTX_OK;
	if (n > s->rayCap) {
		s->rayCap = 0;      // (until both are in place)
		HIPCHK(s->rayKeys.reserve(2 * (size_t)n));
		HIPCHK(s->rayOrder.reserve(n));
		s->rayCap = n;
	}
	size_t bytes = 0;
	HIPCHK(rtxSortRayKeys(nullptr, &bytes, s->rayKeys, s->rayKeys + s->rayCap, s->rayOrder, n, kRayKeyBits, st));
	HIPCHK(s->raySortTemp.reserve(bytes));
	return RTX_OK;
}

// The order of n rays grouped by key (rtx_rays.hip: box, key with the coherence check, stable sort), queued on st after rtxRayInitKernel:
// *order = the scene's rayOrder (ensureRayScratch has sized it).
int groupRays(rtx_scene* s, const Params& p, const float* rays_dev, uint32_t n, hipStream_t st, const uint32_t** order)
{
	// the camera's position and axes: the frame of the key's coordinates (rtx_rays.hip, rayCoords)
	const float* M = p.view.camM;
	const RayAxes ax = { { M[0], M[1], M[2], M[4], M[5], M[6], M[8], M[9], M[10] }, { p.view.camPos[0], p.view.camPos[1], p.view.camPos[2] } };
	const uint32_t groups = (uint32_t)(((size_t)n + 255) / 256);
	double* spread = (double*)(s->rayWork + 44);
	hipLaunchKernelGGL(rtxRayBoxKernel, dim3(std::min<uint32_t>(groups, (uint32_t)s->numCUs * 8u)), dim3(256), 0, st, rays_dev, n, ax, s->rayWork + 32, spread);
	// (by default the caller's order is kept where it is already as coherent: rtxRayKeyKernel; trace_reorder = 1 always sorts)
	hipLaunchKernelGGL(rtxRayKeyKernel, dim3(groups), dim3(256), 0, st, rays_dev, n, ax, (const uint32_t*)(s->rayWork + 32), (const double*)spread,
	                   s->knobs.traceOriginFirst, s->knobs.traceReorder < 0 ? 1 : 0, s->rayKeys);
	size_t bytes = s->raySortTemp.capacity();
	HIPCHK(rtxSortRayKeys(s->raySortTemp.get(), &bytes, s->rayKeys, s->rayKeys + s->rayCap, s->rayOrder, n, kRayKeyBits, st));
	*order = s->rayOrder;
	return RTX_OK;
}

// What the ray and point queries do before their own launches: the scene's work buffers, the order against the preparation, the decision
// to group the rays (from kReorderMin rays on, unless the knob trace_reorder says always / never) and, if so, their order.
// p: the argument block of the launches to come.
int beginRays(rtx_scene* s, uint32_t n, const float* rays_dev, hipStream_t st, Params& p, const uint32_t** order)
{
	int rc = ensureWork(s);
	if (rc) return rc;
	if ((rc = renderOn(s, st))) return rc;
	const bool reorder = s->knobs.traceReorder < 0 ? n >= kReorderMin : s->knobs.traceReorder != 0;
	if ((rc = ensureRayScratch(s, n, reorder, st))) return rc;
	p = s->params;
	p.probeRays = rays_dev; p.nProbe = n;
	hipLaunchKernelGGL(rtxRayInitKernel, dim3(1), dim3(64), 0, st, s->rayWork.get());
	*order = nullptr;
	if (reorder && (rc = groupRays(s, p, rays_dev, n, st, order))) return rc;
	return RTX_OK;
}

// The common start of the ray and point queries, after their own checks: the checks of n and rays, then beginRays, which fill c (RayCall;
// its queue head is the first of rayWork).
// false: the call ends here with rc -- no ray (RTX_OK), or an error.
bool startRays(rtx_scene* s, uint32_t n, const float* rays_dev, void* stream, RayCall& c, int& rc)
{
	rc = RTX_OK;
	if (n == 0) return false;
	if (!rays_dev) { rc = fail(RTX_ERR_ARG, "rays is NULL"); return false; }
	if (n > 0xffffffc0u) { rc = fail(RTX_ERR_ARG, "too many rays"); return false; }
	c.st = (hipStream_t)stream;
	c.order = nullptr;
	c.waves = (n + 63) / 64;
	if ((rc = beginRays(s, n, rays_dev, c.st, c.p, &c.order)) != RTX_OK) return false;
	c.p.workCounter = s->rayWork;
	return true;
}

// A frame query on its way to its kernel (startTiles): the argument block with the plain grid over the tiles, and the stream.
struct TileCall { Params p; hipStream_t st; };

// The common start of the frame queries, after their own checks: the plain grid of the normals view over the rows (plainTileGrid), the
// device and the order against the preparation.  No event is recorded (rtx_last_kernel_ms and the frame-mode measurements keep what the
// ordinary frames left).
// false: the call ends here with rc -- no pixel (RTX_OK), or an error.
bool startTiles(rtx_scene* s, uint32_t rowBegin, uint32_t rowEnd, void* stream, TileCall& c, int& rc)
{
	c.p = s->params;
	c.st = (hipStream_t)stream;
	if (!plainTileGrid(s, rowBegin, rowEnd, c.p, rc)) return false;
	rc = [&]() -> int { HIPCHK(hipSetDevice(s->device)); return renderOn(s, c.st); }();
	return rc == RTX_OK;
}

// ... and its launch: one wave per tile
template <typename... KArgs, typename... Args>
int launchTiles(void (*kernel)(KArgs...), const TileCall& c, Args... args)
{
	hipLaunchKernelGGL(kernel, dim3((c.p.nTiles + 3) / 4), dim3(256), 0, c.st, c.p, args...);
	HIPCHK(hipGetLastError());
	return RTX_OK;
}

// What the calls with per-light buffers refuse of them (a per-light buffer sized before rtx_scene_set_lights would be written past its
// end, or with another stride).  who: the call's name.
int checkPerLight(const char* who, const rtx_scene* s, bool perLight, uint32_t nLights)
{
	if (perLight && nLights != s->params.nLights) return fail(RTX_ERR_ARG, std::string(who) + ": n_lights is not the scene's number of lights");
	if (perLight && s->params.nLights == 0) return fail(RTX_ERR_ARG, std::string(who) + ": per-light buffers on a scene without lights");
	return RTX_OK;
}

// ... and the ambient-occlusion calls of their outputs and parameters
int checkAoParams(const char* who, const rtx_ao_params* par, const float* ao, const uint32_t* counts)
{
	if (!ao && !counts) return fail(RTX_ERR_ARG, std::string(who) + ": no output (both buffers are NULL)");
	if (!par->dirs_dev) return fail(RTX_ERR_ARG, std::string(who) + ": dirs_dev is NULL");
	if (par->n_dirs < 1 || par->n_dirs > 256) return fail(RTX_ERR_ARG, std::string(who) + ": n_dirs must be 1 .. 256");
	if (!(par->radius > 0)) return fail(RTX_ERR_ARG, std::string(who) + ": radius must be > 0 (+inf: the whole ray)");
	return RTX_OK;
}

} // namespace

extern "C" {

int rtx_trace_rays(rtx_scene* s, uint32_t n, const float* rays_dev, float* hits_dev, float* colours_dev, void* stream)
{
	RoctxRange range("Trace rays (rtx_trace_rays)");
	if (!s) return fail(RTX_ERR_ARG, "scene is NULL");
	if (!hits_dev && !colours_dev) return fail(RTX_ERR_ARG, "rtx_trace_rays: no output (hits and colours are both NULL)");
	RayCall c;
	int rc;
	if (!startRays(s, n, rays_dev, stream, c, rc)) return rc;
	const Variant v = variantOf(s);
	// (the recursion frames of the pass-1 area hold blocksPass1 blocks: the grid of the kernels that shade)
	const uint32_t blocksShade = std::min<uint32_t>((uint32_t)s->blocksPass1, (c.waves + 3) / 4);
	if (showNormals(s)) hipLaunchKernelGGL(rtxRayNormalsKernel, dim3(blocksShade), dim3(256), 0, c.st, c.p, c.order, hits_dev, colours_dev);
	else {
		if (hits_dev && (rc = launchRays(s, rayHitKernel(v), c, hits_dev))) return rc;
		if (colours_dev) {
			c.p.workCounter = s->rayWork + 16;
			hipLaunchKernelGGL(rayColourKernel(v), dim3(blocksShade), dim3(256), 0, c.st, c.p, c.order, colours_dev);
		}
	}
	HIPCHK(hipGetLastError());
	return RTX_OK;
}

int rtx_occluded_rays(rtx_scene* s, uint32_t n, const float* rays_dev, const float* tmax_dev, uint8_t* occluded_dev, void* stream)
{
	RoctxRange range("Occluded rays (rtx_occluded_rays)");
	if (!s) return fail(RTX_ERR_ARG, "scene is NULL");
	// (this call has always looked at n and rays first: an empty batch needs no output, and "rays is NULL" comes before this message)
	if (n != 0 && rays_dev && !occluded_dev) return fail(RTX_ERR_ARG, "rtx_occluded_rays: no output (occluded is NULL)");
	RayCall c;
	int rc;
	if (!startRays(s, n, rays_dev, stream, c, rc)) return rc;
	return launchRays(s, rayOccludedKernel(variantOf(s), s->knobs.occludedSceneOrder != 0), c, tmax_dev, occluded_dev);
}

int rtx_surface_rays(rtx_scene* s, uint32_t n, const float* rays_dev, const rtx_surface_buffers* out, void* stream)
{
	RoctxRange range("Surface rays (rtx_surface_rays)");
	if (!s || !out) return fail(RTX_ERR_ARG, "scene/out is NULL");
	const bool surface = out->position_dev || out->normal_dev || out->albedo_dev || out->specular_dev;
	if (!out->hits_dev && !surface) return fail(RTX_ERR_ARG, "rtx_surface_rays: no output (all five buffers are NULL)");
	RayCall c;
	int rc;
	if (!startRays(s, n, rays_dev, stream, c, rc)) return rc;
	// the hit records alone: rtx_trace_rays' launch (no surface fetch is compiled into that kernel)
	if (!surface) return launchRays(s, rayHitKernel(variantOf(s)), c, out->hits_dev);
	return launchRays(s, raySurfaceKernel(variantOf(s)), c, *out);
}

int rtx_light_rays(rtx_scene* s, uint32_t n, const float* rays_dev, const rtx_light_buffers* out, void* stream)
{
	RoctxRange range("Light rays (rtx_light_rays)");
	if (!s || !out) return fail(RTX_ERR_ARG, "scene/out is NULL");
	const bool perLight = out->light_diffuse_dev || out->light_specular_dev || out->light_open_dev;
	const bool light = out->diffuse_dev || out->specular_dev || perLight;
	if (!out->hits_dev && !light) return fail(RTX_ERR_ARG, "rtx_light_rays: no output (all six buffers are NULL)");
	int rc = checkPerLight("rtx_light_rays", s, perLight, out->n_lights);
	if (rc) return rc;
	RayCall c;
	if (!startRays(s, n, rays_dev, stream, c, rc)) return rc;
	// the hit records alone: rtx_trace_rays' launch
	if (!light) return launchRays(s, rayHitKernel(variantOf(s)), c, out->hits_dev);
	return launchRays(s, rayLightKernel(variantOf(s)), c, *out);
}

int rtx_scatter_rays(rtx_scene* s, uint32_t n, const float* rays_dev, const rtx_scatter_buffers* out, void* stream)
{
	RoctxRange range("Scatter rays (rtx_scatter_rays)");
	if (!s || !out) return fail(RTX_ERR_ARG, "scene/out is NULL");
	const bool scatter = out->local_dev || out->reflect_dev || out->refract_dev || out->weight_dev || out->kinds_dev;
	if (!out->hits_dev && !scatter) return fail(RTX_ERR_ARG, "rtx_scatter_rays: no output (all six buffers are NULL)");
	RayCall c;
	int rc;
	if (!startRays(s, n, rays_dev, stream, c, rc)) return rc;
	// the hit records alone: rtx_trace_rays' launch
	if (!scatter) return launchRays(s, rayHitKernel(variantOf(s)), c, out->hits_dev);
	return launchRays(s, rayScatterKernel(variantOf(s)), c, *out);
}

// include/rtx_points.h: the batch is {P, N} in the layout of a ray buffer, so startRays' checks and grouping are the rays'
int rtx_light_points(rtx_scene* s, uint32_t n, const float* points_dev, const float* view_dev, const rtx_light_buffers* out, void* stream)
{
	RoctxRange range("Light points (rtx_light_points)");
	if (!s || !out) return fail(RTX_ERR_ARG, "scene/out is NULL");
	if (out->hits_dev) return fail(RTX_ERR_ARG, "rtx_light_points: hits_dev must be NULL (a point has no hit record)");
	const bool perLight = out->light_diffuse_dev || out->light_specular_dev || out->light_open_dev;
	if (!out->diffuse_dev && !out->specular_dev && !perLight) return fail(RTX_ERR_ARG, "rtx_light_points: no output (all five buffers are NULL)");
	if (!view_dev && (out->specular_dev || out->light_specular_dev)) return fail(RTX_ERR_ARG, "rtx_light_points: a specular buffer without view_dev");
	int rc = checkPerLight("rtx_light_points", s, perLight, out->n_lights);
	if (rc) return rc;
	if (n != 0 && !points_dev) return fail(RTX_ERR_ARG, "rtx_light_points: points is NULL");
	RayCall c;
	if (!startRays(s, n, points_dev, stream, c, rc)) return rc;
	return launchRays(s, pointLightKernel(variantOf(s)), c, view_dev, *out);
}

int rtx_ao_points(rtx_scene* s, uint32_t n, const float* points_dev, const rtx_ao_params* par, float* ao, uint32_t* counts, void* stream)
{
	RoctxRange range("Ambient occlusion at points (rtx_ao_points)");
	if (!s || !par) return fail(RTX_ERR_ARG, "scene/params is NULL");
	int rc = checkAoParams("rtx_ao_points", par, ao, counts);
	if (rc) return rc;
	if (n != 0 && !points_dev) return fail(RTX_ERR_ARG, "rtx_ao_points: points is NULL");
	RayCall c;
	if (!startRays(s, n, points_dev, stream, c, rc)) return rc;
	const AoArgs args = { par->dirs_dev, par->n_dirs, par->radius, ao, counts };
	return launchRays(s, pointAoKernel(variantOf(s)), c, args);
}

// include/rtx_project.h: the point queries' steps; the cameras are a table in device memory, used as stored
int rtx_project_points(rtx_scene* s, uint32_t n, const float* points_dev, uint32_t n_cams, const float* cameras_dev, int with_visibility,
                       const rtx_project_buffers* out, void* stream)
{
	RoctxRange range("Project points (rtx_project_points)");
	if (!s || !out) return fail(RTX_ERR_ARG, "scene/out is NULL");
	if (!out->pixel_dev && !out->depth_dev && !out->flags_dev) return fail(RTX_ERR_ARG, "rtx_project_points: no output (all three buffers are NULL)");
	if (!cameras_dev) return fail(RTX_ERR_ARG, "rtx_project_points: cameras_dev is NULL");
	if (n_cams < 1 || n_cams > 256) return fail(RTX_ERR_ARG, "rtx_project_points: n_cams must be 1 .. 256");
	if (n != 0 && !points_dev) return fail(RTX_ERR_ARG, "rtx_project_points: points is NULL");
	RayCall c;
	int rc;
	if (!startRays(s, n, points_dev, stream, c, rc)) return rc;
	const ProjectArgs args = { cameras_dev, n_cams, (with_visibility != 0 && out->flags_dev) ? 1u : 0u, out->pixel_dev, out->depth_dev, out->flags_dev };
	return launchRays(s, pointProjectKernel(variantOf(s)), c, args);
}

// include/rtx_radiance.h: the point queries' steps, and rtx_trace_rays' grid for the kernel that shades
int rtx_radiance_points(rtx_scene* s, uint32_t n, const float* points_dev, const rtx_radiance_params* par, float* sum, uint32_t* counts, void* stream)
{
	RoctxRange range("Radiance at points (rtx_radiance_points)");
	if (!s || !par) return fail(RTX_ERR_ARG, "scene/params is NULL");
	if (!sum && !counts) return fail(RTX_ERR_ARG, "rtx_radiance_points: no output (both buffers are NULL)");
	if (!par->dirs_dev) return fail(RTX_ERR_ARG, "rtx_radiance_points: dirs_dev is NULL");
	if (par->n_dirs < 1 || par->n_dirs > 256) return fail(RTX_ERR_ARG, "rtx_radiance_points: n_dirs must be 1 .. 256");
	if (par->cosine != 0 && par->cosine != 1) return fail(RTX_ERR_ARG, "rtx_radiance_points: cosine must be 0 or 1");
	if (n != 0 && !points_dev) return fail(RTX_ERR_ARG, "rtx_radiance_points: points is NULL");
	if (n > 0xffffffc0u) return fail(RTX_ERR_ARG, "rtx_radiance_points: too many points (n)");
	if (showNormals(s)) return fail(RTX_ERR_UNSUPPORTED, "rtx_radiance_points: RTX_FLAG_SHOW_NORMALS is set (a debug view has no radiance)");
	RayCall c;
	int rc;
	if (!startRays(s, n, points_dev, stream, c, rc)) return rc;
	// (the recursion frames of the pass-1 area hold blocksPass1 blocks: rtx_trace_rays' blocksShade)
	const uint32_t blocksShade = std::min<uint32_t>((uint32_t)s->blocksPass1, (c.waves + 3) / 4);
	const RadianceArgs args = { par->dirs_dev, par->weights_dev, par->n_dirs, par->cosine, sum, counts };
	hipLaunchKernelGGL(pointRadianceKernel(variantOf(s)), dim3(blocksShade), dim3(256), 0, c.st, c.p, c.order, args);
	HIPCHK(hipGetLastError());
	return RTX_OK;
}

int rtx_sky_rays(rtx_scene* s, uint32_t n, const float* rays_dev, float* colours_dev, void* stream)
{
	RoctxRange range("Sky rays (rtx_sky_rays)");
	if (!s) return fail(RTX_ERR_ARG, "scene is NULL");
	if (n == 0) return RTX_OK;
	if (!rays_dev) return fail(RTX_ERR_ARG, "rays is NULL");
	if (!colours_dev) return fail(RTX_ERR_ARG, "rtx_sky_rays: no output (colours is NULL)");
	if (n > 0xffffffc0u) return fail(RTX_ERR_ARG, "too many rays");
	// a plain grid over the rays: no walk, no queue, none of the scene's ray scratch
	const hipStream_t st = (hipStream_t)stream;
	int rc = ensureWork(s);
	if (rc) return rc;
	if ((rc = renderOn(s, st))) return rc;
	Params p = s->params;
	p.probeRays = rays_dev; p.nProbe = n;
	hipLaunchKernelGGL(rtxRaySkyKernel, dim3((uint32_t)(((size_t)n + 255) / 256)), dim3(256), 0, st, p, colours_dev);
	HIPCHK(hipGetLastError());
	return RTX_OK;
}

int rtx_render_aov(rtx_scene* s, uint32_t rowBegin, uint32_t rowEnd, const rtx_aov_buffers* out, void* stream)
{
	RoctxRange range("First-hit buffers (rtx_render_aov)");
	if (!s || !out) return fail(RTX_ERR_ARG, "scene/out is NULL");
	if (!out->depth_dev && !out->object_dev && !out->triangle_dev && !out->uv_dev && !out->normal_dev && !out->albedo_dev)
		return fail(RTX_ERR_ARG, "rtx_render_aov: no output (all six buffers are NULL)");
	if (s->stats) return fail(RTX_ERR_UNSUPPORTED, "rtx_render_aov collects no statistics (rtx_counters_enable)");
	TileCall c;
	int rc;
	if (!startTiles(s, rowBegin, rowEnd, stream, c, rc)) return rc;
	return launchTiles(aovKernel(variantOf(s), out->normal_dev || out->albedo_dev), c, *out);
}

int rtx_render_ao(rtx_scene* s, uint32_t rowBegin, uint32_t rowEnd, const rtx_ao_params* par, float* ao, uint32_t* counts, void* stream)
{
	RoctxRange range("Ambient occlusion (rtx_render_ao)");
	if (!s || !par) return fail(RTX_ERR_ARG, "scene/params is NULL");
	int rc = checkAoParams("rtx_render_ao", par, ao, counts);
	if (rc) return rc;
	if (s->stats) return fail(RTX_ERR_UNSUPPORTED, "rtx_render_ao collects no statistics (rtx_counters_enable)");
	TileCall c;
	if (!startTiles(s, rowBegin, rowEnd, stream, c, rc)) return rc;
	const AoArgs a = { par->dirs_dev, par->n_dirs, par->radius, ao, counts };
	return launchTiles(aoKernel(variantOf(s)), c, a);
}

int rtx_render_light(rtx_scene* s, uint32_t rowBegin, uint32_t rowEnd, const rtx_frame_light_buffers* out, void* stream)
{
	RoctxRange range("Direct light (rtx_render_light)");
	if (!s || !out) return fail(RTX_ERR_ARG, "scene/out is NULL");
	const bool perLight = out->light_diffuse_dev || out->light_specular_dev || out->light_open_dev;
	if (!out->diffuse_dev && !out->specular_dev && !perLight) return fail(RTX_ERR_ARG, "rtx_render_light: no output (all five buffers are NULL)");
	int rc = checkPerLight("rtx_render_light", s, perLight, out->n_lights);
	if (rc) return rc;
	if (s->stats) return fail(RTX_ERR_UNSUPPORTED, "rtx_render_light collects no statistics (rtx_counters_enable)");
	TileCall c;
	if (!startTiles(s, rowBegin, rowEnd, stream, c, rc)) return rc;
	return launchTiles(lightFrameKernel(variantOf(s)), c, *out);
}

} // extern "C"
