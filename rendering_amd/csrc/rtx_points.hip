// Direct light and ambient occlusion at caller-supplied surface points (rtx_light_points and rtx_ao_points, include/rtx_points.h; DESIGN.md
// section 3.20): the second halves of rtxRayLightKernel (rtx_light.hip) and rtxAoKernel (rtx_ao.hip) for a caller who already has the
// point and its normal.  The batch is n x 6 floats {P, N} in the layout of a ray buffer, so the front end is that of the ray queries --
// forEachRayWave's persistent waves over the order, whose `origin` and `direction` are P and N here -- and the grouping of large batches
// is theirs.  There is no trace before the loops, no surfaceAtHit, no state machine and no park area: every point counts as a hit.
//
// rtxPointLightKernel: castRay's loop over the lights (rtx_light_loop.h, the text rtxRayLightKernel and rtxRayScatterKernel include) with
// dir = V and ns from the caller's view record, one 16-byte load per point.  The shadow rays of point light i < P.nSrcLights walk with
// source class 2 + i under the two rules that make that copy valid for an origin anywhere in space: the length rule is in the loop's text
// (len2(n) <= P.srcNmax2), the origin-magnitude rule is applied per record by the walk itself (pruneEval8: ainf <= kSrcAinfMax).
// rtxPointAoKernel: rtxAoKernel's loop over the directions (RTX_AO_DIRECTIONS, rtx_rays.hip) -- direction k through the scalar unit, spheres
// and planes asked first, the mesh walk for the lanes still open, a range above FLT_MAX capped for the walk.
#pragma clang fp contract(off)

namespace {
// {V.xyz, ns} of one point: 16 bytes that need not be 16-byte aligned (a caller's slice of a larger buffer)
typedef float PointView __attribute__((ext_vector_type(4), aligned(4)));
} // namespace

template <bool MESH, bool BOXES, int CULLK>
__global__ void __launch_bounds__(256) rtxPointLightKernel(const Params P, const uint32_t* order, const float* view, const rtx_light_buffers out)
{
	fillPowTab();      // (powfRef's tables, in LDS)
	Counts cnt = {};
	// (wave-uniform: what the caller asked for; without a view nothing specular is computed)
	const bool wantD = out.diffuse_dev || out.light_diffuse_dev, wantS = view && (out.specular_dev || out.light_specular_dev);
	const bool wantOpen = out.light_open_dev != nullptr;
	forEachRayWave(P, order, [&](bool valid, uint32_t i, const V3& p, const V3& n) {
		const bool hit = valid;                                // (every point counts as a hit)
		V3 d = mk(0, 0, 0);                                    // castRay's dir: the direction of the ray that arrived at p
		float ns = 0.f;
		if (valid && view) {
			const PointView vw = *(const PointView*)(view + (size_t)i * 4);
			d = mk(vw.x, vw.y, vw.z); ns = vw.w;
		}
		Hit h;
		// the loop over the lights (declares diff and spec, the sums); after every light its terms are stored:
#define RTX_LIGHT_LOOP_PER_LIGHT \
			if (valid) { \
				const size_t at = (size_t)i * nLights + li; \
				if (out.light_diffuse_dev) store3(out.light_diffuse_dev + at * 3, D); \
				if (wantS && out.light_specular_dev) store3(out.light_specular_dev + at * 3, S); \
				if (out.light_open_dev) out.light_open_dev[at] = nOpen; \
			}
#include "rtx_light_loop.h"
		if (valid) {
			if (out.diffuse_dev) store3(out.diffuse_dev + (size_t)i * 3, diff);
			if (wantS && out.specular_dev) store3(out.specular_dev + (size_t)i * 3, spec);
		}
	});
}
RTX_QUERY_INSTANCES(rtxPointLightKernel, (const Params, const uint32_t*, const float*, const rtx_light_buffers))

template <bool MESH, bool BOXES, int CULLK>
__global__ void __launch_bounds__(256) rtxPointAoKernel(const Params P, const uint32_t* order, const AoArgs A)
{
	Counts cnt = {};
	const float tmWalk = RTX_WALK_RANGE(A.radius);
	const uint32_t nDirs = uni(A.nDirs);
	forEachRayWave(P, order, [&](bool valid, uint32_t i, const V3& p, const V3& N) {
		const V3 O = p + N * P.view.bias;                      // castRay's shadow-ray origin (scene.cpp:787)
		Hit h;
		RTX_AO_DIRECTIONS(valid, O, N, A)      // (declares acc; every point counts as a hit)
		if (!valid) return;
		const uint32_t nTraced = acc >> 16, nOpen = acc & 0xFFFFu;
		if (A.counts) A.counts[i] = acc;
		if (A.ao) A.ao[i] = nTraced ? (float)nOpen / (float)nTraced : 1.0f;
	});
}
RTX_QUERY_INSTANCES(rtxPointAoKernel, (const Params, const uint32_t*, const AoArgs))
