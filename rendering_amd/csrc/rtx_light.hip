// Direct light at the hits of caller-supplied rays (rtx_light_rays, include/rtx_light.h): Render::trace of every
// ray of a batch, getSurfaceData at its hit, and castRay's loop over the lights there (scene.cpp:780-846) -- the diffuse and the specular
// sum, each light's term of both and the number of its shadow rays that arrive -- each written at the ray's own index.
//
// First half: the shared steps of rtx_rays.hip (forEachRayWave, traceWave in its trace-only form with the general source class,
// surfaceAtHit), of which P, N and the ray's direction stay alive.  Second half: a wave-uniform loop over the lights, as castRayPlainWave's:
// light i's record comes through the scalar unit and is the same for all 64 lanes, so is the sample point of an area light in the inner
// loop; every bundle the walk is handed is 64 shadow rays towards one source.  The any-hit trace has rtxAoKernel's shape -- spheres and
// planes first, the mesh walk only for the lanes still open -- and is that kernel's text, RTX_ANY_HIT of rtx_rays.hip (one site for every
// kind of light): as a function shared with the other kernels it cost them 1-5 %.  The loop's text is rtx_light_loop.h, which rtx_scatter.hip includes as well.  The shadow rays of point light i < P.nSrcLights walk with source class 2 + i, the rule
// of advance() in rtx_kernels.hip.  No state machine, no park area, no recursion frames.
#pragma clang fp contract(off)

namespace {
__device__ __forceinline__ bool plusZero(const V3& v) { return (__float_as_uint(v.x) | __float_as_uint(v.y) | __float_as_uint(v.z)) == 0u; }
} // namespace

template <bool MESH, bool BOXES, int CULLK>
__global__ void __launch_bounds__(256) rtxRayLightKernel(const Params P, const uint32_t* order, const rtx_light_buffers out)
{
	fillPowTab();      // (powfRef's tables, in LDS)
	Counts cnt = {};
	// (wave-uniform: what the caller asked for)
	const bool wantD = out.diffuse_dev || out.light_diffuse_dev, wantS = out.specular_dev || out.light_specular_dev;
	const bool wantOpen = out.light_open_dev != nullptr;
	forEachRayWave(P, order, [&](bool valid, uint32_t i, const V3& o, const V3& d) {
		Hit h;
		traceWave<false, MESH, false, BOXES, CULLK>(P, valid, false, o, d, kFltMax, h, cnt);
		if (valid && out.hits_dev) storeHit(P, h, out.hits_dev + (size_t)i * 8);
		if (!(wantD || wantS || wantOpen)) return;
		const bool hit = valid && h.obj >= 0;
		V3 p, n, albedo;
		float ks;
		surfaceAtHit(P, h, o, d, p, n, albedo, ks);          // (of which only p and n are used)
		const float ns = hit ? P.objects[h.obj].nSpecular : 0.f;
		// the loop over the lights (declares diff and spec, the sums); after every light its terms are stored:
#define RTX_LIGHT_LOOP_PER_LIGHT \
			if (valid) { \
				const size_t at = (size_t)i * nLights + li; \
				if (out.light_diffuse_dev) store3(out.light_diffuse_dev + at * 3, D); \
				if (out.light_specular_dev) store3(out.light_specular_dev + at * 3, S); \
				if (out.light_open_dev) out.light_open_dev[at] = nOpen; \
			}
#include "rtx_light_loop.h"
		if (valid) {
			if (out.diffuse_dev) store3(out.diffuse_dev + (size_t)i * 3, diff);
			if (out.specular_dev) store3(out.specular_dev + (size_t)i * 3, spec);
		}
	});
}
RTX_QUERY_INSTANCES(rtxRayLightKernel, (const Params, const uint32_t*, const rtx_light_buffers))
