// Reflection and refraction rays at the hits of caller-supplied rays (rtx_scatter_rays and rtx_sky_rays, include/rtx_scatter.h; DESIGN.md
// section 3.19): Render::trace of every ray of a batch, getSurfaceData at its hit, castRay's sums over the lights there where the hit's
// material reads them, and what castRay does next (scene.cpp:808, 852, 856-858, 893-907, 940) short of recursing -- the part of the colour
// that needs no further ray, the reflection and the refraction ray, their factors and which of them exist -- each written at the ray's own index.
//
// One launch and one walk of the caller's ray: the shared steps of rtx_rays.hip (forEachRayWave, traceWave in its trace-only form,
// surfaceAtHit), then the wave-uniform light loop of rtx_light.hip (rtx_light_loop.h) with per-lane requests -- a Diffuse hit asks for the diffuse
// sum, a Reflective or Transparent one for the specular sum, a Phong one for both, a miss for neither; no light is looked at when the caller
// wants no `local`, nor by a wave none of whose lanes asks --, then the arithmetic of ST_LIGHTS_DONE in rtx_kernels.hip with its device
// functions and operand order.  No state machine, no park area, no recursion frames.
#pragma clang fp contract(off)

template <bool MESH, bool BOXES, int CULLK>
__global__ void __launch_bounds__(256) rtxRayScatterKernel(const Params P, const uint32_t* order, const rtx_scatter_buffers out)
{
	// (wave-uniform: what the caller asked for)
	const bool wantLocal = out.local_dev != nullptr;
	const bool wantRays = out.reflect_dev || out.refract_dev;
	if (wantLocal) fillPowTab();      // (powfRef's tables, in LDS; the same branch in every wave of the grid)
	Counts cnt = {};
	forEachRayWave(P, order, [&](bool valid, uint32_t i, const V3& o, const V3& d) {
		Hit h;
		traceWave<false, MESH, false, BOXES, CULLK>(P, valid, false, o, d, kFltMax, h, cnt);
		if (valid && out.hits_dev) storeHit(P, h, out.hits_dev + (size_t)i * 8);
		const bool hit = valid && h.obj >= 0;
		V3 p, n, albedo;
		float ks;
		surfaceAtHit(P, h, o, d, p, n, albedo, ks);          // (a miss: albedo = getSkybox(d))
		const Object* ob = P.objects + (hit ? h.obj : 0);
		const int mat = hit ? ob->material : -1;             // 0 Diffuse, 1 Reflective, 2 Transparent, 3 Phong
		V3 sumD = mk(0, 0, 0), sumS = mk(0, 0, 0);             // rtx_light_rays' diffuse and specular, where the material reads them
		// (per lane: a Diffuse hit reads the diffuse sum, a Reflective or Transparent one the specular sum, a Phong one both, a miss neither)
		const bool wantD = wantLocal && (mat == 0 || mat == 3), wantS = wantLocal && mat >= 1;
		if (ballot(wantD || wantS) != 0) {
			const float ns = hit ? ob->nSpecular : 0.f;
			const bool wantOpen = false;
#define RTX_LIGHT_LOOP_PER_LIGHT
#include "rtx_light_loop.h"
			sumD = diff; sumS = spec;
		}
		if (!valid) return;
		V3 local = albedo;                                   // a miss: scene.cpp:945
		V3 fo = mk(0, 0, 0), fd = mk(0, 0, 0), ro = mk(0, 0, 0), rd = mk(0, 0, 0);
		float wf = 0, wr = 0;
		uint32_t kinds = 0;
		if (mat == 0) local = albedo * sumD;                                              // scene.cpp:808
		else if (mat == 3) local = albedo * ob->ambient + sumD * ob->diffuse + sumS * ks;   // scene.cpp:852
		else if (mat == 1) {                                                              // scene.cpp:856-858, 890
			local = sumS;
			fo = p + n * P.view.bias; fd = d - n * (2 * dot(d, n));
			wf = 0.8f; kinds = 1;
		}
		else if (mat == 2) {                                                              // scene.cpp:893-907, 940
			const float ior = ob->ior;
			const float kr = fresnelKr(d, n, ior);
			const bool outside = dot(d, n) < 0;
			const V3 biasVec = n * P.view.bias;
			local = sumS * kr;
			if (wantRays) fd = normalized(reflectDir(d, n));
			fo = outside ? p + biasVec : p - biasVec;
			wf = kr; kinds = 1;
			if (kr < 1) {
				if (wantRays) rd = normalized(refractDir(d, n, ior));
				ro = outside ? p - biasVec : p + biasVec;
				wr = 1 - kr; kinds = 3;
			}
		}
		if (out.local_dev) store3(out.local_dev + (size_t)i * 3, local);
		if (out.reflect_dev) { store3(out.reflect_dev + (size_t)i * 6, fo); store3(out.reflect_dev + (size_t)i * 6 + 3, fd); }
		if (out.refract_dev) { store3(out.refract_dev + (size_t)i * 6, ro); store3(out.refract_dev + (size_t)i * 6 + 3, rd); }
		if (out.weight_dev) { out.weight_dev[(size_t)i * 2] = wf; out.weight_dev[(size_t)i * 2 + 1] = wr; }
		if (out.kinds_dev) out.kinds_dev[i] = (uint8_t)kinds;
	});
}
RTX_QUERY_INSTANCES(rtxRayScatterKernel, (const Params, const uint32_t*, const rtx_scatter_buffers))

// rtx_sky_rays: Scene::getSkybox of every ray's direction (scene.cpp:381-442), a plain grid.
__global__ void __launch_bounds__(256) rtxRaySkyKernel(const Params P, float* colours)
{
	const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= P.nProbe) return;
	store3(colours + i * 3, skyColor(P, load3(P.probeRays + i * 6 + 3)));
}
