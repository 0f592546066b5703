// Surface data at the hits of caller-supplied rays (rtx_surface_rays, include/rtx_surface.h): Render::trace of
// every ray of a batch and getSurfaceData at its hit -- hit record, hit point, shading normal, albedo, specular coefficient -- each
// written at the ray's own index.
//
// Built from the shared steps of rtx_rays.hip: forEachRayWave hands every persistent wave its rays through the order, traceWave runs in
// its trace-only form with the general source class (these rays start anywhere), surfaceAtHit fetches the surface of the lanes that hit
// and the sky colour of the others, storeHit and store3 write.  A request for the hit records alone never comes here (rtx_query.hip
// launches rtxRayHitKernel for it), so the surface fetch is the only form of this kernel.
#pragma clang fp contract(off)

template <bool MESH, bool BOXES, int CULLK>
__global__ void __launch_bounds__(256) rtxRaySurfaceKernel(const Params P, const uint32_t* order, const rtx_surface_buffers out)
{
	Counts cnt = {};
	forEachRayWave(P, order, [&](bool valid, uint32_t i, const V3& o, const V3& d) {
		Hit h;
		traceWave<false, MESH, false, BOXES, CULLK>(P, valid, false, o, d, kFltMax, h, cnt);
		if (!valid) return;
		if (out.hits_dev) storeHit(P, h, out.hits_dev + (size_t)i * 8);
		V3 p, n, a;
		float ks;
		surfaceAtHit(P, h, o, d, p, n, a, ks);
		// one 12-byte store per lane and channel
		if (out.position_dev) store3(out.position_dev + (size_t)i * 3, p);
		if (out.normal_dev) store3(out.normal_dev + (size_t)i * 3, n);
		if (out.albedo_dev) store3(out.albedo_dev + (size_t)i * 3, a);
		if (out.specular_dev) out.specular_dev[i] = ks;
	});
}
RTX_QUERY_INSTANCES(rtxRaySurfaceKernel, (const Params, const uint32_t*, const rtx_surface_buffers))
