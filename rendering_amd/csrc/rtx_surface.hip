// Surface data at the hits of caller-supplied rays (rtx_surface_rays, include/rtx_surface.h): Render::trace of
// every ray of a batch and getSurfaceData at its hit -- hit record, hit point, shading normal, albedo, specular coefficient -- each
// written at the ray's own index.
//
// rtxRayHitKernel's loop (persistent waves, nextWork, loadRay through the order, traceWave in its trace-only form with the general source
// class: these rays start anywhere) followed by rtxAovKernel's surface tail (shadePrimary on the lanes that hit, skyColor on the others).
// A request for the hit records alone never comes here (rtx_api.hip launches rtxRayHitKernel for it), so the surface fetch is the only
// form of this kernel.
#pragma clang fp contract(off)

template <bool MESH, bool BOXES, int CULLK>
__global__ void __launch_bounds__(256) rtxRaySurfaceKernel(const Params P, const uint32_t* order, const rtx_surface_buffers out)
{
	const uint32_t lane = __lane_id();
	const uint32_t nWork = (P.nProbe + 63) / 64;
	Counts cnt = {};
	for (;;) {
		const uint32_t work = nextWork(P.workCounter);
		if (work >= nWork) break;
		const uint32_t k = work * 64 + lane;
		const bool valid = k < P.nProbe;
		uint32_t i; V3 o, d;
		loadRay(P, order, k, valid, i, o, d);
		Hit h;
		traceWave<false, MESH, false, BOXES, CULLK>(P, valid, false, o, d, kFltMax, h, cnt);
		if (valid) {
			if (out.hits_dev) storeHit(P, h, out.hits_dev + (size_t)i * 8);
			V3 p = mk(0, 0, 0), n = mk(0, 0, 0), a;
			float ks = 0;
			if (h.obj >= 0) {
				Lane s;
				s.ro = o; s.rd = d;
				shadePrimary(P, s, h);      // (only the lanes that hit are here: its loop is over their objects)
				p = s.P; n = s.N; a = s.objColor; ks = s.specCoef;
			}
			else a = skyColor(P, d);
			// one 12-byte store per lane and channel
			if (out.position_dev) { float* q = out.position_dev + (size_t)i * 3; q[0] = p.x; q[1] = p.y; q[2] = p.z; }
			if (out.normal_dev) { float* q = out.normal_dev + (size_t)i * 3; q[0] = n.x; q[1] = n.y; q[2] = n.z; }
			if (out.albedo_dev) { float* q = out.albedo_dev + (size_t)i * 3; q[0] = a.x; q[1] = a.y; q[2] = a.z; }
			if (out.specular_dev) out.specular_dev[i] = ks;
		}
	}
}

// per (box test of the prune records, culling) as the hit kernel; scenes without meshes have the walk-free form
template __global__ void rtxRaySurfaceKernel<true, true, 1>(const Params, const uint32_t*, const rtx_surface_buffers);
template __global__ void rtxRaySurfaceKernel<true, false, 1>(const Params, const uint32_t*, const rtx_surface_buffers);
template __global__ void rtxRaySurfaceKernel<true, true, 0>(const Params, const uint32_t*, const rtx_surface_buffers);
template __global__ void rtxRaySurfaceKernel<true, false, 0>(const Params, const uint32_t*, const rtx_surface_buffers);
template __global__ void rtxRaySurfaceKernel<false, true, -1>(const Params, const uint32_t*, const rtx_surface_buffers);
