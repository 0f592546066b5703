// First-hit buffers of a frame (rtx_render_aov, include/rtx_aov.h): for every pixel of pass 1 the channels of
// Render::trace of its primary ray and of getSurfaceData at the hit -- depth, object id, triangle id, uv, normal, albedo.
//
// One 8x8 tile per wave over a plain grid (the pattern of rtxNormalsKernel's mode 0), the pixel's ray from
// primaryRay (never stored), traceWave in its trace-only form with source class 1 (the camera's copies of the prune records, which only
// rays that start at view.camPos may use).  No state machine, no park area, no recursion frames, no queue.
// SURFACE = false: only the hit record is written; surfaceAtHit of rtx_rays.hip (shadePrimary and its fetches: uv, normals, tangents, maps) is not
// compiled in, which keeps the kernel in the register class of rtxRayHitKernel.  SURFACE = true: its normal and albedo are written as well.
#pragma clang fp contract(off)

template <bool MESH, bool BOXES, int CULLK, bool SURFACE>
__global__ void __launch_bounds__(256) rtxAovKernel(const Params P, const rtx_aov_buffers out)
{
	RTX_TILE_PIXEL()      // (x, y, valid, W)
	V3 o, d;
	primaryRay(P, (float)x + 0.5f, (float)y + 0.5f, o, d);
	Hit h;
	Counts cnt = {};
	traceWave<false, MESH, false, BOXES, CULLK>(P, valid, false, o, d, kFltMax, h, cnt, 1u);
	if (!valid) return;
	// The stores of one channel stay together: a tile row's eight lanes write 32 (depth, ids), 64 (uv) or 96 (normal, albedo) consecutive
	// bytes, eight such runs per instruction.
	const size_t i = (size_t)y * W + x;
	const bool hit = h.obj >= 0;
	if (out.depth_dev) out.depth_dev[i] = h.t;      // (a miss keeps the range it started with: FLT_MAX)
	if (out.object_dev) out.object_dev[i] = hit ? h.obj : -1;
	if (out.triangle_dev) {
		// rtx_cast_rays' record: the triangle of a mesh only (a sphere's or a plane's h.tri is whatever an earlier mesh left)
		const bool mesh = hit && P.objects[hit ? h.obj : 0].type == 3;
		out.triangle_dev[i] = mesh ? (int32_t)h.tri : -1;
	}
	if (out.uv_dev) { float* p = out.uv_dev + i * 2; p[0] = hit ? h.u : -1.f; p[1] = hit ? h.v : -1.f; }
	if (SURFACE) {
		V3 p, n, a;
		float ks;
		surfaceAtHit(P, h, o, d, p, n, a, ks);
		if (out.normal_dev) store3(out.normal_dev + i * 3, n);
		if (out.albedo_dev) store3(out.albedo_dev + i * 3, a);
	}
}
// (each with and without the surface fetch)
RTX_QUERY_INSTANCES(rtxAovKernel, (const Params, const rtx_aov_buffers), false)
RTX_QUERY_INSTANCES(rtxAovKernel, (const Params, const rtx_aov_buffers), true)
