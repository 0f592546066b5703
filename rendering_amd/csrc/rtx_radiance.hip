// Radiance gathered over a set of directions at caller-supplied surface points (rtx_radiance_points, include/rtx_radiance.h; DESIGN.md
// section 3.23): for every point {P, N} the weighted sum of Render::castRay({P + N * bias, d_k}, scene, 0) over the caller's directions
// that leave the surface on the side of the normal.
//
// The front end is the point queries' (rtx_points.hip): forEachRayWave's persistent waves over the order, whose `origin` and `direction`
// are P and N.  The loop over the directions has the pattern of RTX_AO_DIRECTIONS (rtx_rays.hip) -- direction k through the scalar unit,
// the same for all 64 lanes, traced by a lane iff N . d > 0, skipped when no lane traces it -- and inside it is what rtxRayColourKernel
// does with a ray: castRayPlainWave for PLAIN mesh scenes, castRayWave otherwise, with CAM = false and the lane predicate `traced`.  So a
// wave casts 64 rays of one direction that leave neighbouring points: no ray is stored, nothing of n x n_dirs rays is regrouped.
//
// What stays alive across the recursion: the point's index, and nothing else per lane.
//  - P, N and the direction are read again per direction (the batch's 24 bytes per point stay in L2 between two directions; the direction
//    and its weight come through the scalar unit), and c = N . d is computed again after the recursion from the same operands in the same
//    order, which gives the same bits.
//  - The sums wait in the caller's own buffer, at the point's own index: +0 is stored first, and every traced direction loads the three
//    floats, adds its products and stores them again -- the same additions in the same order as in registers.
//  - The number of traced directions needs no ray: it is counted in a loop of its own over the dot products.  A call that asks for the
//    counts alone casts nothing.
// The recursion frames are the pass-1 area indexed by the global lane, as rtxRayColourKernel's: the grid is at most blocksPass1
// (rtx_query.hip).
#pragma clang fp contract(off)

struct RadianceArgs {
	const float* dirs;       // nDirs x 3
	const float* weights;    // nDirs or nullptr (1.0f)
	uint32_t nDirs;
	int32_t cosine;          // the weight of direction k times c = N . d_k
	float* sum;              // n x 3 or nullptr
	uint32_t* counts;        // n or nullptr
};

template <bool MESH, bool BOXES, int CULLK, bool PLAIN>
__global__ void __launch_bounds__(256, MESH ? (PLAIN ? RTX_WAVES_PLAIN : RTX_WAVES) : RTX_WAVES_ANALYTIC) rtxPointRadianceKernel(const Params P, const uint32_t* order, const RadianceArgs A)
{
	if (!PLAIN) fillPowTab();
	const uint32_t gl = blockIdx.x * blockDim.x + threadIdx.x;
	Counts cnt = {};
	const uint32_t nDirs = uni(A.nDirs);
	forEachRayWave(P, order, [&](bool valid, uint32_t i, const V3&, const V3&) {
		// (a lane without a point reads point 0's record, loadRay's i, and traces nothing)
		const float* pn = P.probeRays + (size_t)i * 6;
		if (A.counts) {
			const V3 N = load3(pn + 3);
			uint32_t nTraced = 0;
			for (uint32_t k = 0; k < nDirs; k = uni(k + 1)) {
				const float* dk = uni(A.dirs + (size_t)k * 3);
				if (dot(N, mk(sloadf(dk), sloadf(dk + 1), sloadf(dk + 2))) > 0) nTraced++;
			}
			if (valid) A.counts[i] = nTraced;
		}
		if (!A.sum) return;
		float* acc = A.sum + (size_t)i * 3;
		if (valid) store3(acc, mk(0, 0, 0));
		for (uint32_t k = 0; k < nDirs; k = uni(k + 1)) {
			V3 L;
			bool traced;
			{
				const float* dk = uni(A.dirs + (size_t)k * 3);
				const V3 d = mk(sloadf(dk), sloadf(dk + 1), sloadf(dk + 2));
				const V3 p = load3(pn), N = load3(pn + 3);
				traced = valid && dot(N, d) > 0;      // strict: a zero or NaN direction or normal is never traced
				if (ballot(traced) == 0) continue;
				const V3 O = p + N * P.view.bias;     // castRay's shadow-ray origin (scene.cpp:787)
				if constexpr (PLAIN) L = castRayPlainWave<false, false, BOXES, false, CULLK>(P, traced, O, d, gl, cnt);
				else L = castRayWave<false, MESH, false, BOXES, false, CULLK, PLAIN>(P, traced, O, d, gl, cnt);
			}
			// the weight: through the scalar unit, times c when asked -- N and d again, the same products and sums as above
			float w = 1.0f;
			if (A.weights) w = sloadf(uni(A.weights + k));
			if (A.cosine) {
				const float* dk = uni(A.dirs + (size_t)k * 3);
				w = w * dot(load3(pn + 3), mk(sloadf(dk), sloadf(dk + 1), sloadf(dk + 2)));
			}
			if (traced) store3(acc, load3(acc) + L * w);
		}
	});
}
RTX_QUERY_INSTANCES(rtxPointRadianceKernel, (const Params, const uint32_t*, const RadianceArgs), false)
RTX_MESH_INSTANCES(rtxPointRadianceKernel, (const Params, const uint32_t*, const RadianceArgs), true)
