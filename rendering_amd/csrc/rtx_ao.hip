// Ambient occlusion of a frame (rtx_render_ao, include/rtx_ao.h): for every pixel of pass 1 the number of the
// caller's directions that leave its first hit on the side of the normal, and how many of those reach the range unoccluded.
//
// rtxAovKernel's launch and first half -- one 8x8 tile per wave over a plain grid, primaryRay, traceWave in its trace-only form with source
// class 1, shadePrimary on the lanes that hit (of which only P and N stay alive) -- followed by rtxRayOccludedKernel's any-hit trace in a
// wave-uniform loop over the directions.  Direction k comes through the scalar unit and is the same for all 64 lanes, so every bundle the
// walk is handed is 64 parallel rays that leave one 8x8 patch of surface: no ray is stored or read, nothing is sorted.  The origins are not
// the camera's, so these traces use the general source class (0).  No state machine, no park area, no recursion frames, no queue.
// The first half is written out here and the second is shared as text (RTX_AO_DIRECTIONS and RTX_ANY_HIT, rtx_rays.hip): on the shared
// steps of rtx_rays.hip (surfaceAtHit) and with the any-hit trace as a helper function of its own this kernel measured 1 % slower at 4096^2
// (DESIGN.md 3.14).
#pragma clang fp contract(off)

struct AoArgs {
	const float* dirs;      // nDirs x 3
	uint32_t nDirs;
	float radius;
	float* ao;              // H*W or nullptr
	uint32_t* counts;       // H*W or nullptr
};

template <bool MESH, bool BOXES, int CULLK>
__global__ void __launch_bounds__(256) rtxAoKernel(const Params P, const AoArgs A)
{
	RTX_TILE_PIXEL()      // (x, y, valid, W)
	Hit h;
	Counts cnt = {};
	V3 O = mk(0, 0, 0), N = mk(0, 0, 0);
	bool hit;
	{
		V3 o, d;
		primaryRay(P, (float)x + 0.5f, (float)y + 0.5f, o, d);
		traceWave<false, MESH, false, BOXES, CULLK>(P, valid, false, o, d, kFltMax, h, cnt, 1u);
		hit = valid && h.obj >= 0;
		if (hit) {
			Lane s;
			s.ro = o; s.rd = d;
			shadePrimary(P, s, h);      // (only the lanes that hit are here: its loop is over their objects)
			N = s.N;
			O = s.P + s.N * P.view.bias;        // castRay's shadow-ray origin (scene.cpp:787)
		}
	}
	const float tmWalk = RTX_WALK_RANGE(A.radius);
	const uint32_t nDirs = uni(A.nDirs);
	RTX_AO_DIRECTIONS(hit, O, N, A)      // (declares acc)
	if (!valid) return;
	// one 4-byte store per output: a tile row's eight lanes write 32 consecutive bytes, eight such runs per instruction
	const size_t i = (size_t)y * W + x;
	const uint32_t nTraced = acc >> 16, nOpen = acc & 0xFFFFu;
	if (A.counts) A.counts[i] = acc;
	if (A.ao) A.ao[i] = nTraced ? (float)nOpen / (float)nTraced : 1.0f;
}

RTX_QUERY_INSTANCES(rtxAoKernel, (const Params, const AoArgs))
