// Ambient occlusion of a frame (rtx_render_ao, include/rtx_ao.h): for every pixel of pass 1 the number of the
// caller's directions that leave its first hit on the side of the normal, and how many of those reach the range unoccluded.
//
// rtxAovKernel's launch and first half -- one 8x8 tile per wave over a plain grid, primaryRay, traceWave in its trace-only form with source
// class 1, shadePrimary on the lanes that hit (of which only P and N stay alive) -- followed by rtxRayOccludedKernel's any-hit trace in a
// wave-uniform loop over the directions.  Direction k comes through the scalar unit and is the same for all 64 lanes, so every bundle the
// walk is handed is 64 parallel rays that leave one 8x8 patch of surface: no ray is stored or read, nothing is sorted.  The origins are not
// the camera's, so these traces use the general source class (0).  No state machine, no park area, no recursion frames, no queue.
// Both halves are written out here: on the shared steps of rtx_rays.hip (surfaceAtHit) and with the any-hit trace as a helper of its own this
// kernel measured 1 % slower at 4096^2.
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
	const uint32_t wave = blockIdx.x * 4 + (threadIdx.x >> 6), lane = __lane_id();
	if (wave >= P.nTiles) return;
	const uint32_t W = P.view.width, H = P.view.height;
	const uint32_t tx = wave % P.tilesX, ty = P.tileRow0 + wave / P.tilesX;
	const uint32_t x = tx * 8 + (lane & 7), y = ty * 8 + (lane >> 3);
	// rtxAovKernel's pixels: pass 1's, of the rows this part owns
	const bool valid = x < W - 1 && y < H - 1 && y >= P.rowBegin && y < P.rowEnd && rowOwned(P.bandH, P.nParts, P.part, y);
	if (ballot(valid) == 0) return;
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
	// A mesh records only t < FLT_MAX, so a range above FLT_MAX is FLT_MAX for its walk, whose bundle limit has to stay finite; a sphere or
	// a plane is compared with the range itself (rtxRayOccludedKernel).
	const float tm = A.radius;
	const float tmWalk = tm > kFltMax ? kFltMax : tm;
	uint32_t acc = 0;               // open | traced << 16
	const uint32_t nDirs = uni(A.nDirs);
	for (uint32_t k = 0; k < nDirs; k = uni(k + 1)) {
		const float* dk = uni(A.dirs + (size_t)k * 3);
		const V3 d = mk(sloadf(dk), sloadf(dk + 1), sloadf(dk + 2));
		const float c = dot(N, d);
		const bool traced = hit && c > 0;       // (strict: a zero or NaN direction, or a NaN normal, is never traced)
		if (ballot(traced) == 0) continue;
		bool open = traced;
		if (!MESH) {
			traceWave<false, false, false, BOXES, CULLK>(P, open, true, O, d, tm, h, cnt);
			open = open && h.obj < 0;
		}
		else {
			traceWave<false, false, false, BOXES, CULLK, 1>(P, open, true, O, d, tm, h, cnt);
			open = open && h.obj < 0;
			if (ballot(open) != 0) {
				traceWave<false, true, false, BOXES, CULLK, 2>(P, open, true, O, d, tmWalk, h, cnt);
				open = open && h.obj < 0;
			}
		}
		acc += (traced ? 0x10000u : 0u) + (open ? 1u : 0u);
	}
	if (!valid) return;
	// one 4-byte store per output: a tile row's eight lanes write 32 consecutive bytes, eight such runs per instruction
	const size_t i = (size_t)y * W + x;
	const uint32_t nTraced = acc >> 16, nOpen = acc & 0xFFFFu;
	if (A.counts) A.counts[i] = acc;
	if (A.ao) A.ao[i] = nTraced ? (float)nOpen / (float)nTraced : 1.0f;
}

RTX_QUERY_INSTANCES(rtxAoKernel, (const Params, const AoArgs))
