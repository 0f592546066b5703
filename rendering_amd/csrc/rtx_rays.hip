// Caller-supplied rays on the device (rtx_trace_rays, include/rtx.h): Render::trace and Render::castRay at depth 0 for a batch of rays
// handed over in device memory, on the caller's stream.  DESIGN.md section 3.6.
//
// The walk (traceWave) is built for bundles of 64 coherent rays: one box of origins times one box of directions.  Rays in the order a
// caller hands them over can be anything but coherent, so by default they are first grouped (the launch code in rtx_query.hip):
//   1. rtxRayBoxKernel: the range of the rays' five key coordinates (direction and origin as seen from the camera: rayCoords), and how
//      far they spread within the caller's own groups of 64;
//   2. rtxRayKeyKernel: a 30-bit key per ray, the Morton interleave of the coordinates whose range is not empty, normalised to it
//      (camera rays: all bits go to the direction -- their 64-ray groups are 8 x 8 pixel blocks) -- or 0 for every ray when the caller's
//      groups are already as tight as sorted ones would be (the sort then keeps the caller's order);
//   3. a stable radix sort of (key, index) pairs (rtx_sort.hip: rocPRIM), ties in index order;
//   4. rtxRayHitKernel / rtxRayColourKernel / rtxRayNormalsKernel: persistent waves take 64 consecutive entries of the order, read
//      their rays through it and write every result at the ray's own index.
// Grouping changes the amount of work only: the walk's result for a ray does not depend on the other lanes of its bundle (the filter
// rejects only what the reference is certain to reject, ties are broken in index order), so every ray's hit record and colour are
// the bits rtx_cast_rays returns for it (tests/test_gpu_trace_rays.py).
#pragma clang fp contract(off)

namespace {

constexpr int kRayKeyBits = 30;          // bits of the sort key (the radix sort runs over these only)

// float <-> uint32 with the order of the floats (min / max by integer atomics)
__device__ __forceinline__ uint32_t orderedBits(float f)
{
	const uint32_t u = __float_as_uint(f);
	return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float orderedFloat(uint32_t u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }

// A direction in the frame of the camera axes (ax), as a point of the octahedral map whose centre is the camera's view direction (-z):
// the map's only seam, its corners, is then behind the camera.  (A zero vector gives NaN.)
struct RayAxes { float m[9]; float cam[3]; };
__device__ __forceinline__ void octahedral(const RayAxes& ax, float dx, float dy, float dz, float& u, float& v)
{
	const float x = dx * ax.m[0] + dy * ax.m[1] + dz * ax.m[2];
	const float y = dx * ax.m[3] + dy * ax.m[4] + dz * ax.m[5];
	const float z = dx * ax.m[6] + dy * ax.m[7] + dz * ax.m[8];
	const float l1 = fabsf(x) + fabsf(y) + fabsf(z);
	u = x / l1; v = y / l1;
	if (z > 0) {
		const float fu = (1.0f - fabsf(v)) * (u < 0 ? -1.0f : 1.0f), fv = (1.0f - fabsf(u)) * (v < 0 ? -1.0f : 1.0f);
		u = fu; v = fv;
	}
}

// The five key coordinates of a ray: its direction on the map, and its origin as seen from the camera -- the map point of the way from
// the camera to it and the log of its distance.  (Hit points of camera rays keep their pixels' neighbourhoods, and a far-away plane
// does not squeeze the rest of the scene into a few cells.  A ray starting at the camera has no finite origin coordinates.)
__device__ __forceinline__ void rayCoords(const float* ray, const RayAxes& ax, float c[5])
{
	octahedral(ax, ray[3], ray[4], ray[5], c[0], c[1]);
	const float ox = ray[0] - ax.cam[0], oy = ray[1] - ax.cam[1], oz = ray[2] - ax.cam[2];
	octahedral(ax, ox, oy, oz, c[2], c[3]);
	c[4] = __builtin_log2f(fabsf(ox) + fabsf(oy) + fabsf(oz));
}

__device__ __forceinline__ float waveMinF(float v)
{
	for (int k = 32; k >= 1; k >>= 1) v = fminf(v, __shfl_xor(v, k));
	return v;
}
__device__ __forceinline__ float waveMaxF(float v)
{
	for (int k = 32; k >= 1; k >>= 1) v = fmaxf(v, __shfl_xor(v, k));
	return v;
}

} // namespace

// box[0, 5): the ordered bits of the smallest finite value of each coordinate, box[5, 10) of the largest (~0 / 0 before the launch);
// spread[k]: the sum over the caller's groups of 64 consecutive rays of the range of coordinate k within the group (0 before the launch).
// Non-finite coordinates take no part: such rays go to the edges of the key's range.  One wave per group.
__global__ void __launch_bounds__(256) rtxRayBoxKernel(const float* rays, uint32_t n, RayAxes ax, uint32_t* box, double* spread)
{
	float lo[5], hi[5];
	double sp[5];
	for (int k = 0; k < 5; k++) { lo[k] = __builtin_inff(); hi[k] = -__builtin_inff(); sp[k] = 0.0; }
	const uint32_t groups = (uint32_t)(((size_t)n + 63) / 64), waves = gridDim.x * 4;
	for (uint32_t g = blockIdx.x * 4 + (threadIdx.x >> 6); g < groups; g += waves) {
		const size_t i = (size_t)g * 64 + __lane_id();
		float c[5] = { 0, 0, 0, 0, 0 };
		const bool valid = i < n;
		if (valid) rayCoords(rays + i * 6, ax, c);
		for (int k = 0; k < 5; k++) {
			const bool fin = valid && fabsf(c[k]) < __builtin_inff();
			const float a = waveMinF(fin ? c[k] : __builtin_inff()), b = waveMaxF(fin ? c[k] : -__builtin_inff());
			if (a <= b) { lo[k] = fminf(lo[k], a); hi[k] = fmaxf(hi[k], b); sp[k] += (double)b - (double)a; }
		}
	}
	// (lo, hi, sp are the same in every lane of a wave)
	__shared__ float part[2][5][4];
	__shared__ double partSp[5][4];
	const uint32_t w = threadIdx.x >> 6;
	if (__lane_id() == 0) for (int k = 0; k < 5; k++) { part[0][k][w] = lo[k]; part[1][k][w] = hi[k]; partSp[k][w] = sp[k]; }
	__syncthreads();
	if (threadIdx.x < 5) {
		const int k = threadIdx.x;
		const float a = fminf(fminf(part[0][k][0], part[0][k][1]), fminf(part[0][k][2], part[0][k][3]));
		const float b = fmaxf(fmaxf(part[1][k][0], part[1][k][1]), fmaxf(part[1][k][2], part[1][k][3]));
		if (a <= b) {
			atomicMin(box + k, orderedBits(a)); atomicMax(box + 5 + k, orderedBits(b));
			atomicAdd(spread + k, (partSp[k][0] + partSp[k][1]) + (partSp[k][2] + partSp[k][3]));
		}
	}
}

// keys[i] = the Morton interleave of ray i's coordinates, each normalised to the box of rtxRayBoxKernel.  A coordinate whose range is
// empty (every camera ray has the same origin) gets no bits; the others share kRayKeyBits in turns, most significant bits first,
// starting with the direction (originFirst = 0) or the origin (1).
// check != 0: every key is 0 -- the stable sort then keeps the caller's order -- when the caller's groups of 64 rays are already as tight
// as sorting would make them in the coordinates the walks depend on most: the origin's, which shadow rays share (the direction's for rays
// from one point).  Sorted, a group covers about (64 / n)^(1 / dims) of each coordinate's range (n rays filling the box); the caller's
// groups cover spread[k] / groups of it on average.
__global__ void __launch_bounds__(256) rtxRayKeyKernel(const float* rays, uint32_t n, RayAxes ax, const uint32_t* box, const double* spread,
                                                       int originFirst, int check, uint32_t* keys)
{
	const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	int dims[5], nd = 0;
	float base[5], scale[5];
	double haveO = 0, haveD = 0;
	int nO = 0, nD = 0;
	const double groups = (double)(((size_t)n + 63) / 64);
	for (int j = 0; j < 5; j++) {
		const int k = originFirst ? (j + 2) % 5 : j;
		const float a = orderedFloat(box[k]), b = orderedFloat(box[5 + k]);
		if (!(b > a) || !(b - a < __builtin_inff())) continue;
		base[nd] = a; scale[nd] = 1.0f / (b - a); dims[nd] = k; nd++;
		const double have = spread[k] / groups / ((double)b - (double)a);
		if (k >= 2) { haveO += have; nO++; } else { haveD += have; nD++; }
	}
	uint32_t key = 0;
	const bool keep = check && nd > 0 && (nO ? haveO / nO : haveD / nD) <= exp2(log2(64.0 / (double)n) / nd);
	if (nd > 0 && !keep) {
		float c[5];
		rayCoords(rays + i * 6, ax, c);
		const int per = kRayKeyBits / nd;
		uint32_t q[5];
		for (int j = 0; j < nd; j++) {
			// (NaN: fmaxf gives 0)
			const float f = fminf(fmaxf((c[dims[j]] - base[j]) * scale[j], 0.0f), 1.0f) * (float)(1u << per);
			q[j] = min((uint32_t)f, (1u << per) - 1u);
		}
		for (int b = per - 1; b >= 0; b--)
			for (int j = 0; j < nd; j++) key = key << 1 | ((q[j] >> b) & 1u);
		key <<= kRayKeyBits - per * nd;
	}
	keys[i] = key;
}

namespace {

// ---- The steps the query kernels share (this file's and those of rtx_surface.hip and rtx_aov.hip, which come after it) ----

// Entry k of the order: the index of the ray lane k takes (order == nullptr: the rays as handed over).
__device__ __forceinline__ void loadRay(const Params& P, const uint32_t* order, uint32_t k, bool valid, uint32_t& i, V3& o, V3& d)
{
	i = valid ? (order ? order[k] : k) : 0u;
	o = mk(0, 0, 0); d = mk(0, 0, -1);
	if (valid) { o = load3(P.probeRays + (size_t)i * 6); d = load3(P.probeRays + (size_t)i * 6 + 3); }
}

// The loop of a persistent wave over the P.nProbe rays at P.probeRays: the next 64 entries of the order off the launch's queue
// (P.workCounter) until it is empty, one ray per lane.  body(valid, i, o, d) -- valid: the lane has a ray (the last group may be short);
// i: the ray's own index, where its results go.  The whole wave is in body, so that it can walk its rays as one bundle.
// (rtxRayOccludedKernel and rtxRayNormalsKernel have this loop written out: DESIGN.md 3.14.)
template <typename Body>
__device__ __forceinline__ void forEachRayWave(const Params& P, const uint32_t* order, Body&& body)
{
	const uint32_t lane = __lane_id();
	const uint32_t nWork = (P.nProbe + 63) / 64;
	for (;;) {
		const uint32_t work = nextWork(P.workCounter);
		if (work >= nWork) break;
		const uint32_t k = work * 64 + lane;
		const bool valid = k < P.nProbe;
		uint32_t i; V3 o, d;
		loadRay(P, order, k, valid, i, o, d);
		body(valid, i, o, d);
	}
}

// getSurfaceData at the first hit h of the ray (o, d): hit point, shading normal, albedo and specular coefficient of the lanes that hit
// (shadePrimary: its loop is over their objects); the others get the sky / background colour of their direction as albedo and zeros.
// What a caller does not use is not computed.
__device__ __forceinline__ void surfaceAtHit(const Params& P, const Hit& h, const V3& o, const V3& d, V3& p, V3& n, V3& albedo, float& ks)
{
	p = mk(0, 0, 0); n = mk(0, 0, 0); ks = 0;
	if (h.obj >= 0) {
		Lane s;
		s.ro = o; s.rd = d;
		shadePrimary(P, s, h);
		p = s.P; n = s.N; albedo = s.objColor; ks = s.specCoef;
	}
	else albedo = skyColor(P, d);
}

// rtx_cast_rays' hit record (rtxProbeKernel)
__device__ __forceinline__ void storeHit(const Params& P, const Hit& h, float* out)
{
	const bool hit = h.obj >= 0;
	const bool mesh = hit && P.objects[hit ? h.obj : 0].type == 3;
	out[0] = hit ? 1.f : 0.f; out[1] = hit ? (float)h.obj : -1.f; out[2] = mesh ? (float)h.tri : -1.f;
	out[3] = h.t; out[4] = hit ? h.u : -1.f; out[5] = hit ? h.v : -1.f; out[6] = 0; out[7] = 0;
}

// one 12-byte store
__device__ __forceinline__ void store3(float* out, const V3& v) { out[0] = v.x; out[1] = v.y; out[2] = v.z; }

} // namespace

// The kernels of a family for every scene kind: mesh scenes per (box test of the prune records, culling); scenes without meshes the
// walk-free form (as rtxPass1Kernel<false, false>).  After the kernel's argument list come its further template arguments, if any.
#define RTX_MESH_INSTANCES(KERNEL, ARGS, ...)                       \
template __global__ void KERNEL<true, true, 1, ##__VA_ARGS__> ARGS;    \
template __global__ void KERNEL<true, false, 1, ##__VA_ARGS__> ARGS;   \
template __global__ void KERNEL<true, true, 0, ##__VA_ARGS__> ARGS;    \
template __global__ void KERNEL<true, false, 0, ##__VA_ARGS__> ARGS;
#define RTX_QUERY_INSTANCES(KERNEL, ARGS, ...)                      \
RTX_MESH_INSTANCES(KERNEL, ARGS, ##__VA_ARGS__)                        \
template __global__ void KERNEL<false, true, -1, ##__VA_ARGS__> ARGS;

// Texts that several kernels share, as function-like macros: they expand inside a kernel's body, where P (Params), h (a Hit the traces may
// overwrite), cnt (Counts) and the template arguments MESH, BOXES and CULLK are in scope.  Macros and not __forceinline__ functions because
// every kernel has to stay the machine code it was: as functions these steps came out with other register allocations, 1 - 5 % slower
// (DESIGN.md 3.14, 3.19).

// A mesh records only t < FLT_MAX (scene.cpp:735, 740), so a range above FLT_MAX is FLT_MAX for its walk, whose bundle limit has to stay
// finite; a sphere or a plane is compared with the range itself.
#define RTX_WALK_RANGE(TM) ((TM) > kFltMax ? kFltMax : (TM))

// rtx_occluded_rays' question in its default order, for a wave: is the ray {O, D} of range TM (never NaN) open?  OPEN: in, the lanes that
// ask; out, those of them that no opaque object blocks.  The spheres and planes are asked first (a few instructions per object), the
// meshes are walked only for the lanes still open, with the source class SRC (evaluated only if some lane is) and the range TMWALK --
// RTX_WALK_RANGE(TM), as that expression or as a value the kernel computed once.
// PARK, UNPARK: statements right before and after the mesh walk, for a kernel that keeps values the walk does not read somewhere else
// meanwhile (rtx_render_light.hip); may be empty.
#define RTX_ANY_HIT(OPEN, O, D, TM, TMWALK, SRC, PARK, UNPARK)                                                    \
	if (!MESH) {                                                                                                  \
		traceWave<false, false, false, BOXES, CULLK>(P, OPEN, true, O, D, TM, h, cnt);                            \
		OPEN = OPEN && h.obj < 0;                                                                                 \
	}                                                                                                             \
	else {                                                                                                        \
		traceWave<false, false, false, BOXES, CULLK, 1>(P, OPEN, true, O, D, TM, h, cnt);                         \
		OPEN = OPEN && h.obj < 0;                                                                                 \
		if (ballot(OPEN) != 0) {                                                                                  \
			const uint32_t anyHitSrc = (SRC);                                                                     \
			PARK                                                                                                  \
			traceWave<false, true, false, BOXES, CULLK, 2>(P, OPEN, true, O, D, TMWALK, h, cnt, anyHitSrc);         \
			UNPARK                                                                                                \
			OPEN = OPEN && h.obj < 0;                                                                             \
		}                                                                                                         \
	}

// Ambient occlusion's loop over the directions (rtxAoKernel, rtxPointAoKernel): direction k comes through the scalar unit and is the same
// for all 64 lanes; a lane traces it if LIVE and it leaves the surface on the side of the normal N, from O, with the any-hit question
// above.  Declares acc = open | traced << 16.  A: the kernel's AoArgs.  Reads nDirs = uni(A.nDirs) and tmWalk = RTX_WALK_RANGE(A.radius),
// which the kernel declares once: in front of forEachRayWave's loop in rtxPointAoKernel, whose machine code differs (other registers,
// another schedule) with either inside it.
#define RTX_AO_DIRECTIONS(LIVE, O, N, A)                                                                          \
	uint32_t acc = 0;                                                                                             \
	for (uint32_t k = 0; k < nDirs; k = uni(k + 1)) {                                                             \
		const float* dk = uni(A.dirs + (size_t)k * 3);                                                            \
		const V3 d = mk(sloadf(dk), sloadf(dk + 1), sloadf(dk + 2));                                              \
		const float c = dot(N, d);                                                                                \
		const bool traced = (LIVE) && c > 0;       /* strict: a zero or NaN direction or normal is never traced */ \
		if (ballot(traced) == 0) continue;                                                                        \
		bool open = traced;                                                                                       \
		RTX_ANY_HIT(open, O, d, A.radius, tmWalk, 0u, , )                                                         \
		acc += (traced ? 0x10000u : 0u) + (open ? 1u : 0u);                                                       \
	}

// The pixel of a lane in the frame queries' plain grid (rtxAovKernel, rtxAoKernel, rtxLightFrameKernel): one 8x8 tile per wave (the pattern
// of rtxNormalsKernel's mode 0).  Declares wave, lane, W, H, tx, ty, x, y and valid -- pass 1's pixels of the rows this part owns (no halo
// rows: nothing here looks at a neighbour) -- and ends the waves beyond the grid and those without a valid pixel.
#define RTX_TILE_PIXEL()                                                                                          \
	const uint32_t wave = blockIdx.x * 4 + (threadIdx.x >> 6), lane = __lane_id();                                \
	if (wave >= P.nTiles) return;                                                                                 \
	const uint32_t W = P.view.width, H = P.view.height;                                                           \
	const uint32_t tx = wave % P.tilesX, ty = P.tileRow0 + wave / P.tilesX;                                       \
	const uint32_t x = tx * 8 + (lane & 7), y = ty * 8 + (lane >> 3);                                             \
	const bool valid = x < W - 1 && y < H - 1 && y >= P.rowBegin && y < P.rowEnd && rowOwned(P.bandH, P.nParts, P.part, y); \
	if (ballot(valid) == 0) return;

// Render::trace alone (hits only): no castRay state machine, no LDS park area, no recursion frames.  P.workCounter: this launch's queue
// head; P.nProbe rays at P.probeRays.
template <bool MESH, bool BOXES, int CULLK>
__global__ void __launch_bounds__(256) rtxRayHitKernel(const Params P, const uint32_t* order, float* hits)
{
	Counts cnt = {};
	forEachRayWave(P, order, [&](bool valid, uint32_t i, const V3& o, const V3& d) {
		Hit h;
		traceWave<false, MESH, false, BOXES, CULLK>(P, valid, false, o, d, kFltMax, h, cnt);
		if (valid) storeHit(P, h, hits + (size_t)i * 8);
	});
}
RTX_QUERY_INSTANCES(rtxRayHitKernel, (const Params, const uint32_t*, float*))

// rtx_occluded_rays (include/rtx_query.h): Render::trace of a ShadowRay whose info.tNear starts at the ray's range --
// one byte per ray, 1 iff some opaque object reports tNear < tmax.  That is "the minimum of tNear over the opaque objects < tmax", which
// depends neither on the order of the objects nor on which blocker is found first.  So the spheres and planes are asked first (a few
// instructions per object) and the meshes are walked only for the lanes still unanswered (ORDER = false); ORDER = true keeps the scene
// order (knob occluded_scene_order, for A/B runs).  A lane that is answered takes no further part (traceWave: live / consider), and an
// object no lane has a question for is not entered (its ballot).  tmax == nullptr: +inf for every ray.
// No hit record is kept or stored: of the Hit only obj >= 0 is read, so t, tri, u and v of the nearest triangle are dead outside the walk.
// The loop is forEachRayWave's, written out: inside the helper this kernel measured up to 4.6 % slower.
template <bool MESH, bool BOXES, int CULLK, bool ORDER>
__global__ void __launch_bounds__(256) rtxRayOccludedKernel(const Params P, const uint32_t* order, const float* tmax, uint8_t* occluded)
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
		const float tm = (valid && tmax) ? tmax[i] : __builtin_inff();
		// (a NaN range occludes nothing: such a lane asks no object)
		const bool asked = valid && !(tm != tm);
		bool open = asked;
		Hit h;
		if (MESH && ORDER) {
			traceWave<false, true, false, BOXES, CULLK>(P, open, true, o, d, RTX_WALK_RANGE(tm), h, cnt);
			open = open && h.obj < 0;
			// (what only the unbounded range admits: a sphere or plane at exactly FLT_MAX)
			if (ballot(open && tm > kFltMax) != 0) {
				traceWave<false, false, false, BOXES, CULLK, 1>(P, open && tm > kFltMax, true, o, d, tm, h, cnt);
				open = open && h.obj < 0;
			}
		}
		else {
			RTX_ANY_HIT(open, o, d, tm, RTX_WALK_RANGE(tm), 0u, , )
		}
		if (valid) occluded[i] = (asked && !open) ? 1 : 0;
	}
}
RTX_MESH_INSTANCES(rtxRayOccludedKernel, (const Params, const uint32_t*, const float*, uint8_t*), false)
RTX_QUERY_INSTANCES(rtxRayOccludedKernel, (const Params, const uint32_t*, const float*, uint8_t*), true)

// Render::castRay(ray, scene, 0): the pass-1 kernels' state machine (castRayWave) with CAM = false -- no ray is known to start at the
// camera.  Recursion frames: the pass-1 area of rtx_scene::frames, indexed by the global lane (the grid is at most blocksPass1).
// Mesh scenes also per PLAIN.
template <bool MESH, bool BOXES, int CULLK, bool PLAIN>
__global__ void __launch_bounds__(256, MESH ? (PLAIN ? RTX_WAVES_PLAIN : RTX_WAVES) : RTX_WAVES_ANALYTIC) rtxRayColourKernel(const Params P, const uint32_t* order, float* colours)
{
	if (!PLAIN) fillPowTab();
	const uint32_t gl = blockIdx.x * blockDim.x + threadIdx.x;
	Counts cnt = {};
	forEachRayWave(P, order, [&](bool valid, uint32_t i, const V3& o, const V3& d) {
		V3 c;
		if constexpr (PLAIN) c = castRayPlainWave<false, false, BOXES, false, CULLK>(P, valid, o, d, gl, cnt);
		else c = castRayWave<false, MESH, false, BOXES, false, CULLK, PLAIN>(P, valid, o, d, gl, cnt);
		if (valid) store3(colours + (size_t)i * 3, c);
	});
}
RTX_QUERY_INSTANCES(rtxRayColourKernel, (const Params, const uint32_t*, float*), false)
RTX_MESH_INSTANCES(rtxRayColourKernel, (const Params, const uint32_t*, float*), true)

// RTX_FLAG_SHOW_NORMALS: rtxNormalsKernel's mode 2 through the order; either output may be NULL.  (forEachRayWave's loop, written out: inside
// the helper this kernel measured about 1 % slower)
__global__ void __launch_bounds__(256) rtxRayNormalsKernel(const Params P, const uint32_t* order, float* hits, float* colours)
{
	const uint32_t lane = __lane_id();
	const uint32_t nWork = (P.nProbe + 63) / 64;
	for (;;) {
		const uint32_t work = nextWork(P.workCounter);
		if (work >= nWork) break;
		const uint32_t k = work * 64 + lane;
		const bool valid = k < P.nProbe;
		uint32_t i; V3 o, d;
		loadRay(P, order, k, valid, i, o, d);
		Hit h;
		const V3 c = normalsCast(P, valid, o, d, 0u, h);
		if (valid && hits) storeHit(P, h, hits + (size_t)i * 8);
		if (valid && colours) { float* pc = colours + (size_t)i * 3; pc[0] = c.x; pc[1] = c.y; pc[2] = c.z; }
	}
}

// The queue heads of the trace launches ([0] hits, [16] colours), the box of rtxRayBoxKernel ([32, 37) minima as ~0, [37, 42) maxima as 0)
// and its spreads ([44, 54): five doubles, 0).
__global__ void __launch_bounds__(64) rtxRayInitKernel(uint32_t* work)
{
	const uint32_t t = threadIdx.x;
	if (t < 54) work[t] = (t >= 32 && t < 37) ? ~0u : 0u;
}
