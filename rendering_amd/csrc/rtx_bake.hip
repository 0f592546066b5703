// Texel points of a mesh's UV layout and the margin fill (include/rtx_bake.h): the header's contract as four small kernels.
// Ownership takes two launches with a scan between them -- triangle sizes span six orders of magnitude, so the triangles are binned by the
// area of their clipped texel box -- and one more launch writes the outputs.  Part of rtx_api.hip's translation unit, after every other
// kernel: none of them changes.  (-ffp-contract=off is part of the build: no product below is fused with a sum.)

#include "../../include/rtx_bake.h"

// rtx_sort.hip: base[0 .. n) = the exclusive prefix sums of base[0 .. n), in place (temp == nullptr: *tempBytes = the scratch it needs)
hipError_t rtxScanChunks(void* temp, size_t* tempBytes, unsigned long long* base, uint32_t n, hipStream_t st);

namespace rtxbake {

// A lane never walks more texels than this: a triangle whose clipped box is larger goes to the chunk kernel.
constexpr uint32_t kSmallBox = 64;
constexpr uint32_t kNoOwner = 0xffffffffu;
// blocks per CU of the chunk kernel's grid (its waves share the chunks evenly, so the grid only has to fill the device)
constexpr uint32_t kChunkBlocksPerCU = 8;

__device__ __forceinline__ float texelCentre(uint32_t i, uint32_t n) { return ((float)i + 0.5f) / (float)n; }

// E(p, q, c) in fp64 over widened operands, and its canonical form
__device__ __forceinline__ double edgeRaw(float px, float py, float qx, float qy, float cx, float cy)
{
	return ((double)qx - (double)px) * ((double)cy - (double)py) - ((double)qy - (double)py) * ((double)cx - (double)px);
}
__device__ __forceinline__ double edge(float px, float py, float qx, float qy, float cx, float cy)
{
	const bool greater = px > qx || (px == qx && py > qy);
	return greater ? -edgeRaw(qx, qy, px, py, cx, cy) : edgeRaw(px, py, qx, qy, cx, cy);
}

struct TriUv { float ax, ay, bx, by, cx, cy; };
__device__ __forceinline__ TriUv loadUv(const float* __restrict__ uv, uint32_t t)
{
	const float2* p = (const float2*)(uv + (size_t)t * 6);      // (24-byte records of an allocation of their own: 8-byte aligned)
	const float2 a = p[0], b = p[1], c = p[2];
	return { a.x, a.y, b.x, b.y, c.x, c.y };
}

struct Cover { double wa, wb, wc, D; bool in; };
__device__ __forceinline__ Cover cover(const TriUv& u, float cx, float cy)
{
	Cover c;
	c.wa = edge(u.bx, u.by, u.cx, u.cy, cx, cy);
	c.wb = edge(u.cx, u.cy, u.ax, u.ay, cx, cy);
	c.wc = edge(u.ax, u.ay, u.bx, u.by, cx, cy);
	c.D = (c.wa + c.wb) + c.wc;
	const bool box = cx >= fminf(fminf(u.ax, u.bx), u.cx) && cx <= fmaxf(fmaxf(u.ax, u.bx), u.cx) &&
	                 cy >= fminf(fminf(u.ay, u.by), u.cy) && cy <= fmaxf(fmaxf(u.ay, u.by), u.cy);
	c.in = box && ((c.D > 0 && c.wa >= 0 && c.wb >= 0 && c.wc >= 0) || (c.D < 0 && c.wa <= 0 && c.wb <= 0 && c.wc <= 0));
	return c;
}

// The texels of one axis (n of them) whose centre can lie in [lo, hi]: the fp32 centre of texel i is within 3 * 2^-24 (i + 1/2) / n of
// (i + 1/2) / n, so the range is taken that much wider -- a superset; cover() decides.  count == 0: none (an empty or NaN interval too).
__device__ __forceinline__ void texelSpan(float lo, float hi, uint32_t n, uint32_t& first, uint32_t& count)
{
	first = count = 0;
	if (!(lo <= hi)) return;
	const double slack = 1e-3 + (double)n * 2e-7;
	double a = floor((double)lo * (double)n - 0.5 - slack), b = ceil((double)hi * (double)n - 0.5 + slack);
	if (a < 0) a = 0;
	if (b > (double)(n - 1)) b = (double)(n - 1);
	if (!(a <= b)) return;
	first = (uint32_t)a;
	count = (uint32_t)(b - a) + 1u;
}
struct Box { uint32_t i0, j0, bw, bh; };      // (bw * bh == 0: empty)
__device__ __forceinline__ Box texelBox(const TriUv& u, uint32_t w, uint32_t h)
{
	Box b;
	texelSpan(fminf(fminf(u.ax, u.bx), u.cx), fmaxf(fmaxf(u.ax, u.bx), u.cx), w, b.i0, b.bw);
	texelSpan(fminf(fminf(u.ay, u.by), u.cy), fmaxf(fmaxf(u.ay, u.by), u.cy), h, b.j0, b.bh);
	// (a NaN coordinate: some edge function is NaN at every centre, so the triangle covers nothing)
	if (u.ax != u.ax || u.ay != u.ay || u.bx != u.bx || u.by != u.by || u.cx != u.cx || u.cy != u.cy) b.bw = b.bh = 0;
	return b;
}

// texel (i, j) of the map (both inside it) against triangle t
__device__ __forceinline__ void claim(const TriUv& u, uint32_t t, uint32_t i, uint32_t j, uint32_t w, uint32_t h, uint32_t* __restrict__ owner)
{
	if (cover(u, texelCentre(i, w), texelCentre(j, h)).in) atomicMin(owner + (size_t)j * w + i, t);
}

// 1. One lane per triangle: a box of at most kSmallBox texels is walked here; a larger one is counted in 8 x 8-texel chunks
// (chunks[t]; 0 for the others) for the chunk kernel.  chunks[nTris] = 0: after the scan, the total.
__global__ void __launch_bounds__(256) rtxTexelBinKernel(const float* __restrict__ uv, uint32_t nTris, uint32_t w, uint32_t h, uint32_t* __restrict__ owner,
                                                           unsigned long long* __restrict__ chunks)
{
	const uint32_t t = blockIdx.x * 256u + threadIdx.x;
	if (t >= nTris) return;
	const TriUv u = loadUv(uv, t);
	const Box b = texelBox(u, w, h);
	const unsigned long long area = (unsigned long long)b.bw * b.bh;
	unsigned long long n = 0;
	if (area > kSmallBox) n = (unsigned long long)((b.bw + 7u) / 8u) * ((b.bh + 7u) / 8u);
	else
		for (uint32_t k = 0; k < (uint32_t)area; k++) claim(u, t, b.i0 + k % b.bw, b.j0 + k / b.bw, w, h, owner);
	chunks[t] = n;
	if (t == 0) chunks[nTris] = 0;
}

// 2. The chunks of the large boxes, base[t] .. base[t + 1] being triangle t's (base[nTris]: their number), shared evenly among the waves of
// the grid: wave k takes a contiguous run, one chunk at a time, one lane per texel.  The chunk's triangle is found by bisection when
// the run leaves the current one; its corner data is the same in every lane.
__global__ void __launch_bounds__(256) rtxTexelChunkKernel(const float* __restrict__ uv, uint32_t nTris, uint32_t w, uint32_t h,
                                                             const unsigned long long* __restrict__ base, uint32_t* __restrict__ owner)
{
	const unsigned long long total = base[nTris];
	const unsigned long long waves = (unsigned long long)gridDim.x * 4u, wave = (unsigned long long)blockIdx.x * 4u + (threadIdx.x >> 6);
	const unsigned long long q = total / waves, r = total % waves;
	const unsigned long long begin = wave * q + (wave < r ? wave : r), end = begin + q + (wave < r ? 1u : 0u);
	const uint32_t lane = threadIdx.x & 63u;
	uint32_t t = 0, ncx = 1;
	unsigned long long lo = 0, hi = 0;      // the chunks of triangle t: [lo, hi)
	TriUv u = { 0, 0, 0, 0, 0, 0 };
	Box b = { 0, 0, 0, 0 };
	for (unsigned long long g = begin; g < end; g++) {
		if (g >= hi) {
			// base[a] <= g < base[c] holds throughout (base[0] = 0, g < total = base[nTris]); a triangle without chunks is never the answer
			uint32_t a = 0, c = nTris;
			while (c - a > 1) {
				const uint32_t m = a + (c - a) / 2;
				if (base[m] <= g) a = m; else c = m;
			}
			t = a; lo = base[a]; hi = base[a + 1];
			u = loadUv(uv, t);
			b = texelBox(u, w, h);
			ncx = (b.bw + 7u) / 8u;
		}
		const uint32_t k = (uint32_t)(g - lo);
		const uint32_t di = (k % ncx) * 8u + (lane & 7u), dj = (k / ncx) * 8u + (lane >> 3);
		if (di < b.bw && dj < b.bh) claim(u, t, b.i0 + di, b.j0 + dj, w, h, owner);
	}
}

// 3. One lane per texel: the owner's edge functions again, the barycentrics, the surface point.  The points leave through LDS so that a
// block writes its 256 x 6 floats as one contiguous run, 16 bytes per lane where the buffer is aligned for it.
__global__ void __launch_bounds__(256) rtxTexelWriteKernel(const float* __restrict__ pos, const float* __restrict__ nrm, const float* __restrict__ uv, uint32_t w,
                                                             uint32_t h, const uint32_t* __restrict__ owner, const rtx_texel_buffers out)
{
	__shared__ __attribute__((aligned(16))) float stage[256 * 6];
	const size_t n = (size_t)w * h, first = (size_t)blockIdx.x * 256u;
	const uint32_t count = (uint32_t)(n - first < 256u ? n - first : 256u), tid = threadIdx.x;
	const size_t idx = first + tid;
	V3 P = mk(0.0f, 0.0f, 0.0f), N = P;
	float bu = 0.0f, bv = 0.0f;
	int32_t tri = -1;
	if (tid < count) {
		const uint32_t t = owner[idx];
		if (t != kNoOwner) {
			const Cover c = cover(loadUv(uv, t), texelCentre((uint32_t)(idx % w), w), texelCentre((uint32_t)(idx / w), h));
			bu = (float)(c.wb / c.D); bv = (float)(c.wc / c.D);
			tri = (int32_t)t;
			if (out.points_dev) {
				const float* p = pos + (size_t)t * 9;
				const float* m = nrm + (size_t)t * 9;
				const float k = (1.0f - bu) - bv;
				P = (mk(p[3], p[4], p[5]) * bu + mk(p[6], p[7], p[8]) * bv) + mk(p[0], p[1], p[2]) * k;
				N = normalized(((mk(m[3], m[4], m[5]) * bu + mk(m[6], m[7], m[8]) * bv) + mk(m[0], m[1], m[2]) * k) / 3.0f);
			}
		}
		if (out.tri_dev) out.tri_dev[idx] = tri;
		if (out.bary_dev) {
			if (((uintptr_t)out.bary_dev & 7u) == 0) ((float2*)out.bary_dev)[idx] = make_float2(bu, bv);
			else { out.bary_dev[idx * 2] = bu; out.bary_dev[idx * 2 + 1] = bv; }
		}
	}
	if (!out.points_dev) return;      // (the same in every thread of the grid: every thread of a block reaches the barrier)
	float* s = stage + tid * 6;
	s[0] = P.x; s[1] = P.y; s[2] = P.z; s[3] = N.x; s[4] = N.y; s[5] = N.z;
	__syncthreads();
	float* dst = out.points_dev + first * 6;      // (first * 24 bytes: a multiple of 16)
	if (count == 256u && ((uintptr_t)out.points_dev & 15u) == 0) {
		for (uint32_t k = tid; k < 256u * 6u / 4u; k += 256u) ((float4*)dst)[k] = ((const float4*)stage)[k];
	}
	else
		for (uint32_t k = tid; k < count * 6u; k += 256u) dst[k] = stage[k];
}

// One pass of the margin fill: triIn is the state at the start of the pass.  Only texels with triIn == -1 are written in `image`, only
// texels with triIn != -1 are read from it: the pass does not depend on the order of its lanes.
__global__ void __launch_bounds__(256) rtxDilateKernel(uint32_t w, uint32_t h, uint32_t channels, float* __restrict__ image, const int32_t* __restrict__ triIn,
                                                         int32_t* __restrict__ triOut)
{
	const size_t idx = (size_t)blockIdx.x * 256u + threadIdx.x;
	if (idx >= (size_t)w * h) return;
	int32_t t = triIn[idx];
	if (t == -1) {
		const int di[8] = { -1, 1, 0, 0, -1, 1, -1, 1 }, dj[8] = { 0, 0, -1, 1, -1, -1, 1, 1 };
		const long long i = (long long)(idx % w), j = (long long)(idx / w);
#pragma unroll
		for (int k = 0; k < 8; k++) {
			const long long ni = i + di[k], nj = j + dj[k];
			if (t != -1 || ni < 0 || nj < 0 || ni >= (long long)w || nj >= (long long)h) continue;
			const size_t src = (size_t)nj * w + (size_t)ni;
			if (triIn[src] == -1) continue;
			for (uint32_t c = 0; c < channels; c++) image[idx * channels + c] = image[src * channels + c];
			t = -2;
		}
	}
	triOut[idx] = t;
}

} // namespace rtxbake

extern "C" {

int rtx_texel_points(rtx_scene* s, uint32_t mesh, uint32_t w, uint32_t h, const rtx_texel_buffers* out, void* stream)
{
	RoctxRange range("Texel points (rtx_texel_points)");
	if (!s || !out) return fail(RTX_ERR_ARG, "scene/out is NULL");
	if (!out->points_dev && !out->tri_dev && !out->bary_dev) return fail(RTX_ERR_ARG, "rtx_texel_points: no output (all three buffers are NULL)");
	if (mesh >= s->meshRecs.size()) return fail(RTX_ERR_ARG, "mesh index out of range");
	if (!w || !h) return fail(RTX_ERR_ARG, "rtx_texel_points: a zero width or height");
	if ((unsigned long long)w * h > 0x7fffffffull) return fail(RTX_ERR_ARG, "rtx_texel_points: w * h is above 0x7fffffff");
	const Mesh& dm = s->meshRecs[mesh];
	const uint32_t nt = dm.nTris;
	const float* pos = mesh < s->meshTriPos.size() ? s->meshTriPos[mesh].get() : nullptr;
	if (nt && (!pos || !dm.nrm || !dm.uv)) return fail(RTX_ERR_UNSUPPORTED, "rtx_texel_points: the mesh's triangles are not on the device");
	const hipStream_t st = (hipStream_t)stream;
	const size_t n = (size_t)w * h;
	HIPCHK(hipSetDevice(s->device));
	int rc;
	if ((rc = renderOn(s, st))) return rc;
	// the scratch: only a larger map or mesh than ever before allocates (the old buffers are freed first, which waits for the device)
	HIPCHK(s->texelOwner.reserve(n));
	size_t scanBytes = 0;
	if (nt) {
		HIPCHK(s->texelChunks.reserve((size_t)nt + 1));
		HIPCHK(rtxScanChunks(nullptr, &scanBytes, s->texelChunks, nt + 1, st));
		HIPCHK(s->texelScanTemp.reserve(std::max<size_t>(scanBytes, 1)));
	}
	uint32_t* owner = s->texelOwner;
	HIPCHK(hipMemsetAsync(owner, 0xff, n * sizeof(uint32_t), st));
	if (nt) {
		hipLaunchKernelGGL(rtxbake::rtxTexelBinKernel, dim3((nt + 255u) / 256u), dim3(256), 0, st, dm.uv, nt, w, h, owner, s->texelChunks.get());
		HIPCHK(hipGetLastError());
		scanBytes = s->texelScanTemp.capacity();
		HIPCHK(rtxScanChunks(s->texelScanTemp.get(), &scanBytes, s->texelChunks, nt + 1, st));
		hipLaunchKernelGGL(rtxbake::rtxTexelChunkKernel, dim3((uint32_t)s->numCUs * rtxbake::kChunkBlocksPerCU), dim3(256), 0, st, dm.uv, nt, w, h,
		                   (const unsigned long long*)s->texelChunks.get(), owner);
		HIPCHK(hipGetLastError());
	}
	hipLaunchKernelGGL(rtxbake::rtxTexelWriteKernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, pos, dm.nrm, dm.uv, w, h, (const uint32_t*)owner, *out);
	HIPCHK(hipGetLastError());
	return RTX_OK;
}

int rtx_dilate_texels(rtx_scene* s, uint32_t w, uint32_t h, uint32_t channels, float* image_dev, int32_t* tri_dev, uint32_t passes, void* stream)
{
	RoctxRange range("Dilate texels (rtx_dilate_texels)");
	if (!s || !image_dev || !tri_dev) return fail(RTX_ERR_ARG, "scene/image/tri is NULL");
	if (channels < 1 || channels > 4) return fail(RTX_ERR_ARG, "rtx_dilate_texels: channels must be 1 .. 4");
	if (!w || !h) return fail(RTX_ERR_ARG, "rtx_dilate_texels: a zero width or height");
	if ((unsigned long long)w * h > 0x7fffffffull) return fail(RTX_ERR_ARG, "rtx_dilate_texels: w * h is above 0x7fffffff");
	if (!passes) return RTX_OK;
	const hipStream_t st = (hipStream_t)stream;
	const size_t n = (size_t)w * h;
	HIPCHK(hipSetDevice(s->device));
	int rc;
	if ((rc = renderOn(s, st))) return rc;
	HIPCHK(s->texelOwner.reserve(n));
	// the two copies of tri take turns: a pass reads one and writes every texel of the other
	int32_t* bufs[2] = { tri_dev, (int32_t*)s->texelOwner.get() };
	for (uint32_t p = 0; p < passes; p++) {
		hipLaunchKernelGGL(rtxbake::rtxDilateKernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, w, h, channels, image_dev, (const int32_t*)bufs[p & 1], bufs[(p & 1) ^ 1]);
		HIPCHK(hipGetLastError());
	}
	if (passes & 1) HIPCHK(hipMemcpyAsync(tri_dev, bufs[1], n * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
	return RTX_OK;
}

} // extern "C"
