// Direct light of a frame (rtx_render_light, include/rtx_render_light.h): for every pixel of pass 1 castRay's loop
// over the lights at the first hit of its primary ray -- the diffuse and the specular sum, each light's term of both and the number of its
// shadow rays that arrive -- written as plain images, the per-light ones light-major.
//
// First half: rtxAoKernel's -- one 8x8 tile per wave over a plain grid, primaryRay (never stored), traceWave in its trace-only form with
// source class 1 (the camera's copies of the prune records), shadePrimary on the lanes that hit, of which P, N, the ray's direction and
// the object's nSpecular stay alive.  Second half: rtx_light_loop.h, the text rtxRayLightKernel includes -- a wave-uniform loop over the
// lights, every bundle the walk is handed 64 shadow rays from one 8x8 patch of surface towards one source.  No ray is stored or read,
// nothing is sorted.  No state machine, no recursion frames, no queue.
#pragma clang fp contract(off)

// RTX_LIGHT_FRAME_PARK = 1 (the default): around the mesh walk of every shadow bundle the sixteen values the walk does not read -- P, N,
// the ray's direction, nSpecular and the two sums -- wait in LDS, as castRayPlainWave's do, through the two hooks of rtx_light_loop.h:
// 90 VGPRs and five waves per SIMD instead of 102 and four.  16 KiB per block on top of the walk's 5376 B and powfRef's 512 B: 22 272 B,
// of which a CU's 160 KiB hold seven, two more than the five blocks its registers admit.  0: everything stays in registers.
// DESIGN.md 3.21 has the resource table and the timing of both forms.
#ifndef RTX_LIGHT_FRAME_PARK
#define RTX_LIGHT_FRAME_PARK 1
#endif
#if RTX_LIGHT_FRAME_PARK
namespace {
constexpr int kParkFieldsLightFrame = 16;
__device__ __forceinline__ float (*parkAreaLightFrame())[256]
{
	__shared__ float area[kParkFieldsLightFrame][256];
	return area;
}
} // namespace
#endif

template <bool MESH, bool BOXES, int CULLK>
__global__ void __launch_bounds__(256) rtxLightFrameKernel(const Params P, const rtx_frame_light_buffers out)
{
	fillPowTab();      // (powfRef's tables, in LDS; before any wave leaves: it holds the block's barrier)
	RTX_TILE_PIXEL()      // (x, y, valid, W, H)
	// (wave-uniform: what the caller asked for)
	const bool wantD = out.diffuse_dev || out.light_diffuse_dev, wantS = out.specular_dev || out.light_specular_dev;
	const bool wantOpen = out.light_open_dev != nullptr;
	Hit h;
	Counts cnt = {};
	V3 p = mk(0, 0, 0), n = mk(0, 0, 0), d;
	float ns = 0.f;
	bool hit;
	{
		V3 o;
		primaryRay(P, (float)x + 0.5f, (float)y + 0.5f, o, d);
		traceWave<false, MESH, false, BOXES, CULLK>(P, valid, false, o, d, kFltMax, h, cnt, 1u);
		hit = valid && h.obj >= 0;
		if (hit) {
			Lane s;
			s.ro = o; s.rd = d;
			shadePrimary(P, s, h);      // (only the lanes that hit are here: its loop is over their objects)
			p = s.P; n = s.N; ns = s.nSpec;
		}
	}
	// One plane of a per-light buffer; a pixel's place in every plane.  (x < W-1 and y < H-1: inside the image; li < nLights, which
	// rtx_render_light has compared with the caller's n_lights: inside the buffer.)
	const size_t plane = (size_t)W * H, i = (size_t)y * W + x;
	// the loop over the lights (declares diff and spec, the sums); after every light its terms are stored, one dword or three per lane:
	// a tile row's eight lanes write 32 or 96 consecutive bytes
#if RTX_LIGHT_FRAME_PARK
	[[maybe_unused]] float (*parked)[256] = parkAreaLightFrame();      // (not used by the walk-free instance)
	[[maybe_unused]] const uint32_t t = threadIdx.x;
#define RTX_LIGHT_LOOP_PARK \
	parked[0][t] = p.x; parked[1][t] = p.y; parked[2][t] = p.z; parked[3][t] = n.x; parked[4][t] = n.y; parked[5][t] = n.z; \
	parked[6][t] = d.x; parked[7][t] = d.y; parked[8][t] = d.z; parked[9][t] = ns; \
	parked[10][t] = diff.x; parked[11][t] = diff.y; parked[12][t] = diff.z; parked[13][t] = spec.x; parked[14][t] = spec.y; parked[15][t] = spec.z; \
	asm volatile("" ::: "memory");
#define RTX_LIGHT_LOOP_UNPARK \
	asm volatile("" ::: "memory"); \
	p = mk(parked[0][t], parked[1][t], parked[2][t]); n = mk(parked[3][t], parked[4][t], parked[5][t]); \
	d = mk(parked[6][t], parked[7][t], parked[8][t]); ns = parked[9][t]; \
	diff = mk(parked[10][t], parked[11][t], parked[12][t]); spec = mk(parked[13][t], parked[14][t], parked[15][t]);
#endif
#define RTX_LIGHT_LOOP_PER_LIGHT \
	if (valid) { \
		const size_t at = (size_t)li * plane + i; \
		if (out.light_diffuse_dev) store3(out.light_diffuse_dev + at * 3, D); \
		if (out.light_specular_dev) store3(out.light_specular_dev + at * 3, S); \
		if (out.light_open_dev) out.light_open_dev[at] = nOpen; \
	}
#include "rtx_light_loop.h"
	if (!valid) return;
	if (out.diffuse_dev) store3(out.diffuse_dev + i * 3, diff);
	if (out.specular_dev) store3(out.specular_dev + i * 3, spec);
}
RTX_QUERY_INSTANCES(rtxLightFrameKernel, (const Params, const rtx_frame_light_buffers))
