// Replacing the texture maps and the skybox of a live scene from device memory (include/rtx_texture.h): the loader's texel
// arithmetic (rendering_amd/host/src/objects.cpp, decodeTexels) as one kernel family, and the four entry points over it.  Part of
// rtx_api.hip's translation unit, after every other kernel: none of them changes.

#include "../../include/rtx_texture.h"

namespace rtxtex {

// A rectangle of w x h texels from `src` (row r at src + r * pitch: pitch may be negative) into the map `dst` of dstW texels per row, at (x0, y0).
struct Job {
	const unsigned char* src;
	long long pitch;
	float* dst;
	uint32_t w, h, dstW, x0, y0;
};

__device__ __forceinline__ bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// One RGB8 texel as the loader keeps it for a map of KIND (objects.cpp:395-446, scene.cpp:292-311); out: 3 words, 1 for SPECULAR.
template <int KIND> __device__ __forceinline__ void decode(uint32_t r, uint32_t g, uint32_t b, uint32_t* out)
{
	const V3 c = mk((float)r / 256, (float)g / 256, (float)b / 256);
	if (KIND == RTX_TEX_SPECULAR) { out[0] = __float_as_uint((c.x + c.y + c.z) / 3.0f); return; }
	// (g == 128: -(+0) = -0 survives the normalisation; (128, 128, 0) has length 0 and stays as it is)
	const V3 v = KIND == RTX_TEX_NORMAL ? normalized(mk(c.x * 2 - 1, -(c.y * 2 - 1), c.z)) : c;
	out[0] = __float_as_uint(v.x); out[1] = __float_as_uint(v.y); out[2] = __float_as_uint(v.z);
}

// A lane takes four consecutive texels of a row.  RGB8: 12 source bytes, three dword loads where they are 4-byte aligned, bytewise at a ragged row
// end and in unaligned rows, decoded into 12 floats (4 for SPECULAR).  STORED: the floats themselves, 16 bytes at a time where aligned.  Either
// way the lane writes 48 (16) contiguous bytes next to its neighbour's, as float4 stores where the destination is 16-byte aligned -- a rectangle
// at an odd x0, or a map whose width is no multiple of four, is written float by float.  KIND selects the arithmetic; SKY runs DIFFUSE's.
template <int KIND, bool STORED> __global__ void __launch_bounds__(256) rtxTexelsKernel(const Job j)
{
	constexpr int CH = KIND == RTX_TEX_SPECULAR ? 1 : 3;
	const uint32_t groups = (j.w + 3) / 4;
	const unsigned long long item = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
	if (item >= (unsigned long long)groups * j.h) return;
	const uint32_t row = (uint32_t)(item / groups), x = (uint32_t)(item % groups) * 4u;
	const uint32_t n = min(4u, j.w - x);      // texels of this lane: 4 but at a ragged row end
	const unsigned char* src = j.src + (long long)row * j.pitch + (size_t)x * (STORED ? CH * 4 : 3);
	uint32_t out[4 * CH];
	if (STORED) {
		if (n == 4 && aligned(src, 16)) {
			const uint4* q = (const uint4*)src;
#pragma unroll
			for (int k = 0; k < CH; k++) { const uint4 v = q[k]; out[4 * k] = v.x; out[4 * k + 1] = v.y; out[4 * k + 2] = v.z; out[4 * k + 3] = v.w; }
		}
		else {
			const uint32_t* q = (const uint32_t*)src;
#pragma unroll
			for (int k = 0; k < 4 * CH; k++) out[k] = (uint32_t)k < n * CH ? q[k] : 0u;
		}
	}
	else {
		uint32_t w0 = 0, w1 = 0, w2 = 0;      // the 12 bytes, little-endian
		if (n == 4 && aligned(src, 4)) {
			const uint32_t* q = (const uint32_t*)src;
			w0 = q[0]; w1 = q[1]; w2 = q[2];
		}
		else {
#pragma unroll
			for (int k = 0; k < 12; k++) {
				const uint32_t byte = (uint32_t)k < n * 3 ? src[k] : 0u;
				if (k < 4) w0 |= byte << (8 * k); else if (k < 8) w1 |= byte << (8 * (k - 4)); else w2 |= byte << (8 * (k - 8));
			}
		}
		decode<KIND>(w0 & 255u, (w0 >> 8) & 255u, (w0 >> 16) & 255u, out);
		decode<KIND>(w0 >> 24, w1 & 255u, (w1 >> 8) & 255u, out + CH);
		decode<KIND>((w1 >> 16) & 255u, w1 >> 24, w2 & 255u, out + 2 * CH);
		decode<KIND>((w2 >> 8) & 255u, (w2 >> 16) & 255u, w2 >> 24, out + 3 * CH);
	}
	uint32_t* dst = (uint32_t*)j.dst + ((size_t)(j.y0 + row) * j.dstW + j.x0 + x) * CH;
	if (n == 4 && aligned(dst, 16)) {
		uint4* q = (uint4*)dst;
#pragma unroll
		for (int k = 0; k < CH; k++) q[k] = make_uint4(out[4 * k], out[4 * k + 1], out[4 * k + 2], out[4 * k + 3]);
	}
	else {
#pragma unroll
		for (int k = 0; k < 4 * CH; k++)
			if ((uint32_t)k < n * CH) dst[k] = out[k];
	}
}

inline uint32_t channels(int32_t kind) { return kind == RTX_TEX_SPECULAR ? 1u : 3u; }
inline size_t rowBytes(int32_t kind, const rtx_texels& t) { return (size_t)t.width * (t.format == RTX_TEXELS_STORED ? channels(kind) * 4u : 3u); }

// The checks of a rtx_texels record for a map of `kind` (every entry point).
int check(int32_t kind, const rtx_texels& t)
{
	if (t.format != RTX_TEXELS_STORED && t.format != RTX_TEXELS_RGB8) return fail(RTX_ERR_ARG, "texels: format is no RTX_TEXELS_*");
	if (!t.width || !t.height) return fail(RTX_ERR_ARG, "texels: a zero width or height");
	if (!t.data_dev) return fail(RTX_ERR_ARG, "texels: data_dev is NULL");
	const unsigned long long pitch = t.row_pitch < 0 ? 0ull - (unsigned long long)t.row_pitch : (unsigned long long)t.row_pitch;
	if (pitch < rowBytes(kind, t)) return fail(RTX_ERR_ARG, "texels: |row_pitch| is below one row");
	if (pitch > (1ull << 62) / t.height) return fail(RTX_ERR_ARG, "texels: |row_pitch| x height does not fit an address");
	if (t.format == RTX_TEXELS_STORED && (((uintptr_t)t.data_dev | pitch) & 3u)) return fail(RTX_ERR_ARG, "texels: stored texels must be 4-byte aligned, their pitch a multiple of 4");
	return RTX_OK;
}

// Queues the kernel for a checked record: the rectangle (x0, y0, t.width, t.height) lies inside the map `dst` of dstW texels per row.
int launch(int32_t kind, const rtx_texels& t, float* dst, uint32_t dstW, uint32_t x0, uint32_t y0, hipStream_t stream)
{
	const Job j{ (const unsigned char*)t.data_dev, (long long)t.row_pitch, dst, t.width, t.height, dstW, x0, y0 };
	const unsigned long long items = (unsigned long long)((t.width + 3) / 4) * t.height;
	if ((items + 255) / 256 > 0x7fffffffull) return fail(RTX_ERR_ARG, "texels: too many texels for one call");
	const dim3 grid((unsigned)((items + 255) / 256)), block(256);
	const bool stored = t.format == RTX_TEXELS_STORED;
	if (kind == RTX_TEX_SPECULAR) {
		if (stored) hipLaunchKernelGGL((rtxTexelsKernel<RTX_TEX_SPECULAR, true>), grid, block, 0, stream, j);
		else hipLaunchKernelGGL((rtxTexelsKernel<RTX_TEX_SPECULAR, false>), grid, block, 0, stream, j);
	}
	else if (stored) hipLaunchKernelGGL((rtxTexelsKernel<RTX_TEX_DIFFUSE, true>), grid, block, 0, stream, j);
	else if (kind == RTX_TEX_NORMAL) hipLaunchKernelGGL((rtxTexelsKernel<RTX_TEX_NORMAL, false>), grid, block, 0, stream, j);
	else hipLaunchKernelGGL((rtxTexelsKernel<RTX_TEX_DIFFUSE, false>), grid, block, 0, stream, j);
	HIPCHK(hipGetLastError());
	return RTX_OK;
}

// pointer and size of map `kind` in a mesh record
struct MapRef { const float** p; uint32_t* w; uint32_t* h; };
MapRef mapOf(Mesh& m, int32_t kind)
{
	if (kind == RTX_TEX_DIFFUSE) return { &m.diffuse, &m.dW, &m.dH };
	if (kind == RTX_TEX_NORMAL) return { &m.normal, &m.nW, &m.nH };
	return { &m.specular, &m.sW, &m.sH };
}

} // namespace rtxtex

extern "C" {

int rtx_scene_set_map(rtx_scene* s, uint32_t mesh, int32_t kind, const rtx_texels* t, void* stream)
{
	if (!s) return fail(RTX_ERR_ARG, "scene is NULL");
	if (mesh >= s->meshRecs.size()) return fail(RTX_ERR_ARG, "mesh index out of range");
	if (kind == RTX_TEX_SKY) return fail(RTX_ERR_ARG, "rtx_scene_set_map: the skybox is rtx_scene_set_sky's");
	if (kind < RTX_TEX_DIFFUSE || kind > RTX_TEX_SPECULAR) return fail(RTX_ERR_ARG, "kind is no RTX_TEX_*");
	int rc;
	if (t && (rc = rtxtex::check(kind, *t))) return rc;
	if (t && kind == RTX_TEX_NORMAL && !s->meshRecs[mesh].tb) return fail(RTX_ERR_ARG, "normal map without tangents");
	if ((rc = editBegin(s, stream))) return rc;
	Mesh dm = s->meshRecs[mesh];
	const rtxtex::MapRef ref = rtxtex::mapOf(dm, kind);
	const float* old = *ref.p;
	DevBag& bag = s->meshFixed[mesh];
	float* fresh = nullptr;
	if (t) {
		// the new map beside the old one until everything that can fail has been done
		HIPCHK(bag.alloc(&fresh, (size_t)t->width * t->height * rtxtex::channels(kind) * sizeof(float)));
		if ((rc = rtxtex::launch(kind, *t, fresh, t->width, 0, 0, nullptr)) || hipStreamSynchronize(nullptr) != hipSuccess) {
			bag.drop(fresh);
			return rc ? rc : fail(RTX_ERR_DEVICE, "rtx_scene_set_map: the texels could not be decoded");
		}
	}
	*ref.p = fresh; *ref.w = t ? t->width : 0u; *ref.h = t ? t->height : 0u;
	if (hipMemcpy((Mesh*)s->params.meshes + mesh, &dm, sizeof(Mesh), hipMemcpyHostToDevice) != hipSuccess) {
		bag.drop(fresh);
		return fail(RTX_ERR_DEVICE, "rtx_scene_set_map: the record could not be uploaded");
	}
	bag.drop(old);      // (nothing queued reads it: editBegin)
	s->meshRecs[mesh] = dm;
	s->lastFused.valid = false;
	return RTX_OK;
}

int rtx_scene_set_sky(rtx_scene* s, const rtx_texels faces[6], void* stream)
{
	if (!s) return fail(RTX_ERR_ARG, "scene is NULL");
	int rc;
	if (!faces) {
		if (s->params.view.flags & RTX_FLAG_SKYBOX) return fail(RTX_ERR_ARG, "rtx_scene_set_sky: the current view has RTX_FLAG_SKYBOX set");
	}
	else
		for (int k = 0; k < 6; k++) {
			if ((rc = rtxtex::check(RTX_TEX_SKY, faces[k]))) return rc;
			if (faces[k].width != faces[0].width || faces[k].height != faces[0].height || faces[k].format != faces[0].format)
				return fail(RTX_ERR_ARG, "rtx_scene_set_sky: the six faces must share one size and one format");
		}
	if ((rc = editBegin(s, stream))) return rc;
	const float* fresh[6] = { nullptr, nullptr, nullptr, nullptr, nullptr, nullptr };
	const float* const* table = nullptr;
	auto dropFresh = [&]() { for (int k = 0; k < 6; k++) s->owned.drop(fresh[k]); s->owned.drop(table); };
	if (faces) {
		bool ok = true;
		for (int k = 0; k < 6 && ok; k++) {
			float* f = nullptr;
			ok = s->owned.alloc(&f, (size_t)faces[k].width * faces[k].height * 3 * sizeof(float)) == hipSuccess;
			fresh[k] = f;
			ok = ok && rtxtex::launch(RTX_TEX_SKY, faces[k], f, faces[k].width, 0, 0, nullptr) == RTX_OK;
		}
		ok = ok && hipStreamSynchronize(nullptr) == hipSuccess && s->owned.upload(fresh, 6, &table) == hipSuccess;
		if (!ok) { dropFresh(); return fail(RTX_ERR_DEVICE, "rtx_scene_set_sky: the faces could not be allocated or decoded"); }
	}
	// the old faces and their table (nothing queued reads them: editBegin)
	for (int k = 0; k < 6; k++) { s->owned.drop(s->skyFaces[k]); s->skyFaces[k] = fresh[k]; }
	s->owned.drop(s->params.sky);
	s->params.sky = table;
	s->params.skyW = faces ? faces[0].width : 0u; s->params.skyH = faces ? faces[0].height : 0u;
	s->lastFused.valid = false;
	return RTX_OK;
}

int rtx_scene_texture_info(rtx_scene* s, int32_t kind, uint32_t index, uint32_t* width, uint32_t* height, const float** texels_dev)
{
	if (!s) return fail(RTX_ERR_ARG, "scene is NULL");
	if (kind < RTX_TEX_DIFFUSE || kind > RTX_TEX_SKY) return fail(RTX_ERR_ARG, "kind is no RTX_TEX_*");
	if (index >= (kind == RTX_TEX_SKY ? (size_t)6 : s->meshRecs.size())) return fail(RTX_ERR_ARG, kind == RTX_TEX_SKY ? "sky face out of range" : "mesh index out of range");
	const float* p; uint32_t w, h;
	if (kind == RTX_TEX_SKY) { p = s->params.sky ? s->skyFaces[index] : nullptr; w = s->params.skyW; h = s->params.skyH; }
	else {
		Mesh dm = s->meshRecs[index];
		const rtxtex::MapRef ref = rtxtex::mapOf(dm, kind);
		p = *ref.p; w = *ref.w; h = *ref.h;
	}
	if (!p) w = h = 0;
	if (width) *width = w;
	if (height) *height = h;
	if (texels_dev) *texels_dev = p;
	return RTX_OK;
}

int rtx_scene_write_texels(rtx_scene* s, int32_t kind, uint32_t index, uint32_t x0, uint32_t y0, const rtx_texels* t, void* stream)
{
	if (!s || !t) return fail(RTX_ERR_ARG, "scene/texels is NULL");
	uint32_t w = 0, h = 0;
	const float* dst = nullptr;
	int rc;
	if ((rc = rtx_scene_texture_info(s, kind, index, &w, &h, &dst))) return rc;
	if (!dst) return fail(RTX_ERR_ARG, "rtx_scene_write_texels: there is no such map");
	if ((rc = rtxtex::check(kind, *t))) return rc;
	if (x0 >= w || y0 >= h || t->width > w - x0 || t->height > h - y0) return fail(RTX_ERR_ARG, "rtx_scene_write_texels: the rectangle does not lie inside the map");
	HIPCHK(hipSetDevice(s->device));
	return rtxtex::launch(kind, *t, (float*)dst, w, x0, y0, (hipStream_t)stream);
}

} // extern "C"
