// Deforming a mesh of a live scene from vertices in device memory (include/rtx_deform.h): the loader's placement and triangle
// assembly (rtx_place.h: Mesh::place restated) as three small kernels, whose triangles go the way rtx_scene_update_mesh goes (rtx_edit.hip).
// Part of rtx_api.hip's translation unit, after every other kernel: none of them changes.

#include "../../include/rtx_deform.h"
#include "rtx_place.h"

namespace rtxdeform {

// the topology in device memory
struct TopoDev {
	uint32_t nTris = 0, nPos = 0, nNrm = 0, nUv = 0, placedPos = 0, placedNrm = 0;
	const uint32_t* cornerPos = nullptr;
	const int32_t* cornerNrm = nullptr;
	const int32_t* cornerUv = nullptr;
	const float* uv = nullptr;
	const float* nrm = nullptr;
};

// The words the kernels report through: [0, 3) the box's lo and [3, 6) its hi, as unsigned numbers ordered like the floats (ordKey), [6] some input
// is not finite, [7] some placed position is not finite.
constexpr int kWords = 8;
__host__ __device__ inline uint32_t ordKey(float v)
{
	uint32_t u;
	memcpy(&u, &v, 4);
	return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
inline float ordValue(uint32_t k)
{
	const uint32_t u = (k & 0x80000000u) ? k ^ 0x80000000u : ~k;
	float v;
	memcpy(&v, &u, 4);
	return v;
}

// 1. The running min and max of the first placedPos vertices (from FLT_MAX and FLT_MIN: the words start there) and the finite check of every
// input.  A parallel reduction gives the loader's sequential values for finite input but for the sign of a zero minimum (-0 wins here wherever it
// stands; on the host the zero read last), which cannot reach a placed vertex: rtx_place.h, placeVertex.  One item per vertex or normal: a lane
// reads 12 bytes next to its neighbour's.
__global__ void __launch_bounds__(256) rtxDeformBoxKernel(const float* __restrict__ pos, uint32_t nPos, uint32_t placedPos, const float* __restrict__ nrm, uint32_t nNrm,
                                                            uint32_t* __restrict__ words)
{
	float lo[3] = { rtxplace::kFltMax, rtxplace::kFltMax, rtxplace::kFltMax }, hi[3] = { rtxplace::kFltMin, rtxplace::kFltMin, rtxplace::kFltMin };
	bool bad = false;
	const size_t n = (size_t)nPos + nNrm, step = (size_t)gridDim.x * blockDim.x;
	for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
		const float* p = i < nPos ? pos + i * 3 : nrm + (i - nPos) * 3;
		const float v[3] = { p[0], p[1], p[2] };
		bad |= !rtxplace::finiteBits(v[0]) || !rtxplace::finiteBits(v[1]) || !rtxplace::finiteBits(v[2]);
		if (i < placedPos)
			for (int k = 0; k < 3; k++) { lo[k] = rtxplace::minRef(v[k], lo[k]); hi[k] = rtxplace::maxRef(v[k], hi[k]); }
	}
	uint32_t klo[3], khi[3];
	for (int k = 0; k < 3; k++) { klo[k] = ordKey(lo[k]); khi[k] = ordKey(hi[k]); }
	for (int off = 32; off > 0; off >>= 1)
		for (int k = 0; k < 3; k++) {
			klo[k] = min(klo[k], (uint32_t)__shfl_xor((int)klo[k], off));
			khi[k] = max(khi[k], (uint32_t)__shfl_xor((int)khi[k], off));
		}
	const bool anyBad = __any(bad);
	if ((threadIdx.x & 63) == 0) {
		for (int k = 0; k < 3; k++) { atomicMin(words + k, klo[k]); atomicMax(words + 3 + k, khi[k]); }
		if (anyBad) atomicOr(words + 6, 1u);
	}
}

// 2. Placement: items [0, nPos) are the vertices (the first placedPos placed, the others as given), items [nPos, nPos + nNrm) the normals
// (normalised when they are the caller's raw ones, the first placedNrm rotated), into placed[(nPos + nNrm) x 3].
__global__ void __launch_bounds__(256) rtxDeformPlaceKernel(const rtxplace::Fit f, const float* __restrict__ pos, uint32_t nPos, uint32_t placedPos,
                                                              const float* __restrict__ nrm, uint32_t nNrm, uint32_t placedNrm, int normalise,
                                                              float* __restrict__ placed, uint32_t* __restrict__ words)
{
	const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= (size_t)nPos + nNrm) return;
	float v[3];
	if (i < nPos) {
		const float* p = pos + i * 3;
		v[0] = p[0]; v[1] = p[1]; v[2] = p[2];
		if (i < placedPos) rtxplace::placeVertex(f, v);
		if (!rtxplace::finiteBits(v[0]) || !rtxplace::finiteBits(v[1]) || !rtxplace::finiteBits(v[2])) atomicOr(words + 7, 1u);
	}
	else {
		const size_t j = i - nPos;
		const float* p = nrm + j * 3;
		v[0] = p[0]; v[1] = p[1]; v[2] = p[2];
		if (normalise) {
			// Vec3::normalize through its fp64 factor: the device's exact one (rtx_math.h, normalized)
			const V3 u = normalized(mk(v[0], v[1], v[2]));
			v[0] = u.x; v[1] = u.y; v[2] = u.z;
		}
		if (j < placedNrm) rtxplace::rotateNormal(f, v);
	}
	float* o = placed + i * 3;
	o[0] = v[0]; o[1] = v[1]; o[2] = v[2];
}

// 3. Assembly: one triangle per lane (its corners are gathered by index, which no split makes contiguous), its 24 floats staged through LDS so
// that the block writes its 256 x 9, 256 x 9 and 256 x 6 floats as three contiguous runs, a lane next to its neighbour, instead of 36-byte
// strides per lane.  triTb == nullptr: the mesh was created without tangents.
__global__ void __launch_bounds__(256) rtxDeformAssembleKernel(const TopoDev t, const float* __restrict__ placedP, const float* __restrict__ placedN,
                                                                 float* __restrict__ triPos, float* __restrict__ triNrm, float* __restrict__ triTb)
{
	__shared__ float stage[256 * 9];
	const uint32_t base = blockIdx.x * 256u;
	const uint32_t count = min(256u, t.nTris - base);
	const uint32_t tid = threadIdx.x;
	float pos9[9], nrm9[9], tb6[6];
	if (tid < count) {
		const size_t c = ((size_t)base + tid) * 3;
		const uint32_t v0 = t.cornerPos[c], v1 = t.cornerPos[c + 1], v2 = t.cornerPos[c + 2];
		const int32_t n0 = t.cornerNrm[c], n1 = t.cornerNrm[c + 1], n2 = t.cornerNrm[c + 2];
		const int32_t u0 = t.cornerUv[c], u1 = t.cornerUv[c + 1], u2 = t.cornerUv[c + 2];
		const bool hasN = n0 >= 0, hasT = hasN && u0 >= 0;
		float a[3], b[3], cc[3], na[3] = { 0, 0, 0 }, nb[3] = { 0, 0, 0 }, nc[3] = { 0, 0, 0 }, ta[2] = { 0, 0 }, tb[2] = { 0, 0 }, tc[2] = { 0, 0 };
		for (int k = 0; k < 3; k++) { a[k] = placedP[(size_t)v0 * 3 + k]; b[k] = placedP[(size_t)v1 * 3 + k]; cc[k] = placedP[(size_t)v2 * 3 + k]; }
		if (hasN)
			for (int k = 0; k < 3; k++) { na[k] = placedN[(size_t)n0 * 3 + k]; nb[k] = placedN[(size_t)n1 * 3 + k]; nc[k] = placedN[(size_t)n2 * 3 + k]; }
		if (hasT)
			for (int k = 0; k < 2; k++) { ta[k] = t.uv[(size_t)u0 * 2 + k]; tb[k] = t.uv[(size_t)u1 * 2 + k]; tc[k] = t.uv[(size_t)u2 * 2 + k]; }
		rtxplace::assemble(a, b, cc, hasN, na, nb, nc, hasT, ta, tb, tc, pos9, nrm9, tb6);
	}
	// (every thread of the block reaches every barrier)
	if (tid < count)
		for (int k = 0; k < 9; k++) stage[tid * 9 + k] = pos9[k];
	__syncthreads();
	for (uint32_t k = tid; k < count * 9; k += 256) triPos[(size_t)base * 9 + k] = stage[k];
	__syncthreads();
	if (tid < count)
		for (int k = 0; k < 9; k++) stage[tid * 9 + k] = nrm9[k];
	__syncthreads();
	for (uint32_t k = tid; k < count * 9; k += 256) triNrm[(size_t)base * 9 + k] = stage[k];
	if (!triTb) return;
	__syncthreads();
	if (tid < count)
		for (int k = 0; k < 6; k++) stage[tid * 6 + k] = tb6[k];
	__syncthreads();
	for (uint32_t k = tid; k < count * 6; k += 256) triTb[(size_t)base * 6 + k] = stage[k];
}

// the buffers of a run: the reported words, the placed vertices and normals, the triangles (grown, never shrunk)
struct Scratch {
	DevArray<uint32_t> words;
	DevArray<float> placed, tris;
};

// Checks of a topology given in host memory (what keeps every gather of the assembly kernel inside its arrays)
int checkTopology(const rtx_mesh_topology& t)
{
	if (t.placed_pos > t.n_pos || t.placed_nrm > t.n_nrm) return fail(RTX_ERR_ARG, "mesh topology: placed_pos / placed_nrm above n_pos / n_nrm");
	if (t.n_tris && (!t.corner_pos || !t.corner_nrm || !t.corner_uv)) return fail(RTX_ERR_ARG, "mesh topology: corner arrays missing");
	if ((t.n_uv && !t.uv) || (t.n_nrm && !t.nrm)) return fail(RTX_ERR_ARG, "mesh topology: uv / nrm missing");
	if (t.n_tris > 0x55555555u / 3 || t.n_pos > 0x55555555u || t.n_nrm > 0x55555555u) return fail(RTX_ERR_ARG, "mesh topology: too large");
	for (size_t i = 0; i < (size_t)t.n_uv * 2; i++)
		if (!rtxplace::finiteBits(t.uv[i])) return fail(RTX_ERR_ARG, "mesh topology: a uv is not finite");
	for (size_t i = 0; i < (size_t)t.n_nrm * 3; i++)
		if (!rtxplace::finiteBits(t.nrm[i])) return fail(RTX_ERR_ARG, "mesh topology: a stored normal is not finite");
	for (size_t i = 0; i < t.n_tris; i++) {
		const uint32_t* v = t.corner_pos + i * 3;
		const int32_t* n = t.corner_nrm + i * 3;
		const int32_t* u = t.corner_uv + i * 3;
		if (v[0] >= t.n_pos || v[1] >= t.n_pos || v[2] >= t.n_pos) return fail(RTX_ERR_ARG, "mesh topology: a position index is out of range");
		if (n[0] < 0) continue;
		for (int k = 0; k < 3; k++)
			if (n[k] < 0 || (uint32_t)n[k] >= t.n_nrm) return fail(RTX_ERR_ARG, "mesh topology: a normal index is out of range");
		if (u[0] < 0) continue;
		for (int k = 0; k < 3; k++)
			if (u[k] < 0 || (uint32_t)u[k] >= t.n_uv) return fail(RTX_ERR_ARG, "mesh topology: a uv index is out of range");
	}
	return RTX_OK;
}

// a checked topology into device memory (allocations of `bag`, not counted as scene data)
int uploadTopology(const rtx_mesh_topology& t, DevBag& bag, TopoDev& d)
{
	d = TopoDev();
	d.nTris = t.n_tris; d.nPos = t.n_pos; d.nNrm = t.n_nrm; d.nUv = t.n_uv; d.placedPos = t.placed_pos; d.placedNrm = t.placed_nrm;
	auto up = [&](const void* src, size_t bytes, const void** out) -> hipError_t {
		*out = nullptr;
		if (!bytes) return hipSuccess;
		char* p = nullptr;
		hipError_t e = bag.alloc(&p, bytes, false);
		if (e == hipSuccess) e = hipMemcpy(p, src, bytes, hipMemcpyHostToDevice);
		*out = p;
		return e;
	};
	HIPCHK(up(t.corner_pos, (size_t)t.n_tris * 12, (const void**)&d.cornerPos));
	HIPCHK(up(t.corner_nrm, (size_t)t.n_tris * 12, (const void**)&d.cornerNrm));
	HIPCHK(up(t.corner_uv, (size_t)t.n_tris * 12, (const void**)&d.cornerUv));
	HIPCHK(up(t.uv, (size_t)t.n_uv * 8, (const void**)&d.uv));
	HIPCHK(up(t.nrm, (size_t)t.n_nrm * 12, (const void**)&d.nrm));
	return RTX_OK;
}

// The three kernels on the null stream of the current device, with their two read-backs: the box and the input flag (28 bytes) before the
// fit, which the host does; the placed flag after the assembly.  loHi12: the vertices' box lo, hi, the root box lo, hi.  flags2 as
// rtx_place_probe reports them; after flags2[0] nothing else has run.  The triangles are in sc.tris: nTris x 9, nTris x 9, nTris x 6 (withTb).
int run(const TopoDev& t, const float* posDev, const float* nrmDev, const rtx_mesh_pose& pose, bool withTb, Scratch& sc, float loHi12[12], uint32_t flags2[2])
{
	HIPCHK(sc.words.reserve(kWords));
	HIPCHK(sc.placed.reserve(std::max<size_t>(1, ((size_t)t.nPos + t.nNrm) * 3)));
	HIPCHK(sc.tris.reserve(std::max<size_t>(1, (size_t)t.nTris * 24)));
	uint32_t w[kWords] = { 0 };
	for (int k = 0; k < 3; k++) { w[k] = ordKey(rtxplace::kFltMax); w[3 + k] = ordKey(rtxplace::kFltMin); }
	HIPCHK(hipMemcpy(sc.words, w, sizeof(w), hipMemcpyHostToDevice));
	const size_t nIn = (size_t)t.nPos + (nrmDev ? t.nNrm : 0);
	if (nIn) {
		const unsigned blocks = (unsigned)std::min<size_t>((nIn + 255) / 256, 1024);
		hipLaunchKernelGGL(rtxDeformBoxKernel, dim3(blocks), dim3(256), 0, nullptr, posDev, t.nPos, t.placedPos, nrmDev, nrmDev ? t.nNrm : 0u, sc.words.get());
		HIPCHK(hipGetLastError());
	}
	HIPCHK(hipMemcpy(w, sc.words, 7 * sizeof(uint32_t), hipMemcpyDeviceToHost));
	flags2[0] = w[6]; flags2[1] = 0;
	float lo[3], hi[3];
	for (int k = 0; k < 3; k++) { lo[k] = ordValue(w[k]); hi[k] = ordValue(w[3 + k]); }
	memcpy(loHi12, lo, 12); memcpy(loHi12 + 3, hi, 12);
	if (flags2[0]) return RTX_OK;
	rtxplace::Fit f;
	rtxplace::fit(lo, hi, pose.size, pose.bias, pose.rot_matrix, pose.pos, f);
	memcpy(loHi12 + 6, f.rootLo, 12); memcpy(loHi12 + 9, f.rootHi, 12);
	const size_t nItems = (size_t)t.nPos + t.nNrm;
	if (nItems) {
		hipLaunchKernelGGL(rtxDeformPlaceKernel, dim3((unsigned)((nItems + 255) / 256)), dim3(256), 0, nullptr, f, posDev, t.nPos, t.placedPos,
		                   nrmDev ? nrmDev : t.nrm, t.nNrm, t.placedNrm, nrmDev ? 1 : 0, sc.placed.get(), sc.words.get());
		HIPCHK(hipGetLastError());
	}
	if (t.nTris) {
		float* tris = sc.tris;
		hipLaunchKernelGGL(rtxDeformAssembleKernel, dim3((t.nTris + 255) / 256), dim3(256), 0, nullptr, t, (const float*)sc.placed.get(),
		                   (const float*)(sc.placed.get() + (size_t)t.nPos * 3), tris, tris + (size_t)t.nTris * 9, withTb ? tris + (size_t)t.nTris * 18 : nullptr);
		HIPCHK(hipGetLastError());
	}
	HIPCHK(hipMemcpy(&flags2[1], sc.words.get() + 7, sizeof(uint32_t), hipMemcpyDeviceToHost));
	return RTX_OK;
}

// The same on the CPU (rtx_place_probe with device < 0): the box by the loader's sequential rule, then the functions of rtx_place.h.
void runHost(const rtx_mesh_topology& t, const float* pos, const float* nrm, const rtx_mesh_pose& pose, float* tri24, float loHi12[12], uint32_t flags2[2])
{
	flags2[0] = flags2[1] = 0;
	for (size_t i = 0; i < (size_t)t.n_pos * 3; i++) if (!rtxplace::finiteBits(pos[i])) flags2[0] = 1;
	for (size_t i = 0; nrm && i < (size_t)t.n_nrm * 3; i++) if (!rtxplace::finiteBits(nrm[i])) flags2[0] = 1;
	float lo[3] = { rtxplace::kFltMax, rtxplace::kFltMax, rtxplace::kFltMax }, hi[3] = { rtxplace::kFltMin, rtxplace::kFltMin, rtxplace::kFltMin };
	for (size_t i = 0; i < t.placed_pos && !flags2[0]; i++)
		for (int k = 0; k < 3; k++) { lo[k] = rtxplace::minRef(pos[i * 3 + k], lo[k]); hi[k] = rtxplace::maxRef(pos[i * 3 + k], hi[k]); }
	memcpy(loHi12, lo, 12); memcpy(loHi12 + 3, hi, 12);
	if (flags2[0]) return;
	rtxplace::Fit f;
	rtxplace::fit(lo, hi, pose.size, pose.bias, pose.rot_matrix, pose.pos, f);
	memcpy(loHi12 + 6, f.rootLo, 12); memcpy(loHi12 + 9, f.rootHi, 12);
	std::vector<float> P(pos, pos + (size_t)t.n_pos * 3), N((size_t)t.n_nrm * 3);
	for (size_t i = 0; i < t.n_pos; i++) {
		if (i < t.placed_pos) rtxplace::placeVertex(f, &P[i * 3]);
		if (!rtxplace::finiteBits(P[i * 3]) || !rtxplace::finiteBits(P[i * 3 + 1]) || !rtxplace::finiteBits(P[i * 3 + 2])) flags2[1] = 1;
	}
	for (size_t j = 0; j < t.n_nrm; j++) {
		float* n = &N[j * 3];
		const float* src = (nrm ? nrm : t.nrm) + j * 3;
		n[0] = src[0]; n[1] = src[1]; n[2] = src[2];
		if (nrm) {
			// Vec3::normalize (geometry.h)
			const float l2 = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
			if (l2 > 0) { const float fac = (float)(1 / std::sqrt((double)l2)); n[0] *= fac; n[1] *= fac; n[2] *= fac; }
		}
		if (j < t.placed_nrm) rtxplace::rotateNormal(f, n);
	}
	const size_t nt = t.n_tris;
	const float zero[3] = { 0, 0, 0 };
	for (size_t i = 0; i < nt; i++) {
		const uint32_t* v = t.corner_pos + i * 3;
		const int32_t* n = t.corner_nrm + i * 3;
		const int32_t* u = t.corner_uv + i * 3;
		const bool hasN = n[0] >= 0, hasT = hasN && u[0] >= 0;
		rtxplace::assemble(&P[(size_t)v[0] * 3], &P[(size_t)v[1] * 3], &P[(size_t)v[2] * 3], hasN, hasN ? &N[(size_t)n[0] * 3] : zero, hasN ? &N[(size_t)n[1] * 3] : zero,
		                   hasN ? &N[(size_t)n[2] * 3] : zero, hasT, hasT ? t.uv + (size_t)u[0] * 2 : zero, hasT ? t.uv + (size_t)u[1] * 2 : zero,
		                   hasT ? t.uv + (size_t)u[2] * 2 : zero, tri24 + i * 9, tri24 + nt * 9 + i * 9, tri24 + nt * 18 + i * 6);
	}
}

} // namespace rtxdeform

// what a scene keeps per mesh for rtx_scene_deform_mesh (rtx_scene::meshDeform: moved with a kept mesh by rtx_scene_set_objects, freed with the others)
struct rtx_scene_mesh_deform {
	bool set = false;
	rtxdeform::TopoDev topo;
	DevBag bag;
	rtxdeform::Scratch scratch;
};

extern "C" {

int rtx_scene_set_mesh_topology(rtx_scene* s, uint32_t mesh, const rtx_mesh_topology* t)
{
	if (!s || !t) return fail(RTX_ERR_ARG, "scene/topology is NULL");
	if (mesh >= s->meshRecs.size()) return fail(RTX_ERR_ARG, "mesh index out of range");
	if (t->n_tris != s->meshRecs[mesh].nTris) return fail(RTX_ERR_ARG, "rtx_scene_set_mesh_topology: n_tris is not the mesh's own count");
	int rc;
	if ((rc = rtxdeform::checkTopology(*t))) return rc;
	HIPCHK(hipSetDevice(s->device));
	auto fresh = std::make_shared<rtx_scene_mesh_deform>();
	if ((rc = rtxdeform::uploadTopology(*t, fresh->bag, fresh->topo))) return rc;
	fresh->set = true;
	// (a launch that read the old arrays has finished: rtx_scene_deform_mesh waits for its kernels)
	s->meshDeform.resize(s->meshRecs.size());
	s->meshDeform[mesh] = std::move(fresh);
	return RTX_OK;
}

int rtx_scene_deform_mesh(rtx_scene* s, uint32_t mesh, const float* pos_dev, uint32_t n_pos, const float* nrm_dev, uint32_t n_nrm, const rtx_mesh_pose* pose,
                          float obj_lo[3], float obj_hi[3], void* stream)
{
	if (!s || !pose) return fail(RTX_ERR_ARG, "scene/pose is NULL");
	if (mesh >= s->meshRecs.size()) return fail(RTX_ERR_ARG, "mesh index out of range");
	if (mesh >= s->meshDeform.size() || !s->meshDeform[mesh] || !s->meshDeform[mesh]->set)
		return fail(RTX_ERR_ARG, "rtx_scene_deform_mesh: the mesh has no topology (rtx_scene_set_mesh_topology)");
	rtx_scene_mesh_deform& d = *s->meshDeform[mesh];
	const Mesh& old = s->meshRecs[mesh];
	if (d.topo.nTris != old.nTris) return fail(RTX_ERR_ARG, "rtx_scene_deform_mesh: the topology's n_tris is not the mesh's count");
	if (n_pos != d.topo.nPos) return fail(RTX_ERR_ARG, "rtx_scene_deform_mesh: n_pos is not the topology's count");
	if (nrm_dev && n_nrm != d.topo.nNrm) return fail(RTX_ERR_ARG, "rtx_scene_deform_mesh: n_nrm is not the topology's count");
	if (n_pos && !pos_dev) return fail(RTX_ERR_ARG, "rtx_scene_deform_mesh: pos_dev is NULL");
	if (!old.nTris) return fail(RTX_ERR_ARG, "rtx_scene_deform_mesh: a mesh without triangles");
	for (int k = 0; k < 16; k++)
		if (!rtxplace::finiteBits(pose->rot_matrix[k])) return fail(RTX_ERR_ARG, "rtx_scene_deform_mesh: the pose is not finite");
	for (int k = 0; k < 3; k++)
		if (!rtxplace::finiteBits(pose->pos[k]) || !rtxplace::finiteBits(pose->size[k])) return fail(RTX_ERR_ARG, "rtx_scene_deform_mesh: the pose is not finite");
	int rc;
	if ((rc = editBegin(s, stream))) return rc;
	float loHi[12];
	uint32_t flags[2] = { 0, 0 };
	const bool withTb = old.tb != nullptr;
	if ((rc = rtxdeform::run(d.topo, pos_dev, nrm_dev, *pose, withTb, d.scratch, loHi, flags))) return rc;
	if (flags[0]) return fail(RTX_ERR_ARG, "rtx_scene_deform_mesh: a vertex or a normal is not finite");
	if (flags[1]) return fail(RTX_ERR_ARG, "rtx_scene_deform_mesh: a placed position is not finite (a flat axis away from zero)");
	// nothing of the scene has been touched so far; from here the mesh goes rtx_scene_update_mesh's way
	const float* tris = d.scratch.tris;
	const size_t nt = old.nTris;
	if ((rc = rtx_scene_update_mesh(s, mesh, tris, tris + nt * 9, withTb ? tris + nt * 18 : nullptr, loHi + 6, loHi + 9, pose->ac_penalty, nullptr))) return rc;
	if (obj_lo) memcpy(obj_lo, loHi, 12);
	if (obj_hi) memcpy(obj_hi, loHi + 3, 12);
	return RTX_OK;
}

int rtx_place_probe(int device, const rtx_mesh_topology* t, const float* pos, const float* nrm, const rtx_mesh_pose* pose, float* tri24_out, float* lo_hi_out,
                    uint32_t* flags_out)
{
	if (!t || !pose || !tri24_out || !lo_hi_out || !flags_out || (t->n_pos && !pos)) return fail(RTX_ERR_ARG, "bad argument");
	int rc;
	if ((rc = rtxdeform::checkTopology(*t))) return rc;
	memset(tri24_out, 0, (size_t)t->n_tris * 24 * sizeof(float));
	memset(lo_hi_out, 0, 12 * sizeof(float));
	if (device < 0) { rtxdeform::runHost(*t, pos, nrm, *pose, tri24_out, lo_hi_out, flags_out); return RTX_OK; }
	int cnt = 0;
	if (hipGetDeviceCount(&cnt) != hipSuccess || cnt <= 0) return fail(RTX_ERR_NO_DEVICE, "no HIP device visible");
	HIPCHK(hipSetDevice(device));
	DevBag bag;
	rtxdeform::TopoDev d;
	rtxdeform::Scratch sc;
	if ((rc = rtxdeform::uploadTopology(*t, bag, d))) return rc;
	const float* posDev = nullptr;
	const float* nrmDev = nullptr;
	HIPCHK(bag.upload(pos, (size_t)t->n_pos * 3, &posDev));
	if (nrm) HIPCHK(bag.upload(nrm, (size_t)t->n_nrm * 3, &nrmDev));
	if (nrm && !nrmDev) { float* one = nullptr; HIPCHK(bag.alloc(&one, 16)); nrmDev = one; }      // (no normals at all: "given" all the same)
	HIPCHK(hipDeviceSynchronize());
	if ((rc = rtxdeform::run(d, posDev, nrmDev, *pose, true, sc, lo_hi_out, flags_out))) return rc;
	if (flags_out[0] || !t->n_tris) return RTX_OK;
	HIPCHK(hipMemcpy(tri24_out, sc.tris, (size_t)t->n_tris * 24 * sizeof(float), hipMemcpyDeviceToHost));
	return RTX_OK;
}

} // extern "C"
