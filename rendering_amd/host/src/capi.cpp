// Thin C API over the host-side Scene for the Python tests / bench (ctypes).  Plain C types only.
#include <cstring>
#include <string>
#include <unistd.h>

#include "../../../include/rtx.h"
#include "../../../include/rtx_views.h"
#include "../../../include/rtx_texture.h"
#include <hip/hip_runtime_api.h>
#include "scene.h"
#include "stats.h"
#include "util.h"

namespace {
thread_local std::string gLastError;
// Runs f with LOG_ERROR() throwing instead of exiting; a thrown error is kept for rah_last_error() and `bad` is returned.
template <typename R, typename F> R guarded(R bad, F&& f)
{
	ThrowErrorsScope scope;
	try { gLastError.clear(); return f(); }
	catch (const std::exception& e) { gLastError = e.what(); return bad; }
}
}

extern "C" {

const char* rah_last_error(void) { return gLastError.c_str(); }

// Loads a .scene file (relative asset paths resolve against cwd when given; the process's working directory is
// restored afterwards); w/h > 0 override the file's resolution.  The process-global options:: switches are reset to
// their defaults for the load and the ones the render reads are then pinned on the Scene (Scene::pinFlags), so that
// loading another scene later does not change this one.  NULL on failure (rah_last_error).
void* rah_scene_load(const char* cwd, const char* path, int width, int height)
{
	return guarded<void*>(nullptr, [&]() -> void* {
		options::reset();
		options::enableOutput = false;
		options::imageOutput = false;
		stats::reset();
		char back[4096];
		const bool moved = cwd && cwd[0];
		if (moved && (!getcwd(back, sizeof(back)) || chdir(cwd) != 0)) { gLastError = "cannot change to the scene's base directory"; return nullptr; }
		struct Restore { const char* dir; ~Restore() { if (dir && chdir(dir) != 0) {} } } restore{ moved ? back : nullptr };
		Scene* s = new Scene(path);
		if (!s->sceneLoadSuccess) { delete s; gLastError = std::string("could not load scene ") + path; return nullptr; }
		if (width > 0) s->options.width = (size_t)width;
		if (height > 0) s->options.height = (size_t)height;
		s->pinFlags();
		return s;
	});
}
void rah_scene_free(void* h) { delete (Scene*)h; }

void rah_scene_dims(void* h, int* w, int* ht, int* nObjects, int* nLights)
{
	Scene* s = (Scene*)h;
	*w = (int)s->options.width; *ht = (int)s->options.height; *nObjects = (int)s->objects.size(); *nLights = (int)s->lights.size();
}
void rah_scene_resize(void* h, int w, int ht)
{
	Scene* s = (Scene*)h;
	s->options.width = (size_t)w; s->options.height = (size_t)ht;
	s->invalidateView();
}
// Moves the camera (position, Euler angles in degrees: Camera::pos / Camera::rot, scene.h:52-66); the next use re-applies the view (rtx_scene_set_view).
void rah_camera_set(void* h, const float* pos3, const float* rot3)
{
	Scene* s = (Scene*)h;
	s->camera.pos = Vec3f(pos3[0], pos3[1], pos3[2]); s->camera.rot = Vec3f(rot3[0], rot3[1], rot3[2]);
	s->camera.cameraRotated = false;
	s->invalidateView();
}
void rah_camera_get(void* h, float* pos3, float* rot3)
{
	Scene* s = (Scene*)h;
	pos3[0] = s->camera.pos.x; pos3[1] = s->camera.pos.y; pos3[2] = s->camera.pos.z; rot3[0] = s->camera.rot.x; rot3[1] = s->camera.rot.y; rot3[2] = s->camera.rot.z;
}
void rah_scene_set_device(void* h, int device) { ((Scene*)h)->device = device; }
void rah_set_flag(void* h, const char* name, int v)
{
	Scene* s = (Scene*)h;
	if (!strcmp(name, "useBackfaceCulling")) s->useBackfaceCulling = v != 0;
	else if (!strcmp(name, "collectStatistics")) s->collectStatistics = v != 0;
	else if (!strcmp(name, "useSkybox")) s->useSkybox = v != 0;
	else if (!strcmp(name, "showNormals")) s->showNormals = v != 0;
	else if (!strcmp(name, "showAC")) s->showAC = v != 0;
	s->invalidateView();
}

// Flattened description (host arrays stay alive until rah_flat_free).
void* rah_flatten(void* h) { return flattenScene(*(Scene*)h); }
const rtx_scene_desc* rah_flat_desc(void* f) { return flatDesc((FlatScene*)f); }
void rah_flat_free(void* f) { freeFlatScene((FlatScene*)f); }

// Where the next rah_scene_load builds acceleration structures: -1 auto, 0 host builder, 1 device (rtx_bvh_build).
void rah_set_ac_build(int mode, int device) { options::acBuildOnDevice = mode; options::acBuildDevice = device; }
// Only the device (one process per GPU: every rank builds on the GPU it renders on, as render_amd does per rank).
void rah_set_ac_build_device(int device) { options::acBuildDevice = device; }

// {built on the device (0/1), device build time in ms}
int rah_bvh_build_info(void* h, int obj, int* onDevice, float* ms)
{
	Scene* s = (Scene*)h;
	if (guarded<int>(-1, [&] { s->syncTrees(); return 0; }) != 0) return -1;
	if (obj < 0 || obj >= (int)s->objects.size() || s->objects[obj]->objectType != ObjectType::Mesh) return -1;
	const Mesh& m = static_cast<const Mesh&>(*s->objects[obj]);
	if (!m.ac) return -1;
	*onDevice = m.ac->builtOnDevice ? 1 : 0; *ms = m.ac->buildMs;
	return 0;
}

// BVH in the dump layout shared with the oracle / reference harness.
int rah_bvh_counts(void* h, int obj, long long* c)
{
	Scene* s = (Scene*)h;
	if (guarded<int>(-1, [&] { s->syncTrees(); return 0; }) != 0) return -1;
	if (obj < 0 || obj >= (int)s->objects.size() || s->objects[obj]->objectType != ObjectType::Mesh) return -1;
	const Mesh& m = static_cast<const Mesh&>(*s->objects[obj]);
	if (!m.ac) return -1;
	c[0] = (long long)m.ac->nodes.size(); c[1] = (long long)m.ac->leafCount(); c[2] = (long long)m.ac->refs.size();
	c[3] = m.ac->maxDepth; c[4] = (long long)m.allTris.size();
	return 0;
}

int rah_bvh_dump(void* h, int obj, float* bounds, int32_t* skip, int32_t* leafBegin, int32_t* leafCount, uint32_t* refs)
{
	Scene* s = (Scene*)h;
	if (guarded<int>(-1, [&] { s->syncTrees(); return 0; }) != 0) return -1;
	if (obj < 0 || obj >= (int)s->objects.size() || s->objects[obj]->objectType != ObjectType::Mesh) return -1;
	const Mesh& m = static_cast<const Mesh&>(*s->objects[obj]);
	if (!m.ac) return -1;
	for (size_t i = 0; i < m.ac->nodes.size(); ++i) {
		const auto& n = m.ac->nodes[i];
		float* b = bounds + i * 6;
		b[0] = n.bounds[0].x; b[1] = n.bounds[0].y; b[2] = n.bounds[0].z; b[3] = n.bounds[1].x; b[4] = n.bounds[1].y; b[5] = n.bounds[1].z;
		skip[i] = n.skip; leafBegin[i] = n.leafBegin; leafCount[i] = n.leafCount;
	}
	memcpy(refs, m.ac->refs.data(), m.ac->refs.size() * sizeof(uint32_t));
	return 0;
}

// The host builder (AccelerationStructure::setup, objects.cpp:385-392 + 470-526 + 633-763 of the reference restated) on a bare triangle array:
// pos = n x 9 floats (a, b, c), lo / hi = the root box, in the dump layout of rah_bvh_dump.  counts = {nodes, leaves, refs, maxDepth};
// the arrays may be NULL to ask for the counts only (the structure is built twice then).  For the parity tests on the reference's own models
// where the OBJ files are not at hand (tests/test_ref_models.py: the golden file keeps the triangles the reference's loader produced).
int rah_bvh_from_tris(const float* pos, int n, const float* lo, const float* hi, int acPenalty, long long* counts,
                      float* bounds, int32_t* skip, int32_t* leafBegin, int32_t* leafCount, uint32_t* refs)
{
	return guarded<int>(-1, [&]() -> int {
		std::vector<Triangle> tris((size_t)n);
		for (int i = 0; i < n; ++i) {
			tris[i].a = Vec3f(pos[i * 9], pos[i * 9 + 1], pos[i * 9 + 2]); tris[i].b = Vec3f(pos[i * 9 + 3], pos[i * 9 + 4], pos[i * 9 + 5]);
			tris[i].c = Vec3f(pos[i * 9 + 6], pos[i * 9 + 7], pos[i * 9 + 8]);
		}
		Options o; o.acPenalty = acPenalty;
		// the host builder, quietly; both process-wide options are put back on EVERY way out (setup may throw: guarded<> catches it -- ADVICE r5)
		struct Restore {
			decltype(options::acBuildOnDevice) keep = options::acBuildOnDevice; const bool quiet = options::enableOutput;
			Restore() { options::acBuildOnDevice = 0; options::enableOutput = false; }
			~Restore() { options::acBuildOnDevice = keep; options::enableOutput = quiet; }
		};
		AccelerationStructure ac;
		ac.setBounds(Vec3f(lo[0], lo[1], lo[2]), Vec3f(hi[0], hi[1], hi[2]));
		bool ok;
		{ Restore restore; ok = ac.setup(tris, o); }
		if (!ok) return -1;
		counts[0] = (long long)ac.nodes.size(); counts[1] = (long long)ac.leafCount(); counts[2] = (long long)ac.refs.size(); counts[3] = ac.maxDepth;
		if (!bounds) return 0;
		for (size_t i = 0; i < ac.nodes.size(); ++i) {
			const auto& nd = ac.nodes[i];
			float* b = bounds + i * 6;
			b[0] = nd.bounds[0].x; b[1] = nd.bounds[0].y; b[2] = nd.bounds[0].z; b[3] = nd.bounds[1].x; b[4] = nd.bounds[1].y; b[5] = nd.bounds[1].z;
			skip[i] = nd.skip; leafBegin[i] = nd.leafBegin; leafCount[i] = nd.leafCount;
		}
		memcpy(refs, ac.refs.data(), ac.refs.size() * sizeof(uint32_t));
		return 0;
	});
}

// 30 floats per triangle: a b c n_a n_b n_c | t_a t_b t_c | tangent bitangent
int rah_tris(void* h, int obj, float* out)
{
	Scene* s = (Scene*)h;
	if (obj < 0 || obj >= (int)s->objects.size() || s->objects[obj]->objectType != ObjectType::Mesh) return -1;
	const Mesh& m = static_cast<const Mesh&>(*s->objects[obj]);
	for (size_t i = 0; i < m.allTris.size(); ++i) {
		const Triangle& t = m.allTris[i];
		float* o = out + i * 30;
		const Vec3f* v[6] = { &t.a, &t.b, &t.c, &t.n_a, &t.n_b, &t.n_c };
		for (int k = 0; k < 6; ++k) { o[k * 3] = v[k]->x; o[k * 3 + 1] = v[k]->y; o[k * 3 + 2] = v[k]->z; }
		o[18] = t.t_a.x; o[19] = t.t_a.y; o[20] = t.t_b.x; o[21] = t.t_b.y; o[22] = t.t_c.x; o[23] = t.t_c.y;
		o[24] = t.tangent.x; o[25] = t.tangent.y; o[26] = t.tangent.z; o[27] = t.bitangent.x; o[28] = t.bitangent.y; o[29] = t.bitangent.z;
	}
	return 0;
}

// camera constants exactly as uploaded (rtx_view::scale/aspect/cam_matrix/cam_pos)
void rah_camera(void* h, float* scale, float* aspect, float* m16, float* pos3)
{
	guarded<int>(-1, [&] {
		FlatScene* f = flattenScene(*(Scene*)h);
		const rtx_view& v = flatDesc(f)->view;
		*scale = v.scale; *aspect = v.aspect;
		memcpy(m16, v.cam_matrix, 64); memcpy(pos3, v.cam_pos, 12);
		freeFlatScene(f);
		return 0;
	});
}

// The camera fields and the size of one view of a batch (rtx_view_target, include/rtx_views.h): exactly what fillView gives the scene's own view
// after rah_camera_set(pos3, rot3) + rah_scene_resize(w, ht) -- and, with fov >= 0, with that fov in the scene file -- through the same Camera
// code and the same tanf.  fov < 0: the scene's.  The scene is not changed; the buffers of `out` are left as they are.  -1: a bad size.
int rah_view_target(void* h, const float* pos3, const float* rot3, float fov, int w, int ht, rtx_view_target* out)
{
	Scene* s = (Scene*)h;
	if (w <= 0 || ht <= 0) { gLastError = "rah_view_target: width and height must be > 0"; return -1; }
	Camera cam;
	cam.pos = Vec3f(pos3[0], pos3[1], pos3[2]); cam.rot = Vec3f(rot3[0], rot3[1], rot3[2]);
	cam.fov = fov >= 0 ? fov : s->camera.fov;
	cam.ensureMatrix();
	out->width = (uint32_t)w; out->height = (uint32_t)ht;
	out->cam_pos[0] = cam.pos.x; out->cam_pos[1] = cam.pos.y; out->cam_pos[2] = cam.pos.z;
	for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) out->cam_matrix[i * 4 + j] = cam.rMatrix[i][j];
	viewScaleAspect(cam.fov, (size_t)w, (size_t)ht, out->scale, out->aspect);
	return 0;
}

// rtx_view::flags this scene uploads (RTX_FLAG_*), -1 on error
int rah_view_flags(void* h)
{
	return guarded<int>(-1, [&] {
		FlatScene* f = flattenScene(*(Scene*)h);
		const int flags = (int)flatDesc(f)->view.flags;
		freeFlatScene(f);
		return flags;
	});
}

// rtx_view::max_ray_depth this scene uploads: the scene file's max_ray_depth (Scene.cast_tree's default depth)
int rah_max_ray_depth(void* h) { return ((Scene*)h)->options.maxRayDepth; }

// loadBMP (util.h) into a caller buffer of `cap` bytes; returns the number of bytes the image needs (3*w*h).
// (-1: unreadable / unsupported file, rah_last_error; -2: the image needs more than INT_MAX bytes)
int rah_load_bmp(const char* path, int* w, int* h, unsigned char* out, int cap)
{
	return guarded<int>(-1, [&] {
		unsigned char* d = loadBMP(path, *w, *h);
		const size_t need = (size_t)3 * (size_t)*w * (size_t)*h;
		if (out && cap >= 0 && (size_t)cap >= need) memcpy(out, d, need);
		delete[] d;
		return need > 0x7fffffffu ? -2 : (int)need;
	});
}

// Places object `obj` again as its [object] block would with these values (Scene::moveObject; NULL = unchanged): mesh pos3 / rot3 / size3,
// sphere pos3 / radius1, plane pos3 / normal3.  0, or -1 with rah_last_error (bad index, a key the type does not have, a device error).
int rah_object_move(void* h, int obj, const float* pos3, const float* rot3, const float* size3, const float* radius1, const float* normal3)
{
	return guarded<int>(-1, [&] {
		if (obj < 0) { noteError("moveObject: object index out of range"); LOG_ERROR(); }
		((Scene*)h)->moveObject((size_t)obj, pos3, rot3, size3, radius1, normal3);
		return 0;
	});
}

namespace {
Mesh* meshOf(void* h, int obj)
{
	Scene* s = (Scene*)h;
	if (obj < 0 || obj >= (int)s->objects.size() || s->objects[obj]->objectType != ObjectType::Mesh) return nullptr;
	return static_cast<Mesh*>(s->objects[obj].get());
}
}

// What the loader kept of mesh `obj`'s OBJ file: c[8] = {triangles, vertices, normals, uv, vertices read before the first face, normals read
// before it, has faces, -}.  -1: no such mesh.
int rah_mesh_counts(void* h, int obj, long long* c)
{
	const Mesh* m = meshOf(h, obj);
	if (!m) return -1;
	c[0] = (long long)m->corners.size(); c[1] = (long long)m->objP.size(); c[2] = (long long)m->objN.size(); c[3] = (long long)m->objT.size();
	c[4] = (long long)m->placedP; c[5] = (long long)m->placedN; c[6] = m->hasFaces ? 1 : 0; c[7] = 0;
	return 0;
}

// The vertices (n x 3) and normals (n x 3, as stored: normalised) of mesh `obj`; either may be NULL.
int rah_mesh_vertices(void* h, int obj, float* P, float* N)
{
	const Mesh* m = meshOf(h, obj);
	if (!m) return -1;
	if (P && !m->objP.empty()) memcpy(P, &m->objP[0].x, m->objP.size() * sizeof(Vec3f));
	if (N && !m->objN.empty()) memcpy(N, &m->objN[0].x, m->objN.size() * sizeof(Vec3f));
	return 0;
}

// The corners of mesh `obj`'s triangles (n x 3 each: position indices; normal and uv indices, [0] = -1 where the face gave none) and its uv (n x 2).
int rah_mesh_topology(void* h, int obj, uint32_t* cornerPos, int32_t* cornerNrm, int32_t* cornerUv, float* uv)
{
	const Mesh* m = meshOf(h, obj);
	if (!m) return -1;
	for (size_t i = 0; i < m->corners.size(); ++i)
		for (int k = 0; k < 3; ++k) {
			if (cornerPos) cornerPos[i * 3 + k] = m->corners[i].v[k];
			if (cornerNrm) cornerNrm[i * 3 + k] = m->corners[i].n[k];
			if (cornerUv) cornerUv[i * 3 + k] = m->corners[i].t[k];
		}
	if (uv && !m->objT.empty()) memcpy(uv, &m->objT[0].x, m->objT.size() * sizeof(Vec2f));
	return 0;
}

// New vertices (nP x 3) and, with N, raw normals (nN x 3) for mesh `obj` (Scene::setVertices); onDevice: device pointers produced on `stream`.
// 0, or -1 with rah_last_error: the scene is then as it was.
int rah_mesh_set_vertices(void* h, int obj, const float* P, long long nP, const float* N, long long nN, int onDevice, void* stream)
{
	return guarded<int>(-1, [&] {
		if (obj < 0 || nP < 0 || nN < 0) { noteError("setVertices: bad index or count"); LOG_ERROR(); }
		((Scene*)h)->setVertices((size_t)obj, P, (size_t)nP, N, (size_t)nN, onDevice != 0, stream);
		return 0;
	});
}

// The loaders' texel arithmetic (objects.h, decodeTexels): n RGB8 texels into 3 n floats, n for RTX_TEX_SPECULAR.  -1: no such kind.
int rah_decode_texels(int kind, const unsigned char* rgb8, long long n, float* out)
{
	if (n < 0 || (n && (!rgb8 || !out))) return -1;
	return decodeTexels(kind, rgb8, (size_t)n, out) ? 0 : -1;
}

// 1: the scene has been uploaded (Scene::gpu has run), 0: it lives on the host alone
int rah_scene_has_gpu(void* h) { return ((Scene*)h)->hasGpu() ? 1 : 0; }

// Map `kind` (RTX_TEX_DIFFUSE / NORMAL / SPECULAR) of mesh `obj` replaced by `texels` (Scene::setMap; NULL: removed); onDevice: its data is in
// device memory, produced on `stream`.  0, or -1 with rah_last_error: the scene is then as it was.
int rah_mesh_set_map(void* h, int obj, int kind, const rtx_texels* texels, int onDevice, void* stream)
{
	return guarded<int>(-1, [&] {
		if (obj < 0) { noteError("setMap: object index out of range"); LOG_ERROR(); }
		((Scene*)h)->setMap((size_t)obj, kind, texels, onDevice != 0, stream);
		return 0;
	});
}

// The six skybox faces replaced (Scene::setSky; NULL: the scene loses its skybox).  0, or -1 with rah_last_error.
int rah_scene_set_sky(void* h, const rtx_texels* faces6, int onDevice, void* stream)
{
	return guarded<int>(-1, [&] {
		((Scene*)h)->setSky(faces6, onDevice != 0, stream);
		return 0;
	});
}

// A rectangle of texels written at (x0, y0) into map `kind` of mesh `index`, or into sky face `index` for RTX_TEX_SKY (Scene::writeTexels):
// queued on `stream` with a live GPU scene.  0, or -1 with rah_last_error.
int rah_write_texels(void* h, int kind, int index, unsigned x0, unsigned y0, const rtx_texels* texels, int onDevice, void* stream)
{
	return guarded<int>(-1, [&] {
		if (index < 0 || !texels) { noteError("writeTexels: bad index or texels"); LOG_ERROR(); }
		((Scene*)h)->writeTexels(kind, (size_t)index, x0, y0, *texels, onDevice != 0, stream);
		return 0;
	});
}

// Size of map `kind` of mesh `index` (of sky face `index`), 0 x 0 where there is none, and with `out` its stored texels: into host memory from
// the host's copy (read back first where a write left it behind), or with outOnDevice into device memory by a copy queued on `stream`
// (a live GPU scene only).  0, or -1 with rah_last_error.
int rah_texture(void* h, int kind, int index, int* width, int* height, float* out, int outOnDevice, void* stream)
{
	return guarded<int>(-1, [&] {
		Scene* s = (Scene*)h;
		if (index < 0) { noteError("texture: index out of range"); LOG_ERROR(); }
		if (!outOnDevice && (out || !s->hasGpu())) {
			const float* p = s->texture(kind, (size_t)index, *width, *height);
			if (out && p) memcpy(out, p, (size_t)*width * *height * (kind == RTX_TEX_SPECULAR ? 1 : 3) * sizeof(float));
			return 0;
		}
		if (!s->hasGpu()) { noteError("texture: a device copy without a GPU scene"); LOG_ERROR(); }
		uint32_t devIndex = (uint32_t)index;
		if (kind != RTX_TEX_SKY) {
			if (!meshOf(h, index)) { noteError("texture: no such mesh"); LOG_ERROR(); }
			devIndex = 0;
			for (int i = 0; i < index; ++i) devIndex += s->objects[i]->objectType == ObjectType::Mesh;
		}
		uint32_t w = 0, ht = 0;
		const float* dev = nullptr;
		if (rtx_scene_texture_info(s->gpu(), kind, devIndex, &w, &ht, &dev) != RTX_OK) { noteError(rtx_last_error()); LOG_ERROR(); }
		*width = (int)w; *height = (int)ht;
		if (dev && out && hipMemcpyAsync(out, dev, (size_t)w * ht * (kind == RTX_TEX_SPECULAR ? 1 : 3) * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess) {
			noteError("texture: the copy could not be queued"); LOG_ERROR();
		}
		return 0;
	});
}

// host wall ms of the last rah_mesh_set_vertices: {device call without the rebuild, the rebuild, the host mirror, whole call}
void rah_mesh_deform_times(void* h, float* ms4)
{
	for (int k = 0; k < 4; k++) ms4[k] = (float)((Scene*)h)->lastDeformMs[k];
}

// The rotation matrix the loader places a mesh with (Matrix44f::fromEulerDegrees, row-major): what rtx_mesh_pose::rot_matrix takes.
void rah_euler_matrix(const float* rot3, float* m16)
{
	const Matrix44f R = Matrix44f::fromEulerDegrees(Vec3f(rot3[0], rot3[1], rot3[2]));
	for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) m16[i * 4 + j] = R[i][j];
}

// pos3, rot3, size3 of mesh `obj` and the scene's bias and acPenalty: the pose it is placed with.
int rah_mesh_pose(void* h, int obj, float* pos3, float* rot3, float* size3, float* bias, int* acPenalty)
{
	const Mesh* m = meshOf(h, obj);
	if (!m) return -1;
	const Scene* s = (Scene*)h;
	pos3[0] = m->pos.x; pos3[1] = m->pos.y; pos3[2] = m->pos.z; rot3[0] = m->rot.x; rot3[1] = m->rot.y; rot3[2] = m->rot.z;
	size3[0] = m->size.x; size3[1] = m->size.y; size3[2] = m->size.z;
	*bias = s->options.bias; *acPenalty = s->options.acPenalty;
	return 0;
}

// RTX_OBJ_* of object `obj` (-1: no such object)
int rah_object_type(void* h, int obj)
{
	Scene* s = (Scene*)h;
	if (obj < 0 || obj >= (int)s->objects.size()) return -1;
	const ObjectType t = s->objects[obj]->objectType;
	return t == ObjectType::Sphere ? RTX_OBJ_SPHERE : t == ObjectType::Plane ? RTX_OBJ_PLANE : t == ObjectType::Mesh ? RTX_OBJ_MESH : -1;
}

// RTX_LIGHT_* of light `index` (-1: no such light)
int rah_light_type(void* h, int index)
{
	Scene* s = (Scene*)h;
	if (index < 0 || index >= (int)s->lights.size()) return -1;
	const LightType t = s->lights[index]->type;
	return t == LightType::DistantLight ? RTX_LIGHT_DISTANT : t == LightType::PointLight ? RTX_LIGHT_POINT : t == LightType::AreaLight ? RTX_LIGHT_AREA : -1;
}

namespace {
LightKeys lightKeys(const float* color3, const float* intensity1, const float* direction3, const float* position3, const float* pos3, const float* i3,
                    const float* j3, const int* samples1)
{
	LightKeys k;
	k.color = color3; k.intensity = intensity1; k.direction = direction3; k.position = position3; k.pos = pos3; k.i = i3; k.j = j3; k.samples = samples1;
	return k;
}
}

// Light `index` as its [light] block would load with these keys set (Scene::setLight; NULL = unchanged): every type color3 / intensity1, a
// distant light direction3, a point light position3, an area light pos3 / i3 / j3 / samples1.  0, or -1 with rah_last_error (bad index, a key
// the type does not have, a device error): the scene is then as it was.
int rah_light_set(void* h, int index, const float* color3, const float* intensity1, const float* direction3, const float* position3, const float* pos3,
                  const float* i3, const float* j3, const int* samples1)
{
	return guarded<int>(-1, [&] {
		if (index < 0) { noteError("setLight: light index out of range"); LOG_ERROR(); }
		((Scene*)h)->setLight((size_t)index, lightKeys(color3, intensity1, direction3, position3, pos3, i3, j3, samples1));
		return 0;
	});
}

// A new light of RTX_LIGHT_* `type` after the last one, with the parser's defaults for absent keys (Scene::addLight): its index, or -1.
int rah_light_add(void* h, int type, const float* color3, const float* intensity1, const float* direction3, const float* position3, const float* pos3,
                  const float* i3, const float* j3, const int* samples1)
{
	return guarded<int>(-1, [&] {
		const char* name = type == RTX_LIGHT_DISTANT ? "distant" : type == RTX_LIGHT_POINT ? "point" : type == RTX_LIGHT_AREA ? "area" : "?";
		return (int)((Scene*)h)->addLight(name, lightKeys(color3, intensity1, direction3, position3, pos3, i3, j3, samples1));
	});
}

// Removes light `index` (Scene::removeLight): 0, or -1 with rah_last_error.
int rah_light_remove(void* h, int index)
{
	return guarded<int>(-1, [&] {
		if (index < 0) { noteError("removeLight: light index out of range"); LOG_ERROR(); }
		((Scene*)h)->removeLight((size_t)index);
		return 0;
	});
}

// A new object of RTX_OBJ_* `type` before object `at` (at < 0: after the last one), as a new [object] block with these keys would load
// (Scene::addObject; NULL = absent, the loader's default): every type pos3 / color3 / material (the text of a material= line), a mesh size3 /
// rot3 / name / diffuse_map / normal_map / specular_map, a sphere radius1, a plane normal3.  File names resolve against cwd when given, as in
// rah_scene_load.  Its index, or -1 with rah_last_error (a key the type does not have, an OBJ or a map that cannot be loaded, a bad index,
// a device error): the scene is then as it was.
int rah_object_add(void* h, int type, int at, const char* cwd, const float* pos3, const float* size3, const float* rot3, const float* color3,
                   const char* material, const float* radius1, const float* normal3, const char* name, const char* diffuse_map, const char* normal_map,
                   const char* specular_map)
{
	return guarded<int>(-1, [&]() -> int {
		const char* kind = type == RTX_OBJ_SPHERE ? "sphere" : type == RTX_OBJ_PLANE ? "plane" : type == RTX_OBJ_MESH ? "mesh" : "?";
		Scene* s = (Scene*)h;
		ObjectKeys k;
		k.pos = pos3; k.size = size3; k.rot = rot3; k.color = color3; k.material = material; k.radius = radius1; k.normal = normal3;
		k.name = name; k.diffuse_map = diffuse_map; k.normal_map = normal_map; k.specular_map = specular_map;
		char back[4096];
		const bool moved = cwd && cwd[0];
		if (moved && (!getcwd(back, sizeof(back)) || chdir(cwd) != 0)) { noteError("cannot change to the scene's base directory"); LOG_ERROR(); }
		struct Restore { const char* dir; ~Restore() { if (dir && chdir(dir) != 0) {} } } restore{ moved ? back : nullptr };
		const bool quiet = options::enableOutput;
		struct Quiet { bool keep; ~Quiet() { options::enableOutput = keep; } } q{ quiet };
		options::enableOutput = false;
		return (int)s->addObject(kind, k, at < 0 ? (size_t)-1 : (size_t)at);
	});
}

// Removes object `index` (Scene::removeObject): 0, or -1 with rah_last_error.
int rah_object_remove(void* h, int index)
{
	return guarded<int>(-1, [&] {
		if (index < 0) { noteError("removeObject: object index out of range"); LOG_ERROR(); }
		((Scene*)h)->removeObject((size_t)index);
		return 0;
	});
}

// host wall ms of the last rah_object_move: {placement, upload of the triangles, rtx_scene_set_object, rtx_scene_update_mesh}
void rah_object_move_times(void* h, float* ms4)
{
	for (int k = 0; k < 4; k++) ms4[k] = (float)((Scene*)h)->lastMoveMs[k];
}

// Numeric digest of objects and lights (for loader tests): per object 16 floats
// [type, material, pos3, color3, ior, ambient, diffuse, specular, nSpecular, r2 | normal.x, ...], per light 12 floats.
int rah_scene_digest(void* h, float* out, int maxFloats)
{
	Scene* s = (Scene*)h;
	FlatScene* f = flattenScene(*s);
	const rtx_scene_desc* d = flatDesc(f);
	int n = 0;
	auto put = [&](float v) { if (n < maxFloats) out[n] = v; n++; };
	for (uint32_t i = 0; i < d->n_objects; i++) {
		const rtx_object& o = d->objects[i];
		put((float)o.type); put((float)o.material);
		for (int k = 0; k < 3; k++) put(o.pos[k]);
		for (int k = 0; k < 3; k++) put(o.color[k]);
		put(o.ior); put(o.ambient); put(o.diffuse); put(o.specular); put(o.n_specular); put(o.radius2);
		for (int k = 0; k < 3; k++) put(o.normal[k]);
	}
	for (uint32_t i = 0; i < d->n_lights; i++) {
		const rtx_light& l = d->lights[i];
		put((float)l.type);
		for (int k = 0; k < 3; k++) put(l.color[k]);
		put(l.intensity);
		for (int k = 0; k < 3; k++) put(l.dir[k]);
		for (int k = 0; k < 3; k++) put(l.pos[k]);
		put((float)l.n_points);
	}
	freeFlatScene(f);
	return n;
}

// The uploaded GPU scene (created on first use); NULL when it cannot be created, e.g. without a GPU (rah_last_error).
rtx_scene* rah_scene_gpu(void* h) { return guarded<rtx_scene*>(nullptr, [&] { return ((Scene*)h)->gpu(); }); }

// Whole-frame convenience mirroring Scene::render() into a host buffer (H*W*3 floats, zero-initialised by caller).
int rah_render_host(void* h, float* fb, int withSsaa)
{
	return guarded<int>(-1, [&] {
		Scene* s = (Scene*)h;
		s->launchWorkers((Vec3f*)fb);
		if (withSsaa) s->launchSSAA((Vec3f*)fb);
		return 0;
	});
}

int rah_save_bmp(void* h, const float* fb, const char* nameNoExt)
{
	Scene* s = (Scene*)h;
	s->options.imageName = nameNoExt;
	return saveImage((const Vec3f*)fb, s->options);
}

} // extern "C"
