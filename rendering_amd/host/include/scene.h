// Scene / Camera / Render (reference: include/scene.h).  Same public surface -- Scene(path), render(),
// launchWorkers(Vec3f*), launchSSAA(Vec3f*), getTiles(), objects / lights / options / camera -- but the
// two worker loops are launches of the gfx950 kernels through the C ABI in include/rtx.h.
#pragma once
#include <string>
#include <vector>

#include "geometry.h"
#include "lights.h"
#include "objects.h"
#include "options.h"

#include <memory>

struct rtx_scene;
struct rtx_scene_desc;
struct rtx_comm;
struct rtx_texels;

typedef struct { size_t x0, x1, y0, y1; } tileInfo;

class Camera {
public:
	Vec3f pos{ 0, 0, 0 };
	Vec3f rot{ 0, 0, 0 };
	Matrix44f rMatrix;
	float fov = 60.0f;
	float zNear = 0.1f, zFar = 100.0f;
	bool cameraRotated = false;
	void ensureMatrix();          // the lazy part of Camera::getRay (scene.cpp:22-49), done before upload
};

// Render::trace's result record (reference: scene.h:17-23)
struct IntersectInfo {
	const Object* hitObject = nullptr;
	float tNear = 3.402823466e+38f;
	const Triangle* triPtr = nullptr;
	Vec2f uv{ -1, -1 };
};

class Scene;

// Single-ray entry points of the reference (scene.h:31-48), evaluated on the GPU through rtx_cast_rays.
// They take the Scene (which owns the uploaded GPU twin) instead of the bare ObjectVector; castRay supports
// depth 0 only (deeper levels are internal to the kernel's recursion frames).  Meant for tools and tests --
// frames go through Scene::launchWorkers.
class Render {
public:
	static bool trace(const Ray& ray, Scene& scene, IntersectInfo& intrInfo);
	static Vec3f castRay(const Ray& ray, Scene& scene, const int depth);
};

class Scene {
public:
	bool sceneLoadSuccess = true;
	ObjectVector objects;
	LightsVector lights;
	Options options;
	Camera camera;
	int skyboxWidth = 0, skyboxHeight = 0;
	std::vector<Vec3f> skyboxes[6];

	explicit Scene(const std::string& sceneName);
	~Scene();
	Scene(const Scene&) = delete;
	Scene& operator=(const Scene&) = delete;

	bool loadScene(const std::string& sceneName);
	void loadSkybox();
	void render();
	void launchWorkers(Vec3f* frameBuffer);   // pass 1 on the GPU, result copied into the caller's buffer
	void launchSSAA(Vec3f* frameBuffer);      // Sobel + 4-ray re-render on the GPU
	std::vector<tileInfo> getTiles();

	// MI355X side
	int device = 0;
	rtx_scene* gpu();                          // flattens + uploads on first use; LOG_ERROR()s without a GPU
	void invalidateView();                     // call after changing options.width/height, camera, flags
	// Places object `index` as its [object] block would with these values (NULL: unchanged): a mesh takes pos / rot / size (its vertices are
	// placed again by the loader's own code), a sphere pos / radius, a plane pos / normal; any other key is an error.  With a live GPU scene
	// the new triangles go up and the device rebuilds the structure (rtx_scene_set_object / rtx_scene_update_mesh, include/rtx_scene_edit.h);
	// without one the host structure is built again as the loader builds it.
	void moveObject(size_t index, const float* pos3, const float* rot3, const float* size3, const float* radius1, const float* normal3);
	void moveObjectApply(size_t index, const float* pos3, const float* rot3, const float* size3, const float* radius1, const float* normal3, double (*now)());
	// The lights edited as their [light] blocks would be (lights.h: the keys go through the code the parser applies them with; a key the
	// type does not have is an error and nothing changes).  addLight appends -- a new block after the last one -- and returns the index.
	// With a live GPU scene each ends in one rtx_scene_set_lights (include/rtx_scene_edit.h); if that fails the lights are put back.
	void setLight(size_t index, const LightKeys& keys);
	size_t addLight(const std::string& type, const LightKeys& keys);
	void removeLight(size_t index);
	// The object list edited as the scene file's [object] blocks would be (objects.h: the keys go through the code the parser applies them
	// with).  addObject puts a new block's object before object `at` (default: after the last one) and returns its index; an OBJ or a map
	// that fails to load, a key the type does not have or a bad index is an error and nothing changes.  With a live GPU scene each ends in
	// one rtx_scene_set_objects (include/rtx_scene_edit.h) that keeps every other mesh as it is; if that fails the objects are put back.
	size_t addObject(const std::string& type, const ObjectKeys& keys, size_t at = (size_t)-1);
	void removeObject(size_t index);
	// Gives mesh `index` the vertices (and, with N, the raw normals) an OBJ file with these v / vn lines would give it: nP x 3 / nN x 3 floats, the
	// counts the mesh was loaded with.  onDevice: P and N are device pointers, produced on `stream`.  With a live GPU scene the device places the
	// vertices, assembles the triangles and rebuilds the structure (rtx_scene_deform_mesh, include/rtx_deform.h); the host keeps objP / objN / objLo /
	// objHi and places its own triangles when something reads them (syncTrees).  Without one the loader's code runs on the host.  Refused, the
	// scene as it was: a bad index, an object that is no mesh, a wrong count, a vertex, normal or placed position that is not finite.
	void setVertices(size_t index, const float* P, size_t nP, const float* N, size_t nN, bool onDevice, void* stream);
	// host wall ms of the last setVertices: {the device call without the rebuild, the rebuild (rtx_scene_update_mesh), the host mirror, whole call}
	double lastDeformMs[4] = { 0, 0, 0, 0 };
	// Texture maps and skybox replaced or written into (include/rtx_texture.h; kind: RTX_TEX_*, index: the object, or the sky face).  The
	// texels are a rtx_texels record whose data is in host memory, or with onDevice in device memory produced on `stream`.  With a live GPU
	// scene the device decodes them (host texels go up as they are, never decoded) and this Scene's own copy of the map -- which a later
	// flatten uploads -- is read back: at once after setMap / setSky, before the next reader after writeTexels, which is asynchronous
	// (mapStale, skyStale; syncMaps).  Without one the edit is decoded into the host copy by the loaders' functions (objects.h).  texels ==
	// NULL removes the map / the skybox.  Refused, the scene as it was: a bad index, kind or record, an object that is no mesh, a normal
	// map for a mesh without texture coordinates, a rectangle outside the map, removing the skybox while useSkybox is on.
	void setMap(size_t index, int kind, const rtx_texels* texels, bool onDevice, void* stream);
	void setSky(const rtx_texels* faces6, bool onDevice, void* stream);
	void writeTexels(int kind, size_t index, uint32_t x0, uint32_t y0, const rtx_texels& texels, bool onDevice, void* stream);
	// the host copy, current: size and texels (NULL where there is none)
	const float* texture(int kind, size_t index, int& width, int& height);
	void syncMaps();
	bool skyStale = false;
	bool hasGpu() const { return gpu_ != nullptr; }
	void syncTrees();                          // meshes moved on the GPU: their `ac` read back from the device (done by every reader of `ac`)
	// host wall ms of the last moveObject: {placement (Mesh::place), upload of the triangles, rtx_scene_set_object, rtx_scene_update_mesh}
	double lastMoveMs[4] = { 0, 0, 0, 0 };
	// Multi-GPU (one process per GPU): with a communicator of the C ABI attached (rtx_comm_create), render() renders this
	// rank's rows only and collects the image on rank 0 (rtx_gather), which writes the file.
	void attachComm(rtx_comm* comm, int nRanks, int rank);
	double lastPass1Ms = 0, lastSobelMs = 0, lastSsaaMs = 0, lastFrameMs = 0;      // (lastFrameMs: the whole of render(), rtx_render_frame)
	// The switches the render reads are process-global in the reference (options::useBackfaceCulling, useSkybox,
	// collectStatistics, and the debug views showNormals / showAC).  A host that keeps several scenes alive (the C API in capi.cpp) pins them
	// per scene here: -1 = follow the global (the reference's behaviour), 0 / 1 = this scene's own value.
	int useBackfaceCulling = -1, useSkybox = -1, collectStatistics = -1, showNormals = -1, showAC = -1;
	bool cullingOn() const { return useBackfaceCulling < 0 ? options::useBackfaceCulling : useBackfaceCulling != 0; }
	bool skyboxOn() const { return useSkybox < 0 ? options::useSkybox : useSkybox != 0; }
	bool statisticsOn() const { return collectStatistics < 0 ? options::collectStatistics : collectStatistics != 0; }
	bool normalsOn() const { return showNormals < 0 ? options::showNormals : showNormals != 0; }
	bool acOn() const { return showAC < 0 ? options::showAC : showAC != 0; }
	void pinFlags()
	{
		useBackfaceCulling = options::useBackfaceCulling; useSkybox = options::useSkybox; collectStatistics = options::collectStatistics;
		showNormals = options::showNormals; showAC = options::showAC;
	}

private:
	struct DeviceFrame;
	DeviceFrame& deviceFrame();                // the frame's device buffers (fp32 framebuffer, Sobel mask, BGR8 image)
	void pass1OnDevice();
	void ssaaOnDevice();
	void readTimes();
	void renderAC();
	void lightsToDevice();
	void objectsToDevice(const std::vector<const Object*>& before);
	rtx_scene* gpu_ = nullptr;
	bool viewDirty_ = true;
	std::unique_ptr<DeviceFrame> frame_;
	rtx_comm* comm_ = nullptr;
	int nRanks_ = 1, rank_ = 0;
};

// Host-side flattening used by Scene::gpu(); exposed for tests and for maintainers wiring the reference's own
// Scene to the C ABI.
struct FlatScene;
// rtx_view::scale / aspect of a camera's fov (degrees) and a frame size, as the flattened view gets them (also rah_view_target, capi.cpp)
void viewScaleAspect(float fov, size_t width, size_t height, float& scale, float& aspect);
FlatScene* flattenScene(Scene& scene);
const rtx_scene_desc* flatDesc(const FlatScene*);
void freeFlatScene(FlatScene*);
