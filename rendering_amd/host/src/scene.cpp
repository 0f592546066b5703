// Scene loading, flattening and frame orchestration of the MI355X renderer (reference: src/scene.cpp:57-360,
// 362-379, 470-657).  The reference's two worker loops -- Scene::launchWorkers / Scene::launchSSAA -- are
// replaced by launches of the gfx950 kernels through the C ABI (include/rtx.h); there is no CPU rendering
// path in this library.
#include "scene.h"

#include <algorithm>
#include <chrono>
#include <cstring>
#include <fstream>
#include <iostream>
#include <limits>
#include <thread>

#include <hip/hip_runtime_api.h>

#include "../../../include/rtx.h"
#include "../../../include/rtx_debug.h"
#include "../../../include/rtx_scene_edit.h"
#include "../../../include/rtx_deform.h"
#include "../../../include/rtx_texture.h"
#include "stats.h"
#include "timer.h"
#include "util.h"

void Camera::ensureMatrix()
{
	if (cameraRotated) return;
	rMatrix = Matrix44f::fromEulerDegrees(rot);
	cameraRotated = true;
}

// ------------------------------------------------------------------------------------------------
// .scene parser (scene.cpp:62-334): [options] / [light] / [object] blocks of key=value lines
// ------------------------------------------------------------------------------------------------
namespace {

bool contains(const std::string& s, const char* what) { return s.find(what) != std::string::npos; }

struct KeyValue { std::string key, value; };

KeyValue splitKeyValue(const std::string& line, bool stripBlanks)
{
	const size_t eq = line.find('=');
	if (eq == std::string::npos) LOG_ERROR();
	KeyValue kv{ line.substr(0, eq), line.substr(eq + 1) };
	if (stripBlanks) kv.key.erase(std::remove_if(kv.key.begin(), kv.key.end(), [](char c) { return c == ' ' || c == '\t'; }), kv.key.end());
	return kv;
}

void parseOption(Scene& sc, const KeyValue& kv)
{
	const std::string& k = kv.key; const std::string& v = kv.value;
	if (k == "outputProgress") options::outputProgress = strToBool(v);
	else if (k == "useBackfaceCulling") options::useBackfaceCulling = strToBool(v);
	else if (k == "collectStatistics") options::collectStatistics = strToBool(v);
	else if (k == "enableOutput") options::enableOutput = strToBool(v);
	else if (k == "imageOutput") options::imageOutput = strToBool(v);
	else if (k == "useAC") options::useAC = strToBool(v);
	else if (k == "showAC") options::showAC = strToBool(v);
	else if (k == "useSkybox") options::useSkybox = strToBool(v);
	else if (k == "useTextures") options::useTextures = strToBool(v);
	else if (k == "showNormals") options::showNormals = strToBool(v);
	else if (k == "width") sc.options.width = strToInt(v);
	else if (k == "height") sc.options.height = strToInt(v);
	else if (k == "fov") sc.camera.fov = strToFloat(v);
	else if (k == "image_name") {
		sc.options.imageName = v;
		// legacy files quote the name
		sc.options.imageName.erase(std::remove(sc.options.imageName.begin(), sc.options.imageName.end(), '"'), sc.options.imageName.end());
	}
	else if (k == "n_workers") sc.options.nWorkers = strToInt(v);
	else if (k == "max_ray_depth") sc.options.maxRayDepth = strToInt(v);
	else if (k == "ac_penalty") sc.options.acPenalty = strToInt(v);
	else if (k == "background_color") sc.options.backgroundColor = str3ToFloat(splitString(v, ','));
	else if (k == "position") sc.camera.pos = str3ToFloat(splitString(v, ','));
	else if (k == "rotation") sc.camera.rot = str3ToFloat(splitString(v, ','));
	else if (k == "skyboxes") {
		const auto names = splitString(v, ',');
		if (names.size() < 6) LOG_ERROR();
		for (int i = 0; i < 6; ++i) {
			strncpy(sc.options.skyboxNames[i], names[i].c_str(), 63);
			sc.options.skyboxNames[i][63] = 0;
		}
		options::useSkybox = true;
	}
	else std::cout << "Scene, unknown key: " << k << '\n';
}

// One key=value line of a [light] block: its values go through applyLightKeys (lights.h), as an edit's do (Scene::setLight).
void parseLight(std::unique_ptr<Light>& light, const KeyValue& kv)
{
	const std::string& k = kv.key; const std::string& v = kv.value;
	if (k == "type") {
		if (auto made = makeLight(v)) light = std::move(made);
		return;
	}
	if (!light) { std::cout << "Error, light type missing\n"; return; }
	LightKeys keys;
	Vec3f v3;
	float f = 0; int n = 0;
	const float** vec = k == "color" ? &keys.color : k == "direction" ? &keys.direction : k == "position" ? &keys.position : k == "pos" ? &keys.pos
	                    : k == "i" ? &keys.i : k == "j" ? &keys.j : nullptr;
	if (vec) { v3 = str3ToFloat(splitString(v, ',')); *vec = &v3.x; }
	else if (k == "intensity") { f = strToFloat(v); keys.intensity = &f; }
	else if (k == "samples") { n = strToInt(v); keys.samples = &n; }
	else return;
	if (lightKeyRefused(light->type, keys)) LOG_ERROR();
	applyLightKeys(*light, keys);
}

// One key=value line of an [object] block: its value goes through applyObjectKeys (objects.h), as an added object's do (Scene::addObject).
// A key the object's type does not have is skipped, as an unknown one is.
void parseObject(Scene& sc, std::unique_ptr<Object>& object, const KeyValue& kv)
{
	const std::string& k = kv.key; const std::string& v = kv.value;
	if (k == "type") {
		if (auto made = makeObject(v)) object = std::move(made);
		return;
	}
	if (!object) { std::cout << "Error, object type missing\n"; return; }
	ObjectKeys keys;
	Vec3f v3;
	float f = 0;
	const float** vec = k == "color" ? &keys.color : k == "pos" ? &keys.pos : k == "normal" ? &keys.normal : k == "size" ? &keys.size : k == "rot" ? &keys.rot : nullptr;
	const char** text = k == "material" ? &keys.material : k == "name" ? &keys.name : k == "diffuse_map" ? &keys.diffuse_map
	                    : k == "normal_map" ? &keys.normal_map : k == "specular_map" ? &keys.specular_map : nullptr;
	if (vec) {
		*vec = &v3.x;
		if (objectKeyRefused(object->objectType, keys)) return;
		v3 = str3ToFloat(splitString(v, ','));
	}
	else if (text) {
		*text = v.c_str();
		if (objectKeyRefused(object->objectType, keys)) return;
	}
	else if (k == "radius") {
		keys.radius = &f;
		if (objectKeyRefused(object->objectType, keys)) return;
		f = strToFloat(v);
	}
	else return;
	applyObjectKeys(*object, keys, sc.options);
}

// ---- legacy dialect (hardening) ------------------------------------------------
// The reference ships input/smooth_shading.scene in an older one-line-per-entity form that its current loader
// rejects (LOG_ERROR at scene.cpp:200-201):
//     [light]   name, point_light|distant_light, x,y,z, r,g,b, intensity
//     [object]  name, plane,  px,py,pz, nx,ny,nz, r,g,b, material
//               name, sphere, px,py,pz, radius,   r,g,b, material
//               name, mesh, "file.obj", px,py,pz, sx,sy,sz [, r,g,b [, material]]
// material = none | diffuse | reflective | transparent[:ior] | phong:ambient:diffuse:specular:n
// A line without '=' inside [light]/[object] is read this way and becomes one entity.
std::vector<std::string> legacyFields(const std::string& line)
{
	std::vector<std::string> out;
	for (std::string cell : splitString(line, ',')) {
		cell.erase(std::remove_if(cell.begin(), cell.end(), [](char c) { return c == ' ' || c == '\t' || c == '"' || c == '\r'; }), cell.end());
		out.push_back(cell);
	}
	while (!out.empty() && out.back().empty()) out.pop_back();
	return out;
}

Vec3f legacy3(const std::vector<std::string>& f, size_t at)
{
	if (at + 3 > f.size()) LOG_ERROR();
	return Vec3f(strToFloat(f[at]), strToFloat(f[at + 1]), strToFloat(f[at + 2]));
}

void legacyMaterial(Object& o, const std::string& token)
{
	const auto parts = splitString(token, ':');
	if (parts.empty() || parts[0] == "none" || parts[0] == "diffuse") return;
	if (parts[0] == "reflective") o.materialType = MaterialType::Reflective;
	else if (parts[0] == "transparent") {
		o.materialType = MaterialType::Transparent;
		if (parts.size() > 1) o.indexOfRefraction = strToFloat(parts[1]);
	}
	else if (parts[0] == "phong") {
		if (parts.size() < 5) LOG_ERROR();
		o.materialType = MaterialType::Phong;
		o.ambient = strToFloat(parts[1]); o.diffuse = strToFloat(parts[2]); o.specular = strToFloat(parts[3]); o.nSpecular = strToFloat(parts[4]);
	}
	else LOG_ERROR();
}

void parseLegacyLight(Scene& sc, const std::string& line)
{
	const auto f = legacyFields(line);
	if (f.size() < 9) LOG_ERROR();
	std::unique_ptr<Light> l;
	if (f[1] == "point_light" || f[1] == "point") { auto p = std::make_unique<PointLight>(); p->pos = legacy3(f, 2); l = std::move(p); }
	else if (f[1] == "distant_light" || f[1] == "distant") { auto p = std::make_unique<DistantLight>(); p->dir = legacy3(f, 2); l = std::move(p); }
	else LOG_ERROR();
	l->color = legacy3(f, 5);
	l->intensity = strToFloat(f[8]);
	sc.lights.push_back(std::move(l));
}

void parseLegacyObject(Scene& sc, const std::string& line)
{
	const auto f = legacyFields(line);
	if (f.size() < 2) LOG_ERROR();
	if (f[1] == "plane") {
		if (f.size() < 11) LOG_ERROR();
		auto p = std::make_unique<Plane>();
		p->pos = legacy3(f, 2); p->normal = legacy3(f, 5); p->color = legacy3(f, 8);
		if (f.size() > 11) legacyMaterial(*p, f[11]);
		sc.objects.push_back(std::move(p));
	}
	else if (f[1] == "sphere") {
		if (f.size() < 9) LOG_ERROR();
		auto p = std::make_unique<Sphere>();
		p->pos = legacy3(f, 2); p->r = strToFloat(f[5]); p->r2 = p->r * p->r; p->color = legacy3(f, 6);
		if (f.size() > 9) legacyMaterial(*p, f[9]);
		sc.objects.push_back(std::move(p));
	}
	else if (f[1] == "mesh") {
		if (f.size() < 9) LOG_ERROR();
		auto p = std::make_unique<Mesh>();
		p->pos = legacy3(f, 3); p->size = legacy3(f, 6);
		if (f.size() >= 12) p->color = legacy3(f, 9);
		if (f.size() > 12) legacyMaterial(*p, f[12]);
		p->loadOBJ(f[2], sc.options);
		sc.objects.push_back(std::move(p));
	}
	else LOG_ERROR();
}

} // namespace

Scene::Scene(const std::string& sceneName) { sceneLoadSuccess = loadScene(sceneName); }


bool Scene::loadScene(const std::string& scenePath)
{
	if (options::enableOutput) std::cout << "Loading scene " << scenePath << '\n';
	const unsigned hw = std::thread::hardware_concurrency();
	if (hw != 0) options.nWorkers = (int)hw;
	std::ifstream in(scenePath);
	if (!in.good()) {
		std::cout << "Could not open scene file: " << scenePath << '\n';
		LOG_ERROR();
	}
	enum class Block { None, Options, Light, Object } block = Block::None;
	std::unique_ptr<Light> light;
	std::unique_ptr<Object> object;
	bool legacyBlock = false;     // the current [light]/[object] block held legacy one-line entities
	// a block is committed when the next line containing '[' is read (scene.cpp:96-107)
	auto commit = [&]() {
		if (block == Block::Light) { if (light) lights.push_back(std::move(light)); else if (!legacyBlock) LOG_ERROR(); }
		else if (block == Block::Object) { if (object) objects.push_back(std::move(object)); else if (!legacyBlock) LOG_ERROR(); }
		legacyBlock = false;
	};
	std::string line;
	while (in.good()) {
		std::getline(in, line);
		if (line.empty()) continue;
		if (contains(line, "[")) commit();
		if (contains(line, "#[")) {                        // commented-out block: skip to the next live header
			do { std::getline(in, line); } while (in.good() && (!contains(line, "[") || contains(line, "#[")));
			if (!in.good()) break;
		}
		if (contains(line, "#")) line.erase(line.find('#'));
		if (line.empty()) continue;
		if (line[0] == '[') {
			if (line == "[options]") block = Block::Options;
			else if (line == "[light]") block = Block::Light;
			else if (line == "[object]") block = Block::Object;
			else if (line == "[end]") break;
			else LOG_ERROR();
			continue;
		}
		switch (block) {
		case Block::Options: parseOption(*this, splitKeyValue(line, true)); break;
		case Block::Light:
			if (!contains(line, "=") && contains(line, ",")) { parseLegacyLight(*this, line); legacyBlock = true; }
			else parseLight(light, splitKeyValue(line, false));
			break;
		case Block::Object:
			if (!contains(line, "=") && contains(line, ",")) { parseLegacyObject(*this, line); legacyBlock = true; }
			else parseObject(*this, object, splitKeyValue(line, false));
			break;
		case Block::None: break;
		}
	}
	if (options::useSkybox) loadSkybox();
	return true;
}

void Scene::loadSkybox()
{
	if (!options::useSkybox) return;
	for (int k = 0; k < 6; ++k) {
		int w = 0, h = 0;
		std::unique_ptr<unsigned char[]> px(loadBMP(options.skyboxNames[k], w, h));
		if (k > 0 && (w != skyboxWidth || h != skyboxHeight)) {      // the lookup uses one size for all six faces (scene.cpp:383-385)
			std::cout << "Skybox faces differ in size: " << options.skyboxNames[k] << '\n';
			noteError("skybox faces differ in size");
			LOG_ERROR();
		}
		skyboxWidth = w; skyboxHeight = h;
		skyboxes[k].resize((size_t)w * h);
		if (!skyboxes[k].empty()) decodeColourTexels(px.get(), skyboxes[k].size(), &skyboxes[k][0].x);      // scene.cpp:354
	}
}

std::vector<tileInfo> Scene::getTiles()
{
	// 128x128 tiles, column-major, x1/y1 clamped to W-1/H-1 (scene.cpp:362-379).  The GPU path does not use
	// them for scheduling (it shards by rows and renders 8x8 wave tiles); they define which pixels exist.
	const size_t ts = 128;
	std::vector<tileInfo> tiles;
	for (size_t i = 0; i < options.width / ts + 1; ++i)
		for (size_t j = 0; j < options.height / ts + 1; ++j) {
			tileInfo t{ i * ts, std::min((i + 1) * ts, options.width - 1), j * ts, std::min((j + 1) * ts, options.height - 1) };
			if (t.x1 > t.x0 && t.y1 > t.y0) tiles.push_back(t);
		}
	return tiles;
}

// ------------------------------------------------------------------------------------------------
// flattening: Scene -> rtx_scene_desc (the arrays stay alive inside FlatScene)
// ------------------------------------------------------------------------------------------------
struct FlatScene {
	rtx_scene_desc desc{};
	std::vector<rtx_object> objects;
	std::vector<rtx_mesh> meshes;
	std::vector<rtx_light> lights;
	struct MeshArrays {
		std::vector<float> bounds, pos, nrm, uv, tb, diffuse, normal, specular;
		std::vector<int32_t> skip, leafBegin, leafCount;
	};
	std::vector<std::unique_ptr<MeshArrays>> meshArrays;
	std::vector<std::vector<float>> lightPoints;
};

void viewScaleAspect(float fov, size_t width, size_t height, float& scale, float& aspect)
{
	scale = tanf(fov * 0.5f / 180.0f * (float)(3.14159265358979323846));   // scene.cpp:447
	aspect = (width) / (float)height;                                      // scene.cpp:448
}

namespace {

void put3(float* d, const Vec3f& v) { d[0] = v.x; d[1] = v.y; d[2] = v.z; }

// the object's record in the description (mesh: its index among the meshes)
rtx_object objectRecord(const Object& o, int32_t mesh)
{
	rtx_object ro{};
	ro.type = o.objectType == ObjectType::Sphere ? RTX_OBJ_SPHERE : (o.objectType == ObjectType::Plane ? RTX_OBJ_PLANE : RTX_OBJ_MESH);
	ro.material = (int32_t)o.materialType;
	put3(ro.pos, o.pos); put3(ro.color, o.color);
	ro.ior = o.indexOfRefraction; ro.ambient = o.ambient; ro.diffuse = o.diffuse; ro.specular = o.specular; ro.n_specular = o.nSpecular;
	ro.mesh = -1;
	if (o.objectType == ObjectType::Sphere) ro.radius2 = static_cast<const Sphere&>(o).r2;
	else if (o.objectType == ObjectType::Plane) put3(ro.normal, static_cast<const Plane&>(o).normal);
	else ro.mesh = mesh;
	return ro;
}

void fillView(Scene& sc, rtx_view& v)
{
	sc.camera.ensureMatrix();
	v.width = (uint32_t)sc.options.width; v.height = (uint32_t)sc.options.height;
	v.bias = sc.options.bias; v.max_ray_depth = sc.options.maxRayDepth;
	put3(v.background, sc.options.backgroundColor);
	v.flags = (sc.cullingOn() ? RTX_FLAG_BACKFACE_CULL : 0u) | (sc.skyboxOn() ? RTX_FLAG_SKYBOX : 0u) | (sc.normalsOn() ? RTX_FLAG_SHOW_NORMALS : 0u);
	put3(v.cam_pos, sc.camera.pos);
	for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) v.cam_matrix[i * 4 + j] = sc.camera.rMatrix[i][j];
	viewScaleAspect(sc.camera.fov, sc.options.width, sc.options.height, v.scale, v.aspect);
}

// the lights' records in the description (an area light's sample points: AreaLight::setPoints, kept alive in `points`)
void flattenLights(LightsVector& lights, std::vector<rtx_light>& out, std::vector<std::vector<float>>& points)
{
	out.clear(); points.clear();
	for (auto& lp : lights) {
		rtx_light rl{};
		put3(rl.color, lp->color); rl.intensity = lp->intensity;
		if (lp->type == LightType::DistantLight) { rl.type = RTX_LIGHT_DISTANT; put3(rl.dir, static_cast<DistantLight&>(*lp).dir); }
		else if (lp->type == LightType::PointLight) { rl.type = RTX_LIGHT_POINT; put3(rl.pos, static_cast<PointLight&>(*lp).pos); }
		else if (lp->type == LightType::AreaLight) {
			auto& al = static_cast<AreaLight&>(*lp);
			al.setPoints();
			rl.type = RTX_LIGHT_AREA; put3(rl.pos, al.pos);
			points.emplace_back(al.points.size() * 3);
			for (size_t i = 0; i < al.points.size(); ++i) put3(&points.back()[i * 3], al.points[i]);
			rl.n_points = (uint32_t)al.points.size();
		}
		else LOG_ERROR();
		out.push_back(rl);
	}
	// area-light point arrays may have been reallocated while pushing: fix the pointers up now
	size_t k = 0;
	for (auto& rl : out) if (rl.type == RTX_LIGHT_AREA) rl.points = points[k++].data();
}

} // namespace

namespace {
// A mesh's record in the description, its arrays kept alive in A.  withTree = false: the acceleration structure stays out (the device
// form of rtx_scene_set_objects builds it from the triangles).
rtx_mesh flattenMesh(const Mesh& m, FlatScene::MeshArrays& A, bool withTree)
{
	rtx_mesh rm{};
	if (withTree) {
		const auto& nodes = m.ac->nodes;
		A.bounds.resize(nodes.size() * 6); A.skip.resize(nodes.size()); A.leafBegin.resize(nodes.size()); A.leafCount.resize(nodes.size());
		for (size_t i = 0; i < nodes.size(); ++i) {
			put3(&A.bounds[i * 6], nodes[i].bounds[0]); put3(&A.bounds[i * 6 + 3], nodes[i].bounds[1]);
			A.skip[i] = nodes[i].skip; A.leafBegin[i] = nodes[i].leafBegin; A.leafCount[i] = nodes[i].leafCount;
		}
		rm.n_nodes = (uint32_t)nodes.size(); rm.n_refs = (uint32_t)m.ac->refs.size();
		rm.node_bounds = A.bounds.data(); rm.node_skip = A.skip.data(); rm.leaf_begin = A.leafBegin.data(); rm.leaf_count = A.leafCount.data();
		rm.refs = m.ac->refs.data();
	}
	const size_t nt = m.allTris.size();
	A.pos.resize(nt * 9); A.nrm.resize(nt * 9); A.uv.resize(nt * 6); A.tb.resize(nt * 6);
	for (size_t i = 0; i < nt; ++i) {
		const Triangle& t = m.allTris[i];
		put3(&A.pos[i * 9], t.a); put3(&A.pos[i * 9 + 3], t.b); put3(&A.pos[i * 9 + 6], t.c);
		put3(&A.nrm[i * 9], t.n_a); put3(&A.nrm[i * 9 + 3], t.n_b); put3(&A.nrm[i * 9 + 6], t.n_c);
		A.uv[i * 6] = t.t_a.x; A.uv[i * 6 + 1] = t.t_a.y; A.uv[i * 6 + 2] = t.t_b.x; A.uv[i * 6 + 3] = t.t_b.y;
		A.uv[i * 6 + 4] = t.t_c.x; A.uv[i * 6 + 5] = t.t_c.y;
		put3(&A.tb[i * 6], t.tangent); put3(&A.tb[i * 6 + 3], t.bitangent);
	}
	rm.n_tris = (uint32_t)nt;
	rm.tri_pos = A.pos.data(); rm.tri_nrm = A.nrm.data(); rm.tri_uv = A.uv.data(); rm.tri_tb = A.tb.data();
	auto flat3 = [](const std::vector<Vec3f>& src, std::vector<float>& dst) {
		dst.resize(src.size() * 3);
		for (size_t i = 0; i < src.size(); ++i) put3(&dst[i * 3], src[i]);
	};
	if (m.diffuseMapLoaded) { flat3(m.diffuseMap, A.diffuse); rm.diffuse_w = m.diffuseMapWidth; rm.diffuse_h = m.diffuseMapHeight; rm.diffuse_map = A.diffuse.data(); }
	if (m.normalMapLoaded) { flat3(m.normalMap, A.normal); rm.normal_w = m.normalMapWidth; rm.normal_h = m.normalMapHeight; rm.normal_map = A.normal.data(); }
	if (m.specularMapLoaded) { rm.specular_w = m.specularMapWidth; rm.specular_h = m.specularMapHeight; rm.specular_map = m.specularMap.data(); }
	return rm;
}
} // namespace

FlatScene* flattenScene(Scene& sc)
{
	sc.syncTrees();
	sc.syncMaps();
	auto* fs = new FlatScene;
	fillView(sc, fs->desc.view);
	for (auto& op : sc.objects) {
		const Object& o = *op;
		rtx_object ro = objectRecord(o, (int32_t)fs->meshes.size());
		if (o.objectType == ObjectType::Mesh) {
			const Mesh& m = static_cast<const Mesh&>(o);
			if (!m.ac) { std::cout << "Mesh without acceleration structure (OBJ failed to load)\n"; LOG_ERROR(); }
			fs->meshArrays.push_back(std::make_unique<FlatScene::MeshArrays>());
			fs->meshes.push_back(flattenMesh(m, *fs->meshArrays.back(), true));
		}
		fs->objects.push_back(ro);
	}
	flattenLights(sc.lights, fs->lights, fs->lightPoints);
	fs->desc.n_objects = (uint32_t)fs->objects.size(); fs->desc.objects = fs->objects.data();
	fs->desc.n_meshes = (uint32_t)fs->meshes.size(); fs->desc.meshes = fs->meshes.data();
	fs->desc.n_lights = (uint32_t)fs->lights.size(); fs->desc.lights = fs->lights.data();
	if (sc.skyboxOn() && sc.skyboxWidth > 0) {
		fs->desc.sky_w = (uint32_t)sc.skyboxWidth; fs->desc.sky_h = (uint32_t)sc.skyboxHeight;
		for (int k = 0; k < 6; ++k) fs->desc.sky[k] = &sc.skyboxes[k][0].x;   // Vec3f is 3 packed floats
	}
	return fs;
}

const rtx_scene_desc* flatDesc(const FlatScene* fs) { return &fs->desc; }
void freeFlatScene(FlatScene* fs) { delete fs; }

// ------------------------------------------------------------------------------------------------
// GPU side
// ------------------------------------------------------------------------------------------------
namespace {
void gpuCheck(int rc, const char* what)
{
	if (rc == RTX_OK) return;
	std::cout << what << " failed: " << rtx_last_error() << '\n';
	noteError(std::string(what) + " failed: " + rtx_last_error());
	LOG_ERROR();
}
}

void Scene::invalidateView() { viewDirty_ = true; }

namespace {
void probeOne(Scene& sc, const Ray& ray, float hit[8], float colour[3])
{
	const float r[6] = { ray.orig.x, ray.orig.y, ray.orig.z, ray.dir.x, ray.dir.y, ray.dir.z };
	gpuCheck(rtx_cast_rays(sc.gpu(), 1, r, hit, colour), "rtx_cast_rays");
}
}

bool Render::trace(const Ray& ray, Scene& scene, IntersectInfo& info)
{
	if (ray.rayType != RayType::PrimaryRay) { std::cout << "Render::trace: only primary rays can be probed\n"; LOG_ERROR(); }
	float h[8], c[3];
	probeOne(scene, ray, h, c);
	info = IntersectInfo();
	if (h[0] == 0.0f) return false;
	info.hitObject = scene.objects[(size_t)h[1]].get();
	info.tNear = h[3];
	info.uv = Vec2f(h[4], h[5]);
	if (info.hitObject->objectType == ObjectType::Mesh)
		info.triPtr = &static_cast<const Mesh*>(info.hitObject)->allTris[(size_t)h[2]];
	return true;
}

Vec3f Render::castRay(const Ray& ray, Scene& scene, const int depth)
{
	if (depth != 0) { std::cout << "Render::castRay: depth must be 0 at the API boundary\n"; LOG_ERROR(); }
	float h[8], c[3];
	probeOne(scene, ray, h, c);
	return Vec3f(c[0], c[1], c[2]);
}

rtx_scene* Scene::gpu()
{
	if (!gpu_) {
		FlatScene* fs = flattenScene(*this);
		const int rc = rtx_scene_create(flatDesc(fs), device, &gpu_);
		freeFlatScene(fs);
		gpuCheck(rc, "rtx_scene_create");
		viewDirty_ = false;
	}
	if (viewDirty_) {
		rtx_view v{};
		fillView(*this, v);
		gpuCheck(rtx_scene_set_view(gpu_, &v), "rtx_scene_set_view");
		viewDirty_ = false;
	}
	return gpu_;
}

namespace {
void hipCheck(hipError_t e, const char* what)
{
	if (e == hipSuccess) return;
	std::cout << what << ": " << hipGetErrorString(e) << '\n';
	noteError(std::string(what) + ": " + hipGetErrorString(e));
	LOG_ERROR();
}
}

void Scene::moveObject(size_t index, const float* pos3, const float* rot3, const float* size3, const float* radius1, const float* normal3)
{
	if (index >= objects.size()) { noteError("moveObject: object index out of range"); LOG_ERROR(); }
	Object& o = *objects[index];
	// the keys of the type's [object] block (scene.cpp:285-312)
	const char* bad = nullptr;
	if (o.objectType == ObjectType::Mesh) bad = radius1 ? "radius" : normal3 ? "normal" : nullptr;
	else if (o.objectType == ObjectType::Sphere) bad = rot3 ? "rot" : size3 ? "size" : normal3 ? "normal" : nullptr;
	else if (o.objectType == ObjectType::Plane) bad = rot3 ? "rot" : size3 ? "size" : radius1 ? "radius" : nullptr;
	else bad = "pos";
	if (bad) { noteError(std::string("moveObject: object ") + std::to_string(index) + " has no key " + bad); LOG_ERROR(); }
	if (o.objectType == ObjectType::Mesh && !static_cast<Mesh&>(o).ac) { noteError("moveObject: mesh without acceleration structure"); LOG_ERROR(); }
	auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
	for (double& t : lastMoveMs) t = 0;
	// what a failed move puts back (the triangles by swapping, not copying)
	const Vec3f keepPos = o.pos;
	float keepR = 0, keepR2 = 0;
	Vec3f keepNormal, keepRot, keepSize, keepBounds[2];
	std::vector<Triangle> keepTris;
	bool keepStale = false;
	if (o.objectType == ObjectType::Sphere) { keepR = static_cast<Sphere&>(o).r; keepR2 = static_cast<Sphere&>(o).r2; }
	if (o.objectType == ObjectType::Plane) keepNormal = static_cast<Plane&>(o).normal;
	if (o.objectType == ObjectType::Mesh) {
		auto& m = static_cast<Mesh&>(o);
		keepRot = m.rot; keepSize = m.size; keepBounds[0] = m.ac->rootBounds[0]; keepBounds[1] = m.ac->rootBounds[1];
		keepTris.swap(m.allTris);
		keepStale = m.trisStale;
	}
	auto restore = [&]() {
		o.pos = keepPos;
		if (o.objectType == ObjectType::Sphere) { static_cast<Sphere&>(o).r = keepR; static_cast<Sphere&>(o).r2 = keepR2; }
		if (o.objectType == ObjectType::Plane) static_cast<Plane&>(o).normal = keepNormal;
		if (o.objectType == ObjectType::Mesh) {
			auto& m = static_cast<Mesh&>(o);
			m.rot = keepRot; m.size = keepSize; m.ac->setBounds(keepBounds[0], keepBounds[1]);
			m.allTris.swap(keepTris);
			m.trisStale = keepStale;
		}
	};
	try {
		moveObjectApply(index, pos3, rot3, size3, radius1, normal3, now);
	}
	catch (...) {
		restore();
		throw;
	}
}

void Scene::moveObjectApply(size_t index, const float* pos3, const float* rot3, const float* size3, const float* radius1, const float* normal3,
                            double (*now)())
{
	Object& o = *objects[index];
	if (pos3) o.pos = Vec3f(pos3[0], pos3[1], pos3[2]);
	if (o.objectType == ObjectType::Sphere && radius1) {
		auto& sp = static_cast<Sphere&>(o);
		sp.r = radius1[0];
		sp.r2 = sp.r * sp.r;          // as the loader computes it (scene.cpp:294)
	}
	if (o.objectType == ObjectType::Plane && normal3) static_cast<Plane&>(o).normal = Vec3f(normal3[0], normal3[1], normal3[2]);
	int32_t meshIndex = -1;
	if (o.objectType == ObjectType::Mesh) {
		meshIndex = 0;
		for (size_t i = 0; i < index; ++i) meshIndex += objects[i]->objectType == ObjectType::Mesh;
		auto& m = static_cast<Mesh&>(o);
		if (rot3) m.rot = Vec3f(rot3[0], rot3[1], rot3[2]);
		if (size3) m.size = Vec3f(size3[0], size3[1], size3[2]);
		const double t0 = now();
		m.place(options);
		m.trisStale = false;
		lastMoveMs[0] = now() - t0;
		if (!gpu_) {
			m.treeOnDevice = false;
			if (!m.ac->setup(m.allTris, options)) { noteError("moveObject: the acceleration structure could not be built"); LOG_ERROR(); }
		}
	}
	if (!gpu_) return;
	const rtx_object ro = objectRecord(o, meshIndex);
	double t0 = now();
	gpuCheck(rtx_scene_set_object(gpu_, (uint32_t)index, &ro), "rtx_scene_set_object");
	lastMoveMs[2] = now() - t0;
	if (o.objectType != ObjectType::Mesh) return;
	auto& m = static_cast<Mesh&>(o);
	t0 = now();
	// the placed triangles in the description's layout (flattenScene): positions, normals, tangent + bitangent
	const size_t nt = m.allTris.size();
	std::vector<float> host(nt * 24);
	float* pos = host.data(); float* nrm = pos + nt * 9; float* tb = nrm + nt * 9;
	for (size_t i = 0; i < nt; ++i) {
		const Triangle& t = m.allTris[i];
		put3(&pos[i * 9], t.a); put3(&pos[i * 9 + 3], t.b); put3(&pos[i * 9 + 6], t.c);
		put3(&nrm[i * 9], t.n_a); put3(&nrm[i * 9 + 3], t.n_b); put3(&nrm[i * 9 + 6], t.n_c);
		put3(&tb[i * 6], t.tangent); put3(&tb[i * 6 + 3], t.bitangent);
	}
	const float lo[3] = { m.ac->rootBounds[0].x, m.ac->rootBounds[0].y, m.ac->rootBounds[0].z };
	const float hi[3] = { m.ac->rootBounds[1].x, m.ac->rootBounds[1].y, m.ac->rootBounds[1].z };
	hipCheck(hipSetDevice(device), "hipSetDevice");
	float* dev = nullptr;
	if (nt) {
		hipCheck(hipMalloc((void**)&dev, host.size() * sizeof(float)), "hipMalloc");
		const hipError_t e = hipMemcpy(dev, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice);
		if (e != hipSuccess) { (void)hipFree(dev); hipCheck(e, "hipMemcpy"); }
	}
	lastMoveMs[1] = now() - t0;
	t0 = now();
	const int rc = rtx_scene_update_mesh(gpu_, (uint32_t)meshIndex, dev, nt ? dev + nt * 9 : nullptr, nt ? dev + nt * 18 : nullptr, lo, hi, options.acPenalty, nullptr);
	lastMoveMs[3] = now() - t0;
	if (dev) (void)hipFree(dev);
	gpuCheck(rc, "rtx_scene_update_mesh");
	m.treeOnDevice = true;
	float ms[4];
	if (rtx_scene_edit_times(gpu_, ms) == RTX_OK) { m.ac->buildMs = ms[0]; m.ac->builtOnDevice = true; }
}

// The vertices (and normals) of a mesh replaced (scene.h).  The host's copy of the inputs gives objP / objN and, by the loader's sequential
// rule, objLo / objHi; the triangles come from Mesh::place on the host only where the host needs them.
void Scene::setVertices(size_t index, const float* P, size_t nP, const float* N, size_t nN, bool onDevice, void* stream)
{
	auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
	const double tStart = now();
	for (double& t : lastDeformMs) t = 0;
	if (index >= objects.size()) { noteError("setVertices: object index out of range"); LOG_ERROR(); }
	if (objects[index]->objectType != ObjectType::Mesh) { noteError("setVertices: object " + std::to_string(index) + " is not a mesh"); LOG_ERROR(); }
	auto& m = static_cast<Mesh&>(*objects[index]);
	if (!m.ac || !m.hasFaces) { noteError("setVertices: a mesh without faces"); LOG_ERROR(); }
	if (!P || nP != m.objP.size()) { noteError("setVertices: the mesh has " + std::to_string(m.objP.size()) + " vertices, got " + std::to_string(nP)); LOG_ERROR(); }
	if (N && nN != m.objN.size()) { noteError("setVertices: the mesh has " + std::to_string(m.objN.size()) + " normals, got " + std::to_string(nN)); LOG_ERROR(); }
	// the host's copy of the inputs (12 bytes per vertex; the triangles never come down)
	std::vector<Vec3f> newP(nP), newN(N ? nN : 0);
	if (onDevice) {
		hipCheck(hipSetDevice(device), "hipSetDevice");
		if (stream) hipCheck(hipStreamSynchronize((hipStream_t)stream), "hipStreamSynchronize");
		if (nP) hipCheck(hipMemcpy(newP.data(), P, nP * sizeof(Vec3f), hipMemcpyDeviceToHost), "hipMemcpy (vertices)");
		if (N && nN) hipCheck(hipMemcpy(newN.data(), N, nN * sizeof(Vec3f), hipMemcpyDeviceToHost), "hipMemcpy (normals)");
	}
	else {
		if (nP) memcpy(newP.data(), P, nP * sizeof(Vec3f));
		if (N && nN) memcpy(newN.data(), N, nN * sizeof(Vec3f));
	}
	auto finite3 = [](const Vec3f& v) { return std::isfinite(v.x) && std::isfinite(v.y) && std::isfinite(v.z); };
	for (const Vec3f& v : newP) if (!finite3(v)) { noteError("setVertices: a vertex is not finite"); LOG_ERROR(); }
	for (const Vec3f& v : newN) if (!finite3(v)) { noteError("setVertices: a normal is not finite"); LOG_ERROR(); }
	const double tCopied = now();
	for (Vec3f& n : newN) n.normalize();      // (as the loader stores a vn line)
	// the running box of the vertices read before the first face (objects.cpp:231-246)
	const float big = std::numeric_limits<float>::max(), tiny = std::numeric_limits<float>::min();
	Vec3f lo(big), hi(tiny);
	for (size_t i = 0; i < m.placedP; ++i) {
		const Vec3f& v = newP[i];
		lo.x = std::min(v.x, lo.x); lo.y = std::min(v.y, lo.y); lo.z = std::min(v.z, lo.z);
		hi.x = std::max(v.x, hi.x); hi.y = std::max(v.y, hi.y); hi.z = std::max(v.z, hi.z);
	}
	// what a refusal puts back (by swapping, not copying)
	const Vec3f keepLo = m.objLo, keepHi = m.objHi, keepBounds[2] = { m.ac->rootBounds[0], m.ac->rootBounds[1] };
	const bool keepStale = m.trisStale;
	std::vector<Triangle> keepTris;
	m.objP.swap(newP);
	if (N) m.objN.swap(newN);
	m.objLo = lo; m.objHi = hi;
	auto restore = [&]() {
		m.objP.swap(newP);
		if (N) m.objN.swap(newN);
		m.objLo = keepLo; m.objHi = keepHi; m.ac->setBounds(keepBounds[0], keepBounds[1]);
		m.trisStale = keepStale;
	};
	const double tMirrored = now();
	if (!gpu_) {
		keepTris.swap(m.allTris);
		try {
			m.place(options);
			for (const Triangle& t : m.allTris)
				if (!finite3(t.a) || !finite3(t.b) || !finite3(t.c)) { noteError("setVertices: a placed position is not finite (a flat axis away from zero)"); LOG_ERROR(); }
			m.trisStale = false;
			m.treeOnDevice = false;
			if (!m.ac->setup(m.allTris, options)) { noteError("setVertices: the acceleration structure could not be built"); LOG_ERROR(); }
		}
		catch (...) {
			m.allTris.swap(keepTris);
			restore();
			throw;
		}
		lastDeformMs[2] = (tMirrored - tCopied) + (onDevice ? tCopied - tStart : 0);
		lastDeformMs[3] = now() - tStart;
		return;
	}
	float* dev = nullptr;
	try {
		uint32_t meshIndex = 0;
		for (size_t i = 0; i < index; ++i) meshIndex += objects[i]->objectType == ObjectType::Mesh;
		hipCheck(hipSetDevice(device), "hipSetDevice");
		if (!m.topologyOnDevice || (!N && m.topologyNormalsStale)) {
			// once per mesh: the corners, the uv and the stored normals (again when a call without normals follows one that replaced them)
			const size_t nt = m.corners.size();
			std::vector<uint32_t> cv(nt * 3);
			std::vector<int32_t> cn(nt * 3), ct(nt * 3);
			for (size_t i = 0; i < nt; ++i)
				for (int k = 0; k < 3; ++k) { cv[i * 3 + k] = m.corners[i].v[k]; cn[i * 3 + k] = m.corners[i].n[k]; ct[i * 3 + k] = m.corners[i].t[k]; }
			rtx_mesh_topology t{};
			t.n_tris = (uint32_t)nt; t.n_pos = (uint32_t)m.objP.size(); t.n_nrm = (uint32_t)m.objN.size(); t.n_uv = (uint32_t)m.objT.size();
			t.placed_pos = (uint32_t)m.placedP; t.placed_nrm = (uint32_t)m.placedN;
			t.corner_pos = cv.data(); t.corner_nrm = cn.data(); t.corner_uv = ct.data();
			t.uv = m.objT.empty() ? nullptr : &m.objT[0].x;
			// (the normals as they were stored before this call: what a call without normals keeps)
			const std::vector<Vec3f>& stored = N ? newN : m.objN;
			t.nrm = stored.empty() ? nullptr : &stored[0].x;
			gpuCheck(rtx_scene_set_mesh_topology(gpu_, meshIndex, &t), "rtx_scene_set_mesh_topology");
			m.topologyOnDevice = true;
			m.topologyNormalsStale = false;
		}
		const float* Pdev = P;
		const float* Ndev = N;
		if (!onDevice) {
			// a host array goes up as vertices, never as triangles
			const size_t nf = (nP + (N ? nN : 0)) * 3;
			hipCheck(hipMalloc((void**)&dev, std::max<size_t>(nf, 1) * sizeof(float)), "hipMalloc");
			hipCheck(hipMemcpy(dev, P, nP * 3 * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy");
			if (N && nN) hipCheck(hipMemcpy(dev + nP * 3, N, nN * 3 * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy");
			Pdev = dev; Ndev = N ? dev + nP * 3 : nullptr;
		}
		rtx_mesh_pose pose{};
		put3(pose.pos, m.pos); put3(pose.size, m.size);
		const Matrix44f R = Matrix44f::fromEulerDegrees(m.rot);
		for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) pose.rot_matrix[i * 4 + j] = R[i][j];
		pose.bias = options.bias; pose.ac_penalty = options.acPenalty;
		const double t0 = now();
		const int rc = rtx_scene_deform_mesh(gpu_, meshIndex, Pdev, (uint32_t)nP, Ndev, (uint32_t)(N ? nN : 0), &pose, nullptr, nullptr, onDevice ? stream : nullptr);
		const double t1 = now();
		gpuCheck(rc, "rtx_scene_deform_mesh");
		float ms[4] = { 0, 0, 0, 0 };
		if (rtx_scene_edit_times(gpu_, ms) == RTX_OK) { m.ac->buildMs = ms[0]; m.ac->builtOnDevice = true; }
		lastDeformMs[1] = ms[3];
		lastDeformMs[0] = (t1 - t0) - ms[3];
	}
	catch (...) {
		if (dev) (void)hipFree(dev);
		restore();
		throw;
	}
	if (dev) (void)hipFree(dev);
	m.treeOnDevice = true;
	m.trisStale = true;
	if (N) m.topologyNormalsStale = true;
	lastDeformMs[2] = tMirrored - tStart;
	lastDeformMs[3] = now() - tStart;
}

// ------------------------------------------------------------------------------------------------
// texture maps and skybox replaced or written into (scene.h; include/rtx_texture.h)
// ------------------------------------------------------------------------------------------------
namespace {
[[noreturn]] void refuse(const std::string& what)
{
	noteError(what);
	LOG_ERROR();
}

uint32_t texChannels(int kind) { return kind == RTX_TEX_SPECULAR ? 1u : 3u; }
size_t texRowBytes(int kind, const rtx_texels& t) { return (size_t)t.width * (t.format == RTX_TEXELS_STORED ? texChannels(kind) * 4u : 3u); }
uint64_t texPitch(const rtx_texels& t) { return t.row_pitch < 0 ? 0ull - (uint64_t)t.row_pitch : (uint64_t)t.row_pitch; }

// the checks of the library (rtx_texture.hip), for the edits that stay on the host
void checkTexels(const char* who, int kind, const rtx_texels& t)
{
	const std::string w = std::string(who) + ": ";
	if (t.format != RTX_TEXELS_STORED && t.format != RTX_TEXELS_RGB8) refuse(w + "format is no RTX_TEXELS_*");
	if (!t.width || !t.height) refuse(w + "a zero width or height");
	if (!t.data_dev) refuse(w + "the texels are NULL");
	if (texPitch(t) < texRowBytes(kind, t)) refuse(w + "|row_pitch| is below one row");
}

// a checked rectangle of texels in host memory into the host map `dst` of dstW texels per row, at (x0, y0): stored texels as they are,
// bytes through the loaders' functions (objects.h)
void applyTexels(int kind, const rtx_texels& t, float* dst, uint32_t dstW, uint32_t x0, uint32_t y0)
{
	const uint32_t ch = texChannels(kind);
	for (uint32_t r = 0; r < t.height; ++r) {
		const unsigned char* src = (const unsigned char*)t.data_dev + (int64_t)r * t.row_pitch;
		float* out = dst + ((size_t)(y0 + r) * dstW + x0) * ch;
		if (t.format == RTX_TEXELS_STORED) memcpy(out, src, (size_t)t.width * ch * sizeof(float));
		else decodeTexels(kind, src, t.width, out);
	}
}

// checked texels of host memory in device memory, as they are: the bytes from the lowest row's first to the highest row's last, the record
// pointing into them with the caller's pitch.  Freed with the object (hipFree waits for the device: a queued kernel has read them by then).
struct StagedTexels {
	rtx_texels t{};
	void* dev = nullptr;
	StagedTexels() = default;
	StagedTexels(const StagedTexels&) = delete;
	~StagedTexels() { if (dev) (void)hipFree(dev); }
	void stage(int kind, const rtx_texels& in)
	{
		const size_t span = (size_t)(in.height - 1) * texPitch(in) + texRowBytes(kind, in);
		const unsigned char* first = (const unsigned char*)in.data_dev + (in.row_pitch < 0 ? (int64_t)(in.height - 1) * in.row_pitch : 0);
		hipCheck(hipMalloc(&dev, span), "hipMalloc (texels)");
		hipCheck(hipMemcpy(dev, first, span, hipMemcpyHostToDevice), "hipMemcpy (texels)");
		t = in;
		t.data_dev = (const unsigned char*)dev + ((const unsigned char*)in.data_dev - first);
	}
};

// the host copy of map `kind` of a mesh
float* mapData(Mesh& m, int kind)
{
	if (kind == RTX_TEX_DIFFUSE) return m.diffuseMap.empty() ? nullptr : &m.diffuseMap[0].x;
	if (kind == RTX_TEX_NORMAL) return m.normalMap.empty() ? nullptr : &m.normalMap[0].x;
	return m.specularMap.empty() ? nullptr : m.specularMap.data();
}
void mapSize(const Mesh& m, int kind, bool& loaded, int& w, int& h)
{
	if (kind == RTX_TEX_DIFFUSE) { loaded = m.diffuseMapLoaded; w = m.diffuseMapWidth; h = m.diffuseMapHeight; }
	else if (kind == RTX_TEX_NORMAL) { loaded = m.normalMapLoaded; w = m.normalMapWidth; h = m.normalMapHeight; }
	else { loaded = m.specularMapLoaded; w = m.specularMapWidth; h = m.specularMapHeight; }
	if (!loaded) w = h = 0;
}
// ... of another size (w = h = 0: the mesh has no such map), its texels unset
void mapResize(Mesh& m, int kind, int w, int h)
{
	const bool loaded = w > 0 && h > 0;
	const size_t n = (size_t)w * h;
	if (kind == RTX_TEX_DIFFUSE) { m.diffuseMapLoaded = loaded; m.diffuseMapWidth = w; m.diffuseMapHeight = h; m.diffuseMap.assign(n, Vec3f(0, 0, 0)); }
	else if (kind == RTX_TEX_NORMAL) { m.normalMapLoaded = loaded; m.normalMapWidth = w; m.normalMapHeight = h; m.normalMap.assign(n, Vec3f(0, 0, 0)); }
	else { m.specularMapLoaded = loaded; m.specularMapWidth = w; m.specularMapHeight = h; m.specularMap.assign(n, 0.0f); }
}
}

void Scene::syncMaps()
{
	if (!gpu_) return;
	bool any = skyStale;
	for (auto& op : objects)
		if (op->objectType == ObjectType::Mesh) { const auto& m = static_cast<const Mesh&>(*op); any = any || m.mapStale[0] || m.mapStale[1] || m.mapStale[2]; }
	if (!any) return;
	hipCheck(hipSetDevice(device), "hipSetDevice");
	hipCheck(hipDeviceSynchronize(), "hipDeviceSynchronize");      // (a write may be queued on any stream)
	uint32_t meshIndex = 0;
	for (auto& op : objects) {
		if (op->objectType != ObjectType::Mesh) continue;
		auto& m = static_cast<Mesh&>(*op);
		const uint32_t mi = meshIndex++;
		for (int kind = 0; kind < 3; ++kind) {
			if (!m.mapStale[kind]) continue;
			uint32_t w = 0, h = 0;
			const float* dev = nullptr;
			gpuCheck(rtx_scene_texture_info(gpu_, kind, mi, &w, &h, &dev), "rtx_scene_texture_info");
			mapResize(m, kind, (int)w, (int)h);
			if (dev) hipCheck(hipMemcpy(mapData(m, kind), dev, (size_t)w * h * texChannels(kind) * sizeof(float), hipMemcpyDeviceToHost), "hipMemcpy (map)");
			m.mapStale[kind] = false;
		}
	}
	if (skyStale) {
		for (uint32_t k = 0; k < 6; ++k) {
			uint32_t w = 0, h = 0;
			const float* dev = nullptr;
			gpuCheck(rtx_scene_texture_info(gpu_, RTX_TEX_SKY, k, &w, &h, &dev), "rtx_scene_texture_info");
			skyboxWidth = (int)w; skyboxHeight = (int)h;
			skyboxes[k].assign((size_t)w * h, Vec3f(0, 0, 0));
			if (dev) hipCheck(hipMemcpy(&skyboxes[k][0].x, dev, (size_t)w * h * 3 * sizeof(float), hipMemcpyDeviceToHost), "hipMemcpy (sky face)");
		}
		skyStale = false;
	}
}

void Scene::setMap(size_t index, int kind, const rtx_texels* t, bool onDevice, void* stream)
{
	if (index >= objects.size()) refuse("setMap: object index out of range");
	if (objects[index]->objectType != ObjectType::Mesh) refuse("setMap: object " + std::to_string(index) + " is not a mesh");
	if (kind < RTX_TEX_DIFFUSE || kind > RTX_TEX_SPECULAR) refuse("setMap: kind is no map of a mesh");
	auto& m = static_cast<Mesh&>(*objects[index]);
	if (t) checkTexels("setMap", kind, *t);
	// (the load's rule "normal map without tangents": the tangents come from the texture coordinates)
	if (t && kind == RTX_TEX_NORMAL && m.objT.empty()) refuse("setMap: normal map without tangents (the mesh's OBJ has no texture coordinates)");
	if (!gpu_) {
		if (onDevice) refuse("setMap: texels in device memory without a GPU scene");
		if (!t) { mapResize(m, kind, 0, 0); return; }
		std::vector<float> fresh((size_t)t->width * t->height * texChannels(kind));
		applyTexels(kind, *t, fresh.data(), t->width, 0, 0);
		mapResize(m, kind, (int)t->width, (int)t->height);
		memcpy(mapData(m, kind), fresh.data(), fresh.size() * sizeof(float));
		return;
	}
	uint32_t meshIndex = 0;
	for (size_t i = 0; i < index; ++i) meshIndex += objects[i]->objectType == ObjectType::Mesh;
	hipCheck(hipSetDevice(device), "hipSetDevice");
	StagedTexels staged;
	if (t && !onDevice) { staged.stage(kind, *t); t = &staged.t; }
	gpuCheck(rtx_scene_set_map(gpu_, meshIndex, kind, t, onDevice ? stream : nullptr), "rtx_scene_set_map");
	// the decoded map, read back once
	m.mapStale[kind] = true;
	syncMaps();
}

void Scene::setSky(const rtx_texels* faces, bool onDevice, void* stream)
{
	if (!faces && skyboxOn()) refuse("setSky: the skybox cannot be removed while useSkybox is on");
	for (int k = 0; faces && k < 6; ++k) {
		checkTexels("setSky", RTX_TEX_SKY, faces[k]);
		if (faces[k].width != faces[0].width || faces[k].height != faces[0].height || faces[k].format != faces[0].format)
			refuse("setSky: the six faces must share one size and one format");
	}
	if (!gpu_) {
		if (onDevice) refuse("setSky: texels in device memory without a GPU scene");
		std::vector<Vec3f> fresh[6];
		for (int k = 0; faces && k < 6; ++k) {
			fresh[k].assign((size_t)faces[k].width * faces[k].height, Vec3f(0, 0, 0));
			applyTexels(RTX_TEX_SKY, faces[k], &fresh[k][0].x, faces[k].width, 0, 0);
		}
		for (int k = 0; k < 6; ++k) skyboxes[k].swap(fresh[k]);
		skyboxWidth = faces ? (int)faces[0].width : 0; skyboxHeight = faces ? (int)faces[0].height : 0;
		return;
	}
	hipCheck(hipSetDevice(device), "hipSetDevice");
	if (viewDirty_) gpu();      // (the library refuses by the flags of the view it holds: a useSkybox switched off since goes up first)
	StagedTexels staged[6];
	rtx_texels dev[6];
	for (int k = 0; faces && k < 6; ++k) {
		dev[k] = faces[k];
		if (!onDevice) { staged[k].stage(RTX_TEX_SKY, faces[k]); dev[k] = staged[k].t; }
	}
	gpuCheck(rtx_scene_set_sky(gpu_, faces ? dev : nullptr, onDevice ? stream : nullptr), "rtx_scene_set_sky");
	skyStale = true;
	syncMaps();
}

void Scene::writeTexels(int kind, size_t index, uint32_t x0, uint32_t y0, const rtx_texels& t, bool onDevice, void* stream)
{
	if (kind < RTX_TEX_DIFFUSE || kind > RTX_TEX_SKY) refuse("writeTexels: kind is no RTX_TEX_*");
	Mesh* m = nullptr;
	int w = 0, h = 0;
	if (kind == RTX_TEX_SKY) {
		if (index >= 6) refuse("writeTexels: sky face out of range");
		w = skyboxWidth; h = skyboxHeight;
	}
	else {
		if (index >= objects.size()) refuse("writeTexels: object index out of range");
		if (objects[index]->objectType != ObjectType::Mesh) refuse("writeTexels: object " + std::to_string(index) + " is not a mesh");
		m = static_cast<Mesh*>(objects[index].get());
		bool loaded = false;
		mapSize(*m, kind, loaded, w, h);
	}
	// (the sizes of the host copy are those of the device's map: only writeTexels leaves the copy behind, and it changes no size)
	if (w <= 0 || h <= 0) refuse("writeTexels: there is no such map");
	checkTexels("writeTexels", kind, t);
	if (x0 >= (uint32_t)w || y0 >= (uint32_t)h || t.width > (uint32_t)w - x0 || t.height > (uint32_t)h - y0) refuse("writeTexels: the rectangle does not lie inside the map");
	if (!gpu_) {
		if (onDevice) refuse("writeTexels: texels in device memory without a GPU scene");
		applyTexels(kind, t, kind == RTX_TEX_SKY ? &skyboxes[index][0].x : mapData(*m, kind), (uint32_t)w, x0, y0);
		return;
	}
	uint32_t devIndex = (uint32_t)index;
	if (m) { devIndex = 0; for (size_t i = 0; i < index; ++i) devIndex += objects[i]->objectType == ObjectType::Mesh; }
	hipCheck(hipSetDevice(device), "hipSetDevice");
	StagedTexels staged;
	const rtx_texels* dt = &t;
	if (!onDevice) { staged.stage(kind, t); dt = &staged.t; }
	gpuCheck(rtx_scene_write_texels(gpu_, kind, devIndex, x0, y0, dt, stream), "rtx_scene_write_texels");
	if (m) m->mapStale[kind] = true; else skyStale = true;
}

const float* Scene::texture(int kind, size_t index, int& width, int& height)
{
	width = height = 0;
	if (kind < RTX_TEX_DIFFUSE || kind > RTX_TEX_SKY) refuse("texture: kind is no RTX_TEX_*");
	syncMaps();
	if (kind == RTX_TEX_SKY) {
		if (index >= 6) refuse("texture: sky face out of range");
		if (skyboxWidth <= 0 || skyboxes[index].empty()) return nullptr;
		width = skyboxWidth; height = skyboxHeight;
		return &skyboxes[index][0].x;
	}
	if (index >= objects.size()) refuse("texture: object index out of range");
	if (objects[index]->objectType != ObjectType::Mesh) refuse("texture: object " + std::to_string(index) + " is not a mesh");
	auto& m = static_cast<Mesh&>(*objects[index]);
	bool loaded = false;
	mapSize(m, kind, loaded, width, height);
	return loaded ? mapData(m, kind) : nullptr;
}

// The lights as the device should hold them now: one rtx_scene_set_lights (nothing to do before the GPU scene exists: it is created
// from the edited lights).
void Scene::lightsToDevice()
{
	if (!gpu_) return;
	std::vector<rtx_light> recs;
	std::vector<std::vector<float>> points;
	flattenLights(lights, recs, points);
	gpuCheck(rtx_scene_set_lights(gpu_, (uint32_t)recs.size(), recs.data()), "rtx_scene_set_lights");
}

namespace {
void checkLightKeys(const char* who, LightType type, const LightKeys& keys)
{
	const char* bad = lightKeyRefused(type, keys);
	if (!bad) return;
	const char* name = type == LightType::DistantLight ? "distant" : type == LightType::PointLight ? "point" : "area";
	noteError(std::string(who) + ": a " + name + " light has no key " + bad);
	LOG_ERROR();
}
}

void Scene::setLight(size_t index, const LightKeys& keys)
{
	if (index >= lights.size()) { noteError("setLight: light index out of range"); LOG_ERROR(); }
	checkLightKeys("setLight", lights[index]->type, keys);
	std::unique_ptr<Light> keep = cloneLight(*lights[index]);
	applyLightKeys(*lights[index], keys);
	try { lightsToDevice(); }
	catch (...) { lights[index] = std::move(keep); throw; }
}

size_t Scene::addLight(const std::string& type, const LightKeys& keys)
{
	std::unique_ptr<Light> light = makeLight(type);
	if (!light) { noteError("addLight: unknown light type " + type); LOG_ERROR(); }
	checkLightKeys("addLight", light->type, keys);
	applyLightKeys(*light, keys);
	lights.push_back(std::move(light));
	try { lightsToDevice(); }
	catch (...) { lights.pop_back(); throw; }
	return lights.size() - 1;
}

void Scene::removeLight(size_t index)
{
	if (index >= lights.size()) { noteError("removeLight: light index out of range"); LOG_ERROR(); }
	std::unique_ptr<Light> keep = std::move(lights[index]);
	lights.erase(lights.begin() + (std::ptrdiff_t)index);
	try { lightsToDevice(); }
	catch (...) { lights.insert(lights.begin() + (std::ptrdiff_t)index, std::move(keep)); throw; }
}

// The objects as the device should hold them now: one rtx_scene_set_objects (nothing to do before the GPU scene exists: it is created from
// the edited objects).  `before`: the objects in the device's order -- every mesh among them is kept, under its index there; a mesh that is
// not among them is new, and its placed triangles go up in the layout moveObjectApply uploads for the device to build the structure from.
void Scene::objectsToDevice(const std::vector<const Object*>& before)
{
	if (!gpu_) return;
	std::vector<std::pair<const Object*, int32_t>> oldMesh;
	for (const Object* o : before)
		if (o->objectType == ObjectType::Mesh) oldMesh.emplace_back(o, (int32_t)oldMesh.size());
	std::vector<rtx_object> recs;
	std::vector<rtx_mesh_source> srcs;
	// (at most one mesh is new: its description, its triangles on the device)
	FlatScene::MeshArrays A;
	rtx_mesh rm{};
	rtx_mesh_build build{};
	Mesh* fresh = nullptr;
	for (auto& op : objects) {
		recs.push_back(objectRecord(*op, (int32_t)srcs.size()));
		if (op->objectType != ObjectType::Mesh) continue;
		rtx_mesh_source src{};
		src.keep = -1;
		for (const auto& om : oldMesh) if (om.first == op.get()) src.keep = om.second;
		if (src.keep < 0) {
			if (fresh) { noteError("objectsToDevice: more than one new mesh"); LOG_ERROR(); }
			fresh = static_cast<Mesh*>(op.get());
			src.mesh = &rm;
		}
		srcs.push_back(src);
	}
	float* dev = nullptr;
	bool onDevice = false;
	if (fresh) {
		onDevice = !fresh->allTris.empty() && fresh->ac->nodes.empty();
		rm = flattenMesh(*fresh, A, !onDevice);
		if (onDevice) {
			const size_t nt = fresh->allTris.size();
			hipCheck(hipSetDevice(device), "hipSetDevice");
			hipCheck(hipMalloc((void**)&dev, nt * 24 * sizeof(float)), "hipMalloc");
			hipError_t e = hipMemcpy(dev, A.pos.data(), nt * 9 * sizeof(float), hipMemcpyHostToDevice);
			if (e == hipSuccess) e = hipMemcpy(dev + nt * 9, A.nrm.data(), nt * 9 * sizeof(float), hipMemcpyHostToDevice);
			if (e == hipSuccess) e = hipMemcpy(dev + nt * 18, A.tb.data(), nt * 6 * sizeof(float), hipMemcpyHostToDevice);
			if (e != hipSuccess) { (void)hipFree(dev); hipCheck(e, "hipMemcpy"); }
			build.tri_pos_dev = dev; build.tri_nrm_dev = dev + nt * 9; build.tri_tb_dev = dev + nt * 18;
			put3(build.root_lo, fresh->ac->rootBounds[0]); put3(build.root_hi, fresh->ac->rootBounds[1]);
			build.ac_penalty = options.acPenalty;
			for (auto& src : srcs) if (src.mesh == &rm) src.build = &build;
		}
	}
	const int rc = rtx_scene_set_objects(gpu_, (uint32_t)recs.size(), recs.data(), (uint32_t)srcs.size(), srcs.data(), nullptr);
	if (dev) (void)hipFree(dev);
	gpuCheck(rc, "rtx_scene_set_objects");
	if (onDevice) { fresh->treeOnDevice = true; fresh->ac->builtOnDevice = true; }
}

size_t Scene::addObject(const std::string& type, const ObjectKeys& keys, size_t at)
{
	std::unique_ptr<Object> object = makeObject(type);
	if (!object) { noteError("addObject: unknown object type " + type); LOG_ERROR(); }
	if (at == (size_t)-1) at = objects.size();
	if (at > objects.size()) { noteError("addObject: object index out of range"); LOG_ERROR(); }
	if (const char* bad = objectKeyRefused(object->objectType, keys)) { noteError("addObject: a " + type + " has no key " + bad); LOG_ERROR(); }
	// (with a live GPU scene the device builds a new mesh's structure from its placed triangles)
	applyObjectKeys(*object, keys, options, !gpu_);
	if (object->objectType == ObjectType::Mesh) {
		auto& m = static_cast<Mesh&>(*object);
		if (!m.ac) { noteError(std::string("addObject: the mesh's OBJ could not be loaded: ") + (keys.name ? keys.name : "(no name)")); LOG_ERROR(); }
		if (gpu_ && m.allTris.empty() && !m.ac->setup(m.allTris, options)) { noteError("addObject: the acceleration structure could not be built"); LOG_ERROR(); }
	}
	std::vector<const Object*> before;
	for (auto& op : objects) before.push_back(op.get());
	objects.insert(objects.begin() + (std::ptrdiff_t)at, std::move(object));
	try { objectsToDevice(before); }
	catch (...) { objects.erase(objects.begin() + (std::ptrdiff_t)at); throw; }
	return at;
}

void Scene::removeObject(size_t index)
{
	if (index >= objects.size()) { noteError("removeObject: object index out of range"); LOG_ERROR(); }
	std::vector<const Object*> before;
	for (auto& op : objects) before.push_back(op.get());
	std::unique_ptr<Object> keep = std::move(objects[index]);
	objects.erase(objects.begin() + (std::ptrdiff_t)index);
	try { objectsToDevice(before); }
	catch (...) { objects.insert(objects.begin() + (std::ptrdiff_t)index, std::move(keep)); throw; }
}

void Scene::syncTrees()
{
	int32_t meshIndex = 0;
	for (auto& op : objects) {
		if (op->objectType != ObjectType::Mesh) continue;
		auto& m = static_cast<Mesh&>(*op);
		const int32_t mi = meshIndex++;
		// (a mesh the device deformed: the host's triangles of its current vertices, by the loader's code)
		if (m.trisStale) { m.place(options); m.trisStale = false; }
		if (!m.treeOnDevice || !gpu_) continue;
		uint32_t counts[2] = { 0, 0 };
		gpuCheck(rtx_scene_mesh_read(gpu_, (uint32_t)mi, counts, nullptr, nullptr, nullptr, nullptr, nullptr), "rtx_scene_mesh_read");
		const uint32_t nn = counts[0];
		std::vector<float> bounds((size_t)nn * 6);
		std::vector<int32_t> skip(nn), lb(nn), lc(nn);
		m.ac->refs.resize(counts[1]);
		gpuCheck(rtx_scene_mesh_read(gpu_, (uint32_t)mi, counts, bounds.data(), skip.data(), lb.data(), lc.data(), m.ac->refs.data()), "rtx_scene_mesh_read");
		m.ac->nodes.resize(nn);
		// (the depth of the deepest node, the root at depth 1, as the builders count it)
		std::vector<int32_t> ends;
		int maxDepth = 0;
		for (uint32_t i = 0; i < nn; ++i) {
			auto& nd = m.ac->nodes[i];
			nd.bounds[0] = Vec3f(bounds[(size_t)i * 6], bounds[(size_t)i * 6 + 1], bounds[(size_t)i * 6 + 2]);
			nd.bounds[1] = Vec3f(bounds[(size_t)i * 6 + 3], bounds[(size_t)i * 6 + 4], bounds[(size_t)i * 6 + 5]);
			nd.skip = skip[i]; nd.leafBegin = lb[i]; nd.leafCount = lc[i];
			while (!ends.empty() && ends.back() <= (int32_t)i) ends.pop_back();
			ends.push_back(skip[i]);
			maxDepth = std::max(maxDepth, (int)ends.size());
		}
		m.ac->maxDepth = maxDepth;
		m.treeOnDevice = false;
	}
}

// The frame lives in HBM across pass 1, the Sobel mask and the 4-ray pass (one allocation per Scene, re-used by every
// render): the host sees it once, at the end.
struct Scene::DeviceFrame {
	float* fb = nullptr; uint8_t* mask = nullptr; uint8_t* bgr = nullptr;
	size_t pixels = 0;
	~DeviceFrame() { if (fb) (void)hipFree(fb); if (mask) (void)hipFree(mask); if (bgr) (void)hipFree(bgr); }
};

Scene::~Scene()
{
	frame_.reset();
	if (gpu_) rtx_scene_destroy(gpu_);
}

Scene::DeviceFrame& Scene::deviceFrame()
{
	const size_t px = options.width * options.height;
	hipCheck(hipSetDevice(device), "hipSetDevice");
	if (!frame_ || frame_->pixels != px) {
		frame_.reset(new DeviceFrame);
		hipCheck(hipMalloc((void**)&frame_->fb, px * sizeof(Vec3f)), "hipMalloc");
		hipCheck(hipMalloc((void**)&frame_->mask, px), "hipMalloc");
		hipCheck(hipMalloc((void**)&frame_->bgr, px * 3), "hipMalloc");
		frame_->pixels = px;
	}
	return *frame_;
}

void Scene::pass1OnDevice()
{
	rtx_scene* g = gpu();
	DeviceFrame& d = deviceFrame();
	gpuCheck(rtx_counters_enable(g, statisticsOn()), "rtx_counters_enable");
	gpuCheck(rtx_render_pass1(g, 0, (uint32_t)options.height, d.fb, nullptr), "rtx_render_pass1");
}

void Scene::ssaaOnDevice()
{
	rtx_scene* g = gpu();
	DeviceFrame& d = deviceFrame();
	gpuCheck(rtx_counters_enable(g, statisticsOn()), "rtx_counters_enable");
	gpuCheck(rtx_sobel(g, d.fb, 0, (uint32_t)options.height, d.mask, nullptr), "rtx_sobel");
	gpuCheck(rtx_render_ssaa(g, d.mask, 0, (uint32_t)options.height, d.fb, nullptr), "rtx_render_ssaa");
}

void Scene::readTimes()
{
	float ms = 0;
	if (rtx_last_kernel_ms(gpu_, 0, &ms) == RTX_OK) lastPass1Ms = ms;
	if (rtx_last_kernel_ms(gpu_, 1, &ms) == RTX_OK) lastSobelMs = ms;
	if (rtx_last_kernel_ms(gpu_, 2, &ms) == RTX_OK) lastSsaaMs = ms;
	if (rtx_last_kernel_ms(gpu_, 3, &ms) == RTX_OK) lastFrameMs = ms;
}

// The reference's entry points keep their meaning for a caller that owns a host framebuffer (scene.h:68-100): the
// workers write their pixels into it and leave the others alone, so the buffer is uploaded, updated and copied back.
// Scene::render() does not go through them: it keeps the frame on the device.
void Scene::launchWorkers(Vec3f* frameBuffer)
{
	Timer t("Render scene");
	DeviceFrame& d = deviceFrame();
	const size_t bytes = options.width * options.height * sizeof(Vec3f);
	hipCheck(hipMemcpy(d.fb, frameBuffer, bytes, hipMemcpyHostToDevice), "hipMemcpy");
	pass1OnDevice();
	hipCheck(hipMemcpy(frameBuffer, d.fb, bytes, hipMemcpyDeviceToHost), "hipMemcpy");
	readTimes();
}

void Scene::launchSSAA(Vec3f* frameBuffer)
{
	Timer t("MSAA");
	DeviceFrame& d = deviceFrame();
	const size_t bytes = options.width * options.height * sizeof(Vec3f);
	hipCheck(hipMemcpy(d.fb, frameBuffer, bytes, hipMemcpyHostToDevice), "hipMemcpy");
	ssaaOnDevice();
	hipCheck(hipMemcpy(frameBuffer, d.fb, bytes, hipMemcpyDeviceToHost), "hipMemcpy");
	readTimes();
}

void Scene::attachComm(rtx_comm* comm, int nRanks, int rank)
{
	comm_ = comm; nRanks_ = nRanks < 1 ? 1 : nRanks; rank_ = rank;
}

// Scene::render (scene.cpp:595-606): pass 1, the adaptive 4-ray pass, saveImage.  The frame stays in HBM; what comes
// back to the host is the BGR8 image saveImage writes (3 bytes per pixel instead of 4 x 12).  With a communicator
// attached (one process per GPU) this rank renders its own bands of rows, and the bands are collected on rank 0 with
// rtx_gather (RCCL over xGMI) -- rank 0 writes the file.
// Rows per band: about eight bands per device, between 64 and 256 rows (every band costs two halo rows; the same rule as
// rendering_amd/parallel.py band_height, measured there).
static uint32_t bandHeight(uint32_t height, uint32_t nParts)
{
	const uint32_t b = height / (8u * (nParts ? nParts : 1u)) / 64u * 64u;
	return b < 64u ? 64u : (b > 256u ? 256u : b);
}

// The showAC branch of Scene::render (scene.cpp:607-633): the heat map of the whole frame (rtx_render_ac), then saveImage.
void Scene::renderAC()
{
	if (comm_ && nRanks_ > 1) {
		std::cout << "showAC: the heat map is normalised by the maximum of the whole frame and is rendered on one GPU only\n";
		noteError("showAC with more than one rank");
		LOG_ERROR();
	}
	if (statisticsOn()) {
		std::cout << "showAC: statistics are not collected in the debug views\n";
		noteError("showAC with collectStatistics");
		LOG_ERROR();
	}
	rtx_scene* g = gpu();
	DeviceFrame& d = deviceFrame();
	{
		Timer tp("Render AC heat map");
		gpuCheck(rtx_render_ac(g, d.fb, nullptr, nullptr), "rtx_render_ac");
		hipCheck(hipDeviceSynchronize(), "hipDeviceSynchronize");
	}
	if (options::imageOutput) {
		if (options.width % 4 != 0) { std::cout << "saveImage is only defined for width % 4 == 0 (util.cpp:28-29)\n"; LOG_ERROR(); }
		gpuCheck(rtx_quantize_bgr8(g, d.fb, d.bgr, nullptr), "rtx_quantize_bgr8");
		std::vector<unsigned char> bgr(options.width * options.height * 3);
		hipCheck(hipMemcpy(bgr.data(), d.bgr, bgr.size(), hipMemcpyDeviceToHost), "hipMemcpy");
		saveImageBGR(bgr.data(), options);
	}
	if (options::enableOutput) std::cout << '\n';
}

void Scene::render()
{
	if (!sceneLoadSuccess) return;
	Timer t("Total time");
	if (!options::useAC) {
		std::cout << "useAC=0 (every box test forced to pass) is a debug mode outside the accelerated hot path\n";
		LOG_ERROR();
	}
	// showAC first, as in the reference (scene.cpp:601); showNormals is a flag of the view (fillView) and takes the ordinary path
	if (acOn()) { renderAC(); return; }
	if (normalsOn() && statisticsOn()) {
		std::cout << "showNormals: statistics are not collected in the debug views\n";
		noteError("showNormals with collectStatistics");
		LOG_ERROR();
	}
	rtx_scene* g = gpu();
	DeviceFrame& d = deviceFrame();
	const bool sharded = comm_ && nRanks_ > 1;
	gpuCheck(rtx_set_row_ownership(g, sharded ? bandHeight((uint32_t)options.height, (uint32_t)nRanks_) : 0u, (uint32_t)nRanks_, (uint32_t)rank_, 1), "rtx_set_row_ownership");
	hipCheck(hipMemset(d.fb, 0, options.width * options.height * sizeof(Vec3f)), "hipMemset");    // new Vec3f[H*W]() (scene.cpp:599)
	// With other ranks waiting for this one's bands, a failure of ANY stage must not simply exit (the others would hang in rtx_gather):
	// the verdicts of the stages are collected in rc, and the ranks agree on them once, immediately before the gather.
	int rc = RTX_OK;
	auto stage = [&](int r, const char* what) { if (sharded) { if (rc == RTX_OK && r != RTX_OK) { rc = r; std::cout << "rank " << rank_ << ": " << what << ": " << rtx_last_error() << '\n'; } } else gpuCheck(r, what); };
	auto hipStage = [&](hipError_t e, const char* what) { if (sharded) { if (rc == RTX_OK && e != hipSuccess) { rc = RTX_ERR_DEVICE; std::cout << "rank " << rank_ << ": " << what << ": " << hipGetErrorString(e) << '\n'; } } else hipCheck(e, what); };
	uint32_t status = 0;
	if (options::enableSSAA && !statisticsOn()) {
		// launchWorkers + launchSSAA as one call: the stages overlap on the device (rtx_render_frame)
		Timer tp("Render scene + MSAA");
		stage(rtx_counters_enable(g, 0), "rtx_counters_enable");
		if (rc == RTX_OK) stage(rtx_render_frame(g, 0, (uint32_t)options.height, d.fb, d.mask, nullptr), "rtx_render_frame");
		// the host's synchronisation point: a single launch that gave up has been rendered again in three (include/rtx.h)
		if (rc == RTX_OK) stage(rtx_frame_status(g, &status), "rtx_frame_status");
		if (status && options::enableOutput) std::cout << "frame rendered again in three launches (single launch status " << (status & 0xffu) << ")\n";
	}
	else {
		{
			Timer tp("Render scene");
			stage(rtx_counters_enable(g, statisticsOn()), "rtx_counters_enable");
			if (rc == RTX_OK) stage(rtx_render_pass1(g, 0, (uint32_t)options.height, d.fb, nullptr), "rtx_render_pass1");
			hipStage(hipDeviceSynchronize(), "hipDeviceSynchronize");
		}
		if (options::enableSSAA) {
			Timer ts("MSAA");
			if (rc == RTX_OK) stage(rtx_sobel(g, d.fb, 0, (uint32_t)options.height, d.mask, nullptr), "rtx_sobel");
			if (rc == RTX_OK) stage(rtx_render_ssaa(g, d.mask, 0, (uint32_t)options.height, d.fb, nullptr), "rtx_render_ssaa");
			hipStage(hipDeviceSynchronize(), "hipDeviceSynchronize");
		}
	}
	readTimes();
	if (options::imageOutput || sharded) {
		if (options.width % 4 != 0) { std::cout << "saveImage is only defined for width % 4 == 0 (util.cpp:28-29)\n"; LOG_ERROR(); }
		if (rc == RTX_OK) stage(rtx_quantize_bgr8(g, d.fb, d.bgr, nullptr), "rtx_quantize_bgr8");
		if (sharded) {
			int allOk = 0;
			gpuCheck(rtx_comm_agree(comm_, rc == RTX_OK, &allOk, nullptr), "rtx_comm_agree");
			if (!allOk) { std::cout << "rank " << rank_ << ": " << (rc == RTX_OK ? "another rank failed to render its rows" : "this rank failed to render its rows") << '\n'; LOG_ERROR(); }
			gpuCheck(rtx_gather(g, comm_, d.bgr, options.width * 3, 1, 0, nullptr), "rtx_gather");
		}
		hipCheck(hipDeviceSynchronize(), "hipDeviceSynchronize");
		if (options::imageOutput && rank_ == 0) {
			std::vector<unsigned char> bgr(options.width * options.height * 3);
			hipCheck(hipMemcpy(bgr.data(), d.bgr, bgr.size(), hipMemcpyDeviceToHost), "hipMemcpy");
			saveImageBGR(bgr.data(), options);
		}
	}
	// launchWorkers / launchSSAA (the reference's entry points) render ALL rows: the sharding is this call's own business
	if (sharded) gpuCheck(rtx_set_row_ownership(g, 0u, 1u, 0u, 1), "rtx_set_row_ownership");
	if (statisticsOn()) {
		rtx_counters c{};
		if (rtx_counters_read(gpu(), &c) == RTX_OK) {
			stats::raysCasted = c.rays; stats::accelStructTests = c.box_tests; stats::rayTriTests = c.tri_tests;
		}
		stats::printStats();
	}
	if (options::enableOutput) std::cout << '\n';
}
