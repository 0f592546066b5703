// Scene objects (reference: include/objects.h): Object / Sphere / Plane / Mesh / Triangle /
// AccelerationStructure with the reference's public members.  Intersection and shading live on the device;
// the host side loads, builds the acceleration structure bit-identically to objects.cpp:470-526,633-763
// and keeps it in the flat pre-order form the kernels consume.
#pragma once
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "geometry.h"
#include "options.h"

enum class ObjectType { Object, Sphere, Plane, Mesh };
enum class MaterialType { Diffuse, Reflective, Transparent, Phong };

class Object {
public:
	virtual ~Object() = default;
	ObjectType objectType = ObjectType::Object;
	Vec3f pos{ 1, 1, 1 };
	Vec3f color{ 1, 1, 1 };
	MaterialType materialType = MaterialType::Diffuse;
	float indexOfRefraction = 1.4f;
	float ambient = 0.1f;
	float diffuse = 0.1f;
	float specular = 1.0f;
	float nSpecular = 5.0f;
};
using ObjectVector = std::vector<std::unique_ptr<Object>>;

class Sphere : public Object {
public:
	Sphere() { objectType = ObjectType::Sphere; pos = Vec3f(0, 0, 0); }
	float r = 1, r2 = 1;
};

class Plane : public Object {
public:
	Plane() { objectType = ObjectType::Plane; }
	Vec3f normal{ 0, 1, 0 };   // assigned raw by the loader, never re-normalised (scene.cpp:300)
};

class Triangle {
public:
	Vec3f a, b, c;
	Vec3f n_a, n_b, n_c;
	Vec2f t_a, t_b, t_c;
	Vec3f tangent, bitangent;
};

// Flat acceleration structure: nodes in pre-order (left subtree first), leaf references in visiting order.
class AccelerationStructure {
public:
	struct Node {
		Vec3f bounds[2];
		int32_t skip = 0;        // pre-order index of the first node after this subtree
		int32_t leafBegin = -1;  // -1 for inner nodes
		int32_t leafCount = -1;
	};
	void setBounds(const Vec3f& a, const Vec3f& b) { rootBounds[0] = a; rootBounds[1] = b; }
	bool setup(const std::vector<Triangle>& tris, const Options& options);   // false: the device build failed (message printed)
	float buildMs = 0;   // device build: time of the build on the GPU (HIP events)
	bool builtOnDevice = false;
	Vec3f rootBounds[2];
	std::vector<Node> nodes;
	std::vector<uint32_t> refs;
	int maxDepth = 0;
	size_t leafCount() const;
};

class Mesh : public Object {
public:
	Mesh() { objectType = ObjectType::Mesh; }
	// buildTree = false: `ac` gets its root box only -- the GPU scene builds the structure (Scene::addObject, then treeOnDevice)
	bool loadOBJ(const std::string& filename, const Options& options, bool buildTree = true);
	bool loadDiffuseMap(const std::string& filename);
	bool loadNormalMap(const std::string& filename);
	bool loadSpecularMap(const std::string& filename);

	Vec3f size, rot;
	std::vector<Triangle> allTris;
	std::unique_ptr<AccelerationStructure> ac;

	// What the loader read, kept so that the mesh can be placed again (Scene::moveObject): the OBJ's vertices and normals as read, how many
	// of them existed when the first face was read (only those are placed -- later ones stay as read, as in the reference), the vertices'
	// box at that moment, the uv, and the corners of every triangle (0-based; n[0] / t[0] = -1: the face gave no normals / no uv).
	struct Corners { uint32_t v[3]; int32_t n[3], t[3]; };
	std::vector<Vec3f> objP, objN;
	std::vector<Vec2f> objT;
	std::vector<Corners> corners;
	size_t placedP = 0, placedN = 0;
	Vec3f objLo, objHi;
	bool hasFaces = false;
	// allTris from the above with the current pos / rot / size, and the root box of `ac` (the loader's own placement, objects.cpp:282-331)
	void place(const Options& options);
	bool treeOnDevice = false;      // the GPU scene holds the structure of allTris and `ac` an older one (Scene::syncTrees)
	// Scene::setVertices with a live GPU scene: the device placed the new vertices and allTris are an older shape's until something reads them
	// (Scene::syncTrees places them again); the GPU scene holds corners, uv and stored normals of this mesh (rtx_scene_set_mesh_topology)
	// (topologyNormalsStale: objN has been replaced since, so a call that keeps the normals sends the topology again)
	bool trisStale = false, topologyOnDevice = false, topologyNormalsStale = false;

	bool diffuseMapLoaded = false; int diffuseMapWidth = 0, diffuseMapHeight = 0; std::vector<Vec3f> diffuseMap;
	bool normalMapLoaded = false; int normalMapWidth = 0, normalMapHeight = 0; std::vector<Vec3f> normalMap;
	bool specularMapLoaded = false; int specularMapWidth = 0, specularMapHeight = 0; std::vector<float> specularMap;
	// [kind]: the GPU scene's map has been written since this copy was made (Scene::writeTexels); read back before anything reads it (Scene::syncMaps)
	bool mapStale[3] = { false, false, false };
};

// The loaders' texel arithmetic (objects.cpp:395-446, scene.cpp:292-311), each formula written once: n texels of 3 bytes, R G B as loadBMP
// returns them, into 3 n floats -- n for the specular map.  kind: RTX_TEX_* of include/rtx_texture.h (0 diffuse, 1 normal, 2 specular, 3 sky).
void decodeColourTexels(const unsigned char* rgb8, size_t n, float* out);      // byte / 256 (diffuse maps and skybox faces)
void decodeNormalTexels(const unsigned char* rgb8, size_t n, float* out);      // Vec3f(c.x*2-1, -(c.y*2-1), c.z).normalize()
void decodeSpecularTexels(const unsigned char* rgb8, size_t n, float* out);    // (c.x + c.y + c.z) / 3.0f
bool decodeTexels(int kind, const unsigned char* rgb8, size_t n, float* out);  // false: no such kind

// The values of an [object] block's keys (NULL: the key is absent).  The .scene parser applies every key=value line of a block through
// applyObjectKeys, and so does Scene::addObject: an added object is the object its block loads.  material, name and the maps are the text
// of their lines' values ("transparent,1.3"; a file name).
struct ObjectKeys {
	const float *pos = nullptr, *size = nullptr, *rot = nullptr, *color = nullptr;      // pos, color: every type; size, rot: mesh
	const char* material = nullptr;                                                     // every type
	const float *radius = nullptr, *normal = nullptr;                                   // sphere; plane
	const char *name = nullptr, *diffuse_map = nullptr, *normal_map = nullptr, *specular_map = nullptr;      // mesh
};
std::unique_ptr<Object> makeObject(const std::string& type);       // "plane" / "sphere" / "mesh" (the block's type= line); null otherwise
const char* objectKeyRefused(ObjectType type, const ObjectKeys& keys);      // the first key given that the type does not have; NULL when all fit
// Sets the given keys (all of which the type has) in the order pos, size, rot, color, material, radius | normal, name, diffuse_map,
// normal_map, specular_map: a mesh's OBJ is read and placed with the pos, size and rot set before it, as in a block that names them first.
void applyObjectKeys(Object& object, const ObjectKeys& keys, const Options& options, bool buildTree = true);
