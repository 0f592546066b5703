// Light sources (reference: include/lights.h).  illuminate() is evaluated on the device
// (rtx_kernels.hip: ST_NEXT_LIGHT); the host classes only carry the parameters.
#pragma once
#include <memory>
#include <string>
#include <vector>

#include "geometry.h"

enum class LightType { BaseLight, DistantLight, PointLight, AreaLight };

class Light {
public:
	virtual ~Light() = default;
	Vec3f color{ 1, 1, 1 };
	float intensity = 1;
	LightType type = LightType::BaseLight;
};
using LightsVector = std::vector<std::unique_ptr<Light>>;

class DistantLight : public Light {
public:
	DistantLight() { type = LightType::DistantLight; }
	Vec3f dir{ 0, 0, -1 };   // assigned raw by the loader, never re-normalised (scene.cpp:222)
};

class PointLight : public Light {
public:
	PointLight() { type = LightType::PointLight; }
	Vec3f pos{ 0, 0, 0 };
};

class AreaLight : public Light {
public:
	AreaLight() { type = LightType::AreaLight; }
	void setPoints();        // samples x samples grid over the parallelogram (lights.cpp:46-63)
	Vec3f pos, i, j;
	int samples = 1;
	bool pointsCreated = false;
	std::vector<Vec3f> points;
};

// The values of a [light] block's keys (NULL: the key is absent).  The .scene parser applies every key=value line of a block through
// applyLightKeys, and so do the edits of a loaded scene (Scene::setLight / addLight): an edited light is the light its edited block loads.
struct LightKeys {
	const float *color = nullptr, *intensity = nullptr;                  // every type
	const float *direction = nullptr;                                    // distant
	const float *position = nullptr;                                     // point
	const float *pos = nullptr, *i = nullptr, *j = nullptr;              // area
	const int* samples = nullptr;
};
std::unique_ptr<Light> makeLight(const std::string& type);       // "distant" / "point" / "area" (the block's type= line); null otherwise
std::unique_ptr<Light> cloneLight(const Light& light);
const char* lightKeyRefused(LightType type, const LightKeys& keys);   // the first key given that the type does not have; NULL when all fit
// Sets the given keys (all of which the type has).  An area light whose pos, i, j or samples change gets its sample points again
// at the next setPoints().
void applyLightKeys(Light& light, const LightKeys& keys);
