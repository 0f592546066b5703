// Area-light sample grid (reference: src/lights.cpp:46-63); the other light types carry parameters only.
#include "lights.h"

void AreaLight::setPoints()
{
	if (pointsCreated) return;
	pointsCreated = true;
	const Vec3f corner = pos - (i / 2.0f) - (j / 2.0f);
	if (samples > 1) {
		for (int a = 0; a < samples; ++a)
			for (int b = 0; b < samples; ++b)
				points.push_back(corner + (i * (((float)a) / (samples - 1))) + (j * (((float)b) / (samples - 1))));
	}
	else points.push_back(pos);
}

std::unique_ptr<Light> makeLight(const std::string& type)
{
	if (type == "distant") return std::make_unique<DistantLight>();
	if (type == "point") return std::make_unique<PointLight>();
	if (type == "area") return std::make_unique<AreaLight>();
	return nullptr;
}

std::unique_ptr<Light> cloneLight(const Light& l)
{
	if (l.type == LightType::DistantLight) return std::make_unique<DistantLight>(static_cast<const DistantLight&>(l));
	if (l.type == LightType::PointLight) return std::make_unique<PointLight>(static_cast<const PointLight&>(l));
	if (l.type == LightType::AreaLight) return std::make_unique<AreaLight>(static_cast<const AreaLight&>(l));
	return nullptr;
}

const char* lightKeyRefused(LightType t, const LightKeys& k)
{
	if (k.direction && t != LightType::DistantLight) return "direction";
	if (k.position && t != LightType::PointLight) return "position";
	if (k.pos && t != LightType::AreaLight) return "pos";
	if (k.i && t != LightType::AreaLight) return "i";
	if (k.j && t != LightType::AreaLight) return "j";
	if (k.samples && t != LightType::AreaLight) return "samples";
	return nullptr;
}

void applyLightKeys(Light& light, const LightKeys& k)
{
	auto v3 = [](const float* v) { return Vec3f(v[0], v[1], v[2]); };
	if (k.color) light.color = v3(k.color);
	if (k.intensity) light.intensity = k.intensity[0];
	if (k.direction) static_cast<DistantLight&>(light).dir = v3(k.direction);
	if (k.position) static_cast<PointLight&>(light).pos = v3(k.position);
	if (k.pos || k.i || k.j || k.samples) {
		auto& a = static_cast<AreaLight&>(light);
		if (k.pos) a.pos = v3(k.pos);
		if (k.i) a.i = v3(k.i);
		if (k.j) a.j = v3(k.j);
		if (k.samples) a.samples = k.samples[0];
		a.points.clear(); a.pointsCreated = false;      // (setPoints() runs once per set of values)
	}
}
