// Loading a scene: the checks and uploads of meshes, objects and lights, chooseAnalytic / choosePlain, the analytic objects' share of the cost
// estimate, and the entry points rtx_last_error, rtx_device_count, rtx_scene_create, rtx_scene_destroy and rtx_scene_set_view.  Part of
// rtx_api.hip: uses what stands above its include there (readKnobs, chooseBoxPrune, setView, ensureWork, the declaration of prepareView,
// prepBegin / prepEnd) and uploadMeshGeometry of rtx_flatten.hip.  Opens and closes its own namespace and extern "C" blocks.
namespace {

// The fields of a mesh object's record that derive from its mesh (bx: the mesh's root box, its six floats of meshBounds).
void meshObjectRecord(const float* bx, Object& d, const Mesh& dm, const rtx_scene::SrcMesh& sm)
{
	for (int c = 0; c < 3; c++) { d.rootBox[2 * c] = bx[c]; d.rootBox[2 * c + 1] = bx[3 + c]; }
	d.fatRadius = dm.fatRadius; memcpy(d.centre, dm.centre, 12); d.radius = dm.radius;
	d.meshFlags = (dm.nNodes ? 1u : 0u) | (dm.boxesRegular ? 2u : 0u) | (dm.nWide ? 4u : 0u);
	d.nodes = dm.nodes; d.refA = dm.refA; d.refB = dm.refB; d.refC = dm.refC; d.wide = dm.wide; d.prune = dm.prune;
	d.nNodes = dm.nNodes; d.vmax = dm.vmax;
	d.srcStride = (dm.prune && sm.base) ? sm.nWide : 0u;
	// The box test inflates a slot's true box by 216 dmax |orig - v0|_inf P (pruneAlive): with the origin about a mesh size away
	// that is 216 P mesh sizes, so only meshes of small triangles gain from it; the plane test does not depend on P.
	d.pruneBoxes = (dm.prune && std::isfinite(dm.rootRec.P) && dm.rootRec.P < 1.0f / 216.0f) ? 1u : 0u;
}

// A mesh of a description, checked before anything of it is uploaded (rtx_scene_create, rtx_scene_set_objects).
int checkMesh(const rtx_mesh& m)
{
	if (!m.node_bounds || !m.node_skip || !m.leaf_begin || !m.leaf_count || (m.n_refs && !m.refs) || (m.n_tris && (!m.tri_pos || !m.tri_nrm || !m.tri_uv)))
		return fail(RTX_ERR_ARG, "mesh arrays missing");
	if (m.normal_map && !m.tri_tb) return fail(RTX_ERR_ARG, "normal map without tangents");
	return RTX_OK;
}

// What of a mesh stays when its triangles move (rtx_scene_update_mesh): uv and maps, into a bag of their own.
int uploadMeshFixed(const rtx_mesh& m, DevBag& fixed, Mesh& dm)
{
	HIPCHK(fixed.upload(m.tri_uv, (size_t)m.n_tris * 6, &dm.uv));
	HIPCHK(fixed.upload(m.diffuse_map, (size_t)m.diffuse_w * m.diffuse_h * 3, &dm.diffuse));
	HIPCHK(fixed.upload(m.normal_map, (size_t)m.normal_w * m.normal_h * 3, &dm.normal));
	HIPCHK(fixed.upload(m.specular_map, (size_t)m.specular_w * m.specular_h, &dm.specular));
	dm.dW = m.diffuse_w; dm.dH = m.diffuse_h; dm.nW = m.normal_w; dm.nH = m.normal_h; dm.sW = m.specular_w; dm.sH = m.specular_h;
	return RTX_OK;
}

// Mesh `mi` of a description as the load uploads it, for nLights lights: the geometry, normals and tangents into `owned` (what
// rtx_scene_update_mesh replaces), uv and maps into `fixed`.
int uploadMesh(rtx_scene* s, const rtx_mesh& m, uint32_t mi, uint32_t nLights, DevBag& owned, DevBag& fixed, Mesh& dm, rtx_scene::SrcMesh& sm,
               rtx_scene::MeshLeaves& leaves, float bounds[6])
{
	memset(&dm, 0, sizeof(dm));
	int rc;
	if ((rc = uploadMeshGeometry(s, m, mi, nLights, owned, dm, sm, leaves, bounds))) return rc;
	HIPCHK(owned.upload(m.tri_nrm, (size_t)m.n_tris * 9, &dm.nrm));
	HIPCHK(owned.upload(m.tri_tb, m.tri_tb ? (size_t)m.n_tris * 6 : 0, &dm.tb));
	return uploadMeshFixed(m, fixed, dm);
}

// A mesh's triangle positions kept beside it for rtx_texel_points (rtx_scene::meshTriPos): nTris x 9 floats from host or device memory.
int keepTriPos(DevArray<float>& kept, const float* src, uint32_t nTris, hipMemcpyKind kind)
{
	if (!nTris) return RTX_OK;
	HIPCHK(kept.reserve((size_t)nTris * 9));
	HIPCHK(hipMemcpy(kept, src, (size_t)nTris * 9 * sizeof(float), kind));
	return RTX_OK;
}

// The objects of a description, checked before anything is uploaded or replaced (rtx_scene_create, rtx_scene_set_objects).
int checkObjects(uint32_t n, const rtx_object* objects, uint32_t nMeshes)
{
	if (n && !objects) return fail(RTX_ERR_ARG, "objects is NULL");
	for (uint32_t i = 0; i < n; i++) {
		const rtx_object& o = objects[i];
		if (o.type < RTX_OBJ_SPHERE || o.type > RTX_OBJ_MESH) return fail(RTX_ERR_ARG, "bad object type");
		if (o.material < 0 || o.material > 3) return fail(RTX_ERR_ARG, "bad material");
		if (o.type == RTX_OBJ_MESH && (o.mesh < 0 || (uint32_t)o.mesh >= nMeshes)) return fail(RTX_ERR_ARG, "bad mesh index");
	}
	return RTX_OK;
}

// The object records of a description (checked: checkObjects) over the mesh records, source records and root boxes of its meshes.
std::vector<Object> objectRecords(uint32_t n, const rtx_object* objects, const std::vector<Mesh>& meshes, const std::vector<rtx_scene::SrcMesh>& sms,
                                  const std::vector<float>& meshBounds)
{
	std::vector<Object> objs(n);
	for (uint32_t i = 0; i < n; i++) {
		const rtx_object& o = objects[i];
		Object& d = objs[i];
		memset(&d, 0, sizeof(d));
		d.type = o.type; d.material = o.material;
		memcpy(d.pos, o.pos, 12); memcpy(d.color, o.color, 12); memcpy(d.normal, o.normal, 12);
		d.ior = o.ior; d.ambient = o.ambient; d.diffuse = o.diffuse; d.specular = o.specular; d.nSpecular = o.n_specular;
		d.r2 = o.radius2; d.mesh = o.mesh;
		if (o.type == RTX_OBJ_MESH) meshObjectRecord(&meshBounds[(size_t)o.mesh * 6], d, meshes[o.mesh], sms[o.mesh]);
	}
	return objs;
}

// The Mesh[] and Object[] arrays and the spheres' entry of the cost estimate (sb: analyticEstimate) into `bag`.
int uploadRecords(const std::vector<Mesh>& meshes, const std::vector<Object>& objs, const std::vector<float>& sb, DevBag& bag, const Mesh** devMeshes,
                  const Object** devObjs, const float** devSpheres)
{
	HIPCHK(bag.upload(sb.data(), sb.size(), devSpheres));
	HIPCHK(bag.upload(meshes.data(), meshes.size(), devMeshes));
	HIPCHK(bag.upload(objs.data(), objs.size(), devObjs));
	return RTX_OK;
}

// No object is a triangle mesh: the kernels without the walk are launched (over the current records).
void chooseAnalytic(rtx_scene* s)
{
	s->analytic = true;
	for (const Object& d : s->objectRecs) if (d.type == RTX_OBJ_MESH) s->analytic = false;
}

// The lights of a description, checked before anything is uploaded or replaced (rtx_scene_create, rtx_scene_set_lights).
int checkLights(uint32_t n, const rtx_light* lights)
{
	if (n && !lights) return fail(RTX_ERR_ARG, "lights is NULL");
	for (uint32_t i = 0; i < n; i++) {
		const rtx_light& l = lights[i];
		if (l.type < RTX_LIGHT_DISTANT || l.type > RTX_LIGHT_AREA) return fail(RTX_ERR_ARG, "bad light type");
		if (l.type == RTX_LIGHT_AREA && (!l.points || l.n_points == 0)) return fail(RTX_ERR_ARG, "area light without sample points");
	}
	return RTX_OK;
}

// The light records and the area lights' sample points into `bag`: recs = the records as the device holds them, *dev = their array.
int uploadLights(uint32_t n, const rtx_light* lights, DevBag& bag, std::vector<Light>& recs, const Light** dev)
{
	recs.resize(n);
	for (uint32_t i = 0; i < n; i++) {
		const rtx_light& l = lights[i];
		Light& d = recs[i];
		memset(&d, 0, sizeof(d));
		d.type = l.type; memcpy(d.color, l.color, 12); d.intensity = l.intensity;
		memcpy(d.dir, l.dir, 12); memcpy(d.pos, l.pos, 12);
		d.nPoints = l.n_points;
		if (l.type == RTX_LIGHT_AREA) HIPCHK(bag.upload(l.points, (size_t)l.n_points * 3, &d.points));
	}
	HIPCHK(bag.upload(recs.data(), recs.size(), dev));
	return RTX_OK;
}

// What preparing a view and the launches read of the lights beside their records: the lights that have a source copy of the prune
// records, the light terms of the first-frame estimate, the counts of the argument block.
void deriveLights(rtx_scene* s, uint32_t n, const rtx_light* lights)
{
	s->srcLightPos.clear(); s->srcLightIsPoint.clear(); s->estLights.clear();
	for (uint32_t i = 0; i < n; i++) {
		const rtx_light& l = lights[i];
		s->srcLightPos.push_back({ { l.pos[0], l.pos[1], l.pos[2] } });
		s->srcLightIsPoint.push_back(l.type == RTX_LIGHT_POINT ? 1 : 0);
		if (l.type == RTX_LIGHT_POINT) s->estLights.push_back({ { l.pos[0], l.pos[1], l.pos[2], 2.0f } });
		else if (l.type == RTX_LIGHT_DISTANT) s->estLights.push_back({ { l.dir[0], l.dir[1], l.dir[2], 1.0f } });
		// an area light casts n_points shadow rays per shaded point (scene.cpp:790-806) from about its centre: a point light whose shadow counts n_points times
		else if (l.type == RTX_LIGHT_AREA) s->estLights.push_back({ { l.pos[0], l.pos[1], l.pos[2], 2.0f + 4.0f * (float)std::min<uint32_t>(l.n_points, 4096u) } });
	}
	s->params.nLights = n;
	s->params.nSrcLights = s->knobs.sources ? std::min<uint32_t>(n, kMaxSrcLights) : 0u;
}

// The PLAIN kernel family holds while every object is Diffuse and no light an area light (over the current records).
void choosePlain(rtx_scene* s)
{
	s->plain = true;
	for (const Object& d : s->objectRecs) if (d.material != 0) s->plain = false;
	for (const Light& l : s->lightRecs) if (l.type == RTX_LIGHT_AREA) s->plain = false;
}

// The spheres' and planes' share of what preparing a view reads (rtx_scene_create; again after rtx_scene_set_object, rtx_edit.hip): the planes the
// cost estimate casts shadows on, the longest plane normal a shadow ray's origin is offset along and, returned, the spheres' entry of the estimate.
std::vector<float> analyticEstimate(rtx_scene* s, const rtx_object* objects, size_t n)
{
	std::vector<float> sb;
	s->estPlanes.clear();
	s->srcNmax = 1.0f;
	for (size_t i = 0; i < n; i++) {
		const rtx_object& o = objects[i];
		if (o.type == RTX_OBJ_PLANE) {
			s->estPlanes.push_back({ { o.pos[0], o.pos[1], o.pos[2], o.normal[0], o.normal[1], o.normal[2] } });
			const double nl = std::sqrt((double)o.normal[0] * o.normal[0] + (double)o.normal[1] * o.normal[1] + (double)o.normal[2] * o.normal[2]);
			if (!(nl <= 1e30)) s->srcNmax = INFINITY; else s->srcNmax = std::max(s->srcNmax, (float)(nl * 1.000001));
		}
		// spheres take part in the first-frame cost estimate like leaves: a mirror or a glass ball is where the deep recursions start
		if (o.type != RTX_OBJ_SPHERE || !(o.radius2 > 0) || !std::isfinite(o.radius2)) continue;
		const float r = std::sqrt(o.radius2), w = (o.material == 1 || o.material == 2) ? 4000.0f : 300.0f;
		sb.insert(sb.end(), { o.pos[0] - r, o.pos[1] - r, o.pos[2] - r, o.pos[0] + r, o.pos[1] + r, o.pos[2] + r, w, 0.0f });
	}
	s->params.srcNmax2 = s->srcNmax * s->srcNmax * 1.00001f;
	return sb;
}

} // namespace

extern "C" {

const char* rtx_last_error(void) { return gErr.c_str(); }

int rtx_device_count(int* count)
{
	if (!count) return fail(RTX_ERR_ARG, "count is NULL");
	*count = 0;
	int n = 0;
	hipError_t e = hipGetDeviceCount(&n);
	if (e != hipSuccess) return fail(RTX_ERR_NO_DEVICE, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
	*count = n;
	return RTX_OK;
}

int rtx_scene_create(const rtx_scene_desc* desc, int device, rtx_scene** out)
{
	if (!desc || !out) return fail(RTX_ERR_ARG, "desc/out is NULL");
	*out = nullptr;
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(RTX_ERR_NO_DEVICE, "no HIP device visible");
	if (device < 0 || device >= n) return fail(RTX_ERR_ARG, "device index out of range");
	HIPCHK(hipSetDevice(device));
	hipDeviceProp_t prop;
	HIPCHK(hipGetDeviceProperties(&prop, device));

	// (a scene that cannot be completed is destroyed on the way out)
	std::unique_ptr<rtx_scene, void (*)(rtx_scene*)> hold(new rtx_scene, rtx_scene_destroy);
	rtx_scene* s = hold.get();
	readKnobs(s->knobs);
	s->tileQueues.reserve(16);
	s->device = device;
	s->numCUs = prop.multiProcessorCount;
	memset(&s->params, 0, sizeof(Params));

	// meshes: nodes -> 32-byte records, leaf references -> (v0, e1, e2, tri) in three parallel arrays
	int rc;
	std::vector<Mesh> meshes(desc->n_meshes);
	s->meshOwned.resize(desc->n_meshes);
	s->meshFixed.resize(desc->n_meshes);
	s->meshTriPos.resize(desc->n_meshes);
	for (uint32_t mi = 0; mi < desc->n_meshes; mi++) {
		const rtx_mesh& m = desc->meshes[mi];
		if ((rc = checkMesh(m))) return rc;
		rtx_scene::SrcMesh sm;
		rtx_scene::MeshLeaves leaves{ nullptr, 0 };
		float bounds[6];
		// (the mesh's own allocations are what rtx_scene_update_mesh replaces; uv and maps stay for the mesh's life)
		if ((rc = uploadMesh(s, m, mi, desc->n_lights, s->meshOwned[mi], s->meshFixed[mi], meshes[mi], sm, leaves, bounds))) return rc;
		if ((rc = keepTriPos(s->meshTriPos[mi], m.tri_pos, m.n_tris, hipMemcpyHostToDevice))) return rc;
		s->meshBounds.insert(s->meshBounds.end(), bounds, bounds + 6);
		s->meshLeaves.push_back(leaves);
		s->srcMeshes.push_back(sm);
	}
	if ((rc = checkObjects(desc->n_objects, desc->objects, desc->n_meshes))) return rc;
	std::vector<Object> objs = objectRecords(desc->n_objects, desc->objects, meshes, s->srcMeshes, s->meshBounds);
	if ((rc = checkLights(desc->n_lights, desc->lights))) return rc;
	{
		const std::vector<float> sb = analyticEstimate(s, desc->objects, desc->n_objects);
		const float* dev = nullptr;
		if ((rc = uploadRecords(meshes, objs, sb, s->recordsOwned, &s->params.meshes, &s->params.objects, &dev))) return rc;
		if (!sb.empty()) s->meshLeaves.push_back({ dev, (uint32_t)(sb.size() / 8) });
	}
	s->meshRecs = meshes; s->objectRecs = objs;
	chooseAnalytic(s);
	chooseBoxPrune(s);
	s->objectDescs.assign(desc->objects, desc->objects + desc->n_objects);
	if ((rc = uploadLights(desc->n_lights, desc->lights, s->lightsOwned, s->lightRecs, &s->params.lights))) return rc;
	s->params.nObjects = desc->n_objects;
	deriveLights(s, desc->n_lights, desc->lights);
	choosePlain(s);
	if (desc->sky_w && desc->sky_h && desc->sky[0]) {
		const float* faces[6];
		for (int k = 0; k < 6; k++) {
			if (!desc->sky[k]) return fail(RTX_ERR_ARG, "skybox face missing");
			HIPCHK(s->owned.upload(desc->sky[k], (size_t)desc->sky_w * desc->sky_h * 3, &faces[k]));
		}
		HIPCHK(s->owned.upload(faces, 6, &s->params.sky));
		std::copy(faces, faces + 6, s->skyFaces);
		s->params.skyW = desc->sky_w; s->params.skyH = desc->sky_h;
	}
	if ((rc = setView(s, &desc->view))) return rc;
	if ((rc = ensureWork(s))) return rc;
	if ((rc = prepareView(s))) return rc;
	if ((rc = prepEnd(s))) return rc;
	*out = hold.release();
	return RTX_OK;
}

void rtx_scene_destroy(rtx_scene* s)
{
	if (!s) return;
	(void)hipSetDevice(s->device);
	(void)hipDeviceSynchronize();
	delete s;
}

int rtx_scene_set_view(rtx_scene* s, const rtx_view* v)
{
	if (!s || !v) return fail(RTX_ERR_ARG, "scene/view is NULL");
	int rc = setView(s, v);
	if (rc) return rc;
	s->viewSerial++;
	s->lastFused.valid = false;
	if ((rc = ensureWork(s))) return rc;
	if ((rc = prepBegin(s))) return rc;
	if ((rc = prepareView(s))) return rc;
	return prepEnd(s);
}

} // extern "C"
