// Editing a live scene (include/rtx_scene_edit.h): an object's record (rtx_scene_set_object), a mesh's triangles
// (rtx_scene_update_mesh), the lights (rtx_scene_set_lights) and the object and mesh lists (rtx_scene_set_objects).  A scene edited here holds what rtx_scene_create would have uploaded for the edited description: the mesh's
// structure is built again on the device with the reference's builder (rtx_bvh.hip) and flattened there with the record formulas the load runs on
// the host (rtx_flatten.hip: deviceMeshGeometry beside uploadMeshGeometry, both over rtx_flat_records.h); everything derived from the geometry that
// preparing a view reads is rebuilt.  Part of rtx_api.hip's translation unit (no kernel of its own).

#include <chrono>

#include "rtx_scene.h"

int rtxBvhBuildDevice(const float* tri_pos_dev, uint32_t n_tris, const float* root_lo, const float* root_hi, int32_t ac_penalty, int device, rtx_bvh** out);

namespace {

double wallMs()
{
	return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// Waits for everything queued on the scene: its render streams, the preparation on the null stream, the caller's `stream` (a
// device-wide synchronisation covers them all).  After it no launch reads the records an edit replaces.
int editBegin(rtx_scene* s, void* stream)
{
	HIPCHK(hipSetDevice(s->device));
	if (stream) HIPCHK(hipStreamSynchronize((hipStream_t)stream));
	HIPCHK(hipDeviceSynchronize());
	return RTX_OK;
}

// The spheres' and planes' share of the derived state, from the current descriptions (analyticEstimate, rtx_upload.hip).
int refreshAnalytic(rtx_scene* s)
{
	const std::vector<float> sb = analyticEstimate(s, s->objectDescs.data(), s->objectDescs.size());
	// (the meshes' entries come first, one per mesh; the spheres' is the one after them when there is any)
	DevArray<float> dev;
	if (!sb.empty()) {
		HIPCHK(dev.reserve(sb.size()));
		if (hipMemcpy(dev, sb.data(), sb.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) return fail(RTX_ERR_DEVICE, "hipMemcpy (sphere leaves)");
	}
	s->meshLeaves.resize(s->meshRecs.size());
	s->sphereLeafDev = std::move(dev);
	if (s->sphereLeafDev) s->meshLeaves.push_back({ s->sphereLeafDev.get(), (uint32_t)(sb.size() / 8) });
	return RTX_OK;
}

// Everything a view preparation derives from the geometry is dropped and prepared again (queued on the null stream, as
// rtx_scene_set_view does): the source copies of the prune records, the cost estimate, every cached tile list (meshTileRect reads the
// root boxes) with the frame-mode measurements made on it, the frame kept for rtx_frame_status.
int refreshView(rtx_scene* s)
{
	s->srcCamBuilt = false; s->srcLightsBuilt = false; s->srcLightFresh.clear();
	for (auto& q : s->tileQueues) { q.forget(); q.lastUse = 0; }
	s->lastFrameQueue = ~(size_t)0;
	s->viewSerial++;
	s->lastFused.valid = false;
	int rc;
	if ((rc = ensureWork(s))) return rc;
	if ((rc = prepBegin(s))) return rc;
	if ((rc = prepareView(s))) return rc;
	return prepEnd(s);
}

// The geometry of mesh `mi` from nt triangles in device memory (rtx_scene_update_mesh, a new mesh of rtx_scene_set_objects): the reference's
// builder on the device, then the flatten on the device (rtx_flatten.hip: node records, wide nodes, prune blocks and their copies for the
// lights of the moment, leaf references, leaf boxes), normals and tangents.  dm keeps its uv and maps; *built: the wall clock after the build.
int deviceMesh(rtx_scene* s, uint32_t nt, const float* tri_pos_dev, const float* tri_nrm_dev, const float* tri_tb_dev, const float* root_lo, const float* root_hi,
               int32_t ac_penalty, uint32_t mi, DevBag& owned, Mesh& dm, rtx_scene::SrcMesh& sm, rtx_scene::MeshLeaves& leaves, float box[6], double* built)
{
	int rc;
	rtx_bvh* b = nullptr;
	if ((rc = rtxBvhBuildDevice(tri_pos_dev, nt, root_lo, root_hi, ac_penalty, s->device, &b))) return rc;
	const std::unique_ptr<rtx_bvh, void (*)(rtx_bvh*)> hold(b, rtx_bvh_destroy);
	if (built) *built = wallMs();
	if ((rc = deviceMeshGeometry(s, b, tri_pos_dev, nt, mi, (uint32_t)s->srcLightPos.size(), owned, dm, sm, leaves, box))) return rc;
	HIPCHK(owned.copyFrom(tri_nrm_dev, (size_t)nt * 9, &dm.nrm));
	HIPCHK(owned.copyFrom(tri_tb_dev, (size_t)nt * 6, &dm.tb));
	return RTX_OK;
}

} // namespace

extern "C" {

int rtx_scene_set_object(rtx_scene* s, uint32_t index, const rtx_object* o)
{
	if (!s || !o) return fail(RTX_ERR_ARG, "scene/object is NULL");
	if (index >= s->objectRecs.size()) return fail(RTX_ERR_ARG, "object index out of range");
	Object d = s->objectRecs[index];
	if (o->type != d.type || o->material != d.material || (d.type == RTX_OBJ_MESH && o->mesh != d.mesh))
		return fail(RTX_ERR_ARG, "rtx_scene_set_object: type, material and mesh stay as created");
	int rc;
	if ((rc = editBegin(s, nullptr))) return rc;
	// (rtx_scene_create's fields of the description; a mesh object's derived fields stay)
	memcpy(d.pos, o->pos, 12); memcpy(d.color, o->color, 12); memcpy(d.normal, o->normal, 12);
	d.ior = o->ior; d.ambient = o->ambient; d.diffuse = o->diffuse; d.specular = o->specular; d.nSpecular = o->n_specular;
	d.r2 = o->radius2;
	HIPCHK(hipMemcpy((Object*)s->params.objects + index, &d, sizeof(Object), hipMemcpyHostToDevice));
	s->objectRecs[index] = d;
	s->objectDescs[index] = *o;
	s->lastFused.valid = false;
	// (nothing a view's preparation derives reads a mesh object's record: its geometry is rtx_scene_update_mesh's)
	if (d.type == RTX_OBJ_MESH) return RTX_OK;
	if ((rc = refreshAnalytic(s))) return rc;
	return refreshView(s);
}

int rtx_scene_update_mesh(rtx_scene* s, uint32_t mesh, const float* tri_pos_dev, const float* tri_nrm_dev, const float* tri_tb_dev,
                          const float root_lo[3], const float root_hi[3], int32_t ac_penalty, void* stream)
{
	if (!s) return fail(RTX_ERR_ARG, "scene is NULL");
	if (mesh >= s->meshRecs.size()) return fail(RTX_ERR_ARG, "mesh index out of range");
	if (!root_lo || !root_hi) return fail(RTX_ERR_ARG, "root bounds missing");
	const Mesh& old = s->meshRecs[mesh];
	const uint32_t nt = old.nTris;
	if (nt && (!tri_pos_dev || !tri_nrm_dev)) return fail(RTX_ERR_ARG, "tri_pos_dev / tri_nrm_dev missing");
	if (nt && (old.tb != nullptr) != (tri_tb_dev != nullptr))
		return fail(RTX_ERR_ARG, old.tb ? "tri_tb_dev missing: the mesh was created with tangents" : "tri_tb_dev given: the mesh was created without tangents");
	const double t0 = wallMs();
	int rc;
	if ((rc = editBegin(s, stream))) return rc;

	// 1. the reference's builder on the device, from the caller's triangles; 2. the flatten on the device (deviceMesh)
	Mesh dm;
	memset(&dm, 0, sizeof(dm));
	dm.uv = old.uv; dm.diffuse = old.diffuse; dm.normal = old.normal; dm.specular = old.specular;      // (uv and maps stay)
	dm.dW = old.dW; dm.dH = old.dH; dm.nW = old.nW; dm.nH = old.nH; dm.sW = old.sW; dm.sH = old.sH;
	rtx_scene::SrcMesh sm;
	rtx_scene::MeshLeaves leaves{ nullptr, 0 };
	float box[6];
	DevBag owned;      // (dropped with everything in it unless the edit goes through)
	double t1 = t0;
	if ((rc = deviceMesh(s, nt, tri_pos_dev, tri_nrm_dev, old.tb ? tri_tb_dev : nullptr, root_lo, root_hi, ac_penalty, mesh, owned, dm, sm, leaves, box, &t1))) return rc;
	// the objects of this mesh with their derived fields; then everything is in place on the host and goes up in two copies
	std::vector<Object> objs = s->objectRecs;
	const std::vector<float> oldBounds(s->meshBounds.begin() + (size_t)mesh * 6, s->meshBounds.begin() + (size_t)mesh * 6 + 6);
	std::copy(box, box + 6, s->meshBounds.begin() + (size_t)mesh * 6);
	for (Object& d : objs)
		if (d.type == RTX_OBJ_MESH && d.mesh == (int32_t)mesh) meshObjectRecord(&s->meshBounds[(size_t)mesh * 6], d, dm, sm);
	if (hipMemcpy((Mesh*)s->params.meshes + mesh, &dm, sizeof(Mesh), hipMemcpyHostToDevice) != hipSuccess ||
	    hipMemcpy((Object*)s->params.objects, objs.data(), objs.size() * sizeof(Object), hipMemcpyHostToDevice) != hipSuccess) {
		// (put the old records back: the scene stays as it was)
		std::copy(oldBounds.begin(), oldBounds.end(), s->meshBounds.begin() + (size_t)mesh * 6);
		(void)hipMemcpy((Mesh*)s->params.meshes + mesh, &old, sizeof(Mesh), hipMemcpyHostToDevice);
		(void)hipMemcpy((Object*)s->params.objects, s->objectRecs.data(), s->objectRecs.size() * sizeof(Object), hipMemcpyHostToDevice);
		return fail(RTX_ERR_DEVICE, "rtx_scene_update_mesh: the records could not be uploaded");
	}
	s->meshOwned[mesh].swap(owned);
	owned.clear();      // (the old geometry)
	// (the positions rtx_texel_points interpolates: as many as before, so nothing is allocated)
	if ((rc = keepTriPos(s->meshTriPos[mesh], tri_pos_dev, nt, hipMemcpyDeviceToDevice))) return rc;
	s->meshRecs[mesh] = dm; s->objectRecs.swap(objs);
	s->meshLeaves[mesh] = leaves; s->srcMeshes[mesh] = sm;
	chooseBoxPrune(s);
	const double t2 = wallMs();

	// 3. the view's preparation again (sources of the prune records, cost estimate, tile lists)
	if ((rc = refreshView(s))) return rc;
	const double t3 = wallMs();
	s->editMs[0] = (float)(t1 - t0); s->editMs[1] = (float)(t2 - t1); s->editMs[2] = (float)(t3 - t2); s->editMs[3] = (float)(t3 - t0);
	return RTX_OK;
}

// The object list and the mesh list of a live scene replaced as a whole (include/rtx_scene_edit.h).  Kept meshes move to their new
// index with everything of theirs; new ones are uploaded as the load uploads them (host form) or built on the device as rtx_scene_update_mesh
// builds them (device form); removed ones are freed.  Everything rtx_scene_create derives from the objects is derived again, and no source
// copy of any mesh's prune records survives the call: they are certified for the srcNmax of the moment, which a new plane may change.
int rtx_scene_set_objects(rtx_scene* s, uint32_t nObjects, const rtx_object* objects, uint32_t nMeshes, const rtx_mesh_source* sources, void* stream)
{
	if (!s) return fail(RTX_ERR_ARG, "scene is NULL");
	int rc;
	if (nMeshes && !sources) return fail(RTX_ERR_ARG, "meshes is NULL");
	const size_t nOld = s->meshRecs.size();
	std::vector<uint8_t> kept(nOld, 0);
	for (uint32_t mi = 0; mi < nMeshes; mi++) {
		const rtx_mesh_source& src = sources[mi];
		if (src.keep >= 0) {
			if ((size_t)src.keep >= nOld) return fail(RTX_ERR_ARG, "rtx_scene_set_objects: keep out of range");
			if (kept[src.keep]) return fail(RTX_ERR_ARG, "rtx_scene_set_objects: a mesh is kept twice");
			kept[src.keep] = 1;
			continue;
		}
		if (src.keep != -1) return fail(RTX_ERR_ARG, "rtx_scene_set_objects: keep out of range");
		if (!src.mesh) return fail(RTX_ERR_ARG, "rtx_scene_set_objects: a new mesh without its description");
		const rtx_mesh& m = *src.mesh;
		if (!src.build) { if ((rc = checkMesh(m))) return rc; continue; }
		// (there is nothing to build a tree from without triangles: an empty mesh goes the host form's way, as Scene::addObject sends it)
		if (!m.n_tris) return fail(RTX_ERR_ARG, "rtx_scene_set_objects: a mesh without triangles has no device form");
		if (!src.build->tri_pos_dev || !src.build->tri_nrm_dev || !m.tri_uv) return fail(RTX_ERR_ARG, "mesh arrays missing");
		if (m.normal_map && !src.build->tri_tb_dev) return fail(RTX_ERR_ARG, "normal map without tangents");
	}
	if ((rc = checkObjects(nObjects, objects, nMeshes))) return rc;
	if ((rc = editBegin(s, stream))) return rc;

	// 1. the new meshes, beside the scene's until everything that can fail has been done
	const uint32_t nLights = (uint32_t)s->srcLightPos.size();
	std::vector<Mesh> meshes(nMeshes);
	std::vector<DevBag> owned(nMeshes), fixed(nMeshes);
	std::vector<rtx_scene::SrcMesh> sms(nMeshes);
	std::vector<rtx_scene::MeshLeaves> leaves(nMeshes, rtx_scene::MeshLeaves{ nullptr, 0 });
	std::vector<float> bounds((size_t)nMeshes * 6);
	std::vector<std::shared_ptr<rtx_scene_mesh_deform>> deform(nMeshes);      // (a kept mesh's topology follows it: include/rtx_deform.h)
	std::vector<DevArray<float>> triPos(nMeshes);                              // (a kept mesh's follow it in step 3: include/rtx_bake.h)
	for (uint32_t mi = 0; mi < nMeshes; mi++) {
		const rtx_mesh_source& src = sources[mi];
		if (src.keep >= 0) {
			if ((size_t)src.keep < s->meshDeform.size()) deform[mi] = s->meshDeform[src.keep];
			meshes[mi] = s->meshRecs[src.keep]; sms[mi] = s->srcMeshes[src.keep]; leaves[mi] = s->meshLeaves[src.keep];
			sms[mi].meshIndex = mi;
			std::copy(s->meshBounds.begin() + (size_t)src.keep * 6, s->meshBounds.begin() + (size_t)src.keep * 6 + 6, bounds.begin() + (size_t)mi * 6);
			continue;
		}
		const rtx_mesh& m = *src.mesh;
		if (!src.build) {
			if ((rc = uploadMesh(s, m, mi, nLights, owned[mi], fixed[mi], meshes[mi], sms[mi], leaves[mi], &bounds[(size_t)mi * 6]))) return rc;
			if ((rc = keepTriPos(triPos[mi], m.tri_pos, m.n_tris, hipMemcpyHostToDevice))) return rc;
			continue;
		}
		const rtx_mesh_build& b = *src.build;
		memset(&meshes[mi], 0, sizeof(Mesh));
		if ((rc = uploadMeshFixed(m, fixed[mi], meshes[mi]))) return rc;
		if ((rc = deviceMesh(s, m.n_tris, b.tri_pos_dev, b.tri_nrm_dev, b.tri_tb_dev, b.root_lo, b.root_hi, b.ac_penalty, mi, owned[mi], meshes[mi], sms[mi], leaves[mi],
		                     &bounds[(size_t)mi * 6], nullptr))) return rc;
		if ((rc = keepTriPos(triPos[mi], b.tri_pos_dev, m.n_tris, hipMemcpyDeviceToDevice))) return rc;
	}

	// 2. the records over them, and the spheres' and planes' share of the derived state (put back if the upload fails)
	std::vector<Object> objs = objectRecords(nObjects, objects, meshes, sms, bounds);
	const std::vector<std::array<float, 6>> oldPlanes = s->estPlanes;
	const float oldNmax = s->srcNmax, oldNmax2 = s->params.srcNmax2;
	const std::vector<float> sb = analyticEstimate(s, objects, nObjects);
	DevBag records;
	const Mesh* devMeshes = nullptr; const Object* devObjs = nullptr; const float* devSpheres = nullptr;
	if ((rc = uploadRecords(meshes, objs, sb, records, &devMeshes, &devObjs, &devSpheres))) {
		s->estPlanes = oldPlanes; s->srcNmax = oldNmax; s->params.srcNmax2 = oldNmax2;
		return rc;
	}

	// 3. everything takes the old scene's place: kept meshes carry their allocations over, what is left behind is freed (nothing queued
	// reads it: editBegin)
	for (uint32_t mi = 0; mi < nMeshes; mi++)
		if (sources[mi].keep >= 0) {
			owned[mi].swap(s->meshOwned[sources[mi].keep]); fixed[mi].swap(s->meshFixed[sources[mi].keep]);
			triPos[mi] = std::move(s->meshTriPos[sources[mi].keep]);
		}
	s->meshOwned.swap(owned); s->meshFixed.swap(fixed); s->meshTriPos.swap(triPos);
	owned.clear(); fixed.clear(); triPos.clear();
	s->meshDeform.swap(deform);
	deform.clear();
	s->recordsOwned.swap(records);
	records.clear();
	s->sphereLeafDev.reset();
	s->meshRecs.swap(meshes); s->srcMeshes.swap(sms); s->meshBounds.swap(bounds); s->objectRecs.swap(objs);
	s->objectDescs.assign(objects, objects + nObjects);
	s->meshLeaves.swap(leaves);
	if (!sb.empty()) s->meshLeaves.push_back({ devSpheres, (uint32_t)(sb.size() / 8) });
	s->params.meshes = devMeshes; s->params.objects = devObjs; s->params.nObjects = nObjects;

	// 4. the kernel variant again; with another family pass 1's grid (the ray kernels' occupancy is kept per kernel: blocksPerCU)
	const bool wasAnalytic = s->analytic, wasPlain = s->plain;
	chooseAnalytic(s);
	chooseBoxPrune(s);
	choosePlain(s);
	if (s->analytic != wasAnalytic || s->plain != wasPlain)
		if ((rc = askResidentBlocks(s))) return rc;

	// 5. the view's preparation again: every source copy is built again, every tile list and frame-mode measurement forgotten
	return refreshView(s);
}

// The lights of a live scene replaced as a whole (include/rtx_scene_edit.h).  Everything rtx_scene_create derives from the
// lights is derived again: their records and sample points (a bag of their own), the number of source copies per mesh, the copies of the
// point lights, the kernel family, the light terms of the cost estimate.
int rtx_scene_set_lights(rtx_scene* s, uint32_t n, const rtx_light* lights)
{
	if (!s) return fail(RTX_ERR_ARG, "scene is NULL");
	int rc;
	if ((rc = checkLights(n, lights))) return rc;
	if ((rc = editBegin(s, nullptr))) return rc;

	// 1. the new records and sample points, beside the old ones until everything that can fail has been done
	DevBag bag;
	std::vector<Light> recs;
	const Light* dev = nullptr;
	if ((rc = uploadLights(n, lights, bag, recs, &dev))) return rc;

	// 2. the meshes' prune blocks when the number of lights with a source copy changes: copy 0 and the camera's copy are carried over
	const uint32_t oldSrc = std::min<uint32_t>((uint32_t)s->srcLightPos.size(), kMaxSrcLights), newSrc = std::min<uint32_t>(n, kMaxSrcLights);
	const bool relay = s->knobs.sources && oldSrc != newSrc;
	std::vector<PruneBlock*> fresh(s->srcMeshes.size(), nullptr);
	if (relay) {
		bool ok = true;
		for (size_t mi = 0; mi < s->srcMeshes.size() && ok; mi++) {
			const rtx_scene::SrcMesh& sm = s->srcMeshes[mi];
			if (!sm.pruneAlloc) continue;
			const size_t one = (size_t)sm.pruneWide * sizeof(PruneBlock);
			ok = s->meshOwned[mi].alloc(&fresh[mi], (2 + (size_t)newSrc) * one) == hipSuccess;
			for (uint32_t c = 0; c < 2 + newSrc && ok; c++)      // (the lights' copies: generic until buildSources)
				ok = hipMemcpy(fresh[mi] + (size_t)c * sm.pruneWide, sm.pruneAlloc + (size_t)(c == 1 ? 1 : 0) * sm.pruneWide, one, hipMemcpyDeviceToDevice) == hipSuccess;
		}
		if (!ok) {
			for (size_t mi = 0; mi < fresh.size(); mi++) s->meshOwned[mi].drop(fresh[mi]);
			return fail(RTX_ERR_DEVICE, "rtx_scene_set_lights: the prune blocks could not be laid out again");
		}
		std::vector<Mesh> meshes = s->meshRecs;
		std::vector<Object> objs = s->objectRecs;
		std::vector<rtx_scene::SrcMesh> sms = s->srcMeshes;
		for (size_t mi = 0; mi < sms.size(); mi++) {
			if (!fresh[mi]) continue;
			if (meshes[mi].prune) meshes[mi].prune = fresh[mi];
			if (sms[mi].base) sms[mi].base = fresh[mi];
			sms[mi].pruneAlloc = fresh[mi];
		}
		for (Object& d : objs)
			if (d.type == RTX_OBJ_MESH) meshObjectRecord(&s->meshBounds[(size_t)d.mesh * 6], d, meshes[d.mesh], sms[d.mesh]);
		if ((!meshes.empty() && hipMemcpy((Mesh*)s->params.meshes, meshes.data(), meshes.size() * sizeof(Mesh), hipMemcpyHostToDevice) != hipSuccess) ||
		    (!objs.empty() && hipMemcpy((Object*)s->params.objects, objs.data(), objs.size() * sizeof(Object), hipMemcpyHostToDevice) != hipSuccess)) {
			// (put the old records back: the scene stays as it was)
			if (!meshes.empty()) (void)hipMemcpy((Mesh*)s->params.meshes, s->meshRecs.data(), meshes.size() * sizeof(Mesh), hipMemcpyHostToDevice);
			if (!objs.empty()) (void)hipMemcpy((Object*)s->params.objects, s->objectRecs.data(), objs.size() * sizeof(Object), hipMemcpyHostToDevice);
			for (size_t mi = 0; mi < fresh.size(); mi++) s->meshOwned[mi].drop(fresh[mi]);
			return fail(RTX_ERR_DEVICE, "rtx_scene_set_lights: the records could not be uploaded");
		}
		for (size_t mi = 0; mi < sms.size(); mi++)
			if (fresh[mi]) s->meshOwned[mi].drop(s->srcMeshes[mi].pruneAlloc);      // (the old blocks)
		s->meshRecs.swap(meshes); s->objectRecs.swap(objs); s->srcMeshes.swap(sms);
	}

	// 3. which point lights keep their copy: same index, same position, built for the current bias, in blocks that stayed.  A copy whose
	// light is no longer a point light goes back to copy 0's content, as after a load; buildSources builds the others.
	std::vector<uint8_t> keep(newSrc, 0);
	bool allKept = s->srcLightsBuilt;
	for (uint32_t l = 0; l < newSrc && s->knobs.sources; l++) {
		const bool point = lights[l].type == RTX_LIGHT_POINT;
		keep[l] = !relay && s->srcLightsBuilt && point && s->srcLightIsPoint[l] && !memcmp(s->srcLightPos[l].data(), lights[l].pos, 12);
		if (point && !keep[l]) allKept = false;
		if (point || relay || !s->srcLightIsPoint[l]) continue;
		for (const auto& sm : s->srcMeshes)
			if (sm.base) HIPCHK(hipMemcpyAsync(sm.base + (size_t)(2 + l) * sm.nWide, sm.base, (size_t)sm.nWide * sizeof(PruneBlock), hipMemcpyDeviceToDevice, nullptr));
	}

	// 4. the new lights take the old ones' place (which are freed with `bag`: nothing queued reads them, editBegin)
	s->lightsOwned.swap(bag);
	s->lightRecs.swap(recs);
	s->params.lights = dev;
	deriveLights(s, n, lights);
	s->srcLightFresh = keep; s->srcLightsBuilt = allKept;
	if (allKept) s->srcLightFresh.clear();
	s->lastFused.valid = false;
	const bool wasPlain = s->plain;
	choosePlain(s);
	if (s->plain != wasPlain) {
		// (another kernel family: pass 1's grid, and what was measured of the frame modes with the old one)
		if ((rc = askResidentBlocks(s))) return rc;
		for (auto& q : s->tileQueues) q.forgetMeasurements();
	}
	if ((rc = ensureWork(s))) return rc;

	// 5. The view's preparation again: the sources of the new point lights and the cost estimate.  What does not depend on the lights is
	// kept -- the camera's source copy (built from the camera and the geometry), the cached tile lists (which tiles a launch lists and in
	// which queue: the view, the row range, the row ownership and the meshes' root boxes) and, within a kernel family, the frame-mode
	// measurements (they only choose between two ways of rendering the same pixels) -- so a light animation renders at a warm frame's
	// cost.  No pixel depends on any of it: tile costs only order the work.
	if ((rc = prepBegin(s))) return rc;
	if ((rc = prepareView(s))) return rc;
	return prepEnd(s);
}

// rtx_debug.h: the device's current tree of mesh `mesh` in the rtx_mesh layout (decoded from its node records and leaf references)
int rtx_scene_mesh_read(rtx_scene* s, uint32_t mesh, uint32_t* counts2, float* node_bounds, int32_t* node_skip, int32_t* leaf_begin,
                        int32_t* leaf_count, uint32_t* refs)
{
	if (!s || !counts2) return fail(RTX_ERR_ARG, "scene/counts is NULL");
	if (mesh >= s->meshRecs.size()) return fail(RTX_ERR_ARG, "mesh index out of range");
	const Mesh& dm = s->meshRecs[mesh];
	counts2[0] = dm.nNodes; counts2[1] = dm.nRefs;
	if (!node_bounds && !node_skip && !leaf_begin && !leaf_count && !refs) return RTX_OK;
	HIPCHK(hipSetDevice(s->device));
	HIPCHK(hipDeviceSynchronize());
	std::vector<Node> nodes(dm.nNodes);
	if (dm.nNodes) HIPCHK(hipMemcpy(nodes.data(), dm.nodes, nodes.size() * sizeof(Node), hipMemcpyDeviceToHost));
	for (uint32_t i = 0; i < dm.nNodes; i++) {
		const Node& nd = nodes[i];
		if (node_bounds)
			for (int c = 0; c < 3; c++) { node_bounds[(size_t)i * 6 + c] = nd.b[2 * c]; node_bounds[(size_t)i * 6 + 3 + c] = nd.b[2 * c + 1]; }
		const bool leaf = nd.link < 0;
		if (node_skip) node_skip[i] = leaf ? (int32_t)i + 1 : nd.link;
		if (leaf_begin) leaf_begin[i] = leaf ? nd.first : -1;
		if (leaf_count) leaf_count[i] = leaf ? ~nd.link : -1;
	}
	if (refs && dm.nRefs) {
		std::vector<RefA> ra(dm.nRefs);
		HIPCHK(hipMemcpy(ra.data(), dm.refA, ra.size() * sizeof(RefA), hipMemcpyDeviceToHost));
		for (uint32_t r = 0; r < dm.nRefs; r++) refs[r] = ra[r].tri;
	}
	return RTX_OK;
}

// rtx_debug.h: the device's wide nodes, prune blocks (copy 0) and root record of mesh `mesh` in rtx_mesh_flatten_probe's layout
int rtx_scene_mesh_flat_read(rtx_scene* s, uint32_t mesh, uint32_t* n_wide, void* wide_out, void* prune_out, uint32_t cap_wide, float* root_rec8)
{
	if (!s || !n_wide) return fail(RTX_ERR_ARG, "scene/n_wide is NULL");
	if (mesh >= s->meshRecs.size()) return fail(RTX_ERR_ARG, "mesh index out of range");
	const Mesh& dm = s->meshRecs[mesh];
	*n_wide = dm.nWide;
	if (root_rec8) memcpy(root_rec8, &dm.rootRec, sizeof(PruneRec));
	const size_t n = std::min<size_t>(cap_wide, dm.nWide);
	if (!n || (!wide_out && !prune_out)) return RTX_OK;
	HIPCHK(hipSetDevice(s->device));
	HIPCHK(hipDeviceSynchronize());
	if (wide_out) HIPCHK(hipMemcpy(wide_out, dm.wide, n * sizeof(WideNode), hipMemcpyDeviceToHost));
	if (prune_out) {
		if (dm.prune) HIPCHK(hipMemcpy(prune_out, dm.prune, n * sizeof(PruneBlock), hipMemcpyDeviceToHost));
		else memset(prune_out, 0, n * sizeof(PruneBlock));
	}
	return RTX_OK;
}

// rtx_debug.h: the light records and the area lights' sample points as the device holds them
int rtx_scene_lights_read(rtx_scene* s, uint32_t* n_lights, rtx_light* lights_out, uint32_t cap_lights, size_t* n_point_floats, float* points_out, size_t cap_point_floats)
{
	if (!s || !n_lights) return fail(RTX_ERR_ARG, "scene/n_lights is NULL");
	const uint32_t n = s->params.nLights;
	*n_lights = n;
	if (n_point_floats) *n_point_floats = 0;
	if (!n || (!lights_out && !n_point_floats && !points_out)) return RTX_OK;
	HIPCHK(hipSetDevice(s->device));
	HIPCHK(hipDeviceSynchronize());
	std::vector<Light> recs(n);
	HIPCHK(hipMemcpy(recs.data(), s->params.lights, n * sizeof(Light), hipMemcpyDeviceToHost));
	size_t at = 0;
	for (uint32_t i = 0; i < n; i++) {
		const Light& d = recs[i];
		if (lights_out && i < cap_lights) {
			rtx_light& l = lights_out[i];
			memset(&l, 0, sizeof(l));
			l.type = d.type; memcpy(l.color, d.color, 12); l.intensity = d.intensity; memcpy(l.dir, d.dir, 12); memcpy(l.pos, d.pos, 12);
			l.n_points = d.nPoints;      // (points stays NULL: the sample points follow one another in points_out, in light order)
		}
		if (d.type != RTX_LIGHT_AREA) continue;
		const size_t nf = (size_t)d.nPoints * 3;
		if (points_out && at + nf <= cap_point_floats && nf) HIPCHK(hipMemcpy(points_out + at, d.points, nf * sizeof(float), hipMemcpyDeviceToHost));
		at += nf;
	}
	if (n_point_floats) *n_point_floats = at;
	return RTX_OK;
}

// rtx_debug.h: the object records decoded from device memory into the description's layout
int rtx_scene_objects_read(rtx_scene* s, uint32_t* n_objects, rtx_object* objects_out, uint32_t cap_objects, uint32_t* n_meshes)
{
	if (!s || !n_objects) return fail(RTX_ERR_ARG, "scene/n_objects is NULL");
	const uint32_t n = s->params.nObjects;
	*n_objects = n;
	if (n_meshes) *n_meshes = (uint32_t)s->meshRecs.size();
	const uint32_t m = std::min(n, cap_objects);
	if (!m || !objects_out) return RTX_OK;
	HIPCHK(hipSetDevice(s->device));
	HIPCHK(hipDeviceSynchronize());
	std::vector<Object> recs(m);
	HIPCHK(hipMemcpy(recs.data(), s->params.objects, (size_t)m * sizeof(Object), hipMemcpyDeviceToHost));
	for (uint32_t i = 0; i < m; i++) {
		const Object& d = recs[i];
		rtx_object& o = objects_out[i];
		memset(&o, 0, sizeof(o));
		o.type = d.type; o.material = d.material;
		memcpy(o.pos, d.pos, 12); memcpy(o.color, d.color, 12); memcpy(o.normal, d.normal, 12);
		o.ior = d.ior; o.ambient = d.ambient; o.diffuse = d.diffuse; o.specular = d.specular; o.n_specular = d.nSpecular;
		o.radius2 = d.r2; o.mesh = d.mesh;
	}
	return RTX_OK;
}

// rtx_debug.h: copy `copy` of mesh `mesh`'s prune blocks (0 any ray, 1 the camera's, 2 + l point light l's)
int rtx_scene_mesh_prune_copy_read(rtx_scene* s, uint32_t mesh, uint32_t copy, uint32_t* n_copies, uint32_t* n_wide, void* prune_out, uint32_t cap_wide)
{
	if (!s || !n_copies || !n_wide) return fail(RTX_ERR_ARG, "scene/n_copies/n_wide is NULL");
	if (mesh >= s->srcMeshes.size()) return fail(RTX_ERR_ARG, "mesh index out of range");
	const rtx_scene::SrcMesh& sm = s->srcMeshes[mesh];
	*n_wide = sm.pruneWide;
	*n_copies = !sm.pruneAlloc ? 0u : (s->knobs.sources ? 2u + std::min<uint32_t>((uint32_t)s->srcLightPos.size(), kMaxSrcLights) : 1u);
	if (!prune_out) return RTX_OK;
	if (copy >= *n_copies) return fail(RTX_ERR_ARG, "copy out of range");
	const size_t nw = std::min<size_t>(cap_wide, sm.pruneWide);
	if (!nw) return RTX_OK;
	HIPCHK(hipSetDevice(s->device));
	HIPCHK(hipDeviceSynchronize());
	HIPCHK(hipMemcpy(prune_out, sm.pruneAlloc + (size_t)copy * sm.pruneWide, nw * sizeof(PruneBlock), hipMemcpyDeviceToHost));
	return RTX_OK;
}

// rtx_debug.h: host wall time of the stages of the last rtx_scene_update_mesh
int rtx_scene_edit_times(rtx_scene* s, float* ms4)
{
	if (!s || !ms4) return fail(RTX_ERR_ARG, "scene/ms4 is NULL");
	memcpy(ms4, s->editMs, sizeof(s->editMs));
	return RTX_OK;
}

} // extern "C"
