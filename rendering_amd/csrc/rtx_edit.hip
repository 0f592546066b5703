// Editing a live scene (include/rtx_scene_edit.h): an object's record (rtx_scene_set_object) and a mesh's triangles
// (rtx_scene_update_mesh).  A scene edited here holds what rtx_scene_create would have uploaded for the edited description: the mesh's
// structure is built again on the device with the reference's builder (rtx_bvh.hip) and flattened with the very code the load runs
// (flattenMesh / uploadMeshGeometry in rtx_api.hip); everything derived from the geometry that preparing a view reads is rebuilt.
// Part of rtx_api.hip's translation unit (no kernel of its own).

#include <chrono>

int rtxBvhBuildDevice(const float* tri_pos_dev, uint32_t n_tris, const float* root_lo, const float* root_hi, int32_t ac_penalty, int device, rtx_bvh** out);

#include "rtx_flatten.hip"

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

// The spheres' and planes' share of the derived state, from the current descriptions (analyticEstimate, rtx_api.hip).
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
	s->srcCamBuilt = false; s->srcLightsBuilt = false;
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

	// 1. the reference's builder on the device, from the caller's triangles
	rtx_bvh* b = nullptr;
	if ((rc = rtxBvhBuildDevice(tri_pos_dev, nt, root_lo, root_hi, ac_penalty, s->device, &b))) return rc;
	const std::unique_ptr<rtx_bvh, void (*)(rtx_bvh*)> hold(b, rtx_bvh_destroy);
	const double t1 = wallMs();

	// 2. the flatten on the device (rtx_flatten.hip): node records, wide nodes, prune blocks and their copies, leaf references, leaf boxes
	Mesh dm;
	memset(&dm, 0, sizeof(dm));
	dm.uv = old.uv; dm.diffuse = old.diffuse; dm.normal = old.normal; dm.specular = old.specular;      // (uv and maps stay)
	dm.dW = old.dW; dm.dH = old.dH; dm.nW = old.nW; dm.nH = old.nH; dm.sW = old.sW; dm.sH = old.sH;
	rtx_scene::SrcMesh sm;
	rtx_scene::MeshLeaves leaves{ nullptr, 0 };
	float box[6];
	DevBag owned;      // (dropped with everything in it unless the edit goes through)
	if ((rc = deviceMeshGeometry(s, b, tri_pos_dev, nt, mesh, (uint32_t)s->srcLightPos.size(), owned, dm, sm, leaves, box))) return rc;
	HIPCHK(owned.copyFrom(tri_nrm_dev, (size_t)nt * 9, &dm.nrm));
	HIPCHK(owned.copyFrom(old.tb ? tri_tb_dev : nullptr, (size_t)nt * 6, &dm.tb));
	// the objects of this mesh with their derived fields; then everything is in place on the host and goes up in two copies
	std::vector<Object> objs = s->objectRecs;
	const std::vector<float> oldBounds(s->meshBounds.begin() + (size_t)mesh * 6, s->meshBounds.begin() + (size_t)mesh * 6 + 6);
	std::copy(box, box + 6, s->meshBounds.begin() + (size_t)mesh * 6);
	for (Object& d : objs)
		if (d.type == RTX_OBJ_MESH && d.mesh == (int32_t)mesh) meshObjectRecord(s, d, dm, sm);
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

// rtx_debug.h: host wall time of the stages of the last rtx_scene_update_mesh
int rtx_scene_edit_times(rtx_scene* s, float* ms4)
{
	if (!s || !ms4) return fail(RTX_ERR_ARG, "scene/ms4 is NULL");
	memcpy(ms4, s->editMs, sizeof(s->editMs));
	return RTX_OK;
}

} // extern "C"
