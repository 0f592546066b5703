/* Editing a live scene: objects of a scene created by rtx_scene_create move between frames, its lights change
 *  and its objects appear and disappear.  An extension of the C ABI
 * in rtx.h -- the reference has no edit API; moving an object there means editing its [object] block and loading the file again, and a
 * scene edited here renders, bit for bit, what a scene created from the edited description renders.
 *
 * Ordering: every call here may synchronise with the device.  They wait for everything queued on the scene (every stream a render call was
 * made on, and `stream`, where the caller produced the triangles); renders queued before an edit see the old scene, renders queued
 * after it the new one, and the caller's buffers may be reused once the call returns.  Row ownership, counters and the frame mode stay
 * as they are.  A refused argument (RTX_ERR_ARG) leaves the scene as it was; after RTX_ERR_DEVICE an edit may be partly applied, and the
 * scene is only fit for rtx_scene_destroy. */
#ifndef RTX_SCENE_EDIT_H
#define RTX_SCENE_EDIT_H
#include "rtx.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Replace object `index`'s record. type, material and mesh must be the ones it was created with (RTX_ERR_ARG otherwise);
 * every other field may change (sphere pos / radius2, plane pos / normal, colour, ior, Phong terms). For a mesh object,
 * the fields derived from its mesh stay as created or as the last rtx_scene_update_mesh left them. */
int rtx_scene_set_object(rtx_scene* scene, uint32_t index, const rtx_object* object);

/* Give mesh `mesh` new world-space triangles: n_tris of the mesh as created (topology, uv and maps unchanged).
 * Inputs in device memory: tri_pos_dev n_tris x 9, tri_nrm_dev n_tris x 9, tri_tb_dev n_tris x 6 (required iff the mesh
 * was created with tangents, else NULL). root_lo / root_hi: the root box Mesh::loadModel sets. ac_penalty: options::acPenalty.
 * The acceleration structure is rebuilt on the device with the reference's builder. The result must be bit-identical to
 * what rtx_scene_create would have uploaded for a description holding these triangles and the tree built from them. */
int rtx_scene_update_mesh(rtx_scene* scene, uint32_t mesh, const float* tri_pos_dev, const float* tri_nrm_dev,
                          const float* tri_tb_dev, const float root_lo[3], const float root_hi[3], int32_t ac_penalty,
                          void* stream);

/* Replace the scene's lights by the n_lights records of `lights` (host memory, copied during the call, like the lights of
 * rtx_scene_create's description; n_lights == 0 is legal).  One call covers a light moved, recoloured, dimmed, of another type or
 * another number of sample points at its index, added or removed.  Refused (RTX_ERR_ARG): NULL lights with n_lights > 0, a type that
 * is no RTX_LIGHT_*, an area light with points == NULL or n_points == 0.  Afterwards the device holds what rtx_scene_create would
 * have uploaded and prepared for the same description with these lights: the records and sample points (the old ones are freed;
 * rtx_scene_bytes reports a fresh scene's number), the source copies of every mesh's prune records -- laid out again when
 * min(n_lights, 6) changes --, the kernel family (RTX_VARIANT_PLAIN holds while no light is an area light), the cost estimate. */
int rtx_scene_set_lights(rtx_scene* scene, uint32_t n_lights, const rtx_light* lights);

/* The object list and the mesh list replaced as a whole: one call covers an object appended or inserted at any index, removed, reordered,
 * of another type or material at its index, and n_objects == 0.  meshes[i] says where mesh i of the new list comes from; the `mesh` field
 * of the objects indexes the new list.  Refused (RTX_ERR_ARG, the scene untouched): NULL arrays with a count, a bad type, material or
 * mesh index (the checks of the load), keep out of range, one old mesh kept twice, a new mesh with missing arrays, a normal map without
 * tangents.  It waits for the device and for `stream` first.  Afterwards the device holds what the load would have uploaded and prepared
 * for the current view, lights and sky with these objects and meshes: a kept mesh is neither uploaded nor built again, a mesh that is
 * not kept is freed with everything of its own (rtx_scene_bytes reports a fresh scene's number), the kernel variant is chosen again, and
 * every source copy of every mesh's prune records is built again. */
typedef struct rtx_mesh_build {   /* triangles in device memory; the tree is built on the device as by rtx_scene_update_mesh */
	const float* tri_pos_dev;     /* n_tris x 9 */
	const float* tri_nrm_dev;     /* n_tris x 9 */
	const float* tri_tb_dev;      /* n_tris x 6, or NULL (required iff mesh->normal_map) */
	float root_lo[3], root_hi[3]; /* the root box Mesh::loadModel sets */
	int32_t ac_penalty;
} rtx_mesh_build;

typedef struct rtx_mesh_source {
	int32_t keep;                 /* >= 0: mesh `keep` of the scene as it is now takes this index, untouched; -1: a new mesh */
	const rtx_mesh* mesh;         /* new mesh: host memory, as in rtx_scene_desc */
	const rtx_mesh_build* build;  /* NULL: `mesh` carries tree and triangles (the load path);
	                                 else n_tris (> 0), tri_uv and the maps come from `mesh`, its tree and tri_pos/nrm/tb are ignored */
} rtx_mesh_source;

int rtx_scene_set_objects(rtx_scene* scene, uint32_t n_objects, const rtx_object* objects, uint32_t n_meshes,
                          const rtx_mesh_source* meshes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
