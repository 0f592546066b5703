/* Editing a live scene: objects of a scene created by rtx_scene_create move between frames and its lights change
 * (DESIGN.md 3.9).  An extension of the C ABI
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

#ifdef __cplusplus
}
#endif
#endif
