/* Deforming a mesh of a live scene from vertices in device memory.  An extension of the C ABI in rtx.h, beside the edits of
 * rtx_scene_edit.h, whose ordering and error rules hold here: a call waits for everything queued on the scene and for `stream`; a refused
 * argument (RTX_ERR_ARG) leaves the scene as it was.
 *
 * The device runs the loader's placement and triangle assembly (Mesh::place: the fit of `size` to the vertices' box, rotation, translation,
 * pinned flat axes, face normals, tangent frames) on the new vertices and hands the triangles to the rebuild of the mesh-update call of
 * rtx_scene_edit.h: afterwards the scene holds, bit for bit, what a fresh load of an OBJ file with these `v` (and `vn`) lines would have
 * uploaded.  No triangle crosses the bus. */
#ifndef RTX_DEFORM_H
#define RTX_DEFORM_H
#include "rtx.h"
#ifdef __cplusplus
extern "C" {
#endif

/* What the loader kept of a mesh's OBJ file beside its vertices: host memory, copied to the device by the call and kept there until the mesh
 * is freed (it follows a mesh that the object-list edit keeps).  Not counted in the scene's bytes; visible in the live device memory. */
typedef struct rtx_mesh_topology {
	uint32_t n_tris, n_pos, n_nrm, n_uv;
	uint32_t placed_pos, placed_nrm;    /* the vertices / normals read before the first face: only those are placed / rotated */
	const uint32_t* corner_pos;         /* n_tris x 3, each < n_pos */
	const int32_t* corner_nrm;          /* n_tris x 3; [0] < 0: the face gave no normals (face normal) */
	const int32_t* corner_uv;           /* n_tris x 3; [0] < 0: the face gave no uv (no tangent frame) */
	const float* uv;                    /* n_uv x 2, finite */
	const float* nrm;                   /* n_nrm x 3 as stored (normalised by the loader): what nrm_dev == NULL keeps */
} rtx_mesh_topology;

/* Refused (RTX_ERR_ARG): n_tris other than the mesh's own count, a missing array, a corner index out of range, placed_* above n_*, a uv
 * that is not finite. */
int rtx_scene_set_mesh_topology(rtx_scene* scene, uint32_t mesh, const rtx_mesh_topology* topology);

typedef struct rtx_mesh_pose {
	float pos[3];
	float rot_matrix[16];               /* Matrix44f::fromEulerDegrees(rot), row-major, computed on the host (the device calls no sin or cos) */
	float size[3];
	float bias;                         /* options.bias: an axis whose range is below it is flat */
	int32_t ac_penalty;
} rtx_mesh_pose;

/* pos_dev: n_pos x 3 model-space vertices; nrm_dev: n_nrm x 3 raw normals (normalised here as the loader normalises them) or NULL (the
 * topology's stored normals are used: a caller that gave normals once and wants them kept sets the topology again with them stored);
 * both in device memory, n_pos / n_nrm the topology's counts.  obj_lo / obj_hi (either may be NULL): the box of
 * the first placed_pos vertices as the loader keeps it (lo from FLT_MAX, hi from FLT_MIN; the sign of a zero minimum is unspecified).
 * Refused (RTX_ERR_ARG, the scene untouched): a mesh without topology, wrong counts, a vertex or normal that is not finite, a placed
 * position that is not finite (a flat axis away from zero: the loader's own 0 / 0). */
int rtx_scene_deform_mesh(rtx_scene* scene, uint32_t mesh, const float* pos_dev, uint32_t n_pos, const float* nrm_dev, uint32_t n_nrm,
                          const rtx_mesh_pose* pose, float obj_lo[3], float obj_hi[3], void* stream);

#ifdef __cplusplus
}
#endif
#endif
