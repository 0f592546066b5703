/* Surface points projected into cameras, with visibility: the way back from the scene into a camera -- which pixel of this
 * camera does the surface point P fall into, and can that camera see it?  For a caller who projects a rendered or photographed view onto a
 * mesh's texture (rtx_texel_points -> rtx_project_points -> gather -> rtx_scene_set_map), reprojects a kept G-buffer into the next camera,
 * chooses which of many cameras sees a vertex or a probe, or splats particles into a frame.  The camera is the renderer's own, field by
 * field, not a restatement of it, and no ray or range buffer is built for the visibility.
 * An extension of the C ABI in rtx.h. */
#ifndef RTX_PROJECT_H
#define RTX_PROJECT_H
#include "rtx_points.h"
#ifdef __cplusplus
extern "C" {
#endif

#define RTX_PROJECT_CAMERA_FLOATS 24   /* one record of cameras_dev */
/* record: [0..2] cam_pos, [3] scale, [4] aspect, [5] width, [6] height (as floats), [7] 0 (reserved),
           [8..23] cam_matrix -- the fields of rtx_view / rtx_view_target, meaning the same */
#define RTX_PROJ_FRONT  1u
#define RTX_PROJ_INSIDE 2u
#define RTX_PROJ_FACING 4u
#define RTX_PROJ_OPEN   8u

/* Three device pointers, any of them NULL (it is not written), not all:
 * pixel_dev n_cams x n x 2 floats, depth_dev n_cams x n floats, flags_dev n_cams x n bytes -- camera-major, so that each camera's results
 * form one contiguous block: element (c, i) is at c * n + i, indexed in size_t. */
typedef struct rtx_project_buffers { float* pixel_dev; float* depth_dev; uint8_t* flags_dev; } rtx_project_buffers;

/* points_dev: rtx_points.h's n x 6 floats {P.xyz, N.xyz} in device memory, with its rules: N is used as stored (not normalised; any length,
 * zero included), O = P + N * view.bias per component.  cameras_dev: n_cams x 24 floats in DEVICE memory (4-byte aligned), n_cams in
 * 1 .. 256; the table is used as stored and is not validated, like rtx_ao_params.dirs_dev.  Every result is written at the point's own
 * index of its camera's block; nothing outside [0, n_cams * n) of a given buffer is touched, and nothing of a buffer that is not given.
 *
 * For camera record R and point i, in fp32 without contraction, dot products summed x, y, z; C = R.cam_pos, M = R.cam_matrix:
 *  1. c = P - C per component; dist = length(c) and L = normalized(c), exactly as rtx_light_points computes them for a point light at C
 *     (PointLight::illuminate without the intensity).
 *  2. Camera space, the transpose of the product in the renderer's primary ray:
 *       sx = (c.x*M[0] + c.y*M[1]) + c.z*M[2],  sy = (c.x*M[4] + c.y*M[5]) + c.z*M[6],  sz = (c.x*M[8] + c.y*M[9]) + c.z*M[10].
 *  3. Pixel coordinates, with IEEE fp32 divisions:  inz = -sz, xp = sx / inz, yp = sy / inz, ax = R.scale * R.aspect,
 *       px = (xp / ax + 1) * (R.width * 0.5f) - 1,   py = (1 - yp / R.scale) * (R.height * 0.5f) - 1.
 *     pixel = {px, py} is written as computed, inf and NaN (sz == 0) included.  An integer (x, y) means the pixel whose primary ray the
 *     renderer aims at (x + 0.5, y + 0.5) -- that ray evaluates 2 * (x + 1) / w - 1, hence the "- 1".  The nearest pixel is
 *     floor(px + 0.5), floor(py + 0.5).
 *  4. depth = dist.
 *  5. flags:  FRONT iff sz < 0.
 *     INSIDE iff FRONT and px >= -0.5f && px < width - 1.5f && py >= -0.5f && py < height - 1.5f: the nearest pixel is then one that pass 1
 *     renders (x < width - 1, y < height - 1).  NaN compares false.
 *     FACING iff N . (-L) > 0, strict.
 *     OPEN iff with_visibility != 0, FRONT and INSIDE, dist is not NaN, and rtx_occluded_rays answers 0 for {O, -L} with tmax = dist under
 *     the view's culling flag: the shadow ray castRay would cast at P towards a point light at the camera.  Pairs that are not
 *     FRONT && INSIDE are never walked; nothing is walked at all when with_visibility == 0 or flags_dev == NULL.
 *  6. A pair's results depend on that point and that camera only: not on the other points or cameras, nor on their order.
 *
 * This arithmetic is the inverse of the renderer's primary ray (up to rounding) only for a rotation cam_matrix -- what rtx_scene_set_view
 * and the host's view targets (rah_view_target) make: there the transpose of the upper 3 x 3 is its inverse, the translation row is zero
 * and the projective column is (0, 0, 0, 1).  For any other matrix the arithmetic above is still what is computed.
 *
 * Asynchronous on `stream` and ordered against the view's preparation as rtx_light_rays is; nothing is queued on the NULL stream; nothing
 * is allocated and nothing waits for the device once the scene's ray scratch has grown to n.  Large batches are regrouped as
 * rtx_trace_rays' with {P, N} in the place of origin and direction (knobs trace_reorder, trace_key_origin_first).  n == 0 does nothing;
 * n > 0xffffffc0 is refused.  Row ownership is ignored; counters (rtx_counters_enable) are neither collected nor refused;
 * max_ray_depth, RTX_FLAG_SHOW_NORMALS and the skybox flag change nothing.  The scratch is the scene's, so calls on one scene must not
 * overlap on different streams.
 *
 * RTX_ERR_ARG, the buffers untouched: NULL scene, NULL out, the three output pointers all NULL, NULL points_dev with n > 0, NULL
 * cameras_dev, n_cams outside 1 .. 256, n > 0xffffffc0. */
int rtx_project_points(rtx_scene* scene, uint32_t n, const float* points_dev, uint32_t n_cams, const float* cameras_dev,
                       int with_visibility, const rtx_project_buffers* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
