/* Ambient occlusion of a frame: for every pixel, how many of the caller's directions leave its first hit on the side of
 * the normal and how many of those are unoccluded within a radius -- in one launch over the view, without a ray buffer.  An extension of
 * the C ABI in rtx.h. */
#ifndef RTX_AO_H
#define RTX_AO_H
#include "rtx.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct rtx_ao_params {
    uint32_t     n_dirs;    /* 1 .. 256 */
    const float* dirs_dev;  /* DEVICE memory, n_dirs x 3, world space, used as stored (not normalised) */
    float        radius;    /* the range of every AO ray: > 0, +inf = the whole ray */
} rtx_ao_params;

/* ao_dev and counts_dev: device memory owned by the caller, H*W each, indexed x + y * W like the framebuffer; either may be NULL (it is
 * not written), not both.
 *
 * Pixels written: those rtx_render_aov writes -- x < W-1, y < H-1, y in [row_begin, min(row_end, H)), under rtx_set_row_ownership the
 * rows this part OWNS (no halo rows).  Nothing else in either buffer is touched.
 *
 * The contract, per pixel, in fp32 without contraction:
 *  1. The ray and its first hit are rtx_render_aov's: primaryRay(x + 0.5f, y + 0.5f) and Render::trace under the view's culling flag.
 *     P = orig + dir * tNear per component (castRay's hit point, scene.cpp:763), N = hitNormal (the `normal` channel of
 *     rtx_render_aov), O = P + N * view.bias (castRay's shadow-ray origin, scene.cpp:787).
 *  2. For k = 0 .. n_dirs-1 with d = dirs[k]:  c = N.x*d.x + N.y*d.y + N.z*d.z  (summed in that order).  Direction k is TRACED for the
 *     pixel iff c > 0 -- strict, so a zero or NaN direction is never traced.  A traced direction is OPEN iff rtx_occluded_rays answers 0
 *     for the ray {O, d} with tmax = radius (include/rtx_query.h: transparent objects do not block, strict tNear < radius, a mesh
 *     answers under the culling flag).
 *  3. counts = open | traced << 16;  ao = traced ? (float)open / (float)traced : 1.0f  (IEEE fp32 division).  A pixel whose ray hits
 *     nothing: ao = 1.0f, counts = 0.
 *  4. max_ray_depth, RTX_FLAG_SHOW_NORMALS and the skybox flag change nothing.
 *
 * Asynchronous on `stream` and ordered against the view's preparation as rtx_render_aov is; nothing is queued on the NULL stream, the
 * host does not wait and nothing is allocated.  The tile lists, the tile costs and the frame-mode measurements of the ordinary frames
 * are neither used nor changed.  row_begin >= row_end does nothing.
 * RTX_ERR_ARG, the buffers untouched: NULL scene, NULL params, both outputs NULL, NULL dirs_dev, n_dirs outside 1 .. 256, radius NaN or
 * <= 0.  RTX_ERR_UNSUPPORTED with counters enabled (rtx_counters_enable).
 *
 * Several GPUs: each output is a plain image of H rows of W * 4 bytes, so rtx_gather with that row_bytes assembles a frame whose parts
 * were rendered under rtx_set_row_ownership; there is no communication code of its own. */
int rtx_render_ao(rtx_scene* scene, uint32_t row_begin, uint32_t row_end, const rtx_ao_params* params,
                  float* ao_dev, uint32_t* counts_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif
