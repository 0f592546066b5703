/* Radiance gathered over a set of directions at caller-supplied surface points: the third question a baker, an irradiance
 * probe or a final-gather pass asks at a point it already has -- after how much direct light arrives (rtx_light_points) and how open the
 * point is (rtx_ao_points): what does the scene look like from here, summed over these directions?  Sky light tinted by the skybox,
 * colour bleeding from a lit wall, a mirror's contribution.  No ray buffer of n x n_dirs rays exists anywhere: a wave casts 64 rays that
 * share a direction and leave neighbouring points.  An extension of the C ABI in rtx.h.  (Not "gather": rtx_gather is the multi-GPU image
 * gather.) */
#ifndef RTX_RADIANCE_H
#define RTX_RADIANCE_H
#include "rtx_points.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct rtx_radiance_params {
    uint32_t     n_dirs;       /* 1 .. 256 */
    const float* dirs_dev;     /* DEVICE memory, n_dirs x 3, world space, used as stored (not normalised) */
    const float* weights_dev;  /* DEVICE memory, n_dirs floats, or NULL = 1.0f for every direction */
    int32_t      cosine;       /* 0 or 1: multiply direction k's weight by c = N . d_k */
} rtx_radiance_params;

/* points_dev: rtx_points.h's n x 6 floats {P.xyz, N.xyz} in device memory.  N is used as stored (not normalised; any length, zero
 * included); O = P + N * view.bias, per component (castRay's shadow-ray origin, scene.cpp:787).  sum_dev: n x 3 floats, counts_dev: n,
 * device memory owned by the caller; either may be NULL (it is not written), not both.
 *
 * The contract, per point, in fp32 without contraction, dot products summed x, y, z:
 *  1. For k = 0 .. n_dirs-1 with d = dirs[k]:  c = N.x*d.x + N.y*d.y + N.z*d.z.  Direction k is TRACED for the point iff c > 0 -- strict,
 *     so a zero or NaN normal or direction is never traced.
 *  2. For a traced direction, L = Render::castRay({O, d}, scene, 0): bit for bit the colour rtx_trace_rays writes for the ray {O, d}
 *     under the current view (culling flag, skybox flag, max_ray_depth, background).
 *  3. w = weights ? weights[k] : 1.0f, then w = w * c if cosine.  Per component acc = acc + L * w -- the product is rounded, then the
 *     sum; acc starts at +0 and runs over the traced directions in ascending k.
 *  4. sum = acc; counts = the number of traced directions.  A point with no traced direction gets sum = +0 and counts = 0.
 *  5. A point's results depend on nothing but that point: not on the other points of the batch, nor on their order.  They are written
 *     at the point's own index, and nothing else in either buffer is touched.
 *
 * Asynchronous on `stream` and ordered against the view's preparation as rtx_light_rays is; nothing is queued on the NULL stream; nothing
 * is allocated and nothing waits for the device once the scene's ray scratch has grown to n.  Large batches are regrouped as
 * rtx_trace_rays' with {P, N} in the place of origin and direction (knobs trace_reorder, trace_key_origin_first).  n == 0 does nothing.
 * Row ownership is ignored; counters (rtx_counters_enable) are neither collected nor refused.  The scratch is the scene's, so calls on
 * one scene must not overlap on different streams.
 * RTX_ERR_ARG, the buffers untouched: NULL scene, NULL params, both outputs NULL, NULL dirs_dev, n_dirs outside 1 .. 256, cosine not 0
 * or 1, NULL points_dev with n > 0, n > 0xffffffc0.  RTX_ERR_UNSUPPORTED while RTX_FLAG_SHOW_NORMALS is set: a debug view has no
 * radiance. */
int rtx_radiance_points(rtx_scene* scene, uint32_t n, const float* points_dev, const rtx_radiance_params* params,
                        float* sum_dev, uint32_t* counts_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif
