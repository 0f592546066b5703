/* Direct light and ambient occlusion at caller-supplied surface points: the two questions the renderer spends most of its
 * rays on -- how much light reaches this point, how open is it -- for a caller who has points and no rays: vertices or lightmap texels to
 * bake, irradiance probes, particles, a G-buffer kept from rtx_render_aov or rtx_surface_rays.  No ray is traced to find the point, and
 * its normal is not looked up: P and N are used as given.  The points of a mesh's lightmap texels are rtx_texel_points' (rtx_bake.h).
 * An extension of the C ABI in rtx.h. */
#ifndef RTX_POINTS_H
#define RTX_POINTS_H
#include "rtx_light.h"
#include "rtx_ao.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Both calls.  points_dev: n x 6 floats {P.xyz, N.xyz} in device memory -- the layout of a ray buffer, P where the origin is and N where
 * the direction is.  N is used as stored (not normalised; any length, zero included).  Everything is fp32 without contraction unless
 * stated otherwise; dot products are summed x, y, z.  O = P + N * view.bias, per component (castRay's shadow-ray origin, scene.cpp:787).
 * Every result is written at the point's own index, and nothing else in any buffer is touched.  A point's results depend on nothing but
 * that point: not on the other points of the batch, nor on their order.
 *
 * Asynchronous on `stream` and ordered against the view's preparation as rtx_light_rays is; nothing is queued on the NULL stream; nothing
 * is allocated and nothing waits for the device once the scene's ray scratch has grown to n.  Large batches are regrouped as
 * rtx_trace_rays' with {P, N} in the place of origin and direction (knobs trace_reorder, trace_key_origin_first).  n == 0 does nothing;
 * n > 0xffffffc0 is refused.  Row ownership is ignored; counters (rtx_counters_enable) are neither collected nor refused;
 * max_ray_depth, RTX_FLAG_SHOW_NORMALS and the skybox flag change nothing.  The scratch is the scene's, so calls on one scene must not
 * overlap on different streams. */

/* rtx_light_points: what castRay sums over the lights at a hit at P with the shading normal N, reached by a ray of direction V.
 * view_dev: n x 4 floats {V.xyz, ns} in device memory, or NULL -- V the direction of the ray that arrived at P (castRay's dir, used as
 * stored), ns the specular exponent (the hit object's n_specular).  out: rtx_light_rays' buffers, indexed by point (the per-light
 * buffers by point, then light); any may be NULL, at least one is not; out->hits_dev must be NULL (there is no hit to report).
 *
 * Steps 2 to 5 of rtx_light_rays' contract (rtx_light.h) hold word for word with P and N the point's, dir = V and ns = view[3]; every
 * point counts as a hit:
 *  - for lights i = 0 .. n_lights - 1 in scene order, (L, I, dist) = illuminate(P), the point light's and the area light's factor in
 *    double; every shadow ray is rtx_occluded_rays' question for {O, -L} with tmax = dist, under the view's culling flag;
 *    D_i and S_i as there, with the reference's powf;
 *  - diffuse = (((+0) + D_0) + D_1) + ..., specular likewise: the sums start at +0 and run in light order;
 *  - light_open is the true visibility of every (point, light) pair.  When light_open_dev is NULL, a pair whose D and S are +0 for either
 *    answer is not walked.
 * With view_dev == NULL the two specular pointers must be NULL, and nothing specular is computed.
 * With zero lights diffuse and specular are +0.
 * RTX_ERR_ARG, the buffers untouched: NULL scene, NULL out, the five output pointers all NULL, hits_dev set, a specular pointer without
 * view_dev, a per-light pointer with n_lights != the scene's current number of lights or on a scene without lights, NULL points_dev with
 * n > 0, n > 0xffffffc0. */
int rtx_light_points(rtx_scene* scene, uint32_t n, const float* points_dev, const float* view_dev, const rtx_light_buffers* out, void* stream);

/* rtx_ao_points: steps 2 and 3 of rtx_render_ao's contract (rtx_ao.h), per point.  ao_dev and counts_dev: n each, device memory; either
 * may be NULL (it is not written), not both.
 *  - For k = 0 .. n_dirs-1 with d = dirs[k]:  c = N.x*d.x + N.y*d.y + N.z*d.z.  Direction k is TRACED for the point iff c > 0 -- strict,
 *    so a zero or NaN direction or normal is never traced.  A traced direction is OPEN iff rtx_occluded_rays answers 0 for the ray {O, d}
 *    with tmax = radius.
 *  - counts = open | traced << 16;  ao = traced ? (float)open / (float)traced : 1.0f  (IEEE fp32 division).
 * RTX_ERR_ARG, the buffers untouched: NULL scene, NULL params, both outputs NULL, NULL dirs_dev, n_dirs outside 1 .. 256, radius NaN or
 * <= 0 (rtx_render_ao's checks), NULL points_dev with n > 0, n > 0xffffffc0. */
int rtx_ao_points(rtx_scene* scene, uint32_t n, const float* points_dev, const rtx_ao_params* params, float* ao_dev, uint32_t* counts_dev,
                  void* stream);

#ifdef __cplusplus
}
#endif
#endif
