/* Queries on a loaded scene that render nothing.  An extension of the C ABI in rtx.h, next to rtx_trace_rays' "what
 * does this ray hit first": "is anything between here and there", answered with the reference's own shadow-ray rule. */
#ifndef RTX_QUERY_H
#define RTX_QUERY_H
#include "rtx.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Occlusion (any-hit) for a batch of caller-supplied rays in device memory:
 *
 *     occluded_dev[i] = Render::trace(Ray{orig_i, dir_i, RayType::ShadowRay}, scene.objects, info)   with info.tNear preset to tmax_i
 *
 * what Render::castRay evaluates for `vis` (scene.cpp:787, the light's distance being the range).  1 iff some object whose material is
 * not Transparent reports an intersection with tNear < tmax_i, every object's tNear being the one Render::trace computes (a mesh's the
 * result of its whole walk under the view's back-face-culling flag, a sphere's and a plane's as intersectObject gives them); 0
 * otherwise.  The comparison is the reference's strict fp32 `<`: tNear == tmax_i is not occluded, a NaN range occludes nothing, +inf
 * means the whole ray.  The answer is "the minimum of tNear over the opaque objects is below tmax_i", so it depends neither on the order
 * of the objects, nor on which of several blockers is found first, nor on the other rays of the batch: the device stops at a ray's
 * first blocker, looks at spheres and planes before it walks a mesh, and groups large batches into coherent bundles first as
 * rtx_trace_rays does (knobs trace_reorder and trace_key_origin_first act on this call too; knob occluded_scene_order = 1 keeps the
 * objects in scene order, for A/B runs: 0, analytic objects first, is the default).
 *
 * rays_dev n x 6 floats {orig xyz, dir xyz}; tmax_dev n floats, or NULL for +inf for every ray; occluded_dev n bytes, each 0 or 1,
 * written at the ray's own index (nothing outside [0, n) is written).  RTX_FLAG_SHOW_NORMALS and the skybox flag do not change an
 * answer; the view's culling flag does.
 * Asynchronous on `stream`: nothing is queued on the NULL stream and, once the scene's scratch has grown to n rays, nothing waits for
 * the device.  n == 0 does nothing; row ownership is ignored; counters are neither collected nor refused.  The scratch is the one
 * rtx_trace_rays uses: calls on one scene are not to overlap on different streams (as the render calls).  NULL rays_dev or
 * occluded_dev with n > 0: RTX_ERR_ARG, and the scene is untouched. */
int rtx_occluded_rays(rtx_scene* scene, uint32_t n, const float* rays_dev, const float* tmax_dev, uint8_t* occluded_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif
