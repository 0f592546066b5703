/* Surface data at the hits of caller-supplied rays: what rtx_trace_rays' hit record stops short of -- the hit point,
 * the shading normal, the albedo and the specular coefficient of every ray of a batch -- in one launch.  With it a caller closes the loop
 * trace -> surface -> new rays built on the caller's side -> rtx_trace_rays / rtx_occluded_rays / rtx_surface_rays again (custom cameras,
 * secondary rays, light probes).  An extension of the C ABI in rtx.h. */
#ifndef RTX_SURFACE_H
#define RTX_SURFACE_H
#include "rtx.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Device pointers owned by the caller, each indexed by the ray's own index; any may be NULL (that channel is not written), at least one
 * is not. */
typedef struct rtx_surface_buffers {
    float* hits_dev;      /* n x 8: rtx_trace_rays' record */
    float* position_dev;  /* n x 3 */
    float* normal_dev;    /* n x 3 */
    float* albedo_dev;    /* n x 3 */
    float* specular_dev;  /* n     */
} rtx_surface_buffers;

/* For each of the n rays {orig.xyz, dir.xyz} at rays_dev (the layout of rtx_trace_rays), the channels of
 *
 *     Render::trace(ray, scene.objects, info)      (scene.cpp:724-756)
 *
 * of the ray as stored, under the view's culling flag, and of getSurfaceData at its hit (scene.cpp:763-770).  Everything is fp32 without
 * contraction.  Nothing else in any buffer is touched.
 *   hits: the bits rtx_trace_rays writes for the same ray.
 *   position: hitPoint = orig + dir * tNear, a product then a sum per component (scene.cpp:768).  A miss: (0, 0, 0).
 *   normal: hitNormal (scene.cpp:769) -- a sphere's objects.cpp:788-796, a plane's stored normal, a mesh's objects.cpp:121-151 with its
 *       normal map.  normal / 2 + 0.5 in fp32 is bit for bit the colour rtx_trace_rays returns for the ray under RTX_FLAG_SHOW_NORMALS.
 *       A miss: (0, 0, 0).
 *   albedo: the object's colour, or getDiffuseColor (objects.cpp:153-163) for a mesh with a diffuse map.  A miss: getSkybox(dir), the
 *       sky texel under RTX_FLAG_SKYBOX and the background colour otherwise.
 *   specular: the coefficient castRay multiplies the specular sum by (scene.cpp:849-851) -- getSpecularValue for a mesh with a specular
 *       map, otherwise the object's `specular` field; written for every material, not only Phong.  A miss: 0.
 * For a camera ray of the current view, hits (its ids as integers), normal and albedo equal the channels rtx_render_aov writes for that
 * pixel.  max_ray_depth and RTX_FLAG_SHOW_NORMALS change nothing (in particular a negative max_ray_depth does not turn hits into
 * misses, as it does for the RTX_FLAG_SHOW_NORMALS colours).  Every ray's results are independent of the other rays of the batch and
 * of their order.
 *
 * The other per-object constants a caller shades with -- material, ior, ambient, diffuse, n_specular -- are constants of the object,
 * not of the ray: they are in the object table (rtx_scene_objects_read), which the object id of `hits` (field 1) indexes, and are not
 * repeated per ray.
 *
 * Everything else follows rtx_trace_rays: asynchronous on `stream` and ordered against the view's preparation; nothing is queued on
 * the NULL stream; nothing waits for the device once the scene's ray scratch has grown to n; n == 0 does nothing; n > 0xffffffc0 is
 * refused; row ownership is ignored; counters (rtx_counters_enable) are neither collected nor refused.  The scratch is the scene's, so
 * calls on one scene must not overlap on different streams.  A request for hits alone is rtx_trace_rays' for hits alone: the same launch.
 * RTX_ERR_ARG, the buffers untouched: NULL scene, NULL out, all five pointers NULL, NULL rays_dev with n > 0. */
int rtx_surface_rays(rtx_scene* scene, uint32_t n, const float* rays_dev, const rtx_surface_buffers* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
