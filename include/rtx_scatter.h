/* Reflection and refraction rays at the hits of caller-supplied rays: what castRay does at the first hit of every ray of a
 * batch besides recursing -- the part of the hit's colour that needs no further ray, the secondary rays the recursion itself would cast and
 * the factors their colours enter with -- in one launch and one walk.  With rtx_sky_rays, what castRay returns for a ray beyond
 * max_ray_depth, it closes the loop trace -> surface -> new rays built on the caller's side at mirrors and glass: a caller rebuilds castRay
 * level by level from public calls, with a depth rule, a weight cut-off or per-bounce buffers of their own, and restates neither reflect,
 * refract and fresnel, nor Vec3::normalize's double-precision factor, nor the bias rule inside the medium, nor the kr < 1 rule.
 * An extension of the C ABI in rtx.h. */
#ifndef RTX_SCATTER_H
#define RTX_SCATTER_H
#include "rtx.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Device pointers owned by the caller, each indexed by the ray's own index; any may be NULL (that buffer is not written), at least one
 * is not. */
typedef struct rtx_scatter_buffers {
    float*   hits_dev;     /* n x 8: rtx_trace_rays' record                                                   */
    float*   local_dev;    /* n x 3: the part of castRay's colour at this hit that needs no further ray       */
    float*   reflect_dev;  /* n x 6: {orig, dir} of the reflection ray                                        */
    float*   refract_dev;  /* n x 6: {orig, dir} of the refraction ray                                        */
    float*   weight_dev;   /* n x 2: {the reflection ray's factor, the refraction ray's factor}               */
    uint8_t* kinds_dev;    /* n: bit 0 a reflection ray exists, bit 1 a refraction ray exists                 */
} rtx_scatter_buffers;

/* For each of the n rays {o.xyz, d.xyz} at rays_dev (the layout of rtx_trace_rays).  Everything is fp32 without contraction; dot products
 * are summed x, y, z.  Nothing else in any buffer is touched.
 *
 * 1. hits, P = o + d * tNear, N = hitNormal, albedo, ks and the hit object are rtx_surface_rays' values for the same ray, under the view's
 *    culling flag.  bias = view.bias, B = N * bias.  max_ray_depth, RTX_FLAG_SHOW_NORMALS and the skybox flag change nothing, except that
 *    the sky colour follows the skybox flag as rtx_surface_rays' albedo at a miss does.
 * 2. D and S are rtx_light_rays' diffuse and specular for the same ray (for Reflective and Transparent hits only S is needed); rule 4 of
 *    rtx_light.h about the pairs that are not walked applies.
 * 3. The channels by case; "nothing" means every word is +0:
 *      miss          kinds 0   local = getSkybox(d)                                children and weight: nothing
 *      Diffuse       kinds 0   local = albedo * D                                  nothing                              (scene.cpp:808)
 *      Phong         kinds 0   local = (albedo * ambient + D * kd) + S * ks        nothing                              (scene.cpp:852)
 *      Reflective    kinds 1   local = S       reflect = {P + B, d - N * (2 * (d . N))}, not normalised; weight = {0.8f, 0}; refract:
 *                                              nothing                                                                  (scene.cpp:856)
 *      Transparent   (scene.cpp:893-907, 940)  kr = fresnel(d, N, ior), outside = (d . N) < 0;  local = S * kr;
 *                    reflect = {outside ? P + B : P - B, normalize(reflect(d, N))}, bit 0 of kinds is set, weight[0] = kr;
 *                    if kr < 1: refract = {outside ? P - B : P + B, normalize(refract(d, N, ior))}, bit 1 is set, weight[1] = 1 - kr;
 *                    otherwise (total internal reflection) there is no refraction ray: refract and weight[1] are +0.
 *    reflect, refract, fresnel and normalize are the frame kernels' device functions with their operand order: the children are the rays
 *    the recursion itself builds.
 * 4. The identities, with C(r) = castRay(r, depth + 1):
 *      Reflective:    castRay = C(reflect) * 0.8f + local
 *      Transparent:   castRay = (((+0) + C(refract) * weight[1]) + C(reflect) * weight[0]) + local, the refraction term only where bit 1 is set
 *      kinds == 0:    castRay = local  (not 0 + local: a negative background colour keeps its sign of zero)
 *    So for a Diffuse or Phong hit, or a miss, local is the bits of rtx_trace_rays' colour.
 * 5. Every ray's results are independent of the other rays of the batch and of their order.
 *
 * What was not asked for is not computed: no light is looked at when local_dev is NULL, and with it only for the hits whose material needs
 * D or S.
 *
 * Everything else follows rtx_light_rays: asynchronous on `stream` and ordered against the view's preparation; nothing is queued on the
 * NULL stream; nothing is allocated and nothing waits for the device once the scene's ray scratch has grown to n; large batches are
 * regrouped as rtx_trace_rays' (knobs trace_reorder, trace_key_origin_first); n == 0 does nothing; n > 0xffffffc0 is refused; row
 * ownership is ignored; counters (rtx_counters_enable) are neither collected nor refused.  The scratch is the scene's, so calls on one
 * scene must not overlap on different streams.  A request for hits alone is rtx_trace_rays' for hits alone: the same launch.
 * RTX_ERR_ARG, the buffers untouched: NULL scene, NULL out, all six pointers NULL, NULL rays_dev with n > 0. */
int rtx_scatter_rays(rtx_scene* scene, uint32_t n, const float* rays_dev, const rtx_scatter_buffers* out, void* stream);

/* colours_dev[i] = Scene::getSkybox(dir of ray i), n x 3: the sky texel of the direction under RTX_FLAG_SKYBOX, the background colour
 * otherwise -- whatever the ray would hit.  It is what castRay returns for a ray beyond max_ray_depth, which no other entry point gives for
 * a ray that hits something.  A plain grid launch on `stream`, ordered against the view's preparation; no walk, no scratch, no
 * regrouping.  n == 0 does nothing; RTX_ERR_ARG: NULL scene, NULL colours_dev, NULL rays_dev with n > 0, n > 0xffffffc0. */
int rtx_sky_rays(rtx_scene* scene, uint32_t n, const float* rays_dev, float* colours_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif
