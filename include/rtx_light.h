/* Direct light at the hits of caller-supplied rays: what castRay sums over the lights at the first hit of every ray of a
 * batch -- diffuseComponent and specularComponent, each light's own term of both, and the number of each light's shadow rays that arrive --
 * in one launch.  It closes the loop trace -> surface -> new rays built on the caller's side where the renderer spends most of its rays:
 * the caller restates neither illuminate nor the reference's powf, builds no shadow rays, and the shadow walks use the point lights' source
 * copies of the prune records as the frame kernels' do.  An extension of the C ABI in rtx.h. */
#ifndef RTX_LIGHT_H
#define RTX_LIGHT_H
#include "rtx.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Device pointers owned by the caller, each indexed by the ray's own index (the per-light buffers by ray, then light); any may be NULL
 * (that buffer is not written), at least one is not. */
typedef struct rtx_light_buffers {
    uint32_t  n_lights;           /* the scene's current number of lights = 2nd dimension of the per-light buffers */
    float*    hits_dev;           /* n x 8: rtx_trace_rays' record                 */
    float*    diffuse_dev;        /* n x 3: castRay's diffuseComponent             */
    float*    specular_dev;       /* n x 3: castRay's specularComponent            */
    float*    light_diffuse_dev;  /* n x n_lights x 3: what light i adds to it     */
    float*    light_specular_dev; /* n x n_lights x 3                              */
    uint32_t* light_open_dev;     /* n x n_lights: visible shadow rays of light i  */
} rtx_light_buffers;

/* For each of the n rays {orig.xyz, dir.xyz} at rays_dev (the layout of rtx_trace_rays).  Everything is fp32 without contraction unless
 * stated otherwise; max0(x) = std::max(0.f, x), so NaN gives 0; dot products are summed x, y, z.  Nothing else in any buffer is touched.
 *
 * 1. hits, P = orig + dir * tNear, N = hitNormal and the hit object are rtx_surface_rays' values for the same ray, under the view's
 *    culling flag (Render::trace, scene.cpp:724-756; getSurfaceData, scene.cpp:763-770).  A miss writes zeros everywhere, and
 *    light_open = 0.  max_ray_depth, RTX_FLAG_SHOW_NORMALS and the skybox flag change nothing.
 *    O = P + N * view.bias (scene.cpp:787); ns = the hit object's n_specular, for any material.
 * 2. For lights i = 0 .. n_lights - 1 in scene order:
 *    Distant / point: (L, I, dist) = illuminate(P) (lights.cpp:18-38; the point light's factor intensity / (4 pi |P - pos|^2 / 1000) is
 *      computed in double, cast to float and capped at 1; dist = FLT_MAX for a distant light).
 *      open_i = 1 - the answer of rtx_occluded_rays for the ray {O, -L} with tmax = dist.
 *      m = max0(N . -L), R = reflect(L, N) = L - N * (2 * (L . N)) (scene.cpp:674).
 *      D_i = open_i ? I * m : +0;  S_i = open_i ? I * powf(max0(R . -dir), ns) : +0, with the reference's powf (glibc's).
 *    Area (scene.cpp:792-805, 828-846): I = color * attenuation(intensity, |P - pos|^2), the same double factor.  For each sample point p
 *      in stored order: Ld = P - p, dist = length(Ld), Ln = normalized(Ld); open_k as above for {O, -Ln} with tmax = dist;
 *      dsum += open_k * max0(N . -Ln);  ssum += open_k * max0(reflect(Ln, N) . -dir).
 *      D_i = (dsum / (float)n_points) * I;  S_i = powf(ssum / (float)n_points, ns) * I;  open_i = the sum of open_k.
 * 3. diffuse = (((+0) + D_0) + D_1) + ..., specular likewise: castRay's sums (scene.cpp:788, 820, 824).  Its Diffuse branch associates
 *    I * (vis * m) and its Phong branch (vis * I) * m; both give the bits above up to the sign of a zero term, which cannot change a sum
 *    that starts at +0.  So for a Diffuse hit rtx_trace_rays' colour is albedo * diffuse, and for a Phong hit
 *    (albedo * ambient + diffuse * kd) + specular * ks, bit for bit (scene.cpp:808, 852).
 * 4. light_open is the true visibility of every (ray, light) pair, the pairs with m == 0 included, which the frame kernels do not walk.
 *    When light_open_dev is NULL, a pair whose D and S are +0 for either answer is not walked.
 * 5. Every ray's results are independent of the other rays of the batch and of their order.
 *
 * Everything else follows rtx_surface_rays: asynchronous on `stream` and ordered against the view's preparation; nothing is queued on the
 * NULL stream; nothing is allocated and nothing waits for the device once the scene's ray scratch has grown to n; large batches are
 * regrouped as rtx_trace_rays' (knobs trace_reorder, trace_key_origin_first); n == 0 does nothing; n > 0xffffffc0 is refused; row
 * ownership is ignored; counters (rtx_counters_enable) are neither collected nor refused.  The scratch is the scene's, so calls on one
 * scene must not overlap on different streams.  A request for hits alone is rtx_trace_rays' for hits alone: the same launch.
 * RTX_ERR_ARG, the buffers untouched: NULL scene, NULL out, all six pointers NULL, a per-light pointer with n_lights != the scene's
 * current number of lights (a buffer sized before rtx_scene_set_lights) or on a scene without lights, NULL rays_dev with n > 0.
 * With zero lights diffuse and specular are +0. */
int rtx_light_rays(rtx_scene* scene, uint32_t n, const float* rays_dev, const rtx_light_buffers* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
