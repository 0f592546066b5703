/* Direct light of a frame: what castRay sums over the lights at the first hit of every pixel of pass 1 -- diffuseComponent
 * and specularComponent, each light's own term of both, and the number of each light's shadow rays that arrive -- in one launch over the
 * view, without a ray buffer: shadow masks per light, relighting a kept G-buffer, deferred composition with rtx_render_aov's albedo.  The
 * frame form of rtx_light_rays, declared in rtx_light.h, as rtx_render_ao is the frame form of rtx_occluded_rays.  An extension of the C ABI in rtx.h. */
#ifndef RTX_RENDER_LIGHT_H
#define RTX_RENDER_LIGHT_H
#include "rtx.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Device pointers owned by the caller; any may be NULL (that buffer is not written), at least one is not.  Every buffer is made of plain
 * images indexed x + y * W like the framebuffer; a per-light buffer is n_lights such images one after the other (light-major), so plane i
 * is an image of its own. */
typedef struct rtx_frame_light_buffers {
    uint32_t  n_lights;           /* the scene's current number of lights */
    float*    diffuse_dev;        /* H*W*3, pixel x + y*W: castRay's diffuseComponent at the pixel's first hit */
    float*    specular_dev;       /* H*W*3 */
    float*    light_diffuse_dev;  /* n_lights planes of H*W*3, light-major: plane i is an image of its own */
    float*    light_specular_dev; /* n_lights planes of H*W*3 */
    uint32_t* light_open_dev;     /* n_lights planes of H*W: shadow rays of light i that arrive */
} rtx_frame_light_buffers;

/* Pixels written: those rtx_render_aov writes -- x < W-1, y < H-1, y in [row_begin, min(row_end, H)), under rtx_set_row_ownership the
 * rows this part OWNS (no halo rows).  Nothing else in any buffer is touched; a NULL pointer is not written.
 *
 * The contract, per pixel, in fp32 without contraction:
 *  1. The ray and its first hit are rtx_render_aov's: primaryRay(x + 0.5f, y + 0.5f) and Render::trace under the view's culling flag;
 *     P = orig + dir * tNear, N = hitNormal (the `normal` channel of rtx_render_aov), ns = the hit object's n_specular.
 *  2. From there on steps 1 to 4 of rtx_light_rays' contract (rtx_light.h) apply word for word: O = P + N * view.bias; for the lights in
 *     scene order illuminate, open_i, D_i and S_i (an area light: its samples in stored order, dsum, ssum, the reference's powf); diffuse
 *     and specular are the sums from +0 in scene order; light_open is the true visibility of every (pixel, light) pair, and when
 *     light_open_dev is NULL a pair whose D and S are +0 for either answer is not walked.
 *     Every written value is the bits rtx_light_rays writes for the pixel's primary ray.
 *  3. A pixel whose ray hits nothing: zeros everywhere, light_open = 0.
 *  4. max_ray_depth, RTX_FLAG_SHOW_NORMALS and the skybox flag change nothing.
 *
 * Asynchronous on `stream` and ordered against the view's preparation as rtx_render_ao is; nothing is queued on the NULL stream, the
 * host does not wait, nothing is allocated and no event is recorded.  The tile lists, the tile costs and the frame-mode measurements of
 * the ordinary frames are neither used nor changed.  row_begin >= row_end does nothing.
 * RTX_ERR_ARG, the buffers untouched: NULL scene, NULL out, all five pointers NULL, a per-light pointer with n_lights != the scene's
 * current number of lights (a buffer sized before rtx_scene_set_lights) or on a scene without lights.  RTX_ERR_UNSUPPORTED with counters
 * enabled (rtx_counters_enable).  With zero lights diffuse and specular are +0 at every written pixel.
 *
 * Several GPUs: each plane is a plain image of H rows of W * 12 (W * 4: light_open) bytes, so rtx_gather with that row_bytes assembles
 * a plane whose parts were rendered under rtx_set_row_ownership; there is no communication code of its own. */
int rtx_render_light(rtx_scene* scene, uint32_t row_begin, uint32_t row_end, const rtx_frame_light_buffers* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
