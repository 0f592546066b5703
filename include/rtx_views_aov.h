/* First-hit buffers and primary rays of many views in one call: for a batch of cameras and frame sizes, what the primary
 * ray of every pixel met -- the six channels of rtx_render_aov --, the hit point, and the ray itself, each view into its own buffers, in
 * one launch over the whole batch and without preparing a view.  For multi-view data, depth cube maps at probes, id thumbnails along a
 * camera path -- and, through the `rays` channel, the link from a camera to the ray queries (rtx_trace_rays, rtx_surface_rays, ...).  An
 * extension of the C ABI in rtx.h. */
#ifndef RTX_VIEWS_AOV_H
#define RTX_VIEWS_AOV_H
#include "rtx.h"
#include "rtx_views.h"      /* RTX_VIEWS_MAX_*: the limits of a batch are that header's */
#ifdef __cplusplus
extern "C" {
#endif

/* One view of a batch: a frame size, a camera and the caller's device buffers, each indexed x + y * width.  The camera fields are
 * rtx_view_target's and mean the same.  A channel whose pointer is NULL is not computed. */
typedef struct rtx_view_aov_target {
    uint32_t width, height;      /* > 0 (a view 1 pixel wide or high has no pixel that pass 1 renders) */
    float cam_pos[3];
    float cam_matrix[16];        /* as rtx_view's */
    float scale, aspect;         /* as rtx_view's */
    float*   depth_dev;          /* height*width     */
    int32_t* object_dev;         /* height*width     */
    int32_t* triangle_dev;       /* height*width     */
    float*   uv_dev;             /* height*width x 2 */
    float*   normal_dev;         /* height*width x 3 */
    float*   albedo_dev;         /* height*width x 3 */
    float*   position_dev;       /* height*width x 3 */
    float*   rays_dev;           /* height*width x 6 */
} rtx_view_aov_target;

/* For every view i of `views` (a host array, which may be reused as soon as the call returns) and every pixel pass 1 renders --
 * x < width-1, y < height-1; a view one pixel wide or high gets nothing -- the channels of the pixel's primary ray: viewRay of the view at
 * (x + 0.5f, y + 0.5f), the ray rtx_render_views casts for that pixel and rtx_render_pass1 casts after rtx_scene_set_view with this
 * camera and size.  Nothing else in any buffer is touched.  Views may differ in size; two views must not share a buffer.
 *   depth, object, triangle, uv, normal, albedo: bit for bit what rtx_render_aov writes after rtx_scene_set_view with the view's camera
 *       and size, its miss values included: FLT_MAX, -1, -1, (-1, -1), (0, 0, 0), the sky texel / the background colour.
 *   position: bit for bit rtx_surface_rays' position for that ray -- orig + dir * tNear, the product rounded before the sum; a miss:
 *       (0, 0, 0).
 *   rays: {cam_pos, d}, the six floats of the ray itself, for hits and misses alike.  Handed to rtx_trace_rays they give the hit record
 *       whose fields 3, 1, 2 and (4, 5) are this call's depth, object, triangle and uv, and the colour rtx_render_views writes for
 *       the pixel.
 *
 * Shared by every view of the batch, taken from the scene's CURRENT view (rtx_scene_set_view) as in rtx_render_views: the culling flag,
 * and the skybox flag and the background, which decide albedo at a miss.  max_ray_depth, bias and RTX_FLAG_SHOW_NORMALS change nothing,
 * as for rtx_render_aov.
 *
 * One channel set for the batch: a pointer is NULL in every view or in none, and at least one channel is given (a launch compiles its
 * stores once; a caller who wants other channels for some views makes two calls).  When none of normal, albedo and position is asked
 * for, no surface data (uv coordinates, normals, tangents, maps) is fetched at all.
 *
 * The call leaves the scene's current view, its tile lists, tile costs, frame-mode measurements and timing slots (rtx_last_kernel_ms) as
 * they are: a rtx_render_frame after it renders what it would have rendered, and nothing is prepared again.
 *
 * Asynchronous on `stream`, ordered against the view's preparation as rtx_render_views is; nothing is queued on the NULL stream.  The
 * host waits only where the batch's table has to grow (more views than any batch before), or for the previous call's copy of the table
 * out of its staging buffer -- never for a kernel.  A second call with the same batch allocates nothing.  As with the other render
 * calls, calls on one scene must not overlap on different streams.  n_views == 0 does nothing.
 *
 * Refused with the buffers untouched and the reason in rtx_last_error, which names the view and the argument --
 * RTX_ERR_ARG: NULL scene; NULL views with n_views > 0; a zero width or height; more than RTX_VIEWS_MAX_VIEWS views, a side above
 *   RTX_VIEWS_MAX_SIDE, more than RTX_VIEWS_MAX_TILES tiles; no channel at all; a channel given in some views and not in others; row
 *   ownership with more than one part (rtx_set_row_ownership: a multi-GPU caller deals out views, not rows).
 * RTX_ERR_UNSUPPORTED: counters enabled (rtx_counters_enable). */
int rtx_render_views_aov(rtx_scene* scene, uint32_t n_views, const rtx_view_aov_target* views /* host */, void* stream);

#ifdef __cplusplus
}
#endif
#endif
