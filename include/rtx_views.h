/* Many views of a scene in one call: pass 1 -- and, when asked, the Sobel mask and the 4-sample pass -- of a batch of cameras
 * and frame sizes, each into its own buffers, in one launch per stage over the whole batch.  For batches of views too small to fill the device
 * one at a time: the faces of a cube map, a ring of cameras, thumbnails of a camera path.  An extension of the C ABI in rtx.h. */
#ifndef RTX_VIEWS_H
#define RTX_VIEWS_H
#include "rtx.h"
#ifdef __cplusplus
extern "C" {
#endif

/* One view of a batch: a frame size, a camera and the caller's device buffers.  The camera fields are rtx_view's and mean the same. */
typedef struct rtx_view_target {
    uint32_t width, height;      /* > 0 (a view 1 pixel wide or high has no pixel that pass 1 renders) */
    float cam_pos[3];
    float cam_matrix[16];        /* as rtx_view's */
    float scale, aspect;         /* as rtx_view's */
    float* fb_dev;               /* height*width*3 floats, rtx_render_pass1's layout and rules (zeroed by the caller) */
    uint8_t* mask_dev;           /* height*width bytes; required when with_ssaa != 0, else may be NULL (it is not written) */
} rtx_view_target;

/* The limits of a batch: more views, a larger side, or more 8x8 tiles in all -- the sum of ceil(width/8) * ceil(height/8) over the views --
 * are refused.  (4 194 304 tiles: 4 096 views of 256 x 256, or four of 8 192 x 8 192.) */
#define RTX_VIEWS_MAX_VIEWS 65536u
#define RTX_VIEWS_MAX_SIDE  32768u
#define RTX_VIEWS_MAX_TILES 4194304u

/* Renders the n_views views of `views` (a host array, which may be reused as soon as the call returns).  View i receives, bit for bit, what
 * the one-view calls produce after rtx_scene_set_view with its camera and size:
 *   with_ssaa == 0: rtx_render_pass1 over all rows -- the pixels x < width-1, y < height-1; the last row and column are not written.
 *   with_ssaa != 0: rtx_render_pass1 + rtx_sobel + rtx_render_ssaa over all rows -- mask_dev is written completely, its borders 0.
 * Nothing outside a view's buffers is written.  Views may differ in size; two views must not share a buffer.
 *
 * Shared by every view of the batch, taken from the scene's CURRENT view (rtx_scene_set_view): bias, max_ray_depth, background and flags
 * (culling, skybox).  Only the camera and the size are per view: the ray kernels read those options from their argument block, which a
 * launch has once.
 *
 * The call leaves the scene's current view, its tile lists, tile costs, frame-mode measurements and timing slots (rtx_last_kernel_ms) as
 * they are: a rtx_render_frame after it renders what it would have rendered, and nothing is prepared again.
 *
 * Asynchronous on `stream`, ordered against the view's preparation as rtx_render_pass1 is.  The host waits only where the scene's scratch
 * for batches has to grow (a batch of more views or tiles than any before: 4 bytes per pixel with SSAA), or for the previous call's copy of
 * the view table out of its staging buffer -- never for a kernel.  As with the other render calls, calls on one scene must not overlap
 * on different streams.  n_views == 0 does nothing.
 *
 * Refused with the buffers untouched and the reason in rtx_last_error --
 * RTX_ERR_ARG: NULL scene; NULL views with n_views > 0; a zero width or height; a NULL fb_dev; a NULL mask_dev with with_ssaa; more than
 *   RTX_VIEWS_MAX_VIEWS views, a side above RTX_VIEWS_MAX_SIDE, more than RTX_VIEWS_MAX_TILES tiles; row ownership with more than one
 *   part (rtx_set_row_ownership: a multi-GPU caller deals out views, not rows).
 * RTX_ERR_UNSUPPORTED: counters enabled (rtx_counters_enable); RTX_FLAG_SHOW_NORMALS in the current view. */
int rtx_render_views(rtx_scene* scene, uint32_t n_views, const rtx_view_target* views /* host */, int with_ssaa, void* stream);

#ifdef __cplusplus
}
#endif
#endif
