/* First-hit buffers of a frame: what the primary ray of every pixel met -- depth, object and triangle id, barycentric
 * uv, shading normal, albedo -- in one launch over the view, without a ray buffer.  An extension of the C ABI in rtx.h. */
#ifndef RTX_AOV_H
#define RTX_AOV_H
#include "rtx.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Device pointers owned by the caller, each indexed x + y * W like the framebuffer; any may be NULL (that channel is not computed), at
 * least one is not. */
typedef struct rtx_aov_buffers {
    float*   depth_dev;     /* H*W      */
    int32_t* object_dev;    /* H*W      */
    int32_t* triangle_dev;  /* H*W      */
    float*   uv_dev;        /* H*W x 2  */
    float*   normal_dev;    /* H*W x 3  */
    float*   albedo_dev;    /* H*W x 3  */
} rtx_aov_buffers;

/* For every pixel pass 1 renders -- x < W-1, y < H-1, y in [row_begin, min(row_end, H)), under rtx_set_row_ownership the rows this part
 * OWNS (halo rows are not needed here and are not written) -- the channels of
 *
 *     Render::trace(primaryRay(x + 0.5f, y + 0.5f), scene.objects, info)      (renderWorker scene.cpp:444-468, trace scene.cpp:724-756)
 *
 * and of getSurfaceData at its hit (scene.cpp:763-770).  Nothing else in any buffer is touched.
 *   depth, object, triangle, uv: fields 3, 1, 2 and (4, 5) of the record rtx_cast_rays returns for that ray, the ids as int32.  A miss:
 *       depth FLT_MAX, object -1, triangle -1, uv (-1, -1); a hit on a sphere or a plane: triangle -1.
 *   normal: hitNormal -- a sphere's objects.cpp:788-796, a plane's stored normal, a mesh's objects.cpp:121-151 with its normal map.
 *       normal / 2 + 0.5 in fp32 is bit for bit the colour the RTX_FLAG_SHOW_NORMALS view gives the ray.  A miss: (0, 0, 0).
 *   albedo: hitColor -- the object's colour or the texel of its diffuse map (objects.cpp:153-163).  A miss: getSkybox(dir), the sky texel
 *       under RTX_FLAG_SKYBOX and the background colour otherwise (what castRay returns for a ray that hits nothing).
 * The view's culling flag applies; max_ray_depth and RTX_FLAG_SHOW_NORMALS change nothing.  When neither normal nor albedo is asked for,
 * no surface data (uv coordinates, normals, tangents, maps) is fetched at all.
 *
 * Asynchronous on `stream` and ordered against the view's preparation as rtx_render_pass1 is; nothing is queued on the NULL stream, the
 * host does not wait and nothing is allocated.  The tile lists, the tile costs and the frame-mode measurements of the ordinary frames
 * are neither used nor changed.  row_begin >= row_end does nothing.
 * RTX_ERR_ARG, the buffers untouched: NULL scene, NULL out, all six pointers NULL.  RTX_ERR_UNSUPPORTED with counters enabled
 * (rtx_counters_enable), as for the debug views.
 *
 * Several GPUs: every channel is a plain image of H rows of W * 4, W * 8 or W * 12 bytes, so rtx_gather with that row_bytes assembles
 * any channel of a frame whose parts were rendered under rtx_set_row_ownership; there is no communication code of its own. */
int rtx_render_aov(rtx_scene* scene, uint32_t row_begin, uint32_t row_end, const rtx_aov_buffers* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
