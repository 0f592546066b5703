/* Texel points of a mesh's UV layout: which surface point {P, N} belongs to texel (i, j) of a map laid over a mesh by its
 * texture coordinates, and the margin fill a nearest-neighbour sampler needs around the charts.  The step between the scene's triangles and
 * the point queries (rtx_points.h, rtx_radiance.h), whose results go back into a map without leaving the device (rtx_texture.h):
 *     rtx_texel_points  ->  rtx_light_points / rtx_ao_points / rtx_radiance_points  ->  rtx_dilate_texels  ->  rtx_scene_set_map / _write_texels
 * The reference has no such function: the contract is written out here, every operation and its order.  An extension of the C ABI in rtx.h. */
#ifndef RTX_BAKE_H
#define RTX_BAKE_H
#include "rtx.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct rtx_texel_buffers {
    float*   points_dev; /* w*h x 6 {P.xyz, N.xyz}, rtx_light_points' layout */
    int32_t* tri_dev;    /* w*h: owning triangle, -1 = uncovered */
    float*   bary_dev;   /* w*h x 2 {bu, bv} */
} rtx_texel_buffers;     /* any may be NULL, not all */

/* rtx_texel_points: the surface point of every texel of a w x h map over mesh `mesh` (index among the scene's meshes).
 *
 * Layout.  Texel (i, j) is at index j * w + i, the row order in which the scene stores its maps: row j is v in [j/h, (j+1)/h), the texel the
 * sampler reads for (int)(w * u), (int)(h * v).  A float32 (h, w, 3) image computed from the points goes into rtx_scene_set_map unflipped.
 *
 * Arithmetic.  Every operation below is a single IEEE operation in the stated format, without contraction (no FMA).
 *  - Centre of texel (i, j): cx = ((float)i + 0.5f) / (float)w, cy = ((float)j + 0.5f) / (float)h, fp32.
 *  - Edge function of two UV vertices p, q at the centre c, fp64, every operand widened first:
 *        E(p, q, c) = (qx - px) * (cy - py) - (qy - py) * (cx - px)
 *    in canonical form: if (px, py) is lexicographically greater than (qx, qy) -- fp32 comparisons, x first, then y -- it is -E(q, p, c).
 *    Two triangles that share an edge see the same magnitude with opposite signs: the layout is watertight by construction.
 *  - Triangle t with UV corners a, b, c (tri_uv's order): w_a = E(b, c, .), w_b = E(c, a, .), w_c = E(a, b, .), D = (w_a + w_b) + w_c.
 *    t COVERS the texel iff the centre lies in the triangle's UV bounding box -- min(ax, bx, cx) <= cx <= max(ax, bx, cx) and likewise in y,
 *    fp32 comparisons, in exact arithmetic implied by what follows -- and
 *        D > 0 && w_a >= 0 && w_b >= 0 && w_c >= 0,   or   D < 0 && w_a <= 0 && w_b <= 0 && w_c <= 0.
 *    D == 0 and any NaN cover nothing; mirrored charts (D < 0) are legal.  Only the map's own texels exist: texture coordinates outside
 *    [0, 1) are not wrapped, and a triangle's bounding box is clipped to the map.
 *  - The OWNER of a texel is the lowest triangle index among the triangles that cover it: overlapping charts and exact ties on shared
 *    edges resolve by index, whatever the launch order and whatever the other triangles.
 *  - bu = (float)(w_b / D), bv = (float)(w_c / D), the divisions in fp64.
 *  - Per component in fp32, with k = (1.0f - bu) - bv, the owner's positions A, B, C and normals n_a, n_b, n_c:
 *        P = (B * bu + C * bv) + A * k        M = ((n_b * bu + n_c * bv) + n_a * k) / 3        N = Vec3::normalize(M)
 *    -- Mesh::getSurfaceData's formulas (objects.cpp:125-127) in their operand order.  The normal map is NOT applied (out of scope: a baker
 *    that wants the mapped normal perturbs N itself).
 *  - An uncovered texel gets tri = -1 and +0 in every float: a zero normal is never traced by rtx_ao_points and yields +0 light, unwalked,
 *    from rtx_light_points.
 * Every element of every non-NULL buffer is written, and nothing else.
 *
 * Asynchronous on `stream`; nothing is queued on the NULL stream; the host does not wait once the scene's scratch has grown to the map and
 * the mesh (w*h x 4 bytes and n_tris x 8 bytes, owned by the scene like the ray scratch and not counted by rtx_scene_bytes).  Ordered
 * against edits as the query calls are: a deformation (rtx_deform.h) or rtx_scene_set_objects before the call is seen.  The scratch is the
 * scene's, so calls on one scene must not overlap on different streams.
 *
 * RTX_ERR_ARG, the buffers untouched: NULL scene or out, all three pointers NULL, mesh >= the scene's number of meshes, w or h zero,
 * w * h > 0x7fffffff. */
int rtx_texel_points(rtx_scene* scene, uint32_t mesh, uint32_t w, uint32_t h, const rtx_texel_buffers* out, void* stream);

/* rtx_dilate_texels: the margin.  The sampler is nearest-neighbour, so a texel whose centre lies in no triangle is still read by hits whose
 * texture coordinate lies in its square (chart borders).  image_dev: w*h x channels floats (channels 1 .. 4), tri_dev: w*h as written by
 * rtx_texel_points; both are updated in place.  One pass: a texel with tri == -1 looks at its neighbours (di, dj) in the fixed order
 *     (-1,0) (1,0) (0,-1) (0,1) (-1,-1) (1,-1) (-1,1) (1,1),
 * skips those outside the map, and copies the image value of the first one whose tri != -1 AS OF THE START OF THE PASS; it then takes
 * tri = -2 (filled) at the end of the pass, so later passes grow from it.  A copy, no arithmetic: bit-exact and independent of the launch
 * order.  passes == 0 does nothing.  Asynchronous on `stream`, no host wait once the scene's scratch holds w*h words.
 * RTX_ERR_ARG, the buffers untouched: NULL scene, image_dev or tri_dev, channels outside 1 .. 4, w or h zero, w * h > 0x7fffffff. */
int rtx_dilate_texels(rtx_scene* scene, uint32_t w, uint32_t h, uint32_t channels, float* image_dev, int32_t* tri_dev, uint32_t passes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
