/* Diagnostics, probes and tuning hooks of librtx_hip.so -- NOT part of the drop-in boundary (include/rtx.h is): nothing a
 * reference-side caller binds.  They exist for the parity tests (tests/), bench.py's reporting and the A/B
 * tools; every symbol here may change between rounds.  No entry point in this header changes a pixel. */
#ifndef RTX_DEBUG_H
#define RTX_DEBUG_H
#include "rtx.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Which way rtx_render_frame rendered the last frame (0 three launches, 1 one) and what it measured; forcing either (tests, A/B runs). */
int rtx_frame_mode(rtx_scene* scene, int* mode, float* split_ms, float* fused_ms);
int rtx_set_frame_mode(rtx_scene* scene, int mode); /* -1 measure and choose (default), 0 always three launches, 1 always one */

/* Host only (no device is touched): what rtx_scene_create derives from a mesh before uploading it -- the tree with S = rtx_wide_node_slots()
 * descendants per node (log2 S binary levels per fetch; n_wide records of 32 S bytes: S slots of {lo.x hi.x lo.y hi.y lo.z hi.z, link,
 * first}; 0 when the boxes are not nested) and the prune blocks of its slots (n_wide records of 64 S bytes: S {c[3], P, h[3], Pgen} then S
 * {qc[3], wlo, qr[3], whi}; rtx_device.h, DESIGN_HISTORY.md 3.1c), plus the record of the whole mesh.  For the CPU tests of their
 * invariants (tests/test_host_cpu.py); cap_wide = records the output arrays hold. */
int rtx_mesh_flatten_probe(const rtx_mesh* mesh, uint32_t* n_wide, void* wide_out, void* prune_out, uint32_t cap_wide, float* root_rec8);
int rtx_wide_node_slots(void);      /* slots of a wide node: 8 */

/* Host only (no device is touched): the one-launch-or-three policy of rtx_render_frame (csrc/rtx_frame_plan.h, decideFrameMode).  forced -1 / 0 / 1
 * (rtx_set_frame_mode combined with the knob), has_list: the call renders some row; of its tile list: fused_gave_up, listed tiles, warm (its
 * costs are known), frame_samples2 / frame_ms2 (frames measured in three launches and in one, the best time of either), frames_seen;
 * rule_tiles: the knob frame_rule_tiles of the scene's kind.  *mode 0 three launches, 1 one; *reprobe: the frame's time replaces what was
 * known of its way; *probing: the frame is bracketed by its own pair of events.  tests/test_frame_plan_cpu.py. */
int rtx_frame_mode_probe(int forced, int has_list, int fused_gave_up, uint32_t listed, uint32_t rule_tiles, int warm, const uint32_t* frame_samples2,
                         const float* frame_ms2, uint32_t frames_seen, int* mode, int* reprobe, int* probing);

/* Host only (no device is touched): the pass-1 tile list of the rows [row_begin, row_end) of a width x height view under the row ownership
 * (band_height, n_parts, part, halo: rtx_set_row_ownership), with the 64 x 1 strips of lone halo rows when strips != 0 and the frame's size allows
 * them, and the tile rectangle rect4 = {tx0, tx1, ty0, ty1} whose tiles go first in their queues: the words the device is made to write
 * (csrc/rtx_frame_plan.h: TileGrid, planTileList, expectedTileList) -- [0, 8) the first entry of each of the eight queues, [8, 16) their
 * lengths, then the entries (ty << 16 | tx, or 0x10000000 | strip << 16 | y).  *need = the words; written to out when cap >= *need (out may
 * be NULL to ask for the length).  tests/test_frame_plan_cpu.py. */
int rtx_tile_list_probe(uint32_t width, uint32_t height, uint32_t band_height, uint32_t n_parts, uint32_t part, int halo, uint32_t row_begin, uint32_t row_end,
                        int strips, const uint32_t* rect4, uint32_t* out, size_t cap, size_t* need);

/* Host only (no device is touched): the work items of a batch of views (include/rtx_views.h: rtx_render_views) for n_views views of the sizes sizes2 = {width0,
 * height0, width1, height1, ...}, through the map the kernels use (csrc/rtx_views_plan.h: the first item of every view, viewOfItem,
 * tileOfItem).  *n_items = their number; items3_out (may be NULL to ask for the number) receives, when cap_items >= *n_items, three words
 * per item in item order: its view and the tile (tx, ty) of the view -- the pixels [8 tx, 8 tx + 8) x [8 ty, 8 ty + 8).  RTX_ERR_ARG for
 * the sizes and counts rtx_render_views refuses.  tests/test_render_views_cpu.py. */
int rtx_views_plan_probe(uint32_t n_views, const uint32_t* sizes2, uint32_t* items3_out, size_t cap_items, size_t* n_items);

/* Host only: the P of the source copies of the prune records (rtx_device.h PruneRec, csrc/rtx_source.hip sourceP; DESIGN_HISTORY.md 3.1d)
 * for n triangles given as (v0, e1, e2) = 9 floats each, the source point S3, its radius sigma and cam != 0 when the rays start
 * at S (the camera) rather than pass through it (a point light).  The function the device kernels run, for the CPU tests of the
 * bound (tests/test_prune_bound_cpu.py). */
int rtx_source_p_probe(const float* tris9, uint32_t n, const double* S3, double sigma, int cam, float* out);

/* First-frame cost estimate (rtx_scene_create / rtx_scene_set_view project every leaf box of the meshes through the camera;
 * the reference renders one frame per process, main.cpp:15, so there is no previous frame to learn the tile costs from):
 * per cell of 2 x 2 tiles (16 x 16 pixels) the references and the leaves whose boxes cover it, interleaved (refs, leaves),
 * grid_w x grid_h cells.  out == NULL: only the dimensions.  Diagnostic (tools/cost_fit.py); no pixel depends on the estimate. */
int rtx_cost_grid_read(rtx_scene* scene, uint32_t* out, size_t n, uint32_t* grid_w, uint32_t* grid_h);

/* Experiment / test knobs of a live scene.  Their environment variables (RTX_STRIP_LIMIT, RTX_SSAA_HEAVY_TICKS,
 * RTX_SSAA_SPREAD_SLOTS, RTX_SPLIT_PERCENT, RTX_SSAA_LOCAL_BELOW, RTX_SSAA_SPARSE_BELOW, RTX_FRAME_QUEUE_CAP, RTX_DEBUG_ITEMS, ...) are read
 * once, by rtx_scene_create, and only when RTX_ALLOW_ENV_KNOBS=1 is set (the product ignores RTX_* variables otherwise); names here: strip_limit, ssaa_heavy_ticks, ssaa_spread_slots, split_percent,
 * ssaa_local_below, ssaa_sparse_below, frame_queue_cap, frame_rule_tiles, frame_rule_tiles_analytic, debug_items; and for rtx_trace_rays
 * trace_reorder (1 always group the rays by key first, 0 never, -1 by their number and the coherence of their order: the default) and trace_key_origin_first (1: the key's interleave
 * starts with the origin's bits, the default; 0: with the direction's), both of which act on the occlusion query of include/rtx_query.h too, whose own knob is
 * occluded_scene_order (1: the objects in scene order; 0: spheres and planes before the meshes, the default).  prune_boxes (RTX_PRUNE_BOXES): the mesh kernels with the box test of
 * the prune records -1 where some mesh has small enough triangles (the default), 0 never, 1 for every mesh with prune records; taken by the
 * next launch.  No knob changes a pixel or a ray's result. */
int rtx_set_knob(rtx_scene* scene, const char* name, double value);

/* The compile-time variant the scene's next mesh launches take (pass 1, SSAA, the single-launch frame, rtx_trace_rays' hit and colour
 * kernels): the fields the launches read, as bits.  The hit kernel has no PLAIN variant; analytic scenes (no mesh) launch kernels without the
 * walk, and statistics the instrumented ones, whatever the other bits say. */
#define RTX_VARIANT_BOXES    1u      /* the box test of the prune records */
#define RTX_VARIANT_PLAIN    2u      /* every object Diffuse, no area light: no recursion, powf or area-light sums */
#define RTX_VARIANT_ANALYTIC 4u      /* no triangle mesh */
#define RTX_VARIANT_STATS    8u      /* statistics collected (rtx_counters_enable) */
#define RTX_VARIANT_CULL     16u     /* back-face culling of the view */
int rtx_kernel_variant(rtx_scene* scene, uint32_t* bits);

/* What the last rtx_render_ssaa built (also the SSAA stage of a frame rendered in three launches); synchronises the device.
 * info[16]: [0] tile-local layout (every tile's pixels padded to whole waves), [1] the flagged pixels the layout was decided from,
 * [2] the "sparse" layout, [3] tiles of the list (T = ceil(width/8) * ceil(height/8) for a whole frame), [4] tiles per row
 * (ceil(width/8)), [5] the heavy threshold the list was built with (ticks), [6] its slot budget of the 4-pixel and one-pixel waves,
 * [7] RTX_SSAA_VERY, [8] RTX_SSAA_SPREAD_PX; of the last frame rendered in one launch: [9] [10] its two split limits (ticks, 0xffffffff:
 * nothing split), [11] [12] the cost sum they were derived from (low, high word), [13] its waves.  scan (NULL: only info), n = 2 T + 1:
 * the list's exclusive scan -- tile t owns the slots [scan[t], scan[t + 1]) when it was heavy, [scan[T + t], scan[T + t + 1]) otherwise,
 * and its other range is empty.  Valid until the next rtx_render_ssaa of the scene: a frame in one launch builds no list and leaves it. */
int rtx_ssaa_list_read(rtx_scene* scene, uint32_t* info, uint32_t* scan, size_t n);

/* Launch counts and summed durations of kernel `which` (rtx_last_kernel_ms in rtx.h) since rtx_kernel_time_reset; synchronises on the recorded events. */
int rtx_kernel_time_reset(rtx_scene* scene);
int rtx_kernel_time_stats(rtx_scene* scene, int which, uint32_t* launches, double* total_ms);

/* Per-tile cost of the most recent rtx_render_pass1 (profiling aid; also what orders the SSAA work list):
 * out[ty * ceil(width/8) + tx] = wall-clock ticks (100 MHz) one wave spent on the 8x8 pixel tile (tx, ty).
 * n must be ceil(width/8) * ceil(height/8) -- or twice that: the second half then holds, per tile, the slowest SSAA
 * work item of the most recent rtx_render_ssaa (ticks, scaled to a 16-pixel item).  Synchronises the device. */
int rtx_tile_cost_read(rtx_scene* scene, uint32_t* out, size_t n);

/* Self-check of the device math the parity contract depends on: evaluates powf / normalize / division /
 * sqrt on `n` inputs on the device so tests can compare with the host.  op: 0 powf(x,y), 1 1/x,
 * 2 sqrtf(x), 3 (float)(1/sqrt((double)x)), 4 x/y. */
int rtx_math_probe(int device, int op, uint32_t n, const float* x, const float* y, float* out);

/* The shading path's vector helpers on the device, n inputs at a time (host buffers, n x 3 floats; unit tests against the
 * reference's vectors).  op: 0 Render::reflect(a, b) (scene.cpp:672-675), 1 Render::refract(a, b, ior) (677-696),
 * 2 Render::fresnel(a, b, ior) in out[3 i] (698-722), 3 Vec3::normalize(a) (geometry.h:104-112; b may be NULL). */
int rtx_vec_probe(int device, int op, uint32_t n, const float* a, const float* b, float ior, float* out);

/* Host only: the description as one canonical byte string (every scalar and the contents of every array rtx_scene_create reads, in declaration
 * order; no pointers, no padding).  *need = its length; written to out when cap >= *need (out may be NULL to ask for the length).  The parity
 * check of the reference-side binding (oracle/ref_binding.cpp) against this repo's host: tests/test_ref_binding.py. */
int rtx_desc_serialize(const rtx_scene_desc* desc, void* out, size_t cap, size_t* need);

/* rtx_bvh_build builds in a handful of launches (two persistent ones walk the tree through a queue of nodes); the level-by-level build of rounds 1-4 remains
 * as its fallback (a pool ran out, its watchdog fired).  mode 1 forces the fallback (tests compare the two), mode 2 gives the persistent launches pools that are far
 * too small (tests: they must give up cleanly and the fallback must take over); process-wide. */
int rtx_bvh_build_mode(int mode);
/* Kernel launches (fills included) of a finished build, and whether the persistent launches did it (1) or the level-by-level build (0). */
int rtx_bvh_launches(const rtx_bvh* bvh, uint32_t* launches, int* queued);

/* Read-backs of a scene's current geometry (the edits of include/rtx_scene_edit.h are checked through them).  rtx_scene_mesh_read: mesh
 * `mesh`'s tree as the device holds it, in the rtx_mesh layout (counts2 = {n_nodes, n_refs}; with every array NULL only the counts).
 * rtx_scene_mesh_flat_read: its wide nodes, prune blocks (the copy any ray uses) and whole-mesh record in rtx_mesh_flatten_probe's layout.
 * rtx_scene_edit_times: host wall ms of the last rtx_scene_update_mesh -- {device build, flatten on the device + records swapped in, view
 * preparation queued, whole call}. */
int rtx_scene_mesh_read(rtx_scene* scene, uint32_t mesh, uint32_t* counts2, float* node_bounds, int32_t* node_skip, int32_t* leaf_begin,
                        int32_t* leaf_count, uint32_t* refs);
int rtx_scene_mesh_flat_read(rtx_scene* scene, uint32_t mesh, uint32_t* n_wide, void* wide_out, void* prune_out, uint32_t cap_wide, float* root_rec8);
int rtx_scene_edit_times(rtx_scene* scene, float* ms4);
/* rtx_scene_lights_read: the light records as the device holds them, in the rtx_light layout with points = NULL -- the sample points of the
 * area lights follow one another in points_out, in light order, 3 n_points floats each.  *n_lights / *n_point_floats: what there is;
 * lights_out / points_out (either may be NULL) are written up to cap_lights records / when all the points fit cap_point_floats.
 * rtx_scene_mesh_prune_copy_read: copy `copy` of mesh `mesh`'s prune blocks (0 the one any ray uses, 1 the camera's, 2 + l point light
 * l's; rtx_mesh_flatten_probe's prune layout, up to cap_wide records); *n_copies = the copies the mesh holds (0: no prune blocks), with
 * prune_out == NULL only the counts.  Both synchronise the device. */
int rtx_scene_lights_read(rtx_scene* scene, uint32_t* n_lights, rtx_light* lights_out, uint32_t cap_lights, size_t* n_point_floats,
                          float* points_out, size_t cap_point_floats);
int rtx_scene_mesh_prune_copy_read(rtx_scene* scene, uint32_t mesh, uint32_t copy, uint32_t* n_copies, uint32_t* n_wide, void* prune_out,
                                   uint32_t cap_wide);
/* The object records decoded from device memory (not from the host's copy) into the description's layout: *n_objects / *n_meshes what
 * the scene holds, objects_out (may be NULL) written up to cap_objects records.  Synchronises the device. */
int rtx_scene_objects_read(rtx_scene* scene, uint32_t* n_objects, rtx_object* objects_out, uint32_t cap_objects, uint32_t* n_meshes);

/* Device allocations this library holds at the moment, in this process, and their bytes: everything behind scenes, acceleration structures and
 * communicators, scratch of calls in progress included (not the caller's own buffers).  Back where it was once everything created since has been
 * destroyed -- which a test can check on a GPU it shares with others.  Either pointer may be NULL. */
int rtx_live_device_memory(size_t* allocations, size_t* bytes);

/* The placement and triangle assembly of include/rtx_deform.h on host arrays, without a scene and without a tree: pos n_pos x 3, nrm n_nrm x 3
 * raw normals or NULL (the topology's stored ones).  device >= 0: exactly the three kernels of csrc/rtx_deform.hip on that device, their
 * results copied back; device < 0: the same functions (csrc/rtx_place.h) on the CPU, the box by the loader's sequential rule.  tri24_out: n_tris x 9
 * positions, then n_tris x 9 normals, then n_tris x 6 tangents and bitangents (always computed); lo_hi_out[12]: the vertices' box lo, hi, the root
 * box lo, hi; flags_out[2]: some input is not finite (nothing else is written then), some placed position is not finite (the triangles are
 * written all the same: how the NaN cases are compared).  tests/test_deform_cpu.py, tests/test_gpu_deform.py. */
struct rtx_mesh_topology;
struct rtx_mesh_pose;
int rtx_place_probe(int device, const struct rtx_mesh_topology* topology, const float* pos, const float* nrm, const struct rtx_mesh_pose* pose,
                    float* tri24_out, float* lo_hi_out, uint32_t* flags_out);

#ifdef __cplusplus
}
#endif
#endif
