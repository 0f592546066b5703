"""rendering_amd -- MI355X (gfx950) implementation of the holoskii/Rendering per-pixel ray-trace hot path.

Python is plumbing only: this module binds (ctypes)
  * librtx_hip.so          -- the C ABI of include/rtx.h: HIP kernels + one-time scene upload
  * librendering_host.so   -- the C++17 host side (Scene/Options/Object API, .scene/OBJ/BMP loaders, BVH build)
and moves device pointers of torch tensors across that boundary (torch is used for device memory, streams and
torch.distributed only).  There is NO CPU fallback: without the compiled libraries `load()` raises, and
without a GPU every render call fails loudly with the HIP error.  Nothing here imports oracle/.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB_RTX = os.path.join(HERE, "librtx_hip.so")
LIB_HOST = os.path.join(HERE, "librendering_host.so")

__all__ = ["load", "Scene", "Comm", "RtxError", "device_count", "math_probe", "gather_plan", "exported_symbols", "sphere_directions", "cube_cameras", "decode_texels"]


class RtxError(RuntimeError):
    pass


class Counters(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("box_tests", C.c_uint64), ("tri_tests", C.c_uint64), ("moot_rays", C.c_uint64)]


_rtx = None
_host = None

# every entry point declared in include/rtx.h (the boundary) and include/rtx_debug.h (probes, diagnostics, tuning hooks)
RTX_SYMBOLS = [
    "rtx_last_error", "rtx_device_count", "rtx_scene_create", "rtx_scene_destroy", "rtx_scene_set_view", "rtx_scene_bytes",
    "rtx_render_pass1", "rtx_sobel", "rtx_render_ssaa", "rtx_render_frame", "rtx_render_ac", "rtx_frame_status", "rtx_frame_mode", "rtx_set_frame_mode", "rtx_set_knob", "rtx_cost_grid_read", "rtx_mesh_flatten_probe", "rtx_wide_node_slots", "rtx_source_p_probe", "rtx_quantize_bgr8", "rtx_render_frame_host",
    "rtx_counters_enable", "rtx_counters_reset", "rtx_counters_read", "rtx_last_kernel_ms", "rtx_math_probe",
    "rtx_cast_rays", "rtx_trace_rays", "rtx_kernel_time_reset", "rtx_kernel_time_stats", "rtx_tile_cost_read", "rtx_set_row_ownership",
    "rtx_bvh_build", "rtx_bvh_info", "rtx_bvh_read", "rtx_bvh_destroy",
    "rtx_vec_probe", "rtx_desc_serialize", "rtx_bvh_build_mode", "rtx_bvh_launches", "rtx_comm_unique_id", "rtx_comm_create", "rtx_comm_info", "rtx_comm_destroy", "rtx_comm_agree", "rtx_gather", "rtx_gather_plan",
    "rtx_scene_mesh_read", "rtx_scene_mesh_flat_read", "rtx_scene_edit_times", "rtx_kernel_variant", "rtx_ssaa_list_read", "rtx_live_device_memory",
    "rtx_scene_lights_read", "rtx_scene_mesh_prune_copy_read", "rtx_scene_objects_read",
    "rtx_frame_mode_probe", "rtx_tile_list_probe", "rtx_place_probe",
    "rtx_views_plan_probe",
]

# the extension of include/rtx_scene_edit.h: editing a live scene (not part of the drop-in boundary)
RTX_EDIT_SYMBOLS = ["rtx_scene_set_object", "rtx_scene_update_mesh", "rtx_scene_set_lights", "rtx_scene_set_objects"]

# the extension of include/rtx_query.h: queries on a loaded scene that render nothing (not part of the drop-in boundary)
RTX_QUERY_SYMBOLS = ["rtx_occluded_rays"]

# the extension of include/rtx_aov.h: first-hit buffers of a frame (not part of the drop-in boundary)
RTX_AOV_SYMBOLS = ["rtx_render_aov"]


# the extension of include/rtx_ao.h: ambient occlusion of a frame (not part of the drop-in boundary)
RTX_AO_SYMBOLS = ["rtx_render_ao"]

# the extension of include/rtx_surface.h: surface data at the hits of caller-supplied rays (not part of the drop-in boundary)
RTX_SURFACE_SYMBOLS = ["rtx_surface_rays"]

# the extension of include/rtx_light.h: direct light at the hits of caller-supplied rays (not part of the drop-in boundary)
RTX_LIGHT_SYMBOLS = ["rtx_light_rays"]

# the extension of include/rtx_scatter.h: reflection and refraction rays at the hits of caller-supplied rays, and the sky colour of rays
# (not part of the drop-in boundary)
RTX_SCATTER_SYMBOLS = ["rtx_scatter_rays", "rtx_sky_rays"]

# the extension of include/rtx_points.h: direct light and ambient occlusion at caller-supplied surface points (not part of the drop-in
# boundary)
RTX_POINTS_SYMBOLS = ["rtx_light_points", "rtx_ao_points"]

# the extension of include/rtx_render_light.h: direct light of a frame (not part of the drop-in boundary)
RTX_RENDER_LIGHT_SYMBOLS = ["rtx_render_light"]

# the extension of include/rtx_radiance.h: radiance gathered over directions at caller-supplied surface points (not part of the drop-in
# boundary)
RTX_RADIANCE_SYMBOLS = ["rtx_radiance_points"]

# the extension of include/rtx_deform.h: deforming a mesh of a live scene from vertices on the device (not part of the drop-in boundary)
RTX_DEFORM_SYMBOLS = ["rtx_scene_set_mesh_topology", "rtx_scene_deform_mesh"]

# the extension of include/rtx_views.h: many views of a scene in one call (not part of the drop-in boundary; its probe, rtx_views_plan_probe, is
# declared in include/rtx_debug.h and listed with the probes above)
RTX_VIEWS_SYMBOLS = ["rtx_render_views"]

# the extension of include/rtx_views_aov.h: first-hit buffers and primary rays of many views in one call (not part of the drop-in boundary)
RTX_VIEWS_AOV_SYMBOLS = ["rtx_render_views_aov"]

# the extension of include/rtx_texture.h: texture maps and skybox of a live scene replaced from device memory (not part of the drop-in boundary)
RTX_TEXTURE_SYMBOLS = ["rtx_scene_set_map", "rtx_scene_set_sky", "rtx_scene_write_texels", "rtx_scene_texture_info"]
TEXTURE_KINDS = {"diffuse": 0, "normal": 1, "specular": 2, "sky": 3}      # RTX_TEX_*
TEXELS_STORED, TEXELS_RGB8 = 0, 1                                          # RTX_TEXELS_*

# the extension of include/rtx_bake.h: the surface points of a mesh's texels and the margin fill (not part of the drop-in boundary)
RTX_BAKE_SYMBOLS = ["rtx_texel_points", "rtx_dilate_texels"]


# the extension of include/rtx_project.h: surface points projected into cameras, with visibility (not part of the drop-in boundary)
RTX_PROJECT_SYMBOLS = ["rtx_project_points"]
PROJECT_CAMERA_FLOATS = 24                                                 # RTX_PROJECT_CAMERA_FLOATS
PROJ_FRONT, PROJ_INSIDE, PROJ_FACING, PROJ_OPEN = 1, 2, 4, 8               # RTX_PROJ_*


class ProjectBuffers(C.Structure):
    """rtx_project_buffers (include/rtx_project.h): three device pointers, any of them NULL."""
    _fields_ = [(n, C.c_void_p) for n in ("pixel_dev", "depth_dev", "flags_dev")]


class TexelBuffers(C.Structure):
    """rtx_texel_buffers (include/rtx_bake.h): three device pointers, any of them NULL."""
    _fields_ = [(n, C.c_void_p) for n in ("points_dev", "tri_dev", "bary_dev")]


class RtxTexels(C.Structure):
    """rtx_texels (include/rtx_texture.h)"""
    _fields_ = [("format", C.c_int32), ("width", C.c_uint32), ("height", C.c_uint32), ("data_dev", C.c_void_p), ("row_pitch", C.c_int64)]


class MeshTopology(C.Structure):
    """rtx_mesh_topology (include/rtx_deform.h): six counts, then five host pointers."""
    _fields_ = [(n, C.c_uint32) for n in ("n_tris", "n_pos", "n_nrm", "n_uv", "placed_pos", "placed_nrm")] + \
               [(n, C.c_void_p) for n in ("corner_pos", "corner_nrm", "corner_uv", "uv", "nrm")]


class MeshPose(C.Structure):
    """rtx_mesh_pose (include/rtx_deform.h)"""
    _fields_ = [("pos", C.c_float * 3), ("rot_matrix", C.c_float * 16), ("size", C.c_float * 3), ("bias", C.c_float), ("ac_penalty", C.c_int32)]


class AovBuffers(C.Structure):
    """rtx_aov_buffers (include/rtx_aov.h): six device pointers, any of them NULL."""
    _fields_ = [(n, C.c_void_p) for n in ("depth_dev", "object_dev", "triangle_dev", "uv_dev", "normal_dev", "albedo_dev")]


class SurfaceBuffers(C.Structure):
    """rtx_surface_buffers (include/rtx_surface.h): five device pointers, any of them NULL."""
    _fields_ = [(n, C.c_void_p) for n in ("hits_dev", "position_dev", "normal_dev", "albedo_dev", "specular_dev")]


class LightBuffers(C.Structure):
    """rtx_light_buffers (include/rtx_light.h): the scene's number of lights and six device pointers, any of them NULL."""
    _fields_ = [("n_lights", C.c_uint32)] + [(n, C.c_void_p) for n in ("hits_dev", "diffuse_dev", "specular_dev", "light_diffuse_dev",
                                                                       "light_specular_dev", "light_open_dev")]


class FrameLightBuffers(C.Structure):
    """rtx_frame_light_buffers (include/rtx_render_light.h): the scene's number of lights and five device pointers, any of them NULL."""
    _fields_ = [("n_lights", C.c_uint32)] + [(n, C.c_void_p) for n in ("diffuse_dev", "specular_dev", "light_diffuse_dev",
                                                                       "light_specular_dev", "light_open_dev")]


class ScatterBuffers(C.Structure):
    """rtx_scatter_buffers (include/rtx_scatter.h): six device pointers, any of them NULL."""
    _fields_ = [(n, C.c_void_p) for n in ("hits_dev", "local_dev", "reflect_dev", "refract_dev", "weight_dev", "kinds_dev")]


class ViewTarget(C.Structure):
    """rtx_view_target (include/rtx_views.h): one view of a batch -- size, camera, device buffers."""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("cam_pos", C.c_float * 3), ("cam_matrix", C.c_float * 16),
                ("scale", C.c_float), ("aspect", C.c_float), ("fb_dev", C.c_void_p), ("mask_dev", C.c_void_p)]


class ViewAovTarget(C.Structure):
    """rtx_view_aov_target (include/rtx_views_aov.h): one view of a batch -- size and camera as ViewTarget's, then eight device pointers."""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("cam_pos", C.c_float * 3), ("cam_matrix", C.c_float * 16),
                ("scale", C.c_float), ("aspect", C.c_float)] + \
               [(n, C.c_void_p) for n in ("depth_dev", "object_dev", "triangle_dev", "uv_dev", "normal_dev", "albedo_dev", "position_dev", "rays_dev")]


def cube_cameras(pos):
    """The six cameras of a cube map at `pos` for Scene.render_views, as (pos, rot, 90): the faces +x, -x, +y, -y, +z, -z (the camera
    looks along -z of its own frame; rot in degrees, as in a scene file's [camera] block)."""
    p = tuple(float(x) for x in np.asarray(pos, np.float32).reshape(3))
    return [(p, rot, 90.0) for rot in ((0.0, 90.0, 0.0), (0.0, -90.0, 0.0), (-90.0, 0.0, 0.0), (90.0, 0.0, 0.0), (0.0, 180.0, 0.0), (0.0, 0.0, 0.0))]


def views_plan_probe(sizes):
    """Host only: the work items of Scene.render_views for views of the sizes [(width, height), ...] (rtx_views_plan_probe): uint32
    (n_items, 3) of (view, tx, ty) in item order."""
    rtx, _ = load()
    sz = np.ascontiguousarray(np.asarray(sizes, np.uint32).reshape(-1, 2))
    n = C.c_size_t(0)
    _check(rtx.rtx_views_plan_probe(sz.shape[0], _np_ptr(sz), None, 0, C.byref(n)), "rtx_views_plan_probe")
    out = np.zeros((n.value, 3), np.uint32)
    _check(rtx.rtx_views_plan_probe(sz.shape[0], _np_ptr(sz), _np_ptr(out), n.value, C.byref(n)), "rtx_views_plan_probe")
    return out


class AoParams(C.Structure):
    """rtx_ao_params (include/rtx_ao.h)"""
    _fields_ = [("n_dirs", C.c_uint32), ("dirs_dev", C.c_void_p), ("radius", C.c_float)]


class RadianceParams(C.Structure):
    """rtx_radiance_params (include/rtx_radiance.h)"""
    _fields_ = [("n_dirs", C.c_uint32), ("dirs_dev", C.c_void_p), ("weights_dev", C.c_void_p), ("cosine", C.c_int32)]


def sphere_directions(n):
    """n directions (n even) as float32 (n, 3): the first n / 2 are the upper half of a Fibonacci spiral over the sphere --
    z = 1 - 2 (i + 0.5) / n, phi = (i + 0.5) pi (3 - sqrt 5), (r cos phi, r sin phi, z) with r = sqrt(1 - z^2), in float64 rounded to
    float32 --, the others their negatives: an antipodal set, of which every surface point has about n / 2 on the side of its normal
    (Scene.render_ao)."""
    n = int(n)
    if n < 2 or n % 2:
        raise ValueError("sphere_directions: n must be even and at least 2, got %d" % n)
    i = np.arange(n // 2, dtype=np.float64) + 0.5
    z = 1.0 - 2.0 * i / n
    phi = i * (np.pi * (3.0 - np.sqrt(5.0)))
    r = np.sqrt(1.0 - z * z)
    half = np.stack([r * np.cos(phi), r * np.sin(phi), z], 1).astype(np.float32)
    return np.concatenate([half, -half], 0)


def load():
    """Loads the native libraries (raises RtxError when they have not been built: run ./build.sh)."""
    global _rtx, _host
    if _rtx is not None:
        return _rtx, _host
    for p in (LIB_RTX, LIB_HOST):
        if not os.path.exists(p):
            raise RtxError("native library %s is missing -- build it with ./build.sh (hipcc, gfx950); "
                           "there is no CPU fallback" % p)
    try:
        # let torch's bundled HIP runtime (same SONAME libamdhip64.so.7) win if torch is going to be used
        import torch  # noqa: F401
    except Exception:
        pass
    rtx = C.CDLL(LIB_RTX, mode=C.RTLD_GLOBAL)
    host = C.CDLL(LIB_HOST, mode=C.RTLD_GLOBAL)
    rtx.rtx_last_error.restype = C.c_char_p
    vp, u32, i32 = C.c_void_p, C.c_uint32, C.c_int
    rtx.rtx_device_count.argtypes = [C.POINTER(C.c_int)]
    rtx.rtx_render_pass1.argtypes = [vp, u32, u32, vp, vp]
    rtx.rtx_sobel.argtypes = [vp, vp, u32, u32, vp, vp]
    rtx.rtx_render_ssaa.argtypes = [vp, vp, u32, u32, vp, vp]
    rtx.rtx_render_frame.argtypes = [vp, u32, u32, vp, vp, vp]
    rtx.rtx_render_ac.argtypes = [vp, vp, vp, vp]
    rtx.rtx_frame_status.argtypes = [vp, C.POINTER(C.c_uint32)]
    rtx.rtx_set_frame_mode.argtypes = [vp, C.c_int]
    rtx.rtx_set_knob.argtypes = [vp, C.c_char_p, C.c_double]
    rtx.rtx_cost_grid_read.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    rtx.rtx_mesh_flatten_probe.argtypes = [vp, C.POINTER(C.c_uint32), vp, vp, C.c_uint32, vp]
    rtx.rtx_source_p_probe.argtypes = [vp, u32, vp, C.c_double, i32, vp]
    rtx.rtx_frame_mode_probe.argtypes = [i32, i32, i32, u32, u32, i32, vp, vp, u32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    rtx.rtx_tile_list_probe.argtypes = [u32, u32, u32, u32, u32, i32, u32, u32, i32, vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    rtx.rtx_frame_mode.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_float)]
    rtx.rtx_quantize_bgr8.argtypes = [vp, vp, vp, vp]
    rtx.rtx_render_frame_host.argtypes = [vp, i32, vp]
    rtx.rtx_counters_enable.argtypes = [vp, i32]
    rtx.rtx_counters_reset.argtypes = [vp]
    rtx.rtx_counters_read.argtypes = [vp, C.POINTER(Counters)]
    rtx.rtx_last_kernel_ms.argtypes = [vp, i32, C.POINTER(C.c_float)]
    rtx.rtx_math_probe.argtypes = [i32, i32, u32, vp, vp, vp]
    rtx.rtx_cast_rays.argtypes = [vp, u32, vp, vp, vp]
    rtx.rtx_trace_rays.argtypes = [vp, u32, vp, vp, vp, vp]
    rtx.rtx_occluded_rays.argtypes = [vp, u32, vp, vp, vp, vp]
    rtx.rtx_render_aov.argtypes = [vp, u32, u32, C.POINTER(AovBuffers), vp]
    rtx.rtx_render_ao.argtypes = [vp, u32, u32, C.POINTER(AoParams), vp, vp, vp]
    rtx.rtx_surface_rays.argtypes = [vp, u32, vp, C.POINTER(SurfaceBuffers), vp]
    if hasattr(rtx, "rtx_light_rays"):      # (a library without it is reported by exported_symbols)
        rtx.rtx_light_rays.argtypes = [vp, u32, vp, C.POINTER(LightBuffers), vp]
    if hasattr(rtx, "rtx_scatter_rays"):      # (a library without them is reported by exported_symbols)
        rtx.rtx_scatter_rays.argtypes = [vp, u32, vp, C.POINTER(ScatterBuffers), vp]
        rtx.rtx_sky_rays.argtypes = [vp, u32, vp, vp, vp]
    if hasattr(rtx, "rtx_light_points"):      # (a library without them is reported by exported_symbols)
        rtx.rtx_light_points.argtypes = [vp, u32, vp, vp, C.POINTER(LightBuffers), vp]
        rtx.rtx_ao_points.argtypes = [vp, u32, vp, C.POINTER(AoParams), vp, vp, vp]
    if hasattr(rtx, "rtx_radiance_points"):      # (a library without it is reported by exported_symbols)
        rtx.rtx_radiance_points.argtypes = [vp, u32, vp, C.POINTER(RadianceParams), vp, vp, vp]
    if hasattr(rtx, "rtx_render_light"):      # (a library without it is reported by exported_symbols)
        rtx.rtx_render_light.argtypes = [vp, u32, u32, C.POINTER(FrameLightBuffers), vp]
    if hasattr(rtx, "rtx_render_views"):      # (a library without them is reported by exported_symbols)
        rtx.rtx_render_views.argtypes = [vp, u32, C.POINTER(ViewTarget), i32, vp]
        rtx.rtx_views_plan_probe.argtypes = [u32, vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        # (the last: a ViewTarget or a ViewAovTarget, whose size and camera fields lie alike; the function leaves the buffers alone)
        host.rah_view_target.argtypes = [vp, vp, vp, C.c_float, i32, i32, vp]
    if hasattr(rtx, "rtx_render_views_aov"):      # (a library without it is reported by exported_symbols)
        rtx.rtx_render_views_aov.argtypes = [vp, u32, C.POINTER(ViewAovTarget), vp]
    rtx.rtx_kernel_time_reset.argtypes = [vp]
    rtx.rtx_kernel_time_stats.argtypes = [vp, i32, C.POINTER(C.c_uint32), C.POINTER(C.c_double)]
    rtx.rtx_tile_cost_read.argtypes = [vp, vp, C.c_size_t]
    rtx.rtx_set_row_ownership.argtypes = [vp, u32, u32, u32, i32]
    rtx.rtx_bvh_build.argtypes = [vp, u32, vp, vp, C.c_int32, i32, C.POINTER(vp)]
    rtx.rtx_bvh_info.argtypes = [vp, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32), C.POINTER(C.c_float)]
    rtx.rtx_bvh_launches.argtypes = [vp, C.POINTER(u32), C.POINTER(C.c_int)]
    rtx.rtx_bvh_read.argtypes = [vp, vp, vp, vp, vp, vp]
    rtx.rtx_bvh_destroy.argtypes = [vp]
    rtx.rtx_bvh_destroy.restype = None
    rtx.rtx_scene_bytes.argtypes = [vp, C.POINTER(C.c_size_t)]
    rtx.rtx_vec_probe.argtypes = [i32, i32, u32, vp, vp, C.c_float, vp]
    rtx.rtx_comm_unique_id.argtypes = [vp]
    rtx.rtx_comm_create.argtypes = [vp, i32, i32, i32, C.POINTER(vp)]
    rtx.rtx_comm_info.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    rtx.rtx_comm_destroy.argtypes = [vp]
    rtx.rtx_comm_agree.argtypes = [vp, C.c_int, C.POINTER(C.c_int), vp]
    rtx.rtx_comm_destroy.restype = None
    rtx.rtx_gather.argtypes = [vp, vp, vp, C.c_size_t, i32, i32, vp]
    rtx.rtx_gather_plan.argtypes = [u32, u32, u32, C.c_size_t, i32, u32, vp, vp, vp, C.POINTER(u32)]
    host.rah_set_ac_build.argtypes = [i32, i32]
    host.rah_set_ac_build.restype = None
    host.rah_set_ac_build_device.argtypes = [i32]
    host.rah_set_ac_build_device.restype = None
    host.rah_bvh_build_info.argtypes = [vp, i32, C.POINTER(C.c_int), C.POINTER(C.c_float)]
    host.rah_last_error.restype = C.c_char_p
    host.rah_scene_load.restype = vp
    host.rah_scene_load.argtypes = [C.c_char_p, C.c_char_p, i32, i32]
    host.rah_scene_free.argtypes = [vp]
    host.rah_scene_dims.argtypes = [vp] + [C.POINTER(C.c_int)] * 4
    host.rah_scene_resize.argtypes = [vp, i32, i32]
    host.rah_scene_set_device.argtypes = [vp, i32]
    host.rah_set_flag.argtypes = [vp, C.c_char_p, i32]
    host.rah_flatten.restype = vp
    host.rah_flatten.argtypes = [vp]
    host.rah_flat_desc.restype = vp
    host.rah_flat_desc.argtypes = [vp]
    host.rah_flat_free.argtypes = [vp]
    host.rah_bvh_counts.argtypes = [vp, i32, vp]
    host.rah_scene_gpu.restype = vp
    host.rah_scene_gpu.argtypes = [vp]
    host.rah_render_host.argtypes = [vp, vp, i32]
    host.rah_save_bmp.argtypes = [vp, vp, C.c_char_p]
    host.rah_bvh_dump.argtypes = [vp, i32, vp, vp, vp, vp, vp]
    host.rah_tris.argtypes = [vp, i32, vp]
    host.rah_camera.argtypes = [vp, vp, vp, vp, vp]
    host.rah_scene_digest.argtypes = [vp, vp, i32]
    host.rah_view_flags.argtypes = [vp]
    if hasattr(host, "rah_max_ray_depth"):
        host.rah_max_ray_depth.argtypes = [vp]
    host.rah_load_bmp.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), vp, i32]
    host.rah_object_move.argtypes = [vp, i32] + [vp] * 5
    host.rah_object_type.argtypes = [vp, i32]
    host.rah_object_move_times.argtypes = [vp, vp]
    rtx.rtx_scene_set_object.argtypes = [vp, C.c_uint32, vp]
    rtx.rtx_scene_update_mesh.argtypes = [vp, C.c_uint32, vp, vp, vp, vp, vp, i32, vp]
    rtx.rtx_scene_mesh_read.argtypes = [vp, C.c_uint32] + [vp] * 6
    rtx.rtx_scene_mesh_flat_read.argtypes = [vp, C.c_uint32, vp, vp, vp, C.c_uint32, vp]
    rtx.rtx_scene_edit_times.argtypes = [vp, vp]
    rtx.rtx_kernel_variant.argtypes = [vp, C.POINTER(C.c_uint32)]
    rtx.rtx_ssaa_list_read.argtypes = [vp, vp, vp, C.c_size_t]
    rtx.rtx_live_device_memory.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    rtx.rtx_scene_set_lights.argtypes = [vp, C.c_uint32, vp]
    rtx.rtx_scene_lights_read.argtypes = [vp, C.POINTER(C.c_uint32), vp, C.c_uint32, C.POINTER(C.c_size_t), vp, C.c_size_t]
    rtx.rtx_scene_mesh_prune_copy_read.argtypes = [vp, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), vp, C.c_uint32]
    host.rah_light_type.argtypes = [vp, i32]
    host.rah_light_set.argtypes = [vp, i32] + [vp] * 8
    host.rah_light_add.argtypes = [vp, i32] + [vp] * 8
    host.rah_light_remove.argtypes = [vp, i32]
    rtx.rtx_scene_set_objects.argtypes = [vp, C.c_uint32, vp, C.c_uint32, vp, vp]
    rtx.rtx_scene_objects_read.argtypes = [vp, C.POINTER(C.c_uint32), vp, C.c_uint32, C.POINTER(C.c_uint32)]
    host.rah_object_add.argtypes = [vp, i32, i32, C.c_char_p] + [vp] * 4 + [C.c_char_p] + [vp] * 2 + [C.c_char_p] * 4
    host.rah_object_remove.argtypes = [vp, i32]
    if hasattr(rtx, "rtx_scene_deform_mesh"):      # (a library without them is reported by exported_symbols)
        rtx.rtx_scene_set_mesh_topology.argtypes = [vp, u32, C.POINTER(MeshTopology)]
        rtx.rtx_scene_deform_mesh.argtypes = [vp, u32, vp, u32, vp, u32, C.POINTER(MeshPose), vp, vp, vp]
        rtx.rtx_place_probe.argtypes = [i32, C.POINTER(MeshTopology), vp, vp, C.POINTER(MeshPose), vp, vp, vp]
    host.rah_mesh_counts.argtypes = [vp, i32, vp]
    host.rah_mesh_vertices.argtypes = [vp, i32, vp, vp]
    host.rah_mesh_topology.argtypes = [vp, i32, vp, vp, vp, vp]
    host.rah_mesh_set_vertices.argtypes = [vp, i32, vp, C.c_longlong, vp, C.c_longlong, i32, vp]
    host.rah_mesh_deform_times.argtypes = [vp, vp]
    host.rah_mesh_deform_times.restype = None
    host.rah_euler_matrix.argtypes = [vp, vp]
    host.rah_euler_matrix.restype = None
    host.rah_mesh_pose.argtypes = [vp, i32, vp, vp, vp, C.POINTER(C.c_float), C.POINTER(C.c_int)]
    if hasattr(rtx, "rtx_scene_set_map"):      # (a library without them is reported by exported_symbols)
        rtx.rtx_scene_set_map.argtypes = [vp, u32, C.c_int32, C.POINTER(RtxTexels), vp]
        rtx.rtx_scene_set_sky.argtypes = [vp, C.POINTER(RtxTexels), vp]
        rtx.rtx_scene_write_texels.argtypes = [vp, C.c_int32, u32, u32, u32, C.POINTER(RtxTexels), vp]
        rtx.rtx_scene_texture_info.argtypes = [vp, C.c_int32, u32, C.POINTER(u32), C.POINTER(u32), C.POINTER(vp)]
        host.rah_decode_texels.argtypes = [i32, vp, C.c_longlong, vp]
        host.rah_scene_has_gpu.argtypes = [vp]
        host.rah_mesh_set_map.argtypes = [vp, i32, i32, C.POINTER(RtxTexels), i32, vp]
        host.rah_scene_set_sky.argtypes = [vp, C.POINTER(RtxTexels), i32, vp]
        host.rah_write_texels.argtypes = [vp, i32, i32, u32, u32, C.POINTER(RtxTexels), i32, vp]
        host.rah_texture.argtypes = [vp, i32, i32, C.POINTER(C.c_int), C.POINTER(C.c_int), vp, i32, vp]
    if hasattr(rtx, "rtx_texel_points"):      # (a library without them is reported by exported_symbols)
        rtx.rtx_texel_points.argtypes = [vp, u32, u32, u32, C.POINTER(TexelBuffers), vp]
        rtx.rtx_dilate_texels.argtypes = [vp, u32, u32, u32, vp, vp, u32, vp]
    if hasattr(rtx, "rtx_project_points"):      # (a library without it is reported by exported_symbols)
        rtx.rtx_project_points.argtypes = [vp, u32, vp, u32, vp, i32, C.POINTER(ProjectBuffers), vp]
    _rtx, _host = rtx, host
    return rtx, host


def exported_symbols():
    """(declared, missing) C-ABI symbols of librtx_hip.so -- used by the CPU-side load test."""
    rtx, _ = load()
    missing = [s for s in RTX_SYMBOLS + RTX_EDIT_SYMBOLS + RTX_QUERY_SYMBOLS + RTX_AOV_SYMBOLS + RTX_AO_SYMBOLS + RTX_SURFACE_SYMBOLS + RTX_LIGHT_SYMBOLS + RTX_DEFORM_SYMBOLS + RTX_VIEWS_SYMBOLS + RTX_VIEWS_AOV_SYMBOLS + RTX_SCATTER_SYMBOLS + RTX_POINTS_SYMBOLS + RTX_RENDER_LIGHT_SYMBOLS + RTX_RADIANCE_SYMBOLS + RTX_TEXTURE_SYMBOLS + RTX_BAKE_SYMBOLS + RTX_PROJECT_SYMBOLS
               if not hasattr(rtx, s)]
    return list(RTX_SYMBOLS), missing


# rtx_kernel_variant's bits (include/rtx_debug.h RTX_VARIANT_*)
VARIANT_BITS = {"boxes": 1, "plain": 2, "analytic": 4, "stats": 8, "cull": 16}


def _check(rc, what):
    if rc != 0:
        raise RtxError("%s failed (%d): %s" % (what, rc, _rtx.rtx_last_error().decode(errors="replace")))


def device_count():
    rtx, _ = load()
    n = C.c_int(0)
    _check(rtx.rtx_device_count(C.byref(n)), "rtx_device_count")
    return n.value


def live_device_memory():
    """(allocations, bytes) of device memory the native library holds in this process (rtx_live_device_memory)."""
    rtx, _ = load()
    n, b = C.c_size_t(0), C.c_size_t(0)
    _check(rtx.rtx_live_device_memory(C.byref(n), C.byref(b)), "rtx_live_device_memory")
    return n.value, b.value


def decode_texels(kind, rgb8):
    """The loaders' texel arithmetic on the host (rah_decode_texels): uint8 (..., 3) texels, R G B as the BMP loader returns them, into float32
    (..., 3) -- (...) for "specular" -- as a map of `kind` ("diffuse", "normal", "specular", "sky") stores them: byte / 256; for a normal map
    Vec3f(c.x*2-1, -(c.y*2-1), c.z).normalize(); for a specular map (c.x+c.y+c.z)/3."""
    _, host = load()
    if kind not in TEXTURE_KINDS:
        raise ValueError("decode_texels: unknown kind %r (%s)" % (kind, ", ".join(TEXTURE_KINDS)))
    a = np.asarray(rgb8)
    if a.dtype != np.uint8 or a.ndim < 1 or a.shape[-1] != 3:
        raise ValueError("decode_texels: rgb8 must be uint8 (..., 3), got %s %s" % (a.dtype, a.shape))
    a = np.ascontiguousarray(a)
    out = np.zeros(a.shape[:-1] if kind == "specular" else a.shape, np.float32)
    if host.rah_decode_texels(TEXTURE_KINDS[kind], _np_ptr(a), a.size // 3, _np_ptr(out)) != 0:
        raise RtxError("decode_texels: %s" % kind)
    return out


def _np_ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _ptr(t):
    """A tensor's device address as a C argument; None is NULL."""
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _check_tensor(who, name, t, dtype, shape, device=None):
    """Argument `name` of the wrapper `who` (the prefix of every message) is a contiguous torch tensor of `dtype` and `shape` -- a tuple whose
    entries are sizes, or names such as "n" for a size that is free -- on cuda:`device` (None: the wrapper checks the device itself)."""
    import torch
    if not isinstance(t, torch.Tensor):
        raise ValueError("%s: %s must be a torch tensor, got %s" % (who, name, type(t).__name__))
    if t.dtype != dtype:
        raise ValueError("%s: %s must be %s, got %s" % (who, name, str(dtype).replace("torch.", ""), t.dtype))
    if t.dim() != len(shape) or any(want != have for want, have in zip(shape, t.shape) if not isinstance(want, str)):
        raise ValueError("%s: %s must have shape %s, got %s" % (who, name, str(shape).replace("'", ""), tuple(t.shape)))
    if not t.is_contiguous():
        raise ValueError("%s: %s must be contiguous" % (who, name))
    if device is not None:
        _check_device(who, name, t, device)


def _check_device(who, name, t, device):
    """... and is on cuda:`device` (_check_tensor's last check, for a wrapper that makes it after the shapes of all its tensors)."""
    import torch
    if t.device.type != "cuda" or (t.device.index if t.device.index is not None else torch.cuda.current_device()) != device:
        raise ValueError("%s: %s must be on cuda:%d, the scene's device, got %s" % (who, name, device, t.device))


def _check_rays(who, rays, device, noun="rays"):
    """The rays of the wrapper `who`: a contiguous float32 tensor (n, 6) on cuda:`device` of at most 0xFFFFFFC0 rays.  Returns n.
    noun "points": the batch is {P xyz, N xyz} in the same layout (light_points, ao_points)."""
    import torch
    _check_tensor(who, noun, rays, torch.float32, ("n", 6), device)
    if rays.shape[0] > 0xFFFFFFC0:
        raise ValueError("%s: at most %d %s per call, got %d" % (who, 0xFFFFFFC0, noun, rays.shape[0]))
    return rays.shape[0]


def _query_stream(stream, device, inputs):
    """(alloc_on, pointer) of the stream a query call runs on: `stream`, or torch's current stream of `device` for None.  With a
    torch.cuda.Stream, alloc_on is that stream -- the outputs are allocated on it and the tensors of `inputs` (None entries skipped) are
    recorded on it while it uses them (torch's caching allocator); a raw hipStream_t handle is used as given (alloc_on None), so the
    caller keeps the tensors alive and unreused until it has finished with them."""
    import torch
    alloc_on = stream if isinstance(stream, torch.cuda.Stream) else None
    if alloc_on is not None:
        for t in inputs:
            if t is not None:
                t.record_stream(alloc_on)
    return alloc_on, C.c_void_p(torch.cuda.current_stream(device).cuda_stream) if stream is None else Scene._stream_ptr(stream)


def _query_outputs(channels, n, device, alloc_on):
    """The outputs of a query over n rays or points from its channel table, rows (name, on, tail shape, dtype): a dict of the channels
    that are on, new tensors (n,) + tail on `device` allocated on the query stream (_query_stream's alloc_on), and the pointers of all
    channels in the table's order -- None for a channel that is off or empty (a per-light channel of a scene without lights has no
    pointer for the library)."""
    import torch
    with torch.cuda.stream(alloc_on):
        out = {name: torch.empty((n,) + tail, dtype=dtype, device=device) for name, on, tail, dtype in channels if on}
    return out, [out[name].data_ptr() if name in out and out[name].numel() else None for name, _, _, _ in channels]


def _frame_tensors(who, outputs, device, stream, inputs=()):
    """The tensors of the frame call `who`, rows (name, tensor, dtype, shape): `outputs`, of which the caller gives any subset but at
    least one, and `inputs`, which are all required.  Each is checked (_check_tensor, the inputs first) and, with a torch.cuda.Stream,
    recorded on it.  Returns (the stream's pointer, the outputs' pointers in order: None for one that is not given or is empty -- a
    per-light tensor of a scene without lights has no pointer for the library)."""
    if all(t is None for _, t, _, _ in outputs):
        raise ValueError("%s: nothing to compute (at least one buffer is needed)" % who)
    for name, t, dtype, shape in inputs:
        _check_tensor(who, name, t, dtype, shape, device)
    for name, t, dtype, shape in outputs:
        if t is not None:
            _check_tensor(who, name, t, dtype, shape, device)
    _, st = _query_stream(stream, device, [t for _, t, _, _ in tuple(inputs) + tuple(outputs)])
    return st, [t.data_ptr() if t is not None and t.numel() else None for _, t, _, _ in outputs]


def set_ac_build(mode, device=0):
    """Where the host loader builds acceleration structures from now on: "host", "device" (rtx_bvh_build) or
    "auto" (the device when one is visible).  Both give the same structure bit for bit."""
    _, host = load()
    host.rah_set_ac_build({"auto": -1, "host": 0, "device": 1}[mode], device)


def bvh_build(tri_pos, root_lo, root_hi, ac_penalty=1, device=0):
    """rtx_bvh_build + rtx_bvh_read: the reference's acceleration structure (objects.cpp:470-526, 633-763) built on
    the GPU.  Returns the dump layout of Scene.bvh() plus `build_ms` (HIP events around the build)."""
    rtx, _ = load()
    pos = np.ascontiguousarray(tri_pos, np.float32).reshape(-1, 9)
    lo = np.ascontiguousarray(root_lo, np.float32); hi = np.ascontiguousarray(root_hi, np.float32)
    b = C.c_void_p()
    _check(rtx.rtx_bvh_build(_np_ptr(pos), pos.shape[0], _np_ptr(lo), _np_ptr(hi), ac_penalty, device, C.byref(b)), "rtx_bvh_build")
    try:
        nn, nr, md, ms = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_float()
        _check(rtx.rtx_bvh_info(b, C.byref(nn), C.byref(nr), C.byref(md), C.byref(ms)), "rtx_bvh_info")
        d = dict(bounds=np.zeros((nn.value, 6), np.float32), skip=np.zeros(nn.value, np.int32),
                 leaf_begin=np.zeros(nn.value, np.int32), leaf_count=np.zeros(nn.value, np.int32),
                 refs=np.zeros(nr.value, np.uint32))
        _check(rtx.rtx_bvh_read(b, _np_ptr(d["bounds"]), _np_ptr(d["skip"]), _np_ptr(d["leaf_begin"]), _np_ptr(d["leaf_count"]),
                                _np_ptr(d["refs"])), "rtx_bvh_read")
        d.update(n_nodes=nn.value, n_refs=nr.value, max_depth=md.value, build_ms=ms.value)
        ln, q = C.c_uint32(), C.c_int()
        _check(rtx.rtx_bvh_launches(b, C.byref(ln), C.byref(q)), "rtx_bvh_launches")
        d.update(launches=ln.value, queued=bool(q.value))
        return d
    finally:
        rtx.rtx_bvh_destroy(b)


def bvh_build_mode(mode):
    """0: rtx_bvh_build in its persistent launches (default); 1: level by level (the fallback of the former; tests compare the two)."""
    rtx, _ = load()
    _check(rtx.rtx_bvh_build_mode(int(mode)), "rtx_bvh_build_mode")


def bvh_build_host(tri_pos, root_lo, root_hi, ac_penalty=1):
    """The HOST builder (rendering_amd/host/src/objects.cpp) on a bare triangle array, in the dump layout of Scene.bvh(); no GPU."""
    _, host = load()
    pos = np.ascontiguousarray(tri_pos, np.float32).reshape(-1, 9)
    lo = np.ascontiguousarray(root_lo, np.float32); hi = np.ascontiguousarray(root_hi, np.float32)
    cnt = np.zeros(4, np.int64)
    host.rah_bvh_from_tris.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p] + [C.c_void_p] * 5
    if host.rah_bvh_from_tris(_np_ptr(pos), pos.shape[0], _np_ptr(lo), _np_ptr(hi), ac_penalty, _np_ptr(cnt), None, None, None, None, None) != 0:
        raise RtxError("rah_bvh_from_tris: %s" % host.rah_last_error().decode(errors="replace"))
    nn, nl, nr, md = [int(x) for x in cnt]
    d = dict(bounds=np.zeros((nn, 6), np.float32), skip=np.zeros(nn, np.int32), leaf_begin=np.zeros(nn, np.int32), leaf_count=np.zeros(nn, np.int32),
             refs=np.zeros(max(nr, 1), np.uint32)[:nr])
    host.rah_bvh_from_tris(_np_ptr(pos), pos.shape[0], _np_ptr(lo), _np_ptr(hi), ac_penalty, _np_ptr(cnt), _np_ptr(d["bounds"]), _np_ptr(d["skip"]),
                           _np_ptr(d["leaf_begin"]), _np_ptr(d["leaf_count"]), _np_ptr(d["refs"]))
    d.update(n_nodes=nn, n_leaves=nl, n_refs=nr, max_depth=md)
    return d


def gather_plan(height, band_height, n_parts, row_bytes, bottom_up=False):
    """rtx_gather_plan: [(owner, byte offset, bytes), ...] -- the transfers rtx_gather executes (host only)."""
    rtx, _ = load()
    n = C.c_uint32(0)
    cap = (height + band_height - 1) // band_height
    owner = np.zeros(cap, np.uint32); off = np.zeros(cap, np.uint64); ln = np.zeros(cap, np.uint64)
    _check(rtx.rtx_gather_plan(height, band_height, n_parts, row_bytes, int(bottom_up), cap, _np_ptr(owner), _np_ptr(off), _np_ptr(ln), C.byref(n)),
           "rtx_gather_plan")
    return [(int(owner[i]), int(off[i]), int(ln[i])) for i in range(n.value)]


class Comm:
    """RCCL communicator behind the C ABI (rtx_comm_*): one rank per GPU.  `exchange(id_bytes_or_None)` must hand rank 0's
    128-byte id to every rank (e.g. a torch.distributed / MPI broadcast, a pipe): it receives the id on rank 0 and None
    elsewhere, and returns the id on every rank."""

    def __init__(self, n_ranks, rank, device, exchange):
        self.rtx, _ = load()
        buf = (C.c_ubyte * 128)()
        if rank == 0:
            _check(self.rtx.rtx_comm_unique_id(buf), "rtx_comm_unique_id")
        raw = exchange(bytes(buf) if rank == 0 else None)
        if len(raw) != 128:
            raise RtxError("communicator id must be 128 bytes")
        self.h = C.c_void_p()
        _check(self.rtx.rtx_comm_create(raw, n_ranks, rank, device, C.byref(self.h)), "rtx_comm_create")
        self.n_ranks, self.rank = n_ranks, rank

    def gather(self, scene, img, bottom_up=False, root=0, stream=None):
        """rtx_gather: every rank's owned rows of the device tensor img (H, ...) end up in rank `root`'s img."""
        row_bytes = img[0].numel() * img.element_size()
        _check(self.rtx.rtx_gather(scene.gpu(), self.h, C.c_void_p(img.data_ptr()), row_bytes, int(bottom_up), root,
                                   Scene._stream_ptr(stream)), "rtx_gather")

    def info(self):
        """rtx_comm_info: (n_ranks, rank) as the RCCL communicator itself reports them (ncclCommCount / ncclCommUserRank)."""
        n, r = C.c_int(0), C.c_int(0)
        _check(self.rtx.rtx_comm_info(self.h, C.byref(n), C.byref(r)), "rtx_comm_info")
        return n.value, r.value

    def agree(self, ok, stream=None):
        """rtx_comm_agree: True iff every rank passed ok=True (called before gather, so that a failed rank does not leave the others waiting)."""
        out = C.c_int(0)
        _check(self.rtx.rtx_comm_agree(self.h, int(bool(ok)), C.byref(out), Scene._stream_ptr(stream)), "rtx_comm_agree")
        return bool(out.value)

    def close(self):
        if self.h:
            self.rtx.rtx_comm_destroy(self.h)
            self.h = C.c_void_p()


class RtxLight(C.Structure):
    """rtx_light (include/rtx.h)"""
    _fields_ = [("type", C.c_int32), ("color", C.c_float * 3), ("intensity", C.c_float), ("dir", C.c_float * 3), ("pos", C.c_float * 3),
                ("n_points", C.c_uint32), ("points", C.c_void_p)]


# the keys of a [light] block per type, in rah_light_set's argument order, and the values each takes
LIGHT_TYPES = {"distant": 1, "point": 2, "area": 3}
LIGHT_KEYS = {"distant": ("direction", "color", "intensity"), "point": ("position", "color", "intensity"),
              "area": ("pos", "i", "j", "samples", "color", "intensity")}
_LIGHT_ARGS = ("color", "intensity", "direction", "position", "pos", "i", "j", "samples")


class RtxObject(C.Structure):
    """rtx_object (include/rtx.h)"""
    _fields_ = [("type", C.c_int32), ("material", C.c_int32), ("pos", C.c_float * 3), ("color", C.c_float * 3), ("ior", C.c_float),
                ("ambient", C.c_float), ("diffuse", C.c_float), ("specular", C.c_float), ("n_specular", C.c_float), ("radius2", C.c_float),
                ("normal", C.c_float * 3), ("mesh", C.c_int32)]


# the keys of an [object] block per type, in the order they are applied, and the values a material= line takes after its name
OBJECT_TYPES = {"sphere": 1, "plane": 2, "mesh": 3}
OBJECT_KEYS = {"sphere": ("pos", "color", "material", "radius"), "plane": ("pos", "color", "material", "normal"),
               "mesh": ("pos", "size", "rot", "color", "material", "name", "diffuse_map", "normal_map", "specular_map")}
_OBJECT_ARGS = ("pos", "size", "rot", "color", "material", "radius", "normal", "name", "diffuse_map", "normal_map", "specular_map")
_OBJECT_TEXT = ("material", "name", "diffuse_map", "normal_map", "specular_map")
MATERIAL_VALUES = {"diffuse": 0, "reflective": 0, "transparent": 1, "phong": 4}


class _RtxMesh(C.Structure):
    _fields_ = [("n_nodes", C.c_uint32), ("n_refs", C.c_uint32), ("n_tris", C.c_uint32), ("node_bounds", C.c_void_p), ("node_skip", C.c_void_p),
                ("leaf_begin", C.c_void_p), ("leaf_count", C.c_void_p), ("refs", C.c_void_p), ("tri_pos", C.c_void_p), ("tri_nrm", C.c_void_p),
                ("tri_uv", C.c_void_p), ("tri_tb", C.c_void_p), ("diffuse_w", C.c_uint32), ("diffuse_h", C.c_uint32), ("diffuse_map", C.c_void_p),
                ("normal_w", C.c_uint32), ("normal_h", C.c_uint32), ("normal_map", C.c_void_p), ("specular_w", C.c_uint32), ("specular_h", C.c_uint32),
                ("specular_map", C.c_void_p)]


class RtxView(C.Structure):
    """rtx_view (include/rtx.h)"""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("bias", C.c_float), ("max_ray_depth", C.c_int32), ("background", C.c_float * 3),
                ("flags", C.c_uint32), ("cam_pos", C.c_float * 3), ("cam_matrix", C.c_float * 16), ("scale", C.c_float), ("aspect", C.c_float)]


class RtxSceneDesc(C.Structure):
    """rtx_scene_desc (include/rtx.h): what rah_flat_desc points to"""
    _fields_ = [("view", RtxView), ("n_objects", C.c_uint32), ("objects", C.POINTER(RtxObject)), ("n_meshes", C.c_uint32),
                ("meshes", C.POINTER(_RtxMesh)), ("n_lights", C.c_uint32), ("lights", C.POINTER(RtxLight)), ("sky_w", C.c_uint32), ("sky_h", C.c_uint32),
                ("sky", C.c_void_p * 6)]


class RtxMeshBuild(C.Structure):
    """rtx_mesh_build (include/rtx_scene_edit.h)"""
    _fields_ = [("tri_pos_dev", C.c_void_p), ("tri_nrm_dev", C.c_void_p), ("tri_tb_dev", C.c_void_p), ("root_lo", C.c_float * 3),
                ("root_hi", C.c_float * 3), ("ac_penalty", C.c_int32)]


class RtxMeshSource(C.Structure):
    """rtx_mesh_source (include/rtx_scene_edit.h)"""
    _fields_ = [("keep", C.c_int32), ("mesh", C.POINTER(_RtxMesh)), ("build", C.POINTER(RtxMeshBuild))]


def mesh_flatten_probe(bvh):
    """Host only: the wide nodes and prune blocks rtx_scene_create derives from a mesh (rtx_mesh_flatten_probe).  bvh = Scene.bvh(obj).
    Returns (wide [n, S, 8] float32 -- link / first as bit patterns in [..., 6:8] --, box records [n, S, 8], plane records [n, S, 8], root record [8]);
    S = rtx_wide_node_slots()."""
    rtx, _ = load()
    bounds = np.ascontiguousarray(bvh["bounds"], np.float32); skip = np.ascontiguousarray(bvh["skip"], np.int32)
    lb = np.ascontiguousarray(bvh["leaf_begin"], np.int32); lc = np.ascontiguousarray(bvh["leaf_count"], np.int32)
    refs = np.ascontiguousarray(bvh["refs"], np.uint32); pos = np.ascontiguousarray(bvh["tris"][:, 0:9], np.float32)
    m = _RtxMesh()
    m.n_nodes, m.n_refs, m.n_tris = len(skip), len(refs), len(pos)
    m.node_bounds, m.node_skip, m.leaf_begin, m.leaf_count = bounds.ctypes.data, skip.ctypes.data, lb.ctypes.data, lc.ctypes.data
    m.refs, m.tri_pos = refs.ctypes.data, pos.ctypes.data
    n = C.c_uint32(0)
    root = np.zeros(8, np.float32)
    _check(rtx.rtx_mesh_flatten_probe(C.byref(m), C.byref(n), None, None, 0, _np_ptr(root)), "rtx_mesh_flatten_probe")
    S = int(rtx.rtx_wide_node_slots())
    wide = np.zeros((n.value, S, 8), np.float32); prune = np.zeros((n.value, 2 * S, 8), np.float32)
    _check(rtx.rtx_mesh_flatten_probe(C.byref(m), C.byref(n), _np_ptr(wide), _np_ptr(prune), n.value, _np_ptr(root)), "rtx_mesh_flatten_probe")
    return wide, prune[:, 0:S], prune[:, S:2 * S], root


def source_p_probe(v0, e1, e2, S, sigma, cam):
    """Host only: P of the source copies of the prune records for triangles (v0, e1, e2: [n, 3] float32), source point S, radius sigma;
    cam: the rays start at S (rtx_source_p_probe; csrc/rtx_source.hip)."""
    rtx, _ = load()
    t = np.ascontiguousarray(np.concatenate([v0, e1, e2], 1), np.float32)
    S = np.ascontiguousarray(S, np.float64)
    out = np.zeros(len(t), np.float32)
    _check(rtx.rtx_source_p_probe(_np_ptr(t), len(t), _np_ptr(S), float(sigma), 1 if cam else 0, _np_ptr(out)), "rtx_source_p_probe")
    return out


def frame_mode_probe(forced, has_list, fused_gave_up, listed, rule_tiles, warm, frame_samples, frame_ms, frames_seen):
    """Host only: (mode, reprobe, probing) of rtx_render_frame's one-launch-or-three policy (rtx_frame_mode_probe; csrc/rtx_frame_plan.h)."""
    rtx, _ = load()
    n = np.ascontiguousarray(frame_samples, np.uint32); ms = np.ascontiguousarray(frame_ms, np.float32)
    assert n.shape == (2,) and ms.shape == (2,)
    mode, reprobe, probing = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    _check(rtx.rtx_frame_mode_probe(int(forced), int(has_list), int(fused_gave_up), int(listed), int(rule_tiles), int(warm), _np_ptr(n), _np_ptr(ms),
                                    int(frames_seen), C.byref(mode), C.byref(reprobe), C.byref(probing)), "rtx_frame_mode_probe")
    return mode.value, bool(reprobe.value), bool(probing.value)


def tile_list_probe(width, height, ownership, rows, strips, rect):
    """Host only: the words of the pass-1 tile list (header of 16, then the eight queues) of the rows `rows` of a width x height view under
    ownership = (band_height, n_parts, part, halo), with the mesh tile rectangle rect = (tx0, tx1, ty0, ty1) (rtx_tile_list_probe)."""
    rtx, _ = load()
    r = np.ascontiguousarray(rect, np.uint32)
    assert r.shape == (4,)
    args = [int(width), int(height)] + [int(x) for x in ownership] + [int(rows[0]), int(rows[1]), 1 if strips else 0, _np_ptr(r)]
    need = C.c_size_t(0)
    _check(rtx.rtx_tile_list_probe(*args, None, 0, C.byref(need)), "rtx_tile_list_probe")
    out = np.zeros(need.value, np.uint32)
    _check(rtx.rtx_tile_list_probe(*args, _np_ptr(out), out.size, C.byref(need)), "rtx_tile_list_probe")
    return out


def math_probe(op, x, y=None, device=0):
    """Evaluates the device math the parity contract depends on (see rtx_math_probe in include/rtx.h)."""
    rtx, _ = load()
    x = np.ascontiguousarray(x, np.float32)
    out = np.zeros_like(x)
    yp = None
    if y is not None:
        y = np.ascontiguousarray(np.broadcast_to(np.asarray(y, np.float32), x.shape))
        yp = _np_ptr(y)
    _check(rtx.rtx_math_probe(device, op, x.size, _np_ptr(x), yp, _np_ptr(out)), "rtx_math_probe")
    return out


def vec_probe(op, a, b=None, ior=1.0, device=0):
    """rtx_vec_probe: reflect / refract / fresnel / normalize on the device (n x 3 arrays)."""
    rtx, _ = load()
    a = np.ascontiguousarray(a, np.float32).reshape(-1, 3)
    out = np.zeros_like(a)
    bp = None
    if b is not None:
        b = np.ascontiguousarray(b, np.float32).reshape(-1, 3)
        bp = _np_ptr(b)
    _check(rtx.rtx_vec_probe(device, op, a.shape[0], _np_ptr(a), bp, ior, _np_ptr(out)), "rtx_vec_probe")
    return out


def euler_matrix(rot):
    """The rotation matrix the loader places a mesh with (Matrix44f::fromEulerDegrees of `rot` in degrees, host libm), float32 (4, 4)."""
    _, host = load()
    r = np.ascontiguousarray(np.asarray(rot, np.float32).reshape(3))
    m = np.zeros((4, 4), np.float32)
    host.rah_euler_matrix(_np_ptr(r), _np_ptr(m))
    return m


def place_probe(topology, stored_normals, vertices, normals, pose, device=-1):
    """The placement and triangle assembly of Scene.set_vertices on bare arrays (rtx_place_probe): no scene, no tree.  topology: the dict of
    Scene.mesh_topology; stored_normals: float32 (n_nrm, 3), used when `normals` is None; vertices float32 (n_pos, 3); normals raw, float32
    (n_nrm, 3), or None; pose: the dict of Scene.mesh_pose.  device >= 0: the three kernels on that device; device < 0: the same functions on
    the CPU.  Returns dict(pos (n, 9), nrm (n, 9), tb (n, 6), obj_lo, obj_hi, root_lo, root_hi, bad_input, bad_placed)."""
    rtx, _ = load()
    f32 = lambda a, cols: np.ascontiguousarray(np.asarray(a, np.float32).reshape(-1, cols))
    cp = np.ascontiguousarray(topology["corner_pos"], np.uint32).reshape(-1, 3)
    cn = np.ascontiguousarray(topology["corner_nrm"], np.int32).reshape(-1, 3)
    cu = np.ascontiguousarray(topology["corner_uv"], np.int32).reshape(-1, 3)
    uv, sn, P = f32(topology["uv"], 2), f32(stored_normals, 3), f32(vertices, 3)
    N = f32(normals, 3) if normals is not None else None
    if N is not None and N.shape != sn.shape:
        raise ValueError("place_probe: normals must have the stored normals' shape %s, got %s" % (sn.shape, N.shape))
    nt = cp.shape[0]
    t = MeshTopology(nt, P.shape[0], sn.shape[0], uv.shape[0], int(topology["placed_pos"]), int(topology["placed_nrm"]),
                     cp.ctypes.data, cn.ctypes.data, cu.ctypes.data, uv.ctypes.data if uv.size else None, sn.ctypes.data if sn.size else None)
    ps = MeshPose()
    ps.pos[:] = [float(x) for x in np.asarray(pose["pos"], np.float32)]
    ps.size[:] = [float(x) for x in np.asarray(pose["size"], np.float32)]
    ps.rot_matrix[:] = [float(x) for x in euler_matrix(pose["rot"]).reshape(-1)]
    ps.bias = float(pose["bias"]); ps.ac_penalty = int(pose["ac_penalty"])
    tri = np.zeros(max(nt, 1) * 24, np.float32)
    lo_hi = np.zeros(12, np.float32)
    flags = np.zeros(2, np.uint32)
    _check(rtx.rtx_place_probe(device, C.byref(t), _np_ptr(P), _np_ptr(N) if N is not None else None, C.byref(ps), _np_ptr(tri), _np_ptr(lo_hi), _np_ptr(flags)),
           "rtx_place_probe")
    return dict(pos=tri[:nt * 9].reshape(nt, 9).copy(), nrm=tri[nt * 9:nt * 18].reshape(nt, 9).copy(), tb=tri[nt * 18:nt * 24].reshape(nt, 6).copy(),
                obj_lo=lo_hi[0:3].copy(), obj_hi=lo_hi[3:6].copy(), root_lo=lo_hi[6:9].copy(), root_hi=lo_hi[9:12].copy(),
                bad_input=bool(flags[0]), bad_placed=bool(flags[1]))


class Scene:
    """Host Scene (loaded by the C++ loader) + its uploaded GPU twin.

    Mirrors the reference's Scene surface for the hot path: render() = launchWorkers + launchSSAA
    (scene.cpp:595-606).  `width`/`height` > 0 override the scene file's resolution.
    """

    def __init__(self, scene_path, width=-1, height=-1, device=0, cwd=ROOT):
        self.rtx, self.host = load()
        self.host.rah_set_ac_build_device(device)      # a rank builds its structures on the GPU it renders on
        self.h = C.c_void_p(self.host.rah_scene_load(cwd.encode(), scene_path.encode(), width, height))
        if not self.h:
            raise RtxError("could not load scene %s: %s" % (scene_path, self.host.rah_last_error().decode(errors="replace")))
        self.device = device
        self._cwd = cwd
        self.host.rah_scene_set_device(self.h, device)
        self._dims()
        self._gpu = None

    def _dims(self):
        w, h, no, nl = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        self.host.rah_scene_dims(self.h, C.byref(w), C.byref(h), C.byref(no), C.byref(nl))
        self.width, self.height, self.n_objects, self.n_lights = w.value, h.value, no.value, nl.value

    def close(self):
        if self.h:
            self.host.rah_scene_free(self.h)
            self.h = None
            self._gpu = None

    def resize(self, width, height):
        self.host.rah_scene_resize(self.h, width, height)
        self._dims()

    def camera_pose(self):
        """(position, rotation in degrees) of the camera (Camera::pos / Camera::rot)."""
        pos, rot = np.zeros(3, np.float32), np.zeros(3, np.float32)
        self.host.rah_camera_get.argtypes = [C.c_void_p] * 3
        self.host.rah_camera_get(self.h, _np_ptr(pos), _np_ptr(rot))
        return pos, rot

    def set_camera(self, pos, rot):
        """Moves the camera; the next render re-applies the view (rtx_scene_set_view: queued on the device, the host does not wait)."""
        pos = np.ascontiguousarray(pos, np.float32); rot = np.ascontiguousarray(rot, np.float32)
        self.host.rah_camera_set.argtypes = [C.c_void_p] * 3
        self.host.rah_camera_set(self.h, _np_ptr(pos), _np_ptr(rot))

    def set_flag(self, name, value):
        """Pins one of the switches the render reads on this scene only: useBackfaceCulling, useSkybox, collectStatistics,
        showNormals (the normals view) or showAC (the heat map of Scene::render; see render_ac)."""
        self.host.rah_set_flag(self.h, name.encode(), int(value))

    # ---- host-side structures (no GPU needed) -------------------------------------------------
    def camera(self):
        scale, aspect = C.c_float(), C.c_float()
        m = np.zeros(16, np.float32)
        pos = np.zeros(3, np.float32)
        self.host.rah_camera(self.h, C.byref(scale), C.byref(aspect), _np_ptr(m), _np_ptr(pos))
        return np.float32(scale.value), np.float32(aspect.value), m, pos

    def view_flags(self):
        """rtx_view::flags this scene uploads (bit 0 back-face culling, bit 1 skybox, bit 2 the showNormals view)."""
        return self.host.rah_view_flags(self.h)

    def digest(self):
        """Numeric fields of all objects and lights as uploaded (loader tests)."""
        out = np.zeros(4096, np.float32)
        n = self.host.rah_scene_digest(self.h, _np_ptr(out), out.size)
        return out[:n].copy()

    def bvh(self, obj_idx):
        cnt = np.zeros(5, np.int64)
        if self.host.rah_bvh_counts(self.h, obj_idx, _np_ptr(cnt)) != 0:
            return None
        nn, nl, nr, md, nt = [int(x) for x in cnt]
        d = dict(bounds=np.zeros((nn, 6), np.float32), skip=np.zeros(nn, np.int32),
                 leaf_begin=np.zeros(nn, np.int32), leaf_count=np.zeros(nn, np.int32),
                 refs=np.zeros(nr, np.uint32))
        self.host.rah_bvh_dump(self.h, obj_idx, _np_ptr(d["bounds"]), _np_ptr(d["skip"]), _np_ptr(d["leaf_begin"]),
                               _np_ptr(d["leaf_count"]), _np_ptr(d["refs"]))
        tris = np.zeros((nt, 30), np.float32)
        self.host.rah_tris(self.h, obj_idx, _np_ptr(tris))
        d.update(tris=tris, n_nodes=nn, n_leaves=nl, n_refs=nr, max_depth=md, n_tris=nt)
        on, ms = C.c_int(0), C.c_float(0)
        self.host.rah_bvh_build_info(self.h, obj_idx, C.byref(on), C.byref(ms))
        d.update(built_on_device=bool(on.value), build_ms=ms.value)
        return d

    def bvh_build_info(self, obj_idx):
        """(built on the device?, build ms) of object obj_idx's acceleration structure; None for objects without one."""
        on, ms = C.c_int(0), C.c_float(-1)
        if self.host.rah_bvh_build_info(self.h, obj_idx, C.byref(on), C.byref(ms)) != 0:
            return None
        return bool(on.value), ms.value

    def move_object(self, index, pos=None, rot=None, size=None, radius=None, normal=None):
        """Places object `index` (scene-file order) as its [object] block would with these values; None keeps a value.  A mesh takes
        pos / rot / size (its vertices are placed again by the loader's code), a sphere pos / radius, a plane pos / normal; any other key
        raises ValueError.  With a live GPU scene the device rebuilds the mesh's structure (rtx_scene_update_mesh): renders queued before
        the move see the old scene, later ones the new one.  Afterwards bvh(), digest() and the frames describe the moved scene."""
        keys = {"mesh": ("pos", "rot", "size"), "sphere": ("pos", "radius"), "plane": ("pos", "normal")}
        given = {k: v for k, v in (("pos", pos), ("rot", rot), ("size", size), ("radius", radius), ("normal", normal)) if v is not None}
        if not 0 <= index < self.n_objects:
            raise ValueError("move_object: object index %d out of range (%d objects)" % (index, self.n_objects))
        kind = {1: "sphere", 2: "plane", 3: "mesh"}.get(self.host.rah_object_type(self.h, index))
        bad = [k for k in given if kind is None or k not in keys[kind]]
        if bad:
            raise ValueError("move_object: a %s has no key %s (it takes %s)" % (kind, ", ".join(bad), ", ".join(keys.get(kind, ()))))
        arrs = {}
        for k, v in given.items():
            a = np.ascontiguousarray(np.asarray(v, np.float32).reshape(-1))
            if a.size != (1 if k == "radius" else 3):
                raise ValueError("move_object: %s takes %d values, got %d" % (k, 1 if k == "radius" else 3, a.size))
            arrs[k] = a
        ptr = lambda k: _np_ptr(arrs[k]) if k in arrs else None
        if self.host.rah_object_move(self.h, index, ptr("pos"), ptr("rot"), ptr("size"), ptr("radius"), ptr("normal")) != 0:
            raise RtxError("move_object: %s" % self.host.rah_last_error().decode(errors="replace"))

    def light_type(self, index):
        """"distant", "point" or "area": the type of light `index` (scene-file order)."""
        if not 0 <= index < self.n_lights:
            raise ValueError("light_type: light index %d out of range (%d lights)" % (index, self.n_lights))
        return {v: k for k, v in LIGHT_TYPES.items()}[self.host.rah_light_type(self.h, index)]

    @staticmethod
    def _light_args(who, kind, keys):
        """The arguments of rah_light_set / rah_light_add for `keys` of a light of type `kind` (ValueError: a key the type does not have, a
        wrong number of values); the arrays are returned with them to keep them alive."""
        bad = [k for k in keys if k not in LIGHT_KEYS[kind]]
        if bad:
            raise ValueError("%s: a %s light has no key %s (it takes %s)" % (who, kind, ", ".join(bad), ", ".join(LIGHT_KEYS[kind])))
        arrs = {}
        for k, v in keys.items():
            want = 1 if k in ("intensity", "samples") else 3
            a = np.ascontiguousarray(np.asarray(v, np.int32 if k == "samples" else np.float32).reshape(-1))
            if a.size != want:
                raise ValueError("%s: %s takes %d value%s, got %d" % (who, k, want, "" if want == 1 else "s", a.size))
            if k == "samples" and a[0] != np.asarray(v).reshape(-1)[0]:
                raise ValueError("%s: samples must be a whole number, got %r" % (who, v))
            arrs[k] = a
        return [_np_ptr(arrs[k]) if k in arrs else None for k in _LIGHT_ARGS], arrs

    def set_light(self, index, **keys):
        """Light `index` (scene-file order) as its [light] block would load with these keys set; a key not given keeps its value.  A point
        light takes position / color / intensity, a distant light direction / color / intensity, an area light pos / i / j / samples /
        color / intensity (its sample points are made again when pos, i, j or samples change); any other key, a wrong number of values or
        a bad index raises ValueError and nothing changes.  With a live GPU scene the device's lights are replaced (rtx_scene_set_lights):
        renders queued before the call see the old lights, later ones the new."""
        if not 0 <= index < self.n_lights:
            raise ValueError("set_light: light index %d out of range (%d lights)" % (index, self.n_lights))
        args, _keep = self._light_args("set_light", self.light_type(index), keys)
        if self.host.rah_light_set(self.h, index, *args) != 0:
            raise RtxError("set_light: %s" % self.host.rah_last_error().decode(errors="replace"))

    def add_light(self, type, **keys):
        """A new light of `type` ("point", "distant", "area") after the last one, as a new [light] block with these keys would load (absent
        keys: the loader's defaults); returns its index.  Keys and errors as for set_light."""
        if type not in LIGHT_TYPES:
            raise ValueError("add_light: unknown light type %r (point, distant, area)" % (type,))
        args, _keep = self._light_args("add_light", type, keys)
        index = self.host.rah_light_add(self.h, LIGHT_TYPES[type], *args)
        if index < 0:
            raise RtxError("add_light: %s" % self.host.rah_last_error().decode(errors="replace"))
        self._dims()
        return index

    def remove_light(self, index):
        """Removes light `index` (its [light] block deleted); the lights after it move up by one."""
        if not 0 <= index < self.n_lights:
            raise ValueError("remove_light: light index %d out of range (%d lights)" % (index, self.n_lights))
        if self.host.rah_light_remove(self.h, index) != 0:
            raise RtxError("remove_light: %s" % self.host.rah_last_error().decode(errors="replace"))
        self._dims()

    def add_object(self, type, at=None, **keys):
        """A new object of `type` ("sphere", "plane", "mesh") before object `at` (None: after the last one), as a new [object] block with
        these keys would load (absent keys: the loader's defaults); returns its index.  Every type takes pos / color / material, a sphere
        radius, a plane normal, a mesh size / rot / name (its OBJ file) / diffuse_map / normal_map / specular_map; material is the text of
        a material= line ("reflective", "transparent,1.3", "phong,0.3,0.5,0.6,20"; absent: Diffuse), file names resolve as the scene
        file's do.  An unknown type, a key the type does not have, a wrong number of values or a bad index raises ValueError, a file that
        cannot be loaded RtxError, and nothing changes.  With a live GPU scene the device's objects are replaced (rtx_scene_set_objects):
        every other mesh stays as it is, renders queued before the call see the old objects, later ones the new."""
        if type not in OBJECT_TYPES:
            raise ValueError("add_object: unknown object type %r (sphere, plane, mesh)" % (type,))
        if at is not None and not 0 <= at <= self.n_objects:
            raise ValueError("add_object: object index %d out of range (%d objects)" % (at, self.n_objects))
        bad = [k for k in keys if k not in OBJECT_KEYS[type]]
        if bad:
            raise ValueError("add_object: a %s has no key %s (it takes %s)" % (type, ", ".join(bad), ", ".join(OBJECT_KEYS[type])))
        arrs = {}
        for k, v in keys.items():
            if k in _OBJECT_TEXT:
                if not isinstance(v, str) or not v or "\n" in v:
                    raise ValueError("add_object: %s takes a line of text, got %r" % (k, v))
                if k == "material":
                    parts = v.split(",")
                    if parts[0] not in MATERIAL_VALUES or len(parts) - 1 != MATERIAL_VALUES[parts[0]]:
                        raise ValueError("add_object: material %r (diffuse, reflective, transparent,<ior>, phong,<ambient>,<diffuse>,<specular>,<n>)" % (v,))
                    try:
                        [float(x) for x in parts[1:]]
                    except ValueError:
                        raise ValueError("add_object: material %r: its values must be numbers" % (v,))
                arrs[k] = v.encode()
                continue
            want = 1 if k == "radius" else 3
            a = np.ascontiguousarray(np.asarray(v, np.float32).reshape(-1))
            if a.size != want:
                raise ValueError("add_object: %s takes %d value%s, got %d" % (k, want, "" if want == 1 else "s", a.size))
            arrs[k] = a
        args = [(arrs[k] if k in _OBJECT_TEXT else _np_ptr(arrs[k])) if k in arrs else None for k in _OBJECT_ARGS]
        index = self.host.rah_object_add(self.h, OBJECT_TYPES[type], -1 if at is None else at, self._cwd.encode(), *args)
        if index < 0:
            raise RtxError("add_object: %s" % self.host.rah_last_error().decode(errors="replace"))
        self._dims()
        return index

    def remove_object(self, index):
        """Removes object `index` (its [object] block deleted); the objects after it move up by one.  With a live GPU scene a removed mesh is
        freed with everything of its own, and every other mesh stays as it is (rtx_scene_set_objects)."""
        if not 0 <= index < self.n_objects:
            raise ValueError("remove_object: object index %d out of range (%d objects)" % (index, self.n_objects))
        if self.host.rah_object_remove(self.h, index) != 0:
            raise RtxError("remove_object: %s" % self.host.rah_last_error().decode(errors="replace"))
        self._dims()

    # ---- GPU ------------------------------------------------------------------------------------
    def gpu(self):
        """rtx_scene* of the uploaded scene (flatten + upload on first use; re-applies the view after resize)."""
        self._gpu = C.c_void_p(self.host.rah_scene_gpu(self.h))
        if not self._gpu:
            raise RtxError("no GPU scene: %s" % self.host.rah_last_error().decode(errors="replace"))
        return self._gpu

    @staticmethod
    def _stream_ptr(stream):
        if stream is None:
            try:
                import torch
                if torch.cuda.is_available():
                    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
            except Exception:
                pass
            return None
        return C.c_void_p(getattr(stream, "cuda_stream", stream))

    def render_pass1(self, fb, rows=None, stream=None):
        """Scene::launchWorkers on rows [r0,r1) into the device tensor fb (H,W,3 float32, pre-zeroed)."""
        r0, r1 = rows if rows is not None else (0, self.height)
        _check(self.rtx.rtx_render_pass1(self.gpu(), r0, r1, C.c_void_p(fb.data_ptr()), self._stream_ptr(stream)),
               "rtx_render_pass1")

    def sobel(self, fb, mask, rows=None, stream=None):
        r0, r1 = rows if rows is not None else (0, self.height)
        _check(self.rtx.rtx_sobel(self.gpu(), C.c_void_p(fb.data_ptr()), r0, r1, C.c_void_p(mask.data_ptr()),
                                  self._stream_ptr(stream)), "rtx_sobel")

    def render_ssaa(self, mask, fb, rows=None, stream=None):
        r0, r1 = rows if rows is not None else (0, self.height)
        _check(self.rtx.rtx_render_ssaa(self.gpu(), C.c_void_p(mask.data_ptr()), r0, r1, C.c_void_p(fb.data_ptr()),
                                        self._stream_ptr(stream)), "rtx_render_ssaa")

    def render_frame(self, fb, mask, rows=None, stream=None):
        """Pass 1 + Sobel + SSAA of rows [r0,r1) in one launch (rtx_render_frame): same fb and mask as the three calls."""
        r0, r1 = rows if rows is not None else (0, self.height)
        _check(self.rtx.rtx_render_frame(self.gpu(), r0, r1, C.c_void_p(fb.data_ptr()), C.c_void_p(mask.data_ptr()),
                                         self._stream_ptr(stream)), "rtx_render_frame")

    def render_ac(self, fb, counts=None, stream=None):
        """The showAC heat map (rtx_render_ac, Scene::render scene.cpp:601-634) into the device tensor fb (H,W,3 float32): every pixel
        = its count of passed acceleration-structure boxes / the frame's largest count.  counts: optional device tensor of H*W
        int32 / uint32 that receives the raw per-pixel counts (their max is the normaliser)."""
        cp = C.c_void_p(counts.data_ptr()) if counts is not None else None
        _check(self.rtx.rtx_render_ac(self.gpu(), C.c_void_p(fb.data_ptr()), cp, self._stream_ptr(stream)), "rtx_render_ac")

    def set_knob(self, name, value):
        """Experiment / test knob of this scene (include/rtx.h, rtx_set_knob); no knob changes a pixel."""
        _check(self.rtx.rtx_set_knob(self.gpu(), name.encode(), float(value)), "rtx_set_knob")

    def kernel_variant(self):
        """The compile-time variant the next mesh launches take (rtx_kernel_variant): dict of booleans boxes, plain, analytic, stats, cull."""
        b = C.c_uint32(0)
        _check(self.rtx.rtx_kernel_variant(self.gpu(), C.byref(b)), "rtx_kernel_variant")
        return {k: bool(b.value & bit) for k, bit in VARIANT_BITS.items()}

    def ssaa_list(self):
        """What the last render_ssaa built, and the split limits of the last frame rendered in one launch (rtx_ssaa_list_read; synchronises
        the device).  dict: local, sparse (layouts), flagged (the pixels the layout was decided from), tiles, tiles_x, heavy_ticks,
        spread_slots, very, spread_px, split4, split16, cost_sum, frame_waves, and scan: the 2 tiles + 1 exclusive-scan offsets
        (None before the first list)."""
        g = self.gpu()
        info = np.zeros(16, np.uint32)
        _check(self.rtx.rtx_ssaa_list_read(g, _np_ptr(info), None, 0), "rtx_ssaa_list_read")
        d = dict(local=bool(info[0]), flagged=int(info[1]), sparse=bool(info[2]), tiles=int(info[3]), tiles_x=int(info[4]),
                 heavy_ticks=int(info[5]), spread_slots=int(info[6]), very=int(info[7]), spread_px=int(info[8]),
                 split4=int(info[9]), split16=int(info[10]), cost_sum=int(info[11]) | int(info[12]) << 32, frame_waves=int(info[13]), scan=None)
        if d["tiles"]:
            scan = np.zeros(2 * d["tiles"] + 1, np.uint32)
            _check(self.rtx.rtx_ssaa_list_read(g, _np_ptr(info), _np_ptr(scan), scan.size), "rtx_ssaa_list_read")
            d["scan"] = scan
        return d

    def cost_grid(self):
        """First-frame cost estimate of the current view: (refs, leaves) per cell of 2 x 2 tiles, arrays grid_h x grid_w."""
        gw, gh = C.c_uint32(0), C.c_uint32(0)
        _check(self.rtx.rtx_cost_grid_read(self.gpu(), None, 0, C.byref(gw), C.byref(gh)), "rtx_cost_grid_read")
        g = np.zeros((gh.value, gw.value, 2), np.uint32)
        _check(self.rtx.rtx_cost_grid_read(self.gpu(), _np_ptr(g), g.size, C.byref(gw), C.byref(gh)), "rtx_cost_grid_read")
        return g[..., 0], g[..., 1]

    def frame_status(self):
        """The host's synchronisation point for render_frame: 0, or error | 0x100 when the single launch gave up and the
        frame was rendered again in three launches (include/rtx.h)."""
        st = C.c_uint32(0)
        _check(self.rtx.rtx_frame_status(self.gpu(), C.byref(st)), "rtx_frame_status")
        return st.value

    def set_frame_mode(self, mode):
        """render_frame: -1 measure and choose (default), 0 always three launches, 1 always one launch."""
        _check(self.rtx.rtx_set_frame_mode(self.gpu(), int(mode)), "rtx_set_frame_mode")

    def frame_mode(self):
        """(mode of the last render_frame: 0 three launches / 1 one launch, measured split ms, measured fused ms; -1 = not yet)."""
        m, a, b = C.c_int(-1), C.c_float(-1), C.c_float(-1)
        _check(self.rtx.rtx_frame_mode(self.gpu(), C.byref(m), C.byref(a), C.byref(b)), "rtx_frame_mode")
        return m.value, a.value, b.value

    def quantize(self, fb, out, stream=None):
        _check(self.rtx.rtx_quantize_bgr8(self.gpu(), C.c_void_p(fb.data_ptr()), C.c_void_p(out.data_ptr()),
                                          self._stream_ptr(stream)), "rtx_quantize_bgr8")

    def render_host(self, ssaa=True):
        """Whole frame into a numpy array through the host-buffer convenience entry (PCIe-inclusive)."""
        fb = np.zeros((self.height, self.width, 3), np.float32)
        _check(self.rtx.rtx_render_frame_host(self.gpu(), int(bool(ssaa)), _np_ptr(fb)), "rtx_render_frame_host")
        return fb

    def cast_rays(self, rays):
        """Render::trace + Render::castRay(depth 0) for n probe rays (n x 6 host array) -> (hits n x 8, colours n x 3)."""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        n = rays.shape[0]
        hits = np.zeros((n, 8), np.float32)
        col = np.zeros((n, 3), np.float32)
        _check(self.rtx.rtx_cast_rays(self.gpu(), n, _np_ptr(rays), _np_ptr(hits), _np_ptr(col)), "rtx_cast_rays")
        return hits, col

    def trace_rays(self, rays, hits=True, colours=True, stream=None):
        """rtx_trace_rays: Render::trace + Render::castRay(depth 0) for the rays of a device tensor, on the device.
        rays: contiguous float32 torch tensor (n, 6) = {orig xyz, dir xyz} on this scene's device.  Returns (hits (n, 8) | None,
        colours (n, 3) | None): new float32 tensors on that device, each ray's the bits of cast_rays.  Asynchronous on `stream` (None:
        torch's current stream of the rays' device); the results are ready when that stream is.  With a torch.cuda.Stream the outputs are
        allocated on it and the rays recorded on it (torch's caching allocator); a raw hipStream_t handle is used as given, so the caller
        then keeps the rays and the outputs alive and unreused until that stream has finished with them."""
        import torch
        if not (hits or colours):
            raise ValueError("trace_rays: nothing to compute (hits and colours are both off)")
        n = _check_rays("trace_rays", rays, self.device)
        alloc_on, st = _query_stream(stream, rays.device, (rays,))
        with torch.cuda.stream(alloc_on):
            h = torch.empty((n, 8), dtype=torch.float32, device=rays.device) if hits else None
            c = torch.empty((n, 3), dtype=torch.float32, device=rays.device) if colours else None
        if n:
            _check(self.rtx.rtx_trace_rays(self.gpu(), n, _ptr(rays), _ptr(h), _ptr(c), st), "rtx_trace_rays")
        return h, c

    def surface_rays(self, rays, hits=False, position=False, normal=True, albedo=True, specular=False, stream=None):
        """rtx_surface_rays: Render::trace of the rays of a device tensor and getSurfaceData at their hits, on the device -- what a caller
        needs to shade a hit or to build the next ray from it.  rays: as for trace_rays.  Returns a dict of the channels asked for, new
        float32 tensors on the rays' device: "hits" (n, 8), trace_rays' record; "position" (n, 3), orig + dir * tNear; "normal" (n, 3),
        the shading normal (vertex normals, normal map); "albedo" (n, 3), the object's colour or its diffuse map's texel, at a miss the
        sky / background colour of the direction; "specular" (n,), the object's specular coefficient or its specular map's value.
        position, normal and specular are 0 at a miss.  The object's other constants are in device_objects(), indexed by hits[:, 1].
        Asynchronous on `stream`, which is handled as in trace_rays."""
        import torch
        f32 = torch.float32
        channels = (("hits", hits, (8,), f32), ("position", position, (3,), f32), ("normal", normal, (3,), f32),
                    ("albedo", albedo, (3,), f32), ("specular", specular, (), f32))
        if not any(on for _, on, _, _ in channels):
            raise ValueError("surface_rays: nothing to compute (every channel is off)")
        n = _check_rays("surface_rays", rays, self.device)
        alloc_on, st = _query_stream(stream, rays.device, (rays,))
        out, ptrs = _query_outputs(channels, n, rays.device, alloc_on)
        if n:
            _check(self.rtx.rtx_surface_rays(self.gpu(), n, _ptr(rays), C.byref(SurfaceBuffers(*ptrs)), st), "rtx_surface_rays")
        return out

    def light_rays(self, rays, diffuse=True, specular=True, hits=False, per_light=False, stream=None):
        """rtx_light_rays: the direct light at the first hits of the rays of a device tensor, on the device -- castRay's sums over the
        lights with their shadow rays, bit for bit (include/rtx_light.h).  rays: as for trace_rays.  Returns a dict of new tensors on the
        rays' device: "diffuse" (n, 3) and "specular" (n, 3), float32, the sums a Diffuse hit's colour (albedo * diffuse) and a Phong hit's
        ((albedo * ambient + diffuse * kd) + specular * ks) are made of; "hits" (n, 8), trace_rays' record; with per_light also
        "light_diffuse" (n, L, 3) and "light_specular" (n, L, 3), float32, what each of the scene's L lights adds to the sums, and
        "light_open" (n, L), int32, how many of the light's shadow rays arrive (0 / 1; up to its number of samples for an area light).
        Everything is 0 at a miss, and the sums are 0 on a scene without lights (L = 0).  Asynchronous on `stream`, which is handled as in
        trace_rays."""
        import torch
        if not (diffuse or specular or hits or per_light):
            raise ValueError("light_rays: nothing to compute (every channel is off)")
        n = _check_rays("light_rays", rays, self.device)
        nl = self.n_lights if per_light else 0
        channels = (("hits", hits, (8,), torch.float32), ("diffuse", diffuse, (3,), torch.float32), ("specular", specular, (3,), torch.float32),
                    ("light_diffuse", per_light, (nl, 3), torch.float32), ("light_specular", per_light, (nl, 3), torch.float32),
                    ("light_open", per_light, (nl,), torch.int32))
        alloc_on, st = _query_stream(stream, rays.device, (rays,))
        out, ptrs = _query_outputs(channels, n, rays.device, alloc_on)
        if n and any(p is not None for p in ptrs):
            _check(self.rtx.rtx_light_rays(self.gpu(), n, _ptr(rays), C.byref(LightBuffers(nl, *ptrs)), st), "rtx_light_rays")
        return out

    def light_points(self, points, view=None, diffuse=True, specular=None, per_light=False, stream=None):
        """rtx_light_points: the direct light at surface points the caller already has, on the device -- castRay's sums over the lights with
        their shadow rays at a hit at P with the shading normal N, bit for bit (include/rtx_points.h).  points: contiguous float32 torch
        tensor (n, 6) = {P xyz, N xyz} on this scene's device; N is used as stored.  view: None, or a float32 tensor (n, 4) = {V xyz, ns}
        on that device -- V the direction of the ray that arrived at P, ns the specular exponent.  specular: None means "iff view is
        given"; True without a view is refused.  Returns a dict of new tensors on the points' device, as light_rays does: "diffuse" (n, 3)
        and "specular" (n, 3), float32; with per_light also "light_diffuse" (n, L, 3), "light_specular" (n, L, 3) when specular is on, and
        "light_open" (n, L), int32, how many of the light's shadow rays arrive.  The sums are 0 on a scene without lights (L = 0).
        Asynchronous on `stream`, which is handled as in trace_rays (the view is recorded on it like the points)."""
        import torch
        if specular is None:
            specular = view is not None
        if specular and view is None:
            raise ValueError("light_points: specular needs a view")
        if not (diffuse or specular or per_light):
            raise ValueError("light_points: nothing to compute (every channel is off)")
        n = _check_rays("light_points", points, self.device, "points")
        if view is not None:
            _check_tensor("light_points", "view", view, torch.float32, (n, 4), self.device)
        nl = self.n_lights if per_light else 0
        channels = (("diffuse", diffuse, (3,), torch.float32), ("specular", specular, (3,), torch.float32),
                    ("light_diffuse", per_light, (nl, 3), torch.float32), ("light_specular", per_light and specular, (nl, 3), torch.float32),
                    ("light_open", per_light, (nl,), torch.int32))
        alloc_on, st = _query_stream(stream, points.device, (points, view))
        out, ptrs = _query_outputs(channels, n, points.device, alloc_on)
        if n and any(p is not None for p in ptrs):
            _check(self.rtx.rtx_light_points(self.gpu(), n, _ptr(points), _ptr(view), C.byref(LightBuffers(nl, None, *ptrs)), st), "rtx_light_points")
        return out

    def ao_points(self, points, dirs, radius=float("inf"), ao=True, counts=False, stream=None):
        """rtx_ao_points: ambient occlusion at surface points the caller already has, on the device (include/rtx_points.h).  points: as
        for light_points.  For every point, each direction of `dirs` (float32 (K, 3), K in 1 .. 256, world space, used as stored) with
        N . d > 0 is traced from P + N * bias with the rule of occluded() and the range `radius` (> 0; inf: the whole ray; the library
        refuses anything else, and K outside 1 .. 256).  Returns a dict of the channels asked for, new tensors (n,) on the points' device:
        "ao", float32, open / traced, 1.0 where nothing was traced; "counts", int32, open | traced << 16.  Asynchronous on `stream`,
        which is handled as in trace_rays (dirs is recorded on it like the points)."""
        import torch
        if not (ao or counts):
            raise ValueError("ao_points: nothing to compute (ao and counts are both off)")
        n = _check_rays("ao_points", points, self.device, "points")
        _check_tensor("ao_points", "dirs", dirs, torch.float32, ("K", 3), self.device)
        alloc_on, st = _query_stream(stream, points.device, (points, dirs))
        out, ptrs = _query_outputs((("ao", ao, (), torch.float32), ("counts", counts, (), torch.int32)), n, points.device, alloc_on)
        if n:
            par = AoParams(dirs.shape[0], dirs.data_ptr(), float(radius))
            _check(self.rtx.rtx_ao_points(self.gpu(), n, _ptr(points), C.byref(par), ptrs[0], ptrs[1], st), "rtx_ao_points")
        return out

    def radiance_points(self, points, dirs, weights=None, cosine=False, total=True, counts=False, stream=None):
        """rtx_radiance_points: the radiance that arrives at surface points the caller already has, summed over a set of directions, on
        the device (include/rtx_radiance.h).  points: as for light_points.  For every point, each direction of `dirs` (float32 (K, 3), K
        in 1 .. 256, world space, used as stored) with c = N . d > 0 is cast from P + N * bias as trace_rays(colours=True) casts a ray --
        the whole recursion, bit for bit -- and its colour enters the sum with the weight weights[k] (float32 (K,); None: 1) times c when
        `cosine` is on, in the order of the directions.  Returns a dict of the channels asked for, new tensors on the points' device:
        "sum" (n, 3), float32, +0 where nothing was traced (total=True); "counts" (n,), int32, the number of traced directions.
        Refused while the "show_normals" flag is set.  Asynchronous on `stream`, which is handled as in trace_rays (dirs and weights are
        recorded on it like the points)."""
        import torch
        if not (total or counts):
            raise ValueError("radiance_points: nothing to compute (total and counts are both off)")
        n = _check_rays("radiance_points", points, self.device, "points")
        _check_tensor("radiance_points", "dirs", dirs, torch.float32, ("K", 3), self.device)
        k = dirs.shape[0]
        if k < 1 or k > 256:
            raise ValueError("radiance_points: 1 .. 256 directions per call, got %d" % k)
        if weights is not None:
            _check_tensor("radiance_points", "weights", weights, torch.float32, (k,), self.device)
        alloc_on, st = _query_stream(stream, points.device, (points, dirs, weights))
        out, ptrs = _query_outputs((("sum", total, (3,), torch.float32), ("counts", counts, (), torch.int32)), n, points.device, alloc_on)
        if n:
            par = RadianceParams(k, dirs.data_ptr(), weights.data_ptr() if weights is not None else None, 1 if cosine else 0)
            _check(self.rtx.rtx_radiance_points(self.gpu(), n, _ptr(points), C.byref(par), ptrs[0], ptrs[1], st), "rtx_radiance_points")
        return out

    SCATTER_CHANNELS = ("hits", "local", "reflect", "refract", "weight", "kinds")

    def scatter_rays(self, rays, local=True, reflect=True, refract=True, weight=True, kinds=True, hits=False, stream=None):
        """rtx_scatter_rays: what castRay does at the first hits of the rays of a device tensor short of recursing, on the device, bit for
        bit (include/rtx_scatter.h).  rays: as for trace_rays.  Returns a dict of the channels asked for, new tensors on the rays' device:
        "local" (n, 3), the part of the hit's colour that needs no further ray (all of it at a Diffuse or Phong hit and at a miss, the
        specular highlight at a Reflective or Transparent one); "reflect" and "refract" (n, 6), the {orig, dir} of the secondary rays the
        recursion casts; "weight" (n, 2), the factors their colours enter with; "kinds" (n,), torch.uint8, bit 0: there is a reflection
        ray, bit 1: a refraction ray; "hits" (n, 8), trace_rays' record.  Rays and weights that do not exist are 0.  With C(r) the
        colour of a child, the ray's colour is C(reflect) * 0.8 + local at a mirror, ((0 + C(refract) * weight[1]) + C(reflect) *
        weight[0]) + local at glass (the refraction term only where bit 1 is set) and local itself where kinds is 0: cast_tree.
        Asynchronous on `stream`, which is handled as in trace_rays."""
        import torch
        channels = (("hits", hits, (8,), torch.float32), ("local", local, (3,), torch.float32), ("reflect", reflect, (6,), torch.float32),
                    ("refract", refract, (6,), torch.float32), ("weight", weight, (2,), torch.float32), ("kinds", kinds, (), torch.uint8))
        if not any(on for _, on, _, _ in channels):
            raise ValueError("scatter_rays: nothing to compute (every channel is off)")
        n = _check_rays("scatter_rays", rays, self.device)
        alloc_on, st = _query_stream(stream, rays.device, (rays,))
        out, ptrs = _query_outputs(channels, n, rays.device, alloc_on)      # (in the order of SCATTER_CHANNELS, the struct's)
        if n:
            _check(self.rtx.rtx_scatter_rays(self.gpu(), n, _ptr(rays), C.byref(ScatterBuffers(*ptrs)), st), "rtx_scatter_rays")
        return out

    def sky(self, rays, stream=None):
        """rtx_sky_rays: Scene::getSkybox of the directions of the rays of a device tensor -- the sky texel with useSkybox, the background
        colour without, whatever the ray would hit: castRay's answer for a ray beyond max_ray_depth.  rays: as for trace_rays.  Returns a
        new float32 tensor (n, 3) on the rays' device.  Asynchronous on `stream`, which is handled as in trace_rays."""
        import torch
        n = _check_rays("sky", rays, self.device)
        alloc_on, st = _query_stream(stream, rays.device, (rays,))
        with torch.cuda.stream(alloc_on):
            c = torch.empty((n, 3), dtype=torch.float32, device=rays.device)
        if n:
            _check(self.rtx.rtx_sky_rays(self.gpu(), n, _ptr(rays), _ptr(c), st), "rtx_sky_rays")
        return c

    @property
    def max_ray_depth(self):
        """the scene file's max_ray_depth: the deepest level of castRay's recursion that is still traced"""
        return int(self.host.rah_max_ray_depth(self.h))

    def cast_tree(self, rays, depth=None, stream=None):
        """castRay level by level, in torch on top of scatter_rays and sky: level 0 is `rays`, level k + 1 the children of level k in the
        order of their parents, a parent's refraction ray before its reflection ray.  A level up to `depth` (None: the scene's
        max_ray_depth) is one scatter_rays call; the rays of the level beyond it are not traced, their colour is sky(); a negative depth
        makes level 0 sky.  The children are compacted with a boolean mask, which costs one host synchronisation per level.  The colours
        are then composed from the deepest level up with the identities of include/rtx_scatter.h as written there, so with depth=None
        they are the bits of trace_rays(rays)[1].
        Returns (colours (n, 3), levels): levels[k] is a dict of "rays" (m, 6), "parent" (m,) int64 index into level k - 1 (None at
        level 0), "kind" (m,) uint8 (0 for a ray that is not traced), "weight" (m, 2), "local" (m, 3) and "colour" (m, 3).
        Everything is queued on `stream`: None, torch's current stream, or a torch.cuda.Stream, which is made the current one for the
        torch operations in between (a raw handle is refused)."""
        import torch
        _check_rays("cast_tree", rays, self.device)
        if stream is not None and not isinstance(stream, torch.cuda.Stream):
            raise ValueError("cast_tree: stream must be a torch.cuda.Stream or None, got %s" % type(stream).__name__)
        depth = self.max_ray_depth if depth is None else int(depth)
        levels, cur, parent = [], rays, None
        if stream is not None:
            rays.record_stream(stream)
        with torch.cuda.stream(stream):
            for k in range(max(depth, -1) + 2):
                m = cur.shape[0]
                if k > depth or m == 0:
                    sky = self.sky(cur)
                    levels.append(dict(rays=cur, parent=parent, kind=torch.zeros(m, dtype=torch.uint8, device=cur.device),
                                       weight=torch.zeros((m, 2), dtype=torch.float32, device=cur.device), local=sky, colour=sky))
                    break
                s = self.scatter_rays(cur)
                levels.append(dict(rays=cur, parent=parent, kind=s["kinds"], weight=s["weight"], local=s["local"], colour=None))
                # the children: per parent {refract, reflect}, those that exist (the mask's count comes to the host: one synchronisation)
                both = torch.stack([s["refract"], s["reflect"]], 1).reshape(2 * m, 6)
                exists = torch.stack([(s["kinds"] & 2) != 0, (s["kinds"] & 1) != 0], 1).reshape(2 * m)
                at = torch.nonzero(exists).reshape(-1)
                if at.numel() == 0:
                    break
                cur, parent = both[at].contiguous(), at // 2
                levels[-1]["child_slot"] = at
            for k in range(len(levels) - 1, -1, -1):
                lv = levels[k]
                if lv["colour"] is not None:
                    continue
                m = lv["rays"].shape[0]
                at = lv.pop("child_slot", None)
                col = lv["local"].clone()
                if at is not None:
                    # colours of the children in the parents' slots: [:, 0] of the refraction ray, [:, 1] of the reflection ray
                    cc = torch.zeros((2 * m, 3), dtype=torch.float32, device=col.device)
                    cc[at] = levels[k + 1]["colour"]
                    cc = cc.reshape(m, 2, 3)
                    kind, w = lv["kind"], lv["weight"]
                    # a mirror and glass in total internal reflection both have kind 1; glass composes from +0 as castRay does, which differs
                    # from the mirror's form only in the sign of a zero, so the form is chosen by the weight the contract gives a mirror
                    mirror = (kind == 1) & (w[:, 0] == torch.tensor(0.8, dtype=torch.float32, device=col.device))
                    acc = torch.zeros((m, 3), dtype=torch.float32, device=col.device)
                    acc = torch.where(((kind & 2) != 0)[:, None], acc + cc[:, 0] * w[:, 1:2], acc)
                    glass = (acc + cc[:, 1] * w[:, 0:1]) + lv["local"]
                    col = torch.where(((kind & 1) != 0)[:, None], glass, col)
                    col = torch.where(mirror[:, None], cc[:, 1] * w[:, 0:1] + lv["local"], col)
                lv["colour"] = col
        return levels[0]["colour"], levels

    def occluded(self, rays, tmax=None, stream=None):
        """rtx_occluded_rays: is anything between a ray's origin and its range?  Render::trace of a shadow ray whose info.tNear starts at
        tmax -- 1 iff some object that is not Transparent is hit at tNear < tmax (strict, float32; a NaN range occludes nothing).
        rays: contiguous float32 torch tensor (n, 6) = {orig xyz, dir xyz} on this scene's device.  tmax: a float32 tensor (n,) on that
        device, a Python float (one range for every ray) or None (+inf: the whole ray).  Returns a new torch.uint8 tensor (n,) of 0 / 1
        on that device.  Asynchronous on `stream`, which is handled as in trace_rays (a tmax tensor is recorded on it like the rays)."""
        import torch
        n = _check_rays("occluded", rays, self.device)
        if isinstance(tmax, torch.Tensor):
            _check_tensor("occluded", "tmax", tmax, torch.float32, (n,))
            if tmax.device != rays.device:
                raise ValueError("occluded: tmax must be on the rays' device %s, got %s" % (rays.device, tmax.device))
        elif tmax is not None and not isinstance(tmax, (int, float)):
            raise ValueError("occluded: tmax must be a torch tensor, a float or None, got %s" % type(tmax).__name__)
        alloc_on, st = _query_stream(stream, rays.device, (rays, tmax if isinstance(tmax, torch.Tensor) else None))
        with torch.cuda.stream(alloc_on):
            out = torch.empty((n,), dtype=torch.uint8, device=rays.device)
            if tmax is not None and not isinstance(tmax, torch.Tensor):
                tmax = torch.full((n,), float(tmax), dtype=torch.float32, device=rays.device)
                if stream is not None and alloc_on is None:
                    torch.cuda.current_stream(rays.device).synchronize()      # (a raw handle: torch cannot order the fill before it)
        if n:
            _check(self.rtx.rtx_occluded_rays(self.gpu(), n, _ptr(rays), _ptr(tmax), _ptr(out), st), "rtx_occluded_rays")
        return out

    def render_aov(self, depth=None, object_id=None, triangle_id=None, uv=None, normal=None, albedo=None, rows=None, stream=None):
        """rtx_render_aov: what the primary ray of every pixel of pass 1 met, written into the device tensors that are given (any subset,
        at least one): depth float32 (H, W), object_id and triangle_id int32 (H, W), uv float32 (H, W, 2), normal and albedo float32
        (H, W, 3) -- contiguous, on this scene's device.  Written: the pixels x < W-1, y < H-1 of rows [r0, r1) that this part owns;
        nothing else of a tensor is touched.  A miss: depth FLT_MAX, ids -1, uv (-1, -1), normal 0, albedo the sky / background colour.
        Asynchronous on `stream` (None: torch's current stream of the scene's device); with a torch.cuda.Stream the tensors are
        recorded on it."""
        import torch
        hw = (self.height, self.width)
        given = (("depth", depth, torch.float32, hw), ("object_id", object_id, torch.int32, hw), ("triangle_id", triangle_id, torch.int32, hw),
                 ("uv", uv, torch.float32, hw + (2,)), ("normal", normal, torch.float32, hw + (3,)), ("albedo", albedo, torch.float32, hw + (3,)))
        st, ptrs = _frame_tensors("render_aov", given, self.device, stream)
        r0, r1 = rows if rows is not None else (0, self.height)
        _check(self.rtx.rtx_render_aov(self.gpu(), r0, r1, C.byref(AovBuffers(*ptrs)), st), "rtx_render_aov")

    def view_target(self, pos, rot, fov=None, width=None, height=None):
        """The camera fields and size of one view of a batch (ViewTarget with NULL buffers; rah_view_target): what this scene's own view
        would hold after set_camera(pos, rot) + resize(width, height) -- with the fov `fov` in degrees instead of the scene's when it is
        given.  The scene itself is not changed.  Host only."""
        t = ViewTarget()
        self._fill_view_target(t, pos, rot, fov, self.width if width is None else int(width), self.height if height is None else int(height))
        return t

    def _fill_view_target(self, t, pos, rot, fov, w, h):
        # (plain ctypes, no numpy: render_views does this once per camera)
        p = (C.c_float * 3)(float(pos[0]), float(pos[1]), float(pos[2])); r = (C.c_float * 3)(float(rot[0]), float(rot[1]), float(rot[2]))
        if self.host.rah_view_target(self.h, p, r, -1.0 if fov is None else float(fov), w, h, C.byref(t)) != 0:
            raise ValueError("view_target: %s" % self.host.rah_last_error().decode(errors="replace"))

    def render_views(self, cameras, fbs, masks=None, ssaa=False, stream=None):
        """rtx_render_views: many views of this scene in one call.  cameras: a sequence of (pos, rot) or (pos, rot, fov) -- rot and fov in
        degrees, fov None or absent: the scene's; cube_cameras(pos) gives the six of a cube map.  fbs: one float32 tensor (N, H, W, 3) or a
        list of N tensors (H_i, W_i, 3), zeroed by the caller; the sizes of the views are the tensors'.  masks (required with ssaa, else
        not written): uint8 (N, H, W) or a list of (H_i, W_i).  All contiguous and on this scene's device; no two views share memory.
        View i receives the bits of set_camera + resize + render_pass1 (ssaa: + sobel + render_ssaa) with its camera and size; bias, ray
        depth, background and the culling / skybox flags are this scene's current ones for every view.  The scene's own view, its tile
        costs and its timings are left as they are.  Asynchronous on `stream` (None: torch's current stream of the scene's device); with a
        torch.cuda.Stream the tensors are recorded on it."""
        import torch
        cameras = list(cameras)
        n = len(cameras)
        # one tensor for the batch: checked once, the views' addresses follow from its shape (no per-view tensor is made)
        whole = isinstance(fbs, torch.Tensor)
        if whole:
            _check_tensor("render_views", "fbs", fbs, torch.float32, ("N", "H", "W", 3), self.device)
        if isinstance(masks, torch.Tensor) != whole and masks is not None:
            raise ValueError("render_views: fbs and masks must both be one tensor or both be lists")
        if whole and masks is not None:
            _check_tensor("render_views", "masks", masks, torch.uint8, (fbs.shape[0], fbs.shape[1], fbs.shape[2]), self.device)
        fb_list = fbs if whole else list(fbs)
        mask_list = masks if whole or masks is None else list(masks)
        if len(fb_list) != n:
            raise ValueError("render_views: %d cameras but %d framebuffers" % (n, len(fb_list)))
        if ssaa and mask_list is None:
            raise ValueError("render_views: ssaa needs masks")
        if mask_list is not None and len(mask_list) != n:
            raise ValueError("render_views: %d cameras but %d masks" % (n, len(mask_list)))
        targets = (ViewTarget * max(n, 1))()
        for i, cam in enumerate(cameras):
            if len(cam) not in (2, 3):
                raise ValueError("render_views: camera %d must be (pos, rot) or (pos, rot, fov)" % i)
            if whole:
                h, w = int(fbs.shape[1]), int(fbs.shape[2])
                fb_ptr = fbs.data_ptr() + i * h * w * 12
                mask_ptr = masks.data_ptr() + i * h * w if masks is not None else None
            else:
                fb = fb_list[i]
                _check_tensor("render_views", "fbs[%d]" % i, fb, torch.float32, ("H", "W", 3), self.device)
                h, w = int(fb.shape[0]), int(fb.shape[1])
                fb_ptr, mask_ptr = fb.data_ptr(), None
                if mask_list is not None:
                    _check_tensor("render_views", "masks[%d]" % i, mask_list[i], torch.uint8, (h, w), self.device)
                    mask_ptr = mask_list[i].data_ptr()
            if h < 1 or w < 1:
                raise ValueError("render_views: fbs[%d] is empty" % i)
            t = targets[i]
            self._fill_view_target(t, cam[0], cam[1], cam[2] if len(cam) == 3 else None, w, h)
            t.fb_dev = fb_ptr
            t.mask_dev = mask_ptr
        _, st = _query_stream(stream, self.device, ([fbs, masks] if whole else fb_list + (mask_list or [])))
        _check(self.rtx.rtx_render_views(self.gpu(), n, targets, 1 if ssaa else 0, st), "rtx_render_views")

    def render_views_aov(self, cameras, depth=None, object_id=None, triangle_id=None, uv=None, normal=None, albedo=None, position=None, rays=None,
                         stream=None):
        """rtx_render_views_aov: first-hit buffers and primary rays of many views of this scene in one call.  cameras: render_views'
        sequence of (pos, rot) or (pos, rot, fov); cube_cameras(pos) gives the six of a cube map.  Every channel that is given (any subset,
        at least one) is one tensor (N, H, W[, c]) or a list of N tensors (H_i, W_i[, c]) -- all channels in the same form --, contiguous
        and on this scene's device: depth float32, object_id and triangle_id int32, uv float32 c = 2, normal, albedo and position float32
        c = 3, rays float32 c = 6.  The sizes of the views are the tensors'; the channels of a view agree in size.
        View i receives in its pixels x < W-1, y < H-1 the bits of set_camera + resize + render_aov with its camera and size, in `position`
        the bits of surface_rays' position for the pixel's primary ray ((0, 0, 0) at a miss) and in `rays` that ray itself, {orig, dir}:
        trace_rays(rays_i.reshape(-1, 6)) is render_pass1 of that view.  Nothing else of a tensor is touched.  The culling and skybox flags
        and the background are this scene's current ones for every view.  The scene's own view, its tile costs and its timings are left
        as they are.  Asynchronous on `stream` (None: torch's current stream of the scene's device); with a torch.cuda.Stream the tensors
        are recorded on it."""
        import torch
        who = "render_views_aov"
        cameras = list(cameras)
        n = len(cameras)
        f32, i32 = torch.float32, torch.int32
        table = (("depth", depth, f32, ()), ("object_id", object_id, i32, ()), ("triangle_id", triangle_id, i32, ()), ("uv", uv, f32, (2,)),
                 ("normal", normal, f32, (3,)), ("albedo", albedo, f32, (3,)), ("position", position, f32, (3,)), ("rays", rays, f32, (6,)))
        given = [(k, name, t, dtype, tail) for k, (name, t, dtype, tail) in enumerate(table) if t is not None]
        if not given:
            raise ValueError("%s: nothing to compute (at least one channel is needed)" % who)
        for _, name, t, _, _ in given:
            if not isinstance(t, (torch.Tensor, list, tuple)):
                raise ValueError("%s: %s must be a torch tensor or a list of torch tensors, got %s" % (who, name, type(t).__name__))
        # one tensor per channel for the batch: checked once, the views' addresses follow from its shape (no per-view tensor is made)
        whole = isinstance(given[0][2], torch.Tensor)
        if any(isinstance(t, torch.Tensor) != whole for _, _, t, _, _ in given):
            raise ValueError("%s: the channels must all be one tensor or all be lists" % who)
        if whole:
            nhw = None
            for _, name, t, dtype, tail in given:
                _check_tensor(who, name, t, dtype, (nhw or ("N", "H", "W")) + tail)
                nhw = nhw or tuple(int(x) for x in t.shape[:3])
            if nhw[0] != n:
                raise ValueError("%s: %d cameras but %d views in %s" % (who, n, nhw[0], given[0][1]))
            if nhw[1] < 1 or nhw[2] < 1:
                raise ValueError("%s: %s is empty" % (who, given[0][1]))
        else:
            for _, name, t, _, _ in given:
                if len(t) != n:
                    raise ValueError("%s: %d cameras but %d tensors in %s" % (who, n, len(t), name))
        targets = (ViewAovTarget * max(n, 1))()
        for i, cam in enumerate(cameras):
            if len(cam) not in (2, 3):
                raise ValueError("%s: camera %d must be (pos, rot) or (pos, rot, fov)" % (who, i))
            t = targets[i]
            if whole:
                h, w = nhw[1], nhw[2]
                for k, _, ten, _, tail in given:
                    setattr(t, ViewAovTarget._fields_[6 + k][0], ten.data_ptr() + i * h * w * 4 * (tail[0] if tail else 1))
            else:
                hw = None
                for k, name, tens, dtype, tail in given:
                    _check_tensor(who, "%s[%d]" % (name, i), tens[i], dtype, (hw or ("H", "W")) + tail)
                    hw = hw or (int(tens[i].shape[0]), int(tens[i].shape[1]))
                    setattr(t, ViewAovTarget._fields_[6 + k][0], tens[i].data_ptr())
                h, w = hw
                if h < 1 or w < 1:
                    raise ValueError("%s: %s[%d] is empty" % (who, given[0][1], i))
            self._fill_view_target(t, cam[0], cam[1], cam[2] if len(cam) == 3 else None, w, h)
        # (the device last, so that what is wrong with the shapes and the cameras is said first)
        for _, name, t, _, _ in given:
            for j, x in enumerate((t,) if whole else t):
                _check_device(who, name if whole else "%s[%d]" % (name, j), x, self.device)
        _, st = _query_stream(stream, self.device, [g[2] for g in given] if whole else [x for g in given for x in g[2]])
        _check(self.rtx.rtx_render_views_aov(self.gpu(), n, targets, st), "rtx_render_views_aov")

    def render_ao(self, dirs, radius=float("inf"), ao=None, counts=None, rows=None, stream=None):
        """rtx_render_ao: ambient occlusion of the frame in one launch.  For every pixel of pass 1 whose primary ray hits, each direction
        of `dirs` (float32 (K, 3), K in 1 .. 256, world space, used as stored) with N . d > 0 is traced from P + N * bias with the rule of
        occluded() and the range `radius` (> 0; inf: the whole ray; the library refuses anything else, and K outside 1 .. 256).
        ao, float32 (H, W): open / traced, 1.0 where nothing was traced or hit; counts, int32 (H, W): open | traced << 16.  At least
        one of the two is given; all tensors are contiguous and on this scene's device.  Written: the pixels x < W-1, y < H-1 of rows [r0, r1) that this part owns; nothing else of a tensor is touched.
        Asynchronous on `stream` (None: torch's current stream of the scene's device); with a torch.cuda.Stream the tensors are
        recorded on it."""
        import torch
        hw = (self.height, self.width)
        st, ptrs = _frame_tensors("render_ao", (("ao", ao, torch.float32, hw), ("counts", counts, torch.int32, hw)), self.device, stream,
                                  inputs=(("dirs", dirs, torch.float32, ("K", 3)),))
        r0, r1 = rows if rows is not None else (0, self.height)
        par = AoParams(dirs.shape[0], dirs.data_ptr(), float(radius))
        _check(self.rtx.rtx_render_ao(self.gpu(), r0, r1, C.byref(par), ptrs[0], ptrs[1], st), "rtx_render_ao")

    def render_light(self, diffuse=None, specular=None, light_diffuse=None, light_specular=None, light_open=None, rows=None, stream=None):
        """rtx_render_light: the direct light of the frame in one launch -- for every pixel of pass 1 castRay's sums over the lights with
        their shadow rays at the first hit of its primary ray, the bits of light_rays for that ray (include/rtx_render_light.h) -- written
        into the device tensors that are given (any subset, at least one): diffuse and specular float32 (H, W, 3), the sums a Diffuse
        hit's colour (albedo * diffuse) and a Phong hit's ((albedo * ambient + diffuse * kd) + specular * ks) are made of; light_diffuse
        and light_specular float32 (L, H, W, 3), what each of the scene's L lights adds to them, one image per light; light_open int32
        (L, H, W), how many of the light's shadow rays arrive (0 / 1; up to its number of samples for an area light).  Contiguous, on
        this scene's device.  Written: the pixels x < W-1, y < H-1 of rows [r0, r1) that this part owns; nothing else of a tensor is
        touched.  A miss: zeros.  Asynchronous on `stream` (None: torch's current stream of the scene's device); with a
        torch.cuda.Stream the tensors are recorded on it."""
        import torch
        hw, nl = (self.height, self.width), self.n_lights
        given = (("diffuse", diffuse, torch.float32, hw + (3,)), ("specular", specular, torch.float32, hw + (3,)),
                 ("light_diffuse", light_diffuse, torch.float32, (nl,) + hw + (3,)), ("light_specular", light_specular, torch.float32, (nl,) + hw + (3,)),
                 ("light_open", light_open, torch.int32, (nl,) + hw))
        st, ptrs = _frame_tensors("render_light", given, self.device, stream)
        r0, r1 = rows if rows is not None else (0, self.height)
        _check(self.rtx.rtx_render_light(self.gpu(), r0, r1, C.byref(FrameLightBuffers(nl, *ptrs)), st), "rtx_render_light")

    def device_mesh(self, mesh):
        """The device's current tree of mesh `mesh` (index among the meshes) in the layout of bvh(): bounds, skip, leaf_begin, leaf_count,
        refs (rtx_scene_mesh_read)."""
        g = self.gpu()
        cnt = np.zeros(2, np.uint32)
        _check(self.rtx.rtx_scene_mesh_read(g, mesh, _np_ptr(cnt), None, None, None, None, None), "rtx_scene_mesh_read")
        nn, nr = int(cnt[0]), int(cnt[1])
        d = dict(bounds=np.zeros((nn, 6), np.float32), skip=np.zeros(nn, np.int32), leaf_begin=np.zeros(nn, np.int32),
                 leaf_count=np.zeros(nn, np.int32), refs=np.zeros(nr, np.uint32))
        _check(self.rtx.rtx_scene_mesh_read(g, mesh, _np_ptr(cnt), _np_ptr(d["bounds"]), _np_ptr(d["skip"]), _np_ptr(d["leaf_begin"]),
                                            _np_ptr(d["leaf_count"]), _np_ptr(d["refs"])), "rtx_scene_mesh_read")
        return d

    def device_mesh_flat(self, mesh):
        """(wide, box records, plane records, root record) of mesh `mesh` as the device holds them, in mesh_flatten_probe's layout
        (rtx_scene_mesh_flat_read)."""
        g = self.gpu()
        n = C.c_uint32(0)
        root = np.zeros(8, np.float32)
        _check(self.rtx.rtx_scene_mesh_flat_read(g, mesh, C.byref(n), None, None, 0, _np_ptr(root)), "rtx_scene_mesh_flat_read")
        S = int(self.rtx.rtx_wide_node_slots())
        wide = np.zeros((n.value, S, 8), np.float32); prune = np.zeros((n.value, 2 * S, 8), np.float32)
        _check(self.rtx.rtx_scene_mesh_flat_read(g, mesh, C.byref(n), _np_ptr(wide), _np_ptr(prune), n.value, _np_ptr(root)), "rtx_scene_mesh_flat_read")
        return wide, prune[:, 0:S], prune[:, S:2 * S], root

    def device_lights(self):
        """The lights as the device holds them (rtx_scene_lights_read): (records, points) -- a structured array with the fields of
        rtx_light but the pointer (type, color, intensity, dir, pos, n_points) and the area lights' sample points one after the other,
        float32 (n, 3)."""
        g = self.gpu()
        n, nf = C.c_uint32(0), C.c_size_t(0)
        _check(self.rtx.rtx_scene_lights_read(g, C.byref(n), None, 0, C.byref(nf), None, 0), "rtx_scene_lights_read")
        raw = (RtxLight * max(n.value, 1))()
        pts = np.zeros(nf.value, np.float32)
        _check(self.rtx.rtx_scene_lights_read(g, C.byref(n), raw, n.value, C.byref(nf), _np_ptr(pts), pts.size), "rtx_scene_lights_read")
        recs = np.zeros(n.value, [("type", np.int32), ("color", np.float32, 3), ("intensity", np.float32), ("dir", np.float32, 3),
                                  ("pos", np.float32, 3), ("n_points", np.uint32)])
        for i in range(n.value):
            recs[i] = (raw[i].type, tuple(raw[i].color), raw[i].intensity, tuple(raw[i].dir), tuple(raw[i].pos), raw[i].n_points)
        return recs, pts.reshape(-1, 3)

    def device_objects(self):
        """The objects as the device holds them (rtx_scene_objects_read): (records, n_meshes) -- a structured array with the fields of
        rtx_object (type, material, pos, color, ior, ambient, diffuse, specular, n_specular, radius2, normal, mesh), decoded from the
        device's records, and the number of meshes."""
        g = self.gpu()
        n, nm = C.c_uint32(0), C.c_uint32(0)
        _check(self.rtx.rtx_scene_objects_read(g, C.byref(n), None, 0, C.byref(nm)), "rtx_scene_objects_read")
        raw = (RtxObject * max(n.value, 1))()
        _check(self.rtx.rtx_scene_objects_read(g, C.byref(n), raw, n.value, C.byref(nm)), "rtx_scene_objects_read")
        recs = np.zeros(n.value, [("type", np.int32), ("material", np.int32), ("pos", np.float32, 3), ("color", np.float32, 3), ("ior", np.float32),
                                  ("ambient", np.float32), ("diffuse", np.float32), ("specular", np.float32), ("n_specular", np.float32),
                                  ("radius2", np.float32), ("normal", np.float32, 3), ("mesh", np.int32)])
        for i in range(n.value):
            r = raw[i]
            recs[i] = (r.type, r.material, tuple(r.pos), tuple(r.color), r.ior, r.ambient, r.diffuse, r.specular, r.n_specular, r.radius2,
                       tuple(r.normal), r.mesh)
        return recs, nm.value

    def device_prune_copies(self, mesh):
        """Every copy of mesh `mesh`'s prune blocks as the device holds them (rtx_scene_mesh_prune_copy_read): float32 (copies, n_wide, 2 S, 8)
        -- copy 0 the one any ray uses, 1 the camera's, 2 + l point light l's; S = rtx_wide_node_slots()."""
        g = self.gpu()
        nc, nw = C.c_uint32(0), C.c_uint32(0)
        _check(self.rtx.rtx_scene_mesh_prune_copy_read(g, mesh, 0, C.byref(nc), C.byref(nw), None, 0), "rtx_scene_mesh_prune_copy_read")
        S = int(self.rtx.rtx_wide_node_slots())
        out = np.zeros((nc.value, nw.value, 2 * S, 8), np.float32)
        for c in range(nc.value):
            _check(self.rtx.rtx_scene_mesh_prune_copy_read(g, mesh, c, C.byref(nc), C.byref(nw), _np_ptr(out[c]), nw.value), "rtx_scene_mesh_prune_copy_read")
        return out

    def edit_times(self):
        """Host wall ms of the last rtx_scene_update_mesh: {build, flatten (on the device, records swapped in), sources + estimate queued,
        whole call} (rtx_scene_edit_times)."""
        ms = np.zeros(4, np.float32)
        _check(self.rtx.rtx_scene_edit_times(self.gpu(), _np_ptr(ms)), "rtx_scene_edit_times")
        return dict(zip(("build", "flatten", "prepare", "total"), (float(x) for x in ms)))

    def move_times(self):
        """Host wall ms of the last move_object: {place (the loader's placement), upload (the triangles), set_object, update_mesh}."""
        ms = np.zeros(4, np.float32)
        self.host.rah_object_move_times(self.h, _np_ptr(ms))
        return dict(zip(("place", "upload", "set_object", "update_mesh"), (float(x) for x in ms)))

    # ---- deforming a mesh (include/rtx_deform.h) ------------------------------------------------
    def _mesh_counts(self, who, index):
        if not 0 <= index < self.n_objects:
            raise ValueError("%s: object index %d out of range (%d objects)" % (who, index, self.n_objects))
        c = np.zeros(8, np.int64)
        if self.host.rah_mesh_counts(self.h, index, _np_ptr(c)) != 0:
            raise ValueError("%s: object %d is not a mesh" % (who, index))
        return dict(zip(("n_tris", "n_pos", "n_nrm", "n_uv", "placed_pos", "placed_nrm", "has_faces"), (int(x) for x in c)))

    def mesh_vertices(self, index):
        """(P, N) of mesh `index` (scene-file order of the objects) as stored: the vertices of its OBJ file, float32 (n_pos, 3), and its
        normals, normalised as the loader normalises them, float32 (n_nrm, 3)."""
        c = self._mesh_counts("mesh_vertices", index)
        P, N = np.zeros((c["n_pos"], 3), np.float32), np.zeros((c["n_nrm"], 3), np.float32)
        self.host.rah_mesh_vertices(self.h, index, _np_ptr(P), _np_ptr(N))
        return P, N

    def mesh_topology(self, index):
        """What the loader kept of mesh `index`'s faces: corner_pos uint32 (n_tris, 3), corner_nrm and corner_uv int32 (n_tris, 3) with -1 in
        column 0 where the face gave none, uv float32 (n_uv, 2), and placed_pos / placed_nrm: how many vertices / normals were read before
        the first face (only those are placed / rotated, as in the reference)."""
        c = self._mesh_counts("mesh_topology", index)
        d = dict(corner_pos=np.zeros((c["n_tris"], 3), np.uint32), corner_nrm=np.zeros((c["n_tris"], 3), np.int32),
                 corner_uv=np.zeros((c["n_tris"], 3), np.int32), uv=np.zeros((c["n_uv"], 2), np.float32))
        self.host.rah_mesh_topology(self.h, index, _np_ptr(d["corner_pos"]), _np_ptr(d["corner_nrm"]), _np_ptr(d["corner_uv"]), _np_ptr(d["uv"]))
        d.update(placed_pos=c["placed_pos"], placed_nrm=c["placed_nrm"])
        return d

    def mesh_pose(self, index):
        """pos, rot (degrees), size of mesh `index` and the scene's bias and ac_penalty: what its vertices are placed with."""
        self._mesh_counts("mesh_pose", index)
        pos, rot, size = (np.zeros(3, np.float32) for _ in range(3))
        bias, pen = C.c_float(0), C.c_int(0)
        self.host.rah_mesh_pose(self.h, index, _np_ptr(pos), _np_ptr(rot), _np_ptr(size), C.byref(bias), C.byref(pen))
        return dict(pos=pos, rot=rot, size=size, bias=np.float32(bias.value), ac_penalty=pen.value)

    def set_vertices(self, index, vertices, normals=None, stream=None):
        """Gives mesh `index` new vertices, float32 (n_pos, 3) in its OBJ file's order and space, and with `normals` new raw normals, float32
        (n_nrm, 3) (None keeps the stored ones): afterwards the scene is, bit for bit, a fresh load of the scene whose mesh reads an OBJ file
        with these v (and vn) lines.  A torch tensor on the scene's device is used in place -- with a live GPU scene the device places the
        vertices, assembles the triangles and rebuilds the structure (rtx_scene_deform_mesh), and no triangle crosses the bus; the call waits
        for `stream` (None: torch's current stream), on which the tensors were produced.  A numpy array or a CPU tensor is uploaded as
        vertices.  ValueError: a bad index, an object that is not a mesh, a wrong shape, dtype or device; RtxError: a refusal of the library
        (a value that is not finite, a placed position that is not finite) -- the scene is then as it was."""
        c = self._mesh_counts("set_vertices", index)
        keep = []

        def arg(name, a, rows):
            if a is None:
                return None, False
            on_device = False
            if isinstance(a, np.ndarray):
                if a.dtype != np.float32:
                    raise ValueError("set_vertices: %s must be float32, got %s" % (name, a.dtype))
                shape = a.shape
            else:
                import torch
                if not isinstance(a, torch.Tensor):
                    raise ValueError("set_vertices: %s must be a numpy array or a torch tensor, got %s" % (name, type(a).__name__))
                if a.dtype != torch.float32:
                    raise ValueError("set_vertices: %s must be float32, got %s" % (name, a.dtype))
                shape = tuple(a.shape)
                if a.device.type == "cuda":
                    if (a.device.index if a.device.index is not None else torch.cuda.current_device()) != self.device:
                        raise ValueError("set_vertices: %s must be on cuda:%d, the scene's device, or on the host, got %s" % (name, self.device, a.device))
                    on_device = True
                elif a.device.type != "cpu":
                    raise ValueError("set_vertices: %s must be on cuda:%d or on the host, got %s" % (name, self.device, a.device))
            if len(shape) != 2 or shape[1] != 3 or shape[0] != rows:
                raise ValueError("set_vertices: %s must have shape (%d, 3), got %s" % (name, rows, tuple(shape)))
            if on_device:
                a = a.contiguous()
                keep.append(a)
                return C.c_void_p(a.data_ptr()), True
            a = np.ascontiguousarray(a if isinstance(a, np.ndarray) else a.numpy())
            keep.append(a)
            return _np_ptr(a), False

        p, p_dev = arg("vertices", vertices, c["n_pos"])
        if p is None:
            raise ValueError("set_vertices: vertices is None")
        n, n_dev = arg("normals", normals, c["n_nrm"])
        if normals is not None and n_dev != p_dev:
            raise ValueError("set_vertices: vertices and normals must both be on the device or both on the host")
        st = None
        if p_dev:
            import torch
            st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream) if stream is None else self._stream_ptr(stream)
        if self.host.rah_mesh_set_vertices(self.h, index, p, c["n_pos"], n, c["n_nrm"] if normals is not None else 0, int(p_dev), st) != 0:
            raise RtxError("set_vertices: %s" % self.host.rah_last_error().decode(errors="replace"))

    # ---- texture maps and skybox (include/rtx_texture.h) -----------------------------------------
    def has_gpu(self):
        """True once the scene has been uploaded (gpu(), or any render or query); until then edits change the host's scene alone."""
        return bool(self.host.rah_scene_has_gpu(self.h))

    def _texels(self, who, kind, image, top_down):
        """(RtxTexels, in device memory?, what keeps the data alive) of `image` for a map of `kind`: uint8 (H, W, 3) is RGB8, float32 (H, W, 3)
        -- (H, W) for "specular" -- the stored texels; numpy or torch.  A tensor on the scene's device is used in place while the scene is
        uploaded; anything else is handed over in host memory.  top_down: row 0 of `image` is the map's last row."""
        a = image
        on_device = False
        if not isinstance(a, np.ndarray):
            try:
                import torch
            except Exception:
                torch = None
            if torch is None or not isinstance(a, torch.Tensor):
                raise ValueError("%s: image must be a numpy array or a torch tensor, got %s" % (who, type(a).__name__))
            if a.dtype not in (torch.uint8, torch.float32):
                raise ValueError("%s: image must be uint8 or float32, got %s" % (who, a.dtype))
            if a.device.type == "cuda":
                if (a.device.index if a.device.index is not None else torch.cuda.current_device()) != self.device:
                    raise ValueError("%s: image must be on cuda:%d, the scene's device, or on the host, got %s" % (who, self.device, a.device))
                on_device = True
            elif a.device.type != "cpu":
                raise ValueError("%s: image must be on cuda:%d or on the host, got %s" % (who, self.device, a.device))
            rgb8 = a.dtype == torch.uint8
        else:
            if a.dtype not in (np.uint8, np.float32):
                raise ValueError("%s: image must be uint8 or float32, got %s" % (who, a.dtype))
            rgb8 = a.dtype == np.uint8
        shape = tuple(a.shape)
        want = (2,) if (kind == "specular" and not rgb8) else (3,)
        if len(shape) not in want or (len(shape) == 3 and shape[2] != 3):
            raise ValueError("%s: a %s %s image must have shape %s, got %s" % (who, "uint8" if rgb8 else "float32", kind,
                                                                                 "(H, W)" if want == (2,) else "(H, W, 3)", shape))
        if on_device and not self.has_gpu():
            a, on_device = a.cpu(), False
        # (rows that are packed go over as they lie, whatever the step from row to row: a view of a wider image, a flipped one)
        h, w = shape[0], shape[1]
        item = 1 if rgb8 else 4
        row = w * item * (3 if len(shape) == 3 else 1)
        if on_device:
            strides = tuple(s * item for s in a.stride())
        else:
            a = a if isinstance(a, np.ndarray) else a.numpy()
            strides = a.strides
        packed = h > 0 and w > 0 and strides[1:] == ((3 * item, item) if len(shape) == 3 else (item,)) and (h == 1 or abs(strides[0]) >= row)
        if not packed:
            a = a.contiguous() if on_device else np.ascontiguousarray(a)
        pitch = strides[0] if packed and h > 1 else row
        base = a.data_ptr() if on_device else a.ctypes.data
        if top_down and h:
            base, pitch = base + (h - 1) * pitch, -pitch
        return RtxTexels(TEXELS_RGB8 if rgb8 else TEXELS_STORED, w, h, base, pitch), on_device, a

    def _texel_stream(self, stream, on_device, keep):
        """The stream pointer of a texture edit: `stream`, else torch's current stream of the scene's device while the scene is uploaded."""
        if not self.has_gpu():
            return None
        import torch
        if isinstance(stream, torch.cuda.Stream) and on_device:
            keep.record_stream(stream)
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream) if stream is None else self._stream_ptr(stream)

    @staticmethod
    def _map_kind(who, kind):
        if kind not in ("diffuse", "normal", "specular"):
            raise ValueError("%s: unknown kind %r (diffuse, normal, specular)" % (who, kind))
        return TEXTURE_KINDS[kind]

    def set_texture(self, index, kind, image, top_down=False, stream=None):
        """Replaces map `kind` ("diffuse", "normal", "specular") of mesh `index` (scene-file order of the objects) as a whole: afterwards the
        scene is, bit for bit, a fresh load of the scene file whose mesh names an image file holding `image`.  image: uint8 (H, W, 3) -- R G B
        as a BMP holds them, decoded with the loader's arithmetic --, or float32 (H, W, 3), (H, W) for "specular": the texels as the scene stores
        them (texture()); numpy or torch, any size; None removes the map.  Row 0 is the first stored row, the bottom row of a BMP;
        top_down=True hands the image in from its last row.  A tensor on the scene's device is decoded on the device in place
        (rtx_scene_set_map; the call waits for `stream`, None: torch's current stream).  ValueError: a bad index, an object that is not a mesh,
        a wrong dtype, shape or device; RtxError: a refusal of the library (a normal map for a mesh without texture coordinates) -- the
        scene is then as it was."""
        self._mesh_counts("set_texture", index)
        k = self._map_kind("set_texture", kind)
        if image is None:
            t, on_device, keep = None, False, None
        else:
            t, on_device, keep = self._texels("set_texture", kind, image, top_down)
        st = self._texel_stream(stream, on_device, keep) if on_device else None
        if self.host.rah_mesh_set_map(self.h, index, k, C.byref(t) if t is not None else None, int(on_device), st) != 0:
            raise RtxError("set_texture: %s" % self.host.rah_last_error().decode(errors="replace"))

    def write_texture(self, index, kind, image, x0=0, y0=0, top_down=False, stream=None):
        """Writes `image` (as for set_texture) into map `kind` of mesh `index` at texel (x0, y0) -- the rectangle must lie inside the map, texels
        outside it keep their bits.  With an uploaded scene the write is queued on `stream` (None: torch's current stream) and the host does
        not wait (rtx_scene_write_texels): renders queued on that stream before it see the old texels, later ones the new; a tensor on the
        device must stay as it is until the stream has passed the write.  This is the per-frame path of a video texture."""
        self._mesh_counts("write_texture", index)
        k = self._map_kind("write_texture", kind)
        self._write_texels("write_texture", k, kind, index, image, x0, y0, top_down, stream)

    def _write_texels(self, who, k, kind, index, image, x0, y0, top_down, stream):
        if image is None:
            raise ValueError("%s: image is None" % who)
        if int(x0) < 0 or int(y0) < 0:
            raise ValueError("%s: x0 and y0 must not be negative, got %d, %d" % (who, x0, y0))
        t, on_device, keep = self._texels(who, kind, image, top_down)
        st = self._texel_stream(stream, on_device, keep)
        if self.host.rah_write_texels(self.h, k, index, int(x0), int(y0), C.byref(t), int(on_device), st) != 0:
            raise RtxError("%s: %s" % (who, self.host.rah_last_error().decode(errors="replace")))

    def set_skybox(self, faces, top_down=False, stream=None):
        """Replaces the six skybox faces (the order of the scene file's skyboxes= line) by six images of one size and one format, as for
        set_texture's "diffuse"; None: the scene loses its skybox (refused while useSkybox is on).  A scene without a skybox gains one;
        set_flag("useSkybox", 1) then shows it."""
        if faces is None:
            ts, on_device, keep = None, False, []
        else:
            faces = list(faces)
            if len(faces) != 6:
                raise ValueError("set_skybox: six faces are needed, got %d" % len(faces))
            parts = [self._texels("set_skybox", "sky", f, top_down) for f in faces]
            if len({p[1] for p in parts}) != 1:
                raise ValueError("set_skybox: the six faces must all be on the device or all on the host")
            if len({(p[0].format, p[0].width, p[0].height) for p in parts}) != 1:
                raise ValueError("set_skybox: the six faces must share one size and one dtype")
            ts, on_device, keep = (RtxTexels * 6)(*[p[0] for p in parts]), parts[0][1], [p[2] for p in parts]
        st = None
        if on_device:
            for a in keep:
                st = self._texel_stream(stream, on_device, a)
        if self.host.rah_scene_set_sky(self.h, ts, int(on_device), st) != 0:
            raise RtxError("set_skybox: %s" % self.host.rah_last_error().decode(errors="replace"))

    def write_skybox(self, face, image, x0=0, y0=0, top_down=False, stream=None):
        """write_texture for skybox face `face` (0..5)."""
        if not 0 <= int(face) < 6:
            raise ValueError("write_skybox: face %d out of range (0..5)" % face)
        self._write_texels("write_skybox", TEXTURE_KINDS["sky"], "sky", int(face), image, x0, y0, top_down, stream)

    def _texture(self, who, k, index, host=False):
        w, h = C.c_int(0), C.c_int(0)
        live = self.has_gpu() and not host
        st = self._texel_stream(None, False, None)
        # (with an uploaded scene the size is the device's; a queued write changes no size)
        if self.host.rah_texture(self.h, k, index, C.byref(w), C.byref(h), None, 0, None) != 0:
            raise RtxError("%s: %s" % (who, self.host.rah_last_error().decode(errors="replace")))
        if not w.value or not h.value:
            return None
        shape = (h.value, w.value) if k == TEXTURE_KINDS["specular"] else (h.value, w.value, 3)
        if live:
            import torch
            out = torch.empty(shape, dtype=torch.float32, device="cuda:%d" % self.device)
            rc = self.host.rah_texture(self.h, k, index, C.byref(w), C.byref(h), C.c_void_p(out.data_ptr()), 1, st)
        else:
            out = np.zeros(shape, np.float32)
            rc = self.host.rah_texture(self.h, k, index, C.byref(w), C.byref(h), _np_ptr(out), 0, None)
        if rc != 0:
            raise RtxError("%s: %s" % (who, self.host.rah_last_error().decode(errors="replace")))
        return out

    def texture(self, index, kind, host=False):
        """A float32 copy of map `kind` of mesh `index` as the scene stores it, (H, W, 3) -- (H, W) for "specular" --, row 0 the first stored
        row: a tensor on the scene's device once the scene is uploaded (copied on torch's current stream, after the writes queued on it),
        else a numpy array; None where the mesh has no such map.  host=True: always a numpy array, from the host's own copy of the map --
        the one a later upload starts from --, which is first read back from the device where a write_texture has left it behind."""
        self._mesh_counts("texture", index)
        return self._texture("texture", self._map_kind("texture", kind), index, host)

    def skybox_face(self, k, host=False):
        """texture() for skybox face k (0..5); None for a scene without a skybox."""
        if not 0 <= int(k) < 6:
            raise ValueError("skybox_face: face %d out of range (0..5)" % k)
        return self._texture("skybox_face", TEXTURE_KINDS["sky"], int(k), host)

    # ---- texel points of a mesh's UV layout (include/rtx_bake.h) ---------------------------------
    def _bake_size(self, who, index, width, height):
        """(device mesh index, w, h) of a map over mesh `index`: the given size, else the size of the mesh's diffuse map."""
        self._mesh_counts(who, index)
        if (width is None) != (height is None):
            raise ValueError("%s: width and height go together" % who)
        if width is None:
            w, h = C.c_int(0), C.c_int(0)
            if self.host.rah_texture(self.h, TEXTURE_KINDS["diffuse"], index, C.byref(w), C.byref(h), None, 0, None) != 0:
                raise RtxError("%s: %s" % (who, self.host.rah_last_error().decode(errors="replace")))
            if not w.value or not h.value:
                raise ValueError("%s: object %d has no diffuse map, and no size is given" % (who, index))
            width, height = w.value, h.value
        width, height = int(width), int(height)
        if width < 1 or height < 1 or width * height > 0x7fffffff:
            raise ValueError("%s: width and height must be positive, their product at most %d, got %d x %d" % (who, 0x7fffffff, width, height))
        # (the device's meshes are the mesh objects in scene order)
        mesh = sum(1 for i in range(index) if self.host.rah_object_type(self.h, i) == OBJECT_TYPES["mesh"])
        return mesh, width, height

    def texel_points(self, index, width=None, height=None, points=True, tri=True, bary=False, stream=None):
        """rtx_texel_points: the surface point of every texel of a width x height map laid over mesh `index` (scene-file order of the objects,
        as in set_texture) by its texture coordinates, on the device (include/rtx_bake.h: texel (i, j) covers the centre
        ((i + .5) / width, (j + .5) / height); the lowest triangle index owns a shared texel).  The size defaults to the mesh's diffuse map.
        Returns a dict of the channels asked for, new tensors on the scene's device: "points" float32 (height * width, 6) = {P xyz, N xyz},
        what light_points, ao_points and radiance_points take; "tri" int32 (height, width), the owning triangle, -1 where no triangle covers
        the centre (its point is all +0); "bary" float32 (height, width, 2).  Row 0 is the map's first stored row: an image computed from
        the points goes into set_texture as it is.  Asynchronous on `stream`, which is handled as in trace_rays."""
        import torch
        if not (points or tri or bary):
            raise ValueError("texel_points: nothing to compute (every channel is off)")
        mesh, w, h = self._bake_size("texel_points", index, width, height)
        g = self.gpu()
        dev = torch.device("cuda", self.device)
        alloc_on, st = _query_stream(stream, dev, ())
        with torch.cuda.stream(alloc_on):
            out = {}
            if points:
                out["points"] = torch.empty((h * w, 6), dtype=torch.float32, device=dev)
            if tri:
                out["tri"] = torch.empty((h, w), dtype=torch.int32, device=dev)
            if bary:
                out["bary"] = torch.empty((h, w, 2), dtype=torch.float32, device=dev)
        buf = TexelBuffers(*[out[k].data_ptr() if k in out else None for k in ("points", "tri", "bary")])
        _check(self.rtx.rtx_texel_points(g, mesh, w, h, C.byref(buf), st), "rtx_texel_points")
        return out

    def dilate_texels(self, image, tri, passes=1, stream=None):
        """rtx_dilate_texels: the margin around the charts, in place.  image: contiguous float32 tensor (H, W) or (H, W, C), C in 1 .. 4, on the
        scene's device; tri: int32 (H, W) as texel_points returns it.  Per pass every texel with tri == -1 copies the first neighbour (left,
        right, below, above, then the diagonals) that was covered or filled at the start of the pass, and becomes -2.  Returns `image`."""
        import torch
        _check_tensor("dilate_texels", "tri", tri, torch.int32, ("H", "W"), self.device)
        h, w = tri.shape
        if image is not None and isinstance(image, torch.Tensor) and image.dim() == 2:
            _check_tensor("dilate_texels", "image", image, torch.float32, (h, w), self.device)
            ch = 1
        else:
            _check_tensor("dilate_texels", "image", image, torch.float32, (h, w, "C"), self.device)
            ch = image.shape[2]
        if not 1 <= ch <= 4:
            raise ValueError("dilate_texels: image must have 1 .. 4 channels, got %d" % ch)
        if int(passes) < 0:
            raise ValueError("dilate_texels: passes must not be negative, got %d" % passes)
        _, st = _query_stream(stream, image.device, (image, tri))
        if h and w and int(passes):
            _check(self.rtx.rtx_dilate_texels(self.gpu(), w, h, ch, _ptr(image), _ptr(tri), int(passes), st), "rtx_dilate_texels")
        return image

    def bake_light(self, index, width=None, height=None, margin=2, stream=None):
        """A lightmap of mesh `index`: light_points(texel_points(...)["points"], diffuse=True) as an image (height, width, 3), dilated
        `margin` passes.  Returns (image, tri); set_texture(index, "diffuse", image) takes the image as it is."""
        t = self.texel_points(index, width, height, points=True, tri=True, stream=stream)
        h, w = t["tri"].shape
        image = self.light_points(t["points"], diffuse=True, stream=stream)["diffuse"].reshape(h, w, 3)
        return self.dilate_texels(image, t["tri"], margin, stream=stream), t["tri"]

    # ---- surface points projected into cameras (include/rtx_project.h) -------------------------------
    def camera_table(self, cameras, width=None, height=None):
        """The camera records of project_points: a float32 tensor (K, 24) on the scene's device, one record per camera of `cameras` --
        render_views' sequence of (pos, rot) or (pos, rot, fov), K in 1 .. 256 -- at the size width x height (one size for all; the default
        is the scene's): {cam_pos, scale, aspect, width, height, 0, cam_matrix}, the fields view_target(pos, rot, fov, width, height) holds
        (rah_view_target), so the renderer's own camera and not a restatement of it.  The scene is not changed."""
        import torch
        return torch.from_numpy(self._camera_records(cameras, width, height)).to(torch.device("cuda", self.device))

    def _camera_records(self, cameras, width=None, height=None):
        """camera_table's records as a numpy array float32 (K, 24).  Host only."""
        cameras = list(cameras)
        if not 1 <= len(cameras) <= 256:
            raise ValueError("camera_table: 1 .. 256 cameras, got %d" % len(cameras))
        w, h = self.width if width is None else int(width), self.height if height is None else int(height)
        if w < 1 or h < 1:
            raise ValueError("camera_table: width and height must be positive, got %d x %d" % (w, h))
        table = np.zeros((len(cameras), PROJECT_CAMERA_FLOATS), np.float32)
        t = ViewTarget()
        for i, cam in enumerate(cameras):
            if len(cam) not in (2, 3):
                raise ValueError("camera_table: camera %d must be (pos, rot) or (pos, rot, fov)" % i)
            self._fill_view_target(t, cam[0], cam[1], cam[2] if len(cam) == 3 else None, w, h)
            table[i, 0:3] = t.cam_pos
            table[i, 3:7] = (t.scale, t.aspect, t.width, t.height)
            table[i, 8:24] = t.cam_matrix
        return table

    def project_points(self, points, cameras, width=None, height=None, pixel=True, depth=False, flags=True, visibility=True, stream=None):
        """rtx_project_points: which pixel of each camera a surface point falls into, and whether that camera sees it, on the device
        (include/rtx_project.h).  points: as for light_points, (n, 6) = {P xyz, N xyz}.  cameras: render_views' sequence of (pos, rot[, fov])
        at the size width x height (camera_table), or a table tensor float32 (K, 24) on the scene's device, which is used in place (width
        and height must then be None); K in 1 .. 256.  Returns a dict of the channels asked for, new tensors on the points' device,
        camera-major: "pixel" float32 (K, n, 2) = (px, py), an integer meaning the centre of that pixel of pass 1 -- the nearest pixel is
        floor(p + 0.5); "depth" float32 (K, n), the distance from the camera's position; "flags" uint8 (K, n) of PROJ_FRONT | PROJ_INSIDE |
        PROJ_FACING | PROJ_OPEN.  PROJ_OPEN -- the shadow ray from P + N * bias to the camera meets no opaque object, occluded()'s rule
        -- is only computed with `visibility`, and only for the pairs that are in front of the camera and inside its frame.
        Asynchronous on `stream`, which is handled as in trace_rays (a table tensor is recorded on it like the points)."""
        import torch
        if not (pixel or depth or flags):
            raise ValueError("project_points: nothing to compute (every channel is off)")
        n = _check_rays("project_points", points, self.device, "points")
        if isinstance(cameras, torch.Tensor):
            if width is not None or height is not None:
                raise ValueError("project_points: a camera table has its sizes in it (width and height must be None)")
            _check_tensor("project_points", "cameras", cameras, torch.float32, ("K", PROJECT_CAMERA_FLOATS), self.device)
            table = cameras
        else:
            # (the upload is queued where the call will run)
            with torch.cuda.stream(stream if isinstance(stream, torch.cuda.Stream) else None):
                table = self.camera_table(cameras, width, height)
            if stream is not None and not isinstance(stream, torch.cuda.Stream):
                torch.cuda.current_stream(points.device).synchronize()      # (a raw handle: torch cannot order the upload before it)
        k = table.shape[0]
        if not 1 <= k <= 256:
            raise ValueError("project_points: 1 .. 256 cameras, got %d" % k)
        alloc_on, st = _query_stream(stream, points.device, (points, table))
        with torch.cuda.stream(alloc_on):
            out = {}
            if pixel:
                out["pixel"] = torch.empty((k, n, 2), dtype=torch.float32, device=points.device)
            if depth:
                out["depth"] = torch.empty((k, n), dtype=torch.float32, device=points.device)
            if flags:
                out["flags"] = torch.empty((k, n), dtype=torch.uint8, device=points.device)
        if n:
            buf = ProjectBuffers(*[out[c].data_ptr() if c in out else None for c in ("pixel", "depth", "flags")])
            _check(self.rtx.rtx_project_points(self.gpu(), n, _ptr(points), k, _ptr(table), 1 if visibility else 0, C.byref(buf), st),
                   "rtx_project_points")
        return out

    def bake_view(self, index, camera, image, width=None, height=None, margin=2, stream=None):
        """The projective bake of one view onto mesh `index`: texel_points(index, width, height), projected with project_points into
        `camera` = (pos, rot[, fov]) at the size of `image` -- float32 (H, W, 3) on the scene's device, in the row order of render_views'
        framebuffers.  A texel whose flags are PROJ_INSIDE | PROJ_FACING | PROJ_OPEN (so PROJ_FRONT too) takes
        image[floor(py + 0.5), floor(px + 0.5)], every other covered texel is 0; then dilate_texels over `margin` passes.  Returns
        (texels, seen): float32 (height, width, 3), which set_texture(index, "diffuse", texels) takes as it is, and bool (height, width),
        the texels that took a pixel.  Several cameras are merged by the caller: torch.where(seen_b[..., None] & ~seen_a[..., None], b, a).
        `stream` is handled as in trace_rays; with a raw hipStream_t handle the host waits for the device around the gather, which is torch's."""
        import torch
        _check_tensor("bake_view", "image", image, torch.float32, ("H", "W", 3), self.device)
        ih, iw = int(image.shape[0]), int(image.shape[1])
        if ih < 1 or iw < 1:
            raise ValueError("bake_view: image is empty")
        if len(camera) not in (2, 3):
            raise ValueError("bake_view: camera must be (pos, rot) or (pos, rot, fov)")
        t = self.texel_points(index, width, height, points=True, tri=True, stream=stream)
        h, w = t["tri"].shape
        p = self.project_points(t["points"], [camera], iw, ih, pixel=True, flags=True, visibility=True, stream=stream)
        alloc_on, _ = _query_stream(stream, image.device, (image,))
        # (a raw hipStream_t handle: torch cannot order its own work between the calls queued on it, so the host waits on either side)
        raw = stream is not None and alloc_on is None
        if raw:
            torch.cuda.synchronize(image.device)
        with torch.cuda.stream(alloc_on):
            want = PROJ_FRONT | PROJ_INSIDE | PROJ_FACING | PROJ_OPEN
            seen = ((p["flags"][0] & want) == want).reshape(h, w) & (t["tri"] >= 0)
            # (INSIDE: the nearest pixel is inside the image; the clamp only keeps the texels that are not seen from indexing outside it)
            near = torch.floor(p["pixel"][0] + 0.5).nan_to_num(0.0, 0.0, 0.0)
            x = near[:, 0].clamp(0, iw - 1).long().reshape(h, w)
            y = near[:, 1].clamp(0, ih - 1).long().reshape(h, w)
            texels = torch.where(seen[..., None], image[y, x], torch.zeros((), dtype=torch.float32, device=image.device)).contiguous()
        if raw:
            torch.cuda.current_stream(image.device).synchronize()
        return self.dilate_texels(texels, t["tri"], margin, stream=stream), seen

    def deform_times(self):
        """Host wall ms of the stages of the last set_vertices: {kernels (placement and assembly on the device with their read-backs),
        rebuild (rtx_scene_update_mesh: edit_times), mirror (the host's copy of the vertices), total}."""
        ms = np.zeros(4, np.float32)
        self.host.rah_mesh_deform_times(self.h, _np_ptr(ms))
        return dict(zip(("kernels", "rebuild", "mirror", "total"), (float(x) for x in ms)))

    def counters_enable(self, on=True):
        _check(self.rtx.rtx_counters_enable(self.gpu(), int(on)), "rtx_counters_enable")

    def counters_reset(self):
        _check(self.rtx.rtx_counters_reset(self.gpu()), "rtx_counters_reset")

    def counters(self):
        c = Counters()
        _check(self.rtx.rtx_counters_read(self.gpu(), C.byref(c)), "rtx_counters_read")
        self.moot_rays = int(c.moot_rays)      # shadow rays that cannot influence the pixel (only the instrumented variant traces them)
        return np.array([c.rays, c.box_tests, c.tri_tests], np.int64)

    def scene_bytes(self):
        n = C.c_size_t(0)
        _check(self.rtx.rtx_scene_bytes(self.gpu(), C.byref(n)), "rtx_scene_bytes")
        return n.value

    def last_kernel_ms(self, which=0):
        ms = C.c_float(0)
        _check(self.rtx.rtx_last_kernel_ms(self.gpu(), which, C.byref(ms)), "rtx_last_kernel_ms")
        return ms.value

    def kernel_time_reset(self):
        _check(self.rtx.rtx_kernel_time_reset(self.gpu()), "rtx_kernel_time_reset")

    def kernel_time_stats(self, which=0):
        """(launches, total_ms) of kernel `which` (0 pass 1, 1 sobel, 2 ssaa, 3 whole frame) since kernel_time_reset()."""
        n, ms = C.c_uint32(0), C.c_double(0)
        _check(self.rtx.rtx_kernel_time_stats(self.gpu(), which, C.byref(n), C.byref(ms)), "rtx_kernel_time_stats")
        return n.value, ms.value

    def tile_cost(self):
        """(ceil(H/8), ceil(W/8)) uint32 array: 100 MHz ticks pass 1 spent on each 8x8 tile (rtx_tile_cost_read)."""
        self._dims()
        out = np.zeros(((self.height + 7) // 8, (self.width + 7) // 8), np.uint32)
        _check(self.rtx.rtx_tile_cost_read(self.gpu(), _np_ptr(out), out.size), "rtx_tile_cost_read")
        return out

    def ssaa_item_cost(self):
        """(ceil(H/8), ceil(W/8)) uint32 array: per tile, the slowest SSAA work item of the most recent render_ssaa in
        100 MHz ticks, scaled to a 16-pixel item (0 = the tile had no flagged pixel); the second half of rtx_tile_cost_read."""
        self._dims()
        out = np.zeros((2, (self.height + 7) // 8, (self.width + 7) // 8), np.uint32)
        _check(self.rtx.rtx_tile_cost_read(self.gpu(), _np_ptr(out), out.size), "rtx_tile_cost_read")
        return out[1]

    def set_row_ownership(self, band_height, n_parts, part, halo=True):
        _check(self.rtx.rtx_set_row_ownership(self.gpu(), band_height, n_parts, part, int(halo)), "rtx_set_row_ownership")

    def save_bmp(self, fb, name_no_ext):
        fb = np.ascontiguousarray(fb, np.float32)
        return self.host.rah_save_bmp(self.h, _np_ptr(fb), name_no_ext.encode())
