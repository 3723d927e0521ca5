"""rtx — Python host interface of the MI355X path tracer (ctypes over librtx.so).

Mirrors the reference renderer API, ``class RayTracer`` (/root/reference/src/kernel.cuh:431-470):
``RayTracer(screen_w, screen_h, config)`` -> ``init()`` -> ``draw()`` ... -> ``cleanup()``,
plus the hot-path stages (``build_bvh``, ``trace_primary``) and array downloads used by the
parity tests and bench.  Everything runs in librtx.so (hand-written HIP for gfx950); there
is no CPU fallback: a missing or unloadable library raises ``RuntimeError``.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(_PKG, "lib", "librtx.so")
DATA_DIR = os.path.join(_PKG, "data")

RT_OK = 0
ERRORS = {-1: "RT_ERR_ARG", -2: "RT_ERR_HIP", -3: "RT_ERR_IO", -4: "RT_ERR_STATE", -5: "RT_ERR_NO_DEVICE", -6: "RT_ERR_DEVICE"}

# rt_array_name (include/rtx_amd.h)
ARR = dict(VERTICES=0, INDICES=1, NORMALS=2, TRI_POS=3, AABBS=4, MORTON=5, REORDER=6, NODES=7, TLAS_AABBS=8,
           TLAS_MORTON=9, TLAS_REORDER=10, TLAS_NODES=11, TLAS_SCENE_AABB=12, BATCH_SCENE_AABBS=13, HITS=14,
           HIT_NORMALS=15, HIT_FAKE_NORMALS=16, HIT_STATS=17, TRI_NRM=18, RAYS=19, SKY_PDF=20, SKY_CDF=21,
           SUN_PDF=22, SUN_CDF=23, SUN_DIR=24, HISTOGRAM=25, EXPOSURE=26, COLOR4=27, COLOR16=28, COLOR64=29,
           RGBA8=30, PT_STATS=31, PT_QUEUE=32, PT_Q3_ORIGINS=33, PT_Q3_DIRS=34,
           PT_Q4_ORIGINS=35, PT_Q4_DIRS=36, TEX_ALBEDO_AO=37, TEX_NORMAL_ROUGHNESS=38, TEX_HEIGHT=39, HDR=40,
           BVH_ARENA=41, TRI_MATERIALS=42, ADJ_OFFSETS=43, CORNER_SLOTS=44, TRI_MATERIAL_CENSUS=45,
           EMITTER_TRIS=46, EMITTER_WEIGHTS=47, EMITTER_CDF=48, PT_Q3_BETA=49, SPEC_STATS=50,
           PSEUDO_NORMALS=51)
TEX = dict(SOIL_ALBEDO_AO=0, SOIL_NORMAL_ROUGHNESS=1, SOIL_HEIGHT=2)  # MipmapTextureName (texture.h:5-12)
# rt_buffer_name (Buffer2DName, kernel.cuh:286-315)
BUF = dict(RENDER_COLOR=0, ACCUMULATION=1, HISTORY_COLOR=2, SCALED_COLOR=3, NORMAL=10, DEPTH=11, HISTORY_DEPTH=12,
           MOTION=13, NOISE_LEVEL=14, NOISE_LEVEL16=15, SKY=16, SUN=17, ALBEDO=18, RGBA8=19, HISTOGRAM=20)

# canonical 64-byte BVH node as a numpy record (see RT_ARR_NODES)
NODE_DTYPE = np.dtype([("lmin", "<f4", 3), ("lmax", "<f4", 3), ("rmin", "<f4", 3), ("rmax", "<f4", 3),
                       ("idxLeft", "<u4"), ("idxRight", "<u4"), ("isLeftLeaf", "<u4"), ("isRightLeaf", "<u4")])


class SkyParams(C.Structure):
    _fields_ = [("needRegenerate", C.c_int32), ("timeOfDay", C.c_float), ("sunAxisAngle", C.c_float),
                ("skyScalar", C.c_float), ("sunScalar", C.c_float), ("sunAngle", C.c_float)]


class SampleParams(C.Structure):
    _fields_ = [("sampleSurfaceVsLightUseMisWeight", C.c_int32), ("sampleSkyVsSunUseFluxWeight", C.c_int32),
                ("sampleSurfaceVsLight", C.c_float), ("sampleSkyVsSun", C.c_float)]


class RenderPassSettings(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "enableTemporalDenoising", "enableLocalSpatialFilter", "enableNoiseLevelVisualize",
        "enableWideSpatialFilter", "enableTemporalDenoising2", "enablePostProcess", "enableDownScalePasses",
        "enableHistogram", "enableAutoExposure", "enableBloomEffect", "enableLensFlare", "enableToneMapping",
        "enableSharpening")]


class PostProcessParams(C.Structure):
    _fields_ = [("toneMappingType", C.c_int32), ("exposure", C.c_float), ("gain", C.c_float),
                ("maxWhite", C.c_float), ("gamma", C.c_float)]


class DenoisingParams(C.Structure):
    _fields_ = [(n, C.c_float) for n in (
        "local_denoise_sigma_normal", "local_denoise_sigma_depth", "local_denoise_sigma_material",
        "large_denoise_sigma_normal", "large_denoise_sigma_depth", "large_denoise_sigma_material",
        "temporal_denoise_sigma_normal", "temporal_denoise_sigma_depth", "temporal_denoise_sigma_material",
        "noise_threshold_local", "noise_threshold_large")]


class Params(C.Structure):
    _fields_ = [("sky", SkyParams), ("sample", SampleParams), ("pass_", RenderPassSettings),
                ("post", PostProcessParams), ("denoise", DenoisingParams)]


class Camera(C.Structure):
    _fields_ = [("pos", C.c_float * 3), ("yaw", C.c_float), ("pitch", C.c_float), ("focal", C.c_float),
                ("aperture", C.c_float), ("fovX", C.c_float)]


class Info(C.Structure):
    _fields_ = [("triCount", C.c_uint32), ("triCountPadded", C.c_uint32), ("batchCount", C.c_uint32),
                ("vertexCount", C.c_uint32), ("renderWidth", C.c_int32), ("renderHeight", C.c_int32),
                ("screenWidth", C.c_int32), ("screenHeight", C.c_int32), ("frameNum", C.c_int32),
                ("deviceId", C.c_int32), ("spp", C.c_uint32), ("gbufferSet", C.c_int32),
                ("denoiseRowBegin", C.c_int32), ("denoiseRowEnd", C.c_int32),
                ("gbufferRowBegin", C.c_int32), ("gbufferRowEnd", C.c_int32), ("stripLocalDenoise", C.c_int32),
                ("shadeOnSide", C.c_int32), ("lastChain", C.c_int32)]


class StripExchange(C.Structure):
    """rt_strip_exchange: what a strip-local denoise asks the host to exchange (rt_set_collective_hook)."""
    _fields_ = [("frameNum", C.c_int32), ("rowBegin", C.c_int32), ("rowEnd", C.c_int32), ("historySet", C.c_int32),
                ("gbufferSet", C.c_int32), ("stripLocal", C.c_int32)]


class RayQuery(C.Structure):
    """rt_ray_query: one device ray query (rt_trace_rays_device)."""
    _fields_ = [("org", C.c_void_p), ("org_stride", C.c_uint32), ("dir", C.c_void_p), ("dir_stride", C.c_uint32),
                ("n", C.c_uint32), ("hits", C.c_void_p), ("iters", C.c_void_p), ("flags", C.c_uint32),
                ("ready_event", C.c_void_p), ("done_event", C.c_void_p)]


class SurfaceQuery(C.Structure):
    """rt_surface_query: one device surface query (rt_trace_surfaces_device)."""
    _fields_ = [("rays", RayQuery), ("surface", C.c_void_p), ("flags", C.c_uint32)]


class ClosestQuery(C.Structure):
    """rt_closest_query: one device closest-point query (rt_closest_points_device)."""
    _fields_ = [("points", C.c_void_p), ("stride", C.c_uint32), ("n", C.c_uint32), ("max_distance", C.c_float),
                ("out", C.c_void_p), ("ready_event", C.c_void_p), ("done_event", C.c_void_p)]


class DistanceQuery(C.Structure):
    """rt_distance_query: one device signed distance query (rt_signed_distance_device)."""
    _fields_ = [("closest", ClosestQuery), ("signed_out", C.c_void_p), ("flags", C.c_uint32)]


class Mesh(C.Structure):
    """rt_mesh: an indexed mesh for rt_set_mesh / rt_set_mesh_device."""
    _fields_ = [("xyz", C.c_void_p), ("vertex_count", C.c_uint32), ("indices", C.c_void_p),
                ("triangle_count", C.c_uint32), ("ready_event", C.c_void_p)]


class Skin(C.Structure):
    """rt_skin: a bind pose with four joints and weights per vertex (rt_set_skin, rt_skin_vertices)."""
    _fields_ = [("rest_xyz", C.c_void_p), ("joints", C.c_void_p), ("weights", C.c_void_p),
                ("vertex_count", C.c_uint32), ("joint_count", C.c_uint32)]


class Pose(C.Structure):
    """rt_pose: one 3 x 4 matrix per joint (rt_pose_skin / rt_pose_skin_device)."""
    _fields_ = [("matrices", C.c_void_p), ("joint_count", C.c_uint32), ("ready_event", C.c_void_p)]


class MaterialUpdate(C.Structure):
    """rt_material_update: one device material set (rt_set_triangle_materials_device)."""
    _fields_ = [("ids", C.c_void_p), ("first", C.c_uint32), ("count", C.c_uint32), ("classes", C.c_uint32),
                ("ready_event", C.c_void_p)]


class TextureUpload(C.Structure):
    """rt_texture_upload: one device texture upload (rt_upload_texture_set_device)."""
    _fields_ = [("texels", C.c_void_p), ("set", C.c_uint32), ("which", C.c_int32), ("format", C.c_uint32),
                ("ready_event", C.c_void_p)]


class Environment(C.Structure):
    """rt_environment: one environment image (rt_set_environment / rt_set_environment_device)."""
    _fields_ = [("texels", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32), ("format", C.c_uint32),
                ("layout", C.c_uint32), ("scale", C.c_float), ("ready_event", C.c_void_p)]


class Material(C.Structure):
    """rt_material: one entry of the material table (rt_set_materials)."""
    _fields_ = [("type", C.c_int32), ("flags", C.c_uint32), ("color", C.c_float * 3), ("emission", C.c_float * 3),
                ("ior", C.c_float), ("alpha", C.c_float), ("f0", C.c_float * 3)]

    def __eq__(self, other):
        return isinstance(other, Material) and bytes(self) == bytes(other)

    __hash__ = None

    def __repr__(self):
        return "Material(type=%d, flags=%d, color=%s, emission=%s, ior=%r, alpha=%r, f0=%s)" % (
            self.type, self.flags, list(self.color), list(self.emission), self.ior, self.alpha, list(self.f0))


MAT_LAMBERTIAN, MAT_MIRROR, MAT_GLASS, MAT_MICROFACET, MAT_EMISSIVE = range(5)  # RT_MAT_*
MAT_FLAG_FLAT = 1  # RT_MAT_FLAG_FLAT
TEXTURE_SETS_MAX = 16  # RT_TEXTURE_SETS_MAX
TEX_FORMAT_U16, TEX_FORMAT_U8 = 0, 1  # RT_TEX_FORMAT_*
TEX_SIZE = 1024  # the atlases are TEX_SIZE x TEX_SIZE, 4 channels
SKY_SETS_MAX = 8  # RT_SKY_SETS_MAX
ENV_FORMAT_F32X4, ENV_FORMAT_F16X4 = 0, 1  # RT_ENV_FORMAT_*
ENV_LAYOUT_TABLE, ENV_LAYOUT_LATLONG = 0, 1  # RT_ENV_LAYOUT_*
ENV_TABLE_W, ENV_TABLE_H = 512, 256  # the sky table an environment becomes (RT_BUF_SKY)

QUERY_ANY_HIT = 1          # RT_QUERY_ANY_HIT
QUERY_MAX_RAYS = 1 << 30   # RT_QUERY_MAX_RAYS
SURFACE_FROM_HITS, SURFACE_MOTION = 1, 2  # RT_SURFACE_*


CLOSEST_FLOATS = 8                           # RT_CLOSEST_FLOATS
CLOSEST_FRONT, CLOSEST_FOUND = 1 << 16, 1 << 17  # RT_CLOSEST_*: bits of a closest-point record's last word
DISTANCE_FROM_RECORDS = 1                    # RT_DISTANCE_FROM_RECORDS


def surface_floats(flags: int) -> int:
    """RT_SURFACE_FLOATS: floats per ray of a surface record."""
    return 16 if flags & SURFACE_MOTION else 12


COLLECTIVE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(StripExchange))
HOOK_HISTOGRAM, HOOK_ROWS, HOOK_GBUFFERS = 0, 1, 2


# every entry point declared in include/rtx_amd.h, with its ctypes signature
SIGNATURES = {
    "rt_create": (C.c_int, [C.c_int, C.c_int, C.c_char_p, C.POINTER(C.c_void_p)]),
    "rt_init": (C.c_int, [C.c_void_p]),
    "rt_draw": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_draw_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]),
    "rt_destroy": (None, [C.c_void_p]),
    "rt_last_error": (C.c_char_p, [C.c_void_p]),
    "rt_get_params": (C.c_int, [C.c_void_p, C.POINTER(Params)]),
    "rt_set_params": (C.c_int, [C.c_void_p, C.POINTER(Params)]),
    "rt_get_camera": (C.c_int, [C.c_void_p, C.POINTER(Camera)]),
    "rt_set_camera": (C.c_int, [C.c_void_p, C.POINTER(Camera)]),
    "rt_set_frame_index": (C.c_int, [C.c_void_p, C.c_int]),
    "rt_set_delta_time": (C.c_int, [C.c_void_p, C.c_float]),
    "rt_keyboard_update": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]),
    "rt_cursor_pos_update": (C.c_int, [C.c_void_p, C.c_double, C.c_double]),
    "rt_scroll_update": (C.c_int, [C.c_void_p, C.c_double, C.c_double]),
    "rt_mouse_button_update": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "rt_set_cursor_reset": (C.c_int, [C.c_void_p, C.c_int]),
    "rt_get_info": (C.c_int, [C.c_void_p, C.POINTER(Info)]),
    "rt_get_buffer": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]),
    "rt_buffer_bytes": (C.c_size_t, [C.c_void_p, C.c_int]),
    "rt_path_trace": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "rt_denoise_post": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "rt_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rt_set_post_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rt_set_gather_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rt_bind_buffer": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]),
    "rt_set_collective_hook": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_set_hook_stages": (C.c_int, [C.c_void_p, C.c_uint32]),
    "rt_get_ray_count": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_int]),
    "rt_build_bvh": (C.c_int, [C.c_void_p]),
    "rt_trace_primary": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "rt_sync": (C.c_int, [C.c_void_p]),
    "rt_time_stage": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "rt_debug_pk_math": (C.c_int, [C.c_int, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_size_t]),
    "rt_time_path_trace_kernels": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float), C.c_int]),
    "rt_time_frame_kernels": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int]),
    "rt_trace_rays": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]),
    "rt_trace_rays_device": (C.c_int, [C.c_void_p, C.POINTER(RayQuery)]),
    "rt_trace_surfaces_device": (C.c_int, [C.c_void_p, C.POINTER(SurfaceQuery)]),
    "rt_closest_points_device": (C.c_int, [C.c_void_p, C.POINTER(ClosestQuery)]),
    "rt_point_triangle": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_closest_points_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_float, C.c_void_p]),
    "rt_set_signed_distance": (C.c_int, [C.c_void_p, C.c_int]),
    "rt_get_signed_distance": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "rt_signed_distance_device": (C.c_int, [C.c_void_p, C.POINTER(DistanceQuery)]),
    "rt_pseudo_normals": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]),
    "rt_signed_distance_rule": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_download": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]),
    "rt_array_bytes": (C.c_size_t, [C.c_void_p, C.c_int]),
    "rt_save_camera": (C.c_int, [C.c_void_p, C.c_char_p]),
    "rt_load_camera": (C.c_int, [C.c_void_p, C.c_char_p]),
    "rt_save_image": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    "rt_upload_texture": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "rt_scene_noise3d": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p]),
    "rt_filter_kernel": (C.c_int, [C.c_int, C.c_void_p, C.c_int]),
    "rt_scan_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "rt_frame_marks_begin": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32]),
    "rt_frame_marks_read": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_int)]),
    "rt_update_vertices": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]),
    "rt_update_vertices_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    "rt_get_geometry_epoch": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "rt_set_mesh": (C.c_int, [C.c_void_p, C.POINTER(Mesh)]),
    "rt_set_mesh_device": (C.c_int, [C.c_void_p, C.POINTER(Mesh)]),
    "rt_mesh_adjacency": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_time_mesh_set": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float)]),
    "rt_set_skin": (C.c_int, [C.c_void_p, C.POINTER(Skin)]),
    "rt_reset_skin": (C.c_int, [C.c_void_p]),
    "rt_get_skin": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "rt_pose_skin": (C.c_int, [C.c_void_p, C.POINTER(Pose)]),
    "rt_pose_skin_device": (C.c_int, [C.c_void_p, C.POINTER(Pose)]),
    "rt_skin_vertices": (C.c_int, [C.POINTER(Skin), C.c_void_p, C.c_void_p]),
    "rt_set_geometry_motion": (C.c_int, [C.c_void_p, C.c_int]),
    "rt_get_geometry_motion": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "rt_set_emitter_sampling": (C.c_int, [C.c_void_p, C.c_int, C.c_float]),
    "rt_get_emitter_sampling": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float)]),
    "rt_emitter_weight": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]),
    "rt_emitter_select": (C.c_int, [C.c_void_p, C.c_uint32, C.c_float, C.POINTER(C.c_uint32), C.POINTER(C.c_float)]),
    "rt_set_triangle_materials": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]),
    "rt_reset_triangle_materials": (C.c_int, [C.c_void_p]),
    "rt_material_classes": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)]),
    "rt_set_triangle_materials_device": (C.c_int, [C.c_void_p, C.POINTER(MaterialUpdate)]),
    "rt_material_class_rule": (C.c_uint32, [C.c_uint32]),
    "rt_default_material": (C.c_int, [C.c_uint32, C.POINTER(Material)]),
    "rt_set_materials": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(Material)]),
    "rt_get_materials": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(Material)]),
    "rt_reset_materials": (C.c_int, [C.c_void_p]),
    "rt_get_texture_sets": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    "rt_upload_texture_set": (C.c_int, [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "rt_upload_texture_set_device": (C.c_int, [C.c_void_p, C.POINTER(TextureUpload)]),
    "rt_set_material_textures": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    "rt_get_material_textures": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    "rt_reset_material_textures": (C.c_int, [C.c_void_p]),
    "rt_get_sky_sets": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    "rt_set_environment": (C.c_int, [C.c_void_p, C.POINTER(Environment)]),
    "rt_set_environment_device": (C.c_int, [C.c_void_p, C.POINTER(Environment)]),
    "rt_reset_environment": (C.c_int, [C.c_void_p]),
    "rt_get_environment": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "rt_environment_table": (C.c_int, [C.POINTER(Environment), C.c_void_p, C.c_void_p]),
}
MAT_CLASS_GLOSSY, MAT_CLASS_MICROFACET = 1, 2  # RT_MAT_CLASS_*
MAT_CLASS_ALL = MAT_CLASS_GLOSSY | MAT_CLASS_MICROFACET
IMAGE_PPM_RGBA8, IMAGE_PFM_HDR = 0, 1
DRAW_ASYNC = 1  # rt_draw_device flag
BUF_SET1, BUF_SET2, BUF_SET3 = 0x100, 0x200, 0x300  # rt_bind_buffer: further G-buffer sets (frame pipelining)
SKIN_INFLUENCES, SKIN_JOINTS_MAX = 4, 4096  # RT_SKIN_*
GBUFFER_SETS = 4  # G-buffer sets a pipelined context cycles through (rt_set_post_stream; RT_GBUFFER_SETS)

_lib = None


def load_library(path: str | None = None) -> C.CDLL:
    """Load librtx.so (RTX_LIB overrides the in-tree path, for ablation builds); raises if it is
    missing (no fallback path exists)."""
    global _lib
    if _lib is not None:
        return _lib
    path = path or os.environ.get("RTX_LIB") or LIB_PATH
    if not os.path.exists(path):
        raise RuntimeError("librtx.so not found at %s — run `make` (or __graft_entry__.build())" % path)
    # One HIP runtime per process: torch ships its own libamdhip64 (same soname, different path).
    # Loaded after librtx it would be a second runtime that finds no GPU, so when torch is
    # installed it is loaded first and librtx binds to it; streams then pass freely between them.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


class RtError(RuntimeError):
    pass


def write_config(path: str, width: int, height: int, dynamic: bool = False, chunk_dim: int = 1, spp: int = 1,
                 extra: str = "", max_size=(3840, 2160), camera_file: str | None = None, min_size=(640, 480),
                 target_fps: float = 60.0, mesh_file: str | None = None, tuning: dict | None = None,
                 geometry_motion: bool | None = None, max_triangles: int | None = None,
                 max_vertices: int | None = None, texture_sets: int | None = None,
                 emitter_sampling: bool | None = None, emitter_probability: float | None = None,
                 sky_sets: int | None = None, signed_distance: bool | None = None) -> str:
    """Write a config.toml with the reference's three tables (resources/config.toml) + extensions.

    `tuning`: the [tuning] table (scheduling A/B aids, include/rtx_amd.h).  When None, the
    RTX_TUNING environment variable ("key=value,key=value", e.g. "chain=off,tracePerCu=2") fills
    it: the A/B tools (tools/ab.sh) set it per variant.  The library itself reads no environment.
    `geometry_motion`: [render] geometryMotion, the initial state of rt_set_geometry_motion (None:
    the key is not written, the default is off).
    `max_triangles` / `max_vertices`: [scene] maxTriangles / maxVertices, the capacity of set_mesh
    (None: the keys are not written, the capacity is the init mesh).
    `texture_sets`: [scene] textureSets, the texture sets the context holds (None: the key is not
    written, one set).
    `emitter_sampling` / `emitter_probability`: [render] emitterSampling / emitterProbability, the initial
    state of rt_set_emitter_sampling (None: the keys are not written; off, 0.5).
    `sky_sets`: [scene] skySets, the sky sets the context holds (None: the key is not written, one set).
    `signed_distance`: [render] signedDistance, the initial state of rt_set_signed_distance (None: the key
    is not written, the default is off)."""
    with open(path, "w") as f:
        f.write("[resolution]\nwidth = %d\nheight = %d\n\n" % (width, height))
        if camera_file:
            f.write('[file]\nloadCameraAtInit = true\ninputCameraFileName = "%s"\ncameraSaveFileName = "%s"\n\n'
                    % (camera_file, camera_file))
        else:
            f.write("[file]\nloadCameraAtInit = false\n\n")
        f.write("[optimziation]\nuseDynamicResolution = %s\ntargetFps = %r\nmaxWidth = %d\nmaxHeight = %d\n"
                "minWidth = %d\nminHeight = %d\n\n" % ("true" if dynamic else "false", float(target_fps), max_size[0],
                                                      max_size[1], min_size[0], min_size[1]))
        f.write("[scene]\nchunkDim = %d\n" % chunk_dim)
        if mesh_file:  # a meshProcessor .bin instead of the procedural terrain (init.cu:28-50)
            f.write('meshFile = "%s"\n' % mesh_file)
        if max_triangles is not None:
            f.write("maxTriangles = %s\n" % max_triangles)
        if max_vertices is not None:
            f.write("maxVertices = %s\n" % max_vertices)
        if texture_sets is not None:
            f.write("textureSets = %s\n" % texture_sets)
        if sky_sets is not None:
            f.write("skySets = %s\n" % sky_sets)
        f.write("\n[render]\nspp = %d\n" % spp)
        if geometry_motion is not None:
            f.write("geometryMotion = %s\n" % ("true" if geometry_motion else "false"))
        if emitter_sampling is not None:
            f.write("emitterSampling = %s\n" % ("true" if emitter_sampling else "false"))
        if emitter_probability is not None:
            f.write("emitterProbability = %r\n" % float(emitter_probability))
        if signed_distance is not None:
            f.write("signedDistance = %s\n" % ("true" if signed_distance else "false"))
        f.write(extra)
        if tuning is None:
            tuning = tuning_from_env()
        if tuning:
            f.write("\n[tuning]\n")
            for k, v in tuning.items():
                f.write("%s = %s\n" % (k, _toml_value(v)))
    return path


def _toml_value(v) -> str:
    if isinstance(v, bool):
        return "true" if v else "false"
    if isinstance(v, (int, float)):
        return repr(v)
    s = str(v)
    if s in ("true", "false") or s.lstrip("-").isdigit():
        return s
    return '"%s"' % s


def tuning_from_env() -> dict:
    """RTX_TUNING="key=value,..." as a [tuning] table (A/B tools only)."""
    out = {}
    for item in filter(None, (x.strip() for x in os.environ.get("RTX_TUNING", "").split(","))):
        k, _, v = item.partition("=")
        out[k.strip()] = v.strip()
    return out


class RayTracer:
    """The reference's RayTracer lifecycle over the C-ABI (kernel.cuh:431-470)."""

    def __init__(self, screen_width: int, screen_height: int, config: str | None = None):
        self.lib = load_library()
        h = C.c_void_p()
        rc = self.lib.rt_create(screen_width, screen_height, config.encode() if config else None, C.byref(h))
        if rc != RT_OK:
            raise RtError("rt_create: %s %s" % (ERRORS.get(rc, rc), self.lib.rt_last_error(None).decode()))
        self.h = h

    # ---- lifecycle
    def _check(self, rc, what):
        if rc != RT_OK:
            raise RtError("%s: %s %s" % (what, ERRORS.get(rc, rc), self.lib.rt_last_error(self.h).decode()))

    def init(self):
        self._check(self.lib.rt_init(self.h), "rt_init")
        return self

    def draw(self, rgba8: np.ndarray | None = None, hdr: np.ndarray | None = None):
        self._check(self.lib.rt_draw(self.h, _ptr(rgba8), _ptr(hdr)), "rt_draw")

    def draw_device(self, device_ptr: int, pitch_bytes: int = 0, asynchronous: bool = False):
        """draw(SurfObj*): the RGBA8 frame into caller-owned device memory (e.g. a torch uint8
        tensor's data_ptr()); asynchronous=True enqueues the frame and pipelines frames."""
        self._check(self.lib.rt_draw_device(self.h, device_ptr, pitch_bytes, DRAW_ASYNC if asynchronous else 0),
                    "rt_draw_device")

    def cleanup(self):
        if getattr(self, "h", None):
            self.lib.rt_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.cleanup()
        except Exception:
            pass

    # ---- parameters
    @property
    def params(self) -> Params:
        p = Params()
        self._check(self.lib.rt_get_params(self.h, C.byref(p)), "rt_get_params")
        return p

    @params.setter
    def params(self, p: Params):
        self._check(self.lib.rt_set_params(self.h, C.byref(p)), "rt_set_params")

    @property
    def camera(self) -> Camera:
        c = Camera()
        self._check(self.lib.rt_get_camera(self.h, C.byref(c)), "rt_get_camera")
        return c

    @camera.setter
    def camera(self, c: Camera):
        self._check(self.lib.rt_set_camera(self.h, C.byref(c)), "rt_set_camera")

    def set_frame_index(self, n: int):
        self._check(self.lib.rt_set_frame_index(self.h, n), "rt_set_frame_index")

    def set_delta_time(self, ms: float):
        self._check(self.lib.rt_set_delta_time(self.h, ms), "rt_set_delta_time")

    # ---- input (inputControl.cu): GLFW key / action / modifier values
    def keyboard_update(self, key: int, scancode: int, action: int, mods: int):
        self._check(self.lib.rt_keyboard_update(self.h, key, scancode, action, mods), "rt_keyboard_update")

    def cursor_pos_update(self, x: float, y: float):
        self._check(self.lib.rt_cursor_pos_update(self.h, x, y), "rt_cursor_pos_update")

    def scroll_update(self, dx: float, dy: float):
        self._check(self.lib.rt_scroll_update(self.h, dx, dy), "rt_scroll_update")

    def mouse_button_update(self, button: int, action: int, mods: int):
        self._check(self.lib.rt_mouse_button_update(self.h, button, action, mods), "rt_mouse_button_update")

    def set_cursor_reset(self, reset: bool = True):
        self._check(self.lib.rt_set_cursor_reset(self.h, int(reset)), "rt_set_cursor_reset")

    def info(self) -> Info:
        i = Info()
        self._check(self.lib.rt_get_info(self.h, C.byref(i)), "rt_get_info")
        return i

    # ---- hot-path stages
    def build_bvh(self):
        self._check(self.lib.rt_build_bvh(self.h), "rt_build_bvh")

    # ---- animated geometry (rt_update_vertices*, include/rtx_amd.h)
    def update_vertices(self, xyz: np.ndarray, first: int = 0):
        """New positions for vertices [first, first + len(xyz)) from a C-contiguous (n, 3) float32
        array; the smooth normals of the whole mesh follow, and every later build_bvh / draw."""
        if not isinstance(xyz, np.ndarray) or xyz.dtype != np.float32 or xyz.ndim != 2 or xyz.shape[1] != 3:
            raise ValueError("update_vertices: xyz must be an (n, 3) float32 array")
        if not xyz.flags["C_CONTIGUOUS"]:
            raise ValueError("update_vertices: xyz must be C-contiguous")
        if not 0 <= int(first) <= 0xFFFFFFFF or len(xyz) > 0xFFFFFFFF:
            raise ValueError("update_vertices: first and the vertex count must fit 32 bits")
        self._check(self.lib.rt_update_vertices(self.h, xyz.ctypes.data, int(first), len(xyz)), "rt_update_vertices")

    def update_vertices_device(self, ptr: int, count: int, first: int = 0, ready_event: int | None = None):
        """The same from device memory (count xyz float32 triples at ptr), asynchronous.  ready_event:
        a hipEvent_t handle (e.g. torch.cuda.Event.cuda_event) the read waits for; None: the read
        follows everything enqueued on the context stream so far."""
        if not 0 <= int(first) <= 0xFFFFFFFF or not 0 <= int(count) <= 0xFFFFFFFF:
            raise ValueError("update_vertices_device: first and count must fit 32 bits")
        self._check(self.lib.rt_update_vertices_device(self.h, ptr, int(first), int(count), ready_event),
                    "rt_update_vertices_device")

    # ---- mesh replacement (rt_set_mesh*, include/rtx_amd.h)
    def set_mesh(self, vertices: np.ndarray, indices: np.ndarray):
        """A new indexed mesh from host arrays: (nv, 3) float32 positions and (ntri, 3) uint32 indices,
        C-contiguous, within the capacity ([scene] maxTriangles / maxVertices).  The smooth normals
        and every later build_bvh / draw follow; info() and the mesh-level downloads at once."""
        if not isinstance(vertices, np.ndarray) or vertices.dtype != np.float32 or vertices.ndim != 2 or vertices.shape[1] != 3:
            raise ValueError("set_mesh: vertices must be an (n, 3) float32 array")
        if not isinstance(indices, np.ndarray) or indices.dtype != np.uint32 or indices.ndim != 2 or indices.shape[1] != 3:
            raise ValueError("set_mesh: indices must be an (n, 3) uint32 array")
        if not vertices.flags["C_CONTIGUOUS"] or not indices.flags["C_CONTIGUOUS"]:
            raise ValueError("set_mesh: the arrays must be C-contiguous")
        if len(vertices) > 0xFFFFFFFF or len(indices) > 0xFFFFFFFF:
            raise ValueError("set_mesh: the counts must fit 32 bits")
        m = Mesh(vertices.ctypes.data, len(vertices), indices.ctypes.data, len(indices), None)
        self._check(self.lib.rt_set_mesh(self.h, C.byref(m)), "rt_set_mesh")

    def set_mesh_device(self, xyz_ptr: int, nv: int, idx_ptr: int, ntri: int, ready_event: int | None = None):
        """The same from device memory (nv xyz float32 triples at xyz_ptr, ntri uint32 index triples
        at idx_ptr), asynchronous; ready_event as in update_vertices_device."""
        if not 0 <= int(nv) <= 0xFFFFFFFF or not 0 <= int(ntri) <= 0xFFFFFFFF:
            raise ValueError("set_mesh_device: nv and ntri must fit 32 bits")
        m = Mesh(xyz_ptr, int(nv), idx_ptr, int(ntri), ready_event)
        self._check(self.lib.rt_set_mesh_device(self.h, C.byref(m)), "rt_set_mesh_device")

    # ---- skinned meshes (rt_set_skin / rt_pose_skin*, include/rtx_amd.h)
    def set_skin(self, rest: np.ndarray, joints: np.ndarray, weights: np.ndarray, joint_count: int):
        """The mesh's skin from host arrays: (nv, 3) float32 rest positions, (nv, 4) uint16 joint indices and
        (nv, 4) float32 weights, C-contiguous, nv the mesh's vertex count.  A host-style setter: it waits
        for the renderer's streams; the arrays are free on return.  No vertex moves until a pose."""
        s = _skin(rest, joints, weights, joint_count, "set_skin")
        self._check(self.lib.rt_set_skin(self.h, C.byref(s)), "rt_set_skin")

    def reset_skin(self):
        """No skin: a pose is an error until the next set_skin (a host-style setter)."""
        self._check(self.lib.rt_reset_skin(self.h), "rt_reset_skin")

    @property
    def skin(self):
        """(vertex_count, joint_count) of the skin, (0, 0) without one."""
        nv, nj = C.c_uint32(), C.c_uint32()
        self._check(self.lib.rt_get_skin(self.h, C.byref(nv), C.byref(nj)), "rt_get_skin")
        return nv.value, nj.value

    def pose_skin(self, matrices: np.ndarray):
        """One pose from host matrices, a C-contiguous (J, 3, 4) or (J, 12) float32 array, J the skin's
        joint count: every vertex moves to the skinning rule's position, and the normals and every later
        build_bvh / draw follow as after a whole-mesh update_vertices."""
        m = _pose_matrices(matrices, "pose_skin")
        p = Pose(m.ctypes.data, len(m), None)
        self._check(self.lib.rt_pose_skin(self.h, C.byref(p)), "rt_pose_skin")

    def pose_skin_device(self, tensor_or_ptr, joint_count: int, ready_event: int | None = None):
        """The same from device memory (joint_count x 12 float32, 16-byte aligned), given as a device pointer
        or an object with data_ptr() (a contiguous float32 torch tensor, whose size is checked);
        asynchronous, no host wait.  ready_event as in update_vertices_device."""
        if not 0 <= int(joint_count) <= 0xFFFFFFFF:
            raise ValueError("pose_skin_device: joint_count must fit 32 bits")
        ptr = tensor_or_ptr
        if hasattr(tensor_or_ptr, "data_ptr"):
            t = tensor_or_ptr
            if t.element_size() != 4 or not t.is_floating_point() or t.numel() != int(joint_count) * 12 or not t.is_contiguous():
                raise ValueError("pose_skin_device: the tensor must be contiguous float32 and hold joint_count x 12 values")
            ptr = t.data_ptr()
        p = Pose(int(ptr) if ptr else None, int(joint_count), ready_event)
        self._check(self.lib.rt_pose_skin_device(self.h, C.byref(p)), "rt_pose_skin_device")

    def time_mesh_set(self, iters: int = 1):
        """(ingest, adjacency, normals) milliseconds summed over `iters` whole-mesh sets of the
        current mesh (rt_time_mesh_set)."""
        ms = (C.c_float * 3)()
        self._check(self.lib.rt_time_mesh_set(self.h, iters, ms), "rt_time_mesh_set")
        return tuple(float(v) for v in ms)

    @property
    def geometry_epoch(self) -> int:
        """0 after init, +1 per vertex update or mesh set."""
        v = C.c_uint64()
        self._check(self.lib.rt_get_geometry_epoch(self.h, C.byref(v)), "rt_get_geometry_epoch")
        return v.value

    @property
    def geometry_motion(self) -> bool:
        """Geometry motion vectors (rt_set_geometry_motion): the MOTION G-buffer follows vertex updates."""
        v = C.c_int()
        self._check(self.lib.rt_get_geometry_motion(self.h, C.byref(v)), "rt_get_geometry_motion")
        return bool(v.value)

    @geometry_motion.setter
    def geometry_motion(self, on: bool):
        self._check(self.lib.rt_set_geometry_motion(self.h, 1 if on else 0), "rt_set_geometry_motion")

    # ---- emitter sampling (rt_set_emitter_sampling, include/rtx_amd.h)
    def set_emitter_sampling(self, on: bool, probability: float = 0.5):
        """Next-event estimation of the emissive triangles of a custom material table: a diffuse
        interaction's light sample goes to an emitter with `probability`, else to the sun or sky.  Takes
        effect from the next LBVH build; download("EMITTER_TRIS" / "EMITTER_WEIGHTS" / "EMITTER_CDF")
        return the list of the last build."""
        self._check(self.lib.rt_set_emitter_sampling(self.h, 1 if on else 0, float(probability)), "rt_set_emitter_sampling")

    @property
    def emitter_sampling(self):
        """(on, probability) of rt_get_emitter_sampling."""
        on, q = C.c_int(), C.c_float()
        self._check(self.lib.rt_get_emitter_sampling(self.h, C.byref(on), C.byref(q)), "rt_get_emitter_sampling")
        return bool(on.value), q.value

    # ---- signed distance queries (rt_set_signed_distance, include/rtx_amd.h)
    @property
    def signed_distance(self) -> bool:
        """Signed distance queries (rt_set_signed_distance): every LBVH build writes its pseudo-normal table,
        which signed_distance_device reads.  Takes effect from the next build; download("PSEUDO_NORMALS")
        returns the table of the last build."""
        v = C.c_int()
        self._check(self.lib.rt_get_signed_distance(self.h, C.byref(v)), "rt_get_signed_distance")
        return bool(v.value)

    @signed_distance.setter
    def signed_distance(self, on: bool):
        self._check(self.lib.rt_set_signed_distance(self.h, 1 if on else 0), "rt_set_signed_distance")

    # ---- per-triangle materials (rt_set_triangle_materials, include/rtx_amd.h)
    def set_triangle_materials(self, ids: np.ndarray, first: int = 0):
        """Material ids of triangles [first, first + len(ids)) from a contiguous 1-D uint8 array: 0..9
        index the reference's material table, an id >= 10 is a mirror with that mask.  Takes effect
        for every path trace enqueued after it; download("TRI_MATERIALS") returns the table."""
        if not isinstance(ids, np.ndarray) or ids.dtype != np.uint8 or ids.ndim != 1:
            raise ValueError("set_triangle_materials: ids must be a 1-D uint8 array")
        if not ids.flags["C_CONTIGUOUS"]:
            raise ValueError("set_triangle_materials: ids must be contiguous")
        if not 0 <= int(first) <= 0xFFFFFFFF or len(ids) > 0xFFFFFFFF:
            raise ValueError("set_triangle_materials: first and the triangle count must fit 32 bits")
        self._check(self.lib.rt_set_triangle_materials(self.h, ids.ctypes.data, int(first), len(ids)),
                    "rt_set_triangle_materials")

    def set_triangle_materials_device(self, ptr: int, count: int, first: int = 0, classes: int = MAT_CLASS_ALL,
                                      ready_event: int | None = None):
        """The same from device memory (count uint8 ids at ptr, any alignment), stream-ordered: no
        host wait.  classes: the MAT_CLASS_* bits that bound the classes of every id of the whole
        table after the update (material_classes() of it; declaring more costs speed only, an id of
        an undeclared class is stored as 3 and reported by the next checking call).  ready_event as
        in update_vertices_device."""
        if not 0 <= int(first) <= 0xFFFFFFFF or not 0 <= int(count) <= 0xFFFFFFFF:
            raise ValueError("set_triangle_materials_device: first and count must fit 32 bits")
        if not 0 <= int(classes) <= 0xFFFFFFFF:
            raise ValueError("set_triangle_materials_device: classes must fit 32 bits")
        u = MaterialUpdate(ptr, int(first), int(count), int(classes), ready_event)
        self._check(self.lib.rt_set_triangle_materials_device(self.h, C.byref(u)), "rt_set_triangle_materials_device")

    def reset_triangle_materials(self):
        """Back to the reference's table, material 3 for every triangle."""
        self._check(self.lib.rt_reset_triangle_materials(self.h), "rt_reset_triangle_materials")

    # ---- the material table (rt_set_materials, include/rtx_amd.h)
    def set_materials(self, first_id: int, materials):
        """Replace entries [first_id, first_id + len(materials)) of the material table (a sequence of
        Material); the other entries stay as they were.  Takes effect for every path trace enqueued
        after it."""
        mats = list(materials)
        if not all(isinstance(m, Material) for m in mats):
            raise ValueError("set_materials: materials must be rtx.Material instances")
        if not 0 <= int(first_id) <= 0xFFFFFFFF:
            raise ValueError("set_materials: first_id must fit 32 bits")
        arr = (Material * max(len(mats), 1))(*mats)
        self._check(self.lib.rt_set_materials(self.h, int(first_id), len(mats), arr), "rt_set_materials")

    def get_materials(self, first_id: int = 0, count: int = 256):
        """Entries [first_id, first_id + count) as a list of Material: what was set, or the defaults."""
        if not 0 <= int(first_id) <= 0xFFFFFFFF or not 0 <= int(count) <= 0xFFFFFFFF:
            raise ValueError("get_materials: first_id and count must fit 32 bits")
        arr = (Material * max(int(count), 1))()
        self._check(self.lib.rt_get_materials(self.h, int(first_id), int(count), arr), "rt_get_materials")
        return [Material.from_buffer_copy(arr[k]) for k in range(int(count))]

    def reset_materials(self):
        """Back to the reference's constants: no custom table."""
        self._check(self.lib.rt_reset_materials(self.h), "rt_reset_materials")

    # ---- texture sets (rt_upload_texture_set, rt_set_material_textures; include/rtx_amd.h)
    @property
    def texture_sets(self) -> int:
        """The texture sets the context holds ([scene] textureSets; 1 without the key)."""
        n = C.c_uint32()
        self._check(self.lib.rt_get_texture_sets(self.h, C.byref(n)), "rt_get_texture_sets")
        return n.value

    def upload_texture_device(self, name: str, tensor_or_ptr, set: int, fmt: int, ready_event: int | None = None):
        """Level 0 of map `name` of texture set `set` from device memory, stream-ordered (no host wait):
        1024 x 1024 x 4 channels of uint16 (TEX_FORMAT_U16) or uint8 (TEX_FORMAT_U8, each channel
        v * 257), given as a device pointer or an object with data_ptr() (a contiguous torch tensor,
        whose size is checked).  ready_event as in update_vertices_device."""
        if name not in ("SOIL_ALBEDO_AO", "SOIL_NORMAL_ROUGHNESS"):
            raise ValueError("upload_texture_device: name must be SOIL_ALBEDO_AO or SOIL_NORMAL_ROUGHNESS")
        if fmt not in (TEX_FORMAT_U16, TEX_FORMAT_U8):
            raise ValueError("upload_texture_device: fmt must be TEX_FORMAT_U16 or TEX_FORMAT_U8")
        if not 0 <= int(set) <= 0xFFFFFFFF:
            raise ValueError("upload_texture_device: set must fit 32 bits")
        ptr = tensor_or_ptr
        if hasattr(tensor_or_ptr, "data_ptr"):
            t = tensor_or_ptr
            want = TEX_SIZE * TEX_SIZE * 4 * (2 if fmt == TEX_FORMAT_U16 else 1)
            if t.numel() * t.element_size() != want or not t.is_contiguous():
                raise ValueError("upload_texture_device: the tensor must be contiguous and hold %d bytes" % want)
            ptr = t.data_ptr()
        u = TextureUpload(int(ptr), int(set), TEX[name], int(fmt), ready_event)
        self._check(self.lib.rt_upload_texture_set_device(self.h, C.byref(u)), "rt_upload_texture_set_device")

    def set_material_textures(self, first_id: int, sets):
        """Bind material ids [first_id, first_id + len(sets)) to texture sets (a sequence of set
        indices); the other ids keep theirs.  Takes effect for every path trace enqueued after it."""
        a = np.asarray(sets)
        if a.size == 0:
            a = np.zeros(0, np.uint8)
        if a.ndim != 1 or a.dtype.kind not in "iu" or (a.size and (a.min() < 0 or a.max() > 255)):
            raise ValueError("set_material_textures: sets must be a 1-D sequence of integers in 0..255")
        if not 0 <= int(first_id) <= 0xFFFFFFFF:
            raise ValueError("set_material_textures: first_id must fit 32 bits")
        a = np.ascontiguousarray(a, np.uint8)
        buf = a if a.size else np.zeros(1, np.uint8)
        self._check(self.lib.rt_set_material_textures(self.h, int(first_id), int(a.size), buf.ctypes.data),
                    "rt_set_material_textures")

    def get_material_textures(self, first_id: int = 0, count: int = 256) -> np.ndarray:
        """The texture set of ids [first_id, first_id + count) as a uint8 array."""
        if not 0 <= int(first_id) <= 0xFFFFFFFF or not 0 <= int(count) <= 0xFFFFFFFF:
            raise ValueError("get_material_textures: first_id and count must fit 32 bits")
        out = np.zeros(max(int(count), 1) if int(count) <= 256 else 1, np.uint8)
        self._check(self.lib.rt_get_material_textures(self.h, int(first_id), int(count), out.ctypes.data),
                    "rt_get_material_textures")
        return out[:int(count)]

    def reset_material_textures(self):
        """Every id back to set 0: no binding."""
        self._check(self.lib.rt_reset_material_textures(self.h), "rt_reset_material_textures")

    # ---- sky sets and environment maps (include/rtx_amd.h)
    @property
    def sky_sets(self) -> int:
        """The sky sets the context holds ([scene] skySets; 1 without the key)."""
        n = C.c_uint32()
        self._check(self.lib.rt_get_sky_sets(self.h, C.byref(n)), "rt_get_sky_sets")
        return n.value

    @property
    def environment_active(self) -> bool:
        on = C.c_int()
        self._check(self.lib.rt_get_environment(self.h, C.byref(on)), "rt_get_environment")
        return bool(on.value)

    def set_environment(self, image, layout: int, scale: float = 1.0):
        """rt_set_environment: `image` is a (height, width, 4) float32 or float16 array, TABLE (512 x 256,
        the renderer's equal-area table) or LATLONG (row 0 at the zenith).  A host-style setter: it waits
        for the renderer's streams; the array is free on return."""
        a, e = _environment(image, layout, scale)
        self._check(self.lib.rt_set_environment(self.h, C.byref(e)), "rt_set_environment")

    def set_environment_device(self, tensor_or_ptr, width: int, height: int, fmt: int, layout: int, scale: float = 1.0,
                               ready_event: int | None = None):
        """rt_set_environment_device: width x height x 4 channels of float32 (ENV_FORMAT_F32X4) or float16
        (ENV_FORMAT_F16X4) in device memory, given as a device pointer or an object with data_ptr() (a
        contiguous torch tensor, whose size is checked); stream-ordered, no host wait; needs sky_sets >= 2.
        ready_event as in update_vertices_device."""
        if fmt not in (ENV_FORMAT_F32X4, ENV_FORMAT_F16X4):
            raise ValueError("set_environment_device: fmt must be ENV_FORMAT_F32X4 or ENV_FORMAT_F16X4")
        for name, v in (("width", width), ("height", height), ("layout", layout)):
            if not 0 <= int(v) <= 0xFFFFFFFF:
                raise ValueError("set_environment_device: %s must fit 32 bits" % name)
        ptr = tensor_or_ptr
        if hasattr(tensor_or_ptr, "data_ptr"):
            t = tensor_or_ptr
            want = int(width) * int(height) * (16 if fmt == ENV_FORMAT_F32X4 else 8)
            if t.numel() * t.element_size() != want or not t.is_contiguous():
                raise ValueError("set_environment_device: the tensor must be contiguous and hold %d bytes" % want)
            ptr = t.data_ptr()
        e = Environment(int(ptr) if ptr else None, int(width), int(height), int(fmt), int(layout), float(scale), ready_event)
        self._check(self.lib.rt_set_environment_device(self.h, C.byref(e)), "rt_set_environment_device")

    def reset_environment(self):
        """Back to the Hosek sky table (a host-style setter)."""
        self._check(self.lib.rt_reset_environment(self.h), "rt_reset_environment")

    def trace_primary(self, frame_num: int = 1, detail: bool = False):
        self._check(self.lib.rt_trace_primary(self.h, frame_num, 1 if detail else 0), "rt_trace_primary")

    def path_trace(self, frame_num: int = 1, detail: bool = False):
        self._check(self.lib.rt_path_trace(self.h, frame_num, 1 if detail else 0), "rt_path_trace")

    def denoise_post(self, frame_num: int, hdr: bool = False):
        self._check(self.lib.rt_denoise_post(self.h, frame_num, 1 if hdr else 0), "rt_denoise_post")

    def set_stream(self, stream_ptr: int | None):
        """Enqueue on a hipStream_t handle (0: the null stream, torch's default stream); None
        restores the context's own stream (RT_OWN_STREAM)."""
        ptr = C.c_void_p(-1) if stream_ptr is None else C.c_void_p(stream_ptr)
        self._check(self.lib.rt_set_stream(self.h, ptr), "rt_set_stream")

    def set_post_stream(self, stream_ptr: int | None):
        """Run denoise + post on a second stream and alternate two G-buffer sets (frame pipelining)."""
        self._check(self.lib.rt_set_post_stream(self.h, stream_ptr), "rt_set_post_stream")

    def set_gather_stream(self, stream: int | None):
        """Stream the caller gathers G-buffers on; each later denoise also waits for it.
        0 is the null stream (torch's default stream), as in set_stream; None turns it off."""
        ptr = C.c_void_p(-2) if stream is None else C.c_void_p(stream)  # RT_STREAM_OFF
        self._check(self.lib.rt_set_gather_stream(self.h, ptr), "rt_set_gather_stream")

    def set_collective_hook(self, fn):
        """fn(stage, stream_handle, exchange) -> None, called on the host when a strip-local denoise
        needs its histogram all-reduce (HOOK_HISTOGRAM) or its rows all-gather (HOOK_ROWS) enqueued
        on stream_handle; None removes the hook (every rank then denoises the whole frame)."""
        if fn is None:
            self._hook = None
            self._check(self.lib.rt_set_collective_hook(self.h, None, None), "rt_set_collective_hook")
            return

        def tramp(arg, stage, stream, x):
            try:
                fn(stage, stream or 0, x.contents)
                return 0
            except Exception:  # reported through rt_last_error's RT_ERR_STATE
                import traceback
                traceback.print_exc()
                return 1

        self._hook = COLLECTIVE_FN(tramp)  # keep the thunk alive as long as the context
        self._check(self.lib.rt_set_collective_hook(self.h, C.cast(self._hook, C.c_void_p), None),
                    "rt_set_collective_hook")

    def set_hook_stages(self, *stages):
        """The hook stages the renderer calls (HOOK_HISTOGRAM, HOOK_ROWS, HOOK_GBUFFERS)."""
        mask = 0
        for st in stages:
            mask |= 1 << int(st)
        self._check(self.lib.rt_set_hook_stages(self.h, mask), "rt_set_hook_stages")

    def bind_buffer(self, name: str, device_ptr: int, nbytes: int, gbuffer_set: int = 0):
        what = BUF[name] | (int(gbuffer_set) << 8)  # RT_BUF_SET1 / RT_BUF_SET2 / RT_BUF_SET3
        self._check(self.lib.rt_bind_buffer(self.h, what, device_ptr, nbytes), "rt_bind_buffer")

    def buffer_bytes(self, name: str) -> int:
        return self.lib.rt_buffer_bytes(self.h, BUF[name])

    def ray_count(self, reset: bool = False) -> int:
        v = C.c_uint64()
        self._check(self.lib.rt_get_ray_count(self.h, C.byref(v), 1 if reset else 0), "rt_get_ray_count")
        return v.value

    def sync(self):
        self._check(self.lib.rt_sync(self.h), "rt_sync")

    def time_stage(self, stage: int, iters: int) -> float:
        ms = C.c_float()
        self._check(self.lib.rt_time_stage(self.h, stage, iters, C.byref(ms)), "rt_time_stage")
        return ms.value

    PT_KERNELS = ("k_pt_camera", "k_pt_shade0", "k_trace_queue<3>", "k_pt_resume<3>", "k_trace_queue<4>",
                  "k_pt_resume<4>", "k_pt_resolve")
    DN_KERNELS = ("k_temporal", "k_spatial7", "k_spatial5<3>", "k_spatial5<6>", "k_spatial5<12>", "k_temporal2",
                  "k_downscale_chain", "k_scale_post")
    FRAME_KERNELS = PT_KERNELS + DN_KERNELS

    def time_path_trace_kernels(self, iters=10):
        """Average ms of each path-trace kernel (HIP events on the context stream)."""
        ms = (C.c_float * len(self.PT_KERNELS))()
        self._check(self.lib.rt_time_path_trace_kernels(self.h, iters, ms, len(ms)), "rt_time_path_trace_kernels")
        return dict(zip(self.PT_KERNELS, (float(v) for v in ms)))

    def time_frame_kernels(self, first_frame: int, iters: int = 10):
        """Average ms of each path-trace and denoise / post kernel over `iters` whole frames run as
        the caller runs them (pipelined when a post stream is set); waits for the frames."""
        ms = (C.c_float * len(self.FRAME_KERNELS))()
        self._check(self.lib.rt_time_frame_kernels(self.h, first_frame, iters, ms, len(ms)), "rt_time_frame_kernels")
        return dict(zip(self.FRAME_KERNELS, (float(v) for v in ms)))

    def frame_marks_begin(self, frames: int, kernels=None):
        """Bracket the kernels named in `kernels` (all 15 when None) of the next `frames` frames with
        HIP events on the streams they run on."""
        names = self.FRAME_KERNELS if kernels is None else kernels
        mask = sum(1 << self.FRAME_KERNELS.index(k) for k in names)
        self._check(self.lib.rt_frame_marks_begin(self.h, frames, mask), "rt_frame_marks_begin")

    def frame_marks_read(self):
        """({kernel: average ms over the recorded frames} for the marked kernels, frames recorded); waits."""
        ms = (C.c_float * len(self.FRAME_KERNELS))()
        n = C.c_int()
        self._check(self.lib.rt_frame_marks_read(self.h, ms, len(ms), C.byref(n)), "rt_frame_marks_read")
        return {k: float(v) for k, v in zip(self.FRAME_KERNELS, ms) if v >= 0.0}, n.value

    # ---- camera file I/O and offscreen image dumps
    def save_camera(self, path: str):
        self._check(self.lib.rt_save_camera(self.h, path.encode()), "rt_save_camera")

    def load_camera(self, path: str):
        self._check(self.lib.rt_load_camera(self.h, path.encode()), "rt_load_camera")

    def save_image(self, path: str, kind: int = IMAGE_PPM_RGBA8):
        self._check(self.lib.rt_save_image(self.h, path.encode(), kind), "rt_save_image")

    def upload_texture(self, name: str, texels: np.ndarray, set: int = 0):
        """init.cu:524-580: a 16-bit (H, W, C) level-0 image into the atlas; mips built on the device.
        set: the texture set ([scene] textureSets) whose map is replaced; 0 is the soil atlas."""
        t = np.ascontiguousarray(texels, np.uint16)
        if t.ndim not in (2, 3):
            raise ValueError("upload_texture: texels must be (H, W) or (H, W, C)")
        if not 0 <= int(set) <= 0xFFFFFFFF:
            raise ValueError("upload_texture: set must fit 32 bits")
        h, w = t.shape[:2]
        c = 1 if t.ndim == 2 else t.shape[2]
        if int(set) == 0:
            self._check(self.lib.rt_upload_texture(self.h, TEX[name], t.ctypes.data, w, h, c), "rt_upload_texture")
        else:
            self._check(self.lib.rt_upload_texture_set(self.h, int(set), TEX[name], t.ctypes.data, w, h, c),
                        "rt_upload_texture_set")

    # ---- downloads
    def download(self, name: str, dtype=np.uint8, set: int = 0) -> np.ndarray:
        """Array `name`; set: the texture set of TEX_ALBEDO_AO / TEX_NORMAL_ROUGHNESS (RT_ARR_TEX_SET)."""
        what = ARR[name]
        if set:
            if name not in ("TEX_ALBEDO_AO", "TEX_NORMAL_ROUGHNESS") or not 0 < int(set) < (1 << 22):
                raise ValueError("download: set applies to TEX_ALBEDO_AO / TEX_NORMAL_ROUGHNESS, as a small positive index")
            what |= int(set) << 8
        n = self.lib.rt_array_bytes(self.h, what)
        if n == 0 and (name.startswith("EMITTER_") or name == "PSEUDO_NORMALS"):  # an empty emitter list, or none; no table
            return np.empty(0, dtype=dtype)
        buf = np.empty(n, dtype=np.uint8)
        self._check(self.lib.rt_download(self.h, what, buf.ctypes.data, n), "rt_download(%s)" % name)
        return buf.view(dtype)

    def trace_rays(self, org, dirs, want_iters=False):
        """Closest hits of n rays (RaySceneIntersect traversal) through the queue tracer.
        Returns (t, tri, u, v[, iters], kernel_ms); tri = -1 on a miss."""
        org = np.asarray(org, np.float32).reshape(-1, 3)
        dirs = np.asarray(dirs, np.float32).reshape(-1, 3)
        n = len(org)
        rays = np.zeros((n, 8), np.float32)
        rays[:, 0:3] = org
        rays[:, 4:7] = dirs
        hits = np.zeros((n, 4), np.float32)
        iters = np.zeros(n, np.uint32) if want_iters else None
        ms = C.c_float()
        self._check(self.lib.rt_trace_rays(self.h, rays.ctypes.data, n, hits.ctypes.data, _ptr(iters), C.byref(ms)),
                    "rt_trace_rays")
        out = (hits[:, 0], hits[:, 1].view(np.int32), hits[:, 2], hits[:, 3])
        return out + ((iters,) if want_iters else ()) + (ms.value,)

    def trace_rays_device(self, org_ptr: int, dir_ptr: int, n: int, hits_ptr: int, *, org_stride: int = 3,
                          dir_stride: int = 3, iters_ptr: int | None = None, any_hit: bool = False,
                          ready_event: int | None = None, done_event: int | None = None):
        """rt_trace_rays_device: n rays from device memory (origin i at org_ptr + 4 * i * org_stride
        bytes, directions alike) into n (t, triangle bits, u, v) float32 records at hits_ptr, enqueued
        on the context stream; the host is not synchronised.  ready_event / done_event: hipEvent_t
        handles (torch.cuda.Event.cuda_event) the kernel waits for / that is recorded behind it.
        rtx.query.trace is the torch-tensor form."""
        for name, v in (("n", n), ("org_stride", org_stride), ("dir_stride", dir_stride)):
            if not 0 <= int(v) <= 0xFFFFFFFF:
                raise ValueError("trace_rays_device: %s must fit 32 bits" % name)
        q = RayQuery(org_ptr, int(org_stride), dir_ptr, int(dir_stride), int(n), hits_ptr, iters_ptr,
                     QUERY_ANY_HIT if any_hit else 0, ready_event, done_event)
        self._check(self.lib.rt_trace_rays_device(self.h, C.byref(q)), "rt_trace_rays_device")

    def trace_surfaces_device(self, org_ptr: int, dir_ptr: int, n: int, hits_ptr: int, surface_ptr: int, *,
                              org_stride: int = 3, dir_stride: int = 3, iters_ptr: int | None = None,
                              any_hit: bool = False, from_hits: bool = False, motion: bool = False,
                              ready_event: int | None = None, done_event: int | None = None):
        """rt_trace_surfaces_device: trace_rays_device's query, and behind it the surface pass that writes
        n records of 12 float32 (16 with motion) at surface_ptr: position and ray offset, geometric normal
        and its dot with the direction, shading normal and the material / front-face / hit word, and with
        motion the hit point's displacement.  from_hits: nothing is traced, the records at hits_ptr (an
        earlier query of the same rays on the same build) are read.  rtx.query.trace(surface=True) and
        rtx.query.surfaces are the torch-tensor forms."""
        for name, v in (("n", n), ("org_stride", org_stride), ("dir_stride", dir_stride)):
            if not 0 <= int(v) <= 0xFFFFFFFF:
                raise ValueError("trace_surfaces_device: %s must fit 32 bits" % name)
        rays = RayQuery(org_ptr, int(org_stride), dir_ptr, int(dir_stride), int(n), hits_ptr, iters_ptr,
                        QUERY_ANY_HIT if any_hit else 0, ready_event, done_event)
        q = SurfaceQuery(rays, surface_ptr, (SURFACE_FROM_HITS if from_hits else 0) | (SURFACE_MOTION if motion else 0))
        self._check(self.lib.rt_trace_surfaces_device(self.h, C.byref(q)), "rt_trace_surfaces_device")

    def closest_points_device(self, points_ptr: int, n: int, out_ptr: int, *, stride: int = 3,
                              max_distance: float = float("inf"), ready_event: int | None = None,
                              done_event: int | None = None):
        """rt_closest_points_device: for n points in device memory (point i at points_ptr + 4 * i * stride
        bytes) the nearest triangle of the current build within max_distance, as n records of 8 float32 at
        out_ptr: the closest point and the squared distance, then the triangle index bits, u, v and the
        feature / front / found word.  Enqueued on the context stream; the host is not synchronised.
        ready_event / done_event as in trace_rays_device.  rtx.query.closest is the torch-tensor form."""
        for name, v in (("n", n), ("stride", stride)):
            if not 0 <= int(v) <= 0xFFFFFFFF:
                raise ValueError("closest_points_device: %s must fit 32 bits" % name)
        q = ClosestQuery(points_ptr, int(stride), int(n), float(max_distance), out_ptr, ready_event, done_event)
        self._check(self.lib.rt_closest_points_device(self.h, C.byref(q)), "rt_closest_points_device")

    def signed_distance_device(self, points_ptr: int, n: int, out_ptr: int, signed_ptr: int, *, stride: int = 3,
                               max_distance: float = float("inf"), from_records: bool = False,
                               ready_event: int | None = None, done_event: int | None = None):
        """rt_signed_distance_device: closest_points_device, whose records go to out_ptr, and behind it the
        sign pass: n quads of float32 at signed_ptr, the nearest feature's pseudo-normal and the distance,
        negative inside.  from_records: out_ptr holds the records of an earlier query of the same points on
        the same build, and only the sign pass runs.  Needs signed_distance on since before the current
        build.  rtx.query.signed_distance is the torch-tensor form."""
        for name, v in (("n", n), ("stride", stride)):
            if not 0 <= int(v) <= 0xFFFFFFFF:
                raise ValueError("signed_distance_device: %s must fit 32 bits" % name)
        q = DistanceQuery(ClosestQuery(points_ptr, int(stride), int(n), float(max_distance), out_ptr, ready_event, done_event),
                          signed_ptr, DISTANCE_FROM_RECORDS if from_records else 0)
        self._check(self.lib.rt_signed_distance_device(self.h, C.byref(q)), "rt_signed_distance_device")

    def get_buffer(self, name: str, shape=None, dtype=np.uint8) -> np.ndarray:
        if shape is None:
            n = self.lib.rt_buffer_bytes(self.h, BUF[name])
            shape = (n // np.dtype(dtype).itemsize,)
        out = np.empty(shape, dtype=dtype)
        self._check(self.lib.rt_get_buffer(self.h, BUF[name], out.ctypes.data, out.nbytes), "rt_get_buffer")
        return out


def material_classes(ids) -> int:
    """rt_material_classes: the MAT_CLASS_* bits of the kernel variants a table holding these ids
    needs (mirror / glass ids: GLOSSY; id 4: MICROFACET).  Host only."""
    a = np.ascontiguousarray(ids, dtype=np.uint8).reshape(-1)
    c = C.c_uint32()
    rc = load_library().rt_material_classes(a.ctypes.data if a.size else None, a.size, C.byref(c))
    if rc != RT_OK:
        raise RtError("rt_material_classes: %s" % ERRORS.get(rc, rc))
    return c.value


def emitter_weight(xyz, emission) -> np.float32:
    """rt_emitter_weight: the emitter list's weight of the triangle xyz = v0 | v1 | v2 (9 floats) under
    `emission` (3 floats), as the device computes it in fp32.  Host only."""
    a = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1)
    e = np.ascontiguousarray(emission, dtype=np.float32).reshape(-1)
    if a.size != 9 or e.size != 3:
        raise ValueError("emitter_weight: nine position floats and three emission floats")
    w = C.c_float()
    rc = load_library().rt_emitter_weight(a.ctypes.data, e.ctypes.data, C.byref(w))
    if rc != RT_OK:
        raise RtError("rt_emitter_weight: %s" % ERRORS.get(rc, rc))
    return np.float32(w.value)


def emitter_select(cdf, r: float):
    """rt_emitter_select: (slot, prob) that r in [0, 1) selects from an inclusive float32 CDF.  Host only."""
    a = np.ascontiguousarray(cdf, dtype=np.float32).reshape(-1)
    slot, prob = C.c_uint32(), C.c_float()
    rc = load_library().rt_emitter_select(a.ctypes.data if a.size else None, a.size, float(r), C.byref(slot), C.byref(prob))
    if rc != RT_OK:
        raise RtError("rt_emitter_select: %s" % ERRORS.get(rc, rc))
    return slot.value, np.float32(prob.value)


def _environment(image, layout: int, scale: float):
    """(array kept alive, Environment) of a (height, width, 4) float32 / float16 host image."""
    a = np.asarray(image)
    if a.dtype not in (np.float32, np.float16):
        raise ValueError("environment: the image must be float32 or float16")
    if a.ndim != 3 or a.shape[2] != 4:
        raise ValueError("environment: the image must have the shape (height, width, 4)")
    if not 0 <= int(layout) <= 0xFFFFFFFF:
        raise ValueError("environment: layout must fit 32 bits")
    a = np.ascontiguousarray(a)
    fmt = ENV_FORMAT_F32X4 if a.dtype == np.float32 else ENV_FORMAT_F16X4
    return a, Environment(a.ctypes.data, a.shape[1], a.shape[0], fmt, int(layout), float(scale), None)


def _skin(rest, joints, weights, joint_count, who):
    """The rt_skin of three host arrays, which it refuses unless they are what the library reads."""
    for a, dt, cols, name in ((rest, np.float32, 3, "rest"), (joints, np.uint16, 4, "joints"), (weights, np.float32, 4, "weights")):
        if not isinstance(a, np.ndarray) or a.dtype != dt or a.ndim != 2 or a.shape[1] != cols:
            raise ValueError("%s: %s must be an (n, %d) %s array" % (who, name, cols, np.dtype(dt).name))
        if not a.flags["C_CONTIGUOUS"]:
            raise ValueError("%s: %s must be C-contiguous" % (who, name))
    if not len(rest) == len(joints) == len(weights) or len(rest) > 0xFFFFFFFF:
        raise ValueError("%s: rest, joints and weights must have one row per vertex" % who)
    if not 0 <= int(joint_count) <= 0xFFFFFFFF:
        raise ValueError("%s: joint_count must fit 32 bits" % who)
    return Skin(rest.ctypes.data, joints.ctypes.data, weights.ctypes.data, len(rest), int(joint_count))


def _pose_matrices(matrices, who):
    """A pose's host matrices as a (J, 12) view, refused unless C-contiguous float32 (J, 3, 4) or (J, 12)."""
    m = matrices
    if not isinstance(m, np.ndarray) or m.dtype != np.float32 or not (
            (m.ndim == 3 and m.shape[1:] == (3, 4)) or (m.ndim == 2 and m.shape[1] == 12)):
        raise ValueError("%s: matrices must be a (J, 3, 4) or (J, 12) float32 array" % who)
    if not m.flags["C_CONTIGUOUS"]:
        raise ValueError("%s: matrices must be C-contiguous" % who)
    if len(m) > 0xFFFFFFFF:
        raise ValueError("%s: the joint count must fit 32 bits" % who)
    return m.reshape(len(m), 12)


def skin_vertices(rest, joints, weights, matrices) -> np.ndarray:
    """rt_skin_vertices: the skinning rule on the host (no context, no device), the positions a pose of
    `matrices` gives the skin, bit for bit what the device computes.  The joint count is len(matrices)."""
    m = _pose_matrices(matrices, "skin_vertices")
    s = _skin(rest, joints, weights, len(m), "skin_vertices")
    out = np.zeros((len(rest), 3), np.float32)
    rc = load_library().rt_skin_vertices(C.byref(s), m.ctypes.data, out.ctypes.data)
    if rc != RT_OK:
        raise RtError("rt_skin_vertices: %s" % ERRORS.get(rc, rc))
    return out


def point_triangle(p, triangle) -> np.ndarray:
    """rt_point_triangle: the closest-point rule on the host (no context, no device) for one point and one
    triangle ((3, 3): v1, v2, v3): the 8-float record with triangle index 0, bit for bit the device's."""
    p = np.ascontiguousarray(p, np.float32)
    t = np.ascontiguousarray(triangle, np.float32)
    if p.shape != (3,) or t.size != 9:
        raise ValueError("point_triangle: p is (3,), triangle is (3, 3)")
    out = np.zeros(8, np.float32)
    rc = load_library().rt_point_triangle(p.ctypes.data, t.ctypes.data, out.ctypes.data)
    if rc != RT_OK:
        raise RtError("rt_point_triangle: %s" % ERRORS.get(rc, rc))
    return out


def closest_points_host(triangles, points, *, ids=None, max_distance: float = float("inf")) -> np.ndarray:
    """rt_closest_points_host: the definition of a closest-point query's answer, exhaustively on the host:
    triangles (ntri, 3, 3), points (n, 3), ids (ntri,) the index each triangle is reported under (None:
    its row).  Returns the (n, 8) float32 records; on equal squared distances the lower id wins."""
    t = np.ascontiguousarray(triangles, np.float32).reshape(-1, 9)
    p = np.ascontiguousarray(points, np.float32)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError("closest_points_host: points is (n, 3)")
    i = None
    if ids is not None:
        i = np.ascontiguousarray(ids, np.uint32)
        if i.shape != (len(t),):
            raise ValueError("closest_points_host: ids holds one index per triangle")
    out = np.zeros((len(p), 8), np.float32)
    rc = load_library().rt_closest_points_host(t.ctypes.data if len(t) else None, None if i is None else i.ctypes.data,
                                               len(t), p.ctypes.data if len(p) else None, len(p),
                                               float(max_distance), out.ctypes.data if len(p) else None)
    if rc != RT_OK:
        raise RtError("rt_closest_points_host: %s" % ERRORS.get(rc, rc))
    return out


def pseudo_normals(vertices, indices) -> np.ndarray:
    """rt_pseudo_normals: the pseudo-normal table of a mesh on the host (no context, no device): vertices
    (nv, 3), indices (ntri, 3).  Returns (ntri, 6, 4) float32: per triangle vertex 1 2 3, edge 12 23 31,
    .w = 0; bit for bit what download("PSEUDO_NORMALS") gives for a build of the same mesh."""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    i = np.ascontiguousarray(indices, np.uint32).reshape(-1, 3)
    out = np.zeros((len(i), 6, 4), np.float32)
    rc = load_library().rt_pseudo_normals(v.ctypes.data if len(v) else None, len(v), i.ctypes.data if len(i) else None,
                                          len(i), out.ctypes.data if len(i) else None)
    if rc != RT_OK:
        raise RtError("rt_pseudo_normals: %s" % ERRORS.get(rc, rc))
    return out


def signed_distance_rule(points, records, vertices, indices, table) -> np.ndarray:
    """rt_signed_distance_rule for every point: points (n, 3), their closest records (n, 8), the mesh and
    its table (pseudo_normals or download("PSEUDO_NORMALS")).  Returns (n, 4) float32: the nearest
    feature's pseudo-normal and the signed distance (negative inside); a miss gives (0, 0, 0, inf).  A
    record whose triangle index is not below the table's triangle count is finished as a miss, as the
    device query does."""
    p = np.ascontiguousarray(points, np.float32)
    r = np.ascontiguousarray(records, np.float32)
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    idx = np.ascontiguousarray(indices, np.uint32).reshape(-1, 3)
    t = np.ascontiguousarray(table, np.float32).reshape(-1, 24)
    if p.ndim != 2 or p.shape[1] != 3 or r.shape != (len(p), 8):
        raise ValueError("signed_distance_rule: points is (n, 3), records is (n, 8)")
    if len(t) > len(idx):
        raise ValueError("signed_distance_rule: the table has more triangles than the mesh")
    lib = load_library()
    out = np.zeros((len(p), 4), np.float32)
    tri = r.view(np.uint32)[:, 4]
    miss = np.array([0.0, 0.0, 0.0, np.inf], np.float32)
    for k in range(len(p)):
        if tri[k] >= len(t):
            out[k] = miss
            continue
        xyz = np.ascontiguousarray(v[idx[tri[k]]]).reshape(9)
        rc = lib.rt_signed_distance_rule(p[k].ctypes.data, r[k].ctypes.data, xyz.ctypes.data, t[tri[k]].ctypes.data,
                                         out[k].ctypes.data)
        if rc != RT_OK:
            raise RtError("rt_signed_distance_rule: %s" % ERRORS.get(rc, rc))
    return out


def environment_table(image, layout: int, scale: float = 1.0):
    """rt_environment_table: (table (256, 512, 4) float32, pdf (256, 512) float32) that `image` gives as an
    environment, the rule the device matches bit for bit.  Host only: no context, no device."""
    a, e = _environment(image, layout, scale)
    table = np.empty((ENV_TABLE_H, ENV_TABLE_W, 4), np.float32)
    pdf = np.empty((ENV_TABLE_H, ENV_TABLE_W), np.float32)
    rc = load_library().rt_environment_table(C.byref(e), table.ctypes.data, pdf.ctypes.data)
    if rc != RT_OK:
        raise RtError("rt_environment_table: %s" % ERRORS.get(rc, rc))
    return table, pdf


def default_material(id: int) -> Material:
    """rt_default_material: the reference's meaning of material id 0..255.  Host only."""
    if not 0 <= int(id) <= 0xFFFFFFFF:
        raise ValueError("default_material: id must fit 32 bits")
    m = Material()
    rc = load_library().rt_default_material(int(id), C.byref(m))
    if rc != RT_OK:
        raise RtError("rt_default_material: %s" % ERRORS.get(rc, rc))
    return m


def mesh_adjacency(indices_padded, nv: int):
    """rt_mesh_adjacency: (adj_offsets[nv + 1], adj_corners[3 NP], corner_slots[3 NP]) of a padded
    index array, the vertex -> corner adjacency rt_init builds and set_mesh reproduces.  Host only."""
    a = np.ascontiguousarray(indices_padded, dtype=np.uint32).reshape(-1)
    if a.size % 3:
        raise ValueError("mesh_adjacency: three indices per triangle")
    off = np.empty(int(nv) + 1, np.uint32)
    corners = np.empty(a.size, np.uint32)
    slots = np.empty(a.size, np.uint32)
    rc = load_library().rt_mesh_adjacency(a.ctypes.data, a.size // 3, int(nv), off.ctypes.data, corners.ctypes.data,
                                          slots.ctypes.data)
    if rc != RT_OK:
        raise RtError("rt_mesh_adjacency: %s" % ERRORS.get(rc, rc))
    return off, corners, slots


def _ptr(a):
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data
