"""ctypes mirror of ``include/dcrt.h`` (the C ABI of the MI355X tracer).

Only plain C types cross the boundary; numpy is used for host views of the
flattened scene buffers. Loading fails loudly when the native library is
missing: there is no CPU fallback for the product path.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

PKG_DIR = Path(__file__).resolve().parent
LIB_PATH = PKG_DIR / "libdcrt.so"

# ---- status codes / flags (dcrt.h) -----------------------------------------
DCRT_OK = 0
ABI_VERSION = 6         # DCRT_ABI_VERSION: load_library refuses a libdcrt.so of another
ERRORS = {-1: "DCRT_E_INVALID_ARG", -2: "DCRT_E_HIP", -3: "DCRT_E_NO_SCENE", -4: "DCRT_E_IO",
          -5: "DCRT_E_LIMIT", -6: "DCRT_E_NO_DEVICE"}
LIGHT_INDEX_INVALID = 0xFFFFFFFF
FEATURE_GGX_SAMPLE_VNDF = 0x01
FEATURE_NO_FRONT_TO_BACK = 0x02
FEATURE_LIGHT_VISIBLE = 0x04
FEATURE_WATERTIGHT = 0x08
FEATURE_ALLOW_ANYHIT = 0x10
FEATURE_DEFAULT = FEATURE_GGX_SAMPLE_VNDF | FEATURE_LIGHT_VISIBLE | FEATURE_WATERTIGHT
# dcrt_tracer_cast_rays' out_variant (DCRT_CAST_VARIANT_*)
CAST_VARIANT = {"opacity": 0x01, "all_cached": 0x02, "pair": 0x04, "ident": 0x08, "ring": 0x10, "flat": 0x20}
FILTER_BOX, FILTER_TRIANGLE, FILTER_GAUSSIAN, FILTER_MITCHELL, FILTER_LANCZOS = range(5)
MATERIAL_DIFFUSE, MATERIAL_PLASTIC, MATERIAL_CONDUCTOR, MATERIAL_DIELECTRIC, MATERIAL_THIN_DIELECTRIC = range(5)
MAX_LIGHT_COUNT = 5000
# DCRT_DIRTY_*: what dcrt_scene_acquire_dirty reports
DIRTY_LIGHTS = 0x01
DIRTY_MATERIALS = 0x02
DIRTY_INSTANCE_FLAGS = 0x04
DIRTY_CAMERA = 0x08
DIRTY_SCENE = 0x10
# DCRT_OUTPUT_*: the megakernel tracer's "Output" views, in s_OutputNames order
(OUTPUT_PATH_TRACING, OUTPUT_SHADING_NORMAL, OUTPUT_SHADING_TANGENT, OUTPUT_ALBEDO, OUTPUT_NEGATIVE_NDOTV,
 OUTPUT_BACKFACE, OUTPUT_ITERATION_COUNT) = range(7)


class Vertex(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("normal", C.c_float * 3), ("tangent", C.c_float * 3),
                ("texcoord", C.c_float * 2)]


class BVHNode(C.Structure):
    _fields_ = [("bbox_min", C.c_float * 3), ("bbox_max", C.c_float * 3), ("right_child_or_prim_index", C.c_uint32),
                ("misc", C.c_uint32)]


class Material(C.Structure):
    _fields_ = [("albedo", C.c_float * 3), ("albedo_texture_index", C.c_int32), ("ior", C.c_float * 3),
                ("roughness", C.c_float), ("tex_tiling", C.c_float * 2), ("opacity", C.c_float),
                ("flags", C.c_uint32), ("opacity_texture_index", C.c_int32)]


class Light(C.Structure):
    _fields_ = [("radiance", C.c_float * 3), ("position_or_triangle_range", C.c_float * 3), ("flags", C.c_uint32)]


class Float4x3(C.Structure):
    _fields_ = [("m", C.c_float * 12)]


class Texture(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("format", C.c_uint32),
                ("pixels", C.POINTER(C.c_uint8))]


class FlatScene(C.Structure):
    _fields_ = [
        ("vertices", C.POINTER(Vertex)), ("vertex_count", C.c_uint32),
        ("triangles", C.POINTER(C.c_uint32)), ("triangle_count", C.c_uint32),
        ("bvh_nodes", C.POINTER(BVHNode)), ("bvh_node_count", C.c_uint32),
        ("tlas_node_count", C.c_uint32),
        ("material_ids", C.POINTER(C.c_uint32)),
        ("instance_transforms", C.POINTER(Float4x3)), ("instance_count", C.c_uint32),
        ("instance_light_indices", C.POINTER(C.c_uint32)),
        ("instance_flags", C.POINTER(C.c_uint32)),
        ("instance_material_overrides", C.POINTER(C.c_uint32)),
        ("materials", C.POINTER(Material)), ("material_count", C.c_uint32),
        ("lights", C.POINTER(Light)), ("light_count", C.c_uint32),
        ("environment_light_index", C.c_uint32),
        ("textures", C.POINTER(Texture)), ("texture_count", C.c_uint32),
        ("env_cube_rgb", C.POINTER(C.c_float)), ("env_cube_size", C.c_uint32),
        ("bvh_traversal_stack_size", C.c_uint32),
    ]


class BxDFLuts(C.Structure):
    _fields_ = [("brdf", C.c_uint16 * (32 * 32)), ("brdf_avg", C.c_uint16 * 32),
                ("brdf_dielectric", C.c_uint16 * (32 * 16 * 32)), ("brdf_dielectric_avg", C.c_uint16 * (16 * 16 * 2)),
                ("bsdf", C.c_uint16 * (32 * 16 * 32)), ("bsdf_avg", C.c_uint16 * (16 * 16 * 2))]


class FrameParams(C.Structure):
    _fields_ = [("camera_transform", C.c_float * 16), ("resolution", C.c_uint32 * 2), ("film_size", C.c_float * 2),
                ("aperture_radius", C.c_float), ("focal_distance", C.c_float), ("film_distance", C.c_float),
                ("blade_count", C.c_uint32), ("blade_vertex_pos", C.c_float * 2), ("aperture_base_angle", C.c_float),
                ("frame_seed", C.c_uint32), ("max_bounce_count", C.c_uint32), ("light_count", C.c_uint32),
                ("environment_light_index", C.c_uint32), ("features", C.c_uint32)]


class FilterParams(C.Structure):
    _fields_ = [("filter", C.c_uint32), ("radius", C.c_float), ("gaussian_alpha", C.c_float),
                ("mitchell_b", C.c_float), ("mitchell_c", C.c_float), ("lanczos_tau", C.c_uint32)]


class Ray(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("t_max", C.c_float), ("direction", C.c_float * 3), ("t_min", C.c_float)]


class RayHit(C.Structure):
    _fields_ = [("t", C.c_float), ("u", C.c_float), ("v", C.c_float), ("triangle_id", C.c_uint32),
                ("instance_index", C.c_uint32)]


class PostFxParams(C.Structure):
    _fields_ = [("enabled", C.c_int32), ("auto_exposure", C.c_int32), ("ev100", C.c_float), ("luminance_white", C.c_float)]


class TracerConfig(C.Structure):
    _fields_ = [("path_pool_size", C.c_uint32), ("iterations_per_render", C.c_uint32), ("device", C.c_int32),
                ("stream", C.c_void_p), ("debug_rng", C.c_uint32)]


class OutputParams(C.Structure):
    _fields_ = [("output_type", C.c_uint32), ("iteration_threshold", C.c_uint32)]


class DenoiseParams(C.Structure):
    """dcrt_denoise_params; dcrt_denoise_default_params fills in 5, 4.0, 0.2, 0.1, 1."""
    _fields_ = [("iterations", C.c_uint32), ("sigma_luminance", C.c_float), ("sigma_normal", C.c_float),
                ("sigma_albedo", C.c_float), ("demodulate", C.c_uint32)]


class FireflyParams(C.Structure):
    """dcrt_firefly_params (dcrt.h "firefly re-weighting"); dcrt_firefly_default_params fills in 6, 1.0, 8.0, 3.0."""
    _fields_ = [("cascades", C.c_uint32), ("start", C.c_float), ("base", C.c_float), ("min_support", C.c_float)]


class NoiseStats(C.Structure):
    """dcrt_noise_stats: the half-film noise estimate of a film (dcrt.h "film noise estimate")."""
    _fields_ = [("images", C.c_uint32), ("valid_pixels", C.c_uint32), ("converged_pixels", C.c_uint32),
                ("mean_error", C.c_float), ("max_error", C.c_float), ("max_tile_error", C.c_float)]


class ConvergeParams(C.Structure):
    """dcrt_converge_params of dcrt_tracer_render_converged."""
    _fields_ = [("threshold", C.c_float), ("target_fraction", C.c_float), ("min_images", C.c_uint32),
                ("max_images", C.c_uint32), ("check_interval", C.c_uint32)]


class AdaptiveReport(C.Structure):
    """dcrt_adaptive_report of dcrt_tracer_render_adaptive."""
    _fields_ = [("images", C.c_uint32), ("check_points", C.c_uint32), ("pixel_samples", C.c_uint64),
                ("active_blocks", C.c_uint32), ("total_blocks", C.c_uint32)]


class RayStats(C.Structure):
    _fields_ = [("extension_rays", C.c_uint64), ("shadow_rays", C.c_uint64), ("new_paths", C.c_uint64),
                ("iterations", C.c_uint64), ("images_completed", C.c_uint64), ("early_finished", C.c_uint64)]


class FilmPartition(C.Structure):
    _fields_ = [("world_size", C.c_uint32), ("rank", C.c_uint32), ("stripe_height", C.c_uint32),
                ("halo_rows", C.c_uint32)]


class TraversalStats(C.Structure):
    _fields_ = [("ext_node_visits", C.c_uint64), ("ext_triangle_tests", C.c_uint64), ("ext_blas_entries", C.c_uint64),
                ("shadow_node_visits", C.c_uint64), ("shadow_triangle_tests", C.c_uint64),
                ("shadow_blas_entries", C.c_uint64), ("ext_launches", C.c_uint64), ("ext_kernel_ms", C.c_double),
                ("ext_max_node_visits", C.c_uint64), ("shadow_max_node_visits", C.c_uint64),
                ("material_launches", C.c_uint64), ("material_kernel_ms", C.c_double),
                ("control_launches", C.c_uint64), ("control_kernel_ms", C.c_double)]


class TracerInfo(C.Structure):
    _fields_ = [("path_pool_size", C.c_uint32), ("scene_in_lds", C.c_uint32), ("cached_nodes", C.c_uint32),
                ("cached_triangles", C.c_uint32), ("cast_block", C.c_uint32), ("traversal_stack", C.c_uint32),
                ("material_generic", C.c_uint32), ("pair_traversal", C.c_uint32), ("control_grid", C.c_uint32),
                ("material_grid", C.c_uint32), ("cast_grid", C.c_uint32), ("material_lds", C.c_uint32),
                ("cast_identity", C.c_uint32), ("stack_lds_rows", C.c_uint32), ("ring_rows", C.c_uint32),
                ("cast_waves_per_cu", C.c_uint32), ("shadow_cells", C.c_uint32), ("shadow_cell_max_leaves", C.c_uint32),
                ("shadow_cell_mean_leaves", C.c_float), ("shadow_inline", C.c_uint32), ("shading_tables", C.c_uint32),
                ("dielectric_row_bytes", C.c_uint32), ("dielectric_row_lds", C.c_uint32), ("frame_table_bytes", C.c_uint32),
                ("early_finish", C.c_uint32)]


class ShadowCellsInfo(C.Structure):
    _fields_ = [("resolution", C.c_uint32), ("leaf_count", C.c_uint32), ("node_count", C.c_uint32),
                ("max_leaves", C.c_uint32), ("mean_leaves", C.c_float), ("r0", C.c_float)]


class UploadStats(C.Structure):
    _fields_ = [("scene_uploads", C.c_uint64), ("material_updates", C.c_uint64), ("light_updates", C.c_uint64),
                ("instance_flag_updates", C.c_uint64), ("geometry_bytes", C.c_uint64), ("shading_bytes", C.c_uint64),
                ("graph_invalidations", C.c_uint64)]


class MaterialSetting(C.Structure):
    _fields_ = [("albedo", C.c_float * 3), ("roughness", C.c_float), ("ior", C.c_float * 3), ("opacity", C.c_float),
                ("k", C.c_float * 3), ("tiling", C.c_float * 2), ("material_type", C.c_uint32),
                ("albedo_texture_index", C.c_int32), ("opacity_texture_index", C.c_int32),
                ("internal_scattering_mode", C.c_uint32), ("multiscattering", C.c_uint32),
                ("is_two_sided", C.c_uint32), ("has_roughness_texture", C.c_uint32)]


class SceneSettings(C.Structure):
    _fields_ = [("resolution", C.c_uint32 * 2), ("max_bounce_count", C.c_uint32), ("camera_type", C.c_uint32),
                ("fov_x", C.c_float), ("focal_length", C.c_float), ("focal_distance", C.c_float),
                ("relative_aperture", C.c_float), ("aperture_blade_count", C.c_uint32), ("aperture_rotation", C.c_float),
                ("film_size", C.c_float * 2), ("camera_position", C.c_float * 3), ("camera_euler_angles", C.c_float * 3),
                ("features", C.c_uint32), ("has_environment_light", C.c_uint32), ("environment_color", C.c_float * 3),
                ("env_cube_rgb", C.POINTER(C.c_float)), ("env_cube_size", C.c_uint32),
                ("mesh_light_count", C.c_uint32), ("punctual_light_count", C.c_uint32),
                ("material_count", C.c_uint32), ("texture_count", C.c_uint32)]


class ObjMesh(C.Structure):
    _fields_ = [("vertices", C.POINTER(Vertex)), ("vertex_count", C.c_uint32), ("indices", C.POINTER(C.c_uint32)),
                ("material_ids", C.POINTER(C.c_uint32)), ("triangle_count", C.c_uint32)]


class ObjMaterial(C.Structure):
    _fields_ = [("albedo", C.c_float * 3), ("ior", C.c_float), ("roughness", C.c_float), ("opacity", C.c_float),
                ("albedo_texture_index", C.c_int32), ("opacity_texture_index", C.c_int32)]


class BsdfProbeMaterial(C.Structure):
    _fields_ = [("type", C.c_uint32), ("albedo", C.c_float * 3), ("ior", C.c_float * 3), ("alpha", C.c_float),
                ("two_sided", C.c_uint32), ("multiscattering", C.c_uint32), ("internal_scattering_mode", C.c_uint32)]


class RouletteParams(C.Structure):
    """dcrt_roulette_params (dcrt.h "Russian roulette")."""
    _fields_ = [("enable", C.c_uint32), ("start_bounce", C.c_uint32), ("min_survival", C.c_float), ("max_survival", C.c_float)]


class LightTableInfo(C.Structure):
    """dcrt_light_table_info (dcrt.h "light selection")."""
    _fields_ = [("light_count", C.c_uint32), ("triangle_entries", C.c_uint32), ("scene_radius", C.c_double), ("total_weight", C.c_double)]


OBJ_SCENE_LAYOUT = 1

# Every symbol include/dcrt.h declares: (name, restype, argtypes)
_P = C.c_void_p
_I = C.c_int
_U = C.c_uint32
_FP = C.POINTER(C.c_float)
SIGNATURES = [
    ("dcrt_abi_version", _I, []),
    ("dcrt_version", C.c_char_p, []),
    ("dcrt_last_error", C.c_char_p, []),
    ("dcrt_device_count", _I, [C.POINTER(C.c_int)]),
    ("dcrt_scene_create", _I, [C.POINTER(_P)]),
    ("dcrt_scene_destroy", None, [_P]),
    ("dcrt_scene_reset", _I, [_P, _U, _U]),
    ("dcrt_scene_load_from_file", _I, [_P, C.c_char_p]),
    ("dcrt_scene_add_punctual_light", _I, [_P, _FP, _FP, _FP, _I]),
    ("dcrt_scene_set_punctual_light", _I, [_P, _U, _FP, _FP, _FP, _I]),
    ("dcrt_scene_remove_punctual_light", _I, [_P, _U]),
    ("dcrt_scene_remove_environment_light", _I, [_P]),
    ("dcrt_scene_acquire_dirty", _I, [_P, C.POINTER(C.c_uint32)]),
    ("dcrt_scene_flatten", _I, [_P]),
    ("dcrt_scene_set_environment_light", _I, [_P, _FP, _FP, _U]),
    ("dcrt_scene_set_camera", _I, [_P, _FP, _FP]),
    ("dcrt_scene_set_lens", _I, [_P, _I, C.c_float, C.c_float, C.c_float, C.c_float, _U, C.c_float, _FP]),
    ("dcrt_scene_set_max_bounce", _I, [_P, _U]),
    ("dcrt_scene_set_filter", _I, [_P, C.POINTER(FilterParams)]),
    ("dcrt_scene_get_filter", _I, [_P, C.POINTER(FilterParams)]),
    ("dcrt_scene_get_resolution", _I, [_P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    ("dcrt_scene_get_material_count", _I, [_P, C.POINTER(C.c_uint32)]),
    ("dcrt_scene_set_material", _I, [_P, _U, _I, _FP, C.c_float, _FP, _FP, _I, _I]),
    ("dcrt_scene_set_material_opacity", _I, [_P, _U, C.c_float, C.c_int32]),
    ("dcrt_scene_get_material_setting", _I, [_P, _U, C.POINTER(MaterialSetting)]),
    ("dcrt_scene_set_material_multiscattering", _I, [_P, _U, _I]),
    ("dcrt_scene_get_settings", _I, [_P, C.POINTER(SceneSettings)]),
    ("dcrt_scene_get_mesh_light", _I, [_P, _U, C.POINTER(C.c_uint32), _FP]),
    ("dcrt_scene_get_punctual_light", _I, [_P, _U, _FP, _FP, _FP, C.POINTER(C.c_int)]),
    ("dcrt_scene_get_instance_material_override", _I, [_P, _U, C.POINTER(C.c_uint32)]),
    ("dcrt_scene_set_features", _I, [_P, _U]),
    ("dcrt_scene_get_features", _I, [_P, C.POINTER(C.c_uint32)]),
    ("dcrt_scene_get_flat", _I, [_P, C.POINTER(FlatScene)]),
    ("dcrt_scene_get_frame_params", _I, [_P, _U, C.POINTER(FrameParams)]),
    ("dcrt_scene_get_bvh_info", _I, [_P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    ("dcrt_bvh_build_blas", _I, [C.POINTER(Vertex), C.POINTER(C.c_uint32), _U, C.POINTER(BVHNode),
                                 C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                 C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    ("dcrt_scene_get_content_counts", _I, [_P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    ("dcrt_scene_get_loaded_mesh", _I, [_P, _U, C.POINTER(ObjMesh)]),
    ("dcrt_scene_get_instance", _I, [_P, _U, C.POINTER(C.c_uint32), _FP]),
    ("dcrt_obj_load", _I, [C.c_char_p, _U, _U, C.POINTER(_P)]),
    ("dcrt_obj_mesh_count", _I, [_P, C.POINTER(C.c_uint32)]),
    ("dcrt_obj_get_mesh", _I, [_P, _U, C.POINTER(ObjMesh)]),
    ("dcrt_obj_material_count", _I, [_P, C.POINTER(C.c_uint32)]),
    ("dcrt_obj_get_material", _I, [_P, _U, C.POINTER(ObjMaterial)]),
    ("dcrt_obj_free", None, [_P]),
    ("dcrt_xml_dump_tree", _I, [C.c_char_p, C.c_char_p, _U, C.POINTER(C.c_uint32)]),
    ("dcrt_tracer_create", _I, [C.POINTER(TracerConfig), C.POINTER(_P)]),
    ("dcrt_tracer_destroy", None, [_P]),
    ("dcrt_tracer_upload_scene", _I, [_P, C.POINTER(FlatScene)]),
    ("dcrt_tracer_update_materials", _I, [_P, C.POINTER(Material), _U]),
    ("dcrt_tracer_update_lights", _I, [_P, C.POINTER(Light), _U]),
    ("dcrt_tracer_update_instance_flags", _I, [_P, C.POINTER(C.c_uint32), _U]),
    ("dcrt_tracer_upload_stats", _I, [_P, C.POINTER(UploadStats)]),
    ("dcrt_tracer_set_frame_params", _I, [_P, C.POINTER(FrameParams)]),
    ("dcrt_tracer_set_film_partition", _I, [_P, C.POINTER(FilmPartition)]),
    ("dcrt_tracer_set_film_bands", _I, [_P, C.POINTER(C.c_uint32), _U, _U]),
    ("dcrt_tracer_set_row_cost_probe", _I, [_P, _I]),
    ("dcrt_tracer_read_row_cost", _I, [_P, C.POINTER(C.c_uint32)]),
    ("dcrt_tracer_render", _I, [_P, _U]),
    ("dcrt_tracer_render_images", _I, [_P, _U, _U, C.POINTER(FilterParams)]),
    ("dcrt_tracer_render_images_strided", _I, [_P, _U, _U, _U, _I, C.POINTER(FilterParams)]),
    ("dcrt_tracer_image_sample_ptrs", _I, [_P, _U, C.POINTER(_P), C.POINTER(_P)]),
    ("dcrt_tracer_accumulate_images", _I, [_P, C.POINTER(_P), C.POINTER(_P), _U, C.POINTER(FilterParams)]),
    ("dcrt_tracer_set_mode", _I, [_P, _I]),
    ("dcrt_tracer_set_output", _I, [_P, C.POINTER(OutputParams)]),
    ("dcrt_tracer_get_output", _I, [_P, C.POINTER(OutputParams)]),
    ("dcrt_tracer_set_image_batch", _I, [_P, C.c_uint32]),
    ("dcrt_tracer_reset_image", _I, [_P]),
    ("dcrt_tracer_is_image_complete", _I, [_P, C.POINTER(C.c_int)]),
    ("dcrt_tracer_acquire_film_clear_trigger", _I, [_P, C.POINTER(C.c_int)]),
    ("dcrt_tracer_clear_film", _I, [_P]),
    ("dcrt_tracer_accumulate_film", _I, [_P, C.POINTER(FilterParams)]),
    ("dcrt_tracer_read_film", _I, [_P, _FP]),
    ("dcrt_tracer_read_samples", _I, [_P, _FP, _FP]),
    ("dcrt_tracer_read_rng", _I, [_P, C.POINTER(C.c_uint32)]),
    ("dcrt_tracer_film_device_ptr", _I, [_P, C.POINTER(_P)]),
    ("dcrt_tracer_sample_device_ptrs", _I, [_P, C.POINTER(_P), C.POINTER(_P)]),
    ("dcrt_tracer_copy_film_device", _I, [_P, _P]),
    ("dcrt_tracer_add_film_device", _I, [_P, _P]),
    ("dcrt_tracer_prepare_images", _I, [_P, C.c_uint32]),
    ("dcrt_tracer_counters", _I, [_P, C.POINTER(RayStats)]),
    ("dcrt_tracer_set_instrumentation", _I, [_P, _I, _I]),
    ("dcrt_tracer_traversal_stats", _I, [_P, C.POINTER(TraversalStats)]),
    ("dcrt_tracer_reset_stats", _I, [_P]),
    ("dcrt_tracer_get_info", _I, [_P, C.POINTER(TracerInfo)]),
    ("dcrt_tracer_debug_ring_spills", _I, [_P, C.POINTER(C.c_uint64)]),
    ("dcrt_tracer_synchronize", _I, [_P]),
    ("dcrt_tracer_get_luts", _I, [_P, C.POINTER(BxDFLuts)]),
    ("dcrt_tracer_set_luts", _I, [_P, C.POINTER(BxDFLuts)]),
    ("dcrt_tracer_trace_rays", _I, [_P, C.POINTER(Ray), _U, C.POINTER(RayHit), _U]),
    ("dcrt_tracer_occluded", _I, [_P, C.POINTER(Ray), _U, C.POINTER(C.c_uint32), _U]),
    ("dcrt_tracer_cast_rays", _I, [_P, C.POINTER(Ray), C.POINTER(C.c_uint32), _FP, _U, _U, C.POINTER(RayHit), C.POINTER(C.c_uint32),
                                   C.POINTER(C.c_uint32)]),
    ("dcrt_tracer_trace_rays_device", _I, [_P, _P, _U, _P, _U]),
    ("dcrt_tracer_trace_occlusion_cells", _I, [_P, C.POINTER(Ray), _U, C.POINTER(C.c_uint32), _U]),
    ("dcrt_shadow_cells_build", _I, [C.POINTER(FlatScene), _U, C.POINTER(ShadowCellsInfo), C.POINTER(C.c_uint64),
                                     C.POINTER(C.c_uint32), C.POINTER(BVHNode), _U]),
    ("dcrt_shadow_cell_indices", _I, [_U, _FP, _U, C.POINTER(C.c_uint32)]),
    ("dcrt_scene_get_postfx_params", _I, [_P, C.POINTER(PostFxParams)]),
    ("dcrt_srgb_encode_thresholds", _I, [_FP]),
    ("dcrt_tracer_resolve_image", _I, [_P, C.POINTER(PostFxParams), C.POINTER(C.c_uint8), _FP]),
    ("dcrt_denoise_default_params", _I, [C.POINTER(DenoiseParams)]),
    ("dcrt_tracer_render_guides", _I, [_P, _U, _U]),
    ("dcrt_tracer_guide_device_ptrs", _I, [_P, C.POINTER(_P), C.POINTER(_P)]),
    ("dcrt_tracer_read_guides", _I, [_P, _FP, _FP]),
    ("dcrt_tracer_denoise", _I, [_P, C.POINTER(DenoiseParams)]),
    ("dcrt_tracer_denoise_device", _I, [_P, C.POINTER(DenoiseParams), _U, _U, _P, _P, _P, _P]),
    ("dcrt_tracer_denoise_images", _I, [_P, C.POINTER(DenoiseParams), _U, _U, _FP, _FP, _FP, _FP]),
    ("dcrt_tracer_read_denoised", _I, [_P, _FP]),
    ("dcrt_tracer_denoised_device_ptr", _I, [_P, C.POINTER(_P)]),
    ("dcrt_tracer_resolve_denoised", _I, [_P, C.POINTER(PostFxParams), C.POINTER(C.c_uint8), _FP]),
    ("dcrt_tracer_denoise_timings", _I, [_P, _FP, _U, C.POINTER(C.c_uint32)]),
    ("dcrt_firefly_default_params", _I, [C.POINTER(FireflyParams)]),
    ("dcrt_tracer_set_firefly", _I, [_P, C.POINTER(FireflyParams)]),
    ("dcrt_tracer_get_firefly", _I, [_P, C.POINTER(C.c_int), C.POINTER(FireflyParams)]),
    ("dcrt_tracer_firefly_resolve", _I, [_P]),
    ("dcrt_tracer_read_firefly", _I, [_P, _FP]),
    ("dcrt_tracer_firefly_device_ptr", _I, [_P, C.POINTER(_P)]),
    ("dcrt_tracer_resolve_firefly", _I, [_P, C.POINTER(PostFxParams), C.POINTER(C.c_uint8), _FP]),
    ("dcrt_tracer_denoise_firefly", _I, [_P, C.POINTER(DenoiseParams)]),
    ("dcrt_tracer_read_cascades", _I, [_P, _FP]),
    ("dcrt_tracer_cascade_device_ptrs", _I, [_P, C.POINTER(_P), _U, C.POINTER(C.c_uint32)]),
    ("dcrt_tracer_firefly_resolve_device", _I, [_P, C.POINTER(FireflyParams), _U, _U, _U, _P, C.POINTER(_P), _P]),
    ("dcrt_tracer_firefly_timings", _I, [_P, _FP, _FP]),
    ("dcrt_tracer_set_convergence", _I, [_P, _I]),
    ("dcrt_tracer_film_image_count", _I, [_P, C.POINTER(C.c_uint32)]),
    ("dcrt_tracer_half_film_device_ptr", _I, [_P, C.POINTER(_P)]),
    ("dcrt_tracer_read_half_film", _I, [_P, _FP]),
    ("dcrt_tracer_add_half_film_device", _I, [_P, _P]),
    ("dcrt_tracer_noise", _I, [_P, C.c_float, C.POINTER(NoiseStats)]),
    ("dcrt_tracer_noise_device", _I, [_P, _U, _U, _P, _P, C.c_float, _P, _P, C.POINTER(NoiseStats)]),
    ("dcrt_tracer_film_pass_timing", _I, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
    ("dcrt_tracer_noise_map_device_ptrs", _I, [_P, C.POINTER(_P), C.POINTER(_P)]),
    ("dcrt_tracer_read_noise_maps", _I, [_P, _FP, _FP]),
    ("dcrt_tracer_render_converged", _I, [_P, _U, C.POINTER(ConvergeParams), C.POINTER(FilterParams), C.POINTER(NoiseStats),
                                          C.POINTER(C.c_int)]),
    ("dcrt_tracer_set_adaptive", _I, [_P, _I]),
    ("dcrt_tracer_set_sample_blocks", _I, [_P, C.POINTER(C.c_uint32), _U]),
    ("dcrt_tracer_get_sample_blocks", _I, [_P, C.POINTER(C.c_uint32), _U, C.POINTER(C.c_uint32)]),
    ("dcrt_tracer_update_sample_blocks", _I, [_P, C.c_float, _U, C.POINTER(C.c_uint32)]),
    ("dcrt_tracer_sample_blocks_device", _I, [_P, _U, _U, _P, _P, C.c_float, _U, _P, _P, C.POINTER(C.c_uint32)]),
    ("dcrt_tracer_adaptive_timings", _I, [_P, _FP, _FP, _FP]),
    ("dcrt_tracer_render_adaptive", _I, [_P, _U, C.POINTER(ConvergeParams), _U, C.POINTER(FilterParams), C.POINTER(NoiseStats),
                                         C.POINTER(C.c_int), C.POINTER(AdaptiveReport)]),
    ("dcrt_tracer_set_environment_sampling", _I, [_P, _I]),
    ("dcrt_tracer_get_environment_sampling", _I, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("dcrt_tracer_read_environment_distribution", _I, [_P, _FP, _FP, _FP]),
    ("dcrt_tracer_environment_build_timing", _I, [_P, _FP]),
    ("dcrt_tracer_set_light_sampling", _I, [_P, _I]),
    ("dcrt_tracer_get_light_sampling", _I, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("dcrt_tracer_read_light_distribution", _I, [_P, C.POINTER(LightTableInfo), _FP, _FP, C.POINTER(C.c_uint32), _FP, _FP]),
    ("dcrt_tracer_light_table_build_timing", _I, [_P, _FP]),
    ("dcrt_roulette_default_params", _I, [C.POINTER(RouletteParams)]),
    ("dcrt_tracer_set_roulette", _I, [_P, C.POINTER(RouletteParams)]),
    ("dcrt_tracer_get_roulette", _I, [_P, C.POINTER(RouletteParams)]),
    ("dcrt_device_roulette", _I, [_P, C.POINTER(RouletteParams), _FP, _FP, _U, _FP, C.POINTER(C.c_uint32), _FP]),
    ("dcrt_write_bmp", _I, [C.c_char_p, _U, _U, C.POINTER(C.c_uint8)]),
    ("dcrt_device_math_eval", _I, [_P, _I, _FP, _U, _FP]),
    ("dcrt_device_bsdf_eval", _I, [_P, C.POINTER(BsdfProbeMaterial), _U, _FP, _FP, _U, _FP, _FP]),
    ("dcrt_device_frame_probe", _I, [_P, C.POINTER(C.c_uint32), _U, _I, _FP]),
    ("dcrt_device_camera_ray", _I, [_P, _FP, _FP, _U, _FP, _FP]),
    ("dcrt_device_intersection_probe", _I, [_P, C.POINTER(C.c_uint32), _U, _I, _FP, C.POINTER(C.c_uint32)]),
    ("dcrt_device_light_sample", _I, [_P, _FP, C.POINTER(C.c_uint32), _U, _FP, C.POINTER(C.c_uint32)]),
    ("dcrt_device_light_eval", _I, [_P, C.POINTER(C.c_uint32), _FP, _U, _FP]),
    ("dcrt_device_env_lookup", _I, [_P, _FP, _U, _FP]),
    ("dcrt_flat_scene_triangle_instances", _I, [C.POINTER(FlatScene), C.POINTER(C.c_uint32), _U, C.POINTER(C.c_int)]),
    ("dcrt_device_bsdf_sample", _I, [_P, C.POINTER(BsdfProbeMaterial), _U, _FP, _FP, _U, _FP, _FP, _FP, C.POINTER(C.c_uint32)]),
]

_lib = None


class DCRTError(RuntimeError):
    pass


def load_library(path: os.PathLike | str | None = None):
    """Load libdcrt.so (built in-tree by __graft_entry__.build()). Raises if absent."""
    global _lib
    if _lib is not None:
        return _lib
    p = Path(path) if path else Path(os.environ.get("DCRT_LIB", LIB_PATH))
    if not p.exists():
        raise DCRTError(f"native library {p} is missing: run __graft_entry__.build() (no CPU fallback exists)")
    lib = C.CDLL(str(p))
    for name, res, args in SIGNATURES:
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.dcrt_abi_version() != ABI_VERSION:
        raise DCRTError(f"{p}: ABI version {lib.dcrt_abi_version()}, this binding expects {ABI_VERSION}")
    _lib = lib
    return lib


def check(rc: int, what: str = "") -> None:
    if rc != DCRT_OK:
        lib = load_library()
        msg = lib.dcrt_last_error().decode(errors="replace")
        raise DCRTError(f"{what or 'dcrt call'} failed: {ERRORS.get(rc, rc)}: {msg}")


def f3(v) -> C.Array:
    return (C.c_float * 3)(*[float(x) for x in v])
