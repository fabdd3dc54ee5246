"""ctypes binding of libvolpath_hip.so (include/volpath.h).

This is the host-side mirror of the reference's kernel-TU interface (src/volumeRender.cpp:117-128,
:347-356): the same entry points under the same names, called the way the reference host calls
them.  Everything here runs on the GPU through the C ABI; there is no CPU fallback -- if the
library or a gfx950 device is missing the calls raise.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VOLPATH_LIB", os.path.join(os.path.dirname(_HERE), "libvolpath_hip.so"))  # override: A/B builds

EST_GLOBAL, EST_DECOMP, EST_BOUNDED = 0, 1, 2
RNG_SAMPLERH, RNG_PHILOX, RNG_PHILOX7 = 0, 1, 2
ENV_PASSIVE, ENV_MIS = 0, 1
TRACK_SPECTRAL, TRACK_SCALAR, TRACK_MULTI_CHANNEL = 0, 1, 2
ARITH_EXACT, ARITH_FAST = 0, 1
VOL_U8, VOL_F32, VOL_F16 = 0, 1, 2   # VP_VOL_*: the formats of vp_init_volume
# include/volpath.h VP_ARITH_FAST_REL_L2: the stated bound on ||I_fast - I_exact||_2 / ||I_exact||_2 (mean images of 1024 frames)
ARITH_FAST_REL_L2 = 2e-3
# include/volpath.h VP_SUBPIXEL_MAX: the largest sub-pixel factor (set_subpixel takes 1, 2, 4, 8)
SUBPIXEL_MAX = 8

# every symbol include/volpath.h declares (tests check the library exports each one)
PART1_SYMBOLS = ["init_cuda", "set_texture_filter_mode", "free_cuda_buffers", "precompute_opacity", "init_envmap",
                 "free_envmap", "set_sun", "copy_inv_view_matrix", "copy_inv_model_matrix", "init_rng", "free_rng",
                 "render_kernel", "scale", "gamma_correct"]
PART2_SYMBOLS = ["vp_last_error", "vp_version", "vp_device_count", "vp_set_device", "vp_set_stream", "vp_get_stream", "vp_synchronize",
                 "vp_set_estimator", "vp_set_rng", "vp_set_envmap_sampling", "vp_get_env_tables", "vp_set_lookahead", "vp_set_tracking", "vp_set_bound_brick", "vp_set_shard", "vp_render_frames", "vp_init_volume", "vp_get_volume_info",
                 "vp_enable_counters", "vp_read_counters", "vp_render_time_ms", "vp_get_bound_table", "vp_get_opacity", "vp_get_pixel_table", "vp_get_null_collision_table", "vp_get_sun_clip_table", "vp_get_exit_table", "vp_set_exit_flights", "vp_render_class_time_ms", "vp_last_approach_mode", "vp_last_approach_table", "vp_last_light_const", "vp_last_lds_form", "vp_set_arithmetic", "vp_last_arithmetic", "vp_set_subpixel", "vp_get_subpixel", "vp_subpixel_offset", "vp_set_pipeline", "vp_last_pipelined", "vp_lookahead_stats", "vp_prepare", "vp_reserve_frames", "vp_get_pixel_lists", "vp_get_segment_table", "vp_get_ray_table", "vp_last_ray_table",
                 "vp_render_frames_stats", "vp_render_adaptive", "vp_scale_by_count", "vp_stats_rel_error",
                 "vp_denoise", "vp_set_denoise_form", "vp_last_denoise_form",
                 "vp_render_frames_layers", "vp_composite",
                 "vp_render_frames_groups", "vp_relight", "vp_reserve_frames_groups", "vp_groups_frames_per_launch", "vp_test_groups_census",
                 "vp_render_frames_groups_stats", "vp_render_frames_layers_stats",
                 "vp_render_adaptive_groups", "vp_render_adaptive_layers",
                 "vp_render_frames_group_layers", "vp_render_frames_group_layers_stats", "vp_relight_composite", "vp_test_group_layers_census",
                 "vp_render_adaptive_group_layers",
                 "vp_render_features",
                 "vp_denoise_guided",
                 "vp_render_frames_halves_stats", "vp_merge_halves", "vp_accumulate_stats",
                 "vp_halves_variance", "vp_filter_variance", "vp_denoise_var",
                 "vp_cross_error", "vp_select",
                 "vp_render_frames_planes_halves_stats",
                 "vp_render_adaptive_halves", "vp_render_adaptive_planes_halves",
                 "vp_julia_voxelize", "vp_cloud_voxelize", "vp_test_math", "vp_test_rng", "vp_test_sample_density", "vp_test_hg", "vp_test_roots", "vp_test_log_forms", "vp_test_approach_walk", "vp_test_sun_start", "vp_test_fetch_split", "vp_test_fetch_fold_axis", "vp_test_fetch_form", "vp_test_launch_census", "vp_test_intersect_box", "vp_test_camera_ray",
                 "vp_test_eval_envmap", "vp_ctx_create", "vp_ctx_destroy", "vp_ctx_set_current", "vp_ctx_get_current", "vp_ctx_device",
                 "vp_accumulate", "vp_tile_owner", "vp_malloc", "vp_free", "vp_memset",
                 "vp_upload", "vp_download"]


class Float3(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]


class Dim3(C.Structure):
    _fields_ = [("x", C.c_uint32), ("y", C.c_uint32), ("z", C.c_uint32)]


class VolumeInfo(C.Structure):
    """vp_volume_info"""
    _fields_ = [("format", C.c_int), ("nx", C.c_int), ("ny", C.c_int), ("nz", C.c_int), ("cell_bytes", C.c_int),
                ("cells_bytes", C.c_uint64)]


class Extent(C.Structure):
    _fields_ = [("width", C.c_size_t), ("height", C.c_size_t), ("depth", C.c_size_t)]


class Param(C.Structure):
    """src/param.h:4-12"""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("density", C.c_float), ("brightness", C.c_float),
                ("albedo", Float3), ("g", C.c_float), ("sigma_t", Float3)]


class Counters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("samples", "density_lookups", "density_loads", "bound_lookups",
                                          "opacity_lookups", "env_lookups", "scatters", "rng_draws")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class PixelStats(C.Structure):
    """include/volpath.h vp_pixel_stats: 24 bytes per pixel, indexed like the accumulator"""
    _fields_ = [("sum_y", C.c_double), ("sum_y2", C.c_double), ("n", C.c_uint32), ("flags", C.c_uint32)]


# the same record as a numpy dtype (StatsBuffer.download)
PIXEL_STATS_DTYPE = np.dtype([("sum_y", np.float64), ("sum_y2", np.float64), ("n", np.uint32), ("flags", np.uint32)])
STATS_FROZEN = 1


class Adaptive(C.Structure):
    """include/volpath.h vp_adaptive"""
    _fields_ = [("rel_tol", C.c_float), ("floor_y", C.c_float), ("min_frames", C.c_int), ("round_frames", C.c_int)]


class AdaptivePlanes(C.Structure):
    """include/volpath.h vp_adaptive_planes: [0] the first plane's (sun / fg), [1] the second's (sky / trans)"""
    _fields_ = [("rel_tol", C.c_float * 2), ("floor_y", C.c_float * 2), ("min_frames", C.c_int), ("round_frames", C.c_int)]


class AdaptivePlanes3(C.Structure):
    """include/volpath.h vp_adaptive_planes3: [0] sun, [1] sky, [2] trans"""
    _fields_ = [("rel_tol", C.c_float * 3), ("floor_y", C.c_float * 3), ("min_frames", C.c_int), ("round_frames", C.c_int)]


class AdaptiveResult(C.Structure):
    """include/volpath.h vp_adaptive_result"""
    _fields_ = [("samples", C.c_uint64), ("rounds", C.c_uint32), ("active_left", C.c_uint32), ("frames_used", C.c_uint32)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class DenoiseParams(C.Structure):
    """include/volpath.h vp_denoise_params"""
    _fields_ = [("radius", C.c_int), ("patch", C.c_int), ("k", C.c_float)]


DENOISE_MAX_RADIUS, DENOISE_MAX_PATCH = 10, 3


class DenoiseFeature(C.Structure):
    """include/volpath.h vp_denoise_feature: channel `channel` (0..3 = x, y, z, w) of a float4 plane and its sigma"""
    _fields_ = [("plane", C.c_void_p), ("channel", C.c_int), ("sigma", C.c_float)]


DENOISE_MAX_FEATURES = 4


class SelectParams(C.Structure):
    """include/volpath.h vp_select_params"""
    _fields_ = [("smooth_radius", C.c_int), ("blend_radius", C.c_int)]


SELECT_MAX_CANDIDATES, SELECT_MAX_RADIUS = 4, 3


# include/volpath.h VP_PLANES_*: the modes of vp_render_frames_planes_halves_stats, and each mode's planes in order
PLANES_LAYERS, PLANES_GROUPS, PLANES_GROUP_LAYERS = 1, 2, 3
PLANE_NAMES = {PLANES_LAYERS: ("fg", "trans"), PLANES_GROUPS: ("sun", "sky"), PLANES_GROUP_LAYERS: ("sun", "sky", "trans")}


class PlaneBufs(C.Structure):
    """include/volpath.h vp_plane_bufs: the accumulators and record buffers of one half's planes, in the mode's order"""
    _fields_ = [("acc", C.c_void_p * 3), ("rec", C.c_void_p * 3)]


class FeatureParams(C.Structure):
    """include/volpath.h vp_feature_params"""
    _fields_ = [("step", C.c_float), ("tau_z", C.c_float)]


# include/volpath.h VP_FEATURE_TAU_Z_DEFAULT (ln 2 as a float32 literal), VP_FEATURE_MAX_STEPS
FEATURE_TAU_Z_DEFAULT = float(np.float32(0.6931472))
FEATURE_MAX_STEPS = 1 << 20


class VolpathError(RuntimeError):
    pass


_lib = None


def lib():
    """Load the shared library (no GPU is touched until the first call that needs one)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise VolpathError(f"{LIB_PATH} is missing: run `make -C cuda-volpath_amd` (or __graft_entry__.build())")
        L = C.CDLL(LIB_PATH)
        L.vp_last_error.restype = C.c_char_p
        L.vp_version.restype = C.c_char_p
        L.vp_malloc.restype = C.c_void_p
        L.vp_malloc.argtypes = [C.c_size_t]
        L.vp_free.argtypes = [C.c_void_p]
        L.vp_memset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
        L.vp_upload.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.vp_download.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.vp_set_stream.argtypes = [C.c_void_p]
        L.vp_get_stream.restype = C.c_void_p
        L.vp_set_rng.argtypes = [C.c_int, C.c_uint32, C.c_uint32]
        L.vp_get_env_tables.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]
        L.vp_render_frames.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(Param)]
        L.vp_render_frames_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(Param)]
        L.vp_render_adaptive.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(Param), C.POINTER(Adaptive), C.POINTER(AdaptiveResult)]
        L.vp_scale_by_count.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float]
        L.vp_stats_rel_error.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_float]
        L.vp_denoise.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_int, C.POINTER(DenoiseParams)]
        L.vp_set_denoise_form.argtypes = [C.c_int]
        L.vp_denoise_guided.argtypes = [C.c_void_p] * 5 + [C.POINTER(DenoiseFeature), C.c_int, C.c_int, C.c_int, C.POINTER(DenoiseParams)]
        L.vp_render_frames_halves_stats.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_int, C.POINTER(Param)]
        L.vp_merge_halves.argtypes = [C.c_void_p] * 6 + [C.c_int, C.c_float]
        L.vp_accumulate_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.vp_halves_variance.argtypes = [C.c_void_p] * 4 + [C.c_int]
        L.vp_filter_variance.argtypes = [C.c_void_p] * 3 + [C.c_int, C.c_int, C.POINTER(DenoiseParams)]
        L.vp_denoise_var.argtypes = [C.c_void_p] * 6 + [C.POINTER(DenoiseFeature), C.c_int, C.c_int, C.c_int, C.POINTER(DenoiseParams)]
        L.vp_cross_error.argtypes = [C.c_void_p] * 7 + [C.c_int]
        L.vp_render_frames_planes_halves_stats.argtypes = [C.c_int, C.POINTER(PlaneBufs), C.POINTER(PlaneBufs), C.c_int, C.c_int, C.POINTER(Param)]
        L.vp_render_adaptive_halves.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_int, C.POINTER(Param), C.POINTER(Adaptive), C.POINTER(AdaptiveResult)]
        L.vp_render_adaptive_planes_halves.argtypes = [C.c_int, C.POINTER(PlaneBufs), C.POINTER(PlaneBufs), C.c_int, C.c_int, C.POINTER(Param),
                                                       C.POINTER(AdaptivePlanes3), C.POINTER(AdaptiveResult)]
        L.vp_select.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.POINTER(SelectParams)]
        L.vp_render_frames_layers.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(Param)]
        L.vp_composite.argtypes = [C.c_void_p] * 4 + [C.POINTER(C.c_float), C.c_int, C.c_float]
        L.vp_render_frames_groups.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(Param)]
        L.vp_relight.argtypes = [C.c_void_p] * 3 + [C.POINTER(C.c_float)] * 2 + [C.c_int, C.c_float]
        L.vp_reserve_frames_groups.argtypes = [C.POINTER(Param), C.c_int]
        L.vp_groups_frames_per_launch.argtypes = [C.POINTER(Param), C.c_int]
        L.vp_test_groups_census.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        L.vp_render_frames_groups_stats.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_int, C.POINTER(Param)]
        L.vp_render_frames_layers_stats.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_int, C.POINTER(Param)]
        for f in (L.vp_render_adaptive_groups, L.vp_render_adaptive_layers):
            f.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_int, C.POINTER(Param), C.POINTER(AdaptivePlanes), C.POINTER(AdaptiveResult)]
        L.vp_render_frames_group_layers.argtypes = [C.c_void_p] * 3 + [C.c_int, C.c_int, C.POINTER(Param)]
        L.vp_render_frames_group_layers_stats.argtypes = [C.c_void_p] * 6 + [C.c_int, C.c_int, C.POINTER(Param)]
        L.vp_render_adaptive_group_layers.argtypes = [C.c_void_p] * 6 + [C.c_int, C.c_int, C.POINTER(Param), C.POINTER(AdaptivePlanes3), C.POINTER(AdaptiveResult)]
        L.vp_render_features.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Param), C.POINTER(FeatureParams)]
        L.vp_relight_composite.argtypes = [C.c_void_p] * 4 + [C.POINTER(C.c_float)] * 2 + [C.c_void_p, C.POINTER(C.c_float), C.c_int, C.c_float]
        L.vp_test_group_layers_census.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        L.vp_read_counters.argtypes = [C.POINTER(Counters), C.c_int]
        L.vp_render_time_ms.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_int]
        L.vp_get_bound_table.argtypes = [C.c_void_p, C.c_size_t] + [C.POINTER(C.c_int)] * 5
        L.vp_get_opacity.argtypes = [C.c_void_p, C.c_size_t]
        L.vp_get_pixel_table.argtypes = [C.POINTER(Param), C.c_void_p, C.c_size_t]
        L.vp_get_null_collision_table.argtypes = [C.POINTER(Param), C.c_void_p, C.c_size_t]
        L.vp_get_sun_clip_table.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_float)]
        L.vp_render_class_time_ms.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.c_int]
        L.vp_prepare.argtypes = [C.POINTER(Param)]
        L.vp_set_subpixel.argtypes = [C.c_int]
        L.vp_subpixel_offset.argtypes = [C.c_uint, C.c_uint, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.vp_get_pixel_lists.argtypes = [C.POINTER(Param), C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)]
        L.vp_get_segment_table.argtypes = [C.POINTER(Param), C.c_void_p, C.c_size_t, C.POINTER(C.c_int)]
        L.vp_get_ray_table.argtypes = [C.POINTER(Param), C.c_void_p, C.c_size_t]
        L.vp_test_camera_ray.argtypes = [C.c_uint, C.c_uint, C.c_void_p, C.c_void_p, C.c_int]
        L.vp_julia_voxelize.argtypes = [C.c_int, C.c_void_p]
        L.vp_cloud_voxelize.argtypes = [C.c_int, C.c_uint32, C.c_void_p]
        L.vp_test_math.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        L.vp_test_roots.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
        L.vp_test_log_forms.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
        L.vp_test_approach_walk.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        L.vp_test_sun_start.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.vp_test_fetch_split.argtypes = [C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.vp_test_fetch_fold_axis.argtypes = [C.c_float, C.c_int]
        L.vp_test_fetch_form.argtypes = [C.POINTER(C.c_int), C.c_void_p, C.c_void_p]
        L.vp_test_launch_census.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        L.vp_test_rng.argtypes = [C.c_int] + [C.c_uint32] * 5 + [C.c_int, C.c_void_p]
        L.vp_test_sample_density.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.vp_test_hg.argtypes = [C.c_void_p] * 7 + [C.c_int]
        L.vp_test_intersect_box.argtypes = [C.c_void_p] * 5 + [C.c_int]
        L.vp_test_eval_envmap.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.vp_ctx_create.restype = C.c_void_p
        L.vp_ctx_create.argtypes = [C.c_int]
        L.vp_ctx_destroy.argtypes = [C.c_void_p]
        L.vp_ctx_set_current.argtypes = [C.c_void_p]
        L.vp_ctx_get_current.restype = C.c_void_p
        L.vp_accumulate.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.vp_tile_owner.argtypes = [C.c_uint, C.c_uint, C.c_int]
        L.init_cuda.argtypes = [C.c_void_p, Extent, C.c_bool, C.POINTER(Float3), C.POINTER(Float3)]
        L.init_cuda.restype = None
        L.vp_init_volume.argtypes = [C.c_void_p, Extent, C.c_int, C.POINTER(Float3), C.POINTER(Float3)]
        L.vp_get_volume_info.argtypes = [C.POINTER(VolumeInfo)]
        L.set_texture_filter_mode.argtypes = [C.c_bool]
        L.precompute_opacity.argtypes = [C.POINTER(C.c_float)]
        L.init_envmap.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.set_sun.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.copy_inv_view_matrix.argtypes = [C.POINTER(C.c_float), C.c_size_t]
        L.copy_inv_model_matrix.argtypes = [C.POINTER(C.c_float), C.c_size_t]
        L.init_rng.argtypes = [Dim3, Dim3, C.c_int, C.c_int]
        L.render_kernel.argtypes = [Dim3, Dim3, C.c_void_p, C.c_int, C.POINTER(Param)]
        L.scale.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_float]
        L.gamma_correct.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float]
        for name in ("set_texture_filter_mode", "free_cuda_buffers", "precompute_opacity", "init_envmap",
                     "free_envmap", "set_sun", "copy_inv_view_matrix", "copy_inv_model_matrix", "init_rng",
                     "free_rng", "render_kernel", "scale", "gamma_correct"):
            getattr(L, name).restype = None
        _lib = L
    return _lib


def _chk(rc):
    if rc != 0:
        raise VolpathError(f"volpath error {rc}: {lib().vp_last_error().decode()}")


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def device_count():
    return lib().vp_device_count()


def make_param(width, height, density=800.0, g=0.877, brightness=1.0, albedo=(1, 1, 1), sigma_t=(1, 1, 1)):
    """host.cpp:1286-1292 defaults with preset #13 (host.cpp:1308)."""
    P = Param()
    P.width, P.height, P.density, P.brightness, P.g = width, height, density, brightness, g
    P.albedo = Float3(*albedo)
    P.sigma_t = Float3(*sigma_t)
    return P


def mat(P, X, Y, Z, R, G, B):
    """Mat(), host.cpp:44-57: sigma_s, sigma_a -> sigma_t normalised by its max, albedo = sigma_s/sigma_t."""
    f = np.float32
    st = [f(X) + f(R), f(Y) + f(G), f(Z) + f(B)]
    al = [f(X) / st[0], f(Y) / st[1], f(Z) / st[2]]
    m = max(st)
    st = [s / m for s in st]
    P.albedo = Float3(*[float(a) for a in al])
    P.sigma_t = Float3(*[float(s) for s in st])
    return P


# H4: the default camera of the reference (host.cpp:108-115 through lookAt/inverse/transpose, :617-623)
DEFAULT_CAMERA = (0.0, 0.207912, 0.978148, 3.922986, 0.0, 0.978148, -0.207912, -0.782739, -1.0, 0.0, 0.0, 0.03)


class DeviceBuffer:
    """A caller-owned float4 accumulator in HBM (CudaFrameBuffer, host.cpp:358-389)."""

    def __init__(self, width, height):
        self.width, self.height = width, height
        self.nbytes = width * height * 16
        self.ptr = lib().vp_malloc(self.nbytes)
        if not self.ptr:
            raise VolpathError(lib().vp_last_error().decode())
        self.reset()

    def reset(self):
        _chk(lib().vp_memset(self.ptr, 0, self.nbytes))

    def upload(self, arr):
        arr = np.ascontiguousarray(arr, np.float32)
        assert arr.nbytes == self.nbytes
        _chk(lib().vp_upload(self.ptr, _p(arr), self.nbytes))

    def download(self):
        out = np.empty((self.height, self.width, 4), np.float32)
        _chk(lib().vp_download(_p(out), self.ptr, self.nbytes))
        return out

    def free(self):
        if self.ptr:
            lib().vp_free(self.ptr)
            self.ptr = None


def set_device(i):
    _chk(lib().vp_set_device(i))


def set_stream(stream_ptr):
    _chk(lib().vp_set_stream(stream_ptr))


def synchronize():
    _chk(lib().vp_synchronize())


def init_volume(grid, box=None, brick=1, linear=True):
    """init_cuda + set_texture_filter_mode as host.cpp:1336-1344 calls them. grid[k][j][i]: uint8, float32, or float16 (a binary16
    volume, vp_init_volume(VP_VOL_F16): the bits of the float32 volume grid.astype(float32) from 16-byte cells); any other dtype is
    converted to float32."""
    L = lib()
    grid = np.ascontiguousarray(grid)
    quantized = grid.dtype == np.uint8
    if not quantized and grid.dtype != np.float16:
        grid = np.ascontiguousarray(grid, np.float32)
    nz, ny, nx = grid.shape
    _chk(L.vp_set_bound_brick(brick))
    ext = Extent(nx, ny, nz)
    if grid.dtype == np.float16:
        bmin, bmax = (None, None) if box is None else (C.byref(Float3(*box[0])), C.byref(Float3(*box[1])))
        _chk(L.vp_init_volume(_p(grid), ext, VOL_F16, bmin, bmax))
    elif box is None:
        L.init_cuda(_p(grid), ext, quantized, None, None)
    else:
        L.init_cuda(_p(grid), ext, quantized, C.byref(Float3(*box[0])), C.byref(Float3(*box[1])))
    L.set_texture_filter_mode(bool(linear))


def volume_info():
    """vp_get_volume_info: the current volume's format (VOL_*), extent, bytes per packed cell and bytes of all cells on the device"""
    v = VolumeInfo()
    _chk(lib().vp_get_volume_info(C.byref(v)))
    return {"format": v.format, "nx": v.nx, "ny": v.ny, "nz": v.nz, "cell_bytes": v.cell_bytes, "cells_bytes": v.cells_bytes}


def init_envmap(env):
    env = np.ascontiguousarray(env, np.float32)
    h, w = env.shape[:2]
    lib().init_envmap(_p(env), w, h)


def set_sun(direction, power):
    d = (C.c_float * 3)(*direction)
    p = (C.c_float * 3)(*power)
    lib().set_sun(d, p)


def set_camera(m=DEFAULT_CAMERA):
    a = (C.c_float * 12)(*m)
    lib().copy_inv_view_matrix(a, 48)


def precompute_opacity(direction):
    d = (C.c_float * 3)(*direction)
    lib().precompute_opacity(d)


def set_estimator(est):
    _chk(lib().vp_set_estimator(est))


def set_rng(mode, key=(0, 0)):
    _chk(lib().vp_set_rng(mode, key[0], key[1]))


def set_tracking(mode):
    """TRACK_SPECTRAL (shipped) / TRACK_SCALAR (SPECTRAL_TRACKING 0) / TRACK_MULTI_CHANNEL (MULTI_CHANNEL 1)"""
    _chk(lib().vp_set_tracking(mode))


LOOKAHEAD_DEFAULT = 256


def set_lookahead(max_frames=LOOKAHEAD_DEFAULT):
    """frames render_kernel may render ahead per launch (0/1: one launch per call; default 256)"""
    _chk(lib().vp_set_lookahead(max_frames))


def set_envmap_sampling(mode):
    """ENV_PASSIVE (the reference's shipped build) or ENV_MIS (its !PASSIVE_ENVMAP alternative)"""
    _chk(lib().vp_set_envmap_sampling(mode))


def env_tables(width, height):
    cdf_y = np.empty(height, np.float32)
    cdf_x = np.empty((height, width), np.float32)
    norm = C.c_float()
    _chk(lib().vp_get_env_tables(_p(cdf_y), _p(cdf_x), C.byref(norm)))
    return cdf_y, cdf_x, norm.value


def set_shard(rank, world):
    _chk(lib().vp_set_shard(rank, world))


def render_kernel(buf_ptr, spp, P):
    """The reference's per-frame call (host.cpp:631): one sample per pixel of frame `spp`."""
    g = Dim3((P.width + 7) // 8, (P.height + 7) // 8, 1)
    b = Dim3(8, 8, 1)
    lib().render_kernel(g, b, buf_ptr, spp, C.byref(P))


def render_frames(buf_ptr, first, n, P):
    _chk(lib().vp_render_frames(buf_ptr, first, n, C.byref(P)))


class StatsBuffer:
    """A caller-owned buffer of width * height PixelStats records in HBM, zeroed (include/volpath.h vp_pixel_stats)."""

    def __init__(self, width, height):
        self.width, self.height = width, height
        self.nbytes = width * height * C.sizeof(PixelStats)
        self.ptr = lib().vp_malloc(self.nbytes)
        if not self.ptr:
            raise VolpathError(lib().vp_last_error().decode())
        self.reset()

    def reset(self):
        _chk(lib().vp_memset(self.ptr, 0, self.nbytes))

    def upload(self, arr):
        arr = np.ascontiguousarray(arr, PIXEL_STATS_DTYPE)
        assert arr.nbytes == self.nbytes
        _chk(lib().vp_upload(self.ptr, _p(arr), self.nbytes))

    def download(self):
        """(height, width) structured array of PIXEL_STATS_DTYPE"""
        out = np.empty((self.height, self.width), PIXEL_STATS_DTYPE)
        _chk(lib().vp_download(_p(out), self.ptr, self.nbytes))
        return out

    def free(self):
        if self.ptr:
            lib().vp_free(self.ptr)
            self.ptr = None


def render_frames_stats(buf_ptr, stats_ptr, first, n, P):
    """render_frames that also adds every sample's luminance to its pixel's record (vp_render_frames_stats): the same accumulator bits"""
    _chk(lib().vp_render_frames_stats(buf_ptr, stats_ptr, first, n, C.byref(P)))


def render_adaptive(buf_ptr, stats_ptr, first, max_frames, P, rel_tol, floor_y=1e-3, min_frames=16, round_frames=32):
    """Rounds of round_frames frames on the pixels whose record is not frozen, until none is left or max_frames are used
    (vp_render_adaptive); returns {"samples", "rounds", "active_left", "frames_used"}"""
    a = Adaptive(rel_tol, floor_y, min_frames, round_frames)
    r = AdaptiveResult()
    _chk(lib().vp_render_adaptive(buf_ptr, stats_ptr, first, max_frames, C.byref(P), C.byref(a), C.byref(r)))
    return r.as_dict()


def render_frames_layers(fg_ptr, trans_ptr, first, n, P):
    """the frames of render_frames as two compositing layers (vp_render_frames_layers): foreground sums into fg_ptr, per-channel
    transmittance sums (w: the count of unscattered samples) into trans_ptr; pixel = fg + trans * background"""
    _chk(lib().vp_render_frames_layers(fg_ptr, trans_ptr, first, n, C.byref(P)))


def composite(dst_ptr, fg_ptr, trans_ptr, n, s, plate_ptr=None, plate_rgb=None):
    """dst.xyz = fg.xyz * s + (trans.xyz * s) * B, dst.w = 1 - trans.w * s (vp_composite); B is the plate's pixel, or the constant
    plate_rgb where plate_ptr is None"""
    rgb = (C.c_float * 3)(*[float(v) for v in plate_rgb]) if plate_rgb is not None else None
    _chk(lib().vp_composite(dst_ptr, fg_ptr, trans_ptr, plate_ptr, rgb, n, s))


def render_frames_groups(sun_ptr, sky_ptr, first, n, P):
    """the frames of render_frames as two light groups (vp_render_frames_groups): what the sun lights sums into sun_ptr, what the sky
    lights into sky_ptr; both carry the heat channel in w"""
    _chk(lib().vp_render_frames_groups(sun_ptr, sky_ptr, first, n, C.byref(P)))


def relight(dst_ptr, sun_ptr, sky_ptr, n, s, sun_gain=(1.0, 1.0, 1.0), sky_gain=(1.0, 1.0, 1.0)):
    """dst.c = (sun.c * s) * sun_gain[c] + (sky.c * s) * sky_gain[c], dst.w = sun.w * s (vp_relight); in place is allowed"""
    gs = (C.c_float * 3)(*[float(v) for v in sun_gain])
    gk = (C.c_float * 3)(*[float(v) for v in sky_gain])
    _chk(lib().vp_relight(dst_ptr, sun_ptr, sky_ptr, gs, gk, n, s))


def render_frames_groups_stats(sun_ptr, sky_ptr, sun_stats_ptr, sky_stats_ptr, first, n, P):
    """render_frames_groups that also adds every sample's luminance to its pixel's record of the sample's group
    (vp_render_frames_groups_stats): the same accumulator bits, one StatsBuffer per group"""
    _chk(lib().vp_render_frames_groups_stats(sun_ptr, sky_ptr, sun_stats_ptr, sky_stats_ptr, first, n, C.byref(P)))


def render_frames_layers_stats(fg_ptr, trans_ptr, fg_stats_ptr, trans_stats_ptr, first, n, P):
    """render_frames_layers likewise (vp_render_frames_layers_stats): the same accumulator bits, one StatsBuffer per layer"""
    _chk(lib().vp_render_frames_layers_stats(fg_ptr, trans_ptr, fg_stats_ptr, trans_stats_ptr, first, n, C.byref(P)))


def _render_adaptive_planes(fn, p0, p1, s0, s1, first, max_frames, P, rel_tol, floor_y, min_frames, round_frames):
    a = AdaptivePlanes((C.c_float * 2)(*[float(v) for v in rel_tol]), (C.c_float * 2)(*[float(v) for v in floor_y]), min_frames, round_frames)
    r = AdaptiveResult()
    _chk(fn(p0, p1, s0, s1, first, max_frames, C.byref(P), C.byref(a), C.byref(r)))
    return r.as_dict()


def render_adaptive_groups(sun_ptr, sky_ptr, sun_stats_ptr, sky_stats_ptr, first, max_frames, P, rel_tol, floor_y=(1e-3, 1e-3), min_frames=16, round_frames=32):
    """render_adaptive's rounds on the two light groups (vp_render_adaptive_groups): a pixel is sampled, in both groups, while neither
    of its records is frozen, and both are frozen once each meets its own (rel_tol[k], floor_y[k]); returns render_adaptive's dict"""
    return _render_adaptive_planes(lib().vp_render_adaptive_groups, sun_ptr, sky_ptr, sun_stats_ptr, sky_stats_ptr, first, max_frames, P, rel_tol, floor_y,
                                   min_frames, round_frames)


def render_adaptive_layers(fg_ptr, trans_ptr, fg_stats_ptr, trans_stats_ptr, first, max_frames, P, rel_tol, floor_y=(1e-3, 1e-2), min_frames=16, round_frames=32):
    """the same on the two compositing layers (vp_render_adaptive_layers): [0] the foreground, [1] the transmittance"""
    return _render_adaptive_planes(lib().vp_render_adaptive_layers, fg_ptr, trans_ptr, fg_stats_ptr, trans_stats_ptr, first, max_frames, P, rel_tol, floor_y,
                                   min_frames, round_frames)


def render_frames_group_layers(sun_ptr, sky_ptr, trans_ptr, first, n, P):
    """light groups and layers of the same paths in one render (vp_render_frames_group_layers): what the sun lights on scattered paths
    sums into sun_ptr, what the sky lights on them into sky_ptr, the unscattered paths' per-channel transmittance (w: their count) into
    trans_ptr; pixel = gain_sun * sun + gain_sky * sky + trans * background"""
    _chk(lib().vp_render_frames_group_layers(sun_ptr, sky_ptr, trans_ptr, first, n, C.byref(P)))


def render_frames_group_layers_stats(sun_ptr, sky_ptr, trans_ptr, sun_stats_ptr, sky_stats_ptr, trans_stats_ptr, first, n, P):
    """render_frames_group_layers with one StatsBuffer per plane (vp_render_frames_group_layers_stats): the same accumulator bits"""
    _chk(lib().vp_render_frames_group_layers_stats(sun_ptr, sky_ptr, trans_ptr, sun_stats_ptr, sky_stats_ptr, trans_stats_ptr, first, n, C.byref(P)))


def render_adaptive_group_layers(sun_ptr, sky_ptr, trans_ptr, sun_stats_ptr, sky_stats_ptr, trans_stats_ptr, first, max_frames, P, rel_tol,
                                 floor_y=(1e-3, 1e-3, 1e-2), min_frames=16, round_frames=32):
    """render_adaptive's rounds on the three planes of a group-layers render (vp_render_adaptive_group_layers): a pixel is sampled, in
    all three planes, while none of its records is frozen, and all three are frozen once each meets its own (rel_tol[k], floor_y[k]);
    [0] sun, [1] sky, [2] trans; returns render_adaptive's dict"""
    a = AdaptivePlanes3((C.c_float * 3)(*[float(v) for v in rel_tol]), (C.c_float * 3)(*[float(v) for v in floor_y]), min_frames, round_frames)
    r = AdaptiveResult()
    _chk(lib().vp_render_adaptive_group_layers(sun_ptr, sky_ptr, trans_ptr, sun_stats_ptr, sky_stats_ptr, trans_stats_ptr, first, max_frames, C.byref(P),
                                               C.byref(a), C.byref(r)))
    return r.as_dict()


def relight_composite(dst_ptr, sun_ptr, sky_ptr, trans_ptr, n, s, sun_gain=(1.0, 1.0, 1.0), sky_gain=(1.0, 1.0, 1.0), plate_ptr=None, plate_rgb=None):
    """relight, then composite, in one pass (vp_relight_composite): dst.c = ((sun.c * s) * sun_gain[c] + (sky.c * s) * sky_gain[c]) +
    (trans.c * s) * B.c, dst.w = 1 - trans.w * s; B is the plate's pixel, or the constant plate_rgb where plate_ptr is None"""
    gs = (C.c_float * 3)(*[float(v) for v in sun_gain])
    gk = (C.c_float * 3)(*[float(v) for v in sky_gain])
    rgb = (C.c_float * 3)(*[float(v) for v in plate_rgb]) if plate_rgb is not None else None
    _chk(lib().vp_relight_composite(dst_ptr, sun_ptr, sky_ptr, trans_ptr, gs, gk, plate_ptr, rgb, n, s))


def reserve_frames_groups(P, nframes):
    """reserve_frames for a coming render_frames_groups job: two staging planes per frame (vp_reserve_frames_groups)"""
    _chk(lib().vp_reserve_frames_groups(C.byref(P), int(nframes)))


def groups_frames_per_launch(P, planes=2):
    """the frames one staged launch holds for this image now: planes = 1 render_frames, 2 render_frames_groups (vp_groups_frames_per_launch)"""
    n = lib().vp_groups_frames_per_launch(C.byref(P), int(planes))
    if n < 0:
        _chk(n)
    return n


def scale_by_count(dst_ptr, src_ptr, stats_ptr, n, s):
    """dst[i] = src[i] * (s / n_i) per channel, 0 where n_i == 0 (vp_scale_by_count); in place is allowed"""
    _chk(lib().vp_scale_by_count(dst_ptr, src_ptr, stats_ptr, n, s))


def stats_rel_error(stats_ptr, width, height, floor_y=1e-3):
    """(height, width) float32 noise map: estimated standard error of the mean luminance over max(mean, floor_y) (vp_stats_rel_error)"""
    n = width * height
    d = lib().vp_malloc(n * 4)
    if not d:
        raise VolpathError(lib().vp_last_error().decode())
    try:
        _chk(lib().vp_stats_rel_error(d, stats_ptr, n, floor_y))
        out = np.empty((height, width), np.float32)
        _chk(lib().vp_download(_p(out), d, n * 4))
    finally:
        lib().vp_free(d)
    return out


def denoise(dst_ptr, src_ptr, stats_ptr, width, height, radius=5, patch=1, k=0.45, guide_ptr=None, guide_stats_ptr=None):
    """dst = the NL-means filtered MEAN image of the accumulator src and its records (vp_denoise): weights from the guide pair
    (default: src itself), colours from src; queued on the context's stream, never synchronises"""
    dp = DenoiseParams(radius, patch, k)
    _chk(lib().vp_denoise(dst_ptr, src_ptr, stats_ptr, guide_ptr, guide_stats_ptr, width, height, C.byref(dp)))


def denoise_guided(dst_ptr, src_ptr, stats_ptr, width, height, features=(), radius=5, patch=1, k=0.45, guide_ptr=None, guide_stats_ptr=None):
    """denoise() with the weight of an offset cut by noise-free features (vp_denoise_guided): features is a sequence of
    (plane_ptr, channel, sigma), at most DENOISE_MAX_FEATURES of them; none: denoise()'s bytes"""
    dp = DenoiseParams(radius, patch, k)
    feats = [(getattr(p, "value", p), c, s) for p, c, s in features]
    arr = (DenoiseFeature * len(feats))(*[DenoiseFeature(p, c, s) for p, c, s in feats]) if feats else None
    _chk(lib().vp_denoise_guided(dst_ptr, src_ptr, stats_ptr, guide_ptr, guide_stats_ptr, arr, len(feats), width, height, C.byref(dp)))


def half_of_frame(frame, subpixel=1):
    """the half frame `frame` belongs to under sub-pixel factor `subpixel` (vp_render_frames_halves_stats): (f >> 2 log2 S) & 1"""
    return (int(frame) >> (2 * (int(subpixel).bit_length() - 1))) & 1


def render_frames_halves_stats(h0_ptr, h1_ptr, h0_stats_ptr, h1_stats_ptr, first, n, P):
    """render_frames_stats with the frames split between two (accumulator, records) pairs by half_of_frame: each half ends with the
    bits of its own frames' one-frame calls (vp_render_frames_halves_stats)"""
    _chk(lib().vp_render_frames_halves_stats(h0_ptr, h1_ptr, h0_stats_ptr, h1_stats_ptr, first, n, C.byref(P)))


def merge_halves(dst_ptr, resid_ptr, a_ptr, a_stats_ptr, b_ptr, b_stats_ptr, n, floor_y=1e-3):
    """dst = the count-weighted mean of the MEAN images a and b; resid (may be None) = half their luminance disagreement over
    max(lum(dst), floor_y) (vp_merge_halves); dst may be a or b"""
    _chk(lib().vp_merge_halves(dst_ptr, resid_ptr, a_ptr, a_stats_ptr, b_ptr, b_stats_ptr, n, floor_y))


def accumulate_stats(dst_ptr, src_ptr, n_records):
    """dst += src for records: sums added in binary64, n added, flags or-ed (vp_accumulate_stats)"""
    _chk(lib().vp_accumulate_stats(dst_ptr, src_ptr, n_records))


def halves_variance(u_ptr, q_ptr, a_stats_ptr, b_stats_ptr, n):
    """u = the pooled per-sample luminance variance of two halves' records, q (may be None) = the variance of that estimate: a quarter
    of the halves' squared difference (vp_halves_variance)"""
    _chk(lib().vp_halves_variance(u_ptr, q_ptr, a_stats_ptr, b_stats_ptr, n))


def filter_variance(dst_ptr, u_ptr, q_ptr, width, height, radius=1, patch=3, k=0.45):
    """dst = the NL-means filtered scalar plane u, weights from u itself with q as the noise of its values; a pixel with u == 0 stays 0
    (vp_filter_variance); queued on the context's stream, never synchronises"""
    dp = DenoiseParams(radius, patch, k)
    _chk(lib().vp_filter_variance(dst_ptr, u_ptr, q_ptr, width, height, C.byref(dp)))


def denoise_var(dst_ptr, src_ptr, stats_ptr, width, height, sample_var_ptr, features=(), radius=5, patch=1, k=0.45, guide_ptr=None, guide_stats_ptr=None):
    """denoise_guided() with the guide's variance taken from the caller's per-sample variance plane, times the guide's 1 / n
    (vp_denoise_var); sample_var_ptr None: denoise_guided()'s bytes"""
    dp = DenoiseParams(radius, patch, k)
    feats = [(getattr(p, "value", p), c, s) for p, c, s in features]
    arr = (DenoiseFeature * len(feats))(*[DenoiseFeature(p, c, s) for p, c, s in feats]) if feats else None
    _chk(lib().vp_denoise_var(dst_ptr, src_ptr, stats_ptr, guide_ptr, guide_stats_ptr, sample_var_ptr, arr, len(feats), width, height, C.byref(dp)))


def denoise_cross(dst_ptr, resid_ptr, h0, h0_stats, h1, h1_stats, tmp_a_ptr, tmp_b_ptr, width, height, radius, patch, k, features=None, floor_y=1e-3,
                  variance=None, var_ptrs=None):
    """the cross-filter of two half-buffers (accumulators h0, h1 and their records): each half filtered with the weights of the other into
    the caller's temporaries, then merged into dst and, where resid_ptr is given, the residual map -- three calls queued on the
    context's stream, nothing allocated.  variance=(R, F, k): the variance stage first (halves_variance, filter_variance with these
    parameters) and both filters through denoise_var with the one filtered plane; var_ptrs are then the caller's three float planes
    (u, q, filtered), width * height floats each"""
    feats = tuple(features) if features else ()
    if variance is None:
        denoise_guided(tmp_a_ptr, h0, h0_stats, width, height, feats, radius, patch, k, guide_ptr=h1, guide_stats_ptr=h1_stats)
        denoise_guided(tmp_b_ptr, h1, h1_stats, width, height, feats, radius, patch, k, guide_ptr=h0, guide_stats_ptr=h0_stats)
    else:
        if var_ptrs is None or len(var_ptrs) != 3:
            raise ValueError("denoise_cross: variance=(R, F, k) needs var_ptrs=(u, q, filtered), three device planes of width * height floats")
        vr, vf, vk = variance
        u_ptr, q_ptr, uf_ptr = var_ptrs
        halves_variance(u_ptr, q_ptr, h0_stats, h1_stats, width * height)
        filter_variance(uf_ptr, u_ptr, q_ptr, width, height, vr, vf, vk)
        denoise_var(tmp_a_ptr, h0, h0_stats, width, height, uf_ptr, feats, radius, patch, k, guide_ptr=h1, guide_stats_ptr=h1_stats)
        denoise_var(tmp_b_ptr, h1, h1_stats, width, height, uf_ptr, feats, radius, patch, k, guide_ptr=h0, guide_stats_ptr=h0_stats)
    merge_halves(dst_ptr, resid_ptr, tmp_a_ptr, h0_stats, tmp_b_ptr, h1_stats, width * height, floor_y)


def plane_bufs(planes):
    """a PlaneBufs from a sequence of (acc_ptr, rec_ptr) per plane, at most three; the entries beyond it stay NULL"""
    planes = list(planes)
    if len(planes) > 3:
        raise ValueError("plane_bufs: %d planes, at most 3" % len(planes))
    b = PlaneBufs()
    for k, (a, r) in enumerate(planes):
        b.acc[k] = getattr(a, "value", a)
        b.rec[k] = getattr(r, "value", r)
    return b


def render_frames_planes_halves_stats(mode, h0, h1, first, n, P):
    """the mode's _stats plane call (PLANES_LAYERS, PLANES_GROUPS, PLANES_GROUP_LAYERS) with the frames split between two halves of
    every plane by half_of_frame; h0 / h1: sequences of (acc_ptr, rec_ptr) per plane in the mode's order (PLANE_NAMES), or PlaneBufs
    (vp_render_frames_planes_halves_stats)"""
    b0 = h0 if isinstance(h0, PlaneBufs) else plane_bufs(h0)
    b1 = h1 if isinstance(h1, PlaneBufs) else plane_bufs(h1)
    _chk(lib().vp_render_frames_planes_halves_stats(mode, C.byref(b0), C.byref(b1), first, n, C.byref(P)))


def render_adaptive_halves(h0_ptr, h1_ptr, h0_stats_ptr, h1_stats_ptr, first, max_frames, P, rel_tol, floor_y=1e-3, min_frames=16, round_frames=32):
    """render_adaptive's rounds into two half-buffers (vp_render_adaptive_halves): a pixel is sampled while neither of its two records is
    frozen, frame f into half half_of_frame(f) alone, and both records are frozen once each half holds two samples and the two records
    together hold min_frames and meet the criterion; returns render_adaptive's dict"""
    a = Adaptive(rel_tol, floor_y, min_frames, round_frames)
    r = AdaptiveResult()
    _chk(lib().vp_render_adaptive_halves(h0_ptr, h1_ptr, h0_stats_ptr, h1_stats_ptr, first, max_frames, C.byref(P), C.byref(a), C.byref(r)))
    return r.as_dict()


def render_adaptive_planes_halves(mode, h0, h1, first, max_frames, P, rel_tol, floor_y, min_frames=16, round_frames=32):
    """the same on the two halves of every plane of a plane call (vp_render_adaptive_planes_halves): mode, h0 and h1 as in
    render_frames_planes_halves_stats; rel_tol and floor_y one value per plane of the mode (PLANE_NAMES), each plane's two records
    pooled, the planes AND-ed; returns render_adaptive's dict"""
    b0 = h0 if isinstance(h0, PlaneBufs) else plane_bufs(h0)
    b1 = h1 if isinstance(h1, PlaneBufs) else plane_bufs(h1)
    tol, fl = [float(v) for v in rel_tol], [float(v) for v in floor_y]
    if len(tol) > 3 or len(fl) > 3:
        raise ValueError("render_adaptive_planes_halves: at most 3 tolerances and floors")
    a = AdaptivePlanes3((C.c_float * 3)(*tol), (C.c_float * 3)(*fl), min_frames, round_frames)
    r = AdaptiveResult()
    _chk(lib().vp_render_adaptive_planes_halves(mode, C.byref(b0), C.byref(b1), first, max_frames, C.byref(P), C.byref(a), C.byref(r)))
    return r.as_dict()


# the residual floor of a plane by its name: trans lies in [0, 1] and is constant over most pixels
PLANE_RESID_FLOOR = {"fg": 1e-3, "sun": 1e-3, "sky": 1e-3, "trans": 1e-2}


def denoise_cross_planes(mode, dsts, resids, h0, h1, tmp_a_ptr, tmp_b_ptr, width, height, radius, patch, k, features=None, variance=None, var_ptrs=None):
    """denoise_cross per plane of a planes-halves render: plane j of `mode` (PLANE_NAMES) from its two halves h0[j], h1[j] -- each an
    (acc_ptr, rec_ptr) pair -- into dsts[j] and, where resids is given and resids[j] is not None, its residual map with the plane's
    floor (PLANE_RESID_FLOOR: 1e-3, trans 1e-2).  The temporaries and var_ptrs are shared by the planes: everything is queued in order
    on the context's stream, nothing is allocated.  variance / var_ptrs as in denoise_cross"""
    names = PLANE_NAMES[mode]
    if not (len(dsts) == len(h0) == len(h1) == len(names)) or (resids is not None and len(resids) != len(names)):
        raise ValueError("denoise_cross_planes: mode %d has %d planes" % (mode, len(names)))
    for j, name in enumerate(names):
        denoise_cross(dsts[j], resids[j] if resids is not None else None, h0[j][0], h0[j][1], h1[j][0], h1[j][1], tmp_a_ptr, tmp_b_ptr, width, height,
                      radius, patch, k, features=features, floor_y=PLANE_RESID_FLOOR[name], variance=variance, var_ptrs=var_ptrs)


def render_features(P, step, tau_z=FEATURE_TAU_Z_DEFAULT, alpha_ptr=None, depth_ptr=None):
    """the feature pass (vp_render_features): the deterministic march along every camera ray with a fixed step.  alpha = per-channel
    opacity (w: optical depth per unit sigma_t), depth = (first matter, where the luminance optical depth reaches tau_z, last matter,
    cover), +inf where a depth does not exist.  With both device pointers: fills them (queued on the context's stream, only the pixels
    the context owns) and returns None; with neither: returns the two (height, width, 4) float32 arrays"""
    fp = FeatureParams(step, tau_z)
    if (alpha_ptr is None) != (depth_ptr is None):
        raise ValueError("render_features: give both device buffers or neither")
    if alpha_ptr is not None:
        _chk(lib().vp_render_features(alpha_ptr, depth_ptr, C.byref(P), C.byref(fp)))
        return None
    a, d = DeviceBuffer(P.width, P.height), DeviceBuffer(P.width, P.height)
    try:
        _chk(lib().vp_render_features(a.ptr, d.ptr, C.byref(P), C.byref(fp)))
        synchronize()
        return a.download(), d.download()
    finally:
        a.free()
        d.free()


def cross_error(err_ptr, fa_ptr, fb_ptr, h0, h0_stats, h1, h1_stats, n):
    """err = one candidate's per-pixel error estimate: the filtered halves' MEAN images fa, fb held against the unfiltered means of the
    other half, less their variance; unclamped (vp_cross_error); queued on the context's stream, never synchronises"""
    _chk(lib().vp_cross_error(err_ptr, fa_ptr, fb_ptr, h0, h0_stats, h1, h1_stats, n))


def select(dst_ptr, index_ptr, image_ptrs, error_ptrs, width, height, smooth=1, blend=1):
    """dst = per pixel the candidate image whose box-smoothed error plane is smallest, the picks blended over (2 blend + 1)^2 pixels;
    index_ptr (may be None) receives the pick as one byte per pixel (vp_select); dst may be one of the images"""
    imgs = [getattr(p, "value", p) for p in image_ptrs]
    errs = [getattr(p, "value", p) for p in error_ptrs]
    if len(imgs) != len(errs):
        raise ValueError("select: %d images and %d error planes" % (len(imgs), len(errs)))
    n = len(imgs)
    sp = SelectParams(smooth, blend)
    _chk(lib().vp_select(dst_ptr, index_ptr, (C.c_void_p * max(n, 1))(*imgs), (C.c_void_p * max(n, 1))(*errs), n, width, height, C.byref(sp)))


def denoise_select(dst_ptr, index_ptr, h0, h0_stats, h1, h1_stats, width, height, candidates=((5, 1, 0.45), (10, 3, 0.45)), smooth=1, blend=1,
                   variance=(1, 3, 0.45), var_ptrs=None, tmp=None, features=None, floor_y=1e-3):
    """the cross-filter at several windows with a per-pixel choice among them: the variance stage once; per candidate (R, F, k) both
    halves through denoise_var with the roles swapped, cross_error of the pair, merge_halves into that candidate's image; then one
    select() into dst (and index_ptr, may be None) -- all queued on the context's stream, nothing allocated, nothing synchronised.  The
    caller supplies every device buffer: var_ptrs=(u, q, filtered), three planes of width * height floats, and tmp=(tmp_a, tmp_b, images,
    errors): two float4 images for the filtered halves, and per candidate one float4 image and one float plane"""
    cands = [tuple(c) for c in candidates]
    if var_ptrs is None or len(var_ptrs) != 3:
        raise ValueError("denoise_select: needs var_ptrs=(u, q, filtered), three device planes of width * height floats")
    if tmp is None or len(tmp) != 4 or len(tmp[2]) != len(cands) or len(tmp[3]) != len(cands):
        raise ValueError("denoise_select: needs tmp=(tmp_a, tmp_b, images, errors) with one float4 image and one float plane per candidate (%d)" % len(cands))
    if not 1 <= len(cands) <= SELECT_MAX_CANDIDATES:
        raise ValueError("denoise_select: %d candidates outside 1..%d" % (len(cands), SELECT_MAX_CANDIDATES))
    tmp_a, tmp_b, images, errors = tmp
    feats = tuple(features) if features else ()
    vr, vf, vk = variance
    u_ptr, q_ptr, uf_ptr = var_ptrs
    n = width * height
    halves_variance(u_ptr, q_ptr, h0_stats, h1_stats, n)
    filter_variance(uf_ptr, u_ptr, q_ptr, width, height, vr, vf, vk)
    for (radius, patch, k), img, err in zip(cands, images, errors):
        denoise_var(tmp_a, h0, h0_stats, width, height, uf_ptr, feats, radius, patch, k, guide_ptr=h1, guide_stats_ptr=h1_stats)
        denoise_var(tmp_b, h1, h1_stats, width, height, uf_ptr, feats, radius, patch, k, guide_ptr=h0, guide_stats_ptr=h0_stats)
        cross_error(err, tmp_a, tmp_b, h0, h0_stats, h1, h1_stats, n)
        merge_halves(img, None, tmp_a, h0_stats, tmp_b, h1_stats, n, floor_y)
    select(dst_ptr, index_ptr, images, errors, width, height, smooth, blend)


def set_denoise_form(form):
    """test hook: 0 tiled through LDS (default), 1 one thread per pixel from global memory; the same bits"""
    _chk(lib().vp_set_denoise_form(form))


def last_denoise_form():
    return lib().vp_last_denoise_form()


def enable_counters(on=True):
    _chk(lib().vp_enable_counters(int(on)))


def read_counters(reset=True):
    c = Counters()
    _chk(lib().vp_read_counters(C.byref(c), int(reset)))
    return c.as_dict()


def render_time_ms(reset=True):
    t = C.c_double()
    n = C.c_int()
    _chk(lib().vp_render_time_ms(C.byref(t), C.byref(n), int(reset)))
    return t.value, n.value


def render_class_time_ms(reset=True):
    """({"general": ms, "light": ms, "misses_box": ms}, {class: pixels}): kernel time per pixel class since the last reset"""
    ms = (C.c_double * 3)()
    px = (C.c_uint32 * 3)()
    _chk(lib().vp_render_class_time_ms(ms, px, int(reset)))
    names = ("general", "light", "misses_box")
    return dict(zip(names, ms[:])), dict(zip(names, px[:]))


def last_approach_mode():
    """0 / 1 / 2: how the last render launch took its general pixels' camera rays to the medium (vp_last_approach_mode)"""
    return int(lib().vp_last_approach_mode())


def last_approach_table():
    """1 if that walk read the per-view table of restart segments (vp_last_approach_table)"""
    return int(lib().vp_last_approach_table())


def reserve_frames(P, nframes):
    """size the sample staging for a coming render_frames job of nframes now (vp_reserve_frames)"""
    _chk(lib().vp_reserve_frames(C.byref(P), int(nframes)))


def lookahead_stats():
    """(look-ahead batches launched, batches told to stop while still running) of the current context (vp_lookahead_stats)"""
    a, b = C.c_uint(0), C.c_uint(0)
    _chk(lib().vp_lookahead_stats(C.byref(a), C.byref(b)))
    return int(a.value), int(b.value)


def last_lds_form():
    """0 / 1 / 2: how the last launch of the decomposition estimator read its brick table (vp_last_lds_form)"""
    return int(lib().vp_last_lds_form())


def set_arithmetic(mode):
    """ARITH_EXACT (the default: bit for bit the oracle's) or ARITH_FAST (hardware transcendentals and reciprocals, within
    ARITH_FAST_REL_L2 of the exact image; counter-based streams, spectral tracking, passive environment only)"""
    _chk(lib().vp_set_arithmetic(mode))


def set_subpixel(s):
    """Anti-aliasing: sub-pixel factor 1 (off, the default), 2, 4 or 8 of the current context (vp_set_subpixel): the sample of pixel
    (x, y) in frame f is the S = 1 sample of pixel (S x + i, S y + j) of the S W x S H image, (i, j) = subpixel_offset(x, y, f, S)"""
    _chk(lib().vp_set_subpixel(int(s)))


def get_subpixel():
    return int(lib().vp_get_subpixel())


def subpixel_offset(x, y, frame, s):
    """(i, j): which of the S x S fine pixels of pixel (x, y) frame `frame` samples (vp_subpixel_offset; no device needed)"""
    i, j = C.c_int(0), C.c_int(0)
    _chk(lib().vp_subpixel_offset(int(x), int(y), int(frame), int(s), C.byref(i), C.byref(j)))
    return i.value, j.value


def last_arithmetic():
    """ARITH_EXACT / ARITH_FAST: the arithmetic of the last render launch of the current context (vp_last_arithmetic)"""
    return int(lib().vp_last_arithmetic())


def set_pipeline(on=True):
    """staged render_frames calls on two alternating render targets (default on; vp_set_pipeline)"""
    _chk(lib().vp_set_pipeline(int(on)))


def last_pipelined():
    """1 if the last render call of the current context ran on a pipeline target (vp_last_pipelined)"""
    return int(lib().vp_last_pipelined())


def last_light_const():
    """True if the last render call wrote its light pixel class as per-pixel constants (vp_last_light_const)"""
    return bool(lib().vp_last_light_const())


def prepare(P):
    """build the per-camera tables, pixel lists and sun table of the current state now (vp_prepare)"""
    _chk(lib().vp_prepare(C.byref(P)))


def pixel_lists(P):
    """(general, light, misses_box): uint32 arrays of y << 16 | x, the pixel lists of the current shard / camera (test hook)"""
    cnt = (C.c_uint32 * 3)()
    _chk(lib().vp_get_pixel_lists(C.byref(P), None, 0, cnt))
    n = sum(cnt[:])
    out = np.empty(max(n, 1), np.uint32)
    _chk(lib().vp_get_pixel_lists(C.byref(P), _p(out), n, cnt))
    a, b = cnt[0], cnt[0] + cnt[1]
    return out[:a], out[a:b], out[b:n]


def bound_table(quantized=True):
    bnx, bny, bnz, brick, radius = (C.c_int() for _ in range(5))
    _chk(lib().vp_get_bound_table(None, 0, bnx, bny, bnz, brick, radius))
    out = np.empty((bnz.value, bny.value, bnx.value, 2), np.uint8 if quantized else np.float32)
    _chk(lib().vp_get_bound_table(_p(out), out.nbytes, bnx, bny, bnz, brick, radius))
    return out, brick.value, radius.value


def sun_clip_table(shape):
    """(uint16[nz, ny, nx], step): per cell, the distance in units of `step` beyond which a ray from anywhere in the cell toward
    the sun meets empty cells only; 0xffff = unknown (counter-based streams; include/volpath.h vp_get_sun_clip_table)"""
    out = np.empty(shape, np.uint16)
    step = C.c_float()
    _chk(lib().vp_get_sun_clip_table(_p(out), out.size, C.byref(step)))
    return out, step.value


def set_exit_flights(mode):
    """0 off, 1 global-majorant estimator only (default), 2 also the decomposition estimator (include/volpath.h)"""
    _chk(lib().vp_set_exit_flights(mode))


def exit_table(shape):
    """uint8[3, nz, ny, nx]: the direction table of the exit flights (include/volpath.h vp_get_exit_table)"""
    out = np.empty((3,) + tuple(shape), np.uint8)
    _chk(lib().vp_get_exit_table(_p(out), out.size))
    return out


def pixel_table(P):
    """(H, W, 8) float32: crawl end xyz, packed counts (view as uint32), certified-empty distance, pixel class (0 general,
    1 the whole chord is certified empty: light kernel, 2 the camera ray misses the box), 2 unused"""
    out = np.empty((P.height, P.width, 8), np.float32)
    _chk(lib().vp_get_pixel_table(C.byref(P), _p(out), out.size))
    return out


def segment_table(P):
    """(records, origins, cap): float32 [n_general, cap, 4] and [n_general, cap, 4], the per-view segment table of the decomposition
    estimator's approach walk for the general pixels in the order of pixel_lists(P)[0]; records[..., 2] viewed as uint32 = the brick's
    maximum byte | stop << 8; what lies behind a chain's stop record was never written (include/volpath.h vp_get_segment_table).
    Raises VolpathError where the configuration has no table."""
    cap = C.c_int()
    _chk(lib().vp_get_segment_table(C.byref(P), None, 0, C.byref(cap)))
    n = len(pixel_lists(P)[0])
    out = np.empty((n, 2, cap.value, 4), np.float32)
    _chk(lib().vp_get_segment_table(C.byref(P), _p(out), out.size, C.byref(cap)))
    return out[:, 0], out[:, 1], cap.value


def ray_table(P):
    """float32 [n_general, 8]: the per-view ray table of the global-majorant integrator for the general pixels in the order of
    pixel_lists(P)[0] -- (rd.x, rd.y, rd.z, t_near, t_far, t_empty, 0, 0) (include/volpath.h vp_get_ray_table).
    Raises VolpathError where the configuration has no table."""
    n = len(pixel_lists(P)[0])
    out = np.empty((max(n, 1), 8), np.float32)
    _chk(lib().vp_get_ray_table(C.byref(P), _p(out), n * 8))
    return out[:n]


def last_ray_table():
    """1 if the last render launch of the general class read the ray table (vp_last_ray_table)"""
    return int(lib().vp_last_ray_table())


def null_collision_table(P, count):
    """float32[count]: throughput of an unscattered global-majorant path after n null collisions in empty space"""
    out = np.empty(count, np.float32)
    _chk(lib().vp_get_null_collision_table(C.byref(P), _p(out), out.size))
    return out


def opacity_table(shape):
    out = np.empty(shape, np.float32)
    _chk(lib().vp_get_opacity(_p(out), out.size))
    return out


def test_math(which, x):
    x = np.ascontiguousarray(x, np.float32)
    out = np.empty_like(x)
    _chk(lib().vp_test_math(which, _p(x), _p(out), x.size))
    return out


def test_roots(which, lo_bits, hi_bits):
    """(mismatches, first bad bit pattern or None) of the in-range root helper `which` (0 sqrt_inrange_, 1 rsqrt_unit_) against the
    general form, over every binary32 bit pattern in [lo_bits, hi_bits]; walked on the device"""
    m, f = C.c_uint64(0), C.c_uint32(0)
    _chk(lib().vp_test_roots(which, lo_bits, hi_bits, C.byref(m), C.byref(f)))
    return m.value, (None if m.value == 0 else f.value)


def test_log_forms(which, lo_bits, hi_bits):
    """(mismatches, first bad bit pattern or None) of the logarithm `which` (0 logf_, 1 logf_pos_) against the chain as it stood, over
    every binary32 bit pattern in [lo_bits, hi_bits]; walked on the device"""
    m, f = C.c_uint64(0), C.c_uint32(0)
    _chk(lib().vp_test_log_forms(which, lo_bits, hi_bits, C.byref(m), C.byref(f)))
    return m.value, (None if m.value == 0 else f.value)


def test_approach_walk(kind, params, script, words):
    """(new, ref): uint32 [n, 5] hand-overs (distance bits, steps, two state words, through) of the approach walk `kind` (0 approach_k's,
    1 the local walks' inner loop) as built and as it stood, on n scripted cases: params float32 [n, 4] = (distance, t_empty, t_end or
    t_far, 1 / majorant), script uint32 [n, 4] = (cap, first word, words, first pair index), words uint32 (include/volpath.h)"""
    params = np.ascontiguousarray(params, np.float32).reshape(-1, 4)
    script = np.ascontiguousarray(script, np.uint32).reshape(-1, 4)
    words = np.ascontiguousarray(words, np.uint32).ravel()
    n = params.shape[0]
    if script.shape[0] != n:
        raise ValueError("params and script describe different numbers of cases")
    new, ref = np.zeros((n, 5), np.uint32), np.zeros((n, 5), np.uint32)
    _chk(lib().vp_test_approach_walk(kind, n, _p(params), _p(script), _p(words), words.size, _p(new), _p(ref)))
    return new, ref


def test_sun_start(origins, sun_dir, box):
    """(new, ref): uint32 [n, 8] starts of the sun shadow ray from the n collision points `origins` (float32 [n, 3]) toward sun_dir
    (three floats, taken as they are) against the box (bmin xyz, bmax xyz), with the sun row and as it stood: bits of the direction,
    the length, tnear, tfar; hit; in `new` the branches the origin's wave of 64 took (include/volpath.h)"""
    origins = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
    sun_dir = np.ascontiguousarray(sun_dir, np.float32).ravel()
    box = np.ascontiguousarray(box, np.float32).ravel()
    if sun_dir.size != 3 or box.size != 6:
        raise ValueError("sun_dir has three components, box six (bmin, bmax)")
    n = origins.shape[0]
    new, ref = np.zeros((n, 8), np.uint32), np.zeros((n, 8), np.uint32)
    _chk(lib().vp_test_sun_start(n, _p(origins), _p(sun_dir), _p(box), _p(new), _p(ref)))
    return new, ref


def test_fetch_split(linv, n, s_bits):
    """(two_step, folded): uint32 [count, 5] splits of one axis of n texels with the box scale linv at the offsets s = p - bmin given
    as bit patterns: (index, weight bits) of the uchar split, (index, weight bits, low) of the float split (include/volpath.h)"""
    s_bits = np.ascontiguousarray(s_bits, np.uint32).ravel()
    two, fold = np.zeros((s_bits.size, 5), np.uint32), np.zeros((s_bits.size, 5), np.uint32)
    _chk(lib().vp_test_fetch_split(float(linv), int(n), s_bits.size, _p(s_bits), _p(two), _p(fold)))
    return two, fold


def fetch_fold_axis(linv, n):
    """whether an axis of n texels with the box scale linv takes the folded form (vp_test_fetch_fold_axis); no device"""
    return bool(lib().vp_test_fetch_fold_axis(float(np.float32(linv)), int(n)))


def fetch_form():
    """(fold, fscale[3], fmul[3]) of the current volume and filter mode (vp_test_fetch_form)"""
    f, sc, mu = C.c_int(0), np.zeros(3, np.float32), np.zeros(3, np.float32)
    _chk(lib().vp_test_fetch_form(C.byref(f), _p(sc), _p(mu)))
    return f.value, sc, mu


CENSUS_EXACT, CENSUS_FAST = 0, 1                         # vp_test_launch_census: unit ...
CENSUS_RENDER, CENSUS_LAYERS, CENSUS_APPROACH = 0, 1, 2    # ... and kind


def census_name(kind, index):
    """the name of table entry `index` (include/volpath.h vp_test_launch_census) as tests/golden/render_variants.txt spells it:
    render_k's template arguments as digits, EST RNG . QUANT COUNT LDSB ACH MIS . TRK LIGHT CANCEL HALF; approach_k<RNG> gR,
    approach_local_k<RNG, QUANT> lRQ, approach_local_tab_k<RNG> tR"""
    i = int(index)
    if kind == CENSUS_APPROACH:
        i, quant = divmod(i, 2)
        walk, rng = divmod(i, 3)
        return f"g{rng}" if walk == 0 else f"t{rng}" if walk == 2 else f"l{rng}{quant}"
    d = []
    for radix in (2, 2, 2, 3, 2, 2, 3, 2, 2, 3):     # HALF CANCEL LIGHT TRK MIS ACH LDSB COUNT QUANT RNG, the least significant first
        i, r = divmod(i, radix)
        d.append(r)
    half, cancel, light, trk, mis, ach, ldsb, count, quant, rng = d
    return f"{i}{rng}.{quant}{count}{ldsb}{ach}{mis}.{trk}{light}{cancel}{half}"


def launch_census(unit, kind, reset=False):
    """{name: launches since the last reset} for every kernel that translation unit `unit` (CENSUS_EXACT / CENSUS_FAST) compiles of
    `kind` (CENSUS_RENDER, CENSUS_LAYERS: render_k of a layers launch, CENSUS_APPROACH), names as census_name spells them; process-wide,
    needs no device (vp_test_launch_census)"""
    n = lib().vp_test_launch_census(unit, kind, None, None, 0, 0)
    if n < 0:
        _chk(n)
    launches, built = np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    _chk(lib().vp_test_launch_census(unit, kind, _p(launches), _p(built), n, int(reset)))
    return {census_name(kind, i): int(launches[i]) for i in np.flatnonzero(built)}


def groups_census(reset=False):
    """launch_census for the table a render_frames_groups launch goes through: {name: launches since the last reset} for every groups
    instance of render_k the exact unit compiles (vp_test_groups_census); needs no device"""
    n = lib().vp_test_groups_census(None, None, 0, 0)
    if n < 0:
        _chk(n)
    launches, built = np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    _chk(lib().vp_test_groups_census(_p(launches), _p(built), n, int(reset)))
    return {census_name(CENSUS_RENDER, i): int(launches[i]) for i in np.flatnonzero(built)}


def group_layers_census(reset=False):
    """the same for the table a render_frames_group_layers launch goes through (vp_test_group_layers_census); needs no device"""
    n = lib().vp_test_group_layers_census(None, None, 0, 0)
    if n < 0:
        _chk(n)
    launches, built = np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    _chk(lib().vp_test_group_layers_census(_p(launches), _p(built), n, int(reset)))
    return {census_name(CENSUS_RENDER, i): int(launches[i]) for i in np.flatnonzero(built)}


def test_rng(mode, x, y, frame, n, key=(0, 0)):
    out = np.empty(n, np.float32)
    _chk(lib().vp_test_rng(mode, x, y, frame, key[0], key[1], n, _p(out)))
    return out


def test_sample_density(pos):
    pos = np.ascontiguousarray(pos, np.float32)
    out = np.empty(pos.shape[0], np.float32)
    _chk(lib().vp_test_sample_density(_p(pos), _p(out), pos.shape[0]))
    return out


def test_hg(g, r0, r1, normal, cos_query):
    """(direction after HGPhaseFunction::sample through Frame(normal), HGPhaseFunction::evaluate(cos_query)) on the device"""
    f = lambda a: np.ascontiguousarray(a, np.float32)
    g, r0, r1, normal, cos_query = f(g), f(r0), f(r1), f(normal), f(cos_query)
    n = g.size
    d = np.empty((n, 3), np.float32)
    e = np.empty(n, np.float32)
    _chk(lib().vp_test_hg(_p(g), _p(r0), _p(r1), _p(normal), _p(cos_query), _p(d), _p(e), n))
    return d, e


def test_intersect_box(origin, direction):
    o = np.ascontiguousarray(origin, np.float32)
    d = np.ascontiguousarray(direction, np.float32)
    n = o.shape[0]
    hit = np.empty(n, np.int32)
    tn = np.empty(n, np.float32)
    tf = np.empty(n, np.float32)
    _chk(lib().vp_test_intersect_box(_p(o), _p(d), _p(hit), _p(tn), _p(tf), n))
    return hit.astype(bool), tn, tf


def test_camera_ray(width, height, pixels):
    """(rd float32[n, 3], t_near, t_far, hit): camera_ray() and intersect_box() of the pixels (y << 16 | x) of a width x height image, in
    the arithmetic unit of the current mode (include/volpath.h vp_test_camera_ray)"""
    px = np.ascontiguousarray(pixels, np.uint32)
    out = np.empty((px.shape[0], 6), np.float32)
    _chk(lib().vp_test_camera_ray(width, height, _p(px), _p(out), px.shape[0]))
    return out[:, :3].copy(), out[:, 3].copy(), out[:, 4].copy(), out[:, 5] != 0.0


def test_eval_envmap(direction):
    d = np.ascontiguousarray(direction, np.float32)
    out = np.empty_like(d)
    _chk(lib().vp_test_eval_envmap(_p(d), _p(out), d.shape[0]))
    return out


class Context:
    """One scene on one GPU (include/volpath.h "Contexts").  `with ctx:` makes it the calling thread's current context."""

    def __init__(self, device=0):
        self.h = lib().vp_ctx_create(device)
        if not self.h:
            raise VolpathError(lib().vp_last_error().decode())
        self._prev = []

    def __enter__(self):
        self._prev.append(lib().vp_ctx_get_current())
        _chk(lib().vp_ctx_set_current(self.h))
        return self

    def __exit__(self, *exc):
        _chk(lib().vp_ctx_set_current(self._prev.pop()))

    def destroy(self):
        if self.h:
            _chk(lib().vp_ctx_destroy(self.h))
            self.h = None


def accumulate(dst_ptr, src_ptr, n_float4):
    _chk(lib().vp_accumulate(dst_ptr, src_ptr, n_float4))


def tile_owner(tx, ty, world):
    return lib().vp_tile_owner(tx, ty, world)


def julia_volume(n):
    """FractalJuliaSet (kernel.cu:84-140) voxelised on the GPU -> uint8 [k][j][i]."""
    out = np.empty((n, n, n), np.uint8)
    _chk(lib().vp_julia_voxelize(n, _p(out)))
    return out


def cloud_volume(n, seed=1):
    """the flagged synthetic cloud (vp_cloud_voxelize) voxelised on the GPU -> float32 [k][j][i] in [0,1]"""
    out = np.empty((n, n, n), np.float32)
    _chk(lib().vp_cloud_voxelize(n, seed, _p(out)))
    return out


def scale(dst_ptr, src_ptr, n, s):
    lib().scale(dst_ptr, src_ptr, n, s)


def gamma_correct(dst_ptr, src_ptr, n, s, gamma):
    lib().gamma_correct(dst_ptr, src_ptr, n, s, gamma)
