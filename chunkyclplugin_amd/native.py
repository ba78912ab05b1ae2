"""ctypes binding of the C ABI declared in include/chunky_hip.h (libchunky_hip.so).

This is the only way Python reaches the device path; there is no fallback.  If the shared library
is missing it is built with hipcc (`build()`); if that is impossible, or no HIP device is present
when a context is created, the error propagates — nothing here routes to a CPU implementation.
"""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess
from typing import List, Optional

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG_DIR, "csrc")
LIB_PATH = os.environ.get("CHUNKY_HIP_LIB") or os.path.join(PKG_DIR, "libchunky_hip.so")  # override: tuning builds (tools/variants.sh)
HEADER = os.path.join(os.path.dirname(PKG_DIR), "include", "chunky_hip.h")
SOURCES = ["render_pool.hip", "render_pool_bvh.hip", "render_pool_biome.hip", "render_pool_biome_bvh.hip", "render_pool_fog.hip", "render_pool_fog_bvh.hip", "render_pool_glass.hip", "render_pool_glass_bvh.hip", "render_biome.hip", "aov_biome.hip", "render_fallback.hip", "aux_kernels.hip", "filter.hip", "aov.hip", "occlusion.hip", "lights.hip", "lights_groups.hip", "matte.hip", "denoise.hip", "adaptive.hip", "robust.hip",
           "capi_context.hip", "capi_group.hip", "capi_scene.hip", "capi_render.hip", "capi_aov.hip", "capi_occlusion.hip", "capi_lights.hip", "capi_matte.hip", "capi_adaptive.hip", "capi_denoise.hip", "capi_robust.hip", "capi_fog.hip", "capi_glass.hip",
           "capi_run.hip", "capi_filter.hip", "capi_selftest.hip", "capi_error.cpp", "capi_host.cpp", "canvas_host.cpp", "adaptive_host.cpp", "denoise_host.cpp", "matte_host.cpp", "lights_host.cpp", "robust_host.cpp", "fog_host.cpp", "glass_host.cpp",
           "scene_records.cpp", "widetree.cpp", "launch_plan.cpp"]
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize", "-fPIC", "-shared"]

MAX_TRACES = 10
HIT_DTYPE = np.dtype([("hit", "<i4"), ("material", "<i4"), ("distance", "<f4"), ("normal", "<f4", 3),
                      ("color", "<f4", 4), ("emittance", "<f4"), ("point", "<f4", 3)])

PALETTE_BLOCK, PALETTE_MATERIAL, PALETTE_AABB, PALETTE_QUAD, PALETTE_TRIG = range(5)
BVH_WORLD, BVH_ACTOR = 0, 1
OPT_DRAW_DEPTH, OPT_MAX_DEPTH, OPT_EMITTER_SCALE, OPT_KERNEL, OPT_SUN_SAMPLING, OPT_EMITTERS, OPT_BSDF, OPT_EMITTER_NEE, OPT_BVH_CULL_BEHIND, OPT_BIOME_TINT = range(10)
BIOME_MAX_CELLS = 1 << 26  # CHUNKY_BIOME_MAX_CELLS: the most cells chunky_scene_set_biome_tints takes
KERNEL_BIOME = 2  # word 5 of chunky_render_kernel_info and bit 1 of word 1 of chunky_render_aov_kernel_info: a biome-tint instantiation
KERNEL_FOG = 3  # word 5 of chunky_render_kernel_info: a ground-fog instantiation
KERNEL_GLASS = 4  # word 5 of chunky_render_kernel_info: a translucent-blocks instantiation
PEER_LOCAL, PEER_DIRECT, PEER_STAGED = 0, 1, 2
TRANSPORT_PEER_COPY, TRANSPORT_RCCL_SENDRECV, TRANSPORT_RCCL_REDUCE = 0, 1, 2
E_INVALID, E_NO_DEVICE, E_HIP, E_STATE, E_ABORTED = -1, -2, -3, -4, -5
AOV_ALBEDO, AOV_NORMAL = 0, 1  # chunky_render_aov_read
AOV_ALPHA, AOV_DEPTH, AOV_POSITION, AOV_EMITTANCE, AOV_BLOCK = 2, 3, 4, 5, 6  # chunky_render_aov_read_ex (with the two above)
AOV_WORDS = {AOV_ALBEDO: 3, AOV_NORMAL: 3, AOV_ALPHA: 1, AOV_DEPTH: 1, AOV_POSITION: 3, AOV_EMITTANCE: 1, AOV_BLOCK: 1}  # words per pixel
AOV_AO, AOV_SUN = 7, 8  # chunky_render_occlusion_read (a float per pixel each)
LIGHT_SKY, LIGHT_SUN, LIGHT_EMITTERS, LIGHT_ALL = range(4)  # chunky_render_light_read (3 floats per pixel each)
LIGHT_MAX_EMITTER_GROUPS = 8  # CHUNKY_LIGHT_MAX_EMITTER_GROUPS
KERNEL_LIGHT_GROUPS = 4  # bit 2 of word 1 of chunky_render_light_kernel_info: the kernel that carries the emitter groups ran
MATTE_SLOTS = 6  # CHUNKY_MATTE_*: slots per pixel, the ids of a miss and of the two entity BVHs, the id an empty rank reports
MATTE_SKY, MATTE_WORLD_ENTITY, MATTE_ACTOR_ENTITY, MATTE_EMPTY = -1, -2, -3, -2 ** 31
DENOISE_DEMODULATE = 1  # chunky_denoise_params.flags
DENOISE_KERNEL_SHIFT = 8  # ... bits 8-9: 0 the default kernels (the images as they are), 1 the packed words
DENOISE_KERNEL_GATHER, DENOISE_KERNEL_PACKED = 0, 1
PROJ_PREGENERATED, PROJ_PINHOLE = -1, 0  # chunky_render_set_camera: the reference's two projector types
PROJ_PARALLEL, PROJ_FISHEYE, PROJ_PANORAMIC, PROJ_PANORAMIC_SLOT, PROJ_STEREOGRAPHIC = 1, 2, 3, 4, 5  # CHUNKY_PROJ_* (projected cameras)
PROJ_ODS, PROJ_ODS_STACKED = 7, 8  # omnidirectional stereo: one eye, both eyes stacked (6 is unassigned)


class ChunkyHipError(RuntimeError):
    """Raised for any non-zero status (the JNI layer would throw RuntimeException the same way;
    the reference gets CLException from JOCL, RendererInstance.java:36)."""

    def __init__(self, code: int, message: str):
        super().__init__(f"chunky-hip error {code}: {message}")
        self.code = code


def _stale(lib_path: str) -> bool:
    """The library is missing, or older than a source or the header."""
    if not os.path.exists(lib_path):
        return True
    t = os.path.getmtime(lib_path)
    # the sources (files only: csrc/build/ holds objects and tools that are written after the link)
    deps = [p for p in (os.path.join(CSRC, f) for f in os.listdir(CSRC)) if os.path.isfile(p)] + [HEADER]
    return any(os.path.getmtime(d) > t for d in deps)


def _needs_build() -> bool:
    return not os.environ.get("CHUNKY_HIP_LIB") and _stale(LIB_PATH)


def build(force: bool = False, extra_flags=(), out: Optional[str] = None, objdir: Optional[str] = None) -> str:
    """Compile the HIP library for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    if force or _needs_build():
        # one hipcc per translation unit, side by side (objects under csrc/build/, git-ignored), then one link
        import fcntl
        from concurrent.futures import ThreadPoolExecutor
        objdir = objdir or os.path.join(CSRC, "build")
        os.makedirs(objdir, exist_ok=True)
        # several ranks of one job may arrive here at once (bench.py --gpus N on a box without the library): one builds,
        # the others wait for it and find the library there
        lock = open(os.path.join(objdir, ".lock"), "w")
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not force and not _needs_build():
            lock.close()
            return out or LIB_PATH
        flags = [f for f in HIPCC_FLAGS if f != "-shared"] + list(extra_flags)

        def compile_one(src):
            obj = os.path.join(objdir, os.path.splitext(src)[0] + ".o")
            cmd = ["hipcc", *flags, "-x", "hip", "-c", os.path.join(CSRC, src), "-o", obj]
            proc = subprocess.run(cmd, capture_output=True, text=True)
            if proc.returncode != 0:
                raise RuntimeError(f"hipcc failed on {src}:\n" + proc.stderr[-4000:])
            return obj

        with ThreadPoolExecutor(max_workers=min(len(SOURCES), os.cpu_count() or 4, 16)) as pool:  # (more compile jobs than that gain nothing)
            objs = list(pool.map(compile_one, SOURCES))
        proc = subprocess.run(["hipcc", "--offload-arch=gfx950", "-shared", "-fPIC", *objs, "-o", out or LIB_PATH], capture_output=True, text=True)
        lock.close()  # (also released when an exception unwinds past here: the file object goes away)
        if proc.returncode != 0:
            raise RuntimeError("hipcc link failed:\n" + proc.stderr[-4000:])
    return out or LIB_PATH


TUNING_LIB_PATH = os.path.join(PKG_DIR, "libchunky_hip_tuning.so")


def build_tuning(force: bool = False) -> str:
    """The same library compiled with -DCHUNKY_TUNING: the build that reads the tuning / test-rig environment variables
    (CHUNKY_WIDE_LEVELS, CHUNKY_WIDE_TOP_BITS, CHUNKY_DEBUG_WIDE_BITS, CHUNKY_BVH_LAYOUT, CHUNKY_GROUP_TRANSPORT,
    CHUNKY_GROUP_SELF_EXCHANGE, CHUNKY_GROUP_NO_PROBE, CHUNKY_GROUP_TIMEOUT_MS, CHUNKY_RCCL_TRY_SHARED, CHUNKY_ADDR32_MASK).  The shipping
    library reads none of them; tests and tools that need one run a child process with CHUNKY_HIP_LIB pointing here."""
    if force or _stale(TUNING_LIB_PATH):
        build(force=True, extra_flags=["-DCHUNKY_TUNING"], out=TUNING_LIB_PATH, objdir=os.path.join(CSRC, "build", "tuning"))
    return TUNING_LIB_PATH


def declared_symbols() -> List[str]:
    """Every function include/chunky_hip.h declares."""
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(chunky_[a-z_0-9]+)\s*\(", text)) - {"chunky_post_render_fn"})


_lib: Optional[C.CDLL] = None
POST_RENDER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p)


PROGRESS_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int32)
SAVE_EVENT_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32)
REGEN_FN = C.CFUNCTYPE(None, C.c_void_p)


class RunCallbacks(C.Structure):
    """chunky_run_callbacks (include/chunky_hip.h)."""
    _fields_ = [("struct_size", C.c_size_t), ("post_render", POST_RENDER_FN), ("progress", PROGRESS_FN), ("merged", PROGRESS_FN),
                ("save_event", SAVE_EVENT_FN), ("regenerate_camera", REGEN_FN), ("user", C.c_void_p),
                ("poll_gate", POST_RENDER_FN)]


class DenoiseParams(C.Structure):
    """chunky_denoise_params (include/chunky_hip.h)."""
    _fields_ = [("size", C.c_size_t), ("iterations", C.c_int32), ("sigma_color", C.c_float), ("sigma_normal", C.c_float),
                ("sigma_albedo", C.c_float), ("flags", C.c_uint32)]


class AdaptiveParams(C.Structure):
    """chunky_adaptive_params (include/chunky_hip.h)."""
    _fields_ = [("size", C.c_size_t), ("threshold", C.c_float), ("floor", C.c_float), ("min_spp", C.c_int32), ("check_interval", C.c_int32),
                ("flags", C.c_uint32), ("reserved", C.c_uint32)]


ADAPTIVE_MAX_CHECKS = 64


class AdaptiveSummary(C.Structure):
    """chunky_adaptive_summary (include/chunky_hip.h)."""
    _fields_ = [("rounds", C.c_int32), ("checks", C.c_int32), ("passes", C.c_int32), ("reserved", C.c_int32), ("samples", C.c_int64),
                ("active", C.c_int32 * ADAPTIVE_MAX_CHECKS)]


class AdaptiveState(C.Structure):
    """chunky_adaptive_state (include/chunky_hip.h): the header of a run's state; the arrays travel beside it."""
    _fields_ = [("size", C.c_size_t), ("width", C.c_int32), ("height", C.c_int32), ("passes", C.c_int32), ("last_check", C.c_int32),
                ("active", C.c_int32), ("reserved", C.c_int32), ("params", AdaptiveParams), ("summary", AdaptiveSummary)]


class Fog(C.Structure):
    """chunky_fog (include/chunky_hip.h)."""
    _fields_ = [("size", C.c_size_t), ("density", C.c_float), ("y_min", C.c_float), ("y_max", C.c_float), ("color", C.c_float * 3)]


class Translucency(C.Structure):
    """chunky_translucency (include/chunky_hip.h)."""
    _fields_ = [("size", C.c_size_t), ("opaque_alpha", C.c_float), ("max_crossings", C.c_int32)]


ROUND_DONE_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int32, C.c_int32)

ROBUST_MEAN, ROBUST_MEDIAN, ROBUST_GINI = 0, 1, 2  # chunky_robust_params.mode
ROBUST_BUCKETS = (3, 5, 7, 9, 11, 13, 15)  # the bucket counts chunky_render_robust_begin takes


class RobustParams(C.Structure):
    """chunky_robust_params (include/chunky_hip.h)."""
    _fields_ = [("size", C.c_int32), ("mode", C.c_int32), ("gain", C.c_float)]


class AdaptiveCallbacks(C.Structure):
    """chunky_adaptive_callbacks (include/chunky_hip.h)."""
    _fields_ = [("struct_size", C.c_size_t), ("post_render", POST_RENDER_FN), ("round_done", ROUND_DONE_FN), ("user", C.c_void_p)]


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            build()
        L = C.CDLL(LIB_PATH)
        L.chunky_last_error.restype = C.c_char_p
        L.chunky_version.restype = C.c_char_p
        vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
        sig = {
            "chunky_device_count": [],
            "chunky_device_name": [C.c_int, C.c_char_p, C.c_int],
            "chunky_init": [C.c_int, C.POINTER(vp)],
            "chunky_shutdown": [vp],
            "chunky_group_create": [vp, C.c_int, C.POINTER(vp)],
            "chunky_group_size": [vp],
            "chunky_group_device": [vp, C.c_int],
            "chunky_group_peer_status": [vp, vp, C.c_int],
            "chunky_group_transport": [vp, C.POINTER(C.c_int), C.c_char_p, C.c_int],
            "chunky_group_set_transport": [vp, C.c_int],
            "chunky_scene_create": [vp, C.POINTER(vp)],
            "chunky_scene_destroy": [vp],
            "chunky_scene_set_octree": [vp, vp, i64, C.c_int],
            "chunky_scene_load_octree": [vp, vp, i64, C.c_int, vp, i64],
            "chunky_scene_set_palette": [vp, C.c_int, vp, i64],
            "chunky_scene_set_bvh": [vp, C.c_int, vp, i64],
            "chunky_scene_set_atlas": [vp, vp, C.c_int, C.c_int, C.c_int],
            "chunky_scene_write_atlas_tile": [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp],
            "chunky_scene_set_sky": [vp, vp, C.c_int, C.c_int, f32],
            "chunky_scene_set_sun": [vp, vp],
            "chunky_scene_set_biome_tints": [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int],
            "chunky_scene_emitters": [vp, vp, i32, C.POINTER(i32)],
            "chunky_render_create": [vp, vp, C.c_int, C.c_int, C.POINTER(vp)],
            "chunky_render_destroy": [vp],
            "chunky_render_set_camera": [vp, C.c_int, vp, i64],
            "chunky_render_set_lens": [vp, f32, f32],
            "chunky_render_set_option": [vp, C.c_int, i32],
            "chunky_render_set_shard": [vp, C.c_int, C.c_int, C.c_int],
            "chunky_render_set_device_buffer": [vp, vp],
            "chunky_render_device_buffer": [vp, C.POINTER(vp)],
            "chunky_render_reset": [vp],
            "chunky_render_passes": [vp, vp, C.c_int, C.c_int],
            "chunky_render_sync": [vp],
            "chunky_render_read": [vp, vp, i64],
            "chunky_render_gather": [vp],
            "chunky_render_kernel_time": [vp, C.POINTER(f32), C.POINTER(C.c_int)],
            "chunky_render_preview": [vp, vp],
            "chunky_render_phase_stats": [vp, vp, C.c_int],
            "chunky_render_kernel_info": [vp, vp],
            "chunky_render_trace_records": [vp, i32, vp, C.c_int, vp, vp, vp],
            "chunky_render_aov_passes": [vp, vp, C.c_int, C.c_int],
            "chunky_render_aov_read": [vp, C.c_int, vp, i64],
            "chunky_render_aov_reset": [vp],
            "chunky_render_aov_kernel_time": [vp, C.POINTER(f32), C.POINTER(C.c_int)],
            "chunky_render_aov_kernel_info": [vp, vp],
            "chunky_render_aov_passes_ex": [vp, vp, C.c_int, C.c_int],
            "chunky_render_aov_read_ex": [vp, C.c_int, vp, i64],
            "chunky_render_occlusion_passes": [vp, vp, C.c_int, C.c_int, f32],
            "chunky_render_occlusion_read": [vp, C.c_int, vp, i64],
            "chunky_render_occlusion_reset": [vp],
            "chunky_render_occlusion_kernel_time": [vp, C.POINTER(f32), C.POINTER(C.c_int)],
            "chunky_render_occlusion_kernel_info": [vp, vp],
            "chunky_render_light_passes": [vp, vp, C.c_int, C.c_int],
            "chunky_render_light_read": [vp, C.c_int, vp, i64],
            "chunky_render_light_mix": [vp, vp, vp, i64],
            "chunky_render_light_reset": [vp],
            "chunky_render_light_set_emitter_groups": [vp, C.c_int, vp, vp, C.c_int],
            "chunky_render_light_read_group": [vp, C.c_int, vp, i64],
            "chunky_render_light_mix_groups": [vp, f32, f32, vp, C.c_int, vp, i64],
            "chunky_render_light_kernel_time": [vp, C.POINTER(f32), C.POINTER(C.c_int)],
            "chunky_render_light_kernel_info": [vp, vp],
            "chunky_render_matte_passes": [vp, vp, C.c_int],
            "chunky_render_matte_reset": [vp],
            "chunky_render_matte_read": [vp, vp, vp, vp, i64, C.POINTER(i32)],
            "chunky_render_matte_restore": [vp, vp, vp, vp, i64, i32],
            "chunky_render_matte_ranks": [vp, vp, vp, i64],
            "chunky_render_matte_extract": [vp, vp, C.c_int, vp, i64],
            "chunky_render_matte_kernel_time": [vp, C.POINTER(f32), C.POINTER(C.c_int)],
            "chunky_render_matte_kernel_info": [vp, vp],
            "chunky_matte_host_fold": [vp, C.c_int, i64, vp, vp, vp],
            "chunky_matte_host_ranks": [vp, vp, i64, i32, vp, vp],
            "chunky_matte_host_extract": [vp, vp, i64, i32, vp, C.c_int, vp],
            "chunky_matte_state_check": [vp, vp, vp, i64, i32],
            "chunky_denoise_default_params": [C.POINTER(DenoiseParams)],
            "chunky_denoise_host": [C.c_int, C.c_int, vp, vp, vp, C.POINTER(DenoiseParams), vp],
            "chunky_denoise_frame": [vp, C.c_int, C.c_int, vp, vp, vp, C.POINTER(DenoiseParams), vp],
            "chunky_render_denoise": [vp, C.POINTER(DenoiseParams), vp, i64],
            "chunky_render_denoise_kernel_time": [vp, C.POINTER(f32), C.POINTER(C.c_int)],
            "chunky_denoise_exp": [vp, C.c_int, vp],
            "chunky_adaptive_default_params": [C.POINTER(AdaptiveParams)],
            "chunky_adaptive_host": [C.c_int, C.c_int, vp, C.c_int, C.POINTER(AdaptiveParams), vp, vp, vp],
            "chunky_render_adaptive": [vp, vp, C.c_int, C.POINTER(AdaptiveParams), C.POINTER(AdaptiveSummary)],
            "chunky_render_adaptive_counts": [vp, vp, i64],
            "chunky_render_adaptive_noise": [vp, vp, i64],
            "chunky_render_adaptive_kernel_time": [vp, C.POINTER(f32), C.POINTER(C.c_int)],
            "chunky_selftest_render_list": [vp, vp, C.c_int, vp, C.c_int],
            "chunky_selftest_plan_biome": [vp, i64, vp, vp],
            "chunky_adaptive_host_begin": [C.c_int, C.c_int, C.POINTER(AdaptiveParams), C.POINTER(AdaptiveState), vp, vp, vp, vp],
            "chunky_adaptive_host_resume": [C.POINTER(AdaptiveState), vp, C.c_int, vp, vp, vp, vp],
            "chunky_adaptive_state_check": [C.POINTER(AdaptiveState), vp, vp],
            "chunky_render_adaptive_ex": [vp, vp, C.c_int, C.POINTER(AdaptiveParams), C.POINTER(AdaptiveCallbacks), C.POINTER(AdaptiveSummary)],
            "chunky_render_adaptive_resume": [vp, vp, C.c_int, C.POINTER(AdaptiveParams), C.POINTER(AdaptiveCallbacks), C.POINTER(AdaptiveSummary)],
            "chunky_render_adaptive_state": [vp, C.POINTER(AdaptiveState), vp, i64],
            "chunky_render_adaptive_restore": [vp, C.POINTER(AdaptiveState), vp, vp, vp, vp],
            "chunky_robust_default_params": [C.POINTER(RobustParams)],
            "chunky_robust_host": [C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp],
            "chunky_robust_host_resolve": [C.c_int, i64, vp, C.POINTER(RobustParams), vp, vp],
            "chunky_render_robust_begin": [vp, C.c_int],
            "chunky_render_robust_passes": [vp, vp, C.c_int, C.c_int],
            "chunky_render_robust_read_bucket": [vp, C.c_int, vp, i64, C.POINTER(i32)],
            "chunky_render_robust_resolve": [vp, C.POINTER(RobustParams), vp, i64, vp, i64],
            "chunky_render_robust_denoise": [vp, C.POINTER(RobustParams), C.POINTER(DenoiseParams), vp, i64],
            "chunky_render_robust_kernel_time": [vp, C.POINTER(f32), C.POINTER(C.c_int), C.POINTER(f32)],
            "chunky_selftest_robust": [vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.POINTER(RobustParams), vp, vp, vp],
            "chunky_render_run": [vp, vp, C.POINTER(i32), i32, i32, POST_RENDER_FN, vp],
            "chunky_render_run_ex": [vp, vp, C.POINTER(i32), i32, i32, C.POINTER(RunCallbacks)],
            "chunky_java_random_ints": [i64, vp, C.c_int],
            "chunky_selftest_math": [vp, C.c_int, C.c_int, vp, vp, vp],
            "chunky_selftest_helpers": [vp, C.c_int, C.c_int, C.c_int, vp, vp, C.POINTER(i32)],
            "chunky_selftest_gamma_scan": [vp, C.c_int, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(f32)],
            "chunky_selftest_camera_rays": [vp, i32, vp, i64],
            "chunky_selftest_shard_map": [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp],
            "chunky_camera_rays": [C.c_int, vp, i64, C.c_int, C.c_int, i32, vp],
            "chunky_camera_rays_lens": [C.c_int, vp, i64, C.c_int, C.c_int, i32, f32, f32, vp],
            "chunky_camera_rays_window": [C.c_int, vp, i64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, i32, f32, f32, vp],
            "chunky_render_set_canvas": [vp, C.c_int, C.c_int, C.c_int, C.c_int],
            "chunky_render_canvas": [vp, vp],
            "chunky_render_set_fog": [vp, C.POINTER(Fog)],
            "chunky_render_fog": [vp, C.POINTER(Fog)],
            "chunky_fog_check": [C.POINTER(Fog)],
            "chunky_selftest_plan_fog": [vp, i64, vp, vp],
            "chunky_render_set_translucency": [vp, C.POINTER(Translucency)],
            "chunky_render_translucency": [vp, C.POINTER(Translucency), C.POINTER(C.c_int)],
            "chunky_translucency_check": [C.POINTER(Translucency)],
            "chunky_selftest_plan_glass": [vp, i64, vp, vp],
            "chunky_canvas_check": [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int],
            "chunky_selftest_canvas_pixel": [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, i32, vp],
            "chunky_filter_frame": [vp, C.c_int, C.c_int, C.c_double, vp, vp, C.c_int],
            "chunky_filter_frame_alpha": [vp, C.c_int, C.c_int, C.c_double, vp, vp, vp, C.c_int],
            "chunky_filter_alpha_bytes": [vp, i64, vp],
            "chunky_filter_gamma_thresholds": [vp],
            "chunky_filter_frame_device": [vp, i64, f32, vp, vp, C.c_int, C.c_int, C.POINTER(f32)],
            "chunky_widetree_lookup": [vp, i64, C.c_int, vp, C.c_int, vp, C.c_int, vp, vp, C.POINTER(i64)],
            "chunky_addr32_word": [vp, vp, C.c_int, C.POINTER(C.c_uint32)],
            "chunky_scene_addr32": [vp, C.POINTER(C.c_uint32)],
            "chunky_widetree_hit_top": [vp, i64, C.c_int, vp, C.c_int, vp, i64, C.POINTER(i32)],
            "chunky_scene_hit_top": [vp, C.POINTER(i32)],
            "chunky_render_march_above": [vp, vp, C.c_int],
        }
        for name, args in sig.items():
            if not hasattr(L, name) and os.environ.get("CHUNKY_HIP_LIB") and os.environ.get("CHUNKY_HIP_LIB_EARLIER") == "1":
                continue  # only tools/adaptive_bench.py --resume-legs and tools/headline_ab.py set this, for the child that times an earlier commit's build: what that lacks stays unbound
            fn = getattr(L, name)
            fn.argtypes = args
            fn.restype = C.c_int
        _lib = L
    return _lib


def check(rc: int) -> None:
    if rc != 0:
        raise ChunkyHipError(rc, (lib().chunky_last_error() or b"").decode("utf-8", "replace"))


def ptr(a: np.ndarray) -> int:
    return a.ctypes.data


def java_random_ints(n: int, seed: int = 0) -> np.ndarray:
    out = np.zeros(n, np.int32)
    check(lib().chunky_java_random_ints(seed, ptr(out), n))
    return out


def camera_rays(projector_type: int, settings, width: int, height: int, seed: int, lens=None) -> np.ndarray:
    """chunky_camera_rays: the width*height*6-float table (projector type -1) of a projected camera for the pass of `seed`,
    computed on the host with the kernels' arithmetic (no device needed).  lens = (aperture, focus): chunky_camera_rays_lens,
    the table of the camera with that lens (chunky_render_set_lens)."""
    s = np.ascontiguousarray(settings, np.float32)
    out = np.zeros(int(width) * int(height) * 6, np.float32)
    seed32 = int(np.int32(np.uint32(seed & 0xFFFFFFFF)))
    if lens is None:
        check(lib().chunky_camera_rays(int(projector_type), ptr(s), s.size, int(width), int(height), seed32, ptr(out)))
    else:
        check(lib().chunky_camera_rays_lens(int(projector_type), ptr(s), s.size, int(width), int(height), seed32, float(lens[0]), float(lens[1]), ptr(out)))
    return out


def camera_rays_window(projector_type: int, settings, width: int, height: int, canvas_width: int, canvas_height: int, x0: int, y0: int,
                       seed: int, lens=None) -> np.ndarray:
    """chunky_camera_rays_window: the width*height*6-float table of the WINDOW at (x0, y0) of a canvas_width x canvas_height canvas
    (chunky_render_set_canvas) — the crop of camera_rays on the canvas, computed for the window's pixels alone.  Host only."""
    s = np.ascontiguousarray(settings, np.float32)
    out = np.zeros(max(int(width), 0) * max(int(height), 0) * 6, np.float32)
    seed32 = int(np.int32(np.uint32(seed & 0xFFFFFFFF)))
    a, f = (0.0, 0.0) if lens is None else (float(lens[0]), float(lens[1]))
    check(lib().chunky_camera_rays_window(int(projector_type), ptr(s), s.size, int(width), int(height), int(canvas_width), int(canvas_height),
                                          int(x0), int(y0), seed32, a, f, ptr(out)))
    return out


def canvas_check(width: int, height: int, canvas_width: int, canvas_height: int, x0: int, y0: int, projector_type: int = 0) -> int:
    """chunky_canvas_check: chunky_render_set_canvas' own test of a window, without a target or a device; the status code (0 = accepted)."""
    return int(lib().chunky_canvas_check(int(width), int(height), int(canvas_width), int(canvas_height), int(x0), int(y0), int(projector_type)))


def canvas_pixel(width: int, height: int, canvas_width: int, canvas_height: int, x0: int, y0: int, g: int):
    """chunky_selftest_canvas_pixel: (G, X, Y) of the window's local index g, by the helper the kernels use."""
    out = np.zeros(3, np.int32)
    check(lib().chunky_selftest_canvas_pixel(int(width), int(height), int(canvas_width), int(canvas_height), int(x0), int(y0), int(g), ptr(out)))
    return tuple(int(v) for v in out)


def filter_alpha_bytes(alpha) -> np.ndarray:
    """chunky_filter_alpha_bytes: the alpha byte chunky_filter_frame_alpha writes for each value, on the host (no device needed)."""
    a = np.ascontiguousarray(alpha, np.float32).reshape(-1)
    out = np.zeros(a.size, np.int32)
    check(lib().chunky_filter_alpha_bytes(ptr(a), a.size, ptr(out)))
    return out


def widetree_lookup(tree: np.ndarray, depth: int, xyz: np.ndarray, level_bits=None):
    """Host-side check of the upload-time octree re-layout: (data, level, n_entries) for each cell."""
    tree = np.ascontiguousarray(tree, np.int32)
    xyz = np.ascontiguousarray(xyz, np.int32).reshape(-1, 3)
    data = np.zeros(len(xyz), np.int32)
    level = np.zeros(len(xyz), np.int32)
    n_entries = C.c_int64()
    lb = None if level_bits is None else np.ascontiguousarray(level_bits, np.int32)
    check(lib().chunky_widetree_lookup(ptr(tree), tree.size, depth, None if lb is None else ptr(lb),
                                       0 if lb is None else lb.size, ptr(xyz), len(xyz), ptr(data), ptr(level),
                                       C.byref(n_entries)))
    return data, level, n_entries.value


def widetree_hit_top(tree: np.ndarray, depth: int, blocks: np.ndarray, level_bits=None) -> int:
    """chunky_widetree_hit_top: 1 + the highest cell y of any leaf of the re-laid-out octree that can be hit under the block
    palette `blocks` (0: none can; 2^depth: one reaches the world's top)."""
    tree = np.ascontiguousarray(tree, np.int32)
    blocks = np.ascontiguousarray(blocks, np.int32)
    lb = None if level_bits is None else np.ascontiguousarray(level_bits, np.int32)
    top = C.c_int32()
    check(lib().chunky_widetree_hit_top(ptr(tree), tree.size, depth, None if lb is None else ptr(lb), 0 if lb is None else lb.size,
                                        ptr(blocks) if blocks.size else None, blocks.size, C.byref(top)))
    return top.value


# the instantiations of the kernels that tint by position (csrc/launch_plan.hpp CHUNKY_POOL_BIOME_INSTANCES, _BIOME_BVH_INSTANCES, CHUNKY_LANES_INSTANCES)
BIOME_POOL_FORMS, BIOME_POOL_BVH_FORMS, BIOME_LANES_FORMS = (0, 17, 18, -1), (17, -1), (0, -1)
BIOME_POOL_PARK, BIOME_POOL_BVH_PARKS = 64, (16, 32)


def plan_biome(plans16):
    """chunky_selftest_plan_biome: (plans (n, 16) int32, refusals (n,) int32) for launch plans given as rows of 16 ints (no device needed)."""
    p = np.ascontiguousarray(plans16, np.int32).reshape(-1, 16)
    out, why = np.zeros_like(p), np.zeros(len(p), np.int32)
    check(lib().chunky_selftest_plan_biome(ptr(p), len(p), ptr(out), ptr(why)))
    return out, why


# the instantiations of the kernels with the ground-fog layer (csrc/launch_plan.hpp CHUNKY_POOL_FOG_INSTANCES, _FOG_BVH_INSTANCES)
FOG_POOL_FORMS, FOG_POOL_PARK, FOG_POOL_BVH_PARK = (17, 18, -1), 32, 16
FOG_REFUSALS = ("none", "biome", "stats", "rig_bits", "projected", "max_depth", "wide_tree", "bvh_records", "not_pool")  # csrc/launch_plan.hpp FogRefusal


def fog_struct(density: float, y_min: float, y_max: float, color=(1.0, 1.0, 1.0)) -> Fog:
    """A chunky_fog with this library's size."""
    f = Fog()
    f.size = C.sizeof(Fog)
    f.density, f.y_min, f.y_max = float(density), float(y_min), float(y_max)
    for k in range(3):
        f.color[k] = float(color[k])
    return f


def fog_check(fog: Optional[Fog]) -> int:
    """chunky_fog_check: chunky_render_set_fog's own test of a layer, without a target or a device; the status code (0 = accepted)."""
    return int(lib().chunky_fog_check(None if fog is None else C.byref(fog)))


def plan_fog(rows8):
    """chunky_selftest_plan_fog: rows of 8 ints {kernel word, projector type, max depth, wide tree, entity BVHs, BVH records, biome map
    applied, wide levels} -> (out (n, 8) int32 {status, refusal, tree, park, bvh, ext, family, 0}, the refusals' texts).  No device needed."""
    p = np.ascontiguousarray(rows8, np.int32).reshape(-1, 8)
    out = np.zeros_like(p)
    text = C.create_string_buffer(256 * max(len(p), 1))
    check(lib().chunky_selftest_plan_fog(ptr(p), len(p), ptr(out), text))
    return out, [text.raw[256 * i:256 * (i + 1)].split(b"\0", 1)[0].decode() for i in range(len(p))]


# the instantiations of the kernels with translucent blocks (csrc/launch_plan.hpp CHUNKY_POOL_GLASS_INSTANCES, _GLASS_BVH_INSTANCES)
GLASS_POOL_FORMS, GLASS_POOL_PARK, GLASS_POOL_BVH_PARK, GLASS_POOL_WORDS = (17, 18, -1), 32, 16, 12
GLASS_REFUSALS = ("none", "fog", "biome", "stats", "rig_bits", "projected", "max_depth", "wide_tree", "bvh_records", "not_pool")  # csrc/launch_plan.hpp GlassRefusal


def translucency_struct(opaque_alpha: float = 0.99, max_crossings: int = 8) -> Translucency:
    """A chunky_translucency with this library's size."""
    t = Translucency()
    t.size = C.sizeof(Translucency)
    t.opaque_alpha, t.max_crossings = float(opaque_alpha), int(max_crossings)
    return t


def translucency_check(t: Optional[Translucency]) -> int:
    """chunky_translucency_check: chunky_render_set_translucency's own test, without a target or a device; the status code (0 = accepted)."""
    return int(lib().chunky_translucency_check(None if t is None else C.byref(t)))


def plan_glass(rows9):
    """chunky_selftest_plan_glass: rows of 9 ints {kernel word, projector type, max depth, wide tree, entity BVHs, BVH records, biome map
    applied, wide levels, fog layer} -> (out (n, 8) int32 {status, refusal, tree, park, bvh, ext, family, words}, the refusals' texts).
    No device needed."""
    p = np.ascontiguousarray(rows9, np.int32).reshape(-1, 9)
    out = np.zeros((len(p), 8), np.int32)
    text = C.create_string_buffer(256 * max(len(p), 1))
    check(lib().chunky_selftest_plan_glass(ptr(p), len(p), ptr(out), text))
    return out, [text.raw[256 * i:256 * (i + 1)].split(b"\0", 1)[0].decode() for i in range(len(p))]


ADDR32_ATLAS, ADDR32_SKY, ADDR32_RECORDS = 1, 2, 4  # chunky_addr32_word / chunky_scene_addr32 (csrc/addr32.h)


def addr32_word(atlas=(1, 1, 1), sky=(1, 1), record_bytes=(0, 0), indices_checked: bool = True) -> int:
    """chunky_addr32_word: which scene arrays kernels may address by 32-bit offsets, for an atlas (width, height, layers), a sky
    (width, height), the sizes in bytes of (aabb_rec, quad_rec) and whether those arrays are the library's own."""
    dims = np.array([*atlas, *sky], np.int64)
    sizes = np.array(record_bytes, np.uint64)
    assert dims.size == 5 and sizes.size == 2
    word = C.c_uint32()
    check(lib().chunky_addr32_word(ptr(dims), ptr(sizes), 1 if indices_checked else 0, C.byref(word)))
    return word.value


def denoise_params(iterations: Optional[int] = None, sigma_color: Optional[float] = None, sigma_normal: Optional[float] = None,
                   sigma_albedo: Optional[float] = None, demodulate: Optional[bool] = None, kernel: int = 0) -> DenoiseParams:
    """chunky_denoise_default_params with the given members replaced; `kernel` picks the tap-fetch form (bit-identical)."""
    p = DenoiseParams()
    check(lib().chunky_denoise_default_params(C.byref(p)))
    if iterations is not None:
        p.iterations = int(iterations)
    if sigma_color is not None:
        p.sigma_color = float(sigma_color)
    if sigma_normal is not None:
        p.sigma_normal = float(sigma_normal)
    if sigma_albedo is not None:
        p.sigma_albedo = float(sigma_albedo)
    if demodulate is not None:
        p.flags = (p.flags & ~DENOISE_DEMODULATE) | (DENOISE_DEMODULATE if demodulate else 0)
    p.flags |= int(kernel) << DENOISE_KERNEL_SHIFT
    return p


def _images(width, height, *arrays):
    out = []
    for a in arrays:
        a = np.ascontiguousarray(a, np.float32).reshape(-1)
        if a.size != 3 * int(width) * int(height):
            raise ValueError(f"expected {3 * int(width) * int(height)} floats, got {a.size}")
        out.append(a)
    return out


def denoise_host(width: int, height: int, color, albedo, normal, params: Optional[DenoiseParams] = None) -> np.ndarray:
    """chunky_denoise_host: the filter's specification, evaluated on the host (no device needed)."""
    c, a, n = _images(width, height, color, albedo, normal)
    p = params if params is not None else denoise_params()
    out = np.zeros(c.size, np.float32)
    check(lib().chunky_denoise_host(int(width), int(height), ptr(c), ptr(a), ptr(n), C.byref(p), ptr(out)))
    return out


def denoise_exp(x) -> np.ndarray:
    """chunky_denoise_exp: the filter's e^(-x) on the host."""
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    out = np.zeros(x.size, np.float32)
    check(lib().chunky_denoise_exp(ptr(x), x.size, ptr(out)))
    return out


def adaptive_params(threshold: Optional[float] = None, floor: Optional[float] = None, min_spp: Optional[int] = None,
                    check_interval: Optional[int] = None) -> AdaptiveParams:
    """chunky_adaptive_default_params with the given members replaced."""
    p = AdaptiveParams()
    check(lib().chunky_adaptive_default_params(C.byref(p)))
    if threshold is not None:
        p.threshold = float(threshold)
    if floor is not None:
        p.floor = float(floor)
    if min_spp is not None:
        p.min_spp = int(min_spp)
    if check_interval is not None:
        p.check_interval = int(check_interval)
    return p


def adaptive_host(samples, params: Optional[AdaptiveParams] = None):
    """chunky_adaptive_host: the specification of adaptive sampling evaluated on the host (no device needed).  samples: (n, height,
    width, 3) float32, the sample of every pass.  Returns (counts (h, w) int32, image (h, w, 3), noise (h, w, 2) = (m, M2))."""
    s = np.ascontiguousarray(samples, np.float32)
    if s.ndim != 4 or s.shape[3] != 3:
        raise ValueError(f"expected samples of shape (n, height, width, 3), got {s.shape}")
    n, h, w, _ = s.shape
    p = params if params is not None else adaptive_params()
    counts = np.zeros((h, w), np.int32)
    mean = np.zeros((h, w, 3), np.float32)
    stat = np.zeros((h, w, 2), np.float32)
    check(lib().chunky_adaptive_host(w, h, ptr(s), n, C.byref(p), ptr(counts), ptr(mean), ptr(stat)))
    return counts, mean, stat


def matte_host_fold(sample_ids, state=None):
    """chunky_matte_host_fold: the ID-matte state after the samples sample_ids (n_passes, n_pixels) int32, continued from `state` =
    (ids (6, n_pixels), counts (6, n_pixels), other (n_pixels,)) or from the empty state.  Returns new arrays (no device needed)."""
    s = np.ascontiguousarray(sample_ids, np.int32)
    if s.ndim != 2:
        raise ValueError(f"expected sample ids of shape (n_passes, n_pixels), got {s.shape}")
    n = s.shape[1]
    if state is None:
        ids, counts, other = np.zeros((MATTE_SLOTS, n), np.int32), np.zeros((MATTE_SLOTS, n), np.int32), np.zeros(n, np.int32)
    else:
        ids, counts, other = (np.array(a, np.int32, order="C") for a in state)
    check(lib().chunky_matte_host_fold(ptr(s), s.shape[0], n, ptr(ids), ptr(counts), ptr(other)))
    return ids, counts, other


def matte_host_ranks(ids, counts, passes: int):
    """chunky_matte_host_ranks: (ids (6, n_pixels) int32, coverage (6, n_pixels) float32) by rank."""
    i, c = np.ascontiguousarray(ids, np.int32), np.ascontiguousarray(counts, np.int32)
    n = i.shape[-1]
    out_ids, out_cov = np.zeros((MATTE_SLOTS, n), np.int32), np.zeros((MATTE_SLOTS, n), np.float32)
    check(lib().chunky_matte_host_ranks(ptr(i), ptr(c), n, int(passes), ptr(out_ids), ptr(out_cov)))
    return out_ids, out_cov


def matte_host_extract(ids, counts, passes: int, id_set) -> np.ndarray:
    """chunky_matte_host_extract: the (n_pixels,) float32 mask of the ids in id_set."""
    i, c = np.ascontiguousarray(ids, np.int32), np.ascontiguousarray(counts, np.int32)
    st = np.ascontiguousarray(id_set, np.int32).reshape(-1)
    n = i.shape[-1]
    out = np.zeros(n, np.float32)
    check(lib().chunky_matte_host_extract(ptr(i), ptr(c), n, int(passes), ptr(st) if st.size else None, st.size, ptr(out)))
    return out


def matte_state_check(ids, counts, other, passes: int) -> int:
    """chunky_matte_state_check: the status (0, or E_INVALID with the rule in chunky_last_error)."""
    i, c, o = (np.ascontiguousarray(a, np.int32) for a in (ids, counts, other))
    return lib().chunky_matte_state_check(ptr(i), ptr(c), ptr(o), o.size, int(passes))


def adaptive_summary_dict(summ: AdaptiveSummary) -> dict:
    return {"rounds": summ.rounds, "checks": summ.checks, "passes": summ.passes, "samples": summ.samples,
            "active": [int(a) for a in summ.active[:min(summ.checks, ADAPTIVE_MAX_CHECKS)]]}


class AdaptiveRun:
    """A run's whole state on the host: the header (`state`, an AdaptiveState) and the arrays `mean` (h, w, 3) float32, `count`
    (h, w) int32, `stat` (h, w, 2) float32 and `active` (h, w) uint8 — what chunky_adaptive_host_begin / _resume work on in place and
    what chunky_render_adaptive_state / _restore move between a target and the host."""

    def __init__(self, state: AdaptiveState, mean, count, stat, active):
        h, w = state.height, state.width
        self.state = state
        self.mean = np.ascontiguousarray(mean, np.float32).reshape(h, w, 3)
        self.count = np.ascontiguousarray(count, np.int32).reshape(h, w)
        self.stat = np.ascontiguousarray(stat, np.float32).reshape(h, w, 2)
        self.active = np.ascontiguousarray(active, np.uint8).reshape(h, w)

    def copy(self) -> "AdaptiveRun":
        st = AdaptiveState()
        C.memmove(C.byref(st), C.byref(self.state), C.sizeof(st))
        return AdaptiveRun(st, self.mean.copy(), self.count.copy(), self.stat.copy(), self.active.copy())

    @property
    def summary(self) -> dict:
        return adaptive_summary_dict(self.state.summary)

    def header_bytes(self) -> bytes:
        return bytes(memoryview(self.state))


def adaptive_host_begin(width: int, height: int, params: Optional[AdaptiveParams] = None) -> AdaptiveRun:
    """chunky_adaptive_host_begin: the start state (no pass yet, every pixel active)."""
    p = params if params is not None else adaptive_params()
    st = AdaptiveState()
    st.size = C.sizeof(AdaptiveState)
    h, w = int(height), int(width)
    run = AdaptiveRun.__new__(AdaptiveRun)
    run.state = st
    run.mean, run.count = np.empty((h, w, 3), np.float32), np.empty((h, w), np.int32)
    run.stat, run.active = np.empty((h, w, 2), np.float32), np.empty((h, w), np.uint8)
    check(lib().chunky_adaptive_host_begin(w, h, C.byref(p), C.byref(st), ptr(run.count), ptr(run.mean), ptr(run.stat), ptr(run.active)))
    return run


def adaptive_host_resume(run: AdaptiveRun, samples) -> AdaptiveRun:
    """chunky_adaptive_host_resume: continues `run` in place with the samples of its next len(samples) passes; returns it."""
    s = np.ascontiguousarray(samples, np.float32)
    if s.ndim != 4 or s.shape[1:] != (run.state.height, run.state.width, 3):
        raise ValueError(f"expected samples of shape (n, {run.state.height}, {run.state.width}, 3), got {s.shape}")
    check(lib().chunky_adaptive_host_resume(C.byref(run.state), ptr(s), s.shape[0], ptr(run.count), ptr(run.mean), ptr(run.stat), ptr(run.active)))
    return run


def adaptive_state_check(run: AdaptiveRun) -> None:
    """chunky_adaptive_state_check: raises ChunkyHipError (E_INVALID) for a state no run can have left."""
    check(lib().chunky_adaptive_state_check(C.byref(run.state), ptr(run.count), ptr(run.active)))


def robust_params(mode: Optional[int] = None, gain: Optional[float] = None) -> RobustParams:
    """chunky_robust_default_params (ROBUST_GINI, gain 1) with the given members replaced."""
    p = RobustParams()
    check(lib().chunky_robust_default_params(C.byref(p)))
    if mode is not None:
        p.mode = int(mode)
    if gain is not None:
        p.gain = float(gain)
    return p


def robust_host(samples, n_buckets: int, first_index: int = 0, buckets=None) -> np.ndarray:
    """chunky_robust_host: the bucket means (n_buckets, h, w, 3) after the per-pass samples (n, h, w, 3) float32, taken as robust
    samples first_index .. and folded into a copy of `buckets` (default: zero).  No device needed."""
    s = np.ascontiguousarray(samples, np.float32)
    if s.ndim != 4 or s.shape[3] != 3:
        raise ValueError(f"expected samples of shape (n, height, width, 3), got {s.shape}")
    n, h, w, _ = s.shape
    b = np.zeros((int(n_buckets), h, w, 3), np.float32) if buckets is None else np.array(buckets, np.float32, order="C").reshape(int(n_buckets), h, w, 3)
    check(lib().chunky_robust_host(w, h, ptr(s), n, int(n_buckets), int(first_index), ptr(b)))
    return b


def robust_host_resolve(buckets, params: Optional[RobustParams] = None):
    """chunky_robust_host_resolve: (image (..., 3) float32, trim (...) uint8) of bucket means (n_buckets, ..., 3).  No device needed."""
    b = np.ascontiguousarray(buckets, np.float32)
    if b.ndim < 3 or b.shape[-1] != 3:
        raise ValueError(f"expected buckets of shape (n_buckets, ..., 3), got {b.shape}")
    p = params if params is not None else robust_params()
    out = np.empty(b.shape[1:], np.float32)
    trim = np.empty(b.shape[1:-1], np.uint8)
    check(lib().chunky_robust_host_resolve(b.shape[0], trim.size, ptr(b), C.byref(p), ptr(out), ptr(trim)))
    return out, trim
