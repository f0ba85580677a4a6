"""ctypes binding of libpais_hip.so (include/pais_hip.h, include/pais_mvs.h).

The product path fails loudly when the HIP library is missing or no GPU is
present: there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os

from . import build as _build

MAX_LEVELS = 16
MAX_VIS = 64


class Config(C.Structure):
    _fields_ = [
        ("cellSize", C.c_int32), ("patchRadius", C.c_int32), ("patchSize", C.c_int32), ("minCamNum", C.c_int32),
        ("textureVariation", C.c_double), ("visibleCorrelation", C.c_double), ("minCorrelation", C.c_double),
        ("maxFitness", C.c_double), ("lodRatio", C.c_double),
        ("minLOD", C.c_int32), ("maxLOD", C.c_int32), ("maxCellPatchNum", C.c_int32), ("_pad0", C.c_int32),
        ("reduceNormalRange", C.c_double),
        ("adaptiveDistanceEnable", C.c_int32), ("adaptiveDifferenceEnable", C.c_int32),
        ("adaptiveGradientEnable", C.c_int32), ("_pad1", C.c_int32),
        ("distWeighting", C.c_double), ("diffWeighting", C.c_double), ("gradientWeighting", C.c_double),
        ("neighborRadius", C.c_double), ("neighborRadiusScalar", C.c_double), ("minRegionRatio", C.c_double),
        ("depthRangeScalar", C.c_double),
        ("particleNum", C.c_int32), ("maxIteration", C.c_int32), ("expansionStrategy", C.c_int32), ("_pad2", C.c_int32),
    ]


class CameraDesc(C.Structure):
    _fields_ = [
        ("focal", C.c_double * 2), ("principle_point", C.c_double * 2), ("rotation", C.c_double * 9),
        ("translation", C.c_double * 3), ("center", C.c_double * 3), ("KR", C.c_double * 9), ("KT", C.c_double * 3),
        ("optical_normal", C.c_double * 3), ("max_lod", C.c_int32), ("_pad", C.c_int32),
        ("level_width", C.c_int32 * MAX_LEVELS), ("level_height", C.c_int32 * MAX_LEVELS),
        ("level_stride", C.c_int64 * MAX_LEVELS),
        ("level_image", C.c_void_p * MAX_LEVELS), ("level_edge", C.c_void_p * MAX_LEVELS),
    ]


class PatchState(C.Structure):
    _fields_ = [("ray", C.c_double * 3), ("ref_cam", C.c_int32), ("lod", C.c_int32), ("num_cam", C.c_int32),
                ("_pad", C.c_int32), ("cam_idx", C.c_int32 * MAX_VIS)]


class Candidate(C.Structure):
    _fields_ = [("center", C.c_double * 3), ("normal", C.c_double * 3), ("normalS", C.c_double * 2),
                ("key", C.c_uint64), ("type", C.c_int32), ("num_cam", C.c_int32), ("cam_idx", C.c_int32 * MAX_VIS)]


class PatchResult(C.Structure):
    _fields_ = [
        ("center", C.c_double * 3), ("normal", C.c_double * 3), ("normalS", C.c_double * 2), ("ray", C.c_double * 3),
        ("depth", C.c_double), ("depthRange", C.c_double * 2), ("fitness", C.c_double), ("priority", C.c_double),
        ("correlation", C.c_double), ("imgPoint", (C.c_double * 2) * MAX_VIS), ("key", C.c_uint64),
        ("type", C.c_int32), ("dropped", C.c_int32), ("num_cam", C.c_int32), ("ref_cam", C.c_int32),
        ("lod", C.c_int32), ("pso_runs", C.c_int32), ("pso_iterations", C.c_int32), ("pso_evals", C.c_int32),
        ("cam_idx", C.c_int32 * MAX_VIS),
        ("stage", C.c_int32), ("before_ref", C.c_int32), ("before_num", C.c_int32), ("after_ref", C.c_int32),
        ("after_num", C.c_int32), ("count", C.c_int32), ("total_cam_num", C.c_int32), ("ncc_tables", C.c_int32),
    ]

    def cams(self):
        return [int(self.cam_idx[i]) for i in range(self.num_cam)]


class ViewState(C.Structure):
    """pais_view_state: what Patch::removeInvisibleCamera reads (pais_ncc_batch)."""
    _fields_ = [("center", C.c_double * 3), ("normal", C.c_double * 3), ("ref_cam", C.c_int32), ("lod", C.c_int32),
                ("num_cam", C.c_int32), ("_pad", C.c_int32), ("cam_idx", C.c_int32 * MAX_VIS)]


class ViewResult(C.Structure):
    """pais_view_result: one removeInvisibleCamera with its intermediates (pais_ncc_batch)."""
    _fields_ = [("correlation", C.c_double), ("region_ratio", C.c_double * MAX_VIS), ("dropped", C.c_int32),
                ("max_idx", C.c_int32), ("num_kept", C.c_int32), ("_pad", C.c_int32), ("reason", C.c_int32 * MAX_VIS),
                ("kept_idx", C.c_int32 * MAX_VIS)]


class LoadedPatch(C.Structure):
    """pais_loaded_patch: one patch record of an MVS file (pais_load_state_batch, pais_mvs_load_patches)."""
    _fields_ = [("center", C.c_double * 3), ("normalS", C.c_double * 2), ("fitness", C.c_double), ("correlation", C.c_double),
                ("num_cam", C.c_int32), ("_pad", C.c_int32), ("cam_idx", C.c_int32 * MAX_VIS)]


# pais_view_result.reason / .dropped (include/pais_hip.h)
VIEW_KEEP, VIEW_REGION, VIEW_BACKFACING, VIEW_CORRELATION = 0, 1, 2, 3
VIEW_DROP_SAMPLE, VIEW_DROP_MINCAM = 1, 2


class CostDetail(C.Structure):
    """pais_cost_detail: the outcome and the sums of one cost evaluation (pais_fitness_detail)."""
    _fields_ = [("fitness", C.c_double), ("sum_weight", C.c_double), ("sum_weighted_sad", C.c_double), ("pt", C.c_double * 2),
                ("outcome", C.c_int32), ("nx", C.c_int32), ("ny", C.c_int32), ("live_pixels", C.c_int32),
                ("overflow_pixel", C.c_int32), ("overflow_cam", C.c_int32), ("ref_pos", C.c_int32), ("_pad", C.c_int32)]


# pais_cost_detail.outcome / the per-pixel codes of pais_fitness_detail (include/pais_hip.h)
COST_OK, COST_BACKFACING, COST_OFF_IMAGE, COST_WINDOW, COST_OVERFLOW, COST_ALL_MASKED = 0, 1, 2, 3, 4, 5
PIX_COUNTED, PIX_MASKED, PIX_OVERFLOW, PIX_NONE = 0, 1, 2, 3


class PsoRunInfo(C.Structure):
    """pais_pso_run_info: one psoOptimization() call of a pais_pso_trace (patch.cpp:180-219)."""
    _fields_ = [("range_l", C.c_double * 3), ("range_u", C.c_double * 3), ("init", C.c_double * 3), ("ray", C.c_double * 3),
                ("run", C.c_int32), ("ref_cam", C.c_int32), ("lod", C.c_int32), ("num_cam", C.c_int32),
                ("n_particles", C.c_int32), ("max_iteration", C.c_int32), ("iterations", C.c_int32), ("_pad", C.c_int32),
                ("cam_idx", C.c_int32 * MAX_VIS)]


class PsoIter(C.Structure):
    """pais_pso_iter: one row of a pais_pso_trace -- the swarm after updateGbest and the inertia update."""
    _fields_ = [("gbest_fitness", C.c_double), ("gbest", C.c_double * 3), ("iw", C.c_double), ("dispersion", C.c_double),
                ("velocity", C.c_double), ("g_idx", C.c_int32), ("iteration", C.c_int32), ("ended", C.c_int32), ("_pad", C.c_int32)]


class View(C.Structure):
    """pais_view (include/pais_render.h): X' = R X + T, u = focal[0] X'0 / X'2 + pp[0]."""
    _fields_ = [("R", C.c_double * 9), ("T", C.c_double * 3), ("focal", C.c_double * 2), ("pp", C.c_double * 2)]


# include/pais_render.h
RENDER_DISC, RENDER_POINT, RENDER_CULL_BACK, RENDER_MAX_POINT_SIZE = 0, 1, 1, 64
VIS_VISIBLE, VIS_OCCLUDED, VIS_IN_FRONT, VIS_EMPTY, VIS_OUTSIDE, VIS_BEHIND, VIS_SELF = 0, 1, 2, 3, 4, 5, 0x100
CLOUD_MAX_K, KNN_SKIP_SAME_INDEX = 32, 1      # include/pais_cloud.h
PLANE_WITH_QUERY, PLANE_ORIENT = 2, 4
PLANE_OK, PLANE_FEW, PLANE_NOCONV, PLANE_SWEEPS = 0, 1, 2, 60


class Plane(C.Structure):
    """pais_plane (include/pais_cloud.h): the plane fitted to one query's neighbourhood (pais_cloud_planes)."""
    _fields_ = [("centroid", C.c_double * 3), ("normal", C.c_double * 3), ("eigen", C.c_double * 3), ("offset", C.c_double),
                ("variation", C.c_double), ("count", C.c_int32), ("status", C.c_int32)]


class Grid(C.Structure):
    """pais_grid (include/pais_mesh.h): n vertices per axis at origin + i h."""
    _fields_ = [("origin", C.c_double * 3), ("h", C.c_double), ("n", C.c_int32 * 3), ("reserved", C.c_int32)]


MESH_MAX_VERTICES = 1 << 28                   # include/pais_mesh.h


class Lens(C.Structure):
    """pais_lens (include/pais_undistort.h): the radial term k of a camera with focal / pp, and the direction G runs in."""
    _fields_ = [("focal", C.c_double * 2), ("pp", C.c_double * 2), ("k", C.c_double), ("model", C.c_int32), ("_pad", C.c_int32)]


# include/pais_undistort.h
LENS_MEASURED_TO_IDEAL, LENS_IDEAL_TO_MEASURED = 0, 1


class KernelStats(C.Structure):
    _fields_ = [("pso_ms", C.c_double), ("begin_ms", C.c_double), ("after_ms", C.c_double),
                ("pso_launches", C.c_int64), ("pso_evals", C.c_int64), ("pso_patches", C.c_int64),
                ("pso_algorithmic_bytes", C.c_double), ("ncc_algorithmic_bytes", C.c_double),
                ("ncc_tables", C.c_int64), ("eval_ms", C.c_double), ("eval_launches", C.c_int64),
                ("eval2_ms", C.c_double), ("eval2_launches", C.c_int64), ("eval2_evals", C.c_int64),
                ("eval2_algorithmic_bytes", C.c_double), ("tile_launches", C.c_int64), ("eval2_busy_ms", C.c_double), ("ring_launches", C.c_int64),
                ("ring_ms", C.c_double), ("ring_evals", C.c_int64), ("ring_algorithmic_bytes", C.c_double), ("ring_fallbacks", C.c_int64)]


_lib = None


def load(build_if_needed: bool = True):
    """Load libpais_hip.so; raises if it is absent (no fallback path exists)."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("PAIS_LIB_PATH") or _build.LIB   # PAIS_LIB_PATH: another build of the library (scripts/ab.sh, measurement builds)
    if path != _build.LIB:
        build_if_needed = False
    # several ranks of one job must not race to rebuild the same file: a multi-process launch (torch.distributed.run
    # sets WORLD_SIZE) only ever loads what __graft_entry__.build() / `python -m pais_mvs_amd.build` produced
    if int(os.environ.get("WORLD_SIZE", "1")) > 1 or os.environ.get("PAIS_NO_BUILD"):
        build_if_needed = False
    if build_if_needed and _build.needs_build():
        try:
            _build.build()
        except Exception as e:  # built .so travels to the GPU box; hipcc may be absent there
            if not os.path.exists(path):
                raise RuntimeError("libpais_hip.so is missing and could not be built: %s" % e)
    if not os.path.exists(path):
        raise RuntimeError("libpais_hip.so not found at %s -- run `python -m pais_mvs_amd.build`" % path)
    L = C.CDLL(path)
    L.pais_last_error.restype = C.c_char_p
    for n in ("pais_sizeof_config", "pais_sizeof_camera_desc", "pais_sizeof_candidate", "pais_sizeof_patch_result",
              "pais_sizeof_view_state", "pais_sizeof_view_result", "pais_sizeof_cost_detail",
              "pais_sizeof_pso_run_info", "pais_sizeof_pso_iter", "pais_sizeof_loaded_patch"):
        getattr(L, n).restype = C.c_size_t
    assert L.pais_sizeof_config() == C.sizeof(Config), (L.pais_sizeof_config(), C.sizeof(Config))
    assert L.pais_sizeof_camera_desc() == C.sizeof(CameraDesc)
    assert L.pais_sizeof_candidate() == C.sizeof(Candidate)
    assert L.pais_sizeof_patch_result() == C.sizeof(PatchResult), (L.pais_sizeof_patch_result(), C.sizeof(PatchResult))
    assert L.pais_sizeof_view_state() == C.sizeof(ViewState), (L.pais_sizeof_view_state(), C.sizeof(ViewState))
    assert L.pais_sizeof_view_result() == C.sizeof(ViewResult), (L.pais_sizeof_view_result(), C.sizeof(ViewResult))
    assert L.pais_sizeof_cost_detail() == C.sizeof(CostDetail), (L.pais_sizeof_cost_detail(), C.sizeof(CostDetail))
    assert L.pais_sizeof_pso_run_info() == C.sizeof(PsoRunInfo), (L.pais_sizeof_pso_run_info(), C.sizeof(PsoRunInfo))
    assert L.pais_sizeof_pso_iter() == C.sizeof(PsoIter), (L.pais_sizeof_pso_iter(), C.sizeof(PsoIter))
    assert L.pais_sizeof_loaded_patch() == C.sizeof(LoadedPatch), (L.pais_sizeof_loaded_patch(), C.sizeof(LoadedPatch))
    L.pais_ctx_create.restype = C.c_int
    L.pais_ctx_create.argtypes = [C.POINTER(Config), C.c_int, C.POINTER(CameraDesc), C.c_int, C.c_uint64,
                                  C.POINTER(C.c_void_p)]
    L.pais_ctx_set_config.argtypes = [C.c_void_p, C.POINTER(Config)]
    L.pais_ctx_set_neighbor_radius.argtypes = [C.c_void_p, C.c_double]
    L.pais_ctx_destroy.argtypes = [C.c_void_p]
    L.pais_ctx_destroy.restype = None
    L.pais_ctx_stream.restype = C.c_void_p
    L.pais_ctx_stream.argtypes = [C.c_void_p]
    L.pais_ctx_synchronize.argtypes = [C.c_void_p]
    L.pais_fitness_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(PatchState), C.c_int, C.POINTER(C.c_int32),
                                     C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.pais_refine_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(Candidate), C.POINTER(PatchResult)]
    L.pais_refine_batch_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    L.pais_refine_batch_begin.argtypes = [C.c_void_p, C.c_int, C.POINTER(Candidate)]
    L.pais_refine_batch_open.argtypes = [C.c_void_p, C.c_int, C.POINTER(Candidate), C.c_int]
    L.pais_refine_batch_enqueue.argtypes = [C.c_void_p, C.c_int]
    L.pais_ctx_set_round_hint.argtypes = [C.c_void_p, C.c_int]
    L.pais_refine_batch_end.argtypes = [C.c_void_p, C.POINTER(C.POINTER(PatchResult))]
    L.pais_ctx_fork_lane.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    L.pais_get_kernel_stats.argtypes = [C.c_void_p, C.POINTER(KernelStats), C.c_int]
    L.pais_ctx_set_fine_timing.argtypes = [C.c_void_p, C.c_int]
    L.pais_neighbor_count.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.c_double, C.POINTER(C.c_int32), C.POINTER(C.c_double)]
    L.pais_ncc_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(ViewState), C.POINTER(ViewResult), C.POINTER(C.c_double), C.c_int]
    L.pais_fitness_detail.argtypes = [C.c_void_p, C.c_int, C.POINTER(PatchState), C.c_int, C.POINTER(C.c_int32),
                                      C.POINTER(C.c_double), C.POINTER(CostDetail), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                      C.POINTER(C.c_int8), C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int]
    L.pais_pso_trace.argtypes = [C.c_void_p, C.c_int, C.POINTER(Candidate), C.c_int, C.POINTER(PatchResult), C.c_void_p, C.c_void_p,
                                 C.POINTER(C.c_double)]
    L.pais_pso_trace_shape.argtypes = [C.c_void_p, C.c_int, C.POINTER(Candidate), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.pais_get_trace_stats.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int]
    L.pais_get_detail_stats.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int]
    L.pais_get_ncc_stats.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int]
    L.pais_load_state_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(LoadedPatch), C.POINTER(PatchResult)]
    L.pais_get_load_stats.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int]
    # include/pais_cloud.h
    L.pais_cloud_nearest.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double),
                                     C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.pais_cloud_knn.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double),
                                 C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.pais_cloud_outlier_rule.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_double,
                                          C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint8)]
    L.pais_cloud_normals.argtypes = [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.pais_sizeof_plane.restype = C.c_size_t
    assert L.pais_sizeof_plane() == C.sizeof(Plane), (L.pais_sizeof_plane(), C.sizeof(Plane))
    L.pais_cloud_planes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double),
                                    C.POINTER(C.c_double), C.POINTER(Plane), C.POINTER(C.c_int32), C.POINTER(C.c_double),
                                    C.POINTER(C.c_double)]
    L.pais_cloud_planes_last_ms.restype = None
    L.pais_cloud_planes_last_ms.argtypes = [C.POINTER(C.c_double)]
    L.pais_cloud_normal_rule.argtypes = [C.c_int, C.POINTER(Plane), C.POINTER(C.c_double), C.c_double, C.POINTER(C.c_uint8)]
    L.pais_cloud_launches.restype = C.c_int64
    L.pais_cloud_launches.argtypes = []
    L.pais_cloud_last_error.restype = C.c_char_p
    # include/pais_mesh.h
    L.pais_sizeof_grid.restype = C.c_size_t
    assert L.pais_sizeof_grid() == C.sizeof(Grid), (L.pais_sizeof_grid(), C.sizeof(Grid))
    L.pais_cloud_field.argtypes = [C.c_int, C.c_int, C.POINTER(Grid), C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double,
                                   C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.pais_field_surface.argtypes = [C.c_int, C.POINTER(Grid), C.POINTER(C.c_double), C.c_int, C.c_int64, C.POINTER(C.c_int64),
                                     C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.pais_mesh_weld.argtypes = [C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_int64,
                                 C.POINTER(C.c_double), C.POINTER(C.c_int32)]
    L.pais_mesh_last_ms.restype = None
    L.pais_mesh_last_ms.argtypes = [C.POINTER(C.c_double)]
    L.pais_mesh_launches.restype = C.c_int64
    L.pais_mesh_launches.argtypes = []
    L.pais_mesh_last_error.restype = C.c_char_p
    # include/pais_render.h
    L.pais_sizeof_view.restype = C.c_size_t
    assert L.pais_sizeof_view() == C.sizeof(View), (L.pais_sizeof_view(), C.sizeof(View))
    L.pais_cloud_render.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                    C.POINTER(C.c_double), C.c_double, C.c_int, C.POINTER(View), C.c_int, C.c_int,
                                    C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_double)]
    L.pais_render_launches.restype = C.c_int64
    L.pais_render_launches.argtypes = []
    L.pais_render_last_error.restype = C.c_char_p
    L.pais_render_last_counts.restype = None
    L.pais_render_last_counts.argtypes = [C.POINTER(C.c_int64)] * 4
    L.pais_depth_test.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_int, C.POINTER(View), C.c_int, C.c_int,
                                  C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_double, C.POINTER(C.c_uint8), C.POINTER(C.c_int32),
                                  C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.pais_cloud_visibility.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                        C.POINTER(C.c_double), C.c_double, C.c_int, C.POINTER(C.c_double), C.c_int, C.POINTER(View),
                                        C.c_int, C.c_int, C.c_double, C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_double),
                                        C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_double)]
    L.pais_mesh_render.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int32), C.c_int, C.POINTER(View),
                                   C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_double)]
    L.pais_mesh_visibility.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int32), C.c_int,
                                       C.POINTER(C.c_double), C.c_int, C.POINTER(View), C.c_int, C.c_int, C.c_double, C.POINTER(C.c_uint8),
                                       C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32),
                                       C.POINTER(C.c_double)]
    L.pais_render_last_packed.restype = C.c_int64
    L.pais_render_last_packed.argtypes = []
    L.pais_mesh_render_last_ms.restype = None
    L.pais_mesh_render_last_ms.argtypes = [C.POINTER(C.c_double)]
    L.pais_cloud_visibility_last_ms.restype = None
    L.pais_cloud_visibility_last_ms.argtypes = [C.POINTER(C.c_double)]
    L.pais_cloud_visibility_rule.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int,
                                             C.POINTER(C.c_int32), C.POINTER(C.c_uint8)]
    # include/pais_undistort.h
    L.pais_sizeof_lens.restype = C.c_size_t
    assert L.pais_sizeof_lens() == C.sizeof(Lens), (L.pais_sizeof_lens(), C.sizeof(Lens))
    for n in ("pais_undistort_points", "pais_distort_points"):
        getattr(L, n).argtypes = [C.c_int, C.POINTER(Lens), C.c_int64, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                  C.POINTER(C.c_uint8), C.POINTER(C.c_double)]
    L.pais_undistort_image.argtypes = [C.c_int, C.POINTER(Lens), C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_void_p,
                                       C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_double)]
    L.pais_undistort_launches.restype = C.c_int64
    L.pais_undistort_launches.argtypes = []
    L.pais_undistort_last_error.restype = C.c_char_p
    L.pais_rand31.restype = C.c_uint32
    L.pais_rand31.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32]
    L.pais_child_key.restype = C.c_uint64
    L.pais_child_key.argtypes = [C.c_uint64, C.c_int, C.c_int, C.c_int]
    _lib = L
    return L


def check(rc: int, what: str = ""):
    if rc != 0:
        raise RuntimeError("%s failed (%d): %s" % (what or "pais call", rc, load().pais_last_error().decode()))
