"""Per-scene GPU context (pais_ctx) and the batch entry points."""
from __future__ import annotations

import ctypes as C
import math
from typing import List, Sequence

import numpy as np

from . import _lib
from .camera import Camera
from .config import MvsConfig


def camera_desc(cam: Camera, with_edges: bool, keep: list) -> "_lib.CameraDesc":
    d = _lib.CameraDesc()
    d.focal[:] = list(map(float, cam.focal))
    d.principle_point[:] = list(map(float, cam.principle_point))
    d.rotation[:] = cam.rotation.ravel().tolist()
    d.translation[:] = cam.translation.tolist()
    d.center[:] = cam.center.tolist()
    d.KR[:] = cam.KR.ravel().tolist()
    d.KT[:] = cam.KT.tolist()
    d.optical_normal[:] = cam.optical_normal.tolist()
    d.max_lod = cam.max_lod
    for l, img in enumerate(cam.pyramid):
        img = np.ascontiguousarray(img, dtype=np.uint8)
        keep.append(img)
        d.level_width[l] = img.shape[1]
        d.level_height[l] = img.shape[0]
        d.level_stride[l] = img.strides[0]
        d.level_image[l] = img.ctypes.data
        if with_edges and cam.edge_pyramid:     # no host edge pyramid: the library evaluates the maps on the fly
            e = np.ascontiguousarray(cam.edge_pyramid[l], dtype=np.float64)
            keep.append(e)
            d.level_edge[l] = e.ctypes.data
    return d


def normal_to_spherical(n) -> List[float]:
    """Utility::normal2Spherical (utility.h:17-22)."""
    return [math.acos(float(n[2])), math.atan2(float(n[1]), float(n[0]))]


class Context:
    """Owns one pais_ctx: scene data resident in HBM on one GPU."""

    def __init__(self, cfg: MvsConfig, cameras: Sequence[Camera], device: int = 0, seed: int = 42):
        self.L = _lib.load()
        self.cfg = cfg
        self.cameras = list(cameras)
        self._keep: list = []
        n = len(self.cameras)
        descs = (_lib.CameraDesc * n)()
        for i, cam in enumerate(self.cameras):
            descs[i] = camera_desc(cam, bool(cfg.adaptiveGradientEnable), self._keep)
        self._c_cfg = cfg.to_c()
        h = C.c_void_p()
        _lib.check(self.L.pais_ctx_create(C.byref(self._c_cfg), n, descs, device, seed, C.byref(h)), "pais_ctx_create")
        self.h = h
        self._keep.clear()   # the library copied everything into HBM

    def close(self):
        if getattr(self, "h", None):
            self.L.pais_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_config(self, cfg: MvsConfig):
        """Replace the configuration of this context and of its lanes (pais_ctx_set_config); the scene stays.  Raises RuntimeError
        when the library refuses cfg (a field out of range, the gradient weighting on a context created without edges, a lane, an
        open batch): the context then keeps the configuration it had, and so does `self.cfg`."""
        c_cfg = cfg.to_c()
        _lib.check(self.L.pais_ctx_set_config(self.h, C.byref(c_cfg)), "pais_ctx_set_config")
        self.cfg = cfg
        self._c_cfg = c_cfg

    def set_neighbor_radius(self, r: float):
        _lib.check(self.L.pais_ctx_set_neighbor_radius(self.h, float(r)))

    def fitness_batch(self, states: Sequence["_lib.PatchState"], state_index: Sequence[int], particles) -> np.ndarray:
        ns = len(states)
        arr = (_lib.PatchState * ns)(*states)
        idx = np.ascontiguousarray(state_index, dtype=np.int32)
        pts = np.ascontiguousarray(particles, dtype=np.float64).reshape(-1, 3)
        assert len(idx) == len(pts)
        out = np.empty(len(idx), dtype=np.float64)
        _lib.check(self.L.pais_fitness_batch(self.h, ns, arr, len(idx), idx.ctypes.data_as(C.POINTER(C.c_int32)),
                                             pts.ctypes.data_as(C.POINTER(C.c_double)),
                                             out.ctypes.data_as(C.POINTER(C.c_double))), "pais_fitness_batch")
        return out

    def refine_batch(self, cands: Sequence["_lib.Candidate"]):
        n = len(cands)
        arr = (_lib.Candidate * n)(*cands)
        out = (_lib.PatchResult * n)()
        _lib.check(self.L.pais_refine_batch(self.h, n, arr, out), "pais_refine_batch")
        return out

    def ncc_batch(self, states: Sequence["_lib.ViewState"], tables: bool = False) -> "NccBatch":
        """Patch::removeInvisibleCamera of each given state (pais_ncc_batch): which cameras see the patch and how well their
        warped patches agree, without refining it.  Raises RuntimeError on an invalid state (nothing is run then)."""
        n = len(states)
        arr = (_lib.ViewState * max(n, 1))(*states)
        out = (_lib.ViewResult * max(n, 1))()
        stride = max([int(s.num_cam) for s in states] + [2])
        tab = np.zeros((n, stride, stride), dtype=np.float64) if tables else None
        tp = tab.ctypes.data_as(C.POINTER(C.c_double)) if tables else None
        _lib.check(self.L.pais_ncc_batch(self.h, n, arr, out, tp, stride), "pais_ncc_batch")
        return NccBatch([int(s.num_cam) for s in states], out, tab)

    def load_state_batch(self, patches: Sequence["_lib.LoadedPatch"]):
        """The loader constructor Patch(center, normalS, camIdx, fitness, correlation) (patch.cpp:45-59) of each file record
        (pais_load_state_batch): the pais_patch_result array with reference camera, depth, ray, depth range, LOD, priority and
        image points, key = index.  Raises RuntimeError on an invalid record (nothing is run then)."""
        n = len(patches)
        arr = (_lib.LoadedPatch * max(n, 1))(*patches)
        out = (_lib.PatchResult * max(n, 1))()
        _lib.check(self.L.pais_load_state_batch(self.h, n, arr, out), "pais_load_state_batch")
        return out

    def load_stats(self, reset: bool = False):
        """(kernel ms, launches, patches) of the pais_load_state_batch calls since the last reset."""
        ms, launches, np_ = C.c_double(), C.c_int64(), C.c_int64()
        _lib.check(self.L.pais_get_load_stats(self.h, C.byref(ms), C.byref(launches), C.byref(np_), 1 if reset else 0))
        return ms.value, launches.value, np_.value

    def fitness_detail(self, states: Sequence["_lib.PatchState"], state_index: Sequence[int], particles, colours: bool = False,
                       homographies: bool = False) -> "CostDetail":
        """PAIS::getFitness of each particle (the inputs of fitness_batch) with its per-pixel breakdown (pais_fitness_detail), in
        the literal arithmetic whatever PAIS_ARITH says.  Maps are S x S in walk order ([e, xi, yi]); colours (n, K, S, S) and
        homographies (n, K, 9) have K = the largest num_cam of the states, rows beyond an evaluation's own num_cam are 0.
        Raises RuntimeError on an invalid state or index (nothing is run then)."""
        ns = len(states)
        arr = (_lib.PatchState * max(ns, 1))(*states)
        idx = np.ascontiguousarray(state_index, dtype=np.int32)
        pts = np.ascontiguousarray(particles, dtype=np.float64).reshape(-1, 3)
        assert len(idx) == len(pts)
        n, S = len(idx), int(self.cfg.patchSize)
        K = max([int(s.num_cam) for s in states] + [1])
        rec = (_lib.CostDetail * max(n, 1))()
        weight = np.zeros((n, S, S), dtype=np.float64)
        avg_sad = np.zeros((n, S, S), dtype=np.float64)
        code = np.zeros((n, S, S), dtype=np.int8)
        col = np.zeros((n, K, S, S), dtype=np.float64) if colours else None
        hom = np.zeros((n, K, 9), dtype=np.float64) if homographies else None
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None
        _lib.check(self.L.pais_fitness_detail(self.h, ns, arr, n, idx.ctypes.data_as(C.POINTER(C.c_int32)), dp(pts), rec, dp(weight),
                                              dp(avg_sad), code.ctypes.data_as(C.POINTER(C.c_int8)), dp(col), dp(hom), K),
                   "pais_fitness_detail")
        num_cam = [int(states[i].num_cam) for i in idx.tolist()]
        return CostDetail(rec, n, weight, avg_sad, code, col, hom, num_cam, int(self.cfg.patchRadius))

    def pso_trace(self, cands: Sequence["_lib.Candidate"], max_runs: int = 1, particles: bool = False) -> "PsoTrace":
        """refine() of each candidate exactly as refine_batch (the same records byte for byte, in this context's arithmetic), with
        every PSO run of its refine loop (at most max_runs recorded) and every iteration of each run (pais_pso_trace).  Raises
        RuntimeError on an invalid candidate or argument (nothing is run then)."""
        n = len(cands)
        arr = (_lib.Candidate * max(n, 1))(*cands)
        rows, npart = C.c_int(0), C.c_int(0)
        _lib.check(self.L.pais_pso_trace_shape(self.h, n, arr, C.byref(rows), C.byref(npart)), "pais_pso_trace_shape")
        R, N = rows.value, npart.value
        out = (_lib.PatchResult * max(n, 1))()
        run_info = np.zeros((n, max(int(max_runs), 1)), dtype=PSO_RUN_INFO_DTYPE)
        iters = np.zeros((n, max(int(max_runs), 1), R), dtype=PSO_ITER_DTYPE)
        parts = np.zeros((n, max(int(max_runs), 1), R, N, 11), dtype=np.float64) if particles else None
        pp = parts.ctypes.data_as(C.POINTER(C.c_double)) if parts is not None else None
        _lib.check(self.L.pais_pso_trace(self.h, n, arr, int(max_runs), out, run_info.ctypes.data_as(C.c_void_p),
                                         iters.ctypes.data_as(C.c_void_p), pp), "pais_pso_trace")
        return PsoTrace(out, n, run_info, iters, parts)

    def trace_stats(self, reset: bool = False):
        """(ms of the traced PSO iterations, k_pso_step_trace launches, evaluations) of the pais_pso_trace calls since the last reset."""
        ms, launches, ne = C.c_double(), C.c_int64(), C.c_int64()
        _lib.check(self.L.pais_get_trace_stats(self.h, C.byref(ms), C.byref(launches), C.byref(ne), 1 if reset else 0))
        return ms.value, launches.value, ne.value

    def detail_stats(self, reset: bool = False):
        """(kernel ms, launches, evaluations) of the pais_fitness_detail calls since the last reset."""
        ms, launches, ne = C.c_double(), C.c_int64(), C.c_int64()
        _lib.check(self.L.pais_get_detail_stats(self.h, C.byref(ms), C.byref(launches), C.byref(ne), 1 if reset else 0))
        return ms.value, launches.value, ne.value

    def ncc_stats(self, reset: bool = False):
        """(kernel ms, launches, states) of the pais_ncc_batch calls since the last reset."""
        ms, launches, nst = C.c_double(), C.c_int64(), C.c_int64()
        _lib.check(self.L.pais_get_ncc_stats(self.h, C.byref(ms), C.byref(launches), C.byref(nst), 1 if reset else 0))
        return ms.value, launches.value, nst.value

    def kernel_stats(self, reset: bool = False) -> "_lib.KernelStats":
        st = _lib.KernelStats()
        _lib.check(self.L.pais_get_kernel_stats(self.h, C.byref(st), 1 if reset else 0))
        return st


def make_candidate(center, normal, cam_idx, key: int, ptype: int, normalS=None) -> "_lib.Candidate":
    c = _lib.Candidate()
    c.center[:] = [float(v) for v in center]
    c.normal[:] = [float(v) for v in normal]
    ns = normalS if normalS is not None else normal_to_spherical(normal)
    c.normalS[:] = [float(ns[0]), float(ns[1])]
    c.key = int(key)
    c.type = int(ptype)
    c.num_cam = len(cam_idx)
    for i, v in enumerate(cam_idx):
        c.cam_idx[i] = int(v)
    return c


class NccBatch:
    """Result of Context.ncc_batch.  Per-state fields are numpy arrays; the per-camera ones are lists of arrays, each sliced to
    its state's own camera count (kept: to its num_kept; tables: K x K, or None when not asked for).  `records` is the raw
    pais_view_result array."""

    def __init__(self, num_cam, records, tables):
        n = len(num_cam)
        self.records = records
        self.correlation = np.array([records[i].correlation for i in range(n)], dtype=np.float64)
        self.dropped = np.array([records[i].dropped for i in range(n)], dtype=np.int32)
        self.max_idx = np.array([records[i].max_idx for i in range(n)], dtype=np.int32)
        self.num_kept = np.array([records[i].num_kept for i in range(n)], dtype=np.int32)
        self.region_ratio = [np.array(records[i].region_ratio[:k], dtype=np.float64) for i, k in enumerate(num_cam)]
        self.reason = [np.array(records[i].reason[:k], dtype=np.int32) for i, k in enumerate(num_cam)]
        self.kept = [np.array(records[i].kept_idx[:records[i].num_kept], dtype=np.int32) for i in range(n)]
        self.tables = [tables[i, :k, :k].copy() for i, k in enumerate(num_cam)] if tables is not None else None

    def __len__(self):
        return len(self.dropped)


class CostDetail:
    """Result of Context.fitness_detail.  Per evaluation: fitness, sum_weight, sum_weighted_sad, pt (n, 2), outcome, nx, ny,
    live_pixels, overflow_pixel, overflow_cam, ref_pos (numpy arrays of length n); weight, avg_sad, code: (n, S, S) maps in walk
    order, [e, xi, yi]; colour (n, K, S, S) and homographies (n, K, 9) or None.  `records` is the raw pais_cost_detail array."""

    def __init__(self, records, n, weight, avg_sad, code, colour, homographies, num_cam, radius):
        self.records = records
        for name in ("fitness", "sum_weight", "sum_weighted_sad"):
            setattr(self, name, np.array([getattr(records[i], name) for i in range(n)], dtype=np.float64))
        for name in ("outcome", "nx", "ny", "live_pixels", "overflow_pixel", "overflow_cam", "ref_pos"):
            setattr(self, name, np.array([getattr(records[i], name) for i in range(n)], dtype=np.int32))
        self.pt = np.array([records[i].pt[:] for i in range(n)], dtype=np.float64).reshape(n, 2)
        self.weight, self.avg_sad, self.code = weight, avg_sad, code
        self.colour, self.homographies = colour, homographies
        self.num_cam = list(num_cam)
        self.radius = radius

    def __len__(self):
        return len(self.fitness)

    def error_image(self, e: int) -> np.ndarray:
        """Patch::showError's map (patch.cpp:822-912) of evaluation e: avgSad min-max normalised over the COUNTED pixels, rows = y
        (error.at(ey, ex)); the other pixels are NaN."""
        sad = self.avg_sad[e].T
        counted = self.code[e].T == _lib.PIX_COUNTED
        out = np.full(sad.shape, np.nan)
        if counted.any():
            lo, hi = float(sad[counted].min()), float(sad[counted].max())
            out[counted] = (sad[counted] - lo) / (hi - lo) if hi > lo else 0.0
        return out

    def window_corners(self, e: int) -> np.ndarray:
        """The five points Patch::showRefinedResult draws (patch.cpp:785-801) in every camera of evaluation e: the corners
        (-r, -r), (-r, +r), (+r, -r), (+r, +r) and the centre of the window around pt, through H_i, each rounded with cvRound.
        (num_cam, 5, 2) integer array; needs homographies=True."""
        if self.homographies is None:
            raise ValueError("window_corners needs fitness_detail(..., homographies=True)")
        r = self.radius
        px, py = self.pt[e]
        x = np.array([px - r, px - r, px + r, px + r, px])
        y = np.array([py - r, py + r, py - r, py + r, py])
        out = np.empty((self.num_cam[e], 5, 2), dtype=np.int64)
        for i in range(self.num_cam[e]):
            H = self.homographies[e, i]
            with np.errstate(divide="ignore", invalid="ignore"):
                w = H[6] * x + H[7] * y + H[8]
                ix = (H[0] * x + H[1] * y + H[2]) / w
                iy = (H[3] * x + H[4] * y + H[5]) / w
            out[i, :, 0] = np.rint(ix)       # cvRound: round half to even
            out[i, :, 1] = np.rint(iy)
        return out


def _dtype_of(struct) -> np.dtype:
    """numpy structured dtype of a ctypes structure of scalars and scalar arrays (the same layout: asserted by size)."""
    fields = [(name, (np.dtype(ct._type_), (ct._length_,)) if hasattr(ct, "_length_") else np.dtype(ct)) for name, ct in struct._fields_]
    dt = np.dtype(fields)
    assert dt.itemsize == C.sizeof(struct), (dt.itemsize, C.sizeof(struct))
    return dt


PSO_RUN_INFO_DTYPE = _dtype_of(_lib.PsoRunInfo)
PSO_ITER_DTYPE = _dtype_of(_lib.PsoIter)


class PsoTrace:
    """Result of Context.pso_trace.  records: the pais_patch_result array (refine_batch's records); run_info (n, max_runs) and
    iters (n, max_runs, rows) numpy structured arrays with the fields of pais_pso_run_info / pais_pso_iter; particles: None or
    (n, max_runs, rows, N, 11) -- pos[3] vec[3] pBest[3] fitness pBestFitness per particle.  Unused slots are zero."""

    def __init__(self, records, n, run_info, iters, particles):
        self.records = records
        self.n = n
        self.run_info, self.iters, self.particles = run_info, iters, particles
        self.max_runs = run_info.shape[1]

    def __len__(self):
        return self.n

    def total_runs(self, c: int) -> int:
        """PSO runs of candidate c's refine loop (recorded or not)."""
        return int(self.records[c].pso_runs)

    def runs(self, c: int) -> int:
        """Recorded runs of candidate c: min(pso_runs, max_runs)."""
        return min(self.total_runs(c), self.max_runs)

    def rows(self, c: int, r: int) -> int:
        """Rows of run r of candidate c: iterations + 1."""
        return int(self.run_info[c, r]["iterations"]) + 1

    def swarm(self, c: int, r: int, t: int) -> dict:
        """Row t of run r of candidate c: pos, vec, pbest (N, 3), fit, pbest_fit (N,) of the run's N particles; needs
        pso_trace(..., particles=True)."""
        if self.particles is None:
            raise ValueError("swarm needs pso_trace(..., particles=True)")
        N = int(self.run_info[c, r]["n_particles"])
        q = self.particles[c, r, t, :N]
        return {"pos": q[:, 0:3], "vec": q[:, 3:6], "pbest": q[:, 6:9], "fit": q[:, 9], "pbest_fit": q[:, 10]}

    def improved(self, c: int, r: int, t: int) -> np.ndarray:
        """Indices of the particles whose pBest updateFitness replaced on row t >= 1 (fitness < the previous row's pBestFitness,
        psosolver.cpp:128)."""
        cur, prev = self.swarm(c, r, t), self.swarm(c, r, t - 1)
        return np.nonzero(cur["fit"] < prev["pbest_fit"])[0]

    def first_branch(self, other: "PsoTrace") -> list:
        """Per candidate, the first (run, row) where this trace's discrete trajectory and other's differ, or None.  They differ
        on a row where g_idx differs; or, when both traces carry particles, where the set of particles whose pBest was replaced
        differs; at run r's row 0 where the run's reference camera, LOD or camera set differ; at row min(rows) - 1 of a run
        whose row counts differ (one run stopped after that row, the other went on); at (min(runs), 0) when the numbers of runs
        differ.  The fitness bits play no part: a default and a literal trace differ in them from row 0 on."""
        assert len(self) == len(other)
        both = self.particles is not None and other.particles is not None
        out = []
        for c in range(self.n):
            out.append(_first_branch_of(self, other, c, both))
        return out


def _first_branch_of(a: "PsoTrace", b: "PsoTrace", c: int, both: bool):
    nr = min(a.runs(c), b.runs(c))
    for r in range(nr):
        ia, ib = a.run_info[c, r], b.run_info[c, r]
        k = int(ia["num_cam"])
        if (int(ia["ref_cam"]), int(ia["lod"]), k) != (int(ib["ref_cam"]), int(ib["lod"]), int(ib["num_cam"])) or \
                list(ia["cam_idx"][:k]) != list(ib["cam_idx"][:k]):
            return (r, 0)
        ra, rb = a.rows(c, r), b.rows(c, r)
        for t in range(min(ra, rb)):
            if int(a.iters[c, r, t]["g_idx"]) != int(b.iters[c, r, t]["g_idx"]):
                return (r, t)
            if both and t >= 1 and not np.array_equal(a.improved(c, r, t), b.improved(c, r, t)):
                return (r, t)
        if ra != rb:
            return (r, min(ra, rb) - 1)
    if a.total_runs(c) != b.total_runs(c):
        return (min(a.total_runs(c), b.total_runs(c)), 0)
    return None


def patch_state_from_record(rec) -> "_lib.PatchState":
    """The pais_patch_state of a pais_patch_result (ray, reference camera, LOD and camera set of the record): with
    particle_from_record, the inputs that re-evaluate a record's final patch through fitness_batch / fitness_detail.  A record's
    own `fitness` belongs to the state of its last PSO run, which refine() may have changed afterwards (removeInvisibleCamera,
    a new reference camera or LOD), so it need not equal the cost of this state."""
    s = _lib.PatchState()
    s.ray[:] = [float(x) for x in rec.ray[:]]
    s.ref_cam = int(rec.ref_cam)
    s.lod = int(rec.lod)
    s.num_cam = int(rec.num_cam)
    for i in range(rec.num_cam):
        s.cam_idx[i] = int(rec.cam_idx[i])
    return s


def particle_from_record(rec) -> List[float]:
    """The particle (normalS[0], normalS[1], depth) of a pais_patch_result."""
    return [float(rec.normalS[0]), float(rec.normalS[1]), float(rec.depth)]


def view_state_from_record(rec) -> "_lib.ViewState":
    """The pais_view_state of a pais_patch_result (centre, normal, reference camera, LOD and camera set of the record)."""
    v = _lib.ViewState()
    v.center[:] = [float(x) for x in rec.center[:]]
    v.normal[:] = [float(x) for x in rec.normal[:]]
    v.ref_cam = int(rec.ref_cam)
    v.lod = int(rec.lod)
    v.num_cam = int(rec.num_cam)
    for i in range(rec.num_cam):
        v.cam_idx[i] = int(rec.cam_idx[i])
    return v


def make_loaded_patch(center, normalS, cam_idx, fitness: float, correlation: float) -> "_lib.LoadedPatch":
    """A pais_loaded_patch from the fields of a patch record of an MVS file (io.IoPatch has the same ones)."""
    p = _lib.LoadedPatch()
    p.center[:] = [float(x) for x in center]
    p.normalS[:] = [float(normalS[0]), float(normalS[1])]
    p.fitness = float(fitness)
    p.correlation = float(correlation)
    p.num_cam = len(cam_idx)
    for i, c in enumerate(cam_idx):
        p.cam_idx[i] = int(c)
    return p


def make_view_state(center, normal, ref_cam: int, lod: int, cam_idx) -> "_lib.ViewState":
    v = _lib.ViewState()
    v.center[:] = [float(x) for x in center]
    v.normal[:] = [float(x) for x in normal]
    v.ref_cam = int(ref_cam)
    v.lod = int(lod)
    v.num_cam = len(cam_idx)
    for i, c in enumerate(cam_idx):
        v.cam_idx[i] = int(c)
    return v
