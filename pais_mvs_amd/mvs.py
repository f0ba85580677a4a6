"""Host mirror of PAIS::MVS for the hot path: refineSeedPatches / expansionPatches
(TMVS/mvs/mvs.h:229,231) over include/pais_mvs.h."""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence

import numpy as np

from . import _lib
from .camera import Camera
from .config import MvsConfig
from .context import camera_desc


class MvsStats(C.Structure):
    _fields_ = [("seeds_refined", C.c_int64), ("candidates_refined", C.c_int64), ("candidates_effective", C.c_int64),
                ("patches_inserted", C.c_int64), ("patches_deleted", C.c_int64), ("rounds", C.c_int64),
                ("parents_popped", C.c_int64), ("pso_evals_effective", C.c_int64),
                ("host_enumerate_ms", C.c_double), ("host_commit_ms", C.c_double), ("gpu_refine_ms", C.c_double),
                ("batches_sharded", C.c_int64), ("batches_replicated", C.c_int64), ("exchange_ms", C.c_double),
                ("exchange_bytes", C.c_int64), ("rounds_streamed", C.c_int64), ("emu_replay_ms", C.c_double),
                ("exchange_retries", C.c_int64), ("rounds_enum_sharded", C.c_int64)]


class RoundLog(C.Structure):
    _fields_ = [("n", C.c_int32), ("has_seeds", C.c_int32), ("sharded", C.c_int32), ("max_num_cam", C.c_int32),
                ("refine_ms", C.c_double), ("enumerate_ms", C.c_double), ("commit_ms", C.c_double)]


UNIQUE_ID_BYTES = 128


class UniqueId(C.Structure):
    _fields_ = [("bytes", C.c_char * UNIQUE_ID_BYTES)]


# int fn(void *user, const void *send, void *recv, size_t bytes_per_rank)
ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t)
# int fn(void *user, int n, const pais_candidate *cands, pais_patch_result *out, int has_seeds)
# int fn(void *user, pais_mvs *m, int num_patches)
CHECKPOINT_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int)
RECORD_SOURCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(_lib.Candidate), C.POINTER(_lib.PatchResult), C.c_int)


def _bind(L):
    if getattr(L, "_mvs_bound", False):
        return
    vp = C.c_void_p
    L.pais_mvs_create.argtypes = [C.POINTER(_lib.Config), C.c_int, C.POINTER(_lib.CameraDesc), C.c_int, C.c_uint64,
                                  C.POINTER(vp)]
    L.pais_mvs_destroy.argtypes = [vp]
    L.pais_mvs_destroy.restype = None
    L.pais_mvs_ctx.restype = vp
    L.pais_mvs_ctx.argtypes = [vp]
    L.pais_mvs_reset.argtypes = [vp]
    L.pais_mvs_add_seed.argtypes = [vp, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int32)]
    L.pais_mvs_refine_seed_patches.argtypes = [vp]
    L.pais_mvs_expansion_patches.argtypes = [vp, C.c_int, C.c_int]
    L.pais_mvs_set_thin_front.argtypes = [vp, C.c_int]
    L.pais_mvs_add_seed_measured.argtypes = [vp, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_int]
    L.pais_mvs_load_patch.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int32), C.c_double, C.c_double]
    L.pais_mvs_load_patches.argtypes = [vp, C.c_int, C.POINTER(_lib.LoadedPatch), C.POINTER(C.c_int)]
    L.pais_mvs_set_checkpoint.argtypes = [vp, C.c_int, CHECKPOINT_FN, vp]
    L.pais_mvs_cell_filtering.argtypes = [vp]
    L.pais_mvs_visibility_filtering.argtypes = [vp]
    L.pais_mvs_neighbor_cell_filtering.argtypes = [vp, C.c_double]
    L.pais_mvs_neighbor_patch_filtering.argtypes = [vp, C.c_double, C.POINTER(C.c_double)]
    L.pais_mvs_statistical_filtering.argtypes = [vp, C.c_int, C.c_double, C.POINTER(C.c_int), C.POINTER(C.c_double)]
    L.pais_mvs_normal_filtering.argtypes = [vp, C.c_int, C.c_double, C.POINTER(C.c_int), C.POINTER(C.c_double)]
    L.pais_mvs_depth_filtering.argtypes = [vp, C.c_double, C.c_double, C.POINTER(C.c_int), C.POINTER(C.c_double)]
    L.pais_mvs_seed_begin.argtypes = [vp, C.POINTER(C.POINTER(_lib.Candidate)), C.POINTER(C.c_int)]
    L.pais_mvs_seed_commit.argtypes = [vp, C.POINTER(_lib.PatchResult), C.c_int]
    L.pais_mvs_expansion_begin.argtypes = [vp]
    L.pais_mvs_round_begin.argtypes = [vp, C.c_int, C.POINTER(C.POINTER(_lib.Candidate)), C.POINTER(C.c_int)]
    L.pais_mvs_round_commit.argtypes = [vp, C.POINTER(_lib.PatchResult), C.c_int]
    L.pais_mvs_expansion_end.argtypes = [vp]
    L.pais_mvs_num_patches.argtypes = [vp]
    L.pais_mvs_num_slots.argtypes = [vp]
    L.pais_mvs_get_patch.argtypes = [vp, C.c_int, C.POINTER(_lib.PatchResult), C.POINTER(C.c_int)]
    L.pais_mvs_neighbor_radius.restype = C.c_double
    L.pais_mvs_neighbor_radius.argtypes = [vp]
    L.pais_mvs_get_stats.argtypes = [vp, C.POINTER(MvsStats)]
    L.pais_mvs_get_round_log.argtypes = [vp, C.POINTER(RoundLog), C.c_int]
    L.pais_mvs_last_error.restype = C.c_char_p
    L.pais_comm_get_unique_id.argtypes = [C.POINTER(UniqueId)]
    L.pais_mvs_comm_init_rccl.argtypes = [vp, C.c_int, C.c_int, C.POINTER(UniqueId)]
    L.pais_mvs_create_ranked.argtypes = [C.POINTER(_lib.Config), C.c_int, C.POINTER(_lib.CameraDesc), C.c_int, C.c_uint64,
                                         C.c_int, C.c_int, C.POINTER(UniqueId), C.POINTER(vp)]
    L.pais_mvs_comm_init_callback.argtypes = [vp, C.c_int, C.c_int, ALLGATHER_FN, vp]
    L.pais_mvs_set_replicate_below.argtypes = [vp, C.c_int]
    L.pais_mvs_set_record_source.argtypes = [vp, RECORD_SOURCE_FN, vp]
    L.pais_mvs_emulate.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    L.pais_mvs_test_inject.argtypes = [vp, C.c_int, C.c_int]
    L._mvs_bound = True


def patches_sha1(rows) -> str:
    """rows: (center[3], normalS[2], camIdx list, fitness, correlation) per patch in id order -> hex SHA-1 of the bytes
    FileWriter::writeMVS stores for them (io/filewriter.cpp:97-99)."""
    import hashlib
    import struct
    h = hashlib.sha1()
    for cen, ns, cams, fit, corr in rows:
        k = len(cams)
        h.update(struct.pack("<5di%di2d" % k, *cen, *ns, k, *cams, fit, corr))
    return h.hexdigest()


def get_unique_id() -> bytes:
    """ncclGetUniqueId through the C ABI: call on ONE rank and hand the 128 bytes to the others."""
    L = _lib.load()
    _bind(L)
    u = UniqueId()
    if L.pais_comm_get_unique_id(C.byref(u)) != 0:
        raise RuntimeError("pais_comm_get_unique_id failed: %s" % L.pais_mvs_last_error().decode())
    return bytes(bytearray(u))


class CheckpointAbort(RuntimeError):
    """expansionPatches was stopped by the checkpoint callback; `code` is what the callback returned."""

    def __init__(self, code: int):
        super().__init__("expansion aborted by the checkpoint callback (%d)" % code)
        self.code = code


class MVS:
    """Reconstruction driver.  device < 0: scheduler only (stepwise API)."""

    def __init__(self, cfg: MvsConfig, cameras: Sequence[Camera], device: int = 0, seed: int = 42):
        self.L = _lib.load()
        _bind(self.L)
        self.cfg = cfg
        self.cameras = list(cameras)
        self.device = device
        keep: list = []
        n = len(self.cameras)
        descs = (_lib.CameraDesc * n)()
        for i, cam in enumerate(self.cameras):
            descs[i] = camera_desc(cam, bool(cfg.adaptiveGradientEnable), keep)
        c = cfg.to_c()
        h = C.c_void_p()
        self._check(self.L.pais_mvs_create(C.byref(c), n, descs, device, seed, C.byref(h)), "pais_mvs_create")
        self.h = h

    def _check(self, rc, what):
        if rc < 0:
            msg = self.L.pais_mvs_last_error().decode() or self.L.pais_last_error().decode()
            raise RuntimeError("%s failed (%d): %s" % (what, rc, msg))
        return rc

    def close(self):
        if getattr(self, "h", None):
            self.L.pais_mvs_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def ctx_handle(self):
        return self.L.pais_mvs_ctx(self.h)

    def reset(self):
        self._check(self.L.pais_mvs_reset(self.h), "pais_mvs_reset")

    def add_seed(self, center, cam_idx) -> int:
        cen = (C.c_double * 3)(*[float(v) for v in center])
        idx = (C.c_int32 * len(cam_idx))(*[int(v) for v in cam_idx])
        return self._check(self.L.pais_mvs_add_seed(self.h, cen, len(cam_idx), idx), "pais_mvs_add_seed")

    def add_seed_measured(self, center, cam_idx, img_points, recenter: bool = True) -> int:
        """NVM seed with its image measurements (pixels); recenter: MVS::reCentering first, as loadNVM does."""
        cen = (C.c_double * 3)(*[float(v) for v in center])
        idx = (C.c_int32 * len(cam_idx))(*[int(v) for v in cam_idx])
        flat = [float(v) for p in img_points for v in p]
        pts = (C.c_double * len(flat))(*flat)
        return self._check(self.L.pais_mvs_add_seed_measured(self.h, cen, len(cam_idx), idx, pts, 1 if recenter else 0),
                           "pais_mvs_add_seed_measured")

    def seed_from_images(self, max_dist: float = 3.0, params=None) -> int:
        """FeatureManager::setSeedPatches(cameras, max_dist, mvs) whole: features of every camera's level-0 image on the GPU
        (include/pais_feature.h), matching, epipolar filter, n-view union, one seed per feature; returns the seeds added."""
        from . import features
        L = features._bind(self.L)
        n = C.c_int(0)
        self._check(L.pais_mvs_seed_from_images(self.h, float(max_dist), None if params is None else C.byref(params), C.byref(n)),
                    "pais_mvs_seed_from_images")
        return n.value

    # ---- MVS::refineSeedPatches / MVS::expansionPatches
    def refineSeedPatches(self):
        self._check(self.L.pais_mvs_refine_seed_patches(self.h), "pais_mvs_refine_seed_patches")

    # ---- FileLoader::loadMvsPatch + the `-f` filter verbs (TMVS.cpp:124-172)
    def load_patch(self, center, normalS, cam_idx, fitness, correlation) -> int:
        cen = (C.c_double * 3)(*[float(v) for v in center])
        ns = (C.c_double * 2)(*[float(v) for v in normalS])
        idx = (C.c_int32 * len(cam_idx))(*[int(v) for v in cam_idx])
        return self._check(self.L.pais_mvs_load_patch(self.h, cen, ns, len(cam_idx), idx, float(fitness), float(correlation)), "pais_mvs_load_patch")

    # ---- `-r file.mvs` (TMVS.cpp:87-88): FileLoader::loadMVS's patch loop, then refineSeedPatches / expansionPatches as usual
    def load_patches(self, patches) -> int:
        """patches: records with center, normalS, num_cam, cam_idx, fitness, correlation (io.IoPatch as io.load_mvs returns them,
        or _lib.LoadedPatch).  The loader constructor of all of them in one GPU call; stored as unexpanded seeds under
        consecutive ids.  Returns the first id."""
        n = len(patches)
        arr = (_lib.LoadedPatch * max(n, 1))()
        for i, p in enumerate(patches):
            a = arr[i]
            a.center[:] = p.center[:]
            a.normalS[:] = p.normalS[:]
            a.fitness, a.correlation, a.num_cam = p.fitness, p.correlation, p.num_cam
            k = min(max(int(p.num_cam), 0), _lib.MAX_VIS)
            a.cam_idx[:k] = p.cam_idx[:k]
        first = C.c_int(0)
        self._check(self.L.pais_mvs_load_patches(self.h, n, arr, C.byref(first)), "pais_mvs_load_patches")
        return first.value

    def set_checkpoint(self, every: int, fn):
        """The reference's auto_save.mvs rule (mvs.cpp:265-268) per round: after a committed round of expansionPatches,
        fn(num_patches) is called if num_patches // every exceeds the calls made so far; a non-zero return stops the expansion
        (expansionPatches raises CheckpointAbort with that code).  fn may read this driver, not change it.  every <= 0 or
        fn None: off."""
        if fn is None or every <= 0:
            self._checkpoint_cb = CHECKPOINT_FN(0)
            self._check(self.L.pais_mvs_set_checkpoint(self.h, 0, self._checkpoint_cb, None), "pais_mvs_set_checkpoint")
            return

        def cb(_user, _m, num_patches):
            try:
                return int(fn(num_patches) or 0)
            except Exception:   # the C side reports the abort
                import traceback
                traceback.print_exc()
                return -3
        self._checkpoint_cb = CHECKPOINT_FN(cb)      # keep the trampoline alive
        self._check(self.L.pais_mvs_set_checkpoint(self.h, int(every), self._checkpoint_cb, None), "pais_mvs_set_checkpoint")

    def cellFiltering(self):
        self._check(self.L.pais_mvs_cell_filtering(self.h), "pais_mvs_cell_filtering")

    def visibilityFiltering(self):
        self._check(self.L.pais_mvs_visibility_filtering(self.h), "pais_mvs_visibility_filtering")

    def neighborCellFiltering(self, neighbor_ratio: float = 0.25):
        self._check(self.L.pais_mvs_neighbor_cell_filtering(self.h, float(neighbor_ratio)), "pais_mvs_neighbor_cell_filtering")

    def neighborPatchFiltering(self, neighbor_ratio: float = 0.25) -> float:
        """GPU all-pairs neighbour counts; returns the kernel's milliseconds."""
        ms = C.c_double(0)
        self._check(self.L.pais_mvs_neighbor_patch_filtering(self.h, float(neighbor_ratio), C.byref(ms)), "pais_mvs_neighbor_patch_filtering")
        return ms.value

    def statisticalFiltering(self, k: int = 8, sigma: float = 2.0):
        """Statistical outlier filter (pais_mvs_statistical_filtering): deletes the patches whose mean distance to their k
        nearest alive patches exceeds mu + sigma sd of that mean over the cloud; GPU k-nearest search, no host path.
        -> (patches removed, the search kernels' milliseconds)."""
        ms, removed = C.c_double(0), C.c_int(0)
        self._check(self.L.pais_mvs_statistical_filtering(self.h, int(k), float(sigma), C.byref(removed), C.byref(ms)),
                    "pais_mvs_statistical_filtering")
        return removed.value, ms.value

    def normalFiltering(self, k: int = 16, max_angle_deg: float = 30.0):
        """Normal-agreement filter (pais_mvs_normal_filtering): deletes the patches whose normal lies more than max_angle_deg
        from the normal of the plane through their k nearest alive patches and themselves, either way round (the rule takes
        |cos|); GPU search and fit, no host path.  -> (patches removed, the kernels' milliseconds)."""
        import math
        ms, removed = C.c_double(0), C.c_int(0)
        self._check(self.L.pais_mvs_normal_filtering(self.h, int(k), math.cos(math.radians(float(max_angle_deg))), C.byref(removed), C.byref(ms)),
                    "pais_mvs_normal_filtering")
        return removed.value, ms.value

    def depthFiltering(self, rho: Optional[float] = None, tol: Optional[float] = None):
        """Depth-consistency filter (pais_mvs_depth_filtering): the live patches as discs of radius rho (default
        neighbor_radius()) into every camera of the scene, each centre depth-tested against those maps with tolerance tol
        (default rho); a patch that fewer than minCamNum of its own cameras see unoccluded goes.  All decisions come from one
        render: they are simultaneous.  GPU render and test, no host path.  -> (patches removed, the kernels' milliseconds)."""
        ms, removed = C.c_double(0), C.c_int(0)
        self._check(self.L.pais_mvs_depth_filtering(self.h, -1.0 if rho is None else float(rho), -1.0 if tol is None else float(tol),
                                                    C.byref(removed), C.byref(ms)), "pais_mvs_depth_filtering")
        return removed.value, ms.value

    # ---- multi-GPU (include/pais_mvs.h): one process per GPU, sharded refinement, one all-gather per batch
    def comm_init_rccl(self, rank: int, world: int, unique_id: bytes):
        u = UniqueId.from_buffer_copy(unique_id)
        self._check(self.L.pais_mvs_comm_init_rccl(self.h, rank, world, C.byref(u)), "pais_mvs_comm_init_rccl")

    def comm_init_callback(self, rank: int, world: int, all_gather):
        """all_gather(send: bytes-like view, bytes_per_rank) -> bytes of world * bytes_per_rank (rank order); host memory."""
        def cb(_user, send, recv, nbytes):
            try:
                out = all_gather((C.c_char * nbytes).from_address(send), nbytes)
                C.memmove(recv, bytes(out), nbytes * world)
                return 0
            except Exception:   # the C side reports the failure
                import traceback
                traceback.print_exc()
                return 1
        self._gather_cb = ALLGATHER_FN(cb)       # keep the trampoline alive
        self._check(self.L.pais_mvs_comm_init_callback(self.h, rank, world, self._gather_cb, None), "pais_mvs_comm_init_callback")

    def emulate(self, mode: int, rank: int = 0, world: int = 1):
        """include/pais_mvs.h pais_mvs_emulate: 1 record a single-rank run, 2 be rank `rank` of `world` on this one GPU, 0 off."""
        self._check(self.L.pais_mvs_emulate(self.h, int(mode), int(rank), int(world)), "pais_mvs_emulate")

    def set_replicate_below(self, per_rank: int):
        self._check(self.L.pais_mvs_set_replicate_below(self.h, int(per_rank)), "pais_mvs_set_replicate_below")

    def test_inject(self, what: int, count: int):
        """include/pais_test_hooks.h pais_mvs_test_inject: 1 ring-retry status, 2 failing buffer growth, 3 failing refinement."""
        self._check(self.L.pais_mvs_test_inject(self.h, int(what), int(count)), "pais_mvs_test_inject")

    def set_record_source(self, fn):
        """GPU-less drivers (device < 0) only: fn(n, cands_ptr, out_ptr, has_seeds) fills out[0:n]."""
        def cb(_user, n, cands, out, has_seeds):
            try:
                fn(n, cands, out, bool(has_seeds))
                return 0
            except Exception:
                import traceback
                traceback.print_exc()
                return 1
        self._record_cb = RECORD_SOURCE_FN(cb)
        self._check(self.L.pais_mvs_set_record_source(self.h, self._record_cb, None), "pais_mvs_set_record_source")

    def set_thin_front(self, thin_front: int):
        """Rounds with <= thin_front active parents take all remaining camera slots of each parent (0 = never)."""
        self._check(self.L.pais_mvs_set_thin_front(self.h, int(thin_front)), "pais_mvs_set_thin_front")

    def expansionPatches(self, parents_per_round: int = 1, max_rounds: int = 0):
        rc = self._check(self.L.pais_mvs_expansion_patches(self.h, parents_per_round, max_rounds), "pais_mvs_expansion_patches")
        if rc > 0:
            raise CheckpointAbort(rc)

    # ---- stepwise
    def seed_begin(self):
        p = C.POINTER(_lib.Candidate)()
        n = C.c_int(0)
        self._check(self.L.pais_mvs_seed_begin(self.h, C.byref(p), C.byref(n)), "pais_mvs_seed_begin")
        return p, n.value

    def seed_commit(self, results, n: int):
        self._check(self.L.pais_mvs_seed_commit(self.h, results, n), "pais_mvs_seed_commit")

    def expansion_begin(self):
        self._check(self.L.pais_mvs_expansion_begin(self.h), "pais_mvs_expansion_begin")

    def round_begin(self, parents_per_round: int):
        p = C.POINTER(_lib.Candidate)()
        n = C.c_int(0)
        rc = self._check(self.L.pais_mvs_round_begin(self.h, parents_per_round, C.byref(p), C.byref(n)), "pais_mvs_round_begin")
        return rc == 1, p, n.value

    def round_commit(self, results, n: int):
        self._check(self.L.pais_mvs_round_commit(self.h, results, n), "pais_mvs_round_commit")

    def expansion_end(self):
        self._check(self.L.pais_mvs_expansion_end(self.h), "pais_mvs_expansion_end")

    # ---- inspection
    def num_patches(self) -> int:
        return self.L.pais_mvs_num_patches(self.h)

    def num_slots(self) -> int:
        return self.L.pais_mvs_num_slots(self.h)

    def get_patch(self, i: int) -> Optional["_lib.PatchResult"]:
        r = _lib.PatchResult()
        e = C.c_int(0)
        if self.L.pais_mvs_get_patch(self.h, i, C.byref(r), C.byref(e)) != 0:
            return None
        return r

    def patches(self) -> List["_lib.PatchResult"]:
        out = []
        for i in range(self.num_slots()):
            p = self.get_patch(i)
            if p is not None:
                out.append(p)
        return out

    def neighbor_radius(self) -> float:
        return self.L.pais_mvs_neighbor_radius(self.h)

    def stats(self) -> MvsStats:
        s = MvsStats()
        self.L.pais_mvs_get_stats(self.h, C.byref(s))
        return s

    def round_log(self):
        """One RoundLog per GPU batch of the last reconstruction (seed batch first)."""
        n = self.L.pais_mvs_get_round_log(self.h, None, 0)
        buf = (RoundLog * max(n, 1))()
        n = self.L.pais_mvs_get_round_log(self.h, buf, n)
        return [buf[i] for i in range(n)]

    def cloud(self) -> np.ndarray:
        """(N, 6) array of patch centres and normals in id order."""
        ps = self.patches()
        return np.array([[*p.center[:], *p.normal[:]] for p in ps], dtype=np.float64).reshape(-1, 6)

    def score(self, truth, threshold: float, fraction: float = 0.9) -> dict:
        """Accuracy and completeness of cloud() against a ground truth of (m, 6) points and normals (pais_mvs_amd.evaluate.score),
        searched on this driver's GPU; a scheduler-only driver (device < 0) is refused."""
        from . import evaluate
        return evaluate.score(self.cloud(), truth, threshold, fraction, self.device)

    def spacing(self) -> float:
        """The sample spacing of the live patches (pais_mvs_amd.evaluate.spacing): the median distance from a centre to the
        nearest other one, searched on this driver's GPU; a disc radius for render(), a threshold for score()."""
        from . import evaluate
        return evaluate.spacing(self.cloud()[:, :3], self.device)

    def planes(self, k: int = 16) -> dict:
        """pais_mvs_amd.evaluate.planes of the live centres against themselves (each centre takes part in its own fit; rows index
        patches() / cloud()), on this driver's GPU."""
        from . import evaluate
        return evaluate.planes(self.cloud()[:, :3], k, device=self.device)

    def roughness(self, k: int = 16) -> float:
        """The noise of the live centres across their own surface (pais_mvs_amd.evaluate.roughness), on this driver's GPU."""
        from . import evaluate
        return evaluate.roughness(self.cloud()[:, :3], k, self.device)

    def mesh(self, h=None, k: int = 8, support=None, trunc=None):
        """The surface of cloud() as a triangle mesh (pais_mvs_amd.mesh.mesh: distance field and marching tetrahedra), on this
        driver's GPU; a scheduler-only driver (device < 0) is refused.  h: the grid pitch, default twice spacing()."""
        from . import mesh as msh
        return msh.mesh(self.cloud(), h, k, support, trunc, self.device)

    def camera_images_bgr(self) -> list:
        """per camera its (H,W,3) uint8 BGR image (the grey image three times where the camera holds no colour)"""
        out = []
        for cam in self.cameras:
            if cam.rgb is not None and cam.rgb.ndim == 3 and cam.rgb.shape[-1] == 3:
                out.append(np.ascontiguousarray(cam.rgb[:, :, ::-1]))
            else:
                out.append(np.repeat(np.asarray(cam.image, np.uint8)[:, :, None], 3, axis=2))
        return out

    def render_mesh(self, mesh=None, views=None, width: Optional[int] = None, height: Optional[int] = None, cull: bool = True, h=None):
        """pais_mvs_amd.render.render_mesh of `mesh` (default: mesh(h) of the live patches) into `views`: pais_view records, or
        indices of this driver's cameras (default all) -- those must share one size, which is the default width x height."""
        from . import render as rnd
        if mesh is None:
            mesh = self.mesh(h)
        views = list(range(len(self.cameras))) if views is None else list(views)
        cams = [self.cameras[int(v)] for v in views if isinstance(v, (int, np.integer))]
        vs = [rnd.view_of(self.cameras[int(v)]) if isinstance(v, (int, np.integer)) else v for v in views]
        sizes = {(c.width, c.height) for c in cams}
        if len(sizes) > 1:
            raise ValueError("MVS.render_mesh: cameras of different sizes go in separate calls")
        if sizes and width is None and height is None:
            width, height = next(iter(sizes))
        if width is None or height is None:
            raise ValueError("MVS.render_mesh: width and height are needed for views that are not cameras of the scene")
        return rnd.render_mesh(mesh.vertices, mesh.triangles, vs, width, height, cull, self.device)

    # ---- the viewer's part (`-v`, view/mvsviewer.cpp): the live patches rendered on this driver's GPU
    def render(self, views, width: Optional[int] = None, height: Optional[int] = None, mode: str = "disc", radius: Optional[float] = None,
               cull_back: bool = True):
        """pais_mvs_amd.render.render of the live patches (ids index patches() / cloud()) into `views`: pais_view records, or
        indices of this driver's cameras -- those must share one size, which is the default width x height.  The default
        radius is neighbor_radius(), in point mode 1 pixel."""
        from . import render as rnd
        views = list(views)
        cams = [self.cameras[int(v)] for v in views if isinstance(v, (int, np.integer))]
        vs = [rnd.view_of(self.cameras[int(v)]) if isinstance(v, (int, np.integer)) else v for v in views]
        sizes = {(c.width, c.height) for c in cams}
        if len(sizes) > 1:
            raise ValueError("MVS.render: cameras of different sizes go in separate calls")
        if sizes and width is None and height is None:
            width, height = next(iter(sizes))
        if width is None or height is None:
            raise ValueError("MVS.render: width and height are needed for views that are not cameras of the scene")
        if radius is None:
            radius = self.neighbor_radius() if mode == "disc" else 1.0
        c = self.cloud()
        return rnd.render(c[:, :3], c[:, 3:], vs, width, height, mode=mode, radius=radius, cull_back=cull_back, device=self.device)

    def depth_maps(self, mode: str = "disc", radius: Optional[float] = None):
        """One single-view Render per camera of the scene, each at its camera's size (cameras of one size share a call)."""
        from . import render as rnd
        by_size = {}
        for i, cam in enumerate(self.cameras):
            by_size.setdefault((cam.width, cam.height), []).append(i)
        out = [None] * len(self.cameras)
        for (w, h), idx in by_size.items():
            r = self.render(idx, w, h, mode=mode, radius=radius)
            for k, i in enumerate(idx):
                out[i] = rnd.Render(r.depth[k:k + 1], r.id[k:k + 1], r.kernel_ms, r.views[k:k + 1], r.counts)
        return out

    def visibility(self, views=None, radius: Optional[float] = None, tol: Optional[float] = None, self_index: bool = True,
                   keep_maps: bool = False):
        """pais_mvs_amd.render.visibility of the live patches against themselves (rows of .code index `views`, columns index
        patches() / cloud()) as discs of `radius` (default neighbor_radius()), tol defaulting to the radius.  views: indices of
        this driver's cameras (default all), which must share one size."""
        from . import render as rnd
        idx = list(range(len(self.cameras))) if views is None else [int(v) for v in views]
        sizes = {(self.cameras[i].width, self.cameras[i].height) for i in idx}
        if len(sizes) > 1:
            raise ValueError("MVS.visibility: cameras of different sizes go in separate calls")
        if not idx:
            raise ValueError("MVS.visibility: no camera")
        w, h = next(iter(sizes))
        if radius is None:
            radius = self.neighbor_radius()
        c = self.cloud()
        return rnd.visibility(c[:, :3], c[:, 3:], [rnd.view_of(self.cameras[i]) for i in idx], w, h, radius=radius, tol=tol,
                              self_index=self_index, keep_maps=keep_maps, device=self.device)

    def cloud_sha1(self) -> str:
        """SHA-1 over the PATCHES payload of an MVS_V3 file (io/filewriter.cpp:97-99: per patch in id order centre[3],
        normalS[2], int K, int camIdx[K], fitness, correlation -- raw little-endian bytes): one string that pins every
        accepted patch, its order and its camera set."""
        return patches_sha1((p.center[:], p.normalS[:], p.cams(), p.fitness, p.correlation) for p in self.patches())

    # ---- writers (MVS::writeMVS / writePLY / writePSR, mvs.cpp:174-184 -> io/filewriter.cpp)
    def _io_cameras(self):
        from . import io
        return [io.io_camera(c.name or ("cam%04d" % i), c.focal, c.principle_point, c.quaternion, c.center, c.radial_distortion)
                for i, c in enumerate(self.cameras)]

    def colors_bgr(self) -> np.ndarray:
        """Patch colour as Patch::setImagePoint picks it (patch.cpp:649-652): the reference camera's pixel at
        the rounded projection of the centre (gray pipelines replicate the gray value)."""
        out = []
        for p in self.patches():
            if p.ref_cam < 0 or p.ref_cam not in p.cams():
                raise RuntimeError("patch without a reference camera: colours are defined through it (patch.cpp:649-652)")
            cam = self.cameras[p.ref_cam]
            k = p.cams().index(p.ref_cam)
            x, y = int(np.rint(p.imgPoint[k][0])), int(np.rint(p.imgPoint[k][1]))
            x = min(max(x, 0), cam.width - 1); y = min(max(y, 0), cam.height - 1)
            if cam.rgb is not None:
                out.append(cam.rgb[y, x, ::-1] if cam.rgb.shape[-1] == 3 else [cam.rgb[y, x]] * 3)
            else:
                out.append([cam.image[y, x]] * 3)
        return np.asarray(out, dtype=np.uint8).reshape(-1, 3)

    def writeMVS(self, path: str):
        from . import io
        cfg = self.cfg
        cfg.neighborRadius = self.neighbor_radius()
        pats = [io.io_patch(p.center[:], p.normalS[:], p.cams(), p.fitness, p.correlation) for p in self.patches()]
        io.write_mvs(path, cfg, self._io_cameras(), pats)

    def writePLY(self, path: str):
        from . import io
        c = self.cloud()
        io.write_ply(path, c[:, :3], c[:, 3:], self.colors_bgr())

    def writePSR(self, path: str):
        from . import io
        c = self.cloud()
        io.write_psr(path, c[:, :3], c[:, 3:])
