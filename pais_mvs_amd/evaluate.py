"""Score a cloud against ground truth: accuracy and completeness (the reference's only published kind of result: Middlebury,
SURVEY.md section 6) over the exact GPU nearest-neighbour search of include/pais_cloud.h.

    accuracy      the distance d such that `fraction` of the cloud lies within d of the truth
    completeness  the share of the truth that lies within `threshold` of the cloud

Both searches (cloud -> truth, truth -> cloud) run on the GPU and there is no CPU fallback; the order statistics and counts
are numpy on the host.  Order statistics are taken without interpolation -- element ceil(fraction n) - 1 of the sorted
distances, the smallest distance that holds at least that share -- so two runs can be compared exactly.

    python -m pais_mvs_amd.evaluate cloud.{mvs,ply,npy} --truth truth.{ply,npy} --threshold T [--fraction 0.9] [--json OUT]
    python -m pais_mvs_amd.evaluate --write-truth-for pawn|ring|dome --truth truth.npy [--stride 2] [--min-views 3]
    python -m pais_mvs_amd.evaluate cloud.{mvs,ply,npy} --spacing
    python -m pais_mvs_amd.evaluate cloud.{mvs,ply,npy} --roughness K
    python -m pais_mvs_amd.evaluate points.{mvs,ply,npy} --estimate-normals K [--viewpoint X,Y,Z] --out FILE.{npy,psr}

The plane through every point's k nearest neighbours (planes, pais_cloud_planes) gives bare points a normal
(estimate_normals), a cloud a truth-free measure of its noise across the surface (roughness) and the driver a filter that
compares a patch's photo-consistent normal with the geometry around it (MVS.normalFiltering).

The k nearest neighbours of every point (knn) give a cloud its own scale and an outlier rule that adapts to it: spacing() is
the median distance to the nearest other point (a disc radius for render, a threshold for score when no truth pitch is at
hand), statistical_outliers() flags the points whose mean distance to their k nearest lies sigma deviations above the cloud's.

visible_cameras() answers "which cameras see this point" from geometry alone, for a cloud that has no images: the cloud
rendered as discs into every camera and each point depth-tested against those maps (render.visibility, pais_cloud_visibility).
"""
from __future__ import annotations

import ctypes as C
import json
import math
import sys

import numpy as np

from . import _lib


def nearest(queries, targets, device: int = 0):
    """pais_cloud_nearest: for every query (n,3) the lowest index of the nearest target (m,3) and the squared distance
    ((dx dx) + (dy dy)) + (dz dz) to it, every operation rounded to double -> (idx int32 (n,), d2 float64 (n,), kernel_ms)."""
    q = np.ascontiguousarray(queries, dtype=np.float64)
    t = np.ascontiguousarray(targets, dtype=np.float64)
    if q.ndim != 2 or q.shape[1] != 3 or t.ndim != 2 or t.shape[1] != 3:
        raise ValueError("nearest: queries and targets are (n, 3) arrays, got %s and %s" % (q.shape, t.shape))
    L = _lib.load()
    idx = np.empty(len(q), dtype=np.int32)
    d2 = np.empty(len(q), dtype=np.float64)
    ms = C.c_double(0)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    rc = L.pais_cloud_nearest(int(device), len(q), dp(q), len(t), dp(t), idx.ctypes.data_as(C.POINTER(C.c_int32)), dp(d2), C.byref(ms))
    if rc:
        raise RuntimeError("pais_cloud_nearest failed (%d): %s" % (rc, L.pais_cloud_last_error().decode()))
    return idx, d2, ms.value


def order_index(fraction: float, n: int) -> int:
    """ceil(fraction n) - 1, kept inside [0, n - 1]."""
    return min(max(int(math.ceil(fraction * n)) - 1, 0), n - 1)


def _knn(queries, targets, k: int, skip_self: bool, device: int):
    q = np.ascontiguousarray(queries, dtype=np.float64)
    t = q if targets is queries else np.ascontiguousarray(targets, dtype=np.float64)
    if q.ndim != 2 or q.shape[1] != 3 or t.ndim != 2 or t.shape[1] != 3:
        raise ValueError("knn: queries and targets are (n, 3) arrays, got %s and %s" % (q.shape, t.shape))
    L = _lib.load()
    k = int(k)
    idx = np.empty((len(q), max(k, 0)), dtype=np.int32)
    d2 = np.empty((len(q), max(k, 0)), dtype=np.float64)
    ms = C.c_double(0)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    rc = L.pais_cloud_knn(int(device), _lib.KNN_SKIP_SAME_INDEX if skip_self else 0, k, len(q), dp(q), len(t), dp(t),
                          idx.ctypes.data_as(C.POINTER(C.c_int32)), dp(d2), C.byref(ms))
    if rc:
        raise RuntimeError("pais_cloud_knn failed (%d): %s" % (rc, L.pais_cloud_last_error().decode()))
    return idx, d2, ms.value


def knn(queries, targets, k: int, skip_self: bool = False, device: int = 0):
    """pais_cloud_knn: row i holds the first k targets (m,3) of query i (n,3) ordered by (squared distance, target index), the
    distance being nearest()'s; skip_self leaves target i out of row i (a set against itself).  A row with fewer than k
    admissible targets ends in index -1, dist2 +inf -> (index int32 (n,k), dist2 float64 (n,k))."""
    return _knn(queries, targets, k, skip_self, device)[:2]


def spacing(points, device: int = 0) -> float:
    """The sample spacing of a point set (n >= 2, (n,3)): the median distance to the nearest other point -- the square root of
    element ceil(n / 2) - 1 of the sorted first-neighbour dist2 of the set against itself."""
    p = np.ascontiguousarray(points, dtype=np.float64)
    if p.ndim != 2 or p.shape[1] != 3 or len(p) < 2:
        raise ValueError("spacing: an (n, 3) array of at least two points, got %s" % (p.shape,))
    d2 = _knn(p, p, 1, True, device)[1][:, 0]
    return float(math.sqrt(np.sort(d2)[order_index(0.5, len(p))]))


def outlier_rule(index, dist2, sigma: float) -> dict:
    """pais_cloud_outlier_rule over a knn table: the host arithmetic of statistical_outliers."""
    index = np.ascontiguousarray(index, dtype=np.int32)
    dist2 = np.ascontiguousarray(dist2, dtype=np.float64)
    if index.ndim != 2 or index.shape != dist2.shape:
        raise ValueError("outlier_rule: index and dist2 are (n, k) tables, got %s and %s" % (index.shape, dist2.shape))
    n, k = index.shape
    mean, stats, out = np.empty(n, np.float64), np.empty(3, np.float64), np.zeros(n, np.uint8)
    L = _lib.load()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    if L.pais_cloud_outlier_rule(n, k, index.ctypes.data_as(C.POINTER(C.c_int32)), dp(dist2), float(sigma), dp(mean), dp(stats),
                                 out.ctypes.data_as(C.POINTER(C.c_uint8))):
        raise RuntimeError("pais_cloud_outlier_rule failed: %s" % L.pais_cloud_last_error().decode())
    return {"outlier": out.astype(bool), "mean_dist": mean, "mu": float(stats[0]), "sd": float(stats[1]), "threshold": float(stats[2])}


def statistical_outliers(points, k: int = 8, sigma: float = 2.0, device: int = 0) -> dict:
    """The statistical outlier rule on a point set (n,3) (or (n,6): the normals are not read): a point is an outlier if the
    mean distance to its k nearest other points exceeds mu + sigma sd of that mean over the set (include/pais_cloud.h).
    -> {"outlier" bool (n,), "mean_dist" (n,), "mu", "sd", "threshold"}."""
    p = np.ascontiguousarray(np.asarray(points, np.float64)[:, :3])
    idx, d2, _ = _knn(p, p, k, True, device)
    return outlier_rule(idx, d2, sigma)


def _plane_arrays(rec, n: int) -> dict:
    """(n) _lib.Plane -> dict of arrays"""
    size = C.sizeof(_lib.Plane)
    raw = np.frombuffer(bytes(rec)[:n * size], dtype=np.uint8).reshape(n, size)
    d = np.ascontiguousarray(raw[:, :88]).view(np.float64).reshape(n, 11)
    i = np.ascontiguousarray(raw[:, 88:]).view(np.int32).reshape(n, 2)
    return {"centroid": d[:, 0:3].copy(), "normal": d[:, 3:6].copy(), "eigen": d[:, 6:9].copy(), "offset": d[:, 9].copy(),
            "variation": d[:, 10].copy(), "count": i[:, 0].copy(), "status": i[:, 1].copy()}


def planes(points, k: int, targets=None, with_query: bool = True, toward=None, device: int = 0, skip_self=None, table: bool = True) -> dict:
    """pais_cloud_planes: the plane through every point's k nearest targets (include/pais_cloud.h has the statements).  targets
    None: the points against themselves without their own index (skip_self, which may be forced either way); with_query: the point
    itself takes part in its fit; toward (n,3): the normals are signed toward these vectors, else so that their largest component is
    positive.  -> {"centroid" (n,3), "normal" (n,3), "eigen" (n,3) ascending, "offset" (n,), "variation" (n,), "count", "status"
    int32 (n,), "kernel_ms": [search + merge, fit]} and, with table, "index" / "dist2" (n,k): pais_cloud_knn's table."""
    q = np.ascontiguousarray(np.asarray(points, np.float64))
    t = q if targets is None else np.ascontiguousarray(np.asarray(targets, np.float64))
    if q.ndim != 2 or q.shape[1] != 3 or t.ndim != 2 or t.shape[1] != 3:
        raise ValueError("planes: points and targets are (n, 3) arrays, got %s and %s" % (q.shape, t.shape))
    if skip_self is None:
        skip_self = targets is None
    flags = (_lib.KNN_SKIP_SAME_INDEX if skip_self else 0) | (_lib.PLANE_WITH_QUERY if with_query else 0)
    tw = None
    if toward is not None:
        tw = np.ascontiguousarray(np.asarray(toward, np.float64))
        if tw.shape != q.shape:
            raise ValueError("planes: toward is one vector per point, got %s for %s" % (tw.shape, q.shape))
        flags |= _lib.PLANE_ORIENT
    L = _lib.load()
    k, n = int(k), len(q)
    rec = (_lib.Plane * max(n, 1))()
    idx = np.empty((n, max(k, 0)), dtype=np.int32) if table else None
    d2 = np.empty((n, max(k, 0)), dtype=np.float64) if table else None
    ms, split = C.c_double(0), (C.c_double * 2)(0, 0)
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    rc = L.pais_cloud_planes(int(device), flags, k, n, dp(q), len(t), dp(t), dp(tw), rec,
                             None if idx is None else idx.ctypes.data_as(C.POINTER(C.c_int32)), dp(d2), C.byref(ms))
    if rc:
        raise RuntimeError("pais_cloud_planes failed (%d): %s" % (rc, L.pais_cloud_last_error().decode()))
    out = _plane_arrays(rec, n)
    if n:
        L.pais_cloud_planes_last_ms(split)
    out["kernel_ms"] = [float(split[0]), float(split[1])]
    if table:
        out["index"], out["dist2"] = idx, d2
    return out


def normal_rule(plane_records: dict, normals, min_cos: float) -> np.ndarray:
    """pais_cloud_normal_rule over the output of planes(): True where the fit is OK and |fitted . given| < min_cos."""
    n = len(plane_records["status"])
    given = np.ascontiguousarray(np.asarray(normals, np.float64))
    if given.shape != (n, 3):
        raise ValueError("normal_rule: one normal per record, got %s for %d" % (given.shape, n))
    rec = (_lib.Plane * max(n, 1))()
    for i in range(n):
        rec[i].normal[:] = plane_records["normal"][i].tolist()
        rec[i].status = int(plane_records["status"][i])
    out = np.zeros(n, np.uint8)
    L = _lib.load()
    if L.pais_cloud_normal_rule(n, rec, given.ctypes.data_as(C.POINTER(C.c_double)), float(min_cos), out.ctypes.data_as(C.POINTER(C.c_uint8))):
        raise RuntimeError("pais_cloud_normal_rule failed: %s" % L.pais_cloud_last_error().decode())
    return out.astype(bool)


def estimate_normals(points, k: int = 16, viewpoint=None, device: int = 0) -> np.ndarray:
    """Bare points (n,3) -> (n,6) points and the normals of planes(points, k) (the point takes part in its own fit), signed toward
    viewpoint - point when a viewpoint (3,) is given.  A point with fewer than three neighbours keeps a zero normal."""
    p = np.ascontiguousarray(np.asarray(points, np.float64)[:, :3])
    toward = None if viewpoint is None else np.asarray(viewpoint, np.float64).reshape(1, 3) - p
    return np.concatenate([p, planes(p, k, toward=toward, device=device, table=False)["normal"]], axis=1)


def roughness(points, k: int = 16, device: int = 0) -> float:
    """The noise of a point set across its own surface, without a truth: the median |offset| of planes(points, k) over the rows
    that were fitted -- element ceil(n / 2) - 1 of the sorted values, as spacing() takes its median.  spacing() measures along
    the surface; the ratio of the two is scale-free."""
    p = np.ascontiguousarray(np.asarray(points, np.float64)[:, :3])
    r = planes(p, k, device=device, table=False)
    off = np.sort(np.abs(r["offset"][r["status"] == _lib.PLANE_OK]))
    if not len(off):
        raise ValueError("roughness: no point of %d has three neighbours" % len(p))
    return float(off[order_index(0.5, len(off))])


def visible_cameras(points_with_normals, cameras, radius=None, tol=None, device: int = 0) -> list:
    """The geometric answer to "which cameras see this point" for a cloud that has no images: the (n,6) cloud rendered as
    back-face-culled discs of `radius` (default spacing()) into every camera (camera.Camera or io.IoCamera records with a
    width and a height; cameras of one size share a call) and each point depth-tested against those maps with tolerance tol
    (default the radius), its own disc counting as the surface (render.visibility, pais_cloud_visibility).
    -> per point the ascending list of camera indices whose code is PAIS_VIS_VISIBLE."""
    from . import render as rnd
    cloud = np.ascontiguousarray(np.asarray(points_with_normals, np.float64))
    if cloud.ndim != 2 or cloud.shape[1] != 6:
        raise ValueError("visible_cameras: an (n, 6) array of points and normals is needed, got %s" % (cloud.shape,))
    cameras = list(cameras)
    if radius is None:
        radius = spacing(cloud[:, :3], device)
    by_size = {}
    for i, cam in enumerate(cameras):
        by_size.setdefault((int(cam.width), int(cam.height)), []).append(i)
    seen = np.zeros((len(cameras), len(cloud)), bool)
    for (w, h), idx in by_size.items():
        v = rnd.visibility(cloud[:, :3], cloud[:, 3:], [rnd.view_of(cameras[i]) for i in idx], w, h, radius=float(radius), tol=tol,
                           occluder=False, margin=False, device=device)
        seen[idx] = v.code == _lib.VIS_VISIBLE
    return [np.flatnonzero(seen[:, i]).tolist() for i in range(len(cloud))]


def score_from_matches(cloud, truth, idx_ct, d2_ct, idx_tc, d2_tc, threshold: float, fraction: float = 0.9) -> dict:
    """The host arithmetic of score(): idx_ct / d2_ct are the nearest truth sample of every cloud point and its squared
    distance, idx_tc / d2_tc the nearest cloud point of every truth sample.  idx_tc is not read: completeness needs the
    distances alone."""
    cloud = np.asarray(cloud, np.float64).reshape(-1, 6)
    truth = np.asarray(truth, np.float64).reshape(-1, 6)
    n, m = len(cloud), len(truth)
    if n == 0 or m == 0:
        raise ValueError("score: empty cloud (%d) or truth (%d)" % (n, m))
    if not 0.0 < fraction <= 1.0:
        raise ValueError("score: fraction %r outside (0, 1]" % (fraction,))
    d2_ct, d2_tc = np.asarray(d2_ct, np.float64), np.asarray(d2_tc, np.float64)
    g = truth[np.asarray(idx_ct, np.int64)]
    k = order_index(fraction, n)
    d_ct, d_tc = np.sqrt(d2_ct), np.sqrt(d2_tc)
    # point-to-plane: the distance to the tangent plane of the nearest truth sample takes the sampling pitch out to first order
    plane = np.abs(np.einsum("ij,ij->i", cloud[:, :3] - g[:, :3], g[:, 3:]))
    # signed, as cloudcmp: a normal pointing the other way is 180 degrees off, not 0
    dot = np.einsum("ij,ij->i", cloud[:, 3:], g[:, 3:])
    ang = np.arccos(np.clip(dot, -1.0, 1.0))
    return {"n": int(n), "m": int(m), "threshold": float(threshold), "fraction": float(fraction),
            "accuracy": float(math.sqrt(np.sort(d2_ct)[k])),
            "accuracy_plane": float(np.sort(plane)[k]),
            "completeness": float(np.count_nonzero(d_tc <= threshold) / m),
            "cloud_to_truth_median": float(np.median(d_ct)), "cloud_to_truth_max": float(d_ct.max()),
            "truth_to_cloud_median": float(np.median(d_tc)), "truth_to_cloud_max": float(d_tc.max()),
            "normal_angle_p90_rad": float(np.sort(ang)[order_index(0.9, n)]),
            "flipped_normals": int(np.count_nonzero(dot < 0))}


def score(cloud, truth, threshold: float, fraction: float = 0.9, device: int = 0) -> dict:
    """cloud (n,6), truth (m,6): points and unit normals.  Two GPU searches, then score_from_matches; the kernel times of the
    two searches are added as kernel_ms_cloud_to_truth / kernel_ms_truth_to_cloud."""
    cloud = np.asarray(cloud, np.float64).reshape(-1, 6)
    truth = np.asarray(truth, np.float64).reshape(-1, 6)
    if not len(cloud) or not len(truth):
        raise ValueError("score: empty cloud (%d) or truth (%d)" % (len(cloud), len(truth)))
    idx_ct, d2_ct, ms_ct = nearest(cloud[:, :3], truth[:, :3], device)
    idx_tc, d2_tc, ms_tc = nearest(truth[:, :3], cloud[:, :3], device)
    out = score_from_matches(cloud, truth, idx_ct, d2_ct, idx_tc, d2_tc, threshold, fraction)
    out["kernel_ms_cloud_to_truth"] = ms_ct
    out["kernel_ms_truth_to_cloud"] = ms_tc
    return out


TIMING_KEYS = ("kernel_ms_cloud_to_truth", "kernel_ms_truth_to_cloud")


# ------------------------------------------------------------------------------------------------------------ files ---
def normals_from_spherical(normalS) -> np.ndarray:
    """(n,2) normalS -> (n,3) normals by the library's own spherical2normal (pais_cloud_normals): the bits a loaded patch holds."""
    ns = np.ascontiguousarray(normalS, dtype=np.float64).reshape(-1, 2)
    out = np.empty((len(ns), 3), dtype=np.float64)
    L = _lib.load()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    if L.pais_cloud_normals(len(ns), dp(ns), dp(out)):
        raise RuntimeError("pais_cloud_normals failed: %s" % L.pais_cloud_last_error().decode())
    return out


def read_ply(path: str, normals: bool = True) -> np.ndarray:
    """The ascii layout pais_io_write_ply writes (x y z nx ny nz + colours) -> (n,6); normals False: x y z alone -> (n,3)."""
    with open(path, "r") as f:
        if f.readline().strip() != "ply":
            raise IOError("%s: not a PLY file" % path)
        n, props, fmt = None, [], None
        for line in f:
            w = line.split()
            if not w:
                continue
            if w[0] == "format":
                fmt = w[1]
            elif w[0] == "element":
                if n is not None or w[1] != "vertex":
                    raise IOError("%s: only a single vertex element is read" % path)
                n = int(w[2])
            elif w[0] == "property":
                props.append(w[-1])
            elif w[0] == "end_header":
                break
        if fmt != "ascii" or n is None:
            raise IOError("%s: not an ascii PLY with a vertex element" % path)
        try:
            cols = [props.index(p) for p in (("x", "y", "z", "nx", "ny", "nz") if normals else ("x", "y", "z"))]
        except ValueError:
            raise IOError("%s: vertex properties %s lack x y z%s" % (path, props, " nx ny nz" if normals else ""))
        rows = np.loadtxt(f, dtype=np.float64, ndmin=2, max_rows=n) if n else np.zeros((0, len(props)))
    if rows.shape != (n, len(props)):
        raise IOError("%s: %s vertex rows, header says %d x %d" % (path, rows.shape, n, len(props)))
    return np.ascontiguousarray(rows[:, cols])


def load_cloud(path: str) -> np.ndarray:
    """.mvs (io.load_mvs; normals from normalS), .ply (read_ply) or .npy ((n,6)) -> (n,6)."""
    ext = path.lower().rsplit(".", 1)[-1]
    if ext == "mvs":
        from . import io
        pats = io.load_mvs(path)[2]
        cen = np.array([p.center[:] for p in pats], dtype=np.float64).reshape(-1, 3)
        return np.concatenate([cen, normals_from_spherical([p.normalS[:] for p in pats])], axis=1)
    if ext == "ply":
        return read_ply(path)
    if ext == "npy":
        a = np.load(path)
        if a.ndim != 2 or a.shape[1] != 6:
            raise IOError("%s: expected an (n, 6) array, got %s" % (path, a.shape))
        return np.asarray(a, np.float64)
    raise IOError("%s: unknown cloud format (expected .mvs, .ply or .npy)" % path)


def load_points(path: str) -> np.ndarray:
    """The points (n,3) of a cloud file: whatever load_cloud reads, and bare points -- .npy (n,3), a PLY without normals."""
    ext = path.lower().rsplit(".", 1)[-1]
    if ext == "npy":
        a = np.load(path)
        if a.ndim != 2 or a.shape[1] not in (3, 6):
            raise IOError("%s: expected an (n, 3) or (n, 6) array, got %s" % (path, a.shape))
        return np.ascontiguousarray(np.asarray(a, np.float64)[:, :3])
    if ext == "ply":
        return read_ply(path, normals=False)
    return np.ascontiguousarray(load_cloud(path)[:, :3])


def save_cloud(path: str, cloud) -> None:
    """(n,6) points and normals -> .npy, or a PSR file (io.write_psr) under any other extension."""
    cloud = np.asarray(cloud, np.float64).reshape(-1, 6)
    if path.lower().endswith(".npy"):
        np.save(path, cloud)
    else:
        from . import io
        io.write_psr(path, cloud[:, :3], cloud[:, 3:])


def parse_viewpoint(text: str):
    """--viewpoint X,Y,Z -> [x, y, z]"""
    import argparse
    try:
        v = [float(w) for w in text.split(",")]
        if len(v) != 3:
            raise ValueError
        return v
    except ValueError:
        raise argparse.ArgumentTypeError("expected X,Y,Z, got %r" % text)


def synthetic_truth(name: str, stride: int = 2, min_views: int = 3, scene_kwargs=None):
    """(truth (m,6), spacing) of the synthetic scene `name` (pais_mvs_amd.synth)."""
    from . import synth
    make = {"pawn": synth.pawn_scene, "ring": synth.ring_scene, "dome": synth.dome_scene}[name]
    pts, nrm, spacing = synth.ground_truth(make(**(scene_kwargs or {})), stride, min_views)
    return np.concatenate([pts, nrm], axis=1), spacing


def main(argv=None) -> int:
    import argparse
    ap = argparse.ArgumentParser(prog="python -m pais_mvs_amd.evaluate", description=__doc__.split("\n\n")[0])
    ap.add_argument("cloud", nargs="?", help="cloud.mvs, cloud.ply or cloud.npy ((n,6))")
    ap.add_argument("--truth", help="truth.ply or truth.npy ((m,6)); the output of --write-truth-for")
    ap.add_argument("--spacing", action="store_true", help="print the cloud's sample spacing (spacing()) and stop; needs no truth")
    ap.add_argument("--threshold", type=float, help="completeness distance (the synthetic scenes: 2 x the printed spacing)")
    ap.add_argument("--fraction", type=float, default=0.9)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--json", help="write the scores here as well")
    ap.add_argument("--write-truth-for", choices=["pawn", "ring", "dome"], help="write the synthetic truth of a scene to --truth (.npy) and stop")
    ap.add_argument("--stride", type=int, default=2)
    ap.add_argument("--min-views", type=int, default=3)
    ap.add_argument("--scene-kwargs", default="{}", help="JSON arguments of the synth scene function (e.g. a smaller rig)")
    ap.add_argument("--roughness", type=int, metavar="K", help="print the cloud's roughness over K neighbours, its spacing and their ratio, and stop; needs no truth")
    ap.add_argument("--estimate-normals", type=int, metavar="K", help="fit a normal to every point of the cloud (bare points will do) "
                    "over K neighbours and write points and normals to --out; needs no truth")
    ap.add_argument("--viewpoint", type=parse_viewpoint, metavar="X,Y,Z", help="with --estimate-normals: sign the normals toward this point "
                    "(a negative X needs the form --viewpoint=X,Y,Z)")
    ap.add_argument("--out", help="with --estimate-normals: FILE.npy ((n,6)), any other extension a PSR file")
    a = ap.parse_args(argv)
    if a.viewpoint and a.estimate_normals is None:
        ap.error("--viewpoint belongs to --estimate-normals")
    if a.estimate_normals is not None:
        if not a.cloud or not a.out:
            ap.error("--estimate-normals needs a cloud and --out")
        cloud = estimate_normals(load_points(a.cloud), a.estimate_normals, a.viewpoint, a.device)
        save_cloud(a.out, cloud)
        print(json.dumps({"n": int(len(cloud)), "k": a.estimate_normals, "out": a.out}))
        return 0
    if a.roughness is not None:
        if not a.cloud:
            ap.error("--roughness needs a cloud")
        pts = load_points(a.cloud)
        r, s = roughness(pts, a.roughness, a.device), spacing(pts, a.device)
        print(json.dumps({"n": int(len(pts)), "k": a.roughness, "roughness": r, "spacing": s, "ratio": r / s if s > 0 else float("nan")}))
        return 0
    if a.spacing:
        if not a.cloud:
            ap.error("--spacing needs a cloud")
        cloud = load_cloud(a.cloud)
        print(json.dumps({"n": int(len(cloud)), "spacing": spacing(cloud[:, :3], a.device)}))
        return 0
    if not a.truth:
        ap.error("the following arguments are required: --truth")
    if a.write_truth_for:
        truth, pitch = synthetic_truth(a.write_truth_for, a.stride, a.min_views, json.loads(a.scene_kwargs))
        np.save(a.truth, truth)
        print(json.dumps({"scene": a.write_truth_for, "m": int(len(truth)), "spacing": pitch, "truth": a.truth}))
        return 0
    if not a.cloud or a.threshold is None:
        ap.error("a cloud and --threshold are required")
    truth = load_cloud(a.truth)
    out = score(load_cloud(a.cloud), truth, a.threshold, a.fraction, a.device)
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
