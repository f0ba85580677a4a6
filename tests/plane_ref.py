"""Helpers of tests/test_planes_cpu.py and tests/test_planes_gpu.py: the host shim of pais_plane.hpp (tests/plane_host_shim.cpp),
the test inputs, and the statements of pais_cloud_planes (include/pais_cloud.h) restated with Python floats -- IEEE doubles, one
rounding per operation, every loop strictly from left to right, as knn_ref.rule_loops does -- over a knn_ref.brute_knn table."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np

from tests import knn_ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OK, FEW, NOCONV, SWEEPS = 0, 1, 2, 60
EPS = sys.float_info.epsilon
FIELDS = ("centroid", "normal", "eigen", "offset", "variation")

# (nq, nt, k, skip_self) of the bit-for-bit comparisons: m < 3 with and without the query, padded rows, sizes that are no multiple
# of the block (256) or the tile (512), every list size (8, 16, 32) and a set against itself
CASES = ((5, 2, 4, False), (300, 5, 8, False), (257, 513, 8, False), (63, 511, 32, False), (700, 700, 9, True))


class CPlane(C.Structure):
    _fields_ = [("centroid", C.c_double * 3), ("normal", C.c_double * 3), ("eigen", C.c_double * 3), ("offset", C.c_double),
                ("variation", C.c_double), ("count", C.c_int32), ("status", C.c_int32)]


def case_points(nq, nt, k, skip):
    rng = np.random.default_rng(1000 * nq + k)
    q, t = rng.normal(size=(nq, 3)), rng.normal(size=(nt, 3))
    return (t, t) if skip else (q, t)


# --------------------------------------------------------------------------------------------------------- the shim ---
_shim = None


def _compile(out, extra):
    src = os.path.join(HERE, "plane_host_shim.cpp")
    csrc = os.path.join(ROOT, "pais_mvs_amd", "csrc")
    deps = [src, os.path.join(csrc, "pais_plane.hpp"), os.path.join(csrc, "pais_dev.hpp"), os.path.join(ROOT, "include", "pais_cloud.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off"] + extra + ["-o", out, src])
    return out


def shim():
    global _shim
    if _shim is None:
        S = C.CDLL(_compile(os.path.join(HERE, "build", "libplane_host_shim.so"), ["-fPIC", "-shared"]))
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        S.shim_sizeof_plane.restype = C.c_size_t
        assert S.shim_sizeof_plane() == C.sizeof(CPlane)
        S.shim_planes.restype = None
        S.shim_planes.argtypes = [C.c_int, C.c_int, C.c_int, dp, C.c_int, dp, ip, dp, C.POINTER(CPlane), C.POINTER(C.c_int)]
        _shim = S
    return _shim


def sanitized_program():
    """The shim with its own main, built with -fsanitize=address,undefined: a stand-alone program."""
    return _compile(os.path.join(HERE, "build", "plane_shim_asan"),
                    ["-g", "-DPLANE_SHIM_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def records(arr):
    """(n) CPlane -> dict of arrays, the layout evaluate.planes returns"""
    n = len(arr)
    a = np.frombuffer(arr, dtype=np.uint8).reshape(n, C.sizeof(CPlane)) if n else np.zeros((0, C.sizeof(CPlane)), np.uint8)
    d = np.ascontiguousarray(a[:, :88]).view(np.float64).reshape(n, 11)
    i = np.ascontiguousarray(a[:, 88:]).view(np.int32).reshape(n, 2)
    return {"centroid": d[:, 0:3].copy(), "normal": d[:, 3:6].copy(), "eigen": d[:, 6:9].copy(), "offset": d[:, 9].copy(),
            "variation": d[:, 10].copy(), "count": i[:, 0].copy(), "status": i[:, 1].copy()}


def shim_planes(q, t, index, with_query, toward=None):
    """-> (dict of arrays, rotating sweeps (n,))"""
    q, t = np.ascontiguousarray(q, np.float64), np.ascontiguousarray(t, np.float64)
    index = np.ascontiguousarray(index, np.int32)
    n, k = index.shape
    out, sweeps = (CPlane * max(n, 1))(), np.zeros(max(n, 1), np.int32)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    tw = None if toward is None else np.ascontiguousarray(toward, np.float64)
    shim().shim_planes(1 if with_query else 0, k, n, dp(q), len(t), dp(t), index.ctypes.data_as(C.POINTER(C.c_int32)),
                       None if tw is None else dp(tw), out, sweeps.ctypes.data_as(C.POINTER(C.c_int)))
    return records((CPlane * n).from_buffer_copy(bytes(out)[:n * C.sizeof(CPlane)])), sweeps[:n].copy()


# ------------------------------------------------------------------------------------------------------ restatement ---
def _rotate(a, v, p, q, r):
    """one pair of a sweep on the symmetric a (3 x 3 lists, both triangles kept) and v -> whether it rotated"""
    g = a[p][q]
    if g == 0.0:
        return False
    if abs(g) <= EPS * math.sqrt(abs(a[p][p]) * abs(a[q][q])):
        a[p][q] = a[q][p] = 0.0
        return False
    zeta = (a[q][q] - a[p][p]) / (2.0 * g)
    t = (1.0 if zeta >= 0 else -1.0) / (abs(zeta) + math.sqrt(1.0 + zeta * zeta))
    c = 1.0 / math.sqrt(1.0 + t * t)
    s = c * t
    h = t * g
    a[p][p] = a[p][p] - h
    a[q][q] = a[q][q] + h
    a[p][q] = a[q][p] = 0.0
    x, y = a[r][p], a[r][q]
    a[r][p] = a[p][r] = c * x - s * y
    a[r][q] = a[q][r] = s * x + c * y
    for j in range(3):
        x, y = v[j][p], v[j][q]
        v[j][p] = c * x - s * y
        v[j][q] = s * x + c * y
    return True


def covariance(pts):
    """the centroid and covariance statements over a neighbourhood of m >= 1 points -> (centroid list, 3 x 3 lists)"""
    m = len(pts)
    cen = []
    for ax in range(3):
        s = 0.0
        for p in pts:
            s += float(p[ax])
        cen.append(s / float(m))
    a = [[0.0] * 3 for _ in range(3)]
    for i, j in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)):
        s = 0.0
        for p in pts:
            s += (float(p[i]) - cen[i]) * (float(p[j]) - cen[j])
        a[i][j] = a[j][i] = s / float(m)
    return cen, a


def fit_one(query, pts, toward=None):
    """pts: the neighbourhood in its order (the query first if it takes part) -> (record dict of Python values, rotating sweeps)"""
    qx, qy, qz = (float(v) for v in query)
    m = len(pts)
    rec = {"centroid": [0.0] * 3, "normal": [0.0] * 3, "eigen": [0.0] * 3, "offset": 0.0, "variation": 0.0, "count": m,
           "status": FEW if m < 3 else OK}
    if m < 3:
        return rec, 0
    cen, a = covariance(pts)
    v =[[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    rotating, converged = 0, False
    for _ in range(SWEEPS):
        rotated = _rotate(a, v, 0, 1, 2)
        rotated = _rotate(a, v, 0, 2, 1) or rotated
        rotated = _rotate(a, v, 1, 2, 0) or rotated
        if not rotated:
            converged = True
            break
        rotating += 1
    if not converged:
        rec["status"] = NOCONV
    pairs = [[a[j][j], [v[0][j], v[1][j], v[2][j]]] for j in range(3)]
    for lo, hi in ((0, 1), (1, 2), (0, 1)):                  # the stable insertion sort of three under `<`
        if pairs[hi][0] < pairs[lo][0]:
            pairs[lo], pairs[hi] = pairs[hi], pairs[lo]
    e = [pairs[0][0], pairs[1][0], pairs[2][0]]
    n = list(pairs[0][1])
    if toward is not None:
        tx, ty, tz = (float(w) for w in toward)
        flip = ((n[0] * tx) + (n[1] * ty)) + (n[2] * tz) < 0.0
    else:
        big = n[0]
        if abs(n[1]) > abs(big):
            big = n[1]
        if abs(n[2]) > abs(big):
            big = n[2]
        flip = big < 0.0
    if flip:
        n = [-n[0], -n[1], -n[2]]
    with np.errstate(invalid="ignore", divide="ignore"):
        variation = float(np.float64(e[0]) / np.float64((e[0] + e[1]) + e[2]))    # a Python float raises on / 0
    rec.update(centroid=cen, normal=n, eigen=e, offset=((n[0] * (qx - cen[0])) + (n[1] * (qy - cen[1]))) + (n[2] * (qz - cen[2])),
               variation=variation)
    return rec, rotating


def ref_planes(q, t, index, with_query, toward=None):
    """the restatement over a table -> (dict of arrays, rotating sweeps)"""
    q, t = np.asarray(q, np.float64), np.asarray(t, np.float64)
    recs, sweeps = [], []
    for i in range(len(q)):
        pts = ([q[i].tolist()] if with_query else []) + [t[j].tolist() for j in index[i] if 0 <= j < len(t)]
        r, s = fit_one(q[i], pts, None if toward is None else toward[i])
        recs.append(r)
        sweeps.append(s)
    n = len(recs)
    out = {f: np.array([r[f] for r in recs], np.float64).reshape((n, 3) if f in FIELDS[:3] else (n,)) for f in FIELDS}
    out["count"] = np.array([r["count"] for r in recs], np.int32)
    out["status"] = np.array([r["status"] for r in recs], np.int32)
    return out, np.array(sweeps, np.int32)


def assert_same_records(got, want, what=""):
    """every field bit for bit, NaN equal to NaN"""
    for f in FIELDS:
        assert np.asarray(got[f]).shape == np.asarray(want[f]).shape, (what, f)
        g, w = np.asarray(got[f], np.float64).ravel(), np.asarray(want[f], np.float64).ravel()
        bad = np.flatnonzero(~((g.view(np.uint64) == w.view(np.uint64)) | (np.isnan(g) & np.isnan(w))))
        assert not len(bad), (what, f, len(bad), bad[:5], g[bad[:5]], w[bad[:5]])
    for f in ("count", "status"):
        assert np.array_equal(got[f], want[f]), (what, f)


def normal_rule_loop(status, fitted, given, min_cos):
    """pais_cloud_normal_rule, one statement per row"""
    out = []
    for st, g, p in zip(status, fitted, given):
        g, p = [float(x) for x in g], [float(x) for x in p]
        out.append(bool(st == OK and abs(((g[0] * p[0]) + (g[1] * p[1])) + (g[2] * p[2])) < min_cos))
    return out


def check_refusals():
    """every refusal of pais_cloud_planes: < 0 with the error text, nothing launched, no output touched; nq == 0 is no error"""
    from pais_mvs_amd import _lib
    L = _lib.load()
    K = 3
    q, t, tw = np.zeros((4, 3)), np.ones((4, 3)), np.ones((4, 3))
    idx, d2 = np.full((4, K), 77, np.int32), np.full((4, K), 77.0)
    rec = (_lib.Plane * 4)()
    for r in rec:
        r.offset, r.count = 77.0, 77
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ip = idx.ctypes.data_as(C.POINTER(C.c_int32))
    nan, inf, bad_tw = q.copy(), t.copy(), tw.copy()
    nan[3, 2], inf[0, 1], bad_tw[2, 0] = float("nan"), float("-inf"), float("inf")
    SKIP, WQ, OR = _lib.KNN_SKIP_SAME_INDEX, _lib.PLANE_WITH_QUERY, _lib.PLANE_ORIENT
    before = L.pais_cloud_launches()
    for args, msg in [((0, 0, 0, 4, dp(q), 4, dp(t), None, rec, ip, dp(d2), None), "k = 0"),
                      ((0, WQ, 33, 4, dp(q), 4, dp(t), None, rec, ip, dp(d2), None), "k = 33"),
                      ((0, 8, K, 4, dp(q), 4, dp(t), None, rec, ip, dp(d2), None), "unknown flag bits"),
                      ((0, -1, K, 4, dp(q), 4, dp(t), dp(tw), rec, ip, dp(d2), None), "unknown flag bits"),
                      ((0, SKIP | WQ, K, 3, dp(q), 4, dp(t), None, rec, ip, dp(d2), None), "nq != nt"),
                      ((0, SKIP, K, 0, dp(q), 4, dp(t), None, rec, ip, dp(d2), None), "nq != nt"),
                      ((0, 0, K, -4, dp(q), 4, dp(t), None, rec, ip, dp(d2), None), "negative count"),
                      ((0, 0, K, 4, dp(q), -1, dp(t), None, rec, ip, dp(d2), None), "negative count"),
                      ((0, 0, K, 4, None, 4, dp(t), None, rec, ip, dp(d2), None), "null pointer"),
                      ((0, 0, K, 4, dp(q), 4, None, None, rec, ip, dp(d2), None), "null pointer"),
                      ((0, 0, K, 4, dp(q), 4, dp(t), None, rec, None, dp(d2), None), "null pointer"),      # the table: both or neither
                      ((0, 0, K, 4, dp(q), 4, dp(t), None, rec, ip, None, None), "null pointer"),
                      ((0, 0, K, 4, dp(q), 0, dp(t), None, rec, ip, dp(d2), None), "nt == 0"),
                      ((-1, WQ, K, 4, dp(q), 4, dp(t), None, rec, ip, dp(d2), None), "device < 0"),
                      ((0, 0, K, 4, dp(nan), 4, dp(t), None, rec, ip, dp(d2), None), "queries[3] coordinate 2 is not finite"),
                      ((0, SKIP, K, 4, dp(q), 4, dp(inf), None, rec, ip, dp(d2), None), "targets[0] coordinate 1 is not finite"),
                      ((0, WQ, K, 4, dp(q), 4, dp(t), None, None, ip, dp(d2), None), "null planes"),
                      ((0, OR, K, 4, dp(q), 4, dp(t), None, rec, ip, dp(d2), None), "PAIS_PLANE_ORIENT without toward"),
                      ((0, WQ, K, 4, dp(q), 4, dp(t), dp(tw), rec, ip, dp(d2), None), "toward without PAIS_PLANE_ORIENT"),
                      ((0, OR | WQ, K, 4, dp(q), 4, dp(t), dp(bad_tw), rec, None, None, None), "toward[2] coordinate 0 is not finite")]:
        rc = L.pais_cloud_planes(*args)
        err = L.pais_cloud_last_error().decode()
        assert rc < 0 and err.startswith("pais_cloud_planes:") and msg in err, (rc, err, msg)
    assert L.pais_cloud_planes(0, 0, K, 0, None, 0, None, None, None, None, None, None) == 0
    assert L.pais_cloud_planes(-1, WQ, K, 0, dp(q), 4, dp(t), None, rec, ip, dp(d2), None) == 0
    assert L.pais_cloud_launches() == before and (idx == 77).all() and (d2 == 77.0).all()
    assert all(r.offset == 77.0 and r.count == 77 for r in rec)


# ------------------------------------------------------------------------------------------------------------ inputs ---
def anchor_points(axis, seed=0):
    """nine random points with coordinate `axis` set to 0.5: the plane is exact"""
    p = np.random.default_rng(40 + axis + 10 * seed).normal(size=(9, 3))
    p[:, axis] = 0.5
    return p


def degenerate_rows():
    """name -> nine points: all equal, exactly collinear, duplicated"""
    rng = np.random.default_rng(91)
    one = np.repeat(rng.normal(size=(1, 3)), 9, axis=0)
    line = np.arange(9.0)[:, None] * np.array([[1.0, 2.0, 3.0]])
    dup = np.repeat(rng.normal(size=(3, 3)), 3, axis=0)
    return {"all equal": one, "collinear": line, "duplicates": dup}


def lapack_inputs():
    """(name, queries, targets, index, with_query): the five plane_case seeds under a random rotation at k = 8 and 16 (the point
    takes part in its fit), and 3000 random neighbourhoods of 3 .. 32 points with per-axis scales from 1e-3 to 1e3"""
    out = []
    for seed in knn_ref.PLANE_SEEDS:
        rot = np.linalg.qr(np.random.default_rng(700 + seed).normal(size=(3, 3)))[0]
        p = np.ascontiguousarray(knn_ref.plane_case(seed)[0] @ rot.T)
        for k in (8, 16):
            out.append(("plane_case %d, k %d" % (seed, k), p, p, knn_ref.brute_knn(p, p, k, True)[0], True))
    rng = np.random.default_rng(3000)
    index, pts = np.full((3000, 32), -1, np.int32), []
    at = 0
    for i in range(3000):
        m = int(rng.integers(3, 33))
        pts.append(rng.normal(size=(m, 3)) * 10.0 ** rng.uniform(-3.0, 3.0, 3))
        index[i, :m] = np.arange(at, at + m)
        at += m
    out.append(("random neighbourhoods", np.zeros((3000, 3)), np.concatenate(pts), index, False))
    return out


def lapack_errors(rec, q, t, index, with_query):
    """numpy.linalg.eigh on the covariance the statements form -> (largest eigenvalue error in units of DBL_EPSILON lambda_2, largest
    angle in degrees between the normals over the rows with lambda_1 > 20 lambda_0, the number of such rows)"""
    worst_e, worst_a, rows = 0.0, 0.0, 0
    for i in range(len(q)):
        pts = ([q[i].tolist()] if with_query else []) + [t[j].tolist() for j in index[i] if j >= 0]
        w, v = np.linalg.eigh(np.array(covariance(pts)[1]))
        worst_e = max(worst_e, float(np.abs(rec["eigen"][i] - w).max() / (EPS * w[2])))
        if w[1] > 20.0 * w[0]:
            rows += 1
            n = rec["normal"][i]
            worst_a = max(worst_a, math.degrees(math.atan2(float(np.linalg.norm(np.cross(n, v[:, 0]))), abs(float(n @ v[:, 0])))))
    return worst_e, worst_a, rows


def self_table(p, k=8):
    """a set against itself: (index, dist2) without the query's own index"""
    return knn_ref.brute_knn(p, p, k, True)


def tilted_case(seed, tilted=20, angle_deg=60.0):
    """knn_ref.plane_case with a stored normal per point, as the spherical pair (angle from z, azimuth) a patch record holds: z on
    every point, except `tilted` grid points whose normal is tilted `angle_deg` from z -> (points, added, normalS, tilted bool)"""
    pts, added = knn_ref.plane_case(seed)
    rng = np.random.default_rng(500 + seed)
    pick = rng.choice(np.flatnonzero(~added), size=tilted, replace=False)
    ns = np.zeros((len(pts), 2))
    ns[pick] = np.stack([np.full(tilted, math.radians(angle_deg)), rng.uniform(-math.pi, math.pi, tilted)], axis=1)
    mask = np.zeros(len(pts), bool)
    mask[pick] = True
    return pts, added, ns, mask
