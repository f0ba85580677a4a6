"""Helpers of tests/test_seed_generation.py for the descriptor matcher (k_nearest_descriptor of pais_seed.hip): a numpy float32
restatement of the nearest search written from the kernel's comment alone, the oracle's po_seed_match behind numpy arrays, and
the descriptor sets at which a wave-per-query search can go wrong -- fewer train rows than lanes, exact ties across and inside
lanes, rows no distance beats, the grid-stride loop, dimensions that are no multiple of the wave."""
import ctypes as C

import numpy as np

FLT_MAX = np.float32(3.4028235e+38)


def np_nearest(q, t):
    """For every row of q (nq, dim) its nearest row of t (nt, dim): (index int32, distance float32).  Per block of four
    differences s = s + (((v0 v0 + v1 v1) + v2 v2) + v3 v3), every product and sum rounded to float32, a tail of single
    s = s + v v, then sqrt in float32.  The scan starts from (-1, FLT_MAX) and takes a row only when it is strictly nearer:
    the first of the least distances below FLT_MAX (a NaN or an infinite distance never wins)."""
    q, t = np.asarray(q, np.float32), np.asarray(t, np.float32)
    nq, dim = q.shape
    nt = len(t)
    if nt == 0:
        return np.full(nq, -1, np.int32), np.full(nq, FLT_MAX, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        s = np.zeros((nq, nt), np.float32)
        i = 0
        while i <= dim - 4:
            v0, v1, v2, v3 = (q[:, None, i + k] - t[None, :, i + k] for k in range(4))
            s = s + (((v0 * v0 + v1 * v1) + v2 * v2) + v3 * v3)
            i += 4
        while i < dim:
            v = q[:, None, i] - t[None, :, i]
            s = s + v * v
            i += 1
        assert s.dtype == np.float32
        d = np.sqrt(s)
        beats = d < FLT_MAX
    least = np.where(beats, d, np.float32(np.inf))
    first = np.argmin(least, axis=1).astype(np.int32)            # argmin: the first of equal values
    some = beats.any(axis=1)
    return np.where(some, first, np.int32(-1)).astype(np.int32), np.where(some, d[np.arange(nq), first], FLT_MAX).astype(np.float32)


def np_match(q, t):
    """BFMatcher(NORM_L2, crossCheck=True): q keeps its nearest t only if t's nearest is q -> (train of query or -1, distance)."""
    bq, dist = np_nearest(q, t)
    bt, _ = np_nearest(t, q)
    safe = np.clip(bq, 0, max(len(t) - 1, 0))
    keep = (bq >= 0) & (bt[safe] == np.arange(len(q))) if len(t) else np.zeros(len(q), bool)
    return np.where(keep, bq, -1).astype(np.int32), dist


def oracle_match(q, t):
    """po_seed_match of oracle/po_seed.c -> (train of query or -1 (int32), distance (float32))."""
    from oracle import po
    L = po.lib()
    fpp = C.POINTER(C.c_float)
    q, t = np.ascontiguousarray(q, np.float32), np.ascontiguousarray(t, np.float32)
    want = (C.c_int * max(len(q), 1))()
    wd = (C.c_float * max(len(q), 1))()
    L.po_seed_match(len(q), q.ctypes.data_as(fpp), len(t), t.ctypes.data_as(fpp), q.shape[1], want, wd)
    return np.array(want[:len(q)], np.int32), np.frombuffer(wd, dtype=np.float32)[:len(q)].copy()


def _rows(rng, n, dim):
    return rng.integers(0, 256, size=(n, dim)).astype(np.float32)


def _pair(rng, nq, nt, dim):
    """Random 0..255 rows; the first min(nq, nt) // 2 train rows are noisy copies of the queries (true partners)."""
    q, t = _rows(rng, nq, dim), _rows(rng, nt, dim)
    k = min(nq, nt) // 2
    t[:k] = q[:k] + rng.normal(0, 2.0, (k, dim)).astype(np.float32)
    return q, t


def matcher_cases():
    """name -> (query, train).  The same arrays for the CPU pin of np_match and for the GPU tests."""
    rng = np.random.default_rng(21)
    out = {}
    for nt in (1, 2, 63, 64, 65, 127, 129):                      # nt < 64: 64 - nt lanes enter the reduction with no row
        out["nt%d" % nt] = _pair(rng, 70, nt, 128)
    out["nq1"] = _pair(rng, 1, 200, 128)
    row = _rows(rng, 1, 128)
    out["all-equal"] = (np.repeat(row, 70, axis=0), np.repeat(row, 130, axis=0))
    q, t = _rows(rng, 10, 128), _rows(rng, 200, 128)
    t[63] = t[64] = q[3]                                         # the lower index sits in the higher lane
    t[5] = t[69] = q[4]                                          # both in lane 5
    t[2] = t[130] = q[5]
    out["ties"] = (q, t)
    q, t = _pair(rng, 70, 130, 128)
    q[11] = np.nan
    t[7] = np.nan
    out["nan"] = (q, t)
    q, t = _pair(rng, 70, 130, 128)
    q[13] = 3e30                                                 # every squared sum overflows to +inf
    out["overflow"] = (q, t)
    out["grid-stride"] = (rng.integers(0, 4, size=(65536 + 70, 4)).astype(np.float32), rng.integers(0, 4, size=(3, 4)).astype(np.float32))
    for dim in (4, 8, 64, 132):                                  # below one wave of floats; no multiple of 64
        out["dim%d" % dim] = _pair(rng, 70, 130, dim)
    return out


def check_case_properties(name, q, t, idx, dist):
    """What the issue states about a case's expected result, asserted on a REFERENCE result (oracle or restatement)."""
    if name == "all-equal":
        assert np.all(dist == 0.0) and list(idx) == [0] + [-1] * (len(q) - 1)
    elif name == "ties":
        assert (idx[3], idx[4], idx[5]) == (63, 5, 2) and dist[3] == dist[4] == dist[5] == 0.0
    elif name == "nan":
        assert idx[11] == -1 and dist[11] == FLT_MAX and 7 not in set(idx.tolist())
        assert (np.delete(idx, 11) >= 0).sum() >= 20
    elif name == "overflow":
        assert idx[13] == -1 and dist[13] == FLT_MAX
    elif name == "grid-stride":
        assert len(q) == 65536 + 70
