"""References of the k-nearest tests (test_knn_cpu.py, test_knn_gpu.py): a numpy brute force of pais_cloud_knn's definition and
the outlier rule of include/pais_cloud.h restated with plain Python loops.

The brute force evaluates the three distance statements as separate rounded elementwise passes (no FMA), as
tests/test_evaluate_gpu.py::_brute does, then orders every row with a stable argsort -- (d2 ascending, index ascending), +inf in
index order -- sets the query's own column aside when skipping self and pads with -1 / +inf.  The rule uses Python floats:
IEEE doubles, one rounding per operation, sums strictly from left to right (np.sum is pairwise and is not the statement)."""
import math

import numpy as np


def brute_knn(q, t, k, skip_self=False, chunk=64):
    q, t = np.ascontiguousarray(q, np.float64), np.ascontiguousarray(t, np.float64)
    nq, nt = len(q), len(t)
    assert not skip_self or nq == nt
    idx = np.full((nq, k), -1, np.int32)
    d2 = np.full((nq, k), np.inf, np.float64)
    tx, ty, tz = t[None, :, 0].copy(), t[None, :, 1].copy(), t[None, :, 2].copy()
    with np.errstate(over="ignore"):
        for a in range(0, nq, chunk):
            b = min(nq, a + chunk)
            dx = q[a:b, None, 0] - tx
            dy = q[a:b, None, 1] - ty
            dz = q[a:b, None, 2] - tz
            d = ((dx * dx) + (dy * dy)) + (dz * dz)
            order = np.argsort(d, axis=1, kind="stable")
            if skip_self:
                order = order[order != np.arange(a, b)[:, None]].reshape(b - a, nt - 1)
            order = order[:, :k]
            w = order.shape[1]
            idx[a:b, :w] = order
            d2[a:b, :w] = np.take_along_axis(d, order, axis=1)
    return idx, d2


def rule_loops(index, dist2, sigma):
    """pais_cloud_outlier_rule, statement by statement -> (mean_dist list, (mu, sd, threshold), outlier list)"""
    n = len(index)
    nan = float("nan")
    mean, rows = [], True
    for i in range(n):
        s, ki = 0.0, 0
        for j in range(len(index[i])):
            if index[i][j] >= 0:
                s += math.sqrt(float(dist2[i][j]))
                ki += 1
        if ki == 0:
            rows = False
        mean.append(s / ki if ki else nan)
    total = 0.0
    for m in mean:
        total += m
    mu = total / n if n else nan
    ss = 0.0
    for m in mean:
        ss += (m - mu) * (m - mu)
    sd = math.sqrt(ss / (n - 1)) if n > 1 else nan
    threshold = mu + sigma * sd
    if n < 2 or not rows or not math.isfinite(mu) or not math.isfinite(sd):
        return mean, (mu, sd, threshold), [False] * n
    return mean, (mu, sd, threshold), [m > threshold for m in mean]


def same_doubles(got, want):
    """bit-equal, or both NaN (the sign and payload of a NaN are not part of the statement)"""
    got, want = np.asarray(got, np.float64).ravel(), np.asarray(want, np.float64).ravel()
    if got.shape != want.shape:
        return False
    return bool(np.all((got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))))


def assert_rule(res, index, dist2, sigma, what=""):
    """res: evaluate.outlier_rule / statistical_outliers output against rule_loops on the table"""
    mean, stats, out = rule_loops(index, dist2, sigma)
    assert same_doubles(res["mean_dist"], mean), (what, "mean_dist")
    assert same_doubles([res["mu"], res["sd"], res["threshold"]], stats), (what, res["mu"], res["sd"], res["threshold"], stats)
    assert res["outlier"].dtype == bool and res["outlier"].tolist() == out, (what, "mask")
    return mean, stats, out


PLANE_SEEDS = (0, 1, 2, 3, 4)
PLANE_K, PLANE_SIGMA, PLANE_ADDED = 8, 2.0, 12


def plane_case(seed):
    """576 points of a jittered 24 x 24 unit grid (+- 0.2 in the plane, sigma 0.05 off it) and 12 points 6 .. 12 units off the
    plane, shuffled -> (points (588, 3), added bool (588,))"""
    rng = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.arange(24.0), np.arange(24.0), indexing="ij")
    grid = np.stack([gx.ravel() + rng.uniform(-0.2, 0.2, 576), gy.ravel() + rng.uniform(-0.2, 0.2, 576), rng.normal(0.0, 0.05, 576)], axis=1)
    far = np.stack([rng.uniform(0.0, 23.0, PLANE_ADDED), rng.uniform(0.0, 23.0, PLANE_ADDED), rng.uniform(6.0, 12.0, PLANE_ADDED)], axis=1)
    pts = np.concatenate([grid, far])
    added = np.arange(len(pts)) >= 576
    perm = rng.permutation(len(pts))
    return np.ascontiguousarray(pts[perm]), added[perm]
