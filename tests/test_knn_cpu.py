"""The k-nearest feature without a GPU: the host statement of the statistical outlier rule (pais_cloud_outlier_rule) against
its restatement in Python loops on brute-force neighbour tables, the rule doing its job on a plane with far points, and every
refusal of pais_cloud_knn / pais_mvs_statistical_filtering that happens before anything is launched."""
import ctypes as C

import numpy as np
import pytest

from tests import knn_ref


def _rule_on(points, k, sigma, what):
    from pais_mvs_amd import evaluate
    idx, d2 = knn_ref.brute_knn(points, points, k, skip_self=True)
    res = evaluate.outlier_rule(idx, d2, sigma)
    return res, knn_ref.assert_rule(res, idx, d2, sigma, what)


def test_outlier_rule_equals_the_loop_restatement_bit_for_bit():
    from pais_mvs_amd import evaluate
    rng = np.random.default_rng(5)
    for n in (2, 3, 300):                                    # 2 and 3: rows padded with -1 / +inf (n - 1 < k)
        pts = rng.normal(size=(n, 3))
        pts[-1] += 4.0
        res, (_, _, out) = _rule_on(pts, 8, 1.0, ("random", n))
        assert len(res["outlier"]) == n
        if n == 300:
            assert 0 < sum(out) < n // 4
    idx, d2 = knn_ref.brute_knn(pts, pts, 8, skip_self=True)
    # duplicates: nine copies of one point give those rows eight zeros
    dup = pts.copy()
    dup[10:19] = dup[10]
    res, (mean, _, _) = _rule_on(dup, 8, 2.0, "duplicates")
    assert mean[10] == 0.0 and mean[18] == 0.0 and np.isfinite(res["threshold"])
    # a +inf distance makes mu infinite: nothing is flagged
    inf_d2 = d2.copy()
    inf_d2[7, 7] = np.inf
    res = evaluate.outlier_rule(idx, inf_d2, 1.0)
    knn_ref.assert_rule(res, idx, inf_d2, 1.0, "+inf")
    assert np.isinf(res["mu"]) and not res["outlier"].any()
    big = np.concatenate([np.full((5, 3), 1e200), np.full((5, 3), -1e200)])   # overflowing distances from the search itself
    res, _ = _rule_on(big, 8, 1.0, "overflow")
    assert not res["outlier"].any()
    # a row without a valid entry: nothing is flagged either
    hole_i, hole_d = idx.copy(), d2.copy()
    hole_i[3], hole_d[3] = -1, np.inf
    res = evaluate.outlier_rule(hole_i, hole_d, 1.0)
    knn_ref.assert_rule(res, hole_i, hole_d, 1.0, "empty row")
    assert np.isnan(res["mean_dist"][3]) and not res["outlier"].any()
    # n = 1 (its row is all padding) and n = 0
    res, _ = _rule_on(pts[:1], 8, 2.0, "n = 1")
    assert res["outlier"].tolist() == [False]
    res = evaluate.outlier_rule(np.zeros((0, 8), np.int32), np.zeros((0, 8)), 2.0)
    assert len(res["outlier"]) == 0 and len(res["mean_dist"]) == 0 and np.isnan(res["mu"]) and np.isnan(res["sd"]) and np.isnan(res["threshold"])


@pytest.mark.parametrize("seed", knn_ref.PLANE_SEEDS)
def test_rule_flags_the_points_off_a_plane_and_nothing_else(seed):
    pts, added = knn_ref.plane_case(seed)
    res, (mean, stats, out) = _rule_on(pts, knn_ref.PLANE_K, knn_ref.PLANE_SIGMA, ("plane", seed))
    mean = np.array(mean)
    print("\nseed %d: added m_i >= %.3f, grid m_i <= %.3f, mu %.4f sd %.4f threshold %.4f"
          % (seed, mean[added].min(), mean[~added].max(), *stats))
    assert added.sum() == knn_ref.PLANE_ADDED and len(pts) == 588
    assert res["outlier"][added].all(), "an added point survived"
    assert not res["outlier"][~added].any(), "a grid point was flagged"


def test_rule_refuses_bad_arguments():
    from pais_mvs_amd import _lib
    L = _lib.load()
    idx, d2 = np.zeros((4, 2), np.int32), np.ones((4, 2))
    mean, stats, out = np.zeros(4), np.zeros(3), np.zeros(4, np.uint8)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ip, op = idx.ctypes.data_as(C.POINTER(C.c_int32)), out.ctypes.data_as(C.POINTER(C.c_uint8))
    for args in ((-1, 2, ip, dp(d2), 2.0, dp(mean), dp(stats), op), (4, 0, ip, dp(d2), 2.0, dp(mean), dp(stats), op),
                 (4, 2, None, dp(d2), 2.0, dp(mean), dp(stats), op), (4, 2, ip, dp(d2), 2.0, dp(mean), None, op),
                 (0, 2, None, None, 2.0, None, None, None)):
        assert L.pais_cloud_outlier_rule(*args) < 0 and b"pais_cloud_outlier_rule" in L.pais_cloud_last_error()
    assert L.pais_cloud_outlier_rule(0, 2, None, None, 2.0, None, dp(stats), None) == 0
    assert L.pais_cloud_outlier_rule(4, 2, ip, dp(d2), 2.0, dp(mean), dp(stats), op) == 0 and list(mean) == [1.0] * 4


def test_knn_refusals_launch_nothing_and_touch_nothing():
    from pais_mvs_amd import _lib, evaluate
    L = _lib.load()
    K = 3
    q, t = np.zeros((4, 3)), np.ones((4, 3))
    idx, d2 = np.full((4, K), 77, np.int32), np.full((4, K), 77.0)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ip = idx.ctypes.data_as(C.POINTER(C.c_int32))
    nan, inf = q.copy(), t.copy()
    nan[3, 2] = float("nan")
    inf[0, 1] = float("-inf")
    SKIP = _lib.KNN_SKIP_SAME_INDEX
    assert _lib.CLOUD_MAX_K == 32 and SKIP == 1
    before = L.pais_cloud_launches()
    for args, msg in [((0, 0, 0, 4, dp(q), 4, dp(t), ip, dp(d2), None), "k = 0"),
                      ((0, 0, -1, 4, dp(q), 4, dp(t), ip, dp(d2), None), "k = -1"),
                      ((0, 0, 33, 4, dp(q), 4, dp(t), ip, dp(d2), None), "k = 33"),
                      ((0, 2, K, 4, dp(q), 4, dp(t), ip, dp(d2), None), "unknown flag bits"),
                      ((0, -1, K, 4, dp(q), 4, dp(t), ip, dp(d2), None), "unknown flag bits"),
                      ((0, SKIP, K, 3, dp(q), 4, dp(t), ip, dp(d2), None), "nq != nt"),
                      ((0, SKIP, K, 0, dp(q), 4, dp(t), ip, dp(d2), None), "nq != nt"),
                      ((0, 0, K, -4, dp(q), 4, dp(t), ip, dp(d2), None), "negative count"),
                      ((0, 0, K, 4, dp(q), -1, dp(t), ip, dp(d2), None), "negative count"),
                      ((0, 0, K, 4, None, 4, dp(t), ip, dp(d2), None), "null pointer"),
                      ((0, 0, K, 4, dp(q), 4, None, ip, dp(d2), None), "null pointer"),
                      ((0, 0, K, 4, dp(q), 4, dp(t), None, dp(d2), None), "null pointer"),
                      ((0, 0, K, 4, dp(q), 4, dp(t), ip, None, None), "null pointer"),
                      ((0, 0, K, 4, dp(q), 0, dp(t), ip, dp(d2), None), "nt == 0"),
                      ((-1, 0, K, 4, dp(q), 4, dp(t), ip, dp(d2), None), "device < 0"),
                      ((-1, SKIP, K, 4, dp(q), 4, dp(q), ip, dp(d2), None), "device < 0"),
                      ((0, 0, K, 4, dp(nan), 4, dp(t), ip, dp(d2), None), "queries[3] coordinate 2 is not finite"),
                      ((0, SKIP, K, 4, dp(q), 4, dp(inf), ip, dp(d2), None), "targets[0] coordinate 1 is not finite")]:
        rc = L.pais_cloud_knn(*args)
        err = L.pais_cloud_last_error().decode()
        assert rc < 0 and err.startswith("pais_cloud_knn:") and msg in err, (rc, err, msg)
    # nq == 0 is no error and touches nothing
    assert L.pais_cloud_knn(0, 0, K, 0, None, 0, None, None, None, None) == 0
    assert L.pais_cloud_knn(-1, 0, K, 0, dp(q), 4, dp(t), ip, dp(d2), None) == 0
    assert L.pais_cloud_knn(0, SKIP, K, 0, None, 0, None, None, None, None) == 0
    assert L.pais_cloud_launches() == before and (idx == 77).all() and (d2 == 77.0).all()
    # the Python entries raise on the same refusals
    for call in (lambda: evaluate.knn(q, t, 33, device=-1), lambda: evaluate.knn(q, t[:3], 2, skip_self=True, device=-1),
                 lambda: evaluate.knn(q, t, 2, device=-1), lambda: evaluate.spacing(q, device=-1),
                 lambda: evaluate.statistical_outliers(q, device=-1)):
        with pytest.raises(RuntimeError, match="pais_cloud_knn"):
            call()
    with pytest.raises(ValueError):
        evaluate.knn(np.zeros((4, 2)), t, 2, device=-1)
    with pytest.raises(ValueError):
        evaluate.spacing(q[:1], device=-1)
    assert L.pais_cloud_launches() == before


def test_statistical_filtering_without_a_gpu_context_fails_loudly(pawn_small):
    from pais_mvs_amd.config import readme_config
    from pais_mvs_amd.mvs import MVS
    m = MVS(readme_config(), pawn_small.cameras, device=-1, seed=42)
    with pytest.raises(RuntimeError, match="no GPU context"):
        m.statisticalFiltering(8, 2.0)
    m.close()


def test_command_lines_know_the_new_flags(tmp_path, capsys):
    from pais_mvs_amd import evaluate, reconstruct
    assert reconstruct.parse_statistical("8,2") == (8, 2.0) and reconstruct.parse_statistical("16,1.5") == (16, 1.5)
    for bad in (["cloud.mvs", "--filter", "--statistical", "8"], ["cloud.mvs", "--filter", "--statistical", "a,b"],
                ["scene.nvm", "--statistical", "8,2"]):
        with pytest.raises(SystemExit):
            reconstruct.main(bad)
    with pytest.raises(SystemExit):
        evaluate.main(["--spacing"])
    with pytest.raises(SystemExit):
        evaluate.main([str(tmp_path / "cloud.npy")])                      # no --truth: still required without --spacing
    capsys.readouterr()
