"""pais_cloud_nearest on the MI355X against a numpy brute force of its three statements -- every index equal, every squared
distance bit-equal, whatever the split into slices and chunks -- and the scores of a reconstruction end to end.

The brute force is chunked over the queries so that its (chunk x nt) temporaries stay small; numpy evaluates each statement
as its own rounded elementwise pass (no FMA), and np.argmin returns the first minimum."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _brute(q, t, chunk=64):
    q, t = np.ascontiguousarray(q, np.float64), np.ascontiguousarray(t, np.float64)
    idx, d2 = np.empty(len(q), np.int32), np.empty(len(q), np.float64)
    tx, ty, tz = t[None, :, 0].copy(), t[None, :, 1].copy(), t[None, :, 2].copy()
    for a in range(0, len(q), chunk):
        b = min(len(q), a + chunk)
        dx = q[a:b, None, 0] - tx
        dy = q[a:b, None, 1] - ty
        dz = q[a:b, None, 2] - tz
        d = ((dx * dx) + (dy * dy)) + (dz * dz)
        j = np.argmin(d, axis=1)
        idx[a:b] = j
        d2[a:b] = d[np.arange(b - a), j]
    return idx, d2


def _same(got, want, what):
    gi, gd = got[0], got[1]
    wi, wd = want
    assert gi.dtype == np.int32 and gd.dtype == np.float64 and gi.shape == wi.shape and gd.shape == wd.shape, what
    bad = np.nonzero((gi != wi) | (gd.view(np.uint64) != wd.view(np.uint64)))[0]
    assert not len(bad), (what, len(bad), bad[:5], gi[bad[:5]], wi[bad[:5]], gd[bad[:5]], wd[bad[:5]])


def test_nearest_equals_the_brute_force_bit_for_bit():
    from pais_mvs_amd import evaluate
    rng = np.random.default_rng(77)
    # sizes that are no multiple of the block (256) or the tile (512)
    for nq, nt in ((1, 1), (257, 513), (1000, 3001), (63, 511), (300, 1)):
        q, t = rng.normal(size=(nq, 3)), rng.normal(size=(nt, 3))
        _same(evaluate.nearest(q, t), _brute(q, t), ("random", nq, nt))
    # duplicated targets: the tie goes to the lowest index, across tiles and slices as well
    base = rng.normal(size=(700, 3))
    t = np.concatenate([base, base[::-1], base])             # every target three times, 2100 targets
    q = base[rng.permutation(700)[:333]] + rng.normal(size=(333, 3)) * 1e-3
    got = evaluate.nearest(q, t)
    _same(got, _brute(q, t), "duplicates")
    assert (got[0] < 700).all()
    # queries equal to targets: d2 == 0 at the first copy
    got = evaluate.nearest(base, t)
    _same(got, _brute(base, t), "self")
    assert not got[1].any() and np.array_equal(got[0], np.arange(700, dtype=np.int32))
    # all targets equal: index 0 everywhere
    same_t = np.repeat(rng.normal(size=(1, 3)), 1500, axis=0)
    got = evaluate.nearest(q, same_t)
    _same(got, _brute(q, same_t), "one point many times")
    assert not got[0].any()
    # coordinates near 1e3, differences near 1e-9: the difference form keeps them, the norm expansion would not
    t = 1e3 + rng.uniform(-1.0, 1.0, size=(2500, 3))
    q = t[rng.permutation(2500)[:900]] + rng.normal(size=(900, 3)) * 1e-9
    got = evaluate.nearest(q, t)
    _same(got, _brute(q, t), "1e3 / 1e-9")
    assert 0 < np.sqrt(got[1]).max() < 1e-7
    # distances that overflow to +inf are still ordered as a sequential scan orders them: the first target
    big_t = np.full((600, 3), 1e200)
    big_q = np.full((3, 3), -1e200)
    got = evaluate.nearest(big_q, big_t)
    _same(got, _brute(big_q, big_t), "overflow")
    assert np.isinf(got[1]).all() and not got[0].any()


def test_result_does_not_depend_on_slices_or_chunks(monkeypatch):
    """One case large enough for many slices and several chunks; the bytes with 1 slice, the default split, the maximum slice
    count and with small chunks are those of the brute force."""
    from pais_mvs_amd import _lib, evaluate
    L = _lib.load()
    rng = np.random.default_rng(78)
    nq, nt = 3000, 32763                                      # 64 tiles of 512: up to 64 slices of one tile
    t = rng.normal(size=(nt, 3))
    t[20000:20500] = t[100:600]                               # ties between far-apart slices
    q = np.concatenate([rng.normal(size=(nq - 500, 3)), t[20000:20500] + rng.normal(size=(500, 3)) * 1e-6])
    want = _brute(q, t)
    monkeypatch.delenv("PAIS_CLOUD_SLICES", raising=False)
    monkeypatch.delenv("PAIS_CLOUD_CHUNK", raising=False)
    runs = {}
    for name, slices, chunk in (("default", None, None), ("one slice", 1, None), ("max slices", 64, None), ("beyond max", 1000, None),
                                ("chunks", None, 1000), ("chunks, max slices", 64, 700), ("chunks, one slice", 1, 256)):
        for k, v in (("PAIS_CLOUD_SLICES", slices), ("PAIS_CLOUD_CHUNK", chunk)):
            if v is None:
                monkeypatch.delenv(k, raising=False)
            else:
                monkeypatch.setenv(k, str(v))
        before = L.pais_cloud_launches()
        got = evaluate.nearest(q, t)
        passes = -(-nq // (chunk or nq))
        assert L.pais_cloud_launches() - before == 2 * passes, (name, L.pais_cloud_launches() - before, passes)
        assert got[2] > 0
        _same(got, want, name)
        runs[name] = got[0].tobytes() + got[1].tobytes()
    assert len(set(runs.values())) == 1
    assert (want[0][nq - 500:] < 20000).all()                # the ties went to the first copy


def test_bad_arguments_are_refused_without_a_launch():
    from pais_mvs_amd import _lib
    L = _lib.load()
    q, t = np.zeros((4, 3)), np.ones((5, 3))
    idx, d2 = np.zeros(4, np.int32), np.zeros(4)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ip = idx.ctypes.data_as(C.POINTER(C.c_int32))
    nan, inf = q.copy(), t.copy()
    nan[3, 2] = float("nan")
    inf[0, 1] = float("inf")
    before = L.pais_cloud_launches()
    for args, msg in [((0, 4, dp(q), 0, dp(t), ip, dp(d2), None), "nt == 0"),
                      ((0, -4, dp(q), 5, dp(t), ip, dp(d2), None), "negative count"),
                      ((0, 4, dp(q), -1, dp(t), ip, dp(d2), None), "negative count"),
                      ((0, 4, None, 5, dp(t), ip, dp(d2), None), "null pointer"),
                      ((0, 4, dp(q), 5, dp(t), ip, None, None), "null pointer"),
                      ((0, 4, dp(nan), 5, dp(t), ip, dp(d2), None), "queries[3] coordinate 2 is not finite"),
                      ((0, 4, dp(q), 5, dp(inf), ip, dp(d2), None), "targets[0] coordinate 1 is not finite")]:
        rc = L.pais_cloud_nearest(*args)
        err = L.pais_cloud_last_error().decode()
        assert rc < 0 and err and msg in err, (rc, err, msg)
    assert L.pais_cloud_nearest(0, 0, None, 0, None, None, None, None) == 0
    assert L.pais_cloud_nearest(0, 0, dp(q), 5, dp(t), ip, dp(d2), None) == 0
    assert L.pais_cloud_launches() == before and not idx.any() and not d2.any()
    ms = C.c_double(-1)
    assert L.pais_cloud_nearest(0, 4, dp(q), 5, dp(t), ip, dp(d2), C.byref(ms)) == 0
    assert L.pais_cloud_launches() == before + 2 and ms.value > 0 and list(d2) == [3.0] * 4 and not idx.any()


B, ROUNDS = 16, 6


@pytest.fixture(scope="module")
def pawn_recon(pawn_small):
    """a bounded reconstruction of the small pawn scene, its driver still open, and the scene's ground truth"""
    from pais_mvs_amd import synth
    from pais_mvs_amd.config import readme_config
    from pais_mvs_amd.mvs import MVS
    m = MVS(readme_config(), pawn_small.cameras, device=0, seed=42)
    for X, vis in pawn_small.seeds:
        m.add_seed(X, vis)
    m.refineSeedPatches()
    m.expansionPatches(B, ROUNDS)
    pts, nrm, spacing = synth.ground_truth(pawn_small)
    yield m, np.concatenate([pts, nrm], axis=1), spacing
    m.close()


def test_score_of_a_reconstruction_equals_the_host_arithmetic_on_brute_force_matches(pawn_recon):
    from pais_mvs_amd import evaluate
    m, truth, spacing = pawn_recon
    cloud = m.cloud()
    assert len(cloud) >= 100 and len(truth) >= 5000
    got = m.score(truth, 2 * spacing)
    i_ct, d_ct = _brute(cloud[:, :3], truth[:, :3])
    i_tc, d_tc = _brute(truth[:, :3], cloud[:, :3])
    want = evaluate.score_from_matches(cloud, truth, i_ct, d_ct, i_tc, d_tc, 2 * spacing)
    print("\npawn_small, %d rounds of %d parents: %s" % (ROUNDS, B, got))
    assert set(got) == set(want) | set(evaluate.TIMING_KEYS)
    for k, v in want.items():
        assert type(got[k]) is type(v) and np.float64(got[k]).view(np.uint64) == np.float64(v).view(np.uint64), (k, got[k], v)
    assert all(got[k] > 0 for k in evaluate.TIMING_KEYS)
    assert got["n"] == len(cloud) and got["m"] == len(truth) and got["threshold"] == 2 * spacing
    assert 0 < got["accuracy_plane"] <= got["accuracy"] and 0 < got["completeness"] < 1


def test_truth_against_itself_is_perfect(pawn_recon):
    from pais_mvs_amd import evaluate
    _m, truth, spacing = pawn_recon
    s = evaluate.score(truth, truth, 2 * spacing, fraction=1.0)
    assert s["accuracy"] == 0.0 and s["accuracy_plane"] == 0.0 and s["completeness"] == 1.0
    assert s["cloud_to_truth_max"] == 0.0 and s["truth_to_cloud_max"] == 0.0 and s["flipped_normals"] == 0
    assert s["normal_angle_p90_rad"] < 1e-7         # arccos of a unit normal's dot with itself, within rounding of 1


def test_a_cloud_moved_along_its_normals_scores_worse_by_the_shift(pawn_recon):
    """Every patch moved by delta = 4 spacing along its own normal: the plane-distance order statistic grows by at least
    delta / 2, because the cosine between an unflipped patch normal and the truth normal next to it is above 0.5."""
    from pais_mvs_amd import evaluate
    m, truth, spacing = pawn_recon
    cloud = m.cloud()
    base = evaluate.score(cloud, truth, 2 * spacing)
    assert base["flipped_normals"] == 0
    delta = 4 * spacing
    moved = cloud.copy()
    moved[:, :3] += delta * moved[:, 3:]
    far = evaluate.score(moved, truth, 2 * spacing)
    print("\nplane-distance statistic %.6g -> %.6g (delta %.6g); accuracy %.6g -> %.6g; completeness %.4f -> %.4f"
          % (base["accuracy_plane"], far["accuracy_plane"], delta, base["accuracy"], far["accuracy"], base["completeness"], far["completeness"]))
    assert far["accuracy_plane"] - base["accuracy_plane"] >= delta / 2
    assert far["accuracy"] > base["accuracy"] and far["completeness"] <= base["completeness"]
