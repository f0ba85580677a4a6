"""Scoring a cloud against ground truth, the parts that need no GPU: the ground-truth sampler of the synthetic scenes
(synth.ground_truth), the host arithmetic of the scores (evaluate.score_from_matches) on nearest neighbours supplied by numpy,
the file readers of the command line, and the refusals of pais_cloud_nearest that happen before anything is launched."""
import ctypes as C
import math

import numpy as np
import pytest


def _brute(q, t):
    """nearest target of every query by the three statements of include/pais_cloud.h; np.argmin returns the first minimum"""
    dx, dy, dz = (q[:, None, k] - t[None, :, k] for k in range(3))
    d = ((dx * dx) + (dy * dy)) + (dz * dz)
    j = np.argmin(d, axis=1)
    return j.astype(np.int32), d[np.arange(len(q)), j]


# --------------------------------------------------------------------------------------------------- ground truth ---
def test_ground_truth_of_the_small_pawn_scene(pawn_small):
    """Measured on the 320 x 240 pawn rig (stride 2, min_views 3): 5922 samples kept of 7433 raw hits; the rig's middle camera
    (index 2) keeps 1219 of its 1483 raw hits, a share of 0.822 -- half of that, 0.41, is asserted, so that the sampler cannot
    hide an empty or nearly empty result."""
    from pais_mvs_amd import synth
    min_views = 3
    s = synth.ground_truth_samples(pawn_small, stride=2, min_views=min_views)
    pts, nrm, spacing = synth.ground_truth(pawn_small, stride=2, min_views=min_views)
    assert np.array_equal(pts, s["points"]) and np.array_equal(nrm, s["normals"]) and spacing == float(np.median(s["pitch"]))
    m = len(pts)
    assert pts.shape == (m, 3) and nrm.shape == (m, 3) and s["part"].shape == (m,)
    mid = len(pawn_small.cameras) // 2
    share = s["kept"][mid] / s["raw_hits"][mid]
    print("\nground truth: %d samples, raw %s kept %s, middle-camera share %.3f, spacing %.6g" % (m, s["raw_hits"], s["kept"], share, spacing))
    assert s["raw_hits"][mid] > 1000 and share >= 0.41, (s["raw_hits"], s["kept"])
    assert m == sum(s["kept"]) and spacing > 0
    # every sample lies on the part it was hit on
    q = pawn_small.obj.part_coords(pts, s["part"])
    assert np.abs(np.einsum("ij,ij->i", q, q) - 1.0).max() <= 1e-9
    assert set(np.unique(s["part"])) <= set(range(len(pawn_small.obj.parts))) and len(np.unique(s["part"])) >= 2
    # the normal is the analytic one of that part (the gradient of q.q in the world frame), unit length
    assert np.abs(np.linalg.norm(nrm, axis=1) - 1.0).max() <= 1e-12
    r = np.array([[e.rxy, e.rxy, e.rz] for e in pawn_small.obj.parts])[s["part"]]
    grad = (q / r) @ pawn_small.obj.frame()
    grad /= np.linalg.norm(grad, axis=1, keepdims=True)
    assert np.abs(grad - nrm).max() <= 1e-12
    # ... and points towards at least min_views camera centres
    towards = np.zeros(m, dtype=int)
    for c in pawn_small.cameras:
        towards += np.einsum("ij,ij->i", c.center[None, :] - pts, nrm) > 0
    assert towards.min() >= min_views
    # the scalar visibility test the seeds are made with agrees on a fixed random subset
    for i in np.random.default_rng(20240).choice(m, 200, replace=False):
        vis = synth._visible_cams(pawn_small.obj, pts[i], nrm[i], pawn_small.cameras)
        assert len(vis) >= min_views, (i, vis)
    # the pitch is that of the camera whose ray hit: stride * depth / focal
    i = int(np.argmax(s["pitch"]))
    cam = pawn_small.cameras[int(s["camera"][i])]
    depth = (cam.rotation @ pts[i] + cam.translation)[2]
    assert abs(s["pitch"][i] - 2 * depth / cam.focal[0]) <= 1e-12
    # a denser sampling and a stricter view test move the result the way they must
    assert len(synth.ground_truth(pawn_small, stride=4)[0]) < m
    assert len(synth.ground_truth(pawn_small, stride=2, min_views=5)[0]) < m


def test_intersect_parts_is_intersect_with_the_part(pawn_small):
    obj, cam = pawn_small.obj, pawn_small.cameras[0]
    rng = np.random.default_rng(5)
    dirs = (np.stack([rng.uniform(-0.3, 0.3, 4000), rng.uniform(-0.3, 0.3, 4000), np.ones(4000)], axis=1)) @ cam.rotation
    t, part = obj.intersect_parts(cam.center, dirs)
    assert np.array_equal(t, obj.intersect(cam.center, dirs))
    hit = np.isfinite(t)
    assert hit.sum() > 100 and (~hit).sum() > 100 and (part[~hit] == -1).all() and (part[hit] >= 0).all()
    X = cam.center + t[hit, None] * dirs[hit]
    q = obj.part_coords(X, part[hit])
    assert np.abs(np.einsum("ij,ij->i", q, q) - 1.0).max() <= 1e-9


# ----------------------------------------------------------------------------------------------- score arithmetic ---
def _plane_case():
    """truth: the 10 x 10 unit grid of the plane z = 0, normals +z.  cloud: 10 points above the grid points (i, 0) at the
    heights (i + 1) / 64 (exact in binary, so every distance is exact), normals +z."""
    gx, gy = np.meshgrid(np.arange(10.0), np.arange(10.0), indexing="ij")
    truth = np.zeros((100, 6))
    truth[:, 0], truth[:, 1], truth[:, 5] = gx.ravel(), gy.ravel(), 1.0
    cloud = np.zeros((10, 6))
    cloud[:, 0], cloud[:, 2], cloud[:, 5] = np.arange(10.0), (np.arange(10.0) + 1) / 64, 1.0
    return cloud, truth


def test_order_statistics_and_completeness_on_a_plane():
    from pais_mvs_amd import evaluate
    cloud, truth = _plane_case()
    i_ct, d_ct = _brute(cloud[:, :3], truth[:, :3])
    i_tc, d_tc = _brute(truth[:, :3], cloud[:, :3])
    assert list(i_ct) == [10 * i for i in range(10)] and list(d_ct) == [((i + 1) / 64) ** 2 for i in range(10)]
    assert [evaluate.order_index(f, 10) for f in (0.9, 1.0, 0.05, 0.1, 0.11, 1e-9)] == [8, 9, 0, 0, 1, 0]
    s = evaluate.score_from_matches(cloud, truth, i_ct, d_ct, i_tc, d_tc, threshold=1.0, fraction=0.9)
    assert s["accuracy"] == 9 / 64 == s["accuracy_plane"] and s["n"] == 10 and s["m"] == 100 and s["threshold"] == 1.0
    assert s["cloud_to_truth_max"] == 10 / 64 and s["cloud_to_truth_median"] == 5.5 / 64
    assert s["flipped_normals"] == 0 and s["normal_angle_p90_rad"] == 0.0
    s1 = evaluate.score_from_matches(cloud, truth, i_ct, d_ct, i_tc, d_tc, threshold=1.0, fraction=1.0)
    assert s1["accuracy"] == 10 / 64 == s1["accuracy_plane"]
    # completeness: the row y = 0 lies under the cloud (distance <= 10/64), the row y = 1 at sqrt(1 + h^2) > 1, ...
    assert s["completeness"] == 10 / 100
    assert s["truth_to_cloud_max"] == math.sqrt(81.0 + (10 / 64) ** 2)      # the sample (9, 9) under the highest cloud point
    # a distance exactly equal to the threshold is counted in; one ulp below it is not
    j = 10 * 3 + 1                       # truth sample (3, 1): nearest cloud point (3, 0, 4/64)
    thr = float(np.sqrt(d_tc[j]))
    assert thr == math.sqrt(1.0 + (4 / 64) ** 2)
    inside = int(np.count_nonzero(np.sqrt(d_tc) <= thr))
    assert inside == 10 + 4              # the row y = 0 and the samples (0..3, 1)
    at = evaluate.score_from_matches(cloud, truth, i_ct, d_ct, i_tc, d_tc, threshold=thr)
    below = evaluate.score_from_matches(cloud, truth, i_ct, d_ct, i_tc, d_tc, threshold=float(np.nextafter(thr, 0.0)))
    assert at["completeness"] == 14 / 100 and below["completeness"] == 13 / 100
    # flipped normals are counted and are 180 degrees off
    flipped = cloud.copy()
    flipped[:2, 5] = -1.0
    f = evaluate.score_from_matches(flipped, truth, i_ct, d_ct, i_tc, d_tc, threshold=1.0)
    assert f["flipped_normals"] == 2 and f["normal_angle_p90_rad"] == math.pi
    assert evaluate.score_from_matches(flipped[2:], truth, i_ct[2:], d_ct[2:], i_tc, d_tc, threshold=1.0)["normal_angle_p90_rad"] == 0.0
    with pytest.raises(ValueError):
        evaluate.score_from_matches(cloud[:0], truth, i_ct[:0], d_ct[:0], i_tc, d_tc, threshold=1.0)
    with pytest.raises(ValueError):
        evaluate.score_from_matches(cloud, truth, i_ct, d_ct, i_tc, d_tc, threshold=1.0, fraction=0.0)


def test_plane_distance_uses_the_truth_normal():
    from pais_mvs_amd import evaluate
    truth = np.array([[0.0, 0.0, 0.0, 0.6, 0.0, 0.8]])
    cloud = np.array([[1.0, 0.0, 1.0, 0.0, 0.0, 1.0], [0.0, 3.0, 0.0, 0.6, 0.0, 0.8]])
    i_ct, d_ct = _brute(cloud[:, :3], truth[:, :3])
    i_tc, d_tc = _brute(truth[:, :3], cloud[:, :3])
    s = evaluate.score_from_matches(cloud, truth, i_ct, d_ct, i_tc, d_tc, threshold=1.5, fraction=1.0)
    assert s["accuracy_plane"] == 0.6 * 1.0 + 0.8 * 1.0           # |(p - g) . n_g| of the first point; the second lies in the plane
    assert s["accuracy"] == 3.0 and s["completeness"] == 1.0
    h = evaluate.score_from_matches(cloud, truth, i_ct, d_ct, i_tc, d_tc, threshold=1.0, fraction=0.5)
    assert h["accuracy_plane"] == 0.0 and h["accuracy"] == math.sqrt(2.0) and h["completeness"] == 0.0
    assert abs(s["normal_angle_p90_rad"] - math.acos(0.8)) < 1e-15


# ---------------------------------------------------------------------------------------------------------- files ---
def test_ply_reader_round_trips_the_librarys_writer(tmp_path):
    from pais_mvs_amd import evaluate, io
    rng = np.random.default_rng(3)
    cen = rng.normal(size=(37, 3)) * [1.0, 100.0, 1e-3]
    nor = rng.normal(size=(37, 3))
    nor /= np.linalg.norm(nor, axis=1, keepdims=True)
    path = str(tmp_path / "c.ply")
    io.write_ply(path, cen, nor, rng.integers(0, 256, size=(37, 3), dtype=np.uint8))
    got = evaluate.load_cloud(path)
    # the writer prints with the stream's default six significant digits
    want = np.array([[float("%g" % v) for v in row] for row in np.concatenate([cen, nor], axis=1)])
    assert got.shape == (37, 6) and np.array_equal(got, want)
    io.write_ply(path, cen[:0], nor[:0])
    assert evaluate.load_cloud(path).shape == (0, 6)
    (tmp_path / "bad.ply").write_text("ply\nformat binary_little_endian 1.0\nelement vertex 0\nend_header\n")
    with pytest.raises(IOError):
        evaluate.load_cloud(str(tmp_path / "bad.ply"))
    np.save(str(tmp_path / "c.npy"), want)
    assert np.array_equal(evaluate.load_cloud(str(tmp_path / "c.npy")), want)
    np.save(str(tmp_path / "bad.npy"), want[:, :3])
    with pytest.raises(IOError):
        evaluate.load_cloud(str(tmp_path / "bad.npy"))
    with pytest.raises(IOError):
        evaluate.load_cloud(str(tmp_path / "c.xyz"))


def test_mvs_file_yields_the_normals_of_the_loaded_patches(tmp_path, pawn_small):
    """evaluate.load_cloud(.mvs) == MVS.cloud() of a driver that loaded the same records (pais_mvs_load_patch, host only)."""
    from pais_mvs_amd import evaluate, io
    from pais_mvs_amd.config import readme_config
    from pais_mvs_amd.mvs import MVS
    cfg = readme_config()
    rng = np.random.default_rng(11)
    pats = []
    for X, vis in pawn_small.seeds:
        ns = [rng.uniform(0.0, math.pi), rng.uniform(-math.pi, math.pi)]
        pats.append(io.io_patch(X, ns, vis, rng.uniform(), rng.uniform()))
    m = MVS(cfg, pawn_small.cameras, device=-1, seed=42)
    path = str(tmp_path / "c.mvs")
    io.write_mvs(path, cfg, m._io_cameras(), pats)
    for p in io.load_mvs(path)[2]:
        m.load_patch(p.center[:], p.normalS[:], list(p.cam_idx[:p.num_cam]), p.fitness, p.correlation)
    want = m.cloud()
    m.close()
    got = evaluate.load_cloud(path)
    assert got.shape == want.shape == (len(pats), 6) and got.tobytes() == want.tobytes()


def test_write_truth_for_writes_the_samplers_points(tmp_path, capsys):
    import json
    from pais_mvs_amd import evaluate, synth
    kw = {"width": 160, "height": 120, "n_seeds": 0, "build_edges": False}
    out = str(tmp_path / "truth.npy")
    assert evaluate.main(["--write-truth-for", "pawn", "--truth", out, "--stride", "3", "--scene-kwargs", json.dumps(kw)]) == 0
    rep = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    pts, nrm, spacing = synth.ground_truth(synth.pawn_scene(**kw), stride=3)
    got = evaluate.load_cloud(out)
    assert rep["m"] == len(pts) > 100 and rep["spacing"] == spacing
    assert np.array_equal(got[:, :3], pts) and np.array_equal(got[:, 3:], nrm)


# ------------------------------------------------------------------------------------- refusals (nothing is launched) ---
def test_nearest_refuses_bad_input_and_a_missing_gpu_before_any_launch():
    from pais_mvs_amd import _lib, evaluate
    L = _lib.load()
    q = np.zeros((4, 3))
    t = np.ones((5, 3))
    idx = np.zeros(4, np.int32)
    d2 = np.zeros(4)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ip = idx.ctypes.data_as(C.POINTER(C.c_int32))
    before = L.pais_cloud_launches()
    nan, inf = q.copy(), t.copy()
    nan[2, 1] = float("nan")
    inf[4, 0] = float("-inf")
    for args, msg in [((0, 4, dp(q), 0, dp(t), ip, dp(d2), None), "nt == 0"),
                      ((0, -1, dp(q), 5, dp(t), ip, dp(d2), None), "negative count"),
                      ((0, 4, dp(q), -5, dp(t), ip, dp(d2), None), "negative count"),
                      ((0, 4, None, 5, dp(t), ip, dp(d2), None), "null pointer"),
                      ((0, 4, dp(q), 5, None, ip, dp(d2), None), "null pointer"),
                      ((0, 4, dp(q), 5, dp(t), None, dp(d2), None), "null pointer"),
                      ((0, 4, dp(q), 5, dp(t), ip, None, None), "null pointer"),
                      ((-1, 4, dp(q), 5, dp(t), ip, dp(d2), None), "needs a GPU"),
                      ((0, 4, dp(nan), 5, dp(t), ip, dp(d2), None), "queries[2] coordinate 1 is not finite"),
                      ((0, 4, dp(q), 5, dp(inf), ip, dp(d2), None), "targets[4] coordinate 0 is not finite")]:
        rc = L.pais_cloud_nearest(*args)
        err = L.pais_cloud_last_error().decode()
        assert rc < 0 and "pais_cloud_nearest" in err and msg in err, (rc, err, msg)
    assert L.pais_cloud_nearest(0, 0, None, 0, None, None, None, None) == 0
    assert L.pais_cloud_nearest(-1, 0, dp(q), 5, dp(t), ip, dp(d2), None) == 0
    assert L.pais_cloud_launches() == before and not idx.any() and not d2.any()
    # the Python surface fails as loudly: no CPU fallback
    with pytest.raises(RuntimeError, match="needs a GPU"):
        evaluate.nearest(q, t, device=-1)
    with pytest.raises(RuntimeError, match="needs a GPU"):
        evaluate.score(np.zeros((4, 6)), np.ones((5, 6)), threshold=1.0, device=-1)
    with pytest.raises(RuntimeError, match="not finite"):
        evaluate.nearest(nan, t)
    with pytest.raises(ValueError):
        evaluate.nearest(np.zeros((4, 2)), t)


def test_scheduler_only_driver_cannot_score(pawn_small):
    from pais_mvs_amd.config import readme_config
    from pais_mvs_amd.mvs import MVS
    m = MVS(readme_config(), pawn_small.cameras, device=-1, seed=42)
    X, vis = pawn_small.seeds[0]
    m.load_patch(X, [1.0, 0.5], vis, 0.0, 1.0)
    with pytest.raises(RuntimeError, match="needs a GPU"):
        m.score(np.ones((5, 6)), threshold=1.0)
    m.close()
