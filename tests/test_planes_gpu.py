"""pais_cloud_planes on the MI355X against the restatement of its definition with Python floats (tests/plane_ref.py) -- every
field of every record bit-equal, whatever the split into slices and passes -- and what is built on it: the normal-agreement
filter of the driver, estimate_normals, roughness and the two command lines."""
import copy
import json
import math
import os

import numpy as np
import pytest

from tests import knn_ref
from tests import plane_ref as pr
from tests.test_knn_gpu import _alive, _loaded, grown  # noqa: F401  (grown: fixture)

pytestmark = pytest.mark.gpu

SPLIT_ENV = ("PAIS_CLOUD_SLICES", "PAIS_CLOUD_CHUNK")


@pytest.fixture(autouse=True)
def _default_split(monkeypatch):
    for k in SPLIT_ENV:
        monkeypatch.delenv(k, raising=False)


def _record_bytes(r):
    return b"".join(np.ascontiguousarray(r[f]).tobytes() for f in pr.FIELDS + ("count", "status"))


@pytest.mark.parametrize("nq,nt,k,skip", pr.CASES + ((1, 1, 1, False), (1000, 3001, 16, False)))
def test_planes_equal_the_restatement_bit_for_bit(nq, nt, k, skip):
    """every list size of the search (1, 8, 16, 32), sizes that are no multiple of the 256-lane block or the 512-point tile, nt < k,
    m < 3 with and without the query"""
    from pais_mvs_amd import evaluate
    q, t = pr.case_points(nq, nt, k, skip)
    table = knn_ref.brute_knn(q, t, k, skip)
    for with_query in (False, True):
        got = evaluate.planes(q, k, targets=t, with_query=with_query, skip_self=skip)
        want, _ = pr.ref_planes(q, t, table[0], with_query)
        pr.assert_same_records(got, want, (nq, nt, k, skip, with_query))
        assert got["index"].tobytes() == table[0].tobytes() and got["dist2"].tobytes() == table[1].tobytes()
        assert got["kernel_ms"][0] > 0 and got["kernel_ms"][1] > 0
    if (nq, nt) in ((257, 513), (1000, 3001)):
        toward = np.random.default_rng(9).normal(size=(nq, 3))
        got = evaluate.planes(q, k, targets=t, toward=toward)
        pr.assert_same_records(got, pr.ref_planes(q, t, table[0], True, toward)[0], ("orient", nq))
        n = got["normal"]
        assert (((n[:, 0] * toward[:, 0]) + (n[:, 1] * toward[:, 1])) + (n[:, 2] * toward[:, 2]) >= 0).all()


def test_result_does_not_depend_on_slices_or_passes(monkeypatch):
    """700 points against themselves in passes of 256 (three passes, the last one partial): a fit that gathered from its pass
    instead of the whole set, or skipped its index in the pass, would show here"""
    from pais_mvs_amd import _lib, evaluate
    L = _lib.load()
    nq, nt, k, skip = 700, 700, 9, True
    q, t = pr.case_points(nq, nt, k, skip)
    want, _ = pr.ref_planes(q, t, knn_ref.brute_knn(q, t, k, skip)[0], True)
    runs = set()
    for slices in (1, 3, 64):
        for chunk in (256, 512):
            monkeypatch.setenv("PAIS_CLOUD_SLICES", str(slices))
            monkeypatch.setenv("PAIS_CLOUD_CHUNK", str(chunk))
            before = L.pais_cloud_launches()
            got = evaluate.planes(q, k)
            assert L.pais_cloud_launches() - before == 3 * -(-nq // chunk), (slices, chunk)     # search, merge and fit per pass
            pr.assert_same_records(got, want, (slices, chunk))
            runs.add(_record_bytes(got) + got["index"].tobytes() + got["dist2"].tobytes())
    assert len(runs) == 1


def test_the_returned_table_is_pais_cloud_knn_byte_for_byte():
    from pais_mvs_amd import evaluate
    rng = np.random.default_rng(31)
    q, t = rng.normal(size=(900, 3)), rng.normal(size=(2100, 3))
    for qq, tt, skip in ((q, t, False), (t, t, True)):
        idx, d2 = evaluate.knn(qq, tt, 12, skip_self=skip)
        got = evaluate.planes(qq, 12, targets=tt, skip_self=skip)
        assert got["index"].dtype == np.int32 and got["index"].tobytes() == idx.tobytes() and got["dist2"].tobytes() == d2.tobytes()
        bare = evaluate.planes(qq, 12, targets=tt, skip_self=skip, table=False)       # index = dist2 = NULL: nothing else changes
        assert "index" not in bare and _record_bytes(bare) == _record_bytes(got)


def test_anchors_and_degenerate_rows_on_the_device():
    from pais_mvs_amd import evaluate
    for axis in range(3):
        p = pr.anchor_points(axis)
        got = evaluate.planes(p, 8)
        pr.assert_same_records(got, pr.ref_planes(p, p, pr.self_table(p)[0], True)[0], ("anchor", axis))
        assert (got["eigen"][:, 0] == 0.0).all() and (got["normal"] == np.eye(3)[axis]).all() and (got["offset"] == 0.0).all()
        assert (got["centroid"][:, axis] == 0.5).all()
    for name, p in pr.degenerate_rows().items():
        got = evaluate.planes(p, 8)
        pr.assert_same_records(got, pr.ref_planes(p, p, pr.self_table(p)[0], True)[0], name)
        assert (got["status"] == pr.OK).all() and np.isfinite(got["eigen"]).all(), name
    p = pr.anchor_points(2)
    down = evaluate.planes(p, 8, toward=np.tile([0.0, 0.0, -1.0], (9, 1)))
    assert np.signbit(down["normal"]).all() and (down["normal"][:, 2] == -1.0).all()              # 0 components became -0.0


def test_refusals_launch_nothing_beside_a_device():
    from pais_mvs_amd import evaluate
    evaluate.planes(np.random.default_rng(1).normal(size=(9, 3)), 4)                               # the device is up
    pr.check_refusals()


@pytest.mark.parametrize("seed", knn_ref.PLANE_SEEDS)
def test_driver_filter_deletes_what_the_rule_predicts(pawn_small, seed):
    """a jittered plane with stored normal z, 20 grid patches tilted 60 degrees: with numpy eigh the fitted normal of every grid
    point lies within 6.4 degrees of z at k = 8, so at 30 degrees every tilted patch goes (60 - 6.4 > 30) and no untouched grid
    patch does (6.4 < 30); the 12 far points are not asserted either way"""
    from pais_mvs_amd.config import readme_config
    from pais_mvs_amd.mvs import MVS
    pts, added, ns, tilted = pr.tilted_case(seed)
    cfg = readme_config()
    m = _loaded(cfg, pawn_small.cameras, [(p.tolist(), s.tolist(), [], 0.5, 0.9) for p, s in zip(pts, ns)])
    ids = _alive(m)
    cloud = m.cloud()
    assert ids == list(range(len(pts))) and np.array_equal(cloud[:, :3], pts)
    stored = cloud[:, 3:]
    assert (stored[~tilted] == [0.0, 0.0, 1.0]).all() and np.allclose(stored[tilted, 2], 0.5, atol=1e-12)
    want_rec, _ = pr.ref_planes(pts, pts, knn_ref.brute_knn(pts, pts, 8, True)[0], True)
    pr.assert_same_records(m.planes(8), want_rec, ("driver planes", seed))
    flagged = np.array(pr.normal_rule_loop(want_rec["status"], want_rec["normal"], stored, math.cos(math.radians(30.0))))
    before = {i: bytes(m.get_patch(i)) for i in ids}
    removed, ms = m.normalFiltering(8, 30.0)
    gone = np.array([i not in set(_alive(m)) for i in ids])
    print("\nseed %d: %d removed (%d tilted, %d far), %.3f ms" % (seed, removed, (gone & tilted).sum(), (gone & added).sum(), ms))
    assert np.array_equal(gone, flagged) and removed == int(flagged.sum()) == len(pts) - m.num_patches() and ms > 0
    assert gone[tilted].all(), "a tilted patch survived"
    assert not gone[~tilted & ~added].any(), "an untouched grid patch was deleted"
    for i in _alive(m):
        assert bytes(m.get_patch(i)) == before[i], i
    m.close()
    host = MVS(cfg, pawn_small.cameras, device=-1, seed=42)
    with pytest.raises(RuntimeError, match="no GPU context"):
        host.normalFiltering(8, 30.0)
    host.close()


@pytest.fixture(scope="module")
def truth_points(pawn_small):
    from pais_mvs_amd import synth
    return np.ascontiguousarray(synth.ground_truth(pawn_small, stride=4)[0])


def test_estimate_normals(tmp_path, truth_points, pawn_small, capsys):
    from pais_mvs_amd import evaluate
    pts = truth_points
    eye = np.asarray(pawn_small.cameras[0].center, np.float64)
    cloud = evaluate.estimate_normals(pts, 16, viewpoint=eye)
    assert cloud.shape == (len(pts), 6) and np.array_equal(cloud[:, :3], pts) and len(pts) > 1000
    n, v = cloud[:, 3:], eye[None, :] - pts
    assert (((n[:, 0] * v[:, 0]) + (n[:, 1] * v[:, 1])) + (n[:, 2] * v[:, 2]) >= 0).all()
    assert np.abs(np.linalg.norm(n, axis=1) - 1.0).max() < 1e-14
    near = knn_ref.brute_knn(pts[:200], pts, 17)[0]                                  # the point itself is among its 17 nearest
    index = np.array([[j for j in row if j != i][:16] for i, row in enumerate(near)], np.int32)
    want = pr.ref_planes(pts[:200], pts, index, True, v[:200])[0]
    assert knn_ref.same_doubles(n[:200], want["normal"])
    # the normals are unit to a few DBL_EPSILON, not renormalised: n . n = 1 - e gives acos(1 - e) = sqrt(2 e) < 1e-7 for e < 20 eps
    s = evaluate.score(cloud, cloud, threshold=1.0)
    assert s["normal_angle_p90_rad"] < 1e-7 and s["flipped_normals"] == 0 and s["accuracy"] == 0.0 and s["accuracy_plane"] == 0.0
    # bare points through the command line to a PSR file (float32 x y z nx ny nz) and to .npy
    bare = str(tmp_path / "bare.npy")
    np.save(bare, pts)
    view = "--viewpoint=" + ",".join(repr(float(c)) for c in eye)       # with `=`: a negative X would read as an option
    assert evaluate.main([bare, "--estimate-normals", "16", view, "--out", str(tmp_path / "out.psr")]) == 0
    assert evaluate.main([bare, "--estimate-normals", "16", view, "--out", str(tmp_path / "out.npy")]) == 0
    capsys.readouterr()
    psr = np.fromfile(str(tmp_path / "out.psr"), dtype=np.float32).reshape(-1, 6)
    assert np.array_equal(psr, cloud.astype(np.float32)) and np.array_equal(np.load(str(tmp_path / "out.npy")), cloud)
    # without a viewpoint: the canonical sign
    plain = evaluate.estimate_normals(pts[:500], 16)[:, 3:]
    big = plain[np.arange(500), np.abs(plain).argmax(axis=1)]
    assert (big > 0).all()


@pytest.mark.parametrize("seed", knn_ref.PLANE_SEEDS)
def test_roughness_of_the_plane_case(seed):
    """the grid's points lie sigma = 0.05 off the plane; a fit over 17 of them absorbs part of that, and numpy's eigh gives
    0.030 .. 0.034 over the five seeds"""
    from pais_mvs_amd import evaluate
    pts, _ = knn_ref.plane_case(seed)
    want, _ = pr.ref_planes(pts, pts, knn_ref.brute_knn(pts, pts, 16, True)[0], True)
    off = np.sort(np.abs(want["offset"][want["status"] == pr.OK]))
    r = evaluate.roughness(pts)
    print("\nseed %d: roughness %.5f, spacing %.5f" % (seed, r, evaluate.spacing(pts)))
    assert r == float(off[-(-len(off) // 2) - 1]) and 0.005 < r < 0.05


def test_command_lines(tmp_path, pawn_small, grown, capsys):  # noqa: F811
    """--filter --normal-agreement K,DEG writes NA_filter.* with the driver's patch count after the other files, which it leaves
    as they are; evaluate --roughness prints roughness, spacing and their ratio"""
    from PIL import Image
    from pais_mvs_amd import evaluate, io, reconstruct
    cfg, cl = copy.copy(grown[0]), grown[1]
    cams = []
    for i, cam in enumerate(pawn_small.cameras):
        c = copy.copy(cam)
        c.name = "cam%d.png" % i
        Image.fromarray(np.repeat(cam.pyramid[0][:, :, None], 3, axis=2)).save(str(tmp_path / c.name))
        cams.append(c)
    m = _loaded(cfg, cams, cl)
    path = str(tmp_path / "cloud.mvs")
    m.writeMVS(path)
    m.close()
    a, b = tmp_path / "sor", tmp_path / "na"
    a.mkdir()
    b.mkdir()
    common = [path, "--filter", "--config", str(tmp_path / "none.txt"), "--statistical", "8,2"]
    reconstruct.main(common + ["--out", str(a)])
    reconstruct.main(common + ["--out", str(b), "--normal-agreement", "8,30"])
    today = {s + e for s in ("PMVS_filter1", "PMVS_filter2", "PMVS_filter3", "PCMVS_filter", "SOR_filter") for e in (".mvs", ".ply")}
    assert set(os.listdir(a)) == today and set(os.listdir(b)) == today | {"NA_filter.mvs", "NA_filter.ply"}
    for f in today:
        assert (a / f).read_bytes() == (b / f).read_bytes(), f
    # the same chain through the driver
    file_cfg, cams_io, pats = io.load_mvs(path)
    m = _loaded(file_cfg, reconstruct.load_cameras(cams_io, str(tmp_path), file_cfg),
                [(p.center[:], p.normalS[:], list(p.cam_idx[:p.num_cam]), p.fitness, p.correlation) for p in pats])
    m.cellFiltering(); m.visibilityFiltering(); m.neighborCellFiltering(0.25); m.neighborPatchFiltering(0.25)
    m.statisticalFiltering(8, 2.0)
    n_sor = m.num_patches()
    removed, _ = m.normalFiltering(8, 30.0)
    na = io.load_mvs(str(b / "NA_filter.mvs"))[2]
    assert len(io.load_mvs(str(b / "SOR_filter.mvs"))[2]) == n_sor
    assert len(na) == m.num_patches() == n_sor - removed and 0 < len(na)
    assert len(evaluate.read_ply(str(b / "NA_filter.ply"))) == len(na)
    assert [list(p.center[:]) for p in na] == [list(p.center[:]) for p in m.patches()]
    rough, sp = m.roughness(8), m.spacing()
    m.close()
    capsys.readouterr()
    assert evaluate.main([str(b / "NA_filter.mvs"), "--roughness", "8"]) == 0
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out == {"n": len(na), "k": 8, "roughness": rough, "spacing": sp, "ratio": rough / sp} and rough > 0
