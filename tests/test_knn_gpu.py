"""pais_cloud_knn on the MI355X against the numpy brute force of its definition (tests/knn_ref.py) -- every index equal, every
squared distance bit-equal, whatever the split into slices and passes -- and what is built on it: the sample spacing, the
statistical outlier rule, the driver's filter and the two command lines."""
import copy
import json
import os

import numpy as np
import pytest

from tests import knn_ref

pytestmark = pytest.mark.gpu

SPLIT_ENV = ("PAIS_CLOUD_SLICES", "PAIS_CLOUD_CHUNK")


def _same(got, want, what):
    gi, gd = got[0], got[1]
    wi, wd = want
    assert gi.dtype == np.int32 and gd.dtype == np.float64 and gi.shape == wi.shape and gd.shape == wd.shape, what
    bad = np.argwhere((gi != wi) | (gd.view(np.uint64) != wd.view(np.uint64)))
    assert not len(bad), (what, len(bad), bad[:5], [(gi[tuple(b)], wi[tuple(b)], gd[tuple(b)], wd[tuple(b)]) for b in bad[:5]])


@pytest.fixture(autouse=True)
def _default_split(monkeypatch):
    for k in SPLIT_ENV:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def big_case():
    """(1000, 3001): shared by the k = 16 case and the k = 1 comparison with pais_cloud_nearest"""
    rng = np.random.default_rng(177)
    return rng.normal(size=(1000, 3)), rng.normal(size=(3001, 3))


@pytest.mark.parametrize("nq,nt,k,skip", [(1, 1, 1, False), (1, 1, 4, False), (300, 5, 8, False), (257, 513, 8, False), (63, 511, 32, False),
                                          (1000, 3001, 16, False), (700, 700, 9, True), (700, 700, 17, True)])
def test_knn_equals_the_brute_force_bit_for_bit(nq, nt, k, skip, big_case):
    """padding (nt < k), sizes that are no multiple of the block (256) or the tile (512), k between two instantiations, and
    every instantiation (1, 8, 16, 32)"""
    from pais_mvs_amd import evaluate
    rng = np.random.default_rng(1000 * nq + k)
    q, t = big_case if (nq, nt) == (1000, 3001) else (rng.normal(size=(nq, 3)), rng.normal(size=(nt, 3)))
    if skip:
        t = q
    got = evaluate.knn(q, t, k, skip_self=skip)
    _same(got, knn_ref.brute_knn(q, t, k, skip), (nq, nt, k, skip))
    admissible = nt - (1 if skip else 0)
    assert (got[0][:, :min(k, admissible)] >= 0).all() and (got[0][:, admissible:] == -1).all() and np.isinf(got[1][:, admissible:]).all()
    if skip:
        assert (got[0] != np.arange(nq)[:, None]).all()


def test_ties_come_in_ascending_index():
    from pais_mvs_amd import evaluate
    rng = np.random.default_rng(77)
    base = rng.normal(size=(700, 3))
    t = np.concatenate([base, base[::-1], base])             # every target three times, 2100 targets: 5 tiles, 5 slices
    got = evaluate.knn(base, t, 4)
    _same(got, knn_ref.brute_knn(base, t, 4), "three copies")
    i = np.arange(700)
    assert np.array_equal(got[0][:, :3], np.stack([i, 1399 - i, 1400 + i], axis=1)) and not got[1][:, :3].any() and (got[1][:, 3] > 0).all()
    # a set with duplicates against itself: the query's own index goes, its duplicate stays at distance 0
    two = np.concatenate([base, base])
    got = evaluate.knn(two, two, 3, skip_self=True)
    _same(got, knn_ref.brute_knn(two, two, 3, True), "duplicates, skip_self")
    assert np.array_equal(got[0][:, 0], (np.arange(1400) + 700) % 1400) and not got[1][:, 0].any() and (got[1][:, 1] > 0).all()
    # all targets equal: the first k of them
    q = base[:333]
    same_t = np.repeat(rng.normal(size=(1, 3)), 1500, axis=0)
    got = evaluate.knn(q, same_t, 8)
    _same(got, knn_ref.brute_knn(q, same_t, 8), "one point many times")
    assert (got[0] == np.arange(8)).all()


def test_small_differences_and_overflowing_distances():
    from pais_mvs_amd import evaluate
    rng = np.random.default_rng(79)
    # coordinates near 1e3, differences near 1e-9: the difference form keeps them
    t = 1e3 + rng.uniform(-1.0, 1.0, size=(2500, 3))
    q = t[rng.permutation(2500)[:900]] + rng.normal(size=(900, 3)) * 1e-9
    got = evaluate.knn(q, t, 8)
    _same(got, knn_ref.brute_knn(q, t, 8), "1e3 / 1e-9")
    assert 0 < np.sqrt(got[1][:, 0]).max() < 1e-7
    # every distance +inf: index order
    big_t, big_q = np.full((600, 3), 1e200), np.full((3, 3), -1e200)
    got = evaluate.knn(big_q, big_t, 8)
    _same(got, knn_ref.brute_knn(big_q, big_t, 8), "overflow")
    assert np.isinf(got[1]).all() and (got[0] == np.arange(8)).all()
    # finite and +inf distances in one row: the finite ones first, then +inf in index order
    mixed = np.concatenate([big_t[:5], rng.normal(size=(3, 3)), big_t[:5]])
    got = evaluate.knn(np.zeros((2, 3)), mixed, 8)
    _same(got, knn_ref.brute_knn(np.zeros((2, 3)), mixed, 8), "finite then +inf")
    assert set(got[0][0, :3]) == {5, 6, 7} and got[0][0, 3:].tolist() == [0, 1, 2, 3, 4]


def test_k_1_is_pais_cloud_nearest_byte_for_byte(big_case):
    from pais_mvs_amd import evaluate
    q, t = big_case
    near = evaluate.nearest(q, t)
    got = evaluate.knn(q, t, 1)
    assert got[0].shape == (1000, 1) and got[0].tobytes() == near[0].tobytes() and got[1].tobytes() == near[1].tobytes()
    big_t, big_q = np.full((600, 3), 1e200), np.full((3, 3), -1e200)         # all +inf: the first target, as the scan leaves it
    near, got = evaluate.nearest(big_q, big_t), evaluate.knn(big_q, big_t, 1)
    assert got[0].tobytes() == near[0].tobytes() and got[1].tobytes() == near[1].tobytes()


def test_result_does_not_depend_on_slices_or_passes(monkeypatch):
    """(1500, 6000, 8), and 2600 of those targets against themselves with skip_self -- with passes of 256 queries a pass that
    skipped its local index instead of the index in the whole set would show here"""
    from pais_mvs_amd import _lib, evaluate
    L = _lib.load()
    rng = np.random.default_rng(178)
    t = rng.normal(size=(6000, 3))
    t[4000:4300] = t[100:400]                                 # ties between far-apart slices
    q = np.concatenate([rng.normal(size=(1200, 3)), t[4000:4300] + rng.normal(size=(300, 3)) * 1e-6])
    s = np.ascontiguousarray(t[2000:4600])
    s[700:1000] = s[2000:2300]                                # duplicates within the set: only the query's own index goes
    for what, a, b, skip in (("two sets", q, t, False), ("self", s, s, True)):
        want = knn_ref.brute_knn(a, b, 8, skip)
        runs = {}
        for name, slices, chunk in (("default", None, None), ("one slice", 1, None), ("max slices", 64, None), ("passes of 256", None, 256),
                                    ("passes of 256, max slices", 64, 256)):
            for k, v in zip(SPLIT_ENV, (slices, chunk)):
                if v is None:
                    monkeypatch.delenv(k, raising=False)
                else:
                    monkeypatch.setenv(k, str(v))
            before = L.pais_cloud_launches()
            got = evaluate._knn(a, b, 8, skip, 0)
            passes = -(-len(a) // (chunk or len(a)))
            assert L.pais_cloud_launches() - before == 2 * passes and got[2] > 0, (what, name)
            _same(got, want, (what, name))
            runs[name] = got[0].tobytes() + got[1].tobytes()
        assert len(set(runs.values())) == 1


@pytest.mark.parametrize("seed", knn_ref.PLANE_SEEDS)
def test_statistical_outliers_on_the_plane_case(seed):
    from pais_mvs_amd import evaluate
    pts, added = knn_ref.plane_case(seed)
    res = evaluate.statistical_outliers(pts, knn_ref.PLANE_K, knn_ref.PLANE_SIGMA)
    knn_ref.assert_rule(res, *knn_ref.brute_knn(pts, pts, knn_ref.PLANE_K, True), knn_ref.PLANE_SIGMA, ("plane", seed))
    assert np.array_equal(res["outlier"], added)
    # the spacing of the jittered unit grid: the median first-neighbour distance, without interpolation
    d2 = np.sort(knn_ref.brute_knn(pts, pts, 1, True)[1][:, 0])
    sp = evaluate.spacing(pts)
    assert sp == float(np.sqrt(d2[588 // 2 - 1])) and 0.5 < sp < 1.0


# ------------------------------------------------------------------------------------------------------- the driver ---
@pytest.fixture(scope="module")
def grown(pawn_small):
    """a cloud of the small pawn scene as a .mvs file holds it, and its configuration (tests/test_filters.py's: a small swarm,
    a loose cell budget and correlation gate)"""
    from pais_mvs_amd.config import readme_config
    from pais_mvs_amd.mvs import MVS
    cfg = readme_config(particleNum=6, maxIteration=8, maxCellPatchNum=6, minCorrelation=0.6)
    m = MVS(cfg, pawn_small.cameras, device=0, seed=42)
    for X, vis in pawn_small.seeds:
        m.add_seed(X, vis)
    m.refineSeedPatches()
    m.expansionPatches(64, 40)
    cloud = [(list(p.center[:]), list(p.normalS[:]), p.cams(), p.fitness, p.correlation) for p in m.patches()]
    m.close()
    assert len(cloud) > 200
    return cfg, cloud


def _loaded(cfg, cameras, cloud):
    from pais_mvs_amd.mvs import MVS
    m = MVS(cfg, cameras, device=0, seed=42)
    for c, ns, cams, fit, corr in cloud:
        m.load_patch(c, ns, cams, fit, corr)
    return m


def _alive(m):
    return [i for i in range(m.num_slots()) if m.get_patch(i) is not None]


def test_driver_filter_deletes_what_the_rule_predicts(pawn_small, grown, monkeypatch):
    from pais_mvs_amd import evaluate
    cfg, cl = grown
    m = _loaded(cfg, pawn_small.cameras, cl)
    ids = _alive(m)
    pts = m.cloud()[:, :3]
    assert ids == list(range(len(cl))) and len(pts) == len(cl)
    res = evaluate.statistical_outliers(m.cloud(), 8, 2.0)
    knn_ref.assert_rule(res, *knn_ref.brute_knn(pts, pts, 8, True), 2.0, "pawn cloud")
    want = [i for i, o in zip(ids, res["outlier"]) if not o]
    d2 = np.sort(knn_ref.brute_knn(pts, pts, 1, True)[1][:, 0])
    assert m.spacing() == float(np.sqrt(d2[-(-len(pts) // 2) - 1])) > 0
    removed, ms = m.statisticalFiltering(8, 2.0)
    print("\npawn_small cloud of %d: %d removed, mu %.5g sd %.5g threshold %.5g, %.3f ms" % (len(cl), removed, res["mu"], res["sd"], res["threshold"], ms))
    assert _alive(m) == want and removed == len(cl) - len(want) and m.num_patches() == len(want) and ms > 0
    assert 1 <= removed < len(cl) // 4                        # at least one patch goes and most stay
    m.close()
    monkeypatch.setenv("PAIS_CLOUD_SLICES", "64")
    m2 = _loaded(cfg, pawn_small.cameras, cl)
    assert m2.statisticalFiltering(8, 2.0)[0] == removed and _alive(m2) == want
    m2.close()


def test_command_lines(tmp_path, pawn_small, grown, capsys):
    """--filter --statistical K,SIGMA writes SOR_filter.* with the driver's patch count after today's files, which it leaves
    as they are; evaluate --spacing prints evaluate.spacing of the file's cloud"""
    from PIL import Image
    from pais_mvs_amd import evaluate, io, reconstruct
    cfg, cl = copy.copy(grown[0]), grown[1]                  # writeMVS notes the neighbour radius in its configuration
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
    a, b = tmp_path / "plain", tmp_path / "sor"
    a.mkdir()
    b.mkdir()
    reconstruct.main([path, "--filter", "--config", str(tmp_path / "none.txt"), "--out", str(a)])
    reconstruct.main([path, "--filter", "--config", str(tmp_path / "none.txt"), "--out", str(b), "--statistical", "8,2"])
    today = {s + e for s in ("PMVS_filter1", "PMVS_filter2", "PMVS_filter3", "PCMVS_filter") for e in (".mvs", ".ply")}
    assert set(os.listdir(a)) == today and set(os.listdir(b)) == today | {"SOR_filter.mvs", "SOR_filter.ply"}
    for f in today:
        assert (a / f).read_bytes() == (b / f).read_bytes(), f
    # the same chain through the driver
    file_cfg, cams_io, pats = io.load_mvs(path)
    m = _loaded(file_cfg, reconstruct.load_cameras(cams_io, str(tmp_path), file_cfg),
                [(p.center[:], p.normalS[:], list(p.cam_idx[:p.num_cam]), p.fitness, p.correlation) for p in pats])
    m.cellFiltering(); m.visibilityFiltering(); m.neighborCellFiltering(0.25); m.neighborPatchFiltering(0.25)
    n_pcmvs = m.num_patches()
    removed, _ = m.statisticalFiltering(8, 2.0)
    sor = io.load_mvs(str(b / "SOR_filter.mvs"))[2]
    assert len(io.load_mvs(str(b / "PCMVS_filter.mvs"))[2]) == n_pcmvs
    assert len(sor) == m.num_patches() == n_pcmvs - removed and 0 < len(sor)
    assert len(evaluate.read_ply(str(b / "SOR_filter.ply"))) == len(sor)
    assert [list(p.center[:]) for p in sor] == [list(p.center[:]) for p in m.patches()]
    want = m.spacing()
    m.close()
    capsys.readouterr()
    assert evaluate.main([str(b / "SOR_filter.mvs"), "--spacing"]) == 0
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out == {"n": len(sor), "spacing": want}
