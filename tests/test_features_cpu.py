"""include/pais_feature.h without a GPU: pais::det_atan2 against libm, the lane-local arithmetic of pais_feature.hpp (compiled
for the host by tests/feature_host_shim.cpp) against a numpy restatement of the header (tests/features_ref.py), the exact
shift property, the seeds the keypoints of the small pawn scene give, and the refusals of the C entry."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import features_ref as fr


def test_det_atan2_against_libm():
    S = fr.shim()
    rng = np.random.default_rng(5)
    n = 100000
    y = rng.standard_normal(n) * np.exp(rng.uniform(-30, 30, n))
    x = rng.standard_normal(n) * np.exp(rng.uniform(-30, 30, n))
    y[: n // 4] = rng.uniform(-300, 300, n // 4)            # the magnitudes of image gradients
    x[: n // 4] = rng.uniform(-300, 300, n // 4)
    got = np.zeros(n)
    dp = C.POINTER(C.c_double)
    S.shim_atan2_many(y.ctypes.data_as(dp), x.ctypes.data_as(dp), n, got.ctypes.data_as(dp))
    worst = 0.0
    for a, b, g in zip(y.tolist(), x.tolist(), got.tolist()):
        w = math.atan2(a, b)
        if g != w:
            worst = max(worst, abs(g - w) / math.ulp(w))
    print("det_atan2 worst error: %.3f ulp over %d pairs" % (worst, n))
    assert worst <= 1.0                                     # fdlibm's documented bound for atan2
    inf, nan = math.inf, math.nan
    special = [(0.0, 1.0), (-0.0, 1.0), (0.0, -1.0), (-0.0, -1.0), (1.0, 0.0), (-1.0, 0.0), (1.0, -0.0), (-1.0, -0.0),
               (0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0), (inf, inf), (-inf, inf), (inf, -inf), (-inf, -inf),
               (1.0, inf), (-1.0, inf), (1.0, -inf), (-1.0, -inf), (inf, 1.0), (-inf, 1.0), (inf, -1.0), (-inf, -1.0),
               (5.0, 0.0), (-5.0, -0.0), (1.0, 1.0), (-1.0, 1.0), (1.0, -1.0), (-1.0, -1.0), (1e-310, 1.0), (1.0, 1e-310)]
    for a, b in special:
        g, w = S.shim_atan2(a, b), math.atan2(a, b)
        assert g == w and math.copysign(1.0, g) == math.copysign(1.0, w), (a, b, g, w)
    for a, b in ((nan, 1.0), (1.0, nan), (nan, nan), (nan, inf), (0.0, nan)):
        assert math.isnan(S.shim_atan2(a, b))


@pytest.fixture(scope="module")
def legs():
    """Shim and numpy restatement on the two committed images, computed once."""
    out = {}
    for (w, h, seed) in ((97, 61, 1), (160, 120, 2)):
        g = fr.noise_image(w, h, seed)
        out[(w, h)] = (g, fr.ShimRun(g, stages=True), fr.np_detect(g))
    return out


def test_tap_tables_equal_the_restatement():
    S = fr.shim()
    for s in fr.np_sigmas(fr.DEFAULTS) + [0.3, 2.5, 7.0]:
        t, R = fr.np_taps(s)
        assert S.shim_feat_tap_radius(s) == R
        got = np.zeros(2 * R + 1, np.float32)
        S.shim_feat_taps(s, got.ctypes.data_as(C.POINTER(C.c_float)))
        assert np.array_equal(got, t), s


@pytest.mark.parametrize("size", [(97, 61), (160, 120)])
def test_scale_space_and_candidates_equal_the_restatement(legs, size):
    g, sh, ref = legs[size]
    assert len(sh.octaves) == len(ref["octaves"]) >= 2
    total = 0
    for o, (a, b) in enumerate(zip(sh.octaves, ref["octaves"])):
        assert a["layers"].shape == b["layers"].shape, o
        assert np.array_equal(a["layers"].view(np.uint32), b["layers"].view(np.uint32)), o        # no libm in them: BIT-equal
        assert np.array_equal((a["layers"][1:] - a["layers"][:-1]).view(np.uint32), b["dog"].view(np.uint32)), o
        assert {tuple(int(v) for v in c) for c in a["cands"]} == b["cands"], o
        total += len(b["cands"])
    assert total > 50


@pytest.mark.parametrize("size", [(97, 61), (160, 120)])
def test_keypoints_equal_the_restatement(legs, size):
    g, sh, ref = legs[size]
    keys = []
    for k in range(sh.n):
        o, i = int(sh.ol[k, 0]), int(sh.ol[k, 1])
        f = 2.0 ** (o - 1)
        keys.append((o, i, int(math.floor(float(sh.xy[k, 1]) / f + 0.5)), int(math.floor(float(sh.xy[k, 0]) / f + 0.5)),
                     int(math.floor(float(sh.angle[k]) * (36.0 / fr.PI2) + 0.5)) % 36))
    assert sh.n == len(ref["keys"]) > 20
    assert keys == sorted(keys)                              # ORDER
    assert keys == ref["keys"]                               # the same keypoints, as (octave, layer, y, x, peak)
    # positions before the rounding to float: the FIT of every candidate, in doubles
    want_xy = {k[:4]: tuple(p) for k, p in zip(ref["keys"], ref["xy"].tolist())}
    seen = 0
    for o, octv in enumerate(sh.octaves):
        f = 2.0 ** (o - 1)
        for (x, y, i, ok), (px, py, s) in zip(octv["fit_int"].tolist(), octv["fit_val"].tolist()):
            if ok:
                w = want_xy[(o, i, y, x)]
                assert abs(px * f - w[0]) <= 1e-9 and abs(py * f - w[1]) <= 1e-9
                seen += 1
    assert seen >= len(want_xy)
    f32 = lambda a: np.asarray(a, np.float64).astype(np.float32).astype(np.float64)
    # the shim rounds to float at the end: compare against the restatement rounded the same way, 1e-9 apart before it
    for got, want in ((sh.xy, ref["xy"]), (sh.scale, ref["scale"]), (sh.angle, ref["angle"])):
        ulp = np.spacing(np.abs(f32(want)).astype(np.float32)).astype(np.float64)
        assert np.all(np.abs(got.astype(np.float64) - np.asarray(want)) <= 0.5 * ulp + 1e-9)
    err = float(np.abs(sh.desc.astype(np.float64) - ref["desc"].astype(np.float64)).max())
    print("descriptor max difference on the 0..255 scale: %.3g" % err)
    assert err <= 1e-3
    assert 0.0 <= sh.desc.min() and sh.desc.max() <= 255.0
    assert np.allclose(np.linalg.norm(sh.desc, axis=1), 512.0, rtol=0.05)


def _inside(run, box, k):
    x0, y0, x1, y1 = box
    r = fr.support_radius(float(run.scale[k]))
    x, y = float(run.xy[k, 0]), float(run.xy[k, 1])
    return x - r >= x0 and y - r >= y0 and x + r <= x1 - 1 and y + r <= y1 - 1


def check_shift(ra, rb, shift):
    """The keypoints whose support lies inside the texture are the same list, shifted: octave, layer, scale, angle and all
    128 descriptor floats bit-equal.  xy is a float: with a = the exact position, fl(a) and fl(a + shift) each carry half a
    float ulp of their own, so xy_b equals xy_a + shift to within one float ulp at the larger of the two -- that is what
    "shifted exactly" can mean for a rounded number, and it is asserted as such."""
    sx, sy = shift
    ia = [k for k in range(ra.n) if _inside(ra, (32, 32, 128, 128), k)]
    ib = [k for k in range(rb.n) if _inside(rb, (32 + sx, 32 + sy, 128 + sx, 128 + sy), k)]
    assert len(ia) == len(ib) >= 5, (len(ia), len(ib))
    for a, b in zip(ia, ib):
        assert tuple(ra.ol[a]) == tuple(rb.ol[b])
        assert ra.scale[a] == rb.scale[b] and ra.angle[a] == rb.angle[b]
        assert np.array_equal(ra.desc[a].view(np.uint32), rb.desc[b].view(np.uint32))
        for c, s in ((0, sx), (1, sy)):
            assert abs(float(rb.xy[b, c]) - (float(ra.xy[a, c]) + s)) <= float(np.spacing(rb.xy[b, c]))
    return len(ia)


def test_shift_property_is_exact():
    a, b, shift = fr.shift_pair()
    n = check_shift(fr.ShimRun(a), fr.ShimRun(b), shift)
    print("shift property: %d keypoints with their support inside the texture" % n)


def pawn_keypoints(scene):
    runs = [fr.ShimRun(np.ascontiguousarray(c.image)) for c in scene.cameras]
    return [r.xy for r in runs], [r.desc for r in runs]


def seed_bound(scene):
    """3 px depth / (f sin a): 3 px the epipolar bound given, depth the median distance of the cameras from the object, f the
    focal length, a the smallest angle between the viewing directions of a camera and its nearest neighbour."""
    centre = np.mean([X for X, _ in scene.seeds], axis=0)
    d = [c.center - centre for c in scene.cameras]
    depth = float(np.median([np.linalg.norm(v) for v in d]))
    u = [v / np.linalg.norm(v) for v in d]
    ang = min(min(math.acos(max(-1.0, min(1.0, float(u[i] @ u[j])))) for j in range(len(u)) if j != i) for i in range(len(u)))
    return 3.0 * depth / (float(scene.cameras[0].focal[0]) * math.sin(ang)), math.degrees(ang)


def test_seeds_on_pawn_small(pawn_small):
    from pais_mvs_amd import synth
    from pais_mvs_amd.config import readme_config
    from tests import common
    from tests.test_seed_generation import oracle_features
    cfg = readme_config()
    S = common.oracle_scene(cfg, pawn_small)
    xy, desc = pawn_keypoints(pawn_small)
    assert min(len(p) for p in xy) > 50
    seeds = oracle_features(S, xy, desc, 3.0)
    assert len(seeds) >= 1
    assert all(len(nodes) >= cfg.minCamNum for nodes, _ in seeds)
    gt, _, _ = synth.ground_truth(pawn_small)
    cen = np.array([c for _, c in seeds])
    dist = np.array([np.sqrt(((gt - c) ** 2).sum(axis=1).min()) for c in cen])
    bound, ang = seed_bound(pawn_small)
    print("pawn_small: %d keypoints, %d seeds, median seed-to-surface distance %.5f, bound %.5f (smallest adjacent angle %.1f deg)"
          % (sum(len(p) for p in xy), len(seeds), float(np.median(dist)), bound, ang))
    assert float(np.median(dist)) <= bound


def test_refusals_and_no_gpu_means_loud_failure(pawn_small):
    from pais_mvs_amd import _lib, features
    L = features._bind(_lib.load())
    g = fr.noise_image(64, 48, 3)
    before = features.launches()

    def call(gray=g, w=64, h=48, stride=64, prm=None, cap=8, device=0, num=True, outs=True):
        n = C.c_int32(0)
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        bufs = [np.zeros(2 * 8, np.float32), np.zeros(8, np.float32), np.zeros(8, np.float32), np.zeros(2 * 8, np.int32), np.zeros(128 * 8, np.float32)]
        ptr = lambda a: a.ctypes.data_as(ip if a.dtype == np.int32 else fp) if outs else None
        return L.pais_feature_detect(device, None if gray is None else gray.ctypes.data, w, h, stride, None if prm is None else C.byref(prm), cap,
                                     C.byref(n) if num else None, ptr(bufs[0]), ptr(bufs[1]), ptr(bufs[2]), ptr(bufs[3]), ptr(bufs[4]), None)

    def prm(**kw):
        p = features.default_params()
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    assert (features.default_params().layers, features.default_params().sigma) == (3, 1.6)
    refused = [dict(gray=None), dict(num=False), dict(outs=False), dict(device=-1), dict(w=0), dict(h=0), dict(w=-3), dict(stride=63),
               dict(cap=-1), dict(prm=prm(sigma=0.0)), dict(prm=prm(sigma=-1.0)), dict(prm=prm(sigma=math.nan)), dict(prm=prm(sigma=math.inf)),
               dict(prm=prm(sigma=1e4)), dict(prm=prm(input_blur=0.0)), dict(prm=prm(contrast_threshold=-0.04)),
               dict(prm=prm(contrast_threshold=math.nan)), dict(prm=prm(edge_threshold=0.0)), dict(prm=prm(edge_threshold=math.inf)),
               dict(prm=prm(layers=0)), dict(prm=prm(layers=9))]
    for kw in refused:
        assert call(**kw) < 0, kw
        assert L.pais_feature_last_error()
    assert features.launches() == before                     # refused: nothing launched
    with pytest.raises(RuntimeError):
        features.detect(g, device=-1)
    with pytest.raises(ValueError):
        features.detect(np.zeros((4, 4, 2), np.uint8))
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):                    # no GPU: loud failure, never a host result
            features.detect(g, device=0)
        assert features.launches() == before
        from pais_mvs_amd.config import readme_config
        from pais_mvs_amd.mvs import MVS
        m = MVS(readme_config(), pawn_small.cameras, device=-1, seed=1)
        with pytest.raises(RuntimeError):
            m.seed_from_images(3.0)
        m.close()


# ---------------------------------------------------- the cases of tests/test_features_stages_gpu.py, on the host build ---
def assert_shim_equals_restatement(sh, ref):
    """A ShimRun(stages=True) against np_detect of the same image and parameters: layers and DoG bit-equal, candidate sets and
    key lists equal, descriptors within the 1e-3 of test_keypoints_equal_the_restatement.  -> (candidates, keypoints)."""
    assert len(sh.octaves) == len(ref["octaves"])
    total = 0
    for o, (a, b) in enumerate(zip(sh.octaves, ref["octaves"])):
        assert a["layers"].shape == b["layers"].shape, o
        assert np.array_equal(a["layers"].view(np.uint32), b["layers"].view(np.uint32)), o
        assert np.array_equal((a["layers"][1:] - a["layers"][:-1]).view(np.uint32), b["dog"].view(np.uint32)), o
        assert {tuple(int(v) for v in c) for c in a["cands"]} == b["cands"], o
        total += len(b["cands"])
    keys = []
    for k in range(sh.n):
        o, i = int(sh.ol[k, 0]), int(sh.ol[k, 1])
        f = 2.0 ** (o - 1)
        keys.append((o, i, int(math.floor(float(sh.xy[k, 1]) / f + 0.5)), int(math.floor(float(sh.xy[k, 0]) / f + 0.5)),
                     int(math.floor(float(sh.angle[k]) * (36.0 / fr.PI2) + 0.5)) % 36))
    assert sh.n == len(ref["keys"])
    assert keys == sorted(keys) and keys == ref["keys"]
    if sh.n:
        err = float(np.abs(sh.desc.astype(np.float64) - ref["desc"].astype(np.float64)).max())
        assert err <= 1e-3, err
    return total, sh.n


@pytest.mark.parametrize("case", list(fr.PARAM_CASES))
def test_host_build_equals_the_restatement_at_other_parameters(case):
    """The host build the GPU is compared with, pinned to the independent statement at every parameter set the GPU tests run."""
    prm = fr.PARAM_CASES[case]
    g = fr.noise_image(97, 61, 1)
    cands, n = assert_shim_equals_restatement(fr.ShimRun(g, stages=True, **prm), fr.np_detect(g, **prm))
    print("%s: %d candidates, %d keypoints" % (case, cands, n))
    assert cands >= 30 and n >= 30


@pytest.mark.parametrize("case,count", [("checkerboard5-97x61", 792), ("saturated-noise", 488), ("blobs", 90)])
def test_host_build_equals_the_restatement_on_ties_and_duplicates(case, count):
    g = fr.CONTENT_CASES[case]()
    cands, n = assert_shim_equals_restatement(fr.ShimRun(g, stages=True), fr.np_detect(g))
    assert n == count, (case, n)
