"""include/pais_feature.h on the GPU, stage by stage: pais_test_feature_stages (the product's backend behind a recorder, handed
to the product's walk) against the host build of the same statements (tests/feature_host_shim.cpp) -- every octave's sizes,
layers, candidates and FIT rows, BIT for bit -- and pais_feature_detect's five arrays, at parameter sets other than the
defaults, at sizes on, one past and one short of the kernels' block edges, and on images of exact ties and of candidates that
are all rejected.  The non-vacuity conditions are asserted on the host build's result before the GPU is looked at."""
import numpy as np
import pytest

from tests import features_ref as fr
from tests.test_features_gpu import assert_same

pytestmark = pytest.mark.gpu


def gpu_params(prm):
    from pais_mvs_amd import features
    if not prm:
        return None
    p = features.default_params()
    names = dict(layers="layers", sigma="sigma", input_blur="input_blur", contrast="contrast_threshold", edge="edge_threshold")
    for k, v in prm.items():
        setattr(p, names[k], v)
    return p


def _by_key(cands):
    """The permutation that sorts candidate rows (x, y, layer) by (layer, y, x): the GPU appends them in any order."""
    return np.lexsort((cands[:, 0], cands[:, 1], cands[:, 2]))


def assert_stages_and_output(g, ref, prm=None):
    """(a) every octave through the hook, (b) detect_raw, both against the ShimRun `ref` of the same image and parameters."""
    from pais_mvs_amd import features
    P = gpu_params(prm)
    layers = dict(fr.DEFAULTS, **(prm or {}))["layers"]
    for o, want in enumerate(ref.octaves):
        st = features.stages(g, o, params=P)
        assert st["octaves"] == len(ref.octaves) and st["keypoints"] == ref.n, o
        assert (st["layers"].shape[0], st["H"], st["W"]) == want["layers"].shape == (layers + 3,) + want["layers"].shape[1:], o
        bad = np.argwhere(st["layers"].view(np.uint32) != want["layers"].view(np.uint32))
        assert len(bad) == 0, (o, len(bad), bad[:4].tolist())            # (layer, y, x) of the first wrong samples
        assert len(st["cands"]) == len(want["cands"]), o
        a, b = _by_key(st["cands"]), _by_key(want["cands"])
        assert np.array_equal(st["cands"][a], want["cands"][b]), o
        assert len(st["fit_int"]) == len(want["cands"]), o
        assert np.array_equal(st["fit_int"][a], want["fit_int"][b]), o
        assert np.array_equal(st["fit_val"][a].view(np.uint64), want["fit_val"][b].view(np.uint64)), o
    past = features.stages(g, len(ref.octaves), params=P)                # an octave the walk never reaches: sizes only
    assert (past["octaves"], past["W"], past["H"], past["layers"].size, len(past["cands"])) == (len(ref.octaves), 0, 0, 0, 0)
    n, xy, scale, angle, ol, desc, _ = features.detect_raw(g, ref.n + 8, params=P)
    assert n == ref.n
    assert_same((xy[:n], scale[:n], angle[:n], ol[:n], desc[:n]), ref)


@pytest.mark.parametrize("case", list(fr.PARAM_CASES))
def test_stages_equal_the_host_build_at_other_parameters(case):
    prm = fr.PARAM_CASES[case]
    g = fr.noise_image(97, 61, 1)
    ref = fr.ShimRun(g, stages=True, **prm)
    assert ref.n >= 30 and len(ref.octaves) >= 1 and all(len(o["cands"]) >= 1 for o in ref.octaves)
    if case == "layers1":
        assert fr.max_tap_radius(**prm) > 32                             # the row pass stages more than 64 apron samples
    assert_stages_and_output(g, ref, prm)


def test_halving_reads_layer_one_when_there_is_one_layer():
    """layers 1 on 160 x 120: the second octave's L_0 is every second sample of L_1; its widest blur has a radius above 32 on a
    doubled width of 320 = 256 + 64, so a block's apron reaches across the block edge from both sides."""
    prm = dict(layers=1)
    g = fr.noise_image(160, 120, 2)
    ref = fr.ShimRun(g, stages=True, **prm)
    assert len(ref.octaves) >= 2 and ref.n >= 30 and fr.max_tap_radius(**prm) > 32
    assert_stages_and_output(g, ref, prm)


SHAPES = [(128, 33), (129, 34), (127, 35), (256, 36), (33, 128), (385, 31), (16, 300), (300, 16)]


@pytest.mark.parametrize("size", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_stages_equal_the_host_build_at_block_edges(size):
    """Doubled widths 256, 258, 254, 512, 66, 770, 32, 600: the 256-sample strip of the row pass at, one past and one short of a
    block edge; doubled and halved heights 66 .. 600 and 33 .. 128: the 4-row blocks of the column pass on 2-row, 0-row and odd
    tails.  16 is the smallest side that still passes the walk's size test."""
    g = fr.noise_image(size[0], size[1], 7)
    ref = fr.ShimRun(g, stages=True)
    assert ref.n >= 30 and len(ref.octaves) == (2 if min(size) > 31 else 1)
    assert ref.octaves[0]["layers"].shape[1:] == (2 * size[1], 2 * size[0])
    assert_stages_and_output(g, ref)


def test_an_image_too_small_for_an_octave_launches_nothing():
    from pais_mvs_amd import features
    g = fr.noise_image(15, 300, 7)
    ref = fr.ShimRun(g, stages=True)
    assert ref.n == 0 and len(ref.octaves) == 0
    before = features.launches()
    assert_stages_and_output(g, ref)
    assert features.launches() == before


def test_stages_of_a_strided_view():
    buf = np.full((34, 192), 255, np.uint8)                              # the padding must never be read as image
    buf[:, :129] = fr.noise_image(129, 34, 7)
    g = buf[:, :129]
    assert g.strides == (192, 1)
    ref = fr.ShimRun(g, stages=True)
    assert ref.n >= 30
    assert_stages_and_output(g, ref)
    same = fr.ShimRun(np.ascontiguousarray(g))
    assert same.n == ref.n and np.array_equal(same.desc, ref.desc)


@pytest.mark.parametrize("case", list(fr.CONTENT_CASES))
def test_stages_equal_the_host_build_on_ties_and_rejections(case):
    g = fr.CONTENT_CASES[case]()
    ref = fr.ShimRun(g, stages=True)
    cands = sum(len(o["cands"]) for o in ref.octaves)
    if case in ("checkerboard8-160x120", "step-160x120"):
        assert cands >= 100 and ref.n == 0                               # the walk's `no keypoint` path behind candidates
    else:
        assert ref.n >= 30
    if case == "saturated-noise":
        assert sum(fr.fit_duplicates(o) for o in ref.octaves) >= 1       # the sort and unique have something to remove
    assert_stages_and_output(g, ref)


def test_the_result_does_not_depend_on_the_candidate_order(monkeypatch):
    """The saturated image, whose FIT lands two candidates on one key, detected twice: with the default candidate buffer and
    with one of 7 entries, which is grown and filled again in another append order.  Both byte-identical to the host build."""
    from pais_mvs_amd import features
    g = fr.saturated_noise()
    ref = fr.ShimRun(g, stages=True)
    assert sum(fr.fit_duplicates(o) for o in ref.octaves) >= 1 and ref.n >= 30
    first = features.detect_full(g)
    monkeypatch.setenv("PAIS_FEATURE_CANDS", "7")
    second = features.detect_full(g)
    monkeypatch.delenv("PAIS_FEATURE_CANDS")
    assert_same(first[:5], ref)
    assert_same(second[:5], ref)
    for a, b in zip(first[:5], second[:5]):
        assert a.tobytes() == b.tobytes()


def test_seed_from_images_with_parameters_equals_the_oracle_seeds(pawn_small):
    """MVS.seed_from_images(3.0, params) at layers 4, contrast 0.02: the seeds are the oracle's setSeedPatches on the host
    build's keypoints at the same parameters."""
    from pais_mvs_amd.config import readme_config
    from pais_mvs_amd.mvs import MVS
    from tests import common
    from tests.test_seed_generation import _seeds_of, oracle_features
    prm = dict(layers=4, contrast=0.02)
    cfg = readme_config()
    S = common.oracle_scene(cfg, pawn_small)
    runs = [fr.ShimRun(np.ascontiguousarray(c.image), **prm) for c in pawn_small.cameras]
    xy, desc = [r.xy for r in runs], [r.desc for r in runs]
    want = oracle_features(S, xy, desc, 3.0)
    assert len(want) >= 1
    m = MVS(cfg, pawn_small.cameras, device=0, seed=42)
    n = m.seed_from_images(3.0, params=gpu_params(prm))
    got = _seeds_of(m)
    assert n == len(want) == len(got)
    for (nodes, cen), (cams, pts, c) in zip(want, got):
        assert cams == [a for a, _ in nodes]
        assert pts == [(float(xy[a][f][0]), float(xy[a][f][1])) for a, f in nodes]
        assert c == cen
    m.close()
