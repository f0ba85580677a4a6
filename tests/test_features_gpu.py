"""include/pais_feature.h on the GPU: pais_feature_detect against the host build of the same statements
(tests/feature_host_shim.cpp) BIT for bit, the growth of its buffers, the shift property, MVS.seed_from_images against the
oracle's seeds, and `reconstruct` on a scene without points."""
import os

import numpy as np
import pytest

from tests import features_ref as fr

pytestmark = pytest.mark.gpu


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_same(got, ref, n=None):
    """got: (xy, scale, angle, octave_layer, desc) of the GPU; ref: a ShimRun; the first n keypoints (all of them by default)."""
    n = ref.n if n is None else n
    for g, r, name in zip(got, (ref.xy, ref.scale, ref.angle, ref.ol, ref.desc), ("xy", "scale", "angle", "octave_layer", "desc")):
        assert len(g) == n, (name, len(g), n)
        assert np.array_equal(_bits(g), _bits(r[:n])), name


def _pawn_image(pawn_small):
    return np.ascontiguousarray(pawn_small.cameras[0].image)


def _strided():
    buf = np.full((70, 192), 255, np.uint8)                  # the padding must never be read as image
    buf[:, :130] = fr.noise_image(130, 70, 4)
    return buf[:, :130]


CASES = {
    "97x61": lambda s: fr.noise_image(97, 61, 1),            # odd sizes: every octave halves to an odd dimension
    "160x120": lambda s: fr.noise_image(160, 120, 2),
    "64x64-constant": lambda s: np.full((64, 64), 93, np.uint8),
    "12x12": lambda s: fr.noise_image(12, 12, 6),            # too small for an octave
    "pawn-320x240": _pawn_image,
    "130x70-stride-192": lambda s: _strided(),
}


@pytest.mark.parametrize("case", list(CASES))
def test_detect_equals_the_host_build_bit_for_bit(case, pawn_small):
    from pais_mvs_amd import features
    g = CASES[case](pawn_small)
    if case == "130x70-stride-192":
        assert g.strides == (192, 1)
    ref = fr.ShimRun(g)
    n, xy, scale, angle, ol, desc, ms = features.detect_raw(g, ref.n + 8)
    print("%s: %d keypoints, kernels %.3f ms" % (case, n, ms))
    assert n == ref.n
    if case in ("64x64-constant", "12x12"):
        assert n == 0
    else:
        assert n > 20
    assert_same((xy[:n], scale[:n], angle[:n], ol[:n], desc[:n]), ref)
    key = [(int(o), int(l)) for o, l in ol[:n]]
    assert key == sorted(key)


def test_buffers_grow_and_nothing_is_dropped(monkeypatch):
    from pais_mvs_amd import features
    g = fr.noise_image(160, 120, 2)
    ref = fr.ShimRun(g)
    third = ref.n // 3
    n, xy, scale, angle, ol, desc, _ = features.detect_raw(g, third)
    assert n == ref.n and third >= 5                         # *num is the full count, the prefix is the prefix of the full result
    assert_same((xy, scale, angle, ol, desc), ref, third)
    n0, *_ = features.detect_raw(g, 0)
    assert n0 == ref.n
    full = features.detect_full(g, first=7)                  # the retry loop of the binding
    assert_same(full[:5], ref)
    monkeypatch.setenv("PAIS_FEATURE_CANDS", "5")            # a candidate buffer far too small: grown, the launch repeated
    before = features.launches()
    small = features.detect_full(g)
    grown = features.launches() - before
    monkeypatch.delenv("PAIS_FEATURE_CANDS")
    before = features.launches()
    features.detect_full(g)
    assert grown > features.launches() - before              # the extrema launch did run again
    assert_same(small[:5], ref)


def test_shift_property_on_the_gpu():
    from pais_mvs_amd import features
    from tests.test_features_cpu import check_shift

    class Run:
        def __init__(self, g):
            self.xy, self.scale, self.angle, self.ol, self.desc, _ = features.detect_full(g)
            self.n = len(self.xy)

    a, b, shift = fr.shift_pair()
    assert check_shift(Run(a), Run(b), shift) >= 5


def test_seed_from_images_equals_the_oracle_seeds(pawn_small):
    """MVS.seed_from_images(3.0): cameras, image points and centres of the seeds are those the oracle's setSeedPatches gives on
    the host build's keypoints; the seeds then go through refineSeedPatches."""
    from pais_mvs_amd.config import readme_config
    from pais_mvs_amd.mvs import MVS
    from tests import common
    from tests.test_features_cpu import pawn_keypoints
    from tests.test_seed_generation import _seeds_of, oracle_features
    cfg = readme_config()
    S = common.oracle_scene(cfg, pawn_small)
    xy, desc = pawn_keypoints(pawn_small)
    want = oracle_features(S, xy, desc, 3.0)
    m = MVS(cfg, pawn_small.cameras, device=0, seed=42)
    n = m.seed_from_images(3.0)
    got = _seeds_of(m)
    assert n == len(want) == len(got) >= 1
    for (nodes, cen), (cams, pts, c) in zip(want, got):
        assert cams == [a for a, _ in nodes]
        assert pts == [(float(xy[a][f][0]), float(xy[a][f][1])) for a, f in nodes]
        assert c == cen
    m.refineSeedPatches()
    assert m.stats().seeds_refined == n
    m.close()


def test_reconstruct_seeds_a_scene_without_points(tmp_path, pawn_small, capsys):
    """The verb end to end: cameras and images, zero points.  Before the detector this wrote an empty cloud."""
    from PIL import Image
    from pais_mvs_amd import io, reconstruct
    d = tmp_path
    lines = ["NVM_V3", "", str(len(pawn_small.cameras))]
    for i, cam in enumerate(pawn_small.cameras):
        name = "cam%d.png" % i
        Image.fromarray(np.repeat(cam.pyramid[0][:, :, None], 3, axis=2)).save(str(d / name))
        lines.append("%s %r %r %r %r %s %s" % (name, float(cam.focal[0]), float(cam.focal[1]), float(cam.principle_point[0]),
                                               float(cam.principle_point[1]), " ".join(repr(float(v)) for v in cam.quaternion),
                                               " ".join(repr(float(v)) for v in cam.center)))
    lines += ["", "0", "", "0"]
    (d / "scene.nvm2").write_text("\n".join(lines) + "\n")
    (d / "config.txt").write_text("particleNum 6\nmaxIteration 8\n")
    assert io.load_nvm(str(d / "scene.nvm2"), nvm2=True)[1] == []
    reconstruct.main([str(d / "scene.nvm2"), "--config", str(d / "config.txt"), "--out", str(d), "--max-rounds", "2", "--autosave-every", "0"])
    assert "try less minCamNum" not in capsys.readouterr().out
    n_init = len(io.load_mvs(str(d / "init.mvs"))[2])
    n_exp = len(io.load_mvs(str(d / "exp.mvs"))[2])
    print("init.mvs %d patches, exp.mvs %d patches" % (n_init, n_exp))
    assert n_init >= 1 and n_exp >= 1
    assert os.path.getsize(str(d / "exp.ply")) > 0
