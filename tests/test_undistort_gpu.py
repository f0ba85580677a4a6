"""include/pais_undistort.h on the MI355X: every byte, flag and count equal to the numpy restatement of the header
(tests/undistort_ref.py) whatever the launch split, refused inputs that launch nothing, the effect of the undistortion on a
reconstruction scored against ground truth, and the `reconstruct --undistort` verb from files."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import undistort_ref as ur
from tests.test_undistort_cpu import refused_calls

pytestmark = pytest.mark.gpu

MODELS = (ur.M2I, ur.I2M)
OVERRIDES = (None, 1)      # PAIS_UNDISTORT_ROWS / PAIS_UNDISTORT_POINTS: the default, and the minimum


def api_lens(L):
    from pais_mvs_amd import undistort
    return undistort.Lens(L.focal[:], L.pp[:], L.k, L.model)


def set_override(monkeypatch, name, value):
    if value is None:
        monkeypatch.delenv(name, raising=False)
    else:
        monkeypatch.setenv(name, str(value))


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("k", ur.KS)
def test_points_equal_the_restatement_bit_for_bit(monkeypatch, model, k):
    from pais_mvs_amd import undistort
    calls = {ur.UNDISTORT_POINTS: undistort.undistort_points, ur.DISTORT_POINTS: undistort.distort_points}
    for (w, h), L in (((130, 70), ur.rig_lens(130, 70, k, model)), ((2, 2), ur.clens((1.0, 1.0), (0.0, 0.0), k, model))):
        pts = ur.boundary_points(L, w, h, 3)
        assert len(pts) > 2 * 256                                 # more than one block
        for what, call in calls.items():
            want = ur.np_points(L, what, pts)
            for forced in OVERRIDES:
                set_override(monkeypatch, "PAIS_UNDISTORT_POINTS", forced)
                before = undistort.launches()
                xy, ok, ms = call(pts, api_lens(L))
                assert undistort.launches() - before == (1 if forced is None else len(pts))
                assert np.array_equal(xy.view(np.uint64), want[0].view(np.uint64)) and np.array_equal(ok, want[1]), (model, k, what, forced)
                assert ms > 0
    xy, ok, ms = undistort.undistort_points(np.zeros((0, 2)), api_lens(L))        # n == 0 is no error
    assert xy.shape == (0, 2) and ok.shape == (0,) and ms == 0.0


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("k", ur.KS)
def test_images_equal_the_restatement_bit_for_bit(monkeypatch, model, k):
    from pais_mvs_amd import _lib, undistort
    lib = _lib.load()
    for (w, h) in ur.SIZES:
        L = ur.rig_lens(w, h, k, model)                           # anisotropic focal, off-centre principal point
        for ch, pad in ((1, 0), (3, 0), (1, 7), (3, 5)):          # pad: stride > width x channels
            img = ur.noise_image(w, h, ch, 11 + w + ch, pad)
            want = ur.np_image(L, img)
            for forced in OVERRIDES:
                set_override(monkeypatch, "PAIS_UNDISTORT_ROWS", forced)
                before = undistort.launches()
                dst, mask, ms = undistort.undistort_image(img, api_lens(L))
                assert undistort.launches() - before == (1 if forced is None else -(-h // 16)), (w, h, forced)
                assert np.array_equal(dst, want[0]) and np.array_equal(mask, want[1]), (model, k, w, h, ch, pad, forced)
                assert ms > 0
            # valid_pixels, and a NULL mask
            n, out = C.c_int64(-1), np.empty(want[0].shape, np.uint8)
            z = api_lens(L)
            assert lib.pais_undistort_image(0, C.byref(z), ch, img.ctypes.data, w, h, img.strides[0], out.ctypes.data, None, C.byref(n), None) == 0
            assert n.value == want[2] and np.array_equal(out, want[0])


def test_every_refused_input_launches_nothing():
    from pais_mvs_amd import _lib, undistort
    L = _lib.load()
    before = undistort.launches()
    res = refused_calls(L)
    assert len(res) >= 50
    for what, rc, err in res:
        assert rc < 0 and err, (what, rc, err)
    assert undistort.launches() == before
    lens = undistort.Lens((300.0, 310.0), (8.0, 6.0), -0.2, 0)
    undistort.undistort_image(np.zeros((12, 16), np.uint8), lens)
    undistort.distort_points(np.ones((3, 2)), lens)
    assert undistort.launches() == before + 2


def test_image_verb_writes_the_restatement(tmp_path, capsys):
    """`python -m pais_mvs_amd.undistort IMAGE --focal F --k K --model M --out FILE`, in process: RGB and grey files."""
    from PIL import Image
    from pais_mvs_amd import undistort
    for ch, model in ((3, "ideal-to-measured"), (1, "measured-to-ideal")):
        img = np.ascontiguousarray(ur.noise_image(67, 41, ch, 21))
        Image.fromarray(img).save(str(tmp_path / "in.png"))
        undistort.main([str(tmp_path / "in.png"), "--focal", "60.5", "--k", "-0.2", "--model", model, "--out", str(tmp_path / "out.png")])
        L = ur.clens((60.5, 60.5), (33.0, 20.0), -0.2, undistort.MODELS[model])      # the default principal point: (w >> 1, h >> 1)
        want = ur.np_image(L, img)
        assert np.array_equal(np.asarray(Image.open(str(tmp_path / "out.png"))), want[0])
        assert "%d of %d pixels valid" % (want[2], 67 * 41) in capsys.readouterr().out


# ------------------------------------------------------------------------------------------------------ end to end ---
K_SCALE = -128.0   # x the README's k of about -0.2: k = +25.5, the first of the scales tried at which B loses half of A
MODEL = ur.M2I
B, ROUNDS = 4096, 0    # until the queue is empty


def reconstruct_and_score(cameras, seeds, truth, threshold):
    from pais_mvs_amd.config import readme_config
    from pais_mvs_amd.mvs import MVS
    m = MVS(readme_config(), cameras, device=0, seed=42)
    try:
        for X, vis in seeds:
            m.add_seed(X, vis)
        m.refineSeedPatches()
        m.expansionPatches(B, ROUNDS)
        if m.num_patches() == 0:
            return {"n": 0, "completeness": 0.0, "cloud_to_truth_median": float("inf")}
        return m.score(truth, threshold)
    finally:
        m.close()


@pytest.fixture(scope="module")
def three_reconstructions(pawn_small):
    from pais_mvs_amd import synth, undistort
    from pais_mvs_amd.config import readme_config
    cfg = readme_config()
    pts, nrm, spacing = synth.ground_truth(pawn_small)
    truth = np.concatenate([pts, nrm], axis=1)
    bent = synth.pawn_scene(width=320, height=240, n_seeds=24, distort=(MODEL, K_SCALE))
    fixed = undistort.undistort_scene(bent.cameras, MODEL, cfg.lodRatio, cfg.maxLOD, build_edges=bool(cfg.adaptiveGradientEnable))
    out = {"bent": bent, "fixed": fixed}
    for name, cams in (("A", pawn_small.cameras), ("B", bent.cameras), ("C", fixed)):
        out[name] = reconstruct_and_score(cams, pawn_small.seeds, truth, 2 * spacing)
    return out


def test_undistortion_brings_the_reconstruction_back(three_reconstructions, pawn_small):
    """Three reconstructions of the small pawn from the same seeds, scored against synth.ground_truth: A on ideal images, B on
    images measured through the lens with k ignored (the behaviour without the feature), C on those images undistorted.
    C is closer to A than to B in completeness and in the median cloud-to-truth distance.  k is scaled until B loses at
    least half of A's completeness (the pawn sits near the image centre: at the README's own k the cameras disagree by 1-2
    pixels only); that is a precondition, asserted here.
    Measured, measured-to-ideal, expansion until the queue is empty (patches, completeness, median distance):
        A                                    2534  0.9922  0.003311
        K_SCALE   -8 (k =  +1.6)    B        2371  0.9446  0.004390      C  2582  0.9948  0.003536
        K_SCALE  -32 (k =  +6.4)    B        1909  0.6707  0.005990      C  2586  0.9968  0.003491
        K_SCALE  -64 (k = +12.8)    B        1662  0.5692  0.008423      C  2674  0.9981  0.003538
        K_SCALE -128 (k = +25.5)    B        1396  0.4026  0.011674      C  2637  0.9988  0.003536
    The five cameras all look at the pawn, so near the centre the term acts much like one common change of scale, which the
    reconstruction tolerates: B loses half of A only at k = +25.5."""
    r = three_reconstructions
    A, Bs, Cs = r["A"], r["B"], r["C"]
    for name in "ABC":
        print("\n%s: patches %d  completeness %.4f  median distance %.6g" % (name, r[name]["n"], r[name]["completeness"], r[name]["cloud_to_truth_median"]))
    for cam in r["fixed"]:
        assert cam.radial_distortion == 0.0 and cam.image.shape == (240, 320) and len(cam.pyramid) == cam.max_lod + 1
    for cam, src in zip(r["fixed"], r["bent"].cameras):
        assert src.radial_distortion > 20.0 and np.array_equal(cam.focal, src.focal) and np.array_equal(cam.principle_point, src.principle_point)
    assert A["completeness"] > 0.2
    assert Bs["completeness"] <= 0.5 * A["completeness"]                       # the precondition
    assert abs(Cs["completeness"] - A["completeness"]) < abs(Cs["completeness"] - Bs["completeness"])
    assert abs(Cs["cloud_to_truth_median"] - A["cloud_to_truth_median"]) < abs(Cs["cloud_to_truth_median"] - Bs["cloud_to_truth_median"])


def test_undistorted_measurements_recentre_onto_their_seeds(three_reconstructions, pawn_small):
    """The NVM path: every measurement through pais_undistort_points, then add_seed_measured / reCentering from a displaced
    centre lands on the seed; the measurements left as they are do not."""
    from pais_mvs_amd import undistort
    from pais_mvs_amd.config import readme_config
    from pais_mvs_amd.mvs import MVS
    bent, fixed = three_reconstructions["bent"], three_reconstructions["fixed"]
    m = MVS(readme_config(), fixed, device=0, seed=42)
    good, bad = [], []
    for (X, vis), meas in zip(bent.seeds, bent.measurements):
        ideal = [undistort.undistort_points([uv], undistort.lens_of(bent.cameras[c], MODEL))[0][0] for c, uv in zip(vis, meas)]
        for pts, errs in ((ideal, good), (meas, bad)):
            pid = m.add_seed_measured([X[0] + 0.01, X[1] - 0.01, X[2] + 0.02], vis, [list(p) for p in pts], recenter=True)
            errs.append(float(np.linalg.norm(np.array(m.get_patch(pid).center[:]) - X)))
    m.close()
    print("\nre-centred seeds: worst distance %.3g with undistorted measurements, median %.3g with the measured ones" % (max(good), float(np.median(bad))))
    assert max(good) < 1e-8 and np.median(bad) > 1e3 * max(good)


def test_measurements_beyond_the_fold_are_dropped_and_starved_points_skipped(capsys):
    """reconstruct.undistort_measurements: k = -5 on camera 0 puts its fold inside the image.  A measurement beyond it leaves
    with its camera; a point left with fewer than two measurements comes back as None with a message, so the load goes on."""
    from pais_mvs_amd import reconstruct, undistort
    lenses = [undistort.Lens(100.0, (64.0, 48.0), -5.0, "measured-to-ideal"), undistort.Lens(100.0, (64.0, 48.0), 0.0, "measured-to-ideal"),
              undistort.Lens(100.0, (64.0, 48.0), 0.3, "measured-to-ideal")]
    inside, beyond = [66.0, 50.0], [120.0, 90.0]                  # radii 0.028 and 0.70 against the fold's 0.258
    pts = [([0, 1, 2], [inside, [70.0, 40.0], [10.0, 90.0]]),     # all kept
           ([0, 1, 2], [beyond, [70.0, 40.0], [10.0, 90.0]]),     # camera 0 dropped, two left
           ([0, 1], [beyond, [70.0, 40.0]]),                      # one left: skipped
           ([0], [beyond]),                                       # none left: skipped
           ([1], [[70.0, 40.0]])]                                 # came with one: passed on as it is
    out = reconstruct.undistort_measurements(pts, lenses, 0)
    assert [None if o is None else o[0] for o in out] == [[0, 1, 2], [1, 2], None, None, [1]]
    assert out[1][1][0] == [70.0, 40.0] and out[4][1] == [[70.0, 40.0]]           # k = 0: the measurement itself
    for (idx, meas), lens_idx in ((out[0], [0, 1, 2]),):
        for c, got, uv in zip(lens_idx, meas, pts[0][1]):
            L = lenses[c]
            want = ur.np_points(ur.clens(L.focal[:], L.pp[:], L.k, L.model), ur.UNDISTORT_POINTS, [uv])[0][0]
            assert got == list(want)
    msg = capsys.readouterr().out
    assert "point 2: 1 of its 2 measurements" in msg and "point 3: 0 of its 1 measurements" in msg and "point 1" not in msg


def test_undistorted_names_never_collide(tmp_path):
    """a.jpg, a.png and a_1.png of one scene get three different files under undistorted/."""
    from PIL import Image
    from pais_mvs_amd import reconstruct
    from pais_mvs_amd.camera import Camera
    from pais_mvs_amd.config import readme_config
    cfg = readme_config()
    cams = []
    for i, name in enumerate(("a.jpg", "sub/a.png", "a_1.png")):
        img = ur.noise_image(32, 24, 1, 40 + i)
        cams.append(Camera(focal=np.array([30.0, 30.0]), principle_point=np.array([-1.0, -1.0]), quaternion=np.array([1.0, 0, 0, 0]),
                           center=np.zeros(3), image=np.ascontiguousarray(img), name=name, radial_distortion=-0.1 * (i + 1))
                    .finalize(cfg.lodRatio, cfg.maxLOD, False))
    new, lenses = reconstruct.undistort_cameras(cams, "measured-to-ideal", cfg, str(tmp_path), 0)
    names = [c.name for c in new]
    assert names == [str(tmp_path / "undistorted" / n) for n in ("a.png", "a_1.png", "a_1_1.png")]
    for c, old_cam, L in zip(new, cams, lenses):
        assert np.array_equal(np.asarray(Image.open(c.name)), c.image) and L.k == old_cam.radial_distortion and c.radial_distortion == 0.0
    assert len({c.image.tobytes() for c in new}) == 3


# --------------------------------------------------------------------------------------------------------- the verb ---
def write_nvm(d, scene):
    """scene.nvm with the cameras' radial terms, their (measured) images as PNG, and the seeds' measured pixels."""
    from PIL import Image
    lines = ["NVM_V3", "", str(len(scene.cameras))]
    for i, cam in enumerate(scene.cameras):
        name = "cam%d.png" % i
        Image.fromarray(np.repeat(cam.pyramid[0][:, :, None], 3, axis=2)).save(str(d / name))
        lines.append("%s\t%r %s %s %r 0" % (name, float(cam.focal[0]), " ".join(repr(float(v)) for v in cam.quaternion),
                                           " ".join(repr(float(v)) for v in cam.center), float(cam.radial_distortion)))
    lines += ["", str(len(scene.seeds))]
    for (X, vis), meas in zip(scene.seeds, scene.measurements):
        ms = " ".join("%d 0 %r %r" % (c, float(uv[0] - scene.cameras[c].width // 2), float(uv[1] - scene.cameras[c].height // 2)) for c, uv in zip(vis, meas))
        lines.append("%r %r %r 128 128 128 %d %s" % (float(X[0]) + 0.01, float(X[1]) - 0.01, float(X[2]) + 0.02, len(vis), ms))
    lines += ["", "0"]
    (d / "scene.nvm").write_text("\n".join(lines) + "\n")
    (d / "config.txt").write_text("particleNum 6\nmaxIteration 8\n")


def test_reconstruct_verb_undistorts_and_resumes_from_its_own_images(tmp_path, three_reconstructions):
    from PIL import Image
    from pais_mvs_amd import io, reconstruct
    bent = three_reconstructions["bent"]
    d = tmp_path
    write_nvm(d, bent)
    out = d / "out"
    out.mkdir()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, "-m", "pais_mvs_amd.reconstruct", str(d / "scene.nvm"), "--undistort", "measured-to-ideal", "--max-rounds", "2",
           "--parents-per-round", "16", "--config", str(d / "config.txt"), "--out", str(out)]
    r = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=300)      # a fresh child process
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    names = sorted(os.listdir(out / "undistorted"))
    assert names == ["cam%d.png" % i for i in range(len(bent.cameras))]
    file_cfg, cams_io, pats = io.load_mvs(str(out / "exp.mvs"))
    assert len(cams_io) == len(bent.cameras) and len(pats) >= len(bent.seeds) // 2
    fixed = three_reconstructions["fixed"]
    for i, c in enumerate(cams_io):
        assert c.radial_distortion == 0.0                                               # every radial term is 0
        assert c.file_name.decode() == str(out / "undistorted" / ("cam%d.png" % i))     # and the names point at the new files
        png = np.asarray(Image.open(c.file_name.decode()))
        assert png.shape == (240, 320, 3) and np.array_equal(png[..., 0], fixed[i].image)   # grey in, grey out: the library's bytes
    # a resume from that exp.mvs loads those images
    cfg = io.load_config(str(d / "config.txt"), file_cfg)
    cams = reconstruct.load_cameras(cams_io, str(d), cfg)
    for cam, want in zip(cams, fixed):
        assert np.array_equal(cam.image, want.image) and cam.radial_distortion == 0.0
    res = d / "resumed"
    res.mkdir()
    r2 = subprocess.run([sys.executable, "-m", "pais_mvs_amd.reconstruct", str(out / "exp.mvs"), "--max-rounds", "1", "--parents-per-round", "16",
                         "--config", str(d / "config.txt"), "--out", str(res)], cwd=root, capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0, (r2.stdout[-1000:], r2.stderr[-3000:])
    again = io.load_mvs(str(res / "exp.mvs"))
    assert len(again[2]) > 0 and all(c.radial_distortion == 0.0 for c in again[1])
    assert [c.file_name for c in again[1]] == [c.file_name for c in cams_io]
    # for an .mvs scene the flag is refused with a message
    r3 = subprocess.run([sys.executable, "-m", "pais_mvs_amd.reconstruct", str(out / "exp.mvs"), "--undistort", "measured-to-ideal", "--out", str(res)],
                        cwd=root, capture_output=True, text=True, timeout=120)
    assert r3.returncode != 0 and "already say what they are" in r3.stderr
