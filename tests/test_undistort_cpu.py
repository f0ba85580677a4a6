"""include/pais_undistort.h without a GPU: the lane-local arithmetic of pais_undistort.hpp (compiled for the host by
tests/undistort_host_shim.cpp) against the numpy restatement of the header (tests/undistort_ref.py) bit for bit, the
properties of the two maps at their boundaries, the direction of the correction on a rendered camera, the refusals of the C
entries, and the shim as a stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

from tests import undistort_ref as ur

MODELS = (ur.M2I, ur.I2M)


def same_points(a, b):
    return (np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]))


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("k", ur.KS)
def test_points_of_shim_and_restatement_are_bit_equal(model, k):
    for (w, h), L in (((130, 70), ur.rig_lens(130, 70, k, model)), ((2, 2), ur.clens((1.0, 1.0), (0.0, 0.0), k, model))):
        pts = ur.boundary_points(L, w, h, 3)
        for what in (ur.UNDISTORT_POINTS, ur.DISTORT_POINTS):
            got, want = ur.shim_points(L, what, pts), ur.np_points(L, what, pts)
            assert same_points(got, want), (model, k, what)
            assert np.isnan(got[0][~got[1]]).all() and np.isfinite(got[0][got[1]]).all()    # invalid: NaN, NaN and valid = 0
            if k >= 0:
                assert got[1].all()
            else:
                assert got[1].any() and not got[1].all()                                    # the points bracket the boundary


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("k", ur.KS)
def test_images_of_shim_and_restatement_are_bit_equal(model, k):
    seen_invalid = False
    for (w, h) in ur.SIZES:
        L = ur.rig_lens(w, h, k, model)
        for ch, pad in ((1, 0), (3, 0), (1, 7), (3, 5)):
            img = ur.noise_image(w, h, ch, 11 + w + ch, pad)
            got, want = ur.shim_image(L, img), ur.np_image(L, img)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2], (w, h, ch, pad)
            assert got[2] == int(got[1].sum()) and not got[0].reshape(h, w, -1)[~got[1]].any()  # invalid: value 0 and mask 0
            seen_invalid |= not got[1].all()
    assert seen_invalid == (k != 0.0)        # a sample leaves the image, or (k = -5) the fold lies inside it


@pytest.mark.parametrize("model", MODELS)
def test_k_zero_is_a_copy_with_a_full_mask(model):
    for (w, h) in ur.SIZES:
        for ch, pad in ((1, 3), (3, 0)):
            img = ur.noise_image(w, h, ch, 5, pad)
            dst, mask, n = ur.shim_image(ur.rig_lens(w, h, 0.0, model), img)
            assert np.array_equal(dst, img) and mask.all() and n == w * h


def near_the_fold(L, k):
    """For k < 0: points on 16 rays at radii r (1 - 10^-e), e = 2..15, and r itself, for r the fold circle 3 k q + 1 = 0 (the
    edge of G's domain) and for its image (2/3) r (the edge of G^-1's domain, 27 c = -4)."""
    if k >= 0:
        return np.zeros((0, 2))
    rf = math.sqrt(-1.0 / (3.0 * k))
    ang = np.linspace(0.1, 0.1 + 2.0 * math.pi, 16, endpoint=False)
    out = []
    for r in (rf, rf * 2.0 / 3.0):
        for e in list(range(2, 16)) + [None]:
            rr = r if e is None else r * (1.0 - 10.0 ** -e)
            out.append(np.stack([L.pp[0] + rr * L.focal[0] * np.cos(ang), L.pp[1] + rr * L.focal[1] * np.sin(ang)], axis=1))
    return np.concatenate(out)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("k", ur.KS)
def test_round_trips_land_within_1e_9_pixels(model, k):
    """distort(undistort(p)) and the reverse, on random points over several times the image and on points that close in on
    the fold from inside.

    The flat bound of 1e-9 px this feature was specified with rests on the residual of c s^3 + s - 1 alone.  The error of s is that residual over the
    derivative d = 3 c s^2 + 1 Newton divides by, which equals 3 k q + 1 at the point G is applied to and reaches 0 at the
    fold, where the cubic has a double root and the inverse a square-root singularity.  So the flat bound cannot hold on
    every valid point, and this test REPLACES it by one that does, asserted on ALL valid points:

        err <= rad (min(2 delta / d, 2 sqrt(2 delta / |f''|)) + 1e-15) + 4e-12 px

    delta = 2e-15: the residual (at most 1.0e-15, test_no_valid_input_takes_every_step) plus the rounding of c (7 roundings
    from (u, v), times |c s^3| <= 0.5) and of the forward map's output.  For f(s* + e) = d e + f'' e^2 / 2 = delta the near
    root is at most 2 delta / d; where there is none the iterate ends within sqrt(2 delta / |f''|) of the maximum; |f''| =
    6 |c| s = 4/3 at the double root, which gives 5.5e-8, taken twice for margin: 1.1e-7.  Below d = 1e-6 (20 sqrt(delta))
    only that cap is used, because d is computed from a point that carries the error itself; above it d is good to 1 % and
    the first term is taken 1.1 times.  rad is the larger distance from the principal point of the point and of its image,
    in pixels, which scales an error of s into pixels; 1e-15 rad and 4e-12 px are the roundings of the two maps' own
    products and sums at coordinates of at most 1e4 px.
    The strict 1e-9 px is asserted wherever d >= 0.1: there the bound above is at most 1.4e4 x 4.4e-14 + 1.4e-11 + 4e-12 =
    6.4e-10 px.  Measured: err / bound at most 0.31 over all valid points; worst error 8.8e-6 px, at d = 1.6e-15."""
    L = ur.rig_lens(640, 480, k, model)
    rng = np.random.default_rng(9)
    pts = rng.uniform((-3000.0, -3000.0), (3000.0, 3000.0), size=(20000, 2))
    pts[:5000] = rng.uniform((0.0, 0.0), (639.0, 479.0), size=(5000, 2))
    pts[0] = (L.pp[0], L.pp[1])
    pts = np.concatenate([pts, near_the_fold(L, k)])
    pp = np.array(L.pp[:])
    for first, second in ((ur.UNDISTORT_POINTS, ur.DISTORT_POINTS), (ur.DISTORT_POINTS, ur.UNDISTORT_POINTS)):
        a, ok_a, _ = ur.shim_points(L, first, pts)
        big = ok_a & (np.abs(a) <= 1e4).all(axis=1)
        b, ok_b, _ = ur.shim_points(L, second, a[big])
        # a valid point maps onto the monotone branch, up to the rounding of the two validity tests at the boundary itself
        near = len(near_the_fold(L, k))
        assert ok_b.sum() >= len(ok_b) - 2 - near // 4 and ok_b.sum() > 100
        err = np.abs(b - pts[big]).max(axis=1)
        g_side = (a[big] if ur.uses_inverse(model, first) else pts[big])      # the points G is applied to
        x, y = (g_side[:, 0] - L.pp[0]) / L.focal[0], (g_side[:, 1] - L.pp[1]) / L.focal[1]
        d = 3.0 * k * (x * x + y * y) + 1.0
        rad = np.maximum(np.hypot(*(pts[big] - pp).T), np.hypot(*(a[big] - pp).T))
        lim_s = np.where(d < 1e-6, 1.1e-7, np.minimum(1.1 * 4e-15 / np.maximum(d, 1e-6), 1.1e-7))
        lim = rad * (lim_s + 1e-15) + 4e-12
        held = ok_b & (d >= 0.1)
        close = ok_b & (d < 0.1)
        print("model %d k %g %d->%d: %d valid points, worst round trip %.3g px, worst err / bound %.3g; %d with d >= 0.1, worst %.3g px; "
              "%d with d < 0.1 (smallest d %.3g), worst %.3g px"
              % (model, k, first, second, int(ok_b.sum()), err[ok_b].max(), (err / lim)[ok_b].max(), int(held.sum()), err[held].max(),
                 int(close.sum()), d[ok_b].min(), err[close].max() if close.any() else 0.0))
        assert (err[ok_b] <= lim[ok_b]).all()                      # every valid point
        assert held.sum() > 100 and err[held].max() <= 1e-9        # the flat bound, away from the fold
        if k < 0:
            assert close.sum() >= 100 and d[ok_b].min() < 1e-6     # the points do close in on the fold


def test_the_centre_pixel_is_a_fixed_point():
    for model in MODELS:
        for k in ur.KS:
            L = ur.rig_lens(67, 41, k, model)
            for what in (ur.UNDISTORT_POINTS, ur.DISTORT_POINTS):
                out, ok, steps = ur.shim_points(L, what, [(L.pp[0], L.pp[1])])
                assert ok[0] and tuple(out[0]) == (L.pp[0], L.pp[1]) and steps[0] <= 1


def test_validity_flips_between_adjacent_doubles():
    """focal 1 and pp 0 make x = u exactly.  Along y = 0, q = u u and c = k q: the forward map is valid iff
    (3 k) q + 1 > 0 and the inverse iff 27 c >= -4, evaluated in doubles exactly as the header writes them."""
    k = -5.0
    for model in MODELS:
        L = ur.clens((1.0, 1.0), (0.0, 0.0), k, model)
        for target, inverse in ((math.sqrt(-1.0 / (3.0 * k)), False), (math.sqrt(-4.0 / (27.0 * k)), True)):
            us = np.array(ur.adjacent(target, 8))
            pts = np.stack([us, np.zeros_like(us)], axis=1)
            what = next(w for w in (ur.UNDISTORT_POINTS, ur.DISTORT_POINTS) if ur.uses_inverse(model, w) == inverse)
            _, ok, _ = ur.shim_points(L, what, pts)
            q = us * us
            want = (27.0 * (k * q) >= -4.0) if inverse else ((3.0 * k) * q + 1.0 > 0.0)
            assert np.array_equal(ok, want)
            flips = np.nonzero(ok[:-1] != ok[1:])[0]
            assert len(flips) == 1 and ok[0] and not ok[-1]      # valid inside, invalid outside, one flip between neighbours


def test_the_fold_circle_bounds_the_valid_region():
    """Forward map, k < 0: valid exactly inside the circle 3 k q + 1 = 0, where the radius t r stops growing; the valid image
    radii therefore stay below the fold's own image, (2/3) r_fold."""
    k = -5.0
    L = ur.clens((100.0, 100.0), (0.0, 0.0), k, ur.M2I)
    rf = math.sqrt(-1.0 / (3.0 * k))
    ang = np.linspace(0.0, 2.0 * math.pi, 720, endpoint=False)
    for r, valid in ((rf * (1 - 1e-6), True), (rf * (1 + 1e-6), False)):
        pts = np.stack([100.0 * r * np.cos(ang), 100.0 * r * np.sin(ang)], axis=1)
        out, ok, _ = ur.shim_points(L, ur.UNDISTORT_POINTS, pts)
        assert ok.all() == valid and ok.any() == valid
        if valid:
            assert (np.hypot(out[:, 0], out[:, 1]) <= 100.0 * (2.0 / 3.0) * rf).all()


def test_no_valid_input_takes_every_step():
    """c over [-4/27, 1e6] with the double root and its neighbours (4000 mantissas in each binade and a linear sweep of
    [-4/27, 0], built without libm so that every machine sweeps the same doubles): Newton ends by its own rule after at most
    27 steps (19 for c > 0; the most at the double root, where convergence is linear) and leaves a residual
    |c s^3 + s - 1| of at most 9 x 2^-53 = 1.0e-15.  Both are the measured figures, the ones DESIGN section 5.7 gives."""
    man = np.linspace(1.0, 2.0, 4001)[:-1]
    pos = np.concatenate([np.ldexp(man, e) for e in range(-40, 20)])
    pos = pos[pos <= 1e6]
    neg = -np.concatenate([np.linspace(0.0, 4.0 / 27.0, 100001), np.array(ur.adjacent(4.0 / 27.0, 50)), pos[pos < 4.0 / 27.0]])
    for sign, cc, most in ((1.0, np.concatenate([pos, [0.0]]), 19), (-1.0, neg, 27)):
        u = np.sqrt(np.abs(cc))                                   # k = +-1, focal 1, pp 0, v = 0: c = +-(u u)
        L = ur.clens((1.0, 1.0), (0.0, 0.0), sign, ur.I2M)
        pts = np.stack([u, np.zeros_like(u)], axis=1)
        out, ok, steps = ur.shim_points(L, ur.UNDISTORT_POINTS, pts)
        assert same_points((out, ok, steps), ur.np_points(L, ur.UNDISTORT_POINTS, pts))
        ce = sign * (u * u)
        assert np.array_equal(ok, 27.0 * ce >= -4.0) and ok.sum() >= len(ok) - 60
        nz = ok & (u > 0)
        s = out[nz, 0] / u[nz]
        res = np.abs(((ce[nz] * (s * s)) * s + s) - 1.0).max()
        print("sign %+d: %d values of c, at most %d steps, residual %.3g" % (sign, int(ok.sum()), int(steps[ok].max()), res))
        assert res <= 9 * 2.0 ** -53
        assert int(steps[ok].max()) <= most < ur.MAX_STEPS


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("k", [None, 0.3])
def test_undistortion_moves_a_rendered_camera_towards_its_ideal_image(model, k):
    """Pawn camera 0 rendered ideal (I) and through the lens (D), D undistorted (U): on valid foreground pixels U is closer to
    I than D is.  An inverted model fails this.  k None: the camera's own k of the README, -0.199."""
    from pais_mvs_amd import synth
    from pais_mvs_amd.undistort import lens_of
    own = synth.PAWN_NVM[0][4]
    ideal = synth.pawn_scene(width=320, height=240, n_seeds=1, build_edges=False).cameras[0]
    cam = synth.pawn_scene(width=320, height=240, n_seeds=1, build_edges=False, distort=(model, 1.0 if k is None else k / own)).cameras[0]
    assert cam.radial_distortion == pytest.approx(own if k is None else k)
    lens = lens_of(cam, model)
    U, mask, _ = ur.shim_image(ur.clens(lens.focal, lens.pp, lens.k, lens.model), np.ascontiguousarray(cam.image))
    I, D = ideal.image.astype(np.float64), cam.image.astype(np.float64)
    fg = mask & (ideal.image > 0)
    assert fg.sum() > 2000
    eu, ed = np.abs(U.astype(np.float64) - I)[fg].mean(), np.abs(D - I)[fg].mean()
    print("model %d k %g: mean |U - I| %.3f against mean |D - I| %.3f on %d pixels" % (model, lens.k, eu, ed, int(fg.sum())))
    assert eu < ed
    # the other model's correction of the same image does worse than the right one
    wrong = ur.clens(lens.focal, lens.pp, lens.k, 1 - model)
    W_, wm, _ = ur.shim_image(wrong, np.ascontiguousarray(cam.image))
    both = fg & wm
    assert np.abs(W_.astype(np.float64) - I)[both].mean() > np.abs(U.astype(np.float64) - I)[both].mean()


def refused_calls(L, device=0):
    """Every refused input of the three entries -> [(what, rc, message)]; nothing of it may launch."""
    from pais_mvs_amd import _lib
    dp, bp = C.POINTER(C.c_double), C.POINTER(C.c_uint8)

    def lens(**kw):
        z = _lib.Lens()
        z.focal[:] = kw.get("focal", (300.0, 310.0))
        z.pp[:] = kw.get("pp", (8.0, 6.0))
        z.k, z.model = kw.get("k", -0.2), kw.get("model", 0)
        return z

    pts, out, valid = np.ones((4, 2)), np.zeros((4, 2)), np.zeros(4, np.uint8)
    nan, inf = pts.copy(), pts.copy()
    nan[2, 1], inf[1, 0] = math.nan, math.inf
    img, dst, mask = np.zeros((12, 16, 3), np.uint8), np.zeros((12, 16, 3), np.uint8), np.zeros((12, 16), np.uint8)
    bad_lenses = [("model 2", lens(model=2)), ("model -1", lens(model=-1)), ("focal 0", lens(focal=(0.0, 300.0))), ("focal1 0", lens(focal=(300.0, 0.0))),
                  ("focal nan", lens(focal=(math.nan, 1.0))), ("pp inf", lens(pp=(1.0, math.inf))), ("k nan", lens(k=math.nan)), ("k inf", lens(k=-math.inf))]
    res = []
    for name in ("pais_undistort_points", "pais_distort_points"):
        f = getattr(L, name)

        def call(dev=device, ln=lens(), n=4, i=pts, o=out, v=valid):
            return f(dev, None if ln is None else C.byref(ln), n, None if i is None else i.ctypes.data_as(dp),
                     None if o is None else o.ctypes.data_as(dp), None if v is None else v.ctypes.data_as(bp), None)
        cases = [("device < 0", dict(dev=-1)), ("null lens", dict(ln=None)), ("negative count", dict(n=-1)), ("null in", dict(i=None)),
                 ("null out", dict(o=None)), ("null valid", dict(v=None)), ("nan point", dict(i=nan)), ("inf point", dict(i=inf))]
        cases += [(w, dict(ln=z)) for w, z in bad_lenses]
        for what, kw in cases:
            res.append((name + ": " + what, call(**kw), L.pais_undistort_last_error().decode()))
        assert call(n=0) == 0 and call(n=0, i=None, o=None, v=None) == 0                # n == 0 is no error

    def image(dev=device, ln=lens(), ch=3, s=img, w=16, h=12, stride=48, d=dst, m=mask):
        return L.pais_undistort_image(dev, None if ln is None else C.byref(ln), ch, None if s is None else s.ctypes.data, w, h, stride,
                                      None if d is None else d.ctypes.data, None if m is None else m.ctypes.data, None, None)
    cases = [("device < 0", dict(dev=-1)), ("null lens", dict(ln=None)), ("null src", dict(s=None)), ("null dst", dict(d=None)),
             ("channels 2", dict(ch=2)), ("channels 4", dict(ch=4)), ("channels 0", dict(ch=0)), ("width 0", dict(w=0)), ("height 0", dict(h=0)),
             ("width -1", dict(w=-1)), ("2^31 pixels", dict(w=1 << 16, h=1 << 15, stride=3 << 16)), ("stride", dict(stride=47))]
    cases += [(w, dict(ln=z)) for w, z in bad_lenses]
    for what, kw in cases:
        res.append(("pais_undistort_image: " + what, image(**kw), L.pais_undistort_last_error().decode()))
    return res


def test_refused_inputs_launch_nothing_and_no_gpu_means_loud_failure():
    from pais_mvs_amd import _lib, undistort
    L = _lib.load()
    before = undistort.launches()
    for what, rc, err in refused_calls(L):
        assert rc < 0 and err, (what, rc, err)
    assert undistort.launches() == before
    assert L.pais_sizeof_lens() == C.sizeof(_lib.Lens) == 48
    lens = undistort.Lens(300.0, (8.0, 6.0), -0.2, "ideal-to-measured")
    assert (lens.focal[0], lens.focal[1], lens.model) == (300.0, 300.0, 1)
    with pytest.raises(ValueError):
        undistort.Lens(300.0, (8.0, 6.0), -0.2, "sideways")
    with pytest.raises(ValueError):
        undistort.undistort_image(np.zeros((4, 4, 2), np.uint8), lens)
    with pytest.raises(RuntimeError):
        undistort.undistort_points(np.ones((3, 2)), lens, device=-1)
    import torch
    if not torch.cuda.is_available():
        for call in (lambda: undistort.undistort_points(np.ones((3, 2)), lens), lambda: undistort.distort_points(np.ones((3, 2)), lens),
                     lambda: undistort.undistort_image(np.zeros((4, 4), np.uint8), lens)):
            with pytest.raises(RuntimeError):                    # no GPU: loud failure, never a host result
                call()
        assert undistort.launches() == before


def test_reconstruct_refuses_undistort_for_an_mvs_scene(tmp_path, capsys):
    from pais_mvs_amd import reconstruct
    with pytest.raises(SystemExit):
        reconstruct.main([str(tmp_path / "exp.mvs"), "--undistort", "measured-to-ideal", "--out", str(tmp_path)])
    assert "already say what they are" in capsys.readouterr().err


def test_synthetic_defaults_are_unchanged_and_measurements_follow_the_lens(pawn_small):
    """distort=None is the scene as before; with a lens the seeds are the same points and camera sets, and every measurement
    is the distorted projection of its seed: undistorting it gives the ideal projection back."""
    from pais_mvs_amd import synth
    from pais_mvs_amd.undistort import lens_of
    assert pawn_small.measurements is None
    for model in MODELS:
        s = synth.pawn_scene(width=320, height=240, n_seeds=24, distort=(model, -3.0))
        assert len(s.seeds) == len(pawn_small.seeds) == len(s.measurements)
        worst, shift = 0.0, 0.0
        for (X, vis), (X0, vis0), meas in zip(s.seeds, pawn_small.seeds, s.measurements):
            assert np.array_equal(X, X0) and vis == vis0 and meas.shape == (len(vis), 2)
            for c, uv in zip(vis, meas):
                cam = s.cameras[c]
                assert cam.radial_distortion == -3.0 * synth.PAWN_NVM[c][4]
                z = lens_of(cam, model)
                back, ok, _ = ur.shim_points(ur.clens(z.focal, z.pp, z.k, z.model), ur.UNDISTORT_POINTS, [uv])
                q = cam.rotation @ X + cam.translation
                ideal = (cam.focal[0] * q[0] / q[2] + cam.principle_point[0], cam.focal[1] * q[1] / q[2] + cam.principle_point[1])
                assert ok[0]
                worst = max(worst, float(np.abs(back[0] - ideal).max()))
                shift = max(shift, float(np.abs(uv - ideal).max()))
        assert worst <= 1e-9 and shift > 0.5            # k = 0.6, seeds within 60 pixels of the centre: about a pixel
        assert not np.array_equal(s.cameras[0].image, pawn_small.cameras[0].image)


def test_the_shim_runs_clean_under_the_sanitizers():
    """The shim with its own main, built with -fsanitize=address,undefined, as a stand-alone program over the odd sizes."""
    prog = ur.sanitized_program()                                # a build failure fails the test
    r = subprocess.run([prog], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.returncode, r.stdout[-500:], r.stderr[-2000:])
