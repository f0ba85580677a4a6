"""The renderer's host side without a GPU: every refusal of pais_cloud_render (include/pais_render.h) before anything is
launched, the ctypes mirror of pais_view, the orbit views, the host arithmetic of a Render on hand-made maps, the command line's
arguments -- and the statements themselves, restated in numpy (tests/test_render_gpu.py: _brute), on an analytic plane."""
import ctypes as C
import math

import numpy as np
import pytest

from pais_mvs_amd import _lib
from pais_mvs_amd import render as rnd
from tests.test_render_gpu import CULL, DISC, _brute

W, H = 16, 12


def _call(L, device=0, mode=0, flags=1, n=2, centers="ok", normals="ok", radii=None, radius=0.1, num_views=1, views="ok", width=W,
          height=H, depth="ok", idm="ok"):
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    m = max(n, 1)
    cen = np.tile([0.0, 0.0, 3.0], (m, 1)) if isinstance(centers, str) else centers
    nrm = np.tile([0.0, 0.0, -1.0], (m, 1)) if isinstance(normals, str) else normals
    vs = (_lib.View * max(num_views, 1))(*[rnd.make_view(np.eye(3), np.zeros(3), (20.0, 20.0), (8.0, 6.0))] * max(num_views, 1)) if isinstance(views, str) else views
    d = np.zeros((max(num_views, 1), max(height, 1), max(width, 1)))
    i = np.zeros(d.shape, np.int32)
    ms = C.c_double(-1)
    rc = L.pais_cloud_render(device, mode, flags, n, None if cen is None else dp(np.ascontiguousarray(cen, np.float64)),
                             None if nrm is None else dp(np.ascontiguousarray(nrm, np.float64)),
                             None if radii is None else dp(np.ascontiguousarray(radii, np.float64)), radius, num_views, vs, width, height,
                             dp(d) if depth == "ok" else None, i.ctypes.data_as(C.POINTER(C.c_int32)) if idm == "ok" else None, C.byref(ms))
    return rc, L.pais_render_last_error().decode()


def _view_with(**kw):
    v = rnd.make_view(np.eye(3), np.zeros(3), (20.0, 20.0), (8.0, 6.0))
    for k, (i, x) in kw.items():
        getattr(v, k)[i] = x
    return (_lib.View * 1)(v)


def test_every_refusal_comes_with_a_message_and_launches_nothing():
    L = _lib.load()
    before = L.pais_render_launches()
    nan, inf = float("nan"), float("inf")
    bad = lambda i, j, x: np.array([[0.0, 0.0, 3.0], [0.0, 0.0, 3.0]]) + np.where((np.arange(6).reshape(2, 3) == 3 * i + j), x, 0.0)
    cases = {
        "negative n": dict(n=-1), "negative views": dict(num_views=-1),
        "null centers": dict(centers=None), "null views": dict(views=None), "null depth": dict(depth=None), "null id": dict(idm=None),
        "device": dict(device=-1),
        "width 0": dict(width=0), "height 0": dict(height=0), "width negative": dict(width=-5),
        "mode 2": dict(mode=2), "mode -1": dict(mode=-1),
        "nan centre": dict(centers=bad(1, 2, nan)), "inf centre": dict(centers=bad(0, 0, inf)),
        "nan normal": dict(normals=bad(1, 1, nan)),
        "nan radius": dict(radius=nan), "inf radius": dict(radius=inf), "nan radii": dict(radii=np.array([0.1, nan])),
        "nan R": dict(views=_view_with(R=(4, nan))), "inf T": dict(views=_view_with(T=(2, inf))), "nan pp": dict(views=_view_with(pp=(1, nan))),
        "nan focal": dict(views=_view_with(focal=(0, nan))),
        "rho 0": dict(radius=0.0), "rho negative": dict(radius=-0.1), "radii 0": dict(radii=np.array([0.1, 0.0])), "radii negative": dict(radii=np.array([-1.0, 0.1])),
        "focal 0": dict(views=_view_with(focal=(1, 0.0))),
        "disc without normals": dict(normals=None),
        "point size 0": dict(mode=1, radius=0.0), "point size 0.5": dict(mode=1, radius=0.5), "point size 65": dict(mode=1, radius=65.0),
        "point size nan": dict(mode=1, radius=nan), "point size huge": dict(mode=1, radius=1e300), "point size negative": dict(mode=1, radius=-3.0),
    }
    for what, kw in cases.items():
        rc, msg = _call(L, **kw)
        assert rc < 0 and msg.startswith("pais_cloud_render:"), (what, rc, msg)
    rc, msg = _call(L, device=-1)
    assert rc < 0 and "needs a GPU" in msg and "nothing is computed on the host" in msg
    assert L.pais_render_launches() == before


def test_view_mirror_and_constants():
    L = _lib.load()
    assert L.pais_sizeof_view() == C.sizeof(_lib.View) == 16 * 8
    hdr = open(__file__.replace("tests/test_render_cpu.py", "include/pais_render.h")).read()
    for name, val in (("PAIS_RENDER_DISC", _lib.RENDER_DISC), ("PAIS_RENDER_POINT", _lib.RENDER_POINT), ("PAIS_RENDER_CULL_BACK", _lib.RENDER_CULL_BACK),
                      ("PAIS_RENDER_MAX_POINT_SIZE", _lib.RENDER_MAX_POINT_SIZE)):
        assert ("#define %s" % name) in hdr and int(hdr.split("#define %s" % name)[1].split()[0]) == val


def test_view_of_a_camera_and_of_a_file_camera_agree():
    from pais_mvs_amd import io
    from pais_mvs_amd.camera import Camera
    q = np.array([0.705410371683, 0.160690743319, 0.671401589359, 0.160605237544])
    cen = np.array([-0.556085150075, 0.0481223921551, -0.00781510757143])
    cam = Camera(focal=np.array([300.0, 300.0]), principle_point=np.array([-1.0, -1.0]), quaternion=q, center=cen,
                 image=np.zeros((24, 32), np.uint8)).finalize(0.8, 2, build_edges=False)
    a = rnd.view_of(cam)
    b = rnd.view_of(io.io_camera("x", cam.focal, cam.principle_point, q, cen))
    assert bytes(a) == bytes(b)
    assert list(a.pp[:]) == [16.0, 12.0] and np.array_equal(np.array(a.R[:]).reshape(3, 3), cam.rotation)


def test_orbit_views():
    rng = np.random.default_rng(3)
    pts = rng.normal(size=(500, 3)) * np.array([1.0, 2.0, 0.5]) + np.array([5.0, -3.0, 2.0])
    Wd, Hd, focal = 640, 480, 700.0
    views = rnd.orbit_views(pts, 7, focal, Wd, Hd, elevation_deg=25.0)
    mid, r, dist = rnd.orbit_geometry(pts, focal, Wd, Hd)
    assert np.allclose(mid, 0.5 * (pts.min(axis=0) + pts.max(axis=0))) and len(views) == 7
    assert r >= np.linalg.norm(pts - mid, axis=1).max()
    centres = []
    for v in views:
        R, T = np.array(v.R[:]).reshape(3, 3), np.array(v.T[:])
        assert np.allclose(R @ R.T, np.eye(3), atol=1e-12) and abs(np.linalg.det(R) - 1.0) < 1e-12
        m = R @ mid + T                       # the box centre on the optical axis, in front
        assert abs(m[0]) < 1e-9 and abs(m[1]) < 1e-9 and abs(m[2] - dist) < 1e-9
        Cw = -R.T @ T
        centres.append(Cw)
        assert R[1, 2] < 0                    # image y points down: world up (z) maps to -y
        assert abs((Cw - mid)[2] / dist - math.sin(math.radians(25.0))) < 1e-12
        # the bounding sphere's outline: points of the sphere on its tangent cone project inside the frame
        k = rng.normal(size=(2000, 3))
        k /= np.linalg.norm(k, axis=1, keepdims=True)
        X = (mid + r * k) @ R.T + T
        u, w = v.focal[0] * X[:, 0] / X[:, 2] + v.pp[0], v.focal[1] * X[:, 1] / X[:, 2] + v.pp[1]
        assert (X[:, 2] > 0).all() and u.min() >= 0 and u.max() <= Wd - 1 and w.min() >= 0 and w.max() <= Hd - 1
        assert max(u.max() - v.pp[0], w.max() - v.pp[1]) > 0.8 * (Hd / 2 - 1)   # and fills it
    assert len({tuple(np.round(c, 9)) for c in centres}) == 7


def test_render_host_arithmetic_on_hand_made_maps():
    inf = np.inf
    depth = np.array([[[inf, 2.0, 3.0], [4.0, inf, 2.5]]])
    idm = np.array([[[-1, 0, 1], [2, -1, 0]]], np.int32)
    view = rnd.make_view(np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]), np.zeros(3), (10.0, 10.0), (1.0, 1.0))
    r = rnd.Render(depth, idm, 0.0, [view])
    bgr = np.array([[10, 20, 30], [40, 50, 60], [70, 80, 90]], np.uint8)
    col = r.color(bgr, background=(1, 2, 3))
    assert col.shape == (1, 2, 3, 3) and col.dtype == np.uint8
    assert col[0, 0, 0].tolist() == [1, 2, 3] and col[0, 1, 1].tolist() == [1, 2, 3]
    assert col[0, 0, 1].tolist() == [10, 20, 30] and col[0, 0, 2].tolist() == [40, 50, 60] and col[0, 1, 0].tolist() == [70, 80, 90] and col[0, 1, 2].tolist() == [10, 20, 30]
    assert r.color(bgr)[0, 0, 0].tolist() == [0, 0, 0]
    nrm = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])
    nm = r.normal_map(nrm)
    assert nm[0, 0, 0].tolist() == [0, 0, 0] and nm[0, 1, 1].tolist() == [0, 0, 0]          # empty: the background
    assert nm[0, 0, 1].tolist() == [127, 0, 127]      # n' = R (1,0,0) = (0,-1,0)
    assert nm[0, 0, 2].tolist() == [127, 127, 0]      # n' = (0,0,-1)
    assert nm[0, 1, 0].tolist() == [255, 127, 127]    # n' = R (0,1,0) = (1,0,0)
    assert r.pick(0, 0, 0) == -1 and r.pick(0, 1, 0) == 0 and r.pick(0, 2, 0) == 1 and r.pick(0, 0, 1) == 2 and r.pick(0, 1, 1) == -1
    assert r.pick(0, 3, 0) == -1 and r.pick(0, -1, 0) == -1 and r.pick(0, 0, 2) == -1
    di = r.depth_image(0)
    assert di.dtype == np.uint8 and di[0, 0] == 0 and di[1, 1] == 0 and di[0, 1] == 255 and di[1, 0] == 1 and 1 < di[0, 2] < di[1, 2] < 255
    with pytest.raises(ValueError):
        rnd.Render(depth, idm[:, :1])
    from_b, d = rnd.composite(r, rnd.Render(np.full((1, 2, 3), 2.5), np.zeros((1, 2, 3), np.int32)))
    assert from_b.tolist() == [[[True, False, True], [True, True, False]]] and d.min() == 2.0 and d.max() == 2.5


def test_the_statements_on_an_analytic_plane():
    """400 samples on a plane 3 units in front of a view and tilted by 30 degrees, exact normals, rho = 1.5 x the pitch: every
    pixel inside the sampled area is covered and each depth is the analytic ray-plane depth to 1e-12 relative -- a handful of
    2^-53 roundings with |a| about 2.6 against terms of at most 3, so nothing cancels: more than 1000 x margin."""
    Wp, Hp, focal = 48, 40, 60.0
    view = rnd.make_view(np.eye(3), np.zeros(3), (focal, focal), (float(Wp >> 1), float(Hp >> 1)))
    th = math.radians(30.0)
    e1, e2 = np.array([math.cos(th), 0.0, math.sin(th)]), np.array([0.0, 1.0, 0.0])   # the plane through (0,0,3) spanned by e1, e2
    nrm = np.cross(e1, e2)
    nrm = nrm if nrm[2] < 0 else -nrm
    p0 = np.array([0.0, 0.0, 3.0])
    pitch = 0.05
    g = (np.arange(20) - 9.5) * pitch
    a, b = np.meshgrid(g, g)
    pts = p0 + a.reshape(-1, 1) * e1 + b.reshape(-1, 1) * e2
    assert len(pts) == 400
    depth, idm = _brute(DISC, CULL, pts, np.tile(nrm, (400, 1)), 1.5 * pitch, [view], Wp, Hp)
    u, v = np.meshgrid(np.arange(Wp, dtype=np.float64), np.arange(Hp, dtype=np.float64))
    rx, ry = (u - view.pp[0]) / focal, (v - view.pp[1]) / focal
    t = (nrm @ p0) / (nrm[0] * rx + nrm[1] * ry + nrm[2])
    hit = np.stack([t * rx, t * ry, t], axis=-1) - p0
    ca, cb = hit @ e1, hit @ e2
    inside = (np.abs(ca) <= g[-1]) & (np.abs(cb) <= g[-1])
    assert inside.sum() > 300
    assert np.isfinite(depth[0][inside]).all() and (idm[0][inside] >= 0).all()
    seen = np.isfinite(depth[0])
    assert (np.abs(depth[0][seen] - t[seen]) <= 1e-12 * t[seen]).all()
    # the id is a splat whose disc holds the hit, and no pixel farther than rho outside the sampled area is covered
    far = (np.abs(ca) > g[-1] + 1.5 * pitch) | (np.abs(cb) > g[-1] + 1.5 * pitch)
    assert not seen[far].any()
    d = np.linalg.norm(np.stack([t * rx, t * ry, t], axis=-1)[seen] - pts[idm[0][seen]], axis=1)
    assert (d <= 1.5 * pitch * (1 + 1e-12)).all()
    # seen from behind, culling removes everything; without it the same depths
    assert not np.isfinite(_brute(DISC, CULL, pts, np.tile(-nrm, (400, 1)), 1.5 * pitch, [view], Wp, Hp)[0]).any()
    assert np.array_equal(_brute(DISC, 0, pts, np.tile(-nrm, (400, 1)), 1.5 * pitch, [view], Wp, Hp)[0], depth)


def test_command_line_arguments(capsys):
    from pais_mvs_amd import view
    a = view.parse_args(["c.mvs", "--camera", "0", "3", "--orbit", "4", "--out", "d", "--mode", "point", "--point-size", "5", "--pick", "10,20",
                         "--animate", "6", "--cameras"])
    assert a.cloud == "c.mvs" and a.camera == [0, 3] and a.orbit == 4 and a.out == "d" and a.mode == "point" and a.point_size == 5
    assert a.pick == (10, 20) and a.animate == 6 and a.cameras
    a = view.parse_args(["c.npy", "--orbit", "2", "--radius", "0.25"])
    assert a.mode == "disc" and a.radius == 0.25 and a.camera == [] and a.shade == "auto"
    for argv in (["c.npy", "--camera", "0"], ["c.ply", "--camera", "1", "--orbit", "3"], ["c.npy", "--orbit", "2", "--cameras"], ["c.mvs"],
                 ["c.mvs", "--orbit", "2", "--pick", "7"], ["c.mvs", "--orbit", "2", "--mode", "mesh"]):
        with pytest.raises(SystemExit) as e:
            view.parse_args(argv)
        assert e.value.code == 2, argv
    assert "has none" in capsys.readouterr().err
