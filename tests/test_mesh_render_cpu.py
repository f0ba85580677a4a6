"""The triangle renderer without a GPU: the statements of include/pais_render.h (TRIANGLE) as the kernels compile them
(pais_raster.hpp through tests/raster_host_shim.cpp) against their restatement (tests/raster_ref.py) bit for bit on random
soups and on dyadic edge cases, the pixel box (with it and without it the same maps), closed meshes without holes, the header's
constants, the refusals that happen before anything is launched, barycentric() against the rendered depth, the mesh readers, the
argument errors of the command lines, and the shim as a stand-alone program under the address and undefined-behaviour
sanitizers."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

from pais_mvs_amd import _lib
from pais_mvs_amd import mesh as msh
from pais_mvs_amd import render as rnd
from tests import raster_ref as rr


def test_the_array_restatement_equals_the_float_restatement():
    ver, tri = rr.soup(9, 3)
    views = rr.soup_views(2, 13, 9, 1)
    for flags in (0, rr.CULL):
        d, i = rr.render_floats(ver, tri, views, 13, 9, flags)
        wd, wi, _ = rr.render(ver, tri, views, 13, 9, flags)
        assert rr.same_maps(d, i, wd, wi) and (i >= 0).any()
    d, i = rr.render_floats(*[np.array(x) for x in rr.edge_cases()["through the camera plane"][:2]], [rr.dyadic_view()], 65, 48)
    wd, wi, _ = rr.render(*[np.array(x) for x in rr.edge_cases()["through the camera plane"][:2]], [rr.dyadic_view()], 65, 48)
    assert rr.same_maps(d, i, wd, wi)


@pytest.mark.parametrize("size", rr.SOUP_SIZES)
def test_shim_equals_the_restatement_bit_for_bit(size):
    W, H = size
    codes = np.zeros(6, np.int64)
    for nt in rr.SOUP_NT:
        for V in rr.SOUP_VIEWS:
            ver, tri = rr.soup(nt, nt + W)
            views = rr.soup_views(V, W, H, nt)
            for flags in (0, rr.CULL):
                wd, wi, wn = rr.render(ver, tri, views, W, H, flags)
                for box in (False, True):                            # the box removes no covered pixel
                    d, i, n, skips = rr.shim_render(ver, tri, views, W, H, flags, box)
                    assert rr.same_maps(d, i, wd, wi) and n == wn, (W, H, nt, V, flags, box, n, wn)
                codes += np.bincount(skips.ravel(), minlength=6)
    assert codes[rr.LIVE] > 0 and codes[rr.REPEATED] > 0 and codes[rr.CULLED] > 0 and codes[rr.OFF_IMAGE] > 0, codes


def test_edge_cases_on_dyadic_coordinates():
    rr.check_edge_cases(lambda *a: rr.shim_render(*a)[:2])
    rr.check_edge_cases(lambda *a: rr.shim_render(*a, use_box=False)[:2])


def test_closed_meshes_have_no_holes():
    """The marching-tetrahedra sphere of |p| - 1 at 17^3 (pitch h = 0.15) lies in the shell 1 - e <= |p| <= 1 with
    e = 0.02285 (raster_ref.sphere_chord_error derives it from h and R), and it is closed: a ray from outside that hits the
    sphere of radius 1 - e crosses it, front face first, between the two spheres.  Along the ray the spheres lie
    sqrt(R^2 - b^2) - sqrt((R - e)^2 - b^2) <= e / cos(incidence on the inner sphere) apart (b: the ray's distance from the
    centre; d/d rho sqrt(rho^2 - b^2) = 1 / cos falls with rho), and the camera-z differs by no more than the path.  Rays with
    cos < 0.5 on the inner sphere are excluded from the depth bound, under a quarter of those that hit (hole_views)."""
    v, t, h = rr.sphere_mesh()
    e = rr.sphere_chord_error(h)
    assert h == pytest.approx(0.15) and 0.0228 < e < 0.0229
    r = np.sqrt((v * v).sum(axis=1))
    assert r.min() >= rr.SPHERE_R - e and r.max() <= rr.SPHERE_R + 1e-12 and msh.Mesh(v, t).is_closed()
    views = rr.hole_views()
    d, i, _, _ = rr.shim_render(v, t, views, rr.HOLE_W, rr.HOLE_H, rr.CULL)
    wd, wi, _ = rr.render(v, t, views[:1], rr.HOLE_W, rr.HOLE_H, rr.CULL)
    assert rr.same_maps(d[:1], i[:1], wd, wi)
    rr.check_closed_sphere(d, i, views, rr.SPHERE_R - e, rr.SPHERE_R, e)
    # an octahedron of circumradius 1 contains the sphere of radius 1 / sqrt(3)
    ov, ot = rr.octahedron()
    d, i, _, _ = rr.shim_render(ov, ot, views, rr.HOLE_W, rr.HOLE_H, rr.CULL)
    for k, view in enumerate(views):
        t_in, _ = rr.ray_sphere(view, rr.HOLE_W, rr.HOLE_H, (1.0 - 1e-9) / math.sqrt(3.0))
        assert np.isfinite(t_in).sum() > 2000 and not (np.isfinite(t_in) & (i[k] < 0)).any()
        assert len(np.unique(i[k][i[k] >= 0])) >= 3


def test_the_headers_constants_equal_the_bindings():
    S = rr.shim()
    want = [_lib.RENDER_DISC, _lib.RENDER_POINT, _lib.RENDER_CULL_BACK, _lib.RENDER_MAX_POINT_SIZE, _lib.VIS_VISIBLE, _lib.VIS_OCCLUDED,
            _lib.VIS_IN_FRONT, _lib.VIS_EMPTY, _lib.VIS_OUTSIDE, _lib.VIS_BEHIND, _lib.VIS_SELF, C.sizeof(_lib.View)]
    assert [S.shim_constant(k) for k in range(len(want))] == want and S.shim_constant(len(want)) == -1
    assert (rr.LIVE, rr.BEHIND, rr.REPEATED, rr.CULLED, rr.FLAT, rr.OFF_IMAGE) == (0, 1, 2, 3, 4, 5)
    skips = rr.shim_render(*[np.array(x) for x in rr.edge_cases()["D == 0"][:2]], [rr.dyadic_view()], 65, 48)[3]
    assert skips.tolist() == [[rr.FLAT]]
    skips = rr.shim_render(*[np.array(x) for x in rr.edge_cases()["behind"][:2]], [rr.dyadic_view()], 65, 48)[3]
    assert skips.tolist() == [[rr.BEHIND, rr.BEHIND]]


def test_refusals_launch_nothing_and_touch_nothing():
    L = _lib.load()
    before = L.pais_render_launches()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    ver = np.array([[0.0, 0.0, 2.0], [1.0, 0.0, 2.0], [0.0, 1.0, 2.0], [1.0, 1.0, 3.0]])
    tri = np.array([[0, 1, 2], [1, 3, 2]], np.int32)
    nan_v, inf_v, bad_t, neg_t = ver.copy(), ver.copy(), tri.copy(), tri.copy()
    nan_v[2, 1], inf_v[3, 0], bad_t[1, 1], neg_t[0, 2] = float("nan"), float("inf"), 4, -1
    views = (_lib.View * 2)(rr.dyadic_view(), rr.dyadic_view())
    bad_view, zero_f = (_lib.View * 2)(rr.dyadic_view(), rr.dyadic_view()), (_lib.View * 2)(rr.dyadic_view(), rr.dyadic_view())
    bad_view[1].T[2] = float("nan")
    zero_f[0].focal[1] = 0.0
    depth, idm = np.full((2, 5, 7), 77.0), np.full((2, 5, 7), 77, np.int32)
    ok = (0, 0, 4, dp(ver), 2, ip(tri), 2, views, 7, 5, dp(depth), ip(idm), None)

    def args(**kw):
        names = ("device", "flags", "nv", "vertices", "nt", "triangles", "num_views", "views", "width", "height", "depth", "id", "ms")
        a = dict(zip(names, ok))
        a.update(kw)
        return tuple(a[k] for k in names)
    cases = [(args(nv=-1), "negative count"), (args(nt=-1), "negative count"), (args(num_views=-2), "negative count"),
             (args(width=0), "width and height"), (args(height=-3), "width and height"), (args(width=65536, height=65536), "exceeds 2^31"),
             (args(flags=2), "unknown flag bits 2"), (args(flags=_lib.VIS_SELF), "unknown flag bits"), (args(vertices=None), "null pointer"),
             (args(triangles=None), "null pointer"), (args(views=None), "null pointer"), (args(depth=None), "null pointer"),
             (args(id=None), "null pointer"), (args(device=-1), "device < 0"), (args(vertices=dp(nan_v)), "vertices[2] entry 1 is not finite"),
             (args(vertices=dp(inf_v)), "vertices[3] entry 0 is not finite"), (args(triangles=ip(bad_t)), "triangles[1] corner 1 = 4 outside [0, 4)"),
             (args(triangles=ip(neg_t)), "triangles[0] corner 2 = -1 outside"), (args(nv=3), "outside [0, 3)"),
             (args(views=bad_view), "views[1] entry 11 is not finite"), (args(views=zero_f), "focal == 0 (view 0)")]
    for a, msg in cases:
        rc = L.pais_mesh_render(*a)
        err = L.pais_render_last_error().decode()
        assert rc < 0 and err.startswith("pais_mesh_render:") and msg in err, (rc, err, msg)
    assert (depth == 77.0).all() and (idm == 77).all()

    q = np.array([[0.2, 0.2, 2.0], [0.0, 0.0, 5.0], [0.0, 0.0, 1.0]])
    nan_q = q.copy()
    nan_q[1, 2] = float("nan")
    code, occ, mar = np.full((2, 3), 77, np.uint8), np.full((2, 3), 77, np.int32), np.full((2, 3), 77.0)
    cp = code.ctypes.data_as(C.POINTER(C.c_uint8))
    vok = (0, 0, 4, dp(ver), 2, ip(tri), 3, dp(q), 2, views, 7, 5, 0.1, cp, ip(occ), dp(mar), dp(depth), ip(idm), None)

    def vargs(**kw):
        names = ("device", "flags", "nv", "vertices", "nt", "triangles", "nq", "queries", "num_views", "views", "width", "height", "tol", "code",
                 "occluder", "margin", "depth", "id", "ms")
        a = dict(zip(names, vok))
        a.update(kw)
        return tuple(a[k] for k in names)
    vcases = [(vargs(nq=-1), "negative count"), (vargs(depth=None), "both given or both NULL"), (vargs(id=None), "both given or both NULL"),
              (vargs(flags=_lib.VIS_SELF), "PAIS_VIS_SELF is refused"), (vargs(flags=_lib.VIS_SELF | 1), "PAIS_VIS_SELF is refused"),
              (vargs(flags=4), "unknown flag bits 4"), (vargs(device=-1), "device < 0"), (vargs(device=-1, depth=None, id=None), "device < 0"),
              (vargs(queries=None), "null pointer"), (vargs(code=None), "null pointer"), (vargs(tol=-1.0), "tol is negative"),
              (vargs(tol=float("nan")), "tol is negative or not finite"), (vargs(queries=dp(nan_q)), "points[1] entry 2 is not finite"),
              (vargs(triangles=ip(bad_t)), "triangles[1] corner 1 = 4"), (vargs(vertices=dp(nan_v)), "vertices[2] entry 1"),
              (vargs(views=zero_f), "focal == 0"), (vargs(nt=-1), "negative count"), (vargs(width=0), "width and height")]
    for a, msg in vcases:
        rc = L.pais_mesh_visibility(*a)
        err = L.pais_render_last_error().decode()
        assert rc < 0 and err.startswith("pais_mesh_visibility:") and msg in err, (rc, err, msg)
    assert (depth == 77.0).all() and (idm == 77).all() and (code == 77).all() and (occ == 77).all() and (mar == 77.0).all()

    # the conventions that need no device: no view touches nothing, no triangle fills the maps
    assert L.pais_mesh_render(*args(num_views=0)) == 0 and L.pais_mesh_visibility(*vargs(num_views=0)) == 0
    assert (depth == 77.0).all() and (idm == 77).all() and (code == 77).all()
    assert L.pais_mesh_render(*args(nt=0)) == 0 and np.isinf(depth).all() and (idm == -1).all()
    assert L.pais_render_launches() == before
    assert rnd.last_counts() == {"tiles": 0, "covered_pairs": 0, "depth_atomics": 0, "id_atomics": 0, "packed": 0}


def test_without_a_gpu_the_python_layer_fails_loudly():
    v, t = rr.octahedron()
    m = msh.Mesh(v, t, grid=msh.Grid([0.0, 0.0, 0.0], 0.25, (3, 3, 3)))
    views = rr.hole_views()[:1]
    before = _lib.load().pais_render_launches()
    with pytest.raises(RuntimeError, match="pais_mesh_render.*device < 0"):
        m.render(views, 32, 24, device=-1)
    with pytest.raises(RuntimeError, match="pais_mesh_render.*device < 0"):
        rnd.render_mesh(v, t, views, 32, 24, device=-1)
    with pytest.raises(RuntimeError, match="pais_mesh_visibility.*device < 0"):
        m.visibility(views, 32, 24, device=-1)
    with pytest.raises(RuntimeError, match="pais_mesh_visibility.*device < 0"):
        m.colors_from_images([_Cam(views[0])], [np.zeros((24, 32, 3), np.uint8)], device=-1)
    with pytest.raises(ValueError, match="give tol"):
        msh.Mesh(v, t).visibility(views, 32, 24, device=-1)
    for call in (lambda: rnd.render_mesh(v[:, :2], t, views, 32, 24, device=-1), lambda: rnd.render_mesh(v, t[:, :2], views, 32, 24, device=-1),
                 lambda: rnd.mesh_visibility(v, t, views, 32, 24, v[:, :2], 0.1, device=-1),
                 lambda: m.colors_from_images([], [np.zeros((24, 32, 3), np.uint8)], device=-1)):
        with pytest.raises(ValueError):
            call()
    assert _lib.load().pais_render_launches() == before


class _Cam:
    """a camera as view_of reads it"""

    def __init__(self, view):
        self.rotation, self.translation = np.array(view.R[:]).reshape(3, 3), np.array(view.T[:])
        self.focal, self.principle_point = np.array(view.focal[:]), np.array(view.pp[:])


def test_barycentric_reproduces_the_depth_bit_for_bit():
    for W, H, nt, V in ((37, 29, 300, 3), (65, 48, 7, 1)):
        ver, tri = rr.soup(nt, nt + W)
        views = rr.soup_views(V, W, H, nt)
        d, i, _, _ = rr.shim_render(ver, tri, views, W, H, 0)
        r = rnd.Render(d, i, 0.0, views)
        b = rnd.barycentric(r, ver, tri)
        assert (i >= 0).sum() > 50 and np.array_equal(b.t.view(np.uint64), d.view(np.uint64))
        w = b.weights[i >= 0]
        assert np.isnan(b.weights[i < 0]).all() and np.allclose(w.sum(axis=1), 1.0, rtol=0, atol=1e-9)
        assert (w >= 0).all()                                       # covered: the three w share the sign of S
        # interpolating the camera-space z of the corners gives the depth; a constant stays constant
        z = np.stack([np.array([rr.camera(view, p)[2] for p in ver.tolist()]) for view in views])
        for v in range(V):
            one = rnd.Render(d[v:v + 1], i[v:v + 1], 0.0, views[v:v + 1])
            bv = rnd.barycentric(one, ver, tri)
            got = one.interpolate(z[v][:, None], bv)[0, :, :, 0]
            hit = i[v] >= 0
            assert np.allclose(got[hit], d[v][hit], rtol=1e-9, atol=1e-9) and (got[~hit] == 0.0).all()
        assert np.allclose(r.interpolate(np.full((len(ver), 3), 5.0), b)[i >= 0], 5.0)
    nm = r.triangle_normals(ver, tri)
    assert nm.shape == (1, 48, 65, 3) and nm.dtype == np.uint8 and (nm[i < 0] == 0).all() and (nm[i >= 0] > 0).any()
    with pytest.raises(ValueError, match="no views"):
        rnd.barycentric(rnd.Render(d, i), ver, tri)


def test_read_ply_and_read_obj_round_trip(tmp_path):
    v, t, _ = rr.sphere_mesh()
    m = msh.Mesh(v, t)
    col = (np.arange(3 * len(v)).reshape(-1, 3) % 251).astype(np.uint8)
    m.write_ply(str(tmp_path / "a.ply"))
    m.write_ply(str(tmp_path / "c.ply"), col)
    m.write_obj(str(tmp_path / "a.obj"))
    for name, want_col in (("a.ply", None), ("c.ply", col), ("a.obj", None)):
        got, bgr = msh.read_mesh(str(tmp_path / name))
        assert np.array_equal(got.vertices.view(np.uint64), v.view(np.uint64)) and np.array_equal(got.triangles, t), name
        assert got.triangles.dtype == np.int32 and (bgr is None if want_col is None else np.array_equal(bgr, want_col)), name
    assert np.array_equal(msh.read_obj(str(tmp_path / "a.obj")).triangles, t) and msh.read_ply(str(tmp_path / "c.ply"))[1].dtype == np.uint8
    empty = msh.Mesh(np.zeros((0, 3)), np.zeros((0, 3), np.int32))
    empty.write_ply(str(tmp_path / "e.ply"))
    got, bgr = msh.read_ply(str(tmp_path / "e.ply"))
    assert got.vertices.shape == (0, 3) and got.triangles.shape == (0, 3) and bgr is None
    (tmp_path / "bad.ply").write_text("ply\nformat ascii 1.0\nelement vertex 2\nelement face 0\nend_header\n0 0 0\n")
    (tmp_path / "quad.obj").write_text("v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nf 1 2 3 4\n")
    (tmp_path / "no.ply").write_text("solid\n")
    for bad in ("bad.ply", "quad.obj", "no.ply"):
        with pytest.raises(IOError):
            msh.read_mesh(str(tmp_path / bad))
    with pytest.raises(ValueError):
        msh.read_mesh(str(tmp_path / "m.stl"))


def test_command_line_argument_errors(tmp_path, capsys):
    from pais_mvs_amd import reconstruct, view
    cloud = str(tmp_path / "cloud.npy")
    np.save(cloud, np.zeros((4, 6)))
    mesh = str(tmp_path / "m.ply")
    for bad in ([cloud, "--orbit", "2", "--mesh", str(tmp_path / "m.stl")], [cloud, "--orbit", "2", "--mesh"],
                [cloud, "--orbit", "2", "--mesh", mesh, "--mode", "point"], [cloud, "--mesh", mesh],
                [cloud, "--orbit", "2", "--mesh", mesh, "--visibility"], [cloud, "--orbit", "2", "--mesh", mesh, "--camera", "0"],
                [cloud, "--orbit", "2", "--mesh", mesh, "--pick", "3"]):
        with pytest.raises(SystemExit):
            view.parse_args(bad)
    a = view.parse_args([cloud, "--orbit", "2", "--mesh", mesh, "--pick", "3,4", "--shade", "z"])
    assert a.mesh == mesh and a.pick == (3, 4) and view.parse_args([cloud, "--orbit", "2"]).mesh is None
    for bad in (["scene.nvm", "--mesh-color"], ["cloud.mvs", "--filter", "--mesh-color"], ["cloud.mvs", "--filter", "--mesh", "--mesh-color"]):
        with pytest.raises(SystemExit):
            reconstruct.main(bad)
    capsys.readouterr()


def test_mvs_render_mesh_without_a_gpu_fails_loudly(pawn_small):
    from pais_mvs_amd.config import readme_config
    from pais_mvs_amd.mvs import MVS
    m = MVS(readme_config(), pawn_small.cameras, device=-1, seed=42)
    v, t = rr.octahedron()
    with pytest.raises(RuntimeError, match="pais_mesh_render.*device < 0"):
        m.render_mesh(msh.Mesh(v, t))
    with pytest.raises(RuntimeError, match="pais_mesh_render.*device < 0"):
        m.render_mesh(msh.Mesh(v, t), views=[0, 2])
    with pytest.raises(ValueError, match="width and height"):
        m.render_mesh(msh.Mesh(v, t), views=rr.hole_views()[:1])
    imgs = m.camera_images_bgr()
    assert len(imgs) == len(pawn_small.cameras) and all(im.shape == (240, 320, 3) and im.dtype == np.uint8 for im in imgs)
    m.close()


def test_the_shim_runs_clean_under_the_sanitizers():
    """The shim with its own main, built with -fsanitize=address,undefined, as a stand-alone program over the odd sizes."""
    prog = rr.sanitized_program()                                # a build failure fails the test
    r = subprocess.run([prog], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.returncode, r.stdout[-500:], r.stderr[-2000:])
