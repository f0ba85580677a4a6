"""pais_mesh_render and pais_mesh_visibility on the MI355X against the restatement of their definition (tests/raster_ref.py):
random welded soups bit for bit through both walks, dyadic edge cases, closed meshes without holes, independence of the split
and of the disc renderer, the visibility entry against render + depth test, and the whole path on the small pawn scene: the
truth cloud meshed and rendered into its cameras, vertex colours from the images, the two command lines."""
import json
import os

import numpy as np
import pytest

from pais_mvs_amd import _lib
from pais_mvs_amd import mesh as msh
from pais_mvs_amd import render as rnd
from tests import pipelines
from tests import raster_ref as rr
from tests.test_knn_gpu import _loaded, grown  # noqa: F401  (the fixture: a grown cloud of the small pawn scene)

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _default_split(monkeypatch):
    for k in ("PAIS_RENDER_VIEWS", "PAIS_RENDER_SPLATS"):
        monkeypatch.delenv(k, raising=False)


def _gpu(ver, tri, views, W, H, flags=0):
    r = rnd.render_mesh(ver, tri, views, W, H, cull=bool(flags & rr.CULL))
    return r.depth, r.id


# ------------------------------------------------------------------------------------------------------ 1. bit for bit ---
@pytest.mark.parametrize("V", rr.SOUP_VIEWS)
@pytest.mark.parametrize("nt", rr.SOUP_NT)
@pytest.mark.parametrize("W,H", rr.SOUP_SIZES)
def test_random_soups_equal_the_brute_force_bit_for_bit(W, H, nt, V):
    ver, tri = rr.soup(nt, nt + W)
    views = rr.soup_views(V, W, H, nt)
    for flags in (0, rr.CULL):
        wd, wi, wn = rr.render(ver, tri, views, W, H, flags)
        r = rnd.render_mesh(ver, tri, views, W, H, cull=bool(flags))
        assert rr.same_maps(r.depth, r.id, wd, wi), (W, H, nt, V, flags, int((r.id != wi).sum()))
        assert r.counts["covered_pairs"] == wn and r.counts["depth_atomics"] <= wn and r.kernel_ms > 0
        if nt >= 300:                                               # sizes are mixed: both walks ran
            assert r.counts["packed"] > 0 and r.counts["tiles"] > 0, r.counts
        ms = rnd.mesh_last_ms()
        assert ms["setup"] > 0 and ms["depth"] > 0 and ms["id"] > 0


def test_edge_cases_on_dyadic_coordinates():
    rr.check_edge_cases(_gpu)


def test_a_small_box_across_tile_edges_takes_the_packed_walk():
    """a triangle of three pixels around (32, 32) of the 65 x 48 image: its box crosses the 32-pixel lines and is packed"""
    ver = np.array([rr.at_pixel(31, 31), rr.at_pixel(33, 31), rr.at_pixel(32, 33), rr.at_pixel(63, 46), rr.at_pixel(64, 46), rr.at_pixel(64, 47)])
    tri = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    view = rr.dyadic_view()
    r = rnd.render_mesh(ver, tri, [view], 65, 48, cull=False)
    wd, wi, _ = rr.render(ver, tri, [view], 65, 48, 0)
    assert rr.same_maps(r.depth, r.id, wd, wi) and r.counts["packed"] == 2 and r.counts["tiles"] == 0
    assert r.id[0, 31, 31] == 0 and r.id[0, 33, 32] == 0 and r.id[0, 47, 64] == 1 and r.id[0, 46, 63] == 1


# ---------------------------------------------------------------------------------------------------- 2. closed meshes ---
def test_closed_meshes_have_no_holes():
    """test_mesh_render_cpu.test_closed_meshes_have_no_holes on the GPU: the 17^3 marching-tetrahedra sphere lies in the shell
    1 - e <= |p| <= 1 with e = 0.02285 from the pitch 0.15 (raster_ref.sphere_chord_error), so every ray that hits the sphere
    of radius 1 - e is covered, and where its incidence there has cos >= 0.5 the depth lies within e / cos of the analytic
    depth on the unit sphere; under a quarter of the hitting rays are excluded as grazing (raster_ref.hole_views)."""
    v, t, h = rr.sphere_mesh()
    e = rr.sphere_chord_error(h)
    views = rr.hole_views()
    r = rnd.render_mesh(v, t, views, rr.HOLE_W, rr.HOLE_H, cull=True)
    rr.check_closed_sphere(r.depth, r.id, views, rr.SPHERE_R - e, rr.SPHERE_R, e)
    d, i, _, _ = rr.shim_render(v, t, views, rr.HOLE_W, rr.HOLE_H, rr.CULL)
    assert rr.same_maps(r.depth, r.id, d, i)
    ov, ot = rr.octahedron()
    r = rnd.render_mesh(ov, ot, views, rr.HOLE_W, rr.HOLE_H, cull=True)
    for k, view in enumerate(views):
        t_in, _ = rr.ray_sphere(view, rr.HOLE_W, rr.HOLE_H, (1.0 - 1e-9) / np.sqrt(3.0))
        assert np.isfinite(t_in).sum() > 2000 and not (np.isfinite(t_in) & (r.id[k] < 0)).any()


# ------------------------------------------------------------------------------------------------------- 3. the split ---
def test_the_output_does_not_depend_on_the_split(monkeypatch):
    W, H = 65, 48
    ver, tri = rr.soup(5000, 77)
    views = rr.soup_views(3, W, H, 5)
    wd, wi, _ = rr.render(ver, tri, views, W, H, rr.CULL)
    # a disc case before and after
    rng = np.random.default_rng(9)
    c = rng.uniform(-1.0, 1.0, (500, 3))
    n = rng.normal(size=(500, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    disc = rnd.render(c, n, views, W, H, radius=0.08, cull_back=False)
    first = rnd.render_mesh(ver, tri, views, W, H)
    assert rr.same_maps(first.depth, first.id, wd, wi)
    for nviews in (None, "1", "2"):
        for splats in (None, "7", "64", "1000"):
            env = {k: v for k, v in (("PAIS_RENDER_VIEWS", nviews), ("PAIS_RENDER_SPLATS", splats)) if v is not None}
            with pipelines.knobs(monkeypatch, env):
                got = rnd.render_mesh(ver, tri, views, W, H)
            assert got.depth.tobytes() == first.depth.tobytes() and got.id.tobytes() == first.id.tobytes(), env
            assert got.counts["covered_pairs"] == first.counts["covered_pairs"], env
    again = rnd.render(c, n, views, W, H, radius=0.08, cull_back=False)
    assert again.depth.tobytes() == disc.depth.tobytes() and again.id.tobytes() == disc.id.tobytes() and (disc.id >= 0).sum() > 500
    assert again.counts["packed"] == 0 and again.counts["tiles"] == disc.counts["tiles"]


# ------------------------------------------------------------------------------------------------------- 4. visibility ---
def test_mesh_visibility_equals_render_then_depth_test(monkeypatch):
    W, H = 65, 48
    ver, tri = rr.soup(300, 21)
    views = rr.soup_views(3, W, H, 2)
    rng = np.random.default_rng(4)
    q = np.concatenate([ver[:40], rng.uniform(-1.5, 1.5, (160, 3))])
    for cull in (True, False):
        r = rnd.render_mesh(ver, tri, views, W, H, cull=cull)
        want = rnd.depth_test(q, views, r.depth, r.id, tol=0.05)
        for env in ({}, {"PAIS_RENDER_VIEWS": "2"}):
            with pipelines.knobs(monkeypatch, env):
                kept = rnd.mesh_visibility(ver, tri, views, W, H, q, 0.05, cull=cull, keep_maps=True)
                bare = rnd.mesh_visibility(ver, tri, views, W, H, q, 0.05, cull=cull)
            assert kept.render.depth.tobytes() == r.depth.tobytes() and kept.render.id.tobytes() == r.id.tobytes()
            assert bare.render is None
            for got in (kept, bare):
                assert got.code.tobytes() == want.code.tobytes() and got.occluder.tobytes() == want.occluder.tobytes()
                assert got.margin.tobytes() == want.margin.tobytes()
                assert got.ms["render"] > 0 and got.ms["test"] > 0 and got.kernel_ms == pytest.approx(got.ms["render"] + got.ms["test"])
        assert len(np.unique(want.code)) >= 4
    L = _lib.load()
    before = L.pais_render_launches()
    with pytest.raises(RuntimeError, match="PAIS_VIS_SELF is refused"):
        _self_call(L, ver, tri, q, views, W, H)
    assert L.pais_render_launches() == before
    none = rnd.mesh_visibility(ver, tri, views, W, H, np.zeros((0, 3)), 0.05, keep_maps=True)       # nq == 0 renders
    assert none.code.shape == (3, 0) and none.render.depth.tobytes() == rnd.render_mesh(ver, tri, views, W, H).depth.tobytes()


def _self_call(L, ver, tri, q, views, W, H):
    import ctypes as C
    ver, tri, q = np.ascontiguousarray(ver), np.ascontiguousarray(tri, np.int32), np.ascontiguousarray(q)
    code = np.zeros((len(views), len(q)), np.uint8)
    arr = (_lib.View * len(views))(*views)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    rc = L.pais_mesh_visibility(0, _lib.VIS_SELF, len(ver), dp(ver), len(tri), tri.ctypes.data_as(C.POINTER(C.c_int32)), len(q), dp(q), len(views),
                                arr, W, H, 0.05, code.ctypes.data_as(C.POINTER(C.c_uint8)), None, None, None, None, None)
    if rc:
        raise RuntimeError(L.pais_render_last_error().decode())


def test_the_spheres_own_vertices_near_and_far():
    """at tol = h / 2 a vertex of the sphere mesh on the side of the camera is VISIBLE, one on the far side OCCLUDED (the near
    surface lies about 2 R in front of it); `near` and `far` leave out the belt around the silhouette, where the pixel's ray
    meets a neighbouring triangle up to a pixel away at a grazing angle"""
    v, t, h = rr.sphere_mesh()
    m = msh.Mesh(v, t, grid=msh.Grid([0.0, 0.0, 0.0], h, (17, 17, 17)))
    views = rr.hole_views()
    vis = m.visibility(views, rr.HOLE_W, rr.HOLE_H)
    assert vis.code.shape == (3, len(v)) and vis.occluder.max() < len(t)
    for k, view in enumerate(views):
        R, T = np.array(view.R[:]).reshape(3, 3), np.array(view.T[:])
        eye = -R.T @ T
        cos = (v @ eye) / (np.linalg.norm(v, axis=1) * np.linalg.norm(eye))           # > 1 / 3: the vertex faces the camera at distance 3
        inside = vis.code[k] != _lib.VIS_OUTSIDE
        near, far = inside & (cos > 0.6), inside & (cos < 0.0)
        assert near.sum() > 100 and far.sum() > 100
        assert (vis.code[k][near] == _lib.VIS_VISIBLE).all(), np.bincount(vis.code[k][near], minlength=6)
        assert (vis.code[k][far] == _lib.VIS_OCCLUDED).all(), np.bincount(vis.code[k][far], minlength=6)


# ------------------------------------------------------------------------------------------------------ 5. end to end ---
@pytest.fixture(scope="module")
def truth_mesh(pawn_small):
    """the truth cloud of the small pawn scene at stride 2, meshed at the pitch of its own sampling: (points, normals, spacing,
    Mesh).  `spacing` is the pitch the truth was sampled at, the radius test_render_gpu.py gives its discs; the truth is sampled
    more densely along the profile than around the axis, so the mesher's default pitch -- twice the median nearest-neighbour
    distance, 0.00375 here against a spacing of 0.0068 -- truncates the field between the rows of samples and leaves holes there
    (seen on the MI355X at that pitch: 5450 of 29745 silhouette pixels empty, the disc render 4840)."""
    from pais_mvs_amd import synth
    pts, nrm, spacing = synth.ground_truth(pawn_small, stride=2)
    return pts, nrm, spacing, msh.mesh(np.concatenate([pts, nrm], axis=1), h=spacing)


def test_the_pawn_truth_mesh_rendered_into_its_own_cameras(pawn_small, truth_mesh):
    """Inside the object's silhouette (the analytic depth of the solid is finite) the mesh's depth maps leave no more pixels
    empty than the disc render of the same cloud at radius `spacing`; both numbers are printed."""
    from tests.test_render_gpu import truth_depth
    pts, nrm, spacing, m = truth_mesh
    cams = pawn_small.cameras
    views = [rnd.view_of(cam) for cam in cams]
    W, H = cams[0].width, cams[0].height
    discs = rnd.render(pts, nrm, views, W, H, radius=spacing)
    r = m.render(views, W, H)
    maps = m.depth_maps(cams)
    assert len(maps) == len(cams) and all(np.array_equal(a.view(np.uint64), b.view(np.uint64)) for a, b in zip(maps, r.depth))
    assert r.id.max() < len(m.triangles) and np.array_equal(r.id >= 0, np.isfinite(r.depth)) and r.counts["packed"] > 0
    sil = np.stack([np.isfinite(truth_depth(pawn_small, cam)) for cam in cams])
    empty_mesh, empty_disc = int((sil & (r.id < 0)).sum()), int((sil & (discs.id < 0)).sum())
    print("\npawn truth: %d points, %d triangles at pitch %.6g; of %d silhouette pixels %d empty in the mesh render, %d in the disc render; "
          "kernel ms %.3f (mesh) %.3f (discs)" % (len(pts), len(m.triangles), m.grid.h, int(sil.sum()), empty_mesh, empty_disc, r.kernel_ms,
                                                  discs.kernel_ms))
    assert empty_mesh <= empty_disc
    b = rnd.barycentric(r, m.vertices, m.triangles)
    assert np.array_equal(b.t.view(np.uint64), r.depth.view(np.uint64))


def test_colors_from_images(pawn_small, truth_mesh):
    pts, nrm, spacing, m = truth_mesh
    cams = pawn_small.cameras
    rng = np.random.default_rng(12)
    images = [rng.integers(0, 256, (cam.height, cam.width, 3), dtype=np.uint8) for cam in cams]
    col = m.colors_from_images(cams, images, fallback=(1, 2, 3))
    views = [rnd.view_of(cam) for cam in cams]
    vis = m.visibility(views, cams[0].width, cams[0].height)
    seen = (vis.code == _lib.VIS_VISIBLE).sum(axis=0)
    assert col.shape == (len(m.vertices), 3) and col.dtype == np.uint8 and (seen > 0).sum() > len(m.vertices) // 2
    assert (col[seen == 0] == (1, 2, 3)).all()
    several = np.flatnonzero(seen >= 2)
    for i in (several[0], several[len(several) // 2], np.flatnonzero(seen == 1)[0] if (seen == 1).any() else several[-1]):
        total, k = np.zeros(3), 0
        for j, cam in enumerate(cams):                              # by hand: project_raw, cvRound, the pixel's BGR
            if vis.code[j, i] != _lib.VIS_VISIBLE:
                continue
            p, R = m.vertices[i], cam.rotation
            x = [((R[r, 0] * p[0] + R[r, 1] * p[1]) + R[r, 2] * p[2]) + cam.translation[r] for r in range(3)]
            u = int(np.rint(cam.focal[0] * (x[0] / x[2]) + cam.principle_point[0]))
            v = int(np.rint(cam.focal[1] * (x[1] / x[2]) + cam.principle_point[1]))
            total += images[j][v, u]
            k += 1
        assert k == seen[i] and col[i].tolist() == np.rint(total / k).astype(np.uint8).tolist(), (i, k)
    # the default fallback: the nearest patch's colour when a cloud is given, black otherwise
    bgr = rng.integers(0, 256, (len(pts), 3), dtype=np.uint8)
    with_cloud = m.colors_from_images(cams, images, cloud_bgr=bgr, centers=pts)
    assert np.array_equal(with_cloud[seen > 0], col[seen > 0]) and np.array_equal(with_cloud[seen == 0], m.colors(bgr, pts)[seen == 0])
    assert (m.colors_from_images(cams, images)[seen == 0] == 0).all()


def test_view_command_line_draws_the_mesh(pawn_small, truth_mesh, tmp_path, capsys):
    from PIL import Image
    from pais_mvs_amd import view
    pts, nrm, spacing, m = truth_mesh
    cloud, out = str(tmp_path / "cloud.npy"), str(tmp_path / "out")
    np.save(cloud, np.concatenate([pts, nrm], axis=1))
    col = (np.arange(3 * len(m.vertices)).reshape(-1, 3) % 200 + 30).astype(np.uint8)
    m.write_ply(str(tmp_path / "m.ply"), col)
    m.write_obj(str(tmp_path / "m.obj"))
    views = rnd.orbit_views(pts, 2, 1.2 * 160, 160, 120, 20.0)
    want = m.render(views, 160, 120)
    vv, uu = np.argwhere(want.id[0] >= 0)[len(np.argwhere(want.id[0] >= 0)) // 2]
    for name, shade in (("m.ply", "color"), ("m.obj", "normal"), ("m.ply", "z")):
        capsys.readouterr()
        assert view.main([cloud, "--mesh", str(tmp_path / name), "--orbit", "2", "--width", "160", "--height", "120", "--out", out, "--shade", shade,
                          "--pick", "%d,%d" % (uu, vv), "--animate", "2"]) == 0
        line = json.loads(capsys.readouterr().out.strip().split("\n")[-1])
        assert line["mode"] == "mesh" and line["triangles"] == len(m.triangles) and line["covered_pixels"] == int((want.id >= 0).sum())
        assert line["pick"]["triangle"] == int(want.id[0, vv, uu]) and sum(line["pick"]["barycentric"]) == pytest.approx(1.0)
        assert line["pick"]["depth"] == want.depth[0, vv, uu]
        for k in range(2):
            with Image.open(os.path.join(out, "view_%03d.png" % k)) as im:
                assert im.size == (160, 120) and np.asarray(im)[want.id[k] >= 0].any() and not np.asarray(im)[want.id[k] < 0].any()
            d = np.load(os.path.join(out, "depth_%03d.npy" % k))
            assert np.array_equal(d.view(np.uint64), want.depth[k].view(np.uint64))
            assert os.path.exists(os.path.join(out, "anim_%03d.png" % k))
    with pytest.raises(SystemExit, match="no vertex colours"):
        view.main([cloud, "--mesh", str(tmp_path / "m.obj"), "--orbit", "1", "--out", out, "--shade", "color"])


def test_view_visibility_and_reconstructs_mesh_color(pawn_small, grown, tmp_path, capsys):
    from pais_mvs_amd import reconstruct, view
    cfg, cl = grown
    m = _loaded(cfg, pawn_small.cameras, cl)
    mesh = reconstruct.write_mesh(m, str(tmp_path / "mesh.ply"), None, True)
    got, bgr = msh.read_ply(str(tmp_path / "mesh.ply"))
    want = mesh.colors_from_images(m.cameras, m.camera_images_bgr(), cloud_bgr=m.colors_bgr(), centers=m.cloud()[:, :3])
    assert np.array_equal(got.triangles, mesh.triangles) and np.array_equal(bgr, want)
    nearest = mesh.colors(m.colors_bgr(), m.cloud()[:, :3])
    assert (bgr != nearest).any()                                   # the images, not the nearest patch
    r = m.render_mesh(mesh, views=[0, 1])
    assert r.depth.shape == (2, 240, 320) and (r.id >= 0).any()
    # view --mesh --visibility: the cloud's points against the mesh, per camera of the .mvs file
    mvs, out = str(tmp_path / "exp.mvs"), str(tmp_path / "out")
    m.writeMVS(mvs)
    capsys.readouterr()
    assert view.main([mvs, "--mesh", str(tmp_path / "mesh.ply"), "--camera", "0", "2", "--out", out, "--visibility", "--radius", str(mesh.grid.h)]) == 0
    line = json.loads(capsys.readouterr().out.strip().split("\n")[-1])
    rows = line["visibility"]
    assert [row["camera"] for row in rows] == [0, 2] and all(sum(row[k] for k in rnd.VIS_CODES) == line["n"] for row in rows)
    assert line["n"] > 0 and all(row["visible"] > 0 for row in rows) and os.path.exists(os.path.join(out, "view_001.png"))
    m.close()
