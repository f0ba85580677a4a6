"""The mesher without a GPU: the statements of include/pais_mesh.h as the kernels compile them (pais_mesh.hpp through
tests/mesh_host_shim.cpp) against their restatement with Python floats (tests/mesh_ref.py) bit for bit, the orientation table
derived again, analytic fields through the surface stage (closed, Euler characteristic, volume, exact plane), empty and partial
surfaces, the key identity, the host weld, the capacity protocol, the refusals that happen before anything is launched, the
argument errors of the two command lines, a sampled sphere, and the shim as a stand-alone program under the address and
undefined-behaviour sanitizers."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

from pais_mvs_amd import mesh as msh
from tests import knn_ref
from tests import mesh_ref as mr

# |volume - 4 pi / 3| / (4 pi / 3) of the sampled sphere (800 Fibonacci points, 17^3, k = 8, support 3 h, trunc 2 h) and of the
# analytic sphere field at 17^3 as the restatement gives them, and the factor asserted over them: the
# error is a property of the definition (pitch and weights), not of rounding, so the code under test may differ from the seen
# value by rounding only; the factor leaves room for a change of the case generators, not of the code.
VOLUME_SEEN = {"sampled": 0.017031, "analytic": 0.011268}
VOLUME_FACTOR = 1.25
SPHERE = 4.0 * math.pi / 3.0


def _welded(keys, xyz, grid=None):
    v, t, k = msh.weld(keys, xyz)
    return msh.Mesh(v, t, k, None, grid)


@pytest.fixture(scope="module")
def cases():
    """name -> (grid, field, count, keys, xyz) through the shim"""
    return {name: (g, f) + mr.shim_surface(g, f) for name, (g, f) in mr.surface_cases().items()}


@pytest.fixture(scope="module")
def sampled():
    """the sampled sphere at trunc = 2 h: (grid, field by the restatement, field by the shim)"""
    grid, c, n, k, support, trunc = mr.sampled_sphere()
    idx, d2 = mr.field_table(grid, c, k)
    return grid, mr.ref_field(grid, idx, d2, c, n, support, trunc), mr.shim_field(grid, idx, d2, c, n, support, trunc)


@pytest.mark.parametrize("n", mr.FIELD_GRIDS)
def test_field_shim_equals_the_restatement_bit_for_bit(n):
    seen_nan = seen_value = 0
    for nt in mr.FIELD_CLOUDS:
        for k in mr.FIELD_KS:
            grid, c, nrm, support, trunc = mr.field_case(n, nt, k)
            idx, d2 = mr.field_table(grid, c, k)
            got = mr.shim_field(grid, idx, d2, c, nrm, support, trunc)
            want = mr.ref_field(grid, idx, d2, c, nrm, support, trunc)
            assert knn_ref.same_doubles(got, want), (n, nt, k)
            seen_nan += int(np.isnan(got).sum())
            seen_value += int(np.isfinite(got).sum())
            assert not np.isinf(got).any()
    assert seen_value > 0 and (n == (2, 2, 2) or seen_nan > 0)


def test_field_edge_cases_from_dyadic_coordinates():
    """a neighbour at exactly d2 == r2 is skipped; a vertex at exactly d2_0 == trunc * trunc is kept"""
    grid = mr.Grid([0.0, 0.0, 0.0], 1.0, (2, 2, 2))
    # vertex (0,0,0): the nearest point at distance 0.5 along x (d2 = 0.25), a second at distance exactly 2 = support along y
    c = np.array([[0.5, 0.0, 0.0], [0.0, 2.0, 0.0]])
    nrm = np.array([[1.0, 0.0, 0.0], [0.0, 64.0, 0.0]])          # the skipped one would dominate the sum
    idx, d2 = mr.field_table(grid, c, 2)
    assert idx[0].tolist() == [0, 1] and d2[0].tolist() == [0.25, 4.0]
    for fn in (mr.shim_field, mr.ref_field):
        f = fn(grid, idx, d2, c, nrm, 2.0, 1.5)
        assert f[0] == -0.5                                       # (w * -0.5) / w with the one weight alone
    inside = mr.shim_field(grid, idx, d2, c, nrm, 2.5, 1.5)
    assert inside[0] < -1.0                                       # with more support it takes part, and dominates
    # trunc exactly 0.5: d2_0 == trunc * trunc is kept; a hair less and the vertex is NaN
    for fn in (mr.shim_field, mr.ref_field):
        assert fn(grid, idx, d2, c, nrm, 2.0, 0.5)[0] == -0.5
        assert math.isnan(fn(grid, idx, d2, c, nrm, 2.0, 0.5 - 2.0 ** -40)[0])


def test_the_headers_tables_equal_the_derived_ones():
    S = mr.shim()
    flip = mr.derive_flip_table()
    for t in range(6):
        assert [S.shim_mesh_tet_corner(t, j) for j in range(4)] == list(mr.TETS[t])
        for mask in range(16):
            assert S.shim_mesh_count(mask) == len(mr.case_edges(mask)), mask
            if 1 <= mask <= 14:
                assert bool(S.shim_mesh_flip(t, mask)) == flip[t][mask], (t, mask)
    bits = [sum(1 << m for m in range(1, 15) if flip[t][m]) for t in range(6)]
    assert bits[0] == bits[3] == bits[4] and bits[1] == bits[2] == bits[5] and bits[0] ^ bits[1] == 0x7FFE
    # every edge of the split runs from a corner to one whose offset bits contain its own: the lower grid index comes first
    for tet in mr.TETS:
        assert all((tet[p] & tet[q]) == tet[p] for p in range(4) for q in range(p + 1, 4))


def test_surface_shim_equals_the_restatement_bit_for_bit(cases):
    for name, (grid, f, count, keys, xyz) in cases.items():
        rk, rx = mr.ref_surface(grid, f)
        assert count == len(rk) == len(keys), name
        assert np.array_equal(keys, rk) and knn_ref.same_doubles(xyz, rx), name


@pytest.mark.parametrize("name,triangles,chi", [("sphere 9x9x9", 1264, 2), ("sphere 17x13x11", 1936, 2), ("torus", 5436, 0)])
def test_analytic_surfaces_are_closed(cases, name, triangles, chi):
    grid, f, count, keys, xyz = cases[name]
    m = _welded(keys, xyz)
    print("\n%s: %d triangles, %d vertices, volume %.6f, area %.6f" % (name, count, len(m.vertices), m.volume(), m.area()))
    assert triangles is None or count == triangles
    assert mr.is_closed(m.triangles) and m.is_closed() and len(m.boundary_edges()) == 0
    assert mr.euler(len(m.vertices), m.triangles) == m.euler() == chi
    assert m.volume() > 0 and m.volume() == pytest.approx(mr.volume(m.vertices, m.triangles), rel=1e-12)


def test_the_cube_grid_sphere_of_the_prototype_and_its_volume():
    grid = mr.analytic_grid((17, 17, 17))
    count, keys, xyz = mr.shim_surface(grid, mr.sphere_field(grid))
    m = _welded(keys, xyz)
    err = abs(m.volume() - SPHERE) / SPHERE
    print("\nanalytic sphere 17^3: %d triangles, volume %.6f, relative error %.5f" % (count, m.volume(), err))
    assert count == 5036 and m.is_closed() and m.euler() == 2
    assert err <= VOLUME_FACTOR * VOLUME_SEEN["analytic"]


def test_the_plane_with_exact_zeros_at_vertices(cases):
    grid, f, count, keys, xyz = cases["plane"]
    m = _welded(keys, xyz)
    assert count == 200 and m.area() == 25.0
    assert (m.vertices[:, 2] == 2.0).all() and (xyz[:, :, 2] == 2.0).all()
    a, b, c = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    nz = np.cross(b - a, c - a)[:, 2]
    assert (nz >= 0).all() and 0 < (nz == 0).sum() < count       # the degenerate ones are kept; the others face +z (outside)


def test_empty_and_partial_surfaces(cases):
    for name in ("all positive", "all negative", "all nan"):
        assert cases[name][2] == 0, name
    grid, f, count, keys, xyz = cases["nan band"]
    m = _welded(keys, xyz)
    assert 0 < count < cases["sphere 9x9x9"][2] and not m.is_closed() and len(m.boundary_edges()) > 0


def test_equal_keys_have_equal_position_bits(cases):
    for name, (grid, f, count, keys, xyz) in cases.items():
        if not count:
            continue
        k, p = keys.reshape(-1), xyz.reshape(-1, 3).view(np.uint64)
        order = np.argsort(k, kind="stable")
        k, p = k[order], p[order]
        same = k[1:] == k[:-1]
        assert same.any() and (p[1:][same] == p[:-1][same]).all(), name
        assert (k % 8 >= 1).all() and (k // 8 < grid.num_vertices()).all(), name


def test_weld_against_numpy_unique(cases):
    for name in ("sphere 9x9x9", "nan band", "plane"):
        grid, f, count, keys, xyz = cases[name]
        v, t, vk = msh.weld(keys, xyz)
        uk, first, inverse = np.unique(keys.reshape(-1), return_index=True, return_inverse=True)
        assert np.array_equal(vk, uk) and t.dtype == np.int32 and np.array_equal(t.reshape(-1), inverse)
        assert knn_ref.same_doubles(v, xyz.reshape(-1, 3)[first]), name
        rv, rt = mr.ref_weld(keys, xyz)
        assert knn_ref.same_doubles(v, rv) and np.array_equal(t, rt), name
    v, t, vk = msh.weld(np.zeros((0, 3), np.int64), np.zeros((0, 3, 3)))
    assert v.shape == (0, 3) and t.shape == (0, 3) and len(vk) == 0
    # first occurrence: two corners with one key and different positions (never from the surface stage) -> the first one's
    keys = np.array([[9, 17, 25], [25, 9, 33]], np.int64)
    xyz = np.arange(18.0).reshape(2, 3, 3)
    v, t, vk = msh.weld(keys, xyz)
    assert vk.tolist() == [9, 17, 25, 33] and t.tolist() == [[0, 1, 2], [2, 0, 3]]
    assert v.tolist() == [[0.0, 1.0, 2.0], [3.0, 4.0, 5.0], [6.0, 7.0, 8.0], [15.0, 16.0, 17.0]]


def test_weld_capacity_and_refusals():
    from pais_mvs_amd import _lib
    L = _lib.load()
    keys = np.array([[9, 17, 25], [25, 9, 33]], np.int64)
    xyz = np.arange(18.0).reshape(2, 3, 3)
    kp, xp = keys.ctypes.data_as(C.POINTER(C.c_int64)), xyz.ctypes.data_as(C.POINTER(C.c_double))
    n = C.c_int64(-1)
    assert L.pais_mesh_weld(2, kp, xp, C.byref(n), 0, None, None) == 0 and n.value == 4          # counts only
    v, t = np.full((4, 3), 77.0), np.full((2, 3), 77, np.int32)
    vp, tp = v.ctypes.data_as(C.POINTER(C.c_double)), t.ctypes.data_as(C.POINTER(C.c_int32))
    for args, msg in (((-1, kp, xp, C.byref(n), 0, None, None), "negative count"), ((2, kp, xp, C.byref(n), -1, vp, tp), "negative count"),
                      ((2, None, xp, C.byref(n), 4, vp, tp), "null pointer"), ((2, kp, None, C.byref(n), 4, vp, tp), "null pointer"),
                      ((2, kp, xp, None, 4, vp, tp), "null pointer"), ((2, kp, xp, C.byref(n), 4, None, tp), "null vertices or triangles"),
                      ((2, kp, xp, C.byref(n), 4, vp, None), "null vertices or triangles"), ((2, kp, xp, C.byref(n), 3, vp, tp), "below the 4 distinct keys")):
        assert L.pais_mesh_weld(*args) < 0
        err = L.pais_mesh_last_error().decode()
        assert err.startswith("pais_mesh_weld:") and msg in err, (err, msg)
    assert (v == 77.0).all() and (t == 77).all() and n.value == 4
    assert L.pais_mesh_weld(0, None, None, C.byref(n), 0, None, None) == 0 and n.value == 0


def test_capacity_protocol_of_the_shim(cases):
    grid, f, count, keys, xyz = cases["sphere 9x9x9"]
    n0, k0, x0 = mr.shim_surface(grid, f, 0)
    assert n0 == count and len(k0) == 0
    n1, k1, x1 = mr.shim_surface(grid, f, count - 1)
    assert n1 == count and np.array_equal(k1, keys[:-1]) and knn_ref.same_doubles(x1, xyz[:-1])
    n2, k2, x2 = mr.shim_surface(grid, f, count + 5)
    assert n2 == count and np.array_equal(k2[:count], keys) and (k2[count:] == -7).all() and (x2[count:] == -7.0).all()


def test_refusals_launch_nothing_and_touch_nothing():
    """every refusal of pais_cloud_field and pais_field_surface; none of them needs a GPU"""
    from pais_mvs_amd import _lib
    L = _lib.load()
    assert L.pais_sizeof_grid() == C.sizeof(_lib.Grid) == C.sizeof(mr.CGrid) == 48 and _lib.MESH_MAX_VERTICES == 2 ** 28
    before = (L.pais_mesh_launches(), L.pais_cloud_launches())
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    grid = lambda origin=(0.0, 0.0, 0.0), h=1.0, n=(3, 3, 3): C.byref(_lib.Grid((C.c_double * 3)(*origin), h, (C.c_int32 * 3)(*n), 0))
    cen, nrm = np.zeros((4, 3)), np.tile([0.0, 0.0, 1.0], (4, 1))
    out = np.full(27, 77.0)
    nan_c, inf_n = cen.copy(), nrm.copy()
    nan_c[2, 1], inf_n[3, 0] = float("nan"), float("inf")
    nan, inf = float("nan"), float("inf")
    good = grid()
    for args, msg in [((0, 8, None, 4, dp(cen), dp(nrm), 3.0, 2.0, dp(out), None), "null pointer"),
                      ((0, 8, good, 4, None, dp(nrm), 3.0, 2.0, dp(out), None), "null pointer"),
                      ((0, 8, good, 4, dp(cen), None, 3.0, 2.0, dp(out), None), "null pointer"),
                      ((0, 8, good, 4, dp(cen), dp(nrm), 3.0, 2.0, None, None), "null pointer"),
                      ((0, 8, grid(h=0.0), 4, dp(cen), dp(nrm), 3.0, 2.0, dp(out), None), "grid h"),
                      ((0, 8, grid(h=-1.0), 4, dp(cen), dp(nrm), 3.0, 2.0, dp(out), None), "grid h"),
                      ((0, 8, grid(h=nan), 4, dp(cen), dp(nrm), 3.0, 2.0, dp(out), None), "grid h"),
                      ((0, 8, grid(h=inf), 4, dp(cen), dp(nrm), 3.0, 2.0, dp(out), None), "grid h"),
                      ((0, 8, grid(n=(3, 1, 3)), 4, dp(cen), dp(nrm), 3.0, 2.0, dp(out), None), "n[1] = 1 is below 2"),
                      ((0, 8, grid(n=(1024, 1024, 257)), 4, dp(cen), dp(nrm), 3.0, 2.0, dp(out), None), "more than 2^28"),
                      ((0, 8, grid(n=(65536, 65536, 65536)), 4, dp(cen), dp(nrm), 3.0, 2.0, dp(out), None), "more than 2^28"),
                      ((0, 8, grid(origin=(0.0, nan, 0.0)), 4, dp(cen), dp(nrm), 3.0, 2.0, dp(out), None), "origin[1] is not finite"),
                      ((0, 8, good, 4, dp(cen), dp(nrm), 3.0, 0.0, dp(out), None), "trunc"),
                      ((0, 8, good, 4, dp(cen), dp(nrm), 3.0, -2.0, dp(out), None), "trunc"),
                      ((0, 8, good, 4, dp(cen), dp(nrm), 3.0, nan, dp(out), None), "trunc"),
                      ((0, 8, good, 4, dp(cen), dp(nrm), 2.0, 2.0, dp(out), None), "support"),
                      ((0, 8, good, 4, dp(cen), dp(nrm), 1.0, 2.0, dp(out), None), "support"),
                      ((0, 8, good, 4, dp(cen), dp(nrm), inf, 2.0, dp(out), None), "support"),
                      ((0, 8, good, 4, dp(cen), dp(inf_n), 3.0, 2.0, dp(out), None), "normals[3] component 0 is not finite"),
                      # what pais_cloud_knn refuses, under this entry's name
                      ((0, 0, good, 4, dp(cen), dp(nrm), 3.0, 2.0, dp(out), None), "k = 0"),
                      ((0, 33, good, 4, dp(cen), dp(nrm), 3.0, 2.0, dp(out), None), "k = 33"),
                      ((0, 8, good, -4, dp(cen), dp(nrm), 3.0, 2.0, dp(out), None), "negative count"),
                      ((0, 8, good, 0, dp(cen), dp(nrm), 3.0, 2.0, dp(out), None), "nt == 0"),
                      ((-1, 8, good, 4, dp(cen), dp(nrm), 3.0, 2.0, dp(out), None), "device < 0"),
                      ((0, 8, good, 4, dp(nan_c), dp(nrm), 3.0, 2.0, dp(out), None), "targets[2] coordinate 1 is not finite"),
                      ((0, 8, grid(origin=(1e308, 0.0, 0.0), h=1e308), 4, dp(cen), dp(nrm), 3.0, 2.0, dp(out), None), "queries[")]:
        rc = L.pais_cloud_field(*args)
        err = L.pais_mesh_last_error().decode()
        assert rc < 0 and err.startswith("pais_cloud_field:") and msg in err, (rc, err, msg)
    assert (out == 77.0).all()

    f = np.ones(27)
    bad = f.copy()
    bad[13] = -inf
    fp = dp(f)
    n = C.c_int64(-7)
    keys, xyz = np.full(30, 77, np.int64), np.full(90, 77.0)
    kp = keys.ctypes.data_as(C.POINTER(C.c_int64))
    for args, msg in [((0, None, fp, 0, 10, C.byref(n), kp, dp(xyz), None), "null pointer"),
                      ((0, good, None, 0, 10, C.byref(n), kp, dp(xyz), None), "null pointer"),
                      ((0, good, fp, 0, 10, None, kp, dp(xyz), None), "null pointer"),
                      ((0, grid(h=0.0), fp, 0, 10, C.byref(n), kp, dp(xyz), None), "grid h"),
                      ((0, grid(n=(3, 3, 0)), fp, 0, 10, C.byref(n), kp, dp(xyz), None), "n[2] = 0 is below 2"),
                      ((0, good, fp, -1, 10, C.byref(n), kp, dp(xyz), None), "layers = -1"),
                      ((0, good, fp, 0, -1, C.byref(n), kp, dp(xyz), None), "max_triangles is negative"),
                      ((0, good, fp, 0, 10, C.byref(n), None, dp(xyz), None), "null keys or xyz"),
                      ((0, good, fp, 0, 10, C.byref(n), kp, None, None), "null keys or xyz"),
                      ((-1, good, fp, 0, 10, C.byref(n), kp, dp(xyz), None), "device < 0"),
                      ((-1, good, fp, 0, 0, C.byref(n), None, None, None), "device < 0"),
                      ((0, good, dp(bad), 0, 10, C.byref(n), kp, dp(xyz), None), "field[13] is infinite")]:
        rc = L.pais_field_surface(*args)
        err = L.pais_mesh_last_error().decode()
        assert rc < 0 and err.startswith("pais_field_surface:") and msg in err, (rc, err, msg)
    assert n.value == -7 and (keys == 77).all() and (xyz == 77.0).all()
    assert (L.pais_mesh_launches(), L.pais_cloud_launches()) == before

    # the Python layer: loud without a GPU, and its own argument errors
    g = msh.Grid([0.0, 0.0, 0.0], 1.0, (3, 3, 3))
    cloud = np.concatenate([cen, nrm], axis=1)
    with pytest.raises(RuntimeError, match="pais_cloud_field.*device < 0"):
        msh.field(cloud, g, device=-1)
    with pytest.raises(RuntimeError, match="pais_field_surface.*device < 0"):
        msh.surface(f, g, device=-1)
    with pytest.raises(RuntimeError, match="device < 0"):
        msh.mesh(cloud, h=0.5, device=-1)
    with pytest.raises(RuntimeError, match="pais_cloud_knn"):
        msh.mesh(np.concatenate([cen + np.arange(4)[:, None], nrm], axis=1), device=-1)      # h from evaluate.spacing: the search refuses
    for call in (lambda: msh.field(cen, g, device=-1), lambda: msh.surface(f[:5], g, device=-1), lambda: msh.grid_for(cen, 0.0, 1.0),
                 lambda: msh.grid_for(cen, 1.0, -1.0), lambda: msh.grid_for(np.zeros((0, 3)), 1.0, 1.0), lambda: msh.mesh(cen, device=-1),
                 lambda: msh.grid_for(np.array([[0.0, 0.0, 0.0], [1e4, 1e4, 1e4]]), 1.0, 0.0), lambda: msh.Grid([0.0, 0.0], 1.0, (2, 2, 2))):
        with pytest.raises(ValueError):
            call()
    assert (L.pais_mesh_launches(), L.pais_cloud_launches()) == before


def test_grid_for_covers_the_points():
    pts = np.random.default_rng(5).normal(size=(50, 3))
    g = msh.grid_for(pts, 0.25, 0.6)
    lo = np.array(g.origin)
    hi = lo + (np.array(g.n) - 1) * g.h
    assert g.h == 0.25 and (lo <= pts.min(axis=0) - 0.6).all() and (hi >= pts.max(axis=0) + 0.6).all() and (hi < pts.max(axis=0) + 0.6 + 0.25).all()
    assert msh.grid_for(pts[:1], 1.0, 0.0).n == [2, 2, 2]
    assert g.num_vertices() == g.n[0] * g.n[1] * g.n[2] and g.num_cells() == (g.n[0] - 1) * (g.n[1] - 1) * (g.n[2] - 1)


def test_mvs_mesh_without_a_gpu_fails_loudly(pawn_small):
    from pais_mvs_amd.config import readme_config
    from pais_mvs_amd.mvs import MVS
    m = MVS(readme_config(), pawn_small.cameras, device=-1, seed=42)
    m.load_patch(pawn_small.seeds[0][0], [1.0, 0.5], pawn_small.seeds[0][1], 0.5, 0.95)
    with pytest.raises(RuntimeError, match="device < 0"):
        m.mesh(h=0.1)
    m.close()


def test_command_line_argument_errors(tmp_path, capsys):
    from pais_mvs_amd import reconstruct
    cloud = str(tmp_path / "cloud.npy")
    np.save(cloud, np.zeros((4, 6)))
    out = str(tmp_path / "m.ply")
    for bad in ([cloud], [cloud, "--out", str(tmp_path / "m.stl")], [cloud, "--out", out, "--h", "0"], [cloud, "--out", out, "--h", "x"],
                [cloud, "--out", out, "--k", "0"], [cloud, "--out", out, "--k", "33"], [cloud, "--out", out, "--trunc", "-1"],
                [cloud, "--out", out, "--support", "1", "--trunc", "2"], ["--out", out]):
        with pytest.raises(SystemExit):
            msh.main(bad)
    assert reconstruct.parse_mesh_pitch("0.5") == 0.5
    for bad in (["scene.nvm", "--mesh", "0"], ["scene.nvm", "--mesh", "-1"], ["scene.nvm", "--mesh", "x"], ["cloud.mvs", "--filter", "--mesh"],
                ["cloud.mvs", "--filter", "--mesh", "0.5"]):
        with pytest.raises(SystemExit):
            reconstruct.main(bad)
    capsys.readouterr()


def test_mesh_methods_and_writers(tmp_path, cases):
    grid, f, count, keys, xyz = cases["sphere 9x9x9"]
    m = _welded(keys, xyz, grid)
    for name in ("m.ply", "m.obj"):
        path = str(tmp_path / name)
        m.write_ply(path) if name.endswith("ply") else m.write_obj(path)
        assert msh.read_counts(path) == (len(m.vertices), len(m.triangles))
    col = np.arange(3 * len(m.vertices), dtype=np.int64).reshape(-1, 3) % 251
    path = str(tmp_path / "c.ply")
    m.write_ply(path, col.astype(np.uint8))
    assert msh.read_counts(path) == (len(m.vertices), len(m.triangles))
    text = open(path).read()
    assert "property list uchar int vertex_indices" in text and "property uchar red" in text
    first = text.split("end_header\n")[1].split("\n")[0].split()
    assert [float(x) for x in first[:3]] == m.vertices[0].tolist() and [int(x) for x in first[3:]] == col[0, ::-1].tolist()
    with pytest.raises(ValueError):
        m.write_ply(path, col[:5])
    # a tetrahedron by hand: closed, characteristic 2, volume 1/6, area from the formula; one face removed: three boundary edges
    v = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    t = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)
    tet = msh.Mesh(v, t)
    assert tet.is_closed() and tet.euler() == 2 and tet.volume() == pytest.approx(1.0 / 6.0) and tet.area() == pytest.approx(1.5 + math.sqrt(3.0) / 2.0)
    open_tet = msh.Mesh(v, t[:3])
    assert not open_tet.is_closed() and sorted(map(tuple, open_tet.boundary_edges().tolist())) == [(1, 3), (2, 1), (3, 2)] and open_tet.euler() == 1
    assert not msh.Mesh(v, np.zeros((0, 3), np.int32)).is_closed()


def test_sampled_sphere(sampled):
    grid, want, got = sampled
    assert knn_ref.same_doubles(got, want)
    count, keys, xyz = mr.shim_surface(grid, got)
    m = _welded(keys, xyz)
    err = abs(m.volume() - SPHERE) / SPHERE
    print("\nsampled sphere: %d triangles, volume %.6f, relative error %.5f, NaN vertices %d" % (count, m.volume(), err, int(np.isnan(got).sum())))
    assert count == 5080 and m.is_closed() and m.euler() == 2 and np.isnan(got).any()
    assert err <= VOLUME_FACTOR * VOLUME_SEEN["sampled"]
    # at trunc = h cells that straddle the surface lose a corner to NaN: holes
    grid, c, n, k, support, trunc = mr.sampled_sphere(trunc_h=1.0)
    idx, d2 = mr.field_table(grid, c, k)
    thin = mr.shim_field(grid, idx, d2, c, n, support, trunc)
    count1, keys1, xyz1 = mr.shim_surface(grid, thin)
    assert 0 < count1 < count and not _welded(keys1, xyz1).is_closed()


def test_the_shim_runs_clean_under_the_sanitizers():
    """The shim with its own main, built with -fsanitize=address,undefined, as a stand-alone program over the odd sizes."""
    prog = mr.sanitized_program()                                # a build failure fails the test
    r = subprocess.run([prog], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.returncode, r.stdout[-500:], r.stderr[-2000:])
