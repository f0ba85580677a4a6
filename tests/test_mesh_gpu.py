"""The mesher on the MI355X against the restatement of its definition (tests/mesh_ref.py): pais_cloud_field bit for bit whatever
the split of the search, pais_field_surface byte for byte whatever the number of layers per pass, the scans across block
boundaries, the capacity protocol with a canary behind the buffers, and the whole path: a sampled sphere through mesh.mesh() and
the cloud of the small pawn scene through MVS.mesh() and the writers."""
import ctypes as C

import numpy as np
import pytest

from pais_mvs_amd import mesh as msh
from tests import knn_ref
from tests import mesh_ref as mr
from tests.test_knn_gpu import _loaded, grown  # noqa: F401  (the fixture: a grown cloud of the small pawn scene)

pytestmark = pytest.mark.gpu

SPLIT_ENV = ("PAIS_CLOUD_SLICES", "PAIS_CLOUD_CHUNK")


@pytest.fixture(autouse=True)
def _default_split(monkeypatch):
    for k in SPLIT_ENV:
        monkeypatch.delenv(k, raising=False)


def _launches():
    from pais_mvs_amd import _lib
    L = _lib.load()
    return L.pais_mesh_launches(), L.pais_cloud_launches()


def _gpu_field(grid, c, nrm, k, support, trunc):
    return msh.field(np.concatenate([c, nrm], axis=1), grid, k, support, trunc).reshape(-1)


@pytest.fixture(scope="module")
def surfaces():
    """name -> (grid, field, keys, xyz by the restatement): computed once"""
    return {name: (g, f) + mr.ref_surface(g, f) for name, (g, f) in mr.surface_cases().items()}


@pytest.fixture(scope="module")
def big_field():
    """a 17 x 13 x 11 grid (2431 vertices: no multiple of a block) against 3001 points: (grid, c, n, support, trunc, restatement)"""
    grid = mr.analytic_grid((17, 13, 11))
    rng = np.random.default_rng(3001)
    c = rng.normal(size=(3001, 3))
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    support, trunc = 3.0 * grid.h, 2.0 * grid.h
    idx, d2 = mr.field_table(grid, c, 8)
    return grid, c, c.copy(), support, trunc, mr.ref_field(grid, idx, d2, c, c, support, trunc)


@pytest.mark.parametrize("n", mr.FIELD_GRIDS)
def test_field_equals_the_restatement_on_the_cpu_cases(n):
    for nt in mr.FIELD_CLOUDS:
        for k in mr.FIELD_KS:
            grid, c, nrm, support, trunc = mr.field_case(n, nt, k)
            idx, d2 = mr.field_table(grid, c, k)
            before = _launches()
            got = _gpu_field(grid, c, nrm, k, support, trunc)
            after = _launches()
            assert knn_ref.same_doubles(got, mr.ref_field(grid, idx, d2, c, nrm, support, trunc)), (n, nt, k)
            assert after[0] - before[0] == 1 and after[1] - before[1] == 2          # one pass: search, merge, field


def test_field_on_a_grid_that_is_no_multiple_of_a_block(big_field):
    grid, c, nrm, support, trunc, want = big_field
    got = _gpu_field(grid, c, nrm, 8, support, trunc)
    assert knn_ref.same_doubles(got, want) and np.isnan(got).any() and np.isfinite(got).any()
    few = c[:300]
    idx, d2 = mr.field_table(grid, few, 8)
    assert knn_ref.same_doubles(_gpu_field(grid, few, few, 8, support, trunc), mr.ref_field(grid, idx, d2, few, few, support, trunc))


@pytest.mark.parametrize("slices", (1, 3, 64))
@pytest.mark.parametrize("chunk", (256, 512))
def test_field_does_not_depend_on_the_split(big_field, monkeypatch, slices, chunk):
    grid, c, nrm, support, trunc, want = big_field
    monkeypatch.setenv("PAIS_CLOUD_SLICES", str(slices))
    monkeypatch.setenv("PAIS_CLOUD_CHUNK", str(chunk))
    before = _launches()
    got = _gpu_field(grid, c, nrm, 8, support, trunc)
    after = _launches()
    assert knn_ref.same_doubles(got, want), (slices, chunk)
    passes = -(-grid.num_vertices() // chunk)
    assert after[0] - before[0] == passes and after[1] - before[1] == 2 * passes


def test_surface_equals_the_restatement_byte_for_byte(surfaces):
    for name, (grid, f, rk, rx) in surfaces.items():
        assert msh.surface_count(f, grid) == len(rk), name
        keys, xyz = msh.surface(f, grid)
        assert keys.dtype == np.int64 and keys.shape == rk.shape and xyz.shape == rx.shape, name
        assert np.array_equal(keys, rk) and knn_ref.same_doubles(xyz, rx), name


def test_surface_does_not_depend_on_layers(surfaces):
    grid, f, rk, rx = surfaces["sphere 17x13x11"]
    cells_z = grid.n[2] - 1
    for layers in (0, 1, 2, 3, cells_z):
        passes = 1 if layers == 0 else -(-cells_z // layers)
        before = _launches()
        assert msh.surface_count(f, grid, layers) == len(rk)
        counted = _launches()
        keys, xyz = msh.surface(f, grid, layers, max_triangles=len(rk))[1:]
        after = _launches()
        assert np.array_equal(keys, rk) and knn_ref.same_doubles(xyz, rx), layers
        assert counted[0] - before[0] == 2 * passes and after[0] - counted[0] == 3 * passes, layers
        assert after[1] == before[1]
    # more layers than the grid has: one pass
    assert np.array_equal(msh.surface(f, grid, 1000)[0], rk)


def _wavy(grid):
    p = grid.positions()
    return np.sin(3.1 * p[:, 0]) * np.cos(2.3 * p[:, 1]) + 0.7 * np.sin(1.9 * p[:, 2] + 0.4) + 0.05


@pytest.mark.parametrize("n", [(41, 38, 4), (48, 47, 33)])
def test_scans_across_block_boundaries(n):
    """4440 cells: more than one block of 256 and no multiple of it; 69184 cells: 271 blocks, so the scan of the block totals
    carries over its own 256.  The reference is the host shim, which test_mesh_cpu.py holds to the restatement."""
    grid = mr.Grid([-1.0, -0.9, -0.2], 0.05, n)
    f = _wavy(grid)
    count, sk, sx = mr.shim_surface(grid, f)
    cells = (n[0] - 1) * (n[1] - 1) * (n[2] - 1)
    assert cells > 256 and cells % 256 and count > cells // 4
    keys, xyz = msh.surface(f, grid)
    assert np.array_equal(keys, sk) and knn_ref.same_doubles(xyz, sx)
    keys, xyz = msh.surface(f, grid, 1)
    assert np.array_equal(keys, sk) and knn_ref.same_doubles(xyz, sx)


def test_a_grid_with_exactly_one_cell():
    grid = mr.Grid([0.25, -0.5, 1.0], 0.5, (2, 2, 2))
    for f in ([-1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0], [-1.0, -2.0, 0.5, 1.0, -0.25, 3.0, 1.0, 0.0], [1.0] * 8, [float("nan")] + [-1.0] * 7):
        f = np.array(f)
        rk, rx = mr.ref_surface(grid, f)
        keys, xyz = msh.surface(f, grid)
        assert np.array_equal(keys, rk) and knn_ref.same_doubles(xyz, rx), f
    assert len(mr.ref_surface(grid, np.array([-1.0] + [1.0] * 7))[0]) == 6       # the corner every tetrahedron shares


def test_capacity_protocol_on_the_device(surfaces):
    from pais_mvs_amd import _lib
    L = _lib.load()
    grid, f, rk, rx = surfaces["sphere 9x9x9"]
    count = len(rk)
    g = msh.Grid(grid.origin, grid.h, grid.n).c()
    gp = C.byref(g)
    fp = np.ascontiguousarray(f).ctypes.data_as(C.POINTER(C.c_double))
    n = C.c_int64(-1)
    before = _launches()
    assert L.pais_field_surface(0, gp, fp, 0, 0, C.byref(n), None, None, None) == 0 and n.value == count
    assert _launches()[0] - before[0] == 2                                       # count and scan: no emit kernel
    for cap in (count - 1, 1, count + 7):
        keys, xyz = np.full((count + 8, 3), -7, np.int64), np.full((count + 8, 3, 3), -7.0)
        n = C.c_int64(-1)
        assert L.pais_field_surface(0, gp, fp, 3, cap, C.byref(n), keys.ctypes.data_as(C.POINTER(C.c_int64)),
                                    xyz.ctypes.data_as(C.POINTER(C.c_double)), None) == 0
        m = min(cap, count)
        assert n.value == count and np.array_equal(keys[:m], rk[:m]) and knn_ref.same_doubles(xyz[:m], rx[:m]), cap
        assert (keys[m:] == -7).all() and (xyz[m:] == -7.0).all(), cap            # the canary: nothing beyond the prefix
    assert msh.surface(f, grid, max_triangles=count - 1)[0] == count


def test_sampled_sphere_through_mesh():
    c, nrm = mr.fibonacci_sphere(800)
    cloud = np.concatenate([c, nrm], axis=1)
    h = 0.15
    m = msh.mesh(cloud, h=h, k=8)
    grid = mr.Grid(m.grid.origin, m.grid.h, m.grid.n)
    assert m.grid.h == h and m.field.shape == tuple(m.grid.n[::-1])
    idx, d2 = mr.field_table(grid, c, 8)
    want = mr.ref_field(grid, idx, d2, c, nrm, 3.0 * h, 2.0 * h)
    assert knn_ref.same_doubles(m.field, want)
    rk, rx = mr.ref_surface(grid, want)
    rv, rt = mr.ref_weld(rk, rx)
    assert knn_ref.same_doubles(m.vertices, rv) and np.array_equal(m.triangles, rt) and np.array_equal(m.keys, np.unique(rk))
    assert m.is_closed() and m.euler() == 2 and m.volume() > 0 and len(m.boundary_edges()) == 0
    print("\nsampled sphere through mesh(): grid %s, %d triangles, volume %.6f" % (m.grid.n, len(m.triangles), m.volume()))
    # the spacing default: h = 2 spacing, and the mesh of a sphere is still closed
    from pais_mvs_amd import evaluate
    auto = msh.mesh(cloud)
    assert auto.grid.h == 2.0 * evaluate.spacing(c) and auto.is_closed() and auto.euler() == 2


def test_mvs_mesh_of_the_pawn_cloud(tmp_path, pawn_small, grown):
    from pais_mvs_amd import evaluate
    cfg, cl = grown
    m = _loaded(cfg, pawn_small.cameras, cl)
    mesh = m.mesh()
    h = mesh.grid.h
    centers = m.cloud()[:, :3]
    assert h == 2.0 * m.spacing() and len(mesh.triangles) > 0 and np.isfinite(mesh.vertices).all()
    d2 = evaluate.nearest(mesh.vertices, centers)[1]
    assert float(np.sqrt(d2.max())) <= 2.0 * h + h                               # trunc + h
    col = mesh.colors(m.colors_bgr(), centers)
    assert col.shape == (len(mesh.vertices), 3) and col.dtype == np.uint8
    for name in ("mesh.ply", "mesh.obj"):
        path = str(tmp_path / name)
        mesh.write_ply(path, col) if name.endswith("ply") else mesh.write_obj(path)
        assert msh.read_counts(path) == (len(mesh.vertices), len(mesh.triangles))
    print("\npawn cloud of %d: grid %s, %d vertices, %d triangles" % (len(cl), mesh.grid.n, len(mesh.vertices), len(mesh.triangles)))
    # reconstruct's --mesh step writes the same mesh
    from pais_mvs_amd import reconstruct
    got = reconstruct.write_mesh(m, str(tmp_path / "r.ply"))
    assert np.array_equal(got.triangles, mesh.triangles) and msh.read_counts(str(tmp_path / "r.ply")) == (len(mesh.vertices), len(mesh.triangles))
    m.close()


def test_command_line_writes_the_mesh(tmp_path, capsys):
    import json
    c, nrm = mr.fibonacci_sphere(800)
    cloud = str(tmp_path / "cloud.npy")
    np.save(cloud, np.concatenate([c, nrm], axis=1))
    want = msh.mesh(np.load(cloud), h=0.15)
    for name in ("m.ply", "m.obj"):
        out = str(tmp_path / name)
        capsys.readouterr()
        assert msh.main([cloud, "--h", "0.15", "--k", "8", "--out", out]) == 0
        line = json.loads(capsys.readouterr().out.strip().split("\n")[-1])
        assert line["triangles"] == len(want.triangles) and line["vertices"] == len(want.vertices) and line["closed"] is True
        assert msh.read_counts(out) == (len(want.vertices), len(want.triangles))


def test_no_gpu_is_refused_beside_a_device():
    grid = msh.Grid([0.0, 0.0, 0.0], 1.0, (3, 3, 3))
    cloud = np.concatenate([np.ones((4, 3)), np.tile([0.0, 0.0, 1.0], (4, 1))], axis=1)
    before = _launches()
    with pytest.raises(RuntimeError, match="pais_cloud_field.*device < 0"):
        msh.field(cloud, grid, device=-1)
    with pytest.raises(RuntimeError, match="pais_field_surface.*device < 0"):
        msh.surface(np.ones(27), grid, device=-1)
    assert _launches() == before
