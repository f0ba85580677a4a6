"""pais_cloud_planes without a GPU: the statements of include/pais_cloud.h as the kernel compiles them (pais_plane.hpp through
tests/plane_host_shim.cpp) against their restatement with Python floats (tests/plane_ref.py) bit for bit, the exact anchors, the
degenerate rows, the sign rules, the eigen-solve against LAPACK, the host rule pais_cloud_normal_rule, the refusals that happen
before anything is launched, the argument errors of the two command lines, and the shim as a stand-alone program under the
address and undefined-behaviour sanitizers."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

from tests import knn_ref
from tests import plane_ref as pr

# What numpy.linalg.eigh showed against the shim on this code, and the factor that covers other seeds.
# eigenvalues: in units of DBL_EPSILON lambda_2; angles: degrees, over the rows with lambda_1 > 20 lambda_0.  The random
# neighbourhoods have axis scales up to 1e6 apart, so lambda_2 / (lambda_1 - lambda_0), which is what an eigenvector's rounding
# error scales with, reaches 1e11 there and stays below 1e4 on the plane cases.
LAPACK_SEEN = {"plane_case": (5.97, 7.6e-14), "random": (5.53, 1.45e-3)}
LAPACK_FACTOR = 8.0


def _both(q, t, index, with_query, toward=None, what=""):
    got, sweeps = pr.shim_planes(q, t, index, with_query, toward)
    want, ref_sweeps = pr.ref_planes(q, t, index, with_query, toward)
    pr.assert_same_records(got, want, what)
    assert np.array_equal(sweeps, ref_sweeps), what
    return got, sweeps


@pytest.mark.parametrize("nq,nt,k,skip", pr.CASES)
def test_shim_equals_the_restatement_bit_for_bit(nq, nt, k, skip):
    q, t = pr.case_points(nq, nt, k, skip)
    index = knn_ref.brute_knn(q, t, k, skip)[0]
    for with_query in (False, True):
        got, sweeps = _both(q, t, index, with_query, what=(nq, nt, k, skip, with_query))
        m = (index >= 0).sum(axis=1) + (1 if with_query else 0)
        assert np.array_equal(got["count"], m) and np.array_equal(got["status"], np.where(m < 3, pr.FEW, pr.OK))
        few = got["status"] == pr.FEW
        for f in pr.FIELDS:
            assert not np.asarray(got[f])[few].any(), f           # every double of a FEW record is 0
        assert sweeps.max() < pr.SWEEPS
    if (nq, nt) == (5, 2):
        assert m.tolist() == [3] * 5                              # m = 2 without the query, 3 with it
    if (nq, nt) == (257, 513):
        toward = np.random.default_rng(9).normal(size=(nq, 3))
        got, _ = _both(q, t, index, True, toward, "orient")
        assert (np.einsum("ij,ij->i", got["normal"], toward) >= 0).all()


@pytest.mark.parametrize("axis", (0, 1, 2))
def test_exact_anchors(axis):
    """nine points with one coordinate equal: the plane is exact, and the sort and the column pick are exercised on every axis"""
    p = pr.anchor_points(axis)
    got, sweeps = _both(p, p, pr.self_table(p)[0], True, what=("anchor", axis))
    unit = np.eye(3)[axis]
    assert (got["status"] == pr.OK).all() and (got["count"] == 9).all()
    assert (got["eigen"][:, 0] == 0.0).all() and (got["eigen"][:, 1] > 0).all()
    assert (got["normal"] == unit).all() and (got["centroid"][:, axis] == 0.5).all() and (got["offset"] == 0.0).all()
    assert (got["variation"] == 0.0).all() and (sweeps == 1).all()


def test_degenerate_rows():
    for name, p in pr.degenerate_rows().items():
        got, sweeps = _both(p, p, pr.self_table(p)[0], True, what=name)
        assert (got["status"] == pr.OK).all() and np.isfinite(got["eigen"]).all() and sweeps.max() < pr.SWEEPS, name
        if name == "collinear":
            assert (got["eigen"][:, 2] > 90.0).all() and (np.abs(got["eigen"][:, :2]) < 1e-12).all()
        if name == "all equal":
            assert (np.abs(got["eigen"]) < 1e-28).all()          # not exact zeros: the centroid is rounded
    # fewer than three points whichever way: every double 0
    p = np.random.default_rng(3).normal(size=(2, 3))
    got, _ = _both(p, p, pr.self_table(p, 4)[0], True, what="two points")
    assert (got["status"] == pr.FEW).all() and (got["count"] == 2).all() and not got["centroid"].any()


def test_sign_rules():
    # a normal along (1, -1, 0) / sqrt 2: the two largest components tie in fabs, the lowest axis decides
    rng = np.random.default_rng(12)
    u, w = np.array([1.0, 1.0, 0.0]), np.array([0.0, 0.0, 1.0])
    p = rng.normal(size=(9, 1)) * u + rng.normal(size=(9, 1)) * w
    got, _ = _both(p, p, pr.self_table(p)[0], True, what="tie")
    n = got["normal"]
    assert (np.abs(n[:, 0]) == np.abs(n[:, 1])).all() and (n[:, 0] > 0).all() and (n[:, 1] < 0).all()
    # ORIENT negates all three components and nothing else: a 0 component becomes -0.0
    p = pr.anchor_points(2)
    index = pr.self_table(p)[0]
    plain, _ = _both(p, p, index, True, what="plain")
    down, _ = _both(p, p, index, True, np.tile([0.0, 0.0, -1.0], (9, 1)), "down")
    up, _ = _both(p, p, index, True, np.tile([0.0, 0.0, 2.0], (9, 1)), "up")
    assert knn_ref.same_doubles(down["normal"], -plain["normal"]) and np.signbit(down["normal"]).all()
    assert knn_ref.same_doubles(up["normal"], plain["normal"]) and not np.signbit(up["normal"]).any()
    for f in ("centroid", "eigen", "variation"):
        assert knn_ref.same_doubles(down[f], plain[f]), f
    assert np.array_equal(down["offset"], -plain["offset"])     # as values: the offsets are zeros whose sign the sums decide
    # a vector in the plane (dot product 0) does not negate
    flat, _ = _both(p, p, index, True, np.tile([1.0, 0.0, 0.0], (9, 1)), "in the plane")
    assert knn_ref.same_doubles(flat["normal"], plain["normal"])


def test_eigen_solve_against_lapack():
    seen = {"plane_case": [0.0, 0.0], "random": [0.0, 0.0]}
    most = 0
    for name, q, t, index, with_query in pr.lapack_inputs():
        got, sweeps = pr.shim_planes(q, t, index, with_query)
        e, a, rows = pr.lapack_errors(got, q, t, index, with_query)
        assert (got["status"] == pr.OK).all() and rows > len(q) // 2, name
        group = seen[name.split()[0]]
        group[0], group[1], most = max(group[0], e), max(group[1], a), max(most, int(sweeps.max()))
    print("\neigenvalue error / (eps lambda_2), normal angle [deg]: %s; rotating sweeps <= %d" % (seen, most))
    for g, (e, a) in LAPACK_SEEN.items():
        assert seen[g][0] <= LAPACK_FACTOR * e and seen[g][1] <= LAPACK_FACTOR * a, (g, seen[g])
    assert most < 60


def test_normal_rule_equals_the_loop():
    from pais_mvs_amd import _lib, evaluate
    L = _lib.load()
    assert L.pais_sizeof_plane() == C.sizeof(_lib.Plane) == C.sizeof(pr.CPlane) == 96
    assert (_lib.PLANE_WITH_QUERY, _lib.PLANE_ORIENT, _lib.PLANE_OK, _lib.PLANE_FEW, _lib.PLANE_NOCONV, _lib.PLANE_SWEEPS) == (2, 4, 0, 1, 2, 60)
    rng = np.random.default_rng(21)
    n = 400
    fitted = rng.normal(size=(n, 3))
    fitted /= np.linalg.norm(fitted, axis=1, keepdims=True)
    given = fitted + rng.normal(size=(n, 3)) * 0.5
    given /= np.linalg.norm(given, axis=1, keepdims=True)
    given[::7] *= -1.0                                           # the sign of a normal does not matter
    given[5], given[6] = fitted[5], np.cross(fitted[6], [0.3, 0.2, 0.9])          # |cos| = 1 (to rounding) and about 0
    status = np.where(np.arange(n) % 11 == 3, pr.FEW, np.where(np.arange(n) % 13 == 5, pr.NOCONV, pr.OK)).astype(np.int32)
    rec = {"normal": fitted, "status": status}
    for min_cos in (0.0, 0.5, math.cos(math.radians(30.0)), 1.0):
        got = evaluate.normal_rule(rec, given, min_cos)
        assert got.dtype == bool and got.tolist() == pr.normal_rule_loop(status, fitted, given, min_cos), min_cos
        assert not got[status != pr.OK].any()
        if min_cos == 0.0:
            assert not got.any()
        if min_cos == 1.0:
            assert got[status == pr.OK].sum() >= (status == pr.OK).sum() - 3      # all but the rows that round to 1
    assert 0 < evaluate.normal_rule(rec, given, 0.5).sum() < n
    # refusals
    out = np.zeros(n, np.uint8)
    recs = (_lib.Plane * n)()
    gp, op = given.ctypes.data_as(C.POINTER(C.c_double)), out.ctypes.data_as(C.POINTER(C.c_uint8))
    for args in ((-1, recs, gp, 0.5, op), (n, None, gp, 0.5, op), (n, recs, None, 0.5, op), (n, recs, gp, 0.5, None)):
        assert L.pais_cloud_normal_rule(*args) < 0 and b"pais_cloud_normal_rule" in L.pais_cloud_last_error()
    assert L.pais_cloud_normal_rule(0, None, None, 0.5, None) == 0
    with pytest.raises(ValueError):
        evaluate.normal_rule(rec, given[:5], 0.5)


def test_planes_refusals_launch_nothing_and_touch_nothing():
    """every refusal of pais_cloud_planes; none of them needs a GPU (test_planes_gpu.py repeats them beside a device)"""
    from pais_mvs_amd import _lib, evaluate
    before = _lib.load().pais_cloud_launches()
    pr.check_refusals()
    q = np.zeros((4, 3))
    for call in (lambda: evaluate.planes(q, 33, device=-1), lambda: evaluate.planes(q, 2, device=-1), lambda: evaluate.roughness(q, 2, device=-1),
                 lambda: evaluate.estimate_normals(q, 2, device=-1), lambda: evaluate.planes(q, 2, targets=q[:3], skip_self=True, device=-1)):
        with pytest.raises(RuntimeError, match="pais_cloud_planes"):
            call()
    for call in (lambda: evaluate.planes(np.zeros((4, 2)), 2, device=-1), lambda: evaluate.planes(q, 2, toward=np.zeros((3, 3)), device=-1)):
        with pytest.raises(ValueError):
            call()
    assert _lib.load().pais_cloud_launches() == before


def test_normal_filtering_without_a_gpu_context_fails_loudly(pawn_small):
    from pais_mvs_amd.config import readme_config
    from pais_mvs_amd.mvs import MVS
    m = MVS(readme_config(), pawn_small.cameras, device=-1, seed=42)
    with pytest.raises(RuntimeError, match="no GPU context"):
        m.normalFiltering(8, 30.0)
    m.close()


def test_command_lines_know_the_new_flags(tmp_path, capsys):
    from pais_mvs_amd import evaluate, reconstruct
    assert reconstruct.parse_normal_agreement("16,30") == (16, 30.0) and reconstruct.parse_normal_agreement("8,22.5") == (8, 22.5)
    assert evaluate.parse_viewpoint("1,2.5,-3") == [1.0, 2.5, -3.0]
    for bad in (["cloud.mvs", "--filter", "--normal-agreement", "8"], ["cloud.mvs", "--filter", "--normal-agreement", "a,b"],
                ["scene.nvm", "--normal-agreement", "8,30"], ["scene.nvm", "--statistical", "8,2", "--normal-agreement", "8,30"]):
        with pytest.raises(SystemExit):
            reconstruct.main(bad)
    cloud = str(tmp_path / "cloud.npy")
    for bad in (["--roughness", "8"], ["--roughness", "x", cloud], ["--estimate-normals", "8", "--out", str(tmp_path / "o.npy")],
                [cloud, "--estimate-normals", "8"], [cloud, "--estimate-normals", "8", "--viewpoint", "1,2", "--out", str(tmp_path / "o.npy")],
                [cloud, "--viewpoint", "1,2,3", "--spacing"]):
        with pytest.raises(SystemExit):
            evaluate.main(bad)
    capsys.readouterr()
    # bare points are read: .npy (n,3), and a PLY without normals
    pts = np.random.default_rng(2).normal(size=(7, 3))
    np.save(cloud, pts)
    assert np.array_equal(evaluate.load_points(cloud), pts)
    ply = tmp_path / "bare.ply"
    ply.write_text("ply\nformat ascii 1.0\nelement vertex 7\nproperty float x\nproperty float y\nproperty float z\nend_header\n"
                   + "".join("%r %r %r\n" % tuple(r) for r in pts.tolist()))
    assert np.array_equal(evaluate.load_points(str(ply)), pts)
    with pytest.raises(IOError):
        evaluate.load_cloud(str(ply))                            # a scored cloud still needs its normals


def test_the_shim_runs_clean_under_the_sanitizers():
    """The shim with its own main, built with -fsanitize=address,undefined, as a stand-alone program over the odd sizes."""
    prog = pr.sanitized_program()                                # a build failure fails the test
    r = subprocess.run([prog], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.returncode, r.stdout[-500:], r.stderr[-2000:])
