"""pais_depth_test / pais_cloud_visibility without a GPU: the statements of include/pais_render.h as the kernel compiles them
(pais_vis.hpp through tests/vis_host_shim.cpp) against their numpy restatement (tests/vis_ref.py) bit for bit on random pairs
and on the edge list, the host rule pais_cloud_visibility_rule against plain loops with each of its refusals, every refusal of
the two device entries before anything is launched, the Python wrappers' argument checks and host arithmetic, the command
lines' new flags, and the shim as a stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from pais_mvs_amd import _lib
from pais_mvs_amd import render as rnd
from tests import vis_ref as vr
from tests.test_render_gpu import _ball_views

W, H = 16, 12


def _random_maps(rng, V, Wd, Hd, n):
    """maps as a render leaves them: +inf / -1 where empty, else a depth around the ball and an id below n"""
    depth = rng.uniform(2.0, 4.0, size=(V, Hd, Wd))
    idm = rng.integers(0, max(n, 1), size=(V, Hd, Wd)).astype(np.int32)
    hole = rng.uniform(size=depth.shape) < 0.3
    depth[hole], idm[hole] = np.inf, -1
    return depth, idm


@pytest.mark.parametrize("n,V,Wd,Hd", [(1, 1, 37, 29), (65, 3, 37, 29), (300, 3, 65, 48), (1000, 2, 5, 3)])
def test_shim_equals_the_restatement_bit_for_bit(n, V, Wd, Hd):
    rng = np.random.default_rng(100 * n + V)
    views = _ball_views(rng, V, Wd, Hd)
    pts = rng.normal(size=(n, 3)) * 1.2
    pts[::17] *= 4.0                                             # some behind the cameras and far outside
    depth, idm = _random_maps(rng, V, Wd, Hd, n)
    seen = set()
    for tol in (0.0, 0.3):
        for use_id, self_index in ((False, False), (True, False), (True, True)):
            got = vr.shim_depth_test(pts, views, depth, idm if use_id else None, tol, self_index)
            want = vr.ref_depth_test(pts, views, depth, idm if use_id else None, tol, self_index)
            vr.assert_same(got, want, (n, V, Wd, Hd, tol, use_id, self_index))
            seen |= set(np.unique(got[0]).tolist())
            tested = got[0] <= vr.IN_FRONT
            assert np.isnan(got[2][~tested]).all() and (got[1][~tested] == -1).all() and not np.isnan(got[2][tested]).any()
            if not use_id:
                assert (got[1] == -1).all()
    if n >= 65:
        assert len(seen) >= 5, seen


def test_edge_list_on_the_host():
    view, depth, idm, pts, tol, names, plain, with_self = vr.edge_case()
    for self_index, expect in ((False, plain), (True, with_self)):
        got = vr.shim_depth_test(pts, [view], depth, idm, tol, self_index)
        vr.assert_same(got, vr.ref_depth_test(pts, [view], depth, idm, tol, self_index), ("edge", self_index))
        for k, name in enumerate(names):
            assert got[0][0, k] == expect[k], (name, self_index, int(got[0][0, k]), float(got[2][0, k]))
    got = vr.shim_depth_test(pts, [view], depth, idm, tol, False)
    m = dict(zip(names, got[2][0]))
    assert m["m == tol"] == tol and m["m == -tol"] == -tol and m["m == 0"] == 0.0
    # tol = 0: only m == 0 is VISIBLE
    zero = vr.shim_depth_test(pts, [view], depth, idm, 0.0, False)
    vr.assert_same(zero, vr.ref_depth_test(pts, [view], depth, idm, 0.0, False), "tol 0")
    z = dict(zip(names, zero[0][0]))
    assert z["m == 0"] == vr.VISIBLE and z["m == tol"] == vr.OCCLUDED and z["m == -tol"] == vr.IN_FRONT


def test_two_walls_on_the_restatement():
    """the hand-derived expectations of vis_ref.two_walls hold on the numpy restatements (renderer: _brute), without a GPU"""
    from tests.test_render_gpu import CULL, DISC, _brute
    view, Wd, Hd, cen, nrm, rad, qry, tol, code, occ, mar = vr.two_walls()
    depth, idm = _brute(DISC, CULL, cen, nrm, rad, [view], Wd, Hd)
    assert (depth[0][:, :32] == 2.0).all() and (depth[0][:, 32:] == 4.0).all()
    got = vr.ref_depth_test(qry, [view], depth, idm, tol)
    assert np.array_equal(got[0][0], code) and np.array_equal(got[1][0], occ) and np.array_equal(got[2][0], mar)


def test_rule_equals_the_loops_and_refuses():
    L = _lib.load()
    rng = np.random.default_rng(7)
    n, V = 300, 6
    code = rng.integers(0, 6, size=(V, n)).astype(np.uint8)
    lists = [sorted(rng.choice(V, size=int(rng.integers(0, V + 1)), replace=False).tolist()) for _ in range(n)]
    lists[5] = [2, 2, 2]                                         # a camera listed three times counts three times
    for min_visible in (0, 1, 3, 7):
        visible, outlier = rnd.visibility_rule(code, lists, min_visible)
        want_v, want_o = vr.rule_loop(code, lists, min_visible)
        assert visible.dtype == np.int32 and outlier.dtype == bool
        assert visible.tolist() == want_v and outlier.tolist() == want_o, min_visible
    assert 0 < rnd.visibility_rule(code, lists, 3)[1].sum() < n
    only = np.full((V, n), vr.IN_FRONT, np.uint8)
    only[1], only[2], only[3] = vr.EMPTY, vr.OUTSIDE, vr.BEHIND   # none of these subtracts
    assert rnd.visibility_rule(only, lists, 0)[0].tolist() == [len(c) for c in lists]
    # refusals
    off = np.zeros(n + 1, np.int32)
    off[1:] = np.cumsum([len(c) for c in lists])
    cams = np.array([c for lst in lists for c in lst], np.int32)
    vis, out = np.full(n, 77, np.int32), np.full(n, 77, np.uint8)
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    good = dict(n=n, V=V, code=p(code, C.c_uint8), off=p(off, C.c_int32), cams=p(cams, C.c_int32), vis=p(vis, C.c_int32), out=p(out, C.c_uint8))
    call = lambda **kw: (lambda a: L.pais_cloud_visibility_rule(a["n"], a["V"], a["code"], a["off"], a["cams"], 3, a["vis"], a["out"]))({**good, **kw})
    shifted, falling, low, high = off.copy(), off.copy(), cams.copy(), cams.copy()
    shifted[0], falling[40], low[3], high[-1] = 1, falling[39] - 1, -1, V
    for what, kw in {"negative n": dict(n=-1), "negative views": dict(V=-1), "null code": dict(code=None), "null offsets": dict(off=None),
                     "null cams": dict(cams=None), "null visible": dict(vis=None), "null outlier": dict(out=None),
                     "offsets[0]": dict(off=p(shifted, C.c_int32)), "offsets decrease": dict(off=p(falling, C.c_int32)),
                     "camera -1": dict(cams=p(low, C.c_int32)), "camera V": dict(cams=p(high, C.c_int32)), "fewer views": dict(V=V - 1)}.items():
        if what == "fewer views" and not (cams == V - 1).any():
            continue
        assert call(**kw) < 0 and L.pais_render_last_error().decode().startswith("pais_cloud_visibility_rule:"), what
    assert (vis == 77).all() and (out == 77).all()               # a refusal writes nothing
    assert L.pais_cloud_visibility_rule(0, V, None, None, None, 3, None, None) == 0
    assert call() == 0 and vis.tolist() == vr.rule_loop(code, lists, 3)[0]
    with pytest.raises(ValueError):
        rnd.visibility_rule(code, lists[:-1], 3)


def _views(num=1, **kw):
    v = rnd.make_view(np.eye(3), np.zeros(3), (20.0, 20.0), (8.0, 6.0))
    for k, (i, x) in kw.items():
        getattr(v, k)[i] = x
    return (_lib.View * max(num, 1))(*[v] * max(num, 1))


def _depth_test(L, device=0, flags=0, n=2, points="ok", num_views=1, views="ok", width=W, height=H, depth="ok", idm=None, tol=0.1, code="ok"):
    dp = lambda a: None if a is None else np.ascontiguousarray(a, np.float64).ctypes.data_as(C.POINTER(C.c_double))
    pts = np.tile([0.0, 0.0, 3.0], (max(n, 1), 1)) if isinstance(points, str) else points
    d = np.full((max(num_views, 1), max(height, 1), max(width, 1)), 3.0) if isinstance(depth, str) else depth
    i = None if idm is None else np.zeros((max(num_views, 1), max(height, 1), max(width, 1)), np.int32)
    out = np.full((max(num_views, 1), max(n, 1)), 77, np.uint8)
    rc = L.pais_depth_test(device, flags, n, dp(pts), num_views, _views(num_views) if isinstance(views, str) else views, width, height, dp(d),
                           None if i is None else i.ctypes.data_as(C.POINTER(C.c_int32)), tol,
                           out.ctypes.data_as(C.POINTER(C.c_uint8)) if code == "ok" else None, None, None, None)
    assert (out == 77).all()
    return rc, L.pais_render_last_error().decode()


def _visibility(L, device=0, mode=0, flags=1, n=2, centers="ok", normals="ok", radii=None, radius=0.1, nq=2, queries="ok", num_views=1,
                views="ok", width=W, height=H, tol=0.1, code="ok", maps="none"):
    dp = lambda a: None if a is None else np.ascontiguousarray(a, np.float64).ctypes.data_as(C.POINTER(C.c_double))
    cen = np.tile([0.0, 0.0, 3.0], (max(n, 1), 1)) if isinstance(centers, str) else centers
    nrm = np.tile([0.0, 0.0, -1.0], (max(n, 1), 1)) if isinstance(normals, str) else normals
    qry = np.tile([0.0, 0.0, 3.0], (max(nq, 1), 1)) if isinstance(queries, str) else queries
    out = np.full((max(num_views, 1), max(nq, 1)), 77, np.uint8)
    d = np.zeros((max(num_views, 1), max(height, 1), max(width, 1)))
    i = np.zeros(d.shape, np.int32)
    rc = L.pais_cloud_visibility(device, mode, flags, n, dp(cen), dp(nrm), dp(radii), radius, nq, dp(qry), num_views,
                                 _views(num_views) if isinstance(views, str) else views, width, height, tol,
                                 out.ctypes.data_as(C.POINTER(C.c_uint8)) if code == "ok" else None, None, None,
                                 dp(d) if maps in ("both", "depth") else None, i.ctypes.data_as(C.POINTER(C.c_int32)) if maps in ("both", "id") else None, None)
    assert (out == 77).all()
    return rc, L.pais_render_last_error().decode()


def test_every_refusal_comes_with_a_message_and_launches_nothing():
    L = _lib.load()
    before = L.pais_render_launches()
    nan, inf = float("nan"), float("inf")
    bad = lambda i, j, x: np.array([[0.0, 0.0, 3.0], [0.0, 0.0, 3.0]]) + np.where((np.arange(6).reshape(2, 3) == 3 * i + j), x, 0.0)
    bad_depth = np.full((1, H, W), 3.0)
    bad_depth[0, 3, 4] = nan
    shared = {
        "negative views": dict(num_views=-1), "null views": dict(views=None), "device": dict(device=-1),
        "width 0": dict(width=0), "height 0": dict(height=0), "width negative": dict(width=-5),
        "nan R": dict(views=_views(R=(4, nan))), "inf T": dict(views=_views(T=(2, inf))), "nan pp": dict(views=_views(pp=(1, nan))),
        "nan focal": dict(views=_views(focal=(0, nan))), "focal 0": dict(views=_views(focal=(1, 0.0))),
        "tol negative": dict(tol=-0.1), "tol nan": dict(tol=nan), "tol inf": dict(tol=inf), "null code": dict(code=None),
        "unknown flag": dict(flags=2), "unknown high flag": dict(flags=0x200),
    }
    own = {
        "negative n": dict(n=-1), "null points": dict(points=None), "nan point": dict(points=bad(1, 2, nan)), "inf point": dict(points=bad(0, 0, -inf)),
        "null depth": dict(depth=None), "nan depth": dict(depth=bad_depth), "self without id": dict(flags=_lib.VIS_SELF),
        "cull flag": dict(flags=_lib.RENDER_CULL_BACK),
    }
    for what, kw in {**shared, **own}.items():
        rc, msg = _depth_test(L, **kw)
        assert rc < 0 and msg.startswith("pais_depth_test:"), (what, rc, msg)
    rc, msg = _depth_test(L, device=-1)
    assert rc < 0 and "needs a GPU" in msg
    own = {
        "negative n": dict(n=-1), "negative nq": dict(nq=-1), "null centers": dict(centers=None), "null queries": dict(queries=None),
        "nan query": dict(queries=bad(1, 2, nan)), "nan centre": dict(centers=bad(0, 1, nan)), "nan normal": dict(normals=bad(1, 1, nan)),
        "disc without normals": dict(normals=None), "mode 2": dict(mode=2), "rho 0": dict(radius=0.0), "nan radius": dict(radius=nan),
        "radii 0": dict(radii=np.array([0.1, 0.0])), "point size 65": dict(mode=1, radius=65.0),
        "depth without id": dict(maps="depth"), "id without depth": dict(maps="id"),
        "self with other queries": dict(flags=_lib.RENDER_CULL_BACK | _lib.VIS_SELF, nq=3),
    }
    for what, kw in {**shared, **own}.items():
        rc, msg = _visibility(L, **kw)
        assert rc < 0 and msg.startswith("pais_cloud_visibility:"), (what, rc, msg)
    rc, msg = _visibility(L, device=-1, maps="both")
    assert rc < 0 and "needs a GPU" in msg
    # nothing to do is no error, and needs no device
    assert _depth_test(L, n=0, points=None, code=None)[0] == 0 and _depth_test(L, num_views=0, views=None, depth=None)[0] == 0
    assert _visibility(L, num_views=0, views=None)[0] == 0 and _visibility(L, nq=0, queries=None, code=None)[0] == 0
    assert L.pais_render_launches() == before


def test_constants_and_the_header_comment():
    hdr = open(__file__.replace("tests/test_visibility_cpu.py", "include/pais_render.h")).read()
    for name, val in (("PAIS_VIS_VISIBLE", _lib.VIS_VISIBLE), ("PAIS_VIS_OCCLUDED", _lib.VIS_OCCLUDED), ("PAIS_VIS_IN_FRONT", _lib.VIS_IN_FRONT),
                      ("PAIS_VIS_EMPTY", _lib.VIS_EMPTY), ("PAIS_VIS_OUTSIDE", _lib.VIS_OUTSIDE), ("PAIS_VIS_BEHIND", _lib.VIS_BEHIND),
                      ("PAIS_VIS_SELF", _lib.VIS_SELF)):
        assert int(hdr.split("#define %s " % name)[1].split()[0], 0) == val, name
    assert (_lib.VIS_VISIBLE, _lib.VIS_OCCLUDED, _lib.VIS_IN_FRONT, _lib.VIS_EMPTY, _lib.VIS_OUTSIDE, _lib.VIS_BEHIND) == (0, 1, 2, 3, 4, 5)
    assert _lib.VIS_SELF & _lib.RENDER_CULL_BACK == 0 and _lib.VIS_SELF == vr.SELF
    assert "m == tol and m == -tol are VISIBLE" in hdr


def test_python_wrappers():
    code = np.array([[0, 1, 2, 3, 0], [0, 1, 4, 5, 1], [0, 0, 0, 3, 2]], np.uint8)
    v = rnd.Visibility(code)
    assert v.counts().tolist() == [[3, 0, 0, 0, 0, 0], [1, 2, 0, 0, 0, 0], [1, 0, 1, 0, 1, 0], [0, 0, 0, 2, 0, 1], [1, 1, 1, 0, 0, 0]]
    assert v.counts().dtype == np.int64 and (v.counts().sum(axis=1) == 3).all()
    assert v.view_counts().tolist() == [[2, 1, 1, 1, 0, 0], [1, 2, 0, 0, 1, 1], [3, 0, 1, 1, 0, 0]]
    assert v.visible_views() == [[0, 1, 2], [2], [2], [], [0]]
    assert rnd.VIS_CODES == ("visible", "occluded", "in_front", "empty", "outside", "behind")
    for bad in (lambda: rnd.Visibility(code[0]), lambda: rnd.Visibility(np.array([[6]], np.uint8)), lambda: rnd.Visibility(code, occluder=np.zeros((3, 4)))):
        with pytest.raises(ValueError):
            bad()
    view = rnd.make_view(np.eye(3), np.zeros(3), (20.0, 20.0), (8.0, 6.0))
    pts, d = np.zeros((4, 3)), np.full((1, H, W), 3.0)
    for bad in (lambda: rnd.depth_test(np.zeros((4, 2)), [view], d, device=-1), lambda: rnd.depth_test(pts, [view, view], d, device=-1),
                lambda: rnd.depth_test(pts, [view], d[0], device=-1), lambda: rnd.depth_test(pts, [view], d, id=np.zeros((1, H, W + 1), np.int32), device=-1),
                lambda: rnd.depth_test(pts, [view], d, self_index=True, device=-1),
                lambda: rnd.visibility(pts, pts[:3], [view], W, H, radius=0.1, device=-1), lambda: rnd.visibility(pts, pts, [view], W, H, radii=np.ones(3), tol=0.1, device=-1),
                lambda: rnd.visibility(pts, pts, [view], W, H, queries=np.zeros((3, 2)), radius=0.1, device=-1),
                lambda: rnd.visibility(pts, pts, [view], W, H, queries=pts[:3], self_index=True, radius=0.1, device=-1),
                lambda: rnd.visibility(pts, pts, [view], W, H, radii=np.ones(4), device=-1),            # no default tol with per-splat radii
                lambda: rnd.visibility(pts, None, [view], W, H, mode="point", radius=1, device=-1),     # nor in point mode
                lambda: rnd.visibility(pts, pts, [view], W, H, mode="mesh", radius=0.1, device=-1)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(RuntimeError, match="pais_depth_test"):
        rnd.depth_test(pts, [view], d, device=-1)
    with pytest.raises(RuntimeError, match="pais_cloud_visibility: needs a GPU"):
        rnd.visibility(pts + [0.0, 0.0, 3.0], np.tile([0.0, 0.0, -1.0], (4, 1)), [view], W, H, radius=0.1, device=-1)
    from pais_mvs_amd import evaluate
    with pytest.raises(ValueError):
        evaluate.visible_cameras(np.zeros((4, 3)), [], radius=0.1, device=-1)
    assert evaluate.visible_cameras(np.zeros((4, 6)), [], radius=0.1, device=-1) == [[], [], [], []]


def test_depth_filtering_without_a_gpu_context_fails_loudly(pawn_small):
    from pais_mvs_amd.config import readme_config
    from pais_mvs_amd.mvs import MVS
    m = MVS(readme_config(), pawn_small.cameras, device=-1, seed=42)
    with pytest.raises(RuntimeError, match="no GPU context"):
        m.depthFiltering()
    m.close()


def test_command_lines_know_the_new_flags(capsys):
    from pais_mvs_amd import reconstruct, view
    assert reconstruct.parse_depth_consistency("0.01,0.02") == (0.01, 0.02) and reconstruct.parse_depth_consistency("auto,auto") == (None, None)
    assert reconstruct.parse_depth_consistency("AUTO,0") == (None, 0.0) and reconstruct.parse_depth_consistency("0.5,auto") == (0.5, None)
    for bad in (["cloud.mvs", "--filter", "--depth-consistency", "0.1"], ["cloud.mvs", "--filter", "--depth-consistency", "a,b"],
                ["cloud.mvs", "--filter", "--depth-consistency", "0,auto"], ["cloud.mvs", "--filter", "--depth-consistency", "auto,-1"],
                ["scene.nvm", "--depth-consistency", "auto,auto"]):
        with pytest.raises(SystemExit):
            reconstruct.main(bad)
    a = view.parse_args(["c.mvs", "--camera", "0", "2", "--visibility"])
    assert a.visibility and a.camera == [0, 2]
    assert not view.parse_args(["c.mvs", "--camera", "0"]).visibility
    for argv in (["c.mvs", "--orbit", "2", "--visibility"], ["c.mvs", "--camera", "0", "--mode", "point", "--visibility"]):
        with pytest.raises(SystemExit) as e:
            view.parse_args(argv)
        assert e.value.code == 2, argv
    capsys.readouterr()


def test_the_shim_runs_clean_under_the_sanitizers():
    """The shim with its own main, built with -fsanitize=address,undefined, as a stand-alone program over odd sizes."""
    prog = vr.sanitized_program()                                # a build failure fails the test
    r = subprocess.run([prog], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    assert all(int(x) > 0 for x in r.stdout.split()[1:]), r.stdout
