"""pais_depth_test and pais_cloud_visibility on the MI355X against the numpy restatement of their statements (tests/vis_ref.py)
over the renderer's restatement (_brute of tests/test_render_gpu.py): code, occluder and margin bit-equal on the ball rig, on
the edge list and on two walls with hand-derived expectations; the fused entry against render-then-test and against every
split; the soundness of the statements and of the default tolerance on the pawn's ground truth; and the driver's
depth-consistency filter with its command line."""
import copy
import math
import os

import numpy as np
import pytest

from tests import vis_ref as vr
from tests.test_knn_gpu import _alive, _loaded, grown  # noqa: F401  (grown: fixture)
from tests.test_render_gpu import CULL, DISC, _ball_splats, _ball_views, _brute, _same

pytestmark = pytest.mark.gpu

SPLIT_ENV = ("PAIS_RENDER_VIEWS", "PAIS_RENDER_SPLATS")


@pytest.fixture(autouse=True)
def _default_split(monkeypatch):
    for k in SPLIT_ENV:
        monkeypatch.delenv(k, raising=False)


# ------------------------------------------------------------------------------------------- 1. the ball rig, bit for bit ---
@pytest.mark.parametrize("W,H", [(37, 29), (65, 48)])
def test_codes_occluders_and_margins_equal_the_restatement_bit_for_bit(W, H):
    """n across the 64-lane wave and the 256-lane block, one view and three, the splats as their own queries with and without
    PAIS_VIS_SELF and 200 other queries in a ball of radius 1.5 (so that OUTSIDE and EMPTY occur), tol 0 and the median rho"""
    from pais_mvs_amd.render import visibility
    seen = set()
    for n in (1, 63, 64, 65, 300):
        for V in (1, 3):
            rng = np.random.default_rng(1000 * n + 10 * W + V)
            views = _ball_views(rng, V, W, H)
            c, nr, rho = _ball_splats(rng, n)
            q = rng.normal(size=(200, 3))
            q *= 1.5 * (rng.uniform(0, 1, size=(200, 1)) ** (1 / 3)) / np.linalg.norm(q, axis=1, keepdims=True)
            maps = _brute(DISC, CULL, c, nr, rho, views, W, H)
            for tol in (0.0, float(np.median(rho))):
                for queries, self_index in ((None, False), (None, True), (q, False)):
                    got = visibility(c, nr, views, W, H, queries=queries, radii=rho, tol=tol, self_index=self_index)
                    want = vr.ref_depth_test(c if queries is None else queries, views, maps[0], maps[1], tol, self_index)
                    vr.assert_same(got, want, (W, H, n, V, tol, queries is None, self_index))
                    seen |= set(np.unique(got.code).tolist())
                    assert got.render is None and got.kernel_ms > 0 and got.ms["render"] > 0 and got.ms["test"] > 0
    assert len(seen) >= 4, seen                                  # the sweep is not vacuous
    assert {vr.VISIBLE, vr.OCCLUDED, vr.EMPTY, vr.OUTSIDE} <= seen, seen


# ------------------------------------------------------------------------------------------------------- 2. the edge list ---
def test_edge_list_on_one_front_view():
    """pu at k + 0.5 for even and odd k, at -0.5 and W - 0.5, c'2 = 0 and < 0, |pu| = 2^30, a pixel holding +inf, m equal to tol,
    to -tol and to 0 from dyadic coordinates, tol = 0, and PAIS_VIS_SELF turning an OCCLUDED pair into VISIBLE"""
    from pais_mvs_amd.render import depth_test
    view, depth, idm, pts, tol, names, plain, with_self = vr.edge_case()
    for self_index, expect in ((False, plain), (True, with_self)):
        got = depth_test(pts, [view], depth, idm, tol=tol, self_index=self_index)
        vr.assert_same(got, vr.ref_depth_test(pts, [view], depth, idm, tol, self_index), ("edge", self_index))
        for k, name in enumerate(names):
            assert got.code[0, k] == expect[k], (name, self_index, int(got.code[0, k]), float(got.margin[0, k]))
    assert plain[13] == vr.OCCLUDED and with_self[13] == vr.VISIBLE
    got = depth_test(pts, [view], depth, idm, tol=tol)
    m = dict(zip(names, got.margin[0]))
    assert m["m == tol"] == tol and m["m == -tol"] == -tol and m["m == 0"] == 0.0
    assert got.occluder[0, 13] == 13 and got.occluder[0, names.index("a pixel holding +inf")] == -1
    zero = depth_test(pts, [view], depth, idm, tol=0.0)
    vr.assert_same(zero, vr.ref_depth_test(pts, [view], depth, idm, 0.0), "tol 0")
    z = dict(zip(names, zero.code[0]))
    assert z["m == 0"] == vr.VISIBLE and z["m == tol"] == vr.OCCLUDED and z["m == -tol"] == vr.IN_FRONT
    # without an id map every occluder is -1 and the codes are the same
    bare = depth_test(pts, [view], depth, None, tol=tol)
    assert np.array_equal(bare.code, got.code) and (bare.occluder == -1).all()
    assert vr.normalised(bare.margin).tobytes() == vr.normalised(got.margin).tobytes()
    # -inf and finite negative depths are compared as they are
    odd = depth.copy()
    odd[0, 20, 20], odd[0, 20, 22] = -np.inf, -3.0
    vr.assert_same(depth_test(pts, [view], odd, idm, tol=tol), vr.ref_depth_test(pts, [view], odd, idm, tol), "odd depths")


# ---------------------------------------------------------------------------------------------------------- 3. two walls ---
def test_two_walls_with_exact_expectations():
    """vis_ref.two_walls: far-wall points behind the near wall are OCCLUDED by the near disc of their pixel with margin exactly 2,
    the other far-wall points VISIBLE with margin 0 and their own id, a point at z = 1 IN_FRONT with margin -1; tol = 0.25"""
    from pais_mvs_amd.render import visibility
    view, W, H, cen, nrm, rad, qry, tol, code, occ, mar = vr.two_walls()
    got = visibility(cen, nrm, [view], W, H, queries=qry, radii=rad, tol=tol, keep_maps=True)
    assert (got.render.depth[0][:, :32] == 2.0).all() and (got.render.depth[0][:, 32:] == 4.0).all()
    assert np.array_equal(got.code[0], code) and np.array_equal(got.occluder[0], occ) and np.array_equal(got.margin[0], mar)
    assert (code == vr.OCCLUDED).sum() == 24 * 16 and (code == vr.VISIBLE).sum() == 24 * 16 and code[-1] == vr.IN_FRONT
    assert got.counts().tolist() == [[int(k == c) for k in range(6)] for c in code]
    assert got.visible_views() == [[0] if c == vr.VISIBLE else [] for c in code]


# ------------------------------------------------------------------------------------------------------ 4. the fused entry ---
def test_fused_entry_equals_render_then_test_whatever_the_split(monkeypatch):
    from pais_mvs_amd import _lib
    from pais_mvs_amd.render import depth_test, render, visibility
    W, H, n, V = 65, 48, 300, 5
    rng = np.random.default_rng(77)
    views = _ball_views(rng, V, W, H)
    c, nr, rho = _ball_splats(rng, n)
    tol = float(np.median(rho))
    want_maps = _brute(DISC, CULL, c, nr, rho, views, W, H)
    r = render(c, nr, views, W, H, radii=rho)
    _same(r, want_maps, "render through the refactored path")
    one = float(rho[n // 2])
    tiled = vr.brute_tiled(CULL, c, nr, one, views, W, H)
    full = _brute(DISC, CULL, c, nr, one, views, W, H)
    assert tiled[0].tobytes() == full[0].tobytes() and tiled[1].tobytes() == full[1].tobytes()      # the tiled restatement is the untiled one
    L = _lib.load()
    for self_index in (False, True):
        before = L.pais_render_launches()
        two = depth_test(c, views, r.depth, r.id, tol=tol, self_index=self_index)
        assert L.pais_render_launches() == before + 1            # one pass, one launch: the counter sees the new kernel
        vr.assert_same(two, vr.ref_depth_test(c, views, want_maps[0], want_maps[1], tol, self_index), ("two steps", self_index))
        kept = visibility(c, nr, views, W, H, radii=rho, tol=tol, self_index=self_index, keep_maps=True)
        bare = visibility(c, nr, views, W, H, radii=rho, tol=tol, self_index=self_index)
        assert kept.render.depth.tobytes() == r.depth.tobytes() and kept.render.id.tobytes() == r.id.tobytes()
        for got in (kept, bare):
            assert got.code.tobytes() == two.code.tobytes() and got.occluder.tobytes() == two.occluder.tobytes()
            assert got.margin.tobytes() == two.margin.tobytes()  # byte for byte, NaNs included: both come from one kernel
        only = visibility(c, nr, views, W, H, radii=rho, tol=tol, self_index=self_index, occluder=False, margin=False)
        assert only.code.tobytes() == two.code.tobytes() and only.occluder is None and only.margin is None
        for env in ({"PAIS_RENDER_VIEWS": "1"}, {"PAIS_RENDER_VIEWS": "2"}, {"PAIS_RENDER_SPLATS": "7"},
                    {"PAIS_RENDER_VIEWS": "2", "PAIS_RENDER_SPLATS": "7"}):
            for k in SPLIT_ENV:
                monkeypatch.delenv(k, raising=False)
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            got = visibility(c, nr, views, W, H, radii=rho, tol=tol, self_index=self_index, keep_maps=True)
            again = depth_test(c, views, r.depth, r.id, tol=tol, self_index=self_index)
            for g in (got, again):
                assert g.code.tobytes() == two.code.tobytes() and g.occluder.tobytes() == two.occluder.tobytes(), env
                assert g.margin.tobytes() == two.margin.tobytes(), env
            assert got.render.depth.tobytes() == r.depth.tobytes() and got.render.id.tobytes() == r.id.tobytes(), env
        for k in SPLIT_ENV:
            monkeypatch.delenv(k, raising=False)
    # no splat: every pixel empty, no query is tested against a surface; no query: the maps alone
    none = visibility(np.zeros((0, 3)), np.zeros((0, 3)), views, W, H, queries=c, radius=0.1, tol=0.1, keep_maps=True)
    assert np.isposinf(none.render.depth).all() and (none.render.id == -1).all() and set(np.unique(none.code).tolist()) <= {vr.EMPTY, vr.OUTSIDE, vr.BEHIND}
    vr.assert_same(none, vr.ref_depth_test(c, views, none.render.depth, none.render.id, 0.1), "no splat")
    maps_only = visibility(c, nr, views, W, H, queries=np.zeros((0, 3)), radii=rho, tol=tol, keep_maps=True)
    assert maps_only.code.shape == (V, 0) and maps_only.render.depth.tobytes() == r.depth.tobytes()


def test_points_beyond_one_launch():
    """The points of a pass go in launches of 2^20 (no knob sets that size, so the test uses it): 2 x 2^20 + 77 queries are two
    full launches and a partial one, each starting at a non-zero point offset, against two views; all three outputs bit-equal
    to the restatement, through both entries"""
    from pais_mvs_amd import _lib
    from pais_mvs_amd.render import depth_test, visibility
    W, H, n, V, nq = 37, 29, 300, 2, 2 * (1 << 20) + 77
    rng = np.random.default_rng(2020)
    views = _ball_views(rng, V, W, H)
    c, nr, rho = _ball_splats(rng, n)
    q = rng.normal(size=(nq, 3))
    q *= 1.5 * (rng.uniform(0, 1, size=(nq, 1)) ** (1 / 3)) / np.linalg.norm(q, axis=1, keepdims=True)
    tol = float(np.median(rho))
    maps = _brute(DISC, CULL, c, nr, rho, views, W, H)
    want = vr.ref_depth_test(q, views, maps[0], maps[1], tol)
    L = _lib.load()
    before = L.pais_render_launches()
    two = depth_test(q, views, maps[0], maps[1], tol=tol)
    assert L.pais_render_launches() == before + 3
    vr.assert_same(two, want, "three launches, the caller's maps")
    vr.assert_same(visibility(c, nr, views, W, H, queries=q, radii=rho, tol=tol), want, "three launches, fused")
    for k in (0, (1 << 20) - 1, 1 << 20, 2 * (1 << 20), nq - 1):       # the seams, explicitly
        assert two.code[:, k].tolist() == want[0][:, k].tolist(), k
    assert len(set(np.unique(two.code).tolist())) >= 4


def test_refusals_launch_nothing_beside_a_device():
    from pais_mvs_amd import _lib
    from pais_mvs_amd.render import depth_test, make_view, visibility
    view = make_view(np.eye(3), np.zeros(3), (20.0, 20.0), (8.0, 6.0))
    pts = np.tile([0.0, 0.0, 3.0], (4, 1))
    nrm = np.tile([0.0, 0.0, -1.0], (4, 1))
    d = np.full((1, 12, 16), 3.0)
    assert (depth_test(pts, [view], d, tol=0.0).code == vr.VISIBLE).all()           # the device is up
    L = _lib.load()
    before = L.pais_render_launches()
    bad = d.copy()
    bad[0, 0, 0] = np.nan
    for call in (lambda: depth_test(pts, [view], bad), lambda: depth_test(pts, [view], d, tol=-1.0), lambda: depth_test(np.full((4, 3), np.inf), [view], d),
                 lambda: visibility(pts, nrm, [view], 16, 12, radius=0.1, tol=float("nan")), lambda: visibility(pts, nrm, [view], 16, 12, radius=-0.1, tol=0.1),
                 lambda: visibility(pts, nrm, [view], 0, 12, radius=0.1)):
        with pytest.raises(RuntimeError, match="pais_depth_test:|pais_cloud_visibility:"):
            call()
    assert L.pais_render_launches() == before


# ------------------------------------------------------------------------------------------------------------ 5. soundness ---
def analytic_visibility(scene, pts, nrm):
    """(cameras, n) bool: the point is front-facing (-(d . n) > 0) and unoccluded (the solid's nearest hit along the viewing ray is
    the point's own distance within 1e-6 max(1, dist), as synth.visible_counts tests it)"""
    out = np.zeros((len(scene.cameras), len(pts)), bool)
    for k, cam in enumerate(scene.cameras):
        v = pts - cam.center
        dist = np.sqrt(np.einsum("ij,ij->i", v, v))
        d = v / dist[:, None]
        t = scene.obj.intersect(cam.center, d)
        out[k] = (-np.einsum("ij,ij->i", d, nrm) > 0) & np.isfinite(t) & ~(np.abs(t - dist) > 1e-6 * np.maximum(1.0, dist))
    return out


SOUND_VISIBLE_SHARE, SOUND_HIDDEN_MISSES = 28969 / 29447, 5      # from the numpy restatement on a CPU: the docstring below


def test_the_statements_are_sound_on_the_pawn_truth(pawn_small):
    """synth.ground_truth(pawn_small, stride=2) as discs of radius `spacing` with CULL_BACK into the five scene cameras,
    tol = spacing, no SELF, against the analytic truth per (point, camera) of analytic_visibility.

    Measured on the numpy restatement alone, on a CPU (5922 points, 29610 pairs, spacing 0.0067956):
        truly visible 29447:  VISIBLE 28969 (0.98377)  OCCLUDED 262  IN_FRONT 45  EMPTY 171
        truly hidden    163:  VISIBLE 5                OCCLUDED 111  IN_FRONT 0   EMPTY 47
    The test measures both on its own restatement (vis_ref over the tiled _brute, which test_fused_entry_... checks against the
    untiled one) and asserts the first share with 2 percentage points of slack (>= 0.96377) and at most twice the 5 misses
    (<= 10 hidden pairs coded VISIBLE).  The GPU's codes are bit-equal to the restatement's, so it meets the same bounds: the
    statements and the default tolerance are sound.  At tol = 0 only 3 of the 29447 visible pairs are VISIBLE (a disc's hit is
    not its centre): below 1 %, which is why the tolerance exists."""
    from pais_mvs_amd import synth
    from pais_mvs_amd.render import view_of, visibility
    pts, nrm, spacing = synth.ground_truth(pawn_small, stride=2)
    views = [view_of(cam) for cam in pawn_small.cameras]
    W, H = pawn_small.cameras[0].width, pawn_small.cameras[0].height
    truth = analytic_visibility(pawn_small, pts, nrm)
    maps = vr.brute_tiled(CULL, pts, nrm, spacing, views, W, H)
    want = vr.ref_depth_test(pts, views, maps[0], maps[1], spacing)
    got = visibility(pts, nrm, views, W, H, radius=spacing, self_index=False, keep_maps=True)      # tol defaults to the radius
    assert got.render.depth.tobytes() == maps[0].tobytes() and got.render.id.tobytes() == maps[1].tobytes()
    vr.assert_same(got, want, "pawn truth")
    code = want[0]
    share = ((code == vr.VISIBLE) & truth).sum() / truth.sum()
    misses = int(((code == vr.VISIBLE) & ~truth).sum())
    print("\npawn truth: %d points, %d visible pairs: %s; %d hidden pairs: %s; share %.5f misses %d; render %.3f ms test %.3f ms"
          % (len(pts), truth.sum(), [int(((code == k) & truth).sum()) for k in range(6)], (~truth).sum(),
             [int(((code == k) & ~truth).sum()) for k in range(6)], share, misses, got.ms["render"], got.ms["test"]))
    assert share >= SOUND_VISIBLE_SHARE - 0.02 and misses <= 2 * SOUND_HIDDEN_MISSES, (share, misses)
    zero = vr.ref_depth_test(pts, views, maps[0], maps[1], 0.0)[0]
    assert zero.tobytes() == visibility(pts, nrm, views, W, H, radius=spacing, tol=0.0, self_index=False).code.tobytes()
    assert ((zero == vr.VISIBLE) & truth).sum() < 0.01 * truth.sum()


# ----------------------------------------------------------------------------------------------------------- 6. the filter ---
PLANTED, PLANT_DEPTH = 300, 5.0
GENUINE_REMOVED_SHARE = 0.0          # measured on the numpy restatement, on a CPU: the docstring of the filter test


def normal_to_spherical(n):
    return [math.acos(max(-1.0, min(1.0, float(n[2])))), math.atan2(float(n[1]), float(n[0]))]


def planted_cloud(scene, stride=4, seed=5):
    """The pawn truth with each point's analytically visible cameras as its list, then PLANTED of its points pushed PLANT_DEPTH x
    spacing behind the surface along the viewing ray of their first visible camera, listing all cameras.

    A pushed point can only be asked of the filter where it IS behind a surface the cloud holds: along a grazing ray it leaves
    the solid again and floats in free space in sight of the other cameras, and the truth has no samples where fewer than three
    cameras see the surface (the rims of every view stay open, tests/test_render_gpu.py), so there no disc is in front of it.
    Both are decided analytically, before anything is rendered: a site is taken only if, from every camera, the ray to the
    pushed point meets the solid in front of it, and that hit is itself a place the truth samples (synth.visible_counts >= 3,
    the rule ground_truth keeps a sample by).  PLANTED sites are drawn from those.
    -> (rows for load_patch, planted mask, spacing)"""
    from pais_mvs_amd import synth
    pts, nrm, spacing = synth.ground_truth(scene, stride=stride)
    truth = analytic_visibility(scene, pts, nrm)
    rows = [(p.tolist(), normal_to_spherical(n), np.flatnonzero(truth[:, i]).tolist(), 0.5, 0.9) for i, (p, n) in enumerate(zip(pts, nrm))]
    centre = np.array([scene.cameras[r[2][0]].center for r in rows])
    d = pts - centre
    pushed = pts + PLANT_DEPTH * spacing * d / np.linalg.norm(d, axis=1, keepdims=True)
    site = np.ones(len(pts), bool)
    for cam in scene.cameras:
        v = pushed - cam.center
        dist = np.linalg.norm(v, axis=1)
        t, part = scene.obj.intersect_parts(cam.center, v / dist[:, None])
        hidden = t < dist - 1e-6 * np.maximum(1.0, dist)
        hit = cam.center[None, :] + np.where(hidden, t, 1.0)[:, None] * v / dist[:, None]
        site &= hidden & (synth.visible_counts(scene.obj, hit, scene.obj.part_normals(hit, np.maximum(part, 0)), scene.cameras) >= 3)
    rng = np.random.default_rng(seed)
    for i in rng.choice(np.flatnonzero(site), size=PLANTED, replace=False):
        rows.append((pushed[i].tolist(), rows[i][1], list(range(len(scene.cameras))), 0.5, 0.9))
    planted = np.arange(len(rows)) >= len(pts)
    return rows, planted, spacing


def filter_config(rows, spacing):
    """readme_config with neighborRadiusScalar chosen so that the neighbour radius the filters set on a fresh cloud (the cube root
    of the bounding volume times the scalar) is the cloud's spacing: the discs then cover the surface"""
    from pais_mvs_amd.config import readme_config
    c = np.array([r[0] for r in rows])
    ext = c.max(axis=0) - c.min(axis=0)
    return readme_config(neighborRadiusScalar=spacing / float(abs(ext[0] * ext[1] * ext[2])) ** (1.0 / 3.0))


def predicted_outliers(cloud, lists, views, W, H, rho, min_visible):
    """the restatement of the filter: discs of rho with CULL_BACK, the centres tested with PAIS_VIS_SELF and tol = rho, the rule"""
    maps = vr.brute_tiled(CULL, cloud[:, :3], cloud[:, 3:], rho, views, W, H)
    code = vr.ref_depth_test(cloud[:, :3], views, maps[0], maps[1], rho, True)[0]
    return np.array(vr.rule_loop(code, lists, min_visible)[1], bool)


def test_depth_filtering_deletes_what_the_restatement_predicts(pawn_small):
    """The planted cloud of planted_cloud (stride 4: 1486 genuine points, 300 planted) through MVS.depthFiltering() with its
    defaults: exactly the set that vis_ref and the rule give for the driver's own centres, stored normals, camera lists and
    neighbour radius goes; every planted point is in it; a second call removes what the restatement predicts for the thinned
    cloud; the survivors' records are untouched.

    Measured on the numpy restatement alone, on a CPU (1786 patches, spacing 0.0135887): the first call removes 300, all 300
    planted (each OCCLUDED in all five cameras) and 0 of the 1486 genuine points -- GENUINE_REMOVED_SHARE = 0.0, the share the
    driver may not exceed; the second call removes nothing."""
    from pais_mvs_amd.mvs import MVS
    from pais_mvs_amd.render import view_of
    rows, planted, spacing = planted_cloud(pawn_small)
    cfg = filter_config(rows, spacing)
    views = [view_of(cam) for cam in pawn_small.cameras]
    W, H = pawn_small.cameras[0].width, pawn_small.cameras[0].height
    m = _loaded(cfg, pawn_small.cameras, rows)
    ids = _alive(m)
    assert ids == list(range(len(rows)))
    cloud = m.cloud()
    lists = [r[2] for r in rows]
    before = {i: bytes(m.get_patch(i)) for i in ids}
    removed, ms = m.depthFiltering()
    rho = m.neighbor_radius()
    assert abs(rho - spacing) < 1e-9 * spacing
    want = predicted_outliers(cloud, lists, views, W, H, rho, cfg.minCamNum)
    gone = np.array([i not in set(_alive(m)) for i in ids])
    genuine = int((gone & ~planted).sum())
    print("\nplanted cloud of %d: %d removed (%d planted of %d, %d genuine of %d = %.5f), rho %.6g, %.3f ms"
          % (len(rows), removed, (gone & planted).sum(), planted.sum(), genuine, (~planted).sum(), genuine / (~planted).sum(), rho, ms))
    assert np.array_equal(gone, want) and removed == int(want.sum()) == len(rows) - m.num_patches() and ms > 0
    assert gone[planted].all(), "a planted point survived"
    assert genuine / (~planted).sum() <= GENUINE_REMOVED_SHARE
    for i in _alive(m):
        assert bytes(m.get_patch(i)) == before[i], i
    # the thinned cloud
    keep = np.flatnonzero(~gone)
    want2 = predicted_outliers(cloud[keep], [lists[i] for i in keep], views, W, H, rho, cfg.minCamNum)
    removed2, _ = m.depthFiltering()
    assert m.neighbor_radius() == rho
    assert _alive(m) == [int(i) for i in keep[~want2]] and removed2 == int(want2.sum())
    # explicit arguments: a tolerance that nothing exceeds removes nothing
    assert m.depthFiltering(rho=rho, tol=1e6)[0] == 0
    vis = m.visibility()
    assert vis.code.shape == (len(views), m.num_patches())
    m.close()
    host = MVS(cfg, pawn_small.cameras, device=-1, seed=42)
    with pytest.raises(RuntimeError, match="no GPU context"):
        host.depthFiltering()
    host.close()


def test_visible_cameras_of_a_cloud_without_images(pawn_small):
    from pais_mvs_amd import evaluate, synth
    pts, nrm, spacing = synth.ground_truth(pawn_small, stride=4)
    cloud = np.concatenate([pts, nrm], axis=1)
    seen = evaluate.visible_cameras(cloud, pawn_small.cameras, radius=spacing)
    truth = analytic_visibility(pawn_small, pts, nrm)
    agree = sum(len(set(s) & set(np.flatnonzero(truth[:, i]).tolist())) for i, s in enumerate(seen))
    assert len(seen) == len(pts) and agree >= 0.96 * truth.sum()          # with SELF at least the soundness test's share
    assert evaluate.visible_cameras(cloud, pawn_small.cameras) == evaluate.visible_cameras(cloud, pawn_small.cameras, radius=evaluate.spacing(pts))


def test_command_lines(tmp_path, pawn_small, grown, capsys):  # noqa: F811
    """--filter --depth-consistency RHO,TOL writes DC_filter.* with the driver's patch count after the other files, which it
    leaves byte for byte as they are; view --visibility prints the per-camera histogram of the codes"""
    import json
    from PIL import Image
    from pais_mvs_amd import evaluate, io, reconstruct, view
    from pais_mvs_amd import render as rnd
    cfg, cl = copy.copy(grown[0]), grown[1]
    cams = []
    for i, cam in enumerate(pawn_small.cameras):
        c = copy.copy(cam)
        c.name = "cam%d.png" % i
        Image.fromarray(np.repeat(cam.pyramid[0][:, :, None], 3, axis=2)).save(str(tmp_path / c.name))
        cams.append(c)
    m = _loaded(cfg, cams, cl)
    path = str(tmp_path / "cloud.mvs")
    m.writeMVS(path)
    m.close()
    a, b = tmp_path / "plain", tmp_path / "dc"
    a.mkdir()
    b.mkdir()
    common = [path, "--filter", "--config", str(tmp_path / "none.txt")]
    reconstruct.main(common + ["--out", str(a)])
    reconstruct.main(common + ["--out", str(b), "--depth-consistency", "auto,auto"])
    today = {s + e for s in ("PMVS_filter1", "PMVS_filter2", "PMVS_filter3", "PCMVS_filter") for e in (".mvs", ".ply")}
    assert set(os.listdir(a)) == today and set(os.listdir(b)) == today | {"DC_filter.mvs", "DC_filter.ply"}
    for f in today:
        assert (a / f).read_bytes() == (b / f).read_bytes(), f
    # the same chain through the driver
    file_cfg, cams_io, pats = io.load_mvs(path)
    m = _loaded(file_cfg, reconstruct.load_cameras(cams_io, str(tmp_path), file_cfg),
                [(p.center[:], p.normalS[:], list(p.cam_idx[:p.num_cam]), p.fitness, p.correlation) for p in pats])
    m.cellFiltering(); m.visibilityFiltering(); m.neighborCellFiltering(0.25); m.neighborPatchFiltering(0.25)
    n_before = m.num_patches()
    removed, _ = m.depthFiltering()
    dc = io.load_mvs(str(b / "DC_filter.mvs"))[2]
    assert len(io.load_mvs(str(b / "PCMVS_filter.mvs"))[2]) == n_before
    assert len(dc) == m.num_patches() == n_before - removed and 0 < len(dc)
    assert [list(p.center[:]) for p in dc] == [list(p.center[:]) for p in m.patches()]
    assert m.visibility([0, 2]).code.shape == (2, len(dc))
    m.close()
    # what the command line reads: the file's centres, the normals of its spherical angles, its cameras and its neighbour radius
    dc_cfg, dc_cams, _ = io.load_mvs(str(b / "DC_filter.mvs"))
    cloud = evaluate.load_cloud(str(b / "DC_filter.mvs"))
    wh = [int(2 * dc_cams[0].principle_point[k]) for k in (0, 1)]
    counts = rnd.visibility(cloud[:, :3], cloud[:, 3:], [rnd.view_of(dc_cams[i]) for i in (0, 2)], wh[0], wh[1],
                            radius=dc_cfg.neighborRadius).view_counts()
    assert counts.sum() == 2 * len(dc) and counts[:, 0].min() > 0
    capsys.readouterr()
    assert view.main([str(b / "DC_filter.mvs"), "--camera", "0", "2", "--visibility", "--out", str(tmp_path / "v")]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    out = json.loads(lines[-1])
    assert [r["camera"] for r in out["visibility"]] == [0, 2]
    assert [[r[k] for k in ("visible", "occluded", "in_front", "empty", "outside", "behind")] for r in out["visibility"]] == counts.tolist()
    assert lines[-3].startswith("camera 0: visible ") and lines[-2].startswith("camera 2: visible ")
