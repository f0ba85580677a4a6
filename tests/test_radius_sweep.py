"""The window radius swept through every path that depends on it, against the oracle AND against tests/refcost.py, a plain
float64 restatement that shares no code with either side.

The window side S = 2 r + 1 shapes the kernels: the padding of the last 64-pixel step (S^2 < 64: a single partial step), the
window strips of the tile kernel, the corner test that drops the per-tap bounds check, the LDS / global-scratch switch of
the warped patches of the after-stage and of pais_ncc_batch (8 K S^2 bytes against 60 KB), and the x / y tables of the
literal arithmetic (PAIS_ARITH=literal).  Radii:
  1, 2, 3         S^2 = 9, 25, 49: a single partial step;  4: 81 pixels, one full step and a partial one
  7, 8, 15        ordinary windows (15: the README configuration)
  19, 20          the two sides of the LDS / slab switch at K = 5 (60 840 B / 67 240 B of warped patches)
  31, 32, 33      the two sides of 64 window columns (the literal tables held 64 entries before they were sized by S)
  47, 63          large windows;  127: the largest radius pais_ctx_create accepts
distWeighting = r / 3 as default_config sets it.  r <= 20 runs on the small pawn (five cameras), larger radii on the small
ring (480 x 360, windows of up to 261 pixels at level 0).

Besides the particles of tests/test_gpu_parity.py (valid interior, random, back-facing, far off), two kinds are added:
particles whose depth is bisected until exactly one warped window corner of one camera lies just past the image bound (and
the last one before it), and particles whose plane is nearly edge-on to the reference camera's ray, so that the
homogeneous coordinate w of other cameras changes sign across the window.  An evaluation is compared only where refcost's
margin (tests/refcost.py) is at least 1e-7; the skips are counted and bounded.
"""
import math

import numpy as np
import pytest

from tests import common, pipelines as P, refcost
from tests.common import compare_patch, oracle_records
from tests.refcost import MARGIN, check_against_refcost, check_counts
from tests.golden import make_ncc_golden as G

R = (1, 2, 3, 4, 7, 8, 15, 19, 20, 31, 32, 33, 47, 63, 127)
REFINE_R = (1, 3, 4, 19, 20, 32, 33, 63)
RTOL_KERNEL = 1e-9          # the kernel arithmetic against refcost (RTOL_FIT of tests/test_gpu_parity.py)
LDS_HP_LIMIT = 60 * 1024    # warped patches in LDS up to this many bytes (pais_capi.hip pais_ncc_batch, pais_kernels.hip after)


def _cfg(r, **over):
    from pais_mvs_amd.config import readme_config
    return readme_config(patchRadius=r, distWeighting=r / 3.0, **over)


def _scene(request, r):
    return request.getfixturevalue("pawn_small" if r <= 20 else "ring_small")


def _det_normal(th, ph):
    """spherical2normal with the deterministic sin / cos of the kernel arithmetic, costLiteral and PAIS_ARITH=literal."""
    from oracle import po
    L = po.lib()
    return refcost.spherical_to_normal(th, ph, sin=L.po_sin_det, cos=L.po_cos_det)


# ---------------------------------------------------------------------------------------------------------------------
# the two added kinds of particles
# ---------------------------------------------------------------------------------------------------------------------
def _corners(scene, cfg, st, pos):
    """(largest excess of a warped window corner past [2, dim-3) over the other cameras, corners past it, one sign of w at
    the corners of every camera)."""
    cams = scene.cameras
    n = refcost.spherical_to_normal(pos[0], pos[1])
    rc = cams[st.ref]
    center = [st.ray[i] * pos[2] + float(rc.center[i]) for i in range(3)]
    H = refcost.homographies(cams, st, center, n, cfg.lodRatio)
    pt = refcost.project(rc, center, cfg.lodRatio ** st.lod)
    r = cfg.patchRadius
    X = np.array([pt[0] - r, pt[0] + r, pt[0] - r, pt[0] + r])
    Y = np.array([pt[1] - r, pt[1] - r, pt[1] + r, pt[1] + r])
    worst, n_out, one_sign = -math.inf, 0, True
    for i, c in enumerate(st.cams):
        if c == st.ref:
            continue
        rows, cols = refcost.level_shape(cams[c], st.lod)
        w, ix, iy = refcost._warp(H[i], X, Y)
        one_sign = one_sign and (bool(np.all(w > 0)) or bool(np.all(w < 0)))
        e = np.maximum.reduce([2 - ix, ix - (cols - 3), 2 - iy, iy - (rows - 3)])
        n_out += int((e > 0).sum())
        worst = max(worst, float(np.max(e)))
    return worst, n_out, one_sign


def _corner_particles(scene, cfg, st, base):
    """Depths on both sides of the first warped corner crossing an image bound, moving the patch along the reference ray:
    the first one past it has exactly one corner 1e-4 .. 0.05 pixel outside."""
    out = []
    e0 = _corners(scene, cfg, st, base)
    if not (e0[2] and e0[0] < 0):
        return out
    for direction in (-1.0, 1.0):
        far = None
        for k in range(1, 40):
            s = 1.0 + direction * 0.02 * k
            e = _corners(scene, cfg, st, (base[0], base[1], base[2] * s))
            if not e[2]:
                break
            if e[0] > 0:
                far = s
                break
        if far is None:
            continue
        lo, hi = 1.0, far
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            e = _corners(scene, cfg, st, (base[0], base[1], base[2] * mid))
            if e[0] > 0:
                hi = mid
            else:
                lo = mid
            if e[0] > 0 and 1e-4 < e[0] < 0.05:
                break
        e_hi = _corners(scene, cfg, st, (base[0], base[1], base[2] * hi))
        if e_hi[1] == 1 and 1e-4 < e_hi[0] < 0.05:
            out.append((base[0], base[1], base[2] * hi))
            out.append((base[0], base[1], base[2] * lo))
    return out


def _edge_on_particles(scene, cfg, st, base):
    """Planes nearly edge-on to the reference camera, tilted so that w of a target camera changes sign across the window.
    With d the unit ray of a window pixel, the homogeneous w of camera c is proportional to m . d, m = z0 n + k o_c (z0: depth
    of the reference centre in camera c, k = depth (n . d0), o_c: its optical axis); for n . d0 = -eps that is -eps z_c(X)
    at the window centre X and varies by about z0 (n . dd) across it.  So n = t - eps d0, t along the reference camera's x
    axis, eps a fraction of a |z0| / z_c(X) (a: the window's half-angle) for the camera with the largest |z0| / z_c(X)."""
    cams = scene.cameras
    cam = cams[st.ref]
    d = np.asarray(st.ray, float)
    d = d / np.linalg.norm(d)
    X = np.asarray(cam.center, float) + base[2] * np.asarray(st.ray, float)
    depth_in = lambda c, P: float(np.asarray(cams[c].rotation, float)[2] @ (P - np.asarray(cams[c].center, float)))
    q = max(abs(depth_in(c, np.asarray(cam.center, float))) / depth_in(c, X) for c in st.cams if c != st.ref)
    a = cfg.patchRadius / (float(cam.focal[0]) * cfg.lodRatio ** st.lod)
    x = np.asarray(cam.rotation, float)[0]
    t = x - (x @ d) * d
    t = t / np.linalg.norm(t)
    out = []
    for frac in (0.2, 0.5, 0.8):
        n = t - frac * a * q * d
        n = n / np.linalg.norm(n)
        out.append((math.acos(float(n[2])), math.atan2(float(n[1]), float(n[0])), base[2]))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the evaluations of one radius: states, particles, refcost and the three oracle arithmetics (shared by CPU and GPU tests)
# ---------------------------------------------------------------------------------------------------------------------
_EVALS = {}


def _evals(request, r):
    if r in _EVALS:
        return _EVALS[r]
    from tests.test_gpu_parity import _states_and_particles
    scene, cfg = _scene(request, r), _cfg(r)
    S = common.oracle_scene(cfg, scene)
    rng = np.random.default_rng(1000 + r)
    states, pats, idx, parts = _states_and_particles(S, scene, rng, n_per=24 if r >= 47 else 12)
    kinds = ["sample"] * len(parts)
    for si, p in enumerate(pats):
        st = refcost.state_of(p)
        base = (p.normalS[0], p.normalS[1], p.depth)
        for kind, extra in (("corner", _corner_particles(scene, cfg, st, base)), ("edge_on", _edge_on_particles(scene, cfg, st, base))):
            for pos in extra:
                idx.append(si)
                parts.append(list(pos))
                kinds.append(kind)
    ref, ref_det, lit, clit, ker = [], [], [], [], []
    for si, pos in zip(idx, parts):
        st = refcost.state_of(pats[si])
        ref.append(refcost.cost(scene, cfg, st, pos))
        ref_det.append(refcost.cost(scene, cfg, st, pos, normal_fn=_det_normal))
        S.set_kernel_arithmetic(False)
        S.set_cost_literal(False)
        lit.append(S.fitness(pats[si], pos))            # the reference's statements, platform libm
        S.set_kernel_arithmetic(True)
        S.set_cost_literal(True)
        clit.append(S.fitness(pats[si], pos))           # the same statements, deterministic exp / sin / cos
        S.set_cost_literal(False)
        ker.append(S.fitness(pats[si], pos))            # the kernel arithmetic
    S.close()
    ev = dict(scene=scene, cfg=cfg, states=states, pats=pats, idx=idx, parts=parts, kinds=kinds, ref=ref, ref_det=ref_det,
              lit=lit, clit=clit, ker=ker)
    _EVALS[r] = ev
    return ev


# ------------------------------------------------------------------------------------------------------------- CPU ---
@pytest.mark.parametrize("r", R)
def test_oracle_cost_matches_refcost(request, r):
    """The oracle's literal cost and its costLiteral within the literal gate of refcost, its kernel arithmetic within 1e-9;
    DBL_MAX exactly where refcost says so.  The added particles: at least one just past a window corner per radius, and
    some edge-on plane whose w changes sign over the window of a camera."""
    ev = _evals(request, r)
    S = 2 * r + 1
    gate = refcost.literal_gate(S)
    c1 = check_against_refcost(r, ev["ref"], ev["lit"], gate, "oracle literal")
    c2 = check_against_refcost(r, ev["ref_det"], ev["clit"], gate, "oracle costLiteral")
    c3 = check_against_refcost(r, ev["ref"], ev["ker"], RTOL_KERNEL, "oracle kernel arithmetic")
    for c, what in ((c1, "literal"), (c2, "costLiteral"), (c3, "kernel")):
        check_counts(ev, c, what)
    corner = [c for c, k in zip(ev["ref"], ev["kinds"]) if k == "corner"]
    assert len(corner) >= 2, (r, len(corner))
    edge = [(si, pos) for si, pos, k in zip(ev["idx"], ev["parts"], ev["kinds"]) if k == "edge_on"]
    flips = sum(not _corners(ev["scene"], ev["cfg"], refcost.state_of(ev["pats"][si]), pos)[2] for si, pos in edge)
    assert flips >= 1, (r, flips, len(edge))


def _ncc_states(ev, S, rng):
    """View states of one radius: the heads of the evaluation states (centre, normal, reference camera, LOD, cameras) and
    make_ncc_golden's perturbations, subsets, searched tilts and edge states around them."""
    recs = [(list(p.center[:]), list(p.normal[:]), p.refCamIdx, p.LOD, p.cams(), p.cams()) for p in ev["pats"]]
    return G.scene_states(S, ev["scene"], recs[:8], rng, n_search=4)


def _check_tables(r, cfg, scene, states, wants, what):
    gate = refcost.table_gate(2 * r + 1)
    n_tab = n_drop = skipped = 0
    for i, (st, want) in enumerate(zip(states, wants)):
        t = refcost.ncc_table(scene, cfg, st)
        if t.margin < MARGIN:
            skipped += int(not st["kind"].startswith("edge_"))   # (the edge states are bisected to the last bit of the bound)
            continue
        assert t.dropped == (want["dropped"] == G.DROP_SAMPLE), (what, r, i, st["kind"], t.dropped, want["dropped"])
        if t.dropped:
            n_drop += 1
            continue
        n_tab += 1
        K = len(st["cams"])
        got = np.asarray(want["table"], float).reshape(K, K)
        err = float(np.max(np.abs(got - t.table)))
        assert err <= gate, (what, r, i, st["kind"], err, gate)
    return n_tab, n_drop, skipped


@pytest.mark.parametrize("r", R)
def test_oracle_ncc_table_matches_refcost(request, r):
    """G.oracle_ncc's table (kernel arithmetic, and the literal arithmetic) within 4 S^2 2^-53 of refcost.ncc_table; the
    sample-out-of-image drop exactly where refcost's margin allows."""
    ev = _evals(request, r)
    S = common.oracle_scene(ev["cfg"], ev["scene"])
    S.set_kernel_arithmetic(True)
    states = _ncc_states(ev, S, np.random.default_rng(2000 + r))
    assert len(states) >= 8, (r, len(states))
    for kernel in (True, False):
        S.set_kernel_arithmetic(kernel)
        wants = [G.oracle_ncc(S, st) for st in states]
        n_tab, n_drop, skipped = _check_tables(r, ev["cfg"], ev["scene"], states, wants, "kernel" if kernel else "literal")
        assert n_tab >= 4 and skipped <= 2, (r, kernel, n_tab, n_drop, skipped)
    S.close()


# ------------------------------------------------------------------------------------------------------------- GPU ---
@pytest.mark.gpu
@pytest.mark.parametrize("r", R)
def test_gpu_cost_every_radius(request, r, monkeypatch):
    """Context.fitness_batch at radius r: the default arithmetic equals the oracle's kernel arithmetic bit for bit and
    refcost within 1e-9; PAIS_ARITH=literal equals costLiteral bit for bit and refcost within the literal gate; byte taps
    (PAIS_TAP_FLOAT_MAX_MB=0) give the default's bits."""
    ev = _evals(request, r)
    scene, cfg = ev["scene"], ev["cfg"]

    def run(env):
        return P.fitness(monkeypatch, cfg, scene.cameras, ev["states"], ev["idx"], ev["parts"], env)

    got = run({})
    for e, (g, want) in enumerate(zip(got, ev["ker"])):
        assert common.same_value(g, want, 0.0), ("default", r, e, ev["kinds"][e], g, want)
    check_counts(ev, check_against_refcost(r, ev["ref"], got, RTOL_KERNEL, "HIP default"), "HIP default")
    lit = run(P.LITERAL)
    for e, (g, want) in enumerate(zip(lit, ev["clit"])):
        assert common.same_value(g, want, 0.0), ("literal", r, e, ev["kinds"][e], g, want)
    check_counts(ev, check_against_refcost(r, ev["ref_det"], lit, refcost.literal_gate(2 * r + 1), "HIP literal"), "HIP literal")
    byte = run(P.BYTE_TAPS)
    assert byte.tobytes() == got.tobytes(), (r, int(np.sum(byte != got)))


def _refine_scene(request, r, many):
    if many:
        return request.getfixturevalue("dome_small")
    return _scene(request, r)


def _refine_candidates(S, scene, n_seeds):
    """Seeds and two first-ring children each (the patch constructor with expandVisibleCamera) -> (candidates, is_seed)."""
    from pais_mvs_amd.context import make_candidate
    cands, is_seed = [], []
    for i, (X, vis) in enumerate(scene.seeds[:n_seeds]):
        p = S.seed_patch(X, vis, key=i)
        cands.append(make_candidate(p.center[:], p.normal[:], p.cams(), i, 0, normalS=p.normalS[:]))
        is_seed.append(True)
        for j in range(2):
            cen = [p.center[0] + 0.002 * (j - 0.5), p.center[1] + 0.001 * j, p.center[2] - 0.001 * j]
            key = 7000 + 10 * i + j
            child = S.expand_patch(cen, p.normal[:], p.cams(), key)
            cands.append(make_candidate(child.center[:], child.normal[:], child.cams(), key, 1, normalS=child.normalS[:]))
            is_seed.append(False)
    return cands, is_seed


@pytest.mark.gpu
@pytest.mark.parametrize("many", [False, True], ids=["few_cameras", "many_cameras"])
@pytest.mark.parametrize("r", REFINE_R)
def test_gpu_refine_pipelines_every_radius(request, r, many, monkeypatch, capfd):
    """refine() of seeds and first-ring children at radius r (particleNum 6, maxIteration 8) through every evaluation
    pipeline: the same record bytes, equal to the oracle bit for bit.  Few cameras: k_pso_iter, k_pso_eval2 + k_pso_step,
    k_pso_ring and PAIS_ARITH=literal (against costLiteral).  Many cameras (dome, K > 12): the tile kernel, every
    particle verified through k_pso_eval2.  The after-stage computes the records'
    correlation and camera sets on both sides of its LDS / scratch switch over the radii."""
    scene = _refine_scene(request, r, many)
    # maxFitness 100: the cost grows with the window (about 25 at r = 63 on the ring against the README's limit of 10), and a
    # dropped record would not reach the after-stage
    cfg = _cfg(r, particleNum=6, maxIteration=8, maxFitness=100.0,
               **({"reduceNormalRange": 4.0, "visibleCorrelation": 0.6} if many else {}))
    S = common.oracle_scene(cfg, scene)
    S.set_kernel_arithmetic(True)
    S.set_omp(True)
    cands, is_seed = _refine_candidates(S, scene, 8 if many else 12)
    want = oracle_records(S, cands, is_seed)

    def run(env):
        return P.refine(monkeypatch, cfg, scene.cameras, cands, env)

    ref, _ = run(P.NO_TILE if many else {})
    alive = 0
    for i, p in enumerate(want):
        compare_patch(ref[i], p, (r, "default", i, "seed" if is_seed[i] else "child"))
        alive += 0 if p.drop else 1
    assert alive >= 4, (r, alive, len(want))
    if many:
        assert max(c.num_cam for c in cands) > 12
        got, ks = run(P.TILE_VERIFIED)
        assert bytes(got) == bytes(ref), (r, "tile")
        P.assert_took("tile", ks, r)
        assert "tile verify" not in capfd.readouterr().out
    else:
        got, ks = run(P.EVAL2)
        P.assert_took("eval2", ks, r)
        assert bytes(got) == bytes(ref), (r, "k_pso_eval2 + k_pso_step")
        # (a batch with seeds takes the ring only from PAIS_RING_SEED_ABOVE evaluation waves per iteration on)
        got, ks = run(P.RING)
        P.assert_took("ring", ks, r)
        assert ks.ring_launches == ks.eval2_launches, (r, ks.ring_launches, ks.eval2_launches, ks.ring_fallbacks)
        assert bytes(got) == bytes(ref), (r, "k_pso_ring")
        S.set_cost_literal(True)
        want_lit = oracle_records(S, cands, is_seed)
        S.set_cost_literal(False)
        got, _ = run(P.LITERAL)
        for i, p in enumerate(want_lit):
            compare_patch(got[i], p, (r, "literal", i, "seed" if is_seed[i] else "child"))
    S.close()


@pytest.mark.gpu
@pytest.mark.parametrize("r", R)
def test_gpu_ncc_batch_every_radius(request, r):
    """pais_ncc_batch at radius r on view states of GPU refine records and of the evaluation states, with make_ncc_golden's
    perturbations: bit for bit G.oracle_ncc, tables within the table gate of refcost.  At K = 5 the warped patches sit in
    LDS up to r = 19 and in the global scratch slab from r = 20 on: both branches run."""
    from pais_mvs_amd.context import make_view_state
    from tests.test_ncc_batch import _compare
    ev = _evals(request, r)
    scene, cfg = ev["scene"], ev["cfg"]
    S = common.oracle_scene(cfg, scene)
    S.set_kernel_arithmetic(True)
    S.set_omp(True)
    ctx = P.context(cfg, scene.cameras)
    _, seeds = common.seed_candidates(S, scene)
    recs = [(list(x.center[:]), list(x.normal[:]), x.ref_cam, x.lod, x.cams(), x.cams())
            for x in ctx.refine_batch(seeds[:8]) if not x.dropped and x.num_cam >= 2]
    states = G.scene_states(S, scene, recs, np.random.default_rng(3000 + r), n_search=4) + _ncc_states(ev, S, np.random.default_rng(2000 + r))
    assert len(states) >= 8, (r, len(states))
    got = ctx.ncc_batch([make_view_state(st["center"], st["normal"], st["ref"], st["lod"], st["cams"]) for st in states], tables=True)
    for i, st in enumerate(states):
        _compare(got, i, G.oracle_ncc(S, st), (r, i, st["kind"]))
    mine = [{"dropped": int(got.dropped[i]), "table": got.tables[i].ravel().tolist()} for i in range(len(states))]
    n_tab, n_drop, skipped = _check_tables(r, cfg, scene, states, mine, "HIP")
    assert n_tab >= 4 and skipped <= 2, (r, n_tab, n_drop, skipped)
    kmax = max(len(st["cams"]) for st in states)
    in_lds = 8 * kmax * (2 * r + 1) ** 2 <= LDS_HP_LIMIT
    if r == 19:
        assert kmax == 5 and in_lds, kmax
    if r == 20:
        assert kmax == 5 and not in_lds, kmax
    ctx.close()
    S.close()
