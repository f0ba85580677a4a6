"""The number of visible cameras K swept through every cost, refine and NCC path, against the oracle AND against
tests/refcost.py (the plain float64 restatement), at r = 7 (S^2 = 225) with all three adaptive weights on.

The kernels change shape with K far more often than with the window radius:
  1, 2, 3       only the reference camera; one pair; one triple (pais_eval.hpp camera walk)
  6 / 7         two-pixel shape, LDS sub-accumulators -> register sub-accumulators (PAIS_TWO_PIXELS_MAXK)
  12 / 13       two-pixel -> one-pixel kernels; two-level colour sums start (PAIS_TWO_LEVEL_K); tile kernel eligible;
                the ring stops reading the set-up records (pre_ring_ok)
  13 .. 16      two_level_split(K, M) = 2 ((M + 4) / 4) moves the group boundary
  28 / 29       k_pso_tile2<8> -> <12>;   44 / 45: k_pso_tile2<12> -> <16>
  34 / 35       (r = 7) warped patches of pais_ncc_batch / the after-stage in LDS -> global scratch slab (8 K S^2 B against 60 KB)
  63 / 64       PAIS_MAX_VIS
The small scenes of conftest.py reach K <= 20, so the rig here is a spherical cap of 72 cameras 4 units above the top of the
dome object, polar angle <= 32 degrees, every one looking at the top point: points near the top are seen by all of them.
A state of K cameras is the reference camera and the K - 1 most frontal other visible cameras, in ascending camera index;
at a few K the reference camera is left out of the list (hasRef = 0) or a camera is listed twice.
"""
import math

import numpy as np
import pytest

from tests import common, pipelines as P, refcost
from tests.common import DBL_MAX, compare_patch, oracle_records
from tests.golden import make_ncc_golden as G
from tests.refcost import MARGIN, check_against_refcost
from tests.test_radius_sweep import RTOL_KERNEL, LDS_HP_LIMIT, _corner_particles, _det_normal

R = 7
S_WIN = 2 * R + 1
K_SWEEP = (1, 2, 3, 4, 5, 6, 7, 8, 11, 12, 13, 14, 15, 16, 27, 28, 29, 31, 32, 33, 34, 35, 43, 44, 45, 63, 64)
VARIANT_K = (12, 13, 33, 64)
REFINE_K = (0, 1, 2, 3, 6, 7, 12, 13, 14, 28, 29, 32, 33, 44, 45, 64)
TRACE_K = (2, 13, 33, 45, 64)
MAX_VIS = 64
TOP = np.array([0.0, 0.0, 0.95])        # the top point of the dome object (its upper ellipsoid: z = 0.55 + 0.4)
N_POINTS = 4                            # surface points per K


def cap_scene(n_cams=72, width=240, height=180, focal=400.0, dist=4.0, max_polar_deg=32.0, n_seeds=40, tex_seed=4567,
              seed_seed=8901):
    """n_cams cameras on a Fibonacci spherical cap of radius dist around the top point of synth.dome_scene's object (polar
    angle up to max_polar_deg), each looking at that point; the seeds keep every visible camera (_make_seeds max_vis 0)."""
    from pais_mvs_amd import synth
    from pais_mvs_amd.camera import Camera, quaternion_to_rotation, rotation_to_quaternion
    up = np.array([0.0, 0.0, 1.0])
    parts = [synth.Ellipsoid(-0.35, 0.75, 0.3), synth.Ellipsoid(0.0, 0.5, 0.7), synth.Ellipsoid(0.55, 0.4, 0.4)]
    rng = np.random.default_rng(tex_seed)
    px = dist / focal
    k, phi, amp = synth.make_texture(rng, 32, 7 * px, 40 * px, 34.0)
    obj = synth.SolidOfRevolution(np.zeros(3), up, parts, k, phi, amp)
    cams = []
    ga = math.pi * (3 - math.sqrt(5))
    c0 = math.cos(math.radians(max_polar_deg))
    for i in range(n_cams):
        zc = 1.0 - (1.0 - c0) * (i + 0.5) / n_cams
        rr = math.sqrt(1 - zc * zc)
        C = TOP + dist * np.array([rr * math.cos(ga * i), rr * math.sin(ga * i), zc])
        q = rotation_to_quaternion(synth._look_at(C, TOP.copy(), np.array([0.0, 1.0, 0.0])))
        f2 = np.array([focal, focal])
        pp = np.array([float(width >> 1), float(height >> 1)])
        img = synth.render(obj, quaternion_to_rotation(q), C, f2, pp, width, height)
        cams.append(Camera(focal=f2, principle_point=np.array([-1.0, -1.0]), quaternion=q, center=C, image=img,
                           name="cap%04d" % i).finalize(0.8, 15, True))
    seeds = synth._make_seeds(obj, cams, n_seeds, np.random.default_rng(seed_seed), max_vis=0)
    return synth.Scene("cap", cams, obj, seeds)


@pytest.fixture(scope="module")
def cap():
    return cap_scene()


def _cfg(**over):
    from pais_mvs_amd.config import readme_config
    kw = dict(patchRadius=R, distWeighting=R / 3.0, adaptiveDistanceEnable=True, adaptiveDifferenceEnable=True,
              adaptiveGradientEnable=True)
    kw.update(over)
    return readme_config(**kw)


def _frontal(scene, X, vis):
    """vis ordered from the most frontal camera (largest cosine to the surface normal at X) to the least."""
    from pais_mvs_amd import synth
    n = synth._surface_normal(scene.obj, X)
    cosv = [float((scene.cameras[c].center - X) @ n) / float(np.linalg.norm(scene.cameras[c].center - X)) for c in vis]
    return [vis[i] for i in sorted(range(len(vis)), key=lambda i: -cosv[i])]


def _points(scene, K, n=N_POINTS):
    """n surface points seen by at least K + 1 cameras -> [(X, cameras ordered most frontal first)]."""
    return [(X, _frontal(scene, X, vis)) for X, vis in scene.seeds if len(vis) >= K + 1][:n]


def _head(S, X, cams, key):
    """An oracle patch of the K cameras after refine()'s head (reference camera, depth and ray, depth range, level)."""
    import ctypes as C
    from oracle import po
    L = po.lib()
    p = S.seed_patch(X, cams, key=key)
    for f in (L.po_set_reference_camera, L.po_set_depth_and_ray, L.po_set_depth_range, L.po_set_lod):
        f(S.ptr, C.byref(p))
    return p


def _set_cams(p, cams):
    p.numCam = len(cams)
    for i, c in enumerate(cams):
        p.camIdx[i] = int(c)


def _patch_state(p):
    from pais_mvs_amd import _lib
    st = _lib.PatchState()
    st.ray[:] = p.ray[:]
    st.ref_cam, st.lod, st.num_cam = p.refCamIdx, p.LOD, p.numCam
    for k in range(p.numCam):
        st.cam_idx[k] = p.camIdx[k]
    return st


def _variants(p, order):
    """(kind, camera list) of the two extra states of a patch at K: no reference camera (its place taken by the next
    most frontal camera), and the last non-reference camera replaced by a second copy of the first one."""
    cams = p.cams()
    ref = p.refCamIdx
    nxt = next(c for c in order if c not in cams)
    out = [("no_ref", sorted([c for c in cams if c != ref] + [nxt]))]
    others = [c for c in cams if c != ref]
    if len(others) >= 2:
        dup = sorted(cams[:])
        dup.remove(others[-1])
        dup = sorted(dup + [others[0]])
        out.append(("twice", dup))
    return out


def _particles(p, rng, n_per):
    """The particles of tests/test_gpu_parity._states_and_particles: valid interior, near, random, back-facing, far off."""
    out = []
    th, ph, dp = p.normalS[0], p.normalS[1], p.depth
    for j in range(n_per):
        if j % 6 == 0:
            pos = [th, ph, dp]
        elif j % 6 == 1:
            pos = [th + rng.normal(0, 0.2), ph + rng.normal(0, 0.2), dp + rng.normal(0, 0.01)]
        elif j % 6 == 2:
            pos = [rng.uniform(0, math.pi), ph + rng.uniform(-1.5, 1.5), rng.uniform(p.depthRange[0], p.depthRange[1])]
        elif j % 6 == 3:
            pos = [math.pi - th, ph + math.pi, dp]
        elif j % 6 == 4:
            pos = [th, ph, dp * rng.uniform(0.05, 0.4)]
        else:
            pos = [th + rng.normal(0, 0.6), ph + rng.normal(0, 0.6), dp * rng.uniform(0.9, 1.1)]
        out.append(pos)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the evaluations of one K (shared by CPU and GPU tests)
# ---------------------------------------------------------------------------------------------------------------------
_EVALS = {}


def _evals(scene, K):
    if K in _EVALS:
        return _EVALS[K]
    cfg = _cfg()
    S = common.oracle_scene(cfg, scene)
    rng = np.random.default_rng(4000 + K)
    states, pats, kinds_st, idx, parts, kinds = [], [], [], [], [], []

    def add(p, kind, n_per):
        si = len(states)
        states.append(_patch_state(p))
        pats.append(p)
        kinds_st.append(kind)
        st = refcost.state_of(p)
        base = (p.normalS[0], p.normalS[1], p.depth)
        for pos in _particles(p, rng, n_per):
            idx.append(si); parts.append(pos); kinds.append(kind)
        for pos in _corner_particles(scene, cfg, st, base):
            idx.append(si); parts.append(list(pos)); kinds.append(kind + "_corner")

    for i, (X, order) in enumerate(_points(scene, K)):
        p = _head(S, X, sorted(order[:max(K, 3)]), key=100 * K + i)     # (the head drops fewer than minCamNum cameras)
        if p.drop:
            continue
        if K < 3:
            _set_cams(p, sorted([p.refCamIdx] + [c for c in order if c != p.refCamIdx][:K - 1]))
        add(p, "frontal", 18)
        if K in VARIANT_K and i < 2:
            for kind, cams in _variants(p, order):
                q = common.copy_struct(p)
                _set_cams(q, cams)
                add(q, kind, 12)
    ref, ref_det, lit, clit, ker = [], [], [], [], []
    for si, pos in zip(idx, parts):
        st = refcost.state_of(pats[si])
        ref.append(refcost.cost(scene, cfg, st, pos))
        ref_det.append(refcost.cost(scene, cfg, st, pos, normal_fn=_det_normal))
        S.set_kernel_arithmetic(False)
        S.set_cost_literal(False)
        lit.append(S.fitness(pats[si], pos))
        S.set_kernel_arithmetic(True)
        S.set_cost_literal(True)
        clit.append(S.fitness(pats[si], pos))
        S.set_cost_literal(False)
        ker.append(S.fitness(pats[si], pos))
    S.close()
    ev = dict(K=K, scene=scene, cfg=cfg, states=states, pats=pats, kinds_st=kinds_st, idx=idx, parts=parts, kinds=kinds,
              ref=ref, ref_det=ref_det, lit=lit, clit=clit, ker=ker)
    _EVALS[K] = ev
    return ev


def _check_counts(ev, counts, what):      # (refcost.check_counts with K in the messages)
    n_fin, n_max, skipped = counts
    assert n_fin >= 30 and n_max >= 5, (what, ev["K"], n_fin, n_max)
    assert skipped <= max(2, len(ev["parts"]) // 50), (what, ev["K"], skipped, len(ev["parts"]))


# ------------------------------------------------------------------------------------------------------------- CPU ---
def test_cap_rig_sees_a_point_from_64_cameras(cap):
    """The property the sweep relies on: surface points seen by at least 64 (here: all 72) cameras."""
    from pais_mvs_amd import synth
    assert len(cap.cameras) == 72
    assert len(synth._visible_cams(cap.obj, TOP, np.array([0.0, 0.0, 1.0]), cap.cameras)) == 72
    deep = [len(v) for _, v in cap.seeds if len(v) >= MAX_VIS]
    assert len(deep) >= N_POINTS, sorted(len(v) for _, v in cap.seeds)
    assert all(len(_points(cap, K)) == N_POINTS for K in K_SWEEP)


@pytest.mark.parametrize("K", K_SWEEP)
def test_oracle_cost_matches_refcost_every_k(cap, K):
    """The oracle's kernel arithmetic within 1e-9 of refcost (an independent check of its two-level split, PO_TWO_LEVEL_K),
    its literal cost and costLiteral within the literal gate; DBL_MAX exactly where refcost puts it.  Every state has K
    cameras; at K in VARIANT_K also states without the reference camera and with a camera listed twice."""
    ev = _evals(cap, K)
    assert all(st.num_cam == K for st in ev["states"]), [st.num_cam for st in ev["states"]]
    assert ev["kinds_st"].count("frontal") == N_POINTS, ev["kinds_st"]
    if K in VARIANT_K:
        assert {"no_ref", "twice"} <= set(ev["kinds_st"]), ev["kinds_st"]
        for p, kind in zip(ev["pats"], ev["kinds_st"]):
            assert (p.refCamIdx in p.cams()) == (kind != "no_ref")
            assert (len(set(p.cams())) < K) == (kind == "twice")
    gate = refcost.literal_gate(S_WIN)
    c1 = check_against_refcost(K, ev["ref"], ev["lit"], gate, "oracle literal")
    c2 = check_against_refcost(K, ev["ref_det"], ev["clit"], gate, "oracle costLiteral")
    c3 = check_against_refcost(K, ev["ref"], ev["ker"], RTOL_KERNEL, "oracle kernel arithmetic")
    for c, what in ((c1, "literal"), (c2, "costLiteral"), (c3, "kernel")):
        _check_counts(ev, c, what)
    if K in VARIANT_K:
        for kind in ("no_ref", "twice"):
            sel = [e for e, k in enumerate(ev["kinds"]) if k == kind]
            fin = [e for e in sel if ev["ref"][e].margin >= MARGIN and ev["ref"][e].value != DBL_MAX]
            assert len(fin) >= 4, (K, kind, len(fin))


def _view_states(ev, S, rng):
    """View states of one K: the heads of the evaluation states and make_ncc_golden's perturbations, subsets, searched tilts
    and edge states around them."""
    recs = [(list(p.center[:]), list(p.normal[:]), p.refCamIdx, p.LOD, p.cams(), p.cams())
            for p, kind in zip(ev["pats"], ev["kinds_st"]) if kind == "frontal"]
    return G.scene_states(S, ev["scene"], recs, rng, n_search=4)


def _check_tables(K, cfg, scene, states, wants, what):
    gate = refcost.table_gate(S_WIN)
    n_tab = n_drop = skipped = 0
    for i, (st, want) in enumerate(zip(states, wants)):
        t = refcost.ncc_table(scene, cfg, st)
        if t.margin < MARGIN:
            skipped += int(not st["kind"].startswith("edge_"))
            continue
        assert t.dropped == (want["dropped"] == G.DROP_SAMPLE), (what, K, i, st["kind"], t.dropped, want["dropped"])
        if t.dropped:
            n_drop += 1
            continue
        n_tab += 1
        k = len(st["cams"])
        got = np.asarray(want["table"], float).reshape(k, k)
        err = float(np.max(np.abs(got - t.table)))
        assert err <= gate, (what, K, i, st["kind"], err, gate)
    return n_tab, n_drop, skipped


@pytest.mark.parametrize("K", [k for k in K_SWEEP if k >= 2])
def test_oracle_ncc_table_matches_refcost_every_k(cap, K):
    """G.oracle_ncc's table (kernel and literal arithmetic) within 4 S^2 2^-53 of refcost.ncc_table at every K >= 2."""
    ev = _evals(cap, K)
    S = common.oracle_scene(ev["cfg"], cap)
    S.set_kernel_arithmetic(True)
    states = _view_states(ev, S, np.random.default_rng(5000 + K))
    assert any(len(st["cams"]) == K for st in states), K
    for kernel in (True, False):
        S.set_kernel_arithmetic(kernel)
        wants = [G.oracle_ncc(S, st) for st in states]
        n_tab, n_drop, skipped = _check_tables(K, ev["cfg"], cap, states, wants, "kernel" if kernel else "literal")
        assert n_tab >= 4 and skipped <= 2, (K, kernel, n_tab, n_drop, skipped)
    S.close()


# ------------------------------------------------------------------------------------------------------------- GPU ---
@pytest.mark.gpu
@pytest.mark.parametrize("K", K_SWEEP)
def test_gpu_cost_every_k(cap, K, monkeypatch):
    """Context.fitness_batch of the states of one K in a batch of their own: the default arithmetic equals the oracle's
    kernel arithmetic bit for bit and refcost within 1e-9; PAIS_ARITH=literal equals costLiteral bit for bit; byte taps
    (PAIS_TAP_FLOAT_MAX_MB=0) give the default's bytes."""
    ev = _evals(cap, K)
    cfg = ev["cfg"]
    got = P.fitness(monkeypatch, cfg, cap.cameras, ev["states"], ev["idx"], ev["parts"], {})
    for e, (g, want) in enumerate(zip(got, ev["ker"])):
        assert common.same_value(g, want, 0.0), ("default", K, e, ev["kinds"][e], g, want)
    _check_counts(ev, check_against_refcost(K, ev["ref"], got, RTOL_KERNEL, "HIP default"), "HIP default")
    lit = P.fitness(monkeypatch, cfg, cap.cameras, ev["states"], ev["idx"], ev["parts"], P.LITERAL)
    for e, (g, want) in enumerate(zip(lit, ev["clit"])):
        assert common.same_value(g, want, 0.0), ("literal", K, e, ev["kinds"][e], g, want)
    byte = P.fitness(monkeypatch, cfg, cap.cameras, ev["states"], ev["idx"], ev["parts"], P.BYTE_TAPS)
    assert byte.tobytes() == got.tobytes(), (K, np.flatnonzero(byte != got))


def _merged(evs):
    states, idx, parts, want = [], [], [], []
    for ev in evs:
        off = len(states)
        states += ev["states"]
        idx += [off + i for i in ev["idx"]]
        parts += ev["parts"]
        want.append(np.asarray(ev["ker"], dtype=np.float64))
    return states, idx, parts, np.concatenate(want)


@pytest.mark.gpu
@pytest.mark.parametrize("ks", [K_SWEEP, (3, 13)], ids=["every_k", "k3_k13"])
def test_gpu_cost_batch_independence(cap, ks, monkeypatch):
    """One batch holding the states of several K takes its shape from the largest K (the one-pixel, two-level kernels for
    every K in the batch): each evaluation gives the bytes of its own per-K batch -- the oracle's kernel arithmetic."""
    evs = [_evals(cap, K) for K in ks]
    states, idx, parts, want = _merged(evs)
    cfg = evs[0]["cfg"]
    for env in ({}, P.BYTE_TAPS):
        got = P.fitness(monkeypatch, cfg, cap.cameras, states, idx, parts, env)
        bad = np.flatnonzero(got.view(np.int64) != want.view(np.int64))
        assert len(bad) == 0, (env, [(states[idx[e]].num_cam, e, got[e], want[e]) for e in bad[:8]])
    lit = P.fitness(monkeypatch, cfg, cap.cameras, states, idx, parts, P.LITERAL)
    want_lit = np.concatenate([np.asarray(ev["clit"], dtype=np.float64) for ev in evs])
    assert lit.tobytes() == want_lit.tobytes(), np.flatnonzero(lit.view(np.int64) != want_lit.view(np.int64))[:8]


# ---------------------------------------------------------------------------------------------------------------------
# refine(): seeds and first-ring children of K cameras
# ---------------------------------------------------------------------------------------------------------------------
def _refine_cfg():
    return _cfg(particleNum=6, maxIteration=8, maxFitness=100.0)


def _refine_candidates(S, scene, K, n_points=3):
    """Seeds of K cameras (the reference camera and the most frontal others) at n_points surface points, and two children
    each: expansion candidates of the same cameras at centres moved off the surface point -> (candidates, is_seed)."""
    from pais_mvs_amd.context import make_candidate
    cands, is_seed = [], []
    for i, (X, order) in enumerate(_points(scene, max(K, 1), n_points)):
        key = 10000 * (K + 1) + 10 * i
        if K == 0:
            n = np.array([0.0, 0.0, 1.0])
            cands.append(make_candidate(X, n, [], key, 0))
            is_seed.append(True)
            cands.append(make_candidate(X, n, [], key + 1, 1))
            is_seed.append(False)
            continue
        p = S.seed_patch(X, sorted(order[:K]), key=key)
        cands.append(make_candidate(p.center[:], p.normal[:], p.cams(), key, 0, normalS=p.normalS[:]))
        is_seed.append(True)
        for j in range(2):
            cen = [p.center[0] + 0.004 * (j - 0.5), p.center[1] + 0.002 * j, p.center[2] - 0.001 * j]
            cands.append(make_candidate(cen, p.normal[:], p.cams(), key + 1 + j, 1, normalS=p.normalS[:]))
            is_seed.append(False)
    return cands, is_seed


_REFINE = {}


def _refine_case(scene, K):
    if K in _REFINE:
        return _REFINE[K]
    cfg = _refine_cfg()
    S = common.oracle_scene(cfg, scene)
    S.set_kernel_arithmetic(True)
    S.set_omp(True)
    cands, is_seed = _refine_candidates(S, scene, K)
    want = oracle_records(S, cands, is_seed)
    S.set_cost_literal(True)
    want_lit = oracle_records(S, cands, is_seed)
    S.close()
    _REFINE[K] = (cfg, cands, is_seed, want, want_lit)
    return _REFINE[K]


@pytest.mark.gpu
@pytest.mark.parametrize("K", REFINE_K)
def test_gpu_refine_pipelines_every_k(cap, K, monkeypatch, capfd):
    """refine() of seeds and children of K cameras (particleNum 6, maxIteration 8) through every evaluation pipeline: the
    default equals the oracle bit for bit; k_pso_eval2 + k_pso_step with and without the set-up records, the ring,
    k_pso_iter at 1, 2 and 4 parts and, from K = 13 on, the tile kernel (k_pso_tile2<8> / <12> / <16>, every particle verified
    through k_pso_eval2; at K = 64 also without any tile area) give the same record bytes; PAIS_ARITH=literal equals the
    oracle's costLiteral.  At K = 3, 7 and 13 (the three evaluation shapes) the eval2, iter, tile and literal runs are
    repeated with the nine candidates cut into three slices of three on three streams: same bytes."""
    cfg, cands, is_seed, want, want_lit = _refine_case(cap, K)
    assert all(c.num_cam == K for c in cands)
    ref, _ = P.refine(monkeypatch, cfg, cap.cameras, cands, {})
    alive = 0
    for i, p in enumerate(want):
        compare_patch(ref[i], p, (K, "default", i, "seed" if is_seed[i] else "child"))
        alive += 0 if p.drop else 1
    if K >= cfg.minCamNum:
        assert alive >= 3, (K, alive, len(want))
    runs = [(P.EVAL2, "eval2"), (dict(P.EVAL2, **P.NO_PRE), "eval2"), (P.RING, "ring")]
    runs += [({"PAIS_EVAL_PARTS": p}, "iter") for p in ("1", "2", "4")]
    if K >= 13:
        runs.append((P.TILE_VERIFIED, "tile"))
        if K == 64:
            runs.append((dict(P.TILE_VERIFIED, **P.NO_TILES), "tile"))
    sliced = P.SLICED
    if K in (3, 7, 13):
        # slices at candidates 3 and 6; each of them must hold a record that lives, or its offsets would go unseen
        assert len(ref) == 9 and all(any(not ref[i].dropped for i in range(lo, lo + 3)) for lo in (0, 3, 6)), K
        runs += [(dict(env, **sliced), kind) for env, kind in runs if kind in ("eval2", "iter", "tile")]
    live = K >= cfg.minCamNum     # (below minCamNum every candidate is dropped before its PSO)
    for env, kind in runs:
        got, ks = P.refine(monkeypatch, cfg, cap.cameras, cands, env)
        assert bytes(got) == bytes(ref), (K, env)
        if live and kind != "iter":
            P.assert_took(kind, ks, (K, env))
    assert "tile verify" not in capfd.readouterr().out
    got, _ = P.refine(monkeypatch, cfg, cap.cameras, cands, P.LITERAL)
    for i, p in enumerate(want_lit):
        compare_patch(got[i], p, (K, "literal", i, "seed" if is_seed[i] else "child"))
    if K in (3, 7, 13):
        cut, _ = P.refine(monkeypatch, cfg, cap.cameras, cands, dict(sliced, **P.LITERAL))
        assert bytes(cut) == bytes(got), (K, "literal", sliced)


@pytest.mark.gpu
def test_gpu_refine_mixed_k_batch(cap, monkeypatch):
    """Candidates of K = 3, 13 and 64 in one batch: each record has the bytes of its own per-K batch."""
    import ctypes as C
    cases = [_refine_case(cap, K) for K in (3, 13, 64)]
    cfg = cases[0][0]
    cands = [c for case in cases for c in case[1]]
    want = []
    for case in cases:
        recs, _ = P.refine(monkeypatch, cfg, cap.cameras, case[1], {})
        want += [C.string_at(C.addressof(recs[i]), C.sizeof(recs[i])) for i in range(len(case[1]))]
    got, _ = P.refine(monkeypatch, cfg, cap.cameras, cands, {})
    for i in range(len(cands)):
        assert C.string_at(C.addressof(got[i]), C.sizeof(got[i])) == want[i], (i, cands[i].num_cam)


@pytest.mark.gpu
def test_gpu_refine_seed_of_64_cameras_loses_cameras(cap, monkeypatch):
    """Seeds of the 64 most frontal cameras at every surface point seen by more than 64: where the after-stage removes
    cameras (an oblique point, whose far cameras drop), refine() runs another PSO pass; the records equal the oracle's, and
    the tile kernel gives the same bytes."""
    from pais_mvs_amd.context import make_candidate
    cfg = _refine_cfg()
    S = common.oracle_scene(cfg, cap)
    S.set_kernel_arithmetic(True)
    S.set_omp(True)
    cands = []
    for i, (X, order) in enumerate(_points(cap, MAX_VIS, 64)):
        p = S.seed_patch(X, sorted(order[:MAX_VIS]), key=90000 + i)
        cands.append(make_candidate(p.center[:], p.normal[:], p.cams(), 90000 + i, 0, normalS=p.normalS[:]))
    want = common.oracle_refine_many(S, cands, True, threads=16)
    S.close()
    lost = [i for i, p in enumerate(want) if not p.drop and p.numCam < MAX_VIS]
    assert lost and all(want[i].psoRuns >= 2 for i in lost), [(p.psoRuns, p.numCam, p.drop) for p in want]
    ref, _ = P.refine(monkeypatch, cfg, cap.cameras, cands, {})
    for i, p in enumerate(want):
        compare_patch(ref[i], p, (64, "seed", i))
    got, ks = P.refine(monkeypatch, cfg, cap.cameras, cands, P.TILE)
    assert bytes(got) == bytes(ref) and ks.tile_launches > 0


# ---------------------------------------------------------------------------------------------------------------------
# pais_ncc_batch and the after-stage
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("K", [k for k in K_SWEEP if k >= 2])
def test_gpu_ncc_batch_every_k(cap, K):
    """pais_ncc_batch on view states of K cameras (and make_ncc_golden's perturbations, subsets, tilts and edge states):
    bit for bit G.oracle_ncc, tables within the table gate of refcost.  At r = 7 the warped patches of a batch sit in LDS
    up to K = 34 and in the global scratch slab from K = 35 on: both sides run."""
    from pais_mvs_amd.context import make_view_state
    from tests.test_ncc_batch import _compare
    ev = _evals(cap, K)
    cfg = ev["cfg"]
    S = common.oracle_scene(cfg, cap)
    S.set_kernel_arithmetic(True)
    S.set_omp(True)
    states = _view_states(ev, S, np.random.default_rng(5000 + K))
    ctx = P.context(cfg, cap.cameras)
    got = ctx.ncc_batch([make_view_state(st["center"], st["normal"], st["ref"], st["lod"], st["cams"]) for st in states], tables=True)
    for i, st in enumerate(states):
        _compare(got, i, G.oracle_ncc(S, st), (K, i, st["kind"]))
    mine = [{"dropped": int(got.dropped[i]), "table": got.tables[i].ravel().tolist()} for i in range(len(states))]
    n_tab, n_drop, skipped = _check_tables(K, cfg, cap, states, mine, "HIP")
    assert n_tab >= 4 and skipped <= 2, (K, n_tab, n_drop, skipped)
    kmax = max(len(st["cams"]) for st in states)
    assert kmax == K, (K, kmax)
    in_lds = 8 * kmax * S_WIN ** 2 <= LDS_HP_LIMIT
    assert in_lds == (K <= 34), (K, kmax)
    ctx.close()
    S.close()


# ---------------------------------------------------------------------------------------------------------------------
# pais_fitness_detail and pais_pso_trace
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("K", TRACE_K)
def test_gpu_fitness_detail_every_k(cap, K, monkeypatch):
    """pais_fitness_detail of the states of one K: fitness equals PAIS_ARITH=literal bit for bit and the sums restate
    from the per-pixel maps; a few evaluations of every outcome restated pixel by pixel."""
    from tests.test_fitness_detail import _check_identity, _check_pixels, _ctx as detail_ctx
    ev = _evals(cap, K)
    cfg = ev["cfg"]
    ctx = detail_ctx(cfg, cap, monkeypatch)
    d = ctx.fitness_detail(ev["states"], ev["idx"], ev["parts"], colours=True, homographies=True)
    ctx.close()
    lit = P.fitness(monkeypatch, cfg, cap.cameras, ev["states"], ev["idx"], ev["parts"], P.LITERAL)
    _check_identity(d, lit, ("K", K))
    seen = {}
    for e in range(len(ev["parts"])):
        oc = int(d.outcome[e])
        if seen.get(oc, 0) >= 3 and ev["kinds"][e] == "frontal":
            continue
        seen[oc] = seen.get(oc, 0) + 1
        _check_pixels(d, e, cap, cfg, refcost.state_of(ev["pats"][ev["idx"][e]]), ev["parts"][e], ("K", K, e))
    assert len(seen) >= 2, seen


@pytest.mark.gpu
@pytest.mark.parametrize("literal", [False, True], ids=["kernel", "literal"])
@pytest.mark.parametrize("K", TRACE_K)
def test_gpu_pso_trace_every_k(cap, K, literal, monkeypatch):
    """pais_pso_trace of cap-rig seeds and children of K cameras: the records equal refine_batch, every run and row equals
    the oracle's trace bit for bit."""
    import ctypes as C
    from tests.test_pso_trace import _check_oracle_parity, _ctx as trace_ctx, _oracle_runs
    cfg, cands, is_seed, _, _ = _refine_case(cap, K)
    ctx = trace_ctx(cfg, cap, monkeypatch, literal)
    for flag in (True, False):
        sel = [c for c, s in zip(cands, is_seed) if s == flag]
        tr = ctx.pso_trace(sel, max_runs=8, particles=True)
        rec = ctx.refine_batch(sel)
        for i in range(len(sel)):
            assert C.string_at(C.addressof(tr.records[i]), C.sizeof(rec[i])) == C.string_at(C.addressof(rec[i]), C.sizeof(rec[i])), (K, i)
        bad = _check_oracle_parity(tr, _oracle_runs(cfg, cap, sel, flag, literal=literal), ("K", K))
        assert bad is None, "first mismatch (candidate, run, row, what): %r" % (bad,)
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# end to end at the cap
# ---------------------------------------------------------------------------------------------------------------------
def _e2e_cfg():
    return _cfg(particleNum=6, maxIteration=8)


@pytest.mark.gpu
def test_gpu_mvs_64_camera_rig_matches_the_oracle(monkeypatch):
    """MVS seeds and three expansion rounds on a cap of exactly 64 cameras, patch for patch against po_mvs_*; some patch
    keeps at least 45 cameras (the expansion children take every camera of their visibility cone)."""
    from oracle import po
    from pais_mvs_amd.mvs import MVS
    scene = cap_scene(n_cams=64, n_seeds=12)
    cfg = _e2e_cfg()
    S = common.oracle_scene(cfg, scene)
    S.set_kernel_arithmetic(True)
    S.set_omp(True)
    L = po.lib()
    mo = L.po_mvs_create(S.ptr)
    for X, vis in scene.seeds:
        L.po_mvs_add_seed(mo, po.darr(X), len(vis), po.iarr(vis))
    L.po_mvs_refine_seed_patches(mo)
    L.po_mvs_expansion_patches(mo, 8, 3, 1)
    want = []
    for i in range(L.po_mvs_num_slots(mo)):
        pp = L.po_mvs_get_patch(mo, i)
        if pp:
            p = pp.contents
            want.append((list(p.center[:]), list(p.normal[:]), p.cams(), p.fitness, p.correlation, p.priority, p.LOD))
    L.po_mvs_destroy(mo)
    S.close()
    with P.knobs(monkeypatch, {}):
        m = MVS(cfg, scene.cameras, device=0, seed=42)
    for X, vis in scene.seeds:
        m.add_seed(X, vis)
    m.refineSeedPatches()
    m.expansionPatches(8, 3)
    got = [(list(p.center[:]), list(p.normal[:]), p.cams(), p.fitness, p.correlation, p.priority, p.lod) for p in m.patches()]
    m.close()
    assert len(got) == len(want) and len(got) >= 8, (len(got), len(want))
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, (i, a, b)
    assert max(len(g[2]) for g in got) >= 45, sorted(len(g[2]) for g in got)[-8:]


@pytest.mark.gpu
def test_gpu_mvs_65_camera_rig_is_refused(monkeypatch):
    """On a cap of 65 cameras an expansion candidate's visibility cone holds more than PAIS_MAX_VIS cameras:
    expansionPatches raises (no crash, no silent truncation), the seeds' patches stay readable and the object closes."""
    from pais_mvs_amd.mvs import MVS
    scene = cap_scene(n_cams=65, n_seeds=12)
    with P.knobs(monkeypatch, {}):
        m = MVS(_e2e_cfg(), scene.cameras, device=0, seed=42)
    for X, vis in scene.seeds:
        m.add_seed(X, vis[:MAX_VIS])
    m.refineSeedPatches()
    n_seed = len(m.patches())
    assert n_seed >= 4, n_seed
    with pytest.raises(RuntimeError, match="more than PAIS_MAX_VIS cameras"):
        m.expansionPatches(8, 3)
    assert len(m.patches()) >= n_seed
    m.close()
