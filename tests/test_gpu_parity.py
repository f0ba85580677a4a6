"""GPU parity tests proper: the HIP path (through the C ABI) against the oracle.

Two oracle modes are used (oracle/pais_oracle.h, po_scene.detMath/treeSum):

* kernel arithmetic (fdlibm exp/sin/cos + wave64 butterfly sums) -- the arithmetic
  the HIP kernels define.  Here EVERYTHING must be identical: discrete outputs
  (dropped, visible-camera set, reference camera, LOD, PSO iteration counts) and
  every floating-point output bit for bit (RTOL_EXACT = 0).
* literal reference arithmetic (platform libm, sequential sums) -- the cost
  function must agree within 1e-9 relative.  Whole refine() runs are NOT compared
  in this mode on the GPU: the GLN-PSO is chaotic at the last bit (converged
  particles tie with their personal best within an ulp), see
  tests/test_oracle_modes.py for the CPU-side measurement and DESIGN.md 5.3.
  north_star's 1e-4 relative L2 on centres/normals is checked there.
"""
import ctypes as C
import math

import os

import numpy as np
import pytest

from tests import common, pipelines as P
from tests.common import DBL_MAX, RTOL_EXACT, compare_patch

pytestmark = pytest.mark.gpu

RTOL_FIT = 1e-9     # vs the literal-arithmetic oracle


def _states_and_particles(S, scene, rng, n_per=24):
    """Patch states taken from oracle patches after the refine() head, with particles that
    exercise the valid interior, the back-facing branch, window-out-of-image and tap overflow."""
    from oracle import po
    from pais_mvs_amd import _lib
    L = po.lib()
    states, pats, idx, parts = [], [], [], []
    for i, (X, vis) in enumerate(scene.seeds[:12]):
        p = S.seed_patch(X, vis, key=i)
        L.po_set_reference_camera(S.ptr, C.byref(p))
        L.po_set_depth_and_ray(S.ptr, C.byref(p))
        L.po_set_depth_range(S.ptr, C.byref(p))
        L.po_set_lod(S.ptr, C.byref(p))
        if p.drop:
            continue
        if i % 3 == 1:
            p.LOD = min(p.LOD + 2, 5)
        st = _lib.PatchState()
        st.ray[:] = p.ray[:]
        st.ref_cam = p.refCamIdx
        st.lod = p.LOD
        st.num_cam = p.numCam
        for k in range(p.numCam):
            st.cam_idx[k] = p.camIdx[k]
        si = len(states)
        states.append(st)
        pats.append(p)
        for j in range(n_per):
            th, ph, dp = p.normalS[0], p.normalS[1], p.depth
            if j % 6 == 0:
                pos = [th, ph, dp]
            elif j % 6 == 1:
                pos = [th + rng.normal(0, 0.2), ph + rng.normal(0, 0.2), dp + rng.normal(0, 0.01)]
            elif j % 6 == 2:
                pos = [rng.uniform(0, math.pi), ph + rng.uniform(-1.5, 1.5), rng.uniform(p.depthRange[0], p.depthRange[1])]
            elif j % 6 == 3:
                pos = [math.pi - th, ph + math.pi, dp]            # back-facing -> DBL_MAX
            elif j % 6 == 4:
                pos = [th, ph, dp * rng.uniform(0.05, 0.4)]       # far off -> out of image / overflow
            else:
                pos = [th + rng.normal(0, 0.6), ph + rng.normal(0, 0.6), dp * rng.uniform(0.9, 1.1)]
            idx.append(si)
            parts.append(pos)
    return states, pats, idx, parts


@pytest.mark.parametrize("weights", [(1, 1, 0), (1, 1, 1), (0, 0, 0), (0, 1, 1), (1, 0, 0)])
def test_fitness_batch_matches_oracle(pawn_small, weights):
    from pais_mvs_amd.config import readme_config
    cfg = readme_config(adaptiveDistanceEnable=bool(weights[0]), adaptiveDifferenceEnable=bool(weights[1]),
                        adaptiveGradientEnable=bool(weights[2]))
    S = common.oracle_scene(cfg, pawn_small)
    ctx = P.context(cfg, pawn_small.cameras)
    rng = np.random.default_rng(7)
    states, pats, idx, parts = _states_and_particles(S, pawn_small, rng)
    got = ctx.fitness_batch(states, idx, parts)
    n_max = n_fin = 0
    for e, (si, pos) in enumerate(zip(idx, parts)):
        S.set_kernel_arithmetic(False)
        want = S.fitness(pats[si], pos)
        S.set_kernel_arithmetic(True)
        want_k = S.fitness(pats[si], pos)
        if want == DBL_MAX:
            n_max += 1
            assert got[e] == DBL_MAX and want_k == DBL_MAX, (e, got[e])
        else:
            n_fin += 1
            assert common.same_value(got[e], want, RTOL_FIT), (e, got[e], want)
            assert common.same_value(got[e], want_k, RTOL_EXACT), (e, got[e], want_k, got[e] - want_k)
    assert n_max > 10 and n_fin > 50, (n_max, n_fin)
    ctx.close()


@pytest.mark.parametrize("scene_name", ["pawn_small", "ring_small", "dome_small"])
def test_literal_arithmetic_cost_is_the_reference_statement(request, scene_name, monkeypatch):
    """PAIS_ARITH=literal (pais_literal.hpp, round 6): the cost with the reference's per-pixel expressions (no fused
    multiply-adds, a true division per tap, the four-product bilinear of patch.cpp:1014-1017, mean /= K) and its x-outer /
    y-inner SEQUENTIAL sums (patch.cpp:979-1041), the window from the particle's own centre.  Checker: the oracle's literal
    statements of po_get_fitness with the deterministic exp / sin / cos (po_scene.costLiteral) -- bit for bit; against the
    all-literal oracle (platform libm) the values differ by the libm's last bits only (<= 1e-13 relative)."""
    from pais_mvs_amd.config import readme_config
    scene = request.getfixturevalue(scene_name)
    if scene_name == "dome_small":
        cfg = readme_config(patchRadius=25, distWeighting=25 / 3.0, reduceNormalRange=4.0, adaptiveGradientEnable=True)
    else:
        cfg = readme_config(adaptiveGradientEnable=(scene_name == "ring_small"))
    S = common.oracle_scene(cfg, scene)
    ctx = P.context(cfg, scene.cameras, monkeypatch, P.LITERAL)
    rng = np.random.default_rng(11)
    states, pats, idx, parts = _states_and_particles(S, scene, rng, n_per=12 if scene_name == "dome_small" else 24)
    got = ctx.fitness_batch(states, idx, parts)
    n_max = n_fin = 0
    worst = 0.0
    for e, (si, pos) in enumerate(zip(idx, parts)):
        S.set_kernel_arithmetic(False)
        S.set_cost_literal(False)
        lit = S.fitness(pats[si], pos)
        S.set_kernel_arithmetic(True)
        S.set_cost_literal(True)
        want = S.fitness(pats[si], pos)
        assert common.same_value(got[e], want, RTOL_EXACT), (e, got[e], want, got[e] - want)
        if want == DBL_MAX:
            n_max += 1
            assert lit == DBL_MAX
        elif want == want:
            n_fin += 1
            worst = max(worst, abs(got[e] - lit) / abs(lit))
    assert n_max > 5 and n_fin > 30, (n_max, n_fin)
    assert worst <= 1e-13, worst
    ctx.close()


def test_literal_arithmetic_refine_is_the_reference_order_run(pawn_small, monkeypatch):
    """Whole refine() runs under PAIS_ARITH=literal -- seeds and first-ring children of the 320x240 pawn scene -- ARE the
    oracle's runs with the literal cost (po_scene.costLiteral) bit for bit, and are held to north_star's gate against the
    all-literal oracle (platform libm, sequential sums everywhere) like the default arithmetic is: discrete outputs identical,
    centre / normal within 1e-12 on the literal run's trajectory, branched trajectories counted (printed; the default
    arithmetic branches 23 of these 211 candidates)."""
    from pais_mvs_amd.config import readme_config
    from pais_mvs_amd.context import make_candidate
    from tests.test_oracle_modes import refine_pairs, mode_statistics, assert_north_star_parity, PAWN_BRANCHED_CAP
    cfg = readme_config()
    S = common.oracle_scene(cfg, pawn_small)
    S.set_omp(True)
    ctx = P.context(cfg, pawn_small.cameras, monkeypatch, P.LITERAL)

    def gpu(seeds_in, child_in):
        cands = [make_candidate(cen, nrm, cams, key, 0, normalS=ns) for cen, nrm, ns, cams, key in seeds_in]
        for cen, nrm, cams, key in child_in:
            child = S.expand_patch(cen, nrm, cams, key)
            cands.append(make_candidate(child.center[:], child.normal[:], child.cams(), key, 1, normalS=child.normalS[:]))
        return list(ctx.refine_batch(cands))

    S.set_cost_literal(True)          # (only read in kernel arithmetic: refine_pairs' second run)
    lit, ker, got = refine_pairs(S, pawn_small, cfg, run_b=gpu)
    S.set_cost_literal(False)
    st = mode_statistics(lit, ker, hip=got)     # (asserts HIP == oracle with the literal cost, bit for bit)
    print("\nHIP path, PAIS_ARITH=literal, vs the all-literal oracle, pawn:", st)
    assert_north_star_parity(st, 150, PAWN_BRANCHED_CAP)
    ctx.close()


def test_refine_seeds_matches_oracle(pawn_small):
    from oracle import po
    from pais_mvs_amd import _lib
    from pais_mvs_amd.config import readme_config
    from pais_mvs_amd.context import make_candidate
    cfg = readme_config()
    S = common.oracle_scene(cfg, pawn_small)
    S.set_kernel_arithmetic(True)
    ctx = P.context(cfg, pawn_small.cameras)
    L = po.lib()
    pats, cands = [], []
    for i, (X, vis) in enumerate(pawn_small.seeds):
        p = S.seed_patch(X, vis, key=1000 + i)
        pats.append(p)
        cands.append(make_candidate(p.center[:], p.normal[:], p.cams(), 1000 + i, 0, normalS=p.normalS[:]))
    res = ctx.refine_batch(cands)
    alive = 0
    for i, p in enumerate(pats):
        L.po_refine_seed(S.ptr, C.byref(p))
        compare_patch(res[i], p, "seed %d" % i)
        alive += 0 if p.drop else 1
    assert alive >= len(pats) // 2
    ctx.close()


def _literal_gate(cfg, scene, n_min, cap, what):
    """Whole refine() runs of the HIP path -- seeds and first-ring children -- against the oracle's LITERAL arithmetic
    (platform libm, the reference's sequential sums, its own per-particle window) at north_star's gate, per candidate
    (tests/test_oracle_modes.py assert_north_star_parity): the HIP records are the kernel-arithmetic patches bit for bit;
    discrete outputs identical for every candidate; centre / normal within 1e-12 for every candidate on the literal
    run's PSO trajectory; branched trajectories counted against a hard cap."""
    from pais_mvs_amd.context import make_candidate
    from tests.test_oracle_modes import refine_pairs, mode_statistics, assert_north_star_parity
    S = common.oracle_scene(cfg, scene)
    S.set_omp(True)
    ctx = P.context(cfg, scene.cameras)

    def gpu(seeds_in, child_in):
        cands = [make_candidate(cen, nrm, cams, key, 0, normalS=ns) for cen, nrm, ns, cams, key in seeds_in]
        for cen, nrm, cams, key in child_in:
            child = S.expand_patch(cen, nrm, cams, key)          # the expansion constructor incl. expandVisibleCamera
            cands.append(make_candidate(child.center[:], child.normal[:], child.cams(), key, 1, normalS=child.normalS[:]))
        return list(ctx.refine_batch(cands))

    lit, ker, got = refine_pairs(S, scene, cfg, run_b=gpu)
    st = mode_statistics(lit, ker, hip=got)
    print("\nHIP path vs literal arithmetic, %s:" % what, st)
    assert_north_star_parity(st, n_min, cap)
    ctx.close()


def test_refine_against_literal_arithmetic_at_north_star_tolerance(pawn_small):
    """configs[1]'s scene at test size (320x240 pawn, README config): 211 candidates."""
    from pais_mvs_amd.config import readme_config
    from tests.test_oracle_modes import PAWN_BRANCHED_CAP
    _literal_gate(readme_config(), pawn_small, 150, PAWN_BRANCHED_CAP, "pawn")


def test_refine_against_literal_arithmetic_many_cameras(ring_small):
    """24-camera ring, all adaptive weights on (K = 7..11): 532 candidates."""
    from pais_mvs_amd.config import readme_config
    from tests.test_oracle_modes import RING_BRANCHED_CAP
    _literal_gate(readme_config(adaptiveGradientEnable=True), ring_small, 400, RING_BRANCHED_CAP, "ring")


def test_refine_against_literal_arithmetic_dome_radius25(dome_small):
    """configs[4]'s parameters at test size (40-camera dome, patchRadius 25, reduceNormalRange 4, all weights; K up to
    ~20, one-pixel kernels): 548 candidates."""
    from pais_mvs_amd.config import readme_config
    from tests.test_oracle_modes import DOME_BRANCHED_CAP
    cfg = readme_config(patchRadius=25, distWeighting=25 / 3.0, reduceNormalRange=4.0, adaptiveGradientEnable=True)
    _literal_gate(cfg, dome_small, 400, DOME_BRANCHED_CAP, "dome")


def test_low_texture_scene_runs_the_upper_pyramid_levels_end_to_end(pawn_lowtex):
    """R4 / F2 at LOD >= 1 without a hand-bumped level: seeds + expansion rounds of the low-texture pawn
    through the driver against the oracle, patch for patch and bit for bit; a sizeable share of the accepted patches sits on
    levels 1 and 2.  Then the literal gate on the same scene, reported by level."""
    from oracle import po
    from pais_mvs_amd.config import readme_config
    from pais_mvs_amd.mvs import MVS
    from tests.test_oracle_modes import refine_pairs, mode_statistics, LOWTEX_BRANCHED_CAP
    cfg = readme_config()
    rows, calls, acc, spec = common.oracle_reconstruct(cfg, pawn_lowtex, 16, 14, parallel=True)
    S = common.oracle_scene(cfg, pawn_lowtex)
    m = MVS(cfg, pawn_lowtex.cameras, device=0, seed=42)
    for X, vis in pawn_lowtex.seeds:
        m.add_seed(X, vis)
    m.refineSeedPatches()
    m.expansionPatches(16, 14)
    ps = m.patches()
    got = [(list(p.center[:]), list(p.normalS[:]), p.cams(), p.fitness, p.correlation) for p in ps]
    assert len(got) == len(rows) >= 40, (len(got), len(rows))
    for i, (a, b) in enumerate(zip(got, rows)):
        assert a == b, (i, a, b)
    lods = [p.lod for p in ps]
    upper = sum(1 for l in lods if l >= 1)
    print("\nlow-texture pawn: %d accepted, by LOD %s" % (len(lods), {l: lods.count(l) for l in sorted(set(lods))}))
    assert upper >= len(lods) // 5 and max(lods) >= 2, lods
    m.close()
    # literal gate, per candidate (seeds + first-ring children), HIP records == kernel arithmetic bit for bit
    ctx = P.context(cfg, pawn_lowtex.cameras)
    S.set_omp(True)

    def gpu(seeds_in, child_in):
        from pais_mvs_amd.context import make_candidate
        cands = [make_candidate(cen, nrm, cams, key, 0, normalS=ns) for cen, nrm, ns, cams, key in seeds_in]
        for cen, nrm, cams, key in child_in:
            child = S.expand_patch(cen, nrm, cams, key)
            cands.append(make_candidate(child.center[:], child.normal[:], child.cams(), key, 1, normalS=child.normalS[:]))
        return list(ctx.refine_batch(cands))

    lit, ker, hip = refine_pairs(S, pawn_lowtex, cfg, run_b=gpu)
    st = mode_statistics(lit, ker, hip=hip)
    by_lod = {}
    for a, b in zip(lit, ker):
        if a.drop or b.drop:
            continue
        t = by_lod.setdefault(int(a.LOD), [0, 0])
        t[0] += 1
        t[1] += int(not (a.psoSig == b.psoSig and a.psoRuns == b.psoRuns and a.psoIters == b.psoIters))
    print("low-texture pawn, HIP vs literal:", st, "by LOD (n, branched):", by_lod)
    assert st["set_mismatch"] == 0 and st["same_centre_max"] <= 1e-12 and st["same_normal_max"] <= 1e-12, st
    assert sum(v[0] for k, v in by_lod.items() if k >= 1) >= 30, by_lod
    assert st["branched"] <= LOWTEX_BRANCHED_CAP, st
    ctx.close()


def test_expand_candidates_match_oracle(pawn_small):
    """Children of refined seeds: MVS::expandCell (mvs.cpp:566-577) per candidate."""
    from oracle import po
    from pais_mvs_amd.config import readme_config
    from pais_mvs_amd.context import make_candidate
    cfg = readme_config()
    S = common.oracle_scene(cfg, pawn_small)
    S.set_kernel_arithmetic(True)
    ctx = P.context(cfg, pawn_small.cameras)
    L = po.lib()
    cands, want = [], []
    for i, (X, vis) in enumerate(pawn_small.seeds[:10]):
        par = S.seed_patch(X, vis, key=i)
        L.po_refine_seed(S.ptr, C.byref(par))
        if par.drop:
            continue
        for j, camI in enumerate(par.cams()[:3]):
            cx = int(par.imgPoint[j][0] / cfg.cellSize) + (1 if j % 2 == 0 else 0)
            cy = int(par.imgPoint[j][1] / cfg.cellSize) + (0 if j % 2 == 0 else -1)
            cen = (C.c_double * 3)()
            L.po_expansion_center(S.ptr, camI, C.byref(par), cx, cy, cen)
            key = L.po_child_key(par.key, camI, cx, cy)
            child = S.expand_patch(cen[:], par.normal[:], par.cams(), key)   # constructor incl. expandVisibleCamera
            cands.append(make_candidate(child.center[:], child.normal[:], child.cams(), key, 1, normalS=child.normalS[:]))
            full = po.Patch()
            L.po_expand_candidate(S.ptr, C.byref(full), cen, po.darr(par.normal[:]), par.numCam, po.iarr(par.cams()), key)
            want.append(full)
    assert len(cands) >= 10
    res = ctx.refine_batch(cands)
    ok = 0
    for i, p in enumerate(want):
        compare_patch(res[i], p, "child %d" % i)
        ok += 0 if p.drop else 1
    assert ok >= 5
    ctx.close()


@pytest.mark.parametrize("B,max_rounds,strategy", [(1, 40, 0), (16, 20, 0), (8, 10, 1), (8, 10, 2), (8, 10, 3), (1, 30, 3)])
def test_reconstruction_rounds_match_oracle(pawn_small, B, max_rounds, strategy):
    """End to end through the driver (include/pais_mvs.h): seeds + expansion rounds on the GPU
    against the oracle's R(B) loop (B = 1: the reference's own order).  The accepted clouds must
    be identical patch by patch (same order, same camera sets, same bits)."""
    from oracle import po
    from pais_mvs_amd.config import readme_config
    from pais_mvs_amd.mvs import MVS
    cfg = readme_config(expansionStrategy=strategy)   # 0 best-first ... 3 depth-first (mvs.cpp:632-788)
    S = common.oracle_scene(cfg, pawn_small)
    S.set_kernel_arithmetic(True)
    L = po.lib()
    mo = L.po_mvs_create(S.ptr)
    for X, vis in pawn_small.seeds:
        L.po_mvs_add_seed(mo, po.darr(X), len(vis), po.iarr(vis))
    L.po_mvs_refine_seed_patches(mo)
    L.po_mvs_expansion_patches(mo, B, max_rounds, 1)
    want = []
    for i in range(L.po_mvs_num_slots(mo)):
        pp = L.po_mvs_get_patch(mo, i)
        if pp:
            p = pp.contents
            want.append((list(p.center[:]), list(p.normal[:]), p.cams(), p.fitness, p.correlation, p.priority, p.LOD))
    calls = L.po_mvs_refine_calls(mo)
    L.po_mvs_destroy(mo)

    m = MVS(cfg, pawn_small.cameras, device=0, seed=42)
    for X, vis in pawn_small.seeds:
        m.add_seed(X, vis)
    m.refineSeedPatches()
    m.expansionPatches(B, max_rounds)
    got = [(list(p.center[:]), list(p.normal[:]), p.cams(), p.fitness, p.correlation, p.priority, p.lod) for p in m.patches()]
    st = m.stats()
    assert len(got) == len(want) and len(got) >= len(pawn_small.seeds) // 2, (len(got), len(want))
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, (i, a, b)
    assert st.seeds_refined + st.candidates_effective == calls
    m.close()


def test_full_size_properties(pawn_full):
    """BASELINE-size run (640x480 pawn, README config, full expansion): size-independent properties."""
    from pais_mvs_amd.config import readme_config
    from pais_mvs_amd.mvs import MVS
    cfg = readme_config()
    clouds = []
    for rep in range(2):
        m = MVS(cfg, pawn_full.cameras, device=0, seed=42)
        for X, vis in pawn_full.seeds:
            m.add_seed(X, vis)
        m.refineSeedPatches()
        m.expansionPatches(256, 0)
        ps = m.patches()
        st = m.stats()
        clouds.append(m.cloud())
        assert len(ps) > 10 * len(pawn_full.seeds)                 # the surface was actually grown
        for p in ps[:: max(1, len(ps) // 500)]:
            assert not p.dropped and p.num_cam >= cfg.minCamNum
            assert 0 < p.fitness <= cfg.maxFitness and p.correlation >= cfg.minCorrelation
            assert len(set(p.cams())) == p.num_cam
            n = np.array(p.normal[:]); assert abs(np.linalg.norm(n) - 1) < 1e-12
        # every accepted patch lies on the synthetic surface (ray-cast check from its reference camera)
        obj = pawn_full.obj
        errs = []
        for p in ps[:: max(1, len(ps) // 300)]:
            cam = pawn_full.cameras[p.ref_cam]
            d = np.array(p.center[:]) - cam.center
            dist = np.linalg.norm(d)
            t = obj.intersect(cam.center, (d / dist)[None, :])[0]
            errs.append(abs(t - dist) / dist)
        assert np.median(errs) < 2e-3, np.median(errs)
        assert st.candidates_refined >= st.candidates_effective > 0
        m.close()
    # bit-reproducible run to run
    assert clouds[0].shape == clouds[1].shape and np.array_equal(clouds[0], clouds[1])


def test_ring_all_weights_many_cameras(ring_small):
    """Config-2-like rig (ring of cameras, all three adaptive weights on, K = 7..11): cost, seed refinement
    and expansion rounds against the oracle, bit for bit."""
    from oracle import po
    from pais_mvs_amd.config import readme_config
    from pais_mvs_amd.mvs import MVS
    cfg = readme_config(adaptiveGradientEnable=True, particleNum=8, maxIteration=12)
    S = common.oracle_scene(cfg, ring_small)
    S.set_kernel_arithmetic(True)
    L = po.lib()
    # cost
    ctx = P.context(cfg, ring_small.cameras)
    rng = np.random.default_rng(3)
    states, pats, idx, parts = _states_and_particles(S, ring_small, rng, n_per=12)
    assert max(p.numCam for p in pats) >= 7
    got = ctx.fitness_batch(states, idx, parts)
    nfin = 0
    for e, (si, pos) in enumerate(zip(idx, parts)):
        want = S.fitness(pats[si], pos)
        assert common.same_value(got[e], want, RTOL_EXACT), (e, got[e], want)
        nfin += int(want != DBL_MAX)
    assert nfin > 30
    ctx.close()
    # reconstruction rounds
    S.set_omp(True)
    mo = L.po_mvs_create(S.ptr)
    for X, vis in ring_small.seeds:
        L.po_mvs_add_seed(mo, po.darr(X), len(vis), po.iarr(vis))
    L.po_mvs_refine_seed_patches(mo)
    L.po_mvs_expansion_patches(mo, 8, 6, 1)
    want = []
    for i in range(L.po_mvs_num_slots(mo)):
        pp = L.po_mvs_get_patch(mo, i)
        if pp:
            p = pp.contents
            want.append((list(p.center[:]), list(p.normal[:]), p.cams(), p.fitness, p.correlation, p.priority, p.LOD))
    L.po_mvs_destroy(mo)
    m = MVS(cfg, ring_small.cameras, device=0, seed=42)
    for X, vis in ring_small.seeds:
        m.add_seed(X, vis)
    m.refineSeedPatches()
    m.expansionPatches(8, 6)
    got = [(list(p.center[:]), list(p.normal[:]), p.cams(), p.fitness, p.correlation, p.priority, p.lod) for p in m.patches()]
    assert len(got) == len(want) and len(got) > len(ring_small.seeds) // 2, (len(got), len(want))
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, (i, a, b)
    m.close()


_DIST_SCRIPT = """
import os, sys, hashlib
sys.path.insert(0, %r)
from pais_mvs_amd import synth, distributed as D
from pais_mvs_amd.config import readme_config
from pais_mvs_amd.mvs import MVS
job = D.job_from_env(force_group=True)
if os.environ.get("PAIS_TEST_SCENE") == "ring":     # BASELINE configs[3] in small: ring of cameras, all adaptive weights
    scene = synth.ring_scene(n_cams=24, width=480, height=360, focal=450.0, radius=3.0, n_seeds=30)
    cfg = readme_config(adaptiveGradientEnable=True, particleNum=8, maxIteration=12)
else:
    scene = synth.pawn_scene(width=320, height=240, n_seeds=24)
    cfg = readme_config()
m = MVS(cfg, scene.cameras, device=0, seed=42)
mode = os.environ["PAIS_TEST_MODE"]
if mode != "direct":
    D.attach(m, job, transport=mode)
    m.set_replicate_below(int(os.environ.get("PAIS_TEST_REPLICATE", "0")))
for X, vis in scene.seeds: m.add_seed(X, vis)
D.reconstruct(m, 16, max_rounds=8)
st = m.stats()
print("CLOUD", job.rank, hashlib.sha1(m.cloud().tobytes()).hexdigest(), m.num_patches(), st.batches_sharded, st.batches_replicated, flush=True)
m.close(); job.close()
"""


def _run_dist(tmp_path, mode, world, replicate=0, port=29541, scene="pawn"):
    import subprocess, sys, os
    script = tmp_path / "dist_job.py"
    script.write_text(_DIST_SCRIPT % os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   PAIS_TEST_MODE=mode, PAIS_TEST_REPLICATE=str(replicate), PAIS_NO_BUILD="1", PAIS_TEST_SCENE=scene)
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = []
    for p in procs:
        o, e = p.communicate(timeout=900)
        assert p.returncode == 0, o[-2000:] + e[-3000:]
        outs.append([l.split() for l in o.splitlines() if l.startswith("CLOUD")][0])
    return outs


def test_multi_rank_paths_under_the_c_abi_on_one_gpu(tmp_path):
    """SURVEY 8e on a one-GPU box: (a) the RCCL transport (ncclCommInitRank + one ncclAllGather per batch under the C ABI)
    with a world of one rank and every batch forced through the sharded path; (b) two ranks sharing the GPU with the
    host-memory transport (RCCL refuses two ranks on one device), sharding every batch / replicating thin ones.
    All must produce the cloud of the plain single-process driver, byte for byte."""
    direct = _run_dist(tmp_path, "direct", 1, port=29541)[0]
    assert int(direct[3]) > 24
    rccl1 = _run_dist(tmp_path, "rccl", 1, replicate=0, port=29542)[0]
    assert rccl1[2] == direct[2] and int(rccl1[4]) > 0 and int(rccl1[5]) == 0, (direct, rccl1)
    for rep in (0, 600):          # evaluation waves per iteration: 600 = 40 expansion candidates at 15 particles
        two = _run_dist(tmp_path, "host", 2, replicate=rep, port=29543 + (1 if rep else 0))
        for o in two:
            assert o[2] == direct[2], (rep, direct, o)
            assert int(o[4]) > 0 and (rep == 0 or int(o[5]) > 0), o


def test_ring_sharded_over_two_ranks_equals_one_rank(tmp_path):
    """BASELINE configs[3] (ring of cameras, candidates of a round sharded over the ranks, one all-gather per round) at
    test size: 24 cameras 480x360, K = 7..11, all adaptive weights; two ranks share the one GPU of the box through the
    host transport and every batch is sharded.  The cloud must be the single-process cloud byte for byte."""
    direct = _run_dist(tmp_path, "direct", 1, port=29551, scene="ring")[0]
    assert int(direct[3]) > 30
    for o in _run_dist(tmp_path, "host", 2, replicate=0, port=29552, scene="ring"):
        assert o[2] == direct[2] and int(o[4]) > 0 and int(o[5]) == 0, (direct, o)


def test_bench_refuses_a_rank_count_it_cannot_run():
    """`bench.py --gpus 2` on a box with one GPU must fail loudly instead of reporting n_gpus 1 (or 2)."""
    import subprocess, sys, os, torch
    if torch.cuda.device_count() >= 2:
        pytest.skip("needs a one-GPU box")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "PAIS_FORCE_DEVICE")}
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode != 0 and "n_gpus" not in r.stdout and "GPU" in (r.stderr + r.stdout)
    # a launcher that starts the wrong number of ranks is refused too
    env2 = dict(env, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29577")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       capture_output=True, text=True, timeout=600, env=env2)
    assert r.returncode != 0 and "n_gpus" not in r.stdout


@pytest.mark.parametrize("tile", ["tile kernel, cameras split over two waves", "tile kernel, cameras split over two waves, strips of 4 steps, one-row last strip",
                                  "one wave per evaluation"])
def test_dome_radius25_many_cameras(dome_small, monkeypatch, capfd, tile):
    """Config-4-like parameters: patchRadius 25 (S^2 = 2601), reduceNormalRange 4, all weights, many visible
    cameras per patch.  Cost + seeds + a few expansion rounds against the oracle, bit for bit -- through the LDS-tile
    kernel of many-camera batches (pais_tile2.hpp: footprints staged in LDS, colours in registers, a particle's cameras shared
    by two waves; forced for every batch incl. the seeds' 2N particles; also with strips of 4 steps: the last strip is then
    step 40 alone, a single window row, whose footprint may be one image column wide) and through the
    one-wave-per-evaluation kernels."""
    from oracle import po
    if tile.startswith("tile"):
        # (by default only scenes too large for the float tap copy take it); every particle ALSO through k_pso_eval2: a mismatch
        # is printed (and fails below)
        env = dict(P.TILE_VERIFIED, **({"PAIS_TILE_STRIP_SPLIT": "4"} if "strips of 4 steps" in tile else {}))
    else:
        env = P.NO_TILE
    from pais_mvs_amd.config import readme_config
    from pais_mvs_amd.mvs import MVS
    cfg = readme_config(patchRadius=25, distWeighting=25 / 3.0, reduceNormalRange=4.0, adaptiveGradientEnable=True,
                        particleNum=6, maxIteration=8, visibleCorrelation=0.6)
    S = common.oracle_scene(cfg, dome_small)
    S.set_kernel_arithmetic(True)
    S.set_omp(True)
    L = po.lib()
    ctx = P.context(cfg, dome_small.cameras, monkeypatch, env)
    rng = np.random.default_rng(9)
    states, pats, idx, parts = _states_and_particles(S, dome_small, rng, n_per=6)
    kmax = max(p.numCam for p in pats)
    assert kmax >= 12, kmax
    got = ctx.fitness_batch(states, idx, parts)
    nfin = 0
    for e, (si, pos) in enumerate(zip(idx, parts)):
        want = S.fitness(pats[si], pos)
        assert common.same_value(got[e], want, RTOL_EXACT), (e, got[e], want)
        nfin += int(want != DBL_MAX)
    assert nfin > 10
    ctx.close()
    mo = L.po_mvs_create(S.ptr)
    for X, vis in dome_small.seeds:
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
    from pais_mvs_amd import _lib
    with P.knobs(monkeypatch, env):     # (to m.close(): a lane forked during the rounds reads the context-level knobs again)
        m = MVS(cfg, dome_small.cameras, device=0, seed=42)
        for X, vis in dome_small.seeds:
            m.add_seed(X, vis)
        m.refineSeedPatches()
        m.expansionPatches(8, 3)
        got = [(list(p.center[:]), list(p.normal[:]), p.cams(), p.fitness, p.correlation, p.priority, p.lod) for p in m.patches()]
        ks = _lib.KernelStats()
        m.L.pais_get_kernel_stats(m.ctx_handle, C.byref(ks), 0)   # (PAIS_TILE_VERIFY: reports the particles whose two values differ)
        m.close()
    assert len(got) == len(want) and len(got) >= 8, (len(got), len(want))
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, (i, a, b)
    assert "tile verify" not in capfd.readouterr().out


def test_edge_cases(pawn_small):
    """Empty batch, too few cameras (patch.cpp:118-123), a seed whose window leaves every image (whole-call
    DBL_MAX, drop by maxFitness), bad arguments."""
    from oracle import po
    from pais_mvs_amd import _lib
    from pais_mvs_amd.config import readme_config
    from pais_mvs_amd.context import make_candidate
    cfg = readme_config()
    S = common.oracle_scene(cfg, pawn_small)
    S.set_kernel_arithmetic(True)
    L = po.lib()
    ctx = P.context(cfg, pawn_small.cameras)
    assert len(ctx.refine_batch([])) == 0
    assert len(ctx.fitness_batch([], [], np.zeros((0, 3)))) == 0
    X, vis = pawn_small.seeds[0]
    cases = []
    p = S.seed_patch(X, vis[:2], key=7)                       # 2 < minCamNum cameras
    cases.append((p, make_candidate(p.center[:], [0, 0, 1], vis[:2], 7, 0, normalS=[0.0, 0.0])))
    far = np.array(X) + np.array([5.0, 5.0, 5.0])             # projects outside every image
    p = S.seed_patch(far, vis, key=8)
    cases.append((p, make_candidate(p.center[:], p.normal[:], p.cams(), 8, 0, normalS=p.normalS[:])))
    p = S.expand_patch(X, [0.0, 0.0, 1.0], vis, key=9)       # normal facing away from most cameras
    cases.append((p, make_candidate(p.center[:], p.normal[:], p.cams(), 9, 1, normalS=p.normalS[:])))
    res = ctx.refine_batch([c for _, c in cases])
    for i, (p, _) in enumerate(cases):
        if p.type == 0:
            L.po_refine_seed(S.ptr, C.byref(p))
        else:
            if p.numCam < cfg.minCamNum:
                p.drop = 1
            L.po_refine(S.ptr, C.byref(p)); L.po_remove_invisible_camera(S.ptr, C.byref(p))
        assert bool(res[i].dropped) == bool(p.drop), (i, res[i].dropped, p.drop)
        if not p.drop:
            assert list(res[i].center[:]) == list(p.center[:])
    assert res[0].dropped and res[1].dropped
    # argument validation: errors, not crashes
    bad = make_candidate(X, [0, 0, 1], [0, 1, 99], 1, 1)
    with pytest.raises(RuntimeError):
        ctx.refine_batch([bad])
    st = _lib.PatchState(); st.ref_cam = 0; st.lod = 0; st.num_cam = 0
    with pytest.raises(RuntimeError):
        ctx.fitness_batch([st], [0], [[0.0, 0.0, 1.0]])
    ctx.close()


@pytest.mark.gpu
def test_file_level_verbs_reconstruct_then_filter(tmp_path, pawn_small):
    """`-r` then `-f` from files (TMVS.cpp:76-172): NVM2 + PNG images in, seed/exp .mvs/.ply/.psr out, then the filter
    chain on exp.mvs.  The cloud written must be the cloud the in-memory driver produces from the same inputs."""
    from PIL import Image
    from pais_mvs_amd import io, reconstruct
    from pais_mvs_amd.config import readme_config
    from pais_mvs_amd.mvs import MVS
    d = tmp_path
    lines = ["NVM_V3", "", str(len(pawn_small.cameras))]
    for i, cam in enumerate(pawn_small.cameras):
        name = "cam%d.png" % i
        Image.fromarray(np.repeat(cam.pyramid[0][:, :, None], 3, axis=2)).save(str(d / name))
        lines.append("%s %r %r %r %r %s %s" % (name, float(cam.focal[0]), float(cam.focal[1]), float(cam.principle_point[0]),
                                               float(cam.principle_point[1]), " ".join(repr(float(v)) for v in cam.quaternion),
                                               " ".join(repr(float(v)) for v in cam.center)))
    lines += ["", str(len(pawn_small.seeds))]
    seeds_meas = []
    for X, vis in pawn_small.seeds:
        ms = []
        for c in vis:
            cam = pawn_small.cameras[c]
            q = cam.rotation @ np.asarray(X, float) + cam.translation
            u, v = cam.focal[0] * q[0] / q[2] + cam.principle_point[0], cam.focal[1] * q[1] / q[2] + cam.principle_point[1]
            ms.append((c, u - cam.width // 2, v - cam.height // 2))
        seeds_meas.append(ms)
        meas = " ".join("%d 0 %r %r" % (c, float(du), float(dv)) for c, du, dv in ms)
        lines.append("%r %r %r 128 128 128 %d %s" % (float(X[0]) + 0.01, float(X[1]) - 0.01, float(X[2]) + 0.02, len(vis), meas))
    lines += ["", "0"]
    (d / "scene.nvm2").write_text("\n".join(lines) + "\n")
    (d / "config.txt").write_text("particleNum 6\nmaxIteration 8\n")
    reconstruct.main([str(d / "scene.nvm2"), "--config", str(d / "config.txt"), "--out", str(d)])
    for f in ("seed.mvs", "exp.mvs", "exp.ply", "exp.psr"):
        assert (d / f).stat().st_size > 0
    cfg_file, cams_io, pats = io.load_mvs(str(d / "exp.mvs"))
    assert len(cams_io) == len(pawn_small.cameras) and len(pats) > len(pawn_small.seeds)
    # the same inputs through the in-memory driver
    cfg = io.load_config(str(d / "config.txt"), reconstruct.default_config())
    cams = reconstruct.load_cameras(io.load_nvm(str(d / "scene.nvm2"), nvm2=True)[0], str(d), cfg)
    m = MVS(cfg, cams, device=0)
    for (X, vis), ms in zip(pawn_small.seeds, seeds_meas):
        pid = m.add_seed_measured([X[0] + 0.01, X[1] - 0.01, X[2] + 0.02], vis,
                                  [[du + cams[c].width // 2, dv + cams[c].height // 2] for c, du, dv in ms], recenter=True)
        assert np.linalg.norm(np.array(m.get_patch(pid).center[:]) - np.asarray(X, float)) < 1e-9   # re-triangulated
    m.refineSeedPatches()
    m.expansionPatches(4096, 0)
    mine = m.patches()
    assert len(mine) == len(pats)
    for a, b in zip(mine, pats):
        assert list(a.center[:]) == list(b.center[:]) and list(a.normalS[:]) == list(b.normalS[:]) and a.fitness == b.fitness
    m.close()
    # `-f`
    reconstruct.main([str(d / "exp.mvs"), "--filter", "--config", str(d / "config.txt"), "--out", str(d)])
    n_prev = len(pats)
    for f in ("PMVS_filter1.mvs", "PMVS_filter2.mvs", "PMVS_filter3.mvs", "PCMVS_filter.mvs"):
        n = len(io.load_mvs(str(d / f))[2])
        assert 0 < n <= n_prev
        n_prev = n


@pytest.mark.gpu
def test_pyramid_construction_on_gpu_is_the_oracle_statement():
    """N2 (mvs/camera.cpp:45-136): INTER_AREA resize chain from level 0 (:85), Sobel(ksize 1) magnitude (:72-73, 87-88),
    min-max normalisation -- the HIP kernels (pais_pyramid.hip) against the ORACLE's C statement (oracle/po_io.c:
    po_resize_area, po_sobel_magnitude_normalised), array for array, odd sizes included.  The distance to the oracle's
    second statement, po_resize_area_f32 (OpenCV 2.4's float accumulator order as far as its source documents it), is
    reported as numbers: pixels that differ and the largest grey-level difference -- the OpenCV-float gap is unpinned
    here (no OpenCV in the image), so it is bounded, not hidden."""
    import ctypes as C
    from oracle import po
    from pais_mvs_amd.camera import build_pyramid_gpu, max_lod
    L = po.lib()
    u8 = C.POINTER(C.c_uint8)
    L.po_resize_area.argtypes = [u8, C.c_int, C.c_int, C.c_double, u8]
    L.po_resize_area_f32.argtypes = [u8, C.c_int, C.c_int, C.c_double, u8]
    L.po_resize_dims.argtypes = [C.c_int, C.c_int, C.c_double, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.po_sobel_magnitude_normalised.argtypes = [u8, C.c_int, C.c_int, C.POINTER(C.c_double)]
    L.po_camera_max_lod.restype = C.c_int
    rng = np.random.default_rng(3)
    moved = total = 0
    worst = 0
    for (h, w) in ((480, 640), (271, 353), (1080, 1920)):
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.ascontiguousarray((127 + 80 * np.sin(xx / 7.3) * np.cos(yy / 5.1) + rng.normal(0, 20, (h, w))).clip(0, 255).astype(np.uint8))
        levels, edges, ms = build_pyramid_gpu(img, 0.8, 15, True, device=0)
        assert len(levels) == L.po_camera_max_lod(w, h, 0.8, 15) + 1 == max_lod(w, h, 0.8, 15) + 1
        assert len(edges) == len(levels) and ms > 0
        assert np.array_equal(levels[0], img)
        for i in range(len(levels)):
            if i > 0:
                fx = 0.8 ** i
                dw, dh = C.c_int(), C.c_int()
                L.po_resize_dims(w, h, fx, C.byref(dw), C.byref(dh))
                want = np.zeros((dh.value, dw.value), np.uint8)
                L.po_resize_area(img.ctypes.data_as(u8), w, h, fx, want.ctypes.data_as(u8))
                assert levels[i].shape == want.shape and np.array_equal(levels[i], want), (h, w, i)
                f32 = np.zeros_like(want)
                L.po_resize_area_f32(img.ctypes.data_as(u8), w, h, fx, f32.ctypes.data_as(u8))
                d = np.abs(f32.astype(int) - levels[i].astype(int))
                moved += int((d > 0).sum()); total += d.size; worst = max(worst, int(d.max()))
            lv = np.ascontiguousarray(levels[i])
            e = np.zeros(lv.shape, np.float64)
            L.po_sobel_magnitude_normalised(lv.ctypes.data_as(u8), lv.shape[1], lv.shape[0], e.ctypes.data_as(C.POINTER(C.c_double)))
            assert np.array_equal(edges[i], e), (h, w, i)
    print("\nHIP pyramid vs po_resize_area_f32 (OpenCV-float accumulator order): %d of %d pixels differ (%.3f %%), "
          "largest grey-level difference %d" % (moved, total, 100.0 * moved / total, worst))
    assert worst <= 1 and moved <= 0.02 * total, (moved, total, worst)


@pytest.mark.gpu
def test_pipeline_shapes_are_bit_identical(pawn_small, monkeypatch):
    """the two per-iteration pipelines (k_pso_iter for small batches, k_pso_eval2 + k_pso_step for
    large ones) and every waves-per-evaluation setting of k_pso_iter produce the same records bit for bit."""
    from pais_mvs_amd.config import readme_config
    cfg = readme_config()
    S = common.oracle_scene(cfg, pawn_small)
    _, cands = common.seed_candidates(S, pawn_small)
    cands = cands[:24]

    def run(env):
        res, _ = P.refine(monkeypatch, cfg, pawn_small.cameras, cands, env)
        return [(r.dropped, r.pso_runs, r.pso_iterations, r.pso_evals, r.fitness, list(r.center[:]), list(r.normal[:]), r.cams())
                for r in res]

    ref = run({})
    assert any(not r[0] for r in ref)
    assert run(P.SPLIT) == ref, "split"
    for parts in ("1", "2", "4"):
        assert run({"PAIS_EVAL_PARTS": parts}) == ref, parts
    # what the taps read is a property of the uploaded scene (float2 copy for small pyramids, the byte blob for large
    # ones: pais_internal.h PaisImgT); the sampled values are the same
    assert run(P.BYTE_TAPS) == ref, "byte taps"
    assert run(dict(P.BYTE_TAPS, **P.SPLIT)) == ref, "byte taps, split"


@pytest.mark.gpu
@pytest.mark.parametrize("scene_name", ["pawn_small", "ring_small"])
def test_byte_taps_cost_is_the_float_copy_cost(request, scene_name, monkeypatch):
    """The BYTES instantiations of the evaluation kernels (two-pixel and one-pixel shapes) against the oracle, bit for bit."""
    from pais_mvs_amd.config import readme_config
    scene = request.getfixturevalue(scene_name)
    cfg = readme_config(adaptiveGradientEnable=True)
    S = common.oracle_scene(cfg, scene)
    ctx = P.context(cfg, scene.cameras, monkeypatch, P.BYTE_TAPS)
    rng = np.random.default_rng(11)
    states, pats, idx, parts = _states_and_particles(S, scene, rng)
    got = ctx.fitness_batch(states, idx, parts)
    S.set_kernel_arithmetic(True)
    n_fin = 0
    for e, (si, pos) in enumerate(zip(idx, parts)):
        want = S.fitness(pats[si], pos)
        assert common.same_value(got[e], want, RTOL_EXACT), (e, got[e], want)
        n_fin += want != DBL_MAX
    assert n_fin > 50
    ctx.close()


@pytest.mark.gpu
def test_edge_cases_of_the_widened_entry_points(pawn_small):
    from pais_mvs_amd.camera import build_pyramid_gpu, resize_area, max_lod
    from pais_mvs_amd.config import readme_config
    from pais_mvs_amd.mvs import MVS
    # pyramid of a tiny image: levels down to 1 x 1, and invalid ratios are refused
    img = (np.arange(9 * 7, dtype=np.uint8) * 3).reshape(7, 9)
    levels, edges, _ = build_pyramid_gpu(img, 0.8, 15, True, device=0)
    assert len(levels) == max_lod(9, 7, 0.8, 15) + 1
    for i in range(1, len(levels)):
        assert np.array_equal(levels[i], resize_area(img, 0.8 ** i))
    with pytest.raises(RuntimeError):
        build_pyramid_gpu(img, 1.5, 15, False, device=0)
    # neighbour counts: n = 0 and n = 1
    m = MVS(readme_config(), pawn_small.cameras, device=0)
    cnt = np.zeros(1, dtype=np.int32)
    one = np.zeros(3, dtype=np.float64)
    assert m.L.pais_neighbor_count(m.ctx_handle, 0, None, C.c_double(1.0), None, None) == 0
    assert m.L.pais_neighbor_count(m.ctx_handle, 1, one.ctypes.data_as(C.POINTER(C.c_double)), C.c_double(1.0),
                                   cnt.ctypes.data_as(C.POINTER(C.c_int32)), None) == 0 and cnt[0] == 0
    # the PCMVS filter on an empty driver is a no-op
    assert m.neighborPatchFiltering(0.25) == 0.0
    m.close()


@pytest.mark.gpu
def test_large_swarms_and_the_split_pipeline_match_oracle(pawn_small, monkeypatch):
    """Swarms above 64 particles cannot sit in the lanes of one wave (k_pso_iter) and take the k_pso_eval2 + k_pso_step
    pipeline, as large batches do; force that pipeline on a small batch too.  Both must equal the oracle bit for bit."""
    from oracle import po
    from pais_mvs_amd.config import readme_config
    from pais_mvs_amd.context import make_candidate
    L = po.lib()
    for particles, env in ((40, {}), (8, P.SPLIT)):      # seeds run 2 x particleNum: 80 particles > 64; then a forced split
        cfg = readme_config(particleNum=particles, maxIteration=6)
        S = common.oracle_scene(cfg, pawn_small)
        S.set_kernel_arithmetic(True)
        ctx = P.context(cfg, pawn_small.cameras, monkeypatch, env)
        pats, cands = [], []
        for i, (X, vis) in enumerate(pawn_small.seeds[:10]):
            p = S.seed_patch(X, vis, key=7000 + i)
            pats.append(p)
            cands.append(make_candidate(p.center[:], p.normal[:], p.cams(), 7000 + i, 0, normalS=p.normalS[:]))
        res = ctx.refine_batch(cands)
        alive = 0
        for i, p in enumerate(pats):
            L.po_refine_seed(S.ptr, C.byref(p))
            compare_patch(res[i], p, "particles %d seed %d" % (particles, i))
            alive += 0 if p.drop else 1
        assert alive >= 3
        ctx.close()


@pytest.mark.gpu
def test_edges_on_the_fly_equal_the_given_edge_maps(ring_small):
    """level_edge == NULL with adaptiveGradientEnable: the library evaluates Camera::pyramidEdge from the gray levels
    itself (Sobel ksize 1, magnitude, per-level min-max; camera.cpp:72-77,87-91) instead of keeping an 8-byte-per-pixel
    copy in HBM.  Cost values and whole refine() records must equal those computed from the caller's edge
    pyramids bit for bit -- and so, transitively, the oracle, which reads those pyramids."""
    import copy
    from pais_mvs_amd.config import readme_config
    from pais_mvs_amd.context import Context
    cfg = readme_config(adaptiveGradientEnable=True, particleNum=8, maxIteration=12)
    S = common.oracle_scene(cfg, ring_small)
    rng = np.random.default_rng(3)
    states, pats, idx, parts = _states_and_particles(S, ring_small, rng, n_per=12)
    _, cands = common.seed_candidates(S, ring_small)
    bare = []
    for cam in ring_small.cameras:
        c2 = copy.copy(cam)
        c2.edge_pyramid = []
        bare.append(c2)
    out = []
    for cams in (ring_small.cameras, bare):
        ctx = Context(cfg, cams, device=0, seed=42)
        fit = ctx.fitness_batch(states, idx, parts)
        res = ctx.refine_batch(cands[:16])
        out.append((fit.tobytes(), [bytes(r) for r in res]))
        ctx.close()
    assert np.isfinite(np.frombuffer(out[0][0])).sum() > 30
    assert out[0][0] == out[1][0]
    assert out[0][1] == out[1][1]


def _surface_error(scene, patches, every):
    obj = scene.obj
    errs = []
    for p in patches[::every]:
        cam = scene.cameras[p.ref_cam]
        d = np.array(p.center[:]) - cam.center
        dist = np.linalg.norm(d)
        t = obj.intersect(cam.center, (d / dist)[None, :])[0]
        errs.append(abs(t - dist) / dist)
    return float(np.median(errs))


@pytest.mark.gpu
def test_ring_full_size_properties_and_determinism():
    """BASELINE.json configs[2] at FULL size: 32 cameras 1920x1080 on a ring, patchRadius 15, all three adaptive weights
    on (edge maps on the fly), rounds of 4096 parents, a bounded number of rounds.  Size-independent properties: every
    accepted patch satisfies the acceptance rules of runtimeFiltering, lies on the synthetic surface, the surface is
    actually grown, and the cloud is bit-reproducible run to run."""
    import torch
    from pais_mvs_amd import synth
    from pais_mvs_amd.config import readme_config
    from pais_mvs_amd.mvs import MVS
    scene = synth.ring_scene(n_seeds=300, build_edges=False, device=0)
    assert len(scene.cameras) == 32 and scene.cameras[0].image.shape == (1080, 1920)
    cfg = readme_config(adaptiveGradientEnable=True)
    clouds = []
    for rep in range(2):
        m = MVS(cfg, scene.cameras, device=0, seed=42)
        for X, vis in scene.seeds:
            m.add_seed(X, vis)
        m.refineSeedPatches()
        n_seed = m.num_patches()
        m.expansionPatches(4096, 5)
        ps = m.patches()
        st = m.stats()
        clouds.append(m.cloud())
        assert n_seed > len(scene.seeds) // 2 and len(ps) > 8 * n_seed, (n_seed, len(ps))
        ks = [p.num_cam for p in ps]
        assert max(ks) >= 7 and min(ks) >= cfg.minCamNum
        for p in ps[:: max(1, len(ps) // 500)]:
            assert not p.dropped and 0 < p.fitness <= cfg.maxFitness and p.correlation >= cfg.minCorrelation
            assert len(set(p.cams())) == p.num_cam and p.ref_cam in p.cams()
            assert abs(np.linalg.norm(np.array(p.normal[:])) - 1) < 1e-12
        assert _surface_error(scene, ps, max(1, len(ps) // 300)) < 2e-3
        assert st.candidates_refined >= st.candidates_effective > 0
        m.close()
    assert clouds[0].shape == clouds[1].shape and np.array_equal(clouds[0], clouds[1])


@pytest.mark.gpu
def test_ring_full_size_rounds_match_oracle():
    """BASELINE.json configs[2] at FULL size (32 cameras 1920x1080, patchRadius 15, all adaptive weights), seeds + the first
    expansion rounds of R(4096): the HIP path's cloud against the oracle's on the same box (kernel arithmetic, candidates
    evaluated ahead of the sequential replay on the host cores) -- every accepted patch, in order, same bits, same cameras
    (mvs/mvs.cpp:196-275).  The scene is rendered and pyramided on the GPU; the oracle gets the edge maps it reads from the
    host statement of camera.cpp:72-77 over the same levels."""
    from pais_mvs_amd import synth
    from pais_mvs_amd.camera import sobel_magnitude_normalised
    from pais_mvs_amd.config import readme_config
    from pais_mvs_amd.mvs import MVS, patches_sha1
    scene = synth.ring_scene(n_seeds=300, build_edges=False, device=0)
    cfg = readme_config(adaptiveGradientEnable=True)
    B, rounds = 4096, 2
    m = MVS(cfg, scene.cameras, device=0, seed=42)
    for X, vis in scene.seeds:
        m.add_seed(X, vis)
    m.refineSeedPatches()
    m.expansionPatches(B, rounds)
    st = m.stats()
    got = [(list(p.center[:]), list(p.normalS[:]), p.cams(), p.fitness, p.correlation) for p in m.patches()]
    m.close()
    for cam in scene.cameras:
        cam.edge_pyramid = [sobel_magnitude_normalised(l) for l in cam.pyramid]
    want, calls, accepted, spec = common.oracle_reconstruct(cfg, scene, B, rounds, parallel=True)
    assert st.seeds_refined + st.candidates_effective == calls and len(got) == accepted and accepted > 1000, (calls, accepted)
    assert st.candidates_refined - st.candidates_effective == spec
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, (i, a, b)
    assert patches_sha1(got) == patches_sha1(want)


@pytest.mark.gpu
def test_dome_full_size_bounded_rounds(monkeypatch):
    """BASELINE.json configs[4] on ONE GPU at FULL size: 128 cameras 4096x3072 on a Fibonacci dome, patchRadius 25
    (S^2 = 2601), reduceNormalRange 4, all adaptive weights on.  The renders and pyramids are produced on the GPU (hours in
    numpy), the edge maps are never materialised; seeds + a bounded number of expansion rounds; properties as above and the
    HBM footprint is reported (~4.5 GB of gray pyramids, which the taps read directly at this size)."""
    import torch
    from pais_mvs_amd import synth
    from pais_mvs_amd.config import readme_config
    from pais_mvs_amd.mvs import MVS
    free0, total = torch.cuda.mem_get_info(0)
    scene = synth.dome_scene(n_seeds=160, build_edges=False, device=0)
    assert len(scene.cameras) == 128 and scene.cameras[0].image.shape == (3072, 4096)
    cfg = readme_config(patchRadius=25, distWeighting=25 / 3.0, reduceNormalRange=4.0, adaptiveGradientEnable=True)
    torch.cuda.empty_cache()
    free1, _ = torch.cuda.mem_get_info(0)
    m = MVS(cfg, scene.cameras, device=0, seed=42)
    free2, _ = torch.cuda.mem_get_info(0)
    scene_gb = (free1 - free2) / 2 ** 30
    for X, vis in scene.seeds:
        m.add_seed(X, vis)
    m.refineSeedPatches()
    n_seed = m.num_patches()
    m.expansionPatches(1024, 2)
    free3, _ = torch.cuda.mem_get_info(0)
    ps = m.patches()
    st = m.stats()
    print("\ndome 128 x 4096 x 3072: scene in HBM %.1f GB, peak working set %.1f GB of %.0f GB; %d seeds kept, %d patches after 2 rounds, "
          "K max %d, %d candidates refined" % (scene_gb, (free1 - free3) / 2 ** 30, total / 2 ** 30, n_seed, len(ps), max(p.num_cam for p in ps),
                                              st.candidates_refined))
    assert 3.0 < scene_gb < 8.0              # no float2 tap copy (36 GB) at this size: the BYTES kernels run
    assert n_seed >= len(scene.seeds) // 3 and len(ps) > 2 * n_seed
    assert max(p.num_cam for p in ps) >= 12
    for p in ps[:: max(1, len(ps) // 300)]:
        assert not p.dropped and 0 < p.fitness <= cfg.maxFitness and p.correlation >= cfg.minCorrelation
        assert len(set(p.cams())) == p.num_cam and p.ref_cam in p.cams()
    assert _surface_error(scene, ps, max(1, len(ps) // 200)) < 2e-3
    sha_tile = m.cloud_sha1()
    got = [(list(p.center[:]), list(p.normalS[:]), p.cams(), p.fitness, p.correlation) for p in ps]
    m.close()
    # ... against the ORACLE on this box's host cores, every accepted patch in order, same bits, same camera sets (round 4:
    # before, the K > 32 instantiation of the tile kernel was only compared with the one-wave kernels).  The oracle reads edge
    # maps (camera.cpp:72-77): built here by its own C statement over the same levels, a level per thread.
    import ctypes as C
    from concurrent.futures import ThreadPoolExecutor
    from oracle import po
    from pais_mvs_amd.mvs import patches_sha1
    L = po.lib()
    L.po_sobel_magnitude_normalised.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.po_sobel_magnitude_normalised.restype = None

    def edge(level):
        out = np.empty(level.shape, dtype=np.float64)
        L.po_sobel_magnitude_normalised(level.ctypes.data, level.shape[1], level.shape[0], out.ctypes.data)
        return out
    with ThreadPoolExecutor(max_workers=min(128, os.cpu_count() or 8)) as ex:
        jobs = [[ex.submit(edge, np.ascontiguousarray(l, dtype=np.uint8)) for l in cam.pyramid] for cam in scene.cameras]
        for cam, js in zip(scene.cameras, jobs):
            cam.edge_pyramid = [j.result() for j in js]
    want, calls, accepted, spec = common.oracle_reconstruct(cfg, scene, 1024, 2, parallel=True)
    for cam in scene.cameras:
        cam.edge_pyramid = []          # (the library below evaluates them on the fly again)
    assert st.seeds_refined + st.candidates_effective == calls and len(got) == accepted, (calls, accepted, len(got))
    assert st.candidates_refined - st.candidates_effective == spec
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, (i, a, b)
    assert sha_tile == patches_sha1(want)
    # the same reconstruction through the one-wave-per-evaluation kernels: the LDS-tile kernel (pais_tile2.hpp; K up to 44 here)
    # must not change a bit of the cloud
    with P.knobs(monkeypatch, P.NO_TILE):   # (to m.close(): the lane of a streamed round is forked during expansionPatches)
        m = MVS(cfg, scene.cameras, device=0, seed=42)
        for X, vis in scene.seeds:
            m.add_seed(X, vis)
        m.refineSeedPatches()
        m.expansionPatches(1024, 2)
        sha = m.cloud_sha1()
        m.close()
    assert sha == sha_tile


@pytest.mark.gpu
def test_scene_half_of_runtime_filtering_on_the_device(pawn_small, monkeypatch):
    """include/pais_hip.h PAIS_DONE_*: the camera loop of MVS::runtimeFiltering (mvs.cpp:851-863) is evaluated by the batch
    call, one lane per camera; the drivers then run only the cell-map half on the host.  Same cloud as with the host
    evaluating everything, and every flag of a seed batch equals a numpy statement of the loop."""
    from pais_mvs_amd.config import readme_config
    from pais_mvs_amd.context import Context
    from pais_mvs_amd.mvs import MVS
    cfg = readme_config()

    def cloud():
        m = MVS(cfg, pawn_small.cameras, device=0, seed=42)
        for X, vis in pawn_small.seeds:
            m.add_seed(X, vis)
        m.refineSeedPatches()
        m.expansionPatches(64, 12)
        out = m.cloud().tobytes(), m.stats().candidates_effective
        m.close()
        return out

    with P.knobs(monkeypatch, {}):
        ref = cloud()
    with P.knobs(monkeypatch, {"PAIS_HOST_SCENE_TEST": "1"}):
        assert cloud() == ref

    S = common.oracle_scene(cfg, pawn_small)
    _, cands = common.seed_candidates(S, pawn_small)
    ctx = Context(cfg, pawn_small.cameras, device=0, seed=42)
    res = ctx.refine_batch(cands)
    seen = set()
    for r in res:
        if r.dropped:
            assert r.stage == 0
            continue
        ok = True
        for cam in pawn_small.cameras:
            q = cam.rotation @ np.array(r.center[:]) + cam.translation
            x = cam.focal[0] * q[0] / q[2] + cam.principle_point[0]
            y = cam.focal[1] * q[1] / q[2] + cam.principle_point[1]
            h, w = cam.image.shape
            if not (0 <= x < w and 0 <= y < h):
                ok = False
                break
            rx, ry = min(int(np.rint(x)), w - 1), min(int(np.rint(y)), h - 1)
            if cam.image[ry, rx] == 0:
                ok = False
                break
        assert r.stage == (5 if ok else 6), (r.stage, ok)
        seen.add(r.stage)
    assert 5 in seen
    ctx.close()


@pytest.mark.gpu
def test_wire_slots_packed_on_the_device_are_the_host_statement(pawn_small):
    """include/pais_hip.h "wire format of a record": k_pack_records (what a rank sends in the per-round exchange) against the
    host statement pais_pack_records on real records of a seed batch, and pack -> unpack reproduces those records byte for
    byte (the batch calls write no array element beyond a candidate's own camera count)."""
    import torch
    from pais_mvs_amd import _lib
    from pais_mvs_amd.config import readme_config
    from pais_mvs_amd.context import Context
    cfg = readme_config(particleNum=6, maxIteration=8)
    S = common.oracle_scene(cfg, pawn_small)
    _, cands = common.seed_candidates(S, pawn_small)
    ctx = Context(cfg, pawn_small.cameras, device=0, seed=42)
    res = ctx.refine_batch(cands)
    n = len(res)
    L = ctx.L
    L.pais_record_wire_bytes.restype = C.c_size_t
    L.pais_record_wire_bytes.argtypes = [C.c_int]
    L.pais_pack_records.argtypes = [C.c_int, C.POINTER(_lib.PatchResult), C.c_int, C.c_void_p]
    L.pais_unpack_records.argtypes = [C.c_int, C.c_void_p, C.c_int, C.POINTER(_lib.PatchResult)]
    L.pais_pack_records_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    K = max(c.num_cam for c in cands)
    wb = L.pais_record_wire_bytes(K)
    recs = (_lib.PatchResult * n)(*res)
    host = (C.c_uint8 * (wb * n))()
    assert L.pais_pack_records(n, recs, K, host) == 0
    raw = np.frombuffer(recs, dtype=np.uint8).copy()
    d_recs = torch.from_numpy(raw).cuda()
    d_wire = torch.zeros(wb * n, dtype=torch.uint8, device="cuda")
    assert L.pais_pack_records_device(ctx.h, n, C.c_void_p(d_recs.data_ptr()), K, C.c_void_p(d_wire.data_ptr())) == 0
    assert L.pais_ctx_synchronize(ctx.h) == 0
    assert bytes(d_wire.cpu().numpy().tobytes()) == bytes(host)
    back = (_lib.PatchResult * n)()
    assert L.pais_unpack_records(n, host, K, back) == 0
    assert bytes(back) == raw.tobytes()
    ctx.close()



@pytest.mark.gpu
def test_streamed_rounds_are_the_same_reconstruction(pawn_small, monkeypatch):
    """A streamed round (pais_mvs.hip: the first part of the work list is refined on the context while the host enumerates
    the rest for the lane context, and is committed while the lane still refines) is the same round: the cloud of a streamed
    reconstruction equals the oracle's patch for patch, and equals the unstreamed one's hash."""
    from pais_mvs_amd.config import readme_config
    from pais_mvs_amd.mvs import MVS, patches_sha1
    cfg = readme_config(particleNum=8, maxIteration=12)
    rows, calls, acc, _ = common.oracle_reconstruct(cfg, pawn_small, 4096, 14)
    shas = {}
    streamed = {"PAIS_STREAM_ROUNDS": "2", "PAIS_STREAM_ABOVE": "8", "PAIS_STREAM_SPLIT": "0.4"}
    # (the second run keeps the first one's threshold and split, as it always has)
    for mode, env in (("streamed", streamed), ("one batch per round", dict(streamed, PAIS_STREAM_ROUNDS="0"))):
        with P.knobs(monkeypatch, env):
            m = MVS(cfg, pawn_small.cameras, device=0, seed=42)
            for X, vis in pawn_small.seeds:
                m.add_seed(X, vis)
            m.refineSeedPatches()
            m.expansionPatches(4096, 14)
            st = m.stats()
            got = [(list(p.center[:]), list(p.normalS[:]), p.cams(), p.fitness, p.correlation) for p in m.patches()]
            sha = m.cloud_sha1()
            m.close()
        assert st.seeds_refined + st.candidates_effective == calls and len(got) == acc, (mode, st.candidates_effective, calls)
        for i, (a, b) in enumerate(zip(got, rows)):
            assert a == b, (mode, i, a, b)
        assert (st.rounds_streamed > 0) == (mode == "streamed"), (mode, st.rounds_streamed, st.rounds)
        shas[mode] = sha
    assert shas["streamed"] == shas["one batch per round"] == patches_sha1(rows)


@pytest.mark.gpu
def test_two_lanes_refine_concurrently_like_one(pawn_small):
    """pais_refine_batch_begin / _end and pais_ctx_fork_lane (include/pais_hip.h): two batches open at once, one on the
    context and one on its lane, give the records of pais_refine_batch byte for byte; the lane's launches are counted in the
    parent's kernel statistics; a second _begin on a context with an open batch is refused."""
    from pais_mvs_amd import _lib
    from pais_mvs_amd.config import readme_config
    from pais_mvs_amd.context import Context
    from oracle import po
    cfg = readme_config(particleNum=6, maxIteration=8)
    S = common.oracle_scene(cfg, pawn_small)
    S.set_kernel_arithmetic(True)
    parents, seeds = common.seed_candidates(S, pawn_small)
    ctx = Context(cfg, pawn_small.cameras, device=0, seed=42)
    kept = [r for r in ctx.refine_batch(seeds) if not r.dropped]
    assert len(kept) >= 8
    # expansion candidates around the refined seeds (pure expansion batches are the asynchronous ones)
    from pais_mvs_amd.context import make_candidate
    cands = []
    for i, r in enumerate(kept):
        for j in range(3):
            cen = [r.center[0] + 0.002 * (j - 1), r.center[1] + 0.001 * j, r.center[2]]
            cands.append(make_candidate(cen, list(r.normal[:]), [r.cam_idx[k] for k in range(r.num_cam)], 1000 + 7 * i + j, 1,
                                        normalS=list(r.normalS[:])))
    n = len(cands)
    want = ctx.refine_batch(cands)
    L = ctx.L
    ctx.kernel_stats(reset=True)
    lane = C.c_void_p()
    assert L.pais_ctx_fork_lane(ctx.h, C.byref(lane)) == 0
    n0 = n // 3
    a0 = (_lib.Candidate * n0)(*cands[:n0])
    a1 = (_lib.Candidate * (n - n0))(*cands[n0:])
    assert L.pais_refine_batch_open(ctx.h, n0, a0, 2) == 0         # the first two PSO iterations of its launch chain
    assert L.pais_refine_batch_begin(lane, n - n0, a1) == 0       # a whole chain
    assert L.pais_refine_batch_begin(ctx.h, n0, a0) != 0          # one open batch per context
    assert L.pais_refine_batch_enqueue(ctx.h, 3) == 0             # three more: iterations remain
    assert L.pais_refine_batch_enqueue(lane, 1) == 1              # (nothing left to enqueue there)
    v0, v1 = C.POINTER(_lib.PatchResult)(), C.POINTER(_lib.PatchResult)()
    assert L.pais_refine_batch_end(lane, C.byref(v1)) == 0
    assert L.pais_refine_batch_end(ctx.h, C.byref(v0)) == 0
    assert L.pais_refine_batch_end(ctx.h, C.byref(v0)) != 0       # nothing open any more
    sz = C.sizeof(_lib.PatchResult)
    got = C.string_at(v0, sz * n0) + C.string_at(v1, sz * (n - n0))
    assert got == bytes(want)
    ks = ctx.kernel_stats()
    assert ks.pso_patches == sum(r.pso_runs for r in want) > 0, (ks.pso_patches, n)   # both lanes' runs, counted by the parent
    ctx.close()
    S.close()


@pytest.mark.gpu
@pytest.mark.parametrize("scene_name", ["pawn_small", "ring_small"])
def test_task_ring_pass_is_the_launch_per_iteration_pass(request, scene_name, monkeypatch):
    """k_pso_ring (one launch per PSO pass: waves pop (candidate, particle) tasks from per-XCD rings, the wave that delivers a
    candidate's last fitness runs its swarm step and publishes the next iteration) against the per-iteration launches
    (k_pso_eval2 + k_pso_step) and against k_pso_iter: the same records byte for byte, in both evaluation shapes."""
    from pais_mvs_amd import _lib
    from pais_mvs_amd.config import readme_config
    from pais_mvs_amd.context import Context, make_candidate
    scene = request.getfixturevalue(scene_name)
    cfg = readme_config(adaptiveGradientEnable=(scene_name == "ring_small"))
    S = common.oracle_scene(cfg, scene)
    _, seeds = common.seed_candidates(S, scene)
    ctx = Context(cfg, scene.cameras, device=0, seed=42)
    kept = [r for r in ctx.refine_batch(seeds) if not r.dropped]
    ctx.close()
    assert len(kept) >= 8
    cands = []
    for i, r in enumerate(kept[:40]):
        for j in range(4):
            cen = [r.center[0] + 0.002 * (j - 1.5), r.center[1] + 0.001 * j, r.center[2] - 0.001 * j]
            cands.append(make_candidate(cen, list(r.normal[:]), [r.cam_idx[k] for k in range(r.num_cam)], 5000 + 11 * i + j, 1, normalS=list(r.normalS[:])))

    def run(env):
        out, ks = P.refine(monkeypatch, cfg, scene.cameras, cands, env)
        return bytes(out), ks

    ref, _ = run({})                                                       # small batch: k_pso_iter (every evaluation sets itself up)
    ring, ks = run(P.RING_SMALL_BATCH)                                     # (no size threshold: this batch is small)
    assert ks.eval2_launches == 1 and ks.ring_launches == 1 and ks.ring_fallbacks == 0, (ks.eval2_launches, ks.ring_launches)
    assert ks.ring_evals == ks.eval2_evals > 0
    launches, ks2 = run(P.EVAL2)
    assert ks2.eval2_launches > 10 and ks2.ring_launches == 0
    assert ring == launches == ref
    # round 6: in both large-batch pipelines the swarm step writes the evaluations' set-up records (pais_pre.hpp: normal, early
    # exits, homographies, corner test with the particles across the lanes); PAIS_PRE_SETUP=0 runs the kernels whose evaluation
    # waves compute them -- the same records byte for byte
    ring0, ks4 = run(dict(P.RING_SMALL_BATCH, **P.NO_PRE))
    assert ks4.ring_launches == 1 and ks4.ring_fallbacks == 0
    launches0, _ = run(dict(P.EVAL2, **P.NO_PRE))
    assert ring0 == launches0 == ref
    # a ring pass that does not complete (here: no patience at all -- the first wave that has to wait for an entry raises the
    # error word) is re-run through the per-iteration launches: the same records, and the re-run is counted
    fb, ks3 = run(dict(P.RING_SMALL_BATCH, **P.NO_PATIENCE))
    assert ks3.ring_fallbacks == 1 and ks3.eval2_launches > 10, (ks3.ring_fallbacks, ks3.eval2_launches)
    assert fb == ref
    S.close()


@pytest.mark.gpu
def test_seed_batches_and_device_pointer_batches_through_the_task_ring(pawn_small, monkeypatch):
    """Round 4: k_pso_ring also runs the passes of SEED batches (2N particles, several dependent passes: the later ones hold
    only the seeds that lost cameras) and batches on device pointers (pais_refine_batch_device: what a multi-GPU shard is).
    Records equal the default pipelines' byte for byte; a failing ring pass of a seed batch re-runs the whole batch."""
    from pais_mvs_amd.config import readme_config
    from pais_mvs_amd.mvs import MVS
    cfg = readme_config()
    S = common.oracle_scene(cfg, pawn_small)
    _, seeds = common.seed_candidates(S, pawn_small)

    def run(env):
        out, ks = P.refine(monkeypatch, cfg, pawn_small.cameras, seeds, env)
        return bytes(out), ks

    ref, ks0 = run(P.ITER)
    ring, ks1 = run(P.SEED_RING)                                   # every pass of the seed loop as one ring launch
    assert ks0.ring_launches == 0 and ks1.ring_launches >= 2 and ks1.ring_fallbacks == 0, (ks1.ring_launches, ks1.ring_fallbacks)
    assert ring == ref
    fb, ks2 = run(dict(P.SEED_RING, **P.NO_PATIENCE))
    assert ks2.ring_fallbacks >= 1 and fb == ref
    S.close()
    # device-pointer batches: the sharded code path with a world of one rank (RCCL communicator attached) refines every round
    # through pais_refine_batch_device; with no size threshold each round is one ring launch
    def cloud(env):
        import ctypes as C
        from pais_mvs_amd import _lib
        from pais_mvs_amd.mvs import get_unique_id
        with P.knobs(monkeypatch, env):
            m = MVS(cfg, pawn_small.cameras, device=0, seed=42)
            m.comm_init_rccl(0, 1, get_unique_id())
            m.set_replicate_below(0)                               # every batch takes the sharded (device-pointer) path
            for X, vis in pawn_small.seeds:
                m.add_seed(X, vis)
            m.refineSeedPatches()
            m.expansionPatches(64, 6)
            sha, st = m.cloud_sha1(), m.stats()
            ks = _lib.KernelStats()
            m.L.pais_get_kernel_stats(m.ctx_handle, C.byref(ks), 0)
            m.close()
        return sha, st, ks
    a, sta, ksa = cloud(P.ITER)
    b, stb, ksb = cloud(dict(P.RING_ANY_BATCH, **P.SEED_RING))
    assert a == b and sta.batches_sharded == stb.batches_sharded > 3
    assert ksa.ring_launches == 0 and ksb.ring_launches >= sta.batches_sharded and ksb.ring_fallbacks == 0, (ksb.ring_launches, sta.batches_sharded)
    # streamed rounds over the REAL RCCL communicator (a world of one rank): four sharded parts per round on four lanes, every
    # ncclAllGather enqueued on the driver's stream behind an event of the part's lane -- the same cloud as one batch per round
    def cloud_rounds(env):
        from pais_mvs_amd.mvs import get_unique_id
        with P.knobs(monkeypatch, env):
            m = MVS(cfg, pawn_small.cameras, device=0, seed=42)
            m.comm_init_rccl(0, 1, get_unique_id())
            m.set_replicate_below(0)
            for X, vis in pawn_small.seeds:
                m.add_seed(X, vis)
            m.refineSeedPatches()
            m.expansionPatches(4096, 8)
            sha, st = m.cloud_sha1(), m.stats()
            m.close()
        return sha, st
    c0, st0 = cloud_rounds({"PAIS_STREAM_ROUNDS": "0"})
    # (PAIS_STREAM_SHARDED=1: over a real communicator the streamed sharded rounds are opt-in until a run on >= 2 GPUs has been green)
    c1, st1 = cloud_rounds({"PAIS_STREAM_ROUNDS": "2", "PAIS_STREAM_ABOVE": "8", "PAIS_STREAM_PARTS": "4", "PAIS_STREAM_SHARDED": "1"})
    assert c0 == c1 and st0.rounds_streamed == 0 and st1.rounds_streamed > 0 and st1.batches_sharded > st0.batches_sharded


@pytest.mark.gpu
def test_emulated_ranks_of_a_larger_world_rebuild_the_single_rank_cloud(pawn_small, monkeypatch, capfd):
    """include/pais_mvs.h pais_mvs_emulate (round 4): rank r of a world of N on ONE GPU -- the real sharded code path (shard
    refined by the kernels, packed, device-written status header, copy down, unpack, replicated commit), the other ranks'
    blocks replayed from a recorded single-rank run.  Every rank of a world of 2 and of 3 (ragged shards) rebuilds the
    single-rank cloud bit for bit: with rounds as one sharded batch, with every round streamed in two sharded parts (two
    exchanges ordered on one stream), and when this rank's k_pso_ring pass does not complete (status header -> second
    exchange after the per-iteration re-run)."""
    from pais_mvs_amd.config import readme_config
    from pais_mvs_amd.mvs import MVS
    cfg = readme_config(particleNum=8, maxIteration=12)

    def run(env, worlds):
        with P.knobs(monkeypatch, env):
            m = MVS(cfg, pawn_small.cameras, device=0, seed=42)
            m.set_replicate_below(0)                                   # (test-size batches are thin: shard every one of them)

            def step():
                m.reset()
                for X, vis in pawn_small.seeds:
                    m.add_seed(X, vis)
                m.refineSeedPatches()
                m.expansionPatches(4096, 10)
                return m.cloud_sha1(), m.stats()
            ref, st0 = step()
            m.emulate(1)
            rec, _ = step()
            assert rec == ref
            out = []
            for N in worlds:
                for r in range(N):
                    m.emulate(2, r, N)
                    sha, st = step()
                    assert sha == ref, (env, N, r)
                    assert st.batches_sharded > 3 and st.exchange_bytes > 0 and st.candidates_refined == st0.candidates_refined
                    out.append(st)
            import ctypes as C
            from pais_mvs_amd import _lib
            ks = _lib.KernelStats()
            m.L.pais_get_kernel_stats(m.ctx_handle, C.byref(ks), 0)
            m.emulate(0)
            m.close()
        return out, ks

    sts, _ = run({"PAIS_STREAM_ROUNDS": "0"}, (2, 3))
    assert all(s.rounds_streamed == 0 for s in sts)
    sts, _ = run({"PAIS_STREAM_ROUNDS": "2", "PAIS_STREAM_ABOVE": "8", "PAIS_STREAM_PARTS": "2"}, (2, 3))
    assert all(s.rounds_streamed > 0 for s in sts)
    sts, _ = run({"PAIS_STREAM_ROUNDS": "2", "PAIS_STREAM_ABOVE": "8", "PAIS_STREAM_PARTS": "4"}, (2, 3))   # four parts, four lanes
    assert all(s.rounds_streamed > 0 for s in sts)
    sts, ks = run(dict(P.RING_ANY_BATCH, PAIS_STREAM_ROUNDS="0", **P.NO_PATIENCE), (2,))
    assert ks.ring_fallbacks > 0, ks.ring_fallbacks
    assert all(s.exchange_retries > 0 for s in sts)        # (round 6: the second exchanges are counted; bench.py --gpus N refuses a line over them)
    # round 6: the CANARY of streamed sharded rounds over a real communicator -- the first streamed round is refined once more as one
    # unstreamed sharded batch, the two record sets must be the same bytes (then streaming stays on): here on the emulation
    capfd.readouterr()
    sts, _ = run({"PAIS_STREAM_ROUNDS": "2", "PAIS_STREAM_ABOVE": "8", "PAIS_STREAM_PARTS": "2", "PAIS_STREAM_CANARY": "1",
                  "PAIS_STREAM_CANARY_LOG": "1"}, (2,))
    err = capfd.readouterr().err
    assert "== its unstreamed replay -> streaming on" in err and "!=" not in err, err
    assert all(s.rounds_streamed > 0 for s in sts)


@pytest.mark.gpu
def test_literal_gate_on_expansion_candidates_of_the_bench_workload(capsys, monkeypatch):
    """north_star's gate at WORKLOAD size: the bench scene (640x480 pawn, 200 seeds, R(4096)) is driven
    round by round through the stepwise entry points; ~2000 expansion candidates of rounds 5..25 -- late rounds: LOD > 0,
    K = 3 edge cases, parents that are themselves expansion patches -- are kept with the HIP path's records and refined again
    by the oracle in LITERAL arithmetic (platform libm, the reference's sequential sums, per-particle window) and in kernel
    arithmetic.  Same gate as tests/test_oracle_modes.py: the HIP records ARE the kernel-arithmetic patches bit for bit;
    dropped / camera set / reference camera / LOD identical to the literal run for every candidate; centre and normal
    within 1e-12 for every candidate on the literal run's PSO trajectory; branched trajectories counted against a cap, and
    reported by LOD and by camera count (tests/golden/literal_gate_bench_workload.json holds the measured figures that
    bench.py prints)."""
    import json
    from oracle import po
    from pais_mvs_amd import _lib
    from pais_mvs_amd.config import readme_config
    from pais_mvs_amd.mvs import MVS
    from tests.test_oracle_modes import mode_statistics
    from pais_mvs_amd import synth
    cfg = readme_config()
    scene = synth.pawn_scene(n_seeds=200, build_edges=False)    # bench.py's default workload
    m = MVS(cfg, scene.cameras, device=0, seed=42)
    for X, vis in scene.seeds:
        m.add_seed(X, vis)
    m.refineSeedPatches()
    m.expansion_begin()
    L = m.L
    L.pais_refine_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    kept_c, kept_r = [], []
    rnd = 0
    while True:
        done, cands, n = m.round_begin(4096)
        if done:
            break
        out = (_lib.PatchResult * max(n, 1))()
        if n:
            assert L.pais_refine_batch(m.ctx_handle, n, cands, out) == 0
            if 5 <= rnd <= 25:
                stride = max(1, n // 160)
                for i in range(0, n, stride):
                    c = _lib.Candidate()
                    C.memmove(C.byref(c), C.byref(cands[i]), C.sizeof(_lib.Candidate))
                    r = _lib.PatchResult()
                    C.memmove(C.byref(r), C.byref(out[i]), C.sizeof(_lib.PatchResult))
                    kept_c.append(c)
                    kept_r.append(r)
        m.round_commit(out, n)
        rnd += 1
    m.expansion_end()
    m.close()
    nk = len(kept_c)
    assert nk >= 1200 and rnd >= 26, (nk, rnd)
    # the candidates refined again on the box's host cores: literal, the four perturbed literal arithmetics (the CONTROL:
    # tests/test_cloud_parity.py), kernel arithmetic
    ctl, runs = common.literal_control(cfg, scene, kept_c)
    lit, ker = runs[0], runs["kernel"]
    st = mode_statistics(lit, ker, hip=kept_r)          # (asserts HIP == kernel arithmetic bit for bit)
    # round 6: the same candidates through the HIP path under PAIS_ARITH=literal (pais_literal.hpp: the cost in the reference's
    # statements and summation ORDER): its records ARE the oracle's with the literal cost bit for bit, and against the all-literal
    # run they branch no more often than the reference's own source with ONE rounding perturbed (variant 1) -- the floor of
    # BASELINE.md 7.1 as a measurement
    ctx_lit = P.context(cfg, scene.cameras, monkeypatch, P.LITERAL)  # (cfg carries the reconstruction's neighbour radius: MVS wrote it back)
    out_lit = ctx_lit.refine_batch(kept_c)
    ctx_lit.close()
    st_lit = mode_statistics(lit, runs["cost_literal"], hip=list(out_lit))   # (asserts HIP(literal) == oracle(cost literal) bit for bit)
    # branched candidates by LOD and by visible-camera count of the literal result
    by_lod, by_k = {}, {}
    mismatch_same = mismatch_branched = 0
    for a, b in zip(lit, ker):
        br = not (a.psoSig == b.psoSig and a.psoRuns == b.psoRuns and a.psoIters == b.psoIters)
        if bool(a.drop) != bool(b.drop) or (not a.drop and (a.cams() != b.cams() or a.refCamIdx != b.refCamIdx or a.LOD != b.LOD)):
            mismatch_same += int(not br)
            mismatch_branched += int(br)
        if a.drop or b.drop:
            continue
        for d, key in ((by_lod, int(a.LOD)), (by_k, int(a.numCam))):
            t = d.setdefault(key, [0, 0])
            t[0] += 1
            t[1] += int(br)
    rep = {"candidates": st["n"], "branched": st["branched"], "branched_fraction": st["branched"] / max(st["n"], 1),
           "same_trajectory_centre_max": st["same_centre_max"], "same_trajectory_normal_max": st["same_normal_max"],
           "branched_centre_max": st["branched_centre_max"], "branched_normal_max": st["branched_normal_max"],
           "set_mismatch_on_the_same_trajectory": mismatch_same, "set_mismatch_among_branched": mismatch_branched,
           "by_lod": {str(k): {"n": v[0], "branched": v[1]} for k, v in sorted(by_lod.items())},
           "by_num_cam": {str(k): {"n": v[0], "branched": v[1]} for k, v in sorted(by_k.items())},
           "control": {k: {"branched": v["branched"], "beyond_1e-4": v["beyond_1e-4"], "set_mismatch_among_branched": v["set_mismatch_among_branched"]}
                       for k, v in ctl.items() if k != "overlap"}, "control_overlap": ctl["overlap"],
           "hip_literal_arithmetic": {"branched": st_lit["branched"], "branched_fraction": st_lit["branched"] / max(st_lit["n"], 1),
                                      "same_trajectory_centre_max": st_lit["same_centre_max"], "same_trajectory_normal_max": st_lit["same_normal_max"],
                                      "branched_centre_max": st_lit["branched_centre_max"], "branched_normal_max": st_lit["branched_normal_max"],
                                      "set_mismatch": st_lit["set_mismatch"]}}
    with capsys.disabled():
        print("\nliteral gate, bench workload rounds 5..25:", json.dumps(rep))
    os.makedirs(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out"), exist_ok=True)
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out", "literal_gate_bench_workload.json"), "w") as f:
        json.dump(rep, f, indent=1)
    gdir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    gold = json.load(open(os.path.join(gdir, "literal_gate_bench_workload.json")))
    gctl = json.load(open(os.path.join(gdir, "literal_control_bench_workload.json")))
    assert st["n"] >= 1000 and mismatch_same == 0, (st, mismatch_same)       # discrete outputs identical wherever they CAN be compared
    assert st["same_centre_max"] <= 1e-12 and st["same_normal_max"] <= 1e-12, st
    assert st["same_trajectory"] + st["branched"] == st["n"]
    # DRIFT: the run is deterministic (HIP == kernel arithmetic bit for bit; the literal side is this image's
    # libm), so the figures bench.py prints from the committed file must be THE figures -- a change of two candidates fails
    assert st["n"] == gold["candidates"], (st["n"], gold["candidates"])
    assert abs(st["branched"] - gold["branched"]) <= 2, (st["branched"], gold["branched"])
    assert abs(mismatch_branched - gold["set_mismatch_among_branched"]) <= 1, mismatch_branched
    for k in ("variant_1", "variant_2", "variant_4", "variant_6"):
        assert abs(ctl[k]["branched"] - gctl[k]["branched"]) <= 2, (k, ctl[k]["branched"], gctl[k]["branched"])
    # literal arithmetic on the GPU: at or below the one-rounding control (measured: 7 against 15 of 1 817), no discrete mismatch
    assert st_lit["n"] == st["n"] and st_lit["branched"] <= ctl["variant_1"]["branched"], (st_lit, ctl["variant_1"]["branched"])
    assert st_lit["set_mismatch"] == 0 and st_lit["same_centre_max"] <= 1e-12 and st_lit["same_normal_max"] <= 1e-12, st_lit
    assert abs(st_lit["branched"] - gctl["cost_literal"]["branched"]) <= 2, (st_lit["branched"], gctl["cost_literal"]["branched"])
    # PARITY (weak 1): the cap is not "measured + 10" but the CONTROL -- what the reference's own source branches under another
    # loop order and another compiler (variant 6) -- times a margin (tests/test_cloud_parity.py)
    from tests.test_cloud_parity import BRANCH_FACTOR_OVER_CONTROL
    assert st["branched"] <= BRANCH_FACTOR_OVER_CONTROL * ctl["variant_6"]["branched"], (st["branched"], ctl["variant_6"]["branched"])
    assert ctl["kernel"]["beyond_1e-4"] <= BRANCH_FACTOR_OVER_CONTROL * ctl["variant_6"]["beyond_1e-4"]
    assert mismatch_branched <= ctl["variant_6"]["set_mismatch_among_branched"] + 1
