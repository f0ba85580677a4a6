"""pais_pso_trace: refine() (patch.cpp:114-219) with every PSO run of its loop and every iteration of each run
(psosolver.cpp:94-305) recorded.

The checker is a restatement of po_refine / po_refine_seed here (`traced_refine`), built only from what oracle/po.py binds:
the setters, po_pso_run with its trace (fed by po_fit_cb / po_rng_cb and the ranges of patch.cpp:183-200) and
po_pso_optimization for the write-back.  On the CPU it is pinned against po_refine_seed / po_expand_candidate byte for byte;
row 0, which the oracle does not trace, is restated from pais_rand31.  On the GPU the call's records equal refine_batch's,
its rows equal the oracle's trace bit for bit, and the rows agree with fitness_batch and with the convergence test.
"""
import ctypes as C
import math

import numpy as np
import pytest

from tests import common, pipelines as P

# ---------------------------------------------------------------------------------------------------------------------
# the checker
# ---------------------------------------------------------------------------------------------------------------------
def _patch_bytes(p):
    return C.string_at(C.addressof(p), C.sizeof(p))


def _run_box(S, p):
    """Ranges, init, N and maxIt of Patch::psoOptimization (patch.cpp:183-200), as po_pso_optimization forms them."""
    cfg = S.cfg
    ns0, ns1 = float(p.normalS[0]), float(p.normalS[1])
    lo = [0.0, ns1 - math.pi / 2.0, float(p.depthRange[0])]
    hi = [math.pi, ns1 + math.pi / 2.0, float(p.depthRange[1])]
    if p.type == 0:                                                  # seed
        N, maxIt = cfg.particleNum * 2, cfg.maxIteration * 2
    else:
        a, b = ns0 - math.pi / cfg.reduceNormalRange, ns0 + math.pi / cfg.reduceNormalRange
        lo[0] = 0.0 if 0.0 >= a else a
        hi[0] = b if b < math.pi else math.pi
        lo[1] = ns1 - math.pi / cfg.reduceNormalRange
        hi[1] = ns1 + math.pi / cfg.reduceNormalRange
        N, maxIt = cfg.particleNum, cfg.maxIteration
    return lo, hi, [ns0, ns1, float(p.depth)], N, maxIt


def pso_run_traced(S, p):
    """po_pso_run of the patch's next PSO run with its trace (OpenMP off): the run's state, iteration count and rows 1..it as
    (it, N, 11) particles + g_idx + iw."""
    from oracle import po
    L = po.lib()
    lo, hi, init, N, maxIt = _run_box(S, p)
    fc = po.FitCtx(C.cast(S.ptr, C.c_void_p).value, C.addressof(p))
    rc = po.RngCtx(S.s.seed, p.key, p.psoRuns, 0)
    res = po.PsoResult()
    row = N * 11 + 2
    cap = maxIt * row
    tr = (C.c_double * max(cap, 1))()
    tl = C.c_int(0)
    fit_cb = C.cast(L.po_fit_cb, C.c_void_p)
    rng_cb = C.cast(L.po_rng_cb, C.c_void_p)
    omp = S.s.ompParticles
    S.set_omp(False)
    L.po_pso_run(3, po.darr(lo), po.darr(hi), fit_cb, C.byref(fc), maxIt, N, po.darr(init), rng_cb, C.byref(rc), 0, C.byref(res),
                 tr, cap, C.byref(tl))
    S.s.ompParticles = omp
    it = int(res.iterations)
    assert tl.value == it * row
    rows = np.frombuffer(tr, dtype=np.float64, count=it * row).reshape(it, row) if it else np.zeros((0, row))
    return {"range_l": lo, "range_u": hi, "init": init, "ray": list(p.ray[:]), "run": int(p.psoRuns), "ref_cam": int(p.refCamIdx),
            "lod": int(p.LOD), "cams": p.cams(), "N": N, "maxIt": maxIt, "iterations": it,
            "particles": rows[:, :N * 11].reshape(it, N, 11).copy(), "g_idx": rows[:, N * 11].astype(int), "iw": rows[:, N * 11 + 1].copy(),
            "gBest": list(res.gBest[:]), "gBestFitness": float(res.gBestFitness)}


def traced_refine(S, p, is_seed):
    """po_refine_seed (is_seed) or the expansion driver's refine (tests/common.oracle_refine_patch) of patch p, restated from the
    setters, the traced po_pso_run and po_pso_optimization; p is refined in place.  Returns the runs (pso_run_traced)."""
    from oracle import po
    L = po.lib()
    s, cfg = S.ptr, S.cfg
    runs = []
    if not is_seed and p.numCam < cfg.minCamNum:
        p.drop = 1                                                    # expandVisibleCamera :758-760
    if p.numCam < cfg.minCamNum:                                      # patch.cpp:118-123
        p.fitness = common.DBL_MAX
        p.priority = common.DBL_MAX
        p.drop = 1
    else:
        for f in (L.po_set_reference_camera, L.po_set_depth_and_ray, L.po_set_depth_range, L.po_set_lod):
            f(s, C.byref(p))
        if not p.drop:
            before_ref, after_ref, before_num, after_num = p.refCamIdx, -1, p.numCam, -1
            count, total = 0, p.numCam
            dropped = False
            while before_ref != after_ref or before_num != after_num:
                if not count <= total:                                # `count++ <= totalCamNum`
                    break
                count += 1
                if p.numCam < cfg.minCamNum:
                    p.fitness = common.DBL_MAX
                    p.priority = common.DBL_MAX
                    p.drop = 1
                    dropped = True
                    break
                before_ref, before_num = p.refCamIdx, p.numCam
                runs.append(pso_run_traced(S, p))
                L.po_pso_optimization(s, C.byref(p))
                if p.fitness > cfg.maxFitness:
                    p.drop = 1
                    dropped = True
                    break
                for f in (L.po_remove_invisible_camera, L.po_set_reference_camera, L.po_set_depth_and_ray, L.po_set_depth_range,
                          L.po_set_lod):
                    f(s, C.byref(p))
                if p.type == 1:
                    break
                after_ref, after_num = p.refCamIdx, p.numCam
            if not dropped:
                L.po_set_priority(s, C.byref(p))
                L.po_set_image_point(s, C.byref(p))
    L.po_remove_invisible_camera(s, C.byref(p))                       # mvs.cpp:215 / 574
    return runs


def restate_row0(seed, key, run, lo, hi, init, N):
    """The initial swarm (initParticles psosolver.cpp:94-110 + setParticle(init) :267-284) from pais_rand31, following
    k_pso_init: (N, 3) positions and velocities."""
    from pais_mvs_amd import _lib
    L = _lib.load()
    u = lambda k: float(L.pais_rand31(seed, key, run, k)) / 2147483647.0
    pos, vec = np.zeros((N, 3)), np.zeros((N, 3))
    for d in range(3):
        ri = hi[d] - lo[d]
        for i in range(N):
            pos[i, d] = (ri * u(2 * (d * N + i))) + lo[d]
            vec[i, d] = (2.0 * ri * u(2 * (d * N + i) + 1)) - ri
        pos[0, d] = init[d]
        vec[0, d] = (2.0 * ri * u(6 * N + d)) - ri
    return pos, vec


def oracle_trace(S, results, max_runs, R, NP):
    """The checker's runs in pais_pso_trace's layout: a PsoTrace of the refined patches (records from the oracle patches) with
    run info, rows 1..it from po_pso_run's trace and row 0's positions / velocities from restate_row0 (its fitness is not
    traced by the oracle: 0)."""
    from pais_mvs_amd.context import PSO_ITER_DTYPE, PSO_RUN_INFO_DTYPE, PsoTrace
    n = len(results)
    recs = (common._lib.PatchResult * max(n, 1))()
    info = np.zeros((n, max_runs), dtype=PSO_RUN_INFO_DTYPE)
    iters = np.zeros((n, max_runs, R), dtype=PSO_ITER_DTYPE)
    parts = np.zeros((n, max_runs, R, NP, 11))
    for c, (p, runs) in enumerate(results):
        common.record_from_oracle_patch(p, recs[c])
        for r, o in enumerate(runs[:max_runs]):
            N, it = o["N"], o["iterations"]
            ri = info[c, r]
            ri["range_l"], ri["range_u"], ri["init"], ri["ray"] = o["range_l"], o["range_u"], o["init"], o["ray"]
            ri["run"], ri["ref_cam"], ri["lod"], ri["num_cam"] = o["run"], o["ref_cam"], o["lod"], len(o["cams"])
            ri["cam_idx"][:len(o["cams"])] = o["cams"]
            ri["n_particles"], ri["max_iteration"], ri["iterations"] = N, o["maxIt"], it
            pos0, vec0 = restate_row0(S.s.seed, p.key, r, o["range_l"], o["range_u"], o["init"], N)
            parts[c, r, 0, :N, 0:3], parts[c, r, 0, :N, 3:6], parts[c, r, 0, :N, 6:9] = pos0, vec0, pos0
            parts[c, r, 1:it + 1, :N] = o["particles"]
            iters[c, r, 0]["iw"] = 0.8
            for t in range(1, it + 1):
                g = int(o["g_idx"][t - 1])
                row = iters[c, r, t]
                row["g_idx"], row["iw"], row["iteration"] = g, o["iw"][t - 1], t
                row["gbest"], row["gbest_fitness"] = o["particles"][t - 1, g, 6:9], o["particles"][t - 1, g, 10]
            iters[c, r, it]["ended"] = 1
    return PsoTrace(recs, n, info, iters, parts)


def convergence(pos, vec, gbest, N):
    """getDispersionIDX / getVelocityIDX (psosolver.cpp:70-92) as run() uses them (:293-297), sequentially."""
    disp = 0.0
    for i in range(N):
        for d in range(3):
            disp += abs(pos[i, d] - gbest[d])
    disp /= 3 * N
    if not disp < 0.01:
        return disp, float("nan")
    vel = 0.0
    for i in range(N):
        for d in range(3):
            vel += abs(vec[i, d])
    return disp, vel / (3 * N)


# ---------------------------------------------------------------------------------------------------------------------
# scenes and candidates
# ---------------------------------------------------------------------------------------------------------------------
def _seed_pats(S, scene, keys=None):
    pats, cands = common.seed_candidates(S, scene)
    if keys is not None:
        pats, cands = [pats[i] for i in keys], [cands[i] for i in keys]
    return pats, cands


def _cpu_expansions(S, scene, n):
    """Expansion candidates beside refined seeds (the constructor of patch.cpp:36-43), kernel arithmetic."""
    from oracle import po
    from pais_mvs_amd.context import make_candidate
    L = po.lib()
    out = []
    for i, (X, vis) in enumerate(scene.seeds):
        p = S.seed_patch(X, vis, key=i)
        L.po_refine_seed(S.ptr, C.byref(p))
        if p.drop:
            continue
        for j, off in enumerate(((0.004, 0, 0), (0, 0.004, 0), (0, 0, 0.004))):
            c = [p.center[k] + off[k] for k in range(3)]
            q = S.expand_patch(c, p.normal[:], p.cams(), key=1000 + 10 * i + j)
            out.append((q, make_candidate(q.center[:], q.normal[:], q.cams(), q.key, 1, normalS=q.normalS[:])))
            if len(out) >= n:
                return out
    return out


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_sizeof_pso_trace_structs_match_the_ctypes_mirrors():
    from pais_mvs_amd import _lib, context
    L = _lib.load()
    assert L.pais_sizeof_pso_run_info() == C.sizeof(_lib.PsoRunInfo) == context.PSO_RUN_INFO_DTYPE.itemsize == 384
    assert L.pais_sizeof_pso_iter() == C.sizeof(_lib.PsoIter) == context.PSO_ITER_DTYPE.itemsize == 72
    assert _lib.PsoRunInfo.cam_idx.offset == 128 and _lib.PsoIter.g_idx.offset == 56


@pytest.mark.parametrize("literal", [False, True], ids=["kernel", "cost_literal"])
def test_checker_restates_refine(pawn_small, literal):
    """traced_refine's final patch equals po_refine_seed / the expansion driver's refine byte for byte, and each run's last
    gIdx gives the gBest its write-back received."""
    from oracle import po
    from pais_mvs_amd.config import readme_config
    L = po.lib()
    cfg = readme_config()
    S = common.oracle_scene(cfg, pawn_small)
    S.set_kernel_arithmetic(True)
    S.set_cost_literal(literal)
    seeds, _ = _seed_pats(S, pawn_small, keys=range(8))
    cases = [(p, True) for p in seeds] + [(q, False) for q, _ in _cpu_expansions(S, pawn_small, 8)]
    multi = 0
    results = []
    for p0, is_seed in cases:
        a, b = common.copy_struct(p0), common.copy_struct(p0)
        runs = traced_refine(S, a, is_seed)
        results.append((a, runs))
        common.oracle_refine_patch(S, b, is_seed)
        assert _patch_bytes(a) == _patch_bytes(b), (p0.key, is_seed)
        assert len(runs) == b.psoRuns
        multi += len(runs) > 1
        for r in runs:
            if r["iterations"]:
                g = r["g_idx"][-1]
                assert list(r["particles"][-1, g, 6:9]) == r["gBest"]
                assert r["particles"][-1, g, 10] == r["gBestFitness"]
            assert r["iw"].tolist() == _iw_rows(r["maxIt"], r["iterations"])[1:]
    assert multi >= 1                                                 # (the seed loop ran more than one PSO somewhere)
    # in pais_pso_trace's layout: the runs and rows, the last row's gBest is the patch's final particle
    tr = oracle_trace(S, results, 8, 2 * cfg.maxIteration + 1, 2 * cfg.particleNum)
    assert tr.first_branch(tr) == [None] * len(results)
    for c, (p, runs) in enumerate(results):
        assert tr.runs(c) == len(runs) == p.psoRuns
        assert sum(tr.rows(c, r) - 1 for r in range(tr.runs(c))) == p.psoIters
        if runs and runs[-1]["iterations"]:
            last = tr.iters[c, len(runs) - 1, tr.rows(c, len(runs) - 1) - 1]
            assert list(last["gbest"][:2]) == [p.normalS[0], p.normalS[1]] and last["ended"] == 1   # (setDepthAndRay moves depth)
    S.close()


def _iw_rows(maxIt, it):
    iw, out = 0.8, [0.8]
    for _ in range(it):
        iw = (iw - 1.0 / maxIt) if (iw - 1.0 / maxIt) > 0.4 else 0.4
        out.append(iw)
    return out


def test_row0_restatement_is_the_oracles_initial_swarm(pawn_small):
    """restate_row0 gives, bit for bit, the first N positions po_pso_run evaluates (captured through a Python FITNESS_FN)."""
    from oracle import po
    from pais_mvs_amd.config import readme_config
    L = po.lib()
    cfg = readme_config()
    S = common.oracle_scene(cfg, pawn_small)
    S.set_kernel_arithmetic(True)
    seeds, _ = _seed_pats(S, pawn_small, keys=range(3))
    cases = [(p, True) for p in seeds] + [(q, False) for q, _ in _cpu_expansions(S, pawn_small, 2)]
    for p0, is_seed in cases:
        a = common.copy_struct(p0)
        tr = oracle_trace(S, [(a, traced_refine(S, a, is_seed))], 1, 2 * cfg.maxIteration + 1, 2 * cfg.particleNum)
        p, run = common.copy_struct(p0), 0
        for f in (L.po_set_reference_camera, L.po_set_depth_and_ray, L.po_set_depth_range, L.po_set_lod):
            f(S.ptr, C.byref(p))
        p.psoRuns = run
        lo, hi, init, N, maxIt = _run_box(S, p)
        seen = []

        def fit(pos, _obj):
            seen.append([pos[0], pos[1], pos[2]])
            return 1.0

        cb = po.FITNESS_FN(fit)
        rc = po.RngCtx(S.s.seed, p.key, run, 0)
        res = po.PsoResult()
        L.po_pso_run(3, po.darr(lo), po.darr(hi), C.cast(cb, C.c_void_p), None, 2, N, po.darr(init), C.cast(L.po_rng_cb, C.c_void_p),
                     C.byref(rc), 0, C.byref(res), None, 0, None)
        assert tr.runs(0) == 1 and int(tr.run_info[0, 0]["n_particles"]) == N
        assert np.array_equal(np.array(seen[:N]), tr.swarm(0, 0, 0)["pos"]), p.key
    S.close()


def _fake_trace(g_rows, fits=None, runs=None):
    """A PsoTrace of one candidate from g_idx rows per run (and per-row particle fitness / pBest fitness for the improved sets)."""
    from pais_mvs_amd import _lib
    from pais_mvs_amd.context import PSO_ITER_DTYPE, PSO_RUN_INFO_DTYPE, PsoTrace
    R = max(len(g) for g in g_rows) + 2
    N = 4
    rec = (_lib.PatchResult * 1)()
    rec[0].pso_runs = runs if runs is not None else len(g_rows)
    info = np.zeros((1, 3), dtype=PSO_RUN_INFO_DTYPE)
    it = np.zeros((1, 3, R), dtype=PSO_ITER_DTYPE)
    parts = np.zeros((1, 3, R, N, 11)) if fits is not None else None
    for r, g in enumerate(g_rows):
        info[0, r]["iterations"] = len(g) - 1
        info[0, r]["n_particles"] = N
        info[0, r]["num_cam"] = 3
        info[0, r]["cam_idx"][:3] = [0, 1, 2]
        for t, v in enumerate(g):
            it[0, r, t]["g_idx"] = v
            if fits is not None:
                parts[0, r, t, :, 9] = fits[r][t][0]
                parts[0, r, t, :, 10] = fits[r][t][1]
    return PsoTrace(rec, 1, info, it, parts)


def test_first_branch_on_synthetic_traces():
    a = _fake_trace([[0, 1, 1, 2], [3, 3]])
    assert a.first_branch(_fake_trace([[0, 1, 1, 2], [3, 3]])) == [None]
    assert a.first_branch(_fake_trace([[0, 1, 2, 2], [3, 3]])) == [(0, 2)]            # g_idx
    assert a.first_branch(_fake_trace([[0, 1, 1, 2], [3, 0]])) == [(1, 1)]
    assert a.first_branch(_fake_trace([[0, 1, 1], [3, 3]])) == [(0, 2)]               # row count: one run stopped after row 2
    assert a.first_branch(_fake_trace([[0, 1, 1, 2]])) == [(1, 0)]                    # run count
    # improved sets: row 1 replaces particles {0, 1} in one trace, {0} in the other (fit < previous row's pBestFitness)
    f0 = [([5, 5, 5, 5], [5, 5, 5, 5]), ([4, 4, 6, 6], [4, 4, 5, 5]), ([4, 4, 4, 4], [4, 4, 4, 4])]
    f1 = [([5, 5, 5, 5], [5, 5, 5, 5]), ([4, 5, 6, 6], [4, 5, 5, 5]), ([4, 4, 4, 4], [4, 4, 4, 4])]
    b0 = _fake_trace([[0, 0, 0]], fits=[f0])
    assert b0.first_branch(_fake_trace([[0, 0, 0]], fits=[f0])) == [None]
    assert b0.first_branch(_fake_trace([[0, 0, 0]], fits=[f1])) == [(0, 1)]
    assert b0.first_branch(_fake_trace([[0, 0, 0]])) == [None]                        # (one trace without particles: g_idx only)
    assert b0.improved(0, 0, 1).tolist() == [0, 1] and b0.improved(0, 0, 2).tolist() == [2, 3]


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
def _ctx(cfg, scene, monkeypatch, literal=False):
    return P.context(cfg, scene.cameras, monkeypatch, P.LITERAL if literal else {})


def _same(a, b):
    """Bit-identical arrays (NaN rows included)."""
    return a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _rec_bytes(recs, n):
    return [C.string_at(C.addressof(recs[i]), C.sizeof(recs[i])) for i in range(n)]


def _round_candidates(cfg, scene, rounds=(2, 4), per_round=48):
    """Expansion candidates of early rounds of the stepwise scheduler, refined with the GPU's own records; the config comes back
    with the reconstruction's neighbour radius."""
    from pais_mvs_amd.mvs import MVS
    m = MVS(cfg, scene.cameras, device=0, seed=42)
    for X, vis in scene.seeds:
        m.add_seed(X, vis)
    L = m.L
    L.pais_refine_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    cands, n = m.seed_begin()
    out = (common._lib.PatchResult * max(n, 1))()
    assert L.pais_refine_batch(m.ctx_handle, n, cands, out) == 0
    m.seed_commit(out, n)
    m.expansion_begin()
    kept = []
    rnd = 0
    while rnd <= rounds[1]:
        done, cands, n = m.round_begin(256)
        if done:
            break
        out = (common._lib.PatchResult * max(n, 1))()
        if n:
            assert L.pais_refine_batch(m.ctx_handle, n, cands, out) == 0
            if rounds[0] <= rnd:
                for i in range(0, n, max(1, n // per_round)):
                    kept.append(common.copy_struct(cands[i]))
        m.round_commit(out, n)
        rnd += 1
    radius = m.neighbor_radius()
    m.expansion_end()
    m.close()
    cfg.neighborRadius = radius
    return kept


@pytest.fixture(scope="module")
def workload(pawn_small):
    """README config, the pawn seeds and expansion candidates of early rounds (with the radius the reconstruction set)."""
    from pais_mvs_amd.config import readme_config
    cfg = readme_config()
    exp = _round_candidates(cfg, pawn_small)
    assert len(exp) >= 48
    S = common.oracle_scene(cfg, pawn_small)
    _, seeds = _seed_pats(S, pawn_small)
    S.close()
    return cfg, seeds, exp


def _oracle_runs(cfg, scene, cands, is_seed, literal=False):
    S = common.oracle_scene(cfg, scene)
    S.set_kernel_arithmetic(True)
    S.set_cost_literal(literal)
    S.ptr.contents.cfg.neighborRadius = cfg.neighborRadius
    out = []
    for c in cands:
        p = common.oracle_patch_from_candidate(c)
        runs = traced_refine(S, p, is_seed)
        out.append((p, runs))
    S.close()
    return out


def _check_oracle_parity(tr, oracle, what):
    """Records, run info and every row t >= 1 (11 doubles per particle, g_idx, iw) against the oracle's trace bit for bit; the
    two fitness fields of a particle (fit, pBestFitness) also agree when both are NaN, since the sign and payload of a NaN are
    not part of the statement (tests/knn_ref.py).  Returns the first mismatch as (candidate, run, row, what) or None."""
    for c, (p, runs) in enumerate(oracle):
        rec = tr.records[c]
        if (rec.pso_runs, rec.pso_iterations, bool(rec.dropped)) != (p.psoRuns, p.psoIters, bool(p.drop)):
            return (c, -1, -1, "record")
        assert tr.runs(c) == min(len(runs), tr.max_runs)
        for r in range(tr.runs(c)):
            o, ri = runs[r], tr.run_info[c, r]
            k = int(ri["num_cam"])
            got = (list(ri["range_l"]), list(ri["range_u"]), list(ri["init"]), list(ri["ray"]), int(ri["run"]), int(ri["ref_cam"]),
                   int(ri["lod"]), list(ri["cam_idx"][:k]), int(ri["n_particles"]), int(ri["max_iteration"]), int(ri["iterations"]))
            want = (o["range_l"], o["range_u"], o["init"], o["ray"], o["run"], o["ref_cam"], o["lod"], o["cams"], o["N"], o["maxIt"],
                    o["iterations"])
            if got != want:
                return (c, r, 0, "run info")
            N = o["N"]
            for t in range(1, o["iterations"] + 1):
                row = tr.iters[c, r, t]
                if int(row["g_idx"]) != o["g_idx"][t - 1] or float(row["iw"]) != o["iw"][t - 1] or int(row["iteration"]) != t:
                    return (c, r, t, "header")
                if tr.particles is not None:
                    got, want = np.ascontiguousarray(tr.particles[c, r, t, :N]), np.ascontiguousarray(o["particles"][t - 1])
                    same = got.view(np.uint64) == want.view(np.uint64)
                    same[:, 9:11] |= np.isnan(got[:, 9:11]) & np.isnan(want[:, 9:11])
                    if not same.all():
                        return (c, r, t, "particles")
    return None


@pytest.mark.gpu
@pytest.mark.parametrize("literal", [False, True], ids=["kernel", "literal"])
def test_gpu_pso_trace_records_equal_refine_batch(pawn_small, workload, monkeypatch, literal):
    cfg, seeds, exp = workload
    ctx = _ctx(cfg, pawn_small, monkeypatch, literal)
    for cands in (seeds, exp):
        ref = ctx.refine_batch(cands)
        tr = ctx.pso_trace(cands, max_runs=8)
        assert _rec_bytes(tr.records, len(cands)) == _rec_bytes(ref, len(cands))
        for c in range(len(cands)):
            assert tr.runs(c) == min(ref[c].pso_runs, 8)
            for r in range(tr.runs(c)):
                R = tr.rows(c, r)
                assert tr.iters[c, r, R - 1]["ended"] == 1 and (tr.iters[c, r, :R - 1]["ended"] == 0).all()
                assert (tr.iters[c, r, R:]["iteration"] == 0).all() and (tr.iters[c, r, :R]["iteration"] == np.arange(R)).all()
            assert sum(tr.rows(c, r) - 1 for r in range(tr.runs(c))) == ref[c].pso_iterations or ref[c].pso_runs > 8
    ctx.close()


@pytest.mark.gpu
def test_gpu_pso_trace_matches_the_oracle_kernel_arithmetic(pawn_small, workload, monkeypatch):
    cfg, seeds, exp = workload
    ctx = _ctx(cfg, pawn_small, monkeypatch)
    for cands, is_seed in ((seeds[:24], True), (exp[:48], False)):
        tr = ctx.pso_trace(cands, max_runs=8, particles=True)
        oracle = _oracle_runs(cfg, pawn_small, cands, is_seed)
        assert _check_oracle_parity(tr, oracle, "kernel") is None, _check_oracle_parity(tr, oracle, "kernel")
    ctx.close()


@pytest.mark.gpu
def test_gpu_pso_trace_matches_the_oracle_literal_arithmetic(pawn_small, workload, monkeypatch):
    cfg, seeds, exp = workload
    ctx = _ctx(cfg, pawn_small, monkeypatch, literal=True)
    for cands, is_seed in ((seeds[:8], True), (exp[:16], False)):
        tr = ctx.pso_trace(cands, max_runs=8, particles=True)
        oracle = _oracle_runs(cfg, pawn_small, cands, is_seed, literal=True)
        bad = _check_oracle_parity(tr, oracle, "literal")
        assert bad is None, "first mismatch (candidate, run, row, what): %r" % (bad,)
    ctx.close()


@pytest.mark.gpu
def test_gpu_pso_trace_rows_are_self_consistent(pawn_small, workload, monkeypatch):
    """Row 0 is the restatement; every row's fitness is fitness_batch of its positions (state from the run info) bit for bit;
    g_idx / gbest follow from pBestFitness (<=, last index wins); dispersion and velocity are the convergence test's."""
    from pais_mvs_amd import _lib
    cfg, seeds, exp = workload
    ctx = _ctx(cfg, pawn_small, monkeypatch)
    for cands in (seeds[:8], exp[:16]):
        tr = ctx.pso_trace(cands, max_runs=8, particles=True)
        states, idx, pts, fits = [], [], [], []
        for c in range(len(cands)):
            for r in range(tr.runs(c)):
                ri = tr.run_info[c, r]
                N, R, maxIt = int(ri["n_particles"]), tr.rows(c, r), int(ri["max_iteration"])
                sw0 = tr.swarm(c, r, 0)
                pos0, vec0 = restate_row0(42, cands[c].key, r, list(ri["range_l"]), list(ri["range_u"]), list(ri["init"]), N)
                assert np.array_equal(sw0["pos"], pos0) and np.array_equal(sw0["vec"], vec0) and np.array_equal(sw0["pbest"], pos0)
                st = _lib.PatchState()
                st.ray[:] = list(ri["ray"])
                st.ref_cam, st.lod, st.num_cam = int(ri["ref_cam"]), int(ri["lod"]), int(ri["num_cam"])
                for k in range(st.num_cam):
                    st.cam_idx[k] = int(ri["cam_idx"][k])
                states.append(st)
                for t in range(R):
                    sw, row = tr.swarm(c, r, t), tr.iters[c, r, t]
                    idx += [len(states) - 1] * N
                    pts.append(sw["pos"])
                    fits.append(sw["fit"])
                    pf = sw["pbest_fit"]
                    # updateGbest (:137-149): `<=`, last index wins; gBestFitness carried over from the row before
                    g, gf = (0, pf[0]) if t == 0 else (int(tr.iters[c, r, t - 1]["g_idx"]), float(tr.iters[c, r, t - 1]["gbest_fitness"]))
                    for j in range(N):
                        if pf[j] <= gf:
                            g, gf = j, pf[j]
                    assert int(row["g_idx"]) == g, (c, r, t)
                    gi = int(row["g_idx"])
                    assert list(row["gbest"]) == list(sw["pbest"][gi]) and float(row["gbest_fitness"]) == pf[gi]
                    disp, vel = (float("nan"), float("nan")) if t >= maxIt else convergence(sw["pos"], sw["vec"], sw["pbest"][gi], N)
                    for got, want in ((float(row["dispersion"]), disp), (float(row["velocity"]), vel)):
                        assert (math.isnan(got) and math.isnan(want)) or got == want, (c, r, t)
                    assert float(row["iw"]) == _iw_rows(maxIt, t)[t]
        got = ctx.fitness_batch(states, idx, np.concatenate(pts))
        assert np.array_equal(got.view(np.uint64), np.concatenate(fits).view(np.uint64))
    ctx.close()


@pytest.mark.gpu
def test_gpu_pso_trace_shapes_and_edges(pawn_small, workload, monkeypatch):
    from pais_mvs_amd import _lib
    from pais_mvs_amd.config import readme_config
    cfg, seeds, exp = workload
    ctx = _ctx(cfg, pawn_small, monkeypatch)
    full = ctx.pso_trace(seeds, max_runs=8, particles=True)
    # max_runs = 1: the first run as recorded with max_runs 8, the records complete
    one = ctx.pso_trace(seeds, max_runs=1, particles=True)
    assert _rec_bytes(one.records, len(seeds)) == _rec_bytes(full.records, len(seeds))
    assert any(full.records[c].pso_runs > 1 for c in range(len(seeds)))
    assert _same(one.iters[:, 0], full.iters[:, 0]) and _same(one.run_info[:, 0], full.run_info[:, 0])
    assert _same(one.particles[:, 0], full.particles[:, 0])
    # particles = NULL: the same headers
    hdr = ctx.pso_trace(seeds, max_runs=8)
    assert hdr.particles is None and _same(hdr.iters, full.iters) and _same(hdr.run_info, full.run_info)
    # chunks: a tiny staging bound, several chunks, the same output
    with P.knobs(monkeypatch, {"PAIS_TRACE_STAGING_MB": "0.3"}):
        ch = ctx.pso_trace(seeds, max_runs=8, particles=True)
    assert _rec_bytes(ch.records, len(seeds)) == _rec_bytes(full.records, len(seeds))
    assert _same(ch.iters, full.iters) and _same(ch.run_info, full.run_info)
    assert _same(ch.particles, full.particles)
    # candidates dropped before the PSO (fewer than minCamNum cameras) record nothing
    few = [common.copy_struct(c) for c in exp[:4]]
    for c in few:
        c.num_cam = 2
    mixed = few + exp[:4]
    tm = ctx.pso_trace(mixed, max_runs=2, particles=True)
    for c in range(4):
        assert tm.records[c].dropped and tm.runs(c) == 0
        assert not tm.run_info[c].tobytes().strip(b"\0") and not tm.iters[c].tobytes().strip(b"\0") and not tm.particles[c].any()
    assert _rec_bytes(tm.records, 8) == _rec_bytes(ctx.refine_batch(mixed), 8)
    # n = 0
    assert len(ctx.pso_trace([], max_runs=1)) == 0
    ctx.close()
    # particleNum 40: seeds have N = 80 > 64 particles (the step's lane loop)
    cfg40 = readme_config(particleNum=40, maxIteration=10)
    cfg40.neighborRadius = cfg.neighborRadius
    ctx = _ctx(cfg40, pawn_small, monkeypatch)
    tr = ctx.pso_trace(seeds[:4], max_runs=4, particles=True)
    assert tr.particles.shape[3] == 80 and int(tr.run_info[0, 0]["n_particles"]) == 80
    assert _rec_bytes(tr.records, 4) == _rec_bytes(ctx.refine_batch(seeds[:4]), 4)
    assert _check_oracle_parity(tr, _oracle_runs(cfg40, pawn_small, seeds[:4], True), "N 80") is None
    ctx.close()


@pytest.mark.gpu
def test_gpu_pso_trace_64_cameras(monkeypatch):
    """A seed seen by the 64 cameras of a ring: the run info's camera list and the oracle parity at K = 64."""
    from pais_mvs_amd import synth
    from pais_mvs_amd.config import readme_config
    from pais_mvs_amd.context import make_candidate
    scene = synth.ring_scene(n_cams=64, width=160, height=120, focal=150.0, radius=3.0, n_seeds=2)
    cfg = readme_config(patchRadius=4, maxIteration=6, minCamNum=3)
    S = common.oracle_scene(cfg, scene)
    X = scene.seeds[0][0]
    p = S.seed_patch(X, list(range(64)), key=7)
    S.close()
    cand = make_candidate(p.center[:], p.normal[:], p.cams(), 7, 0, normalS=p.normalS[:])
    ctx = _ctx(cfg, scene, monkeypatch)
    tr = ctx.pso_trace([cand], max_runs=4, particles=True)
    assert _rec_bytes(tr.records, 1) == _rec_bytes(ctx.refine_batch([cand]), 1)
    if tr.runs(0):
        assert int(tr.run_info[0, 0]["num_cam"]) <= 64
    assert _check_oracle_parity(tr, _oracle_runs(cfg, scene, [cand], True), "K 64") is None
    ctx.close()


@pytest.mark.gpu
def test_gpu_pso_trace_rejects_bad_input(pawn_small, workload, monkeypatch):
    from pais_mvs_amd import _lib
    cfg, seeds, exp = workload
    ctx = _ctx(cfg, pawn_small, monkeypatch)
    L = ctx.L
    ctx.trace_stats(reset=True)
    ks0 = _lib.KernelStats()
    L.pais_get_kernel_stats(ctx.h, C.byref(ks0), 1)

    def bad(cands, what, **kw):
        with pytest.raises(RuntimeError, match=what):
            ctx.pso_trace(cands, **kw)

    c = [common.copy_struct(x) for x in exp[:3]]
    c[1].num_cam = 65
    bad(c, r"candidate 1: num_cam 65")
    c = [common.copy_struct(x) for x in exp[:3]]
    c[2].cam_idx[1] = 99
    bad(c, r"candidate 2: cam_idx\[1\] = 99")
    c = [common.copy_struct(x) for x in exp[:3]]
    c[0].type = 7
    bad(c, r"candidate 0: type 7")
    bad(exp[:2], r"max_runs 0 < 1", max_runs=0)
    arr = (_lib.Candidate * 2)(*exp[:2])
    out = (_lib.PatchResult * 2)()
    it = (_lib.PsoIter * 128)()
    ri = (_lib.PsoRunInfo * 2)()
    for args, what in (((None, 2, arr, 1, out, ri, it, None), "ctx"), ((ctx.h, 2, None, 1, out, ri, it, None), "cands"),
                       ((ctx.h, 2, arr, 1, None, ri, it, None), "out"), ((ctx.h, 2, arr, 1, out, ri, None, None), "iters")):
        assert L.pais_pso_trace(*args) == -1
        assert ("null pointer (%s)" % what) in L.pais_last_error().decode()
    assert L.pais_refine_batch_open(ctx.h, 2, arr, 1) == 0
    bad(exp[:2], r"stepwise batch is open")
    view = C.POINTER(_lib.PatchResult)()
    assert L.pais_refine_batch_end(ctx.h, C.byref(view)) == 0
    # nothing launched by the rejected calls; a trace call leaves the kernel statistics alone
    assert ctx.trace_stats() == (0.0, 0, 0)
    ks = _lib.KernelStats()
    L.pais_get_kernel_stats(ctx.h, C.byref(ks), 1)
    tr = ctx.pso_trace(exp[:8], max_runs=1)
    ks2 = _lib.KernelStats()
    L.pais_get_kernel_stats(ctx.h, C.byref(ks2), 0)
    assert ks2.pso_launches == 0 and ks2.pso_evals == 0 and ks2.eval_launches == 0 and ks2.pso_patches == 0
    ms, launches, evals = ctx.trace_stats()
    assert launches > 0 and evals == sum(tr.records[i].pso_evals for i in range(8)) and ms > 0
    ctx.close()


@pytest.mark.gpu
def test_gpu_pso_trace_branches_between_arithmetics(pawn_small, workload, monkeypatch):
    """Every candidate whose records differ between the default and the literal arithmetic in pso_runs, pso_iterations or camera
    set has a first branch."""
    cfg, seeds, exp = workload
    a = _ctx(cfg, pawn_small, monkeypatch)
    b = _ctx(cfg, pawn_small, monkeypatch, literal=True)
    for cands in (seeds, exp):
        ta = a.pso_trace(cands, max_runs=8, particles=True)
        tb = b.pso_trace(cands, max_runs=8, particles=True)
        fb = ta.first_branch(tb)
        for c in range(len(cands)):
            ra, rb = ta.records[c], tb.records[c]
            if (ra.pso_runs, ra.pso_iterations, ra.cams()) != (rb.pso_runs, rb.pso_iterations, rb.cams()):
                assert fb[c] is not None, c
    a.close()
    b.close()
