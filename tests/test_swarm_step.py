"""The swarm step (pso_step_wave, pais_kernels.hip) at every boundary of its lane layout.

The step keeps a swarm of N <= 64 particles in the lanes of its wave and moves it with 4 (N <= 16), 2 (N <= 32) or 1 lane per
particle; larger swarms take the serial LDS form.  An expansion candidate runs particleNum particles, a seed twice as many, so
the particle counts below put N on both sides of every change of layout (16 | 17, 32 | 33 | 34, 64 | 66), below, at and above
localK = 5, and at 1.  For each count the records of refine_batch must be the same bytes in the three PSO pipelines
(k_pso_iter: a step replay per evaluation wave; k_pso_eval2 + k_pso_step; k_pso_ring) and the traced rows -- the swarm
k_pso_step_trace leaves after every fitness update -- must be the oracle's bit for bit.

Swarms a scene rarely produces (ties of every distance, divisions by zero, all fitness values DBL_MAX, NaN and +inf fitness,
a swarm pinned on a range bound) go through pais_test_swarm_step (include/pais_test_hooks.h): one step of the GPU's wave against
the serial statements compiled for the host (tests/swarm_step_shim.cpp), byte for byte.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import common, pipelines as P
from tests.test_pso_trace import _check_oracle_parity, _oracle_runs

PARTICLES = [1, 2, 3, 4, 5, 6, 15, 16, 17, 31, 32, 33]


def _cfg(particles):
    from pais_mvs_amd.config import readme_config
    return readme_config(patchRadius=4, distWeighting=4 / 3.0, particleNum=particles, maxIteration=6)


@pytest.fixture(scope="module")
def candidates(pawn_small):
    """24 seed candidates and 36 expansion candidates beside refined seeds (the same for every particle count)."""
    from pais_mvs_amd.context import make_candidate
    cfg = _cfg(15)
    S = common.oracle_scene(cfg, pawn_small)
    _, seeds = common.seed_candidates(S, pawn_small)
    S.close()
    ctx = P.context(cfg, pawn_small.cameras)
    kept = [r for r in ctx.refine_batch(seeds) if not r.dropped]
    ctx.close()
    assert len(kept) >= 6
    exp = []
    for i, r in enumerate(kept[:12]):
        for j in range(3):
            cen = [r.center[0] + 0.002 * (j - 1), r.center[1] + 0.001 * j, r.center[2] - 0.001 * j]
            exp.append(make_candidate(cen, list(r.normal[:]), [r.cam_idx[k] for k in range(r.num_cam)], 9000 + 7 * i + j, 1,
                                      normalS=list(r.normalS[:])))
    return seeds[:24], exp


def _run(cfg, scene, cands, env, monkeypatch):
    res, ks = P.refine(monkeypatch, cfg, scene.cameras, cands, env)
    assert sum(1 for r in res if r.pso_evals > 0 and not r.dropped) >= 3     # (the step ran, and some runs ended in a patch)
    return bytes(res), ks


@pytest.mark.gpu
@pytest.mark.parametrize("particles", PARTICLES)
def test_records_are_the_same_bytes_in_every_pipeline(pawn_small, candidates, monkeypatch, particles):
    cfg = _cfg(particles)
    seeds, exp = candidates
    for cands, n_swarm, ring_env in ((exp, particles, P.RING_SMALL_BATCH), (seeds, 2 * particles, P.SEED_RING)):
        ref, ks0 = _run(cfg, pawn_small, cands, P.ITER, monkeypatch)     # small batch: k_pso_iter while N <= 64
        P.assert_took("iter", ks0, (particles, n_swarm))
        split, ks1 = _run(cfg, pawn_small, cands, P.EVAL2, monkeypatch)
        P.assert_took("eval2", ks1, (particles, n_swarm))
        assert split == ref, ("k_pso_eval2 + k_pso_step", particles, n_swarm)
        ring, ks2 = _run(cfg, pawn_small, cands, ring_env, monkeypatch)
        assert ks2.ring_fallbacks == 0
        if n_swarm <= 64:       # (a ring pass needs the swarm's tasks in the lanes of one wave; beyond, the launches per iteration run)
            assert ks2.ring_launches >= 1 and ks2.ring_evals > 0, (particles, n_swarm)
        assert ring == ref, ("k_pso_ring", particles, n_swarm)


@pytest.mark.gpu
@pytest.mark.parametrize("particles", PARTICLES)
def test_traced_rows_are_the_oracles(pawn_small, candidates, monkeypatch, particles):
    """The rows of k_pso_step_trace against the oracle's trace.  With the trace sink the step takes the SERIAL convergence sums (it
    records their values), so this test does not run the DPP convergence means of the lane form (swarm_mean_below); those are
    checked against an independent reference by the degenerate-swarm test below (its converged swarms against the host shim) and
    by the oracle parity of the untraced pipelines in tests/test_gpu_parity.py -- the three pipelines share them, so the byte
    comparison across pipelines above could not see a fault in them."""
    cfg = _cfg(particles)
    seeds, exp = candidates
    ctx = P.context(cfg, pawn_small.cameras, monkeypatch, {})
    for cands, is_seed in ((seeds[:8], True), (exp[:12], False)):
        tr = ctx.pso_trace(cands, max_runs=8, particles=True)
        oracle = _oracle_runs(cfg, pawn_small, cands, is_seed)
        assert any(len(runs) > 0 and runs[0]["iterations"] >= 1 for _, runs in oracle)
        bad = _check_oracle_parity(tr, oracle, "kernel")
        assert bad is None, (particles, is_seed, bad)
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# degenerate swarms: one step of the wave against the serial statements on the host
# ---------------------------------------------------------------------------------------------------------------------
HERE = os.path.dirname(os.path.abspath(__file__))
DBL_MAX = float(np.finfo(np.float64).max)
LO, HI = np.array([0.5, -1.0, 2.0]), np.array([1.5, 1.0, 4.0])


class TestSwarm(C.Structure):
    """pais_test_swarm (include/pais_test_hooks.h)."""
    __test__ = False
    _fields_ = [("range_l", C.c_double * 3), ("range_u", C.c_double * 3), ("iw", C.c_double), ("gbest_fitness", C.c_double),
                ("stream_base", C.c_uint64), ("n", C.c_int32), ("max_iteration", C.c_int32), ("iteration", C.c_int32),
                ("g_idx", C.c_int32), ("started", C.c_int32), ("run", C.c_int32), ("local_k", C.c_int32), ("continues", C.c_int32),
                ("result", C.c_double * 4)]


def _shim_sources():
    return [os.path.join(HERE, "swarm_step_shim.cpp")], [os.path.join(HERE, "..", "include", "pais_test_hooks.h"),
                                                          os.path.join(HERE, "..", "pais_mvs_amd", "csrc", "pais_dev.hpp")]


@pytest.fixture(scope="module")
def shim():
    bdir = os.path.join(HERE, "build")
    os.makedirs(bdir, exist_ok=True)
    so = os.path.join(bdir, "libswarm_step_shim.so")
    src, deps = _shim_sources()
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in src + deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", so] + src)
    S = C.CDLL(so)
    S.shim_swarm_step.argtypes = [C.POINTER(TestSwarm), C.POINTER(C.c_double)]
    return S


def test_shim_is_clean_under_the_sanitizers():
    """The host statements the GPU is compared with, in a stand-alone program built with -fsanitize=address,undefined."""
    bdir = os.path.join(HERE, "build")
    os.makedirs(bdir, exist_ok=True)
    exe = os.path.join(bdir, "swarm_step_shim_asan")
    src, _ = _shim_sources()
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe] + src + [os.path.join(HERE, "swarm_step_shim_main.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("steps"), (out.returncode, out.stdout[-300:], out.stderr[-2000:])


def _base(rng, N):
    """A swarm in the middle of a run: rows {pos, vec, pBest, nBest, fit, pBestFit}."""
    sw = np.zeros((N, 14))
    sw[:, 0:3] = LO + (HI - LO) * rng.random((N, 3))
    sw[:, 3:6] = 0.2 * (rng.random((N, 3)) - 0.5)
    sw[:, 6:9] = LO + (HI - LO) * rng.random((N, 3))
    sw[:, 9:12] = LO + (HI - LO) * rng.random((N, 3))
    sw[:, 12] = 5.0 * rng.random(N)
    sw[:, 13] = 5.0 * rng.random(N)
    return sw


def _degenerate(rng, N):
    """(name, swarm) of the cases of the issue at swarm size N."""
    out = []
    out.append(("random", _base(rng, N)))
    sw = _base(rng, N); sw[:, 6:9] = 0.5 * (LO + HI); sw[:, 12] = 9.0                 # (no fitness update: the pBests stay equal)
    out.append(("all pBest equal: every distance ties", sw))
    sw = sw.copy(); sw[:, 0:3] = sw[:, 6:9]
    out.append(("all pBest equal and every particle on it: every FDR divides by zero", sw))
    sw = sw.copy(); sw[:, 13] = 1.0
    out.append(("... and every pBestFitness equal: 0 / 0", sw))
    if N >= 4:
        sw = _base(rng, N); sw[3, 6:9] = sw[1, 6:9]; sw[3, 13] = sw[1, 13]; sw[[1, 3], 12] = 9.0
        out.append(("two particles with the same pBest and pBestFitness", sw))
    sw = _base(rng, N); sw[:, 12] = DBL_MAX; sw[:, 13] = DBL_MAX
    out.append(("every fitness DBL_MAX", sw))
    if N >= 2:
        sw = _base(rng, N); sw[:, 7] = sw[0, 1]; sw[:, 12] = 9.0
        out.append(("pos[0][1] == pBest[j][1] for every j, in that dimension only", sw))
    sw = _base(rng, N); sw[:, 0:3] = HI; sw[:, 6:9] = HI; sw[:, 9:12] = HI; sw[:, 3:6] = np.abs(sw[:, 3:6]) + 5.0
    out.append(("all particles clamped on the upper bound", sw))
    sw = _base(rng, N); sw[:, 0:3] = LO; sw[:, 3:6] = -5.0
    out.append(("all positions on the lower bound, velocities outward", sw))
    sw = _base(rng, N); sw[:, 0:3] = sw[0, 6:9]; sw[:, 6:9] = sw[0, 6:9]; sw[:, 3:6] *= 1e-3; sw[:, 12] = 9.0
    out.append(("converged: the run ends", sw))
    # non-finite fitness: a cost is F / W, NaN when the weights of all live pixels vanish (tests/test_weight_sweep.py)
    nan, inf = float("nan"), float("inf")
    sw = _base(rng, N); sw[0, 12] = nan; sw[0, 13] = nan
    out.append(("particle 0's fitness NaN: gBest starts on a NaN and no <= ever moves it", sw))
    sw = _base(rng, N); sw[:, 12] = nan; sw[:, 13] = nan
    out.append(("every fitness NaN", sw))
    sw = _base(rng, N); sw[(1 if N > 1 else 0)::3, 12] = nan
    out.append(("NaN fitness among finite ones, every pBestFitness finite", sw))
    sw = _base(rng, N); sw[(1 if N > 1 else 0)::2, 13] = nan; sw[:, 12] = 0.5 * sw[:, 12]
    out.append(("some pBestFitness NaN: fit < NaN never improves it", sw))
    sw = _base(rng, N); sw[0, 13] = nan
    out.append(("the gBest particle's pBestFitness NaN at a later step", sw))
    sw = _base(rng, N); sw[::2, 12] = inf
    out.append(("+inf fitness among finite ones", sw))
    sw = _base(rng, N); sw[:, 12] = inf; sw[:, 13] = inf
    out.append(("every fitness +inf", sw))
    sw = _base(rng, N); sw[:, 6:9] = 0.5 * (LO + HI); sw[:, 12] = 9.0; sw[(1 if N > 1 else 0)::2, 12] = nan
    out.append(("all pBest equal: every distance ties, NaN fitness among them", sw))
    return out


def _serial_gbest(pbf):
    """updateGbest from particle 0 (psosolver.cpp:137-149): gBest = particles[0], then `<=` over the swarm -- the last index of
    the minimum, and particle 0 for good when its pBestFitness is NaN."""
    g, gf = 0, float(pbf[0])
    for j in range(len(pbf)):
        if pbf[j] <= gf:
            g, gf = j, float(pbf[j])
    return g, gf


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 2, 4, 5, 6, 15, 16, 17, 31, 32, 33, 64, 65, 80])
def test_degenerate_swarms_move_as_the_serial_statements(shim, N):
    from pais_mvs_amd import _lib
    L = _lib.load()
    L.pais_test_swarm_step.argtypes = [C.c_int, C.POINTER(TestSwarm), C.POINTER(C.c_double)]
    rng = np.random.default_rng(100 + N)
    moved = ended = 0
    for name, sw0 in _degenerate(rng, N):
        for started, iteration, max_it in ((0, 0, 30), (1, 2, 30), (1, 28, 30), (1, 29, 30)):   # first step, later steps, the last iteration
            def fresh():
                s = TestSwarm()
                s.range_l[:], s.range_u[:] = list(LO), list(HI)
                s.iw, s.n, s.max_iteration, s.iteration, s.started = 0.7, N, max_it, iteration, started
                s.run, s.local_k, s.stream_base = 1, min(N, 5), 0x9E3779B97F4A7C15 ^ (N * 1000003)
                s.g_idx, s.gbest_fitness = _serial_gbest(sw0[:, 13])
                return s, np.ascontiguousarray(sw0.copy())
            gs, gsw = fresh()
            hs, hsw = fresh()
            rc = L.pais_test_swarm_step(0, C.byref(gs), gsw.ctypes.data_as(C.POINTER(C.c_double)))
            assert rc == 0, (name, rc)
            assert shim.shim_swarm_step(C.byref(hs), hsw.ctypes.data_as(C.POINTER(C.c_double))) == 0
            what = (N, name, started, iteration)
            assert gs.continues == hs.continues, what
            assert gsw.tobytes() == hsw.tobytes(), (what, np.argwhere(gsw.view(np.uint64) != hsw.view(np.uint64))[:6].tolist())
            assert bytes(gs) == bytes(hs), (what, gs.iteration, hs.iteration, gs.g_idx, hs.g_idx, gs.gbest_fitness, hs.gbest_fitness,
                                            list(gs.result), list(hs.result))
            if not hs.continues:
                assert hsw.tobytes() == sw0.tobytes()
                ended += 1
            else:
                assert hs.started == 1 and hs.iteration == (iteration + 1 if started else 0)
                moved += 1
    assert moved >= 10 and ended >= 4
