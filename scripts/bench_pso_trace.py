"""pais_pso_trace cost: candidates/s of refine_batch, of pso_trace with headers only (run info + one row per iteration) and of
pso_trace with particles (11 doubles per particle and iteration), plus the kernel time of the trace's PSO iterations (HIP events
around each pass: evaluation + k_pso_step_trace launches).  Two workloads on the bench scene (pawn, README config): the seeds, and
the expansion candidates of an early round (the stepwise scheduler with the GPU's own records).  One JSON line per workload.

    python scripts/bench_pso_trace.py [--seeds S] [--round R] [--reps N]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pais_mvs_amd import _lib, synth
from pais_mvs_amd.config import readme_config
from pais_mvs_amd.context import Context
from pais_mvs_amd.mvs import MVS


def copy_struct(x):
    y = type(x)()
    C.memmove(C.byref(y), C.byref(x), C.sizeof(type(x)))
    return y


def workloads(cfg, scene, round_no, B=4096):
    """(seed candidates, expansion candidates of round `round_no`); cfg comes back with the reconstruction's neighbour radius."""
    m = MVS(cfg, scene.cameras, device=0, seed=42)
    for X, vis in scene.seeds:
        m.add_seed(X, vis)
    L = m.L
    L.pais_refine_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    cands, n = m.seed_begin()
    seeds = [copy_struct(cands[i]) for i in range(n)]
    out = (_lib.PatchResult * max(n, 1))()
    assert L.pais_refine_batch(m.ctx_handle, n, cands, out) == 0
    m.seed_commit(out, n)
    m.expansion_begin()
    exp, rnd = [], 0
    while not exp:
        done, cands, n = m.round_begin(B)
        if done:
            break
        out = (_lib.PatchResult * max(n, 1))()
        if n:
            assert L.pais_refine_batch(m.ctx_handle, n, cands, out) == 0
            if rnd >= round_no:
                exp = [copy_struct(cands[i]) for i in range(n)]
        m.round_commit(out, n)
        rnd += 1
    cfg.neighborRadius = m.neighbor_radius()
    m.expansion_end()
    m.close()
    return seeds, exp


def timed(fn, reps):
    fn()                                       # warm-up: buffers, code objects
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps


def run(name, ctx, cands, reps):
    n = len(cands)
    t_ref = timed(lambda: ctx.refine_batch(cands), reps)
    ctx.trace_stats(reset=True)
    t_hdr = timed(lambda: ctx.pso_trace(cands, max_runs=4), reps)
    ms_hdr, launches, evals = ctx.trace_stats(reset=True)
    t_par = timed(lambda: ctx.pso_trace(cands, max_runs=4, particles=True), reps)
    ms_par, _, _ = ctx.trace_stats(reset=True)
    tr = ctx.pso_trace(cands, max_runs=4, particles=True)
    rows = sum(tr.rows(c, r) for c in range(n) for r in range(tr.runs(c)))
    per = reps + 1                             # (timed() runs the warm-up call too)
    return {"workload": name, "candidates": n, "rows_per_run": int(tr.iters.shape[2]), "particles_per_row": int(tr.particles.shape[3]),
            "recorded_rows": rows, "particle_bytes": int(tr.particles.nbytes),
            "refine_batch_cand_per_s": round(n / t_ref, 1), "trace_headers_cand_per_s": round(n / t_hdr, 1),
            "trace_particles_cand_per_s": round(n / t_par, 1),
            "trace_headers_kernel_ms": round(ms_hdr / per, 3), "trace_particles_kernel_ms": round(ms_par / per, 3),
            "step_trace_launches_per_call": launches // per, "evals_per_call": evals // per}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=200)
    ap.add_argument("--round", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    cfg = readme_config()
    scene = synth.pawn_scene(n_seeds=a.seeds, build_edges=False)      # bench.py's default workload
    seeds, exp = workloads(cfg, scene, a.round)
    ctx = Context(cfg, scene.cameras, device=0, seed=42)
    print(json.dumps(run("pawn_seeds", ctx, seeds, a.reps)), flush=True)
    print(json.dumps(run("pawn_round_%d_expansion" % a.round, ctx, exp, a.reps)), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
