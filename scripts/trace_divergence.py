"""Where do the default arithmetic and PAIS_ARITH=literal part ways?  A sample of the bench workload's expansion candidates
(rounds 5..25, every n/160-th candidate of a round: the sample of the literal gate in tests/test_gpu_parity.py) is traced in
both arithmetics (two contexts) by pais_pso_trace, and PsoTrace.first_branch gives each candidate's first (run, row) of a
different discrete trajectory.  Prints one JSON line: how many candidates branch, how many differ in their records, and the
histogram of the first branch's (run, row).

    python scripts/trace_divergence.py [--seeds S] [--per-round P]
"""
import argparse
import collections
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pais_mvs_amd import _lib, synth
from pais_mvs_amd.config import readme_config
from pais_mvs_amd.context import Context
from pais_mvs_amd.mvs import MVS


def copy_struct(x):
    y = type(x)()
    C.memmove(C.byref(y), C.byref(x), C.sizeof(type(x)))
    return y


def sample(cfg, scene, per_round, rounds=(5, 25), B=4096):
    m = MVS(cfg, scene.cameras, device=0, seed=42)
    for X, vis in scene.seeds:
        m.add_seed(X, vis)
    m.refineSeedPatches()
    m.expansion_begin()
    L = m.L
    L.pais_refine_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    kept, rnd = [], 0
    while True:
        done, cands, n = m.round_begin(B)
        if done:
            break
        out = (_lib.PatchResult * max(n, 1))()
        if n:
            assert L.pais_refine_batch(m.ctx_handle, n, cands, out) == 0
            if rounds[0] <= rnd <= rounds[1]:
                kept += [copy_struct(cands[i]) for i in range(0, n, max(1, n // per_round))]
        m.round_commit(out, n)
        rnd += 1
    cfg.neighborRadius = m.neighbor_radius()
    m.expansion_end()
    m.close()
    return kept


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=200)
    ap.add_argument("--per-round", type=int, default=160)
    a = ap.parse_args()
    cfg = readme_config()
    scene = synth.pawn_scene(n_seeds=a.seeds, build_edges=False)      # bench.py's default workload
    cands = sample(cfg, scene, a.per_round)
    os.environ.pop("PAIS_ARITH", None)
    ctx = Context(cfg, scene.cameras, device=0, seed=42)
    os.environ["PAIS_ARITH"] = "literal"
    lit = Context(cfg, scene.cameras, device=0, seed=42)
    os.environ.pop("PAIS_ARITH")
    ta = ctx.pso_trace(cands, max_runs=1, particles=True)
    tb = lit.pso_trace(cands, max_runs=1, particles=True)
    fb = ta.first_branch(tb)
    hist = collections.Counter(f for f in fb if f is not None)
    rec_diff = sum(1 for c in range(len(cands)) if (ta.records[c].pso_runs, ta.records[c].pso_iterations, ta.records[c].cams()) !=
                   (tb.records[c].pso_runs, tb.records[c].pso_iterations, tb.records[c].cams()))
    rec_diff_unbranched = sum(1 for c in range(len(cands)) if fb[c] is None and
                              (ta.records[c].pso_runs, ta.records[c].pso_iterations, ta.records[c].cams()) !=
                              (tb.records[c].pso_runs, tb.records[c].pso_iterations, tb.records[c].cams()))
    traced = sum(1 for c in range(len(cands)) if ta.runs(c))
    rows = sorted(hist.items(), key=lambda kv: kv[0])
    print(json.dumps({"candidates": len(cands), "traced": traced, "branched": sum(hist.values()),
                      "records_differ": rec_diff, "records_differ_without_branch": rec_diff_unbranched,
                      "first_branch_row_quartiles": _quartiles([t for (_, t) in hist.elements()]),
                      "first_branch_histogram": {"%d:%d" % k: v for k, v in rows}}), flush=True)
    ctx.close()
    lit.close()


def _quartiles(v):
    if not v:
        return None
    v = sorted(v)
    return [v[len(v) // 4], v[len(v) // 2], v[(3 * len(v)) // 4], v[-1]]


if __name__ == "__main__":
    main()
