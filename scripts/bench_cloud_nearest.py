"""pais_cloud_nearest measurements: kernel time and pair rate on random sets and on the full pawn
cloud against its ground truth, the 1-slice time at nq = 4096 next to the sliced one, scipy's cKDTree on the host cores as
context, and the scores of the full pawn reconstruction in both arithmetics (default and PAIS_ARITH=literal).

    python scripts/bench_cloud_nearest.py [--reps 7] [--skip-quality] [--skip-kdtree]

One warm-up call, then --reps calls; the median kernel time (hipEvents around the search and reduce kernels) is reported.
One JSON line per measurement."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from pais_mvs_amd import evaluate

FP64_VECTOR_PEAK = 78.6e12   # MI355X FP64 vector peak (flop/s, FMA counted as 2); the search uses none: its ceiling is half
FLOP_PER_PAIR = 8            # three differences, three products, two sums


def timed(q, t, reps, env=None):
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        evaluate.nearest(q[:4096], t)                # warm-up: code object, clocks
        ms = [evaluate.nearest(q, t)[2] for _ in range(reps)]
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    med = float(np.median(ms))
    pairs = float(len(q)) * float(len(t))
    return {"nq": len(q), "nt": len(t), "kernel_ms_median": med, "kernel_ms_min": float(min(ms)), "kernel_ms_max": float(max(ms)),
            "reps": reps, "pairs_per_s": pairs / (med * 1e-3), "fraction_of_fp64_vector_peak": pairs * FLOP_PER_PAIR / (med * 1e-3) / FP64_VECTOR_PEAK}


def kdtree(q, t):
    from scipy.spatial import cKDTree
    t0 = time.perf_counter()
    tree = cKDTree(t)
    t1 = time.perf_counter()
    tree.query(q, workers=16)
    t2 = time.perf_counter()
    return {"ckdtree_build_ms": (t1 - t0) * 1e3, "ckdtree_query_ms_16_workers": (t2 - t1) * 1e3}


def emit(what, d):
    print(json.dumps(dict({"what": what}, **d)), flush=True)


def pawn_cloud(scene, literal):
    from pais_mvs_amd.config import readme_config
    from pais_mvs_amd.mvs import MVS
    if literal:
        os.environ["PAIS_ARITH"] = "literal"
    else:
        os.environ.pop("PAIS_ARITH", None)
    try:
        m = MVS(readme_config(), scene.cameras, device=0, seed=42)     # bench.py's workload: R(B = 4096) to convergence
        for X, vis in scene.seeds:
            m.add_seed(X, vis)
        m.refineSeedPatches()
        m.expansionPatches(4096, 0)
        cloud, sha = m.cloud(), m.cloud_sha1()
        m.close()
    finally:
        os.environ.pop("PAIS_ARITH", None)
    return cloud, sha


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--skip-quality", action="store_true")
    ap.add_argument("--skip-kdtree", action="store_true")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    t = rng.uniform(-1, 1, size=(1000000, 3))
    q = rng.uniform(-1, 1, size=(200000, 3))
    r = timed(q, t, a.reps)
    if not a.skip_kdtree:
        r.update(kdtree(q, t))
    emit("random 2e5 x 1e6", r)
    emit("nq 4096 x 1e6, default slices", timed(q[:4096], t, a.reps))
    emit("nq 4096 x 1e6, PAIS_CLOUD_SLICES=1", timed(q[:4096], t, a.reps, {"PAIS_CLOUD_SLICES": "1"}))
    if a.skip_quality:
        return
    from pais_mvs_amd import synth
    scene = synth.pawn_scene(n_seeds=200, build_edges=False)
    pts, nrm, spacing = synth.ground_truth(scene)
    truth = np.concatenate([pts, nrm], axis=1)
    for name, literal in (("default", False), ("literal", True)):
        cloud, sha = pawn_cloud(scene, literal)
        s = evaluate.score(cloud, truth, 2 * spacing)
        emit("full pawn reconstruction, %s arithmetic" % name, dict(s, cloud_sha1=sha, spacing=spacing))
        if not literal:
            r = timed(cloud[:, :3], truth[:, :3], a.reps)
            if not a.skip_kdtree:
                r.update(kdtree(cloud[:, :3], truth[:, :3]))
            emit("pawn cloud -> truth", r)
            emit("pawn truth -> cloud", timed(truth[:, :3], cloud[:, :3], a.reps))


if __name__ == "__main__":
    main()
