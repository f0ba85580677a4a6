"""pais_fitness_detail throughput: the cost with its per-pixel breakdown for N evaluations per call, pawn-like (K 5, r 15)
and dome-like (K 20, r 25), each without and with the colours and homographies.  Prints one JSON line per workload:
evaluations/s of the kernel alone (HIP events around each launch) and of the whole call (upload, kernel, download, repack).

    python scripts/bench_fitness_detail.py [--evals N] [--reps R]
"""
import argparse
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from pais_mvs_amd import _lib, synth
from pais_mvs_amd.config import readme_config
from pais_mvs_amd.context import Context


def states_of(scene, K):
    """One state per seed that sees at least K cameras: the seed's first K cameras, the first as reference, LOD 0; its
    particle: the normal facing the reference camera at the seed's depth."""
    states, parts = [], []
    for X, vis in scene.seeds:
        if len(vis) < K:
            continue
        ref = scene.cameras[vis[0]]
        ray = np.asarray(X, float) - np.asarray(ref.center, float)
        depth = float(np.linalg.norm(ray))
        s = _lib.PatchState()
        s.ray[:] = (ray / depth).tolist()
        s.ref_cam, s.lod, s.num_cam = int(vis[0]), 0, K
        for i, c in enumerate(vis[:K]):
            s.cam_idx[i] = int(c)
        n = -ray / depth
        states.append(s)
        parts.append([math.acos(float(n[2])), math.atan2(float(n[1]), float(n[0])), depth])
    return states, parts


def run(name, scene, cfg, K, n, reps, colours):
    states, base = states_of(scene, K)
    if not states:
        raise SystemExit("%s: no seed sees %d cameras" % (name, K))
    rng = np.random.default_rng(0)
    idx = [i % len(states) for i in range(n)]
    parts = np.array([base[i] for i in idx]) + rng.normal(0, [0.02, 0.02, 0.002], (n, 3))   # particles around each patch
    ctx = Context(cfg, scene.cameras, device=0, seed=42)
    d = ctx.fitness_detail(states, idx[:256], parts[:256], colours, colours)  # warm-up (buffers, code object)
    ctx.detail_stats(reset=True)
    t0 = time.perf_counter()
    for _ in range(reps):
        d = ctx.fitness_detail(states, idx, parts, colours, colours)
    wall = (time.perf_counter() - t0) / reps
    ms, launches, ne = ctx.detail_stats(reset=True)
    ctx.close()
    kms = ms / reps
    return {"workload": name, "evals": n, "K": K, "patch_radius": cfg.patchRadius, "colours_and_H": bool(colours),
            "distinct_states": len(states), "launches_per_call": launches // reps, "kernel_ms": round(kms, 3),
            "kernel_evals_per_s": round(n / (kms * 1e-3), 1) if kms > 0 else None, "call_ms": round(wall * 1e3, 3),
            "call_evals_per_s": round(n / wall, 1), "finite_fraction": round(float(np.mean(d.outcome == 0)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--evals", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    pawn = synth.pawn_scene(width=640, height=480, n_seeds=200, build_edges=False)
    dome = synth.dome_scene(n_cams=40, width=400, height=300, focal=420.0, radius=4.0, n_seeds=200, build_edges=False)
    for colours in (False, True):
        print(json.dumps(run("pawn_like", pawn, readme_config(), 5, a.evals, a.reps, colours)), flush=True)
        print(json.dumps(run("dome_like", dome, readme_config(patchRadius=25, distWeighting=25 / 3.0), 20, a.evals, a.reps, colours)),
              flush=True)


if __name__ == "__main__":
    main()
