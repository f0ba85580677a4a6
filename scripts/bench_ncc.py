"""pais_ncc_batch throughput: removeInvisibleCamera of 100k given states per call, pawn-like (K 5, r 15: warped patches in
LDS) and dome-like (K 20, r 25: warped patches in the per-workgroup scratch slabs).  Prints one JSON line per workload:
states/s of the kernel alone (HIP events around the launch) and of the whole call (upload, kernel, download).

    python scripts/bench_ncc.py [--states N] [--reps R]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from pais_mvs_amd import synth
from pais_mvs_amd.config import readme_config
from pais_mvs_amd.context import Context, make_view_state


def states_of(scene, K):
    """One state per seed that sees at least K cameras: the seed's first K cameras, the first as reference, the normal
    facing it."""
    out = []
    for X, vis in scene.seeds:
        if len(vis) < K:
            continue
        ref = scene.cameras[vis[0]]
        n = np.asarray(ref.center, float) - np.asarray(X, float)
        out.append(make_view_state(X, n / np.linalg.norm(n), vis[0], 0, vis[:K]))
    return out


def run(name, scene, cfg, K, n, reps):
    base = states_of(scene, K)
    if not base:
        raise SystemExit("%s: no seed sees %d cameras" % (name, K))
    states = [base[i % len(base)] for i in range(n)]
    ctx = Context(cfg, scene.cameras, device=0, seed=42)
    res = ctx.ncc_batch(states[: min(n, 4096)])  # warm-up (buffers, code object)
    ctx.ncc_stats(reset=True)
    t0 = time.perf_counter()
    for _ in range(reps):
        res = ctx.ncc_batch(states)
    wall = (time.perf_counter() - t0) / reps
    ms, launches, nst = ctx.ncc_stats(reset=True)
    ctx.close()
    kms = ms / max(launches, 1)
    return {"workload": name, "states": n, "K": K, "patch_radius": cfg.patchRadius, "distinct_states": len(base),
            "kernel_ms": round(kms, 3), "kernel_states_per_s": round(n / (kms * 1e-3), 1) if kms > 0 else None,
            "call_ms": round(wall * 1e3, 3), "call_states_per_s": round(n / wall, 1),
            "dropped_fraction": round(float(np.mean(res.dropped != 0)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--states", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    pawn = synth.pawn_scene(width=640, height=480, n_seeds=200, build_edges=False)
    print(json.dumps(run("pawn_like", pawn, readme_config(), 5, a.states, a.reps)), flush=True)
    dome = synth.dome_scene(n_cams=40, width=400, height=300, focal=420.0, radius=4.0, n_seeds=200, build_edges=False)
    print(json.dumps(run("dome_like", dome, readme_config(patchRadius=25), 20, a.states, a.reps)), flush=True)


if __name__ == "__main__":
    main()
