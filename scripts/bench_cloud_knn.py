"""pais_cloud_knn measurements: kernel time for k = 1, 8, 32 beside pais_cloud_nearest on the same
point sets -- (a) 2e5 points against themselves, (b) 4096 queries against 1e6 targets at the default slice count and at
PAIS_CLOUD_SLICES=1 -- and, with --slices, the slice counts in between on set (b).

    python scripts/bench_cloud_knn.py [--reps 5] [--slices 2,4,8,16,32]

One warm-up call of each entry, then --reps calls; the median kernel time (hipEvents around the search and merge kernels) is
reported with its ratio to pais_cloud_nearest's median under the same split settings.  One JSON line per measurement."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from pais_mvs_amd import evaluate

KS = (1, 8, 32)


def median_ms(call, reps):
    call()                                       # warm-up: code object, clocks
    ms = [call() for _ in range(reps)]
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def measure(what, q, t, reps, env=None, skip_self=False):
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        base = median_ms(lambda: evaluate.nearest(q, t)[2], reps)
        print(json.dumps({"what": what, "entry": "pais_cloud_nearest", "nq": len(q), "nt": len(t), "env": env or {},
                          "kernel_ms_median": base[0], "kernel_ms_min": base[1], "kernel_ms_max": base[2], "reps": reps}), flush=True)
        for k in KS:
            r = median_ms(lambda: evaluate._knn(q, t, k, skip_self, 0)[2], reps)
            print(json.dumps({"what": what, "entry": "pais_cloud_knn", "k": k, "skip_self": skip_self, "nq": len(q), "nt": len(t),
                              "env": env or {}, "kernel_ms_median": r[0], "kernel_ms_min": r[1], "kernel_ms_max": r[2], "reps": reps,
                              "ratio_to_nearest": r[0] / base[0]}), flush=True)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--slices", default="", help="comma-separated PAIS_CLOUD_SLICES values to add on set (b)")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    t = rng.uniform(-1, 1, size=(1000000, 3))
    s = np.ascontiguousarray(t[:200000])
    measure("(a) 2e5 against itself", s, s, a.reps)
    measure("(b) 4096 x 1e6, default slices", s[:4096], t, a.reps)
    measure("(b) 4096 x 1e6, PAIS_CLOUD_SLICES=1", s[:4096], t, a.reps, {"PAIS_CLOUD_SLICES": "1"})
    for n in [int(v) for v in a.slices.split(",") if v]:
        measure("(b) 4096 x 1e6, PAIS_CLOUD_SLICES=%d" % n, s[:4096], t, a.reps, {"PAIS_CLOUD_SLICES": str(n)})


if __name__ == "__main__":
    main()
