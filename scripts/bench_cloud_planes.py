"""pais_cloud_planes measurements: the search + merge kernels and the fit kernel of a cloud against itself
(PAIS_KNN_SKIP_SAME_INDEX | PAIS_PLANE_WITH_QUERY) at n = 1e4, 1e5 and 3e5, k = 8 and 16, beside pais_cloud_knn on the same points.

    python scripts/bench_cloud_planes.py [--reps 5] [--sizes 10000,100000,300000] [--knn-only]

One warm-up call of each entry, then --reps calls; the median kernel time (hipEvents around the kernels) is reported.  One JSON
line per measurement.  --knn-only measures pais_cloud_knn alone and needs nothing of pais_cloud_planes: run it on the parent
commit for the comparison of the shared search."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from pais_mvs_amd import evaluate

KS = (8, 16)


def median3(values):
    return float(np.median(values)), float(min(values)), float(max(values))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="10000,100000,300000")
    ap.add_argument("--knn-only", action="store_true")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    # a noisy surface, as a cloud is: a unit sphere with 1 % radial noise
    p = rng.normal(size=(max(int(v) for v in a.sizes.split(",")), 3))
    p *= (1.0 + 0.01 * rng.normal(size=(len(p), 1))) / np.linalg.norm(p, axis=1, keepdims=True)
    for n in [int(v) for v in a.sizes.split(",")]:
        s = np.ascontiguousarray(p[:n])
        for k in KS:
            evaluate._knn(s, s, k, True, 0)
            med, lo, hi = median3([evaluate._knn(s, s, k, True, 0)[2] for _ in range(a.reps)])
            print(json.dumps({"entry": "pais_cloud_knn", "n": n, "k": k, "kernel_ms_median": med, "kernel_ms_min": lo, "kernel_ms_max": hi,
                              "reps": a.reps}), flush=True)
            if a.knn_only:
                continue
            evaluate.planes(s, k, table=False)
            ms = np.array([evaluate.planes(s, k, table=False)["kernel_ms"] for _ in range(a.reps)])
            search, fit = median3(ms[:, 0]), median3(ms[:, 1])
            print(json.dumps({"entry": "pais_cloud_planes", "n": n, "k": k, "search_ms_median": search[0], "search_ms_min": search[1],
                              "search_ms_max": search[2], "fit_ms_median": fit[0], "fit_ms_min": fit[1], "fit_ms_max": fit[2],
                              "fit_over_search": fit[0] / search[0], "search_over_knn": search[0] / med, "reps": a.reps}), flush=True)


if __name__ == "__main__":
    main()
