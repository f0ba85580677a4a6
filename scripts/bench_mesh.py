"""Mesher measurements: the field of a sampled sphere of 2e5 points on a 128^3 and a 256^3 grid
(search + merge kernels and the field kernel apart), the surface of that field (count + scans and emit apart) and the host weld,
beside pais_cloud_knn for the same pair count.

    python scripts/bench_mesh.py [--reps 3] [--grids 128,256] [--points 200000] [--k 8]

One warm-up call of each entry, then --reps calls; the median kernel time (hipEvents around the kernels) is reported, the weld as
host wall time.  One JSON line per grid."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from pais_mvs_amd import evaluate, mesh as msh


def fibonacci_sphere(n):
    i = np.arange(n) + 0.5
    z = 1.0 - 2.0 * i / n
    r = np.sqrt(1.0 - z * z)
    phi = i * (np.pi * (3.0 - np.sqrt(5.0)))
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--grids", default="128,256")
    ap.add_argument("--points", type=int, default=200000)
    ap.add_argument("--k", type=int, default=8)
    a = ap.parse_args()
    p = fibonacci_sphere(a.points)
    cloud = np.concatenate([p, p], axis=1)
    med = lambda v: float(np.median(v))
    for n in [int(v) for v in a.grids.split(",")]:
        h = 2.4 / (n - 1)
        grid = msh.Grid([-1.2 + 0.0123, -1.2 - 0.0087, -1.2 + 0.0054], h, (n, n, n))
        search, fld, count, emit, weld = [], [], [], [], []
        f = None
        for rep in range(a.reps + 1):
            f = msh.field(cloud, grid, a.k)
            ms = msh.last_ms()
            keys, xyz = msh.surface(f, grid)
            ms2 = msh.last_ms()
            t0 = time.perf_counter()
            v, t, _ = msh.weld(keys, xyz)
            dt = (time.perf_counter() - t0) * 1e3
            if rep:                                               # the first call warms up
                search.append(ms["search"]); fld.append(ms["field"]); count.append(ms2["count"]); emit.append(ms2["emit"]); weld.append(dt)
        m = msh.Mesh(v, t)
        # pais_cloud_knn for the same pair count: the grid's vertices as queries
        q = np.ascontiguousarray(np.stack(np.meshgrid(*[grid.origin[ax] + np.arange(n) * h for ax in (2, 1, 0)], indexing="ij"), axis=-1)
                                 .reshape(-1, 3)[:, ::-1])
        evaluate._knn(q, p, a.k, False, 0)
        knn = med([evaluate._knn(q, p, a.k, False, 0)[2] for _ in range(a.reps)])
        print(json.dumps({"grid": n, "points": a.points, "k": a.k, "pairs": float(n) ** 3 * a.points, "search_ms": med(search), "field_ms": med(fld),
                          "count_scan_ms": med(count), "emit_ms": med(emit), "weld_host_ms": med(weld), "knn_ms": knn,
                          "triangles": int(len(t)), "vertices": int(len(v)), "nan_share": float(np.isnan(f).mean()), "closed": m.is_closed(),
                          "volume": m.volume(), "reps": a.reps}), flush=True)


if __name__ == "__main__":
    main()
