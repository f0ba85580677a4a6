"""pais_mesh_render measurements: kernel milliseconds per view of setup, depth phase and id phase,
covered (pixel, triangle) pairs and how many (triangle, view) pairs took the packed walk, for
  (a) the truth samples of the pawn scene at stride 2 meshed at the pitch of their spacing, into its 5 cameras at 640 x 480 --
      with the DISC render of the same samples at rho = spacing beside it (scripts/bench_render.py (a));
  (b) a bumpy latitude-longitude sphere of about 10^6 triangles a few pixels across into 8 views at 1920 x 1080.

    python scripts/bench_mesh_render.py [--reps 7] [--only a|b]

One warm-up call, then --reps calls; medians are reported.  One JSON line per measurement.  With PAIS_LIB_PATH naming a
library built with -DRENDER_PACK_MAX=0 every box takes the tile walk: the other side of the packed-versus-tile comparison."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from pais_mvs_amd import render as rnd


def timed(reps, ver, tri, views, W, H):
    rnd.render_mesh(ver, tri, views, W, H)      # warm-up: code object, clocks
    total, phases = [], []
    for _ in range(reps):
        r = rnd.render_mesh(ver, tri, views, W, H)
        total.append(r.kernel_ms)
        phases.append(rnd.mesh_last_ms())
    V = len(views)
    c = r.counts
    out = {"kernel_ms_median": float(np.median(total)), "kernel_ms_min": float(min(total)), "kernel_ms_max": float(max(total)), "reps": reps,
           "kernel_ms_per_view": float(np.median(total)) / V, "triangles": int(len(tri)), "vertices": int(len(ver)), "views": V, "width": W,
           "height": H, "covered_pairs": c["covered_pairs"], "tiles": c["tiles"], "packed": c["packed"], "depth_atomics": c["depth_atomics"],
           "id_atomics": c["id_atomics"], "covered_pixels": int((r.id >= 0).sum())}
    for k in ("setup", "depth", "id"):
        out[k + "_ms_per_view"] = float(np.median([p[k] for p in phases])) / V
    return out


def emit(what, d):
    print(json.dumps(dict({"what": what}, **d)), flush=True)


def case_a(reps):
    from pais_mvs_amd import mesh as msh
    from pais_mvs_amd import synth
    scene = synth.pawn_scene(n_seeds=8, build_edges=False)
    pts, nrm, spacing = synth.ground_truth(scene, stride=2)
    views = [rnd.view_of(c) for c in scene.cameras]
    m = msh.mesh(np.concatenate([pts, nrm], axis=1), h=spacing)
    r = timed(reps, m.vertices, m.triangles, views, 640, 480)
    r.update(points=len(pts), pitch=spacing)
    emit("(a) pawn truth mesh, stride 2, pitch = spacing, 5 cameras 640x480", r)
    rnd.render(pts, nrm, views, 640, 480, radius=spacing)
    ms = [rnd.render(pts, nrm, views, 640, 480, radius=spacing).kernel_ms for _ in range(reps)]
    emit("(a) the same samples as discs, rho = spacing (BASELINE section 11 (a))",
         {"kernel_ms_median": float(np.median(ms)), "kernel_ms_per_view": float(np.median(ms)) / 5, "n": len(pts), "reps": reps})


def bumpy_sphere(rows, cols):
    """a welded latitude-longitude sphere of 2 cols (rows - 1) triangles, radius 1 +- 0.05, wound outward"""
    th = np.linspace(0.0, np.pi, rows + 1)[1:-1]
    ph = np.linspace(0.0, 2.0 * np.pi, cols, endpoint=False)
    T, P = np.meshgrid(th, ph, indexing="ij")
    rad = 1.0 + 0.05 * np.sin(5.0 * T) * np.cos(7.0 * P)
    ring = np.stack([rad * np.sin(T) * np.cos(P), rad * np.sin(T) * np.sin(P), rad * np.cos(T)], axis=-1).reshape(-1, 3)
    ver = np.concatenate([ring, [[0.0, 0.0, 1.0], [0.0, 0.0, -1.0]]])
    i, j = np.meshgrid(np.arange(rows - 2), np.arange(cols), indexing="ij")
    a, b = i * cols + j, i * cols + (j + 1) % cols
    c, d = a + cols, b + cols
    quads = np.concatenate([np.stack([a, c, b], axis=-1).reshape(-1, 3), np.stack([b, c, d], axis=-1).reshape(-1, 3)])
    j = np.arange(cols)
    north, south = len(ring), len(ring) + 1
    last = (rows - 2) * cols
    caps = np.concatenate([np.stack([np.full(cols, north), j, (j + 1) % cols], axis=-1),
                           np.stack([np.full(cols, south), last + (j + 1) % cols, last + j], axis=-1)])
    return ver, np.concatenate([quads, caps]).astype(np.int32)


def case_b(reps):
    from scripts.bench_render import random_views
    rng = np.random.default_rng(0)
    W, H, focal, dist = 1920, 1080, 1500.0, 4.0
    ver, tri = bumpy_sphere(708, 708)
    r = timed(reps, ver, tri, random_views(rng, 8, W, H, focal, dist), W, H)
    emit("(b) bumpy sphere of 1e6 triangles, 8 views 1920x1080", r)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", choices=["a", "b"])
    a = ap.parse_args()
    if a.only in (None, "a"):
        case_a(a.reps)
    if a.only in (None, "b"):
        case_b(a.reps)


if __name__ == "__main__":
    main()
