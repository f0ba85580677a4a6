"""pais_cloud_visibility measurements: the fused entry with and without the maps copied down, against
pais_cloud_render followed by pais_depth_test through the host, the cloud tested against itself (PAIS_VIS_SELF, tol = radius).

    python scripts/bench_visibility.py --case pawn  [--reps 7]     the small pawn truth (stride 2) into its five 320 x 240 cameras
    python scripts/bench_visibility.py --case large [--reps 7]     300 000 points of a noisy unit sphere into 8 orbit views of 1280 x 960

Run each case as its own command, under its own time limit.  One warm-up call of each path, then --reps calls; the median, minimum
and maximum of the wall time of the whole call (uploads, kernels, copies back) and of the kernel times (hipEvents around the
kernels) are reported, one JSON line per path."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from pais_mvs_amd import render as rnd


def stats(values):
    return {"median": float(np.median(values)), "min": float(min(values)), "max": float(max(values))}


def case(name):
    if name == "pawn":
        from pais_mvs_amd import synth
        scene = synth.pawn_scene(width=320, height=240, n_seeds=24)
        pts, nrm, spacing = synth.ground_truth(scene, stride=2)
        cam = scene.cameras[0]
        return pts, nrm, [rnd.view_of(c) for c in scene.cameras], cam.width, cam.height, spacing
    rng = np.random.default_rng(0)
    n = 300000
    nrm = rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    pts = nrm * (1.0 + 0.002 * rng.normal(size=(n, 1)))
    W, H = 1280, 960
    return pts, nrm, rnd.orbit_views(pts, 8, 1400.0, W, H), W, H, 1.5 * math_pitch(n)


def math_pitch(n):
    """the pitch of n samples spread evenly over the unit sphere"""
    return float(np.sqrt(4.0 * np.pi / n))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["pawn", "large"], required=True)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    pts, nrm, views, W, H, radius = case(a.case)
    base = {"case": a.case, "n": len(pts), "views": len(views), "width": W, "height": H, "radius": radius, "reps": a.reps}

    def fused(keep):
        t0 = time.perf_counter()
        v = rnd.visibility(pts, nrm, views, W, H, radius=radius, keep_maps=keep, occluder=False, margin=False)
        return (time.perf_counter() - t0) * 1e3, v.ms["render"], v.ms["test"], v.code

    def two_steps():
        t0 = time.perf_counter()
        r = rnd.render(pts, nrm, views, W, H, radius=radius)
        v = rnd.depth_test(pts, views, r.depth, r.id, tol=radius, self_index=True, occluder=False, margin=False)
        return (time.perf_counter() - t0) * 1e3, r.kernel_ms, v.kernel_ms, v.code

    codes = []
    for name, fn in (("pais_cloud_visibility, maps stay on the device", lambda: fused(False)),
                     ("pais_cloud_visibility, maps copied down", lambda: fused(True)),
                     ("pais_cloud_render + pais_depth_test through the host", two_steps)):
        fn()
        runs = [fn() for _ in range(a.reps)]
        codes.append(runs[-1][3])
        print(json.dumps(dict(base, path=name, wall_ms=stats([r[0] for r in runs]), render_kernel_ms=stats([r[1] for r in runs]),
                              test_kernel_ms=stats([r[2] for r in runs]))), flush=True)
    assert all(c.tobytes() == codes[0].tobytes() for c in codes), "the three paths disagree"
    print(json.dumps(dict(base, code_histogram=[int((codes[0] == k).sum()) for k in range(6)])), flush=True)


if __name__ == "__main__":
    main()
