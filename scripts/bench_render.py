"""pais_cloud_render measurements: kernel time, covered (pixel, splat) pairs per second and atomics
issued for
  (a) the truth samples of the pawn scene at stride 2, rho = spacing, into its 5 cameras at 640 x 480, DISC -- with the time of
      the numpy restatement (tests/test_render_gpu.py: _brute) on the host cores beside it, as context only;
  (b) 10^6 random splats with footprints of 1 .. 40 pixels into 8 views at 1920 x 1080, DISC and POINT;
  (c) one splat covering the whole frame next to 10^5 small ones: the bounded-tile rule.

    python scripts/bench_render.py [--reps 7] [--skip-numpy] [--only a|b|c]

One warm-up call, then --reps calls; the median kernel time (hipEvents from the fill kernel to the last kernel of each pass of
views, without the copies) is reported.  One JSON line per measurement."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from pais_mvs_amd import render as rnd


def timed(reps, *args, **kw):
    rnd.render(*args, **kw)                      # warm-up: code object, clocks
    rs = [rnd.render(*args, **kw) for _ in range(reps)]
    ms = [r.kernel_ms for r in rs]
    med = float(np.median(ms))
    c = rs[-1].counts
    return {"kernel_ms_median": med, "kernel_ms_min": float(min(ms)), "kernel_ms_max": float(max(ms)), "reps": reps,
            "covered_pairs": c["covered_pairs"], "covered_pairs_per_s": c["covered_pairs"] / (med * 1e-3), "tiles": c["tiles"],
            "depth_atomics": c["depth_atomics"], "id_atomics": c["id_atomics"], "covered_pixels": int((rs[-1].id >= 0).sum())}


def emit(what, d):
    print(json.dumps(dict({"what": what}, **d)), flush=True)


def case_a(reps, skip_numpy):
    from pais_mvs_amd import synth
    scene = synth.pawn_scene(n_seeds=8, build_edges=False)
    pts, nrm, spacing = synth.ground_truth(scene, stride=2)
    views = [rnd.view_of(c) for c in scene.cameras]
    r = timed(reps, pts, nrm, views, 640, 480, radius=spacing)
    r.update(n=len(pts), views=5, width=640, height=480, rho=spacing)
    if not skip_numpy:
        from tests.test_render_gpu import CULL, DISC, _brute
        t0 = time.perf_counter()
        _brute(DISC, CULL, pts, nrm, spacing, views, 640, 480)
        r["numpy_restatement_ms"] = (time.perf_counter() - t0) * 1e3
    emit("(a) pawn truth, stride 2, 5 cameras 640x480, DISC", r)


def random_views(rng, V, W, H, focal, dist):
    out = []
    for _ in range(V):
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        out.append(rnd.look_at_view(dist * d, np.zeros(3), np.array([0.0, 0.0, 1.0]), focal, W, H))
    return out


def case_b(reps):
    rng = np.random.default_rng(0)
    n, W, H, focal, dist = 1000000, 1920, 1080, 1500.0, 4.0
    c = rng.uniform(-1, 1, size=(n, 3))
    nr = rng.normal(size=(n, 3))
    nr /= np.linalg.norm(nr, axis=1, keepdims=True)
    # footprints of 1 .. 40 pixels across at the centre's distance: rho = pixels / 2 x dist / focal
    rho = rng.uniform(1, 40, size=n) * 0.5 * dist / focal
    views = random_views(rng, 8, W, H, focal, dist)
    r = timed(reps, c, nr, views, W, H, radii=rho)
    r.update(n=n, views=8, width=W, height=H)
    emit("(b) 1e6 random splats, footprints 1..40 px, 8 views 1920x1080, DISC", r)
    for size in (1, 5):
        r = timed(reps, c, None, views, W, H, mode="point", radius=size)
        r.update(n=n, views=8, width=W, height=H, size=size)
        emit("(b) 1e6 random splats, 8 views 1920x1080, POINT size %d" % size, r)


def case_c(reps):
    rng = np.random.default_rng(1)
    n, W, H, focal = 100000, 1920, 1080, 1500.0
    view = rnd.make_view(np.eye(3), np.zeros(3), (focal, focal), (float(W >> 1), float(H >> 1)))
    c = np.concatenate([[[0.0, 0.0, 6.0]], rng.uniform(-1, 1, size=(n, 3)) * np.array([2.0, 1.2, 1.0]) + np.array([0.0, 0.0, 4.0])])
    nr = np.tile([0.0, 0.0, -1.0], (n + 1, 1))
    rho = np.concatenate([[5.5], np.full(n, 0.008)])     # the first covers every pixel of the frame, behind the others
    r = timed(reps, c, nr, [view], W, H, radii=rho)
    r.update(n=n + 1, views=1, width=W, height=H)
    emit("(c) one whole-frame splat + 1e5 small ones, 1 view 1920x1080, DISC", r)
    r = timed(reps, c[1:], nr[1:], [view], W, H, radii=rho[1:])
    r.update(n=n, views=1, width=W, height=H)
    emit("(c) the 1e5 small ones alone", r)
    r = timed(reps, c[:1], nr[:1], [view], W, H, radii=rho[:1])
    r.update(n=1, views=1, width=W, height=H)
    emit("(c) the whole-frame splat alone", r)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--skip-numpy", action="store_true")
    ap.add_argument("--only", choices=["a", "b", "c"])
    a = ap.parse_args()
    if a.only in (None, "c"):
        case_c(a.reps)
    if a.only in (None, "b"):
        case_b(a.reps)
    if a.only in (None, "a"):
        case_a(a.reps, a.skip_numpy)


if __name__ == "__main__":
    main()
