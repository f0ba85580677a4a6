"""pais_feature_detect measurements:
  (a) kernel ms per stage (blur, extrema, fit, orientation, descriptor) for a 640 x 480 and a 1920 x 1080 image -- the pawn
      scene's first camera rendered at that size --, and the bytes per second the blur kernels achieve, counted as the
      ALGORITHMIC traffic (each pass reads its input once and writes its output once; doubling and halving likewise);
  (b) MVS.seed_from_images(3.0) on the full pawn scene (5 cameras, 640 x 480): keypoints, seeds, and the median distance of
      the seeds to the true surface (synth.ground_truth, numpy brute force).

    python scripts/bench_features.py [--reps 7] [--only a|b]

One warm-up call, then --reps calls; medians are reported.  The stage times are hipEvent intervals around each stage's
launches, summed over the octaves, without the host round trips between stages.  One JSON line per measurement."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from pais_mvs_amd import features


def emit(what, d):
    print(json.dumps(dict({"what": what}, **d)), flush=True)


def case_a(reps):
    from pais_mvs_amd import synth
    for w, h in ((640, 480), (1920, 1080)):
        scene = synth.pawn_scene(width=w, height=h, n_seeds=8, build_edges=False)
        g = np.ascontiguousarray(scene.cameras[0].image)
        features.detect_full(g)                                    # warm-up: code object, clocks
        stages, wall = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            out = features.detect_full(g, first=1 << 16)
            wall.append((time.perf_counter() - t0) * 1e3)
            stages.append(features.last_stage_ms())
        med = {k: float(np.median([s[k] for s in stages])) for k in stages[0]}
        r = {"width": w, "height": h, "keypoints": len(out[0]), "reps": reps, "wall_ms_median": float(np.median(wall))}
        r.update({k + "_ms": v for k, v in med.items() if k != "blur_bytes"})
        r["kernel_ms"] = sum(v for k, v in med.items() if k != "blur_bytes")
        r["blur_bytes"] = med["blur_bytes"]
        r["blur_bytes_per_s"] = med["blur_bytes"] / (med["blur"] * 1e-3)
        emit("(a) detect, pawn camera 0 at %d x %d" % (w, h), r)


def case_b():
    from pais_mvs_amd import synth
    from pais_mvs_amd.config import readme_config
    from pais_mvs_amd.mvs import MVS
    scene = synth.pawn_scene(n_seeds=60)
    m = MVS(readme_config(), scene.cameras, device=0, seed=42)
    t0 = time.perf_counter()
    n = m.seed_from_images(3.0)
    dt = time.perf_counter() - t0
    cen = np.array([list(p.center[:]) for p in m.patches()]).reshape(-1, 3)
    m.close()
    gt, _, spacing = synth.ground_truth(scene)
    dist = np.array([np.sqrt(((gt - c) ** 2).sum(axis=1).min()) for c in cen]) if n else np.zeros(0)
    kp = [len(features.detect(np.ascontiguousarray(c.image))[0]) for c in scene.cameras]
    emit("(b) seed_from_images(3.0), pawn_full", {"keypoints_per_camera": kp, "seeds": n, "seconds": dt,
                                                  "median_seed_to_surface": float(np.median(dist)) if n else None,
                                                  "truth_spacing": spacing})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", choices=["a", "b"])
    a = ap.parse_args()
    if a.only in (None, "a"):
        case_a(a.reps)
    if a.only in (None, "b"):
        case_b()


if __name__ == "__main__":
    main()
