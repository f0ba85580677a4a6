"""k_pso_ring with a PART of an evaluation as its task (2 or 4 waves per evaluation): the same records as the per-iteration pass.

A ring task (candidate, part, particle) walks the 64-pixel window steps part, part + P, ... and delivers the canonical
sub-accumulators of those steps; the wave that completes a candidate's N * P arrivals adds them ((a0 + a1) + a2) + a3 in the swarm
step.  Nothing of that may show in a record: every test here compares bytes with the pipeline that takes one launch per iteration.

The scene is the small pawn with camera CROP cut off a few pixels above the window of one refined seed, so that the batch holds
what the part waves can get wrong:
  * patches seen by 3 cameras (M = 2: one pair of taps per trip), by 4 (M = 3: the triple) and by 5;
  * candidates whose swarm straddles an image border -- the oracle's cost is finite for some positions of the search range and
    DBL_MAX for others that are finite while CROP keeps its whole image; the border is the TOP of CROP's image, so the taps that
    leave it belong to the first window rows, i.e. to step 0 alone: with several parts the whole-call DBL_MAX is raised by part 0
    only and the other parts deliver sums;
  * candidates whose reference window holds masked (zero) pixels beside counted ones;
  * window radii 3 (49 pixels: one step -- parts 1 .. 3 have none), 5 (121 pixels: two steps -- parts 2 and 3 of 4 have none) and
    15 (961 pixels: sixteen steps, the last one a single pixel).
"""
import ctypes as C

import numpy as np
import pytest

from tests import common, pipelines as P, refcost

CROP = 1                      # the camera whose image is cut
PARTS = (1, 2, 4)
_BATCH = {}


def _cfg(r):
    from pais_mvs_amd.config import readme_config
    return readme_config(patchRadius=r, distWeighting=r / 3.0)


def _cropped(scene, cfg, y0):
    """The scene with rows [0, y0) of camera CROP's image cut away (principal point moved with them)."""
    from pais_mvs_amd import synth
    from pais_mvs_amd.camera import Camera
    cams = []
    for i, c in enumerate(scene.cameras):
        cut = y0 if i == CROP else 0
        pp = c.principle_point.copy()
        pp[1] -= cut
        cams.append(Camera(focal=c.focal.copy(), principle_point=pp, quaternion=c.quaternion.copy(), center=c.center.copy(),
                           image=np.ascontiguousarray(c.image[cut:]), name=c.name).finalize(cfg.lodRatio, cfg.maxLOD, True))
    return synth.Scene(scene.name + "_cut", cams, scene.obj, scene.seeds)


def _refined_seeds(cfg, scene):
    S = common.oracle_scene(cfg, scene)
    S.set_kernel_arithmetic(True)
    _, seeds = common.seed_candidates(S, scene)
    pats = common.oracle_refine_many(S, seeds, True, threads=16)
    return S, seeds, [p for p in pats if not p.drop]


def _expansion(kept):
    """Four candidates around every refined seed: its cameras, the first three, the first four, its cameras again."""
    from pais_mvs_amd.context import make_candidate
    cands = []
    for i, p in enumerate(kept):
        cams = p.cams()
        for j in range(4):
            cen = [p.center[0] + 0.002 * (j - 1.5), p.center[1] + 0.001 * j, p.center[2] - 0.001 * j]
            use = cams[:3] if j == 1 else (cams[:4] if j == 2 else cams)
            cands.append(make_candidate(cen, list(p.normal[:]), use, 7000 + 11 * i + j, 1, normalS=list(p.normalS[:])))
    return cands


def _batch(pawn_small, r):
    """(cfg, scene, candidates, seeds, certificates) for window radius r; built once."""
    if r in _BATCH:
        return _BATCH[r]
    cfg = _cfg(r)
    # where camera CROP is cut: a few pixels above the radius-15 window of a refined seed that it sees without being its reference
    cfg15 = _cfg(15)
    S0, _, kept0 = _refined_seeds(cfg15, pawn_small)
    S0.close()
    pick = next(p for p in kept0 if CROP in p.cams() and p.refCamIdx != CROP and p.LOD == 0)
    v = refcost.project(pawn_small.cameras[CROP], list(pick.center[:]), 1.0)[1]
    scene = _cropped(pawn_small, cfg, int(round(v)) - 15 - 4)
    S, seeds, kept = _refined_seeds(cfg, scene)
    assert len(kept) >= 10, len(kept)
    cands = _expansion(kept)
    # certificates, from the oracle alone: refine the candidates, then look at each one's search range and reference window
    pats = common.oracle_refine_many(S, cands, False, threads=16)
    Sfull = common.oracle_scene(cfg, pawn_small)                         # the same cameras with CROP's whole image
    Sfull.set_kernel_arithmetic(True)
    rng = np.random.default_rng(77)
    straddle, masked, ncams = [], [], set()
    for k, p in enumerate(pats):
        if p.psoEvals <= 0:
            continue
        ncams.add(cands[k].num_cam)
        cam = scene.cameras[p.refCamIdx]
        u, w = refcost.project(cam, list(p.center[:]), cfg.lodRatio ** p.LOD)
        img = cam.pyramid[p.LOD]
        win = img[max(int(w) - r, 0):int(w) + r + 1, max(int(u) - r, 0):int(u) + r + 1]
        if (win == 0).any() and (win != 0).any():
            masked.append(k)
        if p.drop or CROP not in p.cams() or p.refCamIdx == CROP:
            continue
        half = np.pi / cfg.reduceNormalRange
        # positions of its search range: finite with CROP's whole image, and with the cut image finite for some, DBL_MAX for others
        vals = []
        for _ in range(24):
            pos = [p.normalS[0] + rng.uniform(-half, half), p.normalS[1] + rng.uniform(-half, half),
                   rng.uniform(p.depthRange[0], p.depthRange[1])]
            if Sfull.fitness(p, pos) < common.DBL_MAX:
                vals.append(S.fitness(p, pos))
        if any(x == common.DBL_MAX for x in vals) and any(x < common.DBL_MAX for x in vals):
            straddle.append(k)
    S.close()
    Sfull.close()
    _BATCH[r] = (cfg, scene, cands, seeds, dict(straddle=straddle, masked=masked, ncams=ncams))
    return _BATCH[r]


def _refine(monkeypatch, cfg, scene, cands, env, parts=0):
    """P.refine with the ring's waves per evaluation forced to `parts` (pais_test_set_ring_parts; 0: the library's choice).
    The ring launches of the run must then all be launches of that many waves per evaluation (pais_test_ring_parts_launches):
    a pass that fell back to one wave per evaluation would give the same bytes and prove nothing."""
    with P.knobs(monkeypatch, env):
        c = P.context(cfg, scene.cameras)
        assert c.L.pais_test_set_ring_parts(c.h, C.c_int(parts), C.c_double(0.0)) == 0
        out = c.refine_batch(cands)
        ks = c.kernel_stats()
        by_parts = (C.c_int64 * 3)()
        assert c.L.pais_test_ring_parts_launches(c.h, by_parts) == 0
        c.close()
    if parts:
        want = [ks.ring_launches if p == parts else 0 for p in PARTS]
        assert list(by_parts) == want, (parts, list(by_parts), ks.ring_launches)
    return out, ks


def _records(monkeypatch, cfg, scene, cands, env, parts=0):
    out, ks = _refine(monkeypatch, cfg, scene, cands, env, parts)
    return bytes(out), ks


def _ring(**more):
    return dict(P.RING_SMALL_BATCH, **more)


def test_the_batch_holds_what_a_part_wave_can_get_wrong(pawn_small):
    """The certificates of the module docstring for the radius-15 batch and its first 3 and 9 candidates' camera counts (no GPU)."""
    _, _, cands, _, cert = _batch(pawn_small, 15)
    assert len(cands) >= 40
    assert {3, 4} <= cert["ncams"], cert["ncams"]                        # M = 2 (one pair) and M = 3 (the triple)
    assert {c.num_cam for c in cands[:3]} >= {3, 4} or {c.num_cam for c in cands[:9]} >= {3, 4}
    assert cert["straddle"] and min(cert["straddle"]) < 40, cert["straddle"]   # finite and DBL_MAX evaluations in one swarm
    assert cert["masked"] and min(cert["masked"]) < 40, cert["masked"]


@pytest.mark.gpu
@pytest.mark.parametrize("pre", ["records", "no records"])
@pytest.mark.parametrize("parts", PARTS)
def test_part_ring_pass_is_the_launch_per_iteration_pass(pawn_small, monkeypatch, parts, pre):
    """Batches of 3, 9 and 40 expansion candidates through the ring with `parts` waves per evaluation, the set-up records
    (pais_pre.hpp) on and off, against PAIS_PSO_RING=0: the same bytes; one ring launch, no re-run."""
    cfg, scene, cands, _, _ = _batch(pawn_small, 15)
    extra = {} if pre == "records" else P.NO_PRE
    for n in (3, 9, 40):
        key = ("ref", 15, n)
        if key not in _BATCH:
            _BATCH[key] = _records(monkeypatch, cfg, scene, cands[:n], P.ITER)[0]
        got, ks = _records(monkeypatch, cfg, scene, cands[:n], _ring(**extra), parts)
        assert ks.ring_launches == 1 and ks.ring_fallbacks == 0 and ks.eval2_launches == 1, (n, ks.ring_launches, ks.ring_fallbacks)
        assert got == _BATCH[key], (parts, pre, n)


@pytest.mark.gpu
@pytest.mark.parametrize("r", [3, 5, 15])
def test_parts_without_a_step_deliver_zeros(pawn_small, monkeypatch, r):
    """Window radii whose step count does not divide by the parts: 49 pixels are one step, 121 are two, 961 are sixteen with a
    lone last pixel.  A part that has no step must deliver zero sub-accumulators (not what an earlier iteration left in its
    slots): the records are those of the per-iteration pass for 1, 2 and 4 parts."""
    cfg, scene, cands, _, _ = _batch(pawn_small, r)
    cands = cands[:40]
    ref, _ = _records(monkeypatch, cfg, scene, cands, P.ITER)
    for parts in PARTS:
        got, ks = _records(monkeypatch, cfg, scene, cands, _ring(), parts)
        assert ks.ring_launches == 1 and ks.ring_fallbacks == 0, (r, parts, ks.ring_launches, ks.ring_fallbacks)
        assert got == ref, (r, parts)


@pytest.mark.gpu
@pytest.mark.parametrize("parts", [2, 4])
def test_seed_batch_through_the_part_ring(pawn_small, monkeypatch, parts):
    """A seed batch (2 x particleNum particles, several dependent passes) with every pass as a part-ring launch equals the
    default pipeline."""
    cfg, scene, _, seeds, _ = _batch(pawn_small, 15)
    ref, ks0 = _records(monkeypatch, cfg, scene, seeds, {})
    got, ks = _records(monkeypatch, cfg, scene, seeds, P.SEED_RING, parts)
    assert ks0.ring_launches == 0 and ks.ring_launches >= 2 and ks.ring_fallbacks == 0, (ks.ring_launches, ks.ring_fallbacks)
    assert got == ref


@pytest.mark.gpu
def test_failed_part_pass_is_rerun_by_the_existing_path(pawn_small, monkeypatch):
    """A ring pass of 4 parts that does not complete (no patience: the first wave that waits raises the error word) is re-run
    through the per-iteration launches: the same records, one ring_fallbacks."""
    cfg, scene, cands, _, _ = _batch(pawn_small, 15)
    cands = cands[:40]
    ref, _ = _records(monkeypatch, cfg, scene, cands, P.ITER)
    got, ks = _records(monkeypatch, cfg, scene, cands, _ring(**P.NO_PATIENCE), 4)
    assert ks.ring_fallbacks == 1 and ks.eval2_launches > 10, (ks.ring_fallbacks, ks.eval2_launches)
    assert got == ref


@pytest.mark.gpu
def test_evaluations_are_counted_once_per_evaluation(pawn_small, monkeypatch):
    """ring_evals of a pass is the number of evaluations, whatever the number of waves that share one."""
    cfg, scene, cands, _, _ = _batch(pawn_small, 15)
    counts = {}
    for parts in PARTS:
        out, ks = _refine(monkeypatch, cfg, scene, cands[:40], _ring(), parts)
        counts[parts] = (ks.ring_evals, ks.eval2_evals, sum(r.pso_evals for r in out))
    assert counts[1][0] > 0 and counts[1][0] == counts[1][2], counts
    assert counts[1] == counts[2] == counts[4], counts
