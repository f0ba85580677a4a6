"""The decision thresholds and the begin-stage parameters swept through refine(), pais_ncc_batch and pais_load_state_batch.

The other sweeps (window radius, camera count, swarm size, unequal cameras) all run with the README thresholds, and those
reach few of the branches of refine(): no KEEP follow-up stage, no drop in a removal, no clamped depth range.  ROWS varies
minCamNum, minCorrelation, minRegionRatio, maxFitness, depthRangeScalar, textureVariation and minLOD / maxLOD at the
smallest shape at which every stage still runs (patchRadius 7, particleNum 6, maxIteration 8, the 12 seeds + 24 first-ring
children of tests/test_radius_sweep.py _refine_candidates).  tests/refine_paths.py tells, from the oracle alone, which
branches each candidate takes; test_rows_reach_every_branch pins that the table reaches them, so the bit-for-bit
comparisons of the GPU tests below cannot pass empty.

The first ten rows are a first census of what the thresholds reach; the next nine vary one field each.  The last rows were
searched for, each for a branch the others miss:
  pawn_small  minRegionRatio 0.6                  three records dropped by the trailing removal (one elsewhere)
  ring_small  minRegionRatio 0.8                  KEEP for 18 children at K = 7 .. 11, two more trailing drops
  pawn_small  minCamNum 1, minCorrelation 0.99    a removal leaves one camera, which setDepthRange cannot use: the setter
                                                  drop after a removal (six records)
  pawn_lowtex maxFitness 0.5                      two seeds dropped by maxFitness after their SECOND PSO run
  pawn_lowtex minLOD 20, maxFitness inf           at the top level every cost is DBL_MAX; with no limit on it the records go on
                                                  to the removal, where a warped window leaves its image (correlation == 0)
  pawn_lowtex textureVariation 2 / 400 / 1000     10 / 26 / 27 records above level 0 against 23 at 36 (5, 10 and 100 move none of them)
"""
import ctypes as C
import math

import numpy as np
import pytest

from tests import common, pipelines as P
from tests import refine_paths as RP
from tests.common import compare_patch, oracle_records

# (scene fixture, config overrides, minimum of live records: three quarters of what the oracle gives, 0 = drops only)
ROWS = (
    ("pawn_small", {}, 23),
    ("pawn_small", {"minCorrelation": 0.99}, 18),
    ("pawn_small", {"minRegionRatio": 0.7}, 13),
    ("pawn_small", {"minCamNum": 4, "minCorrelation": 0.97}, 17),
    ("pawn_small", {"minCamNum": 5}, 13),
    ("pawn_small", {"depthRangeScalar": 1e6}, 24),
    ("pawn_small", {"depthRangeScalar": 0.05}, 24),
    ("pawn_small", {"maxFitness": 1.0}, 3),
    ("pawn_lowtex", {}, 25),
    ("ring_small", {"minCorrelation": 0.98, "minRegionRatio": 0.6}, 26),
    ("pawn_small", {"minCamNum": 2}, 23),
    ("pawn_small", {"minCorrelation": -1.0, "minRegionRatio": 0.0}, 23),
    ("pawn_small", {"minRegionRatio": 0.9}, 6),
    ("pawn_lowtex", {"textureVariation": 2.0}, 25),
    ("pawn_lowtex", {"textureVariation": 400.0}, 25),
    ("pawn_lowtex", {"textureVariation": 1000.0}, 24),
    ("pawn_lowtex", {"minLOD": 1}, 25),
    ("pawn_lowtex", {"minLOD": 2, "maxLOD": 2}, 27),
    ("pawn_lowtex", {"minLOD": 20}, 0),
    ("pawn_small", {"minRegionRatio": 0.6}, 15),
    ("ring_small", {"minRegionRatio": 0.8}, 23),
    ("pawn_small", {"minCamNum": 1, "minCorrelation": 0.99}, 18),
    ("pawn_lowtex", {"maxFitness": 0.5}, 6),
    ("pawn_lowtex", {"minLOD": 20, "maxFitness": math.inf}, 0),
)
# the rows meant to consist of drops: the top pyramid level, where every cost is DBL_MAX.  (maxFitness 1.0 is meant to as well,
# but in kernel arithmetic four records have a cost below 1: it drops 32 of 36 after one run.)
DROPS_ONLY = (18, 23)
ROW_IDS = ["%d-%s-%s" % (i, s, ",".join("%s=%g" % kv for kv in sorted(o.items())) or "readme") for i, (s, o, _) in enumerate(ROWS)]

# tags of tests/refine_paths.py that no row reaches, each with what was tried
UNREACHED = (
    (RP.HEAD_DROP_SETTER, "the setters before the first run drop a record only when no camera but the reference one moves by 0.01 "
                          "pixel per unit of depth: every candidate here starts with three or more well separated cameras"),
    (RP.FINAL_AFTER2_LOD, "the PSO moves the centre along the reference camera's ray, so with the same reference camera setLOD "
                          "sees the same window: 10 textureVariation values x 3 depthRangeScalar, minLOD 1 and lodRatio 0.5 on "
                          "pawn_lowtex and 2 values on ring_small gave none"),
    (RP.LOOP_COUNT_GUARD, "needs numCam + 2 trips that each change the reference camera or remove a camera; the longest loop of any "
                          "row (lowtex, depthRangeScalar 0.01 .. 1000, minCamNum 1 / 2) has 5 trips at 5 cameras"),
    (RP.SEED_NOT_SAME, "a seed leaves its loop only when a trip changed neither the reference camera nor the camera count, which is "
                       "SAME unless the LOD alone moved or the count guard ended the loop: see those two"),
    (RP.MAXFIT_DROP[3], "maxFitness 0.5 .. 6 on the three scenes (18 values) dropped seeds after run 1 and run 2 only"),
)

# tags that must occur in at least two records over the table
TWICE = (RP.FINAL_KEEP, RP.TRAILING_DROP, RP.LOOP_DROP_MINCAM, RP.RANGE_LO_CLAMPED, RP.RANGE_HI_CAPPED)


def _cfg(over):
    from tests.test_radius_sweep import _cfg as radius_cfg
    cfg = radius_cfg(7, particleNum=6, maxIteration=8)
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg


def _scene(request, name, cfg, over):
    scene = request.getfixturevalue(name)
    if "maxLOD" in over or "lodRatio" in over:            # (OracleScene asserts that the pyramids are those of the configuration)
        from tests.mixed_rig import with_pyramids
        scene = with_pyramids(scene, cfg.lodRatio, cfg.maxLOD)
    return scene


def _oracle(cfg, scene):
    S = common.oracle_scene(cfg, scene)
    S.set_kernel_arithmetic(True)
    S.set_omp(True)
    return S


_ROW = {}


def _row(request, i):
    """Row i: scene, configuration, candidates, and per candidate the oracle's record (kernel arithmetic) and its branch tags.
    The restated record equals common.oracle_refine_patch's byte for byte, for every candidate."""
    if i in _ROW:
        return _ROW[i]
    from tests.test_radius_sweep import _refine_candidates
    name, over, min_live = ROWS[i]
    cfg = _cfg(over)
    scene = _scene(request, name, cfg, over)
    S = _oracle(cfg, scene)
    cands, is_seed = _refine_candidates(S, scene, 12)
    assert len(cands) == 36
    direct = oracle_records(S, cands, is_seed)
    want, tags = [], []
    for c, seed, d in zip(cands, is_seed, direct):
        p = common.oracle_patch_from_candidate(c)
        tags.append(RP.refine_paths(S, p, seed))
        assert RP.patch_bytes(p) == RP.patch_bytes(d), (ROW_IDS[i], c.key, sorted(tags[-1]))
        want.append(p)
    S.close()
    _ROW[i] = dict(name=name, over=over, cfg=cfg, scene=scene, cands=cands, is_seed=is_seed, want=want, tags=tags,
                   live=sum(not p.drop for p in want), min_live=min_live)
    return _ROW[i]


# ------------------------------------------------------------------------------------------------------------- CPU ---
def test_rows_reach_every_branch(request):
    """Over ROWS the oracle takes every branch refine_paths knows but those of UNREACHED -- exactly those, so a later row or
    scene that reaches one asks for its removal from the list; KEEP, the trailing drop, the loop drop and both clamps of the
    depth range at least twice; every row keeps its stated minimum of live records, and only the rows meant to drop everything do."""
    count = {}
    lod_up = {}
    for i in range(len(ROWS)):
        row = _row(request, i)
        assert row["live"] >= row["min_live"], (ROW_IDS[i], row["live"])
        if i in DROPS_ONLY:
            assert row["min_live"] == 0 and row["live"] == 0, (ROW_IDS[i], row["live"])
        else:
            assert row["min_live"] >= 3, ROW_IDS[i]
        for t in row["tags"]:
            assert t <= RP.ALL_TAGS
            for tag in t:
                count[tag] = count.get(tag, 0) + 1
        lod_up[i] = sum(RP.LOD_UP in t for t in row["tags"])
    unreached = {t for t, _ in UNREACHED}
    assert len(unreached) == len(UNREACHED) and all(why for _, why in UNREACHED)
    assert RP.ALL_TAGS - set(count) == unreached, (sorted(RP.ALL_TAGS - set(count)), sorted(unreached & set(count)))
    for tag in TWICE:
        assert count[tag] >= 2, (tag, count[tag])
    # the top level of minLOD 20: every cost is DBL_MAX, dropped by maxFitness after one run -- or, without a limit, in the removal
    assert all(t == {RP.LOD_UP, RP.RUNS[1], RP.MAXFIT_DROP[1]} for t in _row(request, 18)["tags"])
    # (a seed goes round its loop once more and is dropped at the head of that trip: its camera list was emptied by the zero table)
    assert all(t - {RP.LOOP_DROP_MINCAM} == {RP.LOD_UP, RP.RUNS[1], RP.REMOVAL_DROP_WINDOW} for t in _row(request, 23)["tags"])
    # the textureVariation rows move the LOD decision of pawn_lowtex (row 8: 36), minLOD 1 and 2 put every record above level 0
    assert lod_up[13] < lod_up[8] < lod_up[14] < lod_up[15], [lod_up[i] for i in (13, 8, 14, 15)]
    assert lod_up[16] == lod_up[17] == 36
    assert lod_up[0] == 0
    # minCorrelation -1 and minRegionRatio 0: nothing is ever removed (but a back-facing camera)
    assert not any(t & {RP.REMOVAL_DROP_FEW, RP.LOOP_DROP_MINCAM, RP.TRAILING_DROP, RP.FINAL_KEEP} for t in _row(request, 11)["tags"])


# ------------------------------------------------------------------------------------------------------------- GPU ---
def _kernel_counters(ks):
    return {n: getattr(ks, n) for n, t in ks._fields_ if t is C.c_int64}


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(ROWS)), ids=ROW_IDS)
def test_refine_every_row(request, i, monkeypatch):
    """refine_batch of the row's candidates: the default pipeline equals the oracle's records bit for bit; k_pso_eval2 + k_pso_step
    and k_pso_ring give the default's bytes; PAIS_ARITH=literal equals the oracle's costLiteral records."""
    row = _row(request, i)
    cfg, scene, cands, is_seed = row["cfg"], row["scene"], row["cands"], row["is_seed"]

    def run(env):
        return P.refine(monkeypatch, cfg, scene.cameras, cands, env)

    ref, _ = run({})
    for k, p in enumerate(row["want"]):
        compare_patch(ref[k], p, (ROW_IDS[i], "default", k, "seed" if is_seed[k] else "child", sorted(row["tags"][k])))
    assert sum(not r.dropped for r in ref) == row["live"]
    ran = any(p.psoRuns for p in row["want"])
    got, ks = run(P.EVAL2)
    assert (ks.eval2_launches > 0) == ran and ks.ring_launches == 0, (ks.eval2_launches, ks.ring_launches)
    assert bytes(got) == bytes(ref), (ROW_IDS[i], "k_pso_eval2 + k_pso_step")
    got, ks = run(P.RING)
    assert ks.ring_launches >= int(ran) and ks.ring_launches == ks.eval2_launches and ks.ring_fallbacks == 0, (
        ROW_IDS[i], ks.ring_launches, ks.eval2_launches, ks.ring_fallbacks)
    assert bytes(got) == bytes(ref), (ROW_IDS[i], "k_pso_ring")
    S = _oracle(cfg, scene)
    S.set_cost_literal(True)
    want_lit = oracle_records(S, cands, is_seed)
    S.close()
    got, _ = run(P.LITERAL)
    for k, p in enumerate(want_lit):
        compare_patch(got[k], p, (ROW_IDS[i], "literal", k, "seed" if is_seed[k] else "child"))


def _live_records(row):
    """(centre, normal, ref, lod, record cameras, candidate cameras) of the row's live oracle records."""
    return [(list(p.center[:]), list(p.normal[:]), p.refCamIdx, p.LOD, p.cams(), [int(c.cam_idx[k]) for k in range(c.num_cam)])
            for p, c in zip(row["want"], row["cands"]) if not p.drop]


@pytest.mark.gpu
def test_ncc_batch_verdicts_every_row(request):
    """pais_ncc_batch under each row's minRegionRatio / minCorrelation / minCamNum on view states of the row's live oracle
    records (with make_ncc_golden's perturbations, camera subsets and tilts): kept cameras, reasons, region ratios, correlation,
    table and drop verdict equal po_remove_invisible_camera + po_region_ratio bit for bit.  Every reason occurs."""
    from pais_mvs_amd.context import Context, make_view_state
    from tests.golden import make_ncc_golden as G
    from tests.test_ncc_batch import _compare
    reasons, drops, n_states = {}, {}, 0
    for i in range(len(ROWS)):
        row = _row(request, i)
        recs = _live_records(row)
        if not recs:
            assert i in DROPS_ONLY
            continue
        cfg, scene = row["cfg"], row["scene"]
        S = _oracle(cfg, scene)
        states = G.scene_states(S, scene, recs[:8], np.random.default_rng(4000 + i), n_search=4)
        assert len(states) >= 8, (ROW_IDS[i], len(states))
        ctx = Context(cfg, scene.cameras, device=0, seed=42)
        got = ctx.ncc_batch([make_view_state(st["center"], st["normal"], st["ref"], st["lod"], st["cams"]) for st in states], tables=True)
        ctx.close()
        for k, st in enumerate(states):
            want = G.oracle_ncc(S, st)
            _compare(got, k, want, (ROW_IDS[i], k, st["kind"]))
            drops[want["dropped"]] = drops.get(want["dropped"], 0) + 1
            if want["dropped"] != G.DROP_SAMPLE:
                for why in want["reasons"]:
                    reasons[why] = reasons.get(why, 0) + 1
        n_states += len(states)
        S.close()
    print("\n%d states, reasons %s, drops %s" % (n_states, reasons, drops))
    assert all(reasons.get(w, 0) >= 1 for w in (G.KEEP, G.REGION, G.BACKFACING, G.CORRELATION)), reasons
    assert all(drops.get(d, 0) >= 1 for d in (0, G.DROP_SAMPLE, G.DROP_MINCAM)), drops


@pytest.mark.gpu
def test_load_state_every_row(request):
    """pais_load_state_batch (k_load_state: the setters of the begin stage) under each row's configuration, on the row's live
    oracle records and its first six candidates written the way an .mvs file holds them, against po_mvs_load_patch in every
    field: the clamped depth ranges of depthRangeScalar 1e6 and the first levels of the minLOD rows among them."""
    from oracle import po
    from pais_mvs_amd.context import Context
    from tests.golden import make_resume_cloud as G
    from tests.test_resume import _assert_loader_state, _loaded
    L = po.lib()
    clamped = capped = 0
    lods = {}
    for i in range(len(ROWS)):
        row = _row(request, i)
        cfg, scene = row["cfg"], row["scene"]
        recs = [{"kind": "record", "center": list(p.center[:]), "normalS": list(p.normalS[:]), "cams": p.cams(), "fitness": p.fitness,
                 "correlation": p.correlation} for p in row["want"] if not p.drop]
        recs += [{"kind": "candidate", "center": list(c.center[:]), "normalS": list(c.normalS[:]),
                  "cams": [int(c.cam_idx[k]) for k in range(c.num_cam)], "fitness": 1.0, "correlation": 0.5} for c in row["cands"][:6]]
        S = _oracle(cfg, scene)
        ctx = Context(cfg, scene.cameras, device=0, seed=42)
        out = ctx.load_state_batch(_loaded(recs))
        ctx.close()
        mo = L.po_mvs_create(S.ptr)
        for k, r in enumerate(recs):
            p = G.oracle_load(S, mo, r)
            _assert_loader_state(out[k], p, k, ROW_IDS[i])
            by, _ = G.classify(S, p, r)
            assert bool(out[k].dropped) == (by is not None), (ROW_IDS[i], k, r["kind"], out[k].dropped, by)
            if by is None:
                clamped += int(p.depthRange[0] == 0.0)
                capped += int(p.depthRange[1] == p.depth + cfg.neighborRadius * 100)
                lods.setdefault(i, set()).add(int(p.LOD))
        L.po_mvs_destroy(mo)
        S.close()
    assert clamped >= 6 and capped >= 6, (clamped, capped)
    assert min(lods[16]) >= 1 and lods[17] == {2}, (lods[16], lods[17])                 # minLOD 1; minLOD = maxLOD = 2
    top = {c.max_lod for c in _row(request, 18)["scene"].cameras}
    assert lods[18] <= top and lods[23] <= top, (lods[18], lods[23], top)               # minLOD 20: the reference camera's top level


# the walk of test_set_config_equals_a_fresh_context: the pawn_small rows in table order (the thresholds flip from row to row)
# with the README window and swarm (patchRadius 15, particleNum 15) in the middle, so the radius and the swarm grow and shrink
def _walk():
    from pais_mvs_amd.config import readme_config
    rows = [_cfg(over) for name, over, _ in ROWS if name == "pawn_small"]
    big = readme_config(maxIteration=8)
    assert big.patchRadius == 15 and big.particleNum == 15
    return rows[:5] + [big] + rows[5:8] + [big] + rows[8:]


@pytest.mark.gpu
def test_set_config_equals_a_fresh_context(request, pawn_small):
    """One context taken through every pawn_small row with Context.set_config (pais_ctx_set_config: the Gauss table is
    reallocated, the work buffers are sized per batch) returns after each change the bytes of a context created with that
    configuration, and so does a lane forked before the first change; the lane itself and the gradient weighting on a context
    without edges are refused and leave the configuration alone, and so is a change while a batch is open."""
    from pais_mvs_amd import _lib
    from pais_mvs_amd.context import Context
    cands = _row(request, 0)["cands"]
    n = len(cands)
    arr = (_lib.Candidate * n)(*cands)
    walk = _walk()
    assert len(walk) >= 12
    ctx = Context(walk[-1], pawn_small.cameras, device=0, seed=42)
    L = ctx.L
    lane = C.c_void_p()
    assert L.pais_ctx_fork_lane(ctx.h, C.byref(lane)) == 0

    def on_lane():
        out = (_lib.PatchResult * n)()
        _lib.check(L.pais_refine_batch(lane, n, arr, out), "pais_refine_batch on the lane")
        return bytes(out)

    distinct = set()
    for step, cfg in enumerate(walk):
        ctx.set_config(cfg)
        assert ctx.cfg is cfg
        got = bytes(ctx.refine_batch(cands))
        fresh = Context(cfg, pawn_small.cameras, device=0, seed=42)
        want = bytes(fresh.refine_batch(cands))
        fresh.close()
        assert got == want, ("context", step)
        assert on_lane() == want, ("lane", step)
        distinct.add(want)
        # the lane takes no configuration of its own, and the refusal changes nothing
        c_cfg = walk[0].to_c()
        assert L.pais_ctx_set_config(lane, C.byref(c_cfg)) != 0 and b"lane" in L.pais_last_error()
        assert on_lane() == want, ("lane after its refusal", step)
    assert len(distinct) >= 8, len(distinct)                         # (the rows do give different records)
    # the gradient weighting needs the edges of create time
    last = walk[-1]
    with pytest.raises(RuntimeError, match="adaptiveGradientEnable"):
        ctx.set_config(_cfg(dict(ROWS[1][1], adaptiveGradientEnable=True)))
    assert ctx.cfg is last
    assert bytes(ctx.refine_batch(cands)) == want and on_lane() == want
    # an open batch was sized and planned with the configuration it was opened under: on the context or on its lane it bars a change
    view = C.POINTER(_lib.PatchResult)()
    for h in (ctx.h, lane):
        assert L.pais_refine_batch_begin(h, n, arr) == 0
        with pytest.raises(RuntimeError, match="a batch is open"):
            ctx.set_config(walk[0])
        assert ctx.cfg is last
        assert L.pais_refine_batch_end(h, C.byref(view)) == 0
        assert C.string_at(view, C.sizeof(_lib.PatchResult) * n) == want
    ctx.close()


REFUSED = (
    ({"minLOD": -1}, "minLOD"),
    ({"minLOD": -20}, "minLOD"),
    ({"textureVariation": 0.0}, "textureVariation"),
    ({"textureVariation": -36.0}, "textureVariation"),
    ({"textureVariation": math.nan}, "textureVariation"),
    ({"lodRatio": 0.0}, "lodRatio"),
    ({"lodRatio": 1.0}, "lodRatio"),
    ({"lodRatio": -0.8}, "lodRatio"),
    ({"lodRatio": math.nan}, "lodRatio"),
    ({"maxIteration": 0}, "maxIteration"),
    ({"maxIteration": -8}, "maxIteration"),
    ({"cellSize": 0}, "cellSize"),
    ({"cellSize": -2}, "cellSize"),
    ({"patchRadius": 0}, "patchRadius"),
    ({"patchRadius": 128}, "patchRadius"),
    ({"particleNum": 0}, "particleNum"),
    ({"maxLOD": -1}, "maxLOD"),
    ({"maxLOD": 16}, "maxLOD"),
)


@pytest.mark.gpu
def test_refused_configurations_launch_nothing(request, pawn_small):
    """Configurations that would index or divide outside their arrays on the device (set_lod from minLOD - 1, a
    textureVariation no variance is below, ...) are refused by pais_ctx_create and by Context.set_config with a message naming
    the field.  None of them gets past apply_config: the live context shows no new launch and still returns the bytes of its
    configuration."""
    from pais_mvs_amd.context import Context
    cands = _row(request, 0)["cands"]
    cfg = _cfg({})
    ctx = Context(cfg, pawn_small.cameras, device=0, seed=42)
    want = bytes(ctx.refine_batch(cands))
    before = _kernel_counters(ctx.kernel_stats())
    assert before["pso_launches"] > 0
    for over, field in REFUSED:
        bad = _cfg(over)
        with pytest.raises(RuntimeError, match=r"pais_ctx_set_config failed.*%s out of range" % field):
            ctx.set_config(bad)
        assert ctx.cfg is cfg
        with pytest.raises(RuntimeError, match=r"pais_ctx_create failed.*%s out of range" % field):
            Context(bad, pawn_small.cameras, device=0, seed=42)
    assert _kernel_counters(ctx.kernel_stats()) == before
    assert bytes(ctx.refine_batch(cands)) == want
    ctx.close()
