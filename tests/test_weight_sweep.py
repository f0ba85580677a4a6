"""The three scales of the adaptive pixel weight -- diffWeighting, gradientWeighting, distWeighting -- swept through the cost and
the PSO, against the oracle AND against tests/refcost.py.

Every other test runs diffWeighting = 16384 = 2^14, gradientWeighting = 10 and distWeighting = r / 3 or 5.  Three things depend
on exactly those values:
  * the kernels multiply -(sad * sad) by 1.0 / diffWeighting where the reference divides: the same bits for a power of two, a
    last-bit difference of the exp argument otherwise (rows 10000, 100);
  * with the README values the exp argument stays in about [-4, 0]: det_exp_poly's guard, its scaling into the denormals and its
    exact 0 below -746 are reached only with small scales (rows 16, 1.0, 0.05, 1e-3 and the gradient rows);
  * a cost is F / W, NaN when the weights of all live pixels vanish: the NaN branches of the swarm step (swarm_update_gbest,
    pso_move_own, the lexicographic arg-mins, the quad forms of pso_move_lanes, the serial form for N > 64) see a NaN fitness
    only in the rows 1.0, 0.05, 1e-3, gradient 0.007 / 0.005 / 1e-3 and the combined row.
All rows at r = 4 (81 pixels: one full 64-pixel step and a partial one) on the small pawn; the refine rows also on the small dome
(K > 12: the tile kernel).

An evaluation is compared only where refcost's margin is at least 1e-7 AND its sum of weights is not made of denormals
(refcost.denormal_sum: two correct multiplication orders of the three factors may differ there by more than any gate); both
kinds of skips are counted and bounded by 5 % of a row.

Measured on the CPU (144 evaluations per row; worst relative error against refcost of the oracle's literal cost, its
costLiteral and its kernel arithmetic; the gates are 1.9e-14, 1.9e-14 and 1e-9):

  row               finite DBL_MAX  NaN  skipped (margin + denormal)          literal costLiteral      kernel
  base                93      51    0   0 + 0                         1.3e-15   1.3e-15     1.5e-13
  diff_10000          93      51    0   0 + 0                         8.6e-16   8.3e-16     1.6e-13
  diff_100            93      51    0   0 + 0                         1.1e-15   1.1e-15     9.6e-14
  diff_16             93      51    0   0 + 0                         1.1e-15   1.1e-15     7.2e-13
  diff_1              88      51    5   0 + 0                         8.0e-16   8.0e-16     7.3e-13
  diff_0.05           77      51   16   0 + 0                         5.5e-16   5.5e-16     8.4e-13
  diff_1e-3           61      51   32   0 + 0                         2.1e-16   2.1e-16     2.3e-12
  diff_1e300          93      51    0   0 + 0                         9.5e-16   9.5e-16     1.7e-13
  grad_1e6            93      51    0   0 + 0                         1.2e-15   1.2e-15     1.6e-13
  grad_0.007          62      51   31   0 + 0                         2.5e-16   2.5e-16     3.8e-14
  grad_0.005          54      51   39   0 + 0                         2.5e-16   2.5e-16     3.5e-14
  grad_1e-3            0      51   93   0 + 0                         0.0e+00   0.0e+00     0.0e+00
  dist_0.3            93      51    0   0 + 0                         5.0e-16   5.0e-16     7.6e-13
  dist_0.05           93      51    0   0 + 0                         0.0e+00   1.4e-16     7.9e-13
  dist_1e6            93      51    0   0 + 0                         1.2e-15   1.2e-15     7.8e-14
  diff_1_grad_0.03    85      51    6   0 + 2                         4.8e-16   4.8e-16     5.8e-12

The 1e300 row equals adaptiveDifferenceEnable = False bit for bit (exp(-sad^2 / 1e300) is exactly 1.0).  The distWeighting 1e6
half of that check is dropped: the Gaussian table is normalised to sum 1, so at distWeighting 1e6 it holds 1 / 81 to eleven
digits and not 1.0, and the quotient F / W of weights scaled so is not the quotient of the unscaled ones bit for bit
(test_flat_distance_table_is_not_exactly_one pins the reason and compares the costs to 1e-10).

The gradient rows 0.007 and 0.005 and the combined row's 0.03 stand where gradientWeighting 0.01, 0.003 and 0.01 were first
meant: on these windows the largest gradient weight of a candidate is exp(-1 / (e * gradientWeighting)) with e about 0.137 or
0.155, so that 0.01 and 0.003 put the sums of weights of 8 to 16 of 144 evaluations between 1e-319 and 1e-281, below the 2^-900
of the denormal rule -- more than its 5 %.  At 0.007 and 0.005 those sums are exactly 0 or far above it (no skip), with 31 and 39
NaN costs beside 62 and 54 finite ones.  The gradient weight depends on the reference pixel alone and the window centre lies on
the candidate's ray, so in a gradient row the costs of a swarm are all NaN (or DBL_MAX) or none is: its mixed rows hold NaN
beside DBL_MAX, those of the diffWeighting rows NaN beside costs.

Swarm rows of the oracle's refine trace (36 candidates, particleNum 6, maxIteration 8) that hold both a NaN and a finite fitness:
  diff_1      pawn: alive 26 of 36, swarm rows 496, with NaN and finite 309 (308 of them with a cost below DBL_MAX), NaN particles  611 / 4800
  diff_0.05   pawn: alive 24 of 36, swarm rows 608, with NaN and finite 495 (471 of them with a cost below DBL_MAX), NaN particles 1539 / 6144
  diff_1e-3   pawn: alive 32 of 36, swarm rows 512, with NaN and finite 491 (426 of them with a cost below DBL_MAX), NaN particles 2671 / 4992
  grad_0.005  pawn: alive 24 of 36, swarm rows 432, with NaN and finite 240 (  0 of them with a cost below DBL_MAX), NaN particles 1787 / 4032
  base        pawn: alive 35 of 36, swarm rows 640, with NaN and finite   0 (  0 of them with a cost below DBL_MAX), NaN particles    0 / 6528
  base        dome: alive 24 of 24, swarm rows 368, with NaN and finite   0 (  0 of them with a cost below DBL_MAX), NaN particles    0 / 3648
  diff_1      dome: alive 18 of 24, swarm rows 480, with NaN and finite 210 (210 of them with a cost below DBL_MAX), NaN particles  440 / 4992
  grad_0.007  dome: alive 24 of 24, swarm rows 288, with NaN and finite 110 (  0 of them with a cost below DBL_MAX), NaN particles 1640 / 2688
"""
import math

import numpy as np
import pytest

from tests import common, pipelines as P, refcost
from tests.common import compare_patch, oracle_records
from tests.refcost import check_against_refcost, denormal_sum
from tests.test_radius_sweep import _det_normal, _refine_candidates

R = 4
RTOL_KERNEL = 1e-9          # the kernel arithmetic against refcost (tests/test_radius_sweep.py)
DBL_MAX = refcost.DBL_MAX
GRAD = {"adaptiveGradientEnable": True}
ROWS = (
    ("base", dict(GRAD)),                                            # the control: all three switches on, README values
    ("diff_10000", {"diffWeighting": 10000.0}),                      # not a power of two
    ("diff_100", {"diffWeighting": 100.0}),
    ("diff_16", {"diffWeighting": 16.0}),                            # arguments pass -700 and -746 for sad above about 106
    ("diff_1", {"diffWeighting": 1.0}),                              # vanishing weights, NaN costs
    ("diff_0.05", {"diffWeighting": 0.05}),
    ("diff_1e-3", {"diffWeighting": 1e-3}),
    ("diff_1e300", {"diffWeighting": 1e300}),                        # every difference weight exactly 1.0
    ("grad_1e6", dict(GRAD, gradientWeighting=1e6)),                 # weights near 1
    ("grad_0.007", dict(GRAD, gradientWeighting=0.007)),             # partly NaN
    ("grad_0.005", dict(GRAD, gradientWeighting=0.005)),
    ("grad_1e-3", dict(GRAD, gradientWeighting=1e-3)),               # e <= 1: argument <= -1000, every weight exactly 0
    ("dist_0.3", {"distWeighting": 0.3}),
    ("dist_0.05", {"distWeighting": 0.05}),                          # the Gaussian underflows to 0 away from the centre (1 there)
    ("dist_1e6", {"distWeighting": 1e6}),                            # flat
    ("diff_1_grad_0.03", dict(GRAD, diffWeighting=1.0, gradientWeighting=0.03)),
)
OVER = dict(ROWS)
NAMES = [n for n, _ in ROWS]
ALL_NAN = "grad_1e-3"
NAN_ROWS = ("diff_1", "diff_0.05", "diff_1e-3")                     # at least 5 NaN costs among the evaluations
MIXED_ROWS = ("diff_1", "diff_0.05", "diff_1e-3", "grad_0.005")     # at least 50 swarm rows with NaN and finite fitness
DETAIL_ROWS = ("diff_16", "diff_1", "diff_1e-3", "grad_1e-3")
DOME_ROWS = ("base", "diff_1", "grad_0.007")
DOME_FLOOR = {"base": 0, "diff_1": 105, "grad_0.007": 55}          # about half of the measured counts (module docstring)
SKIP_SHARE = 0.05


def _cfg(name, **over):
    from pais_mvs_amd.config import readme_config
    kw = dict(patchRadius=R, distWeighting=R / 3.0)
    kw.update(OVER[name] if isinstance(name, str) else name)
    kw.update(over)
    return readme_config(**kw)


# ---------------------------------------------------------------------------------------------------------------------
# the evaluations of one row: states, particles, refcost and the three oracle arithmetics (shared by CPU and GPU tests)
# ---------------------------------------------------------------------------------------------------------------------
_EVALS = {}


def _evals(request, name, over=None):
    """The evaluations of row `name` (or of the config overrides `over`, cached under `name`): the states and particles do not
    depend on the weights, so every row evaluates the same ones."""
    if name in _EVALS:
        return _EVALS[name]
    from tests.test_gpu_parity import _states_and_particles
    scene = request.getfixturevalue("pawn_small")
    cfg = _cfg(name if over is None else over)
    S = common.oracle_scene(cfg, scene)
    rng = np.random.default_rng(1000 + R)
    states, pats, idx, parts = _states_and_particles(S, scene, rng, n_per=12)
    ref, ref_det, lit, clit, ker = [], [], [], [], []
    for si, pos in zip(idx, parts):
        st = refcost.state_of(pats[si])
        ref.append(refcost.cost(scene, cfg, st, pos))
        ref_det.append(refcost.cost(scene, cfg, st, pos, normal_fn=_det_normal))
        S.set_kernel_arithmetic(False)
        S.set_cost_literal(False)
        lit.append(S.fitness(pats[si], pos))            # the reference's statements, platform libm
        S.set_kernel_arithmetic(True)
        S.set_cost_literal(True)
        clit.append(S.fitness(pats[si], pos))           # the same statements, deterministic exp / sin / cos
        S.set_cost_literal(False)
        ker.append(S.fitness(pats[si], pos))            # the kernel arithmetic
    S.close()
    ev = dict(scene=scene, cfg=cfg, states=states, pats=pats, idx=idx, parts=parts, ref=ref, ref_det=ref_det, lit=lit, clit=clit,
              ker=ker)
    _EVALS[name] = ev
    return ev


def _check_row(name, ev, refs, vals, gate, what):
    """check_against_refcost under the denormal rule, and the counts of the row -> (finite, DBL_MAX, NaN, skipped, worst)."""
    st = {}
    n_fin, n_max, skipped = check_against_refcost(name, refs, vals, gate, what, skip=denormal_sum, stats=st)
    n = len(ev["parts"])
    assert st["skipped_margin"] <= max(2, n // 50), (what, name, st)
    assert skipped <= SKIP_SHARE * n, (what, name, skipped, n, st)
    if name == ALL_NAN:
        assert n_fin == 0 and n_max >= 5, (what, name, n_fin, n_max)
    else:
        assert n_fin >= 30 and n_max >= 5, (what, name, n_fin, n_max)
    if name in NAN_ROWS:
        assert st["nan"] >= 5, (what, name, st)
    return n_fin, n_max, st["nan"], st["skipped_margin"], st["skipped_denormal"], st["worst"]


# ------------------------------------------------------------------------------------------------------------- CPU ---
@pytest.mark.parametrize("name", NAMES)
def test_oracle_cost_matches_refcost_every_weight_row(request, name):
    """The oracle's literal cost and its costLiteral within the literal gate of refcost, its kernel arithmetic within 1e-9;
    DBL_MAX exactly where refcost says DBL_MAX and NaN exactly where refcost says NaN; the counts of the row."""
    ev = _evals(request, name)
    gate = refcost.literal_gate(2 * R + 1)
    c1 = _check_row(name, ev, ev["ref"], ev["lit"], gate, "oracle literal")
    c2 = _check_row(name, ev, ev["ref_det"], ev["clit"], gate, "oracle costLiteral")
    c3 = _check_row(name, ev, ev["ref"], ev["ker"], RTOL_KERNEL, "oracle kernel arithmetic")
    print("weight row %-17s finite %3d DBL_MAX %3d NaN %3d skipped %d + %d   worst %.1e %.1e %.1e"
          % (name, c1[0], c1[1], c1[2], c1[3], c1[4], c1[5], c2[5], c3[5]))
    if name == ALL_NAN:     # as many NaN costs as the control has finite ones: every cost that is not DBL_MAX
        base = _evals(request, "base")
        want = sum(1 for c in base["ref"] if c.margin >= refcost.MARGIN and not denormal_sum(c) and c.value != DBL_MAX
                   and not math.isnan(c.value))
        all_masked = sum(1 for c in base["ref"] if c.margin >= refcost.MARGIN and math.isnan(c.value))
        assert c1[2] == want + all_masked and want >= 30, (c1, want, all_masked)
        assert all(c.sum_weight == 0 for c in ev["ref"] if c.outcome == "ok")


def test_huge_diff_weighting_is_the_switch_turned_off(request):
    """exp(-sad^2 / 1e300) is exactly 1.0 (the argument is far below 2^-54 in magnitude): the row's costs are those of
    adaptiveDifferenceEnable = False bit for bit, in refcost and in the three oracle arithmetics."""
    a = _evals(request, "diff_1e300")
    b = _evals(request, "diff_off", dict(adaptiveDifferenceEnable=False))
    for key in ("lit", "clit", "ker"):
        assert np.array(a[key]).tobytes() == np.array(b[key]).tobytes(), key
    for x, y in zip(a["ref"], b["ref"]):
        assert common.same_value(x.value, y.value, 0.0) and x.sum_weight == y.sum_weight, (x, y)
    assert sum(1 for c in a["ref"] if c.outcome == "ok" and c.live_pixels) >= 30


def test_flat_distance_table_is_not_exactly_one(request):
    """distWeighting 1e6: the entries of the distance table are 1 / 81 to eleven digits (the table is normalised to sum 1, and
    exp(-d^2 / 2e12) still differs from 1 in its last bits), not 1.0 -- so the row is NOT adaptiveDistanceEnable = False bit for
    bit, and that half of the metamorphic check is left out.  The costs agree to 1e-10."""
    g = refcost.gauss_table(_cfg("dist_1e6"))
    assert g.max() < 0.0124 and float(np.max(np.abs(g * len(g) - 1.0))) < 1e-10
    a = _evals(request, "dist_1e6")
    b = _evals(request, "dist_off", dict(adaptiveDistanceEnable=False))
    n = 0
    for x, y in zip(a["ref"], b["ref"]):
        if x.outcome == "ok" and x.live_pixels:
            n += 1
            assert refcost._rel(x.value, y.value) <= 1e-10, (x.value, y.value)
        else:
            assert common.same_value(x.value, y.value, 0.0)
    assert n >= 30


# ---------------------------------------------------------------------------------------------------------------------
# refine: candidates and the oracle's trace
# ---------------------------------------------------------------------------------------------------------------------
def _refine_cfg(name, many, **over):
    kw = dict(particleNum=6, maxIteration=8)             # (maxFitness stays the README's: drops by fitness happen too)
    if many:
        kw.update(reduceNormalRange=4.0, visibleCorrelation=0.6)
    kw.update(over)
    return _cfg(name, **kw)


_REFINE = {}


def _refine_case(request, name, many, particles=6, iterations=8):
    """Candidates of a refine row and the oracle's trace of them: (scene, cfg, cands, is_seed, runs per candidate, counts)."""
    key = (name, many, particles, iterations)
    if key in _REFINE:
        return _REFINE[key]
    from tests.test_pso_trace import _oracle_runs
    scene = request.getfixturevalue("dome_small" if many else "pawn_small")
    cfg = _refine_cfg(name, many, particleNum=particles, maxIteration=iterations)
    S = common.oracle_scene(cfg, scene)
    cands, is_seed = _refine_candidates(S, scene, 8 if many else 12)
    S.close()
    traced = [None] * len(cands)
    for flag in (True, False):
        ids = [i for i, s in enumerate(is_seed) if s == flag]
        for i, o in zip(ids, _oracle_runs(cfg, scene, [cands[i] for i in ids], flag)):
            traced[i] = o
    rows = mixed = with_cost = nan_parts = parts = 0
    for p, runs in traced:
        for o in runs:
            f = o["particles"][:, :, 9]                  # the fitness of every particle of every row of the run
            nan, fin = np.isnan(f), np.isfinite(f)       # (finite: a cost or DBL_MAX)
            rows += len(f)
            mixed += int(np.sum(nan.any(axis=1) & fin.any(axis=1)))
            with_cost += int(np.sum(nan.any(axis=1) & (fin & (f < DBL_MAX)).any(axis=1)))
            nan_parts += int(nan.sum())
            parts += f.size
    alive = sum(1 for p, _ in traced if not p.drop)
    case = dict(scene=scene, cfg=cfg, cands=cands, is_seed=is_seed, traced=traced,
                counts=dict(alive=alive, rows=rows, mixed=mixed, with_cost=with_cost, nan=nan_parts, particles=parts))
    _REFINE[key] = case
    return case


@pytest.mark.parametrize("name", MIXED_ROWS + ("base",))
def test_oracle_trace_holds_mixed_nan_swarms(request, name):
    """The oracle's refine trace of a NaN row holds at least 50 swarm rows with both a NaN and a finite fitness -- the input of
    the NaN branches of the swarm step --, that of the control none."""
    n = _refine_case(request, name, False)["counts"]
    print("weight row %-17s pawn: alive %d of 36, swarm rows %d, rows with NaN and finite %d (with a cost below DBL_MAX %d), "
          "NaN particles %d / %d" % (name, n["alive"], n["rows"], n["mixed"], n["with_cost"], n["nan"], n["particles"]))
    if name == "base":
        assert n["nan"] == 0 and n["rows"] >= 100, n
    else:
        assert n["mixed"] >= 50, n
        if name.startswith("diff"):     # (the gradient weight is one value per reference pixel: a candidate's costs are all NaN or none)
            assert n["with_cost"] >= 50, n


@pytest.mark.parametrize("name", DOME_ROWS)
def test_oracle_trace_of_the_dome_rows(request, name):
    n = _refine_case(request, name, True)["counts"]
    print("weight row %-17s dome: alive %d of 24, swarm rows %d, rows with NaN and finite %d (with a cost below DBL_MAX %d), "
          "NaN particles %d / %d" % (name, n["alive"], n["rows"], n["mixed"], n["with_cost"], n["nan"], n["particles"]))
    assert n["mixed"] >= DOME_FLOOR[name], n
    if name == "base":
        assert n["nan"] == 0, n


# ------------------------------------------------------------------------------------------------------------- GPU ---
def _gpu_costs(ev, monkeypatch, env):
    return P.fitness(monkeypatch, ev["cfg"], ev["scene"].cameras, ev["states"], ev["idx"], ev["parts"], env)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_cost_every_weight_row(request, name, monkeypatch):
    """Context.fitness_batch of a row: the default arithmetic equals the oracle's kernel arithmetic bit for bit (NaN as NaN)
    and refcost within 1e-9 under the skip rule; PAIS_ARITH=literal equals costLiteral bit for bit and refcost within the
    literal gate; byte taps and PAIS_PRE_SETUP=0 (the second copy of the static-weight code) give the default's bytes."""
    ev = _evals(request, name)
    got = _gpu_costs(ev, monkeypatch, {})
    for e, (g, want) in enumerate(zip(got, ev["ker"])):
        assert common.same_value(g, want, 0.0), ("default", name, e, g, want)
    _check_row(name, ev, ev["ref"], got, RTOL_KERNEL, "HIP default")
    lit = _gpu_costs(ev, monkeypatch, P.LITERAL)
    for e, (g, want) in enumerate(zip(lit, ev["clit"])):
        assert common.same_value(g, want, 0.0), ("literal", name, e, g, want)
    _check_row(name, ev, ev["ref_det"], lit, refcost.literal_gate(2 * R + 1), "HIP literal")
    for env, what in ((P.BYTE_TAPS, "byte taps"), (P.NO_PRE, "no pre-setup")):
        other = _gpu_costs(ev, monkeypatch, env)
        assert other.tobytes() == got.tobytes(), (name, what, int(np.sum(other.view(np.uint64) != got.view(np.uint64))))
    if name == "diff_1e300":
        off = _evals(request, "diff_off", dict(adaptiveDifferenceEnable=False))
        for env in ({}, P.LITERAL, P.NO_PRE):
            a, b = _gpu_costs(ev, monkeypatch, env), _gpu_costs(off, monkeypatch, env)
            assert a.tobytes() == b.tobytes(), (name, env)


@pytest.mark.gpu
@pytest.mark.parametrize("name", DETAIL_ROWS)
def test_gpu_detail_every_weight_row(request, name, monkeypatch):
    """pais_fitness_detail of a row: fitness bit-equal to the PAIS_ARITH=literal batch, the sums over the COUNTED pixels, and
    per-pixel weight and avgSad against the restatement of tests/test_fitness_detail.py.  A window of live pixels whose weights
    all vanish is outcome OK with sum_weight == 0 and fitness NaN; ALL_MASKED is live_pixels == 0."""
    from tests.test_fitness_detail import ALL_MASKED, OK, _check_identity, _check_pixels, _outcome_of
    ev = _evals(request, name)
    scene, cfg, states, idx, parts = ev["scene"], ev["cfg"], ev["states"], ev["idx"], ev["parts"]
    ctx = P.context(cfg, scene.cameras, monkeypatch, {})
    d = ctx.fitness_detail(states, idx, parts, colours=True, homographies=True)
    ctx.close()
    lit = _gpu_costs(ev, monkeypatch, P.LITERAL)
    _check_identity(d, lit, name)
    n_zero = 0
    for e, c in enumerate(ev["ref_det"]):
        oc, live, sw, fit = int(d.outcome[e]), int(d.live_pixels[e]), float(d.sum_weight[e]), float(d.fitness[e])
        assert (oc == ALL_MASKED) == (oc in (OK, ALL_MASKED) and live == 0), (name, e, oc, live)
        assert math.isnan(fit) == (oc in (OK, ALL_MASKED) and sw == 0), (name, e, oc, sw, fit)
        if oc == OK and sw == 0:
            n_zero += 1
            assert live > 0 and float(d.sum_weighted_sad[e]) == 0 and math.isnan(fit), (name, e, live)
        if c.margin >= refcost.MARGIN:
            assert oc in _outcome_of(c), (name, e, oc, c.outcome, c.live_pixels)
            if not denormal_sum(c):
                assert (c.sum_weight == 0) == (sw == 0), (name, e, c.sum_weight, sw)
    if name == ALL_NAN:
        assert n_zero == int(np.sum(d.outcome == OK)) >= 30, (name, n_zero)
    elif name != "diff_16":
        assert n_zero >= 5, (name, n_zero)
    picks, seen = [], {}
    for e in range(len(d)):
        kind = (int(d.outcome[e]), bool(d.sum_weight[e] == 0))
        if seen.get(kind, 0) < 4:
            seen[kind] = seen.get(kind, 0) + 1
            picks.append(e)
    for e in picks:
        _check_pixels(d, e, scene, cfg, refcost.state_of(states[idx[e]]), parts[e], name)


@pytest.mark.gpu
@pytest.mark.parametrize("name,many", [(n, False) for n in NAMES] + [(n, True) for n in DOME_ROWS],
                         ids=[n + "-few_cameras" for n in NAMES] + [n + "-many_cameras" for n in DOME_ROWS])
def test_gpu_refine_pipelines_every_weight_row(request, name, many, monkeypatch, capfd):
    """refine() of seeds and first-ring children of a row (particleNum 6, maxIteration 8, the README's maxFitness) through every
    evaluation pipeline: the same record bytes, equal to the oracle bit for bit.  Few cameras: k_pso_iter, k_pso_eval2 +
    k_pso_step, k_pso_ring and PAIS_ARITH=literal (against costLiteral).  Many cameras (dome, K > 12; three rows): the tile
    kernel, every particle verified through k_pso_eval2."""
    case = _refine_case(request, name, many)
    scene, cfg, cands, is_seed = case["scene"], case["cfg"], case["cands"], case["is_seed"]
    if not many and name in MIXED_ROWS:         # (before anything runs on the GPU)
        assert case["counts"]["mixed"] >= 50, case["counts"]
    if many:
        assert case["counts"]["mixed"] >= DOME_FLOOR[name], case["counts"]
    S = common.oracle_scene(cfg, scene)
    S.set_kernel_arithmetic(True)
    S.set_omp(True)
    want = oracle_records(S, cands, is_seed)

    def run(env):
        return P.refine(monkeypatch, cfg, scene.cameras, cands, env)

    ref, _ = run(P.NO_TILE if many else {})
    alive = 0
    for i, p in enumerate(want):
        compare_patch(ref[i], p, (name, "default", i, "seed" if is_seed[i] else "child"))
        alive += 0 if p.drop else 1
    assert alive >= 4, (name, alive, len(want))
    if many:
        assert max(c.num_cam for c in cands) > 12
        got, ks = run(P.TILE_VERIFIED)
        assert bytes(got) == bytes(ref), (name, "tile")
        P.assert_took("tile", ks, name)
        assert "tile verify" not in capfd.readouterr().out
    else:
        got, ks = run(P.ITER)
        P.assert_took("iter", ks, name)
        assert bytes(got) == bytes(ref), (name, "k_pso_iter")
        got, ks = run(P.EVAL2)
        P.assert_took("eval2", ks, name)
        assert bytes(got) == bytes(ref), (name, "k_pso_eval2 + k_pso_step")
        got, ks = run(P.RING)
        P.assert_took("ring", ks, name)
        assert ks.ring_launches == ks.eval2_launches, (name, ks.ring_launches, ks.eval2_launches, ks.ring_fallbacks)
        assert bytes(got) == bytes(ref), (name, "k_pso_ring")
        S.set_cost_literal(True)
        want_lit = oracle_records(S, cands, is_seed)
        S.set_cost_literal(False)
        got, _ = run(P.LITERAL)
        for i, p in enumerate(want_lit):
            compare_patch(got[i], p, (name, "literal", i, "seed" if is_seed[i] else "child"))
    S.close()


@pytest.mark.gpu
@pytest.mark.parametrize("particles", [6, 17, 33])
def test_gpu_nan_swarms_in_every_lane_layout(request, particles, monkeypatch):
    """Row diffWeighting 1.0 at particleNum 6, 17 and 33 (maxIteration 6): seeds of N = 12, 34, 66 and children of N = 6, 17,
    33 particles -- 4, 2 and 1 lanes per particle, the two-row DPP form, the 64-lane shuffle form and the serial LDS form --
    with swarms that hold NaN and finite fitness.  The records are the same bytes in k_pso_iter, k_pso_eval2 + k_pso_step and
    k_pso_ring; the traced rows are the oracle's (a NaN fitness as NaN, everything else bit for bit)."""
    from tests.test_pso_trace import _check_oracle_parity
    case = _refine_case(request, "diff_1", False, particles=particles, iterations=6)
    scene, cfg, cands, is_seed, traced = case["scene"], case["cfg"], case["cands"], case["is_seed"], case["traced"]
    for flag, ring_env, n_swarm in ((False, P.RING_SMALL_BATCH, particles), (True, P.SEED_RING, 2 * particles)):
        ids = [i for i, s in enumerate(is_seed) if s == flag]
        sub, oracle = [cands[i] for i in ids], [traced[i] for i in ids]
        mixed = 0
        for p, runs in oracle:
            for o in runs:
                assert o["N"] == n_swarm
                f = o["particles"][:, :, 9]
                mixed += int(np.sum(np.isnan(f).any(axis=1) & (f < DBL_MAX).any(axis=1)))
        assert mixed >= 50, (particles, n_swarm, mixed)
        ref, ks = P.refine(monkeypatch, cfg, scene.cameras, sub, P.ITER)
        P.assert_took("iter", ks, (particles, n_swarm))
        for i, (p, _) in enumerate(oracle):
            compare_patch(ref[i], p, (particles, n_swarm, i))
        got, ks = P.refine(monkeypatch, cfg, scene.cameras, sub, P.EVAL2)
        P.assert_took("eval2", ks, (particles, n_swarm))
        assert bytes(got) == bytes(ref), ("k_pso_eval2 + k_pso_step", particles, n_swarm)
        got, ks = P.refine(monkeypatch, cfg, scene.cameras, sub, ring_env)
        assert ks.ring_fallbacks == 0
        if n_swarm <= 64:       # (a ring pass needs the swarm's tasks in the lanes of one wave)
            assert ks.ring_launches >= 1 and ks.ring_evals > 0, (particles, n_swarm)
        assert bytes(got) == bytes(ref), ("k_pso_ring", particles, n_swarm)
        ctx = P.context(cfg, scene.cameras, monkeypatch, {})
        tr = ctx.pso_trace(sub, max_runs=8, particles=True)
        ctx.close()
        bad = _check_oracle_parity(tr, oracle, "kernel")
        assert bad is None, (particles, n_swarm, bad)
