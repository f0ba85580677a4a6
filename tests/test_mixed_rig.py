"""The cost, refine, NCC, loader and driver paths on a rig of UNEQUAL cameras (tests/mixed_rig.py): 16 cameras in eight shape
classes -- 320 x 240, 240 x 320 (portrait), 333 x 251 with a calibrated principal point, fx != fy, 160 x 120, 480 x 360,
96 x 72, 257 x 193 -- against the oracle AND against tests/refcost.py.

Every other scene of the suite is homogeneous (one image size, fx == fy, the integer image centre as principal point, lodRatio
0.8): a kernel that strides another camera's rows by the reference camera's width, reads focal[0] where focal[1] belongs, bounds
a tap by the wrong camera's height or takes one camera's maxLOD for another's changes no bit there.  Here every shape class is the
reference camera in turn, the camera lists hold K = 3, 6, 7, 12, 13, 16 cameras of mixed classes (the two-pixel and one-pixel
kernels, the two-level sums), and the levels run from 0 to the highest one at which the reference window still fits.

The small-level group: a large reference camera at a level where a LISTED small camera's level has fewer than 6 columns or
rows -- or no such level at all.  The reference's tap rule 2 <= ix < cols - 3 (patch.cpp:999) passes nothing there: the cost is
DBL_MAX (outcome overflow) as soon as one window pixel counts.

Configurations: A r = 3, all three adaptive weights; B r = 7 (the two-pixel walk at S^2 = 225); C lodRatio 0.5 (the cameras get
different maxLOD: 8 at 480 wide, 6 at 96 wide); D lodRatio 0.7, maxLOD 3, minLOD 1 (the configuration's cap and a non-zero first
level).
"""
import copy
import ctypes as C
import math

import numpy as np
import pytest

from tests import common, pipelines as P, refcost
from tests import mixed_rig as MR
from tests.common import DBL_MAX, compare_patch, oracle_records
from tests.golden import make_ncc_golden as G
from tests.refcost import MARGIN, check_against_refcost
from tests.test_camera_sweep import _particles, _patch_state
from tests.test_radius_sweep import RTOL_KERNEL, _check_tables, _corner_particles, _det_normal, _edge_on_particles

KS = (3, 6, 7, 12, 13, 16)
CONFIGS = {"A": dict(patchRadius=3, distWeighting=1.0),
           "B": dict(patchRadius=7, distWeighting=7 / 3.0),
           "C": dict(patchRadius=3, distWeighting=1.0, lodRatio=0.5),
           "D": dict(patchRadius=3, distWeighting=1.0, lodRatio=0.7, maxLOD=3, minLOD=1)}
LARGE_CAMS = (MR.LARGE, MR.LARGE + 8)       # the two 480 x 360 cameras
TINY_CAM, SMALL_CAM = MR.TINY, MR.SMALL     # 96 x 72, 160 x 120


def _cfg(name, **over):
    from pais_mvs_amd.config import readme_config
    kw = dict(adaptiveDistanceEnable=True, adaptiveDifferenceEnable=True, adaptiveGradientEnable=True)
    kw.update(CONFIGS[name])
    kw.update(over)
    return readme_config(**kw)


@pytest.fixture(scope="module")
def rig():
    return MR.rig_scene()


_SCENES = {}


def _scene(rig, name):
    """The rig with the pyramids of configuration `name`."""
    cfg = _cfg(name)
    key = (cfg.lodRatio, cfg.maxLOD)
    if key not in _SCENES:
        _SCENES[key] = rig if key == (0.8, 15) else MR.with_pyramids(rig, cfg.lodRatio, cfg.maxLOD)
    return _SCENES[key]


# ---------------------------------------------------------------------------------------------------------------------
# hand-built states
# ---------------------------------------------------------------------------------------------------------------------
def _others(ref, n, n_cams=MR.N_CAMS):
    """The n cameras behind `ref` in index order (cyclic): neighbouring indices are different shape classes."""
    return [(ref + 1 + i) % n_cams for i in range(n)]


def _head(S, X, ref, cams, lod, key):
    """An oracle patch of the listed cameras with the reference camera and the level SET (refine()'s head otherwise: depth and
    ray from the reference camera, the depth range)."""
    from oracle import po
    L = po.lib()
    p = S.seed_patch(X, cams, key=key)
    p.refCamIdx = int(ref)
    L.po_set_depth_and_ray(S.ptr, C.byref(p))
    L.po_set_depth_range(S.ptr, C.byref(p))
    assert not p.drop, (ref, cams, lod)
    p.LOD = int(lod)
    return p


def _class_specs(scene, cfg, full):
    """Every shape class as reference camera: four states each, K cycling through KS, at levels 0, 1, 2 and the highest one
    that holds the reference window; at K = 7 the reference camera is left out of the list; at K = 13 and 16 (levels 0 and 1)
    also the list without the reference camera and with a camera listed twice (test_camera_sweep.py's VARIANT_K kinds)."""
    r = cfg.patchRadius
    specs = []
    for c in range(len(MR.SHAPES)):
        for j in range(4 if full else 2):
            ref = c + 8 * (j % 2)
            X = scene.seeds[(3 * c + j) % len(scene.seeds)][0]
            top = MR.highest_fitting_lod(scene.cameras[ref], X, cfg.lodRatio, r)
            assert top >= 2, (c, ref, top)
            lod = (0, 1, 2, top)[j]
            K = KS[(c + j) % len(KS)] if full else (6, 12)[j]
            group = "class%d" % c
            if K == 7:
                specs.append(dict(group=group, kind="no_ref", X=X, ref=ref, cams=sorted(_others(ref, 7)), lod=lod, n_per=12))
                continue
            specs.append(dict(group=group, kind="listed", X=X, ref=ref, cams=sorted([ref] + _others(ref, K - 1)), lod=lod, n_per=12))
            if K in (13, 16) and lod <= 1:
                o = _others(ref, 15)
                no_ref = sorted(o[:13]) if K == 13 else sorted(o + o[:1])
                twice = sorted([ref] + o[:K - 2] + o[:1])
                specs.append(dict(group=group, kind="no_ref", X=X, ref=ref, cams=no_ref, lod=lod, n_per=6))
                specs.append(dict(group=group, kind="twice", X=X, ref=ref, cams=twice, lod=lod, n_per=6))
    return specs


def _small_specs(scene, cfg):
    """A 480 x 360 reference camera at the levels where the listed 96 x 72 (160 x 120) camera's level has fewer than 6 columns
    or rows, up to the highest level that holds the reference window; K = 3 (two-pixel kernels) and every camera (one-pixel)."""
    r = cfg.patchRadius
    specs = []
    for n, ref in enumerate(LARGE_CAMS):
        X = scene.seeds[n][0]
        top = MR.highest_fitting_lod(scene.cameras[ref], X, cfg.lodRatio, r)
        for lod in range(top + 1):
            for small in (TINY_CAM, SMALL_CAM + 8):
                if lod > scene.cameras[small].max_lod:
                    continue
                rows, cols = scene.cameras[small].pyramid[lod].shape
                if min(rows, cols) >= 6:
                    continue
                other = LARGE_CAMS[1 - n]
                specs.append(dict(group="small", kind="dim%d" % min(rows, cols, 5), X=X, ref=ref, cams=sorted([ref, small, other]), lod=lod, n_per=6))
                if small == TINY_CAM:
                    specs.append(dict(group="small", kind="dim%d" % min(rows, cols, 5), X=X, ref=ref, cams=list(range(MR.N_CAMS)), lod=lod, n_per=6))
    # a level the listed camera does not have: on this rig (images up to 480 wide, the smallest 96) the reference window
    # no longer fits there -- the evaluation is DBL_MAX by its window, and the kernels must not address the absent level
    for ref in LARGE_CAMS:
        ml = scene.cameras[TINY_CAM].max_lod
        if scene.cameras[ref].max_lod > ml:
            specs.append(dict(group="absent_outside", kind="absent", X=scene.seeds[0][0], ref=ref, cams=sorted([ref, TINY_CAM, TINY_CAM + 8]),
                              lod=ml + 1, n_per=6))
    return specs


def _build_evals(scene, cfg, specs, seed):
    """States, particles (test_gpu_parity.py's kinds, test_radius_sweep.py's corner and edge-on particles), refcost and the three
    oracle arithmetics of every evaluation."""
    S = common.oracle_scene(cfg, scene)
    rng = np.random.default_rng(seed)
    states, pats, spec_of, idx, parts, groups, kinds = [], [], [], [], [], [], []
    for n, sp in enumerate(specs):
        p = _head(S, sp["X"], sp["ref"], sp["cams"], sp["lod"], key=n)
        si = len(states)
        states.append(_patch_state(p))
        pats.append(p)
        spec_of.append(sp)
        st = refcost.state_of(p)
        base = (p.normalS[0], p.normalS[1], p.depth)
        extra = []
        if sp["group"].startswith("class"):
            extra = [("corner", pos) for pos in _corner_particles(scene, cfg, st, base)] + \
                    [("edge_on", pos) for pos in _edge_on_particles(scene, cfg, st, base)]
        for kind, pos in [("sample", pos) for pos in _particles(p, rng, sp["n_per"])] + extra:
            idx.append(si); parts.append(list(pos)); groups.append(sp["group"]); kinds.append(sp["kind"] + "/" + kind)
    ref, ref_det, lit, clit, ker = [], [], [], [], []
    for si, pos in zip(idx, parts):
        st = refcost.state_of(pats[si])
        ref.append(refcost.cost(scene, cfg, st, pos))
        ref_det.append(refcost.cost(scene, cfg, st, pos, normal_fn=_det_normal))
        S.set_kernel_arithmetic(False)
        S.set_cost_literal(False)
        lit.append(S.fitness(pats[si], pos))
        S.set_kernel_arithmetic(True)
        S.set_cost_literal(True)
        clit.append(S.fitness(pats[si], pos))
        S.set_cost_literal(False)
        ker.append(S.fitness(pats[si], pos))
    S.close()
    return dict(scene=scene, cfg=cfg, states=states, pats=pats, specs=spec_of, idx=idx, parts=parts, groups=groups, kinds=kinds,
                ref=ref, ref_det=ref_det, lit=lit, clit=clit, ker=ker)


_EVALS = {}


def _evals(rig, name):
    if name not in _EVALS:
        scene, cfg = _scene(rig, name), _cfg(name)
        specs = _class_specs(scene, cfg, full=name != "B")
        if name != "B":
            specs += _small_specs(scene, cfg)
        _EVALS[name] = _build_evals(scene, cfg, specs, 7000 + ord(name))
    return _EVALS[name]


def _absent_evals(rig):
    """The level a listed camera does not have, under a VALID reference window: it takes a reference level of at least
    2 r + 6 pixels where the listed camera's is below one pixel -- a size ratio the rig's classes (96 .. 480) do not span.  So:
    the two 480 x 360 cameras and a 24 x 18 view from camera 6's place, lodRatio 0.5, r = 1; at level 5 the reference level is
    15 x 11 and the small camera (maxLOD 4) has none."""
    if "absent" in _EVALS:
        return _EVALS["absent"]
    from pais_mvs_amd import synth
    from pais_mvs_amd.camera import Camera, quaternion_to_rotation
    from pais_mvs_amd.config import readme_config
    cfg = readme_config(patchRadius=1, distWeighting=1 / 3.0, lodRatio=0.5, adaptiveDistanceEnable=True, adaptiveDifferenceEnable=True,
                        adaptiveGradientEnable=True)
    cams = []
    for i in LARGE_CAMS:
        c = rig.cameras[i]
        cams.append(Camera(focal=c.focal.copy(), principle_point=c.principle_point.copy(), quaternion=c.quaternion.copy(),
                           center=c.center.copy(), image=c.image, name=c.name).finalize(0.5, 15, True))
    c = rig.cameras[TINY_CAM]
    f2, pp = np.array([30.0, 30.0]), np.array([12.0, 9.0])
    img = synth.render(rig.obj, quaternion_to_rotation(c.quaternion), c.center, f2, pp, 24, 18)
    cams.append(Camera(focal=f2, principle_point=np.array([-1.0, -1.0]), quaternion=c.quaternion.copy(), center=c.center.copy(), image=img,
                       name="mix24").finalize(0.5, 15, True))
    scene = synth.Scene("absent", cams, rig.obj, rig.seeds)
    assert cams[2].max_lod == 4 and cams[0].max_lod == 8
    X = rig.seeds[0][0]
    assert MR.highest_fitting_lod(cams[0], X, 0.5, 1) == 5
    specs = [dict(group="absent", kind="absent", X=X, ref=ref, cams=[0, 1, 2], lod=5, n_per=12) for ref in (0, 1)]
    specs += [dict(group="absent", kind="dim%d" % d, X=X, ref=0, cams=[0, 1, 2], lod=lod, n_per=6) for lod, d in ((2, 4), (3, 2), (4, 1))]
    _EVALS["absent"] = _build_evals(scene, cfg, specs, 7999)
    return _EVALS["absent"]


def _group_counts(ev, vals, gate, what, refs="ref"):
    """check_against_refcost per group -> {group: (finite, DBL_MAX, skipped, evaluations)}."""
    out = {}
    for g in sorted(set(ev["groups"])):
        sel = [e for e, x in enumerate(ev["groups"]) if x == g]
        n_fin, n_max, skipped = check_against_refcost((what, g), [ev[refs][e] for e in sel], [vals[e] for e in sel], gate, what)
        out[g] = (n_fin, n_max, skipped, len(sel))
    return out


def _valid_overflows(ev, group):
    """Evaluations of a group that refcost ends as `overflow` (the reference window valid, a counted tap out of bounds) at a
    margin of at least MARGIN."""
    return [e for e, g in enumerate(ev["groups"]) if g == group and ev["ref"][e].outcome == "overflow" and ev["ref"][e].margin >= MARGIN]


def _check_conditions(ev, counts, name):
    for g, (n_fin, n_max, skipped, n) in counts.items():
        assert skipped <= 0.1 * n, (name, g, skipped, n)
        if g.startswith("class") and name != "B":
            assert n_fin >= 10 and n_max >= 3, (name, g, n_fin, n_max)
    if name != "B":
        assert set(counts) >= {"class%d" % c for c in range(len(MR.SHAPES))} | {"small"}, sorted(counts)
        assert len(_valid_overflows(ev, "small")) >= 6, (name, len(_valid_overflows(ev, "small")))


# ------------------------------------------------------------------------------------------------------------- CPU ---
def test_the_rig_is_unequal(rig):
    """What the tests below rely on: eight shape classes, two cameras each; fx != fy and off-centre principal points among
    them; every seed seen by all 16 cameras (each with the margin in its own image); under lodRatio 0.5 the cameras' maxLOD
    differ (8 at 480 wide, 6 at 96 wide); under configuration D the cap (3) holds for all."""
    cams = rig.cameras
    assert len(cams) == MR.N_CAMS and len({(c.width, c.height) for c in cams}) == 7
    assert any(c.focal[0] != c.focal[1] for c in cams) and any(c.height > c.width for c in cams)
    assert any(tuple(c.principle_point) != (float(c.width >> 1), float(c.height >> 1)) for c in cams)
    assert len(rig.seeds) == 12 and all(len(vis) == MR.N_CAMS for _, vis in rig.seeds)
    c5 = _scene(rig, "C").cameras
    assert c5[MR.LARGE].max_lod == 8 and c5[MR.TINY].max_lod == 6
    assert {c.max_lod for c in _scene(rig, "D").cameras} == {3}
    assert all(c.max_lod == 15 for c in cams)


def test_refcost_absent_level_passes_no_tap(rig):
    """refcost's definition of a level a camera does not have: shape (0, 0) -- every tap and every NCC sample fails."""
    cam = _scene(rig, "C").cameras[MR.TINY]
    assert refcost.level_shape(cam, 6) == cam.pyramid[6].shape and refcost.level_shape(cam, 7) == (0, 0)


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_oracle_cost_matches_refcost_on_the_mixed_rig(rig, name):
    """The proof that the inputs are good before anything touches a GPU: the oracle's kernel arithmetic within RTOL_KERNEL of
    refcost, its literal cost and costLiteral within the literal gate, DBL_MAX exactly where refcost puts it.  Per reference
    shape class at least 10 finite and 3 DBL_MAX evaluations; in the small-level group at least 6 whose refcost outcome is
    `overflow` under a valid reference window; at most 10 % of a group skipped for its margin."""
    ev = _evals(rig, name)
    gate = refcost.literal_gate(ev["cfg"].patchSize)
    _group_counts(ev, ev["lit"], gate, "oracle literal")
    _group_counts(ev, ev["clit"], gate, "oracle costLiteral", refs="ref_det")
    counts = _group_counts(ev, ev["ker"], RTOL_KERNEL, "oracle kernel arithmetic")
    _check_conditions(ev, counts, name)
    if name == "B":
        return
    # the states: every K, every class as reference camera, no_ref and twice lists, levels from 0 to beyond 2
    ks = {st.num_cam for st in ev["states"]}
    assert ks >= set(KS), ks
    kinds = {sp["kind"] for sp in ev["specs"]}
    assert {"listed", "no_ref", "twice"} <= kinds, kinds
    assert max(sp["lod"] for sp in ev["specs"] if sp["group"].startswith("class")) >= 3
    for sp, p in zip(ev["specs"], ev["pats"]):
        assert (p.refCamIdx in p.cams()) == (sp["kind"] != "no_ref") and p.cams() == sorted(p.cams())
    small = {sp["kind"] for sp in ev["specs"] if sp["group"] == "small"}
    assert small >= ({"dim5", "dim4", "dim3"} if name == "A" else {"dim4"}), small
    finite_k = {ev["states"][ev["idx"][e]].num_cam for e, c in enumerate(ev["ref"]) if c.margin >= MARGIN and c.outcome == "ok"}
    assert finite_k >= set(KS), finite_k


def test_oracle_cost_matches_refcost_at_an_absent_level(rig):
    """A listed camera without the state's level under a valid reference window: `overflow` in refcost, DBL_MAX in every
    oracle arithmetic."""
    ev = _absent_evals(rig)
    counts = _group_counts(ev, ev["ker"], RTOL_KERNEL, "oracle kernel arithmetic")
    _group_counts(ev, ev["lit"], refcost.literal_gate(3), "oracle literal")
    assert counts["absent"][2] <= 0.1 * counts["absent"][3]
    over = [e for e in _valid_overflows(ev, "absent") if ev["kinds"][e].startswith("absent")]
    assert len(over) >= 6, len(over)
    assert all(ev["ker"][e] == ev["clit"][e] == ev["lit"][e] == DBL_MAX for e in over)


def test_scheduler_on_the_mixed_rig_reproduces_oracle_rounds(rig):
    """The host driver's per-camera cell maps without a GPU: the scheduler (device -1) fed with oracle records against the
    oracle's own driver, B = 8, 8 rounds, patch for patch."""
    from tests.test_scheduler_cpu import _run_oracle, _run_product_with_oracle_records
    cfg = _cfg("A", particleNum=6, maxIteration=8)
    want, calls, _S = _run_oracle(cfg, rig, 8, 8)
    m = _run_product_with_oracle_records(cfg, rig, 8, 8)
    got = [(list(p.center[:]), list(p.normal[:]), p.cams(), p.fitness, p.priority) for p in m.patches()]
    assert len(got) == len(want) and len(got) >= 100, (len(got), len(want))
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, (i, a, b)
    st = m.stats()
    assert st.candidates_effective + st.seeds_refined == calls
    m.close()


# ------------------------------------------------------------------------------------------------------------- GPU ---
def _get_evals(rig, name):
    return _absent_evals(rig) if name == "absent" else _evals(rig, name)


def _fitness(monkeypatch, ev, env, cameras=None):
    """fitness_batch of the evaluations, one batch per camera count (a batch takes its kernel shape from its largest K: the
    two-pixel kernels up to 12 cameras, the one-pixel kernels beyond)."""
    with P.knobs(monkeypatch, env):
        ctx = P.context(ev["cfg"], cameras or ev["scene"].cameras)
        out = np.empty(len(ev["parts"]), dtype=np.float64)
        for K in sorted({st.num_cam for st in ev["states"]}):
            sel = [si for si, st in enumerate(ev["states"]) if st.num_cam == K]
            pos = {si: n for n, si in enumerate(sel)}
            es = [e for e, si in enumerate(ev["idx"]) if si in pos]
            out[es] = ctx.fitness_batch([ev["states"][si] for si in sel], [pos[ev["idx"][e]] for e in es], [ev["parts"][e] for e in es])
        ctx.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "B", "C", "absent"])
def test_gpu_cost_on_the_mixed_rig(rig, name, monkeypatch):
    """fitness_batch equals the oracle's kernel arithmetic bit for bit and refcost within RTOL_KERNEL, with the float2 taps
    and with the byte taps (PAIS_TAP_FLOAT_MAX_MB=0); PAIS_ARITH=literal equals costLiteral bit for bit.  The small-level
    group (a listed camera's level below 6 pixels, or absent) is DBL_MAX wherever refcost says `overflow`."""
    ev = _get_evals(rig, name)
    got = _fitness(monkeypatch, ev, {})
    for e, (g, want) in enumerate(zip(got, ev["ker"])):
        assert common.same_value(g, want, 0.0), ("default", name, e, ev["groups"][e], ev["kinds"][e], ev["specs"][ev["idx"][e]]["lod"], g, want)
    counts = _group_counts(ev, got, RTOL_KERNEL, "HIP default")
    if name != "absent":
        _check_conditions(ev, counts, name)
    for grp in ("small", "absent"):
        for e in _valid_overflows(ev, grp):
            assert got[e] == DBL_MAX, (name, grp, e, ev["kinds"][e], got[e])
    byte = _fitness(monkeypatch, ev, P.BYTE_TAPS)
    assert byte.tobytes() == got.tobytes(), (name, np.flatnonzero(byte.view(np.int64) != got.view(np.int64))[:8])
    lit = _fitness(monkeypatch, ev, P.LITERAL)
    for e, (g, want) in enumerate(zip(lit, ev["clit"])):
        assert common.same_value(g, want, 0.0), ("literal", name, e, ev["groups"][e], ev["kinds"][e], g, want)
    _group_counts(ev, lit, refcost.literal_gate(ev["cfg"].patchSize), "HIP literal", refs="ref_det")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "C"])
def test_gpu_cost_edges_on_the_fly_on_the_mixed_rig(rig, name, monkeypatch):
    """level_edge == NULL: k_level_edge_minmax over unequal levels, the edge weight evaluated from each camera's own gray
    level -- the bytes of the cost computed from the given edge maps."""
    ev = _get_evals(rig, name)
    bare = []
    for cam in ev["scene"].cameras:
        c2 = copy.copy(cam)
        c2.edge_pyramid = []
        bare.append(c2)
    given = _fitness(monkeypatch, ev, {})
    fly = _fitness(monkeypatch, ev, {}, cameras=bare)
    assert np.isfinite(given[given != DBL_MAX]).sum() > 100
    assert fly.tobytes() == given.tobytes(), (name, np.flatnonzero(fly.view(np.int64) != given.view(np.int64))[:8])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "C", "absent"])
def test_gpu_fitness_detail_on_the_mixed_rig(rig, name, monkeypatch):
    """pais_fitness_detail of the small-level group and of one state per reference shape class: the fitness equals
    PAIS_ARITH=literal bit for bit, the outcome is refcost's (the small-level evaluations report OVERFLOW, not OK), and the
    per-camera H, colour rows, codes and sums of a few evaluations of every outcome restate pixel by pixel."""
    from tests.test_fitness_detail import OVERFLOW, _check_identity, _check_pixels, _ctx as detail_ctx, _outcome_of
    ev = _get_evals(rig, name)
    scene, cfg = ev["scene"], ev["cfg"]
    first = {}
    for si, sp in enumerate(ev["specs"]):
        first.setdefault(sp["group"], si)
    keep = [si for si, sp in enumerate(ev["specs"]) if not sp["group"].startswith("class") or first[sp["group"]] == si]
    pos = {si: n for n, si in enumerate(keep)}
    es = [e for e, si in enumerate(ev["idx"]) if si in pos]
    states, idx, parts = [ev["states"][si] for si in keep], [pos[ev["idx"][e]] for e in es], [ev["parts"][e] for e in es]
    ctx = detail_ctx(cfg, scene, monkeypatch)
    d = ctx.fitness_detail(states, idx, parts, colours=True, homographies=True)
    ctx.close()
    lit = _fitness(monkeypatch, ev, P.LITERAL)[es]
    _check_identity(d, lit, ("mixed", name))
    over = set(_valid_overflows(ev, "small") + _valid_overflows(ev, "absent"))
    seen, n_over = {}, 0
    for k, e in enumerate(es):
        c = ev["ref_det"][e]
        if c.margin < MARGIN:
            continue
        oc = int(d.outcome[k])
        assert oc in _outcome_of(c), (name, e, ev["kinds"][e], oc, c.outcome)
        key = (ev["groups"][e], oc)
        if e in over:
            assert oc == OVERFLOW and ev["ref"][e].outcome == "overflow", (name, e, oc)
            n_over += 1
        if seen.get(key, 0) >= 3:
            continue
        seen[key] = seen.get(key, 0) + 1
        _check_pixels(d, k, scene, cfg, refcost.state_of(ev["pats"][ev["idx"][e]]), parts[k], ("mixed", name, e, ev["kinds"][e]))
    assert n_over >= 6, (name, n_over)
    assert len({g for g, _ in seen}) >= (2 if name == "absent" else 9) - 1, sorted(seen)


# ---------------------------------------------------------------------------------------------------------------------
# refine(): the 12 seeds (camera lists thinned so that every shape class is the reference camera of some candidate), two
# expansion candidates beside each, and centres beside the object, whose empty window climbs the reference camera's pyramid
# ---------------------------------------------------------------------------------------------------------------------
def _refine_candidates(S, scene):
    from pais_mvs_amd.context import make_candidate, normal_to_spherical
    from tests.golden.make_resume_cloud import back_project
    cands, is_seed = [], []
    for i, (X, vis) in enumerate(scene.seeds):
        cams = [c for c in vis if c % 8 >= i % 8] if i % 8 < 7 else [c for c in vis if c % 8 in (6, 4, 5)]
        key = 1000 + 10 * i
        p = S.seed_patch(X, cams, key=key)
        cands.append(make_candidate(p.center[:], p.normal[:], p.cams(), key, 0, normalS=p.normalS[:]))
        is_seed.append(True)
        for j in range(2):
            cen = [p.center[0] + 0.004 * (j - 0.5), p.center[1] + 0.002 * j, p.center[2] - 0.001 * j]
            cands.append(make_candidate(cen, p.normal[:], p.cams(), key + 1 + j, 1, normalS=p.normalS[:]))
            is_seed.append(False)
    for k, ci in enumerate((MR.SMALL, MR.PORTRAIT)):       # beside the object: every window pixel masked, variance 0
        cam = scene.cameras[ci]
        n = [-float(v) for v in cam.optical_normal]
        X = back_project(cam, 0.19 * cam.width, 0.5 * cam.height, 4.0)
        cands.append(make_candidate(X, n, list(range(MR.N_CAMS)), 2000 + k, 0, normalS=normal_to_spherical(n)))
        is_seed.append(True)
    return cands, is_seed


_REFINE = {}


def _refine_case(rig, name):
    if name not in _REFINE:
        scene, cfg = _scene(rig, name), _cfg(name, particleNum=6, maxIteration=8)
        S = common.oracle_scene(cfg, scene)
        S.set_kernel_arithmetic(True)
        S.set_omp(True)
        cands, is_seed = _refine_candidates(S, scene)
        want = oracle_records(S, cands, is_seed)
        S.close()
        _REFINE[name] = (scene, cfg, cands, is_seed, want)
    return _REFINE[name]


@pytest.mark.parametrize("name", ["A", "C", "D"])
def test_refine_candidates_of_the_mixed_rig(rig, name):
    """What the GPU test compares, on the oracle alone: 12 seeds, 24 expansion candidates beside them and two empty-window
    centres; the surviving records have reference cameras of at least six shape classes and 3 .. 16 cameras.  lodRatio 0.5:
    some record ends at a level >= 1.  Configuration D: every record at a level >= 1 (minLOD) and some at its reference
    camera's maxLOD (3, the configuration's cap).  (Under lodRatio 0.5 no S x S window fits the 1 x 1 top level of a camera,
    so setLOD cannot END at a camera's own maxLOD there: it falls back one level, patch.cpp:548-552.)"""
    scene, cfg, cands, is_seed, want = _refine_case(rig, name)
    assert sum(is_seed[:36]) == 12 and len(cands) == 38
    alive = [p for p in want if not p.drop]
    assert len(alive) >= 24, len(alive)
    assert len({MR.shape_class(p.refCamIdx) for p in alive}) >= 6, sorted({p.refCamIdx for p in alive})
    assert min(p.numCam for p in alive) <= 4 and max(p.numCam for p in alive) == 16
    ran = [p for p in want if p.psoRuns >= 1]
    if name in ("C", "D"):
        assert any(p.LOD >= 1 for p in ran), [p.LOD for p in ran]
    if name == "D":
        assert all(p.LOD >= 1 for p in ran) and any(p.LOD == scene.cameras[p.refCamIdx].max_lod == 3 for p in ran), [p.LOD for p in ran]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "C", "D"])
def test_gpu_refine_pipelines_on_the_mixed_rig(rig, name, monkeypatch, capfd):
    """refine_batch of the candidates above: the default equals the oracle field by field; k_pso_iter, k_pso_eval2 + k_pso_step
    (with and without the set-up records), k_pso_ring and the tile kernel (every particle verified through k_pso_eval2) give
    the same record bytes.  A record that ran its PSO carries the oracle's reference camera and level whether it survived or
    not (setLOD against the reference camera's own maxLOD)."""
    scene, cfg, cands, is_seed, want = _refine_case(rig, name)
    ref, _ = P.refine(monkeypatch, cfg, scene.cameras, cands, {})
    for i, p in enumerate(want):
        compare_patch(ref[i], p, (name, "default", i, "seed" if is_seed[i] else "child"))
        if p.psoRuns >= 1:
            assert (ref[i].ref_cam, ref[i].lod) == (p.refCamIdx, p.LOD), (name, i, ref[i].ref_cam, ref[i].lod, p.refCamIdx, p.LOD)
    runs = [(P.ITER, "iter"), (P.EVAL2, "eval2"), (dict(P.EVAL2, **P.NO_PRE), "eval2"), (P.RING, "ring"), (P.TILE_VERIFIED, "tile")]
    for env, kind in runs:
        got, ks = P.refine(monkeypatch, cfg, scene.cameras, cands, env)
        assert bytes(got) == bytes(ref), (name, env)
        P.assert_took(kind, ks, (name, env))
    assert "tile verify" not in capfd.readouterr().out


# ---------------------------------------------------------------------------------------------------------------------
# pais_ncc_batch
# ---------------------------------------------------------------------------------------------------------------------
def _inside(scene, cfg, st):
    """Per listed camera: the warped window stays inside [0, cols-1) x [0, rows-1) (refcost) -> ([inside], margin)."""
    s = refcost.State(st["ref"], st["lod"], st["cams"])
    H = refcost.homographies(scene.cameras, s, st["center"], st["normal"], cfg.lodRatio)
    pt = refcost.project(scene.cameras[st["ref"]], st["center"], cfg.lodRatio ** st["lod"])
    out, margin = [], math.inf
    with np.errstate(invalid="ignore", divide="ignore"):
        for i, c in enumerate(st["cams"]):
            _, ok, m = refcost.homography_patch(scene.cameras[c].pyramid[st["lod"]], pt, H[i], cfg.patchRadius)
            out.append(ok)
            margin = min(margin, m)
    return out, margin


def _leave_state(scene, cfg):
    """A centre moved along the image axes of the 480 x 360 reference camera until the window leaves the listed 96 x 72
    camera's image and nobody else's."""
    ref, cams = MR.LARGE, [MR.LARGE, MR.TINY, MR.LARGE + 8]
    cam = scene.cameras[ref]
    X0 = np.asarray(scene.seeds[0][0], float)
    R = np.asarray(cam.rotation, float)
    depth = float(np.linalg.norm(X0 - cam.center))
    for axis, sign in ((0, 1), (0, -1), (1, 1), (1, -1)):
        step = sign * R[axis] * depth / float(cam.focal[axis])          # about one pixel of the reference camera
        for t in range(0, 240, 2):
            st = G._state(X0 + t * step, [0.0, 0.0, 1.0], ref, 0, cams, "leaves_small")
            ins, margin = _inside(scene, cfg, st)
            if ins == [True, False, True] and margin >= MARGIN:
                return st
    return None


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "C"])
def test_gpu_ncc_batch_on_the_mixed_rig(rig, name):
    """pais_ncc_batch on view states of refined records (K up to 16; make_ncc_golden's perturbations, subsets, tilts and edge
    states) and on a state whose window leaves the 96 x 72 camera's image but not the reference camera's: bit for bit
    G.oracle_ncc, tables within the table gate of refcost."""
    from pais_mvs_amd.context import make_view_state
    from tests.golden.make_resume_cloud import back_project
    from tests.test_ncc_batch import _compare
    scene, cfg, cands, is_seed, want = _refine_case(rig, name)
    S = common.oracle_scene(cfg, scene)
    S.set_kernel_arithmetic(True)
    S.set_omp(True)
    ctx = P.context(cfg, scene.cameras)
    res = ctx.refine_batch([c for c, s in zip(cands, is_seed) if s])
    recs = [(list(x.center[:]), list(x.normal[:]), x.ref_cam, x.lod, x.cams(), [int(v) for v in scene.seeds[0][1]])
            for x in res if not x.dropped and x.num_cam >= 2]
    assert len(recs) >= 8, len(recs)
    states = G.scene_states(S, scene, recs, np.random.default_rng(6000 + ord(name)), n_search=4)
    leave = _leave_state(scene, cfg)
    assert leave is not None
    states.append(leave)
    # below the landscape cameras' field of view, inside the two portrait cameras': rows 260 .. 266 of a 240 x 320 image, which a
    # bound by the width would refuse (beside the object: the patches are empty, so no table of refcost's to compare)
    port = scene.cameras[MR.PORTRAIT]
    tall = G._state(back_project(port, 120.0, 262.0, 4.0), [-float(v) for v in port.optical_normal], MR.PORTRAIT, 0,
                    [MR.PORTRAIT, MR.PORTRAIT + 8], "portrait_rows")
    ins, margin = _inside(scene, cfg, tall)
    assert ins == [True, True] and margin >= MARGIN and 240 + cfg.patchRadius < MR.project0(scene.cameras[MR.PORTRAIT + 8], tall["center"])[1]
    states.append(tall)
    got = ctx.ncc_batch([make_view_state(st["center"], st["normal"], st["ref"], st["lod"], st["cams"]) for st in states], tables=True)
    for i, st in enumerate(states):
        _compare(got, i, G.oracle_ncc(S, st), (name, i, st["kind"]))
    assert int(got.dropped[len(states) - 2]) == G.DROP_SAMPLE and int(got.dropped[len(states) - 1]) != G.DROP_SAMPLE
    mine = [{"dropped": int(got.dropped[i]), "table": got.tables[i].ravel().tolist()} for i in range(len(states) - 1)]
    n_tab, n_drop, skipped = _check_tables(cfg.patchRadius, cfg, scene, states[:-1], mine, "HIP")
    assert n_tab >= 8 and n_drop >= 1 and skipped <= 2, (name, n_tab, n_drop, skipped)
    assert max(len(st["cams"]) for st in states) == 16
    assert len({MR.shape_class(st["ref"]) for st in states}) >= 5
    ctx.close()
    S.close()


# ---------------------------------------------------------------------------------------------------------------------
# the loader constructor
# ---------------------------------------------------------------------------------------------------------------------
def _loader_records(scene):
    """Hand-placed .mvs records: surface points with thinned camera lists (reference cameras of several shape classes), a
    centre at the left and one at the lower border of the portrait camera (its 7 x 7 window leaves the image at level 0: setLOD's
    fallback), centres beside the object in the 160 x 120 and the 96 x 72 camera (an empty window: setLOD climbs their pyramids),
    a record below minCamNum."""
    from pais_mvs_amd.context import normal_to_spherical
    from pais_mvs_amd import synth
    from tests.golden.make_resume_cloud import back_project

    def rec(kind, center, normal, cams):
        return {"kind": kind, "center": [float(v) for v in center], "normalS": normal_to_spherical([float(v) for v in normal]),
                "cams": [int(c) for c in cams], "fitness": 1.0, "correlation": 0.9}

    recs = []
    for i, (X, vis) in enumerate(scene.seeds[:6]):
        recs.append(rec("surface", X, synth._surface_normal(scene.obj, X), [c for c in vis if c % 8 >= i]))
    every = list(range(MR.N_CAMS))
    port, small, tiny = scene.cameras[MR.PORTRAIT], scene.cameras[MR.SMALL], scene.cameras[MR.TINY]
    recs.append(rec("portrait_border", back_project(port, 2.0, 160.0, 4.0), -port.optical_normal, every))
    recs.append(rec("portrait_border", back_project(port, 120.0, 317.5, 4.0), -port.optical_normal, every))
    recs.append(rec("climbs", back_project(small, 30.0, 60.0, 4.0), -small.optical_normal, every))
    recs.append(rec("climbs", back_project(small, 30.0, 60.0, 4.0), -small.optical_normal, [4, 5, 6, 7]))
    recs.append(rec("climbs_tiny", back_project(tiny, 18.0, 36.0, 4.0), -tiny.optical_normal, every))
    recs.append(rec("few_cams", scene.seeds[0][0], [0.0, 0.0, 1.0], [MR.TINY, MR.LARGE]))
    return recs


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "C"])
def test_gpu_loader_state_on_the_mixed_rig(rig, name):
    """pais_load_state_batch == po_mvs_load_patch in every field on hand-placed records: the reference camera by the normal,
    depth range from every listed camera's own projection, setLOD in the reference camera's own level sizes and maxLOD."""
    from oracle import po
    from tests.golden import make_resume_cloud as GR
    from tests.test_resume import _assert_loader_state, _loaded
    scene, cfg = _scene(rig, name), _cfg(name)
    recs = _loader_records(scene)
    assert len(recs) >= 8
    S = common.oracle_scene(cfg, scene)
    S.set_kernel_arithmetic(True)
    L = po.lib()
    ctx = P.context(cfg, scene.cameras)
    out = ctx.load_state_batch(_loaded(recs))
    mo = L.po_mvs_create(S.ptr)
    seen = {}
    for i, r in enumerate(recs):
        p = GR.oracle_load(S, mo, r)
        _assert_loader_state(out[i], p, i, (name, r["kind"]))
        by, q = GR.classify(S, p, r)
        assert bool(out[i].dropped) == (by is not None), (name, i, r["kind"], out[i].dropped, by)
        seen.setdefault(r["kind"], []).append((p.refCamIdx, q.LOD, by, GR.lod_fell_back(S, scene, q)))
    L.po_mvs_destroy(mo)
    ctx.close()
    S.close()
    assert len({MR.shape_class(ref) for ref, _, _, _ in seen["surface"]}) >= 4, seen["surface"]
    assert all(ref == MR.PORTRAIT and lod == 0 and by is None and fb for ref, lod, by, fb in seen["portrait_border"]), seen["portrait_border"]
    assert all(ref == MR.SMALL and lod >= 2 and by is None for ref, lod, by, _ in seen["climbs"]), seen["climbs"]
    assert all(ref == MR.TINY and lod >= 2 for ref, lod, _, _ in seen["climbs_tiny"]), seen["climbs_tiny"]
    assert seen["few_cams"][0][2] == "po_set_reference_camera"


# ---------------------------------------------------------------------------------------------------------------------
# reconstruction rounds
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "C"])
def test_gpu_reconstruction_rounds_on_the_mixed_rig(rig, name):
    """Seeds + 8 expansion rounds of B = 8 parents through the driver against the oracle's R(B) loop, patch for patch."""
    from oracle import po
    from pais_mvs_amd.mvs import MVS
    scene, cfg = _scene(rig, name), _cfg(name, particleNum=6, maxIteration=8)
    S = common.oracle_scene(cfg, scene)
    S.set_kernel_arithmetic(True)
    L = po.lib()
    mo = L.po_mvs_create(S.ptr)
    for X, vis in scene.seeds:
        L.po_mvs_add_seed(mo, po.darr(X), len(vis), po.iarr(vis))
    L.po_mvs_refine_seed_patches(mo)
    L.po_mvs_expansion_patches(mo, 8, 8, 1)
    want = []
    for i in range(L.po_mvs_num_slots(mo)):
        pp = L.po_mvs_get_patch(mo, i)
        if pp:
            p = pp.contents
            want.append((list(p.center[:]), list(p.normal[:]), p.cams(), p.fitness, p.correlation, p.priority, p.LOD))
    calls = L.po_mvs_refine_calls(mo)
    L.po_mvs_destroy(mo)
    S.close()
    m = MVS(cfg, scene.cameras, device=0, seed=42)
    for X, vis in scene.seeds:
        m.add_seed(X, vis)
    m.refineSeedPatches()
    m.expansionPatches(8, 8)
    got = [(list(p.center[:]), list(p.normal[:]), p.cams(), p.fitness, p.correlation, p.priority, p.lod) for p in m.patches()]
    st = m.stats()
    assert len(got) == len(want) and len(got) >= 100, (len(got), len(want))
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, (i, a, b)
    assert st.seeds_refined + st.candidates_effective == calls
    m.close()


# ---------------------------------------------------------------------------------------------------------------------
# pyramid construction at other ratios
# ---------------------------------------------------------------------------------------------------------------------
def _pyramid_strided(buf, w, h, stride, lod_ratio, cfg_max_lod=15):
    """pais_pyramid_build on a buffer whose rows are `stride` bytes apart (camera.build_pyramid_gpu passes stride = w)."""
    from pais_mvs_amd import _lib

    class _Pyr(C.Structure):
        _fields_ = [("max_lod", C.c_int), ("width", C.c_int * 16), ("height", C.c_int * 16),
                    ("image", C.POINTER(C.c_uint8) * 16), ("edge", C.POINTER(C.c_double) * 16), ("kernel_ms", C.c_double)]
    L = _lib.load()
    L.pais_pyramid_build.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_double, C.c_int, C.c_int,
                                     C.POINTER(C.POINTER(_Pyr))]
    L.pais_pyramid_free.argtypes = [C.POINTER(_Pyr)]
    L.pais_pyramid_free.restype = None
    L.pais_pyramid_last_error.restype = C.c_char_p
    out = C.POINTER(_Pyr)()
    rc = L.pais_pyramid_build(0, buf.ctypes.data, w, h, stride, float(lod_ratio), cfg_max_lod, 1, C.byref(out))
    assert rc == 0, L.pais_pyramid_last_error().decode()
    try:
        p = out.contents
        levels, edges = [], []
        for l in range(p.max_lod + 1):
            n = p.width[l] * p.height[l]
            levels.append(np.ctypeslib.as_array(p.image[l], shape=(n,)).reshape(p.height[l], p.width[l]).copy())
            edges.append(np.ctypeslib.as_array(p.edge[l], shape=(n,)).reshape(p.height[l], p.width[l]).copy())
        return levels, edges
    finally:
        L.pais_pyramid_free(out)


def _halved(img):
    """Level 1 at lodRatio 0.5 of an image of even sizes in closed form: the round-half-even mean of each 2 x 2 block, in
    integers (sum / 4 with remainder 2 rounding to the even quotient)."""
    a = img.astype(np.int64)
    s = a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2]
    q, r = s // 4, s % 4
    return (q + ((r > 2) | ((r == 2) & (q % 2 == 1)))).astype(np.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("ratio", [0.5, 0.7, 0.9])
def test_gpu_pyramid_at_other_ratios(rig, ratio):
    """build_pyramid_gpu at lodRatio 0.5, 0.7, 0.9 against resize_area / sobel_magnitude_normalised bit for bit: thin, odd and
    one-pixel-wide shapes, a constant image, the rig's own level-0 images, and a 130-wide image inside a 192-byte-stride
    buffer through the C entry.  At 0.5 with even sizes level 1 is also the 2 x 2 block mean in closed form."""
    from pais_mvs_amd.camera import build_pyramid_gpu, max_lod, resize_area, sobel_magnitude_normalised
    rng = np.random.default_rng(17)
    images = [rng.integers(0, 256, size=(h, w), dtype=np.uint8) for w, h in ((257, 17), (255, 16), (1, 40), (40, 1))]
    images.append(np.full((64, 64), 137, dtype=np.uint8))
    images.append(rng.integers(0, 256, size=(48, 96), dtype=np.uint8))
    images += [cam.pyramid[0] for cam in rig.cameras[:8]]

    def check(levels, edges, img, what):
        h, w = img.shape
        assert len(levels) == len(edges) == max_lod(w, h, ratio, 15) + 1, what
        assert np.array_equal(levels[0], img), what
        for i in range(len(levels)):
            if i > 0:
                want = resize_area(img, ratio ** i)
                assert levels[i].shape == want.shape and np.array_equal(levels[i], want), (what, i)
            assert np.array_equal(edges[i], sobel_magnitude_normalised(levels[i])), (what, i)
        if ratio == 0.5 and h % 2 == 0 and w % 2 == 0 and len(levels) > 1:
            assert np.array_equal(levels[1], _halved(img)), what

    for n, img in enumerate(images):
        levels, edges, _ = build_pyramid_gpu(img, ratio, 15, True, device=0)
        check(levels, edges, img, (ratio, n, img.shape))
    buf = rng.integers(0, 256, size=(37, 192), dtype=np.uint8)
    levels, edges = _pyramid_strided(buf, 130, 37, 192, ratio)
    check(levels, edges, np.ascontiguousarray(buf[:, :130]), (ratio, "stride 192"))
