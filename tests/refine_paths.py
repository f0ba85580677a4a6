"""The branch census of refine(): which of its decisions one candidate takes, told by the oracle alone.

`refine_paths` restates po_refine (patch.cpp:114-176) and the driver's trailing removeInvisibleCamera (mvs.cpp:215 / :574)
statement by statement from the oracle's own setters, the way tests/test_pso_trace.py traced_refine does, and notes on the way
every branch the HIP after-stage treats on its own (pais_kernels.hip k_begin / k_after): the drops and where they happen, the
clamps of setDepthRange, the number of PSO runs, how the seed loop ends, and which follow-up stage k_after would choose
(PAIS_STAGE_AFTER2_SAME / _KEEP / AFTER2).  Nothing here looks at the code under test; the restated record must equal
common.oracle_refine_patch's byte for byte (tests/test_threshold_sweep.py asserts it for every candidate of every row), which is
what makes a tag trustworthy.
"""
import ctypes as C

from tests import common

# every tag refine_paths can return
HEAD_DROP_MINCAM = "head drop: fewer than minCamNum cameras"
HEAD_DROP_SETTER = "head drop: a setter before the first PSO run"
LOD_UP = "LOD > 0"
RANGE_LO_CLAMPED = "depth range: lower bound clamped to 0"
RANGE_HI_CAPPED = "depth range: upper bound capped by neighborRadius * 100"
RUNS = {1: "1 PSO run", 2: "2 PSO runs", 3: "3 PSO runs", 4: "4 or more PSO runs"}
MAXFIT_DROP = {1: "maxFitness drop after run 1", 2: "maxFitness drop after run 2", 3: "maxFitness drop after run 3 or later"}
REMOVAL_DROP_WINDOW = "drop in a removal of refine(): a warped window leaves its image (correlation == 0)"
REMOVAL_DROP_FEW = "drop in a removal of refine(): fewer than minCamNum cameras left"
LOOP_DROP_MINCAM = "drop at the head of a loop trip: fewer than minCamNum cameras"
LOOP_COUNT_GUARD = "seed loop ended by its count guard"
SETTER_DROP_AFTER_REMOVAL = "drop by a setter after a removal"
FINAL_SAME = "final stage SAME"
FINAL_KEEP = "final stage KEEP"
FINAL_AFTER2_REF = "final stage AFTER2: the reference camera changed"
FINAL_AFTER2_LOD = "final stage AFTER2: the LOD alone changed"
SEED_NOT_SAME = "a seed ends in KEEP / AFTER2"
TRAILING_REMOVED = "trailing removal removed a camera"
TRAILING_DROP = "trailing removal dropped the record"

ALL_TAGS = frozenset((HEAD_DROP_MINCAM, HEAD_DROP_SETTER, LOD_UP, RANGE_LO_CLAMPED, RANGE_HI_CAPPED, REMOVAL_DROP_WINDOW,
                      REMOVAL_DROP_FEW, LOOP_DROP_MINCAM, LOOP_COUNT_GUARD, SETTER_DROP_AFTER_REMOVAL, FINAL_SAME, FINAL_KEEP,
                      FINAL_AFTER2_REF, FINAL_AFTER2_LOD, SEED_NOT_SAME, TRAILING_REMOVED, TRAILING_DROP)
                     + tuple(RUNS.values()) + tuple(MAXFIT_DROP.values()))


def patch_bytes(p):
    return C.string_at(C.addressof(p), C.sizeof(p))


def _window_leaves_an_image(S, L, p):
    """Would the removal's setCorrelationTable drop p (getHomographyPatch: a warped sample outside an image)?  On a copy."""
    from oracle import po
    q = common.copy_struct(p)
    H = (C.c_double * (9 * po.MAX_VIS))()
    L.po_homographies(S.ptr, C.byref(q), q.center, q.normal, H)
    L.po_set_correlation_table(S.ptr, C.byref(q), H)
    return bool(q.drop)


def _note_state(S, p, tags):
    """What the setter chain left for the next PSO run / the record: the level and the two clamps of setDepthRange."""
    cfg = S.ptr.contents.cfg
    if p.LOD > 0:
        tags.add(LOD_UP)
    if p.depthRange[0] == 0.0:                                        # max(depth - maxWorldDist * depthRangeScalar, 0.0)
        tags.add(RANGE_LO_CLAMPED)
    if p.depthRange[1] == p.depth + cfg.neighborRadius * 100:         # depth + min(maxWorldDist * depthRangeScalar, that)
        tags.add(RANGE_HI_CAPPED)


def refine_paths(S, p, is_seed):
    """refine() and the trailing removeInvisibleCamera of the constructed patch p (common.oracle_patch_from_candidate) as
    common.oracle_refine_patch runs them; p is refined in place.  Returns the set of tags of the branches taken."""
    from oracle import po
    L = po.lib()
    s, cfg = S.ptr, S.ptr.contents.cfg
    ref = C.byref(p)
    tags = set()
    setters = (L.po_set_reference_camera, L.po_set_depth_and_ray, L.po_set_depth_range, L.po_set_lod)

    def refine():
        if p.numCam < cfg.minCamNum:                                  # patch.cpp:118-123
            p.fitness = common.DBL_MAX
            p.priority = common.DBL_MAX
            p.drop = 1
            tags.add(HEAD_DROP_MINCAM)
            return
        for f in setters:
            f(s, ref)
        if p.drop:
            tags.add(HEAD_DROP_SETTER)
            return
        _note_state(S, p, tags)
        before_ref, after_ref, before_num, after_num = p.refCamIdx, -1, p.numCam, -1
        count, total = 0, p.numCam
        final = None
        while True:
            if not (before_ref != after_ref or before_num != after_num):
                break
            c, count = count, count + 1                               # `count++ <= totalCamNum`
            if not c <= total:
                tags.add(LOOP_COUNT_GUARD)
                break
            if p.numCam < cfg.minCamNum:                              # :142-147
                p.fitness = common.DBL_MAX
                p.priority = common.DBL_MAX
                p.drop = 1
                tags.add(LOOP_DROP_MINCAM)
                return
            before_ref, before_num = p.refCamIdx, p.numCam
            L.po_pso_optimization(s, ref)
            if p.fitness > cfg.maxFitness:
                p.drop = 1
                tags.add(MAXFIT_DROP[min(p.psoRuns, 3)])
                return
            was_dropped = bool(p.drop)
            ref0, lod0, num0 = p.refCamIdx, p.LOD, p.numCam
            window = (not was_dropped) and _window_leaves_an_image(S, L, p)
            L.po_remove_invisible_camera(s, ref)
            if p.drop and not was_dropped:
                tags.add(REMOVAL_DROP_WINDOW if window else REMOVAL_DROP_FEW)
            removed_none = p.numCam == num0
            dropped_by_removal = bool(p.drop)
            for f in setters:
                f(s, ref)
            if p.drop and not dropped_by_removal:
                tags.add(SETTER_DROP_AFTER_REMOVAL)
            if not p.drop:
                _note_state(S, p, tags)
            # the stage k_after chooses for the driver's removal when the loop ends here
            if p.refCamIdx != ref0:
                final = FINAL_AFTER2_REF
            elif p.LOD != lod0:
                final = FINAL_AFTER2_LOD
            else:
                final = FINAL_SAME if removed_none else FINAL_KEEP
            if p.type == 1:
                break
            after_ref, after_num = p.refCamIdx, p.numCam
        L.po_set_priority(s, ref)
        L.po_set_image_point(s, ref)
        if not p.drop and final is not None:
            tags.add(final)
            if is_seed and final != FINAL_SAME:
                tags.add(SEED_NOT_SAME)

    if not is_seed and p.numCam < cfg.minCamNum:
        p.drop = 1                                                    # expandVisibleCamera :758-760
    refine()
    if p.psoRuns:
        tags.add(RUNS[min(p.psoRuns, 4)])
    alive, num = not p.drop, p.numCam
    L.po_remove_invisible_camera(s, ref)                              # mvs.cpp:215 / 574
    if alive:
        if p.numCam < num:
            tags.add(TRAILING_REMOVED)
        if p.drop:
            tags.add(TRAILING_DROP)
    return tags
