"""pais_fitness_detail: PAIS::getFitness (patch.cpp:914-1047) with its per-pixel breakdown -- the weight, avgSad, colours and
pixel codes of the window walk, the homographies of Patch::getHomographies (patch.cpp:290-330) and the outcome of the
evaluation.

The checker is a per-pixel restatement here (`restate`): the reference's statements of the literal arithmetic in numpy, one
operation at a time, on refcost's walk, warp, bilinear, homographies and distance table, with the oracle's deterministic exp /
sin / cos.  On the CPU it is pinned against tests/refcost.py and the oracle's costLiteral; on the GPU the call's maps are
checked against it pixel by pixel, and its fitness against pais_fitness_batch under PAIS_ARITH=literal bit for bit.
"""
import ctypes as C
import math

import numpy as np
import pytest

from tests import common, pipelines as P, refcost
from tests.common import DBL_MAX

MARGIN = 1e-7               # refcost margins below this: two arithmetics may decide differently (tests/test_radius_sweep.py)
RTOL_KERNEL = 1e-9          # the default (kernel) arithmetic against the literal one
R = (1, 2, 15, 31, 32, 63, 127)
WEIGHTS = [(1, 1, 0), (1, 1, 1), (0, 0, 0), (0, 1, 1), (1, 0, 0)]     # the flag combinations of test_fitness_batch_matches_oracle
OK, BACKFACING, OFF_IMAGE, WINDOW, OVERFLOW, ALL_MASKED = 0, 1, 2, 3, 4, 5
COUNTED, MASKED, PIX_OVERFLOW, NONE = 0, 1, 2, 3


def _cfg(r, weights=(1, 1, 0), **over):
    from pais_mvs_amd.config import readme_config
    return readme_config(patchRadius=r, distWeighting=r / 3.0, adaptiveDistanceEnable=bool(weights[0]),
                         adaptiveDifferenceEnable=bool(weights[1]), adaptiveGradientEnable=bool(weights[2]), **over)


def _det_normal(th, ph):
    from oracle import po
    L = po.lib()
    return refcost.spherical_to_normal(th, ph, sin=L.po_sin_det, cos=L.po_cos_det)


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------
def restate(scene, cfg, st, pos, H=None, pt=None, gauss=None):
    """The literal cost of particle pos of state st, pixel by pixel (maps in walk order, k = xi * S + yi).  H (K x 3 x 3) and
    pt: use these instead of refcost's homographies and projection (what the GPU returned), so that the per-pixel statements
    are compared on their own; gauss: the distance table (default refcost.gauss_table)."""
    from oracle import po
    exp = po.lib().po_exp_det
    cams = scene.cameras
    S, r, K = int(cfg.patchSize), int(cfg.patchRadius), len(st.cams)
    S2 = S * S
    out = dict(outcome=None, value=DBL_MAX, sw=0.0, fit=0.0, pt=(0.0, 0.0), nx=0, ny=0, live=0, ov_pix=-1, ov_cam=-1, H=None,
               weight=np.zeros(S2), sad=np.zeros(S2), code=np.full(S2, NONE, dtype=np.int8), colour=np.zeros((K, S2)))
    th, ph, depth = (float(v) for v in pos)
    n = _det_normal(th, ph)
    rc = cams[st.ref]
    if refcost._dot3(n, rc.optical_normal) > 0:                                        # :939
        out["outcome"] = BACKFACING
        return out
    center = [float(st.ray[i]) * depth + float(rc.center[i]) for i in range(3)]       # :944
    out["H"] = H = refcost.homographies(cams, st, center, n, cfg.lodRatio) if H is None else [np.asarray(h).reshape(3, 3) for h in H]
    lod = st.lod
    if pt is None:
        pt = refcost.project(rc, center, cfg.lodRatio ** lod)
    out["pt"] = pt = (float(pt[0]), float(pt[1]))
    if lod > rc.max_lod:
        out["outcome"] = OFF_IMAGE
        return out
    ref_img = rc.pyramid[lod]
    rows, cols = ref_img.shape
    if not (pt[0] == pt[0] and pt[1] == pt[1] and 0 <= pt[0] < cols and 0 <= pt[1] < rows):   # :952
        out["outcome"] = OFF_IMAGE
        return out
    if pt[0] - r < 2 or pt[0] + r >= cols - 3 or pt[1] - r < 2 or pt[1] + r >= rows - 3:      # :957-962
        out["outcome"] = WINDOW
        return out
    xs, ys = refcost._walk(pt[0] - r, pt[0] + r)[:S], refcost._walk(pt[1] - r, pt[1] + r)[:S]   # :979-980
    nx, ny = len(xs), len(ys)
    total = nx * ny
    X, Y = np.repeat(xs, ny), np.tile(ys, nx)
    rx, ry = refcost.cv_round(X), refcost.cv_round(Y)
    live = ref_img[ry, rx] != 0                                                          # :986
    colour = np.zeros((K, total))
    bad_any = np.zeros(total, dtype=bool)
    first_bad = np.full(total, -1)
    for i, c in enumerate(st.cams):
        crows, ccols = refcost.level_shape(cams[c], lod)                                  # (an absent level: (0, 0), no tap passes)
        w, ix, iy = refcost._warp(H[i], X, Y)                                             # :994-996
        bad = (ix < 2) | (ix >= ccols - 3) | (iy < 2) | (iy >= crows - 3) | (w == 0) | np.isnan(ix) | np.isnan(iy)   # :999
        first_bad[(first_bad < 0) & bad] = i
        bad_any |= bad
        if not bad.all():   # (a pixel with a bad tap is never COUNTED: its colours are not part of the result)
            colour[i][~bad] = refcost._bilinear(cams[c].pyramid[lod], ix[~bad], iy[~bad])   # :1014-1017
    over, counted = live & bad_any, live & ~bad_any
    mean = np.zeros(total)
    for i in range(K):
        mean = mean + colour[i]
    mean = mean / K                                                                      # :1022
    sad = np.zeros(total)
    for i in range(K):
        sad = sad + np.abs(colour[i] - mean)
    sad = sad / K                                                                        # :1027
    weight = np.ones(total)
    if cfg.adaptiveDistanceEnable:
        weight = weight * (refcost.gauss_table(cfg) if gauss is None else gauss)[:total]  # :1031
    if cfg.adaptiveDifferenceEnable:
        e = np.ones(total)
        e[counted] = [exp(v) for v in (-sad[counted] * sad[counted] / cfg.diffWeighting).tolist()]
        weight = weight * e                                                              # :1034
    if cfg.adaptiveGradientEnable:
        edge = rc.edge_pyramid[lod][ry, rx]
        e = np.ones(total)
        with np.errstate(divide="ignore"):                                               # (edge 0: exp(-inf) = 0)
            e[counted] = [exp(v) for v in (-1.0 / (edge[counted] * cfg.gradientWeighting)).tolist()]
        weight = weight * e                                                              # :1037
    nan = np.full(total, np.nan)
    out["weight"][:total] = np.where(counted, weight, np.where(over, nan, 0.0))
    out["sad"][:total] = np.where(counted, sad, np.where(over, nan, 0.0))
    out["colour"][:, :total] = np.where(counted, colour, np.where(over, nan, 0.0))
    out["code"][:total] = np.where(counted, COUNTED, np.where(over, PIX_OVERFLOW, MASKED))
    sw, fit = _seq_sums(out["weight"], out["sad"], out["code"])                          # :1040-1041
    out.update(nx=nx, ny=ny, live=int(counted.sum()), sw=sw, fit=fit)
    if over.any():
        k = int(np.argmax(over))
        out.update(outcome=OVERFLOW, ov_pix=k, ov_cam=int(first_bad[k]))
    else:
        out["outcome"] = ALL_MASKED if not counted.any() else OK
        with np.errstate(invalid="ignore", divide="ignore"):
            out["value"] = float(np.float64(fit) / np.float64(sw))                        # :1046
    return out


def _library_gauss(cfg):
    """The distance table as the library builds it (pais_capi.hip build_gauss, mvs.cpp:97-114): normalised by a sequential sum
    where refcost.gauss_table takes an exactly rounded one, so that the two differ in the last bits."""
    r, S, sigma = int(cfg.patchRadius), int(cfg.patchSize), float(cfg.distWeighting)
    s2 = 1.0 / (2.0 * sigma * sigma)
    s = 1.0 / (2.0 * math.pi * sigma * sigma)
    g = [s * math.exp(-(float(x - r) ** 2 + float(y - r) ** 2) * s2) for x in range(S) for y in range(S)]
    n = 0.0
    for v in g:
        n += v
    inv = 1.0 / n
    return np.array([v * inv for v in g])


def _seq_sums(weight, sad, code):
    """sumWeight and fitness of :1040-1041: left-to-right over the COUNTED pixels in walk order (np.add.accumulate is a
    strictly sequential sum)."""
    m = np.asarray(code).ravel() == COUNTED
    w = np.asarray(weight).ravel()[m]
    if not len(w):
        return 0.0, 0.0
    return float(np.add.accumulate(w)[-1]), float(np.add.accumulate(w * np.asarray(sad).ravel()[m])[-1])


def _outcome_of(c):
    """refcost.Cost -> the outcome code (OFF_IMAGE and WINDOW are one refcost outcome)."""
    if c.outcome == "backfacing":
        return (BACKFACING,)
    if c.outcome == "outside":
        return (OFF_IMAGE, WINDOW)
    if c.outcome == "overflow":
        return (OVERFLOW,)
    return (OK,) if c.live_pixels else (ALL_MASKED,)      # (OK with NaN fitness: live pixels whose weights all vanish)


# ---------------------------------------------------------------------------------------------------------------------
# states and particles
# ---------------------------------------------------------------------------------------------------------------------
def _scene(request, r):
    return request.getfixturevalue("pawn_small" if r <= 20 else "ring_small")


_CASES = {}


def _case(request, r, weights=(1, 1, 0), scene_name=None):
    """States, particles (tests/test_gpu_parity.py's kinds plus test_radius_sweep.py's corner and edge-on planes) and refcost's
    cost of each evaluation."""
    key = (r, weights, scene_name)
    if key in _CASES:
        return _CASES[key]
    from tests.test_gpu_parity import _states_and_particles
    from tests.test_radius_sweep import _corner_particles, _edge_on_particles
    scene = request.getfixturevalue(scene_name) if scene_name else _scene(request, r)
    cfg = _cfg(r, weights, **({"reduceNormalRange": 4.0} if scene_name == "dome_small" else {}))
    S = common.oracle_scene(cfg, scene)
    rng = np.random.default_rng(500 + r)
    states, pats, idx, parts = _states_and_particles(S, scene, rng, n_per=12)
    for si, p in enumerate(pats[:4]):
        st = refcost.state_of(p)
        base = (p.normalS[0], p.normalS[1], p.depth)
        for pos in _corner_particles(scene, cfg, st, base) + _edge_on_particles(scene, cfg, st, base):
            idx.append(si)
            parts.append(list(pos))
    ref = [refcost.cost(scene, cfg, refcost.state_of(pats[si]), pos, normal_fn=_det_normal) for si, pos in zip(idx, parts)]
    case = dict(scene=scene, cfg=cfg, S=S, states=states, pats=pats, idx=idx, parts=parts, ref=ref)
    _CASES[key] = case
    return case


def _ray_through(cam, u, v, lod_scale):
    """A world direction whose points project to pixel (u, v) of the camera's level (project: R (C + t d) + T = t [x, y, 1])."""
    x = (u / lod_scale - float(cam.principle_point[0])) / float(cam.focal[0])
    y = (v / lod_scale - float(cam.principle_point[1])) / float(cam.focal[1])
    return np.asarray(cam.rotation, float).T @ np.array([x, y, 1.0])


def _facing(ray):
    """(theta, phi) of the normal that faces the camera along ray (normal2Spherical of -ray)."""
    n = -np.asarray(ray, float) / np.linalg.norm(ray)
    return math.acos(float(n[2])), math.atan2(float(n[1]), float(n[0]))


def _state(ray, ref, lod, cams):
    from pais_mvs_amd import _lib
    s = _lib.PatchState()
    s.ray[:] = [float(v) for v in ray]
    s.ref_cam, s.lod, s.num_cam = int(ref), int(lod), len(cams)
    for i, c in enumerate(cams):
        s.cam_idx[i] = int(c)
    return s


# ------------------------------------------------------------------------------------------------------------- CPU ---
def test_sizeof_cost_detail_matches_the_ctypes_mirror():
    from pais_mvs_amd import _lib
    L = _lib.load()
    assert L.pais_sizeof_cost_detail() == C.sizeof(_lib.CostDetail) == 8 * 5 + 4 * 8


def test_state_and_particle_from_record():
    from pais_mvs_amd import _lib
    from pais_mvs_amd.context import particle_from_record, patch_state_from_record
    r = _lib.PatchResult()
    r.ray[:] = [0.1, -0.2, 0.97]
    r.normalS[:] = [2.5, -1.25]
    r.depth = 3.75
    r.ref_cam, r.lod, r.num_cam = 2, 1, 3
    for i, c in enumerate([4, 2, 0]):
        r.cam_idx[i] = c
    r.cam_idx[3] = 99                                  # beyond num_cam: not part of the state
    assert bytes(patch_state_from_record(r)) == bytes(_state([0.1, -0.2, 0.97], 2, 1, [4, 2, 0]))
    assert particle_from_record(r) == [2.5, -1.25, 3.75]


@pytest.mark.parametrize("scene_name,r,weights", [("pawn_small", 15, (1, 1, 0)), ("ring_small", 15, (1, 1, 1)),
                                                  ("dome_small", 25, (1, 1, 1))])
def test_restatement_sums_give_the_cost(request, scene_name, r, weights):
    """The restatement's sequential sums of weight and weight * avgSad over its COUNTED pixels give refcost.cost and the
    oracle's costLiteral within refcost.literal_gate(S); its outcome is refcost's wherever the margin allows."""
    case = _case(request, r, weights, scene_name)
    scene, cfg, S = case["scene"], case["cfg"], case["S"]
    gate = refcost.literal_gate(2 * r + 1)
    S.set_kernel_arithmetic(True)
    S.set_cost_literal(True)
    n = {k: 0 for k in (OK, BACKFACING, OFF_IMAGE, WINDOW, OVERFLOW, ALL_MASKED)}
    skipped = 0
    for e, (si, pos) in enumerate(zip(case["idx"], case["parts"])):
        c = case["ref"][e]
        if c.margin < MARGIN:
            skipped += 1
            continue
        got = restate(scene, cfg, refcost.state_of(case["pats"][si]), pos)
        assert got["outcome"] in _outcome_of(c), (e, got["outcome"], c.outcome)
        n[got["outcome"]] += 1
        clit = S.fitness(case["pats"][si], pos)
        if got["outcome"] != OK:
            assert got["value"] == clit == c.value or (math.isnan(got["value"]) and math.isnan(clit)), (e, got["value"], clit)
            continue
        assert got["live"] == int(np.sum(got["code"] == COUNTED)) > 0
        assert got["value"] == got["fit"] / got["sw"]
        assert abs(got["value"] - c.value) <= gate * abs(c.value), (e, got["value"], c.value)
        assert abs(got["value"] - clit) <= gate * abs(clit), (e, got["value"], clit)
    S.set_cost_literal(False)
    assert n[OK] >= 20 and n[BACKFACING] >= 5 and n[OVERFLOW] + n[WINDOW] + n[OFF_IMAGE] >= 5, n
    assert skipped <= max(2, len(case["parts"]) // 50), skipped


# ------------------------------------------------------------------------------------------------------------- GPU ---
def _ctx(cfg, scene, monkeypatch, literal=False):
    return P.context(cfg, scene.cameras, monkeypatch, P.LITERAL if literal else {})


def _check_identity(d, lit, what):
    """fitness == fitness_batch under PAIS_ARITH=literal bit for bit; plain sequential sums over the COUNTED pixels give
    sum_weight, sum_weighted_sad and the fitness."""
    assert d.fitness.tobytes() == np.asarray(lit, dtype=np.float64).tobytes(), (what, np.flatnonzero(d.fitness.view(np.int64) != np.asarray(lit).view(np.int64)))
    for e in range(len(d)):
        oc = int(d.outcome[e])
        assert int(d.live_pixels[e]) == int(np.sum(d.code[e] == COUNTED)), (what, e)
        sw, fit = _seq_sums(d.weight[e], d.avg_sad[e], d.code[e])
        assert (sw, fit) == (float(d.sum_weight[e]), float(d.sum_weighted_sad[e])), (what, e, sw, d.sum_weight[e], fit, d.sum_weighted_sad[e])
        if oc in (OK, ALL_MASKED):
            with np.errstate(invalid="ignore", divide="ignore"):
                v = np.float64(fit) / np.float64(sw)
            assert np.array_equal(v, d.fitness[e], equal_nan=True), (what, e, v, d.fitness[e])
            assert (oc == ALL_MASKED) == (d.live_pixels[e] == 0), (what, e)
        else:
            assert d.fitness[e] == DBL_MAX, (what, e, oc)
        if oc in (BACKFACING, OFF_IMAGE, WINDOW):
            assert (d.code[e] == NONE).all() and not d.weight[e].any() and not d.avg_sad[e].any(), (what, e)
        if oc == OVERFLOW:
            assert d.overflow_pixel[e] >= 0 and d.overflow_cam[e] >= 0
            assert d.code[e].ravel()[d.overflow_pixel[e]] == PIX_OVERFLOW
        else:
            assert d.overflow_pixel[e] == -1 and d.overflow_cam[e] == -1
        pix = d.code[e] == PIX_OVERFLOW
        assert (oc == OVERFLOW) == bool(pix.any()) and np.isnan(d.weight[e][pix]).all()
        quiet = (d.code[e] == MASKED) | (d.code[e] == NONE)
        assert not d.weight[e][quiet].any() and not d.avg_sad[e][quiet].any()


def _check_pixels(d, e, scene, cfg, st, pos, what):
    """Evaluation e of d against the restatement from the returned H and pt: colours and avgSad bit for bit, weight within
    2 ulp (the library's distance table restated: exp may differ in the last bit), the codes, the outcome fields; H within
    1e-12 of refcost's."""
    K = len(st.cams)
    H = d.homographies[e, :K]
    want = restate(scene, cfg, st, pos, H=H, pt=d.pt[e], gauss=_library_gauss(cfg))
    assert int(d.outcome[e]) == want["outcome"], (what, e, d.outcome[e], want["outcome"])
    assert (int(d.nx[e]), int(d.ny[e]), int(d.live_pixels[e])) == (want["nx"], want["ny"], want["live"]), (what, e)
    assert (int(d.overflow_pixel[e]), int(d.overflow_cam[e])) == (want["ov_pix"], want["ov_cam"]), (what, e)
    assert np.array_equal(d.code[e].ravel(), want["code"]), (what, e)
    assert d.avg_sad[e].ravel().tobytes() == want["sad"].tobytes(), (what, e)
    assert d.colour[e, :K].reshape(K, -1).tobytes() == want["colour"].tobytes(), (what, e)
    w, ww = d.weight[e].ravel(), want["weight"]
    assert np.array_equal(np.isnan(w), np.isnan(ww))
    ok = ~np.isnan(ww)
    assert (np.abs(w[ok] - ww[ok]) <= 2 * np.spacing(np.abs(ww[ok]))).all(), (what, e, float(np.max(np.abs(w[ok] - ww[ok]))))
    rc = scene.cameras[st.ref]
    th, ph, depth = (float(v) for v in pos)
    n = _det_normal(th, ph)
    center = [float(st.ray[i]) * depth + float(rc.center[i]) for i in range(3)]
    pt = refcost.project(rc, center, cfg.lodRatio ** st.lod)
    if want["outcome"] == BACKFACING:
        assert not H.any() and not d.pt[e].any(), (what, e)
        return
    assert max(abs(pt[0] - d.pt[e, 0]), abs(pt[1] - d.pt[e, 1])) <= 1e-12 * max(1.0, abs(pt[0]), abs(pt[1])), (what, e, pt, d.pt[e])
    for i, h in enumerate(refcost.homographies(scene.cameras, st, center, n, cfg.lodRatio)):
        assert np.max(np.abs(H[i] - h.ravel())) <= 1e-12 * np.max(np.abs(h)), (what, e, i, H[i], h.ravel())


def _pick(d, n):
    """Up to n evaluations of each walked outcome (OK, OVERFLOW, ALL_MASKED) and every other one."""
    picks, seen = [], {}
    for e in range(len(d)):
        oc = int(d.outcome[e])
        if seen.get(oc, 0) < (n if oc in (OK, OVERFLOW, ALL_MASKED) else 2):
            seen[oc] = seen.get(oc, 0) + 1
            picks.append(e)
    return picks


@pytest.mark.gpu
@pytest.mark.parametrize("r,weights", [(r, (1, 1, 0)) for r in R] + [(15, w) for w in WEIGHTS[1:]])
def test_gpu_fitness_detail_identity_and_pixels(request, r, weights, monkeypatch):
    """Identity: fitness equals fitness_batch under PAIS_ARITH=literal bit for bit, on a context of either arithmetic; sums
    over the COUNTED pixels give the record; the default arithmetic's fitness_batch within 1e-9 where refcost's margin
    allows.  Per pixel: maps, colours, codes and H of a few evaluations of each outcome against the restatement."""
    case = _case(request, r, weights)
    scene, cfg = case["scene"], case["cfg"]
    states, idx, parts = case["states"], case["idx"], case["parts"]
    ctx = _ctx(cfg, scene, monkeypatch)
    lit_ctx = _ctx(cfg, scene, monkeypatch, literal=True)
    d = ctx.fitness_detail(states, idx, parts, colours=True, homographies=True)
    d2 = lit_ctx.fitness_detail(states, idx, parts, colours=True, homographies=True)
    lit = lit_ctx.fitness_batch(states, idx, parts)
    ker = ctx.fitness_batch(states, idx, parts)
    for a in ("fitness", "weight", "avg_sad", "code", "colour", "homographies", "pt"):
        assert getattr(d, a).tobytes() == getattr(d2, a).tobytes(), (r, a)
    _check_identity(d, lit, (r, weights))
    n_fin = skipped = 0
    for e, c in enumerate(case["ref"]):
        if c.margin < MARGIN:
            skipped += 1
            continue
        assert int(d.outcome[e]) in _outcome_of(c), (r, e, d.outcome[e], c.outcome)
        if d.outcome[e] == OK:
            n_fin += 1
            assert common.same_value(float(d.fitness[e]), float(ker[e]), RTOL_KERNEL), (r, e, d.fitness[e], ker[e])
        else:
            assert common.same_value(float(d.fitness[e]), float(ker[e]), 0.0), (r, e, d.outcome[e], d.fitness[e], ker[e])
    assert skipped <= max(2, len(parts) // 50), (r, skipped)
    assert n_fin >= 3, (r, n_fin)
    for e in _pick(d, 3 if r >= 63 else 6):
        _check_pixels(d, e, scene, cfg, refcost.state_of(states[idx[e]]), parts[e], (r, weights))
    # the window-image helpers
    e = int(np.flatnonzero(d.outcome == OK)[0])
    img = d.error_image(e)
    counted = d.code[e].T == COUNTED
    assert img.shape == (cfg.patchSize,) * 2 and np.nanmin(img) == 0.0 and np.nanmax(img) <= 1.0 and np.isnan(img[~counted]).all()
    corners = d.window_corners(e)
    ref_pos = int(d.ref_pos[e])
    if ref_pos >= 0:
        pt, rr = d.pt[e], cfg.patchRadius
        want = np.rint([[pt[0] - rr, pt[1] - rr], [pt[0] - rr, pt[1] + rr], [pt[0] + rr, pt[1] - rr], [pt[0] + rr, pt[1] + rr], pt])
        assert np.array_equal(corners[ref_pos], want), (corners[ref_pos], want)
    ctx.close()
    lit_ctx.close()


@pytest.mark.gpu
def test_gpu_fitness_detail_every_outcome(request, monkeypatch):
    """Particles and states that end in each outcome, checked against the restatement pixel by pixel: back-facing, a ray off
    the image, a window across the border, the corner and sign-changing-w particles of test_radius_sweep.py (overflow: the
    first bad pixel and camera), a window on the masked background (NaN); a state that lists its reference camera twice and
    one whose reference camera is not in cam_idx."""
    r = 15
    case = _case(request, r)
    scene, cfg = case["scene"], case["cfg"]
    p0 = case["pats"][0]
    st0 = refcost.state_of(p0)
    rc = scene.cameras[st0.ref]
    lod = st0.lod
    sc = cfg.lodRatio ** lod
    img = rc.pyramid[lod]
    rows, cols = img.shape
    th0, ph0, dp0 = float(p0.normalS[0]), float(p0.normalS[1]), float(p0.depth)
    others = [c for c in st0.cams if c != st0.ref]
    states, parts, idx = [], [], []

    def add(ray, cams, pos, ref=st0.ref, lod_=lod):
        states.append(_state(ray, ref, lod_, cams))
        idx.append(len(states) - 1)
        parts.append(list(pos))

    ray0 = [float(v) for v in p0.ray[:]]
    add(ray0, st0.cams, (math.pi - th0, ph0 + math.pi, dp0))                         # back-facing
    ray = _ray_through(rc, cols + 40.0, rows / 2.0, sc)                              # projects beyond the image
    add(ray, st0.cams, (*_facing(ray), dp0))
    ray = _ray_through(rc, cols / 2.0, -30.0, sc)                                    # ... above it
    add(ray, st0.cams, (*_facing(ray), dp0))
    ray = _ray_through(rc, r - 5.0, rows / 2.0, sc)                                  # window across the left border
    add(ray, st0.cams, (*_facing(ray), dp0))
    # a window on the masked background
    bg = None
    for v in range(r + 3, rows - r - 4, 7):
        for u in range(r + 3, cols - r - 4, 7):
            if not img[v - r - 1:v + r + 2, u - r - 1:u + r + 2].any():
                bg = (u, v)
                break
        if bg:
            break
    assert bg is not None
    ray = _ray_through(rc, bg[0] + 0.25, bg[1] + 0.25, sc)
    add(ray, st0.cams, (*_facing(ray), dp0))
    # the reference camera listed twice; the reference camera absent
    add(ray0, st0.cams + [st0.ref], (th0, ph0, dp0))
    add(ray0, others, (th0, ph0, dp0))
    add(ray0, [others[0], st0.ref] + others[1:] + [st0.ref], (th0, ph0, dp0))
    # the case's own evaluations (tests/test_gpu_parity.py's kinds: valid, random, back-facing, far off -> overflow), then
    # corners and planes whose w changes sign (test_radius_sweep.py) for the first states of the case
    for si, pos in zip(case["idx"][:72], case["parts"][:72]):
        st = refcost.state_of(case["pats"][si])
        add(st.ray, st.cams, pos, ref=st.ref, lod_=st.lod)
    from tests.test_radius_sweep import _corner_particles, _edge_on_particles
    for p in case["pats"][:6]:
        st = refcost.state_of(p)
        base = (p.normalS[0], p.normalS[1], p.depth)
        for pos in _corner_particles(scene, cfg, st, base) + _edge_on_particles(scene, cfg, st, base):
            add(st.ray, st.cams, pos, ref=st.ref, lod_=st.lod)
    ctx = _ctx(cfg, scene, monkeypatch)
    lit_ctx = _ctx(cfg, scene, monkeypatch, literal=True)
    d = ctx.fitness_detail(states, idx, parts, colours=True, homographies=True)
    _check_identity(d, lit_ctx.fitness_batch(states, idx, parts), "outcomes")
    assert list(d.outcome[:5]) == [BACKFACING, OFF_IMAGE, OFF_IMAGE, WINDOW, ALL_MASKED], list(d.outcome[:5])
    assert np.isnan(d.fitness[4]) and d.live_pixels[4] == 0 and (d.code[4] == MASKED).all()
    assert not d.homographies[0].any() and not d.pt[0].any()
    assert list(d.ref_pos[5:8]) == [st0.cams.index(st0.ref), -1, 1]
    seen = set()
    for e in range(len(states)):
        st = refcost.state_of(states[e])
        want = restate(scene, cfg, st, parts[e])
        if e >= 8 and refcost.cost(scene, cfg, st, parts[e], normal_fn=_det_normal).margin < MARGIN:
            continue
        _check_pixels(d, e, scene, cfg, st, parts[e], ("outcome", e))
        assert int(d.outcome[e]) == want["outcome"], (e, d.outcome[e], want["outcome"])
        K = len(st.cams)
        for i, c in enumerate(st.cams):                       # every listing of the reference camera: the identity
            if c == st.ref and d.outcome[e] != BACKFACING:
                assert d.homographies[e, i].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1], (e, i)
        assert not d.homographies[e, K:].any() and not d.colour[e, K:].any()
        seen.add(int(d.outcome[e]))
    assert seen == {OK, BACKFACING, OFF_IMAGE, WINDOW, OVERFLOW, ALL_MASKED}, seen
    ctx.close()
    lit_ctx.close()


@pytest.mark.gpu
def test_gpu_fitness_detail_is_independent_of_batch_and_chunks(request, monkeypatch):
    """One evaluation alone, in a shuffled batch of about 1 000 and in chunks of a few evaluations
    (PAIS_DETAIL_STAGING_MB=0.4): the same bytes."""
    case = _case(request, 15)
    scene, cfg, states = case["scene"], case["cfg"], case["states"]
    rng = np.random.default_rng(3)
    order = rng.permutation(np.resize(np.arange(len(case["idx"])), 1000))
    idx = [case["idx"][i] for i in order]
    parts = [case["parts"][i] for i in order]
    ctx = _ctx(cfg, scene, monkeypatch)
    ctx.detail_stats(reset=True)
    full = ctx.fitness_detail(states, idx, parts, colours=True, homographies=True)
    assert ctx.detail_stats()[1] == 1
    with P.knobs(monkeypatch, {"PAIS_DETAIL_STAGING_MB": "0.4"}):
        chunked = ctx.fitness_detail(states, idx, parts, colours=True, homographies=True)
    _, launches, n = ctx.detail_stats()
    assert launches >= 20 and n == 2000, (launches, n)
    fields = ("fitness", "sum_weight", "sum_weighted_sad", "pt", "outcome", "nx", "ny", "live_pixels", "overflow_pixel",
              "overflow_cam", "ref_pos", "weight", "avg_sad", "code", "colour", "homographies")
    for a in fields:
        assert getattr(full, a).tobytes() == getattr(chunked, a).tobytes(), a
    for j in rng.choice(len(idx), 12, replace=False):
        one = ctx.fitness_detail([states[idx[j]]], [0], [parts[j]], colours=True, homographies=True)
        K = int(states[idx[j]].num_cam)
        for a in fields:
            x, y = getattr(one, a)[0], getattr(full, a)[j]
            if a in ("colour", "homographies"):
                x, y = x[:K], y[:K]
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), (j, a)
    ctx.close()


def _call(ctx, states, idx, parts, stride, want=(True, True), null=None, fill=None):
    """pais_fitness_detail with an explicit cam_stride; outputs prefilled with `fill` -> (rc, arrays)."""
    from pais_mvs_amd import _lib
    n, S = len(idx), int(ctx.cfg.patchSize)
    arr = (_lib.PatchState * max(len(states), 1))(*states)
    ix = np.ascontiguousarray(idx, dtype=np.int32)
    pts = np.ascontiguousarray(parts, dtype=np.float64).reshape(-1, 3)
    out = dict(rec=(_lib.CostDetail * max(n, 1))(), weight=np.zeros((n, S, S)), avg_sad=np.zeros((n, S, S)),
               code=np.zeros((n, S, S), dtype=np.int8), colour=np.zeros((n, stride, S, S)) if want[0] else None,
               homographies=np.zeros((n, stride, 9)) if want[1] else None)
    if fill is not None:
        for k in ("colour", "homographies"):
            if out[k] is not None:
                out[k][:] = fill
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None
    args = dict(rec=out["rec"], weight=dp(out["weight"]), avg_sad=dp(out["avg_sad"]), code=out["code"].ctypes.data_as(C.POINTER(C.c_int8)),
                colour=dp(out["colour"]), homographies=dp(out["homographies"]))
    if null:
        args[null] = None
    rc = ctx.L.pais_fitness_detail(ctx.h, len(states), arr, n, ix.ctypes.data_as(C.POINTER(C.c_int32)), dp(pts), args["rec"],
                                   args["weight"], args["avg_sad"], args["code"], args["colour"], args["homographies"], stride)
    return rc, out


@pytest.mark.gpu
def test_gpu_fitness_detail_k64_r127(request, monkeypatch):
    """K = 64 (cameras listed several times, the reference camera among them) at r = 127: colours and H with cam_stride 64
    and 80; the padding rows keep their bytes, the values equal the K = 64 identity of the other tests."""
    case = _case(request, 127)
    scene, cfg = case["scene"], case["cfg"]
    p0 = next(p for p in case["pats"]
              if refcost.cost(scene, cfg, refcost.state_of(p), (p.normalS[0], p.normalS[1], p.depth)).outcome in ("ok", "overflow"))
    st0 = refcost.state_of(p0)
    cams = (st0.cams * 64)[:64]
    states = [_state(st0.ray, st0.ref, st0.lod, cams)]
    th, ph, dp = float(p0.normalS[0]), float(p0.normalS[1]), float(p0.depth)
    parts = [[th, ph, dp], [th + 0.05, ph - 0.05, dp], [th, ph, dp * 1.02], [math.pi - th, ph + math.pi, dp]]
    idx = [0] * len(parts)
    ctx = _ctx(cfg, scene, monkeypatch)
    lit_ctx = _ctx(cfg, scene, monkeypatch, literal=True)
    d = ctx.fitness_detail(states, idx, parts, colours=True, homographies=True)
    _check_identity(d, lit_ctx.fitness_batch(states, idx, parts), "K64")
    assert d.colour.shape[1] == 64 and int(d.outcome[0]) in (OK, OVERFLOW), d.outcome
    for stride in (64, 80):
        rc, out = _call(ctx, states, idx, parts, stride, fill=-7.5)
        assert rc == 0, ctx.L.pais_last_error()
        assert out["colour"][:, :64].tobytes() == d.colour.tobytes() and out["homographies"][:, :64].tobytes() == d.homographies.tobytes()
        assert (out["colour"][:, 64:] == -7.5).all() and (out["homographies"][:, 64:] == -7.5).all()
        assert out["weight"].tobytes() == d.weight.tobytes() and out["code"].tobytes() == d.code.tobytes()
    _check_pixels(d, 0, scene, cfg, refcost.state_of(states[0]), parts[0], "K64")
    ctx.close()
    lit_ctx.close()


@pytest.mark.gpu
def test_gpu_fitness_detail_rejects_bad_input(request, monkeypatch):
    """A bad state_index, num_cam outside [1, 64], cam_stride below a num_cam and NULL required outputs: rc < 0 with a named
    error, before any launch; a valid call on the same context afterwards succeeds."""
    case = _case(request, 15)
    scene, cfg = case["scene"], case["cfg"]
    states, idx, parts = case["states"][:3], case["idx"][:6], case["parts"][:6]
    idx = [i % 3 for i in idx]
    ctx = _ctx(cfg, scene, monkeypatch)
    err = lambda: ctx.L.pais_last_error().decode()
    rc, _ = _call(ctx, states, [0, 5] + idx[2:], parts, 64)
    assert rc < 0 and "state_index[1] = 5" in err(), err()
    rc, _ = _call(ctx, states, [0, -1] + idx[2:], parts, 64)
    assert rc < 0 and "state_index[1] = -1" in err(), err()
    for k in (0, 65):
        bad = [_state(s.ray, s.ref_cam, s.lod, [s.cam_idx[i] for i in range(s.num_cam)]) for s in states]
        bad[2].num_cam = k
        rc, _ = _call(ctx, bad, idx, parts, 64)
        assert rc < 0 and ("state 2: num_cam %d" % k) in err(), err()
    K = max(int(s.num_cam) for s in states)
    for want in ((True, False), (False, True)):
        rc, _ = _call(ctx, states, idx, parts, K - 1, want=want)
        assert rc < 0 and "cam_stride %d below num_cam %d" % (K - 1, K) in err(), err()
    rc, _ = _call(ctx, states, idx, parts, 0, want=(False, False))       # no per-camera output: cam_stride is not read
    assert rc == 0, err()
    for name in ("rec", "weight", "avg_sad", "code"):
        rc, _ = _call(ctx, states, idx, parts, K, null=name)
        label = {"rec": "out", "code": "pixel_code"}.get(name, name)
        assert rc < 0 and "null pointer (%s)" % label in err(), err()
    d = ctx.fitness_detail(states, idx, parts, colours=True, homographies=True)
    lit_ctx = _ctx(cfg, scene, monkeypatch, literal=True)
    _check_identity(d, lit_ctx.fitness_batch(states, idx, parts), "after rejections")
    ctx.close()
    lit_ctx.close()
