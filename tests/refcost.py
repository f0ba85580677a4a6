"""A plain float64 restatement of the cost and of the NCC table, independent of oracle/ and of the HIP library.

Written from the Python Camera mirror (pais_mvs_amd/camera.py: KR, KT, center, optical_normal, pyramid, edge_pyramid) and the
config, in the spirit of oracle/: the reference's per-pixel statements, evaluated one numpy operation at a time (numpy
never contracts a * b + c into a fused multiply-add), with the window sums formed by math.fsum, so that they are exactly
rounded.  Its purpose is to pin the oracle and the kernels against something outside both: a mistake they share (the
distance-table walk, the window origin, the S^2 normalisations) shows up here.

* gauss_table     -- the distance weighting of mvs.cpp:97-114 (pais_oracle.c:156-176), laid out x * S + y;
* homographies    -- Patch::getHomographies, patch.cpp:290-330, with the LOD matrix and the 3 x 3 inverse;
* cost            -- PAIS::getFitness, patch.cpp:914-1047;
* ncc_table       -- Patch::getHomographyPatch (patch.cpp:332-386) and Patch::setCorrelationTable (patch.cpp:221-267).

Next to each value comes a margin: the smallest distance of any quantity that decides a discrete outcome to its threshold
(the back-facing dot product against 0, the window pt +- r against [2, w-3), every counted tap against [2, cols-3) and
[2, rows-3), |w| against 0, and the window coordinates against the half-integers where cvRound picks the mask pixel).  Two
arithmetics of the same function may decide differently only where the margin is of the order of their rounding: a test
skips such an evaluation and counts the skip.

Rounding analysis of the gates (u = 2^-53):
* the literal paths (oracle literal, oracle costLiteral, PAIS_ARITH=literal) compute every per-pixel value with the same
  statements; their two window sums are sequential sums of S^2 non-negative terms, each within (S^2 - 1) u of the exactly
  rounded sum here, so the quotient is within 2 S^2 u; exp and the distance table may differ in the last bit (1e-15);
* NCC table entries are dot products of two unit vectors of S^2 entries: the normalisation of either vector and the dot
  product are each within S^2 u of the exact value, hence |delta| <= 4 S^2 u.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Callable, List, Sequence

import numpy as np

DBL_MAX = 1.7976931348623157e308
U = 2.0 ** -53


def literal_gate(S: int) -> float:
    """Relative gate between refcost.cost and a literal path (module docstring)."""
    return 2.0 * S * S * U + 1e-15


def table_gate(S: int) -> float:
    """Absolute gate between refcost.ncc_table and a table of the oracle or of the kernels."""
    return 4.0 * S * S * U


@dataclass
class State:
    """What the cost needs of a patch besides the particle: reference camera, level, visible cameras (camIdx order), ray."""
    ref: int
    lod: int
    cams: List[int]
    ray: Sequence[float] = (0.0, 0.0, 0.0)


def state_of(p) -> State:
    """State of an oracle po.Patch or a pais_patch_state / pais_view_state (ray absent: zeros)."""
    if hasattr(p, "refCamIdx"):
        return State(int(p.refCamIdx), int(p.LOD), [int(p.camIdx[i]) for i in range(p.numCam)], [float(v) for v in p.ray[:]])
    ray = [float(v) for v in p.ray[:]] if hasattr(p, "ray") else [0.0, 0.0, 0.0]
    return State(int(p.ref_cam), int(p.lod), [int(p.cam_idx[i]) for i in range(p.num_cam)], ray)


def cv_round(v):
    """cvRound: round half to even (lrint under the default rounding mode)."""
    return np.rint(v).astype(np.int64)


def _dot3(a, b) -> float:
    s = 0.0          # Matx::ddot: sequential from 0
    for i in range(3):
        s += float(a[i]) * float(b[i])
    return s


def _half_distance(v) -> float:
    """Distance of the values v to the nearest half-integer (where cvRound switches pixel)."""
    v = np.asarray(v, dtype=np.float64)
    return float(np.min(np.abs(v - np.floor(v) - 0.5))) if v.size else math.inf


# ---------------------------------------------------------------------------------------------------------------------
# distance weighting (mvs.cpp:97-114)
# ---------------------------------------------------------------------------------------------------------------------
_GAUSS = {}


def gauss_table(cfg) -> np.ndarray:
    """Gaussian of the distance to the window centre, sigma = distWeighting, normalised to sum 1; entry x * S + y."""
    r, S, sigma = int(cfg.patchRadius), int(cfg.patchSize), float(cfg.distWeighting)
    key = (r, sigma)
    if key not in _GAUSS:
        s2 = 1.0 / (2.0 * sigma * sigma)
        s = 1.0 / (2.0 * math.pi * sigma * sigma)
        g = np.empty(S * S, dtype=np.float64)
        for x in range(S):
            for y in range(S):
                g[x * S + y] = s * math.exp(-(float(x - r) ** 2 + float(y - r) ** 2) * s2)
        g = g * (1.0 / math.fsum(g))
        _GAUSS[key] = g
    return _GAUSS[key]


# ---------------------------------------------------------------------------------------------------------------------
# geometry: camera.cpp:138-160 (project), patch.cpp:290-330 (homographies)
# ---------------------------------------------------------------------------------------------------------------------
def level_shape(cam, lod: int):
    """(rows, cols) of a camera's level; (0, 0) for a level the camera does not have (lod > max_lod).  Such a camera passes no
    tap and no sample and is never inImage (Camera::inImage, camera.h:117 and :134): with cols = rows = 0 every bound test
    of the cost (2 <= ix < cols - 3) and of the NCC window (0 <= ix < cols - 1) fails, and no pixel is read."""
    return cam.pyramid[lod].shape if 0 <= lod <= cam.max_lod else (0, 0)


def project(cam, X, lod_scale: float):
    """Camera::project without distortion: R X + T, focal * (x / z) + pp, times the level scale."""
    R, T = np.asarray(cam.rotation, float), np.asarray(cam.translation, float)
    X2 = [0.0, 0.0, 0.0]
    for i in range(3):
        a = 0.0
        for k in range(3):
            a += float(R[i, k]) * float(X[k])
        X2[i] = a + float(T[i])
    u = float(cam.focal[0]) * (X2[0] / X2[2]) + float(cam.principle_point[0])
    v = float(cam.focal[1]) * (X2[1] / X2[2]) + float(cam.principle_point[1])
    return [u * lod_scale, v * lod_scale]


def _mat33(a, b):
    out = np.empty((3, 3))
    for i in range(3):
        for j in range(3):
            s = 0.0
            for k in range(3):
                s += float(a[i][k]) * float(b[k][j])
            out[i, j] = s
    return out


def _plane_matrix(d: float, sc: float, KR, KT, n):
    """d * LODM * KR - LODM * KT * n^T, LODM = diag(sc, sc, 1)."""
    L = (sc, sc, 1.0)
    M = np.empty((3, 3))
    for i in range(3):
        lkt = L[i] * float(KT[i])
        for j in range(3):
            M[i, j] = (L[i] * float(KR[i][j])) * d - lkt * float(n[j])
    return M


def _inv3(m):
    """3 x 3 inverse by the adjugate over the determinant (cv::invert DECOMP_LU of a 3 x 3); singular: zeros."""
    m = np.asarray(m, float)
    d = (m[0, 0] * (m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1]) - m[0, 1] * (m[1, 0] * m[2, 2] - m[1, 2] * m[2, 0]) +
         m[0, 2] * (m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0]))
    if d == 0:
        return np.zeros((3, 3))
    d = 1.0 / d
    return np.array([[(m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1]) * d, (m[0, 2] * m[2, 1] - m[0, 1] * m[2, 2]) * d,
                      (m[0, 1] * m[1, 2] - m[0, 2] * m[1, 1]) * d],
                     [(m[1, 2] * m[2, 0] - m[1, 0] * m[2, 2]) * d, (m[0, 0] * m[2, 2] - m[0, 2] * m[2, 0]) * d,
                      (m[0, 2] * m[1, 0] - m[0, 0] * m[1, 2]) * d],
                     [(m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0]) * d, (m[0, 1] * m[2, 0] - m[0, 0] * m[2, 1]) * d,
                      (m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]) * d]])


def homographies(cams, state: State, center, normal, lod_ratio: float) -> List[np.ndarray]:
    """One 3 x 3 homography per camera of state.cams, reference window -> that camera's level; identity for the reference."""
    sc = lod_ratio ** state.lod          # pow(mvs.lodRatio, LOD)
    d = -_dot3(center, normal)
    rc = cams[state.ref]
    inv = _inv3(_plane_matrix(d, sc, rc.KR, rc.KT, normal))
    out = []
    for c in state.cams:
        if c == state.ref:
            out.append(np.eye(3))
        else:
            out.append(_mat33(_plane_matrix(d, sc, cams[c].KR, cams[c].KT, normal), inv))
    return out


def _walk(start: float, stop: float) -> np.ndarray:
    """for (double v = start; v <= stop; ++v): the values the reference's loop variable takes (repeated ++)."""
    vals = []
    v = start
    while v <= stop:
        vals.append(v)
        v += 1.0
    return np.array(vals, dtype=np.float64)


def _warp(H, X, Y):
    """w, ix, iy of patch.cpp:994-996 / 355-357 (no contraction, true division)."""
    w = H[2, 0] * X + H[2, 1] * Y + H[2, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        ix = (H[0, 0] * X + H[0, 1] * Y + H[0, 2]) / w
        iy = (H[1, 0] * X + H[1, 1] * Y + H[1, 2]) / w
    return w, ix, iy


def _bilinear(img, ix, iy):
    """The four-product bilinear of patch.cpp:1014-1017 / 372-375 at in-bounds (ix, iy)."""
    px0 = ix.astype(np.int64)
    py0 = iy.astype(np.int64)
    px1, py2 = px0 + 1, py0 + 1
    a, b = px1 - ix, ix - px0
    c, e = py2 - iy, iy - py0
    i0 = img[py0, px0].astype(np.float64)
    i1 = img[py0, px1].astype(np.float64)
    i2 = img[py2, px0].astype(np.float64)
    i3 = img[py2, px1].astype(np.float64)
    return i0 * a * c + i1 * b * c + i2 * a * e + i3 * b * e


def spherical_to_normal(th: float, ph: float, sin=math.sin, cos=math.cos):
    """Utility::spherical2normal (utility.h:25-29)."""
    return [sin(th) * cos(ph), sin(th) * sin(ph), cos(th)]


# ---------------------------------------------------------------------------------------------------------------------
# cost: PAIS::getFitness (patch.cpp:914-1047)
# ---------------------------------------------------------------------------------------------------------------------
@dataclass
class Cost:
    value: float            # DBL_MAX, a finite value, or NaN (sum_weight == 0: every window pixel masked, or every weight 0)
    outcome: str            # "backfacing", "outside" (window / projection), "overflow" (a counted tap), "ok"
    margin: float           # distance of the deciding quantities to their thresholds (module docstring)
    backface_dot: float     # n . optical_normal(ref)
    min_abs_w: float        # smallest |w| over the counted taps (inf when none was reached)
    live_pixels: int = 0    # counted pixels of an "ok" evaluation (0: every window pixel masked)
    sum_weight: float = 0.0           # the exactly rounded sum of the pixel weights (the divisor of :1046)
    min_weight: float = math.inf      # smallest positive pixel weight (inf when no weight is positive)
    max_arg: float = -math.inf        # largest sum of a counted pixel's exp arguments (the distance factor as its logarithm):
                                      # above -745 that pixel's weight is positive in exact arithmetic


def cost(scene, cfg, state: State, particle, normal_fn: Callable = None) -> Cost:
    """The cost of particle (theta, phi, depth) of the patch state.  normal_fn(theta, phi) -> normal: the elementary
    functions of the path compared with (default: the platform's sin / cos, what the reference calls)."""
    cams = scene.cameras if hasattr(scene, "cameras") else scene
    th, ph, depth = (float(v) for v in particle)
    n = normal_fn(th, ph) if normal_fn else spherical_to_normal(th, ph)
    rc = cams[state.ref]
    bf = _dot3(n, rc.optical_normal)
    if bf > 0:                                                                       # :939
        return Cost(DBL_MAX, "backfacing", abs(bf), bf, math.inf)
    margin = abs(bf)
    center = [float(state.ray[i]) * depth + float(rc.center[i]) for i in range(3)]  # :944
    H = homographies(cams, state, center, n, cfg.lodRatio)                            # :948
    lod, r = state.lod, int(cfg.patchRadius)
    sc = cfg.lodRatio ** lod
    if lod > rc.max_lod:
        return Cost(DBL_MAX, "outside", math.inf, bf, math.inf)
    ref_img = rc.pyramid[lod]
    rows, cols = ref_img.shape
    pt = project(rc, center, sc)
    if not (pt[0] == pt[0] and pt[1] == pt[1] and 0 <= pt[0] < cols and 0 <= pt[1] < rows):   # :952
        return Cost(DBL_MAX, "outside", margin, bf, math.inf)
    lo = (pt[0] - r, pt[1] - r)
    hi = (pt[0] + r, pt[1] + r)
    margin = min(margin, abs(lo[0] - 2), abs(hi[0] - (cols - 3)), abs(lo[1] - 2), abs(hi[1] - (rows - 3)))
    if lo[0] < 2 or hi[0] >= cols - 3 or lo[1] < 2 or hi[1] >= rows - 3:            # :957-962
        return Cost(DBL_MAX, "outside", margin, bf, math.inf)
    xs, ys = _walk(lo[0], hi[0]), _walk(lo[1], hi[1])                                # :979-980
    margin = min(margin, _half_distance(xs), _half_distance(ys))
    X = np.repeat(xs, len(ys))                       # pixel k of the walk: x outer, y inner
    Y = np.tile(ys, len(xs))
    rx, ry = cv_round(X), cv_round(Y)
    live = ref_img[ry, rx] != 0                      # :986 (a masked pixel is skipped before any tap)
    g = gauss_table(cfg)[:len(X)]                    # :1031 (the table iterator advances once per pixel of the walk)
    X, Y, rx, ry, g = X[live], Y[live], rx[live], ry[live], g[live]
    K = len(state.cams)
    colours = []
    over = False
    min_w = math.inf
    for i, c in enumerate(state.cams):
        crow, ccol = level_shape(cams[c], lod)         # (an absent level: no tap passes)
        img = cams[c].pyramid[lod] if ccol else None
        w, ix, iy = _warp(H[i], X, Y)
        bad = (ix < 2) | (ix >= ccol - 3) | (iy < 2) | (iy >= crow - 3) | (w == 0) | np.isnan(ix) | np.isnan(iy)   # :999
        if len(w):
            min_w = min(min_w, float(np.min(np.abs(w))))
            with np.errstate(invalid="ignore"):
                dist = np.minimum(np.minimum(np.abs(ix - 2), np.abs(ix - (ccol - 3))), np.minimum(np.abs(iy - 2), np.abs(iy - (crow - 3))))
            margin = min(margin, float(np.nanmin(np.where(np.isnan(dist), 0.0, dist))), float(np.min(np.abs(w))))
        if bad.any():
            over = True
            continue
        colours.append(_bilinear(img, ix, iy))
    if over:                                                                          # :1001 (the whole call)
        return Cost(DBL_MAX, "overflow", margin, bf, min_w)
    mean = np.zeros(len(X))
    for c in colours:
        mean = mean + c
    mean = mean / K                                                                   # :1022
    sad = np.zeros(len(X))
    for c in colours:
        sad = sad + np.abs(c - mean)
    sad = sad / K                                                                     # :1027
    weight = np.ones(len(X))
    arg = np.zeros(len(X))                           # (not part of the cost: the exponent of the exact weight, for max_arg)
    if cfg.adaptiveDistanceEnable:
        weight = weight * g                                                           # :1031
        with np.errstate(divide="ignore"):
            arg = arg + np.log(g)
    if cfg.adaptiveDifferenceEnable:
        a = -sad * sad / cfg.diffWeighting
        weight = weight * np.array(list(map(math.exp, a.tolist())))                   # :1034
        arg = arg + a
    if cfg.adaptiveGradientEnable:
        edge = rc.edge_pyramid[lod][ry, rx]
        with np.errstate(divide="ignore"):                                            # (edge 0: exp(-inf) = 0)
            a = -1.0 / (edge * cfg.gradientWeighting)
        weight = weight * np.array(list(map(math.exp, a.tolist())))                   # :1037
        arg = arg + a
    sw = math.fsum(weight.tolist())                                                   # :1040
    fit = math.fsum((weight * sad).tolist())                                          # :1041
    value = fit / sw if sw != 0 else math.nan                                         # :1046
    pos = weight[weight > 0]
    return Cost(value, "ok", margin, bf, min_w, live_pixels=len(X), sum_weight=sw,
                min_weight=float(pos.min()) if len(pos) else math.inf, max_arg=float(arg.max()) if len(arg) else -math.inf)


# ---------------------------------------------------------------------------------------------------------------------
# NCC table: Patch::getHomographyPatch (patch.cpp:332-386), Patch::setCorrelationTable (patch.cpp:221-267)
# ---------------------------------------------------------------------------------------------------------------------
@dataclass
class NccTable:
    dropped: bool           # a warped sample left [0, cols-1) x [0, rows-1): the patch is dropped (no table)
    table: np.ndarray       # K x K, zero diagonal (zeros when dropped)
    margin: float           # distance of every sample's ix / iy to 0 and dim-1, and of w to 0


def homography_patch(img, pt, H, r: int):
    """(values of the warped window in the reference's walk order normalised to unit length, in bounds, margin); img None:
    the camera has no such level (level_shape) -- no sample is in bounds."""
    rows, cols = img.shape if img is not None else (0, 0)
    xs, ys = _walk(pt[0] - r, pt[0] + r), _walk(pt[1] - r, pt[1] + r)
    X, Y = np.repeat(xs, len(ys)), np.tile(ys, len(xs))
    w, ix, iy = _warp(H, X, Y)
    bad = (ix < 0) | (ix >= cols - 1) | (iy < 0) | (iy >= rows - 1) | (w == 0) | np.isnan(ix) | np.isnan(iy)
    with np.errstate(invalid="ignore"):
        dist = np.minimum(np.minimum(np.abs(ix), np.abs(ix - (cols - 1))), np.minimum(np.abs(iy), np.abs(iy - (rows - 1))))
    margin = min(float(np.min(np.where(np.isnan(dist), 0.0, dist))), float(np.min(np.abs(w))))
    if bad.any():
        return None, False, margin
    hp = _bilinear(img, ix, iy)
    return hp / math.sqrt(math.fsum((hp * hp).tolist())), True, margin     # hp /= sqrt(sum)


def ncc_table(scene, cfg, view) -> NccTable:
    """The correlation table of view = (center, normal, ref, lod, cams) -- a dict in the form of
    tests/golden/make_ncc_golden.py's states, or anything with those attributes."""
    get = (lambda k: view[k]) if isinstance(view, dict) else (lambda k: getattr(view, k))
    cams = scene.cameras if hasattr(scene, "cameras") else scene
    center, normal = [float(v) for v in get("center")], [float(v) for v in get("normal")]
    st = State(int(get("ref")), int(get("lod")), [int(c) for c in get("cams")])
    H = homographies(cams, st, center, normal, cfg.lodRatio)
    pt = project(cams[st.ref], center, cfg.lodRatio ** st.lod)
    K = len(st.cams)
    hps, margin, dropped = [], math.inf, False
    for i, c in enumerate(st.cams):
        img = cams[c].pyramid[st.lod] if level_shape(cams[c], st.lod)[1] else None
        hp, ok, m = homography_patch(img, pt, H[i], int(cfg.patchRadius))
        margin = min(margin, m)
        dropped = dropped or not ok
        hps.append(hp)
    T = np.zeros((K, K))
    if dropped:
        return NccTable(True, T, margin)
    for i in range(K):
        for j in range(i + 1, K):
            T[i, j] = T[j, i] = math.fsum((hps[i] * hps[j]).tolist())
    return NccTable(False, T, margin)


# ---------------------------------------------------------------------------------------------------------------------
# the checkers the sweeps share
# ---------------------------------------------------------------------------------------------------------------------
MARGIN = 1e-7       # below this margin two arithmetics may decide differently: the evaluation is skipped and counted


def _rel(a, b):
    if b == 0:                  # (a patch of the reference camera alone: every finite cost is exactly 0)
        return 0.0 if a == 0 else math.inf
    return abs(a - b) / abs(b)


def denormal_sum(c: Cost) -> bool:
    """The sum of weights of c is made of denormals: two correct orders of the three-factor product (the kernels multiply
    (gauss * grad) * diff, the reference (gauss * diff) * grad) may then differ by more than any relative gate, or one of them
    may lose the last positive weight.  True when the sum is non-zero and below 2^-900, or zero while some counted pixel's weight
    is positive in exact arithmetic (the sum of its exp arguments above -745)."""
    if c.outcome != "ok" or c.live_pixels == 0:
        return False
    if c.sum_weight != 0:
        return c.sum_weight < 2.0 ** -900
    return c.max_arg > -745.0


def check_against_refcost(r, refs, vals, gate, what, skip=None, stats=None):
    """vals against refcost results: discrete outcome identical and finite values within gate (relative) wherever the
    margin is at least MARGIN -> (finite, DBL_MAX, skipped) counts.  skip: a predicate on the refcost result that skips (and
    counts) an evaluation besides the margin, e.g. denormal_sum; stats: a dict that receives the NaN count, the skips of
    either kind and the worst relative error."""
    n_fin = n_max = skipped = n_nan = n_pred = 0
    worst = 0.0
    for e, (c, v) in enumerate(zip(refs, vals)):
        if c.margin < MARGIN:
            skipped += 1
            continue
        if skip is not None and skip(c):
            skipped += 1
            n_pred += 1
            continue
        if c.value == DBL_MAX:
            n_max += 1
            assert v == DBL_MAX, (what, r, e, c.outcome, v)
            continue
        assert v != DBL_MAX, (what, r, e, c.value, c.margin)
        if math.isnan(c.value):
            n_nan += 1
            assert math.isnan(v), (what, r, e, v)
            continue
        n_fin += 1
        assert _rel(v, c.value) <= gate, (what, r, e, v, c.value, _rel(v, c.value), gate)
        worst = max(worst, _rel(v, c.value))
    if stats is not None:
        stats.update(nan=n_nan, skipped_margin=skipped - n_pred, skipped_denormal=n_pred, worst=worst)
    return n_fin, n_max, skipped


def check_counts(ev, counts, what):
    n_fin, n_max, skipped = counts
    assert n_fin >= 30 and n_max >= 5, (what, n_fin, n_max)
    assert skipped <= max(2, len(ev["parts"]) // 50), (what, skipped, len(ev["parts"]))
