"""Generates tests/golden/oracle_ncc_vectors.json (fixture G4: NCC table, region ratios and camera removal of given
patch states).  Run in the build container only:

    python tests/golden/make_ncc_golden.py

The values come from the oracle in kernel arithmetic (po_homographies, po_region_ratio, po_set_correlation_table,
po_remove_invisible_camera: Patch::removeInvisibleCamera, patch.cpp:655-721) on states of the small synthetic pawn,
low-texture pawn, ring and dome scenes (the session fixtures of tests/conftest.py):

* states of oracle refine records (centre, normal, reference camera, LOD), with the record's cameras and with the seed's
  whole visible set;
* the same states with perturbed normals and centres, and with two- / three-camera subsets;
* hand-built states: a centre moved until a warped sample lies just past dim-1 (and the last one before it), and states
  searched for the reasons a camera is removed.

tests/test_ncc_batch.py checks that the oracle still reproduces the file (CPU) and that pais_ncc_batch does (GPU).
The helpers below are shared with that test.
"""
import base64
import ctypes as C
import hashlib
import json
import math
import os
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np
from oracle import po

KEEP, REGION, BACKFACING, CORRELATION = 0, 1, 2, 3
DROP_SAMPLE, DROP_MINCAM = 1, 2
OUT = os.path.join(HERE, "oracle_ncc_vectors.json")


def hexd(x):
    return struct.pack(">d", float(x)).hex()


def unhex(h):
    return struct.unpack(">d", bytes.fromhex(h))[0]


def b64d(vals):
    return base64.b64encode(np.asarray(vals, dtype="<f8").tobytes()).decode()


def unb64d(s):
    return np.frombuffer(base64.b64decode(s), dtype="<f8").astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------------
# scenes and configurations (the session fixtures of tests/conftest.py)
# ---------------------------------------------------------------------------------------------------------------------
def scene_config(name):
    from pais_mvs_amd.config import readme_config
    if name == "dome_small":
        return readme_config(patchRadius=25, distWeighting=25 / 3.0, reduceNormalRange=4.0, adaptiveGradientEnable=True,
                             particleNum=6, maxIteration=8, visibleCorrelation=0.6)
    return readme_config()


def make_scene(name):
    from pais_mvs_amd import synth
    if name == "pawn_small":
        return synth.pawn_scene(width=320, height=240, n_seeds=24)
    if name == "pawn_lowtex":
        return synth.pawn_scene(width=320, height=240, n_seeds=24, tex_std=5.0, tex_lam=(40.0, 260.0))
    if name == "ring_small":
        return synth.ring_scene(n_cams=24, width=480, height=360, focal=450.0, radius=3.0, n_seeds=30)
    if name == "dome_small":
        return synth.dome_scene(n_cams=40, width=400, height=300, focal=420.0, radius=4.0, n_seeds=24)
    raise ValueError(name)


def image_sha1(scene):
    h = hashlib.sha1()
    for c in scene.cameras:
        h.update(np.ascontiguousarray(c.image).tobytes())
    return h.hexdigest()


# ---------------------------------------------------------------------------------------------------------------------
# the oracle's removeInvisibleCamera with its intermediates
# ---------------------------------------------------------------------------------------------------------------------
def _patch(st):
    p = po.Patch()
    p.id = -1
    p.center[:] = [float(v) for v in st["center"]]
    p.normal[:] = [float(v) for v in st["normal"]]
    p.refCamIdx = int(st["ref"])
    p.LOD = int(st["lod"])
    p.numCam = len(st["cams"])
    for i, c in enumerate(st["cams"]):
        p.camIdx[i] = int(c)
    return p


def oracle_ncc(S, st):
    """Patch::removeInvisibleCamera of state st = {center, normal, ref, lod, cams} in the oracle's current arithmetic ->
    {correlation, ratios, table (K*K, row-major), max_idx, reasons, kept, dropped}.  The reasons are those of the test
    order of patch.cpp:686-706; the kept list is checked against po_remove_invisible_camera's own."""
    L = po.lib()
    K = len(st["cams"])
    p = _patch(st)
    H = (C.c_double * (9 * K))()
    L.po_homographies(S.ptr, C.byref(p), p.center, p.normal, H)
    pt = (C.c_double * 2)()
    L.po_project(S.ptr, p.refCamIdx, p.center, pt, p.LOD)
    ratios = [float(L.po_region_ratio(S.ptr, pt, (C.c_double * 9)(*H[9 * i:9 * i + 9]))) for i in range(K)]
    q = _patch(st)
    L.po_set_correlation_table(S.ptr, C.byref(q), H)
    r = _patch(st)
    L.po_remove_invisible_camera(S.ptr, C.byref(r))
    if q.drop:
        assert r.drop
        return {"correlation": 0.0, "ratios": ratios, "table": [0.0] * (K * K), "max_idx": 0, "reasons": [0] * K,
                "kept": [], "dropped": DROP_SAMPLE}
    table = [float(q.corrTable[i]) for i in range(K * K)]
    max_corr, max_idx = -sys.float_info.max, 0
    for i in range(K):
        s = 0.0
        for j in range(K):
            s += table[i * K + j]
        if s >= max_corr:
            max_idx, max_corr = i, s
    cfg = S.ptr.contents.cfg
    reasons, kept = [], []
    for i, c in enumerate(st["cams"]):
        o = S._cams[c].optN
        n = p.normal
        dd = n[0] * (-o[0]) + n[1] * (-o[1]) + n[2] * (-o[2])
        if ratios[i] < cfg.minRegionRatio:
            why = REGION
        elif dd < 0:
            why = BACKFACING
        elif i != max_idx and table[max_idx * K + i] < cfg.minCorrelation:
            why = CORRELATION
        else:
            why = KEEP
            kept.append(int(c))
        reasons.append(why)
    assert kept == r.cams(), (kept, r.cams())
    dropped = DROP_MINCAM if len(kept) < cfg.minCamNum else 0
    assert bool(dropped) == bool(r.drop)
    return {"correlation": float(q.correlation), "ratios": ratios, "table": table, "max_idx": max_idx, "reasons": reasons,
            "kept": kept, "dropped": dropped}


# ---------------------------------------------------------------------------------------------------------------------
# states
# ---------------------------------------------------------------------------------------------------------------------
def _rotate(n, axis, ang):
    n = np.asarray(n, float)
    k = np.asarray(axis, float)
    k = k / np.linalg.norm(k)
    v = n * math.cos(ang) + np.cross(k, n) * math.sin(ang) + k * (k @ n) * (1 - math.cos(ang))
    return v / np.linalg.norm(v)


def _state(center, normal, ref, lod, cams, kind):
    return {"center": [float(v) for v in center], "normal": [float(v) for v in normal], "ref": int(ref), "lod": int(lod),
            "cams": [int(c) for c in cams], "kind": kind}


def oracle_records(S, scene):
    """refine() of every seed by the oracle (kernel arithmetic): (centre, normal, ref, lod, record cams, seed cams) of the
    records that survive."""
    L = po.lib()
    out = []
    for i, (X, vis) in enumerate(scene.seeds):
        p = S.seed_patch(X, vis, key=i)
        L.po_refine_seed(S.ptr, C.byref(p))
        if not p.drop:
            out.append((list(p.center[:]), list(p.normal[:]), p.refCamIdx, p.LOD, p.cams(), [int(v) for v in vis]))
    return out


def _valid(scene, st):
    """What pais_ncc_batch accepts."""
    cams = st["cams"]
    if not 2 <= len(cams) <= 64 or len(set(cams)) != len(cams):
        return False
    ml = min(scene.cameras[c].max_lod for c in cams + [st["ref"]])
    return 0 <= st["lod"] <= ml


def edge_states(S, scene, rec):
    """A centre moved along the reference camera's image x axis until a warped sample leaves [0, dim-1): the last state
    that stays inside and the first one that leaves (bisection to the last bit of the shift)."""
    center, normal, ref, lod, cams, _ = rec
    cam = scene.cameras[ref]
    R = np.asarray(cam.rotation, float)
    depth = float(np.linalg.norm(np.asarray(center) - np.asarray(cam.center)))
    step = R[0] * depth / float(cam.focal[0])          # about one pixel at level 0

    def at(t):
        return _state(np.asarray(center) + t * step, normal, ref, lod, cams, "edge")

    def drops(t):
        return oracle_ncc(S, at(t))["dropped"] == DROP_SAMPLE

    if drops(0.0):
        return []
    hi = 1.0
    while not drops(hi):
        hi *= 2.0
        if hi > 1e5:
            return []
    lo = 0.0
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        if mid == lo or mid == hi:
            break
        if drops(mid):
            hi = mid
        else:
            lo = mid
    a, b = at(lo), at(hi)
    a["kind"], b["kind"] = "edge_inside", "edge_past"
    return [a, b]


def scene_states(S, scene, records, rng, n_perturb=1, n_search=24):
    """The state set of one scene from its refine records (deterministic for a given rng)."""
    states = []
    for rec in records:
        center, normal, ref, lod, cams, vis = rec
        if len(cams) >= 2:
            states.append(_state(center, normal, ref, lod, cams, "record"))
        if vis != cams:
            states.append(_state(center, normal, ref, lod, vis, "record_seed_cams"))
        for _ in range(n_perturb):
            ang = float(rng.uniform(0.05, 0.9))
            n2 = _rotate(normal, rng.normal(size=3), ang)
            c2 = np.asarray(center) + rng.normal(size=3) * 0.002 * float(np.linalg.norm(center) + 1.0)
            states.append(_state(c2, n2, ref, lod, vis, "perturbed"))
        k = int(rng.integers(2, 4))
        if len(vis) > k:
            sub = sorted(rng.choice(len(vis), size=k, replace=False).tolist())
            states.append(_state(center, normal, ref, lod, [vis[i] for i in sub], "subset"))
    # searched: strong tilts until every reason has occurred (backfacing needs a camera beyond 90 degrees of the normal
    # whose window stays in the image and is not foreshortened below minRegionRatio)
    seen = set()
    for st in states:
        o = oracle_ncc(S, st)
        seen.update(o["reasons"])
    tries = 0
    while tries < n_search * len(records) and not {REGION, BACKFACING, CORRELATION} <= seen:
        rec = records[tries % len(records)]
        tries += 1
        center, normal, ref, lod, cams, vis = rec
        n2 = _rotate(normal, rng.normal(size=3), float(rng.uniform(0.6, 1.6)))
        st = _state(center, n2, ref, lod, vis, "searched")
        o = oracle_ncc(S, st)
        if o["dropped"] != DROP_SAMPLE and not set(o["reasons"]) <= seen:
            seen.update(o["reasons"])
            states.append(st)
    for rec in records[:2]:
        states.extend(edge_states(S, scene, rec))
    return [st for st in states if _valid(scene, st)]


def encode_case(st, o):
    K = len(st["cams"])
    tri = [o["table"][i * K + j] for i in range(K) for j in range(i + 1, K)]
    return {"kind": st["kind"], "center": [hexd(v) for v in st["center"]], "normal": [hexd(v) for v in st["normal"]],
            "ref": st["ref"], "lod": st["lod"], "cams": st["cams"], "correlation": hexd(o["correlation"]),
            "ratios": b64d(o["ratios"]), "table_upper": b64d(tri), "max_idx": o["max_idx"], "reasons": o["reasons"],
            "kept": o["kept"], "dropped": o["dropped"]}


def decode_case(c):
    """-> (state, expected) in the form of _state / oracle_ncc."""
    st = {"center": [unhex(h) for h in c["center"]], "normal": [unhex(h) for h in c["normal"]], "ref": c["ref"],
          "lod": c["lod"], "cams": list(c["cams"]), "kind": c["kind"]}
    K = len(st["cams"])
    tri = unb64d(c["table_upper"])
    table = [0.0] * (K * K)
    t = 0
    for i in range(K):
        for j in range(i + 1, K):
            table[i * K + j] = table[j * K + i] = float(tri[t])
            t += 1
    exp = {"correlation": unhex(c["correlation"]), "ratios": [float(v) for v in unb64d(c["ratios"])], "table": table,
           "max_idx": c["max_idx"], "reasons": list(c["reasons"]), "kept": list(c["kept"]), "dropped": c["dropped"]}
    return st, exp


SCENES = ("pawn_small", "pawn_lowtex", "ring_small", "dome_small")


def main():
    from tests import common
    out = {"about": "fixture G4: pais_ncc_batch / Patch::removeInvisibleCamera by the oracle in kernel arithmetic "
                    "(tests/golden/make_ncc_golden.py)", "scenes": {}}
    for name in SCENES:
        scene = make_scene(name)
        cfg = scene_config(name)
        S = common.oracle_scene(cfg, scene)
        S.set_kernel_arithmetic(True)
        S.set_omp(True)
        records = oracle_records(S, scene)
        rng = np.random.default_rng(2024 + SCENES.index(name))
        limit = 12 if name == "dome_small" else len(records)
        states = scene_states(S, scene, records[:limit], rng)
        cases = [encode_case(st, oracle_ncc(S, st)) for st in states]
        out["scenes"][name] = {"image_sha1": image_sha1(scene), "cases": cases}
        S.close()
        rs = [r for c in cases for r in c["reasons"]]
        print("%-12s %3d states  K %d..%d  reasons %s  drops %s" % (
            name, len(cases), min(len(c["cams"]) for c in cases), max(len(c["cams"]) for c in cases),
            [rs.count(k) for k in range(4)], [sum(c["dropped"] == d for c in cases) for d in (0, 1, 2)]))
    with open(OUT, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
