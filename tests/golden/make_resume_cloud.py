"""Writes tests/golden/resume_cloud.json: the hand-picked part of the cloud of tests/test_resume.py -- patch records of an .mvs
file that drive the loader constructor Patch(center, normalS, camIdx, fitness, correlation) (patch.cpp:45-59) through the branches
a reconstructed cloud never reaches.  Picked here with the ORACLE alone (no GPU):

    python tests/golden/make_resume_cloud.py          (~20 s)

Per scene (the 320x240 pawn of the parity tests and its low-texture variant; README configuration) the file holds records of
these kinds, each checked below to take the branch it is named after:

    few_cams     fewer than minCamNum cameras: setReferenceCameraIndex drops (patch.cpp:419-422)
    no_cams      num_cam == 0: the same branch, and setImagePoint's empty list
    same_cam     minCamNum entries that all name the reference camera: setDepthRange skips every camera,
                 maxWorldDist stays -DBL_MAX (:486, :502-505)
    far          a centre 1e7 scene units down the reference camera's ray: every imgDist < 0.01 (:497), the same drop
    border_0     the window leaves the reference image at level 0: setLOD's fallback max(LOD - 1, 0) at LOD 0 (:548-552)
    border_up    a centre on the background (gray value 0: variance 0 at every level) near the image border: the loop climbs until
                 the window leaves the image at a level >= 2 and falls back to LOD - 1 >= 1
    seed         (low-texture scene) the scene's seeds as the oracle refines them: setLOD settles on levels 0, 1 and 2

`classify` replays the constructor's setters one by one through the oracle and names the setter that dropped the patch; the test
uses it to assert that the cloud it loads still contains every kind."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "tests", "golden", "resume_cloud.json")
DBL_MAX = 1.7976931348623157e308
SETTERS = ("po_set_reference_camera", "po_set_depth_and_ray", "po_set_depth_range", "po_set_lod", "po_set_priority",
           "po_set_image_point")


def scenes():
    from pais_mvs_amd import synth
    return {"pawn_small": synth.pawn_scene(width=320, height=240, n_seeds=24),
            "pawn_lowtex": synth.pawn_scene(width=320, height=240, n_seeds=24, tex_std=5.0, tex_lam=(40.0, 260.0))}


def oracle_load(S, mo, rec):
    """po_mvs_load_patch of one record {center, normalS, cams, fitness, correlation} -> the stored oracle patch"""
    from oracle import po
    L = po.lib()
    i = L.po_mvs_load_patch(mo, po.darr(rec["center"]), po.darr(rec["normalS"]), len(rec["cams"]), po.iarr(rec["cams"]),
                            rec["fitness"], rec["correlation"])
    return L.po_mvs_get_patch(mo, i).contents


def classify(S, loaded, rec):
    """The constructor's setter chain on a fresh patch with `loaded`'s normal (the oracle's setNormal(Vec2d)), one setter at a
    time -> (name of the setter that set `drop`, or None; the patch after the chain, drop as the reference leaves it)."""
    from oracle import po
    L = po.lib()
    p = po.Patch()
    p.id = -1; p.refCamIdx = -1; p.LOD = -1
    p.priority = DBL_MAX
    p.type = 0
    p.center[:] = rec["center"]
    p.normalS[:] = rec["normalS"]
    p.normal[:] = loaded.normal[:]
    p.numCam = len(rec["cams"])
    for i, c in enumerate(rec["cams"]):
        p.camIdx[i] = c
    p.fitness, p.correlation = rec["fitness"], rec["correlation"]
    dropped_by = None
    for name in SETTERS:
        getattr(L, name)(S.ptr, C.byref(p))
        if p.drop and dropped_by is None:
            dropped_by = name
    return dropped_by, p


def window_state(S, scene, p, lod):
    """(the centre projects into the reference image at `lod`, the S x S window around it lies inside, its gray values)"""
    from oracle import po
    L = po.lib()
    pt = (C.c_double * 2)()
    ok = bool(L.po_project(S.ptr, p.refCamIdx, p.center, pt, lod))
    img = scene.cameras[p.refCamIdx].pyramid[lod]
    r = int(S.cfg.patchRadius)
    cx, cy = int(np.rint(pt[0])), int(np.rint(pt[1]))            # cvRound: half to even
    inside = ok and cx - r >= 0 and cy - r >= 0 and cx + r < img.shape[1] and cy + r < img.shape[0]
    return ok, inside, (img[cy - r:cy + r + 1, cx - r:cx + r + 1] if inside else None)


def lod_fell_back(S, scene, p):
    """setLOD of patch p ended in one of its `LOD - 1` fallbacks (patch.cpp:530-533, 548-552): it did not stop at the top level, and
    at the level it settled on either the window is not inside the image (the fallback of level 0), or the window is inside with
    variance exactly 0 < textureVariation -- so the loop went on to the next level and came back."""
    if p.drop or p.LOD < 0 or p.LOD >= scene.cameras[p.refCamIdx].max_lod:
        return False
    ok, inside, win = window_state(S, scene, p, p.LOD)
    if not inside:
        return p.LOD == 0
    return int(win.max()) == int(win.min())


def back_project(cam, u, v, z):
    """the point at camera-space depth z that projects to pixel (u, v) of `cam` at level 0"""
    q = np.array([(u - cam.principle_point[0]) / cam.focal[0] * z, (v - cam.principle_point[1]) / cam.focal[1] * z, z])
    return (cam.rotation.T @ (q - cam.translation)).tolist()


def pick(name, scene):
    from oracle import po
    from pais_mvs_amd.config import readme_config
    from tests import common
    cfg = readme_config()
    S = common.oracle_scene(cfg, scene)
    S.set_kernel_arithmetic(True)
    L = po.lib()
    seeds = []
    for i, (X, vis) in enumerate(scene.seeds):
        p = S.seed_patch(X, vis, key=i)
        L.po_refine_seed(S.ptr, C.byref(p))
        if not p.drop:
            seeds.append(p)
    assert len(seeds) >= 12, len(seeds)
    rec = lambda kind, p, center=None, cams=None: {
        "kind": kind, "center": list(center if center is not None else p.center[:]), "normalS": list(p.normalS[:]),
        "cams": list(cams if cams is not None else p.cams()), "fitness": p.fitness, "correlation": p.correlation}
    out = []
    for p in seeds[:3]:
        cam = scene.cameras[p.refCamIdx]
        z = float(cam.rotation[2] @ np.asarray(p.center[:]) + cam.translation[2])
        ray = np.asarray(p.center[:]) - cam.center
        out.append(rec("few_cams", p, cams=p.cams()[:cfg.minCamNum - 1]))
        out.append(rec("no_cams", p, cams=[]))
        out.append(rec("same_cam", p, cams=[p.refCamIdx] * cfg.minCamNum))
        out.append(rec("far", p, center=(cam.center + ray / np.linalg.norm(ray) * 1e7).tolist()))
        out.append(rec("border_0", p, center=back_project(cam, 6.0, cam.height / 2.0, z)))
        for u, v in ((36.0, 30.0), (cam.width - 40.0, cam.height - 34.0), (30.0, cam.height - 30.0)):
            out.append(rec("border_up", p, center=back_project(cam, u, v, z)))
    if name == "pawn_lowtex":
        out += [rec("seed", p) for p in seeds]
    # every record takes the branch it is named after
    mo = L.po_mvs_create(S.ptr)
    want = {"few_cams": "po_set_reference_camera", "no_cams": "po_set_reference_camera", "same_cam": "po_set_depth_range",
            "far": "po_set_depth_range", "border_0": None, "border_up": None, "seed": None}
    kept = []
    for r in out:
        by, p = classify(S, oracle_load(S, mo, r), r)
        if r["kind"] == "border_up" and not (by is None and p.LOD >= 1 and lod_fell_back(S, scene, p)):
            continue                                            # (this pixel is not background in this camera)
        assert by == want[r["kind"]], (name, r["kind"], by)
        if r["kind"] == "border_0":
            assert p.LOD == 0 and lod_fell_back(S, scene, p), (name, p.LOD)
        if r["kind"] in ("same_cam", "far"):
            assert p.refCamIdx >= 0 and p.depth > 0 and list(p.depthRange[:]) == [0.0, 0.0]
        kept.append(r)
    kinds = [r["kind"] for r in kept]
    assert all(kinds.count(k) >= 1 for k in want if k != "seed"), kinds
    if name == "pawn_lowtex":
        lods = [classify(S, oracle_load(S, mo, r), r)[1].LOD for r in kept if r["kind"] == "seed"]
        assert sum(1 for l in lods if l >= 1) >= 4 and max(lods) >= 2, lods
    L.po_mvs_destroy(mo)
    S.close()
    return kept


def main():
    doc = {"made_by": "tests/golden/make_resume_cloud.py (oracle, kernel arithmetic)",
           "scenes": {name: pick(name, scene) for name, scene in scenes().items()}}
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=0)
    for name, recs in doc["scenes"].items():
        kinds = [r["kind"] for r in recs]
        print(name, {k: kinds.count(k) for k in sorted(set(kinds))})
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
