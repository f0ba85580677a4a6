"""`python -m pais_mvs_amd.reconstruct scene.{nvm,nvm2,mvs} [--config config.txt] [--out DIR] [--max-rounds N] [--autosave-every N]
                                       [--undistort {measured-to-ideal,ideal-to-measured}] [--mesh [H] [--mesh-color]]`
`python -m pais_mvs_amd.reconstruct --filter cloud.mvs [--config config.txt] [--out DIR] [--statistical K,SIGMA] [--normal-agreement K,DEG]`
                                                                                      (the `-f` verb, TMVS.cpp:124-172)

The reference's `TMVS.exe -r` verb (TMVS.cpp:76-122) on the MI355X path: load NVM/NVM2 (+ images via PIL),
apply config.txt on top of the compiled-in defaults, refine the seeds, expand, write exp.mvs / exp.ply /
exp.psr.  NVM points are re-triangulated from their measurements like MVS::loadNVM does (`reCentering`,
patch.cpp:67-112).  An NVM / NVM2 scene WITHOUT points seeds itself as runReconstruct does (TMVS.cpp:97-103): features of
every image on the GPU (include/pais_feature.h), FeatureManager::setSeedPatches with --feature-max-dist, init.mvs written
before the seeds are refined.

A scene that ends in `.mvs` (seed.mvs, exp.mvs, auto_save.mvs; TMVS.cpp:87-88) resumes from that cloud: the file's embedded
configuration (MVS_V3) first, config.txt on top (:91-93), every patch through the loader constructor on the GPU
(MVS.load_patches), then the same refineSeedPatches / expansionPatches / writers.  While expanding, auto_save.mvs is written
every --autosave-every patches (mvs.cpp:265-268, checked after each round).

--mesh [H] meshes the expanded cloud after the cloud files are written (pais_mvs_amd.mesh: distance field and marching tetrahedra
on the GPU, grid pitch H or twice the cloud's sample spacing) and writes mesh.ply, coloured from the nearest patch; with
--mesh-color from the images of the cameras that see each vertex (the mesh rendered into every camera, Mesh.colors_from_images)."""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

from . import io
from .camera import Camera
from .config import default_config
from .mvs import MVS


def rgb_to_gray(rgb):
    # OpenCV's BGR2GRAY weights, fixed point as cv::cvtColor does for 8-bit (R 4899, G 9617, B 1868, shift 14)
    g = (rgb[..., 0].astype(np.int64) * 4899 + rgb[..., 1].astype(np.int64) * 9617 + rgb[..., 2].astype(np.int64) * 1868 + 8192) >> 14
    return np.clip(g, 0, 255).astype(np.uint8)


def load_image_gray(path: str):
    from PIL import Image
    im = Image.open(path)
    rgb = np.asarray(im.convert("RGB"))
    return rgb_to_gray(rgb), rgb


def load_cameras(cams_io, base, cfg):
    cams = []
    for c in cams_io:
        name = c.file_name.decode()
        path = name if os.path.isabs(name) else os.path.join(base, name)
        gray, rgb = load_image_gray(path)
        cams.append(Camera(focal=np.array(c.focal[:]), principle_point=np.array(c.principle_point[:]),
                           quaternion=np.array(c.quaternion[:]), center=np.array(c.center[:]), image=gray, name=name,
                           rgb=rgb, radial_distortion=c.radial_distortion).finalize(cfg.lodRatio, cfg.maxLOD,
                                                                                    build_edges=cfg.adaptiveGradientEnable))
    return cams


def undistort_cameras(cams, model: str, cfg, out: str, device: int):
    """--undistort: every camera through undistort_camera (include/pais_undistort.h).  The resampled RGB goes losslessly to
    OUT/undistorted/<stem>.png and the camera is renamed to that file with its radial term 0, so the .mvs files written
    afterwards resume from the ideal images: load_cameras re-reads images by name, and the grey image is taken from the
    resampled RGB exactly as a reload takes it.  -> (the new cameras, the lens of each old one)."""
    from PIL import Image
    from . import undistort as und
    folder = os.path.join(os.path.abspath(out), "undistorted")
    os.makedirs(folder, exist_ok=True)
    new, lenses, seen = [], [], set()
    for i, cam in enumerate(cams):
        base = os.path.splitext(os.path.basename(cam.name))[0] or ("cam%04d" % i)
        stem, n = base, 0
        while stem in seen:               # a.jpg and a.png of one scene: a, a_1 -- never a name another camera was given
            n += 1
            stem = "%s_%d" % (base, n)
        seen.add(stem)
        path = os.path.join(folder, stem + ".png")
        if len(path.encode()) > 255:
            raise RuntimeError("--undistort: %s does not fit the 255 bytes an MVS file holds for a camera's name" % path)
        lenses.append(und.lens_of(cam, model))
        c = und.undistort_camera(cam, model, cfg.lodRatio, cfg.maxLOD, build_edges=cfg.adaptiveGradientEnable, device=device, name=path,
                                 gray_of_rgb=rgb_to_gray)
        Image.fromarray(c.rgb if c.rgb is not None else c.image).save(path)
        new.append(c)
    return new, lenses


def undistort_measurements(pts_meas, lenses, device: int):
    """pts_meas: per point (camera indices, measured pixels) -> the same with every measurement ideal; one call of
    pais_undistort_points per camera.  A measurement beyond its lens's fold is dropped with its camera; a point left with
    fewer than two measurements cannot be re-triangulated and comes back as None, with a message."""
    from . import undistort as und
    by_cam = {}
    for p, (idx, meas) in enumerate(pts_meas):
        for k, c in enumerate(idx):
            by_cam.setdefault(c, []).append((p, k))
    ideal = [[None] * len(idx) for idx, _ in pts_meas]
    for c, where in sorted(by_cam.items()):
        xy, ok, _ = und.undistort_points([pts_meas[p][1][k] for p, k in where], lenses[c], device)
        for (p, k), q, good in zip(where, xy.tolist(), ok.tolist()):
            ideal[p][k] = q if good else None
    out = []
    for p, ((idx, _), row) in enumerate(zip(pts_meas, ideal)):
        keep = [k for k, q in enumerate(row) if q is not None]
        if len(keep) < len(idx) and len(keep) < 2:   # a point that came with fewer than two is passed on as it is
            print("point %d: %d of its %d measurements lie within their lens's fold; skipped" % (p, len(keep), len(idx)))
            out.append(None)
            continue
        out.append(([idx[k] for k in keep], [row[k] for k in keep]))
    return out


def parse_statistical(text: str):
    """--statistical K,SIGMA -> (k, sigma)"""
    try:
        k, sigma = text.split(",")
        return int(k), float(sigma)
    except ValueError:
        raise argparse.ArgumentTypeError("expected K,SIGMA (e.g. 8,2), got %r" % text)


def parse_normal_agreement(text: str):
    """--normal-agreement K,DEG -> (k, max_angle_deg)"""
    try:
        k, deg = text.split(",")
        return int(k), float(deg)
    except ValueError:
        raise argparse.ArgumentTypeError("expected K,DEG (e.g. 16,30), got %r" % text)


def parse_mesh_pitch(text: str):
    """--mesh H -> the grid pitch, positive"""
    try:
        h = float(text)
        if not (h > 0 and h < float("inf")):
            raise ValueError
        return h
    except ValueError:
        raise argparse.ArgumentTypeError("expected a positive grid pitch, got %r" % text)


def write_mesh(m: MVS, path: str, h=None, from_images: bool = False):
    """MVS.mesh of the driver's cloud as a PLY coloured from the nearest patch -> the Mesh.  from_images: every vertex takes
    the mean colour of the cameras that see it (Mesh.colors_from_images), the nearest patch's where none does."""
    msh = m.mesh(h)
    if from_images:
        bgr = msh.colors_from_images(m.cameras, m.camera_images_bgr(), cloud_bgr=m.colors_bgr(), centers=m.cloud()[:, :3], device=m.device)
    else:
        bgr = msh.colors(m.colors_bgr(), m.cloud()[:, :3], m.device)
    msh.write_ply(path, bgr)
    return msh


def parse_depth_consistency(text: str):
    """--depth-consistency RHO,TOL -> (rho, tol); either may be `auto` -> None"""
    try:
        rho, tol = (None if t.strip().lower() == "auto" else float(t) for t in text.split(","))
        if (rho is not None and not rho > 0) or (tol is not None and not tol >= 0):
            raise ValueError
        return rho, tol
    except ValueError:
        raise argparse.ArgumentTypeError("expected RHO,TOL with RHO > 0 and TOL >= 0, either may be `auto` (e.g. auto,auto), got %r" % text)


def run_filtering(path: str, config: str, out: str, device: int = 0, statistical=None, normal_agreement=None, depth_consistency=None):
    """runFiltering (TMVS.cpp:124-172): PMVS filters 1-3, then the PCMVS neighbour filter, with the reference's
    output names.  statistical = (k, sigma): the statistical outlier filter (MVS.statisticalFiltering) after them, written
    as SOR_filter.mvs / SOR_filter.ply.  normal_agreement = (k, degrees): the normal-agreement filter (MVS.normalFiltering)
    after those, written as NA_filter.mvs / NA_filter.ply.  depth_consistency = (rho, tol), either None for the default: the
    depth-consistency filter (MVS.depthFiltering) last, written as DC_filter.mvs / DC_filter.ply."""
    file_cfg, cams_io, pats = io.load_mvs(path)
    cfg = file_cfg or default_config()
    if os.path.exists(config):
        cfg = io.load_config(config, cfg)
    cams = load_cameras(cams_io, os.path.dirname(os.path.abspath(path)), cfg)
    m = MVS(cfg, cams, device=device)
    for p in pats:
        m.load_patch(p.center[:], p.normalS[:], list(p.cam_idx[:p.num_cam]), p.fitness, p.correlation)
    print("patches: %d" % m.num_patches())
    t0 = time.perf_counter()
    m.cellFiltering()
    m.writeMVS(os.path.join(out, "PMVS_filter1.mvs")); m.writePLY(os.path.join(out, "PMVS_filter1.ply"))
    m.visibilityFiltering()
    m.writeMVS(os.path.join(out, "PMVS_filter2.mvs")); m.writePLY(os.path.join(out, "PMVS_filter2.ply"))
    m.neighborCellFiltering(0.25)
    m.writeMVS(os.path.join(out, "PMVS_filter3.mvs")); m.writePLY(os.path.join(out, "PMVS_filter3.ply"))
    ms = m.neighborPatchFiltering(0.25)
    m.writeMVS(os.path.join(out, "PCMVS_filter.mvs")); m.writePLY(os.path.join(out, "PCMVS_filter.ply"))
    print("patches after filtering: %d  time %.3f s (neighbour-count kernel %.3f ms)" % (m.num_patches(), time.perf_counter() - t0, ms))
    if statistical is not None:
        removed, ms = m.statisticalFiltering(*statistical)
        m.writeMVS(os.path.join(out, "SOR_filter.mvs")); m.writePLY(os.path.join(out, "SOR_filter.ply"))
        print("patches after the statistical filter (k %d, sigma %g): %d  removed %d (k-nearest kernels %.3f ms)"
              % (statistical[0], statistical[1], m.num_patches(), removed, ms))
    if normal_agreement is not None:
        removed, ms = m.normalFiltering(*normal_agreement)
        m.writeMVS(os.path.join(out, "NA_filter.mvs")); m.writePLY(os.path.join(out, "NA_filter.ply"))
        print("patches after the normal-agreement filter (k %d, %g degrees): %d  removed %d (search and fit kernels %.3f ms)"
              % (normal_agreement[0], normal_agreement[1], m.num_patches(), removed, ms))
    if depth_consistency is not None:
        removed, ms = m.depthFiltering(*depth_consistency)
        m.writeMVS(os.path.join(out, "DC_filter.mvs")); m.writePLY(os.path.join(out, "DC_filter.ply"))
        print("patches after the depth-consistency filter (rho %s, tol %s): %d  removed %d (render and test kernels %.3f ms)"
              % tuple(["auto" if x is None else "%g" % x for x in depth_consistency] + [m.num_patches(), removed, ms]))
    m.close()


def scene_kind(path: str) -> str:
    """runReconstruct's dispatch on the file extension (TMVS.cpp:78-89): "mvs", "nvm2", else the NVM loader."""
    low = path.lower()
    return "mvs" if low.endswith(".mvs") else ("nvm2" if low.endswith(".nvm2") else "nvm")


def load_scene(a):
    """The driver with the scene's cameras and patches: NVM / NVM2 seeds, or the cloud of an .mvs file (unexpanded)."""
    kind = scene_kind(a.scene)
    base = os.path.dirname(os.path.abspath(a.scene))
    if kind == "mvs":
        # MVS::loadMVS first (an MVS_V3 file carries its configuration), config.txt on top (TMVS.cpp:87-93)
        file_cfg, cams_io, pats = io.load_mvs(a.scene)
        cfg = file_cfg or default_config()
        if os.path.exists(a.config):
            cfg = io.load_config(a.config, cfg)
        m = MVS(cfg, load_cameras(cams_io, base, cfg), device=a.device)
        m.load_patches(pats)
        return m
    cfg = default_config()
    if os.path.exists(a.config):
        cfg = io.load_config(a.config, cfg)
    cams_io, pts = io.load_nvm(a.scene, nvm2=kind == "nvm2")
    cams = load_cameras(cams_io, base, cfg)
    # FileLoader::loadNvmPatch (fileloader.cpp:155-160): measurements are offsets from the image centre;
    # MVS::loadNVM then re-triangulates every point (reCentering, mvs.cpp:160-168)
    pts_meas = []
    for p in pts:
        idx = list(p.cam_idx[:p.num_meas])
        pts_meas.append((idx, [[p.xy[i][0] + cams[c].width // 2, p.xy[i][1] + cams[c].height // 2] for i, c in enumerate(idx)]))
    if a.undistort:
        cams, lenses = undistort_cameras(cams, a.undistort, cfg, a.out, a.device)
        pts_meas = undistort_measurements(pts_meas, lenses, a.device)
    m = MVS(cfg, cams, device=a.device)
    for p, pm in zip(pts, pts_meas):
        if pm is None:                    # --undistort left it fewer than two measurements
            continue
        idx, meas = pm
        m.add_seed_measured(p.center[:], idx, meas, recenter=not a.no_recenter)
    return m


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("scene")
    ap.add_argument("--filter", action="store_true", help="the -f verb: filter an .mvs cloud instead of reconstructing")
    ap.add_argument("--config", default="config.txt")
    ap.add_argument("--out", default=".")
    ap.add_argument("--parents-per-round", type=int, default=4096)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--no-recenter", action="store_true", help="keep the NVM points as they are (skip MVS::reCentering)")
    ap.add_argument("--max-rounds", type=int, default=0, help="stop the expansion after N rounds (0: until the queue is empty)")
    ap.add_argument("--feature-max-dist", type=float, default=3.0,
                    help="epipolar distance bound (pixels) of the feature seeding of a scene without points (TMVS.cpp:98)")
    ap.add_argument("--autosave-every", type=int, default=500,
                    help="write auto_save.mvs whenever the cloud has grown by N patches (mvs.cpp:265-268); 0: never")
    ap.add_argument("--undistort", choices=["measured-to-ideal", "ideal-to-measured"], default=None,
                    help="take the NVM radial term out of images and measurements first (include/pais_undistort.h): the direction "
                         "in which the closed form of the term runs; default: the term is ignored, as the reference does")
    ap.add_argument("--statistical", type=parse_statistical, default=None, metavar="K,SIGMA",
                    help="with --filter: after the PCMVS step, delete the patches whose mean distance to their K nearest patches "
                         "lies SIGMA deviations above the cloud's mean, and write SOR_filter.mvs / SOR_filter.ply")
    ap.add_argument("--normal-agreement", type=parse_normal_agreement, default=None, metavar="K,DEG",
                    help="with --filter: after the steps above, delete the patches whose normal lies more than DEG degrees from the "
                         "plane through their K nearest patches, and write NA_filter.mvs / NA_filter.ply")
    ap.add_argument("--depth-consistency", type=parse_depth_consistency, default=None, metavar="RHO,TOL",
                    help="with --filter: last, render the patches as discs of radius RHO into every camera and delete those that fewer "
                         "than minCamNum of their own cameras see within TOL of the depth map; either may be `auto` (the file's "
                         "neighbour radius, and RHO); writes DC_filter.mvs / DC_filter.ply")
    ap.add_argument("--mesh", type=parse_mesh_pitch, nargs="?", const=0.0, default=None, metavar="H",
                    help="after the cloud files, mesh the cloud on a grid of pitch H (default: twice its sample spacing) and write mesh.ply")
    ap.add_argument("--mesh-color", action="store_true",
                    help="with --mesh: colour the mesh's vertices from the images of the cameras that see them, not from the nearest patch")
    a = ap.parse_args(argv)
    if a.mesh_color and a.mesh is None:
        ap.error("--mesh-color belongs to --mesh")
    if a.mesh is not None and a.filter:
        ap.error("--mesh belongs to a reconstruction, not to --filter")
    if a.depth_consistency and not a.filter:
        ap.error("--depth-consistency belongs to --filter")
    if a.statistical and not a.filter:
        ap.error("--statistical belongs to --filter")
    if a.normal_agreement and not a.filter:
        ap.error("--normal-agreement belongs to --filter")
    if a.undistort and (a.filter or scene_kind(a.scene) == "mvs"):
        ap.error("--undistort is for .nvm / .nvm2 scenes: the cameras of an .mvs file already say what they are")
    if a.filter:
        return run_filtering(a.scene, a.config, a.out, a.device, a.statistical, a.normal_agreement, a.depth_consistency)
    m = load_scene(a)
    if scene_kind(a.scene) != "mvs" and m.num_patches() == 0:
        # no initial seeds: FeatureManager::setSeedPatches(cameras, 3.0, &mvs), then init.mvs (TMVS.cpp:97-103)
        m.seed_from_images(a.feature_max_dist)
        if m.num_patches() == 0:
            print("try less minCamNum")
        m.writeMVS(os.path.join(a.out, "init.mvs"))
    if a.autosave_every > 0:
        m.set_checkpoint(a.autosave_every, lambda _n: m.writeMVS(os.path.join(a.out, "auto_save.mvs")))
    t0 = time.perf_counter()
    m.refineSeedPatches()
    m.writeMVS(os.path.join(a.out, "seed.mvs"))
    m.expansionPatches(a.parents_per_round, a.max_rounds)
    dt = time.perf_counter() - t0
    m.writeMVS(os.path.join(a.out, "exp.mvs"))
    m.writePLY(os.path.join(a.out, "exp.ply"))
    m.writePSR(os.path.join(a.out, "exp.psr"))
    if a.mesh is not None:
        msh = write_mesh(m, os.path.join(a.out, "mesh.ply"), a.mesh or None, a.mesh_color)
        print("mesh: %d vertices  %d triangles  pitch %g" % (len(msh.vertices), len(msh.triangles), msh.grid.h))
    st = m.stats()
    print("patches %d  refined %d  time %.3f s" % (m.num_patches(), st.seeds_refined + st.candidates_effective, dt))
    m.close()


if __name__ == "__main__":
    main()
