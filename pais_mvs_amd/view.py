"""Look at a cloud: the reference's `-v` (viewer) and `-a` (animate) verbs (TMVS.cpp:54-74, view/mvsviewer.cpp) without a
display -- the cloud is rendered on the GPU (pais_mvs_amd.render) through cameras of its own file or from an orbit around it,
and the frames are written as images.

    python -m pais_mvs_amd.view cloud.{mvs,ply,npy} [--camera I [I ...]] [--orbit N] [--mode disc|point] [--radius R]
           [--point-size S] [--out DIR] [--cameras] [--animate F] [--pick U,V] [--shade auto|color|normal|z] [--visibility]

Per view k: view_kkk.png (the patch colours if the cloud has some, else the normal map 127.5 (n' + 1); --shade z: grey by
|n'z|) and depth_kkk.npy (float64, +inf where nothing is seen).  Views are the --camera ones in the order given, then the
--orbit ones.  --cameras draws the rig as red points of size 5 (mvsviewer.cpp:144-179); --animate F writes anim_fff.png, frame
f showing the first ceil((f + 1) n / F) patches through the first view (addPatchesAnimate, mvsviewer.cpp:258-265); --pick U,V
prints the record of the patch under that pixel of the first view (printPatchInformation, mvsviewer.cpp:441-471);
--visibility depth-tests every point against the disc render of each --camera view (render.visibility, tolerance = the
radius) and prints, per listed camera, how many points fall under each code (visible, occluded, in_front, empty, outside,
behind).

--mesh mesh.{ply,obj} draws that triangle mesh (pais_mvs_amd.mesh's writers) in place of the discs, through the same views
(render.render_mesh): --shade normal is flat shading by the triangle's normal, z grey by |n'z|, color Gouraud from the PLY's
vertex colours; --pick prints the triangle and the pixel's barycentric weights; --animate grows the triangle list;
--visibility tests the cloud's points against the mesh (tolerance --radius, default as for discs)."""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import numpy as np


def parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m pais_mvs_amd.view", description=__doc__.split("\n\n")[0])
    ap.add_argument("cloud", help="cloud.mvs, cloud.ply or cloud.npy ((n,6))")
    ap.add_argument("--camera", type=int, nargs="+", default=[], metavar="I", help="cameras of the .mvs file to look through")
    ap.add_argument("--orbit", type=int, default=0, metavar="N", help="N views on a circle around the cloud")
    ap.add_argument("--elevation", type=float, default=20.0)
    ap.add_argument("--mode", choices=["disc", "point"], default="disc")
    ap.add_argument("--radius", type=float, help="disc radius in world units (default: the file's neighborRadius, else from the point density)")
    ap.add_argument("--point-size", type=int, default=1, help="point mode: square of S pixels")
    ap.add_argument("--width", type=int)
    ap.add_argument("--height", type=int)
    ap.add_argument("--focal", type=float, help="focal of the orbit views (default: the first camera's, else 1.2 x width)")
    ap.add_argument("--out", default="view_out")
    ap.add_argument("--cameras", action="store_true", help="draw the rig as red points of size 5")
    ap.add_argument("--animate", type=int, default=0, metavar="F")
    ap.add_argument("--pick", metavar="U,V")
    ap.add_argument("--shade", choices=["auto", "color", "normal", "z"], default="auto")
    ap.add_argument("--no-cull", action="store_true", help="also draw discs seen from behind")
    ap.add_argument("--visibility", action="store_true", help="per --camera view: how many points are visible, occluded, ... (disc mode)")
    ap.add_argument("--mesh", metavar="MESH", help="mesh.ply or mesh.obj: draw this triangle mesh in place of the discs")
    ap.add_argument("--device", type=int, default=0)
    return ap


def parse_args(argv=None):
    ap = parser()
    a = ap.parse_args(argv)
    ext = a.cloud.lower().rsplit(".", 1)[-1]
    if ext != "mvs" and (a.camera or a.cameras):
        ap.error("--camera / --cameras need the cameras of an .mvs file; a .%s cloud has none" % ext)
    if not a.camera and a.orbit <= 0:
        ap.error("give --camera I [I ...] and / or --orbit N")
    if a.pick:
        try:
            a.pick = tuple(int(x) for x in a.pick.split(","))
            assert len(a.pick) == 2
        except Exception:
            ap.error("--pick takes U,V (two integers)")
    if a.mesh is not None:
        if a.mesh.lower().rsplit(".", 1)[-1] not in ("ply", "obj"):
            ap.error("--mesh ends in .ply or .obj")
        if a.mode != "disc" or a.cameras:
            ap.error("--mesh draws triangles: --mode point and --cameras do not apply")
    if a.visibility and (not a.camera or a.mode != "disc"):
        ap.error("--visibility tests against the disc render of the --camera views: give --camera, and not --mode point")
    if a.animate < 0 or a.orbit < 0:
        ap.error("--animate and --orbit are counts")
    return a


def ply_colors(path: str):
    """(n,3) uint8 BGR of an ascii PLY with red / green / blue (or diffuse_*) vertex properties, else None."""
    props, n = [], 0
    with open(path, "r") as f:
        for line in f:
            w = line.split()
            if w[:1] == ["element"] and w[1] == "vertex":
                n = int(w[2])
            elif w[:1] == ["property"]:
                props.append(w[-1].replace("diffuse_", ""))
            elif w[:1] == ["end_header"]:
                break
        if not all(c in props for c in ("red", "green", "blue")) or not n:
            return None
        rows = np.loadtxt(f, dtype=np.float64, ndmin=2, max_rows=n)
    return rows[:, [props.index("blue"), props.index("green"), props.index("red")]].astype(np.uint8)


def default_radius(centers) -> float:
    """Without a neighborRadius: 1.5 x the pitch of n samples spread over a surface of the bounding box's diagonal squared."""
    c = np.asarray(centers, np.float64).reshape(-1, 3)
    d = float(np.linalg.norm(c.max(axis=0) - c.min(axis=0))) if len(c) else 0.0
    return 1.5 * d / math.sqrt(len(c)) if d > 0 else 1.0


def shade(r, a, normals, bgr):
    """(V,H,W,3) uint8 RGB"""
    how = a.shade if a.shade != "auto" else ("color" if bgr is not None else "normal")
    if how == "color":
        if bgr is None:
            raise SystemExit("--shade color: the cloud has no colours")
        return r.color(bgr)[..., ::-1]
    nm = r.normal_map(normals)
    if how == "normal":
        return nm
    z = np.abs(nm[..., 2].astype(np.float64) - 127.5) * 2.0
    g = np.where(r.id >= 0, np.clip(z, 32, 255), 0).astype(np.uint8)
    return np.stack([g, g, g], axis=-1)


def patch_information(k: int, cloud, patches) -> dict:
    info = {"patch": int(k), "center": [float(x) for x in cloud[k, :3]], "normal": [float(x) for x in cloud[k, 3:]]}
    if patches is not None:
        p = patches[k]
        info.update(fitness=float(p.fitness), correlation=float(p.correlation), cameras=[int(p.cam_idx[i]) for i in range(p.num_cam)])
    return info


def shade_mesh(r, a, m, bgr):
    """(V,H,W,3) uint8 RGB of a mesh render"""
    from . import render as rnd
    how = a.shade if a.shade != "auto" else ("color" if bgr is not None else "normal")
    if how == "color":
        if bgr is None:
            raise SystemExit("--shade color: the mesh has no vertex colours")
        col = r.interpolate(bgr.astype(np.float64), rnd.barycentric(r, m.vertices, m.triangles))
        return np.clip(np.rint(col), 0, 255).astype(np.uint8)[..., ::-1]
    nm = r.triangle_normals(m.vertices, m.triangles)
    if how == "normal":
        return nm
    z = np.abs(nm[..., 2].astype(np.float64) - 127.5) * 2.0
    g = np.where(r.id >= 0, np.clip(z, 32, 255), 0).astype(np.uint8)
    return np.stack([g, g, g], axis=-1)


def main_mesh(a, cloud, views, width, height, radius) -> int:
    """the --mesh branch of main(): the same views, files and JSON line, triangles in place of discs"""
    from PIL import Image
    from . import mesh as msh
    from . import render as rnd
    m, bgr = msh.read_mesh(a.mesh)
    r = rnd.render_mesh(m.vertices, m.triangles, views, width, height, cull=not a.no_cull, device=a.device)
    img = shade_mesh(r, a, m, bgr)
    os.makedirs(a.out, exist_ok=True)
    for k in range(len(views)):
        Image.fromarray(np.ascontiguousarray(img[k]), "RGB").save(os.path.join(a.out, "view_%03d.png" % k))
        np.save(os.path.join(a.out, "depth_%03d.npy" % k), r.depth[k])
    n = len(m.triangles)
    for f in range(a.animate):
        k = min(n, int(math.ceil((f + 1) * n / a.animate)))
        part = msh.Mesh(m.vertices, m.triangles[:k])
        fr = rnd.render_mesh(part.vertices, part.triangles, views[:1], width, height, cull=not a.no_cull, device=a.device)
        Image.fromarray(np.ascontiguousarray(shade_mesh(fr, a, part, bgr)[0]), "RGB").save(os.path.join(a.out, "anim_%03d.png" % f))
    out = {"views": len(views), "width": width, "height": height, "n": len(cloud), "mode": "mesh", "vertices": len(m.vertices), "triangles": n,
           "kernel_ms": r.kernel_ms, "covered_pixels": int((r.id >= 0).sum()), "out": a.out}
    if a.visibility:
        vis = rnd.mesh_visibility(m.vertices, m.triangles, views[:len(a.camera)], width, height, cloud[:, :3], radius, cull=not a.no_cull,
                                  occluder=False, margin=False, device=a.device)
        out["visibility"] = [dict(camera=int(i), **{name: int(c) for name, c in zip(rnd.VIS_CODES, row)})
                             for i, row in zip(a.camera, vis.view_counts())]
        for row in out["visibility"]:
            print("camera %d: " % row["camera"] + "  ".join("%s %d" % (name, row[name]) for name in rnd.VIS_CODES))
    if a.pick:
        k = r.pick(0, a.pick[0], a.pick[1])
        out["pick"] = None
        if k >= 0:
            w = rnd.barycentric(rnd.Render(r.depth[:1], r.id[:1], 0.0, views[:1]), m.vertices, m.triangles).weights[0, a.pick[1], a.pick[0]]
            out["pick"] = {"triangle": int(k), "vertices": [int(x) for x in m.triangles[k]], "barycentric": [float(x) for x in w],
                           "depth": float(r.depth[0, a.pick[1], a.pick[0]])}
    print(json.dumps(out))
    return 0


def main(argv=None) -> int:
    a = parse_args(argv)
    from PIL import Image
    from . import render as rnd
    from .evaluate import load_cloud
    cloud = load_cloud(a.cloud)
    cen, nrm = cloud[:, :3], cloud[:, 3:]
    ext = a.cloud.lower().rsplit(".", 1)[-1]
    cfg, cams, pats, bgr = None, [], None, None
    if ext == "mvs":
        from . import io
        cfg, cams, pats = io.load_mvs(a.cloud)
    elif ext == "ply":
        bgr = ply_colors(a.cloud)
    for i in a.camera:
        if not 0 <= i < len(cams):
            raise SystemExit("--camera %d: the file holds %d cameras" % (i, len(cams)))
    # an .mvs camera carries no image size: its principal point is the image centre (camera.cpp:101-106)
    first = cams[a.camera[0]] if a.camera else (cams[0] if cams else None)
    width = a.width or (int(2 * first.principle_point[0]) if first is not None else 640)
    height = a.height or (int(2 * first.principle_point[1]) if first is not None else 480)
    focal = a.focal or (float(first.focal[0]) if first is not None else 1.2 * width)
    views = [rnd.view_of(cams[i]) for i in a.camera]
    if a.orbit:
        up = (0.0, 0.0, 1.0)
        if cams:  # image y points down in every camera: the rig's up is the mean of -R[1]
            up = -np.mean([np.array(rnd.view_of(c).R[3:6]) for c in cams], axis=0)
        views += rnd.orbit_views(cen, a.orbit, focal, width, height, a.elevation, up)
    if a.mode == "disc":
        radius = a.radius or (cfg.neighborRadius if cfg is not None and cfg.neighborRadius > 0 else default_radius(cen))
    else:
        radius = float(a.point_size)
    if a.mesh is not None:
        return main_mesh(a, cloud, views, width, height, radius)
    kw = dict(mode=a.mode, radius=radius, cull_back=not a.no_cull, device=a.device)
    r = rnd.render(cen, nrm, views, width, height, **kw)
    img = shade(r, a, nrm, bgr)
    depth = r.depth
    if a.cameras:
        rig = rnd.render(np.array([c.center[:] for c in cams], np.float64), None, views, width, height, mode="point", radius=5, device=a.device)
        from_rig, depth = rnd.composite(r, rig)
        img = np.where(from_rig[..., None], np.array([255, 0, 0], np.uint8), img)
    os.makedirs(a.out, exist_ok=True)
    for k in range(len(views)):
        Image.fromarray(np.ascontiguousarray(img[k]), "RGB").save(os.path.join(a.out, "view_%03d.png" % k))
        np.save(os.path.join(a.out, "depth_%03d.npy" % k), depth[k])
    n = len(cen)
    for f in range(a.animate):
        m = min(n, int(math.ceil((f + 1) * n / a.animate)))
        fr = rnd.render(cen[:m], nrm[:m], views[:1], width, height, **kw)
        Image.fromarray(np.ascontiguousarray(shade(fr, a, nrm, bgr)[0]), "RGB").save(os.path.join(a.out, "anim_%03d.png" % f))
    out = {"views": len(views), "width": width, "height": height, "n": n, "mode": a.mode, "radius": radius, "kernel_ms": r.kernel_ms,
           "covered_pixels": int((r.id >= 0).sum()), "out": a.out}
    if a.visibility:
        vis = rnd.visibility(cen, nrm, views[:len(a.camera)], width, height, radius=radius, cull_back=not a.no_cull, occluder=False,
                             margin=False, device=a.device)
        out["visibility"] = [dict(camera=int(i), **{name: int(c) for name, c in zip(rnd.VIS_CODES, row)})
                             for i, row in zip(a.camera, vis.view_counts())]
        for row in out["visibility"]:
            print("camera %d: " % row["camera"] + "  ".join("%s %d" % (name, row[name]) for name in rnd.VIS_CODES))
    if a.pick:
        k = r.pick(0, a.pick[0], a.pick[1])
        out["pick"] = patch_information(k, cloud, pats) if k >= 0 else None
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
