"""Render a cloud into pinhole views: z-buffered patch splats on the GPU (include/pais_render.h).

The reference checks a result by looking at it (the `-v` / `-a` verbs, view/mvsviewer.cpp).  Here the GPU produces, per view, a
depth map and a patch-id map; colour images, normal maps, depth images and picking are host arithmetic on those two maps.
There is no CPU fallback: render() raises without a GPU.

    r = render(centers, normals, [view_of(cam) for cam in cameras], 640, 480, radius=spacing)
    r.depth[v], r.id[v], r.color(bgr)[v], r.normal_map(normals)[v], r.pick(v, u, v_px)
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Sequence

import numpy as np

from . import _lib
from .camera import quaternion_to_rotation

MODES = {"disc": _lib.RENDER_DISC, "point": _lib.RENDER_POINT}


def make_view(R, T, focal, pp) -> "_lib.View":
    v = _lib.View()
    v.R[:] = [float(x) for x in np.asarray(R, np.float64).reshape(9)]
    v.T[:] = [float(x) for x in np.asarray(T, np.float64).reshape(3)]
    f = np.asarray(focal, np.float64).reshape(-1)
    v.focal[:] = [float(f[0]), float(f[-1])]
    v.pp[:] = [float(pp[0]), float(pp[1])]
    return v


def view_of(camera) -> "_lib.View":
    """The pais_view of a camera.Camera (its rotation / translation / focal / principle_point) or of an io.IoCamera (R from
    the quaternion and T = -R C by the statements of Camera.finalize, so both give the same bits)."""
    R = getattr(camera, "rotation", None)
    if R is not None:
        return make_view(R, camera.translation, camera.focal, camera.principle_point)
    R = quaternion_to_rotation(camera.quaternion[:])
    c = [float(x) for x in camera.center[:]]
    T = [-(R[i, 0] * c[0] + R[i, 1] * c[1] + R[i, 2] * c[2]) for i in range(3)]
    return make_view(R, T, camera.focal[:], camera.principle_point[:])


def look_at_view(C_, target, up, focal: float, width: int, height: int) -> "_lib.View":
    """A view at C_ looking at target, image y pointing away from `up` (synth._look_at, flipped as the synthetic rigs do)."""
    from .synth import _look_at
    C_, target, up = (np.asarray(a, np.float64) for a in (C_, target, up))
    R = _look_at(C_, target, up)
    if (R[1] @ up) > 0:
        R = np.stack([-R[0], -R[1], R[2]])
    return make_view(R, -(R @ C_), (focal, focal), (float(width >> 1), float(height >> 1)))


def orbit_geometry(centers, focal: float, width: int, height: int):
    """(box centre, bounding-sphere radius, distance) of orbit_views: the sphere around the bounding box's centre through its
    corners, seen from `distance`, projects to a circle of 0.95 x the smallest half extent of the frame around the principal
    point -- the cone tangent to a sphere of radius r at distance D has image radius focal r / sqrt(D D - r r)."""
    c = np.asarray(centers, np.float64).reshape(-1, 3)
    if not len(c):
        raise ValueError("orbit_views: empty cloud")
    lo, hi = c.min(axis=0), c.max(axis=0)
    mid = 0.5 * (lo + hi)
    r = 0.5 * float(np.linalg.norm(hi - lo))
    if not r > 0:
        r = 1.0
    ppx, ppy = float(width >> 1), float(height >> 1)
    half = 0.95 * min(ppx, width - 1 - ppx, ppy, height - 1 - ppy)
    if not half > 0:
        raise ValueError("orbit_views: a %d x %d frame has no room around its principal point" % (width, height))
    return mid, r, r * math.sqrt(1.0 + (focal / half) ** 2)


def orbit_views(centers, n: int, focal: float, width: int, height: int, elevation_deg: float = 20.0, up=(0.0, 0.0, 1.0)):
    """n look-at views on a circle around the centre of the cloud's bounding box, at the distance from which the bounding
    sphere fits the frame: what resetCamera() gives the viewer (mvsviewer.cpp:255), turned around `up`."""
    mid, _, dist = orbit_geometry(centers, focal, width, height)
    up = np.asarray(up, np.float64)
    up = up / np.linalg.norm(up)
    a = np.array([1.0, 0.0, 0.0]) if abs(up[0]) < 0.9 else np.array([0.0, 1.0, 0.0])
    e1 = np.cross(up, a)
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(up, e1)
    el = math.radians(elevation_deg)
    out = []
    for i in range(int(n)):
        az = 2 * math.pi * i / n
        d = math.cos(el) * (math.cos(az) * e1 + math.sin(az) * e2) + math.sin(el) * up
        out.append(look_at_view(mid + dist * d, mid, up, focal, width, height))
    return out


class Render:
    """The product of render(): depth (V,H,W) float64 (+inf where empty), id (V,H,W) int32 (-1 where empty), kernel_ms, and
    the views it was rendered into."""

    def __init__(self, depth, id, kernel_ms: float = 0.0, views=None, counts=None):
        self.depth = np.asarray(depth, np.float64)
        self.id = np.asarray(id, np.int32)
        if self.depth.ndim != 3 or self.depth.shape != self.id.shape:
            raise ValueError("Render: depth and id are (V, H, W) arrays of one shape, got %s and %s" % (self.depth.shape, self.id.shape))
        self.kernel_ms = float(kernel_ms)
        self.views = list(views) if views is not None else None
        self.counts = counts or {}

    def color(self, bgr, background=(0, 0, 0)) -> np.ndarray:
        """(V,H,W,3) uint8: the colour of the patch each pixel shows, `background` where it shows none."""
        col = np.asarray(bgr, np.uint8).reshape(-1, 3)
        out = np.empty(self.id.shape + (3,), np.uint8)
        out[...] = np.asarray(background, np.uint8)
        hit = self.id >= 0
        out[hit] = col[self.id[hit]]
        return out

    def normal_map(self, normals, background=(0, 0, 0)) -> np.ndarray:
        """(V,H,W,3) uint8: 127.5 (n' + 1) with n' = R n the camera-space normal of the patch each pixel shows."""
        if self.views is None:
            raise ValueError("normal_map: this Render carries no views")
        nrm = np.asarray(normals, np.float64).reshape(-1, 3)
        out = np.empty(self.id.shape + (3,), np.uint8)
        out[...] = np.asarray(background, np.uint8)
        for v, view in enumerate(self.views):
            hit = self.id[v] >= 0
            nc = nrm[self.id[v][hit]] @ np.array(view.R[:]).reshape(3, 3).T
            out[v][hit] = np.clip(127.5 * (nc + 1.0), 0, 255).astype(np.uint8)
        return out

    def depth_image(self, v: int) -> np.ndarray:
        """(H,W) uint8 of view v: the finite depths stretched min-max over 255 (nearest) .. 1 (farthest); 0 where empty."""
        d = self.depth[v]
        out = np.zeros(d.shape, np.uint8)
        hit = np.isfinite(d)
        if hit.any():
            lo, hi = float(d[hit].min()), float(d[hit].max())
            s = (hi - d[hit]) / (hi - lo) if hi > lo else np.ones(int(hit.sum()))
            out[hit] = np.rint(1.0 + 254.0 * s).astype(np.uint8)
        return out

    def interpolate(self, vertex_values, bary: "Barycentric", triangles=None, background=0.0) -> np.ndarray:
        """(V,H,W,C) float64: per covered pixel of a mesh render the barycentric mix of its triangle's three vertex values
        (n,C) -- Gouraud colour, smooth normals; `background` where nothing is covered."""
        tri = bary.triangles if triangles is None else np.asarray(triangles, np.int32).reshape(-1, 3)
        val = np.asarray(vertex_values, np.float64)
        val = val.reshape(len(val), -1)
        out = np.empty(self.id.shape + (val.shape[1],), np.float64)
        out[...] = background
        hit = self.id >= 0
        corners = val[tri[self.id[hit]]]                          # (m, 3, C)
        out[hit] = (bary.weights[hit][:, :, None] * corners).sum(axis=1)
        return out

    def triangle_normals(self, vertices, triangles, background=(0, 0, 0)) -> np.ndarray:
        """(V,H,W,3) uint8 of a mesh render: flat shading, 127.5 (n' + 1) with n' the camera-space unit normal
        R ((B - A) x (C - A)) of the triangle each pixel shows."""
        v = np.asarray(vertices, np.float64).reshape(-1, 3)
        t = np.asarray(triangles, np.int32).reshape(-1, 3)
        n = np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])
        ln = np.sqrt((n * n).sum(axis=1, keepdims=True))
        return self.normal_map(n / np.where(ln > 0, ln, 1.0), background)

    def pick(self, v: int, u: int, v_px: int) -> int:
        """The splat shown at pixel (u, v_px) of view v, -1 if none (or outside the image): pointPickEvent."""
        _, h, w = self.id.shape
        if not (0 <= u < w and 0 <= v_px < h):
            return -1
        return int(self.id[v, v_px, u])


def last_counts() -> dict:
    L = _lib.load()
    c = [C.c_int64(0) for _ in range(4)]
    L.pais_render_last_counts(*[C.byref(x) for x in c])
    out = dict(zip(("tiles", "covered_pairs", "depth_atomics", "id_atomics"), (int(x.value) for x in c)))
    out["packed"] = int(L.pais_render_last_packed())
    return out


def _mesh_arrays(what: str, vertices, triangles):
    ver = np.ascontiguousarray(vertices, dtype=np.float64)
    tri = np.ascontiguousarray(triangles, dtype=np.int32)
    if ver.ndim != 2 or ver.shape[1] != 3:
        raise ValueError("%s: vertices is an (n, 3) array, got %s" % (what, ver.shape))
    if tri.ndim != 2 or tri.shape[1] != 3:
        raise ValueError("%s: triangles is an (m, 3) array of vertex indices, got %s" % (what, tri.shape))
    return ver, tri


def mesh_last_ms() -> dict:
    """Kernel milliseconds of this thread's last render_mesh() / mesh_visibility(): setup, depth phase, id phase."""
    ms = (C.c_double * 3)()
    _lib.load().pais_mesh_render_last_ms(ms)
    return {"setup": ms[0], "depth": ms[1], "id": ms[2]}


def render_mesh(vertices, triangles, views: Sequence["_lib.View"], width: int, height: int, cull: bool = True, device: int = 0) -> Render:
    """pais_mesh_render: an indexed mesh (vertices (n,3), triangles (m,3)) into the views; id is the triangle index.  cull:
    PAIS_RENDER_CULL_BACK, triangles whose (B - A) x (C - A) points away from the view are skipped."""
    ver, tri = _mesh_arrays("render_mesh", vertices, triangles)
    views = list(views)
    nv = len(views)
    arr = (_lib.View * max(nv, 1))(*views)
    depth = np.empty((nv, int(height), int(width)), np.float64)
    idm = np.empty((nv, int(height), int(width)), np.int32)
    ms = C.c_double(0)
    L = _lib.load()
    rc = L.pais_mesh_render(int(device), _lib.RENDER_CULL_BACK if cull else 0, len(ver), _ptr(ver, C.c_double), len(tri), _ptr(tri, C.c_int32),
                            nv, arr, int(width), int(height), _ptr(depth, C.c_double), _ptr(idm, C.c_int32), C.byref(ms))
    if rc:
        raise RuntimeError("pais_mesh_render failed (%d): %s" % (rc, L.pais_render_last_error().decode()))
    return Render(depth, idm, ms.value, views, last_counts())


class Barycentric:
    """barycentric()'s product: weights (V,H,W,3) = (w_a, w_b, w_c) / S per covered pixel (NaN where empty), t (V,H,W) = D / S,
    the statements' depth (+inf where empty), and the triangles (m,3) the ids index."""

    def __init__(self, weights, t, triangles):
        self.weights, self.t, self.triangles = weights, t, triangles


def barycentric(render: Render, vertices, triangles) -> Barycentric:
    """The statements of pais_mesh_render (include/pais_render.h) in numpy, for the triangle the id map names at every covered
    pixel: elementwise double arithmetic in the header's order, so t equals the rendered depth bit for bit."""
    ver, tri = _mesh_arrays("barycentric", vertices, triangles)
    if render.views is None:
        raise ValueError("barycentric: this Render carries no views")
    V, H, W = render.id.shape
    weights = np.full((V, H, W, 3), np.nan)
    t = np.full((V, H, W), np.inf)
    for v, view in enumerate(render.views):
        R, T = list(view.R[:]), list(view.T[:])
        cam = np.stack([((R[3 * k] * ver[:, 0] + R[3 * k + 1] * ver[:, 1]) + R[3 * k + 2] * ver[:, 2]) + T[k] for k in range(3)], axis=1)
        vv, uu = np.nonzero(render.id[v] >= 0)
        if not len(vv):
            continue
        ids = tri[render.id[v][vv, uu]]
        rx = (uu.astype(np.float64) - view.pp[0]) / view.focal[0]
        ry = (vv.astype(np.float64) - view.pp[1]) / view.focal[1]

        def edge(p, q):
            fwd = (p < q)[:, None]
            lo, hi = np.where(fwd, cam[p], cam[q]), np.where(fwd, cam[q], cam[p])
            n = np.stack([lo[:, 1] * hi[:, 2] - lo[:, 2] * hi[:, 1], lo[:, 2] * hi[:, 0] - lo[:, 0] * hi[:, 2],
                          lo[:, 0] * hi[:, 1] - lo[:, 1] * hi[:, 0]], axis=1)
            return np.where(fwd, n, -n)

        a, b, c = ids[:, 0], ids[:, 1], ids[:, 2]
        ma, mb, mc = edge(b, c), edge(c, a), edge(a, b)
        w = [((m[:, 0] * rx) + (m[:, 1] * ry)) + m[:, 2] for m in (ma, mb, mc)]
        A = cam[a]
        D = ((A[:, 0] * ma[:, 0]) + (A[:, 1] * ma[:, 1])) + A[:, 2] * ma[:, 2]
        S = (w[0] + w[1]) + w[2]
        t[v, vv, uu] = D / S
        weights[v, vv, uu] = np.stack(w, axis=1) / S[:, None]
    return Barycentric(weights, t, tri)


def mesh_visibility(vertices, triangles, views: Sequence["_lib.View"], width: int, height: int, queries, tol: float, cull: bool = True,
                    keep_maps: bool = False, occluder: bool = True, margin: bool = True, device: int = 0) -> "Visibility":
    """pais_mesh_visibility: the mesh rendered as render_mesh() does, and `queries` (m,3) tested against each view's maps while
    they are on the device.  occluder is the triangle at the query's pixel.  keep_maps: also copy the maps down, as .render."""
    ver, tri = _mesh_arrays("mesh_visibility", vertices, triangles)
    qry = np.ascontiguousarray(queries, dtype=np.float64)
    if qry.ndim != 2 or qry.shape[1] != 3:
        raise ValueError("mesh_visibility: queries is an (m, 3) array, got %s" % (qry.shape,))
    views = list(views)
    nv = len(views)
    arr = (_lib.View * max(nv, 1))(*views)
    code, occ, mar = _vis_outputs(nv, len(qry), occluder, margin)
    depth = np.empty((nv, int(height), int(width)), np.float64) if keep_maps else None
    idm = np.empty((nv, int(height), int(width)), np.int32) if keep_maps else None
    ms = C.c_double(0)
    L = _lib.load()
    rc = L.pais_mesh_visibility(int(device), _lib.RENDER_CULL_BACK if cull else 0, len(ver), _ptr(ver, C.c_double), len(tri), _ptr(tri, C.c_int32),
                                len(qry), _ptr(qry, C.c_double), nv, arr, int(width), int(height), float(tol), _ptr(code, C.c_uint8),
                                _ptr(occ, C.c_int32), _ptr(mar, C.c_double), _ptr(depth, C.c_double), _ptr(idm, C.c_int32), C.byref(ms))
    if rc:
        raise RuntimeError("pais_mesh_visibility failed (%d): %s" % (rc, L.pais_render_last_error().decode()))
    two = (C.c_double * 2)()
    L.pais_cloud_visibility_last_ms(two)
    return Visibility(code, occ, mar, ms.value, Render(depth, idm, two[0], views, last_counts()) if keep_maps else None,
                      {"render": two[0], "test": two[1]})


def render(centers, normals, views: Sequence["_lib.View"], width: int, height: int, mode: str = "disc", radius: float = 1.0,
           radii=None, cull_back: bool = True, device: int = 0) -> Render:
    """pais_cloud_render.  centers (n,3); normals (n,3), may be None in point mode; views: pais_view records (view_of,
    orbit_views); mode "disc": discs of world radius `radius` (or per splat `radii`), "point": squares of `radius` pixels."""
    if mode not in MODES:
        raise ValueError("render: mode %r is not one of %s" % (mode, sorted(MODES)))
    cen = np.ascontiguousarray(centers, dtype=np.float64).reshape(-1, 3)
    nrm = None if normals is None else np.ascontiguousarray(normals, dtype=np.float64).reshape(-1, 3)
    rad = None if radii is None else np.ascontiguousarray(radii, dtype=np.float64).reshape(-1)
    if nrm is not None and len(nrm) != len(cen):
        raise ValueError("render: %d centres and %d normals" % (len(cen), len(nrm)))
    if rad is not None and len(rad) != len(cen):
        raise ValueError("render: %d centres and %d radii" % (len(cen), len(rad)))
    views = list(views)
    nv = len(views)
    arr = (_lib.View * max(nv, 1))(*views)
    depth = np.empty((nv, int(height), int(width)), np.float64)
    idm = np.empty((nv, int(height), int(width)), np.int32)
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    ms = C.c_double(0)
    L = _lib.load()
    rc = L.pais_cloud_render(int(device), MODES[mode], _lib.RENDER_CULL_BACK if cull_back else 0, len(cen), dp(cen), dp(nrm), dp(rad),
                             float(radius), nv, arr, int(width), int(height), dp(depth), idm.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(ms))
    if rc:
        raise RuntimeError("pais_cloud_render failed (%d): %s" % (rc, L.pais_render_last_error().decode()))
    return Render(depth, idm, ms.value, views, last_counts())


VIS_CODES = ("visible", "occluded", "in_front", "empty", "outside", "behind")   # PAIS_VIS_VISIBLE .. PAIS_VIS_BEHIND


class Visibility:
    """The product of depth_test() / visibility(): code (V,n) uint8 (the PAIS_VIS_* codes), occluder (V,n) int32 (the id at
    the point's pixel for codes 0..2, else -1), margin (V,n) float64 (c'2 - depth for codes 0..2, else NaN), kernel_ms, ms
    ({"render", "test"}) and, from visibility(keep_maps=True), the Render of the maps."""

    def __init__(self, code, occluder=None, margin=None, kernel_ms: float = 0.0, render: "Render | None" = None, ms=None):
        self.code = np.asarray(code, np.uint8)
        if self.code.ndim != 2:
            raise ValueError("Visibility: code is a (V, n) array, got %s" % (self.code.shape,))
        if self.code.size and int(self.code.max()) >= len(VIS_CODES):
            raise ValueError("Visibility: code %d is not one of 0 .. %d" % (int(self.code.max()), len(VIS_CODES) - 1))
        self.occluder = None if occluder is None else np.asarray(occluder, np.int32)
        self.margin = None if margin is None else np.asarray(margin, np.float64)
        for a in (self.occluder, self.margin):
            if a is not None and a.shape != self.code.shape:
                raise ValueError("Visibility: occluder and margin have the shape of code, got %s and %s" % (a.shape, self.code.shape))
        self.kernel_ms = float(kernel_ms)
        self.render = render
        self.ms = dict(ms or {})

    def counts(self) -> np.ndarray:
        """(n, 6) int64: per point, how many views gave each of the six codes."""
        return np.stack([(self.code == k).sum(axis=0) for k in range(len(VIS_CODES))], axis=1).astype(np.int64)

    def view_counts(self) -> np.ndarray:
        """(V, 6) int64: per view, how many points fall under each code."""
        return np.stack([(self.code == k).sum(axis=1) for k in range(len(VIS_CODES))], axis=1).astype(np.int64)

    def visible_views(self) -> list:
        """Per point, the views (ascending) that gave PAIS_VIS_VISIBLE."""
        vis = self.code == _lib.VIS_VISIBLE
        return [np.flatnonzero(vis[:, i]).tolist() for i in range(self.code.shape[1])]


def _vis_outputs(nv: int, n: int, occluder: bool, margin: bool):
    code = np.empty((nv, n), np.uint8)
    occ = np.empty((nv, n), np.int32) if occluder else None
    mar = np.empty((nv, n), np.float64) if margin else None
    return code, occ, mar


def _ptr(a, ctype):
    return None if a is None else a.ctypes.data_as(C.POINTER(ctype))


def depth_test(points, views: Sequence["_lib.View"], depth, id=None, tol: float = 0.0, self_index: bool = False, occluder: bool = True,
               margin: bool = True, device: int = 0) -> Visibility:
    """pais_depth_test: points (n,3) against the caller's depth maps (V,H,W) (and id maps, or None) of `views`.  self_index:
    PAIS_VIS_SELF, point i is splat i of the id maps."""
    pts = np.ascontiguousarray(points, dtype=np.float64)
    if pts.ndim != 2 or pts.shape[1] != 3:
        raise ValueError("depth_test: points is an (n, 3) array, got %s" % (pts.shape,))
    views = list(views)
    nv = len(views)
    d = np.ascontiguousarray(depth, dtype=np.float64)
    if d.ndim != 3 or d.shape[0] != nv or d.shape[1] < 1 or d.shape[2] < 1:
        raise ValueError("depth_test: depth is a (V, H, W) array with one map per view, got %s for %d views" % (d.shape, nv))
    idm = None if id is None else np.ascontiguousarray(id, dtype=np.int32)
    if idm is not None and idm.shape != d.shape:
        raise ValueError("depth_test: id has the shape of depth, got %s and %s" % (idm.shape, d.shape))
    if self_index and idm is None:
        raise ValueError("depth_test: self_index needs the id maps")
    arr = (_lib.View * max(nv, 1))(*views)
    code, occ, mar = _vis_outputs(nv, len(pts), occluder, margin)
    ms = C.c_double(0)
    L = _lib.load()
    rc = L.pais_depth_test(int(device), _lib.VIS_SELF if self_index else 0, len(pts), _ptr(pts, C.c_double), nv, arr, d.shape[2], d.shape[1],
                           _ptr(d, C.c_double), _ptr(idm, C.c_int32), float(tol), _ptr(code, C.c_uint8), _ptr(occ, C.c_int32),
                           _ptr(mar, C.c_double), C.byref(ms))
    if rc:
        raise RuntimeError("pais_depth_test failed (%d): %s" % (rc, L.pais_render_last_error().decode()))
    return Visibility(code, occ, mar, ms.value, None, {"render": 0.0, "test": ms.value})


def visibility(centers, normals, views: Sequence["_lib.View"], width: int, height: int, queries=None, mode: str = "disc",
               radius: float = 1.0, radii=None, cull_back: bool = True, tol=None, self_index=None, keep_maps: bool = False,
               occluder: bool = True, margin: bool = True, device: int = 0) -> Visibility:
    """pais_cloud_visibility: the splats rendered as render() does, and `queries` (m,3) -- default: the centres themselves --
    tested against each view's maps while they are on the device.  tol: default `radius` in disc mode (a disc's hit lies
    within its radius of the centre), which needs one radius for all (else give tol).  self_index: PAIS_VIS_SELF, default True
    exactly when the queries are the centres.  keep_maps: also copy the maps down, as .render."""
    if mode not in MODES:
        raise ValueError("visibility: mode %r is not one of %s" % (mode, sorted(MODES)))
    cen = np.ascontiguousarray(centers, dtype=np.float64).reshape(-1, 3)
    nrm = None if normals is None else np.ascontiguousarray(normals, dtype=np.float64).reshape(-1, 3)
    rad = None if radii is None else np.ascontiguousarray(radii, dtype=np.float64).reshape(-1)
    if nrm is not None and len(nrm) != len(cen):
        raise ValueError("visibility: %d centres and %d normals" % (len(cen), len(nrm)))
    if rad is not None and len(rad) != len(cen):
        raise ValueError("visibility: %d centres and %d radii" % (len(cen), len(rad)))
    if self_index is None:
        self_index = queries is None
    if queries is None:
        qry = cen
    else:
        qry = np.ascontiguousarray(queries, dtype=np.float64)
        if qry.ndim != 2 or qry.shape[1] != 3:
            raise ValueError("visibility: queries is an (m, 3) array, got %s" % (qry.shape,))
    if self_index and len(qry) != len(cen):
        raise ValueError("visibility: self_index needs one query per splat, got %d and %d" % (len(qry), len(cen)))
    if tol is None:
        if mode != "disc" or rad is not None:
            raise ValueError("visibility: give tol (the default, the disc radius, needs disc mode and one radius)")
        tol = float(radius)
    views = list(views)
    nv = len(views)
    arr = (_lib.View * max(nv, 1))(*views)
    code, occ, mar = _vis_outputs(nv, len(qry), occluder, margin)
    depth = np.empty((nv, int(height), int(width)), np.float64) if keep_maps else None
    idm = np.empty((nv, int(height), int(width)), np.int32) if keep_maps else None
    ms = C.c_double(0)
    flags = (_lib.RENDER_CULL_BACK if cull_back else 0) | (_lib.VIS_SELF if self_index else 0)
    L = _lib.load()
    rc = L.pais_cloud_visibility(int(device), MODES[mode], flags, len(cen), _ptr(cen, C.c_double), _ptr(nrm, C.c_double), _ptr(rad, C.c_double),
                                 float(radius), len(qry), _ptr(qry, C.c_double), nv, arr, int(width), int(height), float(tol),
                                 _ptr(code, C.c_uint8), _ptr(occ, C.c_int32), _ptr(mar, C.c_double), _ptr(depth, C.c_double),
                                 _ptr(idm, C.c_int32), C.byref(ms))
    if rc:
        raise RuntimeError("pais_cloud_visibility failed (%d): %s" % (rc, L.pais_render_last_error().decode()))
    two = (C.c_double * 2)()
    L.pais_cloud_visibility_last_ms(two)
    return Visibility(code, occ, mar, ms.value, Render(depth, idm, two[0], views, last_counts()) if keep_maps else None,
                      {"render": two[0], "test": two[1]})


def visibility_rule(code, cam_lists, min_visible: int):
    """pais_cloud_visibility_rule: code (V,n); cam_lists: per point the views that list it -> (visible (n,) int32, outlier (n,) bool)."""
    code = np.ascontiguousarray(code, dtype=np.uint8)
    if code.ndim != 2 or code.shape[1] != len(cam_lists):
        raise ValueError("visibility_rule: code is (V, n) with one camera list per point, got %s and %d lists" % (code.shape, len(cam_lists)))
    nv, n = code.shape
    offsets = np.zeros(n + 1, np.int32)
    offsets[1:] = np.cumsum([len(c) for c in cam_lists])
    cams = np.ascontiguousarray([int(c) for lst in cam_lists for c in lst], dtype=np.int32)
    visible, outlier = np.zeros(n, np.int32), np.zeros(n, np.uint8)
    L = _lib.load()
    rc = L.pais_cloud_visibility_rule(n, nv, _ptr(code, C.c_uint8), _ptr(offsets, C.c_int32), _ptr(cams, C.c_int32) if len(cams) else None,
                                      int(min_visible), _ptr(visible, C.c_int32), _ptr(outlier, C.c_uint8))
    if rc:
        raise RuntimeError("pais_cloud_visibility_rule failed (%d): %s" % (rc, L.pais_render_last_error().decode()))
    return visible, outlier.astype(bool)


def composite(a: Render, b: Render):
    """Two renders of the same views composited by depth -> (from_b (V,H,W) bool, depth): b wins where it is strictly nearer."""
    from_b = b.depth < a.depth
    return from_b, np.where(from_b, b.depth, a.depth)
