"""Mesh a cloud: the surface of an oriented point cloud as a triangle mesh, on the GPU (include/pais_mesh.h).

    field      the weighted tangent-plane distance of every vertex of a regular grid from the cloud (pais_cloud_field, over the
               k-nearest search of pais_cloud_knn), NaN beyond `trunc` of the nearest point
    surface    the marching-tetrahedra iso-surface of a field at level 0 as a triangle soup with an edge key per corner
               (pais_field_surface)
    weld       the soup as an indexed mesh: one vertex per distinct key (pais_mesh_weld, host)

Field and surface are HIP kernels and there is no CPU fallback.  The mesh is a pure function of the cloud and the grid.

    python -m pais_mvs_amd.mesh cloud.{mvs,ply,npy} [--h H] [--k K] [--support S] [--trunc T] --out mesh.{ply,obj}
"""
from __future__ import annotations

import ctypes as C
import math
import sys

import numpy as np

from . import _lib


class Grid:
    """A regular grid (pais_grid): n = (nx, ny, nz) vertices per axis, vertex (i,j,k) at origin + (i,j,k) h with index
    (k ny + j) nx + i."""

    def __init__(self, origin, h: float, n):
        self.origin = [float(v) for v in origin]
        self.h = float(h)
        self.n = [int(v) for v in n]
        if len(self.origin) != 3 or len(self.n) != 3:
            raise ValueError("Grid: origin and n have three components, got %r and %r" % (origin, n))

    def c(self) -> "_lib.Grid":
        return _lib.Grid((C.c_double * 3)(*self.origin), self.h, (C.c_int32 * 3)(*self.n), 0)

    def num_vertices(self) -> int:
        return self.n[0] * self.n[1] * self.n[2]

    def num_cells(self) -> int:
        return (self.n[0] - 1) * (self.n[1] - 1) * (self.n[2] - 1)

    def __repr__(self):
        return "Grid(origin=%r, h=%r, n=%r)" % (self.origin, self.h, self.n)


def _as_grid(grid) -> Grid:
    return grid if isinstance(grid, Grid) else Grid(grid.origin, grid.h, grid.n)


def _fail(what: str, rc: int):
    raise RuntimeError("%s failed (%d): %s" % (what, rc, _lib.load().pais_mesh_last_error().decode()))


def grid_for(points, h: float, margin: float) -> Grid:
    """The grid of pitch h that covers the bounding box of points (n,3) widened by margin on every side."""
    p = np.asarray(points, np.float64)
    if p.ndim != 2 or p.shape[1] < 3 or not len(p):
        raise ValueError("grid_for: an (n, 3) array of at least one point, got %s" % (p.shape,))
    if not (math.isfinite(h) and h > 0 and math.isfinite(margin) and margin >= 0):
        raise ValueError("grid_for: h = %r must be positive and margin = %r non-negative" % (h, margin))
    lo, hi = p[:, :3].min(axis=0) - margin, p[:, :3].max(axis=0) + margin
    n = [max(int(math.ceil((b - a) / h)) + 1, 2) for a, b in zip(lo.tolist(), hi.tolist())]
    if n[0] * n[1] * n[2] > _lib.MESH_MAX_VERTICES:
        raise ValueError("grid_for: %d x %d x %d vertices exceed the cap of 2^28; use a larger h" % tuple(n))
    return Grid(lo.tolist(), h, n)


def field(cloud, grid, k: int = 8, support=None, trunc=None, device: int = 0) -> np.ndarray:
    """pais_cloud_field: cloud (n,6) points and normals -> the field at every grid vertex, float64 (nz, ny, nx), NaN where the
    nearest point is farther than trunc (default 2 h); support (default 3 h) is the radius of the weight (1 - d2 / support^2)^2."""
    grid = _as_grid(grid)
    c = np.ascontiguousarray(np.asarray(cloud, np.float64))
    if c.ndim != 2 or c.shape[1] != 6:
        raise ValueError("field: an (n, 6) array of points and normals is needed, got %s" % (c.shape,))
    support = 3.0 * grid.h if support is None else float(support)
    trunc = 2.0 * grid.h if trunc is None else float(trunc)
    cen, nrm = np.ascontiguousarray(c[:, :3]), np.ascontiguousarray(c[:, 3:])
    out = np.empty(max(grid.num_vertices(), 1), np.float64)
    g, ms = grid.c(), C.c_double(0)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    rc = _lib.load().pais_cloud_field(int(device), int(k), C.byref(g), len(c), dp(cen), dp(nrm), support, trunc, dp(out), C.byref(ms))
    if rc:
        _fail("pais_cloud_field", rc)
    return out[:grid.num_vertices()].reshape(grid.n[2], grid.n[1], grid.n[0])


def last_ms() -> dict:
    """Kernel milliseconds of this thread's last field() and surface() calls."""
    ms = (C.c_double * 4)()
    _lib.load().pais_mesh_last_ms(ms)
    return {"search": ms[0], "field": ms[1], "count": ms[2], "emit": ms[3]}


def surface_count(values, grid, layers: int = 0, device: int = 0) -> int:
    """The triangle count of surface(): the counting pass of pais_field_surface alone."""
    grid = _as_grid(grid)
    f = _field_of(values, grid)
    g, n = grid.c(), C.c_int64(0)
    rc = _lib.load().pais_field_surface(int(device), C.byref(g), f.ctypes.data_as(C.POINTER(C.c_double)), int(layers), 0, C.byref(n), None, None, None)
    if rc:
        _fail("pais_field_surface", rc)
    return int(n.value)


def _field_of(values, grid: Grid) -> np.ndarray:
    f = np.ascontiguousarray(np.asarray(values, np.float64)).reshape(-1)
    if len(f) != grid.num_vertices():
        raise ValueError("surface: the field has %d values, the grid %d vertices" % (len(f), grid.num_vertices()))
    return f


def surface(values, grid, layers: int = 0, device: int = 0, max_triangles=None):
    """pais_field_surface: the iso-surface of a field (any shape of nx ny nz values in grid order) at level 0 -> (keys int64 (m,3),
    xyz float64 (m,3,3)): per triangle the edge key and the position of each corner.  A counting call, then a call with the exact
    capacity; max_triangles: one call with that capacity instead -> (count, keys, xyz) with min(count, max_triangles) rows."""
    grid = _as_grid(grid)
    f = _field_of(values, grid)
    g, n = grid.c(), C.c_int64(0)
    L = _lib.load()
    fp = f.ctypes.data_as(C.POINTER(C.c_double))
    cap = surface_count(f, grid, layers, device) if max_triangles is None else int(max_triangles)
    keys, xyz = np.empty((max(cap, 0), 3), np.int64), np.empty((max(cap, 0), 3, 3), np.float64)
    if cap or max_triangles is not None:
        rc = L.pais_field_surface(int(device), C.byref(g), fp, int(layers), cap, C.byref(n), keys.ctypes.data_as(C.POINTER(C.c_int64)),
                                  xyz.ctypes.data_as(C.POINTER(C.c_double)), None)
        if rc:
            _fail("pais_field_surface", rc)
    if max_triangles is None:
        return keys, xyz
    m = min(int(n.value), cap)
    return int(n.value), keys[:m], xyz[:m]


def weld(keys, xyz):
    """pais_mesh_weld: the soup of surface() -> (vertices float64 (n,3), triangles int32 (m,3), vertex keys int64 (n,)): one vertex
    per distinct key in ascending key order, at the position of the key's first occurrence."""
    keys = np.ascontiguousarray(np.asarray(keys, np.int64)).reshape(-1, 3)
    xyz = np.ascontiguousarray(np.asarray(xyz, np.float64)).reshape(-1, 3, 3)
    if len(keys) != len(xyz):
        raise ValueError("weld: %d triangles of keys, %d of positions" % (len(keys), len(xyz)))
    L = _lib.load()
    m, n = len(keys), C.c_int64(0)
    kp, xp = keys.ctypes.data_as(C.POINTER(C.c_int64)), xyz.ctypes.data_as(C.POINTER(C.c_double))
    rc = L.pais_mesh_weld(m, kp, xp, C.byref(n), 0, None, None)
    if rc:
        _fail("pais_mesh_weld", rc)
    vertices, triangles = np.empty((n.value, 3), np.float64), np.empty((m, 3), np.int32)
    if n.value:
        rc = L.pais_mesh_weld(m, kp, xp, C.byref(n), n.value, vertices.ctypes.data_as(C.POINTER(C.c_double)),
                              triangles.ctypes.data_as(C.POINTER(C.c_int32)))
        if rc:
            _fail("pais_mesh_weld", rc)
    return vertices, triangles, np.unique(keys)


class Mesh:
    """vertices float64 (n,3), triangles int32 (m,3), keys int64 (n,): the edge key of every vertex, field: the (nz,ny,nx) field the
    surface was taken from (or None), grid: its Grid (or None).  Triangles of zero area (two equal indices, or three points in
    a line where the field is exactly 0 at a grid vertex) are kept; the topology methods count the triangles with three
    distinct indices."""

    def __init__(self, vertices, triangles, keys=None, field=None, grid=None):
        self.vertices = np.asarray(vertices, np.float64).reshape(-1, 3)
        self.triangles = np.asarray(triangles, np.int32).reshape(-1, 3)
        self.keys = None if keys is None else np.asarray(keys, np.int64)
        self.field, self.grid = field, grid

    def _solid(self) -> np.ndarray:
        t = self.triangles
        return t[(t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])]

    def _corners(self):
        v, t = self.vertices, self.triangles
        return v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]

    def area(self) -> float:
        a, b, c = self._corners()
        return float(np.sqrt((np.cross(b - a, c - a) ** 2).sum(axis=1)).sum() / 2.0)

    def volume(self) -> float:
        """sum(A . (B x C)) / 6: positive for a closed surface whose normals point outward"""
        a, b, c = self._corners()
        return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)

    def _directed(self):
        t = self._solid().astype(np.int64)
        e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
        return e[:, 0] * (len(self.vertices) + 1) + e[:, 1], e

    def boundary_edges(self) -> np.ndarray:
        """(b,2) the directed edges whose reverse does not occur exactly as often: empty for a closed surface"""
        code, e = self._directed()
        rev = e[:, 1] * (len(self.vertices) + 1) + e[:, 0]
        u, n = np.unique(code, return_counts=True)
        ur, nr = np.unique(rev, return_counts=True)
        have = dict(zip(ur.tolist(), nr.tolist()))
        keep = np.array([have.get(c, 0) != k for c, k in zip(u.tolist(), n.tolist())], bool)
        first = {c: i for i, c in reversed(list(enumerate(code.tolist())))}
        return e[[first[c] for c in u[keep].tolist()]].reshape(-1, 2)

    def is_closed(self) -> bool:
        """every directed edge occurs once and its reverse once (and there is a triangle at all)"""
        code, e = self._directed()
        if not len(code):
            return False
        rev = e[:, 1] * (len(self.vertices) + 1) + e[:, 0]
        return bool(len(np.unique(code)) == len(code) and np.array_equal(np.sort(code), np.sort(rev)))

    def euler(self) -> int:
        """V - E + F over the triangles with three distinct indices and the vertices they use"""
        t = self._solid().astype(np.int64)
        e = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), axis=1)
        edges = len(np.unique(e[:, 0] * (len(self.vertices) + 1) + e[:, 1]))
        return int(len(np.unique(t)) - edges + len(t))

    def colors(self, cloud_bgr, centers, device: int = 0) -> np.ndarray:
        """(n,3) uint8: every vertex takes the colour of its nearest cloud point (evaluate.nearest on the GPU)"""
        from . import evaluate
        bgr = np.asarray(cloud_bgr, np.uint8).reshape(-1, 3)
        cen = np.asarray(centers, np.float64).reshape(-1, 3)
        if len(bgr) != len(cen):
            raise ValueError("colors: %d colours for %d centres" % (len(bgr), len(cen)))
        if not len(self.vertices):
            return np.zeros((0, 3), np.uint8)
        return bgr[evaluate.nearest(self.vertices, cen, device)[0]]

    def render(self, views, width: int, height: int, cull: bool = True, device: int = 0):
        """render.render_mesh of this mesh: per view a depth map and a triangle-id map (pais_mesh_render)"""
        from . import render as rnd
        return rnd.render_mesh(self.vertices, self.triangles, views, width, height, cull, device)

    def depth_maps(self, cameras, cull: bool = True, device: int = 0) -> list:
        """per camera (camera.Camera with images, or anything with width / height) its (H,W) depth map of the mesh; cameras of
        one size share a render"""
        from . import render as rnd
        sizes = [_camera_size(cam) for cam in cameras]
        out = [None] * len(sizes)
        for wh in sorted(set(sizes)):
            idx = [k for k, s in enumerate(sizes) if s == wh]
            r = self.render([rnd.view_of(cameras[k]) for k in idx], wh[0], wh[1], cull, device)
            for j, k in enumerate(idx):
                out[k] = r.depth[j]
        return out

    def _tol(self, tol):
        if tol is not None:
            return float(tol)
        if self.grid is None:
            raise ValueError("visibility: give tol (the default, half the grid pitch, needs a mesh with its grid)")
        return 0.5 * _as_grid(self.grid).h

    def visibility(self, views, width: int, height: int, points=None, tol=None, cull: bool = True, keep_maps: bool = False, device: int = 0):
        """render.mesh_visibility: `points` (default: the mesh's own vertices) tested against the mesh's depth maps in the views
        (pais_mesh_visibility).  tol: default half the pitch of the mesh's grid -- the surface lies within one cell."""
        from . import render as rnd
        pts = self.vertices if points is None else points
        return rnd.mesh_visibility(self.vertices, self.triangles, views, width, height, pts, self._tol(tol), cull, keep_maps, device=device)

    def colors_from_images(self, cameras, images, tol=None, fallback=None, cloud_bgr=None, centers=None, device: int = 0) -> np.ndarray:
        """(n,3) uint8: every vertex takes the mean BGR (rounded half to even) of its cvRound pixel over the cameras that see it
        -- code VISIBLE of visibility() against the mesh itself.  images: per camera an (H,W,3) uint8 BGR array (or (H,W) grey).
        A vertex no camera sees takes `fallback` ((3,) or (n,3)); default: colors(cloud_bgr, centers) when a cloud is given, else
        black."""
        from . import render as rnd
        if len(cameras) != len(images):
            raise ValueError("colors_from_images: %d cameras and %d images" % (len(cameras), len(images)))
        n = len(self.vertices)
        total, seen = np.zeros((n, 3), np.float64), np.zeros(n, np.int64)
        sizes = [(int(np.asarray(im).shape[1]), int(np.asarray(im).shape[0])) for im in images]
        for wh in sorted(set(sizes)):
            idx = [k for k, s in enumerate(sizes) if s == wh]
            views = [rnd.view_of(cameras[k]) for k in idx]
            vis = self.visibility(views, wh[0], wh[1], None, tol, device=device)
            for j, k in enumerate(idx):
                img = np.asarray(images[k], np.uint8)
                if img.ndim == 2:
                    img = np.repeat(img[:, :, None], 3, axis=2)
                sel = np.flatnonzero(vis.code[j] == _lib.VIS_VISIBLE)
                pu, pv = _project_round(views[j], self.vertices[sel])
                total[sel] += img[pv, pu]
                seen[sel] += 1
        if fallback is None:
            fallback = self.colors(cloud_bgr, centers, device) if cloud_bgr is not None and centers is not None else (0, 0, 0)
        out = np.empty((n, 3), np.uint8)
        out[...] = np.asarray(fallback, np.uint8)
        got = seen > 0
        out[got] = np.rint(total[got] / seen[got, None]).astype(np.uint8)
        return out

    def write_ply(self, path: str, bgr=None) -> None:
        """ASCII PLY: vertices (with red green blue when bgr (n,3) is given), faces as `vertex_indices` lists"""
        col = None if bgr is None else np.asarray(bgr, np.uint8).reshape(-1, 3)
        if col is not None and len(col) != len(self.vertices):
            raise ValueError("write_ply: %d colours for %d vertices" % (len(col), len(self.vertices)))
        with open(path, "w") as f:
            f.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty double x\nproperty double y\nproperty double z\n" % len(self.vertices))
            if col is not None:
                f.write("property uchar red\nproperty uchar green\nproperty uchar blue\n")
            f.write("element face %d\nproperty list uchar int vertex_indices\nend_header\n" % len(self.triangles))
            for i, v in enumerate(self.vertices.tolist()):
                f.write("%r %r %r" % tuple(v))
                if col is not None:
                    f.write(" %d %d %d" % (col[i, 2], col[i, 1], col[i, 0]))
                f.write("\n")
            for t in self.triangles.tolist():
                f.write("3 %d %d %d\n" % tuple(t))

    def write_obj(self, path: str) -> None:
        with open(path, "w") as f:
            for v in self.vertices.tolist():
                f.write("v %r %r %r\n" % tuple(v))
            for t in self.triangles.tolist():
                f.write("f %d %d %d\n" % (t[0] + 1, t[1] + 1, t[2] + 1))


def _camera_size(cam):
    w, h = getattr(cam, "width", None), getattr(cam, "height", None)
    if w is None or h is None:
        img = cam.image if hasattr(cam, "image") else cam.pyramid[0]
        h, w = np.asarray(img).shape[:2]
    return int(w), int(h)


def _project_round(view, points):
    """the pixel pais_depth_test reads for points the view sees: cvRound(f (c'k / c'2) + pp) by the statements of pais_render.h"""
    R, T = list(view.R[:]), list(view.T[:])
    p = np.asarray(points, np.float64).reshape(-1, 3)
    c = [((R[3 * k] * p[:, 0] + R[3 * k + 1] * p[:, 1]) + R[3 * k + 2] * p[:, 2]) + T[k] for k in range(3)]
    pu = view.focal[0] * (c[0] / c[2]) + view.pp[0]
    pv = view.focal[1] * (c[1] / c[2]) + view.pp[1]
    return np.rint(pu).astype(np.int64), np.rint(pv).astype(np.int64)


def read_ply(path: str):
    """A file written by Mesh.write_ply -> (Mesh, bgr (n,3) uint8 or None); the vertices come back bit for bit (%r round-trips)"""
    with open(path) as f:
        nv = nf = None
        colored = False
        if f.readline().strip() != "ply":
            raise IOError("%s: not a PLY file" % path)
        for line in f:
            w = line.split()
            if w[:2] == ["element", "vertex"]:
                nv = int(w[2])
            elif w[:2] == ["element", "face"]:
                nf = int(w[2])
            elif w[:1] == ["format"] and w[1:2] != ["ascii"]:
                raise IOError("%s: only the ASCII PLY of Mesh.write_ply is read" % path)
            elif w[:3] == ["property", "uchar", "red"]:
                colored = True
            elif w[:1] == ["end_header"]:
                break
        rows = [l.split() for l in f.read().split("\n") if l]
    if nv is None or nf is None or len(rows) != nv + nf:
        raise IOError("%s: %d rows after a header of %r vertices and %r faces" % (path, len(rows), nv, nf))
    ver = np.array([[float(x) for x in r[:3]] for r in rows[:nv]], np.float64).reshape(-1, 3)
    bgr = np.array([[int(r[5]), int(r[4]), int(r[3])] for r in rows[:nv]], np.uint8).reshape(-1, 3) if colored else None
    if any(r[0] != "3" or len(r) != 4 for r in rows[nv:]):
        raise IOError("%s: a face that is not a triangle" % path)
    tri = np.array([[int(x) for x in r[1:]] for r in rows[nv:]], np.int32).reshape(-1, 3)
    return Mesh(ver, tri), bgr


def read_obj(path: str) -> "Mesh":
    """A file written by Mesh.write_obj -> Mesh"""
    ver, tri = [], []
    with open(path) as f:
        for line in f:
            w = line.split()
            if w[:1] == ["v"]:
                ver.append([float(x) for x in w[1:4]])
            elif w[:1] == ["f"]:
                if len(w) != 4:
                    raise IOError("%s: a face that is not a triangle" % path)
                tri.append([int(x.split("/")[0]) - 1 for x in w[1:]])
    return Mesh(np.array(ver, np.float64).reshape(-1, 3), np.array(tri, np.int32).reshape(-1, 3))


def read_mesh(path: str):
    """read_ply / read_obj by the file's ending -> (Mesh, bgr or None)"""
    if path.lower().endswith(".obj"):
        return read_obj(path), None
    if path.lower().endswith(".ply"):
        return read_ply(path)
    raise ValueError("%s: a mesh file ends in .ply or .obj" % path)


def read_counts(path: str):
    """(vertices, faces) of a file written by Mesh.write_ply or Mesh.write_obj"""
    with open(path) as f:
        if path.lower().endswith(".obj"):
            lines = f.read().split("\n")
            return sum(l.startswith("v ") for l in lines), sum(l.startswith("f ") for l in lines)
        nv = nf = None
        for line in f:
            w = line.split()
            if w[:2] == ["element", "vertex"]:
                nv = int(w[2])
            elif w[:2] == ["element", "face"]:
                nf = int(w[2])
            elif w[:1] == ["end_header"]:
                break
        rows = [l for l in f.read().split("\n") if l]
        if nv is None or nf is None or len(rows) != nv + nf:
            raise IOError("%s: %d rows after a header of %r vertices and %r faces" % (path, len(rows), nv, nf))
        return nv, nf


def mesh_of_field(values, grid, layers: int = 0, device: int = 0) -> Mesh:
    """surface() and weld() of a field"""
    grid = _as_grid(grid)
    keys, xyz = surface(values, grid, layers, device)
    vertices, triangles, vkeys = weld(keys, xyz)
    return Mesh(vertices, triangles, vkeys, np.asarray(values, np.float64).reshape(grid.n[2], grid.n[1], grid.n[0]), grid)


def mesh(cloud, h=None, k: int = 8, support=None, trunc=None, device: int = 0) -> Mesh:
    """The surface of a cloud (n,6) of points and normals.  h: the grid pitch, default twice the cloud's sample spacing
    (evaluate.spacing); support default 3 h, trunc default 2 h.  trunc has to exceed the cell diagonal sqrt(3) h, or cells that
    straddle the surface lose a corner to NaN and the mesh gets holes.  The grid covers the cloud's box widened by trunc + h."""
    from . import evaluate
    c = np.ascontiguousarray(np.asarray(cloud, np.float64))
    if c.ndim != 2 or c.shape[1] != 6 or not len(c):
        raise ValueError("mesh: an (n, 6) array of at least one point with its normal is needed, got %s" % (c.shape,))
    if h is None:
        h = 2.0 * evaluate.spacing(c[:, :3], device)
    h = float(h)
    support = 3.0 * h if support is None else float(support)
    trunc = 2.0 * h if trunc is None else float(trunc)
    grid = grid_for(c[:, :3], h, trunc + h)
    return mesh_of_field(field(c, grid, k, support, trunc, device), grid, 0, device)


def main(argv=None) -> int:
    import argparse
    import json
    from . import evaluate
    ap = argparse.ArgumentParser(prog="python -m pais_mvs_amd.mesh", description=__doc__.split("\n\n")[0])
    ap.add_argument("cloud", help="cloud.mvs, cloud.ply or cloud.npy ((n,6)): points with normals")
    ap.add_argument("--h", type=float, default=None, help="grid pitch (default: twice the cloud's sample spacing)")
    ap.add_argument("--k", type=int, default=8, help="neighbours per grid vertex")
    ap.add_argument("--support", type=float, default=None, help="radius of the weight (default 3 h)")
    ap.add_argument("--trunc", type=float, default=None, help="no surface farther than this from the nearest point (default 2 h)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", required=True, help="mesh.ply or mesh.obj")
    a = ap.parse_args(argv)
    ext = a.out.lower().rsplit(".", 1)[-1]
    if ext not in ("ply", "obj"):
        ap.error("--out ends in .ply or .obj")
    if a.h is not None and not a.h > 0:
        ap.error("--h is positive")
    if not 1 <= a.k <= _lib.CLOUD_MAX_K:
        ap.error("--k lies in [1, %d]" % _lib.CLOUD_MAX_K)
    for name in ("support", "trunc"):
        if getattr(a, name) is not None and not getattr(a, name) > 0:
            ap.error("--%s is positive" % name)
    if a.support is not None and a.trunc is not None and not a.support > a.trunc:
        ap.error("--support exceeds --trunc")
    m = mesh(evaluate.load_cloud(a.cloud), a.h, a.k, a.support, a.trunc, a.device)
    m.write_ply(a.out) if ext == "ply" else m.write_obj(a.out)
    print(json.dumps({"vertices": int(len(m.vertices)), "triangles": int(len(m.triangles)), "closed": m.is_closed(), "area": m.area(),
                      "grid": m.grid.n, "h": m.grid.h, "out": a.out}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
