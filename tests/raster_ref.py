"""pais_mesh_render restated: the TRIANGLE statements of include/pais_render.h, brute force over every pixel and every
triangle, with no box and no skip that the header does not name.

pixel() is the restatement with Python floats, one pixel of one triangle at a time.  render() evaluates the same statements for
all pixels of a triangle at once with numpy float64 arrays: elementwise IEEE double operations in the header's order, no
fused operation, so both give the same bits (test_mesh_render_cpu.py holds render() to pixel() on a small case); it is what
makes 5000 triangles x 3 views affordable.  shim() is pais_raster.hpp compiled for the host (tests/raster_host_shim.cpp)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

from pais_mvs_amd import _lib
from pais_mvs_amd import render as rnd

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CULL = _lib.RENDER_CULL_BACK
LIVE, BEHIND, REPEATED, CULLED, FLAT, OFF_IMAGE = range(6)          # pais::RASTER_* (pais_raster.hpp)


# ------------------------------------------------------------------------------------------------- the restatement ---
def camera(view, P):
    R, T = view.R, view.T
    return [((R[3 * k] * P[0] + R[3 * k + 1] * P[1]) + R[3 * k + 2] * P[2]) + T[k] for k in range(3)]


def edge(p, q, P, Q):
    lo, hi = (P, Q) if p < q else (Q, P)
    n = [lo[1] * hi[2] - lo[2] * hi[1], lo[2] * hi[0] - lo[0] * hi[2], lo[0] * hi[1] - lo[1] * hi[0]]
    return n if p < q else [-x for x in n]


def setup(view, vertices, tri):
    """-> (Ma, Mb, Mc, D, (A'2, B'2, C'2)) with Python floats"""
    a, b, c = (int(k) for k in tri)
    A, B, Cc = (camera(view, [float(x) for x in vertices[k]]) for k in (a, b, c))
    ma, mb, mc = edge(b, c, B, Cc), edge(c, a, Cc, A), edge(a, b, A, B)
    D = ((A[0] * ma[0]) + (A[1] * ma[1])) + A[2] * ma[2]
    return ma, mb, mc, D, (A[2], B[2], Cc[2])


def skipped(flags, tri, zs, D):
    a, b, c = (int(k) for k in tri)
    if not (zs[0] > 0.0 or zs[1] > 0.0 or zs[2] > 0.0):
        return True
    if a == b or b == c or a == c:
        return True
    return bool((flags & CULL) and D >= 0.0)


def _div(x, y):
    try:
        return x / y
    except ZeroDivisionError:                                       # IEEE: x / +-0
        if x == 0.0 or x != x:
            return float("nan")
        return math.copysign(float("inf"), x) * math.copysign(1.0, y)


def pixel(view, ma, mb, mc, D, u, v):
    """(covered, t) of pixel (u, v): Python floats, the header's statements in the header's order"""
    rx, ry = (float(u) - view.pp[0]) / view.focal[0], (float(v) - view.pp[1]) / view.focal[1]
    wa = ((ma[0] * rx) + (ma[1] * ry)) + ma[2]
    wb = ((mb[0] * rx) + (mb[1] * ry)) + mb[2]
    wc = ((mc[0] * rx) + (mc[1] * ry)) + mc[2]
    S = (wa + wb) + wc
    t = _div(D, S)
    inside = (wa >= 0.0 and wb >= 0.0 and wc >= 0.0) or (wa <= 0.0 and wb <= 0.0 and wc <= 0.0)
    return bool(inside and math.isfinite(t) and t > 0.0), t


def render_floats(vertices, triangles, views, W, H, flags=0):
    """render() one pixel at a time with Python floats (small cases only)"""
    depth, idm = np.full((len(views), H, W), np.inf), np.full((len(views), H, W), -1, np.int32)
    for vi, view in enumerate(views):
        for s, tri in enumerate(np.asarray(triangles).tolist()):
            ma, mb, mc, D, zs = setup(view, vertices, tri)
            if skipped(flags, tri, zs, D):
                continue
            for v in range(H):
                for u in range(W):
                    hit, t = pixel(view, ma, mb, mc, D, u, v)
                    if hit and t < depth[vi, v, u]:
                        depth[vi, v, u], idm[vi, v, u] = t, s
    return depth, idm


def render(vertices, triangles, views, W, H, flags=0):
    """-> (depth (V,H,W) float64, id (V,H,W) int32, covered (pixel, triangle) pairs)"""
    vertices = np.asarray(vertices, np.float64)
    depth, idm = np.full((len(views), H, W), np.inf), np.full((len(views), H, W), -1, np.int32)
    covered = 0
    with np.errstate(all="ignore"):
        for vi, view in enumerate(views):
            rx = ((np.arange(W, dtype=np.float64) - view.pp[0]) / view.focal[0])[None, :]
            ry = ((np.arange(H, dtype=np.float64) - view.pp[1]) / view.focal[1])[:, None]
            dm, im = depth[vi], idm[vi]
            for s, tri in enumerate(np.asarray(triangles).tolist()):
                ma, mb, mc, D, zs = setup(view, vertices, tri)
                if skipped(flags, tri, zs, D):
                    continue
                wa = ((ma[0] * rx) + (ma[1] * ry)) + ma[2]
                wb = ((mb[0] * rx) + (mb[1] * ry)) + mb[2]
                wc = ((mc[0] * rx) + (mc[1] * ry)) + mc[2]
                t = D / ((wa + wb) + wc)
                hit = (((wa >= 0.0) & (wb >= 0.0) & (wc >= 0.0)) | ((wa <= 0.0) & (wb <= 0.0) & (wc <= 0.0))) & np.isfinite(t) & (t > 0.0)
                covered += int(hit.sum())
                win = hit & (t < dm)                                 # ascending s: the lowest index among equal depths stays
                dm[win] = t[win]
                im[win] = s
    return depth, idm, covered


def same_maps(got_depth, got_id, want_depth, want_id):
    got_depth, want_depth = np.asarray(got_depth, np.float64), np.asarray(want_depth, np.float64)
    return bool(got_depth.shape == want_depth.shape and np.array_equal(got_depth.view(np.uint64), want_depth.view(np.uint64))
                and np.array_equal(got_id, want_id))


# --------------------------------------------------------------------------------------------------------- the shim ---
_shim = None


def _compile(out, extra):
    src = os.path.join(HERE, "raster_host_shim.cpp")
    csrc = os.path.join(ROOT, "pais_mvs_amd", "csrc")
    deps = [src, os.path.join(csrc, "pais_raster.hpp"), os.path.join(csrc, "pais_dev.hpp"), os.path.join(ROOT, "include", "pais_render.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off"] + extra + ["-o", out, src])
    return out


def shim():
    global _shim
    if _shim is None:
        S = C.CDLL(_compile(os.path.join(HERE, "build", "libraster_host_shim.so"), ["-fPIC", "-shared"]))
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        S.shim_mesh_render.restype = C.c_longlong
        S.shim_mesh_render.argtypes = [C.c_int, C.c_int, dp, C.c_int, ip, C.c_int, C.POINTER(_lib.View), C.c_int, C.c_int, C.c_int, dp, ip, ip]
        _shim = S
    return _shim


def sanitized_program():
    """The shim with its own main, built with -fsanitize=address,undefined: a stand-alone program."""
    return _compile(os.path.join(HERE, "build", "raster_shim_asan"),
                    ["-g", "-DRASTER_SHIM_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def shim_render(vertices, triangles, views, W, H, flags=0, use_box=True):
    """-> (depth, id, covered pairs, skip codes (V, nt))"""
    ver = np.ascontiguousarray(vertices, np.float64)
    tri = np.ascontiguousarray(triangles, np.int32).reshape(-1, 3)
    nv = len(views)
    arr = (_lib.View * max(nv, 1))(*views)
    depth, idm = np.empty((nv, H, W)), np.empty((nv, H, W), np.int32)
    skips = np.empty((nv, len(tri)), np.int32)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    n = shim().shim_mesh_render(flags, len(ver), ver.ctypes.data_as(C.POINTER(C.c_double)), len(tri), ip(tri), nv, arr, W, H, int(use_box),
                                depth.ctypes.data_as(C.POINTER(C.c_double)), ip(idm), ip(skips))
    return depth, idm, int(n), skips


# ------------------------------------------------------------------------------------------------------------ cases ---
SOUP_SIZES = ((37, 29), (65, 48))
SOUP_NT = (1, 7, 300, 5000)
SOUP_VIEWS = (1, 3)


def soup_views(V, W, H, seed=0):
    """V views around the origin at distance 3 +- 0.3, focal 0.9 W"""
    rng = np.random.default_rng(1000 + seed)
    out = []
    for k in range(V):
        d = np.array([math.cos(2.1 * k + 0.3), 0.35 * math.sin(1.3 * k), math.sin(2.1 * k + 0.3)])
        C_ = (3.0 + 0.3 * rng.uniform(-1, 1)) * d / np.linalg.norm(d)
        out.append(rnd.look_at_view(C_, rng.uniform(-0.1, 0.1, 3), (0.0, 1.0, 0.0), 0.9 * W, W, H))
    return out


def soup(nt, seed=0):
    """A welded soup of nt triangles -> (vertices, triangles int32): a jittered g x g sheet z = bump(x, y) over [-1.2, 1.2]^2
    whose cells give pairs of small triangles that share an edge and its two vertices; every ninth triangle instead joins three
    vertices from anywhere (large, and with either winding); every 23rd has a repeated index; every 31st uses a vertex pushed far
    along a view direction, so that it passes through or behind the camera plane of the first view."""
    rng = np.random.default_rng(seed)
    g = max(3, int(math.ceil(math.sqrt(nt / 2.0))) + 1)
    x, y = np.meshgrid(np.linspace(-1.2, 1.2, g), np.linspace(-1.2, 1.2, g), indexing="xy")
    pts = np.stack([x.ravel(), y.ravel(), 0.3 * np.sin(2.0 * x.ravel()) * np.cos(1.5 * y.ravel())], axis=1)
    pts += rng.uniform(-0.3, 0.3, pts.shape) * (2.4 / (g - 1)) * np.array([1.0, 1.0, 0.5])
    far = np.array([[4.0, 0.5, 1.5], [2.9, 0.0, 0.9], [-5.0, 1.0, -3.0]])      # around and beyond the first cameras
    ver = np.concatenate([pts, far])
    tri = np.empty((nt, 3), np.int32)
    cells = rng.permutation((g - 1) * (g - 1))
    for s in range(nt):
        cell = int(cells[(s // 2) % len(cells)])
        i, j = cell % (g - 1), cell // (g - 1)
        v00, v10, v01, v11 = j * g + i, j * g + i + 1, (j + 1) * g + i, (j + 1) * g + i + 1
        t = [v00, v10, v11] if s % 2 == 0 else [v00, v11, v01]
        if s % 9 == 4:
            t = rng.choice(len(pts), 3, replace=False).tolist()
        if s % 23 == 7:
            t[2] = t[0]
        if s % 31 == 11:
            t[1] = len(pts) + int(rng.integers(0, len(far)))
        if rng.uniform() < 0.25:
            t = [t[0], t[2], t[1]]
        tri[s] = t
    return ver, tri


def dyadic_view(W=65, H=48, f=32.0):
    """identity rotation, the camera at the origin looking along +z, f and pp powers of two: pixel (u, v) is the ray
    ((u - 32) / 32, (v - 16) / 32, 1), so a vertex (x, y, 1) with x, y multiples of 1/32 sits exactly on a pixel centre"""
    return rnd.make_view(np.eye(3), (0.0, 0.0, 0.0), (f, f), (32.0, 16.0))


def at_pixel(u, v, z=1.0, f=32.0):
    """the point at depth z on the ray of pixel (u, v) of dyadic_view (exact for dyadic z)"""
    return [(u - 32.0) / f * z, (v - 16.0) / f * z, z]


def octahedron(r=1.0):
    v = np.array([[r, 0, 0], [-r, 0, 0], [0, r, 0], [0, -r, 0], [0, 0, r], [0, 0, -r]], np.float64)
    t = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32)   # outward
    return v, t


def ray_sphere(view, W, H, radius):
    """per pixel the analytic camera-z of the first hit of its ray with the sphere |X| = radius around the world origin (NaN
    where it misses) and the cosine of the incidence angle there -> ((H,W), (H,W))"""
    R, T = np.array(view.R[:]).reshape(3, 3), np.array(view.T[:])
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    r = np.stack([(u - view.pp[0]) / view.focal[0], (v - view.pp[1]) / view.focal[1], np.ones_like(u)], axis=-1)
    # camera space: the sphere's centre is T; |t r - T|^2 = radius^2
    a, b, c = (r * r).sum(-1), (r @ T), float(T @ T) - radius * radius
    disc = b * b - a * c
    with np.errstate(invalid="ignore"):
        t = (b - np.sqrt(disc)) / a
        t = np.where((disc >= 0) & (t > 0), t, np.nan)
        n = (t[..., None] * r - T) / radius
        cos = -(n * r).sum(-1) / np.sqrt(a)
    return t, cos


# ---------------------------------------------------------------------------------------------- dyadic edge cases ---
def edge_cases():
    """name -> (vertices, triangles, flags, expectation) in dyadic_view (65 x 48): coordinates on pixel centres, so edges and
    vertices pass exactly through them.  expectation(depth (H,W), id (H,W)) asserts what the case is about; every case is
    compared with render() bit for bit as well."""
    P = at_pixel
    out = {}

    def shared_edge(d, i):
        k = np.arange(10, 31)
        assert (i[k, k] == 0).all(), i[k, k]                       # every pixel centre on the shared diagonal: the lower index
        assert (i[10:31, 10:31] >= 0).all() and (d[10:31, 10:31] == 1.0).all()
        assert (i >= 0).sum() == 21 * 21 and set(np.unique(i[10:31, 10:31]).tolist()) == {0, 1}
    sq = [P(10, 10), P(30, 10), P(30, 30), P(10, 30)]
    out["shared edge"] = (sq, [[0, 1, 2], [0, 2, 3]], 0, shared_edge)
    out["shared edge, other windings"] = (sq, [[2, 1, 0], [0, 2, 3]], 0, shared_edge)

    def coincident(d, i):
        assert (i >= 0).sum() == 21 * 22 // 2 and set(np.unique(i).tolist()) == {-1, 0}
    out["coincident"] = (sq, [[0, 1, 2], [0, 1, 2], [1, 2, 0]], 0, coincident)

    def through_plane(d, i):
        assert (i >= 0).sum() > 0 and (d[i >= 0] > 0).all() and np.isinf(d[i < 0]).all()
        assert (i[20, 21:40] == 0).all()                           # the edge in front of the camera is drawn ...
        assert (i >= 0).sum() < 65 * 48                            # ... and the part behind it is not mirrored over the image
    out["through the camera plane"] = ([P(20, 20), P(40, 20), [0.0, 0.5, -1.0]], [[0, 1, 2]], 0, through_plane)

    def nothing(d, i):
        assert (i == -1).all() and np.isinf(d).all()
    out["behind"] = ([[0.0, 0.0, -1.0], [0.5, 0.0, -2.0], [0.0, 0.5, -1.0], [0.0, 0.0, 0.0]], [[0, 1, 2], [0, 3, 1]], 0, nothing)
    a, b = np.array(P(20, 20)), np.array(P(40, 30, 2.0))
    out["D == 0"] = ([a.tolist(), b.tolist(), (a + b).tolist()], [[0, 1, 2]], 0, nothing)
    out["repeated indices"] = (sq, [[0, 1, 1], [2, 2, 2], [3, 0, 3]], 0, nothing)
    out["off the image"] = ([P(100, 10), P(120, 10), P(110, 20)], [[0, 1, 2], [0, 2, 1]], 0, nothing)

    def one_side(d, i):
        assert (i >= 0).sum() == 21 * 22 // 2 and len(np.unique(i[i >= 0])) == 1
    def both_sides(d, i):
        assert (i >= 0).sum() == 21 * 21 and set(np.unique(i).tolist()) == {-1, 0, 1}
    out["back face kept"] = (sq, [[0, 1, 2], [0, 3, 2]], 0, both_sides)
    out["back face culled"] = (sq, [[0, 1, 2], [0, 3, 2]], CULL, one_side)

    def whole_image(d, i):
        assert (i == 0).all() and (d == 1.0).all()
    out["larger than the image"] = ([P(-200, -100), P(400, -100), P(32, 500)], [[0, 1, 2]], 0, whole_image)
    return out


def check_edge_cases(render_fn):
    """render_fn(vertices, triangles, views, W, H, flags) -> (depth (V,H,W), id (V,H,W))"""
    view = dyadic_view()
    for name, (ver, tri, flags, expect) in edge_cases().items():
        ver, tri = np.array(ver, np.float64), np.array(tri, np.int32)
        d, i = render_fn(ver, tri, [view], 65, 48, flags)
        wd, wi, _ = render(ver, tri, [view], 65, 48, flags)
        assert same_maps(d, i, wd, wi), name
        try:
            expect(d[0], i[0])
        except AssertionError as e:
            raise AssertionError("%s: %s" % (name, e))


# ------------------------------------------------------------------------------------------------- closed meshes ---
SPHERE_R = 1.0
HOLE_W, HOLE_H = 96, 80


def sphere_chord_error(h, R=SPHERE_R):
    """e such that the marching-tetrahedra mesh of |p| - R on a grid of pitch h lies in the shell R - e <= |p| <= R.
    A vertex is the zero of the field's linear interpolant on an edge of a tetrahedron of the cell, of length L <= sqrt(3) h.
    |p| is convex with second derivative <= 1 / |p| along a line, so the interpolant lies above the field by at most
    L^2 / 8 / (R - L): a vertex has R - ev <= |p| <= R with ev = 3 h^2 / (8 (R - sqrt(3) h)).  A point of a triangle is
    q = sum l_i v_i with |q|^2 = sum l_i |v_i|^2 - sum_{i<j} l_i l_j |v_i - v_j|^2 >= (R - ev)^2 - d^2 / 3, the triangle's
    diameter d <= sqrt(3) h and sum_{i<j} l_i l_j <= 1/3; and |q| <= R by convexity of the ball.  So e = R - sqrt((R - ev)^2 - h^2)."""
    ev = 3.0 * h * h / (8.0 * (R - math.sqrt(3.0) * h))
    return R - math.sqrt((R - ev) ** 2 - h * h)


_sphere = None


def sphere_mesh():
    """(vertices, triangles, h): the marching-tetrahedra sphere of |p| - 1 at 17^3 (mesh_ref's case), surface by the mesher's
    host shim, welded by pais_mesh_weld"""
    global _sphere
    if _sphere is None:
        from pais_mvs_amd import mesh as msh
        from tests import mesh_ref as mr
        grid = mr.analytic_grid((17, 17, 17))
        count, keys, xyz = mr.shim_surface(grid, mr.sphere_field(grid, SPHERE_R))
        v, t, _ = msh.weld(keys, xyz)
        _sphere = (v, t, grid.h)
    return _sphere


def hole_views():
    """three 96 x 80 views from outside, at distance 3, zoomed until the silhouette leaves the frame at the top and bottom: the
    share of grazing rays (cos < 0.5) among those that hit stays under a quarter (for a whole silhouette it is a quarter or more)"""
    return [rnd.look_at_view(3.0 * np.array(d) / np.linalg.norm(d), (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), 150.0, HOLE_W, HOLE_H)
            for d in ((1.0, 0.2, 0.3), (-0.5, 1.0, -0.4), (0.1, -0.3, 1.0))]


def check_closed_sphere(depth, idm, views, inner, outer, e):
    """every pixel whose ray hits the sphere `inner` is covered; where cos(incidence on `inner`) >= 0.5 the depth lies within
    e / cos of the analytic depth on `outer` (module docstring of the tests) -> the share of excluded grazing pixels per view"""
    shares = []
    for v, view in enumerate(views):
        t_in, cos_in = ray_sphere(view, HOLE_W, HOLE_H, inner)
        t_out, _ = ray_sphere(view, HOLE_W, HOLE_H, outer)
        hit = np.isfinite(t_in)
        assert hit.sum() > 0.5 * HOLE_W * HOLE_H
        holes = hit & (idm[v] < 0)
        assert not holes.any(), ("view %d: %d holes, first at (v, u) = %s" % (v, holes.sum(), np.argwhere(holes)[0]))
        ok = hit & (cos_in >= 0.5)
        err = np.abs(depth[v][ok] - t_out[ok])
        bound = e / cos_in[ok] + 1e-12
        print("view %d: %d hit, grazing share %.3f, worst depth error / bound %.3f" % (v, hit.sum(), 1.0 - ok.sum() / hit.sum(), (err / bound).max()))
        assert (err <= bound).all(), ("view %d: depth off by %g at bound %g" % (v, err.max(), bound[np.argmax(err - bound)]))
        shares.append(1.0 - ok.sum() / hit.sum())
    assert max(shares) < 0.25, shares
    return shares
