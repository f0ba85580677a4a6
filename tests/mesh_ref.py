"""Helpers of tests/test_mesh_cpu.py and tests/test_mesh_gpu.py: the host shim of pais_mesh.hpp (tests/mesh_host_shim.cpp), the case
generators, and the statements of include/pais_mesh.h restated with Python floats -- IEEE doubles, one rounding per operation,
every loop strictly from left to right -- the field over a knn_ref.brute_knn table, the orientation table from `fractions`, the
surface and the weld."""
import ctypes as C
import math
import os
import subprocess
from fractions import Fraction

import numpy as np

from tests import knn_ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAN = float("nan")
TETS = ((0, 1, 3, 7), (0, 1, 5, 7), (0, 2, 3, 7), (0, 2, 6, 7), (0, 4, 5, 7), (0, 4, 6, 7))

FIELD_GRIDS = ((2, 2, 2), (5, 4, 3), (9, 8, 7))
FIELD_CLOUDS = (1, 7, 300)
FIELD_KS = (1, 8, 9, 32)


class CGrid(C.Structure):
    _fields_ = [("origin", C.c_double * 3), ("h", C.c_double), ("n", C.c_int32 * 3), ("reserved", C.c_int32)]


class Grid:
    """origin (3), h, n (3): the plain values of a pais_grid"""

    def __init__(self, origin, h, n):
        self.origin, self.h, self.n = [float(v) for v in origin], float(h), [int(v) for v in n]

    def c(self):
        return CGrid((C.c_double * 3)(*self.origin), self.h, (C.c_int32 * 3)(*self.n), 0)

    def num_vertices(self):
        return self.n[0] * self.n[1] * self.n[2]

    def coord(self, axis, i):
        return self.origin[axis] + (float(i) * self.h)

    def positions(self):
        """(nv, 3) by the vertex statement, index g = (k ny + j) nx + i"""
        nx, ny, nz = self.n
        x = np.array([self.coord(0, i) for i in range(nx)])
        y = np.array([self.coord(1, j) for j in range(ny)])
        z = np.array([self.coord(2, k) for k in range(nz)])
        out = np.empty((nz, ny, nx, 3))
        out[..., 0], out[..., 1], out[..., 2] = x[None, None, :], y[None, :, None], z[:, None, None]
        return out.reshape(-1, 3)


# --------------------------------------------------------------------------------------------------------- the shim ---
_shim = None


def _compile(out, extra):
    src = os.path.join(HERE, "mesh_host_shim.cpp")
    csrc = os.path.join(ROOT, "pais_mvs_amd", "csrc")
    deps = [src, os.path.join(csrc, "pais_mesh.hpp"), os.path.join(csrc, "pais_dev.hpp"), os.path.join(ROOT, "include", "pais_mesh.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off"] + extra + ["-o", out, src])
    return out


def shim():
    global _shim
    if _shim is None:
        S = C.CDLL(_compile(os.path.join(HERE, "build", "libmesh_host_shim.so"), ["-fPIC", "-shared"]))
        dp, ip, lp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        S.shim_sizeof_grid.restype = C.c_size_t
        assert S.shim_sizeof_grid() == C.sizeof(CGrid) == 48
        S.shim_field.restype = None
        S.shim_field.argtypes = [C.POINTER(CGrid), C.c_int, ip, dp, C.c_int, dp, dp, C.c_double, C.c_double, dp]
        S.shim_surface.restype = C.c_int64
        S.shim_surface.argtypes = [C.POINTER(CGrid), dp, C.c_int64, lp, dp]
        _shim = S
    return _shim


def sanitized_program():
    """The shim with its own main, built with -fsanitize=address,undefined: a stand-alone program."""
    return _compile(os.path.join(HERE, "build", "mesh_shim_asan"),
                    ["-g", "-DMESH_SHIM_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def shim_field(grid, index, dist2, centers, normals, support, trunc):
    index, dist2 = np.ascontiguousarray(index, np.int32), np.ascontiguousarray(dist2, np.float64)
    centers, normals = np.ascontiguousarray(centers, np.float64), np.ascontiguousarray(normals, np.float64)
    out = np.empty(grid.num_vertices())
    g = grid.c()
    shim().shim_field(C.byref(g), index.shape[1], index.ctypes.data_as(C.POINTER(C.c_int32)), _dp(dist2), len(centers), _dp(centers),
                      _dp(normals), float(support), float(trunc), _dp(out))
    return out


def shim_surface(grid, field, max_triangles=None):
    """-> (count, keys (m,3) int64, xyz (m,3,3)); max_triangles None: a counting call, then one with the exact capacity"""
    field = np.ascontiguousarray(field, np.float64)
    g = grid.c()
    count = int(shim().shim_surface(C.byref(g), _dp(field), 0, None, None))
    cap = count if max_triangles is None else int(max_triangles)
    keys, xyz = np.full((cap, 3), -7, np.int64), np.full((cap, 3, 3), -7.0)
    if cap:
        assert shim().shim_surface(C.byref(g), _dp(field), cap, keys.ctypes.data_as(C.POINTER(C.c_int64)), _dp(xyz)) == count
    return count, keys, xyz


# ------------------------------------------------------------------------------------------------------ restatement ---
def ref_field(grid, index, dist2, centers, normals, support, trunc):
    """pais_cloud_field over a knn_ref.brute_knn table of the grid's vertices, statement by statement"""
    pos = grid.positions().tolist()
    cen, nrm = np.asarray(centers, np.float64).tolist(), np.asarray(normals, np.float64).tolist()
    nt = len(cen)
    t2, r2 = trunc * trunc, support * support
    out = []
    for g, (px, py, pz) in enumerate(pos):
        row, d2row = index[g].tolist(), dist2[g].tolist()
        if d2row[0] > t2:
            out.append(NAN)
            continue
        num, den = 0.0, 0.0
        for s, d2 in zip(row, d2row):
            if s < 0 or s >= nt or not d2 < r2:
                continue
            u = 1.0 - (d2 / r2)
            w = u * u
            dx, dy, dz = px - cen[s][0], py - cen[s][1], pz - cen[s][2]
            sd = ((nrm[s][0] * dx) + (nrm[s][1] * dy)) + (nrm[s][2] * dz)
            num += w * sd
            den += w
        out.append(num / den)
    return np.array(out, np.float64)


def _corner(b):
    return (b & 1, (b >> 1) & 1, (b >> 2) & 1)


def case_edges(mask):
    """the triangles of a tetrahedron whose listed vertices `mask` marks inside, before orientation: a list of triangles, each three
    edges (p, q) of listed positions as the case table names them (a-b: a first)"""
    inside = [j for j in range(4) if (mask >> j) & 1]
    outside = [j for j in range(4) if not (mask >> j) & 1]
    if len(inside) == 1:
        a, (b, c, d) = inside[0], outside
        return [[(a, b), (a, c), (a, d)]]
    if len(inside) == 3:
        a, (b, c, d) = outside[0], inside
        return [[(a, b), (a, c), (a, d)]]
    if len(inside) == 2:
        (a, b), (c, d) = inside, outside
        q = [(a, c), (a, d), (b, d), (b, c)]
        return [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    return []


def derive_flip_table():
    """6 x 16 booleans from exact arithmetic: corner values -1 inside and +1 outside, crossings at the midpoints.  The level set of
    the linear interpolant is a plane whose normal is the interpolant's gradient g (solved exactly); a triangle is swapped when
    (B-A)x(C-A) . g < 0."""
    F = Fraction
    table = []
    for tet in TETS:
        row = [False] * 16
        P = [[F(v) for v in _corner(b)] for b in tet]
        for mask in range(1, 15):
            val = [F(-1) if (mask >> j) & 1 else F(1) for j in range(4)]
            # gradient: (P_j - P_0) . g = val_j - val_0, j = 1 .. 3, by Cramer's rule
            M = [[P[j][a] - P[0][a] for a in range(3)] for j in (1, 2, 3)]
            r = [val[j] - val[0] for j in (1, 2, 3)]
            det = lambda m: (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0])
                             + m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]))
            D = det(M)
            g = [det([[r[i] if a == c else M[i][c] for c in range(3)] for i in range(3)]) / D for a in range(3)]
            signs = set()
            for tri in case_edges(mask):
                A, B, Cc = ([(P[p][a] + P[q][a]) / 2 for a in range(3)] for p, q in tri)
                u, v = [B[a] - A[a] for a in range(3)], [Cc[a] - A[a] for a in range(3)]
                n = [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]
                s = sum(n[a] * g[a] for a in range(3))
                assert s != 0
                signs.add(s < 0)
            assert len(signs) == 1, (tet, mask)
            row[mask] = signs.pop()
        table.append(row)
    return table


_FLIP = None


def ref_surface(grid, field):
    """pais_field_surface, statement by statement -> (keys (m,3) int64, xyz (m,3,3))"""
    global _FLIP
    if _FLIP is None:
        _FLIP = derive_flip_table()
    nx, ny, nz = grid.n
    f = np.asarray(field, np.float64).tolist()
    keys, xyz = [], []
    for k in range(nz - 1):
        for j in range(ny - 1):
            for i in range(nx - 1):
                idx = [((k + dz) * ny + (j + dy)) * nx + (i + dx) for dx, dy, dz in map(_corner, range(8))]
                val = [f[g] for g in idx]
                if any(v != v for v in val):
                    continue

                def crossing(ca, cb):
                    if idx[ca] > idx[cb]:
                        ca, cb = cb, ca
                    code = cb - ca
                    assert 1 <= code <= 7 and (ca & cb) == ca
                    fa, fb = val[ca], val[cb]
                    t = fa / (fa - fb)
                    P = []
                    for axis, base in enumerate((i, j, k)):
                        pa = grid.coord(axis, base + _corner(ca)[axis])
                        pb = grid.coord(axis, base + _corner(cb)[axis])
                        P.append(pa + (t * (pb - pa)))
                    return idx[ca] * 8 + code, P

                for t, tet in enumerate(TETS):
                    mask = sum(1 << jj for jj in range(4) if val[tet[jj]] < 0)
                    for tri in case_edges(mask):
                        if _FLIP[t][mask]:
                            tri = [tri[0], tri[2], tri[1]]
                        got = [crossing(tet[p], tet[q]) for p, q in tri]
                        keys.append([kk for kk, _ in got])
                        xyz.append([P for _, P in got])
    return np.array(keys, np.int64).reshape(-1, 3), np.array(xyz, np.float64).reshape(-1, 3, 3)


def ref_weld(keys, xyz):
    """pais_mesh_weld with a dictionary -> (vertices (n,3), triangles (m,3) int32)"""
    first = {}
    for c, key in enumerate(np.asarray(keys).reshape(-1).tolist()):
        first.setdefault(key, c)
    order = sorted(first)
    where = {key: v for v, key in enumerate(order)}
    flat = np.asarray(xyz, np.float64).reshape(-1, 3)
    vertices = np.array([flat[first[key]] for key in order], np.float64).reshape(-1, 3)
    triangles = np.array([where[key] for key in np.asarray(keys).reshape(-1).tolist()], np.int32).reshape(-1, 3)
    return vertices, triangles


# ------------------------------------------------------------------------------------------------------------ cases ---
def field_case(n, nt, k):
    """a grid over about [-1.2, 1.2] in x (h from n[0]) and nt random points on the unit sphere with their outward normals
    -> (grid, centers, normals, support, trunc)"""
    rng = np.random.default_rng(100 * n[0] + 10 * nt + k)
    h = 2.4 / (n[0] - 1)
    grid = Grid(-1.2 + 0.01 * rng.normal(size=3), h, n)
    c = rng.normal(size=(nt, 3))
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    return grid, c, c.copy(), 3.0 * h, 2.0 * h


def field_table(grid, centers, k):
    return knn_ref.brute_knn(grid.positions(), centers, k)


def fibonacci_sphere(n):
    """n points on the unit sphere (the golden-angle spiral) and their exact normals"""
    i = np.arange(n) + 0.5
    z = 1.0 - 2.0 * i / n
    r = np.sqrt(1.0 - z * z)
    phi = i * (math.pi * (3.0 - math.sqrt(5.0)))
    p = np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)
    return p, p.copy()


def analytic_grid(n, span=1.2):
    """n vertices per axis, centred on a small irrational-looking offset from 0, the pitch such that the shortest axis covers
    [-span, span] (the longer ones cover more)"""
    h = 2.0 * span / (min(n) - 1)
    off = (0.0123456789 * math.sqrt(2.0), -0.0087654321 * math.sqrt(3.0), 0.0054321 * math.sqrt(5.0))
    return Grid([o - h * (m - 1) / 2.0 for o, m in zip(off, n)], h, n)


def sphere_field(grid, radius=1.0):
    p = grid.positions()
    return np.sqrt((p * p).sum(axis=1)) - radius


def torus_field(grid, R=1.0, r=0.4):
    p = grid.positions()
    return np.sqrt((np.sqrt(p[:, 0] ** 2 + p[:, 1] ** 2) - R) ** 2 + p[:, 2] ** 2) - r


def plane_case():
    """z - 2 on a 6^3 unit grid: exact zeros at the vertices of layer 2"""
    grid = Grid([0.0, 0.0, 0.0], 1.0, (6, 6, 6))
    return grid, grid.positions()[:, 2] - 2.0


def sampled_sphere(trunc_h=2.0):
    """800 Fibonacci points with exact normals on a 17^3 grid, k = 8, support 3h -> (grid, centers, normals, k, support, trunc)"""
    grid = analytic_grid((17, 17, 17))
    c, n = fibonacci_sphere(800)
    return grid, c, n, 8, 3.0 * grid.h, trunc_h * grid.h


def surface_cases():
    """name -> (grid, field): what test_mesh_cpu.py runs through the shim and test_mesh_gpu.py through the kernels"""
    out = {}
    for n in ((9, 9, 9), (17, 13, 11)):
        g = analytic_grid(n)
        out["sphere %dx%dx%d" % n] = (g, sphere_field(g))
    g = analytic_grid((21, 21, 21), span=1.6)
    out["torus"] = (g, torus_field(g))
    out["plane"] = plane_case()
    g = analytic_grid((9, 9, 9))
    f = sphere_field(g)
    for name, fill in (("all positive", 1.5), ("all negative", -1.5), ("all nan", NAN)):
        out[name] = (g, np.full_like(f, fill))
    band = f.copy().reshape(9, 9, 9)
    band[:, 4, :] = NAN
    out["nan band"] = (g, band.reshape(-1))
    return out


# ------------------------------------------------------------------------------------------------------- topology ---
def directed_edges(triangles):
    """{(a, b): occurrences} over the directed edges of the non-degenerate triangles (a triangle with two equal indices has no area
    and bounds nothing)"""
    count = {}
    for a, b, c in np.asarray(triangles).tolist():
        if a == b or b == c or a == c:
            continue
        for e in ((a, b), (b, c), (c, a)):
            count[e] = count.get(e, 0) + 1
    return count


def is_closed(triangles):
    """every directed edge occurs once and its reverse once"""
    e = directed_edges(triangles)
    return bool(e) and all(n == 1 and e.get((b, a), 0) == 1 for (a, b), n in e.items())


def euler(num_vertices, triangles):
    t = [r for r in np.asarray(triangles).tolist() if len(set(r)) == 3]
    used = {v for r in t for v in r}
    edges = {(min(a, b), max(a, b)) for r in t for a, b in ((r[0], r[1]), (r[1], r[2]), (r[2], r[0]))}
    return len(used) - len(edges) + len(t)


def volume(vertices, triangles):
    v = np.asarray(vertices, np.float64)
    t = np.asarray(triangles)
    return float(np.einsum("ij,ij->i", v[t[:, 0]], np.cross(v[t[:, 1]], v[t[:, 2]])).sum() / 6.0)
