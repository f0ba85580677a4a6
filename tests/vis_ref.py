"""The statements of pais_depth_test / pais_cloud_visibility (include/pais_render.h) restated in numpy -- every product, sum and
quotient its own rounded elementwise pass, sums left to right -- the rule of pais_cloud_visibility_rule as plain loops, the host
build of pais_vis.hpp (tests/vis_host_shim.cpp), and the cases the CPU and the GPU tests share.  The renderer's restatement is
_brute of tests/test_render_gpu.py."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
VISIBLE, OCCLUDED, IN_FRONT, EMPTY, OUTSIDE, BEHIND = range(6)
SELF = 0x100
QNAN = np.array([0x7FF8000000000000], np.uint64).view(np.float64)[0]


# ------------------------------------------------------------------------------------------------------ restatement ---
def ref_depth_test(points, views, depth, idm, tol, self_index=False):
    """points (n,3); views: pais_view records; depth (V,H,W); idm (V,H,W) int32 or None.
    -> code (V,n) uint8, occluder (V,n) int32, margin (V,n) float64 (one fixed quiet NaN where the code is 3..5)."""
    c = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    views = list(views)
    n, V = len(c), len(views)
    depth = np.asarray(depth, np.float64)
    code = np.zeros((V, n), np.uint8)
    occ = np.full((V, n), -1, np.int32)
    margin = np.full((V, n), QNAN)
    me = np.arange(n, dtype=np.int32)
    for v, view in enumerate(views):
        R, T, f, pp = np.array(view.R[:]), np.array(view.T[:]), np.array(view.focal[:]), np.array(view.pp[:])
        H, W = depth[v].shape
        with np.errstate(all="ignore"):
            x = ((R[0] * c[:, 0] + R[1] * c[:, 1]) + R[2] * c[:, 2]) + T[0]
            y = ((R[3] * c[:, 0] + R[4] * c[:, 1]) + R[5] * c[:, 2]) + T[1]
            z = ((R[6] * c[:, 0] + R[7] * c[:, 1]) + R[8] * c[:, 2]) + T[2]
            behind = ~(z > 0)
            pu = f[0] * (x / z)
            pv = f[1] * (y / z)
            pu = pu + pp[0]
            pv = pv + pp[1]
            fin = np.isfinite(pu) & np.isfinite(pv) & (np.abs(pu) < 2.0 ** 30) & (np.abs(pv) < 2.0 ** 30)
            ok = ~behind & fin
            ru = np.rint(np.where(ok, pu, 0.0)).astype(np.int64)             # cvRound: half to even
            rv = np.rint(np.where(ok, pv, 0.0)).astype(np.int64)
            inside = ok & (ru >= 0) & (ru < W) & (rv >= 0) & (rv < H)
            ru, rv = np.where(inside, ru, 0), np.where(inside, rv, 0)
            d = depth[v][rv, ru]
            at = idm[v][rv, ru].astype(np.int32) if idm is not None else np.full(n, -1, np.int32)
            empty = inside & (d == np.inf)
            tested = inside & ~empty
            m = z - d
            own = tested & (at == me) if self_index else np.zeros(n, bool)
            k = np.where(m > tol, OCCLUDED, np.where(m < -tol, IN_FRONT, VISIBLE))
            k = np.where(own, VISIBLE, k)
        code[v] = np.where(behind, BEHIND, np.where(~inside, OUTSIDE, np.where(empty, EMPTY, k)))
        occ[v] = np.where(tested, at, -1)
        margin[v] = np.where(tested, m, QNAN)
    return code, occ, margin


def rule_loop(code, cam_lists, min_visible):
    """pais_cloud_visibility_rule as plain loops -> (visible list, outlier list)"""
    visible, outlier = [], []
    for i, cams in enumerate(cam_lists):
        v = len(cams)
        for cam in cams:
            if int(code[cam][i]) == OCCLUDED:
                v -= 1
        visible.append(v)
        outlier.append(v < min_visible)
    return visible, outlier


def normalised(margin):
    """margin as uint64 with every NaN written as the one fixed quiet NaN"""
    m = np.array(margin, np.float64, copy=True)
    m[np.isnan(m)] = QNAN
    return m.view(np.uint64)


def assert_same(got, want, what):
    """got: a render.Visibility or a (code, occluder, margin) triple; want: the triple of ref_depth_test"""
    g = (got.code, got.occluder, got.margin) if hasattr(got, "code") else got
    assert g[0].dtype == np.uint8 and g[0].shape == want[0].shape, what
    bad = np.argwhere(g[0] != want[0])
    assert not len(bad), (what, "code", len(bad), bad[:5].tolist(), g[0][tuple(bad[:5].T)], want[0][tuple(bad[:5].T)])
    if g[1] is not None:
        bad = np.argwhere(g[1] != want[1])
        assert g[1].dtype == np.int32 and not len(bad), (what, "occluder", len(bad), bad[:5].tolist())
    if g[2] is not None:
        bad = np.argwhere(normalised(g[2]) != normalised(want[2]))
        assert g[2].dtype == np.float64 and not len(bad), (what, "margin", len(bad), bad[:5].tolist(), g[2][tuple(bad[:5].T)], want[2][tuple(bad[:5].T)])


def brute_tiled(flags, centers, normals, rho, views, W, H, tile=32):
    """_brute (DISC mode, one radius) of tests/test_render_gpu.py, tile by tile, for clouds of thousands of splats at full image
    size, where _brute's n x H x W passes take a quarter of a minute.  A tile of the image is itself a view: the same pose with
    the principal point moved by the tile's origin -- (u - x0) - (pp - x0) is u - pp exactly while all three are integers, which
    is asserted -- so each tile's pixels go through _brute's own statements unchanged.  Per tile only the splats that can reach
    it are handed over, in ascending index (the tie rule keeps its meaning) and their ids mapped back: a covered hit lies within
    rho of c', so it projects within f rho / (c'2 - rho) pixels of the centre's projection; twice that plus two pixels is
    kept, and every splat with c'2 <= 2 rho goes to every tile.  tests/test_visibility_gpu.py checks one cloud against the
    untiled _brute."""
    from pais_mvs_amd.render import make_view
    from tests.test_render_gpu import DISC, _brute
    cen = np.ascontiguousarray(centers, np.float64).reshape(-1, 3)
    nrm = np.ascontiguousarray(normals, np.float64).reshape(-1, 3)
    rho = float(rho)
    depth = np.full((len(views), H, W), np.inf)
    idm = np.full((len(views), H, W), -1, np.int32)
    for v, view in enumerate(views):
        R, T, f, pp = np.array(view.R[:]).reshape(3, 3), np.array(view.T[:]), np.array(view.focal[:]), np.array(view.pp[:])
        assert pp[0] == np.floor(pp[0]) and pp[1] == np.floor(pp[1]) and abs(pp[0]) < 2 ** 30 and abs(pp[1]) < 2 ** 30
        cc = cen @ R.T + T
        every = ~(cc[:, 2] > 2.0 * rho)
        z = np.where(every, 1.0, cc[:, 2])
        pu, pv = f[0] * cc[:, 0] / z + pp[0], f[1] * cc[:, 1] / z + pp[1]
        reach = 2.0 * max(abs(f[0]), abs(f[1])) * rho / (z - rho) + 2.0
        for y0 in range(0, H, tile):
            for x0 in range(0, W, tile):
                tw, th = min(tile, W - x0), min(tile, H - y0)
                keep = np.flatnonzero(every | ((pu + reach >= x0) & (pu - reach <= x0 + tw - 1) & (pv + reach >= y0) & (pv - reach <= y0 + th - 1)))
                if not len(keep):
                    continue
                sub = make_view(R, T, f, (pp[0] - x0, pp[1] - y0))
                d, i = _brute(DISC, flags, cen[keep], nrm[keep], rho, [sub], tw, th)
                depth[v, y0:y0 + th, x0:x0 + tw] = d[0]
                idm[v, y0:y0 + th, x0:x0 + tw] = np.where(i[0] >= 0, keep[np.maximum(i[0], 0)], -1)
    return depth, idm


# --------------------------------------------------------------------------------------------------------- the shim ---
_shim = None


def _compile(out, extra):
    src = os.path.join(HERE, "vis_host_shim.cpp")
    csrc = os.path.join(ROOT, "pais_mvs_amd", "csrc")
    deps = [src, os.path.join(csrc, "pais_vis.hpp"), os.path.join(csrc, "pais_dev.hpp"), os.path.join(ROOT, "include", "pais_render.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off"] + extra + ["-o", out, src])
    return out


def shim():
    global _shim
    if _shim is None:
        from pais_mvs_amd import _lib
        S = C.CDLL(_compile(os.path.join(HERE, "build", "libvis_host_shim.so"), ["-fPIC", "-shared"]))
        S.shim_depth_test.restype = None
        S.shim_depth_test.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_double), C.c_int, C.POINTER(_lib.View), C.c_int, C.c_int,
                                      C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_double, C.POINTER(C.c_uint8), C.POINTER(C.c_int32),
                                      C.POINTER(C.c_double)]
        _shim = S
    return _shim


def sanitized_program():
    """The shim with its own main, built with -fsanitize=address,undefined: a stand-alone program."""
    return _compile(os.path.join(HERE, "build", "vis_shim_asan"), ["-g", "-DVIS_SHIM_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def shim_depth_test(points, views, depth, idm, tol, self_index=False):
    """pais_vis.hpp on the host over all (view, point) pairs -> the triple of ref_depth_test"""
    from pais_mvs_amd import _lib
    pts = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    views = list(views)
    d = np.ascontiguousarray(depth, np.float64)
    i = None if idm is None else np.ascontiguousarray(idm, np.int32)
    V, H, W = d.shape
    n = len(pts)
    code, occ, mar = np.zeros((V, n), np.uint8), np.zeros((V, n), np.int32), np.zeros((V, n), np.float64)
    arr = (_lib.View * max(V, 1))(*views)
    shim().shim_depth_test(SELF if self_index else 0, n, pts.ctypes.data_as(C.POINTER(C.c_double)), V, arr, W, H,
                           d.ctypes.data_as(C.POINTER(C.c_double)), None if i is None else i.ctypes.data_as(C.POINTER(C.c_int32)), float(tol),
                           code.ctypes.data_as(C.POINTER(C.c_uint8)), occ.ctypes.data_as(C.POINTER(C.c_int32)), mar.ctypes.data_as(C.POINTER(C.c_double)))
    return code, occ, mar


# ------------------------------------------------------------------------------------------------------------ cases ---
EDGE_W, EDGE_H, EDGE_F = 65, 48, 64.0


def edge_case():
    """One front view (identity pose, focal 64, pp (32, 24)) over hand-made maps, and points whose projections and margins are
    exact (dyadic coordinates, focal and depths powers of two).  -> (view, depth (1,H,W), id (1,H,W), points, tol, names, and
    the expected code per point without and with PAIS_VIS_SELF)."""
    from pais_mvs_amd.render import make_view
    W, H, F = EDGE_W, EDGE_H, EDGE_F
    view = make_view(np.eye(3), np.zeros(3), (F, F), (float(W >> 1), float(H >> 1)))
    at = lambda u, v, z: [(u - (W >> 1)) / F * z, (v - (H >> 1)) / F * z, z]
    depth = np.full((1, H, W), 4.0)
    idm = np.full((1, H, W), 1000, np.int32)
    depth[0, 5, 7], idm[0, 5, 7] = np.inf, -1                     # an empty pixel
    idm[0, 30, 40] = 13                                           # the pixel of point 13 shows splat 13
    tol = 0.25
    rows = [
        ("pu = 10.5 (even below: rounds to 10)", at(10.5, 7, 4.0), VISIBLE),
        ("pu = 11.5 (odd below: rounds to 12)", at(11.5, 7, 4.0), VISIBLE),
        ("pv = 8.5 rounds to 8", at(20, 8.5, 4.0), VISIBLE),
        ("pu = -0.5 rounds to 0: inside", at(-0.5, 7, 4.0), VISIBLE),
        ("pu = W - 0.5 = 64.5 rounds to 64 (even): inside", at(W - 0.5, 7, 4.0), VISIBLE),
        ("pu = W + 0.5 = 65.5 rounds to 66: outside", at(W + 0.5, 7, 4.0), OUTSIDE),
        ("pu = -1.5 rounds to -2: outside", at(-1.5, 7, 4.0), OUTSIDE),
        ("pv = H - 0.5 rounds to H: outside", at(20, H - 0.5, 4.0), OUTSIDE),
        ("c'2 = 0", [0.5, 0.25, 0.0], BEHIND),
        ("c'2 < 0", [0.5, 0.25, -2.0], BEHIND),
        ("|pu| = 2^30", [(2.0 ** 30 - 32.0) / F * 4.0, 0.0, 4.0], OUTSIDE),
        ("|pu| just below 2^30, outside the image", [(2.0 ** 30 - 33.0) / F * 4.0, 0.0, 4.0], OUTSIDE),
        ("a pixel holding +inf", at(7, 5, 4.0), EMPTY),
        ("m == tol", at(20, 20, 4.25), VISIBLE),
        ("m == -tol", at(21, 20, 3.75), VISIBLE),
        ("m == 0", at(22, 20, 4.0), VISIBLE),
        ("m just above tol", at(23, 20, 4.25 + 2.0 ** -50), OCCLUDED),
        ("m just below -tol", at(24, 20, 3.75 - 2.0 ** -50), IN_FRONT),
        ("behind the surface, on the pixel that shows id 13, but not point 13", at(40, 30, 8.0), OCCLUDED),
    ]
    rows.insert(13, ("point 13: occluded, but its pixel shows id 13 -- VISIBLE with PAIS_VIS_SELF", at(40, 30, 6.0), OCCLUDED))
    names = [r[0] for r in rows]
    pts = np.array([r[1] for r in rows], np.float64)
    plain = np.array([r[2] for r in rows], np.uint8)
    with_self = plain.copy()
    with_self[13] = VISIBLE
    return view, depth, idm, pts, tol, names, plain, with_self


def two_walls():
    """A near wall of discs at z = 2 over the left half of a 64 x 48 image and a far wall at z = 4 over all of it, seen by one
    front view (focal 32, pp (32, 24)); all coordinates dyadic.  Near-wall discs sit at pixel columns 0, 2, .. 30 and far-wall
    discs at columns 0, 2, .. 62, rows 0, 2, .. 46, each facing the camera with a radius of 1.5 pixel pitches at its depth, so
    every pixel of columns 0 .. 31 is covered at depth exactly 2 (n' = (0, 0, -1): t = -c'2 / -1) and every other pixel at depth
    exactly 4.  A pixel with both coordinates even lies within rho of one disc of each wall only (the next is 2 pitches away), so
    its id is that disc's index.  The queries are the far wall's own centres and one point at z = 1 over pixel (10, 10); with
    tol = 0.25 a far centre of column u <= 30 has m = 4 - 2 = 2 (OCCLUDED by the near disc of its pixel), one of column u >= 32 has
    m = 0 (VISIBLE, its own disc), the point at z = 1 has m = 1 - 2 = -1 (IN_FRONT).
    -> (view, W, H, centers, normals, radii, queries, tol, expected code, expected occluder, expected margin)."""
    from pais_mvs_amd.render import make_view
    W, H, F = 64, 48, 32.0
    view = make_view(np.eye(3), np.zeros(3), (F, F), (float(W >> 1), float(H >> 1)))
    at = lambda u, v, z: [(u - (W >> 1)) / F * z, (v - (H >> 1)) / F * z, z]
    near = [at(u, v, 2.0) for v in range(0, H, 2) for u in range(0, 32, 2)]
    far = [at(u, v, 4.0) for v in range(0, H, 2) for u in range(0, W, 2)]
    cen = np.array(near + far, np.float64)
    nrm = np.tile([0.0, 0.0, -1.0], (len(cen), 1))
    rad = np.concatenate([np.full(len(near), 1.5 * 2.0 / F), np.full(len(far), 1.5 * 4.0 / F)])
    qry = np.array(far + [at(10, 10, 1.0)], np.float64)
    code, occ, mar = [], [], []
    for v in range(0, H, 2):
        for u in range(0, W, 2):
            hidden = u <= 30
            code.append(OCCLUDED if hidden else VISIBLE)
            occ.append((v // 2) * 16 + u // 2 if hidden else len(near) + (v // 2) * 32 + u // 2)
            mar.append(2.0 if hidden else 0.0)
    code.append(IN_FRONT); occ.append((10 // 2) * 16 + 10 // 2); mar.append(-1.0)
    return view, W, H, cen, nrm, rad, qry, 0.25, np.array(code, np.uint8), np.array(occ, np.int32), np.array(mar)
