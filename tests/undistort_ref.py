"""Helpers of tests/test_undistort_cpu.py and tests/test_undistort_gpu.py: the host shim of pais_undistort.hpp
(tests/undistort_host_shim.cpp), the test inputs, and a numpy restatement of include/pais_undistort.h written from the
header's statements alone -- every statement its own rounded elementwise pass, the Newton loop with masks."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
M2I, I2M = 0, 1                       # PAIS_LENS_MEASURED_TO_IDEAL, PAIS_LENS_IDEAL_TO_MEASURED
UNDISTORT_POINTS, DISTORT_POINTS, IMAGE = 0, 1, 2
MAX_STEPS = 64
KS = (0.0, 0.3, -0.2, -5.0)           # -5: the fold lies inside the image
SIZES = ((1, 1), (4, 1), (67, 41), (256, 3), (130, 70))


class CLens(C.Structure):
    _fields_ = [("focal", C.c_double * 2), ("pp", C.c_double * 2), ("k", C.c_double), ("model", C.c_int32), ("_pad", C.c_int32)]


def clens(focal, pp, k, model):
    L = CLens()
    L.focal[:] = [float(focal[0]), float(focal[1])]
    L.pp[:] = [float(pp[0]), float(pp[1])]
    L.k, L.model = float(k), int(model)
    return L


def rig_lens(w, h, k, model):
    """An anisotropic focal and an off-centre principal point for a w x h image."""
    return clens((0.9 * w + 3.0, 0.7 * w + 5.0), (0.45 * w, 0.55 * h), k, model)


# --------------------------------------------------------------------------------------------------------- the shim ---
_shim = None


def _compile(so, extra):
    src = os.path.join(HERE, "undistort_host_shim.cpp")
    csrc = os.path.join(ROOT, "pais_mvs_amd", "csrc")
    deps = [src, os.path.join(csrc, "pais_undistort.hpp"), os.path.join(csrc, "pais_dev.hpp"), os.path.join(ROOT, "include", "pais_undistort.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off"] + extra + ["-o", so, src])
    return so


def shim():
    global _shim
    if _shim is None:
        S = C.CDLL(_compile(os.path.join(HERE, "build", "libundistort_host_shim.so"), ["-fPIC", "-shared"]))
        dp, bp = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
        S.shim_lens_points.restype = None
        S.shim_lens_points.argtypes = [C.POINTER(CLens), C.c_int, C.c_long, dp, dp, bp, C.POINTER(C.c_int)]
        S.shim_lens_image.restype = C.c_long
        S.shim_lens_image.argtypes = [C.POINTER(CLens), C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_long, C.c_void_p, C.c_void_p]
        _shim = S
    return _shim


def sanitized_program():
    """The shim with its own main, built with -fsanitize=address,undefined: a stand-alone program."""
    return _compile(os.path.join(HERE, "build", "undistort_shim_asan"),
                    ["-g", "-DUNDISTORT_SHIM_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def shim_points(lens, what, xy):
    p = np.ascontiguousarray(xy, np.float64).reshape(-1, 2)
    out, valid, steps = np.empty_like(p), np.zeros(len(p), np.uint8), np.zeros(len(p), np.int32)
    dp = C.POINTER(C.c_double)
    shim().shim_lens_points(C.byref(lens), what, len(p), p.ctypes.data_as(dp), out.ctypes.data_as(dp),
                            valid.ctypes.data_as(C.POINTER(C.c_uint8)), steps.ctypes.data_as(C.POINTER(C.c_int)))
    return out, valid.astype(bool), steps


def shim_image(lens, img):
    """img: (H, W) or (H, W, 3) uint8 with unit pixel stride; rows may be padded."""
    h, w = img.shape[:2]
    ch = 1 if img.ndim == 2 else 3
    dst, mask = np.empty((h, w) + img.shape[2:], np.uint8), np.empty((h, w), np.uint8)
    n = shim().shim_lens_image(C.byref(lens), ch, img.ctypes.data, w, h, img.strides[0], dst.ctypes.data, mask.ctypes.data)
    return dst, mask.astype(bool), int(n)


# ------------------------------------------------------------------------------------------------------ restatement ---
def _finite(a):
    return np.isfinite(a)


def np_forward(L, u, v):
    f0, f1, p0, p1, k = L.focal[0], L.focal[1], L.pp[0], L.pp[1], L.k
    with np.errstate(all="ignore"):
        x = (u - p0) / f0
        y = (v - p1) / f1
        q = (x * x) + (y * y)
        r = k * q
        t = 1.0 + r
        uo = ((t * f0) * x) + p0
        vo = ((t * f1) * y) + p1
        ok = _finite(q) & _finite(t) & _finite(uo) & _finite(vo) & (((3.0 * k) * q) + 1.0 > 0.0)
    return uo, vo, ok, np.zeros(u.shape, np.int32)


def np_inverse(L, u, v):
    f0, f1, p0, p1, k = L.focal[0], L.focal[1], L.pp[0], L.pp[1], L.k
    with np.errstate(all="ignore"):
        x = (u - p0) / f0
        y = (v - p1) / f1
        q = (x * x) + (y * y)
        c = k * q
        ok = _finite(c) & (27.0 * c >= -4.0)
        s = np.ones(u.shape, np.float64)
        steps = np.zeros(u.shape, np.int32)
        active = ok.copy()
        for it in range(MAX_STEPS):
            if not active.any():
                break
            s2 = s * s
            fv = (((c * s2) * s) + s) - 1.0
            d = ((3.0 * c) * s2) + 1.0
            sn = s - (fv / d)
            steps[active] = it + 1
            stop = (c == 0.0) | ((c > 0.0) & (sn >= s)) | ((c < 0.0) & (sn <= s))
            active = active & ~stop
            s = np.where(active, sn, s)
        uo = ((s * f0) * x) + p0
        vo = ((s * f1) * y) + p1
        ok = ok & _finite(uo) & _finite(vo)
    return uo, vo, ok, steps


def uses_inverse(model, what):
    return (model == M2I) == (what != UNDISTORT_POINTS)


def np_map(L, what, u, v):
    uo, vo, ok, steps = (np_inverse if uses_inverse(L.model, what) else np_forward)(L, u, v)
    return np.where(ok, uo, np.nan), np.where(ok, vo, np.nan), ok, steps


def np_points(L, what, xy):
    p = np.asarray(xy, np.float64).reshape(-1, 2)
    uo, vo, ok, steps = np_map(L, what, p[:, 0].copy(), p[:, 1].copy())
    return np.stack([uo, vo], axis=1), ok, steps


def np_image(L, img):
    """-> (dst, mask, valid_pixels) of pais_undistort_image."""
    h, w = img.shape[:2]
    vv, uu = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    sx, sy, ok, _ = np_map(L, IMAGE, uu, vv)
    with np.errstate(all="ignore"):
        ok = ok & (sx >= 0.0) & (sx <= float(w - 1)) & (sy >= 0.0) & (sy <= float(h - 1))
    sx, sy = np.where(ok, sx, 0.0), np.where(ok, sy, 0.0)
    fx, fy = np.floor(sx), np.floor(sy)
    x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    a, b = sx - fx, sy - fy
    a1, b1 = 1.0 - a, 1.0 - b
    w00, w01, w10, w11 = a1 * b1, a * b1, a1 * b, a * b
    src = img.reshape(h, w, -1).astype(np.float64)
    dst = np.zeros(src.shape, np.uint8)
    for ch in range(src.shape[2]):
        I = src[:, :, ch]
        val = ((w00 * I[y0, x0]) + (w01 * I[y0, x1])) + ((w10 * I[y1, x0]) + (w11 * I[y1, x1]))
        dst[:, :, ch] = np.where(ok, np.rint(val), 0.0).astype(np.uint8)
    return dst.reshape(img.shape), ok, int(ok.sum())


# ----------------------------------------------------------------------------------------------------------- inputs ---
def noise_image(w, h, ch, seed, pad=0):
    """Seeded bytes, (h, w) or (h, w, 3); pad > 0: rows `pad` bytes longer than their pixels (a view into a wider buffer)."""
    rng = np.random.default_rng(seed)
    buf = rng.integers(0, 256, size=(h, w * ch + pad), dtype=np.uint8)
    v = buf[:, :w * ch]
    return v if ch == 1 else v.reshape(h, w, 3) if pad == 0 else np.lib.stride_tricks.as_strided(buf, (h, w, 3), (buf.strides[0], 3, 1))


def adjacent(x, n):
    """The n doubles below x, x, and the n above."""
    lo, hi = [x], [x]
    for _ in range(n):
        lo.append(np.nextafter(lo[-1], -np.inf))
        hi.append(np.nextafter(hi[-1], np.inf))
    return lo[:0:-1] + hi


def boundary_points(L, w, h, seed):
    """Points that bracket the boundaries of a lens on a w x h image: a grid over three times the image, the centre pixel
    exactly, and radii at adjacent doubles around the fold circle 3 k q + 1 = 0 and around 27 k q = -4."""
    rng = np.random.default_rng(seed)
    pts = [(L.pp[0], L.pp[1]), (0.0, 0.0), (w - 1.0, h - 1.0)]
    g = np.stack(np.meshgrid(np.linspace(-w, 2.0 * w, 23), np.linspace(-h, 2.0 * h, 19)), axis=-1).reshape(-1, 2)
    pts += [tuple(p) for p in g]
    pts += [tuple(p) for p in rng.uniform((-w, -h), (2.0 * w, 2.0 * h), size=(200, 2))]
    if L.k < 0:
        for q in (-1.0 / (3.0 * L.k), -4.0 / (27.0 * L.k)):
            r = float(np.sqrt(q))
            for du in adjacent(L.pp[0] + r * L.focal[0], 6) + adjacent(L.pp[0] - r * L.focal[0], 6):
                pts.append((du, L.pp[1]))                                  # y = 0 exactly: q = x x
            for dv in adjacent(L.pp[1] + r * L.focal[1], 6):
                pts.append((L.pp[0], dv))
            for x in (r * (1 - 1e-9), r * (1 + 1e-9), r * 0.999, r * 1.001):
                pts.append((L.pp[0] + x * 0.6 * L.focal[0], L.pp[1] + x * 0.8 * L.focal[1]))
    return np.array(pts, np.float64)
