"""Helpers of tests/test_features_cpu.py and tests/test_features_gpu.py: the host shim of pais_feature.hpp
(tests/feature_host_shim.cpp), the test images, and a numpy restatement of include/pais_feature.h written from the header's
statements alone -- float32 blur with an explicit ascending tap loop, everything after it in float64 with numpy's own libm."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PI2 = 6.283185307179586
LN2 = 0.6931471805599453
DEFAULTS = dict(layers=3, sigma=1.6, input_blur=0.5, contrast=0.04, edge=10.0)

_shim = None


def shim():
    global _shim
    if _shim is not None:
        return _shim
    bdir = os.path.join(HERE, "build")
    os.makedirs(bdir, exist_ok=True)
    so = os.path.join(bdir, "libfeature_host_shim.so")
    src = os.path.join(HERE, "feature_host_shim.cpp")
    csrc = os.path.join(ROOT, "pais_mvs_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in ("pais_feature.hpp", "pais_dev.hpp", "pais_detmath.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, src])
    S = C.CDLL(so)
    dp, fp, ip = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int)
    S.shim_atan2.restype = C.c_double
    S.shim_atan2.argtypes = [C.c_double, C.c_double]
    S.shim_atan2_many.argtypes = [dp, dp, C.c_long, dp]
    S.shim_feat_tap_radius.argtypes = [C.c_double]
    S.shim_feat_taps.argtypes = [C.c_double, fp]
    S.shim_feat_run.restype = C.c_long
    S.shim_feat_run.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_long, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double]
    S.shim_feat_result.argtypes = [fp, fp, fp, ip, fp]
    S.shim_feat_octave_size.argtypes = [C.c_int, ip, ip]
    S.shim_feat_layers.argtypes = [C.c_int, fp]
    S.shim_feat_num_cands.restype = C.c_long
    S.shim_feat_num_cands.argtypes = [C.c_int]
    S.shim_feat_cands.argtypes = [C.c_int, ip]
    S.shim_feat_fit.argtypes = [C.c_int, ip, dp]
    _shim = S
    return S


class ShimRun:
    """One run of the shim: the output arrays of pais_feature_detect, and (stages=True) every octave's layers, candidates, fit."""

    def __init__(self, gray, stages=False, **prm):
        S = shim()
        p = dict(DEFAULTS, **prm)
        g = gray if (gray.dtype == np.uint8 and gray.strides[1] == 1) else np.ascontiguousarray(gray, np.uint8)
        h, w = g.shape
        n = S.shim_feat_run(g.ctypes.data, w, h, g.strides[0], p["layers"], p["sigma"], p["input_blur"], p["contrast"], p["edge"])
        if n < 0:
            raise ValueError("shim_feat_run refused the parameters")
        self.n = n
        self.xy, self.scale, self.angle = np.zeros((n, 2), np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
        self.ol, self.desc = np.zeros((n, 2), np.int32), np.zeros((n, 128), np.float32)
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
        S.shim_feat_result(self.xy.ctypes.data_as(fp), self.scale.ctypes.data_as(fp), self.angle.ctypes.data_as(fp),
                           self.ol.ctypes.data_as(ip), self.desc.ctypes.data_as(fp))
        self.octaves = []
        for o in range(S.shim_feat_octaves() if stages else 0):
            W, H = C.c_int(0), C.c_int(0)
            S.shim_feat_octave_size(o, C.byref(W), C.byref(H))
            L = np.zeros((p["layers"] + 3, H.value, W.value), np.float32)
            S.shim_feat_layers(o, L.ctypes.data_as(fp))
            k = S.shim_feat_num_cands(o)
            cands = np.zeros((k, 3), np.int32)
            fi, fv = np.zeros((k, 4), np.int32), np.zeros((k, 3), np.float64)
            if k:
                S.shim_feat_cands(o, cands.ctypes.data_as(ip))
                S.shim_feat_fit(o, fi.ctypes.data_as(ip), fv.ctypes.data_as(C.POINTER(C.c_double)))
            self.octaves.append(dict(layers=L, cands=cands, fit_int=fi, fit_val=fv))


# ------------------------------------------------------------------------------------------------------------- images ---
def noise_image(width, height, seed, smooth=2.0, mean=128.0, std=45.0):
    """Seeded band-limited noise: white noise through a Gaussian of `smooth` pixels, stretched to mean / std, 8 bit."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((height + 32, width + 32))
    r = int(4 * smooth)
    k = np.exp(-np.arange(-r, r + 1) ** 2 / (2.0 * smooth * smooth))
    k /= k.sum()
    a = np.apply_along_axis(lambda v: np.convolve(v, k, mode="same"), 0, a)
    a = np.apply_along_axis(lambda v: np.convolve(v, k, mode="same"), 1, a)[16:-16, 16:-16]
    a = (a - a.mean()) / a.std() * std + mean
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


def shift_pair():
    """A 96 x 96 texture at (32, 32) and at (48, 64) of two 256 x 256 zero images -> (a, b, (16, 32))."""
    tex = noise_image(96, 96, 11)
    a, b = np.zeros((256, 256), np.uint8), np.zeros((256, 256), np.uint8)
    a[32:128, 32:128] = tex
    b[64:160, 48:144] = tex
    return a, b, (16, 32)


def support_radius(scale_px):
    """The descriptor window's radius in IMAGE pixels for a keypoint of `scale` (the header's rad, before rounding, plus the
    rounding and the gradient's own sample either side): nothing further from the keypoint is read by orientation or
    descriptor (the orientation window, 4.5 s, is smaller)."""
    return 3.0 * scale_px * 1.4142135623730951 * 2.5 + 0.5 + 1.0


# --------------------------------------------------------------------------------------------------- numpy restatement ---
def np_taps(s):
    R = int(math.ceil(4.0 * s))
    w = [math.exp(-float((k - R) * (k - R)) / (2.0 * s * s)) for k in range(2 * R + 1)]
    S = 0.0
    for v in w:
        S = S + v
    return np.array([v / S for v in w], dtype=np.float64).astype(np.float32), R


def np_sigmas(p):
    n = p["layers"]
    sig = [math.sqrt(max(p["sigma"] * p["sigma"] - 4.0 * p["input_blur"] * p["input_blur"], 0.01))]
    k = math.pow(2.0, 1.0 / n)
    for i in range(1, n + 3):
        a = p["sigma"] * math.pow(k, float(i - 1))
        b = a * k
        sig.append(math.sqrt(b * b - a * a))
    return sig


def np_blur(I, t, R):
    H, W = I.shape
    xs, ys = np.arange(W), np.arange(H)
    acc = np.zeros((H, W), np.float32)
    for k in range(2 * R + 1):                       # ascending tap index, product and sum each rounded to float32
        acc = acc + t[k] * I[:, np.clip(xs + k - R, 0, W - 1)]
    out = np.zeros((H, W), np.float32)
    for k in range(2 * R + 1):
        out = out + t[k] * acc[np.clip(ys + k - R, 0, H - 1), :]
    return out


def np_double(g):
    G = g.astype(np.float32)
    H, W = G.shape
    x1, y1 = np.minimum(np.arange(W) + 1, W - 1), np.minimum(np.arange(H) + 1, H - 1)
    h = np.float32(0.5)
    D = np.zeros((2 * H, 2 * W), np.float32)
    D[0::2, 0::2] = G
    D[0::2, 1::2] = h * (G + G[:, x1])
    D[1::2, 0::2] = h * (G + G[y1, :])
    D[1::2, 1::2] = h * (h * (G + G[:, x1]) + h * (G[y1, :] + G[y1, :][:, x1]))
    return D


def _inv3(m):
    c00 = m[4] * m[8] - m[5] * m[7]
    c01 = m[3] * m[8] - m[5] * m[6]
    c02 = m[3] * m[7] - m[4] * m[6]
    d = m[0] * c00 - m[1] * c01 + m[2] * c02
    if d == 0.0:
        return [0.0] * 9
    d = 1.0 / d
    return [c00 * d, (m[2] * m[7] - m[1] * m[8]) * d, (m[1] * m[5] - m[2] * m[4]) * d,
            (m[5] * m[6] - m[3] * m[8]) * d, (m[0] * m[8] - m[2] * m[6]) * d, (m[2] * m[3] - m[0] * m[5]) * d,
            (m[3] * m[7] - m[4] * m[6]) * d, (m[1] * m[6] - m[0] * m[7]) * d, (m[0] * m[4] - m[1] * m[3]) * d]


def np_fit(Dg, x, y, i, p):
    """FIT of one candidate on the float64 DoG stack Dg[i][y][x] -> None or (x, y, i, px, py, s)."""
    n = p["layers"]
    _, H, W = Dg.shape
    D = lambda ii, xx, yy: float(Dg[ii, yy, xx])
    for _ in range(5):
        dx = (D(i, x + 1, y) - D(i, x - 1, y)) * 0.5
        dy = (D(i, x, y + 1) - D(i, x, y - 1)) * 0.5
        ds = (D(i + 1, x, y) - D(i - 1, x, y)) * 0.5
        v2 = 2.0 * D(i, x, y)
        dxx = (D(i, x + 1, y) + D(i, x - 1, y)) - v2
        dyy = (D(i, x, y + 1) + D(i, x, y - 1)) - v2
        dss = (D(i + 1, x, y) + D(i - 1, x, y)) - v2
        dxy = ((D(i, x + 1, y + 1) - D(i, x - 1, y + 1)) - (D(i, x + 1, y - 1) - D(i, x - 1, y - 1))) * 0.25
        dxs = ((D(i + 1, x + 1, y) - D(i + 1, x - 1, y)) - (D(i - 1, x + 1, y) - D(i - 1, x - 1, y))) * 0.25
        dys = ((D(i + 1, x, y + 1) - D(i + 1, x, y - 1)) - (D(i - 1, x, y + 1) - D(i - 1, x, y - 1))) * 0.25
        A = _inv3([dxx, dxy, dxs, dxy, dyy, dys, dxs, dys, dss])
        X = [-((A[3 * j] * dx + A[3 * j + 1] * dy) + A[3 * j + 2] * ds) for j in range(3)]
        if all(abs(v) < 0.5 for v in X):
            c = D(i, x, y) + 0.5 * ((dx * X[0] + dy * X[1]) + ds * X[2])
            if abs(c) * n < p["contrast"] * 255.0:
                return None
            tr, det = dxx + dyy, dxx * dyy - dxy * dxy
            e = p["edge"]
            if det <= 0.0 or (tr * tr) * e >= ((e + 1.0) * (e + 1.0)) * det:
                return None
            return (x, y, i, x + X[0], y + X[1], p["sigma"] * math.exp((i + X[2]) / n * LN2))
        if not all(abs(v) <= 1e6 for v in X):
            return None
        x += int(math.floor(X[0] + 0.5)); y += int(math.floor(X[1] + 0.5)); i += int(math.floor(X[2] + 0.5))
        if i < 1 or i > n or not (5 <= x < W - 5 and 5 <= y < H - 5):
            return None
    return None


def _gradients(L, x, y, rad):
    """Window samples in the header's order (dy outer, dx inner): dx, dy, the mask of existing samples, mag, ori."""
    H, W = L.shape
    dy, dx = np.meshgrid(np.arange(-rad, rad + 1), np.arange(-rad, rad + 1), indexing="ij")
    dx, dy = dx.ravel(), dy.ravel()
    xx, yy = x + dx, y + dy
    ok = (xx > 0) & (xx < W - 1) & (yy > 0) & (yy < H - 1)
    xc, yc = np.clip(xx, 1, W - 2), np.clip(yy, 1, H - 2)
    gx = L[yc, xc + 1] - L[yc, xc - 1]
    gy = L[yc - 1, xc] - L[yc + 1, xc]
    return dx, dy, ok, np.sqrt(gx * gx + gy * gy), np.arctan2(gy, gx)


def np_orient(L, x, y, s):
    """-> [(peak index j, theta)] of the keypoint (x, y) of scale s on the float64 layer L."""
    so = 1.5 * s
    rad = int(math.floor(3.0 * so + 0.5))
    e = -1.0 / (2.0 * so * so)
    dx, dy, ok, mag, ori = _gradients(L, x, y, rad)
    b = np.floor(ori * (36.0 / PI2) + 0.5).astype(np.int64)
    b = np.where(b < 0, b + 36, b)
    b = np.where(b >= 36, b - 36, b)
    hist = np.zeros(36)
    np.add.at(hist, b[ok], (np.exp((dx * dx + dy * dy).astype(np.float64) * e) * mag)[ok])
    h = [((hist[j - 2] + hist[(j + 2) % 36]) * (1.0 / 16.0) + (hist[j - 1] + hist[(j + 1) % 36]) * (4.0 / 16.0)) + hist[j] * (6.0 / 16.0)
         for j in range(36)]
    m = max(h)
    out = []
    for j in range(36):
        hl, hr = h[j - 1], h[(j + 1) % 36]
        if h[j] > hl and h[j] > hr and h[j] >= 0.8 * m:
            bn = j + 0.5 * (hl - hr) / ((hl - 2.0 * h[j]) + hr)
            if bn < 0:
                bn += 36.0
            if bn >= 36.0:
                bn -= 36.0
            out.append((j, bn * (PI2 / 36.0)))
    return out


def np_describe(L, x, y, s, theta):
    H, W = L.shape
    hw = 3.0 * s
    rad = min(int(math.floor(hw * 1.4142135623730951 * 2.5 + 0.5)), int(math.floor(math.sqrt(float(W) * W + float(H) * H))))
    ct, st = math.cos(theta) / hw, math.sin(theta) / hw
    dx, dy, ok, mag, ori = _gradients(L, x, y, rad)
    cr, rr = dx * ct - dy * st, dx * st + dy * ct
    rb, cb = rr + 1.5, cr + 1.5
    ok = ok & (rb > -1.0) & (rb < 4.0) & (cb > -1.0) & (cb < 4.0)
    m = mag * np.exp((cr * cr + rr * rr) * (-0.125))
    ori = np.where(ori < 0, ori + PI2, ori)
    ob = (ori - theta) * (8.0 / PI2)
    r0, c0, o0 = np.floor(rb), np.floor(cb), np.floor(ob)
    fr, fc, fo = rb - r0, cb - c0, ob - o0
    o0 = o0.astype(np.int64)
    o0 = np.where(o0 < 0, o0 + 8, o0)
    o0 = np.where(o0 >= 8, o0 - 8, o0)
    v1 = m * fr; v0 = m - v1
    v11 = v1 * fc; v10 = v1 - v11; v01 = v0 * fc; v00 = v0 - v01
    v111 = v11 * fo; v110 = v11 - v111; v101 = v10 * fo; v100 = v10 - v101
    v011 = v01 * fo; v010 = v01 - v011; v001 = v00 * fo; v000 = v00 - v001
    idx = ((r0.astype(np.int64) + 1) * 6 + (c0.astype(np.int64) + 1)) * 10 + o0
    vals = np.stack([v000, v001, v010, v011, v100, v101, v110, v111], axis=1)[ok]
    ids = (idx[ok][:, None] + np.array([0, 1, 10, 11, 60, 61, 70, 71])[None, :])
    Hh = np.zeros(360)
    np.add.at(Hh, ids.ravel(), vals.ravel())          # sample after sample, the eight shares in the header's order
    Hh = Hh.reshape(6, 6, 10)
    Hh[:, :, 0] += Hh[:, :, 8]
    Hh[:, :, 1] += Hh[:, :, 9]
    d = Hh[1:5, 1:5, :8].reshape(128).copy()
    t = 0.2 * math.sqrt(float((d * d).sum()))
    d = np.minimum(d, t)
    g = 512.0 / max(math.sqrt(float((d * d).sum())), 2.0 ** -52)
    return np.minimum(d * g, 255.0).astype(np.float32)


def np_detect(gray, **prm):
    """The whole definition -> dict(octaves=[dict(layers, dog, cands=set of (x, y, i))], keys=[(o, i, y, x, j)], xy, scale,
    angle (float64, before the final rounding to float), desc (n,128) float32)."""
    p = dict(DEFAULTS, **prm)
    n = p["layers"]
    sig = np_sigmas(p)
    tabs = [np_taps(s) for s in sig]
    Rmax = max(R for _, R in tabs)
    pre = np.float32(math.floor(0.5 * p["contrast"] / n * 255.0))
    H0, W0 = gray.shape
    W, H = 2 * W0, 2 * H0
    out = dict(octaves=[], keys=[], xy=[], scale=[], angle=[], desc=[])
    base = None
    o = 0
    while o < 24 and min(W, H) >= 2 * Rmax + 1 + 5:
        L = [np_blur(np_double(gray), *tabs[0]) if o == 0 else base]
        for i in range(1, n + 3):
            L.append(np_blur(L[i - 1], *tabs[i]))
        L = np.stack(L)
        Dg = L[1:] - L[:-1]                               # one float32 subtraction
        cands = set()
        for i in range(1, n + 1):
            v = Dg[i, 5:H - 5, 5:W - 5]
            ge, le = np.ones(v.shape, bool), np.ones(v.shape, bool)
            for di in (-1, 0, 1):
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        u = Dg[i + di, 5 + dy:H - 5 + dy, 5 + dx:W - 5 + dx]
                        ge &= v >= u
                        le &= v <= u
            hit = (np.abs(v) > pre) & (((v > 0) & ge) | ((v < 0) & le))
            ys, xs = np.nonzero(hit)
            cands |= {(int(x) + 5, int(y) + 5, i) for x, y in zip(xs, ys)}
        out["octaves"].append(dict(layers=L, dog=Dg, cands=cands))
        D64, L64 = Dg.astype(np.float64), L.astype(np.float64)
        kps = {}
        for (x, y, i) in cands:
            f = np_fit(D64, x, y, i, p)
            if f is not None:
                kps[(f[2], f[1], f[0])] = f                # one keypoint per (i, y, x)
        f2 = 2.0 ** (o - 1)
        for key in sorted(kps):
            x, y, i, px, py, s = kps[key]
            for j, theta in np_orient(L64[i], x, y, s):
                out["keys"].append((o, i, y, x, j))
                out["xy"].append((px * f2, py * f2))
                out["scale"].append(s * f2)
                out["angle"].append(theta)
                out["desc"].append(np_describe(L64[i], x, y, s, theta))
        base = L[n][0::2, 0::2][:H // 2, :W // 2].copy()
        W, H, o = W // 2, H // 2, o + 1
    out["xy"] = np.array(out["xy"], np.float64).reshape(-1, 2)
    out["scale"], out["angle"] = np.array(out["scale"], np.float64), np.array(out["angle"], np.float64)
    out["desc"] = np.array(out["desc"], np.float32).reshape(-1, 128)
    return out


# -------------------------------------------------------------------------------------------- the cases of the stage tests ---
# One parameter changed at a time from DEFAULTS, and one combination.  layers sets gridDim.z of the extrema kernel, the layer
# count of every buffer and the source layer of the halving; sigma and layers set every tap radius.
PARAM_CASES = {
    "layers1": dict(layers=1), "layers2": dict(layers=2), "layers5": dict(layers=5), "layers8": dict(layers=8),
    "sigma1.2": dict(sigma=1.2), "sigma2.4": dict(sigma=2.4),
    "contrast0.01": dict(contrast=0.01), "contrast0.09": dict(contrast=0.09),
    "edge3": dict(edge=3.0), "edge40": dict(edge=40.0),
    "input_blur0.3": dict(input_blur=0.3),
    "combination": dict(layers=4, sigma=2.0, contrast=0.02, edge=6.0),
}


def checkerboard(width, height, cell):
    y, x = np.mgrid[0:height, 0:width]
    return ((((x // cell) + (y // cell)) % 2) * 255).astype(np.uint8)


def vertical_step(width, height, column):
    g = np.zeros((height, width), np.uint8)
    g[:, column:] = 255
    return g


def saturated_noise():
    return np.clip(3 * noise_image(160, 120, 2).astype(np.int64) - 200, 0, 255).astype(np.uint8)


def blobs(width=160, height=120, pitch=30, first=20, size=7, value=200):
    """Squares of `size` pixels centred on (first + pitch a, first + pitch b), on black."""
    g = np.zeros((height, width), np.uint8)
    for y in range(first - size // 2, height - size, pitch):
        for x in range(first - size // 2, width - size, pitch):
            g[y:y + size, x:x + size] = value
    return g


CONTENT_CASES = {
    "checkerboard5-97x61": lambda: checkerboard(97, 61, 5),       # exact ties, symmetric
    "checkerboard8-160x120": lambda: checkerboard(160, 120, 8),   # every candidate rejected by the FIT
    "step-160x120": lambda: vertical_step(160, 120, 80),          # the same, on an edge
    "saturated-noise": saturated_noise,                           # two candidates refine onto one (x, y, layer)
    "blobs": blobs,
}


def max_tap_radius(**prm):
    """The largest blur radius of a parameter set, from the shim's own feat_tap_radius."""
    S = shim()
    return max(S.shim_feat_tap_radius(s) for s in np_sigmas(dict(DEFAULTS, **prm)))


def fit_duplicates(octv):
    """How many `ok` FIT rows of one ShimRun octave land on an (x, y, layer) that another ok row already holds."""
    keys = [(i, y, x) for x, y, i, ok in octv["fit_int"].tolist() if ok]
    return len(keys) - len(set(keys))
