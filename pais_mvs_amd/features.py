"""ctypes binding of include/pais_feature.h: image features on the GPU -- the scale-space detector and gradient-histogram
descriptor of Lowe (2004) with cv::SIFT's default parameters, as the header defines them.  There is
no CPU fallback: detect() raises without a GPU.

    xy, scale, angle, desc = detect(image)        # (n,2) pixels, (n,) sigma in pixels, (n,) radians, (n,128) on a 0..255 scale

`python -m pais_mvs_amd.features image [--out kp.npz]` prints what one image gives and stores the arrays."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib


class FeatureParams(C.Structure):
    """pais_feature_params."""
    _fields_ = [("layers", C.c_int32), ("_pad", C.c_int32), ("sigma", C.c_double), ("input_blur", C.c_double),
                ("contrast_threshold", C.c_double), ("edge_threshold", C.c_double)]


class StageSizes(C.Structure):
    """pais_test_feature_sizes (include/pais_test_hooks.h)."""
    _fields_ = [("octaves", C.c_int32), ("W", C.c_int32), ("H", C.c_int32), ("layers", C.c_int32), ("num_cands", C.c_int64),
                ("num_fit", C.c_int64), ("num_keypoints", C.c_int64)]


def _bind(L):
    if getattr(L, "_feature_bound", False):
        return L
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    L.pais_sizeof_feature_params.restype = C.c_size_t
    assert L.pais_sizeof_feature_params() == C.sizeof(FeatureParams)
    L.pais_feature_default_params.restype = None
    L.pais_feature_default_params.argtypes = [C.POINTER(FeatureParams)]
    L.pais_feature_detect.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.POINTER(FeatureParams), C.c_int, ip, fp, fp, fp,
                                      ip, fp, C.POINTER(C.c_double)]
    L.pais_test_feature_stages.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.POINTER(FeatureParams), C.c_int,
                                           C.POINTER(StageSizes), C.c_int64, fp, C.c_int, ip, ip, C.POINTER(C.c_double)]
    L.pais_mvs_seed_from_images.argtypes = [C.c_void_p, C.c_double, C.POINTER(FeatureParams), C.POINTER(C.c_int)]
    L.pais_feature_last_stage_ms.restype = None
    L.pais_feature_last_stage_ms.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.pais_feature_last_error.restype = C.c_char_p
    L.pais_feature_launches.restype = C.c_int64
    L.pais_feature_launches.argtypes = []
    L._feature_bound = True
    return L


def default_params() -> FeatureParams:
    p = FeatureParams()
    _bind(_lib.load()).pais_feature_default_params(C.byref(p))
    return p


def launches() -> int:
    return int(_bind(_lib.load()).pais_feature_launches())


def last_stage_ms() -> dict:
    """Kernel ms per stage of the last detect() of this thread, and the bytes its blur kernels moved."""
    ms = (C.c_double * 5)()
    b = C.c_double(0)
    _bind(_lib.load()).pais_feature_last_stage_ms(ms, C.byref(b))
    out = dict(zip(("blur", "extrema", "fit", "orient", "describe"), (float(v) for v in ms)))
    out["blur_bytes"] = b.value
    return out


def to_gray(image) -> np.ndarray:
    """An (H,W) uint8 plane as it is; (H,W,3) RGB through the fixed-point weights of reconstruct.load_image_gray."""
    a = np.asarray(image)
    if a.ndim == 3 and a.shape[2] == 3:
        a = a.astype(np.int64)
        a = np.clip((a[..., 0] * 4899 + a[..., 1] * 9617 + a[..., 2] * 1868 + 8192) >> 14, 0, 255)
    if a.ndim != 2:
        raise ValueError("detect: an image is (H, W) grey or (H, W, 3) RGB, got shape %s" % (a.shape,))
    return a.astype(np.uint8) if a.dtype != np.uint8 else a


def detect_raw(gray: np.ndarray, max_keypoints: int, device: int = 0, params: FeatureParams = None):
    """One pais_feature_detect call -> (num found, xy, scale, angle, octave_layer, desc, kernel ms) with max_keypoints rows."""
    L = _bind(_lib.load())
    if gray.dtype != np.uint8 or gray.ndim != 2 or gray.strides[1] != 1 or gray.strides[0] < 0:
        gray = np.ascontiguousarray(gray, dtype=np.uint8)
    k = int(max_keypoints)
    xy, scale, angle = np.zeros((max(k, 0), 2), np.float32), np.zeros(max(k, 0), np.float32), np.zeros(max(k, 0), np.float32)
    ol, desc = np.zeros((max(k, 0), 2), np.int32), np.zeros((max(k, 0), 128), np.float32)
    num, ms = C.c_int32(0), C.c_double(0)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    h, w = gray.shape
    rc = L.pais_feature_detect(int(device), gray.ctypes.data, w, h, gray.strides[0], None if params is None else C.byref(params), k,
                               C.byref(num), xy.ctypes.data_as(fp), scale.ctypes.data_as(fp), angle.ctypes.data_as(fp),
                               ol.ctypes.data_as(ip), desc.ctypes.data_as(fp), C.byref(ms))
    if rc:
        raise RuntimeError("pais_feature_detect failed (%d): %s" % (rc, L.pais_feature_last_error().decode()))
    return num.value, xy, scale, angle, ol, desc, ms.value


def stages(gray: np.ndarray, octave: int, device: int = 0, params: FeatureParams = None) -> dict:
    """TEST HOOK (pais_test_feature_stages): the run of detect_raw with octave `octave` recorded -> dict(octaves, keypoints of the
    whole run; W, H, layers (layers + 3, H, W) float32, cands (k, 3) in the GPU's order, fit_int (k, 4), fit_val (k, 3) of that
    octave; fit rows are empty when the octave has no candidate).  Two calls: the sizes, then the arrays."""
    L = _bind(_lib.load())
    if gray.dtype != np.uint8 or gray.ndim != 2 or gray.strides[1] != 1 or gray.strides[0] < 0:
        gray = np.ascontiguousarray(gray, dtype=np.uint8)
    h, w = gray.shape
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    prm = None if params is None else C.byref(params)
    sz = StageSizes()

    def call(layers, cands, fi, fv):
        rc = L.pais_test_feature_stages(int(device), gray.ctypes.data, w, h, gray.strides[0], prm, int(octave), C.byref(sz), layers.size,
                                        layers.ctypes.data_as(fp), len(cands), cands.ctypes.data_as(ip), fi.ctypes.data_as(ip),
                                        fv.ctypes.data_as(C.POINTER(C.c_double)))
        if rc:
            raise RuntimeError("pais_test_feature_stages failed (%d): %s" % (rc, L.pais_feature_last_error().decode()))

    call(np.zeros(0, np.float32), np.zeros((0, 3), np.int32), np.zeros((0, 4), np.int32), np.zeros((0, 3), np.float64))
    first = (sz.octaves, sz.W, sz.H, sz.layers, sz.num_cands, sz.num_fit, sz.num_keypoints)
    layers = np.zeros((sz.layers, sz.H, sz.W), np.float32)
    cands, fi, fv = np.zeros((sz.num_cands, 3), np.int32), np.zeros((sz.num_cands, 4), np.int32), np.zeros((sz.num_cands, 3), np.float64)
    call(layers, cands, fi, fv)
    if first != (sz.octaves, sz.W, sz.H, sz.layers, sz.num_cands, sz.num_fit, sz.num_keypoints):
        raise RuntimeError("pais_test_feature_stages: the second run's sizes differ from the first's")
    return dict(octaves=sz.octaves, keypoints=sz.num_keypoints, W=sz.W, H=sz.H, layers=layers, cands=cands, fit_int=fi[:sz.num_fit],
                fit_val=fv[:sz.num_fit])


def detect_full(image, device: int = 0, params: FeatureParams = None, first: int = 4096):
    """detect() with the octave / layer of every keypoint and the kernel time: the call is repeated with room for all
    keypoints when the first buffer was too small."""
    gray = to_gray(image)
    cap = int(first)
    while True:
        n, xy, scale, angle, ol, desc, ms = detect_raw(gray, cap, device, params)
        if n <= cap:
            return xy[:n], scale[:n], angle[:n], ol[:n], desc[:n], ms
        cap = n


def detect(image, device: int = 0, params: FeatureParams = None):
    """-> (xy (n,2), scale (n,), angle (n,), desc (n,128)), sorted by (octave, layer, y, x, orientation peak)."""
    xy, scale, angle, _, desc, _ = detect_full(image, device, params)
    return xy, scale, angle, desc


def main(argv=None):
    import argparse
    from .reconstruct import load_image_gray
    ap = argparse.ArgumentParser(description="keypoints and descriptors of one image")
    ap.add_argument("image")
    ap.add_argument("--out", default="", help="store xy, scale, angle, octave_layer, desc in this .npz")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    gray, _ = load_image_gray(a.image)
    xy, scale, angle, ol, desc, ms = detect_full(gray, a.device)
    print("%s: %d x %d, %d keypoints, kernels %.3f ms" % (a.image, gray.shape[1], gray.shape[0], len(xy), ms))
    for o in sorted(set(ol[:, 0].tolist())):
        print("  octave %d: %d" % (o, int((ol[:, 0] == o).sum())))
    if a.out:
        np.savez(a.out, xy=xy, scale=scale, angle=angle, octave_layer=ol, desc=desc)


if __name__ == "__main__":
    main()
