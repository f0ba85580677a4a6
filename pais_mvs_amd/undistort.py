"""`python -m pais_mvs_amd.undistort IMAGE --focal F --k K --model {measured-to-ideal,ideal-to-measured} --out FILE`

The radial term of an NVM camera taken out of images and measurements on the GPU (include/pais_undistort.h, DESIGN.md
section 5.7).  The cost kernels, the setters, the seeds and reCentering project through the ideal pinhole, so a camera with
k != 0 is made ideal BEFORE its pyramid is built: undistort_camera() resamples its grey and RGB images and returns a new,
finalised Camera with radial_distortion = 0 and the same size, focal and principal point; undistort_points() does the
same to the NVM measurements.  There is no CPU fallback: every call raises without a GPU.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .camera import Camera

MODELS = {"measured-to-ideal": _lib.LENS_MEASURED_TO_IDEAL, "ideal-to-measured": _lib.LENS_IDEAL_TO_MEASURED}


def model_code(model) -> int:
    if isinstance(model, str):
        if model not in MODELS:
            raise ValueError("lens model %r is not one of %s" % (model, sorted(MODELS)))
        return MODELS[model]
    return int(model)


def Lens(focal, pp, k: float, model=_lib.LENS_MEASURED_TO_IDEAL) -> "_lib.Lens":
    """A pais_lens record.  focal: one value or (fx, fy); pp: the principal point in pixels."""
    f = np.asarray(focal, np.float64).reshape(-1)
    L = _lib.Lens()
    L.focal[:] = [float(f[0]), float(f[-1])]
    L.pp[:] = [float(pp[0]), float(pp[1])]
    L.k = float(k)
    L.model = model_code(model)
    return L


def lens_of(camera, model, k: Optional[float] = None) -> "_lib.Lens":
    """The lens of a finalised camera.Camera: its focal, principal point and radial_distortion (or k)."""
    return Lens(camera.focal, camera.principle_point, camera.radial_distortion if k is None else k, model)


def launches() -> int:
    return int(_lib.load().pais_undistort_launches())


def _points(entry: str, xy, lens, device: int) -> Tuple[np.ndarray, np.ndarray, float]:
    p = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
    out = np.empty_like(p)
    valid = np.zeros(len(p), np.uint8)
    ms = C.c_double(0)
    L = _lib.load()
    dp = C.POINTER(C.c_double)
    rc = getattr(L, entry)(int(device), C.byref(lens), len(p), p.ctypes.data_as(dp), out.ctypes.data_as(dp),
                           valid.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(ms))
    if rc:
        raise RuntimeError("%s failed (%d): %s" % (entry, rc, L.pais_undistort_last_error().decode()))
    return out, valid.astype(bool), ms.value


def undistort_points(xy, lens, device: int = 0) -> Tuple[np.ndarray, np.ndarray, float]:
    """Measured pixels (n, 2) -> (ideal pixels (n, 2), valid (n,) bool, kernel_ms); an invalid point is (NaN, NaN)."""
    return _points("pais_undistort_points", xy, lens, device)


def distort_points(xy, lens, device: int = 0) -> Tuple[np.ndarray, np.ndarray, float]:
    """Ideal pixels (n, 2) -> (measured pixels (n, 2), valid (n,) bool, kernel_ms)."""
    return _points("pais_distort_points", xy, lens, device)


def undistort_image(image, lens, device: int = 0) -> Tuple[np.ndarray, np.ndarray, float]:
    """image (H, W) or (H, W, 3) uint8 with unit pixel stride (rows may be padded) -> (the ideal image of the same shape,
    mask (H, W) bool of the pixels whose source lies inside the measured image, kernel_ms)."""
    img = np.asarray(image)
    if img.dtype != np.uint8 or img.ndim not in (2, 3) or (img.ndim == 3 and img.shape[2] != 3):
        raise ValueError("undistort_image: a (H, W) or (H, W, 3) uint8 image is needed, got %s %s" % (img.dtype, img.shape))
    ch = 1 if img.ndim == 2 else 3
    tight = img.strides[-1] == 1 and (ch == 1 or img.strides[1] == 3) and img.strides[0] >= img.shape[1] * ch
    if not tight:
        img = np.ascontiguousarray(img)
    h, w = img.shape[:2]
    dst = np.empty(img.shape, np.uint8)
    mask = np.empty((h, w), np.uint8)
    n, ms = C.c_int64(0), C.c_double(0)
    L = _lib.load()
    rc = L.pais_undistort_image(int(device), C.byref(lens), ch, img.ctypes.data, w, h, img.strides[0], dst.ctypes.data, mask.ctypes.data,
                                C.byref(n), C.byref(ms))
    if rc:
        raise RuntimeError("pais_undistort_image failed (%d): %s" % (rc, L.pais_undistort_last_error().decode()))
    return dst, mask.astype(bool), ms.value


def undistort_camera(cam: Camera, model, lod_ratio: float, cfg_max_lod: int, build_edges: bool = True, device: int = 0,
                     name: Optional[str] = None, gray_of_rgb=None) -> Camera:
    """A new, finalised Camera: cam's grey and RGB images resampled to the ideal pinhole, radial_distortion = 0; size, focal,
    principal point and pose are cam's.  gray_of_rgb (with an RGB image): the grey image is that function of the resampled
    RGB instead -- what a reload of the written RGB gives (reconstruct --undistort)."""
    h, w = cam.image.shape
    pp = np.asarray(cam.principle_point, np.float64).reshape(2)
    if pp[0] < 0 and pp[1] < 0:  # camera.cpp:101-106, as Camera.finalize
        pp = np.array([float(w >> 1), float(h >> 1)])
    lens = Lens(cam.focal, pp, cam.radial_distortion, model)
    gray, _, _ = undistort_image(cam.image, lens, device)
    rgb = None
    if cam.rgb is not None:
        rgb = undistort_image(cam.rgb, lens, device)[0]
        if gray_of_rgb is not None:
            gray = np.ascontiguousarray(gray_of_rgb(rgb), np.uint8)
    return Camera(focal=np.array(cam.focal, np.float64), principle_point=pp.copy(), quaternion=np.array(cam.quaternion, np.float64),
                  center=np.array(cam.center, np.float64), image=gray, name=cam.name if name is None else name, rgb=rgb,
                  radial_distortion=0.0).finalize(lod_ratio, cfg_max_lod, build_edges)


def undistort_scene(cameras: Sequence[Camera], model, lod_ratio: float, cfg_max_lod: int, build_edges: bool = True,
                    device: int = 0) -> List[Camera]:
    return [undistort_camera(c, model, lod_ratio, cfg_max_lod, build_edges, device) for c in cameras]


def main(argv=None):
    import argparse
    from PIL import Image
    ap = argparse.ArgumentParser(description="undistort one image on the GPU")
    ap.add_argument("image")
    ap.add_argument("--focal", type=float, required=True)
    ap.add_argument("--k", type=float, required=True)
    ap.add_argument("--model", choices=sorted(MODELS), required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--pp", type=float, nargs=2, default=None, help="principal point (default: width / 2, height / 2, as Camera::Camera)")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    im = Image.open(a.image)
    img = np.asarray(im.convert("L") if im.mode in ("L", "1", "I", "F") else im.convert("RGB"))
    h, w = img.shape[:2]
    pp = a.pp if a.pp is not None else (float(w >> 1), float(h >> 1))
    out, mask, ms = undistort_image(img, Lens(a.focal, pp, a.k, a.model), a.device)
    Image.fromarray(out).save(a.out)
    print("%d x %d, %d of %d pixels valid, kernel %.3f ms" % (w, h, int(mask.sum()), w * h, ms))


if __name__ == "__main__":
    main()
