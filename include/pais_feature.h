/* pais_feature.h -- image features on the GPU: the step FeatureManager::setSeedPatches starts with
 * (`SIFT sift; sift(img, img, keypoints[i], descriptors[i])`, mvs/featuremanager.cpp:18-26), so that a scene without points
 * seeds itself.  The method is the scale-space detector and gradient-histogram descriptor of Lowe (IJCV 2004) with the
 * parameters of cv::SIFT's default constructor.  The reference links OpenCV 2.4 for it and has no source of its own, so the
 * feature is DEFINED HERE, by the statements below; the result follows them exactly and is a pure function of the image and
 * the parameters.  Parity with OpenCV's bits is not pinned (DESIGN.md 5.1 wording applies): OpenCV detects in float with its
 * own border rule, fastAtan2 and exp tables.  What is pinned is this text.
 *
 * Arithmetic.  FP32 where a statement says float, FP64 elsewhere.  Every product and every sum is rounded on its own (no
 * contraction); a sum written  a + b + c  is (a + b) + c.  sqrt, floor and the conversions are IEEE-exact.  exp, sin, cos, atan2
 * are pais::det_exp, det_sin, det_cos, det_atan2 (pais_detmath.hpp).  PI2 = 6.283185307179586, LN2 = 0.6931471805599453.
 *
 * GREY.  The input is one 8-bit grey plane.  From RGB it is (4899 R + 9617 G + 1868 B + 8192) >> 14, the fixed-point weights of
 * reconstruct.load_image_gray.  G(x, y) is that byte as a float.
 *
 * TAPS(s).  For a blur of standard deviation s: radius R = (int)ceil(4 s), 2R + 1 taps.  On the host, in double:
 * w_k = exp(-((k - R)(k - R)) / (2 s s)), k = 0 .. 2R;  S = w_0 + w_1 + ... in ascending k;  t_k = (float)(w_k / S).  The table goes
 * to the device as floats.
 *
 * BLUR(I, s).  Separable, rows then columns, float.  Border rule: REPLICATE -- a sample index outside the image is clamped to
 * the nearest one inside, clamp(i, 0, n - 1).
 *   rows:     T(x, y) = sum over k = 0 .. 2R ascending of  t_k * I(clamp(x + k - R, 0, W - 1), y)
 *   columns:  O(x, y) = sum over k = 0 .. 2R ascending of  t_k * T(x, clamp(y + k - R, 0, H - 1))
 * each sum one chain  acc = acc + t_k * v  starting from acc = 0.
 *
 * DOUBLING.  Octave 0 is 2W x 2H.  With x1 = min(x + 1, W - 1), y1 = min(y + 1, H - 1):
 *   D(2x, 2y) = G(x, y);  D(2x + 1, 2y) = 0.5f (G(x, y) + G(x1, y));  D(2x, 2y + 1) = 0.5f (G(x, y) + G(x, y1));
 *   D(2x + 1, 2y + 1) = 0.5f (0.5f (G(x, y) + G(x1, y)) + 0.5f (G(x, y1) + G(x1, y1)))            (all exact in float).
 *
 * OCTAVES.  n = layers (3).  An octave holds n + 3 Gaussian layers L_0 .. L_{n+2} and n + 2 differences.
 *   k = 2^(1/n) (pow, host, double);  sig_0 = sigma;  for i >= 1:  p = sigma k^(i-1) (pow), q = p k,  sig_i = sqrt(q q - p p).
 *   octave 0:  L_0 = BLUR(D, sqrt(max(sigma sigma - 4 input_blur input_blur, 0.01)));   L_i = BLUR(L_{i-1}, sig_i).
 *   HALVING: octave o + 1 has W' = W_o / 2, H' = H_o / 2 (integer division) and L_0'(x, y) = L_n(2x, 2y) of octave o.
 *   Octave o exists iff min(W_o, H_o) >= 2 Rmax + 1 + 5, Rmax the radius of the widest of the tables above (default
 *   parameters: 32): below that the widest blur is mostly border.  A 12 x 12 input (24 x 24 doubled) has no octave.
 *   At most 24 octaves.
 * DoG.  D_i(x, y) = L_{i+1}(x, y) - L_i(x, y), one float subtraction, i = 0 .. n + 1.
 *
 * EXTREMA.  Border margin 5: candidates are the samples (x, y, i) with 5 <= x < W_o - 5, 5 <= y < H_o - 5, 1 <= i <= n,
 * v = D_i(x, y), |v| > P with P = (float)floor(0.5 contrast_threshold / n * 255) (the pre-threshold; default 1), and
 * either v > 0 and v >= each of the 26 neighbours in D_{i-1}, D_i, D_{i+1}, or v < 0 and v <= each of them (NON-strict).
 *
 * FIT (FP64; D values converted to double).  At (x, y, i), at most 5 times:
 *   dx = (D_i(x+1, y) - D_i(x-1, y)) 0.5;  dy = (D_i(x, y+1) - D_i(x, y-1)) 0.5;  ds = (D_{i+1}(x, y) - D_{i-1}(x, y)) 0.5
 *   v2 = 2 D_i(x, y);  dxx = (D_i(x+1, y) + D_i(x-1, y)) - v2;  dyy, dss alike along y and along i
 *   dxy = ((D_i(x+1, y+1) - D_i(x-1, y+1)) - (D_i(x+1, y-1) - D_i(x-1, y-1))) 0.25
 *   dxs = ((D_{i+1}(x+1, y) - D_{i+1}(x-1, y)) - (D_{i-1}(x+1, y) - D_{i-1}(x-1, y))) 0.25;  dys alike along y
 *   A = inverse of [dxx dxy dxs; dxy dyy dys; dxs dys dss] by pais::inv3 (cofactors times 1 / det; zeros when det == 0)
 *   X_j = -((A_j0 dx + A_j1 dy) + A_j2 ds),  j = 0, 1, 2  (offsets in x, y, i)
 *   if every |X_j| < 0.5: converged, stop.  If any X_j is not finite or |X_j| > 1e6: reject.
 *   MOVE: x += (int)floor(X_0 + 0.5), y += (int)floor(X_1 + 0.5), i += (int)floor(X_2 + 0.5); reject if i < 1, i > n or (x, y)
 *   leaves the margin.  Not converged after the 5th evaluation: reject.
 *   CONTRAST: c = D_i(x, y) + 0.5 ((dx X_0 + dy X_1) + ds X_2);  reject if |c| n < contrast_threshold 255.
 *   EDGE: tr = dxx + dyy, det = dxx dyy - dxy dxy;  reject if det <= 0 or (tr tr) edge_threshold >= ((edge_threshold + 1)
 *   (edge_threshold + 1)) det.
 *   px = x + X_0, py = y + X_1 (octave pixels);  s = sigma det_exp((i + X_2) / n LN2).
 *   Candidates that end on the same (x, y, i) are ONE keypoint (their values are the same).
 *   Image units: xy = ((float)(px f), (float)(py f)), scale = (float)(s f) with f = 2^(o - 1) for octave o.
 *
 * Gradients on Gaussian layer L_i of the octave, at (xx, yy) with 0 < xx < W_o - 1, 0 < yy < H_o - 1 (other samples are
 * skipped):  gx = L(xx+1, yy) - L(xx-1, yy),  gy = L(xx, yy-1) - L(xx, yy+1)  (doubles),  mag = sqrt(gx gx + gy gy),
 * ori = det_atan2(gy, gx).
 *
 * ORIENTATION.  so = 1.5 s, rad = (int)floor(3 so + 0.5), e = -1 / (2 so so).  hist[36] = 0.  For dy = -rad .. rad (outer), dx =
 * -rad .. rad (inner), sample (x + dx, y + dy):  b = (int)floor(ori (36 / PI2) + 0.5), b += 36 if b < 0, b -= 36 if b >= 36;
 * hist[b] = hist[b] + det_exp((dx dx + dy dy) e) mag, in that sample order.
 *   smoothing (circular):  h[j] = ((hist[j-2] + hist[j+2]) (1/16) + (hist[j-1] + hist[j+1]) (4/16)) + hist[j] (6/16)
 *   peaks: m = max h.  For j = 0 .. 35 ascending, l = j - 1, r = j + 1 (circular): a peak if h[j] > h[l], h[j] > h[r] and
 *   h[j] >= 0.8 m;  bin = j + 0.5 (h[l] - h[r]) / ((h[l] - 2 h[j]) + h[r]),  bin += 36 if bin < 0, bin -= 36 if bin >= 36;
 *   theta = bin (PI2 / 36), radians in [0, PI2): angle = (float)theta.  One keypoint per peak (Lowe); j is the peak index.
 *
 * DESCRIPTOR.  hw = 3 s, rad = min((int)floor(hw 1.4142135623730951 2.5 + 0.5), (int)floor(sqrt(W_o W_o + H_o H_o))),
 * ct = det_cos(theta) / hw, st = det_sin(theta) / hw.  H[6][6][10] = 0.  For dy = -rad .. rad (outer), dx = -rad .. rad (inner):
 *   cr = dx ct - dy st,  rr = dx st + dy ct,  rb = rr + 1.5,  cb = cr + 1.5;  used if -1 < rb < 4, -1 < cb < 4 and the gradient
 *   sample (x + dx, y + dy) exists.  m = mag det_exp((cr cr + rr rr) (-0.125));  o = ori, o += PI2 if o < 0;
 *   ob = (o - theta) (8 / PI2);  r0 = floor(rb), c0 = floor(cb), o0 = floor(ob);  fr = rb - r0, fc = cb - c0, fo = ob - o0;
 *   o0 += 8 if o0 < 0, o0 -= 8 if o0 >= 8.
 *   v1 = m fr, v0 = m - v1;  v11 = v1 fc, v10 = v1 - v11;  v01 = v0 fc, v00 = v0 - v01;
 *   v111 = v11 fo, v110 = v11 - v111;  v101 = v10 fo, v100 = v10 - v101;  v011 = v01 fo, v010 = v01 - v011;
 *   v001 = v00 fo, v000 = v00 - v001.  With (R, C) = (r0 + 1, c0 + 1), added in THIS order, each sample after the one before it:
 *   H[R][C][o0] += v000, H[R][C][o0+1] += v001, H[R][C+1][o0] += v010, H[R][C+1][o0+1] += v011,
 *   H[R+1][C][o0] += v100, H[R+1][C][o0+1] += v101, H[R+1][C+1][o0] += v110, H[R+1][C+1][o0+1] += v111.
 *   One accumulator chain per keypoint: no floating-point atomics, no tree.  Then for i, j = 0 .. 3:
 *   H[i+1][j+1][0] += H[i+1][j+1][8], H[i+1][j+1][1] += H[i+1][j+1][9];  d[(4 i + j) 8 + k] = H[i+1][j+1][k], k = 0 .. 7.
 *   n2 = sum of d d ascending;  t = 0.2 sqrt(n2);  d = min(d, t);  n2' = sum of d d ascending;
 *   g = 512 / max(sqrt(n2'), 2^-52);  desc = (float)min(d g, 255)  -- the 0..255 scale of cv::SIFT's rows, not quantised.
 *
 * ORDER.  Keypoints are sorted by (octave, layer i, y, x, peak index j), the integers after the fit.  No atomic counter
 * decides the order. */
#ifndef PAIS_FEATURE_H
#define PAIS_FEATURE_H

#include "pais_seed.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pais_feature_params {
    int32_t layers;             /* 3    layers per octave, 1 .. 8            */
    int32_t _pad;
    double  sigma;              /* 1.6                                       */
    double  input_blur;         /* 0.5  assumed blur of the input            */
    double  contrast_threshold; /* 0.04                                      */
    double  edge_threshold;     /* 10                                        */
} pais_feature_params;

void pais_feature_default_params(pais_feature_params *prm);
size_t pais_sizeof_feature_params(void);

/* Detect and describe on HIP device `device`.  gray: height rows of width bytes, `stride` bytes apart (host pointer).  prm:
 * NULL means the defaults.  *num: the number of keypoints found; the first min(*num, max_keypoints) in ORDER are written:
 * xy (2 floats each, image pixels), scale (the Gaussian sigma of the keypoint in image pixels), angle (radians, [0, PI2)),
 * octave_layer (2 int32 each: octave -- 0 is the doubled image --, layer), desc (128 floats each).  Any output array may be
 * NULL when max_keypoints == 0.  *num > max_keypoints is not an error: call again with room for *num.
 * Refused with < 0 and nothing launched: a null pointer, device < 0 (there is no host path), width or height < 1, stride <
 * width, max_keypoints < 0, parameters that are not finite or not positive, layers outside 1 .. 8, a blur radius above 512.
 * An image too small for an octave, or a constant one, gives *num = 0.  kernel_ms (may be NULL): the kernel time of all stages, host
 * round trips between them left out.  height is at most 32767. */
int  pais_feature_detect(int device, const uint8_t *gray, int width, int height, int64_t stride,
                         const pais_feature_params *prm, int max_keypoints,
                         int32_t *num, float *xy, float *scale, float *angle, int32_t *octave_layer, float *desc,
                         double *kernel_ms);

/* FeatureManager::setSeedPatches(cameras, max_dist, mvs) whole: pais_feature_detect on every camera's level-0 image on the
 * driver's GPU, then pais_mvs_set_seed_patches with dim 128 and max_dist.  *num_seeds: seeds added. */
int  pais_mvs_seed_from_images(pais_mvs *m, double max_dist, const pais_feature_params *prm, int *num_seeds);

/* per-stage kernel time of the calling thread's last pais_feature_detect, ms: blur (doubling, halving, rows, columns),
 * extrema, fit, orientation, descriptor; and the bytes the blur kernels read and wrote */
void pais_feature_last_stage_ms(double ms[5], double *blur_bytes);

const char *pais_feature_last_error(void);
int64_t pais_feature_launches(void);

#ifdef __cplusplus
}
#endif
#endif
