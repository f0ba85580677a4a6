/* pais_undistort.h -- the radial term of an NVM camera taken out of images and measurements on the GPU.
 *
 * Every NVM camera line carries one radial-distortion coefficient.  The cost kernels, the setters, the seeds and reCentering
 * project through the ideal pinhole -- Camera::project's default applyDistortion = false, which the reference never
 * switches on (camera.cpp:138-160) -- so images and measurements have to be made ideal BEFORE Camera::Camera builds its
 * pyramid.  A device-level entry like pais_cloud_render: it takes a `device`, not a pais_ctx.  The result is defined by the
 * FP64 statements below and by nothing else.
 *
 * Two models, named by the direction in which the closed form G runs; each uses G for one of {images, points} and its
 * inverse for the other. */
#ifndef PAIS_UNDISTORT_H
#define PAIS_UNDISTORT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PAIS_LENS_MEASURED_TO_IDEAL 0   /* ideal = G_k(measured): the NVM radial term as VisualSFM defines it */
#define PAIS_LENS_IDEAL_TO_MEASURED 1   /* measured = G_k(ideal): Camera::project's applyDistortion branch, camera.cpp:149-154 */
#define PAIS_UNDISTORT_MAX_STEPS 64

typedef struct { double focal[2], pp[2], k; int model; } pais_lens;

/* Every product, sum and quotient below is rounded to double (no FMA); evaluation runs left to right, as written.
 * For a point (u, v) and a lens (f, pp, k):
 *     x = (u - pp0) / f0      y = (v - pp1) / f1      q = (x x) + (y y)
 * Forward G:
 *     r = k q                 t = 1.0 + r
 *     u' = ((t f0) x) + pp0   v' = ((t f1) y) + pp1
 *     valid iff q, t, u' and v' are finite and (3.0 k) q + 1.0 > 0: the monotone branch, beyond it the map folds over.
 * Inverse G^-1: the scale s with c s s s + s = 1, c = k q (no square root, no 0/0 at the centre pixel):
 *     s = 1; at most PAIS_UNDISTORT_MAX_STEPS times:
 *         s2 = s s            fv = ((c s2) s + s) - 1.0       d = (3.0 c) s2 + 1.0       sn = s - fv / d
 *         stop and keep s when c == 0, or c > 0 and sn >= s, or c < 0 and sn <= s; otherwise s = sn
 *     u' = ((s f0) x) + pp0   v' = ((s f1) y) + pp1
 *     valid iff c is finite, 27.0 c >= -4.0 (a real root on the monotone branch exists) and u' and v' are finite.
 *     In exact arithmetic Newton is monotone from s = 1 for both signs of c; the rule ends the sequence where rounding
 *     breaks the monotonicity.
 * An invalid point is returned as (NaN, NaN) with valid = 0.
 *
 *                          MEASURED_TO_IDEAL     IDEAL_TO_MEASURED
 *   pais_undistort_points  G                     G^-1
 *   pais_distort_points    G^-1                  G
 *   pais_undistort_image   G^-1 per pixel        G per pixel          (the source position of an ideal output pixel)
 *
 * All pointers are host pointers.  xy arrays are n x 2; valid is n bytes (0 / 1).
 * Refused (< 0, pais_undistort_last_error(), nothing launched): a null pointer, a negative count, device < 0, an unknown
 * model, a non-finite lens entry, focal == 0, a non-finite input point.  n == 0 is no error.
 * Points go in launches of bounded size; PAIS_UNDISTORT_POINTS (points per launch) overrides it and changes the time only.
 * kernel_ms (may be NULL): milliseconds from the first kernel to the last, without the copies. */
int pais_undistort_points(int device, const pais_lens *lens, int64_t n, const double *xy_measured, double *xy_ideal,
                          uint8_t *valid, double *kernel_ms);
int pais_distort_points(int device, const pais_lens *lens, int64_t n, const double *xy_ideal, double *xy_measured,
                        uint8_t *valid, double *kernel_ms);

/* The ideal image of a measured one.  src: height rows of width pixels of `channels` (1, or 3 interleaved) bytes, `stride`
 * bytes from row to row; dst: the same size, tight; mask: width x height bytes (1 valid, 0 not) or NULL.
 * For each integer output pixel (u, v): (sx, sy) = the ideal -> measured map of the model at (u, v).  The pixel is valid iff
 * the map is valid and 0 <= sx <= width - 1 and 0 <= sy <= height - 1.  Then
 *     x0 = floor(sx)   x1 = min(x0 + 1, width - 1)   a = sx - x0          y0, y1, b likewise from sy
 *     val = (((1 - a)(1 - b)) I(x0,y0) + (a (1 - b)) I(x1,y0)) + (((1 - a) b) I(x0,y1) + (a b) I(x1,y1))    per channel
 * rounded half to even into a byte.  An invalid pixel gets value 0 (every channel) and mask 0.
 * The output has the input's size, focal and principal point; only k becomes 0.
 * valid_pixels (may be NULL): the number of valid pixels.
 * Refused as above, and: channels other than 1 or 3, width or height < 1 (or width x height >= 2^31),
 * stride < width x channels.
 * Rows go in launches of bounded size; PAIS_UNDISTORT_ROWS (rows per launch, rounded up to whole tiles) overrides it and
 * changes the time only, never a byte of the output. */
int pais_undistort_image(int device, const pais_lens *lens, int channels, const uint8_t *src, int width, int height,
                         int64_t stride, uint8_t *dst, uint8_t *mask, int64_t *valid_pixels, double *kernel_ms);

/* Kernels launched by this process so far (tests: a refused call launches nothing). */
int64_t pais_undistort_launches(void);

const char *pais_undistort_last_error(void);

size_t pais_sizeof_lens(void);

#ifdef __cplusplus
}
#endif
#endif /* PAIS_UNDISTORT_H */
