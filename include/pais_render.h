/* pais_render.h -- a cloud rendered into pinhole views: z-buffered patch splats on the GPU.
 *
 * The reference's only way of checking a result is looking at it (the `-v` / `-a` verbs, view/mvsviewer.cpp; SURVEY section
 * 4).  This project is headless, so the product is a renderer: per view a depth map and a patch-id map, from which colour
 * images, normal maps, picking (pointPickEvent -> printPatchInformation, mvsviewer.cpp:75-87, 441-471), orbit frames and the
 * animate sequence are built on the host (pais_mvs_amd/render.py, python -m pais_mvs_amd.view).
 * A device-level entry like pais_cloud_nearest: it takes a `device`, not a pais_ctx, and needs no images.  The result is
 * defined by the FP64 statements below and by nothing else. */
#ifndef PAIS_RENDER_H
#define PAIS_RENDER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* A pinhole view: X' = R X + T (R row-major), u = focal[0] X'0 / X'2 + pp[0], v likewise -- Camera::project
 * (camera.cpp:141-157). */
typedef struct { double R[9], T[3], focal[2], pp[2]; } pais_view;

#define PAIS_RENDER_DISC       0   /* oriented disc of world radius rho in the patch plane */
#define PAIS_RENDER_POINT      1   /* screen-space square of `size` pixels: the viewer's pointSize */
#define PAIS_RENDER_CULL_BACK  1   /* flag: skip splats whose normal faces away from the view */

#define PAIS_RENDER_MAX_POINT_SIZE 64

/* Splats n (centers n x 3, normals n x 3, radii n or NULL) into num_views views of width x height pixels.
 * All pointers are host pointers; depth and id are num_views x height x width, row-major.
 *
 * Every product, sum and quotient below is rounded to double (no FMA); sums are evaluated left to right.
 * Per splat i (centre c, normal n) and view (R, T, f, pp), in camera space:
 *     c'k = ((R[3k] c0 + R[3k+1] c1) + R[3k+2] c2) + T[k]          n'k = (R[3k] n0 + R[3k+1] n1) + R[3k+2] n2
 *     a   = (n'0 c'0 + n'1 c'1) + n'2 c'2
 * DISC:  rho = radii ? radii[i] : radius.  The splat is skipped unless c'2 > rho (its bounding sphere reaches the camera
 *     plane or lies behind it), and with PAIS_RENDER_CULL_BACK when a >= 0.  For the integer pixel (u, v), sampled at the
 *     integer coordinate like every image access of this library:
 *         rx = (u - pp0) / f0      ry = (v - pp1) / f1
 *         den = (n'0 rx + n'1 ry) + n'2
 *         t = a / den
 *         hx = t rx - c'0          hy = t ry - c'1          hz = t - c'2
 *         d2 = ((hx hx) + (hy hy)) + (hz hz)
 *     The pixel is covered iff den != 0, t is finite, t > 0 and d2 <= rho rho.  Its depth is t: the ray (rx, ry, 1) has
 *     camera-z 1, so t is the camera-space z of the hit.
 * POINT: s = (int)radius, 1 <= s <= PAIS_RENDER_MAX_POINT_SIZE.  The splat is skipped unless c'2 > 0.
 *         pu = f0 (c'0 / c'2) + pp0      pv = f1 (c'1 / c'2) + pp1          (project_raw at scale 1)
 *     It is skipped when pu or pv is not finite or of magnitude >= 2^30.  ru = cvRound(pu), rv = cvRound(pv) (half to
 *     even).  Covered: u in [ru - (s-1)/2, ru + s/2] and v in [rv - (s-1)/2, rv + s/2] (integer division), clipped to the
 *     image.  The depth is c'2.  normals may be NULL; flags are not read.
 * Z-buffer: depth[p] = the minimum depth over all splats covering p, id[p] = the LOWEST splat index that attains it (the
 *     tie rule of pais_cloud_nearest); a pixel no splat covers holds +inf and -1.  So the result does not depend on the
 *     launch order, on any bounding box or on how the work is split.
 *
 * Refused (< 0, pais_render_last_error(), nothing launched): a negative count, a null pointer, device < 0, width or height
 * < 1 (or width x height >= 2^31), an unknown mode, a non-finite centre, normal (DISC), radius or view entry, rho <= 0,
 * focal == 0, DISC without normals, a POINT size out of range.  n == 0 or num_views == 0 is no error: the buffers are
 * filled with +inf / -1.
 * Views are rendered in passes when num_views x height x width exceeds an internal cap, splats in launches of bounded
 * size; PAIS_RENDER_VIEWS (views per pass) and PAIS_RENDER_SPLATS (splats per launch) override both and change the time
 * only, never a byte of the output.
 * kernel_ms (may be NULL): milliseconds from the first kernel to the last, without the copies. */
int pais_cloud_render(int device, int mode, int flags,
                      int n, const double *centers, const double *normals,
                      const double *radii, double radius,
                      int num_views, const pais_view *views, int width, int height,
                      double *depth, int32_t *id, double *kernel_ms);

/* Counters of the last successful pais_cloud_render of this thread (any may be NULL): footprint tiles walked by the depth
 * pass, covered (pixel, splat) pairs it found, depth atomics it issued (the rest lost against the value already there),
 * id atomics issued by the second pass. */
void pais_render_last_counts(int64_t *tiles, int64_t *covered_pairs, int64_t *depth_atomics, int64_t *id_atomics);

/* Kernels launched by this process so far (tests: a refused call launches nothing). */
int64_t pais_render_launches(void);

const char *pais_render_last_error(void);

size_t pais_sizeof_view(void);

/* ---- depth test: does a point, in a view, lie on the surface the view sees, behind it, or in front of it? -------------- */
#define PAIS_VIS_VISIBLE   0   /* within tol of the depth map at its pixel (or, with PAIS_VIS_SELF, its own disc is there) */
#define PAIS_VIS_OCCLUDED  1   /* more than tol behind the depth map */
#define PAIS_VIS_IN_FRONT  2   /* more than tol in front of it */
#define PAIS_VIS_EMPTY     3   /* its pixel holds +inf: the view sees nothing there */
#define PAIS_VIS_OUTSIDE   4   /* it projects outside the image (or not to a finite pixel) */
#define PAIS_VIS_BEHIND    5   /* it lies on or behind the camera plane */
#define PAIS_VIS_SELF  0x100   /* flag: point i is splat i; a pixel whose id is i makes the pair VISIBLE.  Shares the flags
                                * word with PAIS_RENDER_CULL_BACK. */

/* Tests n points against num_views depth maps (and id maps, or id == NULL) of width x height pixels, as pais_cloud_render
 * writes them: num_views x height x width, row-major.  All pointers are host pointers; the maps are the caller's -- rendered
 * earlier, composited, or from elsewhere.
 *
 * Every product, sum and quotient below is rounded to double (no FMA); sums are evaluated left to right.
 * For point c (index i), view (R, T, f, pp), maps D and I of the view, and tol >= 0:
 *     c'k = ((R[3k] c0 + R[3k+1] c1) + R[3k+2] c2) + T[k]                   (the renderer's statement)
 *     c'2 <= 0 (or not > 0)                                 -> PAIS_VIS_BEHIND
 *     pu = f0 (c'0 / c'2) + pp0     pv = f1 (c'1 / c'2) + pp1               (POINT mode's project)
 *     pu or pv not finite, or of magnitude >= 2^30          -> PAIS_VIS_OUTSIDE
 *     ru = cvRound(pu), rv = cvRound(pv) (half to even);  outside [0,W) x [0,H) -> PAIS_VIS_OUTSIDE
 *     d = D[rv][ru];   d == +inf                            -> PAIS_VIS_EMPTY
 *     m = c'2 - d
 *     with PAIS_VIS_SELF and I[rv][ru] == i                 -> PAIS_VIS_VISIBLE   (its own disc is the nearest surface)
 *     m >  tol                                              -> PAIS_VIS_OCCLUDED
 *     m < -tol                                              -> PAIS_VIS_IN_FRONT
 *     else                                                  -> PAIS_VIS_VISIBLE    (m == tol and m == -tol are VISIBLE)
 * Outputs are view-major, [v * n + i]: code (uint8); occluder (int32, may be NULL): I[rv][ru] for codes 0..2, else -1, and
 * -1 throughout when id == NULL; margin (double, may be NULL): m for codes 0..2, else NaN.
 *
 * Refused (< 0, pais_render_last_error(), nothing launched): what pais_cloud_render refuses about counts, sizes, views and
 * device < 0; a non-finite point; a NaN in depth (+inf is the empty pixel, anything else is compared as it is); tol negative
 * or not finite; flag bits other than PAIS_VIS_SELF; PAIS_VIS_SELF without id; a null points, views, depth or code.
 * n == 0 or num_views == 0 returns 0 and touches nothing.
 * Views go in passes under the renderer's pixel cap (PAIS_RENDER_VIEWS overrides), points in launches of bounded size
 * (2^20 points, no override): neither changes a byte.
 * kernel_ms (may be NULL): the kernels' milliseconds, without the copies. */
int pais_depth_test(int device, int flags, int n, const double *points,
                    int num_views, const pais_view *views, int width, int height,
                    const double *depth, const int32_t *id, double tol,
                    uint8_t *code, int32_t *occluder, double *margin, double *kernel_ms);

/* pais_cloud_render of the n splats (mode, flags & PAIS_RENDER_CULL_BACK, centers, normals, radii, radius: exactly as
 * there) and pais_depth_test of the nq queries against each pass of views while its maps are still on the device.
 * code / occluder / margin: num_views x nq, as above.  depth and id are both given or both NULL: given, they receive
 * pais_cloud_render's output byte for byte; NULL, the maps are never copied to the host.
 * PAIS_VIS_SELF requires nq == n, and query i is then splat i.
 * Refused: what pais_cloud_render and pais_depth_test refuse (flag bits other than PAIS_RENDER_CULL_BACK | PAIS_VIS_SELF
 * included), under this entry's name.  num_views == 0 returns 0 and touches nothing; nq == 0 renders (when depth is given)
 * and tests nothing.
 * kernel_ms (may be NULL): render and test kernels together; pais_cloud_visibility_last_ms splits them.
 * pais_render_last_counts then describes this call's render. */
int pais_cloud_visibility(int device, int mode, int flags,
                          int n, const double *centers, const double *normals,
                          const double *radii, double radius,
                          int nq, const double *queries,
                          int num_views, const pais_view *views, int width, int height, double tol,
                          uint8_t *code, int32_t *occluder, double *margin,
                          double *depth, int32_t *id, double *kernel_ms);

/* {render, test} kernel milliseconds of this thread's last pais_cloud_visibility. */
void pais_cloud_visibility_last_ms(double ms[2]);

/* ---- triangles: an indexed mesh (pais_mesh_weld's output, or any other) rendered into the same views ------------------- */

/* Triangles nt (index triples into vertices nv x 3) into num_views views; depth and id as pais_cloud_render writes them,
 * id = the triangle's index.  The statements are written once in pais_mvs_amd/csrc/pais_raster.hpp.
 *
 * Every product, sum, difference and quotient below is rounded to double (no FMA); sums are evaluated left to right; only
 * + - x / and comparisons are used.
 * Per vertex P and view:   P'k = ((R[3k] P0 + R[3k+1] P1) + R[3k+2] P2) + T[k]                (the renderer's statement)
 * TRIANGLE (a, b, c) (vertex indices; A', B', C' their camera-space positions):
 *     Per edge walked p -> q, with lo = min(p, q), hi = max(p, q) by vertex INDEX:
 *         N = P'lo x P'hi:   N0 = lo1 hi2 - lo2 hi1     N1 = lo2 hi0 - lo0 hi2     N2 = lo0 hi1 - lo1 hi0
 *         M = N when p < q, else -N (each component negated, which is exact)
 *     Ma from edge (b, c), Mb from (c, a), Mc from (a, b).  For the integer pixel (u, v):
 *         rx = (u - pp0) / f0      ry = (v - pp1) / f1
 *         w_a = ((Ma0 rx) + (Ma1 ry)) + Ma2        w_b, w_c likewise from Mb, Mc
 *         D = ((A'0 Ma0) + (A'1 Ma1)) + A'2 Ma2
 *         S = (w_a + w_b) + w_c                    t = D / S
 *     The pixel is covered iff w_a, w_b, w_c are all >= 0 or all <= 0, t is finite and t > 0.  Its depth is t: with
 *     r = (rx, ry, 1), t r = (w_a A' + w_b B' + w_c C') / S is the point of the triangle's plane on the ray, and r has
 *     camera-z 1 -- the depth convention of DISC.
 *     Shared edges: the triangle on the other side of an edge walks it q -> p and gets -M exactly; rounding to nearest is
 *     symmetric, so its w for that edge is the negated w of this one, bit for bit (up to the sign of a zero, which no
 *     comparison reads and which leaves S unchanged unless S is itself zero, where t is not finite).  Edges are inclusive: a
 *     pixel centre on a shared edge is covered by both neighbours and the z-buffer's tie rule decides; no pixel is lost
 *     between them through the rounding of that edge.
 *     No clipping: a triangle that crosses the camera plane contributes exactly its part with t > 0.
 *     Skipped for a view: no corner with P'2 > 0; two equal indices; with PAIS_RENDER_CULL_BACK when D >= 0 (the mesher orients
 *     (B - A) x (C - A) outward, so a front face has D < 0).  D == 0 gives t == 0 or NaN, so such a triangle covers nothing.
 * Z-buffer: as above -- the minimum t, the LOWEST triangle index among equal bits, +inf / -1 where nothing covers; the result
 *     does not depend on the launch order, on any bounding box, on the walk a triangle takes or on how the work is split.
 *
 * Refused (< 0, pais_render_last_error(), nothing launched): what pais_cloud_render refuses about counts, sizes, views and
 * device; a null pointer; a non-finite vertex; an index outside [0, nv); flag bits other than PAIS_RENDER_CULL_BACK.
 * nt == 0 or num_views == 0 is no error: the buffers are filled with +inf / -1.
 * PAIS_RENDER_VIEWS (views per pass) and PAIS_RENDER_SPLATS (here: triangles per launch) change the time only.
 * pais_render_last_counts describes this render too: tiles of the boxes that took the tile walk; pais_render_last_packed the
 * (triangle, view) pairs whose small box took the packed walk (0 after a cloud render). */
int pais_mesh_render(int device, int flags,
                     int nv, const double *vertices, int nt, const int32_t *triangles,
                     int num_views, const pais_view *views, int width, int height,
                     double *depth, int32_t *id, double *kernel_ms);

int64_t pais_render_last_packed(void);

/* {setup, depth phase, id phase} kernel milliseconds of this thread's last pais_mesh_render / pais_mesh_visibility. */
void pais_mesh_render_last_ms(double ms[3]);

/* pais_mesh_render of the mesh (flags & PAIS_RENDER_CULL_BACK) and pais_depth_test of the nq queries against each pass of
 * views while its maps are still on the device: the counterpart of pais_cloud_visibility, with occluder = the triangle at
 * the query's pixel.  depth and id are both given or both NULL: given, they receive pais_mesh_render's output byte for byte;
 * NULL, the maps are never copied to the host.
 * Refused: what pais_mesh_render and pais_depth_test refuse, under this entry's name, and PAIS_VIS_SELF (a query is not a
 * triangle).  num_views == 0 returns 0 and touches nothing; nq == 0 renders (when depth is given) and tests nothing.
 * kernel_ms (may be NULL): render and test kernels together; pais_cloud_visibility_last_ms splits them. */
int pais_mesh_visibility(int device, int flags,
                         int nv, const double *vertices, int nt, const int32_t *triangles,
                         int nq, const double *queries,
                         int num_views, const pais_view *views, int width, int height, double tol,
                         uint8_t *code, int32_t *occluder, double *margin,
                         double *depth, int32_t *id, double *kernel_ms);

/* The occlusion count of MVS::visibilityFiltering (mvs.cpp:399-446) with the z-buffer in place of the cell lists; host only.
 * code: num_views x n as above; the camera list of point i is cams[offsets[i] .. offsets[i+1]), entries that index views.
 *     visible[i] = (offsets[i+1] - offsets[i]) - #{ j : code[cams[j] * n + i] == PAIS_VIS_OCCLUDED }
 *     outlier[i] = visible[i] < min_visible
 * Only OCCLUDED subtracts: EMPTY, OUTSIDE, BEHIND and IN_FRONT say nothing about an occluder.
 * Refused (< 0, pais_render_last_error()): a negative count, a null pointer when n > 0 (cams may be NULL when every list is
 * empty), offsets[0] != 0 or offsets that decrease, a camera index outside [0, num_views). */
int pais_cloud_visibility_rule(int n, int num_views, const uint8_t *code, const int32_t *offsets, const int32_t *cams,
                               int min_visible, int32_t *visible, uint8_t *outlier);

#ifdef __cplusplus
}
#endif
#endif /* PAIS_RENDER_H */
