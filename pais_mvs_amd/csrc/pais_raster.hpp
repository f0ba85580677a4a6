// pais_raster.hpp -- the lane-local arithmetic of pais_mesh_render (include/pais_render.h, TRIANGLE): the statements of the
// header written once, inlined into k_tri_setup and the two triangle walks of pais_render.hip and compiled for the host by
// tests/raster_host_shim.cpp.  Both builds use -ffp-contract=off, so every product, sum and quotient is rounded to double on
// its own; only + - x / and comparisons are used.  No array is indexed dynamically: on the GPU everything stays in registers.
#pragma once
#include <math.h>
#include <stdint.h>
#include "../../include/pais_render.h"
#include "pais_dev.hpp"

namespace pais {

enum { RASTER_LIVE = 0, RASTER_BEHIND = 1, RASTER_REPEATED = 2, RASTER_CULLED = 3, RASTER_FLAT = 4, RASTER_OFF_IMAGE = 5 };

// One (triangle, view) pair: the signed N of the edges (b,c), (c,a), (a,b) -- they give w_a, w_b, w_c -- and D.
struct RasterTri {
    double ma[3], mb[3], mc[3], D;
};

// P' = (R P) + T, the renderer's statement.
PAIS_HD void raster_camera(const pais_view &V, const double *c, double *cc)
{
    cc[0] = ((V.R[0] * c[0] + V.R[1] * c[1]) + V.R[2] * c[2]) + V.T[0];
    cc[1] = ((V.R[3] * c[0] + V.R[4] * c[1]) + V.R[5] * c[2]) + V.T[1];
    cc[2] = ((V.R[6] * c[0] + V.R[7] * c[1]) + V.R[8] * c[2]) + V.T[2];
}

// The signed N of the edge the triangle walks p -> q (vertex indices; P, Q their camera-space positions): N = P'lo x P'hi
// with lo = min(p, q), negated when the walk is hi -> lo.  The triangle on the other side of the edge walks it the other
// way round and so gets exactly the negated components; every later operation commutes with that negation.
PAIS_HD void raster_edge(int p, int q, const double *P, const double *Q, double *m)
{
    const bool fwd = p < q;
    const double *lo = fwd ? P : Q, *hi = fwd ? Q : P;
    const double n0 = lo[1] * hi[2] - lo[2] * hi[1];
    const double n1 = lo[2] * hi[0] - lo[0] * hi[2];
    const double n2 = lo[0] * hi[1] - lo[1] * hi[0];
    m[0] = fwd ? n0 : -n0;
    m[1] = fwd ? n1 : -n1;
    m[2] = fwd ? n2 : -n2;
}

// The record of triangle (a, b, c) with camera-space corners A, B, C.
PAIS_HD void raster_setup(int a, int b, int c, const double *A, const double *B, const double *C, RasterTri *t)
{
    raster_edge(b, c, B, C, t->ma);
    raster_edge(c, a, C, A, t->mb);
    raster_edge(a, b, A, B, t->mc);
    t->D = ((A[0] * t->ma[0]) + (A[1] * t->ma[1])) + A[2] * t->ma[2];
}

// The skips of the header (RASTER_FLAT: D == 0 gives t == 0 or NaN at every pixel, so nothing is ever covered).
PAIS_HD int raster_skip(int flags, int a, int b, int c, double az, double bz, double cz, double D)
{
    if (!(az > 0.0 || bz > 0.0 || cz > 0.0)) return RASTER_BEHIND;
    if (a == b || b == c || a == c) return RASTER_REPEATED;
    if ((flags & PAIS_RENDER_CULL_BACK) && D >= 0.0) return RASTER_CULLED;
    if (D == 0.0) return RASTER_FLAT;
    return RASTER_LIVE;
}

// The TRIANGLE statements for pixel (u, v): covered or not, and the depth t.
PAIS_HD bool raster_hit(const RasterTri &T, double f0, double f1, double pp0, double pp1, int u, int v, double *tOut)
{
    const double rx = ((double)u - pp0) / f0, ry = ((double)v - pp1) / f1;
    const double wa = ((T.ma[0] * rx) + (T.ma[1] * ry)) + T.ma[2];
    const double wb = ((T.mb[0] * rx) + (T.mb[1] * ry)) + T.mb[2];
    const double wc = ((T.mc[0] * rx) + (T.mc[1] * ry)) + T.mc[2];
    const double S = (wa + wb) + wc;
    const double t = T.D / S;
    *tOut = t;
    const bool inside = (wa >= 0.0 && wb >= 0.0 && wc >= 0.0) || (wa <= 0.0 && wb <= 0.0 && wc <= 0.0);
    return inside && isfinite(t) && t > 0.0;
}

// One axis of the pixel box: [lo, hi] from the three projections p, clipped to [0, size - 1]; false: none of the axis.
PAIS_HD bool raster_box_axis(double p0, double p1, double p2, double pp, int size, int *lo, int *hi)
{
    double a = fmin(p0, fmin(p1, p2)), b = fmax(p0, fmax(p1, p2));
    *lo = 0;
    *hi = size - 1;
    if (!(isfinite(a) && isfinite(b))) return true;
    const double pad = 1.0 + 0x1p-10 * (b - a) + 0x1p-20 * fmax(fabs(a - pp), fabs(b - pp));
    a = floor(a - pad);
    b = ceil(b + pad);
    if (!(isfinite(a) && isfinite(b))) return true;
    if (b < 0.0 || a > (double)(size - 1)) return false;
    if (a > 0.0) *lo = (int)a;
    if (b < (double)(size - 1)) *hi = (int)b;
    return true;
}

// A conservative pixel box [u0, u1] x [v0, v1] of a live triangle; false: it lies off the image.  Not part of the definition:
// the box only ever removes pixels the statements leave uncovered.  With a corner on or behind the camera plane, or with
// D D < 2^-80 (A'A')(B'B')(C'C') (the corner rays almost in one plane: edge-on, or no larger than 2^-20 of its distance), it
// is the whole image.  Otherwise all corners lie in front: in exact arithmetic a covered ray meets the triangle, which lies
// in z > 0, so its pixel lies in the hull of the three projections.  Rounding turns the plane of an edge by at most
// 2^-51 / sin(angle of its two corner rays) and the evaluation of w by 2^-51 more; D = |A'||B'||C'| sin sin sin (two edge
// angles and the corner angle between them) with the bound above keeps the overshoot past a corner below 2^-11 of the edge
// itself.  The box is taken 2^-10 of its extent, 2^-20 of its distance from the principal point and one pixel wider.
PAIS_HD bool raster_box(const pais_view &V, const double *A, const double *B, const double *C, double D, int W, int H, int *u0, int *u1,
                        int *v0, int *v1)
{
    *u0 = 0; *u1 = W - 1; *v0 = 0; *v1 = H - 1;
    if (!(A[2] > 0.0 && B[2] > 0.0 && C[2] > 0.0)) return true;
    const double a2 = ((A[0] * A[0]) + (A[1] * A[1])) + A[2] * A[2];
    const double b2 = ((B[0] * B[0]) + (B[1] * B[1])) + B[2] * B[2];
    const double c2 = ((C[0] * C[0]) + (C[1] * C[1])) + C[2] * C[2];
    if (!(D * D >= ((0x1p-80 * a2) * b2) * c2)) return true;
    bool any = raster_box_axis(V.focal[0] * (A[0] / A[2]) + V.pp[0], V.focal[0] * (B[0] / B[2]) + V.pp[0], V.focal[0] * (C[0] / C[2]) + V.pp[0],
                               V.pp[0], W, u0, u1);
    any = raster_box_axis(V.focal[1] * (A[1] / A[2]) + V.pp[1], V.focal[1] * (B[1] / B[2]) + V.pp[1], V.focal[1] * (C[1] / C[2]) + V.pp[1],
                          V.pp[1], H, v0, v1) && any;
    return any;
}

} // namespace pais
