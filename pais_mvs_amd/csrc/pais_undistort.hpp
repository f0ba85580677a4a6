// pais_undistort.hpp -- the lane-local arithmetic of include/pais_undistort.h: the statements of the header written once,
// inlined into the kernels of pais_undistort.hip and compiled for the host by tests/undistort_host_shim.cpp.  Both builds
// use -ffp-contract=off, so every product, sum and quotient is rounded to double on its own.
#pragma once
#include <math.h>
#include <stdint.h>
#include "../../include/pais_undistort.h"
#include "pais_dev.hpp"

namespace pais {

struct LensPoint {
    double u, v;
    int ok, steps; // steps: Newton steps taken by the inverse (0 for the forward map)
};

PAIS_HD bool lens_finite(double a) { return (a - a) == 0.0; }

// Forward G.
PAIS_HD LensPoint lens_forward(const pais_lens &L, double u, double v)
{
    const double x = (u - L.pp[0]) / L.focal[0], y = (v - L.pp[1]) / L.focal[1];
    const double q = (x * x) + (y * y);
    const double r = L.k * q, t = 1.0 + r;
    LensPoint o;
    o.u = ((t * L.focal[0]) * x) + L.pp[0];
    o.v = ((t * L.focal[1]) * y) + L.pp[1];
    o.steps = 0;
    o.ok = lens_finite(q) && lens_finite(t) && lens_finite(o.u) && lens_finite(o.v) && ((3.0 * L.k) * q + 1.0 > 0.0);
    return o;
}

// Inverse G^-1: Newton on c s^3 + s = 1 from s = 1, ended where rounding breaks its monotonicity.
PAIS_HD LensPoint lens_inverse(const pais_lens &L, double u, double v)
{
    const double x = (u - L.pp[0]) / L.focal[0], y = (v - L.pp[1]) / L.focal[1];
    const double q = (x * x) + (y * y);
    const double c = L.k * q;
    LensPoint o;
    o.steps = 0;
    o.ok = lens_finite(c) && (27.0 * c >= -4.0);
    double s = 1.0;
    if (o.ok) {
        for (int it = 0; it < PAIS_UNDISTORT_MAX_STEPS; ++it) {
            const double s2 = s * s;
            const double fv = ((c * s2) * s + s) - 1.0;
            const double d = (3.0 * c) * s2 + 1.0;
            const double sn = s - fv / d;
            o.steps = it + 1;
            if (c == 0.0 || (c > 0.0 && sn >= s) || (c < 0.0 && sn <= s)) break;
            s = sn;
        }
    }
    o.u = ((s * L.focal[0]) * x) + L.pp[0];
    o.v = ((s * L.focal[1]) * y) + L.pp[1];
    o.ok = o.ok && lens_finite(o.u) && lens_finite(o.v);
    return o;
}

// The table of the header: which of G, G^-1 a call uses.
enum { LENS_UNDISTORT_POINTS = 0, LENS_DISTORT_POINTS = 1, LENS_IMAGE = 2 };
PAIS_HD bool lens_uses_inverse(int model, int what)
{
    const bool towardsMeasured = what != LENS_UNDISTORT_POINTS;
    return (model == PAIS_LENS_MEASURED_TO_IDEAL) == towardsMeasured;
}

PAIS_HD LensPoint lens_map(const pais_lens &L, bool inverse, double u, double v)
{
    LensPoint o = inverse ? lens_inverse(L, u, v) : lens_forward(L, u, v);
    if (!o.ok) o.u = o.v = NAN;
    return o;
}

// The four taps of one output pixel and their weights.
struct LensTap {
    int x0, x1, y0, y1, ok;
    double w00, w01, w10, w11;
};

PAIS_HD LensTap lens_tap(const pais_lens &L, bool inverse, int W, int H, int u, int v)
{
    const LensPoint p = lens_map(L, inverse, (double)u, (double)v);
    LensTap t;
    t.ok = p.ok && p.u >= 0.0 && p.u <= (double)(W - 1) && p.v >= 0.0 && p.v <= (double)(H - 1);
    t.x0 = t.x1 = t.y0 = t.y1 = 0;
    t.w00 = t.w01 = t.w10 = t.w11 = 0.0;
    if (!t.ok) return t;
    const double fx = floor(p.u), fy = floor(p.v);
    t.x0 = (int)fx;
    t.y0 = (int)fy;
    t.x1 = t.x0 + 1 < W - 1 ? t.x0 + 1 : W - 1;
    t.y1 = t.y0 + 1 < H - 1 ? t.y0 + 1 : H - 1;
    const double a = p.u - fx, b = p.v - fy;
    const double a1 = 1.0 - a, b1 = 1.0 - b;
    t.w00 = a1 * b1;
    t.w01 = a * b1;
    t.w10 = a1 * b;
    t.w11 = a * b;
    return t;
}

// val of the header for one channel, rounded half to even: the weights are in [0, 1] and sum to 1 within rounding, so the
// value lies in [0, 255 + 1e-12] and rint() of it fits a byte.
PAIS_HD uint8_t lens_blend(const LensTap &t, uint8_t i00, uint8_t i01, uint8_t i10, uint8_t i11)
{
    const double val = ((t.w00 * (double)i00) + (t.w01 * (double)i01)) + ((t.w10 * (double)i10) + (t.w11 * (double)i11));
    const double r = rint(val);
    return (uint8_t)(r > 255.0 ? 255 : (int)r);
}

} // namespace pais
