// pais_plane.hpp -- the lane-local arithmetic of pais_cloud_planes (include/pais_cloud.h): the statements of the header
// written once, inlined into k_cloud_planes (pais_cloud.hip) and compiled for the host by tests/plane_host_shim.cpp.  Both
// builds use -ffp-contract=off, so every product, sum and quotient is rounded to double on its own.
// The symmetric matrix is six named scalars and V nine, every index static: on the GPU all of it stays in registers.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>
#include "../../include/pais_cloud.h"
#include "pais_dev.hpp"

namespace pais {

// One pair (p, q) of a sweep: app, aqq, apq the pair's entries, arp, arq those of the third row, (v0p, v0q) .. (v2p, v2q)
// the columns p and q of V.  Returns whether it rotated.
PAIS_HD bool plane_rotate(double &app, double &aqq, double &apq, double &arp, double &arq, double &v0p, double &v0q, double &v1p,
                          double &v1q, double &v2p, double &v2q)
{
    const double g = apq;
    if (g == 0.0) return false;
    if (fabs(g) <= DBL_EPSILON * sqrt(fabs(app) * fabs(aqq))) {
        apq = 0.0;
        return false;
    }
    const double zeta = (aqq - app) / (2.0 * g);
    const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
    const double h = t * g;
    app = app - h;
    aqq = aqq + h;
    apq = 0.0;
    double x = arp, y = arq;
    arp = c * x - s * y;
    arq = s * x + c * y;
    x = v0p, y = v0q;
    v0p = c * x - s * y;
    v0q = s * x + c * y;
    x = v1p, y = v1q;
    v1p = c * x - s * y;
    v1q = s * x + c * y;
    x = v2p, y = v2q;
    v2p = c * x - s * y;
    v2q = s * x + c * y;
    return true;
}

// (eigenvalue, column) pairs a and b in order under `<`: the step of a stable insertion sort
PAIS_HD void plane_order(double &ea, double (&va)[3], double &eb, double (&vb)[3])
{
    if (eb < ea) {
        double x = ea;
        ea = eb;
        eb = x;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            x = va[j];
            va[j] = vb[j];
            vb[j] = x;
        }
    }
}

// The record of one query.  row[j], j < k: its row of the neighbourhood table; targets nt x 3; toward: the query's three
// components or nullptr.  *sweeps (may be nullptr): the sweeps that rotated.
PAIS_HD pais_plane plane_fit(bool withQuery, double qx, double qy, double qz, int k, const int32_t *row, int nt,
                             const double *targets, const double *toward, int *sweeps)
{
    pais_plane P;
#pragma unroll
    for (int j = 0; j < 3; ++j) P.centroid[j] = P.normal[j] = P.eigen[j] = 0.0;
    P.offset = P.variation = 0.0;
    if (sweeps) *sweeps = 0;
    int m = withQuery ? 1 : 0;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    if (withQuery) {
        sx += qx;
        sy += qy;
        sz += qz;
    }
    for (int j = 0; j < k; ++j) {
        const int32_t t = row[j];
        if (t < 0 || t >= nt) continue;
        sx += targets[3 * (size_t)t];
        sy += targets[3 * (size_t)t + 1];
        sz += targets[3 * (size_t)t + 2];
        ++m;
    }
    P.count = m;
    P.status = m < 3 ? PAIS_PLANE_FEW : PAIS_PLANE_OK;
    if (m < 3) return P;
    const double cx = sx / (double)m, cy = sy / (double)m, cz = sz / (double)m;
    double xx = 0.0, xy = 0.0, xz = 0.0, yy = 0.0, yz = 0.0, zz = 0.0;
    if (withQuery) {
        const double dx = qx - cx, dy = qy - cy, dz = qz - cz;
        xx += dx * dx;
        xy += dx * dy;
        xz += dx * dz;
        yy += dy * dy;
        yz += dy * dz;
        zz += dz * dz;
    }
    for (int j = 0; j < k; ++j) {
        const int32_t t = row[j];
        if (t < 0 || t >= nt) continue;
        const double dx = targets[3 * (size_t)t] - cx, dy = targets[3 * (size_t)t + 1] - cy, dz = targets[3 * (size_t)t + 2] - cz;
        xx += dx * dx;
        xy += dx * dy;
        xz += dx * dz;
        yy += dy * dy;
        yz += dy * dz;
        zz += dz * dz;
    }
    double a00 = xx / (double)m, a01 = xy / (double)m, a02 = xz / (double)m, a11 = yy / (double)m, a12 = yz / (double)m, a22 = zz / (double)m;
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
    bool converged = false;
    int rotating = 0;
    for (int sweep = 0; sweep < PAIS_PLANE_SWEEPS; ++sweep) {
        bool rotated = plane_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);      // (0,1), third row 2
        rotated = plane_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22) || rotated; // (0,2), third row 1
        rotated = plane_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22) || rotated; // (1,2), third row 0
        if (!rotated) {
            converged = true;
            break;
        }
        ++rotating;
    }
    if (sweeps) *sweeps = rotating;
    if (!converged) P.status = PAIS_PLANE_NOCONV;
    double e0 = a00, e1 = a11, e2 = a22;
    double c0[3] = {v00, v10, v20}, c1[3] = {v01, v11, v21}, c2[3] = {v02, v12, v22};
    plane_order(e0, c0, e1, c1);
    plane_order(e1, c1, e2, c2);
    plane_order(e0, c0, e1, c1);
    double nx = c0[0], ny = c0[1], nz = c0[2];
    bool flip;
    if (toward) {
        flip = ((nx * toward[0]) + (ny * toward[1])) + (nz * toward[2]) < 0.0;
    } else {
        double big = nx;
        if (fabs(ny) > fabs(big)) big = ny;
        if (fabs(nz) > fabs(big)) big = nz;
        flip = big < 0.0;
    }
    if (flip) {
        nx = -nx;
        ny = -ny;
        nz = -nz;
    }
    P.centroid[0] = cx;
    P.centroid[1] = cy;
    P.centroid[2] = cz;
    P.normal[0] = nx;
    P.normal[1] = ny;
    P.normal[2] = nz;
    P.eigen[0] = e0;
    P.eigen[1] = e1;
    P.eigen[2] = e2;
    P.offset = ((nx * (qx - cx)) + (ny * (qy - cy))) + (nz * (qz - cz));
    P.variation = e0 / ((e0 + e1) + e2);
    return P;
}

} // namespace pais
