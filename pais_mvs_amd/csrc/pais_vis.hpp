// pais_vis.hpp -- the lane-local arithmetic of pais_depth_test / pais_cloud_visibility (include/pais_render.h): the statements
// of the header written once, inlined into k_depth_test (pais_render.hip) and compiled for the host by
// tests/vis_host_shim.cpp.  Both builds use -ffp-contract=off, so every product, sum and quotient is rounded to double on its
// own.  No array is indexed dynamically: on the GPU everything stays in registers.
#pragma once
#include <math.h>
#include <stdint.h>
#include "../../include/pais_render.h"
#include "pais_dev.hpp"

namespace pais {

// One (point, view) pair.  D (H x W doubles) and I (H x W ids, or nullptr) are the maps of this view; self: the index of the
// point (read with PAIS_VIS_SELF only).  Returns the code; *occluder and *margin as the header defines them.
PAIS_HD int vis_test(const pais_view &V, double c0, double c1, double c2, int W, int H, const double *D, const int32_t *I, int flags,
                     int32_t self, double tol, int32_t *occluder, double *margin)
{
    *occluder = -1;
    *margin = __builtin_nan("");
    const double x = ((V.R[0] * c0 + V.R[1] * c1) + V.R[2] * c2) + V.T[0];
    const double y = ((V.R[3] * c0 + V.R[4] * c1) + V.R[5] * c2) + V.T[1];
    const double z = ((V.R[6] * c0 + V.R[7] * c1) + V.R[8] * c2) + V.T[2];
    if (!(z > 0.0)) return PAIS_VIS_BEHIND;
    const double pu = V.focal[0] * (x / z) + V.pp[0];
    const double pv = V.focal[1] * (y / z) + V.pp[1];
    if (!(isfinite(pu) && isfinite(pv) && fabs(pu) < 0x1p30 && fabs(pv) < 0x1p30)) return PAIS_VIS_OUTSIDE;
    const int ru = cv_round(pu), rv = cv_round(pv);
    if (ru < 0 || ru >= W || rv < 0 || rv >= H) return PAIS_VIS_OUTSIDE;
    const size_t p = (size_t)rv * (size_t)W + (size_t)ru;
    const double d = D[p];
    if (d == (double)INFINITY) return PAIS_VIS_EMPTY;
    const int32_t at = I ? I[p] : -1;
    const double m = z - d;
    *occluder = at;
    *margin = m;
    if ((flags & PAIS_VIS_SELF) && at == self) return PAIS_VIS_VISIBLE;
    if (m > tol) return PAIS_VIS_OCCLUDED;
    if (m < -tol) return PAIS_VIS_IN_FRONT;
    return PAIS_VIS_VISIBLE;
}

} // namespace pais
