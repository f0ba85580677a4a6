// vis_host_shim.cpp -- TEST ONLY.  Compiles pais_mvs_amd/csrc/pais_vis.hpp (the lane-local arithmetic inlined into k_depth_test
// of pais_render.hip) for the host with -ffp-contract=off, with a plain loop in place of the kernel.  Not part of the product;
// nothing in the product links this.  With -DVIS_SHIM_MAIN it is a stand-alone program that walks odd sizes over maps of its
// own, for a sanitizer build.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include "../pais_mvs_amd/csrc/pais_vis.hpp"

extern "C" {
// pais_depth_test over host maps: depth / id (or NULL) num_views x height x width; outputs view-major [v * n + i].
void shim_depth_test(int flags, int n, const double *points, int num_views, const pais_view *views, int width, int height, const double *depth,
                     const int32_t *id, double tol, uint8_t *code, int32_t *occluder, double *margin)
{
    const size_t pix = (size_t)width * (size_t)height;
    for (int v = 0; v < num_views; ++v)
        for (int i = 0; i < n; ++i) {
            const size_t o = (size_t)v * (size_t)n + (size_t)i;
            code[o] = (uint8_t)pais::vis_test(views[v], points[3 * (size_t)i], points[3 * (size_t)i + 1], points[3 * (size_t)i + 2], width, height,
                                              depth + (size_t)v * pix, id ? id + (size_t)v * pix : nullptr, flags, (int32_t)i, tol, &occluder[o],
                                              &margin[o]);
        }
}
}

#ifdef VIS_SHIM_MAIN
int main()
{
    const int cases[][4] = {{1, 1, 1, 1}, {63, 1, 37, 29}, {65, 3, 65, 48}, {300, 2, 7, 5}, {1000, 3, 1, 3}}; // n, views, width, height
    long seen[6] = {0, 0, 0, 0, 0, 0};
    uint64_t z = 88172645463325252ULL;
    auto rnd = [&z]() { z ^= z << 13; z ^= z >> 7; z ^= z << 17; return (double)(z >> 11) / 9007199254740992.0 - 0.5; };
    for (const auto &c : cases) {
        const int n = c[0], V = c[1], W = c[2], H = c[3];
        std::vector<double> pts(3 * (size_t)n), depth((size_t)V * W * H), margin((size_t)V * n);
        std::vector<int32_t> id((size_t)V * W * H), occ((size_t)V * n);
        std::vector<uint8_t> code((size_t)V * n);
        std::vector<pais_view> views((size_t)V);
        for (double &p : pts) p = 6.0 * rnd();
        for (size_t k = 0; k < depth.size(); ++k) {
            depth[k] = (k % 7 == 3) ? (double)INFINITY : 3.0 + 2.0 * rnd();
            id[k] = (k % 7 == 3) ? -1 : (int32_t)(k % (size_t)n);
        }
        for (pais_view &v : views) {
            const double a = 6.0 * rnd(), ca = cos(a), sa = sin(a);
            const double R[9] = {ca, 0.0, sa, 0.0, 1.0, 0.0, -sa, 0.0, ca};
            for (int k = 0; k < 9; ++k) v.R[k] = R[k];
            v.T[0] = rnd(); v.T[1] = rnd(); v.T[2] = 3.0;
            v.focal[0] = v.focal[1] = 0.7 * W;
            v.pp[0] = (double)(W >> 1); v.pp[1] = (double)(H >> 1);
        }
        for (int flags = 0; flags < 2; ++flags)
            for (int withId = 0; withId < 2; ++withId) {
                if (flags && !withId) continue;
                shim_depth_test(flags ? PAIS_VIS_SELF : 0, n, pts.data(), V, views.data(), W, H, depth.data(), withId ? id.data() : nullptr, 0.25,
                                code.data(), occ.data(), margin.data());
                for (size_t k = 0; k < code.size(); ++k) {
                    if (code[k] > PAIS_VIS_BEHIND) { printf("pair %zu: code %d\n", k, (int)code[k]); return 1; }
                    if ((code[k] <= PAIS_VIS_IN_FRONT) != !isnan(margin[k])) { printf("pair %zu: code %d with margin %g\n", k, (int)code[k], margin[k]); return 1; }
                    ++seen[code[k]];
                }
            }
    }
    printf("ok %ld %ld %ld %ld %ld %ld\n", seen[0], seen[1], seen[2], seen[3], seen[4], seen[5]);
    return 0;
}
#endif
