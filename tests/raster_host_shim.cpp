// raster_host_shim.cpp -- TEST ONLY.  Compiles pais_mvs_amd/csrc/pais_raster.hpp (the lane-local arithmetic inlined into
// k_tri_setup, k_tri_walk and k_tri_packed of pais_render.hip) for the host with -ffp-contract=off, with plain loops in place
// of the kernels and a sequential z-buffer in place of the atomics.  Not part of the product; nothing in the product links
// this.  With -DRASTER_SHIM_MAIN it is a stand-alone program that renders odd sizes of its own, for a sanitizer build.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include "../pais_mvs_amd/csrc/pais_raster.hpp"

extern "C" {
int shim_constant(int k)
{
    const int c[] = {PAIS_RENDER_DISC, PAIS_RENDER_POINT, PAIS_RENDER_CULL_BACK, PAIS_RENDER_MAX_POINT_SIZE, PAIS_VIS_VISIBLE, PAIS_VIS_OCCLUDED,
                     PAIS_VIS_IN_FRONT, PAIS_VIS_EMPTY, PAIS_VIS_OUTSIDE, PAIS_VIS_BEHIND, PAIS_VIS_SELF, (int)sizeof(pais_view)};
    return (k >= 0 && k < (int)(sizeof(c) / sizeof(c[0]))) ? c[k] : -1;
}

// pais_mesh_render on the host.  use_box 1: every triangle walks its raster_box only, as the kernels do; 0: every pixel.
// skips (may be NULL): num_views x nt, the RASTER_* code of every pair.  Returns the covered (pixel, triangle) pairs.
long long shim_mesh_render(int flags, int nv, const double *vertices, int nt, const int32_t *triangles, int num_views, const pais_view *views,
                           int width, int height, int use_box, double *depth, int32_t *id, int32_t *skips)
{
    (void)nv;
    const size_t pix = (size_t)width * (size_t)height;
    long long covered = 0;
    for (int v = 0; v < num_views; ++v) {
        double *Dm = depth + (size_t)v * pix;
        int32_t *Im = id + (size_t)v * pix;
        for (size_t p = 0; p < pix; ++p) { Dm[p] = (double)INFINITY; Im[p] = -1; }
        const pais_view &V = views[v];
        for (int s = 0; s < nt; ++s) {
            const int a = triangles[3 * (size_t)s], b = triangles[3 * (size_t)s + 1], c = triangles[3 * (size_t)s + 2];
            double A[3], B[3], C[3];
            pais::raster_camera(V, vertices + 3 * (size_t)a, A);
            pais::raster_camera(V, vertices + 3 * (size_t)b, B);
            pais::raster_camera(V, vertices + 3 * (size_t)c, C);
            pais::RasterTri T;
            pais::raster_setup(a, b, c, A, B, C, &T);
            int skip = pais::raster_skip(flags, a, b, c, A[2], B[2], C[2], T.D);
            int u0 = 0, u1 = width - 1, v0 = 0, v1 = height - 1;
            if (skip == pais::RASTER_LIVE && use_box && !pais::raster_box(V, A, B, C, T.D, width, height, &u0, &u1, &v0, &v1)) skip = pais::RASTER_OFF_IMAGE;
            if (skips) skips[(size_t)v * (size_t)nt + (size_t)s] = skip;
            if (skip != pais::RASTER_LIVE) continue;
            for (int y = v0; y <= v1; ++y)
                for (int x = u0; x <= u1; ++x) {
                    double t;
                    if (!pais::raster_hit(T, V.focal[0], V.focal[1], V.pp[0], V.pp[1], x, y, &t)) continue;
                    ++covered;
                    const size_t p = (size_t)y * (size_t)width + (size_t)x;
                    if (t < Dm[p]) { Dm[p] = t; Im[p] = s; } // ascending s: the lowest index among equal depths stays
                }
        }
    }
    return covered;
}
}

#ifdef RASTER_SHIM_MAIN
int main()
{
    const int cases[][4] = {{1, 1, 1, 1}, {7, 1, 37, 29}, {300, 3, 65, 48}, {63, 2, 7, 5}, {1000, 2, 33, 3}}; // nt, views, width, height
    uint64_t z = 88172645463325252ULL;
    auto rnd = [&z]() { z ^= z << 13; z ^= z >> 7; z ^= z << 17; return (double)(z >> 11) / 9007199254740992.0 - 0.5; };
    long long total = 0, live = 0;
    for (const auto &c : cases) {
        const int nt = c[0], V = c[1], W = c[2], H = c[3], nv = nt / 2 + 3;
        std::vector<double> ver(3 * (size_t)nv), d0((size_t)V * W * H), d1((size_t)V * W * H);
        std::vector<int32_t> tri(3 * (size_t)nt), i0((size_t)V * W * H), i1((size_t)V * W * H), skips((size_t)V * nt);
        std::vector<pais_view> views((size_t)V);
        for (double &p : ver) p = 3.0 * rnd();
        for (int s = 0; s < nt; ++s) {
            const int a = (int)((rnd() + 0.5) * nv) % nv; // near-by indices: small triangles; every seventh one spans the cloud
            tri[3 * (size_t)s] = a;
            tri[3 * (size_t)s + 1] = s % 7 == 3 ? (int)((rnd() + 0.5) * nv) % nv : (a + 1) % nv;
            tri[3 * (size_t)s + 2] = s % 11 == 5 ? a : (a + 2) % nv;
        }
        for (pais_view &v : views) {
            const double a = 6.0 * rnd(), ca = cos(a), sa = sin(a);
            const double R[9] = {ca, 0.0, sa, 0.0, 1.0, 0.0, -sa, 0.0, ca};
            for (int k = 0; k < 9; ++k) v.R[k] = R[k];
            v.T[0] = rnd(); v.T[1] = rnd(); v.T[2] = 1.5; // the cloud reaches behind the camera plane
            v.focal[0] = v.focal[1] = 0.7 * W;
            v.pp[0] = (double)(W >> 1); v.pp[1] = (double)(H >> 1);
        }
        for (int flags = 0; flags < 2; ++flags) {
            const long long n0 = shim_mesh_render(flags, nv, ver.data(), nt, tri.data(), V, views.data(), W, H, 0, d0.data(), i0.data(), nullptr);
            const long long n1 = shim_mesh_render(flags, nv, ver.data(), nt, tri.data(), V, views.data(), W, H, 1, d1.data(), i1.data(), skips.data());
            if (n0 != n1) { printf("case nt=%d flags=%d: %lld covered pairs without the box, %lld with it\n", nt, flags, n0, n1); return 1; }
            for (size_t k = 0; k < d0.size(); ++k)
                if (i0[k] != i1[k] || !(d0[k] == d1[k]) || (i0[k] < 0) != (d0[k] == (double)INFINITY) || i0[k] >= nt) {
                    printf("case nt=%d flags=%d pixel %zu: %g / %d without the box, %g / %d with it\n", nt, flags, k, d0[k], i0[k], d1[k], i1[k]);
                    return 1;
                }
            for (int32_t s : skips) {
                if (s < 0 || s > pais::RASTER_OFF_IMAGE) { printf("skip code %d\n", s); return 1; }
                live += s == pais::RASTER_LIVE;
            }
            total += n0;
        }
    }
    printf("ok %lld %lld\n", total, live);
    return 0;
}
#endif
