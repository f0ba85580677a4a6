// undistort_host_shim.cpp -- TEST ONLY.  Compiles pais_mvs_amd/csrc/pais_undistort.hpp (the lane-local arithmetic inlined into
// the kernels of pais_undistort.hip) for the host with -ffp-contract=off, with plain loops in place of the kernels.  Not part
// of the product; nothing in the product links this.  With -DUNDISTORT_SHIM_MAIN it is a stand-alone program that walks the
// odd image sizes and the boundary points, for a sanitizer build.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include "../pais_mvs_amd/csrc/pais_undistort.hpp"

using namespace pais;

extern "C" {
// what: 0 undistort_points, 1 distort_points.  steps (may be NULL): Newton steps per point.
void shim_lens_points(const pais_lens *L, int what, long n, const double *in, double *out, unsigned char *valid, int *steps)
{
    const bool inverse = lens_uses_inverse(L->model, what);
    for (long i = 0; i < n; ++i) {
        const LensPoint p = lens_map(*L, inverse, in[2 * i], in[2 * i + 1]);
        out[2 * i] = p.u;
        out[2 * i + 1] = p.v;
        valid[i] = p.ok ? 1 : 0;
        if (steps) steps[i] = p.steps;
    }
}

// Returns the number of valid pixels.
long shim_lens_image(const pais_lens *L, int ch, const unsigned char *src, int W, int H, long stride, unsigned char *dst, unsigned char *mask)
{
    const bool inverse = lens_uses_inverse(L->model, LENS_IMAGE);
    long live = 0;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const LensTap t = lens_tap(*L, inverse, W, H, x, y);
            const size_t p = (size_t)y * (size_t)W + (size_t)x;
            if (mask) mask[p] = t.ok ? 1 : 0;
            live += t.ok ? 1 : 0;
            const unsigned char *r0 = src + (size_t)t.y0 * (size_t)stride, *r1 = src + (size_t)t.y1 * (size_t)stride;
            for (int c = 0; c < ch; ++c)
                dst[p * ch + c] = t.ok ? lens_blend(t, r0[t.x0 * ch + c], r0[t.x1 * ch + c], r1[t.x0 * ch + c], r1[t.x1 * ch + c]) : 0;
        }
    return live;
}
}

#ifdef UNDISTORT_SHIM_MAIN
int main()
{
    const int sizes[][2] = {{1, 1}, {4, 1}, {67, 41}, {256, 3}, {130, 70}};
    const double ks[] = {0.0, 0.3, -0.2, -5.0};
    long total = 0;
    for (const auto &sz : sizes)
        for (double k : ks)
            for (int model = 0; model < 2; ++model)
                for (int ch = 1; ch <= 3; ch += 2) {
                    const int W = sz[0], H = sz[1];
                    const long stride = (long)W * ch + 5;
                    const pais_lens L{{0.9 * W + 3.0, 0.7 * W + 5.0}, {0.45 * W, 0.55 * H}, k, model};
                    std::vector<unsigned char> src((size_t)stride * (H - 1) + (size_t)W * ch), dst((size_t)W * H * ch), mask((size_t)W * H);
                    for (size_t i = 0; i < src.size(); ++i) src[i] = (unsigned char)(i * 37u + 11u);
                    total += shim_lens_image(&L, ch, src.data(), W, H, stride, dst.data(), mask.data());
                    std::vector<double> in, out;
                    for (int y = -H; y < 2 * H + 1; y += 3)
                        for (int x = -W; x < 2 * W + 1; x += 3) { in.push_back(x + 0.25); in.push_back(y - 0.5); }
                    out.resize(in.size());
                    std::vector<unsigned char> valid(in.size() / 2);
                    std::vector<int> steps(in.size() / 2);
                    for (int what = 0; what < 2; ++what) {
                        shim_lens_points(&L, what, (long)valid.size(), in.data(), out.data(), valid.data(), steps.data());
                        for (size_t i = 0; i < valid.size(); ++i)
                            if (valid[i] && steps[i] >= PAIS_UNDISTORT_MAX_STEPS) { printf("a valid point took every step\n"); return 1; }
                    }
                }
    printf("ok %ld\n", total);
    return 0;
}
#endif
