// feature_host_shim.cpp -- TEST ONLY.  Compiles pais_mvs_amd/csrc/pais_feature.hpp (the lane-local arithmetic inlined into
// the kernels of pais_feature.hip, and the walk over octaves that drives them) for the host with -ffp-contract=off, with
// plain loops in place of the kernels, and keeps every stage of the last run so that a test can look at it.  Not part of
// the product; nothing in the product links this.
#include <math.h>
#include <string.h>
#include <vector>
#include "../pais_mvs_amd/csrc/pais_feature.hpp"

using namespace pais;

namespace {
struct Stage { // one octave of the last run
    int W, H;
    std::vector<float> layers;
    std::vector<FeatCand> cands;
    std::vector<FeatKp> fit;
};
std::vector<Stage> g_stages;
FeatResult g_result;

struct HostFeatures {
    const uint8_t *gray;
    int64_t stride;
    int W0, H0, n;
    double sigma, contrast, edge;
    int W = 0, H = 0;
    std::vector<float> layers;

    size_t px() const { return (size_t)W * (size_t)H; }
    FeatOctave view() const { return FeatOctave{layers.data(), W, H, n}; }
    void blur(const float *src, float *dst, const float *taps, int R)
    {
        std::vector<float> tmp(px());
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) tmp[(size_t)y * W + x] = feat_blur_at(src + (size_t)y * W, 1, x, W, taps, R);
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) dst[(size_t)y * W + x] = feat_blur_at(tmp.data() + x, W, y, H, taps, R);
    }
    void open()
    {
        g_stages.push_back(Stage());
        g_stages.back().W = W;
        g_stages.back().H = H;
    }
    int octave0(int Wo, int Ho, const float *t, int R)
    {
        W = Wo; H = Ho;
        std::vector<float> D(px());
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) D[(size_t)y * W + x] = feat_double_at(gray, stride, W0, H0, x, y);
        layers.assign(px() * (size_t)(n + 3), 0.0f);
        blur(D.data(), layers.data(), t, R);
        open();
        return 0;
    }
    int halve()
    {
        const int Ws = W;
        const std::vector<float> prev(layers.begin() + (long)((size_t)n * px()), layers.begin() + (long)((size_t)(n + 1) * px()));
        W /= 2; H /= 2;
        layers.assign(px() * (size_t)(n + 3), 0.0f);
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) layers[(size_t)y * W + x] = prev[(size_t)(2 * y) * Ws + 2 * x];
        open();
        return 0;
    }
    int layer(int i, const float *t, int R)
    {
        blur(layers.data() + (size_t)(i - 1) * px(), layers.data() + (size_t)i * px(), t, R);
        if (i == n + 2) g_stages.back().layers = layers;
        return 0;
    }
    int extrema(float pre, std::vector<FeatCand> *out)
    {
        const FeatOctave o = view();
        for (int i = 1; i <= n; ++i)
            for (int y = FEAT_MARGIN; y < H - FEAT_MARGIN; ++y)
                for (int x = FEAT_MARGIN; x < W - FEAT_MARGIN; ++x)
                    if (feat_is_extremum(o, i, x, y, pre)) out->push_back(FeatCand{x, y, i});
        g_stages.back().cands = *out;
        return 0;
    }
    int refine(const std::vector<FeatCand> &c, std::vector<FeatKp> *out)
    {
        for (const FeatCand &q : c) out->push_back(feat_refine(view(), q.x, q.y, q.layer, sigma, contrast, edge));
        g_stages.back().fit = *out;
        return 0;
    }
    int orient(const std::vector<FeatKp> &k, std::vector<FeatPeaks> *out)
    {
        for (const FeatKp &kp : k) {
            const float *L = layers.data() + (size_t)kp.layer * px();
            double hist[FEAT_ORI_BINS] = {0};
            const int rad = feat_ori_radius(kp.s);
            for (int dy = -rad; dy <= rad; ++dy)
                for (int dx = -rad; dx <= rad; ++dx) {
                    double v;
                    const int b = feat_ori_sample(L, W, H, kp.x, kp.y, kp.s, dx, dy, &v);
                    if (b >= 0) hist[b] = hist[b] + v;
                }
            FeatPeaks p;
            feat_ori_peaks(hist, &p);
            out->push_back(p);
        }
        return 0;
    }
    int describe(const std::vector<FeatOriented> &k, std::vector<float> *out)
    {
        out->resize(k.size() * FEAT_DESC);
        for (size_t q = 0; q < k.size(); ++q) {
            const FeatOriented &kp = k[q];
            const float *L = layers.data() + (size_t)kp.layer * px();
            const double hw = 3.0 * kp.s;
            const double ct = det_cos(kp.theta) / hw, st = det_sin(kp.theta) / hw;
            const int rad = feat_desc_radius(kp.s, W, H);
            double Hh[FEAT_HIST] = {0};
            for (int dy = -rad; dy <= rad; ++dy)
                for (int dx = -rad; dx <= rad; ++dx) {
                    const FeatDescSample s = feat_desc_sample(L, W, H, kp.x, kp.y, dx, dy, ct, st, kp.theta);
                    if (s.idx >= 0) feat_desc_add(Hh, s.idx, s.v);
                }
            feat_desc_finish(Hh, out->data() + q * FEAT_DESC);
        }
        return 0;
    }
};
} // namespace

extern "C" {
double shim_atan2(double y, double x) { return det_atan2(y, x); }
void shim_atan2_many(const double *y, const double *x, long n, double *out)
{
    for (long i = 0; i < n; ++i) out[i] = det_atan2(y[i], x[i]);
}
int shim_feat_tap_radius(double s) { return feat_tap_radius(s); }
void shim_feat_taps(double s, float *out)
{
    const std::vector<float> t = feat_taps(s);
    memcpy(out, t.data(), sizeof(float) * t.size());
}
// prm: layers, sigma, input_blur, contrast, edge.  Returns the number of keypoints (< 0: refused parameters).
long shim_feat_run(const unsigned char *gray, int W, int H, long stride, int layers, double sigma, double input_blur, double contrast, double edge)
{
    g_stages.clear();
    HostFeatures be{gray, (int64_t)stride, W, H, layers, sigma, contrast, edge};
    const FeatParams p{layers, sigma, input_blur, contrast, edge};
    if (feat_walk(be, W, H, p, &g_result)) return -1;
    return (long)g_result.count();
}
void shim_feat_result(float *xy, float *scale, float *angle, int *octave_layer, float *desc)
{
    const size_t n = (size_t)g_result.count();
    if (!n) return;
    memcpy(xy, g_result.xy.data(), sizeof(float) * 2 * n);
    memcpy(scale, g_result.scale.data(), sizeof(float) * n);
    memcpy(angle, g_result.angle.data(), sizeof(float) * n);
    memcpy(octave_layer, g_result.octave_layer.data(), sizeof(int) * 2 * n);
    memcpy(desc, g_result.desc.data(), sizeof(float) * FEAT_DESC * n);
}
int shim_feat_octaves(void) { return (int)g_stages.size(); }
void shim_feat_octave_size(int o, int *W, int *H) { *W = g_stages[o].W; *H = g_stages[o].H; }
void shim_feat_layers(int o, float *out) { memcpy(out, g_stages[o].layers.data(), sizeof(float) * g_stages[o].layers.size()); }
long shim_feat_num_cands(int o) { return (long)g_stages[o].cands.size(); }
void shim_feat_cands(int o, int *out) // x, y, layer per candidate
{
    for (size_t k = 0; k < g_stages[o].cands.size(); ++k) {
        out[3 * k] = g_stages[o].cands[k].x; out[3 * k + 1] = g_stages[o].cands[k].y; out[3 * k + 2] = g_stages[o].cands[k].layer;
    }
}
// the FIT of every candidate, in the candidates' order: x, y, layer, ok and px, py, s
void shim_feat_fit(int o, int *ints, double *vals)
{
    for (size_t k = 0; k < g_stages[o].fit.size(); ++k) {
        const FeatKp &f = g_stages[o].fit[k];
        ints[4 * k] = f.x; ints[4 * k + 1] = f.y; ints[4 * k + 2] = f.layer; ints[4 * k + 3] = f.ok;
        vals[3 * k] = f.px; vals[3 * k + 1] = f.py; vals[3 * k + 2] = f.s;
    }
}
}
