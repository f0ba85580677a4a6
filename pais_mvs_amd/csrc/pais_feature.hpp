// pais_feature.hpp -- the statements of include/pais_feature.h, written once.
//
// The first part is PAIS_HD lane-local arithmetic: inlined into the kernels of pais_feature.hip and compiled for the host by
// tests/feature_host_shim.cpp, so both produce the same bits.  The second part (host only) is the walk over octaves that
// both share: tap tables, the order of the stages, the sort.  It drives a backend -- the kernels in the product, plain loops
// in the test shim.  Neither is a CPU fallback of the product: no product entry point runs the loops.
#pragma once
#include "pais_dev.hpp"

namespace pais {

constexpr int FEAT_MARGIN = 5, FEAT_MAX_LAYERS = 8, FEAT_MAX_OCTAVES = 24, FEAT_MAX_RADIUS = 512;
constexpr int FEAT_ORI_BINS = 36, FEAT_MAX_PEAKS = 18, FEAT_DESC = 128, FEAT_HIST = 6 * 6 * 10;
constexpr double FEAT_PI2 = 6.283185307179586, FEAT_LN2 = 0.6931471805599453;

// One octave: n + 3 Gaussian layers of W x H floats, layer after layer.
struct FeatOctave {
    const float *L;
    int W, H, n;
};
struct FeatCand { int32_t x, y, layer; };
struct FeatKp {       // a candidate after the FIT
    int32_t x, y, layer, ok;
    double px, py, s; // octave pixels
};
struct FeatPeaks {    // the orientation peaks of one keypoint
    int32_t n, bin[FEAT_MAX_PEAKS];
    int32_t _pad;
    double theta[FEAT_MAX_PEAKS];
};
struct FeatOriented { // one keypoint per peak
    int32_t x, y, layer, peak;
    double px, py, s, theta;
};
struct FeatDescSample {
    int idx;          // ((R 6) + C) 10 + o0; -1: the sample adds nothing
    double v[8];      // v000 v001 v010 v011 v100 v101 v110 v111
};

PAIS_HD int feat_clamp(int i, int n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }

// DOUBLING: sample (X, Y) of the 2W x 2H image
PAIS_HD float feat_double_at(const uint8_t *g, int64_t stride, int W, int H, int X, int Y)
{
    const int x = X >> 1, y = Y >> 1;
    const int x1 = x + 1 < W ? x + 1 : W - 1, y1 = y + 1 < H ? y + 1 : H - 1;
    const float a = (float)g[(int64_t)y * stride + x], b = (float)g[(int64_t)y * stride + x1];
    const float c = (float)g[(int64_t)y1 * stride + x], d = (float)g[(int64_t)y1 * stride + x1];
    if (!(Y & 1)) return (X & 1) ? 0.5f * (a + b) : a;
    if (!(X & 1)) return 0.5f * (a + c);
    return 0.5f * (0.5f * (a + b) + 0.5f * (c + d));
}

// BLUR: one output sample of a pass along a line of n samples `step` floats apart
PAIS_HD float feat_blur_at(const float *line, int64_t step, int pos, int n, const float *taps, int R)
{
    float acc = 0.0f;
    for (int k = 0; k <= 2 * R; ++k) acc = acc + taps[k] * line[(int64_t)feat_clamp(pos + k - R, n) * step];
    return acc;
}

PAIS_HD float feat_dog(const FeatOctave &o, int i, int x, int y)
{
    const size_t ls = (size_t)o.W * (size_t)o.H, p = (size_t)y * (size_t)o.W + (size_t)x;
    return o.L[(size_t)(i + 1) * ls + p] - o.L[(size_t)i * ls + p];
}

// EXTREMA: (x, y) inside the margin, 1 <= i <= n
PAIS_HD bool feat_is_extremum(const FeatOctave &o, int i, int x, int y, float pre)
{
    const float v = feat_dog(o, i, x, y);
    if (!(fabsf(v) > pre)) return false;
    bool isMax = v > 0.0f, isMin = v < 0.0f;
    for (int di = -1; di <= 1; ++di)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                const float u = feat_dog(o, i + di, x + dx, y + dy);
                isMax = isMax && v >= u;
                isMin = isMin && v <= u;
            }
    return isMax || isMin;
}

PAIS_HD bool feat_in_margin(const FeatOctave &o, int x, int y)
{
    return x >= FEAT_MARGIN && x < o.W - FEAT_MARGIN && y >= FEAT_MARGIN && y < o.H - FEAT_MARGIN;
}

// FIT
PAIS_HD FeatKp feat_refine(const FeatOctave &o, int x, int y, int i, double sigma, double contrast, double edge)
{
    FeatKp r;
    r.x = x; r.y = y; r.layer = i; r.ok = 0;
    r.px = r.py = r.s = 0.0;
#define FD(ii, xx, yy) ((double)feat_dog(o, (ii), (xx), (yy)))
    for (int it = 0; it < 5; ++it) {
        const double dx = (FD(i, x + 1, y) - FD(i, x - 1, y)) * 0.5;
        const double dy = (FD(i, x, y + 1) - FD(i, x, y - 1)) * 0.5;
        const double ds = (FD(i + 1, x, y) - FD(i - 1, x, y)) * 0.5;
        const double v2 = 2.0 * FD(i, x, y);
        const double dxx = (FD(i, x + 1, y) + FD(i, x - 1, y)) - v2;
        const double dyy = (FD(i, x, y + 1) + FD(i, x, y - 1)) - v2;
        const double dss = (FD(i + 1, x, y) + FD(i - 1, x, y)) - v2;
        const double dxy = ((FD(i, x + 1, y + 1) - FD(i, x - 1, y + 1)) - (FD(i, x + 1, y - 1) - FD(i, x - 1, y - 1))) * 0.25;
        const double dxs = ((FD(i + 1, x + 1, y) - FD(i + 1, x - 1, y)) - (FD(i - 1, x + 1, y) - FD(i - 1, x - 1, y))) * 0.25;
        const double dys = ((FD(i + 1, x, y + 1) - FD(i + 1, x, y - 1)) - (FD(i - 1, x, y + 1) - FD(i - 1, x, y - 1))) * 0.25;
        const double Hm[9] = {dxx, dxy, dxs, dxy, dyy, dys, dxs, dys, dss};
        double A[9];
        inv3(Hm, A);
        const double X0 = -((A[0] * dx + A[1] * dy) + A[2] * ds);
        const double X1 = -((A[3] * dx + A[4] * dy) + A[5] * ds);
        const double X2 = -((A[6] * dx + A[7] * dy) + A[8] * ds);
        if (fabs(X0) < 0.5 && fabs(X1) < 0.5 && fabs(X2) < 0.5) {
            const double c = FD(i, x, y) + 0.5 * ((dx * X0 + dy * X1) + ds * X2);
            if (fabs(c) * (double)o.n < contrast * 255.0) return r;
            const double tr = dxx + dyy, det = dxx * dyy - dxy * dxy;
            if (det <= 0.0 || (tr * tr) * edge >= ((edge + 1.0) * (edge + 1.0)) * det) return r;
            r.x = x; r.y = y; r.layer = i; r.ok = 1;
            r.px = (double)x + X0;
            r.py = (double)y + X1;
            r.s = sigma * det_exp(((double)i + X2) / (double)o.n * FEAT_LN2);
            return r;
        }
        if (!(fabs(X0) <= 1e6 && fabs(X1) <= 1e6 && fabs(X2) <= 1e6)) return r; // (NaN and inf fall here)
        x += (int)floor(X0 + 0.5);
        y += (int)floor(X1 + 0.5);
        i += (int)floor(X2 + 0.5);
        if (i < 1 || i > o.n || !feat_in_margin(o, x, y)) return r;
    }
#undef FD
    return r;
}

// gradient sample of one Gaussian layer; false: the sample does not exist
PAIS_HD bool feat_grad(const float *L, int W, int H, int xx, int yy, double *mag, double *ori)
{
    if (!(xx > 0 && xx < W - 1 && yy > 0 && yy < H - 1)) return false;
    const size_t p = (size_t)yy * (size_t)W + (size_t)xx;
    const double gx = (double)L[p + 1] - (double)L[p - 1];
    const double gy = (double)L[p - (size_t)W] - (double)L[p + (size_t)W];
    *mag = sqrt(gx * gx + gy * gy);
    *ori = det_atan2(gy, gx);
    return true;
}

PAIS_HD int feat_ori_radius(double s) { return (int)floor(3.0 * (1.5 * s) + 0.5); }

// ORIENTATION: sample (dx, dy) -> its bin (or -1) and what it adds
PAIS_HD int feat_ori_sample(const float *L, int W, int H, int x, int y, double s, int dx, int dy, double *val)
{
    double mag, ori;
    if (!feat_grad(L, W, H, x + dx, y + dy, &mag, &ori)) return -1;
    const double so = 1.5 * s;
    const double e = -1.0 / (2.0 * so * so);
    int b = (int)floor(ori * (36.0 / FEAT_PI2) + 0.5);
    if (b < 0) b += FEAT_ORI_BINS;
    if (b >= FEAT_ORI_BINS) b -= FEAT_ORI_BINS;
    if (b < 0 || b >= FEAT_ORI_BINS) return -1; // (cannot occur for finite gradients)
    *val = det_exp((double)(dx * dx + dy * dy) * e) * mag;
    return b;
}

// smoothing and peaks of a filled histogram
PAIS_HD void feat_ori_peaks(const double *hist, FeatPeaks *out)
{
    double h[FEAT_ORI_BINS];
    double m = 0.0;
    for (int j = 0; j < FEAT_ORI_BINS; ++j) {
        const int a2 = (j + 34) % 36, a1 = (j + 35) % 36, b1 = (j + 1) % 36, b2 = (j + 2) % 36;
        h[j] = ((hist[a2] + hist[b2]) * (1.0 / 16.0) + (hist[a1] + hist[b1]) * (4.0 / 16.0)) + hist[j] * (6.0 / 16.0);
        if (j == 0 || h[j] > m) m = h[j];
    }
    out->n = 0;
    out->_pad = 0;
    for (int k = 0; k < FEAT_MAX_PEAKS; ++k) { out->bin[k] = 0; out->theta[k] = 0.0; }
    const double thr = 0.8 * m;
    for (int j = 0; j < FEAT_ORI_BINS; ++j) {
        const double hl = h[(j + 35) % 36], hr = h[(j + 1) % 36];
        if (h[j] > hl && h[j] > hr && h[j] >= thr && out->n < FEAT_MAX_PEAKS) {
            double bin = (double)j + 0.5 * (hl - hr) / ((hl - 2.0 * h[j]) + hr);
            if (bin < 0.0) bin += 36.0;
            if (bin >= 36.0) bin -= 36.0;
            out->bin[out->n] = j;
            out->theta[out->n] = bin * (FEAT_PI2 / 36.0);
            ++out->n;
        }
    }
}

PAIS_HD int feat_desc_radius(double s, int W, int H)
{
    const double hw = 3.0 * s;
    const int rad = (int)floor(hw * 1.4142135623730951 * 2.5 + 0.5);
    const int diag = (int)floor(sqrt((double)W * (double)W + (double)H * (double)H));
    return rad < diag ? rad : diag;
}

// DESCRIPTOR: what sample (dx, dy) adds; ct, st: det_cos(theta) / hw, det_sin(theta) / hw
PAIS_HD FeatDescSample feat_desc_sample(const float *L, int W, int H, int x, int y, int dx, int dy, double ct, double st, double theta)
{
    FeatDescSample r;
    r.idx = -1;
    const double cr = (double)dx * ct - (double)dy * st, rr = (double)dx * st + (double)dy * ct;
    const double rb = rr + 1.5, cb = cr + 1.5;
    if (!(rb > -1.0 && rb < 4.0 && cb > -1.0 && cb < 4.0)) return r;
    double mag, ori;
    if (!feat_grad(L, W, H, x + dx, y + dy, &mag, &ori)) return r;
    const double m = mag * det_exp((cr * cr + rr * rr) * (-0.125));
    if (ori < 0.0) ori += FEAT_PI2;
    const double ob = (ori - theta) * (8.0 / FEAT_PI2);
    const double rf = floor(rb), cf = floor(cb), of = floor(ob);
    const double fr = rb - rf, fc = cb - cf, fo = ob - of;
    int o0 = (int)of;
    if (o0 < 0) o0 += 8;
    if (o0 >= 8) o0 -= 8;
    if (o0 < 0 || o0 >= 8) return r; // (cannot occur for finite angles)
    const double v1 = m * fr, v0 = m - v1;
    const double v11 = v1 * fc, v10 = v1 - v11, v01 = v0 * fc, v00 = v0 - v01;
    r.v[7] = v11 * fo; r.v[6] = v11 - r.v[7];
    r.v[5] = v10 * fo; r.v[4] = v10 - r.v[5];
    r.v[3] = v01 * fo; r.v[2] = v01 - r.v[3];
    r.v[1] = v00 * fo; r.v[0] = v00 - r.v[1];
    r.idx = (((int)rf + 1) * 6 + ((int)cf + 1)) * 10 + o0;
    return r;
}

// the eight additions of one sample, in the header's order
PAIS_HD void feat_desc_add(double *Hh, int idx, const double *v)
{
    Hh[idx] = Hh[idx] + v[0];
    Hh[idx + 1] = Hh[idx + 1] + v[1];
    Hh[idx + 10] = Hh[idx + 10] + v[2];
    Hh[idx + 11] = Hh[idx + 11] + v[3];
    Hh[idx + 60] = Hh[idx + 60] + v[4];
    Hh[idx + 61] = Hh[idx + 61] + v[5];
    Hh[idx + 70] = Hh[idx + 70] + v[6];
    Hh[idx + 71] = Hh[idx + 71] + v[7];
}

// fold, normalise, clamp, renormalise, scale
PAIS_HD void feat_desc_finish(double *Hh, float *out)
{
    double d[FEAT_DESC];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double *c = Hh + ((i + 1) * 6 + (j + 1)) * 10;
            c[0] = c[0] + c[8];
            c[1] = c[1] + c[9];
            for (int k = 0; k < 8; ++k) d[(4 * i + j) * 8 + k] = c[k];
        }
    double n2 = 0.0;
    for (int k = 0; k < FEAT_DESC; ++k) n2 = n2 + d[k] * d[k];
    const double t = 0.2 * sqrt(n2);
    double m2 = 0.0;
    for (int k = 0; k < FEAT_DESC; ++k) {
        d[k] = d[k] < t ? d[k] : t;
        m2 = m2 + d[k] * d[k];
    }
    const double sq = sqrt(m2);
    const double g = 512.0 / (sq > 0x1p-52 ? sq : 0x1p-52);
    for (int k = 0; k < FEAT_DESC; ++k) {
        const double q = d[k] * g;
        out[k] = (float)(q < 255.0 ? q : 255.0);
    }
}

} // namespace pais

// ----------------------------------------------------------------------------------------------------------- host walk ---
#include <algorithm>
#include <cmath>
#include <vector>

namespace pais {

struct FeatParams {
    int layers;
    double sigma, input_blur, contrast, edge;
};
struct FeatResult { // the output arrays of pais_feature_detect, whole
    std::vector<float> xy, scale, angle, desc;
    std::vector<int32_t> octave_layer;
    int64_t count() const { return (int64_t)scale.size(); }
};

inline int feat_tap_radius(double s) { return (int)std::ceil(4.0 * s); }
inline std::vector<float> feat_taps(double s)
{
    const int R = feat_tap_radius(s);
    std::vector<double> w((size_t)(2 * R + 1));
    double S = 0.0;
    for (int k = 0; k <= 2 * R; ++k) {
        w[k] = std::exp(-((double)((k - R) * (k - R))) / (2.0 * s * s));
        S = S + w[k];
    }
    std::vector<float> t(w.size());
    for (int k = 0; k <= 2 * R; ++k) t[k] = (float)(w[k] / S);
    return t;
}
// sig_0 (the blur of the doubled image) and sig_1 .. sig_{n+2}
inline std::vector<double> feat_sigmas(const FeatParams &p)
{
    std::vector<double> sig((size_t)(p.layers + 3));
    sig[0] = std::sqrt(std::max(p.sigma * p.sigma - 4.0 * p.input_blur * p.input_blur, 0.01));
    const double k = std::pow(2.0, 1.0 / (double)p.layers);
    for (int i = 1; i < p.layers + 3; ++i) {
        const double a = p.sigma * std::pow(k, (double)(i - 1)), b = a * k;
        sig[i] = std::sqrt(b * b - a * a);
    }
    return sig;
}
// the widest table's radius; < 0: refused (a radius above FEAT_MAX_RADIUS, or no usable sigma)
inline int feat_max_radius(const FeatParams &p)
{
    int Rmax = 0;
    for (double s : feat_sigmas(p)) {
        if (!(s > 0.0) || !std::isfinite(s) || 4.0 * s > (double)FEAT_MAX_RADIUS) return -1;
        Rmax = std::max(Rmax, feat_tap_radius(s));
    }
    return Rmax;
}

// The walk.  Backend B:  int octave0(W, H, taps, R)  -- doubling and L_0;   int halve()  -- the next octave's L_0 from L_n, and
// the move to it;   int layer(i, taps, R);   int extrema(pre, cands);   int refine(cands, kps);   int orient(kps, peaks);
// int describe(oriented, desc).  Each returns 0 or an error that ends the walk.  cands come back in ANY order.
template <class B> int feat_walk(B &be, int W, int H, const FeatParams &p, FeatResult *out)
{
    *out = FeatResult();
    const int n = p.layers;
    const std::vector<double> sig = feat_sigmas(p);
    const int Rmax = feat_max_radius(p);
    if (Rmax < 0) return -1;
    const int minDim = 2 * Rmax + 1 + FEAT_MARGIN;
    std::vector<std::vector<float>> taps;
    for (double s : sig) taps.push_back(feat_taps(s));
    const float pre = (float)std::floor(0.5 * p.contrast / (double)n * 255.0);
    int64_t Wo = 2 * (int64_t)W, Ho = 2 * (int64_t)H;
    for (int o = 0; o < FEAT_MAX_OCTAVES && std::min(Wo, Ho) >= minDim; ++o, Wo /= 2, Ho /= 2) {
        if (int rc = o == 0 ? be.octave0((int)Wo, (int)Ho, taps[0].data(), feat_tap_radius(sig[0])) : be.halve()) return rc;
        for (int i = 1; i < n + 3; ++i)
            if (int rc = be.layer(i, taps[i].data(), feat_tap_radius(sig[i]))) return rc;
        std::vector<FeatCand> cands;
        if (int rc = be.extrema(pre, &cands)) return rc;
        if (cands.empty()) continue;
        std::vector<FeatKp> fit;
        if (int rc = be.refine(cands, &fit)) return rc;
        // ORDER, and one keypoint per (x, y, i)
        std::vector<FeatKp> kps;
        for (const FeatKp &k : fit)
            if (k.ok) kps.push_back(k);
        auto key = [](const FeatKp &k) { return ((int64_t)k.layer << 48) | ((int64_t)k.y << 24) | (int64_t)k.x; };
        std::sort(kps.begin(), kps.end(), [&](const FeatKp &a, const FeatKp &b) { return key(a) < key(b); });
        kps.erase(std::unique(kps.begin(), kps.end(), [&](const FeatKp &a, const FeatKp &b) { return key(a) == key(b); }), kps.end());
        if (kps.empty()) continue;
        std::vector<FeatPeaks> peaks;
        if (int rc = be.orient(kps, &peaks)) return rc;
        std::vector<FeatOriented> ori;
        for (size_t q = 0; q < kps.size(); ++q)
            for (int j = 0; j < peaks[q].n; ++j)
                ori.push_back(FeatOriented{kps[q].x, kps[q].y, kps[q].layer, peaks[q].bin[j], kps[q].px, kps[q].py, kps[q].s, peaks[q].theta[j]});
        if (ori.empty()) continue;
        std::vector<float> desc;
        if (int rc = be.describe(ori, &desc)) return rc;
        const double f = std::ldexp(1.0, o - 1);
        for (const FeatOriented &k : ori) {
            out->xy.push_back((float)(k.px * f));
            out->xy.push_back((float)(k.py * f));
            out->scale.push_back((float)(k.s * f));
            out->angle.push_back((float)k.theta);
            out->octave_layer.push_back(o);
            out->octave_layer.push_back(k.layer);
        }
        out->desc.insert(out->desc.end(), desc.begin(), desc.end());
    }
    return 0;
}

} // namespace pais
