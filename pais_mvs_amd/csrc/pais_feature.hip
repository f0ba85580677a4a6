// pais_feature.hip -- image features on the GPU (include/pais_feature.h): scale space, extrema, fit, orientation and
// descriptor kernels, and the backend that pais::feat_walk (pais_feature.hpp) drives with them.  Every statement of the
// header lives in pais_feature.hpp; a kernel only decides which lane evaluates which sample.
#include <hip/hip_runtime.h>
#include <atomic>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/pais_feature.h"
#include "../../include/pais_test_hooks.h"
#include "pais_feature.hpp"
#include "pais_host.hpp"

using namespace pais;

static thread_local std::string g_feat_err;
static thread_local double g_feat_stage_ms[5] = {0, 0, 0, 0, 0};
static thread_local double g_feat_blur_bytes = 0.0;
static std::atomic<int64_t> g_feat_launches{0};
extern "C" const char *pais_feature_last_error(void) { return g_feat_err.c_str(); }
extern "C" int64_t pais_feature_launches(void) { return g_feat_launches.load(); }
extern "C" size_t pais_sizeof_feature_params(void) { return sizeof(pais_feature_params); }
extern "C" void pais_feature_default_params(pais_feature_params *p)
{
    if (!p) return;
    p->layers = 3;
    p->_pad = 0;
    p->sigma = 1.6;
    p->input_blur = 0.5;
    p->contrast_threshold = 0.04;
    p->edge_threshold = 10.0;
}
extern "C" void pais_feature_last_stage_ms(double ms[5], double *blur_bytes)
{
    for (int k = 0; ms && k < 5; ++k) ms[k] = g_feat_stage_ms[k];
    if (blur_bytes) *blur_bytes = g_feat_blur_bytes;
}
static int ffail(const std::string &m) { g_feat_err = m; return -1; }
#define FHIP(call)                                                                                   \
    do {                                                                                             \
        hipError_t e_ = (call);                                                                      \
        if (e_ != hipSuccess) { g_feat_err = std::string(#call) + ": " + hipGetErrorString(e_); return -2; } \
    } while (0)

constexpr int FEAT_BLOCK = 256;
enum { ST_BLUR = 0, ST_EXTREMA = 1, ST_FIT = 2, ST_ORIENT = 3, ST_DESCRIBE = 4 };

// One lane per sample of the doubled image.
__global__ __launch_bounds__(FEAT_BLOCK) void k_feat_double(const uint8_t *__restrict__ g, int64_t stride, int W, int H, float *__restrict__ out)
{
    const int X = blockIdx.x * FEAT_BLOCK + threadIdx.x, Y = blockIdx.y;
    if (X >= 2 * W || Y >= 2 * H) return;
    out[(size_t)Y * (size_t)(2 * W) + X] = feat_double_at(g, stride, W, H, X, Y);
}

// HALVING: every second sample of src (Ws wide) into the W x H image dst.
__global__ __launch_bounds__(FEAT_BLOCK) void k_feat_halve(const float *__restrict__ src, int Ws, int W, int H, float *__restrict__ dst)
{
    const int x = blockIdx.x * FEAT_BLOCK + threadIdx.x, y = blockIdx.y;
    if (x >= W || y >= H) return;
    dst[(size_t)y * W + x] = src[(size_t)(2 * y) * Ws + 2 * x];
}

// Row pass: a block takes 256 consecutive samples of one row; the strip and its apron of R samples either side (clamped
// to the row: REPLICATE) are staged in LDS once, then each lane carries its own chain in ascending tap order -- the bits
// do not depend on the tiling.  LDS: (256 + 2R) floats.
__global__ __launch_bounds__(FEAT_BLOCK) void k_feat_blur_rows(const float *__restrict__ src, int W, int H, const float *__restrict__ taps, int R,
                                                               float *__restrict__ dst)
{
    extern __shared__ float strip[];
    const int x0 = blockIdx.x * FEAT_BLOCK, y = blockIdx.y;
    const float *row = src + (size_t)y * W;
    for (int j = threadIdx.x; j < FEAT_BLOCK + 2 * R; j += FEAT_BLOCK) strip[j] = row[feat_clamp(x0 + j - R, W)];
    __syncthreads();
    const int x = x0 + threadIdx.x;
    if (x >= W) return;
    float acc = 0.0f;
    for (int k = 0; k <= 2 * R; ++k) acc = acc + taps[k] * strip[threadIdx.x + k];
    dst[(size_t)y * W + x] = acc;
}

// Column pass: a block takes a strip 64 columns wide and 4 rows tall; lane (cx, ry) walks the taps down its column.  The
// 64 lanes of a wave read 64 consecutive floats per tap, and the four waves of a block share all but three of their rows in
// L1, so nothing is staged.
__global__ __launch_bounds__(FEAT_BLOCK) void k_feat_blur_cols(const float *__restrict__ src, int W, int H, const float *__restrict__ taps, int R,
                                                               float *__restrict__ dst)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    dst[(size_t)y * W + x] = feat_blur_at(src + x, (int64_t)W, y, H, taps, R);
}

// One lane per (x, y) inside the margin and layer 1 .. n; the differences are taken on the fly (two loads and one
// subtraction each: storing them would write and read back as much as it saves).  Candidates are appended through one
// counter; their order is never used (the host sorts by the header's key).  Beyond `cap` only the count grows.
__global__ __launch_bounds__(FEAT_BLOCK) void k_feat_extrema(FeatOctave o, float pre, FeatCand *__restrict__ cands, unsigned int cap,
                                                             unsigned int *__restrict__ counter)
{
    const int x = FEAT_MARGIN + blockIdx.x * FEAT_BLOCK + threadIdx.x, y = FEAT_MARGIN + blockIdx.y, i = 1 + blockIdx.z;
    if (!feat_in_margin(o, x, y) || i > o.n) return;
    if (!feat_is_extremum(o, i, x, y, pre)) return;
    const unsigned int slot = atomicAdd(counter, 1u);
    if (slot < cap) cands[slot] = FeatCand{x, y, i};
}

// One lane per candidate: FP64, branchy, small.
__global__ __launch_bounds__(FEAT_BLOCK) void k_feat_refine(FeatOctave o, const FeatCand *__restrict__ cands, int n, double sigma, double contrast,
                                                            double edge, FeatKp *__restrict__ out)
{
    const int q = blockIdx.x * FEAT_BLOCK + threadIdx.x;
    if (q >= n) return;
    out[q] = feat_refine(o, cands[q].x, cands[q].y, cands[q].layer, sigma, contrast, edge);
}

// One wave per keypoint.  The window is walked 64 samples at a time in the header's order (row outer, column inner): every
// lane evaluates one sample -- loads, gradient, det_exp, det_atan2 -- and parks (bin, value) in LDS; lane 0 then adds the 64
// values to the histogram in sample order.  One accumulator chain per keypoint: the sums do not depend on the lane count.
__global__ __launch_bounds__(64) void k_feat_orient(FeatOctave o, const FeatKp *__restrict__ kps, int n, FeatPeaks *__restrict__ out)
{
    __shared__ double hist[FEAT_ORI_BINS];
    __shared__ double sval[64];
    __shared__ int sbin[64];
    const int q = blockIdx.x, lane = threadIdx.x;
    if (q >= n) return;
    const FeatKp kp = kps[q];
    const float *L = o.L + (size_t)kp.layer * (size_t)o.W * (size_t)o.H;
    const int rad = feat_ori_radius(kp.s), side = 2 * rad + 1;
    const long long total = (long long)side * side;
    if (lane < FEAT_ORI_BINS) hist[lane] = 0.0;
    __syncthreads();
    for (long long base = 0; base < total; base += 64) {
        const long long t = base + lane;
        int b = -1;
        double v = 0.0;
        if (t < total) b = feat_ori_sample(L, o.W, o.H, kp.x, kp.y, kp.s, (int)(t % side) - rad, (int)(t / side) - rad, &v);
        if (__ballot(b >= 0) == 0) continue; // (wave-uniform: the block is one wave)
        sbin[lane] = b;
        sval[lane] = v;
        __syncthreads();
        if (lane == 0)
            for (int j = 0; j < 64; ++j)
                if (sbin[j] >= 0) hist[sbin[j]] = hist[sbin[j]] + sval[j];
        __syncthreads();
    }
    if (lane == 0) {
        FeatPeaks p;
        feat_ori_peaks(hist, &p);
        out[q] = p;
    }
}

// One wave per oriented keypoint, the same discipline: 64 samples evaluated in parallel, their eight trilinear shares
// parked in LDS, lane 0 adds them to the 6 x 6 x 10 histogram in sample order, then folds, normalises and writes the
// 128 floats.
__global__ __launch_bounds__(64) void k_feat_describe(FeatOctave o, const FeatOriented *__restrict__ kps, int n, float *__restrict__ desc)
{
    __shared__ double Hh[FEAT_HIST];
    __shared__ double sv[64][8];
    __shared__ int sidx[64];
    __shared__ float outv[FEAT_DESC];
    const int q = blockIdx.x, lane = threadIdx.x;
    if (q >= n) return;
    const FeatOriented kp = kps[q];
    const float *L = o.L + (size_t)kp.layer * (size_t)o.W * (size_t)o.H;
    const double hw = 3.0 * kp.s;
    const double ct = det_cos(kp.theta) / hw, st = det_sin(kp.theta) / hw;
    const int rad = feat_desc_radius(kp.s, o.W, o.H), side = 2 * rad + 1;
    const long long total = (long long)side * side;
    for (int j = lane; j < FEAT_HIST; j += 64) Hh[j] = 0.0;
    __syncthreads();
    for (long long base = 0; base < total; base += 64) {
        const long long t = base + lane;
        FeatDescSample s;
        s.idx = -1;
        if (t < total) s = feat_desc_sample(L, o.W, o.H, kp.x, kp.y, (int)(t % side) - rad, (int)(t / side) - rad, ct, st, kp.theta);
        if (__ballot(s.idx >= 0) == 0) continue;
        sidx[lane] = s.idx;
        if (s.idx >= 0)
            for (int k = 0; k < 8; ++k) sv[lane][k] = s.v[k];
        __syncthreads();
        if (lane == 0)
            for (int j = 0; j < 64; ++j)
                if (sidx[j] >= 0) feat_desc_add(Hh, sidx[j], sv[j]);
        __syncthreads();
    }
    if (lane == 0) feat_desc_finish(Hh, outv);
    __syncthreads();
    for (int k = lane; k < FEAT_DESC; k += 64) desc[(size_t)q * FEAT_DESC + k] = outv[k];
}

namespace {
// The kernels as the backend of pais::feat_walk: one octave's layers on the device at a time.
struct GpuFeatures {
    int W = 0, H = 0, n = 0;          // the current octave
    int W0 = 0, H0 = 0;               // the input
    double sigma = 0, contrast = 0, edge = 0;
    const uint8_t *d_gray = nullptr;
    int64_t stride = 0;
    DevBuf<float> layers, next, tmp, taps; // n + 3 layers; the next octave's L_0; the row pass's output; one tap table
    DevBuf<FeatCand> cands;
    DevBuf<FeatKp> kps;
    DevBuf<FeatPeaks> peaks;
    DevBuf<FeatOriented> oriented;
    DevBuf<float> desc;
    DevBuf<unsigned int> counter;
    size_t candCap = 0;
    hipEvent_t ev[2] = {nullptr, nullptr};
    double stageMs[5] = {0, 0, 0, 0, 0};
    double blurBytes = 0.0;

    ~GpuFeatures()
    {
        for (int k = 0; k < 2; ++k)
            if (ev[k]) (void)hipEventDestroy(ev[k]);
    }
    FeatOctave view() const { return FeatOctave{layers, W, H, n}; }
    size_t px() const { return (size_t)W * (size_t)H; }
    int begin() { FHIP(hipEventRecord(ev[0], 0)); return 0; }
    int end(int stage) // the stage's launches are done (the caller synchronises with a copy, or here)
    {
        FHIP(hipGetLastError());
        FHIP(hipEventRecord(ev[1], 0));
        FHIP(hipEventSynchronize(ev[1]));
        float ms = 0;
        FHIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
        stageMs[stage] += (double)ms;
        return 0;
    }
    template <class T> int room(DevBuf<T> &b, size_t count)
    {
        if (sizeof(T) * count > b.bytes) FHIP(b.alloc(sizeof(T) * count + sizeof(T) * count / 2));
        return 0;
    }
    // dst = BLUR(src): rows into tmp, columns into dst
    int blur(const float *src, float *dst, const float *hostTaps, int R)
    {
        FHIP(hipMemcpy(taps, hostTaps, sizeof(float) * (size_t)(2 * R + 1), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_feat_blur_rows, dim3((W + FEAT_BLOCK - 1) / FEAT_BLOCK, H), dim3(FEAT_BLOCK), sizeof(float) * (size_t)(FEAT_BLOCK + 2 * R), 0,
                           src, W, H, (const float *)taps, R, (float *)tmp);
        hipLaunchKernelGGL(k_feat_blur_cols, dim3((W + 63) / 64, (H + 3) / 4), dim3(FEAT_BLOCK), 0, 0, (const float *)tmp, W, H, (const float *)taps, R, dst);
        g_feat_launches += 2;
        blurBytes += 4.0 * sizeof(float) * (double)px();
        return 0;
    }
    int octave0(int Wo, int Ho, const float *t, int R)
    {
        W = Wo; H = Ho;
        if (int rc = room(layers, px() * (size_t)(n + 3))) return rc;
        if (int rc = room(tmp, px())) return rc;
        if (int rc = room(next, px())) return rc;
        if (int rc = begin()) return rc;
        hipLaunchKernelGGL(k_feat_double, dim3((W + FEAT_BLOCK - 1) / FEAT_BLOCK, H), dim3(FEAT_BLOCK), 0, 0, d_gray, stride, W0, H0, (float *)next);
        ++g_feat_launches;
        blurBytes += (double)W0 * H0 + sizeof(float) * (double)px();
        if (int rc = blur(next, layers, t, R)) return rc;
        return end(ST_BLUR);
    }
    int halve()
    {
        const int Ws = W;
        const float *src = layers + (size_t)n * px();
        W /= 2; H /= 2;
        if (int rc = begin()) return rc;
        hipLaunchKernelGGL(k_feat_halve, dim3((W + FEAT_BLOCK - 1) / FEAT_BLOCK, H), dim3(FEAT_BLOCK), 0, 0, src, Ws, W, H, (float *)next);
        ++g_feat_launches;
        // (the layers of the octave before are dead once `next` is written: the new L_0 may land on them)
        FHIP(hipMemcpyAsync(layers, next, sizeof(float) * px(), hipMemcpyDeviceToDevice, 0));
        blurBytes += 4.0 * sizeof(float) * (double)px();
        return end(ST_BLUR);
    }
    int layer(int i, const float *t, int R)
    {
        if (int rc = begin()) return rc;
        if (int rc = blur(layers + (size_t)(i - 1) * px(), layers + (size_t)i * px(), t, R)) return rc;
        return end(ST_BLUR);
    }
    int extrema(float pre, std::vector<FeatCand> *out)
    {
        const int iw = W - 2 * FEAT_MARGIN, ih = H - 2 * FEAT_MARGIN;
        if (iw < 1 || ih < 1) return 0;
        for (;;) {
            if (int rc = begin()) return rc;
            FHIP(hipMemsetAsync(counter, 0, sizeof(unsigned int), 0));
            hipLaunchKernelGGL(k_feat_extrema, dim3((iw + FEAT_BLOCK - 1) / FEAT_BLOCK, ih, n), dim3(FEAT_BLOCK), 0, 0, view(), pre, (FeatCand *)cands,
                               (unsigned int)candCap, (unsigned int *)counter);
            ++g_feat_launches;
            if (int rc = end(ST_EXTREMA)) return rc;
            unsigned int found = 0;
            FHIP(hipMemcpy(&found, counter, sizeof(found), hipMemcpyDeviceToHost));
            if ((size_t)found > candCap) { // nothing is dropped: room for all of them, and the same launch again
                candCap = (size_t)found;
                FHIP(cands.alloc(sizeof(FeatCand) * candCap));
                continue;
            }
            out->resize(found);
            if (found) FHIP(hipMemcpy(out->data(), cands, sizeof(FeatCand) * found, hipMemcpyDeviceToHost));
            return 0;
        }
    }
    int refine(const std::vector<FeatCand> &c, std::vector<FeatKp> *out)
    {
        const int m = (int)c.size(); // (still on the device from extrema(), in the same order)
        if (int rc = room(kps, (size_t)m)) return rc;
        if (int rc = begin()) return rc;
        hipLaunchKernelGGL(k_feat_refine, dim3((m + FEAT_BLOCK - 1) / FEAT_BLOCK), dim3(FEAT_BLOCK), 0, 0, view(), (const FeatCand *)cands, m, sigma, contrast,
                           edge, (FeatKp *)kps);
        ++g_feat_launches;
        if (int rc = end(ST_FIT)) return rc;
        out->resize((size_t)m);
        FHIP(hipMemcpy(out->data(), kps, sizeof(FeatKp) * (size_t)m, hipMemcpyDeviceToHost));
        return 0;
    }
    int orient(const std::vector<FeatKp> &k, std::vector<FeatPeaks> *out)
    {
        const int m = (int)k.size();
        if (int rc = room(kps, (size_t)m)) return rc;
        if (int rc = room(peaks, (size_t)m)) return rc;
        FHIP(hipMemcpy(kps, k.data(), sizeof(FeatKp) * (size_t)m, hipMemcpyHostToDevice));
        if (int rc = begin()) return rc;
        hipLaunchKernelGGL(k_feat_orient, dim3(m), dim3(64), 0, 0, view(), (const FeatKp *)kps, m, (FeatPeaks *)peaks);
        ++g_feat_launches;
        if (int rc = end(ST_ORIENT)) return rc;
        out->resize((size_t)m);
        FHIP(hipMemcpy(out->data(), peaks, sizeof(FeatPeaks) * (size_t)m, hipMemcpyDeviceToHost));
        return 0;
    }
    int describe(const std::vector<FeatOriented> &k, std::vector<float> *out)
    {
        const int m = (int)k.size();
        if (int rc = room(oriented, (size_t)m)) return rc;
        if (int rc = room(desc, (size_t)m * FEAT_DESC)) return rc;
        FHIP(hipMemcpy(oriented, k.data(), sizeof(FeatOriented) * (size_t)m, hipMemcpyHostToDevice));
        if (int rc = begin()) return rc;
        hipLaunchKernelGGL(k_feat_describe, dim3(m), dim3(64), 0, 0, view(), (const FeatOriented *)oriented, m, (float *)desc);
        ++g_feat_launches;
        if (int rc = end(ST_DESCRIBE)) return rc;
        out->resize((size_t)m * FEAT_DESC);
        FHIP(hipMemcpy(out->data(), desc, sizeof(float) * (size_t)m * FEAT_DESC, hipMemcpyDeviceToHost));
        return 0;
    }
};
} // namespace

static int feat_check_params(const pais_feature_params *prm, FeatParams *p)
{
    pais_feature_params d;
    pais_feature_default_params(&d);
    if (prm) d = *prm;
    if (d.layers < 1 || d.layers > FEAT_MAX_LAYERS) return ffail("pais_feature_detect: layers " + std::to_string(d.layers) + " outside 1 .. 8");
    const double v[4] = {d.sigma, d.input_blur, d.contrast_threshold, d.edge_threshold};
    const char *name[4] = {"sigma", "input_blur", "contrast_threshold", "edge_threshold"};
    for (int k = 0; k < 4; ++k)
        if (!std::isfinite(v[k]) || !(v[k] > 0.0)) return ffail(std::string("pais_feature_detect: ") + name[k] + " is not a positive finite number");
    *p = FeatParams{d.layers, d.sigma, d.input_blur, d.contrast_threshold, d.edge_threshold};
    if (feat_max_radius(*p) < 0) return ffail("pais_feature_detect: a blur radius above " + std::to_string(FEAT_MAX_RADIUS) + " (sigma too large)");
    return 0;
}

// The argument checks of pais_feature_detect (and of the stage hook below, which takes the same image).
static int feat_check_image(int width, int height, int64_t stride)
{
    if (width < 1 || height < 1) return ffail("pais_feature_detect: width and height must be at least 1");
    if (width > (1 << 24) || height > (1 << 24) || (long long)width * height > (long long)(INT_MAX / 4))
        return ffail("pais_feature_detect: the doubled image exceeds 2^31 - 1 samples");
    if (2 * height > 65535) return ffail("pais_feature_detect: height above 32767 (a launch holds one block row per row of the doubled image)");
    if (stride < (int64_t)width) return ffail("pais_feature_detect: stride < width");
    return 0;
}

// The image on the device and the backend's fixed buffers: what a walk needs before its first octave.
static int feat_open(GpuFeatures &g, DevBuf<uint8_t> &dgray, int device, const uint8_t *gray, int width, int height, int64_t stride, const FeatParams &p)
{
    FHIP(hipSetDevice(device));
    g.n = p.layers; g.W0 = width; g.H0 = height; g.sigma = p.sigma; g.contrast = p.contrast; g.edge = p.edge; g.stride = (int64_t)width;
    FHIP(dgray.alloc((size_t)width * (size_t)height));
    FHIP(hipMemcpy2D(dgray, (size_t)width, gray, (size_t)stride, (size_t)width, (size_t)height, hipMemcpyHostToDevice));
    g.d_gray = dgray;
    FHIP(g.taps.alloc(sizeof(float) * (size_t)(2 * FEAT_MAX_RADIUS + 1)));
    FHIP(g.counter.alloc(sizeof(unsigned int)));
    const char *env = getenv("PAIS_FEATURE_CANDS"); // the first capacity of the candidate buffer (tests: growth)
    const long forced = (env && *env) ? atol(env) : 0;
    g.candCap = forced > 0 ? (size_t)forced : (size_t)1 << 16;
    FHIP(g.cands.alloc(sizeof(FeatCand) * g.candCap));
    FHIP(hipEventCreate(&g.ev[0]));
    FHIP(hipEventCreate(&g.ev[1]));
    return 0;
}

extern "C" int pais_feature_detect(int device, const uint8_t *gray, int width, int height, int64_t stride, const pais_feature_params *prm,
                                   int max_keypoints, int32_t *num, float *xy, float *scale, float *angle, int32_t *octave_layer, float *desc,
                                   double *kernel_ms)
{
    if (!gray || !num) return ffail("pais_feature_detect: null pointer");
    if (max_keypoints < 0) return ffail("pais_feature_detect: max_keypoints < 0");
    if (max_keypoints > 0 && (!xy || !scale || !angle || !octave_layer || !desc)) return ffail("pais_feature_detect: null output array");
    if (feat_check_image(width, height, stride)) return -1;
    FeatParams p;
    if (feat_check_params(prm, &p)) return -1;
    if (device < 0) return ffail("pais_feature_detect: needs a GPU (device < 0): the detector is HIP kernels, nothing is computed on the host");

    GpuFeatures g; // frees its buffers on every return path
    DevBuf<uint8_t> dgray;
    if (int rc = feat_open(g, dgray, device, gray, width, height, stride, p)) return rc;
    FeatResult r;
    if (int rc = feat_walk(g, width, height, p, &r)) return rc;
    for (int k = 0; k < 5; ++k) g_feat_stage_ms[k] = g.stageMs[k];
    g_feat_blur_bytes = g.blurBytes;
    if (r.count() > (int64_t)INT_MAX) return ffail("pais_feature_detect: more than 2^31 - 1 keypoints");
    *num = (int32_t)r.count();
    const size_t w = (size_t)std::min<int64_t>(r.count(), (int64_t)max_keypoints);
    for (size_t k = 0; k < w; ++k) {
        xy[2 * k] = r.xy[2 * k]; xy[2 * k + 1] = r.xy[2 * k + 1];
        scale[k] = r.scale[k];
        angle[k] = r.angle[k];
        octave_layer[2 * k] = r.octave_layer[2 * k]; octave_layer[2 * k + 1] = r.octave_layer[2 * k + 1];
    }
    if (w) memcpy(desc, r.desc.data(), sizeof(float) * FEAT_DESC * w);
    if (kernel_ms) *kernel_ms = g.stageMs[0] + g.stageMs[1] + g.stageMs[2] + g.stageMs[3] + g.stageMs[4];
    return 0;
}

// ------------------------------------------------------------------------------------------- include/pais_test_hooks.h ---
namespace {
// The backend of pais_test_feature_stages: GpuFeatures behind a recorder.  Every call of the walk is forwarded as it comes;
// after extrema() and refine() of the wanted octave what they left is copied to the host.
struct FeatRecorder {
    GpuFeatures &g;
    int want;
    int octave = -1, W = 0, H = 0;
    bool seen = false;
    std::vector<float> layers;
    std::vector<FeatCand> cands;
    std::vector<FeatKp> fit;

    int octave0(int Wo, int Ho, const float *t, int R) { ++octave; return g.octave0(Wo, Ho, t, R); }
    int halve() { ++octave; return g.halve(); }
    int layer(int i, const float *t, int R) { return g.layer(i, t, R); }
    int extrema(float pre, std::vector<FeatCand> *out)
    {
        if (int rc = g.extrema(pre, out)) return rc;
        if (octave != want) return 0;
        seen = true;
        W = g.W; H = g.H;
        layers.resize(g.px() * (size_t)(g.n + 3));
        FHIP(hipMemcpy(layers.data(), g.layers, sizeof(float) * layers.size(), hipMemcpyDeviceToHost));
        cands = *out;
        return 0;
    }
    int refine(const std::vector<FeatCand> &c, std::vector<FeatKp> *out)
    {
        if (int rc = g.refine(c, out)) return rc;
        if (octave == want) fit = *out;
        return 0;
    }
    int orient(const std::vector<FeatKp> &k, std::vector<FeatPeaks> *out) { return g.orient(k, out); }
    int describe(const std::vector<FeatOriented> &k, std::vector<float> *out) { return g.describe(k, out); }
};
} // namespace

extern "C" int pais_test_feature_stages(int device, const uint8_t *gray, int width, int height, int64_t stride, const pais_feature_params *prm,
                                        int octave, pais_test_feature_sizes *sizes, int64_t layer_floats, float *layers, int max_cands,
                                        int32_t *cands, int32_t *fit_int, double *fit_val)
{
    if (!gray || !sizes) return ffail("pais_test_feature_stages: null pointer");
    if (octave < 0 || layer_floats < 0 || max_cands < 0) return ffail("pais_test_feature_stages: negative octave or capacity");
    if ((layer_floats > 0 && !layers) || (max_cands > 0 && (!cands || !fit_int || !fit_val))) return ffail("pais_test_feature_stages: null output array");
    if (feat_check_image(width, height, stride)) return -1;
    FeatParams p;
    if (feat_check_params(prm, &p)) return -1;
    if (device < 0) return ffail("pais_test_feature_stages: needs a GPU (device < 0)");

    GpuFeatures g;
    DevBuf<uint8_t> dgray;
    if (int rc = feat_open(g, dgray, device, gray, width, height, stride, p)) return rc;
    FeatRecorder rec{g, octave};
    FeatResult r;
    if (int rc = feat_walk(rec, width, height, p, &r)) return rc;
    sizes->octaves = rec.octave + 1;
    sizes->W = rec.W;
    sizes->H = rec.H;
    sizes->layers = rec.seen ? p.layers + 3 : 0;
    sizes->num_cands = (int64_t)rec.cands.size();
    sizes->num_fit = (int64_t)rec.fit.size();
    sizes->num_keypoints = r.count();
    if (!rec.layers.empty() && (int64_t)rec.layers.size() <= layer_floats) memcpy(layers, rec.layers.data(), sizeof(float) * rec.layers.size());
    if ((int64_t)rec.cands.size() <= (int64_t)max_cands) {
        for (size_t k = 0; k < rec.cands.size(); ++k) {
            cands[3 * k] = rec.cands[k].x; cands[3 * k + 1] = rec.cands[k].y; cands[3 * k + 2] = rec.cands[k].layer;
        }
        for (size_t k = 0; k < rec.fit.size(); ++k) {
            const FeatKp &f = rec.fit[k];
            fit_int[4 * k] = f.x; fit_int[4 * k + 1] = f.y; fit_int[4 * k + 2] = f.layer; fit_int[4 * k + 3] = f.ok;
            fit_val[3 * k] = f.px; fit_val[3 * k + 1] = f.py; fit_val[3 * k + 2] = f.s;
        }
    }
    return 0;
}
