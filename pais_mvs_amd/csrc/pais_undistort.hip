// pais_undistort.hip -- the radial term of an NVM camera taken out of images and measurements (include/pais_undistort.h).
// FP64 throughout; the statements of the header are written once in pais_undistort.hpp and inlined here.
#include <hip/hip_runtime.h>
#include <atomic>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include "../../include/pais_undistort.h"
#include "pais_undistort.hpp"
#include "pais_host.hpp"

static thread_local std::string g_und_err;
static std::atomic<int64_t> g_und_launches{0};
extern "C" const char *pais_undistort_last_error(void) { return g_und_err.c_str(); }
extern "C" int64_t pais_undistort_launches(void) { return g_und_launches.load(); }
extern "C" size_t pais_sizeof_lens(void) { return sizeof(pais_lens); }
static int ufail(const std::string &m) { g_und_err = m; return -1; }
#define UHIP(call)                                                                                    \
    do {                                                                                              \
        hipError_t e_ = (call);                                                                       \
        if (e_ != hipSuccess) { g_und_err = std::string(#call) + ": " + hipGetErrorString(e_); return -2; } \
    } while (0)

constexpr int UND_BLOCK = 256;                  // image: 16 lanes x 16 rows, four adjacent pixels per lane; points: one per lane
constexpr int UND_PX = 4;                       // pixels of one lane: their bytes leave as dwords
constexpr int UND_TILE_W = 16 * UND_PX;         // 64 x 16 pixels per block, 64 x 4 per wave: a wave's taps span a few source rows
constexpr int UND_TILE_H = 16;
constexpr int64_t UND_PIXEL_CAP = 1 << 24;      // pixels of one image launch
constexpr int UND_MAX_TILE_ROWS = 32768;        // gridDim.y of one image launch
constexpr int64_t UND_POINT_CAP = 1 << 22;      // points of one launch

// Rows [yBegin, yEnd) of the output.  One solve per pixel serves all channels; the Newton loop of neighbouring pixels
// differs by a few steps only, so the wave diverges little.
template <int CH>
__global__ __launch_bounds__(UND_BLOCK) void k_undistort_image(pais_lens L, int inverse, const uint8_t *__restrict__ src, long long stride,
                                                               int W, int H, int yBegin, int yEnd, uint8_t *__restrict__ dst,
                                                               uint8_t *__restrict__ mask, unsigned long long *__restrict__ counter)
{
    static_assert(UND_PX == 4 && (UND_PX * CH) % 4 == 0, "a lane's pixels fill whole dwords");
    const long long xl = (long long)blockIdx.x * UND_TILE_W + (long long)(threadIdx.x & 15) * UND_PX; // may pass INT_MAX in the last tile
    const int y = yBegin + (int)blockIdx.y * UND_TILE_H + (int)(threadIdx.x >> 4);
    // byte b of the lane's UND_PX * CH output bytes is bits 8 (b & 3) .. of out[b >> 2]: little-endian, as the dword store lays them
    uint32_t out[CH], m = 0u;
#pragma unroll
    for (int k = 0; k < CH; ++k) out[k] = 0u;
    unsigned int live = 0;
    if (y < yEnd && xl < (long long)W) {
        const int x = (int)xl;
        const int n = W - x < UND_PX ? W - x : UND_PX; // pixels of this lane inside the row
#pragma unroll
        for (int j = 0; j < UND_PX; ++j) {
            if (j >= n) continue;
            const pais::LensTap t = pais::lens_tap(L, inverse != 0, W, H, x + j, y);
            if (!t.ok) continue;
            const uint8_t *r0 = src + (size_t)t.y0 * (size_t)stride, *r1 = src + (size_t)t.y1 * (size_t)stride;
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                const uint32_t v = pais::lens_blend(t, r0[(size_t)t.x0 * CH + c], r0[(size_t)t.x1 * CH + c], r1[(size_t)t.x0 * CH + c],
                                                    r1[(size_t)t.x1 * CH + c]);
                out[(j * CH + c) >> 2] |= v << (8 * ((j * CH + c) & 3));
            }
            m |= 1u << (8 * j);
            ++live;
        }
        const size_t p = (size_t)y * (size_t)W + (size_t)x; // < 2^31: the host refuses larger images
        const size_t off = p * CH;
        if (n == UND_PX && (off & 3u) == 0) {
#pragma unroll
            for (int k = 0; k < CH; ++k) reinterpret_cast<uint32_t *>(dst + off)[k] = out[k];
        } else {
#pragma unroll
            for (int b = 0; b < UND_PX * CH; ++b)
                if (b < n * CH) dst[off + (size_t)b] = (uint8_t)(out[b >> 2] >> (8 * (b & 3)));
        }
        if (mask) {
            if (n == UND_PX && (p & 3u) == 0) {
                *reinterpret_cast<uint32_t *>(mask + p) = m;
            } else {
#pragma unroll
                for (int j = 0; j < UND_PX; ++j)
                    if (j < n) mask[p + (size_t)j] = (uint8_t)(m >> (8 * j));
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) live += __shfl_down(live, o);
    if ((threadIdx.x & 63) == 0 && live) atomicAdd(counter, (unsigned long long)live);
}

// Points [i0, i1): one lane each.
__global__ __launch_bounds__(UND_BLOCK) void k_lens_points(pais_lens L, int inverse, long long i0, long long i1, const double *__restrict__ in,
                                                           double *__restrict__ out, uint8_t *__restrict__ valid)
{
    const long long i = i0 + (long long)blockIdx.x * UND_BLOCK + threadIdx.x;
    if (i >= i1) return;
    const pais::LensPoint p = pais::lens_map(L, inverse != 0, in[2 * i], in[2 * i + 1]);
    out[2 * i] = p.u;
    out[2 * i + 1] = p.v;
    valid[i] = p.ok ? 1 : 0;
}

static long long und_env(const char *name)
{
    const char *s = getenv(name);
    return (s && *s) ? atoll(s) : 0;
}

static int und_check_lens(const char *who, int device, const pais_lens *lens)
{
    const std::string w(who);
    if (!lens) return ufail(w + ": null pointer (lens)");
    if (device < 0) return ufail(w + ": needs a GPU (device < 0): the maps are HIP kernels, nothing is computed on the host");
    if (lens->model != PAIS_LENS_MEASURED_TO_IDEAL && lens->model != PAIS_LENS_IDEAL_TO_MEASURED)
        return ufail(w + ": unknown model " + std::to_string(lens->model));
    const double e[5] = {lens->focal[0], lens->focal[1], lens->pp[0], lens->pp[1], lens->k};
    for (int k = 0; k < 5; ++k)
        if (!std::isfinite(e[k])) return ufail(w + ": lens entry " + std::to_string(k) + " is not finite");
    if (lens->focal[0] == 0.0 || lens->focal[1] == 0.0) return ufail(w + ": focal == 0");
    return 0;
}

namespace {
struct UndEvents {
    hipEvent_t e[2] = {nullptr, nullptr};
    ~UndEvents() { for (int k = 0; k < 2; ++k) if (e[k]) (void)hipEventDestroy(e[k]); }
};
} // namespace

static int und_points(const char *who, int what, int device, const pais_lens *lens, int64_t n, const double *in, double *out, uint8_t *valid,
                      double *kernel_ms)
{
    const std::string w(who);
    if (n < 0) return ufail(w + ": negative count");
    if (int rc = und_check_lens(who, device, lens)) return rc;
    if (n && (!in || !out || !valid)) return ufail(w + ": null pointer");
    for (int64_t k = 0; k < 2 * n; ++k)
        if (!std::isfinite(in[k])) {
            char buf[160];
            snprintf(buf, sizeof(buf), "%s: point %lld entry %d is not finite (%g)", who, (long long)(k / 2), (int)(k % 2), in[k]);
            return ufail(buf);
        }
    if (kernel_ms) *kernel_ms = 0.0;
    if (n == 0) return 0;
    const long long forced = und_env("PAIS_UNDISTORT_POINTS");
    const int64_t per = forced > 0 && forced < UND_POINT_CAP ? (int64_t)forced : UND_POINT_CAP;
    const int inverse = pais::lens_uses_inverse(lens->model, what) ? 1 : 0;

    UHIP(hipSetDevice(device));
    DevBuf<double> din, dout; // freed on every return path
    DevBuf<uint8_t> dvalid;
    UHIP(din.alloc(sizeof(double) * 2 * (size_t)n));
    UHIP(dout.alloc(sizeof(double) * 2 * (size_t)n));
    UHIP(dvalid.alloc((size_t)n));
    UHIP(hipMemcpy(din, in, sizeof(double) * 2 * (size_t)n, hipMemcpyHostToDevice));
    UndEvents ev;
    UHIP(hipEventCreate(&ev.e[0]));
    UHIP(hipEventCreate(&ev.e[1]));
    UHIP(hipEventRecord(ev.e[0], 0));
    for (int64_t i0 = 0; i0 < n; i0 += per) {
        const int64_t i1 = i0 + per < n ? i0 + per : n;
        const unsigned blocks = (unsigned)((i1 - i0 + UND_BLOCK - 1) / UND_BLOCK);
        hipLaunchKernelGGL(k_lens_points, dim3(blocks), dim3(UND_BLOCK), 0, 0, *lens, inverse, (long long)i0, (long long)i1, (const double *)din,
                           (double *)dout, (uint8_t *)dvalid);
        ++g_und_launches;
        UHIP(hipGetLastError());
    }
    UHIP(hipEventRecord(ev.e[1], 0));
    UHIP(hipEventSynchronize(ev.e[1]));
    float ms = 0;
    UHIP(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
    UHIP(hipMemcpy(out, dout, sizeof(double) * 2 * (size_t)n, hipMemcpyDeviceToHost));
    UHIP(hipMemcpy(valid, dvalid, (size_t)n, hipMemcpyDeviceToHost));
    if (kernel_ms) *kernel_ms = (double)ms;
    return 0;
}

extern "C" int pais_undistort_points(int device, const pais_lens *lens, int64_t n, const double *xy_measured, double *xy_ideal, uint8_t *valid,
                                     double *kernel_ms)
{
    return und_points("pais_undistort_points", pais::LENS_UNDISTORT_POINTS, device, lens, n, xy_measured, xy_ideal, valid, kernel_ms);
}

extern "C" int pais_distort_points(int device, const pais_lens *lens, int64_t n, const double *xy_ideal, double *xy_measured, uint8_t *valid,
                                   double *kernel_ms)
{
    return und_points("pais_distort_points", pais::LENS_DISTORT_POINTS, device, lens, n, xy_ideal, xy_measured, valid, kernel_ms);
}

extern "C" int pais_undistort_image(int device, const pais_lens *lens, int channels, const uint8_t *src, int width, int height, int64_t stride,
                                    uint8_t *dst, uint8_t *mask, int64_t *valid_pixels, double *kernel_ms)
{
    const char *who = "pais_undistort_image";
    const std::string w(who);
    if (channels != 1 && channels != 3) return ufail(w + ": channels must be 1 or 3, got " + std::to_string(channels));
    if (width < 1 || height < 1) return ufail(w + ": width and height must be at least 1");
    if ((long long)width * height > (long long)INT_MAX) return ufail(w + ": width x height exceeds 2^31 - 1 pixels");
    if (stride < (int64_t)width * channels) return ufail(w + ": stride " + std::to_string((long long)stride) + " < width x channels");
    if (!src || !dst) return ufail(w + ": null pointer");
    if (int rc = und_check_lens(who, device, lens)) return rc;

    const long long forced = und_env("PAIS_UNDISTORT_ROWS");
    long long rows = forced > 0 ? forced : UND_PIXEL_CAP / width;
    if (rows > (long long)UND_MAX_TILE_ROWS * UND_TILE_H) rows = (long long)UND_MAX_TILE_ROWS * UND_TILE_H;
    rows = (rows + UND_TILE_H - 1) / UND_TILE_H * UND_TILE_H; // whole tiles, at least one
    if (rows < UND_TILE_H) rows = UND_TILE_H;
    const int inverse = pais::lens_uses_inverse(lens->model, pais::LENS_IMAGE) ? 1 : 0;
    const size_t pix = (size_t)width * (size_t)height;
    const size_t srcBytes = (size_t)stride * (size_t)(height - 1) + (size_t)width * (size_t)channels; // the last row ends with its pixels

    UHIP(hipSetDevice(device));
    DevBuf<uint8_t> dsrc, ddst, dmask; // freed on every return path
    DevBuf<unsigned long long> counter;
    UHIP(dsrc.alloc(srcBytes));
    UHIP(ddst.alloc(pix * (size_t)channels));
    if (mask) UHIP(dmask.alloc(pix));
    UHIP(counter.alloc(sizeof(unsigned long long)));
    UHIP(hipMemcpy(dsrc, src, srcBytes, hipMemcpyHostToDevice));
    UHIP(hipMemset(counter, 0, sizeof(unsigned long long)));
    UndEvents ev;
    UHIP(hipEventCreate(&ev.e[0]));
    UHIP(hipEventCreate(&ev.e[1]));
    UHIP(hipEventRecord(ev.e[0], 0));
    const unsigned gx = (unsigned)(((long long)width + UND_TILE_W - 1) / UND_TILE_W);
    for (long long y0 = 0; y0 < height; y0 += rows) {
        const int y1 = (int)(y0 + rows < height ? y0 + rows : height);
        const dim3 grid(gx, (unsigned)((y1 - (int)y0 + UND_TILE_H - 1) / UND_TILE_H)), block(UND_BLOCK);
        if (channels == 1)
            hipLaunchKernelGGL(k_undistort_image<1>, grid, block, 0, 0, *lens, inverse, (const uint8_t *)dsrc, (long long)stride, width, height,
                               (int)y0, y1, (uint8_t *)ddst, (uint8_t *)dmask, (unsigned long long *)counter);
        else
            hipLaunchKernelGGL(k_undistort_image<3>, grid, block, 0, 0, *lens, inverse, (const uint8_t *)dsrc, (long long)stride, width, height,
                               (int)y0, y1, (uint8_t *)ddst, (uint8_t *)dmask, (unsigned long long *)counter);
        ++g_und_launches;
        UHIP(hipGetLastError());
    }
    UHIP(hipEventRecord(ev.e[1], 0));
    UHIP(hipEventSynchronize(ev.e[1]));
    float ms = 0;
    UHIP(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
    UHIP(hipMemcpy(dst, ddst, pix * (size_t)channels, hipMemcpyDeviceToHost));
    if (mask) UHIP(hipMemcpy(mask, dmask, pix, hipMemcpyDeviceToHost));
    unsigned long long cnt = 0;
    UHIP(hipMemcpy(&cnt, counter, sizeof(cnt), hipMemcpyDeviceToHost));
    if (valid_pixels) *valid_pixels = (int64_t)cnt;
    if (kernel_ms) *kernel_ms = (double)ms;
    return 0;
}
