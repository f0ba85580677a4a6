// pais_cloud.hip -- exact nearest neighbour between two point sets (include/pais_cloud.h): the search behind the accuracy
// and completeness of a cloud against ground truth (pais_mvs_amd/evaluate.py).  All pairs, FP64, difference form -- the
// |q|^2 + |t|^2 - 2 q.t form (and with it the FP64 MFMA) cancels at the very scale the scores live on.
#include <hip/hip_runtime.h>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include "../../include/pais_cloud.h"
#include "pais_dev.hpp"
#include "pais_host.hpp"

static thread_local std::string g_cloud_err;
static std::atomic<int64_t> g_cloud_launches{0};
extern "C" const char *pais_cloud_last_error(void) { return g_cloud_err.c_str(); }
extern "C" int64_t pais_cloud_launches(void) { return g_cloud_launches.load(); }
static int cfail(const std::string &m) { g_cloud_err = m; return -1; }
#define CHIP(call)                                                                                   \
    do {                                                                                             \
        hipError_t e_ = (call);                                                                      \
        if (e_ != hipSuccess) { g_cloud_err = std::string(#call) + ": " + hipGetErrorString(e_); return -2; } \
    } while (0)

constexpr int CLOUD_BLOCK = 256; // queries per block, one per thread
constexpr int CLOUD_TILE = 512;  // targets per LDS tile: 12 KB, so LDS never bounds the blocks resident on a CU
constexpr int CLOUD_MIN_BLOCKS = 512;           // two blocks for each of the 256 CUs
constexpr size_t CLOUD_PARTIAL_CAP = 4u << 20;  // (slice, query) partials held at once: 48 MB

// Block (bx, by): queries 256 bx .. of this pass against the target slice by = tiles [by tilesPerSlice, (by + 1) tilesPerSlice).
// A tile is staged in LDS as three arrays (x, y, z); in the inner loop every lane reads the SAME address, which LDS
// broadcasts without a bank conflict, so the loop is bound by its eight v_mul_f64 / v_add_f64 per pair.  The running
// (min, index) moves under strict `<` while the targets ascend: the lowest index among equal distances.  The loop is
// unrolled so that independent distances fill the FP64 latency of the one dependent compare-and-select chain.
__global__ __launch_bounds__(CLOUD_BLOCK) void k_cloud_nearest(const double *__restrict__ queries, int nq, const double *__restrict__ targets,
                                                               int nt, int tilesPerSlice, double *__restrict__ partD,
                                                               int32_t *__restrict__ partI)
{
    __shared__ double tile[3 * CLOUD_TILE];
    const int i = blockIdx.x * CLOUD_BLOCK + threadIdx.x;
    const bool has = i < nq;
    const double qx = has ? queries[3 * (size_t)i] : 0, qy = has ? queries[3 * (size_t)i + 1] : 0, qz = has ? queries[3 * (size_t)i + 2] : 0;
    const long long begin = (long long)blockIdx.y * tilesPerSlice * CLOUD_TILE;
    const long long stop = begin + (long long)tilesPerSlice * CLOUD_TILE;
    const long long end = stop < nt ? stop : nt;
    double best = INFINITY;
    int32_t bi = (int32_t)begin; // every distance of the slice infinite: its first target, as a sequential scan from +inf leaves it
    for (long long base = begin; base < end; base += CLOUD_TILE) {
        const int m = (int)((end - base) < CLOUD_TILE ? (end - base) : CLOUD_TILE);
        __syncthreads();
        for (int e = threadIdx.x; e < 3 * m; e += CLOUD_BLOCK) tile[(e % 3) * CLOUD_TILE + e / 3] = targets[3 * (size_t)base + e];
        __syncthreads();
        const int32_t b0 = (int32_t)base;
#pragma unroll 8
        for (int j = 0; j < m; ++j) {
            const double dx = qx - tile[j], dy = qy - tile[CLOUD_TILE + j], dz = qz - tile[2 * CLOUD_TILE + j];
            const double d2 = ((dx * dx) + (dy * dy)) + (dz * dz);
            if (d2 < best) {
                best = d2;
                bi = b0 + j;
            }
        }
    }
    if (has) {
        partD[(size_t)blockIdx.y * nq + i] = best;
        partI[(size_t)blockIdx.y * nq + i] = bi;
    }
}

// The partials of one query in slice order under the same strict `<`: what one scan over all targets leaves.
__global__ __launch_bounds__(CLOUD_BLOCK) void k_cloud_reduce(const double *__restrict__ partD, const int32_t *__restrict__ partI, int nq,
                                                              int slices, int32_t *__restrict__ nearest, double *__restrict__ dist2)
{
    const int i = blockIdx.x * CLOUD_BLOCK + threadIdx.x;
    if (i >= nq) return;
    double best = partD[i];
    int32_t bi = partI[i];
    for (int s = 1; s < slices; ++s) {
        const double d = partD[(size_t)s * nq + i];
        if (d < best) {
            best = d;
            bi = partI[(size_t)s * nq + i];
        }
    }
    nearest[i] = bi;
    dist2[i] = best;
}

static int check_finite(const char *what, int n, const double *p)
{
    for (size_t k = 0; k < 3 * (size_t)n; ++k)
        if (!std::isfinite(p[k])) {
            char buf[160];
            snprintf(buf, sizeof(buf), "pais_cloud_nearest: %s[%zu] coordinate %d is not finite (%g)", what, k / 3, (int)(k % 3), p[k]);
            return cfail(buf);
        }
    return 0;
}

static long env_long(const char *name)
{
    const char *s = getenv(name);
    return (s && *s) ? atol(s) : 0;
}

extern "C" int pais_cloud_nearest(int device, int nq, const double *queries, int nt, const double *targets, int32_t *nearest,
                                  double *dist2, double *kernel_ms)
{
    if (nq < 0 || nt < 0) return cfail("pais_cloud_nearest: negative count");
    if (nq == 0) return 0;
    if (!queries || !targets || !nearest || !dist2) return cfail("pais_cloud_nearest: null pointer");
    if (nt == 0) return cfail("pais_cloud_nearest: no targets (nt == 0): the nearest of nothing is undefined");
    if (device < 0) return cfail("pais_cloud_nearest: needs a GPU (device < 0): the search is a HIP kernel, nothing is computed on the host");
    if (check_finite("queries", nq, queries) || check_finite("targets", nt, targets)) return -1;

    // the split: slices of whole tiles, none of them empty; chosen for >= two blocks per CU, forced by PAIS_CLOUD_SLICES
    const int tiles = (int)(((long long)nt + CLOUD_TILE - 1) / CLOUD_TILE);
    const long forcedSlices = env_long("PAIS_CLOUD_SLICES"), forcedChunk = env_long("PAIS_CLOUD_CHUNK");
    size_t chunk = (size_t)nq;
    if (forcedChunk > 0 && (size_t)forcedChunk < chunk) chunk = (size_t)forcedChunk;
    int tilesPerSlice = 0, slices = 0;
    for (;;) {
        const long qBlocks = (long)((chunk + CLOUD_BLOCK - 1) / CLOUD_BLOCK);
        long want = forcedSlices > 0 ? forcedSlices : (CLOUD_MIN_BLOCKS + qBlocks - 1) / qBlocks;
        if (want > PAIS_CLOUD_MAX_SLICES) want = PAIS_CLOUD_MAX_SLICES;
        if (want > tiles) want = tiles;
        tilesPerSlice = (int)((tiles + want - 1) / want);
        slices = (tiles + tilesPerSlice - 1) / tilesPerSlice;
        if (chunk * (size_t)slices <= CLOUD_PARTIAL_CAP || chunk <= CLOUD_BLOCK) break;
        chunk = ((CLOUD_PARTIAL_CAP / (size_t)slices) / CLOUD_BLOCK) * CLOUD_BLOCK; // fewer queries per pass -> maybe more slices: again
    }

    CHIP(hipSetDevice(device));
    DevBuf<double> dq, dt, dd, pd; // freed on every return path
    DevBuf<int32_t> di, pi;
    CHIP(dq.alloc(sizeof(double) * 3 * (size_t)nq));
    CHIP(dt.alloc(sizeof(double) * 3 * (size_t)nt));
    CHIP(dd.alloc(sizeof(double) * (size_t)nq));
    CHIP(di.alloc(sizeof(int32_t) * (size_t)nq));
    CHIP(pd.alloc(sizeof(double) * chunk * (size_t)slices));
    CHIP(pi.alloc(sizeof(int32_t) * chunk * (size_t)slices));
    CHIP(hipMemcpy(dq, queries, sizeof(double) * 3 * (size_t)nq, hipMemcpyHostToDevice));
    CHIP(hipMemcpy(dt, targets, sizeof(double) * 3 * (size_t)nt, hipMemcpyHostToDevice));
    hipEvent_t ev[2] = {nullptr, nullptr};
    struct EvGuard {
        hipEvent_t *e;
        ~EvGuard() { for (int k = 0; k < 2; ++k) if (e[k]) (void)hipEventDestroy(e[k]); }
    } guard{ev};
    CHIP(hipEventCreate(&ev[0]));
    CHIP(hipEventCreate(&ev[1]));
    CHIP(hipEventRecord(ev[0], 0));
    for (size_t q0 = 0; q0 < (size_t)nq; q0 += chunk) {
        const int n = (int)(((size_t)nq - q0) < chunk ? ((size_t)nq - q0) : chunk);
        const int qBlocks = (n + CLOUD_BLOCK - 1) / CLOUD_BLOCK;
        hipLaunchKernelGGL(k_cloud_nearest, dim3(qBlocks, slices), dim3(CLOUD_BLOCK), 0, 0, dq + 3 * q0, n, dt, nt, tilesPerSlice, pd, pi);
        hipLaunchKernelGGL(k_cloud_reduce, dim3(qBlocks), dim3(CLOUD_BLOCK), 0, 0, pd, pi, n, slices, di + q0, dd + q0);
        g_cloud_launches += 2;
    }
    CHIP(hipGetLastError());
    CHIP(hipEventRecord(ev[1], 0));
    CHIP(hipEventSynchronize(ev[1]));
    float ms = 0;
    CHIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
    CHIP(hipMemcpy(nearest, di, sizeof(int32_t) * (size_t)nq, hipMemcpyDeviceToHost));
    CHIP(hipMemcpy(dist2, dd, sizeof(double) * (size_t)nq, hipMemcpyDeviceToHost));
    if (kernel_ms) *kernel_ms = (double)ms;
    return 0;
}

extern "C" int pais_cloud_normals(int n, const double *normalS, double *normals)
{
    if (n < 0 || (n && (!normalS || !normals))) return cfail("pais_cloud_normals: bad argument");
    for (int i = 0; i < n; ++i) pais::spherical2normal(normalS[2 * i], normalS[2 * i + 1], normals + 3 * (size_t)i);
    return 0;
}
