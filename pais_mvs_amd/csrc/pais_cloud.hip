// pais_cloud.hip -- exact nearest neighbour between two point sets (include/pais_cloud.h): the search behind the accuracy
// and completeness of a cloud against ground truth (pais_mvs_amd/evaluate.py).  All pairs, FP64, difference form -- the
// |q|^2 + |t|^2 - 2 q.t form (and with it the FP64 MFMA) cancels at the very scale the scores live on.
// pais_cloud_knn is the same walk with a sorted list of k per query in registers, pais_cloud_outlier_rule
// the statistical outlier rule over its table; pais_cloud_planes fits a plane to every row of that table on the device
// (pais_plane.hpp).
#include <hip/hip_runtime.h>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include "../../include/pais_cloud.h"
#include "pais_cloud_internal.hpp"
#include "pais_dev.hpp"
#include "pais_host.hpp"
#include "pais_plane.hpp"

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

// CLOUD_BLOCK (pais_cloud_internal.hpp): queries per block, one per thread
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

static int check_finite(const char *who, const char *what, int n, const double *p)
{
    for (size_t k = 0; k < 3 * (size_t)n; ++k)
        if (!std::isfinite(p[k])) {
            char buf[160];
            snprintf(buf, sizeof(buf), "%s: %s[%zu] coordinate %d is not finite (%g)", who, what, k / 3, (int)(k % 3), p[k]);
            return cfail(buf);
        }
    return 0;
}

static long env_long(const char *name)
{
    const char *s = getenv(name);
    return (s && *s) ? atol(s) : 0;
}

// The split of one search: slices of whole tiles, none of them empty, chosen for >= two blocks per CU in a pass and forced by
// PAIS_CLOUD_SLICES (the k-nearest search measured fastest under the same rule); `chunk` queries per pass
// (PAIS_CLOUD_CHUNK), shrunk until the slices x chunk x perQuery partial entries of a pass fit CLOUD_PARTIAL_CAP.
// (struct CloudSplit: pais_cloud_internal.hpp)
static CloudSplit cloud_split(int nq, int nt, size_t perQuery)
{
    const int tiles = (int)(((long long)nt + CLOUD_TILE - 1) / CLOUD_TILE);
    const long forcedSlices = env_long("PAIS_CLOUD_SLICES"), forcedChunk = env_long("PAIS_CLOUD_CHUNK");
    const size_t cap = CLOUD_PARTIAL_CAP / perQuery;
    CloudSplit sp{(size_t)nq, 0, 0};
    if (forcedChunk > 0 && (size_t)forcedChunk < sp.chunk) sp.chunk = (size_t)forcedChunk;
    for (;;) {
        const long qBlocks = (long)((sp.chunk + CLOUD_BLOCK - 1) / CLOUD_BLOCK);
        long want = forcedSlices > 0 ? forcedSlices : (CLOUD_MIN_BLOCKS + qBlocks - 1) / qBlocks;
        if (want > PAIS_CLOUD_MAX_SLICES) want = PAIS_CLOUD_MAX_SLICES;
        if (want > tiles) want = tiles;
        sp.tilesPerSlice = (int)((tiles + want - 1) / want);
        sp.slices = (tiles + sp.tilesPerSlice - 1) / sp.tilesPerSlice;
        if (sp.chunk * (size_t)sp.slices <= cap || sp.chunk <= CLOUD_BLOCK) break;
        sp.chunk = ((cap / (size_t)sp.slices) / CLOUD_BLOCK) * CLOUD_BLOCK; // fewer queries per pass -> maybe more slices: again
        if (sp.chunk < CLOUD_BLOCK) sp.chunk = CLOUD_BLOCK;
    }
    return sp;
}

// hipEvents around the kernels of one search, destroyed on every return path (struct CloudTimer: pais_cloud_internal.hpp)
CloudTimer::~CloudTimer() { for (int k = 0; k < 2; ++k) if (ev[k]) (void)hipEventDestroy(ev[k]); }
int CloudTimer::start()
{
    CHIP(hipEventCreate(&ev[0]));
    CHIP(hipEventCreate(&ev[1]));
    CHIP(hipEventRecord(ev[0], 0));
    return 0;
}
int CloudTimer::stop(double *kernel_ms)
{
    CHIP(hipGetLastError());
    CHIP(hipEventRecord(ev[1], 0));
    CHIP(hipEventSynchronize(ev[1]));
    float ms = 0;
    CHIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
    if (kernel_ms) *kernel_ms = (double)ms;
    return 0;
}

extern "C" int pais_cloud_nearest(int device, int nq, const double *queries, int nt, const double *targets, int32_t *nearest,
                                  double *dist2, double *kernel_ms)
{
    if (nq < 0 || nt < 0) return cfail("pais_cloud_nearest: negative count");
    if (nq == 0) return 0;
    if (!queries || !targets || !nearest || !dist2) return cfail("pais_cloud_nearest: null pointer");
    if (nt == 0) return cfail("pais_cloud_nearest: no targets (nt == 0): the nearest of nothing is undefined");
    if (device < 0) return cfail("pais_cloud_nearest: needs a GPU (device < 0): the search is a HIP kernel, nothing is computed on the host");
    if (check_finite("pais_cloud_nearest", "queries", nq, queries) || check_finite("pais_cloud_nearest", "targets", nt, targets)) return -1;

    const CloudSplit sp = cloud_split(nq, nt, 1);
    const size_t chunk = sp.chunk;
    const int tilesPerSlice = sp.tilesPerSlice, slices = sp.slices;

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
    CloudTimer timer;
    double ms = 0;
    if (timer.start()) return -2;
    for (size_t q0 = 0; q0 < (size_t)nq; q0 += chunk) {
        const int n = (int)(((size_t)nq - q0) < chunk ? ((size_t)nq - q0) : chunk);
        const int qBlocks = (n + CLOUD_BLOCK - 1) / CLOUD_BLOCK;
        hipLaunchKernelGGL(k_cloud_nearest, dim3(qBlocks, slices), dim3(CLOUD_BLOCK), 0, 0, dq + 3 * q0, n, dt, nt, tilesPerSlice, pd, pi);
        hipLaunchKernelGGL(k_cloud_reduce, dim3(qBlocks), dim3(CLOUD_BLOCK), 0, 0, pd, pi, n, slices, di + q0, dd + q0);
        g_cloud_launches += 2;
    }
    if (timer.stop(&ms)) return -2;
    CHIP(hipMemcpy(nearest, di, sizeof(int32_t) * (size_t)nq, hipMemcpyDeviceToHost));
    CHIP(hipMemcpy(dist2, dd, sizeof(double) * (size_t)nq, hipMemcpyDeviceToHost));
    if (kernel_ms) *kernel_ms = ms;
    return 0;
}

// ------------------------------------------------------------------------------------------------ k nearest ---
// The one order of the k-nearest search, in the search kernel, the merge kernel and the definition: (d2 ascending, target
// index ascending).  An empty list slot is (+inf, KNN_EMPTY), after every real pair, so the fill phase, +inf distances and
// ties need no counter and no case of their own.
constexpr int32_t KNN_EMPTY = INT32_MAX;
constexpr int KNN_GROUP = 8; // pairs whose distances are tested against the list's last entry under ONE branch

__device__ __forceinline__ bool knn_before(double d, int32_t i, double D, int32_t I) { return d < D || (d == D && i < I); }

// A query's running list: KCAP (d2, index) pairs in ascending order, statically indexed, so it lives in registers.
template <int KCAP> struct KnnList {
    double d[KCAP];
    int32_t i[KCAP];
    __device__ __forceinline__ void clear(double fill)
    {
#pragma unroll
        for (int s = 0; s < KCAP; ++s) { d[s] = fill; i[s] = KNN_EMPTY; }
    }
    __device__ __forceinline__ bool admits(double cd, int32_t ci) const { return knn_before(cd, ci, d[KCAP - 1], i[KCAP - 1]); }
    // Insert a pair that admits() passed: slot s takes its lower neighbour if the pair goes before that one, the pair if
    // it goes before the slot's own entry, else it stays.  Every compare reads the list as it was, none waits for another.
    __device__ __forceinline__ void insert(double cd, int32_t ci)
    {
        bool here = true;
#pragma unroll
        for (int s = KCAP - 1; s > 0; --s) {
            const bool below = knn_before(cd, ci, d[s - 1], i[s - 1]);
            d[s] = below ? d[s - 1] : (here ? cd : d[s]);
            i[s] = below ? i[s - 1] : (here ? ci : i[s]);
            here = below;
        }
        if (here) { d[0] = cd; i[0] = ci; }
    }
};

// Targets [j0, j1) of the staged tile against one query, pair by pair in index order; `self` is the target index the query
// ignores (-1: none).  The slow path of k_cloud_knn: rolled, so that a kernel holds the unrolled insertion once.
template <int KCAP>
__device__ __forceinline__ void knn_scan(KnnList<KCAP> &L, const double *tile, double qx, double qy, double qz, int j0, int j1, int32_t b0,
                                         int32_t self)
{
#pragma unroll 1
    for (int j = j0; j < j1; ++j) {
        const double dx = qx - tile[j], dy = qy - tile[CLOUD_TILE + j], dz = qz - tile[2 * CLOUD_TILE + j];
        const double d2 = ((dx * dx) + (dy * dy)) + (dz * dz);
        const int32_t t = b0 + j;
        if (t != self && L.admits(d2, t)) L.insert(d2, t);
    }
}

// k_cloud_nearest's grid, tiles and distance statements; what differs is the selection.  A group of KNN_GROUP pairs is
// rejected by one compare of its smallest distance against the list's last distance (`<=`: a tie or a +inf may still enter
// an empty slot) and one branch; a rejected pair then costs its eight FP64 operations and one v_min_f64.  Only when a lane passes
// is the group walked again by knn_scan under the full order.  The last entry only ever decreases, so the test made with
// the value from before the group rejects nothing that the order admits.  The query's own index passes the test (d2 = 0)
// and is dropped in knn_scan, so skipping it costs the fast path nothing.  Slice partials: partD / partI[(slice KCAP + s) nq
// + query], s < k (a prefix of a sorted list is the shorter list).
template <int KCAP>
__global__ __launch_bounds__(CLOUD_BLOCK) void k_cloud_knn(const double *__restrict__ queries, int nq, int32_t self0,
                                                           const double *__restrict__ targets, int nt, int tilesPerSlice, int k,
                                                           double *__restrict__ partD, int32_t *__restrict__ partI)
{
    __shared__ double tile[3 * CLOUD_TILE];
    const int i = blockIdx.x * CLOUD_BLOCK + threadIdx.x;
    const bool has = i < nq;
    const double qx = has ? queries[3 * (size_t)i] : 0, qy = has ? queries[3 * (size_t)i + 1] : 0, qz = has ? queries[3 * (size_t)i + 2] : 0;
    const int32_t self = (self0 < 0 || !has) ? -1 : self0 + i; // the query's index in the whole set, not in this pass
    const long long begin = (long long)blockIdx.y * tilesPerSlice * CLOUD_TILE;
    const long long stop = begin + (long long)tilesPerSlice * CLOUD_TILE;
    const long long end = stop < nt ? stop : nt;
    KnnList<KCAP> L;
    L.clear(has ? INFINITY : -INFINITY); // a lane without a query admits nothing
    for (long long base = begin; base < end; base += CLOUD_TILE) {
        const int m = (int)((end - base) < CLOUD_TILE ? (end - base) : CLOUD_TILE);
        __syncthreads();
        for (int e = threadIdx.x; e < 3 * m; e += CLOUD_BLOCK) tile[(e % 3) * CLOUD_TILE + e / 3] = targets[3 * (size_t)base + e];
        __syncthreads();
        const int32_t b0 = (int32_t)base;
        int j = 0;
        for (; j + KNN_GROUP <= m; j += KNN_GROUP) {
            const double last = L.d[KCAP - 1];
            double lo[KNN_GROUP];
#pragma unroll
            for (int u = 0; u < KNN_GROUP; ++u) {
                const double dx = qx - tile[j + u], dy = qy - tile[CLOUD_TILE + j + u], dz = qz - tile[2 * CLOUD_TILE + j + u];
                lo[u] = ((dx * dx) + (dy * dy)) + (dz * dz);
            }
#pragma unroll
            for (int w = KNN_GROUP / 2; w > 0; w /= 2)
#pragma unroll
                for (int u = 0; u < w; ++u) lo[u] = fmin(lo[u], lo[u + w]); // no NaN: the coordinates are finite
            if (lo[0] <= last) knn_scan<KCAP>(L, tile, qx, qy, qz, j, j + KNN_GROUP, b0, self);
        }
        knn_scan<KCAP>(L, tile, qx, qy, qz, j, m, b0, self);
    }
    if (has) {
#pragma unroll
        for (int s = 0; s < KCAP; ++s)
            if (s < k) {
                partD[((size_t)blockIdx.y * KCAP + s) * nq + i] = L.d[s];
                partI[((size_t)blockIdx.y * KCAP + s) * nq + i] = L.i[s];
            }
    }
}

// The slice lists of one query merged in slice order under the same order: what one walk over all targets leaves.  A slice's
// list ascends, so its first entry that the merged list does not admit ends that slice (its empty slots never enter).
template <int KCAP>
__global__ __launch_bounds__(CLOUD_BLOCK) void k_cloud_knn_merge(const double *__restrict__ partD, const int32_t *__restrict__ partI,
                                                                 int nq, int slices, int k, int32_t *__restrict__ index,
                                                                 double *__restrict__ dist2)
{
    const int i = blockIdx.x * CLOUD_BLOCK + threadIdx.x;
    if (i >= nq) return;
    KnnList<KCAP> L;
    L.clear(INFINITY);
    for (int s = 0; s < slices; ++s)
        for (int e = 0; e < k; ++e) {
            const size_t at = ((size_t)s * KCAP + e) * nq + i;
            const double d = partD[at];
            const int32_t t = partI[at];
            if (!L.admits(d, t)) break;
            L.insert(d, t);
        }
#pragma unroll
    for (int s = 0; s < KCAP; ++s)
        if (s < k) {
            index[(size_t)i * k + s] = L.i[s] == KNN_EMPTY ? -1 : L.i[s];
            dist2[(size_t)i * k + s] = L.d[s];
        }
}

template <int KCAP>
static void knn_launch(int qBlocks, int slices, const double *q, int n, int32_t self0, const double *t, int nt, int tilesPerSlice, int k,
                       double *pd, int32_t *pi, int32_t *index, double *dist2)
{
    hipLaunchKernelGGL(k_cloud_knn<KCAP>, dim3(qBlocks, slices), dim3(CLOUD_BLOCK), 0, 0, q, n, self0, t, nt, tilesPerSlice, k, pd, pi);
    hipLaunchKernelGGL(k_cloud_knn_merge<KCAP>, dim3(qBlocks), dim3(CLOUD_BLOCK), 0, 0, pd, pi, n, slices, k, index, dist2);
}

// What pais_cloud_knn and pais_cloud_planes refuse alike, under the caller's name; outNull: the caller's own test of its output
// pointers.  1: nq == 0, nothing to do.
int knn_check(const std::string &who, int device, int flags, int known, int k, int nq, const double *queries, int nt,
              const double *targets, bool outNull)
{
    if (k < 1 || k > PAIS_CLOUD_MAX_K) return cfail(who + ": k = " + std::to_string(k) + " outside [1, " + std::to_string(PAIS_CLOUD_MAX_K) + "]");
    if (flags & ~known) return cfail(who + ": unknown flag bits in " + std::to_string(flags));
    if (nq < 0 || nt < 0) return cfail(who + ": negative count");
    if ((flags & PAIS_KNN_SKIP_SAME_INDEX) && nq != nt) return cfail(who + ": PAIS_KNN_SKIP_SAME_INDEX is for a set against itself (nq != nt)");
    if (nq == 0) return 1;
    if (!queries || !targets || outNull) return cfail(who + ": null pointer");
    if (nt == 0) return cfail(who + ": no targets (nt == 0)");
    if (device < 0) return cfail(who + ": needs a GPU (device < 0): the search is a HIP kernel, nothing is computed on the host");
    if (check_finite(who.c_str(), "queries", nq, queries) || check_finite(who.c_str(), "targets", nt, targets)) return -1;
    return 0;
}

// The k-nearest search of checked arguments, its table left on the device: dq, dt the two point sets, di / dd the nq x k table
// (row-major), sp the split it ran under, ms its search and merge kernels.  Everything is freed with the struct (KnnTable:
// pais_cloud_internal.hpp).
int knn_device(int device, bool skip, int k, int nq, const double *queries, int nt, const double *targets, KnnTable &T)
{
    const int kcap = k <= 1 ? 1 : k <= 8 ? 8 : k <= 16 ? 16 : 32; // the smallest instantiation that holds k
    const CloudSplit sp = T.sp = cloud_split(nq, nt, (size_t)kcap);
    const size_t part = sp.chunk * (size_t)sp.slices * (size_t)kcap, out = (size_t)nq * (size_t)k;

    CHIP(hipSetDevice(device));
    DevBuf<double> pd; // freed on every return path
    DevBuf<int32_t> pi;
    CHIP(T.dq.alloc(sizeof(double) * 3 * (size_t)nq));
    CHIP(T.dt.alloc(sizeof(double) * 3 * (size_t)nt));
    CHIP(T.dd.alloc(sizeof(double) * out));
    CHIP(T.di.alloc(sizeof(int32_t) * out));
    CHIP(pd.alloc(sizeof(double) * part));
    CHIP(pi.alloc(sizeof(int32_t) * part));
    CHIP(hipMemcpy(T.dq, queries, sizeof(double) * 3 * (size_t)nq, hipMemcpyHostToDevice));
    CHIP(hipMemcpy(T.dt, targets, sizeof(double) * 3 * (size_t)nt, hipMemcpyHostToDevice));
    CloudTimer timer;
    if (timer.start()) return -2;
    for (size_t q0 = 0; q0 < (size_t)nq; q0 += sp.chunk) {
        const int n = (int)(((size_t)nq - q0) < sp.chunk ? ((size_t)nq - q0) : sp.chunk);
        const int qBlocks = (n + CLOUD_BLOCK - 1) / CLOUD_BLOCK;
        const int32_t self0 = skip ? (int32_t)q0 : -1;
        auto go = kcap == 1 ? knn_launch<1> : kcap == 8 ? knn_launch<8> : kcap == 16 ? knn_launch<16> : knn_launch<32>;
        go(qBlocks, sp.slices, T.dq + 3 * q0, n, self0, T.dt, nt, sp.tilesPerSlice, k, pd, pi, T.di + q0 * (size_t)k, T.dd + q0 * (size_t)k);
        g_cloud_launches += 2;
    }
    if (timer.stop(&T.ms)) return -2;
    return 0;
}
static int knn_fetch(const KnnTable &T, size_t out, int32_t *index, double *dist2)
{
    CHIP(hipMemcpy(index, T.di, sizeof(int32_t) * out, hipMemcpyDeviceToHost));
    CHIP(hipMemcpy(dist2, T.dd, sizeof(double) * out, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int pais_cloud_knn(int device, int flags, int k, int nq, const double *queries, int nt, const double *targets, int32_t *index,
                              double *dist2, double *kernel_ms)
{
    const int bad = knn_check("pais_cloud_knn", device, flags, PAIS_KNN_SKIP_SAME_INDEX, k, nq, queries, nt, targets, !index || !dist2);
    if (bad) return bad < 0 ? bad : 0;
    KnnTable T;
    if (int rc = knn_device(device, flags & PAIS_KNN_SKIP_SAME_INDEX, k, nq, queries, nt, targets, T)) return rc;
    if (int rc = knn_fetch(T, (size_t)nq * (size_t)k, index, dist2)) return rc;
    if (kernel_ms) *kernel_ms = T.ms;
    return 0;
}

// --------------------------------------------------------------------------------------------------- plane fits ---
// One lane per query of the pass: pais::plane_fit (pais_plane.hpp) over its row of the table.  The row is read where the merge
// kernel wrote it (row-major: a lane walks k consecutive entries, so every line it touches is used whole), the
// neighbours are gathered from the whole target array.  The sweep loop of the eigen-solve is the only divergent part.
__global__ __launch_bounds__(CLOUD_BLOCK) void k_cloud_planes(const double *__restrict__ queries, int nq, const int32_t *__restrict__ index,
                                                              int k, int withQuery, const double *__restrict__ targets, int nt,
                                                              const double *__restrict__ toward, pais_plane *__restrict__ planes)
{
    const int i = blockIdx.x * CLOUD_BLOCK + threadIdx.x;
    if (i >= nq) return;
    planes[i] = pais::plane_fit(withQuery != 0, queries[3 * (size_t)i], queries[3 * (size_t)i + 1], queries[3 * (size_t)i + 2], k,
                                index + (size_t)i * k, nt, targets, toward ? toward + 3 * (size_t)i : nullptr, nullptr);
}

static thread_local double g_planes_ms[2] = {0, 0};
extern "C" void pais_cloud_planes_last_ms(double ms[2])
{
    if (ms) { ms[0] = g_planes_ms[0]; ms[1] = g_planes_ms[1]; }
}
extern "C" size_t pais_sizeof_plane(void) { return sizeof(pais_plane); }

extern "C" int pais_cloud_planes(int device, int flags, int k, int nq, const double *queries, int nt, const double *targets,
                                 const double *toward, pais_plane *planes, int32_t *index, double *dist2, double *kernel_ms)
{
    const std::string who = "pais_cloud_planes";
    const int bad = knn_check(who, device, flags, PAIS_KNN_SKIP_SAME_INDEX | PAIS_PLANE_WITH_QUERY | PAIS_PLANE_ORIENT, k, nq, queries, nt,
                              targets, !index != !dist2);
    if (bad) return bad < 0 ? bad : 0;
    const bool orient = flags & PAIS_PLANE_ORIENT;
    if (!planes) return cfail(who + ": null planes");
    if (orient && !toward) return cfail(who + ": PAIS_PLANE_ORIENT without toward");
    if (!orient && toward) return cfail(who + ": toward without PAIS_PLANE_ORIENT");
    if (orient && check_finite(who.c_str(), "toward", nq, toward)) return -1;

    KnnTable T;
    if (int rc = knn_device(device, flags & PAIS_KNN_SKIP_SAME_INDEX, k, nq, queries, nt, targets, T)) return rc;
    DevBuf<double> dw;
    DevBuf<pais_plane> dp;
    CHIP(dp.alloc(sizeof(pais_plane) * (size_t)nq));
    if (orient) {
        CHIP(dw.alloc(sizeof(double) * 3 * (size_t)nq));
        CHIP(hipMemcpy(dw, toward, sizeof(double) * 3 * (size_t)nq, hipMemcpyHostToDevice));
    }
    CloudTimer timer;
    double ms = 0;
    if (timer.start()) return -2;
    for (size_t q0 = 0; q0 < (size_t)nq; q0 += T.sp.chunk) { // the passes of the search
        const int n = (int)(((size_t)nq - q0) < T.sp.chunk ? ((size_t)nq - q0) : T.sp.chunk);
        hipLaunchKernelGGL(k_cloud_planes, dim3((n + CLOUD_BLOCK - 1) / CLOUD_BLOCK), dim3(CLOUD_BLOCK), 0, 0, T.dq + 3 * q0, n,
                           T.di + q0 * (size_t)k, k, (flags & PAIS_PLANE_WITH_QUERY) ? 1 : 0, T.dt, nt, orient ? dw + 3 * q0 : nullptr, dp + q0);
        g_cloud_launches += 1;
    }
    if (timer.stop(&ms)) return -2;
    CHIP(hipMemcpy(planes, dp, sizeof(pais_plane) * (size_t)nq, hipMemcpyDeviceToHost));
    if (index && knn_fetch(T, (size_t)nq * (size_t)k, index, dist2)) return -2;
    g_planes_ms[0] = T.ms;
    g_planes_ms[1] = ms;
    if (kernel_ms) *kernel_ms = T.ms + ms;
    return 0;
}

extern "C" int pais_cloud_normal_rule(int n, const pais_plane *planes, const double *normals, double min_cos, uint8_t *outlier)
{
    if (n < 0 || (n &&(!planes || !normals || !outlier))) return cfail("pais_cloud_normal_rule: bad argument");
    for (int i = 0; i < n; ++i) {
        const double *g = planes[i].normal, *p = normals + 3 * (size_t)i;
        outlier[i] = planes[i].status == PAIS_PLANE_OK && std::fabs(((g[0] * p[0]) + (g[1] * p[1])) + (g[2] * p[2])) < min_cos;
    }
    return 0;
}

// include/pais_cloud.h: the statements in their order, every sum sequential
extern "C" int pais_cloud_outlier_rule(int n, int k, const int32_t *index, const double *dist2, double sigma, double *mean_dist, double stats[3],
                                       uint8_t *outlier)
{
    if (n < 0 || k < 1 || !stats || (n && (!index || !dist2 || !mean_dist || !outlier))) return cfail("pais_cloud_outlier_rule: bad argument");
    bool rows = true; // every row has a valid entry
    double sum = 0;
    for (int i = 0; i < n; ++i) {
        double s = 0;
        int ki = 0;
        for (int j = 0; j < k; ++j)
            if (index[(size_t)i * k + j] >= 0) {
                s += std::sqrt(dist2[(size_t)i * k + j]);
                ++ki;
            }
        if (!ki) rows = false;
        mean_dist[i] = ki ? s / (double)ki : (double)NAN;
        sum += mean_dist[i];
        outlier[i] = 0;
    }
    const double mu = n ? sum / (double)n : (double)NAN;
    double ss = 0;
    for (int i = 0; i < n; ++i) ss += (mean_dist[i] - mu) * (mean_dist[i] - mu);
    const double sd = n > 1 ? std::sqrt(ss / (double)(n - 1)) : (double)NAN;
    const double threshold = mu + sigma * sd;
    stats[0] = mu;
    stats[1] = sd;
    stats[2] = threshold;
    if (n < 2 || !rows || !std::isfinite(mu) || !std::isfinite(sd)) return 0;
    for (int i = 0; i < n; ++i) outlier[i] = mean_dist[i] > threshold;
    return 0;
}

extern "C" int pais_cloud_normals(int n, const double *normalS, double *normals)
{
    if (n < 0 || (n && (!normalS || !normals))) return cfail("pais_cloud_normals: bad argument");
    for (int i = 0; i < n; ++i) pais::spherical2normal(normalS[2 * i], normalS[2 * i + 1], normals + 3 * (size_t)i);
    return 0;
}
