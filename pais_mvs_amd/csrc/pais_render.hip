// pais_render.hip -- z-buffered patch splats (include/pais_render.h): a cloud rendered into pinhole views, per view a depth
// map and a patch-id map.  FP64 throughout; the statements of the header are written once (splat_camera, disc_hit) and
// inlined into every kernel that needs them, so the depth pass and the id pass produce the same bits.
// Then the depth test of points against such maps (k_depth_test, statements in pais_vis.hpp), on the caller's maps
// (pais_depth_test) or on a render's while they are still on the device (pais_cloud_visibility).
// A third primitive beside DISC and POINT is the triangle of an indexed mesh (pais_mesh_render, statements in
// pais_raster.hpp): its own setup and walks, the same z-buffer, passes and hook.
#include <hip/hip_runtime.h>
#include <atomic>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <string>
#include "../../include/pais_render.h"
#include "pais_dev.hpp"
#include "pais_host.hpp"
#include "pais_raster.hpp"
#include "pais_vis.hpp"

static thread_local std::string g_render_err;
static thread_local int64_t g_render_counts[5] = {0, 0, 0, 0, 0}; // [4]: packed (triangle, view) pairs
static thread_local double g_mesh_ms[3] = {0.0, 0.0, 0.0};
static thread_local double g_vis_ms[2] = {0.0, 0.0};
static std::atomic<int64_t> g_render_launches{0};
extern "C" const char *pais_render_last_error(void) { return g_render_err.c_str(); }
extern "C" int64_t pais_render_launches(void) { return g_render_launches.load(); }
extern "C" size_t pais_sizeof_view(void) { return sizeof(pais_view); }
extern "C" void pais_cloud_visibility_last_ms(double ms[2])
{
    if (ms) { ms[0] = g_vis_ms[0]; ms[1] = g_vis_ms[1]; }
}
extern "C" void pais_render_last_counts(int64_t *tiles, int64_t *covered_pairs, int64_t *depth_atomics, int64_t *id_atomics)
{
    if (tiles) *tiles = g_render_counts[0];
    if (covered_pairs) *covered_pairs = g_render_counts[1];
    if (depth_atomics) *depth_atomics = g_render_counts[2];
    if (id_atomics) *id_atomics = g_render_counts[3];
}
extern "C" int64_t pais_render_last_packed(void) { return g_render_counts[4]; }
extern "C" void pais_mesh_render_last_ms(double ms[3])
{
    if (ms) { ms[0] = g_mesh_ms[0]; ms[1] = g_mesh_ms[1]; ms[2] = g_mesh_ms[2]; }
}
static int rfail(const std::string &m) { g_render_err = m; return -1; }
#define RHIP(call)                                                                                    \
    do {                                                                                              \
        hipError_t e_ = (call);                                                                       \
        if (e_ != hipSuccess) { g_render_err = std::string(#call) + ": " + hipGetErrorString(e_); return -2; } \
    } while (0)

constexpr int RENDER_BLOCK = 256;                // setup / fill: one lane per element; walk: four waves, one tile each
constexpr int RENDER_TILE = 32;                  // a footprint is cut into tiles of at most 32 x 32 pixels, one wave each
constexpr size_t RENDER_PIXEL_CAP = 16u << 20;   // pixels of one pass of views: 192 MB of depth and id
constexpr size_t RENDER_ITEM_CAP = 1u << 20;     // (splat, view) records of one launch: 80 MB
constexpr size_t RENDER_LIST_CAP = 4u << 20;     // footprint tiles of one launch: 32 MB
constexpr size_t VIS_POINT_CAP = 1u << 20;       // points of one depth-test launch: 4096 blocks per view
constexpr int VIS_VIEW_CAP = 65535;              // views of one depth-test launch: grid.y
constexpr unsigned long long DEPTH_EMPTY = 0x7FF0000000000000ull; // +inf: above the pattern of every positive finite double
constexpr int32_t ID_EMPTY = INT_MAX;

// One (splat, view) pair as the walk kernels read it.
struct RenderItem {
    double c[3], n[3], a, r2; // c', n', a, rho rho (DISC)
    int u0, v0, bw, bh;       // pixel box: origin and size; bw == 0: skipped
};
enum { CNT_LIST = 0, CNT_COVERED = 1, CNT_DEPTH_ATOMICS = 2, CNT_ID_ATOMICS = 3, CNT_PACKED = 4, CNT_N = 5 };

// The third mode of render_device; pais_cloud_render knows DISC and POINT only.
constexpr int RENDER_TRIANGLE = 2;
// A box of at most RENDER_PACK_MAX x RENDER_PACK_MAX pixels goes to the packed walk: RENDER_PACK_LANES lanes per triangle,
// four triangles per wave.  0: every box takes the tile walk (the measurement build of BASELINE.md section 18).
#ifndef RENDER_PACK_MAX
#define RENDER_PACK_MAX 8
#endif
constexpr int RENDER_PACK_LANES = 16;
// One (triangle, view) pair as the triangle walks read it: 104 bytes.
struct TriItem {
    pais::RasterTri t;
    int u0, v0, bw, bh; // pixel box: origin and size; bw == 0: skipped
    int skip, packed;   // pais::RASTER_*; 1: in the packed list
};

// c' = (R c) + T, rows as project_raw evaluates them; n' = R n; a = (n'0 c'0 + n'1 c'1) + n'2 c'2.
__device__ inline void splat_camera(const pais_view &V, const double *c, const double *n, double *cc, double *nc, double *a)
{
    cc[0] = (V.R[0] * c[0] + V.R[1] * c[1] + V.R[2] * c[2]) + V.T[0];
    cc[1] = (V.R[3] * c[0] + V.R[4] * c[1] + V.R[5] * c[2]) + V.T[1];
    cc[2] = (V.R[6] * c[0] + V.R[7] * c[1] + V.R[8] * c[2]) + V.T[2];
    if (n) {
        nc[0] = V.R[0] * n[0] + V.R[1] * n[1] + V.R[2] * n[2];
        nc[1] = V.R[3] * n[0] + V.R[4] * n[1] + V.R[5] * n[2];
        nc[2] = V.R[6] * n[0] + V.R[7] * n[1] + V.R[8] * n[2];
        *a = pais::dot3(nc, cc);
    } else {
        nc[0] = nc[1] = nc[2] = 0.0;
        *a = 0.0;
    }
}

// The DISC statements for pixel (u, v): covered or not, and the depth t.
__device__ inline bool disc_hit(const RenderItem &it, double f0, double f1, double pp0, double pp1, int u, int v, double *tOut)
{
    const double rx = ((double)u - pp0) / f0, ry = ((double)v - pp1) / f1;
    const double den = (it.n[0] * rx + it.n[1] * ry) + it.n[2];
    const double t = it.a / den;
    const double hx = t * rx - it.c[0], hy = t * ry - it.c[1], hz = t - it.c[2];
    const double d2 = ((hx * hx) + (hy * hy)) + (hz * hz);
    *tOut = t;
    return den != 0.0 && isfinite(t) && t > 0.0 && d2 <= it.r2;
}

// Pixels [lo, hi] of one axis that the interval [x - r, x + r] at depths [zlo, zhi] (zlo > 0) can project to, padded by
// one pixel and clipped to [0, size - 1]; false: none.  Anything not finite gives the whole axis.
__device__ inline bool box_axis(double x, double r, double zlo, double zhi, double f, double pp, int size, int *lo, int *hi)
{
    const double xlo = x - r, xhi = x + r;
    const double rlo = xlo < 0.0 ? xlo / zlo : xlo / zhi, rhi = xhi > 0.0 ? xhi / zlo : xhi / zhi;
    const double p1 = f * rlo + pp, p2 = f * rhi + pp;
    double a = fmin(p1, p2), b = fmax(p1, p2);
    *lo = 0;
    *hi = size - 1;
    if (!(isfinite(p1) && isfinite(p2))) return true;
    a = floor(a) - 1.0;
    b = ceil(b) + 1.0;
    if (b < 0.0 || a > (double)(size - 1)) return false;
    if (a > 0.0) *lo = (int)a;
    if (b < (double)(size - 1)) *hi = (int)b;
    return true;
}

// One lane per (splat, view) of the launch: the camera-space record, the skip decisions, a conservative pixel box and
// the box's tiles appended to the work list.  The box only ever removes pixels the statements leave uncovered: a covered
// hit lies within rho of c' in every coordinate, so its ray lies inside the projection of the cube c' +- rho; the cube is
// taken 2^-20 larger and the pixel range one pixel wider, which is far above the rounding of the statements.
__global__ __launch_bounds__(RENDER_BLOCK) void k_render_setup(int mode, int flags, int S, int s0, const double *__restrict__ centers,
                                                               const double *__restrict__ normals, const double *__restrict__ radii,
                                                               double radius, int Vc, const pais_view *__restrict__ views, int W, int H,
                                                               RenderItem *__restrict__ items, unsigned long long *__restrict__ list,
                                                               unsigned long long listCap, unsigned long long *__restrict__ counters)
{
    const long long i = (long long)blockIdx.x * RENDER_BLOCK + threadIdx.x;
    if (i >= (long long)S * Vc) return;
    const int vl = (int)(i / S), s = s0 + (int)(i % S);
    const pais_view &V = views[vl];
    RenderItem it;
    const double *c = centers + 3 * (size_t)s;
    splat_camera(V, c, mode == PAIS_RENDER_DISC ? normals + 3 * (size_t)s : nullptr, it.c, it.n, &it.a);
    int u0 = 0, u1 = -1, v0 = 0, v1 = -1;
    it.r2 = 0.0;
    if (mode == PAIS_RENDER_DISC) {
        const double rho = radii ? radii[s] : radius;
        it.r2 = rho * rho;
        const bool skip = !(it.c[2] > rho) || ((flags & PAIS_RENDER_CULL_BACK) && it.a >= 0.0);
        if (!skip) {
            const double rp = rho * (1.0 + 0x1p-20);
            const double zlo = it.c[2] - rp, zhi = it.c[2] + rp;
            bool any = true;
            u0 = 0; u1 = W - 1; v0 = 0; v1 = H - 1;
            if (zlo > 0.0 && isfinite(zhi)) {
                any = box_axis(it.c[0], rp, zlo, zhi, V.focal[0], V.pp[0], W, &u0, &u1);
                any = box_axis(it.c[1], rp, zlo, zhi, V.focal[1], V.pp[1], H, &v0, &v1) && any;
            }
            if (!any) { u1 = u0 - 1; v1 = v0 - 1; }
        }
    } else {
        const int sz = (int)radius;
        if (it.c[2] > 0.0) {
            double p[2];
            pais::project_raw(V.R, V.T, V.focal, V.pp, 1.0, c, p);
            if (isfinite(p[0]) && isfinite(p[1]) && fabs(p[0]) < 0x1p30 && fabs(p[1]) < 0x1p30) {
                const int ru = pais::cv_round(p[0]), rv = pais::cv_round(p[1]);
                u0 = ru - (sz - 1) / 2; u1 = ru + sz / 2;
                v0 = rv - (sz - 1) / 2; v1 = rv + sz / 2;
                if (u0 < 0) u0 = 0;
                if (v0 < 0) v0 = 0;
                if (u1 > W - 1) u1 = W - 1;
                if (v1 > H - 1) v1 = H - 1;
            }
        }
    }
    const bool live = u1 >= u0 && v1 >= v0;
    it.u0 = u0;
    it.v0 = v0;
    it.bw = live ? u1 - u0 + 1 : 0;
    it.bh = live ? v1 - v0 + 1 : 0;
    items[i] = it;
    if (!live) return;
    const unsigned long long nt = (unsigned long long)((it.bw + RENDER_TILE - 1) / RENDER_TILE) * (unsigned long long)((it.bh + RENDER_TILE - 1) / RENDER_TILE);
    const unsigned long long off = atomicAdd(&counters[CNT_LIST], nt);
    if (off + nt > listCap) return; // the host sees the total, halves the launch and sets up again
    for (unsigned long long k = 0; k < nt; ++k) list[off + k] = ((unsigned long long)i << 32) | k;
}

// One wave per footprint tile; its lanes walk the tile's pixels row by row, 64 at a time.
// PHASE 0, depth: positive finite doubles order as their bit patterns, so the z-buffer is a no-return 64-bit unsigned
// atomic min on the bits.  A plain load first: depth[p] only ever falls, so a stale value is only ever larger and the skip
// it allows is conservative.
// PHASE 1, id: the same statements give the same t; where its bits are the final depth[p], a 32-bit atomic min of the splat
// index -- the lowest index among equal depths.
template <int MODE, int PHASE>
__global__ __launch_bounds__(RENDER_BLOCK) void k_render_walk(const unsigned long long *__restrict__ list, unsigned int total,
                                                              const RenderItem *__restrict__ items, int S, int s0,
                                                              const pais_view *__restrict__ views, int W, int H,
                                                              unsigned long long *depth, int32_t *id, unsigned long long *__restrict__ counters)
{
    const unsigned int w = __builtin_amdgcn_readfirstlane(blockIdx.x * (RENDER_BLOCK / 64) + (threadIdx.x >> 6));
    if (w >= total) return;
    const int lane = threadIdx.x & 63;
    const unsigned long long e = list[w];
    const unsigned int item = (unsigned int)(e >> 32), tile = (unsigned int)e;
    const RenderItem it = items[item];
    const int vl = (int)(item / (unsigned int)S), s = s0 + (int)(item % (unsigned int)S);
    const double f0 = views[vl].focal[0], f1 = views[vl].focal[1], pp0 = views[vl].pp[0], pp1 = views[vl].pp[1];
    const int tilesX = (it.bw + RENDER_TILE - 1) / RENDER_TILE;
    const int tx = (int)(tile % (unsigned int)tilesX), ty = (int)(tile / (unsigned int)tilesX);
    const int x0 = it.u0 + tx * RENDER_TILE, y0 = it.v0 + ty * RENDER_TILE;
    const int tw = min(RENDER_TILE, it.u0 + it.bw - x0), th = min(RENDER_TILE, it.v0 + it.bh - y0);
    if (tw <= 0 || th <= 0) return;
    const int npx = tw * th;
    const size_t base = (size_t)vl * (size_t)H * (size_t)W;
    unsigned int covered = 0, issued = 0;
    for (int q = lane; q < npx; q += 64) {
        const int x = x0 + q % tw, y = y0 + q / tw;
        double t;
        bool hit;
        if (MODE == PAIS_RENDER_DISC) {
            hit = disc_hit(it, f0, f1, pp0, pp1, x, y, &t);
        } else {
            t = it.c[2];
            hit = true;
        }
        if (!hit) continue;
        const size_t p = base + (size_t)y * (size_t)W + (size_t)x;
        const unsigned long long bits = (unsigned long long)__double_as_longlong(t);
        if (PHASE == 0) {
            ++covered;
            if (bits < depth[p]) {
                atomicMin(&depth[p], bits);
                ++issued;
            }
        } else if (bits == depth[p] && s < id[p]) {
            atomicMin(&id[p], s);
            ++issued;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        covered += __shfl_down(covered, o);
        issued += __shfl_down(issued, o);
    }
    if (lane == 0) {
        if (PHASE == 0 && covered) atomicAdd(&counters[CNT_COVERED], (unsigned long long)covered);
        if (issued) atomicAdd(&counters[PHASE == 0 ? CNT_DEPTH_ATOMICS : CNT_ID_ATOMICS], (unsigned long long)issued);
    }
}

// One lane per (triangle, view) of the launch: the three corners in camera space, the record, the skips, the box.  A small
// box is appended to the packed list -- one atomic per wave, the lanes ranked by a ballot -- a larger one cut into tiles
// and appended to the tile list as k_render_setup does.  plist holds S x Vc entries, so it cannot overflow.
__global__ __launch_bounds__(RENDER_BLOCK) void k_tri_setup(int flags, int S, int s0, const double *__restrict__ vertices,
                                                            const int32_t *__restrict__ triangles, int Vc, const pais_view *__restrict__ views,
                                                            int W, int H, TriItem *__restrict__ items, unsigned long long *__restrict__ list,
                                                            unsigned long long listCap, unsigned int *__restrict__ plist,
                                                            unsigned long long *__restrict__ counters)
{
    const long long i = (long long)blockIdx.x * RENDER_BLOCK + threadIdx.x;
    const bool lane_on = i < (long long)S * Vc;
    bool small = false;
    unsigned long long nt = 0;
    if (lane_on) {
        const int vl = (int)(i / S), s = s0 + (int)(i % S);
        const pais_view &V = views[vl];
        const int a = triangles[3 * (size_t)s], b = triangles[3 * (size_t)s + 1], c = triangles[3 * (size_t)s + 2];
        double A[3], B[3], C[3];
        pais::raster_camera(V, vertices + 3 * (size_t)a, A);
        pais::raster_camera(V, vertices + 3 * (size_t)b, B);
        pais::raster_camera(V, vertices + 3 * (size_t)c, C);
        TriItem it;
        pais::raster_setup(a, b, c, A, B, C, &it.t);
        it.skip = pais::raster_skip(flags, a, b, c, A[2], B[2], C[2], it.t.D);
        int u0 = 0, u1 = -1, v0 = 0, v1 = -1;
        if (it.skip == pais::RASTER_LIVE && !pais::raster_box(V, A, B, C, it.t.D, W, H, &u0, &u1, &v0, &v1)) {
            it.skip = pais::RASTER_OFF_IMAGE;
            u1 = u0 - 1;
        }
        const bool live = it.skip == pais::RASTER_LIVE;
        it.u0 = u0;
        it.v0 = v0;
        it.bw = live ? u1 - u0 + 1 : 0;
        it.bh = live ? v1 - v0 + 1 : 0;
        small = live && it.bw <= RENDER_PACK_MAX && it.bh <= RENDER_PACK_MAX;
        it.packed = small ? 1 : 0;
        items[i] = it;
        if (live && !small)
            nt = (unsigned long long)((it.bw + RENDER_TILE - 1) / RENDER_TILE) * (unsigned long long)((it.bh + RENDER_TILE - 1) / RENDER_TILE);
    }
    const unsigned long long vote = __ballot(small);
    if (vote) {
        const int lane = threadIdx.x & 63, leader = __ffsll((long long)vote) - 1;
        unsigned long long off = 0;
        if (lane == leader) off = atomicAdd(&counters[CNT_PACKED], (unsigned long long)__popcll(vote));
        off = __shfl(off, leader);
        if (small) plist[off + (unsigned long long)__popcll(vote & ((1ull << lane) - 1ull))] = (unsigned int)i;
    }
    if (!nt) return;
    const unsigned long long off = atomicAdd(&counters[CNT_LIST], nt);
    if (off + nt > listCap) return; // the host sees the total, halves the launch and sets up again
    for (unsigned long long k = 0; k < nt; ++k) list[off + k] = ((unsigned long long)i << 32) | k;
}

// What both triangle walks do with one pixel: the z-buffer of k_render_walk.
template <int PHASE>
__device__ inline void tri_pixel(const pais::RasterTri &T, double f0, double f1, double pp0, double pp1, int x, int y, size_t base, int W, int s,
                                 unsigned long long *depth, int32_t *id, unsigned int *covered, unsigned int *issued)
{
    double t;
    if (!pais::raster_hit(T, f0, f1, pp0, pp1, x, y, &t)) return;
    const size_t p = base + (size_t)y * (size_t)W + (size_t)x;
    const unsigned long long bits = (unsigned long long)__double_as_longlong(t);
    if (PHASE == 0) {
        ++*covered;
        if (bits < depth[p]) {
            atomicMin(&depth[p], bits);
            ++*issued;
        }
    } else if (bits == depth[p] && s < id[p]) {
        atomicMin(&id[p], s);
        ++*issued;
    }
}

__device__ inline void tri_count(int phase, int lane, unsigned int covered, unsigned int issued, unsigned long long *counters)
{
    for (int o = 32; o > 0; o >>= 1) {
        covered += __shfl_down(covered, o);
        issued += __shfl_down(issued, o);
    }
    if (lane == 0) {
        if (phase == 0 && covered) atomicAdd(&counters[CNT_COVERED], (unsigned long long)covered);
        if (issued) atomicAdd(&counters[phase == 0 ? CNT_DEPTH_ATOMICS : CNT_ID_ATOMICS], (unsigned long long)issued);
    }
}

// The tile walk of a large box: one wave per 32 x 32 tile, as k_render_walk.
template <int PHASE>
__global__ __launch_bounds__(RENDER_BLOCK) void k_tri_walk(const unsigned long long *__restrict__ list, unsigned int total,
                                                           const TriItem *__restrict__ items, int S, int s0, const pais_view *__restrict__ views,
                                                           int W, int H, unsigned long long *depth, int32_t *id,
                                                           unsigned long long *__restrict__ counters)
{
    const unsigned int w = __builtin_amdgcn_readfirstlane(blockIdx.x * (RENDER_BLOCK / 64) + (threadIdx.x >> 6));
    if (w >= total) return;
    const int lane = threadIdx.x & 63;
    const unsigned long long e = list[w];
    const unsigned int item = (unsigned int)(e >> 32), tile = (unsigned int)e;
    const TriItem *it = items + item;
    const pais::RasterTri T = it->t;
    const int u0 = it->u0, v0 = it->v0, bw = it->bw, bh = it->bh;
    const int vl = (int)(item / (unsigned int)S), s = s0 + (int)(item % (unsigned int)S);
    const double f0 = views[vl].focal[0], f1 = views[vl].focal[1], pp0 = views[vl].pp[0], pp1 = views[vl].pp[1];
    const int tilesX = (bw + RENDER_TILE - 1) / RENDER_TILE;
    const int tx = (int)(tile % (unsigned int)tilesX), ty = (int)(tile / (unsigned int)tilesX);
    const int x0 = u0 + tx * RENDER_TILE, y0 = v0 + ty * RENDER_TILE;
    const int tw = min(RENDER_TILE, u0 + bw - x0), th = min(RENDER_TILE, v0 + bh - y0);
    if (tw <= 0 || th <= 0) return;
    const int npx = tw * th;
    const size_t base = (size_t)vl * (size_t)H * (size_t)W;
    unsigned int covered = 0, issued = 0;
    for (int q = lane; q < npx; q += 64) tri_pixel<PHASE>(T, f0, f1, pp0, pp1, x0 + q % tw, y0 + q / tw, base, W, s, depth, id, &covered, &issued);
    tri_count(PHASE, lane, covered, issued, counters);
}

// The packed walk of small boxes: RENDER_PACK_LANES lanes per (triangle, view), four of them per wave; a lane takes every
// sixteenth pixel of its triangle's box (at most four).  The triangles of a marching-tetrahedra mesh are a few pixels
// across, and one wave per box would leave most of its lanes without a pixel.
template <int PHASE>
__global__ __launch_bounds__(RENDER_BLOCK) void k_tri_packed(const unsigned int *__restrict__ plist, unsigned int total,
                                                             const TriItem *__restrict__ items, int S, int s0,
                                                             const pais_view *__restrict__ views, int W, int H, unsigned long long *depth,
                                                             int32_t *id, unsigned long long *__restrict__ counters)
{
    const unsigned int g = (blockIdx.x * RENDER_BLOCK + threadIdx.x) / RENDER_PACK_LANES;
    const int sub = threadIdx.x % RENDER_PACK_LANES;
    unsigned int covered = 0, issued = 0;
    if (g < total) {
        const unsigned int item = plist[g];
        const TriItem *it = items + item;
        const pais::RasterTri T = it->t;
        const int u0 = it->u0, v0 = it->v0, bw = it->bw, npx = it->bw * it->bh;
        const int vl = (int)(item / (unsigned int)S), s = s0 + (int)(item % (unsigned int)S);
        const double f0 = views[vl].focal[0], f1 = views[vl].focal[1], pp0 = views[vl].pp[0], pp1 = views[vl].pp[1];
        const size_t base = (size_t)vl * (size_t)H * (size_t)W;
        for (int q = sub; q < npx; q += RENDER_PACK_LANES)
            tri_pixel<PHASE>(T, f0, f1, pp0, pp1, u0 + q % bw, v0 + q / bw, base, W, s, depth, id, &covered, &issued);
    }
    tri_count(PHASE, threadIdx.x & 63, covered, issued, counters);
}

__global__ __launch_bounds__(RENDER_BLOCK) void k_render_fill(unsigned long long *__restrict__ depth, int32_t *__restrict__ id, size_t n)
{
    const size_t i = (size_t)blockIdx.x * RENDER_BLOCK + threadIdx.x;
    if (i >= n) return;
    depth[i] = DEPTH_EMPTY;
    id[i] = ID_EMPTY;
}

__global__ __launch_bounds__(RENDER_BLOCK) void k_render_finish(int32_t *__restrict__ id, size_t n)
{
    const size_t i = (size_t)blockIdx.x * RENDER_BLOCK + threadIdx.x;
    if (i < n && id[i] == ID_EMPTY) id[i] = -1;
}

// One lane per (point, view) pair: block x covers 256 points of [i0, i1), block y is the view, so the view's sixteen doubles
// are read through a block-uniform address.  Per pair one 8-byte gather from the depth map and, with an id map, one 4-byte
// gather; the statements are vis_test (pais_vis.hpp).  Outputs view-major with row length n: a wave's stores are contiguous.
__global__ __launch_bounds__(RENDER_BLOCK) void k_depth_test(int flags, int n, int i0, int i1, const double *__restrict__ points,
                                                             const pais_view *__restrict__ views, int W, int H,
                                                             const double *__restrict__ depth, const int32_t *__restrict__ id, double tol,
                                                             uint8_t *__restrict__ code, int32_t *__restrict__ occluder,
                                                             double *__restrict__ margin)
{
    const long long i = (long long)i0 + (long long)blockIdx.x * RENDER_BLOCK + threadIdx.x;
    if (i >= (long long)i1) return;
    const size_t vl = blockIdx.y, pix = (size_t)H * (size_t)W;
    const double *c = points + 3 * (size_t)i;
    int32_t occ;
    double m;
    const int k = pais::vis_test(views[vl], c[0], c[1], c[2], W, H, depth + vl * pix, id ? id + vl * pix : nullptr, flags, (int32_t)i, tol,
                                 &occ, &m);
    const size_t o = vl * (size_t)n + (size_t)i;
    code[o] = (uint8_t)k;
    if (occluder) occluder[o] = occ;
    if (margin) margin[o] = m;
}

static long render_env_long(const char *name)
{
    const char *s = getenv(name);
    return (s && *s) ? atol(s) : 0;
}

// Refusals carry the name of the entry the caller called (`who`).
static int render_check_finite(const char *who, const char *what, size_t count, int per, const double *p)
{
    for (size_t k = 0; k < count; ++k)
        if (!std::isfinite(p[k])) {
            char buf[192];
            snprintf(buf, sizeof(buf), "%s: %s[%zu] entry %d is not finite (%g)", who, what, k / per, (int)(k % per), p[k]);
            return rfail(buf);
        }
    return 0;
}

// What every entry refuses about counts and sizes, about the device, and about the views (in the order they are asked).
static int check_sizes(const std::string &who, int n, int num_views, int width, int height)
{
    if (n < 0 || num_views < 0) return rfail(who + ": negative count");
    if (width < 1 || height < 1) return rfail(who + ": width and height must be at least 1");
    if ((long long)width * height > (long long)INT_MAX) return rfail(who + ": width x height exceeds 2^31 - 1 pixels");
    return 0;
}
static int check_device(const std::string &who, int device)
{
    if (device < 0) return rfail(who + ": needs a GPU (device < 0): the renderer is a HIP kernel, nothing is computed on the host");
    return 0;
}
static int check_views(const std::string &who, int num_views, const pais_view *views)
{
    static_assert(sizeof(pais_view) == 16 * sizeof(double), "pais_view is sixteen doubles");
    if (render_check_finite(who.c_str(), "views", 16 * (size_t)num_views, 16, (const double *)views)) return -1;
    for (int v = 0; v < num_views; ++v)
        if (views[v].focal[0] == 0.0 || views[v].focal[1] == 0.0) return rfail(who + ": focal == 0 (view " + std::to_string(v) + ")");
    return 0;
}

namespace {
// One pass of views on the device, and the launches of one range of splats into it.
struct RenderPass {
    int mode, flags, W, H, Vc;
    double radius;
    const double *centers, *normals, *radii;
    const pais_view *views; // first view of the pass
    RenderItem *items;
    unsigned long long *list, *counters, *depth;
    int32_t *id;
    int64_t tiles = 0;
    unsigned long long listed = 0; // tiles in the list after the last setup
    int setups = 0;
    // TRIANGLE: vertices in `centers`, the index triples, the records, the packed list and its length after the last setup,
    // the pairs the packed depth walk took, and the kernel milliseconds of setup / depth phase / id phase
    const int32_t *tris = nullptr;
    TriItem *titems = nullptr;
    unsigned int *plist = nullptr;
    unsigned long long packed = 0;
    int64_t packedPairs = 0;
    double phaseMs[3] = {0.0, 0.0, 0.0};
    hipEvent_t tev[2] = {nullptr, nullptr};

    int timed(int slot)
    {
        RHIP(hipEventRecord(tev[1], 0));
        RHIP(hipEventSynchronize(tev[1]));
        float ms = 0;
        RHIP(hipEventElapsedTime(&ms, tev[0], tev[1]));
        phaseMs[slot] += (double)ms;
        return 0;
    }
    int tri_setup(int s0, int s1, unsigned long long *total)
    {
        const int S = s1 - s0;
        const long long lanes = (long long)S * Vc;
        RHIP(hipMemsetAsync(counters + CNT_LIST, 0, sizeof(unsigned long long), 0));
        RHIP(hipMemsetAsync(counters + CNT_PACKED, 0, sizeof(unsigned long long), 0));
        RHIP(hipEventRecord(tev[0], 0));
        hipLaunchKernelGGL(k_tri_setup, dim3((unsigned)((lanes + RENDER_BLOCK - 1) / RENDER_BLOCK)), dim3(RENDER_BLOCK), 0, 0, flags, S, s0, centers,
                           tris, Vc, views, W, H, titems, list, (unsigned long long)RENDER_LIST_CAP, plist, counters);
        ++g_render_launches;
        ++setups;
        RHIP(hipGetLastError());
        if (int rc = timed(0)) return rc;
        unsigned long long c[CNT_N];
        RHIP(hipMemcpy(c, counters, sizeof(c), hipMemcpyDeviceToHost));
        listed = *total = c[CNT_LIST];
        packed = c[CNT_PACKED];
        return 0;
    }
    int tri_walk(int phase, int s0, int s1, unsigned long long total)
    {
        if (!total && !packed) return 0;
        const int S = s1 - s0;
        RHIP(hipEventRecord(tev[0], 0));
        if (total) {
            const dim3 grid((unsigned)((total + RENDER_BLOCK / 64 - 1) / (RENDER_BLOCK / 64)));
            if (phase == 0) hipLaunchKernelGGL((k_tri_walk<0>), grid, dim3(RENDER_BLOCK), 0, 0, list, (unsigned int)total, titems, S, s0, views, W, H, depth, id, counters);
            else hipLaunchKernelGGL((k_tri_walk<1>), grid, dim3(RENDER_BLOCK), 0, 0, list, (unsigned int)total, titems, S, s0, views, W, H, depth, id, counters);
            ++g_render_launches;
        }
        if (packed) {
            const unsigned perBlock = RENDER_BLOCK / RENDER_PACK_LANES;
            const dim3 grid((unsigned)((packed + perBlock - 1) / perBlock));
            if (phase == 0) hipLaunchKernelGGL((k_tri_packed<0>), grid, dim3(RENDER_BLOCK), 0, 0, plist, (unsigned int)packed, titems, S, s0, views, W, H, depth, id, counters);
            else hipLaunchKernelGGL((k_tri_packed<1>), grid, dim3(RENDER_BLOCK), 0, 0, plist, (unsigned int)packed, titems, S, s0, views, W, H, depth, id, counters);
            ++g_render_launches;
        }
        RHIP(hipGetLastError());
        if (int rc = timed(1 + phase)) return rc;
        if (phase == 0) { tiles += (int64_t)total; packedPairs += (int64_t)packed; }
        return 0;
    }

    int setup(int s0, int s1, unsigned long long *total)
    {
        if (mode == RENDER_TRIANGLE) return tri_setup(s0, s1, total);
        const int S = s1 - s0;
        const long long lanes = (long long)S * Vc;
        RHIP(hipMemsetAsync(counters + CNT_LIST, 0, sizeof(unsigned long long), 0));
        hipLaunchKernelGGL(k_render_setup, dim3((unsigned)((lanes + RENDER_BLOCK - 1) / RENDER_BLOCK)), dim3(RENDER_BLOCK), 0, 0, mode, flags, S, s0,
                           centers, normals, radii, radius, Vc, views, W, H, items, list, (unsigned long long)RENDER_LIST_CAP, counters);
        ++g_render_launches;
        ++setups;
        RHIP(hipGetLastError());
        RHIP(hipMemcpy(total, counters + CNT_LIST, sizeof(unsigned long long), hipMemcpyDeviceToHost));
        listed = *total;
        return 0;
    }
    int walk(int phase, int s0, int s1, unsigned long long total)
    {
        if (mode == RENDER_TRIANGLE) return tri_walk(phase, s0, s1, total);
        if (!total) return 0;
        const dim3 grid((unsigned)((total + RENDER_BLOCK / 64 - 1) / (RENDER_BLOCK / 64))), block(RENDER_BLOCK);
        const int S = s1 - s0;
#define RENDER_WALK(M, P) hipLaunchKernelGGL((k_render_walk<M, P>), grid, block, 0, 0, list, (unsigned int)total, items, S, s0, views, W, H, depth, id, counters)
        if (mode == PAIS_RENDER_DISC) {
            if (phase == 0) RENDER_WALK(PAIS_RENDER_DISC, 0); else RENDER_WALK(PAIS_RENDER_DISC, 1);
        } else {
            if (phase == 0) RENDER_WALK(PAIS_RENDER_POINT, 0); else RENDER_WALK(PAIS_RENDER_POINT, 1);
        }
#undef RENDER_WALK
        ++g_render_launches;
        RHIP(hipGetLastError());
        if (phase == 0) tiles += (int64_t)total;
        return 0;
    }
    // Splats [s0, s1): set up, and walk if the tiles fit the list; else each half on its own.  One splat always fits: the
    // views of a pass are chosen so that all of their tiles do.
    int range(int phase, int s0, int s1)
    {
        unsigned long long total = 0;
        if (int rc = setup(s0, s1, &total)) return rc;
        if (total > RENDER_LIST_CAP) {
            if (s1 - s0 <= 1) return rfail("render: internal: the tiles of one splat exceed the work list");
            const int mid = s0 + (s1 - s0) / 2;
            if (int rc = range(phase, s0, mid)) return rc;
            return range(phase, mid, s1);
        }
        return walk(phase, s0, s1, total);
    }
};
} // namespace

// ---- the renderer in two parts (the pattern of knn_check / knn_device in pais_cloud.hip): the argument check, whose
// refusals carry the caller's name, and the device part, which runs the passes of views and hands each finished pass to a hook
// while its maps are still on the device.  pais_cloud_render is those two plus the copy back; pais_cloud_visibility tests its
// queries in the hook.
static int render_check(const char *name, bool needMaps, int device, int mode, int n, const double *centers, const double *normals,
                        const double *radii, double radius, int num_views, const pais_view *views, int width, int height,
                        const double *depth, const int32_t *id)
{
    const std::string who(name);
    if (check_sizes(who, n, num_views, width, height)) return -1;
    if (mode != PAIS_RENDER_DISC && mode != PAIS_RENDER_POINT) return rfail(who + ": unknown mode " + std::to_string(mode));
    if ((num_views && (!views || (needMaps && (!depth || !id)))) || (n && !centers)) return rfail(who + ": null pointer");
    if (mode == PAIS_RENDER_DISC && n && !normals) return rfail(who + ": DISC mode needs normals (normals == NULL)");
    if (check_device(who, device)) return -1;
    if (!std::isfinite(radius)) return rfail(who + ": radius is not finite");
    if (mode == PAIS_RENDER_POINT && !(radius >= 1.0 && radius < (double)(PAIS_RENDER_MAX_POINT_SIZE + 1)))
        return rfail(who + ": POINT size " + std::to_string(radius) + " outside [1, " + std::to_string(PAIS_RENDER_MAX_POINT_SIZE) + "]");
    if (mode == PAIS_RENDER_DISC) {
        if (!radii && n && !(radius > 0.0)) return rfail(who + ": rho <= 0 (radius " + std::to_string(radius) + ")");
        if (radii) {
            if (render_check_finite(name, "radii", (size_t)n, 1, radii)) return -1;
            for (int i = 0; i < n; ++i)
                if (!(radii[i] > 0.0)) return rfail(who + ": rho <= 0 (radii[" + std::to_string(i) + "] = " + std::to_string(radii[i]) + ")");
        }
        if (render_check_finite(name, "normals", 3 * (size_t)n, 3, normals)) return -1;
    }
    if (render_check_finite(name, "centers", 3 * (size_t)n, 3, centers)) return -1;
    if (check_views(who, num_views, views)) return -1;
    const size_t tilesPerImage = (size_t)((width + RENDER_TILE - 1) / RENDER_TILE) * (size_t)((height + RENDER_TILE - 1) / RENDER_TILE);
    if (tilesPerImage > RENDER_LIST_CAP) return rfail(who + ": one view has more 32 x 32 tiles than the work list holds");
    return 0;
}

// Views of one pass under the pixel cap; PAIS_RENDER_VIEWS overrides.
static size_t views_per_pass(int num_views, size_t pix)
{
    const long forcedViews = render_env_long("PAIS_RENDER_VIEWS");
    size_t Vc = forcedViews > 0 ? (size_t)forcedViews : (RENDER_PIXEL_CAP / pix ? RENDER_PIXEL_CAP / pix : 1);
    return Vc > (size_t)num_views ? (size_t)num_views : Vc;
}

namespace {
struct EvPair {
    hipEvent_t e[2] = {nullptr, nullptr};
    ~EvPair() { for (int k = 0; k < 2; ++k) if (e[k]) (void)hipEventDestroy(e[k]); }
    hipError_t create()
    {
        for (int k = 0; k < 2; ++k)
            if (!e[k]) {
                const hipError_t rc = hipEventCreate(&e[k]);
                if (rc != hipSuccess) return rc;
            }
        return hipSuccess;
    }
};
// hook(v0, vc, views, depth, id): the maps of views [v0, v0 + vc) are final on the device (`views`: the first of them there)
using PassHook = std::function<int(size_t, int, const pais_view *, const unsigned long long *, const int32_t *)>;
} // namespace

// Checked arguments, num_views > 0 (n may be 0: every pixel empty).  *ms: milliseconds from the first kernel of each pass
// to its last, without the hook.
// mode RENDER_TRIANGLE: n triangles `tris` over nv vertices in `centers`; normals, radii and radius are not read.
static int render_device(int device, int mode, int flags, int n, const double *centers, const double *normals, const double *radii,
                         double radius, int num_views, const pais_view *views, int width, int height, double *ms, const PassHook &hook,
                         int nv = 0, const int32_t *tris = nullptr)
{
    const bool tri = mode == RENDER_TRIANGLE;
    const size_t pix = (size_t)width * (size_t)height;
    const size_t tilesPerImage = (size_t)((width + RENDER_TILE - 1) / RENDER_TILE) * (size_t)((height + RENDER_TILE - 1) / RENDER_TILE);
    // the split: views per pass bounded by the pixel cap (PAIS_RENDER_VIEWS overrides) and by the tiles the work list holds;
    // splats per launch bounded by the record buffer (PAIS_RENDER_SPLATS overrides)
    const long forcedSplats = render_env_long("PAIS_RENDER_SPLATS");
    size_t Vc = views_per_pass(num_views, pix);
    if (Vc > RENDER_LIST_CAP / tilesPerImage) Vc = RENDER_LIST_CAP / tilesPerImage;
    if (Vc > RENDER_ITEM_CAP) Vc = RENDER_ITEM_CAP;
    size_t Sc = RENDER_ITEM_CAP / Vc;
    if (forcedSplats > 0 && (size_t)forcedSplats < Sc) Sc = (size_t)forcedSplats;
    if (Sc > (size_t)n) Sc = (size_t)n;

    RHIP(hipSetDevice(device));
    DevBuf<double> dc, dn, dr; // freed on every return path
    DevBuf<pais_view> dv;
    DevBuf<RenderItem> items;
    DevBuf<TriItem> titems;
    DevBuf<unsigned int> plist;
    DevBuf<unsigned long long> list, counters, dd;
    DevBuf<int32_t> di, dt;
    EvPair tev;
    double phaseMs[3] = {0.0, 0.0, 0.0};
    int64_t packedPairs = 0;
    if (tri && n) {
        RHIP(dc.alloc(sizeof(double) * 3 * (size_t)nv));
        RHIP(hipMemcpy(dc, centers, sizeof(double) * 3 * (size_t)nv, hipMemcpyHostToDevice));
        RHIP(dt.alloc(sizeof(int32_t) * 3 * (size_t)n));
        RHIP(hipMemcpy(dt, tris, sizeof(int32_t) * 3 * (size_t)n, hipMemcpyHostToDevice));
        RHIP(titems.alloc(sizeof(TriItem) * Sc * Vc));
        RHIP(plist.alloc(sizeof(unsigned int) * Sc * Vc));
        RHIP(list.alloc(sizeof(unsigned long long) * RENDER_LIST_CAP));
        RHIP(tev.create());
    } else if (n) {
        RHIP(dc.alloc(sizeof(double) * 3 * (size_t)n));
        RHIP(hipMemcpy(dc, centers, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice));
        if (mode == PAIS_RENDER_DISC) {
            RHIP(dn.alloc(sizeof(double) * 3 * (size_t)n));
            RHIP(hipMemcpy(dn, normals, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice));
            if (radii) {
                RHIP(dr.alloc(sizeof(double) * (size_t)n));
                RHIP(hipMemcpy(dr, radii, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
            }
        }
        RHIP(items.alloc(sizeof(RenderItem) * Sc * Vc));
        RHIP(list.alloc(sizeof(unsigned long long) * RENDER_LIST_CAP));
    }
    RHIP(dv.alloc(sizeof(pais_view) * (size_t)num_views));
    RHIP(hipMemcpy(dv, views, sizeof(pais_view) * (size_t)num_views, hipMemcpyHostToDevice));
    RHIP(counters.alloc(sizeof(unsigned long long) * CNT_N));
    RHIP(dd.alloc(sizeof(unsigned long long) * Vc * pix));
    RHIP(di.alloc(sizeof(int32_t) * Vc * pix));
    RHIP(hipMemset(counters, 0, sizeof(unsigned long long) * CNT_N));
    EvPair ev;
    RHIP(ev.create());
    double msTotal = 0.0;
    int64_t tiles = 0;
    for (size_t v0 = 0; v0 < (size_t)num_views; v0 += Vc) {
        const int vc = (int)(((size_t)num_views - v0) < Vc ? ((size_t)num_views - v0) : Vc);
        const size_t cells = (size_t)vc * pix;
        RenderPass P;
        P.mode = mode; P.flags = flags; P.W = width; P.H = height; P.Vc = vc; P.radius = radius;
        P.centers = dc; P.normals = dn; P.radii = dr; P.views = dv + v0;
        P.items = items; P.list = list; P.counters = counters; P.depth = dd; P.id = di;
        P.tris = dt; P.titems = titems; P.plist = plist; P.tev[0] = tev.e[0]; P.tev[1] = tev.e[1];
        const unsigned fillBlocks = (unsigned)((cells + RENDER_BLOCK - 1) / RENDER_BLOCK);
        RHIP(hipEventRecord(ev.e[0], 0));
        hipLaunchKernelGGL(k_render_fill, dim3(fillBlocks), dim3(RENDER_BLOCK), 0, 0, dd, di, cells);
        ++g_render_launches;
        // every depth is final before the first id is taken: all splats through phase 0, then all of them through phase 1
        for (size_t s0 = 0; s0 < (size_t)n; s0 += Sc) {
            const int s1 = (int)(s0 + Sc < (size_t)n ? s0 + Sc : (size_t)n);
            if (int rc = P.range(0, (int)s0, s1)) return rc;
        }
        if (P.setups == 1 && P.listed <= RENDER_LIST_CAP) { // one launch held everything: its records and its lists still stand
            if (int rc = P.walk(1, 0, n, P.listed)) return rc;
        } else {
            for (size_t s0 = 0; s0 < (size_t)n; s0 += Sc) {
                const int s1 = (int)(s0 + Sc < (size_t)n ? s0 + Sc : (size_t)n);
                if (int rc = P.range(1, (int)s0, s1)) return rc;
            }
        }
        hipLaunchKernelGGL(k_render_finish, dim3(fillBlocks), dim3(RENDER_BLOCK), 0, 0, di, cells);
        ++g_render_launches;
        RHIP(hipGetLastError());
        RHIP(hipEventRecord(ev.e[1], 0));
        RHIP(hipEventSynchronize(ev.e[1]));
        float passMs = 0;
        RHIP(hipEventElapsedTime(&passMs, ev.e[0], ev.e[1]));
        msTotal += (double)passMs;
        tiles += P.tiles;
        packedPairs += P.packedPairs;
        for (int k = 0; k < 3; ++k) phaseMs[k] += P.phaseMs[k];
        if (int rc = hook(v0, vc, dv + v0, dd, di)) return rc;
    }
    unsigned long long cnt[CNT_N];
    RHIP(hipMemcpy(cnt, counters, sizeof(cnt), hipMemcpyDeviceToHost));
    g_render_counts[0] = tiles;
    g_render_counts[1] = (int64_t)cnt[CNT_COVERED];
    g_render_counts[2] = (int64_t)cnt[CNT_DEPTH_ATOMICS];
    g_render_counts[3] = (int64_t)cnt[CNT_ID_ATOMICS];
    g_render_counts[4] = packedPairs;
    if (tri)
        for (int k = 0; k < 3; ++k) g_mesh_ms[k] = phaseMs[k];
    if (ms) *ms = msTotal;
    return 0;
}

static int copy_maps_down(size_t v0, int vc, size_t pix, const unsigned long long *dd, const int32_t *di, double *depth, int32_t *id)
{
    const size_t cells = (size_t)vc * pix;
    RHIP(hipMemcpy(depth + v0 * pix, dd, sizeof(double) * cells, hipMemcpyDeviceToHost));
    RHIP(hipMemcpy(id + v0 * pix, di, sizeof(int32_t) * cells, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int pais_cloud_render(int device, int mode, int flags, int n, const double *centers, const double *normals, const double *radii,
                                 double radius, int num_views, const pais_view *views, int width, int height, double *depth, int32_t *id,
                                 double *kernel_ms)
{
    if (int rc = render_check("pais_cloud_render", true, device, mode, n, centers, normals, radii, radius, num_views, views, width, height, depth, id))
        return rc;
    const size_t pix = (size_t)width * (size_t)height;
    for (int k = 0; k < 5; ++k) g_render_counts[k] = 0;
    if (kernel_ms) *kernel_ms = 0.0;
    if (num_views == 0) return 0;
    if (n == 0) { // no splat: nothing to launch, every pixel is empty
        for (size_t k = 0; k < (size_t)num_views * pix; ++k) { depth[k] = INFINITY; id[k] = -1; }
        return 0;
    }
    return render_device(device, mode, flags, n, centers, normals, radii, radius, num_views, views, width, height, kernel_ms,
                         [&](size_t v0, int vc, const pais_view *, const unsigned long long *dd, const int32_t *di) {
                             return copy_maps_down(v0, vc, pix, dd, di, depth, id);
                         });
}

// ------------------------------------------------------------------------------------------------------- depth test ---
namespace {
// The queries on the device and the outputs of one pass of views; pass() tests all queries against the maps of a pass and
// copies the rows of its views down.
struct VisTester {
    int flags, nq, W, H;
    double tol;
    const double *queries;
    uint8_t *code;
    int32_t *occluder;
    double *margin;
    DevBuf<double> dq, dm;
    DevBuf<uint8_t> dcode;
    DevBuf<int32_t> docc;
    EvPair ev;
    double ms = 0.0;

    int pass(size_t v0, int vc, const pais_view *dviews, const double *dd, const int32_t *di)
    {
        if (!dq.p) { // the first pass is the largest
            RHIP(dq.alloc(sizeof(double) * 3 * (size_t)nq));
            RHIP(hipMemcpy(dq, queries, sizeof(double) * 3 * (size_t)nq, hipMemcpyHostToDevice));
            RHIP(dcode.alloc((size_t)vc * (size_t)nq));
            if (occluder) RHIP(docc.alloc(sizeof(int32_t) * (size_t)vc * (size_t)nq));
            if (margin) RHIP(dm.alloc(sizeof(double) * (size_t)vc * (size_t)nq));
            RHIP(ev.create());
        }
        const size_t Pc = VIS_POINT_CAP;
        const size_t pix = (size_t)H * (size_t)W;
        RHIP(hipEventRecord(ev.e[0], 0));
        for (int y0 = 0; y0 < vc; y0 += VIS_VIEW_CAP) {
            const int yc = vc - y0 < VIS_VIEW_CAP ? vc - y0 : VIS_VIEW_CAP;
            const size_t o = (size_t)y0 * (size_t)nq;
            for (size_t i0 = 0; i0 < (size_t)nq; i0 += Pc) {
                const size_t i1 = i0 + Pc < (size_t)nq ? i0 + Pc : (size_t)nq;
                const dim3 grid((unsigned)((i1 - i0 + RENDER_BLOCK - 1) / RENDER_BLOCK), (unsigned)yc);
                hipLaunchKernelGGL(k_depth_test, grid, dim3(RENDER_BLOCK), 0, 0, flags, nq, (int)i0, (int)i1, (const double *)dq, dviews + y0, W, H,
                                   dd + (size_t)y0 * pix, di ? di + (size_t)y0 * pix : nullptr, tol, dcode + o, occluder ? docc + o : nullptr,
                                   margin ? dm + o : nullptr);
                ++g_render_launches;
            }
        }
        RHIP(hipGetLastError());
        RHIP(hipEventRecord(ev.e[1], 0));
        RHIP(hipEventSynchronize(ev.e[1]));
        float passMs = 0;
        RHIP(hipEventElapsedTime(&passMs, ev.e[0], ev.e[1]));
        ms += (double)passMs;
        const size_t rows = (size_t)vc * (size_t)nq, at = v0 * (size_t)nq;
        RHIP(hipMemcpy(code + at, dcode, rows, hipMemcpyDeviceToHost));
        if (occluder) RHIP(hipMemcpy(occluder + at, docc, sizeof(int32_t) * rows, hipMemcpyDeviceToHost));
        if (margin) RHIP(hipMemcpy(margin + at, dm, sizeof(double) * rows, hipMemcpyDeviceToHost));
        return 0;
    }
};
} // namespace

// What both entries refuse about the queries, the tolerance, the flags and the outputs.
static int vis_check(const std::string &who, int flags, int allowed, bool haveId, int nq, const double *queries, double tol, const uint8_t *code)
{
    if (flags & ~allowed) return rfail(who + ": unknown flag bits " + std::to_string(flags & ~allowed));
    if ((flags & PAIS_VIS_SELF) && !haveId) return rfail(who + ": PAIS_VIS_SELF needs an id map");
    if (nq && (!queries || !code)) return rfail(who + ": null pointer");
    if (!(tol >= 0.0) || !std::isfinite(tol)) return rfail(who + ": tol is negative or not finite");
    return render_check_finite(who.c_str(), "points", 3 * (size_t)nq, 3, queries);
}

extern "C" int pais_depth_test(int device, int flags, int n, const double *points, int num_views, const pais_view *views, int width, int height,
                               const double *depth, const int32_t *id, double tol, uint8_t *code, int32_t *occluder, double *margin,
                               double *kernel_ms)
{
    const std::string who("pais_depth_test");
    if (check_sizes(who, n, num_views, width, height)) return -1;
    if (num_views && (!views || !depth)) return rfail(who + ": null pointer");
    if (num_views && n && !code) return rfail(who + ": null pointer (code)");
    if (check_device(who, device)) return -1;
    if (vis_check(who, flags, PAIS_VIS_SELF, id != nullptr, num_views ? n : 0, points, tol, code)) return -1;
    if (check_views(who, num_views, views)) return -1;
    const size_t pix = (size_t)width * (size_t)height;
    for (size_t k = 0; k < (size_t)num_views * pix; ++k)
        if (std::isnan(depth[k])) return rfail(who + ": depth holds a NaN (view " + std::to_string(k / pix) + ", pixel " + std::to_string(k % pix) + ")");
    if (kernel_ms) *kernel_ms = 0.0;
    if (n == 0 || num_views == 0) return 0;

    const size_t Vc = views_per_pass(num_views, pix);
    RHIP(hipSetDevice(device));
    DevBuf<pais_view> dv;
    DevBuf<double> dd;
    DevBuf<int32_t> di;
    RHIP(dv.alloc(sizeof(pais_view) * (size_t)num_views));
    RHIP(hipMemcpy(dv, views, sizeof(pais_view) * (size_t)num_views, hipMemcpyHostToDevice));
    RHIP(dd.alloc(sizeof(double) * Vc * pix));
    if (id) RHIP(di.alloc(sizeof(int32_t) * Vc * pix));
    VisTester T{flags, n, width, height, tol, points, code, occluder, margin};
    for (size_t v0 = 0; v0 < (size_t)num_views; v0 += Vc) {
        const int vc = (int)(((size_t)num_views - v0) < Vc ? ((size_t)num_views - v0) : Vc);
        RHIP(hipMemcpy(dd, depth + v0 * pix, sizeof(double) * (size_t)vc * pix, hipMemcpyHostToDevice));
        if (id) RHIP(hipMemcpy(di, id + v0 * pix, sizeof(int32_t) * (size_t)vc * pix, hipMemcpyHostToDevice));
        if (int rc = T.pass(v0, vc, dv + v0, dd, id ? (const int32_t *)di : nullptr)) return rc;
    }
    if (kernel_ms) *kernel_ms = T.ms;
    return 0;
}

extern "C" int pais_cloud_visibility(int device, int mode, int flags, int n, const double *centers, const double *normals, const double *radii,
                                     double radius, int nq, const double *queries, int num_views, const pais_view *views, int width, int height,
                                     double tol, uint8_t *code, int32_t *occluder, double *margin, double *depth, int32_t *id, double *kernel_ms)
{
    const char *name = "pais_cloud_visibility";
    const std::string who(name);
    if (nq < 0) return rfail(who + ": negative count");
    if ((depth == nullptr) != (id == nullptr)) return rfail(who + ": depth and id are both given or both NULL");
    if (int rc = render_check(name, false, device, mode, n, centers, normals, radii, radius, num_views, views, width, height, depth, id)) return rc;
    if (vis_check(who, flags, PAIS_RENDER_CULL_BACK | PAIS_VIS_SELF, true, num_views ? nq : 0, queries, tol, code)) return -1;
    if ((flags & PAIS_VIS_SELF) && nq != n) return rfail(who + ": PAIS_VIS_SELF needs nq == n (query i is splat i)");
    for (int k = 0; k < 5; ++k) g_render_counts[k] = 0;
    g_vis_ms[0] = g_vis_ms[1] = 0.0;
    if (kernel_ms) *kernel_ms = 0.0;
    if (num_views == 0 || (nq == 0 && !depth)) return 0;

    const size_t pix = (size_t)width * (size_t)height;
    VisTester T{flags & PAIS_VIS_SELF, nq, width, height, tol, queries, code, occluder, margin};
    double renderMs = 0.0;
    const int rc = render_device(device, mode, flags & PAIS_RENDER_CULL_BACK, n, centers, normals, radii, radius, num_views, views, width, height,
                                 &renderMs, [&](size_t v0, int vc, const pais_view *dviews, const unsigned long long *dd, const int32_t *di) {
                                     if (nq)
                                         if (int e = T.pass(v0, vc, dviews, (const double *)dd, di)) return e;
                                     return depth ? copy_maps_down(v0, vc, pix, dd, di, depth, id) : 0;
                                 });
    if (rc) return rc;
    g_vis_ms[0] = renderMs;
    g_vis_ms[1] = T.ms;
    if (kernel_ms) *kernel_ms = renderMs + T.ms;
    return 0;
}

// ------------------------------------------------------------------------------------------------------- triangles ---
// What both mesh entries refuse, in the order of render_check.
static int mesh_check(const char *name, bool needMaps, int device, int flags, int nv, const double *vertices, int nt, const int32_t *triangles,
                      int num_views, const pais_view *views, int width, int height, const double *depth, const int32_t *id)
{
    const std::string who(name);
    if (nv < 0) return rfail(who + ": negative count");
    if (check_sizes(who, nt, num_views, width, height)) return -1;
    if (flags & ~PAIS_RENDER_CULL_BACK) return rfail(who + ": unknown flag bits " + std::to_string(flags & ~PAIS_RENDER_CULL_BACK));
    if ((num_views && (!views || (needMaps && (!depth || !id)))) || (nv && !vertices) || (nt && !triangles)) return rfail(who + ": null pointer");
    if (check_device(who, device)) return -1;
    if (render_check_finite(name, "vertices", 3 * (size_t)nv, 3, vertices)) return -1;
    for (size_t k = 0; k < 3 * (size_t)nt; ++k)
        if (triangles[k] < 0 || triangles[k] >= nv)
            return rfail(who + ": triangles[" + std::to_string(k / 3) + "] corner " + std::to_string(k % 3) + " = " + std::to_string(triangles[k]) +
                         " outside [0, " + std::to_string(nv) + ")");
    if (check_views(who, num_views, views)) return -1;
    const size_t tilesPerImage = (size_t)((width + RENDER_TILE - 1) / RENDER_TILE) * (size_t)((height + RENDER_TILE - 1) / RENDER_TILE);
    if (tilesPerImage > RENDER_LIST_CAP) return rfail(who + ": one view has more 32 x 32 tiles than the work list holds");
    return 0;
}

extern "C" int pais_mesh_render(int device, int flags, int nv, const double *vertices, int nt, const int32_t *triangles, int num_views,
                                const pais_view *views, int width, int height, double *depth, int32_t *id, double *kernel_ms)
{
    if (int rc = mesh_check("pais_mesh_render", true, device, flags, nv, vertices, nt, triangles, num_views, views, width, height, depth, id)) return rc;
    const size_t pix = (size_t)width * (size_t)height;
    for (int k = 0; k < 5; ++k) g_render_counts[k] = 0;
    for (int k = 0; k < 3; ++k) g_mesh_ms[k] = 0.0;
    if (kernel_ms) *kernel_ms = 0.0;
    if (num_views == 0) return 0;
    if (nt == 0) { // no triangle: nothing to launch, every pixel is empty
        for (size_t k = 0; k < (size_t)num_views * pix; ++k) { depth[k] = INFINITY; id[k] = -1; }
        return 0;
    }
    return render_device(device, RENDER_TRIANGLE, flags, nt, vertices, nullptr, nullptr, 0.0, num_views, views, width, height, kernel_ms,
                         [&](size_t v0, int vc, const pais_view *, const unsigned long long *dd, const int32_t *di) {
                             return copy_maps_down(v0, vc, pix, dd, di, depth, id);
                         },
                         nv, triangles);
}

extern "C" int pais_mesh_visibility(int device, int flags, int nv, const double *vertices, int nt, const int32_t *triangles, int nq,
                                    const double *queries, int num_views, const pais_view *views, int width, int height, double tol, uint8_t *code,
                                    int32_t *occluder, double *margin, double *depth, int32_t *id, double *kernel_ms)
{
    const char *name = "pais_mesh_visibility";
    const std::string who(name);
    if (nq < 0) return rfail(who + ": negative count");
    if ((depth == nullptr) != (id == nullptr)) return rfail(who + ": depth and id are both given or both NULL");
    if (flags & PAIS_VIS_SELF) return rfail(who + ": PAIS_VIS_SELF is refused: a query is not a triangle");
    if (int rc = mesh_check(name, false, device, flags, nv, vertices, nt, triangles, num_views, views, width, height, depth, id)) return rc;
    if (vis_check(who, flags, PAIS_RENDER_CULL_BACK, true, num_views ? nq : 0, queries, tol, code)) return -1;
    for (int k = 0; k < 5; ++k) g_render_counts[k] = 0;
    for (int k = 0; k < 3; ++k) g_mesh_ms[k] = 0.0;
    g_vis_ms[0] = g_vis_ms[1] = 0.0;
    if (kernel_ms) *kernel_ms = 0.0;
    if (num_views == 0 || (nq == 0 && !depth)) return 0;

    const size_t pix = (size_t)width * (size_t)height;
    VisTester T{0, nq, width, height, tol, queries, code, occluder, margin};
    double renderMs = 0.0;
    const int rc = render_device(device, RENDER_TRIANGLE, flags, nt, vertices, nullptr, nullptr, 0.0, num_views, views, width, height, &renderMs,
                                 [&](size_t v0, int vc, const pais_view *dviews, const unsigned long long *dd, const int32_t *di) {
                                     if (nq)
                                         if (int e = T.pass(v0, vc, dviews, (const double *)dd, di)) return e;
                                     return depth ? copy_maps_down(v0, vc, pix, dd, di, depth, id) : 0;
                                 },
                                 nv, triangles);
    if (rc) return rc;
    g_vis_ms[0] = renderMs;
    g_vis_ms[1] = T.ms;
    if (kernel_ms) *kernel_ms = renderMs + T.ms;
    return 0;
}

extern "C" int pais_cloud_visibility_rule(int n, int num_views, const uint8_t *code, const int32_t *offsets, const int32_t *cams, int min_visible,
                                          int32_t *visible, uint8_t *outlier)
{
    const std::string who("pais_cloud_visibility_rule");
    if (n < 0 || num_views < 0) return rfail(who + ": negative count");
    if (n == 0) return 0;
    if (!code || !offsets || !visible || !outlier) return rfail(who + ": null pointer");
    if (offsets[0] != 0) return rfail(who + ": offsets[0] != 0");
    for (int i = 0; i < n; ++i)
        if (offsets[i + 1] < offsets[i]) return rfail(who + ": offsets decrease at point " + std::to_string(i));
    if (offsets[n] > 0 && !cams) return rfail(who + ": null pointer (cams)");
    for (int32_t j = 0; j < offsets[n]; ++j)
        if (cams[j] < 0 || cams[j] >= num_views) return rfail(who + ": camera index " + std::to_string(cams[j]) + " outside [0, num_views) at entry " + std::to_string(j));
    for (int i = 0; i < n; ++i) {
        int32_t v = offsets[i + 1] - offsets[i];
        for (int32_t j = offsets[i]; j < offsets[i + 1]; ++j)
            if (code[(size_t)cams[j] * (size_t)n + (size_t)i] == PAIS_VIS_OCCLUDED) --v;
        visible[i] = v;
        outlier[i] = v < min_visible ? 1 : 0;
    }
    return 0;
}
