// pais_mesh.hip -- the surface of a cloud (include/pais_mesh.h): the weighted tangent-plane distance field over pais_cloud_knn's
// device-resident table, the marching-tetrahedra iso-surface of a field (count, exclusive scan, emit) and the host weld of the
// triangle soup.  The arithmetic is pais_mesh.hpp's; the search, its split and the timer are pais_cloud.hip's
// (pais_cloud_internal.hpp).  DESIGN.md 5.11.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>
#include "../../include/pais_cloud.h"
#include "../../include/pais_mesh.h"
#include "pais_cloud_internal.hpp"
#include "pais_host.hpp"
#include "pais_mesh.hpp"

static thread_local std::string g_mesh_err;
static std::atomic<int64_t> g_mesh_launches{0};
static thread_local double g_mesh_ms[4] = {0, 0, 0, 0};
extern "C" const char *pais_mesh_last_error(void) { return g_mesh_err.c_str(); }
extern "C" int64_t pais_mesh_launches(void) { return g_mesh_launches.load(); }
extern "C" size_t pais_sizeof_grid(void) { return sizeof(pais_grid); }
extern "C" void pais_mesh_last_ms(double ms[4])
{
    if (ms) for (int k = 0; k < 4; ++k) ms[k] = g_mesh_ms[k];
}
static int mfail(const std::string &m) { g_mesh_err = m; return -1; }
static int mcloud(int rc) { g_mesh_err = pais_cloud_last_error(); return rc; } // an error of the shared search or timer
#define MHIP(call)                                                                                   \
    do {                                                                                             \
        hipError_t e_ = (call);                                                                      \
        if (e_ != hipSuccess) { g_mesh_err = std::string(#call) + ": " + hipGetErrorString(e_); return -2; } \
    } while (0)

constexpr int MESH_BLOCK = 256;               // lanes per block of the surface kernels: four waves, one cell per lane
constexpr int64_t MESH_PASS_VERTICES = 1 << 24; // vertices of a pass when `layers` is left to the entry: a 128 MB slab

static int grid_check(const std::string &who, const pais_grid *g)
{
    if (!std::isfinite(g->h) || !(g->h > 0.0)) return mfail(who + ": grid h = " + std::to_string(g->h) + " is not a positive finite number");
    int64_t nv = 1;
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(g->origin[a])) return mfail(who + ": grid origin[" + std::to_string(a) + "] is not finite");
        if (g->n[a] < 2) return mfail(who + ": grid n[" + std::to_string(a) + "] = " + std::to_string(g->n[a]) + " is below 2");
        nv *= g->n[a];
        if (nv > PAIS_MESH_MAX_VERTICES) return mfail(who + ": grid has more than 2^28 vertices");
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------------- field ---
// One lane per grid vertex of the pass: pais::mesh_field over its row of the table, read where the merge kernel wrote it
// (row-major, as k_cloud_planes reads it); the neighbours' centres and normals are gathered from the whole arrays.
__global__ __launch_bounds__(CLOUD_BLOCK) void k_mesh_field(const double *__restrict__ queries, int nq, const int32_t *__restrict__ index,
                                                            const double *__restrict__ dist2, int k, int nt,
                                                            const double *__restrict__ centers, const double *__restrict__ normals,
                                                            double support, double trunc, double *__restrict__ field)
{
    const int i = blockIdx.x * CLOUD_BLOCK + threadIdx.x;
    if (i >= nq) return;
    field[i] = pais::mesh_field(queries[3 * (size_t)i], queries[3 * (size_t)i + 1], queries[3 * (size_t)i + 2], k, index + (size_t)i * k,
                                dist2 + (size_t)i * k, nt, centers, normals, support, trunc);
}

extern "C" int pais_cloud_field(int device, int k, const pais_grid *grid, int nt, const double *centers, const double *normals,
                                double support, double trunc, double *field, double *kernel_ms)
{
    const std::string who = "pais_cloud_field";
    if (!grid || !centers || !normals || !field) return mfail(who + ": null pointer");
    if (grid_check(who, grid)) return -1;
    if (!(trunc > 0.0)) return mfail(who + ": trunc = " + std::to_string(trunc) + " is not positive");
    if (!std::isfinite(support) || !(support > trunc)) return mfail(who + ": support = " + std::to_string(support) + " must be finite and exceed trunc = " + std::to_string(trunc));
    const int nx = grid->n[0], ny = grid->n[1], nz = grid->n[2];
    const int nv = nx * ny * nz;
    std::vector<double> q(3 * (size_t)nv);
    {
        size_t g = 0;
        for (int z = 0; z < nz; ++z)
            for (int y = 0; y < ny; ++y)
                for (int x = 0; x < nx; ++x, ++g) {
                    q[3 * g] = pais::mesh_coord(grid->origin[0], grid->h, x);
                    q[3 * g + 1] = pais::mesh_coord(grid->origin[1], grid->h, y);
                    q[3 * g + 2] = pais::mesh_coord(grid->origin[2], grid->h, z);
                }
    }
    const int bad = knn_check(who, device, 0, 0, k, nv, q.data(), nt, centers, false);
    if (bad) return mcloud(bad); // nv > 0: never 1
    for (size_t e = 0; e < 3 * (size_t)nt; ++e)
        if (!std::isfinite(normals[e])) return mfail(who + ": normals[" + std::to_string(e / 3) + "] component " + std::to_string(e % 3) + " is not finite");

    KnnTable T;
    if (int rc = knn_device(device, false, k, nv, q.data(), nt, centers, T)) return mcloud(rc);
    DevBuf<double> dn, df;
    MHIP(dn.alloc(sizeof(double) * 3 * (size_t)nt));
    MHIP(df.alloc(sizeof(double) * (size_t)nv));
    MHIP(hipMemcpy(dn, normals, sizeof(double) * 3 * (size_t)nt, hipMemcpyHostToDevice));
    CloudTimer timer;
    double ms = 0;
    if (timer.start()) return mcloud(-2);
    for (size_t q0 = 0; q0 < (size_t)nv; q0 += T.sp.chunk) { // the passes of the search
        const int n = (int)(((size_t)nv - q0) < T.sp.chunk ? ((size_t)nv - q0) : T.sp.chunk);
        hipLaunchKernelGGL(k_mesh_field, dim3((n + CLOUD_BLOCK - 1) / CLOUD_BLOCK), dim3(CLOUD_BLOCK), 0, 0, T.dq + 3 * q0, n,
                           T.di + q0 * (size_t)k, T.dd + q0 * (size_t)k, k, nt, T.dt, dn, support, trunc, df + q0);
        g_mesh_launches += 1;
    }
    if (timer.stop(&ms)) return mcloud(-2);
    MHIP(hipMemcpy(field, df, sizeof(double) * (size_t)nv, hipMemcpyDeviceToHost));
    g_mesh_ms[0] = T.ms;
    g_mesh_ms[1] = ms;
    if (kernel_ms) *kernel_ms = T.ms + ms;
    return 0;
}

// ----------------------------------------------------------------------------------------------------- surface ---
// The slab of a pass: `layers` cell layers from cell layer z0, that is layers + 1 vertex layers of the field, of which the last
// is the first of the next pass.  Cell c of the pass is (i, j, kl), kl counted from z0.
struct MeshPass {
    pais_grid G;
    int z0, cells;
};

__device__ __forceinline__ void mesh_load_cell(const MeshPass &P, const double *__restrict__ slab, int c, int &i, int &j, int &kl, double (&f)[8])
{
    const int cx = P.G.n[0] - 1, cy = P.G.n[1] - 1;
    i = c % cx;
    j = (c / cx) % cy;
    kl = c / (cx * cy);
#pragma unroll
    for (int b = 0; b < 8; ++b)
        f[b] = slab[((size_t)(kl + ((b >> 2) & 1)) * P.G.n[1] + (j + ((b >> 1) & 1))) * P.G.n[0] + (i + (b & 1))];
}

// One lane per cell: its triangle count from the six masks of its eight corner values, then the exclusive scan of the block's
// counts in LDS (Hillis-Steele over 256 entries).  local[c]: the triangles of the block's cells before c; blockTotal[b]: the
// block's sum.  The scans define the order of the output; there is no atomic.
__global__ __launch_bounds__(MESH_BLOCK) void k_mesh_count(MeshPass P, const double *__restrict__ slab, int32_t *__restrict__ local,
                                                           int32_t *__restrict__ blockTotal)
{
    __shared__ int32_t s[MESH_BLOCK];
    const int c = blockIdx.x * MESH_BLOCK + threadIdx.x;
    int n = 0;
    if (c < P.cells) {
        int i, j, kl;
        double f[8];
        mesh_load_cell(P, slab, c, i, j, kl, f);
        n = pais::mesh_cell_count(f);
    }
    s[threadIdx.x] = n;
    __syncthreads();
    for (int off = 1; off < MESH_BLOCK; off <<= 1) {
        const int32_t x = (int)threadIdx.x >= off ? s[threadIdx.x - off] : 0;
        __syncthreads();
        s[threadIdx.x] += x;
        __syncthreads();
    }
    if (c < P.cells) local[c] = s[threadIdx.x] - n;
    if (threadIdx.x == MESH_BLOCK - 1) blockTotal[blockIdx.x] = s[MESH_BLOCK - 1];
}

// One block: the exclusive scan of the block totals, 256 at a time with a running carry, and the pass's sum.
__global__ __launch_bounds__(MESH_BLOCK) void k_mesh_scan(const int32_t *__restrict__ blockTotal, int blocks, int64_t *__restrict__ blockOffset,
                                                          int64_t *__restrict__ total)
{
    __shared__ int64_t s[MESH_BLOCK];
    int64_t carry = 0;
    for (int base = 0; base < blocks; base += MESH_BLOCK) {
        const int b = base + (int)threadIdx.x;
        const int64_t v = b < blocks ? (int64_t)blockTotal[b] : 0;
        s[threadIdx.x] = v;
        __syncthreads();
        for (int off = 1; off < MESH_BLOCK; off <<= 1) {
            const int64_t x = (int)threadIdx.x >= off ? s[threadIdx.x - off] : 0;
            __syncthreads();
            s[threadIdx.x] += x;
            __syncthreads();
        }
        if (b < blocks) blockOffset[b] = carry + (s[threadIdx.x] - v);
        carry += s[MESH_BLOCK - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}

// One lane per cell again: the masks recomputed, the cell's triangles written at its offset within the pass (block offset + local
// offset) with plain stores; triangles at or beyond cap (the room left in the caller's buffers) are not written.
__global__ __launch_bounds__(MESH_BLOCK) void k_mesh_emit(MeshPass P, const double *__restrict__ slab, const int32_t *__restrict__ local,
                                                          const int64_t *__restrict__ blockOffset, int64_t cap, int64_t *__restrict__ keys,
                                                          double *__restrict__ xyz)
{
    const int c = blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (c >= P.cells) return;
    const int64_t at = blockOffset[blockIdx.x] + local[c];
    if (at >= cap) return;
    int i, j, kl;
    double f[8];
    mesh_load_cell(P, slab, c, i, j, kl, f);
    pais::mesh_cell_emit(P.G, i, j, P.z0 + kl, f, at, cap, keys, xyz);
}

extern "C" int pais_field_surface(int device, const pais_grid *grid, const double *field, int layers, int64_t max_triangles,
                                  int64_t *num_triangles, int64_t *keys, double *xyz, double *kernel_ms)
{
    const std::string who = "pais_field_surface";
    if (!grid || !field || !num_triangles) return mfail(who + ": null pointer");
    if (grid_check(who, grid)) return -1;
    if (layers < 0) return mfail(who + ": layers = " + std::to_string(layers) + " is negative");
    if (max_triangles < 0) return mfail(who + ": max_triangles is negative");
    if (max_triangles > 0 && (!keys || !xyz)) return mfail(who + ": null keys or xyz with max_triangles > 0");
    if (device < 0) return mfail(who + ": needs a GPU (device < 0): the surface is extracted by HIP kernels, nothing is computed on the host");
    const int nx = grid->n[0], ny = grid->n[1], nz = grid->n[2];
    const size_t layer = (size_t)nx * ny, nv = layer * nz;
    for (size_t g = 0; g < nv; ++g)
        if (std::isinf(field[g])) return mfail(who + ": field[" + std::to_string(g) + "] is infinite");
    if (layers == 0) {
        const int64_t fit = MESH_PASS_VERTICES / (int64_t)layer - 1;
        layers = (int)(fit < 1 ? 1 : fit);
    }
    if (layers > nz - 1) layers = nz - 1;
    const size_t layerCells = (size_t)(nx - 1) * (ny - 1);
    const size_t passCells = layerCells * layers, passBlocks = (passCells + MESH_BLOCK - 1) / MESH_BLOCK;

    MHIP(hipSetDevice(device));
    DevBuf<double> slab, dxyz; // freed on every return path
    DevBuf<int32_t> local, blockTotal;
    DevBuf<int64_t> blockOffset, total, dkeys;
    MHIP(slab.alloc(sizeof(double) * layer * ((size_t)layers + 1)));
    MHIP(local.alloc(sizeof(int32_t) * passCells));
    MHIP(blockTotal.alloc(sizeof(int32_t) * passBlocks));
    MHIP(blockOffset.alloc(sizeof(int64_t) * passBlocks));
    MHIP(total.alloc(sizeof(int64_t)));
    int64_t count = 0;
    double msCount = 0, msEmit = 0;
    for (int z0 = 0; z0 < nz - 1; z0 += layers) {
        const int L = (nz - 1 - z0) < layers ? (nz - 1 - z0) : layers;
        MeshPass P;
        P.G = *grid;
        P.z0 = z0;
        P.cells = (int)(layerCells * L);
        const int blocks = (P.cells + MESH_BLOCK - 1) / MESH_BLOCK;
        MHIP(hipMemcpy(slab, field + layer * z0, sizeof(double) * layer * ((size_t)L + 1), hipMemcpyHostToDevice));
        int64_t passTotal = 0;
        {
            CloudTimer timer;
            double ms = 0;
            if (timer.start()) return mcloud(-2);
            hipLaunchKernelGGL(k_mesh_count, dim3(blocks), dim3(MESH_BLOCK), 0, 0, P, slab, local, blockTotal);
            hipLaunchKernelGGL(k_mesh_scan, dim3(1), dim3(MESH_BLOCK), 0, 0, blockTotal, blocks, blockOffset, total);
            g_mesh_launches += 2;
            if (timer.stop(&ms)) return mcloud(-2);
            msCount += ms;
        }
        MHIP(hipMemcpy(&passTotal, total, sizeof(int64_t), hipMemcpyDeviceToHost));
        if (max_triangles > 0) {
            const int64_t room = max_triangles - count; // of the caller's buffers, before this pass
            const int64_t write = room <= 0 ? 0 : (passTotal < room ? passTotal : room);
            MHIP(dkeys.reserve(0, sizeof(int64_t) * 3 * (size_t)write));
            MHIP(dxyz.reserve(0, sizeof(double) * 9 * (size_t)write));
            CloudTimer timer;
            double ms = 0;
            if (timer.start()) return mcloud(-2);
            hipLaunchKernelGGL(k_mesh_emit, dim3(blocks), dim3(MESH_BLOCK), 0, 0, P, slab, local, blockOffset, write, dkeys, dxyz);
            g_mesh_launches += 1;
            if (timer.stop(&ms)) return mcloud(-2);
            msEmit += ms;
            if (write > 0) {
                MHIP(hipMemcpy(keys + 3 * count, dkeys, sizeof(int64_t) * 3 * (size_t)write, hipMemcpyDeviceToHost));
                MHIP(hipMemcpy(xyz + 9 * count, dxyz, sizeof(double) * 9 * (size_t)write, hipMemcpyDeviceToHost));
            }
        }
        count += passTotal;
    }
    *num_triangles = count;
    g_mesh_ms[2] = msCount;
    g_mesh_ms[3] = msEmit;
    if (kernel_ms) *kernel_ms = msCount + msEmit;
    return 0;
}

// -------------------------------------------------------------------------------------------------------- weld ---
extern "C" int pais_mesh_weld(int64_t num_triangles, const int64_t *keys, const double *xyz, int64_t *num_vertices, int64_t max_vertices,
                              double *vertices, int32_t *triangles)
{
    const std::string who = "pais_mesh_weld";
    if (num_triangles < 0 || max_vertices < 0) return mfail(who + ": negative count");
    if (!num_vertices || (num_triangles && (!keys || !xyz))) return mfail(who + ": null pointer");
    if (max_vertices > 0 && num_triangles && (!vertices || !triangles)) return mfail(who + ": null vertices or triangles with max_vertices > 0");
    const size_t corners = 3 * (size_t)num_triangles;
    std::vector<size_t> order(corners); // the corners by (key, position in the soup): a key's first occurrence leads its run
    for (size_t c = 0; c < corners; ++c) order[c] = c;
    std::sort(order.begin(), order.end(), [keys](size_t a, size_t b) { return keys[a] < keys[b] || (keys[a] == keys[b] && a < b); });
    int64_t nv = 0;
    for (size_t c = 0; c < corners; ++c)
        if (c == 0 || keys[order[c]] != keys[order[c - 1]]) ++nv;
    *num_vertices = nv;
    if (nv > INT32_MAX) return mfail(who + ": more than INT32_MAX vertices");
    if (max_vertices == 0) return 0;
    if (max_vertices < nv) return mfail(who + ": max_vertices = " + std::to_string(max_vertices) + " below the " + std::to_string(nv) + " distinct keys");
    int32_t v = -1;
    for (size_t c = 0; c < corners; ++c) {
        const size_t at = order[c];
        if (c == 0 || keys[at] != keys[order[c - 1]]) {
            ++v;
            for (int a = 0; a < 3; ++a) vertices[3 * (size_t)v + a] = xyz[3 * at + a];
        }
        triangles[at] = v;
    }
    return 0;
}
