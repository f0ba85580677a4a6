// pais_mesh.hpp -- the lane-local arithmetic of pais_cloud_field and pais_field_surface (include/pais_mesh.h): the statements of
// the header written once, inlined into k_mesh_field, k_mesh_count and k_mesh_emit (pais_mesh.hip) and compiled for the host by
// tests/mesh_host_shim.cpp.  Both builds use -ffp-contract=off, so every product, sum and quotient is rounded to double on its own.
#pragma once
#include <math.h>
#include <stdint.h>
#include "../../include/pais_mesh.h"
#include "pais_dev.hpp"

namespace pais {

// the vertex statement, per axis
PAIS_HD double mesh_coord(double origin, double h, int i) { return origin + ((double)i * h); }

// The field value of the vertex p.  row / d2row: its k entries of the neighbourhood table; centers, normals nt x 3.
PAIS_HD double mesh_field(double px, double py, double pz, int k, const int32_t *row, const double *d2row, int nt, const double *centers,
                          const double *normals, double support, double trunc)
{
    if (d2row[0] > (trunc * trunc)) return (double)NAN;
    const double r2 = support * support;
    double num = 0.0, den = 0.0;
    for (int s = 0; s < k; ++s) {
        const int32_t t = row[s];
        if (t < 0 || t >= nt) continue;
        const double d2 = d2row[s];
        if (!(d2 < r2)) continue;
        const double u = 1.0 - (d2 / r2);
        const double w = u * u;
        const double dx = px - centers[3 * (size_t)t], dy = py - centers[3 * (size_t)t + 1], dz = pz - centers[3 * (size_t)t + 2];
        const double sd = ((normals[3 * (size_t)t] * dx) + (normals[3 * (size_t)t + 1] * dy)) + (normals[3 * (size_t)t + 2] * dz);
        num += w * sd;
        den += w;
    }
    return num / den;
}

constexpr int MESH_TETS = 6;
// triangles of a tetrahedron by its mask (bit j: vertex j of the listed four is inside), two bits each: 0 1 1 2 1 2 2 1 1 2 2 1 2 1 1 0
constexpr uint32_t MESH_COUNT_BITS = 0x16696994u;
PAIS_HD int mesh_count(int mask) { return (int)((MESH_COUNT_BITS >> (2 * mask)) & 3u); }

// Cell corner of vertex j (0 .. 3) of tetrahedron t: (0,1,3,7) (0,1,5,7) (0,2,3,7) (0,2,6,7) (0,4,5,7) (0,4,6,7), three bits each.
PAIS_HD int mesh_tet_corner(int t, int j)
{
    constexpr uint32_t TET[MESH_TETS] = {07310, 07510, 07320, 07620, 07540, 07640};
    return (int)((TET[t] >> (3 * j)) & 7u);
}

// Orientation: bit `mask` of entry t set = the last two corners of that case's triangles are swapped, so that (B-A)x(C-A) points
// from inside to outside.  Derived once with exact arithmetic (corner values +-1, crossings at the midpoints; tests/mesh_ref.py
// derives it again): tetrahedra 0, 3 and 4 share one pattern over the masks 1 .. 14, tetrahedra 1, 2 and 5 have its complement.
PAIS_HD bool mesh_flip(int t, int mask)
{
    constexpr uint32_t FLIP[MESH_TETS] = {0x4d24, 0x32da, 0x32da, 0x4d24, 0x4d24, 0x32da};
    return (FLIP[t] >> mask) & 1u;
}

// Whether any of the eight corner values is NaN: such a cell is skipped.
PAIS_HD bool mesh_cell_empty(const double (&f)[8])
{
    bool nan = false;
#pragma unroll
    for (int b = 0; b < 8; ++b) nan = nan || (f[b] != f[b]);
    return nan;
}

PAIS_HD int mesh_tet_mask(const double (&f)[8], int t)
{
    int mask = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) mask |= (f[mesh_tet_corner(t, j)] < 0.0 ? 1 : 0) << j;
    return mask;
}

// The triangles of one cell.
PAIS_HD int mesh_cell_count(const double (&f)[8])
{
    if (mesh_cell_empty(f)) return 0;
    int n = 0;
#pragma unroll
    for (int t = 0; t < MESH_TETS; ++t) n += mesh_count(mesh_tet_mask(f, t));
    return n;
}

// The crossing on the edge between the cell corners ca and cb, ca's offset bits a subset of cb's (the lower grid index first):
// its key and its three coordinates.
PAIS_HD void mesh_crossing(const pais_grid &G, int i, int j, int k, const double (&f)[8], int ca, int cb, int64_t *key, double *P)
{
    const int ia = i + (ca & 1), ja = j + ((ca >> 1) & 1), ka = k + ((ca >> 2) & 1);
    const int ib = i + (cb & 1), jb = j + ((cb >> 1) & 1), kb = k + ((cb >> 2) & 1);
    const int64_t ga = ((int64_t)ka * G.n[1] + ja) * G.n[0] + ia;
    *key = ga * 8 + (cb - ca);
    const double fa = f[ca], fb = f[cb];
    const double t = fa / (fa - fb);
    const double ax = mesh_coord(G.origin[0], G.h, ia), ay = mesh_coord(G.origin[1], G.h, ja), az = mesh_coord(G.origin[2], G.h, ka);
    const double bx = mesh_coord(G.origin[0], G.h, ib), by = mesh_coord(G.origin[1], G.h, jb), bz = mesh_coord(G.origin[2], G.h, kb);
    P[0] = ax + (t * (bx - ax));
    P[1] = ay + (t * (by - ay));
    P[2] = az + (t * (bz - az));
}

// One triangle (tetrahedron vertices: (a0,b0) (a1,b1) (a2,b2), each pair in listed order) as triangle `at` of the output, when
// at < cap.
PAIS_HD void mesh_triangle(const pais_grid &G, int i, int j, int k, const double (&f)[8], int t, bool flip, int a0, int b0, int a1, int b1,
                           int a2, int b2, int64_t at, int64_t cap, int64_t *keys, double *xyz)
{
    if (at >= cap) return;
    if (flip) {
        int x = a1;
        a1 = a2;
        a2 = x;
        x = b1;
        b1 = b2;
        b2 = x;
    }
    mesh_crossing(G, i, j, k, f, mesh_tet_corner(t, a0), mesh_tet_corner(t, b0), keys + 3 * at, xyz + 9 * at);
    mesh_crossing(G, i, j, k, f, mesh_tet_corner(t, a1), mesh_tet_corner(t, b1), keys + 3 * at + 1, xyz + 9 * at + 3);
    mesh_crossing(G, i, j, k, f, mesh_tet_corner(t, a2), mesh_tet_corner(t, b2), keys + 3 * at + 2, xyz + 9 * at + 6);
}

// An edge between the tetrahedron vertices p and q in listed order (the lower first)
#define PAIS_MESH_EDGE(p, q) ((p) < (q) ? (p) : (q)), ((p) < (q) ? (q) : (p))

// The triangles of cell (i,j,k) as triangles at, at + 1, .. of the output; those at or beyond cap are not written.  Returns
// their number, mesh_cell_count's.
PAIS_HD int mesh_cell_emit(const pais_grid &G, int i, int j, int k, const double (&f)[8], int64_t at, int64_t cap, int64_t *keys, double *xyz)
{
    if (mesh_cell_empty(f)) return 0;
    int n = 0;
#pragma unroll 1
    for (int t = 0; t < MESH_TETS; ++t) {
        const int mask = mesh_tet_mask(f, t);
        const int count = mesh_count(mask);
        if (!count) continue;
        const bool flip = mesh_flip(t, mask);
        // the inside vertices in listed order, then the outside ones, two bits each
        int inside = 0;
#pragma unroll
        for (int j4 = 0; j4 < 4; ++j4) inside += (mask >> j4) & 1;
        uint32_t order = 0;
        int in = 0, out = inside;
#pragma unroll
        for (int j4 = 0; j4 < 4; ++j4) {
            if ((mask >> j4) & 1) order |= (uint32_t)j4 << (2 * in++);
            else order |= (uint32_t)j4 << (2 * out++);
        }
        const int v0 = (int)(order & 3u), v1 = (int)((order >> 2) & 3u), v2 = (int)((order >> 4) & 3u), v3 = (int)((order >> 6) & 3u);
        if (count == 1) {
            // one inside: a = v0, (b,c,d) = (v1,v2,v3); three inside: a = v3, (b,c,d) = (v0,v1,v2)
            const bool one = inside == 1;
            const int a = one ? v0 : v3, b = one ? v1 : v0, c = one ? v2 : v1, d = one ? v3 : v2;
            mesh_triangle(G, i, j, k, f, t, flip, PAIS_MESH_EDGE(a, b), PAIS_MESH_EDGE(a, c), PAIS_MESH_EDGE(a, d), at + n, cap, keys, xyz);
        } else {
            const int a = v0, b = v1, c = v2, d = v3; // q = (a-c, a-d, b-d, b-c)
            mesh_triangle(G, i, j, k, f, t, flip, PAIS_MESH_EDGE(a, c), PAIS_MESH_EDGE(a, d), PAIS_MESH_EDGE(b, d), at + n, cap, keys, xyz);
            mesh_triangle(G, i, j, k, f, t, flip, PAIS_MESH_EDGE(a, c), PAIS_MESH_EDGE(b, d), PAIS_MESH_EDGE(b, c), at + n + 1, cap, keys, xyz);
        }
        n += count;
    }
    return n;
}

} // namespace pais
