// mesh_host_shim.cpp -- TEST ONLY.  Compiles pais_mvs_amd/csrc/pais_mesh.hpp (the lane-local arithmetic inlined into k_mesh_field,
// k_mesh_count and k_mesh_emit of pais_mesh.hip) for the host with -ffp-contract=off, with plain loops in place of the kernels and of
// the scan.  Not part of the product; nothing in the product links this.  With -DMESH_SHIM_MAIN it is a stand-alone program that
// walks odd sizes over a brute-force table of its own, for a sanitizer build.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <vector>
#include "../pais_mvs_amd/csrc/pais_mesh.hpp"

extern "C" {
size_t shim_sizeof_grid(void) { return sizeof(pais_grid); }

// the header's tables as the kernels read them
int shim_mesh_count(int mask) { return pais::mesh_count(mask); }
int shim_mesh_tet_corner(int t, int j) { return pais::mesh_tet_corner(t, j); }
int shim_mesh_flip(int t, int mask) { return pais::mesh_flip(t, mask) ? 1 : 0; }

// pais_cloud_field over a given (nx ny nz) x k table (row-major)
void shim_field(const pais_grid *G, int k, const int32_t *index, const double *dist2, int nt, const double *centers, const double *normals,
                double support, double trunc, double *field)
{
    size_t g = 0;
    for (int z = 0; z < G->n[2]; ++z)
        for (int y = 0; y < G->n[1]; ++y)
            for (int x = 0; x < G->n[0]; ++x, ++g)
                field[g] = pais::mesh_field(pais::mesh_coord(G->origin[0], G->h, x), pais::mesh_coord(G->origin[1], G->h, y),
                                            pais::mesh_coord(G->origin[2], G->h, z), k, index + g * k, dist2 + g * k, nt, centers, normals,
                                            support, trunc);
}

// pais_field_surface: the whole count is returned, the first min(count, max_triangles) triangles are written
int64_t shim_surface(const pais_grid *G, const double *field, int64_t max_triangles, int64_t *keys, double *xyz)
{
    const int nx = G->n[0], ny = G->n[1], nz = G->n[2];
    int64_t at = 0;
    for (int k = 0; k < nz - 1; ++k)
        for (int j = 0; j < ny - 1; ++j)
            for (int i = 0; i < nx - 1; ++i) {
                double f[8];
                for (int b = 0; b < 8; ++b)
                    f[b] = field[((size_t)(k + ((b >> 2) & 1)) * ny + (j + ((b >> 1) & 1))) * nx + (i + (b & 1))];
                const int n = pais::mesh_cell_emit(*G, i, j, k, f, at, max_triangles, keys, xyz);
                if (n != pais::mesh_cell_count(f)) return -1;
                at += n;
            }
    return at;
}
}

#ifdef MESH_SHIM_MAIN
int main()
{
    const int grids[][3] = {{2, 2, 2}, {5, 4, 3}, {9, 8, 7}, {17, 13, 11}};
    const int clouds[] = {1, 7, 300};
    const int ks[] = {1, 8, 9, 32};
    long triangles = 0, values = 0;
    uint64_t z = 88172645463325252ULL;
    auto rnd = [&z]() { z ^= z << 13; z ^= z >> 7; z ^= z << 17; return (double)(z >> 11) / 9007199254740992.0 - 0.5; };
    for (const auto &n : grids)
        for (int nt : clouds)
            for (int k : ks) {
                pais_grid G;
                G.h = 2.4 / (double)(n[0] - 1);
                for (int a = 0; a < 3; ++a) { G.origin[a] = -1.2 + 0.01 * rnd(); G.n[a] = n[a]; }
                G.reserved = 0;
                const size_t nv = (size_t)n[0] * n[1] * n[2];
                std::vector<double> c(3 * (size_t)nt), nr(3 * (size_t)nt), field(nv);
                for (int t = 0; t < nt; ++t) { // points on the unit sphere with their outward normals
                    double x = rnd(), y = rnd(), w = rnd();
                    const double r = sqrt(x * x + y * y + w * w) + 1e-9;
                    c[3 * t] = nr[3 * t] = x / r; c[3 * t + 1] = nr[3 * t + 1] = y / r; c[3 * t + 2] = nr[3 * t + 2] = w / r;
                }
                std::vector<int32_t> index(nv * k, -1);
                std::vector<double> dist2(nv * k, INFINITY);
                size_t g = 0;
                for (int zz = 0; zz < n[2]; ++zz)
                    for (int y = 0; y < n[1]; ++y)
                        for (int x = 0; x < n[0]; ++x, ++g) {
                            const double px = pais::mesh_coord(G.origin[0], G.h, x), py = pais::mesh_coord(G.origin[1], G.h, y), pz = pais::mesh_coord(G.origin[2], G.h, zz);
                            std::vector<std::pair<double, int32_t>> row;
                            for (int t = 0; t < nt; ++t) {
                                const double dx = px - c[3 * t], dy = py - c[3 * t + 1], dz = pz - c[3 * t + 2];
                                row.push_back({((dx * dx) + (dy * dy)) + (dz * dz), t});
                            }
                            std::sort(row.begin(), row.end());
                            for (size_t s = 0; s < row.size() && s < (size_t)k; ++s) { index[g * k + s] = row[s].second; dist2[g * k + s] = row[s].first; }
                        }
                shim_field(&G, k, index.data(), dist2.data(), nt, c.data(), nr.data(), 3.0 * G.h, 2.0 * G.h, field.data());
                for (double v : field) values += v == v;
                const int64_t count = shim_surface(&G, field.data(), 0, nullptr, nullptr);
                if (count < 0) { printf("count and emit disagree\n"); return 1; }
                const int64_t cap = count > 3 ? count - 3 : count; // a prefix: nothing is written beyond it
                std::vector<int64_t> keys(3 * (size_t)cap);
                std::vector<double> xyz(9 * (size_t)cap);
                if (shim_surface(&G, field.data(), cap, keys.data(), xyz.data()) != count) { printf("two counts\n"); return 1; }
                for (int64_t key : keys)
                    if (key < 8 * 0 + 1 || key >= (int64_t)nv * 8) { printf("key out of range\n"); return 1; }
                triangles += (long)count;
            }
    printf("ok %ld triangles, %ld values\n", triangles, values);
    return 0;
}
#endif
