// plane_host_shim.cpp -- TEST ONLY.  Compiles pais_mvs_amd/csrc/pais_plane.hpp (the lane-local arithmetic inlined into
// k_cloud_planes of pais_cloud.hip) for the host with -ffp-contract=off, with a plain loop in place of the kernel.  Not part of
// the product; nothing in the product links this.  With -DPLANE_SHIM_MAIN it is a stand-alone program that walks the odd sizes
// over a brute-force table of its own, for a sanitizer build.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <vector>
#include "../pais_mvs_amd/csrc/pais_plane.hpp"

extern "C" {
size_t shim_sizeof_plane(void) { return sizeof(pais_plane); }

// pais_cloud_planes over a given nq x k table (row-major); toward nq x 3 or NULL; sweeps (may be NULL): rotating sweeps per query.
void shim_planes(int with_query, int k, int nq, const double *queries, int nt, const double *targets, const int32_t *index,
                 const double *toward, pais_plane *planes, int *sweeps)
{
    for (int i = 0; i < nq; ++i)
        planes[i] = pais::plane_fit(with_query != 0, queries[3 * (size_t)i], queries[3 * (size_t)i + 1], queries[3 * (size_t)i + 2], k,
                                    index + (size_t)i * k, nt, targets, toward ? toward + 3 * (size_t)i : nullptr, sweeps ? sweeps + i : nullptr);
}
}

#ifdef PLANE_SHIM_MAIN
int main()
{
    const int cases[][4] = {{5, 2, 4, 0}, {300, 5, 8, 0}, {257, 513, 8, 0}, {63, 511, 32, 0}, {700, 700, 9, 1}, {1, 1, 1, 0}};
    long ok = 0;
    uint64_t z = 88172645463325252ULL;
    auto rnd = [&z]() { z ^= z << 13; z ^= z >> 7; z ^= z << 17; return (double)(z >> 11) / 9007199254740992.0 - 0.5; };
    for (const auto &c : cases) {
        const int nq = c[0], nt = c[1], k = c[2], skip = c[3];
        std::vector<double> q(3 * (size_t)nq), t(3 * (size_t)nt), toward(3 * (size_t)nq);
        for (double &v : t) v = rnd();
        for (double &v : q) v = rnd();
        for (double &v : toward) v = rnd();
        if (skip) q = t;
        std::vector<int32_t> index((size_t)nq * k, -1);
        for (int i = 0; i < nq; ++i) {
            std::vector<std::pair<double, int32_t>> row;
            for (int j = 0; j < nt; ++j) {
                if (skip && j == i) continue;
                const double dx = q[3 * i] - t[3 * j], dy = q[3 * i + 1] - t[3 * j + 1], dz = q[3 * i + 2] - t[3 * j + 2];
                row.push_back({((dx * dx) + (dy * dy)) + (dz * dz), j});
            }
            std::sort(row.begin(), row.end());
            for (size_t s = 0; s < row.size() && s < (size_t)k; ++s) index[(size_t)i * k + s] = row[s].second;
        }
        for (int flags = 0; flags < 4; ++flags) { // bit 0: with the query, bit 1: oriented
            std::vector<pais_plane> planes((size_t)nq);
            std::vector<int> sweeps((size_t)nq);
            shim_planes(flags & 1, k, nq, q.data(), nt, t.data(), index.data(), (flags & 2) ? toward.data() : nullptr, planes.data(), sweeps.data());
            for (int i = 0; i < nq; ++i) {
                if (planes[i].status == PAIS_PLANE_NOCONV || sweeps[i] >= PAIS_PLANE_SWEEPS) { printf("row %d did not converge\n", i); return 1; }
                ok += planes[i].status == PAIS_PLANE_OK;
            }
        }
    }
    printf("ok %ld\n", ok);
    return 0;
}
#endif
