// pais_cloud_internal.hpp -- what pais_cloud.hip shares with the other consumers of its neighbourhood table (pais_mesh.hip): the
// checked k-nearest search that leaves its table on the device, the split it ran under and the event timer.  Declarations only;
// the definitions, and with them the one instantiation of the search kernels, stay in pais_cloud.hip.  Errors of these functions
// are reported through pais_cloud_last_error().
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string>
#include "pais_host.hpp"

constexpr int CLOUD_BLOCK = 256; // queries per block, one per thread

// The split of one search: `chunk` queries per pass, `slices` target slices of tilesPerSlice whole tiles each.
struct CloudSplit {
    size_t chunk;
    int tilesPerSlice, slices;
};

// hipEvents around the kernels of one call, destroyed on every return path
struct CloudTimer {
    hipEvent_t ev[2] = {nullptr, nullptr};
    ~CloudTimer();
    int start();
    int stop(double *kernel_ms);
};

// What the entries over the k-nearest table refuse alike, under the caller's name; outNull: the caller's own test of its output
// pointers.  < 0: refused (pais_cloud_last_error()), 1: nq == 0, nothing to do, 0: go on.
int knn_check(const std::string &who, int device, int flags, int known, int k, int nq, const double *queries, int nt,
              const double *targets, bool outNull);

// The k-nearest search of checked arguments, its table left on the device: dq, dt the two point sets, di / dd the nq x k table
// (row-major), sp the split it ran under, ms its search and merge kernels.  Everything is freed with the struct.
struct KnnTable {
    DevBuf<double> dq, dt, dd;
    DevBuf<int32_t> di;
    CloudSplit sp;
    double ms = 0;
};
int knn_device(int device, bool skip, int k, int nq, const double *queries, int nt, const double *targets, KnnTable &T);
