/* pais_cloud.h -- scoring a cloud against ground truth: the exact nearest-neighbour search between two point sets.
 *
 * The reference publishes reconstruction quality only (Middlebury accuracy / completeness); both numbers
 * are order statistics of nearest distances cloud -> truth and truth -> cloud.  The search is all pairs in FP64 on the GPU
 * (DESIGN.md section 5.4); the order statistics are host arithmetic (pais_mvs_amd/evaluate.py).
 * Device-level entries like pais_seed_match: they take a `device`, not a pais_ctx, so a cloud file is scored without its
 * images. */
#ifndef PAIS_CLOUD_H
#define PAIS_CLOUD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The largest number of target slices one search is split into (PAIS_CLOUD_SLICES is clamped to [1, this]). */
#define PAIS_CLOUD_MAX_SLICES 64

/* For every query q the nearest target t under
 *     dx = q.x - t.x;  dy = q.y - t.y;  dz = q.z - t.z;  d2 = ((dx*dx) + (dy*dy)) + (dz*dz)
 * with every product and sum rounded to double (no FMA): nearest[i] = the LOWEST target index that attains the minimum d2,
 * dist2[i] = that minimum (no square root is taken).  Host pointers; queries nq x 3, targets nt x 3, row-major.
 * kernel_ms (may be NULL): milliseconds of the search and reduce kernels, without the copies.
 * nq == 0 returns 0 and touches nothing.  A negative count, a null pointer, nt == 0 with nq > 0, device < 0 and a
 * non-finite coordinate are refused (< 0, pais_cloud_last_error()) before anything is launched.
 * The result does not depend on how the work is split: PAIS_CLOUD_SLICES (target slices per query block, default chosen
 * from nq) and PAIS_CLOUD_CHUNK (queries per pass, default bounded by the partial buffer) change the time only. */
int  pais_cloud_nearest(int device, int nq, const double *queries, int nt, const double *targets,
                        int32_t *nearest, double *dist2, double *kernel_ms);

/* AbstractPatch::setNormal(Vec2d) (abstractpatch.cpp:48-51) for n records: normals[3 i ..] = spherical2normal(normalS[2 i],
 * normalS[2 i + 1]) -- the statement (and the deterministic sin / cos) every loader of the library uses, so the normals of an
 * .mvs file are the bits pais_mvs_load_patch stores.  Host only. */
int  pais_cloud_normals(int n, const double *normalS, double *normals);

/* Search kernels launched by this process so far (tests: a refused call launches nothing). */
int64_t pais_cloud_launches(void);

const char *pais_cloud_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* PAIS_CLOUD_H */
