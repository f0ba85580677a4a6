/* pais_cloud.h -- scoring a cloud against ground truth: the exact nearest-neighbour search between two point sets; and the k
 * nearest neighbours of every point with the statistical outlier rule over them; and the plane through those neighbours
 * (pais_cloud_planes) with the normal-agreement rule over it.
 *
 * The reference publishes reconstruction quality only (Middlebury accuracy / completeness); both numbers
 * are order statistics of nearest distances cloud -> truth and truth -> cloud.  The search is all pairs in FP64 on the GPU
 * (DESIGN.md section 5.4); the order statistics are host arithmetic (pais_mvs_amd/evaluate.py).
 * Device-level entries like pais_seed_match: they take a `device`, not a pais_ctx, so a cloud file is scored without its
 * images. */
#ifndef PAIS_CLOUD_H
#define PAIS_CLOUD_H

#include <stddef.h>
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

/* The k nearest targets of every query: the per-point neighbourhood table (outlier filter, sample spacing, normals).
 *
 * d2 is pais_cloud_nearest's three statements (difference form, every product and sum rounded to double, no FMA, no square
 * root).  A target is admissible for query i unless PAIS_KNN_SKIP_SAME_INDEX is set and its index is i.  Row i of the output
 * (index[i k ..], dist2[i k ..]) holds the first k of all admissible targets ordered by (d2 ascending, target index
 * ascending) -- a stable sort of the distance row; +inf distances take part, in index order.  If fewer than k targets are
 * admissible the rest of the row is index = -1, dist2 = +inf.  With k == 1 and flags == 0 the output is pais_cloud_nearest's
 * byte for byte.
 * The result is a pure function of the inputs: PAIS_CLOUD_SLICES and PAIS_CLOUD_CHUNK change the time only (the default slice
 * count is chosen from nq as in pais_cloud_nearest, the pass size is bounded by the partial buffer; with the flag set a pass
 * skips the query's index in the whole set, not in the pass).
 * kernel_ms (may be NULL): milliseconds of the search and merge kernels, without the copies.
 * nq == 0 returns 0 and touches nothing.  Refused (< 0, pais_cloud_last_error()) before anything is launched: k < 1 or
 * k > PAIS_CLOUD_MAX_K, unknown flag bits, the flag with nq != nt, a negative count, a null pointer, nt == 0 with nq > 0,
 * device < 0 and a non-finite coordinate. */
#define PAIS_CLOUD_MAX_K 32
#define PAIS_KNN_SKIP_SAME_INDEX 1   /* query i ignores target i (a cloud against itself); requires nq == nt */
int  pais_cloud_knn(int device, int flags, int k, int nq, const double *queries, int nt, const double *targets,
                    int32_t *index /* nq*k */, double *dist2 /* nq*k */, double *kernel_ms);

/* The statistical outlier rule over a pais_cloud_knn table of n rows of k (PCL's StatisticalOutlierRemoval): host only, every
 * sum sequential from left to right in double.
 *     m_i  = (sum_j sqrt(dist2[i][j])) / k_i      over the k_i valid entries (index >= 0) of row i, in column order;
 *                                                 k_i == 0 gives NaN
 *     mu   = (sum_i m_i) / n                      sd = sqrt((sum_i (m_i - mu)^2) / (n - 1))
 *     threshold = mu + sigma sd                   outlier[i] = m_i > threshold
 * n < 2, a row without valid entries or a non-finite mu or sd flags nothing (outlier all 0); mean_dist and stats = {mu, sd,
 * threshold} hold what the statements give (NaN where they divide 0 by 0).  n == 0 touches nothing but stats.
 * Refused (< 0): n < 0, k < 1, a null pointer (stats always; the arrays when n > 0). */
int  pais_cloud_outlier_rule(int n, int k, const int32_t *index, const double *dist2, double sigma,
                             double *mean_dist /* n */, double stats[3] /* mu, sd, threshold */, uint8_t *outlier /* n */);

/* The plane of every query's k nearest targets: the third consumer of the neighbourhood table (normals, roughness, the
 * normal-agreement filter).  Not in the reference.  The definition is the FP64 statements below, written once in
 * pais_mvs_amd/csrc/pais_plane.hpp; every operation is rounded to double, there is no FMA, and only + - x / sqrt fabs and
 * comparisons are used, so the kernel, a host build and a restatement with Python floats give the same bits.
 *
 * Neighbourhood of query i, in this order: the query itself if PAIS_PLANE_WITH_QUERY is set, then the targets of the valid
 * entries (0 <= index < nt) of row i of the pais_cloud_knn table (flags & PAIS_KNN_SKIP_SAME_INDEX, k) in column order: m points.
 *   few points   m < 3: status = PAIS_PLANE_FEW, count = m, every double of the record 0.  Else status = PAIS_PLANE_OK.
 *   centroid     per axis: the sum in neighbourhood order from 0, divided by (double)m.
 *   covariance   xx xy xz yy yz zz: with d = point - centroid, the sum in neighbourhood order from 0 of the rounded products
 *                (d.x d.x, d.x d.y, ...), each divided by (double)m.
 *   eigen        cyclic two-sided Jacobi on the symmetric 3 x 3 matrix A, V = I.  A sweep visits the pairs (p,q) = (0,1), (0,2),
 *                (1,2); with g = a_pq:
 *                    g == 0: skip.
 *                    fabs(g) <= DBL_EPSILON * sqrt(fabs(a_pp) * fabs(a_qq)): a_pq = 0, skip.
 *                    else (a rotation): zeta = (a_qq - a_pp) / (2 g);  t = (zeta >= 0 ? 1 : -1) / (fabs(zeta) + sqrt(1 + zeta zeta));
 *                         c = 1 / sqrt(1 + t t);  s = c t;  h = t g;  a_pp = a_pp - h;  a_qq = a_qq + h;  a_pq = 0;
 *                         with r the third index and (x, y) = (a_rp, a_rq): a_rp = c x - s y, a_rq = s x + c y;
 *                         for every row j of V with (x, y) = (v_jp, v_jq): v_jp = c x - s y, v_jq = s x + c y.
 *                The loop ends after the first sweep without a rotation, or after PAIS_PLANE_SWEEPS sweeps that all rotated:
 *                status = PAIS_PLANE_NOCONV (the record holds what the statements below give).
 *   order        the pairs (a_jj, column j of V) are sorted by a_jj ascending with a stable insertion sort under `<` (equal
 *                values keep axis order): eigen[0..2]; normal = the column of eigen[0], not renormalised.
 *   sign         with PAIS_PLANE_ORIENT: the three components are negated when ((n.x t.x) + (n.y t.y)) + (n.z t.z) < 0 for
 *                t = toward[3 i ..].  Without: when the component of largest fabs (the lowest axis among equals) is < 0.
 *   offset       ((n.x d.x) + (n.y d.y)) + (n.z d.z), d = query - centroid: the signed distance of the query from its plane.
 *   variation    eigen[0] / ((eigen[0] + eigen[1]) + eigen[2]): surface variation, NaN when that is 0 / 0.
 * Tiny negative eigenvalues from rounding are returned as they come.
 *
 * The search is pais_cloud_knn's and the table stays on the device: index / dist2 (both or neither; may be NULL) receive
 * pais_cloud_knn's output byte for byte.  The fit gathers its neighbours from the whole target array.  The result is a pure
 * function of the inputs: PAIS_CLOUD_SLICES and PAIS_CLOUD_CHUNK change the time only.
 * kernel_ms (may be NULL): all kernels; pais_cloud_planes_last_ms: {search + merge, fit} of this thread's last call.
 * nq == 0 returns 0 and touches nothing.  Refused (< 0, pais_cloud_last_error()) before anything is launched: everything
 * pais_cloud_knn refuses (of index / dist2: only one of them null), unknown flag bits, PAIS_PLANE_ORIENT without toward or
 * toward without the flag, a non-finite toward, a null planes. */
#define PAIS_PLANE_WITH_QUERY 2
#define PAIS_PLANE_ORIENT 4
#define PAIS_PLANE_OK 0
#define PAIS_PLANE_FEW 1
#define PAIS_PLANE_NOCONV 2
#define PAIS_PLANE_SWEEPS 60
typedef struct pais_plane {
    double centroid[3], normal[3], eigen[3], offset, variation;
    int32_t count, status;
} pais_plane;
size_t pais_sizeof_plane(void);
int  pais_cloud_planes(int device, int flags, int k, int nq, const double *queries, int nt, const double *targets,
                       const double *toward /* nq x 3 with PAIS_PLANE_ORIENT, else NULL */, pais_plane *planes /* nq */,
                       int32_t *index /* nq*k or NULL */, double *dist2 /* nq*k or NULL */, double *kernel_ms);
void pais_cloud_planes_last_ms(double ms[2]);

/* The normal-agreement rule over n pais_plane records and n given unit normals (normals[3 i ..]): host only, one statement
 *     outlier[i] = status_i == PAIS_PLANE_OK && fabs(((g.x p.x) + (g.y p.y)) + (g.z p.z)) < min_cos
 * with g the fitted normal and p the given one (the sign of either does not matter); FEW / NOCONV rows are never flagged.
 * Refused (< 0): n < 0, a null pointer with n > 0. */
int  pais_cloud_normal_rule(int n, const pais_plane *planes, const double *normals, double min_cos, uint8_t *outlier);

/* AbstractPatch::setNormal(Vec2d) (abstractpatch.cpp:48-51) for n records: normals[3 i ..] = spherical2normal(normalS[2 i],
 * normalS[2 i + 1]) -- the statement (and the deterministic sin / cos) every loader of the library uses, so the normals of an
 * .mvs file are the bits pais_mvs_load_patch stores.  Host only. */
int  pais_cloud_normals(int n, const double *normalS, double *normals);

/* Kernels of this header launched by this process so far: two per pass of a search, one more per pass of pais_cloud_planes
 * (tests: a refused call launches nothing). */
int64_t pais_cloud_launches(void);

const char *pais_cloud_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* PAIS_CLOUD_H */
