/* pais_mesh.h -- the surface of a cloud: a weighted tangent-plane distance field on a regular grid (pais_cloud_field), the
 * marching-tetrahedra iso-surface of any scalar field at level 0 (pais_field_surface) and the weld of its triangle soup into an
 * indexed mesh (pais_mesh_weld).  Not in the reference, which writes .psr for an external Poisson mesher.
 *
 * The result is defined by the FP64 statements below, written once in pais_mvs_amd/csrc/pais_mesh.hpp: every operation is rounded
 * to double, there is no FMA, and only + - x / and comparisons are used, so the kernels, a host build of that header and a
 * restatement with Python floats give the same bits, whatever the split into passes.
 * Device-level entries like pais_cloud.h: they take a `device`, not a pais_ctx. */
#ifndef PAIS_MESH_H
#define PAIS_MESH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* A regular grid: n vertices per axis (each >= 2), vertex (i,j,k) has index g = (k ny + j) nx + i and, per axis, the position
 *     origin.x + ((double)i * h)
 * cell (i,j,k) has index c = (k (ny-1) + j) (nx-1) + i.  nx ny nz <= PAIS_MESH_MAX_VERTICES, so that an edge key fits an int64
 * and a vertex index an int32. */
#define PAIS_MESH_MAX_VERTICES 268435456 /* 2^28 */
typedef struct pais_grid { double origin[3]; double h; int32_t n[3]; int32_t reserved; } pais_grid;
size_t pais_sizeof_grid(void);

/* The weighted tangent-plane distance of every grid vertex p from the oriented points (centers nt x 3, normals nt x 3, used as
 * given, not renormalised).  The neighbour row of p is pais_cloud_knn's (queries = the vertex positions, targets = centers,
 * flags 0, k); the search is that entry's and its table does not leave the device.
 *   truncation   with d2_0 the row's first distance: d2_0 > (trunc*trunc) gives NaN -- outside the band, no surface known.
 *   weights      else r2 = support*support; over the valid entries s of the row in column order, skipping !(d2_s < r2):
 *                    u = 1.0 - (d2_s / r2);  w = u*u;  d = p - c_s per axis;  sd = ((n.x*d.x) + (n.y*d.y)) + (n.z*d.z)
 *   value        f = (sum of w*sd) / (sum of w), both sums sequential from 0.
 * trunc < support is required, so the nearest entry always has a positive weight.
 * field: nx ny nz doubles, host.  kernel_ms (may be NULL): the search, merge and field kernels, without the copies.
 * The result is a pure function of the inputs: PAIS_CLOUD_SLICES and PAIS_CLOUD_CHUNK change the time only.
 * Refused (< 0, pais_mesh_last_error()) before anything is launched: everything pais_cloud_knn refuses, a bad grid (h not finite
 * or not positive, an n below 2, a product above the cap), a non-finite origin or normal, trunc <= 0 (or NaN), support <= trunc
 * (or not finite), null pointers, device < 0. */
int  pais_cloud_field(int device, int k, const pais_grid *grid, int nt, const double *centers,
                      const double *normals, double support, double trunc,
                      double *field /* nx*ny*nz */, double *kernel_ms);

/* The marching-tetrahedra iso-surface at level 0 of a scalar field on the grid (host, nx ny nz doubles).  NaN means "no value";
 * an infinite value is refused.
 *   cells        a cell is skipped when any of its 8 corners is NaN.  Corner b is the offset (b&1, (b>>1)&1, (b>>2)&1).  A corner
 *                is inside when f < 0; a value of 0 is outside.
 *   tetrahedra   six, sharing the diagonal 0-7 (the Kuhn split; its face diagonals match between neighbouring cells, so the
 *                surface is watertight and has no ambiguous case), in this order:
 *                    (0,1,3,7) (0,1,5,7) (0,2,3,7) (0,2,6,7) (0,4,5,7) (0,4,6,7)
 *   cases        I the inside vertices of a tetrahedron in listed order, O the outside ones; a-b the crossing on edge a b:
 *                    I = {a}, O = {b,c,d}:  (a-b, a-c, a-d)
 *                    O = {a}, I = {b,c,d}:  (a-b, a-c, a-d)
 *                    I = {a,b}, O = {c,d}:  q = (a-c, a-d, b-d, b-c) as (q0,q1,q2) and (q0,q2,q3)
 *   orientation  the last two corners of each triangle are swapped where needed so that (B-A)x(C-A) points from inside to outside:
 *                one bit per (tetrahedron, mask), the table in pais_mesh.hpp.
 *   order        cells ascending by c, tetrahedra 0 to 5, then the case's triangles.
 *   edges        an edge runs from its endpoint of lower grid index ga to the higher gb (every offset of this split is
 *                non-negative): key = ga*8 + code, code = the offset bits of gb - ga (1 .. 7);
 *                    t = fa / (fa - fb);   P.x = pa.x + (t * (pb.x - pa.x))   per axis, pa and pb by the vertex statement.
 *                A crossing is a function of its key alone: every triangle that shares an edge carries the same 24 bytes.
 * Triangles of zero area (the field exactly 0 at a grid vertex) are kept.
 * layers (>= 0): cell layers in z per pass, 0 = chosen by the entry; the output does not depend on it.
 * *num_triangles: the whole count; the first min(count, max_triangles) triangles in that order are written: keys 3 per
 * triangle, xyz 9 per triangle.  max_triangles == 0: only the counting pass runs, keys and xyz may be NULL.
 * kernel_ms (may be NULL): the kernels without the copies.
 * Refused (< 0, pais_mesh_last_error()) before anything is launched: a bad grid, a null grid / field / num_triangles, layers < 0,
 * max_triangles < 0, null keys or xyz with max_triangles > 0, an infinite field value, device < 0. */
int  pais_field_surface(int device, const pais_grid *grid, const double *field, int layers,
                        int64_t max_triangles, int64_t *num_triangles,
                        int64_t *keys /* 3*max */, double *xyz /* 9*max */, double *kernel_ms);

/* The triangle soup of pais_field_surface as an indexed mesh: host only.  The vertices are the distinct keys, ascending; each
 * takes the position of its key's first occurrence; triangles[3 t ..] are the soup's corners re-indexed to them.
 * *num_vertices: the count.  max_vertices == 0: only counts, vertices and triangles may be NULL.  Refused (< 0): a negative
 * count, a null pointer where one is read or written, 0 < max_vertices < the count (which *num_vertices then holds), more than
 * INT32_MAX vertices. */
int  pais_mesh_weld(int64_t num_triangles, const int64_t *keys, const double *xyz, int64_t *num_vertices,
                    int64_t max_vertices, double *vertices /* 3*max */, int32_t *triangles /* 3*num_triangles */);

/* Kernels of this header launched by this process so far (the search inside pais_cloud_field counts in pais_cloud_launches):
 * pais_cloud_field one per pass of the search; pais_field_surface two per pass (count with its block scan, scan of the block
 * totals) and a third (emit) when max_triangles > 0.  A refused call launches nothing. */
int64_t pais_mesh_launches(void);

/* Kernel milliseconds of this thread's last calls: {search + merge, field} of pais_cloud_field, {count + scans, emit} of
 * pais_field_surface. */
void pais_mesh_last_ms(double ms[4]);

const char *pais_mesh_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* PAIS_MESH_H */
