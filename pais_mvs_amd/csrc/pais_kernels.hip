// pais_kernels.hip -- gfx950 (CDNA4, wave64) kernels of the PAIS-MVS hot path.
//
//   k_begin      : head of Patch::refine()                         (patch.cpp:114-136)
//   k_pso_init   : psoOptimization set-up, initial swarm, the candidate's evaluation constants   (patch.cpp:180-200,
//                                                                                                  psosolver.cpp:94-110)
//   k_pso_eval2  : PAIS::getFitness for one (candidate, particle) per wave          (patch.cpp:914-1047)   } large
//   k_pso_step   : PsoSolver::run() between two fitness passes, one wave per candidate   (psosolver.cpp)    } batches
//   k_pso_iter   : the same step replayed inside the evaluation waves + getFitness: one launch per iteration (small
//                  batches; 1 / 2 / 4 waves per evaluation)
//   k_after      : removeInvisibleCamera + setters + seed-loop control  (patch.cpp:156-175, 655-721; mvs.cpp:215,574)
//   k_fitness    : batched PAIS::getFitness (pais_fitness_batch)
//   k_neighbor_count : all-pairs neighbour counts of MVS::neighborPatchFiltering   (mvs.cpp:448-524)
//
// Mapping: one wave per cost evaluation, window pixels <-> lanes (row-major, so neighbouring
// lanes read neighbouring pixels of the reprojected image rows), the swarm of a candidate <-> lanes in the step, FP64
// xor-butterfly reductions in a fixed order so that a cost value is a pure function of (patch, particle).  Homographies,
// camera constants and the per-camera colours of a pixel live in LDS.  No MFMA: the work is gathers + FP64 VALU
// (SURVEY 8d).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/pais_hip.h"
#include "../../include/pais_test_hooks.h"
#include "pais_dev.hpp"
#include "pais_internal.h"

using namespace pais;

// Compile-time tuning of the cost evaluation:
//   PAIS_NS1_WAVES   waves per SIMD the register allocator is asked for in the one-pixel-per-lane kernels (many cameras)
#ifndef PAIS_NS1_WAVES
#define PAIS_NS1_WAVES 2   // only batches of more than 12 cameras run them: their LDS scratch allows < 2 waves per SIMD anyway
#endif
#ifndef PAIS_NS2_WAVES
#define PAIS_NS2_WAVES 3
#endif
#define PAIS_EVAL_BOUNDS(NS) __launch_bounds__(64, (NS) == 1 ? PAIS_NS1_WAVES : PAIS_NS2_WAVES)
// k_pso_iter launches that share an evaluation among several waves run with the GPU nearly empty and are bound by the latency
// of one wave: no occupancy to protect, so the register allocator gets the whole file (no scratch reloads -- each a memory
// round trip -- on the step replay's critical path)
#ifndef PAIS_ITER_FREE_REGS_FROM
#define PAIS_ITER_FREE_REGS_FROM 2
#endif
#define PAIS_ITER_BOUNDS(P, NS) __launch_bounds__(64, (P) >= PAIS_ITER_FREE_REGS_FROM ? 1 : ((NS) == 1 ? PAIS_NS1_WAVES : PAIS_NS2_WAVES))
//   PAIS_TWO_PIXELS_MAXK  largest camera count of a batch that still runs two window pixels per lane (NS = 2)
#ifndef PAIS_TWO_PIXELS_MAXK
#define PAIS_TWO_PIXELS_MAXK 6
#endif

// --------------------------------------------------------------- helpers ---
// first task / task stride of this wave in the evaluation kernels (grid-stride over tasks, one-wave workgroups).  The
// threadIdx.x >> 6 term is always 0, but dropping it changes the generated code (the task index becomes wave-uniform):
// unmeasured, so it stays
__device__ __forceinline__ int eval_first_task() { return (int)blockIdx.x + (int)(threadIdx.x >> 6); }
__device__ __forceinline__ int eval_task_stride() { return (int)gridDim.x; }

__device__ __forceinline__ void wave_sync()
{
    // LDS/global traffic of one wave is processed in issue order; a
    // wavefront-scope fence only has to stop the compiler from reordering.
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
// value of lane `src` for a WAVE-UNIFORM src (a loop counter, this wave's particle, the winner of a wave-wide selection):
// two v_readlane_b32 through an SGPR index instead of two ds_bpermute_b32 through the LDS crossbar -- the step replay of
// k_pso_iter is chains of such broadcasts (one per particle and quantity), each a ~130-cycle round trip as a bpermute
__device__ __forceinline__ double lane_get(double v, int src)
{
    const int s = __builtin_amdgcn_readfirstlane(src);
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), s), hi = __builtin_amdgcn_readlane(__double2hiint(v), s);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double wave_sum_x(double v);
// the wave64 xor butterfly of every reduction of the path (m = 32, 16, ..., 1): wave_sum_x below computes it without the LDS crossbar
// (round 4: six __shfl_xor = twelve ds_bpermute_b32 per sum)
__device__ __forceinline__ double wave_sum(double v) { return wave_sum_x(v); }
// The same xor butterfly (m = 32, 16, 8, 4, 2, 1: at every level a lane adds its partner's value, both partners get the same sum)
// without the LDS crossbar -- round 5: the eight reductions of an evaluation were 96 ds_bpermute_b32, a quarter of its LDS
// instructions and six dependent ~130-cycle round trips each.  gfx950: v_permlane32_swap / v_permlane16_swap exchange halves /
// rows between two registers (given v twice they leave {v[l], v[l ^ m]} in some order in every lane: the sum is the same either
// way, IEEE addition commutes); xor 8 is a row rotation by 8, xor 4 a half-row mirror followed by a quad reversal, xor 2 and 1
// quad permutations: DPP operand modifiers of v_mov.  Same pairs, same sums, same bits.  ALL 64 lanes must be active.
template <int CTRL> __device__ __forceinline__ double wsum_dpp(double v)
{
    return __hiloint2double(__builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, true),
                            __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ double wave_sum_x(double v)
{
    {
        const int lo = __double2loint(v), hi = __double2hiint(v);
        const auto rl = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
        const auto rh = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
        v = __hiloint2double(rh[0], rl[0]) + __hiloint2double(rh[1], rl[1]);
    }
    {
        const int lo = __double2loint(v), hi = __double2hiint(v);
        const auto rl = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
        const auto rh = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
        v = __hiloint2double(rh[0], rl[0]) + __hiloint2double(rh[1], rl[1]);
    }
    v += wsum_dpp<0x128>(v);                  // row_ror:8          l ^ 8
    v += wsum_dpp<0x1B>(wsum_dpp<0x141>(v));  // row_half_mirror, then quad_perm [3, 2, 1, 0]: l ^ 4
    v += wsum_dpp<0x4E>(v);                   // quad_perm [2, 3, 0, 1]  l ^ 2
    v += wsum_dpp<0xB1>(v);                   // quad_perm [1, 0, 3, 2]  l ^ 1
    return v;
}
// EIGHT butterflies at once (round 6): the (fitness, weight) pairs of an evaluation's four canonical sub-accumulators.  As eight
// wave_sum_x they were ~200 VALU instructions at the end of every evaluation (80 DPP moves, 32 permlane swaps, 48 additions, the
// moves around them) -- 6 % of an evaluation at five cameras.  A level of the butterfly leaves the same sum in BOTH partners, so one
// of them is free to carry another value: v_permlane32_swap(x, y) puts {x[l], x[l + 32]} into the lower 32 lanes and {y[l - 32], y[l]}
// into the upper 32 -- ONE addition then holds the m = 32 level of x below and of y above; v_permlane16_swap does the same for the
// 16-lane rows.  Two levels turn eight values into two registers (four additions + two instead of sixteen); the levels m = 8 ... 1 run
// as before on those two; the eight totals are read from lanes 0 / 16 / 32 / 48.  The SAME pairs are added at every level of every
// value (IEEE addition commutes): the bits of wave_sum_x.  ALL 64 lanes must be active.
__device__ __forceinline__ double wsum_swapadd32(double x, double y)
{
    const auto rl = __builtin_amdgcn_permlane32_swap(__double2loint(x), __double2loint(y), false, false);
    const auto rh = __builtin_amdgcn_permlane32_swap(__double2hiint(x), __double2hiint(y), false, false);
    return __hiloint2double(rh[0], rl[0]) + __hiloint2double(rh[1], rl[1]);
}
__device__ __forceinline__ double wsum_swapadd16(double x, double y)
{
    const auto rl = __builtin_amdgcn_permlane16_swap(__double2loint(x), __double2loint(y), false, false);
    const auto rh = __builtin_amdgcn_permlane16_swap(__double2hiint(x), __double2hiint(y), false, false);
    return __hiloint2double(rh[0], rl[0]) + __hiloint2double(rh[1], rl[1]);
}
__device__ __forceinline__ double wsum_const_lane(double v, int src)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), src), __builtin_amdgcn_readlane(__double2loint(v), src));
}
// a[0 .. 7] per lane -> t[j] = wave_sum_x(a[j]), wave-uniform
__device__ __forceinline__ void wave_sum8(const double *a, double *t)
{
    // m = 32: lanes 0..31 hold the level of a[j], lanes 32..63 that of a[j + 4]
    const double z0 = wsum_swapadd32(a[0], a[4]), z1 = wsum_swapadd32(a[1], a[5]);
    const double z2 = wsum_swapadd32(a[2], a[6]), z3 = wsum_swapadd32(a[3], a[7]);
    // m = 16: rows 0 / 1 / 2 / 3 of w0 hold a[0] / a[2] / a[4] / a[6], of w1 a[1] / a[3] / a[5] / a[7]
    double w0 = wsum_swapadd16(z0, z2), w1 = wsum_swapadd16(z1, z3);
    w0 += wsum_dpp<0x128>(w0);                  w1 += wsum_dpp<0x128>(w1);                  // l ^ 8
    w0 += wsum_dpp<0x1B>(wsum_dpp<0x141>(w0));  w1 += wsum_dpp<0x1B>(wsum_dpp<0x141>(w1));  // l ^ 4
    w0 += wsum_dpp<0x4E>(w0);                   w1 += wsum_dpp<0x4E>(w1);                   // l ^ 2
    w0 += wsum_dpp<0xB1>(w0);                   w1 += wsum_dpp<0xB1>(w1);                   // l ^ 1
    t[0] = wsum_const_lane(w0, 0);  t[2] = wsum_const_lane(w0, 16); t[4] = wsum_const_lane(w0, 32); t[6] = wsum_const_lane(w0, 48);
    t[1] = wsum_const_lane(w1, 0);  t[3] = wsum_const_lane(w1, 16); t[5] = wsum_const_lane(w1, 32); t[7] = wsum_const_lane(w1, 48);
}
// the same for FOUR values (an evaluation shared by two waves: two sub-accumulators each) and for TWO (four waves)
__device__ __forceinline__ void wave_sum4(const double *a, double *t)
{
    const double z0 = wsum_swapadd32(a[0], a[2]), z1 = wsum_swapadd32(a[1], a[3]); // lanes 0..31: a[0] / a[1], lanes 32..63: a[2] / a[3]
    double w = wsum_swapadd16(z0, z1);                                              // rows 0 / 1 / 2 / 3: a[0] / a[1] / a[2] / a[3]
    w += wsum_dpp<0x128>(w);
    w += wsum_dpp<0x1B>(wsum_dpp<0x141>(w));
    w += wsum_dpp<0x4E>(w);
    w += wsum_dpp<0xB1>(w);
    t[0] = wsum_const_lane(w, 0); t[1] = wsum_const_lane(w, 16); t[2] = wsum_const_lane(w, 32); t[3] = wsum_const_lane(w, 48);
}
__device__ __forceinline__ void wave_sum2(const double *a, double *t)
{
    double w = wsum_swapadd32(a[0], a[1]); // lanes 0..31: a[0], lanes 32..63: a[1]
    w = wsum_swapadd16(w, w);
    w += wsum_dpp<0x128>(w);
    w += wsum_dpp<0x1B>(wsum_dpp<0x141>(w));
    w += wsum_dpp<0x4E>(w);
    w += wsum_dpp<0xB1>(w);
    t[0] = wsum_const_lane(w, 0); t[1] = wsum_const_lane(w, 32);
}
__device__ __forceinline__ int wave_sum_i(int v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

#include "pais_eval.hpp"

// ------------------------------------------------------------- k_fitness ---
// pais_fitness_batch: k_state_blocks builds the evaluation block of every patch state (one wave per state), then
// one wave (= one 64-thread workgroup) per evaluation
__global__ __launch_bounds__(64) void k_state_blocks(DevScene sc, const pais_patch_state *states, int nStates, unsigned char *evalBlocks,
                                                     size_t evalBlockBytes, WinPix *win)
{
    const int lane = threadIdx.x;
    const int WS = win_stride(sc);
    for (int s = blockIdx.x; s < nStates; s += gridDim.x) {
        const pais_patch_state *st = &states[s];
        unsigned char *blk = evalBlocks + evalBlockBytes * (size_t)s;
        build_eval_block(sc, (EvalPatch *)blk, (EvalCam *)(blk + sizeof(EvalPatch)), win + (size_t)s * WS, st->ray, st->ref_cam, st->lod,
                         st->num_cam, st->cam_idx, lane);
    }
}
template <int NS, bool BYTES, bool ACCR>
__global__ PAIS_EVAL_BOUNDS(NS) void k_fitness(DevScene sc, const int32_t *stateIndex, const double *particles, double *out,
                                                                  int nEvals, int Kmax, const unsigned char *evalBlocks, size_t evalBlockBytes,
                                                                  const WinPix *win)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem0[];
    unsigned char *smem = smem0 + (threadIdx.x >> 6) * eval_lds_bytes(NS, Kmax, ACCR); // wave-private scratch
    EvalPatch *ep = (EvalPatch *)smem;
    EvalCam *cams = (EvalCam *)(smem + sizeof(EvalPatch));
    double *Hbuf = (double *)(smem + eval_block_bytes(Kmax));
    double *cbuf = Hbuf + Kmax * PAIS_H_STRIDE;
    const int lane = threadIdx.x & 63;
    const int WS = win_stride(sc);
    const int nw = (int)(eval_block_bytes(Kmax) / 8);
    for (int e = eval_first_task(); e < nEvals; e += eval_task_stride()) {
        const int s = stateIndex[e];
        const uint64_t *src = (const uint64_t *)(evalBlocks + evalBlockBytes * (size_t)s);
        const uint64_t v0 = lane < nw ? src[lane] : 0, v1 = lane + 64 < nw ? src[lane + 64] : 0;
        wave_sync();
        stage_eval_block(smem, src, nw, lane, v0, v1);
        wave_sync();
        double f4[4], w4[4];
        const int bad = eval_fitness_parts<NS, BYTES, ACCR>(sc, ep, cams, Hbuf, cbuf, win + (size_t)s * WS, particles[3 * e], particles[3 * e + 1],
                                               particles[3 * e + 2], lane, 0, 1, f4, w4);
        if (lane == 0) out[e] = bad ? DBL_MAX : combine_parts(f4, w4);
    }
}

// ------------------------------------------- scalar setters on an LDS patch --
// All lanes of the (single-wave) workgroup execute these with identical data;
// stores are done by lane 0, callers __syncthreads() between phases.

__device__ bool cam_project(const DevScene &sc, int cam, const double *X, double *out, int LOD)
{
    const DevCamera &c = sc.cams[cam];
    project_raw(c.R, c.T, c.focal, c.pp, sc.lodScale[LOD], X, out);
    if (LOD > c.maxLOD) return false;
    return in_image_d(out, c.w[LOD], c.h[LOD]);
}

// Patch::setReferenceCameraIndex, patch.cpp:415-445
__device__ void set_reference_camera(const DevScene &sc, pais_patch_result *st, int lane)
{
    if (st->dropped) return;
    const int camNum = st->num_cam;
    int ref = -1, drop = 0;
    if (camNum < sc.cfg.minCamNum) {
        drop = 1;
        ref = st->ref_cam;
    } else {
        double maxCorr = -DBL_MAX;
        const double n0 = st->normal[0], n1 = st->normal[1], n2 = st->normal[2];
        for (int i = 0; i < camNum; i++) {
            const DevCamera &c = sc.cams[st->cam_idx[i]];
            double corr = n0 * (-c.optN[0]) + n1 * (-c.optN[1]) + n2 * (-c.optN[2]);
            if (corr > maxCorr) {
                maxCorr = corr;
                ref = st->cam_idx[i];
            }
        }
        if (ref < 0) {
            ref = st->cam_idx[0];
            drop = 1;
        }
    }
    __syncthreads();
    if (lane == 0) {
        st->ref_cam = ref;
        if (drop) st->dropped = 1;
    }
    __syncthreads();
}

// Patch::setDepthAndRay, patch.cpp:447-461
__device__ void set_depth_and_ray(const DevScene &sc, pais_patch_result *st, int lane)
{
    if (st->dropped) return;
    if (st->ref_cam < 0) {
        __syncthreads();
        if (lane == 0) st->dropped = 1;
        __syncthreads();
        return;
    }
    const DevCamera &rc = sc.cams[st->ref_cam];
    double ray[3];
    for (int i = 0; i < 3; ++i) ray[i] = st->center[i] - rc.C[i];
    double depth = norm3(ray);
    double inv = (1.0 / depth);
    __syncthreads();
    if (lane == 0) {
        st->depth = depth;
        for (int i = 0; i < 3; ++i) st->ray[i] = ray[i] * inv;
    }
    __syncthreads();
}

// Patch::setDepthRange, patch.cpp:463-509
__device__ void set_depth_range(const DevScene &sc, pais_patch_result *st, int lane)
{
    if (st->dropped) return;
    const int camNum = st->num_cam;
    if (camNum < sc.cfg.minCamNum) {
        __syncthreads();
        if (lane == 0) st->dropped = 1;
        __syncthreads();
        return;
    }
    const DevCamera &rc = sc.cams[st->ref_cam];
    double c1[3], c2[3];
    for (int i = 0; i < 3; ++i) {
        c1[i] = st->center[i];
        c2[i] = st->ray[i] * (st->depth + 1.0) + rc.C[i];
    }
    // per-camera image displacement in parallel, max() is order independent
    double wd = -DBL_MAX;
    for (int i = lane; i < camNum; i += 64) {
        const int ci = st->cam_idx[i];
        if (ci == st->ref_cam) continue;
        double p1[2], p2[2];
        cam_project(sc, ci, c1, p1, 0);
        cam_project(sc, ci, c2, p2, 0);
        double dx = p1[0] - p2[0], dy = p1[1] - p2[1];
        double imgDist = sqrt(dx * dx + dy * dy);
        double worldDist = 1.0 / imgDist;
        if (worldDist > wd && imgDist >= 0.01) wd = worldDist;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        double o = __shfl_xor(wd, m, 64);
        wd = o > wd ? o : wd;
    }
    __syncthreads();
    if (lane == 0) {
        if (wd == -DBL_MAX) {
            st->dropped = 1;
        } else {
            double a = st->depth - wd * sc.cfg.depthRangeScalar;
            st->depthRange[0] = a > 0.0 ? a : 0.0;
            double b = wd * sc.cfg.depthRangeScalar, cc = sc.cfg.neighborRadius * 100;
            st->depthRange[1] = st->depth + (cc < b ? cc : b);
        }
    }
    __syncthreads();
}

// Patch::setLOD, patch.cpp:511-610
__device__ void set_lod(const DevScene &sc, pais_patch_result *st, int lane)
{
    if (st->dropped) return;
    if (st->ref_cam < 0) {
        __syncthreads();
        if (lane == 0) st->dropped = 1;
        __syncthreads();
        return;
    }
    const int r = sc.cfg.patchRadius, S = sc.cfg.patchSize, S2 = S * S;
    const DevCamera &rc = sc.cams[st->ref_cam];
    double c[3] = {st->center[0], st->center[1], st->center[2]};
    int LOD = sc.cfg.minLOD - 1;
    double variance = 0;
    while (variance < sc.cfg.textureVariation) {
        LOD++;
        if (LOD >= rc.maxLOD) {
            LOD = rc.maxLOD;
            break;
        }
        double pt[2];
        if (!cam_project(sc, st->ref_cam, c, pt, LOD)) {
            LOD = (LOD - 1) > 0 ? (LOD - 1) : 0;
            break;
        }
        const int cx = cv_round(pt[0]), cy = cv_round(pt[1]);
        const int w = rc.w[LOD], h = rc.h[LOD];
        if (cx - r < 0 || cx + r >= w || cy - r < 0 || cy + r >= h) { // inImage(x, y, LOD) for the whole window
            LOD = (LOD - 1) > 0 ? (LOD - 1) : 0;
            break;
        }
        const uint8_t *img = sc.imgBlob + rc.imgOff[LOD];
        int isum = 0;
        for (int k = lane; k < S2; k += 64) {
            int yi = k / S, xi = k - yi * S;
            isum += img[(cy - r + yi) * w + (cx - r + xi)];
        }
        isum = wave_sum_i(isum);
        double mean = (double)isum / (double)S2;
        double v = 0;
        for (int k = lane; k < S2; k += 64) {
            int yi = k / S, xi = k - yi * S;
            double t = (double)img[(cy - r + yi) * w + (cx - r + xi)];
            v += (t - mean) * (t - mean);
        }
        variance = wave_sum(v) / (double)S2;
    }
    __syncthreads();
    if (lane == 0) st->lod = LOD;
    __syncthreads();
}

// Patch::setPriority (patch.cpp:612-625) + Patch::setImagePoint (:627-653, colour is host-side)
__device__ void set_priority_and_image_point(const DevScene &sc, pais_patch_result *st, int lane)
{
    if (st->dropped) return;
    const int camNum = st->num_cam;
    double camRatio = ((double)camNum) / ((double)sc.numCams);
    double pri = st->fitness * det_exp(-st->correlation / 1.0 - camRatio / 1.0) * (st->lod + 1.0);
    double c[3] = {st->center[0], st->center[1], st->center[2]};
    __syncthreads();
    if (lane == 0) st->priority = pri;
    for (int i = lane; i < camNum; i += 64) {
        double p[2];
        cam_project(sc, st->cam_idx[i], c, p, 0);
        st->imgPoint[i][0] = p[0];
        st->imgPoint[i][1] = p[1];
    }
    __syncthreads();
}

// Patch::removeInvisibleCamera, patch.cpp:655-721 (with setCorrelationTable :221-267, getHomographyPatch :332-386), in the
// pieces its two callers share: remove_invisible_camera below (k_after: the record's camera list is compacted) and
// k_ncc_batch (every intermediate is stored).  A workgroup of AFTER_WAVES waves runs them: the cameras' warped patches are
// built by the waves in parallel (one camera per wave at a time), then the camera pairs of the correlation table are
// dealt to the waves; every value is produced by one wave with the operation sequence of the single-wave statement.
// (k_ncc_batch calls the first three pieces and writes the thread-0 tail -- correlation, best camera, verdicts -- out: see there.)
//   hp     : Kmax*S2 doubles (warped patches), LDS or this workgroup's global scratch
//   table  : LDS, Kmax*Kmax doubles ; Hn: LDS, Kmax*9 doubles ; flag: LDS, 1 int (drop)
#define AFTER_WAVES 4
// getHomographies(center, normal, H) by one wave
__device__ __forceinline__ void view_homographies(const DevScene &sc, int refCam, double s, const int *camIdx, int K, const double *center,
                                                  const double *n, double *Hn, int lane)
{
    const DevCamera &rc = sc.cams[refCam];
    const double d = -dot3(center, n);
    double invH[9];
    ref_plane_inverse(d, s, rc.KR, rc.KT, n, invH);
    for (int c = lane; c < K; c += 64) {
        double H[9];
        const int ci = camIdx[c];
        patch_homography(ci == refCam, d, s, sc.cams[ci].KR, sc.cams[ci].KT, n, invH, H);
        for (int i = 0; i < 9; ++i) Hn[c * 9 + i] = H[i];
    }
}
// setCorrelationTable, first half: warped, L2-normalised patches, camera c by wave c mod AFTER_WAVES; (a0, b0) is the window's
// first pixel.  A camera whose window leaves its image sets *flag (patch.cpp:243-247: the patch is dropped).
__device__ __forceinline__ void view_warp_patches(const DevScene &sc, const int *camIdx, int K, int LOD, const double *Hn, double a0, double b0,
                                                  double *hp, int *flag, int lane, int wave)
{
    const int S = sc.cfg.patchSize, S2 = S * S;
    for (int c = wave; c < K; c += AFTER_WAVES) {
        const DevCamera &cam = sc.cams[camIdx[c]];
        const uint8_t *img = sc.imgBlob + cam.imgOff[LOD];
        const int cw = cam.w[LOD], ch = cam.h[LOD];
        const double *H = Hn + 9 * c;
        double *hpc = hp + (size_t)c * S2;
        double sq = 0;
        bool bad = false;
        // no lane-dependent exit inside the walk (an out-of-image sample is flagged and sampled at a clamped position,
        // its value is never used: the whole patch is dropped), so the loads of the steps overlap
        for (int k = lane; k < S2; k += 64) {
            const int yi = k / S, xi = k - yi * S;
            const double x = a0 + (double)xi, y = b0 + (double)yi;
            const double w = (H[6] * x + H[7] * y + H[8]);
            const double ix = (H[0] * x + H[1] * y + H[2]) / w;
            const double iy = (H[3] * x + H[4] * y + H[5]) / w;
            const bool out = !(ix >= 0 && ix < cw - 1 && iy >= 0 && iy < ch - 1) || w == 0; // :355
            bad = bad || out;
            const double v = bilinear(img, cw, out ? 0.0 : ix, out ? 0.0 : iy);
            hpc[k] = v;
            sq += v * v;
        }
        if (__any(bad)) {
            if (lane == 0) atomicOr(flag, 1);
            continue;
        }
        sq = wave_sum(sq);
        const double inv = 1.0 / sqrt(sq);
        for (int k = lane; k < S2; k += 64) hpc[k] = hpc[k] * inv; // hp /= sqrt(sum)
    }
}
// setCorrelationTable, second half: the camera pairs dealt to the waves
__device__ __forceinline__ void view_fill_table(const double *hp, int K, int S2, double *table, int lane, int wave)
{
    int p = 0;
    for (int i = 0; i < K; ++i) {
        for (int j = i + 1; j < K; ++j, ++p) {
            if (p % AFTER_WAVES != wave) continue; // uniform per wave
            const double *a = hp + (size_t)i * S2, *b = hp + (size_t)j * S2;
            double acc = 0;
            for (int k = lane; k < S2; k += 64) acc += a[k] * b[k];
            acc = wave_sum(acc);
            if (lane == 0) {
                table[i * K + j] = acc;
                table[j * K + i] = acc;
            }
        }
    }
}
// the patch's correlation: the table's mean off the diagonal (end of setCorrelationTable), by one thread
__device__ __forceinline__ double view_correlation(const double *table, int K)
{
    double correlation = 0;
    for (int i = 0; i < K; ++i)
        for (int j = 0; j < K; ++j) correlation += table[i * K + j];
    correlation /= (double)(K * K - K);
    return correlation;
}
// the camera that correlates best with the others (:666-680), by one thread
__device__ __forceinline__ int view_max_idx(const double *table, int K)
{
    double maxCorr = -DBL_MAX;
    int maxIdx = 0;
    for (int i = 0; i < K; ++i) {
        double corrSum = 0;
        for (int j = 0; j < K; ++j) corrSum += table[i * K + j];
        if (corrSum >= maxCorr) { // last max wins
            maxIdx = i;
            maxCorr = corrSum;
        }
    }
    return maxIdx;
}
// the verdict on camera i (camera index ci) of the list: PAIS_VIEW_KEEP or the first reason of :688-707 that removes it
__device__ __forceinline__ int view_verdict(const DevScene &sc, double ratio, const double *n, int ci, const double *table, int K, int maxIdx, int i)
{
    // (the camera's optical normal is read whatever the ratio says: the loads of a list's cameras then overlap, where a load behind
    //  the ratio test makes the one thread that runs this wait for each camera in turn)
    const DevCamera &cam = sc.cams[ci];
    const double dd = n[0] * (-cam.optN[0]) + n[1] * (-cam.optN[1]) + n[2] * (-cam.optN[2]);
    int why = PAIS_VIEW_KEEP;
    if (ratio < sc.cfg.minRegionRatio) why = PAIS_VIEW_REGION;
    else if (dd < 0) why = PAIS_VIEW_BACKFACING;
    else if (i != maxIdx && table[maxIdx * K + i] < sc.cfg.minCorrelation) why = PAIS_VIEW_CORRELATION;
    return why;
}

// The after-stage's call: the region ratios of getHomographyRegionRatio :269-288 come from k_region_ratio
//   ratios : global, this candidate's region ratio per visible camera
// The reduction runs redundantly in every thread with single-writer stores (thread 0).
__device__ void remove_invisible_camera(const DevScene &sc, pais_patch_result *st, double *hp, double *table,
                                        double *Hn, int *flag, double *ratios, int lane, int wave)
{
    if (st->dropped) return;
    const bool lead = (lane == 0) && (wave == 0);
    const int K = st->num_cam;
    const int r = sc.cfg.patchRadius, S = sc.cfg.patchSize, S2 = S * S;
    const int LOD = st->lod, refCam = st->ref_cam;
    const double s = sc.lodScale[LOD];
    double center[3] = {st->center[0], st->center[1], st->center[2]};
    double n[3] = {st->normal[0], st->normal[1], st->normal[2]};

    if (wave == 0) view_homographies(sc, refCam, s, st->cam_idx, K, center, n, Hn, lane);
    for (int i = threadIdx.x; i < K * K; i += 64 * AFTER_WAVES) table[i] = 0;
    if (threadIdx.x == 0) *flag = 0;
    __syncthreads();

    double pt[2];
    cam_project(sc, refCam, center, pt, LOD);
    view_warp_patches(sc, st->cam_idx, K, LOD, Hn, pt[0] - r, pt[1] - r, hp, flag, lane, wave);
    __syncthreads(); // the warped patches of all waves are visible (same CU: global stores through the same L1 / L2)
    if (lead) st->ncc_tables += 1;
    if (*flag != 0) {
        // drop, correlation = 0 (and every later step is a no-op)
        __syncthreads();
        if (lead) {
            st->dropped = 1;
            st->correlation = 0;
        }
        __syncthreads();
        return;
    }
    view_fill_table(hp, K, S2, table, lane, wave);
    __syncthreads();

    const double correlation = view_correlation(table, K);
    const int maxIdx = view_max_idx(table, K);

    // mark + erase, keeping order (removeIdx holds distinct camera indices): compacted in place by one thread
    __syncthreads();
    if (lead) {
        int nn = 0;
        for (int i = 0; i < K; ++i) {
            const int ci = st->cam_idx[i];
            if (view_verdict(sc, ratios[i], n, ci, table, K, maxIdx, i) == PAIS_VIEW_KEEP) {
                ratios[nn] = ratios[i]; // stays valid for the trailing removeInvisibleCamera if the homographies do
                st->cam_idx[nn++] = ci;
            }
        }
        st->correlation = correlation;
        st->num_cam = nn;
        if (nn < sc.cfg.minCamNum) st->dropped = 1;
    }
    __syncthreads();
}

// LDS <-> global copy of a patch record by one wave
__device__ void copy_record(pais_patch_result *dst, const pais_patch_result *src, int tid, int nthreads = 64)
{
    const uint32_t *s = (const uint32_t *)src;
    uint32_t *d = (uint32_t *)dst;
    for (int i = tid; i < (int)(sizeof(pais_patch_result) / 4); i += nthreads) d[i] = s[i];
}

// ---------------------------------------------------------------- k_begin ---
// candidate -> record; head of Patch::refine() (patch.cpp:117-136)
struct WinPix;
__device__ void pso_init_candidate(const DevScene &sc, const pais_patch_result *P, int c, unsigned char *states, int Nmax,
                                   int *activeList, int *activeCount, unsigned char *evalBlocks, size_t evalBlockBytes, WinPix *win,
                                   int lane);
// INIT: the wave goes straight on to the set-up of the candidate's first PSO run (k_pso_init's work) from the record it
// still holds in LDS -- one launch and one dependent round trip fewer at the head of every batch.  (The pass counters it
// adds to were cleared by the k_after<2> of the pass before: two sets used alternately, no memset launch per pass.)
template <bool INIT>
__global__ __launch_bounds__(64) void k_begin(DevScene sc, const pais_candidate *cands, pais_patch_result *recs, int n,
                                              unsigned char *states, int Nmax, int *activeList, int *activeCount,
                                              unsigned char *evalBlocks, size_t evalBlockBytes, WinPix *win)
{
    __shared__ pais_patch_result st;
    const int lane = threadIdx.x;
    for (int c = blockIdx.x; c < n; c += gridDim.x) {
        const pais_candidate *cd = &cands[c];
        __syncthreads();
        {
            uint32_t *d = (uint32_t *)&st;
            for (int i = lane; i < (int)(sizeof(pais_patch_result) / 4); i += 64) d[i] = 0;
        }
        __syncthreads();
        if (lane == 0) {
            for (int i = 0; i < 3; ++i) {
                st.center[i] = cd->center[i];
                st.normal[i] = cd->normal[i];
            }
            st.normalS[0] = cd->normalS[0];
            st.normalS[1] = cd->normalS[1];
            st.key = cd->key;
            st.type = cd->type;
            int nc = cd->num_cam;
            st.num_cam = nc > PAIS_MAX_VIS ? PAIS_MAX_VIS : (nc < 0 ? 0 : nc);
            st.ref_cam = -1;
            st.lod = -1;
            st.fitness = DBL_MAX;   // abstractpatch.cpp:37-38
            st.priority = DBL_MAX;
            st.correlation = 0;
            st.stage = PAIS_STAGE_DONE;
        }
        __syncthreads();
        for (int i = lane; i < st.num_cam; i += 64) st.cam_idx[i] = cd->cam_idx[i];
        __syncthreads();

        if (st.num_cam < sc.cfg.minCamNum) { // patch.cpp:118-123
            if (lane == 0) {
                st.fitness = DBL_MAX;
                st.priority = DBL_MAX;
                st.dropped = 1;
            }
        } else {
            set_reference_camera(sc, &st, lane);
            set_depth_and_ray(sc, &st, lane);
            set_depth_range(sc, &st, lane);
            set_lod(sc, &st, lane);
            if (!st.dropped) {
                // patch.cpp:132-150: first evaluation of the while condition is always true
                __syncthreads();
                if (lane == 0) {
                    st.before_ref = st.ref_cam;
                    st.after_ref = -1;
                    st.before_num = st.num_cam;
                    st.after_num = -1;
                    st.total_cam_num = st.num_cam;
                    st.count = 1; // count++ evaluated once
                    st.stage = PAIS_STAGE_PSO;
                }
            }
        }
        __syncthreads();
        copy_record(&recs[c], &st, lane);
        if (INIT) pso_init_candidate(sc, &st, c, states, Nmax, activeList, activeCount, evalBlocks, evalBlockBytes, win, lane);
    }
}

// ----------------------------------------------------------- k_load_state ---
// file record -> record: the loader constructor Patch(center, normalS, camIdx, fitness, correlation), patch.cpp:45-59.  One wave
// per patch, the record in LDS as in k_begin; the setters are the ones k_begin / k_after run.  Every setter starts with
// `if (drop) return`, so the chain below is the constructor's whatever a setter decides; a field a skipped setter never
// wrote keeps its AbstractPatch default (abstractpatch.cpp:24-41), as k_begin initialises it.
__global__ __launch_bounds__(64) void k_load_state(DevScene sc, const pais_loaded_patch *in, pais_patch_result *recs, int n, uint64_t key0)
{
    __shared__ pais_patch_result st;
    const int lane = threadIdx.x;
    for (int c = blockIdx.x; c < n; c += gridDim.x) {
        const pais_loaded_patch *lp = &in[c];
        __syncthreads();
        {
            uint32_t *d = (uint32_t *)&st;
            for (int i = lane; i < (int)(sizeof(pais_patch_result) / 4); i += 64) d[i] = 0;
        }
        __syncthreads();
        if (lane == 0) {
            for (int i = 0; i < 3; ++i) st.center[i] = lp->center[i];
            st.normalS[0] = lp->normalS[0];
            st.normalS[1] = lp->normalS[1];
            spherical2normal(lp->normalS[0], lp->normalS[1], st.normal); // setNormal(Vec2d), abstractpatch.cpp:48-51
            st.key = key0 + (uint64_t)c;
            st.type = PAIS_TYPE_SEED;
            const int nc = lp->num_cam;
            st.num_cam = nc > PAIS_MAX_VIS ? PAIS_MAX_VIS : (nc < 0 ? 0 : nc);
            st.ref_cam = -1;
            st.lod = -1;
            st.fitness = lp->fitness;
            st.priority = DBL_MAX;
            st.correlation = lp->correlation;
            st.stage = PAIS_STAGE_DONE;
        }
        __syncthreads();
        for (int i = lane; i < st.num_cam; i += 64) st.cam_idx[i] = lp->cam_idx[i];
        __syncthreads();
        set_reference_camera(sc, &st, lane);
        set_depth_and_ray(sc, &st, lane);
        set_depth_range(sc, &st, lane);
        set_lod(sc, &st, lane);
        set_priority_and_image_point(sc, &st, lane); // setPriority, setImagePoint
        __syncthreads();
        copy_record(&recs[c], &st, lane);
    }
}

// ------------------------------------- split PSO pipeline (large batches) ---
// The same GLN-PSO as k_pso, as a launch-per-iteration pipeline:
//   k_pso_init : per candidate, Patch::psoOptimization set-up + initParticles/setParticle
//   k_pso_eval : ONE WAVE PER (candidate, particle) -- PAIS::getFitness; no barriers, waves that
//                leave early (DBL_MAX particles) are simply replaced by the next pair
//   k_pso_step : per candidate, initFitness/updateFitness bookkeeping, updateGbest, inertia,
//                convergence test, moveParticles -- or the write-back when the run has ended
// Dependent launches cost ~2 us each against ~100 us of evaluation work per iteration, and the
// evaluation kernel runs at the throughput of the barrier-free k_fitness.
struct PsoState { // one per candidate, in global memory; the per-particle arrays follow (stride Nmax)
    double rangeL[3], rangeU[3], rangeInter[3], init[3];
    double iw, gBestFitness;
    uint64_t streamBase;
    int gIdx, N, maxIt, iteration, active, run, localK, started;
    // what the evaluation reads from the patch (patch.cpp:922-944)
    double ray[3];
    int refCam, LOD, K, pad;
    int camIdx[PAIS_MAX_VIS];
    // k_pso_iter: the loop-carried scalars of PsoSolver::run(), double buffered by launch parity
    struct IterDyn {
        double iw, gBestFitness;
        int gIdx, iteration, started, pad;
    } dyn[2];
};
#define PSO_DOUBLES_PER_PARTICLE (3 * 4 + 2 + 8)
__host__ __device__ inline size_t pso_state_bytes(int Nmax)
{
    // header + two swarm buffers (k_pso_iter reads one and writes the other; the other pipelines use buffer 0);
    // per particle 14 doubles of swarm state + 8 partial sums (evaluations shared by several waves)
    return ((sizeof(PsoState) + 15) & ~(size_t)15) + 2 * sizeof(double) * (size_t)Nmax * PSO_DOUBLES_PER_PARTICLE;
}
struct PsoArrays {
    double (*pos)[3], (*vec)[3], (*pBest)[3], (*nBest)[3];
    double *fit, *pBestFit;
    double (*part)[8]; // (f, w) of the 4 canonical sub-accumulators when an evaluation is shared by several waves
};
__device__ __forceinline__ PsoArrays pso_arrays(unsigned char *base, int Nmax, int buf = 0)
{
    PsoArrays a;
    unsigned char *q = base + ((sizeof(PsoState) + 15) & ~(size_t)15) + (size_t)buf * sizeof(double) * (size_t)Nmax * PSO_DOUBLES_PER_PARTICLE;
    a.pos = (double(*)[3])q; q += sizeof(double) * 3 * Nmax;
    a.vec = (double(*)[3])q; q += sizeof(double) * 3 * Nmax;
    a.pBest = (double(*)[3])q; q += sizeof(double) * 3 * Nmax;
    a.nBest = (double(*)[3])q; q += sizeof(double) * 3 * Nmax;
    a.fit = (double *)q; q += sizeof(double) * Nmax;
    a.pBestFit = (double *)q; q += sizeof(double) * Nmax;
    a.part = (double(*)[8])q;
    return a;
}

// activeList / activeCount (optional): compacted indices of the candidates that run a PSO in this pass, so that
// the per-iteration launches create waves only for them (k_pso_iter)
// evalBlocks / win: per candidate the evaluation block of the run (pais_eval.hpp): EvalPatch + EvalCam[M] exactly as the
// evaluation keeps them in LDS, and the reference window WinPix[S*S]; built ONCE per PSO run here, copied / read coalesced
// by every evaluation wave of the run
// set-up of ONE candidate's PSO run by one wave (P: its record -- in global memory, or the LDS copy k_begin just built)
__device__ void pso_init_candidate(const DevScene &sc, const pais_patch_result *P, int c, unsigned char *states, int Nmax,
                                   int *activeList, int *activeCount, unsigned char *evalBlocks, size_t evalBlockBytes, WinPix *win,
                                   int lane)
{
    const size_t SB = pso_state_bytes(Nmax);
    const int WS = win_stride(sc);
    PsoState *hd = (PsoState *)(states + SB * (size_t)c);
    PsoArrays A = pso_arrays((unsigned char *)hd, Nmax);
    if (P->stage != PAIS_STAGE_PSO || P->dropped) {
        if (lane == 0) { hd->active = 0; hd->started = 0; }
        return;
    }
    const int type = P->type;
    const int N = (type == PAIS_TYPE_SEED) ? sc.cfg.particleNum * 2 : sc.cfg.particleNum;
    const int maxIt = (type == PAIS_TYPE_SEED) ? sc.cfg.maxIteration * 2 : sc.cfg.maxIteration;
    // Patch::psoOptimization set-up (patch.cpp:183-200), identical in all lanes
    const double ns0 = P->normalS[0], ns1 = P->normalS[1];
    double L[3] = {0.0, ns1 - M_PI / 2.0, P->depthRange[0]};
    double U[3] = {M_PI, ns1 + M_PI / 2.0, P->depthRange[1]};
    if (type != PAIS_TYPE_SEED) {
        double lo = ns0 - M_PI / sc.cfg.reduceNormalRange, hi = ns0 + M_PI / sc.cfg.reduceNormalRange;
        L[0] = 0.0 < lo ? lo : 0.0;
        U[0] = hi < M_PI ? hi : M_PI;
        L[1] = ns1 - M_PI / sc.cfg.reduceNormalRange;
        U[1] = ns1 + M_PI / sc.cfg.reduceNormalRange;
    }
    const double init[3] = {ns0, ns1, P->depth};
    const uint64_t sb = stream_base(sc.seed, P->key);
    const uint32_t run = (uint32_t)P->pso_runs;
    if (lane == 0) {
        for (int d = 0; d < 3; ++d) {
            hd->rangeL[d] = L[d];
            hd->rangeU[d] = U[d];
            hd->rangeInter[d] = U[d] - L[d]; // psosolver.cpp:38
            hd->init[d] = init[d];
            hd->ray[d] = P->ray[d];
        }
        hd->N = N;
        hd->maxIt = maxIt;
        hd->localK = N < 5 ? N : 5; // psosolver.cpp:26
        hd->run = (int)run;
        hd->streamBase = sb;
        hd->iw = 0.8;
        hd->iteration = 0;
        hd->gIdx = 0;
        hd->gBestFitness = DBL_MAX;
        hd->active = 1;
        hd->started = 0;
        hd->dyn[0].iw = 0.8;
        hd->dyn[0].gBestFitness = DBL_MAX;
        hd->dyn[0].gIdx = 0;
        hd->dyn[0].iteration = 0;
        hd->dyn[0].started = 0;
        hd->refCam = P->ref_cam;
        hd->LOD = P->lod;
        hd->K = P->num_cam;
        if (activeList) activeList[atomicAdd(activeCount, 1)] = c;
    }
    for (int k = lane; k < P->num_cam; k += 64) hd->camIdx[k] = P->cam_idx[k];
    {
        unsigned char *blk = evalBlocks + evalBlockBytes * (size_t)c;
        build_eval_block(sc, (EvalPatch *)blk, (EvalCam *)(blk + sizeof(EvalPatch)), win + (size_t)c * WS, P->ray, P->ref_cam, P->lod,
                         P->num_cam, P->cam_idx, lane);
    }
    // initParticles (psosolver.cpp:94-110) + setParticle(init) (:267-284)
    for (int i = lane; i < N; i += 64) {
        for (int d = 0; d < 3; ++d) {
            const double ri = U[d] - L[d];
            const double u1 = uniform_from(sb, run, (uint32_t)(2 * (d * N + i)));
            const double u2 = uniform_from(sb, run, (uint32_t)(2 * (d * N + i) + 1));
            double p = (ri * u1) + L[d];
            double v = (2.0 * ri * u2) - ri;
            if (i == 0) {
                p = init[d];
                v = (2.0 * ri * uniform_from(sb, run, (uint32_t)(6 * N + d))) - ri;
            }
            A.pos[i][d] = p;
            A.vec[i][d] = v;
            A.pBest[i][d] = p;
            A.nBest[i][d] = 0; // particle.cpp:16
        }
    }
}
__global__ __launch_bounds__(64) void k_pso_init(DevScene sc, const pais_patch_result *recs, int n, unsigned char *states,
                                                 int Nmax, int *activeList, int *activeCount, unsigned char *evalBlocks,
                                                 size_t evalBlockBytes, WinPix *win)
{
    const int lane = threadIdx.x;
    for (int c = blockIdx.x; c < n; c += gridDim.x)
        pso_init_candidate(sc, &recs[c], c, states, Nmax, activeList, activeCount, evalBlocks, evalBlockBytes, win, lane);
}

// Device-coherent access to the swarm state (k_pso_ring: the state of a candidate is handed from wave to wave INSIDE a launch,
// across XCDs with their own L2): agent-scope relaxed atomics compile to plain loads / stores with the sc1 bit -- served
// at the device's coherence point, no fence, no cache invalidation under the image taps.
// (A one-XCD-scope variant of this state measured no gain: DESIGN Appendix A, profiles/r06_ring_xcd_scope.txt.)
__device__ __forceinline__ double cload(const double *p)
{
    return __longlong_as_double((long long)__hip_atomic_load((const unsigned long long *)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ void cstore(double *p, double v)
{
    __hip_atomic_store((unsigned long long *)p, (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int cload(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void cstore(int *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ unsigned rload(const unsigned *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void rstore(unsigned *p, unsigned v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <bool COH, class T> __device__ __forceinline__ T sload(const T *p) { return COH ? cload(p) : *p; }
template <bool COH, class T> __device__ __forceinline__ void sstore(T *p, T v)
{
    if (COH) cstore(p, v);
    else *p = v;
}

#include "pais_pre.hpp"

// LDS of one swarm step: the swarm (Nmax * 14 doubles) + the scratch of swarm_eval_setup behind it
__host__ __device__ inline size_t step_lds_bytes(int Nmax) { return sizeof(double) * (size_t)Nmax * (3 * 4 + 2) + pre_scratch_bytes(Nmax); }

// The evaluation launch of large batches (split pipeline): one wave per (candidate, particle), nothing but the cost.
// The candidate's constants come from the block k_pso_init prepared; positions from swarm buffer 0 (k_pso_step).
template <int NS, bool BYTES, bool ACCR, bool PRE>
__global__ PAIS_EVAL_BOUNDS(NS) void k_pso_eval2(DevScene sc, unsigned char *states, int n, int Nmax, int Kmax,
                                                                    const unsigned char *evalBlocks, size_t evalBlockBytes, const WinPix *win,
                                                                    int pendingOnly, unsigned long long *verify, const double *pre)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem0[];
    unsigned char *smem = smem0 + (threadIdx.x >> 6) * eval_lds_bytes(NS, Kmax, ACCR); // wave-private scratch
    const size_t preD = pre_rec_doubles(Kmax);
    EvalPatch *ep = (EvalPatch *)smem;
    EvalCam *cams = (EvalCam *)(smem + sizeof(EvalPatch));
    double *Hbuf = (double *)(smem + eval_block_bytes(Kmax));
    double *cbuf = Hbuf + Kmax * PAIS_H_STRIDE;
    const int lane = threadIdx.x & 63;
    const size_t SB = pso_state_bytes(Nmax);
    const int total = n * Nmax;
    const int WS = win_stride(sc);
    const int nwMax = (int)(eval_block_bytes(Kmax) / 8);
    for (int t = eval_first_task(); t < total; t += eval_task_stride()) {
        const int c = t / Nmax, i = t - c * Nmax; // candidate-major: a CU's waves gather from the same few image windows
        PsoState *hd = (PsoState *)(states + SB * (size_t)c);
        PsoArrays A = pso_arrays((unsigned char *)hd, Nmax);
        // everything this wave needs from global memory is requested at once -- the run's state flags, the particle and
        // the first 128 words of the constants -- so that there is ONE memory round trip before the cost starts
        const uint64_t *src = (const uint64_t *)(evalBlocks + evalBlockBytes * (size_t)c);
        const int iLoad = i < Nmax ? i : 0;
        const int active = hd->active, Nrun = hd->N;
        const double p0 = A.pos[iLoad][0], p1 = A.pos[iLoad][1], p2 = A.pos[iLoad][2];
        const uint64_t v0 = lane < nwMax ? src[lane] : 0, v1 = lane + 64 < nwMax ? src[lane + 64] : 0;
        // pre: the particle's record {status, homographies} written by the swarm step (pais_pre.hpp) instead of its position
        const double *rec = PRE ? pre + preD * ((size_t)c * Nmax + iLoad) : nullptr;
        double status0 = 0.0, hv = 0.0;
        if (PRE) {
            status0 = rec[0];
            hv = lane < PAIS_H_STRIDE * Kmax ? rec[PAIS_PRE_HDR + lane] : 0.0;
        }
        // pendingOnly: the launch behind k_pso_tile2 (pais_tile2.hpp) -- only the particles it flagged for the checked walk
        const double pend = pendingOnly ? A.part[iLoad][0] : 1.0;
        if (!active || i >= Nrun || (pend != 1.0 && pendingOnly != 2)) continue;
        wave_sync();
        stage_eval_block(smem, src, nwMax, lane, v0, v1);
        wave_sync();
        double f4[4], w4[4];
        int st;
        if (PRE) st = eval_fitness_pre<NS, BYTES, ACCR, false>(sc, ep, cams, Hbuf, cbuf, win + (size_t)c * WS, rec, status0, hv, lane, f4, w4);
        else st = eval_fitness_parts<NS, BYTES, ACCR>(sc, ep, cams, Hbuf, cbuf, win + (size_t)c * WS, p0, p1, p2, lane, 0, 1, f4, w4);
        if (lane == 0) {
            const double v = st ? DBL_MAX : combine_parts(f4, w4);
            // PAIS_TILE_VERIFY: the tile kernel's value against this walk's; mismatches are counted (and the first one kept)
            // in the debug words -- no printf in this kernel: its mere presence costs every instantiation registers.  Two NaN
            // costs (0 / 0: the weights of all live pixels vanished) agree.
            if (pendingOnly == 2 && pend != 1.0 && verify && A.fit[i] != v && (A.fit[i] == A.fit[i] || v == v)) {
                if (atomicAdd(&verify[0], 1ULL) == 0) {
                    verify[1] = ((unsigned long long)(unsigned)c << 32) | (unsigned)i;
                    verify[2] = (unsigned long long)__double_as_longlong(A.fit[i]);
                    verify[3] = (unsigned long long)__double_as_longlong(v);
                }
            }
            A.fit[i] = v;
        }
    }
}

#include "pais_tile2.hpp"
#include "pais_literal.hpp"

// ------------------------------------------------------------- k_pso_iter ---
// Default PSO pipeline: ONE launch per PSO iteration.  The wave of (candidate c, particle i) first replays
// everything PsoSolver::run() does between two fitness passes (updateFitness, updateGbest, the convergence
// test, the inertia update: psosolver.cpp:121-149, 286-306) from the previous launch's swarm buffer -- the N
// particles of the candidate sit in lanes 0..N-1, so this costs a few hundred instructions instead of a
// dependent k_pso_step launch -- then moves ITS OWN particle (getLocalBest / setNearNeighborBest / moveParticles,
// :151-265), stores it into the other swarm buffer and evaluates the cost there.  Every wave of a candidate
// derives the same loop-carried scalars from the same inputs; particle 0's wave stores them (and, when the run
// ends, the result).  Comparisons and selections are reorganised over lanes, arithmetic is not: each value
// is produced by the same operation sequence as in pso_step_wave / oracle po_pso_run.

// lexicographic wave arg-min over (key, tie) of the lanes with valid != 0; returns the winner's tie or -1
__device__ __forceinline__ int wave_argmin_lex(bool valid, double key, int tie)
{
    double k = key;
    int t = tie;
    int v = valid ? 1 : 0;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double ok = __shfl_xor(k, m, 64);
        const int ot = __shfl_xor(t, m, 64);
        const int ov = __shfl_xor(v, m, 64);
        const bool take = ov && (!v || ok < k || (ok == k && ot < t));
        k = take ? ok : k;
        t = take ? ot : t;
        v = take ? 1 : v;
    }
    return v ? t : -1;
}

// The same selection for a swarm that sits in lanes 0 .. N-1 of the first DPP row(s) (N <= 32: every swarm of an expansion
// candidate or seed with the README's particle count): the exchanges inside a row of 16 lanes are DPP operand modifiers of
// ordinary VALU moves (row_mirror, row_half_mirror, two quad permutations -- four symmetric pairings that together connect
// all 16 lanes) instead of ds_bpermute round trips through the LDS crossbar (~130 cycles each; the step replay of a latency-
// bound launch is a chain of four such selections: measured 16.6 k of the 34 k cycles of a thin launch's wave).  (key, tie)
// pairs are distinct, so any all-to-all pairing order selects the same winner.  Result of lane 0, broadcast.
template <int CTRL> __device__ __forceinline__ int dpp_mov_i(int v) { return __builtin_amdgcn_update_dpp(v, v, CTRL, 0xF, 0xF, false); }
// a permutation in which every lane has a source (rotations, mirrors): no `old` operand, so no copy in front of the move
template <int CTRL> __device__ __forceinline__ int dpp_get_i(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true); }
template <int CTRL> __device__ __forceinline__ void argmin_dpp_step(double &k, int &t, int &v)
{
    // (mirrors and quad permutations give every lane a source: the moves need no `old` operand, i.e. no copy in front of them)
    const int olo = dpp_get_i<CTRL>(__double2loint(k)), ohi = dpp_get_i<CTRL>(__double2hiint(k));
    const int ot = dpp_get_i<CTRL>(t), ov = dpp_get_i<CTRL>(v);
    const double ok = __hiloint2double(ohi, olo);
    const bool take = ov && (!v || ok < k || (ok == k && ot < t));
    k = take ? ok : k;
    t = take ? ot : t;
    v = take ? 1 : v;
}
__device__ __forceinline__ int wave_argmin_lex_n(bool valid, double key, int tie, int N)
{
    if (N > 32) return wave_argmin_lex(valid, key, tie);
    double k = key;
    int t = tie;
    int v = valid ? 1 : 0;
    if (N > 16) { // rows 0 and 1 first (one crossbar exchange)
        const double ok = __shfl_xor(k, 16, 64);
        const int ot = __shfl_xor(t, 16, 64), ov = __shfl_xor(v, 16, 64);
        const bool take = ov && (!v || ok < k || (ok == k && ot < t));
        k = take ? ok : k;
        t = take ? ot : t;
        v = take ? 1 : v;
    }
    argmin_dpp_step<0x140>(k, t, v); // row_mirror: lane i <-> 15 - i
    argmin_dpp_step<0x141>(k, t, v); // row_half_mirror: i <-> 7 - i
    argmin_dpp_step<0x1B>(k, t, v);  // quad_perm [3, 2, 1, 0]
    argmin_dpp_step<0xB1>(k, t, v);  // quad_perm [1, 0, 3, 2]
    return __builtin_amdgcn_readfirstlane(v ? t : -1);
}

// ---- lane-parallel forms of the step replay's serial scans (round 5; swarm of N <= 32 particles in lanes 0 .. N-1) ----------
// profiles/r05_dup_profile.txt: the replay's selections are 6.7 ms of the 80 ms pawn reconstruction's critical path (the
// moveParticles selections 3.9 ms, the gBest scan + convergence sums 2.8 ms), and the ISA shows why -- every `for (j < N)` over
// lane_get(v, j) is a loop of v_readlane_b32 with an SGPR lane index under exec-mask loop control (N came from a vector load),
// ~200 cycles per trip for one wave alone on its SIMD.  Below, each scan is a fixed number of DPP exchanges inside a 16-lane
// row (ordinary VALU moves with a lane-permuting operand modifier: no SGPR round trip, no loop, no branch), one crossbar
// exchange between rows 0 and 1 when N > 16.  Selections only -- every VALUE that is stored is produced by the same
// operation sequence as before, so the records are the same bits (the goldens and the parity suite did not move).
template <int CTRL> __device__ __forceinline__ double dpp_mov_d(double v)
{
    return __hiloint2double(dpp_mov_i<CTRL>(__double2hiint(v)), dpp_mov_i<CTRL>(__double2loint(v)));
}
template <int CTRL> __device__ __forceinline__ double dpp_get_d(double v)
{
    return __hiloint2double(dpp_get_i<CTRL>(__double2hiint(v)), dpp_get_i<CTRL>(__double2loint(v)));
}
// the butterfly of wave_argmin_lex_n as a plain sum: every lane of row 0 ends with the sum over lanes 0 .. 15 (N <= 16) or
// 0 .. 31 (rows 0 and 1).  The association order differs from lane to lane -- callers use lane 0's value (readfirstlane).
__device__ __forceinline__ double swarm_sum_fast(double v, int N)
{
    if (N > 16) v += __shfl_xor(v, 16, 64);
    v += dpp_get_d<0x140>(v); // row_mirror
    v += dpp_get_d<0x141>(v); // row_half_mirror
    v += dpp_get_d<0x1B>(v);  // quad_perm [3, 2, 1, 0]
    v += dpp_get_d<0xB1>(v);  // quad_perm [1, 0, 3, 2]
    return lane_get(v, 0);
}
// `mean of 3 N terms < 0.01` (getDispersionIDX / getVelocityIDX, psosolver.cpp:70-92, 293-297) where the reference adds the
// terms one after the other.  t0, t1, t2: this lane's three terms (lanes >= N: anything).  A tree sum of the same terms differs
// from the sequential sum by < 3 N ulp (~1e-14 relative); when it is farther than 1e-9 from the threshold the comparison cannot
// depend on the order, otherwise (never seen) the sequential sum decides -- the decision is the reference's in every case.
__device__ __forceinline__ bool swarm_mean_below(double t0, double t1, double t2, int lane, int N)
{
    const double own = lane < N ? (t0 + t1) + t2 : 0.0;
    const double fast = swarm_sum_fast(own, N) / (double)(3 * N);
    if (fabs(fast - 0.01) > 1e-9) return fast < 0.01;
    double s = 0;
    for (int j = 0; j < N; ++j) {
        s += lane_get(t0, j);
        s += lane_get(t1, j);
        s += lane_get(t2, j);
    }
    s /= (double)(3 * N);
    return s < 0.01;
}
// updateGbest (psosolver.cpp:137-149): `for j: if (pBestFitness[j] <= gBestFitness) { gBestFitness = ...; gBest = j }` -- the
// scan ends at the LAST index of the swarm's minimum if that minimum is <= the incoming gBestFitness, and leaves (gf, g) alone
// otherwise (a NaN never satisfies `<=`, on either side).
__device__ __forceinline__ void swarm_update_gbest(double pbf, int lane, int N, double &gf, int &g)
{
    const int w = wave_argmin_lex_n(lane < N && pbf == pbf, pbf, 63 - lane, N);
    const int j = 63 - (w < 0 ? 63 : w);
    const double m = lane_get(pbf, j);
    if (w >= 0 && m <= gf) {
        gf = m;
        g = j;
    }
}
// the two scans for ANY swarm in lanes (N <= 64): beyond the two DPP rows, the reference's own sequential walk over the lanes
__device__ __forceinline__ bool swarm_mean_below_any(double t0, double t1, double t2, int lane, int N)
{
    if (N <= 32) return swarm_mean_below(t0, t1, t2, lane, N);
    double s = 0;
    for (int j = 0; j < N; ++j) {
        s += lane_get(t0, j);
        s += lane_get(t1, j);
        s += lane_get(t2, j);
    }
    s /= (double)(3 * N);
    return s < 0.01;
}
__device__ __forceinline__ void swarm_update_gbest_any(double pbf, int lane, int N, double &gf, int &g)
{
    if (N <= 32) {
        swarm_update_gbest(pbf, lane, N, gf, g);
        return;
    }
    for (int j = 0; j < N; ++j) {
        const double v = lane_get(pbf, j);
        if (v <= gf) {
            gf = v;
            g = j;
        }
    }
}
// rank(lane) = #{ j < N : d_j < d_lane or (d_j == d_lane and j < lane) } -- getLocalBest's stable sort position
// (psosolver.cpp:151-191) -- by rotating the distances through the 16-lane row (row_ror:n, n = 1 .. 15: every other lane of the
// row exactly once).  The source lane's index travels with its value, so the tie-break does not rest on the direction of the
// rotation.  Lanes N .. 31 must hold DBL_MAX.
template <int n> __device__ __forceinline__ int rank_ror(double dj, int lane)
{
    const double o = dpp_get_d<0x120 + n>(dj);
    const int j = dpp_get_i<0x120 + n>(lane);
    return (o < dj || (o == dj && j < lane)) ? 1 : 0;
}
template <int n> __device__ __forceinline__ int rank_ror_other(double dj, double od, bool hiRow)
{
    const double o = dpp_get_d<0x120 + n>(od);
    return (o < dj || (o == dj && hiRow)) ? 1 : 0;
}
__device__ __forceinline__ int swarm_rank(double dj, int lane, int N)
{
    int rank = 0;
    rank += rank_ror<1>(dj, lane);  rank += rank_ror<2>(dj, lane);  rank += rank_ror<3>(dj, lane);  rank += rank_ror<4>(dj, lane);
    rank += rank_ror<5>(dj, lane);  rank += rank_ror<6>(dj, lane);  rank += rank_ror<7>(dj, lane);  rank += rank_ror<8>(dj, lane);
    rank += rank_ror<9>(dj, lane);  rank += rank_ror<10>(dj, lane); rank += rank_ror<11>(dj, lane); rank += rank_ror<12>(dj, lane);
    rank += rank_ror<13>(dj, lane); rank += rank_ror<14>(dj, lane); rank += rank_ror<15>(dj, lane);
    if (N > 16) { // the other row's sixteen (rows 0 and 1 exchanged through the crossbar): every one of them precedes a lane of
                  // row 1, none a lane of row 0
        const double od = __shfl_xor(dj, 16, 64);
        const bool hiRow = (lane & 16) != 0;
        rank += (od < dj || (od == dj && hiRow)) ? 1 : 0;
        rank += rank_ror_other<1>(dj, od, hiRow);  rank += rank_ror_other<2>(dj, od, hiRow);  rank += rank_ror_other<3>(dj, od, hiRow);
        rank += rank_ror_other<4>(dj, od, hiRow);  rank += rank_ror_other<5>(dj, od, hiRow);  rank += rank_ror_other<6>(dj, od, hiRow);
        rank += rank_ror_other<7>(dj, od, hiRow);  rank += rank_ror_other<8>(dj, od, hiRow);  rank += rank_ror_other<9>(dj, od, hiRow);
        rank += rank_ror_other<10>(dj, od, hiRow); rank += rank_ror_other<11>(dj, od, hiRow); rank += rank_ror_other<12>(dj, od, hiRow);
        rank += rank_ror_other<13>(dj, od, hiRow); rank += rank_ror_other<14>(dj, od, hiRow); rank += rank_ror_other<15>(dj, od, hiRow);
    }
    return rank;
}

// FOUR lexicographic arg-mins at once (N <= 32): the selections of moveParticles -- the local best and the three per-dimension
// near-neighbour bests -- are independent chains of five dependent exchange-compare-select steps; written one after the other
// each waits for itself (1.5 us of the 13.3 us thin launch for the three FDR selections alone, profiles/r05_thin_launch_latency_
// budget.txt), interleaved step by step the four chains fill each other's latencies.  Same pairings, same comparisons as
// wave_argmin_lex_n: the same winners.
template <int CTRL> __device__ __forceinline__ void argmin4_dpp_step(double (&k)[4], int (&t)[4], int (&v)[4])
{
    int olo[4], ohi[4], ot[4], ov[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        olo[c] = dpp_get_i<CTRL>(__double2loint(k[c]));
        ohi[c] = dpp_get_i<CTRL>(__double2hiint(k[c]));
        ot[c] = dpp_get_i<CTRL>(t[c]);
        ov[c] = dpp_get_i<CTRL>(v[c]);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const double ok = __hiloint2double(ohi[c], olo[c]);
        const bool take = ov[c] && (!v[c] || ok < k[c] || (ok == k[c] && ot[c] < t[c]));
        k[c] = take ? ok : k[c];
        t[c] = take ? ot[c] : t[c];
        v[c] = take ? 1 : v[c];
    }
}
__device__ __forceinline__ void wave_argmin4_lex_n(const bool (&valid)[4], const double (&key)[4], const int (&tie)[4], int N, int (&out)[4])
{
    double k[4];
    int t[4], v[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) { k[c] = key[c]; t[c] = tie[c]; v[c] = valid[c] ? 1 : 0; }
    if (N > 16) { // rows 0 and 1 first (one crossbar exchange per word)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const double ok = __shfl_xor(k[c], 16, 64);
            const int ot = __shfl_xor(t[c], 16, 64), ov = __shfl_xor(v[c], 16, 64);
            const bool take = ov && (!v[c] || ok < k[c] || (ok == k[c] && ot < t[c]));
            k[c] = take ? ok : k[c];
            t[c] = take ? ot : t[c];
            v[c] = take ? 1 : v[c];
        }
    }
    argmin4_dpp_step<0x140>(k, t, v); // row_mirror
    argmin4_dpp_step<0x141>(k, t, v); // row_half_mirror
    argmin4_dpp_step<0x1B>(k, t, v);  // quad_perm [3, 2, 1, 0]
    argmin4_dpp_step<0xB1>(k, t, v);  // quad_perm [1, 0, 3, 2]
#pragma unroll
    for (int c = 0; c < 4; ++c) out[c] = __builtin_amdgcn_readfirstlane(v[c] ? t[c] : -1);
}

// moveParticles for particle i with the swarm in lanes (lane j = particle j, N <= 64): same selections as
// pso_move_particle (pais_dev.hpp), evaluated across lanes
__device__ __forceinline__ void pso_move_own(int i, int N, int localK, double iw, const double *u, const double *pos,
                                             const double *pb, double fitj, double pbf, int lane, const double *gB,
                                             const double *rl, const double *ru, const double *vecI, const double *nbI,
                                             double *outP, double *outV, double *outNb)
{
    const double pw = 1.2, gw = 1.5, lw = 1.0, nw = 1.0; // psosolver.h:110
    const double pVecW = pw * u[0], gVecW = gw * u[1], lVecW = lw * u[2], nVecW = nw * u[3];
    const bool pv = lane < N;
    const double pp0 = lane_get(pb[0], i), pp1 = lane_get(pb[1], i), pp2 = lane_get(pb[2], i);
    // getLocalBest: the localK nearest pBests by (squared distance, index); among them the first strict minimum
    // of pBestFitness in selection order
    double dj;
    {
        const double d0 = pp0 - pb[0], d1 = pp1 - pb[1], d2 = pp2 - pb[2];
        dj = 0;
        dj += d0 * d0;
        dj += d1 * d1;
        dj += d2 * d2;
        // (self: DBL_MAX, psosolver.cpp:161; lanes beyond the swarm: +inf, behind every particle in every order -- also behind
        //  one whose squared distance overflowed to +inf: equal keys are ordered by lane, and they have the higher lanes)
        dj = (lane == i) ? DBL_MAX : (!pv ? __builtin_inf() : dj);
    }
    int rank = 0;
    if (N <= 32) {
        rank = swarm_rank(dj, lane, N);
    } else {
        for (int j = 0; j < N; ++j) {
            const double o = lane_get(dj, j);
            rank += (o < dj || (o == dj && j < lane)) ? 1 : 0;
        }
    }
    const bool sel = pv && rank < localK;
    // setNearNeighborBest: per dimension the first maximum of the fitness-distance ratio
    const double fitI = lane_get(fitj, i);
    if (N <= 32) {
        // the four selections side by side (wave_argmin4_lex_n)
        double FDR[3];
        for (int d = 0; d < 3; ++d) {
            const double pd = lane_get(pos[d], i);
            FDR[d] = (fitI - pbf) / fabs(pd - pb[d]);
        }
        const bool valid[4] = {sel && pbf < DBL_MAX, pv && lane != i && FDR[0] > -DBL_MAX, pv && lane != i && FDR[1] > -DBL_MAX,
                               pv && lane != i && FDR[2] > -DBL_MAX};
        const double key[4] = {pbf, -FDR[0], -FDR[1], -FDR[2]};
        const int tie[4] = {rank * 64 + lane, lane, lane, lane};
        int win[4];
        wave_argmin4_lex_n(valid, key, tie, N, win);
        const int lIdx4 = (win[0] < 0) ? i : (win[0] & 63);
        for (int d = 0; d < 3; ++d) {
            const int wn = win[1 + d];
            const double o = lane_get(pb[d], wn < 0 ? 0 : wn);
            outNb[d] = (wn < 0) ? nbI[d] : o;
        }
        for (int d = 0; d < 3; ++d) {
            double p = lane_get(pos[d], i);
            const double pbi = lane_get(pb[d], i), pbl = lane_get(pb[d], lIdx4);
            double v = iw * vecI[d] + pVecW * (pbi - p) + gVecW * (gB[d] - p) + lVecW * (pbl - p) + nVecW * (outNb[d] - p);
            outV[d] = v;
            p += v;
            if (p > ru[d]) p = ru[d];
            if (p < rl[d]) p = rl[d];
            outP[d] = p;
        }
        return;
    }
    const int w = wave_argmin_lex_n(sel && pbf < DBL_MAX, pbf, rank * 64 + lane, N);
    const int lIdx = (w < 0) ? i : (w & 63);
    for (int d = 0; d < 3; ++d) {
        const double pd = lane_get(pos[d], i);
        const double FDR = (fitI - pbf) / fabs(pd - pb[d]);
        const bool cand = pv && lane != i && FDR > -DBL_MAX;
        const int wn = wave_argmin_lex_n(cand, -FDR, lane, N);
        const double o = lane_get(pb[d], wn < 0 ? 0 : wn);
        outNb[d] = (wn < 0) ? nbI[d] : o;
    }
    for (int d = 0; d < 3; ++d) {
        double p = lane_get(pos[d], i);
        const double pbi = lane_get(pb[d], i), pbl = lane_get(pb[d], lIdx);
        double v = iw * vecI[d] + pVecW * (pbi - p) + gVecW * (gB[d] - p) + lVecW * (pbl - p) + nVecW * (outNb[d] - p);
        outV[d] = v;
        p += v;
        if (p > ru[d]) p = ru[d];
        if (p < rl[d]) p = rl[d];
        outP[d] = p;
    }
}

// launch L = 0: cost of the initial swarm.  L >= 1: step (L-1) + cost of the moved particle.  finishOnly: one
// wave per candidate that only replays the step (the launch after the last possible iteration: every run ends).
// Tasks: positions [listLo, min(listHi, *activeCount)) of the active list written by k_pso_init.
// NS = 2 (3 waves per SIMD) for patches seen by few cameras, NS = 1 (4 waves per SIMD) beyond: a wave's LDS scratch
// grows with NS * K and caps the occupancy (measured: K ~ 4: NS 2 +3 %, K ~ 7: NS 1 +9 %)
template <int nparts, int NS, bool BYTES, bool ACCR>
__global__ PAIS_ITER_BOUNDS(nparts, NS) void k_pso_iter(DevScene sc, unsigned char *states, const int *activeList,
                                            const int *activeCount, int listLo, int listHi, int Nmax, int Kmax,
                                            pais_patch_result *recs, unsigned long long *stat, int L, int finishOnly,
                                            const unsigned char *evalBlocks, size_t evalBlockBytes, const WinPix *win)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem0[];
    unsigned char *smem = smem0 + (threadIdx.x >> 6) * eval_lds_bytes(NS, Kmax, ACCR); // wave-private scratch
    EvalPatch *ep = (EvalPatch *)smem;
    EvalCam *cams = (EvalCam *)(smem + sizeof(EvalPatch));
    double *Hbuf = (double *)(smem + eval_block_bytes(Kmax));
    double *cbuf = Hbuf + Kmax * PAIS_H_STRIDE;
    const int lane = threadIdx.x & 63;
    const size_t SB = pso_state_bytes(Nmax);
    const int WS = win_stride(sc);
    // nparts (1, 2, 4) consecutive waves share one evaluation: small rounds are bound by the latency of a
    // single evaluation wave, not by throughput.  Every part replays the step (identical results), part 0
    // stores the moved particle, each part stores its sub-accumulators; the consumer -- the step replay of
    // the next launch -- adds them in the canonical order.
    const int per = finishOnly ? 1 : Nmax * nparts;
    const int nAct = *activeCount;
    const int total = ((listHi < nAct ? listHi : nAct) - listLo) * per;
    for (int t = eval_first_task(); t < total; t += eval_task_stride()) {
        const int lp = t / per, ip = t - lp * per;
        const int c = activeList[listLo + lp];
        const int i = ip / nparts, part = ip - i * nparts;
        PsoState *hd = (PsoState *)(states + SB * (size_t)c);
        // the candidate's evaluation constants are requested now and stored to LDS after the step replay: their memory
        // round trip overlaps the replay's
        const uint64_t *src = (const uint64_t *)(evalBlocks + evalBlockBytes * (size_t)c);
        const int nwMax = (int)(eval_block_bytes(Kmax) / 8);
        const uint64_t v0 = lane < nwMax ? src[lane] : 0, v1 = lane + 64 < nwMax ? src[lane + 64] : 0;
        // ... and so is everything the step replay reads: all addresses follow from c, i and the lane alone (particle
        // j of the swarm in lane j), so the run's flags, the swarm and the loop-carried scalars come back in ONE memory
        // round trip; a finished run wastes these loads
        PsoArrays Wb = pso_arrays((unsigned char *)hd, Nmax, L & 1);
        PsoArrays Rb = pso_arrays((unsigned char *)hd, Nmax, (L > 0 ? L - 1 : 0) & 1);
        const int jl = lane < Nmax ? lane : 0;
        // (wave-uniform by construction -- every lane loads the same word; said so, or the compiler keeps them in VGPRs and
        //  runs every loop over them under exec-mask control)
        const int active = __builtin_amdgcn_readfirstlane(hd->active), N = __builtin_amdgcn_readfirstlane(hd->N),
                  maxIt = __builtin_amdgcn_readfirstlane(hd->maxIt);
        PsoState::IterDyn dr = hd->dyn[(L > 0 ? L - 1 : 0) & 1];
        dr.started = __builtin_amdgcn_readfirstlane(dr.started);
        dr.iteration = __builtin_amdgcn_readfirstlane(dr.iteration);
        dr.gIdx = __builtin_amdgcn_readfirstlane(dr.gIdx);
        // (what only moveParticles reads is requested here too: behind the convergence test it would be a second round trip)
        const double rl[3] = {hd->rangeL[0], hd->rangeL[1], hd->rangeL[2]};
        const double ru[3] = {hd->rangeU[0], hd->rangeU[1], hd->rangeU[2]};
        const uint64_t streamBase = hd->streamBase;
        const int runIdx = __builtin_amdgcn_readfirstlane(hd->run), localK = __builtin_amdgcn_readfirstlane(hd->localK);
        double pos[3], pb[3];
        for (int d = 0; d < 3; ++d) {
            pos[d] = Rb.pos[jl][d];
            pb[d] = Rb.pBest[jl][d];
        }
        double fitj;
        if (nparts == 1) {
            fitj = Rb.fit[jl];
        } else {
            double f4[4], w4[4];
            bool bad = false;
            for (int a = 0; a < 4; ++a) {
                f4[a] = Rb.part[jl][2 * a];
                w4[a] = Rb.part[jl][2 * a + 1];
                bad = bad || (w4[a] < 0); // a part's call overflowed: DBL_MAX
            }
            fitj = bad ? DBL_MAX : combine_parts(f4, w4);
        }
        double pbf = Rb.pBestFit[jl];
        const double vecI[3] = {Rb.vec[i][0], Rb.vec[i][1], Rb.vec[i][2]};
        const double nbI[3] = {Rb.nBest[i][0], Rb.nBest[i][1], Rb.nBest[i][2]};
        const double q0 = Wb.pos[i][0], q1 = Wb.pos[i][1], q2 = Wb.pos[i][2]; // launch 0: the initial swarm
        if (!active || i >= N) continue;
        double p0, p1, p2;
        if (L == 0) {
            p0 = q0;
            p1 = q1;
            p2 = q2;
        } else {
            int it, g;
            double gf, iw;
            if (!dr.started) {
                // initFitness (:112-119) + run(): gBest = particles[0].pBest; updateGbest (:137-149)
                pbf = fitj;
                g = 0;
                gf = lane_get(pbf, 0);
                iw = dr.iw;
                it = 0;
            } else {
                // updateFitness (:121-135): pBest on strict '<'
                if (fitj < pbf) {
                    pbf = fitj;
                    pb[0] = pos[0];
                    pb[1] = pos[1];
                    pb[2] = pos[2];
                }
                g = dr.gIdx;
                gf = dr.gBestFitness;
                const double niw = dr.iw - 1.0 / maxIt; // :304
                iw = niw > 0.4 ? niw : 0.4;
                it = dr.iteration + 1;
            }
            if (N <= 32) {
                swarm_update_gbest(pbf, lane, N, gf, g);
            } else {
                for (int j = 0; j < N; ++j) {
                    const double v = lane_get(pbf, j);
                    if (v <= gf) {
                        gf = v;
                        g = j;
                    }
                }
            }
            const double gB[3] = {lane_get(pb[0], g), lane_get(pb[1], g), lane_get(pb[2], g)};
            // loop head of run(): `iteration < maxIteration`, then the convergence break (:293-297)
            bool finished = it >= maxIt;
            if (!finished) {
                const double a0 = fabs(pos[0] - gB[0]), a1 = fabs(pos[1] - gB[1]), a2 = fabs(pos[2] - gB[2]);
                bool dispBelow;
                if (N <= 32) {
                    dispBelow = swarm_mean_below(a0, a1, a2, lane, N);
                } else {
                    double disp = 0;
                    for (int j = 0; j < N; ++j) {
                        disp += lane_get(a0, j);
                        disp += lane_get(a1, j);
                        disp += lane_get(a2, j);
                    }
                    disp /= (double)(3 * N);
                    dispBelow = disp < 0.01;
                }
                if (dispBelow) {
                    const double v0 = fabs(Rb.vec[jl][0]), v1 = fabs(Rb.vec[jl][1]), v2 = fabs(Rb.vec[jl][2]);
                    if (N <= 32) {
                        finished = swarm_mean_below(v0, v1, v2, lane, N);
                    } else {
                        double vel = 0;
                        for (int j = 0; j < N; ++j) {
                            vel += lane_get(v0, j);
                            vel += lane_get(v1, j);
                            vel += lane_get(v2, j);
                        }
                        vel /= (double)(3 * N);
                        finished = vel < 0.01;
                    }
                }
            }
            if (finished) {
                if (i == 0 && part == 0 && lane == 0) {
                    // write back (patch.cpp:208-213) and the maxFitness gate (:156-159)
                    pais_patch_result *P = &recs[c];
                    double nn[3];
                    spherical2normal(gB[0], gB[1], nn);
                    P->fitness = gf;
                    P->normalS[0] = gB[0];
                    P->normalS[1] = gB[1];
                    for (int q = 0; q < 3; ++q) P->normal[q] = nn[q];
                    P->depth = gB[2];
                    const DevCamera &rc = sc.cams[hd->refCam];
                    for (int q = 0; q < 3; ++q) P->center[q] = hd->ray[q] * gB[2] + rc.C[q];
                    P->pso_runs += 1;
                    P->pso_iterations += it;
                    const int evals = N * (1 + it);
                    P->pso_evals += evals;
                    if (gf > sc.cfg.maxFitness) {
                        P->dropped = 1;
                        P->stage = PAIS_STAGE_DONE;
                    } else {
                        P->stage = PAIS_STAGE_AFTER;
                    }
                    hd->active = 0;
                    const int K = hd->K;
                    const unsigned long long perEval = (unsigned long long)(4 * K + 1 + (sc.cfg.adaptiveDistanceEnable ? 8 : 0) +
                                                                            (sc.cfg.adaptiveGradientEnable ? 8 : 0));
                    atomicAdd(&stat[0], (unsigned long long)evals);
                    atomicAdd(&stat[1], (unsigned long long)evals * perEval);
                    atomicAdd(&stat[2], 1ULL);
                }
                continue;
            }
            // moveParticles (:220-265) for iteration `it`, own particle only
            double u[4];
            const uint32_t k0 = (uint32_t)(6 * N + 3 + 4 * (it * N + i));
            for (int q = 0; q < 4; ++q) u[q] = uniform_from(streamBase, (uint32_t)runIdx, k0 + q);
            double nP[3], nV[3], nNb[3];
            pso_move_own(i, N, localK, iw, u, pos, pb, fitj, pbf, lane, gB, rl, ru, vecI, nbI, nP, nV, nNb);
            const double pbI[3] = {lane_get(pb[0], i), lane_get(pb[1], i), lane_get(pb[2], i)};
            const double pbfI = lane_get(pbf, i);
            if (lane == 0 && part == 0) {
                for (int d = 0; d < 3; ++d) {
                    Wb.pos[i][d] = nP[d];
                    Wb.vec[i][d] = nV[d];
                    Wb.pBest[i][d] = pbI[d];
                    Wb.nBest[i][d] = nNb[d];
                }
                Wb.pBestFit[i] = pbfI;
                if (i == 0) {
                    PsoState::IterDyn dw;
                    dw.iw = iw;
                    dw.gBestFitness = gf;
                    dw.gIdx = g;
                    dw.iteration = it;
                    dw.started = 1;
                    dw.pad = 0;
                    hd->dyn[L & 1] = dw;
                }
            }
            p0 = nP[0];
            p1 = nP[1];
            p2 = nP[2];
        }
        if (finishOnly) continue; // unreachable for a well-formed schedule: every run has ended by now
        wave_sync();
        stage_eval_block(smem, src, nwMax, lane, v0, v1); // the run's evaluation block, prepared by k_pso_init
        wave_sync();
        double f4[4], w4[4];
        const int st = eval_fitness_parts<NS, BYTES, ACCR>(sc, ep, cams, Hbuf, cbuf, win + (size_t)c * WS, p0, p1, p2, lane, part, nparts, f4, w4);
        if (lane == 0) {
            if (nparts == 1) {
                Wb.fit[i] = st ? DBL_MAX : combine_parts(f4, w4);
            } else {
                for (int a = part; a < 4; a += nparts) {
                    Wb.part[i][2 * a] = st ? 0.0 : f4[a];
                    Wb.part[i][2 * a + 1] = st ? -1.0 : w4[a];
                }
            }
        }
    }
}

// Everything of PsoSolver::run() between two fitness passes, for ONE candidate, by one wave.
// smem: Nmax*(3*4+2) doubles of LDS scratch.
// Everything it reads was written by a previous launch.  Returns 1 if the run continues.
// COH: the state was written by another wave of THIS launch (k_pso_ring) and is read / written coherently
// pre != nullptr: the records of the moved swarm's evaluations (pais_pre.hpp) are written as well -- preEp / preCams: the
// candidate's evaluation block in LDS; pre: the candidate's first record; preD: doubles per record
// Sink: what the step records of the swarm it has just updated (pais_pso_trace).  StepNoSink records nothing: every statement
// of the trace is `if constexpr` and vanishes, so k_pso_step, k_pso_ring and every other kernel compile as before.
// StepTraceSink writes, after the convergence test and before moveParticles / the write-back, the row (candidate c, hd->run,
// iteration) -- the header by lane 0, the particles from the LDS swarm by their lanes -- and, on a run's row 0, the run's info
// from the PsoState header k_begin / k_pso_init filled; nothing for runs >= maxRuns.
//
// Swarms of N <= 64 particles (every swarm a ring pass or k_pso_iter can hold) take the lane-parallel form:
//   * every global load of the step is requested at its top -- all addresses follow from the candidate and the lane, so the
//     swarm, the loop-carried scalars and what only moveParticles reads come back in ONE memory round trip (as in k_pso_iter);
//   * particle j sits in lane j: the pBest update is one compare per lane; at N <= 32 (every swarm of the README's particle
//     count, seeds included) updateGbest and the two convergence means are the DPP forms of k_pso_iter (swarm_update_gbest,
//     swarm_mean_below) -- no serial scan through LDS, no barrier;
//   * moveParticles runs with 4 (N <= 16), 2 (N <= 32) or 1 lane per particle (pso_move_lanes below).
// The LDS arrays still hold the swarm after the fitness update (the trace sink, the moved rows, swarm_eval_setup read them).
// Larger swarms (k_pso_step only) keep the serial LDS form.

// lexicographic (key, j) minimum / (key, j) "first maximum" with the partner lane of a DPP pairing; j < 0: nothing selected yet
template <int CTRL> __device__ __forceinline__ void group_min_step(double &k, int &j)
{
    const double ok = dpp_get_d<CTRL>(k);
    const int oj = dpp_get_i<CTRL>(j);
    const bool take = oj >= 0 && (j < 0 || ok < k || (ok == k && oj < j));
    k = take ? ok : k;
    j = take ? oj : j;
}
template <int CTRL> __device__ __forceinline__ void group_max_step(double &k, int &j, double &val)
{
    const double ok = dpp_get_d<CTRL>(k), oval = dpp_get_d<CTRL>(val);
    const int oj = dpp_get_i<CTRL>(j);
    const bool take = oj >= 0 && (j < 0 || ok > k || (ok == k && oj < j));
    k = take ? ok : k;
    j = take ? oj : j;
    val = take ? oval : val;
}
// moveParticles for the whole swarm in LDS (N <= 64), G = 4 (N <= 16), 2 (N <= 32) or 1 adjacent lanes per particle: lane (i, s)
// walks the partners j = s, s + G, ... of particle i -- the distance selections of getLocalBest and the three fitness-distance-
// ratio selections of setNearNeighborBest -- and the G lanes combine with lexicographic selections inside their quad (DPP quad
// permutations).  Selections only: the partner a serial walk over j = 0 .. N-1 selects (pso_move_particle) is the
// lexicographically first of the lanes' own selections --
//   getLocalBest: `dist < bd` keeps the lowest j of the smallest distance among the partners not yet taken; j == i takes part
//                 with DBL_MAX; a round that finds nobody (localK > N) ends the walk;
//   FDR:          `FDR > maxFDR` from -DBL_MAX keeps the lowest j of the largest ratio; a NaN, -inf or -DBL_MAX never wins.
// (Squared distances of finite pBests are never NaN.)  Every stored value -- vec, pos, nBest -- is the operation sequence of
// pso_move_particle on the same operands; the G lanes of a particle compute the same bits and lane s == 0 writes the rows.
// The walks stay rolled and a round takes its distances from LDS again: kept distances or unrolled walks (nine to forty-eight
// divisions in flight) cost k_pso_ring scratch and the one-pixel ring kernels their third wave.  ALL 64 lanes must be active.
__device__ __forceinline__ void pso_move_lanes(int N, int localK, double iw, int it, uint64_t sb, uint32_t run, double (*pos)[3],
                                               double (*vec)[3], const double (*pBest)[3], double (*nBest)[3], const double *fit,
                                               const double *pBestFit, const double *gBest, const double *rangeL, const double *rangeU,
                                               int lane)
{
    const double pw = 1.2, gw = 1.5, lw = 1.0, nw = 1.0; // psosolver.h:110
    const int sh = N <= 16 ? 2 : (N <= 32 ? 1 : 0), G = 1 << sh; // (wave-uniform)
    const int i0 = lane >> sh, s = lane & (G - 1);
    const bool live = i0 < N;
    const int i = live ? i0 : 0;
    const double pp0 = pBest[i][0], pp1 = pBest[i][1], pp2 = pBest[i][2];
    const double pI[3] = {pos[i][0], pos[i][1], pos[i][2]};
    const double vI[3] = {vec[i][0], vec[i][1], vec[i][2]};
    const double nbI[3] = {nBest[i][0], nBest[i][1], nBest[i][2]};
    const double fitness = fit[i];
    double u[4];
    const uint32_t k0 = (uint32_t)(6 * N + 3 + 4 * (it * N + i));
    for (int q = 0; q < 4; ++q) u[q] = uniform_from(sb, run, k0 + q);
    const double pVecW = pw * u[0], gVecW = gw * u[1], lVecW = lw * u[2], nVecW = nw * u[3];
    const int np = (N + G - 1) >> sh; // partners per lane (a lane whose last partner is beyond the swarm skips it by `j < N`)
    // setNearNeighborBest: one walk over the lane's partners, the three dimensions side by side
    double maxFDR[3] = {-DBL_MAX, -DBL_MAX, -DBL_MAX};
    double nb[3] = {nbI[0], nbI[1], nbI[2]};
    int nj[3] = {-1, -1, -1};
#pragma unroll 1
    for (int p = 0; p < np; ++p) {
        const int j = s + (p << sh);
        const int jj = j < N ? j : 0;
        const double bd[3] = {pBest[jj][0], pBest[jj][1], pBest[jj][2]}, bf = pBestFit[jj];
        const bool other = j < N && j != i;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const double FDR = (fitness - bf) / fabs(pI[d] - bd[d]);
            if (other && FDR > maxFDR[d]) {
                maxFDR[d] = FDR;
                nb[d] = bd[d];
                nj[d] = j;
            }
        }
    }
    if (G >= 2) {
#pragma unroll
        for (int d = 0; d < 3; ++d) group_max_step<0xB1>(maxFDR[d], nj[d], nb[d]); // quad_perm [1, 0, 3, 2]: s ^ 1
    }
    if (G == 4) {
#pragma unroll
        for (int d = 0; d < 3; ++d) group_max_step<0x4E>(maxFDR[d], nj[d], nb[d]); // quad_perm [2, 3, 0, 1]: s ^ 2
    }
    // getLocalBest: localK rounds, each the nearest partner not yet taken; among them the first strict minimum of pBestFitness
    uint64_t taken = 0;
    double minFitness = DBL_MAX;
    int lIdx = i;
#pragma unroll 1
    for (int k = 0; k < localK; ++k) {
        double bd = 0;
        int bj = -1;
#pragma unroll 1
        for (int p = 0; p < np; ++p) {
            const int j = s + (p << sh);
            const int jj = j < N ? j : 0;
            double dj;
            {
                const double d0 = pp0 - pBest[jj][0], d1 = pp1 - pBest[jj][1], d2 = pp2 - pBest[jj][2];
                dj = 0;
                dj += d0 * d0;
                dj += d1 * d1;
                dj += d2 * d2;
                if (j == i) dj = DBL_MAX; // psosolver.cpp:161
            }
            if (j < N && !((taken >> p) & 1) && (bj < 0 || dj < bd)) {
                bd = dj;
                bj = j;
            }
        }
        if (G >= 2) group_min_step<0xB1>(bd, bj);
        if (G == 4) group_min_step<0x4E>(bd, bj);
        if (bj >= 0) {
            if ((bj & (G - 1)) == s) taken |= 1ULL << (bj >> sh);
            const double f = pBestFit[bj];
            if (f < minFitness) {
                minFitness = f;
                lIdx = bj;
            }
        }
    }
    const double pl[3] = {pBest[lIdx][0], pBest[lIdx][1], pBest[lIdx][2]};
    const double pb[3] = {pp0, pp1, pp2};
    double nP[3], nV[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        double p = pI[d];
        double v = iw * vI[d] + pVecW * (pb[d] - p) + gVecW * (gBest[d] - p) + lVecW * (pl[d] - p) + nVecW * (nb[d] - p);
        nV[d] = v;
        p += v;
        if (p > rangeU[d]) p = rangeU[d];
        if (p < rangeL[d]) p = rangeL[d];
        nP[d] = p;
    }
    wave_sync(); // every lane has read its particle's rows
    if (live && s == 0) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            nBest[i][d] = nb[d];
            vec[i][d] = nV[d];
            pos[i][d] = nP[d];
        }
    }
}

struct StepNoSink {
    static constexpr bool on = false;
};
struct StepTraceSink {
    static constexpr bool on = true;
    pais_pso_run_info *runs; // [n][maxRuns]
    pais_pso_iter *iters;    // [n][maxRuns][rows]
    double *particles;       // nullptr or [n][maxRuns][rows][NP][11]
    int maxRuns, rows, NP;
};
// LANES: the lane-parallel form (N <= 64).  The two forms are two instances of one body, chosen once at the top; k_pso_ring
// holds the lane-parallel one alone (both forms in one kernel cost it 70 bytes of scratch per lane).
// PARTS (lane-parallel form, k_pso_ring with several waves per evaluation): the fitness of particle j is put together from the
// (f, w) sub-accumulators the part waves delivered -- k_pso_iter's statement -- instead of being read from A.fit
template <bool COH, class Sink, bool LANES, bool PARTS = false>
__device__ __forceinline__ int pso_step_body(const DevScene &sc, pais_patch_result *recs, int c, PsoState *hd, int N, int Nmax,
                                             unsigned char *smem, unsigned long long *stat, int lane, const EvalPatch *preEp,
                                             const EvalCam *preCams, double *pre, size_t preD, const Sink &sink)
{
    double(*pos)[3] = (double(*)[3])smem;
    double(*vec)[3] = pos + Nmax;
    double(*pBest)[3] = vec + Nmax;
    double(*nBest)[3] = pBest + Nmax;
    double *fit = (double *)(nBest + Nmax);
    double *pBestFit = fit + Nmax;
    PsoArrays A = pso_arrays((unsigned char *)hd, Nmax);
    int maxIt = hd->maxIt;
    constexpr bool lanes = LANES; // the swarm in registers, particle j in lane j
    int it, g, run = 0, localK = 0;
    double gf, iw, rl[3], ru[3], rPos[3], rVec[3], rPb[3];
    uint64_t sb = 0;
    __syncthreads();
    if (lanes) {
        // Everything the step reads, requested before anything waits: the addresses follow from the candidate and the lane
        // alone, so the swarm, the loop-carried scalars and what only moveParticles reads come back in ONE memory round trip.
        // (In k_pso_ring this is behind the arrival count that made this wave the last arriver: the other waves' fitness
        // values are at the coherence point.)
        const int jl = lane < N ? lane : 0;
        it = sload<COH>(&hd->iteration);
        g = sload<COH>(&hd->gIdx);
        gf = sload<COH>(&hd->gBestFitness);
        iw = sload<COH>(&hd->iw);
        int started = sload<COH>(&hd->started);
        for (int d = 0; d < 3; ++d) {
            rl[d] = hd->rangeL[d];
            ru[d] = hd->rangeU[d];
        }
        sb = hd->streamBase;
        run = hd->run;
        localK = hd->localK;
        double rNb[3];
        for (int d = 0; d < 3; ++d) {
            rPos[d] = sload<COH>(&A.pos[jl][d]);
            rVec[d] = sload<COH>(&A.vec[jl][d]);
            rPb[d] = sload<COH>(&A.pBest[jl][d]);
            rNb[d] = sload<COH>(&A.nBest[jl][d]);
        }
        double rFit;
        if constexpr (PARTS) {
            double f4[4], w4[4];
            bool bad = false;
            for (int a = 0; a < 4; ++a) {
                f4[a] = sload<COH>(&A.part[jl][2 * a]);
                w4[a] = sload<COH>(&A.part[jl][2 * a + 1]);
                bad = bad || (w4[a] < 0); // a part's call overflowed: DBL_MAX
            }
            rFit = bad ? DBL_MAX : combine_parts(f4, w4);
        } else {
            rFit = sload<COH>(&A.fit[jl]);
        }
        double rPbf = sload<COH>(&A.pBestFit[jl]);
        // (wave-uniform by construction -- every lane loaded the same word; said so, they live in SGPRs through the step)
        // -- and only here, behind the last request, so that no wait stands between the loads whatever the scheduler does
        it = __builtin_amdgcn_readfirstlane(it);
        g = __builtin_amdgcn_readfirstlane(g);
        maxIt = __builtin_amdgcn_readfirstlane(maxIt);
        started = __builtin_amdgcn_readfirstlane(started);
        run = __builtin_amdgcn_readfirstlane(run);
        localK = __builtin_amdgcn_readfirstlane(localK);
        gf = lane_get(gf, 0);
        iw = lane_get(iw, 0);
        for (int d = 0; d < 3; ++d) {
            rl[d] = lane_get(rl[d], 0);
            ru[d] = lane_get(ru[d], 0);
        }
        sb = (uint64_t)__double_as_longlong(lane_get(__longlong_as_double((long long)sb), 0));
        if (!started) {
            // initFitness (:112-119) + run(): gBest = particles[0].pBest; updateGbest (:137-149)
            rPbf = rFit;
            g = 0;
            gf = lane_get(rPbf, 0);
            it = 0;
        } else {
            // updateFitness (:121-135): pBest on strict '<'
            if (rFit < rPbf) {
                rPbf = rFit;
                rPb[0] = rPos[0];
                rPb[1] = rPos[1];
                rPb[2] = rPos[2];
            }
            const double niw = iw - 1.0 / maxIt; // :304
            iw = niw > 0.4 ? niw : 0.4;
            it += 1;
        }
        swarm_update_gbest_any(rPbf, lane, N, gf, g);
        if (lane < N) {
            for (int d = 0; d < 3; ++d) {
                pos[lane][d] = rPos[d];
                vec[lane][d] = rVec[d];
                pBest[lane][d] = rPb[d];
                nBest[lane][d] = rNb[d];
            }
            fit[lane] = rFit;
            pBestFit[lane] = rPbf;
        }
        __syncthreads();
    } else {
        for (int i = lane; i < N; i += 64) {
            for (int d = 0; d < 3; ++d) {
                pos[i][d] = sload<COH>(&A.pos[i][d]);
                vec[i][d] = sload<COH>(&A.vec[i][d]);
                pBest[i][d] = sload<COH>(&A.pBest[i][d]);
                nBest[i][d] = sload<COH>(&A.nBest[i][d]);
            }
            fit[i] = sload<COH>(&A.fit[i]);
            pBestFit[i] = sload<COH>(&A.pBestFit[i]);
        }
        __syncthreads();
        it = sload<COH>(&hd->iteration);
        g = sload<COH>(&hd->gIdx);
        gf = sload<COH>(&hd->gBestFitness);
        iw = sload<COH>(&hd->iw);
        const int started = sload<COH>(&hd->started);
        if (!started) {
            // initFitness (:112-119) + run(): gBest = particles[0].pBest; updateGbest (:137-149)
            for (int i = lane; i < N; i += 64) pBestFit[i] = fit[i];
            __syncthreads();
            g = 0;
            gf = pBestFit[0];
            for (int j = 0; j < N; ++j)
                if (pBestFit[j] <= gf) { gf = pBestFit[j]; g = j; }
            it = 0;
        } else {
            // updateFitness (:121-135): pBest on strict '<'
            for (int i = lane; i < N; i += 64) {
                if (fit[i] < pBestFit[i]) {
                    pBestFit[i] = fit[i];
                    pBest[i][0] = pos[i][0];
                    pBest[i][1] = pos[i][1];
                    pBest[i][2] = pos[i][2];
                }
            }
            __syncthreads();
            for (int j = 0; j < N; ++j)
                if (pBestFit[j] <= gf) { gf = pBestFit[j]; g = j; }
            const double niw = iw - 1.0 / maxIt; // :304
            iw = niw > 0.4 ? niw : 0.4;
            it += 1;
        }
    }
    // loop head of run(): `iteration < maxIteration`, then the convergence break (:293-297)
    bool finished = it >= maxIt;
    double tDisp = __builtin_nan(""), tVel = __builtin_nan(""); // (the trace's copy of the test's values)
    if (!finished && lanes && !Sink::on) {
        // the two means as k_pso_iter's replay takes them (swarm_mean_below: the decision of the sequential sums)
        const double g0 = lane_get(rPb[0], g), g1 = lane_get(rPb[1], g), g2 = lane_get(rPb[2], g);
        if (swarm_mean_below_any(fabs(rPos[0] - g0), fabs(rPos[1] - g1), fabs(rPos[2] - g2), lane, N))
            finished = swarm_mean_below_any(fabs(rVec[0]), fabs(rVec[1]), fabs(rVec[2]), lane, N);
    } else if (!finished) {
        const double g0 = pBest[g][0], g1 = pBest[g][1], g2 = pBest[g][2];
        double disp = 0;
        for (int i = 0; i < N; ++i) {
            disp += fabs(pos[i][0] - g0);
            disp += fabs(pos[i][1] - g1);
            disp += fabs(pos[i][2] - g2);
        }
        disp /= (double)(3 * N);
        if constexpr (Sink::on) tDisp = disp;
        if (disp < 0.01) {
            double vel = 0;
            for (int i = 0; i < N; ++i) {
                vel += fabs(vec[i][0]);
                vel += fabs(vec[i][1]);
                vel += fabs(vec[i][2]);
            }
            vel /= (double)(3 * N);
            if constexpr (Sink::on) tVel = vel;
            finished = vel < 0.01;
        }
    }
    if constexpr (Sink::on) {
        const int run = hd->run;
        if (run >= 0 && run < sink.maxRuns && it >= 0 && it < sink.rows) {
            const size_t slot = (size_t)c * sink.maxRuns + run;
            if (lane == 0) {
                pais_pso_iter *row = sink.iters + slot * sink.rows + it;
                row->gbest_fitness = gf;
                row->gbest[0] = pBest[g][0];
                row->gbest[1] = pBest[g][1];
                row->gbest[2] = pBest[g][2];
                row->iw = iw;
                row->dispersion = tDisp;
                row->velocity = tVel;
                row->g_idx = g;
                row->iteration = it;
                row->ended = finished ? 1 : 0;
            }
            pais_pso_run_info *ri = sink.runs + slot;
            if (it == 0) {
                if (lane == 0) {
                    for (int d = 0; d < 3; ++d) {
                        ri->range_l[d] = hd->rangeL[d];
                        ri->range_u[d] = hd->rangeU[d];
                        ri->init[d] = hd->init[d];
                        ri->ray[d] = hd->ray[d];
                    }
                    ri->run = run;
                    ri->ref_cam = hd->refCam;
                    ri->lod = hd->LOD;
                    ri->num_cam = hd->K;
                    ri->n_particles = N;
                    ri->max_iteration = maxIt;
                }
                for (int k = lane; k < hd->K && k < PAIS_MAX_VIS; k += 64) ri->cam_idx[k] = hd->camIdx[k];
            }
            if (finished && lane == 0) ri->iterations = it;
            if (sink.particles) {
                double *dst = sink.particles + (slot * sink.rows + it) * (size_t)sink.NP * 11;
                for (int i = lane; i < N && i < sink.NP; i += 64) {
                    double *q = dst + (size_t)i * 11;
                    for (int d = 0; d < 3; ++d) {
                        q[d] = pos[i][d];
                        q[3 + d] = vec[i][d];
                        q[6 + d] = pBest[i][d];
                    }
                    q[9] = fit[i];
                    q[10] = pBestFit[i];
                }
            }
        }
    }
    if (!finished) {
        // moveParticles (:220-265) for iteration `it`
        const double gB[3] = {pBest[g][0], pBest[g][1], pBest[g][2]};
        if (lanes) {
            pso_move_lanes(N, localK, iw, it, sb, (uint32_t)run, pos, vec, pBest, nBest, fit, pBestFit, gB, rl, ru, lane);
        } else {
            const double rangeL[3] = {hd->rangeL[0], hd->rangeL[1], hd->rangeL[2]};
            const double rangeU[3] = {hd->rangeU[0], hd->rangeU[1], hd->rangeU[2]};
            const uint64_t streamBase = hd->streamBase;
            const uint32_t runIdx = (uint32_t)hd->run;
            const int nearK = hd->localK;
            for (int i = lane; i < N; i += 64) {
                double u[4];
                const uint32_t k0 = (uint32_t)(6 * N + 3 + 4 * (it * N + i));
                for (int q = 0; q < 4; ++q) u[q] = uniform_from(streamBase, runIdx, k0 + q);
                pso_move_particle(i, N, nearK, iw, u, pos, vec, pBest, nBest, fit, pBestFit, gB, rangeL, rangeU);
            }
        }
        __syncthreads();
        for (int i = lane; i < N; i += 64) {
            for (int d = 0; d < 3; ++d) {
                sstore<COH>(&A.pos[i][d], pos[i][d]);
                sstore<COH>(&A.vec[i][d], vec[i][d]);
                sstore<COH>(&A.pBest[i][d], pBest[i][d]);
                sstore<COH>(&A.nBest[i][d], nBest[i][d]);
            }
            sstore<COH>(&A.pBestFit[i], pBestFit[i]);
        }
        if (pre) swarm_eval_setup<COH>(sc, preEp, preCams, pos, N, pBestFit + Nmax, pre, preD, lane);
        if (lane == 0) {
            sstore<COH>(&hd->iteration, it);
            sstore<COH>(&hd->gIdx, g);
            sstore<COH>(&hd->gBestFitness, gf);
            sstore<COH>(&hd->iw, iw);
            sstore<COH>(&hd->started, 1);
        }
        return 1;
    } else if (lane == 0) {
        // write back (patch.cpp:208-213) and the maxFitness gate (:156-159)
        pais_patch_result *P = &recs[c];
        const double th = pBest[g][0], ph = pBest[g][1], dp = pBest[g][2];
        double nn[3];
        spherical2normal(th, ph, nn);
        P->fitness = gf;
        P->normalS[0] = th;
        P->normalS[1] = ph;
        for (int q = 0; q < 3; ++q) P->normal[q] = nn[q];
        P->depth = dp;
        const DevCamera &rc = sc.cams[hd->refCam];
        for (int q = 0; q < 3; ++q) P->center[q] = hd->ray[q] * dp + rc.C[q];
        P->pso_runs += 1;
        P->pso_iterations += it;
        const int evals = N * (1 + it);
        P->pso_evals += evals;
        if (gf > sc.cfg.maxFitness) {
            P->dropped = 1;
            P->stage = PAIS_STAGE_DONE;
        } else {
            P->stage = PAIS_STAGE_AFTER;
        }
        hd->active = 0;
        const int K = hd->K;
        const unsigned long long perEval = (unsigned long long)(4 * K + 1 + (sc.cfg.adaptiveDistanceEnable ? 8 : 0) +
                                                                (sc.cfg.adaptiveGradientEnable ? 8 : 0));
        atomicAdd(&stat[0], (unsigned long long)evals);
        atomicAdd(&stat[1], (unsigned long long)evals * perEval);
        atomicAdd(&stat[2], 1ULL);
        atomicAdd(&stat[5], (unsigned long long)evals); // ... of which by the large-batch pipeline (k_pso_eval2 / k_pso_ring)
        atomicAdd(&stat[6], (unsigned long long)evals * perEval);
        if (COH) { // ... of which inside a k_pso_ring launch
            atomicAdd(&stat[22], (unsigned long long)evals);
            atomicAdd(&stat[23], (unsigned long long)evals * perEval);
        }
    }
    return 0;
}
// N: hd->N, which every caller has at hand before the step (it selects the form)
template <bool COH = false, class Sink = StepNoSink>
__device__ int pso_step_wave(const DevScene &sc, pais_patch_result *recs, int c, PsoState *hd, int N, int Nmax,
                             unsigned char *smem, unsigned long long *stat, int lane, const EvalPatch *preEp = nullptr,
                             const EvalCam *preCams = nullptr, double *pre = nullptr, size_t preD = 0, const Sink &sink = Sink())
{
    if (N <= 64) return pso_step_body<COH, Sink, true>(sc, recs, c, hd, N, Nmax, smem, stat, lane, preEp, preCams, pre, preD, sink);
    return pso_step_body<COH, Sink, false>(sc, recs, c, hd, N, Nmax, smem, stat, lane, preEp, preCams, pre, preD, sink);
}
// the step as k_pso_ring calls it, inlined (a real call was measured slower: profiles/r04_ring_step_call_ab.txt)
template <bool PARTS>
__device__ int pso_step_wave_ring(const DevScene &sc, pais_patch_result *recs, int c, PsoState *hd, int N, int Nmax, unsigned char *smem,
                                  unsigned long long *stat, int lane, const EvalPatch *preEp, const EvalCam *preCams, double *pre, size_t preD)
{
    // (a ring pass has Nmax <= 64 -- a candidate's tasks are published by the lanes of one wave: the lane-parallel form alone)
    return pso_step_body<true, StepNoSink, true, PARTS>(sc, recs, c, hd, N, Nmax, smem, stat, lane, preEp, preCams, pre, preD, StepNoSink());
}
// the step kernel of large batches: one wave per candidate
// pre != nullptr: the step also writes the evaluation records of the moved swarm (pais_pre.hpp) from the candidate's evaluation
// block, which it stages in front of its scratch
__global__ __launch_bounds__(64, 4) void k_pso_step(DevScene sc, pais_patch_result *recs, unsigned char *states, int n,
                                                 int Nmax, unsigned long long *stat, const unsigned char *evalBlocks, size_t evalBlockBytes,
                                                 double *pre, int Kmax)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem0[];
    unsigned char *smem = smem0 + (pre ? evalBlockBytes : 0);
    const size_t preD = pre_rec_doubles(Kmax);
    const int nwMax = (int)(evalBlockBytes / 8);
    // the step of one slice runs while the other slice's evaluation launch fills the GPU; its few waves sit on the
    // critical path of their own slice (next evaluation launch), so they take issue priority over the evaluation waves
    __builtin_amdgcn_s_setprio(3);
    const int lane = threadIdx.x;
    const size_t SB = pso_state_bytes(Nmax);
    for (int c = blockIdx.x; c < n; c += gridDim.x) {
        PsoState *hd = (PsoState *)(states + SB * (size_t)c);
        const int active = hd->active, N = __builtin_amdgcn_readfirstlane(hd->N); // (one round trip)
        if (!active) continue;
        if (pre) {
            const uint64_t *src = (const uint64_t *)(evalBlocks + evalBlockBytes * (size_t)c);
            wave_sync();
            stage_eval_block(smem0, src, nwMax, lane, lane < nwMax ? src[lane] : 0, lane + 64 < nwMax ? src[lane + 64] : 0);
            wave_sync();
        }
        pso_step_wave(sc, recs, c, hd, N, Nmax, smem, stat, lane, (const EvalPatch *)smem0, (const EvalCam *)(smem0 + sizeof(EvalPatch)),
                      pre ? pre + preD * (size_t)Nmax * (size_t)c : nullptr, preD);
    }
}

// pais_pso_trace: k_pso_step's loop with the trace sink and without the `pre` records (one slice: c is the batch index)
__global__ __launch_bounds__(64, 4) void k_pso_step_trace(DevScene sc, pais_patch_result *recs, unsigned char *states, int n, int Nmax,
                                                       unsigned long long *stat, StepTraceSink sink)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem0[];
    __builtin_amdgcn_s_setprio(3);
    const int lane = threadIdx.x;
    const size_t SB = pso_state_bytes(Nmax);
    for (int c = blockIdx.x; c < n; c += gridDim.x) {
        PsoState *hd = (PsoState *)(states + SB * (size_t)c);
        const int active = hd->active, N = __builtin_amdgcn_readfirstlane(hd->N); // (one round trip)
        if (!active) continue;
        pso_step_wave<false, StepTraceSink>(sc, recs, c, hd, N, Nmax, smem0, stat, lane, nullptr, nullptr, nullptr, 0, sink);
    }
}

// the records of the INITIAL swarm (k_begin / k_pso_init wrote the positions and the evaluation block): one wave per candidate
__global__ __launch_bounds__(64) void k_pso_setup0(DevScene sc, unsigned char *states, int n, int Nmax, const unsigned char *evalBlocks,
                                                   size_t evalBlockBytes, double *pre, int Kmax)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem0[];
    double(*pos)[3] = (double(*)[3])(smem0 + evalBlockBytes);
    double *scr = (double *)(pos + Nmax);
    const int lane = threadIdx.x;
    const size_t SB = pso_state_bytes(Nmax);
    const size_t preD = pre_rec_doubles(Kmax);
    const int nwMax = (int)(evalBlockBytes / 8);
    for (int c = blockIdx.x; c < n; c += gridDim.x) {
        PsoState *hd = (PsoState *)(states + SB * (size_t)c);
        if (!hd->active) continue;
        PsoArrays A = pso_arrays((unsigned char *)hd, Nmax);
        const int N = hd->N;
        const uint64_t *src = (const uint64_t *)(evalBlocks + evalBlockBytes * (size_t)c);
        wave_sync();
        stage_eval_block(smem0, src, nwMax, lane, lane < nwMax ? src[lane] : 0, lane + 64 < nwMax ? src[lane + 64] : 0);
        for (int i = lane; i < N; i += 64)
            for (int d = 0; d < 3; ++d) pos[i][d] = A.pos[i][d];
        wave_sync();
        swarm_eval_setup<false>(sc, (const EvalPatch *)smem0, (const EvalCam *)(smem0 + sizeof(EvalPatch)), pos, N, scr,
                                pre + preD * (size_t)Nmax * (size_t)c, preD, lane);
    }
}

// ---------------------------------------------------------------- k_pso_ring ---
// A PSO pass of a large batch WITHOUT per-iteration launches.  Iteration i + 1 of a candidate depends on that candidate's N
// evaluations of iteration i and on nothing else, so the pass is a pool of tasks -- (candidate, particle): evaluate the
// particle where it stands -- on a ring in global memory, worked off by a fixed set of resident waves:
//   * a wave takes the next ring index (one atomic), waits until that entry is published, evaluates, stores the fitness
//     and counts itself in at the candidate (one atomic);
//   * the wave that completes a candidate's count runs the candidate's swarm step (pso_step_wave: the code of k_pso_step)
//     and publishes the N tasks of the next iteration at the ring's tail -- or the result, if the run has ended.
// Nobody waits for a particular wave: an index beyond the published tail is only ever held by a wave that would otherwise be
// idle, and the tasks whose completion will publish it are being executed by waves that are not waiting -- no deadlock, with
// any number of resident waves.  The swarm state crosses waves (and XCDs) through sc1 loads / stores (cload / cstore above);
// a payload is complete (s_waitcnt vmcnt(0)) before the atomic that lets another wave look at it.  Every wait is bounded in
// WALL TIME (s_memrealtime, the 100 MHz constant counter: a poll count would depend on the clock, a profiler's serialisation
// or a neighbour on a shared GPU): a wave that has waited `timeoutTicks` raises the error word and leaves; the host then
// re-runs the batch through the per-iteration launches (pais_capi.hip ring_fallback) -- the records are the same.
// Same evaluation code, same step code, per-candidate order of operations unchanged: the records are those of
// k_pso_eval2 + k_pso_step bit for bit.
#define PAIS_RING_EMPTY 0xFFFFFFFFu
// A workgroup is ONE wave: the swarm step (pso_step_wave) synchronises with workgroup barriers inside wave-divergent control
// flow, which is only a wave barrier while a workgroup is one wave.
// PAIS_RINGS (pais_internal.h): a multiple of 8 -- workgroup b runs on XCD b % 8 and works ring b % PAIS_RINGS, so a ring's
// counters and its candidates' state stay in one XCD's L2
// two 64-byte lines per ring: the head counter (one atomic per task, from every wave) alone on the first; what publishers and
// idle waves touch (tail, done, error) on the second -- polling waves do not pull the line the poppers serialise on
// a task word: candidate | part of the evaluation (0 while one wave evaluates alone) | particle (Nmax <= 64)
__host__ __device__ inline unsigned ring_task(int c, int part, int particle) { return ((unsigned)c << 8) | ((unsigned)part << 6) | (unsigned)particle; }
struct RingCtl { unsigned head, pad0[15]; unsigned tail, done, total, error, pad1[12]; };
static_assert(sizeof(RingCtl) == PAIS_RING_CTL_BYTES, "RingCtl layout (pais_internal.h)");

// candidates c with c % PAIS_RINGS == r belong to ring r; its segment of the ring memory starts at r * segWords
// tasks of iteration 0 (the initial swarm); candidates whose refinement ended in k_begin count as done
// parts: waves per evaluation (1, 2, 4) -- a task is (candidate, part, particle)
__global__ __launch_bounds__(256) void k_ring_init(unsigned char *states, int n, int Nmax, unsigned *ring, unsigned segWords, RingCtl *ctl, int parts)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n) return;
    RingCtl *rc = &ctl[c % PAIS_RINGS];
    atomicAdd(&rc->total, 1u);
    const PsoState *hd = (const PsoState *)(states + pso_state_bytes(Nmax) * (size_t)c);
    if (!hd->active) {
        atomicAdd(&rc->done, 1u);
        return;
    }
    const int N = hd->N;
    const unsigned base = atomicAdd(&rc->tail, (unsigned)(N * parts));
    unsigned *seg = ring + (size_t)(c % PAIS_RINGS) * segWords;
    for (int j = 0; j < N * parts; ++j) seg[base + j] = ring_task(c, j / N, j % N);
}

// MEASUREMENT BUILDS ONLY (-DPAIS_RING_PROFILE=1, profiles/r06_ring_group_ab.txt): where a ring wave's time goes -- s_memtime at the phase
// boundaries of every task, summed over all waves: [0] index (head atomic) [1] entry wait [2] loads + staging [3] evaluation
// [4] fitness store + arrival [5] swarm step + publish [6] tasks [7] steps; printed when a context is destroyed
#ifndef PAIS_RING_PROFILE
#define PAIS_RING_PROFILE 0
#endif
#if PAIS_RING_PROFILE
__device__ unsigned long long g_ringProf[8];
#define PAIS_RP_MARK(v) const unsigned long long v = __builtin_amdgcn_s_memtime();
#else
#define PAIS_RP_MARK(v)
#endif
// P (1, 2, 4): waves per evaluation.  A task is then a PART of an evaluation (eval_window's part / nparts: the 64-pixel steps
// part, part + P, ...): a candidate's front is N * P tasks and a link of its chain a P-th of a window walk.  A part wave stores
// its sub-accumulators as k_pso_iter<P> does and counts in; the wave that completes the N * P arrivals runs the step, which adds
// the parts in the canonical order (pso_step_body PARTS).  P = 1 is the kernel it always was.
template <int NS, bool BYTES, bool ACCR, bool PRE, int P = 1>
__global__ PAIS_EVAL_BOUNDS(NS) void k_pso_ring(DevScene sc, pais_patch_result *recs, unsigned char *states, int n, int Nmax, int Kmax,
                                                const unsigned char *evalBlocks, size_t evalBlockBytes, const WinPix *win, unsigned *ringAll,
                                                unsigned segWords, RingCtl *ctlAll, int *arrive, unsigned long long *stat, size_t ldsPerWave,
                                                unsigned long long timeoutTicks, double *pre)
{
    const size_t preD = pre_rec_doubles(Kmax);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem0[];
    unsigned char *smem = smem0 + (threadIdx.x >> 6) * ldsPerWave; // wave-private scratch (evaluation; the step reuses it)
    EvalPatch *ep = (EvalPatch *)smem;
    EvalCam *cams = (EvalCam *)(smem + sizeof(EvalPatch));
    double *Hbuf = (double *)(smem + eval_block_bytes(Kmax));
    double *cbuf = Hbuf + Kmax * PAIS_H_STRIDE;
    const int lane = threadIdx.x & 63;
    const size_t SB = pso_state_bytes(Nmax);
    const int WS = win_stride(sc);
    const int nwMax = (int)(eval_block_bytes(Kmax) / 8);
    const int myRing = (int)(blockIdx.x % PAIS_RINGS);
    RingCtl *ctl = &ctlAll[myRing];
    unsigned *ring = ringAll + (size_t)myRing * segWords;
    const unsigned cap = segWords;
    const unsigned total = ctl->total; // (written by k_ring_init, before this launch)
    for (;;) {
        PAIS_RP_MARK(rpA)
        unsigned idx = 0;
        if (lane == 0) idx = __hip_atomic_fetch_add(&ctl->head, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        idx = (unsigned)__builtin_amdgcn_readfirstlane((int)idx);
        if (idx >= cap) break;
        PAIS_RP_MARK(rpB)
        unsigned e = PAIS_RING_EMPTY;
        unsigned long long t0 = 0;
        for (int spins = 0;; ++spins) {
            e = rload(&ring[idx]);
            if (e != PAIS_RING_EMPTY) break;
            if ((spins & 7) == 7) { // (the shared words are looked at now and then: thousands of idle waves poll)
                if (rload(&ctl->done) >= total) break; // every run of this ring has ended
                if (rload(&ctl->error) != 0) break;
                const unsigned long long now = __builtin_amdgcn_s_memrealtime();
                if (spins == 7) t0 = now;
                if (now - t0 >= timeoutTicks) { // nobody has published this entry for `timeoutTicks` of wall time
                    if (lane == 0) rstore(&ctl->error, 1u);
                    break;
                }
            }
            __builtin_amdgcn_s_sleep(32);
        }
        e = (unsigned)__builtin_amdgcn_readfirstlane((int)e);
        if (e == PAIS_RING_EMPTY) break;
        PAIS_RP_MARK(rpC)
        const int c = (int)(e >> 8), i = (int)(e & (P == 1 ? 255u : 63u)), part = P == 1 ? 0 : (int)((e >> 6) & 3u);
        PsoState *hd = (PsoState *)(states + SB * (size_t)c);
        PsoArrays A = pso_arrays((unsigned char *)hd, Nmax);
        const uint64_t *src = (const uint64_t *)(evalBlocks + evalBlockBytes * (size_t)c);
        // pre: the particle's record {status, homographies} written by the swarm step / k_pso_setup0 (pais_pre.hpp) instead of its position
        double *crec = PRE ? pre + preD * (size_t)Nmax * (size_t)c : nullptr;
        const double *rec = PRE ? crec + preD * (size_t)i : nullptr;
        double p0 = 0, p1 = 0, p2 = 0, status0 = 0, hv = 0;
        if (PRE) {
            status0 = cload(&rec[0]);
            hv = lane < PAIS_H_STRIDE * Kmax ? cload(&rec[PAIS_PRE_HDR + lane]) : 0.0;
        } else {
            p0 = cload(&A.pos[i][0]); p1 = cload(&A.pos[i][1]); p2 = cload(&A.pos[i][2]);
        }
        const uint64_t v0 = lane < nwMax ? src[lane] : 0, v1 = lane + 64 < nwMax ? src[lane + 64] : 0;
        const int N = hd->N; // (written by k_begin, before this launch)
        wave_sync();
        stage_eval_block(smem, src, nwMax, lane, v0, v1);
        wave_sync();
#if PAIS_RING_PROFILE
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
        PAIS_RP_MARK(rpD)
        double f4[4], w4[4];
        int st;
        if (PRE) st = eval_fitness_pre<NS, BYTES, ACCR, true, P>(sc, ep, cams, Hbuf, cbuf, win + (size_t)c * WS, rec, status0, hv, lane, f4, w4, part);
        else st = eval_fitness_parts<NS, BYTES, ACCR>(sc, ep, cams, Hbuf, cbuf, win + (size_t)c * WS, p0, p1, p2, lane, part, P, f4, w4);
        int old = 0;
        PAIS_RP_MARK(rpE)
        if (lane == 0) {
            if (P == 1) {
                cstore(&A.fit[i], st ? DBL_MAX : combine_parts(f4, w4));
            } else { // (a call that is DBL_MAX: weight -1, as k_pso_iter says it)
                for (int a = part; a < 4; a += P) {
                    cstore(&A.part[i][2 * a], st ? 0.0 : f4[a]);
                    cstore(&A.part[i][2 * a + 1], st ? -1.0 : w4[a]);
                }
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the fitness is at the coherence point before it is counted
            old = __hip_atomic_fetch_add(&arrive[(size_t)c * PAIS_ARRIVE_STRIDE], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        old = __builtin_amdgcn_readfirstlane(old);
#if PAIS_RING_PROFILE
        {
            const unsigned long long rpF = __builtin_amdgcn_s_memtime();
            if (lane == 0) {
                atomicAdd(&g_ringProf[0], rpB - rpA); atomicAdd(&g_ringProf[1], rpC - rpB); atomicAdd(&g_ringProf[2], rpD - rpC);
                atomicAdd(&g_ringProf[3], rpE - rpD); atomicAdd(&g_ringProf[4], rpF - rpE); atomicAdd(&g_ringProf[6], 1ULL);
            }
        }
        PAIS_RP_MARK(rpG)
#endif
        if (old != N * P - 1) continue;
        // this wave completed the candidate's iteration: its swarm step, then the next iteration's tasks (or the result)
        __builtin_amdgcn_s_setprio(3); // the step sits on the candidate's critical path
        if (lane == 0) cstore(&arrive[(size_t)c * PAIS_ARRIVE_STRIDE], 0);
        wave_sync();
        // (with records: the step's scratch lies behind the evaluation block, which swarm_eval_setup reads -- this wave has just
        //  evaluated a particle of candidate c, so the block in its LDS is c's)
        const int cont = pso_step_wave_ring<(P > 1)>(sc, recs, c, hd, __builtin_amdgcn_readfirstlane(N), Nmax, smem + (PRE ? eval_block_bytes(Kmax) : 0), stat, lane, ep, cams, crec, preD);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // every lane's part of the new swarm (and the counter reset) is out
        wave_sync();
        if (__builtin_amdgcn_readfirstlane(cont)) {
            unsigned base = 0;
            if (lane == 0) base = __hip_atomic_fetch_add(&ctl->tail, (unsigned)(N * P), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            base = (unsigned)__builtin_amdgcn_readfirstlane((int)base);
            if (base + (unsigned)(N * P) > cap) { // cannot happen (a segment holds every task of its candidates); never write past it
                if (lane == 0) rstore(&ctl->error, 2u);
                break;
            }
            if (P == 1) {
                if (lane < N) rstore(&ring[base + lane], ((unsigned)c << 8) | (unsigned)lane);
            } else { // N * P <= 256 entries, part by part: a lane publishes up to four
                for (int t = lane; t < N * P; t += 64) rstore(&ring[base + t], ring_task(c, t / N, t % N));
            }
        } else if (lane == 0) {
            __hip_atomic_fetch_add(&ctl->done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __builtin_amdgcn_s_setprio(0);
#if PAIS_RING_PROFILE
        {
            const unsigned long long rpH = __builtin_amdgcn_s_memtime();
            if (lane == 0) { atomicAdd(&g_ringProf[5], rpH - rpG); atomicAdd(&g_ringProf[7], 1ULL); }
        }
#endif
    }
}

// ---------------------------------------------------------------- k_after ---
// After one PSO run: patch.cpp:161-175 (+ the caller's removeInvisibleCamera, mvs.cpp:215 / :574, once the refine loop
// has ended).  Four launches:
//   k_region_ratio(AFTER)   region ratio of every (candidate, visible camera): ONE LANE each -- three small Jacobi SVDs
//                           (cv::fitEllipse) are a long serial chain, so they are packed 64 to a wave across candidates
//                           instead of occupying K lanes of a candidate's wave
//   k_after<1>              first removeInvisibleCamera, setters, seed-loop control, priority + image points
//   k_region_ratio(AFTER2)  the same for the state after the setters (other reference camera / LOD / camera set)
//   k_after<2>              the trailing removeInvisibleCamera
__global__ __launch_bounds__(64) void k_region_ratio(DevScene sc, const pais_patch_result *recs, int n, int stage, double *ratios, int Kmax)
{
    const int t = blockIdx.x * 64 + threadIdx.x;
    const int c = t / Kmax, k = t - c * Kmax; // Kmax = the batch's largest camera count: (nearly) every lane has a camera
    if (c >= n) return;
    const pais_patch_result *P = &recs[c];
    if (P->stage != stage || P->dropped || k >= P->num_cam) return;
    const int LOD = P->lod, refCam = P->ref_cam;
    const DevCamera &rc = sc.cams[refCam];
    const double s = sc.lodScale[LOD];
    const double center[3] = {P->center[0], P->center[1], P->center[2]};
    const double nrm[3] = {P->normal[0], P->normal[1], P->normal[2]};
    const int ci = P->cam_idx[k];
    const double d = -dot3(center, nrm);
    double invH[9], H[9];
    ref_plane_inverse(d, s, rc.KR, rc.KT, nrm, invH);
    patch_homography(ci == refCam, d, s, sc.cams[ci].KR, sc.cams[ci].KT, nrm, invH, H);
    double pt[2];
    cam_project(sc, refCam, center, pt, LOD);
    ratios[(size_t)c * PAIS_MAX_VIS + k] = region_ratio(pt[0], pt[1], sc.cfg.patchRadius, H);
}

template <int PHASE>
__global__ __launch_bounds__(64 * AFTER_WAVES) void k_after(DevScene sc, pais_patch_result *recs, int n, double *hpScratch,
                                                              int *counters, unsigned long long *stat, int Kmax, double *ratios,
                                                              int hpInLds, int *nextCounters)
{
    // the counters the NEXT pass (of this or the next batch) will add to; nothing of this pass touches that set
    if (PHASE == 2 && nextCounters && blockIdx.x == 0 && threadIdx.x == 0) {
        nextCounters[0] = 0;
        nextCounters[1] = 0;
        nextCounters[2] = 0;
    }
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    pais_patch_result *st = (pais_patch_result *)smem;
    size_t off = (sizeof(pais_patch_result) + 15) & ~(size_t)15;
    double *table = (double *)(smem + off); off += sizeof(double) * Kmax * Kmax;
    double *Hn = (double *)(smem + off); off += sizeof(double) * 9 * Kmax;
    int *flag = (int *)(smem + off); off += 16;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool lead = threadIdx.x == 0;
    const int S2 = sc.cfg.patchSize * sc.cfg.patchSize;
    // the warped patches (Kmax x S2 doubles, written once, read K times): LDS while they fit, else a global scratch slab
    double *hp = hpInLds ? (double *)(smem + off) : hpScratch + (size_t)blockIdx.x * Kmax * S2;
    for (int c = blockIdx.x; c < n; c += gridDim.x) {
        const int stg = recs[c].stage;
        if (PHASE == 1 ? (stg != PAIS_STAGE_AFTER) : (stg != PAIS_STAGE_AFTER2 && stg != PAIS_STAGE_AFTER2_KEEP && stg != PAIS_STAGE_AFTER2_SAME))
            continue;
        __syncthreads();
        copy_record(st, &recs[c], threadIdx.x, 64 * AFTER_WAVES);
        __syncthreads();

        const int nccBefore = st->ncc_tables;
        double *rat = ratios + (size_t)c * PAIS_MAX_VIS;
        if (PHASE == 1) {
            const int refBefore = st->ref_cam, lodBefore = st->lod, numBefore = st->num_cam;
            remove_invisible_camera(sc, st, hp, table, Hn, flag, rat, lane, wave);
            const bool removedNone = st->num_cam == numBefore; // (read behind the call's closing barrier, by every thread alike)
            set_reference_camera(sc, st, lane);
            set_depth_and_ray(sc, st, lane);
            set_depth_range(sc, st, lane);
            set_lod(sc, st, lane);

            bool again = false;
            if (st->type != PAIS_TYPE_EXPAND && !st->dropped) {
                // patch.cpp:170-171 then the while condition of :140
                const int afterRef = st->ref_cam, afterNum = st->num_cam;
                const int cnt = st->count;
                const bool cond = (st->before_ref != afterRef || st->before_num != afterNum) && (cnt <= st->total_cam_num);
                __syncthreads();
                if (lead) {
                    st->after_ref = afterRef;
                    st->after_num = afterNum;
                    st->count = cnt + 1; // count++ is evaluated whenever the first operand is true ... (see note)
                }
                __syncthreads();
                if (cond) {
                    if (st->num_cam < sc.cfg.minCamNum) { // :142-147
                        __syncthreads();
                        if (lead) {
                            st->fitness = DBL_MAX;
                            st->priority = DBL_MAX;
                            st->dropped = 1;
                        }
                        __syncthreads();
                    } else {
                        again = true;
                        __syncthreads();
                        if (lead) {
                            st->before_ref = st->ref_cam;
                            st->before_num = st->num_cam;
                            st->stage = PAIS_STAGE_PSO;
                        }
                        __syncthreads();
                    }
                }
            }
            if (!again) {
                set_priority_and_image_point(sc, st, lane);
                __syncthreads();
                // mvs.cpp:215 / :574 follows.  Centre and normal are those of the first call; with the same reference camera
                // and LOD the homographies -- and so the region ratios of the cameras that stayed -- are too
                if (lead)
                    st->stage = st->dropped ? PAIS_STAGE_DONE
                                            : ((st->ref_cam == refBefore && st->lod == lodBefore)
                                                   ? (removedNone ? PAIS_STAGE_AFTER2_SAME : PAIS_STAGE_AFTER2_KEEP)
                                                   : PAIS_STAGE_AFTER2);
            }
            __syncthreads();
            if (lead && again) atomicAdd(&counters[1], 1);
        } else {
            // mvs.cpp:215 / :574.  PAIS_STAGE_AFTER2_SAME: the first call removed nothing and the setters left the reference
            // camera and the LOD alone, so this call would warp the same patches of the same cameras with the same
            // homographies, build the same table and again remove nothing -- only its call count is carried
            if (stg == PAIS_STAGE_AFTER2_SAME) {
                if (lead) st->ncc_tables += 1;
            } else {
                remove_invisible_camera(sc, st, hp, table, Hn, flag, rat, lane, wave);
            }
            __syncthreads();
            // the scene half of MVS::runtimeFiltering (mvs.cpp:851-863) for the caller's insertPatch: one thread per camera
            int finalStage = PAIS_DONE;
            if (!st->dropped) {
                bool off = false;
                const double X[3] = {st->center[0], st->center[1], st->center[2]};
                for (int i = threadIdx.x; i < sc.numCams; i += 64 * AFTER_WAVES) {
                    const DevCamera &cam = sc.cams[i];
                    double pt[2];
                    project_raw(cam.R, cam.T, cam.focal, cam.pp, 1.0, X, pt);
                    if (!in_image_d(pt, cam.w[0], cam.h[0])) {
                        off = true;
                    } else {
                        // (the reference reads at(cvRound(y), cvRound(x)); defined as the edge pixel within half a pixel of the
                        // right / bottom edge, as in the host statement)
                        const int rx = min(cv_round(pt[0]), cam.w[0] - 1), ry = min(cv_round(pt[1]), cam.h[0] - 1);
                        if (sc.imgBlob[cam.imgOff[0] + (size_t)ry * cam.w[0] + rx] == 0) off = true;
                    }
                }
                finalStage = __syncthreads_or(off ? 1 : 0) ? PAIS_DONE_OFF_SCENE : PAIS_DONE_IN_SCENE;
            }
            if (lead) st->stage = finalStage;
        }
        __syncthreads();
        if (lead) {
            atomicAdd(&stat[3], (unsigned long long)(st->ncc_tables - nccBefore));
            atomicAdd(&stat[4], (unsigned long long)(st->ncc_tables - nccBefore) * (unsigned long long)st->total_cam_num);
        }
        __syncthreads();
        copy_record(&recs[c], st, threadIdx.x, 64 * AFTER_WAVES);
    }
}

// ------------------------------------------------------------ k_ncc_batch ---
// pais_ncc_batch: Patch::removeInvisibleCamera (patch.cpp:655-721) of caller-given states, every intermediate written to a
// pais_view_result.  One workgroup of AFTER_WAVES waves per state (grid-stride over the batch) calls the pieces that
// remove_invisible_camera calls: view_homographies by wave 0 into LDS; view_warp_patches into LDS or this workgroup's
// slab of hpScratch; view_fill_table; the region ratios one lane per camera of the last wave (region_ratio, no separate
// k_region_ratio launch); correlation, best camera, verdicts and the kept list by thread 0 in the sequential order of the
// after-stage.  The result record is assembled in LDS (zero-filled first) and stored whole, so its bytes depend on the
// state alone, not on the batch.
__global__ __launch_bounds__(64 * AFTER_WAVES) void k_ncc_batch(DevScene sc, const pais_view_state *states, int n,
                                                                  pais_view_result *out, double *tables, int stride,
                                                                  double *hpScratch, int Kmax, int hpInLds)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    pais_view_result *res = (pais_view_result *)smem;
    size_t off = (sizeof(pais_view_result) + 15) & ~(size_t)15;
    double *table = (double *)(smem + off); off += sizeof(double) * Kmax * Kmax;
    double *Hn = (double *)(smem + off); off += sizeof(double) * 9 * Kmax;
    int *flag = (int *)(smem + off); off += 16;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = sc.cfg.patchRadius, S = sc.cfg.patchSize, S2 = S * S;
    double *hp = hpInLds ? (double *)(smem + off) : hpScratch + (size_t)blockIdx.x * Kmax * S2;
    for (int s = blockIdx.x; s < n; s += gridDim.x) {
        const pais_view_state *V = &states[s];
        const int K = V->num_cam, LOD = V->lod, refCam = V->ref_cam;
        const double center[3] = {V->center[0], V->center[1], V->center[2]};
        const double nrm[3] = {V->normal[0], V->normal[1], V->normal[2]};
        __syncthreads(); // the previous state's LDS is no longer read
        {
            uint32_t *w = (uint32_t *)res;
            for (int i = tid; i < (int)(sizeof(pais_view_result) / 4); i += 64 * AFTER_WAVES) w[i] = 0;
        }
        for (int i = tid; i < K * K; i += 64 * AFTER_WAVES) table[i] = 0;
        if (tid == 0) *flag = 0;
        if (wave == 0) view_homographies(sc, refCam, sc.lodScale[LOD], V->cam_idx, K, center, nrm, Hn, lane);
        __syncthreads();

        double pt[2];
        cam_project(sc, refCam, center, pt, LOD);
        // getHomographyRegionRatio: one lane per camera (three small Jacobi SVDs, a serial chain)
        if (wave == AFTER_WAVES - 1)
            for (int c = lane; c < K; c += 64) res->region_ratio[c] = region_ratio(pt[0], pt[1], r, Hn + 9 * c);

        view_warp_patches(sc, V->cam_idx, K, LOD, Hn, pt[0] - r, pt[1] - r, hp, flag, lane, wave);
        __syncthreads();
        const bool dropSample = *flag != 0;
        if (!dropSample) view_fill_table(hp, K, S2, table, lane, wave);
        __syncthreads();
        if (tid == 0) {
            if (dropSample) {
                res->dropped = PAIS_VIEW_DROP_SAMPLE; // correlation = 0; table, reasons and kept list stay 0
            } else {
                // (the reduction and the verdicts of view_correlation / view_max_idx / view_verdict, written out: called as functions, in
                //  any of four shapes measured, they make this thread-0 tail 0.5 % of the whole kernel slower at five cameras)
                double correlation = 0;
                for (int i = 0; i < K; ++i)
                    for (int j = 0; j < K; ++j) correlation += table[i * K + j];
                correlation /= (double)(K * K - K);
                double maxCorr = -DBL_MAX;
                int maxIdx = 0;
                for (int i = 0; i < K; ++i) {
                    double corrSum = 0;
                    for (int j = 0; j < K; ++j) corrSum += table[i * K + j];
                    if (corrSum >= maxCorr) { // last max wins
                        maxIdx = i;
                        maxCorr = corrSum;
                    }
                }
                int nn = 0;
                for (int i = 0; i < K; ++i) {
                    const int ci = V->cam_idx[i];
                    const DevCamera &cam = sc.cams[ci];
                    const double dd = nrm[0] * (-cam.optN[0]) + nrm[1] * (-cam.optN[1]) + nrm[2] * (-cam.optN[2]);
                    int why = PAIS_VIEW_KEEP;
                    if (res->region_ratio[i] < sc.cfg.minRegionRatio) why = PAIS_VIEW_REGION;
                    else if (dd < 0) why = PAIS_VIEW_BACKFACING;
                    else if (i != maxIdx && table[maxIdx * K + i] < sc.cfg.minCorrelation) why = PAIS_VIEW_CORRELATION;
                    res->reason[i] = why;
                    if (why == PAIS_VIEW_KEEP) res->kept_idx[nn++] = ci;
                }
                res->correlation = correlation;
                res->max_idx = maxIdx;
                res->num_kept = nn;
                res->dropped = nn < sc.cfg.minCamNum ? PAIS_VIEW_DROP_MINCAM : 0;
            }
        }
        if (tables) {
            double *T = tables + (size_t)s * stride * stride;
            for (int i = tid; i < stride * stride; i += 64 * AFTER_WAVES) {
                const int a = i / stride, b = i - a * stride;
                T[i] = (a < K && b < K) ? table[a * K + b] : 0.0;
            }
        }
        __syncthreads();
        {
            const uint32_t *src = (const uint32_t *)res;
            uint32_t *dst = (uint32_t *)&out[s];
            for (int i = tid; i < (int)(sizeof(pais_view_result) / 4); i += 64 * AFTER_WAVES) dst[i] = src[i];
        }
    }
}

// ------------------------------------------------------------ record wire ---
// include/pais_hip.h "wire format of a record": one thread per 4-byte word of a slot; the layout below is the one
// pais_pack_records / pais_unpack_records (pais_capi.hip) state on the host
__global__ __launch_bounds__(256) void k_pack_records(const pais_patch_result *recs, int n, int Kw, uint32_t *wire)
{
    const int wordsPerSlot = 52 + 5 * Kw; // 208 / 4 + Kw * (16 + 4) / 4
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < (size_t)n * wordsPerSlot; t += (size_t)gridDim.x * 256) {
        const int r = (int)(t / wordsPerSlot), w = (int)(t - (size_t)r * wordsPerSlot);
        const uint32_t *src = (const uint32_t *)&recs[r];
        // record words: [0,34) the 17 doubles; [34,290) imgPoint; [290,292) key; [292,300) type..pso_evals; [300,364) cam_idx;
        // [364,372) stage..ncc_tables
        int sw;
        if (w < 34) sw = w;
        else if (w < 36) sw = 290 + (w - 34);
        else if (w < 44) sw = 292 + (w - 36);
        else if (w < 52) sw = 364 + (w - 44);
        else if (w < 52 + 4 * Kw) sw = 34 + (w - 52);
        else sw = 300 + (w - 52 - 4 * Kw);
        wire[t] = src[sw];
    }
}

// ------------------------------------------------------- scene preparation ---
// float2 tap copy of the byte blob (pais_internal.h PaisImgT): one thread per pixel, coalesced
// header of a rank's block in a sharded batch's exchange (include/pais_hip.h pais_wire_header): the ring's own words decide
// whether the pass completed, so that the status travels with the records without a host round trip before the collective
__global__ __launch_bounds__(64) void k_wire_header(uint32_t *hdr, const RingCtl *ctl, int ringN, int rank, int count, int hostRc, uint32_t userWord)
{
    if (threadIdx.x >= 16) return;
    int rc = hostRc;
    if (rc == 0 && ctl) {
        unsigned done = 0, err = 0;
        for (int r = 0; r < PAIS_RINGS; ++r) { done += ctl[r].done; err |= ctl[r].error; }
        if (err != 0 || done != (unsigned)ringN) rc = PAIS_WIRE_RC_RING_RETRY;
    }
    const uint32_t w[4] = {PAIS_WIRE_MAGIC, (uint32_t)rc, (uint32_t)count, (uint32_t)rank};
    hdr[threadIdx.x] = threadIdx.x < 4 ? w[threadIdx.x] : (threadIdx.x == 4 ? userWord : 0u);
}

__global__ __launch_bounds__(256) void k_expand_image(const uint8_t *img, PaisImgT *out, size_t n)
{
    // grid-stride: a blob of several GB has more pixels than one launch may have threads (2^32)
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int a = img[i], b = (i + 1 < n) ? img[i + 1] : 0; // the last column's difference is never tapped
        PaisImgT v;
        v.x = a;
        v.y = b - a;
        out[i] = v;
    }
}
// minimum / maximum Sobel magnitude of one level (the statements of k_sobel_mag in pais_pyramid.hip without the map):
// magnitudes are >= 0, so their bit patterns order like the values; one atomic pair per workgroup
__global__ __launch_bounds__(256) void k_level_edge_minmax(const uint8_t *img, int w, int h, unsigned long long *minmax)
{
    __shared__ unsigned long long red[8];
    const int x = blockIdx.x * 256 + threadIdx.x;
    unsigned long long lo = ~0ULL, hi = 0ULL;
    if (x < w) {
        const int xl = x > 0 ? x - 1 : (w > 1 ? 1 : 0), xr = x < w - 1 ? x + 1 : (w > 1 ? w - 2 : 0);
        for (int r = 0; r < 16; ++r) {
            const int y = blockIdx.y * 16 + r;
            if (y >= h) break;
            const int yu = y > 0 ? y - 1 : (h > 1 ? 1 : 0), yd = y < h - 1 ? y + 1 : (h > 1 ? h - 2 : 0);
            const double gx = (double)img[(size_t)y * w + xr] - (double)img[(size_t)y * w + xl];
            const double gy = (double)img[(size_t)yd * w + x] - (double)img[(size_t)yu * w + x];
            const unsigned long long u = (unsigned long long)__double_as_longlong(sqrt(gx * gx + gy * gy));
            lo = u < lo ? u : lo;
            hi = u > hi ? u : hi;
        }
    }
    for (int s = 32; s >= 1; s >>= 1) {
        const unsigned long long ol = __shfl_xor(lo, s, 64), oh = __shfl_xor(hi, s, 64);
        lo = ol < lo ? ol : lo;
        hi = oh > hi ? oh : hi;
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[wave] = lo;
        red[4 + wave] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int q = 1; q < 4; ++q) {
            lo = red[q] < lo ? red[q] : lo;
            hi = red[4 + q] > hi ? red[4 + q] : hi;
        }
        if (lo != ~0ULL) atomicMin(&minmax[0], lo);
        atomicMax(&minmax[1], hi);
    }
}

// -------------------------------------------------------- k_neighbor_count ---
// MVS::neighborPatchFiltering (mvs.cpp:448-524), the O(n^2) part: for every patch the number of OTHER patches
// whose centre lies within neighborRadius (the reference sorts all distances and counts up to the first one
// beyond the radius: the same number).  One thread per patch i; the centres are streamed through LDS in tiles
// of 256.  dist = sqrt(dx*dx + dy*dy + dz*dz) accumulated in that order (cv::norm of a Vec3d), compared as
// `!(dist > radius)` like the reference's `if (dist > neighborRadius) break`.
__global__ __launch_bounds__(256) void k_neighbor_count(const double *centers, int n, double radius, int32_t *counts)
{
    __shared__ double tile[256 * 3];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool has = i < n;
    const double cx = has ? centers[3 * i] : 0, cy = has ? centers[3 * i + 1] : 0, cz = has ? centers[3 * i + 2] : 0;
    int cnt = 0;
    for (int base = 0; base < n; base += 256) {
        const int m = (n - base) < 256 ? (n - base) : 256;
        __syncthreads();
        for (int t = threadIdx.x; t < 3 * m; t += 256) tile[t] = centers[3 * (size_t)base + t];
        __syncthreads();
        for (int j = 0; j < m; ++j) {
            const double dx = cx - tile[3 * j], dy = cy - tile[3 * j + 1], dz = cz - tile[3 * j + 2];
            double s2 = 0;
            s2 += dx * dx;
            s2 += dy * dy;
            s2 += dz * dz;
            const double dist = sqrt(s2);
            cnt += ((base + j) != i && !(dist > radius)) ? 1 : 0;
        }
    }
    if (has) counts[i] = cnt;
}

// --------------------------------------------------------------- launchers ---
namespace pais_launch {

// Every launch of this file goes through here.  A kernel that asks for more than 64 KB of dynamic LDS needs
// hipFuncAttributeMaxDynamicSharedMemorySize raised first, per device: the largest size set so far is remembered per
// (kernel instantiation, device), so a second context on another GPU of the same process sets it again; a device index
// outside the table sets it every time.
template <auto Kern, class... A> static hipError_t launch(dim3 grid, dim3 block, size_t lds, hipStream_t stream, const A &...args)
{
    if (lds > 64 * 1024) {
        static size_t setFor[64] = {0};
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        const bool known = dev >= 0 && dev < 64;
        if (!known || lds > setFor[dev]) {
            e = hipFuncSetAttribute((const void *)Kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
            if (known) setFor[dev] = lds;
        }
    }
    hipLaunchKernelGGL(Kern, grid, block, lds, stream, args...);
    return hipGetLastError();
}
// workgroups of a launch over n items: one at least, `cap` at the most (the kernels stride over the rest)
static inline unsigned grid_for(long n, long cap) { return (unsigned)(n < 1 ? 1 : (n < cap ? n : cap)); }
static const long EVAL_GRID_CAP = 262144; // of an evaluation launch, one wave per task

// LDS of the camera-removal kernels (k_after, k_ncc_batch) in front of the warped patches: the record (recBytes), the NCC
// table, the homographies and the drop flag of remove_invisible_camera
static size_t ncc_scratch_bytes(size_t recBytes, int Kmax)
{
    return ((recBytes + 15) & ~(size_t)15) + sizeof(double) * Kmax * Kmax + sizeof(double) * 9 * Kmax + 16;
}
size_t ncc_lds_bytes(int Kmax) { return ncc_scratch_bytes(sizeof(pais_view_result), Kmax); }
// ... and the warped patches of a workgroup behind them while they are at most 60 KB (<= 2 workgroups per CU otherwise)
static size_t hp_bytes(const DevScene &sc, int Kmax) { return sizeof(double) * (size_t)Kmax * sc.cfg.patchSize * sc.cfg.patchSize; }
bool hp_in_lds(const DevScene &sc, int Kmax) { return hp_bytes(sc, Kmax) <= 60 * 1024; }

// shape of the evaluation kernels for a batch (pais_eval.hpp): 0: NS 2 / LDS accumulators, 1: NS 2 / register
// accumulators, 2: NS 1 / register accumulators
// (two window pixels per lane only while the LDS scratch leaves >= 3 waves per SIMD: M = K - 1 cameras are tapped)
#ifndef PAIS_TWO_PIXELS_REG_MAXK
#define PAIS_TWO_PIXELS_REG_MAXK 12
#endif
static inline int eval_shape(int Kmax) { return Kmax <= PAIS_TWO_PIXELS_MAXK ? 0 : (Kmax <= PAIS_TWO_PIXELS_REG_MAXK ? 1 : 2); }
// the scene decides what the taps read (pais_internal.h PaisImgT)
static inline bool byte_taps(const DevScene &sc) { return sc.imgF == nullptr; }
template <class T, T V> struct Const { constexpr operator T() const { return V; } }; // a value a generic lambda can name as a template argument
template <int V> using Int = Const<int, V>;
template <bool V> using Bool = Const<bool, V>;
// calls f(Int<NS>, Bool<BYTES>, Bool<ACCR>) for the batch's shape and the scene's tap representation
template <class F> static hipError_t shape_dispatch(const DevScene &sc, int Kmax, F f)
{
    const int shape = eval_shape(Kmax);
    if (byte_taps(sc))
        return shape == 0 ? f(Int<2>(), Bool<true>(), Bool<false>())
                          : (shape == 1 ? f(Int<2>(), Bool<true>(), Bool<true>()) : f(Int<1>(), Bool<true>(), Bool<true>()));
    return shape == 0 ? f(Int<2>(), Bool<false>(), Bool<false>())
                      : (shape == 1 ? f(Int<2>(), Bool<false>(), Bool<true>()) : f(Int<1>(), Bool<false>(), Bool<true>()));
}

size_t eval_block_bytes_host(int Kmax) { return eval_block_bytes(Kmax); }
size_t win_bytes_per_candidate(const DevScene &sc) { return sizeof(WinPix) * (size_t)win_stride(sc); }
size_t pso_state_bytes_host(int Nmax) { return pso_state_bytes(Nmax); }
// the evaluation records of the initial swarm of every active candidate (pais_pre.hpp); behind k_begin / k_pso_init
size_t pre_bytes_per_candidate(int Nmax, int Kmax) { return pre_rec_bytes(Kmax) * (size_t)Nmax; }

// the one place that knows the per-candidate strides of a batch's buffers
BatchView BatchView::slice(const DevScene &sc, int lo, int hi, hipStream_t st) const
{
    BatchView s = *this;
    s.recs = recs + lo;
    s.states = states + pso_state_bytes(Nmax) * (size_t)lo;
    s.evalBlocks = evalBlocks + eval_block_bytes(Kmax) * (size_t)lo;
    s.win = win + win_bytes_per_candidate(sc) * (size_t)lo;
    if (pre) s.pre = (double *)((unsigned char *)pre + pre_bytes_per_candidate(Nmax, Kmax) * (size_t)lo);
    s.n = hi - lo;
    s.stream = st;
    return s;
}

// the evaluation blocks and reference windows of caller-given states (pais_fitness_batch, pais_fitness_detail)
hipError_t state_blocks(const DevScene &sc, const pais_patch_state *states, int nStates, int Kmax, unsigned char *evalBlocks, void *win,
                        hipStream_t stream)
{
    if (nStates <= 0) return hipSuccess;
    return launch<k_state_blocks>(grid_for(nStates, 65536), dim3(64), 0, stream, sc, states, nStates, evalBlocks, eval_block_bytes(Kmax),
                                  (WinPix *)win);
}
hipError_t fitness(const DevScene &sc, const pais_patch_state *states, int nStates, const int32_t *idx, const double *particles,
                   double *out, int nEvals, int Kmax, unsigned char *evalBlocks, void *win, int literal, hipStream_t stream)
{
    if (nEvals <= 0) return hipSuccess;
    const hipError_t e = state_blocks(sc, states, nStates, Kmax, evalBlocks, win, stream);
    if (e != hipSuccess) return e;
    const unsigned char *blocks = evalBlocks;
    if (literal) // PAIS_ARITH=literal (pais_literal.hpp)
        return launch<k_fitness_lit>(grid_for(nEvals, 1 << 20), dim3(64), literal_lds_bytes(Kmax, sc.cfg.patchSize), stream, sc, idx, particles,
                                     out, nEvals, Kmax, blocks, eval_block_bytes(Kmax));
    return shape_dispatch(sc, Kmax, [&](auto ns, auto bytes, auto accr) {
        return launch<k_fitness<ns, bytes, accr>>(grid_for(nEvals, EVAL_GRID_CAP), dim3(64), eval_lds_bytes(ns, Kmax, accr), stream, sc, idx,
                                                  particles, out, nEvals, Kmax, blocks, eval_block_bytes(Kmax), (const WinPix *)win);
    });
}
// pais_fitness_detail: behind state_blocks, one wave per evaluation (k_fitness_detail)
hipError_t fitness_detail(const DevScene &sc, const int32_t *idx, const double *particles, int nEvals, int Kmax, const unsigned char *evalBlocks,
                          pais_cost_detail *rec, double *weight, double *avgSad, int8_t *code, double *colour, double *H, hipStream_t stream)
{
    if (nEvals <= 0) return hipSuccess;
    return launch<k_fitness_detail>(grid_for(nEvals, 1 << 20), dim3(64), literal_lds_bytes(Kmax, sc.cfg.patchSize), stream, sc, idx, particles,
                                    nEvals, Kmax, evalBlocks, eval_block_bytes(Kmax), rec, weight, avgSad, code, colour, H);
}

// k_begin + the set-up of the first PSO run of every candidate (what k_pso_init does in later passes)
hipError_t begin(const DevScene &sc, const BatchView &v, const pais_candidate *cands, int *activeList, int *activeCount)
{
    if (v.n <= 0) return hipSuccess;
    return launch<k_begin<true>>(grid_for(v.n, 16384), dim3(64), 0, v.stream, sc, cands, v.recs, v.n, v.states, v.Nmax, activeList, activeCount,
                                 v.evalBlocks, eval_block_bytes(v.Kmax), (WinPix *)v.win);
}
hipError_t pso_init(const DevScene &sc, const BatchView &v, int *activeList, int *activeCount)
{
    return launch<k_pso_init>(grid_for(v.n, 65536), dim3(64), 0, v.stream, sc, v.recs, v.n, v.states, v.Nmax, activeList, activeCount,
                              v.evalBlocks, eval_block_bytes(v.Kmax), (WinPix *)v.win);
}

hipError_t load_state(const DevScene &sc, const pais_loaded_patch *in, pais_patch_result *recs, int n, uint64_t key0, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    return launch<k_load_state>(grid_for(n, 16384), dim3(64), 0, stream, sc, in, recs, n, key0);
}
hipError_t expand_image(const uint8_t *img, PaisImgT *out, size_t n, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    return launch<k_expand_image>(grid_for((long)((n + 255) / 256), 1 << 20), dim3(256), 0, stream, img, out, n);
}
// minmax[0] = ~0, minmax[1] = 0 on entry (ordered bit patterns of the minimum / maximum magnitude on exit)
hipError_t level_edge_minmax(const uint8_t *img, int w, int h, unsigned long long *minmax, hipStream_t stream)
{
    return launch<k_level_edge_minmax>(dim3((w + 255) / 256, (h + 15) / 16), dim3(256), 0, stream, img, w, h, minmax);
}
hipError_t neighbor_count(const double *centers, int n, double radius, int32_t *counts, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    return launch<k_neighbor_count>(dim3((n + 255) / 256), dim3(256), 0, stream, centers, n, radius, counts);
}
hipError_t pack_records(const pais_patch_result *recs, int n, int Kw, void *wire, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    const size_t words = (size_t)n * (52 + 5 * Kw);
    return launch<k_pack_records>(grid_for((long)((words + 255) / 256), 65536), dim3(256), 0, stream, recs, n, Kw, (uint32_t *)wire);
}
hipError_t wire_header(void *header, const unsigned *ringCtl, int ringN, int rank, int count, int hostRc, uint32_t userWord, hipStream_t stream)
{
    return launch<k_wire_header>(dim3(1), dim3(64), 0, stream, (uint32_t *)header, (const RingCtl *)ringCtl, ringN, rank, count, hostRc, userWord);
}

// the evaluation launch of large batches; v.pre: evaluation records (pais_pre.hpp), nullptr: the evaluation sets itself up
hipError_t pso_eval(const DevScene &sc, const BatchView &v, int pendingOnly, unsigned long long *verify)
{
    // pending-only (behind k_pso_tile2): a handful of particles at most -- a few waves scan the flags (grid-stride loop);
    // one workgroup per particle would queue tens of thousands of workgroups, each asking for LDS, behind the tile
    // kernel of the other sub-stream, which holds every CU's LDS (measured: 2.2 ms per launch spent waiting)
    const unsigned grid = grid_for((long)v.n * v.Nmax, pendingOnly == 1 ? 256 : EVAL_GRID_CAP);
    return shape_dispatch(sc, v.Kmax, [&](auto ns, auto bytes, auto accr) {
        constexpr int NS = ns;
        constexpr bool BYTES = bytes, ACCR = accr;
        auto go = [&](auto usePre) {
            return launch<k_pso_eval2<NS, BYTES, ACCR, usePre>>(grid, dim3(64), eval_lds_bytes(NS, v.Kmax, ACCR), v.stream, sc, v.states, v.n, v.Nmax,
                                                                v.Kmax, (const unsigned char *)v.evalBlocks, eval_block_bytes(v.Kmax),
                                                                (const WinPix *)v.win, pendingOnly, verify, (const double *)v.pre);
        };
        return v.pre ? go(Bool<true>()) : go(Bool<false>());
    });
}
// (the one-pixel ring kernel with the step's record code needs 177 VGPRs -- 2 waves / SIMD instead of 3: it keeps setting itself up)
#ifndef PAIS_PRE_RING_NS1
#define PAIS_PRE_RING_NS1 0
#endif
bool pre_ring_ok(int Kmax) { return PAIS_PRE_RING_NS1 || eval_shape(Kmax) != 2; }
hipError_t pso_setup0(const DevScene &sc, const BatchView &v)
{
    if (v.n <= 0) return hipSuccess;
    const size_t lds = eval_block_bytes(v.Kmax) + sizeof(double) * 3 * (size_t)v.Nmax + pre_scratch_bytes(v.Nmax);
    return launch<k_pso_setup0>(grid_for(v.n, 65536), dim3(64), lds, v.stream, sc, v.states, v.n, v.Nmax, (const unsigned char *)v.evalBlocks,
                                eval_block_bytes(v.Kmax), v.pre, v.Kmax);
}
// the evaluation launch of a PSO iteration under PAIS_ARITH=literal (pais_literal.hpp)
hipError_t pso_eval_literal(const DevScene &sc, const BatchView &v)
{
    return launch<k_pso_eval_lit>(grid_for((long)v.n * v.Nmax, 1 << 20), dim3(64), literal_lds_bytes(v.Kmax, sc.cfg.patchSize), v.stream, sc,
                                  v.states, v.n, v.Nmax, v.Kmax, (const unsigned char *)v.evalBlocks, eval_block_bytes(v.Kmax));
}
// many-camera batches: the tile kernel (pais_tile2.hpp) can take the evaluation launch of the large-batch pipeline
bool tile_eligible(int Kmax) { return eval_shape(Kmax) == 2 && Kmax <= TILE_MAX_CAMS; }
// k_pso_tile2<NP>: sixteen waves walk TILE2_SLOTS particles per workgroup; what the fixed part leaves of the LDS is the tile area
template <int NP>
static hipError_t tile_launch(const DevScene &sc, const BatchView &v, const TileOpts &o, unsigned long long *dbg)
{
    const size_t lds = (160 * 1024) & ~(size_t)1023, fixed = tile2_fixed_lds_bytes(v.Kmax);
    if (fixed + 4096 > lds) return hipErrorInvalidValue;
    const int groups = (v.Nmax + TILE2_SLOTS - 1) / TILE2_SLOTS;
    return launch<k_pso_tile2<NP>>(grid_for((long)v.n * groups, 65536), dim3(64 * TILE2_WAVES), lds, v.stream, sc, v.states, v.n, v.Nmax, v.Kmax,
                                   (const unsigned char *)v.evalBlocks, eval_block_bytes(v.Kmax), (const WinPix *)v.win,
                                   o.noTiles ? 0 : (int)(lds - fixed), groups, o.stripSteps, dbg);
}
hipError_t pso_tile(const DevScene &sc, const BatchView &v, const TileOpts &o, unsigned long long *dbg)
{
    // the colours of at most NP pairs per wave: Kmax <= 4 NP cameras, with room for the first half's larger share
    if (v.Kmax <= 28) return tile_launch<8>(sc, v, o, dbg);
    if (v.Kmax <= 44) return tile_launch<12>(sc, v, o, dbg);
    return tile_launch<16>(sc, v, o, dbg);
}
// positions [listLo, listHi) of the active list of the WHOLE batch `v` (on v.stream): list positions are not candidate indices
hipError_t pso_iter(const DevScene &sc, const BatchView &v, const int *activeList, const int *activeCount, int listLo, int listHi,
                    unsigned long long *stat, int L, int finishOnly, int nparts)
{
    if (listHi <= listLo) return hipSuccess;
    return shape_dispatch(sc, v.Kmax, [&](auto ns, auto bytes, auto accr) {
        constexpr int NS = ns;
        constexpr bool BYTES = bytes, ACCR = accr;
        auto go = [&](auto parts) {
            return launch<k_pso_iter<parts, NS, BYTES, ACCR>>(grid_for((long)(listHi - listLo) * (finishOnly ? 1 : v.Nmax * parts), EVAL_GRID_CAP),
                                                              dim3(64), eval_lds_bytes(NS, v.Kmax, ACCR), v.stream, sc, v.states, activeList, activeCount,
                                                              listLo, listHi, v.Nmax, v.Kmax, v.recs, stat, L, finishOnly,
                                                              (const unsigned char *)v.evalBlocks, eval_block_bytes(v.Kmax), (const WinPix *)v.win);
        };
        return nparts == 4 ? go(Int<4>()) : (nparts == 2 ? go(Int<2>()) : go(Int<1>()));
    });
}
// k_pso_ring: a whole PSO pass of a large batch in one launch (ring: n * Nmax * (maxIt + 2) words, ctl: 8 words, arrive: n ints --
// all zeroed / emptied here).  waves: resident waves to work the ring off with.
// parts: waves per evaluation (1, 2, 4): a candidate publishes Nmax * parts tasks per iteration
static size_t ring_seg_words(int n, int Nmax, int maxIt, int parts) { return (size_t)((n + PAIS_RINGS - 1) / PAIS_RINGS) * Nmax * parts * ((size_t)maxIt + 2); }
size_t ring_words(int n, int Nmax, int maxIt, int parts) { return ring_seg_words(n, Nmax, maxIt, parts) * PAIS_RINGS; }
// the part kernels exist for the two-pixel shapes (K <= PAIS_TWO_PIXELS_REG_MAXK): batches of more cameras are large or streamed
bool ring_parts_ok(int Kmax) { return eval_shape(Kmax) != 2; }
hipError_t pso_ring(const DevScene &sc, const BatchView &v, unsigned *ring, unsigned *ctl, int *arrive, unsigned long long *stat, int waves,
                    int phase, unsigned long long timeoutTicks, int parts)
{
    if (parts != 1 && !((parts == 2 || parts == 4) && ring_parts_ok(v.Kmax))) return hipErrorInvalidValue;
    const int n = v.n, Nmax = v.Nmax, Kmax = v.Kmax;
    // k_pso_ring publishes a candidate's tasks by the lanes of one wave and holds the lane-parallel swarm step alone
    // (pso_step_wave_ring: no serial form for larger swarms) -- the caller keeps such batches on the per-iteration launches
    if (Nmax > 64) return hipErrorInvalidValue;
    const size_t words = ring_words(n, Nmax, v.maxIt, parts), seg = ring_seg_words(n, Nmax, v.maxIt, parts);
    if (seg >= 0xFFFFFFF0ull) return hipErrorInvalidValue;
    if (phase == 0) { // empty rings, zero counters, the tasks of iteration 0
        hipError_t e = hipMemsetAsync(ring, 0xFF, words * sizeof(unsigned), v.stream);
        if (e != hipSuccess) return e;
        e = hipMemsetAsync(ctl, 0, sizeof(RingCtl) * PAIS_RINGS, v.stream);
        if (e != hipSuccess) return e;
        e = hipMemsetAsync(arrive, 0, sizeof(int) * PAIS_ARRIVE_STRIDE * (size_t)n, v.stream);
        if (e != hipSuccess) return e;
        return launch<k_ring_init>(dim3((n + 255) / 256), dim3(256), 0, v.stream, v.states, n, Nmax, ring, (unsigned)seg, (RingCtl *)ctl, parts);
    }
    return shape_dispatch(sc, Kmax, [&](auto ns, auto bytes, auto accr) {
        constexpr int NS = ns;
        constexpr bool BYTES = bytes, ACCR = accr;
        // (with records the step's scratch lies behind the evaluation block and includes the scratch of swarm_eval_setup)
        const size_t stepBytes = v.pre ? eval_block_bytes(Kmax) + step_lds_bytes(Nmax) : sizeof(double) * (size_t)Nmax * (3 * 4 + 2) + 16;
        size_t per = eval_lds_bytes(NS, Kmax, ACCR);
        if (per < stepBytes) per = stepBytes;
        per = (per + 15) & ~(size_t)15;
        // `waves` arrives as the number of CUs: resident waves per CU by shape; whole rounds of the rings
        const long resident = (long)waves * (NS == 1 ? 4 * PAIS_NS1_WAVES : 4 * PAIS_NS2_WAVES);
        const unsigned grid = (grid_for((long)n * Nmax * parts, resident) + PAIS_RINGS - 1) / PAIS_RINGS * PAIS_RINGS;
        auto go = [&](auto usePre, auto np) {
            return launch<k_pso_ring<NS, BYTES, ACCR, usePre, np>>(dim3(grid), dim3(64), per, v.stream, sc, v.recs, v.states, n, Nmax, Kmax,
                                                                   (const unsigned char *)v.evalBlocks, eval_block_bytes(Kmax), (const WinPix *)v.win, ring,
                                                                   (unsigned)seg, (RingCtl *)ctl, arrive, stat, per, timeoutTicks, v.pre);
        };
        if constexpr (NS == 2) {
            if (parts == 4) return v.pre ? go(Bool<true>(), Int<4>()) : go(Bool<false>(), Int<4>());
            if (parts == 2) return v.pre ? go(Bool<true>(), Int<2>()) : go(Bool<false>(), Int<2>());
        }
        return v.pre ? go(Bool<true>(), Int<1>()) : go(Bool<false>(), Int<1>());
    });
}
// v.pre: the step also writes the evaluations' set-up records of the moved swarm
hipError_t pso_step(const DevScene &sc, const BatchView &v, unsigned long long *stat)
{
    const size_t lds = v.pre ? eval_block_bytes(v.Kmax) + step_lds_bytes(v.Nmax) : sizeof(double) * (size_t)v.Nmax * (3 * 4 + 2);
    return launch<k_pso_step>(grid_for(v.n, 65536), dim3(64), lds, v.stream, sc, v.recs, v.states, v.n, v.Nmax, stat,
                              (const unsigned char *)v.evalBlocks, eval_block_bytes(v.Kmax), v.pre, v.Kmax);
}
hipError_t pso_step_trace(const DevScene &sc, const BatchView &v, unsigned long long *stat, const TraceSink &t)
{
    if (v.n <= 0) return hipSuccess;
    StepTraceSink sink;
    sink.runs = t.runs;
    sink.iters = t.iters;
    sink.particles = t.particles;
    sink.maxRuns = t.maxRuns;
    sink.rows = t.rows;
    sink.NP = v.Nmax;
    return launch<k_pso_step_trace>(grid_for(v.n, 65536), dim3(64), sizeof(double) * (size_t)v.Nmax * (3 * 4 + 2), v.stream, sc, v.recs, v.states,
                                    v.n, v.Nmax, stat, sink);
}

hipError_t after(const DevScene &sc, pais_patch_result *recs, int n, double *hpScratch, int grid, int *counters,
                 unsigned long long *stat, int Kmax, double *ratios, int *nextCounters, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    const int hpInLds = hp_in_lds(sc, Kmax) ? 1 : 0;
    const size_t lds = ncc_scratch_bytes(sizeof(pais_patch_result), Kmax) + (hpInLds ? hp_bytes(sc, Kmax) : 0);
    const dim3 rgrid((unsigned)(((long)n * Kmax + 63) / 64)), block(64 * AFTER_WAVES);
    hipError_t e = launch<k_region_ratio>(rgrid, dim3(64), 0, stream, sc, recs, n, PAIS_STAGE_AFTER, ratios, Kmax);
    if (e == hipSuccess)
        e = launch<k_after<1>>(dim3(grid), block, lds, stream, sc, recs, n, hpScratch, counters, stat, Kmax, ratios, hpInLds, (int *)nullptr);
    if (e == hipSuccess) e = launch<k_region_ratio>(rgrid, dim3(64), 0, stream, sc, recs, n, PAIS_STAGE_AFTER2, ratios, Kmax);
    if (e == hipSuccess)
        e = launch<k_after<2>>(dim3(grid), block, lds, stream, sc, recs, n, hpScratch, counters, stat, Kmax, ratios, hpInLds, nextCounters);
    return e;
}
hipError_t ncc_batch(const DevScene &sc, const pais_view_state *states, int n, pais_view_result *out, double *tables, int stride,
                     double *hpScratch, int grid, int Kmax, int hpInLds, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    const size_t lds = ncc_lds_bytes(Kmax) + (hpInLds ? hp_bytes(sc, Kmax) : 0);
    return launch<k_ncc_batch>(dim3(grid), dim3(64 * AFTER_WAVES), lds, stream, sc, states, n, out, tables, stride, hpScratch, Kmax, hpInLds);
}

// pais_test_swarm_step: the caller's swarm as a one-candidate PsoState, one k_pso_step-like wave over it
__global__ __launch_bounds__(64) void k_test_swarm_step(DevScene sc, pais_patch_result *recs, unsigned char *states, int Nmax,
                                                        unsigned long long *stat, int *continues)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem0[];
    PsoState *hd = (PsoState *)states;
    const int N = __builtin_amdgcn_readfirstlane(hd->N);
    const int cont = pso_step_wave(sc, recs, 0, hd, N, Nmax, smem0, stat, (int)threadIdx.x);
    if (threadIdx.x == 0) *continues = cont;
}
int test_swarm_step(pais_test_swarm *s, double *swarm)
{
    if (!s || !swarm || s->n < 1 || s->n > 128) return (int)hipErrorInvalidValue;
    const int N = s->n;
    const size_t SB = pso_state_bytes(N), head = (sizeof(PsoState) + 15) & ~(size_t)15;
    unsigned char *host = (unsigned char *)calloc(1, SB);
    if (!host) return (int)hipErrorOutOfMemory;
    PsoState *hd = (PsoState *)host;
    for (int d = 0; d < 3; ++d) {
        hd->rangeL[d] = s->range_l[d];
        hd->rangeU[d] = s->range_u[d];
        hd->ray[d] = d == 2 ? 1.0 : 0.0;
    }
    hd->iw = s->iw;
    hd->gBestFitness = s->gbest_fitness;
    hd->streamBase = s->stream_base;
    hd->gIdx = s->g_idx;
    hd->N = N;
    hd->maxIt = s->max_iteration;
    hd->iteration = s->iteration;
    hd->active = 1;
    hd->run = s->run;
    hd->localK = s->local_k;
    hd->started = s->started;
    hd->K = 3;
    // swarm buffer 0 (pso_arrays): pos, vec, pBest, nBest [N][3], fit, pBestFit [N]
    double *arr = (double *)(host + head);
    for (int i = 0; i < N; ++i) {
        for (int a = 0; a < 4; ++a)
            for (int d = 0; d < 3; ++d) arr[(size_t)a * 3 * N + 3 * i + d] = swarm[14 * i + 3 * a + d];
        arr[(size_t)12 * N + i] = swarm[14 * i + 12];
        arr[(size_t)13 * N + i] = swarm[14 * i + 13];
    }
    unsigned char *dev = nullptr;
    const size_t offRec = (SB + 255) & ~(size_t)255, offStat = offRec + ((sizeof(pais_patch_result) + 255) & ~(size_t)255),
                 offCam = offStat + 256, offCont = offCam + ((sizeof(DevCamera) + 255) & ~(size_t)255), total = offCont + 256;
    hipError_t e = hipMalloc((void **)&dev, total);
    if (e == hipSuccess) e = hipMemset(dev, 0, total);
    if (e == hipSuccess) e = hipMemcpy(dev, host, SB, hipMemcpyHostToDevice);
    pais_patch_result rec;
    int cont = 0;
    if (e == hipSuccess) {
        DevScene sc;
        memset(&sc, 0, sizeof(sc));
        sc.cams = (const DevCamera *)(dev + offCam);
        sc.cfg.maxFitness = 10.0;
        sc.numCams = 1;
        e = launch<k_test_swarm_step>(dim3(1), dim3(64), sizeof(double) * (size_t)N * (3 * 4 + 2) + 16, nullptr, sc,
                                      (pais_patch_result *)(dev + offRec), dev, N, (unsigned long long *)(dev + offStat), (int *)(dev + offCont));
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(host, dev, SB, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(&rec, dev + offRec, sizeof(rec), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(&cont, dev + offCont, sizeof(int), hipMemcpyDeviceToHost);
    if (e == hipSuccess) {
        for (int i = 0; i < N; ++i) {
            for (int a = 0; a < 4; ++a)
                for (int d = 0; d < 3; ++d) swarm[14 * i + 3 * a + d] = arr[(size_t)a * 3 * N + 3 * i + d];
            swarm[14 * i + 12] = arr[(size_t)12 * N + i];
            swarm[14 * i + 13] = arr[(size_t)13 * N + i];
        }
        s->iw = hd->iw;
        s->gbest_fitness = hd->gBestFitness;
        s->g_idx = hd->gIdx;
        s->iteration = hd->iteration;
        s->started = hd->started;
        s->continues = cont;
        s->result[0] = rec.fitness;
        s->result[1] = rec.normalS[0];
        s->result[2] = rec.normalS[1];
        s->result[3] = rec.depth;
    }
    if (dev) (void)hipFree(dev);
    free(host);
    return (int)e;
}

void ring_profile_print()
{
#if PAIS_RING_PROFILE
    unsigned long long h[8] = {0};
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_ringProf), sizeof(h)) != hipSuccess || h[6] == 0) return;
    const char *nm[6] = {"index (head atomic)", "entry wait", "loads + staging", "evaluation", "fitness store + arrival", "swarm step + publish"};
    double tot = 0;
    for (int k = 0; k < 6; ++k) tot += (double)h[k];
    fprintf(stderr, "[ring profile] %llu tasks, %llu steps; s_memtime ticks per task:\n", h[6], h[7]);
    for (int k = 0; k < 6; ++k)
        fprintf(stderr, "[ring profile]   %-26s %10.1f  (%5.1f %%)%s\n", nm[k], (double)h[k] / (double)h[6], 100.0 * (double)h[k] / tot,
                k == 5 ? "  (per step: see steps)" : "");
    fprintf(stderr, "[ring profile]   per step %.1f ticks\n", h[7] ? (double)h[5] / (double)h[7] : 0.0);
#endif
}
} // namespace pais_launch
