// pais_internal.h -- device-side scene layout shared by pais_kernels.hip and pais_capi.hip
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pais_hip.h"

// refine() progress of a record (pais_patch_result::stage)
#define PAIS_STAGE_DONE  0
#define PAIS_STAGE_PSO   1  /* psoOptimization() pending (patch.cpp:153)           */
#define PAIS_STAGE_AFTER 2  /* PSO finished, removeInvisibleCamera etc. pending     */
#define PAIS_STAGE_AFTER2 3 /* refine() has ended: the caller's removeInvisibleCamera (mvs.cpp:215 / :574) pending */
#define PAIS_STAGE_AFTER2_KEEP 4 /* ... and the region ratios of the first call are still valid                     */
#define PAIS_STAGE_AFTER2_SAME 7 /* ... and the first call removed no camera: the second one sees the very same inputs (5, 6: PAIS_DONE_*) */

// HBM layout: one DevCamera per camera in a dense array;
// every pyramid level of every camera repacked row-major with stride == width
// into one byte blob (levels 256-byte aligned), edge levels likewise as doubles.
// The cost kernel's bilinear taps read either a float2 copy of the byte blob (imgF) or the byte blob itself
// (DevScene::imgF == nullptr): see PaisImgT below.
struct DevCamera {
    double KR[9], KT[3], R[9], T[3], C[3], optN[3], focal[2], pp[2];
    int maxLOD;
    int pad;
    int w[PAIS_MAX_LEVELS], h[PAIS_MAX_LEVELS];
    // offsets into DevScene::imgBlob (bytes) / DevScene::edgeBlob (doubles): keeping the base in a
    // kernel argument lets the compiler emit global_load (saddr) instead of flat_load for every tap
    uint64_t imgOff[PAIS_MAX_LEVELS];
    uint64_t edgeOff[PAIS_MAX_LEVELS];
    // edge maps evaluated on the fly (DevScene::edgeBlob == nullptr while adaptiveGradientEnable is set): the minimum and
    // maximum Sobel magnitude of every level, what the per-level normalisation of camera.cpp:72-77,87-91 needs
    double edgeMin[PAIS_MAX_LEVELS], edgeMax[PAIS_MAX_LEVELS];
};

// What the cost taps read (a property of the uploaded scene; the sampled values are identical either way):
//   float2 {I(x), I(x+1) - I(x)}  a copy of the byte blob with identical element offsets (imgOff): a tap row = one aligned
//                                 8-byte load, no unpacking, no subtraction.  +10 % evaluations/s where the working set
//                                 of a batch sits in L2 anyway (pawn: 107 vs 97 M evaluations/s) -- at 8x the bytes;
//   the byte blob itself          a tap row = one 2-byte load + byte->double conversions and one subtraction.  An eighth
//                                 of the footprint: +21 % patches/s on the 128 x 12.6 MP dome (4.5 GB instead of 36 GB
//                                 of pyramids, and the taps of a batch stop missing L2 / the TLB); equal on the ring.
// pais_create expands the float2 copy when the byte pyramids are at most PAIS_TAP_FLOAT_MAX_MB (default 256 MB, i.e. a
// 2 GB copy); larger scenes run the BYTES instantiations of the evaluation kernels.
typedef float2 PaisImgT; // (a double2 copy measured no faster: profiles/r03_tap_representation_ab.txt)

struct DevScene {
    pais_config cfg;
    const DevCamera *cams;
    const uint8_t *imgBlob;
    const PaisImgT *imgF;   // tap copy of imgBlob, same element offsets (imgOff); nullptr: the taps read imgBlob (BYTES kernels)
    const double *edgeBlob; // normalised Sobel magnitude per level as the caller built it; nullptr: evaluated on the fly
    const double *gauss; // patchDistWeight, S*S, indexed [x*S + y] (mvs.cpp:104-109)
    double lodScale[PAIS_MAX_LEVELS]; // pow(lodRatio, LOD) (camera.cpp:157, patch.cpp:309)
    uint64_t seed;
    int numCams;
    int pad;
};

// control words of one task ring of k_pso_ring (pais_kernels.hip RingCtl): head | tail, done, total, error
#ifndef PAIS_RINGS
#define PAIS_RINGS 8 // (16 and 32 rings -- two / four per XCD -- measured: no gain, profiles/r04_ring_count_ab.txt)
#endif
// a candidate's arrival counter (one atomic per delivered evaluation) on a cache line of its own: neighbouring candidates belong
// to other rings, i.e. other XCDs
#ifndef PAIS_ARRIVE_STRIDE
#define PAIS_ARRIVE_STRIDE 16
#endif
#define PAIS_RING_CTL_BYTES 128
#define PAIS_RING_CTL_DONE_WORD 17
#define PAIS_RING_CTL_ERROR_WORD 19

struct pais_test_swarm; // include/pais_test_hooks.h
namespace pais_launch {
// A batch, or a slice of one, as the kernels index it: the buffers point at its first candidate.
struct BatchView {
    pais_patch_result *recs;
    unsigned char *states;     // PsoState blocks
    unsigned char *evalBlocks; // EvalPatch + EvalCam[Kmax] (pais_eval.hpp)
    unsigned char *win;        // reference windows
    double *pre;               // evaluation records {status, homographies} per particle (pais_pre.hpp); nullptr: none are kept
    int n, Nmax, Kmax, maxIt;
    hipStream_t stream;
    BatchView slice(const DevScene &sc, int lo, int hi, hipStream_t st) const; // candidates [lo, hi) on stream st
};
// pais_pso_trace: where the swarm steps of a view record (the view's first candidate first); rows per run
struct TraceSink {
    pais_pso_run_info *runs; // [n][maxRuns]
    pais_pso_iter *iters;    // [n][maxRuns][rows]
    double *particles;       // nullptr or [n][maxRuns][rows][Nmax][11]
    int maxRuns, rows;
};
// the tile kernel's knobs (k_pso_tile2, pais_tile2.hpp), read once in pais_create
struct TileOpts {
    int stripSteps = 16; // PAIS_TILE_STRIP_SPLIT: 64-pixel steps per strip
    int noTiles = 0;     // PAIS_TILE_NOTILES (tests): no tile area at all, every camera is tapped in global memory
};

// buffer sizes per candidate: evaluation block, reference window, PSO state, evaluation records
size_t eval_block_bytes_host(int Kmax);
size_t win_bytes_per_candidate(const DevScene &sc);
size_t pso_state_bytes_host(int Nmax);
size_t pre_bytes_per_candidate(int Nmax, int Kmax);
// the caller-given states of pais_fitness_batch / pais_fitness_detail: their evaluation blocks (k_state_blocks), then one wave per
// evaluation (k_fitness; k_fitness_detail, literal_lds_bytes(Kmax, S) of LDS: colour and H may be nullptr, else Kmax rows per evaluation)
hipError_t state_blocks(const DevScene &sc, const pais_patch_state *states, int nStates, int Kmax, unsigned char *evalBlocks, void *win,
                        hipStream_t stream);
hipError_t fitness(const DevScene &sc, const pais_patch_state *states, int nStates, const int32_t *idx, const double *particles,
                   double *out, int nEvals, int Kmax, unsigned char *evalBlocks, void *win, int literal, hipStream_t stream);
hipError_t fitness_detail(const DevScene &sc, const int32_t *idx, const double *particles, int nEvals, int Kmax, const unsigned char *evalBlocks,
                          pais_cost_detail *rec, double *weight, double *avgSad, int8_t *code, double *colour, double *H, hipStream_t stream);
// pais_load_state_batch (k_load_state): one wave per file record; record i gets key0 + i
hipError_t load_state(const DevScene &sc, const pais_loaded_patch *in, pais_patch_result *recs, int n, uint64_t key0, hipStream_t stream);
hipError_t neighbor_count(const double *centers, int n, double radius, int32_t *counts, hipStream_t stream);
hipError_t expand_image(const uint8_t *img, PaisImgT *out, size_t n, hipStream_t stream);
hipError_t level_edge_minmax(const uint8_t *img, int w, int h, unsigned long long *minmax, hipStream_t stream);
hipError_t pack_records(const pais_patch_result *recs, int n, int Kw, void *wire, hipStream_t stream);
hipError_t wire_header(void *header, const unsigned *ringCtl, int ringN, int rank, int count, int hostRc, uint32_t userWord, hipStream_t stream);

// The PSO pass of a batch: each launcher takes the scene, the view it works on (the launch goes to the view's stream) and what is its own.
hipError_t begin(const DevScene &sc, const BatchView &v, const pais_candidate *cands, int *activeList, int *activeCount);
hipError_t pso_init(const DevScene &sc, const BatchView &v, int *activeList, int *activeCount);
hipError_t pso_setup0(const DevScene &sc, const BatchView &v); // fills v.pre
// pendingOnly 1: only the particles the tile kernel flagged; 2: every particle, compared with the tile kernel's value (verify)
hipError_t pso_eval(const DevScene &sc, const BatchView &v, int pendingOnly, unsigned long long *verify);
hipError_t pso_eval_literal(const DevScene &sc, const BatchView &v);
bool tile_eligible(int Kmax);
hipError_t pso_tile(const DevScene &sc, const BatchView &v, const TileOpts &o, unsigned long long *dbg);
// v: the WHOLE batch; [listLo, listHi): positions in its active list; L: the iteration; nparts: waves per evaluation (1, 2, 4)
hipError_t pso_iter(const DevScene &sc, const BatchView &v, const int *activeList, const int *activeCount, int listLo, int listHi,
                    unsigned long long *stat, int L, int finishOnly, int nparts);
hipError_t pso_step(const DevScene &sc, const BatchView &v, unsigned long long *stat);
// k_pso_step with the trace sink and without the `pre` records
hipError_t pso_step_trace(const DevScene &sc, const BatchView &v, unsigned long long *stat, const TraceSink &t);
size_t ring_words(int n, int Nmax, int maxIt, int parts);
bool pre_ring_ok(int Kmax);
bool ring_parts_ok(int Kmax); // k_pso_ring has its part kernels (parts 2, 4) for batches of this camera count
// waves: CUs' worth of resident waves; phase 0: rings and counters prepared, 1: the launch; timeoutTicks: longest wait of a wave
// for a ring entry, in ticks of the 100 MHz s_memrealtime counter
// parts: waves per evaluation (1; 2 or 4 where ring_parts_ok)
hipError_t pso_ring(const DevScene &sc, const BatchView &v, unsigned *ring, unsigned *ctl, int *arrive, unsigned long long *stat, int waves,
                    int phase, unsigned long long timeoutTicks, int parts);
void ring_profile_print(); // (measurement builds: -DPAIS_RING_PROFILE=1)
hipError_t after(const DevScene &sc, pais_patch_result *recs, int n, double *hpScratch, int grid, int *counters,
                 unsigned long long *stat, int Kmax, double *ratios, int *nextCounters, hipStream_t stream);
// pais_ncc_batch (k_ncc_batch): one workgroup of AFTER_WAVES waves per state; ncc_lds_bytes(Kmax) of LDS for the record, the
// table and the homographies, plus Kmax*S^2 doubles of warped patches when hpInLds (else grid slabs of that size in hpScratch).
// hp_in_lds: the warped patches are small enough for LDS, as the after-stage decides it too
size_t ncc_lds_bytes(int Kmax);
bool hp_in_lds(const DevScene &sc, int Kmax);
hipError_t ncc_batch(const DevScene &sc, const pais_view_state *states, int n, pais_view_result *out, double *tables, int stride,
                     double *hpScratch, int grid, int Kmax, int hpInLds, hipStream_t stream);
// pais_test_swarm_step (include/pais_test_hooks.h): one pso_step_wave on a caller-given swarm, on the current device
int test_swarm_step(pais_test_swarm *s, double *swarm);
} // namespace pais_launch
