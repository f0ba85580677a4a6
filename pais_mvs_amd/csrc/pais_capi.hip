// pais_capi.hip -- the C ABI of include/pais_hip.h: scene upload, batch entry
// points, kernel timing.  No algorithmic fallbacks live here: every entry point
// either runs the gfx950 kernels or returns an error.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdarg.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <utility>
#include <vector>
#include <algorithm>

#include "../../include/pais_hip.h"
#include "../../include/pais_test_hooks.h"
#include "pais_dev.hpp"
#include "pais_host.hpp"
#include "pais_internal.h"

static thread_local std::string g_err;
static int fail(const char *what, hipError_t e)
{
    char buf[512];
    snprintf(buf, sizeof(buf), "%s: %s", what, hipGetErrorString(e));
    g_err = buf;
    return -2;
}
static int fail_msg(const char *what)
{
    g_err = what;
    return -1;
}
__attribute__((format(printf, 1, 2))) static int fail_fmt(const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    return fail_msg(buf);
}
#define HIPCHK(call)                                   \
    do {                                               \
        hipError_t e__ = (call);                       \
        if (e__ != hipSuccess) return fail(#call, e__); \
    } while (0)

struct EventPair {
    hipEvent_t a, b;
};

struct pais_ctx;
// brackets a region of a stream with an event pair while profiling is on (defined below)
struct Timed {
    pais_ctx *ctx = nullptr;
    hipStream_t st = nullptr;
    std::vector<EventPair> *into = nullptr;
    EventPair e{nullptr, nullptr};
    bool on = false;
    int begin(pais_ctx *c, hipStream_t s, std::vector<EventPair> *v);
    int end();
};
// kernel time, launches and items of an entry point that times each of its launches (TimedLaunch; pais_get_*_stats)
struct LaunchStats {
    double ms = 0;
    int64_t launches = 0, items = 0;
};
// The always-on timing of one region of the context's stream: an event pair from the pool around it (begin, end); once the caller
// has synchronised the stream, collect() adds the elapsed time, one launch and `items` to a LaunchStats.  The pair goes back to
// the pool when the object dies -- on every path, the early error returns included.
struct TimedLaunch {
    pais_ctx *ctx;
    EventPair e{nullptr, nullptr};
    explicit TimedLaunch(pais_ctx *c) : ctx(c) {}
    TimedLaunch(TimedLaunch &&o) noexcept : ctx(o.ctx), e(o.e) { o.e = EventPair{nullptr, nullptr}; }
    ~TimedLaunch();
    int begin();
    int end();
    void collect(LaunchStats &s, int64_t items, int64_t launches = 1);
};
// where a pais_pso_trace batch records its swarm (device buffers of one chunk; pso trace section)
struct TraceOut {
    pais_launch::TraceSink sink{nullptr, nullptr, nullptr, 1, 1};
    std::vector<TimedLaunch> passes; // the iterations of each pass
    int64_t launches = 0;            // k_pso_step_trace launches
};
// a PSO pass of a batch between pass_open and pass_close (refine batch section)
struct PassPlan {
    // what the launches of one sub-stream work on: candidates [lo, hi) as the view `v` on its stream -- or, in a k_pso_iter pass,
    // positions [lo, hi) of the active list, `v` being the whole batch on that stream
    struct Slice { int lo, hi, parts; pais_launch::BatchView v; pais_launch::TraceSink trace; };
    pais_launch::BatchView all{}; // the whole batch on the context's stream (pre: set by pass_open)
    int nSl = 0, S = 1, afterGrid = 0, itNext = 0;
    bool useIter = false, useTile = false, useRing = false, hasSeeds = false;
    bool usePre = false; // the swarm step writes the evaluations' set-up records (pais_pre.hpp): k_pso_ring / k_pso_eval2 + k_pso_step passes
    int ringParts = 1; // waves per evaluation of the ring launch (k_pso_ring's P)
    int ringCUs = 0; // CUs' worth of resident waves the ring launch may take (a part of a streamed round: its share)
    Slice sl[16];
    int *cnt = nullptr, *nextCnt = nullptr;
    const pais_candidate *d_cands = nullptr;
    Timed tp;
    TraceOut *trace = nullptr; // pais_pso_trace: the launch-per-iteration pipeline, one slice, k_pso_step_trace as the step
};

struct pais_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    int numCUs = 256;
    size_t ldsLimit = 64 * 1024;
    // the scene: DevScene holds plain views of these; a lane's copy of `sc` views its parent's and its own owners stay
    // empty, so a lane never frees its parent's scene
    DevScene sc;
    DevBuf<DevCamera> d_cams;
    DevBuf<uint8_t> d_img;
    DevBuf<PaisImgT> d_imgF;            // tap copy of d_img (element offsets identical; pais_internal.h PAIS_IMG_MODE)
    DevBuf<double> d_edge;
    bool edgesOnTheFly = false;
    DevBuf<double> d_gauss;
    size_t imgBytes = 0, edgeBytes = 0;
    std::vector<int> camMaxLod;         // host copy of every camera's max_lod (argument checks)
    // work buffers (pais_host.hpp: each knows its capacity, grows on demand through reserve(), never shrinks, and is
    // released by its destructor when pais_ctx_destroy deletes the context)
    DevBuf<pais_candidate> d_cands;     // candidates and records of pais_refine_batch: sized together with ...
    DevBuf<pais_patch_result> d_recs;
    PinBuf<pais_candidate> h_cands;     // ... their pinned staging twins
    PinBuf<pais_patch_result> h_recs;
    DevBuf<double> d_hp;
    DevBuf<double> d_ratios;            // region ratio per (candidate, visible camera) (k_region_ratio)
    DevBuf<int> d_counters;             // two sets of 4: [1] "needs another pass" count, [2] active-list length; pass p uses set
                                        // passSerial & 1, its k_after<2> clears the other one for the pass that follows
    unsigned passSerial = 0;
    bool countersDirty = false;         // a batch ended in an error: both sets are cleared before the next one
    DevBuf<unsigned char> d_evalBlocks; // per candidate: EvalPatch + EvalCam[M] (pais_eval.hpp), written by k_pso_init
    DevBuf<unsigned char> d_win;        // per candidate: the reference window WinPix[S*S] of the PSO run
    DevBuf<int> d_active;               // compacted indices of the candidates that run a PSO in the current pass
    DevBuf<unsigned long long> d_stat;  // [0] evals [1] evals*bytesPerPixel [2] patches [3] ncc tables [4] tables*K
    unsigned long long *stat = nullptr; // where the kernels count now: d_stat, or d_tStat during a pais_pso_trace call (a view)
    PinBuf<int> h_counters;
    DevBuf<unsigned char> d_psoStates;  // one PsoState block per candidate
    // PSO pass of a batch: small batches run one k_pso_iter launch per iteration (the step is replayed
    // inside the evaluation waves); batches of at least `splitAbove` evaluation waves are throughput bound and run
    // k_pso_eval2 + k_pso_step per iteration, cut into slices whose sequences overlap on separate HIP streams
    long splitAbove = 0;
    int psoMinPer = 64;
    int evalParts = 0;                  // waves per cost evaluation in k_pso_iter (1, 2, 4); 0 = chosen per slice
    double partFill = 0.5;              // ... such that parts * waves <= partFill * numCUs * 16 (= the 2 waves per SIMD that the multi-wave kernels'
                                        // 192 registers allow: they are built without an occupancy target, pais_kernels.hip PAIS_ITER_BOUNDS)
    int psoStreams = 2;
    pais_launch::TileOpts tile;         // PAIS_TILE_STRIP_SPLIT / _NOTILES
    int arithLiteral = 0;               // PAIS_ARITH=literal: the cost in the reference's own statements and summation order (pais_literal.hpp);
                                        // every batch then runs the launch-per-iteration pipeline k_pso_eval_lit + k_pso_step
    bool tileVerify = false;            // PAIS_TILE_VERIFY=1: every particle is ALSO walked by k_pso_eval2 and the two values compared (diagnosis)
    bool tileDebug = false;             // PAIS_TILE_DEBUG=1: counters of the tile kernel (printed by pais_get_kernel_stats)
    int tileMode = 1;                   // PAIS_TILE: 0 many-camera batches keep the one-wave-per-evaluation kernels; 1 the tile kernel for
                                        // scenes that tap the byte blob; 2 for every scene
    long tileAbove = 512;               // PAIS_TILE_ABOVE: waves per iteration from which a tile-eligible batch runs the tile kernel
    std::vector<hipStream_t> sub;       // sub-streams
    std::vector<hipEvent_t> subDone;
    hipEvent_t forkEv = nullptr;
    // fitness batch buffers
    DevBuf<pais_patch_state> d_states;
    DevBuf<int32_t> d_idx;
    DevBuf<double> d_particles, d_out;
    // pais_ncc_batch buffers and launch timing
    DevBuf<pais_view_state> d_vStates;
    DevBuf<pais_view_result> d_vOut;
    DevBuf<double> d_vTables, d_vHp;
    LaunchStats ncc;
    // pais_load_state_batch buffers (one chunk of file records) and launch timing
    DevBuf<pais_loaded_patch> d_lIn;
    DevBuf<pais_patch_result> d_lOut;
    LaunchStats load;
    // pais_fitness_detail buffers (one chunk of evaluations) and launch timing
    DevBuf<pais_patch_state> d_dStates;
    DevBuf<int32_t> d_dIdx;
    DevBuf<double> d_dParticles, d_dWeight, d_dSad, d_dColour, d_dH;
    DevBuf<pais_cost_detail> d_dRec;
    DevBuf<int8_t> d_dCode;
    LaunchStats detail;
    // pais_pso_trace buffers (one chunk of candidates), its own counter block for the kernels' statistics, launch timing
    DevBuf<pais_candidate> d_tCands;
    DevBuf<pais_patch_result> d_tRecs;
    DevBuf<pais_pso_run_info> d_tRuns;
    DevBuf<pais_pso_iter> d_tIters;
    DevBuf<double> d_tParts;
    DevBuf<unsigned long long> d_tStat;
    LaunchStats trace;
    // neighbour count buffers
    DevBuf<double> d_nbC;
    DevBuf<int32_t> d_nbN;
    // timing: HIP events are recorded only while profiling is on (pais_ctx_set_fine_timing); every pair is returned to
    // evFree by pais_get_kernel_stats, so the number of live events is bounded by one instrumented batch
    bool fineTiming = false;
    std::vector<EventPair> evPso, evBegin, evAfter, evEval, evEval2;
    std::vector<EventPair> evFree;
    double psoMs = 0, beginMs = 0, afterMs = 0, evalMs = 0, eval2Ms = 0;
    hipEvent_t refEv = nullptr;         // common time origin of the evEval2 intervals (recorded when fine timing is switched on; a lane uses its parent's)
    std::vector<std::pair<float, float>> eval2Intervals; // [start, end] of the drained evEval2 pairs, ms since refEv
    int64_t psoLaunches = 0, evalLaunches = 0, eval2Launches = 0, tileLaunches = 0, ringLaunches = 0;
    // lanes (pais_ctx_fork_lane): contexts over this one's scene with their own stream and work buffers
    pais_ctx *parent = nullptr;         // != nullptr: this is a lane; the scene's allocations belong to the parent
    std::vector<pais_ctx *> lanes;
    int openBatch = -1;                 // records of the batch between pais_refine_batch_begin and _end (-1: none)
    // k_pso_ring (pais_kernels.hip): the PSO pass of a large expansion batch as ONE launch over a device-side task ring
    double ringPerCam = -1.0;           // PAIS_RING_PER_CAM; unset: 540 where the ring has its part kernels -- 2700 waves per iteration (180 candidates)
                                        // at five cameras; profiles/ring_parts_ab.txt: the part ring wins from 193 candidates on, loses at 164 and below --
                                        // and 1843 with one wave per evaluation (many cameras), where it also leaves k_pso_iter's batches alone
    int ringMode = 1;                   // PAIS_PSO_RING=0: large batches take the per-iteration launches (k_pso_eval2 + k_pso_step) instead
    int preMode = 1;                    // PAIS_PRE_SETUP=0: every evaluation wave sets itself up (round 5 behaviour; A/B, tests)
    DevBuf<double> d_pre;               // per candidate and particle {status, homographies} (pais_pre.hpp)
    DevBuf<unsigned> d_ring;            // task ring
    DevBuf<unsigned> d_ringCtl;         // head, tail, done, error
    PinBuf<unsigned> h_ringCtl;         // pinned copy, read when the batch ends
    DevBuf<int> d_arrive;               // per candidate: evaluations of the current iteration that have been delivered
    bool ringUsed = false;              // by the open batch (its error words are read when the batch ends)
    bool ringSuppressed = false;        // while a batch whose ring pass failed is re-run
    bool ringSuppressOnce = false;      // the next device batch is such a re-run (pais_ctx_batch_status returned 1)
    int ringPendingN = 0;               // > 0: candidates of the pais_refine_batch_device_async batch whose ring status has not been read yet
    double ringTimeoutMs = 10000.0;     // PAIS_RING_TIMEOUT_MS: longest wait of a k_pso_ring wave for a ring entry (wall time, s_memrealtime)
    int ringPartsForced = 0;            // pais_test_set_ring_parts (tests, sweeps): waves per evaluation in k_pso_ring (1, 2, 4); 0 = chosen per pass:
    int64_t ringLaunchesByParts[3] = {0, 0, 0}; // ring launches of 1, 2, 4 waves per evaluation (pais_test_ring_parts_launches)
    double ringPartFill = 6.5;          // ... the largest such that parts * tasks <= ringPartFill * the ring's resident waves
                                        // (pawn: 4 parts up to 332 candidates, 2 up to 665; 2 parts win at 628 and lose at 712 -- ring_parts_ab.txt)
    long ringSeedAbove = 0;             // PAIS_RING_SEED_ABOVE: evaluation waves per iteration from which a pass of a SEED batch takes the ring
    size_t ringMaxBytes = (size_t)512 << 20; // PAIS_RING_MAX_MB: batches whose ring would be larger keep the per-iteration launches
    int64_t ringFallbacks = 0;          // ring passes that did not complete and were re-run through the per-iteration launches
    std::vector<EventPair> evRing;      // the ring launches alone (fine timing)
    double ringMs = 0;
    PassPlan plan;                      // of the open batch (pais_refine_batch_open .. _enqueue)
    bool planDone = true;               // the open batch is enqueued to its end
    int roundHint = 0;                  // pais_ctx_set_round_hint: candidates of the round the next batch is a part of (0: it is the round)
};

// MVS::initPatchDistanceWeighting, mvs.cpp:97-114 (host; same arithmetic as the reference)
static void build_gauss(const pais_config &cfg, std::vector<double> &g)
{
    const int S = cfg.patchSize, r = cfg.patchRadius;
    g.assign((size_t)S * S, 0.0);
    const double sigma = cfg.distWeighting;
    const double s2 = 1.0 / (2.0 * sigma * sigma);
    const double s = 1.0 / (2.0 * M_PI * sigma * sigma);
    for (int x = 0; x < S; ++x)
        for (int y = 0; y < S; ++y) {
            double e = -(pow((double)(x - r), 2) + pow((double)(y - r), 2)) * s2;
            g[(size_t)x * S + y] = s * exp(e);
        }
    double n = 0;
    for (size_t i = 0; i < g.size(); ++i) n += g[i];
    const double inv = 1.0 / n;
    for (size_t i = 0; i < g.size(); ++i) g[i] = g[i] * inv;
}

static int apply_config(pais_ctx *ctx, const pais_config *cfg)
{
    pais_config c = *cfg;
    c.patchSize = (c.patchRadius << 1) + 1; // mvs.cpp:67
    if (c.patchRadius < 1 || c.patchRadius > 127) return fail_msg("patchRadius out of range");
    if (c.particleNum < 1 || c.particleNum * 2 > PAIS_MAX_PARTICLES) return fail_msg("particleNum out of range");
    if (c.maxLOD < 0 || c.maxLOD >= PAIS_MAX_LEVELS) return fail_msg("maxLOD out of range");
    // set_lod (pais_kernels.hip) starts at minLOD - 1 and climbs while (variance < textureVariation): a negative minLOD, or a
    // threshold the comparison is never true for, leaves LOD < 0, which then indexes lodScale[], w[], h[] and imgOff[]
    if (c.minLOD < 0) return fail_msg("minLOD out of range (negative)");
    if (!(c.textureVariation > 0)) return fail_msg("textureVariation out of range (must be > 0)");
    // lodScale[l] = lodRatio^l scales the projections and homographies of level l and is inverted with them
    if (!(c.lodRatio > 0 && c.lodRatio < 1)) return fail_msg("lodRatio out of range (must be inside (0, 1))");
    // the inertia weight of a PSO run steps by 1 / maxIteration, and the trace rows of a run are sized by it
    if (c.maxIteration < 1) return fail_msg("maxIteration out of range (must be >= 1)");
    // the expansion driver divides image coordinates by cellSize (pais_mvs.hip slotCell, setCellMaps)
    if (c.cellSize < 1) return fail_msg("cellSize out of range (must be >= 1)");
    std::vector<double> g;
    build_gauss(c, g);
    if (ctx->d_gauss) HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx->d_gauss.alloc(g.size() * sizeof(double)));
    HIPCHK(hipMemcpy(ctx->d_gauss, g.data(), g.size() * sizeof(double), hipMemcpyHostToDevice));
    ctx->sc.cfg = c;
    ctx->sc.gauss = ctx->d_gauss;
    for (int l = 0; l < PAIS_MAX_LEVELS; ++l) ctx->sc.lodScale[l] = pow(c.lodRatio, l);
    return 0;
}

extern "C" const char *pais_last_error(void) { return g_err.c_str(); }
extern "C" size_t pais_sizeof_config(void) { return sizeof(pais_config); }
extern "C" size_t pais_sizeof_camera_desc(void) { return sizeof(pais_camera_desc); }
extern "C" size_t pais_sizeof_candidate(void) { return sizeof(pais_candidate); }
extern "C" size_t pais_sizeof_patch_result(void) { return sizeof(pais_patch_result); }
extern "C" size_t pais_sizeof_view_state(void) { return sizeof(pais_view_state); }
extern "C" size_t pais_sizeof_view_result(void) { return sizeof(pais_view_result); }
extern "C" size_t pais_sizeof_cost_detail(void) { return sizeof(pais_cost_detail); }
extern "C" size_t pais_sizeof_pso_run_info(void) { return sizeof(pais_pso_run_info); }
extern "C" size_t pais_sizeof_pso_iter(void) { return sizeof(pais_pso_iter); }
static_assert(offsetof(pais_pso_run_info, range_u) == 24 && offsetof(pais_pso_run_info, init) == 48 && offsetof(pais_pso_run_info, ray) == 72 &&
              offsetof(pais_pso_run_info, run) == 96 && offsetof(pais_pso_run_info, n_particles) == 112 &&
              offsetof(pais_pso_run_info, iterations) == 120 && offsetof(pais_pso_run_info, cam_idx) == 128 &&
              sizeof(pais_pso_run_info) == 128 + 4 * PAIS_MAX_VIS, "pais_pso_run_info layout");
static_assert(offsetof(pais_pso_iter, gbest) == 8 && offsetof(pais_pso_iter, iw) == 32 && offsetof(pais_pso_iter, dispersion) == 40 &&
              offsetof(pais_pso_iter, velocity) == 48 && offsetof(pais_pso_iter, g_idx) == 56 && offsetof(pais_pso_iter, ended) == 64 &&
              sizeof(pais_pso_iter) == 72, "pais_pso_iter layout");
extern "C" uint32_t pais_rand31(uint64_t seed, uint64_t key, uint32_t run, uint32_t k) { return pais::rand31(seed, key, run, k); }
extern "C" uint64_t pais_child_key(uint64_t parent_key, int cam, int cx, int cy) { return pais::child_key(parent_key, cam, cx, cy); }

static int ctx_init(pais_ctx *ctx, const pais_config *cfg, int num_cams, const pais_camera_desc *cams, int device, uint64_t pso_seed);
static int ctx_init_work(pais_ctx *ctx);
extern "C" int pais_ctx_create(const pais_config *cfg, int num_cams, const pais_camera_desc *cams, int device,
                               uint64_t pso_seed, pais_ctx **out)
{
    if (!cfg || !cams || !out || num_cams <= 0) return fail_msg("pais_ctx_create: bad argument");
    int ndev = 0;
    hipError_t e0 = hipGetDeviceCount(&ndev);
    if (e0 != hipSuccess || ndev <= 0) return fail_msg("pais_ctx_create: no HIP device (this library has no CPU path)");
    if (device < 0 || device >= ndev) return fail_msg("pais_ctx_create: bad device index");
    HIPCHK(hipSetDevice(device));
    pais_ctx *ctx = new pais_ctx();
    // every failure below -- a validation message or a HIP error, e.g. the allocation of a multi-GB blob -- leaves through
    // ctx_init's return value; what had been created by then is released here
    const int rc = ctx_init(ctx, cfg, num_cams, cams, device, pso_seed);
    if (rc) { pais_ctx_destroy(ctx); return rc; }
    *out = ctx;
    return 0;
}

static int ctx_init(pais_ctx *ctx, const pais_config *cfg, int num_cams, const pais_camera_desc *cams, int device, uint64_t pso_seed)
{
    ctx->device = device;
    memset(&ctx->sc, 0, sizeof(ctx->sc));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    ctx->numCUs = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    ctx->ldsLimit = prop.sharedMemPerBlock > 0 ? (size_t)prop.sharedMemPerBlock : 64 * 1024;
    HIPCHK(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
    ctx->sc.seed = pso_seed;
    ctx->sc.numCams = num_cams;
    int rc = apply_config(ctx, cfg);
    if (rc) return rc;
    const bool wantEdge = cfg->adaptiveGradientEnable != 0;
    // edge pyramids: as the caller built them (Camera::pyramidEdge, camera.cpp:72-77,87-91), or -- level_edge == NULL --
    // evaluated on the fly from the gray levels with the same statements (no double-precision copy of every pyramid)
    const bool edgesGiven = wantEdge && cams[0].level_edge[0] != nullptr;

    // layout the blobs
    std::vector<DevCamera> hc((size_t)num_cams);
    std::vector<size_t> imgOff((size_t)num_cams * PAIS_MAX_LEVELS, 0), edgeOff((size_t)num_cams * PAIS_MAX_LEVELS, 0);
    size_t imgBytes = 0, edgeBytes = 0;
    for (int c = 0; c < num_cams; ++c) {
        const pais_camera_desc &d = cams[c];
        if (d.max_lod < 0 || d.max_lod >= PAIS_MAX_LEVELS) return fail_msg("camera max_lod out of range");
        for (int l = 0; l <= d.max_lod; ++l) {
            if (!d.level_image[l] || d.level_width[l] <= 0 || d.level_height[l] <= 0) return fail_msg("camera level missing");
            // the evaluation packs a level's tap bounds (w - 4, h - 4) into 16 bits each and its row offsets into 24 (pais_eval.hpp)
            if (d.level_width[l] > 65535 || d.level_height[l] > 65535) return fail_msg("camera level larger than 65535 pixels in one dimension");
            size_t px = (size_t)d.level_width[l] * d.level_height[l];
            if (px >= ((size_t)1 << 29)) return fail_msg("camera level of 2^29 pixels or more (32-bit tap offsets inside a level)");
            imgOff[(size_t)c * PAIS_MAX_LEVELS + l] = imgBytes;
            imgBytes = (imgBytes + px + 16 + 255) & ~(size_t)255; // +16: taps read (px+1, py+1)
            if (wantEdge && edgesGiven) {
                if (!d.level_edge[l]) return fail_msg("level_edge given for some levels only");
                edgeOff[(size_t)c * PAIS_MAX_LEVELS + l] = edgeBytes;
                edgeBytes = (edgeBytes + px * sizeof(double) + 255) & ~(size_t)255;
            }
        }
    }
    // pyramid levels straight from the caller's buffers into HBM (rows repacked to stride == width); the padding between
    // levels is zero
    if (imgBytes >= ((size_t)1 << 40)) return fail_msg("pyramids of 2^40 bytes or more (a level's start is packed into 40 bits next to its homography)");
    HIPCHK(ctx->d_img.alloc(imgBytes));
    HIPCHK(hipMemsetAsync(ctx->d_img, 0, imgBytes, ctx->stream));
    for (int c = 0; c < num_cams; ++c) {
        const pais_camera_desc &d = cams[c];
        for (int l = 0; l <= d.max_lod; ++l) {
            const int w = d.level_width[l], h = d.level_height[l];
            const size_t stride = d.level_stride[l] > 0 ? (size_t)d.level_stride[l] : (size_t)w;
            HIPCHK(hipMemcpy2DAsync(ctx->d_img + imgOff[(size_t)c * PAIS_MAX_LEVELS + l], (size_t)w, d.level_image[l], stride, (size_t)w,
                                    (size_t)h, hipMemcpyHostToDevice, ctx->stream));
        }
    }
    ctx->imgBytes = imgBytes;
    // the float2 tap copy is expanded on the device -- for scenes whose pyramids are small enough for it to pay
    // (pais_internal.h PaisImgT); larger scenes tap the byte blob
    {
        size_t maxMB = 256;
        if (const char *e = getenv("PAIS_TAP_FLOAT_MAX_MB")) maxMB = (size_t)strtoull(e, nullptr, 10);
        if (imgBytes <= (maxMB << 20)) {
            HIPCHK(ctx->d_imgF.alloc(imgBytes * sizeof(PaisImgT)));
            HIPCHK(pais_launch::expand_image(ctx->d_img, ctx->d_imgF, imgBytes, ctx->stream));
        }
    }
    if (wantEdge && edgesGiven && edgeBytes) {
        HIPCHK(ctx->d_edge.alloc(edgeBytes));
        for (int c = 0; c < num_cams; ++c) {
            const pais_camera_desc &d = cams[c];
            for (int l = 0; l <= d.max_lod; ++l) {
                size_t px = (size_t)d.level_width[l] * d.level_height[l];
                HIPCHK(hipMemcpyAsync((uint8_t *)ctx->d_edge.p + edgeOff[(size_t)c * PAIS_MAX_LEVELS + l], d.level_edge[l],
                                      px * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
            }
        }
        ctx->edgeBytes = edgeBytes;
    }
    // edge maps on the fly (level_edge == NULL): only the per-level minimum / maximum magnitude is precomputed
    std::vector<unsigned long long> mm;
    if (wantEdge && !edgesGiven) {
        mm.assign((size_t)num_cams * PAIS_MAX_LEVELS * 2, 0ULL);
        for (size_t i = 0; i < mm.size(); i += 2) mm[i] = ~0ULL;
        DevBuf<unsigned long long> d_mm; // released on every path
        HIPCHK(d_mm.alloc(mm.size() * sizeof(unsigned long long)));
        HIPCHK(hipMemcpyAsync(d_mm, mm.data(), mm.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, ctx->stream));
        for (int c = 0; c < num_cams; ++c)
            for (int l = 0; l <= cams[c].max_lod; ++l)
                HIPCHK(pais_launch::level_edge_minmax(ctx->d_img + imgOff[(size_t)c * PAIS_MAX_LEVELS + l], cams[c].level_width[l],
                                                      cams[c].level_height[l], d_mm + ((size_t)c * PAIS_MAX_LEVELS + l) * 2, ctx->stream));
        HIPCHK(hipMemcpyAsync(mm.data(), d_mm, mm.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->edgesOnTheFly = wantEdge && !edgesGiven;
    for (int c = 0; c < num_cams; ++c) {
        const pais_camera_desc &d = cams[c];
        DevCamera &h = hc[c];
        memset(&h, 0, sizeof(h));
        memcpy(h.KR, d.KR, sizeof(h.KR));
        memcpy(h.KT, d.KT, sizeof(h.KT));
        memcpy(h.R, d.rotation, sizeof(h.R));
        memcpy(h.T, d.translation, sizeof(h.T));
        memcpy(h.C, d.center, sizeof(h.C));
        memcpy(h.optN, d.optical_normal, sizeof(h.optN));
        h.focal[0] = d.focal[0]; h.focal[1] = d.focal[1];
        h.pp[0] = d.principle_point[0]; h.pp[1] = d.principle_point[1];
        h.maxLOD = d.max_lod;
        ctx->camMaxLod.push_back(d.max_lod);
        for (int l = 0; l <= d.max_lod; ++l) {
            h.w[l] = d.level_width[l];
            h.h[l] = d.level_height[l];
            h.imgOff[l] = (uint64_t)imgOff[(size_t)c * PAIS_MAX_LEVELS + l];
            h.edgeOff[l] = (uint64_t)(edgeOff[(size_t)c * PAIS_MAX_LEVELS + l] / sizeof(double));
            if (!mm.empty()) {
                const unsigned long long lo = mm[((size_t)c * PAIS_MAX_LEVELS + l) * 2], hi = mm[((size_t)c * PAIS_MAX_LEVELS + l) * 2 + 1];
                memcpy(&h.edgeMin[l], &lo, 8);
                memcpy(&h.edgeMax[l], &hi, 8);
            }
        }
    }
    HIPCHK(ctx->d_cams.alloc(sizeof(DevCamera) * (size_t)num_cams));
    HIPCHK(hipMemcpy(ctx->d_cams, hc.data(), sizeof(DevCamera) * (size_t)num_cams, hipMemcpyHostToDevice));
    ctx->sc.cams = ctx->d_cams;
    ctx->sc.imgBlob = ctx->d_img;
    ctx->sc.imgF = ctx->d_imgF;
    ctx->sc.edgeBlob = ctx->d_edge;

    return ctx_init_work(ctx);
}

// Environment knobs.  An unset variable, or a value outside the knob's range, leaves the default -- silently.
template <typename T> static void env_int(const char *name, T &v, long lo = LONG_MIN, long hi = LONG_MAX)
{
    const char *e = getenv(name);
    if (!e) return;
    const long x = atol(e);
    if (x >= lo && x <= hi) v = (T)x;
}
template <typename T> static void env_flag(const char *name, T &v)
{
    if (const char *e = getenv(name)) v = atoi(e) != 0;
}
static void env_real(const char *name, double &v, bool positiveOnly = false)
{
    const char *e = getenv(name);
    if (!e) return;
    const double x = atof(e);
    if (!positiveOnly || x > 0) v = x;
}
// items per chunk of an entry point whose staging buffers stay within `envName` MB (PAIS_*_STAGING_MB, default 256): of n
// items of perItemBytes each, one at least
static int staging_chunk(const char *envName, int n, size_t perItemBytes)
{
    double mb = 256.0;
    env_real(envName, mb);
    const size_t bound = (size_t)std::max(0.0, mb * 1048576.0);
    return (int)std::min((size_t)n, std::max((size_t)1, bound / perItemBytes));
}

// everything of a context that is not the scene: counters, statistics, knobs, sub-streams (a lane has its own)
static int ctx_init_work(pais_ctx *ctx)
{
    HIPCHK(ctx->d_counters.alloc(sizeof(int) * 8));
    HIPCHK(hipMemset(ctx->d_counters, 0, sizeof(int) * 8));
    HIPCHK(ctx->d_stat.alloc(sizeof(unsigned long long) * 24));
    HIPCHK(hipMemset(ctx->d_stat, 0, sizeof(unsigned long long) * 24));
    ctx->stat = ctx->d_stat;
    HIPCHK(ctx->h_counters.alloc(sizeof(int) * 4));
    HIPCHK(ctx->d_ringCtl.alloc(PAIS_RING_CTL_BYTES * PAIS_RINGS));
    HIPCHK(hipMemset(ctx->d_ringCtl, 0, PAIS_RING_CTL_BYTES * PAIS_RINGS));
    HIPCHK(ctx->h_ringCtl.alloc(PAIS_RING_CTL_BYTES * PAIS_RINGS));
    memset(ctx->h_ringCtl, 0, PAIS_RING_CTL_BYTES * PAIS_RINGS);
    // knob, field, accepted range (the fields' initialisers in pais_ctx are the defaults)
    ctx->splitAbove = 3L * ctx->numCUs * 12;
    env_int("PAIS_EVAL_PARTS", ctx->evalParts, 1, 4);
    if (ctx->evalParts == 3) ctx->evalParts = 0; // (1, 2 or 4)
    env_real("PAIS_PART_FILL", ctx->partFill, true);
    env_int("PAIS_SPLIT_ABOVE", ctx->splitAbove, 1);
    env_int("PAIS_PSO_MINPER", ctx->psoMinPer, 1, INT_MAX);
    env_int("PAIS_PSO_STREAMS", ctx->psoStreams, 1, 16);
    env_int("PAIS_PSO_RING", ctx->ringMode, INT_MIN, INT_MAX);
    env_int("PAIS_PRE_SETUP", ctx->preMode, INT_MIN, INT_MAX);
    {
        double v = -1.0;
        env_real("PAIS_RING_PER_CAM", v);
        if (v >= 0) ctx->ringPerCam = v;
    }
    // (0 = never, the default: measured on the pawn bench, profiles/r04_seed_ring_ab.txt -- the first pass of the 200 seeds as one
    //  ring launch costs +3.5 ms per reconstruction against k_pso_iter's 2 x 62 launches: with 2N = 30 particles the one-wave
    //  swarm step is a long serial chain between two evaluations of a candidate, and 6000 tasks per iteration are two residency
    //  passes, so the chain of 61 iterations -- not the throughput -- bounds the launch)
    env_int("PAIS_RING_SEED_ABOVE", ctx->ringSeedAbove);
    long ringMaxMB = 0;
    env_int("PAIS_RING_MAX_MB", ringMaxMB, 1);
    if (ringMaxMB) ctx->ringMaxBytes = (size_t)ringMaxMB << 20;
    env_int("PAIS_TILE", ctx->tileMode, INT_MIN, INT_MAX);
    env_flag("PAIS_TILE_DEBUG", ctx->tileDebug);
    env_flag("PAIS_TILE_VERIFY", ctx->tileVerify);
    env_int("PAIS_TILE_STRIP_SPLIT", ctx->tile.stripSteps, 1, INT_MAX);
    env_flag("PAIS_TILE_NOTILES", ctx->tile.noTiles);
    env_int("PAIS_TILE_ABOVE", ctx->tileAbove, 1);
    env_flag("PAIS_FINE_TIMING", ctx->fineTiming);
    if (const char *e = getenv("PAIS_ARITH")) ctx->arithLiteral = (strcmp(e, "literal") == 0);
    if (const char *e = getenv("PAIS_RING_TIMEOUT_MS")) {
        // 0 is the tests' hook (every ring pass "times out" and is re-run launch by launch); anything else must be a finite wait
        // of at least a millisecond and at most ten minutes -- negative / NaN values are ignored
        const double v = atof(e);
        if (v == 0.0 && e[0] == '0') ctx->ringTimeoutMs = 0.0;
        else if (v >= 1.0 && v <= 600000.0) ctx->ringTimeoutMs = v;
        else fprintf(stderr, "pais: PAIS_RING_TIMEOUT_MS=%s ignored (0, or 1 .. 600000 ms)\n", e);
    }
    HIPCHK(hipEventCreateWithFlags(&ctx->forkEv, hipEventDisableTiming));
    for (int i = 0; i + 1 < ctx->psoStreams; ++i) { // slice 0 runs on ctx->stream itself
        hipStream_t st; hipEvent_t ev;
        HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        ctx->sub.push_back(st);
        ctx->subDone.push_back(ev);
    }
    return 0;
}

extern "C" void pais_ctx_destroy(pais_ctx *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->parent) { // a lane destroyed on its own: the parent forgets it
        auto &v = ctx->parent->lanes;
        for (size_t i = 0; i < v.size(); ++i)
            if (v[i] == ctx) { v.erase(v.begin() + (long)i); break; }
        ctx->parent = nullptr;
    }
    while (!ctx->lanes.empty()) {
        pais_ctx *l = ctx->lanes.back();
        ctx->lanes.pop_back();
        l->parent = nullptr;
        pais_ctx_destroy(l);
    }
    // the frees: every buffer is a member that releases itself in `delete ctx` below -- with the context's device current
    // (set above; a lane shares its parent's) and after this synchronisation of the context's stream, which every use of
    // the buffers is ordered before (pais_host.hpp reserve()).  They come after hipStreamDestroy: the frees
    // take no stream, and nothing is pending on one that has just been synchronised.
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    for (auto *v : {&ctx->evPso, &ctx->evBegin, &ctx->evAfter, &ctx->evEval, &ctx->evEval2, &ctx->evRing, &ctx->evFree})
        for (auto &p : *v) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
    for (auto st : ctx->sub) (void)hipStreamDestroy(st);
    for (auto ev : ctx->subDone) (void)hipEventDestroy(ev);
    if (ctx->forkEv) (void)hipEventDestroy(ctx->forkEv);
    if (ctx->refEv) (void)hipEventDestroy(ctx->refEv);
    pais_launch::ring_profile_print();
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

extern "C" int pais_ctx_set_config(pais_ctx *ctx, const pais_config *cfg)
{
    if (!ctx || !cfg) return fail_msg("pais_ctx_set_config: bad argument");
    HIPCHK(hipSetDevice(ctx->device));
    if (cfg->adaptiveGradientEnable && !ctx->d_edge && !ctx->edgesOnTheFly)
        return fail_msg("adaptiveGradientEnable needs the gradient weighting enabled at create time (edge pyramids or their on-the-fly statistics)");
    if (ctx->parent) return fail_msg("pais_ctx_set_config: a lane takes its configuration from its parent");
    // (an open batch's buffers and launch plan are sized from the configuration it was opened with)
    if (ctx->openBatch >= 0) return fail_msg("pais_ctx_set_config: a batch is open on this context");
    for (pais_ctx *l : ctx->lanes)
        if (l->openBatch >= 0) return fail_msg("pais_ctx_set_config: a batch is open on a lane of this context");
    for (pais_ctx *l : ctx->lanes) HIPCHK(hipStreamSynchronize(l->stream)); // (the table is reallocated)
    int rc = apply_config(ctx, cfg);
    if (rc) return rc;
    for (pais_ctx *l : ctx->lanes) {
        l->sc.cfg = ctx->sc.cfg;
        l->sc.gauss = ctx->sc.gauss;
        for (int i = 0; i < PAIS_MAX_LEVELS; ++i) l->sc.lodScale[i] = ctx->sc.lodScale[i];
    }
    return 0;
}

extern "C" int pais_ctx_fork_lane(pais_ctx *parent, pais_ctx **out)
{
    if (!parent || !out) return fail_msg("pais_ctx_fork_lane: bad argument");
    if (parent->parent) return fail_msg("pais_ctx_fork_lane: a lane cannot be forked");
    HIPCHK(hipSetDevice(parent->device));
    pais_ctx *l = new pais_ctx();
    l->device = parent->device;
    l->numCUs = parent->numCUs;
    l->ldsLimit = parent->ldsLimit;
    l->camMaxLod = parent->camMaxLod;
    l->sc = parent->sc; // the parent's cameras, blobs and table: shared, not owned (d_cams, d_img ... stay null here)
    l->edgesOnTheFly = parent->edgesOnTheFly;
    l->imgBytes = parent->imgBytes;
    l->edgeBytes = parent->edgeBytes;
    hipError_t e = hipStreamCreateWithFlags(&l->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete l; return fail("hipStreamCreateWithFlags", e); }
    const int rc = ctx_init_work(l);
    if (rc) { pais_ctx_destroy(l); return rc; }
    l->fineTiming = parent->fineTiming;
    l->ringPartsForced = parent->ringPartsForced;
    l->ringPartFill = parent->ringPartFill;
    l->parent = parent;
    parent->lanes.push_back(l);
    *out = l;
    return 0;
}

extern "C" int pais_ctx_set_neighbor_radius(pais_ctx *ctx, double r)
{
    if (!ctx) return fail_msg("bad ctx");
    ctx->sc.cfg.neighborRadius = r;
    for (pais_ctx *l : ctx->lanes) l->sc.cfg.neighborRadius = r;
    return 0;
}

extern "C" void *pais_ctx_stream(pais_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }
extern "C" int pais_ctx_synchronize(pais_ctx *ctx)
{
    if (!ctx) return fail_msg("bad ctx");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
}

// ------------------------------------------------------------------- timing --
static int get_event_pair(pais_ctx *ctx, EventPair &p)
{
    if (!ctx->evFree.empty()) {
        p = ctx->evFree.back();
        ctx->evFree.pop_back();
        return 0;
    }
    EventPair q{nullptr, nullptr}; // (p stays as it was behind a failure)
    HIPCHK(hipEventCreate(&q.a));
    const hipError_t e = hipEventCreate(&q.b);
    if (e != hipSuccess) { (void)hipEventDestroy(q.a); return fail("hipEventCreate", e); }
    p = q;
    return 0;
}
static int drain_events(pais_ctx *ctx, std::vector<EventPair> &v, double &acc)
{
    for (auto &p : v) {
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, p.a, p.b));
        acc += ms;
        ctx->evFree.push_back(p);
    }
    v.clear();
    return 0;
}
int Timed::begin(pais_ctx *c, hipStream_t s, std::vector<EventPair> *v)
{
    ctx = c; st = s; into = v; on = c->fineTiming;
    if (!on) return 0;
    if (get_event_pair(c, e)) return -2;
    HIPCHK(hipEventRecord(e.a, s));
    return 0;
}
int Timed::end()
{
    if (!on) return 0;
    HIPCHK(hipEventRecord(e.b, st));
    into->push_back(e);
    return 0;
}

TimedLaunch::~TimedLaunch()
{
    if (e.a) ctx->evFree.push_back(e);
}
int TimedLaunch::begin()
{
    if (get_event_pair(ctx, e)) return -2;
    HIPCHK(hipEventRecord(e.a, ctx->stream));
    return 0;
}
int TimedLaunch::end()
{
    HIPCHK(hipEventRecord(e.b, ctx->stream));
    return 0;
}
void TimedLaunch::collect(LaunchStats &s, int64_t items, int64_t launches)
{
    float ms = 0;
    if (hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess) s.ms += ms;
    s.launches += launches;
    s.items += items;
}

// the pais_get_{ncc,detail,trace,load}_stats entry points (s == nullptr: the context was)
static int read_launch_stats(LaunchStats *s, const char *who, double *kernel_ms, int64_t *launches, int64_t *items, int reset)
{
    if (!s) return fail_fmt("%s: bad argument", who);
    if (kernel_ms) *kernel_ms = s->ms;
    if (launches) *launches = s->launches;
    if (items) *items = s->items;
    if (reset) *s = LaunchStats();
    return 0;
}

// ---------------------------------------------------------- argument checks --
// The camera list of one item of a batch -- a pais_patch_state, a pais_view_state or a pais_candidate -- against the scene.
// Every entry point states its rules once, side by side below; a refused item is named in pais_last_error() with the entry
// point, its index and the offending value.  All of it runs before anything is enqueued: a rejected call leaves the
// context as it was.
struct CamListRules {
    const char *who, *noun; // the entry point; what an item is called in its messages
    int minCam;             // num_cam in [minCam, PAIS_MAX_VIS]
    bool distinct;          // a camera listed twice is refused
    enum Ref {
        NoRef,    // the item has no ref_cam / lod
        AnyLevel, // ref_cam is a camera, lod in [0, PAIS_MAX_LEVELS)
        OwnLevels // ref_cam is a camera, lod in [0, least max_lod of ref_cam and the listed cameras]
    } ref;
};
static const CamListRules kFitnessRules = {"pais_fitness_batch", "state", 1, false, CamListRules::AnyLevel};
static const CamListRules kDetailRules = {"pais_fitness_detail", "state", 1, false, CamListRules::AnyLevel};
static const CamListRules kNccRules = {"pais_ncc_batch", "state", 2, true, CamListRules::OwnLevels};
static CamListRules candidate_rules(const char *who) { return CamListRules{who, "candidate", 0, false, CamListRules::NoRef}; }

static int check_cam_list(const pais_ctx *ctx, const CamListRules &R, int i, int num_cam, const int32_t *cam_idx, int ref_cam, int lod)
{
    const int nc = ctx->sc.numCams;
    if (num_cam < R.minCam || num_cam > PAIS_MAX_VIS)
        return fail_fmt("%s: %s %d: num_cam %d outside [%d, %d]", R.who, R.noun, i, num_cam, R.minCam, PAIS_MAX_VIS);
    if (R.ref != CamListRules::NoRef && (ref_cam < 0 || ref_cam >= nc))
        return fail_fmt("%s: %s %d: ref_cam %d out of range [0, %d)", R.who, R.noun, i, ref_cam, nc);
    for (int k = 0; k < num_cam; ++k) {
        const int c = cam_idx[k];
        bool twice = false;
        for (int j = 0; R.distinct && j < k; ++j) twice = twice || cam_idx[j] == c;
        if (c >= 0 && c < nc && !twice) continue;
        if (R.distinct) // (two reasons: the reason first)
            return fail_fmt("%s: %s %d: %s (cam_idx[%d] = %d)", R.who, R.noun, i, c < 0 || c >= nc ? "cam_idx out of range" : "duplicate camera in cam_idx",
                            k, c);
        return fail_fmt("%s: %s %d: cam_idx[%d] = %d out of range [0, %d)", R.who, R.noun, i, k, c, nc);
    }
    if (R.ref == CamListRules::AnyLevel && (lod < 0 || lod >= PAIS_MAX_LEVELS))
        return fail_fmt("%s: %s %d: lod %d outside [0, %d)", R.who, R.noun, i, lod, PAIS_MAX_LEVELS);
    if (R.ref == CamListRules::OwnLevels) {
        int maxLod = ctx->camMaxLod[ref_cam], lim = ref_cam;
        for (int k = 0; k < num_cam; ++k)
            if (ctx->camMaxLod[cam_idx[k]] < maxLod) {
                maxLod = ctx->camMaxLod[cam_idx[k]];
                lim = cam_idx[k];
            }
        if (lod < 0 || lod > maxLod)
            return fail_fmt("%s: %s %d: lod %d outside [0, %d] (max_lod of camera %d)", R.who, R.noun, i, lod, maxLod, lim);
    }
    return 0;
}

// the states and state indices of pais_fitness_batch / pais_fitness_detail; Kmax: the largest num_cam
static int check_states(const pais_ctx *ctx, const CamListRules &R, int n_states, const pais_patch_state *states, int n_evals,
                        const int32_t *state_index, int &Kmax)
{
    Kmax = 1;
    for (int i = 0; i < n_states; ++i) {
        const pais_patch_state &s = states[i];
        const int rc = check_cam_list(ctx, R, i, s.num_cam, s.cam_idx, s.ref_cam, s.lod);
        if (rc) return rc;
        Kmax = std::max(Kmax, (int)s.num_cam);
    }
    for (int e = 0; e < n_evals; ++e)
        if (state_index[e] < 0 || state_index[e] >= n_states)
            return fail_fmt("%s: state_index[%d] = %d out of range [0, %d)", R.who, e, state_index[e], n_states);
    return 0;
}

// the candidates of pais_refine_batch_open / pais_pso_trace / pais_pso_trace_shape; Kmax: the largest num_cam, hasSeeds: any seed
static int check_candidates(const pais_ctx *ctx, const char *who, int n, const pais_candidate *cands, int &Kmax, int &hasSeeds)
{
    const CamListRules R = candidate_rules(who);
    Kmax = 1;
    hasSeeds = 0;
    for (int i = 0; i < n; ++i) {
        const pais_candidate &c = cands[i];
        const int rc = check_cam_list(ctx, R, i, c.num_cam, c.cam_idx, 0, 0);
        if (rc) return rc;
        if (c.type != PAIS_TYPE_SEED && c.type != PAIS_TYPE_EXPAND)
            return fail_fmt("%s: candidate %d: type %d is neither PAIS_TYPE_SEED nor PAIS_TYPE_EXPAND", who, i, c.type);
        Kmax = std::max(Kmax, (int)c.num_cam);
        if (c.type == PAIS_TYPE_SEED) hasSeeds = 1;
    }
    return 0;
}

// MVS::neighborPatchFiltering's distance counts (mvs.cpp:448-524) -- see k_neighbor_count
extern "C" int pais_neighbor_count(pais_ctx *ctx, int n, const double *centers, double radius, int32_t *counts, double *kernel_ms)
{
    if (!ctx || n < 0 || (n && (!centers || !counts))) return fail_msg("pais_neighbor_count: bad argument");
    if (kernel_ms) *kernel_ms = 0;
    if (n == 0) return 0;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(ctx->d_nbC.reserve(ctx->stream, sizeof(double) * 3 * (size_t)n));
    HIPCHK(ctx->d_nbN.reserve(ctx->stream, sizeof(int32_t) * (size_t)n));
    HIPCHK(hipMemcpyAsync(ctx->d_nbC, centers, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    TimedLaunch t(ctx);
    if (t.begin()) return -2;
    HIPCHK(pais_launch::neighbor_count(ctx->d_nbC, n, radius, ctx->d_nbN, ctx->stream));
    if (t.end()) return -2;
    HIPCHK(hipMemcpyAsync(counts, ctx->d_nbN, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    LaunchStats s;
    t.collect(s, n);
    if (kernel_ms) *kernel_ms = s.ms;
    return 0;
}

extern "C" int pais_ctx_set_fine_timing(pais_ctx *ctx, int on)
{
    if (!ctx) return fail_msg("pais_ctx_set_fine_timing: bad argument");
    if (on && !ctx->parent) {
        HIPCHK(hipSetDevice(ctx->device));
        if (!ctx->refEv) HIPCHK(hipEventCreate(&ctx->refEv));
        HIPCHK(hipEventRecord(ctx->refEv, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    ctx->fineTiming = on != 0;
    for (pais_ctx *l : ctx->lanes) l->fineTiming = on != 0;
    return 0;
}

// ------------------------------------------------------------ fitness batch --
extern "C" int pais_fitness_batch(pais_ctx *ctx, int n_states, const pais_patch_state *states, int n_evals,
                                  const int32_t *state_index, const double *particles, double *out)
{
    if (!ctx || n_states < 0 || n_evals < 0) return fail_msg("pais_fitness_batch: bad argument");
    if (n_evals == 0) return 0;
    if (!states || !state_index || !particles || !out) return fail_msg("pais_fitness_batch: null pointer");
    HIPCHK(hipSetDevice(ctx->device));
    int Kmax = 1;
    const int rc = check_states(ctx, kFitnessRules, n_states, states, n_evals, state_index, Kmax);
    if (rc) return rc;
    HIPCHK(ctx->d_states.reserve(ctx->stream, sizeof(pais_patch_state) * (size_t)n_states));
    HIPCHK(ctx->d_idx.reserve(ctx->stream, sizeof(int32_t) * (size_t)n_evals));
    HIPCHK(ctx->d_particles.reserve(ctx->stream, sizeof(double) * 3 * (size_t)n_evals));
    HIPCHK(ctx->d_out.reserve(ctx->stream, sizeof(double) * (size_t)n_evals));
    HIPCHK(ctx->d_evalBlocks.reserve(ctx->stream, pais_launch::eval_block_bytes_host(Kmax) * (size_t)n_states));
    HIPCHK(ctx->d_win.reserve(ctx->stream, pais_launch::win_bytes_per_candidate(ctx->sc) * (size_t)n_states));
    HIPCHK(hipMemcpyAsync(ctx->d_states, states, sizeof(pais_patch_state) * (size_t)n_states, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->d_idx, state_index, sizeof(int32_t) * (size_t)n_evals, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->d_particles, particles, sizeof(double) * 3 * (size_t)n_evals, hipMemcpyHostToDevice, ctx->stream));
    Timed tf;
    if (tf.begin(ctx, ctx->stream, &ctx->evEval)) return -2; // kernel-only time, reported as eval_ms / eval_launches
    HIPCHK(pais_launch::fitness(ctx->sc, ctx->d_states, n_states, ctx->d_idx, ctx->d_particles, ctx->d_out, n_evals, Kmax,
                                ctx->d_evalBlocks, ctx->d_win, ctx->arithLiteral, ctx->stream));
    if (tf.end()) return -2;
    ctx->evalLaunches++;
    HIPCHK(hipMemcpyAsync(out, ctx->d_out, sizeof(double) * (size_t)n_evals, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
}

// ---------------------------------------------------------------- ncc batch --
// Patch::removeInvisibleCamera of caller-given states (k_ncc_batch)
extern "C" int pais_ncc_batch(pais_ctx *ctx, int n, const pais_view_state *states, pais_view_result *out, double *tables, int stride)
{
    if (!ctx || n < 0) return fail_msg("pais_ncc_batch: bad argument");
    if (n == 0) return 0;
    if (!states || !out) return fail_msg("pais_ncc_batch: null pointer");
    if (tables && stride < 2) return fail_msg("pais_ncc_batch: table stride below 2");
    int Kmax = 2;
    for (int i = 0; i < n; ++i) {
        const pais_view_state &v = states[i];
        const int rc = check_cam_list(ctx, kNccRules, i, v.num_cam, v.cam_idx, v.ref_cam, v.lod);
        if (rc) return rc;
        if (tables && stride < v.num_cam) return fail_fmt("pais_ncc_batch: state %d: table stride %d below num_cam %d", i, stride, v.num_cam);
        Kmax = std::max(Kmax, (int)v.num_cam);
    }
    HIPCHK(hipSetDevice(ctx->device));
    const DevScene &sc = ctx->sc;
    const size_t hpBytes = sizeof(double) * (size_t)Kmax * sc.cfg.patchSize * sc.cfg.patchSize;
    // warped patches in LDS while they fit (as the after-stage keeps them); else one slab per workgroup in HBM, the grid
    // capped so that the slabs stay within 256 MB (K = 64 at r = 127: 33 MB a slab, 8 workgroups)
    const int hpInLds = (pais_launch::hp_in_lds(sc, Kmax) && pais_launch::ncc_lds_bytes(Kmax) + hpBytes <= ctx->ldsLimit) ? 1 : 0;
    long grid = (long)ctx->numCUs * (hpInLds ? 8 : 2);
    if (!hpInLds) {
        const long cap = (long)(((size_t)256 << 20) / hpBytes);
        grid = std::min(grid, std::max(1L, cap));
    }
    grid = std::min(grid, (long)n);
    const size_t tableBytes = tables ? sizeof(double) * (size_t)stride * stride * (size_t)n : 0;
    HIPCHK(ctx->d_vStates.reserve(ctx->stream, sizeof(pais_view_state) * (size_t)n));
    HIPCHK(ctx->d_vOut.reserve(ctx->stream, sizeof(pais_view_result) * (size_t)n));
    if (tables) HIPCHK(ctx->d_vTables.reserve(ctx->stream, tableBytes));
    if (!hpInLds) HIPCHK(ctx->d_vHp.reserve(ctx->stream, hpBytes * (size_t)grid));
    HIPCHK(hipMemcpyAsync(ctx->d_vStates, states, sizeof(pais_view_state) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    TimedLaunch t(ctx);
    if (t.begin()) return -2;
    HIPCHK(pais_launch::ncc_batch(sc, ctx->d_vStates, n, ctx->d_vOut, tables ? ctx->d_vTables.p : nullptr, stride, ctx->d_vHp, (int)grid, Kmax,
                                  hpInLds, ctx->stream));
    if (t.end()) return -2;
    HIPCHK(hipMemcpyAsync(out, ctx->d_vOut, sizeof(pais_view_result) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (tables) HIPCHK(hipMemcpyAsync(tables, ctx->d_vTables, tableBytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    t.collect(ctx->ncc, n);
    return 0;
}

extern "C" int pais_get_ncc_stats(pais_ctx *ctx, double *kernel_ms, int64_t *launches, int64_t *states, int reset)
{
    return read_launch_stats(ctx ? &ctx->ncc : nullptr, "pais_get_ncc_stats", kernel_ms, launches, states, reset);
}

// --------------------------------------------------------------- load state --
// the loader constructor of every patch record of an .mvs cloud (k_load_state)
static const CamListRules kLoadRules = {"pais_load_state_batch", "patch", 0, false, CamListRules::NoRef};

extern "C" int pais_load_state_batch(pais_ctx *ctx, int n, const pais_loaded_patch *in, pais_patch_result *out)
{
    if (n < 0) return fail_msg("pais_load_state_batch: bad argument (n < 0)");
    if (n == 0) return 0;
    const char *missing = !ctx ? "ctx" : !in ? "in" : !out ? "out" : nullptr;
    if (missing) return fail_fmt("pais_load_state_batch: null pointer (%s)", missing);
    for (int i = 0; i < n; ++i) {
        const int rc = check_cam_list(ctx, kLoadRules, i, in[i].num_cam, in[i].cam_idx, 0, 0);
        if (rc) return rc;
    }
    HIPCHK(hipSetDevice(ctx->device));
    const int chunk = staging_chunk("PAIS_LOAD_STAGING_MB", n, sizeof(pais_loaded_patch) + sizeof(pais_patch_result));
    HIPCHK(ctx->d_lIn.reserve(ctx->stream, sizeof(pais_loaded_patch) * (size_t)chunk));
    HIPCHK(ctx->d_lOut.reserve(ctx->stream, sizeof(pais_patch_result) * (size_t)chunk));
    for (int c0 = 0; c0 < n; c0 += chunk) {
        const int m = std::min(chunk, n - c0);
        HIPCHK(hipMemcpyAsync(ctx->d_lIn, in + c0, sizeof(pais_loaded_patch) * (size_t)m, hipMemcpyHostToDevice, ctx->stream));
        TimedLaunch t(ctx);
        if (t.begin()) return -2;
        HIPCHK(pais_launch::load_state(ctx->sc, ctx->d_lIn, ctx->d_lOut, m, (uint64_t)c0, ctx->stream));
        if (t.end()) return -2;
        HIPCHK(hipMemcpyAsync(out + c0, ctx->d_lOut, sizeof(pais_patch_result) * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        t.collect(ctx->load, m);
    }
    return 0;
}

extern "C" int pais_get_load_stats(pais_ctx *ctx, double *kernel_ms, int64_t *launches, int64_t *patches, int reset)
{
    return read_launch_stats(ctx ? &ctx->load : nullptr, "pais_get_load_stats", kernel_ms, launches, patches, reset);
}
extern "C" size_t pais_sizeof_loaded_patch(void) { return sizeof(pais_loaded_patch); }

// ------------------------------------------------------------- fitness detail --
// PAIS::getFitness with its per-pixel intermediates (k_fitness_detail, pais_literal.hpp)
extern "C" int pais_fitness_detail(pais_ctx *ctx, int n_states, const pais_patch_state *states, int n_evals, const int32_t *state_index,
                                   const double *particles, pais_cost_detail *out, double *weight, double *avg_sad, int8_t *pixel_code,
                                   double *colour, double *homographies, int cam_stride)
{
    if (!ctx || n_states < 0 || n_evals < 0) return fail_msg("pais_fitness_detail: bad argument");
    if (n_evals == 0) return 0;
    const char *missing = !states ? "states" : !state_index ? "state_index" : !particles ? "particles" : !out ? "out" : !weight ? "weight"
                          : !avg_sad ? "avg_sad" : !pixel_code ? "pixel_code" : nullptr;
    if (missing) return fail_fmt("pais_fitness_detail: null pointer (%s)", missing);
    int Kmax = 1;
    const int rc = check_states(ctx, kDetailRules, n_states, states, n_evals, state_index, Kmax);
    if (rc) return rc;
    for (int i = 0; (colour || homographies) && i < n_states; ++i)
        if (cam_stride < states[i].num_cam)
            return fail_fmt("pais_fitness_detail: state %d: cam_stride %d below num_cam %d", i, cam_stride, states[i].num_cam);
    HIPCHK(hipSetDevice(ctx->device));
    const DevScene &sc = ctx->sc;
    const size_t S2 = (size_t)sc.cfg.patchSize * sc.cfg.patchSize;
    // the maps of a chunk of evaluations stay within the staging bound (K = 64 at r = 127: 33 MB of colours per evaluation)
    const size_t perEval = sizeof(pais_cost_detail) + sizeof(int32_t) + 3 * sizeof(double) + S2 * (2 * sizeof(double) + 1) +
                           (colour ? sizeof(double) * (size_t)Kmax * S2 : 0) + (homographies ? sizeof(double) * 9 * (size_t)Kmax : 0);
    const int chunk = staging_chunk("PAIS_DETAIL_STAGING_MB", n_evals, perEval);
    hipStream_t st = ctx->stream;
    HIPCHK(ctx->d_dStates.reserve(st, sizeof(pais_patch_state) * (size_t)n_states));
    HIPCHK(ctx->d_evalBlocks.reserve(st, pais_launch::eval_block_bytes_host(Kmax) * (size_t)n_states));
    HIPCHK(ctx->d_win.reserve(st, pais_launch::win_bytes_per_candidate(sc) * (size_t)n_states));
    HIPCHK(ctx->d_dIdx.reserve(st, sizeof(int32_t) * (size_t)chunk));
    HIPCHK(ctx->d_dParticles.reserve(st, 3 * sizeof(double) * (size_t)chunk));
    HIPCHK(ctx->d_dRec.reserve(st, sizeof(pais_cost_detail) * (size_t)chunk));
    HIPCHK(ctx->d_dWeight.reserve(st, sizeof(double) * S2 * chunk));
    HIPCHK(ctx->d_dSad.reserve(st, sizeof(double) * S2 * chunk));
    HIPCHK(ctx->d_dCode.reserve(st, S2 * chunk));
    if (colour) HIPCHK(ctx->d_dColour.reserve(st, sizeof(double) * (size_t)Kmax * S2 * chunk));
    if (homographies) HIPCHK(ctx->d_dH.reserve(st, sizeof(double) * 9 * (size_t)Kmax * chunk));
    HIPCHK(hipMemcpyAsync(ctx->d_dStates, states, sizeof(pais_patch_state) * (size_t)n_states, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(pais_launch::state_blocks(sc, ctx->d_dStates, n_states, Kmax, ctx->d_evalBlocks, ctx->d_win, ctx->stream));
    // colours and homographies come down as Kmax rows per evaluation and are repacked here: only the state's own num_cam rows
    // of the caller's cam_stride block are written
    std::vector<double> hCol(colour ? (size_t)Kmax * S2 * chunk : 0), hH(homographies ? (size_t)9 * Kmax * chunk : 0);
    for (int c0 = 0; c0 < n_evals; c0 += chunk) {
        const int n = std::min(chunk, n_evals - c0);
        HIPCHK(hipMemcpyAsync(ctx->d_dIdx, state_index + c0, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipMemcpyAsync(ctx->d_dParticles, particles + 3 * (size_t)c0, 3 * sizeof(double) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
        TimedLaunch t(ctx);
        if (t.begin()) return -2;
        HIPCHK(pais_launch::fitness_detail(sc, ctx->d_dIdx, ctx->d_dParticles, n, Kmax, ctx->d_evalBlocks, ctx->d_dRec, ctx->d_dWeight, ctx->d_dSad,
                                           ctx->d_dCode, colour ? ctx->d_dColour.p : nullptr, homographies ? ctx->d_dH.p : nullptr, ctx->stream));
        if (t.end()) return -2;
        HIPCHK(hipMemcpyAsync(out + c0, ctx->d_dRec, sizeof(pais_cost_detail) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipMemcpyAsync(weight + S2 * c0, ctx->d_dWeight, sizeof(double) * S2 * n, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipMemcpyAsync(avg_sad + S2 * c0, ctx->d_dSad, sizeof(double) * S2 * n, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipMemcpyAsync(pixel_code + S2 * c0, ctx->d_dCode, S2 * n, hipMemcpyDeviceToHost, ctx->stream));
        if (colour) HIPCHK(hipMemcpyAsync(hCol.data(), ctx->d_dColour, sizeof(double) * (size_t)Kmax * S2 * n, hipMemcpyDeviceToHost, ctx->stream));
        if (homographies) HIPCHK(hipMemcpyAsync(hH.data(), ctx->d_dH, sizeof(double) * 9 * (size_t)Kmax * n, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        t.collect(ctx->detail, n);
        for (int e = 0; e < n; ++e) {
            const size_t K = (size_t)states[state_index[c0 + e]].num_cam, g = (size_t)c0 + e;
            if (colour) memcpy(colour + g * cam_stride * S2, hCol.data() + (size_t)e * Kmax * S2, sizeof(double) * K * S2);
            if (homographies) memcpy(homographies + g * cam_stride * 9, hH.data() + (size_t)e * Kmax * 9, sizeof(double) * K * 9);
        }
    }
    return 0;
}

extern "C" int pais_get_detail_stats(pais_ctx *ctx, double *kernel_ms, int64_t *launches, int64_t *evals, int reset)
{
    return read_launch_stats(ctx ? &ctx->detail : nullptr, "pais_get_detail_stats", kernel_ms, launches, evals, reset);
}

// ------------------------------------------------------------- refine batch --
// One PSO pass of a batch as the host enqueues it: opened (pipeline chosen, slices forked to the sub-streams), its
// iterations enqueued in one or several pieces, closed (sub-streams joined, after-stage).  Pieces exist so that the
// launch sequences of two lanes can be interleaved by a driver (pais_refine_batch_open / _enqueue).
static int pass_open(pais_ctx *ctx, PassPlan &P, int pass, int againCount)
{
    const DevScene &sc = ctx->sc;
    P.cnt = ctx->d_counters + 4 * (ctx->passSerial & 1);
    P.nextCnt = ctx->d_counters + 4 * ((ctx->passSerial + 1) & 1);
    ctx->passSerial++;
    if (P.tp.begin(ctx, ctx->stream, &ctx->evPso)) return -2;
    if (pass > 0) // (pass 0: done by the begin launch)
        HIPCHK(pais_launch::pso_init(sc, P.all, ctx->d_active, P.cnt + 2));
    // k_pso_iter needs the swarm of a candidate in the lanes of one wave; a batch of several residency passes
    // (>= 3 x 12 waves per CU) is throughput bound: there the step replay in every evaluation wave (~13 % of a wave's
    // time) costs more than a separate one-wave-per-candidate k_pso_step launch per iteration, whose latency the other
    // sub-stream hides
    // the tile kernel pays where the taps miss the caches: scenes whose pyramids exceed PAIS_TAP_FLOAT_MAX_MB (those that tap
    // the byte blob; the dome: PSO passes -22 %).  On the 184 MB ring, whose taps hit L2, it LOSES 35 % against the
    // one-wave kernels (profiles/r03_ring_tile_ab.txt) -- PAIS_TILE=2 forces it regardless (tests)
    const bool tileOk = (ctx->tileMode == 2 || (ctx->tileMode == 1 && ctx->sc.imgF == nullptr)) && pais_launch::tile_eligible(P.all.Kmax);
    // (the tile kernel is an evaluation launch of the large-batch pipeline: batches that are eligible for it take that
    // pipeline from PAIS_TILE_ABOVE waves per iteration on)
    // (a batch that is one part of a streamed round shares the GPU with the other part: the pipeline is chosen for the round)
    const int n = P.all.n, Nmax = P.all.Nmax;
    const int nPlan = ctx->roundHint > n ? ctx->roundHint : n;
    P.useIter = Nmax <= 64 && (long)nPlan * Nmax < (tileOk ? ctx->tileAbove : ctx->splitAbove);
    P.useTile = tileOk && !P.useIter;
    if (ctx->arithLiteral) P.useIter = P.useTile = false; // (and no ring below): k_pso_eval_lit + k_pso_step for every batch
    // the PSO pass as ONE launch over device-side task rings (k_pso_ring): host batches, device-pointer batches (the shards of
    // the multi-GPU drivers) and the passes of seed batches alike -- the error words are read at the batch's (pass's) next
    // synchronisation point and a pass that did not complete is re-run through the per-iteration launches (ring_failed below).
    // (a candidate's chain of maxIt evaluation + step latencies bounds a ring launch from below; the longer an evaluation -- more
    // cameras --, the more candidates it takes for throughput to dominate that chain: PAIS_RING_PER_CAM waves per iteration and camera;
    // where the ring has part kernels it takes the pass from that bound on whatever k_pso_iter's own bound says -- it wins well below it)
    const long ringWaves = (long)(P.hasSeeds && pass > 0 ? againCount : n) * Nmax;
    // waves per evaluation: a front of ringWaves tasks that leaves resident waves idle is shared out further -- a link of a
    // candidate's chain is then a part of a window walk (the two-pixel shapes have the part kernels; 12 resident waves per CU)
    P.ringCUs = ctx->numCUs;
    P.ringParts = 1;
    const bool ringHasParts = pais_launch::ring_parts_ok(P.all.Kmax);
    const double ringPerCam = ctx->ringPerCam >= 0 ? ctx->ringPerCam : (ringHasParts ? 540.0 : 1843.0);
    if (ringHasParts) {
        const double resident = (double)P.ringCUs * 12 * ctx->ringPartFill;
        P.ringParts = ctx->ringPartsForced > 0 ? ctx->ringPartsForced : (ringWaves * 4 <= resident ? 4 : (ringWaves * 2 <= resident ? 2 : 1));
    }
    const size_t ringNeed = pais_launch::ring_words(n, Nmax, P.all.maxIt, P.ringParts) * sizeof(unsigned);
    // (Nmax <= 64 is load-bearing: k_pso_ring publishes a swarm's tasks by the lanes of one wave AND holds only the lane-parallel
    //  swarm step, pso_step_wave_ring in pais_kernels.hip -- there is no serial form inside the ring; pais_launch::pso_ring refuses more)
    P.useRing = ctx->ringMode != 0 && !ctx->arithLiteral && !ctx->ringSuppressed && !P.useTile && Nmax <= 64 && n < (1 << 24) && ringNeed <= ctx->ringMaxBytes &&
                (P.hasSeeds ? (ctx->ringSeedAbove > 0 && ringWaves >= ctx->ringSeedAbove)
                            : ((ringHasParts || !P.useIter) && ringWaves >= (long)(ringPerCam * P.all.Kmax)));
    // (the parts of a streamed round keep the per-iteration launches, which interleave on their lanes; two ring launches would
    // run one after the other, or each on its share of the CUs -- ring scene 17.5 s against 18.3 / 19.7 s that way)
    if (P.useRing && nPlan > n && ctx->ringMode != 3) P.useRing = false;
    if (P.trace) P.useIter = P.useTile = P.useRing = false; // (the trace: k_pso_eval2 / k_pso_eval_lit + k_pso_step_trace)
    if (P.useRing) P.useIter = false;
    if (P.useRing) {
        HIPCHK(ctx->d_ring.reserve(ctx->stream, ringNeed));
        HIPCHK(ctx->d_arrive.reserve(ctx->stream, sizeof(int) * PAIS_ARRIVE_STRIDE * (size_t)n));
    }
    // the large-batch pipelines of the kernel arithmetic read the evaluations' set-up from records the swarm step writes
    P.usePre = ctx->preMode != 0 && !ctx->arithLiteral && !P.useIter && !P.useTile && !(P.useRing && !pais_launch::pre_ring_ok(P.all.Kmax)) && !P.trace;
    P.all.pre = nullptr;
    if (P.usePre) {
        HIPCHK(ctx->d_pre.reserve(ctx->stream, pais_launch::pre_bytes_per_candidate(Nmax, P.all.Kmax) * (size_t)n));
        P.all.pre = ctx->d_pre;
        HIPCHK(pais_launch::pso_setup0(sc, P.all));
    }
    // k_pso_iter works on the compacted list of candidates that run a PSO in this pass (k_pso_init);
    // its length is n at most in the first pass and exactly the "again" count afterwards
    const int nRun = P.useIter ? (pass == 0 ? n : againCount) : n;
    int S = P.useRing ? 1 : ctx->psoStreams;
    if (nPlan > n) S = (int)((double)S * n / nPlan + 0.5); // the round's sub-streams are shared out among its parts
    const int minPer = ctx->psoMinPer; // slices smaller than this only add launch overhead
    if (nRun < S * minPer) S = (nRun + minPer - 1) / minPer;
    if (S < 1 || P.trace) S = 1;
    P.S = S;
    if (S > 1) HIPCHK(hipEventRecord(ctx->forkEv, ctx->stream));
    // slice 0 stays on the context's own stream, the others fork to sub-streams and join back
    P.nSl = 0;
    for (int sI = 0; sI < S; ++sI) {
        PassPlan::Slice q;
        q.lo = (int)((long)nRun * sI / S);
        q.hi = (int)((long)nRun * (sI + 1) / S);
        if (q.hi <= q.lo) continue;
        const bool own = (S == 1) || (sI == 0);
        const hipStream_t st = own ? ctx->stream : ctx->sub[sI - 1];
        if (!own) HIPCHK(hipStreamWaitEvent(st, ctx->forkEv, 0));
        // (the slices of a k_pso_iter pass are ranges of the active list, not of the candidates: the whole batch)
        q.v = P.useIter ? P.all.slice(sc, 0, n, st) : P.all.slice(sc, q.lo, q.hi, st);
        q.trace = pais_launch::TraceSink{nullptr, nullptr, nullptr, 1, 1};
        if (P.trace) { // rows of the slice's first candidate
            const pais_launch::TraceSink &t = P.trace->sink;
            const size_t slot0 = (size_t)q.lo * t.maxRuns;
            q.trace = pais_launch::TraceSink{t.runs + slot0, t.iters + slot0 * t.rows, t.particles ? t.particles + slot0 * t.rows * Nmax * 11 : nullptr,
                                             t.maxRuns, t.rows};
        }
        // waves per evaluation: a slice that leaves the GPU mostly empty is bound by the latency of
        // one evaluation wave, so share each evaluation among 4 (2) waves while they all stay resident
        q.parts = 1;
        if (P.useIter) {
            const long waves = (long)(q.hi - q.lo) * Nmax, resident = (long)((double)ctx->numCUs * 16 * ctx->partFill * n / nPlan);
            q.parts = ctx->evalParts > 0 ? ctx->evalParts : (waves * 4 <= resident ? 4 : (waves * 2 <= resident ? 2 : 1));
        }
        P.sl[P.nSl++] = q;
    }
    P.itNext = 0;
    return 0;
}

// iterations [P.itNext, itEnd) of the pass (itEnd is clamped to maxIt + 1: launch `it` = step it - 1 + cost of the moved swarm)
static int pass_iterations(pais_ctx *ctx, PassPlan &P, int itEnd)
{
    const DevScene &sc = ctx->sc;
    if (itEnd > P.all.maxIt + 1) itEnd = P.all.maxIt + 1;
    if (P.useRing) {
        if (P.itNext == 0 && itEnd > 0) {
            const unsigned long long ticks = (unsigned long long)(ctx->ringTimeoutMs * 1e5); // s_memrealtime counts at 100 MHz
            auto ring = [&](int phase) { // 0: the ring's set-up, 1: the pass
                return pais_launch::pso_ring(sc, P.all, ctx->d_ring, ctx->d_ringCtl, ctx->d_arrive, ctx->stat, P.ringCUs, phase, ticks, P.ringParts);
            };
            HIPCHK(ring(0));
            Timed te; // (the kernel alone)
            if (te.begin(ctx, ctx->stream, &ctx->evRing)) return -2;
            HIPCHK(ring(1));
            if (te.end()) return -2;
            HIPCHK(hipMemcpyAsync(ctx->h_ringCtl, ctx->d_ringCtl, PAIS_RING_CTL_BYTES * PAIS_RINGS, hipMemcpyDeviceToHost, ctx->stream));
            ctx->ringUsed = true;
            ctx->evalLaunches++;
            ctx->eval2Launches++;
            ctx->ringLaunches++;
            ctx->ringLaunchesByParts[P.ringParts == 4 ? 2 : (P.ringParts == 2 ? 1 : 0)]++;
            P.itNext = P.all.maxIt + 1; // the launch covers every iteration of the pass
        }
        return 0;
    }
    // enqueued iteration by iteration across the slices: every sub-stream has work from the start (slice by slice, the
    // second slice would begin one host enqueue pass -- 62 launches -- after the first)
    TimedLaunch tpass(ctx); // (a trace: its one slice runs on the context's stream)
    const bool timePass = P.trace && itEnd > P.itNext;
    if (timePass && tpass.begin()) return -2;
    for (int it = P.itNext; it < itEnd; ++it) {
        for (int k = 0; k < P.nSl; ++k) {
            const PassPlan::Slice &q = P.sl[k];
            Timed te; // events on the stream the kernel is launched on
            if (te.begin(ctx, q.v.stream, P.useIter ? &ctx->evEval : &ctx->evEval2)) return -2;
            if (P.useIter)
                HIPCHK(pais_launch::pso_iter(sc, q.v, ctx->d_active, P.cnt + 2, q.lo, q.hi, ctx->stat, it, 0, q.parts));
            else if (P.useTile) {
                // many cameras: footprints staged in LDS (pais_tile2.hpp); the particles it flags take the checked walk
                HIPCHK(pais_launch::pso_tile(sc, q.v, ctx->tile, ctx->tileDebug ? ctx->stat + 8 : nullptr));
                HIPCHK(pais_launch::pso_eval(sc, q.v, ctx->tileVerify ? 2 : 1, ctx->stat + 18));
            } else if (ctx->arithLiteral)
                HIPCHK(pais_launch::pso_eval_literal(sc, q.v));
            else
                HIPCHK(pais_launch::pso_eval(sc, q.v, 0, nullptr));
            if (te.end()) return -2;
            ctx->evalLaunches++;
            if (!P.useIter) ctx->eval2Launches++;
            if (P.useTile) ctx->tileLaunches++;
            if (P.trace) {
                HIPCHK(pais_launch::pso_step_trace(sc, q.v, ctx->stat, q.trace));
                P.trace->launches++;
            } else if (!P.useIter)
                HIPCHK(pais_launch::pso_step(sc, q.v, ctx->stat));
        }
    }
    if (timePass) {
        if (tpass.end()) return -2;
        P.trace->passes.push_back(std::move(tpass));
    }
    if (itEnd > P.itNext) P.itNext = itEnd;
    return 0;
}

// the sub-streams a pass forked to join the context's stream again (also on the error paths: nothing stays forked)
static int pass_join(pais_ctx *ctx, PassPlan &P)
{
    for (int sI = 1; sI < P.S; ++sI) {
        bool used = false;
        for (int k = 0; k < P.nSl; ++k) used = used || (P.sl[k].v.stream == ctx->sub[sI - 1]);
        if (!used) continue;
        HIPCHK(hipEventRecord(ctx->subDone[sI - 1], ctx->sub[sI - 1]));
        HIPCHK(hipStreamWaitEvent(ctx->stream, ctx->subDone[sI - 1], 0));
    }
    P.S = 1;
    return 0;
}

static int pass_close(pais_ctx *ctx, PassPlan &P)
{
    const DevScene &sc = ctx->sc;
    for (int k = 0; k < P.nSl; ++k) {
        const PassPlan::Slice &q = P.sl[k];
        // the launch after the last possible iteration only ends the runs still active
        if (P.useIter)
            HIPCHK(pais_launch::pso_iter(sc, q.v, ctx->d_active, P.cnt + 2, q.lo, q.hi, ctx->stat, P.all.maxIt + 1, 1, q.parts));
    }
    if (pass_join(ctx, P)) return -2;
    if (P.tp.end()) return -2;
    ctx->psoLaunches++;
    Timed ta;
    if (ta.begin(ctx, ctx->stream, &ctx->evAfter)) return -2;
    HIPCHK(pais_launch::after(sc, P.all.recs, P.all.n, ctx->d_hp, P.afterGrid, P.cnt, ctx->stat, P.all.Kmax, ctx->d_ratios, P.nextCnt, ctx->stream));
    if (ta.end()) return -2;
    return 0;
}

// work buffers, the head of refine() and the set-up of every candidate's first PSO run (k_begin)
static int batch_setup(pais_ctx *ctx, PassPlan &P, int n, const pais_candidate *d_cands, pais_patch_result *d_out, int max_num_cam, int has_seeds)
{
    HIPCHK(hipSetDevice(ctx->device));
    const DevScene &sc = ctx->sc;
    int Kmax = max_num_cam > 0 ? max_num_cam : sc.numCams;
    if (Kmax > PAIS_MAX_VIS) Kmax = PAIS_MAX_VIS;
    if (Kmax > sc.numCams) Kmax = sc.numCams;
    if (Kmax < 1) Kmax = 1;
    const int Nmax = has_seeds ? sc.cfg.particleNum * 2 : sc.cfg.particleNum;
    const int S2 = sc.cfg.patchSize * sc.cfg.patchSize;
    const int afterGrid = n < 2048 ? n : 2048;
    { // (a d_hp that has to grow goes to the size of the largest after-stage grid, 2048 slabs, at once)
        size_t hpNeed = (size_t)afterGrid * Kmax * S2 * sizeof(double);
        const size_t full = (size_t)2048 * Kmax * S2 * sizeof(double);
        if (hpNeed > ctx->d_hp.bytes && full < ((size_t)1 << 31)) hpNeed = full;
        HIPCHK(ctx->d_hp.reserve(ctx->stream, hpNeed));
    }
    HIPCHK(ctx->d_active.reserve(ctx->stream, sizeof(int) * (size_t)n));
    HIPCHK(ctx->d_evalBlocks.reserve(ctx->stream, pais_launch::eval_block_bytes_host(Kmax) * (size_t)n));
    HIPCHK(ctx->d_win.reserve(ctx->stream, pais_launch::win_bytes_per_candidate(sc) * (size_t)n));
    HIPCHK(ctx->d_psoStates.reserve(ctx->stream, pais_launch::pso_state_bytes_host(Nmax) * (size_t)n));
    HIPCHK(ctx->d_ratios.reserve(ctx->stream, sizeof(double) * PAIS_MAX_VIS * (size_t)n));
    P.all = pais_launch::BatchView{d_out, ctx->d_psoStates, ctx->d_evalBlocks, ctx->d_win, nullptr, n, Nmax, Kmax,
                                   has_seeds ? sc.cfg.maxIteration * 2 : sc.cfg.maxIteration, ctx->stream};
    P.hasSeeds = has_seeds != 0;
    P.afterGrid = afterGrid;
    P.d_cands = d_cands;

    if (ctx->countersDirty) HIPCHK(hipMemsetAsync(ctx->d_counters, 0, sizeof(int) * 8, ctx->stream));
    ctx->countersDirty = true; // until this batch has run through
    Timed tb;
    if (tb.begin(ctx, ctx->stream, &ctx->evBegin)) return -2;
    // head of refine() and the set-up of the first PSO run of every candidate in one launch
    HIPCHK(pais_launch::begin(sc, P.all, d_cands, ctx->d_active, ctx->d_counters + 4 * (ctx->passSerial & 1) + 2));
    if (tb.end()) return -2;
    return 0;
}

// The error words of the ring pass that has just been synchronised with (h_ringCtl: per ring {head, tail, done, total, error}).
// 0: every run ended; 1: a wave ran out of patience, or runs never ended -- the caller re-runs the batch without the ring.
static int ring_failed(pais_ctx *ctx, int n)
{
    if (!ctx->ringUsed) return 0;
    ctx->ringUsed = false;
    unsigned done = 0, err = 0;
    for (int r = 0; r < PAIS_RINGS; ++r) { done += ctx->h_ringCtl[(PAIS_RING_CTL_BYTES / 4) * r + PAIS_RING_CTL_DONE_WORD]; err |= ctx->h_ringCtl[(PAIS_RING_CTL_BYTES / 4) * r + PAIS_RING_CTL_ERROR_WORD]; }
    if (err == 0 && done == (unsigned)n) return 0;
    ctx->ringFallbacks++;
    // one note per context the first time it happens in production (timeout > 0), every time with PAIS_RING_VERBOSE
    if (getenv("PAIS_RING_VERBOSE") || (ctx->ringFallbacks == 1 && ctx->ringTimeoutMs > 0))
        fprintf(stderr, "[pais] k_pso_ring did not complete (error %u, %u of %d runs ended): the batch is re-run with one launch per iteration\n", err, done, n);
    return 1;
}

// one batch on device pointers, start to end; returns 1 if a ring pass failed (the caller runs it again with the ring off)
// defer: an expansion batch whose pass ran as k_pso_ring returns without waiting for it -- the error words are looked at by
// the wire header the caller asks for next (pais_wire_header_device) and by pais_ctx_batch_status after the caller's own
// synchronisation
// trace: a pais_pso_trace batch (pso trace section)
static int refine_device_once(pais_ctx *ctx, int n, const pais_candidate *d_cands, pais_patch_result *d_out, int max_num_cam, int has_seeds,
                              bool defer = false, TraceOut *trace = nullptr)
{
    PassPlan &P = ctx->plan;
    P.trace = trace;
    ctx->ringUsed = false;
    ctx->ringPendingN = 0;
    int rc = batch_setup(ctx, P, n, d_cands, d_out, max_num_cam, has_seeds);
    int againCount = 0; // seeds that lost cameras in the previous pass and run another PSO (patch.cpp:140-175)
    const int maxPass = has_seeds ? (PAIS_MAX_VIS + 2) : 1;
    for (int pass = 0; !rc && pass < maxPass; ++pass) {
        if ((rc = pass_open(ctx, P, pass, againCount)) != 0) break;
        if ((rc = pass_iterations(ctx, P, P.all.maxIt + 1)) != 0) { (void)pass_join(ctx, P); break; }
        if ((rc = pass_close(ctx, P)) != 0) break;
        if (!has_seeds && !ctx->ringUsed) break; // (asynchronous at return)
        if (!has_seeds && defer) { ctx->ringPendingN = n; break; } // (asynchronous too: the ring's status is read later)
        if (has_seeds) HIPCHK(hipMemcpyAsync(ctx->h_counters, P.cnt, sizeof(int) * 2, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        if (ring_failed(ctx, n)) { ctx->roundHint = 0; return 1; }
        if (!has_seeds || ctx->h_counters[1] == 0) break;
        againCount = ctx->h_counters[1];
    }
    ctx->roundHint = 0;
    if (rc) return rc;
    ctx->countersDirty = false;
    return 0;
}

// A batch whose ring pass did not complete, again from its candidates with the ring suppressed -- one launch per iteration --,
// planned under `hint` (the round hint its first attempt consumed).  The first attempt's after-stage is not trusted to
// have left the counter sets clean.  This is the library's own re-run; behind a deferred status
// (ringPendingN -> pais_ctx_batch_status / the wire header) it is the caller that submits the batch again, and
// ringSuppressOnce routes that submission here.
static int rerun_without_ring(pais_ctx *ctx, int n, const pais_candidate *d_cands, pais_patch_result *d_out, int max_num_cam, int has_seeds,
                              bool defer, int hint)
{
    ctx->ringSuppressed = true;
    ctx->countersDirty = true;
    ctx->roundHint = hint;
    const int rc = refine_device_once(ctx, n, d_cands, d_out, max_num_cam, has_seeds, defer);
    ctx->ringSuppressed = false;
    return rc;
}

// refine_device_once, and the re-run if a ring pass of it did not complete
static int refine_device(pais_ctx *ctx, int n, const pais_candidate *d_cands, pais_patch_result *d_out, int max_num_cam, int has_seeds, bool defer)
{
    const int hint = ctx->roundHint;
    const int rc = refine_device_once(ctx, n, d_cands, d_out, max_num_cam, has_seeds, defer);
    return rc == 1 ? rerun_without_ring(ctx, n, d_cands, d_out, max_num_cam, has_seeds, defer, hint) : rc;
}

extern "C" int pais_refine_batch_device(pais_ctx *ctx, int n, const pais_candidate *d_cands, pais_patch_result *d_out,
                                        int max_num_cam, int has_seeds)
{
    if (!ctx || n < 0) return fail_msg("pais_refine_batch_device: bad argument");
    if (n == 0) return 0;
    if (!d_cands || !d_out) return fail_msg("pais_refine_batch_device: null pointer");
    if (ctx->openBatch >= 0) return fail_msg("pais_refine_batch_device: a batch is open on this context");
    return refine_device(ctx, n, d_cands, d_out, max_num_cam, has_seeds, false);
}

// pais_refine_batch_device that never waits for an expansion batch (a batch with seeds is refined before it returns, as ever)
extern "C" int pais_refine_batch_device_async(pais_ctx *ctx, int n, const pais_candidate *d_cands, pais_patch_result *d_out,
                                              int max_num_cam, int has_seeds)
{
    if (!ctx || n < 0) return fail_msg("pais_refine_batch_device_async: bad argument");
    if (n == 0) return 0;
    if (!d_cands || !d_out) return fail_msg("pais_refine_batch_device_async: null pointer");
    if (ctx->openBatch >= 0) return fail_msg("pais_refine_batch_device_async: a batch is open on this context");
    if (ctx->ringSuppressOnce) { // (pais_ctx_batch_status returned 1 for this batch's first submission)
        ctx->ringSuppressOnce = false;
        return rerun_without_ring(ctx, n, d_cands, d_out, max_num_cam, has_seeds, true, ctx->roundHint);
    }
    return refine_device(ctx, n, d_cands, d_out, max_num_cam, has_seeds, true);
}

// After the caller has synchronised with the context's stream: 0 = the last pais_refine_batch_device_async batch is complete;
// 1 = its k_pso_ring pass did not complete -- the records are NOT valid, the caller refines the same batch again (the next
// batch of this context then takes the per-iteration launches).
extern "C" int pais_ctx_batch_status(pais_ctx *ctx)
{
    if (!ctx) return fail_msg("pais_ctx_batch_status: bad argument");
    if (ctx->ringPendingN <= 0) return 0;
    const int n = ctx->ringPendingN;
    ctx->ringPendingN = 0;
    ctx->countersDirty = false;
    if (!ring_failed(ctx, n)) return 0;
    ctx->countersDirty = true;
    ctx->ringSuppressOnce = true;
    return 1;
}

// 64-byte header of a rank's block in the exchange of a sharded batch, written ON THE DEVICE behind the batch's launches:
// {magic 'PAIS', rc, count, rank, user_word, 0...}; rc = host_rc if that is non-zero, else PAIS_WIRE_RC_RING_RETRY when the batch's
// k_pso_ring pass did not complete (read from the ring's own words: no host round trip before the exchange), else 0.
extern "C" int pais_wire_header_device(pais_ctx *ctx, int rank, int count, int host_rc, uint32_t user_word, void *d_header)
{
    if (!ctx || !d_header) return fail_msg("pais_wire_header_device: bad argument");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(pais_launch::wire_header(d_header, ctx->ringPendingN > 0 ? ctx->d_ringCtl : nullptr, ctx->ringPendingN, rank, count, host_rc, user_word, ctx->stream));
    return 0;
}

// include/pais_test_hooks.h: one swarm step on a caller-given swarm (no context: the step reads no scene)
extern "C" int pais_test_swarm_step(int device, pais_test_swarm *s, double *swarm)
{
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return (int)e;
    return pais_launch::test_swarm_step(s, swarm);
}

// include/pais_test_hooks.h: the ring launches of this context (and of lanes forked from now on) run `parts` waves per evaluation;
// fill > 0: the fill factor of the automatic choice
extern "C" int pais_test_set_ring_parts(pais_ctx *ctx, int parts, double fill)
{
    if (!ctx || !(parts == 0 || parts == 1 || parts == 2 || parts == 4) || !(fill >= 0)) return fail_msg("pais_test_set_ring_parts: bad argument");
    ctx->ringPartsForced = parts;
    if (fill > 0) ctx->ringPartFill = fill;
    return 0;
}
// ... and how many ring launches of 1, 2 and 4 waves per evaluation the context and its lanes have enqueued
extern "C" int pais_test_ring_parts_launches(pais_ctx *ctx, int64_t *launches)
{
    if (!ctx || !launches) return fail_msg("pais_test_ring_parts_launches: bad argument");
    for (int k = 0; k < 3; ++k) {
        launches[k] = ctx->ringLaunchesByParts[k];
        for (pais_ctx *l : ctx->lanes) launches[k] += l->ringLaunchesByParts[k];
    }
    return 0;
}

extern "C" int pais_ctx_set_round_hint(pais_ctx *ctx, int n_round)
{
    if (!ctx) return fail_msg("pais_ctx_set_round_hint: bad argument");
    ctx->roundHint = n_round > 0 ? n_round : 0;
    return 0;
}

// pais_refine_batch without the last copy: *view points at the context's pinned staging buffer (valid until the next batch
// of this context).  The drivers in pais_mvs.hip commit straight from it (2.9 MB of records per large round).
extern "C" int pais_refine_batch_view(pais_ctx *ctx, int n, const pais_candidate *cands, const pais_patch_result **view)
{
    if (!ctx || n < 0) return fail_msg("pais_refine_batch: bad argument");
    if (n == 0) return 0;
    if (!cands || !view) return fail_msg("pais_refine_batch: null pointer");
    int rc = pais_refine_batch_begin(ctx, n, cands);
    if (rc) return rc;
    return pais_refine_batch_end(ctx, view);
}

extern "C" int pais_refine_batch_begin(pais_ctx *ctx, int n, const pais_candidate *cands)
{
    int rc = pais_refine_batch_open(ctx, n, cands, 1 << 20);
    if (rc) return rc;
    rc = pais_refine_batch_enqueue(ctx, 0);
    return rc < 0 ? rc : 0;
}

// the rest of an opened batch's launches, at most `iterations` PSO iterations of them (<= 0: all); 1: the batch is enqueued
// to its end (after-stage and the copy down included), 0: iterations remain
extern "C" int pais_refine_batch_enqueue(pais_ctx *ctx, int iterations)
{
    if (!ctx) return fail_msg("pais_refine_batch_enqueue: bad argument");
    if (ctx->openBatch < 0) return fail_msg("pais_refine_batch_enqueue: no batch is open on this context");
    if (ctx->planDone) return 1;
    HIPCHK(hipSetDevice(ctx->device));
    PassPlan &P = ctx->plan;
    const int itEnd = iterations > 0 && iterations < P.all.maxIt + 1 - P.itNext ? P.itNext + iterations : P.all.maxIt + 1;
    int rc = pass_iterations(ctx, P, itEnd);
    if (!rc && P.itNext <= P.all.maxIt) return 0;
    if (!rc) rc = pass_close(ctx, P);
    if (rc) { (void)pass_join(ctx, P); ctx->openBatch = -1; ctx->ringUsed = false; return rc; } // (the counters stay marked dirty: cleared before the next batch)
    ctx->countersDirty = false;
    HIPCHK(hipMemcpyAsync(ctx->h_recs, ctx->d_recs, sizeof(pais_patch_result) * (size_t)ctx->openBatch, hipMemcpyDeviceToHost, ctx->stream));
    ctx->planDone = true;
    return 1;
}

extern "C" int pais_refine_batch_end(pais_ctx *ctx, const pais_patch_result **view)
{
    if (!ctx || !view) return fail_msg("pais_refine_batch_end: bad argument");
    if (ctx->openBatch < 0) return fail_msg("pais_refine_batch_end: no batch is open on this context");
    if (!ctx->planDone) {
        const int rc = pais_refine_batch_enqueue(ctx, 0);
        if (rc < 0) return rc;
    }
    ctx->openBatch = -1;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (ring_failed(ctx, ctx->plan.all.n)) {
        // the pass did not complete: the same batch again from its candidates (still in d_cands; an open batch has no seeds)
        const int n = ctx->plan.all.n;
        const int rc = rerun_without_ring(ctx, n, ctx->d_cands, ctx->d_recs, ctx->plan.all.Kmax, 0, false, ctx->roundHint);
        if (rc) return rc;
        HIPCHK(hipMemcpyAsync(ctx->h_recs, ctx->d_recs, sizeof(pais_patch_result) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    *view = ctx->h_recs;
    return 0;
}

extern "C" int pais_refine_batch_open(pais_ctx *ctx, int n, const pais_candidate *cands, int iterations)
{
    if (!ctx || n <= 0 || !cands) return fail_msg("pais_refine_batch_begin: bad argument");
    if (ctx->openBatch >= 0) return fail_msg("pais_refine_batch_begin: a batch is open on this context already");
    HIPCHK(hipSetDevice(ctx->device));
    ctx->ringUsed = false;
    int Kmax = 1, hasSeeds = 0;
    int rc = check_candidates(ctx, "pais_refine_batch", n, cands, Kmax, hasSeeds);
    if (rc) return rc;
    // the candidates and records on the device, and pinned staging for the two per-batch copies: a pageable hipMemcpyAsync is
    // staged by the runtime in small synchronous pieces (two copy kernels and ~0.1 ms per round, which thin rounds notice).
    // (a device buffer and its pinned twin are asked for the same bytes, so the two always grow together)
    HIPCHK(ctx->d_cands.reserve(ctx->stream, sizeof(pais_candidate) * (size_t)n));
    HIPCHK(ctx->d_recs.reserve(ctx->stream, sizeof(pais_patch_result) * (size_t)n));
    HIPCHK(ctx->h_cands.reserve(ctx->stream, sizeof(pais_candidate) * (size_t)n));
    HIPCHK(ctx->h_recs.reserve(ctx->stream, sizeof(pais_patch_result) * (size_t)n));
    memcpy(ctx->h_cands, cands, sizeof(pais_candidate) * (size_t)n);
    HIPCHK(hipMemcpyAsync(ctx->d_cands, ctx->h_cands, sizeof(pais_candidate) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    if (hasSeeds) {
        // the seed loop takes a host decision per pass: refined here and now
        rc = pais_refine_batch_device(ctx, n, ctx->d_cands, ctx->d_recs, Kmax, 1);
        if (rc) return rc;
        HIPCHK(hipMemcpyAsync(ctx->h_recs, ctx->d_recs, sizeof(pais_patch_result) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
        ctx->openBatch = n;
        ctx->planDone = true;
        return 0;
    }
    PassPlan &P = ctx->plan;
    rc = batch_setup(ctx, P, n, ctx->d_cands, ctx->d_recs, Kmax, 0);
    if (!rc) rc = pass_open(ctx, P, 0, 0);
    ctx->roundHint = 0;
    if (!rc && (rc = pass_iterations(ctx, P, iterations > 0 ? iterations : 0)) != 0) (void)pass_join(ctx, P); // (nothing stays forked behind an error)
    if (rc) { ctx->ringUsed = false; return rc; }
    ctx->openBatch = n;
    ctx->planDone = false;
    return 0;
}

extern "C" int pais_refine_batch(pais_ctx *ctx, int n, const pais_candidate *cands, pais_patch_result *out)
{
    if (n > 0 && !out) return fail_msg("pais_refine_batch: null pointer");
    const pais_patch_result *view = nullptr;
    int rc = pais_refine_batch_view(ctx, n, cands, &view);
    if (rc || n <= 0) return rc;
    memcpy(out, view, sizeof(pais_patch_result) * (size_t)n);
    return 0;
}

// ---------------------------------------------------------------- pso trace --
// pais_pso_trace: the batch of pais_refine_batch through refine_device_once (the seed loop's host-synchronised passes
// included) with PassPlan::trace set -- the launch-per-iteration pipeline whatever the batch size, k_pso_step_trace as the
// step.
extern "C" int pais_pso_trace_shape(pais_ctx *ctx, int n, const pais_candidate *cands, int *rows_per_run, int *particles_per_row)
{
    if (!ctx || n < 0 || !rows_per_run || !particles_per_row) return fail_msg("pais_pso_trace_shape: bad argument");
    if (n > 0 && !cands) return fail_msg("pais_pso_trace_shape: null pointer (cands)");
    int Kmax = 1, hasSeeds = 0;
    const int rc = check_candidates(ctx, "pais_pso_trace_shape", n, cands, Kmax, hasSeeds);
    if (rc) return rc;
    const pais_config &cfg = ctx->sc.cfg;
    *rows_per_run = (hasSeeds ? 2 * cfg.maxIteration : cfg.maxIteration) + 1; // (batch_setup's maxIt and Nmax)
    *particles_per_row = hasSeeds ? 2 * cfg.particleNum : cfg.particleNum;
    return 0;
}

// What a trace call must leave as it found it: the kernels' statistics (pais_get_kernel_stats; its launches count into a
// block of their own), the host launch counters, fine timing, the round hint and the status of a pending device batch.
struct TraceScope {
    pais_ctx *ctx;
    unsigned long long *stat;
    bool fine, ringUsed;
    int roundHint, ringPendingN;
    int64_t launches[6];
    explicit TraceScope(pais_ctx *c) : ctx(c)
    {
        stat = c->stat;
        c->stat = c->d_tStat;
        fine = c->fineTiming;
        c->fineTiming = false;
        ringUsed = c->ringUsed;
        ringPendingN = c->ringPendingN;
        roundHint = c->roundHint;
        c->roundHint = 0;
        const int64_t l[6] = {c->psoLaunches, c->evalLaunches, c->eval2Launches, c->tileLaunches, c->ringLaunches, c->ringFallbacks};
        memcpy(launches, l, sizeof(launches));
    }
    ~TraceScope()
    {
        ctx->stat = stat;
        ctx->fineTiming = fine;
        ctx->ringUsed = ringUsed;
        ctx->ringPendingN = ringPendingN;
        ctx->roundHint = roundHint;
        ctx->psoLaunches = launches[0];
        ctx->evalLaunches = launches[1];
        ctx->eval2Launches = launches[2];
        ctx->tileLaunches = launches[3];
        ctx->ringLaunches = launches[4];
        ctx->ringFallbacks = launches[5];
        ctx->plan.trace = nullptr;
    }
};

extern "C" int pais_pso_trace(pais_ctx *ctx, int n, const pais_candidate *cands, int max_runs, pais_patch_result *out,
                              pais_pso_run_info *runs, pais_pso_iter *iters, double *particles)
{
    if (n == 0) return 0;
    if (!ctx) return fail_msg("pais_pso_trace: null pointer (ctx)");
    if (n < 0) return fail_msg("pais_pso_trace: n < 0");
    const char *missing = !cands ? "cands" : !out ? "out" : !runs ? "runs" : !iters ? "iters" : nullptr;
    if (missing) return fail_fmt("pais_pso_trace: null pointer (%s)", missing);
    if (max_runs < 1) return fail_fmt("pais_pso_trace: max_runs %d < 1", max_runs);
    if (ctx->openBatch >= 0) return fail_msg("pais_pso_trace: a stepwise batch is open on this context (pais_refine_batch_open .. _end)");
    int Kmax = 1, hasSeeds = 0;
    int rc = check_candidates(ctx, "pais_pso_trace", n, cands, Kmax, hasSeeds);
    if (rc) return rc;
    HIPCHK(hipSetDevice(ctx->device));
    const pais_config &cfg = ctx->sc.cfg;
    const int rows = (hasSeeds ? 2 * cfg.maxIteration : cfg.maxIteration) + 1;
    const int NP = hasSeeds ? 2 * cfg.particleNum : cfg.particleNum;
    // every chunk is refined with the call's Kmax and seed flag: each one is the batch pais_refine_batch would run, cut short
    const size_t runRows = (size_t)max_runs * rows;
    const size_t perCand = sizeof(pais_candidate) + sizeof(pais_patch_result) + (size_t)max_runs * sizeof(pais_pso_run_info) +
                           runRows * sizeof(pais_pso_iter) + (particles ? runRows * NP * 11 * sizeof(double) : 0);
    const int chunk = staging_chunk("PAIS_TRACE_STAGING_MB", n, perCand);
    if (!ctx->d_tStat) {
        HIPCHK(ctx->d_tStat.alloc(sizeof(unsigned long long) * 24));
        HIPCHK(hipMemset(ctx->d_tStat, 0, sizeof(unsigned long long) * 24));
    }
    HIPCHK(ctx->d_tCands.reserve(ctx->stream, sizeof(pais_candidate) * (size_t)chunk));
    HIPCHK(ctx->d_tRecs.reserve(ctx->stream, sizeof(pais_patch_result) * (size_t)chunk));
    HIPCHK(ctx->d_tRuns.reserve(ctx->stream, sizeof(pais_pso_run_info) * (size_t)max_runs * chunk));
    HIPCHK(ctx->d_tIters.reserve(ctx->stream, sizeof(pais_pso_iter) * runRows * chunk));
    if (particles) HIPCHK(ctx->d_tParts.reserve(ctx->stream, sizeof(double) * 11 * runRows * NP * chunk));
    TraceScope scope(ctx);
    for (int c0 = 0; c0 < n; c0 += chunk) {
        const int m = std::min(chunk, n - c0);
        const size_t nRuns = (size_t)max_runs * m;
        HIPCHK(hipMemcpyAsync(ctx->d_tCands, cands + c0, sizeof(pais_candidate) * (size_t)m, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipMemsetAsync(ctx->d_tRuns, 0, sizeof(pais_pso_run_info) * nRuns, ctx->stream));
        HIPCHK(hipMemsetAsync(ctx->d_tIters, 0, sizeof(pais_pso_iter) * nRuns * rows, ctx->stream));
        if (particles) HIPCHK(hipMemsetAsync(ctx->d_tParts, 0, sizeof(double) * 11 * nRuns * rows * NP, ctx->stream));
        TraceOut t;
        t.sink = pais_launch::TraceSink{ctx->d_tRuns, ctx->d_tIters, particles ? ctx->d_tParts.p : nullptr, max_runs, rows};
        rc = refine_device_once(ctx, m, ctx->d_tCands, ctx->d_tRecs, Kmax, hasSeeds, false, &t);
        if (rc) {
            (void)hipStreamSynchronize(ctx->stream);
            return rc < 0 ? rc : fail_msg("pais_pso_trace: unexpected ring pass");
        }
        HIPCHK(hipMemcpyAsync(out + c0, ctx->d_tRecs, sizeof(pais_patch_result) * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipMemcpyAsync(runs + (size_t)max_runs * c0, ctx->d_tRuns, sizeof(pais_pso_run_info) * nRuns, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipMemcpyAsync(iters + runRows * c0, ctx->d_tIters, sizeof(pais_pso_iter) * nRuns * rows, hipMemcpyDeviceToHost, ctx->stream));
        if (particles)
            HIPCHK(hipMemcpyAsync(particles + runRows * NP * 11 * c0, ctx->d_tParts, sizeof(double) * 11 * nRuns * rows * NP, hipMemcpyDeviceToHost,
                                  ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        for (TimedLaunch &p : t.passes) p.collect(ctx->trace, 0, 0); // (launches and items: counted below)
        ctx->trace.launches += t.launches;
        for (int i = 0; i < m; ++i) ctx->trace.items += out[c0 + i].pso_evals;
    }
    return 0;
}

extern "C" int pais_get_trace_stats(pais_ctx *ctx, double *kernel_ms, int64_t *launches, int64_t *evals, int reset)
{
    return read_launch_stats(ctx ? &ctx->trace : nullptr, "pais_get_trace_stats", kernel_ms, launches, evals, reset);
}

// ------------------------------------------------------------- record wire --
// include/pais_hip.h "wire format of a record".  Word offsets of the record are asserted against the struct.
static_assert(offsetof(pais_patch_result, imgPoint) == 136 && offsetof(pais_patch_result, key) == 1160 &&
              offsetof(pais_patch_result, type) == 1168 && offsetof(pais_patch_result, cam_idx) == 1200 &&
              offsetof(pais_patch_result, stage) == 1456 && sizeof(pais_patch_result) == 1488, "pais_patch_result layout");
static inline int wire_kw(int max_num_cam)
{
    int k = max_num_cam < 1 ? 1 : (max_num_cam > PAIS_MAX_VIS ? PAIS_MAX_VIS : max_num_cam);
    return (k + 1) & ~1;
}
extern "C" size_t pais_record_wire_bytes(int max_num_cam) { return 208 + 20 * (size_t)wire_kw(max_num_cam); }
extern "C" int pais_pack_records(int n, const pais_patch_result *recs, int max_num_cam, void *wire)
{
    if (n < 0 || (n && (!recs || !wire))) return fail_msg("pais_pack_records: bad argument");
    const int Kw = wire_kw(max_num_cam);
    const size_t WB = pais_record_wire_bytes(max_num_cam);
    for (int i = 0; i < n; ++i) {
        const unsigned char *r = (const unsigned char *)&recs[i];
        unsigned char *w = (unsigned char *)wire + WB * (size_t)i;
        memcpy(w, r, 136);                  // center .. correlation
        memcpy(w + 136, r + 1160, 8);       // key
        memcpy(w + 144, r + 1168, 32);      // type .. pso_evals
        memcpy(w + 176, r + 1456, 32);      // stage .. ncc_tables
        memcpy(w + 208, r + 136, 16 * (size_t)Kw);
        memcpy(w + 208 + 16 * (size_t)Kw, r + 1200, 4 * (size_t)Kw);
    }
    return 0;
}
extern "C" int pais_unpack_records(int n, const void *wire, int max_num_cam, pais_patch_result *recs)
{
    if (n < 0 || (n && (!recs || !wire))) return fail_msg("pais_unpack_records: bad argument");
    const int Kw = wire_kw(max_num_cam);
    const size_t WB = pais_record_wire_bytes(max_num_cam);
    for (int i = 0; i < n; ++i) {
        unsigned char *r = (unsigned char *)&recs[i];
        const unsigned char *w = (const unsigned char *)wire + WB * (size_t)i;
        memset(r, 0, sizeof(pais_patch_result));
        memcpy(r, w, 136);
        memcpy(r + 1160, w + 136, 8);
        memcpy(r + 1168, w + 144, 32);
        memcpy(r + 1456, w + 176, 32);
        memcpy(r + 136, w + 208, 16 * (size_t)Kw);
        memcpy(r + 1200, w + 208 + 16 * (size_t)Kw, 4 * (size_t)Kw);
    }
    return 0;
}
extern "C" int pais_pack_records_device(pais_ctx *ctx, int n, const pais_patch_result *d_recs, int max_num_cam, void *d_wire)
{
    if (!ctx || n < 0 || (n && (!d_recs || !d_wire))) return fail_msg("pais_pack_records_device: bad argument");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(pais_launch::pack_records(d_recs, n, wire_kw(max_num_cam), d_wire, ctx->stream));
    return 0;
}

// the launches of one context (a lane is folded into its parent's figures by pais_get_kernel_stats)
static int collect_stats(pais_ctx *ctx, unsigned long long *st)
{
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (drain_events(ctx, ctx->evPso, ctx->psoMs)) return -2;
    if (drain_events(ctx, ctx->evBegin, ctx->beginMs)) return -2;
    if (drain_events(ctx, ctx->evAfter, ctx->afterMs)) return -2;
    if (drain_events(ctx, ctx->evEval, ctx->evalMs)) return -2;
    // the large-batch evaluation launches, with their intervals since refEv; the k_pso_ring launches are a part of those
    // figures and are reported on their own as well
    const hipEvent_t ref = ctx->parent ? ctx->parent->refEv : ctx->refEv;
    for (std::vector<EventPair> *v : {&ctx->evEval2, &ctx->evRing}) {
        for (auto &p : *v) {
            float a = 0, b = 0;
            if (ref && hipEventElapsedTime(&a, ref, p.a) == hipSuccess && hipEventElapsedTime(&b, ref, p.b) == hipSuccess)
                ctx->eval2Intervals.push_back(std::make_pair(a, b));
        }
        double ms = 0;
        if (drain_events(ctx, *v, ms)) return -2;
        if (v == &ctx->evRing) ctx->ringMs += ms;
        ctx->eval2Ms += ms;
        ctx->evalMs += ms;
    }
    HIPCHK(hipMemcpy(st, ctx->d_stat, sizeof(unsigned long long) * 24, hipMemcpyDeviceToHost));
    if (ctx->tileDebug)
        fprintf(stderr, "[pais tile] particles through the tiles %llu, DBL_MAX %llu, pending (checked walk) %llu; tiles staged %llu (%.1f KB each), cameras left in global memory %llu\n",
                st[8], st[9], st[10], st[11], st[11] ? (double)st[13] / (double)st[11] / 1024.0 : 0.0, st[12]);
    if (ctx->tileVerify) {
        double a, b;
        memcpy(&a, &st[20], 8); memcpy(&b, &st[21], 8);
        if (st[18]) // (the tests look for this line)
            fprintf(stdout, "[pais tile verify] %llu particles differ; first: candidate %llu particle %llu: tile %.17g one-wave %.17g\n", st[18],
                    st[19] >> 32, st[19] & 0xffffffffULL, a, b);
        fflush(stdout);
    }
    if (ctx->tileDebug)
        fprintf(stderr, "[pais tile] cycles of wave 0 per phase: boxes %.3g, layout %.3g, copy %.3g, walk %.3g\n", (double)st[14], (double)st[15], (double)st[16], (double)st[17]);
    return 0;
}

extern "C" int pais_get_kernel_stats(pais_ctx *ctx, pais_kernel_stats *out, int reset)
{
    if (!ctx || !out) return fail_msg("pais_get_kernel_stats: bad argument");
    HIPCHK(hipSetDevice(ctx->device));
    std::vector<pais_ctx *> all(1, ctx);
    all.insert(all.end(), ctx->lanes.begin(), ctx->lanes.end());
    memset(out, 0, sizeof(*out));
    const double S2 = (double)ctx->sc.cfg.patchSize * ctx->sc.cfg.patchSize;
    std::vector<std::pair<float, float>> iv;
    for (pais_ctx *c : all) {
        unsigned long long st[24];
        const int rc = collect_stats(c, st);
        if (rc) return rc;
        out->pso_ms += c->psoMs;
        out->begin_ms += c->beginMs;
        out->after_ms += c->afterMs;
        out->pso_launches += c->psoLaunches;
        out->pso_evals += (int64_t)st[0];
        out->pso_patches += (int64_t)st[2];
        out->pso_algorithmic_bytes += (double)st[1] * S2;
        out->ncc_tables += (int64_t)st[3];
        out->ncc_algorithmic_bytes += (double)st[4] * S2 * 4.0;
        out->eval_ms += c->evalMs;
        out->eval_launches += c->evalLaunches;
        out->eval2_ms += c->eval2Ms;
        out->eval2_launches += c->eval2Launches;
        out->tile_launches += c->tileLaunches;
        out->ring_launches += c->ringLaunches;
        out->ring_ms += c->ringMs;
        out->ring_evals += (int64_t)st[22];
        out->ring_algorithmic_bytes += (double)st[23] * S2;
        out->ring_fallbacks += c->ringFallbacks;
        iv.insert(iv.end(), c->eval2Intervals.begin(), c->eval2Intervals.end());
        out->eval2_evals += (int64_t)st[5];
        out->eval2_algorithmic_bytes += (double)st[6] * S2;
        if (reset) {
            HIPCHK(hipMemset(c->d_stat, 0, sizeof(unsigned long long) * 24));
            c->psoMs = c->beginMs = c->afterMs = c->evalMs = c->eval2Ms = c->ringMs = 0;
            c->ringFallbacks = 0;
            c->psoLaunches = 0;
            c->evalLaunches = 0;
            c->eval2Launches = 0;
            c->tileLaunches = 0;
            c->ringLaunches = 0;
            c->eval2Intervals.clear();
        }
    }
    // union of the evaluation launches' intervals (all streams, all lanes)
    std::sort(iv.begin(), iv.end());
    double busy = 0;
    float curA = 0, curB = -1;
    for (auto &p : iv) {
        if (curB < curA || p.first > curB) {
            if (curB >= curA) busy += curB - curA;
            curA = p.first;
            curB = p.second;
        } else if (p.second > curB) {
            curB = p.second;
        }
    }
    if (curB >= curA) busy += curB - curA;
    out->eval2_busy_ms = busy;
    return 0;
}
