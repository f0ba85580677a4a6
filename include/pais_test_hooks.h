/* pais_test_hooks.h -- TEST AND MEASUREMENT HOOKS of libpais_hip.so.
 *
 * NOT part of the drop-in boundary: nothing here replaces a function of the reference, and a maintainer binding the
 * library includes pais_mvs.h / pais_hip.h only.  The two entry points exist so that
 *   - the host scheduler can be tested on machines without a GPU (records supplied by the test's checker), and
 *   - the sharded multi-GPU code path can be timed on ONE GPU (bench.py --emulate-world).
 * They are exported from the same shared object because they exercise its internals; neither computes a record on the host.
 * The test aids further down (one swarm step, the stages of the feature detector) run the product's kernels on given inputs.
 */
#ifndef PAIS_TEST_HOOKS_H
#define PAIS_TEST_HOOKS_H

#include "pais_feature.h"
#include "pais_mvs.h"

#ifdef __cplusplus
extern "C" {
#endif

/* MEASUREMENT AID: one rank of a larger world on ONE GPU (bench.py --emulate-world).  mode 1 on a single-rank driver records
 * the records of every batch, keyed by candidate; mode 2 then makes this driver rank `rank` of `world`: every sharded batch
 * runs the real sharded code path (shard refined on the GPU, packed, status header, copy down, unpack, replicated commit;
 * thin batches replicated; large rounds streamed) with the other ranks' blocks replayed from the recorded run in place of the
 * ncclAllGather -- the bytes arrive over PCIe instead of xGMI, plus PAIS_EMU_LATENCY_US (25) of modelled collective launch
 * latency.  mode 0 switches it off.  What it measures: T_rank(world) on this GPU; what it cannot: link contention and the
 * wait for the slowest rank (bench.py takes the maximum over the ranks it emulates). */
int  pais_mvs_emulate(pais_mvs *m, int mode, int rank, int world);

/* (GPU-less drivers only -- schedulers under test, a host that keeps the records elsewhere; a driver that owns a GPU context
 * refuses it.)  A driver created with device < 0 owns no GPU and never computes a record.  This callback lets the owner of the
 * records (a process that has the GPU, a test's checker) feed the monolithic entry points above -- the stepwise
 * entry points below folded into a callback; n candidates in, n records out, host pointers. */
typedef int (*pais_record_source_fn)(void *user, int n, const pais_candidate *cands, pais_patch_result *out, int has_seeds);
int  pais_mvs_set_record_source(pais_mvs *m, pais_record_source_fn fn, void *user);

/* FAILURE INJECTION into the sharded batch protocol on THIS rank (tests/test_distributed_cpu.py; drivers with a caller-supplied
 * all-gather -- the host instance of shard_submit / shard_finish).  The statuses are those the device path produces by itself:
 *   what 1  the next `count` sharded batches: this rank's header says PAIS_WIRE_RC_RING_RETRY (its k_pso_ring pass did not
 *           complete) -> every rank must take a second exchange, after this rank has refined its shard again;
 *   what 2  the `count`-th growth of the exchange buffers from now fails on this rank -> the growth handshake fails every rank;
 *   what 3  the `count`-th sharded refinement from now fails on this rank -> its header carries the status, every rank fails. */
int  pais_mvs_test_inject(pais_mvs *m, int what, int count);

/* TEST AID: ONE swarm step -- what PsoSolver::run() does between two fitness passes (updateFitness / initFitness, updateGbest,
 * the inertia update, the convergence test, moveParticles: pso_step_wave of pais_kernels.hip, as k_pso_step runs it) -- applied
 * by one wave to a caller-given swarm, so that states a scene rarely produces (ties, zero distances, swarms pinned on a range
 * bound) can be compared with the serial statements compiled for the host (tests/swarm_step_shim.cpp).
 * swarm: n rows of 14 doubles {pos[3], vec[3], pBest[3], nBest[3], fit, pBestFit}, read and written (1 <= n <= 128).
 * The header fields are read and, where the run goes on, written as the step writes them; `continues` = 1 then.  When the run
 * ends the swarm and the header stay as they were, `continues` = 0 and result = {gBestFitness, theta, phi, depth} of the write
 * back.  Returns 0 or a hipError_t. */
typedef struct pais_test_swarm {
    double range_l[3], range_u[3];
    double iw, gbest_fitness;
    uint64_t stream_base;
    int32_t n, max_iteration, iteration, g_idx, started, run, local_k, continues;
    double result[4];
} pais_test_swarm;
int  pais_test_swarm_step(int device, pais_test_swarm *s, double *swarm);

/* TEST AND MEASUREMENT AID: the waves per evaluation of this context's k_pso_ring launches (pais_kernels.hip: a ring task is
 * then a part of an evaluation) -- 1, 2 or 4 instead of the value pass_open chooses from the size of the pass; 0 gives the choice
 * back.  fill > 0 replaces the fill factor of that choice (the largest of 4, 2, 1 with tasks * parts <= fill * resident waves;
 * 6.5), 0 leaves it.  A batch of more than 12 cameras has no part kernels and keeps one wave per evaluation whatever is set.
 * Lanes forked afterwards inherit both.  Records do not depend on either (tests/test_ring_parts.py); scripts/round_log.py takes
 * them as --ring-parts / --ring-part-fill for the sweeps of profiles/ring_parts_ab.txt.  Returns 0, or -1 for another value.
 * pais_test_ring_parts_launches: launches[0 .. 2] = ring launches of 1, 2 and 4 waves per evaluation that the context and its
 * lanes have enqueued since it was created -- what tells a test that the part kernels did run. */
int  pais_test_set_ring_parts(pais_ctx *ctx, int parts, double fill);
int  pais_test_ring_parts_launches(pais_ctx *ctx, int64_t *launches);

/* TEST AID: the stages of pais_feature_detect (pais_feature.h) on ONE octave of one image -- what tests/feature_host_shim.cpp
 * keeps of the host build.  The product's backend runs behind a recorder that is handed to the same walk over octaves: every
 * kernel launches as in pais_feature_detect, and after the extrema and the FIT of octave `octave` their results are copied
 * down.  Image and prm as for pais_feature_detect (same refusals).
 * Sizes first: *sizes is always filled -- octaves walked by the whole run, W x H and the layer count (layers + 3; 0 when the
 * run has no such octave) of octave `octave`, its candidates, its FIT rows (0 or num_cands), and the keypoints of the whole
 * run.  `layers` (layer_floats floats of room) receives the layers, layer after layer, when layers * W * H fits; cands
 * (3 int32 each: x, y, layer, in the order the GPU appended them: ANY order), fit_int (4 int32 each: x, y, layer, ok) and
 * fit_val (3 doubles each: px, py, s), row k of both the FIT of candidate k, are written when num_cands <= max_cands.  Call
 * with no room to learn the sizes, then with room.  Returns 0, < 0 as pais_feature_detect (pais_feature_last_error). */
typedef struct pais_test_feature_sizes {
    int32_t octaves, W, H, layers;
    int64_t num_cands, num_fit, num_keypoints;
} pais_test_feature_sizes;
int  pais_test_feature_stages(int device, const uint8_t *gray, int width, int height, int64_t stride,
                              const pais_feature_params *prm, int octave, pais_test_feature_sizes *sizes,
                              int64_t layer_floats, float *layers, int max_cands, int32_t *cands, int32_t *fit_int, double *fit_val);

#ifdef __cplusplus
}
#endif
#endif /* PAIS_TEST_HOOKS_H */
