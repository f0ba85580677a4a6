#!/usr/bin/env python
"""bench.py -- refined+expanded patches/sec of the MI355X-native PAIS-MVS hot path.

One "step" = one full reconstruction of the workload: MVS::refineSeedPatches +
MVS::expansionPatches to convergence (BASELINE.json configs[1]: 5-camera pawn scene,
patchRadius 15, README config) with the scene already resident in HBM.  Units =
patches taken through refine() that the reference's sequential order evaluates
(seeds + effective expansion candidates); speculative extra refines are reported
separately and never counted.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR]
N > 1: one rank per GPU -- started by torch.distributed.run (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* in the
environment) or, when WORLD_SIZE is not set, by this file itself; it refuses to run when the number of ranks differs
from N or a rank has no GPU of its own.  Under the C ABI (include/pais_mvs.h) every round's candidates are sharded
over the ranks and the records exchanged with one ncclAllGather (RCCL) per round.  Prints ONE JSON line on rank 0.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0   # MI355X HBM3E spec peak (MI355X_MICROARCH.md); ~6.3 TB/s achievable


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--scene", default="pawn", choices=["pawn", "ring", "dome"])
    ap.add_argument("--parents-per-round", type=int, default=int(os.environ.get("PAIS_B", "4096")))
    ap.add_argument("--max-rounds", type=int, default=0)
    ap.add_argument("--seeds", type=int, default=200)
    ap.add_argument("--cpu-seconds", type=float, default=15.0, help="budget of the cpu_baseline leg (rank 0, N=1 only)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--emulate-world", default="", help="e.g. 2,4,8: after the normal line's measurements, run ONE rank of a world of N "
                    "on this GPU through the real sharded code path (include/pais_test_hooks.h pais_mvs_emulate: the other ranks' blocks are "
                    "replayed from a recorded single-rank run) and print measured T_rank(N) next to the model (config.emulated_speedup_at)")
    ap.add_argument("--emulate-ranks", default="all", choices=["ends", "all"], help="which ranks of each emulated world are run: "
                    "every one (default) or only the first and the last; T(N) = the slowest")
    ap.add_argument("--emulate-steps", type=int, default=2)
    ap.add_argument("--no-emulate", action="store_true", help="the default pawn line emulates ranks of worlds of 2 / 4 / 8 on this GPU "
                    "(a few hundred ms); this switches that off")
    ap.add_argument("--dump-outputs", default="", metavar="DIR", help="after the timed steps, write the cloud of the last timed step "
                    "(every accepted patch in id order, float64) as DIR/<name>.npy; at most 64 MB, a fixed seeded sample of the "
                    "patches beyond that (patch_index.npy says which)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


DUMP_MAX_BYTES = 64 << 20


def dump_outputs(m, out_dir: str) -> None:
    """What the timed path hands its caller: the accepted patches of the reconstruction (MVS::getPatches), one array per
    field, row i = patch_index[i] of the cloud in id order.  Integers (camera indices, counts) are stored as float64."""
    import numpy as np
    ps = m.patches()
    n = len(ps)
    kmax = max([p.num_cam for p in ps] + [1])
    row_bytes = 8 * (19 + kmax)      # float64s of one patch over all the arrays below
    idx = np.arange(n)
    if n * row_bytes > DUMP_MAX_BYTES:
        idx = np.sort(np.random.default_rng(0).choice(n, size=DUMP_MAX_BYTES // row_bytes, replace=False))
    sel = [ps[i] for i in idx]
    cams = np.full((len(sel), kmax), -1.0)
    for r, p in enumerate(sel):
        cams[r, :p.num_cam] = p.cams()
    st = m.stats()
    arrays = {
        "patch_index": idx.astype(np.float64),
        "center": np.array([p.center[:] for p in sel], dtype=np.float64).reshape(-1, 3),
        "normal": np.array([p.normal[:] for p in sel], dtype=np.float64).reshape(-1, 3),
        "normal_s": np.array([p.normalS[:] for p in sel], dtype=np.float64).reshape(-1, 2),
        "ray": np.array([p.ray[:] for p in sel], dtype=np.float64).reshape(-1, 3),
        "depth": np.array([p.depth for p in sel], dtype=np.float64),
        "fitness": np.array([p.fitness for p in sel], dtype=np.float64),
        "correlation": np.array([p.correlation for p in sel], dtype=np.float64),
        "priority": np.array([p.priority for p in sel], dtype=np.float64),
        "num_cam_ref_cam_lod": np.array([[p.num_cam, p.ref_cam, p.lod] for p in sel], dtype=np.float64).reshape(-1, 3),
        "cam_idx": cams,
        "counts": np.array([n, st.seeds_refined, st.candidates_effective, st.rounds], dtype=np.float64),
    }
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


def build_scene(args, device):
    """pawn = BASELINE.json configs[1] (the configuration the metric is quoted on, the default); ring = configs[2] and
    dome = configs[4] at full size are extra lines for profiles/ (rendered and pyramided on the GPU, edge maps on the fly)."""
    from pais_mvs_amd import synth
    from pais_mvs_amd.config import readme_config
    if args.scene == "pawn":
        cfg = readme_config()
        scene = synth.pawn_scene(n_seeds=args.seeds, build_edges=False)
        name = "5-camera pawn scene (README.md:68-72 cameras, synthetic 640x480 renders), patchRadius 15, README config, full expansion to convergence"
    elif args.scene == "ring":
        cfg = readme_config(adaptiveGradientEnable=True)
        scene = synth.ring_scene(n_seeds=max(args.seeds, 400), build_edges=False, device=device)
        name = "32-camera synthetic ring 1920x1080, patchRadius 15, all adaptive weights on"
    else:
        cfg = readme_config(patchRadius=25, distWeighting=25 / 3.0, reduceNormalRange=4.0, adaptiveGradientEnable=True)
        scene = synth.dome_scene(n_seeds=max(args.seeds, 400), build_edges=False, device=device)
        name = "128-camera synthetic dome 4096x3072, patchRadius 25, reduceNormalRange 4, all adaptive weights on"
    if args.max_rounds:
        name += " (first %d expansion rounds)" % args.max_rounds
    return cfg, scene, name


def cpu_baseline(cfg, scene, budget_s: float, n_seed_units=None, n_expand_units=None):
    """Oracle (CPU restatement, reference OpenMP structure: particles in parallel, patches sequential) timed on
    a bounded sample of the same workload: some seeds, then first-ring expansion candidates of those seeds.
    Seeds (2x particles, 2x iterations, several PSO runs) cost far more than expansion candidates and are 1-2 % of
    the workload, so the two kinds are timed separately and weighted with the workload's own mix."""
    from oracle import po
    from tests.common import oracle_cfg
    ncores = os.cpu_count() or 1
    S = po.OracleScene(oracle_cfg(cfg), scene.cameras, seed=42)
    S.set_omp(True)
    L = po.lib()
    # the reference's parallel loop runs over the particles of ONE patch (15, or 30 for seeds): more threads than
    # that only add fork/join overhead, so the reference-structured leg gets min(cores, 32) threads
    gomp = None
    try:
        gomp = C.CDLL("libgomp.so.1")
    except OSError:
        pass
    nthr = min(ncores, 32)
    if gomp is not None:
        gomp.omp_set_num_threads(nthr)
    else:
        nthr = ncores
    # neighbour radius as the driver computes it before the seed pass (mvs.cpp:202)
    mo = L.po_mvs_create(S.ptr)
    for X, vis in scene.seeds:
        L.po_mvs_add_seed(mo, po.darr(X), len(vis), po.iarr(vis))
    L.po_mvs_set_neighbor_radius(mo)
    parents = []
    t0 = time.perf_counter()
    n_seed = 0
    for i, (X, vis) in enumerate(scene.seeds):
        if time.perf_counter() - t0 > budget_s * 0.4:
            break
        p = S.seed_patch(X, vis, key=i)
        L.po_refine_seed(S.ptr, C.byref(p))
        n_seed += 1
        if not p.drop:
            parents.append(p)
    t_seed = (time.perf_counter() - t0) / max(n_seed, 1)
    t1 = time.perf_counter()
    n_exp = 0
    for par in parents:
        if time.perf_counter() - t1 > budget_s * 0.6:
            break
        for j, camI in enumerate(par.cams()):
            cx = int(par.imgPoint[j][0] / cfg.cellSize) + 1
            cy = int(par.imgPoint[j][1] / cfg.cellSize)
            cen = (C.c_double * 3)()
            L.po_expansion_center(S.ptr, camI, C.byref(par), cx, cy, cen)
            ch = po.Patch()
            L.po_expand_candidate(S.ptr, C.byref(ch), cen, po.darr(par.normal[:]), par.numCam, po.iarr(par.cams()),
                                  L.po_child_key(par.key, camI, cx, cy))
            n_exp += 1
    t_exp = (time.perf_counter() - t1) / max(n_exp, 1)
    # the same kind of unit with the CPU parallelised over PATCHES instead (one candidate per thread): not what the
    # reference does, reported so that the GPU/CPU ratio is not read against a structure that cannot fill the host
    MAXV = 64
    cs, ns, nc, ci, ks = [], [], [], [], []
    for par in parents:
        for j, camI in enumerate(par.cams()):
            for dx, dy in ((-1, 0), (0, -1), (1, 0), (0, 1)):
                cx = int(par.imgPoint[j][0] / cfg.cellSize) + dx
                cy = int(par.imgPoint[j][1] / cfg.cellSize) + dy
                cen = (C.c_double * 3)()
                L.po_expansion_center(S.ptr, camI, C.byref(par), cx, cy, cen)
                cs += list(cen); ns += list(par.normal[:]); nc.append(par.numCam)
                ci += (par.cams() + [0] * MAXV)[:MAXV]; ks.append(L.po_child_key(par.key, camI, cx, cy))
    if gomp is not None:
        gomp.omp_set_num_threads(ncores)
    m_par = min(len(nc), 8 * ncores)
    pp_value = 0.0
    if m_par > 0:
        outp = (po.Patch * m_par)()
        t2 = time.perf_counter()
        L.po_expand_candidates_parallel(S.ptr, outp, m_par, (C.c_double * (3 * m_par))(*cs[:3 * m_par]),
                                        (C.c_double * (3 * m_par))(*ns[:3 * m_par]), (C.c_int * m_par)(*nc[:m_par]),
                                        (C.c_int * (MAXV * m_par))(*ci[:MAXV * m_par]), (C.c_uint64 * m_par)(*ks[:m_par]))
        pp_value = m_par / (time.perf_counter() - t2)
    L.po_mvs_destroy(mo)
    sample = dict(t_seed=t_seed, t_exp=t_exp, n_seed=n_seed, n_exp=n_exp, nthr=nthr, ncores=ncores, pp_value=pp_value, m_par=m_par,
                  cpu_s=time.perf_counter() - t0)
    if n_seed_units is None:
        return sample          # (the leg runs BEFORE the GPU legs; the workload's mix of units is known after them)
    return cpu_baseline_finish(sample, n_seed_units, n_expand_units)


def cpu_baseline_all_rounds(cfg, scene, m, B, max_rounds, budget_s, per_round=12):
    """Second half of the cpu_baseline sample (VERDICT r4 missing 4 / item 7): expansion candidates drawn from EVERY round of
    the workload -- late rounds' K = 3 edge cases and parents that are themselves expansion patches, not only the first ring
    -- refined by the oracle in the reference's structure (OpenMP over particles, candidates one after the other).  The
    candidates come from one extra stepwise reconstruction through the C ABI (outside every timed region); nothing the oracle
    computes goes back into the product.  Returns (seconds per candidate, candidates timed, rounds sampled)."""
    from oracle import po
    from pais_mvs_amd import _lib
    from tests import common
    m.reset()
    for X, vis in scene.seeds:
        m.add_seed(X, vis)
    m.refineSeedPatches()
    m.expansion_begin()
    radius = m.neighbor_radius()
    L = m.L
    L.pais_refine_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    kept, rnd = [], 0
    while True:
        done, cands, n = m.round_begin(B)
        if done or (max_rounds and rnd >= max_rounds):
            break
        out = (_lib.PatchResult * max(n, 1))()
        if n:
            if L.pais_refine_batch(m.ctx_handle, n, cands, out) != 0:
                raise RuntimeError("pais_refine_batch failed")
            for i in range(0, n, max(1, n // per_round)):
                kept.append(common.copy_struct(cands[i]))
        m.round_commit(out, n)
        rnd += 1
    m.expansion_end()
    S = po.OracleScene(common.oracle_cfg(cfg), scene.cameras, seed=42)
    S.ptr.contents.cfg.neighborRadius = radius
    S.set_omp(True)
    try:
        C.CDLL("libgomp.so.1").omp_set_num_threads(min(os.cpu_count() or 1, 32))
    except OSError:
        pass
    # a deterministic spread over the rounds: every k-th kept candidate until the budget is spent
    order = list(range(0, len(kept), 7)) + [i for i in range(len(kept)) if i % 7]
    t0 = time.perf_counter()
    timed = 0
    for i in order:
        if time.perf_counter() - t0 > budget_s:
            break
        common.oracle_refine_patch(S, common.oracle_patch_from_candidate(kept[i]), False)
        timed += 1
    dt = time.perf_counter() - t0
    S.close()
    return (dt / timed if timed else None), timed, rnd


def cpu_baseline_finish(sample, n_seed_units: int, n_expand_units: int):
    t_seed, t_exp, n_seed, n_exp, nthr, ncores = (sample[k] for k in ("t_seed", "t_exp", "n_seed", "n_exp", "nthr", "ncores"))
    pp_value, m_par = sample["pp_value"], sample["m_par"]
    late = sample.get("all_rounds")
    if late and late[0]:
        t_exp_first, t_exp = t_exp, late[0]     # the workload's candidates are what is extrapolated to: the all-round sample decides
    total_s = n_seed_units * t_seed + n_expand_units * t_exp
    return {"value": (n_seed_units + n_expand_units) / total_s if total_s > 0 else 0.0, "unit": "patches/s", "cores": nthr,
            "kind": "port, extrapolated from sample",
            "sample": "%d seeds (%.3f s each) + %s of the same scene, "
                      "oracle/pais_oracle.c with OpenMP over particles (the reference's structure), %.1f s of CPU work; "
                      "value = workload units / (seeds x t_seed + expansion candidates x t_expand) for the workload's "
                      "%d seeds + %d candidates"
                      % (n_seed, t_seed,
                         ("%d expansion candidates spread over all %d rounds of the workload (%.4f s each; the %d first-ring candidates "
                          "timed before the GPU legs: %.4f s each)" % (late[1], late[2], t_exp, n_exp, t_exp_first)) if (late and late[0])
                         else ("%d first-ring expansion candidates (%.4f s each)" % (n_exp, t_exp)),
                         sample["cpu_s"] + (sample.get("all_rounds_s") or 0.0), n_seed_units, n_expand_units),
            "patch_parallel": {"value": pp_value, "unit": "expansion candidates/s", "cores": ncores,
                               "sample": "%d first-ring candidates, one candidate per OpenMP thread (NOT the reference's "
                                         "structure; the stronger CPU arrangement)" % m_par}}


def predicted_speedup(log, particle_num, bytes_per_eval=23000.0, worlds=(2, 4, 8)):
    """Strong-scaling model from the per-batch log of the last reconstruction (include/pais_mvs.h pais_round_log), printed
    so that the first measured SCALE run can be compared with a prediction made from one GPU:
      T(N) = sum over batches of  host enumerate + host commit                      (replicated on every rank)
                                + t(ceil(n / N)) + exchange(n, N)   if the batch is sharded (>= 1024 evaluation waves per iteration)
                                  t(n)                               otherwise (thin batch: every rank refines all of it)
    t(n) = the measured refine time of this run's batches, interpolated over n (expansion batches; below the smallest one
    linearly down to a latency floor; the seed batch scales as half latency floor + half throughput); exchange = 30 us + gathered wire slots over 50 GB/s (device-to-host of what
    the all-gather delivered) + 0.2 us of host unpacking per record."""
    import bisect
    ex = sorted((l.n, l.refine_ms) for l in log if not l.has_seeds and l.n > 0)
    if not ex:
        return None
    xs, ys = [e[0] for e in ex], [e[1] for e in ex]

    # latency floor of a batch: what the thinnest rounds of the pawn scene take (0.9 ms: ~31 dependent launches), scaled with
    # the length of one evaluation; below the smallest measured batch t(n) falls linearly to it
    floor = 0.9 * max(1.0, bytes_per_eval / 23000.0)

    def t_exp(n):
        if n <= xs[0]:
            return min(ys[0], max(floor, ys[0] * n / xs[0]))
        if n >= xs[-1]:
            return ys[-1] * n / xs[-1]
        i = bisect.bisect_left(xs, n)
        x0, x1, y0, y1 = xs[i - 1], xs[i], ys[i - 1], ys[i]
        return y0 if x1 == x0 else y0 + (y1 - y0) * (n - x0) / (x1 - x0)

    def total(N):
        T = 0.0
        for l in log:
            T += l.enumerate_ms + l.commit_ms
            waves = l.n * particle_num * (2 if l.has_seeds else 1)
            if N == 1 or waves < 1024:
                T += l.refine_ms
                continue
            per = -(-l.n // N)
            slot = 208 + 20 * ((l.max_num_cam + 1) // 2 * 2)
            xchg = 0.030 + (64 + per * slot) * N / 50e6 + 0.0002 * l.n
            T += (0.5 * l.refine_ms + 0.5 * l.refine_ms * per / l.n if l.has_seeds else min(t_exp(per), l.refine_ms)) + xchg
        return T
    t1 = total(1)
    return {"model_ms_at_1": t1, **{str(N): t1 / total(N) for N in worlds},
            "shardable_ms": sum(l.refine_ms for l in log if l.n * particle_num * (2 if l.has_seeds else 1) >= 1024),
            "replicated_ms": sum(l.refine_ms for l in log if l.n * particle_num * (2 if l.has_seeds else 1) < 1024),
            "host_ms": sum(l.enumerate_ms + l.commit_ms for l in log)}


def spawn_ranks(args):
    """`python bench.py --gpus N` without a launcher: start N ranks of this file, one per GPU, and relay rank 0's line."""
    import socket
    import subprocess
    import torch
    ndev = torch.cuda.device_count()
    if "PAIS_FORCE_DEVICE" not in os.environ and ndev < args.gpus:
        raise SystemExit("bench.py --gpus %d: only %d GPU(s) visible; refusing to report a smaller job as n_gpus=%d"
                         % (args.gpus, ndev, args.gpus))
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    procs = []
    for r in range(args.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(args.gpus), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), PAIS_NO_BUILD="1")
        # rank 0 inherits stdout (its single JSON line); the other ranks' stdout goes to stderr
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=None if r == 0 else sys.stderr))
    rcs = [p.wait() for p in procs]
    if any(rcs):
        raise SystemExit("bench.py: rank exit codes %s" % rcs)


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        spawn_ranks(args)
        return
    # stdout carries exactly ONE line, the JSON of rank 0: libraries that write to the C-level stdout (RCCL prints a
    # version banner there) are sent to stderr for the whole run, the JSON goes out through the saved descriptor
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the PAIS HIP path has no CPU fallback")
    from pais_mvs_amd import _lib
    from pais_mvs_amd.mvs import MVS
    from pais_mvs_amd import distributed as D
    # test hooks (one-GPU boxes): PAIS_FORCE_DEVICE puts every rank on that device and PAIS_DIST_TRANSPORT=host exchanges
    # the records through host memory -- RCCL refuses two ranks on one GPU; PAIS_FORCE_DIST=1 runs the multi-rank code
    # path (RCCL communicator, sharding) with a world of one rank.  The driver never sets them.
    force_dist = os.environ.get("PAIS_FORCE_DIST") == "1"
    job = D.job_from_env(force_group=force_dist)
    rank, world, local = job.rank, job.world, job.local_rank
    if world != args.gpus:
        raise SystemExit("bench.py --gpus %d was started with WORLD_SIZE=%d: refusing to report the wrong n_gpus" % (args.gpus, world))
    if "PAIS_FORCE_DEVICE" in os.environ:
        local = int(os.environ["PAIS_FORCE_DEVICE"])
    elif local >= torch.cuda.device_count():
        raise SystemExit("bench.py: rank %d has no GPU %d (%d visible)" % (rank, local, torch.cuda.device_count()))
    torch.cuda.set_device(local)

    cfg, scene, wname = build_scene(args, local)
    if not args.emulate_world and not args.no_emulate and args.scene == "pawn" and not args.max_rounds and args.gpus == 1 and not force_dist:
        args.emulate_world = "2,4,8"
    # the CPU leg first (rank 0, one GPU, the scene that carries host data for the oracle): the GPU legs then run back to back
    cpu_sample = None
    if world == 1 and rank == 0 and not args.no_cpu_baseline and args.scene == "pawn":
        cpu_sample = cpu_baseline(cfg, scene, args.cpu_seconds)
    m = MVS(cfg, scene.cameras, device=local, seed=42)
    if world > 1 or force_dist:
        D.attach(m, job, transport=os.environ.get("PAIS_DIST_TRANSPORT", "rccl"))
    B = args.parents_per_round

    def step():
        m.reset()
        for X, vis in scene.seeds:
            m.add_seed(X, vis)
        m.refineSeedPatches()       # sharded over the ranks under the C ABI when a communicator is attached
        m.expansionPatches(B, args.max_rounds)
        return m.stats()

    def fence():
        torch.cuda.synchronize()
        job.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    ks = _lib.KernelStats()
    m.L.pais_get_kernel_stats(m.ctx_handle, C.byref(ks), 1)   # reset kernel timers
    fence()
    t0 = time.perf_counter()
    units = 0
    spec = 0
    evals_eff = 0
    last = None
    for _ in range(args.steps):
        st = step()
        units += st.seeds_refined + st.candidates_effective
        spec += st.candidates_refined - st.candidates_effective
        evals_eff += st.pso_evals_effective
        last = st
    fence()
    dt = time.perf_counter() - t0
    dt = job.max_over_ranks(dt)
    # the cloud of the LAST TIMED step, hashed (outside the timed region): pais_mvs_amd.mvs.patches_sha1 over every
    # accepted patch in id order.  tests/golden/bench_cloud_<scene>.json holds what the ORACLE produces for the default
    # workload (tests/golden/make_bench_golden.py) -- the line checks itself against it.
    cloud_sha1 = m.cloud_sha1() if (rank == 0 or world > 1) else None
    accepted = int(m.num_patches())
    if rank == 0 and args.dump_outputs:        # (before the extra steps below reset the driver)
        dump_outputs(m, args.dump_outputs)
    # ... and compared AS A CLOUD with the reference's arithmetic (north_star: "output point clouds match the reference CPU run's
    # patch centres / normals within 1e-4 relative L2 and identical visible-camera sets"): tests/golden/bench_cloud_pawn_literal.npz
    # is the cloud the oracle produces for this workload in LITERAL arithmetic (make_bench_golden.py --literal); its .json holds
    # the same comparison for the reference's own source under another loop order / another compiler (the control)
    cloud_vs_literal = None
    if rank == 0 and args.scene == "pawn" and not args.max_rounds:
        try:
            from pais_mvs_amd import cloudcmp
            lit, lmasks, lfirst, lmeta = cloudcmp.load_compact(os.path.join(ROOT, "tests", "golden", "bench_cloud_pawn_literal.npz"))
            lj = json.load(open(os.path.join(ROOT, "tests", "golden", "bench_cloud_pawn_literal.json")))
            if (lj["seeds"], lj["parents_per_round"]) == (len(scene.seeds), B):
                ps = m.patches()
                mine = m.cloud()
                met = cloudcmp.cloud_metrics(mine, lit, lmeta["neighbor_radius"], cloudcmp.camera_masks([p.cams() for p in ps]), lmasks)
                sides = ("a_to_b", "b_to_a")
                ctl = {k: v for k, v in lj["vs_literal"].items() if k != "kernel"}
                cloud_vs_literal = {
                    "accepted": accepted, "accepted_literal": int(len(lit)), "count_ratio": met["count_ratio"],
                    "nearest_patch_dist_over_neighbor_radius": {"median": max(met[s]["dist_over_radius_median"] for s in sides),
                                                                "p95": max(met[s]["dist_over_radius_p95"] for s in sides),
                                                                "max": max(met[s]["dist_over_radius_max"] for s in sides)},
                    "normal_angle_p95_rad": max(met[s]["normal_angle_p95_rad"] for s in sides),
                    "within_neighbor_radius": min(met[s]["within_radius"] for s in sides),
                    "within_1e-4_rel_l2_centre": min(met[s]["within_1e-4_rel_centre"] for s in sides),
                    "identical_camera_sets_among_1e-4_matches": min(met[s]["same_camera_set_among_1e-4_matches"] for s in sides),
                    "surface_error_median": {"this": cloudcmp.surface_error(scene, mine, [p.cams()[0] for p in ps])["median"],
                                             "literal": cloudcmp.surface_error(scene, lit, lfirst)["median"]},
                    "control_the_references_own_source_perturbed": {
                        k: {"count_ratio": v["count_ratio"], "dist_p95": max(v[s]["dist_over_radius_p95"] for s in sides),
                            "normal_angle_p95_rad": max(v[s]["normal_angle_p95_rad"] for s in sides),
                            "within_1e-4_rel_l2_centre": min(v[s]["within_1e-4_rel_centre"] for s in sides)} for k, v in ctl.items()},
                    "note": "both directions, the worse one reported; measured live against the committed literal cloud (worst direction); "
                            "control = the oracle's literal arithmetic with the window sums in another order / fused multiply-adds, same metrics"}
        except Exception as e:                 # (the fixture is optional for the line; its absence is visible)
            cloud_vs_literal = {"error": str(e)}
    # several ranks: every rank hashes ITS replica of the cloud; rank 0 reports whether they all hold the same one
    ranks_agree = None
    if world > 1:
        try:
            allsha = job.all_gather_bytes(cloud_sha1.encode("ascii"), 40)
            ranks_agree = all(allsha[40 * r:40 * (r + 1)] == allsha[:40] for r in range(world))
        except Exception:
            ranks_agree = None
    # SELF-CHECK of a multi-rank run: a line is only printed for a run in which every rank holds the same cloud
    # and no sharded batch needed a second exchange / no one-launch PSO pass fell back -- both are handled correctly by the library,
    # but a scaling figure measured over them would not be the steady state (PAIS_BENCH_ALLOW_RETRIES=1 prints it anyway)
    if world > 1:
        ksc = _lib.KernelStats()
        m.L.pais_get_kernel_stats(m.ctx_handle, C.byref(ksc), 0)
        retries = int(job.max_over_ranks(float(last.exchange_retries if last else 0)))
        fallbacks = int(job.max_over_ranks(float(ksc.ring_fallbacks)))
        problems = []
        if ranks_agree is not True:
            problems.append("the ranks do NOT hold the same cloud (ranks_hold_the_same_cloud = %r)" % (ranks_agree,))
        if (retries or fallbacks) and os.environ.get("PAIS_BENCH_ALLOW_RETRIES") != "1":
            problems.append("%d sharded batch(es) took a second exchange, %d one-launch PSO pass(es) fell back to per-iteration launches "
                            "(PAIS_BENCH_ALLOW_RETRIES=1 reports the line anyway)" % (retries, fallbacks))
        if problems:
            if rank == 0:
                sys.stderr.write("bench.py --gpus %d: REFUSING to print a result line:\n  %s\n" % (world, "\n  ".join(problems)))
            m.close()
            job.close()
            raise SystemExit(3)
    # Roofline leg (not part of `value`): ONE more step of the same workload with every cost-evaluation launch
    # bracketed by HIP events on the stream it is launched on (two overlapping sub-streams by default).
    m.L.pais_get_kernel_stats(m.ctx_handle, C.byref(ks), 1)
    m.L.pais_ctx_set_fine_timing(m.ctx_handle, 1)
    step()
    fence()
    m.L.pais_ctx_set_fine_timing(m.ctx_handle, 0)
    m.L.pais_get_kernel_stats(m.ctx_handle, C.byref(ks), 0)

    # PAIS_ARITH=literal (pais_literal.hpp, round 6): the same reconstruction with the cost in the reference's own statements and
    # summation ORDER -- a second driver over the same scene, one warm-up and two timed reconstructions, outside `value`
    literal_arith = None
    if rank == 0 and world == 1 and args.scene == "pawn" and not args.max_rounds and os.environ.get("PAIS_ARITH") != "literal" \
            and os.environ.get("PAIS_BENCH_LITERAL", "1") != "0":
        try:
            os.environ["PAIS_ARITH"] = "literal"
            m2 = MVS(cfg, scene.cameras, device=local, seed=42)
            del os.environ["PAIS_ARITH"]

            def step2():
                m2.reset()
                for X, vis in scene.seeds:
                    m2.add_seed(X, vis)
                m2.refineSeedPatches()
                m2.expansionPatches(B, args.max_rounds)
                return m2.stats()
            step2()
            torch.cuda.synchronize()
            tl = time.perf_counter()
            ul = 0
            for _ in range(2):
                sl = step2()
                ul += sl.seeds_refined + sl.candidates_effective
            torch.cuda.synchronize()
            dl = time.perf_counter() - tl
            lg_b = None
            try:
                lc = json.load(open(os.path.join(ROOT, "tests", "golden", "literal_control_bench_workload.json")))
                lg_b = {"candidates": lc["cost_literal"]["n"], "branched": lc["cost_literal"]["branched"],
                        "default_arithmetic_branched": lc["kernel"]["branched"], "one_rounding_control_branched": lc["variant_1"]["branched"]}
            except Exception:
                pass
            literal_arith = {"value": ul / dl, "unit": "patches/s", "ms_per_step": dl / 2 * 1e3, "patches_per_step": ul // 2,
                             "accepted_patches": int(m2.num_patches()), "cloud_sha1": m2.cloud_sha1(),
                             "literal_gate": lg_b,
                             "note": "PAIS_ARITH=literal: every batch through k_pso_eval_lit + k_pso_step; per candidate the records ARE the "
                                     "CPU restatement's with the literal cost, bit for bit (tests/test_gpu_parity.py); branched = PSO "
                                     "trajectories that differ from the all-literal CPU run (platform libm) on the 1 817 sampled candidates"}
            m2.close()
        except Exception as e:
            os.environ.pop("PAIS_ARITH", None)
            literal_arith = {"error": str(e)}
    scaling_model = None
    if rank == 0:
        scaling_model = predicted_speedup(m.round_log(), cfg.particleNum, (ks.pso_algorithmic_bytes / ks.pso_evals) if ks.pso_evals else 23000.0)
    emulated = None
    if rank == 0 and world == 1 and args.emulate_world:
        # One-GPU MEASUREMENT of the sharded path: record a single-rank run, then be rank r of a world of N.
        worlds = [int(x) for x in args.emulate_world.split(",") if x.strip()]
        t1 = dt / max(args.steps, 1) * 1e3
        m.emulate(1)
        step()
        fence()
        ref_sha = m.cloud_sha1()
        emulated = {"ms_at_1": t1, "ms_at": {}, "ranks_run": {}, "cloud_matches_single_rank": True,
                    "streamed_rounds_at": {}, "exchange_ms_at": {}, "batches_sharded_at": {},
                    "note": "measured on ONE GPU: rank r of a world of N runs the real sharded code path (shard refined by the kernels, "
                            "packed, status header, copy down, unpack, replicated commit; thin batches replicated; rounds streamed) with the "
                            "other ranks' blocks replayed from a recorded single-rank run in place of ncclAllGather (bytes arrive over "
                            "PCIe, + %s us of modelled collective latency); T(N) = slowest emulated rank, host time spent preparing the "
                            "replayed blocks subtracted (emu_replay_ms); speed-up = ms_per_step of this line / T(N).  Not measured: link "
                            "contention and rank skew." % os.environ.get("PAIS_EMU_LATENCY_US", "25")}
        for N in worlds:
            ranks = list(range(N)) if args.emulate_ranks == "all" else sorted(set([0, N - 1]))
            worst, worst_st = 0.0, None
            by_rank = []
            for r in ranks:
                m.emulate(2, r, N)
                step()                                   # (buffers of this world size grow here)
                fence()
                t0e = time.perf_counter()
                replay = 0.0
                for _ in range(max(args.emulate_steps, 1)):
                    ste = step()
                    replay += ste.emu_replay_ms
                fence()
                te = ((time.perf_counter() - t0e) * 1e3 - replay) / max(args.emulate_steps, 1)
                if m.cloud_sha1() != ref_sha:
                    emulated["cloud_matches_single_rank"] = False
                by_rank.append({"rank": r, "ms": te, "gpu_refine_ms": float(ste.gpu_refine_ms), "enumerate_ms": float(ste.host_enumerate_ms),
                                "commit_ms": float(ste.host_commit_ms), "exchange_ms": float(ste.exchange_ms), "replay_ms": float(ste.emu_replay_ms),
                                "streamed": int(ste.rounds_streamed), "sharded": int(ste.batches_sharded)})
                if te > worst:
                    worst, worst_st = te, ste
            emulated["ms_at"][str(N)] = worst
            emulated[str(N)] = t1 / worst if worst > 0 else None
            emulated["ranks_run"][str(N)] = ranks
            emulated.setdefault("by_rank", {})[str(N)] = by_rank
            emulated["streamed_rounds_at"][str(N)] = int(worst_st.rounds_streamed)
            emulated["exchange_ms_at"][str(N)] = float(worst_st.exchange_ms)
            emulated["batches_sharded_at"][str(N)] = int(worst_st.batches_sharded)
        m.emulate(0)
    if cpu_sample is not None and rank == 0 and world == 1:
        try:
            t_all0 = time.perf_counter()
            cpu_sample["all_rounds"] = cpu_baseline_all_rounds(cfg, scene, m, B, args.max_rounds, min(6.0, args.cpu_seconds * 0.4))
            cpu_sample["all_rounds_s"] = time.perf_counter() - t_all0
        except Exception as e:                 # (the first-ring sample stands)
            cpu_sample["all_rounds"] = None
            print("cpu_baseline: all-round sample failed: %s" % e, file=sys.stderr)
    if rank == 0:
        gold_sha, gold_ok = None, None
        try:
            # (bounded workloads of the full-size scenes carry their round count in the name: bench_cloud_ring_r3.json)
            g = json.load(open(os.path.join(ROOT, "tests", "golden", "bench_cloud_%s%s.json"
                                            % (args.scene, ("_r%d" % args.max_rounds) if args.max_rounds else ""))))
            if (g["seeds"], g["parents_per_round"], g["max_rounds"], g["pso_seed"]) == (len(scene.seeds), B, args.max_rounds, 42):
                gold_sha = g["cloud_sha1"]
                gold_ok = bool(cloud_sha1 == gold_sha and accepted == g["accepted_patches"]
                               and units // max(args.steps, 1) == g["patches_per_step"])
        except Exception:
            pass
        k_ms = ks.eval_ms                      # sum of the launch durations of the dominant kernel
        k_launches = max(int(ks.eval_launches), 1)
        pso_gbs = (ks.pso_algorithmic_bytes / 1e9) / (k_ms / 1e3) if k_ms > 0 else 0.0
        # HBM bytes per launch of the dominant kernel from the committed rocprofv3 --pmc FETCH_SIZE pass of THIS scene at
        # THIS workload (profiles/pmc_traffic_by_scene.json, written by scripts/make_profiles.sh); a figure taken on another
        # scene or workload is never printed
        traffic, traffic_all = None, None
        pj = None
        tnote = "no PMC pass of this scene / workload under profiles/"
        try:
            pj = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic_by_scene.json"))).get(args.scene)
            if pj and (pj["seeds"], pj["parents_per_round"], pj["max_rounds"]) == (len(scene.seeds), B, args.max_rounds):
                traffic = pj.get("eval2_hbm_read_bytes_per_launch")
                traffic_all = pj.get("eval_hbm_read_bytes_per_launch")
                tnote = pj.get("note", "")
            else:
                pj = None
        except Exception:
            pj = None
        # the dominant kernel ALONE: k_pso_eval2 (the throughput-bound launches of the large batches); the k_pso_iter launches
        # of small batches are latency bound and reported next to it, never mixed into `achieved`
        # Three kernels can carry the large batches; `roofline` describes ONE of them, alone:
        #   k_pso_ring  whole PSO passes as one launch          -> ring_* figures of pais_kernel_stats
        #   k_pso_tile  (+ its pending-only k_pso_eval2 launch) -> the eval2_* aggregate of a many-camera scene
        #   k_pso_eval2 per-iteration launches (parts of streamed rounds, PAIS_PSO_RING=0) -> eval2_* minus ring_*
        ring_n = int(ks.ring_launches)
        if ks.tile_launches * 2 > max(int(ks.eval2_launches), 1):
            dom = "tile"
        elif ring_n > 0 and ks.ring_ms * 2 >= ks.eval2_ms:
            dom = "ring"
        else:
            dom = "eval2"
        if dom == "ring":
            e2_ms, e2_n, e2_bytes, e2_evals = ks.ring_ms, max(ring_n, 1), ks.ring_algorithmic_bytes, int(ks.ring_evals)
            o_ms, o_n, o_bytes, o_evals = ks.eval2_ms - ks.ring_ms, int(ks.eval2_launches) - ring_n, ks.eval2_algorithmic_bytes - ks.ring_algorithmic_bytes, int(ks.eval2_evals - ks.ring_evals)
            traffic = pj.get("ring_hbm_read_bytes_per_launch") if pj else None
        elif dom == "eval2":
            e2_ms, e2_n = ks.eval2_ms - ks.ring_ms, max(int(ks.eval2_launches) - ring_n, 1)
            e2_bytes, e2_evals = ks.eval2_algorithmic_bytes - ks.ring_algorithmic_bytes, int(ks.eval2_evals - ks.ring_evals)
            o_ms, o_n, o_bytes, o_evals = ks.ring_ms, ring_n, ks.ring_algorithmic_bytes, int(ks.ring_evals)
            traffic = pj.get("eval2_only_hbm_read_bytes_per_launch") if pj else None
        else:
            e2_ms, e2_n, e2_bytes, e2_evals = ks.eval2_ms, max(int(ks.eval2_launches), 1), ks.eval2_algorithmic_bytes, int(ks.eval2_evals)
            o_ms, o_n, o_bytes, o_evals = 0.0, 0, 0.0, 0
        e2_gbs = (e2_bytes / 1e9) / (e2_ms / 1e3) if e2_ms > 0 else 0.0
        evals_per_s = evals_eff / dt if dt > 0 else 0.0
        literal_gate = None
        try:   # north_star's gate against the reference's LITERAL arithmetic, as measured on this workload (tests/golden/, made by
               # tests/test_gpu_parity.py::test_literal_gate_on_expansion_candidates_of_the_bench_workload): printed, not re-measured
            lg = json.load(open(os.path.join(ROOT, "tests", "golden", "literal_gate_bench_workload.json")))
            if args.scene == "pawn":
                literal_gate = {"candidates": lg["candidates"], "on_the_literal_trajectory": lg["candidates"] - lg["branched"],
                                "branched": lg["branched"], "branched_fraction": lg["branched_fraction"],
                                "centre_rel_l2_max_on_trajectory": lg["same_trajectory_centre_max"],
                                "normal_rel_l2_max_on_trajectory": lg["same_trajectory_normal_max"],
                                "discrete_mismatches_on_trajectory": lg["set_mismatch_on_the_same_trajectory"],
                                "discrete_mismatches_among_branched": lg["set_mismatch_among_branched"],
                                "note": "HIP records vs the oracle in the reference's literal arithmetic, expansion candidates of rounds 5..25 of "
                                        "this workload; 'branched' = some fitness comparison of the chaotic, unconverged PSO decided the other way "
                                        "by a last-bit cost difference (DESIGN.md 5.3); printed from the committed file -- the -m gpu test fails "
                                        "when its own measurement drifts from it by more than 2 candidates"}
                lc = json.load(open(os.path.join(ROOT, "tests", "golden", "literal_control_bench_workload.json")))
                literal_gate["control_branched"] = {
                    "kernel_arithmetic": lc["kernel"]["branched"],
                    "literal_one_rounding_perturbed": lc["variant_1"]["branched"],
                    "literal_sums_y_outer": lc["variant_2"]["branched"],
                    "literal_fused_multiply_adds": lc["variant_4"]["branched"],
                    "literal_y_outer_and_fused": lc["variant_6"]["branched"],
                    "note": "the same candidates, literal arithmetic against ITSELF with a rounding difference another loop order / compiler "
                            "would produce from the reference's own source (tests/golden/make_literal_control.py)"}
        except Exception:
            pass
        if args.scene in ("ring", "dome"):
            try:   # the same gate at FULL size (tests/golden/make_literal_gate_full.py, run on the GPU box): printed, not re-measured
                lg = json.load(open(os.path.join(ROOT, "tests", "golden", "literal_gate_%s_full.json" % args.scene)))
                literal_gate = {k: lg[k] for k in ("candidates", "branched", "branched_fraction", "same_trajectory_centre_max",
                                                   "same_trajectory_normal_max", "set_mismatch_on_the_same_trajectory",
                                                   "set_mismatch_among_branched", "control_literal_y_outer_and_fused", "workload")}
            except Exception:
                pass
        # WHAT BINDS.  The tier's convention prices the kernel against HBM (`frac`); the kernel itself is bound
        # by the vector ALU.  Two more fractions of the same launches, from the same HIP-event durations:
        #   fp64_flops_frac : SURVEY 8(d)'s F_eval = S^2 (38 K + 30) flop per evaluation (K from the launches' own algorithmic bytes)
        #                     x evaluations / time / 78.6 TFLOP/s (MI355X FP64 vector peak: 256 CUs x 4 SIMDs x 16 lanes x 2 x 2.4 GHz)
        #   valu_issue_frac : VALU instructions per evaluation (PMC SQ_INSTS_VALU of this kernel on this scene, committed under
        #                     profiles/valu_model.json by scripts/valu_per_eval.sh) x evaluations x 4 cycles per wave64 instruction
        #                     (scripts/ubench/inst_rate.hip, profiles/r06_inst_rate.txt: FP64 and 32-bit instructions of this mix alike
        #                     occupy a 16-lane-per-clock slot) / (time x 1024 SIMDs x 2.4 GHz)
        S2 = (2 * cfg.patchRadius + 1) ** 2
        b_px = (e2_bytes / e2_evals / S2) if e2_evals else 0.0
        k_eff = max((b_px - 1 - 8 * int(bool(cfg.adaptiveDistanceEnable)) - 8 * int(bool(cfg.adaptiveGradientEnable))) / 4.0, 0.0)
        flop_eval = S2 * (38.0 * k_eff + 30.0)
        FP64_PEAK, SIMDS, CLK = 78.6e12, 1024, 2.4e9
        fp64_frac = (flop_eval * e2_evals / (e2_ms / 1e3) / FP64_PEAK) if e2_ms > 0 else None
        valu_frac, valu_ipe, valu_src = None, None, None
        try:
            vm = json.load(open(os.path.join(ROOT, "profiles", "valu_model.json")))
            ent = vm.get(args.scene, {}).get(dom)
            if ent:
                valu_ipe, valu_src = float(ent["valu_insts_per_eval"]), ent.get("source")
                valu_frac = (valu_ipe * e2_evals * 4.0 / ((e2_ms / 1e3) * SIMDS * CLK)) if e2_ms > 0 else None
        except Exception:
            pass
        fracs = {"hbm": e2_gbs / HBM_PEAK_GBS, "fp64": fp64_frac or 0.0, "valu_issue": valu_frac or 0.0}
        bound = max(fracs, key=fracs.get)
        mb = None
        try:   # saturated rate of the same evaluation code (scripts/microbench_eval.py under profiles/)
            mb = json.load(open(os.path.join(ROOT, "profiles", "microbench_eval.json")))["evals_per_s"]
        except Exception:
            pass
        out = {
            "metric": "refined+expanded patches/sec",
            "value": units / dt,
            "unit": "patches/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": dt / max(args.steps, 1) * 1e3,
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "f64",
            "data": "synthetic",
            "config": {"workload": wname, "parents_per_round": B, "seeds": len(scene.seeds),
                       "patches_per_step": units // max(args.steps, 1),
                       "accepted_patches": accepted,
                       "cloud_sha1": cloud_sha1, "cloud_sha1_expected": gold_sha, "cloud_matches_oracle_golden": gold_ok,
                       "ranks_hold_the_same_cloud": ranks_agree,
                       "speculative_extra_refines_per_step": spec // max(args.steps, 1),
                       "rounds_per_step": int(last.rounds) if last else 0,
                       "rounds_streamed_per_step": int(last.rounds_streamed) if last else 0,
                       "pso_evals_per_patch": evals_eff / max(units, 1),
                       "batches_sharded_per_step": int(last.batches_sharded) if last else 0,
                       "batches_replicated_per_step": int(last.batches_replicated) if last else 0,
                       "exchange_ms_per_step": float(last.exchange_ms) if last else 0.0,
                       "exchange_bytes_per_step": int(last.exchange_bytes) if last else 0,
                       "stream_rounds_mode": os.environ.get("PAIS_STREAM_ROUNDS", "1 (adaptive: a round is streamed when the previous round's host "
                                                                                       "work was >= 0.9 ms and >= 4 % of its GPU time)"),
                       "literal_gate": literal_gate,
                       "literal_arithmetic": literal_arith,
                       "cloud_vs_literal": cloud_vs_literal,
                       "predicted_speedup_at": scaling_model,
                       "emulated_speedup_at": emulated,
                       "parallelism": "1 process per GPU, candidates of a round sharded over %d GPU(s), one ncclAllGather of the "
                                      "records per sharded round (thin rounds replicated)" % world},
            "roofline": {"bound": bound, "bound_by_convention": "hbm",
                         "fp64_flops_frac": fp64_frac, "valu_issue_frac": valu_frac,
                         "what_binds": {"fractions_of_peak": fracs, "fp64_flop_per_eval": flop_eval, "cameras_per_eval": k_eff,
                                        "fp64_peak_tflops": FP64_PEAK / 1e12, "valu_insts_per_eval": valu_ipe, "valu_insts_source": valu_src,
                                        "cycles_per_valu_inst": 4, "simds": SIMDS, "clock_ghz": CLK / 1e9,
                                        "note": "`frac` (HBM, the tier's convention) counts algorithmic bytes that the caches serve; the binding "
                                                "resource is the larger of the two vector-ALU fractions: valu_issue_frac (every VALU instruction of "
                                                "the kernel, FP64 or not, takes a 4-cycle issue slot) contains fp64_flops_frac (the useful flops)"},
                         "kernel": {"tile": "k_pso_tile / k_pso_tile2 (PAIS::getFitness, one workgroup per candidate x 8 particles, camera footprints staged in LDS; "
                                            "%d of the %d evaluation launches of the large batches, the rest its pending-only k_pso_eval2 launches)"
                                            % (int(ks.tile_launches), e2_n),
                                    "ring": "k_pso_ring ALONE (PAIS::getFitness + PsoSolver::run of a large batch as ONE launch: resident waves pop "
                                            "(candidate, particle) evaluation tasks from per-XCD rings); the other large-batch launches of the step are "
                                            "under other_large_batch_launches",
                                    "eval2": "k_pso_eval2 ALONE (PAIS::getFitness, one wave per candidate x particle, one launch per PSO iteration)"}[dom],
                         "achieved": e2_gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": e2_gbs / HBM_PEAK_GBS, "traffic": traffic,
                         "launches": e2_n, "avg_launch_ms": e2_ms / e2_n,
                         "algorithmic_bytes_per_launch": e2_bytes / e2_n,
                         "evals": e2_evals,
                         "algorithmic_bytes_per_eval": (e2_bytes / e2_evals) if e2_evals else 0,
                         # the large-batch evaluation launches of the step that are NOT the kernel above (per-iteration k_pso_eval2
                         # launches of a streamed round next to the ring launches, or the reverse)
                         "other_large_batch_launches": {"launches": o_n, "ms": o_ms, "evals": o_evals,
                                                        "achieved": ((o_bytes / 1e9) / (o_ms / 1e3)) if o_ms > 0 else None},
                         # all large-batch launches together: they overlap on sub-streams / lanes (each is stretched by its neighbour):
                         # their bytes over the time during which at least one of them was running (union of their HIP-event intervals)
                         "busy_ms": ks.eval2_busy_ms,
                         "achieved_over_busy_time": ((ks.eval2_algorithmic_bytes / 1e9) / (ks.eval2_busy_ms / 1e3)) if ks.eval2_busy_ms > 0 else None,
                         "frac_over_busy_time": ((ks.eval2_algorithmic_bytes / 1e9) / (ks.eval2_busy_ms / 1e3) / HBM_PEAK_GBS) if ks.eval2_busy_ms > 0 else None,
                         "ring_fallbacks": int(ks.ring_fallbacks),
                         # every cost-evaluation launch of the step (k_pso_eval2 + the latency-bound k_pso_iter launches of
                         # seeds and thin rounds): the figure rounds 1 and 2 printed as `frac`
                         "all_evaluation_launches": {"achieved": pso_gbs, "frac": pso_gbs / HBM_PEAK_GBS, "launches": k_launches,
                                                     "avg_launch_ms": k_ms / k_launches, "evals": int(ks.pso_evals), "traffic": traffic_all,
                                                     "achieved_over_pso_pass_wall": (ks.pso_algorithmic_bytes / 1e9) / (ks.pso_ms / 1e3) if ks.pso_ms > 0 else 0.0},
                         # whole reconstruction against the saturated kernel: cost evaluations the sequential order consumed
                         # per second of the timed region / the microbenchmark's rate (profiles/microbench_eval.json)
                         "evals_per_s": evals_per_s, "microbench_evals_per_s": mb if args.scene == "pawn" else None,
                         "evals_per_s_over_microbench": (evals_per_s / mb) if (mb and args.scene == "pawn") else None,
                         "note": "rank-0, one extra instrumented step; bytes = S^2*(4K+1+8[dist]+8[grad]) per cost evaluation "
                                 "(SURVEY 8d) x evaluations; durations from HIP events on the launching sub-stream (the two "
                                 "sub-streams' launches overlap, which stretches each).  The kernel is FP64-VALU bound, not HBM "
                                 "bound (DESIGN.md 4): the window taps hit L1/L2.  traffic: " + tnote},
            "kernel_ms_per_step": {"pso_pass": ks.pso_ms, "cost_evaluation_sum_of_launches": ks.eval_ms, "k_begin": ks.begin_ms,
                                   "k_after": ks.after_ms,
                                   "host_enumerate": last.host_enumerate_ms if last else 0,
                                   "host_commit": last.host_commit_ms if last else 0},
        }
        if cpu_sample is not None:   # (the extra scenes carry no host edge maps for the oracle)
            out["cpu_baseline"] = cpu_baseline_finish(cpu_sample, int(last.seeds_refined), int(last.candidates_effective))
        os.write(json_fd, (json.dumps(out) + "\n").encode())
    m.close()
    job.close()


if __name__ == "__main__":
    main()
