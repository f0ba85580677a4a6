"""The one place where the GPU tests name an evaluation pipeline and run something under it.

KNOBS is every PAIS_* environment variable the native library reads (tests/test_pipelines_cpu.py holds it to the sources).
knobs() starts a run from ALL of them unset, so "default" means the same in every test whatever an earlier test or the
machine left in the environment.  The constants below are the env dicts that select a pipeline; combine them with
dict(A, **B).  assert_took() is the kernel_stats check that the pipeline meant did run.
"""
import contextlib

KNOBS = (
    # read by pais_ctx_create and again by every pais_ctx_fork_lane, which an MVS calls during its rounds (pais_capi.hip;
    # PAIS_TAP_FLOAT_MAX_MB by pais_ctx_create alone: the lanes share the uploaded scene)
    "PAIS_ARITH", "PAIS_EVAL_PARTS", "PAIS_FINE_TIMING", "PAIS_PART_FILL", "PAIS_PRE_SETUP", "PAIS_PSO_MINPER", "PAIS_PSO_RING",
    "PAIS_PSO_STREAMS", "PAIS_RING_MAX_MB", "PAIS_RING_PER_CAM", "PAIS_RING_SEED_ABOVE", "PAIS_RING_TIMEOUT_MS", "PAIS_SPLIT_ABOVE",
    "PAIS_TAP_FLOAT_MAX_MB", "PAIS_TILE", "PAIS_TILE_ABOVE", "PAIS_TILE_DEBUG", "PAIS_TILE_NOTILES", "PAIS_TILE_STRIP_SPLIT",
    "PAIS_TILE_VERIFY",
    # read once by pais_mvs_create (pais_mvs.hip)
    "PAIS_CELL_BLOCK", "PAIS_HOST_SCENE_TEST", "PAIS_SHARD_ENUM", "PAIS_SHARD_ENUM_ABOVE", "PAIS_SHARD_STRIDED", "PAIS_STREAM_ABOVE",
    "PAIS_STREAM_CANARY", "PAIS_STREAM_FIRST", "PAIS_STREAM_HEAD", "PAIS_STREAM_HOST_MS", "PAIS_STREAM_HOST_SHARE",
    "PAIS_STREAM_PARTS", "PAIS_STREAM_ROUNDS", "PAIS_STREAM_SHARDED", "PAIS_STREAM_SPLIT", "PAIS_STREAM_STEP", "PAIS_THIN_FRONT",
    # read by the call that uses them
    "PAIS_CLOUD_CHUNK", "PAIS_CLOUD_SLICES", "PAIS_DETAIL_STAGING_MB", "PAIS_EMU_LATENCY_US", "PAIS_FEATURE_CANDS",
    "PAIS_LOAD_STAGING_MB", "PAIS_RENDER_SPLATS", "PAIS_RENDER_VIEWS", "PAIS_RING_VERBOSE", "PAIS_STREAM_CANARY_LOG",
    "PAIS_TRACE_STAGING_MB", "PAIS_UNDISTORT_POINTS", "PAIS_UNDISTORT_ROWS",
)

SPLIT = {"PAIS_SPLIT_ABOVE": "1"}                               # every batch takes the large-batch pipeline, whatever its size
ITER = {"PAIS_PSO_RING": "0"}                                   # k_pso_iter while the batch is small and the swarm fits a wave
EVAL2 = dict(SPLIT, PAIS_PSO_RING="0")                          # k_pso_eval2 + k_pso_step, one launch pair per iteration
RING_ANY_BATCH = dict(SPLIT, PAIS_RING_PER_CAM="0")             # no size threshold on the ring; whether it runs is the default's
RING_SMALL_BATCH = dict(RING_ANY_BATCH, PAIS_PSO_RING="1")      # k_pso_ring for a batch of expansion candidates of any size
SEED_RING = {"PAIS_RING_SEED_ABOVE": "1"}                       # k_pso_ring for every pass of a batch that holds seeds
RING = dict(RING_SMALL_BATCH, **SEED_RING)                      # k_pso_ring for any batch, seeds or not
TILE = {"PAIS_TILE": "2", "PAIS_TILE_ABOVE": "1"}               # k_pso_tile2 for a many-camera batch of any size
TILE_VERIFIED = dict(TILE, PAIS_TILE_VERIFY="1")                # ... every particle also through k_pso_eval2 ("tile verify" lines)
NO_TILE = {"PAIS_TILE": "0"}                                    # the one-wave-per-evaluation kernels at any camera count
LITERAL = {"PAIS_ARITH": "literal"}                             # the cost in the reference's statements and summation order
BYTE_TAPS = {"PAIS_TAP_FLOAT_MAX_MB": "0"}                      # the BYTES instantiations: taps from the byte blob, no float copy
SLICED = {"PAIS_PSO_MINPER": "2", "PAIS_PSO_STREAMS": "3"}      # the batch cut into slices of >= 2 candidates on 3 streams
NO_PRE = {"PAIS_PRE_SETUP": "0"}                                # the kernels whose evaluation waves compute their own set-up
NO_TILES = {"PAIS_TILE_NOTILES": "1"}                           # k_pso_tile2 without any tile area
NO_PATIENCE = {"PAIS_RING_TIMEOUT_MS": "0"}                     # the first ring wave that waits gives up: the fallback re-run

_open = []


@contextlib.contextmanager
def knobs(monkeypatch, env):
    """Every name of KNOBS unset, then exactly `env` set; on exit env's names unset again.  All through monkeypatch, so the
    caller's environment returns at teardown.  A key outside KNOBS is refused (a misspelt knob would do nothing), and so is
    nested use (the inner block's exit would leave the outer one without its knobs)."""
    assert not _open, ("knobs() does not nest", _open[-1], env)
    unknown = sorted(set(env) - set(KNOBS))
    assert not unknown, ("not a knob of the library", unknown)
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _open.append(env)
    try:
        yield
    finally:
        _open.pop()
        for k in env:
            monkeypatch.delenv(k, raising=False)


def context(cfg, cameras, monkeypatch=None, env=None):
    """Context(cfg, cameras, device=0, seed=42), created inside knobs(monkeypatch, env) when env is given.  pais_ctx_create
    reads the context-level knobs, so a context used on its own keeps its pipeline after the block.  A lane reads them AGAIN
    when it is forked (pais_ctx_fork_lane), and an MVS forks lanes during expansionPatches: the env of an MVS must stay set
    for its whole run, `with knobs(...)` from MVS(...) to close().  Knobs read per call (PAIS_CLOUD_*, PAIS_RENDER_*,
    PAIS_UNDISTORT_*, PAIS_FEATURE_CANDS, the PAIS_*_STAGING_MB sizes) hold only inside a `with knobs(...)` around the call."""
    from pais_mvs_amd.context import Context
    if env is None:
        return Context(cfg, cameras, device=0, seed=42)
    with knobs(monkeypatch, env):
        return Context(cfg, cameras, device=0, seed=42)


def refine(monkeypatch, cfg, cameras, cands, env):
    """refine_batch of cands on a fresh context under env -> (records, kernel_stats); the context is closed."""
    with knobs(monkeypatch, env):
        c = context(cfg, cameras)
        out = c.refine_batch(cands)
        ks = c.kernel_stats()
        c.close()
    return out, ks


def fitness(monkeypatch, cfg, cameras, states, idx, parts, env):
    """fitness_batch on a fresh context under env -> the array of costs; the context is closed."""
    with knobs(monkeypatch, env):
        c = context(cfg, cameras)
        out = c.fitness_batch(states, idx, parts)
        c.close()
    return out


def assert_took(kind, ks, what):
    """The kernel statistics of a run show the pipeline `kind` (iter, eval2, ring, tile).  Only what holds at every site:
    exact launch counts and relations between counters stay with the test that knows them."""
    if kind == "iter":
        assert ks.ring_launches == 0, (what, ks.ring_launches)
    elif kind == "eval2":
        assert ks.eval2_launches > 0 and ks.ring_launches == 0, (what, ks.eval2_launches, ks.ring_launches)
    elif kind == "ring":
        assert ks.ring_launches >= 1 and ks.ring_fallbacks == 0, (what, ks.ring_launches, ks.ring_fallbacks)
    elif kind == "tile":
        assert ks.tile_launches > 0, what
    else:
        raise ValueError(kind)
