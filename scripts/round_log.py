#!/usr/bin/env python
"""Per-round host-side log of one pawn reconstruction (pais_mvs_get_round_log): candidates, refine ms -- under the current
environment.  python scripts/round_log.py [label] [--ring-parts P] [--ring-part-fill F]
--ring-parts 1|2|4: every k_pso_ring launch runs that many waves per evaluation; --ring-part-fill F: the fill factor of the
library's own choice (pais_test_set_ring_parts, include/pais_test_hooks.h) -- the sweeps of profiles/ring_parts_ab.txt."""
import os, sys, json, ctypes
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pais_mvs_amd import synth
from pais_mvs_amd.config import readme_config
from pais_mvs_amd.mvs import MVS
import time
cfg = readme_config()
scene = synth.pawn_scene(n_seeds=200, build_edges=False)
m = MVS(cfg, scene.cameras, device=0, seed=42)
def _opt(name, kind, default):
    if name in sys.argv:
        i = sys.argv.index(name)
        v = kind(sys.argv[i + 1])
        del sys.argv[i:i + 2]
        return v
    return default
ring_parts, ring_fill = _opt("--ring-parts", int, 0), _opt("--ring-part-fill", float, 0.0)
if ring_parts or ring_fill:  # (before the first round: the lanes an MVS forks inherit it)
    assert m.L.pais_test_set_ring_parts(ctypes.c_void_p(m.ctx_handle), ctypes.c_int(ring_parts), ctypes.c_double(ring_fill)) == 0
def step():
    m.reset()
    for X, vis in scene.seeds:
        m.add_seed(X, vis)
    m.refineSeedPatches()
    m.expansionPatches(4096, 0)
for _ in range(2):
    step()
best = None
for _ in range(5):
    t0 = time.perf_counter(); step(); dt = time.perf_counter() - t0
    log = [(l.n, l.has_seeds, l.refine_ms) for l in m.round_log()]
    if best is None or dt < best[0]:
        best = (dt, log)
dt, log = best
thin = sum(ms for n, s, ms in log if not s and n <= 130)
med = sum(ms for n, s, ms in log if not s and 130 < n <= 600)
big = sum(ms for n, s, ms in log if not s and n > 600)
seed = sum(ms for n, s, ms in log if s)
by_parts = (ctypes.c_int64 * 3)()
m.L.pais_test_ring_parts_launches(ctypes.c_void_p(m.ctx_handle), by_parts)
print(json.dumps({"label": sys.argv[1] if len(sys.argv) > 1 else "", "ring_launches_of_1_2_4_parts": list(by_parts), "ms": dt * 1e3, "sha": m.cloud_sha1()[:10], "seed_ms": seed, "thin_ms": thin, "thin_rounds": sum(1 for n, s, ms in log if not s and n <= 130),
                  "medium_ms": med, "medium_rounds": sum(1 for n, s, ms in log if not s and 130 < n <= 600), "large_ms": big,
                  "rounds": [(n, round(ms, 3)) for n, s, ms in log if not s]}))
m.close()
