"""Resume from an .mvs cloud (`-r file.mvs`, TMVS.cpp:87-88): the loader constructor on the GPU (pais_load_state_batch), the driver's
pais_mvs_load_patches / pais_mvs_set_checkpoint, and the verb, against the oracle -- bit for bit, no tolerance anywhere.

The oracle runs in kernel arithmetic, as in tests/test_gpu_parity.py.  Two deviations of its po_mvs_load_patch are handled here:
it clears `drop` at its end (the reference leaves it set: `dropped` is checked against the branch each record was built for,
tests/golden/make_resume_cloud.py classify) and it marks the patch expanded (a convenience of the filter verbs: cleared through
the pointer po_mvs_get_patch returns before the oracle re-refines / expands).

The cloud of the loader test is in two parts, because a record's LOD is a property of the scene's images: the pawn part (a bounded
reconstruction made by this library + the hand-picked records of tests/golden/resume_cloud.json) is loaded into the pawn scene,
the low-texture part (the scene of test_low_texture_scene_runs_the_upper_pyramid_levels_end_to_end: its refined seeds + the same
hand-picked kinds) into the low-texture scene.

Oracle time of this file on 8 host cores: re-refinement of the 213-patch cloud 5.5 s, 4 resumed rounds 2.3 s, the loader
records < 0.1 s; computed once per module.  The whole file on the MI355X box (16 host cores): 3.4 s, 1.4 s of it the oracle."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from tests import common, pipelines as P
from tests.golden import make_resume_cloud as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "resume_cloud.json")))["scenes"]
B, FIRST_ROUNDS, RESUME_ROUNDS = 16, 2, 4


def _cfg():
    from pais_mvs_amd.config import readme_config
    return readme_config()


def _rec(p):
    """a patch record of an .mvs file from a driver record"""
    return {"kind": "cloud", "center": list(p.center[:]), "normalS": list(p.normalS[:]), "cams": p.cams(), "fitness": p.fitness,
            "correlation": p.correlation}


def _loaded(recs):
    from pais_mvs_amd.context import make_loaded_patch
    return [make_loaded_patch(r["center"], r["normalS"], r["cams"], r["fitness"], r["correlation"]) for r in recs]


@pytest.fixture(scope="module")
def pawn_cloud(pawn_small):
    """(a) the patches of a bounded pawn reconstruction made by this library: seeds + FIRST_ROUNDS rounds of B parents -- a front
    with free neighbouring cells, not a converged cloud"""
    from pais_mvs_amd.mvs import MVS
    m = MVS(_cfg(), pawn_small.cameras, device=0, seed=42)
    for X, vis in pawn_small.seeds:
        m.add_seed(X, vis)
    m.refineSeedPatches()
    m.expansionPatches(B, FIRST_ROUNDS)
    recs = [_rec(p) for p in m.patches()]
    m.close()
    assert len(recs) >= 100, len(recs)
    return recs


def _assert_loader_state(r, p, i, what):
    """every field the constructor defines, except `dropped`"""
    w = (what, i)
    assert r.type == 0 and p.type == 0 and r.stage == 0 and r.key == i == p.key, w
    assert r.num_cam == p.numCam and r.cams() == p.cams(), w
    assert r.ref_cam == p.refCamIdx and r.lod == p.LOD, (w, r.ref_cam, p.refCamIdx, r.lod, p.LOD)
    for name, mine, theirs in (("center", r.center, p.center), ("normal", r.normal, p.normal), ("normalS", r.normalS, p.normalS),
                               ("ray", r.ray, p.ray), ("depthRange", r.depthRange, p.depthRange)):
        assert list(mine[:]) == list(theirs[:]), (w, name, list(mine[:]), list(theirs[:]))
    assert r.depth == p.depth and r.fitness == p.fitness and r.correlation == p.correlation, w
    assert r.priority == p.priority, (w, r.priority, p.priority)
    for k in range(64):
        want = list(p.imgPoint[k][:]) if k < p.numCam else [0.0, 0.0]
        assert list(r.imgPoint[k][:]) == want, (w, k)
    assert r.pso_runs == r.pso_iterations == r.pso_evals == r.ncc_tables == 0, w


@pytest.mark.gpu
@pytest.mark.parametrize("scene_name", ["pawn_small", "pawn_lowtex"])
def test_loader_state_equals_the_oracle(request, scene_name, pawn_cloud, monkeypatch):
    """pais_load_state_batch == po_mvs_load_patch + po_mvs_get_patch in every field, for a cloud that holds (a) the library's own
    pawn reconstruction, (b) records below minCamNum and with no camera, (c) records whose setDepthRange finds no usable camera,
    (d) low-texture records that settle on LOD >= 1, (e) records whose setLOD ends in a `LOD - 1` fallback; once with the
    configuration's neighbour radius and once after set_neighbor_radius; identical under PAIS_ARITH=literal."""
    from oracle import po
    from pais_mvs_amd.context import Context
    scene = request.getfixturevalue(scene_name)
    cfg = _cfg()
    recs = (pawn_cloud if scene_name == "pawn_small" else []) + GOLD[scene_name]
    lps = _loaded(recs)
    S = common.oracle_scene(cfg, scene)
    S.set_kernel_arithmetic(True)
    L = po.lib()
    ctx = Context(cfg, scene.cameras, device=0, seed=42)
    seen = {"lod_up": 0, "fallback": 0, "fallback_up": 0}
    ranges, first = [], None
    for radius in (None, 1e-5):
        if radius is not None:
            ctx.set_neighbor_radius(radius)
        S.ptr.contents.cfg.neighborRadius = cfg.neighborRadius if radius is None else radius
        before = ctx.load_stats()
        out = ctx.load_state_batch(lps)
        after = ctx.load_stats()
        assert after[1] == before[1] + 1 and after[2] == before[2] + len(lps) and after[0] > before[0], (before, after)
        mo = L.po_mvs_create(S.ptr)
        for i, r in enumerate(recs):
            p = G.oracle_load(S, mo, r)
            _assert_loader_state(out[i], p, i, scene_name)
            by, q = G.classify(S, p, r)
            assert bool(out[i].dropped) == (by is not None), (scene_name, i, r["kind"], out[i].dropped, by)
            if radius is None:
                seen[r["kind"]] = seen.get(r["kind"], 0) + 1
                seen[str(by)] = seen.get(str(by), 0) + 1
                seen["lod_up"] += int(by is None and q.LOD >= 1)
                fb = G.lod_fell_back(S, scene, q)
                seen["fallback"] += int(fb)
                seen["fallback_up"] += int(fb and q.LOD >= 1)
        L.po_mvs_destroy(mo)
        ranges.append([list(out[i].depthRange[:]) for i in range(len(recs))])
        if first is None:
            first = bytes(out)
    # the check cannot pass empty: every kind of record is in the cloud and took its branch
    print("\n%s: %d records, %s" % (scene_name, len(recs), seen))
    if scene_name == "pawn_small":
        assert seen["cloud"] == len(pawn_cloud) >= 100                                        # (a)
    else:
        assert seen["seed"] >= 12 and seen["lod_up"] >= 4                                     # (d)
    assert seen["few_cams"] >= 1 and seen["no_cams"] >= 1 and seen["po_set_reference_camera"] >= 2  # (b)
    assert seen["same_cam"] >= 1 and seen["far"] >= 1 and seen["po_set_depth_range"] >= 2     # (c)
    assert seen["border_0"] >= 1 and seen["border_up"] >= 1 and seen["fallback"] >= 2 and seen["fallback_up"] >= 1  # (e)
    assert ranges[0] != ranges[1]          # setDepthRange read the radius the context held at each call
    ctx.close()
    # PAIS_ARITH=literal: none of these statements is in the cost
    ctx = P.context(cfg, scene.cameras, monkeypatch, P.LITERAL)
    assert bytes(ctx.load_state_batch(lps)) == first
    ctx.close()
    S.close()


@pytest.mark.gpu
def test_rejections_launch_nothing_and_chunks_return_the_same_bytes(pawn_small, pawn_cloud, monkeypatch):
    from pais_mvs_amd import _lib
    from pais_mvs_amd.context import Context, make_loaded_patch
    ctx = Context(_cfg(), pawn_small.cameras, device=0, seed=42)
    L = ctx.L
    good = pawn_cloud[0]
    ok = make_loaded_patch(good["center"], good["normalS"], good["cams"], good["fitness"], good["correlation"])
    out = (_lib.PatchResult * 4)()
    ncam = len(pawn_small.cameras)

    def bad(**kw):
        p = common.copy_struct(ok)
        for k, v in kw.items():
            if k == "cam":
                p.cam_idx[v[0]] = v[1]
            else:
                setattr(p, k, v)
        return p

    stats0 = ctx.load_stats()
    cases = [((ctx.h, 2, None, out), "null pointer (in)"),
             ((ctx.h, 2, (_lib.LoadedPatch * 2)(ok, ok), None), "null pointer (out)"),
             ((None, 2, (_lib.LoadedPatch * 2)(ok, ok), out), "null pointer (ctx)"),
             ((ctx.h, -1, (_lib.LoadedPatch * 2)(ok, ok), out), "n < 0"),
             ((ctx.h, 2, (_lib.LoadedPatch * 2)(ok, bad(num_cam=65)), out), "patch 1: num_cam 65 outside [0, 64]"),
             ((ctx.h, 2, (_lib.LoadedPatch * 2)(bad(num_cam=-1), ok), out), "patch 0: num_cam -1 outside [0, 64]"),
             ((ctx.h, 2, (_lib.LoadedPatch * 2)(ok, bad(cam=(1, ncam))), out), "patch 1: cam_idx[1] = %d out of range [0, %d)" % (ncam, ncam)),
             ((ctx.h, 2, (_lib.LoadedPatch * 2)(ok, bad(cam=(0, -1))), out), "patch 1: cam_idx[0] = -1 out of range")]
    for args, msg in cases:
        rc = L.pais_load_state_batch(*args)
        err = L.pais_last_error().decode()
        assert rc < 0 and "pais_load_state_batch" in err and msg in err, (rc, err, msg)
    assert L.pais_load_state_batch(ctx.h, 0, None, None) == 0 and L.pais_load_state_batch(None, 0, None, None) == 0
    assert ctx.load_stats() == stats0                      # nothing was launched
    with pytest.raises(RuntimeError, match="num_cam 65"):
        ctx.load_state_batch([ok, bad(num_cam=65)])
    # a camera below minCamNum is valid input: the reference's drop
    res = ctx.load_state_batch([bad(num_cam=2), bad(num_cam=0)])
    assert res[0].dropped == 1 and res[1].dropped == 1 and res[0].ref_cam == -1 and res[0].lod == -1 and res[0].cams() == good["cams"][:2]
    # chunks: 10 KB of staging hold 5 records (320 + 1488 bytes each)
    lps = _loaded(pawn_cloud[:23] + GOLD["pawn_small"])
    ctx.load_stats(reset=True)
    one = bytes(ctx.load_state_batch(lps))
    assert ctx.load_stats()[1:] == (1, len(lps))
    ctx.load_stats(reset=True)
    with P.knobs(monkeypatch, {"PAIS_LOAD_STAGING_MB": "0.01"}):
        res = ctx.load_state_batch(lps)
    assert ctx.load_stats()[1:] == ((len(lps) + 4) // 5, len(lps))
    assert bytes(res) == one and [res[i].key for i in range(len(lps))] == list(range(len(lps)))
    ctx.close()


def _oracle_rows(L, mo):
    rows = {}
    for i in range(L.po_mvs_num_slots(mo)):
        pp = L.po_mvs_get_patch(mo, i)
        if pp:
            p = pp.contents
            rows[i] = (list(p.center[:]), list(p.normal[:]), p.cams(), p.fitness, p.correlation, p.priority, p.LOD)
    return rows


def _driver_rows(m):
    rows = {}
    for i in range(m.num_slots()):
        p = m.get_patch(i)
        if p is not None:
            rows[i] = (list(p.center[:]), list(p.normal[:]), p.cams(), p.fitness, p.correlation, p.priority, p.lod)
    return rows


@pytest.fixture(scope="module")
def resumed(pawn_small, pawn_cloud):
    """Both sides of the resume, once: load the pawn cloud, re-refine it, continue the expansion for RESUME_ROUNDS rounds of B
    parents with the default thin-front -> {"gpu" / "oracle": (rows after refineSeedPatches, rows after expansionPatches)}"""
    from oracle import po
    from pais_mvs_amd import _lib
    from pais_mvs_amd.mvs import MVS
    cfg = _cfg()
    m = MVS(cfg, pawn_small.cameras, device=0, seed=42)
    first = m.load_patches(_loaded(pawn_cloud))
    assert first == 0 and m.num_slots() == m.num_patches() == len(pawn_cloud)
    loaded = []
    for i in range(m.num_slots()):
        r, e = _lib.PatchResult(), C.c_int(-1)
        assert m.L.pais_mvs_get_patch(m.h, i, C.byref(r), C.byref(e)) == 0
        loaded.append((r, e.value))
    m.refineSeedPatches()
    g1 = _driver_rows(m)
    m.expansionPatches(B, RESUME_ROUNDS)
    g2 = _driver_rows(m)
    st = m.stats()
    m.close()
    S = common.oracle_scene(cfg, pawn_small)
    S.set_kernel_arithmetic(True)
    L = po.lib()
    mo = L.po_mvs_create(S.ptr)
    L.po_mvs_set_parallel(mo, 1)
    for r in pawn_cloud:
        G.oracle_load(S, mo, r).expanded = 0          # the reference's loader does not mark the patch expanded
    L.po_mvs_refine_seed_patches(mo)
    o1 = _oracle_rows(L, mo)
    L.po_mvs_expansion_patches(mo, B, RESUME_ROUNDS, 1)
    o2 = _oracle_rows(L, mo)
    L.po_mvs_destroy(mo)
    S.close()
    return {"gpu": (g1, g2), "oracle": (o1, o2), "loaded": loaded, "inserted": st.patches_inserted, "seeds_refined": st.seeds_refined}


@pytest.mark.gpu
def test_load_patches_stores_the_full_state_unexpanded(pawn_small, pawn_cloud, resumed):
    from pais_mvs_amd.context import Context
    ctx = Context(_cfg(), pawn_small.cameras, device=0, seed=42)
    want = ctx.load_state_batch(_loaded(pawn_cloud))
    for i, (p, expanded) in enumerate(resumed["loaded"]):
        assert bytes(p) == bytes(want[i]) and p.key == i and p.lod >= 0 and p.ref_cam >= 0 and not p.dropped, i
        assert expanded == 0, i
    ctx.close()


@pytest.mark.gpu
def test_re_refinement_of_a_loaded_cloud_equals_the_oracle(pawn_cloud, resumed):
    got, want = resumed["gpu"][0], resumed["oracle"][0]
    assert resumed["seeds_refined"] == len(pawn_cloud)
    assert sorted(got) == sorted(want) and len(got) >= len(pawn_cloud) // 2, (len(got), len(want))
    for i in sorted(want):
        assert got[i] == want[i], (i, got[i], want[i])


@pytest.mark.gpu
def test_resumed_expansion_equals_the_oracle(pawn_cloud, resumed):
    got, want = resumed["gpu"][1], resumed["oracle"][1]
    assert sorted(got) == sorted(want), (len(got), len(want))
    for i in sorted(want):
        assert got[i] == want[i], (i, got[i], want[i])
    assert resumed["inserted"] >= 1 and max(got) >= len(pawn_cloud), (resumed["inserted"], max(got))   # the resumed expansion grew the cloud


def _write_nvm2(d, scene):
    from PIL import Image
    lines = ["NVM_V3", "", str(len(scene.cameras))]
    for i, cam in enumerate(scene.cameras):
        name = "cam%d.png" % i
        Image.fromarray(np.repeat(cam.pyramid[0][:, :, None], 3, axis=2)).save(str(d / name))
        lines.append("%s %r %r %r %r %s %s" % (name, float(cam.focal[0]), float(cam.focal[1]), float(cam.principle_point[0]),
                                               float(cam.principle_point[1]), " ".join(repr(float(v)) for v in cam.quaternion),
                                               " ".join(repr(float(v)) for v in cam.center)))
    lines += ["", str(len(scene.seeds))]
    for X, vis in scene.seeds:
        ms = []
        for c in vis:
            cam = scene.cameras[c]
            q = cam.rotation @ np.asarray(X, float) + cam.translation
            u, v = cam.focal[0] * q[0] / q[2] + cam.principle_point[0], cam.focal[1] * q[1] / q[2] + cam.principle_point[1]
            ms.append("%d 0 %r %r" % (c, float(u - cam.width // 2), float(v - cam.height // 2)))
        lines.append("%r %r %r 128 128 128 %d %s" % (float(X[0]), float(X[1]), float(X[2]), len(vis), " ".join(ms)))
    lines += ["", "0"]
    (d / "scene.nvm2").write_text("\n".join(lines) + "\n")
    (d / "config.txt").write_text("particleNum 6\nmaxIteration 8\n")


@pytest.mark.gpu
def test_file_level_resume_from_exp_mvs(tmp_path, pawn_small):
    """`reconstruct scene.nvm2 --max-rounds k`, then `reconstruct exp.mvs --max-rounds k`: the second run's exp.mvs is the file the
    in-process path writes (io.load_mvs -> load_patches -> the same calls); auto_save.mvs appears and loads when the interval is
    small enough, not with --autosave-every 0, and exp.mvs is the same bytes either way."""
    from pais_mvs_amd import io, reconstruct
    from pais_mvs_amd.mvs import MVS
    d = tmp_path
    _write_nvm2(d, pawn_small)
    common_args = ["--config", str(d / "config.txt"), "--parents-per-round", "16", "--max-rounds", "3"]
    reconstruct.main([str(d / "scene.nvm2"), "--out", str(d), "--autosave-every", "0"] + common_args)
    assert not (d / "auto_save.mvs").exists()
    n_first = len(io.load_mvs(str(d / "exp.mvs"))[2])
    assert n_first > len(pawn_small.seeds) // 2
    outs = {}
    for every in (20, 0):
        o = d / ("resume%d" % every)
        o.mkdir()
        reconstruct.main([str(d / "exp.mvs"), "--out", str(o), "--autosave-every", str(every)] + common_args)
        for f in ("seed.mvs", "exp.mvs", "exp.ply", "exp.psr"):
            assert (o / f).stat().st_size > 0
        outs[every] = (o / "exp.mvs").read_bytes()
    assert outs[20] == outs[0]
    assert not (d / "resume0" / "auto_save.mvs").exists()
    saved = io.load_mvs(str(d / "resume20" / "auto_save.mvs"))
    n_resumed = len(io.load_mvs(str(d / "resume20" / "exp.mvs"))[2])
    assert len(saved[1]) == len(pawn_small.cameras) and 20 <= len(saved[2]) <= n_resumed and n_resumed > 20
    # the in-process path
    file_cfg, cams_io, pats = io.load_mvs(str(d / "exp.mvs"))
    assert file_cfg is not None and len(pats) == n_first
    cfg = io.load_config(str(d / "config.txt"), file_cfg)
    m = MVS(cfg, reconstruct.load_cameras(cams_io, str(d), cfg), device=0)
    m.load_patches(pats)
    m.refineSeedPatches()
    m.expansionPatches(16, 3)
    m.writeMVS(str(d / "inproc.mvs"))
    m.close()
    assert (d / "inproc.mvs").read_bytes() == outs[0]


@pytest.mark.gpu
def test_checkpoint_rule(pawn_small, pawn_cloud):
    """pais_mvs_set_checkpoint: a counting callback is called exactly when the rule says so, given the patch counts after every
    round; a callback returning 7 stops expansionPatches with 7; the records are those of a run without a callback."""
    from pais_mvs_amd.mvs import MVS, CheckpointAbort
    lps = _loaded(pawn_cloud)

    def run(every, fn):
        m = MVS(_cfg(), pawn_small.cameras, device=0, seed=42)
        m.load_patches(lps)
        m.set_checkpoint(every, fn)
        try:
            m.expansionPatches(B, RESUME_ROUNDS)
            code = 0
        except CheckpointAbort as e:
            code = e.code
        recs = [bytes(p) for p in m.patches()]
        m.close()
        return code, recs

    code, plain = run(0, None)
    assert code == 0
    per_round = []
    code, recs = run(1, lambda n: per_round.append(n))          # n // 1 exceeds the calls so far after every round
    assert code == 0 and recs == plain and len(per_round) == RESUME_ROUNDS and per_round[-1] == len(plain), per_round
    assert per_round[-1] > per_round[0] >= len(pawn_cloud) - B * RESUME_ROUNDS

    def rule(every):
        want, calls = [], 0
        for n in per_round:
            if n // every > calls:
                calls += 1
                want.append(n)
        return want

    # an interval for which the rule calls after some rounds and not after others
    every = next((e for e in (100, 150, 80, 200, 60, 300) if 2 <= len(rule(e)) < RESUME_ROUNDS), None)
    assert every is not None, per_round
    want = rule(every)
    seen = []
    code, recs = run(every, lambda n: seen.append(n) or 0)
    assert code == 0 and seen == want and recs == plain, (seen, want)
    seen = []
    code, recs = run(every, lambda n: seen.append(n) or (7 if len(seen) == 2 else 0))
    assert code == 7 and seen == want[:2], (code, seen, want)
    off = []
    m_code, recs = run(-5, lambda n: off.append(n))
    assert m_code == 0 and off == [] and recs == plain


# ------------------------------------------------------------------------------------------------------------------ no GPU ---
def test_headers_with_the_resume_entry_points_are_plain_c(tmp_path):
    import glob
    inc = os.path.join(ROOT, "include")
    headers = sorted(os.path.basename(h) for h in glob.glob(os.path.join(inc, "*.h")))
    src = tmp_path / "resume_abi.c"
    src.write_text("".join('#include "%s"\n' % h for h in headers) + """
#include <stdio.h>
#include <string.h>
static int on_checkpoint(void *user, pais_mvs *m, int num_patches) { (void)m; *(int *)user = num_patches; return 0; }
int main(void)
{
    pais_loaded_patch lp;
    pais_patch_result out;
    pais_checkpoint_fn fn = on_checkpoint;
    double ms = -1;
    memset(&lp, 0, sizeof(lp));
    if (sizeof(pais_loaded_patch) != (size_t)pais_sizeof_loaded_patch()) return 2;
    if (pais_load_state_batch(NULL, 0, NULL, NULL) != 0) return 3;
    if (pais_load_state_batch(NULL, 1, &lp, &out) >= 0 || !strstr(pais_last_error(), "ctx")) return 4;
    if (pais_get_load_stats(NULL, &ms, NULL, NULL, 0) >= 0) return 5;
    if (pais_mvs_load_patches(NULL, 1, &lp, NULL) >= 0 || strlen(pais_mvs_last_error()) == 0) return 6;
    if (pais_mvs_set_checkpoint(NULL, 500, fn, NULL) >= 0) return 7;
    printf("ok %d\\n", (int)sizeof(pais_loaded_patch));
    return 0;
}
""")
    lib_dir = os.path.join(ROOT, "pais_mvs_amd", "csrc")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", inc, "-fsyntax-only", str(src)], check=True)
    cpp = tmp_path / "resume_abi.cpp"
    cpp.write_text("".join('#include "%s"\n' % h for h in headers) + "int main() { return (int)sizeof(pais_loaded_patch) - 320; }\n")
    subprocess.run(["g++", "-std=c++11", "-Wall", "-Werror", "-I", inc, "-fsyntax-only", str(cpp)], check=True)
    exe = tmp_path / "resume_abi"
    subprocess.run(["gcc", "-std=c99", "-I", inc, str(src), "-o", str(exe), "-L", lib_dir, "-lpais_hip", "-Wl,-rpath," + lib_dir],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok 320"), (out.returncode, out.stdout, out.stderr)


def test_loaded_patch_mirror_has_the_abi_size():
    from pais_mvs_amd import _lib
    L = _lib.load()
    assert L.pais_sizeof_loaded_patch() == C.sizeof(_lib.LoadedPatch) == 320
    assert _lib.LoadedPatch.cam_idx.offset == 64 and _lib.LoadedPatch.num_cam.offset == 56


def test_load_patches_needs_the_gpu(pawn_small):
    """a scheduler-only driver (device < 0) refuses: the loader state is a HIP kernel, nothing is computed on the host instead"""
    from pais_mvs_amd.mvs import MVS
    m = MVS(_cfg(), pawn_small.cameras, device=-1, seed=42)
    rec = GOLD["pawn_small"][0]
    with pytest.raises(RuntimeError, match="without a GPU context"):
        m.load_patches(_loaded([rec]))
    assert m.num_slots() == 0 and m.num_patches() == 0
    m.set_checkpoint(10, lambda n: 0)        # (needs no GPU)
    m.set_checkpoint(0, None)
    m.close()


def test_reconstruct_dispatches_on_the_mvs_extension(tmp_path, monkeypatch):
    from pais_mvs_amd import reconstruct
    assert [reconstruct.scene_kind(p) for p in ("a/exp.mvs", "auto_save.MVS", "s.nvm", "s.nvm2", "s.NVM2", "mvs.nvm", "x.mvs.nvm")] == \
        ["mvs", "mvs", "nvm", "nvm2", "nvm2", "nvm", "nvm"]
    calls = []

    class Stop(Exception):
        pass

    def fake(kind):
        def f(path, *a, **k):
            calls.append((kind, os.path.basename(path), k))
            raise Stop()
        return f

    monkeypatch.setattr(reconstruct.io, "load_mvs", fake("mvs"))
    monkeypatch.setattr(reconstruct.io, "load_nvm", fake("nvm"))
    for scene in ("seed.mvs", "scene.nvm", "scene.nvm2"):
        with pytest.raises(Stop):
            reconstruct.main([str(tmp_path / scene), "--config", str(tmp_path / "none.txt"), "--out", str(tmp_path)])
    assert calls == [("mvs", "seed.mvs", {}), ("nvm", "scene.nvm", {"nvm2": False}), ("nvm", "scene.nvm2", {"nvm2": True})]
    a = reconstruct.main.__doc__ or reconstruct.__doc__
    assert "--max-rounds" in a and "--autosave-every" in a
