"""pais_ncc_batch: Patch::removeInvisibleCamera (patch.cpp:655-721) of given patch states -- NCC table, region ratios,
reasons and kept cameras -- against the oracle in kernel arithmetic (bit for bit) and against fixture G4
(tests/golden/oracle_ncc_vectors.json, written by tests/golden/make_ncc_golden.py)."""
import ctypes as C
import json

import numpy as np
import pytest

from tests import common, pipelines as P
from tests.golden import make_ncc_golden as G

RTOL_EXACT = 0.0
SCENES = G.SCENES


def _golden():
    with open(G.OUT) as f:
        return json.load(f)


def _oracle(name, scene):
    S = common.oracle_scene(G.scene_config(name), scene)
    S.set_kernel_arithmetic(True)
    S.set_omp(True)
    return S


def _view_state(st):
    from pais_mvs_amd.context import make_view_state
    return make_view_state(st["center"], st["normal"], st["ref"], st["lod"], st["cams"])


def _compare(got, i, want, what):
    """Result i of a Context.ncc_batch (with tables) against an oracle_ncc dict."""
    K = len(want["ratios"])
    assert int(got.dropped[i]) == want["dropped"], (what, got.dropped[i], want["dropped"])
    assert common.same_value(float(got.correlation[i]), want["correlation"], RTOL_EXACT), (what, got.correlation[i], want["correlation"])
    ratios = got.region_ratio[i]
    assert len(ratios) == K
    for k in range(K):
        assert common.same_value(float(ratios[k]), want["ratios"][k], RTOL_EXACT), (what, k, ratios[k], want["ratios"][k])
    if want["dropped"] == G.DROP_SAMPLE:
        return
    assert int(got.max_idx[i]) == want["max_idx"], (what, got.max_idx[i], want["max_idx"])
    assert got.reason[i].tolist() == want["reasons"], (what, got.reason[i].tolist(), want["reasons"])
    assert got.kept[i].tolist() == want["kept"], (what, got.kept[i].tolist(), want["kept"])
    T = got.tables[i]
    for a in range(K):
        for b in range(K):
            assert common.same_value(float(T[a, b]), want["table"][a * K + b], RTOL_EXACT), (what, a, b, T[a, b])


# ------------------------------------------------------------------------------------------------------------- CPU ---
def test_sizeof_view_structs_match_the_ctypes_mirrors():
    from pais_mvs_amd import _lib
    L = _lib.load()
    assert L.pais_sizeof_view_state() == C.sizeof(_lib.ViewState) == 8 * 6 + 4 * 4 + 4 * 64
    assert L.pais_sizeof_view_result() == C.sizeof(_lib.ViewResult) == 8 + 8 * 64 + 4 * 4 + 2 * 4 * 64


def test_view_state_from_record_takes_the_record_fields():
    from pais_mvs_amd import _lib
    from pais_mvs_amd.context import make_view_state, view_state_from_record
    r = _lib.PatchResult()
    r.center[:] = [0.25, -1.5, 3.0]
    r.normal[:] = [0.0, 0.6, -0.8]
    r.ref_cam, r.lod, r.num_cam = 3, 2, 4
    for i, c in enumerate([7, 3, 11, 0]):
        r.cam_idx[i] = c
    r.cam_idx[4] = 99                                  # beyond num_cam: not part of the state
    v = view_state_from_record(r)
    w = make_view_state([0.25, -1.5, 3.0], [0.0, 0.6, -0.8], 3, 2, [7, 3, 11, 0])
    assert bytes(v) == bytes(w)


def test_oracle_reproduces_the_g4_fixture(request):
    """Pins fixture G4 against drift of the oracle's removeInvisibleCamera, table and region ratio."""
    g = _golden()
    n = 0
    seen_reasons, seen_drops = set(), set()
    for name in SCENES:
        scene = request.getfixturevalue(name)
        entry = g["scenes"][name]
        if G.image_sha1(scene) != entry["image_sha1"]:
            pytest.skip("synthetic renderer produced different bytes on this numpy build; vectors not comparable")
        S = _oracle(name, scene)
        for c in entry["cases"]:
            st, want = G.decode_case(c)
            got = G.oracle_ncc(S, st)
            assert G.encode_case(st, got) == c, (name, c["kind"])
            seen_reasons.update(want["reasons"] if want["dropped"] != G.DROP_SAMPLE else [])
            seen_drops.add(want["dropped"])
            n += 1
        S.close()
    assert 150 <= n <= 400, n
    assert seen_reasons == {G.KEEP, G.REGION, G.BACKFACING, G.CORRELATION}, seen_reasons
    assert seen_drops == {0, G.DROP_SAMPLE, G.DROP_MINCAM}, seen_drops


# ------------------------------------------------------------------------------------------------------------- GPU ---
def _ctx(name, scene, monkeypatch=None, env=None):
    return P.context(G.scene_config(name), scene.cameras, monkeypatch, env)


def _gpu_records(ctx, S, scene):
    """refine() of the seeds on the GPU -> the (centre, normal, ref, lod, record cams, seed cams) tuples of
    make_ncc_golden.scene_states."""
    pats, cands = common.seed_candidates(S, scene)
    res = ctx.refine_batch(cands)
    out = []
    for r, (X, vis) in zip(res, scene.seeds):
        if not r.dropped:
            out.append((list(r.center[:]), list(r.normal[:]), r.ref_cam, r.lod, r.cams(), [int(v) for v in vis]))
    return out


@pytest.mark.gpu
def test_ncc_batch_matches_the_oracle(request):
    """States of GPU refine records of the four small scenes, perturbed, cut to subsets, searched for every removal
    reason, moved until a warped sample lies just past dim-1: table, correlation, ratios, maxIdx bit for bit; reasons,
    kept cameras and drop code exactly.  dome_small runs at r = 25 (its warped patches go to the global scratch slab)."""
    seen_reasons, seen_drops, lods, kmax = set(), set(), set(), 0
    for name in SCENES:
        scene = request.getfixturevalue(name)
        S = _oracle(name, scene)
        ctx = _ctx(name, scene)
        records = _gpu_records(ctx, S, scene)
        assert len(records) >= 6, (name, len(records))
        states = G.scene_states(S, scene, records[:12], np.random.default_rng(77 + SCENES.index(name)))
        got = ctx.ncc_batch([_view_state(st) for st in states], tables=True)
        for i, st in enumerate(states):
            want = G.oracle_ncc(S, st)
            _compare(got, i, want, (name, i, st["kind"]))
            seen_drops.add(want["dropped"])
            if want["dropped"] != G.DROP_SAMPLE:
                seen_reasons.update(want["reasons"])
            lods.add(st["lod"])
            kmax = max(kmax, len(st["cams"]))
        ms, launches, nst = ctx.ncc_stats()
        assert launches == 1 and nst == len(states) and ms > 0
        ctx.close()
        S.close()
    assert seen_reasons == {G.KEEP, G.REGION, G.BACKFACING, G.CORRELATION}, seen_reasons
    assert seen_drops == {0, G.DROP_SAMPLE, G.DROP_MINCAM}, seen_drops
    assert max(lods) >= 1 and kmax >= 12, (lods, kmax)


@pytest.mark.gpu
def test_ncc_batch_matches_the_g4_fixture(request):
    g = _golden()
    for name in SCENES:
        scene = request.getfixturevalue(name)
        entry = g["scenes"][name]
        if G.image_sha1(scene) != entry["image_sha1"]:
            pytest.skip("synthetic renderer produced different bytes on this numpy build; vectors not comparable")
        ctx = _ctx(name, scene)
        dec = [G.decode_case(c) for c in entry["cases"]]
        got = ctx.ncc_batch([_view_state(st) for st, _ in dec], tables=True)
        for i, (st, want) in enumerate(dec):
            _compare(got, i, want, (name, i, st["kind"]))
        ctx.close()


def _rows(res):
    return np.frombuffer(res.records, dtype=np.uint8).reshape(len(res), -1)


@pytest.mark.gpu
@pytest.mark.parametrize("name,total", [("pawn_small", 20000), ("dome_small", 1500)])
def test_same_bytes_alone_in_a_batch_and_under_literal_arithmetic(request, monkeypatch, name, total):
    """A state's result record and table are the same bytes whether it is run alone or at any position of a large batch
    (grid-stride over the states; pawn: patches in LDS, dome: the scratch slabs), and with PAIS_ARITH=literal."""
    scene = request.getfixturevalue(name)
    base = [G.decode_case(c)[0] for c in _golden()["scenes"][name]["cases"]]
    vs = [_view_state(st) for st in base]
    ctx = _ctx(name, scene)
    alone = [ctx.ncc_batch([v], tables=True) for v in vs]
    ctx.close()
    ctx = _ctx(name, scene, monkeypatch, P.LITERAL)
    big = [vs[i % len(vs)] for i in range(total)]
    res = ctx.ncc_batch(big, tables=True)
    ctx.close()
    rows = _rows(res)
    for i in range(total):
        a = alone[i % len(vs)]
        assert rows[i].tobytes() == _rows(a)[0].tobytes(), (name, i)
        assert res.tables[i].tobytes() == a.tables[0].tobytes(), (name, i)   # (bytes: a table may hold NaN)


@pytest.mark.gpu
def test_invalid_states_are_rejected_and_the_context_still_works(pawn_small):
    from pais_mvs_amd import _lib
    from pais_mvs_amd.context import make_view_state
    ctx = _ctx("pawn_small", pawn_small)
    st = G.decode_case(_golden()["scenes"]["pawn_small"]["cases"][0])[0]
    good = _view_state(st)
    want = _rows(ctx.ncc_batch([good], tables=True))[0].tobytes()
    ml = pawn_small.cameras[0].max_lod
    nc = len(pawn_small.cameras)

    def bad(**kw):
        d = dict(center=st["center"], normal=st["normal"], ref_cam=st["ref"], lod=st["lod"], cam_idx=st["cams"])
        d.update(kw)
        return make_view_state(**d)

    cases = [(bad(cam_idx=[0]), "num_cam"),
             (bad(cam_idx=[0, nc]), "cam_idx out of range"),
             (bad(cam_idx=[-1, 1]), "cam_idx out of range"),
             (bad(ref_cam=nc), "ref_cam"),
             (bad(ref_cam=-1), "ref_cam"),
             (bad(cam_idx=[0, 1, 0]), "duplicate"),
             (bad(lod=ml + 1), "lod"),
             (bad(lod=-1), "lod")]
    too_many = bad()
    too_many.num_cam = 65
    cases.append((too_many, "num_cam"))
    for v, msg in cases:
        with pytest.raises(RuntimeError, match=msg):
            ctx.ncc_batch([good, v])
    # a table stride below a num_cam
    arr = (_lib.ViewState * 1)(good)
    out = (_lib.ViewResult * 1)()
    tab = (C.c_double * 4)()
    rc = ctx.L.pais_ncc_batch(ctx.h, 1, arr, out, tab, 2 if good.num_cam > 2 else 1)
    assert rc != 0 and b"stride" in ctx.L.pais_last_error()
    assert _rows(ctx.ncc_batch([good], tables=True))[0].tobytes() == want
    ctx.close()


@pytest.mark.gpu
def test_sixty_four_cameras_agree_with_the_oracle():
    """K = 64 (the largest table: 32 kB of LDS; warped patches in the scratch slab) on a 64-camera ring: a horizontal
    plane at the ring's centre is inside every camera's image, so the whole table is built."""
    from pais_mvs_amd import synth
    from pais_mvs_amd.config import readme_config
    from pais_mvs_amd.context import Context
    scene = synth.ring_scene(n_cams=64, width=320, height=240, focal=300.0, radius=3.0, n_seeds=0)
    cfg = readme_config()
    S = common.oracle_scene(cfg, scene)
    S.set_kernel_arithmetic(True)
    ctx = Context(cfg, scene.cameras, device=0, seed=42)
    states = [dict(center=[0.0, 0.0, 0.2], normal=[0.0, 0.0, 1.0], ref=0, lod=0, cams=list(range(64))),
              dict(center=[0.1, 0.05, 0.3], normal=[0.0, 0.0, 1.0], ref=5, lod=0, cams=list(range(63, -1, -1))),
              dict(center=[0.0, 0.0, 0.2], normal=[0.0, 0.0, 1.0], ref=0, lod=1, cams=list(range(64)))]
    got = ctx.ncc_batch([_view_state(st) for st in states], tables=True)
    built = 0
    for i, st in enumerate(states):
        want = G.oracle_ncc(S, st)
        _compare(got, i, want, ("ring64", i))
        built += int(want["dropped"] != G.DROP_SAMPLE)
    assert built >= 2
    ctx.close()
    S.close()
