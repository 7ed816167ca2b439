"""The marker-level pair model of the joint search on the device: entries egx_pair_marker_dist and
egx_primitive_select_joint_markers (csrc/genop_joint_markers.hip), `generate_sequence_to_goal(groups=, pair_model="markers")` and the
driver's `--pair-model`, against the float64 / float32 restatement tests/genop_joint_markers_ref.py.

Inputs.  The construction of tests/test_genop_joint_gpu.py lifted from pelvises to clouds: per group a base walk, plus a lattice
offset of pitch 0.4 m per (member, candidate), plus a wiggle of at most 0.02 m per row and frame (`_lattice_tracks` there); every row
is a cloud of 67 points within 0.02 m of the vertical axis through that track, z in [0, 1.7].  The local values are R0^T (world - T0)
in float64; the two sources are split as proj = value + delta, pred = value - delta rf / (1 - rf) with rf 0.5 and |delta| <= 0.05,
each rounded once, so both buffers matter.  The least marker distance of two rows is then within 0.08 m of a lattice distance (0,
0.4, 0.566, ...), and with skin 0.2 and margin 0.6 every float64 frame clearance lies outside (-0.05, +0.05) m: asserted over all
candidate pairs (over the sampled ones at N 256), with hits and near misses both present.

Yardsticks.  The distance entry: `held()` against the exhaustive float64 table (device error within 3 x the float32 restatement's,
pooled over at least MIN_GROUP entries); symmetry and batch independence exact.  The sweep entry is fed the device's own table,
and both restatements read that table too: every member step is checked from the device's `choice_trace` as in
tests/test_genop_joint_gpu.py - pair_hit and the classes exact, pair_term / pair_clearance / joint_cost held, the choice the key order
on the device's own values exactly and the float64 choice where its winner is ahead by more than 6 x the largest |joint_cost32 -
joint_cost64| of the step's rows, the other steps at most UNDECIDABLE_CAP of a case's.  The exhaustive tables of the larger cases
are billions of distances: both restatements compute them with torch on the GPU."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import genop_joint_markers_ref as mref
from tests import test_genop_joint_gpu as jg
from tests.genop_gpu_helpers import (CFG_RF, MIN_GROUP, ROOT, V_SMALL, W_TEST, emit, held, patched_loop,  # noqa: F401
                                     search_world, small_world)

pytestmark = pytest.mark.gpu

SKIN, MARGIN, W_PAIR = 0.2, 0.6, 1.3
BAND = 0.05
SPREAD, DELTA, HEIGHT = 0.02, 0.05, 1.7
GOAL_THRESH = jg.GOAL_THRESH
OUTS = jg.OUTS


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def _clouds(xy, seed):
    """axis tracks [b,N,18,2] float64 (NaN: a row that stays as it is) -> world clouds [b,N,18,67,3] float64"""
    g = np.random.default_rng(seed + 5)
    b, N = xy.shape[:2]
    r, a = SPREAD * np.sqrt(g.uniform(0, 1, (b, N, 18, 67))), g.uniform(0, 2 * np.pi, (b, N, 18, 67))
    z = np.broadcast_to(HEIGHT * np.arange(67) / 66.0, (b, N, 18, 67))
    return np.stack([xy[..., None, 0] + r * np.cos(a), xy[..., None, 1] + r * np.sin(a), z], -1)


def _plant_clouds(c, world, seed, rf=CFG_RF):
    """the two marker sources of the launched rows c["i"] rewritten so that their blend with rf is the world cloud of every row (where
    not NaN): local = R0^T (world - T0) in float64, proj = local + delta, pred = local - delta rf / (1 - rf), each rounded once"""
    i = c["i"]
    n = i["mp"].shape[0]
    w = torch.as_tensor(np.asarray(world)).reshape(n, 18, 67, 3)
    keep = torch.isnan(w).reshape(n, -1).any(1)
    R0, T0 = i["R0"].double().cpu(), i["T0"].double().cpu()
    local = torch.einsum("bji,btaj->btai", R0, w - T0[:, None, None])
    delta = (torch.rand(n, 18, 67, 3, generator=torch.Generator().manual_seed(seed + 9), dtype=torch.float64) * 2 - 1) * DELTA
    proj, pred = (local + delta).float().cuda(), (local - delta * rf / (1 - rf)).float().cuda()
    m = (~keep).cuda()
    i["mp"][:, 2:] = torch.where(m[:, None, None, None], proj, i["mp"][:, 2:])
    yg = i["Y_gen"].view(18, n, 67, 3)
    yg.copy_(torch.where(m[None, :, None, None], pred.permute(1, 0, 2, 3), yg))


def _mcase(world, sizes, N, seed, jpb=127, extra=0, interleave=False, mode="plain"):
    """a case of tests/test_genop_joint_gpu.py (its rows, its groups, the selection launched on them) with the lattice clouds planted"""
    c = jg._case(world, sizes, N, seed, jpb, extra, interleave, mode)
    _plant_clouds(c, _clouds(jg._lattice_tracks(c["groups"], c["b"], N, seed), seed), seed)
    return c


def _world(c, dtype, rf=CFG_RF):
    """[b,N,18,67,3] on the device, in `dtype`: what the restatement makes of the launched buffers"""
    i = c["i"]
    return mref.world_markers(i["R0"], i["T0"], i["mp"], i["Y_gen"], rf, dtype).reshape(c["b"], c["N"], 18, 67, 3)


def _csr(groups):
    sizes = np.asarray([len(g) for g in groups], np.int64)
    dev = lambda a: torch.tensor(np.asarray(a), dtype=torch.int32, device="cuda")
    pair_start = np.concatenate([[0], np.cumsum(sizes * (sizes - 1) // 2)])
    return dev(np.concatenate([[0], np.cumsum(sizes)])), dev([m for g in groups for m in g] or [0]), dev(pair_start), pair_start


def _dist(c, groups=None, rf=CFG_RF):
    """egx_pair_marker_dist on case c -> {D [npairs,N,N,18] (None without pairs), bad [b,N], pair_start}, NaN / -7 where nothing was written"""
    from egogen_amd import _lib
    groups = c["groups"] if groups is None else groups
    b, N, i = c["b"], c["N"], c["i"]
    start, member, pstart, ps = _csr(groups)
    npairs = int(ps[-1])
    D = torch.full((npairs, N, N, 18), float("nan"), device="cuda") if npairs else None
    bad = torch.full((b * N,), -7, dtype=torch.int32, device="cuda")
    keep = [i[k].clone() for k in ("mp", "Y_gen", "R0", "T0")]
    _lib.check(_lib.load().egx_pair_marker_dist(_lib.ptr(i["mp"]), _lib.ptr(i["Y_gen"]), float(rf), _lib.ptr(i["R0"]), _lib.ptr(i["T0"]), b, N, _lib.ptr(start),
                                                _lib.ptr(member), _lib.ptr(pstart), len(groups), npairs, _lib.ptr(D), _lib.ptr(bad),
                                                _lib.current_stream_ptr()), "egx_pair_marker_dist")
    torch.cuda.synchronize()
    for k, v in zip(("mp", "Y_gen", "R0", "T0"), keep):
        assert torch.equal(i[k], v) or bool(torch.isnan(v).any()), k                        # the inputs are only read
    return {"D": D, "bad": bad.reshape(b, N), "pair_start": ps, "groups": groups}


def _group_tables(d, gi):
    """the table of group gi of a `_dist` result as the restatement keys it: {(a, b): [N,N,18]}"""
    P, q = len(d["groups"][gi]), int(d["pair_start"][gi])
    out = {}
    for a in range(P):
        for b in range(a + 1, P):
            out[(a, b)] = d["D"][q]
            q += 1
    return out


def _sweep(c, S, d, groups=None, w=W_PAIR, margin=MARGIN, skin=SKIN):
    """egx_primitive_select_joint_markers on the selection outputs of case c and the table d -> outputs on the CPU"""
    from egogen_amd import _lib
    groups = c["groups"] if groups is None else groups
    b, N, i = c["b"], c["N"], c["i"]
    G = len(groups)
    start, member, pstart, ps = _csr(groups)
    o = jg._sweep_outputs(c, S, G)
    goal = c["alive"][0][0]
    keep = {k: c["sel"][k].clone() for k in ("cost", "terms", "colliding")}
    bad = d["bad"].reshape(-1).contiguous()
    _lib.check(_lib.load().egx_primitive_select_joint_markers(
        _lib.ptr(d["D"]), _lib.ptr(bad), _lib.ptr(pstart), int(ps[-1]), _lib.ptr(i["J"]), c["jpb"], _lib.ptr(i["R0"]), _lib.ptr(i["T0"]), _lib.ptr(goal),
        _lib.ptr(c["sel"]["cost"]), _lib.ptr(c["sel"]["terms"]), _lib.ptr(c["sel"]["colliding"]), b, N, _lib.ptr(start), _lib.ptr(member), G, S, w, margin,
        skin, GOAL_THRESH, *[_lib.ptr(o[k]) for k in OUTS], _lib.current_stream_ptr()), "egx_primitive_select_joint_markers")
    torch.cuda.synchronize()
    for k, v in keep.items():
        assert torch.equal(c["sel"][k], v), k                                                # the selection's rows are only read
    return {k: v.cpu() for k, v in o.items()}


def _census(D64):
    """float64 distances of candidate pairs -> (every frame clearance outside the band, hits, near misses)"""
    c = D64 - SKIN
    return bool(((c <= -BAND) | (c >= BAND)).all()), int((c < 0).sum()), int(((c > 0) & (c < MARGIN)).sum())


# ---- the distance entry ----------------------------------------------------------------------------------------------------------
# sizes, N, extra, interleave
DIST_CASES = {
    "P2 N1": ((2,), 1, 0, False),
    "P3 N5": ((3,), 5, 0, False),
    "P32 N4": ((32,), 4, 0, False),
    "mixed N70": ((1, 2, 5), 70, 2, True),
    "65 pairs": ((2,) * 65, 3, 0, False),
    "P2 N256 sampled": ((2,), 256, 0, False),
}
SAMPLES = 2048


@pytest.mark.parametrize("case", list(DIST_CASES))
def test_pair_marker_dist_kernel(small_world, case):
    sizes, N, extra, interleave = DIST_CASES[case]
    name = f"pair_marker_dist {case}"
    got, t64, t32, hits, near, draw = [], [], [], 0, 0, 0
    while draw == 0 or sum(t.numel() for t in got) < MIN_GROUP or not (hits and near):
        assert draw < 12, (name, hits, near)
        c = _mcase(small_world, sizes, N, 60 + 1000 * draw + N + len(sizes), 127, extra, interleave)
        d, n0 = _dist(c), len(t64)
        assert d["D"].shape == (sum(p * (p - 1) // 2 for p in sizes), N, N, 18) and not bool(torch.isnan(d["D"]).any())
        assert not d["bad"].any()                                                            # every row of the launch, grouped or not
        w64, w32 = _world(c, torch.float64), _world(c, torch.float32)
        if N == 256:                                                                         # the exhaustive truth would be 5 G distances
            g = torch.Generator().manual_seed(draw)
            na, nb = (torch.randint(0, N, (SAMPLES,), generator=g).cuda() for _ in range(2))
            m0, m1 = c["groups"][0]
            got.append(d["D"][0, na, nb])
            t64.append(mref.pair_dist_rows(w64[m0, na], w64[m1, nb]))
            t32.append(mref.pair_dist_rows(w32[m0, na], w32[m1, nb]))
        else:
            for gi, members in enumerate(c["groups"]):
                dev, r64, r32 = _group_tables(d, gi), mref.group_table(w64, members), mref.group_table(w32, members)
                for key in dev:
                    got.append(dev[key]), t64.append(r64[key]), t32.append(r32[key])
        ok, h, nm = _census(torch.cat([t.reshape(-1) for t in t64[n0:]]))
        assert ok, (name, draw)
        hits, near, draw = hits + h, near + nm, draw + 1
    emit(f"| {name} | candidate pairs x frames: hits / near misses | {hits} / {near} | draws {draw} | |")
    flat = lambda ts: torch.cat([t.reshape(-1) for t in ts]).cpu()
    held(name, "pair_dist", flat(got), flat(t64), flat(t32))


def test_table_is_symmetric_and_does_not_depend_on_the_batch(small_world):
    sizes, N = (1, 2, 5), 70
    c = _mcase(small_world, sizes, N, 77, extra=2, interleave=True)
    full = _dist(c)
    for gi, members in enumerate(c["groups"]):
        one = _dist(c, groups=[members])
        assert torch.equal(one["bad"], full["bad"])
        if len(members) > 1:
            a, e = int(full["pair_start"][gi]), int(full["pair_start"][gi + 1])
            assert torch.equal(one["D"], full["D"][a:e]), gi
    rev = _dist(c, groups=c["groups"][::-1])                                                 # the order of the groups in the launch
    G = len(c["groups"])
    for gi in range(G):
        a, e = int(full["pair_start"][gi]), int(full["pair_start"][gi + 1])
        ra = int(rev["pair_start"][G - 1 - gi])
        assert torch.equal(rev["D"][ra:ra + e - a], full["D"][a:e]), gi
    # the two members of a pair exchanged: the same bits, transposed
    pair = next(g for g in c["groups"] if len(g) == 2)
    ab, ba = _dist(c, groups=[pair]), _dist(c, groups=[pair[::-1]])
    assert torch.equal(ab["D"][0], ba["D"][0].permute(1, 0, 2))


def _standing(world, rows_xy, seed, frames=None):
    """P people of one row each standing at rows_xy [P,2] (frames: {frame index: [P,2]} where they stand elsewhere) -> case, clouds"""
    P = len(rows_xy)
    c = jg._case(world, (P,), 1, seed)
    xy = np.broadcast_to(np.asarray(rows_xy, np.float64)[:, None, None, :], (P, 1, 18, 2)).copy()
    for f, at in (frames or {}).items():
        xy[:, 0, f] = np.asarray(at, np.float64)
    return c, _clouds(xy, seed)


# local coordinates below 8 m (an ulp of 4.8e-7), about a dozen roundings from the two sources to a distance
CLOSE = 1e-5


def test_the_last_three_markers_count(small_world):
    """the least distance is attained only by markers 64..66 of both people: held 0.45 m out towards each other from axes 1 m apart"""
    c, cl = _standing(small_world, [[0.0, 0.0], [1.0, 0.0]], 11)
    cl[0, :, :, 64:, 0] = 0.45
    cl[1, :, :, 64:, 0] = 0.55
    cl[:, :, :, 64:, 1] = 0.0
    _plant_clouds(c, cl, 11)
    w64 = _world(c, torch.float64)
    t64 = mref.pair_dist(w64[0], w64[1])[0, 0]
    rest = mref.pair_dist(w64[0, :, :, :64], w64[1])[0, 0].minimum(mref.pair_dist(w64[0], w64[1, :, :, :64])[0, 0])
    assert float((t64 - 0.1).abs().max()) < 1e-3 and float(rest.min()) > 0.4               # one of the 3 x 3 pairs at the same height, nobody else near
    d = _dist(c)
    assert float((d["D"][0, 0, 0].double() - t64).abs().max()) < CLOSE


@pytest.mark.parametrize("frame", [0, 17])
def test_the_first_and_the_last_predicted_frame(small_world, frame):
    """the least distance is attained only at frame 2, and only at frame 19: two people 1 m apart but for that frame (0.3 m).  delta
    differs from frame to frame by up to 0.1 m, so either buffer read a frame off misses by far more than CLOSE"""
    c, cl = _standing(small_world, [[0.0, 0.0], [1.0, 0.0]], 13 + frame, frames={frame: [[0.0, 0.0], [0.3, 0.0]]})
    _plant_clouds(c, cl, 13 + frame)
    w64 = _world(c, torch.float64)
    t64 = mref.pair_dist(w64[0], w64[1])[0, 0]
    got = _dist(c)["D"][0, 0, 0].double()
    assert int(t64.argmin()) == frame and float(t64[frame]) < 0.35 and float(t64[torch.arange(18) != frame].min()) > 0.9
    assert float((got - t64).abs().max()) < CLOSE and int(got.argmin()) == frame


@pytest.mark.parametrize("rf", [0.0, 1.0])
def test_either_source_alone(small_world, rf):
    """rf 0: the prior's markers alone; rf 1: the body model's.  The case is planted for rf 0.5, so the two sources differ by 2 delta"""
    c = _mcase(small_world, (3,), 5, 21)
    d = _dist(c, rf=rf)
    w64, w32 = _world(c, torch.float64, rf), _world(c, torch.float32, rf)
    r64, r32, dev = mref.group_table(w64, c["groups"][0]), mref.group_table(w32, c["groups"][0]), _group_tables(d, 0)
    flat = lambda t: torch.cat([t[k].reshape(-1) for k in sorted(t)]).cpu()
    held(f"pair_marker_dist rf {rf}", "pair_dist", flat(dev), flat(r64), flat(r32))
    half = mref.group_table(_world(c, torch.float64), c["groups"][0])
    assert float((flat(half) - flat(r64)).abs().max()) > 0.01                               # another table than the blend's


def test_a_non_finite_marker(small_world):
    """one row-frame of one member: D = +inf there, its row_bad bit set, everybody else's entries the bits they were; the bad row's
    own step is NaN and ranks as non-finite"""
    c = _mcase(small_world, (3,), 4, 31)
    before = _dist(c)
    m1 = c["groups"][0][1]
    row, t, f = m1 * 4 + 2, 9, 7
    for value, where in ((float("nan"), "mp"), (float("inf"), "Y_gen")):
        saved = {k: c["i"][k].clone() for k in ("mp", "Y_gen")}
        if where == "mp":
            c["i"]["mp"][row, t, 66, 2] = value
        else:
            c["i"]["Y_gen"].view(18, -1, 67, 3)[f, row, 0, 0] = value
        d = _dist(c)
        bad = torch.zeros(c["b"], 4, dtype=torch.int32)
        bad[m1, 2] = 1 << f
        assert torch.equal(d["bad"].cpu(), bad), where
        tabs, ref = _group_tables(d, 0), _group_tables(before, 0)
        hole01 = torch.zeros(4, 4, 18, dtype=torch.bool)
        hole01[:, 2, f] = True                                                               # member 1 is the second of pair (0, 1)
        hole12 = torch.zeros(4, 4, 18, dtype=torch.bool)
        hole12[2, :, f] = True                                                               # and the first of pair (1, 2)
        for key, hole in (((0, 1), hole01), ((1, 2), hole12), ((0, 2), torch.zeros(4, 4, 18, dtype=torch.bool))):
            got, was = tabs[key].cpu(), ref[key].cpu()
            assert bool((got[hole] == float("inf")).all()) and torch.equal(got[~hole], was[~hole]), (where, key)
        o = _sweep(c, 1, d)
        assert bool(torch.isnan(o["pair_term"][0, m1, 2])) and bool(torch.isnan(o["pair_clearance"][0, m1, 2])) and bool(torch.isnan(o["joint_cost"][0, m1, 2]))
        assert int(o["pair_hit"][0, m1, 2]) == 0 and int(o["choice_trace"][0, m1]) != 2      # a finite row is there: the bad one is not chosen
        others = [r for r in range(4) if r != 2]
        assert bool(torch.isfinite(o["pair_term"][0, m1, others]).all()) and bool(torch.isfinite(o["joint_cost"][0][c["groups"][0][0]]).all())
        pool = _new_pool()
        _check_launch(f"non-finite {where}", c, o, 1, d, pool)
        for k, v in saved.items():
            c["i"][k].copy_(v)
    # every frame of every row bad: all rows rank as non-finite, by collision and index only
    members = c["groups"][0]
    o = _sweep(c, 1, dict(before, bad=torch.full_like(before["bad"], (1 << 18) - 1)))
    assert bool(torch.isnan(o["joint_cost"][0][members]).all()) and bool((o["status"][members] & 2).ne(0).all()) and not o["pair_hit"][0][members].any()
    coll = c["sel"]["colliding"].cpu().long()
    assert o["choice_trace"][0][members].tolist() == [mref.first_by_key(2 + coll[m], torch.zeros(4)) for m in members]


# ---- the sweep entry, fed the device's own table -------------------------------------------------------------------------------------
_new_pool, _close_pool = jg._new_pool, jg._close_pool


def _check_launch(name, c, o, S, d, pool, w=W_PAIR, margin=MARGIN, skin=SKIN):
    """`_check_launch` of tests/test_genop_joint_gpu.py with the marker model's restatement on the device's table d"""
    model = {"bad": (d["bad"].cpu()[..., None] >> torch.arange(18)) & 1 != 0, "w": w, "margin": margin, "skin": skin}
    tables = [{k: v.cpu() for k, v in _group_tables(d, gi).items()} for gi in range(len(c["groups"]))]
    jg._check_launch(name, c, o, S, pool, mref, lambda gi: dict(model, D=tables[gi]))


# sizes, N, S, jpb, extra, interleave, mode
SWEEP_CASES = {
    "one": ((1,), 1, 1, 127, 0, False, "plain"),
    "P3 N5": ((3,), 5, 1, 55, 0, False, "plain"),
    "full group": ((32,), 8, 2, 127, 0, False, "plain"),
    "mixed": ((1, 2, 5), 70, 3, 127, 2, True, "plain"),
    "65 pairs": ((2,) * 65, 3, 2, 127, 0, False, "plain"),
    "field": ((3, 2), 5, 2, 127, 0, True, "field"),
    "obstacles": ((3, 2), 5, 2, 127, 0, True, "obstacles"),
}


@pytest.mark.parametrize("case", list(SWEEP_CASES))
def test_select_joint_markers_kernel(small_world, case):
    sizes, N, S, jpb, extra, interleave, mode = SWEEP_CASES[case]
    name = f"select_joint_markers {case}"
    pairs = max(sizes) > 1
    pool, hits, near, draw = _new_pool(), 0, 0, 0
    while draw == 0 or (pairs and (sum(t.shape[1] for t in pool["got"]) < MIN_GROUP or not (hits and near))):
        assert draw < 12, (name, hits, near)
        c = _mcase(small_world, sizes, N, 40 + 1000 * draw + N + len(sizes), jpb, extra, interleave, mode)
        d = _dist(c)
        if pairs:
            ok, h, nm = _census(d["D"].double())                                             # the device's table is what the sweeps read
            assert ok, (name, draw)
            hits, near = hits + h, near + nm
        draw += 1
        o = _sweep(c, S, d)
        _check_launch(name, c, o, S, d, pool)
    emit(f"| {name} | candidate pairs x frames: hits / near misses | {hits} / {near} | draws {draw} | |")
    _close_pool(name, pool, pairs)


def test_sweeps_do_not_depend_on_the_batch(small_world):
    sizes, N, S = (1, 2, 5), 70, 3
    c = _mcase(small_world, sizes, N, 77, extra=2, interleave=True)
    full = _sweep(c, S, _dist(c))
    for gi, members in enumerate(c["groups"]):
        one = _sweep(c, S, _dist(c, groups=[members]), groups=[members])
        for k in jg.PER_SEQ:
            assert torch.equal(one[k][members], full[k][members]), (gi, k)
        for k in jg.TRACES + ("choice_trace",):
            assert torch.equal(one[k][:, members], full[k][:, members]), (gi, k)
        assert torch.equal(one["changed"][:, 0], full["changed"][:, gi])
    rev = _sweep(c, S, _dist(c, groups=c["groups"][::-1]), groups=c["groups"][::-1])
    grouped = sorted(m for g in c["groups"] for m in g)
    for k in jg.PER_SEQ:
        assert torch.equal(rev[k][grouped], full[k][grouped]), k
    for k in jg.TRACES + ("choice_trace",):
        assert torch.equal(rev[k][:, grouped], full[k][:, grouped]), k
    assert torch.equal(rev["changed"], full["changed"].flip(1))


# ---- the two hand cases of tests/test_genop_joint_markers_cpu.py on the device ---------------------------------------------------------
def _hand_case(world, tracks, clouds, goal, seed):
    """tracks [P,N,18,2] planted as pelvises (what the cylinder model reads), clouds [P,N,18,67,3] as markers; goal-only weights"""
    P, N = tracks.shape[:2]
    c = jg._case(world, (P,), N, seed, tracks=tracks, weights=jg.GOAL_ONLY, with_pene=False, goal=goal)
    _plant_clouds(c, clouds, seed)
    return c


def test_an_outstretched_arm_is_a_hit_for_the_markers_only(small_world):
    from tests.test_genop_joint_markers_cpu import _walk, cloud
    rows = [[_walk(0.0, 0.0, 0.03, 0.0), _walk(0.0, -0.6, 0.03, 0.0)], [_walk(0.0, 0.7, 0.03, 0.0), _walk(0.0, 1.3, 0.03, 0.0)]]
    arm = (40, 0.0, 0.66)
    tracks = torch.stack([torch.stack(r) for r in rows]).numpy()
    clouds = torch.stack([torch.stack([cloud(t, arm=arm if p == 0 else None) for t in r]) for p, r in enumerate(rows)]).numpy()
    c = _hand_case(small_world, tracks, clouds, torch.tensor([[1.5, 0.0, 0.9], [1.5, 0.7, 0.9]]), 3)
    sel = {k: v.cpu() for k, v in c["sel"].items()}
    assert sel["choice"].tolist() == [0, 0] and not sel["colliding"].any()
    assert bool((sel["cost"][:, 1] - sel["cost"][:, 0] > 0.12).all())                        # the far row is dearer than the cylinder term of 0.1
    cyl = jg._joint(c, 2, w=1.0, margin=0.5, body=0.15)                                      # cylinders 0.4 m clear: nobody moves
    assert cyl["choice_trace"].tolist() == [[0, 0], [0, 0]] and not cyl["pair_hit"].any() and cyl["changed"].reshape(-1).tolist() == [0, 0]
    assert float((cyl["crowd_clearance"] - 0.4).abs().max()) < CLOSE
    d = _dist(c)
    o = _sweep(c, 2, d, w=1.0, margin=0.5, skin=0.05)
    assert o["choice_trace"].tolist() == [[1, 0], [1, 0]] and o["changed"].reshape(-1).tolist() == [1, 0]
    assert o["choice"].tolist() == [1, 0] and o["status"].tolist() == [0, 0] and o["crowd_hit"].tolist() == [0, 0]
    assert o["pair_hit"][0].tolist() == [[1, 0], [0, 0]] and o["pair_hit"][1].tolist() == [[1, 0], [0, 0]]
    assert float(o["pair_clearance"][0, 0, 0]) < -0.005 and float(o["crowd_clearance"].min()) > 0.5
    assert torch.equal(o["goal_dist"][1], sel["goal_dist"][1]) and abs(float(o["goal_dist"][0]) - float(sel["terms"][0, 1, 0])) < CLOSE
    pool = _new_pool()
    _check_launch("arm", c, o, 2, d, pool, w=1.0, margin=0.5, skin=0.05)
    assert all(pool["ok"])


def test_one_above_the_other_is_a_hit_for_the_cylinders_only(small_world):
    from tests.test_genop_joint_markers_cpu import _walk, cloud
    t = _walk(0.3, -0.2, 0.02, 0.01)
    tracks = torch.stack([t[None], t[None]]).numpy()
    clouds = torch.stack([cloud(t, height=0.5)[None], (cloud(t, height=0.5) + torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64))[None]]).numpy()
    c = _hand_case(small_world, tracks, clouds, torch.tensor([[1.5, 0.0, 0.9], [1.5, 0.7, 0.9]]), 5)
    cyl = jg._joint(c, 1, w=1.0, margin=0.5, body=0.15)
    assert cyl["pair_hit"].reshape(-1).tolist() == [1, 1] and cyl["crowd_hit"].tolist() == [1, 1] and cyl["status"].tolist() == [1, 1]
    d = _dist(c)
    o = _sweep(c, 1, d, w=1.0, margin=0.5, skin=0.05)
    assert o["pair_hit"].reshape(-1).tolist() == [0, 0] and o["crowd_hit"].tolist() == [0, 0] and o["status"].tolist() == [0, 0]
    assert float((d["D"][0, 0, 0] - 0.5).abs().max()) < 0.03 and float(d["D"].min()) >= 0.5 - CLOSE
    assert float((o["crowd_clearance"].double() - (d["D"][0, 0, 0].min().double().cpu() - 0.05)).abs().max()) < 1e-7


# ---- argument checks -----------------------------------------------------------------------------------------------------------------
def test_marker_entries_reject_bad_arguments(small_world):
    """Rejected before anything is launched: every pointer may therefore be the same scratch buffer."""
    from egogen_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(16384, device="cuda")
    p = C.c_void_p(buf.data_ptr())
    ins = ["markers_proj", "Y_gen", "R0", "T0", "group_start", "group_member", "pair_start", "row_bad"]

    def dist(N=1, G=1, rf=0.5, npairs=1, table=True, null=None):
        a = {k: None if k == null else p for k in ins}
        return lib.egx_pair_marker_dist(a["markers_proj"], a["Y_gen"], rf, a["R0"], a["T0"], 2, N, a["group_start"], a["group_member"], a["pair_start"], G,
                                        npairs, p if table else None, a["row_bad"], _lib.current_stream_ptr())
    bad = [{"N": 0}, {"N": 257}, {"G": 0}, {"rf": -0.1}, {"rf": 1.5}, {"rf": float("nan")}, {"npairs": -1}, {"npairs": 1, "table": False},
           {"npairs": 0, "table": True}] + [{"null": k} for k in ins]
    for kw in bad:
        assert dist(**kw) == -1, kw
        with pytest.raises(_lib.EgxError):
            _lib.check(dist(**kw), "egx_pair_marker_dist")
    outs = list(OUTS)
    sins = ["row_bad", "pair_start", "joints", "R0", "T0", "goal", "cost", "cost_terms", "colliding", "group_start", "group_member"]

    def sweep(N=1, G=1, S=1, w=1.0, margin=0.5, skin=0.05, npairs=1, table=True, null=None):
        a = {k: None if k == null else p for k in sins + outs}
        return lib.egx_primitive_select_joint_markers(
            p if table else None, a["row_bad"], a["pair_start"], npairs, a["joints"], 127, a["R0"], a["T0"], a["goal"], a["cost"], a["cost_terms"],
            a["colliding"], 2, N, a["group_start"], a["group_member"], G, S, w, margin, skin, 0.1, *[a[k] for k in outs], _lib.current_stream_ptr())
    bad = [{"N": 0}, {"N": 257}, {"S": 0}, {"S": 9}, {"G": 0}, {"margin": -0.1}, {"margin": float("nan")}, {"skin": -0.1}, {"skin": float("nan")},
           {"w": float("inf")}, {"w": float("nan")}, {"npairs": -1}, {"npairs": 1, "table": False}, {"npairs": 0, "table": True}] + \
          [{"null": k} for k in sins + outs]
    for kw in bad:
        assert sweep(**kw) == -1, kw
        with pytest.raises(_lib.EgxError):
            _lib.check(sweep(**kw), "egx_primitive_select_joint_markers")
    torch.cuda.synchronize()
    assert not buf.any()                                                                      # nothing was launched


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    if not torch.is_tensor(a):
        return a == b
    return a.shape == b.shape and bool(((a == b) | (torch.isnan(a.float()) & torch.isnan(b.float()))).all())


def test_explicit_cylinder_is_the_default(search_world):
    base = jg._e2e(search_world, 4, 3, groups=[0, 0, 1, 1])
    res = jg._e2e(search_world, 4, 3, groups=[0, 0, 1, 1], pair_model="cylinder")
    for k in jg.E2E_SAME + res.JOINT_FIELDS:
        assert torch.equal(getattr(res, k), getattr(base, k)) if k in jg.E2E_SAME else _same(getattr(res, k), getattr(base, k)), k
    assert res.search["pair_model"] == base.search["pair_model"] == "cylinder" and res.search["pair_skin"] == base.search["pair_skin"] == 0.05


def test_markers_with_singleton_groups_are_the_search_without_groups(search_world):
    base = jg._e2e(search_world, 4, 3)
    res = jg._e2e(search_world, 4, 3, groups=[0, 1, 2, 3], pair_model="markers")
    for k in jg.E2E_SAME:
        assert torch.equal(getattr(res, k), getattr(base, k)), k
    assert torch.equal(res.individual_choice, res.choice) and not res.joint_changed.any() and not res.pair_term.any() and not res.crowd_hit.any()
    assert bool((res.crowd_clearance == float("inf")).all()) and res.search["pair_model"] == "markers"


def test_generate_sequence_to_goal_with_the_marker_model(search_world, tmp_path):
    from egogen_amd.metrics import MotionSet, crowd_metrics
    w = search_world
    op, K, b, N, S, skin = w["op"], 3, 4, 4, 2, 0.05
    members = [[0, 1], [2, 3]]
    for Kp in range(K - 1, K + 1):               # a run of K - 1 primitives is the prefix of the longer one
        with patched_loop(op, "_search_loop", no_host_wait=True) as seen:
            res = jg._e2e(w, N, Kp, groups=[0, 0, 1, 1], pair_model="markers", pair_skin=skin)
        assert seen.calls == [(Kp, b, N)]
        if Kp == K:
            for k in ("choice", "individual_choice", "choice_trace", "joint_cost", "crowd_clearance", "cost", "pair_clearance"):
                assert _same(getattr(res, k)[:K - 1], getattr(prev, k)), k
        prev = res
        assert res.pair_term.shape == (Kp, S, b, N) and res.choice_trace.shape == (Kp, S, b) and res.joint_changed.shape == (Kp, S, 2)
        assert torch.equal(res.choice, res.choice_trace[:, -1])
        ch = res.choice[Kp - 1].long()
        pp = seen.s["pp"].reshape(b, N, 20, 93)
        assert torch.equal(res.params[Kp - 1], pp[torch.arange(b), ch])                      # the hand-off continued from the joint choice
        assert seen.s["pair_dist"].shape == (2, N, N, 18) and seen.s["row_bad"].shape == (b * N,)
    assert float(res.pair_term.max()) > 0.0                                                  # partners 0.8 m apart: they feel each other
    assert res.search["pair_model"] == "markers" and res.search["pair_skin"] == skin
    assert int(res.n_valid.min()) == K                                                       # every member recorded every primitive
    # the search against the instrument: crowd_clearance + pair_skin is the evaluator's least marker distance over the pairs that hold
    # the member and the motion frames 18k + 2 .. 18k + 19, up to the float32 roundings of the search (the evaluator is float64 from
    # the same float32 records): 16 ulps of the largest world coordinate involved
    cm = crowd_metrics(MotionSet.from_sequences(res))
    md, pi, pj = torch.as_tensor(cm["marker_dist"]), cm["pair"]["i"], cm["pair"]["j"]
    world = torch.einsum("kbij,kbtaj->kbtai", res.rotmat.double().cpu(), res.markers.double().cpu()) + res.transl.double().cpu()[:, :, None, None]
    for k in range(K):
        for g in members:
            big = float(world[k, g, 2:].abs().max())
            bound = 16.0 * 2.0 ** (np.floor(np.log2(big)) - 23)
            for m in g:
                mine = [q for q in range(len(pi)) if m in (int(pi[q]), int(pj[q]))]
                least = float(md[mine, 18 * k + 2:18 * k + 20].min())
                got = float(res.crowd_clearance[k, m].double()) + skin
                print(f"| e2e markers | k {k} member {m} | evaluator {least:.9f} | search {got:.9f} | bound {bound:.3e} |")
                assert abs(got - least) <= bound, (k, m, got, least, bound)
                if abs(least - skin) > bound:
                    assert int(res.crowd_hit[k, m]) == int(least < skin)
    # save and reload: the files of a marker-model result are obstacles for the next person, and the result keeps its model
    res_np = jg._e2e(w, N, K, groups=[0, 0, 1, 1], pair_model="markers", pair_skin=skin, to_numpy=True)
    before = {k: np.array(getattr(res_np, k)) for k in res_np.JOINT_FIELDS}
    paths = [res_np.save(str(tmp_path), i, man_id=f"p_{i}") for i in range(4)]
    from egogen_amd import MovingObstacles
    assert np.array_equal(MovingObstacles.from_rollout_files(paths).xy, MovingObstacles.from_sequences(res_np).xy)
    for k in res_np.JOINT_FIELDS:
        assert np.array_equal(getattr(res_np, k), before[k], equal_nan=True) and res_np.search[k] is getattr(res_np, k), k
    assert res_np.search["pair_model"] == "markers" and res_np.search["pair_skin"] == skin
    assert np.array_equal(res_np.choice_trace, res.choice_trace.cpu().numpy())


def test_gen_motion_driver_pair_model(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = tmp_path / "crowd"
    base = [sys.executable, os.path.join(ROOT, "exp_GAMMAPrimitive", "gen_motion.py"), "--n-primitives", "2", "--seed", "3", "--num-verts", str(V_SMALL),
            "--n-gens", "2", "--n-candidates", "4", "--out", str(out)]
    cmd = base + ["--people", "0,0,0:0.3,3,0.9;0.8,0,0:0.5,3,0.9;0.4,3,180:0.4,0,0.9", "--pair-model", "markers", "--pair-skin", "0.06"]
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    files = sorted(f for f in os.listdir(out) if f.startswith("motion_") and f.endswith(".pkl"))
    assert files == sorted(f"motion_3_{v}_p{p}.pkl" for v in range(2) for p in range(3)), files
    lines = re.findall(r"variant (\d+): minimum crowd clearance (-?[0-9.]+) m, crowd hits (\d+), members still changing in a last sweep (\d+)", r.stdout)
    assert [int(v[0]) for v in lines] == [0, 1] and all(np.isfinite(float(v[1])) for v in lines), r.stdout[-1500:]
    bad = subprocess.run(base + ["--pair-model", "markers"], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert bad.returncode == 2 and "--pair-model markers needs --people" in bad.stderr
