"""Moving obstacles of the primitive search on the device: the obstacle phase of the selection kernels (entries
egx_primitive_select_obstacles / egx_primitive_beam_select_obstacles, csrc/genop.hip), `generate_sequence_to_goal(obstacles=)` and
the driver's `--avoid` / `--start`, against the float64 / float32 restatement tests/genop_obstacles_ref.py.

Values (`obs_term`, `obs_clearance`, `cost`, the beam's `acc`) are held like every term of the search: the device's error against
float64 within R = 3 times the float32 restatement's, over at least MIN_GROUP pooled rows.  The hit is compared EXACTLY: the
obstacle tracks are built from the rows' own float64 world pelvis tracks plus offsets, the rows stand on a lattice 3 m apart, so
every row's float64 clearance is either <= -0.05 m or >= +0.05 m by construction (asserted, with both kinds present), four orders
of magnitude above float32 round-off at these coordinates.  Choices are compared on the groups `decidable()` passes, whose share is
capped by UNDECIDABLE_CAP as in tests/test_genop_search_gpu.py."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import genop_beam_ref as bref
from tests import genop_obstacles_ref as oref
from tests import genop_search_ref as sref
from tests.genop_gpu_helpers import (CFG_RF, MIN_GROUP, POOL, ROOT, UNDECIDABLE_CAP, V_SMALL, W_TEST, _beam_select, _feet, _handmade, _inputs,  # noqa: F401
                                     _rows_inputs, _select, _selection_args, emit, held, patched_loop, search_world, small_world)
from tests.test_genop_beam_gpu import beam_decidable
from tests.test_genop_search_gpu import decidable

pytestmark = pytest.mark.gpu

GOAL_ONLY = {"goal": 1.0, "skate": 0.0, "floor": 0.0, "pene": 0.0, "face": 0.0}
HIT_MARGIN = 0.05           # metres: no row of a constructed case has a float64 clearance inside (-HIT_MARGIN, +HIT_MARGIN)
RADIUS, BODY, MARGIN, W_OBS = 0.2, 0.1, 0.6, 1.7      # the constructed cases; summed radii 0.3 m
NULL_FIELD = (None, None, 0.0, 0, 0, 0, None)


def _obs(xy, radius, count=None, index=None, frame0=0, w=W_OBS, margin=MARGIN, body=BODY):
    """an obstacle descriptor of the tests: xy [S,O_max,T,2], radius [S,O_max] (or one number), count [S] (all live unless given)"""
    xy = torch.as_tensor(np.asarray(xy), dtype=torch.float32)
    S, O = xy.shape[:2]
    radius = torch.as_tensor(np.broadcast_to(np.asarray(radius, np.float32), (S, O)).copy())
    count = torch.full((S,), O, dtype=torch.int32) if count is None else torch.as_tensor(count, dtype=torch.int32)
    index = None if index is None else torch.as_tensor(index, dtype=torch.int32)
    return {"xy": xy, "radius": radius, "count": count, "index": index, "frame0": int(frame0), "w": float(w), "margin": float(margin),
            "body": float(body)}


def _select_obs(x, jpb, ob, fld=None, findex=None, weights=W_TEST, b=None, N=None, rf=CFG_RF, beam=None, acc=None, ncoll=None, group0=0,
                nan_face_rows=(), nan_pelvis=()):
    """egx_primitive_select_obstacles (beam = (W, N): egx_primitive_beam_select_obstacles) on the groups [group0, group0 + b) of the
    row set x with the obstacles `ob` and the fields `fld` (None: a null field) -> (outputs on the CPU, inputs as launched);
    nan_pelvis: (row, frame) pairs whose pelvis y becomes NaN"""
    from egogen_amd import _lib
    b = x["b"] if b is None else b
    M = x["N"] if N is None else N
    lead, i, o, _alive = _selection_args(x, b, M, group0, jpb, rf, weights, 40.0, 0.1, nan_face_rows)
    for r, t in nan_pelvis:
        i["J"][r, t, 0, 1] = float("nan")        # a view of the launched joints
    fi = lambda *s: torch.full(s, -7, dtype=torch.int32, device="cuda")
    ff = lambda *s: torch.full(s, float("nan"), device="cuda")
    if fld is None:
        fa, fidx = NULL_FIELD, None
    else:
        fidx = None if findex is None else torch.as_tensor(findex, dtype=torch.int32, device="cuda")
        fa = (_lib.ptr(fld.dist), _lib.ptr(fld.origin), float(np.float32(fld.cell)), fld.dist.shape[1], fld.dist.shape[2], len(fld), _lib.ptr(fidx))
    d = {k: ob[k].cuda().contiguous() for k in ("xy", "radius", "count")}
    oidx = None if ob["index"] is None else ob["index"][group0:group0 + b].cuda().contiguous()
    o.update({"obs_term": ff(b, M), "obs_clearance": ff(b, M), "obs_hit": fi(b, M)})
    oa = (_lib.ptr(d["xy"]), _lib.ptr(d["radius"]), _lib.ptr(d["count"]), _lib.ptr(oidx), ob["xy"].shape[0], ob["xy"].shape[1], ob["xy"].shape[2],
          ob["frame0"], ob["w"], ob["margin"], ob["body"], _lib.ptr(o["obs_term"]), _lib.ptr(o["obs_clearance"]), _lib.ptr(o["obs_hit"]))
    if beam is None:
        o = {"choice": fi(b), "status": fi(b), "reached": fi(b), "goal_dist": ff(b), **o}
        _lib.check(_lib.load().egx_primitive_select_obstacles(
            *lead, b, M, _lib.ptr(o["choice"]), _lib.ptr(o["status"]), _lib.ptr(o["reached"]), _lib.ptr(o["goal_dist"]), _lib.ptr(o["cost"]),
            _lib.ptr(o["terms"]), _lib.ptr(o["colliding"]), *fa, *oa, _lib.current_stream_ptr()), "egx_primitive_select_obstacles")
    else:
        W, N = beam
        acc = torch.zeros(b, W, device="cuda") if acc is None else acc.float().cuda().contiguous()
        ncoll = torch.zeros(b, W, dtype=torch.int32, device="cuda") if ncoll is None else ncoll.int().cuda().contiguous()
        o.update({"beam_row": fi(b, W), "parent": fi(b, W), "acc": ff(b, W), "ncoll": fi(b, W), "path_cost": ff(b, W), "status": fi(b, W),
                  "goal_dist": ff(b, W), "reached": fi(b, W)})
        _lib.check(_lib.load().egx_primitive_beam_select_obstacles(
            *lead, b, W, N, _lib.ptr(acc), _lib.ptr(ncoll), _lib.ptr(o["cost"]), _lib.ptr(o["terms"]), _lib.ptr(o["colliding"]),
            _lib.ptr(o["beam_row"]), _lib.ptr(o["parent"]), _lib.ptr(o["acc"]), _lib.ptr(o["ncoll"]), _lib.ptr(o["path_cost"]),
            _lib.ptr(o["status"]), _lib.ptr(o["goal_dist"]), _lib.ptr(o["reached"]), *fa, *oa, _lib.current_stream_ptr()),
            "egx_primitive_beam_select_obstacles")
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in o.items()}, i


def _set_of_row(ob, b, M, group0=0):
    idx = torch.zeros(b, dtype=torch.long) if ob["index"] is None else ob["index"][group0:group0 + b].long()
    return idx.repeat_interleave(M)


def _restate_obs(i, ob, b, M, dtype, weights=W_TEST, group0=0, geo=None):
    """the rows of a launch in `dtype`: genop_obstacles_ref.apply on genop_search_ref.score and genop_obstacles_ref.row_terms"""
    r = sref.score(i["Y_gen"], i["X"], i["J"], i["mp"], i["R0"], i["T0"], i["pene"], i["goal_rows"], _feet(), weights, 40.0, CFG_RF, dtype)
    t = oref.row_terms(i["R0"], i["T0"], i["J"], ob["xy"].numpy(), ob["radius"].numpy(), ob["count"].numpy(), _set_of_row(ob, b, M, group0).numpy(),
                       ob["frame0"], ob["margin"], ob["body"], dtype)
    return oref.apply(r, t, ob["w"], dtype, weights, geo)


# ---- constructed cases: every hit decidable --------------------------------------------------------------------------------
def _lattice(x, b, M):
    """the rows of x moved onto a lattice 3 m apart (groups 30 m apart in y): a row's pelvis stays within 0.6 m of its node, so an
    obstacle built round one row is at least 1.5 m from every other"""
    n = torch.arange(b * M) % M
    g = torch.arange(b * M) // M
    x["T0"] = torch.stack([3.0 * (n % 9).float(), 3.0 * (n // 9).float() + 30.0 * g.float(), x["T0"][:, 2]], -1)
    return x


def _pelvis64(x, jpb, b, M):
    """float64 world xy [b*M,20,2] of the pelvis of the rows of x as a launch reads them"""
    _, i, _, _ = _selection_args(x, b, M, 0, jpb, CFG_RF, W_TEST, 40.0, 0.1, ())
    return oref.world_pelvis(i["R0"], i["T0"], i["J"], torch.float64)


def _tracks(p64, b, M, O, T, frame0, per_group, seed, index=None):
    """Obstacle sets round the rows' own pelvis tracks p64 [b*M,20,2].  An obstacle built round a row follows it: at absolute frame
    a it stands at the row's pelvis of frame clamp(a - frame0, 2, 19) plus a fixed offset of 0.1 m (a hit: clearance about -0.2) or
    0.75 m (a near miss inside the margin: about +0.45; with T = 1 the obstacle stands still at the row's frame 10 plus the offset
    while the row walks some 0.25 m either way, which leaves about 0.2), alternating; what is left of the O tracks stands hundreds of metres away.
    per_group: S = b sets, set index[g] round the rows of group g; else one set round rows of all groups in turn.
    -> xy [S,O,T,2] float64"""
    g = np.random.default_rng(seed)
    S = b if per_group else 1
    xy = np.zeros((S, O, T, 2))
    xy[..., 0], xy[..., 1] = -500.0 - 7.0 * np.arange(O)[None, :, None], 400.0
    tt = np.clip(np.arange(T) - frame0, 2, 19) if T > 1 else np.array([10])      # T = 1: it stands where the row is in mid-track
    for s in range(S):
        if per_group:
            grp = s if index is None else int(np.where(np.asarray(index) == s)[0][0])
            targets = [grp * M + n for n in range(min(O, M))]
        else:
            targets = [(k % b) * M + k // b for k in range(min(O, b * M))]
        for o, row in enumerate(targets):
            ang = g.uniform(0, 2 * np.pi)
            off = (0.1 if (o + seed) % 2 == 0 else 0.75) * np.array([np.cos(ang), np.sin(ang)])
            xy[s, o] = p64[row].numpy()[tt] + off
    return xy


KERNEL_CASES = [(1, 1, 1, 1, False), (3, 5, 2, 19, True), (65, 5, 32, 200, True), (3, 70, 32, 200, False), (1, 70, 2, 19, True)]   # b, N, O, T, S = b


@pytest.mark.parametrize("b,N,O,T,per_group", KERNEL_CASES)
def test_select_obstacles_kernel(small_world, b, N, O, T, per_group):
    name = f"select_obstacles b={b} N={N} O={O} T={T} S={'b' if per_group else 1}"
    jpb = 127 if N != 5 else 55
    frame0 = {1: 0, 19: 0, 200: 37}[T]
    got, r64, r32, oks, clear = [], [], [], [], []
    for draw in range(max(1, -(-MIN_GROUP // (b * N)))):
        x = _lattice(_rows_inputs(small_world, b, N, 400 + b * 7 + N + 1000 * draw, True), b, N)
        index = torch.randperm(b, generator=torch.Generator().manual_seed(draw + b)).tolist() if per_group else None
        xy = _tracks(_pelvis64(x, jpb, b, N), b, N, O, T, frame0, per_group, draw, index)
        ob = _obs(xy, RADIUS, index=index, frame0=frame0)
        o, i = _select_obs(x, jpb, ob)
        plain, _ = _select(x, jpb)
        a64, a32 = _restate_obs(i, ob, b, N, torch.float64), _restate_obs(i, ob, b, N, torch.float32)
        c = a64["clearance"]
        assert bool(((c <= -HIT_MARGIN) | (c >= HIT_MARGIN)).all()), (name, draw, c[(c > -HIT_MARGIN) & (c < HIT_MARGIN)])
        clear.append(c)
        # exact: the hit, the collision, what the obstacles do not touch, what follows from the kernel's own choice
        assert torch.equal(o["obs_hit"].reshape(-1).bool(), a64["hit"]) and torch.equal(a32["hit"], a64["hit"])
        assert torch.equal(o["colliding"].reshape(-1).bool(), plain["colliding"].reshape(-1).bool() | a64["hit"])
        assert torch.equal(o["colliding"].reshape(-1).bool(), a64["colliding"])
        assert torch.equal(o["terms"], plain["terms"])
        ch = o["choice"].long()
        assert int(ch.min()) >= 0 and int(ch.max()) < N
        pick = lambda t: t.gather(1, ch[:, None])[:, 0]
        assert torch.equal(o["status"], pick(o["colliding"]))
        assert torch.equal(o["goal_dist"], pick(o["terms"][..., 0])) and torch.equal(o["reached"].bool(), o["goal_dist"] < 0.1)
        own6 = torch.cat([o["terms"], o["obs_term"][..., None]], -1)
        own, own_status = sref.select(o["cost"], own6, o["colliding"].bool())
        assert torch.equal(own, ch) and torch.equal(own_status.int(), o["status"])
        # the choice, where float64 decides it
        t64, t32 = oref._terms6(a64, b, N), oref._terms6(a32, b, N)
        coll = a64["colliding"].reshape(b, N)
        choice64, ok = decidable(a64["cost"].reshape(b, N), t64, coll, a32["cost"].reshape(b, N))
        choice32, _ = sref.select(a32["cost"].reshape(b, N), t32, coll)
        assert torch.equal(choice32[ok], choice64[ok]) and torch.equal(ch[ok], choice64[ok]), (name, draw, ch, choice64)
        oks.append(ok)
        got.append((o["obs_term"].reshape(-1), o["obs_clearance"].reshape(-1), o["cost"].reshape(-1)))
        r64.append((a64["term"], a64["clearance"], a64["cost"]))
        r32.append((a32["term"], a32["clearance"], a32["cost"]))
    c = torch.cat(clear)
    emit(f"| {name} | hits / near misses / clear | {int((c < 0).sum())} / {int(((c > 0) & (c < MARGIN)).sum())} / {int((c >= MARGIN).sum())} | | |")
    assert bool((c <= -HIT_MARGIN).any()) and bool((c >= HIT_MARGIN).any())
    cat = lambda lst, j: torch.cat([v[j] for v in lst], 0)
    assert float(cat(r64, 0).max()) > 0.1                                         # the term is exercised, not only the veto
    for j, what in enumerate(("obs_term", "obs_clearance", "cost")):
        held(name, what, cat(got, j), cat(r64, j), cat(r32, j))
    ok = torch.cat(oks)
    share = 1.0 - float(ok.float().mean())
    emit(f"| {name} | undecidable groups | {int((~ok).sum())} of {ok.numel()} | {share:.3f} | |")
    assert share <= UNDECIDABLE_CAP, (name, share)


# ---- time indexing -----------------------------------------------------------------------------------------------------------
def _one_frame_obstacle(p, T, at, far=10.0):
    """a track [1,1,T,2] that stands at p at absolute frame `at` and `far` metres beside it at every other frame"""
    xy = np.tile(np.asarray(p, np.float64) + np.array([far, 0.0]), (1, 1, T, 1))
    xy[0, 0, at] = p
    return xy


@pytest.mark.parametrize("frame0", [0, 18])
def test_obstacle_time_indexing(small_world, frame0):
    """An obstacle that stands at row r's frame-10 pelvis at exactly one absolute frame, summed radii 5 mm: a hit with the matching
    frame0, none with frame0 shifted by 3 frames either way (the float64 clearance there is at least 1 cm: the walkers move 2 cm a
    frame)."""
    b, N, r, T = 1, 3, 1, 60
    x = _lattice(_rows_inputs(small_world, b, N, 61, False), b, N)
    p64 = _pelvis64(x, 127, b, N)
    kw = dict(radius=0.002, body=0.003)
    ob = _obs(_one_frame_obstacle(p64[r, 10].numpy(), T, frame0 + 10), frame0=frame0, **kw)
    o, i = _select_obs(x, 127, ob)
    a64 = _restate_obs(i, ob, b, N, torch.float64)
    assert o["obs_hit"][0].tolist() == [0, 1, 0] and a64["hit"].tolist() == [False, True, False]
    assert abs(float(o["obs_clearance"][0, r]) + 0.005) < 1e-4 and int(o["colliding"][0, r]) == 1 and int(o["choice"][0]) != r
    for shift in (-3, 3):
        ob_s = dict(ob, frame0=frame0 + shift)
        o_s, i_s = _select_obs(x, 127, ob_s)
        c64 = _restate_obs(i_s, ob_s, b, N, torch.float64)["clearance"]
        assert float(c64.min()) >= 0.01, c64
        assert not o_s["obs_hit"].any() and not o_s["colliding"].any()
        held(f"time indexing frame0={frame0}", f"clearance shift {shift}", o_s["obs_clearance"].reshape(-1), c64,
             _restate_obs(i_s, ob_s, b, N, torch.float32)["clearance"])


def test_obstacle_frames_clamp(small_world):
    b, N, r, T = 1, 3, 1, 30
    x = _lattice(_rows_inputs(small_world, b, N, 62, False), b, N)
    p64 = _pelvis64(x, 127, b, N)
    kw = dict(radius=0.002, body=0.003)
    # off the end: with frame0 = T - 3 every scored frame reads the last one
    last = _one_frame_obstacle(p64[r, 10].numpy(), T, T - 1)
    for f0 in (T - 3, T + 50, 2 ** 31 - 4):
        o, _ = _select_obs(x, 127, _obs(last, frame0=f0, **kw))
        assert o["obs_hit"][0].tolist() == [0, 1, 0], f0
    ob = _obs(last, frame0=T - 3 - 10, **kw)                                      # frame 10 reads T - 3; frame 12 is the first to read the last
    o, i = _select_obs(x, 127, ob)
    assert float(_restate_obs(i, ob, b, N, torch.float64)["clearance"].min()) >= 0.01
    assert not o["obs_hit"].any()
    # before the start: with frame0 = -5 the frames 2..5 read frame 0
    first = _one_frame_obstacle(p64[r, 3].numpy(), T, 0)
    for f0 in (-5, -2 ** 31):
        o, _ = _select_obs(x, 127, _obs(first, frame0=f0, **kw))
        assert o["obs_hit"][0].tolist() == [0, 1, 0], f0
    o, _ = _select_obs(x, 127, _obs(first, frame0=2, **kw))                       # unclamped: frame 0 is never read
    assert not o["obs_hit"].any()
    # T = 1: every frame sees the same position
    single = np.asarray(p64[r, 15].numpy()).reshape(1, 1, 1, 2)
    outs = [_select_obs(x, 127, _obs(single, frame0=f0, **kw))[0] for f0 in (0, 100, -100)]
    for o in outs:
        assert o["obs_hit"][0].tolist() == [0, 1, 0]
        for k in o:
            assert torch.equal(o[k], outs[0][k]), k


# ---- the empty set ---------------------------------------------------------------------------------------------------------
def test_empty_set_is_the_entry_without_obstacles(small_world):
    from tests.test_geodesic_gpu import _room_rows, _select_field
    b, W, N = 3, 2, 3
    x, fld = _room_rows(small_world, b, W * N, 500)
    empties = [_obs(np.zeros((1, 4, 7, 2)), 0.3, count=[0]), _obs(np.zeros((2, 1, 1, 2)), 0.3, count=[0, 0], index=[1, 0, 1])]
    acc, ncoll = torch.rand(b, W, generator=torch.Generator().manual_seed(3)) + 0.1, torch.tensor([[0, 1], [2, 0], [1, 1]], dtype=torch.int32)
    for ob in empties:
        cases = [(_select_obs(x, 127, ob)[0], _select(x, 127)[0]),
                 (_select_obs(x, 127, ob, fld=fld, findex=list(range(b)))[0], _select_field(x, 127, fld, list(range(b)))[0]),
                 (_select_obs(x, 127, ob, beam=(W, N), acc=acc, ncoll=ncoll)[0], _beam_select(x, W, N, 127, acc, ncoll)[0]),
                 (_select_obs(x, 127, ob, fld=fld, findex=list(range(b)), beam=(W, N), acc=acc, ncoll=ncoll)[0],
                  _select_field(x, 127, fld, list(range(b)), beam=(W, N), acc=acc, ncoll=ncoll)[0])]
        for got, want in cases:
            for k in want:
                assert torch.equal(got[k], want[k]), k
            assert not got["obs_term"].any() and not got["obs_hit"].any() and bool((got["obs_clearance"] == float("inf")).all())
    # no obstacle arrays at all: max_obstacles = 0
    from egogen_amd import _lib
    lead, i, o, _alive = _selection_args(x, b, W * N, 0, 127, CFG_RF, W_TEST, 40.0, 0.1, ())
    out = {k: torch.full((b,), -7, dtype=torch.int32, device="cuda") for k in ("choice", "status", "reached")}
    gd, term, clear = (torch.full(s, float("nan"), device="cuda") for s in ((b,), (b, W * N), (b, W * N)))
    hit = torch.full((b, W * N), -7, dtype=torch.int32, device="cuda")
    _lib.check(_lib.load().egx_primitive_select_obstacles(
        *lead, b, W * N, _lib.ptr(out["choice"]), _lib.ptr(out["status"]), _lib.ptr(out["reached"]), _lib.ptr(gd), _lib.ptr(o["cost"]),
        _lib.ptr(o["terms"]), _lib.ptr(o["colliding"]), *NULL_FIELD, None, None, None, None, 1, 0, 1, 0, 1.0, 0.5, 0.3, _lib.ptr(term),
        _lib.ptr(clear), _lib.ptr(hit), _lib.current_stream_ptr()), "egx_primitive_select_obstacles")
    torch.cuda.synchronize()
    want = _select(x, 127)[0]
    assert torch.equal(o["cost"].cpu(), want["cost"]) and torch.equal(out["choice"].cpu(), want["choice"])
    assert not term.any() and not hit.any() and bool((clear == float("inf")).all())


# ---- veto and ranking ----------------------------------------------------------------------------------------------------------
def _block(x, rows, T=5):
    """one set with an obstacle on the whole pelvis track of each of `rows` (summed radii 0.3 m: clearance -0.3)"""
    p64 = _pelvis64(x, 127, 1, x["N"])
    xy = np.zeros((1, max(1, len(rows)), 20, 2))
    for o, r in enumerate(rows):
        xy[0, o] = p64[r].numpy()
    return _obs(xy, RADIUS, count=[len(rows)], frame0=0, w=0.0)


def test_veto_moves_the_choice(small_world):
    costs = [3.0, 1.0, 2.0, 4.0]
    x = _handmade(small_world, costs, [0, 0, 0, 0])
    for n, c in enumerate(costs):                    # the rows of _handmade stand on one line, 1 m apart: an obstacle blocks one row only
        assert abs(float(x["T0"][n, 0] - x["T0"][1, 0]) + (c - 1.0)) < 1e-5
    free, _ = _select(x, 127, weights=GOAL_ONLY)
    assert int(free["choice"][0]) == 1
    o, _ = _select_obs(x, 127, _block(x, [1]), weights=GOAL_ONLY)                 # the cheapest blocked: the next cheapest, status 0
    assert o["obs_hit"][0].tolist() == [0, 1, 0, 0] and o["colliding"][0].tolist() == [0, 1, 0, 0]
    assert int(o["choice"][0]) == 2 and int(o["status"][0]) == 0 and torch.equal(o["cost"], free["cost"])
    o, _ = _select_obs(x, 127, _block(x, [0, 1, 2, 3]), weights=GOAL_ONLY)        # all blocked: the cheapest, status bit 0
    assert o["obs_hit"][0].tolist() == [1, 1, 1, 1] and int(o["choice"][0]) == 1 and int(o["status"][0]) == 1
    # a NaN pelvis in a scored frame: the row is non-finite and not a hit, though it stands on an obstacle in every other frame
    o, _ = _select_obs(x, 127, _block(x, [1]), weights=GOAL_ONLY, nan_pelvis=[(1, 7)])
    assert bool(torch.isnan(o["obs_term"][0, 1])) and bool(torch.isnan(o["obs_clearance"][0, 1])) and int(o["obs_hit"][0, 1]) == 0
    assert int(o["colliding"][0, 1]) == 0 and bool(torch.isnan(o["cost"][0, 1])) and int(o["choice"][0]) == 2 and int(o["status"][0]) == 0
    assert torch.isfinite(o["obs_term"][0, [0, 2, 3]]).all()
    # the seed frames are not scored
    o, _ = _select_obs(x, 127, _block(x, []), weights=GOAL_ONLY, nan_pelvis=[(1, 0), (1, 1)])
    assert torch.isfinite(o["obs_term"]).all() and not o["obs_hit"].any()
    # the weight: the term of a near miss moves the choice without a veto
    p64 = _pelvis64(x, 127, 1, 4)
    near = _obs((p64[1].numpy() + np.array([0.0, 0.5]))[None, None], RADIUS, frame0=0, w=10.0, margin=0.5)          # clearance 0.2: term 0.3, cost + 3
    o, _ = _select_obs(x, 127, near, weights=GOAL_ONLY)
    assert not o["obs_hit"].any() and abs(float(o["obs_term"][0, 1]) - 0.3) < 1e-4 and int(o["choice"][0]) == 2
    assert abs(float(o["cost"][0, 1]) - (1.0 + 3.0)) < 1e-3 and int(o["status"][0]) == 0


# ---- the beam ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,N,b", [(2, 3, 3), (32, 8, 1)])
def test_beam_select_obstacles_kernel(small_world, W, N, b):
    M = W * N
    name = f"beam_select_obstacles W={W} N={N}"
    g = torch.Generator().manual_seed(9 + W)
    got, r64, r32, oks = [], [], [], []
    for draw in range(max(1, -(-MIN_GROUP // (b * M)))):
        x = _lattice(_rows_inputs(small_world, b, M, 600 + M + 1000 * draw, True), b, M)
        O = min(32, M)
        xy = _tracks(_pelvis64(x, 127, b, M), b, M, O, 40, 3, True, draw)
        ob = _obs(xy, RADIUS, index=list(range(b)), frame0=3)
        acc = torch.rand(b, W, generator=g) * 6.0
        ncoll = torch.randint(0, 3, (b, W), generator=g, dtype=torch.int32)
        o, i = _select_obs(x, 127, ob, beam=(W, N), acc=acc, ncoll=ncoll)
        greedy, _ = _select_obs(x, 127, ob)                                       # the same rows through the greedy entry: the same rows' values
        for k in ("cost", "terms", "colliding", "obs_term", "obs_clearance", "obs_hit"):
            assert torch.equal(o[k], greedy[k]), k
        a64, a32 = _restate_obs(i, ob, b, M, torch.float64), _restate_obs(i, ob, b, M, torch.float32)
        c = a64["clearance"]
        assert bool(((c <= -HIT_MARGIN) | (c >= HIT_MARGIN)).all()) and bool((c < 0).any()) and bool((c > 0).any())
        assert torch.equal(o["obs_hit"].reshape(-1).bool(), a64["hit"]) and torch.equal(o["colliding"].reshape(-1).bool(), a64["colliding"])
        # the kernel's slots are the rule on the kernel's own values: exact
        own = {"cost": o["cost"].reshape(-1), "terms": o["terms"].reshape(-1, 5), "term": o["obs_term"].reshape(-1),
               "colliding": o["colliding"].reshape(-1).bool(), "q": bref.q_of(o["terms"], W_TEST).reshape(-1) + torch.tensor(ob["w"], dtype=torch.float32) * o["obs_term"].reshape(-1)}
        s_own = oref.beam_select(own, b, W, N, acc, ncoll)
        for k in ("beam_row", "parent", "ncoll", "status"):
            assert torch.equal(s_own[k], o[k].long()), (k, s_own[k], o[k])
        assert torch.equal(s_own["path_cost"], o["path_cost"])
        br = o["beam_row"].long()
        assert torch.equal(o["ncoll"].long(), ncoll.long().gather(1, br // N) + o["colliding"].long().gather(1, br))      # hits counted exactly
        assert torch.equal(o["goal_dist"], o["terms"][..., 0].gather(1, br)) and torch.equal(o["reached"].bool(), o["goal_dist"] < 0.1)
        # ranks equal to the restatement's on decidable groups
        s64 = oref.beam_select(a64, b, W, N, acc.double(), ncoll)
        s32 = oref.beam_select(a32, b, W, N, acc, ncoll)
        coll = a64["colliding"].reshape(b, M)
        ok = beam_decidable(a64["cost"].reshape(b, M), oref._terms6(a64, b, M), coll, acc, ncoll, W, N, a32["cost"].reshape(b, M))
        oks.append(ok)
        for k in ("beam_row", "parent", "ncoll", "status"):
            assert torch.equal(s32[k][ok], s64[k][ok]), k
            assert torch.equal(o[k].long()[ok], s64[k][ok]), (name, draw, k, o[k], s64[k])
        # acc_out on the kernel's own slots includes w_obs * term
        on_slots = lambda a, ac: ac.gather(1, br // N) + a["q"].reshape(b, M).gather(1, br)
        got.append((o["acc"].reshape(-1), o["cost"].reshape(-1), o["obs_term"].reshape(-1)))
        r64.append((on_slots(a64, acc.double()).reshape(-1), a64["cost"], a64["term"]))
        r32.append((on_slots(a32, acc).reshape(-1), a32["cost"], a32["term"]))
    cat = lambda lst, j: torch.cat([v[j] for v in lst], 0)
    for j, what in enumerate(("acc", "cost", "obs_term")):
        held(name, what, cat(got, j), cat(r64, j), cat(r32, j))
    ok = torch.cat(oks)
    share = 1.0 - float(ok.float().mean())
    emit(f"| {name} | undecidable groups | {int((~ok).sum())} of {ok.numel()} | {share:.3f} | |")
    assert share <= UNDECIDABLE_CAP, (name, share)


def test_beam_acc_carries_the_obstacle_term(small_world):
    """one slot, goal-only weights: q is w_obs * term alone, so acc_out of the kept row is acc + w_obs * term"""
    x = _handmade(small_world, [3.0, 1.0, 2.0, 4.0], [0, 0, 0, 0])
    p64 = _pelvis64(x, 127, 1, 4)
    near = _obs((p64[1].numpy() + np.array([0.0, 0.5]))[None, None], RADIUS, frame0=0, w=2.0, margin=0.5)
    o, _ = _select_obs(x, 127, near, weights=GOAL_ONLY, beam=(1, 4), acc=torch.tensor([[0.25]]))
    assert o["beam_row"][0].tolist() == [1] and abs(float(o["acc"][0, 0]) - (0.25 + 2.0 * 0.3)) < 1e-4 and int(o["ncoll"][0, 0]) == 0
    assert abs(float(o["path_cost"][0, 0]) - (0.25 + 1.0 + 0.6)) < 1e-4


# ---- field and obstacles together --------------------------------------------------------------------------------------------
def test_field_and_obstacles_together(small_world):
    from tests.test_geodesic_gpu import _restate_field, _room_rows, _select_field
    b, N = 3, 5
    name = "select_obstacles with a field"
    got, r64, r32 = [], [], []
    for draw in range(-(-MIN_GROUP // (b * N))):
        x, fld = _room_rows(small_world, b, N, 800 + 1000 * draw)
        p64 = _pelvis64(x, 127, b, N)
        xy = np.stack([p64[g * N:(g + 1) * N, 10:11].numpy().repeat(6, 1) + np.array([0.45, 0.0]) for g in range(b)])     # [b,N,6,2]
        ob = _obs(xy, RADIUS, index=list(range(b)), frame0=0)
        o, i = _select_obs(x, 127, ob, fld=fld, findex=list(range(b)))
        with_field, _ = _select_field(x, 127, fld, list(range(b)))
        alone, _ = _select_obs(x, 127, ob)
        assert torch.equal(o["terms"], with_field["terms"])                       # the field's goal term, untouched by the obstacles
        for k in ("obs_term", "obs_clearance", "obs_hit"):
            assert torch.equal(o[k], alone[k]), k                                  # the obstacle outputs, untouched by the field
        res = []
        for dt in (torch.float64, torch.float32):
            geo, _, _, _ = _restate_field(i, fld, b, N, dt)
            res.append(_restate_obs(i, ob, b, N, dt, geo=geo.reshape(-1)))
        a64, a32 = res
        assert float(a64["term"].max()) > 0.05
        own6 = torch.cat([o["terms"], o["obs_term"][..., None]], -1)
        own, own_status = sref.select(o["cost"], own6, o["colliding"].bool())
        assert torch.equal(own, o["choice"].long()) and torch.equal(own_status.int(), o["status"])
        got.append(o["cost"].reshape(-1))
        r64.append(a64["cost"])
        r32.append(a32["cost"])
    held(name, "cost", torch.cat(got), torch.cat(r64), torch.cat(r32))


# ---- batch independence ----------------------------------------------------------------------------------------------------------
def test_select_obstacles_group_does_not_depend_on_batch(small_world):
    b, N, O, T = 65, 5, 32, 50
    x = _lattice(_rows_inputs(small_world, b, N, 31, True), b, N)
    index = torch.randperm(b, generator=torch.Generator().manual_seed(4)).tolist()
    ob = _obs(_tracks(_pelvis64(x, 127, b, N), b, N, O, T, 11, True, 0, index), RADIUS, index=index, frame0=11)
    full, _ = _select_obs(x, 127, ob)
    assert full["obs_hit"].any() and not full["obs_hit"].all()
    for g in (0, 1, 33, 64):
        one, _ = _select_obs(x, 127, ob, b=1, group0=g)
        for k in full:
            assert torch.equal(one[k][0], full[k][g]), (g, k)
    W = 5
    acc, ncoll = torch.rand(b, W, generator=torch.Generator().manual_seed(6)), torch.randint(0, 3, (b, W), dtype=torch.int32, generator=torch.Generator().manual_seed(7))
    full, _ = _select_obs(x, 127, ob, beam=(W, 1), acc=acc, ncoll=ncoll)
    for g in (0, 64):
        one, _ = _select_obs(x, 127, ob, b=1, group0=g, beam=(W, 1), acc=acc[g:g + 1], ncoll=ncoll[g:g + 1])
        for k in full:
            assert torch.equal(one[k][0], full[k][g]), (g, k)


# ---- bad arguments -------------------------------------------------------------------------------------------------------------
def test_obstacle_entries_reject_bad_arguments(small_world):
    """Rejected before anything is launched: every pointer may therefore be the same scratch buffer."""
    from egogen_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(16384, device="cuda")
    p, q = C.c_void_p(buf.data_ptr()), C.c_void_p(buf.data_ptr() + 4096)
    w = (C.c_float * 5)(1, 1, 1, 1, 0)

    def obs_tail(xy=p, radius=p, count=p, S=1, O=4, T=3, margin=0.5, body=0.3, term=p, clear=p, hit=p):
        return (xy, radius, count, None, S, O, T, 0, 1.0, margin, body, term, clear, hit)

    def sel(N=1, **kw):
        return lib.egx_primitive_select_obstacles(p, p, p, 201, p, 127, p, p, p, None, p, p, w, 40.0, 0.1, 0.5, 1, N, p, p, p, p, p, p, p,
                                                  *NULL_FIELD, *obs_tail(**kw), _lib.current_stream_ptr())

    def beam(W=1, N=1, **kw):
        return lib.egx_primitive_beam_select_obstacles(p, p, p, 201, p, 127, p, p, p, None, p, p, w, 40.0, 0.1, 0.5, 1, W, N, p, p, p, p, p, p, p, q,
                                                       q, p, p, p, p, *NULL_FIELD, *obs_tail(**kw), _lib.current_stream_ptr())
    bad = ({"O": 33}, {"O": -1}, {"T": 0}, {"S": 0}, {"xy": None}, {"radius": None}, {"count": None}, {"margin": -0.1}, {"body": -0.1},
           {"margin": float("nan")}, {"term": None}, {"clear": None}, {"hit": None}, {"N": 0}, {"N": 257})
    for kw in bad:
        for fn, what in ((sel, "egx_primitive_select_obstacles"), (beam, "egx_primitive_beam_select_obstacles")):
            assert fn(**kw) == -1, (what, kw)
            with pytest.raises(_lib.EgxError):
                _lib.check(fn(**kw), what)
    assert beam(W=33) == -1 and beam(W=32, N=9) == -1
    torch.cuda.synchronize()
    assert not buf.any()                                                          # nothing was launched


# ---- end to end ------------------------------------------------------------------------------------------------------------------
E2E_FIELDS = ("markers", "params", "rotmat", "transl", "pelvis", "z", "R0", "T0", "choice", "cost", "cost_terms", "colliding", "status",
              "goal_dist", "n_valid")


def _e2e(w, W, N, K, **extra):
    z = torch.randn(3, w["b"] * W * N, 128, generator=torch.Generator().manual_seed(70 + W))[:K]
    T0 = torch.tensor([[0.0, 0.0, 0.0], [3.0, 0.0, 0.0], [-3.0, 0.0, 0.0]])       # the three walkers start 3 m apart
    kw = dict(z=z, reproj_factor=CFG_RF, weights=W_TEST, goal_thresh=0.0, beam_width=W, to_numpy=False, T0=T0)
    kw.update(extra)
    return w["op"].generate_sequence_to_goal(w["data"], w["bparams"], w["betas"], w["goal"] + T0, K, N, **kw)


def _last_primitive_rows(s, res, K, W):
    """the rows of the last primitive of a run from the loop's own state: joints of all rows, and the frames they stood in"""
    J = s["lbs_out"]["joints"].reshape(-1, 20, 127, 3).cpu()
    rows = J.shape[0]
    if W == 1:
        M = rows // res.rotmat.shape[1]
        return J, res.rotmat[K - 1].cpu().repeat_interleave(M, 0), res.transl[K - 1].cpu().repeat_interleave(M, 0)
    return J, s["R0s"][(K - 1) % 2].cpu(), s["T0s"][(K - 1) % 2].cpu()


@pytest.mark.parametrize("W,N", [(1, 4), (2, 2)])
def test_generate_sequence_to_goal_with_obstacles(search_world, W, N):
    from egogen_amd import MovingObstacles
    w = search_world
    op, K, b, M = w["op"], 3, w["b"], W * N
    loop = "_search_loop" if W == 1 else "_beam_loop"
    base = _e2e(w, W, N, K)
    assert base.obstacle_term is None and base.clearance is None and base.obstacle_hit is None
    # (a) an empty set: the run without obstacles in every field
    empty = MovingObstacles.from_tracks(np.zeros((0, 5, 2)))
    res = _e2e(w, W, N, K, obstacles=empty)
    for k in E2E_FIELDS:
        assert torch.equal(getattr(res, k), getattr(base, k)), k
    assert empty.device == op.device                                               # moved at first use
    assert res.obstacle_term.shape == (K, b, M) and not res.obstacle_term.any() and not res.obstacle_hit.any()
    assert bool((res.clearance == float("inf")).all()) and res.search["clearance"] is res.clearance
    # (b) the earlier run's people as obstacles, the same z; (c) the loop is launches only
    people = MovingObstacles.from_sequences(base)
    assert people.count.tolist() == [b] and people.num_frames == 20 + 18 * (K - 1)
    radii = 0.3 + 0.3
    total = inside = 0
    for Kp in range(1, K + 1):                      # a run of Kp primitives is the prefix of the longer one: its last primitive from the loop's state
        with patched_loop(op, loop, no_host_wait=True) as seen:
            res = _e2e(w, W, N, Kp, obstacles=people)
        assert seen.calls == [(Kp, b, N) if W == 1 else (Kp, b, W, N)]
        if Kp > 1:
            for k in ("cost", "clearance", "obstacle_hit", "colliding") + (("choice", "status") if W == 1 else ()):     # a beam's path is chosen at the end
                assert torch.equal(getattr(res, k)[:Kp - 1], getattr(prev, k)), k
        prev = res
        J, R0, T0 = _last_primitive_rows(seen.s, res, Kp, W)
        t64 = oref.row_terms(R0, T0, J, people.xy, people.radius, people.count, np.zeros(b * M, np.int64), 18 * (Kp - 1), 0.5, 0.3, torch.float64)
        c64 = t64["clearance"].reshape(b, M)
        decided = (c64 <= -HIT_MARGIN) | (c64 >= HIT_MARGIN)
        total, inside = total + decided.numel(), inside + int((~decided).sum())
        hit, clear, coll = res.obstacle_hit[Kp - 1].cpu().bool(), res.clearance[Kp - 1].cpu(), res.colliding[Kp - 1].cpu().bool()
        assert torch.equal(hit[decided], t64["hit"].reshape(b, M)[decided])
        assert torch.equal(coll, hit)                                              # no scene: the hit is the collision
        assert float((clear.double() - c64).abs().max()) < 1e-4
        ch = res.choice[Kp - 1].cpu().long()
        chosen_hit = hit.gather(1, ch[:, None])[:, 0]
        assert torch.equal((res.status[Kp - 1].cpu() & 1).bool(), chosen_hit)
        if W == 1:                                  # wherever a group has a finite free row, the chosen row is no hit
            finite = torch.isfinite(res.cost[Kp - 1].cpu()) & torch.isfinite(res.obstacle_term[Kp - 1].cpu())
            free = (finite & ~hit).any(1)
            assert not chosen_hit[free].any()
        if Kp == 1:                                 # a row that repeats the earlier chosen path is a hit: it stands on that track
            own = base.choice[0].cpu().long()
            assert hit.gather(1, own[:, None]).all()
            assert float((clear.gather(1, own[:, None]) + radii).abs().max()) < 1e-4
    emit(f"| to_goal obstacles W={W} N={N} | rows within {HIT_MARGIN} m of contact | {inside} of {total} | {inside / total:.3f} | |")
    assert inside / total <= 0.05
    res_np = _e2e(w, W, N, K, obstacles=people, to_numpy=True)
    assert isinstance(res_np.clearance, np.ndarray) and np.array_equal(res_np.obstacle_hit, res.obstacle_hit.cpu().numpy())
    # (d) obstacle_frame0 reaches the kernel as frame0 + 18 k: an obstacle that stands, at ONE absolute frame, where the earlier
    # run's chosen row of primitive 1 has its pelvis at frame 10 (summed radii 5 mm); primitive 0 sees it 10 m away and is unchanged
    f64 = lambda t: t.double().cpu()
    base = _e2e(w, W, N, 2)
    spot = (torch.einsum("bij,bj->bi", f64(base.rotmat[1]), f64(base.pelvis[1, :, 10])) + f64(base.transl[1]))[:, :2].numpy()
    own1 = base.choice[1].cpu().long()
    for f0 in (0, 7):
        at = f0 + 18 + 10
        sets = [_one_frame_obstacle(spot[i], at + 5, at)[0] for i in range(b)]
        one = MovingObstacles.from_tracks(sets, radius=0.002)
        res = _e2e(w, W, N, 2, obstacles=one, body_radius=0.003, obstacle_weight=0.0, obstacle_frame0=f0)
        assert not res.obstacle_hit[0].any() and torch.equal(res.choice[0], base.choice[0]) and torch.equal(res.cost[0], base.cost[0])
        assert res.obstacle_hit[1].cpu().gather(1, own1[:, None]).all(), (f0, res.clearance[1])
        assert float((res.clearance[1].cpu().gather(1, own1[:, None]) + 0.005).abs().max()) < 1e-4
        far = _e2e(w, W, N, 2, obstacles=one, body_radius=0.003, obstacle_weight=0.0, obstacle_frame0=f0 + 40)
        assert not far.obstacle_hit.any()
        for k in E2E_FIELDS:
            assert torch.equal(getattr(far, k), getattr(base, k)), k
    # (e) argument errors
    with pytest.raises(TypeError, match="MovingObstacles"):
        _e2e(w, W, N, 1, obstacles=people.xy)
    with pytest.raises(ValueError, match=f"1 or {b} sets"):
        _e2e(w, W, N, 1, obstacles=MovingObstacles.from_tracks([np.zeros((1, 2, 2))] * 2))
    with pytest.raises(ValueError, match="names the set of 2 sequences"):
        _e2e(w, W, N, 1, obstacles=MovingObstacles.from_tracks([np.zeros((1, 2, 2))] * 2, index=[0, 1]))
    with pytest.raises(ValueError, match="the operator on"):
        _e2e(w, W, N, 1, obstacles=MovingObstacles.from_tracks(np.zeros((1, 2, 2))).to("cpu"))
    with pytest.raises(ValueError, match="must not be negative"):
        _e2e(w, W, N, 1, obstacles=people, obstacle_margin=-1.0)


def test_result_with_obstacles_saves_and_reloads(search_world, tmp_path):
    """a result with obstacle fields saves like any other, and its files are obstacles for the next person"""
    from egogen_amd import MovingObstacles
    w = search_world
    base = _e2e(w, 1, 4, 2, to_numpy=True)
    paths = [base.save(str(tmp_path), i, man_id=f"p_{i}") for i in range(w["b"])]
    people = MovingObstacles.from_rollout_files(paths)
    assert np.array_equal(people.xy, MovingObstacles.from_sequences(base).xy)
    res = _e2e(w, 1, 4, 2, obstacles=people, to_numpy=True)
    assert res.save(str(tmp_path), 0, man_id="q_0").endswith("motion_q_0.pkl") and res.obstacle_hit.shape == (2, w["b"], 4)


# ---- the driver ------------------------------------------------------------------------------------------------------------------
def test_gen_motion_driver_avoid(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    base = [sys.executable, os.path.join(ROOT, "exp_GAMMAPrimitive", "gen_motion.py"), "--n-primitives", "2", "--seed", "3", "--num-verts",
            str(V_SMALL), "--n-gens", "2", "--goal", "0.5,2.0,0.9", "--n-candidates", "4"]
    first, second = tmp_path / "first", tmp_path / "second"
    r = subprocess.run(base + ["--out", str(first)], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    files = sorted(str(first / f) for f in os.listdir(first) if f.startswith("motion_") and f.endswith(".pkl"))
    assert len(files) == 2 and "minimum clearance" not in r.stdout
    r = subprocess.run(base + ["--out", str(second), "--avoid", ",".join(files), "--start", "1.5,0.0,30"], cwd=str(tmp_path), env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert len([f for f in os.listdir(second) if f.startswith("motion_") and f.endswith(".pkl")]) == 2
    assert "avoiding 2 people over" in r.stdout
    lines = re.findall(r"variant (\d+): minimum clearance (-?[0-9.]+|inf) m, chosen hits (\d+)", r.stdout)
    assert [int(v[0]) for v in lines] == [0, 1], r.stdout[-1500:]
    assert all(np.isfinite(float(v[1])) for v in lines)
