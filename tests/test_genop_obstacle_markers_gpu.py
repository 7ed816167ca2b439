"""The marker model of recorded tracks on the device: entry egx_obstacle_marker_clearance (csrc/genop_obstacle_markers.hip), the
selection entries egx_primitive_select_obstacle_markers / egx_primitive_beam_select_obstacle_markers (the obstacle phase of
csrc/genop.hip on a table), `generate_sequence_to_goal(obstacles=, obstacle_model="markers")` and the driver's `--obstacle-model`,
against the restatement tests/genop_obstacle_markers_ref.py.

Yardsticks.  The clearance entry and the selection entries are compared BIT FOR BIT with the float32 restatement: include/egogen_hip.h
states every rounding of the frame clearance, the minimum is order-free, and everything after c_t is one rounded operation at a time
in a fixed tree.  The selection entries are fed a hand-made table and the rows as the device scored them without obstacles (the
*_field entries on the same inputs; the beam's q of every row from a beam launch of M slots of one candidate, whose acc_out is 0 + q),
so what is compared is what the marker entries add.  End to end, the recorded fields are the restatement of the loop's own buffers,
bit for bit, and the chosen clearance plus the skin is the evaluator's least marker distance (`crowd_metrics(hold=True)`, float64
from the same float32 records) to 16 ulps of the largest world coordinate involved - the allowance of
tests/test_genop_joint_markers_gpu.py for the same chain of float32 roundings."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import genop_obstacle_markers_ref as kref
from tests.genop_gpu_helpers import (CFG_RF, ROOT, V_SMALL, W_TEST, _rows_inputs, _selection_args, patched_loop,  # noqa: F401
                                     search_world, small_world)
from tests.test_genop_obstacles_gpu import E2E_FIELDS, NULL_FIELD, _e2e, _lattice
from tests.test_geodesic_gpu import _room_rows, _select_field

pytestmark = pytest.mark.gpu

SKIN, MARGIN, W_OBS = 0.05, 0.6, 1.7


def _bits_equal(got, want):
    """float arrays equal bit for bit, a NaN matching any NaN; integer and bool arrays equal"""
    got, want = (np.asarray(v.detach().cpu() if torch.is_tensor(v) else v) for v in (got, want))
    if got.shape != want.shape:
        return False
    if got.dtype.kind != "f":
        return bool(np.array_equal(got.astype(np.int64), want.astype(np.int64)))
    got, want = got.astype(np.float32), want.astype(np.float32)
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.int32)[~nan], want.view(np.int32)[~nan]))


def _report(name, got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    both = np.isfinite(got) & np.isfinite(want)
    diff = float(np.abs(got[both] - want[both]).max()) if both.any() else 0.0
    line = f"| {name} | entries {got.size} | NaN {int(np.isnan(want).sum())} | inf {int(np.isinf(want).sum())} | max |device - restatement| {diff:.3e} |"
    print(line)
    return line


# ---- the clearance entry -------------------------------------------------------------------------------------------------------------
def _clear(i, obs, count, index, frame0, skin, b, M, rf=CFG_RF):
    """egx_obstacle_marker_clearance on the launched rows i -> [b*M,18] numpy (NaN-filled before the launch: -7 marks nothing written)"""
    from egogen_amd import _lib
    dev = lambda a, dt: None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda().contiguous()
    d_obs, d_cnt, d_idx = dev(obs, torch.float32), dev(count, torch.int32), dev(index, torch.int32)
    out = torch.full((b * M, 18), -7.0, device="cuda")
    keep = [i[k].clone() for k in ("mp", "Y_gen", "R0", "T0")]
    S, O, T = obs.shape[:3]
    _lib.check(_lib.load().egx_obstacle_marker_clearance(
        _lib.ptr(i["mp"]), _lib.ptr(i["Y_gen"]), float(rf), _lib.ptr(i["R0"]), _lib.ptr(i["T0"]), b, M, _lib.ptr(d_obs), _lib.ptr(d_cnt),
        _lib.ptr(d_idx), S, O, T, int(frame0), float(skin), _lib.ptr(out), _lib.current_stream_ptr()), "egx_obstacle_marker_clearance")
    torch.cuda.synchronize()
    for k, v in zip(("mp", "Y_gen", "R0", "T0"), keep):
        assert _bits_equal(i[k], v), k                                                       # the inputs are only read
    return out.cpu().numpy()


def _near_miss_shift(w64_row, frames, target):
    """the vertical shift s at which a copy of the row's own cloud (track frame a = the row's predicted frame frames[a]), lifted by s,
    is `target` metres clear of the row over the window frame0 = -3: bisection on a continuous function of s, in float64"""
    def c(s):
        track = (w64_row[frames] + np.array([0.0, 0.0, s]))[None, None]
        return float(kref.frame_clearance64(w64_row[None], track, [1], [0], -3, SKIN).min())
    lo, hi = 0.0, 4.0
    assert c(lo) < target < c(hi)
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if c(mid) < target else (lo, mid)
    return hi


def test_obstacle_marker_clearance_kernel(small_world):
    """b = 3 sequences of 5 rows on a lattice 3 m apart; S = 2 sets with an index, counts 0 and 5 (ragged against a register block of
    4), T = 7, frame0 = -3: absolute frame clamp(f - 1, 0, 6), both clamps inside the window.  The tracks are the rows' own clouds
    plus offsets: 2 cm aside (contact), lifted clear by 0.3 m (inside the margin), and the fifth track alone touches its row."""
    b, M, S, O, T, frame0 = 3, 5, 2, 5, 7, -3
    x = _lattice(_rows_inputs(small_world, b, M, 431, False), b, M)
    _, i, _, _alive = _selection_args(x, b, M, 0, 127, CFG_RF, W_TEST, 40.0, 0.1, ())
    w64 = kref.world_markers64(i["R0"], i["T0"], i["mp"], i["Y_gen"], CFG_RF)
    frames = np.arange(T) + 1                                       # track frame a stands where the row is at predicted frame a + 1
    obs = np.zeros((S, O, T, 67, 3))
    obs[..., 0], obs[..., 1] = -500.0, 400.0                        # set 0 is padding only: its count is 0
    plan = [(0, "hit"), (1, "near"), (10, "hit"), (11, "near"), (12, "hit")]
    for o, (row, kind) in enumerate(plan):
        off = np.array([0.02, 0.0, 0.0]) if kind == "hit" else np.array([0.0, 0.0, _near_miss_shift(w64[row], frames, 0.3)])
        obs[1, o] = w64[row][frames] + off
    obs = obs.astype(np.float32)
    count, index = np.array([0, 5], np.int32), np.array([1, 0, 1], np.int32)
    set_of_row = np.repeat(index, M)
    bad_row, bad_frame = 3, 4
    i["Y_gen"].view(18, b * M, 67, 3)[bad_frame, bad_row, 65, 1] = float("nan")          # one marker of one frame of one row; 65: the lanes' tail
    w32 = kref.world_markers32(i["R0"], i["T0"], i["mp"], i["Y_gen"], CFG_RF)
    want = kref.frame_clearance32(w32, obs, count, set_of_row, frame0, SKIN)
    # coverage, on the restatement first
    nan = np.zeros((b * M, 18), bool)
    nan[bad_row, bad_frame] = True
    assert np.array_equal(np.isnan(want), nan)                                          # NaN there and only there
    assert np.isposinf(want[5:10]).all()                                                # the empty set
    row_min = np.where(nan, np.inf, want).min(1)
    assert (row_min[[0, 10, 12]] < 0).all(), row_min
    assert ((row_min[[1, 11]] > 0) & (row_min[[1, 11]] < MARGIN)).all(), row_min
    assert (row_min[[2, 3, 4, 13, 14]] > MARGIN).all() and np.isfinite(row_min[[2, 3, 4, 13, 14]]).all(), row_min
    assert kref.frames_of(frame0, T).tolist() == [0, 0, 1, 2, 3, 4, 5] + [6] * 11
    got = _clear(i, obs, count, index, frame0, SKIN, b, M)
    line = _report("obstacle_marker_clearance b=3 M=5 S=2 O=5 T=7", got, want)
    assert _bits_equal(got, want), line
    # the fifth track counts: without it row 12 is clear
    four = _clear(i, obs, np.array([0, 4], np.int32), index, frame0, SKIN, b, M)
    assert np.nanmin(four[12]) > MARGIN and _bits_equal(four[:12], want[:12])
    # no index: every sequence reads set 0, the empty one
    assert np.array_equal(np.isnan(_clear(i, obs, count, None, frame0, SKIN, b, M)), nan)
    assert np.isposinf(_clear(i, obs, count, None, frame0, SKIN, b, M)[~nan]).all()
    # a group's rows are the same bits in a batch of one: sequence 2 alone
    sel = slice(2 * M, 3 * M)
    one = {"mp": i["mp"].reshape(b * M, 20, 67, 3)[sel].contiguous(), "Y_gen": i["Y_gen"][:, sel].contiguous(), "R0": i["R0"][sel].contiguous(),
           "T0": i["T0"][sel].contiguous()}
    assert _bits_equal(_clear(one, obs, count, index[2:], frame0, SKIN, 1, M), want[sel])


def test_clearance_entry_rejects_bad_arguments():
    """Rejected before anything is launched: every pointer may therefore be the same scratch buffer."""
    from egogen_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(16384, device="cuda")
    p = C.c_void_p(buf.data_ptr())

    def call(mp=p, yg=p, rf=0.5, R0=p, T0=p, b=1, M=1, obs=p, count=p, S=1, O=4, T=3, skin=0.05, out=p):
        return lib.egx_obstacle_marker_clearance(mp, yg, rf, R0, T0, b, M, obs, count, None, S, O, T, 0, skin, out, _lib.current_stream_ptr())
    bad = ({"mp": None}, {"yg": None}, {"R0": None}, {"T0": None}, {"obs": None}, {"count": None}, {"out": None}, {"skin": -0.01},
           {"skin": float("nan")}, {"skin": float("inf")}, {"T": 0}, {"O": 33}, {"O": -1}, {"S": 0}, {"b": 0}, {"M": 0}, {"M": 257}, {"rf": 1.5})
    for kw in bad:
        assert call(**kw) == -1, kw
        with pytest.raises(_lib.EgxError):
            _lib.check(call(**kw), "egx_obstacle_marker_clearance")
    torch.cuda.synchronize()
    assert not buf.any()                                                          # nothing was launched


# ---- the selection entries on a hand-made table ------------------------------------------------------------------------------------
def _table(b, M, seed):
    """[b*M,18] float32: frames on either side of 0 and of the margin; whole rows clear, +inf (nobody there) and in contact; a NaN frame"""
    g = np.random.default_rng(seed)
    t = g.uniform(-0.15, 1.1, size=(b * M, 18)).astype(np.float32)
    t[1] = np.float32(np.inf)
    t[2] = g.uniform(0.7, 2.0, size=18)
    t[3] = g.uniform(0.01, 0.55, size=18)
    t[M + 1, 7] = np.float32(np.nan)
    t[M + 2, 3] = np.float32(-0.0)
    t[2 * M:] = np.abs(t[2 * M:]) + np.float32(0.001)                # the last sequence has no contact: the term alone orders it
    return t


def _select_table(x, jpb, table, fld=None, findex=None, beam=None, acc=None, ncoll=None, w=W_OBS, margin=MARGIN):
    """egx_primitive_select_obstacle_markers (beam = (W, N): egx_primitive_beam_select_obstacle_markers) on the row set x with the table
    and the fields `fld` (None: a null field) -> outputs on the CPU"""
    from egogen_amd import _lib
    b, M = x["b"], x["N"]
    lead, i, o, _alive = _selection_args(x, b, M, 0, jpb, CFG_RF, W_TEST, 40.0, 0.1, ())
    fi = lambda *s: torch.full(s, -7, dtype=torch.int32, device="cuda")
    ff = lambda *s: torch.full(s, float("nan"), device="cuda")
    if fld is None:
        fa, fidx = NULL_FIELD, None
    else:
        fidx = torch.as_tensor(findex, dtype=torch.int32, device="cuda")
        fa = (_lib.ptr(fld.dist), _lib.ptr(fld.origin), float(np.float32(fld.cell)), fld.dist.shape[1], fld.dist.shape[2], len(fld), _lib.ptr(fidx))
    d_table = torch.as_tensor(table).cuda().contiguous()
    o.update({"obs_term": ff(b, M), "obs_clearance": ff(b, M), "obs_hit": fi(b, M)})
    oa = (_lib.ptr(d_table), float(w), float(margin), _lib.ptr(o["obs_term"]), _lib.ptr(o["obs_clearance"]), _lib.ptr(o["obs_hit"]))
    if beam is None:
        o = {"choice": fi(b), "status": fi(b), "reached": fi(b), "goal_dist": ff(b), **o}
        _lib.check(_lib.load().egx_primitive_select_obstacle_markers(
            *lead, b, M, _lib.ptr(o["choice"]), _lib.ptr(o["status"]), _lib.ptr(o["reached"]), _lib.ptr(o["goal_dist"]), _lib.ptr(o["cost"]),
            _lib.ptr(o["terms"]), _lib.ptr(o["colliding"]), *fa, *oa, _lib.current_stream_ptr()), "egx_primitive_select_obstacle_markers")
    else:
        W, N = beam
        acc_d, ncoll_d = acc.float().cuda().contiguous(), ncoll.int().cuda().contiguous()
        o.update({"beam_row": fi(b, W), "parent": fi(b, W), "acc": ff(b, W), "ncoll": fi(b, W), "path_cost": ff(b, W), "status": fi(b, W),
                  "goal_dist": ff(b, W), "reached": fi(b, W)})
        _lib.check(_lib.load().egx_primitive_beam_select_obstacle_markers(
            *lead, b, W, N, _lib.ptr(acc_d), _lib.ptr(ncoll_d), _lib.ptr(o["cost"]), _lib.ptr(o["terms"]), _lib.ptr(o["colliding"]),
            _lib.ptr(o["beam_row"]), _lib.ptr(o["parent"]), _lib.ptr(o["acc"]), _lib.ptr(o["ncoll"]), _lib.ptr(o["path_cost"]),
            _lib.ptr(o["status"]), _lib.ptr(o["goal_dist"]), _lib.ptr(o["reached"]), *fa, *oa, _lib.current_stream_ptr()),
            "egx_primitive_beam_select_obstacle_markers")
    torch.cuda.synchronize()
    assert _bits_equal(d_table, table)                                                      # the table is only read
    return {k: v.cpu() for k, v in o.items()}


def _rows(world, b, M, seed, with_field):
    if with_field:
        x, fld = _room_rows(world, b, M, seed)
        return x, fld, list(range(b))
    return _rows_inputs(world, b, M, seed, True), None, None


@pytest.mark.parametrize("with_field", [False, True])
def test_select_obstacle_markers_entry(small_world, with_field):
    b, N = 3, 5
    x, fld, findex = _rows(small_world, b, N, 520, with_field)
    table = _table(b, N, 1)
    prev, _ = _select_field(x, 127, fld, findex)                    # the rows as the device scores them without obstacles
    o = _select_table(x, 127, table, fld, findex)
    t = kref.terms_of_clearance(table, MARGIN)
    assert bool((t["term"] > 0).any()) and bool(t["hit"].any()) and bool(torch.isnan(t["term"]).any()) and bool((t["term"] == 0).any())
    a = kref.apply_rows(prev["cost"], prev["terms"], prev["colliding"], t, W_OBS)
    choice, status = kref.select(a, b, N)
    for k, want in (("obs_term", t["term"]), ("obs_clearance", t["clearance"]), ("obs_hit", t["hit"]), ("cost", a["cost"]),
                    ("colliding", a["colliding"]), ("choice", choice), ("status", status), ("terms", prev["terms"])):
        assert _bits_equal(o[k].reshape(-1), want.reshape(-1)), (k, _report(f"select_obstacle_markers field={with_field} {k}", o[k].reshape(-1).numpy(), want.reshape(-1).numpy()))
    assert not _bits_equal(o["cost"], prev["cost"]) and not _bits_equal(o["colliding"], prev["colliding"])      # the table counts
    euclid = _select_field(x, 127, None, None)[0]["terms"][..., 0]                          # goal_dist stays the straight line, field or not
    assert _bits_equal(o["goal_dist"], euclid.gather(1, o["choice"].long()[:, None])[:, 0])
    assert torch.equal(o["reached"].bool(), o["goal_dist"] < 0.1)


@pytest.mark.parametrize("with_field", [False, True])
def test_beam_select_obstacle_markers_entry(small_world, with_field):
    b, W, N = 3, 2, 3
    M = W * N
    x, fld, findex = _rows(small_world, b, M, 530, with_field)
    table = _table(b, M, 2)
    g = torch.Generator().manual_seed(4)
    acc, ncoll = torch.rand(b, W, generator=g) * 6.0, torch.randint(0, 3, (b, W), generator=g, dtype=torch.int32)
    prev, _ = _select_field(x, 127, fld, findex, beam=(W, N), acc=acc, ncoll=ncoll)
    every, _ = _select_field(x, 127, fld, findex, beam=(M, 1))     # M slots of one candidate, acc 0: every row is kept, acc_out = 0 + q
    q = torch.full((b, M), float("nan"))
    q.scatter_(1, every["beam_row"].long(), every["acc"])
    assert bool(torch.isfinite(q).all()) and _bits_equal(every["cost"], prev["cost"])
    o = _select_table(x, 127, table, fld, findex, beam=(W, N), acc=acc, ncoll=ncoll)
    t = kref.terms_of_clearance(table, MARGIN)
    a = kref.apply_rows(prev["cost"], prev["terms"], prev["colliding"], t, W_OBS, q=q)
    s = kref.beam_select(a, b, W, N, acc, ncoll)
    for k, want in (("obs_term", t["term"]), ("obs_clearance", t["clearance"]), ("obs_hit", t["hit"]), ("cost", a["cost"]),
                    ("colliding", a["colliding"]), ("terms", prev["terms"]), ("beam_row", s["beam_row"]), ("parent", s["parent"]),
                    ("acc", s["acc"]), ("ncoll", s["ncoll"]), ("path_cost", s["path_cost"]), ("status", s["status"])):
        assert _bits_equal(o[k].reshape(-1), want.reshape(-1)), (k, _report(f"beam_select_obstacle_markers field={with_field} {k}", o[k].reshape(-1).numpy(), want.reshape(-1).numpy()))
    assert not _bits_equal(o["cost"], prev["cost"]) and not _bits_equal(o["acc"], prev["acc"])      # the table counts, along the path too
    # the greedy entry on the same rows and table: the same rows' values
    greedy = _select_table(x, 127, table, fld, findex)
    for k in ("cost", "terms", "colliding", "obs_term", "obs_clearance", "obs_hit"):
        assert _bits_equal(o[k], greedy[k]), k


def test_selection_entries_reject_bad_arguments():
    from egogen_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(16384, device="cuda")
    p, q = C.c_void_p(buf.data_ptr()), C.c_void_p(buf.data_ptr() + 4096)
    w = (C.c_float * 5)(1, 1, 1, 1, 0)

    def tail(table=p, margin=0.5, term=p, clear=p, hit=p):
        return (table, 1.0, margin, term, clear, hit)

    def sel(N=1, **kw):
        return lib.egx_primitive_select_obstacle_markers(p, p, p, 201, p, 127, p, p, p, None, p, p, w, 40.0, 0.1, 0.5, 1, N, p, p, p, p, p, p, p,
                                                         *NULL_FIELD, *tail(**kw), _lib.current_stream_ptr())

    def beam(W=1, N=1, **kw):
        return lib.egx_primitive_beam_select_obstacle_markers(p, p, p, 201, p, 127, p, p, p, None, p, p, w, 40.0, 0.1, 0.5, 1, W, N, p, p, p, p, p,
                                                              p, p, q, q, p, p, p, p, *NULL_FIELD, *tail(**kw), _lib.current_stream_ptr())
    for kw in ({"table": None}, {"margin": -0.1}, {"margin": float("nan")}, {"term": None}, {"clear": None}, {"hit": None}, {"N": 0}, {"N": 257}):
        for fn, what in ((sel, "egx_primitive_select_obstacle_markers"), (beam, "egx_primitive_beam_select_obstacle_markers")):
            assert fn(**kw) == -1, (what, kw)
            with pytest.raises(_lib.EgxError):
                _lib.check(fn(**kw), what)
    assert beam(W=33) == -1 and beam(W=32, N=9) == -1
    torch.cuda.synchronize()
    assert not buf.any()                                                          # nothing was launched


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    if not torch.is_tensor(a):
        return a == b
    return a.shape == b.shape and bool(((a == b) | (torch.isnan(a.float()) & torch.isnan(b.float()))).all())


@pytest.mark.parametrize("W,N", [(1, 4), (2, 2)])
def test_explicit_cylinder_is_the_default(search_world, W, N):
    from egogen_amd import MovingObstacles
    w = search_world
    first = _e2e(w, W, N, 2)
    people = MovingObstacles.from_sequences(first, markers=True)                  # markers on board change nothing for the cylinders
    near = torch.tensor([[0.4, 0.0, 0.0], [3.4, 0.0, 0.0], [-2.6, 0.0, 0.0]])
    base = _e2e(w, W, N, 2, obstacles=MovingObstacles.from_sequences(first), T0=near)
    res = _e2e(w, W, N, 2, obstacles=people, T0=near, obstacle_model="cylinder", obstacle_skin=0.2)
    assert bool(base.obstacle_term.gt(0).any())
    for k in E2E_FIELDS + res.OBSTACLE_FIELDS:
        assert _same(getattr(res, k), getattr(base, k)), k
    assert res.search["obstacle_model"] == base.search["obstacle_model"] == "cylinder" and base.search["obstacle_skin"] == 0.05
    assert _e2e(w, W, N, 1).search.get("obstacle_model") is None                  # no obstacles: no model on record


@pytest.mark.parametrize("W,N", [(1, 4), (2, 4)])
def test_generate_sequence_to_goal_with_obstacle_markers(search_world, W, N, tmp_path):
    """Person 1 (three sequences, K = 3, N = 4), then person 2 from seeds half a metre beside them.  So that a row inside the margin
    exists whatever the seeded prior does, the obstacles also hold person 2's own first choice of a run without obstacles, 0.3 m
    aside: a `PrimitiveSequence` like the others, so the evaluator reads the same records."""
    from egogen_amd import MovingObstacles
    from egogen_amd.metrics import MotionSet, crowd_metrics
    w = search_world
    op, K, b, M = w["op"], 3, w["b"], W * N
    loop = "_search_loop" if W == 1 else "_beam_loop"
    margin = 0.5
    base = _e2e(w, 1, 4, K)
    near = torch.tensor([[0.5, 0.0, 0.0], [3.5, 0.0, 0.0], [-2.5, 0.0, 0.0]])
    ghost = _e2e(w, W, N, 1, T0=near)
    ghost.transl = ghost.transl + torch.tensor([0.0, 0.3, 0.0], device=ghost.transl.device)
    people = MovingObstacles.from_sequences([base, ghost], markers=True)
    assert people.count.tolist() == [2 * b] and people.markers.shape == (1, 2 * b, 20 + 18 * (K - 1), 67, 3)
    felt = 0
    for Kp in range(1, K + 1):                      # a run of Kp primitives is the prefix of the longer one: its last primitive from the loop's state
        with patched_loop(op, loop, no_host_wait=True) as seen:
            res = _e2e(w, W, N, Kp, T0=near, obstacles=people, obstacle_model="markers", obstacle_skin=SKIN)
        assert seen.calls == [(Kp, b, N) if W == 1 else (Kp, b, W, N)]
        if Kp > 1:
            for k in ("cost", "clearance", "obstacle_term", "obstacle_hit", "colliding") + (("choice", "status") if W == 1 else ()):
                assert _same(getattr(res, k)[:Kp - 1], getattr(prev, k)), k
        prev = res
        s = seen.s
        assert s["frame_clearance"].shape == (b * M, 18)
        if W == 1:
            R0, T0 = res.rotmat[Kp - 1].repeat_interleave(M, 0), res.transl[Kp - 1].repeat_interleave(M, 0)
        else:
            R0, T0 = s["R0s"][(Kp - 1) % 2], s["T0s"][(Kp - 1) % 2]
        w32 = kref.world_markers32(R0, T0, s["lbs_out"]["markers"].reshape(b * M, 20, 67, 3), s["Y_gen"], CFG_RF)
        c32 = kref.frame_clearance32(w32, people.markers, people.count, np.zeros(b * M, np.int64), 18 * (Kp - 1), SKIN)
        assert _bits_equal(s["frame_clearance"], c32), _report(f"e2e W={W} k={Kp - 1} table", s["frame_clearance"].cpu().numpy(), c32)
        t = kref.terms_of_clearance(c32, margin)
        for k, want in (("clearance", t["clearance"]), ("obstacle_term", t["term"]), ("obstacle_hit", t["hit"])):
            assert _bits_equal(getattr(res, k)[Kp - 1].reshape(-1), want), (Kp, k)
        felt += int((t["term"] > 0).sum())
        hit = res.obstacle_hit[Kp - 1].cpu().bool()
        assert torch.equal(res.colliding[Kp - 1].cpu().bool(), hit)                          # no scene: the hit is the collision
        ch = res.choice[Kp - 1].cpu().long()
        assert torch.equal((res.status[Kp - 1].cpu() & 1).bool(), hit.gather(1, ch[:, None])[:, 0])
    assert felt > 0                                                                          # a scored row inside the margin
    assert res.search["obstacle_model"] == "markers" and res.search["obstacle_skin"] == SKIN
    assert int(res.n_valid.min()) == K
    # the search against the instrument: the chosen row's clearance + skin is the evaluator's least marker distance between person 2
    # and the recorded people over the frames 18 k + 2 .. 18 k + 19, the ended ghost held where it stopped
    cm = crowd_metrics(MotionSet.from_sequences([base, ghost, res]), groups=np.zeros(3 * b, np.int64), hold=True)
    md, pi, pj = torch.as_tensor(cm["marker_dist"]), cm["pair"]["i"], cm["pair"]["j"]
    worlds = [torch.einsum("kbij,kbtaj->kbtai", q.rotmat.double().cpu(), q.markers.double().cpu()) + q.transl.double().cpu()[:, :, None, None]
              for q in (base, ghost, res)]
    big = max(float(v.abs().max()) for v in worlds)
    bound = 16.0 * 2.0 ** (np.floor(np.log2(big)) - 23)
    for k in range(K):
        for i in range(b):
            me = 2 * b + i
            mine = [q for q in range(len(pi)) if (int(pi[q]) == me and int(pj[q]) < 2 * b) or (int(pj[q]) == me and int(pi[q]) < 2 * b)]
            assert len(mine) == 2 * b
            least = float(md[mine, 18 * k + 2:18 * k + 20].min())
            got = float(res.clearance[k, i, int(res.choice[k, i])].double()) + SKIN
            print(f"| e2e obstacle markers W={W} | k {k} sequence {i} | evaluator {least:.9f} | search {got:.9f} | bound {bound:.3e} |")
            assert abs(got - least) <= bound, (k, i, got, least, bound)
    # the search keys survive save, and the files are marker obstacles for the next person
    res_np = _e2e(w, W, N, K, T0=near, obstacles=people, obstacle_model="markers", obstacle_skin=SKIN, to_numpy=True)
    before = {k: np.array(getattr(res_np, k)) for k in res_np.OBSTACLE_FIELDS}
    paths = [res_np.save(str(tmp_path), i, man_id=f"p_{i}") for i in range(b)]
    for k in res_np.OBSTACLE_FIELDS:
        assert np.array_equal(getattr(res_np, k), before[k], equal_nan=True) and res_np.search[k] is getattr(res_np, k), k
        assert _bits_equal(before[k], getattr(res, k)), k
    assert res_np.search["obstacle_model"] == "markers" and res_np.search["obstacle_skin"] == SKIN
    assert np.array_equal(MovingObstacles.from_rollout_files(paths, markers=True).markers, MovingObstacles.from_sequences(res_np, markers=True).markers)
    # argument errors of the device path
    with pytest.raises(ValueError, match="carry markers"):
        _e2e(w, W, N, 1, obstacles=MovingObstacles.from_sequences(base), obstacle_model="markers")
    with pytest.raises(ValueError, match="the operator on"):
        _e2e(w, W, N, 1, obstacles=MovingObstacles.from_sequences(base, markers=True).to("cpu"), obstacle_model="markers")


def test_obstacle_markers_with_groups(search_world):
    """the marker model of the obstacles under the joint step: the selection's rows carry its term, the joint launch reads them"""
    from egogen_amd import MovingObstacles
    w = search_world
    base = _e2e(w, 1, 4, 1)
    near = torch.tensor([[0.5, 0.0, 0.0], [3.5, 0.0, 0.0], [-2.5, 0.0, 0.0]])
    people = MovingObstacles.from_sequences(base, markers=True)
    alone = _e2e(w, 1, 4, 1, T0=near, obstacles=people, obstacle_model="markers")
    for pair_model in ("cylinder", "markers"):
        res = _e2e(w, 1, 4, 1, T0=near, obstacles=people, obstacle_model="markers", groups=[0, 1, 2], pair_model=pair_model)
        for k in E2E_FIELDS + res.OBSTACLE_FIELDS:                                           # groups of one: the search without groups
            assert _same(getattr(res, k), getattr(alone, k)), (pair_model, k)
    assert bool(alone.obstacle_term.gt(0).any())


# ---- the driver ----------------------------------------------------------------------------------------------------------------------
def test_gen_motion_driver_obstacle_model(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    base = [sys.executable, os.path.join(ROOT, "exp_GAMMAPrimitive", "gen_motion.py"), "--n-primitives", "2", "--seed", "3", "--num-verts",
            str(V_SMALL), "--n-gens", "2", "--goal", "0.5,2.0,0.9", "--n-candidates", "4"]
    first, second = tmp_path / "first", tmp_path / "second"
    r = subprocess.run(base + ["--out", str(first)], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    files = sorted(str(first / f) for f in os.listdir(first) if f.startswith("motion_") and f.endswith(".pkl"))
    r = subprocess.run(base + ["--out", str(second), "--avoid", ",".join(files), "--start", "0.6,0.0,10", "--obstacle-model", "markers",
                               "--obstacle-skin", "0.06"], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert len([f for f in os.listdir(second) if f.startswith("motion_") and f.endswith(".pkl")]) == 2
    assert "avoiding 2 people over" in r.stdout and "by their markers" in r.stdout
    lines = re.findall(r"variant (\d+): minimum clearance (-?[0-9.]+|inf) m, chosen hits (\d+)", r.stdout)
    assert [int(v[0]) for v in lines] == [0, 1], r.stdout[-1500:]
    assert all(np.isfinite(float(v[1])) for v in lines)
