"""Look-ahead in the primitive search on the device: entries egx_obstacle_ahead_clearance (csrc/genop_obstacle_ahead.hip) and
egx_primitive_select_joint_ahead (csrc/genop_joint_ahead.hip), `generate_sequence_to_goal(lookahead=, lookahead_slack=)` and the
driver's `--lookahead`, against the restatement tests/genop_lookahead_ref.py.

Yardsticks.  Both entries are compared BIT FOR BIT with the float32 restatement (`bits=True`: numpy's one rounding per operation, a
correctly rounded root, the fused nesting of the world pelvis, the wave reduction's summation tree), a NaN truth held exactly:
include/egogen_hip.h states every rounding, and a minimum is order-free.  With H = 0 the entries are compared with the entries they
extend, bit for bit.  Every member step of the joint entry is checked on its own from the state the device's own `choice_trace`
gives, and its choice is the order (class, joint_cost, n) on the restatement's values, which are the device's."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import genop_lookahead_ref as lref
from tests import genop_obstacle_markers_ref as kref
from tests import test_genop_joint_gpu as jg
from tests.genop_gpu_helpers import (CFG_RF, ROOT, V_SMALL, W_TEST, _rows_inputs, _selection_args, patched_loop,  # noqa: F401
                                     search_world, small_world)
from tests.test_genop_obstacle_markers_gpu import _bits_equal, _report, _select_table
from tests.test_genop_obstacles_gpu import E2E_FIELDS, NULL_FIELD, _e2e, _lattice, _obs, _select_obs

pytestmark = pytest.mark.gpu

BODY, MARGIN, W_OBS, SLACK = 0.1, 0.6, 1.7, 0.07
ZERO_W = {"goal": 0.0, "skate": 0.0, "floor": 0.0, "pene": 0.0, "face": 0.0}


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def _plant20(i, xy, frames=tuple(range(1, 20))):
    """joint 0 of the frames `frames` of the launched joints i["J"] rewritten so that the world xy of row r at frame t is xy[r, t]
    ([rows,20,2]; the other frames are left alone); z stays: local = R0^T (world - T0) in float64, rounded once"""
    n, f = i["J"].shape[0], list(frames)
    R0, T0 = i["R0"].double().cpu(), i["T0"].double().cpu()
    world = torch.einsum("bij,btj->bti", R0, i["J"][:, f, 0, :].double().cpu()) + T0[:, None]
    world[..., :2] = torch.as_tensor(np.asarray(xy, np.float64)).reshape(n, 20, 2)[:, f]
    i["J"][:, f, 0, :] = torch.einsum("bji,btj->bti", R0, world - T0[:, None]).float().to(i["J"].device)


def _walks(rows, origin, seed, speed=0.05, spread=1.5):
    """[rows,20,2] float64: every row a straight walk from a point within `spread` m of its origin ([rows,2]) at up to `speed` m a frame,
    plus a wiggle of 0.01 m"""
    g = np.random.default_rng(seed)
    t = np.arange(20)[None, :, None]
    ang, v = g.uniform(0, 2 * np.pi, rows), g.uniform(0.2, 1.0, rows) * speed
    vel = np.stack([np.cos(ang), np.sin(ang)], -1) * v[:, None]
    return np.asarray(origin)[:, None, :] + g.uniform(-spread, spread, (rows, 1, 2)) + vel[:, None, :] * t + g.normal(size=(rows, 20, 2)) * 0.01


# ---- the clearance entry -------------------------------------------------------------------------------------------------------------
def _ahead_clear(i, jpb, xy, radius, count, index, frame0, body, H, slack, b, M):
    """egx_obstacle_ahead_clearance on the launched rows i -> [b*M,18] numpy (filled with -7 before the launch: nothing written)"""
    from egogen_amd import _lib
    dev = lambda a, dt: None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda().contiguous()
    d_xy, d_r, d_cnt, d_idx = dev(xy, torch.float32), dev(radius, torch.float32), dev(count, torch.int32), dev(index, torch.int32)
    out = torch.full((b * M, 18), -7.0, device="cuda")
    keep = [i[k].clone() for k in ("J", "R0", "T0")]
    S, O, T = xy.shape[:3]
    _lib.check(_lib.load().egx_obstacle_ahead_clearance(
        _lib.ptr(i["J"]), jpb, _lib.ptr(i["R0"]), _lib.ptr(i["T0"]), b, M, _lib.ptr(d_xy), _lib.ptr(d_r), _lib.ptr(d_cnt), _lib.ptr(d_idx), S, O, T,
        int(frame0), float(body), int(H), float(slack), _lib.ptr(out), _lib.current_stream_ptr()), "egx_obstacle_ahead_clearance")
    torch.cuda.synchronize()
    for k, v in zip(("J", "R0", "T0"), keep):
        assert _bits_equal(i[k], v), k                                                       # the inputs are only read
    return out.cpu().numpy()


def _tracks_near(p64, b, M, S, O, T, index, seed):
    """xy [S,O,T,2] float64: set index[g] holds O tracks that start within 1.2 m of where a row of sequence g stands at frame 10 and walk
    at up to 0.04 m a frame; a set no sequence names stands far away"""
    g = np.random.default_rng(seed)
    xy = np.zeros((S, O, T, 2))
    xy[..., 0], xy[..., 1] = -500.0, 400.0
    t = np.arange(T)[None, :, None]
    for grp, s in enumerate(index):
        at = p64[grp * M + np.arange(O) % M, 10]                                             # [O,2]
        ang, v = g.uniform(0, 2 * np.pi, O), g.uniform(0, 0.04, O)
        xy[s] = at[:, None, :] + g.uniform(-1.2, 1.2, (O, 1, 2)) + (np.stack([np.cos(ang), np.sin(ang)], -1) * v[:, None])[:, None, :] * t
    return xy


# b, M, counts of the S sets, obs_index (None: set 0), O_max, T, frame0
CLEAR_CASES = {
    "b1 M1 one track": (1, 1, [1], None, 1, 1, 0),
    "b3 M5 ragged sets": (3, 5, [0, 1, 5, 32], [3, 0, 2], 32, 25, -4),
    "b3 M33 second batch of rows": (3, 33, [0, 1, 5, 32], [1, 2, 3], 32, 40, 7),
    "b1 M5 five of eight": (1, 5, [5], None, 8, 30, 3),
}


@pytest.mark.parametrize("case", list(CLEAR_CASES))
def test_obstacle_ahead_clearance_kernel(small_world, case):
    """The rows walk straight (planted tracks, frames 1..19); the tracks of a sequence's set start near its rows.  T is short: the
    absolute frames frame0 + t + 18 h run past T - 1 from h = 1 on (and, with a negative frame0, start below 0).  One row has a NaN pelvis
    at frame 19 only - one NaN frame at H = 0, a NaN row from H = 1 on - and one track has a NaN frame inside the window.  Where a
    sequence reads an empty set, one of its rows has that NaN too (NaN, not +inf: the row's own prediction is not a number), and with
    several sequences one row has an infinite pelvis at frame 1: an infinite displacement, every c_{t,h} = +inf, the row as at H = 0."""
    b, M, counts, index, O, T, frame0 = CLEAR_CASES[case]
    S, jpb = len(counts), 127
    x = _lattice(_rows_inputs(small_world, b, M, 611, False), b, M)
    _, i, _, _alive = _selection_args(x, b, M, 0, jpb, CFG_RF, W_TEST, 40.0, 0.1, ())
    _plant20(i, _walks(b * M, i["T0"][:, :2].double().cpu().numpy(), 612))
    idx = [0] * b if index is None else index
    bad_rows = [b * M - 1] + [g * M + 2 for g in range(b) if counts[idx[g]] == 0 and M > 2]
    for r in bad_rows:
        i["J"][r, 19, 0, 1] = float("nan")
    inf_row = 1 if b > 1 else None
    if inf_row is not None:
        i["J"][inf_row, 1, 0, 1] = float("inf")
    p64 = lref.pelvis(i["R0"], i["T0"], i["J"], torch.float64)
    xy = _tracks_near(np.nan_to_num(p64), b, M, S, O, T, idx, 613).astype(np.float32)
    nan_set = idx[0]
    if T > 1 and counts[nan_set] > 0:
        xy[nan_set, 0, min(max(frame0 + 5, 0), T - 1), 0] = np.nan                          # one frame of one track: it drops out there
    radius = np.random.default_rng(614).uniform(0.1, 0.3, (S, O)).astype(np.float32)
    count, set_of_row = np.asarray(counts, np.int32), np.repeat(np.asarray(idx), M)
    p32 = lref.pelvis(i["R0"], i["T0"], i["J"], torch.float32)
    assert frame0 + 19 + 18 > T - 1                                                          # the clamp at the track's end, from h = 1 on
    base = None
    for H in (0, 1, 3, 8):
        want = lref.obstacle_clearances(p32, xy, radius, count, set_of_row, frame0, BODY, H, SLACK, torch.float32, bits=True)
        nan = np.zeros((b * M, 18), bool)
        nan[bad_rows, 17 if H == 0 else slice(None)] = True
        assert np.array_equal(np.isnan(want), nan), (case, H)                               # NaN there and only there
        got = _ahead_clear(i, jpb, xy, radius, count, None if index is None else np.asarray(index, np.int32), frame0, BODY, H, SLACK, b, M)
        line = _report(f"obstacle_ahead_clearance {case} H={H}", got, want)
        assert _bits_equal(got, want), line
        if H == 0:
            base = want
        else:
            rest = ~np.isin(np.arange(b * M), bad_rows)
            assert (want[rest] <= base[rest]).all()                                          # a prediction only ever lowers a clearance
            assert inf_row is None or (np.array_equal(want[inf_row], base[inf_row]) and not np.isnan(base[inf_row]).any())
    empty = np.asarray(counts)[set_of_row] == 0
    assert np.isposinf(want[empty & ~nan.all(1)]).all()                                      # nobody there, however far ahead
    assert len(bad_rows) == 1 + int(any(counts[idx[g]] == 0 for g in range(b)) and M > 2)
    if max(counts) > 1:                                                                      # coverage, on the restatement
        live = ~empty & ~nan.any(1)
        assert (base[live] < 0).any() and ((base[live] > 0) & (base[live] < MARGIN)).any() and (want[live] < base[live]).any(), case
    if b > 1:       # a sequence's rows are the same bits in a batch of one: the last sequence alone
        sel = slice((b - 1) * M, b * M)
        one = {"J": i["J"][sel].contiguous(), "R0": i["R0"][sel].contiguous(), "T0": i["T0"][sel].contiguous()}
        assert _bits_equal(_ahead_clear(one, jpb, xy, radius, count, np.asarray(index[-1:], np.int32), frame0, BODY, 8, SLACK, 1, M), want[sel])


def test_ahead_entry_rejects_bad_arguments():
    """Rejected before anything is launched: every pointer may therefore be the same scratch buffer."""
    from egogen_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(16384, device="cuda")
    p = C.c_void_p(buf.data_ptr())

    def call(J=p, jpb=127, R0=p, T0=p, b=1, M=1, xy=p, radius=p, count=p, S=1, O=4, T=3, body=0.3, H=2, slack=0.1, out=p):
        return lib.egx_obstacle_ahead_clearance(J, jpb, R0, T0, b, M, xy, radius, count, None, S, O, T, 0, body, H, slack, out, _lib.current_stream_ptr())
    bad = ({"J": None}, {"R0": None}, {"T0": None}, {"xy": None}, {"radius": None}, {"count": None}, {"out": None}, {"H": 9}, {"H": -1},
           {"slack": -0.01}, {"slack": float("nan")}, {"slack": float("inf")}, {"body": -0.1}, {"body": float("nan")}, {"body": float("inf")},
           {"T": 0}, {"O": 33}, {"O": -1}, {"S": 0}, {"b": 0}, {"M": 0}, {"M": 257}, {"jpb": 0}, {"b": 1 << 24, "M": 256})
    for kw in bad:
        assert call(**kw) == -1, kw
        with pytest.raises(_lib.EgxError):
            _lib.check(call(**kw), "egx_obstacle_ahead_clearance")
    torch.cuda.synchronize()
    assert not buf.any()                                                          # nothing was launched


# ---- H = 0: the table gives the cylinder entries' bits -------------------------------------------------------------------------------
def _sets_for(x, b, M, seed):
    """two tracks per sequence near its rows, a set per sequence -> the descriptor of tests/test_genop_obstacles_gpu.py"""
    _, i, _, _ = _selection_args(x, b, M, 0, 127, CFG_RF, W_TEST, 40.0, 0.1, ())
    p64 = lref.pelvis(i["R0"], i["T0"], i["J"], torch.float64)
    xy = _tracks_near(p64, b, M, b, 5, 30, list(range(b)), seed)
    return _obs(xy, 0.2, count=[5, 2, 4][:b], index=list(range(b)), frame0=3, w=W_OBS, margin=MARGIN, body=BODY)


def test_table_at_lookahead_zero_is_the_cylinder_selection(small_world):
    b, N = 3, 5
    x = _lattice(_rows_inputs(small_world, b, N, 640, True), b, N)
    ob = _sets_for(x, b, N, 641)
    want, i = _select_obs(x, 127, ob)
    table = _ahead_clear(i, 127, ob["xy"].numpy(), ob["radius"].numpy(), ob["count"].numpy(), ob["index"].numpy(), ob["frame0"], BODY, 0, SLACK, b, N)
    got = _select_table(x, 127, table, w=W_OBS, margin=MARGIN)
    assert bool((want["obs_term"] > 0).any()) and bool(want["obs_hit"].bool().any()) and bool((want["obs_term"] == 0).any())
    for k in ("obs_term", "obs_clearance", "obs_hit", "cost", "choice", "colliding", "status", "terms", "goal_dist", "reached"):
        assert _bits_equal(got[k], want[k]), (k, _report(f"table H=0 against select_obstacles {k}", got[k].float().numpy(), want[k].float().numpy()))


def test_table_at_lookahead_zero_is_the_cylinder_beam_selection(small_world):
    b, W, N = 3, 2, 3
    M = W * N
    x = _lattice(_rows_inputs(small_world, b, M, 650, True), b, M)
    ob = _sets_for(x, b, M, 651)
    g = torch.Generator().manual_seed(5)
    acc, ncoll = torch.rand(b, W, generator=g) * 6.0, torch.randint(0, 3, (b, W), generator=g, dtype=torch.int32)
    want, i = _select_obs(x, 127, ob, beam=(W, N), acc=acc, ncoll=ncoll)
    table = _ahead_clear(i, 127, ob["xy"].numpy(), ob["radius"].numpy(), ob["count"].numpy(), ob["index"].numpy(), ob["frame0"], BODY, 0, SLACK, b, M)
    got = _select_table(x, 127, table, beam=(W, N), acc=acc, ncoll=ncoll, w=W_OBS, margin=MARGIN)
    assert bool((want["obs_term"] > 0).any())
    for k in ("obs_term", "obs_clearance", "obs_hit", "cost", "colliding", "terms", "beam_row", "parent", "acc", "ncoll", "path_cost", "status",
              "goal_dist", "reached"):
        assert _bits_equal(got[k], want[k]), (k, _report(f"table H=0 against beam_select_obstacles {k}", got[k].float().numpy(), want[k].float().numpy()))


# ---- the joint entry -----------------------------------------------------------------------------------------------------------------
def _joint_ahead(c, S, H, slack=SLACK, groups=None, w=jg.W_PAIR, margin=jg.MARGIN, body=jg.BODY):
    """egx_primitive_select_joint_ahead on the selection outputs of case c (copies: the case can be launched again) -> outputs on the CPU"""
    from egogen_amd import _lib
    groups = c["groups"] if groups is None else groups
    b, N, i = c["b"], c["N"], c["i"]
    G = len(groups)
    start = torch.tensor(np.cumsum([0] + [len(g) for g in groups]), dtype=torch.int32, device="cuda")
    member = torch.tensor([m for g in groups for m in g] or [0], dtype=torch.int32, device="cuda")
    o = jg._sweep_outputs(c, S, G)
    goal = c["alive"][0][0]
    keep = {k: c["sel"][k].clone() for k in ("cost", "terms", "colliding")}
    _lib.check(_lib.load().egx_primitive_select_joint_ahead(
        _lib.ptr(i["J"]), c["jpb"], _lib.ptr(i["R0"]), _lib.ptr(i["T0"]), _lib.ptr(goal), _lib.ptr(c["sel"]["cost"]), _lib.ptr(c["sel"]["terms"]),
        _lib.ptr(c["sel"]["colliding"]), b, N, _lib.ptr(start), _lib.ptr(member), G, S, w, margin, body, int(H), float(slack), jg.GOAL_THRESH,
        *[_lib.ptr(o[k]) for k in jg.OUTS], _lib.current_stream_ptr()), "egx_primitive_select_joint_ahead")
    torch.cuda.synchronize()
    for k, v in keep.items():
        assert torch.equal(c["sel"][k], v), k                                                # the selection's rows are only read
    return {k: v.cpu() for k, v in o.items()}


def _ahead_case(world, sizes, N, seed, extra=0, interleave=False, tracks=None, weights=W_TEST, with_pene=True):
    """a case of tests/test_genop_joint_gpu.py whose rows walk straight over all of frames 1..19 (the members of a group start within 1.5 m
    of the group's spot, groups 20 m apart), so that a displacement means something"""
    b, groups = jg._membership(sizes, extra, interleave, seed)
    if tracks is None:
        origin = np.zeros((b, 2))
        for gi, members in enumerate(groups):
            origin[members] = [20.0 * (gi + 1), 0.0]
        tracks = _walks(b * N, np.repeat(origin, N, 0), seed + 1)
    tracks = np.asarray(tracks).reshape(b, N, 20, 2)
    c = jg._case(world, sizes, N, seed, extra=extra, interleave=interleave, tracks=tracks[:, :, 2:], weights=weights, with_pene=with_pene)
    assert c["groups"] == groups
    _plant20(c["i"], tracks, frames=[1])             # frames 2..19 stand as the selection read them; frame 1 gives the displacement its start
    return c


def _state(c, H, slack, w=jg.W_PAIR, margin=jg.MARGIN, body=jg.BODY):
    sel = {k: v.cpu() for k, v in c["sel"].items()}
    return {"cost": sel["cost"], "terms": sel["terms"], "colliding": sel["colliding"].bool(), "R0": c["i"]["R0"], "T0": c["i"]["T0"], "J": c["i"]["J"],
            "w": w, "margin": margin, "body_radius": body, "lookahead": H, "lookahead_slack": slack, "_pelvis": {}}


def _check_ahead(name, c, o, S, H, slack, **scalars):
    """every member step, trace and output of one launch against the float32 restatement, bit for bit -> (hits, near misses, rows whose
    look-ahead clearance is below the present one)"""
    b, N, sel = c["b"], c["N"], {k: v.cpu() for k, v in c["sel"].items()}
    common, now = _state(c, H, slack, **scalars), _state(c, 0, slack, **scalars)
    now["_pelvis"] = common["_pelvis"]
    start = {m: int(sel["choice"][m]) for m in range(b)}
    trace = o["choice_trace"].long()
    in_group = sorted(m for g in c["groups"] for m in g)
    hits = near = lower = 0
    for s in range(S):
        for gi, members in enumerate(c["groups"]):
            for k, m in enumerate(members):
                before = lref.state_before(members, start, trace, s, k)
                r = lref.member_step(dict(common, members=members, choice=before), k, torch.float32, bits=True)
                for key, got in (("term", "pair_term"), ("clearance", "pair_clearance"), ("joint_cost", "joint_cost"), ("hit", "pair_hit")):
                    assert _bits_equal(o[got][s, m], r[key]), (name, s, m, got, _report(f"{name} {got}", o[got][s, m].float().numpy(), r[key].float().numpy()))
                assert int(trace[s, m]) == r["choice"], (name, s, m)
                r0 = lref.member_step(dict(now, members=members, choice=before), k, torch.float32, bits=True)
                hits, near = hits + int(r["hit"].sum()), near + int(((r["clearance"] > 0) & (r["clearance"] < common["margin"])).sum())
                lower += int((r["clearance"] < r0["clearance"]).sum())
                if s == S - 1:
                    last_cls = int(r["cls"][r["choice"]])
                    assert int(o["status"][m]) == (last_cls & 1) | (2 if last_cls >= 2 else 0), (name, m)
            prev = [start[m] if s == 0 else int(trace[s - 1, m]) for m in members]
            assert int(o["changed"][s, gi]) == sum(int(trace[s, m]) != p for m, p in zip(members, prev)), (name, s, gi)
    final = trace[S - 1]
    for m in in_group:
        ch = int(final[m])
        assert int(o["choice"][m]) == ch
        if ch == start[m]:
            assert torch.equal(o["goal_dist"][m], sel["goal_dist"][m]) and int(o["reached"][m]) == int(sel["reached"][m]), (name, m)
        else:       # the selection's distance arithmetic on the new row: what it wrote for that row (coordinates below 64 m: an ulp is 3.8e-6)
            assert abs(float(o["goal_dist"][m]) - float(sel["terms"][m, ch, 0])) < 1e-5, (name, m)
            if abs(float(sel["terms"][m, ch, 0]) - jg.GOAL_THRESH) > 1e-5:
                assert int(o["reached"][m]) == int(float(sel["terms"][m, ch, 0]) < jg.GOAL_THRESH), (name, m)
    for members in c["groups"]:
        want = lref.crowd_clearance(dict(common, members=members, choice={m: int(final[m]) for m in members}), torch.float32, bits=True)
        assert _bits_equal(o["crowd_clearance"][members], want), name                        # at h = 0 only: the crowd as written
        assert torch.equal(o["crowd_hit"][members].bool(), want < 0), name
    for m in (m for m in range(b) if m not in in_group):                                      # a sequence of no group: nothing of it is touched
        for k in ("choice", "status", "reached"):
            assert int(o[k][m]) == int(sel[k][m]), (k, m)
        assert int(o["crowd_hit"][m]) == -7 and bool((o["choice_trace"][:, m] == -7).all()) and bool((o["pair_hit"][:, m] == -7).all())
        assert bool(torch.isnan(o["pair_term"][:, m]).all()) and bool(torch.isnan(o["crowd_clearance"][m]))
    return hits, near, lower


# N, S, H: groups of 1, 2, 3 and 32 members (and two sequences of no group) in one launch each
JOINT_CASES = {"N1 S8 H2": (1, 8, 2), "N5 S2 H8": (5, 2, 8), "N33 S1 H0": (33, 1, 0), "N33 S2 H2": (33, 2, 2), "N5 S1 H0": (5, 1, 0)}


@pytest.mark.parametrize("case", list(JOINT_CASES))
def test_select_joint_ahead_kernel(small_world, case):
    N, S, H = JOINT_CASES[case]
    c = _ahead_case(small_world, (1, 2, 3, 32), N, 700 + N + H, extra=2, interleave=True)
    bad = c["groups"][2][1] * N + (N - 1)                                                     # a member of the group of three: its last row
    c["i"]["J"][bad, 19 if H else 7, 0, 0] = float("nan")                                     # NaN at frame 19: a NaN row with a look-ahead
    o = _joint_ahead(c, S, H)
    hits, near, lower = _check_ahead(f"select_joint_ahead {case}", c, o, S, H, SLACK)
    print(f"| select_joint_ahead {case} | row evaluations: hits {hits} | near misses {near} | lowered by the look-ahead {lower} |")
    assert bool(torch.isnan(o["pair_term"][:, bad // N, bad % N]).all()) and not bool(o["pair_hit"][:, bad // N, bad % N].any())
    assert hits > 0 and near > 0 and (lower > 0) == (H > 0)
    if H == 0:      # every output is egx_primitive_select_joint's
        plain = jg._joint(c, S)
        for k in jg.OUTS:
            assert _bits_equal(o[k], plain[k]), (case, k)
    else:           # and the look-ahead is no no-op
        plain = jg._joint(c, S)
        assert not _bits_equal(o["pair_term"], plain["pair_term"])


def test_joint_ahead_group_does_not_depend_on_batch(small_world):
    sizes, N, S, H = (1, 2, 5), 33, 3, 2
    c = _ahead_case(small_world, sizes, N, 777, extra=2, interleave=True)
    full = _joint_ahead(c, S, H)
    for gi, members in enumerate(c["groups"]):
        one = _joint_ahead(c, S, H, groups=[members])
        for k in jg.PER_SEQ:
            assert _bits_equal(one[k][members], full[k][members]), (gi, k)
        for k in jg.TRACES + ("choice_trace",):
            assert _bits_equal(one[k][:, members], full[k][:, members]), (gi, k)
        assert torch.equal(one["changed"][:, 0], full["changed"][:, gi])
    rev = _joint_ahead(c, S, H, groups=c["groups"][::-1])
    grouped = sorted(m for g in c["groups"] for m in g)
    for k in jg.PER_SEQ:
        assert _bits_equal(rev[k][grouped], full[k][grouped]), k
    assert torch.equal(rev["changed"], full["changed"].flip(1))


def test_joint_ahead_entry_rejects_bad_arguments():
    """Rejected before anything is launched: every pointer may therefore be the same scratch buffer."""
    from egogen_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(16384, device="cuda")
    p = C.c_void_p(buf.data_ptr())
    outs = list(jg.OUTS)

    def call(N=1, G=1, S=1, w=1.0, margin=0.5, body=0.3, H=2, slack=0.1, null=None, J=p):
        return lib.egx_primitive_select_joint_ahead(J, 127, p, p, p, p, p, p, 1, N, p, p, G, S, w, margin, body, H, slack, 0.1,
                                                    *[None if k == null else p for k in outs], _lib.current_stream_ptr())
    bad = [{"H": 9}, {"H": -1}, {"slack": -0.01}, {"slack": float("nan")}, {"slack": float("inf")}, {"J": None}, {"N": 0}, {"N": 257}, {"S": 0},
           {"S": 9}, {"G": 0}, {"margin": -0.1}, {"body": -0.1}, {"body": float("nan")}, {"w": float("inf")}] + [{"null": k} for k in outs]
    for kw in bad:
        assert call(**kw) == -1, kw
        with pytest.raises(_lib.EgxError):
            _lib.check(call(**kw), "egx_primitive_select_joint_ahead")
    torch.cuda.synchronize()
    assert not buf.any()                                                                      # nothing was launched


# ---- head on: the feature does something ---------------------------------------------------------------------------------------------
def _line(x0, y0, vx, vy):
    t = np.arange(20)[:, None]
    return np.array([x0, y0]) + t * np.array([vx, vy])


def _head_on():
    """[2,2,20,2]: two people 3.2 m apart walk at each other at 0.05 m a frame (rows 0: 1.3 m apart at the end of this primitive, 0.7 m
    clear of summed radii of 0.6 m - more than the margin of 0.5 m - and through each other in the middle of the next) or veer off at the
    same speed (rows 1: never within 1.4 m of the other's straight line's prediction)"""
    return np.stack([np.stack([_line(-1.6, 0.0, 0.05, 0.0), _line(-1.6, 0.0, 0.03, 0.04)]),
                     np.stack([_line(1.6, 0.0, -0.05, 0.0), _line(1.6, 0.0, -0.03, -0.04)])])


def test_head_on_two_members_one_gives_way(small_world):
    """equal selection cost for all four rows: without a look-ahead nobody has a reason to leave row 0; with two primitives of it the
    member that is visited first veers, and the other, who then has nobody in the way, walks on"""
    c = _ahead_case(small_world, (2,), 2, 11, tracks=_head_on().reshape(4, 20, 2), weights=jg.GOAL_ONLY, with_pene=False)
    c["sel"]["cost"].zero_(), c["sel"]["colliding"].zero_(), c["sel"]["choice"].zero_()      # cost_terms stay: they are only asked to be finite
    scalars = dict(w=1.0, margin=0.5, body=0.3)
    o0, o2 = _joint_ahead(c, 2, 0, 0.1, **scalars), _joint_ahead(c, 2, 2, 0.1, **scalars)
    assert o0["choice"].tolist() == [0, 0] and not o0["pair_term"].any() and float(o0["pair_clearance"].min()) > 0.5
    assert o0["changed"].reshape(-1).tolist() == [0, 0]
    assert o2["choice"].tolist() == [1, 0] and o2["choice_trace"].tolist() == [[1, 0], [1, 0]] and o2["changed"].reshape(-1).tolist() == [1, 0]
    assert float(o2["pair_term"][0, 0, 0]) > 0.1 and not o2["pair_hit"].any() and o2["status"].tolist() == [0, 0]        # it costs, it does not veto
    assert float(o2["pair_clearance"][0, 0, 0]) == float(np.float32(0.1))                     # the overlap at h = 1: max(0, .) + 1 * slack
    assert float(o2["pair_term"][0, 0, 1]) == 0.0 and not o2["crowd_hit"].any() and float(o2["crowd_clearance"].min()) > 0.5
    for H, o in ((0, o0), (2, o2)):
        _check_ahead(f"head on H={H}", c, o, 2, H, 0.1, **scalars)


def test_head_on_recorded_track_through_the_table(small_world):
    """the same with the other person on record: one sequence of two rows (all cost weights 0: equal cost), the recorded person walks
    its straight line for 60 frames; the table of H = 0 leaves the greedy selection at row 0, that of H = 2 moves it to row 1"""
    from egogen_amd import _lib
    b, N = 1, 2
    x = _rows_inputs(small_world, b, N, 660, False)
    lead, i, o, _alive = _selection_args(x, b, N, 0, 127, CFG_RF, ZERO_W, 40.0, 0.1, ())
    _plant20(i, _head_on()[0])
    xy = _line(1.6, 0.0, -0.05, 0.0)[:1] + np.arange(60)[:, None] * np.array([-0.05, 0.0])
    xy, radius, count = xy[None, None].astype(np.float32), np.full((1, 1), 0.3, np.float32), np.array([1], np.int32)
    p32 = lref.pelvis(i["R0"], i["T0"], i["J"], torch.float32)
    picks = {}
    for H in (0, 2):
        table = _ahead_clear(i, 127, xy, radius, count, None, 0, 0.3, H, 0.1, b, N)
        assert _bits_equal(table, lref.obstacle_clearances(p32, xy, radius, count, [0, 0], 0, 0.3, H, 0.1, torch.float32, bits=True))
        d_table = torch.as_tensor(table).cuda().contiguous()
        fi = lambda *s: torch.full(s, -7, dtype=torch.int32, device="cuda")
        ff = lambda *s: torch.full(s, float("nan"), device="cuda")
        out = {"choice": fi(b), "status": fi(b), "reached": fi(b), "goal_dist": ff(b), "obs_term": ff(b, N), "obs_clearance": ff(b, N), "obs_hit": fi(b, N)}
        _lib.check(_lib.load().egx_primitive_select_obstacle_markers(
            *lead, b, N, _lib.ptr(out["choice"]), _lib.ptr(out["status"]), _lib.ptr(out["reached"]), _lib.ptr(out["goal_dist"]), _lib.ptr(o["cost"]),
            _lib.ptr(o["terms"]), _lib.ptr(o["colliding"]), *NULL_FIELD, _lib.ptr(d_table), 1.0, 0.5, _lib.ptr(out["obs_term"]),
            _lib.ptr(out["obs_clearance"]), _lib.ptr(out["obs_hit"]), _lib.current_stream_ptr()), "egx_primitive_select_obstacle_markers")
        torch.cuda.synchronize()
        picks[H] = {k: v.cpu() for k, v in {**out, "cost": o["cost"]}.items()}
    assert picks[0]["choice"].tolist() == [0] and not picks[0]["obs_term"].any() and float(picks[0]["obs_clearance"].min()) > 0.5
    assert float(picks[0]["cost"][0, 0]) == float(picks[0]["cost"][0, 1])                     # equal cost: the lower index
    assert picks[2]["choice"].tolist() == [1] and float(picks[2]["obs_term"][0, 0]) > 0.1 and float(picks[2]["obs_term"][0, 1]) == 0.0
    assert not picks[2]["obs_hit"].any() and picks[2]["status"].tolist() == [0]               # it costs, it does not veto
    assert float(picks[2]["obs_clearance"][0, 0]) == float(np.float32(0.1))


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
class _Spy:
    """counts the calls of the two look-ahead entries of the loaded library, and keeps their arguments, for the length of the block"""
    NAMES = ("egx_obstacle_ahead_clearance", "egx_primitive_select_joint_ahead")

    def __enter__(self):
        from egogen_amd import _lib
        self.lib, self.calls, self.real, self.args = _lib.load(), {k: 0 for k in self.NAMES}, {}, {k: [] for k in self.NAMES}
        for name in self.NAMES:
            self.real[name] = getattr(self.lib, name)

            def counted(*a, _name=name):
                self.calls[_name] += 1
                self.args[_name].append(a)
                return self.real[_name](*a)
            setattr(self.lib, name, counted)
        return self

    def __exit__(self, *exc):
        for name, fn in self.real.items():
            setattr(self.lib, name, fn)


def _same(a, b):
    if not torch.is_tensor(a):
        return a == b
    return a.shape == b.shape and bool(((a == b) | (torch.isnan(a.float()) & torch.isnan(b.float()))).all())


NEAR = torch.tensor([[0.4, 0.0, 0.0], [3.4, 0.0, 0.0], [-2.6, 0.0, 0.0]])


@pytest.mark.parametrize("W,N", [(1, 4), (2, 2)])
def test_generate_sequence_to_goal_with_obstacles_and_lookahead(search_world, W, N, tmp_path):
    from egogen_amd import MovingObstacles
    w = search_world
    op, K, b, M, H, slack = w["op"], 3, w["b"], W * N, 2, 0.1
    loop = "_search_loop" if W == 1 else "_beam_loop"
    people = MovingObstacles.from_sequences(_e2e(w, 1, 4, K))
    # lookahead = 0 is the call without the argument, and launches neither new entry
    with _Spy() as spy:
        base = _e2e(w, W, N, K, obstacles=people, T0=NEAR)
        zero = _e2e(w, W, N, K, obstacles=people, T0=NEAR, lookahead=0, lookahead_slack=0.3)
    assert spy.calls == {k: 0 for k in spy.NAMES}
    for k in E2E_FIELDS + base.OBSTACLE_FIELDS:
        assert _same(getattr(zero, k), getattr(base, k)), k
    assert base.search["lookahead"] == 0 and zero.search["lookahead"] == 0 and zero.search["lookahead_slack"] == 0.3
    assert bool(base.obstacle_term.gt(0).any())
    lowered = 0
    for Kp in range(1, K + 1):                      # a run of Kp primitives is the prefix of the longer one: its last primitive from the loop's state
        with _Spy() as spy, patched_loop(op, loop, no_host_wait=True) as seen:
            res = _e2e(w, W, N, Kp, obstacles=people, T0=NEAR, lookahead=H, lookahead_slack=slack)
        assert seen.calls == [(Kp, b, N) if W == 1 else (Kp, b, W, N)]
        assert spy.calls == {"egx_obstacle_ahead_clearance": Kp, "egx_primitive_select_joint_ahead": 0}
        for k, a in enumerate(spy.args["egx_obstacle_ahead_clearance"]):                    # b, M, frame0, body_radius, H, slack as the host was asked
            assert (a[4], a[5], a[13], a[15]) == (b, M, 18 * k, H) and abs(a[14] - 0.3) < 1e-7 and abs(a[16] - slack) < 1e-7, (k, a[4:6], a[13:17])
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
        p32 = lref.pelvis(R0, T0, s["lbs_out"]["joints"].reshape(b * M, 20, 127, 3), torch.float32)
        at = (p32, people.xy, people.radius, people.count, np.zeros(b * M, np.int64), 18 * (Kp - 1), 0.3)
        c32 = lref.obstacle_clearances(*at, H, slack, torch.float32, bits=True)
        assert _bits_equal(s["frame_clearance"], c32), _report(f"e2e lookahead W={W} k={Kp - 1} table", s["frame_clearance"].cpu().numpy(), c32)
        lowered += int((c32 < lref.obstacle_clearances(*at, 0, slack, torch.float32, bits=True)).sum())
        t = kref.terms_of_clearance(c32, 0.5)
        for k, want in (("clearance", t["clearance"]), ("obstacle_term", t["term"]), ("obstacle_hit", t["hit"])):
            assert _bits_equal(getattr(res, k)[Kp - 1].reshape(-1), want), (Kp, k)
        hit = res.obstacle_hit[Kp - 1].cpu().bool()
        assert torch.equal(res.colliding[Kp - 1].cpu().bool(), hit)                          # no scene: the hit is the collision
        ch = res.choice[Kp - 1].cpu().long()
        assert torch.equal((res.status[Kp - 1].cpu() & 1).bool(), hit.gather(1, ch[:, None])[:, 0])
    print(f"| e2e lookahead W={W} | frame clearances a prediction lowered | {lowered} |")
    assert lowered > 0                                                                       # a prediction was the least somewhere: H reached the rows
    assert res.search["lookahead"] == H and res.search["lookahead_slack"] == slack and res.search["obstacle_model"] == "cylinder"
    # the search keys survive save, and the files are obstacles for the next person
    res_np = _e2e(w, W, N, K, obstacles=people, T0=NEAR, lookahead=H, lookahead_slack=slack, to_numpy=True)
    paths = [res_np.save(str(tmp_path), i, man_id=f"p_{i}") for i in range(b)]
    assert res_np.search["lookahead"] == H and res_np.search["lookahead_slack"] == slack
    for k in res_np.OBSTACLE_FIELDS:
        assert res_np.search[k] is getattr(res_np, k) and _bits_equal(getattr(res_np, k), getattr(res, k)), k
    assert np.array_equal(MovingObstacles.from_rollout_files(paths).xy, MovingObstacles.from_sequences(res_np).xy)


def test_generate_sequence_to_goal_with_groups_and_lookahead(search_world, tmp_path):
    w = search_world
    op, K, b, N, S, H, slack = w["op"], 2, 4, 4, 2, 2, 0.1
    members = [[0, 1], [2, 3]]
    with _Spy() as spy:
        base = jg._e2e(w, N, K, groups=[0, 0, 1, 1])
        zero = jg._e2e(w, N, K, groups=[0, 0, 1, 1], lookahead=0)
    assert spy.calls == {k: 0 for k in spy.NAMES}
    for k in jg.E2E_SAME + base.JOINT_FIELDS:
        assert _same(torch.as_tensor(getattr(zero, k)), torch.as_tensor(getattr(base, k))), k
    assert base.search["lookahead"] == 0 and base.search["lookahead_slack"] == 0.1
    for Kp in range(1, K + 1):
        with _Spy() as spy, patched_loop(op, "_search_loop", no_host_wait=True) as seen:
            res = jg._e2e(w, N, Kp, groups=[0, 0, 1, 1], lookahead=H, lookahead_slack=slack)
        assert seen.calls == [(Kp, b, N)] and spy.calls == {"egx_obstacle_ahead_clearance": 0, "egx_primitive_select_joint_ahead": Kp}
        for a in spy.args["egx_primitive_select_joint_ahead"]:                               # S, weight, margin, body_radius, H, slack as the host was asked
            assert (a[8], a[9], a[13], a[17]) == (b, N, S, H) and abs(a[16] - 0.3) < 1e-7 and abs(a[18] - slack) < 1e-7, a[8:19]
        if Kp > 1:
            for k in ("choice", "individual_choice", "choice_trace", "joint_cost", "crowd_clearance", "cost"):
                assert _same(getattr(res, k)[:Kp - 1], getattr(prev, k)), k
        prev = res
        assert res.pair_term.shape == (Kp, S, b, N) and torch.equal(res.choice, res.choice_trace[:, -1])
        k = Kp - 1
        st = {"cost": res.cost[k].cpu(), "terms": res.cost_terms[k].cpu(), "colliding": res.colliding[k].cpu().bool(),
              "R0": res.rotmat[k].repeat_interleave(N, 0), "T0": res.transl[k].repeat_interleave(N, 0),
              "J": seen.s["lbs_out"]["joints"].reshape(b * N, 20, 127, 3), "w": 1.0, "margin": 0.5, "body_radius": 0.3, "lookahead": H,
              "lookahead_slack": slack, "_pelvis": {}}
        start, trace = {m: int(res.individual_choice[k, m]) for m in range(b)}, res.choice_trace[k].cpu().long()
        for s in range(S):
            for grp in members:
                for j, m in enumerate(grp):
                    r = lref.member_step(dict(st, members=grp, choice=lref.state_before(grp, start, trace, s, j)), j, torch.float32, bits=True)
                    for key, got in (("term", "pair_term"), ("clearance", "pair_clearance"), ("joint_cost", "joint_cost"), ("hit", "pair_hit")):
                        assert _bits_equal(getattr(res, got)[k, s, m], r[key]), (Kp, s, m, got)
                    assert int(trace[s, m]) == r["choice"], (Kp, s, m)
        for grp in members:
            want = lref.crowd_clearance(dict(st, members=grp, choice={m: int(trace[-1, m]) for m in grp}), torch.float32, bits=True)
            assert _bits_equal(res.crowd_clearance[k, grp], want) and torch.equal(res.crowd_hit[k, grp].cpu().bool(), want < 0)
        ch = res.choice[k].long()
        assert torch.equal(res.params[k], seen.s["pp"].reshape(b, N, 20, 93)[torch.arange(b), ch])      # the hand-off continued from the joint choice
    assert float(res.pair_term.max()) > 0.0 and res.search["lookahead"] == H and res.search["lookahead_slack"] == slack
    assert res.search["pair_model"] == "cylinder"
    res_np = jg._e2e(w, N, K, groups=[0, 0, 1, 1], lookahead=H, lookahead_slack=slack, to_numpy=True)
    paths = [res_np.save(str(tmp_path), i, man_id=f"p_{i}") for i in range(b)]
    assert [os.path.basename(p) for p in paths] == [f"motion_p_{i}.pkl" for i in range(b)]
    assert res_np.search["lookahead"] == H and res_np.search["lookahead_slack"] == slack
    for k in res_np.JOINT_FIELDS:
        assert res_np.search[k] is getattr(res_np, k) and _bits_equal(np.asarray(getattr(res_np, k)), torch.as_tensor(getattr(res, k))), k


# ---- the driver ----------------------------------------------------------------------------------------------------------------------
def _driver(tmp_path, *flags):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, os.path.join(ROOT, "exp_GAMMAPrimitive", "gen_motion.py"), "--n-primitives", "2", "--seed", "3", "--num-verts", str(V_SMALL),
           "--n-gens", "2", "--n-candidates", "4", *flags]
    return subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)


def test_gen_motion_driver_people_lookahead(tmp_path):
    out = tmp_path / "crowd"
    r = _driver(tmp_path, "--people", "0,0,0:0.3,3,0.9;0.8,0,0:0.5,3,0.9;0.4,3,180:0.4,0,0.9", "--lookahead", "2", "--out", str(out))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    files = sorted(f for f in os.listdir(out) if f.startswith("motion_") and f.endswith(".pkl"))
    assert files == sorted(f"motion_3_{v}_p{p}.pkl" for v in range(2) for p in range(3)), files
    lines = re.findall(r"variant (\d+): minimum crowd clearance (-?[0-9.]+) m, crowd hits (\d+)", r.stdout)
    assert [int(v[0]) for v in lines] == [0, 1] and all(np.isfinite(float(v[1])) for v in lines), r.stdout[-1500:]


def test_gen_motion_driver_avoid_lookahead(tmp_path):
    first, second = tmp_path / "first", tmp_path / "second"
    r = _driver(tmp_path, "--goal", "0.5,2.0,0.9", "--out", str(first))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    files = sorted(str(first / f) for f in os.listdir(first) if f.startswith("motion_") and f.endswith(".pkl"))
    r = _driver(tmp_path, "--goal", "0.5,2.0,0.9", "--out", str(second), "--avoid", ",".join(files), "--start", "1.5,0.0,30", "--lookahead", "2",
                "--lookahead-slack", "0.05")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert len([f for f in os.listdir(second) if f.startswith("motion_") and f.endswith(".pkl")]) == 2 and "avoiding 2 people over" in r.stdout
    lines = re.findall(r"variant (\d+): minimum clearance (-?[0-9.]+|inf) m, chosen hits (\d+)", r.stdout)
    assert [int(v[0]) for v in lines] == [0, 1] and all(np.isfinite(float(v[1])) for v in lines), r.stdout[-1500:]
