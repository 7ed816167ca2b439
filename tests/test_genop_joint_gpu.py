"""The joint step of the greedy primitive search on the device: entry egx_primitive_select_joint (csrc/genop_joint.hip),
`generate_sequence_to_goal(groups=)` and the driver's `--people`, against the float64 / float32 restatement
tests/genop_joint_ref.py.

Inputs.  Rows of the walker pool (`_rows_inputs`) whose pelvis (joint 0) at the predicted frames 2..19 is overwritten so that the
WORLD tracks are hand-made: the local value is R0^T (world - T0) in float64, rounded once.  Per group a base walk, plus a constant
offset per (member, candidate) on a lattice of pitch 0.4 m, plus a wiggle of at most 0.02 m per row and frame.  With body_radius
0.15 (summed radii 0.3) and margin 0.6 every distance between two candidates of different members of a group is within 0.04 m of
a lattice distance (0, 0.4, 0.566, 0.8, ...), so every float64 frame clearance lies outside (-0.05, +0.05) m: asserted over ALL
candidate pairs, with hits and near misses both present.  The real selection entry (plain, with a field, with obstacles) runs
first; its cost, cost_terms, colliding and choice feed the joint entry.

Yardsticks.  Every member step is checked on its own from the state the device's own `choice_trace` gives, so a near-tie cannot
cascade.  pair_hit and the row classes are exact.  pair_term, pair_clearance and joint_cost are held with `held()`: the device's
error against float64 within R = 3 times the float32 restatement's, pooled over at least MIN_GROUP evaluated rows.  The device's
choice equals the order (class, joint_cost, n) on the device's own values exactly, and the float64 choice on the steps whose
float64 winner is ahead of the runner-up of its class by more than 6 x the largest |joint_cost32 - joint_cost64| of the step's
rows; the other steps are at most UNDECIDABLE_CAP of a case's."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import genop_joint_ref as jref
from tests import genop_obstacles_ref as oref
from tests import genop_search_ref as sref
from tests.genop_gpu_helpers import (CFG_RF, MIN_GROUP, ROOT, UNDECIDABLE_CAP, V_SMALL, W_TEST, _feet, _rows_inputs, _selection_args,  # noqa: F401
                                     emit, held, patched_loop, search_world, small_world)

pytestmark = pytest.mark.gpu

GOAL_ONLY = {"goal": 1.0, "skate": 0.0, "floor": 0.0, "pene": 0.0, "face": 0.0}
PITCH, WIGGLE, BODY, MARGIN, W_PAIR = 0.4, 0.02, 0.15, 0.6, 1.3
HIT_MARGIN = 0.05
GOAL_THRESH = 0.1
NULL_FIELD = (None, None, 0.0, 0, 0, 0, None)
TRACES = ("pair_term", "pair_clearance", "joint_cost", "pair_hit")
PER_SEQ = ("choice", "status", "reached", "goal_dist", "crowd_clearance", "crowd_hit")


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def _membership(sizes, extra, interleave, seed):
    """sum(sizes) + extra sequences -> (b, groups: the member lists in ascending order); interleave: the sequences of the groups
    (and the `extra` ones of no group) are dealt in a random order"""
    b = sum(sizes) + extra
    order = torch.randperm(b, generator=torch.Generator().manual_seed(seed)).tolist() if interleave else list(range(b))
    groups, at = [], 0
    for p in sizes:
        groups.append(sorted(order[at:at + p]))
        at += p
    return b, groups


def _lattice_tracks(groups, b, N, seed):
    """world xy [b,N,18,2] float64 of the hand-made tracks (NaN for a sequence of no group: its rows stay as they are)"""
    g = np.random.default_rng(seed)
    xy = np.full((b, N, 18, 2), np.nan)
    t = np.arange(18)[:, None]
    for members in groups:
        P = len(members)
        side = min(12, max(2, int(np.ceil(np.sqrt(1.5 * P * N)))))      # nodes per side: hits and near misses at every size
        ang = g.uniform(0, 2 * np.pi)
        base = g.uniform(-2, 2, 2) + t * 0.02 * np.array([np.cos(ang), np.sin(ang)])          # [18,2]
        for m in members:
            for n in range(N):
                node = g.integers(0, side, 2) * PITCH
                a, u = g.uniform(0, 2 * np.pi), g.uniform(0, 1)
                wig = WIGGLE * u * np.concatenate([np.cos(a + 0.3 * t), np.sin(a + 0.3 * t)], 1)
                xy[m, n] = base + node + wig
    return xy


def _two_people_tracks():
    """the hand case of tests/test_genop_joint_cpu.py: two people 2 m apart walk at each other ("straight", rows 0) or sidestep 0.6 m
    (rows 1) -> world xy [2,2,18,2], goals [2,3] on the straight lines"""
    t = np.arange(18)[:, None]
    line = lambda x0, y0, dx: np.array([x0, y0]) + t * np.array([dx, 0.0])
    xy = np.stack([np.stack([line(-1.0, 0.0, 0.1), line(-1.0, 0.6, 0.1)]), np.stack([line(1.0, 0.0, -0.1), line(1.0, -0.6, -0.1)])])
    return xy, torch.tensor([[2.0, 0.0, 0.9], [-2.0, 0.0, 0.9]])


def _plant(i, xy):
    """joint 0 of frames 2..19 of the launched joints i["J"] rewritten so that the world xy of row (m, n) is xy[m, n] (where not
    NaN); z stays: local = R0^T (world - T0) in float64, rounded once"""
    n = i["J"].shape[0]
    R0, T0 = i["R0"].double().cpu(), i["T0"].double().cpu()
    j = i["J"][:, 2:, 0, :].double().cpu()                                                   # [n,18,3]
    world = torch.einsum("bij,btj->bti", R0, j) + T0[:, None]
    new = torch.as_tensor(xy).reshape(n, 18, 2)
    keep = torch.isnan(new).any(-1).any(-1)
    world[..., :2] = torch.where(keep[:, None, None], world[..., :2], new)
    local = torch.einsum("bji,btj->bti", R0, world - T0[:, None])
    i["J"][:, 2:, 0, :] = local.float().to(i["J"].device)


def _pair_census(i, groups, N):
    """float64 frame clearances between all candidates of different members of every group -> (all outside the band, hits, near
    misses)"""
    b = i["J"].shape[0] // N
    p = oref.world_pelvis(i["R0"], i["T0"], i["J"], torch.float64)[:, 2:].reshape(b, N, 18, 2)
    ok, hits, near = True, 0, 0
    for members in groups:
        q = p[members]                                                                       # [P,N,18,2]
        P = len(members)
        d = q[:, :, None, None] - q[None, None]                                              # [P,N,P,N,18,2]
        c = torch.sqrt((d * d).sum(-1)) - 2 * BODY
        other = ~torch.eye(P, dtype=torch.bool)[:, None, :, None, None].expand_as(c)
        c = c[other]
        ok = ok and bool(((c <= -HIT_MARGIN) | (c >= HIT_MARGIN)).all())
        hits, near = hits + int((c < 0).sum()), near + int(((c > 0) & (c < MARGIN)).sum())
    return ok, hits, near


def _case(world, sizes, N, seed, jpb=127, extra=0, interleave=False, mode="plain", tracks=None, weights=W_TEST, with_pene=True, goal=None):
    """the rows of a case with their planted tracks, the selection launched on them -> dict"""
    from egogen_amd import _lib
    b, groups = _membership(sizes, extra, interleave, seed)
    fld = None
    if mode == "field":
        from tests.test_geodesic_gpu import _room_rows
        x, fld = _room_rows(world, b, N, seed)
    else:
        x = _rows_inputs(world, b, N, seed, with_pene)
    if goal is not None:
        x["goal"] = goal
    lead, i, o, alive = _selection_args(x, b, N, 0, jpb, CFG_RF, weights, 40.0, GOAL_THRESH, ())
    _plant(i, _lattice_tracks(groups, b, N, seed) if tracks is None else tracks)
    fi = lambda *s: torch.full(s, -7, dtype=torch.int32, device="cuda")
    ff = lambda *s: torch.full(s, float("nan"), device="cuda")
    o = {"choice": fi(b), "status": fi(b), "reached": fi(b), "goal_dist": ff(b), **o}
    outs = (_lib.ptr(o["choice"]), _lib.ptr(o["status"]), _lib.ptr(o["reached"]), _lib.ptr(o["goal_dist"]), _lib.ptr(o["cost"]), _lib.ptr(o["terms"]),
            _lib.ptr(o["colliding"]))
    st = _lib.current_stream_ptr()
    lib = _lib.load()
    if mode == "plain":
        _lib.check(lib.egx_primitive_select(*lead, b, N, *outs, st), "egx_primitive_select")
    elif mode == "field":
        idx = torch.arange(b, dtype=torch.int32, device="cuda")
        fa = (_lib.ptr(fld.dist), _lib.ptr(fld.origin), float(np.float32(fld.cell)), fld.dist.shape[1], fld.dist.shape[2], len(fld), _lib.ptr(idx))
        _lib.check(lib.egx_primitive_select_field(*lead, b, N, *outs, *fa, st), "egx_primitive_select_field")
    else:       # two standing people next to the first group's walk, one set for all
        p0 = oref.world_pelvis(i["R0"], i["T0"], i["J"], torch.float64)[groups[0][0] * N, 10]
        oxy = torch.stack([p0 + torch.tensor([0.5, 0.1]), p0 + torch.tensor([-0.3, 0.7])])[None, :, None, :].float().cuda().contiguous()   # [1,2,1,2]
        orad, ocnt = torch.full((1, 2), 0.2, device="cuda"), torch.tensor([2], dtype=torch.int32, device="cuda")
        ot, oc, oh = ff(b, N), ff(b, N), fi(b, N)
        _lib.check(lib.egx_primitive_select_obstacles(*lead, b, N, *outs, *NULL_FIELD, _lib.ptr(oxy), _lib.ptr(orad), _lib.ptr(ocnt), None, 1, 2, 1,
                                                      0, 1.7, 0.6, 0.1, _lib.ptr(ot), _lib.ptr(oc), _lib.ptr(oh), st), "egx_primitive_select_obstacles")
        torch.cuda.synchronize()
        assert float(ot.max()) > 0.05                                                        # the obstacles are felt
    torch.cuda.synchronize()
    return {"b": b, "N": N, "jpb": jpb, "groups": groups, "i": i, "sel": o, "alive": (alive, fld, x), "weights": weights}


OUTS = PER_SEQ[:4] + TRACES + ("choice_trace", "changed", "crowd_clearance", "crowd_hit")      # in the order of both sweep entries


def _sweep_outputs(c, S, G):
    """the twelve outputs of either sweep entry: the selection's four as copies (the case can be launched again), the rest NaN / -7"""
    b, N = c["b"], c["N"]
    fi = lambda *s: torch.full(s, -7, dtype=torch.int32, device="cuda")
    ff = lambda *s: torch.full(s, float("nan"), device="cuda")
    o = {k: c["sel"][k].clone() for k in ("choice", "status", "reached", "goal_dist")}
    o.update({"pair_term": ff(S, b, N), "pair_clearance": ff(S, b, N), "joint_cost": ff(S, b, N), "pair_hit": fi(S, b, N), "choice_trace": fi(S, b),
              "changed": fi(S, G), "crowd_clearance": ff(b), "crowd_hit": fi(b)})
    return o


def _joint(c, S, groups=None, w=W_PAIR, margin=MARGIN, body=BODY):
    """egx_primitive_select_joint on the selection outputs of case c (copies: the case can be launched again) -> outputs on the CPU"""
    from egogen_amd import _lib
    groups = c["groups"] if groups is None else groups
    b, N, i = c["b"], c["N"], c["i"]
    G = len(groups)
    start = torch.tensor(np.cumsum([0] + [len(g) for g in groups]), dtype=torch.int32, device="cuda")
    member = torch.tensor([m for g in groups for m in g] or [0], dtype=torch.int32, device="cuda")
    o = _sweep_outputs(c, S, G)
    goal = c["alive"][0][0]
    keep = {k: c["sel"][k].clone() for k in ("cost", "terms", "colliding")}
    _lib.check(_lib.load().egx_primitive_select_joint(
        _lib.ptr(i["J"]), c["jpb"], _lib.ptr(i["R0"]), _lib.ptr(i["T0"]), _lib.ptr(goal), _lib.ptr(c["sel"]["cost"]), _lib.ptr(c["sel"]["terms"]),
        _lib.ptr(c["sel"]["colliding"]), b, N, _lib.ptr(start), _lib.ptr(member), G, S, w, margin, body, GOAL_THRESH, *[_lib.ptr(o[k]) for k in OUTS],
        _lib.current_stream_ptr()), "egx_primitive_select_joint")
    torch.cuda.synchronize()
    for k, v in keep.items():
        assert torch.equal(c["sel"][k], v), k                                                # the selection's rows are only read
    return {k: v.cpu() for k, v in o.items()}


# ---- the checks of one launch ----------------------------------------------------------------------------------------------------
def _cylinder_state(c, w=W_PAIR, margin=MARGIN, body=BODY):
    """what a state of tests/genop_joint_ref.py carries beyond the common keys, the same for every group (the tracks are cached)"""
    i = c["i"]
    state = {"R0": i["R0"], "T0": i["T0"], "J": i["J"], "w": w, "margin": margin, "body_radius": body, "_tracks": {}}
    return lambda gi: state


def _device_classes(c, o, s):
    """[b,N] the row classes from the device's own values of sweep s"""
    sel = c["sel"]
    finite = torch.isfinite(sel["cost"].cpu()) & torch.isfinite(sel["terms"].cpu()).all(-1) & torch.isfinite(o["pair_term"][s]) & \
        torch.isfinite(o["joint_cost"][s])
    return (~finite).long() * 2 + (sel["colliding"].cpu().bool() | o["pair_hit"][s].bool()).long()


def _check_launch(name, c, o, S, pool, ref, model_state):
    """every member step and the whole launch of case c with outputs o of either sweep entry; the held() groups are appended to
    `pool`.  ref: the pair model's restatement (tests/genop_joint_ref.py, tests/genop_joint_markers_ref.py); model_state(gi): what a
    state of group gi carries for it beyond the common keys (cost, terms, colliding, members, choice)"""
    b, N, sel = c["b"], c["N"], {k: v.cpu() for k, v in c["sel"].items()}
    common = {"cost": sel["cost"], "terms": sel["terms"], "colliding": sel["colliding"].bool()}
    start = {m: int(sel["choice"][m]) for m in range(b)}
    trace = o["choice_trace"].long()
    in_group = sorted(m for g in c["groups"] for m in g)
    out_group = [m for m in range(b) if m not in in_group]
    assert int(trace[:, in_group].min()) >= 0 and int(trace[:, in_group].max()) < N
    for s in range(S):
        cls_dev = _device_classes(c, o, s)
        for gi, members in enumerate(c["groups"]):
            for k, m in enumerate(members):
                st = dict(common, **model_state(gi), members=members, choice=ref.state_before(members, start, trace, s, k))
                r64, r32 = ref.member_step(st, k, torch.float64), ref.member_step(st, k, torch.float32)
                assert torch.equal(o["pair_hit"][s, m].bool(), r64["hit"]) and torch.equal(r32["hit"], r64["hit"]), (name, s, m)
                assert torch.equal(cls_dev[m], r64["cls"]) and torch.equal(r32["cls"], r64["cls"]), (name, s, m)
                key = torch.where(cls_dev[m] < 2, o["joint_cost"][s, m], torch.zeros(N))
                assert int(trace[s, m]) == ref.first_by_key(cls_dev[m], key), (name, s, m)   # the order on the device's own values
                wn = r64["choice"]
                same = [n for n in range(N) if n != wn and int(r64["cls"][n]) == int(r64["cls"][wn])]
                ok = True
                if same and int(r64["cls"][wn]) < 2:
                    gap = min(float(r64["joint_cost"][n]) for n in same) - float(r64["joint_cost"][wn])
                    ok = gap > 6.0 * float((r32["joint_cost"].double() - r64["joint_cost"]).abs().max())
                if ok:
                    assert r32["choice"] == wn and int(trace[s, m]) == wn, (name, s, m, int(trace[s, m]), wn)
                pool["ok"].append(ok)
                pool["got"].append(torch.stack([o["pair_term"][s, m], o["pair_clearance"][s, m], o["joint_cost"][s, m]]))
                pool["r64"].append(torch.stack([r64["term"], r64["clearance"], r64["joint_cost"]]))
                pool["r32"].append(torch.stack([r32["term"], r32["clearance"], r32["joint_cost"]]))
            prev = [start[m] if s == 0 else int(trace[s - 1, m]) for m in members]
            assert int(o["changed"][s, gi]) == sum(int(trace[s, m]) != p for m, p in zip(members, prev)), (name, s, gi)
    # the whole launch
    final = trace[S - 1]
    cls_last = _device_classes(c, o, S - 1)
    r = {dt: sref.score(c["i"]["Y_gen"], c["i"]["X"], c["i"]["J"], c["i"]["mp"], c["i"]["R0"], c["i"]["T0"], c["i"]["pene"], c["i"]["goal_rows"], _feet(),
                        c["weights"], 40.0, CFG_RF, dt)["dist"].reshape(b, N) for dt in (torch.float64, torch.float32)}
    e32 = float((r[torch.float32].double() - r[torch.float64]).abs().max())                 # the yardstick of cost_terms[..., 0], all rows of the case
    for m in in_group:
        ch = int(final[m])
        assert int(o["choice"][m]) == ch
        cl = int(cls_last[m, ch])
        assert int(o["status"][m]) == (cl & 1) | (2 if cl >= 2 else 0), (name, m)
        if ch == start[m]:
            assert torch.equal(o["goal_dist"][m], sel["goal_dist"][m]) and int(o["reached"][m]) == int(sel["reached"][m]), (name, m)
        else:
            d64 = float(r[torch.float64][m, ch])
            err = abs(float(o["goal_dist"][m]) - d64)
            pool["dist"].append((err, e32))
            assert err <= 3.0 * e32, (name, m, err, e32)
            if abs(d64 - GOAL_THRESH) > 3.0 * e32:
                assert int(o["reached"][m]) == int(d64 < GOAL_THRESH), (name, m)
    for gi, members in enumerate(c["groups"]):
        st = dict(common, **model_state(gi), members=members, choice={m: int(final[m]) for m in members})
        c64, c32 = ref.crowd_clearance(st, torch.float64), ref.crowd_clearance(st, torch.float32)
        fin = ~torch.isnan(c64)                                                                 # a NaN truth (a bad row) is held exactly
        assert torch.equal(o["crowd_hit"][members].bool(), c64 < 0) and torch.equal(c32 < 0, c64 < 0), (name, gi)
        assert torch.equal(torch.isnan(o["crowd_clearance"][members]), ~fin), (name, gi)
        pool["crowd"].append((o["crowd_clearance"][members][fin], c64[fin], c32[fin]))
    for m in out_group:                                                                       # a sequence of no group: nothing of it is touched
        for k in ("choice", "status", "reached"):
            assert int(o[k][m]) == int(sel[k][m]), (k, m)
        assert torch.equal(o["goal_dist"][m], sel["goal_dist"][m])
        assert int(o["crowd_hit"][m]) == -7 and bool(torch.isnan(o["crowd_clearance"][m])) and bool((o["choice_trace"][:, m] == -7).all())
        assert bool((o["pair_hit"][:, m] == -7).all())
        for k in TRACES[:3]:
            assert bool(torch.isnan(o[k][:, m]).all()), (k, m)


def _held_finite(name, what, got, t64, t32):
    """held() where the truth is finite; where it is not (+inf: nobody else in the group) the device holds the same value"""
    fin = torch.isfinite(t64)
    assert torch.equal(got[~fin].double(), t64[~fin]) and torch.equal(t32[~fin].double(), t64[~fin]), (name, what)
    if bool(fin.any()):
        held(name, what, got[fin], t64[fin], t32[fin])


def _close_pool(name, pool, need_term):
    """the pooled yardsticks of a case; a NaN truth (a bad row of the marker model) is held exactly"""
    got, r64, r32 = (torch.cat(pool[k], 1) for k in ("got", "r64", "r32"))
    assert got.shape[1] >= MIN_GROUP or not need_term, (name, got.shape)
    if need_term:
        assert float(r64[0][torch.isfinite(r64[0])].max()) > 0.1, name                       # the term is exercised, not only the veto
    for j, what in enumerate(("pair_term", "pair_clearance", "joint_cost")):
        nan = torch.isnan(r64[j])
        assert torch.equal(torch.isnan(got[j]), nan) and torch.equal(torch.isnan(r32[j]), nan), (name, what)
        _held_finite(name, what, got[j][~nan], r64[j][~nan], r32[j][~nan])
    if pool["crowd"]:
        _held_finite(name, "crowd_clearance", *(torch.cat([v[j] for v in pool["crowd"]]) for j in range(3)))
    ok = torch.tensor(pool["ok"])
    share = 1.0 - float(ok.float().mean())
    emit(f"| {name} | undecidable member steps | {int((~ok).sum())} of {ok.numel()} | {share:.3f} | changed goal_dist {len(pool['dist'])} |")
    assert share <= UNDECIDABLE_CAP, (name, share)


def _new_pool():
    return {"ok": [], "got": [], "r64": [], "r32": [], "crowd": [], "dist": []}


# sizes, N, S, jpb, extra, interleave, mode
KERNEL_CASES = {
    "one": ((1,), 1, 1, 127, 0, False, "plain"),
    "P3 N5": ((3,), 5, 1, 55, 0, False, "plain"),
    "full table": ((32,), 8, 2, 127, 0, False, "plain"),
    "mixed": ((1, 2, 5), 70, 3, 127, 2, True, "plain"),
    "N256": ((2,), 256, 1, 127, 0, False, "plain"),
    "65 pairs": ((2,) * 65, 3, 2, 127, 0, False, "plain"),
    "field": ((3, 2), 5, 2, 127, 0, True, "field"),
    "obstacles": ((3, 2), 5, 2, 127, 0, True, "obstacles"),
}


@pytest.mark.parametrize("case", list(KERNEL_CASES))
def test_select_joint_kernel(small_world, case):
    sizes, N, S, jpb, extra, interleave, mode = KERNEL_CASES[case]
    name = f"select_joint {case}"
    pairs = max(sizes) > 1
    pool, hits, near, draw = _new_pool(), 0, 0, 0
    while draw == 0 or (pairs and (sum(t.shape[1] for t in pool["got"]) < MIN_GROUP or not (hits and near))):
        assert draw < 12, (name, hits, near)
        c = _case(small_world, sizes, N, 40 + 1000 * draw + N + len(sizes), jpb, extra, interleave, mode)
        ok, h, nm = _pair_census(c["i"], c["groups"], N)
        assert ok, (name, draw)
        hits, near, draw = hits + h, near + nm, draw + 1
        o = _joint(c, S)
        _check_launch(name, c, o, S, pool, jref, _cylinder_state(c))
    emit(f"| {name} | candidate pairs x frames: hits / near misses | {hits} / {near} | draws {draw} | |")
    assert not pairs or (hits > 0 and near > 0)
    _close_pool(name, pool, pairs)


def test_two_members_one_gives_way(small_world):
    """the hand case of tests/test_genop_joint_cpu.py on the device: the straights overlap, member 0 sidesteps, member 1 stays"""
    xy, goal = _two_people_tracks()
    c = _case(small_world, (2,), 2, 3, tracks=xy, weights=GOAL_ONLY, with_pene=False, goal=goal)
    sel = {k: v.cpu() for k, v in c["sel"].items()}
    assert sel["choice"].tolist() == [0, 0] and not sel["colliding"].any()
    assert bool((sel["cost"][:, 1] - sel["cost"][:, 0] > 0.1).all())                         # the sidestep is dearer by about 0.13 m of goal distance
    o = _joint(c, 2, w=1.0)
    assert o["choice_trace"].tolist() == [[1, 0], [1, 0]] and o["changed"].reshape(-1).tolist() == [1, 0]
    assert o["choice"].tolist() == [1, 0] and o["status"].tolist() == [0, 0] and o["crowd_hit"].tolist() == [0, 0]
    assert o["pair_hit"][0].tolist() == [[1, 0], [0, 0]] and o["pair_hit"][1].tolist() == [[1, 0], [0, 0]]
    # values against the closed form: local coordinates below 8 m (half an ulp 4.8e-7), about a dozen roundings from joint to clearance
    assert float((o["crowd_clearance"] - 0.3).abs().max()) < 1e-5 and abs(float(o["pair_clearance"][0, 0, 0]) + 0.3) < 1e-5
    assert torch.equal(o["goal_dist"][1], sel["goal_dist"][1]) and abs(float(o["goal_dist"][0]) - float(sel["terms"][0, 1, 0])) < 1e-5
    pool = _new_pool()
    _check_launch("select_joint two people", c, o, 2, pool, jref, _cylinder_state(c, w=1.0))
    got, r64 = torch.cat(pool["got"], 1), torch.cat(pool["r64"], 1)
    fin = torch.isfinite(r64)
    assert float((got.double() - r64)[fin].abs().max()) < 1e-5 and all(pool["ok"])


def test_group_does_not_depend_on_batch(small_world):
    sizes, N, S = (1, 2, 5), 70, 3
    c = _case(small_world, sizes, N, 77, extra=2, interleave=True)
    full = _joint(c, S)
    for gi, members in enumerate(c["groups"]):
        one = _joint(c, S, groups=[members])
        for k in PER_SEQ:
            assert torch.equal(one[k][members], full[k][members]), (gi, k)
        for k in TRACES + ("choice_trace",):
            assert torch.equal(one[k][:, members], full[k][:, members]), (gi, k)
        assert torch.equal(one["changed"][:, 0], full["changed"][:, gi])
        rest = [m for m in range(c["b"]) if m not in members]
        assert bool((one["choice_trace"][:, rest] == -7).all()) and bool((one["crowd_hit"][rest] == -7).all())
    # the order of the groups in the launch does not matter either
    rev = _joint(c, S, groups=c["groups"][::-1])
    grouped = sorted(m for g in c["groups"] for m in g)
    for k in PER_SEQ:
        assert torch.equal(rev[k][grouped], full[k][grouped]), k
    for k in TRACES + ("choice_trace",):
        assert torch.equal(rev[k][:, grouped], full[k][:, grouped]), k
    assert torch.equal(rev["changed"], full["changed"].flip(1))


def test_joint_entry_rejects_bad_arguments(small_world):
    """Rejected before anything is launched: every pointer may therefore be the same scratch buffer."""
    from egogen_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(16384, device="cuda")
    p = C.c_void_p(buf.data_ptr())
    outs = ["choice", "status", "reached", "goal_dist", "pair_term", "pair_clearance", "joint_cost", "pair_hit", "choice_trace", "changed",
            "crowd_clearance", "crowd_hit"]

    def call(N=1, G=1, S=1, w=1.0, margin=0.5, body=0.3, null=None):
        return lib.egx_primitive_select_joint(p, 127, p, p, p, p, p, p, 1, N, p, p, G, S, w, margin, body, 0.1,
                                              *[None if k == null else p for k in outs], _lib.current_stream_ptr())
    bad = [{"N": 0}, {"N": 257}, {"S": 0}, {"S": 9}, {"G": 0}, {"margin": -0.1}, {"margin": float("nan")}, {"body": -0.1}, {"body": float("nan")},
           {"w": float("inf")}, {"w": float("nan")}] + [{"null": k} for k in outs]
    for kw in bad:
        assert call(**kw) == -1, kw
        with pytest.raises(_lib.EgxError):
            _lib.check(call(**kw), "egx_primitive_select_joint")
    torch.cuda.synchronize()
    assert not buf.any()                                                                      # nothing was launched


# ---- end to end ------------------------------------------------------------------------------------------------------------------
E2E_SAME = ("markers", "params", "rotmat", "transl", "pelvis", "z", "R0", "T0", "choice", "status", "goal_dist", "cost", "cost_terms", "colliding",
            "n_valid")
E2E_T0 = torch.tensor([[0.0, 0.0, 0.0], [0.8, 0.0, 0.0], [3.0, 0.0, 0.0], [3.8, 0.0, 0.0]])     # two pairs, partners 0.8 m apart


def _e2e(w, N, K, **extra):
    """b = 4: the three walkers of search_world and the first again"""
    four = lambda t, dim: torch.cat([t, t.narrow(dim, 0, 1)], dim)
    z = torch.randn(3, 4 * N, 128, generator=torch.Generator().manual_seed(91))[:K]
    kw = dict(z=z, reproj_factor=CFG_RF, weights=W_TEST, goal_thresh=0.0, to_numpy=False, T0=E2E_T0)
    kw.update(extra)
    return w["op"].generate_sequence_to_goal(four(w["data"], 1), four(w["bparams"], 1), four(w["betas"], 0), four(w["goal"], 0) + E2E_T0, K, N, **kw)


def test_singleton_groups_are_the_search_without_groups(search_world):
    base = _e2e(search_world, 4, 3)
    assert all(getattr(base, k) is None for k in base.JOINT_FIELDS)
    res = _e2e(search_world, 4, 3, groups=[0, 1, 2, 3])
    for k in E2E_SAME:
        assert torch.equal(getattr(res, k), getattr(base, k)), k
    assert torch.equal(res.individual_choice, res.choice) and not res.joint_changed.any() and not res.pair_term.any() and not res.crowd_hit.any()
    assert bool((res.crowd_clearance == float("inf")).all()) and res.groups.tolist() == [0, 1, 2, 3]


def test_generate_sequence_to_goal_with_groups(search_world):
    w = search_world
    op, K, b, N, S = w["op"], 2, 4, 4, 2
    members = [[0, 1], [2, 3]]
    for Kp in range(1, K + 1):                   # a run of Kp primitives is the prefix of the longer one: its last primitive from the loop's state
        with patched_loop(op, "_search_loop", no_host_wait=True) as seen:
            res = _e2e(w, N, Kp, groups=[0, 0, 1, 1])
        assert seen.calls == [(Kp, b, N)]
        if Kp > 1:
            for k in ("choice", "individual_choice", "choice_trace", "joint_cost", "crowd_clearance", "cost"):
                assert torch.equal(getattr(res, k)[:Kp - 1], getattr(prev, k)), k
        prev = res
        assert res.pair_term.shape == (Kp, S, b, N) and res.choice_trace.shape == (Kp, S, b) and res.joint_changed.shape == (Kp, S, 2)
        assert res.crowd_clearance.shape == (Kp, b) and res.individual_choice.shape == (Kp, b) and res.search["crowd_hit"] is res.crowd_hit
        assert torch.equal(res.choice, res.choice_trace[:, -1])
        ch = res.choice[Kp - 1].long()
        pp = seen.s["pp"].reshape(b, N, 20, 93)
        assert torch.equal(res.params[Kp - 1], pp[torch.arange(b), ch])                      # the hand-off continued from the joint choice
    assert float(res.pair_term.max()) > 0.0                                                  # partners 0.8 m apart, margin 0.5 + radii 0.6: they feel each other
    # crowd_clearance from the returned records, in float64: the records are the float32 values the kernel read (joint 0, R0, T0), so the
    # two differ by the kernel's own roundings only: coordinates below 8 m (an ulp of 4.8e-7), about a dozen of them
    f64 = lambda t: t.double().cpu()
    world = torch.einsum("kbij,kbtj->kbti", f64(res.rotmat), f64(res.pelvis)[:, :, 2:]) + f64(res.transl)[:, :, None]
    for k in range(K):
        for g in members:
            d = world[k, g[0], :, :2] - world[k, g[1], :, :2]
            c64 = float((torch.sqrt((d * d).sum(-1)) - 0.6).min())
            for m in g:
                assert abs(float(res.crowd_clearance[k, m]) - c64) < 1e-5, (k, m)
                if abs(c64) > 1e-5:
                    assert int(res.crowd_hit[k, m]) == int(c64 < 0)
    res_np = _e2e(w, N, K, groups=[0, 0, 1, 1], to_numpy=True)
    assert isinstance(res_np.crowd_clearance, np.ndarray) and np.array_equal(res_np.choice_trace, res.choice_trace.cpu().numpy())
    assert np.array_equal(res_np.groups, [0, 0, 1, 1])


def test_result_with_groups_saves_and_reloads(search_world, tmp_path):
    """a joint result saves like any other, its files are obstacles for the next person, and the joint fields stay on the result"""
    from egogen_amd import MovingObstacles
    res = _e2e(search_world, 4, 2, groups=[0, 0, 1, 1], to_numpy=True)
    before = {k: np.array(getattr(res, k)) for k in res.JOINT_FIELDS}
    paths = [res.save(str(tmp_path), i, man_id=f"p_{i}") for i in range(4)]
    assert [os.path.basename(p) for p in paths] == [f"motion_p_{i}.pkl" for i in range(4)]
    people = MovingObstacles.from_rollout_files(paths)
    assert np.array_equal(people.xy, MovingObstacles.from_sequences(res).xy)
    for k in res.JOINT_FIELDS:
        assert np.array_equal(getattr(res, k), before[k], equal_nan=True) and res.search[k] is getattr(res, k), k


def test_gen_motion_driver_people(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = tmp_path / "crowd"
    cmd = [sys.executable, os.path.join(ROOT, "exp_GAMMAPrimitive", "gen_motion.py"), "--n-primitives", "2", "--seed", "3", "--num-verts", str(V_SMALL),
           "--n-gens", "2", "--n-candidates", "4", "--people", "0,0,0:0.3,3,0.9;0.8,0,0:0.5,3,0.9;0.4,3,180:0.4,0,0.9", "--out", str(out)]
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    files = sorted(f for f in os.listdir(out) if f.startswith("motion_") and f.endswith(".pkl"))
    assert files == sorted(f"motion_3_{v}_p{p}.pkl" for v in range(2) for p in range(3)), files
    lines = re.findall(r"variant (\d+): minimum crowd clearance (-?[0-9.]+) m, crowd hits (\d+), members still changing in a last sweep (\d+)", r.stdout)
    assert [int(v[0]) for v in lines] == [0, 1], r.stdout[-1500:]
    assert all(np.isfinite(float(v[1])) for v in lines)
    for flags in (["--start", "0,0,0"], ["--goal", "0,1,0.9"], ["--beam-width", "2"]):
        bad = subprocess.run(cmd + flags, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
        assert bad.returncode == 2 and "--people" in bad.stderr, flags
