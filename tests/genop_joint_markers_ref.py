"""The marker-level pair model of the joint step (`generate_sequence_to_goal(groups=, pair_model="markers")`, entries
egx_pair_marker_dist and egx_primitive_select_joint_markers, csrc/genop_joint_markers.hip) as plain torch, parametrised by dtype: the
float64 truth and the float32 yardstick of tests/test_genop_joint_markers_{cpu,gpu}.py.  The inputs are taken as the float32 values
the device reads; every operation is rounded in `dtype`.  The functions run on whatever device their inputs live on (the
exhaustive tables of the larger GPU cases are billions of distances: those are computed with torch on the GPU, in chunks).

  * `world_markers(R0, T0, mp, Y_gen, rf, dtype)`: the blended markers of every row at the predicted frames, in the world;
  * `bad_frames(world)`: the row-frames with a non-finite coordinate;
  * `pair_dist(wa, wb)`: the exhaustive table of two members' rows, +inf where either row-frame is bad;
  * `group_table(world, members)`: `pair_dist` of every unordered pair of members, keyed by their positions (a, b), a < b.

A `state` is one group, a plain dict: members (sequence indices, in order), choice {sequence: row}, D {(a, b): [N,N,18]} a distance
table as `group_table` gives it (or as the device wrote it), bad [b,N,18] bool, cost [b,N], terms [b,N,5], colliding [b,N], and
the scalars w, margin, skin.  The frame clearance is read from the table, c_t = min over the others of D - skin; from there on
`member_step` and `sweeps` are those of tests/genop_joint_ref.py (`step_of_clearances`, `sweeps`)."""
import torch

from tests import genop_joint_ref as jref
from tests.genop_joint_ref import first_by_key, state_before  # noqa: F401  (the order and the trace bookkeeping are shared)

CHUNK = 1 << 26          # elements of the largest intermediate of `pair_dist`


def world_markers(R0, T0, mp, Y_gen, rf, dtype):
    """R0 [rows,3,3], T0 [rows,3], mp [rows,20,67,3] (the body model's markers), Y_gen [18,rows,201] (the prior's), rf -> [rows,18,67,3]"""
    rows = mp.shape[0]
    proj = mp.reshape(rows, 20, 67, 3)[:, 2:].to(dtype)
    pred = Y_gen.reshape(18, rows, 67, 3).permute(1, 0, 2, 3).to(dtype)
    rf = torch.tensor(float(rf), dtype=torch.float32).to(dtype)
    m = rf * proj + (1 - rf) * pred
    R, T = R0.reshape(rows, 3, 3).to(dtype), T0.reshape(rows, 3).to(dtype)
    w = R[:, None, None, :, 0] * m[..., 0:1]
    w = w + R[:, None, None, :, 1] * m[..., 1:2]
    w = w + R[:, None, None, :, 2] * m[..., 2:3]
    return w + T[:, None, None, :]


def bad_frames(world):
    """[...,18,67,3] -> [...,18] bool"""
    return ~torch.isfinite(world).all(-1).all(-1)


def pair_dist(wa, wb):
    """wa [Na,18,67,3], wb [Nb,18,67,3] -> D [Na,Nb,18]: sqrt of the least of the 67 x 67 values (dx^2 + dy^2) + dz^2; +inf where
    either row-frame is bad"""
    Na, Nb = wa.shape[0], wb.shape[0]
    out = torch.empty(Na, Nb, 18, dtype=wa.dtype, device=wa.device)
    step = max(1, CHUNK // (Nb * 18 * 67 * 67))
    for a0 in range(0, Na, step):
        a = wa[a0:a0 + step]
        d2 = None
        for c in range(3):
            d = a[:, None, :, :, None, c] - wb[None, :, :, None, :, c]          # [na,Nb,18,67,67]
            d2 = d * d if d2 is None else d2 + d * d
        d2 = torch.where(torch.isnan(d2), torch.full_like(d2, float("inf")), d2)
        out[a0:a0 + step] = torch.sqrt(d2.flatten(-2).amin(-1))
    bad = bad_frames(wa)[:, None] | bad_frames(wb)[None]
    return torch.where(bad, torch.full_like(out, float("inf")), out)


def pair_dist_rows(wa, wb):
    """wa, wb [n,18,67,3]: row k of the one against row k of the other -> [n,18] (`pair_dist` on chosen entries of a large table)"""
    d2 = None
    for c in range(3):
        d = wa[:, :, :, None, c] - wb[:, :, None, :, c]          # [n,18,67,67]
        d2 = d * d if d2 is None else d2 + d * d
    out = torch.sqrt(torch.where(torch.isnan(d2), torch.full_like(d2, float("inf")), d2).flatten(-2).amin(-1))
    return torch.where(bad_frames(wa) | bad_frames(wb), torch.full_like(out, float("inf")), out)


def group_table(world, members):
    """world [b,N,18,67,3], members (sequence indices) -> {(a, b): [N,N,18]} over the positions a < b"""
    return {(a, b): pair_dist(world[members[a]], world[members[b]]) for a in range(len(members)) for b in range(a + 1, len(members))}


def _scalars(state, dtype):
    f = lambda v: torch.tensor(v, dtype=torch.float32).to(dtype)
    return f(state["w"]), f(state["margin"]), f(state["skin"])


def _clearances(state, i, rows, dtype):
    """c [len(rows),18] of the rows `rows` of member i against the others' current choices"""
    _, _, skin = _scalars(state, dtype)
    members, m = state["members"], state["members"][i]
    c = torch.full((len(rows), 18), float("inf"), dtype=dtype)
    for j, mj in enumerate(members):
        if j == i:
            continue
        cj = int(state["choice"][mj])
        d = state["D"][(i, j)][rows, cj] if i < j else state["D"][(j, i)][cj, rows]
        c = torch.minimum(c, d.to(dtype).cpu())
    c = c - skin
    return torch.where(torch.as_tensor(state["bad"])[m, rows].cpu(), torch.full_like(c, float("nan")), c)


def member_step(state, i, dtype):
    """-> dict over the N rows of member i: term, clearance, hit, joint_cost, finite, cls, and `choice`"""
    w, margin, _ = _scalars(state, dtype)
    return jref.step_of_clearances(state, i, _clearances(state, i, list(range(state["cost"].shape[1])), dtype), w, margin)


def sweeps(state, S, dtype):
    return jref.sweeps(state, S, dtype, member_step)


def crowd_clearance(state, dtype):
    """[P]: min_t of every member's chosen row against the other members' chosen rows (+inf for a group of one)"""
    out = [_clearances(state, i, [int(state["choice"][m])], dtype).amin(1)[0] for i, m in enumerate(state["members"])]
    return torch.stack(out)
