"""The joint step of the greedy primitive search (`generate_sequence_to_goal(groups=)`, entry egx_primitive_select_joint,
csrc/genop_joint.hip) as plain torch on the CPU, parametrised by dtype: the float64 truth and the float32 yardstick of
tests/test_genop_joint_{cpu,gpu}.py.  The inputs are taken as the float32 values the device reads (the selection's cost, cost_terms
and colliding among them); every operation is rounded in `dtype`.

A `state` is one group, a plain dict: members (sequence indices, in order), choice {sequence: row}, the rows of every sequence -
either track [b,N,18,2] (world xy of the pelvis at the predicted frames, given) or R0 [b*N,3,3] / T0 [b*N,3] / J [b*N,20,jpb,3]
(genop_obstacles_ref.world_pelvis makes the tracks, cached per dtype) - cost [b,N], terms [b,N,5], colliding [b,N], and the scalars
w, margin, body_radius.

  * `member_step(state, i, dtype)`: the rows of member i against the others' current choices -> row terms and the choice;
  * `step_of_clearances(state, i, c, w, margin)`: the same from given frame clearances onward: what every pair model shares;
  * `sweeps(state, S, dtype, step)`: S Gauss-Seidel sweeps of `step` from the state's choices (which follow) -> traces;
  * `crowd_clearance(state, dtype)`: every member's chosen track against the others' chosen tracks;
  * `state_before(start, trace, s, i)`: the choices a member step saw, from a choice trace."""
import torch

from tests import genop_obstacles_ref as oref


def tracks(state, dtype):
    """[b,N,18,2] world xy of the pelvis at frames 2..19 of every row, in `dtype`"""
    cache = state.setdefault("_tracks", {})
    if dtype not in cache:
        if "track" in state:
            cache[dtype] = torch.as_tensor(state["track"]).to(dtype)
        else:
            b, N = state["cost"].shape
            cache[dtype] = oref.world_pelvis(state["R0"], state["T0"], state["J"], dtype)[:, 2:].reshape(b, N, 18, 2)
    return cache[dtype]


def _scalars(state, dtype):
    f = lambda v: torch.tensor(v, dtype=torch.float32).to(dtype)
    r = torch.tensor(state["body_radius"], dtype=torch.float32)
    return f(state["w"]), f(state["margin"]), (r + r).to(dtype)


def _clearances(p, others, rr):
    """p [n,18,2] tracks, others [18,Q,2] -> c [n,18]: min over the Q others of |p_t - o_t| - rr; +inf for Q = 0; a NaN distance from
    another's coordinate drops out; a NaN own position gives NaN"""
    c = torch.full(p.shape[:2], float("inf"), dtype=p.dtype)
    if others.shape[1]:
        d = p[:, :, None, :] - others[None]
        dist = torch.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) - rr
        c = torch.where(torch.isnan(dist), torch.full_like(dist, float("inf")), dist).amin(-1)
    return torch.where(torch.isnan(p).any(-1), torch.full_like(c, float("nan")), c)


def _others(state, i, dtype):
    xy = tracks(state, dtype)
    rows = [xy[j, int(state["choice"][j])] for k, j in enumerate(state["members"]) if k != i]
    return torch.stack(rows, 1) if rows else torch.zeros(18, 0, 2, dtype=dtype)


def first_by_key(cls, cost):
    """the first row in the order (class, cost, index)"""
    return min(range(len(cls)), key=lambda n: (int(cls[n]), float(cost[n]), n))


def step_of_clearances(state, i, c, w, margin):
    """the member step from the frame clearances c [N,18] of the rows of member i onward, whatever the pair model they come from
    -> dict over the N rows: term, clearance, hit, joint_cost, finite, cls, and `choice`"""
    m = state["members"][i]
    pen = torch.where(torch.isnan(c), c, (margin - c).clamp(min=0))
    clearance, term = c.amin(1), pen.sum(1) / 18
    hit = clearance < 0
    cost = torch.as_tensor(state["cost"][m]).to(c.dtype)
    jc = cost + w * term
    finite = torch.isfinite(cost) & torch.isfinite(torch.as_tensor(state["terms"][m])).all(-1) & torch.isfinite(term) & torch.isfinite(jc)
    cls = (~finite).long() * 2 + (torch.as_tensor(state["colliding"][m]).bool() | hit).long()
    choice = first_by_key(cls, torch.where(finite, jc, torch.zeros_like(jc)))
    return {"term": term, "clearance": clearance, "hit": hit, "joint_cost": jc, "finite": finite, "cls": cls, "choice": choice}


def member_step(state, i, dtype):
    """-> dict over the N rows of member i: term, clearance, hit, joint_cost, finite, cls, and `choice`"""
    w, margin, rr = _scalars(state, dtype)
    c = _clearances(tracks(state, dtype)[state["members"][i]], _others(state, i, dtype), rr)
    return step_of_clearances(state, i, c, w, margin)


def sweeps(state, S, dtype, step=member_step):
    """S sweeps over the members in order, from state["choice"], which ends as the joint choice -> dict: steps [S][P] (what
    `step`, the pair model's member step, gave), choice_trace [S,P], changed [S]"""
    P = len(state["members"])
    steps, trace, changed = [], [], []
    for _ in range(S):
        row, n = [], 0
        for i, m in enumerate(state["members"]):
            r = step(state, i, dtype)
            n += int(r["choice"] != int(state["choice"][m]))
            state["choice"][m] = r["choice"]
            row.append(r)
        steps.append(row)
        trace.append([int(state["choice"][m]) for m in state["members"]])
        changed.append(n)
    return {"steps": steps, "choice_trace": torch.tensor(trace, dtype=torch.long).reshape(S, P), "changed": torch.tensor(changed)}


def crowd_clearance(state, dtype):
    """[P]: min_t of every member's chosen track against the other members' chosen tracks (+inf for a group of one)"""
    _, _, rr = _scalars(state, dtype)
    xy = tracks(state, dtype)
    out = [_clearances(xy[m, int(state["choice"][m])][None], _others(state, i, dtype), rr).amin(1)[0]
           for i, m in enumerate(state["members"])]
    return torch.stack(out)


def state_before(members, start, trace, s, i):
    """{sequence: row} as member step (s, i) saw it: members before i hold their choice of sweep s, the others that of sweep
    s - 1 (`start` {sequence: row} before the first sweep); trace [S,b] indexed by sequence"""
    prev = (lambda m: int(start[m])) if s == 0 else (lambda m: int(trace[s - 1][m]))
    return {m: (int(trace[s][m]) if k < i else prev(m)) for k, m in enumerate(members)}
