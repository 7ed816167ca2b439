"""Look-ahead in the primitive search (`generate_sequence_to_goal(lookahead=, lookahead_slack=)`: entries
egx_obstacle_ahead_clearance of csrc/genop_obstacle_ahead.hip and egx_primitive_select_joint_ahead of csrc/genop_joint_ahead.hip)
restated on the CPU, the yardsticks of tests/test_genop_lookahead_{cpu,gpu}.py.  The inputs are taken as the float32 values the
device reads; every operation is rounded on its own in the dtype asked for: float32 is the device's arithmetic rounding for
rounding (include/egogen_hip.h states each one), float64 the truth.

The rule of both entries.  p [rows,20,2] is the world xy of the pelvis of the 20 bodies of a row (`pelvis`: float32 with the
device's three fused multiply-adds, tests/genop_obstacle_markers_ref.fma32; float64 by tests/genop_obstacles_ref.world_pelvis).
d = p(19) - p(1); p_h(t) = p(t) + h * d (`predicted`); c_t = min(c_{t,0}, min_{h=1..H} max(0, c_{t,h}) + h * slack), NaN where
c_{t,0} or any c_{t,h} is NaN (`combine`: the test for NaN comes before the max).

  * `obstacle_clearances`: the [rows,18] table of egx_obstacle_ahead_clearance - the candidate predicted, the recorded tracks read at
    the absolute frames clamp(frame0 + t + 18 h, 0, T - 1) (tests/genop_obstacles_ref.window at frame0 + 18 h);
  * `row_terms`: clearance, term and hit of every row from that table, as tests/genop_obstacles_ref.row_terms returns them (bits: with
    the wave reduction's summation tree, tests/genop_obstacle_markers_ref.terms_of_clearance);
  * `pair_clearances` / `member_step` / `crowd_clearance` / `sweeps`: the joint step with both people predicted, on the states of
    tests/genop_joint_ref.py with three more keys: pelvis [b,N,20,2] (or R0 / T0 / J, from which `pelvis` makes it), lookahead,
    lookahead_slack.

Two arithmetics.  bits=False is that of the cylinder restatements this one extends - torch expressions, torch's sums - so that H = 0
gives their results exactly, in float32 and in float64.  bits=True (float32) is the device's: numpy, whose operations round one at a
time and whose root is correctly rounded (torch's vectorised root differs in the last bit of about one value in 150), and the frame
sum by the wave reduction's tree."""
import numpy as np
import torch

from tests import genop_joint_ref as jref
from tests import genop_obstacle_markers_ref as kref
from tests import genop_obstacles_ref as oref

NF = 18
MAX_OBSTACLES, MAX_LOOKAHEAD = 32, 8
f32 = np.float32


def _np(dtype):
    return np.float32 if dtype in (torch.float32, np.float32) else np.float64


def _a(t, dt=np.float32):
    return np.asarray(t.detach().cpu() if torch.is_tensor(t) else t, dt)


def pelvis(R0, T0, joints, dtype):
    """R0 [B,3,3], T0 [B,3], joints [B,20,J,3] -> world xy [B,20,2] numpy of joint 0 of every body: float32 as the device nests it,
    fma(R0[2], z, fma(R0[1], y, R0[0] x)) + T0; float64 as tests/genop_obstacles_ref.world_pelvis"""
    if _np(dtype) is np.float64:
        return oref.world_pelvis(R0, T0, joints, torch.float64).numpy()
    R, T, j = _a(R0).reshape(-1, 1, 3, 3), _a(T0).reshape(-1, 1, 3), _a(joints)[:, :, 0]
    with np.errstate(invalid="ignore", over="ignore"):
        out = [kref.fma32(R[..., c, 2], j[..., 2], kref.fma32(R[..., c, 1], j[..., 1], R[..., c, 0] * j[..., 0])) + T[..., c] for c in range(2)]
    return np.stack(out, -1).astype(np.float32)


def predicted(p, h, dtype):
    """p [...,20,2] -> [...,18,2]: p(t) + h * d for t = 2..19, d = p(19) - p(1): one rounded difference, one rounded product and one
    rounded addition per axis"""
    dt = _np(dtype)
    p = np.asarray(p, dt)
    with np.errstate(invalid="ignore", over="ignore"):
        d = p[..., 19:20, :] - p[..., 1:2, :]
        return p[..., 2:, :] + dt(h) * d


def combine(c0, ahead, slack, dtype):
    """c0 [...] and ahead = [c_1, .., c_H] -> c = min(c0, min_h max(0, c_h) + h * slack); NaN where any of them is"""
    dt = _np(dtype)
    c = np.asarray(c0, dt).copy()
    bad = np.isnan(c)
    s = dt(f32(slack))
    with np.errstate(invalid="ignore", over="ignore"):
        for h, ch in enumerate(ahead, start=1):
            ch = np.asarray(ch, dt)
            bad = bad | np.isnan(ch)
            c = np.fmin(c, np.maximum(dt(0), np.where(np.isnan(ch), dt(0), ch)) + dt(h) * s)
    return np.where(bad, dt(np.nan), c)


def _cylinders(points, others, rr, bits):
    """points [n,18,2], others [18,Q,2], rr a number or [Q] -> [n,18] numpy: min over the Q others of |p_t - o_t| - rr with the
    clearance's roundings; +inf for Q = 0; another's NaN drops out; a NaN point gives NaN.  bits: numpy, whose float32 operations round
    one at a time and whose root is correctly rounded, as the device's; else the torch expressions of the cylinder restatements
    (tests/genop_joint_ref._clearances; torch's vectorised root is not correctly rounded in every case)."""
    if not bits:
        t = torch.as_tensor(points)
        return jref._clearances(t, torch.as_tensor(others).to(t.dtype), torch.as_tensor(rr).to(t.dtype)).numpy()
    dt = points.dtype.type
    out = np.full(points.shape[:2], np.inf, dt)
    with np.errstate(invalid="ignore", over="ignore"):
        if others.shape[1]:
            d = points[:, :, None, :] - others[None].astype(dt)
            c = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) - np.asarray(rr, dt)
            out = np.where(np.isnan(c), dt(np.inf), c).min(-1)
    return np.where(np.isnan(points).any(-1), dt(np.nan), out)


def obstacle_clearances(p, xy, radius, count, set_of_row, frame0, body_radius, H, slack, dtype, bits=False):
    """p [B,20,2], xy [S,O_max,T,2], radius [S,O_max], count [S], set_of_row [B] -> c [B,18] numpy in `dtype`: the table of
    egx_obstacle_ahead_clearance (H = 0: the c_t of the cylinder entries); bits: see `_cylinders`"""
    dt = _np(dtype)
    p = np.asarray(p, dt)
    xy, radius, count = _a(xy), _a(radius), np.asarray(count).reshape(-1)
    S, O_max = xy.shape[:2]
    set_of_row = np.asarray(set_of_row).reshape(-1)
    pts = [predicted(p, h, dt) for h in range(int(H) + 1)]
    pts[0] = p[:, 2:]
    out = np.zeros((p.shape[0], NF), dt)
    for r in range(p.shape[0]):
        s = int(min(max(set_of_row[r], 0), S - 1))
        n = int(min(max(count[s], 0), min(O_max, MAX_OBSTACLES))) if O_max else 0
        rr = radius[s, :n].astype(dt) + dt(f32(body_radius))                # float32: the one rounded addition the device stages
        c = [_cylinders(pts[h][r][None], oref.window(xy[s, :n], int(frame0) + NF * h, torch.float32).numpy().astype(dt), rr, bits)[0]
             for h in range(int(H) + 1)]
        out[r] = combine(c[0], c[1:], slack, dt)
    return out


def row_terms(p, xy, radius, count, set_of_row, frame0, margin, body_radius, H, slack, dtype, bits=False):
    """-> dict of [B] torch tensors as tests/genop_obstacles_ref.row_terms returns them, from the look-ahead clearances: clearance =
    min_t c_t, term = sum_t max(0, margin - c_t) / 18, hit = clearance < 0; a NaN frame gives a NaN term and clearance and no hit.
    bits: the device's bits in float32 - numpy's roundings and the frame sum by the wave reduction's tree; else the arithmetic of
    tests/genop_obstacles_ref.row_terms, in its order."""
    tdt = torch.float32 if _np(dtype) is np.float32 else torch.float64
    c = obstacle_clearances(p, xy, radius, count, set_of_row, frame0, body_radius, H, slack, dtype, bits)
    if bits:
        return kref.terms_of_clearance(c, margin, tdt)
    c = torch.as_tensor(c)
    m = torch.tensor(margin, dtype=torch.float32).to(tdt)
    pen = torch.where(torch.isnan(c), c, (m - c).clamp(min=0))
    clearance = c.amin(dim=1)
    return {"clearance": clearance, "term": pen.sum(dim=1) / NF, "hit": clearance < 0}


# ---- the joint step ------------------------------------------------------------------------------------------------------------------
def _pelvis_of(state, dtype):
    """[b,N,20,2] torch in `dtype`, cached on the state"""
    cache = state.setdefault("_pelvis", {})
    if dtype not in cache:
        b, N = state["cost"].shape
        if "pelvis" in state:
            cache[dtype] = torch.as_tensor(_a(state["pelvis"], np.float32)).to(dtype).reshape(b, N, 20, 2)
        else:
            cache[dtype] = torch.as_tensor(pelvis(state["R0"], state["T0"], state["J"], dtype)).reshape(b, N, 20, 2)
    return cache[dtype]


def pair_clearances(state, i, rows, dtype, H=None, bits=False):
    """rows [n,20,2] (tracks of member i) against the other members' current choices, both predicted -> c [n,18] torch"""
    H = int(state.get("lookahead", 0)) if H is None else H
    dt = _np(dtype)
    rr = jref._scalars(state, dtype)[2].numpy()
    xy = _pelvis_of(state, dtype).numpy()
    rows = np.asarray(rows, dt)
    others = [xy[j, int(state["choice"][j])] for k, j in enumerate(state["members"]) if k != i]
    at = lambda q, h: q[..., 2:, :] if h == 0 else predicted(q, h, dt)
    c = []
    for h in range(H + 1):
        oth = np.stack([at(o, h) for o in others], 1) if others else np.zeros((NF, 0, 2), dt)
        c.append(_cylinders(at(rows, h), oth, rr, bits))
    return torch.as_tensor(combine(c[0], c[1:], state.get("lookahead_slack", 0.1), dtype))


def member_step(state, i, dtype, bits=False):
    """tests/genop_joint_ref.member_step with the look-ahead clearances -> dict over the N rows of member i: term, clearance, hit,
    joint_cost, finite, cls, and `choice`.  bits: the device's bits in float32 (`_cylinders`, and the frame sum by the wave reduction's tree)."""
    w, margin, _ = jref._scalars(state, dtype)
    m = state["members"][i]
    c = pair_clearances(state, i, _pelvis_of(state, dtype)[m], dtype, bits=bits)
    if not bits:
        return jref.step_of_clearances(state, i, c, w, margin)
    t = kref.terms_of_clearance(c.numpy(), state["margin"], dtype)          # the tree changes the term only, and what follows from it
    cost = torch.as_tensor(state["cost"][m]).to(dtype)
    jc = cost + w * t["term"]
    finite = torch.isfinite(cost) & torch.isfinite(torch.as_tensor(state["terms"][m])).all(-1) & torch.isfinite(t["term"]) & torch.isfinite(jc)
    cls = (~finite).long() * 2 + (torch.as_tensor(state["colliding"][m]).bool() | t["hit"]).long()
    choice = jref.first_by_key(cls, torch.where(finite, jc, torch.zeros_like(jc)))
    return {"term": t["term"], "clearance": t["clearance"], "hit": t["hit"], "joint_cost": jc, "finite": finite, "cls": cls, "choice": choice}


def member_step_bits(state, i, dtype):
    return member_step(state, i, dtype, bits=True)


def sweeps(state, S, dtype, bits=False):
    """tests/genop_joint_ref.sweeps with this model's member step"""
    return jref.sweeps(state, S, dtype, step=member_step_bits if bits else member_step)


def crowd_clearance(state, dtype, bits=False):
    """[P]: min_t of every member's chosen track against the other members' chosen tracks, at h = 0 only: the crowd as written"""
    xy = _pelvis_of(state, dtype)
    out = []
    for i, m in enumerate(state["members"]):
        c = pair_clearances(state, i, xy[m, int(state["choice"][m])][None], dtype, H=0, bits=bits)
        out.append(c.amin(1)[0])
    return torch.stack(out)


state_before, first_by_key = jref.state_before, jref.first_by_key
