"""Restatement of the two people launches of csrc/genop_policy.hip in torch / numpy: the world xy box a sequence publishes of its two
seed frames' markers (float64 the truth of the `held()` rule, float32 its yardstick) and the observation whose rays are cast against
the static polygon minus the UNION of the boxes of the sequence's group-mates and of its obstacle tracks at the two seed frames.
State, dist and time are `genop_policy_ref.observe`'s; the rays restate `oracle.env.calc_egosensing` with the holes' containment
and edges added.  Also the synthetic inputs the CPU and the GPU tests share.  A plain module."""
import numpy as np
import torch

from oracle.env import _point_in_rings
from tests import genop_policy_ref as ref

B = 5
IDS = np.array([1, 0, 1, 1, 2])        # group of three {0, 2, 3} (first to appear), sequence 1 alone, sequence 4 alone with obstacles
SEES, LONE, IN_ONE, IN_TWO, TRACKS = 0, 1, 2, 3, 4      # the part every sequence plays, see `people_inputs`
OBS_INDEX = np.array([0, 1, 1, 1, 0], np.int32)          # set 0: two live tracks; set 1: none, its rows hold boxes round the eyes
O_MAX, T_OBS = 2, 3
FRAMES = (-5, 1, 2, 40)                # both frames before the track, inside it, the second beyond it, both beyond it


# ---- the boxes -------------------------------------------------------------------------------------------------------
def boxes(x0, x1, R0, T0, dtype):
    """-> [b,4] (minx, miny, maxx, maxy) over the world xy R0 m + T0 of the 2 x 67 markers of x0 / x1 [b,201], in `dtype`; four NaN
    where a world coordinate is not finite."""
    c = lambda t: torch.as_tensor(t).to(dtype)
    m = torch.stack([c(x0), c(x1)], 1).reshape(-1, 134, 3)
    w = torch.einsum("bij,bkj->bki", c(R0).reshape(-1, 3, 3), m) + c(T0)[:, None]
    out = torch.cat([w[..., :2].min(1).values, w[..., :2].max(1).values], -1)
    out[~torch.isfinite(w[..., :2]).all(-1).all(-1)] = float("nan")
    return out


def track_boxes(obs, set_i, frame, dtype):
    """The boxes [count,4] of the live tracks of set `set_i` at the absolute frames frame, frame + 1 (a track is held at its first /
    last position): min / max over the two frames of xy -+ radius.  obs: (xy [S,O,T,2], radius [S,O], count [S])."""
    xy, radius, count = (torch.as_tensor(t) for t in obs)
    T = xy.shape[2]
    f = [min(max(int(frame) + a, 0), T - 1) for a in (0, 1)]
    n = min(max(int(count[set_i]), 0), xy.shape[1])
    p, r = xy[set_i, :n][:, f].to(dtype), radius[set_i, :n].to(dtype)[:, None, None]
    return torch.cat([(p - r).min(1).values, (p + r).max(1).values], -1)


def csr(ids):
    """ids [b] -> (group_start, group_member, member_group) int32, as `PersonGroups` lays them out"""
    from egogen_amd.crowd import PersonGroups
    g = PersonGroups.from_ids(np.asarray(ids), len(ids)).to("cpu")
    return g.group_start.numpy(), g.group_member.numpy(), g.member_group.numpy()


def holes(i, box, groups, obs, obs_index, frame, dtype):
    """The holes [n,4] of sequence i: the boxes of the other members of its group (box [b,4], groups None or the `csr` triple), then
    of the tracks of its set (obs None or the obstacle triple; obs_index None: set 0); a box with a non-finite entry is left out."""
    out = [torch.zeros(0, 4, dtype=dtype)]
    if groups is not None:
        start, member, of = groups
        g = int(of[i])
        out += [torch.as_tensor(box).to(dtype)[int(m)][None] for m in member[start[g]:start[g + 1]] if int(m) != i]
    if obs is not None:
        out.append(track_boxes(obs, 0 if obs_index is None else int(obs_index[i]), frame, dtype))
    out = torch.cat(out)
    return out[torch.isfinite(out).all(-1)]


# ---- the rays --------------------------------------------------------------------------------------------------------
def box_edges(bx):
    """[n,4] boxes -> [4n,4] edges (lo,lo) -> (hi,lo) -> (hi,hi) -> (lo,hi) -> (lo,lo), float64"""
    bx = np.asarray(bx, np.float64).reshape(-1, 4)
    cx, cy = bx[:, [0, 2, 2, 0]], bx[:, [1, 1, 3, 3]]
    return np.stack([cx, cy, np.roll(cx, -1, 1), np.roll(cy, -1, 1)], -1).reshape(-1, 4)


def calc_egosensing_holes(joints_w, edges, bx, ray_len=7.0):
    """`oracle.env.calc_egosensing` for one sequence with holes.  joints_w [2,127,3] world, edges [E,4] float64 or None (the unbounded
    plane), bx [n,4] the holes.  The eye sees nothing outside the static polygon (even-odd) or inside ANY box (lo <= p < hi: the
    union, not even-odd over the boxes' edges); otherwise d is the nearest hit over the static and the boxes' edges."""
    joint = torch.as_tensor(joints_w).detach().cpu().numpy().astype(np.float32)
    look_at = (joint[:, 57] - joint[:, 23] + joint[:, 56] - joint[:, 24]).astype(np.float64)
    look_at[:, -1] = 0.0
    look_at = look_at / np.linalg.norm(look_at, axis=-1, keepdims=True)
    eye_2d = (joint[:, 23] + joint[:, 24]) / 2
    ang = np.linspace(-np.pi / 2, np.pi / 2, 32)
    out = np.zeros((2, 32), np.float64)
    bx = np.asarray(bx, np.float64).reshape(-1, 4)
    static = np.zeros((0, 4)) if edges is None else np.asarray(edges, np.float64)
    e = np.concatenate([static, box_edges(bx)])
    ex0, ey0, edx, edy = e[:, 0], e[:, 1], e[:, 2] - e[:, 0], e[:, 3] - e[:, 1]
    for t in range(2):
        ox, oy = float(eye_2d[t, 0]), float(eye_2d[t, 1])
        in_box = bool(((bx[:, 0] <= ox) & (ox < bx[:, 2]) & (bx[:, 1] <= oy) & (oy < bx[:, 3])).any())
        if in_box or (edges is not None and not _point_in_rings(ox, oy, static)):
            continue
        c, s = look_at[t, 0], look_at[t, 1]
        for i in range(32):
            dx = c * np.cos(ang[i]) - s * np.sin(ang[i])
            dy = s * np.cos(ang[i]) + c * np.sin(ang[i])
            den = dx * edy - dy * edx
            with np.errstate(divide="ignore", invalid="ignore"):
                tt = ((ex0 - ox) * edy - (ey0 - oy) * edx) / den
                uu = ((ex0 - ox) * dy - (ey0 - oy) * dx) / den
            ok = (np.abs(den) > 0) & (tt > 0) & (tt <= ray_len) & (uu >= 0) & (uu <= 1)
            d = tt[ok].min() if ok.any() else ray_len
            end = np.array([ox + dx * d, oy + dy * d])
            out[t, i] = np.linalg.norm(end - np.array([ox, oy]))
    return torch.from_numpy((-1 + 2 * (out / ray_len).astype(np.float32)).astype(np.float32))


def observe_people(j2, R_prev, T_prev, R0, T0, x0, x1, goal, poly, ray_len, step, max_depth, dtype, groups=None, obs=None, obs_index=None,
                   frame=0, eye_shift=(0.0, 0.0)):
    """-> state, egosensing, dist, time, people_count, box.  The arguments of `genop_policy_ref.observe`, then the `csr` triple, the
    obstacle triple, the set of every sequence and the absolute frame of the first seed frame.  The mates' holes are the
    restatement's own boxes, in `dtype`."""
    b = j2.shape[0]
    state, _, dist, time = ref.observe(j2, R_prev, T_prev, R0, T0, x0, x1, goal, None, ray_len, step, max_depth, dtype)
    box = boxes(x0, x1, R0, T0, dtype)
    c = lambda t: torch.as_tensor(t).to(dtype)
    jw = torch.einsum("bij,btkj->btki", c(R_prev), c(j2)) + c(T_prev)[:, None, None]
    jw = jw + torch.tensor([eye_shift[0], eye_shift[1], 0.0], dtype=dtype)
    ego, count = torch.ones(b, 2, 32, dtype=torch.float32), torch.zeros(b, dtype=torch.int32)
    for i in range(b):
        h = holes(i, box, groups, obs, obs_index, frame, dtype)
        count[i] = len(h)
        e = None
        if poly is not None:
            edges, off, idx = poly[:3]
            e = np.asarray(edges, np.float64)[off[idx[i]]:off[idx[i] + 1]]
        if e is not None or len(h):
            ego[i] = calc_egosensing_holes(jw[i], e, h.double().numpy(), ray_len)
    return state, ego, dist, time, count, box


# ---- the cases the CPU and the GPU tests share -----------------------------------------------------------------------------
def people_polygon(kind):
    """-> (poly or None, eyes [5,2]).  'square': one scene, the obstacle-only sequence starts outside it (blind, with holes);
    'two': scene 0 the square, scene 1 room0, the group in the square, the two single sequences in room0; 'gon1200': one scene,
    `genop_policy_ref.gon_edges`, everybody inside it."""
    eyes = np.array([[-1.0, -1.2], [2.6, 2.1], [-2.5, 2.0], [0.0, 2.2], [5.0, 0.3]])
    if kind == "none":
        return None, eyes
    if kind == "gon1200":
        gon = ref.gon_edges()
        return (gon, np.array([0, len(gon)], np.int32), np.zeros(B, np.int32)), eyes
    sq = ref.square_hole_edges()
    if kind == "square":
        return (sq, np.array([0, len(sq)], np.int32), np.zeros(B, np.int32)), eyes
    r0 = ref.room0_edges()
    inside = ref.polygon("two")[3]
    eyes[LONE], eyes[TRACKS] = inside[0], inside[2]
    return (np.concatenate([sq, r0]), np.array([0, len(sq), len(sq) + len(r0)], np.int32), np.array([0, 1, 0, 0, 1], np.int32)), eyes


def people_inputs(kind, N, frames_per_row, first, seed=0):
    """Everything the two launches read for the B = 5 sequences of IDS, as float32 CPU tensors, from two draws of
    `genop_policy_ref.observe_inputs`.  The eyes stand at `people_polygon(kind)`'s positions; the seed frames' markers are a cloud of
    0.25 m round a frame origin T0 that is placed so that
        SEES    (group of three) stands clear of every box and sees its mates' and the tracks of set 0
        IN_ONE  (group of three) stands inside the box of IN_TWO alone
        IN_TWO  (group of three) stands inside the boxes of SEES and IN_ONE, which overlap there
        LONE    (a group of one, set 1: no live track) has no hole: rows of set 1 hold boxes round its eye and IN_ONE's, never read
        TRACKS  (a group of one, set 0) sees two tracks, one of them passing 0.6 - 0.8 m beside it
    -> (inputs, poly, obstacle triple)."""
    poly, eyes = people_polygon(kind)
    da = ref.observe_inputs(N, frames_per_row, first, eyes[[0, 1, 2]], seed)
    db = ref.observe_inputs(N, frames_per_row, first, eyes[[3, 4, 4]], seed + 1)
    d = {}
    for k, v in da.items():
        if torch.is_tensor(v):
            per = v.shape[0] // ref.B
            d[k] = torch.cat([v, db[k][:2 * per]]).contiguous()
        else:
            d[k] = v
    g = torch.Generator().manual_seed(4000 + 7 * N + frames_per_row + seed)
    for name in ("x0", "x1"):
        d[name][::N] = torch.randn(B, 201, generator=g) * 0.25
    e = torch.as_tensor(eyes, dtype=torch.float32)
    centre = {SEES: e[IN_TWO] + torch.tensor([0.1, 0.05]), IN_ONE: e[IN_TWO] - torch.tensor([0.1, 0.05]),
              IN_TWO: e[IN_ONE] + torch.tensor([0.05, -0.05]), LONE: e[LONE] + torch.tensor([0.2, 0.1]), TRACKS: e[TRACKS]}
    T0 = d["T0"][::N].clone()
    for i, cxy in centre.items():
        T0[i, :2] = cxy
    d["T0"][::N] = T0
    xy = np.zeros((2, O_MAX, T_OBS, 2), np.float32)
    xy[0, 0] = eyes[TRACKS] + np.array([[0.8, 0.5], [0.7, 0.5], [0.6, 0.5]])
    # SEES' mates stand at 74 and 115 degrees from it, this track at 270: whichever way it looks, one of the three is ahead
    xy[0, 1] = eyes[SEES] + np.array([[0.0, -2.0], [0.1, -2.0], [0.2, -2.0]])
    xy[1, 0], xy[1, 1] = eyes[LONE], eyes[IN_ONE]
    obs = (xy, np.array([[0.3, 0.4], [1.0, 1.0]], np.float32), np.array([2, 0], np.int32))
    return d, poly, obs


def take(d, rows):
    """the sequences `rows` of an input set, in that order"""
    N, fpr = d["N"], d["frames_per_row"]
    out = {}
    for k, v in d.items():
        if torch.is_tensor(v):
            per = v.shape[0] // B
            out[k] = v.reshape(B, per, *v.shape[1:])[list(rows)].reshape(len(rows) * per, *v.shape[1:]).contiguous()
        else:
            out[k] = v
    return out


def seed_bodies(d):
    """The joints [b,2,127,3] of the two seed bodies the launch reads: frames first, first + 1 of row i * N + clamp(choice[i])."""
    N, fpr = d["N"], d["frames_per_row"]
    b = d["choice"].shape[0]
    J = d["joints"].reshape(b * N, fpr, 127, 3)
    rows = torch.arange(b) * N + d["choice"].long().clamp(0, N - 1)
    return J[rows, d["first"]:d["first"] + 2]


def observe_case(d, poly, obs, ray_len, step, max_depth, dtype, groups="ids", obs_index=OBS_INDEX, frame=0, eye_shift=(0.0, 0.0)):
    N = d["N"]
    return observe_people(seed_bodies(d), d["R_prev"], d["T_prev"], d["R0"][::N], d["T0"][::N], d["x0"][::N], d["x1"][::N], d["goal"], poly,
                          ray_len, step, max_depth, dtype, csr(IDS) if isinstance(groups, str) else groups, obs, obs_index, frame, eye_shift)


def undecidable(d, poly, obs, ray_len, frame=0, **kw):
    """bool [b,2,32]: the float64 value of the ray moves by more than EGO_FLOOR when the eye is shifted by SHIFT along +-x or +-y."""
    base = observe_case(d, poly, obs, ray_len, 0, 1, torch.float64, frame=frame, **kw)[1].double()
    out = torch.zeros_like(base, dtype=torch.bool)
    for sx, sy in ((ref.SHIFT, 0.0), (-ref.SHIFT, 0.0), (0.0, ref.SHIFT), (0.0, -ref.SHIFT)):
        out |= (observe_case(d, poly, obs, ray_len, 0, 1, torch.float64, frame=frame, eye_shift=(sx, sy), **kw)[1].double() - base).abs() > ref.EGO_FLOOR
    return out


def case_frame(kind, N, mode):
    """the absolute frame a ray case is run at: the cases between them cover FRAMES"""
    return FRAMES[(ref.OBSERVE_CASES.index((kind, N, mode))) % len(FRAMES)]


PEOPLE_CASES = ref.OBSERVE_CASES
