"""The marker model of recorded tracks (`generate_sequence_to_goal(obstacles=, obstacle_model="markers")`: entry
egx_obstacle_marker_clearance of csrc/genop_obstacle_markers.hip, and the obstacle phase of the *_obstacle_markers selection entries of
csrc/genop.hip on its table) restated on the CPU, the yardsticks of tests/test_genop_obstacle_markers_{cpu,gpu}.py.  The inputs are
taken as the float32 values the device reads.

Two restatements of the frame clearance c[r, f] = sqrt(min over the live tracks and the 67 x 67 marker pairs of the squared distance
of row r at predicted frame f + 2 and a track at absolute frame clamp(frame0 + 2 + f, 0, T - 1)) - skin:

  * `frame_clearance32`: numpy float32 with exactly the roundings include/egogen_hip.h states, so the device must give the same
    bits.  numpy rounds every float32 operation on its own (no contraction); the three fused multiply-adds of a world marker and the
    one of the blend are `fma32`, exact: the product of two float32 is exact in float64, the sum with the addend is rounded to odd in
    float64 (TwoSum tells which way the exact sum lies), and 53 >= 2 * 24 + 2 bits make the final rounding to float32 the rounding
    of the exact value.
  * `frame_clearance64`: brute force in float64 - the world markers of tests/genop_joint_markers_ref.world_markers (plain float64
    arithmetic, no fma), every distance by its norm.

Everything after c_t is the cylinder phase's: `terms_of_clearance` states it (float32: the fixed tree of the wave reduction, lane f
holding frame f, partners 32, 16, 8, 4, 2, 1 lanes up), and `apply` / `select` / `beam_select` of tests/genop_obstacles_ref.py take it
from there.  `apply_rows` feeds `apply` with rows the device scored (cost, terms, colliding of a launch without obstacles, and the
beam's q of every row), so that what the marker entries add is compared bit for bit."""
import numpy as np
import torch

from tests import genop_joint_markers_ref as mref
from tests import genop_obstacles_ref as oref
from tests import genop_search_ref as sref

NF, NMK = 18, 67
MAX_OBSTACLES = 32
f32 = np.float32


def _a(t, dtype=np.float32):
    return np.asarray(t.detach().cpu() if torch.is_tensor(t) else t, dtype)


def fma32(a, b, c):
    """fmaf(a, b, c) of float32 arrays, correctly rounded (see the module docstring)"""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b                                   # exact: 24 + 24 bits
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)             # exact sum = s + err (TwoSum)
        bits = np.ascontiguousarray(np.broadcast_to(s, np.broadcast(s, err).shape)).view(np.int64)
        up = (err > 0) == (s > 0)                   # the exact sum lies further from zero than s
        odd = np.where((bits & 1) == 1, bits, np.where(up, bits + 1, bits - 1)).view(np.float64)
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & (s != 0)
        return np.where(fix, odd, s).astype(np.float32)


def world_markers32(R0, T0, mp, Y_gen, rf):
    """R0 [rows,3,3], T0 [rows,3], mp [rows,20,67,3], Y_gen [18,rows,201] -> [rows,18,67,3] float32: egx_world_marker's roundings"""
    R0, T0, mp, Y_gen = _a(R0), _a(T0), _a(mp), _a(Y_gen)
    rows = mp.shape[0]
    proj = mp.reshape(rows, 20, NMK, 3)[:, 2:]
    pred = Y_gen.reshape(NF, rows, NMK, 3).transpose(1, 0, 2, 3)
    rf = f32(rf)
    with np.errstate(invalid="ignore", over="ignore"):
        m = fma32(rf, proj, (f32(1) - rf) * pred)
        R = R0.reshape(rows, 1, 1, 3, 3)
        out = [fma32(R[..., c, 2], m[..., 2], fma32(R[..., c, 1], m[..., 1], R[..., c, 0] * m[..., 0])) + T0.reshape(rows, 1, 1, 3)[..., c]
               for c in range(3)]
    return np.stack(out, -1).astype(np.float32)


def world_markers64(R0, T0, mp, Y_gen, rf):
    """the same in plain float64 (tests/genop_joint_markers_ref.world_markers) -> numpy [rows,18,67,3]"""
    t = lambda v: torch.as_tensor(_a(v))
    return mref.world_markers(t(R0), t(T0), t(mp), t(Y_gen), rf, torch.float64).numpy()


def frames_of(frame0, T):
    """absolute frame of every predicted frame f: clamp(frame0 + 2 + f, 0, T - 1)"""
    return np.clip(int(frame0) + 2 + np.arange(NF, dtype=np.int64), 0, int(T) - 1)


def _clearance(world, obs_markers, count, set_of_row, frame0, skin, dt, square):
    world, obs = np.asarray(world, dt), np.asarray(obs_markers, dt)
    S, O_max, T = obs.shape[:3]
    count, set_of_row = np.asarray(count).reshape(-1), np.asarray(set_of_row).reshape(-1)
    a = frames_of(frame0, T)
    rows = world.shape[0]
    out = np.full((rows, NF), np.inf, dt)
    skin = dt(f32(skin))
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(rows):
            s = int(min(max(set_of_row[r], 0), S - 1))
            n = int(min(max(count[s], 0), min(O_max, MAX_OBSTACLES)))
            bad = ~np.isfinite(world[r]).all(-1).all(-1)                             # [18]
            if n:
                track = obs[s, :n][:, a]                                             # [n,18,67,3]
                d2 = square(world[r][None, :, :, None, :], track[:, :, None, :, :])  # [n,18,67,67]
                d2 = np.where(np.isnan(d2), dt(np.inf), d2)                          # fminf drops a NaN
                out[r] = np.sqrt(d2.transpose(1, 0, 2, 3).reshape(NF, -1).min(1)) - skin
            out[r, bad] = np.nan
    return out


def frame_clearance32(world, obs_markers, count, set_of_row, frame0, skin):
    """world [rows,18,67,3] float32 (`world_markers32`), obs_markers [S,O_max,T,67,3], count [S], set_of_row [rows] -> [rows,18] float32
    with the device's roundings: three rounded differences, three rounded squares, (dx^2 + dy^2) + dz^2, the root of the least, - skin"""
    def square(w, o):
        d = w - o
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    return _clearance(world, obs_markers, count, set_of_row, frame0, skin, np.float32, square)


def frame_clearance64(world, obs_markers, count, set_of_row, frame0, skin):
    """the same by brute force in float64: every distance a norm"""
    return _clearance(world, obs_markers, count, set_of_row, frame0, skin, np.float64, lambda w, o: np.linalg.norm(w - o, axis=-1) ** 2)


def wave_sum32(v):
    """lane 0 of the selection kernels' wave_sum on [rows,18] float32 values held by lanes 0..17 of a wave of 64 (the rest 0)"""
    lanes = np.zeros(v.shape[:-1] + (64,), np.float32)
    lanes[..., :v.shape[-1]] = v
    with np.errstate(invalid="ignore", over="ignore"):
        for o in (32, 16, 8, 4, 2, 1):
            lanes = np.concatenate([lanes[..., :64 - o] + lanes[..., o:], lanes[..., 64 - o:]], -1)     # what lane 0 ends with reads in range only
    return lanes[..., 0]


def terms_of_clearance(c, margin, dtype=torch.float32):
    """c [rows,18] -> dict of [rows] torch tensors as tests/genop_obstacles_ref.row_terms returns them: clearance = min_f c, term =
    (sum_f max(0, margin - c)) / 18, hit = clearance < 0; a NaN frame makes term and clearance NaN, and no hit.  float32: the
    device's roundings and summation tree."""
    npdt = np.float32 if dtype == torch.float32 else np.float64
    c = np.asarray(c, npdt)
    m = npdt(f32(margin))
    with np.errstate(invalid="ignore", over="ignore"):
        pen = np.where(np.isnan(c), c, np.maximum(npdt(0), m - c))
        total = wave_sum32(pen) if npdt is np.float32 else pen.sum(-1)
        term = total / npdt(NF)
        clearance = np.where(np.isnan(c).any(-1), npdt(np.nan), np.where(np.isnan(c), npdt(np.inf), c).min(-1))
    return {"clearance": torch.as_tensor(clearance), "term": torch.as_tensor(term), "hit": torch.as_tensor(clearance < 0)}


def apply_rows(cost, terms, colliding, ob, w_obs, q=None):
    """tests/genop_obstacles_ref.apply on rows the device scored without obstacles - cost [B], terms [B,5], colliding [B] of the plain
    or the field entry, float32 - and `ob` of `terms_of_clearance`; q [B]: the beam's q of every row as the device accumulates it (None:
    genop_beam_ref.q_of of the terms).  The obstacle phase adds one rounded product to the cost and to q, and the hit to colliding."""
    cost, terms = torch.as_tensor(cost).reshape(-1), torch.as_tensor(terms).reshape(-1, 5)
    r = {t: terms[:, k] for k, t in enumerate(sref.TERMS)}
    r.update(cost=cost, colliding=torch.as_tensor(colliding).reshape(-1).bool())
    a = oref.apply(r, ob, w_obs, cost.dtype)
    if q is not None:
        a["q"] = torch.as_tensor(q).reshape(-1) + torch.tensor(w_obs, dtype=torch.float32).to(cost.dtype) * ob["term"]
    return a


select, beam_select = oref.select, oref.beam_select
