"""Measuring finished motions: what `generate_sequence_to_goal` and the env write, judged after the fact.

`MotionSet` stacks the records of n motions - the primitives of `PrimitiveSequence`s or of `motion_*.pkl` files - and the frame
table that makes each motion one run of frames: primitive 0 contributes its frames 0..19, a later '2-frame' primitive its frames
2..19, a later '1-frame' primitive 1..19 (the rule of `MovingObstacles.from_rollout_files` and `utils.rollout_primitives`).  It is
built on the host and needs no device.  `motion_metrics` gives the per-motion figures of `COLUMNS` (entry egx_motion_metrics),
`crowd_metrics` the person-to-person figures of the people of one scene and time line (entry egx_crowd_metrics), `route_metrics`
whether a motion followed its route of waypoints (entry egx_route_metrics); the kernels are
csrc/motion_metrics.hip, float64 from the float32 records, deterministic, and their definitions are written out in
include/egogen_hip.h.  Like the rest of the product path there is no CPU fallback: without the library or a device both raise
`EgxError`.  (tests/motion_metrics_ref.py is the numpy float64 restatement the kernels are tested against.)

What the figures are NOT: a perceptual score.  They are the reward's own skate and floor arguments carried across hand-offs,
smoothness of the pelvis track, goal attainment, scene penetration counts of the body model's vertices, and between people the
search's cylinder clearance next to a marker-to-marker distance (which the search sees only with `pair_model="markers"`).  The contact score's constants (a 5 cm band,
0.075 m/s) are GAMMA's, and `touch_dist` (5 cm between two people's markers) is a stated choice."""
from __future__ import annotations

import ctypes as C
import os
import pickle
import re
from typing import Optional

import numpy as np
import torch

from . import _lib
from .route import MAX_WAYPOINTS

T_ALL, T_HIS, NMK, XB = 20, 2, 67, 93
FPS = 40.0
MAX_GROUP = 32                  # EGX_MAX_GROUP of include/egogen_hip.h
LBS_CHUNK = 10240 // T_ALL      # primitives per body-model launch: 10 240 bodies

# name, unit, table ("f64" / "i32"), meaning: the order within a table is the column order of include/egogen_hip.h (EGX_MM_*)
COLUMNS = (
    ("duration_s", "s", "f64", "(frames - 1) / 40"),
    ("skate_mean", "m/s", "f64", "mean over the interior frames of max(s_f - 0.075, 0), s_f the slowest feet marker's central-difference speed"),
    ("skate_speed_mean", "m/s", "f64", "mean s_f"),
    ("skate_speed_max", "m/s", "f64", "max s_f"),
    ("floor_mean", "m", "f64", "mean |h_f - 0.02|, h_f the lowest feet marker above floor_z"),
    ("floor_min", "m", "f64", "min h_f (negative: below the floor)"),
    ("floor_max", "m", "f64", "max h_f (floating)"),
    ("contact_score", "1", "f64", "mean exp(-max(|h_f| - 0.05, 0)) exp(-max(s_f - 0.075, 0)): 1 is a planted foot on every frame"),
    ("path_length", "m", "f64", "summed xy steps of the pelvis"),
    ("displacement", "m", "f64", "xy distance from the first to the last pelvis"),
    ("speed_mean", "m/s", "f64", "path_length / duration_s"),
    ("acc_mean", "m/s^2", "f64", "1600 mean |p_{f+1} - 2 p_f + p_{f-1}|"),
    ("jerk_mean", "m/s^3", "f64", "64000 mean |p_{f+2} - 3 p_{f+1} + 3 p_f - p_{f-1}|"),
    ("goal_dist_end", "m", "f64", "3-D distance pelvis to goal on the last frame (NaN without a goal)"),
    ("goal_dist_min", "m", "f64", "the least such distance along the motion"),
    ("pene_mean", "vertices", "f64", "mean per frame of the body's vertices inside the scene (NaN without a scene)"),
    ("frames", "frames", "i32", "frames of the motion at 40 per second"),
    ("skate_frames", "frames", "i32", "frames with s_f > 0.075"),
    ("first_reached_frame", "frame", "i32", "first frame within goal_thresh of the goal, -1 if none"),
    ("pene_max", "vertices", "i32", "largest per-frame count (-1 without a scene)"),
    ("pene_frames", "frames", "i32", "frames with at least pene_thres vertices inside (-1 without a scene)"),
)
F64_COLUMNS = tuple(c[0] for c in COLUMNS if c[2] == "f64")
I32_COLUMNS = tuple(c[0] for c in COLUMNS if c[2] == "i32")
FRAME_COLUMNS = ("s", "h", "c", "d", "pelvis_x", "pelvis_y")       # the per-frame output (EGX_MM_FRAME_COLS)
GOAL_COLUMNS = ("goal_dist_end", "goal_dist_min", "first_reached_frame")
_NAME = re.compile(r"^motion_(.+)_([^_]+)_p(\d+)\.pkl$")


def _np(x, dtype=np.float32):
    return np.ascontiguousarray(np.asarray(x.detach().cpu() if torch.is_tensor(x) else x), dtype)


def groups_from_file_names(paths) -> np.ndarray:
    """[n] group ids: files named motion_<seed>_<variant>_p<person>.pkl (what gen_motion.py --people writes) are one group per
    (seed, variant), in order of first appearance; every other file is a group of its own."""
    keys, ids = {}, []
    for i, p in enumerate(paths):
        m = _NAME.match(os.path.basename(os.fspath(p)))
        key = (m.group(1), m.group(2)) if m else ("", i)
        ids.append(keys.setdefault(key, len(keys)))
    return np.asarray(ids, np.int64)


class MotionSet:
    """n motions of P primitives in all.  markers [P,20,67,3], pelvis [P,20,3], rotmat [P,3,3], transl [P,3], params [P,20,93],
    betas [P,10] (float32, the primitives of motion 0 first); prim_start [n+1] the primitives of each motion; frame_src [Ftot] int32
    (primitive * 20 + t) and motion_start [n+1] int32 the frames of each motion; goals [n,3] float32 (a NaN row: no goal) or None;
    groups [n] ids or None; names [n]; routes: a list of n entries, [n_i,3] float32 (the waypoints of a motion generated with
    `route=`, at most 16) or None for a motion without a route, or None where no motion has one.  `len()` is n."""

    def __init__(self, markers, pelvis, rotmat, transl, params, betas, prim_start, mp_types, goals=None, groups=None, names=None,
                 routes=None):
        self.markers, self.pelvis, self.rotmat, self.transl = _np(markers), _np(pelvis), _np(rotmat), _np(transl)
        self.params, self.betas = _np(params), _np(betas)
        self.prim_start = np.asarray(prim_start, np.int64)
        P, n = self.markers.shape[0], len(self.prim_start) - 1
        if n < 1 or self.prim_start[0] != 0 or self.prim_start[-1] != P or (np.diff(self.prim_start) < 1).any():
            raise ValueError(f"every motion needs at least one primitive: prim_start {self.prim_start.tolist()} over {P} primitives")
        want = {"markers": (P, T_ALL, NMK, 3), "pelvis": (P, T_ALL, 3), "rotmat": (P, 3, 3), "transl": (P, 3), "params": (P, T_ALL, XB),
                "betas": (P, 10)}
        for k, shape in want.items():
            if getattr(self, k).shape != shape:
                raise ValueError(f"{k} must be {shape}, got {getattr(self, k).shape}")
            if k != "params" and k != "betas" and not np.isfinite(getattr(self, k)).all():
                raise ValueError(f"{k} holds a non-finite value")
        if len(mp_types) != P:
            raise ValueError(f"mp_types must name {P} primitives, got {len(mp_types)}")
        self.mp_types = list(mp_types)
        src, start = [], [0]
        for i in range(n):
            for k in range(int(self.prim_start[i]), int(self.prim_start[i + 1])):
                drop = 0 if k == self.prim_start[i] else (1 if self.mp_types[k] == "1-frame" else T_HIS)
                src.extend(range(k * T_ALL + drop, (k + 1) * T_ALL))
            start.append(len(src))
        self.frame_src, self.motion_start = np.asarray(src, np.int32), np.asarray(start, np.int32)
        self.goals = None
        if goals is not None:
            self.goals = _np(goals).reshape(-1, 3)
            if self.goals.shape[0] != n or np.isinf(self.goals).any():
                raise ValueError(f"goals must be [{n},3] without infinities, got {self.goals.shape}")
            if np.isnan(self.goals).all():
                self.goals = None
        self.groups = None
        if groups is not None:
            self.groups = np.asarray(groups.detach().cpu() if torch.is_tensor(groups) else groups).astype(np.int64).reshape(-1)
            if self.groups.shape[0] != n:
                raise ValueError(f"groups must hold {n} ids, got {self.groups.shape[0]}")
        self.names = [str(i) for i in range(n)] if names is None else [str(v) for v in names]
        if len(self.names) != n:
            raise ValueError(f"names must hold {n} entries, got {len(self.names)}")
        self.routes = None
        if routes is not None and any(r is not None for r in routes):
            if len(routes) != n:
                raise ValueError(f"routes must hold {n} entries, got {len(routes)}")
            self.routes = [None if r is None else _np(r).reshape(-1, 3) for r in routes]
            for r in self.routes:
                if r is not None and (not 1 <= len(r) <= MAX_WAYPOINTS or not np.isfinite(r).all()):
                    raise ValueError(f"a route holds 1 to {MAX_WAYPOINTS} finite waypoints, got {len(r)}")
        self._dev = None

    def __len__(self):
        return len(self.motion_start) - 1

    @property
    def frames(self) -> np.ndarray:
        return np.diff(self.motion_start)

    # ------------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_sequences(cls, seqs) -> "MotionSet":
        """seqs: a `PrimitiveSequence` (numpy or torch) or a list of them; every sequence i of every result becomes one motion of
        its first n_valid[i] primitives (all K where the result has no n_valid), every primitive '2-frame'.  The goal is
        `search["goal"][i]` of a goal-steered result; the `groups` of a joint result carry over (two results never share a
        group; a sequence of a result without groups is alone); so do the routes of a result searched with `route=`
        (`PrimitiveSequence.ROUTE_FIELDS`)."""
        seqs = list(seqs) if isinstance(seqs, (list, tuple)) else [seqs]
        if not seqs:
            raise ValueError("no sequence to measure")
        rec = {k: [] for k in ("markers", "pelvis", "rotmat", "transl", "params", "betas")}
        prim_start, goals, groups, names, any_group, next_group, routes = [0], [], [], [], False, 0, []
        for r, q in enumerate(seqs):
            try:
                mk, pl, R, t, pp, bt = (_np(getattr(q, k)) for k in ("markers", "pelvis", "rotmat", "transl", "params", "betas"))
            except AttributeError as e:
                raise ValueError(f"not a PrimitiveSequence: {e}") from None
            if mk.ndim != 5 or mk.shape[2:] != (T_ALL, NMK, 3):
                raise ValueError(f"a sequence needs markers [K,b,20,67,3], got {mk.shape}")
            K, b = mk.shape[:2]
            if pl.shape != (K, b, T_ALL, 3) or R.shape != (K, b, 3, 3) or t.shape != (K, b, 3) or pp.shape != (K, b, T_ALL, XB) or \
                    bt.shape != (b, 10):
                raise ValueError(f"records of a sequence disagree with markers [{K},{b},...]: {pl.shape} / {R.shape} / {t.shape} / "
                                 f"{pp.shape} / {bt.shape}")
            n_valid = np.full(b, K) if getattr(q, "n_valid", None) is None else _np(q.n_valid, np.int64).reshape(b)
            search = getattr(q, "search", None)
            goal = None if not search or search.get("goal") is None else _np(search["goal"]).reshape(b, 3)
            ids = getattr(q, "groups", None)
            ids = None if ids is None else _np(ids, np.int64).reshape(b)
            any_group |= ids is not None
            way = getattr(q, "route_waypoints", None)
            cnt = None if way is None else _np(q.route_count, np.int64).reshape(b)
            remap = {}
            for i in range(b):
                routes.append(None if way is None else _np(way)[i, :int(cnt[i])])
                n = int(min(max(n_valid[i], 1), K))
                for k, a in (("markers", mk), ("pelvis", pl), ("rotmat", R), ("transl", t), ("params", pp)):
                    rec[k].append(a[:n, i])
                rec["betas"].append(np.repeat(bt[i:i + 1], n, 0))
                prim_start.append(prim_start[-1] + n)
                goals.append(np.full(3, np.nan, np.float32) if goal is None else goal[i])
                key = ("alone", i) if ids is None else int(ids[i])
                if key not in remap:
                    remap[key] = next_group
                    next_group += 1
                groups.append(remap[key])
                names.append(f"{r}:{i}" if len(seqs) > 1 else str(i))
        rec = {k: np.concatenate(v, 0) for k, v in rec.items()}
        return cls(rec["markers"], rec["pelvis"], rec["rotmat"], rec["transl"], rec["params"], rec["betas"], prim_start,
                   ["2-frame"] * int(prim_start[-1]), goals, groups if any_group else None, names, routes)

    @classmethod
    def from_rollout_files(cls, paths, groups=None) -> "MotionSet":
        """The same from `motion_*.pkl` files (`PrimitiveSequence.save`, `utils.save_rollout_results`), one motion per file: reads
        blended_marker, smplx_params, betas, transf_rotmat, transf_transl, pelvis_loc and mp_type of every primitive; the goal is
        wpath[-1], as `PrimitiveSequence.save` writes it, and a wpath of more than two points is a route: wpath[1:].  A wpath that
        cannot be one (more than 16 points after the first, as a navmesh path may have, or a non-finite point) leaves the motion
        without a route; its other figures are measured as before.  groups: None, [n] ids, or "names" for `groups_from_file_names`."""
        paths = [paths] if isinstance(paths, (str, bytes)) or hasattr(paths, "__fspath__") else list(paths)
        if not paths:
            raise ValueError("no file to measure")
        rec = {k: [] for k in ("markers", "pelvis", "rotmat", "transl", "params", "betas")}
        prim_start, goals, types, routes = [0], [], [], []
        for path in paths:
            with open(path, "rb") as fh:
                node = pickle.load(fh)
            motion = node.get("motion") if isinstance(node, dict) else None
            if not motion:
                raise ValueError(f"{path} holds no motion primitives")
            try:
                for mp in motion:
                    rec["markers"].append(_np(mp["blended_marker"]).reshape(1, T_ALL, NMK, 3))
                    rec["pelvis"].append(_np(mp["pelvis_loc"]).reshape(1, T_ALL, 3))
                    rec["rotmat"].append(_np(mp["transf_rotmat"]).reshape(1, 3, 3))
                    rec["transl"].append(_np(mp["transf_transl"]).reshape(1, 3))
                    rec["params"].append(_np(mp["smplx_params"]).reshape(1, T_ALL, XB))
                    rec["betas"].append(_np(mp["betas"]).reshape(1, -1)[:, :10])
                    types.append(str(mp.get("mp_type", "2-frame")))
            except (KeyError, ValueError, TypeError) as e:
                raise ValueError(f"{path}: not a primitive of 20 frames and 67 markers: {e!r}") from None
            prim_start.append(prim_start[-1] + len(motion))
            wpath = node.get("wpath")
            goals.append(np.full(3, np.nan, np.float32) if wpath is None else _np(wpath).reshape(-1, 3)[-1])
            way = None if wpath is None else _np(wpath).reshape(-1, 3)[1:]
            routes.append(way if way is not None and 2 <= len(way) <= MAX_WAYPOINTS and np.isfinite(way).all() else None)
        rec = {k: np.concatenate(v, 0) for k, v in rec.items()}
        if isinstance(groups, str):
            if groups != "names":
                raise ValueError(f'groups must be None, ids or "names", got {groups!r}')
            groups = groups_from_file_names(paths)
        return cls(rec["markers"], rec["pelvis"], rec["rotmat"], rec["transl"], rec["params"], rec["betas"], prim_start, types, goals,
                   groups, [os.fspath(p) for p in paths], routes)

    # ------------------------------------------------------------------------------------------------------------------
    def to(self, device) -> dict:
        """The records and the frame table on `device` (made once per device) -> dict of tensors."""
        device = torch.device(device)
        if self._dev is None or self._dev["device"] != device:
            t = lambda a: torch.from_numpy(a).to(device).contiguous()
            self._dev = {"device": device, **{k: t(getattr(self, k)) for k in ("markers", "pelvis", "rotmat", "transl", "params", "betas",
                                                                                 "frame_src", "motion_start")},
                         "goals": None if self.goals is None else t(self.goals)}
        return self._dev

    def lead_args(self, d):
        """The ten leading arguments of both entries, and what must outlive the call."""
        host = np.ascontiguousarray(self.motion_start, np.int32)
        return (_lib.ptr(d["markers"]), _lib.ptr(d["pelvis"]), _lib.ptr(d["rotmat"]), _lib.ptr(d["transl"]), int(self.markers.shape[0]),
                _lib.ptr(d["frame_src"]), int(self.frame_src.shape[0]), _lib.ptr(d["motion_start"]), host.ctypes.data_as(_lib.c_int_p),
                len(self)), host


def _device():
    if not torch.cuda.is_available():
        raise _lib.EgxError("no HIP device visible - the motion metrics have no CPU fallback")
    _lib.load()
    return torch.device("cuda", torch.cuda.current_device())


def _motion_set(motions) -> MotionSet:
    return motions if isinstance(motions, MotionSet) else MotionSet.from_sequences(motions)


def pene_counts(motions: MotionSet, scene, body_model, agent_scene=None) -> torch.Tensor:
    """[P*20] int32 on the device: the vertices of every recorded body inside `scene`, from batched `BodyModelHandle.forward`s
    over all primitives (frames_per_agent = 20, R0 / T0 the primitives' world frames), at most 10 240 bodies per launch - the path
    the search itself uses.  agent_scene [n]: the scene of each motion, with an `SdfSceneSet`."""
    dev = _device()
    d = motions.to(dev)
    P = motions.markers.shape[0]
    prim_scene = None
    if agent_scene is not None:
        idx = torch.as_tensor(agent_scene).reshape(-1).to("cpu", torch.int64)
        if idx.numel() != len(motions):
            raise ValueError(f"agent_scene must hold {len(motions)} indices, one per motion, got {idx.numel()}")
        prim_scene = idx.repeat_interleave(torch.as_tensor(np.diff(motions.prim_start))).to(dev, torch.int32)
    out = torch.empty(P * T_ALL, device=dev, dtype=torch.int32)
    for c0 in range(0, P, LBS_CHUNK):
        c1 = min(c0 + LBS_CHUNK, P)
        body_model.forward(d["params"][c0:c1].reshape(-1, XB), d["betas"][c0:c1], T_ALL, want_verts=False, want_joints=True,
                           want_markers=True, sdf=scene, R0=d["rotmat"][c0:c1], T0=d["transl"][c0:c1],
                           out={"pene_count": out[c0 * T_ALL:c1 * T_ALL]},
                           agent_scene=None if prim_scene is None else prim_scene[c0:c1])
    return out


def launch_motion_metrics(ms: MotionSet, goal_thresh, floor_z, pene_count, pene_thres, per_frame, use_goals=True):
    """One launch of egx_motion_metrics over all motions of `ms` on the current stream, no host wait -> the float64 table
    [n,len(F64_COLUMNS)], the int32 table [n,len(I32_COLUMNS)] and the per-frame table [Ftot,len(FRAME_COLUMNS)] (None unless
    per_frame), on the device.  pene_count: None or [P*20] int32 on the device; use_goals=False measures without the set's goals."""
    from . import synth
    dev = _device()
    d, n, Ftot = ms.to(dev), len(ms), int(ms.frame_src.shape[0])
    feet = (C.c_int32 * 6)(*[int(v) for v in synth.feet_marker_idx()])
    out_f = torch.empty(n, len(F64_COLUMNS), device=dev, dtype=torch.float64)
    out_i = torch.empty(n, len(I32_COLUMNS), device=dev, dtype=torch.int32)
    frames = torch.empty(Ftot, len(FRAME_COLUMNS), device=dev, dtype=torch.float64) if per_frame else None
    lead, _alive = ms.lead_args(d)
    _lib.check(_lib.load().egx_motion_metrics(*lead, feet, _lib.ptr(d["goals"] if use_goals else None), float(goal_thresh), float(floor_z),
                                              _lib.ptr(pene_count), int(pene_thres), _lib.ptr(out_f), _lib.ptr(out_i), _lib.ptr(frames),
                                              _lib.current_stream_ptr()), "egx_motion_metrics")
    return out_f, out_i, frames


def launch_crowd_metrics(ms: MotionSet, pg, body_radius, hold):
    """One launch of egx_crowd_metrics for the groups `pg` (a `PersonGroups` over the motions of `ms`) on the current stream, no
    host wait -> clearance [npairs,Fmax], marker_dist [npairs,Fmax] (float64, NaN where a pair is not compared), the pair list
    [npairs,2] int32, on the device, and pair_start [G+1] (numpy)."""
    dev = _device()
    d = ms.to(dev)
    sizes = pg.sizes.astype(np.int64)
    pair_start = np.concatenate([[0], np.cumsum(sizes * (sizes - 1) // 2)]).astype(np.int32)
    npairs, Fmax = int(pair_start[-1]), int(ms.frames.max())
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(dev)
    gs_host = np.ascontiguousarray(pg.start, np.int32)
    gs, gm, ps = i32(pg.start), i32(pg.member), i32(pair_start)
    clear = torch.full((npairs, Fmax), float("nan"), device=dev, dtype=torch.float64)
    mdist = torch.full((npairs, Fmax), float("nan"), device=dev, dtype=torch.float64)
    plist = torch.zeros(npairs, 2, device=dev, dtype=torch.int32)
    lead, _alive = ms.lead_args(d)
    _lib.check(_lib.load().egx_crowd_metrics(*lead, _lib.ptr(gs), _lib.ptr(gm), _lib.ptr(ps), gs_host.ctypes.data_as(_lib.c_int_p), len(pg),
                                             npairs, Fmax, float(body_radius), int(bool(hold)), _lib.ptr(clear), _lib.ptr(mdist),
                                             _lib.ptr(plist), _lib.current_stream_ptr()), "egx_crowd_metrics")
    return clear, mdist, plist, pair_start


def motion_metrics(motions, goal_thresh: Optional[float] = None, floor_z: float = 0.0, pene_thres: int = 40, scene=None, agent_scene=None,
                   body_model=None, per_frame: bool = False) -> dict:
    """The per-motion figures of `COLUMNS` -> dict of numpy arrays [n] keyed by column name (float64 / int32), from one launch of
    egx_motion_metrics over all motions.
        - motions: a `MotionSet`, or what `MotionSet.from_sequences` takes
        - goal_thresh: None is 0.1 m, the search's default; the goal columns of a motion without a goal are NaN / -1
        - floor_z: height of the floor in the world
        - scene: None (the pene columns are NaN / -1), an `SdfScene`, or an `SdfSceneSet` with agent_scene [n]; needs body_model, the
          `BodyModelHandle` of the motions' gender; the result then also holds "pene_count" [P*20], what `pene_counts` gave
        - pene_thres: a frame with that many vertices inside counts into pene_frames (40: the env's collision threshold)
        - per_frame: the result also holds "per_frame" [Ftot,6] float64 (`FRAME_COLUMNS`; NaN where undefined), "frame_src" and
          "motion_start"
    ValueError for a motion shorter than 4 frames, a negative threshold, a scene without a body model."""
    ms = _motion_set(motions)
    goal_thresh = 0.1 if goal_thresh is None else float(goal_thresh)
    if not (goal_thresh >= 0 and np.isfinite(goal_thresh)) or int(pene_thres) < 0 or not np.isfinite(float(floor_z)):
        raise ValueError(f"goal_thresh and pene_thres must not be negative and floor_z finite, got {goal_thresh}, {pene_thres}, {floor_z}")
    if int(ms.frames.min()) < 4:
        raise ValueError(f"a motion needs at least 4 frames, got {int(ms.frames.min())}")
    if scene is not None and body_model is None:
        raise ValueError("a scene needs body_model, the BodyModelHandle of the motions' gender")
    _device()
    pene = None if scene is None else pene_counts(ms, scene, body_model, agent_scene)
    out_f, out_i, frames = launch_motion_metrics(ms, goal_thresh, floor_z, pene, pene_thres, per_frame)
    of, oi = out_f.cpu().numpy(), out_i.cpu().numpy()
    res = {k: of[:, j].copy() for j, k in enumerate(F64_COLUMNS)}
    res.update({k: oi[:, j].copy() for j, k in enumerate(I32_COLUMNS)})
    if ms.goals is not None:          # a motion without a goal among motions with one
        none = np.isnan(ms.goals).any(1)
        res["goal_dist_end"][none], res["goal_dist_min"][none], res["first_reached_frame"][none] = np.nan, np.nan, -1
    if pene is not None:
        res["pene_count"] = pene.cpu().numpy()
    if per_frame:
        res.update(per_frame=frames.cpu().numpy(), frame_src=ms.frame_src.copy(), motion_start=ms.motion_start.copy())
    return res


def launch_route_metrics(ms: MotionSet, pass_radius):
    """One launch of egx_route_metrics over all motions of `ms` on the current stream, no host wait -> pass_frame [n,16] int32,
    approach_min [n,16] float64, waypoints_passed [n] int32, on the device.  A motion without a route has count 0."""
    dev = _device()
    d, n, P = ms.to(dev), len(ms), MAX_WAYPOINTS
    way, cnt = np.zeros((n, P, 3), np.float32), np.zeros(n, np.int32)
    for i, r in enumerate(ms.routes or []):
        if r is not None:
            way[i, :len(r)], cnt[i] = r, len(r)
    way_d, cnt_d = torch.from_numpy(way).to(dev), torch.from_numpy(cnt).to(dev)
    pass_frame = torch.empty(n, P, device=dev, dtype=torch.int32)
    approach = torch.empty(n, P, device=dev, dtype=torch.float64)
    passed = torch.empty(n, device=dev, dtype=torch.int32)
    lead, _alive = ms.lead_args(d)
    _lib.check(_lib.load().egx_route_metrics(*lead, _lib.ptr(way_d), _lib.ptr(cnt_d), P, float(pass_radius), _lib.ptr(pass_frame),
                                             _lib.ptr(approach), _lib.ptr(passed), _lib.current_stream_ptr()), "egx_route_metrics")
    return pass_frame, approach, passed


def route_metrics(motions, pass_radius: float = 0.5) -> dict:
    """Did every motion follow its route (`MotionSet.routes`): the ordered rule of the search's egx_route_advance at frame
    resolution over the whole motion, from one launch of egx_route_metrics -> dict of numpy arrays
        - pass_frame [n,16] int32: the frame at which waypoint j, not the last one, was first within pass_radius horizontally,
          searched from the pass frame of j - 1 on (frame 0 for j = 0); -1 where it never was, for the last waypoint (it is arrived
          at: `motion_metrics`' first_reached_frame), and on padding
        - approach_min [n,16] float64: the least horizontal distance to waypoint j from that start frame on; NaN where j - 1 was
          never passed and on padding
        - waypoints_passed [n] int32, and count [n] int32 the waypoints of each route
    A motion without a route gets -1 / NaN / 0.  pass_radius: 0.5 m is the search's default (`Routes`), a stated choice."""
    ms = _motion_set(motions)
    if not (float(pass_radius) >= 0 and np.isfinite(float(pass_radius))):
        raise ValueError(f"pass_radius must be finite and not negative, got {pass_radius}")
    pass_frame, approach, passed = launch_route_metrics(ms, pass_radius)
    count = np.asarray([0 if r is None else len(r) for r in (ms.routes or [None] * len(ms))], np.int32)
    return {"pass_frame": pass_frame.cpu().numpy(), "approach_min": approach.cpu().numpy(), "waypoints_passed": passed.cpu().numpy(),
            "count": count}


def crowd_metrics(motions, groups=None, body_radius: float = 0.3, touch_dist: float = 0.05, hold: bool = False) -> dict:
    """The person-to-person figures of the people who share a scene and a time line (every motion starts at absolute frame 0), from
    one launch of egx_crowd_metrics and torch reductions on the device.
        - groups: None takes the motions' own (`MotionSet.groups`; without any, everybody is alone and there is no pair), else [n]
          ids or a `PersonGroups`; at most 32 people per group
        - body_radius: the cylinder of the search's clearance model, clearance = |p_i - p_j|_xy - 2 body_radius
        - touch_dist: two people whose nearest markers are closer than this touch (0.05 m: a stated choice)
        - hold: False compares a pair on the frames both recorded; True lets a member that has ended stand at its last frame until
          the longest member of its group ends, as `MovingObstacles` holds a track
    -> {"clearance", "marker_dist": [npairs,Fmax] float64, NaN where a pair is not compared;
        "pair": {i, j, group, clearance_min, marker_dist_min, overlap_frames, touch_frames, frames_compared} [npairs];
        "person": {clearance_min, marker_dist_min, overlap_frames, touch_frames} [n] (+inf / 0 for somebody alone);
        "group": {id, size, frames_compared, clearance_min, marker_dist_min, overlap_frames, touch_frames} [G]}
    overlap_frames counts frames with clearance < 0, touch_frames frames with marker_dist < touch_dist; for a person or a group a
    frame counts once, whoever of the partners it is; frames_compared of a group: frames on which at least one pair was compared."""
    from .crowd import PersonGroups
    ms = _motion_set(motions)
    n = len(ms)
    if not (float(body_radius) >= 0 and np.isfinite(float(body_radius)) and float(touch_dist) >= 0 and np.isfinite(float(touch_dist))):
        raise ValueError(f"body_radius and touch_dist must be finite and not negative, got {body_radius}, {touch_dist}")
    if groups is None:
        groups = np.arange(n) if ms.groups is None else ms.groups
    pg = groups if isinstance(groups, PersonGroups) else PersonGroups.from_ids(groups, n)
    if len(pg.ids) != n:
        raise ValueError(f"groups must hold {n} ids, one per motion, got {len(pg.ids)}")
    dev = _device()
    G, sizes = len(pg), pg.sizes.astype(np.int64)
    clear, mdist, plist, pair_start = launch_crowd_metrics(ms, pg, body_radius, hold)
    npairs, Fmax = clear.shape
    inf = float("inf")
    pair_group = torch.repeat_interleave(torch.arange(G, device=dev), torch.as_tensor(np.diff(pair_start), device=dev).long())
    pi, pj = plist[:, 0].long(), plist[:, 1].long()
    compared = ~torch.isnan(clear)
    c_inf, m_inf = torch.where(compared, clear, inf), torch.where(compared, mdist, inf)

    def rows(index_sets, rows_out):
        """per-frame minima over the pairs that fall on each of `rows_out` rows -> the four figures and the frames compared"""
        cf = torch.full((rows_out, Fmax), inf, device=dev, dtype=torch.float64)
        mf = torch.full((rows_out, Fmax), inf, device=dev, dtype=torch.float64)
        for idx in index_sets:
            at = idx.view(-1, 1).expand(-1, Fmax)
            cf.scatter_reduce_(0, at, c_inf, "amin")
            mf.scatter_reduce_(0, at, m_inf, "amin")
        return {"clearance_min": cf.amin(1) if Fmax else cf.new_full((rows_out,), inf),
                "marker_dist_min": mf.amin(1) if Fmax else mf.new_full((rows_out,), inf),
                "overlap_frames": (cf < 0).sum(1).int(), "touch_frames": (mf < float(touch_dist)).sum(1).int(),
                "frames_compared": torch.isfinite(cf).sum(1).int()}
    pair = rows([torch.arange(npairs, device=dev)], npairs)
    person = rows([pi, pj], n)
    group = rows([pair_group], G)
    person.pop("frames_compared")
    to_np = lambda t: {k: v.cpu().numpy() for k, v in t.items()}
    pair, person, group = to_np(pair), to_np(person), to_np(group)
    pair.update(i=plist[:, 0].cpu().numpy(), j=plist[:, 1].cpu().numpy(), group=pair_group.cpu().numpy())
    first = pg.member[pg.start[:-1]]
    group.update(id=np.asarray(pg.ids)[first], size=sizes)
    return {"clearance": clear.cpu().numpy(), "marker_dist": mdist.cpu().numpy(), "pair": pair, "person": person, "group": group}
