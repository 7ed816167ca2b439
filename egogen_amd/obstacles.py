"""`MovingObstacles`: other people as moving obstacles of `GAMMAPrimitiveComboGenOP.generate_sequence_to_goal` (`obstacles=`,
entries egx_primitive_select_obstacles / egx_primitive_beam_select_obstacles of csrc/genop.hip; with `obstacle_model="markers"`
egx_obstacle_marker_clearance of csrc/genop_obstacle_markers.hip and the *_obstacle_markers selection entries).

S sets of up to `MAX_OBSTACLES` tracks; S is 1 (every sequence avoids the same people) or b (one set per sequence), or any number
with an `index` [b] that names the set of each sequence.  A track is a world-frame xy position per absolute frame (40 fps, frame 0
= the first frame of the search's first primitive unless `obstacle_frame0` says otherwise) and a radius in metres: a person is a
vertical cylinder, z is ignored.  Outside [0, T-1] the frame index is clamped: before its track starts an obstacle stands at its
first position, after the end it stays where it stopped.  Optionally a track also carries the person's 67 world markers per frame
(`markers`, the same frames and the same clamping): what the marker model of recorded tracks reads instead of the cylinder.

The constructors validate on the host and keep numpy arrays; the device tensors are made by `.to(device)` or at first use, so
argument errors need no device."""
from __future__ import annotations

import pickle
from typing import Optional

import numpy as np
import torch

MAX_OBSTACLES = 32      # EGX_MAX_OBSTACLES of include/egogen_hip.h: the 18-frame window of a set must fit one workgroup's LDS
T_ALL, T_HIS = 20, 2
N_MARKERS = 67
OBSTACLE_MARKERS_CAP_BYTES = 1 << 30     # of the markers array, S * O_max * T * 804 bytes: a stated choice (a set of 32 people over
                                         # 10 minutes at 40 fps is 0.6 GB); above it the constructor raises on the host


def _np(x, dtype=np.float64):
    return np.asarray(x.detach().cpu() if torch.is_tensor(x) else x, dtype)


def _hold(tracks, T):
    """tracks: list of [t_i,...] -> [len,T,...], each held at its last position"""
    out = np.zeros((len(tracks), T) + tracks[0].shape[1:], np.float64)
    for o, tr in enumerate(tracks):
        out[o, :len(tr)] = tr
        out[o, len(tr):] = tr[-1]
    return out


class MovingObstacles:
    """xy [S,O_max,T,2] float32, radius [S,O_max] float32, count [S] int32 (live tracks of each set; the rest is padding),
    index [b] int32 or None, markers [S,O_max,T,67,3] float32 world markers or None.  `len()` is S."""

    def __init__(self, xy, radius, count, index=None, markers=None):
        self.xy, self.radius, self.count, self.index, self.markers = xy, radius, count, index, markers
        self.device = None          # set by .to(): where the tensors below live
        self._dev = None

    def __len__(self):
        return self.xy.shape[0]

    @property
    def max_obstacles(self):
        return self.xy.shape[1]

    @property
    def num_frames(self):
        return self.xy.shape[2]

    # ------------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_tracks(cls, xy, radius=0.3, index=None, markers=None) -> "MovingObstacles":
        """xy: [O,T,2] (one set) or a list of S such arrays (O may differ from set to set, and may be 0; T is shared).  radius: one
        number, [O] for one set, or a list of S such.  index: None or [b] ints in [0,S), the set of each sequence.  markers: None, or
        [O,T,67,3] world markers (one set) or a list of S such arrays, O and T of every set those of its xy.  ValueError for
        non-finite values (float32 overflow included), radius <= 0, O > 32, T < 1, an index outside [0,S), markers of another shape
        than their xy and a markers array above OBSTACLE_MARKERS_CAP_BYTES."""
        sets = [xy] if not isinstance(xy, (list, tuple)) else list(xy)
        if not sets:
            raise ValueError("from_tracks needs at least one set")
        sets = [_np(a) for a in sets]
        for a in sets:
            if a.ndim != 3 or a.shape[2] != 2:
                raise ValueError(f"a set of tracks must be [O,T,2], got {tuple(a.shape)}")
        T = sets[0].shape[1]
        if T < 1:
            raise ValueError("a track needs at least one frame (T >= 1)")
        if any(a.shape[1] != T for a in sets):
            raise ValueError(f"the sets of a call share T, got {[a.shape[1] for a in sets]}")
        S, O_max = len(sets), max(1, max(a.shape[0] for a in sets))
        if O_max > MAX_OBSTACLES:
            raise ValueError(f"a set holds at most {MAX_OBSTACLES} tracks, got {O_max}")
        radii = list(radius) if isinstance(radius, (list, tuple)) and S > 1 else [radius] * S
        if len(radii) != S:
            raise ValueError(f"radius must be one number or one entry per set ({S}), got {len(radii)}")
        out_xy, out_r = np.zeros((S, O_max, T, 2), np.float32), np.ones((S, O_max), np.float32)
        count = np.zeros(S, np.int32)
        for s, a in enumerate(sets):
            O = a.shape[0]
            if not np.isfinite(a).all():
                raise ValueError(f"set {s} holds a non-finite position")
            try:
                r = np.broadcast_to(_np(radii[s]), (O,))
            except ValueError:
                raise ValueError(f"radius of set {s} must be one number or [{O}], got shape {_np(radii[s]).shape}") from None
            if not (np.isfinite(r).all() and (r > 0).all()):
                raise ValueError(f"radius must be positive and finite, got {np.asarray(r).tolist() if O else radii[s]}")
            out_xy[s, :O], out_r[s, :O], count[s] = a, r, O
        if not np.isfinite(out_xy).all():
            raise ValueError("a position overflows float32")
        if index is not None:
            index = _np(index, np.int64).reshape(-1)
            if index.size < 1 or index.min() < 0 or index.max() >= S:
                raise ValueError(f"index must lie in [0, {S}), got {index.tolist()}")
            index = index.astype(np.int32)
        return cls(out_xy, out_r, count, index, cls._checked_markers(markers, sets, O_max))

    @staticmethod
    def _checked_markers(markers, sets, O_max):
        """the `markers` argument of `from_tracks` against the sets of xy -> [S,O_max,T,67,3] float32 (None without)"""
        if markers is None:
            return None
        mk = [markers] if not isinstance(markers, (list, tuple)) else list(markers)
        if len(mk) != len(sets):
            raise ValueError(f"markers must hold one array per set ({len(sets)}), got {len(mk)}")
        S, T = len(sets), sets[0].shape[1]
        nbytes = S * O_max * T * N_MARKERS * 3 * 4
        if nbytes > OBSTACLE_MARKERS_CAP_BYTES:
            raise ValueError(f"the markers of the obstacles would take {nbytes} bytes ({S} sets x {O_max} tracks x {T} frames x 804), above "
                             f"the cap of {OBSTACLE_MARKERS_CAP_BYTES}: fewer or shorter tracks, or the cylinder model")
        out = np.zeros((S, O_max, T, N_MARKERS, 3), np.float32)
        for s, (m, a) in enumerate(zip(mk, sets)):
            m = _np(m)
            if m.shape != a.shape[:2] + (N_MARKERS, 3):
                raise ValueError(f"the markers of set {s} must be {a.shape[:2] + (N_MARKERS, 3)} like its xy, got {tuple(m.shape)}")
            if not np.isfinite(m).all():
                raise ValueError(f"set {s} holds a non-finite marker")
            with np.errstate(over="ignore"):
                out[s, :m.shape[0]] = m
        if not np.isfinite(out).all():
            raise ValueError("a marker overflows float32")
        return out

    @staticmethod
    def _check_radius_start(radius, start_frame=0):
        if not (np.isfinite(radius) and radius > 0):
            raise ValueError(f"radius must be positive and finite, got {radius}")
        if int(start_frame) < 0:
            raise ValueError(f"start_frame must not be negative, got {start_frame}")

    @classmethod
    def from_sequences(cls, seqs, radius=0.3, start_frame=0, markers=False) -> "MovingObstacles":
        """seqs: a `PrimitiveSequence` (numpy or torch) or a list of them; every sequence i of every result becomes one track of ONE
        set.  World pelvis = rotmat[k,i] @ pelvis[k,i,t] + transl[k,i] (float64, rounded once); primitive 0 contributes its frames
        0..19, primitive k > 0 its frames 2..19 (frames 0 and 1 are the seed: frames 18 and 19 of primitive k - 1, which
        `utils.rollout_primitives` drops too), so frame t of primitive k is absolute frame 18 k + t.  A track stops after
        n_valid[i] primitives where the result has n_valid; shorter tracks are held at their last position.  start_frame >= 0: the
        absolute frame of the tracks' first frame (the obstacles stand at their first position before it).  markers=True: the tracks
        also carry the world markers rotmat[k,i] @ markers[k,i,t,a] + transl[k,i] of the same frames (float64, rounded once: what
        egx_crowd_metrics makes of the same records), held and started like the positions."""
        cls._check_radius_start(radius, start_frame)
        seqs = list(seqs) if isinstance(seqs, (list, tuple)) else [seqs]
        tracks, clouds = [], ([] if markers else None)
        for q in seqs:
            R, p, t = _np(q.rotmat), _np(q.pelvis), _np(q.transl)
            if R.ndim != 4 or p.ndim != 4 or p.shape[2] != T_ALL or R.shape[:2] != p.shape[:2] or t.shape != p.shape[:2] + (3,):
                raise ValueError(f"a sequence needs rotmat [K,b,3,3], pelvis [K,b,20,3] and transl [K,b,3], got {R.shape} / {p.shape} / {t.shape}")
            K, b = p.shape[:2]
            n_valid = np.full(b, K) if getattr(q, "n_valid", None) is None else _np(q.n_valid, np.int64).reshape(b)
            world = np.einsum("kbij,kbtj->kbti", R, p) + t[:, :, None, :]            # [K,b,20,3]
            for i in range(b):
                n = int(min(max(n_valid[i], 1), K))
                tracks.append(np.concatenate([world[k, i, (0 if k == 0 else T_HIS):, :2] for k in range(n)], 0))
            if markers:
                m = _np(q.markers)
                if m.shape != (K, b, T_ALL, N_MARKERS, 3):
                    raise ValueError(f"a sequence needs markers [K,b,20,67,3] for markers=True, got {m.shape}")
                for i in range(b):
                    n = int(min(max(n_valid[i], 1), K))
                    clouds.append(np.concatenate([(np.einsum("ij,taj->tai", R[k, i], m[k, i]) + t[k, i])[(0 if k == 0 else T_HIS):]
                                                  for k in range(n)], 0))
        return cls._one_set(tracks, radius, int(start_frame), clouds)

    @classmethod
    def from_rollout_files(cls, paths, radius=0.3, markers=False) -> "MovingObstacles":
        """The same from the `motion` lists of `motion_*.pkl` files (`PrimitiveSequence.save`, `utils.save_rollout_results`), one
        track per file in ONE set: reads pelvis_loc, transf_rotmat, transf_transl and mp_type of every primitive; a primitive after
        the first drops its two seed frames, one where its mp_type is '1-frame'.  markers=True: also blended_marker of every
        primitive, as `from_sequences(markers=True)` takes the markers."""
        cls._check_radius_start(radius)
        paths = [paths] if isinstance(paths, (str, bytes)) or hasattr(paths, "__fspath__") else list(paths)
        tracks, clouds = [], ([] if markers else None)
        for path in paths:
            with open(path, "rb") as fh:
                motion = pickle.load(fh).get("motion")
            if not motion:
                raise ValueError(f"{path} holds no motion primitives")
            chunks, mchunks = [], []
            for k, mp in enumerate(motion):
                R, t, p = _np(mp["transf_rotmat"]).reshape(3, 3), _np(mp["transf_transl"]).reshape(3), _np(mp["pelvis_loc"]).reshape(-1, 3)
                drop = 0 if k == 0 else (1 if mp.get("mp_type") == "1-frame" else T_HIS)
                chunks.append((p @ R.T + t)[drop:, :2])
                if markers:
                    m = _np(mp["blended_marker"]).reshape(-1, N_MARKERS, 3)
                    if m.shape[0] != p.shape[0]:
                        raise ValueError(f"{path}: primitive {k} holds {m.shape[0]} frames of markers and {p.shape[0]} of the pelvis")
                    mchunks.append((np.einsum("ij,taj->tai", R, m) + t)[drop:])
            tracks.append(np.concatenate(chunks, 0))
            if markers:
                clouds.append(np.concatenate(mchunks, 0))
        return cls._one_set(tracks, radius, 0, clouds)

    @classmethod
    def _one_set(cls, tracks, radius, start_frame, clouds=None):
        if not tracks:
            raise ValueError("no sequence to take a track from")
        start = lambda trs: [np.concatenate([np.repeat(tr[:1], start_frame, 0), tr], 0) for tr in trs] if start_frame else trs
        T = max(len(tr) for tr in tracks) + start_frame
        return cls.from_tracks(_hold(start(tracks), T), radius, markers=None if clouds is None else _hold(start(clouds), T))

    # ------------------------------------------------------------------------------------------------------------------
    def to(self, device) -> "MovingObstacles":
        """The tensors on `device` (made once per device); returns self."""
        t = lambda a, dt: None if a is None else torch.as_tensor(a, dtype=dt).to(torch.device(device)).contiguous()
        d = {"xy": t(self.xy, torch.float32), "radius": t(self.radius, torch.float32), "count": t(self.count, torch.int32),
             "index": t(self.index, torch.int32), "markers": t(self.markers, torch.float32)}
        self._dev, self.device = d, d["xy"].device
        return self

    def select_args(self, b: int):
        """The obstacle arguments of the two *_obstacles selection entries from obs_xy to num_frames for b sequences, and what must
        outlive the launches.  ValueError unless there are 1 or b sets, or an index of b entries."""
        from . import _lib
        if self._dev is None:
            raise ValueError("the obstacles are on no device yet: .to(device) first")
        S, d = len(self), self._dev
        index = d["index"]
        if index is not None:
            if index.numel() != b:
                raise ValueError(f"the index of `obstacles` names the set of {index.numel()} sequences, the search has {b}")
        elif S == b and S > 1:
            index = torch.arange(b, device=self.device, dtype=torch.int32)
        elif S != 1:
            raise ValueError(f"obstacles must hold 1 or {b} sets, got {S}")
        return (_lib.ptr(d["xy"]), _lib.ptr(d["radius"]), _lib.ptr(d["count"]), _lib.ptr(index), S, self.max_obstacles, self.num_frames), \
            (d, index)

    def marker_args(self, b: int):
        """The obstacle arguments of egx_obstacle_marker_clearance from obs_markers to num_frames for b sequences, and what must outlive
        the launches.  ValueError as `select_args`, and where the obstacles carry no markers."""
        from . import _lib
        if self.markers is None:
            raise ValueError("the obstacles carry no markers: build them with markers=True (from_sequences, from_rollout_files) or "
                             "from_tracks(..., markers=)")
        sel, alive = self.select_args(b)
        return (_lib.ptr(self._dev["markers"]), sel[2], sel[3], *sel[4:]), alive
