"""The trained policy as the proposal distribution of the primitive search (`generate_sequence_to_goal(..., policy=)`,
egogen_amd/genop.py).  Per primitive and sequence: the observation the env would hand the policy after the chosen primitive
(entry egx_primitive_observe: canonical markers, marker -> goal directions, 32 egosensing rays against the walkable polygon, dist
and time; crowd_ppo/crowd_env_2f.py:311-312,524-613,680-727), the actor branch of the policy on it (egx_policy_forward,
crowd_ppo/ppo_policy.py:142-179), and the candidate latents from `mu, logvar` and the N(0, I) draws the search would have used
as they are (entry egx_policy_propose): `n_mean` rows are mu, the rows up to `n_policy` are samples round it, the rest stay the
prior's samples.  The search's selection then scores them like any other candidates.  With `sense_people=True` the observation is
the reference's crowd evaluation's: the sequence's group-mates and obstacle tracks are holes of the polygon (entries
egx_primitive_people_boxes and egx_primitive_observe_people; all four entries are csrc/genop_policy.hip).  Launches only: nothing here
waits for the device once `prepare` has run."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _lib

MAX_CANDIDATES = 256        # EGX_MAX_CANDIDATES of include/egogen_hip.h
POLICY_FIELDS = ("policy_mu", "policy_logvar", "obs_state", "obs_egosensing", "obs_dist", "obs_time", "policy_temperature",
                 "policy_n_mean", "policy_n_policy", "policy_ray_len", "policy_max_depth")
PEOPLE_FIELDS = ("people_box", "obs_people_count", "policy_sense_people")      # with sense_people; None, None, False without
NO_GROUPS, NO_OBSTACLES = (None, None, None, 0), (None, None, None, None, 0, 0, 0, 0)


def _vp(t):
    return C.c_void_p(t.data_ptr())


def check_beam(beam_width: int):
    """`policy=` is the greedy search only, as `groups=` is."""
    if int(beam_width) > 1:
        raise ValueError(f"policy= is the greedy search only: beam_width must be 1 with it, got {beam_width}")


def scene_file_edges(path: str) -> np.ndarray:
    """The walkable polygon of a scene file as ring edges [E,4] float32: the `edges` key of a file `scene_gen.save_scene` /
    `prepare_scene` wrote, else its rings (`ring_xy`, `ring_off`); `room0` is the polygon of the packaged assets.  ValueError for
    a file with neither."""
    from . import synth
    if path == "room0":
        return synth.rings_to_edges(synth.room0_polygon()).astype(np.float32)
    with np.load(path) as z:
        if "edges" in z.files:
            return np.asarray(z["edges"], np.float32).reshape(-1, 4)
        if "ring_xy" in z.files and "ring_off" in z.files:
            off = z["ring_off"]
            return synth.rings_to_edges([z["ring_xy"][off[i]:off[i + 1]] for i in range(len(off) - 1)]).astype(np.float32)
    raise ValueError(f"{path} holds neither `edges` nor rings (`ring_xy`, `ring_off`)")


class PolicyProposal:
    """What `generate_sequence_to_goal(policy=)` takes.
        - policy: a `GAMMAPPOPolicy`, or anything holding a `PolicyHipRunner` (attribute `_runner`, or the runner itself).  Only
          the actor branch is evaluated (want_critic=False).
        - edges [E,4] (x0,y0,x1,y1) / edge_off [S+1] / scene_idx [b]: the walkable polygons of S scenes as ring edges and the scene
          of every sequence.  edges alone is one scene for everybody; scene_idx None is scene 0 for everybody; no edges: no
          polygon, every ray then reads +1 (the eye is inside an unbounded plane).
        - temperature (1.0, >= 0): scale of the policy's sigma; 0 makes every policy row mu.
        - n_mean (1): rows of a sequence that are mu itself.
        - prior_fraction (0.25, in [0, 1]): share of the N rows left as the prior's N(0, I) samples, a safeguard against a policy
          that is wrong about a place it never saw: n_policy = N - floor(prior_fraction * N); n_mean > n_policy raises.
        - ray_len (7.0 m, the env's), max_depth (None: the packaged policy config's trainconfig.max_depth, 13): `time` of
          primitive k is 1 - min(k, max_depth) / max_depth; the clamp is a stated choice, the policy never saw a step above
          max_depth.
        - sense_people (False): True makes the other people of the call holes of the walkable polygon the rays are cast against, as
          in the reference's crowd evaluation: per primitive every sequence publishes the world xy box of its two seed frames'
          markers (entry egx_primitive_people_boxes), and the observation (entry egx_primitive_observe_people in place of
          egx_primitive_observe) takes the boxes of the sequence's group-mates under `groups=` and of the tracks of its set under
          `obstacles=` at the two seed frames out of the polygon: an eye in a box sees nothing, a ray ends at the first box or wall.
          Without groups and obstacles the observation is egx_primitive_observe's, bit for bit.  The result then holds people_box
          [K,b,4] and obs_people_count [K,b] (the holes of every sequence).
    temperature, n_mean and prior_fraction are stated choices like the search's weights: nobody has measured motion quality with
    them, and no trained checkpoint has been run through this path (the instrument for it: egogen_amd/metrics.py)."""

    def __init__(self, policy, edges=None, edge_off=None, scene_idx=None, temperature: float = 1.0, n_mean: int = 1,
                 prior_fraction: float = 0.25, ray_len: float = 7.0, max_depth: Optional[int] = None, sense_people: bool = False):
        if not isinstance(sense_people, (bool, np.bool_)):
            raise TypeError(f"sense_people must be a bool, got {type(sense_people).__name__}")
        self.sense_people = bool(sense_people)
        runner = getattr(policy, "_runner", policy)
        if not (hasattr(runner, "forward") and hasattr(runner, "actor")):
            raise TypeError(f"policy must be a GAMMAPPOPolicy or hold a PolicyHipRunner, got {type(policy).__name__}")
        self.policy, self.runner = policy, runner
        self.min_logvar, self.max_logvar = float(runner.actor.min_logvar), float(runner.actor.max_logvar)
        if not float(temperature) >= 0 or not np.isfinite(float(temperature)):
            raise ValueError(f"temperature must be finite and not negative, got {temperature}")
        if int(n_mean) != n_mean or int(n_mean) < 0:
            raise ValueError(f"n_mean must be a whole number >= 0, got {n_mean}")
        if not 0.0 <= float(prior_fraction) <= 1.0:
            raise ValueError(f"prior_fraction must be in [0, 1], got {prior_fraction}")
        if not float(ray_len) > 0:
            raise ValueError(f"ray_len must be positive, got {ray_len}")
        if max_depth is None:
            from .crowd_env import DEFAULT_CFG
            max_depth = DEFAULT_CFG["max_depth"]
        if int(max_depth) < 1:
            raise ValueError(f"max_depth must be >= 1, got {max_depth}")
        self.temperature, self.n_mean, self.prior_fraction = float(temperature), int(n_mean), float(prior_fraction)
        self.ray_len, self.max_depth = float(ray_len), int(max_depth)
        self.edges = self.edge_off = self.scene_idx = None
        if edges is None:
            if edge_off is not None or scene_idx is not None:
                raise ValueError("edge_off / scene_idx need edges")
        else:
            e = np.ascontiguousarray(np.asarray(edges.detach().cpu() if torch.is_tensor(edges) else edges, np.float32))
            if e.ndim != 2 or e.shape[1] != 4 or e.shape[0] < 1 or not np.isfinite(e).all():
                raise ValueError(f"edges must be [E,4] finite with E >= 1, got {e.shape}")
            off = np.asarray([0, e.shape[0]] if edge_off is None else
                             (edge_off.detach().cpu() if torch.is_tensor(edge_off) else edge_off)).reshape(-1)
            if off.size < 2 or off[0] != 0 or off[-1] != e.shape[0] or (np.diff(off) < 0).any() or (off != off.astype(np.int64)).any():
                raise ValueError(f"edge_off must rise from 0 to E = {e.shape[0]} over S + 1 entries, got {off.tolist()}")
            self.edges, self.edge_off = e, off.astype(np.int32)
            if scene_idx is not None:
                idx = np.asarray(scene_idx.detach().cpu() if torch.is_tensor(scene_idx) else scene_idx).reshape(-1)
                if idx.size < 1 or (idx != idx.astype(np.int64)).any() or idx.min() < 0 or idx.max() >= self.num_scenes:
                    raise ValueError(f"scene_idx must hold indices in [0, {self.num_scenes}), got {idx.tolist()}")
                self.scene_idx = idx.astype(np.int32)

    @property
    def num_scenes(self) -> int:
        return 0 if self.edge_off is None else len(self.edge_off) - 1

    @classmethod
    def from_scene_file(cls, policy, path: str, **kwargs) -> "PolicyProposal":
        """One scene for every sequence, its polygon read by `scene_file_edges` (a scene file, or `room0`)."""
        return cls(policy, edges=scene_file_edges(path), **kwargs)

    def counts(self, N: int):
        """(n_mean, n_policy) for N candidates; ValueError where n_mean does not fit."""
        n_policy = int(N) - int(np.floor(self.prior_fraction * int(N)))
        if self.n_mean > N:
            raise ValueError(f"n_mean = {self.n_mean} exceeds the {N} candidates of a sequence")
        if self.n_mean > n_policy:
            raise ValueError(f"n_mean = {self.n_mean} exceeds the {n_policy} policy rows that prior_fraction = {self.prior_fraction} "
                             f"leaves of {N} candidates")
        return self.n_mean, n_policy

    # ------------------------------------------------------------------------------------------------------------------
    def prepare(self, op, s: dict, K: int, b: int, N: int):
        """Everything the loop needs, into the state dict `s` of the search, before the loop: the polygon on the device, the
        [K,b,...] records the launches write into, the runner's scratch, and the joints of the b x 2 seed bodies (one body-model
        forward) that the first observation reads."""
        dev, f32 = op.device, torch.float32
        n_mean, n_policy = self.counts(N)
        if self.scene_idx is not None and len(self.scene_idx) != b:
            raise ValueError(f"scene_idx must hold {b} indices, one per sequence, got {len(self.scene_idx)}")
        poly = (None, None, None, 0)
        alive = None
        if self.edges is not None:
            idx = np.zeros(b, np.int32) if self.scene_idx is None else self.scene_idx
            alive = [torch.from_numpy(a).to(dev).contiguous() for a in (self.edges, self.edge_off, idx)]
            poly = (*[_lib.ptr(t) for t in alive], self.num_scenes)
        rec = lambda *tail: torch.empty(K, b, *tail, device=dev, dtype=f32)
        s.update({"policy_mu": rec(128), "policy_logvar": rec(128), "obs_state": rec(2, 402), "obs_egosensing": rec(2, 32),
                  "obs_dist": rec(), "obs_time": rec(), "policy_poly": poly, "policy_alive": alive,
                  "policy_counts": (n_mean, n_policy)})
        if self.sense_people:
            s.update({"people_box": rec(4), "obs_people_count": torch.empty(K, b, device=dev, dtype=torch.int32)})
        # the start: the seed bodies in the frame (R0, T0) of the seed, one row per sequence
        bm = op.body_model
        seed0 = s["seed"][::N].contiguous()
        start = bm.forward(seed0.view(b * 2, seed0.shape[-1]), s["bt"][::N].contiguous(), 2, want_verts=False, want_joints=True,
                           want_markers=False)
        s["policy_start"] = {"joints": start["joints"].contiguous(), "R0": s["R0"][::N].contiguous(), "T0": s["T0"][::N].contiguous()}
        lib = _lib.load()
        self.runner._ws.get(lib.egx_policy_workspace_bytes(b), dev)     # the forward's scratch exists before the loop
        self.runner._weights()

    def launch(self, s: dict, k: int, b: int, N: int, st, groups=NO_GROUPS, obstacles=NO_OBSTACLES):
        """The three launches of primitive k ahead of the search's prefix: observe -> the actor -> propose into s["z"][k].  With
        `sense_people` four: the boxes first, and the observation with the holes of `groups` (group_start, group_member, member_group,
        num_groups) and `obstacles` (the obstacle arguments of a selection entry from obs_xy to num_frames, then the absolute frame of
        the first seed frame)."""
        lib = _lib.load()
        cur = s["xs"][k % 2]
        o = (_vp(s["obs_state"][k]), _vp(s["obs_egosensing"][k]), _vp(s["obs_dist"][k]), _vp(s["obs_time"][k]))
        if k == 0:      # the seed bodies in the seed's frame: one row per sequence, its seed frames N rows apart
            p0 = s["policy_start"]
            lead = (_lib.ptr(p0["joints"]), 2, 0, None, 1, _lib.ptr(p0["R0"]), _lib.ptr(p0["T0"]))
            frame, x_ld, n = (_lib.ptr(p0["R0"]), _lib.ptr(p0["T0"])), 201 * N, 1
        else:           # the last two bodies of the candidate chosen at primitive k - 1, in the frame that primitive was made in
            lead = (_lib.ptr(s["lbs_out"]["joints"]), 20, 18, _vp(s["choice"][k - 1]), N, _vp(s["rotmat"][k - 1]), _vp(s["transl"][k - 1]))
            frame, x_ld, n = (_lib.ptr(s["R0"]), _lib.ptr(s["T0"])), 201, N
        common = (*lead, *frame, _vp(cur[0]), _vp(cur[1]), x_ld, _lib.ptr(s["goal"]), *s["policy_poly"], self.ray_len, k, self.max_depth, b)
        if self.sense_people:
            box = _vp(s["people_box"][k])
            _lib.check(lib.egx_primitive_people_boxes(_vp(cur[0]), _vp(cur[1]), x_ld, *frame, n, b, box, st), "egx_primitive_people_boxes")
            _lib.check(lib.egx_primitive_observe_people(*common, box, *groups, *obstacles, _vp(s["obs_people_count"][k]), *o, st),
                       "egx_primitive_observe_people")
        else:
            _lib.check(lib.egx_primitive_observe(*common, *o, st), "egx_primitive_observe")
        obs ={"state": s["obs_state"][k], "egosensing": s["obs_egosensing"][k], "dist": s["obs_dist"][k], "time": s["obs_time"][k]}
        self.runner.forward(obs, want_actor=True, want_critic=False, out={"mu": s["policy_mu"][k], "logvar": s["policy_logvar"][k]})
        n_mean, n_policy = s["policy_counts"]
        zk = s["z"][k]
        _lib.check(lib.egx_policy_propose(_vp(s["policy_mu"][k]), _vp(s["policy_logvar"][k]), _vp(zk), self.min_logvar, self.max_logvar,
                                          b, N, n_mean, n_policy, self.temperature, _vp(zk), st), "egx_policy_propose")

    def record(self, s: dict) -> dict:
        n_mean, n_policy = s["policy_counts"]
        out = {k: s[k] for k in POLICY_FIELDS[:6]}
        out.update(policy_temperature=self.temperature, policy_n_mean=n_mean, policy_n_policy=n_policy, policy_ray_len=self.ray_len,
                   policy_max_depth=self.max_depth, people_box=s.get("people_box"), obs_people_count=s.get("obs_people_count"),
                   policy_sense_people=self.sense_people)
        return out
