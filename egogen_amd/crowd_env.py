"""Batched CrowdEnv on the GPU: host-side mirror of crowd_ppo/crowd_env_2f.py (SDF scene) and
crowd_ppo/crowd_env_2f_box.py (random box scenes) of the reference, for A independent agents at once.

One `step(actions[A,128])` enqueues, with no host synchronisation:
    egx_sample_prior  ->  egx_assemble_params  ->  egx_lbs_forward (+SDF counts)  ->  egx_vposer_encode
    ->  egx_env_step_post  ->  (auto-reset of finished agents: egx_env_reset)
and can be captured once into a HIP graph (`use_graph=True`).  The reference's per-env gym API
(reset() -> (obs, {}), step(a) -> (obs, reward, terminated, truncated, info)) is provided by `CrowdEnv`,
a 1-agent view, for drop-in use; the vector API is what the trainer uses (the reference's DummyVectorEnv
steps its envs one after the other, main_ppo.py:97).

Observation dict (crowd_env_2f.py:49-51,311-312): state[A,2,402], egosensing[A,2,32], dist[A], time[A].
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple
from dataclasses import dataclass
from typing import Dict, List, NamedTuple, Optional

import numpy as np
import torch

from . import _lib, synth
from .body_model import BodyModelHandle, SdfScene, SdfSceneSet
from .models import GAMMAPrimitiveCombo, VPoserEncoder

DEFAULT_CFG = {  # crowd_ppo/cfg_samp20/MPVAEPolicy_samp_collision.yaml
    "reproj_factor": 0.5, "goal_thresh": 0.1, "max_depth": 13, "pene_thres": 3,
    "weight_vp": 0.1, "weight_floor": 0.1, "weight_skate": 0.3, "weight_target_dist": 1.0,
    "weight_face_target": 0.1, "weight_look_target": 0.3, "weight_pene": 0.1, "weight_success": 0.5,
    "map_res": 16, "map_extent": 0.8, "pene_type": "body", "ray_len": 7.0,
}
BOX_CFG = dict(DEFAULT_CFG, weight_look_target=0.1, max_depth=11)  # ..._collision_2.yaml (primitive_model.py:77-78)

CAND_POOL = 16   # steps of reset candidates drawn at a time (SDF and box scenes)


def _rodrigues_np(aa: np.ndarray) -> np.ndarray:
    aa = np.asarray(aa, np.float64)
    th = np.linalg.norm(aa)
    if th < 1e-12:
        return np.eye(3)
    k = aa / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def block_scene_assignment(num_agents: int, num_scenes: int) -> np.ndarray:
    """Scene of every agent of an SDF env over a set of scenes: contiguous blocks, agent a -> floor(a S / A) (balanced and
    deterministic, like a vector of per-scene envs; a 256-body group of the LBS launch stays inside one scene)."""
    if not 1 <= num_scenes <= num_agents:
        raise ValueError(f"an SDF env over {num_scenes} scenes needs 1 <= scenes <= agents ({num_agents})")
    return (np.arange(num_agents, dtype=np.int64) * num_scenes // num_agents).astype(np.int32)


def env_config(scene_kind: str, cfg: dict, finetuning: bool = False, vp_thresh: float = 11.0,
               goal_terminates: bool = True) -> _lib.EnvConfig:
    """egx_env_config of a scene kind: the yaml's weights, and what the reference's three env classes hard-code."""
    c = cfg
    weight_pene, terminate_on_penetration = {
        "sdf": (0.1 if finetuning else 1.0, 1 if finetuning else 0),   # crowd_env_2f.py:268-271, :299-302
        "crowd": (c["weight_pene"], 0),                                 # crowd_env_crowd_eval.py:367
        "box": (c["weight_pene"], 1)}[scene_kind]                       # crowd_env_2f_box.py:303, :325
    return _lib.fill(
        _lib.EnvConfig(), reproj_factor=c["reproj_factor"], goal_thresh=c["goal_thresh"], pene_thres=c["pene_thres"],
        weight_skate=c["weight_skate"], weight_floor=c["weight_floor"], weight_face_target=c["weight_face_target"],
        weight_look_target=c["weight_look_target"], weight_success=c["weight_success"], weight_target_dist=c["weight_target_dist"],
        weight_vp=c["weight_vp"], weight_pene=weight_pene, terminate_on_penetration=terminate_on_penetration,
        max_depth=int(c["max_depth"]), scene_kind={"sdf": 0, "box": 1, "crowd": 2}[scene_kind],
        pene_type_body=1 if c["pene_type"] == "body" else 0, ray_len=float(c["ray_len"]), vp_thresh=float(vp_thresh),
        no_goal_termination=0 if goal_terminates else 1)


# What a scene kind hands the constructor: per scene its polygon edges [E,4], obstacle triangles [T,6] and floor height; the
# start/target pairs in that kind's layout; candidates per launch K and launches per reset R.
SceneLists = namedtuple("SceneLists", "edges tris floor pairs K R")


def box_scene_lists(box_scenes, num_candidates=None, reset_rounds=None) -> SceneLists:
    if not box_scenes:
        raise ValueError("box scene kind needs box_scenes")
    P = min(len(s["pairs"]) for s in box_scenes)
    return SceneLists([np.asarray(s["edges"], np.float32) for s in box_scenes],
                      [np.asarray(s["tris"], np.float32).reshape(-1, 6) for s in box_scenes],
                      [float(s["floor_height"]) for s in box_scenes],
                      np.stack([np.asarray(s["pairs"][:P], np.float32) for s in box_scenes]),      # [S,P,2,3]
                      int(num_candidates or 8), int(reset_rounds or 4))


def crowd_scene_lists(num_agents: int, crowd_bbox, crowd_pairs, crowd_rings=None) -> SceneLists:
    """main_crowd_eval.py: every scene holds G members; the walkable polygon of a member is the 8x8 m floor minus the marker
    boxes of the others (dummy_vector_env.py:34-39, crowd_env_crowd_eval.py:796-822), so the edge table holds one unused
    zero edge - or, EgoBody variant, the rings of the scene's walkable polygon."""
    A = num_agents
    if crowd_bbox is None or crowd_pairs is None or crowd_bbox.shape[1] != A or crowd_bbox.shape[2] != 4:
        raise ValueError("crowd scene kind needs crowd_bbox[G,A,4] and crowd_pairs[A,2,3]")
    edges = np.zeros((1, 4), np.float32) if crowd_rings is None else synth.rings_to_edges(crowd_rings).astype(np.float32)
    return SceneLists([edges], [np.zeros((0, 6), np.float32)], [0.0], np.asarray(crowd_pairs, np.float32).reshape(A, 1, 2, 3), 1, 1)


def sdf_scene_args(sdf_dict=None, rings=None, pairs=None, sdf_scenes=None) -> List[dict]:
    """The SDF kind's scenes as a list [{sdf_dict, rings, pairs, name}, ...] (`sdf_dict` / `rings` / `pairs` are a set of one)."""
    if sdf_scenes is None:
        if sdf_dict is None or rings is None or pairs is None:
            raise ValueError("sdf scene needs sdf_dict, rings (walkable polygon) and start/target pairs")
        return [dict(sdf_dict=sdf_dict, rings=rings, pairs=pairs, name="scene")]
    if sdf_dict is not None or rings is not None or pairs is not None:
        raise ValueError("pass either sdf_dict / rings / pairs or sdf_scenes, not both")
    return list(sdf_scenes)


def scene_tables(edges, tris=None, floor=None) -> Dict[str, np.ndarray]:
    """The per-scene lists as the kernels read them: rows concatenated, scene s's in [off[s], off[s+1]).  Without any triangle
    `tris` is one zero row (the kernels want an address) under all-zero offsets."""
    tris = tris if tris is not None else [np.zeros((0, 6), np.float32)] * len(edges)
    off = lambda rows: np.cumsum([0] + [len(r) for r in rows]).astype(np.int32)
    return {"edges": np.concatenate(edges, 0).astype(np.float32), "edge_off": off(edges),
            "tris": np.concatenate(tris, 0).astype(np.float32) if sum(len(t) for t in tris) else np.zeros((1, 6), np.float32),
            "tri_off": off(tris), "floor_h": np.asarray(floor if floor is not None else [0.0] * len(edges), np.float32)}


def seed_table_inputs(motion_seed: dict, starts, agent_seeds=None):
    """(pose[NV,2,63], glorot[NV,2,3,3], transl[NV,2,3]) of the two seed frames of every variant v: frames starts[v], +1 of the
    motion seed, or agent v's own two frames."""
    NV = len(starts)
    pose, glorot, transl = np.zeros((NV, 2, 63)), np.zeros((NV, 2, 3, 3)), np.zeros((NV, 2, 3))
    for v, s in enumerate(starts):
        for f in range(2):
            if agent_seeds is not None:
                d = agent_seeds[v]
                po, tr = np.asarray(d["poses"], np.float64)[f], np.asarray(d["trans"], np.float64)[f]
            else:
                po, tr = motion_seed["poses"][s + f], motion_seed["trans"][s + f]
            pose[v, f], glorot[v, f], transl[v, f] = po[3:66], _rodrigues_np(po[:3]), tr
    return pose, glorot, transl


def round_major(t: torch.Tensor, A: int, K: int, R: int, tail=()) -> torch.Tensor:
    """Injected candidates [A, r*K, *tail] (agent a's draws in the order the reference's loop would see them) as round-major
    [r, A, K, *tail]: draw j of agent a is candidate j % K of launch j // K."""
    t = t.reshape(A, -1, *tail)
    r = t.shape[1] // K
    if r < 1 or r > R or t.shape[1] != r * K:
        raise ValueError(f"candidates per agent must be a multiple of K={K} up to {R * K}, got {t.shape[1]}")
    return t.reshape(A, r, K, *tail).transpose(0, 1)


@dataclass
class Candidates:
    """The reset draws in use, round-major (round r's draws are one contiguous block handed to the kernel by address):
    pairs[R,A,K,2,3], yaw / variant / scene[R,A,K]; the next reset launches the first `rounds` of them."""
    pairs: torch.Tensor
    yaw: Optional[torch.Tensor]
    variant: Optional[torch.Tensor]
    scene: Optional[torch.Tensor]
    rounds: int = 1


class PairTables(NamedTuple):
    """Pre-validated pairs of a scene set; per scene s its accepted pairs are valid_pairs[vp_off[s] : vp_off[s] + vp_n[s]]."""
    pairs_all: torch.Tensor
    pair_valid_mask: torch.Tensor
    valid_pairs: torch.Tensor
    vp_n: torch.Tensor
    vp_off: torch.Tensor


class VecCrowdEnv:
    def __init__(self, num_agents: int, body_model: BodyModelHandle, prior: GAMMAPrimitiveCombo, vposer: VPoserEncoder,
                 scene_kind: str = "sdf", sdf_dict: Optional[dict] = None, rings: Optional[List[np.ndarray]] = None,
                 pairs: Optional[np.ndarray] = None, box_scenes: Optional[List[dict]] = None,
                 sdf_scenes: Optional[List[dict]] = None, motion_seed: Optional[dict] = None, cfg: Optional[dict] = None, finetuning: bool = False,
                 seed: int = 0, num_candidates: Optional[int] = None, use_graph: bool = False,
                 keep_rollout: bool = False, device: str = "cuda", crowd_bbox: Optional[torch.Tensor] = None,
                 crowd_member: int = 0, crowd_pairs=None, crowd_floor_half: float = 4.0,
                 crowd_rings: Optional[List[np.ndarray]] = None, crowd_static: bool = False, agent_seeds: Optional[List[dict]] = None,
                 vp_thresh: float = 11.0, goal_terminates: bool = True, gender: str = "male", reset_rounds: Optional[int] = None):
        """`reset_rounds`: box scenes - launches of the reset kernel per reset.  The reference draws starts until one passes
        the walkability check (`while True`, crowd_env_2f_box.py:349-416); here a launch tries `num_candidates` (8) draws per
        agent and the agents none of whose draws passed are re-launched with fresh draws (device mask, no host sync) up to
        `reset_rounds` (4) launches = 32 draws; whoever is still without a valid start after the last round keeps its last
        draw and is counted in `forced_accepts()`.
        `gender` names the body model / motion prior the caller passed in (`crowd_env_2f.py:393` picks
        genop_2frame_male | female by it; every sampler but the EgoBody one draws from ['male'], environments.py:254,555,906);
        it is recorded in the saved rollouts.  `crowd_rings` / `crowd_static` / `agent_seeds` / `vp_thresh` / `goal_terminates` are the EgoBody-evaluation variant of
        the crowd scenes (crowd_env_egobody_eval.py, see CrowdGroupEnv): the scene's walkable polygon as exterior, one motion
        seed (two frames + betas) per agent instead of one table for all, the looser pose filter, no goal termination.
        `sdf_scenes`: the SDF kind over a SET of scenes of the same grid dimensions, [{sdf_dict, rings, pairs, name}, ...]
        (`sdf_dict` / `rings` / `pairs` are a set of one).  Agents are assigned to scenes once, in contiguous blocks
        (`block_scene_assignment`, written to `scene_idx`); each draws its starts from its own scene's valid pairs, its rays hit
        its own scene's polygon and its penetration count reads its own scene's SDF (one LBS launch over the set)."""
        if not torch.cuda.is_available():
            raise _lib.EgxError("VecCrowdEnv needs a HIP device (no CPU fallback)")
        self.lib = _lib.load()
        self.A = A = int(num_agents)
        self.dev = torch.device(device)
        self.bm, self.prior, self.vposer = body_model, prior, vposer
        self.gender, self.scene_kind, self.finetuning = gender, scene_kind, finetuning
        self.cfg = dict(cfg or (BOX_CFG if scene_kind in ("box", "crowd") else DEFAULT_CFG))  # main_crowd_eval.py:224 load_model(box=True)
        self.crowd_bbox, self.crowd_member = crowd_bbox, int(crowd_member)
        self.use_graph, self.keep_rollout = use_graph, keep_rollout
        self.gen = torch.Generator(device=self.dev).manual_seed(int(seed))
        self._alloc_buffers()
        self._init_motion_seed(motion_seed, agent_seeds)
        self.sdf = self.scene_names = self.scene_boxes = self.valid_pairs = None
        self.scene_generation = 0   # swaps of the scene set so far (replace_sdf_scenes)
        if scene_kind == "sdf":
            sl = self._sdf_scenes(sdf_scene_args(sdf_dict, rings, pairs, sdf_scenes), num_candidates)
        elif scene_kind == "box":
            sl = box_scene_lists(box_scenes, num_candidates, reset_rounds)
            self.box_pairs = self._f32(sl.pairs)
        elif scene_kind == "crowd":
            sl = crowd_scene_lists(A, crowd_bbox, crowd_pairs, crowd_rings)
            self.crowd_pairs = self._f32(sl.pairs)
        else:
            raise ValueError(f"unknown scene_kind {scene_kind!r}")
        self.K, self.R, self.num_scenes = sl.K, sl.R, len(sl.edges)   # candidates per launch, launches per reset
        self._upload_scene_tables(scene_tables(sl.edges, sl.tris, sl.floor))
        self._init_candidates()
        self._init_structs(crowd_floor_half, crowd_rings, crowd_static, vp_thresh, goal_terminates)
        # workspaces are sized now so that nothing allocates during graph capture
        self.bm.workspace(A * 20)
        self.prior._ws.get(self.lib.egx_sample_prior_workspace_bytes(A), self.dev)
        if self.vposer._folded is None:
            self.vposer.fold()
        self.prior._weights()
        self._graph = None
        self._z_in = self.z
        self.profile_events = []  # [(start_event, stop_event)] consumed one pair per step (bench.py)
        if scene_kind == "sdf":
            self.pairs_all, self.pair_valid_mask, self.valid_pairs, self._vp_n, self._vp_off = self._validated_pairs(
                self.pairs_scene, self.sdf_scenes, self.scene_names, self._sc)

    # ------------------------------------------------------------------------------------------
    def _f32(self, a) -> torch.Tensor:
        return torch.tensor(a, dtype=torch.float32, device=self.dev).contiguous()

    def _alloc_buffers(self):
        A, A20, keep = self.A, self.A * 20, self.keep_rollout
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=self.dev)
        zi = lambda *s: torch.zeros(*s, dtype=torch.int32, device=self.dev)
        # ---- persistent state ----
        self.state, self.seed = z(A, 2, 402), z(A, 2, 93)
        self.R0, self.T0 = z(A, 3, 3), z(A, 3)
        self.dist, self.wpath = z(A), z(A, 2, 3)
        self.steps, self.scene_idx = zi(A), zi(A)
        # ---- step intermediates / outputs ----
        self.z, self.pred_params = z(A, 128), z(A, 20, 93)
        self.Y_gen, self.Yb_gen = z(18, A, 201), z(18, A, 93)
        self.joints, self.markers = z(A20, synth.NUM_JOINTS_OUT, 3), z(A20, self.bm.M, 3)
        self.pene_count, self.vp_emb = zi(A20), z(A20, 32)
        self.reward, self.rterms, self.terminated = z(A), z(A, 8), zi(A)
        self.obs_ego, self.obs_dist, self.obs_time = z(A, 2, 32), z(A), z(A)
        self.marker_b = z(A, 20, 67, 3) if keep else None
        self.prev_frame = z(A, 12) if keep else None
        self.feet_marker_idx = torch.tensor(synth.feet_marker_idx(), dtype=torch.int32, device=self.dev)
        self._lbs_out = {"joints": self.joints, "markers": self.markers, "pene_count": self.pene_count}
        self.invalid = zi(A)      # EgoBody filters (egx_env_step_io.invalid_flags)
        self.nonfinite = zi(1)
        # ---- reset outputs ----
        self.choice = zi(A)
        self.ones_mask = torch.ones(A, dtype=torch.int32, device=self.dev)
        self.pending = zi(A)      # agents whose draws of the last launch all failed the start check
        self.forced = zi(1)       # starts committed in penetration after the last round

    def _init_motion_seed(self, motion_seed, agent_seeds):
        """Motion seed (data/locomotion/subseq_00343.npz in the reference), the start frames of its variants and the tables of
        the variants' bodies at identity global orient / zero transl (one LBS call): the scene sampler only ever rotates /
        translates them rigidly (environments.py:216-247), so reset needs no SMPL-X call."""
        A, kind = self.A, self.scene_kind
        ms = motion_seed or {k: synth.load_assets()[f"seed_{k}"] for k in ("poses", "trans", "betas")}
        self.motion_seed = {k: np.asarray(v, np.float64) for k, v in ms.items() if k in ("poses", "trans", "betas")}
        self.betas = self._f32(self.motion_seed["betas"]).reshape(1, 10).repeat(A, 1).contiguous()
        self.agent_seeds = agent_seeds
        if agent_seeds is not None:
            if kind != "crowd" or len(agent_seeds) != A:
                raise ValueError("agent_seeds: one {poses[2,66], trans[2,3], betas[10]} per agent, crowd scenes only")
            self.betas = self._f32(np.stack([np.asarray(d["betas"], np.float32).reshape(10) for d in agent_seeds]))
            starts = list(range(A))                                # table row a = agent a's own two frames
        elif kind == "sdf":
            starts = [5]                                           # environments.py:193 fixed start frame
        elif kind == "crowd" and motion_seed is not None and motion_seed.get("fixed_start") is not None:
            starts = [int(motion_seed["fixed_start"])]
        else:
            starts = list(range(len(self.motion_seed["poses"]) - 1))  # environments.py:483 random start frame
        self.variant_starts = starts
        NV = len(starts)
        pose, glorot, transl = seed_table_inputs(self.motion_seed, starts, agent_seeds)
        xb = torch.zeros(NV * 2, 93)
        xb[:, 6:69] = torch.tensor(pose.reshape(NV * 2, 63), dtype=torch.float32)
        betas_rows = (self.betas.repeat_interleave(2, 0) if agent_seeds is not None
                      else self._f32(self.motion_seed["betas"]).reshape(1, 10).repeat(NV * 2, 1)).contiguous()
        out = self.bm.forward(xb.to(self.dev), betas_rows, 1, want_verts=False)
        self.tab_joints = out["joints"].reshape(NV, 2, -1, 3).clone().contiguous()
        self.tab_markers = out["markers"].reshape(NV, 2, -1, 3).clone().contiguous()
        self.tab_glorot, self.tab_transl, self.tab_pose = self._f32(glorot), self._f32(transl), self._f32(pose)

    def _sdf_scene_set(self, sdf_scenes: List[dict], dims=None) -> dict:
        """Everything an SDF env holds per scene set, built without touching the env: the scenes' device grids, what the LBS
        call counts in (the scene itself, egx_lbs_forward, or the set with scene_idx as the agents' scenes), names, the box
        layouts of generated scenes (scene_gen), each scene's polygon edges and its start/target pairs."""
        scenes = [d["sdf_dict"] if isinstance(d["sdf_dict"], SdfScene) else SdfScene(d["sdf_dict"], device=self.dev) for d in sdf_scenes]
        for d, sc in zip(sdf_scenes, scenes):
            if dims is not None and tuple(sc.grid.shape) != dims:
                raise ValueError(f"replace_sdf_scenes: scene {d.get('name')!r} has an SDF grid of {tuple(sc.grid.shape)}, the env's scenes {dims}")
        return dict(sdf_scenes=scenes, sdf=scenes[0] if len(scenes) == 1 else SdfSceneSet(scenes),
                    scene_names=[str(d.get("name", f"scene{s}")) for s, d in enumerate(sdf_scenes)],
                    scene_boxes=[d.get("boxes") for d in sdf_scenes],
                    edge_lists=[synth.rings_to_edges(d["rings"]).astype(np.float32) for d in sdf_scenes],
                    pairs_scene=[self._f32(np.asarray(d["pairs"], np.float32)).reshape(-1, 2, 3) for d in sdf_scenes])

    def _adopt_sdf_scene_set(self, ss: dict):
        self.sdf_scenes, self.sdf, self.scene_names, self.scene_boxes, self.pairs_scene = (
            ss[k] for k in ("sdf_scenes", "sdf", "scene_names", "scene_boxes", "pairs_scene"))

    def _sdf_scenes(self, sdf_scenes: List[dict], num_candidates) -> SceneLists:
        S = len(sdf_scenes)
        self.scene_idx.copy_(torch.from_numpy(block_scene_assignment(self.A, S)))
        ss = self._sdf_scene_set(sdf_scenes)
        self._adopt_sdf_scene_set(ss)
        return SceneLists(ss["edge_lists"], [np.zeros((0, 6), np.float32)] * S, [0.0] * S, self.pairs_scene, int(num_candidates or 1), 1)

    def _upload_scene_tables(self, t: Dict[str, np.ndarray]):
        self.edges, self.floor_h = self._f32(t["edges"]), self._f32(t["floor_h"])
        self.tris = self._f32(t["tris"]) if t["tri_off"][-1] else torch.zeros(1, 6, device=self.dev)   # placeholder: nothing to copy
        self.edge_off = torch.tensor(t["edge_off"], dtype=torch.int32, device=self.dev)
        self.tri_off = torch.tensor(t["tri_off"], dtype=torch.int32, device=self.dev)
        self.map_lin = torch.linspace(-self.cfg["map_extent"], self.cfg["map_extent"], self.cfg["map_res"]).to(self.dev)

    def _init_candidates(self):
        A, K, R = self.A, self.K, self.R
        z = lambda dt: torch.zeros(R, A, K, dtype=dt, device=self.dev)
        self._cands = Candidates(torch.zeros(R, A, K, 2, 3, dtype=torch.float32, device=self.dev), z(torch.float32), z(torch.int32),
                                 z(torch.int32), R)
        self._injected = False               # set_candidates' draws wait for the next reset
        self._pool, self._pool_pos = None, 0
        self._draw = {"sdf": lambda: self._from_pool(self._sdf_pool), "box": lambda: self._from_pool(self._box_pool),
                      "crowd": self._draw_crowd}[self.scene_kind]     # each returns the Candidates of the next reset

    def _init_structs(self, crowd_floor_half, crowd_rings, crowd_static, vp_thresh, goal_terminates):
        scene_kind = self.scene_kind
        self._ec = env_config(scene_kind, self.cfg, self.finetuning, vp_thresh, goal_terminates)
        self._sc = _lib.fill(_lib.EnvScenes(), edges=self.edges, edge_off=self.edge_off, tris=self.tris, tri_off=self.tri_off,
                             floor_height=self.floor_h, map_lin=self.map_lin, map_res=int(self.cfg["map_res"]))
        if scene_kind == "crowd":
            _lib.fill(self._sc, crowd_bbox=self.crowd_bbox, crowd_group=int(self.crowd_bbox.shape[0]), crowd_scenes=self.A,
                      crowd_member=self.crowd_member, crowd_floor_half=float(crowd_floor_half),
                      crowd_polygon=int(crowd_rings is not None), crowd_static=int(bool(crowd_static)))
        self._st = _lib.fill(_lib.EnvState(), state=self.state, seed=self.seed, R0=self.R0, T0=self.T0, dist=self.dist,
                             steps=self.steps, wpath=self.wpath, scene_idx=self.scene_idx)
        self._io = _lib.fill(
            _lib.EnvStepIO(), Y_gen=self.Y_gen, pred_params=self.pred_params, joints=self.joints, markers_proj=self.markers,
            pene_count=self.pene_count if scene_kind == "sdf" else None, vp_emb=self.vp_emb, feet_marker_idx=self.feet_marker_idx,
            reward=self.reward, terminated=self.terminated, reward_terms=self.rterms, nonfinite_count=self.nonfinite,
            invalid_flags=self.invalid, obs_ego=self.obs_ego, obs_dist=self.obs_dist, obs_time=self.obs_time,
            out_marker_b=self.marker_b, out_prev_frame=self.prev_frame)
        self._rio = self._reset_io_fixed(self.K, (self.obs_ego, self.obs_dist, self.obs_time), self.choice,
                                         self.pending if scene_kind == "box" else None)

    def _reset_io_fixed(self, K, obs, choice=None, pending=None) -> _lib.EnvResetIO:
        """egx_env_reset_io without what changes from launch to launch: the seed tables and where to write the observation."""
        return _lib.fill(_lib.EnvResetIO(), num_candidates=K, tab_joints=self.tab_joints, tab_markers=self.tab_markers,
                         tab_glorot=self.tab_glorot, tab_transl=self.tab_transl, tab_pose=self.tab_pose, obs_ego=obs[0],
                         obs_dist=obs[1], obs_time=obs[2], out_choice=choice, out_pending=pending)

    def _reset_io(self, io, c: Candidates, r: int = 0, mask=None, last: bool = True) -> _lib.EnvResetIO:
        """`io` for launch r of the candidate set c (the kernel's arguments are copied at the call: one struct serves all)."""
        _lib.fill(io, mask=mask, cand_pairs=c.pairs[r])
        if self.scene_kind != "sdf":
            _lib.fill(io, cand_yaw=c.yaw[r], cand_variant=c.variant[r])
        if self.scene_kind == "box":
            _lib.fill(io, cand_scene=c.scene[r], forced_count=self.forced if last else None)
        return io

    def _validated_pairs(self, pairs_scene, sdf_scenes, names, sc) -> PairTables:
        """SDF env: the rejection loop of CrowdEnv.reset (crowd_env_2f.py:326-396) accepts a start iff no non-feet
        vertex of the two seed frames has sdf < 0.  For the room sampler that is a deterministic function of the
        start/target pair, so every pair is evaluated once here (sampler kernel -> SMPL-X + SDF kernel) and reset
        then draws uniformly among the accepted pairs - the same distribution as rejection sampling.  With a set of scenes, each
        scene's pairs are checked in that scene; an agent draws from its own scene's accepted pairs.
        RuntimeError when a scene has no pair that passes the start check.  Changes nothing on the env."""
        masks = [self._prevalidate_scene(pairs_scene[s], sdf_scenes[s], s, sc) for s in range(len(sdf_scenes))]
        for s, m in enumerate(masks):
            if not bool(m.any()):
                raise RuntimeError(f"no start/target pair of scene {names[s]!r} passes the SDF start check")
        pairs_all = pairs_scene[0] if len(masks) == 1 else torch.cat(pairs_scene)
        mask = masks[0] if len(masks) == 1 else torch.cat(masks)
        n = torch.tensor([int(m.sum()) for m in masks], dtype=torch.int64, device=self.dev)
        return PairTables(pairs_all, mask, pairs_all[mask].contiguous(), n, torch.cumsum(n, 0) - n)

    def replace_sdf_scenes(self, sdf_scenes: List[dict]):
        """Swap the scenes of a running SDF env for others (domain randomisation over layouts): as many scenes as now, of the
        current grid dimensions, [{sdf_dict, rings, pairs, name}, ...] like the constructor's.  Everything is built first - the
        scenes' bracket tables, the set, the edge table, each scene's pre-validated pairs -, then swapped; if a scene has no valid
        pair the RuntimeError of the constructor is raised and the env is untouched and usable.  After the swap the candidate
        pool and a captured graph are dropped (both hold the old scenes), all agents are reset and `scene_generation` counts up."""
        if self.scene_kind != "sdf":
            raise ValueError("replace_sdf_scenes: an SDF env only")
        sdf_scenes = list(sdf_scenes)
        if len(sdf_scenes) != len(self.sdf_scenes):
            raise ValueError(f"replace_sdf_scenes: {len(sdf_scenes)} scenes for an env over {len(self.sdf_scenes)} (agents keep their scene numbers)")
        ss = self._sdf_scene_set(sdf_scenes, dims=tuple(self.sdf_scenes[0].grid.shape))
        t = scene_tables(ss["edge_lists"])
        edges, edge_off = self._f32(t["edges"]), torch.tensor(t["edge_off"], dtype=torch.int32, device=self.dev)
        sc = _lib.fill(_lib.EnvScenes.from_buffer_copy(self._sc), edges=edges, edge_off=edge_off)
        tables = self._validated_pairs(ss["pairs_scene"], ss["sdf_scenes"], ss["scene_names"], sc)   # raises before anything of the env changed
        self._graph = None                                              # captured with the old grids' addresses
        self._pool, self._pool_pos, self._injected = None, 0, False     # drawn from the old scenes' pairs
        self._adopt_sdf_scene_set(ss)
        self.edges, self.edge_off, self._sc = edges, edge_off, sc
        self.pairs_all, self.pair_valid_mask, self.valid_pairs, self._vp_n, self._vp_off = tables
        self.scene_generation += 1
        return self.reset()

    def _prevalidate_scene(self, pairs_all, sdf, scene, sc, batch: int = 2048):
        N = pairs_all.shape[0]
        f32 = dict(dtype=torch.float32, device=self.dev)
        i32 = dict(dtype=torch.int32, device=self.dev)
        valid = torch.zeros(N, dtype=torch.bool, device=self.dev)
        for s in range(0, N, batch):
            n = min(batch, N - s)
            tmp = dict(state=torch.zeros(n, 2, 402, **f32), seed=torch.zeros(n, 2, 93, **f32), R0=torch.zeros(n, 3, 3, **f32),
                       T0=torch.zeros(n, 3, **f32), dist=torch.zeros(n, **f32), steps=torch.zeros(n, **i32),
                       wpath=torch.zeros(n, 2, 3, **f32), scene_idx=torch.full((n,), int(scene), **i32))
            obs = (torch.zeros(n, 2, 32, **f32), torch.zeros(n, **f32), torch.zeros(n, **f32))
            cands = Candidates(pairs_all[s:s + n].reshape(1, n, 1, 2, 3).contiguous(), None, None, None)
            io = self._reset_io(self._reset_io_fixed(1, obs), cands)
            _lib.check(self.lib.egx_env_reset(C.byref(self._ec), C.byref(sc), C.byref(_lib.fill(_lib.EnvState(), **tmp)), C.byref(io), n,
                                              _lib.current_stream_ptr()), "egx_env_reset")
            betas = self.betas[:1].repeat(n, 1).contiguous()
            out = self.bm.forward(tmp["seed"].reshape(n * 2, 93), betas, 2, want_joints=False, want_markers=False,
                                  sdf=sdf, R0=tmp["R0"], T0=tmp["T0"])
            valid[s:s + n] = out["pene_count"].reshape(n, 2).sum(1) == 0
        return valid

    # ------------------------------------------------------------------------------------------
    def _from_pool(self, fill) -> Candidates:
        """SDF and box scenes draw for CAND_POOL steps at a time, all rounds in one go (the same handful of RNG / gather launches
        per pool whatever the number of rounds, instead of some per step); a step's draws are slice k of the pool, handed to the
        reset kernel by address.  The retry rounds only read theirs for agents that are still pending."""
        if self._pool is None or self._pool_pos >= CAND_POOL:
            self._pool, self._pool_pos = fill(), 0
        c, k = self._cands, self._pool_pos
        self._pool_pos += 1
        for f, t in self._pool.items():   # the other fields stay what they are
            setattr(c, f, t[k])
        c.rounds = self.R
        return c

    def _sdf_pool(self) -> Dict[str, torch.Tensor]:
        A, K, g = self.A, self.K, self.gen
        if len(self.sdf_scenes) == 1:
            idx = torch.randint(0, self.valid_pairs.shape[0], (CAND_POOL * A * K,), generator=g, device=self.dev)
        else:   # each agent among its own scene's accepted pairs
            r = torch.randint(0, 1 << 30, (CAND_POOL, A, K), generator=g, device=self.dev)
            sc = self.scene_idx.long().view(1, A, 1)
            idx = (self._vp_off[sc] + r % self._vp_n[sc]).reshape(-1)
        return {"pairs": self.valid_pairs[idx].reshape(CAND_POOL, 1, A, K, 2, 3)}

    def _box_pool(self) -> Dict[str, torch.Tensor]:
        P, R, A, K, g = CAND_POOL, self.R, self.A, self.K, self.gen
        sc = torch.randint(0, self.num_scenes, (P * R * A * K,), generator=g, device=self.dev)
        pi = torch.randint(0, self.box_pairs.shape[1], (P * R * A * K,), generator=g, device=self.dev)
        u = torch.rand(P, R, A, K, generator=g, device=self.dev) * 2 - 1
        return {"pairs": self.box_pairs[sc, pi].reshape(P, R, A, K, 2, 3),
                "scene": sc.reshape(P, R, A, K).to(torch.int32),
                "variant": torch.randint(0, len(self.variant_starts), (P, R, A, K), generator=g, device=self.dev).to(torch.int32),
                "yaw": u * (2 * np.pi * 0.1)}                    # environments.py:529

    def _draw_crowd(self) -> Candidates:
        """every member restarts from its own fixed pair; written into the buffers in use"""
        A, K, g, c = self.A, self.K, self.gen, self._cands
        c.pairs[0].copy_(self.crowd_pairs)
        if self.agent_seeds is not None:
            c.variant[0].copy_(torch.arange(A, dtype=torch.int32, device=self.dev).reshape(A, K))
        else:
            c.variant[0].copy_(torch.randint(0, len(self.variant_starts), (A, K), generator=g, device=self.dev).to(torch.int32))
        u = torch.rand(A, K, generator=g, device=self.dev) * 2 - 1
        c.yaw[0].copy_(u * (2 * np.pi * 0.2))                    # environments.py:1100-1101 (CrowdMotion.gen_init_body)
        return c

    def sample_candidates(self):
        """Draw reset candidates for every agent (used only where the mask says so)."""
        self._cands = self._draw()

    def set_candidates(self, pairs, yaw=None, variant=None, scene=None):
        """Inject reset candidates (parity tests): pairs[A,r*K,2,3] = agent a's draws in the order the reference's loop would
        see them, for r <= reset_rounds rounds of K (the next reset runs exactly r launches).  An omitted yaw / variant / scene
        keeps the values in use, after a sampled reset the last draw's."""
        A, K, R, c = self.A, self.K, self.R, self._cands
        pairs = round_major(torch.as_tensor(pairs, dtype=torch.float32), A, K, R, (2, 3))
        r = pairs.shape[0]
        # the tensors in use may be views of the sampler's pool: injected draws get their own
        new = Candidates(c.pairs.clone(), c.yaw.clone(), c.variant.clone(), c.scene.clone(), r)
        new.pairs[:r].copy_(pairs)
        for name, t, dt in (("yaw", yaw, torch.float32), ("variant", variant, torch.int32), ("scene", scene, torch.int32)):
            if t is not None:
                getattr(new, name)[:r].copy_(torch.as_tensor(t, dtype=dt).reshape(A, r, K).transpose(0, 1))
        self._cands, self._injected = new, True

    def _launch_reset(self, mask):
        """Launch the reset kernel over the candidates in use (again, when called twice: same draws, same state)."""
        c = self._cands
        for r in range(c.rounds):
            io = self._reset_io(self._rio, c, r, mask if r == 0 else self.pending, last=r == c.rounds - 1)
            _lib.check(self.lib.egx_env_reset(C.byref(self._ec), C.byref(self._sc), C.byref(self._st), C.byref(io), self.A,
                                              _lib.current_stream_ptr()), "egx_env_reset")

    def forced_accepts(self) -> int:
        """Starts committed although none of an agent's reset_rounds x K draws passed the start check, since construction
        (one host sync).  0 means every episode so far started like the reference's `while True` loop would have started it."""
        return int(self.forced.item())

    def obs(self) -> Dict[str, torch.Tensor]:
        return {"state": self.state, "egosensing": self.obs_ego, "dist": self.obs_dist, "time": self.obs_time}

    def reset(self, mask: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """New episodes for the masked agents (all without a mask), from injected candidates if any wait, else fresh draws."""
        if not self._injected:
            self.sample_candidates()
        self._injected = False
        self._launch_reset(mask)
        if mask is None:
            self.invalid.zero_()
        return self.obs()

    def clear_invalid(self, mask: Optional[torch.Tensor] = None):
        """Forget the EgoBody filter flags (`invalid`, OR-accumulated by the step kernel) of the masked agents (all without a
        mask).  A full `reset()` starts new episodes everywhere and clears them; the auto-reset inside `step` does not, so that
        the evaluation driver can still read which scenes tripped a filter after their episodes ended."""
        if mask is None:
            self.invalid.zero_()
        else:
            self.invalid.mul_((mask == 0).to(self.invalid.dtype))

    # ------------------------------------------------------------------------------------------
    def _step_core(self):
        lib, A = self.lib, self.A
        st = _lib.current_stream_ptr()
        # C-VAE decode + regressor (crowd_env_2f.py:109)
        self.prior.sample_prior_into(self.state[:, 0], self.state[:, 1], 804, self.betas, self._z_in, self.Y_gen, self.Yb_gen)
        _lib.check(lib.egx_assemble_params(_lib.ptr(self.seed), _lib.ptr(self.Yb_gen), A, _lib.ptr(self.pred_params), st),
                   "egx_assemble_params")
        # SMPL-X on A*20 bodies; SDF counts fused (crowd_env_2f.py:133-175)
        if self.profile_events:
            ev0, ev1 = self.profile_events.pop(0)
            _lib.check(lib.egx_profile_next_lbs(ev0, ev1), "egx_profile_next_lbs")
        self.bm.forward(self.pred_params.reshape(A * 20, 93), self.betas, 20, want_verts=False,
                        sdf=self.sdf, R0=self.R0 if self.sdf is not None else None,
                        T0=self.T0 if self.sdf is not None else None, out=self._lbs_out,
                        agent_scene=self.scene_idx if isinstance(self.sdf, SdfSceneSet) else None)
        # VPoser embedding of the 20 body poses (crowd_env_2f.py:197-198)
        self.vposer.encode_mean_into(self.pred_params.reshape(A * 20, 93)[:, 6:], 93, A * 20, self.vp_emb)
        _lib.check(lib.egx_env_step_post(C.byref(self._ec), C.byref(self._sc), C.byref(self._st), C.byref(self._io), A, st),
                   "egx_env_step_post")

    def check_finite(self, all_ranks: bool = False):
        """Raise if any step since the last call produced a non-finite reward / target distance (one host sync; the
        reference stops in pdb at the NaN/Inf checks of crowd_env_2f.py:287-297).  `all_ranks`: MAX-reduce the counter over
        the data-parallel ranks first, so that all of them raise together."""
        if all_ranks:
            import torch.distributed as dist
            dist.all_reduce(self.nonfinite, op=dist.ReduceOp.MAX)
        n = int(self.nonfinite.item())
        if n:
            self.nonfinite.zero_()
            raise FloatingPointError(f"{n} agent-steps produced non-finite rewards since the last check")

    def step(self, actions: torch.Tensor, auto_reset: bool = True):
        """actions[A,128] -> (obs, reward[A], terminated[A] int32).  Returned tensors are views of internal
        buffers, valid until the next call.  With auto_reset, finished agents are re-initialised and their
        entries of obs are the reset observation (tianshou Collector semantics)."""
        if actions.shape != (self.A, 128):
            raise ValueError(f"actions must be [{self.A},128], got {tuple(actions.shape)}")
        direct = (not self.use_graph and actions.is_cuda and actions.dtype == torch.float32 and actions.is_contiguous()
                  and actions.device == self.z.device)
        self._z_in = actions if direct else self.z      # the kernels read the caller's tensor where that is safe: no copy
        if not direct:
            self.z.copy_(actions)
        if self.use_graph:
            if self._graph is None:
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    self._step_core()
                self._graph = g
            self._graph.replay()
        else:
            self._step_core()
        return self.reset(self.terminated) if auto_reset else self.obs(), self.reward, self.terminated


class CrowdEnv:
    """Single-agent gym-style view with the reference's interface (crowd_env_2f.py:34-51,78,320,519)."""

    def __init__(self, vec_env: VecCrowdEnv):
        if vec_env.A != 1:
            raise ValueError("CrowdEnv wraps a 1-agent VecCrowdEnv")
        self.vec = vec_env
        from .spaces import crowd_env_spaces
        self.action_space, self.observation_space = crowd_env_spaces()   # crowd_env_2f.py:49-51 (gymnasium's when installed)

    def seed(self, seed):
        self.vec.gen.manual_seed(int(seed))

    def _obs0(self):
        o = self.vec.obs()
        return {"state": o["state"][0], "egosensing": o["egosensing"][0], "dist": o["dist"][0:1], "time": o["time"][0:1]}

    def reset(self, seed=None, options=None):
        if seed is not None:
            self.seed(seed)
        self.vec.reset()
        return self._obs0(), {}

    def step(self, action_z):
        a = torch.as_tensor(action_z, dtype=torch.float32, device=self.vec.dev).reshape(1, 128)
        _, rew, term = self.vec.step(a, auto_reset=False)
        return self._obs0(), float(rew[0].item()), bool(term[0].item()), False, {}


class CrowdGroupEnv:
    """G interacting members per scene, S independent scenes (the reference's main_crowd_eval.py runs S = 1, G = 4 with
    `DummyCrowdVectorEnv`).  Member k of every scene lives in sub-environment k; all share one table of world-space
    marker boxes.  `step` walks the members in order, so member k sees the boxes members 0..k-1 published in THIS round
    and those of k+1.. from the previous round - the ordering of dummy_vector_env.py:81-84."""

    def __init__(self, num_scenes: int, start_target, body_model, prior, vposer, cfg=None, seed=0, keep_rollout=False,
                 motion_seed=None, floor_half: float = 4.0, device="cuda", scene_rings=None, static_scene: bool = False,
                 agent_seeds=None, vp_thresh: float = 11.0, goal_terminates: bool = True, gender: str = "male"):
        """`scene_rings` ... `goal_terminates`: the EgoBody evaluation (main_egobody_eval.py / crowd_env_egobody_eval.py, G = 2):
        the walkable polygon of the scene's navmesh as exterior (:402), `agent_seeds[k][s]` = the two seed frames + betas of
        member k in scene s (Egobody.gen_init_body, environments.py:679-765), pose filter at 14 (:229), only max_depth
        terminates (:378).  `static_scene=True` reproduces what `Polygon(self.scene_poly, holes)` (:824) evaluates to when
        the shell is already a Polygon - shapely returns that polygon, the other person never becomes a hole."""
        st = np.asarray(start_target, np.float32)          # [G,S,2,3]
        self.G, self.S = int(st.shape[0]), int(num_scenes)
        assert st.shape[1] == self.S
        self.bbox = torch.zeros(self.G, self.S, 4, dtype=torch.float32, device=device)
        self.members = [VecCrowdEnv(self.S, body_model, prior, vposer, scene_kind="crowd", cfg=cfg, seed=seed + 17 * k,
                                    keep_rollout=keep_rollout, motion_seed=motion_seed, crowd_bbox=self.bbox, crowd_member=k,
                                    crowd_pairs=st[k], crowd_floor_half=floor_half, device=device, crowd_rings=scene_rings,
                                    crowd_static=static_scene, agent_seeds=None if agent_seeds is None else agent_seeds[k],
                                    vp_thresh=vp_thresh, goal_terminates=goal_terminates, gender=gender) for k in range(self.G)]
        self.gender = gender

    def invalid(self) -> torch.Tensor:
        """[S] OR of the members' filter flags (1: pelvis left the scene polygon early, 2: unrealistic pose)."""
        out = self.members[0].invalid.clone()
        for m in self.members[1:]:
            out |= m.invalid
        return out

    def reset(self):
        """Every member publishes its initial box (constructor of crowd_env_crowd_eval.CrowdEnv, :54-75) before anyone
        builds its first observation (DummyCrowdVectorEnv.__init__ -> update_holes_for_each_agent)."""
        for m in self.members:
            m.reset()                    # new episodes everywhere (the filter flags of the previous ones are history)
        obs = []
        for m in self.members:
            m._launch_reset(None)        # same candidates: identical state, observation now sees all boxes
            obs.append(m.obs())
        return obs

    def step(self, actions, reset_done: bool = True):
        """actions: list of G tensors [S,128].  Returns per-member (obs, reward, terminated)."""
        out = []
        for k, m in enumerate(self.members):
            o, r, t = m.step(actions[k], auto_reset=False)
            r, t = r.clone(), t.clone()
            if reset_done:                # a finished member restarts from its own fixed start (collector reset)
                m.reset(m.terminated)
            out.append((m.obs(), r, t))
        return out
