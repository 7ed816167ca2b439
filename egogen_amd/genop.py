"""`GAMMAPrimitiveComboGenOP` (motion/models/models_GAMMA_primitive.py:1099-1425, constructed by
crowd_ppo/primitive_model.py:69): the interface to a trained motion prior outside an environment - one primitive from a motion
seed (`generate`), the file writer of the primitive evaluation (`generate_primitive_to_files`), and, new here, a chain of
primitives with the re-canonicalisation between them on the device (`generate_sequence`, kernel egx_primitive_advance): the
motion-only part of `CrowdEnv.step` (crowd_ppo/crowd_env_2f.py:109-155, 238-265) without scene, rewards or egosensing; and
`generate_sequence_to_goal`, the greedy best-of-N search over such a chain: per primitive N candidates are scored with the
arguments of the env's reward terms (:171-235) against a goal and an SDF scene, and every candidate of the next primitive
continues from the best one (kernels egx_primitive_select, egx_primitive_advance_select); with `beam_width` W > 1 it is a beam
search that keeps the best W partial paths per sequence (kernels egx_primitive_beam_select, egx_primitive_advance_beam,
egx_beam_backtrack).  With `geodesic=` (a `GeodesicField`, egogen_amd/geodesic.py) the goal term of either search is the distance
along the walkable raster of the scene instead of the straight line (entries egx_primitive_select_field,
egx_primitive_beam_select_field).  With `obstacles=` (a `MovingObstacles`, egogen_amd/obstacles.py) either search also avoids
other people's recorded tracks: a clearance term in the cost and a veto on overlap (entries egx_primitive_select_obstacles,
egx_primitive_beam_select_obstacles; with `obstacle_model="markers"` the recorded people are their 67 world markers per frame: entry
egx_obstacle_marker_clearance, csrc/genop_obstacle_markers.hip, ahead of egx_primitive_select_obstacle_markers /
egx_primitive_beam_select_obstacle_markers).  With `groups=` (ids, or a `PersonGroups`, egogen_amd/crowd.py) the sequences of one group of the
greedy search see each other: after the selection the members choose again against each other's current choices (entry
egx_primitive_select_joint, csrc/genop_joint.hip; with `pair_model="markers"` the people are their 67 blended markers, not
cylinders: entries egx_pair_marker_dist, egx_primitive_select_joint_markers, csrc/genop_joint_markers.hip), and the hand-off
continues from that joint choice.  With `lookahead=` H > 0 the cylinder models of `obstacles=` and `groups=` see H further
primitives ahead: everybody is predicted to repeat the displacement of the own primitive (entries egx_obstacle_ahead_clearance,
csrc/genop_obstacle_ahead.hip, ahead of the *_obstacle_markers selection entries, and egx_primitive_select_joint_ahead,
csrc/genop_joint_ahead.hip, in the place of egx_primitive_select_joint).  With `policy=` (a
`PolicyProposal`, egogen_amd/proposal.py) the candidates of the greedy search are no longer all drawn from N(0, I): per primitive
every sequence senses its surroundings (entry egx_primitive_observe, csrc/genop_policy.hip), the trained policy's actor proposes
mu, logvar over the latent, and the candidate rows become mu, samples round it and a share of prior samples (entry
egx_policy_propose); the selection scores them as before.  With `route=` (a `Routes`, egogen_amd/route.py) every sequence of the
greedy search walks an itinerary of waypoints: one launch per primitive after the hand-off (entry egx_route_advance,
csrc/genop_route.hip) moves a per-sequence cursor and rewrites the goal buffer every kernel of the loop reads.

The three chains share their host path: `_chain_state` builds the state dict (checked inputs, defaults, the loop's buffers, the
records) for b seeds of M rows each, `_primitive` launches what every primitive begins with (prior, parameter assembly, body
model), `_handoff_lead` / `_select_lead` build the leading arguments common to the hand-off and to the selection entries once per
loop, and `_result` turns the records into a `PrimitiveSequence`.  `_advance_loop(K, B, s)`, `_search_loop(K, b, N, s)` and
`_beam_loop(K, b, W, N, s)` are launches only and differ in what follows the prefix.

Differences from the reference, all in `generate` unless noted:
  * `t_his=None` means the model's t_his (the reference computes `20 - None` and fails);
  * only t_his == 2 is supported (egx_sample_prior takes two history frames): anything else raises ValueError;
  * with `return_z=True` a supplied `z` is used and returned (the reference ignores it on that path);
  * inputs may be numpy or torch on either path; `betas` may be (10,), (1,10) or (b,10);
  * `generate_ppo` is not built: nothing in the reference calls it, and its `policy_model(X, obj_points=, target_ori=,
    local_map=)` signature belongs to no class in the tree."""
from __future__ import annotations

import ctypes as C
import os
import pickle
from typing import Optional, Union

import numpy as np
import torch

from . import _lib
from .models import GAMMAPrimitiveCombo

T_ALL, T_PRED, NM3, XB = 20, 18, 201, 93
MAX_CANDIDATES = 256        # EGX_MAX_CANDIDATES of include/egogen_hip.h
MAX_BEAM = 32               # EGX_MAX_BEAM
NULL_FIELD = (None, None, 0.0, 0, 0, 0, None)      # the field arguments of a selection entry without a field
MAX_LOOKAHEAD = 8           # EGX_MAX_LOOKAHEAD
OBSTACLE_MODELS = ("cylinder", "markers")       # what a recorded person of `obstacles=` is: a cylinder round the pelvis, or its 67 world markers
SEARCH_WEIGHTS = {"goal": 1.0, "skate": 1.0, "floor": 1.0, "pene": 1.0, "face": 0.0}
GENERATE_PPO_NOT_BUILT = ("generate_ppo is not built: nothing in the reference calls it, and its policy_model(X, obj_points=, "
                          "target_ori=, local_map=) signature belongs to no class in the tree")


def _section(cfg, name):
    """`cfg.modelconfig` (OmegaConf / namespace) or `cfg['modelconfig']` (plain yaml)."""
    return cfg[name] if isinstance(cfg, dict) else getattr(cfg, name)


def _vp(t):
    """`_lib.ptr` without its checks, for the per-primitive slices of the records (contiguous by construction, never None)"""
    return C.c_void_p(t.data_ptr())


def _load_ckpt(candidates):
    """The first readable checkpoint of `candidates` (the reference's try / except chain) -> (state dict, path)."""
    err = None
    for f in candidates:
        try:
            return torch.load(f, map_location="cpu")["model_state_dict"], f
        except (OSError, FileNotFoundError) as e:
            err = e
    raise FileNotFoundError(f"none of {list(candidates)} could be read: {err}")


def _person_groups(groups, data, beam_width, pair_weight, pair_margin, body_radius, joint_sweeps, pair_model="cylinder", pair_skin=0.05,
                   n_candidates=1):
    """The `groups=` argument of `generate_sequence_to_goal` checked on the host, before any device work -> a `PersonGroups` not yet
    on a device (None without groups).  ValueError: groups with a beam, ids of another length than the b seeds of `data`, a group
    of more than 32, sweeps outside [1, 8], a negative margin or radius, a non-finite weight; an unknown pair_model, "markers"
    without groups, a negative or non-finite pair_skin, a distance table of the marker model above PAIR_TABLE_CAP_BYTES."""
    from .crowd import MAX_SWEEPS, PAIR_MODELS, PAIR_TABLE_CAP_BYTES, PersonGroups
    if pair_model not in PAIR_MODELS:
        raise ValueError(f"pair_model must be one of {PAIR_MODELS}, got {pair_model!r}")
    if not (float(pair_skin) >= 0 and np.isfinite(float(pair_skin))):
        raise ValueError(f"pair_skin must be finite and not negative, got {pair_skin}")
    if groups is None:
        if pair_model == "markers":
            raise ValueError('pair_model="markers" is a model of the joint step: it needs groups=')
        return None
    if beam_width > 1:
        raise ValueError(f"groups= is the greedy search only: beam_width must be 1 with it, got {beam_width}")
    shape = tuple(np.shape(data))
    if len(shape) != 3:
        raise ValueError(f"data must be [>=2,b,>=201], got {shape}")
    b = shape[1]
    if isinstance(groups, PersonGroups):
        if len(groups.ids) != b:
            raise ValueError(f"groups must hold {b} ids, one per sequence, got {len(groups.ids)}")
    else:
        groups = PersonGroups.from_ids(groups, b)
    if int(joint_sweeps) != joint_sweeps or not 1 <= int(joint_sweeps) <= MAX_SWEEPS:
        raise ValueError(f"joint_sweeps must be an integer in [1, {MAX_SWEEPS}], got {joint_sweeps}")
    if not (float(pair_margin) >= 0 and float(body_radius) >= 0 and np.isfinite(float(pair_weight))):
        raise ValueError(f"pair_margin and body_radius must not be negative and pair_weight finite, got {pair_margin}, {body_radius}, "
                         f"{pair_weight}")
    if pair_model == "markers" and groups.pair_table_bytes(n_candidates) > PAIR_TABLE_CAP_BYTES:
        raise ValueError(f"the marker model's distance table would take {groups.pair_table_bytes(n_candidates)} bytes "
                         f"({int(groups.pair_offsets[-1])} pairs x {int(n_candidates)}^2 rows x 72), above the cap of {PAIR_TABLE_CAP_BYTES}: "
                         f"fewer candidates, smaller groups, or the cylinder model")
    return groups


def _checked_lookahead(lookahead, lookahead_slack, obstacles, groups, obstacle_model, pair_model):
    """The `lookahead=` / `lookahead_slack=` arguments of `generate_sequence_to_goal` checked on the host, before any device work ->
    (H, slack).  ValueError: H not an integer in [0, 8], a negative or non-finite slack, H > 0 with neither obstacles nor groups, H > 0
    with a marker model (look-ahead is built for the cylinder models only)."""
    try:
        H = int(lookahead)
        whole = not isinstance(lookahead, bool) and H == lookahead
    except (TypeError, ValueError, OverflowError):
        H, whole = 0, False
    if not whole or not 0 <= H <= MAX_LOOKAHEAD:
        raise ValueError(f"lookahead must be an integer in [0, {MAX_LOOKAHEAD}], got {lookahead!r}")
    try:
        slack = float(lookahead_slack)
    except (TypeError, ValueError):
        slack = float("nan")
    if not (slack >= 0 and np.isfinite(slack)):
        raise ValueError(f"lookahead_slack must be finite and not negative, got {lookahead_slack!r}")
    if H > 0 and obstacles is None and groups is None:
        raise ValueError("lookahead > 0 is about when the other people are seen: it needs obstacles= or groups=")
    if H > 0 and (obstacle_model == "markers" or pair_model == "markers"):
        raise ValueError('lookahead > 0 is built for the cylinder models only: not with obstacle_model="markers" or pair_model="markers"')
    return H, slack


def _checked_route(route, data, goal, beam_width, goal_thresh):
    """The `route=` argument of `generate_sequence_to_goal` checked on the host, before any device work -> the `Routes` (None without
    one).  TypeError for anything but a `Routes`; ValueError: another number of routes than the b seeds of `data`, a route with a
    beam, a `goal` that is neither None nor the routes' last waypoints, a pass_radius below goal_thresh."""
    if route is None:
        return None
    from .route import Routes
    if not isinstance(route, Routes):
        raise TypeError(f"route must be None or a Routes, got {type(route).__name__}")
    if beam_width > 1:
        raise ValueError(f"route= is the greedy search only: beam_width must be 1 with it, got {beam_width}")
    shape = tuple(np.shape(data))
    if len(shape) != 3:
        raise ValueError(f"data must be [>=2,b,>=201], got {shape}")
    if len(route) != shape[1]:
        raise ValueError(f"route must hold {shape[1]} routes, one per sequence, got {len(route)}")
    if goal is not None:
        g = np.asarray(goal.detach().cpu() if torch.is_tensor(goal) else goal, np.float32)
        if g.shape not in ((3,), (shape[1], 3)) or not np.array_equal(np.broadcast_to(g, (shape[1], 3)), route.last()):
            raise ValueError("goal contradicts the route: with route= it must be None or route.last(), the last waypoint of every route")
    if route.pass_radius < float(goal_thresh):
        raise ValueError(f"pass_radius {route.pass_radius} is below goal_thresh {goal_thresh}: a point the selection calls reached must "
                         f"also count as passed")
    return route


class PrimitiveSequence:
    """What `generate_sequence` returns: K primitives of b sequences.
    markers [K,b,20,67,3] blended markers, params [K,b,20,93], rotmat [K,b,3,3] / transl [K,b,3] the world frame each primitive
    is expressed in, pelvis [K,b,20,3], z [K,b,128]; betas [b,10]; R0 [b,3,3] / T0 [b,3] the frame after the last primitive.
    A result of `generate_sequence_to_goal` holds the chosen candidates in those fields and, in `search`, what the selection saw:
    goal [b,3], choice [K,b], cost [K,b,N], cost_terms [K,b,N,5] (dist, skate, floor, pene, face), colliding [K,b,N],
    status [K,b] (bit 0: the chosen candidate collides), goal_dist [K,b], n_valid [b] (primitives up to and including the first
    whose chosen candidate ends within goal_thresh of the goal, K if none does); `primitives` and `save` stop at n_valid;
    geo_dist [K,b], with a `geodesic=` field the field's value at the chosen candidate's last pelvis (cost_terms[..., 0] of the
    chosen row, which then holds the field's value, not the Euclidean distance), else None.
    A beam result (beam_width W > 1) holds the returned path in the same fields: cost / cost_terms / colliding are [K,b,W*N(,5)],
    choice [K,b] the path's row within its W*N, status [K,b] the path node's bits (0: collides, 1: non-finite row, 2: non-finite
    hand-off); and beam_width, path_slot [K,b], parent / beam_row / path_cost / beam_status [K,b,W], which a greedy result has as
    None.  With `obstacles=`: obstacle_term [K,b,M] (metres), clearance [K,b,M] (metres, +inf for an empty set) and obstacle_hit
    [K,b,M] of every row (M = N, or W*N for a beam), colliding then includes the hits; None without obstacles.  `search` then also
    holds obstacle_model ("cylinder" / "markers") and obstacle_skin (metres); with "markers" clearance is the distance between the
    nearest markers of the candidate and of a recorded person minus obstacle_skin, in 3-D.
    With `groups=` (S = joint_sweeps, G groups): groups [b] the ids; individual_choice [K,b] what the selection chose before the
    members saw each other (choice is the joint choice, choice_trace[:, -1]); pair_term / pair_clearance / joint_cost (metres, metres,
    cost) and pair_hit [K,S,b,N] of every row as evaluated in each sweep; choice_trace [K,S,b] the choices after each sweep;
    joint_changed [K,S,G] the members of a group that changed their choice in a sweep (0: a fixed point); crowd_clearance [K,b] the
    clearance of the chosen track against the other members' chosen tracks and crowd_hit [K,b] = crowd_clearance < 0: did the crowd
    as written overlap.  cost / colliding stay what the selection wrote; status follows the joint choice.  None without groups.
    `search` also holds pair_model ("cylinder" / "markers") and pair_skin (metres); with "markers" the clearances are distances
    between the two people's nearest blended markers minus pair_skin, in 3-D.
    With obstacles or groups `search` also holds lookahead (H, 0: none) and lookahead_slack (metres per primitive); with H > 0
    clearance / obstacle_term / obstacle_hit and pair_clearance / pair_term / pair_hit are those of the look-ahead c_t (the least of
    the present clearance and the predicted ones, each floored at 0 and raised by h * slack), crowd_clearance / crowd_hit stay the present's.
    With `policy=PolicyProposal(..., sense_people=True)`: policy_sense_people True, people_box [K,b,4] (minx, miny, maxx, maxy) the
    world xy box of every sequence's two seed frames' markers at each primitive and obs_people_count [K,b] the holes its observation
    was cast against; False, None, None with a policy that does not sense people, None without a policy.
    With `route=`: route_waypoints [b,P,3] / route_count [b] the routes, pass_radius; route_goal [K,b,3] the waypoint primitive k was
    scored against, route_pass_dist [K,b] the least horizontal distance of its 18 predicted frames to that waypoint (NaN for a NaN
    position), route_cursor [K,b] the cursor after primitive k.  goal is then the last waypoint of every route; goal_dist[k] and
    cost_terms[..., 0] stay what the selection wrote: the distance to route_goal[k].  None without a route."""
    SEARCH_FIELDS = ("goal", "choice", "cost", "cost_terms", "colliding", "status", "goal_dist", "n_valid", "geo_dist")
    BEAM_FIELDS = ("beam_width", "path_slot", "parent", "beam_row", "path_cost", "beam_status")
    OBSTACLE_FIELDS = ("obstacle_term", "clearance", "obstacle_hit")
    JOINT_FIELDS = ("individual_choice", "pair_term", "pair_clearance", "pair_hit", "joint_cost", "choice_trace", "joint_changed",
                    "crowd_clearance", "crowd_hit", "groups")
    POLICY_FIELDS = ("policy_mu", "policy_logvar", "obs_state", "obs_egosensing", "obs_dist", "obs_time", "policy_temperature",
                     "policy_n_mean", "policy_n_policy", "policy_ray_len", "policy_max_depth")
    PEOPLE_FIELDS = ("people_box", "obs_people_count", "policy_sense_people")
    ROUTE_FIELDS = ("route_waypoints", "route_count", "route_cursor", "route_goal", "route_pass_dist", "pass_radius")

    def __init__(self, markers, params, rotmat, transl, pelvis, z, betas, gender, R0, T0, search: Optional[dict] = None):
        self.markers, self.params, self.rotmat, self.transl, self.pelvis, self.z = markers, params, rotmat, transl, pelvis, z
        self.betas, self.gender, self.R0, self.T0 = betas, gender, R0, T0
        self.search = search
        for k in self.SEARCH_FIELDS:
            setattr(self, k, None if search is None else search[k])
        for k in self.BEAM_FIELDS + self.OBSTACLE_FIELDS + self.JOINT_FIELDS + self.POLICY_FIELDS + self.PEOPLE_FIELDS + self.ROUTE_FIELDS:
            setattr(self, k, None if search is None else search.get(k))

    def primitives(self, i: int) -> list:
        """Sequence i as the list of 8-item records `utils.save_rollout_results` takes (crowd_env_2f.py:155)."""
        n = self.markers.shape[0] if self.n_valid is None else int(self.n_valid[i])
        return [[self.markers[k, i:i + 1], self.params[k, i:i + 1], self.betas[i:i + 1], self.gender, self.rotmat[k, i],
                 self.transl[k, i:i + 1], self.pelvis[k, i:i + 1], "2-frame"] for k in range(n)]

    def save(self, outfolder: str, i: int, man_id=None) -> str:
        """`motion_<man_id>.pkl` of sequence i with a two-point wpath in the world frame: first pelvis, then the goal of a
        goal-steered result, else the last pelvis.  A result searched with `route=` writes the whole route: first pelvis, then
        every waypoint."""
        from .utils import save_rollout_results
        as_t = lambda x: torch.as_tensor(x)
        first = as_t(self.rotmat[0, i]) @ as_t(self.pelvis[0, i, 0]) + as_t(self.transl[0, i])
        if self.route_waypoints is not None:
            way = as_t(self.route_waypoints[i][:int(self.route_count[i])]).to(first)
            scene = {"wpath": torch.cat([first[None], way]), "navmesh_path": None}
            return save_rollout_results(scene, self.primitives(i), outfolder, man_id=man_id)
        if self.goal is not None:
            last = as_t(self.goal[i]).to(first)
        else:
            last = as_t(self.rotmat[-1, i]) @ as_t(self.pelvis[-1, i, -1]) + as_t(self.transl[-1, i])
        scene = {"wpath": torch.stack([first, last]), "navmesh_path": None}
        return save_rollout_results(scene, self.primitives(i), outfolder, man_id=man_id)


class GAMMAPrimitiveComboGenOP:
    """the interface to GAMMA when using it to produce motions"""

    def __init__(self, predictorcfg, regressorcfg, testconfig):
        self.dtype = torch.float32
        if not torch.cuda.is_available():
            raise _lib.EgxError("no HIP device visible - the motion prior has no CPU fallback")
        _lib.load()
        self.device = torch.device("cuda", index=testconfig.get("gpu_index", 0))
        self.predictorcfg, self.regressorcfg, self.testconfig = predictorcfg, regressorcfg, testconfig
        pm, rm = _section(predictorcfg, "modelconfig"), _section(regressorcfg, "modelconfig")
        self.use_cont = rm.get("use_cont", False)
        self.t_his = pm["t_his"]
        self.var_seed_len = pm.get("var_seed_len", False)
        self.model: Optional[GAMMAPrimitiveCombo] = None
        self.body_model = None

    # ------------------------------------------------------------------------------------------------------------------
    def build_model(self, load_pretrained_model=False, body_model=None):
        """:1116-1148.  load_pretrained_model: predictor `epoch-400.ckp` (else `epoch-200.ckp`) and regressor `epoch-100.ckp`
        from the two configs' trainconfig.save_dir (the loader of setup_world.build_motion_prior); otherwise the combo
        checkpoint `epoch-120.ckp` (else `epoch-10.ckp`) of testconfig['ckpt_dir'], the file train_combo.py writes.  A missing
        file raises, as in the reference.  `body_model`: the BodyModelHandle of the regressor's gender, needed by
        `generate_sequence` only."""
        pm, rm = _section(self.predictorcfg, "modelconfig"), _section(self.regressorcfg, "modelconfig")
        if load_pretrained_model:
            from .setup_world import build_motion_prior
            pdir = _section(self.predictorcfg, "trainconfig")["save_dir"]
            rdir = _section(self.regressorcfg, "trainconfig")["save_dir"]
            _, f = _load_ckpt([os.path.join(pdir, "epoch-400.ckp"), os.path.join(pdir, "epoch-200.ckp")])
            print("[INFO] --load pre-trained predictor: {}".format(f))
            _, f = _load_ckpt([os.path.join(rdir, "epoch-100.ckp")])
            print("[INFO] --load pre-trained regressor: {}".format(f))
            GAMMAPrimitiveCombo(pm, rm)      # the configs must describe the network the loader builds
            self.model = build_motion_prior(device=self.device, ckpt_dirs=(pdir, rdir))
        else:
            self.model = GAMMAPrimitiveCombo(pm, rm)
            cdir = self.testconfig["ckpt_dir"]
            sd, f = _load_ckpt([os.path.join(cdir, "epoch-120.ckp"), os.path.join(cdir, "epoch-10.ckp")])
            self.model.load_state_dict(sd)
            print("[INFO] --load combo model: {}".format(f))
            self.model.to(self.device).eval()
        if body_model is not None:
            self.body_model = body_model

    def _blend_params(self, body_params, t_his=None):
        """:1150-1163, in place on [t,b,93]: frames t_his and t_his + 1 become the mean of their neighbours, pose part only."""
        if t_his is None:
            t_his = self.t_his
        start_idx = 6
        for t in (t_his, t_his + 1):
            body_params[t, :, start_idx:] = (body_params[t - 1, :, start_idx:] + body_params[t + 1, :, start_idx:]) / 2.0
        return body_params

    # ------------------------------------------------------------------------------------------------------------------
    def _dev(self, x, what):
        if isinstance(x, np.ndarray):
            x = torch.from_numpy(np.ascontiguousarray(x))
        elif not torch.is_tensor(x):
            raise TypeError(f"{what} must be a numpy array or a torch tensor, got {type(x).__name__}")
        return x.detach().to(self.device, self.dtype)

    def _seed_inputs(self, data, bparams, betas, n_gens, t_his):
        if self.model is None:
            raise _lib.EgxError("build_model() first")
        if t_his is None:
            t_his = self.t_his
        if t_his != 2:
            raise ValueError(f"only t_his == 2 is supported (egx_sample_prior takes two history frames), got {t_his}")
        X = self._dev(data, "data")[:t_his, :, :NM3]
        Xb = self._dev(bparams, "bparams")[:t_his]
        if X.dim() != 3 or X.shape[0] != 2 or X.shape[2] != NM3 or Xb.shape != (2, X.shape[1], XB):
            raise ValueError(f"data must be [>=2,b,>=201] and bparams [>=2,b,93], got {tuple(data.shape)} / {tuple(bparams.shape)}")
        bt = self._dev(betas, "betas").reshape(-1, 10)
        if bt.shape[0] not in (1, X.shape[1]):
            raise ValueError(f"betas must be (10,), (1,10) or (b,10) with b = {X.shape[1]}, got {tuple(betas.shape)}")
        if n_gens > 0:
            X, Xb = X.repeat(1, n_gens, 1), Xb.repeat(1, n_gens, 1)
            if bt.shape[0] != 1:
                bt = bt.repeat(n_gens, 1)
        if bt.shape[0] == 1:
            bt = bt.repeat(X.shape[1], 1)
        return X.contiguous(), Xb.contiguous(), bt.contiguous()

    def generate(self, data: Union[torch.Tensor, np.ndarray], bparams: Union[torch.Tensor, np.ndarray],
                 betas: Union[torch.Tensor, np.ndarray], n_gens: int = -1, to_numpy: bool = True, return_z: bool = False,
                 param_blending: bool = True, t_his=None, z: Union[None, torch.Tensor, np.ndarray] = None):
        """generate motion primitives based on a motion seed X (:1166-1249)

        Args:
            - data: the motion seed, with the shape [t,b,d]
            - bparams: the body parameters of the motion seed, with the shape [t,b,d]
            - betas: body shape, (10,), (1,10) or (b,10)
            - n_gens: how many motions are generated per seed. If -1, it has the same batch size with the input.
            - to_numpy: produce numpy if true
            - return_z: return the latent variables if set to True
            - param_blending: smooth the body poses, to eliminate the first-frame jump and compensate the regressor inaccuracy
            - t_his: frames in the motion seed; None = the model's t_his; only 2 is supported (ValueError otherwise)
            - z: latent variables [b',128] (b' = b * n_gens when n_gens > 0), or None for N(0, I)

        Returns Y [b',20,201] (seed and predicted markers), Yb [b',20,93] (seed and regressed body parameters, rotations in
        axis-angle) and, with return_z, z.  Differences from the reference: see the module docstring."""
        X, Xb, bt = self._seed_inputs(data, bparams, betas, n_gens, t_his)
        nb = X.shape[1]
        if z is None:
            z = torch.randn(nb, self.model.predictor.z_dim, device=self.device)
        else:
            z = self._dev(z, "z")
            if z.shape != (nb, self.model.predictor.z_dim):
                raise ValueError(f"z must be [{nb},{self.model.predictor.z_dim}], got {tuple(z.shape)}")
        Y_pred, Yb_pred = self.model.sample_prior(X, betas=bt, z=z)
        Y = torch.cat((X, Y_pred), dim=0)
        Yb = torch.cat((Xb, Yb_pred), dim=0)
        if param_blending:
            Yb = self._blend_params(Yb)
        Y, Yb = Y.permute(1, 0, 2), Yb.permute(1, 0, 2)     # from [t,b,d] to [b,t,d]
        if to_numpy:
            Y, Yb = Y.cpu().numpy(), Yb.cpu().numpy()
            z = z.cpu().numpy()
        return (Y, Yb, z) if return_z else (Y, Yb)

    def generate_ppo(self, *args, **kwargs):
        raise NotImplementedError(GENERATE_PPO_NOT_BUILT)

    # ------------------------------------------------------------------------------------------------------------------
    def _chain_state(self, X, seed, bt, K, M, z, reproj_factor, R0, T0) -> dict:
        """What a chain of K primitives starts from, a plain dict: the b seeds of `_seed_inputs` repeated to M rows each (row
        i * M + m continues seed i), the buffers the primitive loop works in over those b * M rows, and the [K,b,...] records of the
        returned primitives.  z: None (drawn here) or [K, b * M, 128]; reproj_factor, R0 [b,3,3], T0 [b,3]: None takes the defaults
        `generate_sequence` states.  No buffer aliases an input: the loop updates R0 / T0, the seed and the seed frames in place."""
        bm, dev, f32 = self.body_model, self.device, torch.float32
        if bm.M != 67:
            raise ValueError(f"the body model carries {bm.M} markers, the motion prior works on 67")
        b, rows, zd = X.shape[1], X.shape[1] * M, self.model.predictor.z_dim
        if z is None:
            z = torch.randn(K, rows, zd, device=dev)
        else:
            z = self._dev(z, "z").contiguous()
            if z.shape != (K, rows, zd):
                raise ValueError(f"z must be [{K},{rows},{zd}], got {tuple(z.shape)}")
        if reproj_factor is None:
            reproj_factor = _section(self.predictorcfg, "modelconfig").get("reproj_factor", 0.5)
        R0 = torch.eye(3, device=dev, dtype=f32).repeat(b, 1, 1) if R0 is None else self._dev(R0, "R0").reshape(b, 3, 3)
        T0 = torch.zeros(b, 3, device=dev, dtype=f32) if T0 is None else self._dev(T0, "T0").reshape(b, 3)
        rep = lambda t, dim=0: t.repeat_interleave(M, dim=dim).contiguous()
        new = lambda *shape: torch.empty(*shape, device=dev, dtype=f32)
        bt = rep(bt)
        s = {"rf": float(reproj_factor), "z": z, "bt": bt, "R0": rep(R0), "T0": rep(T0), "scene": None, "rows_scene": None,
             "xs": [rep(X, 1), new(2, rows, NM3)],                  # seed markers [2,rows,201], ping-pong (no output aliases an input)
             "seed": rep(seed.permute(1, 0, 2)),                    # [rows,2,93]
             "Y_gen": new(T_PRED, rows, NM3), "Yb_gen": new(T_PRED, rows, XB),
             "lbs_out": {"joints": new(rows * T_ALL, 127, 3), "markers": new(rows * T_ALL, bm.M, 3)},
             "markers": new(K, b, T_ALL, 67, 3), "params": new(K, b, T_ALL, XB), "rotmat": new(K, b, 3, 3), "transl": new(K, b, 3),
             "pelvis": new(K, b, T_ALL, 3), "nonfinite": torch.zeros(1, device=dev, dtype=torch.int32),
             # calc_calibrate_offset: joint 0 at zero orientation / translation (the body pose does not move the root)
             "delta_T": bm.joints55(torch.zeros(rows, XB, device=dev, dtype=f32), bt, 1)[:, 0].contiguous()}
        bm.workspace(rows * T_ALL)
        return s

    def _result(self, s, z, betas, R0, T0, to_numpy, search=None) -> PrimitiveSequence:
        res = [s["markers"], s["params"], s["rotmat"], s["transl"], s["pelvis"], z, betas, R0, T0]
        if to_numpy:
            res = [t.cpu().numpy() for t in res]
            search = search and {k: v.cpu().numpy() if torch.is_tensor(v) else v for k, v in search.items()}
        gender = str(_section(self.regressorcfg, "modelconfig").get("gender", "male"))
        return PrimitiveSequence(*res[:7], gender, res[7], res[8], search=search)

    def _primitive(self, s, k, dst, st, R0=None, T0=None):
        """What every primitive begins with, over all rows of the state: sample_prior_into -> egx_assemble_params into `dst`
        [rows,20,93] -> BodyModelHandle.forward into s["lbs_out"], with the penetration counts of the bodies in the frames R0 / T0
        where the state holds a scene.  Launches only."""
        cur, rows = s["xs"][k % 2], dst.shape[0]
        self.model.sample_prior_into(cur[0], cur[1], NM3, s["bt"], s["z"][k], s["Y_gen"], s["Yb_gen"])
        _lib.check(_lib.load().egx_assemble_params(_lib.ptr(s["seed"]), _lib.ptr(s["Yb_gen"]), rows, _lib.ptr(dst), st), "egx_assemble_params")
        in_scene = {} if s["scene"] is None else {"sdf": s["scene"], "R0": R0, "T0": T0, "agent_scene": s["rows_scene"]}
        self.body_model.forward(dst.view(rows * T_ALL, XB), s["bt"], T_ALL, want_verts=False, want_joints=True, want_markers=True,
                                out=s["lbs_out"], **in_scene)

    @staticmethod
    def _handoff_lead(s):
        """The nine arguments that follow pred_params in the three hand-off entries, built once per loop: only the seed frames
        read depend on k, and they alternate, so `[k % 2]` of the result is the tuple of primitive k."""
        lbs = s["lbs_out"]
        return [(_lib.ptr(s["Y_gen"]), _vp(x[0]), _vp(x[1]), NM3, _lib.ptr(lbs["joints"]), 127, _lib.ptr(lbs["markers"]), _lib.ptr(s["delta_T"]),
                 s["rf"]) for x in s["xs"]]

    @staticmethod
    def _select_lead(s, R0s, T0s):
        """The sixteen leading arguments of the two selection entries, likewise `[k % 2]`; R0s / T0s: the frames of the rows at
        even and at odd k."""
        lbs = s["lbs_out"]
        return [(_lib.ptr(s["Y_gen"]), _vp(x[0]), _vp(x[1]), NM3, _lib.ptr(lbs["joints"]), 127, _lib.ptr(lbs["markers"]), _lib.ptr(R0),
                 _lib.ptr(T0), _lib.ptr(lbs.get("pene_count")), _lib.ptr(s["goal"]), _lib.ptr(s["feet"]), s["weights"], s["pene_thres"],
                 s["goal_thresh"], s["rf"]) for x, R0, T0 in zip(s["xs"], R0s, T0s)]

    @staticmethod
    def _clearance_lead(s, K, b, M, R0s, T0s, st):
        """-> (entry name, per primitive its arguments) of the launch that goes before the selection and writes the table of frame
        clearances: egx_obstacle_marker_clearance with the marker model of the obstacles, egx_obstacle_ahead_clearance with the
        look-ahead of the cylinder model; (None, None) without a table.  R0s / T0s: the frames of the rows at even and at odd k."""
        if s.get("frame_clearance") is None:
            return None, None
        if s.get("obs_ahead") is not None:
            lead = [(_lib.ptr(s["lbs_out"]["joints"]), 127, _lib.ptr(R0), _lib.ptr(T0), b, M, *s["obstacles"]) for R0, T0 in zip(R0s, T0s)]
            return "egx_obstacle_ahead_clearance", [(*lead[k % 2], s["obs_frame0"] + T_PRED * k, *s["obs_ahead"], _lib.ptr(s["frame_clearance"]), st)
                                                    for k in range(K)]
        lead = [(_lib.ptr(s["lbs_out"]["markers"]), _lib.ptr(s["Y_gen"]), s["rf"], _lib.ptr(R0), _lib.ptr(T0), b, M, *s["obs_markers"])
                for R0, T0 in zip(R0s, T0s)]
        return "egx_obstacle_marker_clearance", [(*lead[k % 2], s["obs_frame0"] + T_PRED * k, s["obs_skin"], _lib.ptr(s["frame_clearance"]), st)
                                                 for k in range(K)]

    @staticmethod
    def _select_tail(s, K, base):
        """What follows the outputs of a selection entry, built once per loop -> (entry name, field arguments, per primitive the
        obstacle arguments): `base` and nothing; with a field `base`_field and the field; with obstacles `base`_obstacles, the field
        (a null one without) and, for primitive k, the obstacles with frame0 = obstacle_frame0 + 18 k and the outputs' row k; with the
        marker model of the obstacles, or the look-ahead of their cylinder model, `base`_obstacle_markers, the field, and the table, the
        two scalars and the outputs' row k."""
        if s["obstacles"] is None:
            return (base + "_field", s["field"], [()] * K) if s["field"] else (base, (), [()] * K)
        if s.get("frame_clearance") is not None:      # the marker model, the look-ahead: the phase reads the table the clearance launch wrote
            w_obs, margin, _ = s["obs_scalars"]
            obs = [(_lib.ptr(s["frame_clearance"]), w_obs, margin, _vp(s["obstacle_term"][k]), _vp(s["clearance"][k]),
                    _vp(s["obstacle_hit"][k])) for k in range(K)]
            return base + "_obstacle_markers", s["field"] or NULL_FIELD, obs
        obs = [(*s["obstacles"], s["obs_frame0"] + T_PRED * k, *s["obs_scalars"], _vp(s["obstacle_term"][k]), _vp(s["clearance"][k]),
                _vp(s["obstacle_hit"][k])) for k in range(K)]
        return base + "_obstacles", s["field"] or NULL_FIELD, obs

    # ------------------------------------------------------------------------------------------------------------------
    def generate_sequence(self, data, bparams, betas, n_primitives: int, n_gens: int = -1, z=None, reproj_factor=None,
                          to_numpy: bool = True, R0=None, T0=None) -> PrimitiveSequence:
        """A chain of `n_primitives` primitives from the motion seed (data [>=2,b,>=201], bparams [>=2,b,93] in the seed's
        canonical frame; betas as in `generate`; n_gens variants per seed).  Per primitive: sample_prior_into ->
        egx_assemble_params -> BodyModelHandle.forward (joints and markers) -> egx_primitive_advance, written into preallocated
        records; nothing in the loop waits for the device.
            - z: None (N(0, I) from the torch generator, drawn up front for all primitives) or [n_primitives, b', 128]
            - reproj_factor: None takes modelconfig['reproj_factor'] of the predictor config (0.5, the policy configs' value,
              where it has none)
            - R0 [b',3,3] / T0 [b',3]: the world frame of the seed; the identity when omitted
        Raises FloatingPointError when a primitive produced a non-finite value (read once, after the loop)."""
        if self.body_model is None:
            raise _lib.EgxError("generate_sequence needs the body model: build_model(..., body_model=BodyModelHandle)")
        K = int(n_primitives)
        if K < 1:
            raise ValueError("n_primitives must be >= 1")
        X, seed, bt = self._seed_inputs(data, bparams, betas, n_gens, None)
        s = self._chain_state(X, seed, bt, K, 1, z, reproj_factor, R0, T0)
        self._advance_loop(K, X.shape[1], s)
        n = int(s["nonfinite"].item())
        if n:
            raise FloatingPointError(f"{n} primitives of the chain produced non-finite values")
        return self._result(s, s["z"], bt, s["R0"], s["T0"], to_numpy)

    def _advance_loop(self, K, B, s):
        """The primitive loop of `generate_sequence`: launches only, no allocation that depends on k, no host wait."""
        lib, st, hand = _lib.load(), _lib.current_stream_ptr(), self._handoff_lead(s)
        for k in range(K):
            nxt, pp = s["xs"][(k + 1) % 2], s["params"][k]          # assembled straight into the record
            self._primitive(s, k, pp, st)
            _lib.check(lib.egx_primitive_advance(
                _vp(pp), *hand[k % 2], B, _lib.ptr(s["R0"]), _lib.ptr(s["T0"]), _vp(s["markers"][k]), _vp(s["pelvis"][k]),
                _vp(s["rotmat"][k]), _vp(s["transl"][k]), _lib.ptr(s["seed"]), _vp(nxt[0]), _vp(nxt[1]), NM3, _lib.ptr(s["nonfinite"]), st),
                "egx_primitive_advance")

    # ------------------------------------------------------------------------------------------------------------------
    def generate_sequence_to_goal(self, data, bparams, betas, goal, n_primitives: int, n_candidates: int, scene=None,
                                  agent_scene=None, weights: Optional[dict] = None, pene_thres: float = 40, goal_thresh=None,
                                  z=None, reproj_factor=None, to_numpy: bool = True, R0=None, T0=None,
                                  beam_width: int = 1, geodesic=None, obstacles=None, obstacle_weight: float = 1.0,
                                  obstacle_margin: float = 0.5, body_radius: float = 0.3,
                                  obstacle_frame0: int = 0, groups=None, pair_weight: float = 1.0, pair_margin: float = 0.5,
                                  joint_sweeps: int = 2, policy=None, pair_model: str = "cylinder",
                                  pair_skin: float = 0.05, route=None, obstacle_model: str = "cylinder",
                                  obstacle_skin: float = 0.05, lookahead: int = 0,
                                  lookahead_slack: float = 0.1) -> PrimitiveSequence:
        """`generate_sequence` steered to a goal through a scene by a greedy best-of-N search: for each of the `n_primitives`
        primitives, `n_candidates` candidates per sequence are generated, scored and the best one is kept; every candidate of the
        next primitive continues from it.  data / bparams / betas / reproj_factor / R0 / T0 as in `generate_sequence` (b seeds,
        one sequence each).
            - goal: [b,3] or [3], world coordinates; None (or the last waypoints) with `route=`
            - n_candidates: N in [1, 256] (ValueError above)
            - scene: None (no penetration term, nothing collides), an SdfScene, or an SdfSceneSet with agent_scene [b]
            - weights: {goal, skate, floor, pene, face} of cost = sum w * term, the terms being the arguments of the env's reward
              terms (distance to the goal in metres, -ln r_skate, -ln r_floor, -ln r_pene, 1 - r_face_target).  The defaults
              1, 1, 1, 1, 0 are a stated choice: nobody has measured motion quality with them (the instrument for it, for this
              and the stated choices below: egogen_amd/metrics.py, exp_GAMMAPrimitive/eval_motion.py).
            - pene_thres: a candidate one of whose 20 bodies has that many vertices inside the scene collides (40: the env's)
            - goal_thresh: None takes testconfig['goal_thresh'] (the policy configs' trainconfig.goal_thresh) where present, else 0.1
            - z: None (N(0, I) from the torch generator, drawn up front) or [n_primitives, b * N, 128]; row i * N + n is
              candidate n of sequence i
        Choice per sequence: candidates without a non-finite value first, then non-colliding, then the lower cost, then the lower
        index.  Per primitive: sample_prior_into -> egx_assemble_params -> BodyModelHandle.forward (with penetration counts in a
        scene) -> egx_primitive_select -> egx_primitive_advance_select; nothing in the loop waits for the device.
            - beam_width: W in [1, 32] with W * N <= 256 (ValueError otherwise).  1 is the greedy search above.  With W > 1 every
              sequence keeps W partial paths (slots); each slot is expanded into N candidates (row (i * W + s) * N + n is candidate n
              of slot s; z is [n_primitives, b * W * N, 128]; at the first primitive all slots hold the seed) and the W rows with the
              smallest path key (non-finite, colliding nodes on the path, accumulated cost, row) become the next slots, where the
              accumulated cost is the row's cost plus the skate, floor, pene and face terms of its ancestors: the goal distance at
              the path's end plus the motion quality along it.  Per primitive: ... -> egx_primitive_beam_select ->
              egx_primitive_advance_beam; after the loop egx_beam_backtrack gathers the path that ends in the best slot.
            - geodesic: None, or a `GeodesicField` (egogen_amd/geodesic.py) of 1 or b fields whose goals' xy equal `goal`'s
              (ValueError otherwise).  The goal term of the cost, greedy or beam, is then the field's distance along the walkable
              raster at the world xy of the candidate's last pelvis instead of the straight line, so the search goes round an
              obstacle instead of at it; goal_dist, the reached test and n_valid stay Euclidean.  The field is built before the
              loop (that build waits for the device); the loop stays launches only.
            - obstacles: None, or a `MovingObstacles` (egogen_amd/obstacles.py) of 1 or b sets (or with an index of b entries;
              ValueError otherwise) on the operator's device (one not yet on a device is moved there).  Other people as vertical
              cylinders on recorded tracks.  Over the 18 predicted frames of a candidate (frames 0 and 1 are the seed all
              candidates share) c_t is the distance in the plane from the candidate's pelvis to the nearest obstacle at that
              absolute frame, minus both radii; the cost, greedy or beam, gains obstacle_weight * mean_t max(0, obstacle_margin -
              c_t), accumulated along a beam's path like the other quality terms, and a candidate with min_t c_t < 0 (the
              cylinders overlap) counts as colliding: it is chosen only where every candidate collides, and status bit 0 says so.
              Primitive k is scored against the absolute frames obstacle_frame0 + 18 k + t; outside a track's frames an obstacle
              stands at its first or last position.  The loop stays launches only.
            - obstacle_weight (1.0), obstacle_margin (0.5 m), body_radius (0.3 m, the searching body's own cylinder): stated
              choices, like the weights above: nobody has measured motion quality with them.
            - obstacle_model: what a person of `obstacles` is.  "cylinder" (the default) is the model above: the same launches, the
              same buffers.  "markers": a recorded person is the 67 world markers of each of its frames (`MovingObstacles` built with
              markers: `from_sequences(..., markers=True)`, `from_rollout_files(..., markers=True)`, `from_tracks(..., markers=)`), a
              candidate is its own 67 blended markers in the world, in 3-D, as in pair_model "markers".  Per primitive one launch
              (egx_obstacle_marker_clearance, csrc/genop_obstacle_markers.hip) goes before the selection and writes c_t = the least
              of the 67 x 67 marker distances to the nearest recorded person at that absolute frame minus obstacle_skin for every
              row and predicted frame into a [b*M,18] table allocated once before the loop; the selection, greedy or beam
              (egx_primitive_select_obstacle_markers, egx_primitive_beam_select_obstacle_markers), reads it, and cost term, veto,
              order, the beam's accumulation and OBSTACLE_FIELDS are as above with that c_t: `clearance` is then the 3-D marker
              distance minus the skin.  body_radius is not read by this model.  It combines with scene, geodesic, route, policy and
              groups (either pair model) exactly as the cylinder model does; a policy that senses people still senses the tracks'
              cylinders.  ValueError for an unknown model, "markers" without obstacles or with obstacles that hold no markers, a
              negative or non-finite obstacle_skin.  Not built: marker boxes for `sense_people`, a skin per track, culling by
              bounding volumes, vertex-level penetration.  The loop stays launches only.
            - obstacle_skin (0.05 m): a recorded person's marker closer than this to one of the candidate's counts as contact.  The
              evaluator's `touch_dist` (egogen_amd/metrics.py) by intent, like pair_skin.  A stated choice.
            - groups: None, or [b] integer ids (or a `PersonGroups`, egogen_amd/crowd.py): sequences with equal ids are the people of
              one scene and time line, at most 32 of them, and see each other.  The greedy search only (ValueError with beam_width
              > 1).  Per primitive, after the selection (plain, with a field or with obstacles), one more launch
              (egx_primitive_select_joint) runs `joint_sweeps` Gauss-Seidel sweeps over the members of every group in order of
              their sequence index: member i scores each of its N candidates against the others' CURRENTLY chosen tracks with the
              obstacle term's arithmetic - c_t the distance in the plane between the two pelvises at predicted frame t minus 2 *
              body_radius, the cost gains pair_weight * mean_t max(0, pair_margin - c_t), a candidate with min_t c_t < 0 is in
              the colliding class - takes the best by the selection's order, and the next member sees that choice.  The hand-off
              continues from the joint choice; `crowd_clearance` / `crowd_hit` say whether the chosen tracks of a primitive
              overlap.  The model and its limits: a person is a cylinder of body_radius round the pelvis; the horizon is one
              primitive and the others' tracks are their current choices, not predictions; everybody starts from the own best and
              two sweeps need not reach a fixed point (`joint_changed` of the last sweep says whether one did); a member that has
              reached its goal keeps walking, and stays an obstacle, after the primitive at which its file stops.  A group of
              one is the search without groups.  The loop stays launches only.
            - pair_weight (1.0), pair_margin (0.5 m), joint_sweeps (2, in [1, 8]): stated choices like the others, informed by a
              toy on the CPU only: nobody has measured motion quality with them.
            - pair_model: what a person is to the joint step.  "cylinder" (the default) is the model above.  "markers": a person
              is the 67 blended markers of a candidate - the body model's markers and the prior's predicted markers blended by
              reproj_factor, exactly what the hand-off records - in the world, in 3-D.  Two launches stand where
              egx_primitive_select_joint stands: egx_pair_marker_dist writes, for every pair of members of a group and every pair
              of their candidates, the least of the 67 x 67 marker distances at each predicted frame into a table allocated once
              before the loop (pairs x N^2 x 72 bytes; ValueError above 1 GiB, crowd.PAIR_TABLE_CAP_BYTES), and
              egx_primitive_select_joint_markers runs the same sweeps with c_t = that distance to the nearest other member's
              current choice minus pair_skin; cost term, veto, order, traces and `crowd_clearance` / `crowd_hit` are as above with
              that c_t.  body_radius is not read by this model (it still is by `obstacles=`, whose recorded tracks stay
              cylinders).  Needs groups (ValueError without).  The limits that remain: 67 markers sample the surface sparsely, the
              horizon is one primitive, the others' tracks are their current choices.
            - pair_skin (0.05 m): markers of two people closer than this count as contact.  The evaluator's `touch_dist`
              (egogen_amd/metrics.py) by intent: a hit in the search is a touch frame in `crowd_metrics`.  A stated choice.
            - policy: None, or a `PolicyProposal` (egogen_amd/proposal.py): the trained policy as the proposal distribution.  The
              greedy search only (ValueError with beam_width > 1).  `z` (supplied or drawn up front) becomes the eps of the
              proposal.  Before the loop one body-model forward of the b x 2 seed bodies gives the first observation its joints;
              per primitive, ahead of the prefix above: egx_primitive_observe (the observation the env would hand the policy after
              the chosen primitive, from the hand-off's records) -> the policy's actor into the records -> egx_policy_propose,
              which rewrites the rows of z[k]: the first n_mean of a sequence become mu, the rows up to n_policy mu + temperature
              * sigma * eps, the rest stay eps, the prior's samples.  scene, geodesic, obstacles and groups act after the proposal
              and work as without it.  The returned z is the chosen row of the rewritten candidates.  The loop stays launches
              only.  The proposal's parameters are stated choices (see `PolicyProposal`): nobody has measured motion quality with
              them.  A proposal built with `sense_people=True` makes the group-mates of `groups` and the tracks of `obstacles` holes
              of the polygon its rays are cast against (egx_primitive_people_boxes -> egx_primitive_observe_people in place of
              egx_primitive_observe, the obstacles at the absolute frames obstacle_frame0 + 18 k and + 1 of the two seed frames);
              without it the policy senses the static polygon only.
            - route: None, or a `Routes` (egogen_amd/route.py) of b routes: every sequence walks an itinerary of 1 to 16 waypoints,
              the last of which is its goal (`goal` must then be None or `route.last()`; ValueError otherwise).  Every kernel of the
              loop reads the goal from one [b,3] device buffer; that buffer starts at the first waypoints, and one more launch per
              primitive after the hand-off (egx_route_advance, csrc/genop_route.hip) moves a per-sequence cursor and rewrites it -
              and, with `geodesic=`, the [b] index that picks each sequence's field.  The rule, over the 18 predicted frames of the
              chosen primitive in order: a waypoint that is not the last is passed at the first frame whose pelvis is within
              `route.pass_radius` of it horizontally; the next one may be passed from that same frame on.  The greedy search only
              (ValueError with beam_width > 1): the slots of a beam would need a cursor and a goal each.  pass_radius must not be
              below goal_thresh (ValueError): a point the selection calls reached must also count as passed.  With `geodesic=` the
              field must hold one field per entry of `route.field_goals()`, in that order (ValueError otherwise).  scene, obstacles,
              groups (both pair models) and policy work as they are: they read the goal through the same pointer, so a policy's
              observation aims at the current waypoint.  The result's `goal` is `route.last()`, and `ROUTE_FIELDS` hold the trace.
              The loop stays launches only.  The limits: the goal term is the distance to the current waypoint only - a candidate
              that passes it mid-primitive gets no credit for the leg beyond; arrival at the last waypoint can be recognised one
              primitive late when the cursor reaches it during that same primitive (`reached` of a primitive scored against an
              intermediate point is cleared); after the last waypoint the person still keeps walking.
            - lookahead: H in [0, 8], the further primitives the cylinder models of `obstacles` and `groups` look ahead.  0 (the
              default) is the search as described above: the same launches, the same buffers, the same bits.  With H > 0 a candidate
              is predicted to repeat its own net displacement d = p(19) - p(1) (frames 18 and 19 become the next seed, so frame t of
              the next primitive corresponds to t + 18 of this one): p_h(t) = p(t) + h d, and the frame clearance both terms score is
              c_t = min(c_{t,0}, min_{h=1..H} max(0, c_{t,h}) + h * lookahead_slack), c_{t,0} the clearance described above and c_{t,h}
              the same at the predicted positions.  A prediction can cost but only the present can veto: a predicted overlap never
              puts a candidate into the colliding class by itself; the slack makes far predictions count less.  A non-finite own
              pelvis at frame 1, t or 19 that makes a prediction NaN makes the row non-finite, as a NaN pelvis does today.  With
              `obstacles` (greedy or beam) only the candidate is predicted - the recorded person's future is on record and is read
              at the absolute frames obstacle_frame0 + 18 (k + h) + t: one launch per primitive (egx_obstacle_ahead_clearance) goes
              before the selection and writes c_t into a [b*M,18] table allocated once before the loop, which the selection reads
              through the entries that take a table (egx_primitive_select_obstacle_markers /
              egx_primitive_beam_select_obstacle_markers).  With `groups` both people are predicted, the others by the displacement of
              their CURRENT choice: egx_primitive_select_joint_ahead stands where egx_primitive_select_joint stands; pair_clearance /
              pair_term / pair_hit are then those of the look-ahead c_t, crowd_clearance / crowd_hit stay at h = 0.  It combines
              with scene, geodesic, route, policy (with and without sense_people) and beam_width > 1 exactly as the cylinder models
              do.  ValueError for an H that is not an integer in [0, 8], a negative or non-finite slack, H > 0 with neither obstacles
              nor groups, H > 0 with obstacle_model="markers" or pair_model="markers".  The limits: repeating one primitive's
              displacement at constant velocity is a guess, not a plan; predictions use pelvis cylinders only; a member that has
              reached its goal is still predicted to walk on.  Not built: look-ahead for the marker models, velocity obstacles,
              predictions from anything but the own primitive.  The loop stays launches only.
            - lookahead_slack (0.1 m per primitive of look-ahead; with the default margins of 0.5 m a prediction five primitives
              ahead has no cost left) and the default lookahead of 0: stated choices like the others: nobody has measured motion
              quality with them.
        Raises FloatingPointError when a chosen hand-off, or every candidate of a sequence, held a non-finite value (read once,
        after the loop); for a beam, when a node of the returned path did."""
        from .body_model import SdfScene, SdfSceneSet
        from . import synth
        if self.body_model is None:
            raise _lib.EgxError("generate_sequence_to_goal needs the body model: build_model(..., body_model=BodyModelHandle)")
        K, N, W = int(n_primitives), int(n_candidates), int(beam_width)
        if K < 1:
            raise ValueError("n_primitives must be >= 1")
        if N < 1 or N > MAX_CANDIDATES:
            raise ValueError(f"n_candidates must be in [1, {MAX_CANDIDATES}], got {N}")
        if W < 1 or W > MAX_BEAM:
            raise ValueError(f"beam_width must be in [1, {MAX_BEAM}], got {W}")
        if W * N > MAX_CANDIDATES:
            raise ValueError(f"beam_width * n_candidates must be at most {MAX_CANDIDATES}, got {W} * {N}")
        M = W * N       # rows per sequence
        if policy is not None:
            from .proposal import PolicyProposal, check_beam
            if not isinstance(policy, PolicyProposal):
                raise TypeError(f"policy must be None or a PolicyProposal, got {type(policy).__name__}")
            check_beam(W)
            policy.counts(N)
        if obstacle_model not in OBSTACLE_MODELS:
            raise ValueError(f"obstacle_model must be one of {OBSTACLE_MODELS}, got {obstacle_model!r}")
        if not (float(obstacle_skin) >= 0 and np.isfinite(float(obstacle_skin))):
            raise ValueError(f"obstacle_skin must be finite and not negative, got {obstacle_skin}")
        if obstacle_model == "markers" and (obstacles is None or getattr(obstacles, "markers", None) is None):
            raise ValueError('obstacle_model="markers" needs obstacles= that carry markers (MovingObstacles.from_sequences / '
                             'from_rollout_files with markers=True, or from_tracks(..., markers=))')
        people = _person_groups(groups, data, W, pair_weight, pair_margin, body_radius, joint_sweeps, pair_model, pair_skin, N)
        H, slack = _checked_lookahead(lookahead, lookahead_slack, obstacles, groups, obstacle_model, pair_model)
        if goal_thresh is None:
            goal_thresh = self.testconfig.get("goal_thresh", 0.1)
        route = _checked_route(route, data, goal, W, goal_thresh)
        X, seed, bt = self._seed_inputs(data, bparams, betas, -1, None)
        b, dev, f32, i32 = X.shape[1], self.device, torch.float32, torch.int32
        goal = self._dev(goal if route is None else route.last(), "goal")
        if goal.shape == (3,):
            goal = goal.reshape(1, 3).repeat(b, 1)
        if goal.shape != (b, 3):
            raise ValueError(f"goal must be [3] or [{b},3], got {tuple(goal.shape)}")
        goal = goal.contiguous()
        field_args = field_alive = None
        if geodesic is not None:
            from .geodesic import GeodesicField
            if not isinstance(geodesic, GeodesicField):
                raise TypeError(f"geodesic must be None or a GeodesicField, got {type(geodesic).__name__}")
            if route is None and len(geodesic) not in (1, b):
                raise ValueError(f"geodesic must hold 1 or {b} fields, got {len(geodesic)}")
            if geodesic.dist.device != dev:
                raise ValueError(f"geodesic lives on {geodesic.dist.device}, the operator on {dev}")
            if route is None:
                if not torch.equal(geodesic.goals[:, :2].to(dev).expand(b, 2), goal[:, :2]):
                    raise ValueError("the fields of `geodesic` were built for other goals than `goal` (their xy must be equal)")
                field_args, field_alive = geodesic.select_args(b)
            else:       # one field per distinct waypoint; the index of every sequence is a buffer the route launch rewrites
                want = torch.from_numpy(route.field_goals()[:, :2])
                if len(geodesic) != len(want) or not torch.equal(geodesic.goals[:, :2].cpu(), want):
                    raise ValueError("the fields of `geodesic` must be those of route.field_goals(), in that order (their xy must be equal)")
                field_alive = torch.from_numpy(route.field_of[:, 0].copy()).to(dev).contiguous()
                field_args = (*geodesic.select_args(b)[0][:6], _lib.ptr(field_alive))
        obs_args = obs_alive = None
        if obstacles is not None:
            from .obstacles import MovingObstacles
            if not isinstance(obstacles, MovingObstacles):
                raise TypeError(f"obstacles must be None or a MovingObstacles, got {type(obstacles).__name__}")
            if obstacles.index is None and len(obstacles) not in (1, b):
                raise ValueError(f"obstacles must hold 1 or {b} sets, got {len(obstacles)}")
            if obstacles.device is None:
                obstacles.to(dev)
            if obstacles.device != dev:
                raise ValueError(f"obstacles live on {obstacles.device}, the operator on {dev}")
            if not (float(obstacle_margin) >= 0 and float(body_radius) >= 0 and np.isfinite(float(obstacle_weight))):
                raise ValueError(f"obstacle_margin and body_radius must not be negative and obstacle_weight finite, got "
                                 f"{obstacle_margin}, {body_radius}, {obstacle_weight}")
            obs_args, obs_alive = obstacles.select_args(b)
            if obstacle_model == "markers":
                obs_marker_args, obs_marker_alive = obstacles.marker_args(b)
        rows_scene = None
        if isinstance(scene, SdfSceneSet):
            if agent_scene is None:
                raise ValueError("a scene set needs agent_scene [b]")
            idx = torch.as_tensor(agent_scene).reshape(-1).to("cpu", torch.int64)
            if idx.numel() != b or int(idx.min()) < 0 or int(idx.max()) >= len(scene):
                raise ValueError(f"agent_scene must hold {b} indices in [0, {len(scene)}), got {idx.tolist()}")
            rows_scene = idx.to(dev, i32).repeat_interleave(M).contiguous()
        elif agent_scene is not None:
            raise ValueError("agent_scene needs an SdfSceneSet")
        elif scene is not None and not isinstance(scene, SdfScene):
            raise TypeError(f"scene must be None, an SdfScene or an SdfSceneSet, got {type(scene).__name__}")
        w = dict(SEARCH_WEIGHTS)
        if weights:
            unknown = set(weights) - set(w)
            if unknown:
                raise ValueError(f"unknown weights {sorted(unknown)}: the terms are {list(w)}")
            w.update({k: float(v) for k, v in weights.items()})
        s = self._chain_state(X, seed, bt, K, M, z, reproj_factor, R0, T0)
        rec = lambda *tail, dtype=f32: torch.empty(K, b, *tail, device=dev, dtype=dtype)
        s.update({"goal": goal, "scene": scene, "rows_scene": rows_scene, "pp": torch.empty(b * M, T_ALL, XB, device=dev, dtype=f32),
                  "feet": torch.tensor(synth.feet_marker_idx(), device=dev, dtype=i32),
                  "weights": (C.c_float * 5)(*[w[k] for k in ("goal", "skate", "floor", "pene", "face")]),
                  "pene_thres": float(pene_thres), "goal_thresh": float(goal_thresh), "field": field_args, "field_alive": field_alive,
                  "choice": rec(dtype=i32), "status": rec(dtype=i32), "reached": rec(dtype=i32), "goal_dist": rec(),
                  "cost": rec(M), "cost_terms": rec(M, 5), "colliding": rec(M, dtype=i32), "obstacles": obs_args, "obs_alive": obs_alive})
        if obs_args is not None:
            s.update({"obs_scalars": (float(obstacle_weight), float(obstacle_margin), float(body_radius)), "obs_frame0": int(obstacle_frame0),
                      "obstacle_term": rec(M), "clearance": rec(M), "obstacle_hit": rec(M, dtype=i32)})
            if obstacle_model == "markers":      # the table of frame clearances, allocated once: the loop stays launches only
                s.update({"obs_markers": obs_marker_args, "obs_markers_alive": obs_marker_alive, "obs_skin": float(obstacle_skin),
                          "frame_clearance": torch.empty(b * M, T_PRED, device=dev, dtype=f32)})
            elif H > 0:      # the look-ahead's table of frame clearances, likewise allocated once
                s.update({"obs_ahead": (float(body_radius), H, slack), "frame_clearance": torch.empty(b * M, T_PRED, device=dev, dtype=f32)})
        if people is not None:
            S, G = int(joint_sweeps), len(people.to(dev))
            trace = lambda *tail, dtype=f32: torch.empty(K, S, *tail, device=dev, dtype=dtype)
            reach = float(pair_skin if pair_model == "markers" else body_radius)      # what the model's people keep clear of each other
            s.update({"joint": (_lib.ptr(people.group_start), _lib.ptr(people.group_member), G, S, float(pair_weight), float(pair_margin),
                                reach, float(goal_thresh)), "joint_alive": people,
                      "individual_choice": rec(dtype=i32), "pair_term": trace(b, N), "pair_clearance": trace(b, N),
                      "joint_cost": trace(b, N), "pair_hit": trace(b, N, dtype=i32), "choice_trace": trace(b, dtype=i32),
                      "joint_changed": trace(G, dtype=i32), "crowd_clearance": rec(), "crowd_hit": rec(dtype=i32),
                      "groups": torch.as_tensor(people.ids), "pair_model": pair_model, "pair_skin": float(pair_skin)})
            if H > 0:        # the look-ahead entry takes H and the slack after body_radius
                s["joint"] = (*s["joint"][:7], H, slack, s["joint"][7])
                s["joint_ahead"] = True
            if pair_model == "markers":      # the distance table and the bad-frame masks, allocated once: the loop stays launches only
                npairs = int(people.pair_offsets[-1])
                s.update({"pair_dist": torch.empty(npairs, N, N, T_PRED, device=dev, dtype=f32) if npairs else None,
                          "row_bad": torch.zeros(b * N, device=dev, dtype=i32), "npairs": npairs})
        if scene is not None:
            s["lbs_out"]["pene_count"] = torch.empty(b * M * T_ALL, device=dev, dtype=i32)
        s["route"] = None
        if route is not None:       # the live goal is a buffer of its own: search["goal"] stays the last waypoints
            rd, P = route.to(dev), route.waypoints.shape[1]
            s.update({"goal": rd["waypoints"][:, 0].clone().contiguous(), "route_alive": rd, "route_state": torch.zeros(b, device=dev, dtype=i32),
                      "route_cursor": rec(dtype=i32), "route_goal": rec(3), "route_pass_dist": rec(),
                      "route": (_lib.ptr(rd["waypoints"]), _lib.ptr(rd["count"]), _lib.ptr(rd["field_of"]), b, P, float(route.pass_radius))})
        s["policy"] = policy
        if policy is not None:
            if z is not None:
                s["z"] = s["z"].clone()         # the proposal overwrites its eps in place: never the caller's tensor
            policy.prepare(self, s, K, b, N)
        status = s["status"]
        if W == 1:
            self._search_loop(K, b, N, s)
            n = int(s["nonfinite"].item())
            n_all = int((status & 2).ne(0).sum().item())
            if n or n_all:
                raise FloatingPointError(f"the search produced non-finite values: {n} chosen hand-offs, {n_all} sequence steps whose "
                                         f"candidates were all non-finite")
            R0_end, T0_end = s["R0"], s["T0"]
        else:
            s.update({"R0s": [s["R0"], torch.empty_like(s["R0"])], "T0s": [s["T0"], torch.empty_like(s["T0"])],      # ping-pong
                      "acc": torch.zeros(K + 1, b, W, device=dev, dtype=f32), "ncoll": torch.zeros(K + 1, b, W, device=dev, dtype=i32),
                      "rec_markers": rec(W, T_ALL, 67, 3), "rec_params": rec(W, T_ALL, XB), "rec_rotmat": rec(W, 3, 3),
                      "rec_transl": rec(W, 3), "rec_pelvis": rec(W, T_ALL, 3), "beam_row": rec(W, dtype=i32), "parent": rec(W, dtype=i32),
                      "path_cost": rec(W), "beam_status": rec(W, dtype=i32), "slot_goal_dist": rec(W), "slot_reached": rec(W, dtype=i32),
                      "path_slot": rec(dtype=i32)})
            self._beam_loop(K, b, W, N, s)
            n = int((status & 6).ne(0).sum().item())
            if n:
                raise FloatingPointError(f"the beam search produced non-finite values: {n} nodes of the returned paths")
            R0_end, T0_end = s["R0s"][K % 2], s["T0s"][K % 2]      # the rows of slot 0: where the path ends
        reached, zd = s["reached"].ne(0), s["z"].shape[-1]
        first = torch.where(reached.any(0), reached.int().argmax(0) + 1, torch.full((b,), K, device=dev, dtype=torch.int64))
        zc = s["z"].view(K, b, M, zd).gather(2, s["choice"].long().view(K, b, 1, 1).expand(K, b, 1, zd))[:, :, 0]
        search = {"goal": goal, "choice": s["choice"], "cost": s["cost"], "cost_terms": s["cost_terms"], "colliding": s["colliding"],
                  "status": status, "goal_dist": s["goal_dist"], "n_valid": first, "geo_dist": None}
        if geodesic is not None:
            search["geo_dist"] = s["cost_terms"][..., 0].gather(2, s["choice"].long().clamp(0, M - 1).unsqueeze(-1))[..., 0]
        if W > 1:
            search.update({k: s[k] for k in ("path_slot", "parent", "beam_row", "path_cost", "beam_status")}, beam_width=W)
        if obs_args is not None:
            search.update({k: s[k] for k in PrimitiveSequence.OBSTACLE_FIELDS}, obstacle_model=obstacle_model, obstacle_skin=float(obstacle_skin))
        if people is not None:
            search.update({k: s[k] for k in PrimitiveSequence.JOINT_FIELDS + ("pair_model", "pair_skin")})
        if obs_args is not None or people is not None:
            search.update(lookahead=H, lookahead_slack=slack)
        if policy is not None:
            search.update(policy.record(s))
        if route is not None:
            search.update({"route_waypoints": s["route_alive"]["waypoints"], "route_count": s["route_alive"]["count"],
                           "route_cursor": s["route_cursor"], "route_goal": s["route_goal"], "route_pass_dist": s["route_pass_dist"],
                           "pass_radius": float(route.pass_radius)})
        return self._result(s, zc, bt, R0_end[::M].reshape(b, 3, 3).contiguous(), T0_end[::M].contiguous(), to_numpy, search)

    @staticmethod
    def _joint_lead(s, b, N, st):
        """-> (the joint entry of the state's pair model, what it takes before the selection's rows, the arguments of the distance
        launch that goes before it or None)"""
        rows = (_lib.ptr(s["lbs_out"]["joints"]), 127, _lib.ptr(s["R0"]), _lib.ptr(s["T0"]), _lib.ptr(s["goal"]))
        if s.get("row_bad") is None:       # the cylinders; with a look-ahead their entry that predicts (s["joint"] then carries H and the slack)
            return "egx_primitive_select_joint_ahead" if s.get("joint_ahead") else "egx_primitive_select_joint", rows, None
        crowd, npairs = s["joint_alive"], s["npairs"]         # the marker model: the table's launch, then the sweeps on it
        table, bad, pair_start = _lib.ptr(s["pair_dist"]), _lib.ptr(s["row_bad"]), _lib.ptr(crowd.pair_start)
        dist_args = (_lib.ptr(s["lbs_out"]["markers"]), _lib.ptr(s["Y_gen"]), s["rf"], _lib.ptr(s["R0"]), _lib.ptr(s["T0"]), b, N,
                     _lib.ptr(crowd.group_start), _lib.ptr(crowd.group_member), pair_start, len(crowd), npairs, table, bad, st)
        return "egx_primitive_select_joint_markers", (table, bad, pair_start, npairs, *rows), dist_args

    def _search_loop(self, K, b, N, s):
        """The primitive loop of `generate_sequence_to_goal`: launches only, no allocation that depends on k, no host wait.  With
        groups (s["joint"]) the joint launch stands between the selection and the hand-off - with the marker model (s["row_bad"])
        the two launches of csrc/genop_joint_markers.hip in its place; a device copy keeps what the selection chose.  With a route
        (s["route"]) one launch after the hand-off moves the cursors and rewrites the goal buffer the next primitive reads."""
        lib, st, hand, pp = _lib.load(), _lib.current_stream_ptr(), self._handoff_lead(s), _lib.ptr(s["pp"])
        sel = self._select_lead(s, [s["R0"]] * 2, [s["T0"]] * 2)
        name, field, obs = self._select_tail(s, K, "egx_primitive_select")
        select = getattr(lib, name)
        clear_name, clear = self._clearance_lead(s, K, b, N, [s["R0"]] * 2, [s["T0"]] * 2, st)
        clear_entry = clear_name and getattr(lib, clear_name)
        joint, policy, route = s.get("joint"), s.get("policy"), s.get("route")
        if route is not None:
            route_out = (_lib.ptr(s["route_state"]), _lib.ptr(s["goal"]), _lib.ptr(s["field_alive"]) if s["field"] else None)
        if joint is not None:
            joint_name, joint_in, dist_args = self._joint_lead(s, b, N, st)
            joint_entry = getattr(lib, joint_name)
        sensed = [()] * K
        if policy is not None and policy.sense_people:      # what the policy senses of the others: the groups' CSR and the obstacles
            from .proposal import NO_GROUPS, NO_OBSTACLES
            crowd = s.get("joint_alive")
            grp = NO_GROUPS if crowd is None else (_lib.ptr(crowd.group_start), _lib.ptr(crowd.group_member), _lib.ptr(crowd.member_group),
                                                   len(crowd))
            sensed = [(grp, NO_OBSTACLES if s["obstacles"] is None else (*s["obstacles"], s["obs_frame0"] + T_PRED * k)) for k in range(K)]
        for k in range(K):
            nxt = s["xs"][(k + 1) % 2]
            if policy is not None:
                policy.launch(s, k, b, N, st, *sensed[k])
            self._primitive(s, k, s["pp"], st, s["R0"], s["T0"])
            if clear is not None:
                _lib.check(clear_entry(*clear[k]), clear_name)
            _lib.check(select(
                *sel[k % 2], b, N, _vp(s["choice"][k]), _vp(s["status"][k]), _vp(s["reached"][k]),
                _vp(s["goal_dist"][k]), _vp(s["cost"][k]), _vp(s["cost_terms"][k]), _vp(s["colliding"][k]), *field, *obs[k], st), name)
            if joint is not None:
                s["individual_choice"][k].copy_(s["choice"][k])
                if dist_args is not None:
                    _lib.check(lib.egx_pair_marker_dist(*dist_args), "egx_pair_marker_dist")
                _lib.check(joint_entry(
                    *joint_in, _vp(s["cost"][k]), _vp(s["cost_terms"][k]), _vp(s["colliding"][k]), b, N, *joint,
                    _vp(s["choice"][k]), _vp(s["status"][k]), _vp(s["reached"][k]), _vp(s["goal_dist"][k]), _vp(s["pair_term"][k]),
                    _vp(s["pair_clearance"][k]), _vp(s["joint_cost"][k]), _vp(s["pair_hit"][k]), _vp(s["choice_trace"][k]),
                    _vp(s["joint_changed"][k]), _vp(s["crowd_clearance"][k]), _vp(s["crowd_hit"][k]), st), joint_name)
            _lib.check(lib.egx_primitive_advance_select(
                pp, *hand[k % 2], b, _vp(s["choice"][k]), N, _lib.ptr(s["R0"]), _lib.ptr(s["T0"]), _vp(s["markers"][k]),
                _vp(s["pelvis"][k]), _vp(s["rotmat"][k]), _vp(s["transl"][k]), _vp(s["params"][k]), _lib.ptr(s["seed"]), _vp(nxt[0]),
                _vp(nxt[1]), NM3, _lib.ptr(s["nonfinite"]), st), "egx_primitive_advance_select")
            if route is not None:
                _lib.check(lib.egx_route_advance(
                    _vp(s["pelvis"][k]), _vp(s["rotmat"][k]), _vp(s["transl"][k]), *route, *route_out, _vp(s["reached"][k]),
                    _vp(s["route_cursor"][k]), _vp(s["route_goal"][k]), _vp(s["route_pass_dist"][k]), st), "egx_route_advance")

    def _beam_loop(self, K, b, W, N, s):
        """The primitive loop of the beam search and the backtrack after it: launches only, no allocation that depends on k, no
        host wait.  R0 / T0 and the seed frames are read from one buffer and written to the other: a slot may continue from a row
        of another slot of its sequence."""
        lib, st, hand, pp = _lib.load(), _lib.current_stream_ptr(), self._handoff_lead(s), _lib.ptr(s["pp"])
        sel = self._select_lead(s, s["R0s"], s["T0s"])
        name, field, obs = self._select_tail(s, K, "egx_primitive_beam_select")
        select = getattr(lib, name)
        clear_name, clear = self._clearance_lead(s, K, b, W * N, s["R0s"], s["T0s"], st)
        clear_entry = clear_name and getattr(lib, clear_name)
        for k in range(K):
            nxt = s["xs"][(k + 1) % 2]
            R0, T0, R0n, T0n = s["R0s"][k % 2], s["T0s"][k % 2], s["R0s"][(k + 1) % 2], s["T0s"][(k + 1) % 2]
            self._primitive(s, k, s["pp"], st, R0, T0)
            if clear is not None:
                _lib.check(clear_entry(*clear[k]), clear_name)
            _lib.check(select(
                *sel[k % 2], b, W, N, _vp(s["acc"][k]), _vp(s["ncoll"][k]), _vp(s["cost"][k]), _vp(s["cost_terms"][k]),
                _vp(s["colliding"][k]), _vp(s["beam_row"][k]), _vp(s["parent"][k]), _vp(s["acc"][k + 1]), _vp(s["ncoll"][k + 1]),
                _vp(s["path_cost"][k]), _vp(s["beam_status"][k]), _vp(s["slot_goal_dist"][k]), _vp(s["slot_reached"][k]), *field, *obs[k], st),
                name)
            _lib.check(lib.egx_primitive_advance_beam(
                pp, *hand[k % 2], b, W, N, _vp(s["beam_row"][k]), _lib.ptr(R0), _lib.ptr(T0), _lib.ptr(R0n), _lib.ptr(T0n),
                _vp(s["rec_markers"][k]), _vp(s["rec_pelvis"][k]), _vp(s["rec_rotmat"][k]), _vp(s["rec_transl"][k]), _vp(s["rec_params"][k]),
                _lib.ptr(s["seed"]), _vp(nxt[0]), _vp(nxt[1]), NM3, _vp(s["beam_status"][k]), st), "egx_primitive_advance_beam")
        _lib.check(lib.egx_beam_backtrack(
            _lib.ptr(s["parent"]), _lib.ptr(s["beam_row"]), _lib.ptr(s["beam_status"]), _lib.ptr(s["slot_goal_dist"]),
            _lib.ptr(s["slot_reached"]), _lib.ptr(s["rec_markers"]), _lib.ptr(s["rec_pelvis"]), _lib.ptr(s["rec_rotmat"]),
            _lib.ptr(s["rec_transl"]), _lib.ptr(s["rec_params"]), K, b, W, _lib.ptr(s["path_slot"]), _lib.ptr(s["choice"]),
            _lib.ptr(s["status"]), _lib.ptr(s["goal_dist"]), _lib.ptr(s["reached"]), _lib.ptr(s["markers"]), _lib.ptr(s["pelvis"]),
            _lib.ptr(s["rotmat"]), _lib.ptr(s["transl"]), _lib.ptr(s["params"]), st), "egx_beam_backtrack")

    # ------------------------------------------------------------------------------------------------------------------
    def _compose_body_params_(self, data):
        transl, glorot = data["transl"], data["glorot"]
        body_pose = data["poses"][:, :63]
        hand_pose = np.zeros((transl.shape[0], 24))
        return np.concatenate([transl, glorot, body_pose, hand_pose], axis=-1)      # [t,d]

    def generate_primitive_to_files(self, batch_gen, n_seqs, n_gens, t_his=None):
        """:1363-1424.  n_seqs: how many sequences to generate; n_gens: for each input sequence, how many different sequences
        to predict.  `batch_gen`: anything with `next_sequence()` and `amass_subset_name`; sequences of another gender than the
        regressor's are skipped.  Writes <result_dir>/mp_gen_seed<seed>/<subset>/results_<body_repr>_<gender>.pkl and returns
        its path."""
        keys = ("gt", "betas", "gender", "transf_rotmat", "transf_transl", "markers", "smplx_params", "transl")
        gen_results: dict = {k: [] for k in keys}
        gender = _section(self.regressorcfg, "modelconfig")["gender"]
        idx = 0
        while idx < n_seqs:
            print("[INFO] generating with motion seed {}".format(idx))
            data = batch_gen.next_sequence()
            if str(data["gender"]) != gender:
                continue
            motion_np = np.asarray(data["body_feature"])
            motion = torch.as_tensor(motion_np, dtype=torch.float32).unsqueeze(1)                  # [t,b,d]
            bparams = torch.as_tensor(self._compose_body_params_(data), dtype=torch.float32).unsqueeze(1)
            gen_results["gt"].append(motion_np[:, :NM3].reshape((1, motion_np.shape[0], -1, 3)))
            gen_results["betas"].append(data["betas"])
            gen_results["gender"].append(str(data["gender"]))
            gen_results["transf_rotmat"].append(data["transf_rotmat"])
            gen_results["transf_transl"].append(data["transf_transl"])
            gen_results["transl"].append(data["transl"][None, ...])                              # [b,t,d]
            pred_markers, pred_body_params = self.generate(motion, bparams, betas=np.asarray(data["betas"]), n_gens=n_gens, t_his=t_his)
            gen_results["markers"].append(np.reshape(pred_markers, (pred_markers.shape[0], pred_markers.shape[1], -1, 3)))
            gen_results["smplx_params"].append(pred_body_params)
            idx += 1
        for k in ("gt", "markers", "smplx_params", "transl"):
            gen_results[k] = np.stack(gen_results[k])        # markers: [#seq, #genseq_per_pastmotion, t, #markers, 3]
        outdir = os.path.join(self.testconfig["result_dir"], "mp_gen_seed{}".format(self.testconfig["seed"]),
                              batch_gen.amass_subset_name[0])
        os.makedirs(outdir, exist_ok=True)
        outfilename = os.path.join(outdir, "results_{}_{}.pkl".format(_section(self.predictorcfg, "modelconfig")["body_repr"], gender))
        print(outfilename)
        with open(outfilename, "wb") as f:
            pickle.dump(gen_results, f)
        return outfilename
