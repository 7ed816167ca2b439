#!/usr/bin/env python3
"""Turn a motion seed into N seconds of motion in K variants with a trained motion prior, without an environment:
`GAMMAPrimitiveComboGenOP.generate_sequence` (egogen_amd/genop.py) chained over `--n-primitives` primitives (0.45 s each at
40 fps) for `--n-gens` variants of one seed, one `motion_<seed>_<variant>.pkl` per variant in the layout
`utils.rollout_primitives` and the EgoBody consumers read.

With `--goal x,y,z` (world coordinates) the variants are steered there by `generate_sequence_to_goal`: `--n-candidates N` candidates
per primitive and variant, the best one kept (greedy best-of-N on the env's reward arguments), optionally through the SDF scene
`--scene file.npz` (keys sdf, center, scale: the reference's sdf_dict); a file stops at the primitive that reaches the goal.
`--beam-width W` (default 1: greedy) keeps the best W partial paths per variant instead of one, each expanded into N candidates
(W <= 32, W * N <= 256), and writes the path that ends in the best one.  `--walkable file.npz` (a scene file of
`scene_gen.save_scene` that carries its walkable raster; independent of `--scene`) makes the goal term the distance along that
raster (`GeodesicField`), so the variants go round an obstacle instead of at it; the driver then prints that distance next to the
straight-line one.  `--avoid a.pkl,b.pkl` (with `--goal`) makes the people of earlier `motion_*.pkl` files moving obstacles
(`MovingObstacles.from_rollout_files`: a vertical cylinder of 0.3 m round each recorded pelvis track, frame 0 of every file being
frame 0 of this run): a candidate pays for coming within 0.5 m of one and is vetoed where the cylinders overlap, so a crowd is
composed by prioritised planning, one run per person; the driver prints the minimum clearance along each written path.
`--obstacle-model markers` (with `--avoid`; default `cylinder`) makes those recorded people the 67 world markers of each of their
frames, which the files already hold, and a candidate its own 67 blended markers (`generate_sequence_to_goal(obstacle_model=
"markers")`): limbs avoid limbs, the greedy search and the beam alike; `--obstacle-skin M` (default 0.05 m) is the marker distance
below which the two touch, and the printed clearance is then the least marker distance minus that skin.
`--start x,y,yaw_deg` places the seed's world frame (the origin, facing +y, without it): two runs without it start inside each
other.  `--people "x,y,yaw_deg:gx,gy,gz;..."` generates P people TOGETHER instead: each starts at its x,y,yaw_deg and walks to its own
goal, and every variant of `--n-gens` is one group of those P people (`generate_sequence_to_goal(groups=)`, b = n_gens * P
sequences) who choose each primitive against each other's current choices, so nobody has priority; one
`motion_<seed>_<variant>_p<person>.pkl` per person, and per variant the minimum crowd clearance, the number of overlapping
primitives along the written paths and whether the members still changed their minds in a last sweep.  It stands in for
`--start` and `--goal` and is the greedy search (`--beam-width 1`); `--scene`, `--walkable` (one field per distinct goal) and
`--avoid` keep working with it.  `--pair-model markers` (with `--people`; default `cylinder`) makes a person, to the others of the group,
the 67 blended markers of a candidate instead of a cylinder round the pelvis (`generate_sequence_to_goal(pair_model="markers")`):
limbs avoid limbs; `--pair-skin M` (default 0.05 m) is the marker distance below which two people count as touching, and the printed
crowd clearance is then the least marker distance minus that skin.  `--policy CKPT` (with `--goal` or `--people`; the greedy search) makes a trained policy the proposal
distribution of the search (`PolicyProposal`, egogen_amd/proposal.py): the checkpoint main_ppo.py writes (key `model`) is loaded into
`setup_world.build_policy`'s networks, and per primitive every sequence's observation, with its 32 egosensing rays cast against the
walkable polygon `--polygon FILE` (default: the file given to `--walkable` or `--scene` where that file holds `edges`; else no
polygon, every ray reads +1), gives mu, sigma over the latent; the candidates are mu, samples round it (`--policy-temperature`
scales sigma) and a share `--policy-prior-fraction` of prior samples.  Nobody has measured motion quality with these defaults.
`--policy-sees-people` (with `--policy`) makes the other people holes of that polygon, as in the reference's crowd evaluation: the
group-mates of `--people` (the world box of their two seed frames' markers) and the tracks of `--avoid` (the box of their cylinder
at the two seed frames); without it the policy senses the static polygon only and the selection alone knows about the people.
`--goal "x,y,z;x,y,z;..."` is a route (`generate_sequence_to_goal(route=)`, `Routes`, egogen_amd/route.py): every variant walks via
the points in order to the last one, a waypoint counting as passed within `--pass-radius` metres (default 0.5) horizontally; with
`--people` the waypoints of one person are chained with `>`: "x,y,yaw_deg:g1x,g1y,g1z>g2x,g2y,g2z;...".  A route is the greedy
search (`--beam-width 1`); `--walkable` then builds one field per distinct waypoint; the files' `wpath` holds the whole route and
the driver prints how many waypoints each path passed.  One point per person is the path without a route, unchanged.
`--lookahead H` (with `--avoid` or `--people`, cylinder models only; 0 to 8, default 0: the horizon is one primitive) lets those terms
look H further primitives ahead (`generate_sequence_to_goal(lookahead=)`): a candidate, and with `--people` everybody else, is predicted
to repeat the displacement of the own primitive, the recorded people of `--avoid` are read ahead on their tracks; a predicted overlap
costs, less `--lookahead-slack M` metres (default 0.1) per primitive of look-ahead, and only a present one vetoes.

`--cfg <name>` is the combo config (`crowd_ppo/cfg_samp20/<name>.yml` under the working directory, else the packaged copy): it
names the predictor's and the regressor's configs, whose checkpoints are read from `results/crowd_ppo/<config>/checkpoints`
(predictor `epoch-400.ckp` else `epoch-200.ckp`, regressor `epoch-100.ckp`), or, with `--ckpt-dir`, the combo checkpoint
`epoch-120.ckp` else `epoch-10.ckp` that train_GAMMACombo.py writes.  Licensed assets (SMPL-X npz, checkpoints) are used when
present; otherwise the seeded synthetic body and a seeded random-init prior stand in, as in the other drivers."""
import argparse
import os
import pickle
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from egogen_amd import setup_world as sw  # noqa: E402
from egogen_amd import synth  # noqa: E402
from egogen_amd.body_model import BodyModelHandle, SMPLXParser  # noqa: E402
from egogen_amd.canonicalize import canonicalize_frames  # noqa: E402
from egogen_amd.genop import GAMMAPrimitiveComboGenOP  # noqa: E402
from egogen_amd.models import PREDICTOR_CFG, REGRESSOR_CFG  # noqa: E402
from egogen_amd.utils import rollout_primitives  # noqa: E402


def _points(text, sep):
    """ "x,y,z<sep>x,y,z..." -> [n,3] float64; ValueError for anything else"""
    pts = np.asarray([[float(v) for v in one.split(",")] for one in text.split(sep)], np.float64)
    if pts.ndim != 2 or pts.shape[1] != 3 or not np.isfinite(pts).all():
        raise ValueError("every point takes x,y,z")
    return pts


def parse_goal_route(text):
    """`--goal` with ";" -> the waypoints [n,3] float64 (ValueError for anything else)"""
    return _points(text, ";")


def parse_people_routes(text):
    """`--people` with ">" -> (people [P,6] float64: x, y, yaw_deg and the LAST waypoint of each person, the routes: a list of
    [n_i,3] float64); ValueError for anything else"""
    people, routes = [], []
    for one in text.split(";"):
        if not one:
            continue
        halves = one.split(":")
        if len(halves) != 2 or len(halves[0].split(",")) != 3:
            raise ValueError("a person takes x,y,yaw_deg:waypoints")
        start, way = [float(v) for v in halves[0].split(",")], _points(halves[1], ">")
        people.append(start + way[-1].tolist())
        routes.append(way)
    people = np.asarray(people, np.float64)
    if people.ndim != 2 or not 1 <= people.shape[0] <= 32 or not np.isfinite(people).all():
        raise ValueError("1 to 32 people")
    return people, routes


def main(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--cfg", default="MPVAECombo_samp_2frame")
    parser.add_argument("--n-primitives", type=int, default=10)
    parser.add_argument("--n-gens", type=int, default=4)
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--out", default=os.path.join("results", "exp_GAMMAPrimitive", "gen_motion"))
    parser.add_argument("--ckpt-dir", default=None, help="directory of a combo checkpoint (train_GAMMACombo.py)")
    parser.add_argument("--num-verts", type=int, default=synth.NUM_VERTS)
    parser.add_argument("--start-frame", type=int, default=5)
    parser.add_argument("--goal", default=None, help="x,y,z in world coordinates: steer every variant there (best-of-N search)")
    parser.add_argument("--n-candidates", type=int, default=16, help="candidates per primitive and variant (with --goal)")
    parser.add_argument("--beam-width", type=int, default=1, help="partial paths kept per variant (with --goal); 1 = greedy best-of-N")
    parser.add_argument("--scene", default=None, help="npz with sdf, center, scale: penalise and avoid penetration (with --goal)")
    parser.add_argument("--walkable", default=None, help="scene file of scene_gen.save_scene with its walkable raster: the goal term "
                        "becomes the distance along the raster, round obstacles (with --goal; independent of --scene)")
    parser.add_argument("--avoid", default=None, help="comma-separated motion_*.pkl files of earlier runs: their people are moving "
                        "obstacles of this one (with --goal)")
    parser.add_argument("--obstacle-model", choices=("cylinder", "markers"), default="cylinder", help="what a recorded person of --avoid "
                        "is: a cylinder round the pelvis track, or the 67 world markers of every frame of its file (with --avoid)")
    parser.add_argument("--obstacle-skin", type=float, default=None, help="marker distance in metres below which a candidate touches a "
                        "recorded person (with --obstacle-model markers; default 0.05)")
    parser.add_argument("--start", default=None, help="x,y,yaw_deg: where the seed stands in the world and which way it faces")
    parser.add_argument("--people", default=None, help='"x,y,yaw_deg:gx,gy,gz;...": P people with a start and a goal each, generated together; '
                        "every variant is one group who avoid each other (instead of --start / --goal; greedy search)")
    parser.add_argument("--pair-model", choices=("cylinder", "markers"), default="cylinder", help="what a person is to the others of a "
                        "--people group: a cylinder round the pelvis, or the 67 blended markers of a candidate (with --people)")
    parser.add_argument("--pair-skin", type=float, default=None, help="marker distance in metres below which two people touch "
                        "(with --pair-model markers; default 0.05)")
    parser.add_argument("--policy", default=None, help="checkpoint of a trained policy (main_ppo.py, key 'model'): the proposal distribution "
                        "of the search (with --goal or --people; greedy search)")
    parser.add_argument("--policy-temperature", type=float, default=1.0, help="scale of the policy's sigma (with --policy)")
    parser.add_argument("--policy-prior-fraction", type=float, default=0.25, help="share of the candidates left as prior samples (with --policy)")
    parser.add_argument("--polygon", default=None, help="scene file with the walkable polygon (`edges`) the egosensing rays are cast against, or "
                        "room0 (with --policy); default: the --walkable or --scene file where it holds edges")
    parser.add_argument("--policy-sees-people", action="store_true", help="the policy's egosensing rays stop at the other people: the "
                        "group-mates of --people and the tracks of --avoid are holes of the polygon (with --policy)")
    parser.add_argument("--pass-radius", type=float, default=None, help="horizontal distance in metres within which a waypoint of a "
                        'route counts as passed (with ";" in --goal or ">" in --people; default 0.5)')
    parser.add_argument("--lookahead", type=int, default=0, help="further primitives the cylinder models of --avoid and --people look "
                        "ahead, 0 to 8: everybody is predicted to repeat the displacement of the own primitive (0: the horizon is one primitive)")
    parser.add_argument("--lookahead-slack", type=float, default=None, help="metres of clearance a prediction is forgiven per primitive of "
                        "look-ahead (default 0.1; an argument error without --lookahead above 0, as --pair-skin is without its model: "
                        "the operator itself takes a slack at lookahead=0 and does not read it)")
    args = parser.parse_args(argv)
    if not 0 <= args.lookahead <= 8:
        parser.error("--lookahead takes 0 to 8 primitives")
    if args.lookahead_slack is not None and (args.lookahead == 0 or not (args.lookahead_slack >= 0 and np.isfinite(args.lookahead_slack))):
        parser.error("--lookahead-slack needs --lookahead above 0 and must be finite and not negative")
    if args.lookahead > 0 and args.avoid is None and args.people is None:
        parser.error("--lookahead needs --avoid or --people: it is about when the other people are seen")
    if args.lookahead > 0 and (args.obstacle_model == "markers" or args.pair_model == "markers"):
        parser.error("--lookahead is built for the cylinder models only: not with --obstacle-model markers or --pair-model markers")
    people = way = None          # way: the waypoints of every person of a run with a route, a list of [n_i,3]
    if args.people is not None and (args.start is not None or args.goal is not None or args.beam_width != 1):
        parser.error("--people stands in for --start and --goal and is the greedy search (--beam-width 1)")
    if args.people is not None and ">" in args.people:
        try:
            people, way = parse_people_routes(args.people)
        except ValueError:
            parser.error('--people takes "x,y,yaw_deg:gx,gy,gz>gx,gy,gz..." for 1 to 32 people, separated by ";"')
        args.goal = ",".join(str(v) for v in people[0, 3:])
    elif args.people is not None:
        try:
            people = np.asarray([[float(v) for half in one.split(":") for v in half.split(",")] for one in args.people.split(";") if one], np.float64)
        except ValueError:
            people = np.zeros((0, 6))
        if people.ndim != 2 or people.shape[1] != 6 or not 1 <= people.shape[0] <= 32 or not np.isfinite(people).all() or \
                any(len(one.split(":")) != 2 or len(one.split(":")[0].split(",")) != 3 for one in args.people.split(";") if one):
            parser.error('--people takes "x,y,yaw_deg:gx,gy,gz" for 1 to 32 people, separated by ";"')
        args.goal = ",".join(str(v) for v in people[0, 3:])          # the goal-steered path; the goals themselves follow below
    if args.people is None and args.goal is not None and ";" in args.goal:
        if args.beam_width != 1:
            parser.error('a route (";" in --goal) is the greedy search (--beam-width 1)')
        try:
            way = [parse_goal_route(args.goal)]
        except ValueError:
            parser.error('--goal takes x,y,z, or "x,y,z;x,y,z;..." for a route')
        args.goal = ",".join(str(v) for v in way[0][-1])
    if args.pass_radius is not None and way is None:
        parser.error('--pass-radius needs a route: ";" in --goal or ">" in --people')
    if args.people is None and args.pair_model != "cylinder":
        parser.error("--pair-model markers needs --people: it is a model of how the people of a group see each other")
    if args.pair_skin is not None and (args.pair_model != "markers" or not (args.pair_skin >= 0 and np.isfinite(args.pair_skin))):
        parser.error("--pair-skin needs --pair-model markers and must be finite and not negative")
    if args.avoid is None and args.obstacle_model != "cylinder":
        parser.error("--obstacle-model markers needs --avoid: it is a model of the recorded people of those files")
    if args.obstacle_skin is not None and (args.obstacle_model != "markers" or not (args.obstacle_skin >= 0 and np.isfinite(args.obstacle_skin))):
        parser.error("--obstacle-skin needs --obstacle-model markers and must be finite and not negative")
    if args.goal is None and args.scene is not None:
        parser.error("--scene needs --goal")
    if args.goal is None and args.walkable is not None:
        parser.error("--walkable needs --goal")
    if args.goal is None and args.beam_width != 1:
        parser.error("--beam-width needs --goal")
    if args.goal is None and args.avoid is not None:
        parser.error("--avoid needs --goal")
    if args.policy is None and (args.polygon is not None or args.policy_temperature != 1.0 or args.policy_prior_fraction != 0.25):
        parser.error("--polygon, --policy-temperature and --policy-prior-fraction need --policy")
    if args.policy is None and args.policy_sees_people:
        parser.error("--policy-sees-people needs --policy: without a policy nothing senses the people")
    if args.policy is not None and (args.goal is None or args.beam_width != 1):
        parser.error("--policy needs --goal (or --people) and is the greedy search (--beam-width 1)")
    polygon = None
    if args.policy is not None:          # before the models and the device: a bad file ends the run here
        from egogen_amd.proposal import scene_file_edges
        if not os.path.exists(args.policy):
            raise SystemExit("--policy {}: no such file".format(args.policy))
        for f in [args.polygon] if args.polygon else [args.walkable, args.scene]:
            if f is None:
                continue
            try:
                polygon = scene_file_edges(f)
                print("[INFO] egosensing against the {} edges of {}".format(len(polygon), f))
                break
            except (OSError, ValueError, KeyError) as e:
                if args.polygon:
                    raise SystemExit("--polygon {}: {}".format(f, e))
        if polygon is None:
            print("[INFO] no walkable polygon: every egosensing ray reads +1")
    start = None
    if args.start is not None:
        try:
            start = [float(v) for v in args.start.split(",")]
        except ValueError:
            start = []
        if len(start) != 3 or not np.isfinite(start).all():
            parser.error("--start takes x,y,yaw_deg")
    obstacles = None
    if args.avoid:          # before the models and the device: a bad file ends the run here
        from egogen_amd.obstacles import MovingObstacles
        try:
            obstacles = MovingObstacles.from_rollout_files([f for f in args.avoid.split(",") if f], markers=args.obstacle_model == "markers")
        except (OSError, ValueError, KeyError, pickle.UnpicklingError, EOFError, AttributeError) as e:
            raise SystemExit("--avoid {}: {!r}".format(args.avoid, e))
        print("[INFO] avoiding {} people over {} frames{}".format(int(obstacles.count[0]), obstacles.num_frames,
                                                                  " by their markers" if args.obstacle_model == "markers" else ""))
    P = 1 if people is None else people.shape[0]
    route = None
    if way is not None:          # before the models and the device; sequence v * P + p walks the route of person p
        from egogen_amd.route import Routes
        try:
            route = Routes.from_lists([way[i % P] for i in range(args.n_gens * P)], pass_radius=0.5 if args.pass_radius is None else args.pass_radius)
        except ValueError as e:
            raise SystemExit("route: {}".format(e))
    if not torch.cuda.is_available():
        raise SystemExit("gen_motion needs a HIP device: the MI355X path has no CPU fallback")
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    goal = field = None
    if people is not None:          # sequence v * P + p is person p of variant v
        goal = np.tile(people[:, 3:].astype(np.float32), (args.n_gens, 1))
    elif args.goal is not None:
        goal = np.asarray([float(v) for v in args.goal.split(",")], np.float32)
        if goal.shape != (3,):
            raise SystemExit("--goal takes x,y,z")
    if args.walkable:        # before the models: a file without a raster, or a goal off it, ends the run here
        from egogen_amd.geodesic import GeodesicField
        try:
            if route is not None:          # one field per distinct waypoint: the search picks each sequence's by its cursor
                field = GeodesicField.from_scene(sw.load_scene_file(args.walkable, raster=True), route.field_goals())
            else:
                distinct, of_row = np.unique(goal.reshape(-1, 3), axis=0, return_inverse=True)
                field = GeodesicField.from_scene(sw.load_scene_file(args.walkable, raster=True), distinct)
            if people is not None and route is None:          # one field per distinct goal is computed, every sequence then reads its own copy
                idx = torch.as_tensor(of_row.reshape(-1), device=field.dist.device)
                field = GeodesicField(field.dist[idx].contiguous(), field.origin[idx].contiguous(), field.cell, field.goals[idx].contiguous(),
                                      field.passes)
        except ValueError as e:
            raise SystemExit("--walkable {}: {}".format(args.walkable, e))
        print("[INFO] geodesic field: {} x {} cells of {} m, {} passes".format(field.dist.shape[1], field.dist.shape[2], field.cell, field.passes))

    mc = sw._read_yaml(args.cfg + ".yml")["modelconfig"]
    pdir = os.path.join(sw.RESULTS_ROOT, mc["predictor_config"], "checkpoints")
    rdir = os.path.join(sw.RESULTS_ROOT, mc["regressor_config"], "checkpoints")
    gender = "male"
    op = GAMMAPrimitiveComboGenOP({"modelconfig": dict(PREDICTOR_CFG), "trainconfig": {"save_dir": pdir}},
                                  {"modelconfig": dict(REGRESSOR_CFG, gender=gender), "trainconfig": {"save_dir": rdir}},
                                  {"gpu_index": 0, "ckpt_dir": args.ckpt_dir, "result_dir": args.out, "seed": args.seed})
    bm, real_body = sw.load_body_model(gender, seed=args.seed, num_verts=args.num_verts)
    body = BodyModelHandle(bm, synth.marker_ids(args.num_verts), synth.feet_vids(args.num_verts))
    have_pretrained = any(os.path.exists(os.path.join(pdir, f)) for f in ("epoch-400.ckp", "epoch-200.ckp")) and \
        os.path.exists(os.path.join(rdir, "epoch-100.ckp"))
    if args.ckpt_dir:
        op.build_model(load_pretrained_model=False, body_model=body)
    elif have_pretrained:
        op.build_model(load_pretrained_model=True, body_model=body)
    else:
        print("[INFO] no checkpoints under {} / {}: seeded random-init prior".format(pdir, rdir))
        op.model, op.body_model = sw.build_motion_prior(seed=args.seed, ckpt_dirs=(pdir, rdir)), body
    print("[INFO] body model: {}".format("SMPL-X" if real_body else "synthetic"))

    # motion seed: two frames of the packaged mocap clip, moved into the frame of the first (utils_canonicalize_samp.py)
    ms = synth.load_assets()
    s = args.start_frame
    smplx = SMPLXParser({"body_models": {gender: body}})
    can = canonicalize_frames(smplx, np.asarray(ms["seed_trans"])[s:s + 2], np.asarray(ms["seed_poses"])[s:s + 2], np.asarray(ms["seed_betas"]),
                              gender)
    data = can["marker_ssm2_67"].reshape(2, 1, 201).astype(np.float32)
    bparams = np.zeros((2, 1, 93), np.float32)
    bparams[:, 0, :3], bparams[:, 0, 3:69] = can["trans"], can["poses"][:, :66]
    nseq = args.n_gens * P
    R0 = can["transf_rotmat"].astype(np.float32)[None].repeat(nseq, 0)
    T0 = can["transf_transl"].astype(np.float32).reshape(1, 3).repeat(nseq, 0)
    starts = [start] * nseq if people is None else [people[i % P, :3] for i in range(nseq)]
    for i, st in enumerate(starts):
        if st is None:
            continue        # the seed's world frame turned by yaw about z and moved so that its origin stands at (x, y)
        yaw = np.deg2rad(st[2])
        Rz = np.array([[np.cos(yaw), -np.sin(yaw), 0.0], [np.sin(yaw), np.cos(yaw), 0.0], [0.0, 0.0, 1.0]])
        R0[i] = (Rz @ R0[i].astype(np.float64)).astype(np.float32)
        T0[i] = (T0[i].astype(np.float64) @ Rz.T + np.array([st[0], st[1], 0.0])).astype(np.float32)
    if args.goal is None:
        res = op.generate_sequence(data, bparams, can["betas"].astype(np.float32), args.n_primitives, n_gens=args.n_gens, R0=R0, T0=T0)
    else:
        from egogen_amd.body_model import SdfScene
        scene = None
        if args.scene:
            with np.load(args.scene) as f:
                scene = SdfScene({k: f[k] for k in ("sdf", "center", "scale")})
        groups = None if people is None else np.arange(nseq) // P
        proposal = None
        if args.policy is not None:
            from egogen_amd.proposal import PolicyProposal
            pargs = argparse.Namespace(seed=args.seed, lr=3e-4, gamma=0.99, gae_lambda=0.95, max_grad_norm=0.1, vf_coef=1.0, ent_coef=0.01,
                                       weight_kld=0.0, rew_norm=False, eps_clip=0.1, value_clip=0, dual_clip=None, norm_adv=1, recompute_adv=0,
                                       deterministic_eval=True)
            policy = sw.build_policy(pargs)
            policy.load_state_dict(torch.load(args.policy, map_location="cuda")["model"])
            policy.eval()
            proposal = PolicyProposal(policy, edges=polygon, temperature=args.policy_temperature, prior_fraction=args.policy_prior_fraction,
                                      sense_people=args.policy_sees_people)
            print("[INFO] policy {}: {} of {} candidates from the policy, {} of them its mean{}".format(
                args.policy, proposal.counts(args.n_candidates)[1], args.n_candidates, proposal.counts(args.n_candidates)[0],
                "; it senses the other people as holes of the polygon" if args.policy_sees_people else ""))
        search = dict(scene=scene, R0=R0, T0=T0, beam_width=args.beam_width, geodesic=field, obstacles=obstacles, groups=groups, policy=proposal,
                      pair_model=args.pair_model, pair_skin=0.05 if args.pair_skin is None else args.pair_skin,
                      obstacle_model=args.obstacle_model, obstacle_skin=0.05 if args.obstacle_skin is None else args.obstacle_skin,
                      lookahead=args.lookahead, lookahead_slack=0.1 if args.lookahead_slack is None else args.lookahead_slack)
        if route is not None:
            search["route"] = route
        res = op.generate_sequence_to_goal(data.repeat(nseq, 1), bparams.repeat(nseq, 1), can["betas"].astype(np.float32),
                                           None if route is not None else goal, args.n_primitives, args.n_candidates, **search)
        for v in range(args.n_gens if people is not None else 0):
            mine = range(v * P, (v + 1) * P)
            written = np.stack([np.arange(args.n_primitives) < int(res.n_valid[i]) for i in mine], 1)          # [K,P]: the primitives the files hold
            clear, hits = np.asarray(res.crowd_clearance)[:, mine], np.asarray(res.crowd_hit)[:, mine]
            print("[INFO] variant {}: minimum crowd clearance {:.3f} m, crowd hits {}, members still changing in a last sweep {}".format(
                v, float(clear[written].min()), int(hits[written].sum()), int(np.asarray(res.joint_changed)[:, -1, v].max())))
        for i in range(nseq):
            last = int(res.n_valid[i]) - 1
            along = "" if field is None else " ({:.3f} m along the walkable raster)".format(float(res.geo_dist[last, i]))
            aim = "goal"
            if route is not None:          # goal_dist[k] is the distance to the waypoint primitive k was scored against
                scored = int(res.route_cursor[last - 1, i]) if last > 0 else 0
                aim = "goal" if scored == int(route.count[i]) - 1 else "waypoint {} of {} the last primitive aimed at".format(scored + 1, int(route.count[i]))
            print("[INFO] {}: {} primitives, final distance to the {} {:.3f} m{}, colliding choices {}".format(
                "variant {}".format(i) if people is None else "variant {} person {}".format(i // P, i % P), last + 1, aim, float(res.goal_dist[last, i]), along, int((res.status[:last + 1, i] & 1).sum())))
            if route is not None:
                print("[INFO] variant {}{}: passed {} of {} waypoints on the way".format(
                    i // P, "" if people is None else " person {}".format(i % P), int(res.route_cursor[last, i]), int(route.count[i]) - 1))
            if obstacles is not None:
                ch = np.asarray(res.choice[:last + 1, i], np.int64)
                clear = np.asarray(res.clearance)[np.arange(last + 1), i, ch]
                hits = np.asarray(res.obstacle_hit)[np.arange(last + 1), i, ch]
                print("[INFO] variant {}: minimum clearance {:.3f} m, chosen hits {}".format(i, float(clear.min()), int(hits.sum())))
    name = (lambda i: "{}_{}".format(args.seed, i)) if people is None else (lambda i: "{}_{}_p{}".format(args.seed, i // P, i % P))
    paths = [res.save(args.out, i, man_id=name(i)) for i in range(args.n_gens * P)]
    for p in paths:
        print(p)
    with open(paths[0], "rb") as fh:
        seq = rollout_primitives(pickle.load(fh)["motion"], body)
    print("frames: {}".format(seq.shape[0]))


if __name__ == "__main__":
    main()
