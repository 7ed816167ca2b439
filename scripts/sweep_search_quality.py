#!/usr/bin/env python3
"""What the primitive search does to the motions it writes, measured with the evaluator (egogen_amd/metrics.py): the four people
who swap places in the README's `gen_motion.py --people` example, on the synthetic world, at n_candidates 1, 4 and 16, with and
without `groups=`, 8 variants of 10 primitives each.  GPU only.

    python scripts/sweep_search_quality.py [--out-dir profiles] [--num-verts V]
    python scripts/sweep_search_quality.py --pair-models [--out-dir profiles]       (cylinder against marker pair model)

The motion prior is `setup_world.build_motion_prior`'s seeded random initialisation and the body the seeded synthetic one (licensed
assets are not used here even where present, so the table can be reproduced anywhere).  The table therefore measures what the
SEARCH does to such motions - is the goal reached, are overlaps avoided, what does it cost in skating - and says nothing about the
motion quality of a trained model.  Writes `<out-dir>/motion_quality.md`.

`--pair-models`: the same four people, with `groups=`, at n_candidates 4 and 16, the joint step's cylinder model against its marker
model (`pair_model="markers"`, pair_skin 0.05 = the evaluator's touch_dist).  Writes the section between the `effect` markers of
`<out-dir>/genop_joint_markers.md` and leaves motion_quality.md alone."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from egogen_amd import metrics, synth  # noqa: E402
from egogen_amd import setup_world as sw  # noqa: E402

PEOPLE = "2,0,90:-2,0,0.9;-2,0,-90:2,0,0.9;0,2,180:0,-2,0.9;0,-2,0:0,2,0.9"       # the README's four-people swap
CANDIDATES, VARIANTS, K = (1, 4, 16), 8, 10
PER_MOTION = ("frames", "goal_dist_end", "skate_mean", "floor_mean", "contact_score", "speed_mean", "acc_mean", "jerk_mean")
HEAD = """# What the primitive search does to the motions it writes

**The motion prior here is `setup_world.build_motion_prior`'s seeded random initialisation, on the seeded synthetic body.**  This table
measures what the search does to such motions (goal reached, overlaps avoided, at what cost in skating), not the motion quality of a
trained model: no trained checkpoint has been run through it.

Four people swap places (the README's `gen_motion.py --people` example: starts 2 m from the centre, goals opposite), {variants} variants,
{K} primitives, `generate_sequence_to_goal` with its default weights and margins, at n_candidates 1, 4 and 16, with `groups=` (the members of a
variant choose against each other) and without (everybody searches alone).  Figures from `egogen_amd.metrics` (`motion_metrics`, goal_thresh
0.1; `crowd_metrics`, body_radius 0.3, touch_dist 0.05, hold on, the four people of a variant as one group in both arms); per-motion columns
are means over the {files} files of an arm, `reached` the share of files that come within goal_thresh, `overlap` / `touch` the frames summed
over the {variants} groups on which some pair's cylinders overlap / some pair's markers are closer than touch_dist.  Written by
scripts/sweep_search_quality.py.
"""


def setup(num_verts, seed):
    """the operator, the seed and the start frames as exp_GAMMAPrimitive/gen_motion.py builds them"""
    from egogen_amd.body_model import BodyModelHandle, SMPLXParser
    from egogen_amd.canonicalize import canonicalize_frames
    from egogen_amd.genop import GAMMAPrimitiveComboGenOP
    from egogen_amd.models import PREDICTOR_CFG, REGRESSOR_CFG
    gender = "male"
    op = GAMMAPrimitiveComboGenOP({"modelconfig": dict(PREDICTOR_CFG), "trainconfig": {}}, {"modelconfig": dict(REGRESSOR_CFG, gender=gender), "trainconfig": {}},
                                  {"gpu_index": 0})
    body = BodyModelHandle(synth.make_body_model(seed, num_verts=num_verts), synth.marker_ids(num_verts), synth.feet_vids(num_verts))
    op.model, op.body_model = sw.build_motion_prior(seed=seed, ckpt_dirs=(os.devnull, os.devnull)), body      # no checkpoint: the seeded init
    ms = synth.load_assets()
    can = canonicalize_frames(SMPLXParser({"body_models": {gender: body}}), np.asarray(ms["seed_trans"])[5:7], np.asarray(ms["seed_poses"])[5:7],
                              np.asarray(ms["seed_betas"]), gender)
    data = can["marker_ssm2_67"].reshape(2, 1, 201).astype(np.float32)
    bparams = np.zeros((2, 1, 93), np.float32)
    bparams[:, 0, :3], bparams[:, 0, 3:69] = can["trans"], can["poses"][:, :66]
    people = np.asarray([[float(v) for half in one.split(":") for v in half.split(",")] for one in PEOPLE.split(";")], np.float64)
    P, nseq = people.shape[0], VARIANTS * people.shape[0]
    R0 = can["transf_rotmat"].astype(np.float32)[None].repeat(nseq, 0)
    T0 = can["transf_transl"].astype(np.float32).reshape(1, 3).repeat(nseq, 0)
    for i in range(nseq):
        x, y, yaw = people[i % P, :3]
        yaw = np.deg2rad(yaw)
        Rz = np.array([[np.cos(yaw), -np.sin(yaw), 0.0], [np.sin(yaw), np.cos(yaw), 0.0], [0.0, 0.0, 1.0]])
        R0[i] = (Rz @ R0[i].astype(np.float64)).astype(np.float32)
        T0[i] = (T0[i].astype(np.float64) @ Rz.T + np.array([x, y, 0.0])).astype(np.float32)
    goal = np.tile(people[:, 3:].astype(np.float32), (VARIANTS, 1))
    return op, data.repeat(nseq, 1), bparams.repeat(nseq, 1), can["betas"].astype(np.float32), goal, R0, T0, np.arange(nseq) // P


def measure(op, data, bparams, betas, goal, R0, T0, variant, N, seed, **search):
    """one arm: the search with `search`'s keywords at N candidates, then the evaluator -> the figures of a table row"""
    torch.manual_seed(seed)
    res = op.generate_sequence_to_goal(data, bparams, betas, goal, K, N, R0=R0, T0=T0, **search)
    ms = metrics.MotionSet.from_sequences(res)
    per = metrics.motion_metrics(ms, goal_thresh=0.1)
    crowd = metrics.crowd_metrics(ms, groups=variant, hold=True)
    row = {"N": N, "reached": float((per["first_reached_frame"] >= 0).mean())}
    row.update({k: float(np.mean(per[k])) for k in PER_MOTION})
    row.update(clearance_min=float(crowd["group"]["clearance_min"].min()), marker_dist_min=float(crowd["group"]["marker_dist_min"].min()),
               overlap=int(crowd["group"]["overlap_frames"].sum()), touch=int(crowd["group"]["touch_frames"].sum()),
               compared=int(crowd["group"]["frames_compared"].sum()))
    if search.get("groups") is not None:
        row.update(search_hits=int(np.asarray(res.crowd_hit).sum()), still_changing=int(np.asarray(res.joint_changed)[:, -1].sum()))
    return row


EFFECT_MARKS = ("<!-- effect:begin -->", "<!-- effect:end -->")
EFFECT_COLS = ("N", "pair_model", "touch", "marker_dist_min", "overlap", "clearance_min", "goal_dist_end", "reached", "skate_mean", "search_hits",
               "still_changing", "compared")
EFFECT_HEAD = ("n_candidates", "pair_model", "touch (frames)", "marker_dist_min (m)", "overlap (frames)", "clearance_min (m)", "goal_dist_end (m)",
               "reached", "skate_mean (m/s)", "crowd hits in the search (member-primitives)", "members changing in a last sweep", "frames compared")


def pair_models(args):
    """the `effect` section of genop_joint_markers.md"""
    world = setup(args.num_verts, args.seed)
    variant = world[-1]
    rows = []
    for N in (4, 16):
        for model in ("cylinder", "markers"):
            row = measure(*world, N, args.seed, groups=variant, pair_model=model)
            row["pair_model"] = model
            rows.append(row)
            print(row)
    fmt = lambda v: v if isinstance(v, str) else (str(v) if isinstance(v, int) else f"{v:.4g}")
    lines = [EFFECT_MARKS[0],
             f"The four-people swap of motion_quality.md ({VARIANTS} variants, {K} primitives, default weights and margins, `groups=`), the joint step with "
             "its cylinder model against its marker model (pair_skin 0.05 m); the evaluator's figures as there (`crowd_metrics` with body_radius 0.3, "
             "touch_dist 0.05, hold on), per-motion columns means over the files of an arm.  **This is a random-init prior, so the table shows the "
             "mechanism and not motion quality.**  Written by scripts/sweep_search_quality.py --pair-models.", "",
             "| " + " | ".join(EFFECT_HEAD) + " |", "|" + "---|" * len(EFFECT_HEAD)]
    lines += ["| " + " | ".join(fmt(r[k]) for k in EFFECT_COLS) + " |" for r in rows]
    lines += ["", f"Device: {torch.cuda.get_device_name(0)}; synthetic body of {args.num_verts} vertices, seed {args.seed}.", EFFECT_MARKS[1]]
    md = os.path.join(args.out_dir, "genop_joint_markers.md")
    os.makedirs(args.out_dir, exist_ok=True)
    txt = open(md).read() if os.path.exists(md) else "# The marker-level pair model of the joint search\n"
    body = "\n".join(lines)
    if EFFECT_MARKS[0] in txt and EFFECT_MARKS[1] in txt:
        txt = txt[:txt.index(EFFECT_MARKS[0])] + body + txt[txt.index(EFFECT_MARKS[1]) + len(EFFECT_MARKS[1]):]
    else:
        txt += "\n" + body + "\n"
    with open(md, "w") as fh:
        fh.write(txt)
    print(body)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--num-verts", type=int, default=synth.NUM_VERTS)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--pair-models", action="store_true", help="cylinder against marker pair model: the effect section of genop_joint_markers.md")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sweep_search_quality.py runs the search on the GPU; no device is visible")
    if args.pair_models:
        return pair_models(args)
    op, data, bparams, betas, goal, R0, T0, variant = setup(args.num_verts, args.seed)
    rows = []
    for N in CANDIDATES:
        for joint in (False, True):
            row = measure(op, data, bparams, betas, goal, R0, T0, variant, N, args.seed, groups=variant if joint else None)
            row["groups"] = "yes" if joint else "no"
            rows.append(row)
            print(row)
    units = dict((c[0], c[1]) for c in metrics.COLUMNS)
    cols = ["N", "groups", "reached"] + list(PER_MOTION) + ["clearance_min", "marker_dist_min", "overlap", "touch", "compared"]
    head = ["n_candidates", "groups=", "reached"] + [f"{k} ({units[k]})" for k in PER_MOTION] + \
           ["clearance_min (m)", "marker_dist_min (m)", "overlap (frames)", "touch (frames)", "frames compared"]
    fmt = lambda v: v if isinstance(v, str) else (str(v) if isinstance(v, int) else f"{v:.4g}")
    lines = [HEAD.format(variants=VARIANTS, K=K, files=len(variant)), "| " + " | ".join(head) + " |", "|" + "---|" * len(head)]
    lines += ["| " + " | ".join(fmt(r[k]) for k in cols) + " |" for r in rows]
    lines += ["", f"Device: {torch.cuda.get_device_name(0)}; synthetic body of {args.num_verts} vertices, seed {args.seed}."]
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "motion_quality.md"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines[-len(rows) - 4:]))


if __name__ == "__main__":
    main()
