#!/usr/bin/env python3
"""Measure finished motions: the per-motion and crowd quality figures of `egogen_amd.metrics` for `motion_*.pkl` files
(`gen_motion.py`, `PrimitiveSequence.save`, the env's `save_rollout_results`).

`--in` takes files and directories (every motion_*.pkl of a directory, sorted).  Files named motion_<seed>_<variant>_p<person>.pkl, as
`gen_motion.py --people` names them, are the people of one scene and time line: one group per (seed, variant), measured against
each other (`crowd_metrics`); every other file is measured alone.  The goal of a file is the last point of its `wpath`; a
`wpath` of more than two points is a route (`gen_motion.py` with several waypoints), and such a file's row also says which of its
waypoints the motion passed, at which frame, and how near it came (`route_metrics`, `--pass-radius`).  With
`--scene file.npz` (keys sdf, center, scale) the bodies are posed again and their vertices inside the scene counted, on the
licensed SMPL-X model where present, else on the seeded synthetic body of `--num-verts` vertices, as in the other drivers.

Writes one JSON to `--out`: `columns` (name, unit, meaning), `files` (one row per file: the columns of `metrics.COLUMNS` and, for a
member of a group, its crowd figures), `groups` (one row per group of two or more) and `mean` (the mean over files of every
column, ignoring NaN), and prints a short table.  The definitions are written out in include/egogen_hip.h; what the figures are
not is said in egogen_amd/metrics.py."""
import argparse
import glob
import json
import os
import pickle
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from egogen_amd import metrics  # noqa: E402

TABLE = ("frames", "skate_mean", "floor_mean", "contact_score", "speed_mean", "jerk_mean", "goal_dist_end", "first_reached_frame", "pene_max")
PERSON = ("clearance_min", "marker_dist_min", "overlap_frames", "touch_frames")
GROUP = ("size", "frames_compared", "clearance_min", "marker_dist_min", "overlap_frames", "touch_frames")


def _plain(v):
    """a numpy scalar as JSON takes it: NaN and infinities become null"""
    v = v.item() if hasattr(v, "item") else v
    return None if isinstance(v, float) and not np.isfinite(v) else v


def collect(inputs):
    paths = []
    for p in inputs:
        found = sorted(glob.glob(os.path.join(p, "motion_*.pkl"))) if os.path.isdir(p) else [p]
        if not found:
            raise SystemExit("--in {}: no motion_*.pkl there".format(p))
        paths += found
    return paths


def evaluate(paths, scene=None, body_model=None, goal_thresh=None, floor_z=0.0, body_radius=0.3, touch_dist=0.05, hold=False,
             pass_radius=0.5):
    """-> the dict `main` writes"""
    ms = metrics.MotionSet.from_rollout_files(paths, groups="names")
    per = metrics.motion_metrics(ms, goal_thresh=goal_thresh, floor_z=floor_z, scene=scene, body_model=body_model)
    crowd = metrics.crowd_metrics(ms, body_radius=body_radius, touch_dist=touch_dist, hold=hold)
    names = [c[0] for c in metrics.COLUMNS]
    route = None if ms.routes is None else metrics.route_metrics(ms, pass_radius=pass_radius)
    size_of = dict(zip(crowd["group"]["id"].tolist(), crowd["group"]["size"].tolist()))
    files = []
    for i, path in enumerate(paths):
        row = {"file": path, "group": int(ms.groups[i])}
        row.update({k: _plain(per[k][i]) for k in names})
        if size_of[int(ms.groups[i])] > 1:
            row.update({k: _plain(crowd["person"][k][i]) for k in PERSON})
        if route is not None and route["count"][i] > 0:          # the file carries a route: wpath[1:]
            n = int(route["count"][i])
            row.update({"waypoints": n, "waypoints_passed": int(route["waypoints_passed"][i]),
                        "pass_frame": [int(v) for v in route["pass_frame"][i, :n]],
                        "approach_min": [_plain(float(v)) for v in route["approach_min"][i, :n]]})
        files.append(row)
    groups = []
    for g, gid in enumerate(crowd["group"]["id"].tolist()):
        if crowd["group"]["size"][g] < 2:
            continue
        row = {"group": int(gid), "files": [paths[i] for i in np.flatnonzero(ms.groups == gid)]}
        row.update({k: _plain(crowd["group"][k][g]) for k in GROUP})
        groups.append(row)
    with np.errstate(all="ignore"):
        mean = {k: _plain(np.nanmean(per[k].astype(np.float64))) if np.isfinite(per[k].astype(np.float64)).any() else None for k in names}
    return {"columns": [{"name": c[0], "unit": c[1], "meaning": c[3]} for c in metrics.COLUMNS], "goal_thresh": 0.1 if goal_thresh is None else goal_thresh,
            **({} if route is None else {"pass_radius": pass_radius}), "floor_z": floor_z, "body_radius": body_radius, "touch_dist": touch_dist, "hold": bool(hold), "files": files, "groups": groups, "mean": mean}


def main(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--in", dest="inputs", nargs="+", required=True, help="motion_*.pkl files and directories of them")
    parser.add_argument("--scene", default=None, help="npz with sdf, center, scale: count the bodies' vertices inside it")
    parser.add_argument("--goal-thresh", type=float, default=None, help="reached within this distance of the goal (default 0.1 m)")
    parser.add_argument("--floor-z", type=float, default=0.0, help="height of the floor in the world")
    parser.add_argument("--body-radius", type=float, default=0.3, help="radius of the search's cylinder model of a person")
    parser.add_argument("--touch-dist", type=float, default=0.05, help="two people's markers closer than this touch")
    parser.add_argument("--pass-radius", type=float, default=0.5, help="a waypoint of a route counts as passed within this horizontal distance")
    parser.add_argument("--hold", action="store_true", help="a person whose file has ended stands at the last position")
    parser.add_argument("--num-verts", type=int, default=None, help="vertices of the synthetic body (with --scene, without SMPL-X)")
    parser.add_argument("--seed", type=int, default=0, help="seed of the synthetic body (with --scene)")
    parser.add_argument("--out", required=True, help="the JSON to write")
    args = parser.parse_args(argv)
    paths = collect(args.inputs)
    if not torch.cuda.is_available():
        raise SystemExit("eval_motion needs a HIP device: the MI355X path has no CPU fallback")
    scene = body = None
    if args.scene:
        from egogen_amd import setup_world as sw
        from egogen_amd import synth
        from egogen_amd.body_model import BodyModelHandle, SdfScene
        with open(paths[0], "rb") as fh:
            gender = str(pickle.load(fh)["motion"][0].get("gender", "male"))
        nv = synth.NUM_VERTS if args.num_verts is None else args.num_verts
        bm, real_body = sw.load_body_model(gender, seed=args.seed, num_verts=nv)
        body = BodyModelHandle(bm, synth.marker_ids(nv), synth.feet_vids(nv))
        with np.load(args.scene) as f:
            scene = SdfScene({k: f[k] for k in ("sdf", "center", "scale")})
        print("[INFO] body model: {}".format("SMPL-X" if real_body else "synthetic"))
    try:
        res = evaluate(paths, scene, body, args.goal_thresh, args.floor_z, args.body_radius, args.touch_dist, args.hold, args.pass_radius)
    except (ValueError, OSError, KeyError, pickle.UnpicklingError, EOFError) as e:
        raise SystemExit("eval_motion: {!r}".format(e))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1, allow_nan=False)
    fmt = lambda v: "-" if v is None else ("{:d}".format(v) if isinstance(v, int) else "{:.4g}".format(v))
    print(" | ".join(("file",) + TABLE))
    for row in res["files"]:
        print(" | ".join([os.path.basename(row["file"])] + [fmt(row[k]) for k in TABLE]))
    print(" | ".join(["mean"] + [fmt(res["mean"][k]) for k in TABLE]))
    for row in res["groups"]:
        print("group {}: ".format(row["group"]) + ", ".join("{} {}".format(k, fmt(row[k])) for k in GROUP))
    print(args.out)


if __name__ == "__main__":
    main()
