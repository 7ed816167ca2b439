#!/usr/bin/env python3
"""The policy's observation with other people in it (`PolicyProposal(sense_people=True)`, entries egx_primitive_people_boxes and
egx_primitive_observe_people): what it costs, and what it does to the four people who swap places.  GPU only.

    python scripts/bench_genop_policy_people.py [--iters 20] [--out-dir profiles] [--num-verts V]
    python scripts/bench_genop_policy_people.py --unchanged-only --tree <root of another checkout> --json out.json

Launches: b = 64 and 512 sequences in groups of four, N = 16, every group standing at the same four places inside the room0 polygon
(89 edges; groups do not see each other, so where they stand relative to one another does not matter), two recorded tracks per
sequence: egx_primitive_observe, egx_primitive_people_boxes and egx_primitive_observe_people (with its 3 + 2 holes, and with no
hole) on the same inputs.  Search: the README's four-people swap (the setting of scripts/sweep_search_quality.py: 8 variants, K = 10,
N = 16, `groups=`) inside a 12 m square, per primitive, with `policy=None`, with a policy that does not sense the people and with
one that does.  Device events; the legs alternate, three windows per leg after --warmup, median and range.  Evaluation: the motions
of the last two, through `egogen_amd.metrics`.  THE POLICY IS `setup_world.build_policy`'S RANDOM INITIALISATION: the evaluation
shows mechanism and cost, not quality.
`--unchanged-only` times the loop with the policy that does not sense people alone, importing the package from `--tree`: run on this
checkout and on its parent in turns, it is the yardstick for the path this feature must not change.
Writes `<out-dir>/genop_policy_people.md` (sections between markers) and `<out-dir>/genop_policy_people.json`."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARKS = {"launches": ("<!-- launches:begin -->", "<!-- launches:end -->"), "search": ("<!-- search:begin -->", "<!-- search:end -->"),
         "swap": ("<!-- swap:begin -->", "<!-- swap:end -->")}
BATCHES, N, K = (64, 512), 16, 10
PER_MOTION = ("frames", "goal_dist_end", "skate_mean", "floor_mean", "contact_score", "speed_mean")


class PolicyArgs:
    seed = 0; lr = 3e-4; gamma = 0.99; gae_lambda = 0.95; max_grad_norm = 0.1; vf_coef = 1.0; ent_coef = 0.01
    weight_kld = 0; rew_norm = False; eps_clip = 0.1; value_clip = 0; dual_clip = None; norm_adv = 1; recompute_adv = 0
    deterministic_eval = False


def write_section(out_dir, which, lines):
    begin, end = MARKS[which]
    md = os.path.join(out_dir, "genop_policy_people.md")
    os.makedirs(out_dir, exist_ok=True)
    txt = open(md).read() if os.path.exists(md) else "# The policy's observation with other people in it\n"
    body = "\n".join([begin] + lines + [end])
    if begin in txt and end in txt:
        txt = txt[:txt.index(begin)] + body + txt[txt.index(end) + len(end):]
    else:
        txt += "\n" + body + "\n"
    with open(md, "w") as fh:
        fh.write(txt)


fmt = lambda v: f"{v['median_us']:.1f} ({v['min_us']:.1f} .. {v['max_us']:.1f})"


def launch_inputs(b):
    """-> what the launches read for b sequences in groups of four, as CPU tensors, and the two tracks of every sequence [b,2,40,2]:
    member p of every group stands at the p-th of four places 0.9 m apart in the open part of room0, clear of its mates' boxes (a
    marker cloud of 0.08 m) and of its own two tracks (0.9 m beside it, radius 0.3 m)."""
    g = torch.Generator().manual_seed(b)
    rows = b * N
    spot = torch.tensor([[0.4, -0.1], [0.9, 0.7], [0.45, 1.5], [0.9, 2.3]])[torch.arange(b) % 4]
    J = torch.randn(rows * 20, 127, 3, generator=g) * 0.03 + torch.tensor([0.0, 0.0, 1.6])
    J[:, 56:58, 1] += 0.1                                                                        # everybody looks along +y of its frame
    yaw = torch.rand(b, generator=g) * 6.28
    R = torch.zeros(b, 3, 3)
    R[:, 0, 0], R[:, 0, 1], R[:, 1, 0], R[:, 1, 1], R[:, 2, 2] = torch.cos(yaw), -torch.sin(yaw), torch.sin(yaw), torch.cos(yaw), 1.0
    T = torch.zeros(b, 3)
    T[:, :2] = spot
    d = {"joints": J, "choice": torch.randint(0, N, (b,), generator=g).int(), "R_prev": R, "T_prev": T, "R0": R.repeat_interleave(N, 0).contiguous(),
         "T0": T.repeat_interleave(N, 0).contiguous(), "x0": torch.randn(rows, 201, generator=g) * 0.08, "x1": torch.randn(rows, 201, generator=g) * 0.08,
         "goal": T + torch.tensor([0.5, 2.0, 0.9])}
    xy = (spot[:, None, None, :] + torch.tensor([[0.9, 0.2], [-0.3, 0.9]])[None, :, None, :] + torch.zeros(b, 2, 40, 2)).contiguous()
    return d, xy


def launches(args, record):
    from bench_genop import alternate
    from egogen_amd import _lib, synth
    from egogen_amd.crowd import PersonGroups
    lib, st = _lib.load(), _lib.current_stream_ptr()
    vp = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    room0 = torch.from_numpy(synth.rings_to_edges(synth.room0_polygon()).astype(np.float32)).cuda()
    off = torch.tensor([0, room0.shape[0]], dtype=torch.int32, device="cuda")
    lines = [f"Device: {torch.cuda.get_device_name(0)}; N = {N}, groups of four, the room0 polygon (89 edges), 3 mates + 2 tracks per sequence; "
             f"{10 * args.iters} launches per window, three windows per leg, the legs taking turns.  Microseconds per launch: median (range).", "",
             "| b | leg | us |", "|---|---|---|"]
    for b in BATCHES:
        d, xy = launch_inputs(b)
        d, xy = {k: v.cuda().contiguous() for k, v in d.items()}, xy.cuda()
        crowd = PersonGroups.from_ids(np.arange(b) // 4, b).to("cuda")
        radius, count = torch.full((b, 2), 0.3, device="cuda"), torch.full((b,), 2, dtype=torch.int32, device="cuda")
        index = torch.arange(b, dtype=torch.int32, device="cuda")
        scene = torch.zeros(b, dtype=torch.int32, device="cuda")
        o = (torch.empty(b, 2, 402, device="cuda"), torch.empty(b, 2, 32, device="cuda"), torch.empty(b, device="cuda"), torch.empty(b, device="cuda"))
        box, cnt = torch.empty(b, 4, device="cuda"), torch.empty(b, dtype=torch.int32, device="cuda")
        lead = (vp(d["joints"]), 20, 18, vp(d["choice"]), N, vp(d["R_prev"]), vp(d["T_prev"]), vp(d["R0"]), vp(d["T0"]), vp(d["x0"]), vp(d["x1"]), 201,
                vp(d["goal"]), vp(room0), vp(off), vp(scene), 1, 7.0, 3, 13, b)
        outs = tuple(vp(t) for t in o)
        holes = (vp(crowd.group_start), vp(crowd.group_member), vp(crowd.member_group), len(crowd), vp(xy), vp(radius), vp(count), vp(index), b, 2, 40, 19)
        none = (None, None, None, 0, None, None, None, None, 0, 0, 0, 0)
        legs = {"egx_primitive_observe": lambda: _lib.check(lib.egx_primitive_observe(*lead, *outs, st), "observe"),
                "egx_primitive_people_boxes": lambda: _lib.check(lib.egx_primitive_people_boxes(vp(d["x0"]), vp(d["x1"]), 201, vp(d["R0"]), vp(d["T0"]), N, b,
                                                                                                vp(box), st), "boxes"),
                "egx_primitive_observe_people, 3 + 2 holes": lambda: _lib.check(lib.egx_primitive_observe_people(*lead, vp(box), *holes, vp(cnt), *outs, st),
                                                                                "observe_people"),
                "egx_primitive_observe_people, no hole": lambda: _lib.check(lib.egx_primitive_observe_people(*lead, None, *none, vp(cnt), *outs, st),
                                                                            "observe_people")}
        legs["egx_primitive_people_boxes"]()
        legs["egx_primitive_observe_people, 3 + 2 holes"]()
        torch.cuda.synchronize()
        assert cnt.tolist() == [5] * b and float(o[1].min()) > -1.0, "every sequence must see its 3 mates and 2 tracks"
        t = alternate(legs, 10 * args.iters, args.warmup)
        for name, v in t.items():
            lines.append(f"| {b} | {name} | {fmt(v)} |")
        record["launches"][f"b={b}"] = t
    write_section(args.out_dir, "launches", lines)
    print("\n".join(lines))


def swap_world(args):
    import sweep_search_quality as swq
    from egogen_amd import setup_world as sw, synth
    op, data, bparams, betas, goal, R0, T0, variant = swq.setup(args.num_verts, args.seed)
    policy = sw.build_policy(PolicyArgs())
    floor = synth.rings_to_edges([synth.rect_ring(np.array([-6.0, -6.0]), np.array([6.0, 6.0]), True)]).astype(np.float32)
    return op, (data, bparams, betas, goal), dict(R0=R0, T0=T0, groups=variant), policy, floor, variant


def search_legs(args, op, call, kw, props):
    """-> per leg the closure that repeats the primitive loop of one search call on its own buffers, every pass from the same draws"""
    from bench_genop_search import captured
    b = len(kw["groups"])
    z = torch.randn(K, b * N, 128, generator=torch.Generator().manual_seed(args.seed)).cuda()
    legs = {}
    for name, prop in props.items():
        loop, sf = captured(op, "_search_loop", lambda: op.generate_sequence_to_goal(*call, K, N, z=z, to_numpy=False, policy=prop, **kw))

        def run(loop=loop, state=sf[3]):
            state["z"].copy_(z)
            loop()
        legs[name] = run
    return legs


def unchanged_only(args):
    from bench_genop import alternate
    from egogen_amd.proposal import PolicyProposal
    op, call, kw, policy, floor, _ = swap_world(args)
    t = alternate(search_legs(args, op, call, kw, {"loop": PolicyProposal(policy, edges=floor)}), args.iters, args.warmup)["loop"]
    t = {k: v / K for k, v in t.items()}
    with open(args.json, "w") as fh:
        json.dump(dict(t, tree=os.path.abspath(args.tree), device=torch.cuda.get_device_name(0)), fh)
    print(args.tree, fmt(t))


def search_and_swap(args, record):
    from bench_genop import alternate
    from egogen_amd import metrics
    from egogen_amd.proposal import PolicyProposal
    op, call, kw, policy, floor, variant = swap_world(args)
    b = len(variant)
    props = {"policy=None": None, "policy, blind to people": PolicyProposal(policy, edges=floor),
             "policy, sense_people=True": PolicyProposal(policy, edges=floor, sense_people=True)}
    t = alternate(search_legs(args, op, call, kw, props), args.iters, args.warmup)
    lines = [f"Device: {torch.cuda.get_device_name(0)}; the four-people swap, {b // 4} variants (b = {b}), K = {K}, N = {N}, `groups=`, body of "
             f"{args.num_verts} vertices, a 12 m square floor as the polygon, random-init policy; {args.iters} passes of the primitive loop per window, "
             "three windows per leg, the legs taking turns.  Microseconds per primitive: median (range).", "", "| leg | us per primitive |", "|---|---|"]
    for name, v in t.items():
        v = {k: x / K for k, x in v.items()}
        record["search"][name] = v
        lines.append(f"| {name} | {fmt(v)} |")
    d = record["search"]["policy, sense_people=True"]["median_us"] - record["search"]["policy, blind to people"]["median_us"]
    lines.append(f"| sensing the people, per primitive (difference of the two policy medians) | {d:.1f} |")
    write_section(args.out_dir, "search", lines)
    print("\n".join(lines))

    rows = []
    for name in ("policy, blind to people", "policy, sense_people=True"):
        torch.manual_seed(args.seed)
        res = op.generate_sequence_to_goal(*call, K, N, policy=props[name], **kw)
        ms = metrics.MotionSet.from_sequences(res)
        per = metrics.motion_metrics(ms, goal_thresh=0.1)
        crowd = metrics.crowd_metrics(ms, groups=variant, hold=True)
        row = {"leg": name, "reached": float((per["first_reached_frame"] >= 0).mean())}
        row.update({k: float(np.mean(per[k])) for k in PER_MOTION})
        row.update(clearance_min=float(crowd["group"]["clearance_min"].min()), overlap=int(crowd["group"]["overlap_frames"].sum()),
                   touch=int(crowd["group"]["touch_frames"].sum()), compared=int(crowd["group"]["frames_compared"].sum()),
                   rays_below_one=float((np.asarray(res.obs_egosensing) < 1.0).mean()),
                   holes_mean=float(np.mean(res.obs_people_count)) if res.obs_people_count is not None else 0.0)
        rows.append(row)
    record["swap"] = rows
    units = dict((c[0], c[1]) for c in metrics.COLUMNS)
    cols = ["leg", "reached"] + list(PER_MOTION) + ["clearance_min", "overlap", "touch", "compared", "rays_below_one", "holes_mean"]
    head = ["leg", "reached"] + [f"{k} ({units[k]})" for k in PER_MOTION] + ["clearance_min (m)", "overlap (frames)", "touch (frames)", "frames compared",
                                                                           "share of rays below +1", "holes per observation"]
    cell = lambda v: v if isinstance(v, str) else (str(v) if isinstance(v, int) else f"{v:.4g}")
    lines = ["The same call (torch seed " + str(args.seed) + ", default weights and margins) with the two policies, evaluated with `egogen_amd.metrics` as "
             "scripts/sweep_search_quality.py does (goal_thresh 0.1; body_radius 0.3, touch_dist 0.05, hold on).  **The policy is "
             "`setup_world.build_policy`'s random initialisation** (no trained checkpoint is at hand): its mean is near 0 and its sigma near 1 "
             "whatever it senses, so the rows show that the observation changes (the last two columns) and what that costs, not what a trained "
             "policy would do with it.  Nobody has measured quality.", "", "| " + " | ".join(head) + " |", "|" + "---|" * len(head)]
    lines += ["| " + " | ".join(cell(r[k]) for k in cols) + " |" for r in rows]
    write_section(args.out_dir, "swap", lines)
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--num-verts", type=int, default=None)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--tree", default=ROOT, help="root of the checkout whose package is imported")
    ap.add_argument("--unchanged-only", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import egogen_amd                       # first: the package is the tree's, whatever the helper scripts put on the path after it
    assert os.path.dirname(os.path.dirname(os.path.abspath(egogen_amd.__file__))) == os.path.abspath(args.tree), egogen_amd.__file__
    import bench_genop, bench_genop_search, sweep_search_quality  # noqa: E401,F401  (this checkout's: they only drive the package)
    if args.num_verts is None:
        from egogen_amd import synth
        args.num_verts = synth.NUM_VERTS
    if not torch.cuda.is_available():
        sys.exit("bench_genop_policy_people.py measures on the GPU; no device is visible")
    if args.unchanged_only:
        return unchanged_only(args)
    record = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "num_verts": args.num_verts, "launches": {}, "search": {}}
    launches(args, record)
    search_and_swap(args, record)
    with open(os.path.join(args.out_dir, "genop_policy_people.json"), "w") as fh:
        json.dump(record, fh, indent=1)


if __name__ == "__main__":
    main()
