#!/usr/bin/env python3
"""Look-ahead in the primitive search (`generate_sequence_to_goal(lookahead=, lookahead_slack=)`, entries
egx_obstacle_ahead_clearance and egx_primitive_select_joint_ahead): what it costs, that `lookahead=0` did not move, and what it does
to the crowd figures.  GPU only.

    python scripts/bench_genop_lookahead.py [--iters 60] [--out-dir profiles]                 (the `cost` section)
    python scripts/bench_genop_lookahead.py --lib <parent .so> --save parent.json, then --parent parent.json
                                                                  (`lookahead=0` on both builds, one process each: the `parent` section)
    python scripts/bench_genop_lookahead.py --effect [--out-dir profiles]                      (the `effect` section)

Cost, in one process, at the README's four-people shape (4 variants of 4 people who swap places on a circle of 2 m, N = 16, K = 10
primitives, S = 2 sweeps, no scene) and at the README's `--avoid` example (one person, N = 16, against one recorded person): device
events around --iters passes of the whole primitive loop at H = 0, 1, 2 and 8, and around ten times as many single launches of the
new entry at H = 1, 2, 8 next to the launch it stands beside (egx_primitive_select_joint; the cylinder selection
egx_primitive_select_obstacles and the table's selection egx_primitive_select_obstacle_markers) on the same rows; the legs take turns,
three windows per leg after --warmup, median and range (scripts/bench_genop_joint.py's procedure).

`--save` / `--parent`: the loops with groups and with obstacles at `lookahead=0` - the launches of the parent build - on the parent's
library and on this one; held where this build's median is within 3 % of the parent's or inside the parent's own window, the bound
profiles/genop_joint.md uses for a change that should change nothing.

`--effect`: `crowd_metrics` (body_radius 0.3, touch_dist 0.05, hold on) of the four-people swap and of the two-person `--avoid` example
at H = 0 against H = 2, with the seeded random-init prior of scripts/sweep_search_quality.py: what the mechanism does to such motions,
not a quality claim."""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from egogen_amd import _lib  # noqa: E402

MARKS = {k: (f"<!-- {k}:begin -->", f"<!-- {k}:end -->") for k in ("parent", "cost", "effect")}
NEW = ("egx_obstacle_ahead_clearance", "egx_primitive_select_joint_ahead")
G, P, N, K, S = 4, 4, 16, 10, 2
AHEAD = (1, 2, 8)
NAME, TITLE = "genop_lookahead.md", "# Look-ahead in the primitive search\n"


def use_library(path):
    """every later `_lib.load()` opens `path`; the parent build lacks the two new symbols"""
    _lib.LIB_PATH = os.path.abspath(path)
    probe = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        if not hasattr(probe, name):
            _lib.SIGNATURES.pop(name, None)


def write_section(out_dir, which, lines):
    """the section between the `which` markers of <out_dir>/genop_lookahead.md, replaced or appended"""
    begin, end = MARKS[which]
    md = os.path.join(out_dir, NAME)
    os.makedirs(out_dir, exist_ok=True)
    txt = open(md).read() if os.path.exists(md) else TITLE
    body = "\n".join([begin] + lines + [end])
    if begin in txt and end in txt:
        txt = txt[:txt.index(begin)] + body + txt[txt.index(end) + len(end):]
    else:
        txt += "\n" + body + "\n"
    with open(md, "w") as fh:
        fh.write(txt)


def per_primitive(t):
    for v in t.values():
        for q in ("median_us", "min_us", "max_us"):
            v[q] /= K
    return t


def worlds(args):
    """the operator, the four-people swap and the two-person example -> (op, swap: (call, groups), avoid: (call, obstacles))"""
    from bench_genop_joint import swap_people
    from bench_genop_search import build_op
    from egogen_amd import MovingObstacles
    op, body = build_op(args.num_verts)
    g = torch.Generator().manual_seed(1)
    data, xb, betas, goal, kw, groups = swap_people(body, G, P, N, g)
    kw["z"] = torch.randn(K, G * P * N, 128, generator=g).cuda()
    swap = lambda **more: op.generate_sequence_to_goal(data, xb, betas, goal, K, N, groups=groups, joint_sweeps=S, **kw, **more)
    # one person walks from the origin to (0.5, 3); the second starts there, turned round, and walks back past the first
    one = lambda a: a[:, :1].contiguous() if a.dim() == 3 else a[:1].contiguous()
    z1 = torch.randn(K, N, 128, generator=g).cuda()
    first = op.generate_sequence_to_goal(one(data), one(xb), one(betas), torch.tensor([0.5, 3.0, 0.9]), K, N, z=z1, to_numpy=False)
    people = MovingObstacles.from_sequences(first)
    turn = torch.tensor([[[-1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [0.0, 0.0, 1.0]]])
    avoid = lambda **more: op.generate_sequence_to_goal(one(data), one(xb), one(betas), torch.tensor([-1.0, 0.0, 0.9]), K, N, z=z1, to_numpy=False,
                                                         R0=turn, T0=torch.tensor([[0.5, 3.0, 0.0]]), obstacles=people, **more)
    return op, swap, avoid


def cost(args):
    from bench_genop import alternate
    from bench_genop_joint import joint_launches, table
    from bench_genop_search import captured
    lib = _lib.load()
    op, swap, avoid = worlds(args)
    vp = lambda t: C.c_void_p(t.data_ptr())
    st = _lib.current_stream_ptr()
    loops, launches = {}, {}
    for H in (0,) + AHEAD:
        loop, sf = captured(op, "_search_loop", lambda: swap(lookahead=H))
        loops[f"groups: loop, H={H}"] = loop
        launches["groups: egx_primitive_select_joint" if H == 0 else f"groups: egx_primitive_select_joint_ahead, H={H}"] = \
            joint_launches(op, lib, sf[3], K - 1, G * P, N)["joint"]
        if H == 0:      # the selection of the same rows
            s, k = sf[3], K - 1
            cur, lbs = s["xs"][k % 2], s["lbs_out"]
            lead = (_lib.ptr(s["Y_gen"]), vp(cur[0]), vp(cur[1]), 201, _lib.ptr(lbs["joints"]), 127, _lib.ptr(lbs["markers"]), _lib.ptr(s["R0"]),
                    _lib.ptr(s["T0"]), None, _lib.ptr(s["goal"]), _lib.ptr(s["feet"]), s["weights"], s["pene_thres"], s["goal_thresh"], s["rf"], G * P, N,
                    vp(s["choice"][k]), vp(s["status"][k]), vp(s["reached"][k]), vp(s["goal_dist"][k]), vp(s["cost"][k]), vp(s["cost_terms"][k]),
                    vp(s["colliding"][k]), st)
            launches["groups: egx_primitive_select"] = lambda lead=lead: _lib.check(lib.egx_primitive_select(*lead), "egx_primitive_select")
    for H in (0,) + AHEAD:
        loop, sf = captured(op, "_search_loop", lambda: avoid(lookahead=H))
        loops[f"avoid: loop, H={H}"] = loop
        s, k = sf[3], K - 1
        sel = op._select_lead(s, [s["R0"]] * 2, [s["T0"]] * 2)[k % 2]
        name, field, obs = op._select_tail(s, K, "egx_primitive_select")
        outs = (vp(s["choice"][k]), vp(s["status"][k]), vp(s["reached"][k]), vp(s["goal_dist"][k]), vp(s["cost"][k]), vp(s["cost_terms"][k]),
                vp(s["colliding"][k]))
        launches[f"avoid: {name}" + (f", table of H={H}" if H else "")] = \
            lambda name=name, a=(*sel, 1, N, *outs, *field, *obs[k], st): _lib.check(getattr(lib, name)(*a), name)
        if H:
            cname, clear = op._clearance_lead(s, K, 1, N, [s["R0"]] * 2, [s["T0"]] * 2, st)
            launches[f"avoid: {cname}, H={H}"] = lambda cname=cname, a=clear[k]: _lib.check(getattr(lib, cname)(*a), cname)
    t = per_primitive(alternate(loops, args.iters, args.warmup))
    t.update(alternate(launches, 10 * args.iters, args.warmup))
    lines = [f"Device: {torch.cuda.get_device_name(0)}; K = {K} primitives, body of {args.num_verts} vertices, no scene; groups: {G} variants of {P} "
             f"people, N = {N}, S = {S} sweeps (b = {G * P}); avoid: one person, N = {N}, one recorded person.  One process, {args.iters} loop passes "
             f"or {10 * args.iters} launches per window, three windows per leg after {args.warmup} warm-up passes, the legs taking turns; device "
             "events.  Microseconds: median (range of the windows); loops per primitive.", ""]
    lines += table(argparse.Namespace(save=None, parent=None), [("", leg, v) for leg, v in t.items()])
    write_section(args.out_dir, "cost", lines)
    print("\n".join(lines))


def parent(args):
    from bench_genop import alternate
    from bench_genop_joint import table
    from bench_genop_search import captured
    op, swap, avoid = worlds(args)
    loops = {"groups: loop, lookahead=0": captured(op, "_search_loop", lambda: swap())[0],
             "avoid: loop, lookahead=0": captured(op, "_search_loop", lambda: avoid())[0]}
    t = per_primitive(alternate(loops, args.iters, args.warmup))
    lines = [f"Device: {torch.cuda.get_device_name(0)}; the shapes of the cost section; per primitive, microseconds: median (range of three "
             f"windows of {args.iters} loop passes); the parent commit's library and this one, one process each, the parent's first.", ""]
    lines += table(args, [("", leg, v) for leg, v in t.items()])
    if args.parent:
        write_section(args.out_dir, "parent", lines)
    print("\n".join(lines))


def effect(args):
    import sweep_search_quality as sq
    from egogen_amd import MovingObstacles, metrics
    rows = []
    sq.VARIANTS = G
    op, data, bparams, betas, goal, R0, T0, variant = sq.setup(args.num_verts, 0)
    for H in (0, 2):
        r = sq.measure(op, data, bparams, betas, goal, R0, T0, variant, N, 0, groups=variant, lookahead=H)
        rows.append(("four-people swap, groups", H, r))
    # the two-person example: the same operator, person 1 alone, then person 2 from person 1's goal against its record
    keep = sq.PEOPLE, sq.VARIANTS
    try:
        sq.VARIANTS, sq.PEOPLE = 1, "0,0,0:0.5,3,0.9"
        _, d1, b1, bt, g1, R1, T1, _ = sq.setup(args.num_verts, 0)
        sq.PEOPLE = "0.5,3,180:-1,0,0.9"
        _, d2, b2, _, g2, R2, T2, _ = sq.setup(args.num_verts, 0)
    finally:
        sq.PEOPLE, sq.VARIANTS = keep
    torch.manual_seed(0)
    first = op.generate_sequence_to_goal(d1, b1, bt, g1, sq.K, N, R0=R1, T0=T1)
    people = MovingObstacles.from_sequences(first)
    for H in (0, 2):
        torch.manual_seed(1)
        res = op.generate_sequence_to_goal(d2, b2, bt, g2, sq.K, N, R0=R2, T0=T2, obstacles=people, lookahead=H)
        ms = metrics.MotionSet.from_sequences([first, res])
        per, crowd = metrics.motion_metrics(ms, goal_thresh=0.1), metrics.crowd_metrics(ms, groups=np.zeros(2, np.int64), hold=True)
        r = {"reached": float((per["first_reached_frame"] >= 0).mean()), "clearance_min": float(crowd["group"]["clearance_min"].min()),
             "marker_dist_min": float(crowd["group"]["marker_dist_min"].min()), "overlap": int(crowd["group"]["overlap_frames"].sum()),
             "touch": int(crowd["group"]["touch_frames"].sum()), "compared": int(crowd["group"]["frames_compared"].sum()),
             "search_hits": int(np.asarray(res.status & 1).sum())}
        r.update({k: float(np.mean(per[k])) for k in sq.PER_MOTION})
        rows.append(("two people, --avoid", H, r))
    cols = ("overlap", "clearance_min", "touch", "marker_dist_min", "compared", "reached", "search_hits") + tuple(sq.PER_MOTION)
    fmt = lambda v: "" if v is None else (str(v) if isinstance(v, int) else f"{v:.3f}")
    lines = [f"Device: {torch.cuda.get_device_name(0)}; the seeded random-init prior and synthetic body of scripts/sweep_search_quality.py, "
             f"{sq.K} primitives, N = {N}, lookahead_slack 0.1; `crowd_metrics` with body_radius 0.3, touch_dist 0.05, hold on; per-motion columns "
             "are means over the files of an arm; `overlap` / `touch` are frames on which some pair's cylinders overlap / markers are closer than "
             "touch_dist; `search_hits` the chosen rows the search itself calls colliding.", "",
             "| case | lookahead | " + " | ".join(cols) + " |", "|---|---|" + "---|" * len(cols)]
    lines += [f"| {case} | {H} | " + " | ".join(fmt(r.get(c)) for c in cols) + " |" for case, H, r in rows]
    write_section(args.out_dir, "effect", lines)
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--lib", default=None, help="run on this build of libegogen_hip.so instead of the package's")
    ap.add_argument("--save", default=None, help="keep the lookahead=0 table as JSON (on the parent build, with --lib)")
    ap.add_argument("--parent", default=None, help="a table kept by --save on the parent build: both builds side by side")
    ap.add_argument("--effect", action="store_true", help="crowd_metrics at H = 0 against H = 2: the effect section")
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--num-verts", type=int, default=None)
    args = ap.parse_args()
    if args.num_verts is None:
        from egogen_amd import synth
        args.num_verts = synth.NUM_VERTS
    if args.lib:
        use_library(args.lib)
    if not torch.cuda.is_available():
        sys.exit("bench_genop_lookahead.py measures on the GPU; no device is visible")
    if args.effect:
        effect(args)
    elif args.save or args.parent:
        parent(args)
    else:
        cost(args)


if __name__ == "__main__":
    main()
