#!/usr/bin/env python3
"""Waypoint routes in the primitive search (`generate_sequence_to_goal(route=)`, entry egx_route_advance): what the one extra launch
per primitive costs.  GPU only for the measurement; the report needs no device.

    python scripts/bench_genop_route.py --save new_1.json                         (this build)
    python scripts/bench_genop_route.py --lib <parent .so> --save parent_1.json   (the parent commit's build of libegogen_hip.so)
    ... the two taking turns, one process each, on one box ...
    python scripts/bench_genop_route.py --report --parent-runs parent_1.json,parent_2.json --new-runs new_1.json,new_2.json

The shape is the README's four-people example: 4 variants of 4 people who swap places on a circle of 2 m (b = 16, one group per
variant, the cylinder pair model), N = 16 candidates, K = 10 primitives, the full synthetic body, no scene.  With `route=` everybody
walks three waypoints: to the side of the circle's centre, across, then the place opposite (the `goal=` of the other leg).  Device
events around --iters passes of the whole primitive loop on its captured buffers, three windows per leg after --warmup, the legs of a
process taking turns; a process on the parent build has the `goal=` leg only (the build has no route entry), one on this build the
`goal=` leg, the `route=` leg and --iters x 10 single launches of egx_route_advance.  A repeated route loop starts from the cursors
its last pass left; the launch's work does not depend on them.  `--save` also keeps the `route_metrics` of the route run.
`--report` writes the section between the markers of `<out-dir>/genop_route.md`."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from egogen_amd import _lib  # noqa: E402

MARKS = ("<!-- cost:begin -->", "<!-- cost:end -->")
NEW = ("egx_route_advance", "egx_route_metrics")
G, P, N, K = 4, 4, 16, 10
LEG = np.array([[1.0, 1.0], [-1.0, 1.0], [-2.0, 0.0]])          # the waypoints of the person who starts at (2, 0)


def use_library(path):
    """every later `_lib.load()` opens `path`; a build from before routes simply lacks their symbols"""
    _lib.LIB_PATH = os.path.abspath(path)
    probe = C.CDLL(_lib.LIB_PATH)
    have = all(hasattr(probe, name) for name in NEW)
    if not have:
        for name in NEW:
            _lib.SIGNATURES.pop(name, None)
    return have


def people(body, g):
    """-> (data, xb, betas, goal [b,3], the keywords z / T0 / R0 / groups, the routes: b lists of three waypoints)"""
    from bench_genop_search import seeds
    b = G * P
    data, xb, betas = seeds(body, b, g)
    z = torch.randn(K, b * N, 128, generator=g).cuda()
    ang = 2 * np.pi * (np.arange(b) % P) / P
    T0 = torch.tensor(np.stack([2.0 * np.cos(ang), 2.0 * np.sin(ang), np.zeros(b)], -1), dtype=torch.float32)
    yaw = ang + np.pi / 2                                         # the seed walks along +y: turned to face the centre
    R0 = torch.tensor(np.stack([np.stack([np.cos(yaw), -np.sin(yaw), 0 * yaw], -1), np.stack([np.sin(yaw), np.cos(yaw), 0 * yaw], -1),
                                np.stack([0 * yaw, 0 * yaw, 1 + 0 * yaw], -1)], 1), dtype=torch.float32)
    goal = -T0 + torch.tensor([0.0, 0.0, 0.9])
    rot = np.stack([np.stack([np.cos(ang), -np.sin(ang)], -1), np.stack([np.sin(ang), np.cos(ang)], -1)], 1)          # [b,2,2]
    ways = np.concatenate([np.einsum("bij,wj->bwi", rot, LEG), np.full((b, 3, 1), 0.9)], -1).astype(np.float32)
    ways[:, -1] = goal.numpy()                                    # the last waypoint is the other leg's goal, bit for bit
    return data, xb, betas, goal, dict(z=z, T0=T0, R0=R0, to_numpy=False, groups=np.arange(b) // P), [w for w in ways]


def measure(args):
    from bench_genop import alternate
    from bench_genop_search import build_op, captured
    have = use_library(args.lib) if args.lib else True
    lib = _lib.load()
    op, body = build_op(args.num_verts)
    data, xb, betas, goal, kw, ways = people(body, torch.Generator().manual_seed(1))
    legs, out = {}, {"device": torch.cuda.get_device_name(0), "lib": args.lib or "this build", "iters": args.iters, "warmup": args.warmup,
                     "num_verts": args.num_verts, "shape": f"G={G} P={P} N={N} K={K} (b={G * P})"}
    legs["loop, goal="], _ = captured(op, "_search_loop", lambda: op.generate_sequence_to_goal(data, xb, betas, goal, K, N, **kw))
    if have:
        from egogen_amd import metrics
        from egogen_amd.route import Routes
        route, res = Routes.from_lists(ways, pass_radius=args.pass_radius), {}
        legs["loop, route="], sf = captured(op, "_search_loop",
                                            lambda: res.update(r=op.generate_sequence_to_goal(data, xb, betas, None, K, N, route=route, **kw)))
        r = res["r"]
        rm = metrics.route_metrics(metrics.MotionSet.from_sequences(r), pass_radius=route.pass_radius)
        near = rm["approach_min"][:, :3]
        out["route_metrics"] = {"pass_radius": route.pass_radius, "waypoints_passed": rm["waypoints_passed"].tolist(),
                                "cursor_after_last_primitive": r.route_cursor[-1].tolist(),
                                "approach_min_mean_m": [None if np.isnan(near[:, j]).all() else float(np.nanmean(near[:, j])) for j in range(3)],
                                "approached_of_16": [int((~np.isnan(near[:, j])).sum()) for j in range(3)],
                                "goal_dist_end_mean_m": float(r.goal_dist[-1].mean())}
    t = alternate(legs, args.iters, args.warmup)
    for v in t.values():
        for q in ("median_us", "min_us", "max_us"):
            v[q] /= K                                             # per primitive
    if have:
        s, st, k, vp = sf[3], _lib.current_stream_ptr(), K - 1, lambda x: C.c_void_p(x.data_ptr())
        one = lambda: _lib.check(lib.egx_route_advance(
            vp(s["pelvis"][k]), vp(s["rotmat"][k]), vp(s["transl"][k]), *s["route"], _lib.ptr(s["route_state"]), _lib.ptr(s["goal"]), None,
            vp(s["reached"][k]), vp(s["route_cursor"][k]), vp(s["route_goal"][k]), vp(s["route_pass_dist"][k]), st), "egx_route_advance")
        t.update(alternate({"route launch": one}, 10 * args.iters, args.warmup))
    out["legs"] = t
    with open(args.save, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out, indent=1))


def report(args):
    load = lambda names: [json.load(open(f)) for f in names.split(",") if f]
    parent, new = load(args.parent_runs), load(args.new_runs)
    fmt = lambda runs, leg: ", ".join(f"{r['legs'][leg]['median_us']:.1f} ({r['legs'][leg]['min_us']:.1f} .. {r['legs'][leg]['max_us']:.1f})" for r in runs)
    med = lambda runs, leg: float(np.median([r["legs"][leg]["median_us"] for r in runs]))
    n0 = new[0]
    lines = [f"Device: {n0['device']}; {n0['shape']}, body of {n0['num_verts']} vertices, no scene, the cylinder pair model with S = 2 sweeps; "
             f"{len(parent)} processes on the parent commit's build and {len(new)} on this build, taking turns on one box; per process "
             f"{n0['iters']} loop passes or {10 * n0['iters']} launches per window, three windows per leg after {n0['warmup']} warm-up passes, device "
             "events.  Microseconds per primitive: median (range of the windows), one entry per process.", "",
             "| leg | build | us per primitive |", "|---|---|---|",
             f"| loop, `goal=` | parent | {fmt(parent, 'loop, goal=')} |", f"| loop, `goal=` | this | {fmt(new, 'loop, goal=')} |",
             f"| loop, `route=` (three waypoints each) | this | {fmt(new, 'loop, route=')} |",
             f"| one egx_route_advance launch (b = 16) | this | {fmt(new, 'route launch')} |", ""]
    a, b_, c = med(parent, "loop, goal="), med(new, "loop, goal="), med(new, "loop, route=")
    spread = max(abs(r["legs"]["loop, goal="]["median_us"] / a - 1.0) for r in parent)
    lines += [f"`route=` on this build against `goal=` on the parent build: {c:.1f} against {a:.1f} us per primitive, {c - a:+.1f} us "
              f"({100 * (c / a - 1):+.2f} %); `goal=` on this build against the parent build: {b_:.1f} against {a:.1f} us ({100 * (b_ / a - 1):+.2f} %).  "
              f"The parent build's own processes differ from their median by up to {100 * spread:.2f} %.", ""]
    rm = n0["route_metrics"]
    lines += [f"`route_metrics` of the route run (pass_radius {rm['pass_radius']} m, 16 people, 3 waypoints each, the last one the goal): "
              f"waypoints passed per person {rm['waypoints_passed']}; the search's cursor after the last primitive {rm['cursor_after_last_primitive']}; "
              f"mean least approach to waypoint 1 / 2 / 3 over the people who got to look for it (m): "
              f"{' / '.join('-' if v is None else f'{v:.2f}' for v in rm['approach_min_mean_m'])} ({rm['approached_of_16']} of 16 people); mean "
              f"distance to the scored waypoint after the last primitive {rm['goal_dist_end_mean_m']:.2f} m.  **This is a random-init prior: the "
              "figures show the mechanism, not motion quality.**"]
    md = os.path.join(args.out_dir, "genop_route.md")
    txt = open(md).read() if os.path.exists(md) else "# Waypoint routes in the primitive search\n"
    body = "\n".join([MARKS[0]] + lines + [MARKS[1]])
    if MARKS[0] in txt and MARKS[1] in txt:
        txt = txt[:txt.index(MARKS[0])] + body + txt[txt.index(MARKS[1]) + len(MARKS[1]):]
    else:
        txt += "\n" + body + "\n"
    with open(md, "w") as fh:
        fh.write(txt)
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--lib", default=None, help="run on this build of libegogen_hip.so instead of the package's")
    ap.add_argument("--save", default=None, help="measure and keep the figures as JSON")
    ap.add_argument("--report", action="store_true", help="write the section of genop_route.md from kept figures (no device needed)")
    ap.add_argument("--parent-runs", default="", help="comma-separated JSON files kept on the parent build")
    ap.add_argument("--new-runs", default="", help="comma-separated JSON files kept on this build")
    ap.add_argument("--pass-radius", type=float, default=0.5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--num-verts", type=int, default=None)
    args = ap.parse_args()
    if args.report:
        if not args.parent_runs or not args.new_runs:
            sys.exit("--report needs --parent-runs and --new-runs")
        return report(args)
    if not args.save:
        sys.exit("give --save FILE to measure, or --report")
    if args.num_verts is None:
        from egogen_amd import synth
        args.num_verts = synth.NUM_VERTS
    if not torch.cuda.is_available():
        sys.exit("bench_genop_route.py measures on the GPU; no device is visible")
    measure(args)


if __name__ == "__main__":
    main()
