#!/usr/bin/env python3
"""The beam search of `GAMMAPrimitiveComboGenOP.generate_sequence_to_goal` (beam_width W > 1) at b x W x N = 64 x 4 x 4 and
64 x 8 x 2 = 1024 rows, K = 10 primitives, no scene, against the greedy loop at the same 1 024 rows (64 x 16) - of ANOTHER tree
where one is given: the yardstick is the parent commit's loop, never the code under test.  GPU only.

    python scripts/bench_genop_beam.py --yardstick-tree <checkout of the parent commit, library built> [--out-dir profiles] [--illustrate]
    python scripts/bench_genop_beam.py --window greedy|WxN --tree <tree>        (one window of one leg; what the driver starts)

Every window is a process of its own that imports `egogen_amd` from its tree: device events around --iters passes of the captured
primitive loop after --warmup of them.  The driver starts the windows one after the other, legs alternating, three windows per leg,
and reports median and range (min .. max) per primitive.  Without --yardstick-tree the greedy leg runs this tree's loop and is
labelled so.  In the driver's own process then: launches per primitive (kernel records of one profiled loop divided by K; the
backtrack is counted per call), the three beam launches alone on the loop's own buffers (device events), and with --illustrate the
final goal distance / reached / colliding path nodes at an equal row budget W x N in {1x16, 2x8, 4x4, 8x2} in the box scene with the
seeded random-weight prior: an illustration of the mechanism, NOT a statement about motion quality.  Writes
`<out-dir>/genop_beam.json` and replaces the section between the `timings` markers of `<out-dir>/genop_beam.md`."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BEGIN, END = "<!-- timings:begin -->", "<!-- timings:end -->"
BEAMS = ((4, 4), (8, 2))


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--seqs", type=int, default=64)
    ap.add_argument("--rows-per-seq", type=int, default=16)
    ap.add_argument("--primitives", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--num-verts", type=int, default=None)
    ap.add_argument("--sdf-res", type=int, default=256)
    ap.add_argument("--yardstick-tree", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--illustrate", action="store_true")
    ap.add_argument("--window", default=None, help="greedy or WxN: time one window of that leg and print one JSON line")
    ap.add_argument("--tree", default=ROOT, help="with --window: the tree whose egogen_amd is imported")
    return ap.parse_args()


def setup(tree, args):
    """import the package of `tree`, build the operator and the 64 seeds of scripts/bench_genop_search.py"""
    sys.path.insert(0, os.path.join(tree, "scripts"))
    sys.path.insert(0, tree)
    import torch
    from bench_genop_search import build_op, captured, launches_of, seeds
    from egogen_amd import synth
    V = synth.NUM_VERTS if args.num_verts is None else args.num_verts
    b, R, K = args.seqs, args.rows_per_seq, args.primitives
    op, body = build_op(V)
    g = torch.Generator().manual_seed(1)
    data_r, xb_r, betas_r = seeds(body, b * R, g)
    data_b, xb_b, betas_b = data_r[:, ::R].contiguous(), xb_r[:, ::R].contiguous(), betas_r[::R].contiguous()
    z = torch.randn(K, b * R, 128, generator=g).cuda()
    goal = torch.tensor([0.5, 3.0, 0.9])
    T0 = torch.zeros(b, 3)
    T0[:, 0] = torch.linspace(-1.0, 2.5, b)
    T0[:, 1] = -1.5
    return {"op": op, "body": body, "seed": (data_b, xb_b, betas_b), "z": z, "goal": goal, "T0": T0, "V": V, "captured": captured,
            "launches_of": launches_of}


def loop_of(w, leg, K, R, **kw):
    """the captured primitive loop of a leg: 'greedy' (N = R) or (W, N)"""
    op = w["op"]
    if leg == "greedy":
        return w["captured"](op, "_search_loop", lambda: op.generate_sequence_to_goal(*w["seed"], w["goal"], K, R, z=w["z"], T0=w["T0"],
                                                                                     to_numpy=False, **kw))
    W, N = leg
    return w["captured"](op, "_beam_loop", lambda: op.generate_sequence_to_goal(*w["seed"], w["goal"], K, N, z=w["z"], T0=w["T0"],
                                                                                   to_numpy=False, beam_width=W, **kw))


def window(args):
    import torch
    w = setup(os.path.abspath(args.tree), args)
    leg = "greedy" if args.window == "greedy" else tuple(int(v) for v in args.window.split("x"))
    loop, _ = loop_of(w, leg, args.primitives, args.rows_per_seq)
    for _ in range(args.warmup):
        loop()
    torch.cuda.synchronize()
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.iters):
        loop()
    e.record()
    torch.cuda.synchronize()
    print("WINDOW " + json.dumps({"leg": args.window, "tree": os.path.abspath(args.tree),
                                  "us_per_primitive": a.elapsed_time(e) / args.iters / args.primitives * 1e3}), flush=True)


def main():
    args = parse()
    if args.window:
        return window(args)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_genop_beam.py measures on the GPU; no device is visible")
    b, R, K = args.seqs, args.rows_per_seq, args.primitives
    ytree = os.path.abspath(args.yardstick_tree) if args.yardstick_tree else ROOT
    legs = [("greedy", ytree)] + [(f"{W}x{N}", ROOT) for W, N in BEAMS]
    times = {k: [] for k, _ in legs}
    common = ["--seqs", str(b), "--rows-per-seq", str(R), "--primitives", str(K), "--iters", str(args.iters), "--warmup", str(args.warmup),
              "--sdf-res", str(args.sdf_res)] + (["--num-verts", str(args.num_verts)] if args.num_verts else [])
    for _ in range(3):                      # one process per window, one after the other, legs alternating
        for leg, tree in legs:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--window", leg, "--tree", tree] + common, capture_output=True,
                               text=True, timeout=600)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("WINDOW ")]
            if r.returncode != 0 or not line:
                sys.exit(f"window {leg} of {tree} failed ({r.returncode}):\n{r.stdout[-1500:]}\n{r.stderr[-1500:]}")
            times[leg].append(json.loads(line[-1][len("WINDOW "):])["us_per_primitive"])
            print(leg, tree, times[leg][-1], flush=True)
    stat = lambda v: {"median_us": float(np.median(v)), "min_us": float(min(v)), "max_us": float(max(v))}
    per = {k: stat(v) for k, v in times.items()}

    # ---- this process: launches per primitive and the three beam launches alone
    w = setup(ROOT, args)
    from bench_genop import alternate
    from egogen_amd import _lib
    from egogen_amd.body_model import SdfScene
    from egogen_amd import synth
    lib = _lib.load()
    results = {"seqs": b, "rows_per_seq": R, "primitives": K, "iters": args.iters, "warmup": args.warmup, "num_verts": w["V"],
               "device": torch.cuda.get_device_name(0), "yardstick_tree": "the parent commit's" if args.yardstick_tree else "THIS tree's (no yardstick)",
               "per_primitive_us": per, "against_yardstick": {k: per[k]["median_us"] / per["greedy"]["median_us"] - 1.0 for k in per if k != "greedy"}}
    launches, alone = {}, {}
    greedy_loop, _ = loop_of(w, "greedy", K, R)
    launches["greedy (this tree)"] = w["launches_of"](greedy_loop, K)
    for W, N in BEAMS:
        loop, a = loop_of(w, (W, N), K, R)
        n = w["launches_of"](loop, K)
        launches[f"{W}x{N}"] = None if n is None else (n * K - 1) / K          # the backtrack is one launch per call, not per primitive
        s = a[4]
        st = _lib.current_stream_ptr()
        k = K - 1
        cur, nxt = s["xs"][k % 2], s["xs"][(k + 1) % 2]
        R0, T0, R0n, T0n = s["R0s"][k % 2], s["T0s"][k % 2], s["R0s"][(k + 1) % 2], s["T0s"][(k + 1) % 2]
        lbs = s["lbs_out"]
        vp = lambda t: C.c_void_p(t.data_ptr())
        p = _lib.ptr

        def select():
            _lib.check(lib.egx_primitive_beam_select(
                p(s["Y_gen"]), vp(cur[0]), vp(cur[1]), 201, p(lbs["joints"]), 127, p(lbs["markers"]), p(R0), p(T0), None, p(s["goal"]),
                p(s["feet"]), s["weights"], s["pene_thres"], s["goal_thresh"], s["rf"], b, W, N, vp(s["acc"][k]), vp(s["ncoll"][k]),
                vp(s["cost"][k]), vp(s["cost_terms"][k]), vp(s["colliding"][k]), vp(s["beam_row"][k]), vp(s["parent"][k]), vp(s["acc"][k + 1]),
                vp(s["ncoll"][k + 1]), vp(s["path_cost"][k]), vp(s["beam_status"][k]), vp(s["slot_goal_dist"][k]), vp(s["slot_reached"][k]), st),
                "egx_primitive_beam_select")

        def hand_off():
            _lib.check(lib.egx_primitive_advance_beam(
                p(s["pp"]), p(s["Y_gen"]), vp(cur[0]), vp(cur[1]), 201, p(lbs["joints"]), 127, p(lbs["markers"]), p(s["delta_T"]), s["rf"], b, W,
                N, vp(s["beam_row"][k]), p(R0), p(T0), p(R0n), p(T0n), vp(s["rec_markers"][k]), vp(s["rec_pelvis"][k]), vp(s["rec_rotmat"][k]),
                vp(s["rec_transl"][k]), vp(s["rec_params"][k]), p(s["seed"]), vp(nxt[0]), vp(nxt[1]), 201, vp(s["beam_status"][k]), st),
                "egx_primitive_advance_beam")

        def backtrack():
            _lib.check(lib.egx_beam_backtrack(
                p(s["parent"]), p(s["beam_row"]), p(s["beam_status"]), p(s["slot_goal_dist"]), p(s["slot_reached"]), p(s["rec_markers"]),
                p(s["rec_pelvis"]), p(s["rec_rotmat"]), p(s["rec_transl"]), p(s["rec_params"]), K, b, W, p(s["path_slot"]), p(s["choice"]),
                p(s["status"]), p(s["goal_dist"]), p(s["reached"]), p(s["markers"]), p(s["pelvis"]), p(s["rotmat"]), p(s["transl"]),
                p(s["params"]), st), "egx_beam_backtrack")
        alone[f"{W}x{N}"] = alternate({"select": select, "hand_off": hand_off, "backtrack": backtrack}, args.iters, args.warmup)
    results.update(launches_per_primitive=launches, launches_alone_us=alone)
    if args.illustrate:
        scene = SdfScene(synth.make_sdf_scene(args.sdf_res))
        ill = {}
        for W, N in ((1, 16), (2, 8), (4, 4), (8, 2)):
            r = w["op"].generate_sequence_to_goal(*w["seed"], w["goal"], K, N, T0=w["T0"], scene=scene, beam_width=W)
            last = r.goal_dist[np.asarray(r.n_valid) - 1, np.arange(b)]
            ill[f"{W}x{N}"] = {"mean_final_goal_dist_m": float(last.mean()), "reached": int((np.asarray(r.n_valid) < K).sum()),
                               "colliding_path_nodes": int((r.status & 1).sum()), "path_nodes": int(r.status.size)}
        results["illustration_random_weight_prior"] = ill
    print(json.dumps(results, indent=1), flush=True)

    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "genop_beam.json"), "w") as fh:
        json.dump(results, fh, indent=1)
    fmt = lambda v: f"{v['median_us']:.1f} ({v['min_us']:.1f} .. {v['max_us']:.1f})"
    fl = lambda v: "n/a" if v is None else f"{v:.1f}"
    lines = [BEGIN, f"Device: {results['device']}; {b} sequences x {R} rows = {b * R} rows, K = {K}, body of {w['V']} vertices, no scene; "
             f"{args.iters} passes per window, one process per window, three windows per leg, legs alternating.  Microseconds: median "
             f"(min .. max).  Greedy leg: {results['yardstick_tree']} loop.", "",
             "| leg | us per primitive | against the greedy leg | launches per primitive (this tree) |", "|---|---|---|---|",
             f"| greedy {b} x {R} | {fmt(per['greedy'])} | | {fl(launches['greedy (this tree)'])} |"]
    for W, N in BEAMS:
        k = f"{W}x{N}"
        lines.append(f"| beam {b} x {W} x {N} | {fmt(per[k])} | {100 * results['against_yardstick'][k]:+.1f} % | {fl(launches[k])} + 1 backtrack per call |")
    lines += ["", "| launch alone (device events, the loop's own buffers) | " + " | ".join(f"{W} x {N}, us" for W, N in BEAMS) + " |",
              "|---|" + "---|" * len(BEAMS)]
    for what, name in (("select", "egx_primitive_beam_select"), ("hand_off", "egx_primitive_advance_beam"), ("backtrack", "egx_beam_backtrack (per call)")):
        lines.append(f"| {name} | " + " | ".join(fmt(alone[f"{W}x{N}"][what]) for W, N in BEAMS) + " |")
    if args.illustrate:
        lines += ["", "Illustration only, seeded random-weight prior (no statement about motion quality): goal 3 m ahead, box scene, "
                  f"b = {b}, K = {K}, default weights, equal row budget W x N = {R}.", "",
                  "| W x N | mean final goal distance (m) | sequences that reached the goal | colliding path nodes |", "|---|---|---|---|"]
        for k, v in results["illustration_random_weight_prior"].items():
            lines.append(f"| {k.replace('x', ' x ')} | {v['mean_final_goal_dist_m']:.3f} | {v['reached']} of {b} | {v['colliding_path_nodes']} of {v['path_nodes']} |")
    lines.append(END)
    md = os.path.join(args.out_dir, "genop_beam.md")
    txt = open(md).read() if os.path.exists(md) else "# Beam search over motion primitives\n\n" + BEGIN + "\n" + END + "\n"
    if BEGIN in txt and END in txt:
        txt = txt[:txt.index(BEGIN)] + "\n".join(lines) + txt[txt.index(END) + len(END):]
    else:
        txt += "\n" + "\n".join(lines) + "\n"
    with open(md, "w") as fh:
        fh.write(txt)


if __name__ == "__main__":
    main()
