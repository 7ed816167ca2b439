#!/usr/bin/env python3
"""The marker model of recorded tracks (`generate_sequence_to_goal(obstacles=, obstacle_model="markers")`,
egx_obstacle_marker_clearance and the *_obstacle_markers selection entries): what it costs next to the cylinder model, and that the
entries that existed before did not move.  GPU only.

    python scripts/bench_genop_obstacle_markers.py --parent-lib <libegogen_hip.so of the parent commit> [--rounds 3] [--out-dir profiles]
    python scripts/bench_genop_obstacle_markers.py --lib <parent .so> --dump outputs.pt        (once, on the parent build)
    python scripts/bench_genop_obstacle_markers.py --compare outputs.pt [--out-dir profiles]   (once, on this build)

Timing, method of scripts/bench_genop_obstacles.py (whose helpers this imports): each round starts two fresh processes in turn, A on
the parent commit's library and B on this build; inside a process the legs alternate, device events around windows of launches after
a warm-up, three windows per leg, median per leg; the table gives the median over the rounds and the range of the rounds' medians.
Shapes: the README's `--avoid` example (b = 1, N = 16, one recorded person) and the limit (b = 4, W * N = 256 rows per sequence, 32
recorded people).  Legs: the selection launch without obstacles and with cylinder obstacles (both builds), and on this build the
clearance launch and the selection launch that reads its table.

Bit identity: `--dump` writes every output of the six selection entries that existed before (the four of
scripts/bench_genop_obstacles.py and the two *_obstacles entries on constructed tracks); `--compare` recomputes and compares bit for
bit.  Writes the sections between the `timings` and the `identity` markers of `<out-dir>/genop_obstacle_markers.md`."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from egogen_amd import _lib  # noqa: E402
import bench_genop_obstacles as base  # noqa: E402

MARKS = {"timings": ("<!-- timings:begin -->", "<!-- timings:end -->"), "identity": ("<!-- identity:begin -->", "<!-- identity:end -->")}
NEW = ("egx_obstacle_marker_clearance", "egx_primitive_select_obstacle_markers", "egx_primitive_beam_select_obstacle_markers")
SHAPES = ((1, 16, 1), (4, 256, 32))          # b, rows per sequence, recorded people
K = 4


def use_library(path):
    _lib.LIB_PATH = os.path.abspath(path)
    probe = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        if not hasattr(probe, name):
            _lib.SIGNATURES.pop(name, None)


def write_section(out_dir, which, lines):
    begin, end = MARKS[which]
    md = os.path.join(out_dir, "genop_obstacle_markers.md")
    os.makedirs(out_dir, exist_ok=True)
    txt = open(md).read() if os.path.exists(md) else "# Marker model for recorded tracks\n"
    body = "\n".join([begin] + lines + [end])
    if begin in txt and end in txt:
        txt = txt[:txt.index(begin)] + body + txt[txt.index(end) + len(end):]
    else:
        txt += "\n" + body + "\n"
    with open(md, "w") as fh:
        fh.write(txt)


def existing_outputs():
    """the outputs of scripts/bench_genop_obstacles.py and those of the two *_obstacles entries on the constructed tracks of their tests"""
    from egogen_amd import synth
    from egogen_amd.body_model import BodyModelHandle
    from tests import genop_gpu_helpers as gh
    from tests import test_genop_obstacles_gpu as tg
    out = base.existing_outputs()
    V = gh.V_SMALL
    world = {"handle": BodyModelHandle(synth.make_body_model(0, num_verts=V), synth.marker_ids(V), synth.feet_vids(V))}
    for b, N, O, T, per_group, beam in ((3, 5, 2, 19, True, None), (3, 70, 32, 200, False, None), (3, 6, 6, 40, True, (2, 3)), (1, 256, 32, 40, True, (32, 8))):
        x = tg._lattice(gh._rows_inputs(world, b, N, 400 + b * 7 + N, True), b, N)
        xy = tg._tracks(tg._pelvis64(x, 127, b, N), b, N, O, T, 3, per_group, 0)
        ob = tg._obs(xy, tg.RADIUS, index=list(range(b)) if per_group else None, frame0=3)
        for k, v in tg._select_obs(x, 127, ob, beam=beam)[0].items():
            out[f"{'beam_' if beam else ''}select_obstacles b={b} N={N} O={O} {k}"] = v
    return out


def time_child(args):
    from bench_genop import alternate
    from bench_genop_search import build_op, captured, seeds
    from egogen_amd import MovingObstacles
    from egogen_amd.genop import NULL_FIELD
    lib = _lib.load()
    have_markers = all(n in _lib.SIGNATURES for n in NEW)
    op, body = build_op(args.num_verts)
    g = torch.Generator().manual_seed(1)
    vp = lambda t: C.c_void_p(t.data_ptr())
    out, keep = {}, []
    for b, N, O in SHAPES:
        data, xb, betas = seeds(body, b, g)
        z = torch.randn(K, b * N, 128, generator=g).cuda()
        goal = torch.tensor([0.5, 3.0, 0.9])
        T0 = torch.zeros(b, 3)
        T0[:, 0] = torch.linspace(-1.0, 2.5, b)
        kw = dict(z=z, T0=T0, to_numpy=False)
        T = 20 + 18 * (K - 1)
        track = np.arange(T)[None, :, None] * np.array([0.02, 0.0]) + np.stack([np.linspace(-2.0, 3.0, O), np.linspace(0.5, 2.5, O)], -1)[:, None, :]
        cloud = np.concatenate([track, np.zeros((O, T, 1))], -1)[:, :, None, :] + \
            np.random.default_rng(3).uniform(-0.3, 0.3, size=(1, 1, 67, 3)) * np.array([1.0, 1.0, 3.0]) + np.array([0.0, 0.0, 0.9])
        ob = MovingObstacles.from_tracks(track, markers=cloud if have_markers else None).to("cuda")
        _, so = captured(op, "_search_loop", lambda: op.generate_sequence_to_goal(data, xb, betas, goal, K, N, obstacles=ob, **kw))
        s, st = so[3], _lib.current_stream_ptr()
        cur, lbs = s["xs"][(K - 1) % 2], s["lbs_out"]
        lead = (_lib.ptr(s["Y_gen"]), vp(cur[0]), vp(cur[1]), 201, _lib.ptr(lbs["joints"]), 127, _lib.ptr(lbs["markers"]), _lib.ptr(s["R0"]),
                _lib.ptr(s["T0"]), None, _lib.ptr(s["goal"]), _lib.ptr(s["feet"]), s["weights"], s["pene_thres"], s["goal_thresh"], s["rf"], b, N,
                vp(s["choice"][K - 1]), vp(s["status"][K - 1]), vp(s["reached"][K - 1]), vp(s["goal_dist"][K - 1]), vp(s["cost"][K - 1]),
                vp(s["cost_terms"][K - 1]), vp(s["colliding"][K - 1]))
        outs = (vp(s["obstacle_term"][K - 1]), vp(s["clearance"][K - 1]), vp(s["obstacle_hit"][K - 1]))
        cyl = (*s["obstacles"], 18 * (K - 1), *s["obs_scalars"], *outs)
        legs = {"select plain": lambda lead=lead, st=st: _lib.check(lib.egx_primitive_select(*lead, st), "egx_primitive_select"),
                f"select cylinders O={O}": lambda lead=lead, cyl=cyl, st=st: _lib.check(
                    lib.egx_primitive_select_obstacles(*lead, *NULL_FIELD, *cyl, st), "egx_primitive_select_obstacles")}
        if have_markers:
            table = torch.empty(b * N, 18, device="cuda")
            margs, alive = ob.marker_args(b)
            clear = (_lib.ptr(lbs["markers"]), _lib.ptr(s["Y_gen"]), s["rf"], _lib.ptr(s["R0"]), _lib.ptr(s["T0"]), b, N, *margs, 18 * (K - 1), 0.05,
                     _lib.ptr(table), st)
            tab = (_lib.ptr(table), s["obs_scalars"][0], s["obs_scalars"][1], *outs)
            legs[f"clearance markers O={O}"] = lambda clear=clear: _lib.check(lib.egx_obstacle_marker_clearance(*clear), "egx_obstacle_marker_clearance")
            legs[f"select table O={O}"] = lambda lead=lead, tab=tab, st=st: _lib.check(
                lib.egx_primitive_select_obstacle_markers(*lead, *NULL_FIELD, *tab, st), "egx_primitive_select_obstacle_markers")
            keep.append((table, alive))
        keep.append((ob, so))
        for k, v in alternate(legs, 10 * args.iters, args.warmup).items():
            out[f"b={b} M={N} {k}"] = v["median_us"]
    print("RESULT " + json.dumps({"device": torch.cuda.get_device_name(0), "legs": out}), flush=True)


def orchestrate(args):
    me = [sys.executable, os.path.abspath(__file__), "--child", "--iters", str(args.iters), "--warmup", str(args.warmup), "--num-verts",
          str(args.num_verts)]
    runs = {"A": [], "B": []}
    device = ""
    for r in range(args.rounds):
        for side, extra in (("A", ["--lib", args.parent_lib]), ("B", ["--lib", args.lib] if args.lib else [])):
            p = subprocess.run(me + extra, capture_output=True, text=True, timeout=600)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                sys.exit(f"round {r} side {side} failed ({p.returncode}):\n{p.stdout[-1500:]}\n{p.stderr[-1500:]}")
            res = json.loads(line[0][7:])
            device = res["device"]
            runs[side].append(res["legs"])
            print(f"round {r} {side}: {json.dumps(res['legs'])}", flush=True)
    stat = lambda side, k: (float(np.median([r[k] for r in runs[side]])), min(r[k] for r in runs[side]), max(r[k] for r in runs[side]))
    fmt = lambda s: f"{s[0]:.1f} ({s[1]:.1f} .. {s[2]:.1f})"
    lines = [f"Device: {device}; the rows of primitive {K - 1} of a search of K = {K}, body of {args.num_verts} vertices, no scene; {args.rounds} "
             f"rounds of two fresh processes (A: the parent commit's library, B: this build), {10 * args.iters} launches per window, three "
             "windows per leg inside a process.  Microseconds per launch: median over the rounds (range of the rounds' medians = the "
             "run-to-run spread seen).", "",
             "| leg | A: parent build | B: this build | B - A | larger spread of the two | beyond the spread |", "|---|---|---|---|---|---|"]
    moved = []
    for k in runs["A"][0]:
        a, b = stat("A", k), stat("B", k)
        spread = max(a[2] - a[1], b[2] - b[1])
        beyond = abs(b[0] - a[0]) > spread
        moved += [k] if beyond else []
        lines.append(f"| {k} | {fmt(a)} | {fmt(b)} | {b[0] - a[0]:+.1f} | {spread:.1f} | {'yes' if beyond else 'no'} |")
    lines += ["", "The entries that existed before, against the parent build: " + ("none moved beyond the run-to-run spread." if not moved else
                                                                                   "moved beyond the run-to-run spread: " + ", ".join(moved) + "."), "",
              "| leg (this build only) | us |", "|---|---|"]
    lines += [f"| {k} | {fmt(stat('B', k))} |" for k in runs["B"][0] if k not in runs["A"][0]]
    write_section(args.out_dir, "timings", lines)
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--lib", default=None, help="run on this build of libegogen_hip.so instead of the package's")
    ap.add_argument("--parent-lib", default=None, help="the parent commit's build: side A of the timing")
    ap.add_argument("--dump", default=None)
    ap.add_argument("--compare", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--num-verts", type=int, default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.num_verts is None:
        from egogen_amd import synth
        args.num_verts = synth.NUM_VERTS
    if args.lib and (args.child or args.dump or args.compare):
        use_library(args.lib)
    if (args.dump or args.compare or args.child) and not torch.cuda.is_available():
        sys.exit("bench_genop_obstacle_markers.py measures on the GPU; no device is visible")
    if args.dump:
        torch.save(existing_outputs(), args.dump)
        print(f"wrote {args.dump}")
    elif args.compare:
        want, got = torch.load(args.compare), existing_outputs()
        differ = sorted(k for k in want if k not in got or not base.same_bits(want[k], got[k])) + sorted(k for k in got if k not in want)
        lines = [f"{len(want)} outputs of egx_primitive_select, _select_field, _beam_select, _beam_select_field, _select_obstacles and "
                 "_beam_select_obstacles on the pooled test inputs, dumped by the parent commit's build and recomputed by this one: "
                 + ("every one bit-identical." if not differ else f"{len(differ)} differ: " + "; ".join(differ[:20]) + ".")]
        write_section(args.out_dir, "identity", lines)
        print(lines[0])
        sys.exit(1 if differ else 0)
    elif args.child:
        time_child(args)
    else:
        if not args.parent_lib:
            sys.exit("the timing needs --parent-lib: the parent commit's build of libegogen_hip.so")
        orchestrate(args)


if __name__ == "__main__":
    main()
