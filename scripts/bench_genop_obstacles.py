#!/usr/bin/env python3
"""The obstacle phase of the selection kernels (egx_primitive_select_obstacles, `generate_sequence_to_goal(obstacles=)`): what it
costs, and that the entries without obstacles did not move.  GPU only.

    python scripts/bench_genop_obstacles.py --parent-lib <libegogen_hip.so of the parent commit> [--rounds 3] [--out-dir profiles]
    python scripts/bench_genop_obstacles.py --lib <parent .so> --dump outputs.pt        (once, on the parent build)
    python scripts/bench_genop_obstacles.py --compare outputs.pt [--out-dir profiles]   (once, on this build)

Timing: at the driver's shape (b = 4, N = 16) and at M = 256 rows per sequence (b = 4, N = 256), the select launch alone and one
primitive of the whole search loop (K = 4, body of --num-verts vertices, no scene), without obstacles and with sets of O = 0, 8 and
32 tracks.  Each round starts two fresh processes in turn, A on the parent commit's library (plain entries only: it has no others)
and B on this build; inside a process the legs alternate, device events around --iters passes of a loop (ten times as many of
a single launch) after --warmup, three windows per leg, median per leg.  The table gives, per leg, the median over the rounds
and the range of the rounds' medians: the run-to-run spread seen.  `--lib` makes any mode run on another build of the library.

Bit identity: `--dump` writes every output of the four selection entries that existed before (egx_primitive_select, _select_field,
_beam_select, _beam_select_field) on the pooled inputs of the tests; `--compare` recomputes them and compares bit for bit.
Writes the sections between the `timings` and the `identity` markers of `<out-dir>/genop_obstacles.md`."""
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

MARKS = {"timings": ("<!-- timings:begin -->", "<!-- timings:end -->"), "identity": ("<!-- identity:begin -->", "<!-- identity:end -->")}
NEW = ("egx_primitive_select_obstacles", "egx_primitive_beam_select_obstacles")
SHAPES = ((4, 16), (4, 256))
K = 4


def use_library(path):
    """every later `_lib.load()` opens `path`; a build from before the obstacle entries simply lacks their two symbols"""
    _lib.LIB_PATH = os.path.abspath(path)
    probe = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        if not hasattr(probe, name):
            _lib.SIGNATURES.pop(name, None)


def write_section(out_dir, which, lines):
    begin, end = MARKS[which]
    md = os.path.join(out_dir, "genop_obstacles.md")
    os.makedirs(out_dir, exist_ok=True)
    txt = open(md).read() if os.path.exists(md) else "# Moving obstacles in the primitive search\n"
    body = "\n".join([begin] + lines + [end])
    if begin in txt and end in txt:
        txt = txt[:txt.index(begin)] + body + txt[txt.index(end) + len(end):]
    else:
        txt += "\n" + body + "\n"
    with open(md, "w") as fh:
        fh.write(txt)


# ---- bit identity of the entries that existed before -----------------------------------------------------------------------
def existing_outputs():
    from egogen_amd import synth
    from egogen_amd.body_model import BodyModelHandle
    from tests import genop_gpu_helpers as gh
    from tests import test_geodesic_gpu as tg
    V = gh.V_SMALL
    world = {"handle": BodyModelHandle(synth.make_body_model(0, num_verts=V), synth.marker_ids(V), synth.feet_vids(V))}
    out = {}
    g = torch.Generator().manual_seed(11)
    for b, N, jpb, pene in ((3, 5, 127, True), (1, 70, 55, True), (65, 5, 127, False), (1, 256, 127, True)):
        x = gh._rows_inputs(world, b, N, 100 + b * 7 + N, pene)
        for k, v in gh._select(x, jpb)[0].items():
            out[f"select b={b} N={N} {k}"] = v
    for b, W, N in ((3, 2, 3), (1, 32, 8), (65, 2, 5)):
        x = gh._rows_inputs(world, b, W * N, 200 + b * 7 + W * N, True)
        acc, ncoll = torch.rand(b, W, generator=g) * 2.0, torch.randint(0, 3, (b, W), generator=g).int()
        for k, v in gh._beam_select(x, W, N, 127, acc, ncoll)[0].items():
            out[f"beam_select b={b} W={W} N={N} {k}"] = v
    for b, N in ((3, 5), (1, 70)):
        x, fld = tg._room_rows(world, b, N, 300 + b * 7 + N)
        for k, v in tg._select_field(x, 127, fld, list(range(b)))[0].items():
            out[f"select_field b={b} N={N} {k}"] = v
    for b, W, N in ((3, 2, 3), (1, 32, 8)):
        x, fld = tg._room_rows(world, b, W * N, 500 + W * N)
        acc, ncoll = torch.rand(b, W, generator=g) * 6.0, torch.randint(0, 3, (b, W), generator=g).int()
        for k, v in tg._select_field(x, 127, fld, list(range(b)), beam=(W, N), acc=acc, ncoll=ncoll)[0].items():
            out[f"beam_select_field b={b} W={W} N={N} {k}"] = v
    return out


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


# ---- timing, one process on one library -----------------------------------------------------------------------------------------
def time_child(args):
    from bench_genop import alternate
    from bench_genop_search import build_op, captured, seeds
    lib = _lib.load()
    have_obstacles = all(n in _lib.SIGNATURES for n in NEW)
    op, body = build_op(args.num_verts)
    g = torch.Generator().manual_seed(1)
    vp = lambda t: C.c_void_p(t.data_ptr())
    out = {}
    for b, N in SHAPES:
        data, xb, betas = seeds(body, b, g)
        z = torch.randn(K, b * N, 128, generator=g).cuda()
        goal = torch.tensor([0.5, 3.0, 0.9])
        T0 = torch.zeros(b, 3)
        T0[:, 0] = torch.linspace(-1.0, 2.5, b)
        kw = dict(z=z, T0=T0, to_numpy=False)
        plain, sf = captured(op, "_search_loop", lambda: op.generate_sequence_to_goal(data, xb, betas, goal, K, N, **kw))
        legs = {"loop plain": plain}
        s, st = sf[3], _lib.current_stream_ptr()
        cur, lbs = s["xs"][(K - 1) % 2], s["lbs_out"]
        lead = (_lib.ptr(s["Y_gen"]), vp(cur[0]), vp(cur[1]), 201, _lib.ptr(lbs["joints"]), 127, _lib.ptr(lbs["markers"]), _lib.ptr(s["R0"]),
                _lib.ptr(s["T0"]), None, _lib.ptr(s["goal"]), _lib.ptr(s["feet"]), s["weights"], s["pene_thres"], s["goal_thresh"], s["rf"], b, N,
                vp(s["choice"][K - 1]), vp(s["status"][K - 1]), vp(s["reached"][K - 1]), vp(s["goal_dist"][K - 1]), vp(s["cost"][K - 1]),
                vp(s["cost_terms"][K - 1]), vp(s["colliding"][K - 1]))
        legs["select plain"] = lambda lead=lead, st=st: _lib.check(lib.egx_primitive_select(*lead, st), "egx_primitive_select")
        if have_obstacles:
            from egogen_amd import MovingObstacles
            from egogen_amd.genop import NULL_FIELD
            keep = []
            for O in (0, 8, 32):            # people who walk across the searchers' way
                t = np.arange(20 + 18 * (K - 1))[None, :, None] * np.array([0.02, 0.0]) + \
                    np.stack([np.linspace(-2.0, 3.0, max(O, 1)), np.linspace(0.5, 2.5, max(O, 1))], -1)[:O, None, :]
                ob = MovingObstacles.from_tracks(t).to("cuda")                      # [O,T,2]
                legs[f"loop O={O}"], so = captured(op, "_search_loop",
                                                   lambda ob=ob: op.generate_sequence_to_goal(data, xb, betas, goal, K, N, obstacles=ob, **kw))
                so = so[3]
                tail = (*so["obstacles"], 18 * (K - 1), *so["obs_scalars"], vp(so["obstacle_term"][K - 1]), vp(so["clearance"][K - 1]),
                        vp(so["obstacle_hit"][K - 1]))
                legs[f"select O={O}"] = lambda lead=lead, tail=tail, st=st: _lib.check(
                    lib.egx_primitive_select_obstacles(*lead, *NULL_FIELD, *tail, st), "egx_primitive_select_obstacles")
                keep.append((ob, so))
        t = alternate({k: v for k, v in legs.items() if k.startswith("loop")}, args.iters, args.warmup)
        t.update(alternate({k: v for k, v in legs.items() if k.startswith("select")}, 10 * args.iters, args.warmup))   # a launch is short
        for k, v in t.items():
            out[f"b={b} N={N} {k}"] = v["median_us"] / (K if k.startswith("loop") else 1)
    print("RESULT " + json.dumps({"device": torch.cuda.get_device_name(0), "legs": out}), flush=True)


def orchestrate(args):
    me = [sys.executable, os.path.abspath(__file__), "--child", "--iters", str(args.iters), "--warmup", str(args.warmup), "--num-verts",
          str(args.num_verts)]
    runs = {"A": [], "B": []}
    device = ""
    for r in range(args.rounds):
        for side, extra in (("A", ["--lib", args.parent_lib]), ("B", ["--lib", args.lib] if args.lib else [])):
            p = subprocess.run(me + extra, capture_output=True, text=True, timeout=900)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                sys.exit(f"round {r} side {side} failed ({p.returncode}):\n{p.stdout[-1500:]}\n{p.stderr[-1500:]}")
            res = json.loads(line[0][7:])
            device = res["device"]
            runs[side].append(res["legs"])
            print(f"round {r} {side}: {json.dumps(res['legs'])}", flush=True)
    stat = lambda side, k: (float(np.median([r[k] for r in runs[side]])), min(r[k] for r in runs[side]), max(r[k] for r in runs[side]))
    fmt = lambda s: f"{s[0]:.1f} ({s[1]:.1f} .. {s[2]:.1f})"
    lines = [f"Device: {device}; K = {K} primitives, body of {args.num_verts} vertices, no scene; {args.rounds} rounds of two fresh processes "
             f"(A: the parent commit's library, B: this build), {args.iters} loop passes or {10 * args.iters} launches per window, three windows "
             "per leg inside a process.  "
             "Microseconds: median over the rounds (range of the rounds' medians = the run-to-run spread seen); loops per primitive.", "",
             "| leg | A: parent build | B: this build | B - A | larger spread of the two | beyond the spread |", "|---|---|---|---|---|---|"]
    moved = []
    for k in runs["A"][0]:
        a, b = stat("A", k), stat("B", k)
        spread = max(a[2] - a[1], b[2] - b[1])
        beyond = abs(b[0] - a[0]) > spread
        moved += [k] if beyond else []
        lines.append(f"| {k} | {fmt(a)} | {fmt(b)} | {b[0] - a[0]:+.1f} | {spread:.1f} | {'yes' if beyond else 'no'} |")
    lines += ["", "The plain entries against the parent build: " + ("none moved beyond the run-to-run spread." if not moved else
                                                                     "moved beyond the run-to-run spread: " + ", ".join(moved) + "."), "",
              "| leg (this build only) | us | against the plain leg |", "|---|---|---|"]
    for k in runs["B"][0]:
        if k not in runs["A"][0]:
            base = k[:k.rindex(" O=")].rsplit(" ", 1)[0] + (" loop plain" if " loop " in k else " select plain")
            s = stat("B", k)
            lines.append(f"| {k} | {fmt(s)} | {s[0] - stat('B', base)[0]:+.1f} |")
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
    if args.dump or args.compare or args.child:
        if not torch.cuda.is_available():
            sys.exit("bench_genop_obstacles.py measures on the GPU; no device is visible")
    if args.dump:
        torch.save(existing_outputs(), args.dump)
        print(f"wrote {args.dump}")
    elif args.compare:
        want, got = torch.load(args.compare), existing_outputs()
        differ = sorted(k for k in want if k not in got or not same_bits(want[k], got[k])) + sorted(k for k in got if k not in want)
        lines = [f"{len(want)} outputs of egx_primitive_select, egx_primitive_select_field, egx_primitive_beam_select and "
                 f"egx_primitive_beam_select_field on the pooled test inputs, dumped by the parent commit's build and recomputed by this one: "
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
