#!/usr/bin/env python3
"""The geodesic field and the selection launch that reads it, measured on the GPU.

  * field builds (`egx_geodesic_field` alone: host clock around the entry, which ends in a stream synchronise; seeds and masks
    already on the device): passes and milliseconds for F = 64 fields on the 7.8 m box room at 0.05 m (156 x 156) and F = 8 fields
    on a 20 m floor (400 x 400), each empty and with obstacles (four boxes of `scene_gen.random_box_layout` / a comb of walls);
  * the selection launch on the inputs of scripts/bench_genop_search.py (the buffers its scene-free loop leaves behind) in three
    variants, alternating in one process: `egx_primitive_select` of the parent commit's library (`--parent-lib`, loaded next to this
    one; left out when the file is absent), `egx_primitive_select` of this library, `egx_primitive_select_field` with a field.

    python scripts/bench_geodesic.py [--out-dir profiles] [--parent-lib ab_libs/libegogen_hip_parent.so] [--iters 200]

Writes `<out-dir>/geodesic.json` and replaces the section between the `timings` markers of `<out-dir>/geodesic.md`."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_genop import alternate  # noqa: E402
from bench_genop_search import build_op, captured, seeds  # noqa: E402
from egogen_amd import _lib, geodesic, scene_gen, synth  # noqa: E402

BEGIN, END = "<!-- timings:begin -->", "<!-- timings:end -->"


def box_room(with_boxes):
    cell, origin = 0.05, np.array([-3.9, -3.9])
    free = np.ones((156, 156), bool)
    if with_boxes:                       # the first seeded layout that leaves the selection benchmark's goal (0.5, 3.0) walkable
        for seed in range(3, 40):
            layout = scene_gen.random_box_layout(np.random.default_rng(seed), 4, [-3.9, -3.9], [3.9, 3.9])
            boxed = scene_gen.stamp_boxes(free, origin, cell, layout)
            if len(geodesic.seed_cells(boxed, origin, cell, [0.5, 3.0])[0]) >= 4:
                return boxed, origin, cell
        raise RuntimeError("no layout leaves the goal free")
    return free, origin, cell


def big_floor(with_walls):
    cell, origin = 0.05, np.array([-10.0, -10.0])
    free = np.ones((400, 400), bool)
    if with_walls:                       # a comb: a wall every 2.5 m, open for 2 m at alternating ends
        for n, i in enumerate(range(50, 400, 50)):
            free[i:i + 6] = False
            if n % 2:
                free[i:i + 6, :40] = True
            else:
                free[i:i + 6, -40:] = True
    return free, origin, cell


def goals_on(free, origin, cell, F, rng):
    idx = np.flatnonzero(free.reshape(-1))
    pick = rng.choice(idx, F, replace=False)
    ij = np.stack(np.unravel_index(pick, free.shape), 1)
    return origin + (ij + rng.uniform(0.1, 0.9, (F, 2))) * cell


def time_field(free, origin, cell, goals, repeats=5):
    free8, o, cell, g, si, cells, values = geodesic._checked(free, origin, cell, goals, None)
    S, H, W = free8.shape
    F = len(g)
    lib = _lib.load()
    t = lambda a, dt: torch.as_tensor(a, dtype=dt).cuda().contiguous()
    free_d, cells_d, values_d = t(free8, torch.uint8), t(cells, torch.int32), t(values, torch.float32)
    dist, tmp = torch.empty(F, H, W, device="cuda"), torch.empty(F, H, W, device="cuda")
    flags = torch.zeros(geodesic.BATCH, device="cuda", dtype=torch.int32)
    passes = C.c_int32(0)
    w1, w2 = np.float32(cell), np.float32(np.float64(cell) * np.sqrt(2.0))
    ms = []
    for k in range(repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _lib.check(lib.egx_geodesic_field(_lib.ptr(free_d), None, S, F, H, W, float(w1), float(w2), _lib.ptr(cells_d), _lib.ptr(values_d),
                                          len(cells), _lib.ptr(dist), _lib.ptr(tmp), _lib.ptr(flags), C.byref(passes),
                                          _lib.current_stream_ptr()), "egx_geodesic_field")
        if k:                                                   # the first build loads the code object
            ms.append((time.perf_counter() - t0) * 1e3)
    fin = torch.isfinite(dist)
    return {"F": F, "H": H, "W": W, "free_cells": int(free.sum()), "passes": int(passes.value), "median_ms": float(np.median(ms)),
            "min_ms": float(min(ms)), "max_ms": float(max(ms)), "longest_path_m": float(dist[fin].max()), "reached_cells": int(fin.sum()) // F}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--parent-lib", default=os.path.join(ROOT, "ab_libs", "libegogen_hip_parent.so"))
    ap.add_argument("--seqs", type=int, default=64)
    ap.add_argument("--candidates", type=int, default=16)
    ap.add_argument("--primitives", type=int, default=10)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--num-verts", type=int, default=synth.NUM_VERTS)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_geodesic.py measures on the GPU; no device is visible")
    results = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "warmup": args.warmup}

    rng = np.random.default_rng(7)
    builds = {}
    for name, (free, origin, cell), F in (("box room 156 x 156, empty", box_room(False), 64), ("box room 156 x 156, four boxes", box_room(True), 64),
                                          ("floor 400 x 400, empty", big_floor(False), 8), ("floor 400 x 400, comb of walls", big_floor(True), 8)):
        builds[name] = time_field(free, origin, cell, goals_on(free, origin, cell, F, rng))
        print(name, builds[name], flush=True)
    results["field_builds"] = builds

    # ---- the selection launch on the buffers the scene-free search loop of bench_genop_search.py leaves behind
    b, N, K, V = args.seqs, args.candidates, args.primitives, args.num_verts
    lib = _lib.load()
    op, body = build_op(V)
    g = torch.Generator().manual_seed(1)
    data_r, xb_r, betas_r = seeds(body, b * N, g)
    data_b, xb_b, betas_b = data_r[:, ::N].contiguous(), xb_r[:, ::N].contiguous(), betas_r[::N].contiguous()
    z = torch.randn(K, b * N, 128, generator=g).cuda()
    goal = torch.tensor([0.5, 3.0, 0.9])
    T0 = torch.zeros(b, 3)
    T0[:, 0] = torch.linspace(-1.0, 2.5, b)
    T0[:, 1] = -1.5
    _, sf = captured(op, "_search_loop", lambda: op.generate_sequence_to_goal(data_b, xb_b, betas_b, goal, K, N, z=z, T0=T0, to_numpy=False))
    s = sf[3]
    free, origin, cell = box_room(True)
    field = geodesic.GeodesicField.from_raster(free, origin, cell, goal[None].repeat(b, 1).numpy())
    fargs, _alive = field.select_args(b)
    st = _lib.current_stream_ptr()
    cur, lbs = s["xs"][(K - 1) % 2], s["lbs_out"]
    vp = lambda t: C.c_void_p(t.data_ptr())
    lead = (_lib.ptr(s["Y_gen"]), vp(cur[0]), vp(cur[1]), 201, _lib.ptr(lbs["joints"]), 127, _lib.ptr(lbs["markers"]), _lib.ptr(s["R0"]),
            _lib.ptr(s["T0"]), None, _lib.ptr(s["goal"]), _lib.ptr(s["feet"]), s["weights"], s["pene_thres"], s["goal_thresh"], s["rf"], b, N)
    outs = (vp(s["choice"][K - 1]), vp(s["status"][K - 1]), vp(s["reached"][K - 1]), vp(s["goal_dist"][K - 1]), vp(s["cost"][K - 1]),
            vp(s["cost_terms"][K - 1]), vp(s["colliding"][K - 1]))
    legs = {}
    if os.path.exists(args.parent_lib):
        parent = C.CDLL(args.parent_lib)
        parent.egx_primitive_select.restype, parent.egx_primitive_select.argtypes = _lib.SIGNATURES["egx_primitive_select"]
        legs["parent"] = lambda: _lib.check(parent.egx_primitive_select(*lead, *outs, st), "egx_primitive_select (parent)")
    legs["no_field"] = lambda: _lib.check(lib.egx_primitive_select(*lead, *outs, st), "egx_primitive_select")
    legs["field"] = lambda: _lib.check(lib.egx_primitive_select_field(*lead, *outs, *fargs, st), "egx_primitive_select_field")
    if "parent" in legs:                                        # the same inputs give the same bits in both libraries
        legs["parent"]()
        torch.cuda.synchronize()
        keys = ("choice", "status", "reached", "goal_dist", "cost", "cost_terms", "colliding")
        want = [s[k][K - 1].clone() for k in keys]
        for k in keys:
            s[k][K - 1].fill_(-3)
        legs["no_field"]()
        torch.cuda.synchronize()
        differ = [k for a, k in zip(want, keys) if not torch.equal(a, s[k][K - 1])]
        # the beam selection on the same rows (W = 2 slots of N / 2 candidates, a carried cost per slot), both libraries
        W, Nb = 2, N // 2
        acc = torch.rand(b, W, generator=torch.Generator().manual_seed(5)).cuda()
        ncoll = torch.zeros(b, W, dtype=torch.int32, device="cuda")
        parent.egx_primitive_beam_select.restype, parent.egx_primitive_beam_select.argtypes = _lib.SIGNATURES["egx_primitive_beam_select"]
        got = []
        for entry in (parent.egx_primitive_beam_select, lib.egx_primitive_beam_select):
            o = [torch.full((b, W * Nb), -3.0, device="cuda"), torch.full((b, W * Nb, 5), -3.0, device="cuda"),
                 torch.full((b, W * Nb), -3, dtype=torch.int32, device="cuda")] + \
                [torch.full((b, W), -3, dtype=torch.int32, device="cuda") if i32 else torch.full((b, W), -3.0, device="cuda")
                 for i32 in (1, 1, 0, 1, 0, 1, 0, 1)]
            _lib.check(entry(*lead[:16], b, W, Nb, _lib.ptr(acc), _lib.ptr(ncoll), *[_lib.ptr(t) for t in o], st), "egx_primitive_beam_select")
            torch.cuda.synchronize()
            got.append(o)
        differ += [f"beam output {i}" for i, (x, y) in enumerate(zip(*got)) if not torch.equal(x, y)]
        results["no_field_equals_parent"] = not differ
        results["no_field_differs_in"] = differ
    t = alternate(legs, args.iters, args.warmup, repeats=5)
    results.update(select_us=t, seqs=b, candidates=N, num_verts=V, parent_measured="parent" in legs)
    print(json.dumps(results, indent=1), flush=True)

    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "geodesic.json"), "w") as fh:
        json.dump(results, fh, indent=1)
    fmt = lambda v: f"{v['median_us']:.2f} ({v['min_us']:.2f} .. {v['max_us']:.2f})"
    lines = [BEGIN, f"Device: {results['device']}.", "", "Field builds, `egx_geodesic_field` alone (host clock, the entry ends in a stream "
             "synchronise; five builds after a first one): milliseconds, median (min .. max).", "",
             "| raster | F | free cells | passes | ms | longest path (m) |", "|---|---|---|---|---|---|"]
    for name, v in builds.items():
        lines.append(f"| {name} | {v['F']} | {v['free_cells']} | {v['passes']} | {v['median_ms']:.2f} ({v['min_ms']:.2f} .. {v['max_ms']:.2f}) | "
                     f"{v['longest_path_m']:.1f} |")
    lines += ["", f"The selection launch, b x N = {b} x {N} rows on the buffers of the scene-free search loop of scripts/bench_genop_search.py: "
              f"device events around {args.iters} launches, five windows per variant, variants alternating.  Microseconds per launch, median "
              "(min .. max).", "", "| variant | us |", "|---|---|"]
    if "parent" in t:
        lines.append(f"| `egx_primitive_select`, parent commit's library | {fmt(t['parent'])} |")
    else:
        lines.append("| `egx_primitive_select`, parent commit's library | not measured (no library given) |")
    lines += [f"| `egx_primitive_select`, this commit, no field | {fmt(t['no_field'])} |",
              f"| `egx_primitive_select_field`, field of the box room (F = {b}) | {fmt(t['field'])} |"]
    spread = lambda v: v["max_us"] - v["min_us"]
    if "parent" in t:
        lines += ["", f"Spread over the five alternating windows (max - min): parent {spread(t['parent']):.2f} us, no field "
                  f"{spread(t['no_field']):.2f} us, field {spread(t['field']):.2f} us.  Median without a field minus the parent's median: "
                  f"{t['no_field']['median_us'] - t['parent']['median_us']:+.2f} us; with a field minus without: "
                  f"{t['field']['median_us'] - t['no_field']['median_us']:+.2f} us."]
    if "no_field_equals_parent" in results:
        lines += ["", f"Outputs of the no-field launch bit-identical to the parent's on these {b * N} rows: {results['no_field_equals_parent']}"
                  + (f" (differing: {', '.join(results['no_field_differs_in'])})." if results["no_field_differs_in"] else ".")]
    lines.append(END)
    md = os.path.join(args.out_dir, "geodesic.md")
    txt = open(md).read() if os.path.exists(md) else "# Geodesic field\n\n" + BEGIN + "\n" + END + "\n"
    txt = txt[:txt.index(BEGIN)] + "\n".join(lines) + txt[txt.index(END) + len(END):]
    with open(md, "w") as fh:
        fh.write(txt)


if __name__ == "__main__":
    main()
