#!/usr/bin/env python3
"""`GAMMAPrimitiveComboGenOP.generate_sequence_to_goal` at b x N = 64 x 16 = 1024 candidate rows, K = 10 primitives, without a
scene and in the single-box 256^3 SDF scene, against `generate_sequence` at b = 1024 (the same row count), and the two new
launches alone (egx_primitive_select, egx_primitive_advance_select) on the search loop's own buffers.  GPU only.

    python scripts/bench_genop_search.py [--out-dir profiles] [--seqs 64] [--candidates 16] [--primitives 10] [--iters 20] [--warmup 5]
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/bench_genop_search.py --trace-only      (per-kernel times)

Device events around --iters passes after --warmup of them, three windows per leg, legs alternating; median and range (min .. max)
of the three per-pass times.  Launches per primitive: kernel records of one profiled loop (torch.profiler) divided by K.  With
--illustrate, the final goal distance and the colliding choices for N in {1, 4, 16} with the seeded random-weight prior: an
illustration of the mechanism, NOT a statement about motion quality.  Writes `<out-dir>/genop_search.json` and replaces the section
between the `timings` markers of `<out-dir>/genop_search.md`."""
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

from bench_genop import alternate  # noqa: E402
from egogen_amd import _lib, synth  # noqa: E402
from egogen_amd.body_model import BodyModelHandle, SdfScene  # noqa: E402
from egogen_amd.genop import GAMMAPrimitiveComboGenOP  # noqa: E402
from egogen_amd.models import GAMMAPrimitiveCombo, PREDICTOR_CFG, REGRESSOR_CFG  # noqa: E402

BEGIN, END = "<!-- timings:begin -->", "<!-- timings:end -->"


def build_op(V):
    body = BodyModelHandle(synth.make_body_model(0, num_verts=V), synth.marker_ids(V), synth.feet_vids(V))
    combo = GAMMAPrimitiveCombo(PREDICTOR_CFG, REGRESSOR_CFG)
    sd = combo.state_dict()                   # seeded weights at gains that keep a 10-primitive chain finite (bench_genop.py)
    for prefix, seed, gain in (("predictor.", 520, 0.5), ("regressor.", 521, 0.3)):
        shapes = {k[len(prefix):]: tuple(v.shape) for k, v in sd.items() if k.startswith(prefix)}
        sd.update({prefix + k: torch.from_numpy(v) for k, v in synth.seeded_fill(shapes, seed, gain=gain).items()})
    combo.load_state_dict(sd)
    op = GAMMAPrimitiveComboGenOP({"modelconfig": PREDICTOR_CFG}, {"modelconfig": dict(REGRESSOR_CFG, gender="male")}, {"gpu_index": 0})
    op.model, op.body_model = combo.cuda().eval(), body
    return op, body


def seeds(body, B, g):
    xb = torch.zeros(2, B, 93)
    xb[:, :, :3] = torch.arange(2).view(2, 1, 1) * torch.tensor([0.0, 0.02, 0.0]) + torch.tensor([0.0, 0.0, 0.9])
    xb[:, :, 3:69] = torch.randn(1, B, 66, generator=g) * 0.08
    betas = torch.randn(B, 10, generator=g) * 0.5
    data = body.forward(xb.reshape(2 * B, 93).cuda(), betas.cuda().repeat(2, 1), 1, want_verts=False)["markers"].reshape(2, B, 201)
    return data, xb.cuda(), betas


def captured(op, name, call):
    """run `call` once with op.<name> spied on -> a closure that repeats that loop on the same buffers"""
    kept = {}
    real = getattr(op, name)

    def spy(*a):
        kept["args"] = a
        real(*a)
    setattr(op, name, spy)
    try:
        call()
    finally:
        setattr(op, name, real)
    return (lambda: real(*kept["args"])), kept["args"]


def launches_of(loop, K):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            loop()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if "DeviceType.CUDA" in str(getattr(e, "device_type", "")))
        return n / K if n else None
    except Exception as e:      # the profiler is optional equipment
        print("profiler unavailable:", e)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--seqs", type=int, default=64)
    ap.add_argument("--candidates", type=int, default=16)
    ap.add_argument("--primitives", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--num-verts", type=int, default=synth.NUM_VERTS)
    ap.add_argument("--sdf-res", type=int, default=256)
    ap.add_argument("--trace-only", action="store_true", help="three passes of each loop and nothing else (for a kernel trace)")
    ap.add_argument("--illustrate", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_genop_search.py measures on the GPU; no device is visible")
    b, N, K, V = args.seqs, args.candidates, args.primitives, args.num_verts
    rows = b * N
    lib = _lib.load()
    op, body = build_op(V)
    g = torch.Generator().manual_seed(1)
    data_r, xb_r, betas_r = seeds(body, rows, g)         # the parent's chain: one sequence per row
    data_b, xb_b, betas_b = data_r[:, ::N].contiguous(), xb_r[:, ::N].contiguous(), betas_r[::N].contiguous()
    z = torch.randn(K, rows, 128, generator=g).cuda()
    goal = torch.tensor([0.5, 3.0, 0.9])
    T0 = torch.zeros(b, 3)
    T0[:, 0] = torch.linspace(-1.0, 2.5, b)               # starts spread along x in front of the box (x 1..2, y -0.5..0.5)
    T0[:, 1] = -1.5
    scene = SdfScene(synth.make_sdf_scene(args.sdf_res))
    results = {"seqs": b, "candidates": N, "rows": rows, "primitives": K, "iters": args.iters, "warmup": args.warmup, "num_verts": V,
               "sdf_res": args.sdf_res, "device": torch.cuda.get_device_name(0)}

    parent, _ = captured(op, "_advance_loop", lambda: op.generate_sequence(data_r, xb_r, betas_r, K, z=z, to_numpy=False))
    free, sf = captured(op, "_search_loop", lambda: op.generate_sequence_to_goal(data_b, xb_b, betas_b, goal, K, N, z=z, T0=T0, to_numpy=False))
    boxed, _ = captured(op, "_search_loop", lambda: op.generate_sequence_to_goal(data_b, xb_b, betas_b, goal, K, N, z=z, T0=T0, scene=scene,
                                                                                 to_numpy=False))
    legs = {"generate_sequence": parent, "search_no_scene": free, "search_box_scene": boxed}
    if args.trace_only:
        for fn in legs.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        return

    # ---- the two new launches alone, on the buffers the scene-free loop left behind (primitive K - 1)
    s = sf[3]
    st = _lib.current_stream_ptr()
    cur, nxt = s["xs"][(K - 1) % 2], s["xs"][K % 2]
    lbs = s["lbs_out"]
    vp = lambda t: C.c_void_p(t.data_ptr())
    R0b, T0b = s["R0"].clone(), s["T0"].clone()

    def select():
        _lib.check(lib.egx_primitive_select(
            _lib.ptr(s["Y_gen"]), vp(cur[0]), vp(cur[1]), 201, _lib.ptr(lbs["joints"]), 127, _lib.ptr(lbs["markers"]), _lib.ptr(s["R0"]),
            _lib.ptr(s["T0"]), None, _lib.ptr(s["goal"]), _lib.ptr(s["feet"]), s["weights"], s["pene_thres"], s["goal_thresh"], s["rf"], b, N,
            vp(s["choice"][K - 1]), vp(s["status"][K - 1]), vp(s["reached"][K - 1]), vp(s["goal_dist"][K - 1]), vp(s["cost"][K - 1]),
            vp(s["cost_terms"][K - 1]), vp(s["colliding"][K - 1]), st), "egx_primitive_select")

    def hand_off():
        R0b.copy_(s["R0"])      # the kernel updates the frame in place: every launch starts from the same one
        T0b.copy_(s["T0"])
        _lib.check(lib.egx_primitive_advance_select(
            _lib.ptr(s["pp"]), _lib.ptr(s["Y_gen"]), vp(cur[0]), vp(cur[1]), 201, _lib.ptr(lbs["joints"]), 127, _lib.ptr(lbs["markers"]),
            _lib.ptr(s["delta_T"]), s["rf"], b, vp(s["choice"][K - 1]), N, _lib.ptr(R0b), _lib.ptr(T0b), vp(s["markers"][K - 1]),
            vp(s["pelvis"][K - 1]), vp(s["rotmat"][K - 1]), vp(s["transl"][K - 1]), vp(s["params"][K - 1]), _lib.ptr(s["seed"]), vp(nxt[0]),
            vp(nxt[1]), 201, _lib.ptr(s["nonfinite"]), st), "egx_primitive_advance_select")

    def copies():
        R0b.copy_(s["R0"])
        T0b.copy_(s["T0"])
    t = alternate(dict(legs, select=select, hand_off=hand_off, copies=copies), args.iters, args.warmup)
    per = {k: {m: v / K for m, v in t[k].items()} for k in legs}
    ho = {m: t["hand_off"][m] - t["copies"]["median_us"] for m in t["hand_off"]}
    results.update(per_primitive_us=per, select_kernel_us=t["select"], advance_select_kernel_us=ho, frame_copies_us=t["copies"],
                   overhead_no_scene=per["search_no_scene"]["median_us"] / per["generate_sequence"]["median_us"] - 1.0,
                   overhead_box_scene=per["search_box_scene"]["median_us"] / per["generate_sequence"]["median_us"] - 1.0,
                   launches_per_primitive={k: launches_of(fn, K) for k, fn in legs.items()})
    if args.illustrate:
        ill = {}
        for n in (1, 4, 16):
            r = op.generate_sequence_to_goal(data_b, xb_b, betas_b, goal, K, n, T0=T0, scene=scene)
            last = r.goal_dist[np.asarray(r.n_valid) - 1, np.arange(b)]
            ill[str(n)] = {"mean_final_goal_dist_m": float(last.mean()), "reached": int((np.asarray(r.n_valid) < K).sum()),
                           "colliding_choices": int((r.status & 1).sum()), "choices": int(r.status.size)}
        results["illustration_random_weight_prior"] = ill
    print(json.dumps(results, indent=1), flush=True)

    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "genop_search.json"), "w") as fh:
        json.dump(results, fh, indent=1)
    fmt = lambda v: f"{v['median_us']:.1f} ({v['min_us']:.1f} .. {v['max_us']:.1f})"
    ln = results["launches_per_primitive"]
    fl = lambda v: "n/a" if v is None else f"{v:.1f}"
    lines = [BEGIN, f"Device: {results['device']}; b x N = {b} x {N} = {rows} rows, K = {K}, body of {V} vertices, SDF grid {args.sdf_res}^3; "
             f"{args.iters} passes per window, three windows per leg, legs alternating.  Microseconds: median (min .. max).", "",
             "| what | us per primitive | launches per primitive |", "|---|---|---|",
             f"| generate_sequence, b = {rows} (the parent's chain) | {fmt(per['generate_sequence'])} | {fl(ln['generate_sequence'])} |",
             f"| generate_sequence_to_goal, {b} x {N}, no scene | {fmt(per['search_no_scene'])} | {fl(ln['search_no_scene'])} |",
             f"| generate_sequence_to_goal, {b} x {N}, single-box scene | {fmt(per['search_box_scene'])} | {fl(ln['search_box_scene'])} |",
             "", f"Overhead against the parent's chain: {100 * results['overhead_no_scene']:+.1f} % without a scene, "
             f"{100 * results['overhead_box_scene']:+.1f} % in the box scene (which adds the penetration count to the SMPL-X launch).", "",
             "| launch alone (device events, scene-free buffers) | us |", "|---|---|",
             f"| egx_primitive_select | {fmt(t['select'])} |",
             f"| egx_primitive_advance_select (frame copies of {t['copies']['median_us']:.1f} us subtracted) | {fmt(ho)} |"]
    if args.illustrate:
        lines += ["", "Illustration only, seeded random-weight prior (no statement about motion quality): goal 3 m ahead, box scene, "
                  f"b = {b}, K = {K}, default weights.", "", "| N | mean final goal distance (m) | sequences that reached the goal | colliding choices |",
                  "|---|---|---|---|"]
        for n, v in results["illustration_random_weight_prior"].items():
            lines.append(f"| {n} | {v['mean_final_goal_dist_m']:.3f} | {v['reached']} of {b} | {v['colliding_choices']} of {v['choices']} |")
    lines.append(END)
    md = os.path.join(args.out_dir, "genop_search.md")
    txt = open(md).read() if os.path.exists(md) else "# Primitive search\n\n" + BEGIN + "\n" + END + "\n"
    if BEGIN in txt and END in txt:
        txt = txt[:txt.index(BEGIN)] + "\n".join(lines) + txt[txt.index(END) + len(END):]
    else:
        txt += "\n" + "\n".join(lines) + "\n"
    with open(md, "w") as fh:
        fh.write(txt)


if __name__ == "__main__":
    main()
