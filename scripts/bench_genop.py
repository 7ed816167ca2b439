#!/usr/bin/env python3
"""`GAMMAPrimitiveComboGenOP.generate_sequence` at b = 1024 sequences, K = 10 primitives, and inside it the hand-off kernel
egx_primitive_advance against the same hand-off composed on the device from the torch ops of tests/genop_ref.py::advance (test
code, not the code under test).  GPU only.

    python scripts/bench_genop.py [--out-dir profiles] [--batch 1024] [--primitives 10] [--iters 20] [--warmup 5]

Device events around --iters passes after --warmup of them, three windows per leg, legs alternating; median and range (min .. max)
of the three per-pass times.  Legs: the whole primitive loop (ms per primitive), the kernel alone on the loop's own buffers, the
torch-op composition on the same inputs.  Launches per primitive: kernel records of one profiled loop (torch.profiler) divided by
K, or `n/a` where the profiler sees no device activity.  Writes `<out-dir>/genop.json` and replaces the section between the
`timings` markers of `<out-dir>/genop.md`."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from egogen_amd import _lib, synth  # noqa: E402
from egogen_amd.body_model import BodyModelHandle  # noqa: E402
from egogen_amd.genop import GAMMAPrimitiveComboGenOP  # noqa: E402
from egogen_amd.models import GAMMAPrimitiveCombo, PREDICTOR_CFG, REGRESSOR_CFG  # noqa: E402
from tests import genop_ref  # noqa: E402

BEGIN, END = "<!-- timings:begin -->", "<!-- timings:end -->"


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3   # microseconds per pass


def alternate(legs, iters, warmup, repeats=3):
    for fn in legs.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in legs}
    for _ in range(repeats):
        for k, fn in legs.items():
            t[k].append(timed(fn, iters))
    return {k: {"median_us": float(np.median(v)), "min_us": float(min(v)), "max_us": float(max(v))} for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--primitives", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--num-verts", type=int, default=synth.NUM_VERTS)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_genop.py measures on the GPU; no device is visible")
    B, K, V = args.batch, args.primitives, args.num_verts
    lib = _lib.load()
    body = BodyModelHandle(synth.make_body_model(0, num_verts=V), synth.marker_ids(V), synth.feet_vids(V))
    combo = GAMMAPrimitiveCombo(PREDICTOR_CFG, REGRESSOR_CFG)
    sd = combo.state_dict()                   # seeded weights at gains that keep a 10-primitive chain finite
    for prefix, seed, gain in (("predictor.", 520, 0.5), ("regressor.", 521, 0.3)):
        shapes = {k[len(prefix):]: tuple(v.shape) for k, v in sd.items() if k.startswith(prefix)}
        sd.update({prefix + k: torch.from_numpy(v) for k, v in synth.seeded_fill(shapes, seed, gain=gain).items()})
    combo.load_state_dict(sd)
    op = GAMMAPrimitiveComboGenOP({"modelconfig": PREDICTOR_CFG}, {"modelconfig": dict(REGRESSOR_CFG, gender="male")}, {"gpu_index": 0})
    op.model, op.body_model = combo.cuda().eval(), body
    g = torch.Generator().manual_seed(1)
    xb = torch.zeros(2, B, 93)
    xb[:, :, :3] = torch.arange(2).view(2, 1, 1) * torch.tensor([0.0, 0.02, 0.0]) + torch.tensor([0.0, 0.0, 0.9])
    xb[:, :, 3:69] = torch.randn(1, B, 66, generator=g) * 0.08
    betas = torch.randn(B, 10, generator=g) * 0.5
    data = body.forward(xb.reshape(2 * B, 93).cuda(), betas.cuda().repeat(2, 1), 1, want_verts=False)["markers"].reshape(2, B, 201)
    z = torch.randn(K, B, 128, generator=g).cuda()
    results = {"batch": B, "primitives": K, "iters": args.iters, "warmup": args.warmup, "num_verts": V, "device": torch.cuda.get_device_name(0)}

    # ---- the loop: capture the arguments generate_sequence hands to its primitive loop, then time that loop alone
    kept = {}
    real = op._advance_loop

    def spy(*a):
        kept["args"] = a
        real(*a)
    op._advance_loop = spy
    res = op.generate_sequence(data, xb.cuda(), betas, K, z=z, to_numpy=False)
    op._advance_loop = real
    assert bool(torch.isfinite(res.markers).all())
    la = kept["args"]
    s = la[2]                       # the state dict of _advance_loop(K, B, s)
    rf, xs, seed, Y_gen, lbs_out, delta_T, R0, T0 = (s[k] for k in ("rf", "xs", "seed", "Y_gen", "lbs_out", "delta_T", "R0", "T0"))
    markers, params, rotmat, transl, pelvis, nonfinite = (s[k] for k in ("markers", "params", "rotmat", "transl", "pelvis", "nonfinite"))
    loop = lambda: real(*la)

    # ---- the kernel alone, on the buffers the loop left behind (primitive K - 1), and the torch-op composition of the same hand-off
    st = _lib.current_stream_ptr()
    cur, nxt = xs[(K - 1) % 2], xs[K % 2]
    pp = params[K - 1]
    R0b, T0b = R0.clone(), T0.clone()

    def kernel():
        R0b.copy_(R0)           # the kernel updates the frame in place: both legs start from the same one
        T0b.copy_(T0)
        _lib.check(lib.egx_primitive_advance(
            _lib.ptr(pp), _lib.ptr(Y_gen), C.c_void_p(cur[0].data_ptr()), C.c_void_p(cur[1].data_ptr()), 201, _lib.ptr(lbs_out["joints"]), 127,
            _lib.ptr(lbs_out["markers"]), _lib.ptr(delta_T), rf, B, _lib.ptr(R0b), _lib.ptr(T0b), _lib.ptr(markers[K - 1]), _lib.ptr(pelvis[K - 1]),
            _lib.ptr(rotmat[K - 1]), _lib.ptr(transl[K - 1]), _lib.ptr(seed), C.c_void_p(nxt[0].data_ptr()), C.c_void_p(nxt[1].data_ptr()), 201,
            _lib.ptr(nonfinite), st), "egx_primitive_advance")

    def copies():
        R0b.copy_(R0)
        T0b.copy_(T0)
    J, mp = lbs_out["joints"].reshape(B, 20, 127, 3), lbs_out["markers"].reshape(B, 20, 67, 3)
    torch_ops = lambda: genop_ref.advance(pp, Y_gen, cur, J, mp, delta_T, rf, R0, T0, torch.float32, device="cuda")
    t = alternate({"loop": loop, "kernel": kernel, "copies": copies, "torch": torch_ops}, args.iters, args.warmup)
    per_prim = {k: v / K for k, v in t["loop"].items()}
    kern = {k: t["kernel"][k] - t["copies"]["median_us"] for k in t["kernel"]}
    results.update(loop_per_primitive=per_prim, advance_kernel=kern, advance_kernel_with_frame_copies=t["kernel"], frame_copies=t["copies"],
                   advance_torch_ops=t["torch"], advance_share=kern["median_us"] / per_prim["median_us"])
    launches = None
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            loop()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if "DeviceType.CUDA" in str(getattr(e, "device_type", "")))
        launches = n / K if n else None
    except Exception as e:      # the profiler is optional equipment
        print("profiler unavailable:", e)
    results["launches_per_primitive"] = launches
    print(json.dumps(results, indent=1), flush=True)

    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "genop.json"), "w") as fh:
        json.dump(results, fh, indent=1)
    fmt = lambda v: f"{v['median_us']:.1f} ({v['min_us']:.1f} .. {v['max_us']:.1f})"
    lines = [BEGIN, f"Device: {results['device']}; b = {B}, K = {K}, body of {V} vertices; {args.iters} passes per window, three windows per leg, "
             "legs alternating.  Microseconds: median (min .. max).", "",
             "| what | us |", "|---|---|",
             f"| generate_sequence loop, per primitive | {fmt(per_prim)} |",
             f"| launches per primitive | {'n/a' if launches is None else f'{launches:.1f}'} |",
             f"| egx_primitive_advance (frame copies of {t['copies']['median_us']:.1f} us subtracted) | {fmt(kern)} |",
             f"| share of a primitive | {100 * results['advance_share']:.2f} % |",
             f"| the same hand-off from torch ops (tests/genop_ref.py::advance on the device) | {fmt(t['torch'])} |", END]
    md = os.path.join(args.out_dir, "genop.md")
    txt = open(md).read() if os.path.exists(md) else "# Generation operator\n\n" + BEGIN + "\n" + END + "\n"
    if BEGIN in txt and END in txt:
        txt = txt[:txt.index(BEGIN)] + "\n".join(lines) + txt[txt.index(END) + len(END):]
    else:
        txt += "\n" + "\n".join(lines) + "\n"
    with open(md, "w") as fh:
        fh.write(txt)


if __name__ == "__main__":
    main()
