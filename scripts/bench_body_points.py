#!/usr/bin/env python3
"""Gradient through the body model on the 67 marker rows: `MarkerBodyModel` (torch ops under autograd) against `BodyPoints`
(egx_points_forward / egx_points_backward), and one `GAMMARegressorTrainOP.step` with either.  GPU only.

    python scripts/bench_body_points.py [--out-dir profiles] [--iters 200] [--warmup 20]     # timings
    python scripts/bench_body_points.py --trace [--out-dir profiles]                           # launches per step, kernel time

Timings: the two legs alternate in one process; device events around --iters forward + backward passes after --warmup of them,
repeated three times; median and spread (min .. max) of the three per-pass times.  Sizes: n = 320 bodies (16 x 20, the batch of
cfg_samp20/MoshRegressor_v3_male.yml) and n = 2048.  Before timing, the outputs and input gradients of the two legs on the same
inputs are compared.  --trace runs each leg in a process of its own under `rocprofv3 --kernel-trace`, twice with different
numbers of passes, and reports the difference per pass (launches, summed kernel time), so that set-up launches do not count.

Both modes update `<out-dir>/body_points.json` and the section between the `timings` markers of `<out-dir>/body_points.md`."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from egogen_amd import synth  # noqa: E402
from egogen_amd.body_model import BodyPoints  # noqa: E402
from egogen_amd.models import REGRESSOR_CFG  # noqa: E402
from egogen_amd.train_regressor import GAMMARegressorTrainOP, MarkerBodyModel  # noqa: E402

SIZES = (320, 2048)
BEGIN, END = "<!-- timings:begin -->", "<!-- timings:end -->"


def inputs(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    xb = 0.3 * torch.randn(n, 93, generator=g)
    betas = torch.randn(n, 10, generator=g)
    cot = torch.randn(n, 67, 3, generator=g)
    return xb.cuda(), betas.cuda(), cot.cuda()


def make_pass(model, xb, betas, cot):
    """One forward + backward: d sum(points * cot) / d xb."""
    x = xb.clone().requires_grad_(True)

    def run():
        x.grad = None
        model(x, betas).backward(cot)
        return x.grad
    return run, x


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def alternate(legs, warmup, iters, repeats=3):
    """legs: {name: fn}.  -> {name: [ms per pass] x repeats}, the legs taking turns within every repeat."""
    for fn in legs.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in legs}
    for _ in range(repeats):
        for k, fn in legs.items():
            out[k].append(timed(fn, iters))
    return out


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "runs_ms": [float(v) for v in ms]}


def train_op(kind, body, markers, tmp):
    op = GAMMARegressorTrainOP(dict(REGRESSOR_CFG, gender="male", seq_len=10), {"weight_reg_hpose": 0.01},
                               {"log_dir": os.path.join(tmp, "logs_" + kind), "save_dir": os.path.join(tmp, "ckpt_" + kind),
                                "batch_size": 16, "marker_body_model": kind})
    torch.manual_seed(0)
    op.build_model(body, markers)
    return op, torch.optim.Adam(op.model.parameters(), lr=1e-4)


def run_timings(a):
    body, markers = synth.make_body_model(0), [int(v) for v in synth.marker_ids()]
    torch_bm, hip_bm = MarkerBodyModel(body, markers).cuda(), BodyPoints(body, markers)
    rec = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup, "sizes": {}}
    for n in SIZES:
        xb, betas, cot = inputs(n)
        legs, xs = {}, {}
        for name, model in (("torch", torch_bm), ("hip", hip_bm)):
            legs[name], xs[name] = make_pass(model, xb, betas, cot)
        with torch.no_grad():
            d_out = float((torch_bm(xb, betas) - hip_bm(xb, betas)).abs().max())
        g_t, g_h = legs["torch"]().clone(), legs["hip"]().clone()
        d_grad, s_grad = float((g_t - g_h).abs().max()), float(g_t.abs().max())
        t = alternate(legs, a.warmup, a.iters)
        rec["sizes"][str(n)] = {"max_abs_points_diff": d_out, "max_abs_grad_diff": d_grad, "max_abs_grad": s_grad,
                                "torch": stats(t["torch"]), "hip": stats(t["hip"])}
        print(f"n = {n}: torch {np.median(t['torch']):.4f} ms, hip {np.median(t['hip']):.4f} ms per forward + backward "
              f"(outputs differ by {d_out:.1e} m, gradients by {d_grad:.1e} of {s_grad:.1e})", flush=True)
    # one whole optimiser step of the regressor, n = 320
    with tempfile.TemporaryDirectory() as tmp:
        n = SIZES[0]
        g = torch.Generator().manual_seed(1)
        marker_ref, betas = (0.4 * torch.randn(n, 67, 3, generator=g)).cuda(), torch.randn(n, 10, generator=g).cuda()
        legs = {}
        for kind in ("torch", "hip"):
            op, opt = train_op(kind, body, markers, tmp)
            legs[kind] = lambda op=op, opt=opt: op.step(opt, marker_ref, betas)
        t = alternate(legs, a.warmup, a.iters)
        rec["train_step"] = {"n": n, "torch": stats(t["torch"]), "hip": stats(t["hip"])}
        print(f"train step, n = {n}: torch {np.median(t['torch']):.4f} ms, hip {np.median(t['hip']):.4f} ms", flush=True)
    return rec


# ---------------------------------------------------------------------------------------------------------------------------
# kernel trace: a child process per leg and pass count
# ---------------------------------------------------------------------------------------------------------------------------
def child(leg, n, passes):
    body, markers = synth.make_body_model(0), [int(v) for v in synth.marker_ids()]
    model = MarkerBodyModel(body, markers).cuda() if leg == "torch" else BodyPoints(body, markers)
    run, _ = make_pass(model, *inputs(n))
    for _ in range(passes):
        run()
    torch.cuda.synchronize()


def trace_once(leg, n, passes, tmp):
    d = os.path.join(tmp, f"{leg}_{passes}")
    cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "p", "--", sys.executable, os.path.abspath(__file__),
           "--child", leg, "--n", str(n), "--passes", str(passes)]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=300)
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"rocprofv3 wrote no kernel trace under {d}")
    count, ns = 0, 0
    for f in files:
        for row in csv.DictReader(open(f)):
            count += 1
            ns += int(row["End_Timestamp"]) - int(row["Start_Timestamp"])
    return count, ns


def run_trace(a):
    n, p1, p2 = SIZES[0], 20, 60
    rec = {"n": n, "passes": [p1, p2]}
    with tempfile.TemporaryDirectory() as tmp:
        for leg in ("torch", "hip"):
            (c1, t1), (c2, t2) = trace_once(leg, n, p1, tmp), trace_once(leg, n, p2, tmp)
            rec[leg] = {"launches_per_pass": (c2 - c1) / (p2 - p1), "kernel_us_per_pass": (t2 - t1) / (p2 - p1) / 1e3}
            print(f"trace, n = {n}, {leg}: {rec[leg]['launches_per_pass']:.1f} launches, {rec[leg]['kernel_us_per_pass']:.1f} us of kernels per "
                  f"forward + backward", flush=True)
    return rec


# ---------------------------------------------------------------------------------------------------------------------------
def render(rec):
    L = [BEGIN, "## Timings", ""]
    t = rec.get("timings")
    if t:
        L += [f"One run of `scripts/bench_body_points.py` on one {t['device']}; full-size synthetic body (V = 10 475), the 67 SSM2 markers.",
              f"Device events around {t['iters']} forward + backward passes (d sum(points x cotangent) / d xb) after {t['warmup']} warm-up passes, "
              "three repeats with the two legs taking turns; median (min .. max) of the three, per pass.", "",
              "| n bodies | `MarkerBodyModel` (torch ops) ms | `BodyPoints` (HIP) ms | ratio | max abs diff of points (m) | max abs diff of d/dxb (of max) |",
              "|---|---|---|---|---|---|"]
        f = lambda s: f"{s['median_ms']:.4f} ({s['min_ms']:.4f} .. {s['max_ms']:.4f})"
        for n, r in t["sizes"].items():
            L.append(f"| {n} | {f(r['torch'])} | {f(r['hip'])} | {r['torch']['median_ms'] / r['hip']['median_ms']:.1f} x | {r['max_abs_points_diff']:.1e} | "
                     f"{r['max_abs_grad_diff']:.1e} ({r['max_abs_grad']:.1e}) |")
        s = t["train_step"]
        L += ["", f"One optimiser step of `GAMMARegressorTrainOP` (`step`: network forward, loss with its host read-back of the two "
              f"items, backward, Adam; n = {s['n']}), same method:", "",
              "| `marker_body_model` | ms per step |", "|---|---|", f"| `torch` | {f(s['torch'])} |", f"| `hip` | {f(s['hip'])} |"]
    tr = rec.get("trace")
    if tr:
        L += ["", f"Kernel trace (`rocprofv3 --kernel-trace`, a process per leg, n = {tr['n']}; difference between runs of {tr['passes'][1]} and "
              f"{tr['passes'][0]} passes, per forward + backward pass):", "",
              "| leg | launches per pass | kernel time per pass (us) |", "|---|---|---|"]
        for leg in ("torch", "hip"):
            L.append(f"| {leg} | {tr[leg]['launches_per_pass']:.1f} | {tr[leg]['kernel_us_per_pass']:.1f} |")
    return L + [END]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--child", choices=("torch", "hip"))
    ap.add_argument("--n", type=int, default=SIZES[0])
    ap.add_argument("--passes", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_body_points.py measures on the HIP device; there is nothing to report without one")
    if a.iters < 200 and not a.child and not a.trace:
        raise SystemExit("--iters must be at least 200")
    if a.child:
        return child(a.child, a.n, a.passes)
    os.makedirs(a.out_dir, exist_ok=True)
    jpath, mpath = os.path.join(a.out_dir, "body_points.json"), os.path.join(a.out_dir, "body_points.md")
    rec = json.load(open(jpath)) if os.path.exists(jpath) else {}
    rec["trace" if a.trace else "timings"] = run_trace(a) if a.trace else run_timings(a)
    with open(jpath, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    md = open(mpath).read() if os.path.exists(mpath) else "# Differentiable body points\n\n" + BEGIN + "\n" + END + "\n"
    if BEGIN not in md or END not in md:
        md = md.rstrip("\n") + "\n\n" + BEGIN + "\n" + END + "\n"
    head, rest = md.split(BEGIN, 1)
    tail = rest.split(END, 1)[1]
    with open(mpath, "w") as fh:
        fh.write(head + "\n".join(render(rec)) + tail)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
