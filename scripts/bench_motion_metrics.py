#!/usr/bin/env python3
"""The two launches of the motion evaluator (entries egx_motion_metrics and egx_crowd_metrics, csrc/motion_metrics.hip): what they
cost.  GPU only.

    python scripts/bench_motion_metrics.py [--iters 20] [--out-dir profiles] [--table FILE]

Timing, in one process, on seeded random records (the kernels' work does not depend on the values): egx_motion_metrics at 1 024
motions x 10 primitives (182 frames each) with goal, penetration counts and the per-frame output, and without the three;
egx_crowd_metrics at 32 groups x 8 people x 10 primitives, hold off and on.  Device events around --iters launches on preallocated
buffers, the legs alternate, three windows per leg after --warmup, median and range (the conventions of
scripts/bench_genop_policy.py).  Next to it the float64 numpy reference tests/motion_metrics_ref.py on the same box, timed on
--ref-motions motions and one group and scaled to the full shape (it is loops over frames and pairs: a yardstick for the arithmetic,
not a contender).  `--table FILE`: the worst err / bound per column from the table tests/test_motion_metrics_gpu.py writes when
EGX_GENOP_TABLE names a file.  Writes `<out-dir>/motion_metrics.md` (sections between markers) and `<out-dir>/motion_metrics.json`."""
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

from egogen_amd import _lib, metrics, synth  # noqa: E402
from egogen_amd.crowd import PersonGroups  # noqa: E402

MARKS = {"timings": ("<!-- timings:begin -->", "<!-- timings:end -->"), "accuracy": ("<!-- accuracy:begin -->", "<!-- accuracy:end -->")}
HEAD = "# Measuring finished motions: the two launches of the evaluator\n"
K = 10


def write_section(out_dir, which, lines):
    begin, end = MARKS[which]
    md = os.path.join(out_dir, "motion_metrics.md")
    os.makedirs(out_dir, exist_ok=True)
    txt = open(md).read() if os.path.exists(md) else HEAD
    body = "\n".join([begin] + lines + [end])
    if begin in txt and end in txt:
        txt = txt[:txt.index(begin)] + body + txt[txt.index(end) + len(end):]
    else:
        txt += "\n" + body + "\n"
    with open(md, "w") as fh:
        fh.write(txt)


def random_set(n, seed, spread):
    """n motions of K primitives: seeded random records, every primitive in a frame of its own within `spread` metres"""
    rng = np.random.default_rng(seed)
    P = n * K
    f = lambda *s: rng.standard_normal(s, dtype=np.float32)
    yaw = rng.uniform(-np.pi, np.pi, P)
    R = np.zeros((P, 3, 3), np.float32)
    R[:, 0, 0], R[:, 0, 1], R[:, 1, 0], R[:, 1, 1], R[:, 2, 2] = np.cos(yaw), -np.sin(yaw), np.sin(yaw), np.cos(yaw), 1.0
    T = rng.uniform(-spread, spread, (P, 3)).astype(np.float32)
    goals = rng.uniform(-spread, spread, (n, 3)).astype(np.float32)
    return metrics.MotionSet(f(P, 20, 67, 3) * 0.4, f(P, 20, 3) * 0.1, R, T, f(P, 20, 93) * 0.1, f(P, 10), np.arange(n + 1) * K, ["2-frame"] * P, goals)


def accuracy(args):
    worst = {}
    for line in open(args.table):
        cells = [c.strip() for c in line.strip().strip("|").split("|")]
        if len(cells) != 5:
            continue
        kind, col = cells[0].split()[0], cells[1]
        key = (kind, col)
        worst[key] = max(worst.get(key, 0.0), float(cells[2]) / float(cells[3]))      # err / bound
    lines = ["Worst |got - ref| / (1e-10 * scale) per column over all cases of tests/test_motion_metrics_gpu.py (bound: 1; a float32 step",
             "would show as about 1000):", "", "| entry | column | worst ratio |", "|---|---|---|"]
    lines += [f"| {k[0]} | {k[1]} | {v:.1e} |" for k, v in sorted(worst.items())]
    write_section(args.out_dir, "accuracy", lines)
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--motions", type=int, default=1024)
    ap.add_argument("--groups", type=int, default=32)
    ap.add_argument("--people", type=int, default=8)
    ap.add_argument("--ref-motions", type=int, default=8)
    ap.add_argument("--table", default=None)
    args = ap.parse_args()
    if args.table:
        accuracy(args)
        return
    if not torch.cuda.is_available():
        sys.exit("bench_motion_metrics.py measures on the GPU; no device is visible")
    from bench_genop import alternate
    from tests import motion_metrics_ref as ref
    lib, dev, st = _lib.load(), torch.device("cuda", 0), _lib.current_stream_ptr()
    feet_idx = synth.feet_marker_idx()
    feet = (C.c_int32 * 6)(*feet_idx)

    ms = random_set(args.motions, 1, 7.0)
    d = ms.to(dev)
    lead, alive = ms.lead_args(d)
    n, Ftot, P = len(ms), int(ms.frame_src.shape[0]), ms.markers.shape[0]
    pene = torch.randint(0, 90, (P * 20,), device=dev, dtype=torch.int32)
    out_f = torch.empty(n, len(metrics.F64_COLUMNS), device=dev, dtype=torch.float64)
    out_i = torch.empty(n, len(metrics.I32_COLUMNS), device=dev, dtype=torch.int32)
    frames = torch.empty(Ftot, len(metrics.FRAME_COLUMNS), device=dev, dtype=torch.float64)

    def motion(full):
        _lib.check(lib.egx_motion_metrics(*lead, feet, _lib.ptr(d["goals"]) if full else None, 0.1, 0.0, _lib.ptr(pene) if full else None, 40,
                                          _lib.ptr(out_f), _lib.ptr(out_i), _lib.ptr(frames) if full else None, st), "egx_motion_metrics")

    cs = random_set(args.groups * args.people, 2, 1.0)
    cd = cs.to(dev)
    clead, calive = cs.lead_args(cd)
    pg = PersonGroups.from_ids(np.arange(len(cs)) // args.people, len(cs))
    sizes = pg.sizes.astype(np.int64)
    pair_start = np.concatenate([[0], np.cumsum(sizes * (sizes - 1) // 2)]).astype(np.int32)
    npairs, Fmax = int(pair_start[-1]), int(cs.frames.max())
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(dev)
    gs, gm, ps, gs_host = i32(pg.start), i32(pg.member), i32(pair_start), np.ascontiguousarray(pg.start, np.int32)
    clear = torch.empty(npairs, Fmax, device=dev, dtype=torch.float64)
    mdist = torch.empty(npairs, Fmax, device=dev, dtype=torch.float64)
    plist = torch.empty(npairs, 2, device=dev, dtype=torch.int32)

    def crowd(hold):
        _lib.check(lib.egx_crowd_metrics(*clead, _lib.ptr(gs), _lib.ptr(gm), _lib.ptr(ps), gs_host.ctypes.data_as(_lib.c_int_p), len(pg), npairs,
                                         Fmax, 0.3, hold, _lib.ptr(clear), _lib.ptr(mdist), _lib.ptr(plist), st), "egx_crowd_metrics")

    legs = {"motion_full": lambda: motion(True), "motion_plain": lambda: motion(False), "crowd_hold0": lambda: crowd(0), "crowd_hold1": lambda: crowd(1)}
    t = alternate(legs, args.iters, args.warmup)

    # the numpy reference on a part of the same inputs, scaled
    r = args.ref_motions
    rec = {"markers": ms.markers, "pelvis": ms.pelvis, "rotmat": ms.rotmat, "transl": ms.transl}
    t0 = time.perf_counter()
    ref.motion_metrics(rec, ms.frame_src[:ms.motion_start[r]], ms.motion_start[:r + 1], feet_idx, ms.goals[:r], 0.1, 0.0, pene.cpu().numpy(), 40)
    ref_motion_s = (time.perf_counter() - t0) / r * n
    crec = {"markers": cs.markers, "pelvis": cs.pelvis, "rotmat": cs.rotmat, "transl": cs.transl}
    t0 = time.perf_counter()
    ref.crowd_metrics(crec, cs.frame_src, cs.motion_start, pg.start[:2], pg.member, 0.3, False)
    ref_crowd_s = (time.perf_counter() - t0) * len(pg)

    evals = npairs * Fmax * 67 * 67
    record = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "warmup": args.warmup,
              "motion": {"motions": n, "primitives": K, "frames": Ftot, **{k: t[k] for k in ("motion_full", "motion_plain")}},
              "crowd": {"groups": len(pg), "people": args.people, "pairs": npairs, "max_frames": Fmax, "marker_distances": evals,
                        **{k: t[k] for k in ("crowd_hold0", "crowd_hold1")}},
              "numpy_reference_s": {"motion": ref_motion_s, "crowd": ref_crowd_s, "timed_on": {"motions": r, "groups": 1}}}
    row = lambda name, v, extra: f"| {name} | {v['median_us']:.1f} | {v['min_us']:.1f} - {v['max_us']:.1f} | {extra} |"
    mf, mp_, c0, c1 = t["motion_full"], t["motion_plain"], t["crowd_hold0"], t["crowd_hold1"]
    lines = [f"Device: {record['device']}; {args.iters} launches per window, three windows per leg, median (range), microseconds per launch.", "",
             "| launch | median us | range us | per unit |", "|---|---|---|---|",
             row(f"egx_motion_metrics, {n} motions x {K} primitives ({Ftot} frames), goal + pene + per-frame", mf, f"{mf['median_us'] * 1e3 / Ftot:.2f} ns / frame"),
             row("egx_motion_metrics, the same without goal, pene, per-frame", mp_, f"{mp_['median_us'] * 1e3 / Ftot:.2f} ns / frame"),
             row(f"egx_crowd_metrics, {len(pg)} groups x {args.people} people x {K} primitives ({npairs} pairs x {Fmax} frames), hold 0", c0,
                 f"{evals / c0['median_us'] * 1e-3:.1f} G marker distances / s"),
             row("egx_crowd_metrics, the same, hold 1", c1, f"{evals / c1['median_us'] * 1e-3:.1f} G marker distances / s"), "",
             f"numpy float64 reference (tests/motion_metrics_ref.py) on the same box, timed on {r} motions / 1 group and scaled: "
             f"{ref_motion_s:.1f} s for the {n} motions, {ref_crowd_s:.1f} s for the {len(pg)} groups."]
    write_section(args.out_dir, "timings", lines)
    with open(os.path.join(args.out_dir, "motion_metrics.json"), "w") as fh:
        json.dump(record, fh, indent=1)
    print("\n".join(lines))


if __name__ == "__main__":
    main()
