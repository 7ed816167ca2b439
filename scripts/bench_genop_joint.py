#!/usr/bin/env python3
"""The joint step of the greedy primitive search (egx_primitive_select_joint, `generate_sequence_to_goal(groups=)`): what it costs,
and that the entries that existed before did not move.  GPU only.

    python scripts/bench_genop_joint.py [--iters 20] [--out-dir profiles]
    python scripts/bench_genop_joint.py --lib <parent .so> --dump outputs.pt        (once, on the parent build)
    python scripts/bench_genop_joint.py --compare outputs.pt [--out-dir profiles]   (once, on this build)
    python scripts/bench_genop_joint.py --markers [--iters 20] [--out-dir profiles]  (the marker-level pair model)
    python scripts/bench_genop_joint.py [--markers] --lib <parent .so> --save parent.json, then [--markers] --parent parent.json
                                                                                     (both builds side by side, one process each)

Timing, in one process: G groups of P people swap places on a circle of 2 m, N candidates each, S = 2 sweeps, at the driver's shape
(4 variants of 4 people, N = 16) and at 8 groups x 8 people x N = 32.  Device events around --iters passes of the whole primitive
loop (K = 4, body of --num-verts vertices, no scene) with and without `groups`, and around ten times as many single launches of
the selection and of the joint step on the same rows; the legs alternate, three windows per leg after --warmup, median and range.
The joint launch rewrites `choice` in place, so a repeated launch starts from its own last choice; its work does not depend on
that: all sweeps always run over all rows.

Bit identity: `--dump` writes every output of the selection entries that existed before (scripts/bench_genop_obstacles.py's
inputs for egx_primitive_select, _select_field, _beam_select, _beam_select_field, and the obstacle entries on two of the obstacle
tests' constructed cases) and every output of the three joint entries on the first draw of the cases of their kernel tests
(`joint_outputs`); `--compare` recomputes them and compares bit for bit, NaN traces included.
Writes the sections between the `timings` and the `identity` markers of `<out-dir>/genop_joint.md`.

`--markers`: the marker-level pair model (`pair_model="markers"`, csrc/genop_joint_markers.hip) on the same people, at the two shapes
above and at one group of 32 people x N = 16: the primitive loop with the cylinder model and with the marker model, and single
launches of the cylinder joint step, of egx_pair_marker_dist and of egx_primitive_select_joint_markers on the same rows; for the
distance launch also distance evaluations per second (pairs x N^2 x 18 frames x 67 x 67 over the launch time) and what share of
the fp32 vector peak its arithmetic is.  Writes the `cost` section of `<out-dir>/genop_joint_markers.md`."""
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

MARKS = {"timings": ("<!-- timings:begin -->", "<!-- timings:end -->"), "identity": ("<!-- identity:begin -->", "<!-- identity:end -->"),
         "cost": ("<!-- cost:begin -->", "<!-- cost:end -->")}
NEW = ("egx_primitive_select_joint", "egx_pair_marker_dist", "egx_primitive_select_joint_markers")
SHAPES = ((4, 4, 16), (8, 8, 32))       # G, P, N
MARKER_SHAPES = SHAPES + ((1, 32, 16),)
PEAK_FP32_VECTOR = 157.3e12             # FLOP/s, an FMA counted as two: 78.65e12 vector operations a second
OPS_PER_DISTANCE = 9                    # three differences, three squares, two sums, one minimum: none of them fuses
K, S = 4, 2


def use_library(path):
    """every later `_lib.load()` opens `path`; a build from before the joint entry simply lacks its symbol"""
    _lib.LIB_PATH = os.path.abspath(path)
    probe = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        if not hasattr(probe, name):
            _lib.SIGNATURES.pop(name, None)


def write_section(out_dir, which, lines, name="genop_joint.md", title="# The joint primitive search\n"):
    begin, end = MARKS[which]
    md = os.path.join(out_dir, name)
    os.makedirs(out_dir, exist_ok=True)
    txt = open(md).read() if os.path.exists(md) else title
    body = "\n".join([begin] + lines + [end])
    if begin in txt and end in txt:
        txt = txt[:txt.index(begin)] + body + txt[txt.index(end) + len(end):]
    else:
        txt += "\n" + body + "\n"
    with open(md, "w") as fh:
        fh.write(txt)


# ---- bit identity of the entries that existed before -----------------------------------------------------------------------
def existing_outputs():
    from bench_genop_obstacles import existing_outputs as without_obstacles
    from tests import genop_gpu_helpers as gh
    from tests import test_genop_obstacles_gpu as to
    out = without_obstacles()
    from egogen_amd import synth
    from egogen_amd.body_model import BodyModelHandle
    V = gh.V_SMALL
    world = {"handle": BodyModelHandle(synth.make_body_model(0, num_verts=V), synth.marker_ids(V), synth.feet_vids(V))}
    for b, N, O, T, beam in ((3, 5, 2, 19, None), (65, 5, 32, 200, None), (3, 6, 6, 40, (2, 3))):
        x = to._lattice(gh._rows_inputs(world, b, N, 400 + b * 7 + N, True), b, N)
        ob = to._obs(to._tracks(to._pelvis64(x, 127, b, N), b, N, O, T, 3, True, 0, list(range(b))), to.RADIUS, index=list(range(b)), frame0=3)
        for k, v in to._select_obs(x, 127, ob, beam=beam)[0].items():
            out[f"select_obstacles b={b} N={N} O={O} beam={beam} {k}"] = v
    return out


def joint_outputs():
    """every output of the three joint entries on the first draw of each case of their kernel tests"""
    from egogen_amd import synth
    from egogen_amd.body_model import BodyModelHandle
    from tests import genop_gpu_helpers as gh
    from tests import test_genop_joint_gpu as jg
    from tests import test_genop_joint_markers_gpu as mg
    V = gh.V_SMALL
    world = {"handle": BodyModelHandle(synth.make_body_model(0, num_verts=V), synth.marker_ids(V), synth.feet_vids(V))}
    out = {}
    for case, (sizes, N, S, jpb, extra, interleave, mode) in jg.KERNEL_CASES.items():
        c = jg._case(world, sizes, N, 40 + N + len(sizes), jpb, extra, interleave, mode)
        out.update({f"select_joint {case} {k}": v for k, v in jg._joint(c, S).items()})
    for case, (sizes, N, extra, interleave) in mg.DIST_CASES.items():
        d = mg._dist(mg._mcase(world, sizes, N, 60 + N + len(sizes), 127, extra, interleave))
        out.update({f"pair_marker_dist {case} D": d["D"].cpu(), f"pair_marker_dist {case} row_bad": d["bad"].cpu()})
    for case, (sizes, N, S, jpb, extra, interleave, mode) in mg.SWEEP_CASES.items():
        c = mg._mcase(world, sizes, N, 40 + N + len(sizes), jpb, extra, interleave, mode)
        out.update({f"select_joint_markers {case} {k}": v for k, v in mg._sweep(c, S, mg._dist(c)).items()})
    return out


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


# ---- timing ---------------------------------------------------------------------------------------------------------------------
def swap_people(body, G, P, N, g):
    """G groups of P people who swap places on a circle of 2 m -> (data, xb, betas, goal, the keywords z / T0 / R0, groups)"""
    from bench_genop_search import seeds
    b = G * P
    data, xb, betas = seeds(body, b, g)
    z = torch.randn(K, b * N, 128, generator=g).cuda()
    ang = 2 * np.pi * (np.arange(b) % P) / P
    T0 = torch.tensor(np.stack([2.0 * np.cos(ang), 2.0 * np.sin(ang), np.zeros(b)], -1), dtype=torch.float32)
    yaw = ang + np.pi / 2                                         # the seed walks along +y: turned to face the centre
    R0 = torch.tensor(np.stack([np.stack([np.cos(yaw), -np.sin(yaw), 0 * yaw], -1), np.stack([np.sin(yaw), np.cos(yaw), 0 * yaw], -1),
                                np.stack([0 * yaw, 0 * yaw, 1 + 0 * yaw], -1)], 1), dtype=torch.float32)
    return data, xb, betas, -T0 + torch.tensor([0.0, 0.0, 0.9]), dict(z=z, T0=T0, R0=R0, to_numpy=False), np.arange(b) // P


def joint_launches(op, lib, s, k, b, N):
    """single launches of the joint step of a captured loop state s on the rows of primitive k -> {"joint": launch} and, with the
    marker model, {"distance": launch} too"""
    vp = lambda t: C.c_void_p(t.data_ptr())
    st = _lib.current_stream_ptr()
    name, lead, dist = op._joint_lead(s, b, N, st)
    tail = (vp(s["cost"][k]), vp(s["cost_terms"][k]), vp(s["colliding"][k]), b, N, *s["joint"], vp(s["choice"][k]), vp(s["status"][k]),
            vp(s["reached"][k]), vp(s["goal_dist"][k]), vp(s["pair_term"][k]), vp(s["pair_clearance"][k]), vp(s["joint_cost"][k]),
            vp(s["pair_hit"][k]), vp(s["choice_trace"][k]), vp(s["joint_changed"][k]), vp(s["crowd_clearance"][k]), vp(s["crowd_hit"][k]), st)
    out = {"joint": lambda: _lib.check(getattr(lib, name)(*lead, *tail), name)}
    if dist is not None:
        out["distance"] = lambda: _lib.check(lib.egx_pair_marker_dist(*dist), "egx_pair_marker_dist")
    return out


BOUND = 1.03        # a leg's median against the parent build's of the same call; the recorded window ranges of these legs reach about 3 %


def table(args, rows):
    """rows [(shape, leg, {median_us, min_us, max_us})] -> the lines of the table; --save keeps them for a later run, --parent puts
    that run's next to this one's: held where the median is within BOUND of the parent's or inside the parent's own window"""
    import json
    fmt = lambda v: f"{v['median_us']:.1f} ({v['min_us']:.1f} .. {v['max_us']:.1f})"
    if args.save:
        with open(args.save, "w") as fh:
            json.dump(rows, fh)
    if not args.parent:
        return ["| shape | leg | us |", "|---|---|---|"] + [f"| {shape} | {leg} | {fmt(v)} |" for shape, leg, v in rows]
    with open(args.parent) as fh:
        parent = {(shape, leg): v for shape, leg, v in json.load(fh)}
    lines = ["| shape | leg | parent build, us | this build, us | ratio of the medians | held |", "|---|---|---|---|---|---|"]
    for shape, leg, v in rows:
        q = parent[(shape, leg)]
        ok = v["median_us"] <= max(BOUND * q["median_us"], q["max_us"])
        lines.append(f"| {shape} | {leg} | {fmt(q)} | {fmt(v)} | {v['median_us'] / q['median_us']:.3f} | {'yes' if ok else 'NO'} |")
    return lines


def marker_timings(args):
    """the `cost` section of genop_joint_markers.md"""
    from bench_genop import alternate
    from bench_genop_search import build_op, captured
    lib = _lib.load()
    op, body = build_op(args.num_verts)
    g = torch.Generator().manual_seed(1)
    lines = [f"Device: {torch.cuda.get_device_name(0)}; K = {K} primitives, body of {args.num_verts} vertices, no scene, S = {S} sweeps; one "
             f"process, {args.iters} loop passes or {10 * args.iters} launches per window, three windows per leg after {args.warmup} warm-up "
             "passes, the legs taking turns; device events.  Microseconds: median (range of the windows); loops per primitive.", ""]
    rows, notes = [], []
    for G, P, N in MARKER_SHAPES:
        b = G * P
        data, xb, betas, goal, kw, groups = swap_people(body, G, P, N, g)
        run = lambda **more: op.generate_sequence_to_goal(data, xb, betas, goal, K, N, groups=groups, joint_sweeps=S, **kw, **more)
        res = {}
        cyl, sc = captured(op, "_search_loop", lambda: res.update(c=run()))
        mk, sm = captured(op, "_search_loop", lambda: res.update(m=run(pair_model="markers")))
        cylinder, markers = joint_launches(op, lib, sc[3], K - 1, b, N), joint_launches(op, lib, sm[3], K - 1, b, N)
        legs = {"cylinder joint launch": cylinder["joint"], "distance launch": markers["distance"], "sweep launch": markers["joint"]}
        npairs = sm[3]["npairs"]
        t = alternate({"loop, cylinder model": cyl, "loop, marker model": mk}, args.iters, args.warmup)
        for v in t.values():
            for q in ("median_us", "min_us", "max_us"):
                v[q] /= K
        t.update(alternate(legs, 10 * args.iters, args.warmup))
        rows += [(f"G={G} P={P} N={N} (b={b})", name, v) for name, v in t.items()]
        evals = npairs * N * N * 18 * 67 * 67
        rate = evals / (t["distance launch"]["median_us"] * 1e-6)
        rc, rm = res["c"], res["m"]
        notes.append(f"G={G} P={P} N={N}: {npairs} pairs, a table of {npairs * N * N * 72 / 1e6:.2f} MB, {evals / 1e9:.3f} G distance evaluations per "
                     f"launch: {rate / 1e12:.2f} T evaluations/s, {OPS_PER_DISTANCE} vector operations each = "
                     f"{100 * rate * OPS_PER_DISTANCE / (PEAK_FP32_VECTOR / 2):.1f} % of the fp32 vector peak ({PEAK_FP32_VECTOR / 2e12:.2f} T "
                     f"operations/s, an FMA being one; the bound is arithmetic, the launch reads {npairs * N * (N + -(-N // 8)) * 18 * 201 * 8 / 1e6:.1f} "
                     f"MB).  Crowd hits per primitive, cylinder / marker model (each in its own measure): {rc.crowd_hit.sum(1).tolist()} / "
                     f"{rm.crowd_hit.sum(1).tolist()}; members still changing in the last sweep: {rc.joint_changed[:, -1].sum(1).tolist()} / "
                     f"{rm.joint_changed[:, -1].sum(1).tolist()}.")
    lines += table(args, rows) + [""] + notes
    write_section(args.out_dir, "cost", lines, "genop_joint_markers.md", "# The marker-level pair model of the joint search\n")
    print("\n".join(lines))


def timings(args):
    from bench_genop import alternate
    from bench_genop_search import build_op, captured
    lib = _lib.load()
    op, body = build_op(args.num_verts)
    g = torch.Generator().manual_seed(1)
    vp = lambda t: C.c_void_p(t.data_ptr())
    lines = [f"Device: {torch.cuda.get_device_name(0)}; K = {K} primitives, body of {args.num_verts} vertices, no scene, S = {S} sweeps; one "
             f"process, {args.iters} loop passes or {10 * args.iters} launches per window, three windows per leg, the legs taking turns.  "
             "Microseconds: median (range of the windows); loops per primitive.", ""]
    rows, notes = [], []
    for G, P, N in SHAPES:
        b = G * P
        data, xb, betas, goal, kw, groups = swap_people(body, G, P, N, g)
        plain, _ = captured(op, "_search_loop", lambda: op.generate_sequence_to_goal(data, xb, betas, goal, K, N, **kw))
        res = {}
        joint, sf = captured(op, "_search_loop",
                             lambda: res.update(r=op.generate_sequence_to_goal(data, xb, betas, goal, K, N, groups=groups, joint_sweeps=S, **kw)))
        s, st = sf[3], _lib.current_stream_ptr()
        cur, lbs, k = s["xs"][(K - 1) % 2], s["lbs_out"], K - 1
        outs = (vp(s["choice"][k]), vp(s["status"][k]), vp(s["reached"][k]), vp(s["goal_dist"][k]))
        scored = (vp(s["cost"][k]), vp(s["cost_terms"][k]), vp(s["colliding"][k]))
        lead = (_lib.ptr(s["Y_gen"]), vp(cur[0]), vp(cur[1]), 201, _lib.ptr(lbs["joints"]), 127, _lib.ptr(lbs["markers"]), _lib.ptr(s["R0"]),
                _lib.ptr(s["T0"]), None, _lib.ptr(s["goal"]), _lib.ptr(s["feet"]), s["weights"], s["pene_thres"], s["goal_thresh"], s["rf"], b, N)
        launches = {"select launch": lambda: _lib.check(lib.egx_primitive_select(*lead, *outs, *scored, st), "egx_primitive_select"),
                    "joint launch": joint_launches(op, lib, s, k, b, N)["joint"]}
        t = alternate({"loop without groups": plain, "loop with groups": joint}, args.iters, args.warmup)
        for v in t.values():
            for q in ("median_us", "min_us", "max_us"):
                v[q] /= K
        t.update(alternate(launches, 10 * args.iters, args.warmup))
        rows += [(f"G={G} P={P} N={N} (b={b})", name, v) for name, v in t.items()]
        r = res["r"]
        notes.append(f"G={G} P={P} N={N}: members that changed their choice per primitive, first / last sweep: "
                     f"{r.joint_changed[:, 0].sum(1).tolist()} / {r.joint_changed[:, -1].sum(1).tolist()}; crowd hits per primitive "
                     f"{r.crowd_hit.sum(1).tolist()}.")
    lines += table(args, rows) + [""] + notes
    write_section(args.out_dir, "timings", lines)
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--lib", default=None, help="run on this build of libegogen_hip.so instead of the package's")
    ap.add_argument("--dump", default=None)
    ap.add_argument("--compare", default=None)
    ap.add_argument("--markers", action="store_true", help="the marker-level pair model: the cost section of genop_joint_markers.md")
    ap.add_argument("--save", default=None, help="keep the timing table as JSON (on the parent build, with --lib)")
    ap.add_argument("--parent", default=None, help="a table kept by --save on the parent build in the same call: both builds side by side")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--num-verts", type=int, default=None)
    args = ap.parse_args()
    if args.num_verts is None:
        from egogen_amd import synth
        args.num_verts = synth.NUM_VERTS
    if args.lib:
        use_library(args.lib)
    if not torch.cuda.is_available():
        sys.exit("bench_genop_joint.py measures on the GPU; no device is visible")
    if args.dump:
        torch.save({**existing_outputs(), **joint_outputs()}, args.dump)
        print(f"wrote {args.dump}")
    elif args.compare:
        want, got = torch.load(args.compare), {**existing_outputs(), **joint_outputs()}
        differ = sorted(k for k in want if k not in got or not same_bits(want[k], got[k])) + sorted(k for k in got if k not in want)
        lines = [f"{len(want)} outputs of egx_primitive_select, _select_field, _beam_select, _beam_select_field, _select_obstacles and "
                 f"_beam_select_obstacles on the pooled test inputs, and of egx_primitive_select_joint, egx_pair_marker_dist and "
                 f"egx_primitive_select_joint_markers on the first draw of every case of their kernel tests (compared through their int32 "
                 f"view: NaN traces count), dumped by the parent commit's build and recomputed by this one: "
                 + ("every one bit-identical." if not differ else f"{len(differ)} differ: " + "; ".join(differ[:20]) + ".")]
        write_section(args.out_dir, "identity", lines)
        print(lines[0])
        sys.exit(1 if differ else 0)
    elif args.markers:
        marker_timings(args)
    else:
        timings(args)


if __name__ == "__main__":
    main()
