#!/usr/bin/env python3
"""The policy as the proposal distribution of the greedy primitive search (`generate_sequence_to_goal(policy=)`, entries
egx_primitive_observe and egx_policy_propose): what it costs per primitive.  GPU only.

    python scripts/bench_genop_policy.py [--iters 20] [--out-dir profiles]
    rocprofv3 --kernel-trace --stats -d <dir> -o run --output-format csv -- python scripts/bench_genop_policy.py --launches-only
    python scripts/bench_genop_policy.py --kernel-stats <dir>/.../run_kernel_stats.csv [--out-dir profiles]

Timing, in one process: b sequences of N candidates walk from inside the room0 polygon towards a goal, K = 4 primitives, body of
--num-verts vertices, no SDF scene, at b x N = 4 x 16 and 64 x 16.  Device events around --iters passes of the whole primitive loop
with and without `policy=` (the yardstick: `policy=None` launches what the search launched before the proposal existed), and around
ten times as many single launches of the selection, the observation, the actor's forward and the proposal on the same rows; the legs
alternate, three windows per leg after --warmup, median and range.  `--launches-only` runs the single launches alone, for a kernel
trace; `--kernel-stats` copies the two new kernels' rows of that trace's statistics into the profile.
Writes `<out-dir>/genop_policy.md` (sections between markers) and `<out-dir>/genop_policy.json`."""
import argparse
import csv
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

MARKS = {"timings": ("<!-- timings:begin -->", "<!-- timings:end -->"), "kernels": ("<!-- kernels:begin -->", "<!-- kernels:end -->")}
SHAPES = ((4, 16), (64, 16))       # b, N
K = 4
KERNELS = ("egx_primitive_observe_kernel", "egx_policy_propose_kernel", "egx_primitive_select")


class PolicyArgs:
    seed = 0; lr = 3e-4; gamma = 0.99; gae_lambda = 0.95; max_grad_norm = 0.1; vf_coef = 1.0; ent_coef = 0.01
    weight_kld = 0; rew_norm = False; eps_clip = 0.1; value_clip = 0; dual_clip = None; norm_adv = 1; recompute_adv = 0
    deterministic_eval = False


def write_section(out_dir, which, lines):
    begin, end = MARKS[which]
    md = os.path.join(out_dir, "genop_policy.md")
    os.makedirs(out_dir, exist_ok=True)
    txt = open(md).read() if os.path.exists(md) else "# The policy as the proposal distribution of the primitive search\n"
    body = "\n".join([begin] + lines + [end])
    if begin in txt and end in txt:
        txt = txt[:txt.index(begin)] + body + txt[txt.index(end) + len(end):]
    else:
        txt += "\n" + body + "\n"
    with open(md, "w") as fh:
        fh.write(txt)


def timings(args):
    from bench_genop import alternate
    from bench_genop_search import build_op, captured, seeds
    from egogen_amd import setup_world as sw, synth
    from egogen_amd.proposal import PolicyProposal
    lib = _lib.load()
    op, body = build_op(args.num_verts)
    policy = sw.build_policy(PolicyArgs())
    room0 = synth.rings_to_edges(synth.room0_polygon()).astype(np.float32)
    prop = PolicyProposal(policy, edges=room0)
    g = torch.Generator().manual_seed(1)
    vp = lambda t: C.c_void_p(t.data_ptr())
    fmt = lambda v: f"{v['median_us']:.1f} ({v['min_us']:.1f} .. {v['max_us']:.1f})"
    lines = [f"Device: {torch.cuda.get_device_name(0)}; K = {K} primitives, body of {args.num_verts} vertices, no SDF scene, the room0 polygon "
             f"(89 edges), defaults of `PolicyProposal`; one process, {args.iters} loop passes or {10 * args.iters} launches per window, three "
             "windows per leg, the legs taking turns.  Microseconds: median (range of the windows); loops per primitive.", "",
             "| shape | leg | us |", "|---|---|---|"]
    record = {"device": torch.cuda.get_device_name(0), "K": K, "num_verts": args.num_verts, "iters": args.iters, "shapes": {}}
    for b, N in SHAPES:
        data, xb, betas = seeds(body, b, g)
        z = torch.randn(K, b * N, 128, generator=g).cuda()
        T0 = torch.tensor([4.18, 1.73, 0.0]).repeat(b, 1) + torch.randn(b, 3, generator=g) * torch.tensor([0.05, 0.05, 0.0])   # inside room0
        goal = T0 + torch.tensor([0.5, 2.0, 0.9])
        kw = dict(z=z, T0=T0, to_numpy=False)
        legs = {}

        def fresh(loop, state):
            # the proposal rewrites z in place, so a repeated loop would propose round its own last candidates: both legs start every
            # pass from the same draws (one device copy each, so the legs stay comparable)
            def run():
                state["z"].copy_(z)
                loop()
            return run
        if not args.launches_only:
            plain, pf = captured(op, "_search_loop", lambda: op.generate_sequence_to_goal(data, xb, betas, goal, K, N, **kw))
            legs["loop, policy=None"] = fresh(plain, pf[3])
        with_policy, sf = captured(op, "_search_loop", lambda: op.generate_sequence_to_goal(data, xb, betas, goal, K, N, policy=prop, **kw))
        legs["loop, policy="] = fresh(with_policy, sf[3])
        s, st, k = sf[3], _lib.current_stream_ptr(), K - 1
        cur, lbs = s["xs"][k % 2], s["lbs_out"]
        outs = (vp(s["choice"][k]), vp(s["status"][k]), vp(s["reached"][k]), vp(s["goal_dist"][k]))
        rows = (vp(s["cost"][k]), vp(s["cost_terms"][k]), vp(s["colliding"][k]))
        lead = (_lib.ptr(s["Y_gen"]), vp(cur[0]), vp(cur[1]), 201, _lib.ptr(lbs["joints"]), 127, _lib.ptr(lbs["markers"]), _lib.ptr(s["R0"]),
                _lib.ptr(s["T0"]), None, _lib.ptr(s["goal"]), _lib.ptr(s["feet"]), s["weights"], s["pene_thres"], s["goal_thresh"], s["rf"], b, N)
        obs = {"state": s["obs_state"][k], "egosensing": s["obs_egosensing"][k], "dist": s["obs_dist"][k], "time": s["obs_time"][k]}
        out = {"mu": s["policy_mu"][k], "logvar": s["policy_logvar"][k]}
        n_mean, n_policy = s["policy_counts"]
        scratch = s["z"][k].clone()

        def observe():
            _lib.check(lib.egx_primitive_observe(_lib.ptr(lbs["joints"]), 20, 18, vp(s["choice"][k - 1]), N, vp(s["rotmat"][k - 1]),
                                                 vp(s["transl"][k - 1]), _lib.ptr(s["R0"]), _lib.ptr(s["T0"]), vp(cur[0]), vp(cur[1]), 201,
                                                 _lib.ptr(s["goal"]), *s["policy_poly"], prop.ray_len, k, prop.max_depth, b, vp(obs["state"]),
                                                 vp(obs["egosensing"]), vp(obs["dist"]), vp(obs["time"]), st), "egx_primitive_observe")
        launches = {"select launch": lambda: _lib.check(lib.egx_primitive_select(*lead, *outs, *rows, st), "egx_primitive_select"),
                    "observe launch": observe,
                    "actor forward (egx_policy_forward)": lambda: prop.runner.forward(obs, want_actor=True, want_critic=False, out=out),
                    "propose launch": lambda: _lib.check(lib.egx_policy_propose(vp(out["mu"]), vp(out["logvar"]), vp(scratch), prop.min_logvar,
                                                                                prop.max_logvar, b, N, n_mean, n_policy, prop.temperature,
                                                                                vp(scratch), st), "egx_policy_propose")}
        if args.launches_only:
            for fn in launches.values():
                for _ in range(10 * args.iters):
                    fn()
            torch.cuda.synchronize()
            continue
        t = alternate(legs, args.iters, args.warmup)
        for v in t.values():
            for q in ("median_us", "min_us", "max_us"):
                v[q] /= K
        t.update(alternate(launches, 10 * args.iters, args.warmup))
        for name, v in t.items():
            lines.append(f"| b={b} N={N} | {name} | {fmt(v)} |")
        d = t["loop, policy="]["median_us"] - t["loop, policy=None"]["median_us"]
        lines.append(f"| b={b} N={N} | the proposal per primitive (difference of the loop medians) | {d:.1f} |")
        record["shapes"][f"b={b} N={N}"] = dict(t, proposal_per_primitive_us=d)
    if args.launches_only:
        print("launches done")
        return
    write_section(args.out_dir, "timings", lines)
    with open(os.path.join(args.out_dir, "genop_policy.json"), "w") as fh:
        json.dump(record, fh, indent=1)
    print("\n".join(lines))


def kernel_stats(args):
    rows = []
    with open(args.kernel_stats) as fh:
        for r in csv.DictReader(fh):
            if any(k in r.get("Name", "") for k in KERNELS):
                rows.append(r)
    lines = ["Kernel times of a separate `rocprofv3 --kernel-trace --stats` run of `--launches-only` (both shapes pooled; nanoseconds).", "",
             "| kernel | calls | average ns | min ns | max ns |", "|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| `{r['Name'][:90]}` | {r['Calls']} | {float(r['AverageNs']):.0f} | {r['MinNs']} | {r['MaxNs']} |")
    write_section(args.out_dir, "kernels", lines)
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--num-verts", type=int, default=None)
    ap.add_argument("--launches-only", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    args = ap.parse_args()
    if args.kernel_stats:
        return kernel_stats(args)
    if args.num_verts is None:
        from egogen_amd import synth
        args.num_verts = synth.NUM_VERTS
    if not torch.cuda.is_available():
        sys.exit("bench_genop_policy.py measures on the GPU; no device is visible")
    timings(args)


if __name__ == "__main__":
    main()
