#!/usr/bin/env python3
"""One combo training step (`egogen_amd.train_combo.GAMMAPrimitiveComboTrainOP`) with the fused glue kernels of csrc/combo.hip
against the torch-op composition of the same step (`trainconfig['fused'] = False`), and each kernel family against the ops it
replaces.  GPU only.

    python scripts/bench_combo_train.py [--out-dir profiles] [--iters 30] [--warmup 5] [--batch 32]

Legs alternate in one process; device events around --iters passes after --warmup of them, three repeats; median and range
(min .. max) of the three per-pass times.  Step legs: `calc_loss_one` + backward, and a 3-primitive `calc_loss_rollout` + backward
(57 frames, scheduled sampling, with and without `use_Yproj_as_seed`), at the batch of cfg_samp20/MPVAECombo_samp_2frame.yml (32).
Kernel legs, at the shapes of that step: the 6D tail forward + backward on 18 x batch rows, the marker loss forward + backward on
[18, batch, 201], the re-seeding block for `batch` sequences.  Before timing, the two legs' losses on the same inputs are compared.
Writes `<out-dir>/combo_train.json` and replaces the section between the `timings` markers of `<out-dir>/combo_train.md`."""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from egogen_amd import synth  # noqa: E402
from egogen_amd.fused_ops import Cont6dToAaFn, PrimitiveLossFn, primitive_reseed  # noqa: E402
from egogen_amd.models import PREDICTOR_CFG, REGRESSOR_CFG  # noqa: E402
from egogen_amd.train_combo import GAMMAPrimitiveComboTrainOP, _reseed_torch  # noqa: E402
from egogen_amd.train_regressor import MarkerBodyModel, cont6d_params_to_aa  # noqa: E402

BEGIN, END = "<!-- timings:begin -->", "<!-- timings:end -->"
LOSS_CFG = {"weight_rec": 1.0, "weight_td": 3.0, "weight_kld": 1.0, "weight_reg_hpose": 0.01, "annealing_kld": False, "robust_kld": True}


def make_data(bmd, mids, n_t, nb, seed):
    """Smooth body-consistent sequences: betas[n_t,nb,10], markers[n_t,nb,201], joints[n_t,nb,66] on the device."""
    g = torch.Generator().manual_seed(seed)
    xb = torch.zeros(n_t, nb, 93)
    xb[:, :, :3] = torch.arange(n_t).view(n_t, 1, 1) * torch.tensor([0.0, 0.02, 0.0]) + torch.tensor([0.0, 0.0, 0.9])
    xb[:, :, 3:69] = torch.randn(1, nb, 66, generator=g) * 0.08 + (torch.randn(n_t, nb, 66, generator=g) * 0.02).cumsum(0)
    betas = (torch.randn(1, nb, 10, generator=g) * 0.5).repeat(n_t, 1, 1)
    mbm = MarkerBodyModel(bmd, mids)
    with torch.no_grad():
        markers = mbm(xb.reshape(-1, 93), betas.reshape(-1, 10)).reshape(n_t, nb, 201)
    jts = (torch.randn(1, nb, 22, 3, generator=g) * 0.3 + xb[:, :, None, :3]).reshape(n_t, nb, 66)
    return betas.cuda().contiguous(), markers.cuda().contiguous(), jts.cuda().contiguous()


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
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_combo_train.py measures on the GPU; no device is visible")
    nb = args.batch
    bmd, mids = synth.make_body_model(0), [int(v) for v in synth.marker_ids()]
    one = make_data(bmd, mids, 20, nb, 1)
    roll = make_data(bmd, mids, 57, nb, 2)
    results = {"batch": nb, "iters": args.iters, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
    td = tempfile.mkdtemp()

    def new_op(fused, **kw):
        tc = dict({"log_dir": td, "save_dir": td, "batch_size": nb, "num_epochs": 10, "max_rollout": 8, "fused": fused}, **kw)
        torch.manual_seed(0)
        op = GAMMAPrimitiveComboTrainOP({"modelconfig": PREDICTOR_CFG}, {"modelconfig": dict(REGRESSOR_CFG, gender="male")}, dict(LOSS_CFG), tc)
        op.build_model(body_model=bmd, markers=mids)
        sd = op.model.state_dict()                    # seeded weights at the gains of tests/golden/combo_train_ref.npz: a rollout stays finite
        for prefix, seed, gain in (("predictor.", 520, 0.5), ("regressor.", 521, 0.3)):
            shapes = {k[len(prefix):]: tuple(v.shape) for k, v in sd.items() if k.startswith(prefix)}
            sd.update({prefix + k: torch.from_numpy(v) for k, v in synth.seeded_fill(shapes, seed, gain=gain).items()})
        op.model.load_state_dict(sd)
        op.grads.attach()
        return op

    g = torch.Generator(device="cuda").manual_seed(3)
    eps = torch.randn(3, nb, 128, device="cuda", generator=g)

    def step_leg(op, kind):
        def run():
            op.grads.zero()
            if kind == "one":
                loss, _ = op.calc_loss_one([one[0], one[1]], 0, eps=eps[0])
            else:
                loss, _ = op.calc_loss_rollout([roll[0], roll[1], None, None, None, roll[2]], 0, eps_list=list(eps))
            loss.backward()
            return loss
        return run

    for name, kind, kw in (("calc_loss_one + backward", "one", {}),
                           ("calc_loss_rollout (3 primitives) + backward", "roll", {"scheduled_sampling": True}),
                           ("calc_loss_rollout (3 primitives, use_Yproj_as_seed) + backward", "roll",
                            {"scheduled_sampling": True, "use_Yproj_as_seed": True})):
        legs = {"fused": step_leg(new_op(True, **kw), kind), "torch-op glue": step_leg(new_op(False, **kw), kind)}
        lf, lt = float(legs["fused"]()), float(legs["torch-op glue"]())
        assert np.isfinite(lf) and np.isfinite(lt), (name, lf, lt)
        results[name] = alternate(legs, args.iters, args.warmup)
        results[name]["loss"] = {"fused": lf, "torch-op glue": lt}
        print(name, results[name], flush=True)

    # ---- kernel families at the step's shapes
    n = 18 * nb
    gen = torch.Generator(device="cuda").manual_seed(4)
    xb6 = torch.randn(n, 159, device="cuda", generator=gen)
    cot = torch.randn(n, 93, device="cuda", generator=gen)

    def tail(fn):
        x = xb6.clone().requires_grad_(True)

        def run():
            x.grad = None
            fn(x).backward(cot)
        return run
    results["6D tail forward + backward, %d rows" % n] = alternate({"fused": tail(Cont6dToAaFn.apply), "torch-op glue": tail(cont6d_params_to_aa)},
                                                                   args.iters * 4, args.warmup)
    Y = torch.randn(18, nb, 201, device="cuda", generator=gen)
    Yr0 = Y + 0.05 * torch.randn(18, nb, 201, device="cuda", generator=gen)

    def loss_leg(fused):
        Yr = Yr0.clone().requires_grad_(True)

        def run():
            Yr.grad = None
            if fused:
                loss = PrimitiveLossFn.apply(Y, Yr, 1.0, 3.0)[0]
            else:
                loss = torch.nn.functional.l1_loss(Y, Yr) + 3.0 * torch.nn.functional.l1_loss(Yr[1:] - Yr[:-1], Y[1:] - Y[:-1])
            loss.backward()
        return run
    results["marker loss forward + backward, [18,%d,201]" % nb] = alternate({"fused": loss_leg(True), "torch-op glue": loss_leg(False)},
                                                                            args.iters * 4, args.warmup)
    jts = torch.randn(nb, 55, 3, device="cuda", generator=gen)
    Xp, Yg = torch.randn(2, nb, 201, device="cuda", generator=gen), torch.randn(18, nb, 201, device="cuda", generator=gen)
    yaw = torch.rand(nb, device="cuda", generator=gen) * 6.28
    Rp = torch.zeros(nb, 3, 3, device="cuda")
    Rp[:, 0, 0], Rp[:, 0, 1], Rp[:, 1, 0], Rp[:, 1, 1], Rp[:, 2, 2] = yaw.cos(), -yaw.sin(), yaw.sin(), yaw.cos(), 1.0
    Tp = torch.randn(nb, 1, 3, device="cuda", generator=gen)
    results["re-seeding block, %d sequences" % nb] = alternate({"fused": lambda: primitive_reseed(jts, Xp, Yg, Rp, Tp),
                                                               "torch-op glue": lambda: _reseed_torch(jts, Xp, Yg, Rp, Tp)},
                                                              args.iters * 4, args.warmup)
    for k in list(results)[-3:]:
        print(k, results[k], flush=True)

    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "combo_train.json"), "w") as fh:
        json.dump(results, fh, indent=1)
    lines = [BEGIN, f"Device: {results['device']}; batch {nb}; {args.iters} passes per window (kernel legs: {args.iters * 4}), three windows per leg, "
             "legs alternating.  Microseconds per pass: median (min .. max).", "",
             "| what | fused kernels | torch-op glue | ratio of medians |", "|---|---|---|---|"]
    for k, v in results.items():
        if isinstance(v, dict) and "fused" in v:
            f, t = v["fused"], v["torch-op glue"]
            lines.append(f"| {k} | {f['median_us']:.1f} ({f['min_us']:.1f} .. {f['max_us']:.1f}) | {t['median_us']:.1f} ({t['min_us']:.1f} .. {t['max_us']:.1f}) "
                         f"| {t['median_us'] / f['median_us']:.2f} |")
    lines.append(END)
    md = os.path.join(args.out_dir, "combo_train.md")
    txt = open(md).read() if os.path.exists(md) else "# Combo training\n\n" + BEGIN + "\n" + END + "\n"
    if BEGIN in txt and END in txt:
        txt = txt[:txt.index(BEGIN)] + "\n".join(lines) + txt[txt.index(END) + len(END):]
    else:
        txt += "\n" + "\n".join(lines) + "\n"
    with open(md, "w") as fh:
        fh.write(txt)


if __name__ == "__main__":
    main()
