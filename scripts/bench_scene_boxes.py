#!/usr/bin/env python3
"""Random box scenes on the device (egx_sdf_boxes): kernel time and bytes/s for a 256^3 grid, the wall time of a 64 x 3 scene set
with its bracket tables, and the host builder it replaces.  Writes a markdown table (default profiles/scene_boxes.md) and prints
one JSON line.

    python scripts/bench_scene_boxes.py [--out profiles/scene_boxes.md] [--res 256] [--scenes 64] [--iters 50]

Kernel times are HIP events around one launch, after warm-up launches of the same shape, median of --iters; wall times are host
clocks around work that ends in a device synchronise.  Bytes are what the algorithm needs (one 4-byte store per sample, plus one
4-byte load when composing), over the kernel time."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from egogen_amd import scene_gen as sg  # noqa: E402
from egogen_amd import setup_world as sw  # noqa: E402
from egogen_amd import synth  # noqa: E402
from egogen_amd.body_model import SdfScene, SdfSceneSet  # noqa: E402


def event_times_ms(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return np.array([a.elapsed_time(b) for a, b in ev])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "scene_boxes.md"))
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--scenes", type=int, default=64)
    ap.add_argument("--boxes", type=int, default=3)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_scene_boxes.py measures on the HIP device; there is nothing to report without one")
    res, dims = a.res, (a.res,) * 3
    n = res ** 3
    rng = np.random.default_rng(0)
    rec = {"res": res, "device": torch.cuda.get_device_name(0), "kernel": []}
    base = torch.randn(*dims, device="cuda")
    out = torch.empty(*dims, device="cuda")

    fill = event_times_ms(lambda: out.fill_(1.0), a.warmup, a.iters)
    rec["fill_ms"] = float(np.median(fill))
    for K in (0, 3, 16):
        lay = np.zeros((K, 7))
        lay[:, 0:2] = rng.uniform(-3, 3, (K, 2))
        lay[:, 2:4] = rng.uniform(0.25, 0.75, (K, 2))
        lay[:, 5] = rng.uniform(0.5, 1.5, K)
        lay[:, 6] = rng.uniform(-np.pi, np.pi, K)
        for composed in (False, True):
            if composed:
                fn = lambda: sg.sdf_boxes(lay, sg.ROOM_CENTER, 1.0 / sg.ROOM_HALF, base=base, out=out)
            else:
                fn = lambda: sg.sdf_boxes(lay, sg.ROOM_CENTER, 1.0 / sg.ROOM_HALF, dims, room=(sg.ROOM_LO, sg.ROOM_HI), out=out)
            t = event_times_ms(fn, a.warmup, a.iters)
            nbytes = n * 4 * (2 if composed else 1)
            rec["kernel"].append({"boxes": K, "base": composed, "ms_median": float(np.median(t)), "ms_min": float(t.min()),
                                  "ms_p90": float(np.percentile(t, 90)), "bytes": nbytes, "GBps": nbytes / np.median(t) / 1e6})

    # a scene set: layouts, grids, polygons and pairs (build_scene), then the bracket tables and bricks (SdfScene) and the set
    del base, out
    torch.cuda.synchronize()
    spec = f"boxes:{a.scenes}x{a.boxes}"
    sw.build_scene("boxes:1x1", sdf_res=res, seed=1)   # warm-up: code objects, allocator
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    scene = sw.build_scene(spec, sdf_res=res, seed=0)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    sset = SdfSceneSet([SdfScene(d["sdf_dict"]) for d in scene["sdf_scenes"]])
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    rec["set"] = {"spec": spec, "scenes_s": t1 - t0, "tables_s": t2 - t1, "total_s": t2 - t0, "len": len(sset)}
    # the grids alone (layout + kernel), the part make_sdf_scene's host path corresponds to
    lays = [d["boxes"] for d in scene["sdf_scenes"]]
    del sset, scene
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    grids = [sg.sdf_boxes(l, sg.ROOM_CENTER, 1.0 / sg.ROOM_HALF, dims, room=(sg.ROOM_LO, sg.ROOM_HI)) for l in lays]
    torch.cuda.synchronize()
    rec["set"]["grids_s"] = time.perf_counter() - t0
    del grids

    t0 = time.perf_counter()
    host = synth.make_sdf_scene(res)
    rec["host_make_sdf_scene_s"] = time.perf_counter() - t0
    dev = sg.sdf_boxes(np.array([[1.5, 0.0, 0.5, 0.5, 0.0, 1.0, 0.0]]), sg.ROOM_CENTER, 1.0 / sg.ROOM_HALF, dims, room=(sg.ROOM_LO, sg.ROOM_HI))
    rec["host_vs_device_max_abs"] = float(np.abs(dev.cpu().numpy().astype(np.float64) - host["sdf"]).max())

    mib = n * 4 / 2 ** 20
    L = [f"# Random box scenes on the device: `egx_sdf_boxes`", "",
         f"Measured on one box ({rec['device']}), one run of `scripts/bench_scene_boxes.py`; {res}^3 grid ({mib:.0f} MiB of float32).",
         f"Kernel times: HIP events around one launch, {a.warmup} warm-up launches, median of {a.iters} (min / 90th percentile beside it).",
         "GB/s: the bytes the algorithm needs (4 per sample stored, 4 more per sample loaded when composing) over the median.", "",
         "| boxes | start | median ms | min ms | p90 ms | bytes | GB/s |", "|---|---|---|---|---|---|---|"]
    for k in rec["kernel"]:
        L.append(f"| {k['boxes']} | {'base grid' if k['base'] else 'room box'} | {k['ms_median']:.4f} | {k['ms_min']:.4f} | {k['ms_p90']:.4f} | "
                 f"{k['bytes'] / 2 ** 20:.0f} MiB | {k['GBps']:.0f} |")
    L += ["", f"Plain fill of the same grid (`tensor.fill_`, same events): {rec['fill_ms']:.4f} ms = {n * 4 / rec['fill_ms'] / 1e6:.0f} GB/s.", "",
          "| wall time | s |", "|---|---|",
          f"| `build_scene('{spec}')`: layouts, {a.scenes} grids, polygons, {a.scenes} x 4096 pairs (host) | {rec['set']['scenes_s']:.3f} |",
          f"| bracket tables + bricks of the {a.scenes} scenes (`SdfScene`) and the set (`SdfSceneSet`) | {rec['set']['tables_s']:.3f} |",
          f"| total | {rec['set']['total_s']:.3f} |",
          f"| the {a.scenes} grids alone (`sdf_boxes` calls, one synchronise at the end) | {rec['set']['grids_s']:.4f} |",
          f"| host `synth.make_sdf_scene({res})`, ONE scene, one axis-aligned box (float64 numpy) | {rec['host_make_sdf_scene_s']:.3f} |", "",
          f"Largest difference between the host scene and the device grid of the same box: {rec['host_vs_device_max_abs']:.2e} m."]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(L) + "\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
