"""Stage times of scene preparation from a scan, on the >= 1 M-triangle synthetic room of tests/scan_check.py.

    python scripts/bench_scene_prep.py [--res 256] [--mesh-sdf-slab 16] [--out FILE.json]

Host tables (welding + pseudo-normals + BVH build), the egx_scan_sdf grid, egx_mesh_sdf on the same mesh (brute force; timed on
a slab of `--mesh-sdf-slab` z-planes of the same x-y samples and scaled to the full grid - its cost is exactly linear in the
samples), the 2 cm walkable raster over 10 x 10 m, and the whole prepare_scene command.  Kernels are timed with HIP events."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from egogen_amd import _lib, scene_gen as sg  # noqa: E402
from tests import scan_check as sc  # noqa: E402


def timed(fn, reps=1):
    """Best of `reps` runs after a warm-up, HIP events around the launch [s]."""
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        s = torch.cuda.Event(enable_timing=True)
        t = torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        t.record()
        t.synchronize()
        best = min(best, s.elapsed_time(t))
    return best / 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--mesh-sdf-slab", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = _lib.load()
    rows = {}
    v, f = sc.synthetic_room(spacing=0.0125)
    rows["triangles"] = int(len(f))
    center, half, res = np.array([0.013, -0.021, 1.17]), 3.6, a.res
    t0 = time.perf_counter()
    tb = sg.scan_sdf_tables(v, f)
    rows["host_tables_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    sg.build_bvh(v[f])
    rows["bvh_build_s"] = time.perf_counter() - t0
    dev = {k: torch.from_numpy(tb[k]).cuda().contiguous() for k in ("nodes", "tris", "pn")}
    grid = torch.empty(res, res, res, device="cuda")
    c = (C.c_float * 3)(*[float(x) for x in center])

    def scan():
        _lib.check(lib.egx_scan_sdf(_lib.ptr(dev["nodes"]), tb["levels"], _lib.ptr(dev["tris"]), _lib.ptr(dev["pn"]), len(f),
                                    tb["leaf_size"], c, float(1 / half), res, res, res, _lib.ptr(grid), _lib.current_stream_ptr()),
                   "egx_scan_sdf")
    rows["scan_sdf_kernel_s"] = timed(scan, 3)
    rows["scan_sdf_with_host_tables_s"] = rows["scan_sdf_kernel_s"] + rows["host_tables_s"]
    tris9 = torch.tensor(v[f].reshape(-1, 9), dtype=torch.float32, device="cuda")
    slab = torch.empty(res, res, a.mesh_sdf_slab, device="cuda")

    def brute():
        # same x-y samples, a.mesh_sdf_slab z-planes: egx_mesh_sdf's cost is per sample and triangle
        _lib.check(lib.egx_mesh_sdf(_lib.ptr(tris9), len(f), c, float(1 / half), res, res, a.mesh_sdf_slab, 1, _lib.ptr(slab),
                                    _lib.current_stream_ptr()), "egx_mesh_sdf")
    t_slab = timed(brute, 1)
    rows["mesh_sdf_slab_s"] = t_slab
    rows["mesh_sdf_full_grid_s_scaled"] = t_slab * res / a.mesh_sdf_slab
    rows["speedup_vs_mesh_sdf"] = rows["mesh_sdf_full_grid_s_scaled"] / rows["scan_sdf_with_host_tables_s"]
    # 2 cm raster over 10 x 10 m (the room's floor and walls; the rest of the raster has no support)
    tr = torch.tensor(v[f].reshape(-1, 9), dtype=torch.float32, device="cuda")
    nx = ny = 500
    sup = torch.empty(nx, ny, dtype=torch.int32, device="cuda")
    clr = torch.empty(nx, ny, device="cuda")

    def raster():
        _lib.check(lib.egx_walkable_raster(_lib.ptr(tr), len(f), -5.0, -5.0, 0.02, nx, ny, 0.0, 0.03, float(np.cos(np.radians(15))),
                                           0.05, 2.0, _lib.ptr(sup), _lib.ptr(clr), _lib.current_stream_ptr()), "egx_walkable_raster")
    rows["raster_kernel_s"] = timed(raster, 3)
    with tempfile.TemporaryDirectory() as d:
        sg.write_ply(os.path.join(d, "scan.ply"), v, f)
        t0 = time.perf_counter()
        r = subprocess.run([sys.executable, "-m", "egogen_amd.prepare_scene", "--mesh", os.path.join(d, "scan.ply"), "--out",
                            os.path.join(d, "s.npz"), "--scene-dir", os.path.join(d, "dir"), "--res", str(res), "--cell", "0.02"],
                           cwd=ROOT, capture_output=True, text=True, timeout=600)
        rows["prepare_scene_s"] = time.perf_counter() - t0
        rows["prepare_scene_stdout"] = r.stdout
        if r.returncode != 0:
            print(r.stdout, r.stderr)
            raise SystemExit(r.returncode)
    print(json.dumps(rows, indent=1))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
