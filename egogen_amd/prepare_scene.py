"""Bring your own scene: a scanned room mesh (z-up PLY, open triangle soup) -> a scene file `main_ppo.py --scene` trains in, and
optionally the scene directory the EgoBody driver reads (`navmesh_tight.ply` + `mesh_floor_zup.ply`,
`egobody.EgobodySampler.from_scene_dir`).

    python -m egogen_amd.prepare_scene --mesh scan.ply --out my_scene.npz [--scene-dir my_scene/]

The mesh is shifted down by the floor height (detected unless --floor-height is given) so that the floor lies at z = 0, as the
environment assumes; the shift is stored in the npz as `z_offset` and the PLYs under --scene-dir are shifted the same way.
Signed-distance grid and walkable raster run on the GPU (scene_gen.scene_from_scan)."""
from __future__ import annotations

import argparse
import os
import sys
import time
from typing import Optional, Sequence

import numpy as np


def parse_args(argv: Optional[Sequence[str]] = None):
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0], formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--mesh", required=True, help="z-up PLY of the scanned room (ascii or binary little endian)")
    p.add_argument("--out", required=True, help="scene file to write (.npz, scene_gen.save_scene)")
    p.add_argument("--scene-dir", default=None, help="also write navmesh_tight.ply and mesh_floor_zup.ply here")
    p.add_argument("--res", type=int, default=256, help="SDF grid samples per axis")
    p.add_argument("--cell", type=float, default=0.05, help="walkable raster cell [m]")
    p.add_argument("--radius", type=float, default=0.2, help="body radius [m]")
    p.add_argument("--floor-height", type=float, default=None, help="floor height of the input mesh [m] (default: detected)")
    p.add_argument("--flip-normals", action="store_true", help="the scan's normals point into the solids")
    p.add_argument("--pairs", type=int, default=20000, help="start / target pairs to sample")
    p.add_argument("--seed", type=int, default=0)
    return p.parse_args(argv)


def main(argv: Optional[Sequence[str]] = None) -> dict:
    a = parse_args(argv)
    from . import egobody, scene_gen as sg
    t0 = time.perf_counter()
    v, f = egobody.read_ply(a.mesh)
    t_read = time.perf_counter() - t0
    print(f"read {a.mesh}: {len(v)} vertices, {len(f)} triangles ({t_read:.2f} s)")
    scene = sg.scene_from_scan(v, f, res=a.res, cell=a.cell, radius=a.radius, floor_height=a.floor_height,
                               flip_normals=a.flip_normals, n_pairs=a.pairs, seed=a.seed)
    tm = scene["times"]
    area = float(scene["free"].sum()) * scene["cell"] ** 2
    print(f"floor height {scene['z_offset']:.4f} m ({'given' if a.floor_height is not None else 'detected'}; the scene is "
          f"shifted down by it)  [{tm['floor']:.2f} s]")
    print(f"walkable raster {scene['free'].shape[0]} x {scene['free'].shape[1]} cells of {scene['cell']} m: {area:.2f} m^2 free  "
          f"[{tm['raster']:.2f} s]")
    print(f"navmesh, polygon ({len(scene['rings'])} rings), {len(scene['pairs'])} pairs  [{tm['navmesh']:.2f} s]")
    print(f"SDF grid {a.res}^3  [{tm['sdf']:.2f} s]")
    t0 = time.perf_counter()
    out_dir = os.path.dirname(os.path.abspath(a.out))
    os.makedirs(out_dir, exist_ok=True)
    sg.save_scene(a.out, scene, scene["sdf_dict"])
    if a.scene_dir:
        os.makedirs(a.scene_dir, exist_ok=True)
        nv, nf = sg.grid_to_cell_navmesh(scene["free"], scene["origin"], scene["cell"], 0.0)
        sg.write_ply(os.path.join(a.scene_dir, "navmesh_tight.ply"), nv, nf)
        sg.write_ply(os.path.join(a.scene_dir, "mesh_floor_zup.ply"), scene["vertices"], np.asarray(f, np.int64))
    print(f"wrote {a.out}" + (f" and {a.scene_dir}/{{navmesh_tight,mesh_floor_zup}}.ply" if a.scene_dir else "") +
          f"  [{time.perf_counter() - t0:.2f} s]")
    return scene


if __name__ == "__main__":
    main(sys.argv[1:])
