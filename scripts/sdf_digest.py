#!/usr/bin/env python3
"""Does every evaluation of the scene SDF give the same bits in two trees?

  python scripts/sdf_digest.py run > digests.txt                              (in each tree, a fresh process, on the GPU)
  python scripts/sdf_digest.py compare parent1.txt parent2.txt result.txt     (anywhere; prints a markdown table)

`run` prints one SHA-256 per output over its raw bytes, for seeded noise grids of 7x5x2 and 37x50x23 samples and a few
thousand points inside the grid, on its faces, outside it and at NaN / inf: egx_sdf_sample and egx_sdf_value_grad (with and
without cotangent) from the row-major grid and from the bricked copy, egx_sdf_penalty_forward / _backward for one grid (both
layouts) and for a scene set of 3 with an out-of-range scene index, and the penetration counts of egx_lbs_forward in blend
modes 1, 2, 3 and of egx_lbs_forward_scenes (2 agents x 3 frames of the 640-vertex synthetic body).  `compare` takes two runs
of the parent and one of the result: an output that already differs between the parent's two runs is reported as such,
every other one must agree."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = ((7, 5, 2), (37, 50, 23))


def emit(grid, name, t):
    import torch
    torch.cuda.synchronize()
    a = np.ascontiguousarray(t.detach().cpu().numpy())
    print(f"{'x'.join(map(str, grid))} {name} {hashlib.sha256(a.tobytes()).hexdigest()}", flush=True)


def sdf_dict(dims, seed):
    rng = np.random.default_rng(seed)
    return {"sdf": rng.normal(0.0, 0.3, dims).astype(np.float32), "center": np.array([0.1, -0.2, 0.9], np.float32) + 0.01 * seed,
            "scale": np.float32(1.0 / 1.5)}


def points(d, n, seed):
    """[n,3] world points: normalised coordinates in [-1.3, 1.3], a fifth of them with coordinates exactly on a face of the cube
    or on the first / last sample plane, and a few NaN / inf rows"""
    rng = np.random.default_rng(seed)
    u = rng.uniform(-1.3, 1.3, (n, 3))
    dims = np.asarray(d["sdf"].shape, np.float64)
    special = np.stack([np.full(3, -1.0), np.full(3, 1.0), -1.0 + 1.0 / dims, 1.0 - 1.0 / dims])          # faces, first / last sample
    pick = rng.integers(0, 4, (n, 3))
    on_face = (rng.uniform(size=(n, 3)) < 0.5) & (np.arange(n)[:, None] % 5 == 0)
    u = np.where(on_face, special[pick, np.arange(3)[None, :]], u)
    p = (d["center"].astype(np.float64) + u / float(d["scale"])).astype(np.float32)
    p[7] = [np.nan, 0.0, 1.0]
    p[8] = [0.0, np.inf, 1.0]
    p[9] = [0.0, 0.0, -np.inf]
    return p


class RowMajor:
    """the scene without its tables: the calls gather from the row-major grid"""

    def __init__(self, scene):
        self.scene = scene

    def __enter__(self):
        self.saved = self.scene.desc.coarse_minmax
        self.scene.desc.coarse_minmax = None
        return self.scene

    def __exit__(self, *exc):
        self.scene.desc.coarse_minmax = self.saved


def run():
    sys.path[:0] = [ROOT]
    import torch
    from egogen_amd import _lib, synth
    from egogen_amd.body_model import BodyModelHandle, SdfScene, SdfSceneSet
    from egogen_amd.scene_sdf import SdfPenalty
    from egogen_amd.utils import calc_sdf
    lib = _lib.load()
    V = 640
    h = BodyModelHandle(synth.make_body_model(0, num_verts=V), synth.marker_ids(V), synth.feet_vids(V))
    g = torch.Generator().manual_seed(3)
    A, T = 2, 3
    xb = torch.randn(A * T, 93, generator=g) * 0.2
    xb[:, 2] += 1.0
    xb, betas = xb.cuda(), torch.randn(A, 10, generator=g).cuda()

    for dims in GRIDS:
        dicts = [sdf_dict(dims, s) for s in range(3)]
        scenes = [SdfScene(d) for d in dicts]
        sset = SdfSceneSet(scenes)
        pts = torch.from_numpy(points(dicts[0], 4 * 256 * 3 + 1, 11)).cuda()
        cot = torch.randn(pts.shape[0], generator=g).cuda()

        def field(tag, scene):
            v = pts[None]
            emit(dims, f"sample_{tag}", calc_sdf(v, scene))
            val, grad = calc_sdf(v, scene, return_gradient=True)
            emit(dims, f"value_grad_{tag}_value", val)
            emit(dims, f"value_grad_{tag}_gradient", grad)
            x = v.clone().requires_grad_(True)
            calc_sdf(x, scene).backward(cot[None])
            emit(dims, f"value_grad_{tag}_cotangent", x.grad)

        def penalty(tag, op, body_pts, **kw):
            for power in (1, 2):
                op.power = power
                x = body_pts.clone().requires_grad_(True)
                pen, cnt = op(x, want_count=True, **kw)
                emit(dims, f"penalty_{tag}_p{power}_penalty", pen)
                emit(dims, f"penalty_{tag}_p{power}_count", cnt)
                pen.backward(torch.linspace(0.5, 2.0, pen.numel(), device="cuda"))
                emit(dims, f"penalty_{tag}_p{power}_backward", x.grad)

        body_pts = torch.from_numpy(points(dicts[0], 4 * 1031, 12).reshape(4, 1031, 3)).cuda()
        w = torch.rand(1031, generator=g)
        w[::7] = 0.0
        field("bricks", scenes[0])
        penalty("bricks", SdfPenalty(scenes[0], weights=w, margin=0.05), body_pts)
        with RowMajor(scenes[0]) as sc:
            field("rowmajor", sc)
            penalty("rowmajor", SdfPenalty(sc, weights=w, margin=0.05), body_pts)
        penalty("set", SdfPenalty(sset, weights=w, margin=0.05), body_pts, agent_scene=torch.tensor([0, 2, 5, 1]))
        penalty("set_fpa2", SdfPenalty(sset, margin=0.0), body_pts, agent_scene=torch.tensor([-1, 2]), frames_per_agent=2)

        old = lib.egx_lbs_get_blend_mode()
        try:
            for mode in (1, 2, 3):
                _lib.check(lib.egx_lbs_set_blend_mode(mode), "egx_lbs_set_blend_mode")
                out = h.forward(xb, betas, T, want_joints=False, want_markers=True, sdf=scenes[0])
                emit(dims, f"lbs_mode{mode}_count", out["pene_count"])
                out = h.forward(xb, betas, T, want_joints=False, want_markers=True, sdf=sset, agent_scene=torch.tensor([1, 7]))
                emit(dims, f"lbs_scenes_mode{mode}_count", out["pene_count"])
        finally:
            _lib.check(lib.egx_lbs_set_blend_mode(old), "egx_lbs_set_blend_mode")
        out = h.forward(xb, betas, T, want_verts=True, sdf=scenes[0])             # the fp32 kernel of vertex-writing calls
        emit(dims, "lbs_verts_count", out["pene_count"])


def read(path):
    out = {}
    for line in open(path):
        p = line.split()
        if len(p) == 3 and len(p[2]) == 64:
            out[(p[0], p[1])] = p[2]
    return out


def compare(p1, p2, res):
    p1, p2, res = read(p1), read(p2), read(res)
    bad = 0
    print("| grid | digests | unstable between two parent runs | parent = result (stable digests) | mismatches |")
    print("|---|---|---|---|---|")
    for grid in sorted({k[0] for k in p1}):
        keys = [k for k in p1 if k[0] == grid]
        missing = [k for k in keys if k not in p2 or k not in res] + [k for k in res if k[0] == grid and k not in p1]
        unstable = sorted(k[1] for k in keys if k not in missing and p1[k] != p2[k])
        stable = [k for k in keys if k not in missing and p1[k] == p2[k]]
        wrong = [k for k in stable if res[k] != p1[k]]
        bad += len(wrong) + len(missing)
        print(f"| {grid} | {len(keys)} | {', '.join(unstable) or 'none'} | {len(stable) - len(wrong)} of {len(stable)} | "
              f"{', '.join(k[1] for k in (wrong + missing)[:6]) or 'none'} |")
    print(f"\n{bad} digest(s) of the result differ from a stable digest of the parent.")
    return 1 if bad or not p1 else 0


if __name__ == "__main__":
    if sys.argv[1:] == ["run"]:
        run()
    elif len(sys.argv) == 5 and sys.argv[1] == "compare":
        sys.exit(compare(*sys.argv[2:]))
    else:
        print(__doc__)
        sys.exit(2)
