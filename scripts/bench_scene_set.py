"""Time the LBS launch (fused kernel + fix-up, between the HIP events egx_profile_next_lbs records, as bench.py does) of 10 240 bodies
(512 agents x 20 frames, V = 10 475, default blend mode) over a SET of SDF scenes against the one-scene launch:
  one_scene          egx_lbs_forward, one scene
  set1               egx_lbs_forward_scenes with a set of one (the general per-body-scene kernels: the A/B of the S = 1 specialisation)
  S{4,8}_block       a set of S scenes, agents in contiguous blocks a -> floor(a S / A)
  S{4,8}_interleaved a set of S scenes, agents' scenes drawn at random
  S{4,8}_separate    S one-scene launches of 10 240 / S bodies each (sum of their times)
Scenes: 256^3 room shells with boxes, different centres / sizes per scene.  Prints one JSON line; --out writes it to a file."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from egogen_amd import _lib, scene_gen, synth  # noqa: E402
from egogen_amd.body_model import BodyModelHandle, SdfScene, SdfSceneSet  # noqa: E402


def make_scene(i, res):
    rng = np.random.default_rng(100 + i)
    c = (float(rng.uniform(-0.5, 0.5)), float(rng.uniform(-0.5, 0.5)), 1.0)
    half = float(rng.uniform(3.5, 4.5))
    room = scene_gen.box_mesh((c[0] - half * 0.9, c[1] - half * 0.9, -0.05), (c[0] + half * 0.9, c[1] + half * 0.9, 2.6))
    boxes = []
    for _ in range(4):
        lo = rng.uniform(-2.5, 2.0, 2)
        boxes.append(scene_gen.box_mesh((lo[0], lo[1], 0.0), (lo[0] + rng.uniform(0.4, 1.2), lo[1] + rng.uniform(0.4, 1.2), rng.uniform(0.4, 1.0))))
    return scene_gen.scene_sdf_dict(room, scene_gen.merge_meshes(boxes), res=res, center=c, half=half)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=512)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    lib = _lib.load()
    A, T = a.agents, a.frames
    B = A * T
    V = 10475
    bm = synth.make_body_model(0, num_verts=V)
    h = BodyModelHandle(bm, synth.marker_ids(V), synth.feet_vids(V))
    g = torch.Generator().manual_seed(0)
    xb = torch.zeros(B, 93)
    xb[:, 2] = 0.9
    xb[:, 3:6] = torch.randn(B, 3, generator=g) * 0.3
    xb[:, 6:69] = torch.randn(B, 63, generator=g) * 0.2
    xb[:, 69:] = torch.randn(B, 24, generator=g) * 0.5
    betas = torch.randn(A, 10, generator=g)
    yaw = torch.rand(A, generator=g) * 6.28
    R0 = torch.zeros(A, 3, 3)
    R0[:, 0, 0], R0[:, 0, 1], R0[:, 1, 0], R0[:, 1, 1], R0[:, 2, 2] = yaw.cos(), -yaw.sin(), yaw.sin(), yaw.cos(), 1.0
    T0 = torch.cat([torch.rand(A, 2, generator=g) * 6 - 3, torch.zeros(A, 1)], -1)
    xb, betas, R0, T0 = xb.cuda(), betas.cuda(), R0.cuda(), T0.cuda()
    scenes = [SdfScene(make_scene(i, a.res)) for i in range(8)]
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        _lib.check(lib.egx_event_create(C.byref(e)), "egx_event_create")

    def timed(call):
        ts = []
        for it in range(a.warmup + a.iters):
            lib.egx_profile_next_lbs(ev[0], ev[1])
            call()
            ms = C.c_float()
            _lib.check(lib.egx_event_elapsed_ms(ev[0], ev[1], C.byref(ms)), "egx_event_elapsed_ms")
            if it >= a.warmup:
                ts.append(ms.value)
        return float(np.median(ts))

    res = {"bodies": B, "agents": A, "frames": T, "grid": a.res, "blend_mode": int(lib.egx_lbs_get_blend_mode()), "ms": {}}
    ms = res["ms"]
    ms["one_scene"] = timed(lambda: h.forward(xb, betas, T, sdf=scenes[0], R0=R0, T0=T0))
    set1 = SdfSceneSet(scenes[:1])
    zeros = torch.zeros(A, dtype=torch.int32, device="cuda")
    ms["set1"] = timed(lambda: h.forward(xb, betas, T, sdf=set1, R0=R0, T0=T0, agent_scene=zeros))
    for S in (4, 8):
        sset = SdfSceneSet(scenes[:S])
        block = (torch.arange(A) * S // A).to(torch.int32).cuda()
        inter = torch.randint(0, S, (A,), generator=g).to(torch.int32).cuda()
        ms[f"S{S}_block"] = timed(lambda: h.forward(xb, betas, T, sdf=sset, R0=R0, T0=T0, agent_scene=block))
        ms[f"S{S}_interleaved"] = timed(lambda: h.forward(xb, betas, T, sdf=sset, R0=R0, T0=T0, agent_scene=inter))
        n = A // S
        tot = 0.0
        for s in range(S):
            sl = slice(s * n * T, (s + 1) * n * T)
            xs, bs, rs, tt = xb[sl].contiguous(), betas[s * n:(s + 1) * n].contiguous(), R0[s * n:(s + 1) * n].contiguous(), T0[s * n:(s + 1) * n].contiguous()
            tot += timed(lambda: h.forward(xs, bs, T, sdf=scenes[s], R0=rs, T0=tt))
        ms[f"S{S}_separate"] = tot
    ms = {k: round(v, 4) for k, v in ms.items()}
    res["ms"] = ms
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    for e in ev:
        lib.egx_event_destroy(e)


if __name__ == "__main__":
    main()
