#!/usr/bin/env python3
"""Are the trajectories of VecCrowdEnv / CrowdGroupEnv the same, to the bit, in two trees?

  python scripts/env_digest.py run [cases, default abcdefg] > digests.txt     (in each tree, a fresh process, on the GPU)
  python scripts/env_digest.py compare parent1.txt parent2.txt result.txt    (anywhere; prints a markdown table)

`run` builds small environments (A = 6) from the assets of tests/helpers.build_world, drives them with actions from a seeded CPU
torch.randn and prints, after the reset and after every step, one SHA-256 per field over its raw bytes (for a group: its members'
in order).  The cases cover the paths of crowd_env.py: SDF scene with auto-reset past max_depth (candidate pool), the same under
a captured graph, an SDF set with replace_sdf_scenes, box scenes across a pool refill, injected candidates (all fields / pairs
only), the crowd group and the EgoBody variant.  `compare` takes two runs of the parent and one of the result: a field that
already differs between the parent's two runs is reported as such, every other one must agree in every digest."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("state", "seed", "R0", "T0", "dist", "steps", "wpath", "scene_idx", "reward", "terminated", "rterms",
          "obs_ego", "obs_dist", "obs_time", "choice", "pending", "invalid")
A = 6


def emit(case, tag, envs):
    import torch
    torch.cuda.synchronize()
    for f in FIELDS:
        h = hashlib.sha256()
        for e in envs:
            h.update(getattr(e, f).detach().cpu().contiguous().numpy().tobytes())
        print(f"{case} {tag} {f} {h.hexdigest()}", flush=True)


def emit_value(case, tag, name, t):
    print(f"{case} {tag} {name} {hashlib.sha256(np.ascontiguousarray(t).tobytes()).hexdigest()}", flush=True)


def run(cases="abcdefg"):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import torch
    from helpers import build_world
    from egogen_amd import setup_world as sw, synth
    from egogen_amd.crowd_env import CrowdGroupEnv, VecCrowdEnv
    from egogen_amd.egobody import EgobodySampler

    def actions(seed, n, rows=A):
        g = torch.Generator().manual_seed(seed)
        return [torch.randn(rows, 128, generator=g).cuda() for _ in range(n)]

    def drive(case, env, zs, first=0, **kw):
        for i, z in enumerate(zs):
            env.step(z, **kw)
            emit(case, f"step{first + i}", [env])

    w = build_world(A=A, scene_kind="sdf")
    h, prior, vposer = w["handle"], w["env"].prior, w["env"].vposer
    sdf = dict(sdf_dict=w["scene"], rings=w["rings"], pairs=w["pairs"])

    def sdf_scene(case):                                     # 15 steps pass max_depth = 13: auto-reset and the pool
        env = VecCrowdEnv(A, h, prior, vposer, seed=0, use_graph=case == "b", **sdf)
        env.reset()
        emit(case, "reset", [env])
        drive(case, env, actions(1, 15))

    def sdf_set(case):
        scene = sw.build_scene("boxes:3x2", sdf_res=32, seed=0)
        env = VecCrowdEnv(A, h, prior, vposer, sdf_scenes=scene["sdf_scenes"], seed=0)
        env.reset()
        emit("c", "reset", [env])
        zs = actions(2, 8)
        drive("c", env, zs[:4])
        env.replace_sdf_scenes(scene["scene_factory"](1))
        emit("c", "replaced", [env])
        drive("c", env, zs[4:], first=4)

    def box_pool(case):
        boxes = synth.make_box_scenes(3, 64, seed=7)
        env = VecCrowdEnv(A, h, prior, vposer, scene_kind="box", box_scenes=boxes, seed=0)
        env.reset()
        emit("d", "reset", [env])
        drive("d", env, actions(3, 34))                         # 35 draws: crosses two refills of the pool
        print(f"d end forced_accepts {env.forced_accepts()}", flush=True)

    def injected(case):
        boxes = synth.make_box_scenes(3, 64, seed=7)
        env = VecCrowdEnv(A, h, prior, vposer, scene_kind="box", box_scenes=boxes, seed=0)
        rng = np.random.default_rng(4)
        n = 2 * env.K
        scn = rng.integers(0, len(boxes), (A, n))
        row = rng.integers(0, 64, (A, n))
        pairs = np.stack([[np.asarray(boxes[s]["pairs"][r], np.float32) for s, r in zip(scn[a], row[a])] for a in range(A)])
        yaw = (rng.uniform(-1, 1, (A, n)) * 2 * np.pi * 0.1).astype(np.float32)
        variant = rng.integers(0, len(env.variant_starts), (A, n))
        env.set_candidates(pairs, yaw, variant, scn)
        env.reset()
        emit("e", "injected_all", [env])
        env.reset()
        emit("e", "sampled", [env])
        env.set_candidates(pairs[:, ::-1].copy())               # yaw / variant / scene: whatever the last draw left
        env.reset()
        emit("e", "injected_pairs", [env])
        drive("e", env, actions(5, 2), auto_reset=False)
        env.reset()
        emit("e", "reset", [env])

    def group(case):
        S, G = 2, 4
        t = np.linspace(0.3, 0.3 + 2 * np.pi, G, endpoint=False)
        st = np.zeros((G, S, 2, 3), np.float32)
        for k in range(G):
            for s in range(S):
                st[k, s, 0, :2] = (1.2 + 0.2 * s) * np.cos(t[k]), (1.2 + 0.2 * s) * np.sin(t[k])
                st[k, s, 1, :2] = (1.2 + 0.2 * s) * np.cos(t[(k + 2) % G]), (1.2 + 0.2 * s) * np.sin(t[(k + 2) % G])
        grp = CrowdGroupEnv(S, st, h, prior, vposer, seed=5)
        grp.reset()
        emit("f", "reset", grp.members)
        zs = actions(6, 12 * G, rows=S)
        for i in range(12):
            grp.step(zs[i * G:(i + 1) * G], reset_done=True)
            emit("f", f"step{i}", grp.members)

    def egobody(case):
        S, G = 3, 2
        a = synth.load_assets()
        sampler = EgobodySampler(a["room0_nav_v"], a["room0_nav_f"], [{"poses": a["seed_poses"], "trans": a["seed_trans"]}], seed=11)
        drawn = [sampler.next_body() for _ in range(S)]
        st = np.stack([np.stack([drawn[s][k]["wpath"] for s in range(S)]) for k in range(G)])
        seeds = [[drawn[s][k]["seed"] for s in range(S)] for k in range(G)]
        grp = CrowdGroupEnv(S, st, h, prior, vposer, seed=5, scene_rings=sampler.rings, static_scene=True, agent_seeds=seeds,
                            vp_thresh=14.0, goal_terminates=False)
        grp.reset()
        emit("g", "reset", grp.members)
        zs = actions(7, 6 * G, rows=S)
        for i in range(6):
            grp.step([z * 2.0 for z in zs[i * G:(i + 1) * G]], reset_done=True)
            emit("g", f"step{i}", grp.members)
        emit_value("g", "end", "group_invalid", grp.invalid().cpu().numpy())

    todo = {"a": sdf_scene, "b": sdf_scene, "c": sdf_set, "d": box_pool, "e": injected, "f": group, "g": egobody}
    for case in cases:
        todo[case](case)


def read(path):
    out = {}
    for line in open(path):
        p = line.split()
        if len(p) == 4 and len(p[0]) == 1:
            out[(p[0], p[1], p[2])] = p[3]
    return out


def compare(p1, p2, res):
    p1, p2, res = read(p1), read(p2), read(res)
    bad = 0
    print("| case | digests | fields unstable between two parent runs | parent = result (stable digests) | mismatches |")
    print("|---|---|---|---|---|")
    for case in sorted({k[0] for k in p1}):
        keys = [k for k in p1 if k[0] == case]
        missing = [k for k in keys if k not in p2 or k not in res] + [k for k in res if k[0] == case and k not in p1]
        unstable = sorted({k[2] for k in keys if k not in missing and p1[k] != p2[k]})
        stable = [k for k in keys if k not in missing and p1[k] == p2[k]]
        wrong = [k for k in stable if res[k] != p1[k]]
        bad += len(wrong) + len(missing)
        print(f"| {case} | {len(keys)} | {', '.join(unstable) or 'none'} | {len(stable) - len(wrong)} of {len(stable)} | "
              f"{', '.join('/'.join(k[1:]) for k in (wrong + missing)[:6]) or 'none'} |")
    print(f"\n{bad} digest(s) of the result differ from a stable digest of the parent.")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) in (2, 3) and sys.argv[1] == "run":
        run(*sys.argv[2:])
    elif len(sys.argv) == 5 and sys.argv[1] == "compare":
        sys.exit(compare(*sys.argv[2:]))
    else:
        print(__doc__)
        sys.exit(2)
