"""Inputs shared by tests/test_motion_metrics_cpu.py and tests/test_motion_metrics_gpu.py: walking-like primitives
(`genop_gpu_helpers._walkers`) posed on the small synthetic body by the CPU oracle in float32, each put through a random world
frame, and the cases built from them.  Everything is made on the CPU, once per process, so the CPU file can assert what the GPU
file relies on: on these seeds the float64 reference has no frame within 1e-9 of a threshold."""
import functools

import numpy as np
import torch

GOAL_THRESH, TOUCH_DIST, BODY_RADIUS, PENE_THRES, FLOOR_Z = 0.1, 0.05, 0.3, 40, 0.013
MARGIN = 1e-9           # a frame closer than this to a threshold is undecided; the cap on such frames is zero

# name -> (primitives per motion, mp_type of every primitive or None, seed): 20 frames (one primitive); 20 / 38 / 272 in one launch
# (unequal lengths, a hand-off inside every stencil, more frames than a workgroup has threads and no multiple of 64); 39 frames (a
# '1-frame' primitive)
MOTION_CASES = {
    "one": ((1,), None, 11),
    "unequal": ((1, 2, 15), None, 12),
    "one_frame": ((2,), ("2-frame", "1-frame"), 13),
}
# name -> (primitives per motion, group id of every motion, seed)
CROWD_CASES = {
    "alone": ((1,), (0,), 21),
    "two": ((1, 2), (0, 0), 22),
    "three": ((1, 2, 15), (0, 0, 0), 23),
    "thirtytwo": ((1,) * 32, (0,) * 32, 24),
    # "three" again (same seed, same primitives: motions 1, 3, 5) dealt between the members of two other groups
    "interleaved": ((1, 1, 2, 2, 1, 15, 2), (1, 0, 2, 0, 1, 0, 2), 23),
}
INTERLEAVED_THREE = (1, 3, 5)


@functools.lru_cache(maxsize=None)
def _body():
    from egogen_amd import synth
    from oracle.smplx_lbs import BodyModel
    from tests.genop_gpu_helpers import V_SMALL
    return BodyModel(synth.make_body_model(0, num_verts=V_SMALL)), torch.as_tensor(synth.marker_ids(V_SMALL)).long()


def primitives(P, seed, spread=None):
    """P walking-like primitives as float32 records, each in a world frame of its own: a random yaw and a translation of up to 7 m
    in x and y (coordinates up to 8 m); with `spread`, translations within that many metres of (5, -4): people close to each other."""
    from oracle.smplx_lbs import smplx_forward
    from tests.genop_gpu_helpers import _walkers
    xb, betas, g = _walkers(P, seed)
    ob, mk = _body()
    v, j = smplx_forward(ob, xb.reshape(P * 20, 93), betas.repeat_interleave(20, 0))
    yaw = (torch.rand(P, generator=g) * 2 - 1) * np.pi
    R = torch.zeros(P, 3, 3)
    R[:, 0, 0], R[:, 0, 1], R[:, 1, 0], R[:, 1, 1], R[:, 2, 2] = torch.cos(yaw), -torch.sin(yaw), torch.sin(yaw), torch.cos(yaw), 1.0
    T = (torch.rand(P, 3, generator=g) * 2 - 1) * torch.tensor([7.0, 7.0, 0.05])
    if spread is not None:
        T = (torch.rand(P, 3, generator=g) * 2 - 1) * torch.tensor([spread, spread, 0.05]) + torch.tensor([5.0, -4.0, 0.0])
    f32 = lambda t: np.ascontiguousarray(t.detach().numpy(), np.float32)
    return {"markers": f32(v[:, mk].reshape(P, 20, 67, 3)), "pelvis": f32(j[:, 0].reshape(P, 20, 3)), "rotmat": f32(R), "transl": f32(T),
            "params": f32(xb), "betas": f32(betas)}


def _world_pelvis(rec, src):
    k, t = src // 20, src % 20
    return rec["rotmat"][k].astype(np.float64) @ rec["pelvis"][k, t].astype(np.float64) + rec["transl"][k].astype(np.float64)


@functools.lru_cache(maxsize=None)
def motion_case(name):
    """-> dict: rec, prims, mp_types, frame_src, motion_start, goal [n,3] float32 (5 cm beside the pelvis of the middle frame: the
    motion comes within goal_thresh), pene_count [P*20] int32 (synthetic, 39 and 40 among them)"""
    from tests import motion_metrics_ref as ref
    prims, types, seed = MOTION_CASES[name]
    P = sum(prims)
    rec = primitives(P, seed)
    frame_src, motion_start = ref.frame_table(prims, types)
    goal = np.stack([_world_pelvis(rec, int(frame_src[(motion_start[i] + motion_start[i + 1]) // 2])) + np.array([0.05, 0.0, 0.0])
                     for i in range(len(prims))]).astype(np.float32)
    rng = np.random.default_rng(seed)
    pene = rng.integers(0, 90, P * 20).astype(np.int32)
    pene[3], pene[4], pene[10] = 39, 40, 41
    return {"rec": rec, "prims": prims, "mp_types": list(types) if types else ["2-frame"] * P, "frame_src": frame_src,
            "motion_start": motion_start, "goal": goal, "pene_count": pene}


@functools.lru_cache(maxsize=None)
def crowd_case(name):
    """-> dict: rec, prims, ids, frame_src, motion_start, group_start, group_member (groups in order of first appearance, members
    ascending: `PersonGroups`' form).  The people of a case stand within 0.6 m of one point, so cylinders overlap and markers touch."""
    from tests import motion_metrics_ref as ref
    prims, ids, seed = CROWD_CASES[name]
    if name == "interleaved":
        three = crowd_case("three")["rec"]
        other = primitives(sum(prims) - 18, seed + 100, spread=0.6)
        take = {1: (0, 1), 3: (1, 3), 5: (3, 18)}       # motion of this case -> primitives of "three"
        chunks, at = {k: [] for k in three}, 0
        for m, n in enumerate(prims):
            src, (a, b) = (three, take[m]) if m in take else (other, (at, at + n))
            at += 0 if m in take else n
            for k in chunks:
                chunks[k].append(src[k][a:b])
        rec = {k: np.concatenate(v, 0) for k, v in chunks.items()}
    else:
        rec = primitives(sum(prims), seed, spread=0.6)
    frame_src, motion_start = ref.frame_table(prims)
    order = list(dict.fromkeys(ids))
    members = [[i for i, v in enumerate(ids) if v == g] for g in order]
    group_start = np.cumsum([0] + [len(m) for m in members]).astype(np.int32)
    group_member = np.asarray([i for m in members for i in m], np.int32)
    return {"rec": rec, "prims": prims, "ids": np.asarray(ids), "frame_src": frame_src, "motion_start": motion_start,
            "group_start": group_start, "group_member": group_member}


@functools.lru_cache(maxsize=None)
def motion_reference(name, with_goal, with_pene):
    from egogen_amd import synth
    from tests import motion_metrics_ref as ref
    c = motion_case(name)
    return ref.motion_metrics(c["rec"], c["frame_src"], c["motion_start"], synth.feet_marker_idx(), c["goal"] if with_goal else None, GOAL_THRESH,
                              FLOOR_Z, c["pene_count"] if with_pene else None, PENE_THRES)


@functools.lru_cache(maxsize=None)
def crowd_reference(name, hold):
    from tests import motion_metrics_ref as ref
    c = crowd_case(name)
    clear, md, pairs = ref.crowd_metrics(c["rec"], c["frame_src"], c["motion_start"], c["group_start"], c["group_member"], BODY_RADIUS, hold)
    summ, margins = ref.summaries(clear, md, TOUCH_DIST)
    return clear, md, pairs, summ, margins


def motion_set(c, goals=None, groups=None):
    from egogen_amd.metrics import MotionSet
    r = c["rec"]
    return MotionSet(r["markers"], r["pelvis"], r["rotmat"], r["transl"], r["params"], r["betas"], np.cumsum((0,) + tuple(c["prims"])),
                     c.get("mp_types", ["2-frame"] * sum(c["prims"])), goals, groups)
