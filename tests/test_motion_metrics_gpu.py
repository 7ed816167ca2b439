"""The motion evaluator on the device: entries egx_motion_metrics / egx_crowd_metrics (csrc/motion_metrics.hip), `motion_metrics` /
`crowd_metrics` (egogen_amd/metrics.py) and the driver exp_GAMMAPrimitive/eval_motion.py, against the numpy float64 restatement
tests/motion_metrics_ref.py on the inputs of tests/motion_metrics_inputs.py (made on the CPU, shared with the CPU file, which
asserts that no reference frame lies within 1e-9 of a threshold on these seeds).

The bound.  Float outputs: |got - ref| <= 1e-10 * scale, scale the largest magnitude that enters the quantity: max |world
coordinate| for lengths, x 20 for speeds, x 1600 for acc_mean, x 64000 for jerk_mean, 1 for contact_score (and for duration_s and
pene_mean, whose only roundings are one division).  Derivation: 2^-53 = 1.1e-16, times at most 272 summands, times a few tens of
roundings each, is about 1e-12; two orders are left for the device's exp / sqrt and FMA contraction.  A kernel that does any step
in float32 misses by about 1e-7 * scale, three orders on the other side.  Integer outputs must be equal; the cap on undecided
frames is zero.  The worst ratio err / bound per column is printed (profiles/motion_metrics.md records a run).

Measured on an MI355X (worst ratio over all cases): see profiles/motion_metrics.md."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import motion_metrics_inputs as mi
from tests.genop_gpu_helpers import CFG_RF, ROOT, V_SMALL, W_TEST, emit, search_world, small_world  # noqa: F401

pytestmark = pytest.mark.gpu

TOL = 1e-10
SCALE = {"duration_s": 0, "skate_mean": 20, "skate_speed_mean": 20, "skate_speed_max": 20, "floor_mean": 1, "floor_min": 1, "floor_max": 1,
         "contact_score": 0, "path_length": 1, "displacement": 1, "speed_mean": 20, "acc_mean": 1600, "jerk_mean": 64000,
         "goal_dist_end": 1, "goal_dist_min": 1, "pene_mean": 0}        # multiples of max |coordinate|; 0: the scale is 1
FRAME_SCALE = (20, 1, 0, 1, 1, 1)                                       # s, h, c, d, pelvis x, pelvis y


def _max_coordinate(rec, goal=None):
    R, T = rec["rotmat"].astype(np.float64), rec["transl"].astype(np.float64)
    w = np.einsum("kij,ktmj->ktmi", R, rec["markers"].astype(np.float64)) + T[:, None, None]
    p = np.einsum("kij,ktj->kti", R, rec["pelvis"].astype(np.float64)) + T[:, None]
    m = max(float(np.abs(w).max()), float(np.abs(p).max()))
    return m if goal is None else max(m, float(np.abs(goal).max()))


def _held(what, name, got, want, scale):
    """NaN exactly where the reference has NaN; elsewhere within TOL * scale -> the ratio err / bound"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, name, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, name)
    ok = ~np.isnan(want)
    if not ok.any():
        return 0.0
    inf = np.isinf(want) & ok
    assert np.array_equal(got[inf], want[inf]), (what, name)
    ok &= ~inf
    err = float(np.abs(got[ok] - want[ok]).max()) if ok.any() else 0.0
    ratio = err / (TOL * scale)
    emit(f"| {what} | {name} | {err:.3e} | {TOL * scale:.3e} | {ratio:.2e} |")
    assert err <= TOL * scale, (what, name, err, TOL * scale)
    return ratio


def _launch_motion(c, with_goal, with_pene, per_frame):
    from egogen_amd import metrics
    ms = mi.motion_set(c, goals=c["goal"])
    pene = torch.from_numpy(c["pene_count"]).cuda() if with_pene else None
    of, oi, pf = metrics.launch_motion_metrics(ms, mi.GOAL_THRESH, mi.FLOOR_Z, pene, mi.PENE_THRES, per_frame, use_goals=with_goal)
    torch.cuda.synchronize()
    out = {k: of[:, j].cpu().numpy() for j, k in enumerate(metrics.F64_COLUMNS)}
    out.update({k: oi[:, j].cpu().numpy() for j, k in enumerate(metrics.I32_COLUMNS)})
    return out, None if pf is None else pf.cpu().numpy(), (of, oi, pf)


@pytest.mark.parametrize("with_goal,with_pene,per_frame", [(True, True, True), (False, False, False), (True, False, False), (False, True, True)])
@pytest.mark.parametrize("name", list(mi.MOTION_CASES))
def test_motion_kernel_against_reference(name, with_goal, with_pene, per_frame):
    from egogen_amd import metrics
    c = mi.motion_case(name)
    want, want_pf, _ = mi.motion_reference(name, with_goal, with_pene)
    got, got_pf, _ = _launch_motion(c, with_goal, with_pene, per_frame)
    coord = _max_coordinate(c["rec"], c["goal"] if with_goal else None)
    assert coord < 10.0
    what = f"motion {name} goal={int(with_goal)} pene={int(with_pene)}"
    for k in metrics.F64_COLUMNS:
        _held(what, k, got[k], want[k], SCALE[k] * coord if SCALE[k] else 1.0)
    for k in metrics.I32_COLUMNS:
        assert np.array_equal(got[k], want[k]), (what, k, got[k], want[k])
    assert (got_pf is None) == (not per_frame)
    if per_frame:
        for j, k in enumerate(metrics.FRAME_COLUMNS):
            _held(what, "frame " + k, got_pf[:, j], want_pf[:, j], FRAME_SCALE[j] * coord if FRAME_SCALE[j] else 1.0)


def _launch_crowd(c, hold, groups=None):
    from egogen_amd import metrics
    from egogen_amd.crowd import PersonGroups
    ms = mi.motion_set(c)
    pg = PersonGroups.from_ids(c["ids"] if groups is None else groups, len(ms))
    assert np.array_equal(pg.start, c["group_start"]) and np.array_equal(pg.member, c["group_member"])
    clear, md, plist, _ = metrics.launch_crowd_metrics(ms, pg, mi.BODY_RADIUS, hold)
    torch.cuda.synchronize()
    return clear, md, plist


@pytest.mark.parametrize("hold", [False, True])
@pytest.mark.parametrize("name", list(mi.CROWD_CASES))
def test_crowd_kernel_against_reference(name, hold):
    from egogen_amd import metrics
    c = mi.crowd_case(name)
    want_c, want_m, want_pairs, want_s, _ = mi.crowd_reference(name, hold)
    clear, md, plist = _launch_crowd(c, hold)
    coord = _max_coordinate(c["rec"])
    what = f"crowd {name} hold={int(hold)}"
    assert clear.shape == want_c.shape and md.shape == want_m.shape and plist.shape == (len(want_pairs), 2)
    assert clear.dtype == torch.float64 and plist.dtype == torch.int32
    assert np.array_equal(plist.cpu().numpy(), want_pairs), what
    _held(what, "clearance", clear.cpu().numpy(), want_c, coord)
    _held(what, "marker_dist", md.cpu().numpy(), want_m, coord)
    # the host layer: summaries per pair, per person and per group are exact reductions of the reference's arrays
    res = metrics.crowd_metrics(mi.motion_set(c, groups=c["ids"]), body_radius=mi.BODY_RADIUS, touch_dist=mi.TOUCH_DIST, hold=hold)
    assert np.array_equal(res["clearance"], clear.cpu().numpy(), equal_nan=True) and np.array_equal(res["pair"]["i"], want_pairs[:, 0])
    for k in ("overlap_frames", "touch_frames", "frames_compared"):
        assert np.array_equal(res["pair"][k], want_s[k]), (what, k)
    for k in ("clearance_min", "marker_dist_min"):
        _held(what, "pair " + k, res["pair"][k], want_s[k], coord)
    n, ids = len(c["prims"]), c["ids"]
    inf_c, inf_m = np.where(np.isnan(want_c), np.inf, want_c), np.where(np.isnan(want_m), np.inf, want_m)
    person_c, person_m = np.full(n, np.inf), np.full(n, np.inf)
    for i in range(n):
        mine = [q for q in range(len(want_pairs)) if i in want_pairs[q]]
        cf = np.min(inf_c[mine], 0) if mine else np.full(want_c.shape[1], np.inf)
        mf = np.min(inf_m[mine], 0) if mine else np.full(want_c.shape[1], np.inf)
        assert res["person"]["overlap_frames"][i] == (cf < 0).sum() and res["person"]["touch_frames"][i] == (mf < mi.TOUCH_DIST).sum(), (what, i)
        person_c[i], person_m[i] = cf.min(), mf.min()
    _held(what, "person clearance_min", res["person"]["clearance_min"], person_c, coord)
    _held(what, "person marker_dist_min", res["person"]["marker_dist_min"], person_m, coord)
    order = list(dict.fromkeys(ids.tolist()))
    assert res["group"]["id"].tolist() == order and res["group"]["size"].tolist() == [int((ids == g).sum()) for g in order]
    for g, gid in enumerate(order):
        mine = [q for q in range(len(want_pairs)) if ids[want_pairs[q, 0]] == gid]
        cf = np.min(inf_c[mine], 0) if mine else np.full(want_c.shape[1], np.inf)
        assert res["group"]["frames_compared"][g] == np.isfinite(cf).sum() and res["group"]["overlap_frames"][g] == (cf < 0).sum(), (what, g)
    if name == "alone":
        assert clear.shape == (0, 20) and res["group"]["frames_compared"].tolist() == [0] and res["person"]["clearance_min"].tolist() == [np.inf]


def test_group_does_not_depend_on_batch():
    """the group of three evaluated alone and dealt between two other groups: the same bits"""
    alone = [t.cpu().numpy() for t in _launch_crowd(mi.crowd_case("three"), True)]
    c = mi.crowd_case("interleaved")
    mixed = [t.cpu().numpy() for t in _launch_crowd(c, True)]
    rows = [q for q in range(len(mixed[2])) if mixed[2][q, 0] in mi.INTERLEAVED_THREE]
    assert len(rows) == 3 and mixed[2][rows].tolist() == [[1, 3], [1, 5], [3, 5]] and alone[2].tolist() == [[0, 1], [0, 2], [1, 2]]
    for j in (0, 1):
        assert alone[j].shape == (3, 272) and np.isfinite(alone[j]).all()
        assert np.array_equal(alone[j].view(np.int64), mixed[j][rows].view(np.int64))
    for hold in (False,):
        a, m = _launch_crowd(mi.crowd_case("three"), hold), _launch_crowd(c, hold)
        assert torch.equal(a[1].view(torch.int64), m[1][rows].view(torch.int64))


def test_both_entries_are_deterministic():
    c = mi.motion_case("unequal")
    a, b = _launch_motion(c, True, True, True)[2], _launch_motion(c, True, True, True)[2]
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x, y.view(torch.int64) if y.dtype == torch.float64 else y)
    for name in ("three", "thirtytwo"):
        p, q = _launch_crowd(mi.crowd_case(name), True), _launch_crowd(mi.crowd_case(name), True)
        for x, y in zip(p[:2], q[:2]):
            assert torch.equal(x.view(torch.int64), y.view(torch.int64)), name
    # the same motion in another batch: motion 2 of "unequal" measured alone
    from egogen_amd import metrics
    r = {k: v[3:] for k, v in c["rec"].items()}
    alone = metrics.MotionSet(r["markers"], r["pelvis"], r["rotmat"], r["transl"], r["params"], r["betas"], [0, 15], ["2-frame"] * 15, c["goal"][2:])
    of, oi, _ = metrics.launch_motion_metrics(alone, mi.GOAL_THRESH, mi.FLOOR_Z, torch.from_numpy(c["pene_count"][60:]).cuda(), mi.PENE_THRES, False)
    assert torch.equal(of[0].view(torch.int64), a[0][2].view(torch.int64)) and torch.equal(oi[0], a[1][2])


def test_evaluator_agrees_with_the_search(search_world):
    """b = 4 as two groups of two, N = 4, K = 2: the evaluator's minimum clearance over the 18 predicted frames of primitive k is the
    search's crowd_clearance[k, m] within 1e-5 m, the figure tests/test_genop_joint_gpu.py uses for the same quantity recomputed
    from the float32 records"""
    from egogen_amd import metrics
    w, K, N = search_world, 2, 4
    T0 = torch.tensor([[0.0, 0.0, 0.0], [0.8, 0.0, 0.0], [3.0, 0.0, 0.0], [3.8, 0.0, 0.0]])
    four = lambda t, dim: torch.cat([t, t.narrow(dim, 0, 1)], dim)
    z = torch.randn(3, 4 * N, 128, generator=torch.Generator().manual_seed(91))[:K]
    res = w["op"].generate_sequence_to_goal(four(w["data"], 1), four(w["bparams"], 1), four(w["betas"], 0), four(w["goal"], 0) + T0, K, N, z=z,
                                            reproj_factor=CFG_RF, weights=W_TEST, goal_thresh=0.0, to_numpy=False, T0=T0, groups=[0, 0, 1, 1])
    ms = metrics.MotionSet.from_sequences(res)
    assert ms.groups.tolist() == [0, 0, 1, 1] and ms.frames.tolist() == [38] * 4 and np.array_equal(ms.goals, res.goal.cpu().numpy())
    crowd = metrics.crowd_metrics(ms, body_radius=0.3)
    assert crowd["pair"]["i"].tolist() == [0, 2] and crowd["pair"]["j"].tolist() == [1, 3] and crowd["clearance"].shape == (2, 38)
    for k in range(K):
        per_primitive = crowd["clearance"][:, 18 * k + 2:18 * k + 20].min(1)
        for m in range(4):
            assert abs(float(res.crowd_clearance[k, m]) - per_primitive[m // 2]) < 1e-5, (k, m)
    assert np.isfinite(crowd["marker_dist"]).all() and (crowd["marker_dist"] > 0).all()
    per =metrics.motion_metrics(ms, goal_thresh=0.1)
    assert per["frames"].tolist() == [38] * 4 and np.isfinite(per["jerk_mean"]).all()
    for m in range(4):          # the search's goal distance of the last primitive is the evaluator's on the last frame
        assert abs(float(res.goal_dist[K - 1, m]) - per["goal_dist_end"][m]) < 1e-5, m


def test_penetration_plumbing(small_world):
    from egogen_amd import metrics, synth
    from egogen_amd.body_model import SdfScene
    h = small_world["handle"]
    c = dict(mi.motion_case("unequal"))
    P = sum(c["prims"])
    spots = np.array([[-1.0, -1.0, 0.0], [1.5, -0.2, 0.0], [1.5, -0.75, 0.0]], np.float32)      # beside the box, inside, at its edge
    c["rec"] = dict(c["rec"], transl=spots[np.arange(P) % 3].copy())
    ms = mi.motion_set(c, goals=c["goal"])
    scene = SdfScene(synth.make_sdf_scene(32))                                                  # box x 1..2, y -0.5..0.5, z 0..1
    res = metrics.motion_metrics(ms, scene=scene, body_model=h, pene_thres=3)
    d ={k: torch.from_numpy(c["rec"][k]).cuda() for k in ("params", "betas", "rotmat", "transl")}
    direct = h.forward(d["params"].reshape(P * 20, 93), d["betas"], 20, want_verts=False, sdf=scene, R0=d["rotmat"], T0=d["transl"])["pene_count"]
    cnt = direct.cpu().numpy()
    assert np.array_equal(res["pene_count"], cnt) and cnt.max() > 3 and len(np.unique(cnt)) > 1, (cnt.min(), cnt.max())
    for i in range(len(ms)):
        mine = cnt[c["frame_src"][c["motion_start"][i]:c["motion_start"][i + 1]]]
        assert res["pene_max"][i] == mine.max() and res["pene_frames"][i] == (mine >= 3).sum()
        assert abs(res["pene_mean"][i] - mine.astype(np.float64).mean()) < 1e-12
    with pytest.raises(ValueError):
        metrics.motion_metrics(ms, scene=scene)
    # more primitives than one body-model launch takes: the chunks are stitched in order
    old = metrics.LBS_CHUNK
    metrics.LBS_CHUNK = 7
    try:
        assert np.array_equal(metrics.pene_counts(ms, scene, h).cpu().numpy(), cnt)
    finally:
        metrics.LBS_CHUNK = old


def test_entries_reject_bad_arguments():
    """Rejected before anything is launched: every device pointer may therefore be the same scratch buffer."""
    from egogen_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(16384, device="cuda")
    p = C.c_void_p(buf.data_ptr())
    ip = lambda *v: (C.c_int32 * len(v))(*v)
    feet = ip(0, 1, 2, 3, 4, 5)

    def motion(ptrs=(p,) * 8, P=1, F=20, start=ip(0, 20), n=1, feet=feet, thresh=0.1, floor=0.0, pene_thres=40, outs=(p, p)):
        return lib.egx_motion_metrics(*ptrs[:4], P, ptrs[4], F, ptrs[5], start, n, feet, ptrs[6], thresh, floor, ptrs[7], pene_thres, *outs, None,
                                      _lib.current_stream_ptr())
    nulls = [tuple(None if j == k else p for j in range(8)) for k in range(6)]
    bad = [{"ptrs": t} for t in nulls] + [{"start": None}, {"feet": None}, {"outs": (None, p)}, {"outs": (p, None)}, {"P": 0}, {"F": 0}, {"n": 0},
                                          {"start": ip(0, 3), "F": 3}, {"start": ip(0, 20, 23), "n": 2, "F": 23}, {"start": ip(0, 21)},
                                          {"start": ip(-1, 20)}, {"start": ip(20, 0)}, {"feet": ip(0, 1, 2, 3, 4, 67)}, {"feet": ip(-1, 1, 2, 3, 4, 5)},
                                          {"thresh": -0.1}, {"thresh": float("nan")}, {"floor": float("inf")}, {"pene_thres": -1}]
    for kw in bad:
        assert motion(**kw) == -1, kw
        with pytest.raises(_lib.EgxError):
            _lib.check(motion(**kw), "egx_motion_metrics")

    def crowd(ptrs=(p,) * 9, start=ip(0, 20, 40), n=2, gs=ip(0, 2), G=1, npairs=1, Fmax=20, radius=0.3, hold=0, outs=(p, p, p)):
        return lib.egx_crowd_metrics(*ptrs[:4], 2, ptrs[4], 40, ptrs[5], start, n, ptrs[6], ptrs[7], ptrs[8], gs, G, npairs, Fmax, radius, hold,
                                     *outs, _lib.current_stream_ptr())
    nulls = [tuple(None if j == k else p for j in range(9)) for k in range(9)]
    bad = [{"ptrs": t} for t in nulls] + [{"start": None}, {"gs": None}, {"outs": (None, p, p)}, {"outs": (p, None, p)}, {"outs": (p, p, None)},
                                          {"gs": ip(0, 33), "npairs": 528}, {"gs": ip(0, 2), "npairs": 2}, {"gs": ip(1, 2)}, {"gs": ip(2, 0)}, {"G": 0},
                                          {"radius": -0.1}, {"radius": float("nan")}, {"hold": 2}, {"hold": -1}, {"Fmax": 19},
                                          {"start": ip(0, 20, 20)}, {"start": ip(0, 20, 41)}]
    for kw in bad:
        assert crowd(**kw) == -1, kw
        with pytest.raises(_lib.EgxError):
            _lib.check(crowd(**kw), "egx_crowd_metrics")
    assert crowd(gs=ip(0, 1, 2), G=2, npairs=0, outs=(None, None, None)) == 0          # nobody to compare: nothing to launch, no error
    torch.cuda.synchronize()
    assert not buf.any()                                                                # nothing was launched


def test_eval_motion_driver(tmp_path):
    """eval_motion.py on what gen_motion.py --people wrote: 4 file rows, 2 group rows, the values those of direct calls"""
    from egogen_amd import metrics
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = tmp_path / "crowd"
    gen = [sys.executable, os.path.join(ROOT, "exp_GAMMAPrimitive", "gen_motion.py"), "--n-primitives", "2", "--seed", "3", "--num-verts", str(V_SMALL),
           "--n-gens", "2", "--n-candidates", "4", "--people", "0,0,0:0.3,3,0.9;0.8,0,0:0.5,3,0.9", "--out", str(out)]
    r = subprocess.run(gen, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    js = tmp_path / "metrics.json"
    ev = [sys.executable, os.path.join(ROOT, "exp_GAMMAPrimitive", "eval_motion.py"), "--in", str(out), "--touch-dist", "0.2", "--hold", "--out", str(js)]
    r = subprocess.run(ev, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    res = json.loads(js.read_text())
    paths = sorted(str(out / f) for f in os.listdir(out) if f.endswith(".pkl"))
    assert [row["file"] for row in res["files"]] == paths and len(paths) == 4 and len(res["groups"]) == 2
    assert [row["group"] for row in res["files"]] == [0, 0, 1, 1] and [c["name"] for c in res["columns"]] == [c[0] for c in metrics.COLUMNS]
    ms = metrics.MotionSet.from_rollout_files(paths, groups="names")
    per, crowd = metrics.motion_metrics(ms), metrics.crowd_metrics(ms, touch_dist=0.2, hold=True)
    same = lambda a, b: (a is None and not np.isfinite(b)) or a == b
    for i, row in enumerate(res["files"]):
        for c in metrics.COLUMNS:
            assert same(row[c[0]], per[c[0]][i].item()), (i, c[0], row[c[0]], per[c[0]][i])
        for k in ("clearance_min", "marker_dist_min", "overlap_frames", "touch_frames"):
            assert same(row[k], crowd["person"][k][i].item()), (i, k)
    for g, row in enumerate(res["groups"]):
        assert row["files"] == paths[2 * g:2 * g + 2] and row["size"] == 2
        for k in ("frames_compared", "clearance_min", "marker_dist_min", "overlap_frames", "touch_frames"):
            assert same(row[k], crowd["group"][k][g].item()), (g, k)
    assert same(res["mean"]["skate_mean"], float(np.mean(per["skate_mean"]))) and res["mean"]["pene_mean"] is None and res["hold"] is True
    assert "motion_3_0_p0.pkl" in r.stdout and "group 0:" in r.stdout
    alone = subprocess.run(ev[:3] + [paths[0], paths[3], "--out", str(tmp_path / "two.json")], cwd=str(tmp_path), env=env, capture_output=True,
                           text=True, timeout=300)
    assert alone.returncode == 0, alone.stderr[-2000:]
    two = json.loads((tmp_path / "two.json").read_text())
    assert len(two["files"]) == 2 and two["groups"] == [] and "clearance_min" not in two["files"][0]
