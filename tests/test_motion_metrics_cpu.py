"""The motion evaluator without a device: the numpy float64 reference (tests/motion_metrics_ref.py) against hand-made motions with
closed-form answers and against the search's own float64 restatement of the skate and floor arguments; `MotionSet` (frame table,
round trip through motion_*.pkl, n_valid, goal from wpath, grouping by file name, bad inputs); the column list against the header;
and, for the GPU file, that on the shared seeds no frame of the reference lies within 1e-9 of a threshold.

The hand-made coordinates are multiples of 2^-10 below 16 m and the world frames quarter turns, so the float32 records hold them
exactly and the closed forms hold to the roundings of float64 alone (1e-12)."""
import os
import re

import numpy as np
import pytest
import torch

from tests import motion_metrics_inputs as mi
from tests import motion_metrics_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUARTER = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]], np.float32)       # a yaw of 90 degrees: exact
STEP = np.array([2.0 ** -6, 2.0 ** -7, 0.0])                                                  # metres per frame
V = 40.0 * STEP


def _feet():
    from egogen_amd import synth
    return synth.feet_marker_idx()


def _records(world_markers, world_pelvis, K):
    """world tracks [F,67,3] / [F,3] with F = 18 K + 2 -> the records of K '2-frame' primitives, primitive k in the frame (QUARTER^k, a
    dyadic translation), and the frame table"""
    mk, pl, Rs, Ts = [], [], [], []
    for k in range(K):
        R = np.linalg.matrix_power(QUARTER.astype(np.float64), k % 4)
        T = np.array([0.25 * k, -0.5 * k, 0.125])
        sl = slice(18 * k, 18 * k + 20)
        mk.append((world_markers[sl] - T) @ R)          # R^T (w - T) per row
        pl.append((world_pelvis[sl] - T) @ R)
        Rs.append(R)
        Ts.append(T)
    rec = {"markers": np.stack(mk).astype(np.float32), "pelvis": np.stack(pl).astype(np.float32), "rotmat": np.stack(Rs).astype(np.float32),
           "transl": np.stack(Ts).astype(np.float32)}
    assert np.array_equal(rec["markers"].astype(np.float64), np.stack(mk)) and np.array_equal(rec["pelvis"].astype(np.float64), np.stack(pl))
    return rec, ref.frame_table([K])


def _rigid_body(K, seed, pin_feet=False):
    F = 18 * K + 2
    rng = np.random.default_rng(seed)
    body = rng.integers(-512, 512, (67, 3)) / 1024.0 + np.array([1.0, 2.0, 1.0])
    body[_feet(), 2] = rng.integers(0, 64, 6) / 1024.0
    move = np.arange(F)[:, None, None] * STEP
    markers = body[None] + move
    if pin_feet:
        markers[:, _feet()] = body[_feet()]
    pelvis = np.array([1.0, 2.0, 0.875]) + move[:, 0]
    return markers, pelvis, F


def test_rigid_translation_has_closed_form():
    markers, pelvis, F = _rigid_body(3, 1)
    rec, (src, start) = _records(markers, pelvis, 3)
    out, pf, _ = ref.motion_metrics(rec, src, start, _feet())
    speed, dur = float(np.linalg.norm(V)), (F - 1) / 40.0
    assert F == 56 and out["frames"][0] == F and out["duration_s"][0] == dur
    assert np.abs(pf[1:-1, 0] - speed).max() < 1e-12 and np.isnan(pf[[0, -1], 0]).all() and np.isnan(pf[:, 3]).all()
    assert abs(out["skate_speed_mean"][0] - speed) < 1e-12 and abs(out["skate_speed_max"][0] - speed) < 1e-12
    assert abs(out["skate_mean"][0] - (speed - 0.075)) < 1e-12 and out["skate_frames"][0] == F - 2
    assert abs(out["path_length"][0] - speed * dur) < 1e-12 and abs(out["displacement"][0] - speed * dur) < 1e-12
    assert abs(out["speed_mean"][0] - speed) < 1e-12
    assert out["acc_mean"][0] < 1e-12 and out["jerk_mean"][0] < 1e-12
    lowest = markers[0, _feet(), 2].min()
    assert abs(out["floor_min"][0] - lowest) < 1e-12 and abs(out["floor_max"][0] - lowest) < 1e-12
    assert abs(out["floor_mean"][0] - abs(lowest - 0.02)) < 1e-12
    assert np.isnan(out["goal_dist_end"][0]) and out["first_reached_frame"][0] == -1 and np.isnan(out["pene_mean"][0]) and out["pene_max"][0] == -1
    low = ref.motion_metrics(rec, src, start, _feet(), floor_z=0.25)[0]
    assert abs(low["floor_min"][0] - (lowest - 0.25)) < 1e-12


def test_pinned_feet_do_not_skate():
    markers, pelvis, F = _rigid_body(2, 2, pin_feet=True)
    rec, (src, start) = _records(markers, pelvis, 2)
    out, pf, _ = ref.motion_metrics(rec, src, start, _feet())
    assert F == 38 and out["skate_mean"][0] == 0.0 and out["skate_frames"][0] == 0 and out["skate_speed_max"][0] < 1e-12
    h = markers[0, _feet(), 2].min()
    assert abs(out["contact_score"][0] - np.exp(-max(abs(h) - 0.05, 0.0))) < 1e-12       # a planted foot within the band scores 1
    assert abs(out["path_length"][0] - float(np.linalg.norm(V)) * (F - 1) / 40.0) < 1e-12   # the pelvis still moves


def test_two_points_on_parallel_lines():
    d, K = 1.25, 2
    F = 18 * K + 2
    recs = []
    for y in (0.0, d):
        p = np.array([0.5, y, 1.0]) + np.arange(F)[:, None] * np.array([2.0 ** -6, 0.0, 0.0])
        recs.append(_records(np.repeat(p[:, None], 67, 1), p, K)[0])
    rec = {k: np.concatenate([r[k] for r in recs]) for k in recs[0]}
    src, start = ref.frame_table([K, K])
    clear, md, pairs = ref.crowd_metrics(rec, src, start, [0, 2], [0, 1], body_radius=0.3)
    assert pairs.tolist() == [[0, 1]] and clear.shape == (1, F)
    assert np.abs(clear - (d - 0.6)).max() < 1e-12 and np.abs(md - d).max() < 1e-12
    summ, margins = ref.summaries(clear, md, touch_dist=0.05)
    assert summ["overlap_frames"].tolist() == [0] and summ["touch_frames"].tolist() == [0] and summ["frames_compared"].tolist() == [F]
    close, _, _ = ref.crowd_metrics(rec, src, start, [0, 2], [0, 1], body_radius=0.75)
    assert ref.summaries(close, md)[0]["overlap_frames"].tolist() == [F]
    # unequal lengths: the second person recorded one primitive only
    one = {k: np.concatenate([recs[0][k], recs[1][k][:1]]) for k in recs[0]}
    src, start = ref.frame_table([K, 1])
    clear, md, _ = ref.crowd_metrics(one, src, start, [0, 2], [0, 1])
    assert np.isfinite(clear[0, :20]).all() and np.isnan(clear[0, 20:]).all() and np.isnan(md[0, 20:]).all()
    held, md_held, _ = ref.crowd_metrics(one, src, start, [0, 2], [0, 1], hold=True)
    assert np.isfinite(held).all()
    lag = (np.arange(20, F) - 19) * 2.0 ** -6                  # the second person stands at its frame 19, the first walks on
    assert np.abs(md_held[0, 20:] - np.sqrt(d * d + lag * lag)).max() < 1e-12


def test_goal_is_crossed_at_a_known_frame():
    K = 2
    F = 18 * K + 2
    p = np.array([0.0, 1.0, 0.875]) + np.arange(F)[:, None] * np.array([2.0 ** -5, 0.0, 0.0])
    rec, (src, start) = _records(np.repeat(p[:, None], 67, 1), p, K)
    goal = np.array([[1.0, 1.0, 0.875]], np.float32)
    out, pf, margins = ref.motion_metrics(rec, src, start, _feet(), goal=goal, goal_thresh=0.1)
    assert out["first_reached_frame"][0] == 29                  # 29 / 32 = 0.90625 is the first x within 0.1 of 1
    assert abs(out["goal_dist_min"][0] - 1e-12) < 1e-15         # frame 32 stands on the goal: the clip
    assert abs(out["goal_dist_end"][0] - (37 / 32 - 1.0)) < 1e-12
    assert abs(pf[29, 3] - (1.0 - 29 / 32)) < 1e-12 and min(margins["goal"]) > 1e-3
    far, _, _ = ref.motion_metrics(rec, src, start, _feet(), goal=goal + np.float32(8.0), goal_thresh=0.1)
    assert far["first_reached_frame"][0] == -1


def test_definitions_are_the_search_restatements():
    """one 20-frame primitive: skate_mean and floor_mean are the skate and floor arguments of tests/genop_search_ref.py in float64"""
    from tests import genop_search_ref as sref
    rec = {k: v[:1].copy() for k, v in mi.primitives(3, 5).items()}
    rec["rotmat"][0] = QUARTER                                  # an exact rotation: the restatement measures speed in the canonical frame
    src, start = ref.frame_table([1])
    out, _, _ = ref.motion_metrics(rec, src, start, _feet())
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    sc = sref.score(z(18, 1, 201), z(2, 1, 201), torch.randn(1, 20, 3, 3).double(), rec["markers"], rec["rotmat"], rec["transl"], None,
                    z(1, 3), _feet(), reproj_factor=1.0, dtype=torch.float64)
    assert abs(out["skate_mean"][0] - float(sc["skate"][0])) < 1e-12
    assert abs(out["floor_mean"][0] - float(sc["floor"][0])) < 1e-12


def test_pene_columns_are_exact_reductions():
    c = mi.motion_case("unequal")
    out, _, margins = mi.motion_reference("unequal", True, True)
    for i in range(3):
        cnt = c["pene_count"][c["frame_src"][c["motion_start"][i]:c["motion_start"][i + 1]]]
        assert out["pene_max"][i] == cnt.max() and out["pene_frames"][i] == (cnt >= mi.PENE_THRES).sum()
        assert abs(out["pene_mean"][i] - cnt.mean()) < 1e-12
    assert {39, 40} <= set(c["pene_count"].tolist()) and min(margins["pene"]) == 0.5


def test_shared_seeds_have_no_undecided_frame():
    """what tests/test_motion_metrics_gpu.py relies on: integer outputs must be equal, with a cap of zero undecided frames"""
    for name in mi.MOTION_CASES:
        margins = mi.motion_reference(name, True, True)[2]
        assert min(margins["skate"]) > mi.MARGIN and min(margins["goal"]) > mi.MARGIN, name
    for name in mi.CROWD_CASES:
        for hold in (False, True):
            margins = mi.crowd_reference(name, hold)[4]
            assert not margins["overlap"] or min(margins["overlap"]) > mi.MARGIN, (name, hold)
            assert not margins["touch"] or min(margins["touch"]) > mi.MARGIN, (name, hold)
    # the cases reach what they are for: a goal reached, frames on both sides of every threshold
    out = mi.motion_reference("unequal", True, True)[0]
    assert (out["first_reached_frame"] > 0).all() and out["frames"].tolist() == [20, 38, 272]
    assert mi.motion_reference("one_frame", True, True)[0]["frames"].tolist() == [39]
    summ = mi.crowd_reference("thirtytwo", False)[3]
    assert 0 < summ["overlap_frames"].sum() < 496 * 20 and 0 < summ["touch_frames"].sum() < 496 * 20
    assert mi.crowd_reference("alone", False)[0].shape == (0, 20)
    three, inter = mi.crowd_case("three"), mi.crowd_case("interleaved")
    for k in ("markers", "rotmat", "transl"):
        assert np.array_equal(np.concatenate([inter["rec"][k][a:b] for a, b in ((1, 2), (4, 6), (7, 22))]), three["rec"][k])


# ---- MotionSet ---------------------------------------------------------------------------------------------------------------------
def _sequence(K=3, b=2, seed=0, n_valid=None, goal=True, groups=None):
    from egogen_amd.genop import PrimitiveSequence
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    search = None
    if goal or n_valid is not None or groups is not None:
        search = {k: None for k in PrimitiveSequence.SEARCH_FIELDS}
        search.update(goal=f(b, 3) if goal else None, n_valid=None if n_valid is None else np.asarray(n_valid), groups=groups)
    return PrimitiveSequence(f(K, b, 20, 67, 3), f(K, b, 20, 93), f(K, b, 3, 3), f(K, b, 3), f(K, b, 20, 3), f(K, b, 128), f(b, 10), "male",
                             f(b, 3, 3), f(b, 3), search=search)


@pytest.mark.parametrize("types,frames", [(["2-frame"], 20), (["2-frame"] * 2, 38), (["2-frame"] * 15, 272), (["2-frame", "1-frame"], 39)])
def test_frame_table(types, frames):
    from egogen_amd.metrics import MotionSet
    P = len(types)
    z = lambda *s: np.zeros(s, np.float32)
    ms = MotionSet(z(P, 20, 67, 3), z(P, 20, 3), z(P, 3, 3), z(P, 3), z(P, 20, 93), z(P, 10), [0, P], types)
    assert ms.motion_start.tolist() == [0, frames] and ms.frames.tolist() == [frames] and len(ms) == 1
    want, start = ref.frame_table([P], types)
    assert np.array_equal(ms.frame_src, want) and ms.frame_src.dtype == np.int32 and ms.motion_start.dtype == np.int32
    assert ms.frame_src[:20].tolist() == list(range(20))
    if P > 1:
        assert ms.frame_src[20] == (21 if types[1] == "1-frame" else 22)


def test_frame_table_of_several_motions():
    from egogen_amd.metrics import MotionSet
    z = lambda *s: np.zeros(s, np.float32)
    ms = MotionSet(z(18, 20, 67, 3), z(18, 20, 3), z(18, 3, 3), z(18, 3), z(18, 20, 93), z(18, 10), [0, 1, 3, 18], ["2-frame"] * 18)
    assert ms.motion_start.tolist() == [0, 20, 58, 330] and ms.frame_src[20] == 20 and ms.frame_src[40] == 42 and ms.frame_src[58] == 60


def test_from_sequences_honours_n_valid_goal_and_groups():
    from egogen_amd.metrics import MotionSet
    q = _sequence(K=3, b=3, n_valid=[2, 3, 1], groups=np.array([7, 7, 4]))
    ms = MotionSet.from_sequences(q)
    assert ms.prim_start.tolist() == [0, 2, 5, 6] and ms.frames.tolist() == [38, 56, 20]
    assert np.array_equal(ms.markers[:2], q.markers[:2, 0]) and np.array_equal(ms.markers[2:5], q.markers[:, 1])
    assert np.array_equal(ms.pelvis[5], q.pelvis[0, 2]) and np.array_equal(ms.betas[2:5], np.repeat(q.betas[1:2], 3, 0))
    assert np.array_equal(ms.goals, q.goal) and ms.groups.tolist() == [0, 0, 1]
    two = MotionSet.from_sequences([q, _sequence(K=2, b=1, seed=1, goal=False)])
    assert len(two) == 4 and two.groups.tolist() == [0, 0, 1, 2] and np.isnan(two.goals[3]).all() and two.frames[3] == 38
    plain = MotionSet.from_sequences(_sequence(goal=False))
    assert plain.goals is None and plain.groups is None and plain.frames.tolist() == [56, 56]
    torch_q = _sequence(K=2, b=2, seed=3)
    for k in ("markers", "params", "rotmat", "transl", "pelvis", "betas"):
        setattr(torch_q, k, torch.as_tensor(getattr(torch_q, k)))
    assert np.array_equal(MotionSet.from_sequences(torch_q).markers, MotionSet.from_sequences(_sequence(K=2, b=2, seed=3)).markers)


def test_round_trip_through_files(tmp_path):
    from egogen_amd.metrics import MotionSet, groups_from_file_names
    q = _sequence(K=3, b=2, n_valid=[3, 2])
    paths = [q.save(str(tmp_path), i, man_id=f"5_0_p{i}") for i in range(2)]
    a, b = MotionSet.from_sequences(q), MotionSet.from_rollout_files(paths, groups="names")
    for k in ("markers", "pelvis", "rotmat", "transl", "params", "betas", "frame_src", "motion_start", "prim_start"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert np.array_equal(b.goals, q.goal) and b.groups.tolist() == [0, 0] and b.names == paths      # the goal is wpath[-1]
    assert b.mp_types == ["2-frame"] * 5
    # a '1-frame' primitive in a file keeps one more frame
    import pickle
    with open(paths[1], "rb") as fh:
        node = pickle.load(fh)
    node["motion"][1]["mp_type"] = "1-frame"
    with open(tmp_path / "motion_x.pkl", "wb") as fh:
        pickle.dump(node, fh)
    assert MotionSet.from_rollout_files(tmp_path / "motion_x.pkl").frames.tolist() == [39]
    names = ["motion_0_0_p0.pkl", "a/motion_0_1_p0.pkl", "motion_0_0_p1.pkl", "motion_9.pkl", "b/motion_0_1_p1.pkl", "motion_0_3.pkl",
             "motion_s_e_0_p2.pkl"]
    assert groups_from_file_names(names).tolist() == [0, 1, 0, 2, 1, 3, 4]


def test_bad_inputs_raise_value_error(tmp_path):
    import pickle
    from egogen_amd.metrics import MotionSet
    z = lambda *s: np.zeros(s, np.float32)
    ok = lambda **kw: dict(dict(markers=z(2, 20, 67, 3), pelvis=z(2, 20, 3), rotmat=z(2, 3, 3), transl=z(2, 3), params=z(2, 20, 93),
                                betas=z(2, 10), prim_start=[0, 2], mp_types=["2-frame"] * 2), **kw)
    MotionSet(**ok())
    nan = z(2, 20, 3)
    nan[1, 3, 0] = np.nan
    for kw in (dict(markers=z(2, 20, 66, 3)), dict(pelvis=z(2, 19, 3)), dict(prim_start=[0, 1]), dict(prim_start=[0, 0, 2]), dict(prim_start=[0]),
               dict(mp_types=["2-frame"]), dict(goals=z(2, 3)), dict(groups=[0, 1]), dict(pelvis=nan), dict(names=["a", "b"]),
               dict(goals=np.full((1, 3), np.inf, np.float32))):
        with pytest.raises(ValueError):
            MotionSet(**ok(**kw))
    with pytest.raises(ValueError):
        MotionSet.from_sequences([])
    with pytest.raises(ValueError):
        MotionSet.from_sequences(object())
    with pytest.raises(ValueError):
        MotionSet.from_rollout_files([])
    for name, node in (("empty", {"motion": []}), ("short", {"motion": [{"blended_marker": z(19, 67, 3)}]}), ("list", [1, 2])):
        with open(tmp_path / f"motion_{name}.pkl", "wb") as fh:
            pickle.dump(node, fh)
        with pytest.raises(ValueError):
            MotionSet.from_rollout_files(tmp_path / f"motion_{name}.pkl")
    with pytest.raises(ValueError):
        MotionSet.from_rollout_files(tmp_path / "motion_empty.pkl", groups="files")


def test_host_checks_need_no_device(monkeypatch):
    """argument errors are raised before the device is asked for; without a device the product path raises, it does not fall back"""
    from egogen_amd import _lib, metrics
    ms = mi.motion_set(mi.motion_case("one"))
    z = lambda *s: np.zeros(s, np.float32)
    short = metrics.MotionSet(z(1, 20, 67, 3), z(1, 20, 3), z(1, 3, 3), z(1, 3), z(1, 20, 93), z(1, 10), [0, 1], ["2-frame"])
    short.frame_src, short.motion_start = short.frame_src[:3], np.asarray([0, 3], np.int32)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for call in (lambda: metrics.motion_metrics(short), lambda: metrics.motion_metrics(ms, goal_thresh=-0.1),
                 lambda: metrics.motion_metrics(ms, pene_thres=-1), lambda: metrics.motion_metrics(ms, scene=object()),
                 lambda: metrics.crowd_metrics(ms, body_radius=-0.3), lambda: metrics.crowd_metrics(ms, touch_dist=float("nan")),
                 lambda: metrics.crowd_metrics(ms, groups=[0, 0]),
                 lambda: metrics.crowd_metrics(mi.motion_set(mi.crowd_case("thirtytwo")), groups=[0] * 32 + [0])):
        with pytest.raises(ValueError):
            call()
    z33 = metrics.MotionSet(z(33, 20, 67, 3), z(33, 20, 3), z(33, 3, 3), z(33, 3), z(33, 20, 93), z(33, 10), list(range(34)), ["2-frame"] * 33)
    with pytest.raises(ValueError):
        metrics.crowd_metrics(z33, groups=[0] * 33)
    with pytest.raises(_lib.EgxError):
        metrics.motion_metrics(ms)
    with pytest.raises(_lib.EgxError):
        metrics.crowd_metrics(ms)


def test_columns_are_the_header_columns():
    from egogen_amd import metrics
    txt = open(os.path.join(ROOT, "include", "egogen_hip.h")).read()
    defs = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define EGX_MM_([A-Z0-9_]+) (\d+)", txt)}
    assert defs.pop("f64_cols") == len(metrics.F64_COLUMNS) and defs.pop("i32_cols") == len(metrics.I32_COLUMNS)
    assert defs.pop("frame_cols") == len(metrics.FRAME_COLUMNS)
    want = {k: j for j, k in enumerate(metrics.F64_COLUMNS)}
    want.update({k: j for j, k in enumerate(metrics.I32_COLUMNS)})
    assert defs == want
    assert metrics.F64_COLUMNS == ref.F64 and metrics.I32_COLUMNS == ref.I32
    assert all(len(c) == 4 and c[2] in ("f64", "i32") for c in metrics.COLUMNS)
