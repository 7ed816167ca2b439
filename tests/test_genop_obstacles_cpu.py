"""Moving obstacles of the primitive search without a device: the `MovingObstacles` container (egogen_amd/obstacles.py), its
constructors and their errors, the restatement tests/genop_obstacles_ref.py on hand-computed values, the package export and the
argument errors of the driver that precede its device check."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import genop_obstacles_ref as oref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _obstacles():
    from egogen_amd.obstacles import MovingObstacles
    return MovingObstacles


def test_package_export():
    import egogen_amd
    from egogen_amd import MovingObstacles
    from egogen_amd.obstacles import MAX_OBSTACLES
    assert MovingObstacles is _obstacles() and egogen_amd.MovingObstacles is MovingObstacles
    hdr = open(os.path.join(ROOT, "include", "egogen_hip.h")).read()
    assert f"#define EGX_MAX_OBSTACLES {MAX_OBSTACLES} " in hdr and MAX_OBSTACLES == 32


def test_from_tracks_padding_count_and_index():
    MO = _obstacles()
    g = np.random.default_rng(0)
    a, b, c = g.normal(size=(3, 7, 2)), g.normal(size=(1, 7, 2)), np.zeros((0, 7, 2))
    m = MO.from_tracks([a, b, c], radius=[0.3, [0.4], 0.2], index=[2, 0, 0, 1])
    assert len(m) == 3 and m.max_obstacles == 3 and m.num_frames == 7 and m.device is None
    assert m.xy.dtype == np.float32 and m.xy.shape == (3, 3, 7, 2) and m.radius.shape == (3, 3)
    assert m.count.dtype == np.int32 and m.count.tolist() == [3, 1, 0] and m.index.dtype == np.int32 and m.index.tolist() == [2, 0, 0, 1]
    assert np.array_equal(m.xy[0], a.astype(np.float32)) and np.array_equal(m.xy[1, :1], b.astype(np.float32))
    assert (m.xy[1, 1:] == 0).all() and (m.xy[2] == 0).all()                      # padding
    assert np.allclose(m.radius[0], 0.3) and np.allclose(m.radius[1, 0], 0.4) and (m.radius > 0).all()
    one = MO.from_tracks(torch.as_tensor(a), radius=np.array([0.1, 0.2, 0.3]))    # one set, torch in, a radius per track
    assert len(one) == 1 and one.count.tolist() == [3] and one.index is None and np.allclose(one.radius[0], [0.1, 0.2, 0.3])
    empty = MO.from_tracks(np.zeros((0, 1, 2)))
    assert len(empty) == 1 and empty.count.tolist() == [0] and empty.max_obstacles == 1 and empty.num_frames == 1
    full = MO.from_tracks(np.zeros((32, 2, 2)))
    assert full.max_obstacles == 32 and full.count.tolist() == [32]


@pytest.mark.parametrize("kw,match", [
    (dict(xy=np.full((1, 3, 2), np.nan)), "non-finite"),
    (dict(xy=np.array([[[0.0, np.inf]]])), "non-finite"),
    (dict(xy=np.zeros((1, 3, 2)), radius=0.0), "radius"),
    (dict(xy=np.zeros((1, 3, 2)), radius=-0.3), "radius"),
    (dict(xy=np.zeros((2, 3, 2)), radius=[0.3, float("nan")]), "radius"),
    (dict(xy=np.zeros((33, 3, 2))), "at most 32"),
    (dict(xy=np.zeros((1, 0, 2))), "T >= 1"),
    (dict(xy=np.zeros((1, 3, 2)), index=[0, 1]), r"index must lie in \[0, 1\)"),
    (dict(xy=[np.zeros((1, 3, 2))] * 2, index=[-1, 0]), r"index must lie in \[0, 2\)"),
    (dict(xy=np.zeros((3, 2))), r"\[O,T,2\]"),
    (dict(xy=[np.zeros((1, 3, 2)), np.zeros((1, 4, 2))]), "share T"),
])
def test_from_tracks_errors(kw, match):
    with pytest.raises(ValueError, match=match):
        _obstacles().from_tracks(**kw)


def _handmade_sequence(to_torch=False):
    """K = 3, b = 2, n_valid = [3, 2]; the seed frames of primitive k + 1 are frames 18 and 19 of primitive k in the world"""
    from egogen_amd.genop import PrimitiveSequence
    g = np.random.default_rng(5)
    K, b = 3, 2
    yaw = g.normal(size=(K, b))
    R = np.zeros((K, b, 3, 3))
    R[..., 0, 0], R[..., 0, 1], R[..., 1, 0], R[..., 1, 1], R[..., 2, 2] = np.cos(yaw), -np.sin(yaw), np.sin(yaw), np.cos(yaw), 1.0
    T = g.normal(size=(K, b, 3))
    pelvis = g.normal(size=(K, b, 20, 3)) * 0.3
    for k in range(1, K):           # frames 0, 1 of primitive k: the world points of frames 18, 19 of primitive k - 1
        w = np.einsum("bij,btj->bti", R[k - 1], pelvis[k - 1, :, 18:]) + T[k - 1][:, None]
        pelvis[k, :, :2] = np.einsum("bji,btj->bti", R[k], w - T[k][:, None])
    f = (lambda x: torch.as_tensor(x, dtype=torch.float32)) if to_torch else (lambda x: x.astype(np.float32))
    n_valid = np.array([3, 2])
    search = {"goal": f(np.zeros((b, 3))), "choice": None, "cost": None, "cost_terms": None, "colliding": None, "status": None,
              "goal_dist": None, "n_valid": torch.as_tensor(n_valid) if to_torch else n_valid, "geo_dist": None}
    seq = PrimitiveSequence(f(np.zeros((K, b, 20, 67, 3))), f(np.zeros((K, b, 20, 93))), f(R), f(T), f(pelvis), f(np.zeros((K, b, 128))),
                            f(np.zeros((b, 10))), "male", f(np.tile(np.eye(3), (b, 1, 1))), f(np.zeros((b, 3))), search=search)
    world = np.einsum("kbij,kbtj->kbti", R.astype(np.float32).astype(np.float64), pelvis.astype(np.float32).astype(np.float64)) + \
        T.astype(np.float32).astype(np.float64)[:, :, None]
    return seq, world


@pytest.mark.parametrize("to_torch", [False, True])
def test_from_sequences(to_torch):
    MO = _obstacles()
    seq, world = _handmade_sequence(to_torch)
    assert seq.obstacle_term is None and seq.clearance is None and seq.obstacle_hit is None     # results without them construct as before
    m = MO.from_sequences(seq, radius=0.25)
    T = 20 + 18 * 2
    assert len(m) == 1 and m.count.tolist() == [2] and m.num_frames == T and np.allclose(m.radius[0], 0.25)
    for i, n in enumerate([3, 2]):
        for k in range(n):
            for t in range(20):
                assert np.array_equal(m.xy[0, i, 18 * k + t], world[k, i, t, :2].astype(np.float32)) or t < 2 and k > 0, (i, k, t)
    # frames 18, 19 of primitive k are frames 0, 1 of primitive k + 1 (to rounding) and appear once: 20 + 18 (n - 1) frames
    for k in range(2):
        assert np.allclose(world[k, :, 18:], world[k + 1, :, :2], atol=1e-5)
        assert np.allclose(m.xy[0, 0, 18 * (k + 1):18 * (k + 1) + 2], world[k + 1, 0, :2, :2], atol=1e-5)
    last = world[1, 1, 19, :2].astype(np.float32)                                 # the shorter track: held at its last valid frame
    assert (m.xy[0, 1, 20 + 18 - 1:] == last).all() and not np.array_equal(m.xy[0, 1, 20 + 18 - 2], last)
    late = MO.from_sequences([seq, seq], start_frame=7)
    assert late.count.tolist() == [4] and late.num_frames == T + 7
    assert np.array_equal(late.xy[0, :2, 7:], m.xy[0]) and np.array_equal(late.xy[0, 2:], late.xy[0, :2])
    assert (late.xy[0, :, :7] == late.xy[0, :, 7:8]).all()                       # standing at the first position before the start
    with pytest.raises(ValueError, match="start_frame"):
        MO.from_sequences(seq, start_frame=-1)
    with pytest.raises(ValueError, match="radius"):
        MO.from_sequences(seq, radius=0.0)
    with pytest.raises(ValueError, match="at most 32"):
        MO.from_sequences([seq] * 17)


def test_round_trip_through_rollout_files(tmp_path):
    MO = _obstacles()
    seq, _ = _handmade_sequence()
    paths = [seq.save(str(tmp_path), i, man_id=f"t_{i}") for i in range(2)]
    a, b = MO.from_sequences(seq), MO.from_rollout_files(paths)
    assert np.array_equal(a.xy, b.xy) and np.array_equal(a.count, b.count) and np.array_equal(a.radius, b.radius)
    one = MO.from_rollout_files(paths[1], radius=0.2)
    assert one.count.tolist() == [1] and one.num_frames == 20 + 18 and np.array_equal(one.xy[0, 0], a.xy[0, 1, :38])
    # a '1-frame' primitive drops one frame instead of two
    import pickle
    with open(paths[0], "rb") as fh:
        node = pickle.load(fh)
    node["motion"][1]["mp_type"] = "1-frame"
    p1 = str(tmp_path / "one_frame.pkl")
    with open(p1, "wb") as fh:
        pickle.dump(node, fh)
    c = MO.from_rollout_files([p1])
    assert c.num_frames == 20 + 19 + 18 and np.array_equal(c.xy[0, 0, :20], a.xy[0, 0, :20]) and np.array_equal(c.xy[0, 0, 21:39], a.xy[0, 0, 20:38])
    with open(p1, "wb") as fh:
        pickle.dump({"motion": []}, fh)
    with pytest.raises(ValueError, match="no motion primitives"):
        MO.from_rollout_files([p1])
    with pytest.raises(OSError):
        MO.from_rollout_files([str(tmp_path / "absent.pkl")])


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def _one_row(x_step=0.0):
    """one row in the identity frame whose pelvis stands at (0.1 t * x_step, 0, 0.9) at frame t"""
    J = torch.zeros(1, 20, 3, 3)
    J[0, :, 0, 0] = torch.arange(20) * 0.1 * x_step
    J[0, :, 0, 2] = 0.9
    return torch.eye(3)[None], torch.zeros(1, 3), J


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_restatement_empty_set_and_zero_margin(dtype):
    R0, T0, J = _one_row()
    xy, radius = np.zeros((1, 1, 4, 2), np.float32), np.ones((1, 1), np.float32)
    r = oref.row_terms(R0, T0, J, xy, radius, [0], [0], 0, 0.5, 0.3, dtype)
    assert float(r["term"]) == 0.0 and float(r["clearance"]) == float("inf") and not bool(r["hit"])
    # margin 0: a row that keeps clear of the obstacle, however narrowly, pays nothing (with the margin it does) ...
    near = np.tile(np.array([1.4, 0.0], np.float32), (1, 1, 4, 1))                # clearance 1.4 - (1 + 0.3) = 0.1
    r = oref.row_terms(R0, T0, J, near, radius, [1], [0], 0, 0.5, 0.3, dtype)
    assert abs(float(r["term"]) - 0.4) < 1e-6 and abs(float(r["clearance"]) - 0.1) < 1e-6 and not bool(r["hit"])
    r = oref.row_terms(R0, T0, J, near, radius, [1], [0], 0, 0.0, 0.3, dtype)
    assert float(r["term"]) == 0.0 and abs(float(r["clearance"]) - 0.1) < 1e-6 and not bool(r["hit"])
    # ... and the veto is intact: an overlapping row is a hit (max(0, 0 - c_t) is then the depth of the overlap)
    r = oref.row_terms(R0, T0, J, xy, radius, [1], [0], 0, 0.0, 0.3, dtype)
    assert bool(r["hit"]) and abs(float(r["clearance"]) + 1.3) < 1e-6 and abs(float(r["term"]) - 1.3) < 1e-6
    Jn = J.clone()
    Jn[0, 7, 0, 1] = float("nan")                                                 # a NaN pelvis: NaN term, not a hit
    r = oref.row_terms(R0, T0, Jn, xy, radius, [1], [0], 0, 0.5, 0.3, dtype)
    assert torch.isnan(r["term"]).all() and torch.isnan(r["clearance"]).all() and not bool(r["hit"])
    Jn[0, 7, 0, 1], Jn[0, 1, 0, 1] = 0.0, float("nan")                            # the seed frames are not scored
    r = oref.row_terms(R0, T0, Jn, xy, radius, [1], [0], 0, 0.5, 0.3, dtype)
    assert torch.isfinite(r["term"]).all()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_restatement_hand_computed(dtype):
    """One obstacle of radius 0.2 standing at (3, 4): a pelvis at the origin is 5 m away, clearance 5 - (0.2 + 0.3) = 4.5; with
    margin 5 every frame pays 0.5, the term is 0.5.  Walking along x at 0.1 m per frame, frame t is at (0.1 t, 0); against an
    obstacle at (1.9, 0) the closest scored frame is 19: clearance -0.5, a hit; the term with margin 0.5 is the mean over t = 2..19
    of max(0, 0.5 - (|0.1 t - 1.9| - 0.5))."""
    R0, T0, J = _one_row()
    xy = np.tile(np.array([3.0, 4.0], np.float32), (1, 1, 5, 1))
    radius = np.full((1, 1), 0.2, np.float32)
    r = oref.row_terms(R0, T0, J, xy, radius, [1], [0], 0, 5.0, 0.3, dtype)
    tol = 1e-12 if dtype == torch.float64 else 1e-6
    r02 = float(np.float32(0.2)) + float(np.float32(0.3))
    assert abs(float(r["clearance"]) - (5.0 - r02)) < tol * 10 and abs(float(r["term"]) - (r02)) < tol * 10 and not bool(r["hit"])
    R0, T0, J = _one_row(1.0)
    xy = np.tile(np.array([1.9, 0.0], np.float32), (1, 1, 5, 1))
    r = oref.row_terms(R0, T0, J, xy, radius, [1], [0], 0, 0.5, 0.3, dtype)
    c = [abs(float(np.float32(0.1 * t)) - float(np.float32(1.9))) - r02 for t in range(2, 20)]
    assert abs(float(r["clearance"]) - min(c)) < 1e-5 and bool(r["hit"]) and min(c) < -0.49
    assert abs(float(r["term"]) - sum(max(0.0, 0.5 - v) for v in c) / 18) < 1e-5
    # the world frame: the same row turned by 90 degrees about z and moved meets an obstacle moved the same way
    Rz = torch.tensor([[[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]])
    xy2 = np.tile(np.array([2.0, 1.9 - 1.0], np.float32), (1, 1, 5, 1))
    r2 = oref.row_terms(Rz, torch.tensor([[2.0, -1.0, 0.0]]), J, xy2, radius, [1], [0], 0, 0.5, 0.3, dtype)
    assert abs(float(r2["clearance"]) - float(r["clearance"])) < 1e-5 and abs(float(r2["term"]) - float(r["term"])) < 1e-5


def test_restatement_clamp_and_window():
    xy = np.arange(6, dtype=np.float32).reshape(1, 3, 2)                           # T = 3: frames (0,1), (2,3), (4,5)
    w = oref.window(xy, 0, torch.float64)
    assert w.shape == (18, 1, 2) and w[0, 0].tolist() == [4.0, 5.0] and w[-1, 0].tolist() == [4.0, 5.0]     # frame 2, then clamped
    w = oref.window(xy, -3, torch.float64)                                        # frames -1, 0, 1, 2, 2, ...
    assert [v[0] for v in w[:4, 0].tolist()] == [0.0, 0.0, 2.0, 4.0]
    w = oref.window(xy, -40, torch.float64)
    assert (w[:, 0, 0] == 0).all()


def test_restatement_cost_q_and_veto():
    """apply: the cost and q gain w_obs * term, colliding is OR-ed with hit; select: a hit row loses to a dearer free one"""
    f = torch.float64
    r = {"dist": torch.tensor([1.0, 2.0], dtype=f), "skate": torch.tensor([0.1, 0.2], dtype=f), "floor": torch.zeros(2, dtype=f),
         "pene": torch.zeros(2, dtype=f), "face": torch.zeros(2, dtype=f), "colliding": torch.tensor([False, False])}
    r["cost"] = r["dist"] + r["skate"]
    ob = {"term": torch.tensor([0.25, 0.0], dtype=f), "clearance": torch.tensor([-0.1, 2.0], dtype=f), "hit": torch.tensor([True, False])}
    a = oref.apply(r, ob, 2.0, f)
    assert a["cost"].tolist() == [1.1 + 0.5, 2.2] and a["q"].tolist() == [0.1 + 0.5, 0.2] and a["colliding"].tolist() == [True, False]
    choice, status = oref.select(a, 1, 2)
    assert choice.tolist() == [1] and status.tolist() == [0]
    ob["hit"] = torch.tensor([True, True])
    choice, status = oref.select(oref.apply(r, ob, 2.0, f), 1, 2)
    assert choice.tolist() == [0] and status.tolist() == [1]                      # all blocked: the cheapest, status bit 0
    ob["term"] = torch.tensor([float("nan"), 0.0], dtype=f)
    choice, status = oref.select(oref.apply(r, ob, 2.0, f), 1, 2)
    assert choice.tolist() == [1]                                                 # a NaN term: the row ranks as non-finite
    sel = oref.beam_select(a, 1, 2, 1, torch.tensor([[1.0, 0.5]], dtype=f), torch.zeros(1, 2, dtype=torch.long))
    assert sel["beam_row"].tolist() == [[1, 0]] and sel["ncoll"].tolist() == [[0, 1]] and sel["acc"].tolist() == [[0.5 + 0.2, 1.0 + 0.6]]


# ---- the driver, before its device check ------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra,match", [
    (["--avoid", "a.pkl"], "--avoid needs --goal"),
    (["--goal", "0,1,0.9", "--start", "1,2"], "--start takes x,y,yaw_deg"),
    (["--goal", "0,1,0.9", "--start", "1,2,north"], "--start takes x,y,yaw_deg"),
    (["--goal", "0,1,0.9", "--avoid", "absent.pkl"], "--avoid absent.pkl"),
])
def test_driver_argument_errors(tmp_path, extra, match):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "exp_GAMMAPrimitive", "gen_motion.py"), "--out", str(tmp_path / "out")] + extra,
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and match in r.stderr and "HIP device" not in r.stderr, r.stderr[-800:]
    assert not os.path.exists(tmp_path / "out")
