"""The marker model of recorded tracks without a device: `MovingObstacles` with markers (egogen_amd/obstacles.py), the restatement
tests/genop_obstacle_markers_ref.py against itself, and the errors `generate_sequence_to_goal(obstacle_model=, obstacle_skin=)` and the
driver raise before any device work.

The float32 restatement against the float64 one: a world coordinate of magnitude at most `big` carries a few roundings of half an ulp
of `big` each (the blend, three products and sums of the frame, the translation), a difference of two of them one more, and the root
of the sum of three squares is as well conditioned as its largest difference; the subtraction of the skin rounds once more.  16 ulps
of `big` bound all of that - the allowance tests/test_genop_joint_markers_gpu.py grants the same chain against the evaluator."""
import os
import pickle
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import genop_obstacle_markers_ref as kref
from tests.test_genop_obstacles_cpu import _handmade_sequence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _MO():
    from egogen_amd.obstacles import MovingObstacles
    return MovingObstacles


def _sequence(to_torch=False):
    """the hand-made sequence of tests/test_genop_obstacles_cpu.py (K = 3, b = 2, n_valid = [3, 2]) with markers -> it, and its world
    markers [K,b,20,67,3] in float64 from the float32 records"""
    seq, _ = _handmade_sequence(to_torch)
    m = (np.random.default_rng(11).normal(size=(3, 2, 20, 67, 3)) * 0.4).astype(np.float32)
    seq.markers = torch.as_tensor(m) if to_torch else m
    f64 = lambda x: np.asarray(x, np.float32).astype(np.float64)
    world = np.einsum("kbij,kbtaj->kbtai", f64(seq.rotmat), f64(m)) + f64(seq.transl)[:, :, None, None]
    return seq, world


# ---- the constructors --------------------------------------------------------------------------------------------------------------
def test_from_tracks_with_markers():
    MO = _MO()
    g = np.random.default_rng(0)
    xy = [g.normal(size=(2, 5, 2)), g.normal(size=(0, 5, 2)), g.normal(size=(3, 5, 2))]
    mk = [g.normal(size=(2, 5, 67, 3)), np.zeros((0, 5, 67, 3)), g.normal(size=(3, 5, 67, 3))]
    m = MO.from_tracks(xy, radius=0.2, index=[2, 0, 1, 1], markers=mk)
    assert m.markers.shape == (3, 3, 5, 67, 3) and m.markers.dtype == np.float32 and m.count.tolist() == [2, 0, 3]
    assert np.array_equal(m.markers[0, :2], mk[0].astype(np.float32)) and np.array_equal(m.markers[2], mk[2].astype(np.float32))
    assert not m.markers[0, 2:].any() and not m.markers[1].any()                          # padding
    assert m.xy.shape == (3, 3, 5, 2) and np.array_equal(m.xy[2], xy[2].astype(np.float32))   # xy, radius, count, index as without markers
    one = MO.from_tracks(xy[0], markers=torch.as_tensor(mk[0]))                             # one set, a tensor
    assert one.markers.shape == (1, 2, 5, 67, 3) and np.array_equal(one.markers[0], m.markers[0, :2])
    d = one.to("cpu")
    assert d._dev["markers"].dtype == torch.float32 and d._dev["markers"].shape == (1, 2, 5, 67, 3) and d._dev["markers"].is_contiguous()
    args, alive = d.marker_args(4)
    sel, _ = d.select_args(4)
    assert len(args) == 6 and args[3:] == (1, 2, 5) and args[3:] == sel[4:] and args[1].value == sel[2].value and args[2] is None
    assert args[0].value == d._dev["markers"].data_ptr()


@pytest.mark.parametrize("kw,match", [
    (dict(markers=np.zeros((2, 5, 67, 3))), "like its xy"),                       # another O
    (dict(markers=np.zeros((3, 4, 67, 3))), "like its xy"),                       # another T
    (dict(markers=np.zeros((3, 5, 66, 3))), "like its xy"),
    (dict(markers=[np.zeros((3, 5, 67, 3))] * 2), "one array per set"),
    (dict(markers=np.full((3, 5, 67, 3), np.nan)), "non-finite marker"),
    (dict(markers=np.full((3, 5, 67, 3), np.inf)), "non-finite marker"),
    (dict(markers=np.full((3, 5, 67, 3), 1e39)), "overflows float32"),
])
def test_from_tracks_marker_errors(kw, match):
    with pytest.raises(ValueError, match=match):
        _MO().from_tracks(np.zeros((3, 5, 2)), **kw)


def test_the_cap_is_checked_on_the_host(monkeypatch):
    from egogen_amd import obstacles
    assert obstacles.OBSTACLE_MARKERS_CAP_BYTES == 1 << 30
    xy, mk = np.zeros((3, 5, 2)), np.zeros((3, 5, 67, 3))
    monkeypatch.setattr(obstacles, "OBSTACLE_MARKERS_CAP_BYTES", 3 * 5 * 804 - 1)
    with pytest.raises(ValueError, match="above the cap"):
        obstacles.MovingObstacles.from_tracks(xy, markers=mk)
    assert obstacles.MovingObstacles.from_tracks(xy).markers is None                       # the cylinders are not bound by it
    monkeypatch.setattr(obstacles, "OBSTACLE_MARKERS_CAP_BYTES", 3 * 5 * 804)
    assert obstacles.MovingObstacles.from_tracks(xy, markers=mk).markers.nbytes == 3 * 5 * 804


@pytest.mark.parametrize("to_torch", [False, True])
def test_from_sequences_with_markers(to_torch):
    MO = _MO()
    seq, world = _sequence(to_torch)
    m = MO.from_sequences(seq, radius=0.25, markers=True)
    T = 20 + 18 * 2
    assert m.markers.shape == (1, 2, T, 67, 3) and m.num_frames == T
    for i, n in enumerate([3, 2]):
        for k in range(n):
            first = 0 if k == 0 else 2                                                       # a later primitive drops its two seed frames
            want = world[k, i, first:].astype(np.float32)
            assert np.array_equal(m.markers[0, i, 18 * k + first:18 * k + 20], want), (i, k)
    last = world[1, 1, 19].astype(np.float32)                                                # the shorter track: held at its last pose
    assert (m.markers[0, 1, 20 + 18 - 1:] == last).all() and not np.array_equal(m.markers[0, 1, 20 + 18 - 2], last)
    late = MO.from_sequences([seq, seq], start_frame=7, markers=True)
    assert late.markers.shape == (1, 4, T + 7, 67, 3)
    assert np.array_equal(late.markers[0, :2, 7:], m.markers[0]) and np.array_equal(late.markers[0, 2:], late.markers[0, :2])
    assert (late.markers[0, :, :7] == late.markers[0, :, 7:8]).all()                        # standing at the first pose before the start
    # the positions are those of the object without markers
    plain = MO.from_sequences([seq, seq], start_frame=7)
    assert np.array_equal(late.xy, plain.xy) and np.array_equal(late.radius, plain.radius) and np.array_equal(late.count, plain.count)
    seq.markers = seq.markers[:, :, :, :66]
    with pytest.raises(ValueError, match=r"markers \[K,b,20,67,3\]"):
        MO.from_sequences(seq, markers=True)


def test_markers_false_is_the_object_as_it_was():
    MO = _MO()
    seq, _ = _sequence()
    for m in (MO.from_sequences(seq), MO.from_sequences(seq, markers=False), MO.from_tracks(np.zeros((1, 4, 2)))):
        assert m.markers is None and m.to("cpu")._dev["markers"] is None
        assert sorted(k for k in vars(m) if not k.startswith("_")) == ["count", "device", "index", "markers", "radius", "xy"]
        assert len(m.select_args(1)[0]) == 7
        with pytest.raises(ValueError, match="carry no markers"):
            m.marker_args(1)
    a, b = MO.from_sequences(seq), MO.from_sequences(seq, markers=True)
    for k in ("xy", "radius", "count"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert a.index is None and b.index is None


def test_rollout_files_equal_sequences(tmp_path):
    MO = _MO()
    seq, _ = _sequence()
    paths = [seq.save(str(tmp_path), i, man_id=f"t_{i}") for i in range(2)]
    a, b = MO.from_sequences(seq, markers=True), MO.from_rollout_files(paths, markers=True)
    assert np.array_equal(a.markers, b.markers) and np.array_equal(a.xy, b.xy) and np.array_equal(a.count, b.count)
    assert MO.from_rollout_files(paths).markers is None
    one = MO.from_rollout_files(paths[1], radius=0.2, markers=True)
    assert one.markers.shape == (1, 1, 38, 67, 3) and np.array_equal(one.markers[0, 0], a.markers[0, 1, :38])
    # a '1-frame' primitive drops one frame instead of two
    with open(paths[0], "rb") as fh:
        node = pickle.load(fh)
    node["motion"][1]["mp_type"] = "1-frame"
    p1 = str(tmp_path / "one_frame.pkl")
    with open(p1, "wb") as fh:
        pickle.dump(node, fh)
    c = MO.from_rollout_files([p1], markers=True)
    assert c.markers.shape == (1, 1, 20 + 19 + 18, 67, 3)
    assert np.array_equal(c.markers[0, 0, :20], a.markers[0, 0, :20]) and np.array_equal(c.markers[0, 0, 21:39], a.markers[0, 0, 20:38])
    del node["motion"][2]["blended_marker"]
    with open(p1, "wb") as fh:
        pickle.dump(node, fh)
    with pytest.raises(KeyError):
        MO.from_rollout_files([p1], markers=True)
    assert MO.from_rollout_files([p1]).markers is None                                      # the cylinders do not read them


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def test_fma32_is_the_rounding_of_the_exact_value():
    g = np.random.default_rng(3)
    a, b = g.normal(size=4000).astype(np.float32), g.normal(size=4000).astype(np.float32)
    c = (-(a.astype(np.float64) * b) * (1 + g.normal(size=4000) * 1e-7)).astype(np.float32)   # cancelling: where a double rounding shows
    c[::3] = g.normal(size=len(c[::3])).astype(np.float32)
    got = kref.fma32(a, b, c)
    for x, y, z, r in zip(a, b, c, got):
        exact = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        near = np.float32(float(exact))                                                      # float(Fraction) rounds once to double; refine below
        cands = [near, np.nextafter(near, np.float32(np.inf)), np.nextafter(near, np.float32(-np.inf))]
        best = min(cands, key=lambda v: (abs(Fraction(float(v)) - exact), int(np.float32(v).view(np.uint32)) & 1))
        assert r == best, (x, y, z, r, best)
    assert np.isnan(kref.fma32(np.float32("nan"), 1.0, 1.0)) and kref.fma32(2.0, 3.0, np.float32("inf")) == np.inf


def _case(seed=0, rows=6, S=2, O=5, T=7):
    g = np.random.default_rng(seed)
    yaw = g.normal(size=rows)
    R0 = np.zeros((rows, 3, 3), np.float32)
    R0[:, 0, 0], R0[:, 0, 1], R0[:, 1, 0], R0[:, 1, 1], R0[:, 2, 2] = np.cos(yaw), -np.sin(yaw), np.sin(yaw), np.cos(yaw), 1.0
    T0 = (g.normal(size=(rows, 3)) * 2).astype(np.float32)
    local = g.normal(size=(rows, 20, 67, 3)) * np.array([0.3, 0.2, 0.8])
    delta = g.uniform(-0.05, 0.05, size=(rows, 18, 67, 3))
    mp = local.astype(np.float32)
    mp[:, 2:] = (local[:, 2:] + delta).astype(np.float32)
    Y_gen = (local[:, 2:] - delta).transpose(1, 0, 2, 3).reshape(18, rows, 201).astype(np.float32)
    w64 = kref.world_markers64(R0, T0, mp, Y_gen, 0.5)
    obs = np.zeros((S, O, T, 67, 3), np.float32)
    for s in range(S):
        for o in range(O):
            r = (s * O + o) % rows
            obs[s, o] = (w64[r, np.clip(np.arange(T), 0, 17)] + g.normal(size=3) * [0.05, 0.2, 0.6][o % 3]).astype(np.float32)
    return R0, T0, mp, Y_gen, obs


def test_float32_restatement_stays_within_round_off_of_float64():
    R0, T0, mp, Y_gen, obs = _case()
    count, set_of_row = np.array([5, 3]), np.array([0, 1, 0, 1, 1, 0])
    w32, w64 = kref.world_markers32(R0, T0, mp, Y_gen, 0.5), kref.world_markers64(R0, T0, mp, Y_gen, 0.5)
    big = float(max(np.abs(w64).max(), np.abs(obs).max()))
    bound = 16.0 * 2.0 ** (np.floor(np.log2(big)) - 23)
    assert float(np.abs(w32 - w64).max()) <= bound
    for frame0 in (-3, 0, 40):
        c32 = kref.frame_clearance32(w32, obs, count, set_of_row, frame0, 0.05)
        c64 = kref.frame_clearance64(w64, obs, count, set_of_row, frame0, 0.05)
        assert c32.dtype == np.float32 and c32.shape == (6, 18) and np.isfinite(c64).all()
        assert float(np.abs(c32 - c64).max()) <= bound, (frame0, float(np.abs(c32 - c64).max()), bound)
        assert (c64 < 0).any() and ((c64 > 0) & (c64 < 0.6)).any()
    t32, t64 = kref.terms_of_clearance(c32, 0.6), kref.terms_of_clearance(c64, 0.6, torch.float64)
    assert float((t32["term"].double() - t64["term"]).abs().max()) <= bound and torch.equal(t32["hit"], t64["hit"])
    assert float((t32["clearance"].double() - t64["clearance"]).abs().max()) <= bound


def test_restatement_clamps_empty_sets_and_bad_frames():
    R0, T0, mp, Y_gen, obs = _case(1)
    w = kref.world_markers32(R0, T0, mp, Y_gen, 0.5)
    assert kref.frames_of(-3, 7).tolist() == [0, 0, 1, 2, 3, 4, 5] + [6] * 11 and kref.frames_of(40, 7).tolist() == [6] * 18
    c = kref.frame_clearance32(w, obs, np.array([0, 5]), np.array([0, 1, 0, 1, 1, 0]), -3, 0.05)
    assert np.isinf(c[[0, 2, 5]]).all() and (c[[0, 2, 5]] > 0).all() and np.isfinite(c[[1, 3, 4]]).all()      # the empty set: +inf
    # a track that stands still is read at one frame whatever the clamp does
    still = np.repeat(obs[:, :, :1], 7, 2)
    a, b = (kref.frame_clearance32(w, still, np.array([5, 5]), np.zeros(6, int), f0, 0.05) for f0 in (-3, 40))
    assert np.array_equal(a, b)
    # the count is clamped to the tracks there are; the set index into the sets
    assert np.array_equal(kref.frame_clearance32(w, obs, np.array([9, 9]), np.array([-1, 7, 0, 1, 1, 0]), 0, 0.05),
                          kref.frame_clearance32(w, obs, np.array([5, 5]), np.array([0, 1, 0, 1, 1, 0]), 0, 0.05))
    # one NaN marker of one frame of one row: NaN there and only there, also against the empty set
    Y_bad = Y_gen.copy()
    Y_bad[4, 3, 65 * 3 + 1] = np.nan
    Y_bad[7, 0, 0] = np.nan
    cb = kref.frame_clearance32(kref.world_markers32(R0, T0, mp, Y_bad, 0.5), obs, np.array([0, 5]), np.array([0, 1, 0, 1, 1, 0]), -3, 0.05)
    where = np.zeros((6, 18), bool)
    where[3, 4] = where[0, 7] = True
    assert np.array_equal(np.isnan(cb), where) and np.array_equal(cb[~where], c[~where])
    t = kref.terms_of_clearance(cb, 0.6)
    assert torch.isnan(t["term"][[0, 3]]).all() and torch.isnan(t["clearance"][[0, 3]]).all() and not t["hit"][[0, 3]].any()
    # a NaN obstacle marker is not there
    gone = obs.copy()
    gone[1, 2, :, 5, 0] = np.nan
    cg = kref.frame_clearance32(w, gone, np.array([0, 5]), np.array([0, 1, 0, 1, 1, 0]), -3, 0.05)
    assert np.isfinite(cg[[1, 3, 4]]).all() and (cg >= c).all()


def test_terms_follow_the_cylinder_phase():
    c = np.full((4, 18), np.inf, np.float32)
    c[1] = 0.25                                   # inside the margin at every frame
    c[2, 3] = -0.1                                # one frame of contact
    c[3, :] = np.linspace(0.1, 0.9, 18)
    t = kref.terms_of_clearance(c, 0.5)
    assert t["term"][0] == 0 and t["clearance"][0] == float("inf") and not t["hit"][0]
    assert abs(float(t["term"][1]) - 0.25) < 1e-6 and t["clearance"][1] == np.float32(0.25)
    assert abs(float(t["term"][2]) - 0.6 / 18) < 1e-6 and t["hit"].tolist() == [False, False, True, False]
    want = np.maximum(0, np.float32(0.5) - c[3].astype(np.float64)).sum() / 18
    assert abs(float(t["term"][3]) - want) < 1e-6
    # the tree: lane 0 ends with ((v0 + v16) + v8) + v4 ... of the 18 lanes that hold a frame
    v = np.random.default_rng(2).normal(size=18).astype(np.float32)
    s = lambda *i: v[list(i)]
    l0 = ((v[0] + v[16]) + v[8]) + (v[4] + v[12])
    l2 = (v[2] + v[10]) + (v[6] + v[14])
    l1 = ((v[1] + v[17]) + v[9]) + (v[5] + v[13])
    l3 = (v[3] + v[11]) + (v[7] + v[15])
    assert kref.wave_sum32(v[None])[0] == np.float32(np.float32(l0 + l2) + np.float32(l1 + l3))
    # cost, q and the veto through the cylinder restatement's `apply`
    cost, terms = torch.tensor([1.0, 2.0, 3.0, 4.0]), torch.arange(20, dtype=torch.float32).reshape(4, 5)
    a = kref.apply_rows(cost, terms, torch.tensor([0, 1, 0, 0]), t, 2.0, q=torch.tensor([0.5, 0.5, 0.5, 0.5]))
    assert torch.equal(a["cost"], cost + 2.0 * t["term"]) and torch.equal(a["q"], 0.5 + 2.0 * t["term"])
    assert a["colliding"].tolist() == [False, True, True, False]
    assert kref.select(a, 1, 4)[0].tolist() == [0]


# ---- generate_sequence_to_goal and the driver: the errors come before any device work ------------------------------------------------
def test_generate_sequence_to_goal_obstacle_model_errors_need_no_device():
    from egogen_amd.genop import OBSTACLE_MODELS, GAMMAPrimitiveComboGenOP
    assert OBSTACLE_MODELS == ("cylinder", "markers")
    op = GAMMAPrimitiveComboGenOP.__new__(GAMMAPrimitiveComboGenOP)      # no constructor: it asks for a device
    op.body_model, op.model = object(), None
    mk = lambda b: (np.zeros((2, b, 201), np.float32), np.zeros((2, b, 93), np.float32), np.zeros(10, np.float32), np.zeros(3, np.float32))
    call = lambda N=2, b=3, **kw: op.generate_sequence_to_goal(*mk(b), 2, N, **kw)
    MO = _MO()
    plain = MO.from_tracks(np.zeros((1, 4, 2)))
    full = MO.from_tracks(np.zeros((1, 4, 2)), markers=np.zeros((1, 4, 67, 3)))
    with pytest.raises(ValueError, match="obstacle_model must be one of"):
        call(obstacles=full, obstacle_model="capsule")
    with pytest.raises(ValueError, match="needs obstacles= that carry markers"):
        call(obstacle_model="markers")
    with pytest.raises(ValueError, match="needs obstacles= that carry markers"):
        call(obstacles=plain, obstacle_model="markers")
    for skin in (-0.01, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="obstacle_skin"):
            call(obstacles=full, obstacle_model="markers", obstacle_skin=skin)
    assert plain.device is None and full.device is None                   # nothing was moved to a device
    # what passes these checks goes on to ask for the model
    for kw in (dict(obstacles=full, obstacle_model="markers"), dict(obstacles=full, obstacle_model="markers", obstacle_skin=0.0, beam_width=2),
               dict(obstacles=full), dict(obstacles=plain, obstacle_model="cylinder")):
        with pytest.raises(Exception) as e:
            call(**kw)
        assert not isinstance(e.value, ValueError), kw


@pytest.mark.parametrize("extra,match", [
    (["--goal", "0,1,0.9", "--obstacle-model", "markers"], "--obstacle-model markers needs --avoid"),
    (["--goal", "0,1,0.9", "--avoid", "a.pkl", "--obstacle-skin", "0.1"], "--obstacle-skin needs --obstacle-model markers"),
    (["--goal", "0,1,0.9", "--avoid", "a.pkl", "--obstacle-model", "markers", "--obstacle-skin", "-1"], "--obstacle-skin needs"),
    (["--goal", "0,1,0.9", "--avoid", "absent.pkl", "--obstacle-model", "markers"], "--avoid absent.pkl"),
])
def test_driver_argument_errors(tmp_path, extra, match):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "exp_GAMMAPrimitive", "gen_motion.py"), "--out", str(tmp_path / "out")] + extra,
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and match in r.stderr and "HIP device" not in r.stderr, r.stderr[-800:]
    assert not os.path.exists(tmp_path / "out")
