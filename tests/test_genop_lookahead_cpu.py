"""Look-ahead in the primitive search, on the CPU: the restatement tests/genop_lookahead_ref.py against the cylinder restatements it
extends (tests/genop_obstacles_ref.py, tests/genop_joint_ref.py) and against itself in float64, its rule on hand-made cases, and the
errors `generate_sequence_to_goal(lookahead=, lookahead_slack=)` and the driver's `--lookahead` raise before any device work."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import genop_joint_ref as jref
from tests import genop_lookahead_ref as lref
from tests import genop_obstacles_ref as oref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _rows(B, seed, jpb=3):
    """B rows: a frame each, joints whose pelvis walks about 0.1 m a frame -> R0 [B,3,3], T0 [B,3], J [B,20,jpb,3] float32"""
    g = np.random.default_rng(seed)
    yaw = g.uniform(-np.pi, np.pi, B)
    R0 = np.zeros((B, 3, 3))
    R0[:, 0, 0], R0[:, 0, 1], R0[:, 1, 0], R0[:, 1, 1], R0[:, 2, 2] = np.cos(yaw), -np.sin(yaw), np.sin(yaw), np.cos(yaw), 1.0
    T0 = g.normal(size=(B, 3)) * [1.5, 1.5, 0.05]
    J = g.normal(size=(B, 20, jpb, 3)) * 0.05
    J[:, :, 0, 1] += np.arange(20) * 0.1 * g.uniform(0.5, 1.5, (B, 1))
    J[:, :, 0, 2] += 0.9
    return R0.astype(f32), T0.astype(f32), J.astype(f32)


def _sets(S, O, T, seed):
    """S sets of O tracks that wander about the origin, counts ragged -> xy [S,O,T,2], radius [S,O], count [S]"""
    g = np.random.default_rng(seed)
    xy = (g.normal(size=(S, O, 1, 2)) * 2.0 + np.cumsum(g.normal(size=(S, O, T, 2)) * 0.05, 2)).astype(f32)
    return xy, g.uniform(0.1, 0.3, (S, O)).astype(f32), np.array([(3 * s + 1) % (O + 1) for s in range(S)])


def _same(a, b):
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(((a == b) | (torch.isnan(a.double()) & torch.isnan(b.double()))).all())


def _joint_state(b, N, seed, H, slack=0.1, nan_row=None):
    R0, T0, J = _rows(b * N, seed)
    if nan_row is not None:
        J[nan_row[0], nan_row[1], 0, 0] = np.nan
    g = torch.Generator().manual_seed(seed)
    p = lref.pelvis(R0, T0, J, torch.float32).reshape(b, N, 20, 2)
    return {"pelvis": p, "track": p[:, :, 2:], "cost": torch.rand(b, N, generator=g), "terms": torch.rand(b, N, 5, generator=g),
            "colliding": torch.rand(b, N, generator=g) < 0.2, "w": 1.3, "margin": 0.6, "body_radius": 0.15, "lookahead": H, "lookahead_slack": slack,
            "members": list(range(b)), "choice": {m: int(torch.randint(0, N, (1,), generator=g)) for m in range(b)}}


# ---- H = 0 is the restatement of the cylinder models, exactly ------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_lookahead_zero_is_the_obstacle_restatement(dtype):
    B, S, O, T = 12, 3, 5, 9
    R0, T0, J = _rows(B, 1)
    J[4, 7, 0, 1] = np.nan                                                       # a NaN pelvis in one predicted frame
    xy, radius, _ = _sets(S, O, T, 2)
    count, set_of_row = np.array([1, 4, 2]), np.arange(B) % S
    p = oref.world_pelvis(R0, T0, J, dtype).numpy()
    for frame0 in (-3, 0, 4):                                                    # both clamps
        want = oref.row_terms(R0, T0, J, xy, radius, count, set_of_row, frame0, 0.6, 0.1, dtype)
        got = lref.row_terms(p, xy, radius, count, set_of_row, frame0, 0.6, 0.1, 0, 0.1, dtype)
        for k in ("clearance", "term", "hit"):
            assert _same(got[k], want[k]), (frame0, k)
        assert bool(torch.isnan(want["term"][4])) and bool((want["term"] > 0).any())
    # the slack is not read at H = 0
    want = oref.row_terms(R0, T0, J, xy, radius, count, set_of_row, 0, 0.6, 0.1, dtype)
    assert _same(lref.row_terms(p, xy, radius, count, set_of_row, 0, 0.6, 0.1, 0, 7.0, dtype)["term"], want["term"])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_lookahead_zero_is_the_joint_restatement(dtype):
    b, N = 4, 5
    for seed, nan_row in ((3, None), (4, (7, 11))):
        st = _joint_state(b, N, seed, 0, nan_row=nan_row)
        for i in range(b):
            got, want = lref.member_step(dict(st), i, dtype), jref.member_step(dict(st), i, dtype)
            for k in ("term", "clearance", "hit", "joint_cost", "finite", "cls"):
                assert _same(got[k], want[k]), (seed, i, k)
            assert got["choice"] == want["choice"]
        assert _same(lref.crowd_clearance(dict(st), dtype), jref.crowd_clearance(dict(st), dtype))
        a, c = dict(st, choice=dict(st["choice"])), dict(st, choice=dict(st["choice"]))
        assert torch.equal(lref.sweeps(a, 2, dtype)["choice_trace"], jref.sweeps(c, 2, dtype)["choice_trace"]) and a["choice"] == c["choice"]


# ---- float32 against float64 ---------------------------------------------------------------------------------------------------------
def _ulp(x):
    """the spacing of float32 at magnitude x"""
    return float(np.spacing(np.float32(x)))


@pytest.mark.parametrize("H", [0, 1, 3, 8])
def test_float32_restatement_is_within_roundoff_of_float64(H):
    """Both variants start from the same float32 pelvis positions and tracks.  With X the largest magnitude among the coordinates,
    the predicted coordinates and the distances, and every float32 rounding at most half an ulp(X): d carries 1/2 ulp, h * d that times
    h plus 1/2, the sum 1/2 more: (h + 2) / 2 ulps per axis of p_h; the difference to a track 1/2 more; the norm of two such axes sqrt(2)
    times that, plus 2 ulps for the relative roundings of squares, sum and root (1.5 relative half-ulps of the distance, rounded up); r +
    body_radius and its subtraction 1; max(0, .) + h * slack 1 more.  At h = H: sqrt(2) (H + 3) / 2 + 4 ulps of X."""
    B, S, O, T = 40, 2, 6, 30
    R0, T0, J = _rows(B, 10 + H)
    p = lref.pelvis(R0, T0, J, torch.float32)
    xy, radius, count = _sets(S, O, T, 11)
    count = np.array([O, 3])
    set_of_row = np.arange(B) % S
    c32 = lref.obstacle_clearances(p, xy, radius, count, set_of_row, 5, 0.3, H, 0.1, torch.float32, bits=True)
    c64 = lref.obstacle_clearances(p, xy, radius, count, set_of_row, 5, 0.3, H, 0.1, torch.float64)
    assert c32.dtype == np.float32 and c64.dtype == np.float64 and np.isfinite(c64).all()
    ahead = np.abs(lref.predicted(p, H, torch.float64)).max()
    X = max(float(np.abs(p).max()), float(ahead), float(np.abs(xy).max()))
    X = 2.0 * np.sqrt(2.0) * X                                                   # a distance between two such points
    bound = (np.sqrt(2.0) * (H + 3) / 2.0 + 4.0) * _ulp(X)
    err = float(np.abs(c32.astype(np.float64) - c64).max())
    print(f"| lookahead restatement H={H} | X {X:.3f} | max |c32 - c64| {err:.3e} | bound {bound:.3e} |")
    assert err <= bound, (H, err, bound)
    # the joint model: both people carry the prediction's error, the other's subtracted from the own: twice the per-axis share
    st = _joint_state(4, 6, 20 + H, H)
    big = max(float(np.abs(lref.predicted(st["pelvis"], H, torch.float64)).max()), float(np.abs(st["pelvis"]).max()))
    jb = (np.sqrt(2.0) * (2 * (H + 2) / 2.0 + 0.5) + 4.0) * _ulp(2.0 * np.sqrt(2.0) * big)
    for i in range(4):
        m = st["members"][i]
        a = lref.pair_clearances(st, i, lref._pelvis_of(st, torch.float32)[m], torch.float32, bits=True).double()
        c = lref.pair_clearances(st, i, lref._pelvis_of(st, torch.float64)[m], torch.float64)
        assert float((a - c).abs().max()) <= jb, (H, i, float((a - c).abs().max()), jb)


def test_pelvis32_is_the_fused_nesting():
    """three products of which two are fused: fma(R2, z, fma(R1, y, R0 x)) + T: four roundings of values below X = |R||j| + |T|"""
    R0, T0, J = _rows(64, 5)
    p32, p64 = lref.pelvis(R0, T0, J, torch.float32), lref.pelvis(R0, T0, J, torch.float64)
    X = float((np.abs(R0[:, None, :2]) @ np.abs(J[:, :, 0, :, None]))[..., 0].max() + np.abs(T0).max())
    assert p32.dtype == np.float32 and float(np.abs(p32 - p64).max()) <= 2.0 * _ulp(X)
    r, t, j = R0[3].astype(np.float64), T0[3].astype(np.float64), J[3, 6, 0].astype(np.float64)
    inner = f32(f32(R0[3, 0, 0]) * f32(J[3, 6, 0, 0]))
    mid = f32(r[0, 1] * j[1] + float(inner))                                     # one rounding of the exact product plus addend
    assert p32[3, 6, 0] == f32(f32(r[0, 2] * j[2] + float(mid)) + T0[3, 0])


# ---- the rule on hand-made cases -----------------------------------------------------------------------------------------------------
def _walker(x0, step, y=0.0):
    """pelvis [20,2]: x0 + step * t along x"""
    return np.stack([x0 + step * np.arange(20), np.full(20, y)], -1).astype(f32)


def test_predicted_overlap_costs_and_does_not_veto():
    """a walker at 0.1 m a frame towards a person who stands 4 m off: this primitive ends 2.1 m short (clear of a margin of 0.5 m by far),
    the next one would end 0.3 m short: inside the summed radii of 0.6 m"""
    p = _walker(0.0, 0.1)[None]
    xy = np.zeros((1, 1, 60, 2), f32)
    xy[..., 0] = 4.0
    args = (p, xy, np.full((1, 1), 0.3, f32), [1], [0], 0, 0.5, 0.3)
    for dtype in (torch.float32, torch.float64):
        dt = lref._np(dtype)
        now = lref.row_terms(*args, 0, 0.1, dtype)
        assert float(now["term"]) == 0.0 and float(now["clearance"]) > 1.4 and not bool(now["hit"])
        for H, slack in ((1, 0.1), (2, 0.1), (2, 0.05), (8, 0.3)):
            c = lref.obstacle_clearances(*args[:6], args[7], H, slack, dtype)
            assert (lref.obstacle_clearances(*args[:6], args[7], 0, slack, dtype) > 0.5).all()
            # h = 1 stands at 0.1 t + 1.8: within 0.6 m of x = 4 from frame 17 on (frame 16 stands at the very edge); c_t = h * slack exactly there, h = 1 the cheapest
            assert (c[0, 15:] == dt(1) * dt(f32(slack))).all() and (c[0, :14] > dt(f32(slack))).all()
            t = lref.row_terms(*args, H, slack, dtype)
            assert float(t["term"]) > 0.0 and float(t["clearance"]) == float(dt(f32(slack))) and not bool(t["hit"])
        # with a slack of margin / h nothing is left of a prediction h primitives ahead
        assert float(lref.row_terms(*args, 1, 0.5, dtype)["term"]) == 0.0
    # the joint model: two people 6.4 m apart walk at each other, 1.8 m a primitive each
    both = np.stack([_walker(0.0, 0.1), _walker(6.4, -0.1)])[:, None]
    st = {"pelvis": both, "cost": torch.zeros(2, 1), "terms": torch.zeros(2, 1, 5), "colliding": torch.zeros(2, 1, dtype=torch.bool), "w": 1.0,
          "margin": 0.5, "body_radius": 0.3, "members": [0, 1], "choice": {0: 0, 1: 0}, "lookahead_slack": 0.1}
    r0 = lref.member_step(dict(st, lookahead=0), 0, torch.float32)
    r1 = lref.member_step(dict(st, lookahead=1), 0, torch.float32)
    assert float(r0["term"]) == 0.0 and float(r0["clearance"]) > 0.5
    assert float(r1["term"]) > 0.0 and float(r1["clearance"]) == float(f32(0.1)) and not bool(r1["hit"]) and int(r1["cls"]) == 0
    assert float(lref.crowd_clearance(dict(st, lookahead=1), torch.float32).min()) > 0.5          # the crowd as written stays at h = 0


@pytest.mark.parametrize("frame", [1, 19])
def test_nan_at_frame_1_or_19_gives_a_nan_row(frame):
    p = np.stack([_walker(0.0, 0.1), _walker(0.0, 0.1, y=1.0)])
    p[0, frame, 0] = np.nan
    xy = np.zeros((1, 1, 60, 2), f32)
    xy[..., 0] = 4.0
    args = (p, xy, np.full((1, 1), 0.3, f32), [1], [0, 0], 0, 0.5, 0.3)
    for dtype in (torch.float32, torch.float64):
        now = lref.obstacle_clearances(*args[:6], args[7], 0, 0.1, dtype)
        assert np.isnan(now[0]).sum() == (1 if frame == 19 else 0)               # frame 1 is not scored today
        c = lref.obstacle_clearances(*args[:6], args[7], 2, 0.1, dtype)
        assert np.isnan(c[0]).all() and np.isfinite(c[1]).all()                  # max(0, NaN) has not become 0
        for tree in (False, True):
            t = lref.row_terms(*args, 2, 0.1, dtype, bits=tree)
            assert bool(torch.isnan(t["term"][0])) and bool(torch.isnan(t["clearance"][0])) and not bool(t["hit"][0])
            assert bool(torch.isfinite(t["term"][1]))
    # an empty set keeps the NaN: nobody to be clear of, but the row's own prediction is not a number
    none = lref.obstacle_clearances(p, xy, args[2], [0], [0, 0], 0, 0.3, 2, 0.1, torch.float32, bits=True)
    assert np.isnan(none[0]).all() and np.isposinf(none[1]).all()
    # the joint model: the row is NaN, and the other member does not see it
    both = np.stack([p[0], _walker(4.4, -0.1)])[:, None]
    st = {"pelvis": both, "cost": torch.zeros(2, 1), "terms": torch.zeros(2, 1, 5), "colliding": torch.zeros(2, 1, dtype=torch.bool), "w": 1.0,
          "margin": 0.5, "body_radius": 0.3, "members": [0, 1], "choice": {0: 0, 1: 0}, "lookahead": 2, "lookahead_slack": 0.1}
    for tree in (False, True):
        mine, other = lref.member_step(dict(st), 0, torch.float32, bits=tree), lref.member_step(dict(st), 1, torch.float32, bits=tree)
        assert bool(torch.isnan(mine["term"])) and int(mine["cls"]) == 2 and not bool(mine["hit"])
        assert bool(torch.isfinite(other["term"])) and int(other["cls"]) == 0


def test_infinite_pelvis_at_frame_1_or_19():
    """an infinite p(1) or p(19) alone gives an infinite displacement: every prediction stands infinitely far away, c_{t,h} = +inf drops
    out of the minimum and the row is today's; infinite at both with one sign gives inf - inf: a NaN displacement and a NaN row"""
    xy = np.zeros((1, 1, 60, 2), f32)
    xy[..., 0] = 1.5
    for bits in (False, True):
        p = np.stack([_walker(0.0, 0.1)] * 4)
        p[1, 1, 0], p[2, 19, 0], p[3, 1, 0], p[3, 19, 0] = np.inf, -np.inf, np.inf, np.inf
        at = (p, xy, np.full((1, 1), 0.3, f32), [1], [0] * 4, 0, 0.3)
        now, c = (lref.obstacle_clearances(*at, H, 0.1, torch.float32, bits=bits) for H in (0, 2))
        assert np.array_equal(c[1], now[1]) and np.array_equal(c[2], now[2]) and np.isposinf(now[2, 17]) and np.isfinite(now[1]).all()
        assert np.isnan(c[3]).all() and not np.isnan(now[3]).any() and (c[0] <= now[0]).all() and (c[0] < now[0]).any()


def test_tree_sum_is_the_plain_sum_to_roundoff():
    """the wave reduction's tree and torch's sum add the same 18 penalties below the margin: they differ by the order only"""
    st = _joint_state(3, 7, 31, 3)
    for i in range(3):
        a, b = lref.member_step(dict(st), i, torch.float32), lref.member_step(dict(st), i, torch.float32, bits=True)
        assert _same(a["clearance"], b["clearance"]) and _same(a["hit"], b["hit"])
        assert float((a["term"] - b["term"]).abs().max()) <= 18 * 0.6 * 2.0 ** -23


# ---- generate_sequence_to_goal and the driver: the errors come before any device work ------------------------------------------------
def test_generate_sequence_to_goal_lookahead_errors_need_no_device():
    from egogen_amd.genop import MAX_LOOKAHEAD, GAMMAPrimitiveComboGenOP
    from egogen_amd.obstacles import MovingObstacles
    assert MAX_LOOKAHEAD == lref.MAX_LOOKAHEAD == 8
    op = GAMMAPrimitiveComboGenOP.__new__(GAMMAPrimitiveComboGenOP)      # no constructor: it asks for a device
    op.body_model, op.model = object(), None
    mk = lambda b: (np.zeros((2, b, 201), np.float32), np.zeros((2, b, 93), np.float32), np.zeros(10, np.float32), np.zeros(3, np.float32))
    call = lambda N=2, b=4, **kw: op.generate_sequence_to_goal(*mk(b), 2, N, **kw)
    plain = MovingObstacles.from_tracks(np.zeros((1, 4, 2)))
    full = MovingObstacles.from_tracks(np.zeros((1, 4, 2)), markers=np.zeros((1, 4, 67, 3)))
    ids = [0, 0, 1, 1]
    for H in (-1, 9, 1.5, "2", None, float("nan"), True):
        with pytest.raises(ValueError, match="lookahead must be an integer in"):
            call(obstacles=plain, lookahead=H)
    for slack in (-0.01, float("nan"), float("inf"), "a"):
        for H in (0, 2):
            with pytest.raises(ValueError, match="lookahead_slack"):
                call(groups=ids, lookahead=H, lookahead_slack=slack)
    with pytest.raises(ValueError, match="needs obstacles= or groups="):
        call(lookahead=1)
    with pytest.raises(ValueError, match="cylinder models only"):
        call(obstacles=full, obstacle_model="markers", lookahead=1)
    with pytest.raises(ValueError, match="cylinder models only"):
        call(groups=ids, pair_model="markers", lookahead=1)
    with pytest.raises(ValueError, match="cylinder models only"):
        call(obstacles=plain, groups=ids, pair_model="markers", lookahead=8)
    with pytest.raises(ValueError, match="beam_width must be 1"):         # a beam with groups stays refused
        call(groups=ids, lookahead=2, beam_width=2)
    assert plain.device is None and full.device is None                   # nothing was moved to a device
    # what passes these checks goes on to ask for the model
    for kw in (dict(obstacles=plain, lookahead=8), dict(obstacles=plain, lookahead=2, beam_width=2), dict(groups=ids, lookahead=1, lookahead_slack=0.0),
               dict(obstacles=full, groups=ids, lookahead=np.int64(3)), dict(lookahead=0), dict(lookahead=0, lookahead_slack=0.3),
               dict(obstacles=full, obstacle_model="markers", lookahead=0), dict(groups=ids, lookahead=2.0)):
        with pytest.raises(Exception) as e:
            call(**kw)
        assert not isinstance(e.value, ValueError), kw


PEOPLE = "0,0,0:0.3,3,0.9;0.8,0,0:0.5,3,0.9"


@pytest.mark.parametrize("extra,match", [
    (["--goal", "0,1,0.9", "--lookahead", "2"], "--lookahead needs --avoid or --people"),
    (["--people", PEOPLE, "--lookahead", "9"], "--lookahead takes 0 to 8"),
    (["--people", PEOPLE, "--lookahead", "-1"], "--lookahead takes 0 to 8"),
    (["--people", PEOPLE, "--lookahead", "1.5"], "invalid int value"),
    (["--goal", "0,1,0.9", "--avoid", "a.pkl", "--lookahead", "2", "--lookahead-slack", "-1"], "--lookahead-slack needs"),
    (["--goal", "0,1,0.9", "--avoid", "a.pkl", "--lookahead", "2", "--lookahead-slack", "nan"], "--lookahead-slack needs"),
    (["--goal", "0,1,0.9", "--avoid", "a.pkl", "--lookahead-slack", "0.2"], "--lookahead-slack needs --lookahead above 0"),
    (["--goal", "0,1,0.9", "--avoid", "a.pkl", "--obstacle-model", "markers", "--lookahead", "1"], "cylinder models only"),
    (["--people", PEOPLE, "--pair-model", "markers", "--lookahead", "1"], "cylinder models only"),
    (["--avoid", "a.pkl", "--lookahead", "1"], "--avoid needs --goal"),
    (["--goal", "0,1,0.9", "--avoid", "absent.pkl", "--lookahead", "2"], "--avoid absent.pkl"),
])
def test_driver_argument_errors(tmp_path, extra, match):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "exp_GAMMAPrimitive", "gen_motion.py"), "--out", str(tmp_path / "out")] + extra,
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and match in r.stderr and "HIP device" not in r.stderr, r.stderr[-800:]
    assert not os.path.exists(tmp_path / "out")
