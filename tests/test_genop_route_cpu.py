"""Waypoint routes without a device: `Routes` (egogen_amd/route.py), the restatement of the route rule in both precisions
(tests/genop_route_ref.py), the argument checks of `generate_sequence_to_goal(route=)` that come before any device work, the
`wpath` a route result saves and `MotionSet` reads back, and the route syntax of exp_GAMMAPrimitive/gen_motion.py."""
import importlib.util
import os
import pickle

import numpy as np
import pytest
import torch

from tests import genop_route_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIT_MARGIN = 0.05           # the obstacle tests' margin for a discrete outcome


# ---- Routes --------------------------------------------------------------------------------------------------------------------
def test_routes_from_lists_and_padded():
    from egogen_amd import Routes
    r = Routes.from_lists([[[0, 1, 0.9], [1, 1, 0.9], [2, 2, 0.9]], torch.tensor([[3.0, 3.0, 0.9]])], pass_radius=0.4)
    assert len(r) == 2 and r.waypoints.shape == (2, 3, 3) and r.waypoints.dtype == np.float32 and r.count.tolist() == [3, 1]
    assert r.count.dtype == np.int32 and r.pass_radius == 0.4
    assert np.array_equal(r.last(), np.array([[2, 2, 0.9], [3, 3, 0.9]], np.float32))
    assert np.array_equal(r.waypoints[1, 1:], np.zeros((2, 3), np.float32))
    pad = np.full((2, 3, 3), np.nan)
    pad[0], pad[1, 0] = r.waypoints[0], r.waypoints[1, 0]          # whatever stands behind the live waypoints is not read
    q = Routes(pad, [3, 1], 0.4)
    assert np.array_equal(q.waypoints, r.waypoints) and np.array_equal(q.field_of, r.field_of)
    assert [w.tolist() for w in q.lists()] == [r.waypoints[0].tolist(), r.waypoints[1, :1].tolist()]
    assert Routes.from_lists([[[0, 0, 0]]]).pass_radius == 0.5


@pytest.mark.parametrize("make,match", [
    (lambda R: R.from_lists([[[0, 0, 0]], []]), "empty"),
    (lambda R: R.from_lists([]), "no route"),
    (lambda R: R(np.zeros((2, 3, 3)), [1, 0]), "empty route"),
    (lambda R: R.from_lists([[[0, 0, 0], [0, float("nan"), 0]]]), "not finite"),
    (lambda R: R.from_lists([[[0, float("inf"), 0]]]), "not finite"),
    (lambda R: R.from_lists([np.zeros((17, 3))]), "at most 16"),
    (lambda R: R(np.zeros((1, 17, 3)), [3]), "at most 16"),
    (lambda R: R(np.zeros((1, 3, 3)), [4]), "padded length"),
    (lambda R: R.from_lists([[[0, 0, 0]]], pass_radius=-0.1), "pass_radius"),
    (lambda R: R.from_lists([[[0, 0, 0]]], pass_radius=float("nan")), "pass_radius"),
    (lambda R: R.from_lists([[[0, 0, 0]]], pass_radius=float("inf")), "pass_radius"),
    (lambda R: R.from_lists([[[0, 0]]]), r"\[n,3\]"),
    (lambda R: R(np.zeros((2, 3, 3)), [1]), "one per route"),
    (lambda R: R(np.zeros((2, 3)), [1, 1]), r"\[b,P,3\]"),
])
def test_routes_errors(make, match):
    from egogen_amd.route import Routes
    with pytest.raises(ValueError, match=match):
        make(Routes)


def test_field_goals_of_routes_that_share_waypoints():
    from egogen_amd.route import Routes
    door, table, sofa, bed = [1, 0, 0.9], [2, 1, 0.9], [3, 3, 0.9], [0, 4, 0.9]
    r = Routes.from_lists([[door, table, sofa], [table, door], [bed], [sofa, bed, door, sofa]])
    assert np.array_equal(r.field_goals(), np.asarray([door, table, sofa, bed], np.float32))
    assert r.field_of.dtype == np.int32 and r.field_of.tolist() == [[0, 1, 2, 0], [1, 0, 0, 0], [3, 0, 0, 0], [2, 3, 0, 2]]
    for i, way in enumerate(r.lists()):
        assert np.array_equal(r.field_goals()[r.field_of[i, :len(way)]], way)


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def test_restatements_agree_on_the_constructed_cases():
    c = ref.constructed([ref.KINDS[i % len(ref.KINDS)] for i in range(65)], 5)
    run = lambda dt: ref.advance(c["pelvis"], c["R"], c["T"], c["waypoints"], c["count"], c["cursor"], c["radius"], dt, c["reached"], c["field_of"])
    o64, o32 = run(np.float64), run(np.float32)
    live = np.isfinite(o64["slack"])
    assert live.sum() >= 40 and o64["slack"][live].min() >= HIT_MARGIN              # the margin of every decision
    for o in (o64, o32):
        assert np.array_equal(o["cursor"], c["want_cursor"]) and np.array_equal(o["reached"], c["want_reached"])
        assert np.array_equal(o["field_index"], c["field_of"][np.arange(65), c["want_cursor"]])
        assert np.array_equal(np.isnan(o["pass_dist"]), np.asarray([k == "nan" for k in c["kinds"]]))
    moved = o64["cursor"] != np.clip(c["cursor"], 0, None)
    assert moved.any() and (~moved).any()                                           # both outcomes are there
    assert np.array_equal(o64["route_goal"], o32["route_goal"]) and np.array_equal(o64["goal"], o32["goal"])
    ok = ~np.isnan(o64["pass_dist"])
    assert np.abs(o64["pass_dist"][ok] - o32["pass_dist"][ok].astype(np.float64)).max() < 1e-5
    seed = [i for i, k in enumerate(c["kinds"]) if k == "seed_only"]
    assert np.allclose(o64["pass_dist"][seed], 0.18, atol=1e-6)                     # frames 0 and 1 were nearer: they do not count


def test_replay_carries_the_cursor():
    c = ref.constructed(["cascade", "wrong_order"], 9)
    K = 3
    rec = lambda a: np.stack([a] * K)
    tr = ref.replay(rec(c["pelvis"]), rec(c["R"]), rec(c["T"]), c["waypoints"], c["count"], c["radius"], np.float64)
    # the same primitive three times: the cascade is done after the first; the second waypoint of wrong_order, at frames 4 and 5,
    # is passed by the second (a new primitive starts its search at frame 2 again)
    assert tr["cursor"].tolist() == [[2, 1], [2, 2], [2, 2]]
    assert np.array_equal(tr["route_goal"][1, 1], c["waypoints"][1, 1]) and np.array_equal(tr["route_goal"][0, 1], c["waypoints"][1, 0])


# ---- generate_sequence_to_goal: the errors come before any device work ---------------------------------------------------------
def test_generate_sequence_to_goal_route_errors_need_no_device():
    """Every call below fails on the code before routes with a TypeError for the unknown `route` keyword."""
    from egogen_amd.genop import GAMMAPrimitiveComboGenOP
    from egogen_amd.route import Routes
    op = GAMMAPrimitiveComboGenOP.__new__(GAMMAPrimitiveComboGenOP)      # no constructor: it asks for a device
    op.body_model, op.model, op.testconfig = object(), None, {}
    b = 2
    data, bparams, betas = np.zeros((2, b, 201), np.float32), np.zeros((2, b, 93), np.float32), np.zeros(10, np.float32)
    r = Routes.from_lists([[[0, 1, 0.9], [1, 1, 0.9]], [[2, 2, 0.9]]])
    call = lambda goal=None, **kw: op.generate_sequence_to_goal(data, bparams, betas, goal, 2, 2, **kw)
    with pytest.raises(ValueError, match="beam_width must be 1"):
        call(route=r, beam_width=2)
    with pytest.raises(ValueError, match="contradicts the route"):
        call(np.zeros(3, np.float32), route=r)
    with pytest.raises(ValueError, match="contradicts the route"):
        call(r.last()[::-1].copy(), route=r)
    with pytest.raises(ValueError, match="below goal_thresh"):
        call(route=r, goal_thresh=0.6)
    with pytest.raises(ValueError, match="below goal_thresh"):
        call(route=Routes.from_lists(r.lists(), pass_radius=0.05))         # the default goal_thresh is 0.1
    with pytest.raises(TypeError, match="Routes"):
        call(route=[[0, 1, 0.9]])
    with pytest.raises(ValueError, match="2 routes"):
        call(route=Routes.from_lists([[[0, 0, 0.9]]] * 3))
    from egogen_amd import _lib
    for goal in (None, r.last(), torch.from_numpy(r.last())):                # accepted: the next stop is the missing model
        with pytest.raises(_lib.EgxError, match="build_model"):
            call(goal, route=r)


# ---- save / read back ----------------------------------------------------------------------------------------------------------
def _handmade_result(with_route):
    from egogen_amd.genop import PrimitiveSequence
    K, b = 2, 2
    g = np.random.default_rng(3)
    f = lambda *s: g.normal(size=s).astype(np.float32)
    rot = np.tile(np.eye(3, dtype=np.float32), (K, b, 1, 1))
    way = np.zeros((b, 3, 3), np.float32)
    way[0], way[1, :2] = [[1, 0, 0.9], [2, 1, 0.9], [3, 3, 0.9]], [[0, 4, 0.9], [5, 5, 0.9]]
    count = np.asarray([3, 2], np.int32)
    search = {k: None for k in PrimitiveSequence.SEARCH_FIELDS}
    search.update(goal=way[np.arange(b), count - 1], n_valid=np.asarray([K, 1]))
    if with_route:
        search.update(route_waypoints=way, route_count=count, route_cursor=np.zeros((K, b), np.int32), route_goal=np.zeros((K, b, 3), np.float32),
                      route_pass_dist=np.zeros((K, b), np.float32), pass_radius=0.5)
    return PrimitiveSequence(f(K, b, 20, 67, 3), f(K, b, 20, 93), rot, f(K, b, 3), f(K, b, 20, 3), f(K, b, 128), f(b, 10), "male",
                             rot[0], f(b, 3), search=search), way, count


def test_save_writes_the_route_and_motionset_reads_it_back(tmp_path):
    from egogen_amd.metrics import MotionSet
    res, way, count = _handmade_result(True)
    plain, _, _ = _handmade_result(False)
    assert plain.route_waypoints is None and all(getattr(plain, k) is None for k in plain.ROUTE_FIELDS)
    paths = [res.save(str(tmp_path / "route"), i, man_id=f"r{i}") for i in range(2)]
    old = [plain.save(str(tmp_path / "plain"), i, man_id=f"r{i}") for i in range(2)]
    for i, p in enumerate(paths):
        with open(p, "rb") as fh:
            node = pickle.load(fh)
        first = res.rotmat[0, i] @ res.pelvis[0, i, 0] + res.transl[0, i]
        assert node["wpath"].shape == (1 + count[i], 3) and np.array_equal(node["wpath"][1:], way[i, :count[i]])
        assert np.allclose(node["wpath"][0], first, atol=1e-6) and len(node["motion"]) == int(res.n_valid[i])
        with open(old[i], "rb") as fh:
            two = pickle.load(fh)
        assert two["wpath"].shape == (2, 3) and np.array_equal(two["wpath"][1], way[i, count[i] - 1])      # as before routes
        assert np.array_equal(two["wpath"][0], node["wpath"][0])
    ms = MotionSet.from_rollout_files(paths)
    assert [r.tolist() for r in ms.routes] == [way[0].tolist(), way[1, :2].tolist()]
    assert np.array_equal(ms.goals, way[np.arange(2), count - 1])
    ms_old = MotionSet.from_rollout_files(old)
    assert ms_old.routes is None and np.array_equal(ms_old.goals, ms.goals) and np.array_equal(ms_old.frame_src, ms.frame_src)
    both = MotionSet.from_rollout_files([paths[0], old[1]])
    assert both.routes[1] is None and np.array_equal(both.routes[0], way[0])
    # a wpath that cannot be a route (a navmesh path of 30 points; a NaN point) leaves the file measurable, without a route
    with open(paths[0], "rb") as fh:
        node = pickle.load(fh)
    for name, wpath in (("long", np.linspace([0, 0, 0.9], [9, 9, 0.9], 30).astype(np.float32)),
                        ("nan", np.asarray([[0, 0, 0.9], [1, np.nan, 0.9], [2, 2, 0.9]], np.float32))):
        other = str(tmp_path / f"motion_{name}.pkl")
        with open(other, "wb") as fh:
            pickle.dump(dict(node, wpath=wpath), fh)
        ms_other = MotionSet.from_rollout_files([other, paths[1]])
        assert ms_other.routes[0] is None and np.array_equal(ms_other.routes[1], way[1, :2])
        assert np.array_equal(ms_other.goals[1], way[1, 1]) and (name == "nan" or np.array_equal(ms_other.goals[0], wpath[-1]))
    assert MotionSet.from_rollout_files([str(tmp_path / "motion_long.pkl")]).routes is None
    seq = MotionSet.from_sequences(res)
    assert [r.tolist() for r in seq.routes] == [r.tolist() for r in ms.routes] and np.array_equal(seq.goals, ms.goals)
    assert MotionSet.from_sequences(plain).routes is None


# ---- the driver's route syntax -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gen_motion():
    spec = importlib.util.spec_from_file_location("gen_motion_under_test", os.path.join(ROOT, "exp_GAMMAPrimitive", "gen_motion.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_gen_motion_parses_routes(gen_motion):
    pts = gen_motion.parse_goal_route("1,2,0.9;3,4,0.9;-5,6.5,0.9")
    assert pts.tolist() == [[1, 2, 0.9], [3, 4, 0.9], [-5, 6.5, 0.9]]
    people, routes = gen_motion.parse_people_routes("0,0,0:1,2,0.9>3,4,0.9;2,0,90:5,5,0.9;")
    assert people.tolist() == [[0, 0, 0, 3, 4, 0.9], [2, 0, 90, 5, 5, 0.9]]
    assert [r.tolist() for r in routes] == [[[1, 2, 0.9], [3, 4, 0.9]], [[5, 5, 0.9]]]
    for bad in ("1,2;3,4,5", "1,2,3;;4,5,6", "1,2,x;1,2,3", "1,2,3;1,2,nan"):
        with pytest.raises(ValueError):
            gen_motion.parse_goal_route(bad)
    for bad in ("0,0:1,2,3>4,5,6", "0,0,0:1,2,3>4,5", "0,0,0", "0,0,0:1,2,3>", "0,0,0:1,2,3:4,5,6>7,8,9", ";"):
        with pytest.raises(ValueError):
            gen_motion.parse_people_routes(bad)


@pytest.mark.parametrize("argv,message", [
    (["--goal", "1,2,0.9;3,4"], '--goal takes x,y,z, or "x,y,z;x,y,z;..." for a route'),
    (["--goal", "1,2,0.9;3,4,0.9", "--beam-width", "2"], 'a route (";" in --goal) is the greedy search'),
    (["--people", "0,0,0:1,2,0.9>3,4"], '--people takes "x,y,yaw_deg:gx,gy,gz>gx,gy,gz..."'),
    (["--goal", "1,2,0.9", "--pass-radius", "0.4"], "--pass-radius needs a route"),
    (["--people", "0,0,0:1,2,0.9;1,0,0:3,4,0.9", "--pass-radius", "0.4"], "--pass-radius needs a route"),
    (["--pass-radius", "0.4"], "--pass-radius needs a route")])
def test_gen_motion_rejects_bad_route_arguments(gen_motion, argv, message, capsys):
    """argparse's error, before the models and the device, with the message of the route branch (the code before routes also
    exits with status 2 on some of these, for an unknown flag: the text tells them apart)"""
    with pytest.raises(SystemExit) as e:
        gen_motion.main(argv)
    err = capsys.readouterr().err
    assert e.value.code == 2 and message in err, err
