"""Waypoint routes on the device: the entry egx_route_advance (csrc/genop_route.hip) against the restatement of
tests/genop_route_ref.py, `generate_sequence_to_goal(route=)` against its own records, and egx_route_metrics
(csrc/motion_metrics.hip) against its float64 restatement.

Yardsticks, all the project's own (tests/genop_gpu_helpers.py).  Values (route_pass_dist, the distance the selection scored): `held()`,
the device's error against float64 at most R = 3 x the float32 restatement's; route_pass_dist pooled over at least MIN_GROUP
sequences.  Discrete outcomes (cursors, flags, field indices) exactly, on constructed cases whose float64 slack - the least
|distance - pass_radius| over the distances that decided something - is at least HIT_MARGIN = 0.05 m, four orders above float32
round-off at these coordinates; the slack and the presence of both outcomes are asserted.  The cursor trace of a whole search is
replayed from the returned records in float64 and compared on the sequence-steps whose slack is at least 1e-4 m (a sequence is
left out from its first closer step on); their share is capped by UNDECIDABLE_CAP.  Copies (goal, route_goal) bit for bit;
egx_route_metrics' approach_min to 1e-12: both sides are float64, the tolerance of the metrics tests."""
import numpy as np
import pytest
import torch

from tests import genop_route_ref as ref
from tests.genop_gpu_helpers import (CFG_RF, MIN_GROUP, POOL, UNDECIDABLE_CAP, W_TEST, _advance_select, _inputs, _vp, held, patched_loop,
                                     search_world, small_world)  # noqa: F401
from tests.test_genop_policy_gpu import policy_world  # noqa: F401

pytestmark = pytest.mark.gpu
HIT_MARGIN = 0.05           # the obstacle tests' margin for a discrete outcome
DECIDABLE = 1e-4


# ---- the entry -----------------------------------------------------------------------------------------------------------------
def _advance(c, with_index=True, radius=None, b=None, P=None):
    """egx_route_advance on the numpy inputs of `c` (ref.constructed's keys) into NaN / -7 filled outputs (pass_dist: -1) -> dict of numpy arrays"""
    from egogen_amd import _lib
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda().contiguous()
    i = {k: dev(c[k]) for k in ("pelvis", "R", "T", "waypoints", "count", "field_of")}
    n = len(c["count"]) if b is None else b
    o = {"cursor": dev(c["cursor"]), "reached": dev(c["reached"]), "goal": torch.full((n, 3), float("nan"), device="cuda"),
         "field_index": torch.full((n,), -7, dtype=torch.int32, device="cuda"), "route_cursor": torch.full((n,), -7, dtype=torch.int32, device="cuda"),
         "route_goal": torch.full((n, 3), float("nan"), device="cuda"),
         "pass_dist": torch.full((n,), -1.0, device="cuda")}          # NaN is a legitimate output there: -1 marks "not written"
    _lib.check(_lib.load().egx_route_advance(
        _vp(i["pelvis"]), _vp(i["R"]), _vp(i["T"]), _vp(i["waypoints"]), _vp(i["count"]), _vp(i["field_of"]), n,
        c["waypoints"].shape[1] if P is None else P, float(c["radius"] if radius is None else radius), _vp(o["cursor"]), _vp(o["goal"]),
        _vp(o["field_index"]) if with_index else None, _vp(o["reached"]), _vp(o["route_cursor"]), _vp(o["route_goal"]), _vp(o["pass_dist"]),
        _lib.current_stream_ptr()), "egx_route_advance")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def _restated(c, dtype):
    return ref.advance(c["pelvis"], c["R"], c["T"], c["waypoints"], c["count"], c["cursor"], c["radius"], dtype, c["reached"], c["field_of"])


@pytest.mark.parametrize("b,with_index", [(1, True), (65, True), (65, False), (77, True)])
def test_route_advance_constructed_cases(b, with_index):
    """b = 1, and b = 65: more sequences than a block's four waves, with a ragged tail; counts 1, 2, 3 and 16 in one launch with
    P = 16; every kind of ref.KINDS.  b = 77 (ragged too) leaves 71 sequences without a NaN frame: route_pass_dist is pooled over at
    least MIN_GROUP of them for held(); at b = 65 only 60 remain, and each is held to 1e-6 m of float64 instead."""
    kinds = ["cascade"] if b == 1 else [ref.KINDS[i % len(ref.KINDS)] for i in range(b)]
    c = ref.constructed(kinds, 5)
    o64, o32 = _restated(c, np.float64), _restated(c, np.float32)
    live = np.isfinite(o64["slack"])
    assert o64["slack"][live].min() >= HIT_MARGIN and np.array_equal(o64["cursor"], c["want_cursor"])
    if b > 1:
        moved = o64["cursor"] != np.clip(c["cursor"], 0, None)
        assert moved.any() and (~moved).any() and set(c["count"].tolist()) >= {1, 2, 3, 16}
        assert (c["reached"] != c["want_reached"]).any() and (c["want_reached"] == 1).any()          # cleared, and kept
    got = _advance(c, with_index)
    assert np.array_equal(got["cursor"], c["want_cursor"]) and np.array_equal(got["route_cursor"], c["want_cursor"])
    assert np.array_equal(got["reached"], c["want_reached"])
    assert np.array_equal(got["goal"].view(np.int32), o64["goal"].view(np.int32))                   # a copy: bit for bit
    assert np.array_equal(got["route_goal"].view(np.int32), o64["route_goal"].view(np.int32))
    assert np.array_equal(got["field_index"], o64["field_index"] if with_index else np.full(b, -7, np.int32))
    nan = np.asarray([k == "nan" for k in kinds])
    assert np.array_equal(np.isnan(got["pass_dist"]), nan)
    assert ((~nan).sum() >= MIN_GROUP) == (b == 77)
    if (~nan).sum() >= MIN_GROUP:
        held(f"route_advance b={b}", "pass_dist", got["pass_dist"][~nan], o64["pass_dist"][~nan], o32["pass_dist"][~nan])
    else:
        assert np.abs(got["pass_dist"][~nan].astype(np.float64) - o64["pass_dist"][~nan]).max() < 1e-6


def test_route_advance_on_walker_records(small_world):
    """The records egx_primitive_advance_select writes for the 65 walkers of the pool, each in a world frame of its own, and
    routes of 1 to 16 waypoints scattered round each walker's track: cursors against float64 where the slack decides, the distance
    by held()."""
    d = _inputs(small_world, POOL)
    rec = _advance_select(d, list(range(POOL)), [0] * POOL, 1, 127, CFG_RF)
    g = np.random.default_rng(11)
    pelvis, R, T = rec["pelvis"].cpu().numpy(), rec["R"].cpu().numpy(), rec["T"].cpu().numpy()
    x, y = ref.world_xy(pelvis, R, T, np.float64)
    P = 16
    count = (np.arange(POOL) % P + 1).astype(np.int32)
    at = g.integers(0, 20, size=(POOL, P))                       # a waypoint sits some centimetres beside a frame of the track
    way = np.stack([np.take_along_axis(x, at, 1), np.take_along_axis(y, at, 1), np.full((POOL, P), 0.9)], -1) + g.normal(size=(POOL, P, 3)) * 0.08
    c = {"pelvis": pelvis, "R": R, "T": T, "waypoints": way.astype(np.float32), "count": count, "radius": 0.1,
         "cursor": (g.integers(0, 16, size=POOL) % count).astype(np.int32), "reached": g.integers(0, 2, size=POOL).astype(np.int32),
         "field_of": g.integers(0, 30, size=(POOL, P)).astype(np.int32)}
    o64, o32 = _restated(c, np.float64), _restated(c, np.float32)
    got = _advance(c)
    ok = o64["slack"] >= DECIDABLE
    assert (~ok).mean() <= UNDECIDABLE_CAP
    moved = o64["cursor"] != c["cursor"]
    assert moved[ok].sum() >= 10 and (~moved[ok]).sum() >= 10 and (o64["cursor"] - c["cursor"]).max() >= 2       # cascades among them
    for k in ("cursor", "reached", "field_index"):
        assert np.array_equal(got[k][ok], o64[k][ok]), k
    assert np.array_equal(got["route_cursor"], got["cursor"]) and np.array_equal(got["route_goal"], o64["route_goal"])
    assert np.array_equal(got["goal"][ok], o64["goal"][ok])
    held("route_advance walkers", "pass_dist", got["pass_dist"], o64["pass_dist"], o32["pass_dist"])


def test_route_advance_argument_checks():
    from egogen_amd import _lib
    lib = _lib.load()
    c = ref.constructed(["pass"], 1)
    for kw in ({"b": 0}, {"P": 0}, {"P": 17}, {"radius": -0.1}, {"radius": float("nan")}):
        with pytest.raises(_lib.EgxError, match="argument check failed"):
            _advance(c, **kw)
    z, zi = torch.zeros(64, device="cuda"), torch.zeros(64, dtype=torch.int32, device="cuda")
    full = [_vp(z), _vp(z), _vp(z), _vp(z), _vp(zi), _vp(zi), 1, 1, 0.5, _vp(zi), _vp(z), _vp(zi), _vp(zi), _vp(zi), _vp(z), _vp(z), None]
    for null in (0, 1, 2, 3, 4, 9, 10, 12, 13, 14, 15):
        a = list(full)
        a[null] = None
        assert lib.egx_route_advance(*a) == -1 and b"null" in lib.egx_last_error(), null
    a = list(full)
    a[5] = None                     # a field index buffer without field_of
    assert lib.egx_route_advance(*a) == -1 and b"field_of" in lib.egx_last_error()
    a[11] = None                    # neither: fine
    assert lib.egx_route_advance(*a) == 0
    torch.cuda.synchronize()


# ---- end to end ----------------------------------------------------------------------------------------------------------------
K, N = 4, 4
FIELDS = ("markers", "params", "rotmat", "transl", "pelvis", "z", "R0", "T0")
COMMON = ("goal", "choice", "cost", "cost_terms", "colliding", "status", "goal_dist", "n_valid")


def _kw(**extra):
    kw = dict(z=torch.randn(K, 3 * N, 128, generator=torch.Generator().manual_seed(40)), reproj_factor=CFG_RF, weights=W_TEST, goal_thresh=0.0,
              to_numpy=False)
    kw.update(extra)
    return kw


def _search(w, goal, route, k=K, n=N, b=3, **extra):
    """the search under patched_loop(no_host_wait=True) -> (result, the loop's state)"""
    with patched_loop(w["op"], "_search_loop", no_host_wait=True) as seen:
        res = w["op"].generate_sequence_to_goal(w["data"][:, :b].contiguous(), w["bparams"][:, :b].contiguous(), w["betas"][:b], goal, k, n,
                                                route=route, **_kw(**extra))
    assert seen.calls == [(k, b, n)]
    return res, seen.s


def _f64(t):
    return t.detach().cpu().double().numpy()


def _world(res, k, f):
    """world pelvis [b,3] of frame f of primitive k, float64"""
    return np.einsum("bij,bj->bi", _f64(res.rotmat[k]), _f64(res.pelvis[k, :, f])) + _f64(res.transl[k])


@pytest.fixture(scope="module")
def goal_run(search_world):
    w = search_world
    return w["op"].generate_sequence_to_goal(w["data"], w["bparams"], w["betas"], w["goal"], K, N, **_kw())


def _check_replay(name, res, route, pool_dist=True):
    """the cursor trace, the scored waypoints and the recorded distances of a route result against the float64 replay of its own
    records -> the replay"""
    way, count, radius = route.waypoints, route.count, route.pass_radius
    args = (_f64(res.pelvis), _f64(res.rotmat), _f64(res.transl), way, count, radius)
    t64, t32 = ref.replay(*args, np.float64), ref.replay(*args, np.float32)
    ok = np.logical_and.accumulate(t64["slack"] >= DECIDABLE, 0)            # [K,b]: a sequence counts up to its first undecidable step
    assert (~ok).mean() <= UNDECIDABLE_CAP, (name, t64["slack"])
    got = res.route_cursor.cpu().numpy()
    assert np.array_equal(got[ok], t64["cursor"][ok]), (name, got, t64["cursor"])
    assert np.array_equal(res.route_goal.cpu().numpy()[ok], t64["route_goal"][ok])
    assert np.array_equal(res.route_waypoints.cpu().numpy(), way) and np.array_equal(res.route_count.cpu().numpy(), count)
    assert res.pass_radius == radius and np.array_equal(res.goal.cpu().numpy(), route.last())
    if pool_dist:
        held(name, "pass_dist", res.route_pass_dist.cpu().numpy()[ok], t64["pass_dist"][ok], t32["pass_dist"][ok])
    return t64, ok


def test_route_of_one_waypoint_is_the_goal_run(search_world, goal_run):
    from egogen_amd.route import Routes
    w = search_world
    route = Routes.from_lists([[g.tolist()] for g in w["goal"]])
    for goal in (None, w["goal"]):
        res, s = _search(w, goal, route)
        for k in FIELDS:
            assert torch.equal(getattr(res, k), getattr(goal_run, k)), k
        for k in COMMON:
            assert torch.equal(res.search[k], goal_run.search[k]), k
        assert res.geo_dist is None and goal_run.geo_dist is None and goal_run.route_cursor is None
        assert int(res.route_cursor.abs().max()) == 0 and torch.equal(res.route_goal, w["goal"].cuda().expand(K, 3, 3))
        assert res.goal.data_ptr() != s["goal"].data_ptr()                   # the result's goal is not the buffer the loop rewrote
    # with a threshold the selection's flag against the only, hence last, waypoint is kept: the files stop as in the goal run
    kw = dict(goal_thresh=0.45)
    base = w["op"].generate_sequence_to_goal(w["data"], w["bparams"], w["betas"], w["goal"], K, N, **_kw(**kw))
    res, s = _search(w, None, route, **kw)
    assert torch.equal(res.n_valid, base.n_valid) and torch.equal(res.goal_dist, base.goal_dist)
    assert torch.equal(s["reached"].ne(0), res.goal_dist < 0.45)


def test_route_through_the_seed_pelvis(search_world, goal_run):
    """The first waypoint is the seed's own world pelvis, the second is `goal`.  The operator of `search_world` runs a seeded
    random-init prior, whose first predicted frame stands 1.2 to 1.5 m from the seed frames (the goal run's own records say so,
    asserted below), and the seed frames do not count: so the radius of this route is 3 m, which the waypoint is passed with in
    primitive 0 with a slack of more than a metre.  goal_thresh = 0.5 <= pass_radius."""
    from egogen_amd.route import Routes
    w = search_world
    start = _world(goal_run, 0, 1)
    jump = np.linalg.norm((_world(goal_run, 0, 2) - start)[:, :2], axis=1)
    assert 1.0 < jump.min() and jump.max() < 2.0, jump
    route = Routes.from_lists([[start[i], w["goal"][i].numpy()] for i in range(3)], pass_radius=3.0)
    res, s = _search(w, None, route, goal_thresh=0.5)
    t64, ok = _check_replay("seed pelvis", res, route, pool_dist=False)
    assert ok.all() and t64["slack"][0].min() >= HIT_MARGIN
    assert res.route_cursor[0].tolist() == [1, 1, 1] and bool(res.route_cursor.eq(1).all())
    assert torch.equal(res.route_goal[0].cpu(), torch.from_numpy(route.waypoints[:, 0]))
    assert torch.equal(res.route_goal[1:].cpu(), w["goal"].expand(K - 1, 3, 3)) and torch.equal(s["goal"].cpu(), w["goal"])
    assert torch.equal(s["route_state"], res.route_cursor[-1]) and torch.equal(res.goal.cpu(), w["goal"])
    assert int(s["reached"][0].abs().sum()) == 0                                 # scored against an intermediate point
    print("primitives 0 the selection called reached:", int((res.goal_dist[0] < 0.5).sum()), "of 3")
    assert torch.equal(s["reached"][1:].ne(0), res.goal_dist[1:] < 0.5)          # from then on the flag is the selection's own
    # the goal term of the chosen rows: the 3-D distance of the last pelvis to the waypoint the primitive was scored against
    chosen = res.cost_terms[..., 0].gather(2, res.choice.long().unsqueeze(-1))[..., 0]
    assert torch.equal(chosen, res.goal_dist)
    target = np.concatenate([route.waypoints[None, :, 0], np.broadcast_to(w["goal"].numpy(), (K - 1, 3, 3))])          # [K,b,3]

    def dist(dtype):
        e = lambda t: t.detach().cpu().numpy().astype(dtype)
        R, p, T = e(res.rotmat), e(res.pelvis[:, :, 19]), e(res.transl)
        wp = (R[..., 0] * p[..., None, 0] + R[..., 1] * p[..., None, 1]) + R[..., 2] * p[..., None, 2] + T
        d = target.astype(dtype) - wp
        return np.maximum(np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]), dtype(1e-12))
    held("seed pelvis", "goal_dist to goal, k >= 1", res.goal_dist[1:].cpu().numpy(), dist(np.float64)[1:], dist(np.float32)[1:])
    held("seed pelvis", "goal_dist to the waypoint, k = 0", res.goal_dist[:1].cpu().numpy(), dist(np.float64)[:1], dist(np.float32)[:1])


def test_route_with_a_far_first_waypoint_never_moves(search_world):
    from egogen_amd.route import Routes
    w = search_world
    route = Routes.from_lists([[[50.0, 0.0, 0.9], w["goal"][i].numpy()] for i in range(3)])
    res, s = _search(w, None, route, goal_thresh=0.1)
    t64, ok = _check_replay("far", res, route, pool_dist=False)
    assert ok.all() and t64["slack"].min() >= HIT_MARGIN
    assert int(res.route_cursor.abs().max()) == 0 and int(s["reached"].abs().max()) == 0 and res.n_valid.tolist() == [K] * 3
    assert torch.equal(res.route_goal.cpu(), torch.from_numpy(route.waypoints[:, 0]).expand(K, 3, 3))
    assert torch.equal(s["goal"].cpu(), torch.from_numpy(route.waypoints[:, 0])) and torch.equal(res.goal.cpu(), w["goal"])
    assert bool((res.route_pass_dist > 40).all())


def _via(goal_run, w, shift=None):
    """routes of search_world's three walkers: where the goal run stood at the first predicted frame of primitive 0 - more than a
    metre from the seed frames, so no seed frame is within the radius, and near where any candidate of primitive 0 begins - then
    the goal; `shift` [3,3] moves both, with the walkers' T0"""
    via = _world(goal_run, 0, 2)
    shift = np.zeros((3, 3)) if shift is None else np.asarray(shift, np.float64)
    return [[via[i] + shift[i], w["goal"][i].double().numpy() + shift[i]] for i in range(3)]


@pytest.fixture(scope="module")
def route_run(search_world, goal_run):
    from egogen_amd.route import Routes
    route = Routes.from_lists(_via(goal_run, search_world))
    res, s = _search(search_world, None, route)
    return res, s, route


def test_route_replay_plain(route_run):
    res, s, route = route_run
    t64, ok = _check_replay("plain", res, route, pool_dist=False)
    print("route_cursor", res.route_cursor.tolist(), "slack", t64["slack"].tolist())
    assert torch.equal(s["route_state"], res.route_cursor[-1])
    moved = t64["cursor"][-1] > 0
    assert moved.any()                                                          # the fixture's walkers do pass some waypoint


@pytest.mark.parametrize("pair_model", ["cylinder", "markers"])
def test_route_with_groups(search_world, goal_run, pair_model):
    from egogen_amd.route import Routes
    w = search_world
    T0 = torch.tensor([[0.0, 0.0, 0.0], [0.6, 0.0, 0.0], [5.0, 0.0, 0.0]])
    route = Routes.from_lists(_via(goal_run, w, T0.numpy()), pass_radius=1.0)
    res, s = _search(w, None, route, groups=[0, 0, 1], pair_model=pair_model, T0=T0)
    t64, ok = _check_replay(f"groups {pair_model}", res, route, pool_dist=False)
    print("route_cursor", res.route_cursor.tolist(), "slack", t64["slack"].tolist())
    assert res.search["pair_model"] == pair_model and res.choice_trace.shape == (K, 2, 3) and torch.equal(res.choice, res.choice_trace[:, -1])
    assert torch.equal(s["route_state"], res.route_cursor[-1]) and t64["cursor"].max() >= 1
    scored_last = torch.cat([torch.zeros(1, 3, dtype=torch.bool), res.route_cursor[:-1].cpu() == 1])         # [K,b]: count is 2
    assert int(s["reached"].cpu()[~scored_last].abs().sum()) == 0


def test_route_with_a_geodesic_field(search_world, goal_run):
    from egogen_amd.geodesic import GeodesicField
    from egogen_amd.route import Routes
    w, b = search_world, 2
    lists = _via(goal_run, w)[:b]
    lists[1][0] = lists[0][0]                                                      # the two share their first waypoint: three fields
    route = Routes.from_lists(lists, pass_radius=1.0)
    assert len(route.field_goals()) == 3 and route.field_of[:, :2].tolist() == [[0, 1], [0, 2]]
    free = np.ones((120, 120), bool)
    free[30:90, 65:67] = False            # x in [-3, 3], y in [0.5, 0.7]: between the walkers' start and their goals
    fld = GeodesicField.from_raster(free, np.array([-6.0, -6.0]), 0.1, route.field_goals())
    z = _kw()["z"][:, :b * N].contiguous()
    res, s = _search(w, None, route, b=b, z=z, geodesic=fld)
    t64, ok = _check_replay("geodesic", res, route, pool_dist=False)
    print("route_cursor", res.route_cursor.tolist(), "slack", t64["slack"].tolist())
    cur = res.route_cursor[-1].long().cpu().numpy()
    assert s["field_alive"].dtype == torch.int32 and s["field_alive"].cpu().tolist() == route.field_of[np.arange(b), cur].tolist()
    assert torch.equal(s["route_state"], res.route_cursor[-1]) and int(cur.max()) >= 1 and res.geo_dist is not None
    # the goal term of primitive k is the field of the waypoint it was scored against, at the chosen row's last pelvis
    before = np.concatenate([np.zeros((1, b), np.int64), res.route_cursor[:-1].long().cpu().numpy()])          # the cursor primitive k began with
    idx = route.field_of[np.arange(b)[None], before]
    pts = torch.stack([res.rotmat[k] @ res.pelvis[k, :, 19, :, None] for k in range(K)])[..., 0] + res.transl          # [K,b,3]
    for k in range(K):
        pick = GeodesicField(fld.dist[idx[k]].contiguous(), fld.origin[idx[k]].contiguous(), fld.cell, fld.goals[idx[k]].contiguous(), fld.passes)
        want = pick.sample(pts[k][:, None, :2].contiguous())[:, 0]
        assert torch.allclose(res.geo_dist[k], want, atol=2e-4, rtol=1e-5), (k, res.geo_dist[k], want)
    with pytest.raises(ValueError, match="route.field_goals"):
        _search(w, None, route, b=b, z=z, geodesic=GeodesicField.from_raster(free, np.array([-6.0, -6.0]), 0.1, route.field_goals()[:2]))


@pytest.mark.parametrize("sense_people", [False, True])
def test_route_with_a_policy(policy_world, goal_run, sense_people):
    from egogen_amd.proposal import PolicyProposal
    from egogen_amd.route import Routes
    w = policy_world
    Kp, Np = w["z"].shape[0], w["z"].shape[1] // 3
    route = Routes.from_lists(_via(goal_run, w, w["T0"].numpy()), pass_radius=1.0)
    prop = PolicyProposal(w["policy"], edges=w["room0"], sense_people=sense_people)
    extra = dict(groups=[0, 0, 0]) if sense_people else {}
    res, s = _search(w, None, route, k=Kp, n=Np, z=w["z"].cuda(), T0=w["T0"], scene=w["scene"], policy=prop, **extra)
    t64, ok = _check_replay(f"policy people={sense_people}", res, route, pool_dist=False)
    print("route_cursor", res.route_cursor.tolist(), "slack", t64["slack"].tolist())
    assert res.policy_mu.shape == (Kp, 3, 128) and torch.equal(s["route_state"], res.route_cursor[-1])
    # the observation of primitive k aims at the waypoint it is scored against: obs_dist = 1 / (1 + the 3-D distance from the
    # pelvis of the second seed frame to route_goal[k])
    eye = torch.stack([res.rotmat[k] @ res.pelvis[k, :, 1, :, None] for k in range(Kp)])[..., 0] + res.transl
    d = (res.route_goal - eye).norm(dim=-1)
    assert torch.allclose(res.obs_dist, 1.0 / (1.0 + d), atol=1e-4), (res.obs_dist, 1.0 / (1.0 + d))


# ---- egx_route_metrics ---------------------------------------------------------------------------------------------------------
METRIC_RADIUS = 0.12


def _line_motion(Kp, seed):
    """one motion of Kp primitives on a straight line in the world, 0.12 m per frame, each primitive recorded in a frame of its
    own -> (pelvis [Kp,20,3], rotmat [Kp,3,3], transl [Kp,3] float32, m: a -> the point half way between frames a and a + 1 of
    the motion as the float32 records give it in float64)"""
    g = np.random.default_rng(seed)
    F = 18 * Kp + 2
    yaw0 = g.normal() * 2.0
    track = g.normal(size=3) * 2.0 + np.arange(F)[:, None] * 0.12 * np.array([np.cos(yaw0), np.sin(yaw0), 0.0])
    track[:, 2] = 0.9
    yaw, T = g.normal(size=Kp) * 2.0, g.normal(size=(Kp, 3)) * 2.0
    R = np.zeros((Kp, 3, 3))
    R[:, 0, 0], R[:, 0, 1], R[:, 1, 0], R[:, 1, 1], R[:, 2, 2] = np.cos(yaw), -np.sin(yaw), np.sin(yaw), np.cos(yaw), 1.0
    R, T = R.astype(np.float32), T.astype(np.float32)
    pelvis = np.stack([np.einsum("ji,tj->ti", R[k].astype(np.float64), track[18 * k:18 * k + 20] - T[k]) for k in range(Kp)]).astype(np.float32)
    x, y = ref.world_xy(pelvis, R, T, np.float64)
    frames = np.concatenate([np.arange(20)] + [20 * k + np.arange(2, 20) for k in range(1, Kp)])
    q = np.stack([x.reshape(-1)[frames], y.reshape(-1)[frames], np.full(F, 0.9)], -1)
    return pelvis, R, T, (lambda a: (q[a] + q[a + 1]) / 2)


def _metric_set():
    from egogen_amd.metrics import MotionSet
    parts, routes, start = [], [], [0]
    far = np.array([90.0, 90.0, 0.9])
    for Kp, seed, make in ((1, 1, lambda m: [far]),                                                    # one waypoint: nothing to pass
                           (1, 2, lambda m: [m(0), m(7), far]),                                        # the first on a seed frame
                           (3, 3, lambda m: [m(30), far]),                                             # in the second primitive
                           (3, 4, lambda m: [m(1), m(1), m(10), m(8), m(40), far]),                    # m(8) lies behind: it and m(40) wait
                           (3, 5, lambda m: [m(a) for a in range(0, 45, 3)] + [far]),                  # sixteen, fifteen passed
                           (3, 6, lambda m: [m(a) for a in range(20, 50, 2)] + [m(54)]),               # sixteen, the last one near the end
                           (1, 7, None)):                                                              # no route
        pelvis, R, T, m = _line_motion(Kp, seed)
        parts.append((pelvis, R, T))
        routes.append(None if make is None else np.asarray(make(m)))
        start.append(start[-1] + Kp)
    Pn = start[-1]
    cat = lambda j: np.concatenate([p[j] for p in parts])
    z = lambda *s: np.zeros((Pn,) + s, np.float32)
    return MotionSet(z(20, 67, 3), cat(0), cat(1), cat(2), z(20, 93), z(10), start, ["2-frame"] * Pn, routes=routes)


def test_route_metrics_on_straight_lines():
    from egogen_amd import metrics
    ms = _metric_set()
    want = ref.route_metrics(ms, METRIC_RADIUS)
    assert want["slack"][np.isfinite(want["slack"])].min() >= HIT_MARGIN
    assert want["waypoints_passed"].tolist() == [0, 2, 1, 3, 15, 15, 0]                               # by construction
    assert want["pass_frame"][1, :3].tolist() == [0, 7, -1] and want["pass_frame"][2, :2].tolist() == [30, -1]
    assert want["pass_frame"][3, :6].tolist() == [1, 1, 10, -1, -1, -1] and np.isnan(want["approach_min"][3, 4:]).all()
    assert want["pass_frame"][4, :16].tolist() == list(range(0, 45, 3)) + [-1]
    got = metrics.route_metrics(ms, pass_radius=METRIC_RADIUS)
    assert got["pass_frame"].shape == (7, 16) and got["pass_frame"].dtype == np.int32 and got["approach_min"].dtype == np.float64
    assert np.array_equal(got["pass_frame"], want["pass_frame"]) and np.array_equal(got["waypoints_passed"], want["waypoints_passed"])
    assert got["count"].tolist() == [1, 3, 2, 6, 16, 16, 0]
    assert np.array_equal(np.isnan(got["approach_min"]), np.isnan(want["approach_min"]))
    live = ~np.isnan(want["approach_min"])
    assert live.sum() == 1 + 3 + 2 + 4 + 16 + 16 and np.abs(got["approach_min"][live] - want["approach_min"][live]).max() <= 1e-12
    assert abs(got["approach_min"][5, 15] - 0.06) < 1e-6 and abs(got["approach_min"][3, 3] - 0.18) < 1e-6          # m(8) from frame 10 on
    # a set without any route: -1 / NaN / 0
    from egogen_amd.metrics import MotionSet
    bare = MotionSet(ms.markers, ms.pelvis, ms.rotmat, ms.transl, ms.params, ms.betas, ms.prim_start, ms.mp_types)
    none = metrics.route_metrics(bare)
    assert (none["pass_frame"] == -1).all() and np.isnan(none["approach_min"]).all() and not none["waypoints_passed"].any()
    with pytest.raises(ValueError, match="pass_radius"):
        metrics.route_metrics(ms, pass_radius=-1.0)


def test_route_metrics_agree_with_the_search(route_run):
    """Where no waypoint is passed on a seed frame of the first primitive the per-primitive rule of the search and the per-frame
    rule of the evaluator see the same frames: the evaluator's count is the search's last cursor."""
    from egogen_amd import metrics
    from egogen_amd.metrics import MotionSet
    res, s, route = route_run
    ms = MotionSet.from_sequences(res)
    assert [r.tolist() for r in ms.routes] == [r.tolist() for r in route.lists()]
    got = metrics.route_metrics(ms, pass_radius=route.pass_radius)
    want = ref.route_metrics(ms, route.pass_radius)
    t64 = ref.replay(_f64(res.pelvis), _f64(res.rotmat), _f64(res.transl), route.waypoints, route.count, route.pass_radius, np.float64)
    last = res.n_valid.cpu().numpy() - 1
    cursor = res.route_cursor.cpu().numpy()[last, np.arange(3)]
    same = (want["slack"] >= DECIDABLE) & (t64["slack"].min(0) >= DECIDABLE) & ~((want["pass_frame"] >= 0) & (want["pass_frame"] < 2)).any(1)
    print("waypoints_passed", got["waypoints_passed"], "cursor", cursor, "pass_frame", got["pass_frame"][:, :3], "compared", same)
    assert same.any() and cursor[same].max() >= 1
    assert np.array_equal(got["waypoints_passed"][same], cursor[same]) and np.array_equal(got["pass_frame"][same], want["pass_frame"][same])


# ---- the drivers ---------------------------------------------------------------------------------------------------------------
def test_drivers_write_and_measure_routes(tmp_path):
    """gen_motion.py --people with ">"-chained waypoints writes motion_*_p*.pkl files whose wpath holds the whole route, and
    eval_motion.py adds the route figures to their rows; a file without a route has none.  In this process: the drivers' `main`."""
    import importlib.util
    import json
    import os
    import pickle
    from tests.genop_gpu_helpers import ROOT, V_SMALL

    def load(name):
        spec = importlib.util.spec_from_file_location(name + "_under_test", os.path.join(ROOT, "exp_GAMMAPrimitive", name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    gen, ev = load("gen_motion"), load("eval_motion")
    state, np_state = torch.get_rng_state(), np.random.get_state()          # the driver seeds the global generators
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        base = ["--n-primitives", "2", "--n-gens", "1", "--seed", "3", "--num-verts", str(V_SMALL), "--n-candidates", "4"]
        gen.main(base + ["--people", "1,0,90:0,1,0.9>-1,1,0.9>-2,0,0.9;-1,0,-90:2,0,0.9", "--pass-radius", "0.6", "--out", "routes"])
        gen.main(base + ["--goal", "1,1,0.9;2,2,0.9", "--out", "one"])
        gen.main(base + ["--goal", "2,2,0.9", "--out", "plain"])
    finally:
        os.chdir(cwd)
        torch.set_rng_state(state)
        np.random.set_state(np_state)
    want = {"routes/motion_3_0_p0.pkl": [[0, 1, 0.9], [-1, 1, 0.9], [-2, 0, 0.9]], "routes/motion_3_0_p1.pkl": [[2, 0, 0.9]],
            "one/motion_3_0.pkl": [[1, 1, 0.9], [2, 2, 0.9]], "plain/motion_3_0.pkl": [[2, 2, 0.9]]}
    for name, way in want.items():
        with open(tmp_path / name, "rb") as fh:
            node = pickle.load(fh)
        assert node["wpath"].shape == (1 + len(way), 3) and np.array_equal(node["wpath"][1:], np.asarray(way, np.float32)), name
        assert len(node["motion"]) == 2
    out = tmp_path / "metrics.json"
    ev.main(["--in", str(tmp_path / "routes"), str(tmp_path / "plain"), "--out", str(out), "--pass-radius", "0.6"])
    res = json.loads(out.read_text())
    rows = {os.path.relpath(r["file"], tmp_path): r for r in res["files"]}
    assert res["pass_radius"] == 0.6 and rows["routes/motion_3_0_p0.pkl"]["waypoints"] == 3
    r0 = rows["routes/motion_3_0_p0.pkl"]
    assert len(r0["pass_frame"]) == 3 and len(r0["approach_min"]) == 3 and r0["pass_frame"][2] == -1 and r0["approach_min"][0] >= 0
    assert r0["waypoints_passed"] == sum(f >= 0 for f in r0["pass_frame"])
    assert "waypoints" not in rows["routes/motion_3_0_p1.pkl"] and "waypoints" not in rows["plain/motion_3_0.pkl"]
