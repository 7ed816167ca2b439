"""Host-side checks of the joint primitive search, no device: the restatement tests/genop_joint_ref.py on hand cases, `PersonGroups`
(egogen_amd/crowd.py) and the argument errors `generate_sequence_to_goal(groups=)` raises before any device work."""
import numpy as np
import pytest
import torch

from tests import genop_joint_ref as jref

DTYPES = [torch.float64, torch.float32]


def _walk(x0, y0, dx, dy):
    """a straight track [18,2] from (x0, y0), (dx, dy) a frame"""
    t = torch.arange(18, dtype=torch.float64)[:, None]
    return torch.tensor([x0, y0], dtype=torch.float64) + t * torch.tensor([dx, dy], dtype=torch.float64)


def _state(track, cost, choice, members=None, w=1.0, margin=0.5, body_radius=0.15, colliding=None):
    track = torch.as_tensor(track)
    b, N = track.shape[:2]
    cost = torch.as_tensor(cost, dtype=torch.float32).reshape(b, N)
    return {"track": track, "cost": cost, "terms": torch.zeros(b, N, 5), "colliding": torch.zeros(b, N, dtype=torch.bool) if colliding is None
            else torch.as_tensor(colliding).bool(), "members": list(range(b)) if members is None else members,
            "choice": {m: int(c) for m, c in enumerate(choice)}, "w": w, "margin": margin, "body_radius": body_radius}


def _two_people():
    """Two people 2 m apart walk at each other along y = 0 ("straight", cost 1.0: the tracks cross, overlapping) or sidestep 0.6 m
    in y ("sidestep", cost 1.2)."""
    a = torch.stack([_walk(-1.0, 0.0, 0.1, 0.0), _walk(-1.0, 0.6, 0.1, 0.0)])
    c = torch.stack([_walk(1.0, 0.0, -0.1, 0.0), _walk(1.0, -0.6, -0.1, 0.0)])
    return _state(torch.stack([a, c]), [[1.0, 1.2], [1.0, 1.2]], [0, 0])


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_members_one_gives_way(dtype):
    st = _two_people()
    assert bool((jref.crowd_clearance(st, dtype) < 0).all())                       # the two individual bests overlap
    r = jref.sweeps(st, 2, dtype)
    first = r["steps"][0][0]
    assert first["hit"].tolist() == [True, False] and first["cls"].tolist() == [1, 0]
    assert float(first["term"][0]) > float(first["term"][1]) >= 0.0
    assert r["choice_trace"].tolist() == [[1, 0], [1, 0]] and r["changed"].tolist() == [1, 0]
    assert st["choice"] == {0: 1, 1: 0}
    cc = jref.crowd_clearance(st, dtype)
    assert bool((cc >= 0).all()) and abs(float(cc[0]) - 0.3) < 1e-6 and abs(float(cc[1]) - 0.3) < 1e-6     # 0.6 m apart at the closest, radii 0.3


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_pair_term_is_the_mean_shortfall(dtype):
    """one frame-constant distance: two people standing 0.5 m apart, radii 0.15, margin 0.5 -> c_t = 0.2, term 0.3"""
    tr = torch.stack([_walk(0.0, 0.0, 0.0, 0.0)[None], _walk(0.5, 0.0, 0.0, 0.0)[None]])
    st = _state(tr, [[2.0], [3.0]], [0, 0], w=4.0)
    r = jref.member_step(st, 0, dtype)
    assert abs(float(r["clearance"][0]) - 0.2) < 1e-6 and abs(float(r["term"][0]) - 0.3) < 1e-6
    assert abs(float(r["joint_cost"][0]) - (2.0 + 4.0 * 0.3)) < 1e-5 and not bool(r["hit"][0]) and r["choice"] == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_group_of_one_is_the_identity(dtype):
    tr = torch.stack([_walk(0.0, 0.0, 0.1, 0.0), _walk(0.0, 1.0, 0.1, 0.0), _walk(0.0, 2.0, 0.1, 0.0)])[None]
    st = _state(tr, [[3.0, 1.0, 2.0]], [1])
    r = jref.sweeps(st, 3, dtype)
    step = r["steps"][0][0]
    assert not step["term"].any() and bool((step["clearance"] == float("inf")).all()) and not step["hit"].any()
    assert torch.equal(step["joint_cost"], st["cost"][0].to(dtype)) and r["choice_trace"].tolist() == [[1]] * 3 and r["changed"].tolist() == [0, 0, 0]
    assert float(jref.crowd_clearance(st, dtype)[0]) == float("inf")
    # a colliding cheapest row stays behind the clean ones, as in the selection
    st = _state(tr, [[3.0, 1.0, 2.0]], [2], colliding=[[False, True, False]])
    assert jref.sweeps(st, 1, dtype)["choice_trace"].tolist() == [[2]]


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_nan_track_of_another_member_drops_out(dtype):
    st = _two_people()
    st["track"][1, 0, 5] = float("nan")                    # member 1's chosen track, one frame
    r = jref.member_step(st, 0, dtype)
    assert bool(torch.isfinite(r["term"]).all()) and bool(torch.isfinite(r["joint_cost"]).all()) and bool(r["finite"].all())
    st["track"][1, 0] = float("nan")                       # all of it: member 0 walks alone
    st.pop("_tracks")
    r = jref.member_step(st, 0, dtype)
    assert not r["term"].any() and bool((r["clearance"] == float("inf")).all()) and r["choice"] == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_nan_own_pelvis_is_non_finite_and_no_hit(dtype):
    st = _two_people()
    st["track"][0, 0, 7, 1] = float("nan")                 # the overlapping straight row of member 0
    r = jref.member_step(st, 0, dtype)
    assert bool(torch.isnan(r["term"][0])) and bool(torch.isnan(r["clearance"][0])) and bool(torch.isnan(r["joint_cost"][0]))
    assert not bool(r["hit"][0]) and not bool(r["finite"][0]) and int(r["cls"][0]) == 2 and r["choice"] == 1
    assert bool(r["finite"][1]) and int(r["cls"][1]) == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_sweep_after_a_fixed_point_changes_nothing(dtype):
    g = torch.Generator().manual_seed(5)
    P, N = 5, 6
    tr = torch.stack([torch.stack([_walk(*(torch.rand(2, generator=g) * 1.5).tolist(), *((torch.rand(2, generator=g) - 0.5) * 0.1).tolist())
                                   for _ in range(N)]) for _ in range(P)])
    st = _state(tr, torch.rand(P, N, generator=g), [0] * P)
    r = jref.sweeps(st, 8, dtype)
    ch = r["changed"].tolist()
    assert ch[0] > 0 and 0 in ch, ch
    z = ch.index(0)
    assert ch[z:] == [0] * (8 - z) and all(row == r["choice_trace"][z].tolist() for row in r["choice_trace"][z:].tolist())


def test_state_before():
    trace = torch.tensor([[1, 0, 2, 9], [3, 0, 1, 9]])
    start = {0: 0, 2: 0, 1: 5}
    assert jref.state_before([0, 2, 1], start, trace, 0, 0) == {0: 0, 2: 0, 1: 5}
    assert jref.state_before([0, 2, 1], start, trace, 0, 2) == {0: 1, 2: 2, 1: 5}
    assert jref.state_before([0, 2, 1], start, trace, 1, 1) == {0: 3, 2: 2, 1: 0}


# ---- PersonGroups ---------------------------------------------------------------------------------------------------------------
def test_person_groups_order():
    from egogen_amd import PersonGroups
    g = PersonGroups.from_ids([7, 3, 7, 9, 3, 7], 6)
    assert len(g) == 3 and g.start.tolist() == [0, 3, 5, 6] and g.member.tolist() == [0, 2, 5, 1, 4, 3] and g.sizes.tolist() == [3, 2, 1]
    assert g.start.dtype == np.int32 and g.member.dtype == np.int32 and g.device is None
    assert PersonGroups.from_ids(torch.tensor([0, 0, 1]), 3).member.tolist() == [0, 1, 2]
    assert PersonGroups.from_ids(np.array([2.0, 2.0]), 2).start.tolist() == [0, 2]          # whole numbers are integers
    assert len(PersonGroups.from_ids(list(range(40)), 40)) == 40                             # 40 singletons
    assert PersonGroups.from_ids([0] * 32, 32).sizes.tolist() == [32]
    d = g.to("cpu")
    assert d is g and d.group_start.dtype == torch.int32 and d.group_member.tolist() == [0, 2, 5, 1, 4, 3] and d.device == torch.device("cpu")


@pytest.mark.parametrize("ids,b,match", [([0, 1], 3, "3 ids"), ([[0, 1, 2]], 3, "3 ids"), ([0.5, 1, 2], 3, "integers"), ([True, False], 2, "integers"),
                                         ([0, float("nan")], 2, "integers"), ([0] * 33, 33, "at most 32")])
def test_person_groups_errors(ids, b, match):
    from egogen_amd import PersonGroups
    with pytest.raises(ValueError, match=match):
        PersonGroups.from_ids(ids, b)


# ---- generate_sequence_to_goal: the errors come before any device work ---------------------------------------------------------
def test_generate_sequence_to_goal_group_errors_need_no_device():
    from egogen_amd.genop import GAMMAPrimitiveComboGenOP
    op = GAMMAPrimitiveComboGenOP.__new__(GAMMAPrimitiveComboGenOP)      # no constructor: it asks for a device
    op.body_model, op.model = object(), None
    b = 4
    data, bparams, betas, goal = np.zeros((2, b, 201), np.float32), np.zeros((2, b, 93), np.float32), np.zeros(10, np.float32), np.zeros(3, np.float32)
    call = lambda **kw: op.generate_sequence_to_goal(data, bparams, betas, goal, 2, 2, **kw)
    with pytest.raises(ValueError, match="beam_width must be 1"):
        call(groups=[0, 0, 1, 1], beam_width=2)
    with pytest.raises(ValueError, match="4 ids"):
        call(groups=[0, 0, 1])
    with pytest.raises(ValueError, match="at most 32"):
        op.generate_sequence_to_goal(np.zeros((2, 33, 201), np.float32), np.zeros((2, 33, 93), np.float32), betas, goal, 2, 2, groups=[0] * 33)
    for sweeps in (0, 9, 1.5):
        with pytest.raises(ValueError, match="joint_sweeps"):
            call(groups=[0, 0, 1, 1], joint_sweeps=sweeps)
    with pytest.raises(ValueError, match="must not be negative"):
        call(groups=[0, 0, 1, 1], pair_margin=-0.1)
    with pytest.raises(ValueError, match="must not be negative"):
        call(groups=[0, 0, 1, 1], body_radius=-0.1)
    with pytest.raises(ValueError, match="pair_weight finite"):
        call(groups=[0, 0, 1, 1], pair_weight=float("inf"))
