"""Host-side checks of the marker-level pair model of the joint search, no device: the restatement tests/genop_joint_markers_ref.py
on hand cases, next to the cylinder model's (tests/genop_joint_ref.py) on the same people, and the argument errors
`generate_sequence_to_goal(pair_model=, pair_skin=)` raises before any device work."""
import numpy as np
import pytest
import torch

from tests import genop_joint_markers_ref as mref
from tests import genop_joint_ref as jref

DTYPES = [torch.float64, torch.float32]
SKIN, MARGIN, BODY = 0.05, 0.5, 0.15


def cloud(track, height=1.7, arm=None):
    """track [18,2] (world xy of the pelvis) -> [18,67,3]: 67 points within 0.02 m of the vertical axis through the pelvis, z in
    [0, height]; arm = (marker, dx, dy): that marker is held out by (dx, dy) from the axis instead"""
    a = torch.arange(67, dtype=torch.float64)
    off = 0.02 * torch.stack([torch.cos(2.4 * a), torch.sin(2.4 * a)], -1) * (a[:, None] % 5) / 4.0           # [67,2], at most 0.02 m
    if arm is not None:
        off[arm[0]] = torch.tensor([arm[1], arm[2]], dtype=torch.float64)
    xy = torch.as_tensor(track, dtype=torch.float64)[:, None, :] + off[None]
    z = (height * a / 66.0)[None, :, None].expand(18, 67, 1)
    return torch.cat([xy, z], -1)


def _walk(x0, y0, dx, dy):
    t = torch.arange(18, dtype=torch.float64)[:, None]
    return torch.tensor([x0, y0], dtype=torch.float64) + t * torch.tensor([dx, dy], dtype=torch.float64)


def states(tracks, clouds, cost, choice, dtype, w=1.0):
    """the same people for both models -> (cylinder state of genop_joint_ref, marker state of genop_joint_markers_ref)"""
    track = torch.stack([torch.stack(list(rows)) for rows in tracks])                                       # [b,N,18,2]
    world = torch.stack([torch.stack(list(rows)) for rows in clouds]).float()                               # [b,N,18,67,3] as float32 inputs
    b, N = track.shape[:2]
    common = {"cost": torch.as_tensor(cost, dtype=torch.float32).reshape(b, N), "terms": torch.zeros(b, N, 5),
              "colliding": torch.zeros(b, N, dtype=torch.bool), "members": list(range(b)), "w": w, "margin": MARGIN}
    cyl = dict(common, track=track, choice={m: int(c) for m, c in enumerate(choice)}, body_radius=BODY)
    mk = dict(common, D=mref.group_table(world.to(dtype), list(range(b))), bad=mref.bad_frames(world), choice={m: int(c) for m, c in enumerate(choice)},
              skin=SKIN)
    return cyl, mk


def arm_case(dtype):
    """Two people walk side by side, pelvises 0.7 m apart: the cylinders (radii 0.15) clear by 0.4 m.  The straight row of member 0
    holds marker 40 out by 0.66 m towards member 1: 0.04 m from member 1's axis, within the skin.  Member 0's other row walks
    0.6 m further away (cost 1.2 against 1.0)."""
    a0, a1 = _walk(0.0, 0.0, 0.03, 0.0), _walk(0.0, -0.6, 0.03, 0.0)
    c0, c1 = _walk(0.0, 0.7, 0.03, 0.0), _walk(0.0, 1.3, 0.03, 0.0)
    arm = (40, 0.0, 0.66)
    return states([[a0, a1], [c0, c1]], [[cloud(a0, arm=arm), cloud(a1, arm=arm)], [cloud(c0), cloud(c1)]], [[1.0, 1.2], [1.0, 1.2]], [0, 0], dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_an_outstretched_arm_is_a_hit_for_the_markers_only(dtype):
    cyl, mk = arm_case(dtype)
    # the cylinder model: 0.4 m clear, a term of 0.1 on the straight row, nobody moves
    r = jref.sweeps(cyl, 2, dtype)
    assert not r["steps"][0][0]["hit"].any() and abs(float(r["steps"][0][0]["clearance"][0]) - 0.4) < 1e-6
    assert r["choice_trace"].tolist() == [[0, 0], [0, 0]] and r["changed"].tolist() == [0, 0]
    assert bool((jref.crowd_clearance(cyl, dtype) > 0.39).all())
    # the marker model: the arm is within the skin, member 0 sidesteps, member 1 stays
    assert bool((mref.crowd_clearance(mk, dtype) < 0).all())
    r = mref.sweeps(mk, 2, dtype)
    first = r["steps"][0][0]
    assert first["hit"].tolist() == [True, False] and first["cls"].tolist() == [1, 0]
    assert float(first["clearance"][0]) < -0.005 and float(first["term"][0]) > float(first["term"][1]) >= 0.0
    assert r["choice_trace"].tolist() == [[1, 0], [1, 0]] and r["changed"].tolist() == [1, 0] and mk["choice"] == {0: 1, 1: 0}
    cc = mref.crowd_clearance(mk, dtype)
    assert bool((cc > 0.5).all()) and float((cc[0] - cc[1]).abs()) == 0.0           # arm at y = 0.06, the other's axis at 0.7: the same pair both ways


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_above_the_other_is_a_hit_for_the_cylinders_only(dtype):
    """the same xy, 1 m apart in z, clouds 0.5 m tall: the cylinders coincide, the nearest markers are 0.5 m apart"""
    t = _walk(0.3, -0.2, 0.02, 0.01)
    up = cloud(t, height=0.5) + torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64)
    cyl, mk = states([[t], [t]], [[cloud(t, height=0.5)], [up]], [[1.0], [1.0]], [0, 0], dtype)
    rc, rm = jref.member_step(cyl, 0, dtype), mref.member_step(mk, 0, dtype)
    assert bool(rc["hit"][0]) and abs(float(rc["clearance"][0]) + 2 * BODY) < 1e-6
    assert not bool(rm["hit"][0]) and abs(float(rm["clearance"][0]) - (0.5 - SKIN)) < 0.03 and float(rm["clearance"][0]) >= 0.5 - SKIN - 1e-6
    assert abs(float(rm["term"][0]) - (MARGIN - float(rm["clearance"][0]))) < 1e-6 and int(rm["cls"][0]) == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_bad_frames_and_groups_of_one(dtype):
    cyl, mk = arm_case(dtype)
    world = torch.stack([torch.stack([cloud(_walk(0.0, y, 0.03, 0.0)) for y in ys]) for ys in ((0.0, -0.6), (0.7, 1.3))]).float()
    world[1, 0, 5, 66, 2] = float("nan")                   # member 1's chosen row, frame 7
    D = mref.group_table(world.to(dtype), [0, 1])
    assert bool((D[(0, 1)][:, 0, 5] == float("inf")).all()) and bool(torch.isfinite(D[(0, 1)][:, 1]).all())
    assert bool(torch.isfinite(D[(0, 1)][:, 0, [4, 6]]).all())
    bad = mref.bad_frames(world)
    assert bad[1, 0].tolist() == [f == 5 for f in range(18)] and int(bad.sum()) == 1
    mk.update(D=D, bad=bad)
    r0 = mref.member_step(mk, 0, dtype)                    # the other is not there in that frame
    assert bool(r0["finite"].all()) and bool(torch.isfinite(r0["clearance"]).all())
    r1 = mref.member_step(mk, 1, dtype)                    # the bad row's own step
    assert bool(torch.isnan(r1["term"][0])) and bool(torch.isnan(r1["clearance"][0])) and bool(torch.isnan(r1["joint_cost"][0]))
    assert not bool(r1["hit"][0]) and int(r1["cls"][0]) == 2 and r1["choice"] == 1 and int(r1["cls"][1]) == 0
    one = dict(mk, members=[0], D={}, choice={0: 1})
    r = mref.sweeps(one, 2, dtype)
    assert not r["steps"][0][0]["term"].any() and bool((r["steps"][0][0]["clearance"] == float("inf")).all())
    assert r["choice_trace"].tolist() == [[0], [0]] and float(mref.crowd_clearance(one, dtype)[0]) == float("inf")


def test_the_table_is_symmetric_and_exhaustive():
    g = torch.Generator().manual_seed(3)
    wa, wb = torch.randn(3, 18, 67, 3, generator=g).double(), torch.randn(2, 18, 67, 3, generator=g).double() + 0.5
    D = mref.pair_dist(wa, wb)
    assert torch.equal(D, mref.pair_dist(wb, wa).permute(1, 0, 2))
    brute = torch.cdist(wa[1, 4], wb[0, 4]).min()
    assert abs(float(D[1, 0, 4]) - float(brute)) < 1e-12


# ---- PersonGroups: the pairs ------------------------------------------------------------------------------------------------------
def test_person_groups_pairs():
    from egogen_amd import PersonGroups
    from egogen_amd.crowd import PAIR_TABLE_CAP_BYTES
    g = PersonGroups.from_ids([7, 3, 7, 9, 3, 7], 6)       # sizes 3, 2, 1
    assert g.pair_offsets.tolist() == [0, 3, 4, 4] and g.pair_table_bytes(16) == 4 * 256 * 72
    assert g.to("cpu").pair_start.tolist() == [0, 3, 4, 4] and g.pair_start.dtype == torch.int32
    full = PersonGroups.from_ids([0] * 32, 32)
    assert full.pair_table_bytes(16) == 496 * 256 * 72 < PAIR_TABLE_CAP_BYTES < full.pair_table_bytes(256)
    assert PAIR_TABLE_CAP_BYTES == 1 << 30


# ---- generate_sequence_to_goal: the errors come before any device work ---------------------------------------------------------
def test_generate_sequence_to_goal_pair_model_errors_need_no_device():
    from egogen_amd.genop import GAMMAPrimitiveComboGenOP
    op = GAMMAPrimitiveComboGenOP.__new__(GAMMAPrimitiveComboGenOP)      # no constructor: it asks for a device
    op.body_model, op.model = object(), None
    mk = lambda b: (np.zeros((2, b, 201), np.float32), np.zeros((2, b, 93), np.float32), np.zeros(10, np.float32), np.zeros(3, np.float32))
    call = lambda N=2, b=4, **kw: op.generate_sequence_to_goal(*mk(b), 2, N, **kw)
    with pytest.raises(ValueError, match="pair_model must be one of"):
        call(groups=[0, 0, 1, 1], pair_model="capsule")
    with pytest.raises(ValueError, match="pair_model must be one of"):
        call(pair_model="capsule")
    with pytest.raises(ValueError, match="needs groups"):
        call(pair_model="markers")
    for skin in (-0.01, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="pair_skin"):
            call(groups=[0, 0, 1, 1], pair_model="markers", pair_skin=skin)
    with pytest.raises(ValueError, match="above the cap"):
        call(N=256, b=32, groups=[0] * 32, pair_model="markers")
    with pytest.raises(ValueError, match="beam_width must be 1"):       # the group checks still come first
        call(groups=[0, 0, 1, 1], pair_model="markers", beam_width=2)
    # what passes these checks goes on to ask for the model: the cap does not bind the cylinder model, nor 32 people at N 16
    for kw in (dict(N=256, b=32, groups=[0] * 32), dict(N=16, b=32, groups=[0] * 32, pair_model="markers"),
               dict(groups=[0, 0, 1, 1], pair_model="markers", pair_skin=0.0)):
        with pytest.raises(Exception) as e:
            call(**kw)
        assert not isinstance(e.value, ValueError), kw
