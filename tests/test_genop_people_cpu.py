"""The policy's observation with other people in it, without a device: hand cases for the restatement of tests/genop_people_ref.py
(what a hole is: the union of the boxes, never even-odd over their edges), the share of undecidable rays of the cases the GPU test
runs, and the host's argument checks (`PolicyProposal(sense_people=)`, `PersonGroups.member_group`, the driver's flag)."""
import importlib.util
import os
import types

import numpy as np
import pytest
import torch

from oracle.env import calc_egosensing
from tests import genop_people_ref as pref
from tests import genop_policy_ref as ref
from tests.genop_gpu_helpers import ROOT, UNDECIDABLE_CAP

RAY_LEN = 7.0


def _head(x=0.0, y=0.0):
    """joints [2,127,3] of a head whose eye mid-point stands at (x, y) and looks along +y: ray 31 (+pi/2) then points along -x, ray 0
    along +x, both up to 1e-16"""
    J = torch.zeros(2, 127, 3)
    J[:, 23] = torch.tensor([x - 0.03, y, 1.6])
    J[:, 24] = torch.tensor([x + 0.03, y, 1.6])
    J[:, 56] = J[:, 23] + torch.tensor([0.0, 0.1, 0.0])
    J[:, 57] = J[:, 24] + torch.tensor([0.0, 0.1, 0.0])
    return J


def _reads(d):
    return -1.0 + 2.0 * (d / RAY_LEN)


def test_ray_straight_at_a_box():
    ego = pref.calc_egosensing_holes(_head(), None, [[-3.0, -0.5, -2.0, 0.5]], RAY_LEN)
    assert abs(float(ego[0, 31]) - _reads(2.0)) < 1e-6 and abs(float(ego[1, 31]) - _reads(2.0)) < 1e-6
    assert float(ego[0, 0]) == 1.0                       # the ray the other way meets nothing: the unbounded plane
    assert float(ego.min()) > -1.0


def test_eye_inside_one_box_sees_nothing():
    ego = pref.calc_egosensing_holes(_head(), None, [[-0.5, -0.5, 0.5, 0.5], [2.0, 2.0, 3.0, 3.0]], RAY_LEN)
    assert torch.equal(ego, -torch.ones(2, 32))


def test_eye_inside_the_overlap_of_two_boxes_sees_nothing():
    """where union and even-odd differ: two crossings to the right of the eye would make it walkable again"""
    two = [[-0.5, -0.5, 0.5, 0.5], [-0.2, -0.3, 0.8, 0.4]]
    ego = pref.calc_egosensing_holes(_head(), None, two, RAY_LEN)
    assert torch.equal(ego, -torch.ones(2, 32))
    wall = pref.box_edges([[-3.0, -3.0, 3.0, 3.0]])
    assert torch.equal(pref.calc_egosensing_holes(_head(), wall, two, RAY_LEN), -torch.ones(2, 32))
    e = np.concatenate([wall, pref.box_edges(two)])
    assert e.shape == (12, 4) and float(calc_egosensing(_head(), e, RAY_LEN).min()) > -1.0     # even-odd over all edges: walkable again
    # an eye in one of them only, next to the overlap, is blind as well; one outside both sees the nearer
    assert torch.equal(pref.calc_egosensing_holes(_head(-0.4, 0.0), None, two, RAY_LEN), -torch.ones(2, 32))
    out = pref.calc_egosensing_holes(_head(-1.5, 0.0), None, two, RAY_LEN)
    assert abs(float(out[0, 0]) - _reads(1.0)) < 1e-6


def test_box_behind_a_wall_reads_the_wall():
    wall = np.array([[-1.5, -1.5, 1.5, -1.5], [1.5, -1.5, 1.5, 1.5], [1.5, 1.5, -1.5, 1.5], [-1.5, 1.5, -1.5, -1.5]])
    ego = pref.calc_egosensing_holes(_head(), wall, [[-3.0, -0.5, -2.0, 0.5]], RAY_LEN)
    assert torch.equal(ego, calc_egosensing(_head(), wall, RAY_LEN)) and abs(float(ego[0, 31]) - _reads(1.5)) < 1e-6
    # and with no hole the restatement is the oracle's function
    assert torch.equal(pref.calc_egosensing_holes(_head(0.3, -0.2), wall, np.zeros((0, 4)), RAY_LEN), calc_egosensing(_head(0.3, -0.2), wall, RAY_LEN))
    assert torch.equal(pref.calc_egosensing_holes(_head(5.0, 0.0), wall, [[-3.0, -0.5, -2.0, 0.5]], RAY_LEN), -torch.ones(2, 32))   # outside the static polygon


def test_obstacle_is_held_outside_its_frames():
    xy = np.zeros((1, 2, 3, 2), np.float32)
    xy[0, 0] = [[1.0, 0.0], [2.0, 0.5], [3.0, 1.0]]
    xy[0, 1] = [[9.0, 9.0]] * 3                         # beyond the count: never read
    obs = (xy, np.array([[0.25, 5.0]], np.float32), np.array([1], np.int32))
    at = lambda f: pref.track_boxes(obs, 0, f, torch.float64)
    assert torch.equal(at(2), torch.tensor([[2.75, 0.75, 3.25, 1.25]], dtype=torch.float64))
    for beyond in (2, 3, 40, 2 ** 31 - 1):
        assert torch.equal(at(beyond), at(2))
    for before in (-1, -40):
        assert torch.equal(at(before), torch.tensor([[0.75, -0.25, 1.25, 0.25]], dtype=torch.float64))
    assert torch.equal(at(0), torch.tensor([[0.75, -0.25, 2.25, 0.75]], dtype=torch.float64))      # one box for both frames
    assert torch.equal(at(1), torch.tensor([[1.75, 0.25, 3.25, 1.25]], dtype=torch.float64))


def test_boxes_restatement():
    d, _, _ = pref.people_inputs("none", 5, 20, 18)
    N = d["N"]
    b64 = pref.boxes(d["x0"][::N], d["x1"][::N], d["R0"][::N], d["T0"][::N], torch.float64)
    assert bool((b64[:, :2] < b64[:, 2:]).all())
    m = torch.stack([d["x0"][::N], d["x1"][::N]], 1).reshape(pref.B, 134, 3).double()
    for i in range(pref.B):
        w = m[i] @ d["R0"][::N][i].double().T + d["T0"][::N][i].double()
        assert torch.equal(b64[i], torch.cat([w[:, :2].min(0).values, w[:, :2].max(0).values]))
    x0 = d["x0"][::N].clone()
    x0[2, 7] = float("nan")
    bad = pref.boxes(x0, d["x1"][::N], d["R0"][::N], d["T0"][::N], torch.float32)
    assert bool(torch.isnan(bad[2]).all()) and bool(torch.isfinite(bad[[0, 1, 3, 4]]).all())
    groups = pref.csr(pref.IDS)
    assert len(pref.holes(pref.SEES, bad, groups, None, None, 0, torch.float32)) == 1          # the non-finite mate is no hole
    assert len(pref.holes(pref.SEES, b64, groups, None, None, 0, torch.float64)) == 2


@pytest.mark.parametrize("kind", ["none", "square", "two", "gon1200"])
def test_every_sequence_plays_its_part(kind):
    """the layout the GPU test relies on: who sees, who is blind and why, who has how many holes"""
    track_seen = 0
    for kind_, N, (fpr, first) in pref.PEOPLE_CASES:
        if kind_ != kind:
            continue
        d, poly, obs = pref.people_inputs(kind, N, fpr, first)
        plain = ref.observe(pref.seed_bodies(d), d["R_prev"], d["T_prev"], d["R0"][::N], d["T0"][::N], d["x0"][::N], d["x1"][::N], d["goal"],
                            poly, RAY_LEN, 0, 13, torch.float64)[1]
        for frame in pref.FRAMES if (N, fpr) == (5, 20) else (pref.case_frame(kind, N, (fpr, first)),):
            _, ego, _, _, count, box = pref.observe_case(d, poly, obs, RAY_LEN, 0, 13, torch.float64, frame=frame)
            assert count.tolist() == [4, 0, 2, 2, 2]
            assert torch.equal(ego[pref.IN_ONE], -torch.ones(2, 32)) and torch.equal(ego[pref.IN_TWO], -torch.ones(2, 32))
            assert -1.0 < float(ego[pref.SEES].min()) < 0.5                                     # a mate 3.5 m or a track 2 m ahead
            assert not torch.equal(ego[pref.SEES], plain[pref.SEES])
            if kind == "square":
                assert torch.equal(ego[pref.TRACKS], -torch.ones(2, 32))                        # outside its polygon, holes or not
            else:
                assert float(ego[pref.TRACKS].min()) > -1.0
                track_seen += int(not torch.equal(ego[pref.TRACKS], plain[pref.TRACKS]))        # the track beside it, where it looks that way
            assert torch.equal(ego[pref.LONE], plain[pref.LONE])                                # no hole: the observation as it was
    assert kind == "square" or track_seen > 0
    eye =(pref.seed_bodies(d)[:, :, 23] + pref.seed_bodies(d)[:, :, 24]) / 2
    jw = torch.einsum("bij,btj->bti", d["R_prev"], eye) + d["T_prev"][:, None]
    inside = lambda i, m: bool(((box[m, :2] <= jw[i, :, :2].double()) & (jw[i, :, :2].double() < box[m, 2:])).all())
    assert inside(pref.IN_ONE, pref.IN_TWO) and not inside(pref.IN_ONE, pref.SEES)
    assert inside(pref.IN_TWO, pref.SEES) and inside(pref.IN_TWO, pref.IN_ONE)


def test_undecidable_rays_stay_under_the_cap():
    """A condition of the GPU test, held here for its seeds and positions: per case the float64 restatement alone leaves out at most
    UNDECIDABLE_CAP of the rays."""
    for kind, N, (fpr, first) in pref.PEOPLE_CASES:
        d, poly, obs = pref.people_inputs(kind, N, fpr, first)
        u = pref.undecidable(d, poly, obs, RAY_LEN, frame=pref.case_frame(kind, N, (fpr, first)))
        assert float(u.float().mean()) <= UNDECIDABLE_CAP, (kind, N, fpr, int(u.sum()), u.numel())
    d, poly, obs = pref.people_inputs("two", 5, 20, 18)
    alone = pref.take(d, [0, 2, 3])
    u = pref.undecidable(alone, (poly[0], poly[1], poly[2][[0, 2, 3]]), obs, RAY_LEN, groups=pref.csr([0, 0, 0]), obs_index=pref.OBS_INDEX[[0, 2, 3]])
    assert float(u.float().mean()) <= UNDECIDABLE_CAP


# ---- the host ------------------------------------------------------------------------------------------------------------------
def _runner():
    return types.SimpleNamespace(forward=lambda *a, **k: None, actor=types.SimpleNamespace(min_logvar=-2.5, max_logvar=2.5))


def test_sense_people_must_be_a_bool():
    from egogen_amd.proposal import PEOPLE_FIELDS, PolicyProposal
    assert PolicyProposal(_runner()).sense_people is False and PolicyProposal(_runner(), sense_people=True).sense_people is True
    for bad in (1, 0, "yes", None, 1.0):
        with pytest.raises(TypeError, match="sense_people must be a bool"):
            PolicyProposal(_runner(), sense_people=bad)
    from egogen_amd.genop import PrimitiveSequence
    assert PEOPLE_FIELDS == PrimitiveSequence.PEOPLE_FIELDS == ("people_box", "obs_people_count", "policy_sense_people")
    assert not set(PEOPLE_FIELDS) & set(PrimitiveSequence.POLICY_FIELDS)
    seq = PrimitiveSequence(*[None] * 10, search={k: None for k in PrimitiveSequence.SEARCH_FIELDS})
    assert all(getattr(seq, k) is None for k in PEOPLE_FIELDS)


@pytest.mark.parametrize("ids", [[1, 0, 1, 1, 2], [0, 0, 0], [5], [3, 2, 1, 0], [0, 1, 0, 1, 0, 1, 2]])
def test_member_group_is_the_inverse_of_the_csr(ids):
    from egogen_amd.crowd import PersonGroups
    g = PersonGroups.from_ids(ids, len(ids))
    assert g.member_group is None
    g.to("cpu")
    of = g.member_group
    assert of.dtype == torch.int32 and of.shape == (len(ids),) and of.device == g.group_start.device
    for grp in range(len(g)):
        mine = g.group_member[int(g.group_start[grp]):int(g.group_start[grp + 1])].long()
        assert bool((of[mine] == grp).all())
    assert all((ids[i] == ids[j]) == (int(of[i]) == int(of[j])) for i in range(len(ids)) for j in range(len(ids)))


def test_driver_flag_needs_a_policy(capsys):
    spec = importlib.util.spec_from_file_location("gen_motion_people", os.path.join(ROOT, "exp_GAMMAPrimitive", "gen_motion.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with pytest.raises(SystemExit) as e:
        mod.main(["--goal", "0,2,0.9", "--policy-sees-people"])
    assert e.value.code == 2 and "--policy-sees-people needs --policy" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:                # with a policy the flag is taken: the run ends at the missing file, before any device
        mod.main(["--goal", "0,2,0.9", "--policy-sees-people", "--policy", os.path.join(ROOT, "no_such_checkpoint.pt")])
    assert "no such file" in str(e.value.code)
