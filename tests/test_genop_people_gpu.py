"""The policy's observation with other people in it, on the device: the people launches of csrc/genop_policy.hip against the
float64 / float32 restatement of tests/genop_people_ref.py and against egx_primitive_observe, and
`generate_sequence_to_goal(policy=PolicyProposal(..., sense_people=True))` against its records.

Yardsticks.  Boxes: the project's `held()` rule, error against float64 at most 3 x the float32 restatement's.  Rays: the floor the env
tests use for egosensing (3.6e-4), a ray whose float64 value moves by more than that under a 1e-5 m shift of the eye left out, at most
UNDECIDABLE_CAP of the rays of a case (tests/test_genop_people_cpu.py holds that share for these seeds and positions without a device).
A blind eye reads exactly -1; people_count is exact; state, dist and time, and the rays of a sequence without a hole, are the bits of
egx_primitive_observe: torch.equal."""
import numpy as np
import pytest
import torch

from tests import genop_people_ref as pref
from tests import genop_policy_ref as ref
from tests.genop_gpu_helpers import (CFG_RF, MAX_DEPTH, RAY_LEN, W_TEST, _check_rays, _observe, _observe_lead, _observe_outputs, _poly_dev, _vp,
                                     held, patched_loop, search_world, small_world)  # noqa: F401

pytestmark = pytest.mark.gpu
NO_GROUPS, NO_OBS = (None, None, None, 0), (None, None, None, None, 0, 0, 0)


def _dev(a, dtype=None):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a) if isinstance(a, np.ndarray) else a, dtype=dtype).cuda().contiguous()


def _groups_dev(ids):
    if ids is None:
        return NO_GROUPS
    start, member, of = pref.csr(ids)
    return (_dev(start), _dev(member), _dev(of), len(start) - 1)


def _obs_dev(obs, index):
    """-> the obstacle arguments from obs_xy to num_frames"""
    if obs is None:
        return NO_OBS
    xy, radius, count = obs
    return (_dev(xy, torch.float32), _dev(radius, torch.float32), _dev(count, torch.int32), _dev(index, torch.int32), xy.shape[0], xy.shape[1],
            xy.shape[2])


def _boxes(x0, x1, x_ld, R0, T0, N, b):
    from egogen_amd import _lib
    box = torch.full((b, 4), float("nan"), device="cuda")
    _lib.check(_lib.load().egx_primitive_people_boxes(_vp(x0), _vp(x1), x_ld, _vp(R0), _vp(T0), N, b, _vp(box), _lib.current_stream_ptr()),
               "egx_primitive_people_boxes")
    torch.cuda.synchronize()
    return box


def _observe_people(g, fpr, first, N, choice, x_ld, poly, step, b, box, groups, obs, frame):
    """egx_primitive_observe_people into NaN / -7 filled outputs -> state, egosensing, dist, time, people_count"""
    from egogen_amd import _lib
    o = _observe_outputs(b)
    count = torch.full((b,), -7, dtype=torch.int32, device="cuda")
    tail = [_vp(t) if torch.is_tensor(t) else t for t in (*groups, *obs)]
    _lib.check(_lib.load().egx_primitive_observe_people(*_observe_lead(g, fpr, first, N, choice, x_ld, poly, step, b), _vp(box), *tail, int(frame),
                                                        _vp(count), *[_vp(t) for t in o], _lib.current_stream_ptr()),
               "egx_primitive_observe_people")
    torch.cuda.synchronize()
    return (*o, count)


def _to_dev(d):
    return {k: v.cuda().contiguous() for k, v in d.items() if torch.is_tensor(v)}


# ---- the boxes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 5])
def test_boxes_against_float64(N):
    d, _, _ = pref.people_inputs("none", N, 20, 18)
    g = _to_dev(d)
    got = _boxes(g["x0"], g["x1"], 201, g["R0"], g["T0"], N, pref.B)
    args = (d["x0"][::N], d["x1"][::N], d["R0"][::N], d["T0"][::N])
    held("people boxes", f"N={N}", got, pref.boxes(*args, torch.float64), pref.boxes(*args, torch.float32))
    assert bool((got[:, :2] < got[:, 2:]).all())                                    # min and max never swapped
    if N > 1:       # the first launch of the search: one frame per sequence, the seed frames N rows apart
        first = _boxes(g["x0"], g["x1"], 201 * N, g["R0"][::N].contiguous(), g["T0"][::N].contiguous(), 1, pref.B)
        assert torch.equal(first, got)
    # a NaN marker: four NaN for that sequence, the others' bits unchanged, and the box is no hole for its mates
    x0 = g["x0"].clone()
    x0[pref.IN_ONE * N, 7] = float("nan")
    bad = _boxes(x0, g["x1"], 201, g["R0"], g["T0"], N, pref.B)
    rest = [i for i in range(pref.B) if i != pref.IN_ONE]
    assert bool(torch.isnan(bad[pref.IN_ONE]).all()) and torch.equal(bad[rest], got[rest])
    out = _observe_people(g, 20, 18, N, g["choice"], 201, _poly_dev(None), 0, pref.B, bad, _groups_dev(pref.IDS), NO_OBS, 0)
    assert out[4].tolist() == [1, 0, 2, 1, 0]
    x1 = g["x1"].clone()
    x1[pref.SEES * N, 200] = float("inf")
    assert bool(torch.isnan(_boxes(g["x0"], x1, 201, g["R0"], g["T0"], N, pref.B)[pref.SEES]).all())


# ---- the rays ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,N,mode", pref.PEOPLE_CASES, ids=[f"{k}-N{n}-{m[1]}of{m[0]}" for k, n, m in pref.PEOPLE_CASES])
def test_observe_people_against_float64(kind, N, mode):
    fpr, first = mode
    frame = pref.case_frame(kind, N, mode)
    d, poly, obs = pref.people_inputs(kind, N, fpr, first)
    g, pd = _to_dev(d), _poly_dev(poly)
    step = 15 if N == 5 else 4
    box = _boxes(g["x0"], g["x1"], 201, g["R0"], g["T0"], N, pref.B)
    got = _observe_people(g, fpr, first, N, g["choice"], 201, pd, step, pref.B, box, _groups_dev(pref.IDS), _obs_dev(obs, pref.OBS_INDEX), frame)
    t64 = pref.observe_case(d, poly, obs, RAY_LEN, step, MAX_DEPTH, torch.float64, frame=frame)
    group = f"{kind} N={N} frame {first} of {fpr}, obstacle frame {frame}"
    _check_rays("observe_people egosensing", group, got[1], t64[1], pref.undecidable(d, poly, obs, RAY_LEN, frame=frame))
    assert got[4].tolist() == t64[4].tolist() == [4, 0, 2, 2, 2]
    blind = [pref.IN_ONE, pref.IN_TWO] + ([pref.TRACKS] if kind == "square" else [])     # in one box, in two, outside the static polygon
    assert torch.equal(got[1][blind].cpu(), -torch.ones(len(blind), 2, 32))
    assert float(got[1][pref.SEES].min()) > -1.0 and float(got[1][pref.SEES].min()) < 0.5
    plain = _observe(g, fpr, first, N, g["choice"], 201, pd, step, pref.B)
    for q, name in ((0, "state"), (2, "dist"), (3, "time")):
        assert torch.equal(got[q], plain[q]), name
    assert torch.equal(got[1][pref.LONE], plain[1][pref.LONE])                      # no hole: the rays of egx_primitive_observe
    assert not torch.equal(got[1][pref.SEES], plain[1][pref.SEES])
    if frame == pref.FRAMES[-1]:      # a track is held beyond its frames, however far
        far = _observe_people(g, fpr, first, N, g["choice"], 201, pd, step, pref.B, box, _groups_dev(pref.IDS), _obs_dev(obs, pref.OBS_INDEX),
                              2 ** 31 - 1)
        assert all(torch.equal(a, b_) for a, b_ in zip(far, got))
    if N > 1:        # NULL choice is candidate 0
        got0 = _observe_people(g, fpr, first, N, None, 201, pd, step, pref.B, box, _groups_dev(pref.IDS), _obs_dev(obs, pref.OBS_INDEX), frame)
        zero = _observe_people(g, fpr, first, N, torch.zeros(pref.B, dtype=torch.int32, device="cuda"), 201, pd, step, pref.B, box,
                               _groups_dev(pref.IDS), _obs_dev(obs, pref.OBS_INDEX), frame)
        assert all(torch.equal(a, b_) for a, b_ in zip(got0, zero))


# ---- no holes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,N,mode", [("none", 5, (20, 18)), ("square", 1, (2, 0)), ("two", 5, (20, 18))])
def test_without_holes_it_is_egx_primitive_observe(kind, N, mode):
    fpr, first = mode
    d, poly, obs = pref.people_inputs(kind, N, fpr, first)
    g, pd = _to_dev(d), _poly_dev(poly)
    plain = _observe(g, fpr, first, N, g["choice"], 201, pd, 3, pref.B)
    box = _boxes(g["x0"], g["x1"], 201, g["R0"], g["T0"], N, pref.B)
    empty = (obs[0], obs[1], np.zeros(2, np.int32))              # the tracks are there, none of them live
    for what, b_, groups, o in (("NULL groups and obstacles", None, NO_GROUPS, NO_OBS),
                                ("groups of one, no live track", box, _groups_dev(np.arange(pref.B)), _obs_dev(empty, pref.OBS_INDEX)),
                                ("groups of one, max_obstacles 0", box, _groups_dev(np.arange(pref.B)),
                                 (*_obs_dev(obs, pref.OBS_INDEX)[:5], 0, 3))):
        got = _observe_people(g, fpr, first, N, g["choice"], 201, pd, 3, pref.B, b_, groups, o, 1)
        for q, name in enumerate(("state", "egosensing", "dist", "time")):
            assert torch.equal(got[q], plain[q]), (what, name)
        assert not got[4].any(), what


# ---- batch independence --------------------------------------------------------------------------------------------------------
def test_rows_depend_on_their_mates_only():
    """the group of three alone gives the bits it has in the batch of five"""
    N, rows = 5, [pref.SEES, pref.IN_ONE, pref.IN_TWO]
    d, poly, obs = pref.people_inputs("two", N, 20, 18)
    g, pd = _to_dev(d), _poly_dev(poly)
    box = _boxes(g["x0"], g["x1"], 201, g["R0"], g["T0"], N, pref.B)
    full = _observe_people(g, 20, 18, N, g["choice"], 201, pd, 2, pref.B, box, _groups_dev(pref.IDS), _obs_dev(obs, pref.OBS_INDEX), 1)
    a = _to_dev(pref.take(d, rows))
    pa = (pd[0], pd[1], pd[2][rows].contiguous(), pd[3])
    box_a = _boxes(a["x0"], a["x1"], 201, a["R0"], a["T0"], N, 3)
    assert torch.equal(box_a, box[rows])
    alone = _observe_people(a, 20, 18, N, a["choice"], 201, pa, 2, 3, box_a, _groups_dev([0, 0, 0]), _obs_dev(obs, pref.OBS_INDEX[rows]), 1)
    for one, f in zip(alone, full):
        assert torch.equal(one, f[rows])
    assert alone[4].tolist() == [4, 2, 2]


# ---- argument checks -----------------------------------------------------------------------------------------------------------
def test_argument_checks():
    from egogen_amd import _lib
    z = torch.zeros(4096, device="cuda")
    zi = torch.zeros(16, dtype=torch.int32, device="cuda")
    lib, st = _lib.load(), _lib.current_stream_ptr()

    def call(fpr=20, first=18, N=1, x_ld=201, edges=z, off=zi, idx=zi, S=1, ray=7.0, step=0, md=13, state=z, box=z, gs=zi, gm=zi, mg=zi, G=1,
             oxy=z, orad=z, ocnt=zi, oidx=zi, sets=1, omax=2, T=3, frame=0, count=zi):
        return lib.egx_primitive_observe_people(_vp(z), fpr, first, None, N, _vp(z), _vp(z), _vp(z), _vp(z), _vp(z), _vp(z), x_ld, _vp(z), _vp(edges),
                                                _vp(off), _vp(idx), S, ray, step, md, 1, _vp(box), _vp(gs), _vp(gm), _vp(mg), G, _vp(oxy), _vp(orad),
                                                _vp(ocnt), _vp(oidx), sets, omax, T, frame, _vp(count), _vp(state), _vp(z), _vp(z), _vp(z), st)
    for kw in ({"first": 19}, {"fpr": 1, "first": 0}, {"N": 0}, {"N": 257}, {"x_ld": 200}, {"off": None}, {"edges": None}, {"ray": 0.0}, {"step": -1},
               {"md": 0}, {"state": None}, {"S": 0},                                                   # what egx_primitive_observe rejects
               {"box": None}, {"gs": None}, {"gm": None}, {"mg": None}, {"G": 0}, {"gs": None, "gm": None, "mg": None, "box": None, "count": None},
               {"oxy": None}, {"orad": None}, {"ocnt": None}, {"oxy": None, "orad": None, "ocnt": None}, {"sets": 0}, {"omax": -1}, {"omax": 33},
               {"T": 0}, {"count": None}):
        assert call(**kw) == -1, kw

    def boxes(x0=z, x_ld=201, N=1, box=z, R0=z):
        return lib.egx_primitive_people_boxes(_vp(x0), _vp(z), x_ld, _vp(R0), _vp(z), N, 1, _vp(box), st)
    for kw in ({"x0": None}, {"x_ld": 200}, {"N": 0}, {"N": 257}, {"box": None}, {"R0": None}):
        assert boxes(**kw) == -1, kw
    torch.cuda.synchronize()
    assert not z.any() and not zi.any()


# ---- in the search -------------------------------------------------------------------------------------------------------------
class _Args:
    seed = 0; lr = 3e-4; gamma = 0.99; gae_lambda = 0.95; max_grad_norm = 0.1; vf_coef = 1.0; ent_coef = 0.01
    weight_kld = 0; rew_norm = False; eps_clip = 0.1; value_clip = 0; dual_clip = None; norm_adv = 1; recompute_adv = 0
    deterministic_eval = False


K, N, B4 = 3, 4, 4
GROUPS = [0, 0, 1, 0]


@pytest.fixture(scope="module")
def people_world(search_world):
    """search_world's walkers as four people 1 - 1.5 m apart (walker 0 twice), a seeded policy whose head matters, two recorded tracks
    that pass among them; no static polygon: whatever a ray reads below +1 is a person."""
    from egogen_amd import MovingObstacles, setup_world as sw
    pol = sw.build_policy(_Args())
    with torch.no_grad():
        for p_ in pol.parameters():
            if p_.dim() == 1:
                p_.add_(0.05 * torch.randn(p_.shape, generator=torch.Generator().manual_seed(p_.numel())).cuda())
        pol.actor.pnet.out_fc.weight.mul_(30.0)
    idx = [0, 1, 2, 0]
    T0 = torch.tensor([[0.0, 0.0, 0.0], [1.2, 0.3, 0.0], [-1.0, 0.8, 0.0], [0.4, -1.5, 0.0]])
    t = np.arange(60)[:, None] / 40.0
    tracks = np.stack([np.array([2.5, 1.0]) + t * np.array([-1.0, 0.0]), np.array([-2.0, -1.0]) + t * np.array([0.5, 0.5])])
    w = dict(search_world)
    w.update(policy=pol, T0=T0, data=search_world["data"][:, idx].contiguous(), bparams=search_world["bparams"][:, idx].contiguous(),
             betas=search_world["betas"][idx].contiguous(), goal=search_world["goal"][idx] + T0, tracks=tracks,
             obstacles=MovingObstacles.from_tracks(tracks), z=torch.randn(K, B4 * N, 128, generator=torch.Generator().manual_seed(93)))
    return w


def _run(w, Kp, prop, **extra):
    kw = dict(z=w["z"][:Kp].cuda(), reproj_factor=CFG_RF, weights=W_TEST, goal_thresh=0.0, to_numpy=False, T0=w["T0"], policy=prop,
              groups=GROUPS, obstacles=w["obstacles"], obstacle_frame0=3)
    kw.update(extra)
    with patched_loop(w["op"], "_search_loop", no_host_wait=True) as seen:
        res = w["op"].generate_sequence_to_goal(w["data"], w["bparams"], w["betas"], w["goal"], Kp, N, **kw)
    assert seen.calls == [(Kp, B4, N)]
    return res, seen.s


def test_search_senses_people(people_world):
    from egogen_amd.crowd import PersonGroups
    from egogen_amd.proposal import PolicyProposal
    w, b = people_world, B4
    prop = PolicyProposal(w["policy"], sense_people=True)
    runs = {Kp: _run(w, Kp, prop) for Kp in range(1, K + 1)}
    res, s = runs[K]
    assert res.policy_sense_people is True and res.people_box.shape == (K, b, 4) and res.obs_people_count.shape == (K, b)
    assert res.obs_people_count.tolist() == [[4, 4, 2, 4]] * K                     # two mates and two tracks; the single one the tracks
    assert bool((res.people_box[..., :2] < res.people_box[..., 2:]).all())
    assert float(res.obs_egosensing.min()) < 1.0 and torch.equal(res.choice, res.choice_trace[:, -1])
    crowd = PersonGroups.from_ids(GROUPS, b).to("cuda")
    groups = (crowd.group_start, crowd.group_member, crowd.member_group, len(crowd))
    obs_args, _alive = w["obstacles"].select_args(b)
    goal = w["goal"].cuda()
    assert (prop.ray_len, prop.max_depth) == (RAY_LEN, MAX_DEPTH)
    for k in range(K):           # a run of k primitives is the prefix of the longer one: its loop state is what observation k was made from
        rk, sk = runs[max(k, 1)]
        for name in ("choice", "z", "markers", "obs_egosensing", "people_box", "obs_people_count"):
            assert torch.equal(getattr(rk, name), getattr(res, name)[:max(k, 1)]), (name, k)
        cur = sk["xs"][k % 2]
        if k == 0:
            p0 = sk["policy_start"]
            g = {"joints": p0["joints"], "R_prev": p0["R0"], "T_prev": p0["T0"], "R0": p0["R0"], "T0": p0["T0"], "x0": cur[0], "x1": cur[1], "goal": goal}
            fpr, first, n, choice, x_ld = 2, 0, 1, None, 201 * N
        else:
            g = {"joints": sk["lbs_out"]["joints"], "R_prev": rk.rotmat[k - 1], "T_prev": rk.transl[k - 1], "R0": sk["R0"], "T0": sk["T0"],
                 "x0": cur[0], "x1": cur[1], "goal": goal}
            fpr, first, n, choice, x_ld = 20, 18, N, rk.choice[k - 1], 201
        box = _boxes(g["x0"], g["x1"], x_ld, g["R0"], g["T0"], n, b)
        assert torch.equal(box, res.people_box[k]), k
        direct = _observe_people(g, fpr, first, n, choice, x_ld, (None, None, None, 0), k, b, box, groups, obs_args, 3 + 18 * k)
        for mine, name in zip(direct, ("obs_state", "obs_egosensing", "obs_dist", "obs_time", "obs_people_count")):
            assert torch.equal(mine, getattr(res, name)[k]), (name, k)
        # and the record against the float64 restatement on the same hand-off inputs
        j2 = g["joints"].reshape(b, n, fpr, 127, 3)[torch.arange(b), 0 if choice is None else choice.long(), first:first + 2].cpu()
        x0, x1 = (t.reshape(-1)[:b * n * x_ld].reshape(b, n * x_ld)[:, :201].cpu() for t in (g["x0"], g["x1"]))
        R0, T0 = g["R0"].reshape(-1, 3, 3)[::n].cpu(), g["T0"][::n].cpu()
        od = (w["obstacles"].xy, w["obstacles"].radius, w["obstacles"].count)
        args = (j2, g["R_prev"].reshape(b, 3, 3).cpu(), g["T_prev"].cpu(), R0, T0, x0, x1, goal.cpu(), None, prop.ray_len, k, prop.max_depth)
        kw = dict(groups=pref.csr(GROUPS), obs=od, obs_index=None, frame=3 + 18 * k)
        t64 = pref.observe_people(*args, torch.float64, **kw)
        und = torch.zeros(b, 2, 32, dtype=torch.bool)
        for sx, sy in ((ref.SHIFT, 0.0), (-ref.SHIFT, 0.0), (0.0, ref.SHIFT), (0.0, -ref.SHIFT)):
            und |= (pref.observe_people(*args, torch.float64, eye_shift=(sx, sy), **kw)[1].double() - t64[1].double()).abs() > ref.EGO_FLOOR
        _check_rays("search obs_egosensing", f"k={k}", res.obs_egosensing[k], t64[1], und)
        held("search people_box", f"k={k}", res.people_box[k], t64[5], pref.boxes(x0, x1, R0, T0, torch.float32))
        assert t64[4].tolist() == res.obs_people_count[k].tolist()


def test_sense_people_off_is_the_search_as_it_was(people_world):
    from egogen_amd.proposal import PolicyProposal
    w = people_world
    never, _ = _run(w, 2, PolicyProposal(w["policy"]))
    off, _ = _run(w, 2, PolicyProposal(w["policy"], sense_people=False))
    on, _ = _run(w, 2, PolicyProposal(w["policy"], sense_people=True))
    assert set(never.search) == set(off.search)
    for k, v in never.search.items():
        same = torch.equal(v, off.search[k]) if torch.is_tensor(v) else v == off.search[k]
        assert same, k
    for k in ("markers", "params", "rotmat", "transl", "pelvis", "z", "R0", "T0"):
        assert torch.equal(getattr(never, k), getattr(off, k)), k
    assert off.people_box is None and off.obs_people_count is None and off.policy_sense_people is False
    assert torch.equal(off.obs_egosensing, torch.ones_like(off.obs_egosensing))      # no polygon: the blind policy reads +1 everywhere
    assert not torch.equal(on.obs_egosensing, off.obs_egosensing) and torch.equal(on.obs_state[0], off.obs_state[0])
    # without groups and obstacles the sensing policy is the blind one, bit for bit
    alone_on, _ = _run(w, 2, PolicyProposal(w["policy"], sense_people=True), groups=None, obstacles=None)
    alone_off, _ = _run(w, 2, PolicyProposal(w["policy"]), groups=None, obstacles=None)
    for k in ("markers", "z", "choice", "cost", "obs_state", "obs_egosensing", "obs_dist", "obs_time", "policy_mu", "policy_logvar"):
        assert torch.equal(getattr(alone_on, k), getattr(alone_off, k)), k
    assert not alone_on.obs_people_count.any() and bool(torch.isfinite(alone_on.people_box).all())
