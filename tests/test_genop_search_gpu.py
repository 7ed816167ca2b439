"""GPU checks of the primitive search: kernels egx_primitive_select and egx_primitive_advance_select (csrc/genop.hip) and
`GAMMAPrimitiveComboGenOP.generate_sequence_to_goal` (egogen_amd/genop.py).

Yardsticks.  Values: `held()` of tests/genop_gpu_helpers.py - the device within R = 3 times the distance of the float32 restatement
(tests/genop_search_ref.py) from the float64 one, largest entry of a group.  A group is one term (or the cost) over the rows of a
case; the statistic compares two maxima of rounding errors, which says nothing on a handful of values (one row: a restatement that
happens to round to the truth admits no kernel at all), so a case with fewer than 64 rows is launched on as many independent
input draws as it takes to pool 64, every launch at the case's own b and N.  Choices: equal to the float64 choice for every DECIDABLE group - one in which,
in float64, the runner-up of the winner's class is further from the winner than 6 times the largest |cost_f32 - cost_f64| of the
group's rows (3x for each of the two costs compared); the undecidable groups are at most 5 % of the groups, a property of
the inputs alone that is checked on the restatements and printed.  Everything else (flags, status, copies, hand-off against
egx_primitive_advance) is exact."""
import ctypes as C
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import genop_search_ref as sref
from tests.genop_gpu_helpers import (CFG_RF, MIN_GROUP, POOL, ROOT, UNDECIDABLE_CAP, V_SMALL, W_TEST, _advance_select, _feet, _handmade, _inputs,
                                     _launch, _restate, _rows_inputs, _select, emit, held, patched_loop, search_world, small_world)  # noqa: F401
from tests.test_genop_search_cpu import selection_cases

pytestmark = pytest.mark.gpu


def decidable(cost64, terms64, coll, cost32):
    """[b] bool: the float64 winner is ahead of the runner-up of its class by more than 6 x max_rows |cost32 - cost64|"""
    choice, _ = sref.select(cost64, terms64, coll)
    cls = sref.rank_class(cost64, terms64, coll)
    ok = torch.ones(cost64.shape[0], dtype=torch.bool)
    for g in range(cost64.shape[0]):
        w = int(choice[g])
        same = [n for n in range(cost64.shape[1]) if n != w and int(cls[g, n]) == int(cls[g, w])]
        if not same or int(cls[g, w]) >= 2:
            continue
        gap = min(float(cost64[g, n]) for n in same) - float(cost64[g, w])
        err = float((cost32[g].double() - cost64[g]).abs().max())
        ok[g] = gap > 6.0 * err
    return choice, ok


def _draws(b, N):
    """Independent input draws pooled into one case: at least MIN_GROUP candidate rows in all."""
    return max(1, -(-MIN_GROUP // (b * N)))


@pytest.mark.parametrize("with_pene", [True, False])
@pytest.mark.parametrize("jpb", [127, 55])
@pytest.mark.parametrize("N", [1, 2, 5, 70])
@pytest.mark.parametrize("b", [1, 3, 65])
def test_primitive_select_kernel(small_world, b, N, jpb, with_pene):
    name = f"select b={b} N={N} jpb={jpb} pene={int(with_pene)}"
    got, r64, r32, oks = [], [], [], []
    for draw in range(_draws(b, N)):
        x = _rows_inputs(small_world, b, N, 100 + b * 7 + N + 1000 * draw, with_pene)
        o, i = _select(x, jpb)
        c64, t64, coll = _restate(i, b, N, CFG_RF, W_TEST, 40.0, torch.float64)
        c32, t32, coll32 = _restate(i, b, N, CFG_RF, W_TEST, 40.0, torch.float32)
        got.append((o["cost"], o["terms"]))
        r64.append((c64, t64))
        r32.append((c32, t32))
        assert torch.equal(o["colliding"].bool(), coll) and torch.equal(coll32, coll)
        if with_pene and b * N >= 10:
            assert coll.any() and not coll.all()
        choice64, ok = decidable(c64, t64, coll, c32)
        choice32, _ = sref.select(c32, t32, coll)
        oks.append(ok)
        assert torch.equal(choice32[ok], choice64[ok])          # the float32 restatement itself decides those groups alike
        assert torch.equal(o["choice"].long()[ok], choice64[ok]), (name, draw, o["choice"], choice64)
        # what follows from the kernel's own choice is exact
        ch = o["choice"].long()
        assert int(ch.min()) >= 0 and int(ch.max()) < N
        pick = lambda t: t.gather(1, ch[:, None])[:, 0]
        assert torch.equal(o["status"], pick(o["colliding"]))                      # all rows finite: bit 0 only
        assert torch.equal(o["goal_dist"], pick(o["terms"][..., 0]))
        assert torch.equal(o["reached"].bool(), o["goal_dist"] < 0.1)
        # the kernel's choice obeys the four rules on the kernel's own costs
        own, own_status = sref.select(o["cost"], o["terms"], o["colliding"].bool())
        assert torch.equal(own, ch) and torch.equal(own_status.int(), o["status"])
    cat = lambda lst, j: torch.cat([v[j] for v in lst], 0)
    for k, term in enumerate(sref.TERMS):
        held(name, term, cat(got, 1)[..., k], cat(r64, 1)[..., k], cat(r32, 1)[..., k])
    held(name, "cost", cat(got, 0), cat(r64, 0), cat(r32, 0))
    ok = torch.cat(oks)
    share = 1.0 - float(ok.float().mean())
    emit(f"| {name} | undecidable groups | {int((~ok).sum())} of {ok.numel()} | {share:.3f} | |")
    assert share <= UNDECIDABLE_CAP, (name, share)


@pytest.mark.parametrize("name", list(selection_cases()))
def test_primitive_select_handmade_cases(small_world, name):
    costs, coll, nan_rows, want, status = selection_cases()[name]
    x = _handmade(small_world, costs, coll)
    o, _ = _select(x, 127, weights={"goal": 1.0, "skate": 0.0, "floor": 0.0, "pene": 0.0, "face": 0.0}, nan_face_rows=nan_rows)
    assert o["colliding"][0].tolist() == list(coll)
    fin = torch.isfinite(o["cost"][0]).tolist()
    assert fin == [bool(np.isfinite(c)) and n not in nan_rows for n, c in enumerate(costs)], (name, o["cost"])
    for n in nan_rows:
        assert bool(torch.isfinite(o["terms"][0, n, 0])) and not bool(torch.isfinite(o["terms"][0, n, 4]))
    assert int(o["choice"][0]) == want and int(o["status"][0]) == status, (name, o["choice"], o["status"], o["cost"])


def test_primitive_select_group_does_not_depend_on_batch(small_world):
    x = _rows_inputs(small_world, 65, 5, 31, True)
    full, _ = _select(x, 127)
    for g in (0, 1, 33, 64):
        one, _ = _select(x, 127, b=1, group0=g)
        for k in ("choice", "status", "reached", "goal_dist", "cost", "terms", "colliding"):
            assert torch.equal(one[k][0], full[k][g]), (g, k)


@pytest.mark.parametrize("jpb", [127, 55])
@pytest.mark.parametrize("B", [3, 65])
def test_advance_select_with_one_candidate_is_the_advance(small_world, B, jpb):
    d = _inputs(small_world, B)
    nf_a, nf_b = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    want = _launch(d, list(range(B)), jpb, CFG_RF, nf_a)
    got = _advance_select(d, list(range(B)), [0] * B, 1, jpb, CFG_RF, nf_b)
    for k in ("marker_b", "pelvis", "R", "T", "R0", "T0", "seed_params", "seed_markers"):
        assert torch.equal(got[k], want[k]), k
    assert torch.equal(got["params"], d["pp"])
    assert int(nf_a.item()) == int(nf_b.item()) == 0


@pytest.mark.parametrize("jpb", [127, 55])
def test_advance_select_hands_the_chosen_row_to_its_group(small_world, jpb):
    d = _inputs(small_world, POOL)
    N, b = 5, 13
    g = torch.Generator().manual_seed(5)
    choice = torch.randint(0, N, (b,), generator=g)
    assert len(set(choice.tolist())) > 2
    rows = torch.randperm(POOL, generator=g)                   # R0 / T0 of the pool differ from row to row
    chosen = rows.reshape(b, N).gather(1, choice[:, None])[:, 0]
    want = _launch(d, chosen.tolist(), jpb, CFG_RF)
    got = _advance_select(d, rows.tolist(), choice.tolist(), N, jpb, CFG_RF)
    for k in ("marker_b", "pelvis", "R", "T"):
        assert torch.equal(got[k], want[k]), k
    assert torch.equal(got["params"], d["pp"][chosen.cuda()])
    for k in ("R0", "T0", "seed_params", "seed_markers"):       # the winner's next state in all N rows, R0 / T0 in place
        assert torch.equal(got[k], want[k].repeat_interleave(N, 0)), k
    # a choice outside the group is clamped, never followed
    lo = _advance_select(d, rows.tolist(), [-3] * b, N, jpb, CFG_RF)
    hi = _advance_select(d, rows.tolist(), [N + 2] * b, N, jpb, CFG_RF)
    assert torch.equal(lo["pelvis"], _launch(d, rows.reshape(b, N)[:, 0].tolist(), jpb, CFG_RF)["pelvis"])
    assert torch.equal(hi["pelvis"], _launch(d, rows.reshape(b, N)[:, N - 1].tolist(), jpb, CFG_RF)["pelvis"])


def test_search_kernels_reject_bad_arguments(small_world):
    """Rejected before anything is launched: every pointer may therefore be the same scratch buffer."""
    from egogen_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(16384, device="cuda")
    p, off = C.c_void_p(buf.data_ptr()), C.c_void_p(buf.data_ptr() + 4)
    w = (C.c_float * 5)(1, 1, 1, 1, 0)

    def adv(mproj=p, jpb=127, x_ld=201, B=1, N=1, out_marker=p, choice=p):
        return lib.egx_primitive_advance_select(p, p, p, p, x_ld, p, jpb, mproj, p, 0.5, B, choice, N, p, p, out_marker, p, p, p, None, p, p, p,
                                                201, None, _lib.current_stream_ptr())

    def sel(goal=p, jpb=127, x_ld=201, B=1, N=1, weights=w, choice=p):
        return lib.egx_primitive_select(p, p, p, x_ld, p, jpb, p, p, p, None, goal, p, weights, 40.0, 0.1, 0.5, B, N, choice, p, p, p, p, p, p,
                                        _lib.current_stream_ptr())
    for kw in ({"mproj": off}, {"out_marker": off}, {"jpb": 2}, {"x_ld": 200}, {"B": 0}, {"mproj": None}, {"N": 0}, {"N": 257}, {"choice": None}):
        assert adv(**kw) != 0, kw
        with pytest.raises(_lib.EgxError):
            _lib.check(adv(**kw), "egx_primitive_advance_select")
    for kw in ({"goal": None}, {"jpb": 2}, {"x_ld": 200}, {"B": 0}, {"N": 0}, {"N": 257}, {"weights": None}, {"choice": None}):
        assert sel(**kw) != 0, kw
        with pytest.raises(_lib.EgxError):
            _lib.check(sel(**kw), "egx_primitive_select")


# ----------------------------------------------------------------------------------------------------------------------
def test_one_candidate_without_scene_is_generate_sequence(search_world):
    w = search_world
    op, K, b = w["op"], 3, w["b"]
    z = torch.randn(K, b, 128, generator=torch.Generator().manual_seed(1))
    want = op.generate_sequence(w["data"], w["bparams"], w["betas"], K, z=z, reproj_factor=CFG_RF)
    got = op.generate_sequence_to_goal(w["data"], w["bparams"], w["betas"], w["goal"], K, 1, z=z, reproj_factor=CFG_RF, goal_thresh=0.0)
    for k in ("markers", "params", "rotmat", "transl", "pelvis", "z", "betas", "R0", "T0"):
        assert np.array_equal(getattr(got, k), getattr(want, k)), k
    assert got.choice.shape == (K, b) and not got.choice.any() and not got.status.any() and not got.colliding.any()
    assert got.cost.shape == (K, b, 1) and got.cost_terms.shape == (K, b, 1, 5) and got.goal_dist.shape == (K, b)
    assert got.n_valid.tolist() == [K] * b and want.n_valid is None and len(want.primitives(0)) == K


def test_search_chain_matches_float64(search_world, small_world):
    from oracle.smplx_lbs import BodyModel
    from tests.test_env_reference_goldens import _aa_close, _close
    w = search_world
    op, K, b, N = w["op"], 3, w["b"], 4
    z = torch.randn(K, b * N, 128, generator=torch.Generator().manual_seed(2))
    res = op.generate_sequence_to_goal(w["data"], w["bparams"], w["betas"], w["goal"], K, N, z=z, reproj_factor=CFG_RF, weights=W_TEST,
                                       goal_thresh=0.0)
    ref = {dt: sref.search_chain(w["sd"], BodyModel(small_world["bm"], dtype=dt), small_world["mk"], _feet(), w["data"].permute(1, 0, 2),
                                 w["pp"][:, :2], torch.eye(3).repeat(b, 1, 1), torch.zeros(b, 3), w["betas"], z, w["goal"], N, CFG_RF, W_TEST,
                                 goal_thresh=0.0) for dt in (torch.float64, torch.float32)}
    r64, r32 = ref[torch.float64], ref[torch.float32]
    undecided, compared = 0, 0
    for i in range(b):
        for k in range(K):
            coll = torch.zeros(1, N, dtype=torch.bool)
            c64, ok = decidable(r64[k]["cost"][i:i + 1], r64[k]["terms"][i:i + 1], coll, r32[k]["cost"][i:i + 1])
            if not bool(ok[0]) or int(r32[k]["choice"][i]) != int(c64[0]):
                undecided += 1       # from here on the float32 chain and the device may follow another candidate
                break
            assert int(res.choice[k, i]) == int(c64[0]), (i, k, res.choice[:, i], res.cost[k, i], r64[k]["cost"][i])
            compared += 1
            what = f"sequence {i} primitive {k} "
            _close(res.markers[k, i], r64[k]["marker_b"][i], "m", what + "marker_b")
            _close(res.pelvis[k, i], r64[k]["pelvis"][i], "m", what + "pelvis")
            _close(res.rotmat[k, i], r64[k]["R"][i], "unit", what + "R")
            _close(res.transl[k, i], r64[k]["T"][i], "m", what + "T")
            _close(res.params[k, i, :, :3], r64[k]["pred_params"][i, :, :3], "m", what + "transl")
            _aa_close(res.params[k, i, :, 3:6], r64[k]["pred_params"][i, :, 3:6], what + "glorot")
            _close(res.params[k, i, :, 6:], r64[k]["pred_params"][i, :, 6:], "unit", what + "pose")
            _close(res.goal_dist[k, i], r64[k]["goal_dist"][i], "m", what + "goal_dist")
    share = undecided / (b * K)
    emit(f"| search chain b={b} N={N} K={K} | undecidable decisions | {undecided} of {b * K} | {share:.3f} | compared {compared} |")
    assert share <= UNDECIDABLE_CAP, share
    assert len(set(res.choice.reshape(-1).tolist())) > 1          # the search did choose


# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scenes", [1, 2])
def test_scene_invariants(search_world, scenes):
    from egogen_amd import synth
    from egogen_amd.body_model import SdfScene, SdfSceneSet
    w = search_world
    op, h, b, N, K = w["op"], w["handle"], w["b"], 8, 2
    box = SdfScene(synth.make_sdf_scene(32))                                                   # box x 1..2, y -0.5..0.5, z 0..1
    T0 = torch.tensor([[-1.0, -1.0, 0.0], [1.5, -0.2, 0.0], [1.5, -0.75, 0.0]])               # beside, inside, at its edge
    if scenes == 1:
        scene, agent_scene = box, None
    else:       # the second scene has its box where walker 0 stands; walker 1 is sent there too, out of the first scene's box
        other = SdfScene(synth.make_sdf_scene(32, obstacle=([-1.5, -1.5, 0.0], [-0.5, -0.5, 1.0])))
        scene, agent_scene = SdfSceneSet([box, other]), [1, 1, 0]
    z = torch.randn(K, b * N, 128, generator=torch.Generator().manual_seed(3 + scenes))
    with patched_loop(op, "_search_loop") as seen:
        res = op.generate_sequence_to_goal(w["data"], w["bparams"], w["betas"], w["goal"] + T0, K, N, scene=scene, agent_scene=agent_scene,
                                           z=z, reproj_factor=CFG_RF, T0=T0, to_numpy=False)
    s = seen.s
    # the counts the last selection consumed are BodyModelHandle.forward's for the same rows in the frame of that primitive
    rep = lambda t: t.repeat_interleave(N, 0).contiguous()
    kw = {} if scenes == 1 else {"agent_scene": s["rows_scene"]}
    fresh = h.forward(s["pp"].view(b * N * 20, 93), s["bt"], 20, want_verts=False, sdf=scene, R0=rep(res.rotmat[K - 1]),
                      T0=rep(res.transl[K - 1]), **kw)["pene_count"]
    used = s["lbs_out"]["pene_count"]
    assert torch.equal(fresh, used) and int(used.min()) >= 0
    cnt = used.reshape(b, N, 20)
    assert torch.equal(res.colliding[K - 1].bool(), cnt.max(-1).values >= 40)
    # (on the CPU: a true division, which the device's division by a scalar in torch is not)
    assert torch.equal(res.cost_terms[K - 1, :, :, 3].cpu(), cnt.cpu().sum(-1).float() / 20 / 10)
    coll = res.colliding.bool().cpu()
    emit(f"| scene invariants scenes={scenes} | colliding candidates per (k, sequence) | {coll.sum(-1).tolist()} | | |")
    assert coll.any() and not coll.all()
    for k in range(K):
        choice, status = sref.select(res.cost[k].cpu(), res.cost_terms[k].cpu(), coll[k])
        assert torch.equal(choice, res.choice[k].cpu().long()), (k, choice, res.choice[k])
        assert torch.equal(status.int(), res.status[k].cpu())
        assert torch.equal((res.status[k].cpu() & 1).bool(), coll[k].all(-1))                  # bit 0 exactly where every sibling collides
    # every candidate of a group started primitive k from the same state: the seed frames of the records are the winner's
    assert torch.equal(res.R0, s["R0"][::N]) and all(torch.equal(s["R0"][n::N], s["R0"][::N]) for n in range(N))


def test_n_valid_truncates_primitives_and_files(search_world, tmp_path):
    from egogen_amd.utils import rollout_primitives
    w = search_world
    op, h, K, b, N = w["op"], w["handle"], 3, w["b"], 2
    z = torch.randn(K, b * N, 128, generator=torch.Generator().manual_seed(4))
    # w_goal = 0 (and the default w_face = 0): no choice depends on the goal, so both runs below choose alike
    wts = {"goal": 0.0, "skate": 1.0, "floor": 1.0}
    nowhere = np.asarray([40.0, 40.0, 0.9], np.float32)
    far = op.generate_sequence_to_goal(w["data"], w["bparams"], w["betas"], nowhere, K, N, z=z, reproj_factor=CFG_RF, weights=wts)
    assert far.n_valid.tolist() == [K] * b and far.goal.shape == (b, 3)
    goal = far.pelvis[0, :, 19].copy()                  # identity start frame: the first primitive's end pelvis in the world
    goal[2] = nowhere                                   # ... for sequences 0 and 1; sequence 2 never arrives
    res = op.generate_sequence_to_goal(w["data"], w["bparams"], w["betas"], goal, K, N, z=z, reproj_factor=CFG_RF, weights=wts)
    assert np.array_equal(res.choice, far.choice) and np.array_equal(res.pelvis, far.pelvis)
    assert res.n_valid.tolist() == [1, 1, K]
    assert np.all(res.goal_dist[0, :2] < 0.1) and len(res.primitives(0)) == 1 and len(res.primitives(2)) == K
    for i in (0, 2):
        path = res.save(str(tmp_path), i, man_id=f"goal{i}")
        with open(path, "rb") as fh:
            node = pickle.load(fh)
        assert len(node["motion"]) == int(res.n_valid[i])
        assert np.allclose(node["wpath"][1], goal[i]) and np.allclose(node["wpath"][0], res.pelvis[0, i, 0], atol=1e-6)
        seq = rollout_primitives(node["motion"], h)
        assert seq.shape == (2 + 18 * int(res.n_valid[i]), 93) and np.isfinite(seq).all()


def test_search_loop_has_no_host_wait(search_world):
    """torch-level synchronisation only, as tests/test_genop_gpu.py::test_generate_sequence_loop_has_no_host_wait"""
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.skip("this torch build has no torch.cuda.set_sync_debug_mode")
    from egogen_amd import synth
    from egogen_amd.body_model import SdfScene
    w = search_world
    op = w["op"]
    scene = SdfScene(synth.make_sdf_scene(32))
    args = (w["data"], w["bparams"], w["betas"], w["goal"])
    op.generate_sequence_to_goal(*args, 1, 4, scene=scene)      # weight images, workspaces
    with patched_loop(op, "_search_loop", no_host_wait=True) as seen:
        res = op.generate_sequence_to_goal(*args, 3, 4, scene=scene)
    ran = seen.calls
    assert ran == [(3, w["b"], 4)] and np.isfinite(res.markers).all()


def test_generate_sequence_to_goal_argument_handling(search_world):
    from egogen_amd import _lib, synth
    from egogen_amd.body_model import SdfScene, SdfSceneSet
    w = search_world
    op, b = w["op"], w["b"]
    args = (w["data"], w["bparams"], w["betas"])
    with pytest.raises(ValueError, match="z must be"):
        op.generate_sequence_to_goal(*args, w["goal"], 2, 4, z=torch.zeros(2, b, 128))
    with pytest.raises(ValueError, match="256"):
        op.generate_sequence_to_goal(*args, w["goal"], 1, 257)
    with pytest.raises(ValueError, match="n_candidates"):
        op.generate_sequence_to_goal(*args, w["goal"], 1, 0)
    with pytest.raises(ValueError, match="goal must be"):
        op.generate_sequence_to_goal(*args, torch.zeros(b + 1, 3), 1, 2)
    with pytest.raises(ValueError, match="unknown weights"):
        op.generate_sequence_to_goal(*args, w["goal"], 1, 2, weights={"look": 1.0})
    scene = SdfScene(synth.make_sdf_scene(16))
    with pytest.raises(ValueError, match="agent_scene needs an SdfSceneSet"):
        op.generate_sequence_to_goal(*args, w["goal"], 1, 2, scene=scene, agent_scene=[0] * b)
    with pytest.raises(ValueError, match="agent_scene"):
        op.generate_sequence_to_goal(*args, w["goal"], 1, 2, scene=SdfSceneSet([scene]))
    with pytest.raises(ValueError, match="indices in"):
        op.generate_sequence_to_goal(*args, w["goal"], 1, 2, scene=SdfSceneSet([scene]), agent_scene=[0, 1, 0])
    one = op.generate_sequence_to_goal(*args, w["goal"][0], 1, 2, to_numpy=False)           # a single goal for all, z drawn, torch out
    assert one.markers.is_cuda and one.goal.shape == (b, 3) and one.z.shape == (1, b, 128)
    bm, op.body_model = op.body_model, None
    try:
        with pytest.raises(_lib.EgxError, match="body model"):
            op.generate_sequence_to_goal(*args, w["goal"], 1, 2)
    finally:
        op.body_model = bm


def test_gen_motion_driver_goal_search(tmp_path):
    """The driver with --goal; its path without --goal is tests/test_genop_gpu.py::test_gen_motion_driver_writes_readable_files."""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    base = [sys.executable, os.path.join(ROOT, "exp_GAMMAPrimitive", "gen_motion.py"), "--n-primitives", "2", "--seed", "3", "--num-verts",
            str(V_SMALL)]
    scene_file = tmp_path / "scene.npz"
    from egogen_amd import synth
    sc = synth.make_sdf_scene(16)
    np.savez(scene_file, sdf=sc["sdf"], center=sc["center"], scale=sc["scale"])
    out = tmp_path / "goal"
    r = subprocess.run(base + ["--n-gens", "2", "--goal", "40,40,0.9", "--n-candidates", "4", "--scene", str(scene_file), "--out", str(out)],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    files = sorted(f for f in os.listdir(out) if f.startswith("motion_") and f.endswith(".pkl"))
    assert len(files) == 2, files
    for f in files:
        with open(out / f, "rb") as fh:
            node = pickle.load(fh)
        assert len(node["motion"]) == 2 and node["motion"][0]["smplx_params"].shape == (1, 20, 93)
        assert np.allclose(node["wpath"][1], [40.0, 40.0, 0.9])
    assert "frames: 38" in r.stdout, r.stdout[-500:]
