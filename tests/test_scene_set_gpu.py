"""Scene sets (egx_lbs_forward_scenes): one LBS + SDF-count launch over bodies in different scenes of the same grid dimensions.
Each body's count, joints and markers must be those of a one-scene launch (egx_lbs_forward) of the same bodies in its own scene;
an env over a set must behave like one-scene envs, and main_ppo trains across a list of scenes."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

from egogen_amd import scene_gen, synth
from tests.helpers import level_set_band

pytestmark = pytest.mark.gpu

MODES = {"f32": 0, "bf16x3": 1, "bf16x2": 2, "f16mix": 3}


@pytest.fixture(params=list(MODES))
def blend_mode(request):
    from egogen_amd import _lib
    lib = _lib.load()
    old = int(lib.egx_lbs_get_blend_mode())
    _lib.check(lib.egx_lbs_set_blend_mode(MODES[request.param]), "egx_lbs_set_blend_mode")
    yield request.param
    _lib.check(lib.egx_lbs_set_blend_mode(old), "egx_lbs_set_blend_mode")


@pytest.fixture(autouse=True)
def large_wave_tile():
    """Set launches of two or more scenes always run the 32 x 64 wave tile of the mixed blend; the one-scene launches they are
    compared with bit for bit run it too (a small launch would otherwise take the 32 x 32 tile, whose arithmetic order differs)."""
    from egogen_amd import _lib
    lib = _lib.load()
    old = int(lib.egx_lbs_get_wave_tile())
    _lib.check(lib.egx_lbs_set_wave_tile(2), "egx_lbs_set_wave_tile")
    yield
    _lib.check(lib.egx_lbs_set_wave_tile(old), "egx_lbs_set_wave_tile")


# three rooms: different cube centres and sizes (scales), different obstacles; 48^3 grids
_ROOMS = [((0.0, 0.0, 1.0), 2.5, [((-1.0, -1.0, 0.0), (0.2, 0.3, 1.0)), ((0.8, 0.5, 0.0), (1.6, 1.8, 0.6))]),
          ((0.4, -0.3, 1.2), 3.0, [((-2.0, 0.0, 0.0), (-0.5, 1.5, 1.4))]),
          ((-0.2, 0.5, 0.9), 2.0, [((0.0, -1.2, 0.0), (1.2, 0.0, 0.9)), ((-1.5, 0.6, 0.0), (-0.6, 1.5, 2.0))])]


@pytest.fixture(scope="module")
def scenes():
    out = []
    for c, half, boxes in _ROOMS:
        lo = np.array(c) - np.array([half * 0.85, half * 0.85, 1.0])
        hi = np.array(c) + np.array([half * 0.85, half * 0.85, 1.4])
        lo[2] = -0.05
        room = scene_gen.box_mesh(lo, hi)
        obst = scene_gen.merge_meshes([scene_gen.box_mesh(a, b) for a, b in boxes])
        out.append(scene_gen.scene_sdf_dict(room, obst, res=48, center=c, half=half))
    return out


@pytest.fixture(scope="module")
def model():
    from egogen_amd.body_model import BodyModelHandle
    from oracle.smplx_lbs import BodyModel
    V = 2048
    bm = synth.make_body_model(0, num_verts=V)
    mk, feet = synth.marker_ids(V), synth.feet_vids(V)
    return bm, feet, BodyModelHandle(bm, mk, feet), BodyModel(bm)


def _bodies(A, T, seed):
    """Random bodies and agent frames: most agents stand inside their room (some inside obstacles), some straddle or leave the
    cube (border clamp)."""
    g = torch.Generator().manual_seed(seed)
    B = A * T
    xb = torch.zeros(B, 93)
    xb[:, 0:2] = torch.randn(B, 2, generator=g) * 0.05
    xb[:, 2] = 0.9 + 0.1 * torch.rand(B, generator=g)
    xb[:, 3:6] = torch.randn(B, 3, generator=g) * 0.3
    xb[:, 6:69] = torch.randn(B, 63, generator=g) * 0.2
    xb[:, 69:] = torch.randn(B, 24, generator=g) * 0.5
    betas = torch.randn(A, 10, generator=g)
    yaw = torch.rand(A, generator=g) * 6.28
    R0 = torch.zeros(A, 3, 3)
    R0[:, 0, 0], R0[:, 0, 1], R0[:, 1, 0], R0[:, 1, 1], R0[:, 2, 2] = yaw.cos(), -yaw.sin(), yaw.sin(), yaw.cos(), 1.0
    T0 = torch.cat([torch.rand(A, 2, generator=g) * 7 - 3.5, torch.rand(A, 1, generator=g) * 0.3 - 0.1], -1)
    return xb, betas, R0, T0


def _run(h, xb, betas, T, R0, T0, sdf, agent_scene=None, want_verts=False):
    out = h.forward(xb.cuda(), betas.cuda(), T, want_verts=want_verts, sdf=sdf, R0=R0.cuda(), T0=T0.cuda(), agent_scene=agent_scene)
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in out.items()}


@pytest.mark.parametrize("A,T", [(37, 1), (261, 20)])   # B % 32 != 0; 37 and 5 220 bodies (one and 21 body groups)
def test_mixed_launch_is_bit_identical_to_one_scene_launches(model, scenes, blend_mode, A, T):
    from egogen_amd.body_model import SdfScene, SdfSceneSet
    bm, feet, h, _ = model
    xb, betas, R0, T0 = _bodies(A, T, seed=A * 7 + T)
    one = [SdfScene(s) for s in scenes]
    sset = SdfSceneSet(one)
    assert len(sset) == 3
    g = torch.Generator().manual_seed(A)
    agent_scene = torch.randint(0, 3, (A,), generator=g, dtype=torch.int32)   # interleaved
    wv = A * T < 100   # the vertex-writing kernel too (all vertices of every body, in its own scene)
    mixed = _run(h, xb, betas, T, R0, T0, sset, agent_scene, want_verts=wv)
    fixed_mixed = h.fix_stats(A * T) if blend_mode == "f16mix" else 0
    body_scene = agent_scene.repeat_interleave(T).cuda()
    seen = 0
    for s in range(3):
        ref = _run(h, xb, betas, T, R0, T0, one[s], want_verts=wv)
        m = body_scene == s
        for k in ("pene_count", "joints", "markers") + (("vertices",) if wv else ()):
            assert torch.equal(mixed[k][m], ref[k][m]), (s, k)
        seen += int(m.sum())
        if s == 0:
            assert ref["pene_count"].max() > 50 and ref["pene_count"].min() >= 0
    assert seen == A * T
    if blend_mode == "f16mix" and A * T > 5120:
        assert fixed_mixed > 0, "the fix-up band should be active (bodies inside obstacles and walls)"


def test_counts_match_the_oracle_per_scene(model, scenes, blend_mode):
    """The mixed launch's counts against the CPU oracle, each body in its own scene, within the level-set band."""
    from egogen_amd.body_model import SdfSceneSet
    from oracle.sdf import calc_sdf
    from oracle.smplx_lbs import smplx_forward
    bm, feet, h, ob = model
    A, T = 12, 4
    xb, betas, R0, T0 = _bodies(A, T, seed=5)
    agent_scene = torch.tensor([0, 1, 2] * 4, dtype=torch.int32)
    out = _run(h, xb, betas, T, R0, T0, SdfSceneSet(scenes), agent_scene)
    V = bm["v_template"].shape[0]
    v, _ = smplx_forward(ob, xb, betas.repeat_interleave(T, 0))
    vw = (torch.einsum("bij,btpj->btpi", R0, v.reshape(A, T, V, 3)) + T0[:, None, None, :]).reshape(A * T, V, 3)
    got = out["pene_count"].cpu().long()
    body_scene = agent_scene.repeat_interleave(T)
    total = 0
    for s, sc in enumerate(scenes):
        m = body_scene == s
        sd = {k: sc[k].detach().cpu() for k in ("sdf", "center", "scale")}
        sv = calc_sdf(vw[m], sd)
        sv[:, torch.as_tensor(feet).long()] = 1.0
        ref, near = sv.lt(0).sum(-1), (sv.abs() < level_set_band()).sum(-1)
        assert ((got[m] - ref).abs() <= near).all(), (s, (got[m] - ref).abs().max())
        total += int(ref.sum())
    assert total > 0


def test_set_of_one_equals_egx_lbs_forward(model, scenes, blend_mode):
    from egogen_amd.body_model import SdfScene, SdfSceneSet
    bm, feet, h, _ = model
    A, T = 45, 3
    xb, betas, R0, T0 = _bodies(A, T, seed=9)
    sc = SdfScene(scenes[1])
    one = SdfSceneSet([sc])
    zeros = torch.zeros(A, dtype=torch.int32)
    for wv in (False, True):
        a = _run(h, xb, betas, T, R0, T0, sc, want_verts=wv)
        b = _run(h, xb, betas, T, R0, T0, one, zeros, want_verts=wv)
        assert set(a) == set(b)
        for k in a:
            assert torch.equal(a[k], b[k]), (wv, k)


def test_bad_scene_index_gives_minus_one(model, scenes):
    """agent_scene outside [0, S): the agent's bodies get the count -1 and nothing outside the set is read; the other agents and
    every body's joints / markers are unaffected."""
    from egogen_amd.body_model import SdfScene, SdfSceneSet
    bm, feet, h, _ = model
    A, T = 10, 4
    xb, betas, R0, T0 = _bodies(A, T, seed=13)
    sset = SdfSceneSet(scenes[:2])
    agent_scene = torch.tensor([0, -1, 1, 2, 0, 1, 1 << 20, 0, -(1 << 30), 1], dtype=torch.int32)
    bad = torch.tensor([False, True, False, True, False, False, True, False, True, False]).repeat_interleave(T).cuda()
    out = _run(h, xb, betas, T, R0, T0, sset, agent_scene)
    assert (out["pene_count"][bad] == -1).all()
    for s in range(2):
        ref = _run(h, xb, betas, T, R0, T0, SdfScene(scenes[s]))
        m = (agent_scene.repeat_interleave(T) == s).cuda()
        assert torch.equal(out["pene_count"][m], ref["pene_count"][m])
        assert torch.equal(out["joints"], ref["joints"]) and torch.equal(out["markers"], ref["markers"])
    assert (out["pene_count"][~bad] >= 0).all()
    # a set of one (the one-scene kernels, then the -1 of bad indices)
    one = SdfSceneSet(scenes[:1])
    a1 = torch.tensor([0, -1, 0, 1, 0, 0, 7, 0, -3, 0], dtype=torch.int32)
    bad1 = (a1 != 0).repeat_interleave(T).cuda()
    o1 = _run(h, xb, betas, T, R0, T0, one, a1)
    ref = _run(h, xb, betas, T, R0, T0, SdfScene(scenes[0]))
    assert (o1["pene_count"][bad1] == -1).all() and torch.equal(o1["pene_count"][~bad1], ref["pene_count"][~bad1])


def test_set_creation_checks(scenes):
    from egogen_amd import _lib
    from egogen_amd.body_model import SdfSceneSet
    small = scene_gen.scene_sdf_dict(scene_gen.box_mesh((-1, -1, -0.05), (1, 1, 2)), None, res=32, center=(0, 0, 1), half=2.0)
    with pytest.raises(_lib.EgxError, match="scene 1"):
        SdfSceneSet([scenes[0], small])
    with pytest.raises(ValueError):
        SdfSceneSet([])


def _nets():
    from egogen_amd.models import GAMMAPrimitiveCombo, PREDICTOR_CFG, REGRESSOR_CFG, VPoserEncoder
    from tests.helpers import seeded_prior_state_dict, seeded_vposer_state_dict
    combo = GAMMAPrimitiveCombo(PREDICTOR_CFG, REGRESSOR_CFG)
    combo.load_state_dict(seeded_prior_state_dict())
    combo.cuda().eval()
    vp = VPoserEncoder()
    vp.load_state_dict(seeded_vposer_state_dict())
    vp.cuda().eval()
    return combo, vp


def _room_scenes(S, res=48):
    rng = np.random.default_rng(5)
    out = []
    for s in range(S):
        sc = synth.make_sdf_scene(res, seed=s + 1)
        pairs = np.zeros((64, 2, 3), np.float32)
        pairs[:, :, :2] = rng.uniform(-3.0, 3.0, (64, 2, 2))
        out.append(dict(sdf_dict=sc, rings=synth.sdf_scene_polygon(sc), pairs=pairs, name=f"room{s}"))
    return out


def test_env_over_a_set_matches_one_scene_envs(model):
    """An env over S scenes against S one-scene envs (same A, seeds, injected candidates, actions): the agents the set assigns to
    scene s match the one-scene env's same slots bit for bit - observations, reward, termination and counts - over steps and a
    reset; the graph replay of the set env equals its eager run.  (Both run the 32 x 64 wave tile: the set launch always does.)"""
    from egogen_amd import _lib
    from egogen_amd.crowd_env import VecCrowdEnv, block_scene_assignment
    bm, feet, h, _ = model
    lib = _lib.load()
    old_tile = int(lib.egx_lbs_get_wave_tile())
    _lib.check(lib.egx_lbs_set_wave_tile(2), "egx_lbs_set_wave_tile")
    try:
        combo, vp = _nets()
        A, S = 7, 3
        rooms = _room_scenes(S)
        blocks = block_scene_assignment(A, S)
        envs = {"set": VecCrowdEnv(A, h, combo, vp, sdf_scenes=rooms, seed=0),
                "graph": VecCrowdEnv(A, h, combo, vp, sdf_scenes=rooms, seed=0, use_graph=True)}
        for s in range(S):
            envs[s] = VecCrowdEnv(A, h, combo, vp, sdf_dict=rooms[s]["sdf_dict"], rings=rooms[s]["rings"], pairs=rooms[s]["pairs"], seed=0)
        st = envs["set"]
        assert st.scene_idx.cpu().numpy().tolist() == blocks.tolist() and st.scene_names == ["room0", "room1", "room2"]
        for s in range(S):   # each scene's accepted pairs are those of its one-scene env
            lo, n = int(st._vp_off[s]), int(st._vp_n[s])
            assert torch.equal(st.valid_pairs[lo:lo + n], envs[s].valid_pairs)

        def cands(rnd):
            """agent a's candidate: pair (a + rnd) of its own scene's accepted pairs; the one-scene env s gets the same for the agents
            of block s and pairs of scene s for the others"""
            out = {}
            per = [envs[s].valid_pairs for s in range(S)]
            out["set"] = out["graph"] = torch.stack([per[blocks[a]][(a + rnd) % len(per[blocks[a]])] for a in range(A)])
            for s in range(S):
                out[s] = torch.stack([per[s][(a + rnd) % len(per[s])] for a in range(A)])
            return out

        keys = ("state", "obs_ego", "obs_dist", "obs_time", "reward", "terminated", "R0", "T0", "wpath")
        g = torch.Generator().manual_seed(3)
        for rnd in range(2):   # reset, three steps; a second reset with new candidates, three steps
            c = cands(rnd)
            for k, e in envs.items():
                e.set_candidates(c[k].reshape(A, 1, 2, 3))
                e.reset()
            for it in range(3):
                z = torch.randn(A, 128, generator=g).cuda()
                for e in envs.values():
                    e.step(z, auto_reset=False)
                torch.cuda.synchronize()
                for s in range(S):
                    m = torch.as_tensor(blocks == s).cuda()
                    for k in keys:
                        assert torch.equal(getattr(st, k)[m], getattr(envs[s], k)[m]), (rnd, it, s, k)
                    assert torch.equal(st.pene_count.reshape(A, 20)[m], envs[s].pene_count.reshape(A, 20)[m]), (rnd, it, s)
                for k in keys:
                    assert torch.equal(getattr(envs["graph"], k), getattr(st, k)), ("graph", rnd, it, k)
                assert torch.equal(envs["graph"].pene_count, st.pene_count)
        assert int(st.pene_count.max()) > 0
    finally:
        _lib.check(lib.egx_lbs_set_wave_tile(old_tile), "egx_lbs_set_wave_tile")


def _read_scalars(logdir):
    tags = {}
    for dp, _, fns in os.walk(logdir):
        for fn in fns:
            if fn == "scalars.jsonl":
                import json
                for line in open(os.path.join(dp, fn)):
                    d = json.loads(line)
                    tags.setdefault(d["tag"], []).append(d["value"])
            elif fn.startswith("events.out.tfevents"):
                from tensorboard.backend.event_processing.event_accumulator import EventAccumulator
                ea = EventAccumulator(dp)
                ea.Reload()
                for t in ea.Tags()["scalars"]:
                    tags.setdefault(t, []).extend(e.value for e in ea.Scalars(t))
    return tags


def test_main_ppo_trains_across_a_scene_list(tmp_path):
    from egogen_amd import scene_gen
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rooms = _room_scenes(2, res=32)
    paths = []
    for r in rooms:
        p = tmp_path / f"{r['name']}.npz"
        scene = {"edges": synth.rings_to_edges(r["rings"]), "tris": np.zeros((0, 6), np.float32), "floor_height": 0.0,
                 "pairs": r["pairs"], "nav_v": np.zeros((0, 3), np.float32), "nav_f": np.zeros((0, 3), np.int32), "rings": r["rings"]}
        scene_gen.save_scene(str(p), scene, r["sdf_dict"])
        paths.append(str(p))
    env = dict(os.environ, PYTHONPATH=ROOT)
    common = ["--num-verts", "1024", "--scene", ",".join(paths)]
    cmd = [sys.executable, os.path.join(ROOT, "crowd_ppo", "main_ppo.py"), "--training-num", "8", "--test-num", "4", "--epoch", "1",
           "--step-per-epoch", "16", "--step-per-collect", "16", "--batch-size", "8", "--logdir", str(tmp_path / "log"),
           "--save-interval", "1"] + common
    r = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "Final reward:" in r.stdout
    run_dirs = [dp for dp, _, fn in os.walk(tmp_path / "log" / "collision-avoidance" / "ppo" / "0") if "checkpoint_1.pth" in fn]
    assert len(run_dirs) == 1 and os.path.exists(os.path.join(run_dirs[0], "policy.pth"))
    tags = _read_scalars(tmp_path / "log")
    for name in ("room0", "room1"):
        assert f"test/reward_{name}" in tags and f"test/length_{name}" in tags, sorted(tags)
    assert "test/reward" in tags
    # --watch: the rollout pickles name the scene of each episode
    cmd2 = [sys.executable, os.path.join(ROOT, "crowd_ppo", "main_ppo.py"), "--watch", "--resume-path",
            os.path.join(run_dirs[0], "checkpoint_1.pth"), "--test-num", "4", "--logdir", str(tmp_path / "log2")] + common
    r2 = subprocess.run(cmd2, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r2.returncode == 0, r2.stdout[-2000:] + r2.stderr[-4000:]
    pk = sorted((tmp_path / "log" / "eval_results").glob("motion_*.pkl"))
    assert pk, "no rollout pickles written"
    seen = {pickle.load(open(f, "rb"))["scene_path"] for f in pk}
    assert seen <= {"room0", "room1"} and seen
