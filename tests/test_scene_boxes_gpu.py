"""Random box scenes on the GPU: `egx_sdf_boxes` against the float64 closed form (`scene_gen.oriented_box_sdf`), composition onto a
base grid, the mesh path on the same boxes, argument checks, sampling of a device-built scene, an env over a generated set,
`VecCrowdEnv.replace_sdf_scenes`, and `main_ppo.py --scene-resample-every`."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from egogen_amd import scene_gen as sg
from egogen_amd import synth
from tests.helpers import level_set_band

pytestmark = pytest.mark.gpu

CENTER, HALF = (0.1, -0.2, 1.0), 4.0
ROOM = ((-3.7, -3.5, 0.0), (3.9, 3.6, 4.6))
YAWS = (0.0, 0.3, np.pi / 2, -2.0)
DIMS = [(20, 24, 36), (19, 23, 30)]   # non-cubic; rows of 36 (16-byte runs) and of 30 samples (d2 % 4 != 0); 17 280 and 13 110 samples:
#                                       no multiple of 256, more than one block of 256 runs


def _layout(K, seed=0):
    """K boxes anywhere in the room (they may overlap: the kernel takes the maximum), yaws cycling through YAWS."""
    rng = np.random.default_rng(seed + K)
    lay = np.zeros((K, 7))
    lay[:, 0:2] = rng.uniform(-3.0, 3.0, (K, 2))
    lay[:, 2:4] = rng.uniform(0.25, 0.75, (K, 2))
    lay[:, 4] = rng.uniform(0.0, 0.5, K) * (np.arange(K) % 3 == 2)       # every third box hangs above the floor
    lay[:, 5] = lay[:, 4] + rng.uniform(0.5, 1.5, K)
    lay[:, 6] = [YAWS[k % 4] for k in range(K)]
    return lay


def _points(dims, center=CENTER, half=HALF):
    ax = [center[a] + ((2 * np.arange(d) + 1) / d - 1.0) * half for a, d in enumerate(dims)]
    return np.stack(np.meshgrid(*ax, indexing="ij"), -1)


def _reference(dims, lay, start):
    """float64: max(start, max_k(-d_k))"""
    P = _points(dims)
    v = start.copy()
    for b in lay:
        v = np.maximum(v, -sg.oriented_box_sdf(P, b))
    return v


def _room_start(dims):
    return synth._box_sdf(_points(dims), np.asarray(ROOM[0], np.float64), np.asarray(ROOM[1], np.float64))


# fp32 against float64: u = 6e-8; the sample position, the translation and rotation into the box's frame and the norm work on
# coordinates <= 8 m -> about 5e-6 m, times two
TOL = 1e-5


@pytest.mark.parametrize("K", [0, 1, 3, 16])
@pytest.mark.parametrize("dims", DIMS)
def test_kernel_matches_the_closed_form(dims, K):
    lay = _layout(K)
    got = sg.sdf_boxes(lay, CENTER, 1.0 / HALF, dims, room=ROOM)
    assert got.is_cuda and tuple(got.shape) == dims and got.dtype == torch.float32
    got = got.cpu().numpy().astype(np.float64)
    ref = _reference(dims, lay, _room_start(dims))
    err = np.abs(got - ref).max()
    print(f"dims {dims} K {K}: max |delta| = {err:.3e}")
    assert err <= TOL
    far = np.abs(ref) >= TOL
    assert (np.sign(got[far]) == np.sign(ref[far])).all()
    if K:
        assert (ref > _room_start(dims) + 0.1).any() and (ref < 0).any()   # the boxes show, and free space is left


@pytest.mark.parametrize("dims", DIMS)
def test_composition_onto_a_base_grid(dims):
    lay = _layout(5, seed=3)
    g = torch.Generator().manual_seed(dims[0])
    base = (torch.randn(*dims, generator=g) * 0.5 - 0.3).cuda()
    keep = base.clone()
    out = sg.sdf_boxes(lay, CENTER, 1.0 / HALF, base=base)
    assert torch.equal(base, keep) and out.data_ptr() != base.data_ptr()
    ref = _reference(dims, lay, keep.cpu().numpy().astype(np.float64))
    got = out.cpu().numpy().astype(np.float64)
    err = np.abs(got - ref).max()
    print(f"dims {dims} composed: max |delta| = {err:.3e}")
    assert err <= TOL
    assert (got > keep.cpu().numpy()).mean() > 0.003 and (got == keep.cpu().numpy()).mean() > 0.3   # boxes won somewhere, base elsewhere
    assert torch.equal(sg.sdf_boxes(lay, CENTER, 1.0 / HALF, base=base), out)            # two runs
    inplace = base.clone()
    res = sg.sdf_boxes(lay, CENTER, 1.0 / HALF, base=inplace, out=inplace)
    assert res.data_ptr() == inplace.data_ptr() and torch.equal(inplace, out)             # out == base
    # a base grid wins over a room box given with it; no box: the base comes back
    assert torch.equal(sg.sdf_boxes(lay, CENTER, 1.0 / HALF, base=base, room=ROOM), out)
    assert torch.equal(sg.sdf_boxes(np.zeros((0, 7)), CENTER, 1.0 / HALF, base=base), base)
    # a view whose storage is not 16-byte aligned takes the scalar path: the same values
    pad = torch.zeros(base.numel() + 1, device="cuda")
    shifted = pad[1:].view(*dims)
    shifted.copy_(base)
    assert np.abs(sg.sdf_boxes(lay, CENTER, 1.0 / HALF, base=shifted, out=shifted).cpu().numpy() - ref).max() <= TOL


def _rotated_box_mesh(b):
    v, f = sg.box_mesh((-b[2], -b[3], b[4]), (b[2], b[3], b[5]))
    c, s = np.cos(b[6]), np.sin(b[6])
    w = v.copy()
    w[:, 0], w[:, 1] = b[0] + c * v[:, 0] - s * v[:, 1], b[1] + s * v[:, 0] + c * v[:, 1]
    return w, f


def test_free_space_agrees_with_the_mesh_path():
    """The same room and boxes as closed meshes through `scene_sdf_dict` (egx_mesh_sdf): where both grids are < 0 they hold the
    same distance (inside the solids the mesh path of the union and the maximum of the boxes differ by construction)."""
    lay = sg.random_box_layout(np.random.default_rng(11), 3, sg.ROOM_LO, sg.ROOM_HI)
    lay[:, 4] = [0.0, 0.3, 0.0]   # one box off the floor
    lay[:, 5] += lay[:, 4]
    res = 32
    got = sg.sdf_boxes(lay, sg.ROOM_CENTER, 1.0 / sg.ROOM_HALF, (res, res, res), room=(sg.ROOM_LO, sg.ROOM_HI))
    mesh = sg.scene_sdf_dict(sg.box_mesh(sg.ROOM_LO, sg.ROOM_HI), sg.merge_meshes([_rotated_box_mesh(b) for b in lay]), res=res,
                             center=sg.ROOM_CENTER, half=sg.ROOM_HALF)["sdf"]
    free = (got < 0) & (mesh < 0)
    assert int(free.sum()) > 0.3 * res ** 3
    d = (got - mesh)[free].abs().max().item()
    print(f"free space: max |delta| = {d:.3e}")
    assert d <= level_set_band()
    assert ((got < 0) == (mesh < 0))[(got.abs() > level_set_band()) & (mesh.abs() > level_set_band())].all()


def test_argument_errors():
    from egogen_amd import _lib
    ok = _layout(2)
    sg.sdf_boxes(ok, CENTER, 0.25, (8, 8, 8), room=ROOM)
    with pytest.raises(_lib.EgxError, match="num_boxes"):
        sg.sdf_boxes(_layout(17), CENTER, 0.25, (8, 8, 8), room=ROOM)
    with pytest.raises(_lib.EgxError, match="room"):
        sg.sdf_boxes(ok, CENTER, 0.25, (8, 8, 8))
    for dims in ((8, 8, 1), (0, 8, 8), (8, -1, 8)):
        with pytest.raises(_lib.EgxError):
            sg.sdf_boxes(ok, CENTER, 0.25, dims, room=ROOM)
    with pytest.raises(_lib.EgxError, match="scale"):
        sg.sdf_boxes(ok, CENTER, 0.0, (8, 8, 8), room=ROOM)
    bad = ok.copy()
    bad[1, 2] = 0.0
    with pytest.raises(_lib.EgxError, match="box"):
        sg.sdf_boxes(bad, CENTER, 0.25, (8, 8, 8), room=ROOM)
    with pytest.raises(_lib.EgxError, match="room"):
        sg.sdf_boxes(ok, CENTER, 0.25, (8, 8, 8), room=(ROOM[1], ROOM[0]))
    torch.cuda.synchronize()


def test_sampling_a_device_built_scene():
    """`calc_sdf` (egx_sdf_sample through the bricked copy) on a scene whose grid never left the device == the oracle's on the
    downloaded grid.  Both are fp32 trilinear sums of eight products of values <= 7 m: 10 u |v| = 4e-6."""
    from egogen_amd.body_model import SdfScene
    from egogen_amd.utils import calc_sdf
    from oracle.sdf import calc_sdf as oracle_calc_sdf
    sc = sg.box_layout_scene(sg.random_box_layout(np.random.default_rng(2), 3, sg.ROOM_LO, sg.ROOM_HI), res=30, n_pairs=16)
    assert sc["sdf_dict"]["sdf"].is_cuda and len(sc["rings"]) == 4 and sc["pairs"].shape == (16, 2, 3)
    g = torch.Generator().manual_seed(0)
    pts = torch.rand(3, 700, 3, generator=g) * torch.tensor([9.0, 9.0, 6.0]) - torch.tensor([4.5, 4.5, 0.5])   # some outside the cube
    got = calc_sdf(pts.cuda(), SdfScene(sc["sdf_dict"])).cpu()
    ref = oracle_calc_sdf(pts, {k: v.detach().cpu() for k, v in sc["sdf_dict"].items()})
    assert (got - ref).abs().max().item() <= 5e-6 and (ref < 0).any() and (ref > 0).any()


# ------------------------------------------------------------------------------------------------ envs over generated sets
@pytest.fixture(scope="module")
def world():
    from egogen_amd import _lib
    from egogen_amd.body_model import BodyModelHandle
    from egogen_amd.models import GAMMAPrimitiveCombo, PREDICTOR_CFG, REGRESSOR_CFG, VPoserEncoder
    from tests.helpers import seeded_prior_state_dict, seeded_vposer_state_dict
    V = 2048
    h = BodyModelHandle(synth.make_body_model(0, num_verts=V), synth.marker_ids(V), synth.feet_vids(V))
    combo = GAMMAPrimitiveCombo(PREDICTOR_CFG, REGRESSOR_CFG)
    combo.load_state_dict(seeded_prior_state_dict())
    vp = VPoserEncoder()
    vp.load_state_dict(seeded_vposer_state_dict())
    # set launches always run the 32 x 64 wave tile; the one-scene launches they are compared with bit for bit run it too
    lib = _lib.load()
    old = int(lib.egx_lbs_get_wave_tile())
    _lib.check(lib.egx_lbs_set_wave_tile(2), "egx_lbs_set_wave_tile")
    yield h, combo.cuda().eval(), vp.cuda().eval()
    _lib.check(lib.egx_lbs_set_wave_tile(old), "egx_lbs_set_wave_tile")


def test_generated_sets_are_a_function_of_seed_generation_and_scene_number():
    from egogen_amd import setup_world as sw
    a = sw.build_scene("boxes:3x2", sdf_res=32, seed=0)
    b = sw.build_scene("boxes:3x2", sdf_res=32, seed=0)
    assert a["scene_kind"] == "sdf" and len(a["sdf_scenes"]) == 3 and [s["name"] for s in a["sdf_scenes"]] == ["boxes0", "boxes1", "boxes2"]
    g1 = a["scene_factory"](1)
    for s in range(3):
        x, y = a["sdf_scenes"][s], b["sdf_scenes"][s]
        assert x["boxes"].shape == (2, 7) and np.array_equal(x["boxes"], y["boxes"]) and np.array_equal(x["pairs"], y["pairs"])
        assert torch.equal(x["sdf_dict"]["sdf"], y["sdf_dict"]["sdf"]) and x["sdf_dict"]["sdf"].is_cuda
        assert tuple(x["sdf_dict"]["sdf"].shape) == (32, 32, 32)
        assert not np.array_equal(g1[s]["boxes"], x["boxes"])
        assert np.array_equal(a["scene_factory"](0)[s]["boxes"], x["boxes"]) and np.array_equal(b["scene_factory"](1)[s]["boxes"], g1[s]["boxes"])
    assert not np.array_equal(a["sdf_scenes"][0]["boxes"], a["sdf_scenes"][1]["boxes"])
    assert not np.array_equal(sw.build_scene("boxes:3x2", sdf_res=32, seed=1)["sdf_scenes"][0]["boxes"], a["sdf_scenes"][0]["boxes"])
    # in a list with a fixed scene: the fixed entry is kept across generations, scene numbers count through the list
    m = sw.build_scene("single_box,boxes:2", sdf_res=32, seed=0)
    assert [s["name"] for s in m["sdf_scenes"]] == ["single_box", "boxes1", "boxes2"] and m["sdf_scenes"][1]["boxes"].shape == (1, 7)
    assert m["scene_factory"](3)[0] is m["sdf_scenes"][0]


def test_variants_of_a_prepared_scene(tmp_path):
    """`file.npz+boxes:SxK`: each variant is the file's grid with the boxes composed on (max), its raster with the footprints
    stamped out, and rings / pairs from that raster."""
    from egogen_amd import setup_world as sw
    res = 32
    base = synth.make_sdf_scene(res)
    free = np.ones((156, 156), bool)
    origin, cell = np.array([-3.9, -3.9]), 0.05
    rings = sg.grid_to_rings(free, origin, cell)
    scene = {"edges": synth.rings_to_edges(rings), "tris": np.zeros((0, 6), np.float32), "floor_height": 0.0,
             "pairs": sg.sample_pairs(rings, 256), "nav_v": np.zeros((0, 3), np.float32), "nav_f": np.zeros((0, 3), np.int32),
             "rings": rings, "free": free, "origin": origin, "cell": cell}
    p = str(tmp_path / "room.npz")
    sg.save_scene(p, scene, base)
    out = sw.build_scene(f"{p}+boxes:2x2", seed=3)
    assert len(out["sdf_scenes"]) == 2 and out["sdf_scenes"][0]["name"] == "room+boxes0"
    for s, sc in enumerate(out["sdf_scenes"]):
        lay = sc["boxes"]
        ref = _reference_for(base, lay)
        got = sc["sdf_dict"]["sdf"].cpu().numpy().astype(np.float64)
        assert np.abs(got - ref).max() <= TOL
        assert np.array_equal(sc["free"], sg.stamp_boxes(free, origin, cell, lay)) and sc["free"].sum() < free.sum()
        assert sc["pairs"].shape == (256, 2, 3)
        e = sc["pairs"].reshape(-1, 3).astype(np.float64)
        for b in lay:   # pairs lie on free cells: at least the body radius minus half a cell diagonal from every footprint
            assert (sg.footprint_distance(e[:, 0], e[:, 1], b) > 0.2 - cell).all()
    assert not np.array_equal(out["sdf_scenes"][0]["boxes"], out["sdf_scenes"][1]["boxes"])


def _reference_for(base, lay):
    res = base["sdf"].shape[0]
    P = _points((res, res, res), sg.ROOM_CENTER, sg.ROOM_HALF)
    v = base["sdf"].astype(np.float64)
    for b in lay:
        v = np.maximum(v, -sg.oriented_box_sdf(P, b))
    return v


KEYS = ("state", "obs_ego", "obs_dist", "obs_time", "reward", "terminated", "R0", "T0", "wpath")


def test_env_over_a_generated_set_matches_one_scene_envs(world):
    """An env over `boxes:3x2` against three one-scene envs over the same scenes (same A, seeds, injected candidates, actions):
    the agents of block s match the one-scene env's same slots bit for bit."""
    from egogen_amd import setup_world as sw
    from egogen_amd.crowd_env import VecCrowdEnv, block_scene_assignment
    h, combo, vp = world
    A, S = 7, 3
    rooms = sw.build_scene("boxes:3x2", sdf_res=32, seed=0)["sdf_scenes"]
    blocks = block_scene_assignment(A, S)
    st = VecCrowdEnv(A, h, combo, vp, sdf_scenes=rooms, seed=0)
    one = [VecCrowdEnv(A, h, combo, vp, sdf_dict=r["sdf_dict"], rings=r["rings"], pairs=r["pairs"], seed=0) for r in rooms]
    assert st.scene_names == ["boxes0", "boxes1", "boxes2"] and st.scene_generation == 0
    assert all(np.array_equal(b, r["boxes"]) for b, r in zip(st.scene_boxes, rooms))
    for s in range(S):
        lo, n = int(st._vp_off[s]), int(st._vp_n[s])
        assert n > 100 and torch.equal(st.valid_pairs[lo:lo + n], one[s].valid_pairs)
    per = [e.valid_pairs for e in one]
    g = torch.Generator().manual_seed(3)
    for rnd in range(2):
        st.set_candidates(torch.stack([per[blocks[a]][(a + rnd) % len(per[blocks[a]])] for a in range(A)]).reshape(A, 1, 2, 3))
        st.reset()
        for s in range(S):
            one[s].set_candidates(torch.stack([per[s][(a + rnd) % len(per[s])] for a in range(A)]).reshape(A, 1, 2, 3))
            one[s].reset()
        for it in range(3):
            z = torch.randn(A, 128, generator=g).cuda()
            for e in [st] + one:
                e.step(z, auto_reset=False)
            torch.cuda.synchronize()
            for s in range(S):
                m = torch.as_tensor(blocks == s).cuda()
                for k in KEYS:
                    assert torch.equal(getattr(st, k)[m], getattr(one[s], k)[m]), (rnd, it, s, k)
                assert torch.equal(st.pene_count.reshape(A, 20)[m], one[s].pene_count.reshape(A, 20)[m]), (rnd, it, s)


def _wpath_rows_are_accepted_pairs(env):
    """every agent's start (pelvis over it: x, y) and target are those of one accepted pair of ITS scene"""
    wp = env.wpath.cpu()
    for a in range(env.A):
        s = int(env.scene_idx[a])
        lo, n = int(env._vp_off[s]), int(env._vp_n[s])
        rows = env.valid_pairs[lo:lo + n].cpu()
        hit = ((rows[:, 1, :2] - wp[a, 1, :2]).abs().amax(1) < 1e-5) & ((rows[:, 0, :2] - wp[a, 0, :2]).abs().amax(1) < 1e-4)
        assert bool(hit.any()), (a, s)


@pytest.mark.parametrize("use_graph", [False, True])
def test_replace_sdf_scenes(world, use_graph):
    from egogen_amd import setup_world as sw
    from egogen_amd.body_model import SdfScene, SdfSceneSet
    from egogen_amd.crowd_env import VecCrowdEnv
    h, combo, vp = world
    A = 7
    scene = sw.build_scene("boxes:3x2", sdf_res=32, seed=0)
    env = VecCrowdEnv(A, h, combo, vp, sdf_scenes=scene["sdf_scenes"], seed=0, use_graph=use_graph)
    env.reset()
    g = torch.Generator().manual_seed(1)
    env.step(torch.randn(A, 128, generator=g).cuda())            # captures the graph over the old scenes, fills the candidate pool
    new = scene["scene_factory"](1)
    env.replace_sdf_scenes(new)
    assert env.scene_generation == 1 and env._graph is None and all(np.array_equal(b, d["boxes"]) for b, d in zip(env.scene_boxes, new))
    assert int(env.steps.max()) == 0
    for s in range(3):   # the pair tables are the new scenes'
        ref = VecCrowdEnv(A, h, combo, vp, sdf_dict=new[s]["sdf_dict"], rings=new[s]["rings"], pairs=new[s]["pairs"], seed=0)
        lo, n = int(env._vp_off[s]), int(env._vp_n[s])
        assert torch.equal(env.valid_pairs[lo:lo + n], ref.valid_pairs)
        ne = int(env.edge_off[s + 1]) - int(env.edge_off[s])
        assert torch.equal(env.edges[int(env.edge_off[s]):int(env.edge_off[s + 1])], ref.edges) and ne == 4 + 4 * 2
    _wpath_rows_are_accepted_pairs(env)
    R0, T0 = env.R0.clone(), env.T0.clone()
    env.step(torch.randn(A, 128, generator=g).cuda(), auto_reset=False)
    direct = h.forward(env.pred_params.reshape(A * 20, 93), env.betas, 20, want_verts=False,
                       sdf=SdfSceneSet([SdfScene(d["sdf_dict"]) for d in new]), R0=R0, T0=T0, agent_scene=env.scene_idx)
    torch.cuda.synchronize()
    assert torch.equal(env.pene_count, direct["pene_count"])
    old = SdfSceneSet([SdfScene(d["sdf_dict"]) for d in scene["sdf_scenes"]])
    stale = h.forward(env.pred_params.reshape(A * 20, 93), env.betas, 20, want_verts=False, sdf=old, R0=R0, T0=T0,
                      agent_scene=env.scene_idx)["pene_count"].clone()
    for _ in range(3):   # auto-resets draw from the new pool
        env.step(torch.randn(A, 128, generator=g).cuda())
    _wpath_rows_are_accepted_pairs(env)
    print("counts in the new / old scenes:", int(direct["pene_count"].sum()), int(stale.sum()))

    # a replacement one of whose rooms is one solid box: the constructor's error, and the env goes on with the scenes it had
    solid = sg.sdf_boxes(np.array([[0.0, 0.0, 3.9, 3.9, 0.0, 4.9, 0.0]]), sg.ROOM_CENTER, 1.0 / sg.ROOM_HALF, (32, 32, 32),
                         room=(sg.ROOM_LO, sg.ROOM_HI))
    assert float(solid.min()) >= 0
    gen2 = scene["scene_factory"](2)
    bad = [gen2[0], dict(gen2[1], sdf_dict=dict(gen2[1]["sdf_dict"], sdf=solid)), gen2[2]]
    keep = (env.sdf, env.valid_pairs, env.edges, env._sc)
    pairs_before = env.valid_pairs.clone()
    with pytest.raises(RuntimeError, match="no start/target pair of scene 'boxes1'"):
        env.replace_sdf_scenes(bad)
    assert env.scene_generation == 1 and all(a is b for a, b in zip((env.sdf, env.valid_pairs, env.edges, env._sc), keep))
    assert torch.equal(env.valid_pairs, pairs_before)
    R0, T0 = env.R0.clone(), env.T0.clone()
    env.step(torch.randn(A, 128, generator=g).cuda(), auto_reset=False)
    again = h.forward(env.pred_params.reshape(A * 20, 93), env.betas, 20, want_verts=False,
                      sdf=SdfSceneSet([SdfScene(d["sdf_dict"]) for d in new]), R0=R0, T0=T0, agent_scene=env.scene_idx)
    assert torch.equal(env.pene_count, again["pene_count"])
    with pytest.raises(ValueError, match="scenes"):
        env.replace_sdf_scenes(new[:2])
    with pytest.raises(ValueError, match="grid"):
        env.replace_sdf_scenes(sw.build_scene("boxes:3x2", sdf_res=16, seed=0)["sdf_scenes"])
    env.check_finite()


def test_main_ppo_resamples_the_training_scenes(tmp_path):
    from egogen_amd import setup_world as sw
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, os.path.join(ROOT, "crowd_ppo", "main_ppo.py"), "--training-num", "8", "--test-num", "4", "--epoch", "2",
           "--step-per-epoch", "16", "--step-per-collect", "16", "--batch-size", "8", "--logdir", str(tmp_path / "log"),
           "--save-interval", "1", "--num-verts", "1024", "--scene", "boxes:2x1", "--sdf-res", "32", "--scene-resample-every", "1"]
    r = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "Final reward:" in r.stdout and "Epoch #2" in r.stdout
    line = [l for l in r.stdout.splitlines() if l.startswith("Scene layouts: ")]
    assert len(line) == 1
    d = json.loads(line[0][len("Scene layouts: "):])
    sc = sw.build_scene("boxes:2x1", sdf_res=32, seed=0)
    gen0 = [np.round(s["boxes"], 6).tolist() for s in sc["sdf_scenes"]]
    gen1 = [np.round(s["boxes"], 6).tolist() for s in sc["scene_factory"](1)]
    assert d["train_generation"] == 1 and d["train_boxes"] == gen1 and gen1 != gen0
    assert d["test_generation"] == 0 and d["test_boxes"] == gen0
    # losses are finite: the update scalars of both epochs
    from tests.test_scene_set_gpu import _read_scalars
    tags = _read_scalars(tmp_path / "log")
    losses = [v for k, vs in tags.items() if k.startswith("update/") for v in vs]
    assert len(losses) >= 2 and np.isfinite(losses).all(), sorted(tags)
    assert "test/reward_boxes0" in tags and "test/reward_boxes1" in tags
