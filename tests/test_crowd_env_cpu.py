"""The table builders of egogen_amd/crowd_env.py: pure numpy / ctypes, checked without a device."""
import numpy as np
import pytest
import torch

from egogen_amd import crowd_env as ce


def _cfg(**kw):
    return dict(ce.BOX_CFG, weight_pene=0.37, **kw)


@pytest.mark.parametrize("kind,finetuning,weight_pene,terminate,code", [
    ("sdf", False, 1.0, 0, 0), ("sdf", True, 0.1, 1, 0), ("box", False, 0.37, 1, 1), ("box", True, 0.37, 1, 1),
    ("crowd", False, 0.37, 0, 2), ("crowd", True, 0.37, 0, 2)])
def test_env_config_rules_per_scene_kind(kind, finetuning, weight_pene, terminate, code):
    ec = ce.env_config(kind, _cfg(), finetuning)
    assert ec.weight_pene == np.float32(weight_pene) and ec.terminate_on_penetration == terminate and ec.scene_kind == code
    assert ec.max_depth == 11 and ec.weight_look_target == np.float32(0.1) and ec.ray_len == 7.0
    assert ec.pene_type_body == 1 and ec.vp_thresh == 11.0 and ec.no_goal_termination == 0


def test_env_config_filters_and_copied_weights():
    ec = ce.env_config("crowd", _cfg(pene_type="foot"), vp_thresh=14, goal_terminates=False)
    assert ec.pene_type_body == 0 and ec.vp_thresh == 14.0 and ec.no_goal_termination == 1
    c = ce.DEFAULT_CFG
    ec = ce.env_config("sdf", c)
    for name in ("reproj_factor", "goal_thresh", "pene_thres", "weight_skate", "weight_floor", "weight_face_target", "weight_look_target",
                 "weight_success", "weight_target_dist", "weight_vp"):
        assert getattr(ec, name) == np.float32(c[name]), name
    assert ec.max_depth == 13
    with pytest.raises(KeyError):
        ce.env_config("mesh", c)


def test_fill_rejects_a_name_that_is_no_field():
    from egogen_amd import _lib
    with pytest.raises(AttributeError):
        _lib.fill(_lib.EnvConfig(), weight_penetration=1.0)
    assert _lib.fill(_lib.EnvState(), state=None, seed=torch.zeros(3)).state is None


def test_scene_tables_offsets_and_placeholders():
    rng = np.random.default_rng(0)
    edges = [rng.random((n, 4)).astype(np.float32) for n in (4, 12, 7)]
    tris = [rng.random((n, 6)).astype(np.float32) for n in (0, 10, 2)]
    t = ce.scene_tables(edges, tris, [0.0, 0.25, -1.0])
    assert t["edge_off"].tolist() == [0, 4, 16, 23] and t["tri_off"].tolist() == [0, 0, 10, 12]
    assert t["edge_off"].dtype == np.int32 and t["tri_off"].dtype == np.int32
    for s in range(3):
        assert np.array_equal(t["edges"][t["edge_off"][s]:t["edge_off"][s + 1]], edges[s])
        assert np.array_equal(t["tris"][t["tri_off"][s]:t["tri_off"][s + 1]], tris[s])
    assert t["floor_h"].tolist() == [0.0, 0.25, -1.0] and t["floor_h"].dtype == np.float32
    for empty in (ce.scene_tables(edges, [np.zeros((0, 6), np.float32)] * 3, [0.0] * 3), ce.scene_tables(edges)):
        assert empty["tris"].shape == (1, 6) and not empty["tris"].any() and empty["tri_off"].tolist() == [0, 0, 0, 0]
        assert empty["floor_h"].tolist() == [0.0, 0.0, 0.0]


def test_crowd_scene_lists():
    A = 3
    bbox, pairs = torch.zeros(4, A, 4), np.arange(A * 6, dtype=np.float64).reshape(A, 2, 3)
    sl = ce.crowd_scene_lists(A, bbox, pairs)
    assert (sl.K, sl.R) == (1, 1) and len(sl.edges) == 1 and sl.edges[0].shape == (1, 4) and not sl.edges[0].any()
    assert sl.pairs.shape == (A, 1, 2, 3) and sl.pairs.dtype == np.float32 and np.array_equal(sl.pairs[:, 0], pairs)
    t = ce.scene_tables(sl.edges, sl.tris, sl.floor)
    assert t["edge_off"].tolist() == [0, 1] and t["tris"].shape == (1, 6) and t["tri_off"].tolist() == [0, 0]
    square = [np.array([[0, 0], [2, 0], [2, 2], [0, 2], [0, 0]], np.float64)]
    ring = ce.crowd_scene_lists(A, bbox, pairs, square)
    assert np.array_equal(ring.edges[0], ce.synth.rings_to_edges(square).astype(np.float32)) and len(ring.edges[0]) == 4
    for bad in (dict(crowd_bbox=None, crowd_pairs=pairs), dict(crowd_bbox=bbox, crowd_pairs=None),
                dict(crowd_bbox=torch.zeros(4, A + 1, 4), crowd_pairs=pairs), dict(crowd_bbox=torch.zeros(4, A, 3), crowd_pairs=pairs)):
        with pytest.raises(ValueError, match=r"crowd scene kind needs crowd_bbox\[G,A,4\] and crowd_pairs\[A,2,3\]"):
            ce.crowd_scene_lists(A, **bad)


def test_box_and_sdf_argument_checks():
    with pytest.raises(ValueError, match="box scene kind needs box_scenes"):
        ce.box_scene_lists([])
    mk = lambda n, e: dict(edges=np.ones((e, 4)), tris=np.ones((2, 3, 2)), floor_height=0.5, pairs=np.ones((n, 2, 3)))
    sl = ce.box_scene_lists([mk(5, 4), mk(3, 8)])
    assert (sl.K, sl.R) == (8, 4) and sl.pairs.shape == (2, 3, 2, 3) and sl.floor == [0.5, 0.5]      # the shortest pair list
    assert [e.shape for e in sl.edges] == [(4, 4), (8, 4)] and [t.shape for t in sl.tris] == [(2, 6), (2, 6)]
    assert ce.box_scene_lists([mk(5, 4)], 2, 3)[4:] == (2, 3)
    with pytest.raises(ValueError, match="sdf scene needs sdf_dict, rings"):
        ce.sdf_scene_args(sdf_dict={}, rings=[])
    with pytest.raises(ValueError, match="pass either sdf_dict / rings / pairs or sdf_scenes, not both"):
        ce.sdf_scene_args(rings=[], sdf_scenes=[{}])
    one = ce.sdf_scene_args({"sdf": 1}, ["r"], "p")
    assert one == [dict(sdf_dict={"sdf": 1}, rings=["r"], pairs="p", name="scene")]
    assert ce.sdf_scene_args(sdf_scenes=({"a": 1}, {"a": 2})) == [{"a": 1}, {"a": 2}]


def _rodrigues(aa):
    th = np.linalg.norm(aa)
    k = aa / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def test_seed_table_inputs():
    rng = np.random.default_rng(1)
    ms = {"poses": rng.normal(size=(9, 66)) * 0.5, "trans": rng.normal(size=(9, 3))}
    pose, glorot, transl = ce.seed_table_inputs(ms, [5])
    assert pose.shape == (1, 2, 63) and glorot.shape == (1, 2, 3, 3) and transl.shape == (1, 2, 3)
    for f in range(2):
        assert np.array_equal(pose[0, f], ms["poses"][5 + f, 3:66]) and np.array_equal(transl[0, f], ms["trans"][5 + f])
        assert np.allclose(glorot[0, f], _rodrigues(ms["poses"][5 + f, :3]), rtol=0, atol=1e-14)
        assert np.allclose(glorot[0, f] @ glorot[0, f].T, np.eye(3), atol=1e-14)
    starts = list(range(8))
    pose, glorot, transl = ce.seed_table_inputs(ms, starts)
    assert np.array_equal(pose[:, 1], ms["poses"][1:9, 3:66]) and np.array_equal(transl[:, 0], ms["trans"][:8])
    seeds = [{"poses": rng.normal(size=(2, 66)).astype(np.float32), "trans": rng.normal(size=(2, 3)).astype(np.float32)} for _ in range(3)]
    pose, glorot, transl = ce.seed_table_inputs(ms, [0, 1, 2], seeds)
    for v, d in enumerate(seeds):
        assert np.array_equal(pose[v], d["poses"][:, 3:66].astype(np.float64)) and np.array_equal(transl[v], d["trans"].astype(np.float64))
        assert np.allclose(glorot[v, 1], _rodrigues(d["poses"][1, :3].astype(np.float64)), rtol=0, atol=1e-14)
    zero = ce.seed_table_inputs({"poses": np.zeros((2, 66)), "trans": np.zeros((2, 3))}, [0])[1]
    assert np.array_equal(zero[0, 0], np.eye(3))


def test_round_major_layout_and_range_check():
    A, K, R = 3, 4, 2
    flat = torch.arange(A * R * K * 6, dtype=torch.float32).reshape(A, R * K, 2, 3)
    rm = ce.round_major(flat, A, K, R, (2, 3))
    assert rm.shape == (R, A, K, 2, 3)
    for a in range(A):
        for j in range(R * K):
            assert torch.equal(rm[j // K, a, j % K], flat[a, j])
    assert ce.round_major(flat[:, :K], A, K, R, (2, 3)).shape == (1, A, K, 2, 3)          # fewer rounds than R
    assert torch.equal(ce.round_major(torch.arange(A * K), A, K, R)[0], torch.arange(A * K).reshape(A, K))
    for n in (K - 1, K + 1, 3 * K):
        with pytest.raises(ValueError, match=f"candidates per agent must be a multiple of K={K} up to {R * K}, got {n}"):
            ce.round_major(torch.zeros(A, n, 2, 3), A, K, R, (2, 3))
