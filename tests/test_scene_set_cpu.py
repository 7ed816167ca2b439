"""CPU-side checks of SDF scene sets (no GPU): the argument checks of egx_sdf_scene_set_create (every descriptor here carries NULL
device pointers - all checks run before the first device access, so a rejected set touches nothing), the `--scene` list parsing
of setup_world.build_scene and the block assignment of agents to scenes."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from egogen_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib


def _grid(d):
    g = _lib().SdfGrid()
    g.grid = None
    g.d0, g.d1, g.d2 = d
    g.center[0], g.center[1], g.center[2] = 0.0, 0.0, 1.0
    g.scale = 0.25
    g.coarse_minmax = None
    return g


def _create(grids):
    L = _lib()
    lib = L.load()
    arr = (L.SdfGrid * len(grids))(*grids)
    h = C.c_void_p()
    rc = lib.egx_sdf_scene_set_create(arr, len(grids), C.byref(h))
    return rc, lib.egx_last_error().decode(), h


def test_mismatched_dimensions_are_rejected_and_named():
    rc, msg, h = _create([_grid((48, 48, 48)), _grid((48, 48, 48)), _grid((48, 48, 40))])
    assert rc == -1 and not h.value
    assert "scene 2" in msg and "48x48x40" in msg


def test_scene_without_grid_or_bracket_table_is_rejected():
    rc, msg, h = _create([_grid((32, 32, 32)), _grid((32, 32, 32))])
    assert rc == -1 and not h.value and "scene 0" in msg and "egx_sdf_build_coarse" in msg


def test_empty_set_is_rejected():
    L = _lib()
    h = C.c_void_p()
    assert L.load().egx_sdf_scene_set_create(None, 0, C.byref(h)) == -1
    assert L.load().egx_sdf_scene_set_size(None) == 0
    from egogen_amd.body_model import SdfSceneSet
    with pytest.raises(ValueError):
        SdfSceneSet([])


def test_block_assignment():
    from egogen_amd.crowd_env import block_scene_assignment
    a = block_scene_assignment(10, 3)
    assert a.dtype == np.int32 and a.tolist() == [0, 0, 0, 0, 1, 1, 1, 2, 2, 2]
    assert block_scene_assignment(512, 4).tolist() == [s for s in range(4) for _ in range(128)]
    assert block_scene_assignment(5, 5).tolist() == [0, 1, 2, 3, 4]
    assert block_scene_assignment(7, 1).tolist() == [0] * 7
    b = block_scene_assignment(1000, 7)
    counts = np.bincount(b)
    assert counts.max() - counts.min() <= 1 and (np.diff(b) >= 0).all()
    with pytest.raises(ValueError):
        block_scene_assignment(3, 4)
    with pytest.raises(ValueError):
        block_scene_assignment(3, 0)


def _write_scene(path, res, shift, sdf=True):
    from egogen_amd import scene_gen
    rng = np.random.default_rng(int(shift * 10) + res)
    ring = np.array([[-2, -2], [2, -2], [2, 2], [-2, 2]], np.float32) + shift
    scene = {"edges": np.zeros((4, 4), np.float32), "tris": np.zeros((2, 6), np.float32), "floor_height": 0.0,
             "pairs": rng.uniform(-1, 1, (16, 2, 3)).astype(np.float32), "nav_v": np.zeros((4, 3), np.float32),
             "nav_f": np.zeros((2, 3), np.int32), "rings": [ring]}
    sd = {"sdf": rng.standard_normal((res, res, res)).astype(np.float32), "center": np.array([shift, 0, 1], np.float32),
          "scale": np.float32(0.25)} if sdf else None
    scene_gen.save_scene(str(path), scene, sd)


def test_scene_list_parsing(tmp_path):
    from egogen_amd import setup_world as sw
    d = tmp_path / "scans"
    d.mkdir()
    _write_scene(d / "b_room.npz", 16, 1.0)
    _write_scene(d / "a_room.npz", 16, 2.0)
    (d / "notes.txt").write_text("not a scene")
    _write_scene(tmp_path / "c.npz", 16, 3.0)
    # directory expansion, sorted by name, after the explicit entries in list order
    assert sw.scene_entries(f"{tmp_path / 'c.npz'},{d}") == [str(tmp_path / "c.npz"), str(d / "a_room.npz"), str(d / "b_room.npz")]
    sc = sw.build_scene(f"{tmp_path / 'c.npz'},{d}")
    assert sc["scene_kind"] == "sdf" and [s["name"] for s in sc["sdf_scenes"]] == ["c", "a_room", "b_room"]
    one = sw.build_scene(str(d / "a_room.npz"))
    assert np.array_equal(sc["sdf_scenes"][1]["pairs"], one["pairs"])
    assert np.array_equal(sc["sdf_scenes"][1]["sdf_dict"]["sdf"], one["sdf_dict"]["sdf"])
    # a set of one (a directory with one scene) is today's single-scene dict
    d1 = tmp_path / "single"
    d1.mkdir()
    _write_scene(d1 / "only.npz", 16, 1.5)
    a, b = sw.build_scene(str(d1)), sw.build_scene(str(d1 / "only.npz"))
    assert set(a) == set(b) == {"scene_kind", "sdf_dict", "rings", "pairs"}
    assert np.array_equal(a["pairs"], b["pairs"]) and np.array_equal(a["sdf_dict"]["sdf"], b["sdf_dict"]["sdf"])
    # built-in names are allowed entries
    mixed = sw.build_scene(f"single_box,single_box", sdf_res=16)
    assert len(mixed["sdf_scenes"]) == 2
    # mismatched grid dimensions: the error names the entry
    _write_scene(tmp_path / "big.npz", 24, 0.0)
    with pytest.raises(ValueError, match="big.npz"):
        sw.build_scene(f"{tmp_path / 'c.npz'},{tmp_path / 'big.npz'}")
    # a box-kind scene in a list
    _write_scene(tmp_path / "boxes.npz", 16, 0.0, sdf=False)
    with pytest.raises(ValueError, match="boxes.npz"):
        sw.build_scene(f"{tmp_path / 'c.npz'},{tmp_path / 'boxes.npz'}")
    with pytest.raises(ValueError):
        sw.build_scene(f"{tmp_path / 'c.npz'},")


def test_header_documents_the_set_entries():
    txt = open(os.path.join(ROOT, "include", "egogen_hip.h")).read()
    for name in ("egx_sdf_scene_set_create", "egx_sdf_scene_set_destroy", "egx_sdf_scene_set_size", "egx_lbs_forward_scenes"):
        assert name + "(" in txt
    assert "out_pene_count = -1" in txt
