"""Random box scenes, host side (no GPU): the float64 closed form `scene_gen.oriented_box_sdf` that `egx_sdf_boxes` evaluates, the
layout sampler, the polygon and pairs of a layout, the `--scene` spec parser, the raster keys of scene files and the stamping
of boxes onto a prepared scene's raster."""
import numpy as np
import pytest

from egogen_amd import scene_gen as sg

BOX = np.array([0.7, -0.4, 0.6, 0.25, 0.0, 1.1, 0.3])   # cx, cy, half_x, half_y, z_lo, z_hi, yaw


def _to_world(local_xy, box):
    c, s = np.cos(box[6]), np.sin(box[6])
    l = np.asarray(local_xy, np.float64)
    return np.stack([box[0] + c * l[..., 0] - s * l[..., 1], box[1] + s * l[..., 0] + c * l[..., 1]], -1)


def test_closed_form_values():
    hx, hy, z0, z1 = BOX[2], BOX[3], BOX[4], BOX[5]
    zc = (z0 + z1) / 2
    # zero on the six faces (face centres and off-centre points of each face)
    faces = [((hx, 0.1), zc), ((-hx, -0.2), zc + 0.3), ((0.3, hy), zc), ((-0.5, -hy), zc - 0.4), ((0.2, 0.1), z0), ((-0.3, -0.1), z1)]
    for loc, z in faces:
        p = np.append(_to_world(loc, BOX), z)
        assert abs(sg.oriented_box_sdf(p, BOX)) < 1e-15
    # the centre: minus the smallest half extent
    assert sg.oriented_box_sdf(np.array([BOX[0], BOX[1], zc]), BOX) == pytest.approx(-min(hx, hy, (z1 - z0) / 2), abs=1e-15)
    # off a corner: the distance to the corner
    p = np.append(_to_world((hx + 0.3, hy + 0.4), BOX), z1 + 1.2)
    assert sg.oriented_box_sdf(p, BOX) == pytest.approx(np.sqrt(0.3 ** 2 + 0.4 ** 2 + 1.2 ** 2), abs=1e-14)
    # off an edge, off a face
    assert sg.oriented_box_sdf(np.append(_to_world((hx + 0.3, 0.0), BOX), z1 + 0.4), BOX) == pytest.approx(0.5, abs=1e-14)
    assert sg.oriented_box_sdf(np.append(_to_world((0.1, -hy - 0.7), BOX), zc), BOX) == pytest.approx(0.7, abs=1e-14)
    # yaw 0 is the axis-aligned box of synth._box_sdf
    from egogen_amd import synth
    rng = np.random.default_rng(0)
    P = rng.uniform(-3, 3, (500, 3))
    b0 = BOX.copy()
    b0[6] = 0.0
    lo, hi = np.array([b0[0] - hx, b0[1] - hy, z0]), np.array([b0[0] + hx, b0[1] + hy, z1])
    assert np.abs(sg.oriented_box_sdf(P, b0) - synth._box_sdf(P, lo, hi)).max() < 1e-14


def test_closed_form_is_invariant_under_a_common_rotation():
    rng = np.random.default_rng(1)
    P = rng.uniform(-1.5, 1.5, (4, 50, 3)) + np.array([BOX[0], BOX[1], 0.5])
    d = sg.oriented_box_sdf(P, BOX)
    assert d.shape == (4, 50) and (d < 0).any() and (d > 0).any()
    for a in (0.4, -2.0, np.pi / 2):
        c, s = np.cos(a), np.sin(a)
        Q = P.copy()
        Q[..., 0], Q[..., 1] = c * P[..., 0] - s * P[..., 1], s * P[..., 0] + c * P[..., 1]
        b = BOX.copy()
        b[0], b[1], b[6] = c * BOX[0] - s * BOX[1], s * BOX[0] + c * BOX[1], BOX[6] + a
        assert np.abs(sg.oriented_box_sdf(Q, b) - d).max() < 1e-13
    # the footprint distance is the z-inside case
    inside_z = P.copy()
    inside_z[..., 2] = 0.5
    fd = sg.footprint_distance(P[..., 0], P[..., 1], BOX)
    far = fd > 0
    assert np.abs(fd[far] - sg.oriented_box_sdf(inside_z, BOX)[far]).max() < 1e-14


def _check_layout(lay, lo, hi, wall_margin=0.6, gap=0.8, size=(0.5, 1.5), height=(0.5, 1.5)):
    r = np.hypot(lay[:, 2], lay[:, 3])
    assert (lay[:, 0] - r >= lo[0] + wall_margin - 1e-12).all() and (lay[:, 0] + r <= hi[0] - wall_margin + 1e-12).all()
    assert (lay[:, 1] - r >= lo[1] + wall_margin - 1e-12).all() and (lay[:, 1] + r <= hi[1] - wall_margin + 1e-12).all()
    for i in range(len(lay)):
        for j in range(i):
            assert np.linalg.norm(lay[i, :2] - lay[j, :2]) >= r[i] + r[j] + gap - 1e-12
    assert (2 * lay[:, 2:4] >= size[0]).all() and (2 * lay[:, 2:4] <= size[1]).all()
    assert (lay[:, 4] == 0).all() and (lay[:, 5] >= height[0]).all() and (lay[:, 5] <= height[1]).all()
    assert (np.abs(lay[:, 6]) <= np.pi).all()


def test_layout_sampler():
    a = sg.random_box_layout(np.random.default_rng(7), 3, sg.ROOM_LO, sg.ROOM_HI)
    b = sg.random_box_layout(np.random.default_rng(7), 3, sg.ROOM_LO, sg.ROOM_HI)
    c = sg.random_box_layout(np.random.default_rng(8), 3, sg.ROOM_LO, sg.ROOM_HI)
    assert a.shape == (3, 7) and a.dtype == np.float64 and np.array_equal(a, b) and not np.array_equal(a, c)
    yaws = []
    for seed in range(200):
        lay = sg.random_box_layout(np.random.default_rng(seed), 4, sg.ROOM_LO, sg.ROOM_HI)
        _check_layout(lay, sg.ROOM_LO, sg.ROOM_HI)
        yaws.append(lay[:, 6])
    assert np.std(np.concatenate(yaws)) > 1.0
    lay = sg.random_box_layout(np.random.default_rng(0), 2, (0, 0, 0), (6, 5, 3), yaw=False, wall_margin=0.3, gap=0.5)
    _check_layout(lay, (0, 0), (6, 5), 0.3, 0.5)
    assert (lay[:, 6] == 0).all()
    for seed in range(5):
        with pytest.raises(ValueError, match="random_box_layout"):
            sg.random_box_layout(np.random.default_rng(seed), 12, sg.ROOM_LO, sg.ROOM_HI)
    with pytest.raises(ValueError):   # a room too small for any box
        sg.random_box_layout(np.random.default_rng(0), 1, (0, 0, 0), (1.5, 1.5, 3), max_tries=50)


def test_rings_and_pairs_of_a_layout():
    lay = sg.random_box_layout(np.random.default_rng(3), 3, sg.ROOM_LO, sg.ROOM_HI)
    rings = sg.box_layout_rings(lay, sg.ROOM_LO, sg.ROOM_HI)
    assert len(rings) == 4
    area = lambda r: 0.5 * np.sum(r[:-1, 0] * r[1:, 1] - r[1:, 0] * r[:-1, 1])
    assert area(rings[0]) == pytest.approx(7.8 * 7.8)                    # the room, counter-clockwise
    for r, b in zip(rings[1:], lay):
        assert np.array_equal(r[0], r[-1]) and area(r) == pytest.approx(-4 * b[2] * b[3])   # a hole, clockwise
    rng = np.random.default_rng(0)
    P = rng.uniform(-3.85, 3.85, (4000, 2))
    d = np.min([sg.footprint_distance(P[:, 0], P[:, 1], b) for b in lay], 0)
    inside = sg.rings_contain(rings, P[:, 0], P[:, 1])
    assert (d < -1e-9).sum() > 20 and not inside[d < -1e-9].any() and inside[d > 1e-9].all()
    assert not sg.rings_contain(rings, np.array([4.2]), np.array([0.0]))[0]
    pairs = sg.sample_clear_pairs(lay, sg.ROOM_LO, sg.ROOM_HI, 512, clearance=0.5, seed=4)
    assert pairs.shape == (512, 2, 3) and pairs.dtype == np.float32 and (pairs[..., 2] == 0).all()
    assert (np.linalg.norm(pairs[:, 0] - pairs[:, 1], axis=1) >= 1.7 - 1e-6).all()
    e = pairs.reshape(-1, 3).astype(np.float64)
    for b in lay:
        assert (sg.footprint_distance(e[:, 0], e[:, 1], b) >= 0.5 - 1e-6).all()
    assert (np.abs(e[:, :2]) <= 3.9 - 0.5 + 1e-6).all()
    assert np.array_equal(pairs, sg.sample_clear_pairs(lay, sg.ROOM_LO, sg.ROOM_HI, 512, clearance=0.5, seed=4))
    solid = np.array([[0.0, 0.0, 3.9, 3.9, 0.0, 4.9, 0.0]])              # a box that fills the room leaves no pair
    with pytest.raises(ValueError, match="pairs"):
        sg.sample_clear_pairs(solid, sg.ROOM_LO, sg.ROOM_HI, 8)


def test_spec_parsing():
    from egogen_amd import setup_world as sw
    assert sw.parse_box_spec("boxes:5") == {"base": None, "scenes": 5, "boxes": 1}
    assert sw.parse_box_spec("boxes:64x3") == {"base": None, "scenes": 64, "boxes": 3}
    assert sw.parse_box_spec("scans/room.npz+boxes:2x4") == {"base": "scans/room.npz", "scenes": 2, "boxes": 4}
    assert sw.parse_box_spec("a+b.npz+boxes:2") == {"base": "a+b.npz", "scenes": 2, "boxes": 1}
    for other in ("room0", "single_box", "box", "scans/room.npz", "boxes.npz", "boxes"):
        assert sw.parse_box_spec(other) is None
    for bad in ("boxes:", "boxes:0", "boxes:3x0", "boxes:3x5", "boxes:x2", "boxes:2x", "boxes:2x2x2", "boxes:-1", "boxes:1.5",
                "boxes: 3", "room0+boxes:2", "scans/+boxes:2", "+boxes:2"):
        with pytest.raises(ValueError, match="scene entry"):
            sw.parse_box_spec(bad)
    # inside a comma list the entries come through as they are
    assert sw.scene_entries("single_box,boxes:2x2") == ["single_box", "boxes:2x2"]
    with pytest.raises(ValueError, match="scene entry"):
        sw.build_scene("single_box,boxes:2x9", sdf_res=16)


def _raster_scene(with_raster=True):
    rng = np.random.default_rng(5)
    free = np.ones((60, 50), bool)
    free[:3] = False
    origin, cell = np.array([-1.5, -1.25]), 0.05
    rings = sg.grid_to_rings(free, origin, cell)
    scene = {"edges": np.zeros((4, 4), np.float32), "tris": np.zeros((2, 6), np.float32), "floor_height": 0.0,
             "pairs": rng.uniform(-1, 1, (16, 2, 3)).astype(np.float32), "nav_v": np.zeros((4, 3), np.float32),
             "nav_f": np.zeros((2, 3), np.int32), "rings": rings}
    if with_raster:
        scene.update(free=free, origin=origin, cell=cell)
    sd = {"sdf": rng.standard_normal((8, 8, 8)).astype(np.float32), "center": np.array([0, 0, 1], np.float32), "scale": np.float32(0.5)}
    return scene, sd


def test_raster_keys_in_scene_files(tmp_path):
    from egogen_amd import setup_world as sw
    scene, sd = _raster_scene()
    p = str(tmp_path / "with.npz")
    sg.save_scene(p, scene, sd)
    plain = sw.load_scene_file(p)
    assert set(plain) == {"scene_kind", "sdf_dict", "rings", "pairs"}          # what VecCrowdEnv takes, as before
    got = sw.load_scene_file(p, raster=True)
    assert np.array_equal(got["free"], scene["free"]) and got["free"].dtype == bool
    assert np.array_equal(got["origin"], scene["origin"]) and got["cell"] == scene["cell"] and got["floor_height"] == 0.0
    assert np.array_equal(got["sdf_dict"]["sdf"], sd["sdf"]) and np.array_equal(got["pairs"], scene["pairs"])
    # a file without the raster: every other key as before, and the named error when boxes are asked for
    bare, _ = _raster_scene(with_raster=False)
    q = str(tmp_path / "without.npz")
    sg.save_scene(q, bare, sd)
    with np.load(q) as z:
        assert not {"free", "origin", "cell"} & set(z.files)
    with np.load(p) as z:
        assert {"free", "origin", "cell"} <= set(z.files)
    assert "free" not in sw.load_scene_file(q, raster=True)
    with pytest.raises(ValueError, match="prepare_scene"):
        sw.build_scene(f"{q}+boxes:2x1")
    with pytest.raises(ValueError, match="add_boxes_to_scene"):
        sg.add_boxes_to_scene(dict(bare, sdf_dict=sd), BOX[None])


def test_stamping_removes_the_cells_of_the_inflated_footprints():
    rng = np.random.default_rng(2)
    free = rng.uniform(size=(80, 64)) > 0.1
    origin, cell, radius = np.array([-2.0, -1.6]), 0.05, 0.2
    lay = np.array([[0.3, 0.2, 0.5, 0.3, 0.0, 1.0, 0.6], [-1.2, -0.9, 0.25, 0.4, 0.0, 0.7, -2.0]])
    out = sg.stamp_boxes(free, origin, cell, lay, radius)
    assert out.shape == free.shape and out.dtype == bool and free.sum() > out.sum()
    # the float64 rule, cell by cell: blocked iff the centre is within `radius` of a footprint (corners rounded)
    expect = free.copy()
    for i in range(free.shape[0]):
        for j in range(free.shape[1]):
            x, y = origin[0] + (i + 0.5) * cell, origin[1] + (j + 0.5) * cell
            for b in lay:
                c, s = np.cos(b[6]), np.sin(b[6])
                lx, ly = c * (x - b[0]) + s * (y - b[1]), -s * (x - b[0]) + c * (y - b[1])
                qx, qy = abs(lx) - b[2], abs(ly) - b[3]
                d = np.hypot(max(qx, 0.0), max(qy, 0.0)) + min(max(qx, qy), 0.0)
                if d <= radius:
                    expect[i, j] = False
    assert np.array_equal(out, expect)
    assert np.array_equal(sg.stamp_boxes(free, origin, cell, np.zeros((0, 7)), radius), free)   # no box: unchanged


def test_trainer_takes_an_epoch_hook():
    import inspect
    from egogen_amd.trainer import onpolicy_trainer
    assert inspect.signature(onpolicy_trainer).parameters["epoch_begin_fn"].default is None


def test_resample_flag_needs_generated_scenes():
    from crowd_ppo import main_ppo
    from egogen_amd import setup_world as sw
    assert sw.scene_spec_generates("boxes:4x2") and sw.scene_spec_generates("single_box,scan.npz+boxes:2")
    assert not sw.scene_spec_generates("single_box") and not sw.scene_spec_generates("room0,single_box")
    assert main_ppo.get_args([]).scene_resample_every == 0
    for scene in ("single_box", "room0,single_box"):
        with pytest.raises(SystemExit, match="generates nothing"):
            main_ppo.main(main_ppo.get_args(["--scene", scene, "--scene-resample-every", "2"]))
    with pytest.raises(SystemExit, match="scene-resample-every"):
        main_ppo.main(main_ppo.get_args(["--scene", "boxes:2", "--scene-resample-every", "-1"]))
