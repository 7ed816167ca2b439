"""CPU checks of the geodesic field: properties of the restatement (tests/geodesic_ref.py) that the GPU tests compare the device
against, and the host logic of egogen_amd/geodesic.py that runs before a device is needed (`seed_cells`, the argument checks of
`GeodesicField.from_raster`)."""
import numpy as np
import pytest

from tests import geodesic_ref as gref


def test_seed_cells_match_the_restatement():
    from egogen_amd.geodesic import seed_cells
    rng = np.random.default_rng(0)
    free = rng.random((23, 31)) > 0.3
    origin, cell = np.array([-1.3, 0.7]), 0.05
    centre = lambda i, j: origin + (np.array([i, j]) + 0.5) * cell
    goals = [origin + rng.random(2) * np.array([23, 31]) * cell for _ in range(40)]
    goals.append(centre(10, 12) + 0.5 * cell)                         # between four cells
    goals += [centre(0, 0), centre(22, 30), origin - 0.9 * cell, origin + np.array([23.4, 31.4]) * cell]    # corners, just outside
    hit = 0
    for g in goals:
        c, v = seed_cells(free, origin, cell, g)
        rc, rv = gref.seeds(free, origin, cell, g)
        order, rorder = np.argsort(c), np.argsort(rc)
        assert np.array_equal(c[order], rc[rorder]) and np.array_equal(v[order], rv[rorder]), g
        assert v.dtype == np.float32 and (len(c) == 0 or (free.reshape(-1)[c].all() and v.max() <= np.float32(1.5 * cell)))
        hit += len(c) > 0
    assert hit > 30


def test_seed_cells_special_goals():
    from egogen_amd.geodesic import seed_cells
    free = np.ones((9, 9), bool)
    origin, cell = np.zeros(2), 0.1
    # between four cells: the four at half a diagonal; the next eight are sqrt(2.5) = 1.58 cells away, outside
    c, v = seed_cells(free, origin, cell, [0.4, 0.4])
    assert sorted(c.tolist()) == [3 * 9 + 3, 3 * 9 + 4, 4 * 9 + 3, 4 * 9 + 4] and np.isclose(v, 0.05 * np.sqrt(2)).all()
    # on a cell centre: the cell at 0, four at 1 cell, four at sqrt(2) cells
    c, v = seed_cells(free, origin, cell, [0.45, 0.45])
    assert len(c) == 9 and np.sort(v)[0] < 1e-7 and np.isclose(np.sort(v)[1:5], 0.1).all() and np.isclose(np.sort(v)[5:], 0.1 * np.sqrt(2)).all()
    # on a blocked cell with one free neighbour
    free[:] = False
    free[4, 5] = True
    c, v = seed_cells(free, origin, cell, [0.45, 0.45])
    assert c.tolist() == [4 * 9 + 5] and np.isclose(v, 0.1).all()
    # nothing free within 1.5 cells
    c, v = seed_cells(free, origin, cell, [0.45, 0.25])
    assert len(c) == 0 and len(v) == 0
    c, v = seed_cells(free, origin, cell, [40.0, -40.0])
    assert len(c) == 0


def test_open_raster_is_within_the_eight_neighbour_bound():
    """All-free 41 x 57, cell 0.05, goal off-centre in a cell: e - 1e-6 <= d <= 1.0824 e + cell for every cell (an 8-neighbour path
    is at most 1 / cos 22.5 deg longer than the straight line; the seeds carry their Euclidean distance)."""
    H, W, cell = 41, 57, 0.05
    origin, goal = np.array([0.3, -0.2]), np.array([0.3 + 13.3 * cell, -0.2 + 40.8 * cell])
    d = gref.field(np.ones((H, W), bool), origin, cell, goal)
    I, J = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    e = np.sqrt((origin[0] + (I + 0.5) * cell - goal[0]) ** 2 + (origin[1] + (J + 0.5) * cell - goal[1]) ** 2)
    assert np.isfinite(d).all()
    assert (d >= e - 1e-6).all(), float((e - d).max())
    assert (d <= 1.0824 * e + cell).all(), float((d - 1.0824 * e).max() / cell)
    assert float((d / np.maximum(e, 1e-9))[e > 1.0].max()) > 1.07          # the anisotropy is really there


def test_float32_field_is_close_to_float64():
    free = gref.sealed_pocket(gref.serpentine(37, 53), 4, 20)
    origin, cell, goal = np.zeros(2), 0.05, np.array([0.05 * 2.4, 0.05 * 2.7])
    d32, hops = gref.field(free, origin, cell, goal, np.float32, hops=True)
    d64 = gref.field(free, origin, cell, goal, np.float64)
    fin = np.isfinite(d64)
    assert np.array_equal(fin, np.isfinite(d32)) and fin.sum() > 1000
    # n = cells on the path (the seed included): n - 1 float32 additions, each within 2^-24 relative of a running sum that never
    # exceeds the result; seed values and edge weights are the same float32 numbers in both runs
    bound = hops[fin] * 2.0 ** -24 * d64[fin]
    assert (np.abs(d32[fin].astype(np.float64) - d64[fin]) <= bound).all()
    assert d64[fin].max() > 4 * np.hypot(37, 53) * cell * 0.9                # the path is several times the straight line


def test_sealed_pocket_is_unreachable():
    free = gref.sealed_pocket(np.ones((12, 14), bool), 6, 8)
    d = gref.field(free, np.zeros(2), 0.1, np.array([0.25, 0.25]))
    assert np.isinf(d[6, 8]) and np.isinf(d[~free]).all()
    assert np.isfinite(d[free]).sum() == free.sum() - 1


def test_no_diagonal_through_a_corner():
    """Two blocked cells that touch at a corner, on a two-row raster: the only link between the two sides would be the diagonal
    between them."""
    free = np.ones((2, 6), bool)
    free[0, 3], free[1, 2] = False, False
    d = gref.field(free, np.zeros(2), 0.1, np.array([0.05, 0.05]))
    assert np.isfinite(d[:, :2]).all() and np.isfinite(d[0, 2])
    assert np.isinf(d[1, 3]) and np.isinf(d[:, 4:]).all()
    free[1, 2] = True                                                          # one of them freed: the diagonal past the other stays shut
    d = gref.field(free, np.zeros(2), 0.1, np.array([0.05, 0.05]))
    assert np.isfinite(d[free]).all()
    assert np.isclose(d[1, 3], d[1, 2] + 0.1) and d[1, 3] > d[0, 2] + 0.1 * 1.4


def test_from_raster_argument_errors_need_no_device():
    from egogen_amd.geodesic import GeodesicField
    free = np.ones((6, 7), bool)
    free[:, 5:] = False
    ok_goal = [[0.25, 0.25, 0.9]]
    bad = lambda **kw: GeodesicField.from_raster(**{**dict(free=free, origin=[0.0, 0.0], cell=0.1, goals=ok_goal, device="cuda"), **kw})
    with pytest.raises(ValueError, match="goal 0 .*no seed"):
        bad(goals=[[0.3, 0.68, 0.9]])                                         # two cells into the blocked part
    with pytest.raises(ValueError, match="goal 1 .*no seed"):
        bad(goals=[[0.25, 0.25], [5.0, 5.0]])                                  # off the raster
    with pytest.raises(ValueError, match="goal 0 is not finite"):
        bad(goals=[[np.nan, 0.3, 0.9]])
    with pytest.raises(ValueError, match="goals must be"):
        bad(goals=[0.25, 0.25, 0.9])
    with pytest.raises(ValueError, match="free must be"):
        bad(free=np.ones(5, bool))
    with pytest.raises(ValueError, match="origin must be"):
        bad(origin=[0.0, 0.0, 0.0])
    with pytest.raises(ValueError, match="origin must be"):
        bad(free=np.stack([free, free]), origin=np.zeros((3, 2)), scene_index=[0])
    with pytest.raises(ValueError, match="scene_index must lie"):
        bad(free=np.stack([free, free]), scene_index=[2])
    with pytest.raises(ValueError, match="scene_index must lie"):
        bad(scene_index=[-1])
    with pytest.raises(ValueError, match="scene_index must hold"):
        bad(scene_index=[0, 0])
    with pytest.raises(ValueError, match="need scene_index"):
        bad(free=np.stack([free, free]), goals=[[0.25, 0.25], [0.3, 0.3], [0.2, 0.2]])
    with pytest.raises(ValueError, match="cell must be"):
        bad(cell=0.0)
    with pytest.raises(ValueError, match="no walkable raster"):
        GeodesicField.from_scene({"scene_kind": "box"}, ok_goal)


def test_package_exports_the_class():
    import egogen_amd
    from egogen_amd.geodesic import GeodesicField
    assert egogen_amd.GeodesicField is GeodesicField
