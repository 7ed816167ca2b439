"""Scene preparation from scanned meshes on the GPU: `egx_scan_sdf` against the closed-mesh kernel and the float64 CPU check on
an open synthetic scan, `egx_walkable_raster` against `walkable_grid` and the CPU check, and a prepared scan driving the
environment."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from egogen_amd import scene_gen as sg
from tests import scan_check as sc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rot(axis, ang):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K


def _octahedron(c, r, R):
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], float) * r
    f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])
    return v @ R.T + np.asarray(c), f


def _sphere(c, r, levels):
    v, f = _octahedron([0, 0, 0], 1.0, np.eye(3))
    for _ in range(levels):
        nv, nf, mid = list(map(tuple, v)), [], {}
        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                mid[k] = len(nv)
                nv.append(tuple((np.asarray(nv[a]) + np.asarray(nv[b])) / 2))
            return mid[k]
        for a, b, cc in f:
            ab, bc, ca = m(a, b), m(b, cc), m(cc, a)
            nf += [[a, ab, ca], [ab, b, bc], [ca, bc, cc], [ab, bc, ca]]
        v, f = np.asarray(nv), np.asarray(nf)
    v = v / np.linalg.norm(v, axis=1, keepdims=True)
    return v * r + np.asarray(c), f


@pytest.mark.parametrize("case", ["octahedra", "spheres"])
def test_closed_mesh_gives_the_grid_of_the_closed_mesh_kernel(case):
    if case == "octahedra":
        mesh = sg.merge_meshes([_octahedron([0.4, -0.3, 1.1], 1.3, _rot([1, 2, 3], 0.7)),
                                _octahedron([-1.9, 1.6, 0.2], 0.7, _rot([3, -1, 2], 1.9))])
        res, center, half = 28, [0.1, 0.0, 0.9], 3.0
    else:                                                                  # 4 096 triangles
        mesh = sg.merge_meshes([_sphere([0.3, 0.2, 1.0], 1.5, 4), _sphere([-2.1, -1.9, -0.4], 0.8, 4)])
        res, center, half = 64, [0.0, 0.0, 0.9], 3.3
    a = sg.scan_to_sdf_dict(*mesh, res=res, center=center, half=half)["sdf"].cpu().numpy()
    b = sg.mesh_to_sdf_dict(*mesh, res=res, center=center, half=half)["sdf"].cpu().numpy()
    assert np.abs(np.abs(a) - np.abs(b)).max() < 2e-6 * half
    far = np.abs(b) > 1e-5
    assert (np.sign(a[far]) == np.sign(b[far])).all()
    assert (b > 0).sum() > 100 and (b < 0).sum() > 100


def test_open_scan_against_the_cpu_check():
    from oracle.mesh_sdf import sample_positions
    v, f = sc.synthetic_room()
    assert 4000 < len(f) < 6000
    res, center, half = 32, [0.013, -0.021, 1.17], 3.6
    got = sg.scan_to_sdf_dict(v, f, res=res, center=center, half=half)["sdf"].cpu().numpy().reshape(-1).astype(np.float64)
    p = sample_positions(center, 1 / half, res).reshape(-1, 3)
    ref = sc.unsigned_distance(v, f, p)
    assert np.abs(np.abs(got) - ref).max() < 2e-6 * half
    cell = 2 * half / res
    to_open = sc.distance_to_segments(sc.boundary_edges(v, f), p)
    judged = (ref > cell) & (to_open > ref + 1e-6)                       # nearest point not on an open boundary
    label = sc.analytic_positive(p)
    assert judged.sum() > 10000 and label[judged].sum() > 1000 and (~label[judged]).sum() > 1000
    assert np.array_equal(got[judged] > 0, label[judged])
    # the closed-mesh kernel's ray parity gets the space behind the single-sided walls wrong
    old = sg.mesh_to_sdf_dict(v, f, res=res, center=center, half=half)["sdf"].cpu().numpy().reshape(-1)
    wrong = (old[judged] > 0) != label[judged]
    assert wrong.sum() > 100


def test_large_scan():
    v, f = sc.synthetic_room(spacing=0.0125)
    assert len(f) >= 1_000_000
    center, half = [0.013, -0.021, 1.17], 3.6
    a = sg.scan_to_sdf_dict(v, f, res=64, center=center, half=half)["sdf"]
    b = sg.mesh_to_sdf_dict(v, f, res=64, center=center, half=half)["sdf"]
    assert float((a.abs() - b.abs()).abs().max()) < 2e-6 * half
    del a, b
    res = 256
    g = sg.scan_to_sdf_dict(v, f, res=res, center=center, half=half)["sdf"]
    h = 2 * half / res
    lin = torch.tensor(center, dtype=torch.float64).reshape(3, 1) + ((2 * torch.arange(res, dtype=torch.float64) + 1) / res - 1) * half
    inx = (lin[0].abs() < sc.ROOM_X - 2 * h).cuda()
    iny = (lin[1].abs() < sc.ROOM_Y - 2 * h).cuda()
    inz = ((lin[2] > 2 * h) & (lin[2] < sc.WALL_H - 2 * h)).cuda()
    box = inx[:, None, None] & iny[None, :, None] & inz[None, None, :]
    for ax in range(3):
        d = g.diff(dim=ax).abs() / h
        sl = [slice(None)] * 3
        sl[ax] = slice(0, res - 1)
        lo = box[tuple(sl)]
        sl[ax] = slice(1, res)
        both = lo & box[tuple(sl)]
        assert float(d[both].max()) <= 1.0 + 1e-3, ax
    assert float((g[box] > 0).float().mean()) < 0.05 and float((g[box] < 0).float().mean()) > 0.9


def test_raster_equals_walkable_grid_on_boxes():
    rng = np.random.default_rng(4)
    floor = sc._grid([-4, -4, 0], [8, 0, 0], [0, 8, 0], 8, 8, rng, 0.0)
    boxes = []
    for c, s, z, ang in (([-1.3, 0.9], [0.7, 0.4], (0.0, 0.8), 0.37), ([1.1, -1.2], [0.5, 0.9], (0.3, 1.5), 1.1),
                         ([0.7, 1.6], [0.3, 0.3], (1.0, 3.0), 2.3), ([-1.7, -1.9], [0.6, 0.2], (2.5, 3.0), 0.8)):
        bv, bf = sg.box_mesh([-s[0], -s[1], z[0]], [s[0], s[1], z[1]])
        boxes.append((bv @ _rot([0, 0, 1], ang).T + [c[0], c[1], 0.0], bf))
    obs = sg.merge_meshes(boxes)
    ref, o_ref, _ = sg.walkable_grid([-3, -3], [3, 3], *obs, radius=0.2, cell=0.05)
    v, f = sg.merge_meshes([floor, obs])
    got, o, cell, fh = sg.scan_walkable_grid(v, f, radius=0.2, cell=0.05, floor_height=0.0, bounds=((-3, -3), (3, 3)))
    assert got.shape == ref.shape == (120, 120) and np.allclose(o, o_ref) and fh == 0.0
    assert np.array_equal(got, ref)
    assert 0.5 < got.mean() < 0.95


def test_raster_of_the_open_scan_against_the_cpu_check():
    v, f = sc.synthetic_room()
    radius, cell = 0.2, 0.05
    sup, clr, origin, cell, fh = sg.scan_walkable_raster(v, f, radius=radius, cell=cell)
    assert abs(fh) < 1e-9                                                  # detected floor
    ref_sup, ref_clr = sc.walkable_raster(v, f, origin, cell, sup.shape, reach=radius + 0.05)
    assert np.array_equal(sup, ref_sup)
    judged = np.abs(ref_clr - radius) > 1e-5
    assert np.array_equal((clr > radius)[judged], (ref_clr > radius)[judged]) and judged.mean() > 0.99
    free, origin2, _, _ = sg.scan_walkable_grid(v, f, radius=radius, cell=cell)
    ref_free = sc.brute_disc_erosion(ref_sup, radius, cell) & (ref_clr > radius)
    assert np.array_equal(free[judged], ref_free[judged]) and np.allclose(origin, origin2)

    def at(x0, x1, y0, y1):
        return (slice(int(np.ceil((x0 - origin[0]) / cell - 0.5)), int(np.floor((x1 - origin[0]) / cell - 0.5)) + 1),
                slice(int(np.ceil((y0 - origin[1]) / cell - 0.5)), int(np.floor((y1 - origin[1]) / cell - 0.5)) + 1))

    def cells(x0, x1, y0, y1):
        return free[at(x0, x1, y0, y1)]
    for (lo, hi) in sc.HOLES:                                              # no support in the holes, nothing free there
        s = at(lo[0], hi[0], lo[1], hi[1])
        assert free[s].size > 20 and not free[s].any() and not sup[s].any()
    assert not cells(-2.2, -1.6, sc.BOARD_Y[0], sc.BOARD_Y[1]).any()       # under the board's low end
    assert cells(-1.1, -0.5, -1.4, -1.0).all()                             # under its high end (above the slab)
    assert free.mean() > 0.4


def test_prepared_scan_drives_the_env(tmp_path):
    from egogen_amd import setup_world as sw
    from egogen_amd.body_model import BodyModelHandle, SdfScene
    from egogen_amd.crowd_env import VecCrowdEnv
    from oracle.sdf import penetration_counts
    from oracle.smplx_lbs import BodyModel, smplx_forward
    from tests.helpers import build_world
    v, f = sc.synthetic_room()
    v = v + [0.0, 0.0, 0.3]                                                # floor at 0.3: detected and shifted away
    scene = sg.scene_from_scan(v, f, res=48, cell=0.1, radius=0.2, n_pairs=64, seed=2)
    assert abs(scene["z_offset"] - 0.3) < 1e-6
    path = str(tmp_path / "scan_scene.npz")
    sg.save_scene(path, scene, scene["sdf_dict"])
    loaded = sw.build_scene(path)
    assert loaded["scene_kind"] == "sdf"
    # every start and target lies in a free cell of the raster
    pts = loaded["pairs"].reshape(-1, 3)
    ij = np.floor((pts[:, :2] - scene["origin"]) / scene["cell"]).astype(int)
    assert scene["free"][ij[:, 0], ij[:, 1]].all()
    w = build_world(V=1536, A=6, scene_kind="sdf", sdf_res=48)
    env = VecCrowdEnv(6, w["handle"], w["env"].prior, w["env"].vposer, seed=0, **loaded)
    g = torch.Generator().manual_seed(1)
    env.reset()
    for _ in range(2):
        o, r, t = env.step(torch.randn(6, 128, generator=g).cuda(), auto_reset=False)
        assert torch.isfinite(r).all() and torch.isfinite(o["state"]).all()
    # penetration counts on the produced grid: kernel against the CPU oracle, bodies around the table
    h = BodyModelHandle(w["bm"], w["mk"], w["feet"])
    xb = torch.randn(12, 93, generator=g) * 0.2
    xb[:, 0] = torch.linspace(0.3, 2.0, 12)
    xb[:, 1] = 0.9
    xb[:, 2] += 1.0
    betas = torch.randn(3, 10, generator=g)
    out = h.forward(xb.cuda(), betas.cuda(), 4, want_verts=True, sdf=SdfScene(scene["sdf_dict"]))
    vb, _ = smplx_forward(BodyModel(w["bm"]), xb, betas.repeat_interleave(4, 0))
    sd = {k: scene["sdf_dict"][k].cpu() for k in ("sdf", "center", "scale")}
    cnt = penetration_counts(vb, sd, torch.as_tensor(w["feet"]).long())
    assert int((out["pene_count"].cpu().long() - cnt).abs().max()) <= 2
    assert int(cnt.sum()) > 0
    # the command line, in a child process
    out_npz = str(tmp_path / "cli.npz")
    sg.write_ply(str(tmp_path / "scan.ply"), v, f)
    r = subprocess.run([sys.executable, "-m", "egogen_amd.prepare_scene", "--mesh", str(tmp_path / "scan.ply"), "--out", out_npz,
                        "--scene-dir", str(tmp_path / "scene_dir"), "--res", "32", "--cell", "0.1", "--pairs", "32"],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "floor height 0.3" in r.stdout
    assert sw.build_scene(out_npz)["scene_kind"] == "sdf"
    from egogen_amd import egobody
    nv, nf = egobody.read_ply(str(tmp_path / "scene_dir" / "navmesh_tight.ply"))
    assert len(nf) > 0 and np.allclose(nv[:, 2], 0.0)
    mv, mf = egobody.read_ply(str(tmp_path / "scene_dir" / "mesh_floor_zup.ply"))
    assert np.allclose(mv, v - [0, 0, 0.3], atol=1e-5) and np.array_equal(mf, f)
