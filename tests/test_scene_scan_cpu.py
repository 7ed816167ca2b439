"""Scene preparation from scanned meshes, host side: welding, pseudo-normals, the BVH builder, floor detection, disc erosion,
the navmesh PLY that prepare_scene writes, and the numpy path of egobody.read_ply.  No device needed."""
import struct

import numpy as np
import pytest

from egogen_amd import egobody, scene_gen as sg
from tests import scan_check as sc


def _open_cube():
    """Unit cube without its top face (z = 1), outward normals, every face with its own four vertices."""
    v, f = sg.box_mesh([0, 0, 0], [1, 1, 1])
    quads = [f[2 * q:2 * q + 2] for q in range(6)]
    top = [q for q in range(6) if np.all(v[np.unique(quads[q])][:, 2] == 1)]
    parts = [(v[np.unique(quads[q])], np.searchsorted(np.unique(quads[q]), quads[q])) for q in range(6) if q not in top]
    return sg.merge_meshes(parts)


def _find(v, f, pts):
    """(triangle, slot) pairs where the feature of those positions (1 point: vertex, 2: edge) sits."""
    out = []
    for t, tri in enumerate(f):
        p = v[tri]
        hit = [next((k for k in range(3) if np.array_equal(p[k], q)), None) for q in pts]
        if None in hit:
            continue
        if len(pts) == 1:
            out.append((t, 4 + hit[0]))
        else:
            a, b = sorted(hit)
            out.append((t, 1 + {(0, 1): 0, (1, 2): 1, (0, 2): 2}[(a, b)]))
    return out


def test_weld_and_pseudo_normals_of_an_open_cube():
    v, f = _open_cube()
    assert len(v) == 20 and len(f) == 10
    u, wf = sg.weld_vertices(v, f)
    assert len(u) == 8 and np.array_equal(u[wf], v[f])
    pn = sg.pseudo_normals(v, f)
    fn = pn[:, 0]
    assert np.allclose(np.linalg.norm(fn, axis=1), 1)
    assert np.allclose((fn * (v[f].mean(1) - 0.5)).sum(1) > 0, True)     # outward
    # edge between the bottom (-z) and the y = 0 side: the sum of both faces' normals, seen from both triangles
    hits = _find(v, f, [np.array([0.0, 0, 0]), np.array([1.0, 0, 0])])
    assert len(hits) == 2
    for t, s in hits:
        assert np.allclose(pn[t, s], [0, -1, -1])
    # open boundary (top rim of the y = 0 side): the single face's normal
    hits = _find(v, f, [np.array([0.0, 0, 1]), np.array([1.0, 0, 1])])
    assert len(hits) == 1 and np.allclose(pn[hits[0]], [0, -1, 0])
    # the diagonal inside a face: twice its normal
    for t, s in [(t, s) for t in range(10) for s in (1, 2, 3)]:
        a, b = [(0, 1), (1, 2), (2, 0)][s - 1]
        pa, pb = v[f[t, a]], v[f[t, b]]
        if np.count_nonzero(pa != pb) == 2:
            assert np.allclose(pn[t, s], 2 * fn[t])
    # vertices: angle-weighted (pi/2 per incident face); a rim corner has two faces
    for t, s in _find(v, f, [np.array([0.0, 0, 0])]):
        assert np.allclose(pn[t, s], np.pi / 2 * np.array([-1, -1, -1]))
    for t, s in _find(v, f, [np.array([1.0, 1, 1])]):
        assert np.allclose(pn[t, s], np.pi / 2 * np.array([1, 1, 0]))
    assert np.allclose(sg.pseudo_normals(v, f, flip_normals=True), -pn)


def test_degenerate_triangles_decide_no_sign():
    v, f = _open_cube()
    f2 = np.concatenate([f, [[0, 0, 1], [0, 1, 1]]], 0)
    v2 = np.concatenate([v, [[2.0, 0, 0], [3.0, 0, 0], [4.0, 0, 0]]], 0)
    f2 = np.concatenate([f2, [[20, 21, 22]]], 0)                         # collinear
    deg = sg.degenerate_faces(v2, f2)
    assert not deg[:10].any() and deg[10:].all()
    pn = sg.pseudo_normals(v2, f2)
    assert np.allclose(pn[:10], sg.pseudo_normals(v, f)) and not pn[10:, 0].any()
    tb = sg.scan_sdf_tables(v2, f2)
    assert tb["tris"].shape == (13, 12) and tb["pn"].shape == (13, 21)
    assert int(tb["tris"][:, 3].sum()) == 3


@pytest.mark.parametrize("F,leaf", [(1, 4), (5, 4), (1000, 4), (4097, 8)])
def test_bvh_invariants(F, leaf):
    rng = np.random.default_rng(F)
    c = rng.uniform(-3, 3, (F, 1, 3))
    tri = c + rng.normal(0, 0.1, (F, 3, 3))
    tri[:3] = tri[:3, :1]                                                 # some zero-area triangles
    nodes, order, L = sg.build_bvh(tri, leaf)
    assert np.array_equal(np.sort(order), np.arange(F))                   # every triangle in exactly one leaf
    assert (leaf << L) >= F and (L == 0 or (leaf << (L - 1)) < F) and L <= 24
    assert nodes.shape == (2 ** (L + 1) - 1, 8)
    t32 = tri.astype(np.float32)[order]
    lo, hi = nodes[:, 0:3], nodes[:, 4:7]
    first = 2 ** L - 1
    for k in range(2 ** L):
        ts = t32[k * leaf:(k + 1) * leaf]
        if len(ts):
            assert (lo[first + k] <= ts.min((0, 1))).all() and (hi[first + k] >= ts.max((0, 1))).all()
        else:
            assert np.isinf(lo[first + k]).all()
    for h in range(1, 2 ** L):
        for ch in (2 * h, 2 * h + 1):
            ok = np.isinf(lo[ch - 1]).all() or ((lo[h - 1] <= lo[ch - 1]).all() and (hi[h - 1] >= hi[ch - 1]).all())
            assert ok
    with pytest.raises(ValueError):
        sg.build_bvh(tri, 1, max_levels=max(L - 1, 0)) if F > 1 else sg.build_bvh(np.zeros((0, 3, 3)))


def test_floor_detection_with_platform_and_table():
    floor = sg.box_mesh([-3, -2, 0.1], [3, 2, 0.3])                       # top at 0.3
    platform = sg.box_mesh([1, 0, 0.3], [2.5, 1.8, 0.5])                   # raised platform at 0.5
    table = sg.box_mesh([-1, -1, 1.0], [0, 0, 1.05])                       # table top at 1.05
    v, f = sg.merge_meshes([floor, platform, table])
    fine = sc._grid([-3, -2, 0.3], [6, 0, 0], [0, 4, 0], 30, 20, np.random.default_rng(0), 0.3)
    v2, f2 = sg.merge_meshes([fine, platform, table])
    for vv, ff in ((v, f), (v2, f2)):
        assert abs(sg.detect_floor_height(vv, ff) - 0.3) < 1e-9
    assert abs(sg.detect_floor_height(v + [0, 0, -1.7], f) + 1.4) < 1e-9


@pytest.mark.parametrize("radius,cell", [(0.2, 0.05), (0.23, 0.05), (0.1, 0.02), (0.05, 0.05)])
def test_disc_erosion_is_exact(radius, cell):
    rng = np.random.default_rng(int(radius * 1000))
    mask = rng.random((23, 19)) > 0.08
    mask[5:9, 3:12] = False
    assert np.array_equal(sg.disc_erosion(mask, radius, cell), sc.brute_disc_erosion(mask, radius, cell))


def test_navmesh_ply_round_trip(tmp_path):
    """The conforming navmesh prepare_scene writes: navmesh_walkable_rings(read_ply(...)) is the region of grid_to_rings."""
    x, y = np.meshgrid(np.arange(60), np.arange(44), indexing="ij")
    occ = ((x - 20) ** 2 + (y - 15) ** 2 < 30) | ((x > 35) & (x < 44) & (y > 20) & (y < 30)) | (x < 2) | (y > 40)
    free = sg.disc_erosion(~occ, 0.12, 0.05)
    free[50:55, 2:6] = True
    free[51:54, 6] = False
    origin, cell = np.array([-1.3, 0.7]), 0.05
    v, f = sg.grid_to_cell_navmesh(free, origin, cell, 0.0)
    sg.write_ply(str(tmp_path / "navmesh_tight.ply"), v, f)
    rings = egobody.navmesh_walkable_rings(*egobody.read_ply(str(tmp_path / "navmesh_tight.ply")))
    ref = sg.grid_to_rings(free, origin, cell)
    area = lambda rs: sum(abs(egobody._ring_area(r)) * (1 if k == 0 else -1) for k, r in enumerate(rs))
    assert abs(area(rings) - area(ref)) < 1e-6
    rng = np.random.default_rng(0)
    p = rng.uniform(origin, origin + np.array(free.shape) * cell, (4000, 2))
    assert np.array_equal(sg.rings_contain(rings, p[:, 0], p[:, 1]), sg.rings_contain(ref, p[:, 0], p[:, 1]))


def _write_ply_with_extras(path, v, f, quads=()):
    n = np.cross(v[f[0, 1]] - v[f[0, 0]], v[f[0, 2]] - v[f[0, 0]])
    hdr = (f"ply\nformat binary_little_endian 1.0\nelement vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\n"
           f"property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n"
           f"element face {len(f) + len(quads)}\nproperty list uchar int vertex_indices\nend_header\n")
    with open(path, "wb") as fh:
        fh.write(hdr.encode())
        for k, p in enumerate(v):
            fh.write(struct.pack("<ffffffBBB", *p, *n, k % 256, (3 * k) % 256, 7))
        for t in f:
            fh.write(struct.pack("<Biii", 3, *map(int, t)))
        for q in quads:
            fh.write(struct.pack("<Biiii", 4, *map(int, q)))


def test_read_ply_fast_path_equals_the_row_loop(tmp_path, monkeypatch):
    v, f = sc.synthetic_room()
    v = v.astype(np.float32).astype(np.float64)
    fast_calls = []
    real = egobody._read_binary_triangles
    monkeypatch.setattr(egobody, "_read_binary_triangles", lambda *a: fast_calls.append(1) or real(*a))
    for name, quads in (("tri.ply", ()), ("quad.ply", [(0, 1, 2, 3)])):
        path = str(tmp_path / name)
        _write_ply_with_extras(path, v, f, quads)
        got = egobody.read_ply(path)
        with monkeypatch.context() as m:
            m.setattr(egobody, "_read_binary_triangles", lambda *a: None)
            ref = egobody.read_ply(path)
        assert got[0].dtype == ref[0].dtype == np.float64 and got[1].dtype == ref[1].dtype == np.int64
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
        assert np.array_equal(got[0], v) and np.array_equal(got[1][:len(f)], f)
    assert real(open(str(tmp_path / "tri.ply"), "rb").read(), *_header(str(tmp_path / "tri.ply"))) is not None
    assert real(open(str(tmp_path / "quad.ply"), "rb").read(), *_header(str(tmp_path / "quad.ply"))) is None
    # a plain file of write_ply goes through the fast path too
    sg.write_ply(str(tmp_path / "plain.ply"), v, f)
    got = egobody.read_ply(str(tmp_path / "plain.ply"))
    assert np.array_equal(got[0], v) and np.array_equal(got[1], f)


def _header(path):
    data = open(path, "rb").read()
    end = data.index(b"\n", data.index(b"end_header")) + 1
    els = []
    for ln in data[:end].decode().splitlines():
        tok = ln.split()
        if tok and tok[0] == "element":
            els.append({"name": tok[1], "count": int(tok[2]), "props": []})
        elif tok and tok[0] == "property":
            els[-1]["props"].append(tok[1:])
    return end, els


def test_scan_entries_have_no_cpu_fallback(monkeypatch):
    import torch
    from egogen_amd import _lib
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    v, f = sc.synthetic_room()
    with pytest.raises(_lib.EgxError):
        sg.scan_to_sdf_dict(v, f, res=8)
    with pytest.raises(_lib.EgxError):
        sg.scan_walkable_grid(v, f)
