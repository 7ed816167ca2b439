"""Scene preparation: what a new scene needs before `main_ppo.py` can train in it.

The reference ships its scene files ready-made - `data/room0_sdf.pkl` ({center, scale, sdf}: crowd_ppo/utils.py:54-84),
`room_0/navmesh_tight.ply`, `replica_room0_shapely.pkl`, `room0_samples.pkl` (environments.py:54-63) - and points to an external
tool for other scenes (README.md:97).  This module produces the same four artefacts from triangle meshes:

  signed-distance grid   `mesh_to_sdf_dict` / `scene_sdf_dict`  -> HIP kernel `egx_mesh_sdf` (one grid sample per lane)
  navmesh + polygon      `walkable_grid` -> `grid_to_navmesh`, `grid_to_rings`   (obstacle footprints inflated by the body radius
                         on a raster of the floor; rectangles of free cells as triangles, the free region's outline as rings)
  start / target pairs   `sample_pairs`
  files                  `write_ply` (binary little endian, readable by `egobody.read_ply` / trimesh), `save_scene` (npz)
  random box scenes      `random_box_layout` -> `box_layout_scene` (analytic room + oriented boxes; HIP kernel `egx_sdf_boxes`
                         writes the grid on the device), `add_boxes_to_scene` (the same boxes composed onto a prepared scene)

Scanned rooms (open triangle soups: walls without backs, holes, duplicated vertices) take the `scene_from_scan` path instead
(`python -m egogen_amd.prepare_scene`):

  signed-distance grid   `scan_to_sdf_dict` -> HIP kernel `egx_scan_sdf` (BVH nearest triangle, sign from the pseudo-normal of
                         the nearest feature; host tables: `weld_vertices`, `pseudo_normals`, `build_bvh`)
  walkable raster        `scan_walkable_grid` -> HIP kernel `egx_walkable_raster` (floor support + clearance per cell; host:
                         `detect_floor_height`, `disc_erosion`)

The two SDF paths and the scan raster need the HIP library; everything else is host-side numpy (offline, once per scene)."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np


# ------------------------------------------------------------------------------------------------ meshes
def box_mesh(lo: Sequence[float], hi: Sequence[float]) -> Tuple[np.ndarray, np.ndarray]:
    """Closed axis-aligned box: 8 vertices, 12 triangles, outward orientation."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    v = np.array([[(hi if (i >> a) & 1 else lo)[a] for a in range(3)] for i in range(8)], np.float64)
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    f = np.array([t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))], np.int64)
    return v, f


def merge_meshes(meshes: Sequence[Tuple[np.ndarray, np.ndarray]]) -> Tuple[np.ndarray, np.ndarray]:
    vs, fs, off = [], [], 0
    for v, f in meshes:
        vs.append(np.asarray(v, np.float64))
        fs.append(np.asarray(f, np.int64) + off)
        off += len(v)
    return np.concatenate(vs, 0), np.concatenate(fs, 0)


def write_ply(path: str, vertices: np.ndarray, faces: np.ndarray) -> None:
    v, f = np.asarray(vertices, np.float32), np.asarray(faces, np.int32)
    with open(path, "wb") as fh:
        fh.write((f"ply\nformat binary_little_endian 1.0\nelement vertex {len(v)}\nproperty float x\nproperty float y\n"
                  f"property float z\nelement face {len(f)}\nproperty list uchar int vertex_indices\nend_header\n").encode())
        fh.write(v.astype("<f4").tobytes())
        rec = np.zeros(len(f), np.dtype([("n", "u1"), ("i", "<i4", (3,))]))   # packed: the bytes of struct "<Biii" per face
        rec["n"], rec["i"] = 3, f.reshape(-1, 3)
        fh.write(rec.tobytes())


# ------------------------------------------------------------------------------------------------ SDF
def mesh_to_sdf_dict(vertices: np.ndarray, faces: np.ndarray, res: int = 256, center: Optional[Sequence[float]] = None,
                     half: Optional[float] = None, inside_is_obstacle: bool = True, device: str = "cuda") -> Dict[str, "object"]:
    """Signed-distance grid of a closed mesh as an `sdf_dict` ({'center'[3], 'scale'[], 'sdf'[res,res,res]} float32 tensors on
    `device`, the layout of room0_sdf.pkl after crowd_env_2f.py:302-304).  The cube is center +- half (default: the mesh's
    bounding cube plus 10 %).  inside_is_obstacle: the stored value is > 0 inside the mesh (calc_sdf negates it), else < 0."""
    import torch
    from . import _lib
    if not torch.cuda.is_available():
        raise _lib.EgxError("mesh_to_sdf_dict runs on the HIP device only (no CPU fallback)")
    v, f = np.asarray(vertices, np.float64), np.asarray(faces, np.int64)
    if center is None:
        center = (v.min(0) + v.max(0)) / 2
    if half is None:
        half = float(np.abs(v - np.asarray(center)).max()) * 1.1
    tris = torch.tensor(v[f].reshape(-1, 9), dtype=torch.float32, device=device).contiguous()
    grid = torch.empty(res, res, res, dtype=torch.float32, device=device)
    c = (C.c_float * 3)(*[float(x) for x in center])
    lib = _lib.load()
    _lib.check(lib.egx_mesh_sdf(_lib.ptr(tris), int(tris.shape[0]), c, float(1.0 / half), res, res, res, 1 if inside_is_obstacle else 0,
                                _lib.ptr(grid), _lib.current_stream_ptr()), "egx_mesh_sdf")
    return {"sdf": grid, "center": torch.tensor(np.asarray(center, np.float32), device=device),
            "scale": torch.tensor(np.float32(1.0 / half), device=device)}


def scene_sdf_dict(room: Tuple[np.ndarray, np.ndarray], obstacles: Optional[Tuple[np.ndarray, np.ndarray]], res: int = 256,
                   center: Sequence[float] = (0.0, 0.0, 1.0), half: float = 4.0, device: str = "cuda"):
    """Room shell (closed mesh whose interior is the free space) + obstacle solids -> one grid, < 0 in free space:
    max(d_room, d_obstacles) with d_room < 0 inside the room and d_obstacles > 0 inside an obstacle."""
    import torch
    d = mesh_to_sdf_dict(room[0], room[1], res, center, half, inside_is_obstacle=False, device=device)
    if obstacles is not None and len(obstacles[1]):
        o = mesh_to_sdf_dict(obstacles[0], obstacles[1], res, center, half, inside_is_obstacle=True, device=device)
        d["sdf"] = torch.maximum(d["sdf"], o["sdf"])
    return d


# ------------------------------------------------------------------------------------------------ scanned meshes: SDF
def weld_vertices(vertices: np.ndarray, faces: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """Vertices that share a position become one: (unique vertices [U,3], faces re-indexed [F,3])."""
    v, f = np.asarray(vertices, np.float64).reshape(-1, 3), np.asarray(faces, np.int64)
    order = np.lexsort((v[:, 2], v[:, 1], v[:, 0]))
    vs = v[order]
    new = np.ones(len(v), bool)
    new[1:] = np.any(vs[1:] != vs[:-1], axis=1)
    inv = np.empty(len(v), np.int64)
    inv[order] = np.cumsum(new) - 1
    return vs[new], inv[f]


def degenerate_faces(vertices: np.ndarray, faces: np.ndarray, rel_eps: float = 1e-12) -> np.ndarray:
    """Zero-area triangles (after welding): two equal vertices, or |ab x ac| <= rel_eps * longest edge^2."""
    return _degenerate(*weld_vertices(vertices, faces), rel_eps)


def _degenerate(v: np.ndarray, f: np.ndarray, rel_eps: float = 1e-12) -> np.ndarray:
    t = v[f]
    n = np.linalg.norm(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), axis=1)
    e2 = np.max([((t[:, (k + 1) % 3] - t[:, k]) ** 2).sum(1) for k in range(3)], 0)
    same = (f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 2] == f[:, 0])
    return same | (n <= rel_eps * e2)


def pseudo_normals(vertices: np.ndarray, faces: np.ndarray, flip_normals: bool = False) -> np.ndarray:
    """Pseudo-normals (Baerentzen & Aanaes 2005) of every triangle's features after welding, [F,7,3]: face, edge ab / bc / ca,
    vertex a / b / c.  Face: the unit normal (zero for a degenerate triangle).  Edge: the sum of the unit normals of all faces
    on it (one face on an open boundary, more than two on a non-manifold edge).  Vertex: the angle-weighted sum of the unit
    normals of its faces.  flip_normals: scans whose normals point into the solid."""
    v, f = weld_vertices(vertices, faces)
    t = v[f]
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    nl = np.linalg.norm(n, axis=1)
    deg = _degenerate(v, f)
    fn = np.where(deg[:, None], 0.0, n / np.where(nl > 0, nl, 1.0)[:, None])
    out = np.zeros((len(f), 7, 3))
    out[:, 0] = fn
    V = len(v)
    ek = [np.minimum(f[:, k], f[:, (k + 1) % 3]) * V + np.maximum(f[:, k], f[:, (k + 1) % 3]) for k in range(3)]
    uk, inv = np.unique(np.concatenate(ek), return_inverse=True)
    esum = np.stack([np.bincount(inv, weights=np.tile(fn[:, c], 3), minlength=len(uk)) for c in range(3)], 1)
    for k in range(3):
        out[:, 1 + k] = esum[inv[k * len(f):(k + 1) * len(f)]]
    vsum = np.zeros((V, 3))
    for k in range(3):
        a, b = t[:, (k + 1) % 3] - t[:, k], t[:, (k + 2) % 3] - t[:, k]
        den = np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1)
        ang = np.arccos(np.clip((a * b).sum(1) / np.where(den > 0, den, 1.0), -1.0, 1.0))
        for c in range(3):
            vsum[:, c] += np.bincount(f[:, k], weights=ang * fn[:, c], minlength=V)
    for k in range(3):
        out[:, 4 + k] = vsum[f[:, k]]
    return -out if flip_normals else out


def _morton3(q: np.ndarray) -> np.ndarray:
    """30-bit Morton codes of 10-bit integer coordinates [n,3]."""
    def spread(x):
        x = x.astype(np.uint64) & 0x3FF
        x = (x | (x << 16)) & 0x030000FF
        x = (x | (x << 8)) & 0x0300F00F
        x = (x | (x << 4)) & 0x030C30C3
        x = (x | (x << 2)) & 0x09249249
        return x
    return (spread(q[:, 0]) << 2) | (spread(q[:, 1]) << 1) | spread(q[:, 2])


def build_bvh(triangles: np.ndarray, leaf_size: int = 4, max_levels: int = 24):
    """Bounding-volume hierarchy of triangles [F,3,3] for egx_scan_sdf: the triangles sorted along the Morton curve of their
    centroids (a median split along the curve at every level), `leaf_size` consecutive ones per leaf, and the implicit complete
    binary tree over the leaves (heap order, node h at row h-1, children 2h, 2h+1; padding leaves hold empty boxes).  Boxes are
    taken over the float32 vertices the kernel reads.  Returns (nodes [2^(L+1)-1, 8] float32 {lo, 0, hi, 0}, order [F] (leaf
    order -> input triangle), L).  Raises ValueError when the depth L would exceed max_levels."""
    tri = np.asarray(triangles, np.float32).reshape(-1, 3, 3)
    F = len(tri)
    if F == 0:
        raise ValueError("build_bvh needs at least one triangle")
    nleaf = -(-F // leaf_size)
    L = int(np.ceil(np.log2(nleaf))) if nleaf > 1 else 0
    if L > max_levels:
        raise ValueError(f"BVH depth {L} exceeds the cap {max_levels} ({F} triangles, {leaf_size} per leaf)")
    cen = tri.astype(np.float64).mean(1)
    lo, hi = cen.min(0), cen.max(0)
    q = np.clip(((cen - lo) / max(float((hi - lo).max()), 1e-30) * 1023.0).astype(np.int64), 0, 1023)
    order = np.argsort(_morton3(q), kind="stable")
    t = tri[order]
    pad = (leaf_size << L) - F
    tmin = np.concatenate([t.min(1), np.full((pad, 3), np.inf, np.float32)], 0).reshape(1 << L, leaf_size, 3).min(1)
    tmax = np.concatenate([t.max(1), np.full((pad, 3), -np.inf, np.float32)], 0).reshape(1 << L, leaf_size, 3).max(1)
    levels = [(tmin, tmax)]
    for _ in range(L):
        a, b = levels[-1]
        levels.append((a.reshape(-1, 2, 3).min(1), b.reshape(-1, 2, 3).max(1)))
    lo_all = np.concatenate([lv[0] for lv in reversed(levels)], 0)
    hi_all = np.concatenate([lv[1] for lv in reversed(levels)], 0)
    nodes = np.zeros((len(lo_all), 8), np.float32)
    nodes[:, 0:3], nodes[:, 4:7] = lo_all, hi_all
    return nodes, order, L


def scan_sdf_tables(vertices: np.ndarray, faces: np.ndarray, flip_normals: bool = False, leaf_size: int = 4):
    """Host tables of egx_scan_sdf (include/egogen_hip.h): {'nodes', 'levels', 'leaf_size', 'tris' [F,12], 'pn' [F,21]}."""
    v, f = np.asarray(vertices, np.float64), np.asarray(faces, np.int64)
    pn = pseudo_normals(v, f, flip_normals)
    deg = ~pn[:, 0].any(1)   # zero face normal: a degenerate triangle
    nodes, order, L = build_bvh(v[f], leaf_size)
    tris = np.zeros((len(f), 12), np.float32)
    tris[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]] = v[f[order]].reshape(-1, 9)
    tris[:, 3] = deg[order]
    return {"nodes": nodes, "levels": L, "leaf_size": leaf_size, "tris": tris,
            "pn": pn[order].reshape(-1, 21).astype(np.float32)}


def scan_to_sdf_dict(vertices: np.ndarray, faces: np.ndarray, res: int = 256, center: Optional[Sequence[float]] = None,
                     half: Optional[float] = None, flip_normals: bool = False, device: str = "cuda") -> Dict[str, "object"]:
    """Signed-distance grid of an open, oriented mesh (a scanned room: walls without backs, holes, duplicated vertices): the
    `mesh_to_sdf_dict` layout and defaults, exact unsigned distance (BVH), sign from the pseudo-normal of the nearest feature:
    < 0 on the side the normals face (free space), > 0 behind the surface.  HIP kernel `egx_scan_sdf`."""
    import torch
    from . import _lib
    if not torch.cuda.is_available():
        raise _lib.EgxError("scan_to_sdf_dict runs on the HIP device only (no CPU fallback)")
    v, f = np.asarray(vertices, np.float64), np.asarray(faces, np.int64)
    if center is None:
        center = (v.min(0) + v.max(0)) / 2
    if half is None:
        half = float(np.abs(v - np.asarray(center)).max()) * 1.1
    tb = scan_sdf_tables(v, f, flip_normals)
    dev = {k: torch.from_numpy(tb[k]).to(device).contiguous() for k in ("nodes", "tris", "pn")}
    grid = torch.empty(res, res, res, dtype=torch.float32, device=device)
    c = (C.c_float * 3)(*[float(x) for x in center])
    lib = _lib.load()
    _lib.check(lib.egx_scan_sdf(_lib.ptr(dev["nodes"]), tb["levels"], _lib.ptr(dev["tris"]), _lib.ptr(dev["pn"]), len(f), tb["leaf_size"],
                                c, float(1.0 / half), res, res, res, _lib.ptr(grid), _lib.current_stream_ptr()), "egx_scan_sdf")
    return {"sdf": grid, "center": torch.tensor(np.asarray(center, np.float32), device=device),
            "scale": torch.tensor(np.float32(1.0 / half), device=device)}


# ------------------------------------------------------------------------------------------------ scanned meshes: floor
def detect_floor_height(vertices: np.ndarray, faces: np.ndarray, max_slope_deg: float = 15.0, bin_size: float = 0.02,
                        share: float = 0.25) -> float:
    """The lowest height at which up-facing triangles (normal within max_slope_deg of +z) hold a large share of their area:
    area-weighted histogram of their centroid heights, first bin with >= `share` of the fullest bin's area, refined to the
    area-weighted mean height over that bin and the next."""
    v, f = np.asarray(vertices, np.float64), np.asarray(faces, np.int64)
    t = v[f]
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    nl = np.linalg.norm(n, axis=1)
    up = (nl > 0) & (n[:, 2] >= np.cos(np.radians(max_slope_deg)) * nl)
    if not up.any():
        raise ValueError("no up-facing triangle: cannot detect the floor (is the mesh z-up?)")
    z, w = t[up, :, 2].mean(1), 0.5 * nl[up]
    z0 = float(z.min())
    b = np.floor((z - z0) / bin_size).astype(np.int64)
    hist = np.bincount(b, weights=w)
    k = int(np.flatnonzero(hist >= share * hist.max())[0])
    sel = (b == k) | (b == k + 1)
    return float(np.sum(z[sel] * w[sel]) / np.sum(w[sel]))


def disc_erosion(mask: np.ndarray, radius: float, cell: float) -> np.ndarray:
    """Exact disc erosion on the raster: a cell stays iff every raster cell whose centre is closer than `radius` to its centre
    is set (cells beyond the raster do not count).  Distances are compared in cell units, a cell at exactly `radius` (to 1e-9
    cells^2: radius 0.2 on 0.05 m cells) is not closer."""
    mask = np.asarray(mask, bool)
    r = int(np.ceil(radius / cell))
    lim = (radius / cell) ** 2 - 1e-9
    out = mask.copy()
    P = np.pad(mask, r, constant_values=True)
    nx, ny = mask.shape
    for di in range(-r, r + 1):
        for dj in range(-r, r + 1):
            if di * di + dj * dj < lim and (di or dj):
                out &= P[r + di:r + di + nx, r + dj:r + dj + ny]
    return out


def scan_walkable_raster(vertices: np.ndarray, faces: np.ndarray, radius: float = 0.2, cell: float = 0.05,
                         z_range: Tuple[float, float] = (0.05, 2.0), floor_height: Optional[float] = None, bounds=None,
                         max_slope_deg: float = 15.0, floor_tol: float = 0.03, device: str = "cuda"):
    """HIP kernel `egx_walkable_raster` over the floor raster: (support [nx,ny] bool, clearance [nx,ny] float32, origin[2], cell,
    floor_height).  bounds ((x0, y0), (x1, y1)) defaults to the xy box of the supporting triangles grown by `radius`."""
    import torch
    from . import _lib
    if not torch.cuda.is_available():
        raise _lib.EgxError("scan_walkable_grid runs on the HIP device only (no CPU fallback)")
    v, f = np.asarray(vertices, np.float64), np.asarray(faces, np.int64)
    if floor_height is None:
        floor_height = detect_floor_height(v, f, max_slope_deg)
    cos_up = float(np.cos(np.radians(max_slope_deg)))
    if bounds is None:
        t = v[f]
        n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
        nl = np.linalg.norm(n, axis=1)
        sup = (nl > 0) & (n[:, 2] >= cos_up * nl) & (t[:, :, 2].max(1) >= floor_height - floor_tol) & \
            (t[:, :, 2].min(1) <= floor_height + floor_tol)
        if not sup.any():
            raise ValueError(f"no up-facing triangle near the floor height {floor_height}")
        bounds = (t[sup, :, :2].reshape(-1, 2).min(0) - radius, t[sup, :, :2].reshape(-1, 2).max(0) + radius)
    lo, hi = np.asarray(bounds[0], np.float64)[:2], np.asarray(bounds[1], np.float64)[:2]
    nx, ny = max(int(round((hi[0] - lo[0]) / cell)), 1), max(int(round((hi[1] - lo[1]) / cell)), 1)
    tris = torch.tensor(v[f].reshape(-1, 9), dtype=torch.float32, device=device).contiguous()
    support = torch.empty(nx, ny, dtype=torch.int32, device=device)
    clearance = torch.empty(nx, ny, dtype=torch.float32, device=device)
    lib = _lib.load()
    _lib.check(lib.egx_walkable_raster(_lib.ptr(tris), len(f), float(lo[0]), float(lo[1]), float(cell), nx, ny, float(floor_height),
                                       float(floor_tol), cos_up, float(floor_height + z_range[0]), float(floor_height + z_range[1]),
                                       _lib.ptr(support), _lib.ptr(clearance), _lib.current_stream_ptr()), "egx_walkable_raster")
    return support.cpu().numpy() != 0, clearance.cpu().numpy(), lo.copy(), float(cell), float(floor_height)


def scan_walkable_grid(vertices: np.ndarray, faces: np.ndarray, radius: float = 0.2, cell: float = 0.05,
                       z_range: Tuple[float, float] = (0.05, 2.0), floor_height: Optional[float] = None, bounds=None,
                       max_slope_deg: float = 15.0, floor_tol: float = 0.03, device: str = "cuda"):
    """Walkable raster of a scanned room: free = (support eroded by the body disc) & (clearance > radius), where a cell is
    supported when floor lies under its centre and its clearance is the xy distance to anything inside the height slab
    `z_range` above the floor (detected when not given).  Returns (free [nx,ny] bool, origin[2], cell, floor_height)."""
    support, clearance, origin, cell, fh = scan_walkable_raster(vertices, faces, radius, cell, z_range, floor_height, bounds,
                                                                max_slope_deg, floor_tol, device)
    return disc_erosion(support, radius, cell) & (clearance > radius), origin, cell, fh


# ------------------------------------------------------------------------------------------------ walkable region
def _pt_tri_dist2_2d(px, py, tri):
    """Squared distance of points (px, py) [n] to a 2-D triangle [3,2] (0 inside)."""
    a, b, c = tri
    d2 = np.full(px.shape, np.inf)
    inside = np.ones(px.shape, bool)
    area = (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])
    for p, q in ((a, b), (b, c), (c, a)):
        ex, ey = q[0] - p[0], q[1] - p[1]
        L = max(ex * ex + ey * ey, 1e-30)
        t = np.clip(((px - p[0]) * ex + (py - p[1]) * ey) / L, 0.0, 1.0)
        dx, dy = p[0] + t * ex - px, p[1] + t * ey - py
        d2 = np.minimum(d2, dx * dx + dy * dy)
        side = ex * (py - p[1]) - ey * (px - p[0])
        inside &= (side >= 0) if area >= 0 else (side <= 0)
    if abs(area) > 0:
        d2 = np.where(inside, 0.0, d2)
    return d2


def walkable_grid(floor_lo: Sequence[float], floor_hi: Sequence[float], obstacle_vertices: np.ndarray, obstacle_faces: np.ndarray,
                  radius: float = 0.2, cell: float = 0.05, z_range: Tuple[float, float] = (0.05, 2.0)):
    """Raster of the floor rectangle: a cell is free iff its centre is farther than `radius` from the footprint of every
    obstacle triangle that reaches into the height band `z_range` above the floor.  Returns (free[nx,ny] bool, origin[2], cell)."""
    lo, hi = np.asarray(floor_lo, np.float64)[:2], np.asarray(floor_hi, np.float64)[:2]
    nx, ny = int(round((hi[0] - lo[0]) / cell)), int(round((hi[1] - lo[1]) / cell))
    free = np.ones((nx, ny), bool)
    cx = lo[0] + (np.arange(nx) + 0.5) * cell
    cy = lo[1] + (np.arange(ny) + 0.5) * cell
    v, f = np.asarray(obstacle_vertices, np.float64), np.asarray(obstacle_faces, np.int64)
    for t in v[f] if len(f) else []:
        if t[:, 2].max() < z_range[0] or t[:, 2].min() > z_range[1]:
            continue
        i0 = max(int(np.floor((t[:, 0].min() - radius - lo[0]) / cell)), 0)
        i1 = min(int(np.ceil((t[:, 0].max() + radius - lo[0]) / cell)), nx)
        j0 = max(int(np.floor((t[:, 1].min() - radius - lo[1]) / cell)), 0)
        j1 = min(int(np.ceil((t[:, 1].max() + radius - lo[1]) / cell)), ny)
        if i0 >= i1 or j0 >= j1:
            continue
        X, Y = np.meshgrid(cx[i0:i1], cy[j0:j1], indexing="ij")
        d2 = _pt_tri_dist2_2d(X.ravel(), Y.ravel(), t[:, :2]).reshape(X.shape)
        free[i0:i1, j0:j1] &= d2 > radius * radius
    return free, lo.copy(), float(cell)


def grid_to_navmesh(free: np.ndarray, origin: np.ndarray, cell: float, floor_height: float = 0.0):
    """Free cells -> maximal rectangles (runs along y merged along x while identical) -> two triangles each.  Any triangle
    cover of the free region serves `get_map` (a point is walkable iff some triangle contains it, batch_gen_amass.py:949-961)."""
    nx, ny = free.shape
    rects, open_runs = [], {}
    for i in range(nx + 1):
        runs = set()
        if i < nx:
            col = np.concatenate([[False], free[i], [False]])
            edges = np.flatnonzero(col[1:] != col[:-1])
            runs = {(int(edges[k]), int(edges[k + 1])) for k in range(0, len(edges), 2)}
        for r in list(open_runs):
            if r not in runs:
                rects.append((open_runs.pop(r), i, r[0], r[1]))
        for r in runs:
            open_runs.setdefault(r, i)
    v, f = [], []
    for (i0, i1, j0, j1) in rects:
        x0, x1, y0, y1 = origin[0] + i0 * cell, origin[0] + i1 * cell, origin[1] + j0 * cell, origin[1] + j1 * cell
        b = len(v)
        v += [[x0, y0, floor_height], [x1, y0, floor_height], [x1, y1, floor_height], [x0, y1, floor_height]]
        f += [[b, b + 1, b + 2], [b, b + 2, b + 3]]
    return np.asarray(v, np.float64).reshape(-1, 3), np.asarray(f, np.int64).reshape(-1, 3)


def grid_to_rings(free: np.ndarray, origin: np.ndarray, cell: float, largest_only: bool = True) -> List[np.ndarray]:
    """Outline of the free region as closed rings [n,2] (collinear points removed, largest ring first).  With
    `largest_only`, cells not connected (4-neighbourhood) to the largest free component are dropped first - the
    reference keeps the biggest polygon of the navmesh union (environments.py:639-643)."""
    free = free.copy()
    if largest_only:
        lab = -np.ones(free.shape, np.int64)
        sizes = []
        for s in zip(*np.nonzero(free)):
            if lab[s] >= 0:
                continue
            stack, lab[s], cnt = [s], len(sizes), 0
            while stack:
                i, j = stack.pop()
                cnt += 1
                for a, b in ((i + 1, j), (i - 1, j), (i, j + 1), (i, j - 1)):
                    if 0 <= a < free.shape[0] and 0 <= b < free.shape[1] and free[a, b] and lab[a, b] < 0:
                        lab[a, b] = len(sizes)
                        stack.append((a, b))
            sizes.append(cnt)
        if sizes:
            free &= lab == int(np.argmax(sizes))
    P = np.pad(free, 1)
    nxt: Dict[Tuple[int, int], List[Tuple[int, int]]] = {}
    for i, j in zip(*np.nonzero(free)):
        pi, pj = i + 1, j + 1
        if not P[pi, pj - 1]:
            nxt.setdefault((i, j), []).append((i + 1, j))
        if not P[pi + 1, pj]:
            nxt.setdefault((i + 1, j), []).append((i + 1, j + 1))
        if not P[pi, pj + 1]:
            nxt.setdefault((i + 1, j + 1), []).append((i, j + 1))
        if not P[pi - 1, pj]:
            nxt.setdefault((i, j + 1), []).append((i, j))
    rings = []
    while nxt:
        start = next(iter(nxt))
        ring, cur = [start], start
        while True:
            outs = nxt[cur]
            step = outs.pop()
            if not outs:
                del nxt[cur]
            cur = step
            if cur == start:
                break
            ring.append(cur)
        pts = np.asarray(ring, np.float64)
        keep = []
        n = len(pts)
        for k in range(n):
            a, b, c = pts[k - 1], pts[k], pts[(k + 1) % n]
            if (b[0] - a[0]) * (c[1] - b[1]) - (b[1] - a[1]) * (c[0] - b[0]) != 0:
                keep.append(k)
        pts = pts[keep]
        pts = np.concatenate([pts, pts[:1]], 0)
        rings.append(np.stack([origin[0] + pts[:, 0] * cell, origin[1] + pts[:, 1] * cell], 1))
    area = lambda r: abs(0.5 * np.sum(r[:-1, 0] * r[1:, 1] - r[1:, 0] * r[:-1, 1]))
    rings.sort(key=lambda r: -area(r))
    return rings


def rings_contain(rings: List[np.ndarray], x: np.ndarray, y: np.ndarray) -> np.ndarray:
    e = np.concatenate([np.concatenate([r[:-1], r[1:]], 1) for r in rings], 0)
    x, y = np.asarray(x, np.float64).reshape(-1), np.asarray(y, np.float64).reshape(-1)
    x0, y0, x1, y1 = (e[:, k][None, :] for k in range(4))
    with np.errstate(divide="ignore", invalid="ignore"):
        straddle = (y0 > y[:, None]) != (y1 > y[:, None])
        xint = x0 + (y[:, None] - y0) * (x1 - x0) / (y1 - y0)
    return (np.sum(straddle & (x[:, None] < xint), axis=1) & 1) == 1


def sample_pairs(rings: List[np.ndarray], n: int, min_dist: float = 1.7, seed: int = 0, floor_height: float = 0.0) -> np.ndarray:
    """n (start, target) pairs [n,2,3], both inside the walkable polygon and at least `min_dist` apart (the content of
    `*_samples.pkl`, environments.py:59-63)."""
    rng = np.random.default_rng(seed)
    lo = np.min([r.min(0) for r in rings], 0)
    hi = np.max([r.max(0) for r in rings], 0)
    out = np.zeros((0, 2, 3))
    while len(out) < n:
        p = rng.uniform(lo, hi, (4 * n, 2, 2))
        ok = rings_contain(rings, p[:, 0, 0], p[:, 0, 1]) & rings_contain(rings, p[:, 1, 0], p[:, 1, 1]) & \
            (np.linalg.norm(p[:, 0] - p[:, 1], axis=-1) >= min_dist)
        p = p[ok]
        out = np.concatenate([out, np.concatenate([p, np.full(p.shape[:2] + (1,), floor_height)], -1)], 0)
    return out[:n].astype(np.float32)


def box_scene_from_meshes(floor_lo, floor_hi, obstacle_mesh, radius: float = 0.2, cell: float = 0.05, n_pairs: int = 20000,
                          min_dist: float = 1.7, seed: int = 0, floor_height: float = 0.0) -> dict:
    """One entry of `VecCrowdEnv(scene_kind='box', box_scenes=[...])`: {'edges', 'tris', 'floor_height', 'pairs'} plus the
    navmesh ('nav_v', 'nav_f') and polygon ('rings') they were derived from."""
    from . import synth
    free, origin, cell = walkable_grid(floor_lo, floor_hi, obstacle_mesh[0], obstacle_mesh[1], radius, cell)
    nav_v, nav_f = grid_to_navmesh(free, origin, cell, floor_height)
    rings = grid_to_rings(free, origin, cell)
    return {"edges": synth.rings_to_edges(rings).astype(np.float32), "tris": nav_v[nav_f][:, :, :2].reshape(-1, 6).astype(np.float32),
            "floor_height": float(floor_height), "pairs": sample_pairs(rings, n_pairs, min_dist, seed, floor_height),
            "nav_v": nav_v, "nav_f": nav_f, "rings": rings}


def grid_to_cell_navmesh(free: np.ndarray, origin: np.ndarray, cell: float, floor_height: float = 0.0):
    """Free cells -> two triangles each on shared corner vertices: a conforming triangulation (no T-junctions), so the union's
    outline is the set of edges with one triangle - what `egobody.navmesh_walkable_rings` reads from `navmesh_tight.ply`."""
    ii, jj = np.nonzero(free)
    corners = np.stack([np.stack([ii, jj], 1), np.stack([ii + 1, jj], 1), np.stack([ii + 1, jj + 1], 1), np.stack([ii, jj + 1], 1)], 1)
    uniq, inv = np.unique(corners.reshape(-1, 2), axis=0, return_inverse=True)
    q = inv.reshape(-1, 4)
    f = np.concatenate([q[:, [0, 1, 2]], q[:, [0, 2, 3]]], 0)
    v = np.stack([origin[0] + uniq[:, 0] * cell, origin[1] + uniq[:, 1] * cell, np.full(len(uniq), float(floor_height))], 1)
    return v.astype(np.float64), f.astype(np.int64)


def scene_from_scan(vertices: np.ndarray, faces: np.ndarray, res: int = 256, cell: float = 0.05, radius: float = 0.2,
                    floor_height: Optional[float] = None, flip_normals: bool = False, n_pairs: int = 20000, min_dist: float = 1.7,
                    seed: int = 0, z_range: Tuple[float, float] = (0.05, 2.0), max_slope_deg: float = 15.0, floor_tol: float = 0.03,
                    center: Optional[Sequence[float]] = None, half: Optional[float] = None, device: str = "cuda") -> dict:
    """A scanned room (z-up triangle soup) -> the `box_scene_from_meshes` dict (edges, tris, floor_height, pairs, nav_v, nav_f,
    rings) plus 'sdf_dict' (scan_to_sdf_dict), 'z_offset', the raster ('free', 'origin', 'cell') and per-stage 'times' [s].
    The mesh is first shifted down by the floor height (given or detected) - the SDF-kind environment puts bodies on z = 0 -
    and everything is built from the shifted mesh ('vertices'); 'z_offset' records the shift."""
    import time
    import torch
    times = {}
    t0 = time.perf_counter()
    v, f = np.asarray(vertices, np.float64), np.asarray(faces, np.int64)
    if flip_normals:
        f = f[:, ::-1].copy()
    z_off = float(floor_height) if floor_height is not None else detect_floor_height(v, f, max_slope_deg)
    v = v - np.array([0.0, 0.0, z_off])
    times["floor"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    free, origin, cell, _ = scan_walkable_grid(v, f, radius, cell, z_range, 0.0, None, max_slope_deg, floor_tol, device)
    times["raster"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    nav_v, nav_f = grid_to_navmesh(free, origin, cell, 0.0)
    rings = grid_to_rings(free, origin, cell)
    if not rings:
        raise ValueError("no walkable cell: check the floor height, the body radius and the mesh's orientation (z-up)")
    pairs = sample_pairs(rings, n_pairs, min_dist, seed, 0.0)
    times["navmesh"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    sdf = scan_to_sdf_dict(v, f, res, center, half, False, device)
    torch.cuda.synchronize()
    times["sdf"] = time.perf_counter() - t0
    from . import synth
    return {"edges": synth.rings_to_edges(rings).astype(np.float32), "tris": nav_v[nav_f][:, :, :2].reshape(-1, 6).astype(np.float32),
            "floor_height": 0.0, "pairs": pairs, "nav_v": nav_v, "nav_f": nav_f, "rings": rings, "sdf_dict": sdf, "z_offset": z_off,
            "free": free, "origin": origin, "cell": cell, "vertices": v, "faces": f, "times": times}


# ------------------------------------------------------------------------------------------------ random box scenes
# Room, cube centre and half size of `synth.make_sdf_scene` ('single_box'): what `boxes:SxK` scenes are built in.
ROOM_LO, ROOM_HI = (-3.9, -3.9, 0.0), (3.9, 3.9, 4.9)
ROOM_CENTER, ROOM_HALF = (0.0, 0.0, 1.0), 4.0
MAX_BOXES = 16   # EGX_SDF_MAX_BOXES (include/egogen_hip.h)


def _box_frame(x, y, box):
    """|(p - c) rotated by -yaw| - half extents: the two horizontal terms of the box distance."""
    cx, cy, hx, hy, yaw = float(box[0]), float(box[1]), float(box[2]), float(box[3]), float(box[6])
    c, s = np.cos(yaw), np.sin(yaw)
    dx, dy = np.asarray(x, np.float64) - cx, np.asarray(y, np.float64) - cy
    return np.abs(c * dx + s * dy) - hx, np.abs(c * dy - s * dx) - hy


def oriented_box_sdf(points: np.ndarray, box: Sequence[float]) -> np.ndarray:
    """Exact signed distance (float64, negative inside) of points [...,3] to one box of a layout,
    (cx, cy, half_x, half_y, z_lo, z_hi, yaw): the box |x| <= half_x, |y| <= half_y, z_lo <= z <= z_hi rotated by yaw about z
    and moved to (cx, cy).  With q = |R(-yaw)(p - c)| - h per axis:  d = |max(q, 0)| + min(max(q_x, q_y, q_z), 0).  This is the
    definition `egx_sdf_boxes` evaluates in float32."""
    p = np.asarray(points, np.float64)
    qx, qy = _box_frame(p[..., 0], p[..., 1], box)
    z0, z1 = float(box[4]), float(box[5])
    q = np.stack([qx, qy, np.abs(p[..., 2] - 0.5 * (z0 + z1)) - 0.5 * (z1 - z0)], -1)
    return np.linalg.norm(np.maximum(q, 0.0), axis=-1) + np.minimum(q.max(-1), 0.0)


def footprint_distance(x: np.ndarray, y: np.ndarray, box: Sequence[float]) -> np.ndarray:
    """Signed distance in the floor plane to a box's footprint (its rotated rectangle), negative inside."""
    q = np.stack(_box_frame(x, y, box), -1)
    return np.linalg.norm(np.maximum(q, 0.0), axis=-1) + np.minimum(q.max(-1), 0.0)


def footprint_ring(box: Sequence[float], ccw: bool = False) -> np.ndarray:
    """The footprint's corners as a closed ring [5,2] (clockwise by default: a hole of the walkable polygon)."""
    cx, cy, hx, hy, yaw = float(box[0]), float(box[1]), float(box[2]), float(box[3]), float(box[6])
    c, s = np.cos(yaw), np.sin(yaw)
    loc = np.array([[-hx, -hy], [hx, -hy], [hx, hy], [-hx, hy], [-hx, -hy]])
    r = np.stack([cx + c * loc[:, 0] - s * loc[:, 1], cy + s * loc[:, 0] + c * loc[:, 1]], 1)
    return r if ccw else r[::-1].copy()


def random_box_layout(rng: np.random.Generator, num_boxes: int, room_lo: Sequence[float], room_hi: Sequence[float],
                      size: Tuple[float, float] = (0.5, 1.5), height: Tuple[float, float] = (0.5, 1.5), yaw: bool = True,
                      wall_margin: float = 0.6, gap: float = 0.8, max_tries: int = 2000) -> np.ndarray:
    """`num_boxes` boxes standing on the floor of the room, [K,7] float64 rows (cx, cy, half_x, half_y, z_lo, z_hi, yaw): side
    lengths and heights uniform in `size` / `height` (the reference's box obstacles are 0.5 - 1.5 m, environments.py:386-402),
    yaw uniform in [-pi, pi) (0 without `yaw`).  Sequential rejection on bounding circles (radius = half diagonal of the
    footprint): a box's circle lies `wall_margin` inside the walls and its centre at least r_i + r_j + gap from every box placed
    before, so footprints are disjoint holes of the walkable polygon and a body passes between any two.  Every draw (size, yaw
    and centre) counts as one try; ValueError after `max_tries` tries for the whole layout."""
    lo, hi = np.asarray(room_lo, np.float64)[:2], np.asarray(room_hi, np.float64)[:2]
    out = np.zeros((int(num_boxes), 7))
    rad = np.zeros(int(num_boxes))
    k = tries = 0
    while k < num_boxes:
        if tries >= max_tries:
            raise ValueError(f"random_box_layout: placed {k} of {num_boxes} boxes in {max_tries} tries (room {lo} .. {hi}, wall margin "
                             f"{wall_margin}, gap {gap}): fewer boxes or a larger room")
        tries += 1
        half = rng.uniform(size[0], size[1], 2) / 2
        h = rng.uniform(height[0], height[1])
        a = rng.uniform(-np.pi, np.pi) if yaw else 0.0
        u = rng.uniform(0.0, 1.0, 2)
        r = float(np.hypot(half[0], half[1]))
        span = hi - lo - 2 * (r + wall_margin)
        if np.any(span <= 0):
            continue
        c = lo + r + wall_margin + u * span
        if k and np.any(np.linalg.norm(out[:k, :2] - c, axis=1) < rad[:k] + r + gap):
            continue
        out[k], rad[k] = (c[0], c[1], half[0], half[1], 0.0, h, a), r
        k += 1
    return out


def sdf_boxes(layout: np.ndarray, center: Sequence[float], scale: float, dims: Optional[Sequence[int]] = None,
              room: Optional[Tuple[Sequence[float], Sequence[float]]] = None, base=None, out=None, device: str = "cuda"):
    """HIP kernel `egx_sdf_boxes`: max(start, max_k(-oriented_box_sdf(., box_k))) on the sample grid of `mesh_to_sdf_dict`, start
    = `base` (a float32 device grid; `out` may be the same tensor: in place) or the signed distance to the `room` (lo[3], hi[3]).
    Returns the device grid [d0,d1,d2]."""
    import torch
    from . import _lib
    if not torch.cuda.is_available():
        raise _lib.EgxError("sdf_boxes runs on the HIP device only (no CPU fallback)")
    if base is not None:
        if not (isinstance(base, torch.Tensor) and base.is_cuda and base.dtype == torch.float32 and base.dim() == 3 and base.is_contiguous()):
            raise ValueError("base: a contiguous float32 [d0,d1,d2] tensor on the device")
        dims = tuple(base.shape) if dims is None else tuple(dims)
        if tuple(base.shape) != tuple(dims):
            raise ValueError(f"base grid {tuple(base.shape)} != dims {tuple(dims)}")
    if dims is None:
        raise ValueError("dims or a base grid is needed")
    d0, d1, d2 = [int(x) for x in dims]
    if out is None:
        out = torch.empty(max(d0, 0), max(d1, 0), max(d2, 0), dtype=torch.float32, device=base.device if base is not None else device)
    elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (d0, d1, d2)):
        raise ValueError("out: a contiguous float32 device tensor of the grid's dimensions")
    lay = np.ascontiguousarray(np.asarray(layout, np.float32).reshape(-1, 7))
    K = len(lay)
    boxes = (C.c_float * max(7 * K, 1))(*lay.reshape(-1).tolist())
    rm = None if room is None else (C.c_float * 6)(*[float(x) for x in list(room[0])[:3] + list(room[1])[:3]])
    c = (C.c_float * 3)(*[float(x) for x in center])
    _lib.check(_lib.load().egx_sdf_boxes(_lib.ptr(base), rm, boxes, K, c, float(scale), d0, d1, d2, C.c_void_p(out.data_ptr()),
                                         _lib.current_stream_ptr()), "egx_sdf_boxes")
    return out


def sample_clear_pairs(layout: np.ndarray, room_lo, room_hi, n: int, clearance: float = 0.5, min_dist: float = 1.7, seed=0,
                       floor_height: float = 0.0) -> np.ndarray:
    """n (start, target) pairs [n,2,3] float32, at least `min_dist` apart, both ends at least `clearance` from every footprint of
    the layout and from the walls of the room rectangle."""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(room_lo, np.float64)[:2] + clearance, np.asarray(room_hi, np.float64)[:2] - clearance
    if np.any(hi <= lo):
        raise ValueError("the room is narrower than twice the clearance")
    out = np.zeros((0, 2, 3))
    for _ in range(200):
        p = rng.uniform(lo, hi, (4 * n, 2, 2))
        ok = np.linalg.norm(p[:, 0] - p[:, 1], axis=-1) >= min_dist
        for b in np.asarray(layout, np.float64).reshape(-1, 7):
            ok &= (footprint_distance(p[..., 0], p[..., 1], b) >= clearance).all(1)
        p = p[ok]
        out = np.concatenate([out, np.concatenate([p, np.full(p.shape[:2] + (1,), floor_height)], -1)], 0)
        if len(out) >= n:
            return out[:n].astype(np.float32)
    raise ValueError(f"only {len(out)} of {n} pairs found: the boxes leave too little room at clearance {clearance}")


def box_layout_rings(layout: np.ndarray, room_lo, room_hi) -> List[np.ndarray]:
    """Walkable polygon of a box layout: the room rectangle counter-clockwise, one clockwise ring per (un-inflated) footprint -
    what `synth.sdf_scene_polygon` gives for 'single_box'."""
    from . import synth
    return [synth.rect_ring(np.asarray(room_lo, np.float64)[:2], np.asarray(room_hi, np.float64)[:2], True)] + \
        [footprint_ring(b) for b in np.asarray(layout, np.float64).reshape(-1, 7)]


def box_layout_scene(layout: np.ndarray, res: int = 256, device: str = "cuda", n_pairs: int = 4096, clearance: float = 0.5,
                     seed=0, name: Optional[str] = None) -> dict:
    """One entry of `VecCrowdEnv(sdf_scenes=[...])` from a box layout in `make_sdf_scene`'s room: {'sdf_dict' (the grid is built on
    the device by `egx_sdf_boxes` and stays there), 'rings', 'pairs', 'name', 'boxes'}."""
    import torch
    lay = np.asarray(layout, np.float64).reshape(-1, 7)
    grid = sdf_boxes(lay, ROOM_CENTER, 1.0 / ROOM_HALF, (res, res, res), room=(ROOM_LO, ROOM_HI), device=device)
    sdf = {"sdf": grid, "center": torch.tensor(np.asarray(ROOM_CENTER, np.float32), device=grid.device),
           "scale": torch.tensor(np.float32(1.0 / ROOM_HALF), device=grid.device)}
    return {"sdf_dict": sdf, "rings": box_layout_rings(lay, ROOM_LO, ROOM_HI),
            "pairs": sample_clear_pairs(lay, ROOM_LO, ROOM_HI, n_pairs, clearance, seed=seed),
            "name": name or f"boxes{len(lay)}", "boxes": lay}


def stamp_boxes(free: np.ndarray, origin: np.ndarray, cell: float, layout: np.ndarray, radius: float = 0.2) -> np.ndarray:
    """The walkable raster with the boxes of a layout on it: a cell stays free iff it was free and its centre is farther than
    `radius` (the body radius the raster was inflated by) from every footprint - `walkable_grid`'s rule."""
    free = np.asarray(free, bool).copy()
    nx, ny = free.shape
    X, Y = np.meshgrid(origin[0] + (np.arange(nx) + 0.5) * cell, origin[1] + (np.arange(ny) + 0.5) * cell, indexing="ij")
    for b in np.asarray(layout, np.float64).reshape(-1, 7):
        free &= footprint_distance(X, Y, b) > radius
    return free


def add_boxes_to_scene(scene: dict, layout: np.ndarray, radius: float = 0.2, n_pairs: Optional[int] = None, min_dist: float = 1.7,
                       seed=0, name: Optional[str] = None, device: str = "cuda") -> dict:
    """Boxes on the floor of a prepared scene that carries its raster ('free', 'origin', 'cell': `scene_from_scan`, or a file
    saved from one): the cells under the inflated footprints are stamped out, rings and pairs are re-derived with
    `grid_to_rings` / `sample_pairs`, and the boxes are composed onto the scene's SDF grid IN PLACE when it is a device tensor
    (a host grid is uploaded first).  Returns {'sdf_dict', 'rings', 'pairs', 'name', 'boxes', 'free', 'origin', 'cell'}."""
    import torch
    for k in ("free", "origin", "cell", "sdf_dict"):
        if k not in scene:
            raise ValueError(f"add_boxes_to_scene: the scene has no {k!r}; it needs its raster (free, origin, cell) and SDF grid")
    lay = np.asarray(layout, np.float64).reshape(-1, 7)
    origin, cell = np.asarray(scene["origin"], np.float64), float(scene["cell"])
    free = stamp_boxes(scene["free"], origin, cell, lay, radius)
    rings = grid_to_rings(free, origin, cell)
    if not rings:
        raise ValueError("no walkable cell is left after placing the boxes")
    fh = float(scene.get("floor_height", 0.0))
    pairs = sample_pairs(rings, int(n_pairs or len(scene["pairs"])), min_dist, seed, fh)
    sd = scene["sdf_dict"]
    g = sd["sdf"]
    if not (isinstance(g, torch.Tensor) and g.is_cuda):
        g = torch.as_tensor(np.asarray(g, np.float32)).to(device)
    g = g.squeeze()
    if g.dtype != torch.float32 or not g.is_contiguous():
        g = g.float().contiguous()
    c = sd["center"]
    c = (c.detach().cpu().numpy() if hasattr(c, "detach") else np.asarray(c)).reshape(-1)
    s = sd["scale"]
    s = float(s.item() if hasattr(s, "item") else s)
    sdf_boxes(lay, c, s, base=g, out=g)
    return {"sdf_dict": {"sdf": g, "center": sd["center"], "scale": sd["scale"]}, "rings": rings, "pairs": pairs,
            "name": name or f"{scene.get('name', 'scene')}+boxes{len(lay)}", "boxes": lay, "free": free, "origin": origin, "cell": cell}


def save_scene(path: str, scene: dict, sdf_dict: Optional[dict] = None) -> None:
    """npz pack of a generated scene (polygon rings flattened with offsets; the SDF grid if given)."""
    out = {"edges": scene["edges"], "tris": scene["tris"], "floor_height": np.float32(scene["floor_height"]), "pairs": scene["pairs"],
           "nav_v": scene["nav_v"], "nav_f": scene["nav_f"], "ring_xy": np.concatenate(scene["rings"], 0),
           "ring_off": np.cumsum([0] + [len(r) for r in scene["rings"]]).astype(np.int32)}
    if all(k in scene for k in ("free", "origin", "cell")):   # the walkable raster: what add_boxes_to_scene stamps boxes onto
        out["free"], out["origin"], out["cell"] = np.asarray(scene["free"], bool), np.asarray(scene["origin"], np.float64), np.float64(scene["cell"])
    if "z_offset" in scene:   # scene_from_scan: the height the scan was shifted down by (not read back by load_scene_file)
        out["z_offset"] = np.float64(scene["z_offset"])
    if sdf_dict is not None:
        for k in ("sdf", "center", "scale"):
            v = sdf_dict[k]
            out["sdf_" + k] = v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
    np.savez_compressed(path, **out)
