"""`GeodesicField`: the distance to a goal along the walkable raster (`free[nx,ny]`, `origin[2]`, `cell` of
`scene_gen.walkable_grid`, `scene_from_scan`, `add_boxes_to_scene` and of every scene file `save_scene` writes), built on the device
by `egx_geodesic_field` and read by `sample` and by the selection kernels of `GAMMAPrimitiveComboGenOP.generate_sequence_to_goal`
(`geodesic=`).

The metric: shortest paths over the free cells with 8 neighbours, `cell` per axis step and `cell * sqrt(2)` per diagonal step, no
diagonal past a blocked axis neighbour.  Such a path overestimates the Euclidean length by up to 8.24 % (1 / cos 22.5 deg)
depending on its heading.  Seeds: the free cells whose centre lies within 1.5 cells of the goal, each at its Euclidean distance to
the goal, so the field is accurate below a cell near the goal.  Off the field (no finite cell among the four around a point) the
value is `OFF` = 1.0e4 m: finite, and far above any real path."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _lib

OFF = 1.0e4     # EGX_GEODESIC_OFF
BATCH = 8       # EGX_GEODESIC_BATCH
SEED_RADIUS = 1.5


def seed_cells(free: np.ndarray, origin, cell: float, goal):
    """The seeds of one field: free [H,W] bool, origin [2], goal [>=2] -> (cells [n] int64, flat i * W + j; values [n] float32).
    A seed is a free cell whose centre (origin + (i + 0.5, j + 0.5) * cell) lies within 1.5 * cell of the goal's xy; its value
    is that distance, computed in float64 and rounded once.  No seed: two empty arrays."""
    free = np.asarray(free, bool)
    H, W = free.shape
    o, g, cell = np.asarray(origin, np.float64).reshape(2), np.asarray(goal, np.float64).reshape(-1)[:2], float(cell)
    r = SEED_RADIUS * cell
    ci, cj = (g[0] - o[0]) / cell - 0.5, (g[1] - o[1]) / cell - 0.5
    i0, i1 = max(int(np.floor(ci - SEED_RADIUS)) - 1, 0), min(int(np.ceil(ci + SEED_RADIUS)) + 2, H)
    j0, j1 = max(int(np.floor(cj - SEED_RADIUS)) - 1, 0), min(int(np.ceil(cj + SEED_RADIUS)) + 2, W)
    if i0 >= i1 or j0 >= j1:
        return np.zeros(0, np.int64), np.zeros(0, np.float32)
    I, J = np.meshgrid(np.arange(i0, i1), np.arange(j0, j1), indexing="ij")
    d = np.sqrt((o[0] + (I + 0.5) * cell - g[0]) ** 2 + (o[1] + (J + 0.5) * cell - g[1]) ** 2)
    keep = free[i0:i1, j0:j1] & (d <= r)
    return (I[keep].astype(np.int64) * W + J[keep]).reshape(-1), d[keep].astype(np.float32).reshape(-1)


def _checked(free, origin, cell, goals, scene_index):
    """The host half of `from_raster`: shapes, ranges and seeds, no device -> (free [S,H,W] uint8, origin [S,2] float64, cell,
    goals [F,3] float64, scene_index [F] int64, seed cells [n] int64 (flat f*H*W + i*W + j), seed values [n] float32)"""
    free = np.asarray(free.cpu() if torch.is_tensor(free) else free)
    if free.ndim == 2:
        free = free[None]
    if free.ndim != 3 or free.shape[1] < 1 or free.shape[2] < 1:
        raise ValueError(f"free must be [H,W] or [S,H,W], got {tuple(free.shape)}")
    free = free.astype(bool)
    S, H, W = free.shape
    origin = np.asarray(origin.cpu() if torch.is_tensor(origin) else origin, np.float64)
    if origin.shape == (2,):
        origin = np.repeat(origin[None], S, 0)
    if origin.shape != (S, 2) or not np.isfinite(origin).all():
        raise ValueError(f"origin must be [2] or [{S},2] and finite, got shape {tuple(origin.shape)}")
    cell = float(cell)
    if not (np.isfinite(cell) and cell > 0):
        raise ValueError(f"cell must be positive and finite, got {cell}")
    goals = np.asarray(goals.cpu() if torch.is_tensor(goals) else goals, np.float64)
    if goals.ndim != 2 or goals.shape[1] not in (2, 3) or goals.shape[0] < 1:
        raise ValueError(f"goals must be [F,3] or [F,2], got {tuple(goals.shape)}")
    if goals.shape[1] == 2:
        goals = np.concatenate([goals, np.zeros((len(goals), 1))], 1)
    F = len(goals)
    for f in range(F):
        if not np.isfinite(goals[f]).all():
            raise ValueError(f"goal {f} is not finite: {goals[f].tolist()}")
    if scene_index is None:
        if S != 1 and S != F:
            raise ValueError(f"{S} rasters and {F} goals need scene_index [F]")
        scene_index = np.zeros(F, np.int64) if S == 1 else np.arange(F)
    else:
        scene_index = np.asarray(scene_index.cpu() if torch.is_tensor(scene_index) else scene_index).reshape(-1).astype(np.int64)
        if scene_index.shape != (F,):
            raise ValueError(f"scene_index must hold one raster per goal ({F}), got {scene_index.size}")
        if scene_index.min() < 0 or scene_index.max() >= S:
            raise ValueError(f"scene_index must lie in [0, {S}), got {scene_index.tolist()}")
    if F * H * W >= 2 ** 31 or S * H * W >= 2 ** 31:
        raise ValueError(f"{F} fields / {S} rasters of {H} x {W} cells exceed 2^31 cells")
    cells, values = [], []
    for f in range(F):
        c, v = seed_cells(free[scene_index[f]], origin[scene_index[f]], cell, goals[f])
        if len(c) == 0:
            raise ValueError(f"goal {f} at ({goals[f, 0]:.3f}, {goals[f, 1]:.3f}) has no seed: no free cell of its raster has its centre "
                             f"within {SEED_RADIUS} cells ({SEED_RADIUS * cell:.3f} m) of it")
        cells.append(c + f * H * W)
        values.append(v)
    return free.astype(np.uint8), origin, cell, goals, scene_index, np.concatenate(cells), np.concatenate(values)


class GeodesicField:
    """F distance-to-goal fields on the device: dist [F,H,W] float32 metres (+inf on blocked and unreachable cells), origin [F,2],
    cell, goals [F,3], passes (launches the build took).  `sample(points)` reads them; `generate_sequence_to_goal(geodesic=)`
    steers by them."""

    def __init__(self, dist, origin, cell, goals, passes):
        self.dist, self.origin, self.cell, self.goals, self.passes = dist, origin, float(cell), goals, int(passes)

    def __len__(self):
        return self.dist.shape[0]

    @classmethod
    def from_raster(cls, free, origin, cell, goals, scene_index=None, device="cuda") -> "GeodesicField":
        """free [H,W] or [S,H,W] bool, origin [2] or [S,2], cell, goals [F,3] or [F,2] (world), scene_index [F] (the raster of each
        goal; may be omitted for one raster, or one raster per goal).  The rasters of a call share H, W and cell.  ValueError
        for mismatched shapes, a non-finite goal, a scene_index out of range and a goal without a seed (not on or next to a free
        cell); `_lib.EgxError` if the build does not converge within H * W + 1 passes."""
        free, origin, cell, goals, scene_index, cells, values = _checked(free, origin, cell, goals, scene_index)
        S, H, W = free.shape
        F = len(goals)
        dev = torch.device(device)
        lib = _lib.load()
        t = lambda a, dt: torch.as_tensor(a, dtype=dt).to(dev).contiguous()
        free_d, cells_d, values_d = t(free, torch.uint8), t(cells, torch.int32), t(values, torch.float32)
        fs = t(scene_index, torch.int32) if S > 1 else None
        dist, tmp = torch.empty(F, H, W, device=dev), torch.empty(F, H, W, device=dev)
        flags = torch.zeros(BATCH, device=dev, dtype=torch.int32)
        passes = C.c_int32(0)
        w1, w2 = np.float32(cell), np.float32(np.float64(cell) * np.sqrt(2.0))
        with torch.cuda.device(dev):
            _lib.check(lib.egx_geodesic_field(_lib.ptr(free_d), _lib.ptr(fs), S, F, H, W, float(w1), float(w2), _lib.ptr(cells_d),
                                              _lib.ptr(values_d), len(cells), _lib.ptr(dist), _lib.ptr(tmp), _lib.ptr(flags),
                                              C.byref(passes), _lib.current_stream_ptr()), "egx_geodesic_field")
        return cls(dist, t(origin[scene_index], torch.float32), cell, t(goals, torch.float32), passes.value)

    @classmethod
    def from_scene(cls, d: dict, goals, device="cuda") -> "GeodesicField":
        """From the dict `setup_world.load_scene_file(path, raster=True)` returns (or any dict with free, origin, cell)."""
        if not all(k in d for k in ("free", "origin", "cell")):
            raise ValueError("the scene carries no walkable raster (free / origin / cell): load it with load_scene_file(path, raster=True) "
                             "from a file that scene_from_scan or add_boxes_to_scene made, or pass scene_gen.walkable_grid's result to "
                             "from_raster")
        return cls.from_raster(d["free"], d["origin"], d["cell"], goals, device=device)

    def sample(self, points) -> torch.Tensor:
        """points [F,n,2|3] world -> [F,n]: bilinear over the finite cells around each point, `OFF` where there is none, NaN for a
        NaN coordinate."""
        F, H, W = self.dist.shape
        p = torch.as_tensor(points, dtype=torch.float32).to(self.dist.device)
        if p.dim() != 3 or p.shape[0] != F or p.shape[2] not in (2, 3) or p.shape[1] < 1:
            raise ValueError(f"points must be [{F},n,2] or [{F},n,3], got {tuple(p.shape)}")
        p = p[..., :2].contiguous()
        out = torch.empty(F, p.shape[1], device=p.device)
        with torch.cuda.device(p.device):
            _lib.check(_lib.load().egx_geodesic_sample(_lib.ptr(self.dist), _lib.ptr(self.origin), float(np.float32(self.cell)), F, H, W,
                                                       _lib.ptr(p), p.shape[1], _lib.ptr(out), _lib.current_stream_ptr()),
                       "egx_geodesic_sample")
        return out

    def select_args(self, b: int):
        """The field's arguments of the two *_field selection entries for b sequences (len(self) in {1, b}) and what must outlive
        the launches."""
        F, H, W = self.dist.shape
        index = None if F == 1 else torch.arange(b, device=self.dist.device, dtype=torch.int32)
        return (_lib.ptr(self.dist), _lib.ptr(self.origin), float(np.float32(self.cell)), H, W, F, _lib.ptr(index)), index
