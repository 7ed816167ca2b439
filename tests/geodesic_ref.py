"""The geodesic field (`egogen_amd/geodesic.py`, kernels of csrc/geodesic.hip) and the goal term the selection kernels read from it,
restated on the CPU: the float64 truth and the float32 yardstick of tests/test_geodesic_{cpu,gpu}.py.

  * `seeds`: the seed rule, cell by cell;
  * `dijkstra`: shortest paths over the free cells, 8 neighbours, no diagonal past a blocked axis neighbour, one addition in
    `dtype` per edge.  In float32 it is what the device must give bit for bit: rounding is monotone, so the fixed point of the
    relaxation does not depend on its order;
  * `sample`: the renormalised bilinear read of a field, every operation rounded in `dtype`;
  * `cost`: the cost of a candidate row with the field's value as its goal term, summed in the kernel's order;
  * `serpentine`: the test rasters."""
import heapq

import numpy as np
import torch

OFF = 1.0e4
NEIGHBOURS = ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (-1, 1), (1, -1), (1, 1))


def weights(cell):
    """(w1, w2) as the host passes them: float32(cell), float32(float64(cell) * sqrt(2))"""
    return np.float32(cell), np.float32(np.float64(cell) * np.sqrt(2.0))


def seeds(free, origin, cell, goal):
    """-> (cells [n] flat i * W + j, values [n] float32): every free cell whose centre is within 1.5 * cell of the goal's xy"""
    free = np.asarray(free, bool)
    H, W = free.shape
    cells, values = [], []
    for i in range(H):
        for j in range(W):
            if not free[i, j]:
                continue
            cx, cy = float(origin[0]) + (i + 0.5) * float(cell), float(origin[1]) + (j + 0.5) * float(cell)
            d = np.sqrt((cx - float(goal[0])) ** 2 + (cy - float(goal[1])) ** 2)
            if d <= 1.5 * float(cell):
                cells.append(i * W + j)
                values.append(np.float32(d))
    return np.asarray(cells, np.int64), np.asarray(values, np.float32)


def dijkstra(free, seed_cells, seed_values, w1, w2, dtype=np.float32, hops=False):
    """free [H,W] bool -> dist [H,W] in `dtype` (+inf where blocked or unreachable); with hops=True also the number of cells on the
    path that gave each value."""
    free = np.asarray(free, bool)
    H, W = free.shape
    w1, w2 = dtype(w1), dtype(w2)
    dist = np.full((H, W), np.inf, dtype)
    nh = np.zeros((H, W), np.int64)
    heap = []
    for c, v in zip(np.asarray(seed_cells).tolist(), np.asarray(seed_values).tolist()):
        i, j = divmod(int(c), W)
        v = dtype(v)
        if free[i, j] and v < dist[i, j]:
            dist[i, j], nh[i, j] = v, 1
            heapq.heappush(heap, (float(v), i, j))
    while heap:
        d, i, j = heapq.heappop(heap)
        if d > float(dist[i, j]):
            continue
        for di, dj in NEIGHBOURS:
            a, b = i + di, j + dj
            if a < 0 or a >= H or b < 0 or b >= W or not free[a, b]:
                continue
            if di and dj and not (free[i + di, j] and free[i, j + dj]):
                continue
            nd = dtype(dist[i, j] + (w2 if di and dj else w1))
            if nd < dist[a, b]:
                dist[a, b], nh[a, b] = nd, nh[i, j] + 1
                heapq.heappush(heap, (float(nd), a, b))
    return (dist, nh) if hops else dist


def field(free, origin, cell, goal, dtype=np.float32, hops=False):
    """the field of one goal on one raster by the rules of the issue"""
    c, v = seeds(free, origin, cell, goal)
    w1, w2 = weights(cell)
    return dijkstra(free, c, v, w1, w2, dtype, hops)


def sample(dist, origin, cell, points, dtype=np.float32):
    """dist [H,W], origin [2], points [n,2] -> ([n] in `dtype`, [n] number of finite corners of non-zero weight).  The inputs are
    taken as float32 values (what the device reads) and every operation is rounded in `dtype`."""
    dist = np.asarray(dist, np.float32)
    H, W = dist.shape
    f = dtype
    ox, oy, cell = f(np.float32(origin[0])), f(np.float32(origin[1])), f(np.float32(cell))
    pts = np.asarray(points, np.float32)
    out, cnt = np.zeros(len(pts), dtype), np.zeros(len(pts), np.int64)
    for k, (x, y) in enumerate(pts):
        if np.isnan(x) or np.isnan(y):
            out[k] = np.nan
            continue
        u = f(f(f(x) - ox) / cell) - f(0.5)
        v = f(f(f(y) - oy) / cell) - f(0.5)
        if not (u > -1 and u < H and v > -1 and v < W):
            out[k] = OFF
            continue
        fi, fj = np.floor(u), np.floor(v)
        i0, j0 = int(fi), int(fj)
        a1, b1 = f(u - fi), f(v - fj)
        a0, b0 = f(f(1) - a1), f(f(1) - b1)
        sw, sv = f(0), f(0)
        for c in range(4):
            i, j = i0 + (c >> 1), j0 + (c & 1)
            w = f((a1 if c >> 1 else a0) * (b1 if c & 1 else b0))
            if i < 0 or i >= H or j < 0 or j >= W or not w > 0 or not np.isfinite(dist[i, j]):
                continue
            sw = f(sw + w)
            sv = f(sv + f(w * f(dist[i, j])))
            cnt[k] += 1
        out[k] = f(sv / sw) if sw > 0 else OFF
    return out, cnt


def last_pelvis_world(R0, T0, joints, dtype):
    """R0 [B,3,3], T0 [B,3], joints [B,20,J,3] -> world xy [B,2] of joint 0 of body 19, in `dtype`"""
    c = lambda t: torch.as_tensor(t).detach().cpu().to(dtype)
    R0, T0, j = c(R0).reshape(-1, 3, 3), c(T0).reshape(-1, 3), c(joints)[:, 19, 0]
    return (torch.einsum("bij,bj->bi", R0, j) + T0)[:, :2]


def cost(geo, terms, weights_, dtype):
    """geo [B], terms: dict of [B] tensors (skate, floor, pene, face of tests/genop_search_ref.score) -> cost [B] in `dtype`:
    w_goal*geo + w_skate*skate + w_floor*floor + w_pene*pene + w_face*face, summed in this order"""
    w = lambda k: torch.tensor(weights_[k], dtype=dtype)
    out = w("goal") * torch.as_tensor(geo).to(dtype)
    for k in ("skate", "floor", "pene", "face"):
        out = out + w(k) * terms[k].to(dtype)
    return out


def serpentine(H, W, every=8, gap=3):
    """A blocked border, a wall every `every` rows with a `gap`-cell opening at alternating ends, and a sealed one-cell pocket in
    the last wall -> free [H,W] bool.  A path from the first to the last corridor runs the length of every corridor."""
    free = np.ones((H, W), bool)
    free[0], free[-1], free[:, 0], free[:, -1] = False, False, False, False
    walls = list(range(every, H - 2, every))
    for n, r in enumerate(walls):
        free[r] = False
        if n % 2 == 0:
            free[r, W - 1 - gap:W - 1] = True
        else:
            free[r, 1:1 + gap] = True
    return free


def sealed_pocket(free, i, j):
    """blocks the eight cells round (i, j) and frees (i, j): unreachable from anywhere"""
    free[i - 1:i + 2, j - 1:j + 2] = False
    free[i, j] = True
    return free
