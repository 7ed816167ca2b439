"""numpy restatement, in a given dtype, of the route rule of csrc/genop_route.hip (egx_route_advance: `advance`, and `replay` over
the records of a returned `PrimitiveSequence`) and of egx_route_metrics (csrc/motion_metrics.hip: `route_metrics`).  Every
operation rounds in `dtype`; the float32 restatement has no fused multiply-add, which the kernel has - the yardstick of the tests
is the float32 restatement's error against float64, and the kernel's may not exceed 3 x that.

Besides the outputs every function returns `slack`: the least |h - pass_radius|, computed in float64, over the distances that
decided something (the frames from the search start on, for every waypoint the rule looked at).  A discrete outcome is compared
exactly only where the slack says that float32 round-off cannot have changed it."""
import numpy as np

T_ALL, T_HIS = 20, 2


def world_xy(pelvis, R, T, dtype):
    """pelvis [...,20,3], R [...,3,3], T [...,3] -> world x, y [...,20] with the kernel's order: ((R0 p0 + R1 p1) + R2 p2) + T"""
    p, R, T = np.asarray(pelvis, dtype), np.asarray(R, dtype), np.asarray(T, dtype)
    row = lambda i: ((R[..., None, i, 0] * p[..., 0] + R[..., None, i, 1] * p[..., 1]) + R[..., None, i, 2] * p[..., 2]) + T[..., None, i]
    return row(0), row(1)


def _h(x, y, w, dtype):
    dx, dy = x - dtype(w[0]), y - dtype(w[1])
    return np.sqrt(dx * dx + dy * dy)


def _walk(x, y, way, n, c, radius, dtype):
    """the ordered cascade over the frames x, y [F] from cursor c of n live waypoints -> (cursor, first frames of the passes, slack)"""
    f0, frames, slack = 0, [], np.inf
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    while c < n - 1:
        h = _h(x, y, way[c], dtype)
        if len(h) > f0:
            slack = min(slack, float(np.abs(_h(x64, y64, way[c], np.float64)[f0:] - radius).min()))
        hit = np.flatnonzero((h < dtype(radius)) & (np.arange(len(h)) >= f0))
        if len(hit) == 0:
            break
        f0 = int(hit[0])
        frames.append(f0)
        c += 1
    return c, frames, slack


def advance(pelvis, R, T, waypoints, count, cursor, radius, dtype, reached=None, field_of=None):
    """One launch of egx_route_advance on b sequences: pelvis [b,20,3], R [b,3,3], T [b,3], waypoints [b,P,3], count [b], cursor [b]
    -> dict: cursor [b] after, route_goal [b,3], goal [b,3], pass_dist [b], reached [b] (with `reached`), field_index [b] (with
    `field_of`), slack [b]."""
    dtype = np.dtype(dtype).type
    way = np.asarray(waypoints, np.float32)
    b, P = way.shape[:2]
    x, y = world_xy(pelvis, R, T, dtype)
    x, y = x[:, T_HIS:], y[:, T_HIS:]
    out = {"cursor": np.zeros(b, np.int32), "route_goal": np.zeros((b, 3), np.float32), "goal": np.zeros((b, 3), np.float32),
           "pass_dist": np.zeros(b, dtype), "slack": np.full(b, np.inf)}
    if reached is not None:
        out["reached"] = np.asarray(reached, np.int32).copy()
    for g in range(b):
        n = int(min(max(int(count[g]), 1), P))
        c0 = int(min(max(int(cursor[g]), 0), n - 1))
        c = c0
        if np.isnan(x[g]).any() or np.isnan(y[g]).any():
            out["pass_dist"][g] = np.nan
        else:
            out["pass_dist"][g] = _h(x[g], y[g], way[g, c0], dtype).min()
            c, _, out["slack"][g] = _walk(x[g], y[g], way[g], n, c0, radius, dtype)
        out["cursor"][g], out["route_goal"][g], out["goal"][g] = c, way[g, c0], way[g, c]
        if reached is not None and c0 != n - 1:
            out["reached"][g] = 0
    if field_of is not None:
        out["field_index"] = np.asarray(field_of, np.int32)[np.arange(b), out["cursor"]]
    return out


def replay(pelvis, rotmat, transl, waypoints, count, radius, dtype):
    """The cursor trace of a whole search from its records: pelvis [K,b,20,3], rotmat [K,b,3,3], transl [K,b,3] -> dict of
    cursor [K,b] (after each primitive), route_goal [K,b,3], pass_dist [K,b], slack [K,b]"""
    K, b = np.asarray(pelvis).shape[:2]
    cur = np.zeros(b, np.int32)
    keys = ("cursor", "route_goal", "pass_dist", "slack")
    trace = {k: [] for k in keys}
    for k in range(K):
        o = advance(np.asarray(pelvis)[k], np.asarray(rotmat)[k], np.asarray(transl)[k], waypoints, count, cur, radius, dtype)
        cur = o["cursor"]
        for key in keys:
            trace[key].append(o[key])
    return {k: np.stack(v) for k, v in trace.items()}


def route_metrics(ms, radius, dtype=np.float64, P=16):
    """egx_route_metrics over a `MotionSet` -> dict of pass_frame [n,P] int32, approach_min [n,P], waypoints_passed [n] int32,
    slack [n] (over the distances that decided a pass)"""
    dtype = np.dtype(dtype).type
    n = len(ms)
    x, y = world_xy(ms.pelvis, ms.rotmat, ms.transl, dtype)
    x, y = x.reshape(-1), y.reshape(-1)
    out = {"pass_frame": np.full((n, P), -1, np.int32), "approach_min": np.full((n, P), np.nan, dtype), "waypoints_passed": np.zeros(n, np.int32),
           "slack": np.full(n, np.inf)}
    for i in range(n):
        r = None if ms.routes is None else ms.routes[i]
        if r is None:
            continue
        src = ms.frame_src[ms.motion_start[i]:ms.motion_start[i + 1]]
        xi, yi, start = x[src], y[src], 0
        for j in range(len(r)):
            h = _h(xi, yi, r[j], dtype)[start:]
            out["approach_min"][i, j] = h.min()
            if j == len(r) - 1:
                break
            h64 = _h(xi.astype(np.float64), yi.astype(np.float64), r[j], np.float64)[start:]
            out["slack"][i] = min(out["slack"][i], float(np.abs(h64 - radius).min()))
            hit = np.flatnonzero(h < dtype(radius))
            if len(hit) == 0:
                break
            start += int(hit[0])
            out["pass_frame"][i, j] = start
            out["waypoints_passed"][i] += 1
    return out


# ---- constructed cases of the entry tests -------------------------------------------------------------------------------------
CASE_RADIUS, CASE_STEP = 0.12, 0.12
KINDS = ("single", "pass", "cascade", "same_frame", "wrong_order", "seed_only", "on_last", "reached_cleared", "nan", "sixteen",
         "sixteen_from7", "clamped")


def constructed(kinds, seed, P=16):
    """One hand-made sequence per entry of `kinds`: a walker on a straight line, CASE_STEP metres per frame, in a world frame of its
    own (a yaw and an offset of some metres), and waypoints at m(a), the point half way between frames a and a + 1: its distance to
    the frames is 0.06, 0.18, 0.30 ..., so with CASE_RADIUS = 0.12 it is first within the radius at frame a, and every distance
    stays 0.06 m from the radius (the tests assert the slack).  `far` is 70 m off.  -> dict of the entry's inputs (float32 / int32
    numpy), and `want_cursor`, `want_reached`: the outcome by construction."""
    g = np.random.default_rng(seed)
    b = len(kinds)
    yaw, T = g.normal(size=b) * 2.0, (g.normal(size=(b, 3)) * 2.0).astype(np.float32)
    R = np.zeros((b, 3, 3), np.float32)
    R[:, 0, 0], R[:, 0, 1], R[:, 1, 0], R[:, 1, 1], R[:, 2, 2] = np.cos(yaw), -np.sin(yaw), np.sin(yaw), np.cos(yaw), 1.0
    pelvis = np.zeros((b, T_ALL, 3), np.float32)
    pelvis[:, :, 1], pelvis[:, :, 2] = (np.arange(T_ALL) * CASE_STEP).astype(np.float32), 0.9
    x, y = world_xy(pelvis, R, T, np.float64)
    q = np.stack([x, y, np.full_like(x, 0.9)], -1)                        # [b,20,3] float64
    way, count, cursor = np.zeros((b, P, 3), np.float32), np.zeros(b, np.int32), np.zeros(b, np.int32)
    reached, want_cursor, want_reached = np.zeros(b, np.int32), np.zeros(b, np.int32), np.zeros(b, np.int32)
    for i, kind in enumerate(kinds):
        m = lambda a: (q[i, a] + q[i, a + 1]) / 2
        far = q[i, 0] + np.array([50.0, 50.0, 0.0])
        pts, cur, r_in, c_out, r_out, n = {
            "single": ([m(5)], 0, 1, 0, 1, None),
            "pass": ([m(5), far], 0, 0, 1, 0, None),
            "cascade": ([m(5), m(9), far], 0, 0, 2, 0, None),
            "same_frame": ([m(5), m(5), far], 0, 0, 2, 0, None),
            "wrong_order": ([m(12), m(4), far], 0, 0, 1, 0, None),
            "seed_only": ([m(0), far], 0, 1, 0, 0, None),
            "on_last": ([far, far, m(5)], 2, 1, 2, 1, None),
            "reached_cleared": ([m(17), far], 0, 1, 1, 0, None),
            "nan": ([m(5), far], 0, 1, 0, 0, None),
            "sixteen": ([m(a) for a in range(2, 17)] + [far], 0, 0, 15, 0, None),
            "sixteen_from7": ([m(a) for a in range(2, 17)] + [far], 7, 0, 15, 0, None),
            "clamped": ([m(2)] + [far] * 15, -2, 0, 1, 0, 40),              # count 40 is 16, cursor -2 is 0
        }[kind]
        way[i, :len(pts)] = np.asarray(pts)
        count[i], cursor[i], reached[i], want_cursor[i], want_reached[i] = len(pts) if n is None else n, cur, r_in, c_out, r_out
        if kind == "nan":
            pelvis[i, 7, 1] = np.nan
    return {"pelvis": pelvis, "R": R, "T": T, "waypoints": way, "count": count, "cursor": cursor, "reached": reached, "radius": CASE_RADIUS,
            "field_of": g.integers(0, 9, size=(b, P)).astype(np.int32), "want_cursor": want_cursor, "want_reached": want_reached,
            "kinds": list(kinds)}
