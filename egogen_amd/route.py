"""`Routes`: an itinerary per sequence for `GAMMAPrimitiveComboGenOP.generate_sequence_to_goal(route=)` - "from here via the door
and round the table to the sofa".  A route is an ordered list of 1 to 16 world points; the search steers to the current one, and
once per primitive the entry egx_route_advance (csrc/genop_route.hip) moves a per-sequence cursor past every waypoint the chosen
primitive came within `pass_radius` of, in order.  The last waypoint is the goal proper: it is arrived at by the selection's own
test (3-D, last frame, goal_thresh), never passed.

This object is the host half: built and checked before any device work, it needs no device.  `to(device)` makes the device copies
once.

`pass_radius` = 0.5 m is a stated choice, like the search's other defaults: about what one primitive covers at walking pace (18
frames at 40 per second and 1.2 m/s is 0.54 m), so a walker that heads straight over a waypoint passes it in the primitive that
gets there.  Nobody has measured motion quality with it."""
from __future__ import annotations

import numpy as np
import torch

MAX_WAYPOINTS = 16          # EGX_MAX_WAYPOINTS of include/egogen_hip.h
PASS_RADIUS = 0.5


class Routes:
    """b routes.  waypoints [b,P,3] float32, padded with zeros behind the live ones; count [b] int32 with 1 <= count <= P <= 16;
    pass_radius in metres (horizontal).  ValueError for an empty route, a non-finite live waypoint, more than 16 waypoints, a
    negative or non-finite radius, shapes that disagree.  `len()` is b."""

    def __init__(self, waypoints, count, pass_radius: float = PASS_RADIUS):
        as_np = lambda x: np.asarray(x.detach().cpu() if torch.is_tensor(x) else x)
        w, n = as_np(waypoints), as_np(count)
        if w.ndim != 3 or w.shape[2] != 3 or w.shape[0] < 1:
            raise ValueError(f"waypoints must be [b,P,3], got {tuple(w.shape)}")
        b, P = w.shape[:2]
        if n.ndim != 1 or n.shape[0] != b or (n.astype(np.int64) != n).any():
            raise ValueError(f"count must hold {b} integers, one per route, got shape {tuple(n.shape)}")
        n = n.astype(np.int64)
        if (n < 1).any():
            raise ValueError(f"an empty route: every route needs at least one waypoint, got counts {n.tolist()}")
        if P > MAX_WAYPOINTS or (n > MAX_WAYPOINTS).any():
            raise ValueError(f"a route holds at most {MAX_WAYPOINTS} waypoints, got {max(P, int(n.max()))}")
        if (n > P).any():
            raise ValueError(f"count must not exceed the padded length {P}, got {n.tolist()}")
        live = np.arange(P)[None, :] < n[:, None]
        w = np.where(live[..., None], w.astype(np.float64), 0.0)
        if not np.isfinite(w).all():
            raise ValueError("a live waypoint is not finite")
        r = float(pass_radius)
        if not (r >= 0 and np.isfinite(r)):
            raise ValueError(f"pass_radius must be finite and not negative, got {pass_radius}")
        self.waypoints = np.ascontiguousarray(w, np.float32)
        self.count = np.ascontiguousarray(n, np.int32)
        self.pass_radius = r
        # the distinct live waypoints in order of first appearance, and where each live waypoint stands in that list
        seen, goals = {}, []
        self.field_of = np.zeros((b, P), np.int32)
        for i in range(b):
            for j in range(int(n[i])):
                key = self.waypoints[i, j].tobytes()
                if key not in seen:
                    seen[key] = len(goals)
                    goals.append(self.waypoints[i, j])
                self.field_of[i, j] = seen[key]
        self._field_goals = np.stack(goals).astype(np.float32)
        self._dev = None

    @classmethod
    def from_lists(cls, routes, pass_radius: float = PASS_RADIUS) -> "Routes":
        """routes: a list of [n_i,3] point lists (numpy, torch or nested lists), one per sequence"""
        routes = list(routes)
        if not routes:
            raise ValueError("no route given")
        pts = []
        for i, r in enumerate(routes):
            a = np.asarray(r.detach().cpu() if torch.is_tensor(r) else r, np.float64)
            if a.size == 0:
                raise ValueError(f"route {i} is empty: every route needs at least one waypoint")
            if a.ndim != 2 or a.shape[1] != 3:
                raise ValueError(f"route {i} must be [n,3], got {tuple(a.shape)}")
            if a.shape[0] > MAX_WAYPOINTS:
                raise ValueError(f"a route holds at most {MAX_WAYPOINTS} waypoints, route {i} has {a.shape[0]}")
            pts.append(a)
        P = max(a.shape[0] for a in pts)
        w = np.zeros((len(pts), P, 3))
        for i, a in enumerate(pts):
            w[i, :a.shape[0]] = a
        return cls(w, [a.shape[0] for a in pts], pass_radius)

    def __len__(self):
        return self.waypoints.shape[0]

    def last(self) -> np.ndarray:
        """[b,3] float32: the final waypoint of every route, the goal proper"""
        return self.waypoints[np.arange(len(self)), self.count - 1].copy()

    def lists(self) -> list:
        """the live waypoints of every route: a list of [n_i,3] float32"""
        return [self.waypoints[i, :int(self.count[i])].copy() for i in range(len(self))]

    def field_goals(self) -> np.ndarray:
        """[F,3] float32: the distinct live waypoints in order of first appearance - what the `GeodesicField` of the routes is built
        over (`GeodesicField.from_scene(d, routes.field_goals())`); `field_of [b,P]` int32 is the position of every live waypoint in
        this list, 0 on padding."""
        return self._field_goals.copy()

    def to(self, device) -> dict:
        """waypoints, count and field_of on `device` (made once per device) -> dict of tensors"""
        device = torch.device(device)
        if self._dev is None or self._dev["device"] != device:
            t = lambda a: torch.from_numpy(a).to(device).contiguous()
            self._dev = {"device": device, "waypoints": t(self.waypoints), "count": t(self.count), "field_of": t(self.field_of)}
        return self._dev
