"""Restatement of the two launches of csrc/genop_policy.hip in torch / numpy, in float64 (the truth of the `held()` rule) and in
float32 (its yardstick), built from the oracle's pieces: `oracle.env.calc_egosensing` (the rays), `oracle.env.get_feature` (the marker
-> target directions and the clipped target distance); the proposal's arithmetic is ppo_policy.py:169-178 as oracle/ppo.py states
it.  Also the synthetic inputs the CPU and the GPU tests share: they need no body model, the kernel reads numbers.  A plain module."""
import numpy as np
import torch

from egogen_amd import synth
from oracle.env import calc_egosensing, get_feature, points_in_rings
from oracle.ppo import action_dist

EGO_FLOOR = 3.6e-4          # tests/test_env_gpu.py `_FLOOR_FIXED["ego"]`, tests/test_env_reference_goldens.py `FLOOR["ego"]`
SHIFT = 1e-5                # metres: a ray whose float64 value moves by more than the floor under this shift of the eye is undecidable
B = 3
EYE = (23, 24, 56, 57)


def square_hole_edges():
    """The walkable polygon of `synth.make_sdf_scene`: the room's rectangle with the box as a hole (8 edges)."""
    return synth.rings_to_edges(synth.sdf_scene_polygon(synth.make_sdf_scene(8))).astype(np.float32)


def room0_edges():
    return synth.rings_to_edges(synth.room0_polygon()).astype(np.float32)


GON_EDGES, GON_RADIUS = 1200, 6.0


def gon_edges():
    """A regular GON_EDGES-gon of GON_RADIUS metres about the origin: more edges than the 1024 the observe kernel stages in LDS, so it
    reads them from global memory; every eye position of the cases (at most 5.2 m from the origin) lies inside it, walls in reach."""
    a = 2.0 * np.pi * np.arange(GON_EDGES) / GON_EDGES
    ring = GON_RADIUS * np.stack([np.cos(a), np.sin(a)], 1)
    return synth.rings_to_edges([np.concatenate([ring, ring[:1]])]).astype(np.float32)


def polygon(kind):
    """-> (edges [E,4] float32, edge_off [S+1] int32, scene_idx [B] int32, world xy of the B eyes) or None for no polygon.
    'square': one scene, sequence 2 starts outside it; 'two': scene 0 the square, scene 1 room0 (6 rings, 89 edges), the sequences in
    scenes 1, 0, 1; 'gon1200': one scene, `gon_edges`, the square's eye positions, all of them inside."""
    if kind == "none":
        return None
    if kind == "gon1200":
        gon = gon_edges()
        return gon, np.array([0, len(gon)], np.int32), np.zeros(B, np.int32), np.array([[-1.0, -1.2], [2.6, 2.1], [5.0, 0.3]])
    sq = square_hole_edges()
    if kind == "square":
        return sq, np.array([0, len(sq)], np.int32), np.zeros(B, np.int32), np.array([[-1.0, -1.2], [2.6, 2.1], [5.0, 0.3]])
    r0 = room0_edges()
    assert r0.shape == (89, 4)
    rng = np.random.default_rng(0)
    lo, hi = r0[:, :2].min(0), r0[:, :2].max(0)
    pts = rng.uniform(lo, hi, (64, 2))
    inside = pts[points_in_rings(r0.astype(np.float64), pts[:, 0], pts[:, 1])]
    return (np.concatenate([sq, r0]), np.array([0, len(sq), len(sq) + len(r0)], np.int32), np.array([1, 0, 1], np.int32),
            np.stack([inside[0], [-2.0, 1.5], inside[1]]))


def observe_inputs(N, frames_per_row, first, eyes_xy, seed=0):
    """Everything egx_primitive_observe reads for B sequences of N rows, as float32 CPU tensors.  The eye joints of the chosen
    rows' seed bodies stand at `eyes_xy` in the world (the origin without); every other row holds other numbers, and the rows
    i * N + n, n > 0, of R0 / T0 / x0 / x1 hold NaN: the launch reads row i * N.  choice: the first row, the last row, out of range."""
    g = torch.Generator().manual_seed(1000 + 17 * N + frames_per_row + seed)
    rows = B * N
    J = torch.randn(rows, frames_per_row, 127, 3, generator=g) * 0.3 + torch.tensor([0.0, 0.0, 1.0])
    # a head: eyes 6 cm apart about the local origin, joints 56 / 57 ahead of them in a direction of the row's own
    ang = torch.rand(rows, frames_per_row, generator=g) * 6.28
    fwd = torch.stack([torch.cos(ang), torch.sin(ang), torch.zeros_like(ang)], -1) * 0.1
    side = torch.stack([-torch.sin(ang), torch.cos(ang), torch.zeros_like(ang)], -1) * 0.03
    centre = torch.randn(rows, frames_per_row, 3, generator=g) * torch.tensor([0.05, 0.05, 0.0]) + torch.tensor([0.0, 0.0, 1.6])
    J[:, :, 23], J[:, :, 24] = centre - side, centre + side
    J[:, :, 56], J[:, :, 57] = centre - side + fwd, centre + side + fwd
    choice = torch.tensor([0, N - 1, N + 3], dtype=torch.int32)
    yaw = torch.randn(B, generator=g) * 2.0
    R_prev = torch.zeros(B, 3, 3)
    R_prev[:, 0, 0], R_prev[:, 0, 1], R_prev[:, 1, 0], R_prev[:, 1, 1], R_prev[:, 2, 2] = torch.cos(yaw), -torch.sin(yaw), torch.sin(yaw), torch.cos(yaw), 1.0
    T_prev = torch.zeros(B, 3)
    if eyes_xy is not None:
        T_prev[:, :2] = torch.as_tensor(eyes_xy, dtype=torch.float32)
    T_prev[:, 2] = torch.randn(B, generator=g) * 0.02
    yaw = torch.randn(B, generator=g) * 2.0
    R0 = torch.full((rows, 3, 3), float("nan"))
    T0 = torch.full((rows, 3), float("nan"))
    Rn = torch.zeros(B, 3, 3)
    Rn[:, 0, 0], Rn[:, 0, 1], Rn[:, 1, 0], Rn[:, 1, 1], Rn[:, 2, 2] = torch.cos(yaw), -torch.sin(yaw), torch.sin(yaw), torch.cos(yaw), 1.0
    R0[::N], T0[::N] = Rn, T_prev + torch.randn(B, 3, generator=g) * torch.tensor([0.3, 0.3, 0.02])
    x = torch.full((2, rows, 201), float("nan"))
    x[:, ::N] = torch.randn(2, B, 201, generator=g) * 0.4
    goal = T_prev + torch.randn(B, 3, generator=g) * torch.tensor([2.0, 2.0, 0.0]) + torch.tensor([0.0, 0.0, 0.9])
    return {"joints": J.reshape(rows * frames_per_row, 127, 3).contiguous(), "choice": choice, "R_prev": R_prev, "T_prev": T_prev, "R0": R0,
            "T0": T0, "x0": x[0].contiguous(), "x1": x[1].contiguous(), "goal": goal, "N": N, "frames_per_row": frames_per_row, "first": first}


def seed_bodies(d):
    """The joints [B,2,127,3] of the two seed bodies the launch reads: frames first, first + 1 of row i * N + clamp(choice[i])."""
    N, fpr = d["N"], d["frames_per_row"]
    J = d["joints"].reshape(B * N, fpr, 127, 3)
    rows = torch.arange(B) * N + d["choice"].long().clamp(0, N - 1)
    return J[rows, d["first"]:d["first"] + 2]


def observe(j2, R_prev, T_prev, R0, T0, x0, x1, goal, poly, ray_len, step, max_depth, dtype, eye_shift=(0.0, 0.0)):
    """-> state [b,2,402], egosensing [b,2,32], dist [b], time [b] in `dtype` arithmetic.  j2 [b,2,127,3] the seed bodies in the frame
    (R_prev, T_prev); R0 [b,3,3] / T0 [b,3] the new frame, x0 / x1 [b,201] the new seed frames; poly: None or (edges, edge_off,
    scene_idx).  eye_shift: added to the world xy of every joint before the rays are cast (the undecidable test)."""
    c = lambda t: torch.as_tensor(t).to(dtype)
    j2, R_prev, T_prev, R0, T0, x0, x1, goal = (c(t) for t in (j2, R_prev, T_prev, R0, T0, x0, x1, goal))
    b = j2.shape[0]
    Y = torch.stack([x0, x1], 1)                                        # [b,2,201]
    pel = j2[:, :, 0]                                                   # in the frame the joints are expressed in
    fea = get_feature(Y, pel, R0, T0[:, None], goal[:, None])[3]        # marker -> target, target in the NEW frame
    state = torch.cat([Y, fea], -1)
    d = get_feature(Y, pel, R_prev, T_prev[:, None], goal[:, None])[1][:, 1, 0]     # the second seed body's pelvis, the joints' frame
    dist = 1.0 / (d + 1.0)
    time = (1.0 - torch.tensor(float(min(int(step), int(max_depth))), dtype=dtype) / torch.tensor(float(max_depth), dtype=dtype)).expand(b).clone()
    ego = torch.ones(b, 2, 32, dtype=torch.float32)
    if poly is not None:
        edges, off, idx = poly
        jw = torch.einsum("bij,btkj->btki", R_prev, j2) + T_prev[:, None, None]
        jw = jw + torch.tensor([eye_shift[0], eye_shift[1], 0.0], dtype=dtype)
        for i in range(b):
            e = np.asarray(edges, np.float64)[off[idx[i]]:off[idx[i] + 1]]
            ego[i] = calc_egosensing(jw[i], e, ray_len)
    return state, ego, dist, time


def observe_case(d, poly, ray_len, step, max_depth, dtype, eye_shift=(0.0, 0.0)):
    N = d["N"]
    return observe(seed_bodies(d), d["R_prev"], d["T_prev"], d["R0"][::N], d["T0"][::N], d["x0"][::N], d["x1"][::N], d["goal"],
                   None if poly is None else poly[:3], ray_len, step, max_depth, dtype, eye_shift)


def undecidable(d, poly, ray_len):
    """bool [b,2,32]: the float64 value of the ray moves by more than EGO_FLOOR when the eye is shifted by SHIFT along +-x or +-y."""
    base = observe_case(d, poly, ray_len, 0, 1, torch.float64)[1].double()
    out = torch.zeros_like(base, dtype=torch.bool)
    for sx, sy in ((SHIFT, 0.0), (-SHIFT, 0.0), (0.0, SHIFT), (0.0, -SHIFT)):
        out |= (observe_case(d, poly, ray_len, 0, 1, torch.float64, (sx, sy))[1].double() - base).abs() > EGO_FLOOR
    return out


OBSERVE_CASES = [(kind, N, mode) for kind in ("none", "square", "two") for N in (1, 5) for mode in ((20, 18), (2, 0))]
OBSERVE_CASES.append(("gon1200", 5, (20, 18)))          # the branch of a scene too large for LDS


def propose(mu, logvar, eps, min_logvar, max_logvar, N, n_mean, n_policy, temperature, dtype):
    """z [b*N,128]: rows < n_mean are mu, rows in [n_mean, n_policy) mu + temperature * exp(clamp(logvar))^0.5 * eps, the rest eps."""
    mu, logvar, eps = (torch.as_tensor(t).to(dtype) for t in (mu, logvar, eps))
    b = mu.shape[0]
    sigma = action_dist(mu, logvar, min_logvar, max_logvar)[1]
    e = eps.reshape(b, N, 128)
    z = mu[:, None] + (torch.tensor(temperature, dtype=dtype) * sigma)[:, None] * e
    n = torch.arange(N)[None, :, None]
    z = torch.where(n < n_mean, mu[:, None].expand_as(z), z)
    z = torch.where(n >= n_policy, e, z)
    return z.reshape(b * N, 128)


def propose_inputs(N, seed=0):
    """mu, logvar [B,128], eps [B*N,128]; logvar row 0 lies wholly below -2.5, row 1 wholly above 2.5, row 2 straddles both."""
    g = torch.Generator().manual_seed(77 + N + seed)
    mu = torch.randn(B, 128, generator=g)
    logvar = torch.randn(B, 128, generator=g) * 3.0
    logvar[0] = -2.5 - torch.rand(128, generator=g) * 3.0 - 0.01
    logvar[1] = 2.5 + torch.rand(128, generator=g) * 3.0 + 0.01
    return mu, logvar, torch.randn(B * N, 128, generator=g)
