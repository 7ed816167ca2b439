"""The best-of-N primitive search (`GAMMAPrimitiveComboGenOP.generate_sequence_to_goal`, kernels egx_primitive_select and
egx_primitive_advance_select) as plain torch on the CPU, parametrised by dtype: the float64 truth and the float32 yardstick of
tests/test_genop_search_{cpu,gpu}.py.  Built on tests/genop_ref.py (`advance`, and `chain`'s steps).

  * `score`: the cost terms of one candidate row, each the ARGUMENT of a reward term of the reference's `CrowdEnv.step`
    (motion/crowd_ppo/crowd_env_2f.py:171-235), written with the reference's own torch expressions; pinned by the recorded
    rewards of tests/golden/env_step_ref.npz (tests/test_genop_search_cpu.py);
  * `select`: the choice among the N rows of a sequence;
  * `search_chain`: sample_prior -> blend -> SMPL-X -> score -> select -> advance from the winner, primitive after primitive."""
import numpy as np
import torch

from oracle import nets
from oracle.env import blend_params
from oracle.smplx_lbs import smplx_forward
from tests import genop_ref
from tests.genop_ref import T_ALL, T_HIS, T_PRED, _t

TERMS = ("dist", "skate", "floor", "pene", "face")       # the order of cost_terms and of the sum
WEIGHTS = {"goal": 1.0, "skate": 1.0, "floor": 1.0, "pene": 1.0, "face": 0.0}
_W_OF = {"dist": "goal", "skate": "skate", "floor": "floor", "pene": "pene", "face": "face"}


def score(Y_gen, X_seed, joints, markers_proj, R0, T0, pene_count, goal, feet_marker_idx, weights=None, pene_thres=40,
          reproj_factor=0.5, dtype=torch.float32):
    """Y_gen[18,B,201], X_seed[2,B,201], joints[B,20,J,3], markers_proj[B,20,67,3], R0[B,3,3], T0[B,3], pene_count[B,20] int or
    None, goal[B,3] (world, per row) -> dict of [B] tensors: the five terms, `cost` (summed in the order of TERMS, in `dtype`),
    `colliding` (bool)."""
    c = lambda x: _t(x, dtype)
    Yg, X, J, mp, R0, T0, goal = c(Y_gen), c(X_seed), c(joints), c(markers_proj), c(R0).reshape(-1, 3, 3), c(T0).reshape(-1, 3), c(goal)
    B = J.shape[0]
    feet = torch.as_tensor(np.asarray(feet_marker_idx), dtype=torch.long)
    rf = reproj_factor
    pred = torch.cat([X, Yg], dim=0).reshape(T_ALL, B, -1, 3).permute(1, 0, 2, 3)
    mb = rf * mp + (1 - rf) * pred                                                            # :151-152
    h = 1 / 40
    speed = torch.norm(mb[:, 2:] - mb[:, :-2], dim=-1) / 2. / h                               # :183
    skate = (speed[:, :, feet].amin(dim=-1) - 0.075).clamp(min=0).mean(dim=-1)                # :184
    mw = torch.einsum("bij,btpj->btpi", R0, mb) + T0[:, None, None, :]                        # :191-192
    floor = torch.abs(mw[:, :, feet, 2].amin(dim=-1) - 0.02).mean(dim=-1)                     # :193
    if pene_count is None:
        pene = torch.zeros(B, dtype=dtype)
        colliding = torch.zeros(B, dtype=torch.bool)
    else:
        cnt = torch.as_tensor(np.asarray(pene_count.cpu() if torch.is_tensor(pene_count) else pene_count)).reshape(B, T_ALL).long()
        pene = cnt.sum(dim=1).to(dtype) / T_ALL / 10                                          # :174
        colliding = ~(cnt.max(dim=1).values < pene_thres)                                     # :175-176
    je = J[:, -1]                                                                             # :207-213
    x_axis = (je[:, 2] - je[:, 1]).clone()
    x_axis[:, -1] = 0
    x_axis = x_axis / torch.norm(x_axis, dim=-1, keepdim=True).clip(min=1e-12)
    z_axis = torch.tensor([[0, 0, 1]], dtype=dtype).repeat(B, 1)
    b_ori = torch.cross(z_axis, x_axis, dim=-1)[:, :2]
    tl = torch.einsum("bij,bj->bi", R0.permute(0, 2, 1), goal - T0)                           # :215-216
    pelvis = J[:, -1, 0]
    fo = tl[:, :2] - pelvis[:, :2]                                                            # :217-219
    fo = fo / torch.norm(fo, dim=-1, keepdim=True).clip(min=1e-12)
    face = 1 - (torch.einsum("bi,bi->b", fo, b_ori) + 1) / 2.0
    dist = torch.norm(tl - pelvis, dim=-1).clip(min=1e-12)                                    # :232
    out = {"dist": dist, "skate": skate, "floor": floor, "pene": pene, "face": face}
    w = dict(WEIGHTS, **(weights or {}))
    cost = None
    for k in TERMS:
        term = torch.tensor(w[_W_OF[k]], dtype=dtype) * out[k]
        cost = term if cost is None else cost + term
    out.update(cost=cost, colliding=colliding)
    return out


def rank_class(cost, terms, colliding):
    """0 clean, 1 colliding, 2 / 3 the same with a non-finite cost or term; cost[..., N], terms[..., N, 5], colliding[..., N]"""
    finite = torch.isfinite(cost) & torch.isfinite(terms).all(dim=-1)
    return (~finite).long() * 2 + colliding.long()


def select(cost, terms, colliding):
    """cost[b,N], terms[b,N,5], colliding[b,N] -> choice[b], status[b] (bit 0: the chosen row collides, bit 1: every row is
    non-finite).  Order: finite rows first, then non-colliding, then the lower cost, then the lower index."""
    cost, terms, colliding = torch.as_tensor(cost), torch.as_tensor(terms), torch.as_tensor(colliding).bool()
    cls = rank_class(cost, terms, colliding)
    b, N = cost.shape
    choice = torch.zeros(b, dtype=torch.long)
    for i in range(b):
        best = None
        for n in range(N):
            key = (int(cls[i, n]), float(cost[i, n]) if int(cls[i, n]) < 2 else 0.0, n)
            if best is None or key < best:
                best = key
        choice[i] = best[2]
    chosen = cls.gather(1, choice[:, None])[:, 0]
    return choice, (chosen & 1) | (chosen & 2)


def search_chain(sd, bm, marker_ids, feet_marker_idx, X_seed, seed_params, R0, T0, betas, z, goal, N, reproj_factor, weights=None,
                 pene_thres=40, goal_thresh=0.1):
    """K = z.shape[0] primitives of b sequences with N candidates each, no scene, in bm's dtype.  X_seed[b,2,201],
    seed_params[b,2,93], R0[b,3,3], T0[b,3], betas[b,10], z[K,b*N,128] (row i*N + n = candidate n of sequence i), goal[b,3]
    -> list of K dicts: `genop_ref.advance`'s outputs for the b winners plus choice[b], status[b], reached[b], goal_dist[b],
    cost[b,N], terms[b,N,5], pred_params[b,20,93] (winners) and `rows`: what every one of the b*N rows produced."""
    dt = bm.dtype
    sd = genop_ref.cast_state_dict(sd, dt)
    mk = torch.as_tensor(np.asarray(marker_ids), dtype=torch.long)
    rep = lambda x: _t(x, dt).repeat_interleave(N, dim=0)
    X, seed = rep(X_seed).permute(1, 0, 2), rep(seed_params)
    R0, T0, bt, goal_rows = rep(R0).reshape(-1, 3, 3), rep(T0).reshape(-1, 3), rep(betas).reshape(-1, 10), rep(goal)
    z = _t(z, dt)
    BN = bt.shape[0]
    b = BN // N
    dT = genop_ref.delta_T_of(bm, bt)
    out = []
    for k in range(z.shape[0]):
        Y_gen, Yb_gen = nets.sample_prior(sd, X, bt[None].repeat(T_PRED, 1, 1), z[k])
        Yb = blend_params(torch.cat([seed.permute(1, 0, 2), Yb_gen], dim=0).clone(), T_HIS)
        pp = Yb.permute(1, 0, 2).contiguous()
        v, j = smplx_forward(bm, pp.reshape(BN * T_ALL, 93), bt.repeat_interleave(T_ALL, 0))
        joints = j.reshape(BN, T_ALL, -1, 3)
        mproj = v[:, mk].reshape(BN, T_ALL, -1, 3)
        sc = score(Y_gen, X, joints, mproj, R0, T0, None, goal_rows, feet_marker_idx, weights, pene_thres, reproj_factor, dt)
        terms = torch.stack([sc[t] for t in TERMS], dim=-1).reshape(b, N, 5)
        cost = sc["cost"].reshape(b, N)
        choice, status = select(cost, terms, sc["colliding"].reshape(b, N))
        rows = torch.arange(b) * N + choice
        r = genop_ref.advance(pp[rows], Y_gen[:, rows], X[:, rows], joints[rows], mproj[rows], dT[rows], reproj_factor, R0[rows], T0[rows], dt)
        gd = sc["dist"][rows]
        r.update(choice=choice, status=status, reached=gd < goal_thresh, goal_dist=gd, cost=cost, terms=terms, pred_params=pp[rows],
                 Y_gen=Y_gen[:, rows], joints=joints[rows], markers_proj=mproj[rows],
                 rows={"Y_gen": Y_gen, "X": X, "joints": joints, "markers_proj": mproj, "R0": R0, "T0": T0, "pred_params": pp})
        out.append(r)
        X = r["seed_markers"].repeat_interleave(N, dim=0).permute(1, 0, 2)
        seed, R0, T0 = r["seed_params"].repeat_interleave(N, dim=0), r["R0"].repeat_interleave(N, dim=0), r["T0"].repeat_interleave(N, dim=0)
    return out
