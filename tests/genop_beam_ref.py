"""The beam search over motion primitives (`GAMMAPrimitiveComboGenOP.generate_sequence_to_goal(..., beam_width=W)`, kernels
egx_primitive_beam_select, egx_primitive_advance_beam and egx_beam_backtrack) as plain torch on the CPU, parametrised by dtype: the
float64 truth and the float32 yardstick of tests/test_genop_beam_{cpu,gpu}.py.  Built on tests/genop_search_ref.py (`score`) and
tests/genop_ref.py (`advance`).

Per sequence i there are W slots; at depth k slot s expands into N candidates, row (i * W + s) * N + n being candidate n of slot s.
  * `beam_select`: the W rows of a sequence with the smallest path keys (nonfinite, ncoll[s] + colliding, acc[s] + cost, row);
  * `backtrack`: the slots of the path that ends in slot 0 of the last depth;
  * `beam_chain`: sample_prior -> blend -> SMPL-X -> score -> beam_select -> advance from every kept row, depth after depth, then
    the records of the returned path."""
import numpy as np
import torch

from oracle import nets
from oracle.env import blend_params
from oracle.smplx_lbs import smplx_forward
from tests import genop_ref
from tests import genop_search_ref as sref
from tests.genop_ref import T_ALL, T_HIS, T_PRED, _t

Q_TERMS = ("skate", "floor", "pene", "face")        # q: the cost without its goal term, summed in this order


def q_of(terms, weights=None):
    """terms[..., 5] (dist, skate, floor, pene, face) -> q[...] = w_skate skate + w_floor floor + w_pene pene + w_face face in the
    dtype of `terms`, accumulated on its own (not cost - w_goal dist)."""
    terms = torch.as_tensor(terms)
    w = dict(sref.WEIGHTS, **(weights or {}))
    q = None
    for k in Q_TERMS:
        t = torch.tensor(w[k], dtype=terms.dtype) * terms[..., sref.TERMS.index(k)]
        q = t if q is None else q + t
    return q


def path_keys(cost, terms, colliding, acc, ncoll, W, N):
    """cost[b,W*N], terms[b,W*N,5], colliding[b,W*N], acc[b,W], ncoll[b,W] -> nonfinite[b,W*N] (bool), nc[b,W*N] (long),
    path[b,W*N] (acc[s] + cost; 0 where nonfinite).  A row is nonfinite when its cost, a term or acc[s] + cost is not finite."""
    cost, terms, colliding = torch.as_tensor(cost), torch.as_tensor(terms), torch.as_tensor(colliding).bool()
    acc, ncoll = torch.as_tensor(acc).to(cost.dtype), torch.as_tensor(ncoll).long()
    b, M = cost.shape
    assert M == W * N and acc.shape == (b, W) and ncoll.shape == (b, W)
    row_ok = torch.isfinite(cost) & torch.isfinite(terms).all(dim=-1)
    path = acc.repeat_interleave(N, dim=1) + torch.where(row_ok, cost, torch.zeros_like(cost))
    ok = row_ok & torch.isfinite(path)
    nc = ncoll.repeat_interleave(N, dim=1) + colliding.long()
    return ~ok, nc, torch.where(ok, path, torch.zeros_like(path))


def beam_select(cost, terms, colliding, acc, ncoll, W, N, weights=None):
    """-> dict of [b,W] tensors: beam_row (row within the sequence's W*N), parent, acc (acc[parent] + q), ncoll, path_cost, status
    (bit 0: the node collides, bit 1: the row is nonfinite); slot 0 holds the smallest key."""
    cost, terms, colliding = torch.as_tensor(cost), torch.as_tensor(terms), torch.as_tensor(colliding).bool()
    acc = torch.as_tensor(acc).to(cost.dtype)
    nonfinite, nc, path = path_keys(cost, terms, colliding, acc, ncoll, W, N)
    q = q_of(terms, weights)
    b, M = cost.shape
    beam_row = torch.zeros(b, W, dtype=torch.long)
    for i in range(b):
        keys = sorted((int(nonfinite[i, r]), int(nc[i, r]), float(path[i, r]), r) for r in range(M))
        beam_row[i] = torch.tensor([k[3] for k in keys[:W]])
    parent = beam_row // N
    pick = lambda t: t.gather(1, beam_row)
    return {"beam_row": beam_row, "parent": parent, "acc": acc.gather(1, parent) + pick(q), "ncoll": pick(nc), "path_cost": pick(path),
            "status": pick(colliding.long()) | (pick(nonfinite.long()) << 1)}


def backtrack(parent, K):
    """parent[K,b,W] -> path_slot[K,b]: slot 0 at depth K - 1, then parent by parent down to depth 0"""
    parent = torch.as_tensor(parent).long()
    assert parent.shape[0] == K
    b = parent.shape[1]
    slot = torch.zeros(K, b, dtype=torch.long)
    for k in range(K - 2, -1, -1):
        slot[k] = parent[k + 1].gather(1, slot[k + 1][:, None])[:, 0]
    return slot


def beam_chain(sd, bm, marker_ids, feet_marker_idx, X_seed, seed_params, R0, T0, betas, z, goal, W, N, reproj_factor, weights=None,
               pene_thres=40, goal_thresh=0.1):
    """K = z.shape[0] depths of b sequences with W slots of N candidates each, no scene, in bm's dtype.  X_seed[b,2,201],
    seed_params[b,2,93], R0[b,3,3], T0[b,3], betas[b,10], z[K,b*W*N,128], goal[b,3] -> (steps, path): `steps` a list of K dicts with
    `genop_ref.advance`'s outputs for the b*W kept rows (slot-major within a sequence) plus `beam_select`'s outputs, cost[b,W*N],
    terms[b,W*N,5], acc_in / ncoll_in [b,W], goal_dist / reached [b,W], pred_params[b*W,20,93]; `path` a list of K dicts with the
    records of the returned path: marker_b, pelvis, R, T, pred_params, choice, status, goal_dist, reached, slot (all [b,...])."""
    dt = bm.dtype
    sd = genop_ref.cast_state_dict(sd, dt)
    mk = torch.as_tensor(np.asarray(marker_ids), dtype=torch.long)
    M = W * N
    rep = lambda x, n=M: _t(x, dt).repeat_interleave(n, dim=0)
    X, seed = rep(X_seed).permute(1, 0, 2), rep(seed_params)
    R0, T0, bt, goal_rows = rep(R0).reshape(-1, 3, 3), rep(T0).reshape(-1, 3), rep(betas).reshape(-1, 10), rep(goal)
    z = _t(z, dt)
    BN = bt.shape[0]
    b = BN // M
    dT = genop_ref.delta_T_of(bm, bt)
    acc, ncoll = torch.zeros(b, W, dtype=dt), torch.zeros(b, W, dtype=torch.long)
    steps = []
    for k in range(z.shape[0]):
        Y_gen, Yb_gen = nets.sample_prior(sd, X, bt[None].repeat(T_PRED, 1, 1), z[k])
        Yb = blend_params(torch.cat([seed.permute(1, 0, 2), Yb_gen], dim=0).clone(), T_HIS)
        pp = Yb.permute(1, 0, 2).contiguous()
        v, j = smplx_forward(bm, pp.reshape(BN * T_ALL, 93), bt.repeat_interleave(T_ALL, 0))
        joints = j.reshape(BN, T_ALL, -1, 3)
        mproj = v[:, mk].reshape(BN, T_ALL, -1, 3)
        sc = sref.score(Y_gen, X, joints, mproj, R0, T0, None, goal_rows, feet_marker_idx, weights, pene_thres, reproj_factor, dt)
        terms = torch.stack([sc[t] for t in sref.TERMS], dim=-1).reshape(b, M, 5)
        cost = sc["cost"].reshape(b, M)
        sel = beam_select(cost, terms, sc["colliding"].reshape(b, M), acc, ncoll, W, N, weights)
        rows = (torch.arange(b)[:, None] * M + sel["beam_row"]).reshape(-1)          # [b*W]
        r = genop_ref.advance(pp[rows], Y_gen[:, rows], X[:, rows], joints[rows], mproj[rows], dT[rows], reproj_factor, R0[rows], T0[rows], dt)
        gd = sc["dist"][rows].reshape(b, W)
        r.update(sel)
        r.update(cost=cost, terms=terms, acc_in=acc, ncoll_in=ncoll, goal_dist=gd, reached=gd < goal_thresh, pred_params=pp[rows])
        steps.append(r)
        acc, ncoll = sel["acc"], sel["ncoll"]
        X = r["seed_markers"].repeat_interleave(N, dim=0).permute(1, 0, 2)
        seed, R0, T0 = r["seed_params"].repeat_interleave(N, dim=0), r["R0"].repeat_interleave(N, dim=0), r["T0"].repeat_interleave(N, dim=0)
    K = len(steps)
    slot = backtrack(torch.stack([s["parent"] for s in steps]), K)
    path = []
    for k, s in enumerate(steps):
        at = torch.arange(b) * W + slot[k]
        p = {key: s[key][at] for key in ("marker_b", "pelvis", "R", "T", "pred_params")}
        per = lambda key: s[key].gather(1, slot[k][:, None])[:, 0]
        p.update(choice=per("beam_row"), status=per("status"), goal_dist=per("goal_dist"), reached=per("reached"), slot=slot[k])
        path.append(p)
    return steps, path
