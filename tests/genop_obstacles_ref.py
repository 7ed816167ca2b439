"""The moving-obstacle term and veto of the primitive search (`generate_sequence_to_goal(obstacles=)`, entries
egx_primitive_select_obstacles / egx_primitive_beam_select_obstacles, the obstacle phase of csrc/genop.hip) as plain torch on the
CPU, parametrised by dtype: the float64 truth and the float32 yardstick of tests/test_genop_obstacles_{cpu,gpu}.py.  The inputs
are taken as the float32 values the device reads; every operation is rounded in `dtype`.

  * `world_pelvis`: the world xy of joint 0 of the 20 bodies of a row;
  * `window`: the positions of a set's obstacles at the absolute frames clamp(frame0 + t, 0, T - 1), t = 2..19;
  * `row_terms`: clearance, term and hit of every row;
  * `apply`: cost, q and colliding of rows scored by tests/genop_search_ref.score (optionally with a field's goal term,
    tests/geodesic_ref.cost) with the obstacle term added, as the kernels add it;
  * `select` / `beam_select`: the choices on those (genop_search_ref.select, genop_beam_ref.beam_select with q carrying the term)."""
import numpy as np
import torch

from tests import genop_beam_ref as bref
from tests import genop_search_ref as sref
from tests import geodesic_ref as gref

FRAMES = tuple(range(2, 20))       # the predicted frames: what is scored


def _c(t, dtype):
    return torch.as_tensor(np.asarray(t.detach().cpu()) if torch.is_tensor(t) else np.asarray(t)).to(dtype)


def world_pelvis(R0, T0, joints, dtype):
    """R0 [B,3,3], T0 [B,3], joints [B,20,J,3] -> world xy [B,20,2] of joint 0 of every body, in `dtype`"""
    R0, T0, j = _c(R0, dtype).reshape(-1, 3, 3), _c(T0, dtype).reshape(-1, 3), _c(joints, dtype)[:, :, 0]
    return (torch.einsum("bij,btj->bti", R0, j) + T0[:, None])[..., :2]


def window(xy_set, frame0, dtype):
    """xy_set [O,T,2] -> [18,O,2]: every obstacle at absolute frame clamp(frame0 + t, 0, T - 1) for t = 2..19"""
    xy = _c(xy_set, dtype)
    T = xy.shape[1]
    a = torch.tensor([min(max(int(frame0) + t, 0), T - 1) for t in FRAMES], dtype=torch.long)
    return xy[:, a].permute(1, 0, 2)


def row_terms(R0, T0, joints, xy, radius, count, set_of_row, frame0, margin, body_radius, dtype):
    """xy [S,O_max,T,2], radius [S,O_max], count [S], set_of_row [B] -> dict of [B] tensors: clearance = min_t c_t with
    c_t = min_o |p_t - o| - (r_o + body_radius) (+inf for an empty set), term = sum_t max(0, margin - c_t) / 18, hit = clearance <
    0.  A NaN pelvis gives a NaN term and clearance and no hit."""
    p = world_pelvis(R0, T0, joints, dtype)[:, 2:]                               # [B,18,2]
    B = p.shape[0]
    xy, radius, count = np.asarray(xy), np.asarray(radius), np.asarray(count).reshape(-1)
    set_of_row = np.asarray(set_of_row).reshape(-1)
    c = torch.full((B, len(FRAMES)), float("inf"), dtype=dtype)
    c = torch.where(torch.isnan(p).any(-1), torch.full_like(c, float("nan")), c)
    for r in range(B):
        s = int(set_of_row[r])
        n = int(count[s])
        if n == 0:
            continue
        w = window(xy[s, :n], frame0, dtype)                                     # [18,n,2]
        rr = _c(radius[s, :n], dtype) + torch.tensor(body_radius, dtype=torch.float32).to(dtype)
        d = p[r][:, None, :] - w
        dist = torch.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1])
        c[r] = (dist - rr[None]).amin(dim=1)                                     # NaN propagates
    m = torch.tensor(margin, dtype=torch.float32).to(dtype)
    pen = torch.where(torch.isnan(c), c, (m - c).clamp(min=0))
    clearance = c.amin(dim=1)
    return {"clearance": clearance, "term": pen.sum(dim=1) / len(FRAMES), "hit": clearance < 0}


def apply(r, ob, w_obs, dtype, weights=None, geo=None):
    """r: what genop_search_ref.score gave for the rows, ob: what `row_terms` gave -> dict: cost (r's, or with geo [B] the field's
    cost geodesic_ref.cost, plus w_obs * term, one product and one addition in `dtype`), q (the beam's, with the same product
    added), colliding (r's OR hit), terms [B,5] (the goal term replaced by geo where given), and ob's entries."""
    w = torch.tensor(w_obs, dtype=torch.float32).to(dtype)
    terms = torch.stack([r[t] for t in sref.TERMS], -1)
    prev = r["cost"]
    if geo is not None:
        geo = _c(geo, dtype)
        prev = gref.cost(geo, r, dict(sref.WEIGHTS, **(weights or {})), dtype)
        terms = torch.cat([geo[:, None], terms[:, 1:]], -1)
    add = w * ob["term"]
    return {"cost": prev + add, "q": bref.q_of(terms, weights) + add, "colliding": r["colliding"] | ob["hit"], "terms": terms,
            "term": ob["term"], "clearance": ob["clearance"], "hit": ob["hit"]}


def _terms6(a, b, M):
    """the five terms and the obstacle term side by side: a non-finite obstacle term makes the row non-finite, as any term does"""
    return torch.cat([a["terms"], a["term"][:, None]], -1).reshape(b, M, 6)


def select(a, b, N):
    """`apply`'s result for b groups of N rows -> choice [b], status [b] (genop_search_ref.select's order)"""
    return sref.select(a["cost"].reshape(b, N), _terms6(a, b, N), a["colliding"].reshape(b, N))


def beam_select(a, b, W, N, acc, ncoll):
    """`apply`'s result for b groups of W * N rows -> genop_beam_ref.beam_select's dict with acc carrying q + w_obs * term"""
    M = W * N
    cost, terms, coll = a["cost"].reshape(b, M), _terms6(a, b, M), a["colliding"].reshape(b, M)
    acc = torch.as_tensor(acc).to(cost.dtype)
    nonfinite, nc, path = bref.path_keys(cost, terms, coll, acc, ncoll, W, N)
    beam_row = torch.zeros(b, W, dtype=torch.long)
    for i in range(b):
        keys = sorted((int(nonfinite[i, r]), int(nc[i, r]), float(path[i, r]), r) for r in range(M))
        beam_row[i] = torch.tensor([k[3] for k in keys[:W]])
    parent = beam_row // N
    pick = lambda t: t.gather(1, beam_row)
    return {"beam_row": beam_row, "parent": parent, "acc": acc.gather(1, parent) + pick(a["q"].reshape(b, M)), "ncoll": pick(nc),
            "path_cost": pick(path), "status": pick(coll.long()) | (pick(nonfinite.long()) << 1)}
