"""GPU checks of the geodesic field and of the search that reads it: kernels of csrc/geodesic.hip, `GeodesicField`
(egogen_amd/geodesic.py), the entries egx_primitive_select_field / egx_primitive_beam_select_field (csrc/genop.hip) and
`generate_sequence_to_goal(geodesic=)`.

Yardsticks.  The field: bit-identical to float32 Dijkstra (tests/geodesic_ref.py), infinities included; the fixed point does not
depend on the order of relaxation, so nothing less is asked.  Sampled values, the goal term and the cost: `held()` of
tests/genop_gpu_helpers.py, the device within R = 3 times the distance of the float32 restatement from the float64 one over groups
of at least 64 values (the end-to-end check pools the 12 values it has).  Choices: the float64 choice on decidable groups, the 6x
rule and the 5 % cap of tests/test_genop_search_gpu.py.  Everything the field does not touch is `torch.equal` to the launch without it."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import geodesic_ref as gref
from tests import genop_search_ref as sref
from tests.genop_gpu_helpers import (CFG_RF, MIN_GROUP, POOL, ROOT, UNDECIDABLE_CAP, V_SMALL, W_TEST, _beam_select, _feet, _inputs, _restate,
                                     _rows_inputs, _select, _selection_args, emit, held, patched_loop, search_world, small_world)  # noqa: F401
from tests.test_genop_search_gpu import decidable

pytestmark = pytest.mark.gpu

GOAL_ONLY = {"goal": 1.0, "skate": 0.0, "floor": 0.0, "pene": 0.0, "face": 0.0}


def _field(*a, **kw):
    from egogen_amd.geodesic import GeodesicField
    return GeodesicField.from_raster(*a, **kw)


def _serp(H, W, pocket):
    return gref.sealed_pocket(gref.serpentine(H, W), *pocket)


# ---- the field ---------------------------------------------------------------------------------------------------------
RASTERS = {
    "corridor 1x7": (lambda: np.ones((1, 7), bool), 0.1, (0.05, 0.15), False),
    "corridor 130x3": (lambda: np.ones((130, 3), bool), 0.05, (0.12, 0.06), False),
    "serpentine 37x53": (lambda: _serp(37, 53, (4, 20)), 0.05, (0.12, 0.13), True),
    "serpentine 70x45": (lambda: _serp(70, 45, (12, 30)), 0.05, (0.11, 2.08), True),
    "serpentine 200x170": (lambda: _serp(200, 170, (100, 90)), 0.05, (0.2, 0.2), True),      # 7 x 6 tiles of 32 x 32
}


@pytest.mark.parametrize("name", list(RASTERS))
def test_field_is_float32_dijkstra(name):
    make, cell, goal, winding = RASTERS[name]
    free, origin = make(), np.array([0.0, 0.0])
    H, W = free.shape
    fld = _field(free, origin, cell, [[goal[0], goal[1], 0.9]])
    want = gref.field(free, origin, cell, goal)
    assert fld.dist.shape == (1, H, W) and fld.dist.dtype == torch.float32 and len(fld) == 1
    got = fld.dist[0].cpu()
    assert torch.equal(got, torch.from_numpy(want)), (name, int((got != torch.from_numpy(want)).sum()))
    assert 1 <= fld.passes <= H * W + 1
    emit(f"| field {name} | passes | {fld.passes} | longest path {np.max(want[np.isfinite(want)]):.2f} m | |")
    if winding:
        assert fld.passes > 1
        assert np.isinf(want[free]).sum() == 1                                  # the pocket, and nothing else, is cut off
        assert np.max(want[np.isfinite(want)]) > 3 * np.hypot(H, W) * cell     # the wave front winds through every corridor
    assert torch.equal(fld.origin.cpu(), torch.zeros(1, 2)) and fld.cell == cell
    assert torch.equal(fld.goals.cpu(), torch.tensor([[goal[0], goal[1], 0.9]]))


def test_field_several_goals_on_one_raster():
    free, cell, origin = _serp(37, 53, (4, 20)), 0.05, np.array([-0.4, 1.1])
    goals = np.array([[-0.4 + 0.12, 1.1 + 0.13], [-0.4 + 1.0, 1.1 + 2.5], [-0.4 + 1.7, 1.1 + 0.31]])
    fld = _field(free, origin, cell, goals)
    assert len(fld) == 3 and fld.goals.shape == (3, 3)
    for f in range(3):
        assert torch.equal(fld.dist[f].cpu(), torch.from_numpy(gref.field(free, origin, cell, goals[f]))), f


def test_field_two_rasters_with_scene_index():
    a, b = _serp(37, 53, (4, 20)), np.ones((37, 53), bool)
    b[10:30, 25] = False
    free, cell = np.stack([a, b]), 0.05
    origin = np.array([[0.0, 0.0], [3.0, -2.0]])
    idx = [1, 0, 1]
    goals = np.array([[3.0 + 0.6, -2.0 + 0.4], [0.12, 0.13], [3.0 + 1.2, -2.0 + 2.2]])
    fld = _field(free, origin, cell, goals, scene_index=idx)
    assert torch.equal(fld.origin.cpu(), torch.tensor(origin[idx], dtype=torch.float32))
    for f in range(3):
        assert torch.equal(fld.dist[f].cpu(), torch.from_numpy(gref.field(free[idx[f]], origin[idx[f]], cell, goals[f]))), f


def test_field_errors_on_the_device_path():
    from egogen_amd import _lib
    free = np.ones((6, 7), bool)
    free[:, 5:] = False
    assert len(_field(free, [0.0, 0.0], 0.1, [[0.25, 0.25, 0.9]])) == 1
    with pytest.raises(ValueError, match="goal 0 .*no seed"):
        _field(free, [0.0, 0.0], 0.1, [[0.3, 0.68, 0.9]])
    with pytest.raises(ValueError, match="not finite"):
        _field(free, [0.0, 0.0], 0.1, [[0.3, float("inf"), 0.9]])
    with pytest.raises(ValueError, match="scene_index must lie"):
        _field(np.stack([free, free]), [0.0, 0.0], 0.1, [[0.25, 0.25]], scene_index=[2])
    with pytest.raises(ValueError, match="origin must be"):
        _field(free, [[0.0, 0.0], [1.0, 1.0]], 0.1, [[0.25, 0.25]])
    fld = _field(free, [0.0, 0.0], 0.1, [[0.25, 0.25, 0.9]])
    with pytest.raises(ValueError, match="points must be"):
        fld.sample(torch.zeros(2, 4, 2))
    # the C entry checks its own arguments before anything is launched
    lib, buf = _lib.load(), torch.zeros(4096, device="cuda")
    p = C.c_void_p(buf.data_ptr())
    q = C.c_void_p(buf.data_ptr() + 1024)

    def call(free=p, S=1, F=1, H=4, W=4, w1=0.1, n=1, tmp=q):
        return lib.egx_geodesic_field(free, None, S, F, H, W, w1, 0.14, p, p, n, p, tmp, p, None, _lib.current_stream_ptr())
    for kw in ({"free": None}, {"S": 2}, {"H": 0}, {"n": 0}, {"w1": 0.0}, {"tmp": p}, {"F": 70000}):
        assert call(**kw) != 0, kw


# ---- the room of the sampling and selection tests: 120 x 120 cells of 0.1 m over [-6, 6]^2, two walls ---------------------
ROOM_CELL, ROOM_ORIGIN = 0.1, np.array([-6.0, -6.0])


def _room():
    free = np.ones((120, 120), bool)
    free[40:50, 0:90] = False         # x in [-2, -1], y in [-6, 3]
    free[60:120, 70:80] = False       # x in [0, 6], y in [1, 2]
    return free


def _free_goal(free, g):
    """the goal moved along +x until it lies on a free cell of the room"""
    g = np.clip(np.asarray(g, np.float64), -5.5, 5.5)
    cell_of = lambda q: tuple(np.clip(np.floor((q[:2] - ROOM_ORIGIN) / ROOM_CELL).astype(int), 0, 119))
    while not free[cell_of(g)]:
        g[0] = g[0] + 0.37 if g[0] + 0.37 < 5.5 else -5.5
    return g


_ROOM_FIELD = {}


def _room_field():
    """two fields on the room, built once: (GeodesicField, dist as numpy)"""
    if not _ROOM_FIELD:
        fld = _field(_room(), ROOM_ORIGIN, ROOM_CELL, [[3.0, -2.0, 0.9], [-4.0, 4.5, 0.9]])
        _ROOM_FIELD.update(f=fld, d=fld.dist.cpu().numpy())
    return _ROOM_FIELD["f"], _ROOM_FIELD["d"]


def test_room_field_is_float32_dijkstra():
    fld, d = _room_field()
    assert np.array_equal(d[0], gref.field(_room(), ROOM_ORIGIN, ROOM_CELL, [3.0, -2.0]))


def test_sample():
    fld, d = _room_field()
    rng = np.random.default_rng(11)
    n_in, n_edge = 80, 400
    inside = np.stack([rng.uniform(2.2, 5.8, n_in), rng.uniform(-5.8, 0.8, n_in)], 1)            # clear of both walls: four corners
    # within a cell of the outline of the first wall (x in [-2, -1], y up to 3), both sides, its end and its corners
    t = rng.uniform(0, 1, n_edge)
    side = rng.integers(0, 3, n_edge)
    off = rng.uniform(-0.1, 0.1, n_edge)
    edge = np.where((side == 0)[:, None], np.stack([-2.0 + off, -5.9 + 8.95 * t], 1),
                    np.where((side == 1)[:, None], np.stack([-1.0 + off, -5.9 + 8.95 * t], 1), np.stack([-2.1 + 1.2 * t, 3.0 + off], 1)))
    edge[:24] = np.stack([np.where(side[:24] == 0, -2.0, -1.0) + 0.5 * off[:24], -6.0 + 0.05 * t[:24]], 1)   # where the wall meets the raster's edge: one corner
    none = np.array([[-1.5, 0.0], [-1.45, -3.3], [3.0, 1.5], [5.95, 1.55],                         # inside a wall
                     [-7.0, 0.0], [0.0, 6.2], [40.0, -40.0], [np.inf, 0.0], [0.0, -np.inf], [-6.06, -6.06]])   # outside the raster
    nan = np.array([[np.nan, 0.0], [1.0, np.nan]])
    for f in range(2):
        pts = np.concatenate([inside, edge, none, nan]).astype(np.float32)
        r64, cnt = gref.sample(d[f], ROOM_ORIGIN, ROOM_CELL, pts, np.float64)
        r32, cnt32 = gref.sample(d[f], ROOM_ORIGIN, ROOM_CELL, pts, np.float32)
        both = np.zeros((2, len(pts), 2), np.float32)
        both[f] = pts
        got = fld.sample(torch.from_numpy(both))[f].cpu().numpy()
        assert np.array_equal(cnt, cnt32)
        c_in, c_edge = cnt[:n_in], cnt[n_in:n_in + n_edge]
        assert (c_in == 4).all()
        for k in (1, 2, 3):
            assert (c_edge == k).sum() >= 3, (k, np.bincount(c_edge))
        partial = np.flatnonzero((cnt >= 1) & (cnt <= 3))
        assert len(partial) >= MIN_GROUP
        held(f"sample field {f}", "four finite corners", got[:n_in], r64[:n_in], r32[:n_in])
        held(f"sample field {f}", "one to three finite corners", got[partial], r64[partial], r32[partial])
        k0 = n_in + n_edge
        assert (cnt[k0:k0 + len(none)] == 0).all() and (got[k0:k0 + len(none)] == np.float32(1.0e4)).all()
        assert (got[n_in:k0][c_edge == 0] == np.float32(1.0e4)).all()
        assert np.isnan(got[-2:]).all() and np.isnan(r32[-2:]).all()
        assert np.isfinite(got[:-2]).all()


def test_sample_on_a_blocked_last_row_and_column():
    free = gref.serpentine(37, 53)
    fld = _field(free, [0.0, 0.0], 0.05, [[0.12, 0.13]])
    last = np.array([[36.5 * 0.05, 1.0], [36.9 * 0.05, 0.3], [1.0, 52.5 * 0.05], [0.4, 52.99 * 0.05], [36.7 * 0.05, 52.7 * 0.05]], np.float32)
    got = fld.sample(torch.from_numpy(last[None])).cpu().numpy()[0]
    r32, cnt = gref.sample(fld.dist[0].cpu().numpy(), [0.0, 0.0], 0.05, last)
    assert (cnt == 0).all() and (got == np.float32(1.0e4)).all() and (r32 == np.float32(1.0e4)).all()


# ---- the selection entries ---------------------------------------------------------------------------------------------------
def _select_field(x, jpb, fld, index, weights=W_TEST, b=None, N=None, rf=CFG_RF, beam=None, acc=None, ncoll=None):
    """egx_primitive_select_field (beam = (W, N): egx_primitive_beam_select_field, acc / ncoll [b,W] zero unless given) on the
    row set x with the fields `fld` (None: a null field) -> (outputs on the CPU, inputs as launched)"""
    from egogen_amd import _lib
    b = x["b"] if b is None else b
    M = x["N"] if N is None else N
    lead, i, o, _alive = _selection_args(x, b, M, 0, jpb, rf, weights, 40.0, 0.1, ())
    fi = lambda *s: torch.full(s, -7, dtype=torch.int32, device="cuda")
    ff = lambda *s: torch.full(s, float("nan"), device="cuda")
    if fld is None:
        fa, idx = (None, None, 0.0, 0, 0, 0, None), None
    else:
        idx = None if index is None else torch.as_tensor(index, dtype=torch.int32, device="cuda")
        fa = (_lib.ptr(fld.dist), _lib.ptr(fld.origin), float(np.float32(fld.cell)), fld.dist.shape[1], fld.dist.shape[2], len(fld), _lib.ptr(idx))
    if beam is None:
        o = {"choice": fi(b), "status": fi(b), "reached": fi(b), "goal_dist": ff(b), **o}
        _lib.check(_lib.load().egx_primitive_select_field(
            *lead, b, M, _lib.ptr(o["choice"]), _lib.ptr(o["status"]), _lib.ptr(o["reached"]), _lib.ptr(o["goal_dist"]), _lib.ptr(o["cost"]),
            _lib.ptr(o["terms"]), _lib.ptr(o["colliding"]), *fa, _lib.current_stream_ptr()), "egx_primitive_select_field")
    else:
        W, N = beam
        acc = torch.zeros(b, W, device="cuda") if acc is None else acc.float().cuda().contiguous()
        ncoll = torch.zeros(b, W, dtype=torch.int32, device="cuda") if ncoll is None else ncoll.int().cuda().contiguous()
        o.update({"beam_row": fi(b, W), "parent": fi(b, W), "acc": ff(b, W), "ncoll": fi(b, W), "path_cost": ff(b, W), "status": fi(b, W),
                  "goal_dist": ff(b, W), "reached": fi(b, W)})
        _lib.check(_lib.load().egx_primitive_beam_select_field(
            *lead, b, W, N, _lib.ptr(acc), _lib.ptr(ncoll), _lib.ptr(o["cost"]), _lib.ptr(o["terms"]), _lib.ptr(o["colliding"]),
            _lib.ptr(o["beam_row"]), _lib.ptr(o["parent"]), _lib.ptr(o["acc"]), _lib.ptr(o["ncoll"]), _lib.ptr(o["path_cost"]),
            _lib.ptr(o["status"]), _lib.ptr(o["goal_dist"]), _lib.ptr(o["reached"]), *fa, _lib.current_stream_ptr()),
            "egx_primitive_beam_select_field")
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in o.items()}, i


def _room_rows(world, b, N, seed):
    """`_rows_inputs` with every goal on a free cell of the room, and the fields of those goals"""
    x = _rows_inputs(world, b, N, seed, True)
    free = _room()
    x["goal"] = torch.tensor(np.stack([_free_goal(free, g) for g in x["goal"].numpy()]), dtype=torch.float32)
    return x, _field(free, ROOM_ORIGIN, ROOM_CELL, x["goal"].numpy())


def _restate_field(i, fld, b, N, dtype):
    """the goal term and the cost of the rows of a launch with the fields `fld` (one per sequence) in `dtype` -> geo [b,N], cost
    [b,N], the other terms as a dict, number of finite corners [b,N]"""
    r = sref.score(i["Y_gen"], i["X"], i["J"], i["mp"], i["R0"], i["T0"], i["pene"], i["goal_rows"], _feet(), W_TEST, 40.0, CFG_RF, dtype)
    xy = gref.last_pelvis_world(i["R0"], i["T0"], i["J"], dtype).numpy().reshape(b, N, 2)
    d = fld.dist.cpu().numpy()
    npdt = np.float64 if dtype == torch.float64 else np.float32
    geo, cnt = zip(*[gref.sample(d[g], fld.origin[g].cpu().numpy(), fld.cell, xy[g], npdt) for g in range(b)])
    geo = torch.as_tensor(np.stack(geo))
    cost = gref.cost(geo.reshape(-1), r, W_TEST, dtype).reshape(b, N)
    return geo, cost, r, np.stack(cnt)


@pytest.mark.parametrize("N", [5, 70])
@pytest.mark.parametrize("b", [1, 3])
def test_primitive_select_field_kernel(small_world, b, N):
    name = f"select_field b={b} N={N}"
    got, r64, r32, oks, cnts = [], [], [], [], []
    for draw in range(max(1, -(-MIN_GROUP // (b * N)))):
        x, fld = _room_rows(small_world, b, N, 300 + b * 7 + N + 1000 * draw)
        index = list(range(b))
        o, i = _select_field(x, 127, fld, index)
        plain, _ = _select(x, 127)
        null, _ = _select_field(x, 127, None, None)
        for k in plain:                                                          # a null field: the entry without a field
            assert torch.equal(null[k], plain[k]), k
        # what the field does not touch
        assert torch.equal(o["terms"][..., 1:], plain["terms"][..., 1:]) and torch.equal(o["colliding"], plain["colliding"])
        ch = o["choice"].long()
        assert int(ch.min()) >= 0 and int(ch.max()) < N
        pick = lambda t: t.gather(1, ch[:, None])[:, 0]
        assert torch.equal(o["goal_dist"], pick(plain["terms"][..., 0]))          # Euclidean, of the row chosen with the field
        assert torch.equal(o["reached"].bool(), o["goal_dist"] < 0.1) and torch.equal(o["status"], pick(o["colliding"]))
        g64, c64, t64, cnt = _restate_field(i, fld, b, N, torch.float64)
        g32, c32, t32, _ = _restate_field(i, fld, b, N, torch.float32)
        coll = t64["colliding"].reshape(b, N)
        terms64 = torch.stack([g64] + [t64[k].reshape(b, N) for k in sref.TERMS[1:]], -1)
        terms32 = torch.stack([g32] + [t32[k].reshape(b, N) for k in sref.TERMS[1:]], -1)
        choice64, ok = decidable(c64, terms64, coll, c32)
        choice32, _ = sref.select(c32, terms32, coll)
        assert torch.equal(choice32[ok], choice64[ok])
        assert torch.equal(ch[ok], choice64[ok]), (name, draw, ch, choice64)
        own, own_status = sref.select(o["cost"], o["terms"], o["colliding"].bool())
        assert torch.equal(own, ch) and torch.equal(own_status.int(), o["status"])
        got.append((o["cost"], o["terms"][..., 0]))
        r64.append((c64, g64))
        r32.append((c32, g32))
        oks.append(ok)
        cnts.append(cnt.reshape(-1))
    cnt = np.concatenate(cnts)
    emit(f"| {name} | finite corners 0..4 | {np.bincount(cnt, minlength=5).tolist()} | | |")
    assert ((cnt >= 1) & (cnt < 4)).any() and (cnt == 0).any() and (cnt == 4).sum() > len(cnt) // 2
    cat = lambda lst, j: torch.cat([v[j] for v in lst], 0)
    held(name, "geo", cat(got, 1), cat(r64, 1), cat(r32, 1))
    held(name, "cost", cat(got, 0), cat(r64, 0), cat(r32, 0))
    ok = torch.cat(oks)
    share = 1.0 - float(ok.float().mean())
    emit(f"| {name} | undecidable groups | {int((~ok).sum())} of {ok.numel()} | {share:.3f} | |")
    assert share <= UNDECIDABLE_CAP, (name, share)


def test_primitive_select_field_shared_field(small_world):
    """a null field_index: every sequence reads field 0"""
    x, fld = _room_rows(small_world, 3, 5, 77)
    x["goal"] = x["goal"][:1].repeat(3, 1)
    one = _field(_room(), ROOM_ORIGIN, ROOM_CELL, x["goal"][:1].numpy())
    a, _ = _select_field(x, 127, one, None)
    b_, _ = _select_field(x, 127, one, [0, 0, 0])
    c, _ = _select_field(x, 127, one, [-4, 9, 0])                              # clamped into the one field
    for k in a:
        assert torch.equal(a[k], b_[k]) and torch.equal(a[k], c[k]), k


def test_primitive_beam_select_field_kernel(small_world):
    W, N, b = 2, 3, 3
    name = f"beam_select_field W={W} N={N}"
    got, r64, r32 = [], [], []
    for draw in range(-(-MIN_GROUP // (b * W * N))):
        x, fld = _room_rows(small_world, b, W * N, 500 + 1000 * draw)
        o, i = _select_field(x, 127, fld, list(range(b)), beam=(W, N))
        plain, _ = _beam_select(x, W, N, 127)
        null, _ = _select_field(x, 127, None, None, beam=(W, N))
        for k in plain:
            assert torch.equal(null[k], plain[k]), k
        greedy, _ = _select_field(x, 127, fld, list(range(b)))                  # the same rows through the greedy entry: the same scoring
        assert torch.equal(o["cost"], greedy["cost"]) and torch.equal(o["terms"], greedy["terms"])
        assert torch.equal(o["terms"][..., 1:], plain["terms"][..., 1:]) and torch.equal(o["colliding"], plain["colliding"])
        # the kept rows: the W first in (colliding, cost, row) on the kernel's own costs (all rows finite, acc = ncoll = 0)
        for g in range(b):
            order = sorted(range(W * N), key=lambda n: (int(o["colliding"][g, n]), float(o["cost"][g, n]), n))[:W]
            assert o["beam_row"][g].tolist() == order and o["parent"][g].tolist() == [n // N for n in order]
            assert torch.equal(o["goal_dist"][g], plain["terms"][g, order, 0])   # Euclidean
            assert torch.equal(o["path_cost"][g], o["cost"][g, order])
        assert torch.equal(o["reached"].bool(), o["goal_dist"] < 0.1)
        g64, c64, _, _ = _restate_field(i, fld, b, W * N, torch.float64)
        g32, c32, _, _ = _restate_field(i, fld, b, W * N, torch.float32)
        got.append((o["cost"], o["terms"][..., 0]))
        r64.append((c64, g64))
        r32.append((c32, g32))
    cat = lambda lst, j: torch.cat([v[j] for v in lst], 0)
    held(name, "geo", cat(got, 1), cat(r64, 1), cat(r32, 1))
    held(name, "cost", cat(got, 0), cat(r64, 0), cat(r32, 0))


def test_primitive_beam_select_field_carried_state(small_world):
    """The field phase redoes the path key of every row, carried cost plus the field's cost and the carried count of colliding nodes:
    with non-zero acc / ncoll per slot the kept rows are the W first in (ncoll + colliding, acc + cost, row) on the kernel's own costs."""
    W, N, b = 2, 3, 3
    g = torch.Generator().manual_seed(9)
    differs = False
    for draw in range(4):
        x, fld = _room_rows(small_world, b, W * N, 700 + 1000 * draw)
        acc = torch.rand(b, W, generator=g) * 6.0
        ncoll = torch.randint(0, 3, (b, W), generator=g, dtype=torch.int32)
        o, _ = _select_field(x, 127, fld, list(range(b)), beam=(W, N), acc=acc, ncoll=ncoll)
        free_run, _ = _select_field(x, 127, fld, list(range(b)), beam=(W, N))
        assert torch.equal(o["cost"], free_run["cost"]) and torch.equal(o["terms"], free_run["terms"])    # the carried state is not in a row's cost
        plain, _ = _beam_select(x, W, N, 127, acc=acc, ncoll=ncoll)
        path = (acc[:, :, None] + o["cost"].reshape(b, W, N)).reshape(b, W * N)                           # one float32 addition
        nc = (ncoll[:, :, None] + o["colliding"].reshape(b, W, N)).reshape(b, W * N)
        for i in range(b):
            order = sorted(range(W * N), key=lambda n: (int(nc[i, n]), float(path[i, n]), n))[:W]
            assert o["beam_row"][i].tolist() == order and o["parent"][i].tolist() == [n // N for n in order], (draw, i)
            assert torch.equal(o["path_cost"][i], path[i, order]) and torch.equal(o["ncoll"][i], nc[i, order])
            assert torch.equal(o["goal_dist"][i], plain["terms"][i, order, 0])
            assert o["status"][i].tolist() == [int(o["colliding"][i, n]) for n in order]
            # acc_out: the parent's acc plus the row's q, which the launch without a field gives for the rows it kept as well
            for slot, n in enumerate(order):
                if n in plain["beam_row"][i].tolist():
                    assert float(o["acc"][i, slot]) == float(plain["acc"][i, plain["beam_row"][i].tolist().index(n)])
            differs |= order != sorted(range(W * N), key=lambda n: (int(o["colliding"][i, n]), float(o["cost"][i, n]), n))[:W]
    assert differs                                                              # the carried state does change the ranking in these draws


def test_field_sends_the_search_round_the_wall(small_world):
    """What the feature is for.  Goal at (2, 0); a wall x in [0, 0.4] from y = -6 to y = 4.  Candidate A ends at (-1, 0), 3 m from
    the goal in a straight line and behind the wall (over 9 m round its end); candidate B at (5.5, 0), 3.5 m away on the goal's
    side.  The straight line chooses A, the field B."""
    d = _inputs(small_world, POOL)
    pelvis = d["j127"].reshape(POOL, 20, 127, 3)[0, 19, 0].cpu()
    goal = torch.tensor([[2.0, 0.0, float(pelvis[2])]])
    ends = torch.tensor([[-1.0, 0.0, 0.0], [5.5, 0.0, 0.0]])
    T0 = ends - pelvis * torch.tensor([1.0, 1.0, 0.0])
    x = {"rows": torch.zeros(2, dtype=torch.long), "R0": torch.eye(3).repeat(2, 1, 1), "T0": T0, "goal": goal, "pene": None, "pool": d,
         "b": 1, "N": 2}
    free = np.ones((120, 120), bool)
    free[60:64, 0:100] = False
    fld = _field(free, ROOM_ORIGIN, ROOM_CELL, goal.numpy())
    plain, _ = _select(x, 127, weights=GOAL_ONLY)
    with_field, _ = _select_field(x, 127, fld, None, weights=GOAL_ONLY)
    assert np.allclose(plain["cost"][0].numpy(), [3.0, 3.5], atol=1e-5) and int(plain["choice"][0]) == 0
    assert int(with_field["choice"][0]) == 1, with_field["cost"]
    assert float(with_field["cost"][0, 0]) > 8.5 and 3.5 - 0.01 <= float(with_field["cost"][0, 1]) <= 3.5 * 1.0824 + 0.1
    assert torch.equal(with_field["goal_dist"], plain["terms"][:, 1, 0]) and torch.equal(with_field["terms"][..., 0], with_field["cost"])


# ---- end to end ----------------------------------------------------------------------------------------------------------------
def _e2e_field(goal):
    free = np.ones((120, 120), bool)
    free[30:90, 65:67] = False            # x in [-3, 3], y in [0.5, 0.7]: between the walkers' start and their goals
    return _field(free, ROOM_ORIGIN, ROOM_CELL, goal.numpy())


@pytest.mark.parametrize("W,N", [(1, 4), (2, 2)])
def test_generate_sequence_to_goal_with_a_field(search_world, W, N):
    w = search_world
    op, K, b = w["op"], 3, 2
    data, bparams, betas, goal = w["data"][:, :b].contiguous(), w["bparams"][:, :b].contiguous(), w["betas"][:b], w["goal"][:b]
    z = torch.randn(K, b * W * N, 128, generator=torch.Generator().manual_seed(40 + W))
    kw = dict(z=z, reproj_factor=CFG_RF, weights=W_TEST, goal_thresh=0.0, beam_width=W, to_numpy=False)
    base = op.generate_sequence_to_goal(data, bparams, betas, goal, K, N, **kw)
    none = op.generate_sequence_to_goal(data, bparams, betas, goal, K, N, geodesic=None, **kw)
    for k in ("markers", "params", "rotmat", "transl", "pelvis", "z", "R0", "T0", "choice", "cost", "cost_terms", "colliding", "status",
              "goal_dist", "n_valid"):
        assert torch.equal(getattr(none, k), getattr(base, k)), k
    assert none.geo_dist is None and base.geo_dist is None and "geo_dist" in none.search
    fld = _e2e_field(goal)
    with patched_loop(op, "_search_loop" if W == 1 else "_beam_loop", no_host_wait=True) as seen:
        res = op.generate_sequence_to_goal(data, bparams, betas, goal, K, N, geodesic=fld, **kw)
    assert seen.calls == [(K, b, N) if W == 1 else (K, b, W, N)]
    assert res.geo_dist.shape == (K, b)
    chosen = res.cost_terms[..., 0].gather(2, res.choice.long().unsqueeze(-1))[..., 0]
    assert torch.equal(res.geo_dist, chosen) and torch.equal(res.geo_dist, res.search["geo_dist"])
    # the field's value at the end of every chosen primitive, from the records
    f64 = lambda t: t.double().cpu()
    p64 = (torch.einsum("kbij,kbj->kbi", f64(res.rotmat), f64(res.pelvis[:, :, 19])) + f64(res.transl))[..., :2]
    p32 = (torch.einsum("kbij,kbj->kbi", res.rotmat.cpu(), res.pelvis[:, :, 19].cpu()) + res.transl.cpu())[..., :2]
    d = fld.dist.cpu().numpy()
    r64 = np.stack([gref.sample(d[i], ROOM_ORIGIN, ROOM_CELL, p64[:, i].numpy(), np.float64)[0] for i in range(b)], 1)
    r32 = np.stack([gref.sample(d[i], ROOM_ORIGIN, ROOM_CELL, p32[:, i].numpy(), np.float32)[0] for i in range(b)], 1)
    dev = fld.sample(p32.permute(1, 0, 2).contiguous()).cpu().t()
    held(f"to_goal W={W} N={N}", "geo_dist", torch.cat([res.geo_dist.cpu(), dev]), np.concatenate([r64, r64]), np.concatenate([r32, r32]))
    # goal_dist stays the straight line in 3-D; the way along the raster is no shorter than the straight line on the floor
    e = (torch.einsum("kbij,kbj->kbi", f64(res.rotmat), f64(res.pelvis[:, :, 19])) + f64(res.transl) - f64(goal)[None]).norm(dim=-1)
    exy = (p64 - f64(goal)[None, :, :2]).norm(dim=-1)
    assert torch.allclose(f64(res.goal_dist), e, atol=1e-5) and bool((f64(res.geo_dist) >= exy - 2 * ROOM_CELL).all())
    # one field for all sequences, when they share the goal
    shared = goal[:1].repeat(b, 1)
    one = _e2e_field(goal[:1])
    r1 = op.generate_sequence_to_goal(data, bparams, betas, shared, K, N, geodesic=one, **kw)
    rb = op.generate_sequence_to_goal(data, bparams, betas, shared, K, N, geodesic=_e2e_field(shared), **kw)
    assert torch.equal(r1.geo_dist, rb.geo_dist) and torch.equal(r1.cost, rb.cost) and torch.equal(r1.markers, rb.markers)
    with pytest.raises(ValueError, match="other goals"):
        op.generate_sequence_to_goal(data, bparams, betas, goal + torch.tensor([0.1, 0.0, 0.0]), K, N, geodesic=fld, **kw)
    with pytest.raises(ValueError, match="1 or 2 fields"):
        op.generate_sequence_to_goal(data, bparams, betas, goal, K, N, geodesic=_e2e_field(w["goal"]), **kw)


def test_gen_motion_driver_walkable(tmp_path):
    from egogen_amd import scene_gen as sg
    free = np.ones((120, 120), bool)
    free[30:90, 65:67] = False
    scene = {"edges": np.zeros((4, 4), np.float32), "tris": np.zeros((2, 6), np.float32), "floor_height": 0.0,
             "pairs": np.zeros((4, 2, 3), np.float32), "nav_v": np.zeros((4, 3), np.float32), "nav_f": np.zeros((2, 3), np.int32),
             "rings": sg.grid_to_rings(free, ROOM_ORIGIN, ROOM_CELL)}
    bare, with_raster = str(tmp_path / "bare.npz"), str(tmp_path / "walkable.npz")
    sg.save_scene(bare, scene)
    sg.save_scene(with_raster, dict(scene, free=free, origin=ROOM_ORIGIN, cell=ROOM_CELL))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    base = [sys.executable, os.path.join(ROOT, "exp_GAMMAPrimitive", "gen_motion.py"), "--n-primitives", "2", "--seed", "3", "--num-verts",
            str(V_SMALL), "--n-gens", "2", "--goal", "0.5,2.0,0.9", "--n-candidates", "4"]
    out = tmp_path / "out"
    r = subprocess.run(base + ["--walkable", with_raster, "--out", str(out)], cwd=str(tmp_path), env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    files = sorted(f for f in os.listdir(out) if f.startswith("motion_") and f.endswith(".pkl"))
    assert len(files) == 2, files
    assert "geodesic field: 120 x 120 cells" in r.stdout and r.stdout.count("m along the walkable raster") == 2, r.stdout[-800:]
    r = subprocess.run(base + ["--walkable", bare, "--out", str(tmp_path / "none")], cwd=str(tmp_path), env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode != 0 and "no walkable raster" in r.stderr and not os.path.exists(tmp_path / "none"), r.stderr[-800:]
