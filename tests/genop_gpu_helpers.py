"""What tests/test_genop_gpu.py, test_genop_search_gpu.py and test_genop_beam_gpu.py share: the `held()` yardstick, the synthetic
walkers and the input pool built from them, the operator on seeded weights (fixtures `small_world`, `search_world`), a wrapper
per launch of csrc/genop.hip that returns what the kernel wrote, and `patched_loop`, which stands in for a primitive loop of the
operator for the length of a `with` block; and what tests/test_genop_policy_gpu.py and test_genop_people_gpu.py share: the wrappers
of the observe entries of csrc/genop_policy.hip and the yardstick of their rays.  A plain module: the test files import the names they use, fixtures included."""
import contextlib
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

from tests.helpers import seeded_prior_state_dict

R = 3.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V_SMALL = 2048
CFG_RF = 0.5        # modelconfig.reproj_factor of the packaged policy configs
POOL = 65                   # rows of the walker pool (`_inputs`)
W_TEST = {"goal": 1.0, "skate": 2.0, "floor": 0.5, "pene": 0.3, "face": 0.7}
W_ORDER = ("goal", "skate", "floor", "pene", "face")
UNDECIDABLE_CAP = 0.05
MIN_GROUP = 64              # candidate rows pooled into one held() group (docstring of tests/test_genop_search_gpu.py)


def emit(line):
    print(line)
    path = os.environ.get("EGX_GENOP_TABLE")
    if path:
        with open(path, "a") as fh:
            fh.write(line + "\n")


def held(name, group, got, truth64, f32):
    t = torch.as_tensor(truth64, dtype=torch.float64)
    err = float((torch.as_tensor(got).double().cpu() - t).abs().max())
    e32 = float((torch.as_tensor(f32).double() - t).abs().max())
    emit(f"| {name} | {group} | {e32:.3e} | {err:.3e} | {err / e32 if e32 > 0 else float(err > 0):.2f} |")
    assert err <= R * e32, (name, group, err, e32)


def _aa2R64(aa):
    from oracle.rot import tgm_angle_axis_to_rotation_matrix as aa2R
    return aa2R(torch.as_tensor(aa).detach().cpu().double().reshape(-1, 3))


def _feet():
    from egogen_amd import synth
    return synth.feet_marker_idx()


# ----------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def patched_loop(op, name, no_host_wait=False, then=None):
    """op.<name> (`_advance_loop`, `_search_loop` or `_beam_loop`) replaced by a wrapper around the real loop for the length of
    the block and put back in `finally`.  Yields a record of what went through it: `calls`, the integer arguments of every call
    that returned, and `s`, the state dict of the last one, which outlives the call.  no_host_wait: the real loop runs under
    torch.cuda.set_sync_debug_mode("error"), so a host wait inside it raises.  then(s): called after the real loop, before the
    operator reads what the loop left."""
    real = getattr(op, name)
    seen = types.SimpleNamespace(calls=[], s=None)

    def loop(*a):
        if no_host_wait:
            old = torch.cuda.get_sync_debug_mode()
            torch.cuda.set_sync_debug_mode("error")
        try:
            real(*a)
        finally:
            if no_host_wait:
                torch.cuda.set_sync_debug_mode(old)
        seen.calls.append(a[:-1])
        seen.s = a[-1]
        if then is not None:
            then(a[-1])
    setattr(op, name, loop)
    try:
        yield seen
    finally:
        setattr(op, name, real)


# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_world():
    from egogen_amd import synth
    from egogen_amd.body_model import BodyModelHandle
    bm = synth.make_body_model(0, num_verts=V_SMALL)
    mk = synth.marker_ids(V_SMALL)
    return {"bm": bm, "mk": mk, "handle": BodyModelHandle(bm, mk, synth.feet_vids(V_SMALL))}


def _walkers(B, seed):
    """Walking-like primitives (scripts/gen_combo_golden.py::make_sequence) in their canonical frame: xb[B,20,93], betas[B,10].
    Body 1 (B >= 3) is yawed by almost pi, so its hip axis points the other way along x; body 2 carries a global orientation
    of 3.1 rad (frame 18) and 3.25 rad (frame 19) about x: the large-angle branch of rot -> aa with both signs of w."""
    g = torch.Generator().manual_seed(seed)
    xb = torch.zeros(20, B, 93)
    step = torch.tensor([0.0, 0.02, 0.0]) + torch.randn(1, B, 3, generator=g) * 0.004
    xb[:, :, :3] = torch.arange(20).view(20, 1, 1) * step + torch.tensor([0.0, 0.0, 0.9])
    xb[:, :, 3:69] = torch.randn(1, B, 66, generator=g) * 0.08 + (torch.randn(20, B, 66, generator=g) * 0.02).cumsum(0)
    xb[:, :, 69:] = torch.randn(1, B, 24, generator=g) * 0.1
    if B >= 3:
        xb[:, 1, 3:6] = torch.tensor([0.0, 0.0, np.pi - 0.05]) + torch.randn(20, 3, generator=g) * 0.01
        xb[:, 2, 3:6] = torch.tensor([3.1, 0.0, 0.0]) + torch.randn(20, 3, generator=g) * 0.01
        xb[19, 2, 3:6] = torch.tensor([3.25, 0.01, -0.01])
    betas = torch.randn(B, 10, generator=g) * 0.5
    return xb.permute(1, 0, 2).contiguous(), betas.contiguous(), g


_INPUTS = {}


def _inputs(world, B):
    """Everything one launch reads, on the device, for B sequences (computed once per B)."""
    if B in _INPUTS:
        return _INPUTS[B]
    h = world["handle"]
    pp, betas, g = _walkers(B, 900 + B)
    pp_d, bt_d = pp.cuda(), betas.cuda()
    o = h.forward(pp_d.reshape(B * 20, 93), bt_d, 20, want_verts=False)
    j127, mproj = o["joints"].clone(), o["markers"].clone()
    j55 = h.joints55(pp_d.reshape(B * 20, 93), bt_d, 20)
    m = mproj.reshape(B, 20, 201)
    noisy = (m.cpu() + torch.randn(B, 20, 201, generator=g) * 0.01).permute(1, 0, 2).contiguous()
    Rz = torch.randn(B, generator=g) * 2.0
    R0 = torch.zeros(B, 3, 3)
    R0[:, 0, 0], R0[:, 0, 1], R0[:, 1, 0], R0[:, 1, 1], R0[:, 2, 2] = torch.cos(Rz), -torch.sin(Rz), torch.sin(Rz), torch.cos(Rz), 1.0
    T0 = torch.randn(B, 3, generator=g) * 2.0
    delta_T = h.joints55(torch.zeros(B, 93, device="cuda"), bt_d, 1)[:, 0].contiguous()
    torch.cuda.synchronize()
    d = {"pp": pp_d, "X": noisy[:2].cuda().contiguous(), "Y_gen": noisy[2:].cuda().contiguous(), "j127": j127, "j55": j55,
         "mproj": mproj, "delta_T": delta_T, "R0": R0.cuda(), "T0": T0.cuda()}
    _INPUTS[B] = d
    return d


def _op(model=None, body_model=None, cfg_extra=None):
    from egogen_amd.genop import GAMMAPrimitiveComboGenOP
    from egogen_amd.models import PREDICTOR_CFG, REGRESSOR_CFG
    op = GAMMAPrimitiveComboGenOP({"modelconfig": dict(PREDICTOR_CFG, **(cfg_extra or {})), "trainconfig": {}},
                                  {"modelconfig": dict(REGRESSOR_CFG), "trainconfig": {}}, {"gpu_index": 0})
    op.model, op.body_model = model, body_model
    return op


def _combo(sd):
    from egogen_amd.models import GAMMAPrimitiveCombo, PREDICTOR_CFG, REGRESSOR_CFG
    combo = GAMMAPrimitiveCombo(PREDICTOR_CFG, REGRESSOR_CFG)
    combo.load_state_dict(sd)
    return combo.cuda().eval()


@pytest.fixture(scope="module")
def search_world(small_world):
    """b = 3 walkers on the small synthetic body with a seeded prior: the operator and its inputs."""
    h = small_world["handle"]
    sd = seeded_prior_state_dict()
    op = _op(_combo(sd), h)
    b = 3
    pp, betas, g = _walkers(b, 78)
    pp[:, :, 3:6] = torch.randn(b, 1, 3, generator=g) * 0.05        # ordinary orientations for all three walkers
    o = h.forward(pp.cuda().reshape(b * 20, 93), betas.cuda(), 20, want_verts=False)
    data = o["markers"].reshape(b, 20, 201)[:, :2].permute(1, 0, 2).contiguous().cpu()
    bparams = pp[:, :2].permute(1, 0, 2).contiguous()
    goal = torch.tensor([[0.5, 2.0, 0.9], [-1.0, 1.0, 0.9], [0.0, 3.0, 0.9]])
    return {"op": op, "sd": sd, "data": data, "bparams": bparams, "pp": pp, "betas": betas, "goal": goal, "handle": h, "g": g, "b": b}


# ---- the hand-off launches -------------------------------------------------------------------------------------------
def _vp(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _handoff_args(d, rows, jpb, rf, recs, with_params, Y_gen=None, nan_rows=()):
    """The pool rows `rows` of the input set d as a hand-off entry reads them, and NaN-filled outputs for `recs` records ->
    (the entry's ten leading arguments, the inputs, the outputs, its arguments from out_seed_params to out_x_ld)"""
    from egogen_amd._lib import ptr
    rows = torch.as_tensor(rows, device="cuda")
    n = int(rows.numel())
    sel = lambda t, per=1: t.reshape(-1, per, *t.shape[1:])[rows].reshape(n * per, *t.shape[1:]).contiguous()
    i = {"pp": d["pp"][rows].contiguous(), "Y_gen": (d["Y_gen"] if Y_gen is None else Y_gen)[:, rows].contiguous(),
         "X": d["X"][:, rows].contiguous(), "J": sel(d["j127"] if jpb == 127 else d["j55"], 20), "mp": sel(d["mproj"], 20),
         "dT": d["delta_T"][rows].contiguous(), "R0": d["R0"][rows].clone().contiguous(), "T0": d["T0"][rows].clone().contiguous()}
    for r in nan_rows:
        i["J"].view(n, 20, jpb, 3)[r, 5, 0, 1] = float("nan")
    f = lambda *s: torch.full(s, float("nan"), device="cuda")
    o = {"marker_b": f(recs, 20, 67, 3), "pelvis": f(recs, 20, 3), "R": f(recs, 3, 3), "T": f(recs, 3), "seed_params": f(n, 2, 93),
         "seed_markers": f(2, n, 201)}
    if with_params:
        o["params"] = f(recs, 20, 93)
    lead = (ptr(i["pp"]), ptr(i["Y_gen"]), _vp(i["X"][0]), _vp(i["X"][1]), 201, ptr(i["J"]), jpb, ptr(i["mp"]), ptr(i["dT"]), float(rf))
    return lead, i, o, (ptr(o["seed_params"]), _vp(o["seed_markers"][0]), _vp(o["seed_markers"][1]), 201)


def _launch(d, rows, jpb, rf, nonfinite=None, Y_gen=None):
    """egx_primitive_advance on the sequences `rows` of the input set d -> dict of outputs (device tensors)."""
    from egogen_amd import _lib
    B = len(rows)
    lead, i, o, seed_out = _handoff_args(d, rows, jpb, rf, B, False, Y_gen)
    _lib.check(_lib.load().egx_primitive_advance(
        *lead, B, _lib.ptr(i["R0"]), _lib.ptr(i["T0"]), _lib.ptr(o["marker_b"]), _lib.ptr(o["pelvis"]), _lib.ptr(o["R"]), _lib.ptr(o["T"]),
        *seed_out, _lib.ptr(nonfinite), _lib.current_stream_ptr()), "egx_primitive_advance")
    torch.cuda.synchronize()
    rows = torch.as_tensor(rows, device="cuda")
    o.update(R0=i["R0"], T0=i["T0"], seed_markers=o["seed_markers"].permute(1, 0, 2).contiguous())
    o["_in"] = {"pp": i["pp"], "Y_gen": i["Y_gen"], "X": i["X"], "J": i["J"].reshape(B, 20, jpb, 3), "mp": i["mp"].reshape(B, 20, 67, 3),
                "dT": i["dT"], "R0": d["R0"][rows], "T0": d["T0"][rows]}
    return o


def _advance_select(d, rows, choice, N, jpb, rf, nonfinite=None):
    """egx_primitive_advance_select on the candidate rows `rows` (b * N pool rows) of the input set d"""
    from egogen_amd import _lib
    b = len(rows) // N
    lead, i, o, seed_out = _handoff_args(d, rows, jpb, rf, b, True)
    ch = torch.as_tensor(choice, dtype=torch.int32, device="cuda")
    _lib.check(_lib.load().egx_primitive_advance_select(
        *lead, b, _lib.ptr(ch), N, _lib.ptr(i["R0"]), _lib.ptr(i["T0"]), _lib.ptr(o["marker_b"]), _lib.ptr(o["pelvis"]), _lib.ptr(o["R"]),
        _lib.ptr(o["T"]), _lib.ptr(o["params"]), *seed_out, _lib.ptr(nonfinite), _lib.current_stream_ptr()), "egx_primitive_advance_select")
    torch.cuda.synchronize()
    o.update(R0=i["R0"], T0=i["T0"], seed_markers=o["seed_markers"].permute(1, 0, 2).contiguous())
    return o


def _advance_beam(d, rows, beam_row, W, N, jpb, rf, status=None, nan_rows=()):
    """egx_primitive_advance_beam on the rows `rows` (b * W * N pool rows) of the input set d; beam_row [b,W]"""
    from egogen_amd import _lib
    n = len(rows)
    b = n // (W * N)
    lead, i, o, seed_out = _handoff_args(d, rows, jpb, rf, b * W, True, nan_rows=nan_rows)
    keep = (i["R0"].clone(), i["T0"].clone())
    br = torch.as_tensor(beam_row, dtype=torch.int32, device="cuda").reshape(b, W).contiguous()
    st = torch.zeros(b, W, dtype=torch.int32, device="cuda") if status is None else status.int().cuda().contiguous()
    o.update(R0=torch.full((n, 3, 3), float("nan"), device="cuda"), T0=torch.full((n, 3), float("nan"), device="cuda"))
    _lib.check(_lib.load().egx_primitive_advance_beam(
        *lead, b, W, N, _lib.ptr(br), _lib.ptr(i["R0"]), _lib.ptr(i["T0"]), _lib.ptr(o["R0"]), _lib.ptr(o["T0"]), _lib.ptr(o["marker_b"]),
        _lib.ptr(o["pelvis"]), _lib.ptr(o["R"]), _lib.ptr(o["T"]), _lib.ptr(o["params"]), *seed_out, _lib.ptr(st),
        _lib.current_stream_ptr()), "egx_primitive_advance_beam")
    torch.cuda.synchronize()
    assert torch.equal(i["R0"], keep[0]) and torch.equal(i["T0"], keep[1])          # the input frames are only read
    o.update(status=st, seed_markers=o["seed_markers"].permute(1, 0, 2).contiguous())
    return o


# ---- the selection launches ------------------------------------------------------------------------------------------
def _rows_inputs(world, b, N, seed, with_pene):
    """b * N candidate rows drawn from the walker pool, each in a frame (R0, T0) of its own, one goal per sequence."""
    d = _inputs(world, POOL)
    g = torch.Generator().manual_seed(seed)
    rows = (torch.arange(b * N) * 7 + seed) % POOL
    yaw = torch.randn(b * N, generator=g) * 2.0
    R0 = torch.zeros(b * N, 3, 3)
    R0[:, 0, 0], R0[:, 0, 1], R0[:, 1, 0], R0[:, 1, 1], R0[:, 2, 2] = torch.cos(yaw), -torch.sin(yaw), torch.sin(yaw), torch.cos(yaw), 1.0
    T0 = torch.randn(b * N, 3, generator=g) * torch.tensor([2.0, 2.0, 0.05])
    goal = torch.randn(b, 3, generator=g) * torch.tensor([3.0, 3.0, 0.0]) + torch.tensor([0.0, 0.0, 0.9])
    pene = None
    if with_pene:
        top = torch.randint(0, 90, (b * N, 1), generator=g)
        pene = (torch.rand(b * N, 20, generator=g) * (top + 1)).floor().int()
    return {"rows": rows, "R0": R0, "T0": T0, "goal": goal, "pene": pene, "pool": d, "b": b, "N": N}


def _handmade(world, costs, coll):
    """One group of len(costs) duplicates of pool row 0 whose cost (w_goal = 1, every other weight 0) is ordered like `costs`: the
    goal sits `cost` metres beside the last pelvis; a non-finite cost is a NaN in the row's T0.  (A non-finite term is made in
    `_select`: a NaN in a joint the facing term reads.  The skate and floor terms take minima over the feet markers with fminf, as
    the env kernel does, which drops a NaN marker; such a row is caught by the hand-off's non-finite counter when it is chosen.)"""
    N = len(costs)
    d = _inputs(world, POOL)
    pelvis = d["j127"].reshape(POOL, 20, 127, 3)[0, 19, 0].cpu()
    goal = torch.tensor([[0.3, -0.2, 0.9]])
    T0 = torch.zeros(N, 3)
    for n, c in enumerate(costs):
        T0[n] = goal[0] - pelvis - torch.tensor([c, 0.0, 0.0]) if np.isfinite(c) else torch.tensor([float("nan"), 0.0, 0.0])
    pene = torch.zeros(N, 20, dtype=torch.int32)
    pene[:, 3] = 39
    for n, cflag in enumerate(coll):
        if cflag:
            pene[n, 11] = 40
    x = {"rows": torch.zeros(N, dtype=torch.long), "R0": torch.eye(3).repeat(N, 1, 1), "T0": T0, "goal": goal, "pene": pene, "pool": d,
         "b": 1, "N": N}
    return x


def _selection_args(x, b, M, group0, jpb, rf, weights, pene_thres, goal_thresh, nan_face_rows):
    """The groups [group0, group0 + b) of M rows each of the row set x as a selection entry reads them, and NaN / -7 filled per-row
    outputs -> (the entry's sixteen leading arguments, the inputs as launched, the outputs, what else must outlive the launch)"""
    from egogen_amd._lib import ptr
    sl = slice(group0 * M, (group0 + b) * M)
    rows = x["rows"][sl].cuda()
    d = x["pool"]
    n = b * M
    per = lambda t: t.reshape(POOL, 20, *t.shape[1:])[rows].reshape(n * 20, *t.shape[1:]).contiguous()
    Yg = d["Y_gen"][:, rows].contiguous()
    X = d["X"][:, rows].contiguous()
    J = per(d["j127"] if jpb == 127 else d["j55"])
    for r in nan_face_rows:         # joint 2 of the last body: the facing term of row r becomes NaN, its distance stays finite
        J.view(n, 20, jpb, 3)[r, 19, 2, 0] = float("nan")
    mp = per(d["mproj"])
    R0, T0 = x["R0"][sl].cuda().contiguous(), x["T0"][sl].cuda().contiguous()
    goal = x["goal"][group0:group0 + b].cuda().contiguous()
    pene = None if x["pene"] is None else x["pene"][sl].cuda().reshape(-1).contiguous()
    feet = torch.tensor(_feet(), dtype=torch.int32, device="cuda")
    w = (C.c_float * 5)(*[weights[k] for k in W_ORDER])
    o = {"cost": torch.full((b, M), float("nan"), device="cuda"), "terms": torch.full((b, M, 5), float("nan"), device="cuda"),
         "colliding": torch.full((b, M), -7, dtype=torch.int32, device="cuda")}
    lead = (ptr(Yg), _vp(X[0]), _vp(X[1]), 201, ptr(J), jpb, ptr(mp), ptr(R0), ptr(T0), ptr(pene), ptr(goal), ptr(feet), w, float(pene_thres),
            float(goal_thresh), float(rf))
    i = {"Y_gen": Yg, "X": X, "J": J.reshape(n, 20, jpb, 3), "mp": mp.reshape(n, 20, 67, 3), "R0": R0, "T0": T0,
         "goal_rows": goal.repeat_interleave(M, 0), "pene": None if pene is None else pene.reshape(n, 20)}
    return lead, i, o, (goal, feet, w)


def _select(x, jpb, rf=CFG_RF, weights=W_TEST, pene_thres=40.0, goal_thresh=0.1, nan_face_rows=(), b=None, N=None, group0=0):
    """egx_primitive_select on the groups [group0, group0 + b) of the row set x -> (outputs, the inputs as launched)"""
    from egogen_amd import _lib
    b = x["b"] if b is None else b
    N = x["N"] if N is None else N
    lead, i, o, _alive = _selection_args(x, b, N, group0, jpb, rf, weights, pene_thres, goal_thresh, nan_face_rows)
    fi = lambda *s: torch.full(s, -7, dtype=torch.int32, device="cuda")
    o = {"choice": fi(b), "status": fi(b), "reached": fi(b), "goal_dist": torch.full((b,), float("nan"), device="cuda"), **o}
    _lib.check(_lib.load().egx_primitive_select(
        *lead, b, N, _lib.ptr(o["choice"]), _lib.ptr(o["status"]), _lib.ptr(o["reached"]), _lib.ptr(o["goal_dist"]), _lib.ptr(o["cost"]),
        _lib.ptr(o["terms"]), _lib.ptr(o["colliding"]), _lib.current_stream_ptr()), "egx_primitive_select")
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in o.items()}, i


def _beam_select(x, W, N, jpb, acc=None, ncoll=None, rf=CFG_RF, weights=W_TEST, pene_thres=40.0, goal_thresh=0.1, nan_face_rows=(), b=None,
                 group0=0):
    """egx_primitive_beam_select on the groups [group0, group0 + b) of the row set x (W * N rows each) -> (outputs, inputs as
    launched); the inputs are those `_select` launches on"""
    from egogen_amd import _lib
    b = x["b"] if b is None else b
    assert x["N"] == W * N
    lead, i, o, _alive = _selection_args(x, b, W * N, group0, jpb, rf, weights, pene_thres, goal_thresh, nan_face_rows)
    acc = torch.zeros(b, W) if acc is None else acc
    ncoll = torch.zeros(b, W, dtype=torch.int32) if ncoll is None else ncoll
    acc_d, ncoll_d = acc.float().cuda().contiguous(), ncoll.int().cuda().contiguous()
    fi = lambda *s: torch.full(s, -7, dtype=torch.int32, device="cuda")
    ff = lambda *s: torch.full(s, float("nan"), device="cuda")
    o.update({"beam_row": fi(b, W), "parent": fi(b, W), "acc": ff(b, W), "ncoll": fi(b, W), "path_cost": ff(b, W), "status": fi(b, W),
              "goal_dist": ff(b, W), "reached": fi(b, W)})
    _lib.check(_lib.load().egx_primitive_beam_select(
        *lead, b, W, N, _lib.ptr(acc_d), _lib.ptr(ncoll_d), _lib.ptr(o["cost"]), _lib.ptr(o["terms"]), _lib.ptr(o["colliding"]),
        _lib.ptr(o["beam_row"]), _lib.ptr(o["parent"]), _lib.ptr(o["acc"]), _lib.ptr(o["ncoll"]), _lib.ptr(o["path_cost"]),
        _lib.ptr(o["status"]), _lib.ptr(o["goal_dist"]), _lib.ptr(o["reached"]), _lib.current_stream_ptr()), "egx_primitive_beam_select")
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in o.items()}, i


def _restate(i, b, N, rf, weights, pene_thres, dtype):
    from tests import genop_search_ref as sref
    r = sref.score(i["Y_gen"], i["X"], i["J"], i["mp"], i["R0"], i["T0"], i["pene"], i["goal_rows"], _feet(), weights, pene_thres, rf, dtype)
    terms = torch.stack([r[t] for t in sref.TERMS], -1).reshape(b, N, 5)
    return r["cost"].reshape(b, N), terms, r["colliding"].reshape(b, N)


# ---- the observe launches of csrc/genop_policy.hip -------------------------------------------------------------------
RAY_LEN, MAX_DEPTH = 7.0, 13


def _poly_dev(poly):
    """(edges, edge_off, scene_idx, ...) as numpy or None -> the four polygon arguments of an observe entry, on the device"""
    if poly is None:
        return (None, None, None, 0)
    dev = lambda a, dtype: torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda().contiguous()
    return (dev(poly[0], torch.float32), dev(poly[1], torch.int32), dev(poly[2], torch.int32), len(poly[1]) - 1)


def _observe_lead(g, fpr, first, N, choice, x_ld, poly, step, b, ray_len=RAY_LEN, max_depth=MAX_DEPTH):
    """the arguments the two observe entries share, up to num_sequences; g: the device tensors joints, R_prev, T_prev, R0, T0, x0,
    x1 and goal by name, poly: what `_poly_dev` returns"""
    return (_vp(g["joints"]), fpr, first, _vp(choice), N, _vp(g["R_prev"]), _vp(g["T_prev"]), _vp(g["R0"]), _vp(g["T0"]), _vp(g["x0"]), _vp(g["x1"]),
            x_ld, _vp(g["goal"]), *[_vp(t) if torch.is_tensor(t) else t for t in poly], float(ray_len), int(step), int(max_depth), b)


def _observe_outputs(b):
    """NaN-filled state, egosensing, dist, time"""
    f = lambda *s: torch.full(s, float("nan"), device="cuda")
    return (f(b, 2, 402), f(b, 2, 32), f(b), f(b))


def _observe(g, fpr, first, N, choice, x_ld, poly, step, b, **kw):
    """egx_primitive_observe into NaN-filled outputs -> state, egosensing, dist, time (device tensors)"""
    from egogen_amd import _lib
    o = _observe_outputs(b)
    _lib.check(_lib.load().egx_primitive_observe(*_observe_lead(g, fpr, first, N, choice, x_ld, poly, step, b, **kw), *[_vp(t) for t in o],
                                                 _lib.current_stream_ptr()), "egx_primitive_observe")
    torch.cuda.synchronize()
    return o


def _check_rays(name, group, got, ego64, undecidable):
    from tests.genop_policy_ref import EGO_FLOOR
    keep = ~undecidable
    assert float(undecidable.float().mean()) <= UNDECIDABLE_CAP, (name, group, int(undecidable.sum()))
    err = (got.cpu().double() - ego64.double()).abs()[keep]
    print(f"| {name} | {group} | rays {int(keep.sum())} of {keep.numel()} | max error {float(err.max()):.3e} | floor {EGO_FLOOR:.1e} |")
    assert float(err.max()) <= EGO_FLOOR, (name, group, float(err.max()))
