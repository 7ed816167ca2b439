"""The geometry operators around an env step (csrc/env.hip: egx_canonical_frame, egx_update_transl_glorot, egx_env_get_feature,
egx_env_get_map, egx_assemble_params; csrc/nets.hip: egx_cont6d_to_aa), called through the C ABI and held to the float64
references of tests/env_ops_ref.py at their ragged sizes, edge inputs and modes.

Three kinds of bound, none taken from what a kernel returned:
  exact      torch.equal where a kernel moves data or does one IEEE operation per element;
  yardstick  per output group 3 * max|ref32 - ref64| + 2^-23 * max|ref64|, ref32 the same reference in fp32 on the CPU, over the
             operator's whole master input (every shape is a leading block of it); rotation outputs in groups by angle, rows
             within |q0| < 1e-4 of theta = pi compared as rotation matrices;
  same side  the map equals the reference's on every cell but the undecided ones (some |d_k| within the derived fp32 bound of
             that expression, env_ops_ref.map_band); in the exact sub-case on every cell.
Every launch gets valid arguments (fresh contiguous device copies kept alive across it); output buffers are sentinel-filled and
two rows (and columns, where the pitch is free) larger than the kernel may write, and those must come back untouched.  With
EGX_ENV_OPS_TABLE=<file> the per-group table is appended to that file: profiles/env_ops_float64.md.
"""
import ctypes as C

import pytest
import torch

from tests import env_ops_ref as er

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
SENT = -77.25


@pytest.fixture(scope="module")
def L():
    from egogen_amd import _lib
    _lib.load()
    return _lib


def _dev(*ts):
    """Device copies that the caller keeps alive until the launch has run (a temporary's block may be handed out again)."""
    out = tuple(None if t is None else t.detach().clone().contiguous().cuda() for t in ts)
    return out if len(out) > 1 else out[0]


def _padded(rows, *tail, extra=2):
    """A sentinel-filled device tensor with `extra` rows more than the kernel may write."""
    return torch.full((rows + extra,) + tuple(tail), SENT, dtype=F32, device="cuda")


def _untouched(t, rows):
    return bool((t[rows:] == SENT).all())


def _call(L, name, *args):
    L.check(getattr(L.load(), name)(*args, L.current_stream_ptr()), name)
    torch.cuda.synchronize()


def _refused(L, name, *args):
    """The entry point must refuse these arguments (EgxError) before it launches anything."""
    with pytest.raises(L.EgxError):
        L.check(getattr(L.load(), name)(*args, L.current_stream_ptr()), name)
    torch.cuda.synchronize()


def _hold(title, rows):
    """Print / record the table, then hold every row (group, max|f64|, err32, bound, kernel's error) to its bound."""
    er.emit(er.table(title, rows))
    for g, _, _, bound, err in rows:
        assert err <= bound, (title, g, err, bound)


def _group_rows(grp, err, label):
    return [(f"{label} {g}", grp.scale[g], grp.err32[g], grp.bound(g), e) for g, e in err.items()]


# ---------------------------------------------------------------------------------------------------------------------------
# egx_canonical_frame
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("jpb", er.FRAME_JPB)
@pytest.mark.parametrize("B", [1, 128, 129, 300])
def test_canonical_frame(L, B, jpb):
    """One thread per body, 128 per block: one body, one full block, one body into the second block, a ragged third block; the
    stride between bodies is joints_per_body * 3.  R: yardstick; its third row and column are (0, 0, 1) and T is joint 0, exactly."""
    grp = er.frame_group()
    j = _dev(er.frame_master()[:B, :jpb])
    Rg, Tg = _padded(B, 3, 3), _padded(B, 3)
    _call(L, "egx_canonical_frame", L.ptr(j), jpb, B, L.ptr(Rg), L.ptr(Tg))
    assert _untouched(Rg, B) and _untouched(Tg, B)
    assert torch.equal(Tg[:B], j[:, 0])
    e3 = torch.tensor([0.0, 0.0, 1.0], device="cuda").expand(B, 3)
    assert torch.equal(Rg[:B, 2, :], e3) and torch.equal(Rg[:B, :, 2], e3)
    err = grp.error({"R": Rg[:B], "T": Tg[:B]}, pick=lambda g, ref: ref[:B])
    assert err["T"] == 0.0
    _hold(f"egx_canonical_frame B={B} joints_per_body={jpb}", _group_rows(grp, {"R": err["R"]}, f"frame B={B} jpb={jpb}"))


# ---------------------------------------------------------------------------------------------------------------------------
# egx_update_transl_glorot
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_body", [False, True], ids=["frames=1", "frames=B"])
@pytest.mark.parametrize("B", [1, 127, 129, 300])
def test_update_transl_glorot(L, B, per_body):
    """One thread per body, 128 per block: a block short of one body, one body into the second block, a ragged third block, with
    one frame for all and one per body, out of place and in place (out == xb).  transl and the angle groups of glorot: yardstick
    (rows at theta = pi as matrices); columns 6.. equal the input bit for bit; both calls give the same bits in columns 0..5."""
    grp, split = er.transl_glorot_case(per_body)
    Rm, Tm, dm, xm, _ = er.transl_glorot_master()
    F = B if per_body else 1
    Rf, Tf, delta, xb = _dev(Rm[:F], Tm[:F], dm[:B], xm[:B])
    keep = [t.clone() for t in (Rf, Tf, delta, xb)]
    out = _padded(B, 93)
    _call(L, "egx_update_transl_glorot", L.ptr(Rf), L.ptr(Tf), F, L.ptr(delta), L.ptr(xb), B, L.ptr(out))
    assert _untouched(out, B) and all(torch.equal(a, b) for a, b in zip((Rf, Tf, delta, xb), keep))
    assert torch.equal(out[:B, 6:], xb[:, 6:])
    inplace = _padded(B, 93)
    inplace[:B] = xb
    _call(L, "egx_update_transl_glorot", L.ptr(Rf), L.ptr(Tf), F, L.ptr(delta), L.ptr(inplace), B, L.ptr(inplace))
    assert _untouched(inplace, B) and torch.equal(inplace[:B, 6:], xb[:, 6:])
    assert torch.equal(inplace[:B, :6], out[:B, :6])
    assert torch.isfinite(out[:B]).all()
    pick = er.block_pick(split, B, other=lambda g, ref: ref[:B])
    err = grp.error(er.transl_glorot_out(out, split, B), pick)
    _hold(f"egx_update_transl_glorot B={B} num_frames={F}", _group_rows(grp, err, f"transl_glorot B={B} frames={'B' if per_body else '1'}"))


# ---------------------------------------------------------------------------------------------------------------------------
# egx_env_get_feature
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_body", [False, True], ids=["wpath_rows=1", "wpath_rows=nb"])
@pytest.mark.parametrize("nb,nt,nm", [(1, 1, 1), (5, 2, 67), (3, 20, 67), (130, 1, 2)])
def test_env_get_feature(L, nb, nt, nm, per_body):
    """One thread per (body, frame, marker or pelvis), 256 per block: 2 threads, 680 and 4080 (ragged), 390 with 130 bodies (the
    body index runs through two blocks).  Both outputs: yardstick, bodies near their target and far from it in groups of their
    own; with either output NULL the other is bit-identical to the call with both."""
    grp, near, far = er.feature_case(per_body)
    Ym, pm, Rm, Tm, wm = er.feature_master()
    W = nb if per_body else 1
    Y_l, pel, R0, T0, wp = _dev(Ym[:nb, :nt, :nm], pm[:nb, :nt], Rm[:nb], Tm[:nb], wm[:W])
    outs = []
    for want_dist, want_fea in ((True, True), (False, True), (True, False)):
        dist, fea = _padded(nb, nt), _padded(nb, nt, nm * 3)
        _call(L, "egx_env_get_feature", L.ptr(Y_l), L.ptr(pel), L.ptr(R0), L.ptr(T0), L.ptr(wp), W, nb, nt, nm,
              L.ptr(dist) if want_dist else None, L.ptr(fea) if want_fea else None)
        assert _untouched(dist, nb if want_dist else 0) and _untouched(fea, nb if want_fea else 0)
        outs.append((dist, fea))
    (dist, fea), (_, fea_only), (dist_only, _) = outs
    assert torch.equal(fea_only[:nb], fea[:nb]) and torch.equal(dist_only[:nb], dist[:nb])
    got = er.feature_split({"dist": dist[:nb], "fea": fea[:nb].reshape(nb, nt, nm, 3)}, near, far, nb)
    err = grp.error(got, er.feature_pick(near, far, nb, nt, nm))
    _hold(f"egx_env_get_feature nb={nb} nt={nt} nm={nm} wpath_rows={W}", _group_rows(grp, err, f"feature {nb}x{nt}x{nm} wpath_rows={'nb' if per_body else '1'}"))
    # the marker and the pelvis that sit exactly on the target: the 1e-12 clamp, 0 / 1e-12 = 0
    assert float(dist[0, 0]) == float(torch.tensor(1e-12, dtype=F32)) and bool((fea[0, 0, :3] == 0).all())


# ---------------------------------------------------------------------------------------------------------------------------
# egx_env_get_map
# ---------------------------------------------------------------------------------------------------------------------------
def _get_map(L, tris, floor_h, lin, Rf, Tf, with_points):
    nb, res = Rf.shape[0], lin.numel()
    t, ln, Rd, Td = _dev(tris.reshape(-1, 6), lin, Rf, Tf)
    ps, mp = _padded(nb, res * res, 3), _padded(nb, res * res)
    _call(L, "egx_env_get_map", L.ptr(t), int(t.shape[0]), C.c_float(floor_h), L.ptr(ln), res, L.ptr(Rd), L.ptr(Td), nb,
          L.ptr(ps) if with_points else None, L.ptr(mp))
    assert _untouched(ps, nb if with_points else 0) and _untouched(mp, nb)
    return ps[:nb], mp[:nb]


@pytest.mark.parametrize("with_points", [True, False], ids=["points", "points=NULL"])
@pytest.mark.parametrize("nb,res,num_tris", er.MAP_CASES)
def test_env_get_map(L, nb, res, num_tris, with_points):
    """One thread per (body, cell), 256 per block: one cell; 45 cells of a 3 x 3 grid; 17 x 256 (the body index runs through
    seventeen blocks); a single triangle.  The map is 1 / -1 and equals the reference's outside the undecided cells (their share is
    capped at 1 % by the CPU test); points_scene xy: yardstick, z == floor_height; without points_scene the same map, bit for bit."""
    tris, floor_h, lin, Rm, Tm, grp, walk, und = er.map_case(res, num_tris)
    ps, mp = _get_map(L, tris, floor_h, lin, Rm[:nb], Tm[:nb], with_points)
    assert bool(((mp == 1.0) | (mp == -1.0)).all())
    want = torch.where(walk[:nb], 1.0, -1.0)
    decided = ~und[:nb]
    assert torch.equal(mp.cpu()[decided], want[decided])
    if not with_points:
        _, mp2 = _get_map(L, tris, floor_h, lin, Rm[:nb], Tm[:nb], True)
        assert torch.equal(mp, mp2)
        return
    assert bool((ps[:, :, 2] == torch.tensor(floor_h, dtype=F32)).all())
    err = grp.error({"points_xy": ps[:, :, :2]}, pick=lambda g, ref: ref[:nb])
    _hold(f"egx_env_get_map nb={nb} res={res} triangles={num_tris}", _group_rows(grp, err, f"map {nb}x{res}x{res} tris={num_tris}"))


def test_env_get_map_exact_case(L):
    """Quarter turns, dyadic translations, grid and vertices: every operation of the kernel is exact, so the scene points equal the
    float64 reference bit for bit and the map equals it on every cell, those exactly on an edge or a vertex included."""
    tris, floor_h, lin, Rf, Tf, o = er.map_exact_case()
    ps, mp = _get_map(L, tris, floor_h, lin, Rf, Tf, True)
    assert torch.equal(ps[:, :, :2].cpu().double(), o["points_xy"]) and bool((ps[:, :, 2] == floor_h).all())
    assert torch.equal(mp.cpu(), torch.where(o["map"], 1.0, -1.0))
    on_edge, on_vertex = er.map_on_boundary(tris, o["points_xy"])
    assert int(on_edge.sum()) > 0 and int(on_vertex.sum()) > 0 and bool((mp.cpu()[on_edge | on_vertex] == 1.0).all())


# ---------------------------------------------------------------------------------------------------------------------------
# egx_assemble_params
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", [1, 3, 11])
def test_assemble_params(L, A):
    """One thread per (agent, column), 256 per block: 93, 279 and 1023 threads, all ragged.  Copies, and for columns >= 6 of frames
    2 and 3 one IEEE addition and an exact halving each: torch.equal with the reference in fp32."""
    seed_m, Yb_m = er.assemble_master()
    seed, Yb = _dev(seed_m[:A], Yb_m[:, :A])
    out = _padded(A, 20, 93)
    _call(L, "egx_assemble_params", L.ptr(seed), L.ptr(Yb), A, L.ptr(out))
    assert _untouched(out, A)
    assert torch.equal(out[:A].cpu(), er.assemble_ref(seed_m[:A], Yb_m[:, :A]))


# ---------------------------------------------------------------------------------------------------------------------------
# egx_cont6d_to_aa
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 11, 12, 300])
def test_cont6d_to_aa(L, n):
    """One thread per (row, joint or pass-through item), 256 per block: 23 threads, 253 (three short of a block), 276 (a second
    block), 6900 (ragged).  Axis-angles: yardstick by angle group (rows at theta = pi as matrices, collinear columns only finite);
    transl and hands: the input's bits.  At out_ld = 96 and 160 the same bits as at 93 and the padding columns keep the sentinel;
    Cont6dToAaFn's forward returns the same bits."""
    from egogen_amd.fused_ops import Cont6dToAaFn
    grp, split = er.cont6d_case()
    xb6 = _dev(er.cont6d_master()[0][:n])
    outs = {}
    for ld in (93, 96, 160):
        out = _padded(n, ld)
        _call(L, "egx_cont6d_to_aa", L.ptr(xb6), n, L.ptr(out), ld)
        assert _untouched(out, n) and bool((out[:n, 93:] == SENT).all())
        outs[ld] = out[:n, :93]
    assert torch.equal(outs[96], outs[93]) and torch.equal(outs[160], outs[93])
    out = outs[93]
    assert torch.isfinite(out).all()
    assert torch.equal(out[:, :3], xb6[:, :3]) and torch.equal(out[:, 69:], xb6[:, 135:])
    assert torch.equal(Cont6dToAaFn.apply(xb6.clone()), out)
    err = grp.error(er.cont6d_out(out, split, n), er.block_pick(split, n * 22))
    _hold(f"egx_cont6d_to_aa n={n}", _group_rows(grp, err, f"cont6d n={n}"))


# ---------------------------------------------------------------------------------------------------------------------------
# argument checks: refused before anything is launched
# ---------------------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments(L):
    p = L.ptr
    x = torch.full((4096,), SENT, device="cuda")      # stands for every array; no call below may touch it
    a = p(x)
    # egx_canonical_frame(joints, joints_per_body, num_bodies, out_R, out_T)
    for args in ((None, 3, 1, a, a), (a, 3, 1, None, a), (a, 3, 1, a, None), (a, 2, 1, a, a), (a, 3, 0, a, a)):
        _refused(L, "egx_canonical_frame", *args)
    # egx_update_transl_glorot(R, T, num_frames, delta_T, xb, num_bodies, out)
    ok = [a, a, 1, a, a, 4, a]
    for i in (0, 1, 3, 4, 6):
        _refused(L, "egx_update_transl_glorot", *[None if k == i else v for k, v in enumerate(ok)])
    for frames, bodies in ((2, 4), (3, 4), (0, 4), (5, 4), (1, 0)):
        _refused(L, "egx_update_transl_glorot", a, a, frames, a, a, bodies, a)
    # egx_env_get_feature(Y_l, pel, R0, T0, wpath, wpath_rows, nb, nt, nm, out_dist_xyz, out_fea_marker)
    ok = [a, a, a, a, a, 1, 3, 2, 5, a, a]
    for i in range(5):
        _refused(L, "egx_env_get_feature", *[None if k == i else v for k, v in enumerate(ok)])
    for rows, nb, nt, nm in ((2, 3, 2, 5), (0, 3, 2, 5), (4, 3, 2, 5), (1, 0, 2, 5), (1, 3, 0, 5), (1, 3, 2, 0)):
        _refused(L, "egx_env_get_feature", a, a, a, a, a, rows, nb, nt, nm, a, a)
    # egx_env_get_map(tris, num_tris, floor_height, map_lin, res, R, T, num_bodies, out_points_scene, out_local_map)
    ok = [a, 2, C.c_float(0.0), a, 3, a, a, 2, a, a]
    for i in (0, 3, 5, 6, 9):
        _refused(L, "egx_env_get_map", *[None if k == i else v for k, v in enumerate(ok)])
    for i in (1, 4, 7):
        _refused(L, "egx_env_get_map", *[0 if k == i else v for k, v in enumerate(ok)])
    # egx_assemble_params(seed, Yb_gen, num_agents, pred_params)
    for args in ((None, a, 1, a), (a, None, 1, a), (a, a, 1, None), (a, a, 0, a)):
        _refused(L, "egx_assemble_params", *args)
    # egx_cont6d_to_aa(xb6, num_rows, out, out_ld)
    for args in ((None, 1, a, 93), (a, 1, None, 93), (a, 0, a, 93), (a, 1, a, 92)):
        _refused(L, "egx_cont6d_to_aa", *args)
    torch.cuda.synchronize()
    assert bool((x == SENT).all())
