"""The references, input builders and bounds of tests/env_ops_ref.py, checked on the CPU: (a) the references reproduce the
reference-generated goldens, (b) the designed inputs hold what they promise - both caps included -, (c) the bounds reject wrong
kernels: each named wrong variant of a reference, evaluated in float32 on the CPU, exceeds the bound of at least one group on the
master.  A GPU test that compares a kernel with these references (test_env_ops_gpu.py) is only as good as they are."""
import math

import numpy as np
import pytest
import torch

from oracle import rot
from tests import env_ops_ref as er
from tests.helpers import load_golden, max_abs

F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope="module", autouse=True)
def _cases():
    """Every master and group is built (and cached) with the oracle as it is, before any test swaps a wrong variant into it."""
    for per_body in (False, True):
        er.transl_glorot_case(per_body)
        er.feature_case(per_body)
    er.cont6d_case()
    er.frame_group()
    for _, res, nt in er.MAP_CASES:
        er.map_case(res, nt)


# ---------------------------------------------------------------------------------------------------------------------------
# (a) the references reproduce the goldens, at the tolerances of the existing tests
# ---------------------------------------------------------------------------------------------------------------------------
def test_frame_reference_reproduces_canon_golden():
    g = load_golden("canon_ref.npz")
    o = er.canonical_frame_ref(torch.from_numpy(g["jts"]))
    assert max_abs(o["R"].numpy(), g["R"]) < 1e-6 and max_abs(o["T"].numpy(), g["T"][:, 0]) == 0.0


def test_feature_reference_reproduces_feature_golden():
    g = load_golden("feature_ref.npz")
    t = lambda k: torch.from_numpy(g[k])
    nb, nt = g["pel"].shape[:2]
    o = er.feature_ref(t("Y_l").reshape(nb, nt, 67, 3), t("pel"), t("R0"), t("T0").reshape(nb, 3), t("wpath"), per_body=False)
    assert max_abs(o["dist"].numpy(), g["dist_xyz"][:, :, 0]) == 0.0
    assert max_abs(o["fea"].reshape(nb, nt, 201).numpy(), g["fea_marker_3d_n"]) == 0.0
    assert float(o["dist"].min()) == pytest.approx(1e-12)
    assert max_abs(er.assemble_ref(t("blend_in")[:2].permute(1, 0, 2), t("blend_in")[2:]).permute(1, 0, 2).numpy(), g["blend_out"]) == 0.0


def test_map_reference_reproduces_getmap_golden():
    g = load_golden("getmap_ref.npz")
    o = er.map_ref(torch.from_numpy(g["tris"]), torch.from_numpy(g["R"]), torch.from_numpy(g["T"]).reshape(-1, 3), 16, 0.8, float(g["floor_height"]))
    assert max_abs(o["points_xy"].numpy(), g["points_scene"][:, :, :2]) < 1e-6
    assert max_abs(o["z"].numpy(), g["points_scene"][:, :, 2]) == 0.0
    assert np.array_equal(o["map"].numpy(), g["map"]) and np.array_equal(np.where(o["map"].numpy(), 1.0, -1.0), g["box_local_map"])
    assert torch.equal(er.map_lin(16), torch.linspace(-0.8, 0.8, 16))


def test_rotation_references_reproduce_rot2aa_and_aa2rot_goldens():
    g = load_golden("rot2aa_ref.npz")
    n = g["aa_in"].shape[0]
    xb = torch.zeros(n, 93)
    xb[:, 3:6] = torch.from_numpy(g["aa_in"])
    out = er.transl_glorot_ref(torch.eye(3)[None], torch.zeros(1, 3), torch.zeros(n, 3), xb, per_body=False)
    theta = np.linalg.norm(g["aa_in"], axis=1)
    err = np.abs(out[:, 3:6].numpy() - g["aa_out"]).max(axis=1)
    assert err[theta < 2.0].max() < 1e-6 and err.max() < 5e-6, (err[theta < 2.0].max(), err.max())
    # the 6D reference on the first two columns of the same rotations
    Rm = torch.from_numpy(g["R"])[:n // 22 * 22]
    xb6 = torch.zeros(n // 22, 159)
    xb6[:, 3:135] = torch.stack([Rm[:, :, 0], Rm[:, :, 1]], -1).reshape(-1, 132)
    err6 = np.abs(er.cont6d_ref(xb6)[:, 3:69].reshape(-1, 3).numpy() - g["aa_out"][:Rm.shape[0]]).max(axis=1)
    assert err6[theta[:Rm.shape[0]] < 2.0].max() < 1e-6 and err6.max() < 5e-6
    g = load_golden("aa2rot_ref.npz")
    assert max_abs(er.AA2R(torch.from_numpy(g["aa"])).numpy(), g["R"]) < 1e-6       # what the matrix comparison applies


# ---------------------------------------------------------------------------------------------------------------------------
# (b) what the masters promise
# ---------------------------------------------------------------------------------------------------------------------------
def _tg_matrices(per_body):
    Rf, _, _, xb, kinds = er.transl_glorot_master()
    return er._tg_matrix(Rf if per_body else Rf[:1], xb[:, 3:6]), kinds


def _rotation_masters():
    """(name, float64 matrices whose diagonal decides the branches, kinds, RotSplit) of the three rotation masters."""
    xb6, slot_kind = er.cont6d_master()
    yield "cont6d", er._cont_matrix(xb6[:, 3:135].reshape(-1, 6)), slot_kind, er.cont6d_case()[1]
    for per_body in (False, True):
        M, kinds = _tg_matrices(per_body)
        yield f"transl_glorot per_body={per_body}", M, kinds, er.transl_glorot_case(per_body)[1]


def test_matrix_share_is_capped_and_every_branch_occurs_on_vector_rows():
    for name, M, kinds, split in _rotation_masters():
        assert 0 < split.matrix_share <= er.MATRIX_SHARE_CAP, (name, split.matrix_share)
        for g in er.ANGLE_GROUPS:
            assert len(split.idx[g]) > 0, (name, g)
        vec = torch.cat([split.idx[g] for g in er.ANGLE_GROUPS[:-1]])
        br, q0 = er.quat_branch(M[vec]), er.quat64(M[vec])[:, 0]
        assert sorted(set(br.tolist())) == [0, 1, 2, 3], name
        for b in range(3):          # branch 3 has q0 = t > 0 by construction
            assert bool((q0[br == b] < 0).any()) and bool((q0[br == b] > 0).any()), (name, b)
        assert float(q0.abs().min()) >= er.Q0_BAND
        # the matrix rows are the ones at theta = pi: within 2.1e-4 of it, on both signs of q0
        mat = split.idx[er.ANGLE_GROUPS[-1]]
        qm = er.quat64(M[mat])[:, 0]
        assert bool((qm < 0).any()) and bool((qm > 0).any()) and float(qm.abs().max()) < er.Q0_BAND


def test_threshold_rows_sit_inside_the_window_on_both_sides():
    for name, M, kinds, split in _rotation_masters():
        seen = set()
        for which in er.THRESHOLDS:
            for side, sign in (("+", 1.0), ("-", -1.0)):
                rows = [i for i, k in enumerate(kinds) if k.endswith(which + side) and
                        (name == "cont6d" or k.startswith("in:") or k.startswith("outb:" if "True" in name else "out0:"))]
                if name.endswith("False"):     # with one frame for all, the `in` rows (identity frames of their own) are not designed
                    rows = [i for i in rows if not kinds[i].startswith("in:")]
                if not rows:
                    continue
                mv, ok = er.threshold_measure(M[rows], which, margin=0.2)
                assert bool(ok.all()) and bool(((mv * sign) > 0).all()) and bool((mv.abs() < 1e-7).all()), (name, which, side, mv)
                seen.add((which, side))
        assert len(seen) == 6, (name, sorted(seen))


def test_theta2_rows_lie_a_few_ulps_on_both_sides_of_the_switch():
    _, _, _, xb, kinds = er.transl_glorot_master()
    rows = [i for i, k in enumerate(kinds) if k == "in:theta2"]
    ulp = float(np.spacing(np.float32(er.THETA2_SWITCH)))
    d = ((xb[rows, 3:6].double() ** 2).sum(1) - er.THETA2_SWITCH) / ulp
    assert int((d > 0).sum()) == 4 and int((d < 0).sum()) == 4 and float(d.abs().min()) > 3 and float(d.abs().max()) < 8
    t2_32 = (xb[rows, 3:6] ** 2).sum(1)
    assert torch.equal(t2_32 > 1e-6, d > 0)                      # the fp32 evaluation stands on the same side
    # and the whole master: angles on both sides by decades, down to 1e-7
    th = xb[:, 3:6].double().norm(dim=1)
    assert float(th.min()) < 2e-7 and int(((th > 1e-3) & (th < 3.2e-3)).sum()) >= 2 and int(((th > 3.2e-3) & (th < 1e-2)).sum()) >= 2


def test_pi_rows_and_zero_and_collinear_columns_are_what_they_claim():
    aa, kinds = er.rotation_rows()
    pi_rows = aa[[i for i, k in enumerate(kinds) if k == "pi"]]
    assert pi_rows.shape[0] == 8 and torch.allclose(pi_rows.norm(dim=1), torch.full((8,), math.pi, dtype=F64), rtol=0, atol=1e-15)
    assert int((pi_rows.abs() == math.pi).sum()) == 6                                 # +-x, +-y, +-z
    xb6, slot_kind = er.cont6d_master()
    x6 = xb6[:, 3:135].reshape(-1, 3, 2)
    z1 = x6[[i for i, k in enumerate(slot_kind) if k == "zero1"]]
    z2 = x6[[i for i, k in enumerate(slot_kind) if k == "zero2"]]
    co = x6[[i for i, k in enumerate(slot_kind) if k == "collinear"]]
    assert z1.shape[0] == z2.shape[0] == co.shape[0] == 16
    assert bool((z1[:, :, 0] == 0).all()) and bool((z2[:, :, 1] == 0).all())
    for rest in (z1[:, :, 1], z2[:, :, 0]):      # unit column: every component >= 0.1, so m00 > m11 and q0 < 0 are > 1e-3 from a flip
        u = rest.double() / rest.double().norm(dim=1, keepdim=True)
        assert float(u.abs().min()) > 0.1
    ratio = co[:, :, 1].double() / co[:, :, 0].double()
    assert bool(((ratio == 2.0).all(dim=1) | (ratio == -0.5).all(dim=1)).all())
    grp, split = er.cont6d_case()
    held = torch.cat(list(split.idx.values()))
    for i, k in enumerate(slot_kind):
        if k == "collinear":
            assert i not in set(held.tolist())
    assert held.numel() == er.C6_N * 22 - 16 and torch.isfinite(grp.o32[er.ANGLE_GROUPS[1]]).all()
    for g in grp.groups:
        assert torch.isfinite(grp.o64[g]).all() and torch.isfinite(grp.o32[g]).all(), g


def test_frame_master_spans_the_pelvis_widths():
    j = er.frame_master().double()
    nxy = (j[:, 2, :2] - j[:, 1, :2]).norm(dim=1)
    assert float(nxy.min()) < 2e-4 and float(nxy.max()) > 0.9 and float(j[:, 0].abs().max()) > 7.0
    assert float((j[:, 2, 2] - j[:, 1, 2]).abs().median()) > 0.3


def test_feature_master_holds_the_clamp_rows_and_both_target_distances():
    Y_l, pel, R0, T0, wpath = er.feature_master()
    for per_body in (False, True):
        grp, near, far = er.feature_case(per_body)
        o = er.feature_ref(Y_l, pel, R0, T0, wpath, per_body)
        assert float(o["dist"][0, 0]) == pytest.approx(1e-12) and bool((o["fea"][0, 0, 0] == 0).all())
        assert len(near) > 0 and len(far) > 0 and 0 in near.tolist()
    d = er.feature_ref(*er.cast((Y_l, pel, R0, T0, wpath), F64), True)["dist"][:, 0]
    assert bool(((d[2::2] - 1e-3).abs() < 1e-5).all()) and bool(((d[1::2] - 10.0).abs() < 1e-4).all())
    assert float((wpath[1:] - wpath[:-1]).norm(dim=1).min()) > 1.0


def test_map_masters_hold_both_outcomes_and_few_undecided_cells():
    for nb, res, nt in er.MAP_CASES:
        tris, floor_h, lin, Rf, Tf, grp, walk, und = er.map_case(res, nt)
        for rows in (slice(0, nb), slice(0, er.MAP_NB)):
            share = float(walk[rows].float().mean())
            if res > 1:
                assert 0.2 <= share <= 0.8, (nb, res, nt, share)
            assert float(und[rows].float().mean()) <= er.UNDECIDED_CAP, (nb, res, nt)
        # where the fp32 reference disagrees with float64, the cell is undecided: the band covers the reference's own flips
        walk32 = er.map_ref(tris, Rf, Tf, res, er.MAP_EXTENT, floor_h)["map"]
        assert bool((und | (walk32 == walk)).all())
    one = [er.map_case(1, 1)[6][b, 0].item() for b in range(er.MAP_NB)]
    assert True in one and False in one


def test_map_band_flags_a_cell_that_sits_on_an_edge():
    """A frame whose origin lies on the hole's edge, res = 3 (the middle cell is the origin): that cell is undecided, and only
    cells of that kind are."""
    tris = er.map_meshes()[0][8]
    Rf, Tf = er.rotz(torch.tensor([0.3])).float(), torch.tensor([[1.3604892, 1.5, 0.0]])
    und = er.map_band(tris, Rf, Tf, 3, er.MAP_EXTENT)
    assert bool(und[0, 4]) and int(und.sum()) == 1


def test_exact_map_case_is_exact_and_touches_edges_and_vertices():
    tris, floor_h, lin, Rf, Tf, o = er.map_exact_case()
    assert lin.tolist() == [-1.0, -0.5, 0.0, 0.5, 1.0]
    o32 = er.map_ref(tris, Rf, Tf, er.EXACT_RES, er.EXACT_EXTENT, floor_h)
    assert torch.equal(o32["points_xy"].double(), o["points_xy"]) and torch.equal(o32["map"], o["map"])
    on_edge, on_vertex = er.map_on_boundary(tris, o["points_xy"])
    assert int(on_edge.sum()) >= 10 and int(on_vertex.sum()) >= 4 and bool(o["map"][on_edge | on_vertex].all())
    assert 0.2 < float(o["map"].float().mean()) < 0.8
    # the band of an exact case still flags the boundary cells (|d| = 0), which is why this sub-case does not use it
    assert bool(er.map_band(tris, Rf, Tf, er.EXACT_RES, er.EXACT_EXTENT)[on_edge | on_vertex].all())


def test_assemble_reference_is_the_kernels_order():
    seed, Yb = er.assemble_master()
    ref = er.assemble_ref(seed, Yb)
    b2 = (seed[:, 1, 6:] + Yb[1, :, 6:]) / 2.0
    b3 = (b2 + Yb[2, :, 6:]) / 2.0
    assert torch.equal(ref[:, 2, 6:], b2) and torch.equal(ref[:, 3, 6:], b3) and torch.equal(ref[:, 2:4, :6], Yb[:2, :, :6].permute(1, 0, 2))
    assert torch.equal(ref[:, :2], seed) and torch.equal(ref[:, 4:], Yb[2:].permute(1, 0, 2))


# ---------------------------------------------------------------------------------------------------------------------------
# (c) the bounds reject wrong kernels (every variant in float32 on the CPU)
# ---------------------------------------------------------------------------------------------------------------------------
def _exceeded(grp, out, pick=None):
    err = grp.error(out, pick)
    return {g: (e, grp.bound(g)) for g, e in err.items() if not e <= grp.bound(g)}


def _tg32(per_body_ref, per_body_run=None, transpose=False):
    """Groups the float32 reference exceeds when run with `per_body_run` frames (or R transposed) against mode `per_body_ref`."""
    Rf, Tf, delta, xb, _ = er.transl_glorot_master()
    grp, split = er.transl_glorot_case(per_body_ref)
    run = per_body_ref if per_body_run is None else per_body_run
    out = er.transl_glorot_ref(Rf.transpose(1, 2) if transpose else Rf, Tf, delta, xb, run)
    return _exceeded(grp, er.transl_glorot_out(out, split, er.TG_B))


def _c6_32(xb6=None):
    grp, split = er.cont6d_case()
    out = er.cont6d_ref(er.cont6d_master()[0] if xb6 is None else xb6)
    return _exceeded(grp, er.cont6d_out(out, split, er.C6_N))


def test_the_unmodified_float32_references_pass_their_own_bounds():
    assert not _tg32(False) and not _tg32(True) and not _c6_32()


def test_wrong_frame_row_is_rejected():
    bad = _tg32(True, per_body_run=False)       # frame 0 for every body where each has its own
    assert "transl" in bad and len(bad) >= 4, bad
    bad = _tg32(False, per_body_run=True)       # frame b where frame 0 serves every body
    assert "transl" in bad and len(bad) >= 4, bad


def test_untransposed_frame_is_rejected():
    for per_body in (False, True):
        bad = _tg32(per_body, transpose=True)
        assert "transl" in bad and len(bad) >= 3, bad
    Y_l, pel, R0, T0, wpath = er.feature_master()
    for per_body in (False, True):
        grp, near, far = er.feature_case(per_body)
        out = er.feature_split(er.feature_ref(Y_l, pel, R0.transpose(1, 2), T0, wpath, per_body), near, far)
        assert len(_exceeded(grp, out)) == 4


def test_wrong_target_row_is_rejected():
    m = er.feature_master()
    for per_body in (False, True):
        grp, near, far = er.feature_case(per_body)
        out = er.feature_split(er.feature_ref(*m, not per_body), near, far)
        bad = _exceeded(grp, out)
        assert "dist far" in bad and "fea far" in bad, bad


def test_wrong_joint_stride_is_rejected():
    j = er.frame_master()
    grp = er.frame_group()
    as22 = j.reshape(-1)[:er.FRAME_B * 22 * 3].view(er.FRAME_B, 22, 3)          # joints_per_body taken as 22 when it is 55
    bad = _exceeded(grp, er.canonical_frame_ref(as22))
    assert "R" in bad and "T" in bad, bad
    assert not _exceeded(grp, er.canonical_frame_ref(j[:, :3].contiguous()))     # the same bodies at another stride: same result


def test_wrong_blends_are_rejected():
    seed, Yb = er.assemble_master()
    ref = er.assemble_ref(seed, Yb)
    second_from_unblended = ref.clone()
    second_from_unblended[:, 3, 6:] = (Yb[0, :, 6:] + Yb[2, :, 6:]) / 2.0
    assert not torch.equal(second_from_unblended, ref)
    all_columns = ref.clone()
    all_columns[:, 2] = (seed[:, 1] + Yb[1]) / 2.0
    all_columns[:, 3] = (all_columns[:, 2] + Yb[2]) / 2.0
    assert torch.equal(all_columns[..., 6:], ref[..., 6:]) and not torch.equal(all_columns, ref)


def _aa2R_variant(eps, switch):
    """rot.tgm_angle_axis_to_rotation_matrix with the epsilon of the denominator and the Taylor switch as parameters."""
    def fn(aa):
        theta2 = (aa * aa).sum(dim=1, keepdim=True)
        theta = torch.sqrt(theta2)
        w = aa / (theta + eps)
        wx, wy, wz = w[:, 0:1], w[:, 1:2], w[:, 2:3]
        c, s = torch.cos(theta), torch.sin(theta)
        normal = torch.cat([c + wx * wx * (1 - c), wx * wy * (1 - c) - wz * s, wy * s + wx * wz * (1 - c),
                            wz * s + wx * wy * (1 - c), c + wy * wy * (1 - c), -wx * s + wy * wz * (1 - c),
                            -wy * s + wx * wz * (1 - c), wx * s + wy * wz * (1 - c), c + wz * wz * (1 - c)], dim=1).view(-1, 3, 3)
        rx, ry, rz = aa[:, 0:1], aa[:, 1:2], aa[:, 2:3]
        one = torch.ones_like(rx)
        taylor = torch.cat([one, -rz, ry, rz, one, -rx, -ry, rx, one], dim=1).view(-1, 3, 3)
        return torch.where((theta2 > switch).view(-1, 1, 1), normal, taylor)
    return fn


def _R2q_variant(swap_in):
    """rot.tgm_rotation_matrix_to_quaternion with two off-diagonal entries of branch `swap_in` exchanged."""
    def fn(Rm, eps=1e-6):
        m = Rm.transpose(1, 2)
        m00, m11, m22 = m[:, 0, 0], m[:, 1, 1], m[:, 2, 2]
        d2, d01, d0n1 = m22 < eps, m00 > m11, m00 < -m11
        rows = [[m[:, 1, 2] - m[:, 2, 1], 1 + m00 - m11 - m22, m[:, 0, 1] + m[:, 1, 0], m[:, 2, 0] + m[:, 0, 2]],
                [m[:, 2, 0] - m[:, 0, 2], m[:, 0, 1] + m[:, 1, 0], 1 - m00 + m11 - m22, m[:, 1, 2] + m[:, 2, 1]],
                [m[:, 0, 1] - m[:, 1, 0], m[:, 2, 0] + m[:, 0, 2], m[:, 1, 2] + m[:, 2, 1], 1 - m00 - m11 + m22],
                [1 + m00 + m11 + m22, m[:, 1, 2] - m[:, 2, 1], m[:, 2, 0] - m[:, 0, 2], m[:, 0, 1] - m[:, 1, 0]]]
        if swap_in is not None:
            i, j = {0: (2, 3), 1: (1, 3), 2: (1, 2), 3: (1, 2)}[swap_in]
            rows[swap_in][i], rows[swap_in][j] = rows[swap_in][j], rows[swap_in][i]
        br = torch.where(d2 & d01, 0, torch.where(d2, 1, torch.where(d0n1, 2, 3)))
        q = torch.stack([torch.stack(r, -1) for r in rows], 1)[torch.arange(Rm.shape[0]), br]
        t = torch.stack([rows[0][1], rows[1][2], rows[2][3], rows[3][0]], 1)[torch.arange(Rm.shape[0]), br]
        if swap_in is not None:      # t sits on the diagonal slot, which no swap touches
            t = torch.stack([1 + m00 - m11 - m22, 1 - m00 + m11 - m22, 1 - m00 - m11 + m22, 1 + m00 + m11 + m22], 1)[torch.arange(Rm.shape[0]), br]
        return q / torch.sqrt(t)[:, None] * 0.5
    return fn


def _q2aa_without_negative_case(q):
    q1, q2, q3 = q[..., 1], q[..., 2], q[..., 3]
    sin_sq = q1 * q1 + q2 * q2 + q3 * q3
    sin_t = torch.sqrt(sin_sq)
    k = torch.where(sin_sq > 0.0, 2.0 * torch.atan2(sin_t, q[..., 0]) / sin_t, 2.0 * torch.ones_like(sin_t))
    return torch.stack([q1 * k, q2 * k, q3 * k], -1)


def test_restated_conversions_are_the_oracles_own():
    """The parametrised restatements above, at the oracle's parameters, give the oracle's bits: what differs in a variant is the
    named change alone."""
    xb6, _ = er.cont6d_master()
    Rm32 = rot.cont2rotmat(xb6[:, 3:135].reshape(-1, 6))
    aa32 = er.transl_glorot_master()[3][:, 3:6]
    for dtype in (F32, F64):
        assert torch.equal(_aa2R_variant(1e-6, 1e-6)(aa32.to(dtype)), rot.tgm_angle_axis_to_rotation_matrix(aa32.to(dtype)))
        ok = ~torch.tensor([k == "collinear" for k in er.cont6d_master()[1]])
        assert torch.equal(_R2q_variant(None)(Rm32.to(dtype))[ok], rot.tgm_rotation_matrix_to_quaternion(Rm32.to(dtype))[ok])


def test_wrong_angle_axis_to_matrix_is_rejected(monkeypatch):
    """Without the + 1e-6 of the denominator (the smallest variant: about 1e-6 on the off-diagonals for theta in [1e-3, 1e-2], which
    the small-angle group exists for), and with the theta^2 switch at 1e-5.  The switch shows where the designed angle is the input's
    and the output's: the rows with an identity frame of their own, num_frames == B; the missing epsilon under either mode."""
    for variant in (_aa2R_variant(0.0, 1e-6), _aa2R_variant(1e-6, 1e-5)):
        monkeypatch.setattr(rot, "tgm_angle_axis_to_rotation_matrix", variant)
        bad = {**_tg32(False), **_tg32(True)}
        assert er.ANGLE_GROUPS[0] in bad, bad
        monkeypatch.undo()


def test_dropped_negative_q0_case_is_rejected(monkeypatch):
    monkeypatch.setattr(rot, "tgm_quaternion_to_angle_axis", _q2aa_without_negative_case)
    for bad in (_tg32(False), _tg32(True), _c6_32()):
        assert len(bad) >= 3, bad


@pytest.mark.parametrize("branch", [0, 1, 2, 3])
def test_swapped_quaternion_entries_are_rejected_in_every_branch(monkeypatch, branch):
    monkeypatch.setattr(rot, "tgm_rotation_matrix_to_quaternion", _R2q_variant(branch))
    for bad in (_tg32(False), _tg32(True), _c6_32()):
        assert bad, (branch, bad)


def test_wrong_6d_layout_and_wrong_cross_product_are_rejected(monkeypatch):
    xb6, _ = er.cont6d_master()
    x = xb6[:, 3:135].reshape(-1, 6)
    as23 = torch.stack([x[:, :3], x[:, 3:]], -1).reshape(-1, 132)        # the reference then reads a1 = x[0:3], a2 = x[3:6]
    bad = _c6_32(torch.cat([xb6[:, :3], as23, xb6[:, 135:]], 1))
    assert len(bad) >= 4, bad

    def cross_reversed(x6):
        a = x6.contiguous().view(-1, 3, 2)
        b1 = torch.nn.functional.normalize(a[:, :, 0], dim=1)
        b2 = torch.nn.functional.normalize(a[:, :, 1] - torch.sum(b1 * a[:, :, 1], dim=1, keepdim=True) * b1, dim=-1)
        return torch.stack([b1, b2, torch.cross(b2, b1, dim=1)], dim=-1)
    monkeypatch.setattr(rot, "cont2rotmat", cross_reversed)
    bad = _c6_32()
    assert len(bad) >= 4, bad
