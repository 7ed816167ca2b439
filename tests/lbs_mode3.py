"""Float64 emulation of the cheap evaluation of LBS blend mode 3 ("f16mix", csrc/lbs_fused3.hip), the kernel's fix-up band, and a
body built to defeat a statistical band.  TEST INFRASTRUCTURE ONLY (nothing under egogen_amd/ imports it).

The count-only vertex tiles of mode 3 evaluate the blend GEMM as
  * k-steps 1..28 (pose-corrective columns k = 16..463): ONE fp16 product - features R_j - I computed in fp32 by the pose kernel
    and rounded to fp16 (round to nearest even), bases fp32 -> fp16; fp16 x fp16 is exact in the fp32 accumulator;
  * k-steps 0 and 29 (10 betas, the other 11 pose columns, the template and its third bf16 term): two bf16 planes of each
    operand, products hi.hi + hi.mid + mid.hi;
and classify each vertex by its SDF value against a band of fix_e(body) x slope (pose kernel), inside which they re-evaluate in
fp32.  Here the products are exact and the sums float64: what is left is the operand rounding the band must cover.
`band()` mirrors the pose kernel's formula with the constants below (checked against the source by tests/test_lbs_mode3_cpu.py);
`statistical_band()` is the formula the kernel used before (ten standard deviations of independent roundings)."""
import numpy as np
import torch

from egogen_amd import synth

# mirrors of csrc/lbs.h (tests/test_lbs_mode3_cpu.py::test_band_constants_mirror_the_kernel)
LBS_FIX_SLACK_M = 3e-6
LBS_TWO_PLANE_ERR = 1.2e-5
LBS_ACC_ADDS_OFFSETS = 496.0
LBS_ACC_ADDS_LAST = 48.0
LBS_FIX_MARGIN = 1.001
LBS_SKIN_ERR = 2.0e-5

U16 = 2.0 ** -11
MOVABLE = [j for j in range(1, 55) if not 22 <= j <= 24]      # the 51 joints with blend features (compact order)
KCOL = 10 + np.arange(51 * 9)                                 # GEMM column of every pose feature
FP16_COL = (KCOL >= 16) & (KCOL < 464)                        # the columns of the fp16 k-steps


def f16(x):
    """fp32 -> fp16 (round to nearest even) -> float64"""
    return np.asarray(x, np.float32).astype(np.float16).astype(np.float64)


def bf16_planes(x):
    """hi, mid of egx_bf16_split3 (round to nearest even on the upper 16 bits of the fp32 pattern), as float64"""
    t = torch.as_tensor(np.asarray(x, np.float32))
    hi = t.to(torch.bfloat16).to(torch.float32)
    mid = (t - hi).to(torch.bfloat16).to(torch.float32)
    return hi.double().numpy(), mid.double().numpy()


def two_plane_product(f, b):
    fh, fm = bf16_planes(f)
    bh, bm = bf16_planes(b)
    return fh * bh + fh * bm + fm * bh


def _axis_angles_f32(bm, xb):
    """[55,3] fp32 axis-angle vectors of one parameter row, as egx_pose_chain_kernel forms them (hand PCA summed in order)"""
    x = np.asarray(xb, np.float32)
    a = np.zeros((55, 3), np.float32)
    a[0] = x[3:6]
    a[1:22] = x[6:69].reshape(21, 3)
    for side, key in ((0, "l"), (1, "r")):
        comps = np.asarray(bm["hand_comps_" + key], np.float32)
        mean = np.asarray(bm["hand_mean_" + key], np.float32)
        pca = x[69 + 12 * side: 81 + 12 * side]
        s = np.zeros(45, np.float32)
        for k in range(12):
            s = (s + pca[k] * comps[k]).astype(np.float32)
        a[25 + 15 * side: 40 + 15 * side] = (s + mean).reshape(15, 3)
    return a


def features_f32(bm, xb):
    """[51, 9] fp32 blend features R_j - I of one parameter row (rotations in fp32 with the pose kernel's formulas)"""
    a = _axis_angles_f32(bm, xb)
    e = (a + np.float32(1e-8)).astype(np.float32)
    ang = np.sqrt((e * e).sum(-1, dtype=np.float32)).astype(np.float32)
    r = (a / ang[:, None]).astype(np.float32)
    sn, cs = np.sin(ang).astype(np.float32), (np.float32(1) - np.cos(ang)).astype(np.float32)
    rx, ry, rz = r[:, 0], r[:, 1], r[:, 2]
    R = np.stack([cs * -(ry * ry + rz * rz), -sn * rz + cs * (rx * ry), sn * ry + cs * (rx * rz),
                  sn * rz + cs * (rx * ry), cs * -(rx * rx + rz * rz), -sn * rx + cs * (ry * rz),
                  -sn * ry + cs * (rx * rz), sn * rx + cs * (ry * rz), cs * -(rx * rx + ry * ry)], -1).astype(np.float32)
    # the kernel forms 1 + cs * (...) for the diagonal and subtracts 1 again: round through that sum as it does
    for d in (0, 4, 8):
        R[:, d] = ((np.float32(1) + R[:, d]).astype(np.float32) - np.float32(1)).astype(np.float32)
    return R[MOVABLE]


def _pose_block(bm):
    """[459, V, 3] fp32 pose-corrective columns of the movable joints in GEMM column order"""
    V = bm["v_template"].shape[0]
    P = np.asarray(bm["posedirs"], np.float32).reshape(54, 9, V, 3)
    return P[[j - 1 for j in MOVABLE]].reshape(51 * 9, V, 3)


def model_consts(bm):
    """the band constants the packing (csrc/lbs_pack.hip) derives from a model: float64, rounded up to fp32 as there
    (compared bit for bit by tests/test_lbs_pack_cpu.py)"""
    up = lambda x: np.float32(np.asarray(x, np.float64) * (1.0 + 1e-6)).astype(np.float64)
    P = _pose_block(bm).astype(np.float64)                                   # [459, V, 3]
    dP = np.where(FP16_COL[:, None, None], f16(P) - P, 0.0)
    Pall = np.asarray(bm["posedirs"], np.float64).reshape(54, 9, -1, 3)
    col = np.sqrt((Pall ** 2).sum(-1)).max(axis=(1, 2))                       # [54] joints 1..54
    colD = np.sqrt((dP ** 2).sum(-1)).reshape(51, 9, -1).max(axis=(1, 2))     # [51] movable
    S = np.asarray(bm["shapedirs"], np.float64)                               # [V, 3, 10]
    W = np.asarray(bm["lbs_weights"], np.float32).astype(np.float64)
    return {
        "C": up(col[[j - 1 for j in MOVABLE]]), "D": up(colD),
        "PF": float(up(np.sqrt((P ** 2).sum(axis=(0, 2)).max()))), "DPF": float(up(np.sqrt((dP ** 2).sum(axis=(0, 2)).max()))),
        "S": up(np.sqrt((S ** 2).sum(1)).max(0)),
        "vt_max": float(up(np.linalg.norm(np.asarray(bm["v_template"], np.float64), axis=1).max())),
        "w_abs_max": float(up(np.abs(W).sum(1).max())),
    }


def band(consts, F, betas, tn, skin=True):
    """fix_e of one body (metres): the pose kernel's hard bound (csrc/lbs_pose.hip; csrc/lbs.h, LBS_FIX_SLACK_M), float64.
    F [51, 9] fp32 features, betas [10], tn = max_j |t_j| of the body's joint transforms.  Returns (total, terms)."""
    F = np.asarray(F, np.float32).reshape(-1)
    Ft = f16(F)
    Fd = F.astype(np.float64)
    dF = Ft - Fd
    H = FP16_COL
    C9, D9 = np.repeat(consts["C"], 9), np.repeat(consts["D"], 9)
    cs = np.sqrt((dF[H] ** 2).sum()) * consts["PF"] + np.sqrt((Ft[H] ** 2).sum()) * consts["DPF"]
    l1 = (np.abs(dF[H]) * C9[H]).sum() + (np.abs(Ft[H]) * D9[H]).sum()
    shape = (np.abs(np.asarray(betas, np.float64)) * consts["S"]).sum()
    prod = min(cs, l1) + LBS_TWO_PLANE_ERR * ((np.abs(Fd[~H]) * C9[~H]).sum() + shape)
    offs = (shape + min(np.sqrt((Fd ** 2).sum()) * consts["PF"], (np.abs(Fd) * C9).sum())) * LBS_FIX_MARGIN
    vb = consts["vt_max"] + offs
    accr = 2.0 ** -24 * (LBS_ACC_ADDS_OFFSETS * offs + LBS_ACC_ADDS_LAST * vb)
    blend = consts["w_abs_max"] * (prod + accr) * LBS_FIX_MARGIN
    total = blend + LBS_FIX_SLACK_M + (LBS_SKIN_ERR * consts["w_abs_max"] * (vb + tn) * LBS_FIX_MARGIN if skin else 0.0)
    return total, {"cs": cs, "l1": l1, "prod": prod, "accr": accr, "blend": blend, "vb": vb}


def statistical_band(bm, F, tn):
    """fix_e of the kernel before the hard bound: 2 x 2^-11 sqrt(sum_j |R_j - I|_F^2 C_j^2) + 3e-6 + 1e-5 (max|v_template| + 0.25 + tn)"""
    c = model_consts(bm)
    Fj = np.asarray(F, np.float64).reshape(51, 9)
    q = ((Fj ** 2).sum(1) * c["C"] ** 2).sum()
    return 2.0 * U16 * np.sqrt(q) + 3e-6 + 1e-5 * (c["vt_max"] + 0.25 + tn)


def cheap_vposed(bm, F, betas, vids, P16=None):
    """[len(vids), 3] v_posed as the count-only tiles compute it (operand rounding exact, sums float64).  P16 = f16 of the fp16
    columns of _pose_block(bm)[:, vids], if the caller has it already."""
    vids = np.asarray(vids)
    F = np.asarray(F, np.float32).reshape(-1)
    P = _pose_block(bm)[:, vids]                                               # [459, n, 3] fp32
    P16 = f16(P[FP16_COL]) if P16 is None else P16
    out = np.einsum("k,knc->nc", f16(F)[FP16_COL], P16)
    out += np.einsum("knc->nc", two_plane_product(F[~FP16_COL][:, None, None], P[~FP16_COL]))
    S = np.asarray(bm["shapedirs"], np.float32)[vids]                          # [n, 3, 10]
    out += two_plane_product(np.asarray(betas, np.float32)[None, None, :], S).sum(-1)
    t = np.asarray(bm["v_template"], np.float32)[vids]
    th, tm = bf16_planes(t)
    r = ((t - th.astype(np.float32)) - tm.astype(np.float32)).astype(np.float32)
    rh, rm = bf16_planes(r)
    return out + th + tm + rh + rm


def exact_forward(bm, xb, betas):
    """float64 oracle: (posed vertices [B,V,3] without transl, v_posed [B,V,3], max_j |t_j| [B])"""
    from oracle.smplx_lbs import BodyModel, smplx_forward
    ob = BodyModel(bm, dtype=torch.float64)
    xb = torch.as_tensor(np.asarray(xb, np.float32)).double().reshape(-1, 93)
    be = torch.as_tensor(np.asarray(betas, np.float32)).double().reshape(-1, 10)
    v, _, mid = smplx_forward(ob, xb, be, return_intermediate=True)
    tn = mid["A"][:, :, :3, 3].norm(dim=-1).max(-1).values
    return (v - xb[:, None, :3]).numpy(), mid["v_posed"].numpy(), tn.numpy()


def cheap_posed_error(bm, xb, betas, vids=None):
    """per-vertex |posed(cheap v_posed) - posed(float64)| (float64 skinning, one body), and F, tn of that body"""
    xb = np.asarray(xb, np.float32).reshape(93)
    betas = np.asarray(betas, np.float32).reshape(10)
    V = bm["v_template"].shape[0]
    vids = np.arange(V) if vids is None else np.asarray(vids)
    F = features_f32(bm, xb)
    _, vp64, tn = exact_forward(bm, xb, betas)
    from oracle.smplx_lbs import BodyModel, smplx_forward
    ob = BodyModel(bm, dtype=torch.float64)
    _, _, mid = smplx_forward(ob, torch.as_tensor(xb).double()[None], torch.as_tensor(betas).double()[None], return_intermediate=True)
    A = mid["A"][0].numpy()                                                     # [55, 4, 4]
    W = np.asarray(bm["lbs_weights"], np.float32).astype(np.float64)[vids]      # [n, 55]
    dv = cheap_vposed(bm, F, betas, vids) - vp64[0, vids]
    err = np.einsum("nj,jac,nc->na", W, A[:, :3, :3], dv)
    return np.linalg.norm(err, axis=1), err, F, float(tn[0])


def kernel_vertex_order(bm, marker_vids, feet_vids):
    """perm[row] of the packing, csrc/lbs_pack.hip (picked vertices first, then by the set of joints a vertex is bound to;
    compared by tests/test_lbs_pack_cpu.py)"""
    V = bm["v_template"].shape[0]
    pick = np.zeros(V, bool)
    pick[np.asarray(marker_vids)] = True
    pick[np.asarray(bm["extra_vids"])] = True
    pick[np.asarray(bm["lmk_vids"]).reshape(-1)] = True
    W = np.asarray(bm["lbs_weights"], np.float32)
    key = [tuple(np.flatnonzero(W[v] != 0).tolist()) for v in range(V)]
    return sorted(range(V), key=lambda v: (not pick[v], key[v]))


def adversarial_body(seed=0, num_verts=2048, n_adv=96, sigma=0.5, axis=2):
    """synth.make_body_model(seed, num_verts) with `n_adv` vertices whose fp16 product errors all point along `axis` for one pose.

    The vertices are bound to the pelvis alone (a skinning-weight set no other vertex has: the kernel's joint-set sort packs them
    into tiles of their own, count-only since none is a marker, vertex joint, landmark corner or foot).  Every one of their
    pose-corrective columns is m_j e_axis with m_j <= C_j (the base model's largest column of that joint) chosen half an fp16
    ulp off the fp16 grid, and signed so that f~ p~ - F P of every fp16 column is positive for the pose returned.  Their templates
    are shifted by minus the blended offset, so the posed vertices stay where the base body had them.
    Returns (bm, adversarial vertex ids, xb [93] fp32 (global orient and translation zero), betas [10] fp32)."""
    bm = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in synth.make_body_model(seed, num_verts=num_verts).items()}
    V = num_verts
    rng = np.random.default_rng(1000 + seed)
    taken = set(synth.marker_ids(V).tolist()) | set(np.asarray(bm["extra_vids"]).tolist()) | \
        set(np.asarray(bm["lmk_vids"]).reshape(-1).tolist()) | set(synth.feet_vids(V).tolist())
    cand = np.array([v for v in range(V) if v not in taken])
    adv = np.sort(rng.choice(cand, size=n_adv, replace=False))
    xb = np.zeros(93, np.float32)
    xb[6:69] = rng.normal(0.0, sigma, 63)
    xb[69:] = rng.normal(0.0, 2.5 * sigma, 24)
    betas = rng.normal(0.0, 1.0, 10).astype(np.float32)
    F = features_f32(bm, xb).reshape(-1)
    Ft, Fd = f16(F), F.astype(np.float64)
    C = model_consts(bm)["C"] / (1.0 + 1e-6)
    # m_j: an fp32 value 0.49 ulp above an fp16 grid point g (rounds down to g), at most C_j
    m = np.zeros(51)
    for j in range(51):
        g = np.float16(C[j])
        while float(g) + 0.5 * float(np.spacing(g)) > C[j]:
            g = np.nextafter(g, np.float16(0))
        m[j] = float(np.float32(float(g) + 0.49 * float(np.spacing(g))))
        assert float(np.float16(np.float32(m[j]))) == float(g)
    m9 = np.repeat(m, 9)
    dm = f16(m9) - m9                                                          # < 0
    colerr = (Ft - Fd) * m9 + Ft * dm                                         # f~ p~ - F P of a column + m_j e_axis
    sgn = np.where(FP16_COL & (colerr < 0), -1.0, 1.0)
    P = np.asarray(bm["posedirs"], np.float32).reshape(54, 9, V, 3)
    for ci, j in enumerate(MOVABLE):
        for e in range(9):
            k = ci * 9 + e
            P[j - 1, e][adv] = 0.0
            P[j - 1, e][adv, axis] = np.float32(sgn[k] * m9[k])
    for j in (22, 23, 24):
        P[j - 1][:, adv] = 0.0
    bm["posedirs"] = np.ascontiguousarray(P.reshape(54 * 9, V * 3))
    W = np.zeros((n_adv, 55), np.float32)
    W[:, 0] = 1.0
    bm["lbs_weights"][adv] = W
    # offsets at this pose (float64 features of the oracle): the template absorbs them
    _, vp64, _ = exact_forward(bm, xb, betas)
    offs = vp64[0, adv] - np.asarray(bm["v_template"], np.float64)[adv]
    bm["v_template"][adv] = (np.asarray(bm["v_template"], np.float64)[adv] - offs).astype(np.float32)
    return bm, adv, xb, betas
