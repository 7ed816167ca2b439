"""The fix-up band of LBS blend mode 3 ("f16mix") against a float64 emulation of its cheap evaluation (tests/lbs_mode3.py): the
band is a hard bound, and the adversarial body the GPU test uses does defeat a statistical one."""
import os
import re

import numpy as np
import pytest

from egogen_amd import synth
from tests import lbs_mode3 as L

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "egogen_amd", "csrc")


def test_band_constants_mirror_the_kernel():
    src = open(os.path.join(CSRC, "lbs.h")).read()     # the band constants
    for name in ("LBS_FIX_SLACK_M", "LBS_TWO_PLANE_ERR", "LBS_ACC_ADDS_OFFSETS", "LBS_ACC_ADDS_LAST", "LBS_FIX_MARGIN", "LBS_SKIN_ERR"):
        m = re.search(r"constexpr float %s = ([0-9.eE+-]+)f;" % name, src)
        assert m, name
        assert float(m.group(1)) == getattr(L, name), name
    # the columns of the fp16 k-steps: k-steps 1..28 of 16 columns (M4_BASE_PIECES / egx_m4_feat_piece)
    assert "k0 + e >= 16 && k0 + e < 464" in open(os.path.join(CSRC, "lbs_pose.hip")).read()
    assert int(L.FP16_COL.sum()) == 28 * 16


@pytest.fixture(scope="module")
def adversarial():
    bm, adv, xb, betas = L.adversarial_body()
    err_n, err, F, tn = L.cheap_posed_error(bm, xb, betas, adv)
    return bm, adv, xb, betas, err_n, err, F, tn


def test_adversarial_vertices_fill_count_only_tiles(adversarial):
    """The kernel sorts vertices by joint set (picked ones first): the pelvis-only adversarial vertices fill whole 32-row tiles that
    hold no picked vertex and no foot - count-only tiles of a single joint, which mode 3 evaluates with the fp16 product."""
    bm, adv, *_ = adversarial
    V = bm["v_template"].shape[0]
    perm = np.asarray(L.kernel_vertex_order(bm, synth.marker_ids(V), synth.feet_vids(V)))
    is_adv = np.isin(perm, adv)
    full = [t for t in range((V + 31) // 32) if is_adv[32 * t: 32 * t + 32].all() and len(is_adv[32 * t: 32 * t + 32]) == 32]
    assert len(full) >= 2, full
    picks = set(synth.marker_ids(V).tolist()) | set(np.asarray(bm["extra_vids"]).tolist()) | set(np.asarray(bm["lmk_vids"]).ravel().tolist())
    assert not (set(adv.tolist()) & (picks | set(synth.feet_vids(V).tolist())))


def test_adversarial_body_defeats_the_statistical_band(adversarial):
    """All product errors of the adversarial vertices align: the cheap position is off by more than twice the statistical band
    (2 x 2^-11 sqrt(sum_j |R_j - I|_F^2 C_j^2) + the skinning allowance the kernel had), along the chosen axis."""
    bm, adv, xb, betas, err_n, err, F, tn = adversarial
    stat = L.statistical_band(bm, F, tn)
    print(f"\nadversarial cheap error {err_n.min():.3e} .. {err_n.max():.3e} m, statistical band {stat:.3e} m")
    assert err_n.min() > 2.0 * stat, (err_n.min(), stat)
    assert (err[:, 2] > 0.99 * err_n).all()


def _posed_bound(bm, F, betas, tn):
    """what the band must cover of the blend with float64 skinning: fix_e without the matrix-pipe skinning allowance"""
    return L.band(L.model_consts(bm), F, betas, tn, skin=False)[0]


def test_hard_band_covers_the_adversarial_body(adversarial):
    bm, adv, xb, betas, err_n, err, F, tn = adversarial
    bound = _posed_bound(bm, F, betas, tn)
    _, terms = L.band(L.model_consts(bm), F, betas, tn)
    print(f"\nadversarial cheap error {err_n.max():.3e} m, hard band {bound:.3e} m ({terms})")
    assert err_n.max() <= bound
    # the L1 form alone (what the CS form cannot beat for this body) is within a factor of two of the error: the body is adversarial
    assert terms["l1"] < 2.0 * err_n.max()


@pytest.mark.parametrize("kind", ["ordinary", "wild"])
def test_hard_band_covers_random_poses_on_the_default_body(kind):
    """Random ordinary (0.2 rad body, 0.5 hand PCA) and wild (x5) poses on the synthetic body: every vertex's cheap error is inside
    the band; the band is wider than the statistical one by a bounded factor (what the fix-up costs)."""
    V = 2048
    bm = synth.make_body_model(0, num_verts=V)
    c = L.model_consts(bm)
    P16 = L.f16(L._pose_block(bm)[L.FP16_COL])
    rng = np.random.default_rng(7 if kind == "ordinary" else 8)
    scale = 1.0 if kind == "ordinary" else 5.0
    worst = 0.0
    for _ in range(6):
        xb = np.zeros(93, np.float32)
        xb[0:2] = rng.uniform(-2, 2, 2)
        xb[3:6] = rng.normal(0, 0.8, 3)
        xb[6:69] = rng.normal(0, 0.2 * scale, 63)
        xb[69:] = rng.normal(0, 0.5 * scale, 24)
        betas = rng.normal(0, 1, 10).astype(np.float32)
        F = L.features_f32(bm, xb)
        _, vp64, tn = L.exact_forward(bm, xb, betas)
        dv = L.cheap_vposed(bm, F, betas, np.arange(V), P16=P16) - vp64[0]
        err = np.linalg.norm(dv, axis=1) * c["w_abs_max"]       # |sum_j W R_j dv| <= sum_j |W| |dv|
        bound = _posed_bound(bm, F, betas, float(tn[0]))
        assert err.max() <= bound, (err.max(), bound)
        worst = max(worst, err.max() / bound)
        assert L.band(c, F, betas, float(tn[0]))[0] < 8.0 * L.statistical_band(bm, F, float(tn[0]))
    print(f"\n{kind}: worst cheap error / hard band {worst:.3f}")
