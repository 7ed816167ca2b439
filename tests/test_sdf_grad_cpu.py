"""The differentiable scene SDF without a device: the closed form the kernels implement against the reference's recorded autograd
gradient (tests/golden/calc_sdf_grad_ref.npz), the C ABI of the three new calls, and the penalty term of `fit_markers` against a
hand-written Adam loop (tests/sdf_grad_ref.py)."""
import os
import re

import numpy as np
import pytest
import torch

from tests import sdf_grad_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("egx_sdf_value_grad", "egx_sdf_penalty_forward", "egx_sdf_penalty_backward")


@pytest.mark.parametrize("tag", [t for t, _ in ref.GOLDEN_CASES])
def test_closed_form_matches_the_reference_autograd_in_float64(tag):
    c = ref.golden_case(tag)
    grid, pts, cot = ref.golden_inputs(tag, c.grid.shape)              # the fixture holds the inputs the generator draws
    assert np.array_equal(grid, c.grid) and np.array_equal(pts, c.pts) and np.array_equal(cot, c.cot)
    val, grad = ref.closed_form(c.pts, c.grid, c.center, c.scale)
    grad = grad * c.cot[:, None].astype(np.float64)
    ev, eg = np.abs(val - c.val64).max(), np.abs(grad - c.grad64).max()
    print(f"{c.name}: closed form - reference (float64): values {ev:.2e}, gradient {eg:.2e}")
    assert ev <= 1e-12 and eg <= 1e-12
    held = c.clamped()
    assert held[c.n_interior:].any() and not held[:c.n_interior].any()
    assert (grad[held] == 0).all() and (c.grad64[held] == 0).all() and (c.grad32[held] == 0).all()


@pytest.mark.parametrize("tag", [t for t, _ in ref.GOLDEN_CASES])
def test_float32_closed_form_stays_within_the_yardstick(tag):
    """The differences-first evaluation in float32 - what the kernel computes - against the bound the device is held to."""
    c = ref.golden_case(tag)
    val, grad = ref.closed_form(c.pts, c.grid, c.center, c.scale, np.float32)
    assert np.abs(val - c.val32).max() <= 4 * np.finfo(np.float32).eps * np.abs(c.val64).max()   # aten's vectorised CPU kernel sums in another order
    err = c.error(grad.astype(np.float64) * c.cot[:, None].astype(np.float64))
    print("\n".join(c.table(err)).replace("hip", "np32").replace(" (MI355X)", ""))
    assert (err <= ref.R * c.err32).all()


@pytest.mark.parametrize("dims", [(16, 16, 16), (7, 5, 2)])
def test_closed_form_matches_the_oracle_autograd(dims):
    c = ref.oracle_case(dims)
    val, grad = ref.closed_form(c.pts, c.grid, c.center, c.scale)
    assert np.abs(val - c.val64).max() <= 1e-12
    assert np.abs(grad * c.cot[:, None].astype(np.float64) - c.grad64).max() <= 1e-12


def test_closed_form_on_faces_takes_the_upper_cell():
    d, k = ref.FACE_D, ref.FACE_D * 0.5 * ref.FACE_SCALE
    grid = ref.random_field((d, d, d), 5)
    vox = np.array([[3, 2, 5], [0, 6, 1], [d - 1, 2, 3], [4, d - 1, d - 1]])
    pts = (((2 * vox + 1) / d - 1) / ref.FACE_SCALE).astype(np.float32)
    val, grad = ref.closed_form(pts, grid, ref.FACE_CENTER, ref.FACE_SCALE)
    g = grid.astype(np.float64)
    for (x, y, z), v, gr in zip(vox, val, grad):
        assert v == -g[x, y, z]
        expect = [-(g[x + 1, y, z] - g[x, y, z]) * k if 0 < x < d - 1 else 0.0, -(g[x, y + 1, z] - g[x, y, z]) * k if 0 < y < d - 1 else 0.0,
                  -(g[x, y, z + 1] - g[x, y, z]) * k if 0 < z < d - 1 else 0.0]
        assert np.array_equal(gr, np.asarray(expect))
    assert len(ref.face_points()) == 96


def test_header_binding_and_library_carry_the_new_calls():
    from egogen_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "egogen_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(egx_[a-z0-9_]+)\s*\(", txt))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["egx_sdf_value_grad"][1]) == 7
    assert len(_lib.SIGNATURES["egx_sdf_penalty_forward"][1]) == len(_lib.SIGNATURES["egx_sdf_penalty_backward"][1]) == 13
    csrc = os.path.join(ROOT, "egogen_amd", "csrc")
    sources = [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hip", ".h"))] + [os.path.join(ROOT, "include", "egogen_hip.h")]
    if not os.path.exists(_lib.LIB_PATH) or os.path.getmtime(_lib.LIB_PATH) < max(os.path.getmtime(f) for f in sources):
        import __graft_entry__ as g                                    # a library older than its sources says nothing about them
        g.build()
    _lib._lib = None
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert getattr(lib, name) is not None


def test_calc_sdf_return_gradient_is_no_longer_unimplemented():
    """Off the device the call fails for the device's absence, not for a missing feature."""
    from egogen_amd import _lib, utils
    assert "analytic, unnormalised derivative" in utils.calc_sdf.__doc__
    with pytest.raises(_lib.EgxError):                                 # a CPU tensor, with or without a device in the machine
        utils.calc_sdf(torch.zeros(1, 2, 3), ref.oracle_case((16, 16, 16)).sdf_dict(), return_gradient=True)


def test_collision_vids_are_an_even_subsample_without_feet():
    from egogen_amd import synth
    from egogen_amd.scene_sdf import collision_vids
    bm, feet = ref.bref.body(), synth.feet_vids(640)
    v = collision_vids(bm, feet, 200)
    assert v.dtype == np.int32 and v.shape == (200,) and np.all(np.diff(v) > 0) and not set(v.tolist()) & set(int(f) for f in feet)
    assert np.array_equal(v, collision_vids(bm, feet, 200))
    rest = np.setdiff1d(np.arange(640), feet)
    steps = np.diff(np.searchsorted(rest, v))                          # evenly strided among the candidates
    assert v[0] == rest[0] and set(steps.tolist()) <= {rest.size // 200, rest.size // 200 + 1}
    assert np.array_equal(collision_vids(bm, feet, 1024), rest)        # fewer candidates than n: all of them


STEPS = 25


def test_fit_markers_with_a_penalty_reproduces_the_hand_written_adam_loop():
    from egogen_amd.fit import fit_markers
    model, collide, penalty, target, betas, xb0 = ref.cpu_fit_parts(torch.float64)
    xb, hist, pene = fit_markers(model, target, betas, xb0, steps=STEPS, lr=ref.FIT_LR, collision_model=collide, penalty=penalty,
                                 weight_pene=ref.FIT_WEIGHT)
    xb_ref, hist_ref, pene_ref = ref.adam_loop(model, collide, penalty, target, betas, xb0, STEPS, ref.FIT_LR, ref.FIT_WEIGHT)
    assert hist.shape == (STEPS + 1,) and pene.shape == (8,) and not pene.requires_grad
    # float64 throughout; torch's Adam and the loop round their moment updates differently (1e-16 per step), nothing more
    assert np.abs(hist - hist_ref).max() <= 1e-9 * hist_ref.max()
    assert (xb - xb_ref).abs().max() <= 1e-9 and (pene - pene_ref).abs().max() <= 1e-9 * max(1.0, float(pene_ref.max()))
    # the term acts: without it the same start ends with more penetration
    _, hist0, pene0 = fit_markers(model, target, betas, xb0, steps=STEPS, lr=ref.FIT_LR, collision_model=collide, penalty=penalty)
    assert pene0.mean() > 0 and pene.mean() < pene0.mean() and hist0[-1] != hist[-1]


def test_fit_markers_defaults_leave_the_history_bit_identical():
    from egogen_amd.fit import fit_markers
    model, collide, penalty, target, betas, xb0 = ref.cpu_fit_parts(torch.float32)
    xb_a, hist_a = fit_markers(model, target, betas, xb0, steps=STEPS, lr=ref.FIT_LR)
    xb_b, hist_b = fit_markers(model, target, betas, xb0, steps=STEPS, lr=ref.FIT_LR, collision_model=None, penalty=None, weight_pene=0.0)
    assert np.array_equal(hist_a, hist_b) and torch.equal(xb_a, xb_b)
    # a penalty that is only reported (weight 0) does not touch the optimisation either
    xb_c, hist_c, pene = fit_markers(model, target, betas, xb0, steps=STEPS, lr=ref.FIT_LR, collision_model=collide, penalty=penalty)
    assert np.array_equal(hist_a, hist_c) and torch.equal(xb_a, xb_c) and pene.shape == (8,)
    with pytest.raises(ValueError):
        fit_markers(model, target, betas, xb0, steps=STEPS, weight_pene=1.0)
