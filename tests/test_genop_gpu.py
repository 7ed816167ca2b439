"""GPU checks of the generation operator (egogen_amd/genop.py) and its kernel egx_primitive_advance (csrc/genop.hip).

Yardstick of tests 1 and 4 (the one of tests/test_combo_train_gpu.py::held): a result is held to the float64 restatement
(tests/genop_ref.py) within R = 3 times the distance of the float32 restatement from float64, largest entry of a group, the
figures printed before they are asserted.  Groups of test 1, chosen before any run: `marker_b` (4 020 B metres-scale values),
`frame` (the updated R0 | T0, 12 B values of order one), `seed_params` (new transl | new global orientation AS A MATRIX, 24 B
values: axis-angle is discontinuous at pi, where the special bodies sit on purpose), `seed_markers` (402 B values).  Tests 2 and
3 use the bars of the tests they name."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import genop_ref
from tests.genop_gpu_helpers import (CFG_RF, R, ROOT, V_SMALL, _aa2R64, _combo, _inputs, _launch, _op, _walkers, emit, held, patched_loop,
                                     small_world)  # noqa: F401
from tests.helpers import load_golden, max_abs, rebuild_state_dict, seeded_prior_state_dict

pytestmark = pytest.mark.gpu


def _seed_group(r):
    """new transl | new global orientation as a matrix, [B,2,12]"""
    sp = torch.as_tensor(r["seed_params"]).detach().cpu().double()
    B = sp.shape[0]
    return torch.cat([sp[:, :, :3], _aa2R64(sp[:, :, 3:6]).reshape(B, 2, 9)], dim=-1)


@pytest.mark.parametrize("rf", [0.0, 1.0, CFG_RF])
@pytest.mark.parametrize("jpb", [127, 55])
@pytest.mark.parametrize("B", [1, 3, 65])
def test_primitive_advance_kernel(small_world, B, jpb, rf):
    d = _inputs(small_world, B)
    nonfinite = torch.zeros(1, dtype=torch.int32, device="cuda")
    o = _launch(d, list(range(B)), jpb, rf, nonfinite)
    i = o["_in"]
    ref = {dt: genop_ref.advance(i["pp"], i["Y_gen"], i["X"], i["J"], i["mp"], i["dT"], rf, i["R0"], i["T0"], dt)
           for dt in (torch.float64, torch.float32)}
    r64, r32 = ref[torch.float64], ref[torch.float32]
    if B >= 3:      # the special bodies are what their docstring says
        assert float(r64["R_"][0, 0, 0]) * float(r64["R_"][1, 0, 0]) < 0, "hip axes of bodies 0 and 1 point the same way along x"
        from oracle.rot import tgm_angle_axis_to_rotation_matrix as aa2R, tgm_rotation_matrix_to_quaternion as R2q
        go = torch.einsum("bij,bjk->bik", r64["R_"][2:3].repeat(2, 1, 1).permute(0, 2, 1), aa2R(i["pp"][2, 18:20, 3:6].cpu().double()))
        w = R2q(go)[:, 0]
        assert float(w.min()) < 0 < float(w.max()), w
        assert float(r64["seed_params"][2, :, 3:6].norm(dim=-1).min()) > 3.0
    name = f"advance B={B} jpb={jpb} rf={rf:g}"
    held(name, "marker_b", o["marker_b"], r64["marker_b"], r32["marker_b"])
    held(name, "frame", torch.cat([o["R0"].reshape(B, 9), o["T0"]], 1), torch.cat([r64["R0"].reshape(B, 9), r64["T0"]], 1),
         torch.cat([r32["R0"].reshape(B, 9), r32["T0"]], 1))
    held(name, "seed_params", _seed_group(o), _seed_group(r64), _seed_group(r32))
    held(name, "seed_markers", o["seed_markers"], r64["seed_markers"], r32["seed_markers"])
    # pure copies are exact
    assert torch.equal(o["R"], i["R0"]) and torch.equal(o["T"], i["T0"])
    assert torch.equal(o["pelvis"], i["J"][:, :, 0])
    assert torch.equal(o["seed_params"][:, :, 6:], i["pp"][:, 18:20, 6:])
    assert int(nonfinite.item()) == 0


@pytest.mark.parametrize("jpb", [127, 55])
def test_primitive_advance_row_does_not_depend_on_batch(small_world, jpb):
    d = _inputs(small_world, 65)
    full = _launch(d, list(range(65)), jpb, CFG_RF)
    for b in (0, 1, 2, 33, 64):
        one = _launch(d, [b], jpb, CFG_RF)
        for k in ("marker_b", "pelvis", "R", "T", "R0", "T0", "seed_params", "seed_markers"):
            assert torch.equal(one[k][0], full[k][b]), (b, k)


def test_primitive_advance_counts_nonfinite_sequences(small_world):
    d = _inputs(small_world, 3)
    Yg = d["Y_gen"].clone()
    Yg[0, 0, 5] = float("nan")
    Yg[3, 2, 7] = float("nan")
    nonfinite = torch.zeros(1, dtype=torch.int32, device="cuda")
    _launch(d, [0, 1, 2], 127, CFG_RF, nonfinite, Y_gen=Yg)
    assert int(nonfinite.item()) == 2
    _launch(d, [0, 1, 2], 127, CFG_RF, nonfinite)       # a counter, not a flag: a clean launch leaves it
    assert int(nonfinite.item()) == 2


def test_primitive_advance_rejects_bad_arguments(small_world):
    """Rejected before anything is launched: every pointer may therefore be the same scratch buffer."""
    import ctypes as C
    from egogen_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(16384, device="cuda")
    p, off = C.c_void_p(buf.data_ptr()), C.c_void_p(buf.data_ptr() + 4)      # `off`: 4 bytes past a 16-byte boundary

    def call(mproj=p, jpb=127, x_ld=201, B=1, out_marker=p):
        return lib.egx_primitive_advance(p, p, p, p, x_ld, p, jpb, mproj, p, 0.5, B, p, p, out_marker, p, p, p, p, p, p, 201, None,
                                         _lib.current_stream_ptr())
    for kw in ({"mproj": off}, {"out_marker": off}, {"jpb": 2}, {"x_ld": 200}, {"B": 0}, {"mproj": None}):
        assert call(**kw) != 0, kw
        with pytest.raises(_lib.EgxError):
            _lib.check(call(**kw), "egx_primitive_advance")


# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gen_world():
    g = load_golden("genop_ref.npz")
    sd = rebuild_state_dict(g, [int(g["pred_seed"]), int(g["reg_seed"])], ["predictor.", "regressor."],
                            gains=[float(g["pred_gain"]), float(g["reg_gain"])])
    return g, _op(_combo(sd))


def _held_like_sample_prior(Y, Yb, Yo, Ybo, what):
    """the bars of tests/test_nets_gpu.py::test_sample_prior_matches_oracle"""
    Yo, Ybo = np.asarray(Yo), np.asarray(Ybo)
    assert Y.shape == Yo.shape and Yb.shape == Ybo.shape, what
    assert max_abs(Y, Yo) < 1e-4 * max(1.0, float(np.abs(Yo).max())), what
    assert max_abs(Yb[..., :3], Ybo[..., :3]) < 2e-4 * max(1.0, float(np.abs(Ybo[..., :3]).max())), what
    assert max_abs(_aa2R64(Yb[..., 3:69]), _aa2R64(Ybo[..., 3:69])) < 2e-4, what
    assert max_abs(Yb[..., 69:], Ybo[..., 69:]) < 2e-4 * max(1.0, float(np.abs(Ybo[..., 69:]).max())), what


@pytest.mark.parametrize("tag,n_gens", [("gen3", -1), ("gen4", 4)])
def test_generate_matches_reference_execution(gen_world, tag, n_gens):
    g, op = gen_world
    args = (g[tag + "_data"], g[tag + "_bparams"], g[tag + "_betas"])
    Y, Yb = op.generate(*args, n_gens=n_gens, t_his=2, z=g[tag + "_z"])
    assert isinstance(Y, np.ndarray) and isinstance(Yb, np.ndarray)
    _held_like_sample_prior(Y, Yb, g[tag + "_Y"], g[tag + "_Yb"], tag)
    _, Yb_nb = op.generate(*args, n_gens=n_gens, t_his=2, z=g[tag + "_z"], param_blending=False)
    _held_like_sample_prior(Y, Yb_nb, g[tag + "_Y"], g[tag + "_Yb_noblend"], tag + " without blending")
    # _blend_params rows are exact given Yb
    want = Yb_nb.copy()
    want[:, 2, 6:] = (want[:, 1, 6:] + want[:, 3, 6:]) / 2.0
    want[:, 3, 6:] = (want[:, 2, 6:] + want[:, 4, 6:]) / 2.0
    assert np.array_equal(Yb, want)
    # torch inputs on the device, t_his = None (the model's), torch outputs, z returned
    Yt, Ybt, zt = op.generate(*[torch.as_tensor(a).cuda() for a in args], n_gens=n_gens, to_numpy=False, return_z=True,
                              z=torch.as_tensor(g[tag + "_z"]))
    assert Yt.is_cuda and np.array_equal(Yt.cpu().numpy(), Y) and np.array_equal(Ybt.cpu().numpy(), Yb)
    assert np.array_equal(zt.cpu().numpy(), g[tag + "_z"])
    if n_gens == 4:
        assert np.array_equal(g[tag + "_z"][0], g[tag + "_z"][2])
        assert np.array_equal(Y[0], Y[2]) and np.array_equal(Yb[0], Yb[2]) and not np.array_equal(Y[0], Y[1])


def test_generate_argument_handling(gen_world):
    g, op = gen_world
    args = (g["gen3_data"], g["gen3_bparams"])
    with pytest.raises(ValueError, match="t_his"):
        op.generate(*args, g["gen3_betas"], t_his=1, z=g["gen3_z"])
    Y1, Yb1 = op.generate(*args, g["gen3_betas"].reshape(10), z=g["gen3_z"])
    Y2, Yb2 = op.generate(*args, np.repeat(g["gen3_betas"].reshape(1, 10), 3, 0), z=g["gen3_z"])
    assert np.array_equal(Y1, Y2) and np.array_equal(Yb1, Yb2)
    _, _, z = op.generate(*args, g["gen3_betas"], return_z=True)       # drawn here
    assert z.shape == (3, 128) and np.isfinite(z).all()
    bp = torch.as_tensor(g["blend_in"]).cuda()
    assert op._blend_params(bp) is bp and np.array_equal(bp.cpu().numpy(), g["blend_out"])
    with pytest.raises(NotImplementedError):
        op.generate_ppo()


# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,n", [("free", 3), ("pene", 2)])
def test_generate_sequence_matches_reference_env_execution(case, n):
    """The chain from the reset state of env_step_ref.npz with the recorded z, on the fixture's body model and prior weights,
    against what the reference's own CrowdEnv.step recorded; bars and floors of tests/test_env_reference_goldens.py."""
    import json
    from egogen_amd import synth
    from egogen_amd.body_model import BodyModelHandle
    from tests.test_env_reference_goldens import _aa_close, _close
    g = load_golden("env_step_ref.npz")
    pre = case + "_"
    assert int(g[pre + "n_steps"]) == n
    sd = seeded_prior_state_dict(int(g["prior_seed"]), *[float(v) for v in g["prior_gains"]])
    h = BodyModelHandle(synth.make_body_model(0), synth.marker_ids(), synth.feet_vids())
    rf = float(json.loads(str(g["cfg_json"]))["modelconfig"]["reproj_factor"])
    op = _op(_combo(sd), h)
    data = g[pre + "reset_state"][:, None, :201]
    res = op.generate_sequence(data, g[pre + "reset_seed"][:, None], g[pre + "betas"], n, z=g[pre + "z"][:n].reshape(n, 1, 128),
                               reproj_factor=rf, R0=g[pre + "reset_R0"], T0=g[pre + "reset_T0"], to_numpy=False)
    # what each primitive handed on: re-derive the seed of primitive k + 1 from the records (its frames 0, 1) and the final state
    for i in range(n):
        sp = f"{pre}s{i}_"
        pp = res.params[i, 0]
        _close(pp[:, :3], g[sp + "pred_params"][:, :3], "m", sp + "pred transl")
        _aa_close(pp[:, 3:6], g[sp + "pred_params"][:, 3:6], sp + "pred glorot")
        _close(pp[:, 6:], g[sp + "pred_params"][:, 6:], "unit", sp + "pred pose")
        _close(res.markers[i, 0], g[sp + "marker_b"], "m", sp + "marker_b")
        _close(res.pelvis[i, 0], g[sp + "joints"][:, 0], "m", sp + "pelvis")
        prev = g[pre + "reset_R0"] if i == 0 else g[f"{pre}s{i - 1}_after_R0"]
        _close(res.rotmat[i, 0], prev, "unit", sp + "frame of the primitive")
        if i + 1 < n:       # the seed handed on is frames 0, 1 of the next record; the frame is the next record's
            nxt = res.params[i + 1, 0, :2]
            _close(nxt[:, :3], g[sp + "after_seed"][:, :3], "m", sp + "seed transl")
            _aa_close(nxt[:, 3:6], g[sp + "after_seed"][:, 3:6], sp + "seed glorot")
            _close(nxt[:, 6:], g[sp + "after_seed"][:, 6:], "unit", sp + "seed pose")
            _close(res.rotmat[i + 1, 0], g[sp + "after_R0"], "unit", sp + "R0")
            _close(res.transl[i + 1, 0], g[sp + "after_T0"].reshape(-1), "m", sp + "T0")
    last = f"{pre}s{n - 1}_"
    _close(res.R0[0], g[last + "after_R0"], "unit", last + "R0")
    _close(res.T0[0], g[last + "after_T0"].reshape(-1), "m", last + "T0")


def test_generate_sequence_marker_seed_matches_reference_env_execution():
    """The marker seed each primitive hands on (first 201 columns of the env's next state), read from the kernel's own output:
    one primitive at a time, so that the seed buffers can be looked at."""
    import json
    from egogen_amd import synth
    from egogen_amd.body_model import BodyModelHandle
    from tests.test_env_reference_goldens import _aa_close, _close
    g = load_golden("env_step_ref.npz")
    sd = seeded_prior_state_dict(int(g["prior_seed"]), *[float(v) for v in g["prior_gains"]])
    h = BodyModelHandle(synth.make_body_model(0), synth.marker_ids(), synth.feet_vids())
    rf = float(json.loads(str(g["cfg_json"]))["modelconfig"]["reproj_factor"])
    op = _op(_combo(sd), h)
    for case, n in (("free", 3), ("pene", 2)):
        pre = case + "_"
        X = torch.as_tensor(g[pre + "reset_state"][:, None, :201]).cuda()
        seed = torch.as_tensor(g[pre + "reset_seed"][:, None]).cuda()
        R0, T0 = torch.as_tensor(g[pre + "reset_R0"]).cuda(), torch.as_tensor(g[pre + "reset_T0"]).cuda()
        for i in range(n):
            sp = f"{pre}s{i}_"
            with patched_loop(op, "_advance_loop") as seen:
                res = op.generate_sequence(X, seed, g[pre + "betas"], 1, z=g[pre + "z"][i].reshape(1, 1, 128), reproj_factor=rf, R0=R0,
                                           T0=T0, to_numpy=False)
            kept = {"X": seen.s["xs"][1], "seed": seen.s["seed"]}       # what the one primitive handed on: the loop's own buffers
            _close(kept["X"][:, 0], g[sp + "after_state"][:, :201], "unit", sp + "marker seed")
            _close(kept["seed"][0, :, :3], g[sp + "after_seed"][:, :3], "m", sp + "seed transl")
            _aa_close(kept["seed"][0, :, 3:6], g[sp + "after_seed"][:, 3:6], sp + "seed glorot")
            X, seed, R0, T0 = kept["X"], kept["seed"].permute(1, 0, 2), res.R0, res.T0


# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chain_world(small_world):
    """K = 3, b = 2 on synthetic assets: the operator, its inputs, and the float32 / float64 restatements of the same chain."""
    from oracle.smplx_lbs import BodyModel
    h = small_world["handle"]
    sd = seeded_prior_state_dict()
    op = _op(_combo(sd), h)
    pp, betas, g = _walkers(2, 77)
    o = h.forward(pp.cuda().reshape(40, 93), betas.cuda(), 20, want_verts=False)
    data = o["markers"].reshape(2, 20, 201)[:, :2].permute(1, 0, 2).contiguous().cpu()
    bparams = pp[:, :2].permute(1, 0, 2).contiguous()
    z = torch.randn(3, 2, 128, generator=g)
    refs = {dt: genop_ref.chain(sd, BodyModel(small_world["bm"], dtype=dt), small_world["mk"], data.permute(1, 0, 2), pp[:, :2],
                                torch.eye(3).repeat(2, 1, 1), torch.zeros(2, 3), betas, z, CFG_RF) for dt in (torch.float64, torch.float32)}
    return {"op": op, "data": data, "bparams": bparams, "betas": betas, "z": z, "refs": refs, "handle": h}


def _seams(joints_w):
    """joints_w[K,b,20,J,3] in the world frame -> per seam the largest distance between frames 18, 19 of primitive k and frames
    0, 1 of primitive k + 1"""
    return [float((joints_w[k, :, 18:20] - joints_w[k + 1, :, 0:2]).abs().max()) for k in range(joints_w.shape[0] - 1)]


def test_sequence_round_trip_and_seams(chain_world, tmp_path):
    from egogen_amd.utils import rollout_primitives
    w = chain_world
    op, h = w["op"], w["handle"]
    K, b = 3, 2
    res = op.generate_sequence(w["data"], w["bparams"], w["betas"], K, z=w["z"], reproj_factor=CFG_RF, to_numpy=True)
    assert res.markers.shape == (K, b, 20, 67, 3) and res.params.shape == (K, b, 20, 93) and res.rotmat.shape == (K, b, 3, 3)
    assert res.transl.shape == (K, b, 3) and res.pelvis.shape == (K, b, 20, 3)
    assert np.array_equal(res.rotmat[0], np.tile(np.eye(3, dtype=np.float32), (b, 1, 1))) and not res.transl[0].any()
    for i in range(b):
        path = res.save(str(tmp_path), i, man_id=f"seq{i}")
        assert os.path.basename(path) == f"motion_seq{i}.pkl"
        with open(path, "rb") as fh:
            node = pickle.load(fh)
        assert set(node.keys()) == {"motion", "wpath", "navmesh_path"} and len(node["motion"]) == K
        for mp in node["motion"]:
            assert list(mp.keys()) == ["blended_marker", "smplx_params", "betas", "gender", "transf_rotmat", "transf_transl", "pelvis_loc",
                                       "mp_type"]
            assert mp["blended_marker"].shape == (20, 67, 3) and mp["smplx_params"].shape == (1, 20, 93) and mp["mp_type"] == "2-frame"
            assert mp["transf_rotmat"].shape == (3, 3) and mp["transf_transl"].shape == (1, 3) and mp["pelvis_loc"].shape == (20, 3)
        assert node["wpath"].shape == (2, 3)
        assert np.allclose(node["wpath"][0], res.pelvis[0, i, 0], atol=1e-6)       # identity start frame
        seq = rollout_primitives(node["motion"], h)
        assert seq.shape == (2 + 18 * K, 93) and np.isfinite(seq).all()
    # seams: world-frame joints through BodyModelHandle.forward and the recorded frames
    pp = torch.as_tensor(res.params).cuda()
    J = h.forward(pp.reshape(K * b * 20, 93), torch.as_tensor(res.betas).cuda().repeat(K, 1), 20, want_verts=False)["joints"]
    J = J.reshape(K, b, 20, -1, 3).cpu().double()
    Jw = torch.einsum("kbij,kbtpj->kbtpi", torch.as_tensor(res.rotmat).double(), J) + torch.as_tensor(res.transl).double()[:, :, None, None]
    got = _seams(Jw)
    yard = {}
    for dt, steps in w["refs"].items():
        Jr = torch.stack([s["joints"] for s in steps]).double()
        Rr, Tr = torch.stack([s["R"] for s in steps]).double(), torch.stack([s["T"] for s in steps]).double()
        yard[dt] = _seams(torch.einsum("kbij,kbtpj->kbtpi", Rr, Jr) + Tr[:, :, None, None])
    # The seam is not closed in exact arithmetic either: torchgeometry's angle_axis_to_rotation_matrix divides by (theta + 1e-6),
    # so the float64 chain shows ~3e-7 m itself.  What rounding adds is therefore measured from the float64 chain's figure, for
    # the float32 chain and for the device alike: |seam - seam64| of the device within R times that of the float32 chain.
    for k in range(K - 1):
        s64, s32 = yard[torch.float64][k], yard[torch.float32][k]
        e32, err = abs(s32 - s64), abs(got[k] - s64)
        emit(f"| seam {k}->{k + 1} | world joints: float64 {s64:.3e}, float32 {s32:.3e}, device {got[k]:.3e} | {e32:.3e} | {err:.3e} | "
             f"{err / e32 if e32 > 0 else float(err > 0):.2f} |")
    for k in range(K - 1):
        s64 = yard[torch.float64][k]
        assert abs(got[k] - s64) <= R * abs(yard[torch.float32][k] - s64), (k, got[k], yard[torch.float32][k], s64)


def test_generate_sequence_loop_has_no_host_wait(chain_world):
    """torch-level synchronisation only; the library side is by construction (egx_primitive_advance synchronises no stream)."""
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.skip("this torch build has no torch.cuda.set_sync_debug_mode")
    w = chain_world
    op = w["op"]
    op.generate_sequence(w["data"], w["bparams"], w["betas"], 1, z=w["z"][:1])      # weight images, workspaces
    with patched_loop(op, "_advance_loop", no_host_wait=True) as seen:
        res = op.generate_sequence(w["data"], w["bparams"], w["betas"], 3, z=w["z"])
    ran = [call[0] for call in seen.calls]
    assert ran == [3] and np.isfinite(res.markers).all()
    # ... and the mode does catch a wait in that place
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            torch.ones(1, device="cuda").item()
    finally:
        torch.cuda.set_sync_debug_mode("default")


def test_generate_sequence_argument_handling(chain_world):
    from egogen_amd import _lib
    w = chain_world
    op = w["op"]
    with pytest.raises(ValueError, match="z must be"):
        op.generate_sequence(w["data"], w["bparams"], w["betas"], 2, z=w["z"])
    res = op.generate_sequence(w["data"][:, :1], w["bparams"][:, :1], w["betas"][:1], 2, n_gens=3)     # z drawn, variants of one seed
    assert res.markers.shape == (2, 3, 20, 67, 3) and res.z.shape == (2, 3, 128)
    assert np.array_equal(res.markers[0, 0, :2], res.markers[0, 1, :2]) and not np.array_equal(res.markers[0, 0, 2:], res.markers[0, 1, 2:])
    bm, op.body_model = op.body_model, None
    try:
        with pytest.raises(_lib.EgxError, match="body model"):
            op.generate_sequence(w["data"], w["bparams"], w["betas"], 1)
    finally:
        op.body_model = bm


def test_build_model_loads_both_checkpoint_layouts(tmp_path):
    """:1116-1148: predictor epoch-400 (else 200) + regressor epoch-100, or the combo checkpoint epoch-120 (else 10)."""
    from egogen_amd.genop import GAMMAPrimitiveComboGenOP
    from egogen_amd.models import GAMMAPrimitiveCombo, PREDICTOR_CFG, REGRESSOR_CFG
    sd = seeded_prior_state_dict()
    pd, rd, cd = tmp_path / "p", tmp_path / "r", tmp_path / "c"
    for d in (pd, rd, cd):
        d.mkdir()
    torch.save({"model_state_dict": {k[len("predictor."):]: v for k, v in sd.items() if k.startswith("predictor.")}}, pd / "epoch-200.ckp")
    torch.save({"model_state_dict": {k[len("regressor."):]: v for k, v in sd.items() if k.startswith("regressor.")}}, rd / "epoch-100.ckp")
    torch.save({"epoch": 10, "model_state_dict": sd}, cd / "epoch-10.ckp")
    op = GAMMAPrimitiveComboGenOP({"modelconfig": PREDICTOR_CFG, "trainconfig": {"save_dir": str(pd)}},
                                  {"modelconfig": REGRESSOR_CFG, "trainconfig": {"save_dir": str(rd)}}, {"ckpt_dir": str(cd)})
    for pretrained in (True, False):
        op.build_model(load_pretrained_model=pretrained)
        assert isinstance(op.model, GAMMAPrimitiveCombo) and not op.model.training
        got = op.model.state_dict()
        assert all(torch.equal(got[k].cpu(), v) for k, v in sd.items())
        assert next(op.model.parameters()).is_cuda
    (cd / "epoch-10.ckp").unlink()
    with pytest.raises(FileNotFoundError):
        op.build_model(load_pretrained_model=False)


def test_gen_motion_driver_writes_readable_files(tmp_path):
    out = tmp_path / "gen"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "exp_GAMMAPrimitive", "gen_motion.py"), "--n-primitives", "2", "--n-gens", "2",
                        "--seed", "3", "--num-verts", str(V_SMALL), "--out", str(out)], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    files = sorted(f for f in os.listdir(out) if f.startswith("motion_") and f.endswith(".pkl"))
    assert len(files) == 2, files
    for f in files:
        with open(out / f, "rb") as fh:
            node = pickle.load(fh)
        assert len(node["motion"]) == 2 and node["motion"][0]["smplx_params"].shape == (1, 20, 93)
    assert "frames: 38" in r.stdout, r.stdout[-500:]
