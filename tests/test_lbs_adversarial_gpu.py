"""LBS blend mode 3 ("f16mix") on inputs built to break it: a body whose fp16 product errors all align (tests/lbs_mode3.py) placed so
that an SDF level set lies between a vertex's float64 position and its cheap one, and workspaces full of garbage."""
import numpy as np
import pytest
import torch

from egogen_amd import synth
from tests import lbs_mode3 as L

pytestmark = pytest.mark.gpu


def _plane_scene(res=64, half=2.0):
    """grid value = -z (metres): calc_sdf = z, slope exactly 1 per metre; trilinear interpolation of a linear field is exact"""
    lin = (np.arange(res, dtype=np.float64) + 0.5) / res * 2.0 - 1.0
    z = lin * half
    g = np.broadcast_to(-z[None, None, :], (res, res, res))
    return {"sdf": np.ascontiguousarray(g, dtype=np.float32), "center": np.zeros(3, np.float32), "scale": np.float32(1.0 / half)}


def _mode3(tile, cap=0):
    from egogen_amd import _lib
    lib = _lib.load()
    _lib.check(lib.egx_lbs_set_blend_mode(3), "mode")
    _lib.check(lib.egx_lbs_set_wave_tile(tile), "tile")
    _lib.check(lib.egx_lbs_set_fix_queue_capacity(cap), "cap")


def _restore(old_mode):
    from egogen_amd import _lib
    lib = _lib.load()
    _lib.check(lib.egx_lbs_set_blend_mode(old_mode), "mode")
    _lib.check(lib.egx_lbs_set_wave_tile(0), "tile")
    _lib.check(lib.egx_lbs_set_fix_queue_capacity(0), "cap")


def test_lbs_mixed_blend_counts_on_an_adversarial_body():
    """The fix-up band of mode 3 must hold for EVERY rounding pattern of the fp16 product, not only for independent ones.
    The adversarial body (tests/lbs_mode3.py: 96 pelvis-only vertices whose 459 pose-corrective columns each carry the largest
    column norm of their joint, half an fp16 ulp off the grid, signed so that every product error points along +z for one pose)
    moves its cheap vertices by ~4e-4 m - four times the statistical band the kernel used to have.  One body per agent (T = 1),
    all in that pose, over a planar SDF (calc_sdf = world z): 32 bodies are placed so that one adversarial vertex lies at >= 4e-5 m
    on one side of the plane while its cheap position is on the other side by more than that statistical band + 2e-5 (half of them
    flipped upside down by R0, so both wrong decisions occur), 8 where the cheap decision is right, 8 in free space.
    (a) the emulation shows each chosen vertex is mis-classified by a statistical band; (b) the counts equal the float64 oracle's
    within the 2e-5 level-set band; (c) the kernel re-evaluated at least the chosen vertices; (d) wave tile 1 (VALU skinning),
    tile 2 (matrix-pipe skinning) and a fix-up queue of 4 entries per sub-queue (re-evaluation inside the fused kernel) agree."""
    from egogen_amd import _lib
    from egogen_amd.body_model import BodyModelHandle, SdfScene
    from oracle.sdf import calc_sdf
    bm, adv, xb1, be1 = L.adversarial_body()
    V = bm["v_template"].shape[0]
    mk, feet = synth.marker_ids(V), synth.feet_vids(V)
    ex, _, tn = L.exact_forward(bm, xb1, be1)                      # posed, canonical frame (transl 0)
    err_n, err, F, tn = L.cheap_posed_error(bm, xb1, be1, adv)
    stat = L.statistical_band(bm, F, tn)
    n_t, n_ok, n_free = 32, 8, 8
    B = n_t + n_ok + n_free
    R0 = np.tile(np.eye(3), (B, 1, 1))
    T0 = np.zeros((B, 3))
    chosen = []
    for b in range(B):
        i = (7 * b) % len(adv)
        f = -1.0 if b % 2 else 1.0                                 # flipped bodies: world z = -canonical z
        R0[b] = np.diag([1.0, f, f])
        z64, dz = ex[0, adv[i], 2], err[i, 2]
        wz64, wdz = f * z64, f * dz                                # world z (before T0) of the float64 vertex, cheap - float64
        if b < n_t:
            # plane z = 0 between the two: the cheap value on the wrong side by stat + 2e-5 + half of what is left
            room = abs(wdz) - (stat + 2e-5) - 4e-5
            assert room > 0, (abs(wdz), stat)                      # (a)
            sc = np.sign(wdz) * (stat + 2e-5 + 0.5 * room)          # cheap world z after T0
            T0[b, 2] = sc - (wz64 + wdz)
            chosen.append((b, adv[i], wz64 + T0[b, 2], sc))
        elif b < n_t + n_ok:
            T0[b, 2] = -(wz64 + np.sign(wdz) * (3e-4 + abs(wdz)))  # both positions on the same side, 3e-4 m clear
        else:
            T0[b, 2] = 1.2                                          # every vertex above the plane
    for b, v, s64, sc in chosen:                                   # (a) float64 value >= 4e-5 from zero, cheap opposite and past the band
        assert abs(s64) >= 4e-5 and np.sign(s64) != np.sign(sc) and abs(sc) > stat + 2e-5, (b, s64, sc, stat)
    scene = _plane_scene()
    sd = {k: torch.as_tensor(np.asarray(scene[k])).double() for k in ("sdf", "center", "scale")}
    vw = torch.einsum("bij,vj->bvi", torch.as_tensor(R0), torch.as_tensor(ex[0])) + torch.as_tensor(T0)[:, None, :]
    s = calc_sdf(vw, sd)
    s[:, torch.as_tensor(feet).long()] = 1.0
    ref, near = s.lt(0).sum(-1), (s.abs() < 2e-5).sum(-1)
    for b, v, s64, sc in chosen:
        assert abs(float(s[b, v]) - s64) < 1e-9
    assert ref[:n_t].min() > 20 and int(ref[n_t + n_ok:].max()) == 0

    h = BodyModelHandle(bm, mk, feet)
    sc = SdfScene(scene)
    xb = torch.as_tensor(np.tile(xb1, (B, 1))).cuda()
    betas = torch.as_tensor(np.tile(be1, (B, 1))).cuda()
    R0g, T0g = torch.as_tensor(R0, dtype=torch.float32).cuda(), torch.as_tensor(T0, dtype=torch.float32).cuda()
    lib = _lib.load()
    old_mode = int(lib.egx_lbs_get_blend_mode())
    got = {}
    try:
        for name, tile, cap in (("tile2", 2, 0), ("tile1", 1, 0), ("tile2_cap4", 2, 4), ("tile1_cap4", 1, 4)):
            _mode3(tile, cap)
            out = h.forward(xb, betas, 1, sdf=sc, R0=R0g, T0=T0g, out={})
            torch.cuda.synchronize()
            got[name] = (out["pene_count"].cpu().long(), h.fix_stats(B))
    finally:
        _restore(old_mode)
    for name, (cnt, n_fix) in got.items():
        bad = ((cnt - ref).abs() > near).nonzero().flatten().tolist()
        print(f"\n{name}: fix-ups {n_fix}, bodies off the oracle beyond the band: {bad} "
              f"(cheap error {err_n.max():.2e} m, statistical band {stat:.2e} m)")
        assert not bad, (name, bad, (cnt - ref)[bad].tolist())             # (b)
        assert n_fix >= len(chosen), (name, n_fix)                          # (c)
    for name in ("tile1", "tile2_cap4", "tile1_cap4"):
        assert torch.equal(got[name][0], got["tile2"][0]), name             # (d)


@pytest.mark.parametrize("B", [33, 97, 257])
def test_lbs_counts_do_not_depend_on_what_the_workspace_held(B):
    """A call reads only workspace it wrote earlier in the same call: the pose kernel writes the feature images (feat / feat3 /
    feat4), joint transforms (A4), matrix-pipe skinning records (skinB), cell offsets (cinit) and error bounds (fix_e) of every live
    slot and clears the fix-up counters (fix_stats); the fused kernel reads those through lbs_live_slot, which sends the dead columns
    of the last 32-body tile (B % 32 != 0) and of a tile past it to the last live slot; the fix-up queue is read up to the counts this
    call's appends left; `picked` is written by the fused kernel for every pick slot of every body before the gather kernel reads it;
    the culling regions (fvec, jpos, order, flags, items, counts) are written and read only by culled calls, off here.  So counts,
    joints and markers are bit-identical whether the workspace held zeros, 0xFF bytes (NaN in every format) or 0x7F bytes (NaN in
    fp16, 3.4e38 in fp32 and bf16), in every blend mode (mode 3 with the matrix-pipe skinning of wave tile 2)."""
    from egogen_amd import _lib
    from egogen_amd.body_model import BodyModelHandle, SdfScene
    V = 2048
    bm = synth.make_body_model(0, num_verts=V)
    h = BodyModelHandle(bm, synth.marker_ids(V), synth.feet_vids(V))
    g = torch.Generator().manual_seed(B)
    xb = torch.zeros(B, 93)
    xb[:, 0:2] = torch.rand(B, 2, generator=g) * 4 - 2
    xb[:, 2] = 0.3
    xb[:, 3:6] = torch.randn(B, 3, generator=g) * 0.5
    xb[:, 6:69] = torch.randn(B, 63, generator=g) * 0.2
    xb[:, 69:] = torch.randn(B, 24, generator=g) * 0.5
    betas = torch.randn(B, 10, generator=g)
    xb, betas = xb.cuda(), betas.cuda()
    sc = SdfScene(synth.make_sdf_scene(48))
    lib = _lib.load()
    old_mode = int(lib.egx_lbs_get_blend_mode())
    old_cull = int(lib.egx_lbs_get_culling())
    try:
        _lib.check(lib.egx_lbs_set_culling(0), "cull")
        for mode in (0, 1, 2, 3):
            _mode3(2)
            _lib.check(lib.egx_lbs_set_blend_mode(mode), "mode")
            res = []
            for fill in (0x00, 0xFF, 0x7F):
                h.workspace(B).fill_(fill)
                out = h.forward(xb, betas, 1, sdf=sc, out={})
                torch.cuda.synchronize()
                res.append({k: v.clone() for k, v in out.items()})
            assert int(res[0]["pene_count"].sum()) > 0
            for r in res[1:]:
                for k in ("pene_count", "joints", "markers"):
                    assert torch.equal(r[k], res[0][k]), (mode, k)
    finally:
        _restore(old_mode)
        _lib.check(lib.egx_lbs_set_culling(old_cull), "cull")
