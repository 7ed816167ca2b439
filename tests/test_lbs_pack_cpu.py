"""The model packing (egogen_amd/csrc/lbs_pack.hip) on the CPU: tests/lbs_pack_check.hip, a stand-alone host program, packs body
descriptions and prints a hash of every packed array, the scalars, the vertex permutation and the band constants.  Its output for
the built-in models is compared with tests/golden/lbs_pack_check.txt, which was recorded from egx_body_model_create as it was
before the packing became a unit of its own (profiles/lbs_pack.md); for a synthetic body it is compared with the Python mirrors of
tests/lbs_mode3.py."""
import os
import struct
import subprocess

import numpy as np
import pytest

from egogen_amd import synth
from tests import lbs_mode3 as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "lbs_pack_check.txt")


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("lbs_pack") / "lbs_pack_check"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-O2", "-std=c++17", "--cuda-host-only", "-Wall", "-Wno-unused-function",
                    os.path.join(ROOT, "tests", "lbs_pack_check.hip"), os.path.join(ROOT, "egogen_amd", "csrc", "lbs_pack.hip"),
                    "-o", str(exe)], check=True)
    return str(exe)


def write_raw(path, bm, marker_vids, feet_vids):
    """a body description as the raw file `lbs_pack_check raw` reads (fp32 / int32, the field order of egx_body_model_host)"""
    f32 = lambda k: np.ascontiguousarray(bm[k], np.float32)
    i32 = lambda a: np.ascontiguousarray(a, np.int32)
    V = bm["v_template"].shape[0]
    assert f32("shapedirs").shape == (V, 3, 10) and f32("posedirs").shape == (486, 3 * V)
    marker, feet = i32(marker_vids), i32(feet_vids)
    parts = [i32([V, len(marker), len(feet)]), f32("v_template"), f32("shapedirs"), f32("posedirs"), f32("J_regressor"),
             i32(bm["parents"]), f32("lbs_weights"), f32("hand_comps_l"), f32("hand_comps_r"), f32("hand_mean_l"), f32("hand_mean_r"),
             i32(bm["extra_vids"]), i32(bm["lmk_vids"]), f32("lmk_bary"), marker, feet]
    with open(path, "wb") as f:
        for p in parts:
            f.write(p.tobytes())


def floats(fields):
    return np.array([struct.unpack("<f", struct.pack("<I", int(x, 16)))[0] for x in fields], np.float32)


def test_packed_bytes_match_the_recorded_ones(check_exe):
    """every hash, scalar, permutation and band constant of the built-in models, and every error return (EGX_ERR_ARG, its message,
    nothing packed: the program asserts that, and that the models reach every branch of the packing)"""
    got = subprocess.run([check_exe], check=True, capture_output=True, text=True).stdout.splitlines()
    want = open(GOLDEN).read().splitlines()
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w, (g[:160], w[:160])
    errors = [l for l in got if l.startswith("error.")]
    assert [l.split()[0] for l in errors] == ["error." + n for n in ("marker_id", "extra_id", "landmark_id", "feet_id", "parents", "null_table")]
    assert all(l.split()[1] == "rc=-1" and len(l.split()) > 2 for l in errors)


def test_python_mirrors_match_the_packing(check_exe, tmp_path):
    """kernel_vertex_order and model_consts of tests/lbs_mode3.py against the C++ they mirror, bit for bit"""
    V = 300
    bm = synth.make_body_model(0, num_verts=V)
    marker, feet = synth.marker_ids(V), synth.feet_vids(V)
    raw = tmp_path / "body.raw"
    write_raw(raw, bm, marker, feet)
    out = subprocess.run([check_exe, "raw", str(raw)], check=True, capture_output=True, text=True).stdout.splitlines()
    rec = {l.split()[0]: l.split()[1:] for l in out}
    perm = [int(x) for x in rec["raw.permutation"]]
    assert len(perm) == (V + 31) // 32 * 32 and perm[V:] == [-1] * (len(perm) - V)
    assert perm[:V] == list(L.kernel_vertex_order(bm, marker, feet))
    c = L.model_consts(bm)
    f32 = lambda x: np.asarray(x, np.float64).astype(np.float32)
    fix_c, fix_d = floats(rec["raw.band.fix_c"]), floats(rec["raw.band.fix_d"])
    np.testing.assert_array_equal(fix_c[L.MOVABLE], f32(c["C"]))
    np.testing.assert_array_equal(fix_d[L.MOVABLE], f32(c["D"]))
    np.testing.assert_array_equal(floats(rec["raw.band.shape_c"]), f32(c["S"]))
    for name, key in (("fix_pf", "PF"), ("fix_dpf", "DPF"), ("vt_max", "vt_max"), ("w_abs_max", "w_abs_max")):
        assert floats(rec["raw.band." + name])[0] == f32(c[key]), (name, floats(rec["raw.band." + name])[0], c[key])
