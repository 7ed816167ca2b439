#!/usr/bin/env python3
"""tests/golden/calc_sdf_grad_ref.npz: the reference's own calc_sdf (crowd_ppo/utils.py:54-84, imported as scripts/gen_goldens.py
imports it - build container only) and its torch-autograd gradient of sum(values * cotangent) with respect to the vertices, in
float32 and float64, on the grids and points of tests/sdf_grad_ref.py::golden_inputs.  Data only."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))

import gen_goldens as gg                      # noqa: E402  (the reference's location, the import stubs, the output folder)
from tests import sdf_grad_ref as ref         # noqa: E402


def main():
    gg.install_stubs()
    # by file: the repository has a package called crowd_ppo of its own
    import importlib.util
    spec = importlib.util.spec_from_file_location("reference_crowd_ppo_utils", os.path.join(gg.REF, "crowd_ppo", "utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    calc_sdf = mod.calc_sdf
    torch.set_num_threads(1)
    out = {"center": ref.CENTER, "scale": np.float32(ref.SCALE), "n_interior": np.int64(ref.N_INTERIOR)}
    for tag, dims in ref.GOLDEN_CASES:
        grid, pts, cot = ref.golden_inputs(tag, dims)
        out[f"{tag}_sdf"], out[f"{tag}_pts"], out[f"{tag}_cot"] = grid, pts, cot
        for dtype, suffix in ((torch.float32, "32"), (torch.float64, "64")):
            val, grad = ref.autograd_of(calc_sdf, pts, ref.sdf_dict(grid, dtype=dtype), cot, dtype)
            out[f"{tag}_val{suffix}"], out[f"{tag}_grad{suffix}"] = val, grad
        cv, cg = ref.closed_form(pts, grid, ref.CENTER, ref.SCALE)
        print(tag, dims, "closed form (float64) vs the reference: values", np.abs(cv - out[f"{tag}_val64"]).max(), "gradient",
              np.abs(cg * cot[:, None].astype(np.float64) - out[f"{tag}_grad64"]).max())
    os.makedirs(gg.OUT, exist_ok=True)
    path = os.path.join(gg.OUT, "calc_sdf_grad_ref.npz")
    np.savez_compressed(path, **out)
    print("calc_sdf_grad_ref", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
