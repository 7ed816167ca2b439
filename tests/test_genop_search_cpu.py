"""CPU checks of the primitive search's specification (tests/genop_search_ref.py; no GPU):

  1. `score` in float32 on the recorded steps of tests/golden/env_step_ref.npz reproduces what the reference's own
     `CrowdEnv.step` computed: skate = -ln r_skate, floor = -ln r_floor, pene = -ln r_pene (from the recorded pene_count),
     face = 1 - r_face_target, dist = after_dist, colliding = penetration; bar of tests/test_genop_cpu.py (1e-4 |ref| + 2e-5).
     The recorded rewards are float32, so -ln r carries their rounding divided by r: half a float32 ulp of r, 2^-24, in
     absolute terms whatever r is - below the floor of the bar as long as r is a normal number (asserted);
  2. the selection rules on hand-made cost tables;
  3. `search_chain` with one candidate is `genop_ref.chain`."""
import json

import numpy as np
import pytest
import torch

from tests import genop_ref, genop_search_ref as sref
from tests.helpers import load_golden, seeded_prior_state_dict
from tests.test_genop_cpu import _close

NAN, INF = float("nan"), float("inf")


def _recorded_steps():
    g = load_golden("env_step_ref.npz")
    out = []
    for case in [str(c) for c in g["cases"]]:
        for i in range(int(g[f"{case}_n_steps"])):
            out.append((case, i))
    return out


@pytest.mark.parametrize("case,i", _recorded_steps())
def test_score_restatement_matches_reference_step(case, i):
    from egogen_amd import synth
    g = load_golden("env_step_ref.npz")
    pre, sp = case + "_", f"{case}_s{i}_"
    R0 = g[pre + "reset_R0"] if i == 0 else g[f"{pre}s{i - 1}_after_R0"]
    T0 = g[pre + "reset_T0"] if i == 0 else g[f"{pre}s{i - 1}_after_T0"]
    mb = g[sp + "marker_b"].reshape(1, 20, 67, 3)
    cnt = g[sp + "pene_count"].reshape(1, 20)
    # reproj_factor = 1 with the recorded blended markers as the projected ones: mb = 1 * marker_b + 0 * (anything finite)
    r = sref.score(np.zeros((18, 1, 201), np.float32), np.zeros((2, 1, 201), np.float32), g[sp + "joints"][None], mb,
                   R0.reshape(1, 3, 3), T0.reshape(1, 3), cnt, g[sp + "after_wpath"][-1].reshape(1, 3), synth.feet_marker_idx(),
                   reproj_factor=1.0, dtype=torch.float32)
    for term, key in (("skate", "r_skate"), ("floor", "r_floor"), ("pene", "r_pene")):
        rec = float(g[sp + key])
        assert rec >= np.finfo(np.float32).tiny, (term, rec)
        _close(r[term], np.asarray([-np.log(np.float64(rec))]), sp + term)
    _close(r["face"], np.asarray([1.0 - np.float64(g[sp + "r_face_target"])]), sp + "face")
    _close(r["dist"], np.asarray(g[sp + "after_dist"], np.float64).reshape(1), sp + "dist")
    assert bool(r["colliding"][0]) == bool(g[sp + "penetration"]), sp
    assert int(cnt.max()) == int(g[sp + "num_inside_max"])


# ----------------------------------------------------------------------------------------------------------------------
def selection_cases():
    """name -> (cost[N], colliding[N], nan_term_rows, expected choice, expected status); shared with the GPU test."""
    return {
        "a colliding cheap row loses to a clean dear one": ([0.1, 5.0, 7.0], [1, 0, 0], (), 1, 0),
        "all rows colliding: the cheapest, status bit 0": ([3.0, 2.0, 2.5], [1, 1, 1], (), 1, 1),
        "a NaN row is never chosen while a finite one exists": ([NAN, 9.0, INF], [0, 1, 0], (), 1, 1),
        "a row with a non-finite term counts as non-finite": ([0.5, 4.0, 6.0], [0, 0, 0], (0,), 1, 0),
        "all rows non-finite: status bit 1, collision then index decide": ([NAN, INF, NAN], [1, 0, 0], (), 1, 2),
        "all rows non-finite and colliding: both bits": ([NAN, NAN], [1, 1], (), 0, 3),
        "exact ties: the lowest index": ([2.0, 1.0, 1.0, 1.0], [0, 0, 0, 0], (), 1, 0),
        "one candidate": ([4.0], [0], (), 0, 0),
        "one colliding candidate": ([4.0], [1], (), 0, 1),
    }


@pytest.mark.parametrize("name", list(selection_cases()))
def test_selection_rules(name):
    cost, coll, nan_rows, want, status = selection_cases()[name]
    cost = torch.tensor([cost], dtype=torch.float32)
    terms = torch.zeros(1, cost.shape[1], 5)
    for n in nan_rows:
        terms[0, n, 2] = NAN
    choice, st = sref.select(cost, terms, torch.tensor([coll]))
    assert int(choice[0]) == want and int(st[0]) == status, (name, int(choice[0]), int(st[0]))


def test_selection_is_per_sequence():
    names = list(selection_cases())
    three = [n for n in names if len(selection_cases()[n][0]) == 3 and not selection_cases()[n][2]]
    cost = torch.tensor([selection_cases()[n][0] for n in three])
    coll = torch.tensor([selection_cases()[n][1] for n in three])
    choice, st = sref.select(cost, torch.zeros(len(three), 3, 5), coll)
    assert choice.tolist() == [selection_cases()[n][3] for n in three]
    assert st.tolist() == [selection_cases()[n][4] for n in three]


# ----------------------------------------------------------------------------------------------------------------------
def test_search_chain_with_one_candidate_is_the_chain():
    from egogen_amd import synth
    from oracle.smplx_lbs import BodyModel
    g = load_golden("env_step_ref.npz")
    pre, n = "free_", 2
    sd = seeded_prior_state_dict(int(g["prior_seed"]), *[float(v) for v in g["prior_gains"]])
    rf = float(json.loads(str(g["cfg_json"]))["modelconfig"]["reproj_factor"])
    bm = BodyModel(synth.make_body_model(0), dtype=torch.float32)
    z = torch.as_tensor(g[pre + "z"][:n]).reshape(n, 1, 128)
    args = (g[pre + "reset_state"][None, :, :201], g[pre + "reset_seed"][None], g[pre + "reset_R0"].reshape(1, 3, 3),
            g[pre + "reset_T0"].reshape(1, 3), g[pre + "betas"].reshape(1, 10), z)
    want = genop_ref.chain(sd, bm, synth.marker_ids(), *args, rf)
    got = sref.search_chain(sd, bm, synth.marker_ids(), synth.feet_marker_idx(), *args, g[pre + "reset_wpath"][-1].reshape(1, 3), 1, rf)
    for k in range(n):
        assert int(got[k]["choice"][0]) == 0 and int(got[k]["status"][0]) == 0
        for key in ("marker_b", "pelvis", "R", "T", "R0", "T0", "seed_params", "seed_markers", "pred_params"):
            assert torch.equal(got[k][key], want[k][key]), (k, key)
        # ... and its distance is the one the reference's step recorded
        _close(got[k]["goal_dist"], np.asarray(g[f"{pre}s{k}_after_dist"], np.float64).reshape(1), f"{pre}s{k} dist")
