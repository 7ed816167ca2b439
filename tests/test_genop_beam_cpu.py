"""CPU checks of the beam search's specification (tests/genop_beam_ref.py; no GPU):

  1. `beam_select` on hand-made tables: ties by index, a colliding path against a costlier clean one, `ncoll` carried over depth,
     non-finite rows last, fewer finite rows than W;
  2. `beam_chain` with W = 1 is `search_chain`: the same choices and records;
  3. `backtrack` against hand-walked parent tables;
  4. the C header and the ctypes table agree on the three new entries."""
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import genop_beam_ref as bref, genop_search_ref as sref
from tests.helpers import load_golden, seeded_prior_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
NEW_ENTRIES = ("egx_primitive_beam_select", "egx_primitive_advance_beam", "egx_beam_backtrack")


def beam_cases():
    """name -> (W, N, cost[W*N], colliding[W*N], nan_term_rows, acc[W], ncoll[W], beam_row[W], ncoll_out[W], status[W]).  Every
    weight but the goal's is 0 in these tables, so q = 0 and a path's cost is acc[parent] + cost.  Shared with the GPU test."""
    return {
        "exact ties: the lowest rows, in row order": (2, 2, [1.0, 1.0, 1.0, 1.0], [0, 0, 0, 0], (), [0.0, 0.0], [0, 0], [0, 1], [0, 0], [0, 0]),
        "a tie across parents: acc + cost decides, then the row": (2, 2, [3.0, 2.0, 1.0, 2.0], [0, 0, 0, 0], (), [0.0, 1.0], [0, 0],
                                                                  [1, 2], [0, 0], [0, 0]),
        "a colliding cheap row loses to a costlier clean one": (2, 2, [0.1, 5.0, 7.0, 0.2], [1, 0, 0, 1], (), [0.0, 0.0], [0, 0], [1, 2],
                                                                [0, 0], [0, 0]),
        "a parent's collisions outweigh any cost": (2, 2, [0.1, 0.2, 8.0, 9.0], [0, 0, 0, 0], (), [0.0, 50.0], [1, 0], [2, 3], [0, 0], [0, 0]),
        "ncoll accumulates: a clean child of a collided path ties a colliding child of a clean one": (
            2, 2, [4.0, 5.0, 1.0, 6.0], [0, 0, 1, 0], (), [0.0, 0.0], [1, 0], [3, 2], [0, 1], [0, 1]),
        "non-finite rows rank last, by collisions then row": (2, 2, [NAN, 9.0, INF, 8.0], [0, 1, 0, 0], (), [0.0, 0.0], [0, 0], [3, 1], [0, 1],
                                                              [0, 1]),
        "a row with a non-finite term counts as non-finite": (2, 2, [0.5, 4.0, 6.0, 7.0], [0, 0, 0, 0], (0,), [0.0, 0.0], [0, 0], [1, 2], [0, 0],
                                                              [0, 0]),
        "fewer finite rows than W: the non-finite ones fill the beam": (3, 1, [NAN, 2.0, INF], [1, 0, 0], (), [0.0, 0.0, 0.0], [0, 0, 0],
                                                                        [1, 2, 0], [0, 0, 1], [0, 2, 3]),
        "W = 1 is the greedy rule": (1, 3, [0.1, 5.0, 7.0], [1, 0, 0], (), [0.0], [0], [1], [0], [0]),
        "one row": (1, 1, [4.0], [1], (), [2.0], [3], [0], [4], [1]),
    }


GOAL_ONLY = {"goal": 1.0, "skate": 0.0, "floor": 0.0, "pene": 0.0, "face": 0.0}


@pytest.mark.parametrize("name", list(beam_cases()))
def test_beam_selection_rules(name):
    W, N, cost, coll, nan_rows, acc, ncoll, want_rows, want_ncoll, want_status = beam_cases()[name]
    cost = torch.tensor([cost], dtype=torch.float32)
    terms = torch.zeros(1, W * N, 5)
    for n in nan_rows:
        terms[0, n, 2] = NAN
    r = bref.beam_select(cost, terms, torch.tensor([coll]), torch.tensor([acc]), torch.tensor([ncoll]), W, N, GOAL_ONLY)
    assert r["beam_row"][0].tolist() == want_rows, (name, r["beam_row"])
    assert r["parent"][0].tolist() == [x // N for x in want_rows]
    assert r["ncoll"][0].tolist() == want_ncoll and r["status"][0].tolist() == want_status, (name, r["ncoll"], r["status"])
    for s, row in enumerate(want_rows):
        if not want_status[s] & 2:
            assert float(r["path_cost"][0, s]) == acc[row // N] + float(cost[0, row])
        else:
            assert float(r["path_cost"][0, s]) == 0.0


def test_beam_selection_carries_q_not_the_goal_term():
    """acc grows by q = w_skate skate + w_floor floor + w_pene pene + w_face face of the kept row, summed in that order on its own."""
    w = {"goal": 2.0, "skate": 3.0, "floor": 0.5, "pene": 0.25, "face": 4.0}
    terms = torch.tensor([[[1.0, 0.1, 0.2, 0.4, 0.05], [0.5, 1.0, 1.0, 1.0, 1.0]]])
    cost = (terms * torch.tensor([2.0, 3.0, 0.5, 0.25, 4.0])).sum(-1)
    r = bref.beam_select(cost, terms, torch.zeros(1, 2, dtype=torch.bool), torch.tensor([[10.0]]), torch.tensor([[0]]), 1, 2, w)
    assert r["beam_row"].tolist() == [[0]]
    q = torch.tensor(3.0) * 0.1 + torch.tensor(0.5) * 0.2 + torch.tensor(0.25) * 0.4 + torch.tensor(4.0) * 0.05
    assert float(r["acc"][0, 0]) == float(torch.tensor(10.0) + q) and float(r["path_cost"][0, 0]) == float(10.0 + cost[0, 0])


def test_beam_selection_is_per_sequence():
    names = [n for n in beam_cases() if beam_cases()[n][0] == 2 and beam_cases()[n][1] == 2 and not beam_cases()[n][4]]
    col = lambda j: [beam_cases()[n][j] for n in names]
    r = bref.beam_select(torch.tensor(col(2)), torch.zeros(len(names), 4, 5), torch.tensor(col(3)), torch.tensor(col(5)), torch.tensor(col(6)),
                         2, 2, GOAL_ONLY)
    assert r["beam_row"].tolist() == col(7) and r["ncoll"].tolist() == col(8) and r["status"].tolist() == col(9)


# ----------------------------------------------------------------------------------------------------------------------
def test_backtrack_walks_the_parents():
    #            depth 0 (unused)   depth 1                depth 2: slots 0 and 1 share parent 2   depth 3
    parent = [[[0, 0, 0]], [[1, 0, 2]], [[2, 2, 0]], [[1, 0, 2]]]
    # by hand: depth 3 slot 0 -> parent 1 = slot at depth 2; parent[2][1] = 2 = slot at depth 1; parent[1][2] = 2 = slot at depth 0
    assert bref.backtrack(torch.tensor(parent), 4)[:, 0].tolist() == [2, 2, 1, 0]
    two = torch.tensor([[[0, 0, 0], [0, 0, 0]], [[2, 1, 0], [0, 1, 2]]])
    assert bref.backtrack(two, 2).tolist() == [[2, 0], [0, 0]]
    assert bref.backtrack(torch.tensor([[[0, 0, 0]] * 5]), 1).tolist() == [[0] * 5]          # K = 1: the best slot itself


def test_beam_chain_with_one_slot_is_the_search_chain():
    from egogen_amd import synth
    from oracle.smplx_lbs import BodyModel
    g = load_golden("env_step_ref.npz")
    pre, K, N, V = "free_", 2, 3, 2048
    sd = seeded_prior_state_dict(int(g["prior_seed"]), *[float(v) for v in g["prior_gains"]])
    rf = float(json.loads(str(g["cfg_json"]))["modelconfig"]["reproj_factor"])
    bm = BodyModel(synth.make_body_model(0, num_verts=V), dtype=torch.float32)
    z = torch.randn(K, N, 128, generator=torch.Generator().manual_seed(11))
    args = (g[pre + "reset_state"][None, :, :201], g[pre + "reset_seed"][None], g[pre + "reset_R0"].reshape(1, 3, 3),
            g[pre + "reset_T0"].reshape(1, 3), g[pre + "betas"].reshape(1, 10), z, g[pre + "reset_wpath"][-1].reshape(1, 3))
    w = {"goal": 1.0, "skate": 2.0, "floor": 0.5, "pene": 0.3, "face": 0.7}
    want = sref.search_chain(sd, bm, synth.marker_ids(V), synth.feet_marker_idx(), *args, N, rf, w)
    steps, path = bref.beam_chain(sd, bm, synth.marker_ids(V), synth.feet_marker_idx(), *args, 1, N, rf, w)
    assert len({int(s["choice"][0]) for s in want}) > 1 or int(want[0]["choice"][0]) != 0       # the chain does choose
    for k in range(K):
        assert torch.equal(steps[k]["beam_row"][:, 0], want[k]["choice"]) and torch.equal(path[k]["choice"], want[k]["choice"])
        assert torch.equal(steps[k]["status"][:, 0], want[k]["status"]) and int(path[k]["slot"][0]) == 0
        assert torch.equal(steps[k]["cost"], want[k]["cost"]) and torch.equal(steps[k]["terms"], want[k]["terms"])
        assert torch.equal(path[k]["goal_dist"], want[k]["goal_dist"])
        for key in ("marker_b", "pelvis", "R", "T", "R0", "T0", "seed_params", "seed_markers", "pred_params"):
            assert torch.equal(steps[k][key], want[k][key]), (k, key)
        for key in ("marker_b", "pelvis", "R", "T", "pred_params"):
            assert torch.equal(path[k][key], want[k][key]), (k, key)


def test_new_entries_are_declared_and_bound():
    from egogen_amd import _lib, genop
    txt = open(os.path.join(ROOT, "include", "egogen_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in NEW_ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", txt), name
        assert name in _lib.SIGNATURES, name
        decl = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", txt, flags=re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name           # as many arguments on both sides
    assert re.search(r"#define\s+EGX_MAX_BEAM\s+32\b", txt) and genop.MAX_BEAM == 32
    assert re.search(r"#define\s+EGX_MAX_CANDIDATES\s+" + str(genop.MAX_CANDIDATES) + r"\b", txt)
