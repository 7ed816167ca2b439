"""The merged launches of the update chain's backward pass (csrc/update3.hip: the output layer's weight gradients with the first
input gradients, the layers' eight weight gradients in one launch, for a whole minibatch together with the encoders' four) against
the sequence they replace (EGX_UPDATE_MERGE=0, read when a train handle is created).

A merged launch runs every product in the kernel configuration of its old launch and changes nothing else, so everything except
the loss sums (float atomics) is held to `torch.equal`: the flat gradient of every optimiser step, the parameters, both moments
and every weight image after the last one.  The synthetic rollout (4 x 24 = 96 rows) and the initial weights are those of
tests/test_update_head_gpu.py.
"""
import pytest
import torch

from tests import test_update_head_gpu as uh

pytestmark = pytest.mark.gpu

_SENT = -777.25   # exact in fp32
# egx_dense3_kernel launches of one call: forward 5 (four layers, the output layers) + backward; see train_step_parts
_DENSE3 = {True: {"all": 12, "heads": 11, "encoders": 2}, False: {"all": 15, "heads": 13, "encoders": 2}}


class _DeviceBytes:
    """`nbytes` of device memory at `ptr` (an arena of a train handle) for torch.as_tensor."""

    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (int(ptr), False), "version": 2}


def _image_bytes(rows, red):
    """csrc/d3.h: an even count of 16-row tiles x ceil(red / 32) k-steps of 3 planes x 64 lanes x 16 bytes."""
    return 2 * ((rows + 31) // 32) * ((red + 31) // 32) * 3 * 64 * 16


def _weight_images(pol):
    """Copies of every weight image `egx_policy_train_packed` names, of every handle of `pol`."""
    out = {}
    for n, hs in sorted(pol._train_handles.items()):
        pk = hs["packed"]
        imgs = [("x_enc_w_ih", pk.x_enc_w_ih, 1536, 402), ("x_enc_w_hh", pk.x_enc_w_hh, 1536, 512),
                ("ego_enc_w_ih", pk.ego_enc_w_ih, 1536, 32), ("ego_enc_w_hh", pk.ego_enc_w_hh, 1536, 512),
                ("actor_out_w", pk.actor_out_w, 256, 1152), ("critic_out_w", pk.critic_out_w, 1, 1152)]
        imgs += [(f"actor_w{l}", pk.actor_w[l], 1152, 1152) for l in range(4)]
        imgs += [(f"critic_w{l}", pk.critic_w[l], 1152, 1152) for l in range(4)]
        for name, ptr, rows, red in imgs:
            out[(n, name)] = torch.as_tensor(_DeviceBytes(ptr, _image_bytes(rows, red)), device="cuda").clone()
    return out


def _lib():
    from egogen_amd import _lib as L
    return L.load()


def _sentinel_mask(pol, lo):
    """The elements of the flat gradient at or behind `lo` that belong to a tensor (the alignment padding between tensors stays
    zero in every flat buffer: no kernel of the chain writes it, and AdamW's norm reads it)."""
    mask = torch.zeros(pol._flat_grad.numel(), dtype=torch.bool, device="cuda")
    for _, off, cnt in pol._flat_layout():
        if off >= lo:
            mask[off:off + cnt] = True
    return mask


def _run_learn(monkeypatch, merge, graph, prec, batch_size):
    """One learn() pass of three optimiser steps (minibatch 32) or one (64: the ragged rest merges into a 96-row minibatch)."""
    monkeypatch.setenv("EGX_UPDATE_HEAD", "1")
    monkeypatch.setenv("EGX_UPDATE_MERGE", "1" if merge else "0")
    pol = uh._new_policy(graph, prec)
    grads = []
    pol._after_minibatch = lambda i: grads.append(pol._flat_grad.clone())
    stats = pol.learn(uh._batch(), batch_size, 1)
    torch.cuda.synchronize()
    assert pol._train_handles
    for hs in pol._train_handles.values():
        assert _lib().egx_policy_train_dense3_launches(hs["h"]) == _DENSE3[merge]["all"]
    return pol, stats, grads, _weight_images(pol)


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("prec", ["bf16x2", "f32"])
@pytest.mark.parametrize("batch_size", [32, 64])
def test_merged_launches_train_bit_for_bit_like_the_old_sequence(monkeypatch, batch_size, prec, graph):
    new = _run_learn(monkeypatch, True, graph, prec, batch_size)
    old = _run_learn(monkeypatch, False, graph, prec, batch_size)
    want = {"chain+graph" if graph else "chain": 3} if batch_size == 32 else {"chain": 1}
    assert new[0].update_paths == want, new[0].update_paths
    uh._assert_same_training(new[:3], old[:3])   # every flat gradient, p, m, v; the loss terms within 1e-5 max(1, |x|)
    assert new[3].keys() == old[3].keys() and len(new[3]) == 14
    for key in new[3]:
        assert torch.equal(new[3][key], old[3][key]), f"weight image {key}"


def _halves_steps(monkeypatch, merge, prec, n, steps=3):
    """`steps` optimiser steps of minibatch n, each as egx_policy_train_step_heads_cursor then egx_policy_train_step_encoders on a
    flat gradient whose encoder tensors - all of [n_clip, total) but the alignment padding - hold a sentinel.  Returns the policy,
    per step the flat gradient after the heads' half, after the encoders' half and the loss terms, and the final weight images."""
    monkeypatch.setenv("EGX_UPDATE_HEAD", "1")
    monkeypatch.setenv("EGX_UPDATE_MERGE", "1" if merge else "0")
    pol = uh._new_policy(False, prec)
    pol._ensure_flat_grads()
    assert pol._flat_optimizer_ready()
    hs = pol._train_handle(n)
    assert hs is not None and hs["head"]
    nc, total = pol._n_clip, pol._flat_grad.numel()
    assert 0 < nc < total
    enc = _sentinel_mask(pol, nc)
    assert bool(enc.any()) and not bool(enc[:nc].any())
    b = uh._batch()
    perm = torch.randperm(uh.N, generator=torch.Generator().manual_seed(17)).cuda()
    after_heads, after_enc, logs = [], [], []
    for k in range(steps):
        idx = perm[(k * n) % (uh.N - n + 1):][:n].contiguous()
        log = torch.zeros(6, device="cuda")
        pol._flat_grad[enc] = _SENT
        before = pol._flat_grad.clone()
        pol._fwd_bwd_train_step(hs, b, idx, None, log, part="heads")
        assert _lib().egx_policy_train_dense3_launches(hs["h"]) == _DENSE3[merge]["heads"]
        torch.cuda.synchronize()
        g = pol._flat_grad.clone()
        assert torch.equal(g[nc:], before[nc:]), "the heads' half wrote into the encoders' part of the flat gradient"
        after_heads.append(g)
        pol._fwd_bwd_train_step(hs, b, idx, None, log, part="encoders")
        assert _lib().egx_policy_train_dense3_launches(hs["h"]) == _DENSE3[merge]["encoders"]
        torch.cuda.synchronize()
        g2 = pol._flat_grad.clone()
        assert torch.equal(g2[:nc], g[:nc]), "[0, n_clip) was not final after the heads' half"
        assert not bool((g2[enc] == _SENT).any()), "an encoder gradient was left unwritten"
        assert torch.equal(g2[~enc][nc:], before[~enc][nc:]), "the padding behind n_clip was written"
        after_enc.append(g2)
        logs.append(log.cpu())
        pol._clip_and_step()
    torch.cuda.synchronize()
    return pol, after_heads, after_enc, logs, _weight_images(pol)


@pytest.mark.parametrize("prec", ["bf16x2", "f32"])
@pytest.mark.parametrize("n", [32, 64])
def test_the_two_halves_entry_points(monkeypatch, n, prec):
    """Data-parallel training runs the chain as two calls and all-reduces [0, n_clip) while the second runs: merged, the heads'
    half still finalises exactly that prefix (its eight weight gradients go out at its end, the encoders' four at theirs)."""
    new = _halves_steps(monkeypatch, True, prec, n)
    old = _halves_steps(monkeypatch, False, prec, n)
    for k in range(3):
        assert torch.equal(new[1][k], old[1][k]), f"flat gradient after the heads' half of step {k}"
        assert torch.equal(new[2][k], old[2][k]), f"flat gradient of step {k}"
        for a, c in zip(new[3][k].tolist(), old[3][k].tolist()):
            assert abs(a - c) <= 1e-5 * max(1.0, abs(c)), (k, new[3][k], old[3][k])
    for name in ("_flat_p", "_flat_m", "_flat_v"):
        assert torch.equal(getattr(new[0], name), getattr(old[0], name)), name
    for key in new[4]:
        assert torch.equal(new[4][key], old[4][key]), f"weight image {key}"


def test_halves_and_whole_minibatch_leave_the_same_gradient(monkeypatch):
    """The whole-minibatch call defers the layers' weight gradients behind the encoders' backward; the halves do not."""
    monkeypatch.setenv("EGX_UPDATE_HEAD", "1")
    monkeypatch.setenv("EGX_UPDATE_MERGE", "1")
    halves = _halves_steps(monkeypatch, True, "bf16x2", 32, steps=1)
    pol = uh._new_policy(False, "bf16x2")
    pol._ensure_flat_grads()
    assert pol._flat_optimizer_ready()
    hs = pol._train_handle(32)
    perm = torch.randperm(uh.N, generator=torch.Generator().manual_seed(17)).cuda()
    pol._flat_grad[_sentinel_mask(pol, 0)] = _SENT
    pol._fwd_bwd_train_step(hs, uh._batch(), perm[:32].contiguous(), None, torch.zeros(6, device="cuda"))
    assert _lib().egx_policy_train_dense3_launches(hs["h"]) == _DENSE3[True]["all"]
    torch.cuda.synchronize()
    assert torch.equal(pol._flat_grad, halves[2][0])
