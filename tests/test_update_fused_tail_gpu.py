"""The optimiser step's fused tail (`egx_adamw_table_kernel`, csrc/update3.hip: AdamW inside the launch that re-makes the weight
images, `egx_adamw_clip_step_train`) against the two launches it replaces (EGX_UPDATE_FUSED_TAIL=0, read when a train handle is
created: `egx_adamw_flat_kernel`, then the weight `egx_pack3_table_kernel`).

Both run the same element function on the same values, and the images are split from the same updated parameters, so everything
except the loss sums (float atomics in the untouched loss kernel) is held to `torch.equal`: the flat gradient of every optimiser
step, the parameters, both moments and all fourteen weight images after the last one.  The policy's own matrices are the edge
shapes: W_ih of the state encoder [1536, 402] (rows neither 32-column nor 16-byte aligned: element-wise path, ragged last k-step),
W_ih of the ego encoder [1536, 32] (one k-step), the critic's W_out [1, 1152] (one live row of a 32 x 32 block), the actor's
[256, 1152], and the biases and padding for the remainder role.  Rollout, weights and helpers are those of
tests/test_update_head_gpu.py and tests/test_update_merge_gpu.py.
"""
import pytest
import torch

from tests import test_update_head_gpu as uh
from tests import test_update_merge_gpu as um

pytestmark = pytest.mark.gpu


def _lib():
    from egogen_amd import _lib as L
    return L.load()


def _new_policy(monkeypatch, fused, graph, prec):
    monkeypatch.setenv("EGX_UPDATE_HEAD", "1")
    monkeypatch.setenv("EGX_UPDATE_MERGE", "1")
    monkeypatch.setenv("EGX_UPDATE_FUSED_TAIL", "1" if fused else "0")
    return uh._new_policy(graph, prec)


def _assert_tail(pol, fused):
    assert pol._train_handles
    for hs in pol._train_handles.values():
        assert hs["fused_tail"] == fused and _lib().egx_policy_train_fused_tail(hs["h"]) == int(fused)


def _run_learn(monkeypatch, fused, graph, prec, batch_size, n_steps=uh.N_STEPS):
    pol = _new_policy(monkeypatch, fused, graph, prec)
    grads = []
    pol._after_minibatch = lambda i: grads.append(pol._flat_grad.clone())
    stats = pol.learn(uh._batch(n_steps), batch_size, 1)
    torch.cuda.synchronize()
    _assert_tail(pol, fused)
    return pol, stats, grads, um._weight_images(pol)


def _assert_same_images(new, old, count=14):
    assert new.keys() == old.keys() and len(new) == count
    for key in new:
        assert torch.equal(new[key], old[key]), f"weight image {key}"


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("prec", ["bf16x2", "f32"])
@pytest.mark.parametrize("batch_size", [32, 64])
def test_fused_tail_trains_bit_for_bit_like_the_two_launches(monkeypatch, batch_size, prec, graph):
    """Minibatch 32: three optimiser steps (replayed graphs with `graph`); 64: the ragged rest merges into one 96-row minibatch."""
    new = _run_learn(monkeypatch, True, graph, prec, batch_size)
    old = _run_learn(monkeypatch, False, graph, prec, batch_size)
    want = {"chain+graph" if graph else "chain": 3} if batch_size == 32 else {"chain": 1}
    assert new[0].update_paths == want, new[0].update_paths
    uh._assert_same_training(new[:3], old[:3])   # every flat gradient, p, m, v; the loss terms within 1e-5 max(1, |x|)
    _assert_same_images(new[3], old[3])
    assert new[0].refresh_counts == old[0].refresh_counts   # a fused step counts as the refresh it contains


def _halves_steps(monkeypatch, fused, prec, n, steps=3):
    """`steps` optimiser steps of minibatch n through the two-halves entry points (data-parallel training's), each followed by the
    optimiser step of that minibatch's handle."""
    pol = _new_policy(monkeypatch, fused, False, prec)
    pol._ensure_flat_grads()
    assert pol._flat_optimizer_ready()
    hs = pol._train_handle(n)
    assert hs is not None and hs["head"]
    _assert_tail(pol, fused)
    b = uh._batch()
    perm = torch.randperm(uh.N, generator=torch.Generator().manual_seed(17)).cuda()
    grads, logs = [], []
    for k in range(steps):
        idx = perm[(k * n) % (uh.N - n + 1):][:n].contiguous()
        log = torch.zeros(6, device="cuda")
        pol._fwd_bwd_train_step(hs, b, idx, None, log, part="heads")
        pol._fwd_bwd_train_step(hs, b, idx, None, log, part="encoders")
        grads.append(pol._flat_grad.clone())
        logs.append(log.cpu())
        pol._clip_and_step(n=n)
    torch.cuda.synchronize()
    return pol, grads, logs, um._weight_images(pol)


@pytest.mark.parametrize("prec", ["bf16x2", "f32"])
@pytest.mark.parametrize("n", [32, 64])
def test_the_two_halves_entry_points(monkeypatch, n, prec):
    new = _halves_steps(monkeypatch, True, prec, n)
    old = _halves_steps(monkeypatch, False, prec, n)
    for k in range(3):
        assert torch.equal(new[1][k], old[1][k]), f"flat gradient of step {k}"
        for a, c in zip(new[2][k].tolist(), old[2][k].tolist()):
            assert abs(a - c) <= 1e-5 * max(1.0, abs(c)), (k, new[2][k], old[2][k])
    for name in ("_flat_p", "_flat_m", "_flat_v"):
        assert torch.equal(getattr(new[0], name), getattr(old[0], name)), name
    _assert_same_images(new[3], old[3])


def _planes_differ(img, plane):
    """Whether plane `plane` of a packed image ([fragments][3 planes][64 lanes][16 bytes]) holds anything but zeros."""
    return bool(img.view(-1, 3, 64 * 16)[:, plane].any())


def test_rollout_precision_of_three_planes_with_an_update_of_two(monkeypatch):
    """The planes written are the maximum of the update's and the rollout's (egx_policy_train_refresh's rule): with a two-plane
    update and the three-plane rollout default the third plane follows every step; with both at two planes it is left alone."""
    from egogen_amd import _lib as L
    lib = _lib()
    assert lib.egx_policy_get_precision() == 0
    new = _run_learn(monkeypatch, True, False, "bf16x2", 32)
    old = _run_learn(monkeypatch, False, False, "bf16x2", 32)
    _assert_same_images(new[3], old[3])
    assert all(_planes_differ(img, 2) for img in new[3].values())
    # the third plane of the fused images is that of the CURRENT parameters (a fresh three-plane refresh changes nothing)
    for hs in new[0]._train_handles.values():
        L.check(lib.egx_policy_train_refresh(hs["h"], L.current_stream_ptr()), "egx_policy_train_refresh")
    torch.cuda.synchronize()
    _assert_same_images(um._weight_images(new[0]), new[3])
    try:
        L.check(lib.egx_policy_set_precision(2), "egx_policy_set_precision")
        pol = _new_policy(monkeypatch, True, False, "bf16x2")
        pol._ensure_flat_grads()
        assert pol._flat_optimizer_ready()
        assert pol._train_handle(32) is not None
        third = {k: v.view(-1, 3, 64 * 16)[:, 2].clone() for k, v in um._weight_images(pol).items()}
        pol.learn(uh._batch(), 32, 1)
        torch.cuda.synchronize()
        _assert_tail(pol, True)
        after = um._weight_images(pol)
        for key, img in after.items():
            assert torch.equal(img.view(-1, 3, 64 * 16)[:, 2], third[key]), f"third plane of {key} written by a two-plane step"
        ref = _run_learn(monkeypatch, False, False, "bf16x2", 32)
        for key, img in after.items():
            assert torch.equal(img.view(-1, 3, 64 * 16)[:, :2], ref[3][key].view(-1, 3, 64 * 16)[:, :2]), f"planes 0, 1 of {key}"
    finally:
        lib.egx_policy_set_precision(0)


def _guard_flat_buffers(pol):
    """Moves the policy's flat p, m, v between sentinel-filled guards (values kept, parameters and optimiser state re-pointed the
    way _flat_optimizer_ready does it); handles made afterwards are built on the guarded buffers."""
    pol._ensure_flat_grads()
    assert pol._flat_optimizer_ready()
    n = pol._flat_p.numel()
    guards = {k: uh._Guarded(n, pad=256) for k in ("_flat_p", "_flat_m", "_flat_v")}   # 1 KiB: the alignment of the originals' rows
    with torch.no_grad():
        guards["_flat_p"].t.copy_(pol._flat_p)
        for p, off, cnt in pol._flat_layout():
            p.data = guards["_flat_p"].t[off:off + cnt].view_as(p)
    for k, gd in guards.items():
        setattr(pol, k, gd.t)
    pol._graph_cache.clear()
    pol._drop_train_handles()
    assert pol._flat_optimizer_ready()   # adopts the moments into the guarded buffers
    assert pol.optim.state[next(iter(pol.parameters()))]["exp_avg"].data_ptr() == guards["_flat_m"].t.data_ptr()
    return guards


_IMAGES = ([("x_enc_w_ih", 1536, 402), ("x_enc_w_hh", 1536, 512), ("ego_enc_w_ih", 1536, 32), ("ego_enc_w_hh", 1536, 512),
            ("actor_out_w", 256, 1152), ("critic_out_w", 1, 1152)])


def _image_extents(pk):
    """(address, bytes) of the row-major weight images `egx_policy_train_packed` names; a transposed image has no name there and
    follows its row-major one in the arena (layout(), csrc/update3.hip)."""
    ext = [(int(getattr(pk, name)), um._image_bytes(rows, red)) for name, rows, red in _IMAGES]
    ext += [(int(pk.actor_w[l]), um._image_bytes(1152, 1152)) for l in range(4)]
    ext += [(int(pk.critic_w[l]), um._image_bytes(1152, 1152)) for l in range(4)]
    return ext


def test_guard_regions_stay_untouched(monkeypatch):
    """Two optimiser steps on a random gradient, the chain never run: p, m and v lie between sentinel guards, and the handle's
    arena from its first byte (the first weight image) to 64 KiB behind its last weight image is filled with a sentinel byte
    first.  Afterwards the guards are whole, p, m, v are those of the two launches, the named images are theirs - and every
    arena byte the two launches leave alone (the activation buffers between and behind the images) still holds the sentinel."""
    g = torch.Generator().manual_seed(29)
    pols, arenas = {}, {}
    for fused in (True, False):
        pol = _new_policy(monkeypatch, fused, False, "bf16x2")
        guards = _guard_flat_buffers(pol) if fused else None
        pol._ensure_flat_grads()
        assert pol._flat_optimizer_ready()
        hs = pol._train_handle(32)
        assert hs is not None and hs["fused_tail"] == fused
        n = pol._flat_p.numel()
        if "grad" not in pols:
            pols["grad"] = (torch.randn(n, generator=g) * 0.01).cuda()
            pols["m"], pols["v"] = (torch.randn(n, generator=g) * 0.01).cuda(), (torch.rand(n, generator=g) * 1e-4).cuda()
        pol._flat_grad.copy_(pols["grad"]); pol._flat_m.copy_(pols["m"]); pol._flat_v.copy_(pols["v"])
        ext = _image_extents(hs["packed"])
        lo = min(p for p, _ in ext)
        hi = max(p + b for p, b in ext) + um._image_bytes(1152, 1) + 65536   # + the last image's transpose, + 64 KiB
        assert lo == int(hs["packed"].x_enc_w_ih)   # the arena's first buffer
        arena = torch.as_tensor(um._DeviceBytes(lo, hi - lo), device="cuda")
        arena.fill_(0x5A)
        torch.cuda.synchronize()
        for _ in range(2):
            pol._clip_and_step(n=32)
        torch.cuda.synchronize()
        if guards:
            for k, gd in guards.items():
                gd.check(k)
        pols[fused], arenas[fused] = pol, arena.clone()
    for name in ("_flat_p", "_flat_m", "_flat_v"):
        assert torch.equal(getattr(pols[True], name), getattr(pols[False], name)), name
    assert float(pols[True]._step_t) == float(pols[False]._step_t) == 2.0
    # same arena layout in both handles: byte for byte the same, images written and everything else still the sentinel
    assert torch.equal(arenas[True], arenas[False])
    written = arenas[True] != 0x5A
    assert bool(written.any()) and not bool(written[-65536:].any())
    first = um._image_bytes(1536, 402)
    assert bool(written[:first].view(-1, 64 * 16).any(1).all()), "a lane row of the first image was left unwritten"


def test_a_second_live_handle_has_fresh_images_after_a_fused_step(monkeypatch):
    """12 x 24 = 288 rows at minibatch 64: three replays through the 64-row handle, then the merged 96-row rest through a handle of
    its own size, created in mid-epoch - its step is fused too, and the 64-row handle's images follow it by a refresh of their own."""
    new = _run_learn(monkeypatch, True, True, "bf16x2", 64, n_steps=12)
    old = _run_learn(monkeypatch, False, True, "bf16x2", 64, n_steps=12)
    assert new[0].update_paths == {"chain+graph": 3, "chain": 1} and set(new[0]._train_handles) == {64, 96}
    uh._assert_same_training(new[:3], old[:3])
    _assert_same_images(new[3], old[3], count=28)
    for name in um._weight_images(new[0]):   # both handles hold the images of the same, final parameters
        if name[0] == 64:
            assert torch.equal(new[3][name], new[3][(96, name[1])]), name


def test_a_table_that_breaks_the_ownership_rule_falls_back_and_says_so(monkeypatch):
    """Bound to a buffer that ends inside the last weight matrix, and to one that starts behind the first, a handle keeps the
    two-launch tail, egx_last_error() says why, and its optimiser steps still train like every other's."""
    from egogen_amd import _lib as L
    lib = _lib()
    pol = _new_policy(monkeypatch, True, False, "bf16x2")
    pol._ensure_flat_grads()
    assert pol._flat_optimizer_ready()
    hs = pol._train_handle(32)
    assert hs["fused_tail"]
    n = pol._flat_p.numel()
    cut = max(off for p, off, _ in pol._flat_layout() if p.dim() == 2) + 1   # one element into the last weight matrix
    first = min(off for p, off, _ in pol._flat_layout() if p.dim() == 2) + 1   # one element behind the first one's start
    for ptr, cnt in ((L.ptr(pol._flat_p), cut), (pol._flat_p.data_ptr() + 4 * first, n - first)):
        L.check(lib.egx_policy_train_bind_flat(hs["h"], ptr, cnt), "egx_policy_train_bind_flat")
        assert lib.egx_policy_train_fused_tail(hs["h"]) == 0
        why = lib.egx_last_error().decode()
        assert "two-launch tail" in why and "does not lie wholly inside the flat parameter buffer" in why, why
    # the C entry itself falls back for this handle: the same training as the two launches
    grads = []
    pol._after_minibatch = lambda i: grads.append(pol._flat_grad.clone())
    stats = pol.learn(uh._batch(), 32, 1)
    torch.cuda.synchronize()
    old = _run_learn(monkeypatch, False, False, "bf16x2", 32)
    uh._assert_same_training((pol, stats, grads), old[:3])
    _assert_same_images(um._weight_images(pol), old[3])
    # ... and bound to the right buffer again it fuses again
    L.check(lib.egx_policy_train_bind_flat(hs["h"], L.ptr(pol._flat_p), n), "egx_policy_train_bind_flat")
    assert lib.egx_policy_train_fused_tail(hs["h"]) == 1


def test_two_entries_on_the_same_matrix_fall_back(monkeypatch):
    """A weights description in which two layers of the critic name the same matrix: the table's entries overlap, so an element
    would be updated twice - the handle keeps the two-launch tail and egx_last_error() names the overlap.  (The table is built
    inside egx_policy_train_create from whole matrices only, so a transposed or strided entry cannot be made from outside.)"""
    lib = _lib()
    pol = _new_policy(monkeypatch, True, False, "bf16x2")
    pol._ensure_flat_grads()
    assert pol._flat_optimizer_ready()
    w = pol._runner._weights()
    aliased = type(w).from_buffer_copy(w)
    aliased.critic_w[1] = aliased.critic_w[0]
    monkeypatch.setattr(pol._runner, "_weights", lambda: aliased)
    hs = pol._train_handle(32)
    assert hs is not None and not hs["fused_tail"] and lib.egx_policy_train_fused_tail(hs["h"]) == 0
    why = lib.egx_last_error().decode()
    assert "two-launch tail" in why and "overlap" in why, why
