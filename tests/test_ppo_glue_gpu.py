"""The small kernels around the PPO update and the collector (csrc/ppo.hip, tail of csrc/nets.hip), called through the C ABI and
held to the float64 references of tests/ppo_glue_ref.py at their edges and ragged sizes.

Three kinds of bound, none taken from what a kernel returned:
  exact         torch.equal where a kernel moves data or does one IEEE operation per element;
  one rounding  |got - ref64| <= ulp(ref64) where it accumulates in double and rounds once;
  yardstick     per output group 3 * max|ref32 - ref64| + 2^-23 * max|ref64|, ref32 the same reference in fp32 on the CPU; sums
                that meet through trees and atomics: k * 2^-24 * sum|terms|, k stated where it is used.
Every launch gets valid arguments (fresh contiguous allocations, indices in range, sizes that pass the entry point's checks);
output buffers carry sentinel rows past the end that must come back untouched.  With EGX_GLUE_TABLE=<file> the per-group table
(kernel's error next to the fp32 reference's) is appended to that file: profiles/ppo_glue_float64.md.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import ppo_glue_ref as pg

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
SENT = -77.25


@pytest.fixture(scope="module")
def L():
    from egogen_amd import _lib
    _lib.load()
    return _lib


def _dev(*ts):
    """Device copies that the caller keeps alive until the launch has run (a temporary's block may be handed out again)."""
    out = tuple(None if t is None else t.detach().clone().contiguous().cuda() for t in ts)
    return out if len(out) > 1 else out[0]


def _padded(rows, *tail, dtype=F32, extra=2):
    """A sentinel-filled device tensor with `extra` rows more than the kernel may write."""
    return torch.full((rows + extra,) + tuple(tail), SENT, dtype=dtype, device="cuda")


def _untouched(t, rows):
    return bool((t[rows:] == SENT).all())


def _call(L, name, *args):
    L.check(getattr(L.load(), name)(*args, L.current_stream_ptr()), name)
    torch.cuda.synchronize()


def _hold(title, rows):
    """Print / record the table, then hold every row (group, max|f64|, err32, bound, kernel's error) to its bound."""
    pg.emit(pg.table(title, rows))
    for g, _, _, bound, err in rows:
        assert err <= bound, (title, g, err, bound)


def _group_rows(grp, err, label=None):
    return [(f"{label or grp.name} {g}", grp.scale[g], grp.err32[g], grp.bound(g), e) for g, e in err.items()]


# ---------------------------------------------------------------------------------------------------------------------------
# egx_ppo_loss / egx_ppo_loss_packed
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale_kind", ["1/n", "0.37"])
@pytest.mark.parametrize("with_stats", [True, False])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 9, 2053])
def test_ppo_loss(L, n, with_stats, scale_kind):
    """Rows 1 (one working wave, three idle ones feed the block sum), 3, 4, 5 (a second block), 9, 2053 (the 256-block cap: rows
    from 2048 on come from the second grid-stride pass) of the builder's master, through both entry points.

    g_mu, g_logvar, g_value: yardstick over the master's rows.  The six sums: the derived bound of pg.loss_term_bounds - per row
    the first-order error of the row's own term (7 additions deep over the 128 dimensions on elements of up to 7 roundings, expf
    at 2 ulp), across rows k = passes + 2 + blocks + 2 additions (grid-stride accumulation, block sum, one atomic per block,
    scale product and the term's rounding)."""
    scale = float(np.float32(1.0 / n if scale_kind == "1/n" else 0.37))
    part, grp, t64, t32, tb = pg.loss_case(n, with_stats, scale)
    mu, logvar, value, act, adv, ret, lpo = _dev(*part)
    stats = torch.tensor(pg.LOSS_STATS, device="cuda") if with_stats else None
    sc = torch.tensor([scale], device="cuda")
    consts = [C.c_float(x) for x in (pg.ADV_EPS, pg.MIN_LV, pg.MAX_LV, pg.EPS_CLIP, pg.VF_COEF, pg.ENT_COEF)]
    p = L.ptr
    g_mu, g_lv, g_v, terms = _padded(n, 128), _padded(n, 128), _padded(n, extra=8), torch.full((8,), SENT, device="cuda")
    _call(L, "egx_ppo_loss", p(mu), p(logvar), p(value), p(act), p(adv), p(ret), p(lpo), p(stats), p(sc), *consts, n,
          p(g_mu), p(g_lv), p(g_v), p(terms))
    zp = torch.cat([mu, logvar], 1).contiguous()
    g_zp, g_v2, terms2 = _padded(n, 256), _padded(n, extra=8), torch.full((8,), SENT, device="cuda")
    _call(L, "egx_ppo_loss_packed", p(zp), p(value), p(act), p(adv), p(ret), p(lpo), p(stats), p(sc), *consts, n,
          p(g_zp), p(g_v2), p(terms2))
    for buf in (g_mu, g_lv, g_v, g_zp, g_v2):
        assert _untouched(buf, n)
    assert _untouched(terms, 6) and _untouched(terms2, 6)
    # the same arithmetic at another pitch: bit for bit
    assert torch.equal(g_zp[:n, :128], g_mu[:n]) and torch.equal(g_zp[:n, 128:], g_lv[:n]) and torch.equal(g_v2[:n], g_v[:n])
    got = {"g_mu": g_mu[:n], "g_logvar": g_lv[:n], "g_value": g_v[:n]}
    for t in got.values():
        assert torch.isfinite(t).all()
    rows = _group_rows(grp, grp.error(got, pick=lambda g, ref: ref[:n]), f"loss n={n} stats={int(with_stats)} scale={scale_kind}")
    for name, tt in (("terms", terms), ("packed", terms2)):
        tt = tt[:6].cpu().double()
        for j, k in enumerate(pg.TERMS):
            rows.append((f"  {name} {k}", abs(float(t64[j])), abs(float(t32[j] - t64[j])), tb[k], abs(float(tt[j] - t64[j]))))
    _hold(f"egx_ppo_loss / _packed, {n} rows, adv_stats {'given' if with_stats else 'NULL'}, scale {scale_kind}", rows)
    # what the branches must do, independent of any tolerance: blocked gradients are exact zeros
    m = pg.loss_master()
    for r in range(min(n, 45)):
        c = pg.lv_edge_columns(r)
        assert float(g_lv[r, c[2]]) == 0.0 and float(g_lv[r, c[3]]) == 0.0 and float(g_lv[r, c[0]]) != 0.0 and float(g_lv[r, c[1]]) != 0.0
        t_, s_ = float(m["target"][r]), float(m["sign"][r])
        blocked = (t_ == 2.0 and s_ > 0) or (t_ == 0.5 and s_ < 0) or s_ == 0
        assert bool((g_mu[r] == 0).all()) == blocked, (r, t_, s_)


# ---------------------------------------------------------------------------------------------------------------------------
# egx_gru_pointwise / egx_gru_pointwise_bwd
# ---------------------------------------------------------------------------------------------------------------------------
GRU_CASES = [(1, 1), (3, 5), (7, 128), (33, 256)]


def _gru_forward(L, gi, gh, hp, M, H):
    """h_prev and h_out as column blocks (offset 4, pitch > H) of sentinel-filled wider buffers, of which nothing outside the
    block may change; returns h."""
    ld = (H + 3) // 4 * 4 + 8
    off = 4
    out = torch.full((M, ld), SENT, device="cuda")
    mask = torch.zeros(M, ld, dtype=torch.bool, device="cuda")
    mask[:, off:off + H] = True
    hp_ptr = None
    if hp is not None:
        prev = torch.full((M, ld), SENT, device="cuda")
        prev[:, off:off + H] = hp
        hp_ptr = C.c_void_p(prev.data_ptr() + 4 * off)
    _call(L, "egx_gru_pointwise", L.ptr(gi), L.ptr(gh), hp_ptr, ld, C.c_void_p(out.data_ptr() + 4 * off), ld, M, H)
    if hp is not None:
        assert bool((prev[~mask] == SENT).all()) and torch.equal(prev[:, off:off + H], hp)
    assert bool((out[~mask] == SENT).all())
    return out[:, off:off + H].contiguous()


@pytest.mark.parametrize("M,H", GRU_CASES)
def test_gru_pointwise_forward(L, M, H):
    fwd, _, _ = pg.gru_groups()
    gi, gh, hp, _ = (pg.gru_block(t, M, H) for t in pg.gru_master())
    gic, ghc, hpc = _dev(gi, gh, hp)
    got = {"h": _gru_forward(L, gic, ghc, hpc, M, H), "h_noprev": _gru_forward(L, gic, ghc, None, M, H)}
    _hold(f"egx_gru_pointwise M={M} H={H}", _group_rows(fwd, fwd.error(got, pick=lambda g, ref: ref[:M, :H])))


@pytest.mark.parametrize("M,H", GRU_CASES)
def test_gru_pointwise_backward(L, M, H):
    _, bwd, bwd0 = pg.gru_groups()
    gi, gh, hp, dh = _dev(*(pg.gru_block(t, M, H) for t in pg.gru_master()))
    p = L.ptr
    pick = lambda g, ref: (ref[:M, :, :H].reshape(M, 3 * H) if ref.dim() == 3 else ref[:M, :H])
    rows = []
    for grp, hprev, want_dhp in ((bwd, hp, True), (bwd, hp, False), (bwd0, None, False)):
        dgi, dgh, dhp = _padded(M, 3 * H), _padded(M, 3 * H), _padded(M, H)
        _call(L, "egx_gru_pointwise_bwd", p(gi), p(gh), p(hprev), p(dh), M, H, p(dgi), p(dgh), p(dhp) if want_dhp else None)
        assert _untouched(dgi, M) and _untouched(dgh, M) and _untouched(dhp, M if want_dhp else 0)
        got = {"dgi": dgi[:M], "dgh": dgh[:M]}
        if want_dhp:
            got["dh_prev"] = dhp[:M]
        rows += _group_rows(grp, grp.error(got, pick=pick), f"{grp.name}{'' if want_dhp else ' dh_prev=NULL'}")
    _hold(f"egx_gru_pointwise_bwd M={M} H={H}", rows)


def test_gru_pointwise_saturated(L):
    """Pre-activations of +-90 / +-45: expf overflows to inf inside the sigmoid, the results stay finite and equal the float64
    ones to the yardstick (whose fp32 part is zero here: the bound is one ulp of the largest value)."""
    gi, gh, hp, dh = pg.gru_saturated()
    M, H = hp.shape
    gic, ghc, hpc, dhc = _dev(gi, gh, hp, dh)
    fwd = pg.Group("gru saturated", lambda a, b, c: {"h": pg.gru_gates(a, b, c)}, (gi, gh, hp))
    bwd = pg.Group("gru saturated bwd", pg.gru_gates_bwd, (gi, gh, hp, dh))
    h = _gru_forward(L, gic, ghc, hpc, M, H)
    dgi, dgh, dhp = _padded(M, 3 * H), _padded(M, 3 * H), _padded(M, H)
    _call(L, "egx_gru_pointwise_bwd", L.ptr(gic), L.ptr(ghc), L.ptr(hpc), L.ptr(dhc), M, H, L.ptr(dgi), L.ptr(dgh), L.ptr(dhp))
    got = {"dgi": dgi[:M], "dgh": dgh[:M], "dh_prev": dhp[:M]}
    for t in (h, *got.values()):
        assert torch.isfinite(t).all()
    _hold("GRU gates at +-90 / +-45", _group_rows(fwd, fwd.error({"h": h})) + _group_rows(bwd, bwd.error(got)))


# ---------------------------------------------------------------------------------------------------------------------------
# egx_act_fwd / egx_act_bwd_colsum
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", [0, 1, 2, 3])
def test_act_fwd(L, act):
    z, res, _ = pg.act_master()
    grp = pg.Group(f"act_fwd act={act}", lambda z_, r_: pg.act_fwd(z_, r_, act), (z, res))
    rows = []
    for m, w in ((1, 4), (3, 12), (50, 72)):
        for with_res in (True, False):
            a, r = _dev(z[:m, :w], res[:m, :w])
            out = torch.full((m, w), SENT, device="cuda")
            _call(L, "egx_act_fwd", L.ptr(a), L.ptr(r) if with_res else None, L.ptr(out) if with_res else None, m, w, act,
                  C.c_float(pg.SLOPE))
            got = {"a": a}
            if with_res:
                got["out"] = out
            else:
                assert bool((out == SENT).all())
            rows += _group_rows(grp, grp.error(got, pick=lambda g, ref: ref[:m, :w]), f"act={act} {m}x{w} res={int(with_res)}")
    _hold(f"egx_act_fwd act={act}", rows)


def test_act_fwd_rejects_a_size_that_is_no_multiple_of_four(L):
    """The float4 kernel needs rows x width % 4 == 0; the entry point refuses anything else before it launches."""
    z = torch.zeros(16, device="cuda")
    lib = L.load()
    for m, w in ((3, 5), (1, 1), (7, 2)):
        assert lib.egx_act_fwd(L.ptr(z), None, None, m, w, 1, C.c_float(0.0), L.current_stream_ptr()) != 0
    assert lib.egx_act_fwd(L.ptr(z), None, None, 4, 4, 7, C.c_float(0.0), L.current_stream_ptr()) != 0     # unknown activation
    torch.cuda.synchronize()
    assert bool((z == 0).all())


ACT_BWD_SHAPES = [(m, w) for w in (1, 63, 64, 65, 130) for m in (1, 33, 97)] + [(1000, 1152)]


@pytest.mark.parametrize("act", [0, 1, 2, 3])
def test_act_bwd_colsum(L, act):
    """g: yardstick over the master (relu and no activation are exact in fp32: one ulp).  db accumulates onto a non-zero value;
    its bound is k * 2^-24 * (|value held| + sum over rows |g|) per column, k = pg.colsum_depth: the rows one thread walks + 3
    (row phases) + the row splits (atomics) + 1 + 3 roundings per element.  At 1000 x 1152 the split count is capped at 512 / 18."""
    z, _, dy = pg.act_master()
    a32 = pg.act_fwd(z, None, act)["a"]       # the saved output the kernel is handed: holds +0.0 and, for leaky relu, -0.0
    assert int((a32 == 0).sum()) > 0 and (act != 3 or int(((a32 == 0) & torch.signbit(a32)).sum()) > 0)
    grp = pg.Group(f"act_bwd act={act}", lambda d_, a_: {"g": pg.act_bwd(d_, a_, act)["g"]}, (dy, a32))
    assert pg.colsum_depth(1000, 1152)[1] == 512 // 18 and pg.colsum_depth(97, 130)[1] == 4
    rows = []
    prefill = 0.5
    for m, w in ACT_BWD_SHAPES:
        dyc, ac = _dev(dy[:m, :w], a32[:m, :w])
        g64 = grp.o64["g"][:m, :w]
        db64 = prefill + g64.sum(0)
        k, _ = pg.colsum_depth(m, w)
        db_bound = k * pg.U * (prefill + g64.abs().sum(0))
        variants = [("", True, True, True), (" g=NULL", False, True, True), (" db=NULL", True, False, True)]
        if act == 0:
            variants.append((" a=NULL", True, True, False))
        for tag, want_g, want_db, give_a in variants:
            g, db = _padded(m, w), torch.full((w + 8,), prefill, device="cuda")
            db[w:] = SENT
            _call(L, "egx_act_bwd_colsum", L.ptr(dyc), L.ptr(ac) if give_a else None, L.ptr(g) if want_g else None,
                  L.ptr(db) if want_db else None, m, w, act, C.c_float(pg.SLOPE))
            assert _untouched(g, m if want_g else 0) and _untouched(db, w)
            label = f"act={act} {m}x{w}{tag}"
            if want_g:
                rows += _group_rows(grp, grp.error({"g": g[:m]}, pick=lambda _, ref: ref[:m, :w]), label)
            if want_db:
                excess = ((db[:w].cpu().double() - db64).abs() - db_bound)
                j = int(excess.argmax())
                rows.append((label + " db", float(db64.abs().max()), None, float(db_bound[j]), float((db[j].cpu().double() - db64[j]).abs())))
            else:
                assert bool((db[:w] == prefill).all())
    _hold(f"egx_act_bwd_colsum act={act}", rows)
    if act in (2, 3):     # at a saved output of +-0.0: relu passes nothing, leaky relu passes slope * dy - exactly
        m, w = 33, 65
        dyc, ac = _dev(dy[:m, :w], a32[:m, :w])
        g = _padded(m, w)
        _call(L, "egx_act_bwd_colsum", L.ptr(dyc), L.ptr(ac), L.ptr(g), None, m, w, act, C.c_float(pg.SLOPE))
        zero = ac == 0
        want = torch.zeros_like(dyc) if act == 2 else dyc * np.float32(pg.SLOPE)
        assert int(zero.sum()) >= 2 * m and torch.equal(g[:m][zero], want[zero])


# ---------------------------------------------------------------------------------------------------------------------------
# egx_gather_rows
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 77])
@pytest.mark.parametrize("widths", [(804,), (1, 64, 257), (804, 64, 1, 1, 128, 257, 1, 1)])
def test_gather_rows(L, widths, n):
    """Pure data movement: exact.  Indices stay inside [0, N) - the kernel does not clamp - and include the first and the last
    source row and repeats; the column loop repeats above 256 columns (257, 804)."""
    N = 300
    g = torch.Generator().manual_seed(n)
    srcs = [torch.randn(N, w, generator=g).cuda() for w in widths]
    idx = torch.randint(0, N, (n,), generator=g)
    if n > 1:
        idx[:5] = torch.tensor([N - 1, 0, 7, 7, N - 1])
    else:
        idx[0] = N - 1
    assert int(idx.min()) >= 0 and int(idx.max()) < N
    idx = idx.cuda()
    dsts = [_padded(n, w, extra=3) for w in widths]
    k = len(widths)
    sp = (C.c_void_p * k)(*[s.data_ptr() for s in srcs])
    dp = (C.c_void_p * k)(*[d.data_ptr() for d in dsts])
    wp = (C.c_int * k)(*widths)
    keep = [s.clone() for s in srcs]
    _call(L, "egx_gather_rows", L.ptr(idx), n, k, sp, wp, dp)
    for s, s0, d in zip(srcs, keep, dsts):
        assert torch.equal(d[:n], s.index_select(0, idx)) and _untouched(d, n) and torch.equal(s, s0)


# ---------------------------------------------------------------------------------------------------------------------------
# egx_adv_stats
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 255, 256, 257, 1000])
@pytest.mark.parametrize("kind", ["spread", "offset"])
def test_adv_stats(L, n, kind):
    """Double accumulation, one rounding: |got - ref64| <= ulp(ref64).  'offset': 1e4 + small noise, where a one-pass variance
    (or an fp32 mean) cancels to nothing."""
    g = torch.Generator().manual_seed(n)
    adv = torch.randn(n, generator=g) * 3 + 0.7 if kind == "spread" else 1e4 + torch.randn(n, generator=g) * 1e-2
    out = torch.full((4,), SENT, device="cuda")
    advc = _dev(adv)
    _call(L, "egx_adv_stats", L.ptr(advc), n, L.ptr(out))
    ref = pg.adv_stats_ref(adv.double())
    err = (out[:2].cpu().double() - ref).abs()
    bound = pg.ulp32(ref)
    _hold(f"egx_adv_stats n={n} {kind}", [(f"adv_stats n={n} {kind} {k}", abs(float(ref[j])), None, float(bound[j]), float(err[j]))
                                          for j, k in enumerate(("mean", "std"))])
    assert _untouched(out, 2)


def test_adv_stats_of_one_value_has_no_std(L):
    adv = torch.tensor([1.5], device="cuda")
    out = torch.full((4,), SENT, device="cuda")
    _call(L, "egx_adv_stats", L.ptr(adv), 1, L.ptr(out))
    assert float(out[0]) == 1.5 and bool(torch.isnan(out[1])) and bool(torch.isnan(pg.adv_stats_ref(torch.tensor([1.5]))[1]))


# ---------------------------------------------------------------------------------------------------------------------------
# egx_track_episode / egx_rollout_store
# ---------------------------------------------------------------------------------------------------------------------------
def _episode_inputs(A, mode, seed):
    g = torch.Generator().manual_seed(seed)
    rew = torch.randn(A, generator=g)
    term = {"some": (torch.rand(A, generator=g) < 0.3), "none": torch.zeros(A, dtype=torch.bool),
            "all": torch.ones(A, dtype=torch.bool)}[mode].to(torch.int32)
    return rew, term


@pytest.mark.parametrize("mode", ["some", "none", "all"])
@pytest.mark.parametrize("A", [1, 255, 256, 257, 600])
def test_track_episode(L, A, mode):
    """Two calls on the same done_sums (they accumulate).  Per agent: one IEEE addition, exact.  The three sums: k * 2^-24 *
    sum|terms|, k = per call the agents one thread walks (A > 256: the strided loop) + 8 (tree over 256 threads) + 1."""
    g = torch.Generator().manual_seed(A)
    ep_ret, ep_len = torch.randn(A, generator=g), torch.randint(0, 9, (A,), generator=g).float()
    done = torch.tensor([1.0, 2.0, 3.0], dtype=F64)
    er, el, dn = _padded(A), _padded(A), torch.full((8,), SENT, device="cuda")
    er[:A], el[:A], dn[:3] = ep_ret, ep_len, done.float()
    mag = done.abs()
    for call in range(2):
        rew, term = _episode_inputs(A, mode, 10 * A + call)
        rew_c, term_c = _dev(rew, term)
        _call(L, "egx_track_episode", L.ptr(rew_c), L.ptr(term_c), A, L.ptr(er), L.ptr(el), L.ptr(dn))
        ep_ret, ep_len, s_, m_ = pg.track_episode_ref(rew, term, ep_ret, ep_len)
        done, mag = done + s_, mag + m_
        assert torch.equal(er[:A].cpu(), ep_ret) and torch.equal(el[:A].cpu(), ep_len)
    assert _untouched(er, A) and _untouched(el, A) and _untouched(dn, 3)
    if mode != "some":
        assert float(done[2]) == 3.0 + (2 * A if mode == "all" else 0)
    k = pg.done_sums_depth(A, calls=2)
    err = (dn[:3].cpu().double() - done).abs()
    _hold(f"egx_track_episode A={A} {mode}", [(f"track A={A} {mode} {name}", abs(float(done[j])), None, k * pg.U * float(mag[j]), float(err[j]))
                                              for j, name in enumerate(("ret", "len", "count"))])
    assert float(dn[1]) == float(done[1]) and float(dn[2]) == float(done[2])      # lengths and counts are small integers: exact


def _store_inputs(A, seed):
    g = torch.Generator().manual_seed(seed)
    obs = [torch.randn(A, 804, generator=g), torch.randn(A, 64, generator=g), torch.rand(A, generator=g), torch.rand(A, generator=g)]
    rew, term = _episode_inputs(A, "some", seed + 1)
    term[0] = 1                 # some episode ends, whatever the draw
    if A > 1:
        term[1] = 0
    return obs, rew, term


@pytest.mark.parametrize("A", [1, 5, 257])
def test_rollout_store(L, A):
    """The next observation goes to slot t + 1, reward and termination flag to slot t, nothing else moves (all exact), and the
    extra workgroup's bookkeeping is bit-identical to egx_track_episode on the same inputs - the sums included: the two kernels
    walk the agents and the tree in the same order."""
    p = L.ptr
    obs, rew, term = _store_inputs(A, 40 + A)
    obs_c, rew_c, term_c = [o.cuda() for o in obs], rew.cuda(), term.cuda()
    slots = 3
    mk = lambda *tail, dtype=F32: torch.full((slots, A) + tail, SENT, dtype=dtype, device="cuda")
    S, E, D, T, Rw = mk(804), mk(64), mk(), mk(), mk()
    Tm = torch.full((slots, A), -7, dtype=torch.int32, device="cuda")
    g = torch.Generator().manual_seed(A)
    ep_ret0, ep_len0 = torch.randn(A, generator=g).cuda(), torch.randint(0, 9, (A,), generator=g).float().cuda()
    done0 = torch.tensor([1.0, 2.0, 3.0, SENT], device="cuda")
    # the first observation of a collect: slot 0, no reward / termination / bookkeeping
    er, el, dn = ep_ret0.clone(), ep_len0.clone(), done0.clone()
    _call(L, "egx_rollout_store", p(obs_c[0]), p(obs_c[1]), p(obs_c[2]), p(obs_c[3]), None, None, A, p(S[0]), p(E[0]), p(D[0]), p(T[0]),
          None, None, None, p(el), p(dn))
    assert torch.equal(S[0], obs_c[0]) and torch.equal(E[0], obs_c[1]) and torch.equal(D[0], obs_c[2]) and torch.equal(T[0], obs_c[3])
    for buf in (S, E, D, T):
        assert bool((buf[1:] == SENT).all())
    assert bool((Rw == SENT).all()) and bool((Tm == -7).all())
    assert torch.equal(er, ep_ret0) and torch.equal(el, ep_len0) and torch.equal(dn, done0)
    # a step: observation -> slot 2, reward / termination -> slot 1, bookkeeping
    obs2, _, _ = _store_inputs(A, 90 + A)
    obs2_c = [o.cuda() for o in obs2]
    _call(L, "egx_rollout_store", p(obs2_c[0]), p(obs2_c[1]), p(obs2_c[2]), p(obs2_c[3]), p(rew_c), p(term_c), A, p(S[2]), p(E[2]), p(D[2]),
          p(T[2]), p(Rw[1]), p(Tm[1]), p(er), p(el), p(dn))
    assert torch.equal(S[2], obs2_c[0]) and torch.equal(E[2], obs2_c[1]) and torch.equal(D[2], obs2_c[2]) and torch.equal(T[2], obs2_c[3])
    assert torch.equal(S[0], obs_c[0]) and torch.equal(E[0], obs_c[1]) and torch.equal(D[0], obs_c[2]) and torch.equal(T[0], obs_c[3])
    for buf in (S, E, D, T):
        assert bool((buf[1] == SENT).all())
    assert torch.equal(Rw[1], rew_c) and torch.equal(Tm[1], term_c)
    assert bool((Rw[0] == SENT).all()) and bool((Rw[2] == SENT).all()) and bool((Tm[0] == -7).all()) and bool((Tm[2] == -7).all())
    # against egx_track_episode, and the reference
    er2, el2, dn2 = ep_ret0.clone(), ep_len0.clone(), done0.clone()
    _call(L, "egx_track_episode", p(rew_c), p(term_c), A, p(er2), p(el2), p(dn2))
    assert torch.equal(er, er2) and torch.equal(el, el2) and torch.equal(dn, dn2)
    r_, l_, s_, m_ = pg.track_episode_ref(rew, term, ep_ret0.cpu(), ep_len0.cpu())
    assert torch.equal(er.cpu(), r_) and torch.equal(el.cpu(), l_) and float(dn[3]) == SENT
    assert int(term.sum()) > 0
    done = torch.tensor([1.0, 2.0, 3.0], dtype=F64) + s_
    k, mag = pg.done_sums_depth(A), torch.tensor([1.0, 2.0, 3.0], dtype=F64) + m_
    err = (dn[:3].cpu().double() - done).abs()
    _hold(f"egx_rollout_store A={A}", [(f"store A={A} done {name}", abs(float(done[j])), None, k * pg.U * float(mag[j]), float(err[j]))
                                       for j, name in enumerate(("ret", "len", "count"))])


class _Args:
    seed = 0; lr = 3e-4; gamma = 0.99; gae_lambda = 0.95; max_grad_norm = 0.1; vf_coef = 1.0; ent_coef = 0.01
    weight_kld = 0; rew_norm = False; eps_clip = 0.1; value_clip = 0; dual_clip = None; norm_adv = 1; recompute_adv = 0
    deterministic_eval = False; update_graph = False


def test_collector_fused_store_equals_the_copy_path(L, monkeypatch):
    """Two environments and two policies from the same seeds (the policy's exploration noise comes from its own seeded
    generator); one collector runs as it is - and must take the fused egx_rollout_store path -, the other has _fusable turned
    off and goes through copy_ + egx_track_episode.  Everything stored must be bit-identical; the three done sums are held to
    k * 2^-24 * sum|terms| of a float64 replay of the stored rewards, k = 3 steps x (1 + 8 + 1)."""
    from egogen_amd import setup_world as sw
    from egogen_amd.trainer import Collector
    from tests.helpers import build_world
    lib = L.load()
    calls = {"egx_rollout_store": 0, "egx_track_episode": 0}

    def counted(name):
        fn = getattr(lib, name)

        def wrapper(*a):
            calls[name] += 1
            return fn(*a)
        return wrapper
    for name in calls:
        monkeypatch.setattr(lib, name, counted(name), raising=True)
    n, A = 3, 32
    runs = []
    for fused in (True, False):
        w = build_world(V=1024, A=A, scene_kind="box", sdf_res=32, n_pairs=64, n_scenes=4)
        col = Collector(sw.build_policy(_Args()), w["env"])
        if not fused:
            monkeypatch.setattr(col, "_fusable", lambda *a: False)
        before = dict(calls)
        b = col.collect(n)
        torch.cuda.synchronize()
        took = {k: calls[k] - before[k] for k in calls}
        assert took == ({"egx_rollout_store": n + 1, "egx_track_episode": 0} if fused else {"egx_rollout_store": 0, "egx_track_episode": n}), took
        runs.append((col, b))
    (c1, b1), (c2, b2) = runs
    for name in ("state", "ego", "dist", "time", "rew", "term", "act", "logp_old", "values"):
        x, y = getattr(b1, name), getattr(b2, name)
        upto = n if name in ("rew", "term", "act", "logp_old", "values") else n + 1     # values[n] is written by process_fn
        assert torch.equal(x[:upto], y[:upto]), name
    assert float(b1.state[1:].abs().max()) > 0 and float(b1.rew.abs().max()) > 0
    assert torch.equal(c1.ep_ret, c2.ep_ret) and torch.equal(c1.ep_len, c2.ep_len)
    ep_ret, ep_len = torch.zeros(A), torch.zeros(A)
    done, mag = torch.zeros(3, dtype=F64), torch.zeros(3, dtype=F64)
    for t in range(n):
        ep_ret, ep_len, s_, m_ = pg.track_episode_ref(b1.rew[t].cpu(), b1.term[t].cpu(), ep_ret, ep_len)
        done, mag = done + s_, mag + m_
    assert torch.equal(c1.ep_ret.cpu(), ep_ret) and torch.equal(c1.ep_len.cpu(), ep_len)
    k = pg.done_sums_depth(A, calls=n)
    rows = []
    for name, c in (("fused", c1), ("copy path", c2)):
        err = (c._done.cpu().double() - done).abs()
        rows += [(f"collector {name} done {nm}", abs(float(done[j])), None, k * pg.U * float(mag[j]), float(err[j])) for j, nm in enumerate(("ret", "len", "count"))]
    _hold("Collector.collect(3), A = 32, box scenes", rows)
    assert float((c1._done - c2._done).abs().max()) <= 2 * k * pg.U * float(mag.max())


# ---------------------------------------------------------------------------------------------------------------------------
# egx_gae, egx_sample_action, egx_posenc
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gamma,lam", [(0.99, 0.95), (1.0, 1.0)])
@pytest.mark.parametrize("mode", ["some", "none", "all"])
@pytest.mark.parametrize("n,A", [(1, 1), (7, 127), (7, 128), (7, 129), (3, 300)])
def test_gae(L, n, A, mode, gamma, lam):
    """A float64 scan rounded once per output: |got - ref64| <= ulp(ref64) against oracle.ppo.gae_returns."""
    g = torch.Generator().manual_seed(100 * n + A)
    v, rew = torch.randn(n + 1, A, generator=g), torch.randn(n, A, generator=g)
    term = {"some": torch.rand(n, A, generator=g) < 0.2, "none": torch.zeros(n, A, dtype=torch.bool),
            "all": torch.ones(n, A, dtype=torch.bool)}[mode].to(torch.int32)
    ret, adv = _padded(n, A), _padded(n, A)
    vc, rew_c, term_c = _dev(v, rew, term)
    _call(L, "egx_gae", L.ptr(vc), L.ptr(rew_c), L.ptr(term_c), n, A, C.c_double(gamma), C.c_double(lam), L.ptr(ret), L.ptr(adv))
    assert _untouched(ret, n) and _untouched(adv, n)
    ref = pg.gae_ref(v, rew, term, gamma, lam)
    rows = []
    for name, got in (("returns", ret), ("adv", adv)):
        excess = (got[:n].cpu().double() - ref[name]).abs() - pg.ulp32(ref[name])
        j = int(excess.argmax())
        e = (got[:n].cpu().double() - ref[name]).abs().flatten()[j]
        rows.append((f"gae {n}x{A} {mode} g={gamma} {name}", float(ref[name].abs().max()), None, float(pg.ulp32(ref[name]).flatten()[j]), float(e)))
    _hold(f"egx_gae n={n} A={A} {mode} gamma={gamma} lambda={lam}", rows)
    if mode == "all":     # every step ends an episode: adv = rew - v, nothing of the next value
        assert torch.equal(adv[:n].cpu(), (rew.double() - v[:n].double()).float())


@pytest.mark.parametrize("n", [1, 19])
def test_sample_action(L, n):
    """The clamped logvar is exact; act and logp: yardstick over the 19-row master (logp is a tree sum over 128 dimensions - its
    bound comes from what fp32 costs the reference on the same rows, not from a hand-picked tolerance).  logp may be NULL; in the
    deterministic form eps may be NULL and act is mu bit for bit."""
    mu, lv, eps = pg.sample_master()
    grp = pg.Group("sample_action", pg.sample_action_ref, (mu, lv, eps))
    det = pg.Group("sample_action deterministic", lambda m_, l_: pg.sample_action_ref(m_, l_, None), (mu, lv))
    muc, epsc = _dev(mu[:n], eps[:n])
    p = L.ptr
    rows = []
    for want_logp in (True, False):
        lvc, act, logp = _dev(lv[:n]), _padded(n, 128), _padded(n, extra=8)
        _call(L, "egx_sample_action", p(muc), p(lvc), p(epsc), C.c_float(pg.MIN_LV), C.c_float(pg.MAX_LV), 0, n, p(act),
              p(logp) if want_logp else None)
        assert torch.equal(lvc.cpu(), lv[:n].clamp(pg.MIN_LV, pg.MAX_LV)) and _untouched(act, n) and _untouched(logp, n if want_logp else 0)
        got = {"act": act[:n]}
        if want_logp:
            got["logp"] = logp[:n]
        rows += _group_rows(grp, grp.error(got, pick=lambda g, ref: ref[:n]), f"sample n={n} logp={int(want_logp)}")
    lvc, act, logp = _dev(lv[:n]), _padded(n, 128), _padded(n, extra=8)
    _call(L, "egx_sample_action", p(muc), p(lvc), None, C.c_float(pg.MIN_LV), C.c_float(pg.MAX_LV), 1, n, p(act), p(logp))
    assert torch.equal(act[:n], muc) and torch.equal(lvc.cpu(), lv[:n].clamp(pg.MIN_LV, pg.MAX_LV))
    rows += _group_rows(det, det.error({"logp": logp[:n]}, pick=lambda g, ref: ref[:n]), f"sample n={n} deterministic")
    _hold(f"egx_sample_action n={n}", rows)


@pytest.mark.parametrize("A", [1, 3, 129])
def test_posenc(L, A):
    """All 64 columns per input (frequencies 2^0 .. 2^31, sin and cos), on 0, 1, values up to 16 and the environment's ranges."""
    dist, time = pg.posenc_master()
    grp = pg.Group("posenc", pg.posenc_ref, (dist, time))
    out = _padded(A, 128)
    dc, tc = _dev(dist[:A], time[:A])
    _call(L, "egx_posenc", L.ptr(dc), L.ptr(tc), A, L.ptr(out))
    assert _untouched(out, A)
    _hold(f"egx_posenc A={A}", _group_rows(grp, grp.error({"posenc": out[:A]}, pick=lambda g, ref: ref[:A]), f"posenc A={A}"))


# ---------------------------------------------------------------------------------------------------------------------------
# egx_adamw_clip_step / egx_adamw_clip_step_cursor
# ---------------------------------------------------------------------------------------------------------------------------
def _adamw_run(L, p0, grads, n_clip, max_norm, cursor=None, **hp):
    n = p0.numel()
    lib = L.load()
    h = dict(pg.ADAMW, **hp)
    p = torch.full((n + 8,), SENT, device="cuda")
    p[:n] = p0.cuda()
    m, v = torch.full((n + 8,), SENT, device="cuda"), torch.full((n + 8,), SENT, device="cuda")
    m[:n], v[:n] = 0.0, 0.0
    step = torch.zeros(4, device="cuda")
    ws = torch.zeros(int(lib.egx_adamw_workspace_floats()), device="cuda")
    hyper = (C.c_float(max_norm), C.c_double(h["lr"]), C.c_double(h["b1"]), C.c_double(h["b2"]), C.c_double(h["eps"]), C.c_double(h["wd"]))
    for g in grads:
        gc = torch.full((n + 8,), SENT, device="cuda")
        gc[:n] = g.cuda()
        if cursor is None:
            _call(L, "egx_adamw_clip_step", L.ptr(p), L.ptr(gc), L.ptr(m), L.ptr(v), n, n_clip, *hyper, L.ptr(step), L.ptr(ws))
        else:
            _call(L, "egx_adamw_clip_step_cursor", L.ptr(p), L.ptr(gc), L.ptr(m), L.ptr(v), n, n_clip, *hyper, L.ptr(step), L.ptr(ws),
                  L.ptr(cursor))
    for t in (p, m, v):
        assert _untouched(t, n)
    assert bool((step[1:] == 0).all())
    return {"p": p[:n], "m": m[:n], "v": v[:n]}, float(step[0])


@pytest.mark.parametrize("n,n_clip", pg.ADAMW_CASES)
def test_adamw_clip_step(L, n, n_clip):
    """Three steps, the second clipped: p, m, v against the restated clip + AdamW in float64, the yardstick being
    torch.optim.AdamW + clip_grad_norm_ in fp32 on the CPU.  (1, 1) and (3, 0): the tail path alone, no clip; (5, 5): a float4
    and a tail element in the sum of squares; (11, 6): a float4 that straddles n_clip; (1025, 1023): a second block whose only
    float4 is a tail, n_clip % 4 = 3; (4099, 4099): five blocks; 2^20 + 13: the second sweep of the 1024 x 256 x 4 stride."""
    p0, grads, o64, o32, coefs = pg.adamw_case(n, n_clip)
    got, step = _adamw_run(L, p0, grads, n_clip, pg.MAX_NORM)
    assert step == 3.0
    _hold(f"egx_adamw_clip_step n={n} n_clip={n_clip}", pg.yardstick_rows(f"adamw {n}/{n_clip}", o64, o32, got))


def test_adamw_without_clip_and_with_cursor(L):
    """max_norm = 0 switches the clip off (the policy's `if max_grad_norm:`), whatever n_clip; the cursor form does the same
    arithmetic bit for bit and advances the cursor by exactly one per call."""
    n, n_clip = 11, 6
    p0, grads, o64, o32, coefs = pg.adamw_case(n, n_clip, 0.0)
    assert coefs == [1.0, 1.0, 1.0]
    got, step = _adamw_run(L, p0, grads, n_clip, 0.0)
    assert step == 3.0
    _hold("egx_adamw_clip_step max_norm=0", pg.yardstick_rows("adamw 11/6 max_norm=0", o64, o32, got))
    p0, grads, o64, o32, _ = pg.adamw_case(n, n_clip)
    plain, _ = _adamw_run(L, p0, grads, n_clip, pg.MAX_NORM)
    cursor = torch.tensor([5, -7, -7, -7], dtype=torch.int32, device="cuda")
    got, step = _adamw_run(L, p0, grads, n_clip, pg.MAX_NORM, cursor=cursor)
    assert step == 3.0 and cursor.tolist() == [8, -7, -7, -7]
    for k in ("p", "m", "v"):
        assert torch.equal(got[k], plain[k])


@pytest.mark.parametrize("n,n_clip", [(5, 5), (11, 6), (4099, 4099)])
def test_adamw_clip_coefficient(L, n, n_clip):
    """The clip coefficient made visible: with beta1 = 0 and zero state, exp_avg after one step is the clipped gradient itself,
    and g[0] is a power of two, so exp_avg[0] / g[0] IS the coefficient.  Unclipped step: exactly 1.  Clipped step: the norm is
    accumulated in double - one rounding allowed, |coef - coef64| <= ulp(coef64)."""
    g_ = torch.Generator().manual_seed(n)
    p0 = torch.randn(n, generator=g_)
    small = torch.randn(n, generator=g_) * (0.01 / np.sqrt(n_clip))
    small[0] = 2.0 ** -10
    big = torch.randn(n, generator=g_) * (10.0 / np.sqrt(n_clip))
    big[0] = 4.0
    got, _ = _adamw_run(L, p0, [small], n_clip, pg.MAX_NORM, b1=0.0)
    assert float(pg.clip_coef(small.double(), n_clip, pg.MAX_NORM)) == 1.0
    assert torch.equal(got["m"].cpu(), small)
    got, _ = _adamw_run(L, p0, [big], n_clip, pg.MAX_NORM, b1=0.0)
    coef64 = pg.clip_coef(big.double(), n_clip, pg.MAX_NORM)
    assert float(coef64) < 0.1
    coef = got["m"][0].cpu().double() / 4.0
    _hold(f"clip coefficient n={n} n_clip={n_clip}", [(f"adamw {n}/{n_clip} clip coefficient", float(coef64), None, float(pg.ulp32(coef64)),
                                                       float((coef - coef64).abs()))])
    assert torch.equal(got["m"][n_clip:].cpu(), big[n_clip:])      # past the prefix: not clipped
