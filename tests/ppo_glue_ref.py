"""References for the small kernels around the PPO update and the collector (csrc/ppo.hip and the tail of csrc/nets.hip), shared
by test_ppo_glue_ref_cpu.py and test_ppo_glue_gpu.py.

Every function computes in the dtype of the tensors it is given, so one function is both the float64 truth and the float32
yardstick (the rule of tests/precision_yardstick.py): per output group

    bound = R * max|ref32 - ref64| + 2^-23 * max|ref64|          R = 3

Where a kernel maps elements (or rows) independently, the inputs of every shape it is run at are a block of ONE master input, so
the reference is computed once and the yardstick of a group is what fp32 costs over the whole master (`Group`); a one-element case
is then not held to the luck of one rounding of the fp32 reference.  Sums that a kernel combines by trees and atomics are held to
the first-order bound k * 2^-24 * sum|terms| instead, k = the depth of additions that the kernel's code shows.

No GPU needed to import; nothing here is a pytest fixture or setting.
"""
import functools
import math
import os

import numpy as np
import torch

from oracle import ppo as oppo

R = 3.0
ULP = 2.0 ** -23
U = 2.0 ** -24          # unit round-off of fp32
MIN_LV, MAX_LV = -2.5, 2.5
ADV_EPS = float(np.finfo(np.float32).eps)
F32, F64 = torch.float32, torch.float64


def cast(v, dtype):
    if isinstance(v, torch.Tensor):
        return v.detach().to(dtype) if v.is_floating_point() else v
    if isinstance(v, dict):
        return {k: cast(x, dtype) for k, x in v.items()}
    if isinstance(v, (tuple, list)):
        return type(v)(cast(x, dtype) for x in v)
    return v


def f64(out):
    return {k: v.detach().cpu().double() for k, v in out.items()}


def ulp32(x):
    """Spacing of fp32 at |x| (x: float64 tensor): the one-rounding bound of a value formed in double and stored as fp32."""
    a = np.abs(np.asarray(x, np.float64)).astype(np.float32)
    return torch.from_numpy(np.asarray(np.spacing(a), np.float64))


class Group:
    """Reference outputs in float64 and float32 and the yardstick bound per group."""

    def __init__(self, name, fn, inputs):
        """fn(*inputs) -> {group: tensor}, evaluated with the floating-point inputs cast to float64 and to float32.  Where fp32 is
        exact on the inputs (a copy, a ReLU) the fp32 part of the bound is zero and one ulp of the largest value remains."""
        self.name = name
        self.o64 = f64(fn(*cast(tuple(inputs), F64)))
        self.o32 = f64(fn(*cast(tuple(inputs), F32)))
        self.groups = tuple(self.o64)
        self.scale = {g: float(self.o64[g].abs().max()) for g in self.groups}
        self.err32 = {g: float((self.o32[g] - self.o64[g]).abs().max()) for g in self.groups}

    def bound(self, g):
        return R * self.err32[g] + ULP * self.scale[g]

    def error(self, out, pick=None):
        """max|out - ref64| per group of `out`; pick(group, ref64) selects the block of the master that `out` holds."""
        res = {}
        for g, v in f64(out).items():
            ref = self.o64[g] if pick is None else pick(g, self.o64[g])
            assert v.shape == ref.shape, (g, v.shape, ref.shape)
            res[g] = float((v - ref).abs().max()) if v.numel() else 0.0
        return res


def table(title, rows):
    """rows: [(group, max|ref64|, fp32 reference's error or None, bound, kernel's error)] -> lines of text."""
    lines = [f"# {title}", "# group                          max|f64|   |f32-f64|      bound     kernel   kernel/f32  kernel/bound"]
    for g, scale, e32, bound, err in rows:
        e32s, ratio = ("          -", "        -") if not e32 else (f"{e32:11.3e}", f"{err / e32:9.2f}")
        lines.append(f"{g:30s} {scale:10.3e} {e32s} {bound:10.3e} {err:10.3e}    {ratio}     {err / bound if bound else 0.0:8.3f}")
    return lines


def emit(lines, env="EGX_GLUE_TABLE"):
    """Print the table; append it to the file that the environment variable names, if it names one."""
    print("\n".join(lines))
    out = os.environ.get(env)
    if out:
        with open(out, "a") as f:
            f.write("\n".join(lines) + "\n\n")


# ---------------------------------------------------------------------------------------------------------------------------
# egx_ppo_loss / egx_ppo_loss_packed
# ---------------------------------------------------------------------------------------------------------------------------
TERMS = ("loss", "clip", "vf", "ent", "kld", "approx_kl")
TARGET_RATIOS = (0.5, 0.95, 1.0, 1.05, 2.0)
EPS_CLIP, VF_COEF, ENT_COEF = float(np.float32(0.1)), 1.0, float(np.float32(0.01))   # as the kernel receives them (C floats)
LOSS_STATS = (0.25, 1.5)     # (mean, std) handed to the kernel when it normalises; exact in fp32
LV_EDGE_VALUES = (MIN_LV, MAX_LV, -4.0, 3.5)   # both clamp edges (gradient passes) and a value beyond each (gradient 0)


def lv_edge_columns(row):
    """The four columns of `row` that hold LV_EDGE_VALUES: they walk over both halves of the 128 dimensions (the kernel's h = 0, 1)."""
    return [(4 * (row % 32) + j) % 128 for j in range(4)]


def normalised_adv(adv, stats, adv_eps=ADV_EPS):
    return adv if stats is None else (adv - stats[0]) / (stats[1] + adv_eps)


def ppo_loss_ref(mu, logvar, value, act, adv, ret, logp_old, stats, scale, eps_clip=EPS_CLIP, vf_coef=VF_COEF, ent_coef=ENT_COEF):
    """oracle.ppo.ppo_loss on advantages normalised beforehand with the supplied (mean, std), plus approx_kl, differentiated by
    autograd: g_mu, g_logvar (raw, pre-clamp), g_value [n] and the six sums `terms` = scale * sum over rows."""
    n = mu.shape[0]
    mu, logvar, value = (t.detach().clone().requires_grad_(True) for t in (mu, logvar, value))
    A = normalised_adv(adv, stats)
    loss, t = oppo.ppo_loss(mu, logvar, value, act, A, ret, logp_old, eps_clip=eps_clip, vf_coef=vf_coef, ent_coef=ent_coef, norm_adv=False)
    m_, s_ = oppo.action_dist(mu, logvar, MIN_LV, MAX_LV)
    kl = (logp_old - oppo.log_prob(m_, s_, act)).mean()
    k = n * scale        # the oracle takes means, the kernel scale * sum
    (loss * k).backward()
    terms = torch.stack([loss, t["loss/clip"], t["loss/vf"], t["loss/ent"], t["loss/kld"], kl]).detach() * k
    return {"g_mu": mu.grad, "g_logvar": logvar.grad, "g_value": value.grad.reshape(-1), "terms": terms}


def build_loss_inputs(n, seed=0):
    """n rows of fp32 inputs on which every branch of the loss kernel is taken for certain: row r has the probability ratio
    TARGET_RATIOS[r % 5] (logp_old = lp64 - log(target), lp64 the float64 log-probability of the fp32 inputs) and a designed
    advantage that is > 0, < 0, == 0 for (r // 5) % 3 = 0, 1, 2; its raw logvar holds LV_EDGE_VALUES at lv_edge_columns(r).
    `adv` is the designed advantage (for a launch without statistics), `adv_raw` = mean + std * adv in fp32 is what a launch WITH
    LOSS_STATS normalises back to the same sign and to an exact zero.  |lp| is a few hundred, so its fp32 error (~1e-4) cannot move
    a ratio over a clip edge that is 5 % away."""
    g = torch.Generator().manual_seed(seed)
    mu = torch.randn(n, 128, generator=g) * 0.5
    logvar = torch.randn(n, 128, generator=g) * 2.0
    for r in range(n):
        for c, v in zip(lv_edge_columns(r), LV_EDGE_VALUES):
            logvar[r, c] = v
    sigma = torch.exp(logvar.clamp(MIN_LV, MAX_LV)) ** 0.5
    act = mu + 2.0 * sigma * torch.randn(n, 128, generator=g)
    value, ret = torch.randn(n, generator=g), torch.randn(n, generator=g)
    rows = torch.arange(n)
    sign = torch.tensor([1.0, -1.0, 0.0])[(rows // 5) % 3]
    adv = sign * (torch.rand(n, generator=g) * 2.0 + 0.25)
    adv_raw = LOSS_STATS[0] + LOSS_STATS[1] * adv
    m64, s64 = oppo.action_dist(mu.double(), logvar.double(), MIN_LV, MAX_LV)
    lp64 = oppo.log_prob(m64, s64, act.double())
    target = torch.tensor(TARGET_RATIOS, dtype=F64)[rows % 5]
    logp_old = (lp64 - target.log()).float()
    return {"mu": mu, "logvar": logvar, "value": value, "act": act, "adv": adv, "adv_raw": adv_raw, "ret": ret, "logp_old": logp_old,
            "target": target, "sign": sign}


LOSS_ROWS_MASTER = 2053


@functools.lru_cache(maxsize=None)
def loss_master():
    return build_loss_inputs(LOSS_ROWS_MASTER)


@functools.lru_cache(maxsize=None)
def loss_case(n, with_stats, scale):
    """The first n rows of the master run with `scale`: (inputs, Group over ALL master rows with this scale and these statistics -
    g_* of a row do not depend on the other rows -, the float64 terms of the n rows, their derived bounds)."""
    m = loss_master()
    stats = LOSS_STATS if with_stats else None

    def fn(mu, logvar, value, act, adv, ret, logp_old):
        o = ppo_loss_ref(mu, logvar, value, act, adv, ret, logp_old, stats, scale)
        return {k: o[k] for k in ("g_mu", "g_logvar", "g_value")}
    adv = m["adv_raw"] if with_stats else m["adv"]
    full = (m["mu"], m["logvar"], m["value"], m["act"], adv, m["ret"], m["logp_old"])
    grp = Group(f"loss n={n}", fn, full)
    part = tuple(t[:n].contiguous() for t in full)
    t64 = ppo_loss_ref(*cast(part, F64), stats, scale)["terms"]
    t32 = ppo_loss_ref(*cast(part, F32), stats, scale)["terms"].double()
    return part, grp, t64, t32, loss_term_bounds(*cast(part, F64), stats, scale)


def loss_grid(n):
    """(blocks, rows a wave accumulates) of the loss launch: two rows per wave, at most 256 blocks of four waves."""
    blocks = max(1, min(256, -(-n // 8)))
    return blocks, -(-n // (4 * blocks))


def loss_term_bounds(mu, logvar, value, act, adv, ret, logp_old, stats, scale, eps_clip=EPS_CLIP, vf_coef=VF_COEF, ent_coef=ENT_COEF):
    """First-order bounds of the six sums of egx_ppo_loss_kernel, from float64 inputs: sum over rows of the row's own error bound,
    plus k_rows * 2^-24 * scale * sum|row term| for the additions across rows.

    Depth of additions across rows (k_rows): the rows one wave accumulates (grid-stride passes) + 2 (the four waves of a block) +
    the number of blocks (atomics, any order) + 2 (product with scale, rounding of the term itself).
    Within a row: a sum over the 128 dimensions is 1 (two halves per lane) + 6 (wave butterfly) = 7 additions deep on elements
    that cost k_e roundings each; expf is taken at 2 ulp.  lp: k_e = 7 (diff, square, expf = 2, product, two subtractions),
    ent: 3, mu^2: 2 (+ the two constant factors)."""
    n = mu.shape[0]
    lv = logvar.clamp(MIN_LV, MAX_LV)
    z2 = (act - mu) ** 2 * torch.exp(-lv)
    c = 0.5 * math.log(2 * math.pi)
    e_lp = (0.5 * z2 + 0.5 * lv.abs() + c).sum(-1)             # sum of the absolute pieces of lp
    lp = (-0.5 * z2 - 0.5 * lv - c).sum(-1)
    d_lp = (7 + 7) * U * e_lp
    e_ent = (0.5 + c + 0.5 * lv.abs()).sum(-1)
    ent = (0.5 + c + 0.5 * lv).sum(-1)
    d_ent = (3 + 7) * U * e_ent
    kld = 0.5 * (mu ** 2).sum(-1) / 128.0
    d_kld = (2 + 7 + 2) * U * kld
    dv = ret - value
    d_vf = 2 * dv.abs() * U * (ret.abs() + value.abs()) + 2 * U * dv ** 2
    x = lp - logp_old
    ratio = x.exp()
    d_ratio = ratio * (d_lp + U * (lp.abs() + logp_old.abs()) + 3 * U)      # subtraction, expf (2 ulp), one product
    A = normalised_adv(adv, stats)
    d_A = torch.zeros_like(A) if stats is None else 3 * U * (adv.abs() + abs(stats[0])) / (stats[1] + ADV_EPS)
    clip = -torch.min(ratio * A, ratio.clamp(1 - eps_clip, 1 + eps_clip) * A)
    d_clip = A.abs() * d_ratio + torch.max(ratio, torch.full_like(ratio, 1 + eps_clip)) * d_A + 4 * U * clip.abs()
    kl = logp_old - lp
    d_kl = d_lp + U * (lp.abs() + logp_old.abs())
    loss_abs = clip.abs() + vf_coef * dv ** 2 + ent_coef * ent.abs()
    d_loss = d_clip + vf_coef * d_vf + ent_coef * d_ent + 4 * U * loss_abs
    blocks, passes = loss_grid(n)
    k_rows = passes + 2 + blocks + 2
    rows = {"loss": (loss_abs, d_loss), "clip": (clip.abs(), d_clip), "vf": (dv ** 2, d_vf), "ent": (ent.abs(), d_ent),
            "kld": (kld, d_kld), "approx_kl": (kl.abs(), d_kl)}
    return {k: float(abs(scale) * (d.sum() + k_rows * U * a.sum())) for k, (a, d) in rows.items()}


# ---------------------------------------------------------------------------------------------------------------------------
# GRU gates (order r, z, n; gi / gh [M, 3H]) and their backward, by autograd of the plain formula
# ---------------------------------------------------------------------------------------------------------------------------
def gru_gates(gi, gh, h_prev):
    H = gi.shape[-1] // 3
    r = torch.sigmoid(gi[:, :H] + gh[:, :H])
    z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
    n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
    h = (1 - z) * n
    return h if h_prev is None else h + z * h_prev


def gru_gates_bwd(gi, gh, h_prev, dh):
    gi, gh = gi.detach().clone().requires_grad_(True), gh.detach().clone().requires_grad_(True)
    hp = None if h_prev is None else h_prev.detach().clone().requires_grad_(True)
    gru_gates(gi, gh, hp).backward(dh)
    out = {"dgi": gi.grad, "dgh": gh.grad}
    if hp is not None:
        out["dh_prev"] = hp.grad
    return out


GRU_M, GRU_H = 33, 256


@functools.lru_cache(maxsize=None)
def gru_master():
    """gi, gh as [M, 3, H] (a case (m, h) takes [:m, :, :h]), h_prev, dh [M, H]; pre-activations of a few units."""
    g = torch.Generator().manual_seed(11)
    gi, gh = torch.randn(GRU_M, 3, GRU_H, generator=g) * 1.5, torch.randn(GRU_M, 3, GRU_H, generator=g) * 1.5
    hp, dh = torch.randn(GRU_M, GRU_H, generator=g), torch.randn(GRU_M, GRU_H, generator=g)
    return gi, gh, hp, dh


def gru_saturated(m=3, h=5):
    """Pre-activations of +-90 and +-45 in every gate (gh of the r and z gates zero, so the sums are those values): the gates are
    within 3e-20 of 0, 1 and +-1, fp32 and float64 give the same h, expf overflows to inf on the way, and every result must be
    finite."""
    big = torch.tensor([90.0, -90.0, 45.0, -45.0])
    k = torch.arange(m)[:, None, None] + 2 * torch.arange(3)[None, :, None] + torch.arange(h)[None, None, :]
    gi = big[k % 4]
    gh = torch.zeros(m, 3, h)
    gh[:, 2] = big[(k[:, 2] + 1) % 4] / 2
    g = torch.Generator().manual_seed(13)
    return gi.reshape(m, 3 * h), gh.reshape(m, 3 * h), torch.randn(m, h, generator=g), torch.randn(m, h, generator=g)


def gru_block(t, m, h):
    """The (m, h) case of a master tensor: [M, 3, H] -> [m, 3h], [M, H] -> [m, h], contiguous."""
    return (t[:m, :, :h].reshape(m, 3 * h) if t.dim() == 3 else t[:m, :h]).contiguous()


@functools.lru_cache(maxsize=None)
def gru_groups():
    gi, gh, hp, dh = gru_master()
    flat = lambda t: t.reshape(GRU_M, 3 * GRU_H)
    unflat = lambda o: {k: (v.reshape(GRU_M, 3, GRU_H) if v.shape[-1] == 3 * GRU_H else v) for k, v in o.items()}
    fwd = Group("gru fwd", lambda a, b, c: {"h": gru_gates(a, b, c), "h_noprev": gru_gates(a, b, None)}, (flat(gi), flat(gh), hp))
    bwd = Group("gru bwd", lambda a, b, c, d: unflat(gru_gates_bwd(a, b, c, d)), (flat(gi), flat(gh), hp, dh))
    bwd0 = Group("gru bwd h_prev=0", lambda a, b, d: unflat(gru_gates_bwd(a, b, None, d)), (flat(gi), flat(gh), dh))
    return fwd, bwd, bwd0


# ---------------------------------------------------------------------------------------------------------------------------
# activations 0 none, 1 tanh, 2 relu, 3 leaky relu; backward through the SAVED OUTPUT, with column sums
# ---------------------------------------------------------------------------------------------------------------------------
SLOPE = float(np.float32(0.01))   # the slope as the kernel receives it


def act_fwd(z, res, act, slope=SLOPE):
    a = z if act == 0 else torch.tanh(z) if act == 1 else torch.relu(z) if act == 2 else torch.where(z > 0, z, z * slope)
    return {"a": a, "out": a if res is None else a + res}


def act_bwd(dy, a, act, slope=SLOPE):
    """g = dy * act'(a) with the derivative written in the saved output a (at a == +-0: relu 0, leaky relu `slope`, as torch's
    threshold / leaky_relu backward) and db = column sums of g."""
    if act == 0:
        g = dy
    elif act == 1:
        g = dy * (1 - a * a)
    elif act == 2:
        g = dy * (a > 0).to(dy.dtype)
    else:
        g = dy * torch.where(a > 0, torch.ones_like(a), torch.full_like(a, slope))
    return {"g": g, "db": g.sum(0)}


ACT_M, ACT_W = 1000, 1152


@functools.lru_cache(maxsize=None)
def act_master():
    """z, res, dy [1000, 1152]; a case (m, w) takes [:m, :w].  z holds exact 0.0 and -0.0 on two diagonals and down the first
    column (rows 0, 5, .. and 1, 6, ..), so the saved outputs of every activation do, at every width."""
    g = torch.Generator().manual_seed(12)
    z, res, dy = (torch.randn(ACT_M, ACT_W, generator=g) for _ in range(3))
    r = torch.arange(ACT_M)
    z[r, r % ACT_W] = 0.0
    z[r, (r + 1) % ACT_W] = -0.0
    z[0::5, 0] = 0.0
    z[1::5, 0] = -0.0
    return z, res, dy


def colsum_depth(m, w):
    """Depth of additions behind one db entry of egx_act_bwd_colsum: the rows one thread walks + 3 (four row phases) + the row
    splits that meet in db by atomics (one more for the value db held) + 3 roundings of an element (a * a, 1 - ., product)."""
    strips = -(-w // 64)
    splits = max(1, min(-(-m // 32), 512 // strips))
    rpb = -(-m // splits)
    splits = -(-m // rpb)
    return -(-rpb // 4) + 3 + splits + 1 + 3, splits


# ---------------------------------------------------------------------------------------------------------------------------
# GAE, action sampling, positional encoding, advantage statistics, episode bookkeeping
# ---------------------------------------------------------------------------------------------------------------------------
def gae_ref(values, rew, term, gamma, lam):
    """values [n+1, A], rew / term [n, A] (time-major) -> returns, adv [n, A] in float64 by oracle.ppo.gae_returns."""
    n = rew.shape[0]
    v = values.double().numpy()
    tm = term.numpy().astype(bool)
    ret, adv = oppo.gae_returns(v[:n].T, v[1:].T, rew.double().numpy().T, tm.T, np.zeros_like(tm.T), gamma, lam)
    return {"returns": torch.from_numpy(ret.T.copy()), "adv": torch.from_numpy(adv.T.copy())}


def sample_action_ref(mu, logvar, eps):
    """oracle.ppo.action_dist / log_prob: clamped logvar, act = mu + sigma * eps, logp of act."""
    m, s = oppo.action_dist(mu, logvar, MIN_LV, MAX_LV)
    act = m if eps is None else m + s * eps
    return {"logvar": logvar.clamp(MIN_LV, MAX_LV), "act": act, "logp": oppo.log_prob(m, s, act)}


@functools.lru_cache(maxsize=None)
def sample_master():
    """mu, raw logvar, noise [19, 128]; every row holds LV_EDGE_VALUES (exactly +-2.5 and beyond) among logvars of +-3 sigma."""
    g = torch.Generator().manual_seed(14)
    mu, lv, eps = torch.randn(19, 128, generator=g), torch.randn(19, 128, generator=g) * 3, torch.randn(19, 128, generator=g)
    for r in range(19):
        lv[r, lv_edge_columns(r)] = torch.tensor(LV_EDGE_VALUES)
    return mu, lv, eps


@functools.lru_cache(maxsize=None)
def posenc_master():
    """dist, time [129]: 0, 1 and a few values up to 16 first, then the environment's ranges, dist in (0, 1] and time in [0, 1]."""
    g = torch.Generator().manual_seed(15)
    dist, time = 1.0 - torch.rand(129, generator=g), torch.rand(129, generator=g)
    dist[:6] = torch.tensor([0.0, 1.0, 16.0, 2.5, 7.3, 1e-3])
    time[:6] = torch.tensor([1.0, 0.0, 0.5, 16.0, 3.7, 11.1])
    return dist, time


def posenc_ref(dist, time):
    """[A, 128]: per input 32 frequencies 2^k, columns (sin, cos) interleaved.  x * 2^k is formed in fp32 (exact: a power of two
    times an fp32 value, far from overflow) and then taken to sin / cos in the dtype of `dist`."""
    outs = []
    for x in (dist, time):
        f = (x.float()[:, None] * (2.0 ** torch.arange(32, dtype=F32))[None]).to(x.dtype)
        outs.append(torch.stack([torch.sin(f), torch.cos(f)], -1).reshape(x.shape[0], 64))
    return {"posenc": torch.cat(outs, 1)}


def adv_stats_ref(adv):
    """[mean, unbiased std]; a single value has no unbiased std: NaN, as torch.std."""
    n = adv.numel()
    mean = adv.sum() / n
    std = ((adv - mean) ** 2).sum().div(n - 1).sqrt() if n > 1 else torch.tensor(float("nan"), dtype=adv.dtype)
    return torch.stack([mean, std])


def track_episode_ref(rew, term, ep_ret, ep_len):
    """One collector step of the episode bookkeeping: new (ep_ret, ep_len) in fp32 (one IEEE addition per agent, so exact), what
    the step adds to the three sums over the finished episodes (return, length, count) in float64, and the sum of the absolute
    values of those terms."""
    r, l = ep_ret.float() + rew.float(), ep_len.float() + 1.0
    d = term != 0
    zero = torch.zeros_like(r)
    sums = torch.stack([r[d].double().sum(), l[d].double().sum(), d.double().sum()])
    mags = torch.stack([r[d].double().abs().sum(), l[d].double().sum(), d.double().sum()])
    return torch.where(d, zero, r), torch.where(d, zero, l), sums, mags


def done_sums_depth(A, calls=1):
    """Additions behind a done sum: the agents one thread walks + 8 (tree over 256 threads) + 1 (onto the running sum), per call."""
    return calls * (-(-A // 256) + 8 + 1)


# ---------------------------------------------------------------------------------------------------------------------------
# clip_grad_norm_ of a prefix + AdamW on flat tensors
# ---------------------------------------------------------------------------------------------------------------------------
ADAMW = dict(lr=3e-4, b1=0.9, b2=0.999, eps=1e-8, wd=0.01)
MAX_NORM = float(np.float32(0.1))     # as the kernel receives it (a C float)


def clip_coef(g, n_clip, max_norm):
    """torch.nn.utils.clip_grad_norm_ over g[:n_clip]; no clipping for an empty prefix or max_norm <= 0 (the policy's `if
    max_grad_norm:`)."""
    if n_clip == 0 or max_norm <= 0:
        return torch.ones((), dtype=g.dtype)
    return (max_norm / (torch.linalg.vector_norm(g[:n_clip]) + 1e-6)).clamp(max=1.0)


def adamw_clip_step(p, g, m, v, step, n_clip, max_norm, lr, b1, b2, eps, wd):
    """One step of torch.optim.AdamW (decoupled decay, bias corrections) after the clip; returns new (p, m, v, step, coef)."""
    coef = clip_coef(g, n_clip, max_norm)
    g = g.clone()
    g[:n_clip] = g[:n_clip] * coef
    step = step + 1
    p = p * (1 - lr * wd)
    m = m + (1 - b1) * (g - m)
    v = b2 * v + (1 - b2) * g * g
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    denom = v.sqrt() / math.sqrt(bc2) + eps
    p = p - (lr / bc1) * m / denom
    return p, m, v, step, coef


def torch_adamw_steps(p0, grads, n_clip, max_norm, dtype, lr, b1, b2, eps, wd):
    """The same with torch itself: the prefix and the rest as two parameters, clip_grad_norm_ on the first, torch.optim.AdamW."""
    n = p0.numel()
    ps = [torch.nn.Parameter(p0[:n_clip].to(dtype).clone()), torch.nn.Parameter(p0[n_clip:].to(dtype).clone())]
    ps = [q for q in ps if q.numel()]
    opt = torch.optim.AdamW(ps, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    for g in grads:
        g = g.to(dtype)
        parts = [g[:n_clip], g[n_clip:]]
        for q, gq in zip(ps, [x for x in parts if x.numel()]):
            q.grad = gq.clone()
        if n_clip > 0 and max_norm > 0:
            torch.nn.utils.clip_grad_norm_([ps[0]], max_norm)
        opt.step()
    cat = lambda f: torch.cat([f(q) for q in ps]).detach().double()
    assert cat(lambda q: q).numel() == n
    return {"p": cat(lambda q: q), "m": cat(lambda q: opt.state[q]["exp_avg"]), "v": cat(lambda q: opt.state[q]["exp_avg_sq"])}


ADAMW_CASES = ((1, 1), (3, 0), (5, 5), (11, 6), (1025, 1023), (4099, 4099), (2 ** 20 + 13, 2 ** 20 + 7))


@functools.lru_cache(maxsize=None)
def adamw_case(n, n_clip, max_norm=MAX_NORM):
    """Parameters and three gradients (fp32): the norm of the clipped prefix is ~0.01, ~10, ~0.01, so with max_norm = 0.1 the
    second step is clipped and the others are not.  Returns (p0, grads, float64 reference, fp32 torch yardstick, coefficients)."""
    g_ = torch.Generator().manual_seed(1000 + n)
    p0 = torch.randn(n, generator=g_)
    grads = [torch.randn(n, generator=g_) * (s / math.sqrt(max(n_clip, 1))) for s in (0.01, 10.0, 0.01)]
    p, m, v, step = p0.double(), torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64), 0
    coefs = []
    for g in grads:
        p, m, v, step, c = adamw_clip_step(p, g.double(), m, v, step, n_clip, max_norm, **ADAMW)
        coefs.append(float(c))
    o64 = {"p": p, "m": m, "v": v}
    o32 = torch_adamw_steps(p0, grads, n_clip, max_norm, F32, **ADAMW)
    return p0, grads, o64, o32, coefs


def yardstick_rows(name, o64, o32, got):
    """Per group: (label, max|ref64|, max|ref32 - ref64|, bound, max|got - ref64|)."""
    rows = []
    for k in o64:
        scale, e32 = float(o64[k].abs().max()), float((o32[k] - o64[k]).abs().max())
        rows.append((f"{name} {k}", scale, e32, R * e32 + ULP * scale, float((got[k].detach().cpu().double() - o64[k]).abs().max())))
    return rows
