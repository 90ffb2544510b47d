"""TEST INFRASTRUCTURE ONLY -- fp64 model of the matrix row-split kernel's split-f16 arithmetic and its a-priori error bound.

The matrix kernel (csrc/vibo_msplit_kernel.hpp) forms  logit = -a.theta + b,  d LL/d theta = sum_i g a  and
d LL/d a = sum_p g theta  as f16 MFMAs on two-piece operands.  This file restates, from the kernel's comments, WHAT that scheme
computes (it is not a port of the kernel: there is no tiling, no lane layout, no LDS image here), and derives how far the result
may lie from the exact fp64 value of the same expression on the same fp32 inputs.  Everything is numpy float64; an fp32 input
is exactly representable in it, and so is every sum of a few products of f16 pieces.

Scheme (log2 units: the kernel evaluates 2^(+-l2) with l2 = logit log2 e):
  na_k = fl32(-a_k LOG2E32)   (1PL: a == -1, na = LOG2E32 itself)        nb = fl32(b LOG2E32)
  jsh  = -floor(E(max|na|) / 2) clamped to [-14, 12],  E(x) the frexp exponent (x < 2^E) -- the maxima are taken per WORKGROUP,
         i.e. over one panel of at most 1024 consecutive items (PANEL); a launch of up to 1024 items is one panel
  bsh  = max(E(max|nb|) - 15, 0), at most 15 (beyond: the kernel poisons its outputs; not modelled)
  a'   = na 2^jsh,  theta' = theta 2^-jsh,  nb' = nb 2^-bsh                (exact: powers of two)
  x    = hi + lo + residual, hi = rtz16(x), lo = rtz16(x - hi)            (split_rtz; rtz16 = round toward zero onto the f16 grid)
  nb'  = b0 + b1 + b2 + residual                                          (bias_pieces)
  l2   = sum_k (th_hi a_hi + th_lo a_hi + th_hi a_lo) + 2^bsh (b0 + b1 + b2)      -- the lo.lo product is dropped
The products of two f16 values are exact in fp32; the model adds them exactly (fp64) and the BOUND carries the fp32
accumulation as a term of its own (E_acc below).

Error bound of one cell, u = 2^-24 (cell_bound; log2 units, returned in nats = x ln 2):

  E = E_conv + sum_k E_prod,k + E_bias + E_acc

  E_conv  = sum_k |na_k - (-a_k log2 e)| |theta_k| + |nb - b log2 e|: the two fp32 conversions, EVALUATED from the inputs (each is
            at most u of its term; evaluating instead of bounding them is what lets a missing third bias piece show).
  eps(x)  = split residual |x - hi - lo| <= 6u |x| if |x| >= 2^-2, else 2^-24.  An fp32 x has 24 significant bits, hi takes 11,
            lo takes 11 starting at the residual's leading one, which leaves at most the two lowest bits:
            (2^-22 + 2^-23) of the binade's base = 6u |x| at worst.  Once lo falls below the f16 normal range (2^-14) its grid is
            2^-24 ABSOLUTE: for |x| < 2^-2 the residual is bounded by that instead.  (Checked against every mantissa of several
            binades in tests/test_split_model.py.)
  E_prod  = eps(theta') |a'| + eps(a') |theta'| + eps(theta') eps(a') + 2^-20 |theta' a'|
            (|lo| < ulp16(hi) <= 2^-10 |x| under round-toward-zero, so the dropped lo.lo is below 2^-20 of the product).
            With both operands at or above 2^-2 this is c_op |a theta| with c_op = (6 + 6 + 16) u = 28 u; the rest is E_sub:
            2^-24 times the partner operand, which the per-launch scale 2^jsh (set by the LARGEST discrimination) multiplies
            back up for every ordinary item of a panel that holds one outlier.
  E_bias  = 2^bsh (c_b |nb'| + (2^-24 if |nb'| < 1 else 0)),  c_b = 6u 2^-10 = 1.5 2^-32: b2 = rtz16 of a residual that is at most
            eps(nb'); when that residual is subnormal in f16 it is a multiple of ulp32(nb') >= 2^-24 for |nb'| >= 1, hence exact there.
            With bsh > 0 (one difficulty beyond 2^15 in the panel) the 2^-24 becomes 2^(bsh - 24) on every other item.
  E_acc   = (A + 3) u (sum_k |na_k theta_k| + |nb|)  if any product is nonzero, else 0.
            Model: the 3A + 3 exact products are added in fp32 in an order we do not know; the A + 1 terms of full size (hi.hi
            and b0) each cost one rounding of at most u of the running sum, and the 2A + 2 terms a factor 2^-10 smaller are
            given two more roundings between them.  If every product is exactly zero (theta = 0 or a = 0) only the bias pieces
            are added, and every partial sum of pieces of ONE fp32 number is itself an fp32 number: the sum is exact in any
            order and any rounding mode, so E_acc = 0 there -- these are the cells on which a missing b2 stands out.

fp32=True gives the bound of a plain fp32 evaluation (the VALU kernel, the witness): no split terms, no E_sub, conversions
bounded by 2u of each term instead of evaluated (its order of operations is its own business): (A + 5) u (sum|a theta| + |b|).

Gradients.  g = x - sigmoid(l) is evaluated in fp32 from the logit: |dg| <= sigmoid'(l) E + E^2 + C_SIGMA u, C_SIGMA = 6 (one
exp2 at 1 ulp, the rounding of 1 + e, a reciprocal shared between two cells at ~2 ulp, one fma: below 5 ulp of 1, taken as 6).
The difficulty gradient sums g itself in fp32.  The two other contractions split g (unscaled, |g| <= 1: eps(g) <= max(6u|g|, 2^-24))
and take all four piece products:
  d LL/d a_ik     : per cell |theta_k| (dg + eps(g)) + |g| eps(theta'_k) 2^jsh + 4u |g theta_k|
  d LL/d theta_pk : per cell |a_k| (dg + eps(g)) + |g| eps(a'_k) 2^-jsh ln 2 + 4u |g a_k|
summed over the cells that feed an entry, plus (n + 8) u sum|g x| for the fp32 accumulation over n observed cells.

3PL.  p = c + (1 - c) sigmoid(l), c = sigmoid(guess logit).  The logit is the 2PL one (same bound).  Answered right:
g = p'/p = 1/(1 + c E) - 1/(1 + E) with E = e^-l; answered wrong: g = -p'/(1 - p) = -sigmoid(l): differences of two terms in [0, 1],
evaluated from one exp2 and one reciprocal, with c itself from an fp32 expf and a division (a few u of c, at most u of g):
|dg| <= |dg/dl| E + E^2 + C_SIGMA3 u, C_SIGMA3 = 8.  The probability clamp (p outside [eps32, 1 - eps32]: value capped, gradient
zero) flips with the last bits of p: cells whose exact p lies within 4 fp32 ulp of either clamp value are marked `excluded`
by reference() and asserted by nobody; everywhere else the clamp decision is the fp64 one.

Forward only.  ll = log p(x | l) per observed cell, d ll/d l = g:  |d ll| <= |g| E + E^2.  The kernel multiplies the cells'
probabilities four at a time, takes one log2 per product and adds these in fp32: (n / 4 + 20) u sum|ll| for n observed cells
(ll_bound).  Unobserved cells enter the kernel's sum as exact -1s that a count takes back; the forward-only test has none.
"""
import numpy as np

U = 2.0 ** -24
LOG2E = 1.4426950408889634073599246810019          # log2 e
LOG2E32 = float(np.float32(LOG2E))
LN2 = 0.69314718055994530941723212145818
C_SPLIT = 6.0 * U                                   # eps(x) / |x| with both pieces normal
C_LOLO = 2.0 ** -20                                 # dropped lo.lo product / |product|
C_OP = 2.0 * C_SPLIT + C_LOLO                       # 28 u
C_B = C_SPLIT * 2.0 ** -10                          # 1.5 2^-32
C_SIGMA = 6.0
C_SIGMA3 = 8.0
EPS32 = 2.0 ** -23
LOGIT_LO = 15.942384719848633             # -log(eps32 / (1 - eps32))
LOGIT_HI = 16.635532333438686             # 24 ln 2
F16_MAX = 65504.0
DROPS = ('theta_lo*a_hi', 'theta_hi*a_lo', 'b2')


def f32(x):
    return np.asarray(x, dtype=np.float32)


def rtz16(x):
    """Round toward zero onto the f16 grid (subnormals kept, magnitudes above 65 504 saturate there).  x float64."""
    x = np.asarray(x, dtype=np.float64)
    ax = np.abs(x)
    _, e = np.frexp(ax)                              # ax = m 2^e, m in [0.5, 1)
    q = np.exp2(np.maximum(e - 11, -24).astype(np.float64))      # 11 significant bits, grid 2^-24 below 2^-14
    return np.sign(x) * np.minimum(np.floor(ax / q) * q, F16_MAX)


def split_rtz(x):
    """x (an fp32 value) -> (hi, lo), both on the f16 grid: hi = rtz16(x), lo = rtz16(x - hi)."""
    x = np.asarray(x, dtype=np.float64)
    hi = rtz16(x)
    return hi, rtz16(x - hi)


def bias_pieces(nb):
    """nb' -> (b0, b1, b2): split_rtz, then the first piece of the split of what is left."""
    b0, b1 = split_rtz(nb)
    return b0, b1, rtz16(np.asarray(nb, dtype=np.float64) - b0 - b1)


def _frexp_e(x):
    return int(np.frexp(np.float64(x))[1]) if x > 0 else -126


def item_operands(a, b, irt=2):
    """fp32 item parameters -> (na [I, A], nb [I]) as float64 copies of the kernel's fp32 values.  1PL: pass a = -1."""
    a, b = f32(a), f32(b)
    na = (np.full_like(a, np.float32(LOG2E32)) if irt == 1 else (-a) * np.float32(LOG2E32)).astype(np.float64)
    nb = (b * np.float32(LOG2E32)).astype(np.float64)
    return na, nb


PANEL = 1024                                        # items of one workgroup: the scope of the two scales


def launch_scales(a, b, irt=2):
    """-> (jsh, bsh) of ONE panel (workgroup) that holds exactly these items, at most PANEL of them (more: per_panel)."""
    assert np.asarray(b).shape[0] <= PANEL, 'the scales are per panel of 1024 items: use per_panel'
    na, nb = item_operands(a, b, irt)
    e_a, e_b = _frexp_e(np.abs(na).max(initial=0.0)), _frexp_e(np.abs(nb).max(initial=0.0))
    jsh = int(np.clip(-(e_a >> 1), -14, 12))
    bsh = min(max(e_b - 15, 0), 15)
    return jsh, bsh


def scaled_operands(theta, a, b, irt=2, jsh=None, bsh=None):
    na, nb = item_operands(a, b, irt)
    if jsh is None or bsh is None:
        jsh, bsh = launch_scales(a, b, irt)
    return dict(na=na, nb=nb, jsh=jsh, bsh=bsh, a_s=na * 2.0 ** jsh, t_s=np.asarray(f32(theta), np.float64) * 2.0 ** -jsh,
                nb_s=nb * 2.0 ** -bsh)


def per_panel(fn, theta, a, b, *args, **kw):
    """fn(theta, a, b, ...) -> [B, I], evaluated panel by panel (each with its own scales) and concatenated."""
    I = np.asarray(b).shape[0]
    return np.concatenate([fn(theta, np.asarray(a)[lo:lo + PANEL], np.asarray(b)[lo:lo + PANEL], *args, **kw)
                           for lo in range(0, I, PANEL)], axis=1)


def exact_logit(theta, a, b):
    """fp64 value of -a.theta + b on the fp32 inputs, [B, I] (1PL: a = -1)."""
    return -(np.asarray(f32(theta), np.float64) @ np.asarray(f32(a), np.float64).T) + np.asarray(f32(b), np.float64)[None, :]


def logit_model(theta, a, b, irt=2, drop=(), jsh=None, bsh=None):
    """[B, I] logits (nats) of the documented scheme; the fp32 accumulation is modelled as EXACT (cell_bound carries E_acc).
    drop: names from DROPS to leave out."""
    assert all(d in DROPS for d in drop), drop
    o = scaled_operands(theta, a, b, irt, jsh, bsh)
    th, tl = split_rtz(o['t_s'])
    ah, al = split_rtz(o['a_s'])
    l2 = th @ ah.T
    if 'theta_lo*a_hi' not in drop:
        l2 = l2 + tl @ ah.T
    if 'theta_hi*a_lo' not in drop:
        l2 = l2 + th @ al.T
    b0, b1, b2 = bias_pieces(o['nb_s'])
    bias = b0 + b1 + (0.0 if 'b2' in drop else b2)
    return (l2 + (2.0 ** o['bsh']) * bias[None, :]) * LN2


def eps_split(x):
    ax = np.abs(x)
    return np.where(ax >= 0.25, C_SPLIT * ax, np.where(ax > 0, 2.0 ** -24, 0.0))


def sub_share(x):
    """Share of the nonzero scaled operands x whose lo piece lies below the f16 normal range (where eps is absolute)."""
    ax = np.abs(np.asarray(x, dtype=np.float64))
    nz = ax > 0
    return float((ax[nz] < 0.25).mean()) if nz.any() else 0.0


def cell_bound(theta, a, b, irt=2, jsh=None, bsh=None, fp32=False, parts=False):
    """A-priori bound of |kernel logit - exact_logit| per cell, [B, I], nats, from the inputs alone (module docstring)."""
    o = scaled_operands(theta, a, b, irt, jsh, bsh)
    t = np.abs(np.asarray(f32(theta), np.float64))
    A = t.shape[1]
    s_prod = t @ np.abs(o['na']).T                                     # sum_k |na_k theta_k|
    s_all = s_prod + np.abs(o['nb'])[None, :]
    if fp32:
        return (A + 5) * U * s_all * LN2
    a64 = np.asarray(f32(a), np.float64)
    na_exact = np.full_like(a64, LOG2E) if irt == 1 else -a64 * LOG2E
    e_conv = t @ np.abs(o['na'] - na_exact).T + np.abs(o['nb'] - np.asarray(f32(b), np.float64) * LOG2E)[None, :]
    at, aa = np.abs(o['t_s']), np.abs(o['a_s'])
    et, ea = eps_split(o['t_s']), eps_split(o['a_s'])
    e_prod = et @ aa.T + at @ ea.T + et @ ea.T + C_LOLO * (at @ aa.T)
    nbs = np.abs(o['nb_s'])
    e_bias = (2.0 ** o['bsh']) * (C_B * nbs + np.where((nbs < 1.0) & (nbs > 0), 2.0 ** -24, 0.0))[None, :]
    e_acc = np.where(s_prod > 0, (A + 3) * U * s_all, 0.0)
    total = (e_conv + e_prod + e_bias + e_acc) * LN2
    if parts:
        e_sub = (e_prod - C_OP * s_prod + e_bias - (2.0 ** o['bsh']) * C_B * nbs[None, :]) * LN2
        return total, dict(conv=e_conv * LN2, op=C_OP * s_prod * LN2, sub=e_sub, acc=e_acc * LN2, fp32=(A + 5) * U * s_all * LN2)
    return total


def sigmoid(l):
    return 0.5 * (1.0 + np.tanh(0.5 * np.asarray(l, np.float64)))


def sigmoid_rel(l):
    """sigmoid with a small RELATIVE error on both tails (the tanh form above is good to 1e-16 absolute: a guess of 1e-13 needs more)."""
    return np.exp(-np.logaddexp(0.0, -np.asarray(l, np.float64)))


def g_bound(logit, e_logit, dgdl=None, c_eval=C_SIGMA):
    """Bound of the error of g = d ll/d l evaluated in fp32 from a logit that is off by at most e_logit.  dgdl: |d g/d l| where it
    is not sigmoid' (3PL)."""
    s = sigmoid(logit)
    return (s * (1.0 - s) if dgdl is None else np.abs(dgdl)) * e_logit + e_logit ** 2 + c_eval * U


def ll_bound(ll, g, obs, e_logit, fp32=False):
    """Bound of |S_LL - sum of the exact ll| of a forward-only launch (module docstring, 'Forward only'); fp32: a plain fp32 sum,
    one rounding per cell."""
    obs = np.asarray(obs, bool)
    n = obs.sum() if fp32 else obs.sum() / 4
    return float(np.where(obs, np.abs(g) * e_logit + e_logit ** 2, 0.0).sum() + (n + 20) * U * np.abs(np.where(obs, ll, 0.0)).sum())


def eps_g(g):
    return np.maximum(C_SPLIT * np.abs(g), np.where(g != 0, 2.0 ** -24, 0.0))


def grad_a_model(g, theta, jsh, drop_g_lo=False):
    """sum_p g theta of the scheme: (g_hi + g_lo) x (theta'_hi + theta'_lo) 2^jsh; g [B, I] (0 at unobserved cells) -> [I, A].
    Returned with the sign of d LL / d a = -sum_p g theta."""
    gh, gl = split_rtz(g)
    th, tl = split_rtz(np.asarray(f32(theta), np.float64) * 2.0 ** -jsh)
    gs = gh if drop_g_lo else gh + gl
    return -(gs.T @ (th + tl)) * 2.0 ** jsh


def grad_theta_model(g, a, irt, jsh, drop_g_lo=False):
    """d LL / d theta = -sum_i g a of the scheme: (g_hi + g_lo) x (a'_hi + a'_lo) 2^-jsh ln 2 -> [B, A]."""
    na, _ = item_operands(a, np.zeros(np.asarray(a).shape[0], np.float32), irt)
    gh, gl = split_rtz(g)
    ah, al = split_rtz(na * 2.0 ** jsh)
    gs = gh if drop_g_lo else gh + gl
    return (gs @ (ah + al)) * 2.0 ** -jsh * LN2


def grad_bounds(theta, a, b, g, obs, e_logit, irt=2, fp32=False, dgdl=None, c_eval=C_SIGMA):
    """Bounds of the three gradient blocks for responses whose exact g is `g` [B, I] (zero where obs is False), given the
    per-cell logit bound e_logit.  -> (bound d LL/d b [I], bound d LL/d a [I, A], bound d LL/d theta [B, A]); panel by panel,
    d LL/d theta summed over the panels."""
    I = np.asarray(b).shape[0]
    out = [_grad_bounds_panel(theta, np.asarray(a)[lo:lo + PANEL], np.asarray(b)[lo:lo + PANEL], g[:, lo:lo + PANEL], np.asarray(obs)[:, lo:lo + PANEL],
                              e_logit[:, lo:lo + PANEL], irt, fp32, None if dgdl is None else dgdl[:, lo:lo + PANEL], c_eval) for lo in range(0, I, PANEL)]
    return np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out]), sum(o[2] for o in out)


def _grad_bounds_panel(theta, a, b, g, obs, e_logit, irt, fp32, dgdl, c_eval):
    o = scaled_operands(theta, a, b, irt)
    t = np.abs(np.asarray(f32(theta), np.float64))
    a_abs = np.abs(o['na']) * LN2                                      # |a| (1PL: 1) up to 2u
    obs = np.asarray(obs, dtype=bool)
    l = exact_logit(theta, a, b)
    dg = np.where(obs, g_bound(l, e_logit, dgdl, c_eval), 0.0)
    ag = np.abs(g)
    n_i, n_p = obs.sum(0), obs.sum(1)
    bnd_b = dg.sum(0) + (n_i + 8) * U * ag.sum(0)
    if fp32:
        eg = np.zeros_like(dg)
        et_u = np.zeros_like(t)
        ea_u = np.zeros_like(a_abs)
    else:
        eg = np.where(obs, eps_g(g), 0.0)
        et_u = eps_split(o['t_s']) * 2.0 ** o['jsh']
        ea_u = eps_split(o['a_s']) * 2.0 ** -o['jsh'] * LN2
    ga = ag.T @ t                                                      # sum_p |g theta_k|  [I, A]
    bnd_a = (dg + eg).T @ t + ag.T @ et_u + 4 * U * ga + ((n_i + 8) * U)[:, None] * ga
    gt = ag @ a_abs                                                    # sum_i |g a_k|      [B, A]
    bnd_t = (dg + eg) @ a_abs + ag @ ea_u + 4 * U * gt + ((n_p + 8) * U)[:, None] * gt
    return bnd_b, bnd_a, bnd_t


# ---------------------------------------------------------------------------------------------------------------------------
# Adversarial inputs (shared by tests/test_split_model.py and tests/test_gpu_split_worst_case.py)
# ---------------------------------------------------------------------------------------------------------------------------
HOSTILE_MANTISSAS = (0x7FFFFF, 0x7FF001, 0x7FEFFF, 0x7FF000, 0x001FFF, 0x000000, 0x7FE000, 0x400000, 0x7FFFFE, 0x2AAAAA, 0x555555,
                     0x0007FF, 0x000001, 0x3FF800)
DELTAS = (1e-3, -1e-3, 0.1, -0.1, 1.0, -1.0, 3.0, -3.0)
CLASSES = ('cancel', 'hostile', 'bias', 'mixed_a', 'mixed_b', 'clamp3', 'onepl', 'threepl')


def from_bits(sign, exponent, mantissa):
    """fp32 values sign 2^exponent (1 + mantissa 2^-23)."""
    bits = (np.asarray(sign < 0, np.uint32) << 31) | ((np.asarray(exponent, np.int64) + 127).astype(np.uint32) << 23) | \
        np.asarray(mantissa, np.uint32)
    return bits.astype(np.uint32).view(np.float32)


def observer(I, B, shift):
    """Person who observes item i: every item has exactly one observer."""
    return (np.arange(I) + shift) % B


def _hostile(rng, shape, e_lo, e_hi):
    m = rng.choice(np.asarray(HOSTILE_MANTISSAS, np.uint32), size=shape)
    return from_bits(rng.choice([-1, 1], size=shape), rng.integers(e_lo, e_hi + 1, size=shape), m)


def make_case(cls, A, B, I, seed, theta=None, shift=0, outliers=(), same_tile=False, all_signs=False):
    """One seeded problem of class `cls` -> dict(irt, theta [B, A], a [I, A], b [I], resp [B, I], obs [B, I] bool, p_obs [I]).
    theta: given (fp32 [B, A]) when the caller cannot choose the samples (unconditional posterior); else drawn here.
    Every item is observed by the single person p_obs[i]; b is set in fp64 (then rounded to fp32) so that THAT cell's logit is a
    prescribed delta.  outliers (classes mixed_a / mixed_b): exponents k of the items with |a| = 2^k resp. |b| = 2^k; same_tile
    puts them among the first 16 items (the tile of the first observed cells) instead of in the last wave's span.
    all_signs: the signs of theta_p are the bits of p and those of a_i the bits of i >> A, so that the observed cells run through every
    one of the 2^A x 2^A sign patterns (round toward zero is not symmetric in how lo inherits the sign).
    clamp3 (3PL): cancelling logits as in 'cancel', placed so that p = c + (1 - c) sigmoid(l) of the observed cell lies within 1e-6 of a
    probability clamp value: just inside 1 - eps32 (1 - p = 4 ... 8 eps32), on both sides of eps32 (c < eps32: guess logits -16.5 ...
    -30, l = -15.94 +- 0.02 ... 1; where the logit is below -15.94 the guess is so small that the exact p is below eps32 as well, so the
    reference's logit clamp and its probability clamp agree), and about 1 % of the items within 4 ulp of eps32 (guess logit -40).
    threepl (3PL): an ordinary 3PL problem -- logits as in 'cancel', guess logits uniform in (-2, 1): p = 0.12 ... 1 - 1e-2, far from both
    probability clamps, so the guess gradient is alive in every observed cell."""
    rng = np.random.default_rng(seed)
    irt = 1 if cls == 'onepl' else 3 if cls in ('clamp3', 'threepl') else 2
    own_theta = theta is None
    sgn = lambda shape: rng.choice([-1.0, 1.0], size=shape)
    if own_theta:
        if cls == 'hostile':
            theta = _hostile(rng, (B, A), -2, 2)
        elif cls == 'bias':
            theta = (sgn((B, A)) * rng.uniform(0.01, 0.03, (B, A))).astype(np.float32)
        else:
            theta = (sgn((B, A)) * rng.uniform(1.0, 4.0, (B, A))).astype(np.float32)
    theta = f32(theta)
    if cls == 'hostile':
        a = _hostile(rng, (I, A), -2, 2)
    elif cls == 'bias':
        a = (sgn((I, A)) * rng.uniform(0.003, 0.03, (I, A)) / A).astype(np.float32)
        a[::4] = 0.0                                 # every fourth item: all products exactly zero -- the bias pieces alone
    elif cls in ('mixed_a', 'mixed_b'):
        a = (sgn((I, A)) * rng.uniform(0.5, 2.0, (I, A))).astype(np.float32)
        a[1::3] *= np.float32(2.0 ** -6)
    elif cls == 'onepl':
        a = np.full((I, A), -1.0, np.float32)
    else:
        a = (sgn((I, A)) * rng.uniform(1.0, 4.0, (I, A))).astype(np.float32)
    p_obs = observer(I, B, shift)
    if all_signs:
        assert own_theta and cls == 'cancel'
        bits = lambda n: 1.0 - 2.0 * ((np.asarray(n)[:, None] >> np.arange(A)[None, :]) & 1)
        theta = f32(np.abs(theta) * bits(np.arange(B)))
        a = f32(np.abs(a) * bits(np.arange(I) >> A))
    gamma = None
    if cls == 'clamp3':
        kind = rng.integers(0, 99, I)
        kind[np.arange(I) % 97 == 50] = 99                                            # ~1 % of the items: see below
        gamma = rng.uniform(-2.0, 1.0, I)
        target = np.zeros(I)
        hi_side = kind < 45
        c = sigmoid(gamma)
        sgm1 = rng.choice([4.0, 5.0, 6.0, 8.0], I) * EPS32 / (1.0 - c)          # 1 - sigmoid(l) that puts 1 - p at 4 ... 8 eps32
        target[hi_side] = np.log((1.0 - sgm1) / sgm1)[hi_side]
        live_lo = (kind >= 45) & (kind < 75)                                          # p just above eps32, logit alive
        gamma[live_lo] = rng.choice([-16.5, -17.5, -30.0], int(live_lo.sum()))
        target[live_lo] = -LOGIT_LO + rng.choice([0.02, 0.1, 0.5, 1.0], int(live_lo.sum()))
        dead_lo = kind >= 75                                                          # p below eps32 (and the logit below its clamp)
        gamma[dead_lo] = -30.0
        gamma[kind == 99] = -40.0                                                     # ... within 4 ulp of eps32: excluded cells
        target[dead_lo] = -LOGIT_LO - rng.choice([0.02, 0.1, 0.5], int(dead_lo.sum()))
        gamma = f32(gamma)
    if cls == 'threepl':
        gamma = f32(rng.uniform(-2.0, 1.0, I))
    at = np.einsum('ik,ik->i', np.asarray(a, np.float64), np.asarray(theta, np.float64)[p_obs])
    if cls == 'bias':
        b = _hostile(rng, (I,), -3, 2)               # |b| in [1/8, 8)
    else:
        delta = target if cls == 'clamp3' else np.asarray(DELTAS)[rng.integers(0, len(DELTAS), I)]
        b = f32(at + delta)
        if cls == 'hostile':                         # hostile difficulties too: a hostile mantissa in the binade the cancellation asks for
            _, e = np.frexp(np.abs(np.asarray(b, np.float64)))
            hb = from_bits(np.sign(b) + (b == 0), np.clip(e - 1, -20, 20), rng.choice(np.asarray(HOSTILE_MANTISSAS, np.uint32), size=I))
            keep = np.abs(-at + np.asarray(hb, np.float64)) <= 3.0
            b = np.where(keep, hb, b).astype(np.float32)
    out_idx = np.zeros(0, np.int64)
    if outliers:
        out_idx = (np.arange(len(outliers)) * 5 + 2) if same_tile else (I - 3 - np.arange(len(outliers)) * 37)
        for j, k in zip(out_idx, outliers):
            if cls == 'mixed_a':
                a[j] = f32(sgn(A) * 2.0 ** k)
                b[j] = 0.0
            else:
                b[j] = np.float32(-(2.0 ** k) if (j & 1) else 2.0 ** k)
    obs = np.zeros((B, I), bool)
    obs[p_obs, np.arange(I)] = True
    resp = np.random.default_rng([seed, 1]).integers(0, 2, (B, I)).astype(np.float32)      # (a stream of its own: the same for any theta)
    return dict(cls=cls, irt=irt, theta=theta, a=f32(a), b=f32(b), gamma=gamma, resp=resp, obs=obs, p_obs=p_obs, outliers=out_idx)


def item_tensor(case):
    """[I, D] item sample as the kernel takes it (1PL: the difficulty alone)."""
    if case['irt'] == 1:
        return case['b'][:, None].copy()
    cols = [case['a'], case['b'][:, None]] + ([case['gamma'][:, None]] if case['irt'] == 3 else [])
    return np.concatenate(cols, axis=1).astype(np.float32)


def ulp32(x):
    return np.exp2(np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** -126))) - 23)


def reference(case, theta=None):
    """fp64 reference of a case on the fp32 theta the kernel used: exact logits, ll and g = d ll/d l per cell (zero where
    unobserved), |d g/d l|, the three gradients, g_c = d LL / d guess-logit per item with its per-cell terms gc and |d gc/d l| (3PL;
    zeros otherwise), and `excluded` (3PL cells within 4 fp32 ulp of a probability clamp value).
    Saturation as in vibo_table_ref.fused_elbo_ref(exact_saturation=True): the logit held to +-LOGIT_LO for the value, gradient zero
    outside [-LOGIT_LO, LOGIT_HI] and, 3PL, where p leaves [eps32, 1 - eps32]."""
    theta = case['theta'] if theta is None else f32(theta)
    a64, t64 = np.asarray(case['a'], np.float64), np.asarray(theta, np.float64)
    l = exact_logit(theta, case['a'], case['b'])
    x, obs = case['resp'], case['obs']
    lc = np.clip(l, -LOGIT_LO, LOGIT_LO)
    live = (l >= -LOGIT_LO) & (l <= LOGIT_HI)
    sg = sigmoid(lc)
    excluded = np.zeros_like(obs)
    if case['irt'] == 3:
        c = sigmoid(np.asarray(case['gamma'], np.float64))[None, :]
        p = c + (1.0 - c) * sg
        q = (1.0 - c) * (1.0 - sg)                                     # 1 - p without the cancellation
        pc, qc = np.clip(p, EPS32, 1.0 - EPS32), np.clip(q, EPS32, 1.0 - EPS32)
        live = live & (p >= EPS32) & (p <= 1.0 - EPS32)
        excluded = obs & ((np.abs(p - EPS32) < 4 * ulp32(p)) | (np.abs(q - EPS32) < 4 * ulp32(p)))
        ll = np.where(x == 1, np.log(pc), np.log(qc))
        p1, p2 = (1.0 - c) * sg * (1.0 - sg), (1.0 - c) * sg * (1.0 - sg) * (1.0 - 2.0 * sg)
        g = np.where(x == 1, p1 / pc, -sg)
        dgdl = np.where(x == 1, np.abs(p2 / pc - (p1 / pc) ** 2), sg * (1.0 - sg))
        # d ll / d guess-logit = (x / p - (1 - x) / (1 - p)) (1 - sigmoid(l)) c (1 - c): c (1 - c) (1 - sg) / p answered right, -c wrong
        cr = sigmoid_rel(np.asarray(case['gamma'], np.float64))[None, :]
        gc = np.where(x == 1, cr * (1.0 - c) * (1.0 - sg) / pc, -cr * np.ones_like(sg))
        dgcdl = np.where(x == 1, cr * (1.0 - c) * sg * (1.0 - sg) * (1.0 / pc + (1.0 - c) * (1.0 - sg) / pc ** 2), 0.0)
    else:
        ll = x * lc - np.maximum(lc, 0.0) - np.log1p(np.exp(-np.abs(lc)))
        g = x - sg
        dgdl = sg * (1.0 - sg)
        gc, dgcdl = np.zeros_like(l), np.zeros_like(l)
    g = np.where(obs, g, 0.0) * live
    gc = np.where(obs, gc, 0.0) * live
    return dict(logit=l, g=g, dgdl=dgdl, ll=np.where(obs, ll, 0.0), g_b=g.sum(0), g_a=-(g.T @ t64), g_theta=-(g @ a64), live=live,
                excluded=excluded, gc=gc, dgcdl=dgcdl, g_c=gc.sum(0))
