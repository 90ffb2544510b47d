"""TEST INFRASTRUCTURE ONLY -- fp64 model of the MLP decoder kernel's f16 hi/lo arithmetic (csrc/vibo_decoder.hip, decoder_kernel) and
an a-priori error bound per output entry, in the style of oracle/split_model.py.  It restates WHAT the kernel computes per term and how
its records are laid out; it is not a port (no lanes, no LDS image).  Everything is numpy float64: an fp32 input is exact in it, and so
is every product of two f16 pieces.

Pieces
  activations (split8, vibo_decoder_device.hpp): hi = rtz16(x) (v_cvt_pkrtz), lo = rn16(x - hi) (lo_pieces4: v_fma_mix{lo,hi}_f16 of
      hi * -1 + x, round to nearest even; x - hi is an fp32 number, so the fma itself is exact).  f16 subnormals are kept.
  weights (vibo_decoder.hip:69-71): fh = dpk(w)[0], lo = dpk(w - (float)fh)[0]: BOTH pieces round toward zero (split_model.split_rtz).
  Residual of a split, eps(x) = |x - hi - lo|: lo lies on a grid of 2^(E-21) for 2^E <= |x| < 2^(E+1) while it is a normal f16, so
      eps <= 2^(E-22) <= 4u|x| (activations, nearest; twice that for the truncated weights) -- but never below half (weights: one)
      step of the f16 subnormal grid 2^-24: eps <= 2^-25 ABSOLUTE once |x| < 2^-3, and below 2^-14 hi is on that grid too.  The
      kernel does not rescale its operands, so this absolute floor is the scheme's accuracy at small |W2|, |h1| or |dz2|.
      The weights are inputs: their residual is EVALUATED (res_W).  An activation's residual is evaluated where the kernel's value is
      known to the bit (z1 > 0 from one IEEE addition: h1 = z1), and bounded by the grid (apriori) everywhere else.

The scheme's value of one term (terms(scheme=True); every statement of the kernel's person loop in its order)
  z1 = U + V (+ w1 l)          h1 = fl32(ELU(z1))                         ELU(z) = z > 0 ? z : exp2(z log2 e) - 1
  z2 = W_hi.h_hi + W_hi.h_lo + W_lo.h_hi + b2        h2 = ELU(z2)         (lo.lo dropped)
  o  = w3.h2 + b3 (+ resid l)   sg = sigmoid(o), sq = 1 - sg formed apart, p = guess + (1 - guess) sg, q = (1 - guess) sq,
  clamp to [eps32, 1 - eps32] (gradient zero outside), ll = log(p | q), dldp = 1/p | -1/q, d_o = dldp (1 - guess) sg sq,
  dz2 = fl32(d_o w3 ELU'(z2)),  ELU' = 1 | h + 1
  dH1 = W_hi.dz_hi + W_hi.dz_lo + W_lo.dz_hi,  dz1 = dH1 ELU'(z1),  dl = w1.dz1 + resid d_o
  dW2 += dz_hi x h_hi + dz_hi x h_lo + dz_lo x h_hi            (the four through_image pieces Ah, Al, Bh, Bl)

Bound per observable, u = 2^-24 (term_bounds / record_bounds; first order, times 1 + 2^-10 for the second).  Each constant with the
statement of vibo_decoder.hip it counts:
  e_z1   `z1 = u + v`: one addition, u|U + V| (no U: V itself, exact); `fmaf(w1v, l, z1)`: one more rounding, u|z1|.
  e_elu  `elu`: z > 0 exact.  Else `fast_exp2(z * kLog2e) - 1.0f`: the product and the fp32 constant 2u|z| e^z, v_exp_f32 at 1 ulp
         (ASSUMED) <= 2u e^z, the subtraction u|h|: an ABSOLUTE error of about 2u as z -> 0-, not a relative one.  elu(0) = 0 exactly.
         ELU' = h + 1: that error plus u.  Within the argument's own error of 0 either branch may be taken; both formulas cover it.
  E_z2   sum_k |W| (e_h1 + eps_h) + res_W |h1| + |W_lo| |h_lo| (the dropped product: W_lo evaluated, h_lo evaluated where the kernel's
         h1 is known to the bit, else at most one step of hi's grid, lo_max) + E_acc + u|z2| (`acc[j] + b2v`).
         The product of the two operands' errors, res_W (e_h1 + eps_h), is kept as a term of its own (and (E_dz2 + eps_dz)(e_h1 + eps_h) in
         dW2): at small scales eps is not small against its operand -- 2^-25 absolute is 0.2 % of a dz2 of 2^-16 -- and the kernel
         left the first-order bound of dW2 by up to 0.8 % there on the device before this term was counted.
  E_acc  the matrix pipe at 2 roundings per accumulate and nonzero product (ASSUMED, as oracle/onehot_model.py C_MFMA): one MFMA with
         m nonzero products of absolute sum S into an accumulator whose terms so far sum to T in absolute value costs
         2u ((m - 1) S + T).  Forward and backward: six MFMAs per output (`for s: dmfma(ah, h1h); dmfma(ah, h1l); dmfma(al, h1h)`,
         K = 32 each); dW2: three per person pair (`dmfma(Ah, Bh); (Ah, Bl); (Al, Bh)`, K = the pair's 32 terms) into accW for the
         whole launch.  All products zero: no rounding, E_acc = 0.  S and T are taken on NOMINAL sizes: a nonzero subnormal piece counts
         as 2^-14.  Measured on the device (tests/test_gpu_decoder_cells.py, the subnormal x subnormal probe and the `small_g` class): the
         pipe aligns a product by its operands' exponent fields, not by its leading bit, and keeps 24 bits below the largest; with
         dz_hi = 6 2^-24 and h = (1751 2^-13, 4 2^-24) the product dz_hi h_lo = 1.5 2^-44 arrived as 2^-41, one step of that window --
         52 ulp of the result.  On normal operands the two sizes are the same.
  E_o    `opart = fmaf(w3v, h2, opart)` x 16, xor16_add, xor32_add, `+ b3`, `fmaf(resid, l, o)`: 20 roundings of at most
         u (sum|w3 h2| + |b3| + |resid l|), plus sum |w3| e_h2.
  link   `expf` (device libm at 2 ulp, ASSUMED), `1 + eo`, the division (taken as 1 ulp), `eo * big`: 8u relative on sg and on sq plus
         the propagated sq E_o resp. sg E_o; the guess mixture 3 more roundings; `logf` 2 ulp (ASSUMED): 4u|ll|; `1.0f / pc` 2u;
         `dldp * (1 - guess)` 2u; `dsg * sg * sq` 2u.
  E_dz2  `d_o * w3v * (...)`: 2u|dz2| + |w3 ELU'| E_do + |d_o w3| e_ELU'.
  E_dH1  as E_z2 with W transposed; `acc[j] * (...)`: u|dz1|.          E_dl: 16 fmas + 2 swaps + the resid fma: 19u.
  chains `db2 += d`, `dw3 = fmaf`, `dw1 = fmaf`, `dU += dz1`, `llsum += ll`: one rounding per person of the chunk; the DPP row
         reduction (quad_perm x 2, row_half_mirror, row_mirror): 4; wave_total (wave_sum63, six steps of which four meet nonzero
         lanes: only g == 0 holds a value): 6.  Taken as (persons of the chunk + 6) u sum|terms| for every summed record.
Entries whose bound is zero (unobserved terms, padded hidden units, empty chunks, W2 = 0) must be exact zeros / exact values.

The 3PL clamp flips with the last bits of p: cells whose exact p or q lies within 4 fp32 ulp of eps32 / 1 - eps32 are `excluded`
(asserted by nobody; the generator keeps them under 2 % of a case, checked in tests/test_decoder_model.py).

Layout (layout(); vibo_decoder_fwd_bwd): ppc = (ceil(B / chunks) + 1) & ~1; chunk c holds persons [c ppc, min(B, (c + 1) ppc)) and is
empty from c ppc >= B on (its records are zeros); wave_id = (c n_ib + ib) 4 + w with n_ib = ceil(I / 64); wave w of item block ib owns
items 64 ib + 16 w ... + 15.  Records: ll_part [4 n_ib chunks], dW2_part [waves, 64, 64] (n, k), dvec_part [waves, 4, 64] (db2, dw3, dw1,
db3 in column 0), dV_part [4 n_ib, B, 64], dU_part [chunks, I, 64], dguess_part [chunks, I], dL [B, I].  K(g) = {16 kt + 4 g + j}: lane
(i16, g) holds hidden units K(g), in the order kt-major, j-minor; step s of an MFMA contracts k in [32 s, 32 s + 32).

Measured by tests/test_decoder_model.py (pytest -s prints them): the scheme inside every bound on 100 % of the entries; every mutation
outside some bound by at least 4 x in every class where it can act.
"""
import numpy as np

from oracle import split_model as M

U_ = 2.0 ** -24
SECOND = 1.0 + 2.0 ** -10
EPS32 = 2.0 ** -23
H = 64
CLASSES = ('unit', 'hostile', 'cancel', 'small_w', 'small_g', 'large', 'elu0', 'zero', 'guess3')
DROPS = ('f_hl', 'f_lh', 'b_hl', 'b_lh', 'w_hl', 'w_lh')              # W_hi.h_lo, W_lo.h_hi | W_hi.dz_lo, W_lo.dz_hi | dz_hi x h_lo, dz_lo x h_hi
MUTATIONS = DROPS + ('slot', 'lgt_other', 'stale_pair', 'elu_layer', 'pad_person', 'tail_item')
OBSERVABLES = ('prob', 'll', 'dL', 'dV', 'dU', 'dguess', 'dW2', 'db2', 'dw3', 'dw1', 'db3')


def f64(x):
    return None if x is None else np.asarray(x, np.float64)


def fl32(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def rn16(x):
    """Round to nearest even onto the f16 grid, subnormals kept (x: an fp32 number held in float64)."""
    with np.errstate(over='ignore'):
        return np.asarray(x, np.float64).astype(np.float32).astype(np.float16).astype(np.float64)


def split_act(x):
    """split8: hi = rtz16(x), lo = rn16(x - hi)."""
    x = np.asarray(x, np.float64)
    hi = M.rtz16(x)
    return hi, rn16(x - hi)


split_w = M.split_rtz                                   # vibo_decoder.hip:69-71: dpk for both pieces


def apriori(ax):
    """Grid bound of an activation's split residual for a value of magnitude at most ax: half a step of lo's grid."""
    ax = np.asarray(ax, np.float64)
    e = np.floor(np.log2(np.maximum(ax, 2.0 ** -126)))
    return np.where(ax > 0, np.maximum(np.exp2(e - 22), 2.0 ** -25), 0.0)


def lo_max(ax):
    """The largest |lo| of an activation of magnitude at most ax: one step of hi's grid (hi truncates; lo may round up to the step)."""
    ax = np.asarray(ax, np.float64)
    e = np.floor(np.log2(np.maximum(ax, 2.0 ** -126)))
    return np.where(ax > 0, np.maximum(np.exp2(e - 10), 2.0 ** -24), 0.0)


def elu(z):
    return np.where(z > 0, z, np.expm1(np.minimum(z, 0.0)))


def elu_err(z, ez):
    """-> (error of ELU(z), error of ELU'(z)) for an argument off by at most ez (module docstring, e_elu)."""
    ez_ = np.exp(np.minimum(z, 0.0))
    neg = ez_ * (ez + 2 * U_ * np.abs(z)) + 2 * U_ * ez_ + U_ * np.abs(np.expm1(np.minimum(z, 0.0)))
    exact0 = (z == 0) & (ez == 0)
    e_val = np.where(exact0, 0.0, np.where(z > ez, ez, np.maximum(neg, ez)))
    e_der = np.where(exact0 | (z > ez), 0.0, neg + U_)
    return e_val, e_der


def sig_pair(o):
    """(sigmoid(o), 1 - sigmoid(o)), each with a small relative error on its own tail."""
    return np.exp(-np.logaddexp(0.0, -o)), np.exp(-np.logaddexp(0.0, o))


# ---------------------------------------------------------------------------------------------------------------------------
# the launch layout
# ---------------------------------------------------------------------------------------------------------------------------
class Layout:
    def __init__(self, B, I, chunks):
        assert 1 <= chunks <= B
        self.B, self.I, self.chunks = B, I, chunks
        self.ppc = ((B + chunks - 1) // chunks + 1) & ~1
        self.n_ib = (I + 63) // 64
        self.n_wave = 4 * self.n_ib * chunks
        self.ranges = [(min(c * self.ppc, B), min(B, (c + 1) * self.ppc)) for c in range(chunks)]
        self.empty = [c for c, (lo, hi) in enumerate(self.ranges) if lo >= hi]
        self.shapes = dict(ll_part=(self.n_wave,), dW2_part=(self.n_wave, H, H), dvec_part=(self.n_wave, 4, H),
                           dV_part=(4 * self.n_ib, B, H), dU_part=(chunks, I, H), dguess_part=(chunks, I), dL=(B, I))

    def wave_id(self, c, ib, w):
        return (c * self.n_ib + ib) * 4 + w

    def wave_items(self, ib, w):
        lo = 64 * ib + 16 * w
        return np.arange(lo, min(lo + 16, self.I)) if lo < self.I else np.zeros(0, np.int64)

    def tail_lanes(self, ib, w):
        """Lanes of the wave past the last item (they compute item 0 again with ok == false)."""
        return 16 - len(self.wave_items(ib, w))

    def pairs(self, c):
        lo, hi = self.ranges[c]
        return [(p, p + 1 if p + 1 < hi else None) for p in range(lo, hi, 2)]

    def chunk_of(self, p):
        return p // self.ppc

    def waves(self):
        for c in range(self.chunks):
            for ib in range(self.n_ib):
                for w in range(4):
                    yield c, ib, w


def layout(B, I, chunks):
    return Layout(B, I, chunks)


def k_of(g):
    """K(g): the hidden units of lane group g, in register order."""
    return [16 * kt + 4 * g + j for kt in range(4) for j in range(4)]


# ---------------------------------------------------------------------------------------------------------------------------
# per-term values
# ---------------------------------------------------------------------------------------------------------------------------
def _src_person(lay, mut):
    src = np.arange(lay.B)
    if mut == 'stale_pair':                              # cur never advanced: every pair of a chunk reads the first pair's inputs
        for lo, hi in lay.ranges:
            for p in range(lo, hi):
                src[p] = min(lo + (p - lo) % 2, hi - 1)
    return src


def terms(case, lay=None, scheme=True, mut=None):
    """Per-term values [B, I(, 64)] of the exact network (scheme=False) or of the kernel's scheme with exact accumulation."""
    resp, mask = f64(case['resp']), case['mask']
    B, I = resp.shape
    src = _src_person(lay, mut) if lay is not None else np.arange(B)
    rnd = fl32 if scheme else (lambda a: a)
    V, Um, L, guess, w1 = f64(case['V'])[src], f64(case['U']), f64(case['L']), f64(case['guess']), f64(case['w1'])
    W2, b2, w3, b3, resid = f64(case['W2']), f64(case['b2']), f64(case['w3']), float(case['b3']), float(case['resid'])
    x = resp[src]
    obs = (np.ones((B, I), bool) if mask is None else np.asarray(mask, bool))[src]
    z1 = V[:, None, :] + (Um[None] if Um is not None else 0.0)
    if Um is not None:
        z1 = rnd(z1)
    l = L[src] if L is not None else np.zeros((B, I))
    if L is not None:
        z1 = rnd(z1 + (w1 if w1 is not None else np.zeros(H)) * l[..., None])
    h1 = rnd(elu(z1))
    T = dict(z1=z1, h1=h1, l=l, obs=obs)
    if scheme:
        hh, hl = split_act(h1)
        Wh, Wl = split_w(W2)
        Fh, Fl = Wh, Wl
        if mut == 'slot':                               # slot (s, e) = (1, 5) of the forward image reads the kk of e = 4
            ks = np.array([16 * 3 + 4 * g + 1 for g in range(4)])
            Fh, Fl = Wh.copy(), Wl.copy()
            Fh[:, ks], Fl[:, ks] = Wh[:, ks - 1], Wl[:, ks - 1]
        z2 = hh @ Fh.T + (0.0 if mut == 'f_hl' else hl @ Fh.T) + (0.0 if mut == 'f_lh' else hh @ Fl.T) + b2
        T.update(hh=hh, hl=hl, Wh=Wh, Wl=Wl)
    else:
        z2 = h1 @ W2.T + b2
    h2 = elu(z2)
    o = h2 @ w3 + b3 + resid * l
    sg, sq = sig_pair(o)
    g = guess[None, :] if guess is not None else 0.0
    p, q = g + (1.0 - g) * sg, (1.0 - g) * sq
    inside = (p >= EPS32) & (p <= 1.0 - EPS32)
    pc = np.clip(p, EPS32, 1.0 - EPS32)
    qc = np.where(inside, q, 1.0 - pc)
    one = x > 0.5
    px = np.where(one, pc, qc)
    ll = np.where(obs, np.log(np.maximum(px, EPS32)), 0.0)
    dldp = np.where(obs & inside, np.where(one, 1.0 / pc, -1.0 / qc), 0.0)
    d_o = dldp * (1.0 - g) * sg * sq
    d2 = np.where(h2 > 0, 1.0, h2 + 1.0)
    dz2 = rnd(d_o[..., None] * w3 * d2)
    if scheme:
        dzh, dzl = split_act(dz2)
        dH1 = dzh @ Wh + (0.0 if mut == 'b_hl' else dzl @ Wh) + (0.0 if mut == 'b_lh' else dzh @ Wl)
        T.update(dzh=dzh, dzl=dzl)
    else:
        dH1 = dz2 @ W2
    d1 = d2 if mut == 'elu_layer' else np.where(h1 > 0, 1.0, h1 + 1.0)
    dz1 = dH1 * d1
    dl = (dz1 @ w1 if w1 is not None else 0.0) + resid * d_o
    ulp = M.ulp32(p)
    excluded = obs & ((np.abs(p - EPS32) < 4 * ulp) | (np.abs(p - (1.0 - EPS32)) < 4 * ulp) | (np.abs(q - EPS32) < 4 * M.ulp32(q)))
    T.update(z2=z2, h2=h2, o=o, sg=sg, sq=sq, p=p, q=q, px=px, inside=inside, one=one, ll=ll, dldp=dldp, d_o=d_o, d2=d2, dz2=dz2,
             dH1=dH1, d1=d1, dz1=dz1, dl=dl * np.ones((B, I)), dgs=dldp * sq, excluded=excluded, g=g * np.ones((1, I)))
    return T


# ---------------------------------------------------------------------------------------------------------------------------
# records
# ---------------------------------------------------------------------------------------------------------------------------
def _wave_sets(lay, mut):
    """Per wave: (c, ib, w, persons [n], items [m]) with the duplicates the padding mutations count."""
    for c, ib, w in lay.waves():
        lo, hi = lay.ranges[c]
        ps = list(range(lo, hi))
        if mut == 'pad_person' and (hi - lo) % 2:
            ps.append(hi - 1)                           # the padded second person of the last pair (clamped to p_end - 1) counted
        it = list(lay.wave_items(ib, w))
        if mut == 'tail_item' and it:
            it += [0] * lay.tail_lanes(ib, w)           # lanes past the last item compute item 0
        yield c, ib, w, np.asarray(ps, np.int64), np.asarray(it, np.int64)


def records(T, lay, scheme=True, mut=None):
    """The kernel's outputs from per-term values: dict of arrays in the shapes of Layout.shapes, plus prob [B, I]."""
    B, I = lay.B, lay.I
    out = {k: np.zeros(s) for k, s in lay.shapes.items()}
    out['prob'] = T['p'].copy()
    out['dL'] = T['dl'].copy()
    lw = T['l']
    if mut == 'lgt_other':                              # dw1 takes lgt[r ^ 1]: the other person of the pair
        lw = lw.copy()
        for c in range(lay.chunks):
            for a, b in lay.pairs(c):
                if b is not None:
                    lw[[a, b]] = T['l'][[b, a]]
    for c, ib, w, ps, it in _wave_sets(lay, mut):
        wid = lay.wave_id(c, ib, w)
        if not len(ps) or not len(it):
            continue
        sel = np.ix_(ps, it)
        out['ll_part'][wid] = T['ll'][sel].sum()
        out['dvec_part'][wid, 0] = T['dz2'][sel].sum((0, 1))
        out['dvec_part'][wid, 1] = (T['d_o'][sel][..., None] * T['h2'][sel]).sum((0, 1))
        out['dvec_part'][wid, 2] = (T['dz1'][sel] * lw[sel][..., None]).sum((0, 1))
        out['dvec_part'][wid, 3, 0] = T['d_o'][sel].sum()
        if scheme:
            dzh, dzl, hh, hl = (T[k][sel].reshape(-1, H) for k in ('dzh', 'dzl', 'hh', 'hl'))
            out['dW2_part'][wid] = dzh.T @ hh + (0.0 if mut == 'w_hl' else dzh.T @ hl) + (0.0 if mut == 'w_lh' else dzl.T @ hh)
        else:
            out['dW2_part'][wid] = T['dz2'][sel].reshape(-1, H).T @ T['h1'][sel].reshape(-1, H)
        real = it[:len(lay.wave_items(ib, w))]
        out['dU_part'][c][real] = T['dz1'][np.ix_(ps, real)].sum(0)
        out['dguess_part'][c][real] = T['dgs'][np.ix_(ps, real)].sum(0)
        for p in range(*lay.ranges[c]):
            out['dV_part'][4 * ib + w, p] = T['dz1'][p][it].sum(0)
    return out


def run(case, chunks, scheme=True, mut=None):
    lay = layout(*np.asarray(case['resp']).shape, chunks)
    T = terms(case, lay, scheme, mut)
    return T, records(T, lay, scheme, mut), lay


# ---------------------------------------------------------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------------------------------------------------------
def nominal(x):
    """|x| of an f16 piece as the matrix pipe's alignment sees it: a nonzero subnormal counts as 2^-14 (its exponent field)."""
    ax = np.abs(x)
    return np.where(ax > 0, np.maximum(ax, 2.0 ** -14), 0.0)


def _acc(b_hi, b_lo, a_hi, a_lo):
    """E_acc of out[..., n] = sum_k a[n, k] b[..., k] as six MFMAs (module docstring): 2u sum_j ((m_j - 1) S_j + T_j), on nominal sizes."""
    tot, run_ = 0.0, 0.0
    for s in range(2):
        ks = slice(32 * s, 32 * s + 32)
        for a, b in ((a_hi, b_hi), (a_hi, b_lo), (a_lo, b_hi)):
            S = nominal(b[..., ks]) @ nominal(a[:, ks]).T
            m = (b[..., ks] != 0).astype(np.float64) @ (a[:, ks] != 0).astype(np.float64).T
            run_ = run_ + S
            tot = tot + np.maximum(m - 1, 0) * S + (m > 0) * run_
    return 2 * U_ * tot


def condition(case, X, dz2):
    """X with the backward half restated on GIVEN fp32 values of dz2 [B, I, 64] (the kernel's own, read from dvec_part row 0 where a wave
    holds one observed term): dH1, dz1 and dl follow from them exactly; everything before dz2 is X's."""
    W2, w1 = f64(case['W2']), f64(case['w1'])
    Y = dict(X, dz2=f64(dz2))
    Y['dH1'] = Y['dz2'] @ W2
    Y['dz1'] = Y['dH1'] * X['d1']
    Y['dl'] = (Y['dz1'] @ w1 if w1 is not None else 0.0) + float(case['resid']) * X['d_o']
    return Y


GIVEN = ('dV', 'dU', 'dW2', 'dw1')                   # the observables that follow from dz2 alone (and l, h1)


def term_bounds(case, X, given=False):
    """Error bounds of the per-term values against X = terms(case, scheme=False), from the inputs alone.  given: X = condition(...),
    dz2 is known to the bit -- no propagated error, its split residual evaluated."""
    hasl = case['L'] is not None
    W2, w3, w1 = f64(case['W2']), f64(case['w3']), f64(case['w1'])
    resid = float(case['resid'])
    aW = np.abs(W2)
    Wh, Wl = split_w(W2)
    resW = np.abs(W2 - Wh - Wl)
    z1, h1, z2, h2 = X['z1'], X['h1'], X['z2'], X['h2']
    uv = np.abs(f64(case['V'])[:, None, :] + f64(case['U'])[None]) if case['U'] is not None else 0.0
    e_z1 = U_ * uv + U_ * np.abs(z1) * hasl
    e_h1, e_d1 = elu_err(z1, e_z1)
    h1f = fl32(h1)
    hh, hl = split_act(h1f)
    known = (z1 > e_z1) & (not hasl)
    rep_h = np.where(known, np.abs(h1f - hh - hl), apriori(np.abs(h1) + e_h1))
    hl_max = np.where(known, np.abs(hl), lo_max(np.abs(h1) + e_h1))       # the kernel's own h_lo: evaluated where known, else one step
    acc_f = _acc(hh, hl, Wh, Wl)
    E_z2 = (e_h1 + rep_h) @ (aW + resW).T + np.abs(h1) @ resW.T + hl_max @ np.abs(Wl).T + acc_f + U_ * np.abs(z2) * (acc_f > 0)
    e_h2, e_d2 = elu_err(z2, E_z2)
    S_o = np.abs(h2) @ np.abs(w3) + abs(float(case['b3'])) + np.abs(resid * X['l'])
    E_o = e_h2 @ np.abs(w3) + 20 * U_ * S_o
    sg, sq, g = X['sg'], X['sq'], X['g']
    e_sg, e_sq = sg * (sq * E_o + 8 * U_), sq * (sg * E_o + 8 * U_)
    if case['guess'] is not None:
        e_p, e_q = (1 - g) * e_sg + 2 * U_ * (1 - g) * sg + U_ * X['p'], (1 - g) * e_sq + 2 * U_ * X['q']
    else:
        e_p, e_q = e_sg, e_sq
    obs, inside, one = X['obs'], X['inside'], X['one']
    e_px = np.where(inside, np.where(one, e_p, e_q), 0.0)
    rel_px = e_px / X['px']
    E_ll = np.where(obs, rel_px + 4 * U_ * np.abs(X['ll']), 0.0)
    rel_dldp = rel_px + 2 * U_
    rel_do = rel_dldp + e_sg / sg + e_sq / sq + 6 * U_
    E_do = np.abs(X['d_o']) * rel_do
    E_dgs = np.abs(X['dgs']) * (rel_dldp + e_sq / sq + U_)
    dz2 = X['dz2']
    E_dz2 = np.abs(w3 * X['d2']) * E_do[..., None] + np.abs(X['d_o'][..., None] * w3) * e_d2 + 2 * U_ * np.abs(dz2)
    dzf = fl32(dz2)
    dzh, dzl = split_act(dzf)
    rep_dz = apriori(np.abs(dz2) + E_dz2)
    dzl_max = lo_max(np.abs(dz2) + E_dz2)
    if given:
        E_dz2, rep_dz, dzl_max = np.zeros_like(dz2), np.abs(dzf - dzh - dzl), np.abs(dzl)
    acc_b = _acc(dzh, dzl, Wh.T, Wl.T)
    E_dh1 = (E_dz2 + rep_dz) @ (aW + resW) + np.abs(dz2) @ resW + dzl_max @ np.abs(Wl) + acc_b
    E_dz1 = np.abs(X['d1']) * E_dh1 + np.abs(X['dH1']) * e_d1 + U_ * np.abs(X['dz1'])
    if w1 is not None:
        E_dl = E_dz1 @ np.abs(w1) + 19 * U_ * (np.abs(X['dz1']) @ np.abs(w1) + np.abs(resid * X['d_o'])) + abs(resid) * E_do
    else:
        E_dl = abs(resid) * E_do + U_ * np.abs(resid * X['d_o'])
    return dict(p=e_p * SECOND, ll=E_ll * SECOND, d_o=E_do * SECOND, dgs=E_dgs * SECOND, dz2=E_dz2 * SECOND, dz1=E_dz1 * SECOND,
                dl=E_dl * SECOND, h1=(e_h1 + rep_h) * SECOND, dzr=(E_dz2 + rep_dz) * SECOND, h2=e_h2 * SECOND,
                hl=hl_max, dzl=dzl_max, hh=hh, dzh=dzh, hlo=hl, dzlo=dzl, z2=E_z2 * SECOND, o=E_o * SECOND,
                rep_h=rep_h, rep_dz=rep_dz,
                c_z2=rep_h @ (aW + resW).T + np.abs(h1) @ resW.T + hl_max @ np.abs(Wl).T + acc_f,       # the contractions alone
                c_dh1=rep_dz @ (aW + resW) + np.abs(dz2) @ resW + dzl_max @ np.abs(Wl) + acc_b)


def fp32_grade(case, X, E):
    """The three contractions' own bounds (representation, dropped lo.lo, accumulation; nothing propagated) over the bound of a plain
    fp32 evaluation of the same sum (64 fmas: 64 u sum|terms|; the outer product of one term: u |dz2 h1|), on the observed terms with a
    live gradient.  -> {'z2' | 'dH1' | 'dW2': (median, 95th percentile)} over the entries (the maximum belongs to an entry whose exact
    value happens to vanish); about 1 is "fp32-grade"."""
    live = X['obs'] & (X['d_o'] != 0)
    if not live.any():
        return {}
    aW = np.abs(f64(case['W2']))
    out = {}
    for name, c, plain in (('z2', E['c_z2'], H * U_ * (np.abs(X['h1']) @ aW.T)), ('dH1', E['c_dh1'], H * U_ * (np.abs(X['dz2']) @ aW))):
        ok = live[..., None] & (plain > 0)
        if ok.any():
            r = c[ok] / plain[ok]
            out[name] = (float(np.median(r)), float(np.percentile(r, 95)))
    dz, h = np.abs(X['dz2'][live]), np.abs(X['h1'][live])
    prod = dz[:, :, None] * h[:, None, :]
    c = E['rep_dz'][live][:, :, None] * h[:, None, :] + dz[:, :, None] * E['rep_h'][live][:, None, :] \
        + E['dzl'][live][:, :, None] * E['hl'][live][:, None, :] + 6 * U_ * nominal(E['dzh'][live])[:, :, None] * nominal(E['hh'][live])[:, None, :]
    ok = prod > 0
    if ok.any():
        r = c[ok] / (U_ * prod[ok])
        out['dW2'] = (float(np.median(r)), float(np.percentile(r, 95)))
    return out


def record_bounds(case, X, lay, given=False):
    """Bounds of every record entry (and of prob) against records(X, lay, scheme=False); given: see term_bounds (GIVEN only)."""
    E = term_bounds(case, X, given)
    bnd = {k: np.zeros(s) for k, s in lay.shapes.items()}
    bnd['prob'] = E['p']
    bnd['dL'] = E['dl']
    absl = np.abs(X['l'])
    for c, ib, w, ps, it in _wave_sets(lay, None):
        wid = lay.wave_id(c, ib, w)
        if not len(ps) or not len(it):
            continue
        sel = np.ix_(ps, it)
        ch = (len(ps) + 6) * U_ * SECOND
        bnd['ll_part'][wid] = E['ll'][sel].sum() + ch * np.abs(X['ll'][sel]).sum()
        bnd['dvec_part'][wid, 0] = E['dz2'][sel].sum((0, 1)) + ch * np.abs(X['dz2'][sel]).sum((0, 1))
        doh = X['d_o'][sel][..., None] * X['h2'][sel]
        bnd['dvec_part'][wid, 1] = (np.abs(X['h2'][sel]) * E['d_o'][sel][..., None] + np.abs(X['d_o'][sel])[..., None] * E['h2'][sel]).sum((0, 1)) \
            + ch * np.abs(doh).sum((0, 1))
        bnd['dvec_part'][wid, 2] = (E['dz1'][sel] * absl[sel][..., None]).sum((0, 1)) + ch * np.abs(X['dz1'][sel] * absl[sel][..., None]).sum((0, 1))
        bnd['dvec_part'][wid, 3, 0] = E['d_o'][sel].sum() + ch * np.abs(X['d_o'][sel]).sum()
        # dW2: representation and propagation per term, the dropped lo x lo, and the accumulation pair by pair
        r2 = lambda a: a[sel].reshape(-1, H)
        e_w = r2(E['dzr']).T @ (np.abs(r2(X['h1'])) + r2(E['h1'])) + np.abs(r2(X['dz2'])).T @ r2(E['h1']) + r2(E['dzl']).T @ r2(E['hl'])
        tot, run_ = np.zeros((H, H)), np.zeros((H, H))
        for a, b in lay.pairs(c):
            pp = [a] if b is None else [a, b]
            ss = np.ix_(pp, it)
            q2 = lambda k: E[k][ss].reshape(-1, H)
            for A_, B_ in ((q2('dzh'), q2('hh')), (q2('dzh'), q2('hlo')), (q2('dzlo'), q2('hh'))):
                S = nominal(A_).T @ nominal(B_)
                m = (A_ != 0).astype(np.float64).T @ (B_ != 0).astype(np.float64)
                run_ = run_ + S
                tot = tot + np.maximum(m - 1, 0) * S + (m > 0) * run_
        bnd['dW2_part'][wid] = e_w + 2 * U_ * SECOND * tot
        real = it[:len(lay.wave_items(ib, w))]
        rs = np.ix_(ps, real)
        bnd['dU_part'][c][real] = E['dz1'][rs].sum(0) + ch * np.abs(X['dz1'][rs]).sum(0)
        bnd['dguess_part'][c][real] = E['dgs'][rs].sum(0) + ch * np.abs(X['dgs'][rs]).sum(0)
        for p in ps:
            bnd['dV_part'][4 * ib + w, p] = E['dz1'][p][it].sum(0) + 4 * U_ * SECOND * np.abs(X['dz1'][p][it]).sum(0)
    return bnd, E


REC_OF =dict(prob='prob', ll='ll_part', dL='dL', dV='dV_part', dU='dU_part', dguess='dguess_part', dW2='dW2_part')
VEC_ROW = dict(db2=0, dw3=1, dw1=2, db3=3)


def observable(rec, name):
    return rec['dvec_part'][:, VEC_ROW[name]] if name in VEC_ROW else rec[REC_OF[name]]


def ratios(got, exact, bnd, X=None, names=OBSERVABLES):
    """Worst |got - exact| / bound per observable; an entry whose bound is zero has to equal its (exact) reference: else inf.
    prob, ll and the per-term records of excluded cells (3PL clamp band) are left out through X['excluded']."""
    out = {}
    for name in names:
        if name not in VEC_ROW and REC_OF[name] not in got:
            continue
        if name in VEC_ROW and 'dvec_part' not in got:
            continue
        g, e, b = (np.asarray(observable(r, name), np.float64) for r in (got, exact, bnd))
        err = np.abs(g - e)
        if X is not None and name in ('prob', 'dL') and X['excluded'].any():
            err = np.where(X['excluded'], 0.0, err)
        with np.errstate(divide='ignore', invalid='ignore'):
            r = np.where(b > 0, err / b, np.where(err == 0, 0.0, np.inf))
        out[name] = float(np.max(np.nan_to_num(r, nan=np.inf))) if r.size else 0.0      # (NaN: an entry the launch never wrote)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------
def _hostile(rng, shape, e_lo, e_hi):
    m = rng.choice(np.asarray(M.HOSTILE_MANTISSAS, np.uint32), size=shape)
    return M.from_bits(rng.choice([-1, 1], size=shape), rng.integers(e_lo, e_hi + 1, size=shape), m)


def masks(kind, lay, seed=0, where='first'):
    """The three mask layouts (module docstring of tests/test_gpu_decoder_cells.py) -> uint8 [B, I].
    term: one observed item per (person, 16-item wave group).  single: one observed term per (person chunk, wave), its person in the
    chunk's first pair, a later pair or the last pair (`where`), its lane running through every i16.  dense: 30 % missing."""
    B, I = lay.B, lay.I
    m = np.zeros((B, I), np.uint8)
    if kind == 'dense':
        return (np.random.default_rng([seed, 7]).random((B, I)) >= 0.3).astype(np.uint8)
    for ib in range(lay.n_ib):
        for w in range(4):
            it = lay.wave_items(ib, w)
            if not len(it):
                continue
            if kind == 'term':
                for p in range(B):
                    m[p, it[(5 * p + 3 * (4 * ib + w) + seed) % len(it)]] = 1
            else:
                for c, (lo, hi) in enumerate(lay.ranges):
                    if lo >= hi:
                        continue
                    n = hi - lo
                    j = {'first': min(seed & 1, n - 1), 'later': min(2 + (seed & 1), n - 1), 'last': n - 1, 'last0': (n - 1) & ~1}[where]
                    m[lo + j, it[(seed + 7 * c + 4 * ib + w) % len(it)]] = 1
    return m


def make_case(cls, B, I, seed, has_U=True, has_w1=False, resid=0.0, has_guess=False, hidden=H, force_L=False):
    """One seeded problem of class `cls` (CLASSES) -> dict of fp32 arrays U [I, 64] | None, V [B, 64], L [B, I] | None, guess [I] | None,
    w1 [64] | None, W2 [64, 64], b2, w3 [64], b3 (float), resid, resp [B, I], mask None (the test sets its layout's).  hidden < 64: the
    units from `hidden` on are zero (decoder._pad_hidden).  guess3 forces the residual link with a guess."""
    rng = np.random.default_rng([seed, CLASSES.index(cls)])
    n = lambda *s, sc=1.0: rng.standard_normal(s) * sc
    if cls == 'guess3':
        has_U, has_w1, resid, has_guess = True, False, 1.0, True
    hasl = has_w1 or resid != 0.0 or force_L         # (force_L: the logits are passed although nothing reads them but the records)
    U = n(I, H, sc=0.7)
    V = n(B, H, sc=0.7)
    W2, b2, w3, b3 = n(H, H, sc=0.18), n(H, sc=0.1), n(H, sc=0.25), float(np.float32(n(1, sc=0.1)[0]))
    L = n(B, I, sc=1.5)
    w1 = n(H, sc=0.5)
    guess = M.sigmoid(n(I))
    sgn = lambda *s: rng.choice([-1.0, 1.0], size=s)
    if cls == 'hostile':
        W2, U, V = _hostile(rng, (H, H), -5, -2), _hostile(rng, (I, H), -2, 0), _hostile(rng, (B, H), -2, 0)
    elif cls == 'small_w':
        W2 = sgn(H, H) * np.exp2(rng.uniform(-16, -10, (H, H)))
    elif cls == 'small_g':
        w3 = sgn(H) * np.exp2(rng.uniform(-18, -14.01, H))
    elif cls == 'large':
        U = sgn(I, H) * np.exp2(rng.uniform(5, 9, (I, H)))
        V = sgn(B, H) * np.exp2(rng.uniform(5, 9, (B, H)))
        W2 = sgn(H, H) * np.exp2(rng.uniform(-6, -2, (H, H)))
        w3 = n(H, sc=2.0 ** -9)
        w1 = n(H, sc=8.0)
    elif cls == 'elu0':
        U = sgn(I, H) * rng.uniform(0.05, 0.25, (I, H)) * 2.0 ** -20
        V = sgn(B, H) * rng.uniform(0.05, 0.25, (B, H)) * 2.0 ** -20
        w1 = sgn(H) * rng.uniform(0.01, 0.05, H) * 2.0 ** -20
        W2 = sgn(H, H) * rng.uniform(0.001, 0.01, (H, H))
        b2 = sgn(H) * rng.uniform(0.05, 0.5, H) * 2.0 ** -20
    elif cls == 'zero':
        W2 = np.zeros((H, H))
    if not has_U:
        U = None
    if hidden < H:
        for t in (U, V, b2, w3, w1):
            if t is not None:
                t[..., hidden:] = 0.0
        W2[hidden:, :] = 0.0
        W2[:, hidden:] = 0.0
    f = lambda t: None if t is None else np.ascontiguousarray(t, np.float32)
    case = dict(cls=cls, U=f(U), V=f(V), L=f(L) if hasl else None, guess=f(guess) if has_guess else None, w1=f(w1) if has_w1 else None,
                W2=f(W2), b2=f(b2), w3=f(w3), b3=b3, resid=float(resid), mask=None,
                resp=rng.integers(0, 2, (B, I)).astype(np.float32))
    if cls == 'cancel':
        # all terms near one point (u0 + v0) with b2 = -W2.h1 there + a small rest: sum|W h| / |z2| >= 1e3 on every term
        u0, v0 = n(H, sc=0.7), n(H, sc=0.7)
        if has_U:
            case['U'] = f(u0[None, :] + n(I, H, sc=2e-5))
        case['V'] = f((v0 if has_U else v0 + u0)[None, :] + n(B, H, sc=2e-5))
        if hasl:
            case['L'] = f(n(B, I, sc=2e-5))
        W = f64(case['W2'])
        h0 = elu(f64(case['V'])[0] + (f64(case['U'])[0] if has_U else 0.0))
        s_abs = np.abs(W) @ np.abs(h0)
        case['b2'] = f(-(W @ h0) + sgn(H) * rng.uniform(2e-4, 6e-4, H) * s_abs)
    if cls == 'guess3':
        # the residual logit places p at both clamp values: 1 - p = 12 ... 32 eps32 (ordinary guesses) and p = eps32 e^(+-0.05 ... 0.5) (tiny ones)
        kind = rng.integers(0, 100, I)
        gam = rng.uniform(-2.0, 1.0, I)
        lo_side = kind >= 45
        gam[lo_side] = rng.choice([-22.0, -30.0], int(lo_side.sum()))
        c = M.sigmoid_rel(gam)
        sq = rng.choice([12.0, 16.0, 24.0, 32.0], I) * EPS32 / (1.0 - c)      # (24 u and more from 1: the mixture's own bound is 11 u)
        target = np.log((1.0 - sq) / sq)
        target[lo_side] = -M.LOGIT_LO + rng.choice([0.05, 0.1, 0.5, -0.05, -0.1, -0.5], int(lo_side.sum()))
        case['guess'] = f(c)
        case['L'] = np.zeros((B, I), np.float32)
        net = terms(case, scheme=False)['o']
        case['L'] = f(target[None, :] - net)
    return case


def with_mask(case, mask):
    return dict(case, mask=np.ascontiguousarray(mask, np.uint8))
