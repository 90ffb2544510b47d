"""TEST INFRASTRUCTURE ONLY -- the narrow-row kernel (csrc/vibo_narrow.hip) restated twice: an fp64 reference with an a-priori bound per
output entry, and a numpy-float32 emulation of the kernel's statements (an fma is one rounding) that has to stay inside those bounds.

The constants of oracle/split_model.py are imported, not copied.  u = 2^-24 (one round-to-nearest fp32 operation: at most u of its
result); a hardware transcendental (v_exp_f32, v_log_f32, v_rcp_f32, v_rsq_f32) is taken at 1 ulp = 2 u.

Running bounds.  The per-person part is written with `V`: a pair (v, e) of the exact fp64 value of an expression on the fp32 inputs
and a bound e >= |fp32 result - v|.  add / mul / rcp / rsq / log2 propagate e through the exact derivative (first order plus the
second-order product term) and add  n u (|v| + e)  for the n roundings of the statement.  Counts per statement of the kernel:

  line 93   es = __expf(s)            = exp2(s log2e): the fp32 log2e and the product, 2 u |s log2e| in the exponent = 2 u |s| of the
                                        result, plus the exp2 at 1 ulp:                                   (2 |s| + 2) u      [expf]
  line 94   tau = 1.0f / (es + eps)     one add, one correctly rounded division:                          2 roundings
  line 95   mt = m tau                  1
  line 96   te = tau tau es             2
  line 99   prior_w = 1.0f / (1.0f + 1e-8f) is 1.0f in fp32; the reference's 1 / (1 + 1e-8) differs by 1e-8 < u:   1 (C_PRIOR)
  line 207  lam = n0 tau0 + n1 tau1     two products and an add (or one product and an fma):             3, counts exact (<= 128)
  line 208  smu = n0 mt0 + n1 mt1       3
  line 209  lam = fma(I - nobs, prior_w, lam)                                                             1 (+ C_PRIOR on the term)
  line 211  inv_lam = 1.0f / lam        1
  line 212  amu = smu inv_lam           1
  line 213  sig = fast_rsq(lam)         2 (1 ulp)
  line 214  thv = amu + sig eps         2 (1 as an fma)
  line 217  alv = -kLn2 fast_log2(lam)  log2 at 1 ulp: 2; the fp32 ln 2 and the product: 2
  line 221  s_kl += -0.5 (1 + alv - amu amu - inv_lam)       amu amu: 1, three adds: 3; the halving is exact
  line 222  s_logq0 += -0.5 kLog2Pi - 0.5 alv - 0.5 eps eps  the fp32 log 2 pi: 1, eps eps: 1, two adds: 2
  line 223  s_logp += -0.5 kLog2Pi - 0.5 thv thv             1 + 1 + 1
  line 310  g0 = row16_sum(gth[ed]), gth = fma chain over the lane's IL items: IL + 4 (four DPP steps); na = -a log2e: 2;
  line 313  gz0 = g0 kLn2: 2.       -> d LL / d theta:  sum_i dg |a| + (IL + 8) u sum_i |g a|                           [theta_bound]
  line 316  h = 0.5 sig eps             1 (the halving is exact)
  line 319  glv[0] = gz0 h              1
  line 322  glv[1] = -0.5 (1 - inv_lam) 1
  line 331  nl = n_c inv_lam            1
  line 334  acc += (gmu nl) tau_c       1 (the fma's own rounding is the chain's)
  line 335  g_tau = nl (gmu (m_c - amu) - glv)               sub 1, mul 1, sub 1, mul 1
  line 336  acc += -g_tau te_c          (chain)
The sums over persons and cells then carry a CHAIN term  c u sum|terms|  counted from the kernel's reduction:
  item gradients   c = n_u + 2 + 4 + 1: one accumulate per unit of the wave (n_u = units per wave, units_per_wave), put()'s two
                   __shfl_xor adds, the `t += sm.item[w]` over four waves, one rounding of vibo_finalize.hpp's fp64 record sum;
  table gradients  c = n_u + 16 + 1: one fma per unit, `t += sm.tred[w][k][16 gg + a]` over 4 x 4, the record sum;
  S_KL, S_LOGQ0, S_LOGP   c = n_u + 6 + 4 + 1: one add per unit, wave_total's six butterfly steps, four waves, the record sum.
A sum with ONE nonzero term is exact whatever the chain (adding zero never rounds): the one-observer layouts see single cells.

Cells.  The per-cell arithmetic is the VALU row-split kernel's: split_model.cell_bound(..., fp32=True) for the logit, g_bound
(C_SIGMA; 3PL C_SIGMA3) for g = d ll / d logit.  d LL / d a sums fma(th, gl, acc): no rounding of its own beyond the chain.
3PL guess gradient: the kernel forms `common` = g / sigmoid(l) and accumulates fma(common, gs, acc_g): the exact cell term is
gc = g c / sigmoid(l), so its bound is g's evaluation bound times that factor F = c / sigmoid(l):
    |d gc| <= |d gc / d l| E + F E^2 + F C_SIGMA3 u.
S_LL.  Per chunk of four cells: exp2 (2 u), 1 + e (1), three products (3), log2 (2), the fp32 ln 2 and its product (2): C_LL = 10;
`s_log += fast_log2(prod)` NC times per unit.  1PL / 2PL: every unobserved or idle cell of a lane (missing, past the row's end, in a
row past the matrix' end) enters s_log as an exact 1.0 that `s_log - (float)unobs` takes back out; while it is in, the lane's
roundings are relative to a sum that holds it, so a lane with at least one observed cell costs
    (NC n_u + 1) u (ln 2 [unobserved and idle cells of the lane] + sum|ll| of the lane)
and a lane without one sums small integers exactly.  The residuals then go through wave_total, four waves and the record sum:
    |S_LL - exact| <= sum (|g| E + E^2) + (C_LL + 6 + 4 + 1) u sum|ll| + sum over lanes of the term above.
3PL multiplies 1.0 for an unobserved cell: no absolute term.

emulate() follows the kernel statement by statement in float32 (lane partial sums of IL items, the 16-lane tree, one row per
(wave, row group) and unit, the fixed-order epilogue, fp64 over the records) with switches for the mutations the bounds have to
reject (MUTATIONS).  Transcendentals are the correctly rounded ones; the hardware's may differ by an ulp, which the bounds allow.
"""
import numpy as np

from oracle import split_model as M
from oracle.split_model import C_SIGMA, C_SIGMA3, LN2, LOG2E32, LOGIT_HI, LOGIT_LO, EPS32, U, f32, sigmoid

POE_EPS = float(np.float32(1e-8))                    # kPoeEps
LOG_2PI = 1.8378770664093453
C_PRIOR = 1.0
C_LL = 10.0
MUTATIONS = ('tail', 'swap_n', 'no_prior', 'guess_row', 'drop_group')
F = np.float32
D = np.float64


# ---------------------------------------------------------------------------------------------------------------------------
# launch geometry (vibo_planner.hip narrow_blocks, vibo_launch.hpp narrow_waves_per_simd)
# ---------------------------------------------------------------------------------------------------------------------------
def template_width(A):
    return 1 if A <= 1 else 2 if A <= 2 else 4


def items_per_lane(I):
    return 4 if I <= 64 else 8


def grid_blocks(B, A, I, irt, want_grad, num_cu):
    at, il = template_width(A), items_per_lane(I)
    g3 = irt == 3 and want_grad
    wps = (3 if (g3 and il == 8) else 4) if at == 1 else ((4 if il == 4 else 3) if at == 2 else (3 if il == 4 else 2))
    return max(1, min(num_cu * wps, 1020, (B + 15) // 16))


def units_per_wave(B, grid):
    n_units, n_waves = (B + 3) // 4, 4 * grid
    return (n_units + n_waves - 1) // n_waves


# ---------------------------------------------------------------------------------------------------------------------------
# running error bounds
# ---------------------------------------------------------------------------------------------------------------------------
class V:
    """(v, e): exact fp64 value and a bound of |fp32 result - v|."""
    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, D)
        self.e = np.broadcast_to(np.asarray(e, D), self.v.shape) if np.ndim(e) <= self.v.ndim else np.asarray(e, D)

    def __getitem__(self, k):
        return V(self.v[k], np.broadcast_to(self.e, self.v.shape)[k])

    def __neg__(self):
        return V(-self.v, self.e)


def _V(x):
    return x if isinstance(x, V) else V(x)


def _round(v, e, n):
    return V(v, e + n * U * (np.abs(v) + e))


def add(a, b, n=1):
    a, b = _V(a), _V(b)
    return _round(a.v + b.v, a.e + b.e, n)


def mul(a, b, n=1):
    a, b = _V(a), _V(b)
    return _round(a.v * b.v, np.abs(a.v) * b.e + np.abs(b.v) * a.e + a.e * b.e, n)


def rcp(a, n=1):
    return _round(1.0 / a.v, a.e / (np.abs(a.v) * np.maximum(np.abs(a.v) - a.e, 1e-300)), n)


def rsq(a):
    return _round(a.v ** -0.5, np.maximum(a.v - a.e, 1e-300) ** -0.5 - a.v ** -0.5, 2)


def log2(a):
    return _round(np.log2(a.v), np.log2(a.v / np.maximum(a.v - a.e, 1e-300)), 2)


def person_model(table, n0, n1, I_total, eps, drop_missing=False, gz0=None):
    """The per-person part (module docstring): table fp32 [2, 2A], answer counts n0 / n1 [B], eps fp32 [B, A], gz0 = V of d LL / d theta
    [B, A] (None: forward only).  -> dict of V: mu, logvar, theta, lam [B, A]; the per-(person, dim) terms kl, logq0, logp; with gz0 the
    table-gradient terms t[st][c][ms] [B, A] (head st, answer c, ms 0 = mean / 1 = logvar)."""
    table = np.asarray(f32(table), D)
    A = table.shape[1] // 2
    m, s = table[:, :A], table[:, A:]
    eps = np.asarray(f32(eps), D)
    n = [np.asarray(n0, D)[:, None], np.asarray(n1, D)[:, None]]
    nobs = n[0] + n[1]
    es = V(np.exp(s), (2.0 * np.abs(s) + 2.0) * U * np.exp(s))                  # line 93
    tau = rcp(add(es, POE_EPS), 1)                                              # line 94
    mt = mul(m, tau)                                                            # line 95
    te = mul(mul(tau, tau), es)                                                 # line 96
    lam = add(mul(n[0], tau[0][None, :]), mul(n[1], tau[1][None, :]), 1)        # line 207 (3 in all)
    smu = add(mul(n[0], mt[0][None, :]), mul(n[1], mt[1][None, :]), 1)          # line 208
    if not drop_missing:
        pr = (I_total - nobs) / (1.0 + 1e-8)
        lam = add(lam, V(pr, C_PRIOR * U * pr))                                 # lines 99, 209
    inv = rcp(lam)                                                              # line 211
    amu = mul(smu, inv)                                                         # line 212
    sig = rsq(lam)                                                              # line 213
    se = mul(sig, eps)
    thv = add(amu, se)                                                          # line 214
    alv = mul(log2(lam), V(-LN2, U * LN2))                                      # line 217
    half = lambda x: V(0.5 * x.v, 0.5 * x.e)
    kl = -half(add(add(add(1.0, alv), -mul(amu, amu)), -inv))                   # line 221
    c2pi = V(-0.5 * LOG_2PI, U * 0.5 * LOG_2PI)
    logq0 = add(add(c2pi, -half(alv)), V(-0.5 * eps * eps, U * 0.5 * eps * eps))          # line 222
    logp = add(c2pi, -half(mul(thv, thv)))                                      # line 223
    out = dict(mu=amu, logvar=alv, theta=thv, lam=lam, kl=kl, logq0=logq0, logp=logp)
    if gz0 is None:
        return out
    h = half(se)                                                                # line 316
    gmu = [gz0, amu]
    glv = [mul(gz0, h), -half(add(1.0, -inv))]                                  # lines 319, 322
    t = [[[None, None], [None, None]], [[None, None], [None, None]]]
    for c in range(2):
        nl = mul(n[c], inv)                                                     # line 331
        for st in range(2):
            t[st][c][0] = mul(mul(gmu[st], nl), tau[c][None, :], 0)             # line 334 (the fma rounds in the chain)
            g_tau = mul(nl, add(mul(gmu[st], add(m[c][None, :], -amu)), -glv[st]))        # line 335
            t[st][c][1] = mul(-g_tau, te[c][None, :], 0)                        # line 336
    out['t'] = t
    return out


def summed(term, c):
    """sum over persons of a V [B, A] -> (exact [A], bound [A]) with the chain c u sum|terms| (none for a single nonzero term)."""
    k = (term.v != 0).sum(0)
    return term.v.sum(0), term.e.sum(0) + np.where(k > 1, c * U * (np.abs(term.v) + term.e).sum(0), 0.0)


def expected(case, table, eps, theta, *, grid, drop_missing=False):
    """Every observable of one launch on `case` (split_model.make_case; theta: the fp32 sample the kernel returned) as
    name -> (reference, bound), plus 'nobs' (exact), 'excluded' / 'items' / 'persons' (3PL clamp exclusion: split_model.reference)
    and 'logit' -> (|l| <= 3 selector, sigmoid' there, bound) for the one-observer layouts."""
    irt, obs_all, resp_all = case['irt'], np.asarray(case['obs'], bool), case['resp']
    B, I = resp_all.shape
    A = case['a'].shape[1]
    IL, n_u = items_per_lane(I), units_per_wave(B, grid)
    NC = IL // 4
    theta_all = f32(theta)
    # the cell part on the rows that observe anything (a launch of 32 645 rows with one observer per item has at most 128 of them)
    act = np.flatnonzero(obs_all.any(1))
    sub = dict(case, theta=theta_all[act], resp=resp_all[act], obs=obs_all[act])
    obs, resp, theta = sub['obs'], sub['resp'], sub['theta']
    ref = M.reference(sub, theta)
    e_l = M.cell_bound(theta, case['a'], case['b'], irt, fp32=True)
    g, ag = ref['g'], np.abs(ref['g'])
    dg = np.where(obs, M.g_bound(ref['logit'], e_l, ref['dgdl'] if irt == 3 else None, C_SIGMA3 if irt == 3 else C_SIGMA), 0.0)
    dg = np.where(ref['live'] | ~obs, dg, 0.0)           # (a saturated cell's gradient is an exact zero on both sides)
    if irt != 3:
        # ... unless its exact logit lies within 20 bounds of a saturation threshold: fp32 may decide the other way, and the
        # gradient jumps by up to 1 there (dense launches only: no generated cell of the one-observer layouts comes near)
        near = obs & ((np.abs(ref['logit'] + LOGIT_LO) < 20 * e_l) | (np.abs(ref['logit'] - LOGIT_HI) < 20 * e_l))
        dg = dg + near
    t_abs, a_abs = np.abs(np.asarray(theta, D)), np.abs(np.asarray(case['a'], D))
    n_i = (g != 0).sum(0)
    c_item = n_u + 2 + 4 + 1
    chain_i = np.where(n_i > 1, c_item * U, 0.0)
    out = {'dLL/db': (ref['g_b'], dg.sum(0) + chain_i * ag.sum(0))}
    if irt != 1:
        out['dLL/da'] = (ref['g_a'], dg.T @ t_abs + chain_i[:, None] * (ag.T @ t_abs))
    if irt == 3:
        c = M.sigmoid_rel(np.asarray(case['gamma'], D))[None, :]
        Fc = c / sigmoid(np.clip(ref['logit'], -LOGIT_LO, LOGIT_LO))
        dgc = np.where(obs & ref['live'], ref['dgcdl'] * e_l + Fc * e_l ** 2 + Fc * C_SIGMA3 * U, 0.0)
        out['dLL/dguess'] = (ref['g_c'], dgc.sum(0) + chain_i * np.abs(ref['gc']).sum(0))
    gth_v, gth_e = np.zeros((B, A)), np.zeros((B, A))
    gth_v[act] = ref['g_theta'] if irt != 1 else np.repeat(g.sum(1, keepdims=True), A, 1)
    gth_e[act] = dg @ a_abs + (IL + 8) * U * (ag @ a_abs)
    gz0 = V(gth_v, gth_e)
    x1 = obs_all & (resp_all == 1)
    pm = person_model(table, (obs_all & ~x1).sum(1), x1.sum(1), I, eps, drop_missing, gz0)
    for k in ('mu', 'logvar', 'theta'):
        out[k] = (pm[k].v, pm[k].e)
    c_sc = n_u + 6 + 4 + 1
    for k, name in (('kl', 'S_KL'), ('logq0', 'S_LOGQ0'), ('logp', 'S_LOGP')):
        tv = pm[k]
        out[name] = (np.array([tv.v.sum()]), np.array([tv.e.sum() + c_sc * U * (np.abs(tv.v) + tv.e).sum()]))
    c_tab = n_u + 16 + 1
    for st in range(2):
        val, bnd = np.zeros((2, 2 * A)), np.zeros((2, 2 * A))
        for c in range(2):
            for ms in range(2):
                val[c, ms * A:(ms + 1) * A], bnd[c, ms * A:(ms + 1) * A] = summed(pm['t'][st][c][ms], c_tab)
        out[f'grad_table({st})'] = (val, bnd)
    # S_LL
    ll = np.abs(ref['ll'])
    slope = np.ones_like(g) if irt == 3 else ag
    b_ll = np.where(obs, slope * e_l + e_l ** 2, 0.0).sum() + (C_LL + 6 + 4 + 1) * U * ll.sum()
    if irt != 3:
        lane_obs = np.pad(obs, ((0, 0), (0, 16 * IL - I))).reshape(-1, 16, IL).sum(2)   # observed cells per (active row, lane)
        lane_ll = np.pad(ll, ((0, 0), (0, 16 * IL - I))).reshape(-1, 16, IL).sum(2)
        n_units = (B + 3) // 4
        chain_of = lambda r: ((r // 4) % (4 * grid)) * 4 + r % 4                       # (wave, row group) of a row
        ids, inv_ = np.unique(chain_of(act), return_inverse=True)
        c_obs, c_ll = np.zeros((ids.size, 16)), np.zeros((ids.size, 16))
        np.add.at(c_obs, inv_, lane_obs)
        np.add.at(c_ll, inv_, lane_ll)
        wave_of = ids // 4
        c_rows = (n_units - 1 - wave_of) // (4 * grid) + 1                              # rows (existing or not) of the chain
        idle = c_rows[:, None] * IL - c_obs
        b_ll += (np.where(c_obs > 0, (NC * n_u + 1) * U * (LN2 * idle + c_ll), 0.0)).sum()
    else:
        b_ll += (NC * n_u + 1) * U * ll.sum()
    out['S_LL'] = (np.array([ref['ll'].sum()]), np.array([b_ll]))
    out['nobs'] = float(obs_all.sum())
    excl = ref['excluded']
    out['excluded'], out['items'] = excl, ~excl.any(0)
    out['persons'] = np.array([not excl.any()])
    if 'p_obs' in case and irt != 3 and np.all(obs.sum(0) <= 1) and act.size:
        idx = np.arange(I)
        p_sub = np.minimum(np.searchsorted(act, case['p_obs']), act.size - 1)
        l = ref['logit'][p_sub, idx]
        sel = (np.abs(l) <= 3.0) & obs[p_sub, idx]
        sp = (sigmoid(l) * (1 - sigmoid(l)))[sel]
        el = e_l[p_sub, idx][sel]
        out['logit'] = (sel, sp, el + el ** 2 / sp + C_SIGMA * U / sp)
        out['logit_share'] = (int(sel.sum()), int(I))
    out['ref'] = ref
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the kernel's statements in float32
# ---------------------------------------------------------------------------------------------------------------------------
def fma(a, b, c):
    return (np.asarray(a, D) * np.asarray(b, D) + np.asarray(c, D)).astype(F)


def _fn(f, x):
    with np.errstate(all='ignore'):
        return f(np.asarray(x, D)).astype(F)


def _tree(v, axis):
    """Pairwise sum of neighbours along `axis` until one is left (the DPP / butterfly trees: every lane gets the same bits)."""
    v = np.moveaxis(v, axis, -1)
    while v.shape[-1] > 1:
        v = (v[..., 0::2] + v[..., 1::2]).astype(F)
    return v[..., 0]


def emulate(case, table, eps, **kw):
    with np.errstate(all='ignore'):                      # (a mutation may divide by a zero precision: the NaN is the finding)
        return _emulate(case, table, eps, **kw)


def _emulate(case, table, eps, *, drop_missing=False, num_cu=256, want_grad=True, mutate=None):
    """-> dict(mu, logvar, theta [B, A]; g_item [I, D]; g_table [2][2, 2A]; ll, kl, logq0, logp, nobs) in float32, grid included."""
    assert mutate is None or mutate in MUTATIONS
    irt, resp, obs = case['irt'], case['resp'], np.asarray(case['obs'], bool)
    B, I = resp.shape
    A = case['a'].shape[1]
    AT, IL = template_width(A), items_per_lane(I)
    NC, W = IL // 4, 16 * IL
    grid = grid_blocks(B, A, I, irt, want_grad, num_cu)
    n_waves = 4 * grid
    rows = 4 * ((B + 3) // 4)
    one = F(1)
    kLoS, kHiS = F(F(LOGIT_LO) * F(LOG2E32)), F(F(LOGIT_HI) * F(LOG2E32))
    kLn2 = F(LN2)
    tb = f32(table)
    m, s = tb[:, :A], tb[:, A:]
    es = _fn(np.exp, s)
    tau = (one / (es + F(POE_EPS))).astype(F)
    mt, te = (m * tau).astype(F), ((tau * tau).astype(F) * es).astype(F)
    w = np.zeros((rows, W), F)
    w[:B, :I] = np.where(obs, np.where(resp == 1, 1.0, -1.0), 0.0)
    if mutate == 'tail' and I & 3:
        w[:B, I:(I + 3) & ~3] = 1.0                      # padding cells of the tail chunk read as observed and right
    nobs = (w != 0).sum(1).astype(F)
    n1 = (w > 0).sum(1).astype(F)
    n0 = nobs - n1
    if mutate == 'swap_n':
        n0, n1 = n1, n0
    live = np.arange(rows) < B
    pw = F(0) if (drop_missing or mutate == 'no_prior') else (one / (one + F(POE_EPS))).astype(F)
    lam = fma(n1[:, None], tau[1][None], (n0[:, None] * tau[0][None]).astype(F))
    smu = fma(n1[:, None], mt[1][None], (n0[:, None] * mt[0][None]).astype(F))
    lam = fma((F(I) - nobs)[:, None], pw, lam)
    lam[~live] = 1.0
    with np.errstate(all='ignore'):
        inv = (one / lam).astype(F)
    amu = (smu * inv).astype(F)
    sig = _fn(lambda x: x ** -0.5, lam)
    e_c = np.zeros((rows, A), F)
    e_c[:B] = f32(eps)
    thv = fma(sig, e_c, amu)
    thv[~live] = 0.0
    alv = (-kLn2 * _fn(np.log2, lam)).astype(F)
    th = np.zeros((rows, AT), F)
    th[:, :A] = thv
    # items
    na, nb = np.zeros((W, AT), F), np.zeros(W, F)
    na[:I, :A] = F(LOG2E32) if irt == 1 else (-f32(case['a']) * F(LOG2E32)).astype(F)
    nb[:I] = (f32(case['b']) * F(LOG2E32)).astype(F)
    gs, om = np.zeros(W, F), np.zeros(W, F)
    if irt == 3:
        gs[:I] = (one / (one + _fn(np.exp, -f32(case['gamma'])))).astype(F)
        om[:I] = (one - gs[:I]).astype(F)
    l = np.broadcast_to(nb, (rows, W)).astype(F)
    for a in range(AT):
        l = fma(na[None, :, a], th[:, a:a + 1], l)
    common = np.zeros_like(l)
    if irt != 3:
        lc = np.clip(l, -kLoS, kLoS)
        eu = _fn(np.exp2, (-w * lc).astype(F))
        tt = (one + eu).astype(F)
        gl = (w * (eu * (one / tt).astype(F)).astype(F)).astype(F)
        gl[(l < -kLoS) | (l > kHiS)] = 0.0
        fac = tt
    else:
        e = _fn(np.exp2, -np.abs(l))
        rr = (one / (one + e).astype(F)).astype(F)
        er = (e * rr).astype(F)
        sp, sn = np.where(l >= 0, rr, er), np.where(l >= 0, er, rr)
        pr = fma(om[None], sp, gs[None])
        qr = (om[None] * sn).astype(F)
        pc = np.clip(pr, F(EPS32), F(1.0 - EPS32))
        arg = np.where(w > 0, pc, np.clip(qr, F(EPS32), F(1.0 - EPS32)))
        fac = np.where(w != 0, arg, one).astype(F)
        wlv = np.where(pr == pc, w, F(0))
        common = (((wlv * (one / arg).astype(F)).astype(F) * om[None]).astype(F) * sn).astype(F)
        gl = (common * sp).astype(F)
    prod = np.ones((rows, W // 4), F)
    for t4 in range(4):
        prod = (prod * fac[:, t4::4]).astype(F)          # (fac[:, 4 k + t4])
    slog_c = _fn(np.log2, prod).reshape(rows, 16, NC)
    # per-lane accumulators, one row per (wave, row group) and unit, in unit order
    unit = np.arange(rows) // 4
    wv, gg = unit % n_waves, np.arange(rows) % 4
    acc_b, acc_g = np.zeros((n_waves, 4, W), F), np.zeros((n_waves, 4, W), F)
    acc_a = np.zeros((n_waves, 4, W, AT), F)
    acc_t = np.zeros((n_waves, 4, 8, AT), F)
    s_log, unobs = np.zeros((n_waves, 4, 16), F), np.zeros((n_waves, 4, 16), F)
    s_kl, s_q0, s_lp = (np.zeros((n_waves, 4, AT), F) for _ in range(3))
    s_no = np.zeros((n_waves, 4), F)
    # d LL / d theta of the row: fma chain over the lane's items, then the 16-lane tree
    gth = np.zeros((rows, 16, AT), F)
    glr, nar = gl.reshape(rows, 16, IL), na.reshape(16, IL, AT)
    for t in range(IL):
        gth = fma(nar[None, :, t, :], glr[:, :, t, None], gth)
    gz0 = (_tree(gth, 1) * kLn2).astype(F)
    h = (F(0.5) * sig * e_c).astype(F)
    for r in range(rows):
        k = (wv[r], gg[r])
        for c in range(NC):
            s_log[k] = (s_log[k] + slog_c[r, :, c]).astype(F)
        if irt != 3:
            unobs[k] += IL - (w[r] != 0).reshape(16, IL).sum(1)
        if not live[r]:
            continue
        s_kl[k][:A] = (s_kl[k][:A] + F(-0.5) * (((one + alv[r]).astype(F) - (amu[r] * amu[r]).astype(F)).astype(F) - inv[r]).astype(F)).astype(F)
        s_q0[k][:A] = (s_q0[k][:A] + ((F(-0.5) * F(LOG_2PI) - F(0.5) * alv[r]).astype(F) - (F(0.5) * e_c[r] * e_c[r]).astype(F)).astype(F)).astype(F)
        s_lp[k][:A] = (s_lp[k][:A] + (F(-0.5) * F(LOG_2PI) - ((F(0.5) * thv[r]).astype(F) * thv[r]).astype(F)).astype(F)).astype(F)
        s_no[k] += nobs[r]
        if not want_grad:
            continue
        acc_b[k] = (acc_b[k] + gl[r]).astype(F)
        acc_a[k] = fma(th[r][None, :], gl[r][:, None], acc_a[k])
        acc_g[k] = fma(common[r], gs, acc_g[k])
        gmu = [gz0[r, :A], amu[r]]
        glv = [(gz0[r, :A] * h[r]).astype(F), (F(-0.5) * (one - inv[r]).astype(F)).astype(F)]
        for c, n_c in ((0, n0[r]), (1, n1[r])):
            nl = (n_c * inv[r]).astype(F)
            for st in range(2):
                acc_t[k][st * 4 + c * 2, :A] = fma((gmu[st] * nl).astype(F), tau[c], acc_t[k][st * 4 + c * 2, :A])
                g_tau = (nl * ((gmu[st] * (m[c] - amu[r]).astype(F)).astype(F) - glv[st]).astype(F)).astype(F)
                acc_t[k][st * 4 + c * 2 + 1, :A] = fma(-g_tau, te[c], acc_t[k][st * 4 + c * 2 + 1, :A])

    def blocks(per_wave):
        """[n_waves, ...] -> `t += x[w]` over the four waves of a workgroup from 0.f, then the fp64 record sum rounded once."""
        x = per_wave.reshape((grid, 4) + per_wave.shape[1:])
        t = np.zeros_like(x[:, 0])
        for q in range(4):
            t = (t + x[:, q]).astype(F)
        return t.astype(D).sum(0).astype(F)

    out = dict(mu=amu[:B], logvar=alv[:B], theta=thv[:B])
    sgn = kLn2 if irt == 3 else -kLn2
    lanes = lambda x: _tree(_tree(x, 2), 1)                      # wave_total: the lanes of a row group, then the four groups
    out['ll'] = blocks((sgn * lanes((s_log - unobs).astype(F))).astype(F))
    pad4 = lambda x: np.concatenate([x, np.zeros(x.shape[:2] + (4 - AT,), F)], 2) if AT < 4 else x
    out['kl'], out['logq0'], out['logp'] = (blocks(lanes(pad4(x))) for x in (s_kl, s_q0, s_lp))
    out['nobs'] = blocks(_tree(s_no, 1))
    if not want_grad:
        return out

    def put(acc):                                                # [n_waves, 4, ...] -> the wave's sum over its row groups
        if mutate == 'drop_group':
            acc = acc.copy()
            acc[:, 3] = 0.0
        return ((acc[:, 0] + acc[:, 1]).astype(F) + (acc[:, 2] + acc[:, 3]).astype(F)).astype(F)

    staged = np.zeros((AT + 2, W), F)
    if irt != 1:
        for a in range(AT):
            staged[a] = blocks(put(-acc_a[..., a]))
    staged[0 if irt == 1 else AT] = blocks(put(acc_b))
    if irt == 3:
        staged[AT + 1] = blocks(put(acc_g))
    n_rows = 1 if irt == 1 else A + 1 if irt == 2 else A + 2
    g_item = np.zeros((I, n_rows), F)
    for row in range(n_rows):
        srow = 0 if irt == 1 else row if (row < A or mutate == 'guess_row') else AT + (row - A)
        g_item[:, row] = staged[srow, :I]
    out['g_item'] = g_item
    tt_ = np.zeros((grid, 8, AT), F)                             # `t += sm.tred[w][k][16 gg + a]`, w outer, gg inner
    x = acc_t.reshape(grid, 4, 4, 8, AT)
    for q in range(4):
        for g_ in range(4):
            tt_ = (tt_ + x[:, q, g_]).astype(F)
    rec = tt_.astype(D).sum(0).astype(F)
    gt = [np.zeros((2, 2 * A), F), np.zeros((2, 2 * A), F)]
    for st in range(2):
        for c in range(2):
            for ms in range(2):
                gt[st][c, ms * A:(ms + 1) * A] = rec[st * 4 + c * 2 + ms, :A]
    out['g_table'] = gt
    return out


def ratios(exp, got, irt, A):
    """Worst |got - reference| / bound per observable of expected(): got = dict as emulate() returns (or the kernel's outputs in
    that form).  A bound of zero admits no error (inf).  -> dict name -> ratio."""
    items, persons = exp['items'], exp['persons']

    def worst(err, bnd, keep=None):
        err, bnd = np.abs(np.asarray(err, D)), np.asarray(bnd, D)
        if keep is not None:
            err, bnd = err[keep], bnd[keep]
        if err.size == 0:
            return 0.0
        if not np.all(np.isfinite(err)):
            return float('inf')
        zero = bnd == 0
        r = float((err[~zero] / bnd[~zero]).max()) if (~zero).any() else 0.0
        return float('inf') if (zero.any() and err[zero].max() > 0) else r

    out = {}
    for k in ('mu', 'logvar', 'theta'):
        out[k] = worst(np.asarray(got[k], D) - exp[k][0], exp[k][1])
    for k, name in (('ll', 'S_LL'), ('kl', 'S_KL'), ('logq0', 'S_LOGQ0'), ('logp', 'S_LOGP')):
        if exp['excluded'].any() and k == 'll':
            continue                                             # (a cell within 4 ulp of the clamp: its value is not asserted)
        out[name] = worst(np.asarray(got[k], D).reshape(1) - exp[name][0], exp[name][1])
    out['S_NOBS'] = 0.0 if float(got['nobs']) == exp['nobs'] else float('inf')
    if 'g_item' not in got:
        return out
    gi = np.asarray(got['g_item'], D)
    gb = gi[:, 0 if irt == 1 else A]
    out['dLL/db'] = worst(gb - exp['dLL/db'][0], exp['dLL/db'][1], items)
    if 'logit' in exp:
        sel, sp, bnd = exp['logit']
        out['logit'] = worst((gb - exp['dLL/db'][0])[sel] / sp, bnd)
    if irt != 1:
        out['dLL/da'] = worst(gi[:, :A] - exp['dLL/da'][0], exp['dLL/da'][1], items)
    if irt == 3:
        out['dLL/dguess'] = worst(gi[:, A + 1] - exp['dLL/dguess'][0], exp['dLL/dguess'][1], items)
    ok = bool(persons.all())                                     # (the table sums run over every person)
    for st in range(2):
        if ok or st == 1:
            out[f'grad_table({st})'] = worst(np.asarray(got['g_table'][st], D) - exp[f'grad_table({st})'][0], exp[f'grad_table({st})'][1])
    return out


def make_problem(cls, A, B, I, seed, shift=0, drop_missing=False, missing=None, unobserved=()):
    """-> (case, table fp32 [2, 2A], eps fp32 [B, A]): a seeded encoder table (means of a few units), eps != 0, and a class-`cls`
    case whose difficulties are set from the fp64 product of experts' theta on the case's own responses (which do not depend on
    theta: split_model.make_case).  missing: instead of one observer per item, that share of ALL cells is unobserved.  unobserved: items
    that lose their observer (every output they feed is then an exact zero)."""
    rng = np.random.default_rng([seed, 7])
    table = f32(rng.standard_normal((2, 2 * A)) * 0.7)
    table[:, :A] *= 3.0
    eps = f32(rng.standard_normal((B, A)))
    c0 = M.make_case(cls, A, B, I, seed, shift=shift)
    obs = c0['obs'] if missing is None else rng.random((B, I)) >= missing
    obs[:, list(unobserved)] = False
    x1 = obs & (c0['resp'] == 1)
    pm = person_model(table, (obs & ~x1).sum(1), x1.sum(1), I, eps, drop_missing)
    case = M.make_case(cls, A, B, I, seed, theta=f32(pm['theta'].v), shift=shift)
    assert np.array_equal(case['resp'], c0['resp'])
    case['obs'] = obs
    case['theta_oracle'] = pm['theta'].v
    return case, table, eps
