"""TEST INFRASTRUCTURE ONLY -- the three fallback ELBO kernels restated: the launch geometry (how many trips a workgroup or a wave
takes through its persistent loop), an a-priori bound per output entry, and a numpy-float32 emulation of each kernel's trip
structure that has to stay inside those bounds and leave them under every mutation of MUTATIONS.

  tiled          elbo_kernel<A, IRT, NW, SB, CMAX, GRAD>    csrc/vibo_elbo_kernel.hpp     (1PL / 2PL / 3PL, ability_dim <= 8)
  wave-per-row   row_kernel<A, IRT, CH, MK, GRAD>           csrc/vibo_row_kernel.hip      (1PL / 2PL, ability_dim <= 2)
  wave-per-person elbo_general_kernel<8 | 16>               csrc/vibo_general.hip         (plain and conditional posterior, planar flows,
                                                                                           1PL / 2PL / 3PL, REG_KL and REG_SAMPLED), and
                                                                                           encode_kernel (vibo_helpers.hip)

The running-bound class V, person_model, summed, the cell bounds and the problem generator are oracle/narrow_model.py's and
oracle/split_model.py's, imported.  u = 2^-24; a hardware transcendental (v_exp_f32, v_log_f32, v_rcp_f32, v_rsq_f32) is 1 ulp = 2 u
as there.

Per person (tiled: person_dim, lines 166-184 and 469-505; wave-per-row: lines 128-135 and 189-220).  Statement for statement the
narrow-row kernel's: tau = 1 / (__expf(s) + eps), lam = n0 tau0 + n1 tau1 (3), lam += nmiss * 1.0f (1; the product is exact),
inv_lam (1), amu (1), sig = fast_rsq (2), theta (2), alv = -kLn2 fast_log2(lam) (4), the three heads and the eight table-gradient
terms: narrow_model.person_model with the same counts, REG_KL.

Cells.
  wave-per-row   l = fma chain over A dims from nb (lines 149-151): the VALU kernel's count, split_model.cell_bound(fp32=True) =
                 (A + 5) u sum|terms|.
  tiled          L = v_mfma_f32_16x16x4_f32 over KK = ceil((A + 1) / 4) chunks (line 359).  The matrix pipe's rounding mode is not
                 documented and not measured here: ASSUMED 2 roundings per accumulate step and nonzero product, as
                 oracle/onehot_model.py takes it (C_MFMA): 2 (A + 1) for the A + 1 products, 2 for -a log2e (the fp32 log2e and the
                 product), 2 spare for the bias row: (2 A + 6) u sum|terms|.
  g = d ll / d l: split_model.g_bound (C_SIGMA; 3PL C_SIGMA3) as in the narrow model; the guess gradient likewise.
  S_LL per observed cell (lines 375-377 / 169-171): eu = exp2(-w lc) 2 u eu, tt = 1 + eu one rounding u tt, log2 2 u |log2 tt|, the
    fp32 ln 2 and its product 2 u: in nats at most (2 sigma + 1 + 4 |ll|) u <= (3 + 4 |ll|) u on top of |g| E + E^2.  3PL (lines
    380-389): e, rr, er, pr, the clamp: C_SIGMA3 u relative on the argument: (C_SIGMA3 + 4 |ll|) u.  An unobserved cell adds
    fma(0, x, s) = s: exact, no absolute term.

Chains c u sum|terms| (c = 0 for a sum with one nonzero term: adding zero never rounds), T = trips of the workgroup / wave:
  wave-per-row   item gradients   T + 4 + 1    one accumulate per trip (lines 177-179), red[0..3] (line 272), the fp64 record sum
                                               rounded once (vibo_finalize.hpp); a single-term d LL / d a still rounds its fma: 1
                 table heads      T + 4 + 1    one fma per trip (lines 218-220), four waves (line 252), the record sum
                 S_KL, ...        A T + 4 + 1  lane 0 adds A terms per trip
                 d LL / d theta   NI + 6 + 3   fma chain over the lane's NI = 4 CH items, wave_total, kLn2 and na's log2e
                 S_LL             NI T + 6 + 2 + 4 + 1
  tiled          item gradients   2 x 64 T + T + 1   16 MFMAs of 4 persons per tile at 2 roundings per product, `acc_item += cur`
                                               per trip (line 428), the record sum
                 table heads      T + 6 + 1    one fma per trip and lane (lines 503-505), wave_total, the record sum
                 S_KL, ...        DPW T + 6 + NW + 1
                 d LL / d theta   2 x 16 SB + NW + 4   MFMAs over the wave's 16 SB items, kLn2, `g0 += red[w]` over NW waves (482)
                 S_LL             16 SB T + 2 + 6 + NW + 1

Wave-per-person kernel: natural units and the device math library's expf / logf / log1pf / sqrtf.  No ulp figure for them is
stated in the ROCm headers or documents installed with the toolchain (the only figure found, 8192 ulp in opencl-c.h, belongs to the
half_ functions): ASSUMED 2 ulp = 4 u each (C_LIBM).  Statements:
  line 88    tau = 1 / (expf(s) + eps)        4 u es, the add, the division
  89-92      lam += tau | tau_prior           per lane ceil(I / 64) adds, wave_total 6: (K + 6) u lam
  90         smu = fma(m, tau, smu)           (K + 6) u sum|m tau|
  104-109    ilam = 1 / L (1), amu = S ilam (1), alv = logf(ilam) (4 u), sig = sqrtf(ilam) (4 u), th0 = amu + sig eps (2)
  158-161    l = fma chain from b: A u sum|terms|
  165-171    e = expf(-|lc|) 4 u, r = 1 / (1 + e) 2, sgm = r | e r 1, x - sgm 1: C_SIGMA_G = 8
  168        ll += x lc - max(lc, 0) - log1pf(e): (|l| + 7 + |ll|) u per cell on top of |g| E + E^2
  190-201    item gradients by atomics, LDS slab then global: (n - 1) u sum|terms| over the n nonzero terms, plus 1 for the flush
  213-215    heads: A adds per person, `s_kl += kl` per trip, one atomic per wave: (A + n - 1) u sum|terms|
  326-333    table terms: expf 4 u, tau 2, g_m three products, g_tau sub, mul, sub, two products, then three products
  173-185    3PL: see expected_general; 236, 277-283 REG_SAMPLED: gz[1] = theta_K, glv[1] = gz[1] h - 0.5
  82, 288-307  conditional posterior: the expert of cell (p, i) is table[x_pi, i]; the [2, I, 2A] table gradient takes one atomic per
             observed cell: person_model_cond
  119-139, 238-269  planar flows: flows_model (tanhf at C_LIBM; theta_K, ladj per person, S_LADJ, both flow-gradient heads)
encode_kernel (vibo_helpers.hip:318-360): the same sums with __expf at (2 |s| + 2) u, mu = S / L one division, logvar = logf(1 / L).
emulate_*: transcendentals are the correctly rounded ones; the bounds allow the hardware's and the library's ulps.  In the tiled
emulation the MFMA is an fp32 fma chain in k order.
"""
import numpy as np

from oracle import narrow_model as N
from oracle import split_model as M
from oracle.narrow_model import V, add, mul, rcp, person_model, summed, fma, _fn, _tree, POE_EPS, LOG_2PI, F, D
from oracle.split_model import C_SIGMA, C_SIGMA3, LN2, LOG2E32, LOGIT_HI, LOGIT_LO, EPS32, U, f32, sigmoid

C_LIBM = 4.0                   # expf / logf / log1pf / sqrtf of the device library: 2 ulp, ASSUMED (module docstring)
C_SIGMA_G = 8.0
TILE = 64                      # kTilePersons
MUTATIONS = ('stale_eps', 'no_toggle', 'reset_acc', 'second_set', 'tail_words', 'swap_n', 'no_prior', 'drop_last_row')
ACTS_ON = {'tiled': ('stale_eps', 'no_toggle', 'reset_acc', 'tail_words', 'swap_n', 'no_prior'),
           'wave-per-row': ('stale_eps', 'reset_acc', 'second_set', 'swap_n', 'no_prior'),
           'wave-per-person': ('stale_eps', 'reset_acc', 'swap_n', 'no_prior', 'drop_last_row')}


# ---------------------------------------------------------------------------------------------------------------------------
# launch geometry
# ---------------------------------------------------------------------------------------------------------------------------
def padded_ability_dim(A):                                   # vibo_params.hpp:15
    return 1 if A <= 1 else 2 if A <= 2 else 4 if A <= 4 else 8


def clamp_grid(num_cu, per_cu, persons, rows_per_wg):        # vibo_planner.hpp:23-27
    return max(1, min(num_cu * per_cu, (persons + rows_per_wg - 1) // rows_per_wg))


def tiled_plan(B, I, A, num_cu):
    """vibo_planner.hip plan_tiled (lines 288-315) -> dict(waves, SB, CMAX, lds_stride, lds_main, lds, per_cu, grid, n_tiles, trips)."""
    AT = padded_ability_dim(A)
    waves = 2 if I <= 144 else 4 if I <= 304 else 8 if I <= 512 else 16                          # line 292
    SB, CMAX = {2: (8, 1), 4: (8, 2), 8: (4, 2), 16: (4, 4)}[waves]                              # vibo_elbo_kernel.hpp:189
    stride = {16: 1040, 8: 528, 4: 304, 2: 144}[waves]                                           # vibo_params.hpp:12
    main_b = max(TILE * stride, waves * AT * 65 * 4, waves * 32)                                 # lines 294-297
    main_b = (main_b + 15) & ~15
    lds = 2 * main_b + 2 * (AT + 1) * 65 * 4 + waves * 16 * 20 * 4 + 2 * TILE * 4 + 4 * 2 * AT * 4       # lines 299-302
    lds = (lds + 255) & ~255
    per_cu = max(1, min(160 * 1024 // lds, 16 // waves))                                         # lines 304-308
    n_tiles = (B + TILE - 1) // TILE
    grid = min(num_cu * per_cu, n_tiles)                                                         # lines 309-310
    return dict(waves=waves, SB=SB, CMAX=CMAX, lds_stride=stride, lds_main=main_b, lds=lds, per_cu=per_cu, grid=grid, n_tiles=n_tiles,
                AT=AT, trips=trips_of(n_tiles, grid))


def trips_of(n_units, n_workers):
    """(fewest, most) trips of `for (u = id; u < n_units; u += n_workers)` over the workers that exist."""
    n_workers = max(1, n_workers)
    return n_units // n_workers, (n_units + n_workers - 1) // n_workers


def row_plan(B, I, num_cu):
    """vibo_planner.hip:416 `clamp_grid(num_cu, 2, B, 4)`; vibo_row_kernel.hip:294-296 CH; lines 228-234 the row loop."""
    grid = clamp_grid(num_cu, 2, B, 4)
    return dict(grid=grid, n_waves=4 * grid, CH=1 if I <= 256 else 2 if I <= 512 else 4, trips=trips_of(B, 4 * grid))


def general_plan(B, I, item_dim, want_grad, num_cu):
    """vibo_general.hip launch_elbo_general (lines 393-411): the LDS item slab up to 150 KiB, 4 / 2 / 1 workgroups per CU."""
    item_bytes = I * item_dim * 4
    in_lds = bool(want_grad and item_bytes <= 150 * 1024)                                        # line 396
    lds = item_bytes if in_lds else 0
    k = 1 if lds > 80 * 1024 else 2 if lds > 40 * 1024 else 4                                    # line 408
    grid = max(1, min((B + 3) // 4, num_cu * k))                                                 # lines 407-409
    return dict(grid=grid, n_waves=4 * grid, item_in_lds=in_lds, per_cu=k, trips=trips_of(B, 4 * grid))


def multi_trip_persons(kernel, I, A, num_cu, item_dim=None):
    """The issue's B of part (b): every workgroup / wave takes two trips, some a third (wave-per-row: a fifth), the last one ragged."""
    if kernel == 'tiled':
        return 2 * TILE * (num_cu * tiled_plan(1 << 30, I, A, num_cu)['per_cu']) + TILE + 5
    if kernel == 'wave-per-row':
        return 4 * (4 * 2 * num_cu) + 5
    return 2 * 4 * (num_cu * general_plan(1 << 30, I, item_dim, True, num_cu)['per_cu']) + 5


# ---------------------------------------------------------------------------------------------------------------------------
# bounds: tiled and wave-per-row (log2 units, the narrow model's per-person part)
# ---------------------------------------------------------------------------------------------------------------------------
def _consts(kernel, B, I, A, num_cu):
    if kernel == 'tiled':
        p = tiled_plan(B, I, A, num_cu)
        T, NW, SB = p['trips'][1], p['waves'], p['SB']
        DPW = (p['AT'] + NW - 1) // NW
        return dict(plan=p, e_l=(2 * A + 6) / (A + 5), c_item=2 * TILE * T + T + 1, c_one_a=2, c_tab=T + 7, c_sc=DPW * T + 6 + NW + 1,
                    c_th=2 * 16 * SB + NW + 4, c_ll=16 * SB * T + 2 + 6 + NW + 1)
    p = row_plan(B, I, num_cu)
    T, NI = p['trips'][1], 4 * p['CH']
    return dict(plan=p, e_l=1.0, c_item=T + 5, c_one_a=1, c_tab=T + 5, c_sc=A * T + 5, c_th=NI + 9, c_ll=NI * T + 13)


def expected(kernel, case, table, eps, theta, *, num_cu, drop_missing=False):
    """Every observable of one launch of the tiled or the wave-per-row kernel on `case` as name -> (reference, bound), in the form
    narrow_model.expected returns it (narrow_model.ratios reads both)."""
    assert kernel in ('tiled', 'wave-per-row')
    irt, obs_all, resp_all = case['irt'], np.asarray(case['obs'], bool), case['resp']
    B, I = resp_all.shape
    A = case['a'].shape[1]
    k = _consts(kernel, B, I, A, num_cu)
    theta_all = f32(theta)
    act = np.flatnonzero(obs_all.any(1))
    sub = dict(case, theta=theta_all[act], resp=resp_all[act], obs=obs_all[act])
    obs, theta = sub['obs'], sub['theta']
    ref = M.reference(sub, theta)
    e_l = k['e_l'] * M.cell_bound(theta, case['a'], case['b'], irt, fp32=True)
    g, ag = ref['g'], np.abs(ref['g'])
    dg = np.where(obs, M.g_bound(ref['logit'], e_l, ref['dgdl'] if irt == 3 else None, C_SIGMA3 if irt == 3 else C_SIGMA), 0.0)
    dg = np.where(ref['live'] | ~obs, dg, 0.0)
    if irt != 3:
        near = obs & ((np.abs(ref['logit'] + LOGIT_LO) < 20 * e_l) | (np.abs(ref['logit'] - LOGIT_HI) < 20 * e_l))
        dg = dg + near
    t_abs, a_abs = np.abs(np.asarray(theta, D)), np.abs(np.asarray(case['a'], D))
    n_i = (g != 0).sum(0)
    chain_i = np.where(n_i > 1, k['c_item'] * U, 0.0)
    chain_a = np.where(n_i > 1, k['c_item'] * U, k['c_one_a'] * U)
    out = {'dLL/db': (ref['g_b'], dg.sum(0) + chain_i * ag.sum(0))}
    if irt != 1:
        out['dLL/da'] = (ref['g_a'], dg.T @ t_abs + chain_a[:, None] * (ag.T @ t_abs))
    if irt == 3:
        c = M.sigmoid_rel(np.asarray(case['gamma'], D))[None, :]
        Fc = c / sigmoid(np.clip(ref['logit'], -LOGIT_LO, LOGIT_LO))
        dgc = np.where(obs & ref['live'], ref['dgcdl'] * e_l + Fc * e_l ** 2 + Fc * C_SIGMA3 * U, 0.0)
        out['dLL/dguess'] = (ref['g_c'], dgc.sum(0) + chain_a * np.abs(ref['gc']).sum(0))
    gth_v, gth_e = np.zeros((B, A)), np.zeros((B, A))
    gth_v[act] = ref['g_theta'] if irt != 1 else np.repeat(g.sum(1, keepdims=True), A, 1)
    gth_e[act] = dg @ a_abs + k['c_th'] * U * (ag @ a_abs)
    x1 = obs_all & (resp_all == 1)
    pm = person_model(table, (obs_all & ~x1).sum(1), x1.sum(1), I, eps, drop_missing, V(gth_v, gth_e))
    for name in ('mu', 'logvar', 'theta'):
        out[name] = (pm[name].v, pm[name].e)
    for key, name in (('kl', 'S_KL'), ('logq0', 'S_LOGQ0'), ('logp', 'S_LOGP')):
        tv = pm[key]
        out[name] = (np.array([tv.v.sum()]), np.array([tv.e.sum() + k['c_sc'] * U * (np.abs(tv.v) + tv.e).sum()]))
    for st in range(2):
        val, bnd = np.zeros((2, 2 * A)), np.zeros((2, 2 * A))
        for c in range(2):
            for ms in range(2):
                val[c, ms * A:(ms + 1) * A], bnd[c, ms * A:(ms + 1) * A] = summed(pm['t'][st][c][ms], k['c_tab'])
        out[f'grad_table({st})'] = (val, bnd)
    ll = np.abs(ref['ll'])
    slope = np.ones_like(g) if irt == 3 else ag
    c_eval = C_SIGMA3 if irt == 3 else 3.0
    out['S_LL'] = (np.array([ref['ll'].sum()]),
                   np.array([np.where(obs, slope * e_l + e_l ** 2 + (c_eval + 4 * ll) * U, 0.0).sum() + k['c_ll'] * U * ll.sum()]))
    out['nobs'] = float(obs_all.sum())
    excl = ref['excluded']
    if irt == 3:
        excl = excl | _window_only_cells(case, ref, obs)
    out['excluded'], out['items'], out['persons'] = excl, ~excl.any(0), np.array([not excl.any()])
    out['ref'], out['plan'] = ref, k['plan']
    sel = obs & (np.abs(ref['logit']) <= 3.0)
    out['logit_share'] = (int(sel.sum()), int(obs.sum()))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# bounds: wave-per-person (natural units, device math library, atomics)
# ---------------------------------------------------------------------------------------------------------------------------
def _window_only_cells(case, ref, obs):
    """3PL cells on which the fp64 oracles and the kernels disagree.  The kernels, like torch's autograd on p = c + (1 - c) sigmoid(l),
    stop a gradient only where p leaves [eps32, 1 - eps32]; split_model.reference (and vibo_table_ref) also stop it where the LOGIT
    leaves [-LOGIT_LO, LOGIT_HI], which differs in the guess gradient of a cell with a large guess.  No one-observer class generates
    such a cell; a dense launch may hold a few: they are left out like the cells next to a clamp value."""
    cg = sigmoid(np.asarray(case['gamma'], D))[None, :]
    p3 = cg + (1.0 - cg) * M.sigmoid_rel(ref['logit'])           # (the unclamped logit: what the kernel and torch form)
    return obs & ((ref['logit'] < -LOGIT_LO) | (ref['logit'] > LOGIT_HI)) & (p3 >= EPS32) & (p3 <= 1.0 - EPS32)


def _heads_in(gz0, gz1, reg, amu, th, il, h):
    """Lines 270-286: (gmu, glv) of the two heads from d head / d theta_0.  gz1 None: no flows, where gz[1] is 0 (REG_KL: 0 + amu is
    exact) or theta itself (REG_SAMPLED)."""
    half = lambda x: V(0.5 * x.v, 0.5 * x.e)
    if gz1 is None:
        if reg == 'kl':
            return [gz0, amu], [mul(gz0, h), -half(add(1.0, -il))]
        return [gz0, th], [mul(gz0, h), add(mul(th, h), -0.5)]
    if reg == 'kl':
        return [gz0, add(gz1, amu)], [mul(gz0, h), add(mul(gz1, h), -half(add(1.0, -il)))]
    return [gz0, gz1], [mul(gz0, h), add(mul(gz1, h), -0.5)]


def _vtanh(a):
    t = np.tanh(a.v)
    return _libm(t, np.minimum(a.e, (1.0 - t * t) * a.e + a.e ** 2))


def _vlog(a):
    return _libm(np.log(a.v), np.log(a.v / np.maximum(a.v - a.e, 1e-300)))


FLOW_EPS = float(np.float32(1e-8))


def flows_model(th0, flow, gz=None):
    """Planar flows of the wave-per-person kernel on V columns (lines 119-139 forward, 238-269 backward).  th0: V [B, A]; flow fp32
    [n, 2A + 1] = uhat | w | b per flow.  -> dict(theta_k V [B, A], ladj V [B]); with gz = (V, V) [B, A] (d head / d theta_K of the
    two heads) also gz0, gz1 [B, A] (d head / d theta_0) and terms[s][f] = V [B, 2A + 1], the per-person flow-gradient terms.
    Counts: aa A fmas; cwu A fmas on constants; tanhf, logf C_LIBM; 1 - t t 2; psi 2; |psi| + 1e-8 1; ladj += 1; theta += u t 1 per
    dim; backward: the reciprocal 1, -2 t cwu and its product with dl_dpsi 2, A fmas into g_t, g_c 1, g_a 1, each flow-gradient term
    two products and an add, gz += g_a w 1."""
    flow = np.asarray(f32(flow), D)
    B, A = th0.v.shape
    cols = [th0[:, a] for a in range(A)]
    zin, ts, psis = [], [], []
    ladj = V(np.zeros(B))
    for fp in flow:
        u, w, b = fp[:A], fp[A:2 * A], fp[2 * A]
        zin.append(list(cols))
        aa = V(np.full(B, b))
        for a in range(A):
            aa = add(mul(cols[a], w[a], 0), aa)
        cwu = V(np.dot(w, u), A * U * np.abs(w * u).sum())
        t = _vtanh(aa)
        psi = add(1.0, mul(add(1.0, -mul(t, t)), cwu))
        ladj = add(ladj, _vlog(add(V(np.abs(psi.v), psi.e), FLOW_EPS)))
        assert np.all(np.abs(psi.v) > 4 * psi.e), 'a flow next to its singularity: choose other parameters'
        ts.append(t), psis.append(psi)
        cols = [add(mul(t, u[a], 0), cols[a]) for a in range(A)]
    stack = lambda cs: V(np.stack([c.v for c in cs], 1), np.stack([np.broadcast_to(c.e, c.v.shape) for c in cs], 1))
    out = dict(theta_k=stack(cols), ladj=ladj)
    if gz is None:
        return out
    g = [[gz[s][:, a] for a in range(A)] for s in range(2)]
    terms = [[None] * len(flow) for _ in range(2)]
    for f in range(len(flow) - 1, -1, -1):
        u, w = flow[f][:A], flow[f][A:2 * A]
        t, psi = ts[f], psis[f]
        omt = add(1.0, -mul(t, t))
        cwu = V(np.dot(w, u), A * U * np.abs(w * u).sum())
        unit = mul(np.sign(psi.v), rcp(add(V(np.abs(psi.v), psi.e), FLOW_EPS)), 0)
        for s_ in range(2):
            dl = V(np.zeros(B)) if s_ == 0 else -unit
            g_t = mul(dl, mul(V(-2.0 * t.v, 2.0 * t.e), cwu))
            for a in range(A):
                g_t = add(mul(g[s_][a], u[a], 0), g_t)
            g_c, g_a = mul(dl, omt), mul(g_t, omt)
            cols_ = [add(mul(g[s_][a], t), mul(g_c, w[a])) for a in range(A)] + \
                    [add(mul(g_a, zin[f][a]), mul(g_c, u[a])) for a in range(A)] + [g_a]
            terms[s_][f] = stack(cols_)
            g[s_] = [add(mul(g_a, w[a], 0), g[s_][a]) for a in range(A)]
    out.update(gz0=stack(g[0]), gz1=stack(g[1]), terms=terms)
    return out


def _libm(v, e_in, n=C_LIBM):
    return V(v, e_in + n * U * (np.abs(v) + e_in))


def person_model_general(table, n0, n1, I_total, eps, drop_missing, gz0=None, reg='kl', encode=False, gz1=None):
    """vibo_general.hip lines 75-116, 209-216, 270-338 on the unconditional table (the conditional one: person_model_cond);
    reg 'kl' | 'sampled'; gz0 / gz1: d head / d theta_0 of the two heads (gz1 None: no flows, flows_model otherwise) -> dict of V as
    person_model.  encode: encode_kernel (vibo_helpers.hip:318-360), the same sums with __expf at (2 |s| + 2) u, mu = S / L one
    correctly rounded division, logvar = logf(1.0f / L)."""
    table = np.asarray(f32(table), D)
    A = table.shape[1] // 2
    m, s = table[:, :A], table[:, A:]
    eps = np.asarray(f32(eps), D)
    n = [np.asarray(n0, D)[:, None], np.asarray(n1, D)[:, None]]
    nobs = n[0] + n[1]
    K = (I_total + 63) // 64
    es = V(np.exp(s), ((2.0 * np.abs(s) + 2.0) if encode else C_LIBM) * U * np.exp(s))      # line 88 / encode_kernel line 340
    tau = rcp(add(es, POE_EPS), 1)
    nm = np.zeros_like(nobs) if drop_missing else I_total - nobs
    tp = 1.0 / (1.0 + 1e-8)
    lam_v = n[0] * tau.v[0][None] + n[1] * tau.v[1][None] + nm * tp
    lam = V(lam_v, n[0] * tau.e[0][None] + n[1] * tau.e[1][None] + nm * U * tp + (K + 6) * U * lam_v)        # lines 89-92, 102
    mt_abs = n[0] * np.abs(m[0] * tau.v[0])[None] + n[1] * np.abs(m[1] * tau.v[1])[None]
    smu = V(n[0] * (m[0] * tau.v[0])[None] + n[1] * (m[1] * tau.v[1])[None],
            n[0] * (np.abs(m[0]) * tau.e[0])[None] + n[1] * (np.abs(m[1]) * tau.e[1])[None] + (K + 6) * U * mt_abs)   # lines 90, 103
    il = rcp(lam)                                                                # line 104
    amu = mul(smu, rcp(lam, 0), 1) if encode else mul(smu, il)                   # line 105 / encode_kernel line 355: S / L
    lo = np.maximum(il.v - il.e, 1e-300)
    alv = _libm(np.log(il.v), np.log(il.v / lo))                                # line 106
    sig = _libm(np.sqrt(il.v), np.sqrt(il.v) - np.sqrt(lo))                     # line 107
    se = mul(sig, eps)
    th = add(amu, se)                                                            # line 109
    half = lambda x: V(0.5 * x.v, 0.5 * x.e)
    kl = -half(add(add(add(1.0, alv), -mul(amu, amu)), -il))                     # line 213
    c2pi = V(-0.5 * LOG_2PI, U * 0.5 * LOG_2PI)
    logq0 = add(add(c2pi, -half(alv)), V(-0.5 * eps * eps, U * 0.5 * eps * eps))
    logp = add(c2pi, -half(mul(th, th)))
    out = dict(mu=amu, logvar=alv, theta=th, kl=kl, logq0=logq0, logp=logp)
    if gz0 is None:
        return out
    h = half(se)                                                                 # line 273
    gmu, glv = _heads_in(gz0, gz1, reg, amu, th, il, h)
    tt = mul(mul(tau, tau), es)
    t = [[[None, None], [None, None]], [[None, None], [None, None]]]
    for c in range(2):
        for st in range(2):
            t[st][c][0] = mul(mul(mul(gmu[st], il), tau[c][None, :]), n[c])                                     # line 330
            g_tau = mul(mul(add(mul(gmu[st], add(m[c][None, :], -amu)), -glv[st]), il), n[c])                   # line 331
            t[st][c][1] = mul(-g_tau, tt[c][None, :])                                                           # line 333
    out['t'] = t
    return out


def person_model_cond(table, obs, x1, eps, drop_missing, gz0=None, reg='kl', encode=False, chain=0, gz1=None):
    """The conditional posterior of the wave-per-person kernel (table [2, I, 2A]: the expert of cell (p, i) is table[x_pi, i]; lines
    82-95 and 288-307) -> dict of V as person_model_general; with gz0 also 'table': [(value, bound) per head] of the [2, I, 2A]
    table gradient, every entry the atomic sum over the persons who answered item i with c (chain: (n - 1) + `chain` u)."""
    table = np.asarray(f32(table), D)
    A = table.shape[2] // 2
    I = table.shape[1]
    m, s = table[..., :A], table[..., A:]
    eps = np.asarray(f32(eps), D)
    W = [np.asarray(obs & ~x1, D), np.asarray(x1, D)]
    K = (I + 63) // 64
    es = V(np.exp(s), ((2.0 * np.abs(s) + 2.0) if encode else C_LIBM) * U * np.exp(s))
    tau = rcp(add(es, POE_EPS), 1)
    nm = np.zeros((obs.shape[0], 1)) if drop_missing else (I - obs.sum(1, keepdims=True)).astype(D)
    tp = 1.0 / (1.0 + 1e-8)
    lam_v = W[0] @ tau.v[0] + W[1] @ tau.v[1] + nm * tp
    lam = V(lam_v, W[0] @ tau.e[0] + W[1] @ tau.e[1] + nm * U * tp + (K + 6) * U * lam_v)
    mt = m * tau.v
    smu = V(W[0] @ mt[0] + W[1] @ mt[1],
            W[0] @ (np.abs(m[0]) * tau.e[0]) + W[1] @ (np.abs(m[1]) * tau.e[1]) + (K + 6) * U * (W[0] @ np.abs(mt[0]) + W[1] @ np.abs(mt[1])))
    il = rcp(lam)
    amu = mul(smu, rcp(lam, 0), 1) if encode else mul(smu, il)
    lo = np.maximum(il.v - il.e, 1e-300)
    alv = _libm(np.log(il.v), np.log(il.v / lo))
    sig = _libm(np.sqrt(il.v), np.sqrt(il.v) - np.sqrt(lo))
    se = mul(sig, eps)
    th = add(amu, se)
    half = lambda x: V(0.5 * x.v, 0.5 * x.e)
    kl = -half(add(add(add(1.0, alv), -mul(amu, amu)), -il))
    c2pi = V(-0.5 * LOG_2PI, U * 0.5 * LOG_2PI)
    logq0 = add(add(c2pi, -half(alv)), V(-0.5 * eps * eps, U * 0.5 * eps * eps))
    logp = add(c2pi, -half(mul(th, th)))
    out = dict(mu=amu, logvar=alv, theta=th, kl=kl, logq0=logq0, logp=logp)
    if gz0 is None:
        return out
    h = half(se)
    gmu, glv = _heads_in(gz0, gz1, reg, amu, th, il, h)
    act = np.flatnonzero(obs.any(1))
    bc = lambda x: V(x.v[act][:, None, :], np.broadcast_to(x.e, x.v.shape)[act][:, None, :])         # [n, 1, A]
    tt = mul(mul(tau, tau), es)                                                                      # line 304: tau tau es
    heads = []
    for st in range(2):
        val, bnd = np.zeros((2, I, 2 * A)), np.zeros((2, I, 2 * A))
        for c in range(2):
            sel = W[c][act][:, :, None]
            g_m = mul(mul(bc(gmu[st]), bc(il)), tau[c][None])                                        # line 300
            g_tau = mul(add(mul(bc(gmu[st]), add(m[c][None], -bc(amu))), -bc(glv[st])), bc(il))      # line 301
            g_s = mul(-g_tau, tt[c][None], 3)                                                        # line 304: three products
            n = sel.sum(0)
            for ms, g in ((0, g_m), (1, g_s)):
                v_, e_ = (sel * g.v).sum(0), (sel * g.e).sum(0)
                e_ = e_ + np.where(n > 1, (n - 1 + chain) * U * (sel * (np.abs(g.v) + g.e)).sum(0), 0.0)
                val[c, :, ms * A:(ms + 1) * A], bnd[c, :, ms * A:(ms + 1) * A] = v_, e_
        heads.append((val, bnd))
    out['table'] = heads
    return out


def expected_general(case, table, eps, theta, *, num_cu, drop_missing=False, want_grad=True, reg='kl', flow=None):
    """The wave-per-person kernel's observables as name -> (reference, bound): table [2, 2A], or [2, I, 2A] (the conditional
    posterior); 1PL / 2PL / 3PL; reg 'kl' | 'sampled'; flow fp32 [n, 2A + 1] or None -- with flows `theta` is theta_K (the sample the
    cells ran on) and ability_k, ladj, S_LADJ and grad_flow(0 | 1) are added.  3PL (lines 173-185), rho = 6 c / (1 - c) + 1 the relative error of 1 - guess in u (guess =
    1 / (1 + expf(-gamma)): 4 + 1 + 1): pr = fma(1 - guess, sp, guess) rho + 8, its reciprocal + 1, common = dll_dp (1 - guess) sn
    rho + 7 + 2, gl = common sp 7 + 1: (2 rho + 34) u on g; the guess gradient that bound times guess / sigmoid(l) as in the narrow
    model; the value logf(pc | qc): (rho + 9 + 4 |ll|) u."""
    irt, obs_all, resp_all = case['irt'], np.asarray(case['obs'], bool), case['resp']
    cond = np.ndim(table) == 3
    B, I = resp_all.shape
    A = case['a'].shape[1]
    Dm = 1 if irt == 1 else A + irt - 1
    plan = general_plan(B, I, Dm, want_grad, num_cu)
    T, K = plan['trips'][1], (I + 63) // 64
    theta_all = f32(theta)
    act = np.flatnonzero(obs_all.any(1))
    sub = dict(case, theta=theta_all[act], resp=resp_all[act], obs=obs_all[act])
    obs, theta = sub['obs'], sub['theta']
    ref = M.reference(sub, theta)
    t_abs, a_abs = np.abs(np.asarray(theta, D)), np.abs(np.asarray(case['a'], D))
    s_all = (t_abs.sum(1, keepdims=True) if irt == 1 else t_abs @ a_abs.T) + np.abs(np.asarray(case['b'], D))[None, :]
    e_l = A * U * s_all                                   # A fmas (1PL: adds) in natural units, no conversion
    g, ag = ref['g'], np.abs(ref['g'])
    if irt == 3:
        cg = sigmoid(np.asarray(case['gamma'], D))[None, :]
        rho = 6.0 * cg / (1.0 - cg) + 1.0
        dg = np.where(obs & ref['live'], M.g_bound(ref['logit'], e_l, ref['dgdl'], 2.0 * rho + 34.0), 0.0)
    else:
        dg = np.where(obs & ref['live'], M.g_bound(ref['logit'], e_l, None, C_SIGMA_G), 0.0)
        near = obs & ((np.abs(ref['logit'] + LOGIT_LO) < 20 * e_l) | (np.abs(ref['logit'] - LOGIT_HI) < 20 * e_l))
        dg = dg + near
    n_i = (g != 0).sum(0)
    chain_i = np.where(n_i > 1, n_i * U, 0.0)                                    # (n - 1) + the flush
    out = {'dLL/db': (ref['g_b'], dg.sum(0) + chain_i * ag.sum(0))}
    if irt != 1:
        out['dLL/da'] = (ref['g_a'], dg.T @ t_abs + (chain_i + U)[:, None] * (ag.T @ t_abs))      # -gl * th rounds once
    if irt == 3:
        cr = M.sigmoid_rel(np.asarray(case['gamma'], D))[None, :]
        Fc = cr / sigmoid(np.clip(ref['logit'], -LOGIT_LO, LOGIT_LO))
        dgc = np.where(obs & ref['live'], ref['dgcdl'] * e_l + Fc * e_l ** 2 + Fc * (2.0 * rho + 41.0) * U, 0.0)
        out['dLL/dguess'] = (ref['g_c'], dgc.sum(0) + (chain_i + U) * np.abs(ref['gc']).sum(0))
    gth_v, gth_e = np.zeros((B, A)), np.zeros((B, A))
    gth_v[act] = ref['g_theta'] if irt != 1 else np.repeat(g.sum(1, keepdims=True), A, 1)
    gth_e[act] = dg @ a_abs + (K + 6) * U * (ag @ a_abs)
    x1 = obs_all & (resp_all == 1)
    n_w = min(B, plan['n_waves'])
    post = (lambda **kw: person_model_cond(table, obs_all, x1, eps, drop_missing, reg=reg, **kw)) if cond else \
           (lambda **kw: person_model_general(table, (obs_all & ~x1).sum(1), x1.sum(1), I, eps, drop_missing, reg=reg, **kw))
    if flow is None:
        pm = post(gz0=V(gth_v, gth_e))
    else:
        # theta (the caller's) is theta_K, what the cells ran on; the flows are carried from the per-person model's theta_0
        p0 = post()
        g1 = flows_model(p0['theta'], flow)['theta_k'] if reg != 'kl' else V(np.zeros((B, A)))        # line 236: d(-log p(theta_K))
        fm = flows_model(p0['theta'], flow, (V(gth_v, gth_e), g1))
        pm = post(gz0=fm['gz0'], gz1=fm['gz1'])
        out['ability_k'] = (fm['theta_k'].v, fm['theta_k'].e)
        out['ladj'] = (fm['ladj'].v, fm['ladj'].e)
        la = fm['ladj']
        out['S_LADJ'] = (np.array([la.v.sum()]), np.array([la.e.sum() + (T + n_w) * U * (np.abs(la.v) + la.e).sum()]))
        for s_ in range(2):
            pairs = [summed(fm['terms'][s_][f], T + n_w + 1) for f in range(len(flow))]
            out[f'grad_flow({s_})'] = (np.stack([v for v, _ in pairs]), np.stack([e for _, e in pairs]))
        # S_LOGP is taken at theta_K (line 215)
        tk = fm['theta_k']
        half = lambda x: V(0.5 * x.v, 0.5 * x.e)
        pm['logp'] = add(V(-0.5 * LOG_2PI, U * 0.5 * LOG_2PI), -half(mul(tk, tk)))
    for name in ('mu', 'logvar', 'theta'):
        out[name] = (pm[name].v, pm[name].e)
    for key, name in (('kl', 'S_KL'), ('logq0', 'S_LOGQ0'), ('logp', 'S_LOGP')):
        tv = pm[key]
        out[name] = (np.array([tv.v.sum()]), np.array([tv.e.sum() + (A + T + n_w) * U * (np.abs(tv.v) + tv.e).sum()]))
    for st in range(2):
        if cond:
            out[f'grad_table({st})'] = pm['table'][st]
            continue
        val, bnd = np.zeros((2, 2 * A)), np.zeros((2, 2 * A))
        for c in range(2):
            for ms in range(2):
                val[c, ms * A:(ms + 1) * A], bnd[c, ms * A:(ms + 1) * A] = summed(pm['t'][st][c][ms], T + n_w)
        out[f'grad_table({st})'] = (val, bnd)
    ll, al = np.abs(ref['ll']), np.abs(ref['logit'])
    ev = (rho + 9.0 + 4.0 * ll) if irt == 3 else (np.minimum(al, LOGIT_LO) + 7 + ll)
    slope = np.ones_like(g) if irt == 3 else ag
    out['S_LL'] = (np.array([ref['ll'].sum()]),
                   np.array([np.where(obs, slope * e_l + e_l ** 2 + ev * U, 0.0).sum() + (K + T + 6 + n_w) * U * ll.sum()]))
    out['nobs'] = float(obs_all.sum())
    excl = ref['excluded'] | _window_only_cells(case, ref, obs) if irt == 3 else ref['excluded']
    out['excluded'], out['items'], out['persons'] = excl, ~excl.any(0), np.array([not excl.any()])
    out['ref'], out['plan'] = ref, plan
    sel = obs & (np.abs(ref['logit']) <= 3.0)
    out['logit_share'] = (int(sel.sum()), int(obs.sum()))
    return out


def expected_encode(case, table, *, drop_missing=False):
    """encode_kernel's mu and logvar per entry -> {'mu': (reference, bound), 'logvar': ...}."""
    obs, resp = np.asarray(case['obs'], bool), case['resp']
    x1 = obs & (resp == 1)
    zero = np.zeros((resp.shape[0], case['a'].shape[1]))
    if np.ndim(table) == 3:
        pm = person_model_cond(table, obs, x1, zero, drop_missing, encode=True)
    else:
        pm = person_model_general(table, (obs & ~x1).sum(1), x1.sum(1), resp.shape[1], zero, drop_missing, encode=True)
    return {k: (pm[k].v, pm[k].e) for k in ('mu', 'logvar')}


def emulate_encode(case, table, *, drop_missing=False):
    with np.errstate(all='ignore'):
        B, I = case['resp'].shape
        A = case['a'].shape[1]
        w = _codes(case, B, 64 * ((I + 63) // 64))
        tp = F(0) if drop_missing else (ONE / (ONE + F(POE_EPS))).astype(F)
        L, S = _poe_sums(w, np.where(w > 0, 1, 0), f32(table), I, A, tp)
        return dict(mu=(S / L).astype(F), logvar=_fn(np.log, (ONE / L).astype(F)))


def _item_tables(tb, A, W):
    """-> (m, tau, es) [2, W, A] per (answer, item): the conditional table padded to W items, or the unconditional one repeated."""
    tb = f32(tb)
    if tb.ndim == 2:
        tb = np.repeat(tb[:, None, :], W, 1)
    else:
        tb = np.concatenate([tb, np.zeros((2, W - tb.shape[1], 2 * A), F)], 1)
    m, es = tb[..., :A], _fn(np.exp, tb[..., A:])
    return m, (ONE / (es + F(POE_EPS))).astype(F), es


def _poe_sums(w, code, tb, I, A, tp):
    """Lines 79-103 of the wave-per-person kernel (encode_kernel lines 329-353): lane l sums items l, l + 64, ..., then wave_total."""
    rows, W = w.shape
    m, tau = _item_tables(tb, A, W)[:2]                    # [2, W, A]
    in_row = (np.arange(W) < I)[None, :]
    lam, smu = np.zeros((rows, 64, A), F), np.zeros((rows, 64, A), F)
    for k in range(W // 64):
        sl_ = slice(64 * k, 64 * k + 64)
        ob, cd, ir = (w[:, sl_] != 0)[..., None], code[:, sl_], in_row[:, sl_, None]
        it = np.arange(64 * k, 64 * k + 64)[None, :]
        tk = tau[cd, it]                                   # [rows, 64, A]
        lam = np.where(ob, (lam + tk).astype(F), np.where(ir, (lam + tp).astype(F), lam))
        smu = np.where(ob, fma(m[cd, it], tk, smu), smu)
    return _tree(lam, 1), _tree(smu, 1)


# ---------------------------------------------------------------------------------------------------------------------------
# the kernels' statements in float32
# ---------------------------------------------------------------------------------------------------------------------------
ONE = F(1)
K_LOS, K_HIS = F(F(LOGIT_LO) * F(LOG2E32)), F(F(LOGIT_HI) * F(LOG2E32))
K_LN2 = F(LN2)


def _ctab(table, A):
    tb = f32(table)
    m, s = tb[:, :A], tb[:, A:]
    es = _fn(np.exp, s)
    tau = (ONE / (es + F(POE_EPS))).astype(F)
    return m, tau, (m * tau).astype(F), ((tau * tau).astype(F) * es).astype(F)


def _codes(case, B_pad, I_pad):
    """w = +1 answered right / -1 wrong / 0 missing, zero padded to [B_pad, I_pad]."""
    resp, obs = case['resp'], np.asarray(case['obs'], bool)
    B, I = resp.shape
    w = np.zeros((B_pad, I_pad), F)
    w[:B, :I] = np.where(obs, np.where(resp == 1, 1.0, -1.0), 0.0)
    return w


def _posterior(w_cnt, I, eps, ctab, drop_missing, mutate, live):
    """person_dim / lines 122-136 of the row kernel on the counts of the code rows w_cnt."""
    m, tau, mt, te = ctab
    nobs = (w_cnt != 0).sum(1).astype(F)
    n1 = (w_cnt > 0).sum(1).astype(F)
    n0 = nobs - n1
    if mutate == 'swap_n':
        n0, n1 = n1, n0
    pw = F(0) if (drop_missing or mutate == 'no_prior') else (ONE / (ONE + F(POE_EPS))).astype(F)
    lam = fma(n1[:, None], tau[1][None], (n0[:, None] * tau[0][None]).astype(F))
    smu = fma(n1[:, None], mt[1][None], (n0[:, None] * mt[0][None]).astype(F))
    lam = fma((F(I) - nobs)[:, None], pw, lam)
    lam[~live] = 1.0
    inv = (ONE / lam).astype(F)
    amu = (smu * inv).astype(F)
    sig = _fn(lambda x: x ** -0.5, lam)
    th = fma(sig, eps, amu)
    th[~live] = 0.0
    alv = (-K_LN2 * _fn(np.log2, lam)).astype(F)
    return dict(n0=n0, n1=n1, nobs=nobs, lam=lam, inv=inv, amu=amu, sig=sig, th=th, alv=alv, eps=eps)


def _heads(P):
    """The per-(person, dim) terms of s_kl, s_logq0, s_logp (lines 476-478 / 195-197)."""
    kl = (F(-0.5) * (((ONE + P['alv']).astype(F) - (P['amu'] * P['amu']).astype(F)).astype(F) - P['inv']).astype(F)).astype(F)
    q0 = ((F(-0.5) * F(LOG_2PI) - F(0.5) * P['alv']).astype(F) - (F(0.5) * P['eps'] * P['eps']).astype(F)).astype(F)
    lp = (F(-0.5) * F(LOG_2PI) - ((F(0.5) * P['th']).astype(F) * P['th']).astype(F)).astype(F)
    return kl, q0, lp


def _table_terms(P, g0, ctab):
    """-> [rows, A, 8] pairs (factor, multiplicand) of the eight `acc_t = fmaf(x, y, acc_t)` of a row (lines 503-505 / 218-220)."""
    m, tau, mt, te = ctab
    h = (F(0.5) * P['sig'] * P['eps']).astype(F)
    gmu = [g0, P['amu']]
    glv = [(g0 * h).astype(F), (F(-0.5) * (ONE - P['inv']).astype(F)).astype(F)]
    x = np.zeros(g0.shape + (8,), F)
    y = np.zeros(g0.shape + (8,), F)
    for c, n_c in ((0, P['n0']), (1, P['n1'])):
        nl = (n_c[:, None] * P['inv']).astype(F)
        for st in range(2):
            x[..., st * 4 + c * 2] = (gmu[st] * nl).astype(F)
            y[..., st * 4 + c * 2] = tau[c][None]
            g_tau = (nl * ((gmu[st] * (m[c][None] - P['amu']).astype(F)).astype(F) - glv[st]).astype(F)).astype(F)
            x[..., st * 4 + c * 2 + 1] = -g_tau
            y[..., st * 4 + c * 2 + 1] = te[c][None]
    return x, y


def _items(case, AT, I_pad):
    """item_prep_kernel: [-a log2e | +log2e], b log2e, guess, 1 - guess; zero rows past I."""
    irt, I = case['irt'], case['b'].shape[0]
    A = case['a'].shape[1]
    na, nb, gs, om = np.zeros((I_pad, AT), F), np.zeros(I_pad, F), np.zeros(I_pad, F), np.zeros(I_pad, F)
    na[:I, :A] = F(LOG2E32) if irt == 1 else (-f32(case['a']) * F(LOG2E32)).astype(F)
    nb[:I] = (f32(case['b']) * F(LOG2E32)).astype(F)
    if irt == 3:
        gs[:I] = (ONE / (ONE + _fn(np.exp, -f32(case['gamma'])))).astype(F)
        om[:I] = (ONE - gs[:I]).astype(F)
    return na, nb, gs, om


def _cells(l, w, irt, gs, om):
    """The elementwise part (lines 368-397 of the tiled kernel; 163-173 of the row kernel give the same bits) ->
    (gl, the value fma'd into s_log with weight |w|, GG)."""
    if irt != 3:
        l2 = np.clip(l, -K_LOS, K_HIS)
        lc = np.minimum(l2, K_LOS)
        wg = np.where(l == l2, w, F(0))
        eu = _fn(np.exp2, (-w * lc).astype(F))
        tt = (ONE + eu).astype(F)
        gl = (wg * (eu * (ONE / tt).astype(F)).astype(F)).astype(F)
        return gl, _fn(np.log2, tt), np.zeros_like(gl)
    e = _fn(np.exp2, -np.abs(l))
    rr = (ONE / (ONE + e).astype(F)).astype(F)
    er = (e * rr).astype(F)
    sp, sn = np.where(l >= 0, rr, er), np.where(l >= 0, er, rr)
    pr = fma(om[None], sp, gs[None])
    qr = (om[None] * sn).astype(F)
    pc = np.clip(pr, F(EPS32), F(1.0 - EPS32))
    arg = np.where(w > 0, pc, np.clip(qr, F(EPS32), F(1.0 - EPS32))).astype(F)
    wl = np.where(pr == pc, w, F(0))
    common = (((wl * (ONE / arg).astype(F)).astype(F) * om[None]).astype(F) * sn).astype(F)
    return (common * sp).astype(F), _fn(np.log2, arg), (common * gs[None]).astype(F)


def _records(x):
    """[grid, ...] per-workgroup partial records -> the fp64 sum over them rounded once (vibo_finalize.hpp)."""
    return x.astype(D).sum(0).astype(F)


def _stale(x, n, mutate, on='stale_eps'):
    """Mutation: the unit a worker takes on a later trip reads `x` of its previous trip (n units earlier)."""
    if mutate != on or x.shape[0] <= n:
        return x
    y = x.copy()
    y[n:] = x[:-n]
    return y


def emulate(kernel, case, table, eps, **kw):
    with np.errstate(all='ignore'):
        return {'tiled': _emulate_tiled, 'wave-per-row': _emulate_row, 'wave-per-person': _emulate_general}[kernel](case, table, eps, **kw)


def _emulate_row(case, table, eps, *, drop_missing=False, num_cu=256, want_grad=True, mutate=None):
    assert mutate is None or mutate in ACTS_ON['wave-per-row']
    irt, (B, I), A = case['irt'], case['resp'].shape, case['a'].shape[1]
    p = row_plan(B, I, num_cu)
    nW, CH = p['n_waves'], p['CH']
    NI, W = 4 * CH, 256 * CH
    T = p['trips'][1]
    rows = T * nW
    live = np.arange(rows) < B
    w = _codes(case, rows, W)
    e_c = np.zeros((rows, A), F)
    e_c[:B] = f32(eps)
    if mutate == 'second_set':                            # process(xb, mb, epb, ...) handed the first set's row: odd trips
        odd = (np.arange(rows) // nW) % 2 == 1
        w[odd], e_c[odd] = w[np.flatnonzero(odd) - nW], e_c[np.flatnonzero(odd) - nW]
    e_c = _stale(e_c, nW, mutate)
    ctab = _ctab(table, A)
    P = _posterior(w, I, e_c, ctab, drop_missing, mutate, live)
    na, nb, gs, om = _items(case, A, W)
    l = np.broadcast_to(nb, (rows, W)).astype(F)
    for a in range(A):
        l = fma(na[None, :, a], P['th'][:, a:a + 1], l)
    gl, sl, _ = _cells(l, w, irt, gs, om)
    # lane `ln` of a wave owns items 4 (ln + 64 c) + j as t = 4 c + j
    lanes = lambda x: x.reshape(x.shape[0], CH, 64, 4).transpose(0, 2, 1, 3).reshape(x.shape[0], 64, NI)
    gl_l, sl_l, aw_l = lanes(gl), lanes(sl), lanes(np.abs(w))
    na_l = na.reshape(CH, 64, 4, A).transpose(1, 0, 2, 3).reshape(64, NI, A)
    gth = np.zeros((rows, 64, A), F)
    for t in range(NI):
        gth = fma(gl_l[:, :, t, None], na_l[None, :, t, :], gth)
    g0 = (_tree(gth, 1) * K_LN2).astype(F)
    kl, q0, lp = _heads(P)
    tx, ty = _table_terms(P, g0, ctab)
    s_log = np.zeros((nW, 64), F)
    acc_b, acc_a = np.zeros((nW, 64, NI), F), np.zeros((nW, 64, NI, A), F)
    acc_t = np.zeros((nW, A, 8), F)
    s_kl, s_q0, s_lp, s_no = (np.zeros(nW, F) for _ in range(4))
    for trip in range(T):
        r = slice(trip * nW, (trip + 1) * nW)
        lv = live[r]
        if mutate == 'reset_acc':
            s_log[:], acc_b[:], acc_a[:], acc_t[:], s_kl[:], s_q0[:], s_lp[:], s_no[:] = 0, 0, 0, 0, 0, 0, 0, 0
        for t in range(NI):
            s_log = np.where(lv[:, None], fma(aw_l[r, :, t], sl_l[r, :, t], s_log), s_log)
        for a in range(A):
            s_kl = np.where(lv, (s_kl + kl[r, a]).astype(F), s_kl)
            s_q0 = np.where(lv, (s_q0 + q0[r, a]).astype(F), s_q0)
            s_lp = np.where(lv, (s_lp + lp[r, a]).astype(F), s_lp)
        s_no = np.where(lv, s_no + P['nobs'][r], s_no)
        if want_grad:
            acc_b = np.where(lv[:, None, None], (acc_b + gl_l[r]).astype(F), acc_b)
            acc_a = np.where(lv[:, None, None, None], fma(gl_l[r][..., None], P['th'][r][:, None, None, :], acc_a), acc_a)
            acc_t = np.where(lv[:, None, None], fma(tx[r], ty[r], acc_t), acc_t)
    grid = p['grid']

    def wg(x):                                            # red[0] + red[1] + red[2] + red[3], then the record sum
        x = x.reshape((grid, 4) + x.shape[1:])
        return _records((((x[:, 0] + x[:, 1]).astype(F) + x[:, 2]).astype(F) + x[:, 3]).astype(F))

    out = dict(mu=P['amu'][:B], logvar=P['alv'][:B], theta=P['th'][:B])
    out['ll'] = wg((-(K_LN2 * _tree(s_log, 1)).astype(F)))
    out['kl'], out['logq0'], out['logp'], out['nobs'] = wg(s_kl), wg(s_q0), wg(s_lp), wg(s_no)
    if not want_grad:
        return out
    unl = lambda x: x.reshape((64, CH, 4) + x.shape[2:]).swapaxes(0, 1).reshape((W,) + x.shape[2:])      # lanes -> item order
    gb = unl(wg(acc_b))[:I]
    out['g_item'] = gb[:, None] if irt == 1 else np.concatenate([unl(wg(-acc_a))[:I], gb[:, None]], 1)
    rec = wg(acc_t)                                       # [A, 8]
    out['g_table'] = _g_table(rec, A)
    return out


def _g_table(rec, A):
    gt = [np.zeros((2, 2 * A), F), np.zeros((2, 2 * A), F)]
    for st in range(2):
        for c in range(2):
            for ms in range(2):
                gt[st][c, ms * A:(ms + 1) * A] = rec[:A, st * 4 + c * 2 + ms]
    return gt


def _emulate_tiled(case, table, eps, *, drop_missing=False, num_cu=256, want_grad=True, mutate=None):
    assert mutate is None or mutate in ACTS_ON['tiled']
    irt, (B, I), A = case['irt'], case['resp'].shape, case['a'].shape[1]
    p = tiled_plan(B, I, A, num_cu)
    NW, SB, AT, grid, T = p['waves'], p['SB'], p['AT'], p['grid'], p['trips'][1]
    I16 = (I + 15) & ~15
    NB = I16 // 16                                       # 16-item blocks that exist (i0 < I)
    rows = T * grid * TILE
    live = np.arange(rows) < B
    w = _codes(case, rows, I16)
    w_cnt = w.copy()                                     # (the counts are taken while packing: the padding never enters them)
    if mutate == 'tail_words' and I & 15:
        w[:, I:] = 1.0                                   # the row's padding to 16 items keeps whatever the tile held: observed, right
    e_c = np.zeros((rows, A), F)
    e_c[:B] = f32(eps)
    e_c = _stale(e_c, grid * TILE, mutate)
    if mutate == 'no_toggle':                            # every later trip decodes the code tile of the workgroup's first one
        w = np.tile(w[:grid * TILE], (T, 1))
    ctab = _ctab(table, A)
    P = _posterior(w_cnt, I, e_c, ctab, drop_missing, mutate, live)
    na, nb, gs, om = _items(case, AT, I16)
    th = np.zeros((rows, AT), F)
    th[:, :A] = P['th']
    valid = live.astype(F)
    l = np.zeros((rows, I16), F)                          # the MFMA as an fma chain in k order: theta_0 ... theta_{AT-1}, valid
    for a in range(AT):
        l = fma(th[:, a:a + 1], na[None, :, a], l)
    l = fma(valid[:, None], nb[None], l)
    gl, sl, GG = _cells(l, w, irt, gs, om)
    aw = np.abs(w)
    tl = lambda x: x.reshape((T, grid, TILE) + x.shape[1:])
    gl_t, sl_t, aw_t, GG_t, th_t, va_t = tl(gl), tl(sl), tl(aw), tl(GG), tl(th), tl(valid)
    # d LL / d theta per tile: wave wv sums its blocks wv, wv + NW, ... in the MFMA's order (call r, then k = g: item 4 g + r)
    order = [4 * g + r for r in range(4) for g in range(4)]
    red = np.zeros((T, grid, TILE, NW, AT), F)
    for wv in range(NW):
        acc = np.zeros((T, grid, TILE, AT), F)
        for b16 in range(wv, min(NB, NW * SB), NW):
            for j in order:
                i = 16 * b16 + j
                acc = fma(gl_t[..., i, None], na[i][None, None, None, :], acc)
        red[..., wv, :] = (acc * K_LN2).astype(F)
    g0 = np.zeros((T, grid, TILE, AT), F)
    for wv in range(NW):
        g0 = (g0 + red[..., wv, :]).astype(F)
    g0 = g0.reshape(rows, AT)[:, :A]
    kl, q0, lp = _heads(P)
    tx, ty = _table_terms(P, g0, ctab)
    klt, q0t, lpt, txt, tyt, lvt, not_ = tl(kl), tl(q0), tl(lp), tl(tx), tl(ty), tl(live), tl(P['nobs'])
    cols = AT + 2
    bt = np.zeros((T, grid, TILE, cols), F)                # B operand [theta | valid | 1 for the guess column]
    bt[..., :AT], bt[..., AT], bt[..., AT + 1] = th_t, va_t, 1.0
    acc_item = np.zeros((grid, I16, cols), F)
    s_log = np.zeros((grid, NW, 64), F)                    # lane (gq, nq)
    s_kl, s_q0, s_lp = (np.zeros((grid, TILE, AT), F) for _ in range(3))     # lane = person slot, dim a: wave a % NW's k-th dim
    acc_t = np.zeros((grid, TILE, A, 8), F)
    s_no = np.zeros((grid, TILE), F)
    persons = [16 * pt + 4 * g + r for pt in range(4) for r in range(4) for g in range(4)]
    for trip in range(T):
        if mutate == 'reset_acc':
            acc_item[:], s_log[:], s_kl[:], s_q0[:], s_lp[:], acc_t[:], s_no[:] = 0, 0, 0, 0, 0, 0, 0
        if want_grad:
            cur = np.zeros((grid, I16, cols), F)
            for q in persons:
                gcol = np.repeat(gl_t[trip, :, q, :, None], cols, 2)
                gcol[..., AT + 1] = GG_t[trip, :, q, :]
                cur = fma(gcol, bt[trip, :, q, None, :], cur)
            acc_item = (acc_item + cur).astype(F)
        for wv in range(NW):
            for s in range(SB):
                b16 = wv + NW * s
                if b16 >= NB:
                    continue
                for pt in range(4):
                    for r in range(4):
                        # lane (gq, nq): person 16 pt + 4 gq + r, item 16 b16 + nq
                        pp = 16 * pt + 4 * np.arange(4) + r
                        a_ = aw_t[trip][:, pp][:, :, 16 * b16:16 * b16 + 16].reshape(grid, 64)
                        s_ = sl_t[trip][:, pp][:, :, 16 * b16:16 * b16 + 16].reshape(grid, 64)
                        s_log[:, wv] = fma(a_, s_, s_log[:, wv])
        lv = lvt[trip]
        for a in range(A):
            s_kl[..., a] = np.where(lv, (s_kl[..., a] + klt[trip][..., a]).astype(F), s_kl[..., a])
            s_q0[..., a] = np.where(lv, (s_q0[..., a] + q0t[trip][..., a]).astype(F), s_q0[..., a])
            s_lp[..., a] = np.where(lv, (s_lp[..., a] + lpt[trip][..., a]).astype(F), s_lp[..., a])
        s_no = np.where(lv, s_no + not_[trip], s_no)
        if want_grad:
            acc_t = np.where(lv[..., None, None], fma(txt[trip], tyt[trip], acc_t), acc_t)

    def scalar(per_lane_by_wave):                          # [grid, NW, 64] -> wave_total, `t += scr[w]`, the record sum
        t = np.zeros(grid, F)
        wt = _tree(per_lane_by_wave, 2)
        for wv in range(NW):
            t = (t + wt[:, wv]).astype(F)
        return _records(t)

    def by_wave(x):                                        # [grid, TILE, AT] per (person slot, dim) -> the owner wave's lane sum
        y = np.zeros((grid, NW, TILE), F)
        for a in range(A):                                 # a = wave + NW k: k ascending within a wave
            y[:, a % NW] = (y[:, a % NW] + x[..., a]).astype(F) if a >= NW else x[..., a]
        return y

    out = dict(mu=P['amu'][:B], logvar=P['alv'][:B], theta=P['th'][:B])
    sgn = K_LN2 if irt == 3 else -K_LN2
    out['ll'] = scalar((sgn * s_log).astype(F))
    # (a lane of wave a % NW adds dim a's term on every trip: with more dims than waves the trips interleave; the bound's chain
    #  DPW T covers either order)
    out['kl'], out['logq0'], out['logp'] = scalar(by_wave(s_kl)), scalar(by_wave(s_q0)), scalar(by_wave(s_lp))
    no = np.zeros((grid, NW, TILE), F)
    no[:, 0] = s_no
    out['nobs'] = scalar(no)
    if not want_grad:
        return out
    rec = _records(acc_item)[:I]
    if irt == 1:
        out['g_item'] = rec[:, AT:AT + 1]
    else:
        out['g_item'] = np.concatenate([-rec[:, :A], rec[:, AT:AT + 1]] + ([rec[:, AT + 1:AT + 2]] if irt == 3 else []), 1)
    out['g_table'] = _g_table(_records(_tree(acc_t, 1)), A)
    return out


def _emulate_general(case, table, eps, *, drop_missing=False, num_cu=256, want_grad=True, mutate=None, reg='kl', flow=None):
    """The wave-per-person kernel in float32: plain or conditional posterior (table [2, 2A] | [2, I, 2A]), planar flows (flow fp32
    [n, 2A + 1] or None), 1PL / 2PL / 3PL, REG_KL or REG_SAMPLED.  The atomics are summed in wave order (any order is inside the bound)."""
    assert mutate is None or mutate in ACTS_ON['wave-per-person']
    irt, (B, I), A = case['irt'], case['resp'].shape, case['a'].shape[1]
    cond = np.ndim(table) == 3
    Dm = 1 if irt == 1 else A + irt - 1
    p = general_plan(B, I, Dm, want_grad, num_cu)
    nW, T = p['n_waves'], p['trips'][1]
    K = (I + 63) // 64
    rows, W = T * nW, 64 * K
    live = np.arange(rows) < B
    w = _codes(case, rows, W)
    e_c = np.zeros((rows, A), F)
    e_c[:B] = f32(eps)
    e_c = _stale(e_c, nW, mutate)
    tb = f32(table)
    tp = F(0) if (drop_missing or mutate == 'no_prior') else (ONE / (ONE + F(POE_EPS))).astype(F)
    code = np.where(w > 0, 1, 0)
    if mutate == 'swap_n':
        code = 1 - code
    L, S = _poe_sums(w, code, tb, I, A, tp)
    L[~live] = 1.0
    il = (ONE / L).astype(F)
    amu = (S * il).astype(F)
    alv, sig = _fn(np.log, il), _fn(np.sqrt, il)
    th = fma(sig, e_c, amu)
    th[~live] = 0.0
    th0, ladj = th.copy(), np.zeros(rows, F)
    fl = np.zeros((0, 2 * A + 1), F) if flow is None else f32(flow)
    zin, ft, fpsi = [], [], []
    for fp in fl:                                          # lines 122-139
        u_, w_ = fp[:A], fp[A:2 * A]
        zin.append(th.copy())
        aa, cwu = np.full(rows, fp[2 * A], F), F(0)
        for a in range(A):
            aa, cwu = fma(th[:, a], w_[a], aa), fma(w_[a], u_[a], cwu)
        t = _fn(np.tanh, aa)
        psi = (ONE + ((ONE - (t * t).astype(F)).astype(F) * cwu).astype(F)).astype(F)
        ladj = (ladj + _fn(np.log, (np.abs(psi) + F(1e-8)).astype(F))).astype(F)
        ft.append(t), fpsi.append(psi)
        th = fma(u_[None, :], t[:, None], th)
    a_i, b_i = np.zeros((W, A), F), np.zeros(W, F)
    a_i[:I], b_i[:I] = f32(case['a']), f32(case['b'])
    l = np.broadcast_to(b_i, (rows, W)).astype(F)
    for a in range(A):
        l = (l + th[:, a:a + 1]).astype(F) if irt == 1 else fma(-a_i[None, :, a], th[:, a:a + 1], l)
    x = (w > 0).astype(F)
    gg = np.zeros_like(l)
    if irt != 3:
        lc = np.clip(l, F(-LOGIT_LO), F(LOGIT_LO))
        alive = (l >= F(-LOGIT_LO)) & (l <= F(LOGIT_HI)) & (w != 0)
        e = _fn(np.exp, -np.abs(lc))
        llc = (((x * lc).astype(F) - np.maximum(lc, F(0))).astype(F) - _fn(np.log1p, e)).astype(F)
        r_ = (ONE / (ONE + e).astype(F)).astype(F)
        sgm = np.where(lc >= 0, r_, (e * r_).astype(F))
        gl = np.where(alive, (x - sgm).astype(F), F(0))
    else:                                                  # lines 173-185
        gam = np.zeros(W, F)
        gam[:I] = f32(case['gamma'])
        guess = (ONE / (ONE + _fn(np.exp, -gam)).astype(F)).astype(F)[None, :]
        omg = (ONE - guess).astype(F)
        e = _fn(np.exp, -np.abs(l))
        r_ = (ONE / (ONE + e).astype(F)).astype(F)
        er = (e * r_).astype(F)
        sp, sn = np.where(l >= 0, r_, er), np.where(l >= 0, er, r_)
        pr, qr = fma(omg, sp, guess), (omg * sn).astype(F)
        pc, qc = np.clip(pr, F(EPS32), F(1.0 - EPS32)), np.clip(qr, F(EPS32), F(1.0 - EPS32))
        llc = np.where(x > 0.5, _fn(np.log, pc), _fn(np.log, qc))
        dll = np.where(pr == pc, np.where(x > 0.5, (ONE / pc).astype(F), (-ONE / qc).astype(F)), F(0))
        common = ((dll * omg).astype(F) * sn).astype(F)
        gl = np.where(w != 0, (common * sp).astype(F), F(0))
        gg = np.where(w != 0, (common * guess).astype(F), F(0))
    ll = np.zeros((rows, 64), F)
    gth = np.zeros((rows, 64, A), F)
    for k in range(K):
        sl_ = slice(64 * k, 64 * k + 64)
        ob = w[:, sl_] != 0
        ll = np.where(ob, (ll + llc[:, sl_]).astype(F), ll)
        if irt == 1:
            gth = np.where(ob[..., None], (gth + gl[:, sl_, None]).astype(F), gth)
        else:
            gth = np.where(ob[..., None], fma(gl[:, sl_, None], -a_i[None, sl_, :], gth), gth)
    gz = _tree(gth, 1)
    P = dict(amu=amu, alv=alv, inv=il, eps=e_c, th=th)           # (log p is taken at theta_K: line 215)
    klt, q0t, lpt = _heads(P)
    nobs = (w != 0).sum(1).astype(F)
    n1 = ((w != 0) & (code == 1)).sum(1).astype(F)
    n0 = nobs - n1
    h = (F(0.5) * sig * e_c).astype(F)
    gzs = [gz, th.copy() if reg != 'kl' else np.zeros_like(th)]                # line 236
    fterm = np.zeros((rows, 2, len(fl), 2 * A + 1), F)
    for f in range(len(fl) - 1, -1, -1):                   # lines 238-269
        u_, w_ = fl[f][:A], fl[f][A:2 * A]
        t = ft[f]
        omt, cwu = (ONE - (t * t).astype(F)).astype(F), F(0)
        for a in range(A):
            cwu = fma(w_[a], u_[a], cwu)
        unit = (np.where(fpsi[f] >= 0, ONE, -ONE) / (np.abs(fpsi[f]) + F(1e-8)).astype(F)).astype(F)
        for s_ in range(2):
            dl = (F(-1.0 if s_ else 0.0) * unit).astype(F)
            g_t = (dl * ((F(-2) * t).astype(F) * cwu).astype(F)).astype(F)
            for a in range(A):
                g_t = fma(gzs[s_][:, a], u_[a], g_t)
            g_c, g_a = (dl * omt).astype(F), (g_t * omt).astype(F)
            fterm[:, s_, f, :A] = fma(g_c[:, None], w_[None, :], (gzs[s_] * t[:, None]).astype(F))
            fterm[:, s_, f, A:2 * A] = fma(g_c[:, None], u_[None, :], (g_a[:, None] * zin[f]).astype(F))
            fterm[:, s_, f, 2 * A] = g_a
            gzs[s_] = fma(g_a[:, None], w_[None, :], gzs[s_])
    gmu = [gzs[0], (gzs[1] + amu).astype(F) if reg == 'kl' else gzs[1]]
    glv1 = (gzs[1] * h).astype(F)
    glv = [(gzs[0] * h).astype(F), (glv1 + ((F(-0.5) * (ONE - il).astype(F)).astype(F) if reg == 'kl' else F(-0.5))).astype(F)]
    m3, tau3, es3 = _item_tables(tb, A, W)                   # [2, W, A]
    m, tau, es = m3[:, 0], tau3[:, 0], es3[:, 0]           # (the unconditional table: one row per answer)
    gt_cond = np.zeros((2, 2, W, 2 * A), F)                # conditional posterior: the [2][I][2A] table gradient per head
    s_ll = np.zeros((nW, 64), F)
    s_kl, s_q0, s_lp, s_no = (np.zeros(nW, F) for _ in range(4))
    tacc = np.zeros((nW, 2, 2, 2 * A), F)
    facc, s_la = np.zeros((nW, 2, len(fl), 2 * A + 1), F), np.zeros(nW, F)
    slab = np.zeros((p['grid'], W, Dm), F)                  # (without the LDS slab the same sums go to global memory directly)
    for trip in range(T):
        r = slice(trip * nW, (trip + 1) * nW)
        lv = live[r]
        if mutate == 'reset_acc':
            s_ll[:], s_kl[:], s_q0[:], s_lp[:], s_no[:], tacc[:], facc[:], s_la[:] = 0, 0, 0, 0, 0, 0, 0, 0
        s_ll = np.where(lv[:, None], (s_ll + ll[r]).astype(F), s_ll)
        kl_r, q0_r, lp_r = np.zeros(nW, F), np.zeros(nW, F), np.zeros(nW, F)
        for a in range(A):
            kl_r, q0_r, lp_r = (kl_r + klt[r, a]).astype(F), (q0_r + q0t[r, a]).astype(F), (lp_r + lpt[r, a]).astype(F)
        s_kl, s_q0, s_lp = (np.where(lv, (acc + v).astype(F), acc) for acc, v in ((s_kl, kl_r), (s_q0, q0_r), (s_lp, lp_r)))
        s_no = np.where(lv, s_no + nobs[r], s_no)
        s_la = np.where(lv, (s_la + ladj[r]).astype(F), s_la)
        if not want_grad:
            continue
        facc = np.where(lv[:, None, None, None], (facc + fterm[r]).astype(F), facc)
        last = mutate == 'drop_last_row' and trip == T - 1
        if not last:
            gw = np.where(lv[:, None], gl[r], F(0)).reshape(p['grid'], 4, W)
            tw = th[r].reshape(p['grid'], 4, A)
            for q in range(4):
                slab[..., A if irt != 1 else 0] = (slab[..., A if irt != 1 else 0] + gw[:, q]).astype(F)
                if irt != 1:
                    slab[..., :A] = (slab[..., :A] + (-gw[:, q, :, None] * tw[:, q, None, :]).astype(F)).astype(F)
                if irt == 3:
                    slab[..., A + 1] = (slab[..., A + 1] + np.where(lv[:, None], gg[r], F(0)).reshape(p['grid'], 4, W)[:, q]).astype(F)
        if cond:                                           # lines 288-307: one atomic per observed cell, here in row order
            for rr in np.flatnonzero(lv & (w[r] != 0).any(1)) + trip * nW:
                for c in range(2):
                    on = ((w[rr] != 0) & (code[rr] == c))[:, None]
                    for st in range(2):
                        g_m = ((gmu[st][rr] * il[rr]).astype(F)[None] * tau3[c]).astype(F)
                        g_tau = (((gmu[st][rr][None] * (m3[c] - amu[rr][None]).astype(F)).astype(F) - glv[st][rr][None]).astype(F) * il[rr][None]).astype(F)
                        v = (((-g_tau * tau3[c]).astype(F) * tau3[c]).astype(F) * es3[c]).astype(F)
                        gt_cond[st, c, :, :A] = np.where(on, (gt_cond[st, c, :, :A] + g_m).astype(F), gt_cond[st, c, :, :A])
                        gt_cond[st, c, :, A:] = np.where(on, (gt_cond[st, c, :, A:] + v).astype(F), gt_cond[st, c, :, A:])
            continue
        for c, nn in ((0, n0[r]), (1, n1[r])):
            for st in range(2):
                g_m = (((gmu[st][r] * il[r]).astype(F) * tau[c][None]).astype(F) * nn[:, None]).astype(F)
                g_tau = ((((gmu[st][r] * (m[c][None] - amu[r]).astype(F)).astype(F) - glv[st][r]).astype(F) * il[r]).astype(F) * nn[:, None]).astype(F)
                v = (((-g_tau * tau[c][None]).astype(F) * tau[c][None]).astype(F) * es[c][None]).astype(F)
                tacc[:, st, c, :A] = np.where(lv[:, None], (tacc[:, st, c, :A] + g_m).astype(F), tacc[:, st, c, :A])
                tacc[:, st, c, A:] = np.where(lv[:, None], (tacc[:, st, c, A:] + v).astype(F), tacc[:, st, c, A:])

    def atomics(x):                                        # one atomicAdd per wave onto a zeroed word, here in wave order
        t = np.zeros(x.shape[1:], F)
        for q in range(x.shape[0]):
            t = (t + x[q]).astype(F)
        return t

    out = dict(mu=amu[:B], logvar=alv[:B], theta=th0[:B])
    if flow is not None:
        out.update(ability_k=th[:B], ladj=ladj[:B], S_LADJ=atomics(s_la))
        if want_grad:
            fa = atomics(facc)
            out['grad_flow'] = [fa[0], fa[1]]
    out['ll'] = atomics(_tree(s_ll, 1))
    out['kl'], out['logq0'], out['logp'], out['nobs'] = atomics(s_kl), atomics(s_q0), atomics(s_lp), atomics(s_no)
    if want_grad:
        out['g_item'] = atomics(slab)[:I]
        ta = atomics(tacc)
        out['g_table'] = [gt_cond[0][:, :I], gt_cond[1][:, :I]] if cond else [ta[0], ta[1]]
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the cases (tests/test_fallback_model.py emulates them, tests/test_gpu_fallback_cells.py launches them)
# ---------------------------------------------------------------------------------------------------------------------------
CLASSES = ('cancel', 'hostile', 'bias', 'onepl', 'threepl', 'clamp3')
B_CYCLE = (1, 63, 64, 65, 130)


def _case(kernel, cls, A, I, B=None, mask='u8', rows='tight', grad=True, drop=False, reg='kl', cond=False, flows=0):
    """mask: 'u8' | 'i64' | 'none' (every cell observed); rows: 'tight' | 'gather' | 'view' (one float past a 16-byte boundary);
    B None: multi_trip_persons at the device's CU count."""
    return dict(kernel=kernel, cls=cls, A=A, I=I, B=B, mask=mask, rows=rows, grad=grad, drop=drop, reg=reg, cond=cond, flows=flows)


def case_id(c):
    return '-'.join([c['kernel'], c['cls'], f"A{c['A']}", f"I{c['I']}", f"B{c['B'] or 'trips'}", c['mask'], c['rows']] +
                    ([] if c['grad'] else ['forward']) + (['drop'] if c['drop'] else []) + (['sampled'] if c['reg'] != 'kl' else []) + (['cond'] if c['cond'] else []) + ([f"flows{c['flows']}"] if c['flows'] else []))


def _edges():
    out = []
    # tiled, tight rows no 16-byte load can take (I % 4 != 0, or fewer than 4 items): the scalar phase A; every waves boundary, the
    # 16-item block tail, tail_words at I & 15 in {1, 5, 9, 13} (17, 5 / 1003, 143 / 303, 305 / 145, 513, 15, 511, 1023 pad 1, 0)
    for n, I in enumerate((1, 2, 3, 5, 15, 17, 143, 145, 303, 305, 511, 513, 1003, 1023)):
        out.append(_case('tiled', CLASSES[n % 6], (1, 2, 3, 5, 8, 4, 7)[n % 7], I, B_CYCLE[n % 5], grad=n % 4 != 3))
    # tiled, int64 masks at I % 4 == 0 (the vector phase A, load_mask4<1>); ability_dim >= 3 or 3PL or < 192 items keep the
    # wave-per-row kernel away
    for n, I in enumerate((4, 16, 144, 148, 304, 308, 512, 516, 1004, 1024)):
        out.append(_case('tiled', ('threepl', 'cancel', 'clamp3', 'hostile', 'bias')[n % 5], (3, 5, 8)[n % 3], I, B_CYCLE[(n + 2) % 5],
                         mask='i64', grad=n % 4 != 1))
    out += [_case('tiled', 'cancel', 2, 95, 65, rows='gather'), _case('tiled', 'threepl', 3, 148, 63, mask='i64', rows='gather'),
            _case('tiled', 'onepl', 1, 16, 130, mask='i64'), _case('tiled', 'cancel', 3, 143, 64, drop=True),
            _case('tiled', 'threepl', 1, 3, 65), _case('tiled', 'cancel', 2, 144, 65, mask='i64')]
    # wave-per-row: CH 1 / 2 / 4 on both sides of each limit
    for n, I in enumerate((192, 256, 260, 512, 516, 1024)):
        for A in (1, 2):
            out.append(_case('wave-per-row', ('cancel', 'onepl', 'hostile', 'bias')[(n + A) % 4], A, I, (1, 3, 4, 5, 9, 130)[(n + A) % 6],
                             mask='i64', rows='gather' if (n + A) % 3 == 0 else 'tight', grad=(n + 2 * A) % 4 != 0))
    out.append(_case('wave-per-row', 'cancel', 2, 260, 9, mask='i64', drop=True))
    # wave-per-person, unconditional posterior without flows: <16> at ability_dim 9, 12, 16; <8> through tight ragged rows of more
    # than 1024 items; each side of the 40 / 80 / 150 KiB thresholds of the LDS item slab at D = 17
    for n, (A, I) in enumerate(((9, 7), (12, 64), (16, 65), (12, 130), (9, 65), (16, 7))):
        out.append(_case('wave-per-person', ('cancel', 'onepl', 'hostile', 'bias')[n % 4], A, I, (5, 37, 9, 4, 37, 1)[n],
                         mask=('u8', 'i64', 'none')[n % 3], rows='gather' if n % 4 == 1 else 'tight', grad=n != 3, drop=n == 4))
    out += [_case('wave-per-person', 'cancel', 3, 1027, 9), _case('wave-per-person', 'onepl', 8, 1027, 5, mask='none'),
            _case('wave-per-person', 'cancel', 12, 65, 9, reg='sampled'), _case('wave-per-person', 'onepl', 16, 130, 5, mask='i64', reg='sampled'),
            _case('wave-per-person', 'hostile', 8, 1027, 4, reg='sampled'),
            # 3PL, and the conditional posterior (ability_dim <= 8: on tight rows no 16-byte load can take)
            _case('wave-per-person', 'threepl', 12, 65, 37), _case('wave-per-person', 'clamp3', 9, 130, 9, mask='i64'),
            _case('wave-per-person', 'threepl', 16, 603, 9), _case('wave-per-person', 'threepl', 3, 1027, 5, reg='sampled'),
            _case('wave-per-person', 'cancel', 12, 65, 9, cond=True), _case('wave-per-person', 'threepl', 9, 7, 5, mask='i64', cond=True),
            _case('wave-per-person', 'onepl', 16, 130, 4, mask='none', reg='sampled', cond=True),
            _case('wave-per-person', 'cancel', 3, 65, 9, cond=True), _case('wave-per-person', 'threepl', 8, 95, 5, reg='sampled', cond=True),
            _case('wave-per-person', 'hostile', 16, 64, 37, drop=True, cond=True, rows='gather'),
            # planar flows 1 and 8, alone and on the conditional posterior (the library takes flows with REG_SAMPLED only)
            _case('wave-per-person', 'cancel', 12, 65, 9, reg='sampled', flows=1), _case('wave-per-person', 'threepl', 9, 64, 5, mask='i64', reg='sampled', flows=8),
            _case('wave-per-person', 'onepl', 16, 130, 4, mask='none', reg='sampled', flows=8), _case('wave-per-person', 'cancel', 3, 65, 9, reg='sampled', flows=8),
            _case('wave-per-person', 'cancel', 16, 7, 5, reg='sampled', cond=True, flows=1), _case('wave-per-person', 'threepl', 8, 95, 5, reg='sampled', cond=True, flows=8),
            _case('wave-per-person', 'hostile', 12, 64, 37, drop=True, reg='sampled', flows=1, grad=False)]
    for n, I in enumerate((602, 603, 1204, 1205, 2258, 2259)):
        out.append(_case('wave-per-person', 'cancel', 16, I, (37, 9, 5)[n % 3], mask=('u8', 'i64')[n % 2]))
    return out


def _trips():
    return [_case('tiled', 'cancel', 1, 7), _case('tiled', 'threepl', 4, 7), _case('tiled', 'cancel', 1, 8, mask='i64'),
            _case('tiled', 'threepl', 8, 8, mask='i64', grad=False), _case('tiled', 'cancel', 8, 513),
            _case('tiled', 'threepl', 4, 516, mask='i64'), _case('tiled', 'onepl', 1, 513, grad=False),
            _case('wave-per-row', 'cancel', 1, 192, mask='i64'), _case('wave-per-row', 'onepl', 2, 516, mask='i64', rows='gather'),
            _case('wave-per-row', 'cancel', 2, 1024, mask='i64'), _case('wave-per-row', 'cancel', 1, 516, mask='i64', grad=False),
            _case('wave-per-person', 'cancel', 12, 7), _case('wave-per-person', 'cancel', 16, 1208, mask='i64'),
            _case('wave-per-person', 'cancel', 16, 2260), _case('wave-per-person', 'cancel', 9, 65, reg='sampled'),
            _case('wave-per-person', 'cancel', 12, 7, cond=True), _case('wave-per-person', 'threepl', 9, 65),
            _case('wave-per-person', 'cancel', 12, 7, reg='sampled', flows=2)]


# the LDS regime each wave-per-person multi-trip case is named for: (workgroups per CU, item slab in LDS), launch_elbo_general
LDS_REGIMES = {('wave-per-person', 12, 7): (4, True), ('wave-per-person', 16, 1208): (1, True), ('wave-per-person', 16, 2260): (4, False)}


def lds_regimes_met(num_cu):
    """Every regime of LDS_REGIMES has a gradient multi-trip case of TRIPS whose plan is that regime; the one without the slab sends
    its item gradients straight to global atomics (vibo_general.hip:188) over two and three rows of a wave."""
    for (kernel, A, I), (k, in_lds) in LDS_REGIMES.items():
        cs = [c for c in TRIPS if (c['kernel'], c['A'], c['I']) == (kernel, A, I) and c['grad'] and not c['cond'] and not c['flows']
              and c['reg'] == 'kl']
        assert cs, (kernel, A, I)
        p = plan_of(cs[0], persons(cs[0], num_cu), num_cu)
        assert (p['per_cu'], p['item_in_lds']) == (k, in_lds) and p['trips'][0] >= 2 and p['trips'][1] >= 3, (case_id(cs[0]), p)
    return True


def _dense():
    return [_case('tiled', 'cancel', 1, 7), _case('tiled', 'threepl', 2, 8, mask='i64'), _case('wave-per-row', 'cancel', 2, 192, mask='i64'),
            _case('wave-per-row', 'onepl', 1, 260, mask='i64'), _case('wave-per-person', 'cancel', 12, 7),
            # the other template widths: 4, 8 and 16 waves, CH 4, <8>.  Above 4 M cells the observers are dense in three windows of
            # 128 persons (first trip, a later one, the ragged end) and everybody else observes nothing: problem()
            _case('tiled', 'cancel', 3, 148, mask='i64'), _case('tiled', 'cancel', 5, 305), _case('tiled', 'cancel', 8, 513),
            _case('tiled', 'threepl', 4, 516, mask='i64'), _case('wave-per-row', 'cancel', 2, 1024, mask='i64'),
            _case('wave-per-person', 'cancel', 3, 1027), _case('wave-per-person', 'cancel', 12, 7, reg='sampled'),
            _case('wave-per-person', 'cancel', 12, 7, cond=True), _case('wave-per-person', 'threepl', 2, 1027),
            _case('wave-per-person', 'cancel', 12, 7, reg='sampled', flows=2)]


EDGES, TRIPS, DENSE = _edges(), _trips(), _dense()


def item_dim(c):
    irt = 1 if c['cls'] == 'onepl' else 3 if c['cls'] in ('threepl', 'clamp3') else 2
    return 1 if irt == 1 else c['A'] + (irt - 1)


def persons(c, num_cu):
    return c['B'] or multi_trip_persons(c['kernel'], c['I'], c['A'], num_cu, item_dim(c))


def plan_of(c, B, num_cu):
    if c['kernel'] == 'tiled':
        return tiled_plan(B, c['I'], c['A'], num_cu)
    if c['kernel'] == 'wave-per-row':
        return row_plan(B, c['I'], num_cu)
    return general_plan(B, c['I'], item_dim(c), c['grad'], num_cu)


def shifts(c, B):
    """Where the I observers sit on the multi-trip layouts: in the first trip, in a later one, at the ragged end."""
    last = max(0, B - c['I'])
    return tuple(dict.fromkeys((0, min(B // 2 + 3, last), last)))


def problem(c, num_cu, shift=0, missing=None, seed=None):
    B = persons(c, num_cu)
    if c['mask'] == 'none':
        missing = 0.0                                     # no mask: every cell is observed
    if c['drop'] and missing is None:
        assert B <= c['I']                                # --drop-missing leaves a person without answers no posterior at all
    seed = 100 * c['I'] + c['A'] if seed is None else seed
    if c['cond'] or c['flows']:
        return _own_problem(c, B, shift, missing, seed)
    case, table, eps = N.make_problem(c['cls'], c['A'], B, c['I'], seed=seed, shift=shift, drop_missing=c['drop'], missing=missing,
                                      unobserved=unobserved_of(c) if missing is None else ())
    if missing is not None and c['mask'] != 'none' and B * c['I'] > 4_000_000:
        keep = np.zeros(B, bool)
        for lo in (0, B // 2, B - DENSE_WINDOW):
            keep[lo:lo + DENSE_WINDOW] = True
        obs = case['obs'] & keep[:, None]
        x1 = obs & (case['resp'] == 1)
        case['obs'] = obs
        case['theta_oracle'] = person_model(table, (obs & ~x1).sum(1), x1.sum(1), c['I'], eps, c['drop'])['theta'].v
    return case, table, eps


DENSE_WINDOW = 128


def _own_problem(c, B, shift, missing, seed):
    """narrow_model.make_problem for the conditional posterior (table [2, I, 2A]) and for planar flows (case['flow'] fp32 [n, 2A + 1],
    |w . uhat| well below 1): the difficulties are set from the fp64 posterior's theta_K on the case's own responses."""
    A, I = c['A'], c['I']
    rng = np.random.default_rng([seed, 11])
    table = f32(rng.standard_normal((2, I, 2 * A) if c['cond'] else (2, 2 * A)) * 0.7)
    table[..., :A] *= 3.0
    eps = f32(rng.standard_normal((B, A)))
    c0 = M.make_case(c['cls'], A, B, I, seed, shift=shift)
    obs = c0['obs'] if missing is None else rng.random((B, I)) >= missing
    if missing is None:
        obs[:, list(unobserved_of(c))] = False
    x1 = obs & (c0['resp'] == 1)
    pm = person_model_cond(table, obs, x1, eps, c['drop']) if c['cond'] else \
        person_model_general(table, (obs & ~x1).sum(1), x1.sum(1), I, eps, c['drop'])
    flow = f32(rng.standard_normal((c['flows'], 2 * A + 1)) * 0.5 * A ** -0.25) if c['flows'] else None
    th_k = flows_model(pm['theta'], flow)['theta_k'].v if c['flows'] else pm['theta'].v
    case = M.make_case(c['cls'], A, B, I, seed, theta=f32(th_k), shift=shift)
    case['obs'], case['theta_oracle'] = obs, pm['theta'].v
    if c['flows']:
        case['flow'] = flow
    return case, table, eps


def unobserved_of(c):
    """Every other one-observer case takes the observer of item I // 2 away: every output that item feeds is an exact zero."""
    ok = c['I'] >= 5 and (c['I'] + c['A']) % 2 == 0 and not c['drop'] and c['mask'] != 'none'
    return (c['I'] // 2,) if ok else ()


def emulate_of(c, case, table, eps, num_cu, mutate=None):
    kw = dict(drop_missing=c['drop'], num_cu=num_cu, want_grad=c['grad'], mutate=mutate)
    if c['kernel'] == 'wave-per-person':
        kw.update(reg=c['reg'], flow=case.get('flow'))
    return emulate(c['kernel'], case, table, eps, **kw)


def ratios(exp, got, irt, A):
    """narrow_model.ratios plus, with flows, ability_k and ladj per entry, S_LADJ and both flow-gradient heads per entry.  The cell
    reference of a launch with flows is built from theta_K, so got['theta'] is swapped for the check of theta_0 only."""
    r = N.ratios(exp, got, irt, A)
    w = lambda k, g: float(np.max(np.where(exp[k][1] > 0, np.abs(np.asarray(g, D) - exp[k][0]) / np.where(exp[k][1] > 0, exp[k][1], 1.0),
                                           np.where(np.abs(np.asarray(g, D) - exp[k][0]) > 0, np.inf, 0.0))))
    if 'ability_k' in exp:
        r['ability_k'], r['ladj'] = w('ability_k', got['ability_k']), w('ladj', got['ladj'])
        r['S_LADJ'] = w('S_LADJ', np.asarray(got['S_LADJ']).reshape(1))
        if 'grad_flow' in got:
            for s_ in range(2):
                r[f'grad_flow({s_})'] = w(f'grad_flow({s_})', got['grad_flow'][s_])
    return r


def expected_of(c, case, table, eps, theta, num_cu):
    if c['kernel'] == 'wave-per-person':
        return expected_general(case, table, eps, theta, num_cu=num_cu, drop_missing=c['drop'], want_grad=c['grad'], reg=c['reg'],
                                flow=case.get('flow'))
    return expected(c['kernel'], case, table, eps, theta, num_cu=num_cu, drop_missing=c['drop'])
