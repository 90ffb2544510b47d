"""CPU checks of oracle/decoder_model.py: the fp64 value of the decoder kernel's hi/lo scheme stays inside every a-priori bound on
every entry of every input class, mode and mask layout; every value mutation of it leaves some bound by at least 4 x (the factor of
tests/test_split_model.py) in every class where it can act; the restated launch layout equals figures worked out by hand from
vibo_decoder_fwd_bwd's source; the generators reach the regimes they are named after.  tests/test_gpu_decoder_cells.py asserts the same
bounds on the kernel."""
import functools

import numpy as np
import pytest

from oracle import decoder_model as D
from oracle import split_model as M

MODES = dict(deep=dict(), link=dict(has_U=False, has_w1=True), residual=dict(resid=1.0), all=dict(has_w1=True, resid=1.0, has_guess=True))
# B, I, person chunks, mask layout, where the single observer sits
LAYOUTS = ((10, 37, 4, 'dense', None), (7, 70, 1, 'single', 'later'), (9, 17, 2, 'term', None), (7, 33, 1, 'single', 'last'))

# Where a mutation cannot act, and why (the a-priori bound already contains an error of the mutation's size):
#   zero     W2 = 0: every product of the two mat-vecs is zero; dz1 = 0, so dw1 and the layer-1 ELU' have nothing to act on
#   small_w  |W2| < 2^-10: W_lo is a few steps of the subnormal grid or zero, and |W_hi h_lo|, |W_hi dz_lo| are of the size of
#            res_W |h1|, res_W |dz2| (2^-24 absolute per weight), which the bound evaluates
#   small_g  |dz2| <= 2^-14: dz_hi is on the subnormal grid itself, dz_lo is zero or one step
#   elu0     |h1| < 2^-20: h_hi has four bits, h_lo is zero or one step, every W.h1 product is below the 2^-25 floor of eps_h; both
#            ELU' are 1 - O(2^-20)
CANNOT_ACT = {
    'f_hl': ('zero', 'small_w', 'elu0'), 'f_lh': ('zero', 'small_w', 'elu0'),
    'b_hl': ('zero', 'small_w', 'small_g'), 'b_lh': ('zero', 'small_w', 'small_g'),
    'w_hl': (), 'w_lh': ('elu0',),
    'slot': ('zero', 'elu0'), 'lgt_other': ('zero',), 'elu_layer': ('zero', 'elu0'),
    'stale_pair': (), 'pad_person': (), 'tail_item': (),
}


def _ratios(case, lay, chunks, kind, X, exact, bnd, mut):
    T, got, _ = D.run(case, chunks, scheme=True, mut=mut)
    r = D.ratios(got, exact, bnd, X)
    if kind == 'single':                                 # the backward half on the run's own dz2, as the GPU test reads it from dvec_part
        Y = D.condition(case, X, np.where(case['mask'][..., None] != 0, T['dz2'], 0.0))
        bg, _ = D.record_bounds(case, Y, lay, given=True)
        r.update({k + '|dz2': v for k, v in D.ratios(got, D.records(Y, lay, scheme=False), bg, None, names=D.GIVEN).items()})
    return r


@functools.lru_cache(maxsize=None)
def _worst(cls):
    """-> {None | mutation: worst error / bound over the class's modes and layouts}, and the intact model's failures."""
    worst, failed = {m: 0.0 for m in (None,) + D.MUTATIONS}, []
    for mode, kw in MODES.items():
        if cls == 'guess3' and mode != 'residual':
            continue
        for B, I, chunks, kind, where in LAYOUTS:
            lay = D.layout(B, I, chunks)
            case = D.with_mask(D.make_case(cls, B, I, seed=B + I, **kw), D.masks(kind, lay, seed=3, where=where or 'first'))
            X, exact, _ = D.run(case, chunks, scheme=False)
            bnd, _ = D.record_bounds(case, X, lay)
            for mut in worst:
                r = _ratios(case, lay, chunks, kind, X, exact, bnd, mut)
                worst[mut] = max(worst[mut], max(r.values()))
                if mut is None and max(r.values()) > 1.0:
                    failed.append((mode, B, I, kind, {k: v for k, v in r.items() if v > 1.0}))
    return worst, failed


@pytest.mark.parametrize('cls', D.CLASSES)
def test_scheme_stays_inside_every_bound_on_every_entry(cls):
    worst, failed = _worst(cls)
    print(cls, 'intact worst error / bound', round(worst[None], 3))
    assert not failed, failed
    assert worst[None] > 0.02          # (the given-dz2 bounds are evaluated residuals: the intact scheme sits right at them)


@pytest.mark.parametrize('cls', D.CLASSES)
def test_every_mutation_leaves_a_bound_by_a_factor_of_four(cls):
    worst, _ = _worst(cls)
    print(cls, {m: float(f'{worst[m]:.3g}') for m in D.MUTATIONS})
    for mut in D.MUTATIONS:
        if cls not in CANNOT_ACT[mut]:
            assert worst[mut] >= 4.0, (cls, mut, worst[mut])


def test_every_mutation_acts_in_the_unit_class_and_in_most_others():
    assert all('unit' not in v and 'hostile' not in v and 'cancel' not in v and 'large' not in v and 'guess3' not in v for v in CANNOT_ACT.values())


def test_layout_against_figures_worked_out_by_hand():
    """vibo_decoder_fwd_bwd: ppc = ((B + chunks - 1) / chunks + 1) & ~1, grid (ceil(I / 64), chunks); decoder_kernel: p_begin = blockIdx.y
    ppc, p_end = min(p_begin + ppc, B), wave_id = (blockIdx.y gridDim.x + blockIdx.x) 4 + w, item = 64 blockIdx.x + 16 w + i16."""
    a = D.layout(10, 70, 4)                              # ceil(10 / 4) = 3 -> ppc 4: persons 0-3, 4-7, 8-9, and a fourth chunk with nobody
    assert a.ppc == 4 and a.ranges[:3] == [(0, 4), (4, 8), (8, 10)] and a.ranges[3][0] >= a.ranges[3][1] and a.empty == [3]
    assert a.n_ib == 2 and a.n_wave == 32 and a.wave_id(2, 1, 3) == 23 and a.wave_id(3, 0, 0) == 24
    assert a.shapes == dict(ll_part=(32,), dW2_part=(32, 64, 64), dvec_part=(32, 4, 64), dV_part=(8, 10, 64), dU_part=(4, 70, 64),
                            dguess_part=(4, 70), dL=(10, 70))
    assert a.pairs(0) == [(0, 1), (2, 3)] and a.pairs(2) == [(8, 9)] and a.pairs(3) == []
    assert list(a.wave_items(1, 0)) == [64, 65, 66, 67, 68, 69] and a.tail_lanes(1, 0) == 10 and len(a.wave_items(1, 1)) == 0
    assert a.chunk_of(7) == 1 and a.chunk_of(8) == 2
    b = D.layout(7, 16, 1)                               # ceil(7 / 1) = 7 -> ppc 8: one chunk, three full pairs and an odd tail
    assert b.ppc == 8 and b.ranges == [(0, 7)] and b.empty == [] and b.n_wave == 4
    assert b.pairs(0) == [(0, 1), (2, 3), (4, 5), (6, None)]
    assert list(b.wave_items(0, 0)) == list(range(16)) and len(b.wave_items(0, 1)) == 0
    assert D.k_of(1) == [4, 5, 6, 7, 20, 21, 22, 23, 36, 37, 38, 39, 52, 53, 54, 55]
    assert sorted(sum((D.k_of(g)[:8] for g in range(4)), [])) == list(range(32))       # MFMA step s = 0 contracts k < 32
    c = D.layout(9, 130, 5)                              # ceil(9 / 5) = 2 -> ppc 2: 0-1, 2-3, 4-5, 6-7, 8 alone
    assert c.ppc == 2 and c.ranges[4] == (8, 9) and c.pairs(4) == [(8, None)] and c.n_ib == 3 and c.wave_id(4, 2, 0) == 56


def test_mask_layouts():
    lay = D.layout(10, 70, 4)
    t = D.masks('term', lay, seed=1)
    for ib in range(2):
        for w in range(4):
            it = lay.wave_items(ib, w)
            if len(it):
                assert np.all(t[:, it].sum(1) == 1)      # one observed item per (person, 16-item wave group)
    lanes = set()
    for seed in range(16):
        for where in ('first', 'later', 'last', 'last0'):
            s = D.masks('single', lay, seed=seed, where=where)
            for c, (lo, hi) in enumerate(lay.ranges):
                for ib in range(2):
                    for w in range(4):
                        it = lay.wave_items(ib, w)
                        n = int(s[lo:hi][:, it].sum()) if len(it) else 0
                        assert n == (1 if hi > lo and len(it) else 0)
            lanes |= set(np.argwhere(s[:, :16])[:, 1].tolist())
    assert lanes == set(range(16))                       # the observer runs through every i16 lane
    lay7 = D.layout(7, 33, 1)
    assert np.argwhere(D.masks('single', lay7, seed=0, where='last'))[0][0] == 6        # the odd tail, r = 0
    assert np.argwhere(D.masks('single', lay7, seed=0, where='later'))[0][0] == 2       # a later pair, r = 0; seed 1: r = 1
    assert np.argwhere(D.masks('single', lay7, seed=1, where='later'))[0][0] == 3


def test_split_residual_stays_under_the_grid_bound_at_every_scale():
    rng = np.random.default_rng(5)
    for e in range(-27, 15):
        x = np.concatenate([M.from_bits(rng.choice([-1, 1], 4000), e, rng.integers(0, 1 << 23, 4000, dtype=np.uint32)),
                            M.from_bits(1, e, np.asarray(M.HOSTILE_MANTISSAS, np.uint32))]).astype(np.float64)
        hi, lo = D.split_act(x)
        res = np.abs(x - hi - lo)
        assert np.all(res <= D.apriori(np.abs(x))), e
        assert np.all(np.abs(hi) <= np.abs(x)) and np.all(hi * x >= 0)                  # hi truncates
        if e >= -3:
            assert np.all(res <= 4 * D.U_ * np.abs(x))                                  # both pieces normal: 2^-22 relative
        wh, wl = D.split_w(x)
        assert np.all(np.abs(x - wh - wl) <= 2 * D.apriori(np.abs(x)))                  # truncated lo: a whole step
    # the documented limit: at |x| ~ 1e-3 the pieces reassemble x to 2^-25 absolute, 3e-5 relative
    x = np.float64(np.float32(1.0e-3))
    assert D.apriori(x) == 2.0 ** -25 and 2.0 ** -25 / x > 2e-5


@pytest.mark.parametrize('cls', D.CLASSES)
def test_generators_reach_their_regime(cls):
    B, I = 10, 130
    case = D.make_case(cls, B, I, seed=11, **(dict(has_w1=True, resid=1.0) if cls == 'elu0' else {}))
    case = D.with_mask(case, np.ones((B, I), np.uint8))
    X = D.terms(case, scheme=False)
    W = np.abs(np.asarray(case['W2'], np.float64))
    if cls == 'unit':
        assert 0.1 < np.abs(X['z1']).mean() < 2 and np.abs(X['o']).max() < 15
    if cls == 'hostile':
        m = lambda t: np.asarray(t, np.float32).view(np.uint32) & 0x7FFFFF
        assert all(set(m(case[k]).ravel().tolist()) <= set(M.HOSTILE_MANTISSAS) for k in ('W2', 'U', 'V'))
    if cls == 'cancel':
        assert np.all(np.abs(X['h1']) @ W.T >= 1e3 * np.abs(X['z2']))
    if cls == 'small_w':
        assert W.max() <= 2.0 ** -10 and W.min() >= 2.0 ** -16.01
    if cls == 'small_g':
        assert np.abs(X['dz2']).max() <= 2.0 ** -14 and np.abs(X['dz2']).max() > 2.0 ** -18
    if cls == 'large':
        big = max(np.abs(np.asarray(case[k])).max() for k in ('U', 'V', 'W2', 'w3', 'b2'))
        assert big < 2.0 ** 15 and max(np.abs(X['h1']).max(), np.abs(X['h2']).max()) < 2.0 ** 15
        assert 2.0 ** 9 <= np.abs(X['h1']).max() <= 2.0 ** 10 and np.abs(X['o']).max() < 15.9
    if cls == 'elu0':
        for z in (X['z1'], X['z2']):
            assert np.abs(z).max() < 2.0 ** -20 and (z > 0).mean() > 0.2 and (z < 0).mean() > 0.2
    if cls == 'zero':
        assert W.max() == 0 and np.all(X['dz1'] == 0) and np.abs(X['dz2']).max() > 0
    if cls == 'guess3':
        excl = X['excluded']
        assert excl.mean() <= 0.02                       # the cap on cells nobody asserts
        near_hi, near_lo = (1 - X['p']) < 5e-6, X['p'] < 1e-6
        assert near_hi.mean() > 0.3 and near_lo.mean() > 0.3 and (near_hi | near_lo).all()
        assert 0.2 < X['inside'][near_lo].mean() < 0.8 and X['inside'][near_hi].all()       # both sides of the lower clamp value
        E = D.term_bounds(case, X)
        # the value's own error cannot flip a clamp decision: 20 x at eps32; at 1 - eps32 p sits 24 steps of 2^-24 or more below 1,
        # the clamp value 2, and the sigmoid and the mixture are bounded at 11 steps
        lim = np.minimum(np.abs(X['p'] - D.EPS32), np.abs(X['p'] - (1.0 - D.EPS32)))
        assert np.all(lim[~excl & near_lo] > 20 * E['p'][~excl & near_lo]) and np.all(lim[~excl & near_hi] > 1.5 * E['p'][~excl & near_hi])
