"""CPU checks of oracle/split_model.py: the fp64 model of the matrix kernel's split-f16 arithmetic stays inside its own a-priori
bound on every adversarial input class, each single-term mutation of the model does not, and the generators reach the
regimes they are named after.  tests/test_gpu_split_worst_case.py asserts the same bound on the kernel."""
import numpy as np
import pytest

from oracle import split_model as M

CASES = [  # cls, A, B, I, seed, kwargs
    ('cancel', 2, 33, 200, 1, {}), ('cancel', 5, 95, 640, 2, {}), ('cancel', 8, 64, 1000, 3, {}), ('cancel', 2, 64, 640, 18, dict(all_signs=True)),
    ('clamp3', 2, 33, 200, 19, {}), ('clamp3', 8, 64, 1000, 20, {}),
    ('hostile', 2, 64, 640, 4, {}), ('hostile', 8, 33, 1024, 5, {}),
    ('bias', 1, 32, 200, 6, {}), ('bias', 8, 95, 1000, 7, {}),
    ('onepl', 4, 64, 640, 8, {}), ('onepl', 8, 33, 1000, 9, {}),
    ('mixed_a', 8, 64, 1000, 10, dict(outliers=(6,))), ('mixed_a', 8, 64, 1000, 11, dict(outliers=(10,))),
    ('mixed_a', 5, 95, 640, 12, dict(outliers=(14,), same_tile=True)), ('mixed_a', 8, 64, 1024, 13, dict(outliers=(20, 14, 10, 6))),
    ('mixed_b', 8, 64, 1000, 14, dict(outliers=(14,))), ('mixed_b', 2, 33, 200, 15, dict(outliers=(16,), same_tile=True)),
    ('mixed_b', 8, 64, 1000, 16, dict(outliers=(20,))), ('mixed_b', 5, 95, 640, 17, dict(outliers=(29,))),
]
IDS = [f'{c[0]}-A{c[1]}-B{c[2]}-I{c[3]}' + ''.join(f'-2^{k}' for k in c[5].get('outliers', ())) + ('-all-signs' if c[5].get('all_signs') else '')
       for c in CASES]


def _observed(case, x):
    return x[case['p_obs'], np.arange(x.shape[1])]


@pytest.mark.parametrize('cls,A,B,I,seed,kw', CASES, ids=IDS)
def test_model_stays_inside_its_bound_on_every_cell(cls, A, B, I, seed, kw):
    """ALL B x I cells (the unobserved ones run through the same products), not only the constructed ones."""
    c = M.make_case(cls, A, B, I, seed, **kw)
    err = np.abs(M.logit_model(c['theta'], c['a'], c['b'], c['irt']) - M.exact_logit(c['theta'], c['a'], c['b']))
    bound = M.cell_bound(c['theta'], c['a'], c['b'], c['irt'])
    assert np.all(err <= bound), float((err / np.maximum(bound, 1e-300)).max())
    ratio = float((err[bound > 0] / bound[bound > 0]).max())
    assert ratio > 0.02, ratio          # the bound is not orders of magnitude above what the scheme does at its worst cell


def test_every_mutation_leaves_the_bound_by_a_factor_of_four():
    """Worst error / bound over all generated cells, per dropped term.  The un-mutated model: at most 1 (test above)."""
    worst = {d: 0.0 for d in M.DROPS}
    for cls, A, B, I, seed, kw in CASES:
        c = M.make_case(cls, A, B, I, seed, **kw)
        exact = M.exact_logit(c['theta'], c['a'], c['b'])
        bound = M.cell_bound(c['theta'], c['a'], c['b'], c['irt'])
        for d in M.DROPS:
            err = np.abs(M.logit_model(c['theta'], c['a'], c['b'], c['irt'], drop=(d,)) - exact)
            ok = bound > 0
            worst[d] = max(worst[d], float((err[ok] / bound[ok]).max()))
    for d, r in worst.items():
        assert r >= 4.0, (d, r)


def test_gradient_mutation_g_hi_only_leaves_the_bound():
    c = M.make_case('cancel', 8, 64, 1000, 3)
    ref = M.reference(c)
    jsh, bsh = M.launch_scales(c['a'], c['b'], c['irt'])
    e_l = M.cell_bound(c['theta'], c['a'], c['b'], c['irt'])
    _, bnd_a, bnd_t = M.grad_bounds(c['theta'], c['a'], c['b'], ref['g'], c['obs'], e_l * 0.0, c['irt'])      # (exact g fed in: no logit error)
    for fn, exact, bnd, args in ((M.grad_theta_model, ref['g_theta'], bnd_t, (ref['g'], c['a'], c['irt'], jsh)),
                                 (M.grad_a_model, ref['g_a'], bnd_a, (ref['g'], c['theta'], jsh))):
        assert np.all(np.abs(fn(*args) - exact) <= bnd)
        assert float((np.abs(fn(*args, drop_g_lo=True) - exact) / bnd).max()) >= 4.0


@pytest.mark.parametrize('cls,A,B,I,seed,kw', CASES, ids=IDS)
def test_generators_reach_their_regime(cls, A, B, I, seed, kw):
    c = M.make_case(cls, A, B, I, seed, **kw)
    o = M.scaled_operands(c['theta'], c['a'], c['b'], c['irt'])
    l = M.exact_logit(c['theta'], c['a'], c['b'])
    lo, s = _observed(c, l), _observed(c, np.abs(np.asarray(c['theta'], np.float64)) @ np.abs(np.asarray(c['a'], np.float64)).T)
    ordinary = np.ones(I, bool)
    ordinary[c['outliers']] = False
    assert np.all(c['obs'].sum(0) == 1)
    if cls != 'clamp3':
        assert np.all(np.abs(lo[ordinary]) <= 15.9)        # no observed cell past the Bernoulli clamp (the outliers' own cells may be)
    if cls in ('cancel', 'onepl'):
        assert np.all(np.abs(lo) <= 3.001)
        small = np.abs(lo) < 2e-3
        assert small.mean() > 0.15 and np.all(s[small] / np.abs(lo[small]) >= 1e3 * (A >= 2) * (1 if cls == 'cancel' else 0.5))
        assert M.sub_share(o['a_s']) == 0.0 and M.sub_share(o['t_s']) == 0.0
    if kw.get('all_signs'):
        pat = set(zip(((c['a'] < 0) @ (1 << np.arange(A))).tolist(), ((c['theta'][c['p_obs']] < 0) @ (1 << np.arange(A))).tolist()))
        assert len(pat) == 4 ** A                          # every sign pattern of a x every sign pattern of theta, in an observed cell
    if cls == 'clamp3':
        ref = M.reference(c)
        cg = M.sigmoid(np.asarray(c['gamma'], np.float64))
        p = cg + (1 - cg) * M.sigmoid(np.clip(lo, -M.LOGIT_LO, M.LOGIT_LO))
        near = np.minimum(np.abs(p - M.EPS32), np.abs(1 - p - M.EPS32)) <= 1e-6
        assert near.mean() >= 0.99                         # the whole class sits at the clamp band ...
        assert ((1 - p) < 1e-6).mean() > 0.3 and (p < 1e-6).mean() > 0.3      # ... on both sides
        assert np.median(s) > 4 * A and np.all(s >= A)     # products of |a|, |theta| in [1, 4] against a difficulty set for |l| ~ 13 ... 16.4
        excl = _observed(c, ref['excluded'])
        assert 0 < excl.mean() <= 0.02                     # the fp64 reference itself leaves out fewer than the cap
        live = _observed(c, ref['live'])
        assert 0.2 < live[~excl].mean() < 0.9              # asserted cells on both sides of the clamp decision
        # the reference's logit clamp and the probability clamp agree on every asserted cell: no live-p cell below -LOGIT_LO
        p_raw = cg + (1 - cg) * M.sigmoid(lo)
        assert not np.any((lo < -M.LOGIT_LO) & (p_raw >= M.EPS32) & ~excl)
        margin = np.minimum(np.abs(lo + M.LOGIT_LO), np.abs(lo - M.LOGIT_LO))
        e_l = _observed(c, M.cell_bound(c['theta'], c['a'], c['b'], c['irt']))
        assert np.all(margin > 20 * e_l)                   # the logit's own error cannot carry a cell across the logit clamp
    if cls == 'hostile':
        th, tl = M.split_rtz(o['t_s'])
        assert (tl == 0).mean() > 0.1 and (np.abs(o['t_s'] - th - tl) > 0).mean() > 0.2      # exact f16 values and real residuals
        assert (np.abs(lo) <= 3.001).mean() > 0.9
    if cls == 'bias':
        assert np.all(s <= 1e-3) and np.all(np.abs(c['b']) < 8) and (s == 0).mean() >= 0.25
    if cls == 'mixed_a':
        assert M.sub_share(o['a_s'][ordinary]) >= (0.3 if max(kw['outliers']) < 10 else 0.99)
        assert o['jsh'] == -((max(kw['outliers']) + 1) >> 1)
    if cls == 'mixed_b':
        assert o['bsh'] == max(max(kw['outliers']) + 1 - 15, 0)
        if o['bsh']:
            share = float((np.abs(o['nb_s'][ordinary]) < 1.0).mean())      # difficulties held on the absolute 2^(bsh - 24) grid
            assert share >= (0.99 if o['bsh'] >= 6 else 0.2), share


def test_split_rtz_against_every_mantissa_of_several_binades():
    """All 2^23 fp32 mantissas of the binades 2^0, 2^-2 (the last one with a relative residual), 2^7 and 2^15 (the top of the f16
    range); every 64th mantissa of 2^-3, 2^-9 and 2^-14 (absolute regime).  Observed worst |x - hi - lo| / |x|: between 5.9 u
    and 6 u (u = 2^-24; patterns like x = 1 + 2^-11 + 3 2^-23) in each relative binade -- C_SPLIT = 6 u; below 2^-2 the residual
    stays under 2^-24 absolute.  The pieces are f16 values, lo never exceeds 2^-10 |x|, and hi + lo never overshoots."""
    m = np.arange(1 << 23, dtype=np.uint32)
    worst = 0.0
    for e, step in ((0, 1), (-2, 1), (7, 1), (15, 1)):
        x = M.from_bits(np.ones(1, np.int8), e, m[::step]).astype(np.float64)
        hi, lo = M.split_rtz(x)
        r = x - hi - lo
        assert np.all(r >= 0) and np.all(np.abs(lo) <= 2.0 ** -10 * x)
        assert np.all(hi.astype(np.float16).astype(np.float64) == hi) and np.all(lo.astype(np.float16).astype(np.float64) == lo)
        worst = max(worst, float((r / x).max()))
        assert np.all(r <= M.eps_split(x))
    assert 5.9 * M.U < worst <= M.C_SPLIT
    for e in (-3, -9, -14, -20):
        for sign in (1, -1):
            x = M.from_bits(np.full(1, sign, np.int8), e, m[::64]).astype(np.float64)
            hi, lo = M.split_rtz(x)
            r = np.abs(x - hi - lo)
            assert np.all(r < 2.0 ** -24) and np.all(r <= M.eps_split(x)) and np.all(np.abs(hi + lo) <= np.abs(x))
    # saturation and the sign symmetry of round-toward-zero
    assert M.rtz16(70000.0) == 65504.0 and M.rtz16(-70000.0) == -65504.0
    hi, lo = M.split_rtz(np.array([-1.0009765, 1.0009765]))
    assert hi[0] == -hi[1] and lo[0] == -lo[1]


def test_bias_pieces_are_exact_from_one_upwards():
    rng = np.random.default_rng(0)
    nb = M._hostile(rng, (20000,), 0, 15).astype(np.float64)
    b0, b1, b2 = M.bias_pieces(nb)
    assert np.all(b0 + b1 + b2 == nb)
    assert float(np.abs(nb - b0 - b1).max()) > 0                          # ... and the third piece is what makes them so


def test_launch_scales_follow_the_kernel_comment():
    one = np.ones((4, 2), np.float32)
    assert M.launch_scales(one, np.zeros(4, np.float32)) == (0, 0)         # |na| = 1.44 < 2^1: jsh = -(1 >> 1)
    assert M.launch_scales(one * 2.0 ** 20, np.zeros(4, np.float32))[0] == -10
    assert M.launch_scales(one * 2.0 ** -20, np.zeros(4, np.float32))[0] == 10
    assert M.launch_scales(one * 1e-30, np.zeros(4, np.float32))[0] == 12 and M.launch_scales(one * 1e30, one[:, 0])[0] == -14
    assert M.launch_scales(one, np.full(4, 2.0 ** 14, np.float32))[1] == 0
    assert M.launch_scales(one, np.full(4, 2.0 ** 29, np.float32))[1] == 15
