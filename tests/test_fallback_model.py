"""CPU checks of oracle/fallback_model.py: the float32 emulations of the tiled, wave-per-row and wave-per-person kernels stay
inside the a-priori bound of EVERY output entry on every case tests/test_gpu_fallback_cells.py launches (the multi-trip layouts on a
one-CU grid, so that the same trips take seconds here); each mutation of the trip structure leaves a bound by a wide margin wherever it
can act; the geometry functions give the grids the planner's source states; the generators reach their regimes from the fp64 reference
alone."""
import numpy as np
import pytest

from oracle import fallback_model as Fm
from oracle import narrow_model as N

CU = 1                                                   # the multi-trip shapes on one CU: the same trips, a few hundred persons


def run(c, num_cu=256, shift=0, missing=None, mutate=None):
    case, table, eps = Fm.problem(c, num_cu, shift=shift, missing=missing)
    em = Fm.emulate_of(c, case, table, eps, num_cu, mutate)
    exp = Fm.expected_of(c, case, table, eps, em.get('ability_k', em['theta']), num_cu)      # (the cells run on theta_K)
    r = Fm.ratios(exp, em, case['irt'], c['A'])
    if missing is not None:
        r.pop('logit', None)
    return case, exp, r


def regime(c, exp, case):
    """(c) of the issue on the fp64 reference alone: |l| <= 3 on at least 0.8 of the observed cells (the bias class: 0.7, as in the
    narrow file), at most 2 % of them excluded next to a probability clamp."""
    n_l3, n_obs = exp['logit_share']
    if n_obs >= 16 and c['cls'] != 'clamp3' and c['mask'] != 'none':      # (one observer per item; without a mask every cell is observed)
        assert n_l3 >= (0.7 if c['cls'] == 'bias' else 0.8) * n_obs, (Fm.case_id(c), n_l3, n_obs)
    assert int(exp['excluded'].sum()) <= max(1, 0.02 * int(np.asarray(case['obs']).sum())), Fm.case_id(c)


@pytest.mark.parametrize('c', Fm.EDGES, ids=Fm.case_id)
def test_emulation_stays_inside_every_bound_on_the_edge_cases(c):
    case, exp, r = run(c)
    assert max(r.values()) <= 1.0, r
    regime(c, exp, case)
    if c['grad']:                                        # entries whose reference is an exact zero carry a zero bound
        assert np.all(exp['dLL/db'][1][exp['dLL/db'][0] == 0] == 0)
        for i in Fm.unobserved_of(c):                    # the item that lost its observer: zero reference, zero bound
            assert not case['obs'][:, i].any() and exp['dLL/db'][0][i] == 0 and exp['dLL/db'][1][i] == 0
            assert 'dLL/da' not in exp or not (exp['dLL/da'][0][i].any() or exp['dLL/da'][1][i].any())


def encode_cases():
    """The edge cases whose rows ops.encode_posterior hands to the wave-per-person encode_kernel: ability_dim above 8, or tight rows no
    16-byte load can take under a mask the call does not narrow (it narrows int64 masks to bytes)."""
    return [c for c in Fm.EDGES if not c['flows'] and (c['kernel'] == 'wave-per-person' or (c['kernel'] == 'tiled' and c['mask'] == 'u8'))]


@pytest.mark.parametrize('c', encode_cases(), ids=Fm.case_id)
def test_encode_emulation_stays_inside_its_bounds(c):
    case, table, eps = Fm.problem(c, 256)
    em, exp = Fm.emulate_encode(case, table, drop_missing=c['drop']), Fm.expected_encode(case, table, drop_missing=c['drop'])
    for k in ('mu', 'logvar'):
        assert np.all(np.abs(em[k].astype(np.float64) - exp[k][0]) <= exp[k][1]), k
    bad = Fm.emulate_encode(dict(case, resp=1.0 - case['resp']), table, drop_missing=c['drop'])       # n0 / n1 swapped
    x1 = case['obs'] & (case['resp'] == 1)
    if not np.all(x1.sum(1) == (case['obs'] & ~x1).sum(1)):
        assert np.any(np.abs(bad['mu'].astype(np.float64) - exp['mu'][0]) > 4 * exp['mu'][1])


@pytest.mark.parametrize('c', Fm.TRIPS, ids=Fm.case_id)
def test_emulation_over_several_trips(c):
    B = Fm.persons(c, CU)
    lo, hi = Fm.plan_of(c, B, CU)['trips']
    assert lo >= 2 and hi >= 3, (lo, hi)
    for shift in Fm.shifts(c, B):
        case, exp, r = run(c, CU, shift=shift)
        assert max(r.values()) <= 1.0, (shift, r)
        regime(c, exp, case)


@pytest.mark.parametrize('c', Fm.TRIPS + Fm.DENSE, ids=Fm.case_id)
def test_emulation_dense_over_several_trips_with_the_counted_chain(c):
    _, _, r = run(c, CU, missing=0.3)
    assert max(r.values()) <= 1.0, r


# mutation -> the observables one of which has to leave its bound
NAMES = {
    'stale_eps': ('theta',), 'no_toggle': ('dLL/db', 'S_LL', 'grad_table(0)'), 'second_set': ('theta', 'mu'),
    'reset_acc': ('dLL/db', 'S_LL', 'S_KL', 'grad_table(1)'), 'tail_words': ('S_LL',), 'swap_n': ('mu', 'theta'),
    'no_prior': ('logvar', 'mu'), 'drop_last_row': ('dLL/db',),
}
ACTING = {'stale_eps': 33, 'no_toggle': 12, 'reset_acc': 33, 'second_set': 7, 'tail_words': 21, 'swap_n': 77, 'no_prior': 63,
          'drop_last_row': 13}


@pytest.mark.parametrize('mutate', Fm.MUTATIONS)
def test_every_mutation_leaves_a_bound_by_a_factor_of_four(mutate):
    """On EVERY case where the mutation can act: the dense multi-trip launches (every trip holds observers) for the trip mutations,
    the edge cases for the others."""
    least, n = np.inf, 0
    trip_mutation = mutate in ('stale_eps', 'no_toggle', 'reset_acc', 'second_set', 'drop_last_row')
    for c in (Fm.TRIPS + Fm.DENSE if trip_mutation else Fm.EDGES):
        if mutate not in Fm.ACTS_ON[c['kernel']]:
            continue
        if mutate == 'tail_words' and not (c['I'] & 15):
            continue
        if mutate in ('reset_acc', 'drop_last_row', 'no_toggle') and not c['grad']:
            names = tuple(k for k in NAMES[mutate] if k.startswith('S_'))
            if not names:
                continue
        else:
            names = NAMES[mutate]
        case, _, r = run(c, CU if trip_mutation else 256, missing=0.3 if trip_mutation else None, mutate=mutate)
        obs, resp = np.asarray(case['obs']), case['resp']
        if mutate == 'swap_n' and np.all((obs & (resp == 1)).sum(1) == (obs & (resp != 1)).sum(1)):
            continue
        if mutate == 'no_prior' and (c['drop'] or obs.all()):
            continue
        if not any(k in r for k in names):
            continue                                     # (a 3PL cell next to a clamp: S_LL is not asserted on that launch)
        worst = max(r.get(k, 0.0) for k in names)
        assert worst >= 4.0, (mutate, Fm.case_id(c), r)
        least, n = min(least, worst), n + 1
    assert n == ACTING[mutate], (mutate, n)              # a generator change that made cases inapplicable would show here
    assert least >= 1e3, (mutate, least)
    print(mutate, 'cases', n, 'least worst ratio', least)


def test_geometry_follows_the_planner_source():
    """Nothing in the C ABI exposes a grid (vibo_plan_kernel returns the kernel's name alone), so the geometry is held against
    figures worked out by hand from vibo_planner.hip, vibo_row_kernel.hip and vibo_general.hip at 256 CUs."""
    p = Fm.tiled_plan(229445, 7, 1, 256)
    assert (p['waves'], p['lds_main'], p['lds'], p['per_cu']) == (2, 9216, 22784, 7) and p['grid'] == 1792 and p['trips'] == (2, 3)
    assert 229445 == Fm.multi_trip_persons('tiled', 7, 1, 256)
    p = Fm.tiled_plan(32837, 513, 8, 256)
    assert (p['waves'], p['SB'], p['CMAX'], p['lds_stride'], p['per_cu'], p['grid'], p['trips']) == (16, 4, 4, 1040, 1, 256, (2, 3))
    assert Fm.tiled_plan(150, 150, 4, 256)['grid'] == 3 and Fm.tiled_plan(150, 150, 4, 256)['trips'] == (1, 1)
    assert [Fm.tiled_plan(64, I, 1, 256)['waves'] for I in (144, 145, 304, 305, 512, 513)] == [2, 4, 4, 8, 8, 16]
    p = Fm.row_plan(8197, 516, 256)
    assert (p['grid'], p['n_waves'], p['CH'], p['trips']) == (512, 2048, 4, (4, 5))
    assert Fm.row_plan(150, 192, 256)['trips'] == (0, 1) and [Fm.row_plan(9, I, 256)['CH'] for I in (256, 260, 512, 516)] == [1, 2, 2, 4]
    for I, k, lds in ((602, 4, True), (603, 2, True), (1204, 2, True), (1205, 1, True), (2258, 1, True), (2259, 4, False)):
        p = Fm.general_plan(10 ** 6, I, 17, True, 256)
        assert (p['per_cu'], p['item_in_lds']) == (k, lds), (I, p)
    assert Fm.general_plan(8197, 7, 13, True, 256)['trips'] == (2, 3) and Fm.general_plan(200, 7, 13, True, 256)['trips'] == (1, 1)
    assert Fm.general_plan(37, 2259, 17, False, 256)['item_in_lds'] is False
    assert Fm.lds_regimes_met(256) and Fm.lds_regimes_met(1)         # k = 4 with the slab, k = 1 with it, and no slab: each multi-trip
    for c in Fm.TRIPS:
        lo, hi = Fm.plan_of(c, Fm.persons(c, 256), 256)['trips']
        assert lo >= 2 and hi >= 3, (Fm.case_id(c), lo, hi)
