"""CPU checks of oracle/narrow_model.py: the float32 emulation of the narrow-row kernel's statements stays inside the a-priori bound
of EVERY output entry at every width 4..128, ability_dim 1..4 and input class; each mutation of the emulation leaves a bound by a
clear factor; the fp64 values the bounds are centred on are the table oracle's; the generators reach the regimes they are named
after, per sweep over the 125 widths.  tests/test_gpu_narrow_cells.py asserts the same bounds on the kernel."""
import numpy as np
import pytest
import torch

from oracle import narrow_model as N
from oracle import split_model as M
from oracle import vibo_table_ref as T

CLASSES = ('cancel', 'hostile', 'bias', 'onepl', 'threepl', 'clamp3')
WIDTHS = range(4, 129)
B_CYCLE = (1, 2, 3, 5, 9)
SHARE_L3 = {'cancel': 0.8, 'hostile': 0.8, 'onepl': 0.8, 'threepl': 0.8, 'bias': 0.7}


def problem(cls, A, I, drop=False):
    B = B_CYCLE[I % 5]
    if drop:
        B = min(B, I)                      # --drop-missing leaves a person without answers no posterior at all
    return N.make_problem(cls, A, B, I, seed=1000 * A + I, shift=I % 3, drop_missing=drop, unobserved=(I // 2,) if I % 7 == 3 and not drop else ())


def run(cls, A, I, mutate=None, drop=False, want_grad=True):
    case, table, eps = problem(cls, A, I, drop)
    B = case['resp'].shape[0]
    em = N.emulate(case, table, eps, drop_missing=drop, want_grad=want_grad, mutate=mutate)
    exp = N.expected(case, table, eps, em['theta'], grid=N.grid_blocks(B, A, I, case['irt'], want_grad, 256), drop_missing=drop)
    return case, exp, N.ratios(exp, em, case['irt'], A)


@pytest.mark.parametrize('A', [1, 2, 3, 4])
@pytest.mark.parametrize('cls', CLASSES)
def test_emulation_stays_inside_every_bound_at_every_width(cls, A):
    worst, n_l3, n_obs, n_excl = {}, 0, 0, 0
    for I in WIDTHS:
        case, exp, r = run(cls, A, I)
        for k, v in r.items():
            assert v <= 1.0, (cls, A, I, k, v)
            worst[k] = max(worst.get(k, 0.0), v)
        n_obs += int(case['obs'].sum())
        n_excl += int(exp['excluded'].sum())
        if 'logit_share' in exp:
            n_l3 += exp['logit_share'][0]
        elif cls == 'threepl':
            n_l3 += int((np.abs(exp['ref']['logit'][case['obs'][case['obs'].any(1)]]) <= 3.0).sum())
    print(cls, A, {k: round(v, 3) for k, v in worst.items()})
    assert max(worst.values()) > 0.02                   # the bounds are not orders of magnitude above the emulation's worst entry
    # the generators reach their regime, per sweep (a 4-item case has too few cells to say)
    if cls in SHARE_L3:
        assert n_l3 / n_obs >= SHARE_L3[cls], (cls, A, n_l3 / n_obs)
    if cls == 'clamp3':
        assert n_excl <= 0.02 * n_obs, (n_excl, n_obs)
    else:
        assert n_excl == 0


@pytest.mark.parametrize('cls', ['cancel', 'threepl'])
def test_emulation_with_drop_missing_and_forward_only(cls):
    for I in WIDTHS:
        _, _, r = run(cls, 3, I, drop=True)
        assert max(r.values()) <= 1.0, (I, r)
        _, _, r = run(cls, 3, I, want_grad=False)
        assert max(r.values()) <= 1.0 and 'dLL/db' not in r, (I, r)


# mutation -> (class, ability_dim, the observables one of which has to leave its bound, widths)
MUTATION_PLAN = {
    'tail': ('cancel', 2, ('mu', 'logvar', 'S_NOBS', 'S_LL'), [I for I in WIDTHS if I & 3]),
    'swap_n': ('cancel', 2, ('mu', 'theta'), list(WIDTHS)),
    'no_prior': ('hostile', 1, ('logvar', 'mu'), list(WIDTHS)),
    'guess_row': ('threepl', 3, ('dLL/dguess', 'dLL/db'), list(WIDTHS)),
    'drop_group': ('cancel', 4, ('dLL/db', 'dLL/da'), [I for I in WIDTHS if B_CYCLE[I % 5] >= 5]),
}


@pytest.mark.parametrize('mutate', N.MUTATIONS)
def test_every_mutation_of_the_emulation_leaves_a_bound_by_a_factor_of_four(mutate):
    """At EVERY width of the plan, not only in the worst case over them: a width the GPU sweep did not run would hide it."""
    cls, A, names, widths = MUTATION_PLAN[mutate]
    least = np.inf
    for I in widths:
        case, _, r = run(cls, A, I, mutate=mutate)
        if mutate == 'swap_n' and np.all((case['obs'] & (case['resp'] == 1)).sum(1) == (case['obs'] & (case['resp'] != 1)).sum(1)):
            continue                                     # (as many right as wrong answers for every person: nothing to swap)
        if mutate == 'no_prior' and case['obs'].all():
            continue                                     # (B = 1: the one person answers every item, the prior term is zero)
        if mutate == 'drop_group' and not (case['p_obs'] % 4 == 3).any():
            continue
        least = min(least, max(r[k] for k in names))
        assert max(r[k] for k in names) >= 4.0, (mutate, I, r)
    print(mutate, 'least worst ratio over the widths', least)


@pytest.mark.parametrize('irt,cls', [(1, 'onepl'), (2, 'cancel'), (3, 'threepl')])
@pytest.mark.parametrize('drop', [False, True])
def test_reference_values_are_the_table_oracles(irt, cls, drop):
    """The fp64 values the bounds are centred on, against oracle/vibo_table_ref.py on the same inputs (its 1e-8 is a double, the kernel's
    a float: agreement to 1e-9, far below any bound)."""
    A, I, B = 3, 37, 9
    case, table, eps = N.make_problem(cls, A, B, I, seed=5, drop_missing=drop)
    theta = M.f32(case['theta_oracle'])
    exp = N.expected(case, table, eps, theta, grid=1, drop_missing=drop)
    td = lambda x: torch.from_numpy(np.asarray(x, np.float64))
    ref = T.fused_elbo_ref(td(table), td(M.item_tensor(case)), td(case['resp']), torch.from_numpy(case['obs']), td(eps), irt_model=irt,
                           ability_dim=A, replace_missing_with_prior=not drop, mode='kl')
    close = lambda a, b: np.abs(np.asarray(a) - np.asarray(b)).max() <= 1e-9 * max(1.0, np.abs(np.asarray(b)).max())
    assert close(exp['mu'][0], ref['ability_mu']) and close(exp['logvar'][0], ref['ability_logvar']) and close(exp['theta'][0], ref['ability'])
    assert close(exp['S_KL'][0], ref['kl_ability']) and close(exp['S_LOGQ0'][0], ref['logq0'])
    assert close(exp['grad_table(1)'][0], ref['g_table'][1])
    # the cell part is evaluated at the fp32 theta: 6e-8 relative away from the oracle's fp64 sample
    near = lambda a, b: np.abs(np.asarray(a) - np.asarray(b)).max() <= 1e-5 * max(1.0, np.abs(np.asarray(b)).max())
    gi = ref['g_item'].numpy()
    assert near(exp['dLL/db'][0], gi[:, 0 if irt == 1 else A]) and near(exp['grad_table(0)'][0], ref['g_table'][0])
    assert near(exp['S_LL'][0], ref['ll']) and near(exp['S_LOGP'][0], ref['logp'])
    if irt != 1:
        assert near(exp['dLL/da'][0], gi[:, :A])
    if irt == 3:
        assert near(exp['dLL/dguess'][0], gi[:, A + 1])


def test_geometry_follows_the_planner():
    assert N.grid_blocks(16, 1, 100, 2, True, 256) == 1 and N.grid_blocks(8000, 1, 100, 2, True, 256) == 500
    assert N.grid_blocks(32645, 4, 128, 2, True, 256) == 512 and N.grid_blocks(32645, 1, 64, 2, True, 256) == 1020
    assert N.units_per_wave(32645, 1020) == 3 and N.units_per_wave(32645, 512) == 4 and N.units_per_wave(9, 1) == 1


@pytest.mark.parametrize('cls,A,I', [('cancel', 1, 61), ('onepl', 2, 128), ('threepl', 3, 95), ('cancel', 4, 64)])
def test_emulation_over_several_units_per_wave_with_the_counted_chain(cls, A, I):
    """A dense problem (30 % missing) on a one-CU grid: 301 persons are 76 units over 8 ... 16 waves, so every accumulator is carried
    over five to ten loop trips and the last unit holds one row; the summed bounds with the chain counted from the reduction hold."""
    B = 301
    case, table, eps = N.make_problem(cls, A, B, I, seed=40 + I + A, missing=0.3)
    grid = N.grid_blocks(B, A, I, case['irt'], True, 1)
    assert N.units_per_wave(B, grid) >= 5
    em = N.emulate(case, table, eps, num_cu=1)
    r = N.ratios(N.expected(case, table, eps, em['theta'], grid=grid), em, case['irt'], A)
    assert max(r.values()) <= 1.0, r
    bad = N.ratios(N.expected(case, table, eps, em['theta'], grid=grid), N.emulate(case, table, eps, num_cu=1, mutate='drop_group'), case['irt'], A)
    assert bad['dLL/db'] >= 4.0, bad
