"""The narrow-row kernel (csrc/vibo_narrow.hip), output by output, at every width.

tests/test_gpu_narrow.py compares aggregates on N(0, 1) inputs at 11 item counts; here EVERY entry of every output is held to a bound
of its own, derived in oracle/narrow_model.py from the kernel's statements and the inputs alone (the float32 emulation of those
statements is held to the same bounds in tests/test_narrow_model.py, where each mutation of it leaves one).  No kernel pin
(ops.DESC_FLAGS == 0): every launch asserts that the planner chose the narrow-row kernel.  theta is what the kernel returns
(raw.ability), checked per entry against the per-person model; the difficulties are set from the fp64 product of experts' theta and
the cell reference is built from the kernel's.  eps != 0, so sigma eps is in play.

 (a) width sweep: per (input class, ability_dim 1..4, row mode) ALL item counts 4..128 at B = (1, 2, 3, 5, 9)[I % 5] persons -- units of
     one to three rows, and at B = 5 and 9 a second and third unit with a ragged last one --, one observer per item (every seventh
     width leaves one item without any: exact zeros).  Per launch: d LL/d b, the logit behind it where |l| <= 3, d LL/d a,
     d LL/d guess, mu, logvar, theta, both table-gradient heads, S_LL, S_KL, S_LOGQ0, S_LOGP against their bounds; S_NOBS and every
     entry whose reference is an exact zero exactly; the forward-only launch of the same case returns the same posterior bit for bit
     and an S_LL inside its bound.  --drop-missing: the 2PL and 3PL classes at ability_dim 3 (B capped at I: a person without answers
     has no posterior there).
 (b) padding: the cells between a row's end and its stride hold NaN responses under mask bytes 1, resp. code bytes 0 and 1; every
     output is bit for bit that of zero / "missing" padding.
 (c) more than one unit per wave: B = 2 x 16 x 1020 + 5 persons, above twice any grid the planner returns, so that every wave takes
     two or three units (the prefetch into the registers the pack freed, accumulators carried over loop trips) and the last unit
     holds one row.  PAIRS: every pair of values of (template width, item count 61 / 64 / 95 / 128, link, row mode, gradients or
     forward only) occurs; per case the observers sit in the first unit, in a later one and at the ragged end; all 32 645 x A
     posterior entries are held to their bounds and are bit for bit those of the same rows launched in slices of 4 096
     (single-unit launches: the per-person math does not depend on the unit).  One dense launch (30 % missing) per template width and
     items-per-lane form against the summed bounds with the counted chain.

VIBO_TOL_RECORD=path appends the worst error / bound per observable (gpu_common.record, kind 'narrow_cells');
tools/split_record_table.py narrow_cells turns the file into profiles/narrow_cells_record.txt.  The assertions hold either way."""
import dataclasses
import itertools

import numpy as np
import pytest
import torch

from gpu_common import dev, launch_elbo, record
from oracle import narrow_model as N
from oracle import split_model as M
from vibo_amd import _lib, ops
from vibo_amd.ops import ElboSpec

pytestmark = pytest.mark.gpu

NARROW = 'narrow rows (narrow_kernel)'
CLASSES = ('cancel', 'hostile', 'bias', 'onepl', 'threepl', 'clamp3')
B_CYCLE = (1, 2, 3, 5, 9)
ROWS = ('direct', 'gather', 'codes')


def _num_cu():
    return torch.cuda.get_device_properties(dev()).multi_processor_count


def _rows(case, rows):
    """-> (resp, mask, row_index) host tensors of the launch; gather / gcodes: the rows scattered over a matrix with 7 decoys."""
    resp, mask = torch.from_numpy(case['resp']), torch.from_numpy(np.asarray(case['obs'], bool))
    if rows not in ('gather', 'gcodes'):
        return resp, mask, None
    B, I = resp.shape
    P = B + 7
    index = torch.randperm(P, generator=torch.Generator().manual_seed(B + I))[:B]
    resp_all = (torch.rand(P, I, generator=torch.Generator().manual_seed(I)) < 0.5).float()
    mask_all = torch.ones(P, I, dtype=torch.bool)
    resp_all[index], mask_all[index] = resp, mask
    return resp_all, mask_all, index


def _launch(case, table, eps, rows, drop=False, want_grad=True):
    assert ops.DESC_FLAGS == 0
    A = case['a'].shape[1]
    spec = ElboSpec(irt_model=case['irt'], ability_dim=A, drop_missing=drop)
    resp, mask, index = _rows(case, rows)
    codes = rows in ('codes', 'gcodes')
    raw = launch_elbo(spec, resp, mask, torch.from_numpy(table), torch.from_numpy(M.item_tensor(case)), torch.from_numpy(eps),
                      row_index=index, pad=not codes, codes=codes, want_grad=want_grad, kernel=NARROW)
    return spec, raw


def _outputs(spec, raw, I, want_grad=True):
    """The launch's outputs on the host, in the form narrow_model.emulate returns them."""
    host = dataclasses.replace(raw, flat=raw.flat.cpu())
    sc = host.scalars.numpy()
    out = dict(mu=raw.ability_mu.cpu().numpy(), logvar=raw.ability_logvar.cpu().numpy(), theta=raw.ability.cpu().numpy(),
               ll=sc[_lib.S_LL], kl=sc[_lib.S_KL], logq0=sc[_lib.S_LOGQ0], logp=sc[_lib.S_LOGP], nobs=sc[_lib.S_NOBS])
    if want_grad:
        out['g_item'] = host.grad_item((I, spec.item_dim)).numpy()
        out['g_table'] = [host.grad_table(s).numpy() for s in range(2)]
    return out


def _worse(worst, r):
    for k, v in r.items():
        worst[k] = max(worst.get(k, 0.0), v)


def _report(part, cls, A, rows, worst, **extra):
    for k, v in sorted(worst.items()):
        record('narrow_cells', v, part=part, **{'class': cls}, A=A, rows=rows, observable=k, ratio=v, **extra)
    print(part, cls, A, rows, {k: round(v, 3) for k, v in worst.items()})


# ---------------------------------------------------------------------------------------------------------------------------
# (a) every width
# ---------------------------------------------------------------------------------------------------------------------------
SWEEP = [(cls, A, rows, False) for cls in CLASSES for A in (1, 2, 3, 4) for rows in ROWS] + \
        [(cls, 3, 'direct', True) for cls in ('cancel', 'hostile', 'bias', 'threepl', 'clamp3')]


@pytest.mark.parametrize('cls,A,rows,drop', SWEEP, ids=[f'{c}-A{a}-{r}' + ('-drop' if d else '') for c, a, r, d in SWEEP])
def test_every_width_entry_by_entry(cls, A, rows, drop):
    worst, worst_fwd, failed = {}, {}, []
    n_obs = n_excl = 0
    cu = _num_cu()
    for I in range(4, 129):
        B = B_CYCLE[I % 5]
        if drop:
            B = min(B, I)
        case, table, eps = N.make_problem(cls, A, B, I, seed=1000 * A + I, shift=I % 3, drop_missing=drop,
                                          unobserved=(I // 2,) if I % 7 == 3 and not drop else ())
        spec, raw = _launch(case, table, eps, rows, drop)
        got = _outputs(spec, raw, I)
        assert np.abs(got['theta'] - case['theta_oracle']).max() < 2e-5 * max(1.0, np.abs(case['theta_oracle']).max())
        exp = N.expected(case, table, eps, got['theta'], grid=N.grid_blocks(B, A, I, case['irt'], True, cu), drop_missing=drop)
        r = N.ratios(exp, got, case['irt'], A)
        _worse(worst, r)
        n_obs, n_excl = n_obs + int(case['obs'].sum()), n_excl + int(exp['excluded'].sum())
        # forward only: another instantiation; the same posterior bit for bit, S_LL and the three other heads inside their bounds
        _, fwd = _launch(case, table, eps, rows, drop, want_grad=False)
        gf = _outputs(spec, fwd, I, want_grad=False)
        same = all(np.array_equal(gf[k], got[k]) for k in ('mu', 'logvar', 'theta'))
        expf = N.expected(case, table, eps, got['theta'], grid=N.grid_blocks(B, A, I, case['irt'], False, cu), drop_missing=drop)
        rf = N.ratios(expf, gf, case['irt'], A)
        _worse(worst_fwd, rf)
        if max(r.values()) > 1.0 or max(rf.values()) > 1.0 or not same:
            failed.append((I, B, {k: v for k, v in {**r, **{'fwd ' + k: v for k, v in rf.items()}}.items() if v > 1.0}, same))
    _report('sweep', cls + ('/drop' if drop else ''), A, rows, worst)
    _report('sweep-forward', cls + ('/drop' if drop else ''), A, rows, worst_fwd)
    assert n_excl <= 0.02 * n_obs, (n_excl, n_obs)          # 3PL cells within 4 ulp of a clamp value are not asserted: at most 2 %
    assert not failed, failed


# ---------------------------------------------------------------------------------------------------------------------------
# (b) padding is never interpreted
# ---------------------------------------------------------------------------------------------------------------------------
def _bits_equal(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in
               ((a.flat, b.flat), (a.ability_mu, b.ability_mu), (a.ability_logvar, b.ability_logvar), (a.ability, b.ability)))


def _launch_rows(spec, r, m, index, table, item, eps, want_grad):
    """ops._hip_launch_elbo on device rows exactly as they are (no repacking: the padding under test has to survive)."""
    assert ops.DESC_FLAGS == 0
    r2, m2, code = ops.prepare_rows(r, m)
    if not isinstance(r, ops.CellCodes):
        assert r2.data_ptr() == r.data_ptr() and m2.data_ptr() == m.data_ptr()
    B = int(index.numel()) if index is not None else r2.shape[0]
    assert ops.plan_kernel(spec, B, r2.shape[1], code, want_grad) == NARROW
    raw = ops._hip_launch_elbo(spec, r2, m2, code, index, table, item, eps, None, _lib.REG_KL, want_grad, B)
    torch.cuda.synchronize()
    return raw


PADDING = [(irt, A, I, rows) for (irt, A), I in zip(itertools.cycle([(2, 1), (3, 3), (1, 3), (3, 1), (2, 3), (1, 1)]),
                                                   (5, 6, 7, 61, 62, 63, 66, 95, 101, 126, 127, 9)) for rows in ('direct', 'gather', 'codes')]


@pytest.mark.parametrize('irt,A,I,rows', PADDING, ids=[f'{i}pl-A{a}-I{n}-{r}' for i, a, n, r in PADDING])
def test_padding_cells_are_never_interpreted(irt, A, I, rows):
    assert I % 4 and I % 16
    d = dev()
    B, P = 23, 31
    g = torch.Generator().manual_seed(I * 10 + A)
    spec = ElboSpec(irt_model=irt, ability_dim=A)
    resp = (torch.rand(P, I, generator=g) < 0.5).float()
    mask = torch.rand(P, I, generator=g) < 0.8
    table = (torch.randn(2, 2 * A, generator=g) * 0.7).to(d)
    item = torch.randn(I, spec.item_dim, generator=g).to(d)
    eps = torch.randn(B, A, generator=g).to(d)
    index = torch.randperm(P, generator=g)[:B].to(d) if rows == 'gather' else None
    if index is None:
        resp, mask = resp[:B], mask[:B]
    n = resp.shape[0]
    for want_grad in (True, False):
        if rows == 'codes':
            base = launch_elbo(spec, resp, mask, table, item, eps, codes=True, want_grad=want_grad, kernel=NARROW)
            I16 = (I + 15) // 16 * 16
            buf = torch.empty(n, I16, dtype=torch.uint8)
            buf[:] = (torch.arange(I16) & 1).to(torch.uint8)[None, :]                    # code bytes 0 and 1: answered wrong / right
            buf[:, :I] = torch.where(mask, resp.to(torch.uint8), torch.full((), 2, dtype=torch.uint8))
            buf = buf.to(d)
            out = _launch_rows(spec, ops.CellCodes(buf[:, :I]), None, index, table, item, eps, want_grad)
        else:
            base = launch_elbo(spec, resp, mask, table, item, eps, row_index=index, pad=True, want_grad=want_grad, kernel=NARROW)
            I4 = (I + 3) // 4 * 4
            rbuf, mbuf = torch.full((n, I4), float('nan')), torch.ones(n, I4, dtype=torch.uint8)
            rbuf[:, :I], mbuf[:, :I] = resp, mask.to(torch.uint8)
            rbuf, mbuf = rbuf.to(d), mbuf.to(d)
            out = _launch_rows(spec, rbuf[:, :I], mbuf[:, :I], index, table, item, eps, want_grad)
        assert torch.isfinite(out.flat).all() if want_grad else torch.isfinite(out.scalars).all()
        if want_grad:
            assert _bits_equal(out, base), (irt, A, I, rows)
        else:
            assert torch.equal(out.scalars.view(torch.int32), base.scalars.view(torch.int32)) and torch.equal(out.ability, base.ability)


# ---------------------------------------------------------------------------------------------------------------------------
# (c) more than one unit per wave
# ---------------------------------------------------------------------------------------------------------------------------
B_BIG = 2 * 16 * 1020 + 5
FACTORS = ((1, 2, 3), (61, 64, 95, 128), (1, 2, 3), ('direct', 'gather', 'codes', 'gcodes'), (True, False))


def _pairwise(factors):
    """A small set of combinations in which every pair of values of two factors occurs (greedy, deterministic)."""
    need = {(i, a, j, b) for i, j in itertools.combinations(range(len(factors)), 2) for a in factors[i] for b in factors[j]}
    pairs = lambda c: {(i, c[i], j, c[j]) for i, j in itertools.combinations(range(len(c)), 2)}
    chosen = []
    while need:
        best = max(itertools.product(*factors), key=lambda c: len(pairs(c) & need))
        chosen.append(best)
        need -= pairs(best)
    return chosen


PAIRS = _pairwise(FACTORS)
CLS_OF = {1: 'onepl', 2: 'cancel', 3: 'threepl'}


def test_the_plan_meets_every_pair_and_the_second_unit():
    assert len(PAIRS) <= 20
    seen = {(i, c[i], j, c[j]) for c in PAIRS for i, j in itertools.combinations(range(5), 2)}
    assert all((i, a, j, b) in seen for i, j in itertools.combinations(range(5), 2) for a in FACTORS[i] for b in FACTORS[j])
    cu = _num_cu()
    for A, I, irt, _, grad in PAIRS:
        grid = N.grid_blocks(B_BIG, A, I, irt, grad, cu)
        assert B_BIG > 2 * 16 * grid and grid <= 1020 and N.units_per_wave(B_BIG, grid) >= 3
    assert (B_BIG - 1) % 4 == 0                                # the last unit holds one row


def _slices_bit_identical(case, table, eps, rows, want_grad, full):
    """The posterior of the same rows in launches of 4 096 (one unit per wave)."""
    for lo in range(0, B_BIG, 4096):
        sl = slice(lo, min(B_BIG, lo + 4096))
        part = dict(case, resp=case['resp'][sl], obs=case['obs'][sl])
        _, raw = _launch(part, table, eps[sl], rows, want_grad=want_grad)
        for k, t in (('mu', raw.ability_mu), ('logvar', raw.ability_logvar), ('theta', raw.ability)):
            if not np.array_equal(t.cpu().numpy(), full[k][sl]):
                return False
    return True


@pytest.mark.parametrize('A,I,irt,rows,grad', PAIRS, ids=[f'A{a}-I{i}-{m}pl-{r}-{"grad" if g else "forward"}' for a, i, m, r, g in PAIRS])
def test_more_than_one_unit_per_wave(A, I, irt, rows, grad):
    cu = _num_cu()
    grid = N.grid_blocks(B_BIG, A, I, irt, grad, cu)
    assert B_BIG > 2 * 16 * 1020 >= 2 * 16 * grid             # precondition: every wave takes at least two units
    worst, failed = {}, []
    for shift in (0, 16 * 1020 + 3, B_BIG - I):
        case, table, eps = N.make_problem(CLS_OF[irt], A, B_BIG, I, seed=7000 + 10 * I + A, shift=shift)
        assert case['p_obs'].min() == shift and case['p_obs'].max() == shift + I - 1
        spec, raw = _launch(case, table, eps, rows, want_grad=grad)
        got = _outputs(spec, raw, I, want_grad=grad)
        exp = N.expected(case, table, eps, got['theta'], grid=grid)
        r = N.ratios(exp, got, irt, A)
        _worse(worst, r)
        same = _slices_bit_identical(case, table, eps, rows, grad, got)
        if max(r.values()) > 1.0 or not same:
            failed.append((shift, {k: v for k, v in r.items() if v > 1.0}, same))
    _report('units', CLS_OF[irt], A, rows, worst, I=I, grad=grad)
    assert not failed, failed


DENSE = [(1, 61, 'cancel'), (1, 128, 'onepl'), (2, 61, 'onepl'), (2, 128, 'cancel'), (3, 61, 'cancel'), (3, 128, 'cancel')]


@pytest.mark.parametrize('A,I,cls', DENSE, ids=[f'A{a}-I{i}-{c}' for a, i, c in DENSE])
def test_dense_launch_over_several_units_with_the_counted_chain(A, I, cls):
    """30 % missing, every item observed by ~23 000 persons spread over all the waves' units: each gradient entry against the sum of its
    cells' bounds plus the chain counted from the kernel (units per wave + two shuffles + four waves + the record sum)."""
    case, table, eps = N.make_problem(cls, A, B_BIG, I, seed=9000 + I + A, missing=0.3)
    spec, raw = _launch(case, table, eps, 'direct')
    got = _outputs(spec, raw, I)
    exp = N.expected(case, table, eps, got['theta'], grid=N.grid_blocks(B_BIG, A, I, case['irt'], True, _num_cu()))
    r = N.ratios(exp, got, case['irt'], A)
    r.pop('logit', None)
    _report('dense', cls, A, 'direct', r, I=I)
    assert max(r.values()) <= 1.0, r
