"""Planar flows inside the two row-split ELBO kernels when a workgroup takes a second and a third batch (flow_batches_common.py: the
cases, the planner's grids restated, the person-sliced fp64 oracle; tests/test_flow_batches_model.py admits every case on the CPU).

No other launch of the suite gives a workgroup of either kernel a second batch with flows on, so the state those kernels carry over
their batch loop -- the matrix kernel's tps / facc / lacc by batch parity, the VALU kernel's SplitFlowAcc and per-wave log-det sum,
the partial last batch's `live` factors, the primary panel's ownership of the regulariser -- ran under no test.  Per case:

 1. every reduction against the float64 oracle at the bounds test_general_kernel_vs_oracle holds (gpu_common.compare_raw, TOL_GRAD
    for the flow gradients), and every (set, flow, uhat | w | b) block of the flow gradients on its own, over the block's
    max_e sum_batches |batch contribution| -- a `b` gradient of one number per flow does not hide under the uhat block's scale;
 2. the per-person outputs bit for bit against launches of G x R persons each (one batch per workgroup, every row in the workgroup,
    lane and batch offset it has in the long launch);
 3. a second identical launch gives equal bits on every output: the records of both kernels are summed in a fixed order
    (vibo_helpers.hip finalize_kernel) and neither kernel's flow accumulators are shared between lanes out of order -- the matrix
    kernel's facc has one owner lane per address and batch parity, the VALU kernel's SplitFlowAcc one lane of wave 0 per address.

Forward-only cases: the scalars and the per-person outputs, by the same comparisons."""
import functools

import pytest
import torch

import flow_batches_common as Fb
from conftest import rel_err
from gpu_common import TOL_GRAD, check, compare_raw, dev, launch_elbo, record
from oracle import vibo_table_ref as T
from vibo_amd import _lib, ops
from vibo_amd.ops import ElboSpec

pytestmark = pytest.mark.gpu

PER_PERSON = ('ability_mu', 'ability_logvar', 'ability', 'ability_k', 'ability_ladj')


def cus():
    return torch.cuda.get_device_properties(dev()).multi_processor_count


def spec_of(c):
    return ElboSpec(irt_model=c['irt'], ability_dim=c['A'], conditional=c['post'] == 'cond', drop_missing=c['drop'], n_flows=c['flows'],
                    given=c['post'] == 'given')


@functools.lru_cache(maxsize=2)
def device_problem(key):
    """The problem's tensors on the device, uploaded once per problem (the tests of a case follow each other) and never written."""
    p = Fb._problem(key)
    d = {k: p[k].to(dev()) for k in ('table', 'item', 'eps', 'flow')}
    if p['case']['rows'] == 'gathered':
        d.update(resp=p['big_resp'].to(dev()), mask=p['big_mask'].to(dev()), where=p['where'].to(dev()))
    else:
        d.update(resp=p['resp'].to(dev()), mask=p['mask'].to(dev()).bool())
    return d


def launch(c, p, sl=slice(None)):
    """The case's launch on the persons `sl` of its problem: the same pin and row mode, the matching part of eps (and of the
    caller-supplied posterior), the planner's choice asserted."""
    d = device_problem(Fb.problem_key(c, cus()))
    given, gathered = c['post'] == 'given', c['rows'] == 'gathered'
    with ops.desc_flags(c['pin']):
        return launch_elbo(spec_of(c), d['resp'] if gathered else d['resp'][sl], d['mask'] if gathered else d['mask'][sl],
                           d['table'][sl] if given else d['table'], d['item'], d['eps'][sl], row_index=d['where'][sl] if gathered else None,
                           codes=c['rows'] == 'codes', flow=d['flow'], reg_mode=_lib.REG_SAMPLED, want_grad=c['want_grad'],
                           kernel=Fb.KERNEL[c['engine']])


@functools.lru_cache(maxsize=2)
def whole_launch(name):
    """(case, problem, grid, outputs of the launch over all persons) -- one launch per case, shared by its tests."""
    c = next(c for c in Fb.CASES if c['name'] == name)
    p = Fb.problem(c, cus())
    G, R = Fb.grid_of(c, cus(), p['B']), Fb.ROWS[c['engine']]
    # the batch pattern of the case on this device: workgroup 0 takes a second batch (M1: a third), the last batch is partial
    a, b = c['pattern']
    assert G == Fb.grid_of(c, cus()) and Fb.ceil_div(p['B'], R) == a * G + b + 1 and p['B'] % R == Fb.TAIL[c['engine']]
    assert len(Fb.batches_of(p['B'], G, R)) == (3 if (a, b) == (2, 1) else 2)
    return c, p, G, launch(c, p)


def outputs(c, raw):
    out = {k: getattr(raw, k) for k in PER_PERSON}
    if c['want_grad'] and c['post'] == 'given':
        out.update({f'given_grad[{s}]': raw.grad_table(s) for s in range(2)})
    return out


def note(c, observable, err, tol):
    record('flow_batches', err, tol, case=c['name'], kernel=c['engine'], observable=observable, ratio=err / tol)


@pytest.mark.parametrize('name', [c['name'] for c in Fb.CASES])
def test_reductions_against_the_sliced_oracle(name):
    c, p, G, raw = whole_launch(name)
    ref, A, I = p['ref'], c['A'], c['I']
    sc = raw.scalars.cpu().double()
    one = lambda k: max(1.0, abs(float(ref[k])))
    note(c, 'S_LL', rel_err(sc[_lib.S_LL], ref['ll']), Fb.TOL_SCALAR)
    for k, i in (('reg', _lib.S_REG), ('kl_ability', _lib.S_KL), ('logq0', _lib.S_LOGQ0), ('logp', _lib.S_LOGP)):
        note(c, 'S_' + k, abs(float(sc[i]) - float(ref[k])) / one(k), Fb.TOL_SCALAR)
    for k in ('ability_mu', 'ability_logvar', 'ability'):
        note(c, k, float((getattr(raw, k).cpu().double() - ref[k]).abs().max()) / max(1.0, float(ref[k].abs().max())), Fb.TOL_PERSON)
    e_k = float((raw.ability_k.cpu().double() - ref['ability_k']).abs().max())
    e_ladj = float((raw.ability_ladj.cpu().double() - ref['ladj']).abs().max())
    e_sum = abs(float(sc[_lib.S_LADJ]) - float(ref['ladj_sum'])) / one('ladj_sum')
    note(c, 'ability_k', e_k, Fb.TOL_FLOW_PERSON)
    note(c, 'ability_ladj', e_ladj, Fb.TOL_FLOW_PERSON)
    note(c, 'S_LADJ', e_sum, Fb.TOL_LADJ_SUM)
    if c['want_grad']:
        note(c, 'g_item', rel_err(raw.grad_item((I, spec_of(c).item_dim)).cpu(), ref['g_item']), TOL_GRAD)
        for s in range(2):
            note(c, 'given_grad' if c['post'] == 'given' else 'g_table', rel_err(raw.grad_table(s).cpu(), ref['g_table'][s]), TOL_GRAD)
    compare_raw(raw, ref, (I, spec_of(c).item_dim), want_grad=c['want_grad'])
    assert e_k < Fb.TOL_FLOW_PERSON and e_ladj < Fb.TOL_FLOW_PERSON and e_sum < Fb.TOL_LADJ_SUM, (e_k, e_ladj, e_sum)
    if not c['want_grad']:
        return
    got = torch.stack([raw.grad_flow(s).cpu() for s in range(2)]).view(2, c['flows'], 2 * A + 1)
    want = T.flat_flow_grads(ref['g_flow'])
    for s in range(2):
        note(c, 'g_flow', rel_err(got[s], want[s]), TOL_GRAD)
        check(f'g_flow[{s}]', rel_err(got[s], want[s]), TOL_GRAD)
    blocks = Fb.block_errors(got, ref, A)                 # [set, flow, uhat | w | b]
    for k, (kind, _) in enumerate(Fb.flow_blocks(A)):
        note(c, f'g_flow block {kind}', float(blocks[:, :, k].max()), TOL_GRAD)
    assert float(blocks.max()) < TOL_GRAD, blocks


@pytest.mark.parametrize('name', [c['name'] for c in Fb.CASES])
def test_per_person_outputs_equal_one_batch_launches_bit_for_bit(name):
    c, p, G, raw = whole_launch(name)
    R, B = Fb.ROWS[c['engine']], p['B']
    whole = outputs(c, raw)
    n = 0
    for r0 in range(0, B, G * R):
        sl = slice(r0, min(B, r0 + G * R))
        part = outputs(c, launch(c, p, sl))
        for k, t in part.items():
            assert t.shape[0] == sl.stop - sl.start
            assert torch.equal(t, whole[k][sl]), (k, r0, float((t - whole[k][sl]).abs().max()))
        n += 1
    assert n == len(Fb.batches_of(B, G, R))               # as many one-batch launches as workgroup 0 has batches


@pytest.mark.parametrize('name', [c['name'] for c in Fb.CASES])
def test_second_launch_gives_the_same_bits(name):
    c, p, G, raw = whole_launch(name)
    again = launch(c, p)
    flat = (lambda r: r.flat) if c['want_grad'] else (lambda r: r.scalars)      # (forward only: the gradients are not written)
    assert torch.equal(flat(again), flat(raw))
    for k in PER_PERSON:
        assert torch.equal(getattr(again, k), getattr(raw, k)), k
