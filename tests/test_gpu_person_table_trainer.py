"""The native VI / MLE train step (trainer.FusedVITrainer / FusedMLETrainer, include/vibo_hip_person_tables.h) on the GPU.
  1. three steps against float64: loss, every gradient tensor (read back from Adam's first moments, rows outside the minibatch exactly
     zero), Adam's update and second-moment recurrence on EVERY row of the tables (persons visited at step 1 and not at step 2 move on
     momentum) -- the protocol and bounds of test_gpu_trainer_gradients.py, inputs admitted by test_person_table_trainer_host.py
  2. the table update alone, through vibo_person_table_adam, entry by entry against torch.optim.Adam in float64 on the CPU
  3. four steps beside module + autograd + torch.optim.Adam under the same torch seeds
  4. native noise = vibo_fill_normal's at the step's counter and streams, bit for bit
  5. a captured, replayed step = the eager step, bit for bit
  6. vi.py / mle.py --native-step"""
import copy
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import person_table_common as pt
import trainer_gradient_common as tg
from conftest import rel_err
from gpu_common import TOL_GRAD, assert_same_parameters, dev, fill_normal, noise_counter, record, scattered_rows
from oracle import vibo_oracle as O
from vibo_amd import _lib, config, ops
from vibo_amd.trainer import FusedMLETrainer, FusedTrainer, FusedVITrainer

pytestmark = pytest.mark.gpu

CLASS = {'vi': FusedVITrainer, 'mle': FusedMLETrainer}
MATRIX, VALU = 1, 2                     # VIBO_KERNEL_* of the row-split kernels


# ---------------------------------------------------------------------------
# 1. three steps: loss, gradient, Adam
# ---------------------------------------------------------------------------
def minibatch_rows(p, t, rows_mode, d):
    """-> (response, mask, row_index) of step t.  'dense': the minibatch's own rows, padded as the CLI's resident matrix is;
    'gathered' / 'codes': they sit at scattered places of a larger resident matrix (fp32 rows / cell codes), read by row_index."""
    r, m = p.resp[p.index[t]], p.mask[p.index[t]]
    if rows_mode == 'dense':
        return (*ops.pad_rows(r.to(d), m.to(d)), None)
    big_r, big_m, where = scattered_rows(r, m, 2 * p.B + 5)
    big_r, big_m = ops.pad_rows(big_r.to(d), big_m.to(d))
    if rows_mode == 'codes':
        big_r, big_m = ops.pack_cell_codes(big_r, big_m), None
    return big_r, big_m, where.to(d)


def run_three_steps(method, case, rows_mode='dense', lr=5e-3, kernel=None):
    d = dev()
    p = pt.make_problem(method, *case)
    model = pt.build_model(p, d)
    keys = list(model.state_dict())
    tr = FusedTrainer(model, lr=lr)
    assert type(tr) is CLASS[method] and list(model.state_dict()) == keys
    view = pt.TableView(tr)
    D = O.item_feat_dim(p.irt, p.A)
    person_names, _ = pt.names(method)
    what = f'{method} {pt.ident(case)} {rows_mode}'
    for t in range(3):
        resp, mask, row_index = minibatch_rows(p, t, rows_mode, d)
        if kernel is not None:            # the ELBO kernel this case is pinned to is the one asserted
            r_, m_, code = ops.prepare_rows(resp, mask)
            dsc = ops._rows_desc(model.spec, p.B, r_, m_, code, _lib.REG_KL, True)
            assert _lib.load().vibo_plan_kernel(ctypes.byref(dsc)) == kernel
        before, p_before = (tg.moments(view) if t else None), tg.parameters(view)
        at = {k: v.detach().cpu() for k, v in model.state_dict().items()}       # the parameters the kernel starts this step from
        loss64, want = pt.reference(p, at, t)
        loss = tr.step(resp, mask, beta=pt.BETAS[t], row_index=row_index, eps_item=p.eps_item[t].to(d), eps_ability=p.eps_ab[t].to(d),
                       index=p.index[t].to(d))
        print(f'{what} step {t + 1}: loss {float(loss):.6f} rel_err {rel_err(loss, loss64):.2e}')
        assert rel_err(loss, loss64) < tg.TOL_LOSS, (what, t)
        now = tg.moments(view)
        prev = before if before is not None else {k: torch.zeros_like(v) for k, v in now.items()}
        got = types.SimpleNamespace(
            flat={b: (now[b + '_m'] - tg.B1 * prev[b + '_m']) / tg.W1 for b in ('par', 'item')},
            flat_from_v={b: ((now[b + '_v'] - tg.B2 * prev[b + '_v']) / tg.W2).clamp_min(0.0).sqrt() for b in ('par', 'item')})
        tg.assert_gradients(pt.by_name(method, got.flat, p.P, p.A, p.I, D), want, TOL_GRAD, f'{what} step {t + 1}')
        # persons outside the minibatch: the gradient is exactly 0 -- the moments are the old ones decayed, one fp32 product each
        outside = torch.ones(p.P, dtype=torch.bool)
        outside[p.index[t]] = False
        for j, k in enumerate(person_names):
            sl = slice(j * p.P * p.A, (j + 1) * p.P * p.A)
            m_old, v_old = prev['par_m'][sl].float().view(p.P, p.A)[outside], prev['par_v'][sl].float().view(p.P, p.A)[outside]
            m_new, v_new = now['par_m'][sl].float().view(p.P, p.A)[outside], now['par_v'][sl].float().view(p.P, p.A)[outside]
            assert torch.equal(m_new, torch.tensor(0.9) * m_old) and torch.equal(v_new, torch.tensor(0.999) * v_old), (what, t, k)
            assert want[k][outside].abs().max() == 0 if outside.any() else True
        if t == 0:
            tg.assert_second_moment_saw_the_same_gradient(got, what)
        tg.assert_adam(view, p_before, before, got, lr, t + 1, what)
        assert bool((tr.slot == -1).all()) and tr.bad_index_count == 0
    return tr, p


def _pin(i):
    """The last two shapes run on the matrix row-split kernel, the first on the VALU kernel; the others where the planner sends them."""
    return {0: (_lib.FLAG_KERNEL_VALU, VALU), 4: (_lib.FLAG_KERNEL_MATRIX, MATRIX), 5: (_lib.FLAG_KERNEL_MATRIX, MATRIX)}.get(i, (0, None))


@pytest.mark.parametrize('rows_mode', ['dense', 'gathered', 'codes'])
@pytest.mark.parametrize('i', range(len(pt.CASES)), ids=[pt.ident(c) for c in pt.CASES])
@pytest.mark.parametrize('method', ['vi', 'mle'])
def test_gradients_loss_and_adam_over_three_steps(method, i, rows_mode):
    flags, kernel = _pin(i)
    with ops.desc_flags(flags):
        tr, p = run_three_steps(method, pt.CASES[i], rows_mode, kernel=kernel)
    if p.B < p.P:                          # somebody visited at step 1 and not at step 2 moved at step 2 all the same
        gone = sorted(set(p.index[0].tolist()) - set(p.index[1].tolist()))
        assert gone and bool((tr.person_m[0][gone] != 0).all())


@pytest.mark.parametrize('method', ['vi', 'mle'])
def test_the_learning_rate_is_read_not_baked_in(method):
    run_three_steps(method, pt.CASES[2], lr=1e-3)


# ---------------------------------------------------------------------------
# 2. the table update alone
# ---------------------------------------------------------------------------
CAP_ENTRIES = _lib.PTRAIN_MAX_BLOCKS * 256 * 4          # one trip of the capped grid: 2048 workgroups x 256 threads x 4 entries
ITEMS = 7                                                # d->num_item of these calls (MLE: g = -dLL / (B num_item))


def table_adam(mode, A, rows, idx, grows, tables, m, v, beta, lr, t, alloc=None):
    """One vibo_person_table_adam call on device copies -> (tables, m, v, bad count).  tables: [T][alloc, A]; m, v: [T, alloc, A]
    (laid out with a stride that keeps every table's moments 16 bytes aligned); rows: table_rows of the call."""
    d = dev()
    T, alloc = len(tables), tables[0].shape[0]
    stride = (alloc * A + 3) // 4 * 4
    tabs = [x.to(d).contiguous() for x in tables]
    mom = [torch.zeros(T, stride, device=d) for _ in range(2)]
    for buf, src in zip(mom, (m, v)):
        buf[:, :alloc * A] = src.reshape(T, -1).to(d)
    slot = torch.full((alloc,), -1, dtype=torch.int32, device=d)
    bad = torch.zeros(1, dtype=torch.int32, device=d)
    B = idx.numel()
    dsc = ops._make_desc(ops.ElboSpec(irt_model=2, ability_dim=A, given=True), B, ITEMS, _lib.MASK_U8, _lib.REG_KL, True, 8, 8)
    steps = torch.tensor([t, 0], dtype=torch.int32, device=d)
    scal = torch.tensor([beta, lr], device=d)
    idx_d, g_d = idx.to(d), grows.to(d).contiguous()
    ops._call('vibo_person_table_adam', ctypes.byref(dsc), mode, rows, ops._ptr(idx_d), ops._ptr(g_d), ops._ptr(scal[0:1]),
              ops._ptr(scal[1:2]), ops._ptr(steps), ops._ptr(tabs[0]), ops._ptr(tabs[1]) if T > 1 else None, ops._ptr(mom[0]),
              ops._ptr(mom[1]), stride, ops._ptr(slot), ops._ptr(bad), ops._stream(d))
    torch.cuda.synchronize()
    assert bool((slot == -1).all()), 'the slot map is all -1 again after the call'
    assert steps.tolist() == [t, 0]
    return ([x.cpu() for x in tabs], mom[0][:, :alloc * A].reshape(T, alloc, A).cpu(), mom[1][:, :alloc * A].reshape(T, alloc, A).cpu(),
            int(bad))


def dense_gradient(mode, A, rows, alloc, idx, grows, beta):
    """float64 [T, alloc, A]: what embedding backward hands Adam (positions summed per person; positions outside [0, rows) dropped),
    and the same sum of the terms' magnitudes (the size of the fp32 sum's rounding)."""
    g0, g1 = grows[0].double(), grows[1].double()
    B = idx.numel()
    if mode == _lib.PTRAIN_VI:
        per, mag = -g0 + beta * g1, g0.abs() + abs(beta) * g1.abs()
        per, mag = per.view(B, 2, A).transpose(0, 1), mag.view(B, 2, A).transpose(0, 1)
    else:
        per, mag = (-g0[:, :A] / (B * ITEMS)).unsqueeze(0), (g0[:, :A].abs() / (B * ITEMS)).unsqueeze(0)
    ok = (idx >= 0) & (idx < rows)
    g, gm = torch.zeros(per.shape[0], alloc, A, dtype=torch.float64), torch.zeros(per.shape[0], alloc, A, dtype=torch.float64)
    g.index_add_(1, idx[ok], per[:, ok])
    gm.index_add_(1, idx[ok], mag[:, ok])
    return g, gm


def adam64(p, m, v, g, lr, t):
    """torch.optim.Adam in float64 on the CPU over the whole (dense) table, from the given moments at step t."""
    par = torch.nn.Parameter(p.double().clone())
    opt = torch.optim.Adam([par], lr=lr)
    opt.state[par] = {'step': torch.tensor(float(t - 1)), 'exp_avg': m.double().clone(), 'exp_avg_sq': v.double().clone()}
    par.grad = g.clone()
    opt.step()
    return par.detach(), opt.state[par]['exp_avg'], opt.state[par]['exp_avg_sq']


def check_update(mode, A, rows, idx, grows, tables, m, v, beta, lr, t, what):
    """Every entry of every table against float64 Adam: the parameter within adam_step_error's bound (1e-4 lr + 2^-23 |p|), the second
    moment within 4 x 2^-24 relative (+ one denormal step), the first within the same on its two terms' magnitudes -- each plus what
    the fp32 gradient itself carries (four roundings on the summed magnitudes of a person's positions: the constant, the product-sum, two additions)."""
    alloc = tables[0].shape[0]
    got_p, got_m, got_v, bad = table_adam(mode, A, rows, idx, grows, tables, m, v, beta, lr, t)
    g, gmag = dense_gradient(mode, A, rows, alloc, idx, grows, beta)
    eg = 4 * tg.U * gmag
    worst = 0.0
    for k in range(len(tables)):
        p64, m64, v64 = adam64(tables[k], m[k], v[k], g[k], lr, t)
        live = torch.arange(alloc) < rows
        err_p, bound_p = (got_p[k].double() - p64).abs(), 1e-4 * lr + 2.0 ** -23 * tables[k].double().abs()
        err_m = (got_m[k].double() - m64).abs()
        bound_m = 4 * tg.U * (0.9 * m[k].double().abs() + 0.1 * g[k].abs()) + 0.1 * eg[k] + tg.DENORM
        err_v = (got_v[k].double() - v64).abs()
        bound_v = 4 * tg.U * v64 + 0.001 * 2 * g[k].abs() * eg[k] + tg.DENORM
        for name, e, b in (('p', err_p, bound_p), ('m', err_m, bound_m), ('v', err_v, bound_v)):
            ratio = float((e[live] / b[live]).max())
            worst = max(worst, ratio)
            record('trainer_adam', float(e[live].max()), None, what=what, name=f'table {k} {name}', step=t, ratio=ratio)
            assert bool((e[live] <= b[live]).all()), (what, k, name, ratio, int((e[live] > b[live]).sum()))
        # rows the call was not given: bit-unchanged
        assert torch.equal(got_p[k][~live], tables[k][~live]) and torch.equal(got_m[k][~live], m[k][~live]) and torch.equal(got_v[k][~live], v[k][~live])
    print(f'{what}: worst error / bound {worst:.3f}')
    return got_p, got_m, got_v, bad


def table_inputs(mode, A, alloc, B, seed):
    """Parameters, NON-ZERO prior moments (a step of at most about 2 lr) and gradient rows."""
    g = torch.Generator().manual_seed(seed)
    T = 2 if mode == _lib.PTRAIN_VI else 1
    tables = [0.5 * torch.randn(alloc, A, generator=g) for _ in range(T)]
    m = 0.05 * torch.randn(T, alloc, A, generator=g)
    v = 0.01 * (torch.rand(T, alloc, A, generator=g) + 0.1)
    grows = torch.randn(2, B, 2 * A, generator=g)
    return g, tables, m, v, grows


SIZES = ([(1, n) for n in (1, 3, 4, 5, 63, 64, 65, 1023, 1025)] + [(3, n) for n in (1, 21, 341, 342)] +
         [(8, n) for n in (1, 8, 128, 129)])


@pytest.mark.parametrize('mode', [_lib.PTRAIN_VI, _lib.PTRAIN_MLE], ids=['vi', 'mle'])
@pytest.mark.parametrize('A,P', SIZES + [(3, CAP_ENTRIES // 2 + 7)], ids=lambda x: str(x))
def test_table_update_entry_by_entry(mode, A, P):
    """P A in {1, 3, 4, 5, 63, 64, 65, 1023, 1025} and around (every size where the 16-byte groups, their tail and the workgroups
    change shape), and one table of one and a half trips of the capped grid (VIBO_PTRAIN_MAX_BLOCKS = 2048 workgroups x 256 threads
    x 4 entries = 2 097 152 entries per trip: the grid-stride loop goes round twice).  B in {1, a few, P}; the minibatches name row 0 and row P - 1; t = 1 and 1000."""
    big = P * A > CAP_ENTRIES
    for n, (B, t) in enumerate([(1, 1), (min(P, 5), 1000)] + ([] if big else [(P, 1)])):
        g, tables, m, v, grows = table_inputs(mode, A, P, B, 1000 * A + P % 997 + n)
        if B == 1:
            idx = torch.tensor([P - 1])
        elif B == P:
            idx = torch.randperm(P, generator=g)
        else:
            idx = torch.cat([torch.tensor([P - 1]), torch.randperm(P - 2, generator=g)[:B - 2] + 1, torch.tensor([0])])
        assert len(set(idx.tolist())) == B
        *_, bad = check_update(mode, A, P, idx, grows, tables, m, v, 0.7, 5e-3, t, f'table update A={A} P={P} B={B} t={t}')
        assert bad == 0


@pytest.mark.parametrize('mode', [_lib.PTRAIN_VI, _lib.PTRAIN_MLE], ids=['vi', 'mle'])
@pytest.mark.parametrize('A', [1, 3, 8])
def test_duplicate_persons_sum_their_gradients_reproducibly(mode, A):
    """One person twice and one three times: the float64 update with the summed gradient, within the same bounds; two runs agree
    bit for bit."""
    P = 50
    idx = torch.tensor([7, 3, 7, 12, 3, 49, 3, 0])
    _, tables, m, v, grows = table_inputs(mode, A, P, idx.numel(), 77 + A)
    first = check_update(mode, A, P, idx, grows, tables, m, v, 0.7, 5e-3, 3, f'duplicates A={A}')
    again = table_adam(mode, A, P, idx, grows, tables, m, v, 0.7, 5e-3, 3)
    for a, b in zip(first[:3], again[:3]):
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    # the sum really has several terms: the update differs from the one that sees the first positions alone
    alone = table_adam(mode, A, P, torch.tensor([7, 3, 12, 49, 0]), grows[:, [0, 1, 3, 5, 7]].contiguous(), tables, m, v, 0.7, 5e-3, 3)
    if mode == _lib.PTRAIN_VI:          # (MLE: the other minibatch size scales every gradient)
        assert torch.equal(first[1][0][12], alone[1][0][12]) and not torch.equal(first[1][0][7], alone[1][0][7])
        assert not torch.equal(first[1][0][3], alone[1][0][3])


@pytest.mark.parametrize('mode', [_lib.PTRAIN_VI, _lib.PTRAIN_MLE], ids=['vi', 'mle'])
def test_an_index_outside_the_tables_is_counted_and_never_used(mode):
    """Tables ALLOCATED with 64 rows, the call made with table_rows = 40 and some indices in 40 .. 63 (no address outside the
    allocations even if the guard were broken): rows >= 40 and their moments bit-unchanged, the counter = the number of such
    positions, the other rows as the float64 update without them -- and, for VI, bit for bit what the call without those
    positions gives."""
    A, alloc, rows = 3, 64, 40
    idx = torch.tensor([5, 40, 39, 63, 0, 17, 52, 8])
    _, tables, m, v, grows = table_inputs(mode, A, alloc, idx.numel(), 9)
    got = check_update(mode, A, rows, idx, grows, tables, m, v, 0.7, 5e-3, 2, 'index guard')
    assert got[3] == 3
    if mode == _lib.PTRAIN_VI:
        keep = [0, 2, 4, 5, 7]
        without = table_adam(mode, A, rows, idx[keep], grows[:, keep].contiguous(), tables, m, v, 0.7, 5e-3, 2)
        assert without[3] == 0
        for a, b in zip(got[:3], without[:3]):
            for x, y in zip(a, b):
                assert torch.equal(x, y)


def test_the_trainer_counts_bad_indices_and_runs_them_on_the_zero_posterior():
    d = dev()
    p = pt.make_problem('vi', 2, 2, 30, 12, 6, 4)
    model = pt.build_model(p, d)
    tr = FusedTrainer(model, rng='native')
    r, m = ops.pad_rows(p.resp[:6].to(d), p.mask[:6].to(d))
    before = copy.deepcopy(model.state_dict())
    tr.step(r, m, index=torch.tensor([3, 30, 7, -1, 29, 1 << 40], device=d))
    assert tr.bad_index_count == 3 and bool((tr.slot == -1).all())
    post = tr._post[6].cpu()
    assert bool((post[[1, 3, 5]] == 0).all())
    assert torch.equal(post[0], torch.cat([before['ability_mu_lookup.weight'][3], before['ability_logvar_lookup.weight'][3]]).cpu())
    moved = (model.ability_mu_lookup.weight != before['ability_mu_lookup.weight']).any(1).cpu()
    assert moved.nonzero().flatten().tolist() == [3, 7, 29]      # (first step: nobody else has momentum yet)


# ---------------------------------------------------------------------------
# 3. beside the module path
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('i', [0, 1, 2])
@pytest.mark.parametrize('method', ['vi', 'mle'])
def test_follows_module_and_torch_adam(method, i):
    """test_gpu_trainer.assert_follows_torch_adam's scheme: twin models, four steps of module + autograd + torch.optim.Adam on one
    and of the native trainer (rng='torch') on the other, each pair under the same torch.manual_seed(100 + step); every loss
    within 2e-5 relative, every state_dict tensor within 2e-5 at the end; after step 0 every entry whose gradient is above 1e-3 of
    its tensor's largest has moved the same way (a wrong sign shows as 2 lr)."""
    d = dev()
    p = pt.make_problem(method, *pt.CASES[i])
    ref = pt.build_model(p, d)
    fus = copy.deepcopy(ref)
    opt = torch.optim.Adam(ref.parameters(), lr=5e-3)
    trainer = FusedTrainer(fus, lr=5e-3)
    assert type(trainer) is CLASS[method] and list(fus.state_dict()) == list(ref.state_dict())
    resp, mask = ops.pad_rows(p.resp.to(d), p.mask.to(d))
    beta = 0.7
    for step in range(4):
        rows = p.index[step % 3].to(d)
        torch.manual_seed(100 + step)
        opt.zero_grad()
        if method == 'vi':
            loss_ref = ref.elbo(*ref(rows, resp, mask, row_index=rows), annealing_factor=beta)
        else:
            loss_ref = ref.nll_step(rows, resp, mask, row_index=rows)
        loss_ref.backward()
        if step == 0:
            g_ref = {k: q.grad.clone() for k, q in ref.named_parameters()}
        opt.step()
        torch.manual_seed(100 + step)
        loss_fus = trainer.step(resp, mask, beta=beta, row_index=rows)
        assert abs(float(loss_fus) - float(loss_ref.detach())) < 2e-5 * abs(float(loss_ref.detach())), step
        if step == 0:
            for (k, a), (_, b) in zip(ref.named_parameters(), fus.named_parameters()):
                big = g_ref[k].abs() > 1e-3 * g_ref[k].abs().max()
                diff = (a.detach() - b.detach()).abs()
                assert (diff[big] < 1e-4).all(), (k, float(diff.max()), int((diff[big] >= 1e-4).sum()), int(big.sum()))
    for (k, a), (_, b) in zip(ref.state_dict().items(), fus.state_dict().items()):
        assert (a - b).abs().max() < 2e-5, (k, float((a - b).abs().max()))
    assert int(trainer.step_count) == 4


# ---------------------------------------------------------------------------
# 4. noise
# ---------------------------------------------------------------------------
def twins(method, case, **kw):
    d = dev()
    p = pt.make_problem(method, *case)
    m_a = pt.build_model(p, d)
    m_b = copy.deepcopy(m_a)
    return p, m_a, m_b, FusedTrainer(m_a, lr=5e-3, **kw), FusedTrainer(m_b, lr=5e-3, **kw)


def assert_same_state(t_a, t_b):
    assert_same_parameters(t_a.model, t_b.model)
    for name in ('person_m', 'person_v', 'item_m', 'item_v', '_steps', 'slot'):
        a, b = getattr(t_a, name), getattr(t_b, name)
        assert torch.equal(a, b) and bool(torch.isfinite(a.float()).all()), name


def test_noise_drawn_in_the_prologue_equals_separate_fills():
    """Three native-rng steps = three given-noise steps fed with vibo_fill_normal at the step's counter (completed steps), stream 0
    for the items and stream 1 for the abilities: bit for bit in all parameters and moments."""
    seed = 1234
    p, _, _, t_a, t_b = twins('vi', pt.CASES[1], rng='native', seed=seed)
    d = dev()
    resp, mask = ops.pad_rows(p.resp.to(d), p.mask.to(d))
    D = O.item_feat_dim(p.irt, p.A)
    for step in range(3):
        rows = p.index[step].to(d)
        l_a = t_a.step(resp, mask, beta=0.7, row_index=rows)
        counter = noise_counter(step)
        eps_item = fill_normal(p.I * D, seed, counter, 0).view(p.I, D)
        eps_ab = fill_normal(p.B * p.A, seed, counter, 1).view(p.B, p.A)
        l_b = t_b.step(resp, mask, beta=0.7, row_index=rows, eps_item=eps_item, eps_ability=eps_ab)
        assert torch.equal(l_a, l_b), step
        assert torch.equal(t_a._eps_item, eps_item) and torch.equal(t_a._eps_ab[p.B], eps_ab)
    assert_same_state(t_a, t_b)


def test_a_forward_backward_without_update_leaves_no_claims_behind():
    """forward_backward() on one minibatch, then -- no update() -- a whole step on another: the first minibatch's claims must not
    hand its persons the second's gradient rows.  The moments (zero before: they hold the gradient alone, whatever Adam's t) equal
    the twin's that ran the second step only."""
    p, _, _, t_a, t_b = twins('vi', pt.CASES[0])
    d = dev()
    resp, mask = ops.pad_rows(p.resp.to(d), p.mask.to(d))
    noise = dict(eps_item=p.eps_item[0].to(d), eps_ability=p.eps_ab[0].to(d))
    t_a.forward_backward(resp, mask, beta=0.7, row_index=p.index[0].to(d), **noise)
    t_a.step(resp, mask, beta=0.7, row_index=p.index[2].to(d), **noise)
    t_b.step(resp, mask, beta=0.7, row_index=p.index[2].to(d), **noise)
    assert int(t_a.step_count) == 2 and int(t_b.step_count) == 1
    for name in ('person_m', 'person_v', 'item_m', 'item_v', 'slot'):
        assert torch.equal(getattr(t_a, name), getattr(t_b, name)), name
    assert bool((t_a.slot == -1).all())


# ---------------------------------------------------------------------------
# 5. hipGraph
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('method', ['vi', 'mle'])
def test_replayed_step_equals_the_eager_step(method):
    """Twin trainers, rng='native': one captures its step once and replays it with the row-index buffer refreshed, the other
    launches the same steps eagerly; every 7th step the epoch's shorter last minibatch runs eagerly on both.  The same finite bits
    at the end (test_gpu_trainer.assert_replays_bitwise's scheme)."""
    d = dev()
    case = (2, 8, 4099, 200, 130, 1)
    p, m1, m2, t1, t2 = twins(method, case, rng='native', seed=5)
    resp, mask = ops.pad_rows(p.resp.to(d), p.mask.to(d))
    B, P = p.B, p.P
    perm = torch.randperm(P, generator=torch.Generator().manual_seed(3)).to(d)
    rows = torch.zeros(B, dtype=torch.int64, device=d)
    short = perm[-(P % B):]
    assert 0 < short.numel() < B

    def window(it):
        lo = (it * B) % (P - B)
        rows.copy_(perm[lo:lo + B])

    for it in range(3):                   # warm-up, eagerly
        window(it)
        t1.step(resp, mask, row_index=rows)
        t2.step(resp, mask, row_index=rows)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        lg = t1.step(resp, mask, row_index=rows)           # capture only: nothing runs
    for it in range(3, 24):
        if it % 7 == 0:
            t1.step(resp, mask, row_index=short)
            t2.step(resp, mask, row_index=short)
        window(it)
        gr.replay()
        l2 = t2.step(resp, mask, row_index=rows)
        if it % 10 == 0 or it == 23:
            assert torch.equal(lg, l2), it
    torch.cuda.synchronize()
    assert int(t1.step_count) == 3 + 21 + 3 and t1.generation == 0
    assert_same_state(t1, t2)


# ---------------------------------------------------------------------------
# 6. the CLIs
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('method', ['vi', 'mle'])
def test_cli_native_step(method, tmp_path, monkeypatch):
    """200 x 50, 2 epochs (vi.py: replayed from a hipGraph, native noise; mle.py: --no-graph): the same checkpoint keys as without the
    flag, finite and decreasing losses."""
    from vibo_amd.torch_core import mle, vi
    monkeypatch.setattr(config, 'DATA_DIR', str(tmp_path / 'data'))
    cli = vi if method == 'vi' else mle
    argv = ['--irt-model', '2pl', '--dataset', '2pl_simulation', '--num-person', '200', '--num-item', '50', '--epochs', '2',
            '--batch-size', '16', '--cuda']
    argv += ['--num-posterior-samples', '2'] if method == 'vi' else []
    keys = {}
    native = ['--native-step', '--rng', 'native'] if method == 'vi' else ['--native-step', '--no-graph']
    for name, extra in (('module', []), ('native', native)):
        out = cli.main(argv + ['--out-dir', str(tmp_path / name)] + extra)
        ckpt = torch.load(os.path.join(out, 'checkpoint.pth.tar'), weights_only=False)
        keys[name] = (sorted(ckpt), list(ckpt['model_state_dict']))
        losses = np.load(os.path.join(out, 'train_losses.npy'))
        print(method, name, losses)
        assert np.isfinite(losses).all() and (name == 'module' or losses[1] < losses[0]), (name, losses)
        assert all(bool(torch.isfinite(v).all()) for v in ckpt['model_state_dict'].values())
    assert keys['native'] == keys['module']
