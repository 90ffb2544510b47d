"""FusedDecoderTrainer (vibo_dtrain_* / vibo_dtrain_*_cond around vibo_decoder_fwd_bwd): the native train step of --generative-model
link | deep | residual, with the unconditional and (conditional=True) the conditional posterior, against the reference's recorded
Adam steps, the fp64 oracle, the module + torch.optim.Adam step, its own hipGraph replay and itself.  Tests of both posteriors take
`conditional` first; the unconditional cases keep the ids they always had, the conditional ones carry 'cond-' in front."""
import copy
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR, Golden, rel_err
from decoder_trainer_common import (COND_ORACLE_CASES, ORACLE_CASES, TOL_ADAM1, TOL_ADAM3, assert_same_state, compare_kept, keep_entries, make_problem,
                                    oracle_of, print_excluded_shares, resident, state_of)
from golden_common import build_model
from gpu_common import CLS, TOL_ELBO, dev, scattered_rows, simulated
from oracle import vibo_oracle as O
from vibo_amd import decoder, ops
from vibo_amd.torch_core.models import VIBO_2PL
from vibo_amd.trainer import FusedDecoderTrainer, FusedTrainer

pytestmark = pytest.mark.gpu


def both(uncond, cond):
    """(conditional, *case) for the cases of the two posteriors."""
    ident = lambda case: '-'.join(str(x) for x in case)
    return ([pytest.param(False, *case, id=ident(case)) for case in uncond] +
            [pytest.param(True, *case, id='cond-' + ident(case)) for case in cond])


# ---------------------------------------------------------------------------
# 1. the reference's recorded Adam steps
# ---------------------------------------------------------------------------
def golden_rows(golden, rows, d):
    """The golden's minibatch as `rows` says -> response, mask, row_index: direct, gathered out of a larger resident matrix, or as
    cell codes."""
    if rows == 'gathered':
        big_r, big_m, where = scattered_rows(golden.response, golden.mask, 3 * golden.response.shape[0] + 5)
        return (*ops.pad_rows(big_r.to(d), big_m.to(d)), where.to(d))
    if rows == 'cell-codes':
        return ops.pack_cell_codes(golden.response.to(d), golden.mask.to(d).bool()), None, None
    return (*ops.pad_rows(golden.response.to(d), golden.mask.to(d).bool()), None)


@pytest.mark.parametrize('rows', ['direct', 'gathered', 'cell-codes'])
@pytest.mark.parametrize('case', ['case_2pl_a1_link_miss', 'case_2pl_a2_deep_miss', 'case_3pl_a1_residual'])
def test_reference_goldens_through_the_native_step(case, rows):
    """Parameters after 1 and 3 steps of vibo.py:243-268 as the reference itself recorded them (tools/gen_golden.py), the case's
    noise replayed: no autograd and no torch.optim between the goldens and the kernels."""
    golden = Golden(os.path.join(GOLDEN_DIR, case + '.npz'))
    m = golden.meta
    assert m['use_kl_divergence'] and m['n_norm_flows'] == 0 and not m['conditional_posterior']
    d = dev()
    model = build_model(golden).to(d)
    tr = FusedTrainer(model, lr=5e-3)
    assert isinstance(tr, FusedDecoderTrainer)
    resp, mask, row_index = golden_rows(golden, rows, d)
    eps_i, eps_a = golden.eps_item.to(d), golden.eps_ability.to(d)
    for step in range(3):
        loss = tr.step(resp, mask, beta=m['annealing_factor'], row_index=row_index, eps_item=eps_i, eps_ability=eps_a)
        if step == 0:
            print('loss rel_err', rel_err(loss, golden.out['loss']))
            assert rel_err(loss, golden.out['loss']) < TOL_ELBO
            for k, v in golden.adam1.items():
                err = float((model.state_dict()[k].cpu() - v).abs().max())
                print('adam1', k, err)
                assert err < TOL_ADAM1, (k, 'after one step')
    for k, v in golden.adam3.items():
        err = float((model.state_dict()[k].cpu() - v).abs().max())
        print('adam3', k, err)
        assert err < TOL_ADAM3, k


@pytest.mark.parametrize('rows', ['direct', 'gathered', 'cell-codes'])
def test_reference_golden_through_the_native_step(rows):
    """Loss and the parameters after 1 and 3 steps of vibo.py:243-268 as the reference itself recorded them (tools/gen_golden.py),
    the case's noise replayed: no autograd and no torch.optim between the golden and the kernels."""
    golden = Golden(os.path.join(GOLDEN_DIR, 'case_2pl_a2_cond_residual_miss.npz'))
    m = golden.meta
    assert m['use_kl_divergence'] and m['n_norm_flows'] == 0 and m['conditional_posterior']
    d = dev()
    model = build_model(golden).to(d)
    tr = FusedTrainer(model, lr=5e-3, conditional=True)
    assert isinstance(tr, FusedDecoderTrainer) and tr.cond
    resp, mask, row_index = golden_rows(golden, rows, d)
    eps_i, eps_a = golden.eps_item.to(d), golden.eps_ability.to(d)
    for step in range(3):
        loss = tr.step(resp, mask, beta=m['annealing_factor'], row_index=row_index, eps_item=eps_i, eps_ability=eps_a)
        if step == 0:
            print('loss rel_err', rel_err(loss, golden.out['loss']))
            assert rel_err(loss, golden.out['loss']) < TOL_ELBO
            for k, v in golden.out.items():
                if k in ('ability_mu', 'ability_logvar', 'ability'):
                    err = float((getattr(tr.last, k).cpu() - v.reshape(getattr(tr.last, k).shape)).abs().max())
                    print(k, err)
                    assert err < TOL_ELBO * max(1.0, float(v.abs().max())), k
            for k, v in golden.adam1.items():
                err = float((model.state_dict()[k].cpu() - v).abs().max())
                print('adam1', k, err)
                assert err < TOL_ADAM1, (k, 'after one step')
    for k, v in golden.adam3.items():
        err = float((model.state_dict()[k].cpu() - v).abs().max())
        print('adam3', k, err)
        assert err < TOL_ADAM3, k


def test_the_default_trainer_still_refuses_the_conditional_posterior():
    bad = VIBO_2PL(2, 20, generative_model='deep', ability_merge='product', conditional_posterior=True).to(dev())
    with pytest.raises(NotImplementedError, match='conditional=True'):
        FusedTrainer(bad)


# ---------------------------------------------------------------------------
# 2. random shapes against the fp64 oracle (decoder_trainer_common.ORACLE_CASES / COND_ORACLE_CASES)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('conditional,gen,irt,A,B,I,missing,H,drop,seed', both(ORACLE_CASES, COND_ORACLE_CASES))
def test_random_shapes_against_the_fp64_oracle(conditional, gen, irt, A, B, I, missing, H, drop, seed):
    case = (gen, irt, A, B, I, missing, H, drop, seed)
    model, resp, mask, eps_item, eps_ab = make_problem(conditional, *case)
    after, loss0, keep = oracle_of(conditional, case)
    d = dev()
    model = model.to(d)
    tr = FusedTrainer(model, lr=5e-3, conditional=conditional)
    r, m = ops.pad_rows(resp.to(d), mask.bool().to(d))
    for step in range(3):
        loss = tr.step(r, m, beta=1.0, eps_item=eps_item[step].to(d), eps_ability=eps_ab[step].to(d))
        if step == 0:
            print('loss rel_err', rel_err(loss, loss0))
            assert rel_err(loss, loss0) < TOL_ELBO
            compare_kept(model.state_dict(), after[1], keep, TOL_ADAM1, 'adam1')
    compare_kept(model.state_dict(), after[3], keep, TOL_ADAM3, 'adam3')


# ---------------------------------------------------------------------------
# 3. the module + torch.optim.Adam step
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('conditional,gen,irt,A,B,I,missing,H,drop,seed', both(ORACLE_CASES, COND_ORACLE_CASES))
def test_native_step_equals_the_module_step(conditional, gen, irt, A, B, I, missing, H, drop, seed):
    """Both fp32: the bounds and the exclusion rule of the oracle test on the same problems, the threshold taken on the module
    path's own gradients."""
    model, resp, mask, eps_item, eps_ab = make_problem(conditional, gen, irt, A, B, I, missing, H, drop, seed)
    d = dev()
    ref = model.to(d)
    fus = copy.deepcopy(ref)
    opt = torch.optim.Adam(ref.parameters(), lr=5e-3)
    tr = FusedTrainer(fus, lr=5e-3, conditional=conditional)
    r, m = ops.pad_rows(resp.to(d), mask.bool().to(d))
    names = [k for k, _ in ref.named_parameters()]
    assert names == list(ref.state_dict().keys())
    keep = {k: torch.ones_like(v, dtype=torch.bool) for k, v in ref.state_dict().items()}
    for step in range(3):
        opt.zero_grad()
        outs = ref(r, m, eps_item=eps_item[step].to(d), eps_ability=eps_ab[step].to(d))
        loss_ref = ref.elbo(*outs, annealing_factor=1.0)
        loss_ref.backward()
        keep_entries(keep, {k: p.grad for k, p in ref.named_parameters()})
        opt.step()
        loss = tr.step(r, m, beta=1.0, eps_item=eps_item[step].to(d), eps_ability=eps_ab[step].to(d))
        print('step', step, 'loss rel_err', rel_err(loss, loss_ref.detach()))
        assert rel_err(loss, loss_ref.detach()) < TOL_ELBO
        if step == 0:
            compare_kept(fus.state_dict(), {k: v.detach() for k, v in ref.state_dict().items()}, {k: v.cpu() for k, v in keep.items()},
                         TOL_ADAM1, 'adam1')
    compare_kept(fus.state_dict(), {k: v.detach() for k, v in ref.state_dict().items()}, {k: v.cpu() for k, v in keep.items()}, TOL_ADAM3,
                 'adam3')
    assert int(tr.step_count) == 3


# ---------------------------------------------------------------------------
# 4. - 7. replay, reproducibility, chunks, external writes, missing-data modes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('conditional,gen,irt,A,I,B,codes',
                         both([('deep', 2, 2, 100, 16, False), ('link', 3, 1, 95, 16, True), ('residual', 3, 3, 130, 48, False)],
                              [('deep', 2, 2, 100, 16, False), ('link', 3, 1, 95, 16, True)]))
def test_replay_is_the_eager_step_bit_for_bit(conditional, gen, irt, A, I, B, codes):
    """A captured step() replayed 60 times -- native Philox noise, row_index refreshed through a device buffer, beta changed between
    replays, a shorter eager minibatch in between -- against eager steps of a twin: every loss, state_dict tensor and Adam moment
    torch.equal, fresh noise on every replay (the step counters live on the device)."""
    P = 5 * B + 3
    m1, resp, mask, g = resident(conditional, gen, irt, A, P, I, codes=codes)
    m2 = copy.deepcopy(m1)
    t1 = FusedTrainer(m1, lr=5e-3, rng='native', seed=11, conditional=conditional)
    t2 = FusedTrainer(m2, lr=5e-3, rng='native', seed=11, conditional=conditional)
    d = dev()
    rows = torch.randperm(P, generator=g)[:B].to(d)
    for k in range(3):                                   # warm-up (allocations, the resident row counts) before the capture
        assert torch.equal(t1.step(resp, mask, row_index=rows), t2.step(resp, mask, row_index=rows)), k
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        lg = t1.step(resp, mask, row_index=rows)         # capture only: nothing runs
    seen = []
    for k in range(60):
        beta = 1.0 if k < 30 else 0.6
        if k == 20:                                      # the epoch's last, shorter minibatch runs eagerly
            short = torch.arange(P - 5, P, device=d)
            assert torch.equal(t1.step(resp, mask, beta=beta, row_index=short), t2.step(resp, mask, beta=beta, row_index=short))
            continue
        new_rows = torch.randperm(P, generator=g)[:B].to(d)
        rows.copy_(new_rows)
        t1.set_beta(beta)
        graph.replay()
        l2 = t2.step(resp, mask, beta=beta, row_index=new_rows)
        assert torch.equal(lg, l2), (k, float(lg), float(l2))
        assert bool(torch.isfinite(lg))
        seen.append(t1._eps_ab[B].clone())
    assert not any(torch.equal(seen[0], s) for s in seen[1:])
    assert t1._steps.tolist() == t2._steps.tolist() == [63, 63]
    assert_same_state(state_of(m1, t1), state_of(m2, t2))


@pytest.mark.parametrize('conditional,gen,irt,A,I,B', both([('deep', 2, 8, 130, 300), ('link', 2, 1, 95, 33), ('residual', 3, 2, 200, 77)],
                                                           [('residual', 3, 2, 200, 77)]))
def test_two_fresh_trainers_are_bitwise_equal(conditional, gen, irt, A, I, B):
    res = []
    for _ in range(2):
        model, resp, mask, g = resident(conditional, gen, irt, A, B, I)
        tr = FusedTrainer(model, lr=5e-3, rng='native', seed=3, conditional=conditional)
        losses = [tr.step(resp, mask, beta=0.8).clone() for _ in range(5)]
        res.append((losses, state_of(model, tr)))
    (l0, s0), (l1, s1) = res
    assert all(torch.equal(a, b) and bool(torch.isfinite(a)) for a, b in zip(l0, l1))
    assert_same_state(s0, s1)


@pytest.mark.parametrize('gen,irt', [('residual', 3), ('deep', 2), ('link', 2)])
def test_person_chunks_change_nothing_but_the_summation_order(monkeypatch, gen, irt):
    """Minibatches above decoder.PERSON_CHUNK persons run the person kernels and the decoder once per chunk.  Compared after ONE
    step on Adam's first moments (= 0.1 x the gradient: Adam's normalised parameter step would hide the magnitudes), with
    test_person_chunking_changes_nothing_but_the_summation_order's tolerances, tensor by tensor; the chunked step is reproducible.
    301 persons at PERSON_CHUNK 64 are four chunks of 61 and a last one of 57: the uneven tail (workgroups without a tile, d V and
    the decoder's launch sized by the chunk's own count) runs too."""
    B, I, A = 301, 130, 3
    d = dev()
    res = []
    for chunk in (1 << 20, 64, 64):
        monkeypatch.setattr(decoder, 'PERSON_CHUNK', chunk)
        model, resp, mask, g = resident(False, gen, irt, A, B, I)
        eg = torch.Generator().manual_seed(5)
        eps_i, eps_a = torch.randn(I, O.item_feat_dim(irt, A), generator=eg).to(d), torch.randn(B, A, generator=eg).to(d)
        tr = FusedTrainer(model, lr=5e-3)
        loss = tr.step(resp, mask, beta=0.9, eps_item=eps_i, eps_ability=eps_a).clone()
        base, n_item = tr.par_flat.data_ptr(), tr.item_mu.numel()
        where = {k: ((v.data_ptr() - base) // 4, v.numel()) for k, v in model.named_parameters()
                 if base <= v.data_ptr() < base + 4 * tr.par_flat.numel()}          # the parameters are views of par_flat
        assert sum(n for _, n in where.values()) == tr.par_flat.numel()
        res.append((loss, tr.par_m.clone(), tr.item_m.clone(), tr.last.ability.clone()))
    (l0, p0, i0, a0), (l1, p1, i1, a1), (l2, p2, i2, a2) = res
    assert abs(float(l0) - float(l1)) < 1e-6 * abs(float(l0))
    moments = [(k, p0[o:o + n], p1[o:o + n]) for k, (o, n) in where.items()]
    moments += [('item mu', i0[:n_item], i1[:n_item]), ('item logvar', i0[n_item:], i1[n_item:])]
    worst = []
    for k, x, y in moments:
        err, top = float((x - y).abs().max()), float(x.abs().max())
        print(k, 'max-abs', top, 'difference', err, 'relative', err / top)
        if not err <= 2e-6 * top:
            worst.append((k, err, top))
    assert not worst, worst
    assert torch.equal(a0, a1)                                                     # per-person outputs: bitwise
    assert torch.equal(l1, l2) and torch.equal(p1, p2) and torch.equal(i1, i2)     # the chunked step is reproducible


def test_person_chunks_of_the_conditional_step_change_nothing_but_the_summation_order(monkeypatch):
    """77 persons at PERSON_CHUNK 26 run the person kernels and the decoder in three chunks of 26, 26 and 25 around ONE pair of
    code-table calls: the per-person outputs are those of the one-chunk run bit for bit, the loss to 1e-6, the parameters after
    the step to TOL_ADAM1."""
    gen, irt, A, I, B = 'residual', 3, 2, 200, 77
    d = dev()
    res = []
    for chunk in (1 << 20, 26):
        monkeypatch.setattr(decoder, 'PERSON_CHUNK', chunk)
        model, resp, mask, g = resident(True, gen, irt, A, B, I)
        eg = torch.Generator().manual_seed(5)
        eps_i, eps_a = torch.randn(I, O.item_feat_dim(irt, A), generator=eg).to(d), torch.randn(B, A, generator=eg).to(d)
        tr = FusedTrainer(model, lr=5e-3, conditional=True)
        loss = tr.step(resp, mask, beta=0.9, eps_item=eps_i, eps_ability=eps_a).clone()
        assert list(tr._scratch) == [(B, min(chunk, B))]
        res.append((loss, tr.last.ability_mu.clone(), tr.last.ability_logvar.clone(), tr.last.ability.clone(),
                    {k: v.clone() for k, v in model.state_dict().items()}))
    (l0, mu0, lv0, a0, s0), (l1, mu1, lv1, a1, s1) = res
    assert bool(torch.isfinite(l0)) and abs(float(l0) - float(l1)) < 1e-6 * abs(float(l0))
    assert torch.equal(mu0, mu1) and torch.equal(lv0, lv1) and torch.equal(a0, a1)
    for k in s0:
        err = float((s0[k] - s1[k]).abs().max())
        print(k, err)
        assert err < TOL_ADAM1, k


def test_external_parameter_writes_and_refusals():
    B, I, A = 40, 64, 2
    d = dev()
    model, resp, mask, g = resident(False, 'deep', 2, A, B, I)
    sd0 = copy.deepcopy(model.state_dict())
    eps_i, eps_a = torch.randn(I, A + 1, generator=g).to(d), torch.randn(B, A, generator=g).to(d)
    tr = FusedTrainer(model, lr=5e-3)
    first = tr.step(resp, mask, eps_item=eps_i, eps_ability=eps_a).clone()
    second = tr.step(resp, mask, eps_item=eps_i, eps_ability=eps_a).clone()
    assert not torch.equal(first, second)                        # the parameters moved
    model.load_state_dict(sd0)                                   # an external write between two steps ...
    again = tr.step(resp, mask, eps_item=eps_i, eps_ability=eps_a).clone()
    assert torch.equal(first, again)                             # ... is what the next step computes its loss from
    with torch.no_grad():
        for k, v in model.state_dict().items():
            v.data.copy_(sd0[k])
    tr.invalidate()
    assert torch.equal(first, tr.step(resp, mask, eps_item=eps_i, eps_ability=eps_a))
    with pytest.raises(RuntimeError):
        tr.update()                                              # nothing pending
    with pytest.raises(NotImplementedError, match='torch.optim'):
        tr.step(resp, mask.long(), eps_item=eps_i, eps_ability=eps_a)
    for kw, word in (({'conditional_posterior': True}, 'conditional'), ({'n_norm_flows': 2}, 'flows'), ({'ability_merge': 'mean'}, 'mean')):
        bad = VIBO_2PL(A, I, generative_model='deep', **{'ability_merge': 'product', **kw}).to(d)
        with pytest.raises(NotImplementedError, match='torch.optim') as e:
            FusedTrainer(bad)
        assert word in str(e.value)
    sharded = VIBO_2PL(A, I, ability_merge='product', generative_model='link').to(d)
    sharded._reducer = lambda flat: flat
    with pytest.raises(NotImplementedError, match='torch.optim'):
        FusedTrainer(sharded)


def test_gathered_row_buffers_are_never_replaced():
    """A captured graph keeps the addresses it recorded: minibatches of one size gathered with a mask, then without one, then with
    one again go through buffers of their own, and every buffer the trainer ever used stays where it was."""
    B, I, A = 24, 64, 2
    d = dev()
    model, resp, mask, g = resident(False, 'deep', 2, A, 80, I, missing=0.0)
    rows = torch.randperm(80, generator=g)[:B].to(d)
    eps_i, eps_a = torch.randn(I, A + 1, generator=g).to(d), torch.randn(B, A, generator=g).to(d)
    tr = FusedTrainer(model, lr=5e-3)
    seen, gen0 = {}, tr.generation
    for m in (mask, None, mask, None):
        tr.step(resp, m, row_index=rows, eps_item=eps_i, eps_ability=eps_a)
        for bufs in list(tr._rows.values()) + [(s,) for s in tr._scratch.values()]:
            for t in bufs:
                if t is not None:
                    assert seen.setdefault(id(t), t.data_ptr()) == t.data_ptr()
        kept = {id(t) for bufs in list(tr._rows.values()) + [(s,) for s in tr._scratch.values()] for t in bufs if t is not None}
        assert set(seen) <= kept                                  # nothing a graph may point at was dropped
    assert tr.generation == gen0 and len(tr._rows) == 2


@pytest.mark.parametrize('codes', [False, True])
def test_missing_data_modes_and_the_all_missing_row(codes):
    """Prior expert: a person without an observed cell gets exactly the prior-only posterior, mu = 0 and logvar = log(1 / (I / (1 +
    1e-8))), whatever the table holds, and nothing of the step is NaN.  --drop-missing on the same rows without that person: the
    posterior is the observed experts' alone (against models._conditional_posterior_poe)."""
    gen, irt, A, I, B = 'deep', 2, 3, 45, 21
    d = dev()
    resp, mask, g = simulated(irt, B, I, A, 0.3, seed=9)
    mask = mask.bool()
    mask[5] = False
    eps_i, eps_a = torch.randn(I, A + 1, generator=g).to(d), torch.randn(B, A, generator=g).to(d)
    for drop in (False, True):
        rows = torch.arange(B) if not drop else torch.tensor([b for b in range(B) if b != 5])
        r, m = ops.pad_rows(resp[rows].to(d), mask[rows].to(d))
        torch.manual_seed(3)
        model = CLS[irt](A, I, ability_merge='product', generative_model=gen, conditional_posterior=True,
                         replace_missing_with_prior=not drop).to(d)
        ref = copy.deepcopy(model)
        tr = FusedTrainer(model, lr=5e-3, conditional=True)
        if codes:
            loss = tr.step(ops.pack_cell_codes(r, m), None, eps_item=eps_i, eps_ability=eps_a[rows.to(d)])
        else:
            loss = tr.step(r, m, eps_item=eps_i, eps_ability=eps_a[rows.to(d)])
        mu, lv = tr.last.ability_mu, tr.last.ability_logvar
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(mu).all()) and bool(torch.isfinite(lv).all())
        for k, v in model.state_dict().items():
            assert bool(torch.isfinite(v).all()), k
        if not drop:
            assert torch.equal(mu[5], torch.zeros(A, device=d))
            want = torch.log(torch.tensor(1.0) / (torch.tensor(float(I)) * (torch.tensor(1.0) / (torch.tensor(1.0) + 1e-8))))
            assert float((lv[5].cpu() - want).abs().max()) < 1e-6
        with torch.no_grad():
            item_feat = ref.item_encoder.mu_lookup.weight + torch.exp(0.5 * ref.item_encoder.logvar_lookup.weight) * eps_i
            rmu, rlv = ref._conditional_posterior_poe(r, m, None, item_feat)
        print('drop', drop, 'mu', float((mu - rmu).abs().max()), 'logvar', float((lv - rlv).abs().max()))
        assert float((mu - rmu).abs().max()) < TOL_ELBO and float((lv - rlv).abs().max()) < TOL_ELBO


# ---------------------------------------------------------------------------
# 8. the CLI
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('extra', [['--generative-model', 'deep', '--ability-dim', '2'],
                                   ['--generative-model', 'link', '--artificial-missing-perc', '0.2'],
                                   ['--generative-model', 'residual', '--irt-model', '3pl', '--dataset', '3pl_simulation'],
                                   ['--generative-model', 'deep', '--no-graph', '--rng', 'native']])
def test_cli_end_to_end_with_the_native_decoder_step(tmp_path, monkeypatch, extra):
    from vibo_amd import config, trainer
    from vibo_amd.torch_core import vibo as cli
    monkeypatch.setattr(config, 'DATA_DIR', str(tmp_path / 'data'))
    monkeypatch.setattr(config, 'OUT_DIR', str(tmp_path / 'out'))
    steps = []
    real = trainer.FusedDecoderTrainer.step
    monkeypatch.setattr(trainer.FusedDecoderTrainer, 'step', lambda self, *a, **k: (steps.append(1), real(self, *a, **k))[1])
    argv = ['--irt-model', '2pl', '--dataset', '2pl_simulation', '--num-person', '600', '--num-item', '12',
            '--epochs', '4', '--batch-size', '16', '--num-posterior-samples', '3', '--cuda', '--native-decoder-step',
            '--out-dir', str(tmp_path / 'out')] + extra
    cli.main(argv)
    assert steps                                                  # the native trainer ran (eagerly, or once per capture)
    (run_dir,) = os.listdir(tmp_path / 'out')
    ck = torch.load(tmp_path / 'out' / run_dir / 'checkpoint.pth.tar', weights_only=False)
    assert {'model_state_dict', 'epoch', 'args', 'train_logp', 'test_logp'} <= set(ck)
    losses = np.load(tmp_path / 'out' / run_dir / 'train_losses.npy')
    print('epoch losses', losses)
    assert losses.shape == (4,) and np.isfinite(losses).all() and losses[-1] < losses[0]
    a = ck['args']
    fresh = CLS[int(a.irt_model[0])](a.ability_dim, 12, hidden_dim=a.hidden_dim, ability_merge=a.ability_merge,
                                     generative_model=a.generative_model)
    fresh.load_state_dict(ck['model_state_dict'], strict=True)


def test_cli_end_to_end_with_the_native_conditional_step(tmp_path, monkeypatch):
    from vibo_amd import config, trainer
    from vibo_amd.torch_core import vibo as cli
    monkeypatch.setattr(config, 'DATA_DIR', str(tmp_path / 'data'))
    monkeypatch.setattr(config, 'OUT_DIR', str(tmp_path / 'out'))
    steps = []
    real = trainer.FusedDecoderTrainer.step
    monkeypatch.setattr(trainer.FusedDecoderTrainer, 'step', lambda self, *a, **k: (steps.append(self.cond), real(self, *a, **k))[1])
    argv = ['--irt-model', '2pl', '--dataset', '2pl_simulation', '--num-person', '600', '--num-item', '12',
            '--epochs', '4', '--batch-size', '16', '--num-posterior-samples', '3', '--cuda', '--native-decoder-step',
            '--conditional-posterior', '--native-conditional-step', '--generative-model', 'deep', '--out-dir', str(tmp_path / 'out')]
    cli.main(argv)
    assert steps and all(steps)                                   # the native conditional trainer ran (eagerly, or once per capture)
    (run_dir,) = os.listdir(tmp_path / 'out')
    ck = torch.load(tmp_path / 'out' / run_dir / 'checkpoint.pth.tar', weights_only=False)
    assert {'model_state_dict', 'epoch', 'args', 'train_logp', 'test_logp'} <= set(ck)
    losses = np.load(tmp_path / 'out' / run_dir / 'train_losses.npy')
    print('epoch losses', losses)
    assert losses.shape == (4,) and np.isfinite(losses).all() and losses[-1] < losses[0]
    a = ck['args']
    fresh = CLS[int(a.irt_model[0])](a.ability_dim, 12, hidden_dim=a.hidden_dim, ability_merge=a.ability_merge,
                                     generative_model=a.generative_model, conditional_posterior=True)
    fresh.load_state_dict(ck['model_state_dict'], strict=True)


if __name__ == '__main__':
    # input selection for the two lists of oracle cases (CPU only)
    print_excluded_shares(False, ORACLE_CASES)
    print_excluded_shares(True, COND_ORACLE_CASES)
