"""FusedDecoderTrainer (vibo_dtrain_* around vibo_decoder_fwd_bwd): the native train step of --generative-model link | deep |
residual against the reference's recorded Adam steps, the fp64 oracle, the module + torch.optim.Adam step, its own hipGraph replay
and itself."""
import copy
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR, Golden, rel_err
from oracle import vibo_oracle as O
from test_host_logic import build_model
from vibo_amd import decoder, ops
from vibo_amd.torch_core.models import VIBO_1PL, VIBO_2PL, VIBO_3PL
from vibo_amd.trainer import FusedDecoderTrainer, FusedTrainer

pytestmark = pytest.mark.gpu
CLS = {1: VIBO_1PL, 2: VIBO_2PL, 3: VIBO_3PL}
TOL_ELBO, TOL_ADAM1, TOL_ADAM3 = 1e-4, 2e-4, 5e-4       # test_golden_adam_trajectory_through_the_fused_trainers' bounds


def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


# ---------------------------------------------------------------------------
# 1. the reference's recorded Adam steps
# ---------------------------------------------------------------------------
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
    resp, mask = ops.pad_rows(golden.response.to(d), golden.mask.to(d).bool())
    eps_i, eps_a = golden.eps_item.to(d), golden.eps_ability.to(d)
    row_index = None
    if rows == 'gathered':
        B, I = golden.response.shape
        g = torch.Generator().manual_seed(B * I)
        big_r = (torch.rand(3 * B + 5, I, generator=g) < 0.5).float()
        big_m = torch.rand(3 * B + 5, I, generator=g) < 0.8
        where = torch.randperm(3 * B + 5, generator=g)[:B]
        big_r[where], big_m[where] = golden.response, golden.mask.bool()
        resp, mask = ops.pad_rows(big_r.to(d), big_m.to(d))
        row_index = where.to(d)
    elif rows == 'cell-codes':
        resp, mask = ops.pack_cell_codes(golden.response.to(d), golden.mask.to(d).bool()), None
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


# ---------------------------------------------------------------------------
# 2. random shapes against the fp64 oracle
# ---------------------------------------------------------------------------
# (decoder, IRT, A, B, I, missing, hidden, drop_missing, seed).  The seeds were picked on the CPU with oracle_trajectory() below
# (`python tests/test_gpu_decoder_trainer.py` prints the figures): seeds 1, 2, ... were tried per case until the float64
# gradients left at most 1.5 % of any tensor under the exclusion threshold over the three steps -- inside the 2 % cap with room
# for the fp32 gradients of the module-step test, which applies the same rule to the same problems.  Largest excluded share of
# any tensor with the seeds below: 1.0 %, 1.3 %, 1.1 %, 1.5 %, 1.3 %.
ORACLE_CASES = [('link', 3, 1, 33, 95, 0.3, 64, False, 1),
                ('deep', 2, 8, 300, 130, 0.1, 64, False, 2),
                ('residual', 1, 3, 77, 200, 0.2, 64, True, 8),
                ('deep', 2, 2, 64, 64, 0.0, 32, False, 5),
                ('residual', 3, 12, 40, 260, 0.1, 48, False, 9)]
EXCLUDE_BELOW, EXCLUDE_CAP = 1e-4, 0.02


def make_problem(gen, irt, A, B, I, missing, H, drop, seed):
    g = torch.Generator().manual_seed(seed)
    resp, mask = O.simulate_responses(irt, B, I, A, generator=g, missing_frac=missing)
    D = O.item_feat_dim(irt, A)
    eps_item = torch.randn(3, I, D, generator=g)
    eps_ab = torch.randn(3, B, A, generator=g)
    torch.manual_seed(seed)
    model = CLS[irt](A, I, hidden_dim=H, ability_merge='product', generative_model=gen, replace_missing_with_prior=not drop)
    return model, resp, mask, eps_item, eps_ab


def oracle_trajectory(model, resp, mask, eps_item, eps_ab, gen, irt, A, drop, beta=1.0):
    """Three float64 torch.optim.Adam steps (lr 5e-3) on the oracle's gradients.  Returns the parameters after steps 1 and 3, the
    first loss, and per tensor the entries to compare: Adam normalises the step, so an entry whose gradient is at rounding level
    moves by a full +-lr either way -- entries whose float64 gradient is below 1e-4 of the tensor's max-abs in any step are left out."""
    params = {k: v.detach().double().clone().requires_grad_(True) for k, v in model.state_dict().items()}
    opt = torch.optim.Adam(list(params.values()), lr=5e-3)
    keep = {k: torch.ones_like(v, dtype=torch.bool) for k, v in params.items()}
    after, loss0 = {}, None
    for step in range(3):
        out, grads = O.elbo_loss_and_grads({k: v.detach() for k, v in params.items()}, resp.double(), mask, eps_item[step].double(),
                                           eps_ab[step].double(), irt_model=irt, ability_dim=A, replace_missing_with_prior=not drop,
                                           annealing_factor=beta, generative_model=gen)
        if step == 0:
            loss0 = float(out['loss'])
        for k, p in params.items():
            p.grad = grads[k].double()
            keep[k] &= grads[k].abs() >= EXCLUDE_BELOW * grads[k].abs().max()
        opt.step()
        if step in (0, 2):
            after[step + 1] = {k: v.detach().clone() for k, v in params.items()}
    return after, loss0, keep


def compare_kept(state, want, keep, tol, what):
    for k, v in want.items():
        dropped = 1.0 - float(keep[k].float().mean())
        assert dropped <= EXCLUDE_CAP, (k, dropped)
        err = float(((state[k].double().cpu() - v.double().cpu()).abs() * keep[k]).max())
        print(what, k, f'err {err:.3e}', f'excluded {dropped:.4f}')
        assert err < tol, (what, k, err)


@pytest.mark.parametrize('gen,irt,A,B,I,missing,H,drop,seed', ORACLE_CASES)
def test_random_shapes_against_the_fp64_oracle(gen, irt, A, B, I, missing, H, drop, seed):
    model, resp, mask, eps_item, eps_ab = make_problem(gen, irt, A, B, I, missing, H, drop, seed)
    after, loss0, keep = oracle_trajectory(model, resp, mask, eps_item, eps_ab, gen, irt, A, drop)
    d = dev()
    model = model.to(d)
    tr = FusedTrainer(model, lr=5e-3)
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
@pytest.mark.parametrize('gen,irt,A,B,I,missing,H,drop,seed', ORACLE_CASES)
def test_native_step_equals_the_module_step(gen, irt, A, B, I, missing, H, drop, seed):
    """Both fp32: the bounds and the exclusion rule of the oracle test on the same problems, the threshold taken on the module
    path's own gradients."""
    model, resp, mask, eps_item, eps_ab = make_problem(gen, irt, A, B, I, missing, H, drop, seed)
    d = dev()
    ref = model.to(d)
    fus = copy.deepcopy(ref)
    opt = torch.optim.Adam(ref.parameters(), lr=5e-3)
    tr = FusedTrainer(fus, lr=5e-3)
    r, m = ops.pad_rows(resp.to(d), mask.bool().to(d))
    names = [k for k, _ in ref.named_parameters()]
    assert names == list(ref.state_dict().keys())
    keep = {k: torch.ones_like(v, dtype=torch.bool) for k, v in ref.state_dict().items()}
    for step in range(3):
        opt.zero_grad()
        outs = ref(r, m, eps_item=eps_item[step].to(d), eps_ability=eps_ab[step].to(d))
        loss_ref = ref.elbo(*outs, annealing_factor=1.0)
        loss_ref.backward()
        for k, p in ref.named_parameters():
            keep[k] &= p.grad.abs() >= EXCLUDE_BELOW * p.grad.abs().max()
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
# 4. - 7. replay, reproducibility, chunks, external writes
# ---------------------------------------------------------------------------
def resident(gen, irt, A, P, I, H=64, missing=0.15, seed=7, codes=False):
    d = dev()
    g = torch.Generator().manual_seed(seed)
    resp, mask = O.simulate_responses(irt, P, I, A, generator=g, missing_frac=missing)
    resp, mask = ops.pad_rows(resp.to(d), mask.bool().to(d))
    if codes:
        resp, mask = ops.pack_cell_codes(resp, mask), None
    torch.manual_seed(seed)
    model = CLS[irt](A, I, hidden_dim=H, ability_merge='product', generative_model=gen).to(d)
    return model, resp, mask, g


@pytest.mark.parametrize('gen,irt,A,I,B,codes', [('deep', 2, 2, 100, 16, False), ('link', 3, 1, 95, 16, True),
                                                 ('residual', 3, 3, 130, 48, False)])
def test_replay_is_the_eager_step_bit_for_bit(gen, irt, A, I, B, codes):
    """A captured step() replayed 60 times -- row_index refreshed through a device buffer, beta changed between replays, a shorter
    eager minibatch in between -- against eager steps of a twin: every loss and state_dict tensor torch.equal, fresh noise on
    every replay (the step counters live on the device)."""
    P = 5 * B + 3
    m1, resp, mask, g = resident(gen, irt, A, P, I, codes=codes)
    m2 = copy.deepcopy(m1)
    t1 = FusedTrainer(m1, lr=5e-3, rng='native', seed=11)
    t2 = FusedTrainer(m2, lr=5e-3, rng='native', seed=11)
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
        seen.append(t1._eps_ab[B].clone())
    assert not any(torch.equal(seen[0], s) for s in seen[1:])
    assert t1._steps.tolist() == t2._steps.tolist() == [63, 63]
    for (k, a), (_, b) in zip(m1.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), k
    assert torch.equal(t1.par_m, t2.par_m) and torch.equal(t1.par_v, t2.par_v)


@pytest.mark.parametrize('gen,irt,A,I,B', [('deep', 2, 8, 130, 300), ('link', 2, 1, 95, 33), ('residual', 3, 2, 200, 77)])
def test_two_fresh_trainers_are_bitwise_equal(gen, irt, A, I, B):
    res = []
    for _ in range(2):
        model, resp, mask, g = resident(gen, irt, A, B, I)
        tr = FusedTrainer(model, lr=5e-3, rng='native', seed=3)
        losses = [tr.step(resp, mask, beta=0.8).clone() for _ in range(5)]
        res.append((losses, {k: v.clone() for k, v in model.state_dict().items()}, tr.par_m.clone(), tr.item_v.clone()))
    (l0, s0, m0, v0), (l1, s1, m1, v1) = res
    assert all(torch.equal(a, b) for a, b in zip(l0, l1))
    for k in s0:
        assert torch.equal(s0[k], s1[k]), k
    assert torch.equal(m0, m1) and torch.equal(v0, v1)


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
        model, resp, mask, g = resident(gen, irt, A, B, I)
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


def test_external_parameter_writes_and_refusals():
    B, I, A = 40, 64, 2
    d = dev()
    model, resp, mask, g = resident('deep', 2, A, B, I)
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
    model, resp, mask, g = resident('deep', 2, A, 80, I, missing=0.0)
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


if __name__ == '__main__':
    # seed selection for ORACLE_CASES (CPU only): the largest share of any tensor the exclusion rule would leave out
    for case in ORACLE_CASES:
        gen, irt, A, B, I, missing, H, drop, seed = case
        model, resp, mask, eps_item, eps_ab = make_problem(*case)
        _, _, keep = oracle_trajectory(model, resp, mask, eps_item, eps_ab, gen, irt, A, drop)
        worst = max((1.0 - float(v.float().mean()), k) for k, v in keep.items())
        print(case, 'largest excluded share %.4f (%s)' % worst, 'ok' if worst[0] <= EXCLUDE_CAP else 'TRY ANOTHER SEED')
