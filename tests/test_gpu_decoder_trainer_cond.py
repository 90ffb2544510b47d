"""FusedDecoderTrainer(conditional=True) (vibo_dtrain_*_cond): the native train step of --generative-model link | deep | residual
with the conditional posterior against the reference's recorded Adam steps, the fp64 oracle, the module + torch.optim.Adam step,
its own hipGraph replay and itself."""
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
# 2. random shapes against the fp64 oracle
# ---------------------------------------------------------------------------
# (decoder, IRT, A, B, I, missing, hidden, drop_missing, seed).  The inputs were picked on the CPU with oracle_trajectory() below
# (`python tests/test_gpu_decoder_trainer_cond.py` prints the figures) so that the float64 gradients leave at most 1.5 % of any
# tensor under the exclusion threshold over the three steps -- inside the 2 % cap with room for the fp32 gradients of the
# module-step test, which applies the same rule to the same problems.  The conditional table's wide last layer and the item
# log-variances have many near-zero gradients at 8 and more ability dimensions: the unconditional file's shapes at A = 8 / 12
# (130 / 260 items) left 3.5-50 % out with seeds 1-12, with 300-600 persons and missing fractions 0-0.1 still 3.5-51 %; at 30
# items (not a multiple of 4; 60 table rows: four tiles, the last one ragged) and 100 persons (seven person tiles, the last one
# ragged) seeds 1, 2, ... reached the bound at seed 6 (A = 8) and seed 15 (A = 12).  Largest excluded share of any tensor with
# the inputs below: 0.70 %, 1.40 %, 1.04 %, 1.39 %, 0.87 %.
ORACLE_CASES = [('link', 3, 1, 33, 95, 0.3, 64, False, 10),
                ('residual', 1, 3, 77, 200, 0.2, 64, True, 4),
                ('deep', 2, 2, 64, 64, 0.0, 32, False, 2),
                ('deep', 2, 8, 100, 30, 0.1, 64, False, 6),
                ('residual', 3, 12, 100, 30, 0.1, 48, False, 15)]
EXCLUDE_BELOW, EXCLUDE_CAP = 1e-4, 0.02


def make_problem(gen, irt, A, B, I, missing, H, drop, seed):
    g = torch.Generator().manual_seed(seed)
    resp, mask = O.simulate_responses(irt, B, I, A, generator=g, missing_frac=missing)
    D = O.item_feat_dim(irt, A)
    eps_item = torch.randn(3, I, D, generator=g)
    eps_ab = torch.randn(3, B, A, generator=g)
    torch.manual_seed(seed)
    model = CLS[irt](A, I, hidden_dim=H, ability_merge='product', generative_model=gen, replace_missing_with_prior=not drop,
                     conditional_posterior=True)
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
                                           annealing_factor=beta, conditional_posterior=True, generative_model=gen)
        if step == 0:
            loss0 = float(out['loss'])
        for k, p in params.items():
            p.grad = grads[k].double()
            keep[k] &= grads[k].abs() >= EXCLUDE_BELOW * grads[k].abs().max()
        opt.step()
        if step in (0, 2):
            after[step + 1] = {k: v.detach().clone() for k, v in params.items()}
    return after, loss0, keep


_ORACLE = {}


def oracle_of(case):
    """The float64 trajectory of a case, computed once and shared (never written to)."""
    if case not in _ORACLE:
        gen, irt, A, B, I, missing, H, drop, seed = case
        model, resp, mask, eps_item, eps_ab = make_problem(*case)
        _ORACLE[case] = oracle_trajectory(model, resp, mask, eps_item, eps_ab, gen, irt, A, drop)
    return _ORACLE[case]


def compare_kept(state, want, keep, tol, what):
    for k, v in want.items():
        dropped = 1.0 - float(keep[k].float().mean())
        assert dropped <= EXCLUDE_CAP, (k, dropped)
        err = float(((state[k].double().cpu() - v.double().cpu()).abs() * keep[k]).max())
        print(what, k, f'err {err:.3e}', f'excluded {dropped:.4f}')
        assert err < tol, (what, k, err)


@pytest.mark.parametrize('gen,irt,A,B,I,missing,H,drop,seed', ORACLE_CASES)
def test_random_shapes_against_the_fp64_oracle(gen, irt, A, B, I, missing, H, drop, seed):
    case = (gen, irt, A, B, I, missing, H, drop, seed)
    model, resp, mask, eps_item, eps_ab = make_problem(*case)
    after, loss0, keep = oracle_of(case)
    d = dev()
    model = model.to(d)
    tr = FusedTrainer(model, lr=5e-3, conditional=True)
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
    tr = FusedTrainer(fus, lr=5e-3, conditional=True)
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
# 4. - 7. replay, reproducibility, chunks, missing-data modes
# ---------------------------------------------------------------------------
def resident(gen, irt, A, P, I, H=64, missing=0.15, seed=7, codes=False, drop=False):
    d = dev()
    g = torch.Generator().manual_seed(seed)
    resp, mask = O.simulate_responses(irt, P, I, A, generator=g, missing_frac=missing)
    resp, mask = ops.pad_rows(resp.to(d), mask.bool().to(d))
    if codes:
        resp, mask = ops.pack_cell_codes(resp, mask), None
    torch.manual_seed(seed)
    model = CLS[irt](A, I, hidden_dim=H, ability_merge='product', generative_model=gen, conditional_posterior=True,
                     replace_missing_with_prior=not drop).to(d)
    return model, resp, mask, g


def state_of(model, tr):
    return ({k: v.clone() for k, v in model.state_dict().items()}, tr.par_m.clone(), tr.par_v.clone(), tr.item_m.clone(), tr.item_v.clone())


def assert_same_state(s0, s1):
    for k in s0[0]:
        assert torch.equal(s0[0][k], s1[0][k]), k
    for a, b in zip(s0[1:], s1[1:]):
        assert torch.equal(a, b)


@pytest.mark.parametrize('gen,irt,A,I,B,codes', [('deep', 2, 2, 100, 16, False), ('link', 3, 1, 95, 16, True)])
def test_replay_is_the_eager_step_bit_for_bit(gen, irt, A, I, B, codes):
    """Three replays of a captured step() -- native Philox noise, a row_index minibatch of a resident matrix refreshed through a
    device buffer -- against three eager steps of a twin: every loss, state_dict tensor and Adam moment torch.equal."""
    P = 5 * B + 3
    m1, resp, mask, g = resident(gen, irt, A, P, I, codes=codes)
    m2 = copy.deepcopy(m1)
    t1 = FusedTrainer(m1, lr=5e-3, rng='native', seed=11, conditional=True)
    t2 = FusedTrainer(m2, lr=5e-3, rng='native', seed=11, conditional=True)
    d = dev()
    rows = torch.randperm(P, generator=g)[:B].to(d)
    for k in range(2):                                   # warm-up (allocations, the resident row counts) before the capture
        assert torch.equal(t1.step(resp, mask, row_index=rows), t2.step(resp, mask, row_index=rows)), k
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        lg = t1.step(resp, mask, row_index=rows)         # capture only: nothing runs
    seen = []
    for k in range(3):
        new_rows = torch.randperm(P, generator=g)[:B].to(d)
        rows.copy_(new_rows)
        graph.replay()
        l2 = t2.step(resp, mask, row_index=new_rows)
        assert torch.equal(lg, l2), (k, float(lg), float(l2))
        assert bool(torch.isfinite(lg))
        seen.append(t1._eps_ab[B].clone())
    assert not any(torch.equal(seen[0], s) for s in seen[1:])                  # fresh noise on every replay
    assert t1._steps.tolist() == t2._steps.tolist() == [5, 5]
    assert_same_state(state_of(m1, t1), state_of(m2, t2))


def test_two_fresh_trainers_are_bitwise_equal():
    gen, irt, A, I, B = 'residual', 3, 2, 200, 77
    res = []
    for _ in range(2):
        model, resp, mask, g = resident(gen, irt, A, B, I)
        tr = FusedTrainer(model, lr=5e-3, rng='native', seed=3, conditional=True)
        losses = [tr.step(resp, mask, beta=0.8).clone() for _ in range(3)]
        res.append((losses, state_of(model, tr)))
    (l0, s0), (l1, s1) = res
    assert all(torch.equal(a, b) and bool(torch.isfinite(a)) for a, b in zip(l0, l1))
    assert_same_state(s0, s1)


def test_person_chunks_change_nothing_but_the_summation_order(monkeypatch):
    """77 persons at PERSON_CHUNK 26 run the person kernels and the decoder in three chunks of 26, 26 and 25 around ONE pair of
    code-table calls: the per-person outputs are those of the one-chunk run bit for bit, the loss to 1e-6, the parameters after
    the step to TOL_ADAM1."""
    gen, irt, A, I, B = 'residual', 3, 2, 200, 77
    d = dev()
    res = []
    for chunk in (1 << 20, 26):
        monkeypatch.setattr(decoder, 'PERSON_CHUNK', chunk)
        model, resp, mask, g = resident(gen, irt, A, B, I)
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


@pytest.mark.parametrize('codes', [False, True])
def test_missing_data_modes_and_the_all_missing_row(codes):
    """Prior expert: a person without an observed cell gets exactly the prior-only posterior, mu = 0 and logvar = log(1 / (I / (1 +
    1e-8))), whatever the table holds, and nothing of the step is NaN.  --drop-missing on the same rows without that person: the
    posterior is the observed experts' alone (against models._conditional_posterior_poe)."""
    gen, irt, A, I, B = 'deep', 2, 3, 45, 21
    d = dev()
    g = torch.Generator().manual_seed(9)
    resp, mask = O.simulate_responses(irt, B, I, A, generator=g, missing_frac=0.3)
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
    # input selection for ORACLE_CASES (CPU only): the largest share of any tensor the exclusion rule would leave out
    for case in ORACLE_CASES:
        _, _, keep = oracle_of(case)
        worst = max((1.0 - float(v.float().mean()), k) for k, v in keep.items())
        print(case, 'largest excluded share %.4f (%s)' % worst, 'ok' if worst[0] <= EXCLUDE_CAP else 'TRY OTHER INPUTS')
