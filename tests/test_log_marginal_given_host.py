"""log_marginal of the models whose posterior reaches the kernel as given (--ability-merge mean with or without the conditional
posterior, VI_*PL), host side: ONE call of the multi-sample backend per log_marginal, with the posterior shared by the samples
([B, 2A]) or stacked per sample ([S, B, 2A]), the flowed items, the reference's goldens reproduced through it and through the loop
it falls back to.  CPU stand-in (oracle/cpu_backend.py) with a recording fake in ops._BACKEND['multi']; the same path runs on the
HIP kernel in tests/test_gpu_multi_given.py."""
import os

import pytest
import torch

from conftest import GOLDEN_DIR, Golden
from golden_common import build_model
from oracle import cpu_backend
from recording_multi import RecordingMulti
from vibo_amd import _lib, ops
from vibo_amd.torch_core.models import VI_2PL, VIBO_2PL

NEW_GOLDENS = ['logmarg_2pl_a2_mean', 'logmarg_2pl_a2_cond_mean', 'logmarg_3pl_a1_mean_flows2']


@pytest.fixture()
def multi():
    restore = cpu_backend.install(ops)
    fake = RecordingMulti(given=True)
    ops._BACKEND['multi'] = fake
    yield fake
    restore()


@pytest.fixture()
def cpu_ops():
    restore = cpu_backend.install(ops)
    yield
    restore()


def golden_log_marginal(g, model):
    return model.log_marginal(g.response.unsqueeze(2), g.mask.long().unsqueeze(2), num_samples=g.meta['num_samples'],
                              eps_item=g.eps_item, eps_ability=g.eps_ability)


@pytest.mark.parametrize('name', NEW_GOLDENS)
def test_goldens_through_one_multi_sample_call(name, multi):
    g = Golden(os.path.join(GOLDEN_DIR, name + '.npz'))
    m = g.meta
    assert m['ability_merge'] == 'mean'
    model = build_model(g)
    logp = golden_log_marginal(g, model)
    ref = float(g.out['logp'])
    assert abs(float(logp) - ref) < 1e-4 * max(1.0, abs(ref))
    assert len(multi.calls) == 1
    c = multi.calls[0]
    S, B, A, I = m['num_samples'], m['num_person'], m['ability_dim'], m['num_item']
    assert tuple(c['table'].shape) == ((S, B, 2 * A) if m['conditional_posterior'] else (B, 2 * A))
    assert tuple(c['eps'].shape) == (S, B, A) and torch.equal(c['eps'], g.eps_ability) and c['num_person'] == B
    # the items of sample s: the reparameterised item sample, pushed through the item flows where the model has them
    with torch.no_grad():
        item_mu, item_lv = model.item_encoder()
        feat = g.eps_item * torch.exp(0.5 * item_lv) + item_mu
        want = torch.stack([model.item_norm_flows(f)[0] for f in feat]) if m['n_norm_flows'] else feat
    assert tuple(c['items'].shape) == (S, I, model.item_feat_dim) and torch.allclose(c['items'], want, rtol=0, atol=1e-6)
    if m['n_norm_flows']:
        assert float((want - feat).abs().max()) > 1e-3 and tuple(c['flow'].shape) == (m['n_norm_flows'], 2 * A + 1)
    else:
        assert c['flow'] is None
    if m['conditional_posterior']:      # one posterior per item sample
        assert float((c['table'][0] - c['table'][1]).abs().max()) > 1e-6


@pytest.mark.parametrize('name', NEW_GOLDENS)
def test_goldens_through_the_loop_fallback(name, cpu_ops):
    """The stock stand-in answers None: one forward per sample on the noise handed in."""
    g = Golden(os.path.join(GOLDEN_DIR, name + '.npz'))
    logp = golden_log_marginal(g, build_model(g))
    ref = float(g.out['logp'])
    assert abs(float(logp) - ref) < 1e-4 * max(1.0, abs(ref))


@pytest.mark.parametrize('cond', [False, True])
def test_drawn_noise_is_the_loops(cond, multi):
    """No noise supplied: the multi-sample path draws item then ability noise per sample from the same generators, so a seeded
    caller gets the loop's number."""
    torch.manual_seed(3)
    model = VIBO_2PL(2, 20, ability_merge='mean', conditional_posterior=cond)
    g = torch.Generator().manual_seed(5)
    resp = (torch.rand(12, 20, generator=g) < 0.5).float()
    mask = torch.rand(12, 20, generator=g) < 0.8
    torch.manual_seed(11)
    a = model.log_marginal(resp, mask, num_samples=5)
    assert len(multi.calls) == 1
    ops._BACKEND['multi'] = lambda *args: None
    torch.manual_seed(11)
    b = model.log_marginal(resp, mask, num_samples=5)
    assert abs(float(a) - float(b)) < 1e-5 * max(1.0, abs(float(b)))


def test_person_sharded_model_keeps_the_loop(multi):
    torch.manual_seed(4)
    model = VIBO_2PL(2, 20, ability_merge='mean')
    reduced = []

    def reducer(flat):          # world 1: the sum over the ranks is the tensor itself
        reduced.append(flat.numel())
        return flat
    model.enable_person_sharding(reducer, seed=0, rank=0, world=1)
    g = torch.Generator().manual_seed(6)
    resp = (torch.rand(10, 20, generator=g) < 0.5).float()
    mask = torch.rand(10, 20, generator=g) < 0.8
    logp = model.log_marginal(resp, mask, num_samples=3)
    assert torch.isfinite(logp) and multi.calls == [] and len(reduced) >= 3


def test_vi_log_marginal_shares_the_looked_up_rows(multi):
    torch.manual_seed(8)
    model = VI_2PL(2, 30, 20)
    g = torch.Generator().manual_seed(9)
    idx = torch.randperm(30, generator=g)[:12]
    resp = (torch.rand(12, 20, generator=g) < 0.5).float()
    mask = torch.rand(12, 20, generator=g) < 0.8
    torch.manual_seed(21)
    a = model.log_marginal(idx, resp, mask, num_samples=4)
    assert len(multi.calls) == 1
    c = multi.calls[0]
    want = torch.cat([model.ability_mu_lookup(idx), model.ability_logvar_lookup(idx)], dim=1).detach()
    assert tuple(c['table'].shape) == (12, 4) and torch.equal(c['table'], want) and tuple(c['items'].shape) == (4, 20, 3)
    # the loop it replaces, under the same seed: forward + elbo per sample, noise from the default generator
    ops._BACKEND['multi'] = lambda *args: None
    torch.manual_seed(21)
    b = model.log_marginal(idx, resp, mask, num_samples=4)
    torch.manual_seed(21)
    with torch.no_grad():
        lw = torch.stack([-model.elbo(*model(idx, resp, mask), annealing_factor=1, use_kl_divergence=False) for _ in range(4)])
    c_ = torch.logsumexp(lw, 0) - torch.log(torch.tensor(4.0))
    assert abs(float(a) - float(c_)) < 1e-5 * max(1.0, abs(float(c_))) and abs(float(b) - float(c_)) < 1e-5 * max(1.0, abs(float(c_)))


@pytest.mark.parametrize('cond', [False, True])
def test_loop_fallback_reuses_the_posteriors_already_computed(cond, cpu_ops, monkeypatch):
    """The backend answers None after _draw_samples has computed the posteriors: the loop takes those, it does not encode the
    rows a second time (one _mean_posterior call for the shared posterior, S for the conditional one)."""
    torch.manual_seed(13)
    model = VIBO_2PL(2, 20, ability_merge='mean', conditional_posterior=cond)
    g = torch.Generator().manual_seed(14)
    resp = (torch.rand(12, 20, generator=g) < 0.5).float()
    mask = torch.rand(12, 20, generator=g) < 0.8
    calls, inner = [], model._mean_posterior
    monkeypatch.setattr(model, '_mean_posterior', lambda *a, **k: calls.append(1) or inner(*a, **k))
    S = 5
    torch.manual_seed(15)
    a = model.log_marginal(resp, mask, num_samples=S)
    assert len(calls) == (S if cond else 1)
    # the loop on its own (what a person-sharded model runs) gives the same number from the same noise
    torch.manual_seed(15)
    with torch.no_grad():
        lw = []
        for _ in range(S):
            ctx = model._run_fused(resp, mask, reg_mode=_lib.REG_SAMPLED)
            lw.append(ctx.ll + (-0.5 * 1.8378770664093453 - 0.5 * ctx.item_k ** 2).sum() - ctx.reg
                      - (-0.5 * 1.8378770664093453 - 0.5 * ctx.item_lv - 0.5 * (ctx.item_feat - ctx.item_mu) ** 2 / ctx.item_lv.exp()).sum())
        b = torch.logsumexp(torch.stack(lw), 0) - torch.log(torch.tensor(float(S)))
    assert abs(float(a) - float(b)) < 1e-5 * max(1.0, abs(float(b)))
