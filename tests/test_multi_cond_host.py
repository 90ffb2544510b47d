"""log_marginal of the product of experts x conditional posterior, host side: ONE call of the multi-sample backend per
log_marginal, with the conditional spec, the encoder's table of every item sample stacked to [S, 2, I, 2A] (expert_table of the
sample in front of the item flows) and the flowed items; the loop's draw order; the loop it falls back to on the same noise; the
callers that keep the loop.  CPU stand-in (oracle/cpu_backend.py) with a recording fake in ops._BACKEND['multi']; the same path
runs on the HIP kernels in tests/test_gpu_multi_cond.py."""
import os

import pytest
import torch

from conftest import GOLDEN_DIR, Golden
from golden_common import build_model
from oracle import cpu_backend
from recording_multi import RecordingMulti
from vibo_amd import _lib, ops
from vibo_amd.torch_core.models import VIBO_2PL, VIBO_3PL


@pytest.fixture()
def multi():
    restore = cpu_backend.install(ops)
    fake = RecordingMulti()
    ops._BACKEND['multi'] = fake
    yield fake
    restore()


def build(kind):
    torch.manual_seed(17)
    if kind == '3pl_a1_flows2':
        return VIBO_3PL(1, 95, ability_merge='product', conditional_posterior=True, n_norm_flows=2)
    return VIBO_2PL(5, 100, ability_merge='product', conditional_posterior=True, replace_missing_with_prior=False)


def rows_of(model, B=24, seed=19):
    g = torch.Generator().manual_seed(seed)
    I = model.num_item
    return (torch.rand(B, I, generator=g) < 0.5).float(), torch.rand(B, I, generator=g) < 0.8


def close(a, b):
    return abs(float(a) - float(b)) < 1e-5 * max(1.0, abs(float(b)))


@pytest.mark.parametrize('kind', ['3pl_a1_flows2', '2pl_a5_drop'])
def test_backend_receives_the_stacked_tables_and_the_flowed_items(kind, multi):
    model = build(kind)
    resp, mask = rows_of(model)
    S, B, A, I = 6, resp.shape[0], model.ability_dim, model.num_item
    g = torch.Generator().manual_seed(23)
    eps_item, eps_ab = torch.randn(S, I, model.item_feat_dim, generator=g), torch.randn(S, B, A, generator=g)
    a = model.log_marginal(resp, mask, num_samples=S, eps_item=eps_item, eps_ability=eps_ab)
    assert len(multi.calls) == 1
    c = multi.calls[0]
    assert c['spec'] == model.spec and c['spec'].conditional and not c['spec'].given and c['num_person'] == B
    assert c['spec'].drop_missing == (kind == '2pl_a5_drop')
    with torch.no_grad():
        item_mu, item_lv = model.item_encoder()
        feat = eps_item * torch.exp(0.5 * item_lv) + item_mu
        want_tables = torch.stack([model.ability_encoder.expert_table(f) for f in feat])          # in front of the item flows
        want_items = torch.stack([model.item_norm_flows(f)[0] for f in feat]) if model.n_norm_flows else feat
    assert tuple(c['table'].shape) == (S, 2, I, 2 * A) and c['table'].is_contiguous() and torch.equal(c['table'], want_tables)
    assert float((c['table'][0] - c['table'][1]).abs().max()) > 1e-6          # one table per item sample
    assert tuple(c['items'].shape) == (S, I, model.item_feat_dim) and torch.allclose(c['items'], want_items, rtol=0, atol=1e-6)
    assert tuple(c['eps'].shape) == (S, B, A) and torch.equal(c['eps'], eps_ab)
    if model.n_norm_flows:
        assert float((want_items - feat).abs().max()) > 1e-3 and tuple(c['flow'].shape) == (model.n_norm_flows, 2 * A + 1)
    else:
        assert c['flow'] is None
    # the loop it replaces, on the same noise
    ops._BACKEND['multi'] = lambda *args: None
    b = model.log_marginal(resp, mask, num_samples=S, eps_item=eps_item, eps_ability=eps_ab)
    assert close(a, b), (float(a), float(b))


def test_golden_through_one_multi_sample_call(multi):
    g = Golden(os.path.join(GOLDEN_DIR, 'logmarg_3pl_a1_cond_flows2.npz'))
    m = g.meta
    assert m['conditional_posterior'] and m.get('ability_merge', 'product') == 'product'
    logp = build_model(g).log_marginal(g.response.unsqueeze(2), g.mask.long().unsqueeze(2), num_samples=m['num_samples'],
                                       eps_item=g.eps_item, eps_ability=g.eps_ability)
    ref = float(g.out['logp'])
    assert abs(float(logp) - ref) < 1e-4 * max(1.0, abs(ref)) and len(multi.calls) == 1
    assert tuple(multi.calls[0]['table'].shape) == (m['num_samples'], 2, m['num_item'], 2 * m['ability_dim'])


@pytest.mark.parametrize('kind', ['3pl_a1_flows2', '2pl_a5_drop'])
def test_drawn_noise_is_the_loops_and_is_replayed_after_none(kind, multi):
    """No noise supplied: item then ability noise per sample from the model's generators, so a seeded caller gets the loop's
    number; a backend that answers None after the draw leaves the loop the same noise (every single forward is handed the item and
    ability noise the multi-sample call saw) and the same number."""
    model = build(kind)
    resp, mask = rows_of(model)
    S = 5
    torch.manual_seed(11)
    a = model.log_marginal(resp, mask, num_samples=S)
    assert len(multi.calls) == 1
    seen = multi.calls[0]
    # the loop alone under the same seed
    ops._BACKEND['multi'] = lambda *args: None
    torch.manual_seed(11)
    b = model.log_marginal(resp, mask, num_samples=S)
    assert close(a, b), (float(a), float(b))
    # a backend that draws nothing itself, sees the call and refuses it
    refusing = RecordingMulti(answer=False)
    ops._BACKEND['multi'] = refusing
    singles, inner = [], ops._BACKEND['elbo']

    def elbo(spec, response, mask_, mask_code, row_index, table, item, eps, *rest):
        singles.append((table, item, eps))
        return inner(spec, response, mask_, mask_code, row_index, table, item, eps, *rest)
    ops._BACKEND['elbo'] = elbo
    torch.manual_seed(11)
    c = model.log_marginal(resp, mask, num_samples=S)
    assert close(c, b) and len(refusing.calls) == 1 and len(singles) == S
    r = refusing.calls[0]
    assert torch.equal(r['eps'], seen['eps']) and torch.equal(r['items'], seen['items']) and torch.equal(r['table'], seen['table'])
    for s, (table, item, eps) in enumerate(singles):
        assert torch.equal(eps, r['eps'][s]) and torch.allclose(item, r['items'][s], rtol=0, atol=1e-6)
        assert torch.allclose(table, r['table'][s], rtol=0, atol=1e-6)


def test_person_sharded_model_keeps_the_loop(multi):
    model = build('2pl_a5_drop')
    reduced = []

    def reducer(flat):          # world 1: the sum over the ranks is the tensor itself
        reduced.append(flat.numel())
        return flat
    model.enable_person_sharding(reducer, seed=0, rank=0, world=1)
    resp, mask = rows_of(model, B=10)
    logp = model.log_marginal(resp, mask, num_samples=3)
    assert torch.isfinite(logp) and multi.calls == [] and len(reduced) >= 3


def test_an_int64_mask_never_reaches_the_backend_with_a_conditional_table(multi):
    """The library's multi-sample calls refuse int64 masks (-8).  log_marginal narrows the reference loop's `.long()` mask before
    the backend sees it: whatever reaches 'multi' with a [S, 2, I, 2A] table carries a uint8 mask; rows handed over as int64
    (VIBO_MASK_I64) are turned back before anything is drawn."""
    model = build('3pl_a1_flows2')
    resp, mask = rows_of(model)
    torch.manual_seed(5)
    a = model.log_marginal(resp, mask.long(), num_samples=4)
    torch.manual_seed(5)
    b = model.log_marginal(resp, mask, num_samples=4)
    assert close(a, b) and len(multi.calls) == 2
    for c in multi.calls:
        assert c['table'].dim() == 4 and c['mask_code'] == _lib.MASK_U8 and c['mask'].dtype == torch.uint8
    # _draw_samples itself, were a caller to keep the int64 form: None, no call, no draw
    multi.calls.clear()
    state = torch.get_rng_state()
    seen = []
    real = ops.prepare_rows
    try:
        ops.prepare_rows = lambda r, m, keep_int64=False: seen.append(1) or real(r, m, keep_int64=True)
        out = model._draw_samples(resp, mask.long(), 4, None, None)
    finally:
        ops.prepare_rows = real
    assert seen and out is None and multi.calls == [] and torch.equal(torch.get_rng_state(), state)
