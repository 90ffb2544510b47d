"""log_marginal and posterior_predictive of the MLP-decoder models (--generative-model link | deep | residual), host side: ONE call
of ops._BACKEND['decoder_multi'] with the S samples stacked, the loop's draw order, the loop they fall back to on the same noise,
the person-sharded models that keep the loop; the second header's exports and their argument checks.  CPU stand-in
(oracle/cpu_backend.py) with a recording fake in ops._BACKEND['decoder_multi'] that evaluates sample by sample on the stand-in's
'decoder'; the same path runs on the HIP kernel in tests/test_gpu_decoder_multi.py."""
import ctypes
import types

import pytest
import torch

from oracle import cpu_backend
from vibo_amd import _lib, decoder, ops
from vibo_amd.torch_core import vibo
from vibo_amd.torch_core.models import VIBO_2PL, VIBO_3PL


class RecordingDecoderMulti:
    """Stands in for decoder._launch_multi: records the stacked arguments and answers with the CPU 'decoder' stand-in sample by
    sample (answer=False: records and answers None, "not covered")."""

    def __init__(self, answer=True):
        self.calls, self.answer = [], answer

    def __call__(self, response, mask, U, V, L, guess, w1, W2, b2, w3, b3, resid, prob_sum=None, prob_accumulate=False):
        self.calls.append(dict(response=response, mask=mask, U=U, V=V, L=L, guess=guess, w1=w1, W2=W2, resid=resid,
                               prob_sum=prob_sum is not None, prob_accumulate=prob_accumulate))
        if not self.answer:
            return None
        S, parts = V.shape[0], []
        for s in range(S):
            out = ops._BACKEND['decoder'](response, mask, None if U is None else U[s], V[s], None if L is None else L[s],
                                          None if guess is None else guess[s], w1, W2, b2, w3, b3, resid, False,
                                          want_prob=prob_sum is not None)
            parts.append(out['ll_part'])
            if prob_sum is not None:
                if s == 0 and not prob_accumulate:
                    prob_sum.copy_(out['prob'])
                else:
                    prob_sum.add_(out['prob'])
        return {'ll_part': torch.stack(parts)}


@pytest.fixture()
def multi():
    restore = cpu_backend.install(ops)
    saved = ops._BACKEND.get('decoder_multi')
    fake = RecordingDecoderMulti()
    ops._BACKEND['decoder_multi'] = fake
    yield fake
    ops._BACKEND['decoder_multi'] = saved
    restore()


KINDS = {
    'deep2': lambda: VIBO_2PL(2, 20, ability_merge='product', generative_model='deep'),
    'link3': lambda: VIBO_3PL(1, 20, ability_merge='product', generative_model='link'),
    'residual2_flows2': lambda: VIBO_2PL(2, 20, ability_merge='product', generative_model='residual', n_norm_flows=2),
    'deep2_cond': lambda: VIBO_2PL(2, 20, ability_merge='product', generative_model='deep', conditional_posterior=True),
    'deep2_mean': lambda: VIBO_2PL(2, 20, ability_merge='mean', generative_model='deep'),
    'link2_h32': lambda: VIBO_2PL(2, 20, ability_merge='product', generative_model='link', hidden_dim=32),
}


def build(kind):
    torch.manual_seed(17)
    return KINDS[kind]()


def rows_of(model, B=12, seed=19):
    g = torch.Generator().manual_seed(seed)
    I = model.num_item
    return (torch.rand(B, I, generator=g) < 0.5).float(), torch.rand(B, I, generator=g) < 0.8


def close(a, b):
    return abs(float(a) - float(b)) < 1e-5 * max(1.0, abs(float(b)))


def without_multi():
    ops._BACKEND.pop('decoder_multi', None)


@pytest.mark.parametrize('kind', sorted(KINDS))
def test_log_marginal_is_one_stacked_call_that_agrees_with_the_loop(kind, multi):
    model = build(kind)
    resp, mask = rows_of(model)
    S, B, A, I, H = 5, resp.shape[0], model.ability_dim, model.num_item, decoder.HIDDEN
    g = torch.Generator().manual_seed(23)
    eps_item, eps_ab = torch.randn(S, I, model.item_feat_dim, generator=g), torch.randn(S, B, A, generator=g)
    a = model.log_marginal(resp, mask, num_samples=S, eps_item=eps_item, eps_ability=eps_ab)
    assert len(multi.calls) == 1
    c = multi.calls[0]
    gen = model.generative_model
    assert tuple(c['V'].shape) == (S, B, H) and c['V'].is_contiguous() and tuple(c['W2'].shape) == (H, H)
    assert tuple(c['response'].shape) == (B, I) and c['mask'].dtype == torch.uint8 and not c['prob_sum']
    if gen == 'link':
        assert c['U'] is None and tuple(c['w1'].shape) == (H,) and c['resid'] == 0.0
    else:
        assert tuple(c['U'].shape) == (S, I, H) and c['w1'] is None and c['resid'] == (1.0 if gen == 'residual' else 0.0)
        assert float((c['U'][0] - c['U'][1]).abs().max()) > 1e-6          # one item half per item sample
    if gen == 'deep':
        assert c['L'] is None and c['guess'] is None
    else:
        assert tuple(c['L'].shape) == (S, B, I) and c['L'].is_contiguous()
        assert (tuple(c['guess'].shape) == (S, I)) if model.irt_num == 3 else c['guess'] is None
    # the loop it replaces, on the same noise: the backend entry removed
    without_multi()
    b = model.log_marginal(resp, mask, num_samples=S, eps_item=eps_item, eps_ability=eps_ab)
    assert close(a, b), (float(a), float(b))


@pytest.mark.parametrize('kind', ['deep2', 'residual2_flows2', 'deep2_cond'])
def test_drawn_noise_is_the_loops_and_is_replayed_after_none(kind, multi):
    """No noise supplied: item then ability noise per sample, so a seeded caller gets the loop's number and leaves the generator
    where the loop leaves it; a backend that answers None after the draw leaves the loop the same noise."""
    model = build(kind)
    resp, mask = rows_of(model)
    S = 4
    torch.manual_seed(11)
    a = model.log_marginal(resp, mask, num_samples=S)
    state_multi = torch.get_rng_state()
    assert len(multi.calls) == 1
    seen = multi.calls[0]
    refusing = RecordingDecoderMulti(answer=False)
    ops._BACKEND['decoder_multi'] = refusing
    singles, inner = [], ops._BACKEND['decoder']

    def single(response, mask_, U, V, *rest, **kw):
        singles.append((U, V))
        return inner(response, mask_, U, V, *rest, **kw)
    ops._BACKEND['decoder'] = single
    torch.manual_seed(11)
    c = model.log_marginal(resp, mask, num_samples=S)
    state_refused = torch.get_rng_state()
    assert len(refusing.calls) == 1 and len(singles) == S and torch.equal(refusing.calls[0]['V'], seen['V'])
    for s, (U, V) in enumerate(singles):      # every single launch is handed the sample the stacked call saw
        assert torch.allclose(V, seen['V'][s], rtol=0, atol=1e-6) and torch.allclose(U, seen['U'][s], rtol=0, atol=1e-6)
    ops._BACKEND['decoder'] = inner
    without_multi()
    torch.manual_seed(11)
    b = model.log_marginal(resp, mask, num_samples=S)
    state_loop = torch.get_rng_state()
    assert close(a, b) and close(c, b), (float(a), float(b), float(c))
    assert torch.equal(state_multi, state_loop) and torch.equal(state_refused, state_loop)


def test_person_sharded_model_keeps_the_loop(multi):
    model = build('deep2')
    model.enable_person_sharding(lambda flat: flat, seed=0, rank=0, world=1)
    resp, mask = rows_of(model, B=10)
    singles, inner = [], ops._BACKEND['decoder']
    ops._BACKEND['decoder'] = lambda *a, **k: singles.append(1) or inner(*a, **k)
    logp = model.log_marginal(resp, mask, num_samples=3)
    assert torch.isfinite(logp) and multi.calls == [] and len(singles) == 3          # one single launch per sample


def test_the_native_entry_declines_host_rows_before_anything_is_stacked(multi, monkeypatch):
    """The library's own entry stays in place under the CPU stand-in, which covers the single launch only: log_marginal and
    posterior_predictive ask decoder.multi_declined first and go to the loop without forming a stacked argument."""
    ops._BACKEND['decoder_multi'] = decoder._launch_multi
    model = build('residual2_flows2')
    resp, mask = rows_of(model, B=10)
    assert decoder.multi_declined(resp) and decoder.multi_declined(ops.CellCodes(torch.zeros(4, 8, dtype=torch.uint8)))

    def stacked(*a, **k):
        raise AssertionError('stacked arguments formed for a call the backend declines')
    monkeypatch.setattr(type(model.decoder), '_args_multi', stacked)
    monkeypatch.setattr(model, '_decoder_multi_log_weights', stacked)
    torch.manual_seed(11)
    a = model.log_marginal(resp, mask, num_samples=3)
    data, args = _Rows(resp.unsqueeze(2), mask.unsqueeze(2), 4), types.SimpleNamespace(num_posterior_samples=3)
    assert tuple(vibo.posterior_predictive(model, data, args, 4, False)['response'].shape) == (1, 10, model.num_item, 1)
    without_multi()
    assert decoder.multi_declined(resp)
    torch.manual_seed(11)
    assert float(a) == float(model.log_marginal(resp, mask, num_samples=3))
    ops._BACKEND['decoder_multi'] = multi          # a stand-in that is not the library's entry is asked
    assert not decoder.multi_declined(resp)


class _Rows:
    """The slice of vibo.py's dataset that posterior_predictive reads."""

    def __init__(self, response, mask, step):
        self.response, self.mask, self.step = response, mask, step

    def batches(self, batch_size, shuffle=False):
        n = self.response.shape[0]
        return [torch.arange(s, min(n, s + self.step)) for s in range(0, n, self.step)]


def test_posterior_predictive_is_one_stacked_call_per_minibatch(multi):
    model = build('deep2')
    resp, mask = rows_of(model, B=10)
    data, args = _Rows(resp.unsqueeze(2), mask.unsqueeze(2), 4), types.SimpleNamespace(num_posterior_samples=5)
    S, I, H = 5, model.num_item, decoder.HIDDEN
    torch.manual_seed(3)
    a = vibo.posterior_predictive(model, data, args, 4, False)['response']
    state_multi = torch.get_rng_state()
    assert len(multi.calls) == 3 and all(c['prob_sum'] and not c['prob_accumulate'] for c in multi.calls)
    assert [tuple(c['V'].shape) for c in multi.calls] == [(S, 4, H), (S, 4, H), (S, 2, H)]
    assert all(tuple(c['U'].shape) == (S, I, H) for c in multi.calls)
    # not covered -> the loop, same draws; no entry -> the loop
    ops._BACKEND['decoder_multi'] = RecordingDecoderMulti(answer=False)
    torch.manual_seed(3)
    c = vibo.posterior_predictive(model, data, args, 4, False)['response']
    without_multi()
    torch.manual_seed(3)
    b = vibo.posterior_predictive(model, data, args, 4, False)['response']
    assert tuple(a.shape) == (1, 10, I, 1) and torch.allclose(a, b, rtol=0, atol=1e-6) and torch.equal(c, b)
    assert torch.equal(state_multi, torch.get_rng_state())


def test_sample_groups_split_the_call_and_continue_the_sum(multi, monkeypatch):
    """A bound that holds two samples: ceil(S / 2) calls in sample order, the predictive sum continued with prob_accumulate."""
    model = build('residual2_flows2')
    B, I, S = 6, model.num_item, 5
    g = torch.Generator().manual_seed(29)
    abilities, items = torch.randn(S, B, model.ability_dim, generator=g), torch.randn(S, I, model.item_feat_dim, generator=g)
    resp, mask = rows_of(model, B=B)
    with torch.no_grad():
        whole_ll, whole_sum = model.decoder.multi_log_lik(resp, mask, abilities, items), model.decoder.multi_prob_sum(abilities, items)
        assert len(multi.calls) == 2
        multi.calls.clear()
        monkeypatch.setattr(decoder, 'MULTI_STACK_BYTES', 2 * 4 * B * (decoder.HIDDEN + I))
        ll, total = model.decoder.multi_log_lik(resp, mask, abilities, items), model.decoder.multi_prob_sum(abilities, items)
    assert [c['V'].shape[0] for c in multi.calls] == [2, 2, 1, 2, 2, 1]
    assert [c['prob_accumulate'] for c in multi.calls[3:]] == [False, True, True]
    assert torch.allclose(ll, whole_ll, rtol=1e-6, atol=0) and torch.allclose(total, whole_sum, rtol=0, atol=1e-6)


def test_sample_groups_keep_the_stacked_inputs_under_the_bound():
    B, I = 100_000, 1000
    assert decoder.MULTI_STACK_BYTES == 1 << 30
    n = decoder.multi_sample_group(B, I, 16, True)
    assert 1 <= n < 16 and 4 * B * (decoder.HIDDEN + I) * n <= decoder.MULTI_STACK_BYTES < 4 * B * (decoder.HIDDEN + I) * (n + 1)
    assert decoder.multi_sample_group(B, I, 16, False) == 16 and decoder.multi_sample_group(16, 100, 400, True) == 400
    assert decoder.multi_sample_group(10 ** 7, 1000, 16, True) == 1


def test_the_second_headers_exports_are_typed_and_the_pinned_list_is_untouched():
    assert _lib.EXTRA_SYMBOLS == ('vibo_decoder_multi_person_chunks', 'vibo_decoder_multi_forward')
    assert not set(_lib.EXTRA_SYMBOLS) & set(_lib.EXPORTED_SYMBOLS) and _lib.ABI_VERSION == 2
    lib = _lib.load()
    chunks, fwd = lib.vibo_decoder_multi_person_chunks, lib.vibo_decoder_multi_forward
    assert chunks.restype is ctypes.c_int and chunks.argtypes == [ctypes.c_int] * 3
    assert fwd.restype is ctypes.c_int and len(fwd.argtypes) == 17
    assert fwd.argtypes[0] == ctypes.POINTER(_lib.ViboDecoderDesc) and fwd.argtypes[1] is ctypes.c_int
    assert fwd.argtypes[2:15] == [ctypes.c_void_p] * 13 and fwd.argtypes[15] is ctypes.c_int and fwd.argtypes[16] is ctypes.c_void_p
    assert decoder._launch_multi is ops._BACKEND['decoder_multi']


def test_the_chunks_query_counts_the_samples_in():
    q = _lib.load().vibo_decoder_multi_person_chunks
    assert q(0, 100, 4) == 0 and q(16, 0, 4) == 0 and q(16, 100, 0) == 0
    last = None
    for S in (1, 2, 8, 64, 400, 100_000):
        n = q(1000, 100, S)
        assert 1 <= n <= (1000 + 1) // 2 and (last is None or n <= last)
        last = n
    assert last == 1 and q(1000, 100, 1) > q(1000, 100, 64)
    assert q(7, 20, 1) == 4 and q(1, 20, 1) == 1          # at most one chunk per person pair


def test_the_argument_checks_answer_without_a_gpu():
    """Every refusal comes before any launch, with the error string set: none of these calls reaches the device."""
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    ok = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(ok.value + 4)

    def call(desc, S=3, V=ok, U=None, L=None, w1=None, ll=ok):
        d = None if desc is None else ctypes.byref(_lib.ViboDecoderDesc(*desc))
        rc = lib.vibo_decoder_multi_forward(d, S, ok, None, U, V, L, None, w1, ok, ok, ok, ok, ll, None, 0, None)
        return rc, lib.vibo_last_error_string().decode()

    good = (16, 100, 64, 0, 2, 0.0, 100, 0)          # B, I, hidden, want_grad, person_chunks, resid, strides
    assert call(None)[0] == -1
    assert call((0,) + good[1:])[0] == -2 and call((16, 0) + good[2:])[0] == -2 and call(good, S=0)[0] == -2
    rc, msg = call((16, 100, 32) + good[3:])
    assert rc == -6 and 'hidden_dim = 32' in msg
    assert call(good[:4] + (0,) + good[5:])[0] == -3 and call(good[:4] + (17,) + good[5:])[0] == -3
    assert call(good, V=None)[0] == -5 and call(good, ll=None)[0] == -5
    assert call(good, w1=ok)[0] == -5 and call(good[:5] + (1.0,) + good[6:])[0] == -5          # w1 / resid without L
    rc, msg = call(good[:3] + (1,) + good[4:])
    assert rc == -5 and 'want_grad' in msg
    assert call(good, V=odd)[0] == -4 and call(good, U=odd)[0] == -4
