"""The multi-sample forward of the per-term MLP decoders (vibo_decoder_multi_forward, csrc/vibo_decoder_multi.hip): every record
against the single launch's bit for bit, samples that do not leak into each other, prob_sum against the accumulate over single
launches, the per-sample sums against float64, log_marginal / posterior_predictive through it against the loop they replace, the
launches they make, and the refusals."""
import copy
import ctypes
import math
import types

import pytest
import torch
import torch.nn.functional as F

from gpu_common import dev, record, torch_reference
from vibo_amd import _lib, decoder as D, ops
from vibo_amd.torch_core import models as M, vibo

pytestmark = pytest.mark.gpu

H = D.HIDDEN
SHAPES = [(7, 20, 3), (33, 95, 5), (37, 130, 4), (16, 100, 9)]          # (B, I, S): odd B (a half-empty last pair), I off the 16- and
MODES = ['deep', 'link', 'residual', 'link3', 'residual3']               # 64-item grids; so few samples that every workgroup takes
                                                                         # one, or with prob_sum all of them (several, unevenly: GROUPED)


def problem(mode, B, I, S, missing, hidden=H, seed=0):
    """Device tensors of one stacked call, drawn on the host from one generator (test_gpu_decoder.py's scales)."""
    g = torch.Generator().manual_seed(1000 * B + I + 7 * S + seed)
    d = dev()
    rn = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to(d)
    resp = (torch.rand(B, I, generator=g) < 0.5).float().to(d)
    mask = (torch.rand(B, I, generator=g) >= missing).to(torch.uint8).to(d) if missing > 0 else None
    link, has_l = mode.startswith('link'), mode != 'deep'
    return dict(resp=resp, mask=mask, U=None if link else rn(S, I, hidden, sc=0.7), V=rn(S, B, hidden, sc=0.7),
                L=rn(S, B, I, sc=1.5) if has_l else None, guess=torch.sigmoid(rn(S, I)) if mode.endswith('3') else None,
                w1=rn(hidden, sc=0.5) if link else None, W2=rn(hidden, hidden, sc=0.18), b2=rn(hidden, sc=0.1), w3=rn(hidden, sc=0.25),
                b3=rn(1, sc=0.1), resid=1.0 if mode.startswith('residual') else 0.0)


def at(t, s):
    return None if t is None else t[s]


def single(pr, s, chunks, want_prob=False):
    """vibo_decoder_fwd_bwd (want_grad = 0) on sample s alone with `chunks` person chunks -> (ll_part [n_wave], prob [B, I] or None)."""
    B, I = pr['resp'].shape
    d = _lib.ViboDecoderDesc(B, I, H, 0, chunks, pr['resid'], pr['resp'].stride(0), pr['mask'].stride(0) if pr['mask'] is not None else 0)
    ll = torch.full((4 * ((I + 63) // 64) * chunks,), float('nan'), device=dev())
    prob = torch.full((B, I), float('nan'), device=dev()) if want_prob else None
    p = ops._ptr
    ops._call('vibo_decoder_fwd_bwd', ctypes.byref(d), p(pr['resp']), p(pr['mask']), p(at(pr['U'], s)), p(pr['V'][s]), p(at(pr['L'], s)),
              p(at(pr['guess'], s)), p(pr['w1']), p(pr['W2']), p(pr['b2']), p(pr['w3']), p(pr['b3']), p(ll), p(None), p(None), p(None),
              p(None), p(None), p(None), p(prob), ops._stream(dev()))
    return ll, prob


def multi(pr, chunks=None, prob_sum=None, accumulate=False, samples=slice(None)):
    sl = lambda t: None if t is None else t[samples].contiguous()
    return D._launch_multi(pr['resp'], pr['mask'], sl(pr['U']), sl(pr['V']), sl(pr['L']), sl(pr['guess']), pr['w1'], pr['W2'], pr['b2'],
                           pr['w3'], pr['b3'], pr['resid'], prob_sum=prob_sum, prob_accumulate=accumulate, person_chunks=chunks)


# ---------------------------------------------------------------------------
# records bit for bit
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('B,I,S', SHAPES)
@pytest.mark.parametrize('mode', MODES)
def test_every_record_is_the_single_launchs_bit_for_bit(mode, B, I, S):
    for missing in (0.0, 0.3):
        pr = problem(mode, B, I, S, missing)
        for chunks in (1, 3):
            got = multi(pr, chunks)['ll_part']
            assert tuple(got.shape) == (S, 4 * ((I + 63) // 64) * chunks)
            for s in range(S):
                want = single(pr, s, chunks)[0]
                assert torch.equal(got[s], want), (mode, B, I, s, chunks, missing, float((got[s] - want).abs().max()))
            # with prob_sum the call runs ONE sample group: every workgroup takes all S samples in turn, the same records
            cells = torch.empty(B, I, device=dev())
            assert torch.equal(multi(pr, chunks, prob_sum=cells)['ll_part'], got), (mode, B, I, chunks, missing)


def samples_per_group(I, S, chunks):
    """The samples a workgroup takes in a call without prob_sum, as vibo_decoder_multi_forward derives them on this device."""
    cells = ((I + 63) // 64) * chunks
    groups = max(1, min(S, (2 * torch.cuda.get_device_properties(dev()).multi_processor_count + cells - 1) // cells))
    return (S + groups - 1) // groups


# more samples than sample groups, the last group short: a workgroup's sample loop runs several times (the sum zeroed per sample, the
# row s of the records, the prefetch that wraps to the next sample's first pair); (7, 20) at 3 person chunks has a chunk past the last
# person (4 persons per chunk: the third begins at 8), whose records are zeros for every sample of the group
GROUPED = [('residual3', 7, 20, 603, 3), ('deep', 37, 130, 203, 3), ('link', 16, 100, 403, 1), ('link3', 33, 95, 1031, 3)]


@pytest.mark.parametrize('mode,B,I,S,chunks', GROUPED)
def test_every_record_of_a_workgroup_with_several_samples_bit_for_bit(mode, B, I, S, chunks):
    spg = samples_per_group(I, S, chunks)
    assert spg >= 2 and S % spg != 0, (spg, 'the case no longer reaches the regime it is here for')
    for missing in (0.0, 0.3):
        pr = problem(mode, B, I, S, missing)
        got = multi(pr, chunks)['ll_part']
        want = torch.stack([single(pr, s, chunks)[0] for s in range(S)])
        bad = (got != want).any(1).nonzero().flatten().tolist()
        assert not bad, (mode, B, I, chunks, missing, spg, bad[:8])
        if (B, chunks) == (7, 3):
            assert bool((got.view(S, chunks, -1)[:, 2] == 0).all()) and bool((got.view(S, chunks, -1)[:, :2] != 0).any())


def test_hidden_32_goes_through_the_padding_bit_for_bit():
    B, I, S = 33, 95, 5
    pr = problem('link3', B, I, S, 0.3, hidden=32)
    padded = dict(pr)
    padded['U'], padded['V'], padded['W2'], padded['b2'], padded['w3'], padded['w1'] = D._pad_hidden(
        pr['U'], pr['V'], pr['W2'], pr['b2'], pr['w3'], pr['w1'])
    padded = {k: (v.contiguous() if torch.is_tensor(v) else v) for k, v in padded.items()}
    assert tuple(padded['V'].shape) == (S, B, H) and tuple(padded['W2'].shape) == (H, H)
    got = multi(padded, 3)['ll_part']
    for s in range(S):
        assert torch.equal(got[s], single(padded, s, 3)[0])
    # ... and through the public call: the sums of decoder_log_lik per sample, to the summation order of the records
    ll = D.decoder_multi_log_lik(pr['resp'], pr['mask'], U=pr['U'], V=pr['V'], W2=pr['W2'], b2=pr['b2'], w3=pr['w3'], b3=pr['b3'],
                                 logit=pr['L'], w1=pr['w1'], guess=pr['guess'], resid=pr['resid'])
    for s in range(S):
        one = D.decoder_log_lik(pr['resp'], pr['mask'], U=None, V=pr['V'][s], W2=pr['W2'], b2=pr['b2'], w3=pr['w3'], b3=pr['b3'],
                                logit=pr['L'][s], w1=pr['w1'], guess=pr['guess'][s], resid=pr['resid'])
        assert abs(float(ll[s]) - float(one)) <= 2e-6 * abs(float(one))


# ---------------------------------------------------------------------------
# samples do not leak
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('mode,B,I,S', [('residual3', 37, 130, 4), ('deep', 16, 100, 9),
                                        # ... and where a workgroup takes several samples, the last group short (see GROUPED)
                                        ('residual3', 7, 20, 603), ('deep', 16, 100, 403)])
def test_samples_do_not_leak(mode, B, I, S):
    if S > 100:
        spg = samples_per_group(I, S, 3)
        assert spg >= 2 and S % spg != 0, spg
    pr = problem(mode, B, I, S, 0.3)
    base = multi(pr, 3)['ll_part']
    rev = {k: (v.flip(0).contiguous() if k in ('U', 'V', 'L', 'guess') and v is not None else v) for k, v in pr.items()}
    assert torch.equal(multi(rev, 3)['ll_part'], base.flip(0))
    for name, k in (('U', 1), ('V', S - 2)):
        changed = dict(pr)
        changed[name] = pr[name].clone()
        changed[name][k] += 0.25
        got = multi(changed, 3)['ll_part']
        others = [s for s in range(S) if s != k]
        assert torch.equal(got[others], base[others]) and not torch.equal(got[k], base[k])


# ---------------------------------------------------------------------------
# prob_sum
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('mode,B,I,S', [('link3', 7, 20, 3), ('deep', 37, 130, 4)])
def test_prob_sum_is_the_accumulate_over_single_launches(mode, B, I, S):
    pr = problem(mode, B, I, S, 0.0)
    kw = lambda s: dict(U=at(pr['U'], s), V=pr['V'][s], W2=pr['W2'], b2=pr['b2'], w3=pr['w3'], b3=pr['b3'], logit=at(pr['L'], s),
                        w1=pr['w1'], guess=at(pr['guess'], s), resid=pr['resid'])
    want = D.decoder_probs(B, I, **kw(0)).clone()
    for s in range(1, S):
        want += D.decoder_probs(B, I, **kw(s))
    got = D.decoder_multi_prob_sum(B, I, U=pr['U'], V=pr['V'], W2=pr['W2'], b2=pr['b2'], w3=pr['w3'], b3=pr['b3'], logit=pr['L'],
                                   w1=pr['w1'], guess=pr['guess'], resid=pr['resid'])
    assert torch.equal(got, want)
    # a poisoned, padded buffer, the sum split across two calls: the same bits, nothing outside B x I touched
    pad, poison = 64, -12345.0
    for chunks in (1, 3):
        flat = torch.full((B * I + 2 * pad,), poison, device=dev())
        cells = flat[pad:pad + B * I].view(B, I)
        assert multi(pr, chunks, prob_sum=cells, samples=slice(0, 1)) is not None
        assert multi(pr, chunks, prob_sum=cells, accumulate=True, samples=slice(1, S)) is not None
        assert torch.equal(cells, want), chunks
        assert bool((flat[:pad] == poison).all()) and bool((flat[pad + B * I:] == poison).all())
        whole = torch.full((B, I), poison, device=dev())
        multi(pr, chunks, prob_sum=whole)
        assert torch.equal(whole, want)


# ---------------------------------------------------------------------------
# heads against float64
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('mode,B,I,S,missing', [('deep', 37, 130, 4, 0.3), ('link3', 33, 95, 5, 0.3), ('residual', 16, 100, 9, 0.0)])
def test_per_sample_sums_match_float64(mode, B, I, S, missing):
    pr = problem(mode, B, I, S, missing)
    ll = D.decoder_multi_log_lik(pr['resp'], pr['mask'], U=pr['U'], V=pr['V'], W2=pr['W2'], b2=pr['b2'], w3=pr['w3'], b3=pr['b3'],
                                 logit=pr['L'], w1=pr['w1'], guess=pr['guess'], resid=pr['resid'])
    assert tuple(ll.shape) == (S,)
    c = {k: (v.double().cpu() if torch.is_tensor(v) else v) for k, v in pr.items()}
    for s in range(S):
        ref, _ = torch_reference(c['resp'], c['mask'], at(c['U'], s), c['V'][s], c['W2'], c['b2'], c['w3'], c['b3'], at(c['L'], s),
                                 c['w1'], at(c['guess'], s), c['resid'])
        assert abs(float(ll[s]) - float(ref)) < 2e-5 * abs(float(ref)), (s, float(ll[s]), float(ref))


# ---------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------
MODELS = {
    'deep 2PL': lambda: M.VIBO_2PL(2, 100, ability_merge='product', generative_model='deep'),
    'link 3PL': lambda: M.VIBO_3PL(2, 100, ability_merge='product', generative_model='link'),
    'residual 2PL, 2 flows': lambda: M.VIBO_2PL(2, 100, ability_merge='product', generative_model='residual', n_norm_flows=2),
    'deep 2PL, conditional posterior': lambda: M.VIBO_2PL(2, 100, ability_merge='product', generative_model='deep', conditional_posterior=True),
    'deep 2PL, mean merge': lambda: M.VIBO_2PL(2, 100, ability_merge='mean', generative_model='deep'),
}


def model_problem(kind, B=16, S=5):
    torch.manual_seed(17)
    model = MODELS[kind]().to(dev())
    g = torch.Generator().manual_seed(19)
    I = model.num_item
    resp, mask = (torch.rand(B, I, generator=g) < 0.5).float(), torch.rand(B, I, generator=g) < 0.8
    eps_item, eps_ab = torch.randn(S, I, model.item_feat_dim, generator=g), torch.randn(S, B, model.ability_dim, generator=g)
    return model, resp.to(dev()), mask.to(dev()), eps_item.to(dev()), eps_ab.to(dev())


def log_marginal_float64(model, resp, mask, eps_item, eps_ab):
    """log_marginal of an MLP-decoder model stated in float64 on the host, sample by sample: the posterior from the dense rows, the
    flows one by one, the decoder through gpu_common.torch_reference, _decoder_elbo(ctx, 1.0, False)'s terms."""
    m = copy.deepcopy(model).double().cpu()
    r, k = resp.double().cpu(), mask.double().cpu()
    A, I = m.ability_dim, m.num_item
    item_mu, item_lv = m.item_encoder()
    n1, nobs = (r * k).sum(1, keepdim=True), k.sum(1, keepdim=True)
    log_w = []
    for s in range(eps_item.shape[0]):
        item_feat = eps_item[s].double().cpu() * torch.exp(0.5 * item_lv) + item_mu
        enc = m.ability_encoder
        if m.ability_merge == 'mean':
            assert not m.conditional_posterior
            h = F.elu(enc.mlp1(enc._response_values.double()))
            hid = (n1 * h[1] + (nobs - n1) * h[0]) / nobs                      # the mean of the observed cells' features
            amu, alv = torch.chunk(enc.mlp2(hid), 2, dim=1)
        else:
            table = enc.expert_table(item_feat if m.conditional_posterior else None)      # [2, (I,) 2A]
            if not m.conditional_posterior:
                table = table.unsqueeze(1).expand(2, I, 2 * A)
            sel = table[(r == 1).long(), torch.arange(I)]                      # [B, I, 2A]
            tau = k.unsqueeze(2) / (torch.exp(sel[..., A:]) + 1e-8)
            lam = tau.sum(1) + ((I - nobs) * (1.0 / (1.0 + 1e-8)) if m.replace_missing_with_prior else 0.0)
            amu, alv = (sel[..., :A] * tau).sum(1) / lam, torch.log(1.0 / lam)
        ability = eps_ab[s].double().cpu() * torch.exp(0.5 * alv) + amu
        ability_k, item_k, ladj_a, ladj_i = ability, item_feat, 0.0, 0.0
        if m.n_norm_flows > 0:
            for f in m.ability_norm_flows.flows:
                ability_k, l = f(ability_k)
                ladj_a = ladj_a + l.sum()
            for f in m.item_norm_flows.flows:
                item_k, l = f(item_k)
                ladj_i = ladj_i + l.sum()
        a = m.decoder._args(ability_k, item_k)
        ll, _ = torch_reference(r, k, a['U'], a['V'], a['W2'], a['b2'], a['w3'], a['b3'], a.get('logit'), a.get('w1'), a.get('guess'),
                                a.get('resid', 0.0))
        log_q = (M._normal_logpdf(ability, amu, alv).sum() - ladj_a) + (M._normal_logpdf(item_feat, item_mu, item_lv).sum() - ladj_i)
        log_p = ll + M._std_normal_logpdf(ability_k).sum() + M._std_normal_logpdf(item_k).sum()
        log_w.append(log_p - log_q)
    log_w = torch.stack(log_w)
    return float(torch.logsumexp(log_w, 0) - math.log(log_w.shape[0]))


def test_log_marginal_agrees_with_the_loop_it_replaces(monkeypatch):
    """Both paths against float64 on B = 16, I = 100, S = 5 with fixed noise; the stacked path may deviate at most twice as far as the
    loop does (two independently rounded fp32 evaluations).  Measured on an MI355X (profiles/r11_decoder_multi_tolerance.txt)."""
    worst = {'multi': 0.0, 'loop': 0.0}
    with torch.no_grad():
        for kind in MODELS:
            model, resp, mask, eps_item, eps_ab = model_problem(kind)
            ref = log_marginal_float64(model, resp, mask, eps_item, eps_ab)
            seen = []
            real = ops._BACKEND['decoder_multi']
            monkeypatch.setitem(ops._BACKEND, 'decoder_multi', lambda *a, **k: seen.append(1) or real(*a, **k))
            new = float(model.log_marginal(resp, mask, num_samples=5, eps_item=eps_item, eps_ability=eps_ab))
            monkeypatch.delitem(ops._BACKEND, 'decoder_multi')
            loop = float(model.log_marginal(resp, mask, num_samples=5, eps_item=eps_item, eps_ability=eps_ab))
            monkeypatch.undo()
            assert seen == [1] and ops._BACKEND['decoder_multi'] is real
            dev_new, dev_loop = abs(new - ref) / abs(ref), abs(loop - ref) / abs(ref)
            print(f'{kind}: float64 {ref:.9f}  stacked {new:.9f} ({dev_new:.3e})  loop {loop:.9f} ({dev_loop:.3e})')
            record('decoder_multi log_marginal, stacked', dev_new, model=kind)
            record('decoder_multi log_marginal, loop', dev_loop, model=kind)
            worst['multi'], worst['loop'] = max(worst['multi'], dev_new), max(worst['loop'], dev_loop)
    print(f'worst relative deviation from float64: stacked {worst["multi"]:.3e}, loop {worst["loop"]:.3e}')
    assert worst['loop'] < 2e-5          # (the loop itself is sane: test_gpu_decoder.py's bound on a decoder sum)
    assert worst['multi'] <= 2.0 * worst['loop'], worst


@pytest.mark.parametrize('kind', ['deep 2PL', 'residual 2PL, 2 flows', 'deep 2PL, conditional posterior'])
def test_unseeded_noise_leaves_the_generators_where_the_loop_leaves_them(kind, monkeypatch):
    model, resp, mask, _, _ = model_problem(kind)
    states = []
    for path in ('multi', 'loop'):
        if path == 'loop':
            monkeypatch.delitem(ops._BACKEND, 'decoder_multi')
        torch.manual_seed(5)
        value = float(model.log_marginal(resp, mask, num_samples=5))
        states.append((value, torch.cuda.get_rng_state(dev()), torch.get_rng_state()))
    (a, dev_a, cpu_a), (b, dev_b, cpu_b) = states
    assert torch.equal(dev_a, dev_b) and torch.equal(cpu_a, cpu_b)
    assert abs(a - b) < 1e-5 * abs(b)          # ... and the same noise was drawn: the same number


# ---------------------------------------------------------------------------
# launch counts
# ---------------------------------------------------------------------------
def counting(monkeypatch, *names):
    n = {}
    for name in names:
        real = ops._BACKEND[name]
        n[name] = 0

        def counted(*a, _real=real, _name=name, **k):
            n[_name] += 1
            return _real(*a, **k)
        monkeypatch.setitem(ops._BACKEND, name, counted)
    return n


def test_log_marginal_is_one_decoder_launch_and_one_row_count(monkeypatch):
    model, resp, mask, eps_item, eps_ab = model_problem('deep 2PL')
    n = counting(monkeypatch, 'decoder_multi', 'decoder', 'counts')
    value = model.log_marginal(resp, mask, num_samples=5, eps_item=eps_item, eps_ability=eps_ab)
    assert torch.isfinite(value) and n == {'decoder_multi': 1, 'decoder': 0, 'counts': 1}


class _Rows:
    """The slice of vibo.py's dataset that posterior_predictive reads."""

    def __init__(self, response, mask, step):
        self.response, self.mask, self.step = response, mask, step

    def batches(self, batch_size, shuffle=False):
        n = self.response.shape[0]
        return [torch.arange(s, min(n, s + self.step), device=self.response.device) for s in range(0, n, self.step)]


def test_posterior_predictive_equals_the_loop_with_one_launch_per_minibatch(monkeypatch):
    torch.manual_seed(17)
    model = MODELS['deep 2PL']().to(dev())
    g = torch.Generator().manual_seed(23)
    resp, mask = (torch.rand(24, 100, generator=g) < 0.5).float().to(dev()), (torch.rand(24, 100, generator=g) < 0.8).to(dev())
    data, args = _Rows(resp.unsqueeze(2), mask.unsqueeze(2), 16), types.SimpleNamespace(num_posterior_samples=5)
    n = counting(monkeypatch, 'decoder_multi', 'decoder')
    torch.manual_seed(3)
    new = vibo.posterior_predictive(model, data, args, 16, False)['response']
    assert n == {'decoder_multi': 2, 'decoder': 0}
    monkeypatch.delitem(ops._BACKEND, 'decoder_multi')
    torch.manual_seed(3)
    loop = vibo.posterior_predictive(model, data, args, 16, False)['response']
    assert n['decoder'] == 2 * 5 and tuple(new.shape) == (1, 24, 100, 1)
    assert torch.equal(new, loop), float((new - loop).abs().max())


def test_sample_groups_give_the_same_sums(monkeypatch):
    """decoder.MULTI_STACK_BYTES holding two samples: three launches instead of one; the predictive sum, continued across them with
    prob_accumulate, keeps its bits, the log-likelihoods their value (the records' summation order follows the person chunks)."""
    torch.manual_seed(17)
    model = MODELS['residual 2PL, 2 flows']().to(dev())
    B, I, S = 16, model.num_item, 5
    g = torch.Generator().manual_seed(29)
    abilities, items = torch.randn(S, B, 2, generator=g).to(dev()), torch.randn(S, I, 3, generator=g).to(dev())
    resp, mask = (torch.rand(B, I, generator=g) < 0.5).float().to(dev()), (torch.rand(B, I, generator=g) < 0.8).to(dev())
    with torch.no_grad():
        whole_ll, whole_sum = model.decoder.multi_log_lik(resp, mask, abilities, items), model.decoder.multi_prob_sum(abilities, items)
        n = counting(monkeypatch, 'decoder_multi')
        monkeypatch.setattr(D, 'MULTI_STACK_BYTES', 2 * 4 * B * (H + I))
        ll, total = model.decoder.multi_log_lik(resp, mask, abilities, items), model.decoder.multi_prob_sum(abilities, items)
    assert n == {'decoder_multi': 6} and torch.equal(total, whole_sum)
    assert float(((ll - whole_ll) / whole_ll).abs().max()) <= 2e-6


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------
def test_every_refusal_leaves_the_outputs_untouched():
    B, I, S = 16, 100, 3
    pr = problem('residual3', B, I, S, 0.3)
    lib, p, poison = _lib.load(), ops._ptr, -12345.0
    ll = torch.full((S, 4 * 2 * 2), poison, device=dev())
    cells = torch.full((B, I), poison, device=dev())
    odd = lambda t: ctypes.c_void_p(t.data_ptr() + 4)

    def call(desc, num_samples=S, **over):
        a = dict(resp=p(pr['resp']), mask=p(pr['mask']), U=p(pr['U']), V=p(pr['V']), L=p(pr['L']), guess=p(pr['guess']), w1=p(None),
                 W2=p(pr['W2']), b2=p(pr['b2']), w3=p(pr['w3']), b3=p(pr['b3']), ll=p(ll))
        a.update(over)
        d = None if desc is None else ctypes.byref(_lib.ViboDecoderDesc(*desc))
        rc = lib.vibo_decoder_multi_forward(d, num_samples, a['resp'], a['mask'], a['U'], a['V'], a['L'], a['guess'], a['w1'], a['W2'],
                                            a['b2'], a['w3'], a['b3'], a['ll'], p(cells), 0, ops._stream(dev()))
        torch.cuda.synchronize()
        assert bool((ll == poison).all()) and bool((cells == poison).all()), (desc, over)
        return rc, lib.vibo_last_error_string().decode()

    good = (B, I, H, 0, 2, 1.0, I, I)          # B, I, hidden, want_grad, person_chunks, resid, strides
    assert call(None)[0] == -1
    assert call((0,) + good[1:])[0] == -2 and call((B, 0) + good[2:])[0] == -2 and call(good, num_samples=0)[0] == -2
    rc, msg = call((B, I, 32) + good[3:])
    assert rc == -6 and 'hidden_dim = 32' in msg
    assert call(good[:4] + (0,) + good[5:])[0] == -3 and call(good[:4] + (B + 1,) + good[5:])[0] == -3
    assert call(good, V=p(None))[0] == -5 and call(good, resp=p(None))[0] == -5 and call(good, ll=p(None))[0] == -5
    assert call(good, L=p(None))[0] == -5                                      # resid without the logits
    assert call(good[:5] + (0.0,) + good[6:], L=p(None), w1=p(pr['b2']))[0] == -5      # w1 without the logits
    rc, msg = call(good[:3] + (1,) + good[4:])
    assert rc == -5 and 'want_grad' in msg
    assert call(good, V=odd(pr['V']))[0] == -4 and call(good, U=odd(pr['U']))[0] == -4
    # ... and the call they all refused goes through as it stands
    rc = lib.vibo_decoder_multi_forward(ctypes.byref(_lib.ViboDecoderDesc(*good)), S, p(pr['resp']), p(pr['mask']), p(pr['U']), p(pr['V']),
                                        p(pr['L']), p(pr['guess']), p(None), p(pr['W2']), p(pr['b2']), p(pr['w3']), p(pr['b3']), p(ll),
                                        p(cells), 0, ops._stream(dev()))
    torch.cuda.synchronize()
    assert rc == 0 and not bool((ll == poison).any()) and not bool((cells == poison).any())
