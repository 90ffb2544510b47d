"""The per-term MLP decoders of --generative-model link | deep | residual (reference models.py:769-919) on the HIP
library's matrix-pipe kernel (csrc/vibo_decoder.hip, vibo_decoder_fwd_bwd).

All three decoders end in the same per-(person, item) network 64 -> ELU -> [64 x 64] -> ELU -> 64 -> 1.  The first
layer's input is a concatenation / a scalar, so it splits exactly into a per-item half U [I, 64], a per-person half
V [B, 64] and (link) a rank-one term w1 * logit; those halves -- a few small dense layers over I or B rows -- are
ordinary PyTorch modules here, and `decoder_log_lik` is the O(B I 64^2) rest: forward, masked Bernoulli log-likelihood
and the whole backward in one launch, returned to autograd as gradients of (U, V, logit, guess, w1, W2, b2, w3, b3).
Forward only, for S stacked samples in one launch (log_marginal, posterior_predictive): `decoder_multi_log_lik` /
`decoder_multi_prob_sum` on csrc/vibo_decoder_multi.hip (vibo_decoder_multi_forward).
"""
import ctypes

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, ops

HIDDEN = 64


def _launch(response, mask, U, V, L, guess, w1, W2, b2, w3, b3, resid, want_grad, want_prob=False):
    lib = _lib.load()
    for t in (response, V, W2, b2, w3, b3):
        if t.device.type != 'cuda':
            raise _lib.ViboLibraryError('decoder_log_lik: device tensors only (no CPU fallback)')
    B, I = response.shape
    dev = response.device
    chunks = lib.vibo_decoder_person_chunks(B, I)
    n_ib = (I + 63) // 64
    n_wave = 4 * n_ib * chunks
    d = _lib.ViboDecoderDesc(B, I, HIDDEN, int(want_grad), chunks, float(resid), response.stride(0),
                             mask.stride(0) if mask is not None else 0)
    f32 = dict(dtype=torch.float32, device=dev)
    out = {'ll_part': torch.empty(n_wave, **f32)}
    if want_grad:
        out['dW2'] = torch.empty(n_wave, HIDDEN, HIDDEN, **f32)
        out['dvec'] = torch.empty(n_wave, 4, HIDDEN, **f32)
        out['dV'] = torch.empty(4 * n_ib, B, HIDDEN, **f32)
        if U is not None:
            out['dU'] = torch.empty(chunks, I, HIDDEN, **f32)
        if L is not None:
            out['dL'] = torch.empty(B, I, **f32)
        if guess is not None:
            out['dguess'] = torch.empty(chunks, I, **f32)
    if want_prob:
        out['prob'] = torch.empty(B, I, **f32)
    p = ops._ptr
    ops._call('vibo_decoder_fwd_bwd', ctypes.byref(d), p(response), p(mask), p(U), p(V), p(L), p(guess), p(w1), p(W2), p(b2), p(w3),
              p(b3), p(out['ll_part']), p(out.get('dU')), p(out.get('dV')), p(out.get('dL')),
              p(out.get('dguess')), p(out.get('dW2')), p(out.get('dvec')), p(out.get('prob')), ops._stream(dev))
    return out


ops._BACKEND.setdefault('decoder', _launch)      # (tests without a GPU swap in oracle/cpu_backend.py's stand-in)


def _launch_multi(response, mask, U, V, L, guess, w1, W2, b2, w3, b3, resid, prob_sum=None, prob_accumulate=False, person_chunks=None):
    """vibo_decoder_multi_forward: the forward of `_launch` for S stacked samples in one launch -- U [S, I, 64] or None,
    V [S, B, 64], L [S, B, I] or None, guess [S, I] or None, the rest shared.  -> {'ll_part': [S, n_wave]} (sum over dim 1 per sample;
    row s holds the bits of `_launch`'s ll_part for sample s alone at the same person_chunks); prob_sum [B, I]: the samples'
    P(response = 1) are summed into it in sample order (prob_accumulate: onto what it holds).
    None -- "not covered", the caller then makes one `_launch` per sample -- for tensors that are not on the device: this entry
    stays in place under the CPU stand-in of the tests, which covers the single launch only."""
    if any(t.device.type != 'cuda' for t in (response, V, W2, b2, w3, b3)):
        return None
    lib = _lib.load()
    S, B = V.shape[0], V.shape[1]
    I = response.shape[1]
    dev = response.device
    if person_chunks is None:      # (prob_sum: one workgroup owns a cell for all samples, so the samples add no parallelism)
        person_chunks = lib.vibo_decoder_person_chunks(B, I) if prob_sum is not None else lib.vibo_decoder_multi_person_chunks(B, I, S)
    n_wave = 4 * ((I + 63) // 64) * person_chunks
    d = _lib.ViboDecoderDesc(B, I, HIDDEN, 0, person_chunks, float(resid), response.stride(0), mask.stride(0) if mask is not None else 0)
    out = {'ll_part': torch.empty(S, n_wave, dtype=torch.float32, device=dev)}
    p = ops._ptr
    ops._call('vibo_decoder_multi_forward', ctypes.byref(d), S, p(response), p(mask), p(U), p(V), p(L), p(guess), p(w1), p(W2), p(b2),
              p(w3), p(b3), p(out['ll_part']), p(prob_sum), int(bool(prob_accumulate)), ops._stream(dev))
    return out


ops._BACKEND.setdefault('decoder_multi', _launch_multi)


def multi_declined(rows):
    """True where the multi-sample launch will not take a call on `rows` (a tensor or CellCodes), asked before anything is drawn or
    stacked (as ops.multi_forward_declined): no backend entry, or the native entry with rows that are not on the device."""
    backend = ops._BACKEND.get('decoder_multi')
    return backend is None or (backend is _launch_multi and rows.device.type != 'cuda')


def _prep(t):
    return None if t is None else t.detach().contiguous().float()


PERSON_CHUNK = 65536      # persons per launch: bounds the per-wave d V records ([4 ceil(I / 64)][persons][64] floats) to ~1 GB at 1 000 items


class _DecoderLogLik(torch.autograd.Function):
    """sum of the masked Bernoulli log-likelihood; every gradient is produced by the forward launch(es) -- the persons go
    through in chunks of PERSON_CHUNK, the per-chunk partial records are summed here (fixed order)."""

    @staticmethod
    def forward(ctx, response, mask, resid, want_grad, U, V, L, guess, w1, W2, b2, w3, b3):
        # (want_grad is decided by the caller: inside Function.forward grad mode is off and nn.Parameters always say
        #  requires_grad -- under no_grad (test epochs, log_marginal's hundreds of samples) the GRAD kernel variant and its
        #  ~1 GB of d V records per 65 536 persons were produced for nothing)
        Up, Vp, Lp, gp, w1p, W2p, b2p, w3p, b3p = (_prep(t) for t in (U, V, L, guess, w1, W2, b2, w3, b3))
        B = response.shape[0]
        ll = None
        acc = {}
        for s in range(0, B, PERSON_CHUNK):
            e = min(B, s + PERSON_CHUNK)
            whole = s == 0 and e == B
            out = ops._BACKEND['decoder'](response if whole else response[s:e], mask if (mask is None or whole) else mask[s:e], Up,
                                          Vp if whole else Vp[s:e], Lp if (Lp is None or whole) else Lp[s:e], gp, w1p, W2p, b2p, w3p, b3p,
                                          resid, want_grad)
            part = out['ll_part'].sum()
            ll = part if ll is None else ll + part
            if want_grad:
                red = {'dW2': out['dW2'].sum(0), 'dvec': out['dvec'].sum(0)}
                if 'dU' in out:
                    red['dU'] = out['dU'].sum(0)
                if 'dguess' in out:
                    red['dguess'] = out['dguess'].sum(0)
                for k, v in red.items():
                    acc[k] = v if k not in acc else acc[k] + v
                acc.setdefault('dV', []).append(out['dV'].sum(0))
                if 'dL' in out:
                    acc.setdefault('dL', []).append(out['dL'])
        if want_grad:
            acc['dV'] = acc['dV'][0] if len(acc['dV']) == 1 else torch.cat(acc['dV'], 0)
            if 'dL' in acc:
                acc['dL'] = acc['dL'][0] if len(acc['dL']) == 1 else torch.cat(acc['dL'], 0)
        ctx.out = acc if want_grad else None
        ctx.has = (U is not None, L is not None, guess is not None, w1 is not None)
        return ll

    @staticmethod
    def backward(ctx, g):
        o = ctx.out
        has_u, has_l, has_g, has_w1 = ctx.has
        dvec = o['dvec']
        return (None, None, None, None,
                g * o['dU'] if has_u else None,
                g * o['dV'],
                g * o['dL'] if has_l else None,
                g * o['dguess'] if has_g else None,
                g * dvec[2] if has_w1 else None,
                g * o['dW2'], g * dvec[0], g * dvec[1], g * dvec[3, :1])


def _rows(response, mask):
    if isinstance(response, ops.CellCodes):
        response, mask = response.unpack()
    response = ops.prepare_response(response)
    if mask is not None:
        mask = ops.prepare_mask(mask)[0]
    return response.float(), mask


def _pad_hidden(U, V, W2, b2, w3, w1):
    """The kernel's per-term network is 64 units wide.  A narrower one (--hidden-dim < 64) is the same network with its extra
    units switched off: zero rows / columns give z1 = 0 -> elu(0) = 0 -> no contribution to the second layer, whose padded
    units see a zero bias and a zero output weight -- exact, and autograd slices the padding off the gradients again."""
    H = W2.shape[0]
    if H == HIDDEN:
        return U, V, W2, b2, w3, w1
    if H > HIDDEN:
        raise NotImplementedError(f'hidden_dim = {H}: the per-term decoder kernel covers hidden widths up to {HIDDEN} '
                                  '(its 64 x 64 weight-gradient tile lives in registers)')
    k = HIDDEN - H
    pad1 = lambda t: None if t is None else F.pad(t, (0, k))
    return pad1(U), pad1(V), F.pad(W2, (0, k, 0, k)), pad1(b2), pad1(w3), pad1(w1)


def decoder_log_lik(response, mask, *, U, V, W2, b2, w3, b3, logit=None, w1=None, guess=None, resid=0.0):
    """sum_{p,i} mask * log Bernoulli(response | P) of the per-term network (see the module docstring); differentiable in
    every tensor argument but response / mask.  response [B, I(, 1)] fp32, mask [B, I(, 1)] bool/u8 or None."""
    response, mask = _rows(response, mask)
    U, V, W2, b2, w3, w1 = _pad_hidden(U, V, W2, b2, w3, w1)
    want_grad = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (U, V, logit, guess, w1, W2, b2, w3, b3))
    return _DecoderLogLik.apply(response, mask, float(resid), want_grad, U, V, logit, guess, w1, W2, b2, w3, b3)


@torch.no_grad()
def decoder_probs(B, I, *, U, V, W2, b2, w3, b3, logit=None, w1=None, guess=None, resid=0.0):
    """P(response = 1) [B, I] of the per-term network (decode(): models.py:373-378 with a non-IRT generative model)."""
    U, V, W2, b2, w3, w1 = _pad_hidden(U, V, W2, b2, w3, w1)
    Up, Vp, Lp, gp, w1p, W2p, b2p, w3p, b3p = (_prep(t) for t in (U, V, logit, guess, w1, W2, b2, w3, b3))
    outs = []
    for s in range(0, B, PERSON_CHUNK):
        e = min(B, s + PERSON_CHUNK)
        dummy = torch.zeros(e - s, I, device=V.device)
        out = ops._BACKEND['decoder'](dummy, None, Up, Vp[s:e], None if Lp is None else Lp[s:e], gp, w1p, W2p, b2p, w3p, b3p,
                                      resid, False, want_prob=True)
        outs.append(out['prob'])
    return outs[0] if len(outs) == 1 else torch.cat(outs, 0)


MULTI_STACK_BYTES = 1 << 30      # samples per multi-sample call: their stacked per-person inputs (V, the logits) stay under this


def multi_sample_group(B, I, S, has_logit):
    """Samples per decoder_multi call: as many as keep V [s, B, 64] and (link / residual) the logits [s, B, I] under MULTI_STACK_BYTES."""
    per_sample = 4 * B * (HIDDEN + (I if has_logit else 0))
    return max(1, min(S, MULTI_STACK_BYTES // per_sample))


def _multi_chunks(response, mask, U, V, logit, guess, w1, W2, b2, w3, b3):
    """The prepared arguments of ops._BACKEND['decoder_multi'], person chunk by person chunk (PERSON_CHUNK, as the single call)."""
    U, V, W2, b2, w3, w1 = _pad_hidden(U, V, W2, b2, w3, w1)
    Up, Vp, Lp, gp, w1p, W2p, b2p, w3p, b3p = (_prep(t) for t in (U, V, logit, guess, w1, W2, b2, w3, b3))
    B = Vp.shape[1]
    for s in range(0, B, PERSON_CHUNK):
        e = min(B, s + PERSON_CHUNK)
        whole = s == 0 and e == B
        yield s, e, (response if (response is None or whole) else response[s:e], mask if (mask is None or whole) else mask[s:e], Up,
                     Vp if whole else Vp[:, s:e].contiguous(), Lp if (Lp is None or whole) else Lp[:, s:e].contiguous(),
                     gp, w1p, W2p, b2p, w3p, b3p)


@torch.no_grad()
def decoder_multi_log_lik(response, mask, *, U, V, W2, b2, w3, b3, logit=None, w1=None, guess=None, resid=0.0):
    """decoder_log_lik of S stacked samples in one launch per person chunk: U [S, I, H] or None, V [S, B, H], logit [S, B, I] or
    None, guess [S, I] or None; the weights and the rows are shared.  -> [S] log-likelihood sums; forward only (log_marginal).
    None where ops._BACKEND['decoder_multi'] does not cover the call: the caller then evaluates sample by sample."""
    backend = ops._BACKEND.get('decoder_multi')
    if backend is None:
        return None
    response, mask = _rows(response, mask)
    ll = None
    for s, e, args in _multi_chunks(response, mask, U, V, logit, guess, w1, W2, b2, w3, b3):
        out = backend(*args, resid)
        if out is None:
            return None
        part = out['ll_part'].sum(1)
        ll = part if ll is None else ll + part
    return ll


@torch.no_grad()
def decoder_multi_prob_sum(B, I, *, U, V, W2, b2, w3, b3, logit=None, w1=None, guess=None, resid=0.0, out=None):
    """Sum over the S stacked samples of decoder_probs [B, I], added cell by cell in sample order inside one launch per person chunk
    (the bits of accumulating S decoder_probs calls); `out`: a running sum of earlier calls to continue.  None where the backend does
    not cover the call."""
    backend = ops._BACKEND.get('decoder_multi')
    if backend is None:
        return None
    acc = out if out is not None else torch.empty(B, I, dtype=torch.float32, device=V.device)
    for s, e, args in _multi_chunks(None, None, U, V, logit, guess, w1, W2, b2, w3, b3):
        dummy = torch.zeros(e - s, I, device=V.device)
        if backend(dummy, *args[1:], resid, prob_sum=acc[s:e], prob_accumulate=out is not None) is None:
            return None
    return acc


def irt_logit_multi(irt_model, abilities, items):
    """irt_logit of stacked samples: abilities [S, B, A], items [S, I, D] -> logits [S, B, I] (and the 3PL guess [S, I])."""
    A = abilities.shape[2]
    if irt_model == 1:
        return abilities.sum(2, keepdim=True) + items.transpose(1, 2), None
    logit = torch.bmm(abilities, -items[:, :, :A].transpose(1, 2)) + items[:, :, A].unsqueeze(1)
    guess = torch.sigmoid(items[:, :, A + 1]) if irt_model == 3 else None
    return logit, guess


class _MultiSample:
    """log_marginal's and posterior_predictive's S samples through the multi-sample launch, in groups of multi_sample_group samples."""

    def _groups(self, abilities, items):
        S, B, I = abilities.shape[0], abilities.shape[1], items.shape[1]
        n = multi_sample_group(B, I, S, isinstance(self, LinkedIRT) or self.RESIDUAL)
        for s in range(0, S, n):
            yield self._args_multi(abilities[s:s + n], items[s:s + n])

    def multi_log_lik(self, response, mask, abilities, items):
        """[S] log-likelihood sums of the samples (abilities [S, B, A], items [S, I, D]), or None (not covered: evaluate one by one)."""
        if multi_declined(abilities):
            return None
        parts = []
        for args in self._groups(abilities, items):
            ll = decoder_multi_log_lik(response, mask, **args)
            if ll is None:
                return None
            parts.append(ll)
        return parts[0] if len(parts) == 1 else torch.cat(parts)

    def multi_prob_sum(self, abilities, items):
        """sum over the samples of forward(abilities[s], items[s]) [B, I], in sample order, or None (not covered)."""
        if multi_declined(abilities):
            return None
        acc = None
        for args in self._groups(abilities, items):
            acc = decoder_multi_prob_sum(abilities.shape[1], items.shape[1], out=acc, **args)
            if acc is None:
                return None
        return acc


def irt_logit(irt_model, ability, item_feat):
    """irt_model_*pl(..., return_logit=True) (models.py:729-766): [B, I] logits (and the 3PL guess probability [I])."""
    A = ability.shape[1]
    if irt_model == 1:
        return ability.sum(1, keepdim=True) + item_feat.t(), None
    logit = ability @ (-item_feat[:, :A].t()) + item_feat[:, A].unsqueeze(0)
    guess = torch.sigmoid(item_feat[:, A + 1]) if irt_model == 3 else None
    return logit, guess


def _mlp3(i, h, o, last_act=None):
    layers = [nn.Linear(i, h), nn.ELU(inplace=True), nn.Linear(h, h), nn.ELU(inplace=True), nn.Linear(h, o)]
    if last_act is not None:
        layers.append(last_act)
    return nn.Sequential(*layers)


def _xavier(m):
    if isinstance(m, nn.Linear):
        nn.init.xavier_normal_(m.weight.data, gain=nn.init.calculate_gain('relu'))
        nn.init.constant_(m.bias.data, 0)


class LinkedIRT(_MultiSample, nn.Module):
    """models.py:769-813: response_mu = link(irt logit), link = 1 -> H -> H -> 1 -> sigmoid (3PL: guess mixture)."""

    def __init__(self, irt_model=1, hidden_dim=HIDDEN):
        super().__init__()
        if hidden_dim > HIDDEN:
            raise NotImplementedError(f'hidden_dim = {hidden_dim}: the per-term decoder kernel covers hidden widths up to {HIDDEN}')
        self.irt_model, self.hidden_dim = irt_model, hidden_dim
        self.link = _mlp3(1, hidden_dim, 1, nn.Sigmoid())
        self.apply(_xavier)

    def _args(self, ability, item_feat):
        logit, guess = irt_logit(self.irt_model, ability, item_feat)
        lk = self.link
        V = lk[0].bias.unsqueeze(0).expand(ability.shape[0], -1)
        return dict(U=None, V=V, W2=lk[2].weight, b2=lk[2].bias, w3=lk[4].weight.reshape(-1), b3=lk[4].bias,
                    logit=logit, w1=lk[0].weight.reshape(-1), guess=guess, resid=0.0)

    def _args_multi(self, abilities, items):
        """_args of stacked samples: abilities [S, B, A], items [S, I, D]."""
        logit, guess = irt_logit_multi(self.irt_model, abilities, items)
        lk = self.link
        V = lk[0].bias.reshape(1, 1, -1).expand(abilities.shape[0], abilities.shape[1], -1)
        return dict(U=None, V=V, W2=lk[2].weight, b2=lk[2].bias, w3=lk[4].weight.reshape(-1), b3=lk[4].bias,
                    logit=logit, w1=lk[0].weight.reshape(-1), guess=guess, resid=0.0)

    def log_lik(self, response, mask, ability, item_feat):
        return decoder_log_lik(response, mask, **self._args(ability, item_feat))

    def forward(self, ability, item_feat):
        return decoder_probs(ability.shape[0], item_feat.shape[0], **self._args(ability, item_feat)).unsqueeze(2)


class DeepIRT(_MultiSample, nn.Module):
    """models.py:816-877: sigmoid(mlp_concat([mlp_item_feat(item), mlp_ability(ability)]))."""
    RESIDUAL = False

    def __init__(self, latent_dim, irt_model=1, hidden_dim=HIDDEN):
        super().__init__()
        if hidden_dim > HIDDEN:
            raise NotImplementedError(f'hidden_dim = {hidden_dim}: the per-term decoder kernel covers hidden widths up to {HIDDEN}')
        self.latent_dim = self.ability_dim = latent_dim
        self.irt_model, self.hidden_dim = irt_model, hidden_dim
        self.item_feat_dim = {1: 1, 2: latent_dim + 1, 3: latent_dim + 2}[irt_model]
        self.mlp_item_feat = _mlp3(self.item_feat_dim, hidden_dim, hidden_dim)
        self.mlp_ability = _mlp3(latent_dim, hidden_dim, hidden_dim)
        self.mlp_concat = _mlp3(2 * hidden_dim, hidden_dim, 1)
        self.apply(_xavier)

    def _args(self, ability, item_feat):
        mc, H = self.mlp_concat, self.hidden_dim
        # cat([hid_item, hid_ability]) through the first layer = its item half + its ability half (+ bias)
        U = self.mlp_item_feat(item_feat) @ mc[0].weight[:, :H].t()
        V = self.mlp_ability(ability) @ mc[0].weight[:, H:].t() + mc[0].bias
        a = dict(U=U, V=V, W2=mc[2].weight, b2=mc[2].bias, w3=mc[4].weight.reshape(-1), b3=mc[4].bias)
        if self.RESIDUAL:
            logit, guess = irt_logit(self.irt_model, ability, item_feat)
            a.update(logit=logit, guess=guess, resid=1.0)
        return a

    def _args_multi(self, abilities, items):
        """_args of stacked samples: abilities [S, B, A], items [S, I, D] (the small MLPs act on the last dimension)."""
        mc, H = self.mlp_concat, self.hidden_dim
        U = self.mlp_item_feat(items) @ mc[0].weight[:, :H].t()
        V = self.mlp_ability(abilities) @ mc[0].weight[:, H:].t() + mc[0].bias
        a = dict(U=U, V=V, W2=mc[2].weight, b2=mc[2].bias, w3=mc[4].weight.reshape(-1), b3=mc[4].bias)
        if self.RESIDUAL:
            logit, guess = irt_logit_multi(self.irt_model, abilities, items)
            a.update(logit=logit, guess=guess, resid=1.0)
        return a

    def log_lik(self, response, mask, ability, item_feat):
        return decoder_log_lik(response, mask, **self._args(ability, item_feat))

    def forward(self, ability, item_feat):
        return decoder_probs(ability.shape[0], item_feat.shape[0], **self._args(ability, item_feat)).unsqueeze(2)


class ResidualIRT(DeepIRT):
    """models.py:880-919: sigmoid(mlp_concat(...) + irt logit) (3PL: guess mixture)."""
    RESIDUAL = True

    def __init__(self, latent_dim, irt_model=1, hidden_dim=HIDDEN):
        super().__init__(latent_dim, irt_model=irt_model, hidden_dim=hidden_dim)
        self.apply(_xavier)          # (the reference's zero_init is a second xavier pass: same draws from the RNG stream)
