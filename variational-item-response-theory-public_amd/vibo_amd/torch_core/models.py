"""Drop-in VIBO_1PL / VIBO_2PL / VIBO_3PL modules whose ELBO runs in the fused HIP kernel.

Same constructor signature, ``state_dict`` keys, RNG draw order and method
surface as the reference (src/torch_core/models.py:246-548):

    model = VIBO_2PL(ability_dim, num_item, hidden_dim=64, ability_merge='product', ...)
    outputs = model(response, mask)                       # models.py:337-354
    loss = model.elbo(*outputs, annealing_factor=beta)    # models.py:380-443
    loss.backward()

``forward`` launches ONE fused kernel that already contains the backward pass;
``elbo`` only combines its two heads (log-lik, regulariser) with the item-side
terms, so ``loss.backward()`` never touches the response matrix again.

The only piece of forward()'s tuple that is not materialised is ``response_mu``
([B,I,1], as large as the input): it is a :class:`DeferredResponseMu` that
``elbo`` recognises; call ``.materialize()`` (or ``model.decode``) for the values.
"""
import dataclasses
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib, ops
from ..decoder import DeepIRT, LinkedIRT, ResidualIRT, multi_declined as decoder_multi_declined
from ..ops import ElboSpec, decode_probs, encode_posterior, fused_elbo, item_feat_dim

LOG_2PI = math.log(2.0 * math.pi)


# ---------------------------------------------------------------------------
# parameter containers (state_dict-compatible with the reference)
# ---------------------------------------------------------------------------

def _encoder_mlp(in_dim, hidden_dim, out_dim):
    return nn.Sequential(
        nn.Linear(in_dim, hidden_dim), nn.ELU(inplace=True),
        nn.Linear(hidden_dim, hidden_dim), nn.ELU(inplace=True),
        nn.Linear(hidden_dim, out_dim),
    )


class AbilityEncoder(nn.Module):
    """Holds ``mlp`` (keys ability_encoder.mlp.{0,2,4}.*; models.py:575-582).

    The network is evaluated on the 2 (unconditional) or 2 x I (conditional)
    distinct inputs a Bernoulli response can present, never per (person, item).
    """

    def __init__(self, ability_dim, item_dim, hidden_dim, conditional):
        super().__init__()
        self.ability_dim = ability_dim
        self.conditional = conditional
        if conditional:
            # the reference builds (and discards) the unconditional net first
            # (models.py:675-693); do the same so parameter init consumes the RNG identically
            _encoder_mlp(1, hidden_dim, 2 * ability_dim)
        self.mlp = _encoder_mlp(1 + (item_dim if conditional else 0), hidden_dim, 2 * ability_dim)
        # the two observed response values; a non-persistent buffer (not in state_dict) so that building the
        # table needs no host->device copy (keeps the step hipGraph-capturable)
        self.register_buffer('_response_values', torch.tensor([[0.0], [1.0]]), persistent=False)

    def expert_table(self, item_feat=None):
        """[2,2A] (row c = mlp([c])) or [2,I,2A] (entry = mlp([c, item_i]))."""
        vals = self._response_values.to(self.mlp[0].weight.dtype)
        if not self.conditional:
            return self.mlp(vals)
        I = item_feat.shape[0]
        x = torch.cat([vals.unsqueeze(1).expand(2, I, 1), item_feat.unsqueeze(0).expand(2, I, -1)], dim=2)
        return self.mlp(x.reshape(2 * I, -1)).view(2, I, -1)


class _SumGradAcrossRanks(torch.autograd.Function):
    """Identity whose backward all-reduces (sums) the gradient over the person shards: the mean-merge encoder's
    parameters see only this rank's persons through autograd."""

    @staticmethod
    def forward(ctx, x, reducer):
        ctx.reducer = reducer
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous().clone()
        ctx.reducer(g)
        return g, None


class MeanAbilityEncoder(nn.Module):
    """--ability-merge mean (keys ability_encoder.mlp1.{0,2}.*, mlp2.{0,2}.*; models.py:584-594, 631-650).

    mlp1 -> ELU gives one feature vector per (person, item) term, which for a Bernoulli response takes two values;
    the mean over a person's OBSERVED items is therefore (n0 h(0) + n1 h(1)) / n_obs with the counts of
    vibo_row_counts, and mlp2 -- the one dense [B,H] x [H,H] contraction of the path -- maps it to (mu, logvar)."""

    def __init__(self, ability_dim, hidden_dim, item_dim=0, conditional=False):
        super().__init__()
        self.ability_dim = ability_dim
        self.conditional = conditional

        def nets(in_dim):
            return (nn.Sequential(nn.Linear(in_dim, hidden_dim), nn.ELU(inplace=True), nn.Linear(hidden_dim, hidden_dim)),
                    nn.Sequential(nn.Linear(hidden_dim, hidden_dim), nn.ELU(inplace=True), nn.Linear(hidden_dim, 2 * ability_dim)))
        if conditional:
            nets(1)      # the reference builds (and discards) the unconditional nets first (models.py:675-693): same RNG draws
        self.mlp1, self.mlp2 = nets(1 + (item_dim if conditional else 0))
        self.register_buffer('_response_values', torch.tensor([[0.0], [1.0]]), persistent=False)

    def posterior_conditional(self, response, mask, item_feat, reducer=None, row_index=None):
        """--conditional-posterior (models.py:695-710 with _forward_mean :631-650): the per-term feature depends on the item
        too, h[c, i] = elu(mlp1([c, item_i])), so a person's mean over its observed items is the [B, 2I] x [2I, H]
        contraction of its one-hot coded row with the 2 x I feature table -- the encoder's one dense contraction, on the
        matrix pipe straight from the cell codes (ops.CodeTableSumFn: vibo_code_table_sum_forward / _backward; hidden width
        64) -- then mlp2, a plain [B, 64] GEMM.  response: fp32 rows [.., I] + mask, or CellCodes; row_index selects the minibatch."""
        I = item_feat.shape[0]
        vals = self._response_values.to(item_feat.dtype)
        x = torch.cat([vals.unsqueeze(1).expand(2, I, 1), item_feat.unsqueeze(0).expand(2, I, -1)], dim=2)
        h = F.elu(self.mlp1(x.reshape(2 * I, -1))).view(2, I, -1)                 # [2, I, H]
        l0, l2 = self.mlp2[0], self.mlp2[2]
        w0, b0, w2, b2 = l0.weight, l0.bias, l2.weight, l2.bias
        if reducer is not None:      # person-sharded: these see only this rank's persons
            h, w0, b0, w2, b2 = (_SumGradAcrossRanks.apply(t, reducer) for t in (h, w0, b0, w2, b2))
        if h.shape[2] == 64 and I <= 32767:      # (the native path's row counts are packed as n_correct << 16 | n_observed)
            hid_sum, nobs = ops._BACKEND['cond_mean_sum'](h, response, mask, row_index)
        else:
            # other hidden widths, more than 32 767 items: two dense GEMMs on the observed / correct indicator matrices
            if isinstance(response, ops.CellCodes):
                r, m = (response.rows(row_index) if row_index is not None else response).unpack()
            else:
                r = ops.prepare_response(response)
                m = None if mask is None else ops.prepare_mask(mask)[0]
                if row_index is not None:
                    r, m = r[row_index], (None if m is None else m[row_index])
            obs = torch.ones_like(r) if m is None else (m != 0).to(r.dtype)
            right = (r == 1).to(r.dtype) * obs
            hid_sum, nobs = obs @ h[0] + right @ (h[1] - h[0]), obs.sum(1)
        hid_mean = hid_sum / nobs.unsqueeze(1)             # (no observed item: 0/0 = NaN like the reference)
        return F.linear(F.elu(F.linear(hid_mean, w0, b0)), w2, b2)

    def posterior(self, counts, reducer=None):
        """[B, 2A] = (mu | logvar) of every person from the packed row counts (0 observed items -> NaN, as the
        reference's mean over an empty set, models.py:639-642)."""
        h = F.elu(self.mlp1(self._response_values.to(self.mlp1[0].weight.dtype)))        # [2, H]: the two per-term features
        l0, l2 = self.mlp2[0], self.mlp2[2]
        u = F.linear(h[0], l0.weight, l0.bias)              # first layer of mlp2 is affine in w = n_correct / n_observed
        v = F.linear(h[1] - h[0], l0.weight)
        w2, b2 = l2.weight, l2.bias
        if reducer is not None:      # person-sharded: these four see only this rank's persons
            u, v, w2, b2 = (_SumGradAcrossRanks.apply(t, reducer) for t in (u, v, w2, b2))
        return ops.MeanEncoderFn.apply(u, v, w2, b2, counts)


class ItemEncoder(nn.Module):
    """Per-item Gaussian posterior parameters (models.py:713-726)."""

    def __init__(self, num_item, item_dim):
        super().__init__()
        self.mu_lookup = nn.Embedding(num_item, item_dim)
        self.logvar_lookup = nn.Embedding(num_item, item_dim)

    def forward(self, item_index=None):
        if item_index is None:
            return self.mu_lookup.weight, self.logvar_lookup.weight
        idx = item_index.reshape(-1).long()
        return self.mu_lookup(idx), self.logvar_lookup(idx)


class PlanarFlowParams(nn.Module):
    """u, w ~ N(0,1), b = 1 (flows.py:15-19)."""

    def __init__(self, dim):
        super().__init__()
        self.u = nn.Parameter(torch.randn(dim))
        self.w = nn.Parameter(torch.randn(dim))
        self.b = nn.Parameter(torch.ones(1))

    def uhat(self):
        uw = torch.dot(self.u, self.w)
        return self.u + (F.softplus(uw) - 1.0 - uw) * self.w / torch.sum(self.w * self.w)

    def forward(self, z):
        """Planar step on rows of z (flows.py:21-41); used for the [I,D] item side."""
        uhat = self.uhat()
        t = torch.tanh(z @ self.w + self.b)
        z_new = z + uhat.unsqueeze(0) * t.unsqueeze(1)
        psi_u = (1.0 - t * t) * torch.dot(self.w, uhat)
        return z_new, torch.log(torch.abs(1.0 + psi_u) + 1e-8)


class FlowStack(nn.Module):
    """keys <name>.flows.{k}.{u,w,b} (flows.py:44-66)."""

    def __init__(self, dim, n_flows):
        super().__init__()
        self.flows = nn.ModuleList([PlanarFlowParams(dim) for _ in range(n_flows)])

    def forward(self, z):
        """(z_K, sum of log|det J|) of the rows of z: one native forward launch (and one backward launch) for the whole stack."""
        return ops._BACKEND['flow_stack'](z, self.packed())

    def packed(self):
        """[n_flows, 2*dim+1] = (uhat | w | b) rows for the kernels; uhat (flows.py:24-26) for all flows at once."""
        U = torch.stack([f.u for f in self.flows])
        W = torch.stack([f.w for f in self.flows])
        b = torch.cat([f.b for f in self.flows]).unsqueeze(1)
        uw = (U * W).sum(1, keepdim=True)
        uhat = U + (F.softplus(uw) - 1.0 - uw) * W / (W * W).sum(1, keepdim=True)
        return torch.cat([uhat, W, b], dim=1)


# ---------------------------------------------------------------------------
# deferred pieces of forward()'s tuple
# ---------------------------------------------------------------------------

class FusedContext:
    """What one fused kernel call produced, kept until elbo() consumes it."""

    def __init__(self, model, response, mask, eps_ability, table, item_in, flow_packed, reg_mode, heads):
        self.model = model
        self.response, self.mask = response, mask
        self.eps_ability = eps_ability
        self.table, self.item_in, self.flow_packed = table, item_in, flow_packed
        self.reg_mode = reg_mode
        (self.ll, self.reg, self.scalars, self.ability_mu, self.ability_logvar, self.ability,
         self.ability_k, self.ability_ladj) = heads


class DeferredResponseMu:
    """Stands in for response_mu [B,I,1] (models.py:345,351) in forward()'s tuple."""

    def __init__(self, ctx, ability, item_feat):
        self.ctx = ctx
        self._ability, self._item = ability, item_feat

    def materialize(self):
        return self.ctx.model.decode(self._ability.detach(), self._item.detach())

    def __repr__(self):
        return 'DeferredResponseMu(call .materialize() for the [B,I,1] tensor)'


class DecoderContext:
    """One forward of a --generative-model link|deep|residual model: the posterior side is ordinary autograd (it only
    needs the row counts), the log-likelihood is the decoder kernel's (vibo_amd/decoder.py), evaluated when elbo() asks."""

    def __init__(self, model, response, mask, row_index):
        self.model, self.response, self.mask, self.row_index = model, response, mask, row_index
        self._ll = None

    @property
    def ll(self):
        if self._ll is None:
            r, m = self.response, self.mask
            if self.row_index is not None:          # the decoder kernel walks dense rows: gather the minibatch here
                if isinstance(r, ops.CellCodes):
                    r = r.rows(self.row_index)
                else:
                    r = ops.prepare_response(r)[self.row_index]
                    m = None if m is None else ops.prepare_mask(m)[0][self.row_index]
            self._ll = self.model.decoder.log_lik(r, m, self.ability_k, self.item_k)
        return self._ll


# ---------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------

class VIBO_1PL(nn.Module):
    IRT = 1

    def __init__(self, latent_dim, num_item, hidden_dim=64, ability_merge='mean',
                 conditional_posterior=False, generative_model='irt', response_dist='bernoulli',
                 replace_missing_with_prior=True, n_norm_flows=0):
        super().__init__()
        if ability_merge not in ('mean', 'product'):
            raise AssertionError('ability_merge must be mean|product')   # models.py:262
        if generative_model not in ('irt', 'link', 'deep', 'residual'):
            raise AssertionError('bad generative_model')
        if response_dist not in ('bernoulli', 'gaussian'):
            raise AssertionError('bad response_dist')
        # the fused HIP path covers the 1PL/2PL/3PL logistic link with the product-of-experts
        # encoder on Bernoulli responses (BASELINE.json north_star); nothing else is in scope
        if response_dist != 'bernoulli':
            raise NotImplementedError("only --response-dist bernoulli is implemented by the HIP engine")

        self.latent_dim = self.ability_dim = latent_dim
        self.response_dim = 1
        self.hidden_dim = hidden_dim
        self.num_item = num_item
        self.ability_merge = ability_merge
        self.conditional_posterior = conditional_posterior
        self.generative_model = generative_model
        self.response_dist = response_dist
        self.replace_missing_with_prior = replace_missing_with_prior
        self.n_norm_flows = n_norm_flows
        self.irt_num = self.IRT
        self.item_feat_dim = item_feat_dim(self.IRT, latent_dim)
        self.spec = ElboSpec(irt_model=self.IRT, ability_dim=latent_dim,
                             conditional=conditional_posterior and ability_merge != 'mean',
                             drop_missing=not replace_missing_with_prior, n_flows=n_norm_flows,
                             given=ability_merge == 'mean')
        self.spec.check_supported(num_item)

        # construction order = the reference's (models.py:281-309) so seeded init matches
        if ability_merge == 'mean':
            self.ability_encoder = MeanAbilityEncoder(latent_dim, hidden_dim, self.item_feat_dim, conditional_posterior)
        else:
            self.ability_encoder = AbilityEncoder(latent_dim, self.item_feat_dim, hidden_dim, conditional_posterior)
        self.item_encoder = ItemEncoder(num_item, self.item_feat_dim)
        if n_norm_flows > 0:
            self.ability_norm_flows = FlowStack(latent_dim, n_norm_flows)
            self.item_norm_flows = FlowStack(self.item_feat_dim, n_norm_flows)
        # per-term MLP decoders (models.py:310-327, 769-919), built after the flows like the reference
        if generative_model == 'link':
            self.decoder = LinkedIRT(irt_model=self.IRT, hidden_dim=hidden_dim)
        elif generative_model == 'deep':
            self.decoder = DeepIRT(latent_dim, irt_model=self.IRT, hidden_dim=hidden_dim)
        elif generative_model == 'residual':
            self.decoder = ResidualIRT(latent_dim, irt_model=self.IRT, hidden_dim=hidden_dim)
        self.apply(self.weights_init)

        self._reducer = None          # set by enable_person_sharding()
        self._shard_world = 1
        self._last_ctx = None         # the most recent fused step (elbo() with a materialised response_mu finds it here)
        self._last_eps_item = None
        self._item_gen = None
        self._ability_gen = None

    # ---- init / RNG ---------------------------------------------------------
    @staticmethod
    def weights_init(m):
        """xavier-normal(gain=sqrt 2) on linears, zero bias (models.py:512-518)."""
        if isinstance(m, nn.Linear):
            nn.init.xavier_normal_(m.weight.data, gain=nn.init.calculate_gain('relu'))
            nn.init.constant_(m.bias.data, 0)

    def enable_person_sharding(self, reducer, seed, rank, world=None):
        """Data parallelism over persons: `reducer(flat)` all-reduces (sum) the
        kernel's flat [scalars | grads] buffer in place.  Item noise must be
        identical on every rank, ability noise must differ: dedicated generators.
        MLP-decoder models (--generative-model link | deep | residual) take their gradients from autograd on this rank's
        persons: their loss counts the replicated item-side terms 1 / world times and `allreduce_grads()` (one flat
        collective per step, called by the training loop after backward) sums every parameter gradient over the ranks."""
        self._reducer = reducer
        self._shard_rank = int(rank)
        if world is None:
            import torch.distributed as dist
            world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        self._shard_world = int(world)
        dev = self.item_encoder.mu_lookup.weight.device
        self._item_gen = torch.Generator(device=dev).manual_seed(int(seed))
        self._ability_gen = torch.Generator(device=dev).manual_seed(int(seed) + 1 + int(rank))

    def _randn(self, shape, ref, gen):
        return torch.randn(shape, dtype=ref.dtype, device=ref.device, generator=gen)

    @staticmethod
    def reparameterize_gaussian(mean, logvar, eps=None):
        """models.py:506-510."""
        std = torch.exp(0.5 * logvar)
        if eps is None:
            eps = torch.randn_like(std)
        return eps * std + mean

    # ---- pieces -------------------------------------------------------------
    def _item_side(self, eps_item=None):
        item_mu, item_lv = self.item_encoder()
        if eps_item is None:
            eps_item = self._randn(item_mu.shape, item_mu, self._item_gen)
        self._last_eps_item = eps_item          # (kept for elbo()'s re-run in the other regulariser mode)
        item_feat = eps_item * torch.exp(0.5 * item_lv) + item_mu
        return item_feat, item_mu, item_lv

    def _run_fused(self, response, mask, *, eps_item=None, eps_ability=None, reg_mode=None, row_index=None, posterior=None):
        """Item sample -> expert table -> fused kernel.  Draw order: item eps, then
        ability eps (models.py:361,368).  posterior: the mean-merge posterior [B, 2A] of these rows (and this item noise) where
        the caller has it already (log_marginal's loop after _draw_samples)."""
        item_feat, item_mu, item_lv = self._item_side(eps_item)
        if self.n_norm_flows > 0:
            item_k, item_ladj = self.item_norm_flows(item_feat)
            flow_packed = self.ability_norm_flows.packed()
        else:
            item_k, item_ladj, flow_packed = item_feat, None, None
        if self.ability_merge == 'mean':      # per-person posterior from the row counts; the kernel takes it as given
            response, mask, row_index = ops.chunkable_rows(response, mask, row_index)
            table = posterior if posterior is not None else self._mean_posterior(response, mask, row_index, item_feat)
        else:
            table = self.ability_encoder.expert_table(item_feat if self.conditional_posterior else None)
        B = int(row_index.numel()) if row_index is not None else response.shape[0]
        if eps_ability is None:
            eps_ability = self._randn((B, self.ability_dim), item_mu, self._ability_gen)
        if reg_mode is None:
            reg_mode = _lib.REG_SAMPLED if self.n_norm_flows > 0 else _lib.REG_KL
        heads = fused_elbo(self.spec, table, item_k, flow_packed, response, mask, eps_ability,
                           reg_mode=reg_mode, row_index=row_index, reducer=self._reducer)
        ctx = FusedContext(self, response, mask, eps_ability, table, item_k, flow_packed, reg_mode, heads)
        ctx.item_feat, ctx.item_mu, ctx.item_lv = item_feat, item_mu, item_lv
        ctx.item_k, ctx.item_ladj = item_k, item_ladj
        ctx.eps_item = self._last_eps_item          # the item noise actually used, drawn here or handed in
        ctx.row_index = row_index
        self._last_ctx = ctx
        return ctx

    def _mean_posterior(self, response, mask, row_index, item_feat, counts=None, reduce_in_backward=True):
        """(mu | logvar) [B, 2A] of the --ability-merge mean encoder: from the row counts, or (conditional posterior) from
        the minibatch's rows and the item sample.  reduce_in_backward=False: the caller sums all gradients itself."""
        reducer = self._reducer if reduce_in_backward else None
        if not self.conditional_posterior:
            if counts is None:
                counts = ops.row_counts(response, mask, row_index)
            return self.ability_encoder.posterior(counts, reducer=reducer)
        return self.ability_encoder.posterior_conditional(response, mask, item_feat, reducer=reducer, row_index=row_index)

    def _posterior_from_counts(self, counts):
        """(mu, logvar) [B, A] of the unconditional product of experts (models.py:596-629, utils.py:105-113) from the packed
        row counts: every observed cell contributes one of two experts, every missing one the N(0,1) prior (or nothing)."""
        A = self.ability_dim
        table = self.ability_encoder.expert_table(None)                      # [2, 2A]: rows = response 0 / 1
        n1 = (counts >> 16).to(table.dtype).unsqueeze(1)
        nobs = (counts & 0xffff).to(table.dtype).unsqueeze(1)
        n0 = nobs - n1
        tau = 1.0 / (torch.exp(table[:, A:]) + 1e-8)                          # [2, A]
        lam = n0 * tau[0] + n1 * tau[1]
        smu = n0 * (table[0, :A] * tau[0]) + n1 * (table[1, :A] * tau[1])
        if self.replace_missing_with_prior:
            lam = lam + (self.num_item - nobs) * (1.0 / (1.0 + 1e-8))
        return smu / lam, torch.log(1.0 / lam)

    def _conditional_posterior_poe(self, response, mask, row_index, item_feat):
        """Product of experts of the conditional encoder (models.py:695-710, utils.py:105-113) for the MLP-decoder models, where
        the ability gradient does not come out of the fused ELBO kernel.  The experts' per-person sums

            [lam | s][p, :] = sum_i [cell (p, i) observed] [tau | mu tau][code_pi, i, :]      = onehot(codes) [B, 2I] x X [2I, 2A]

        are the one-hot x table contraction of csrc/vibo_cmean.hip, straight from the minibatch's cell codes on the matrix pipe
        (ops.CodeTableSumFn: vibo_code_table_sum_forward, and its transpose vibo_code_table_sum_backward for the gradient that
        reaches the 2 x I-row expert table -- and through it the encoder MLP and the item sample); X is 2 x I x 2A numbers
        of plain autograd.  The kernels' table width is 64 columns: the 2A <= 16 used ones are padded with zeros."""
        A, I = self.ability_dim, item_feat.shape[0]
        table = self.ability_encoder.expert_table(item_feat)                  # [2, I, 2A]
        tau = 1.0 / (torch.exp(table[..., A:]) + 1e-8)
        feature = torch.cat([tau, table[..., :A] * tau, table.new_zeros(2, I, 64 - 2 * A)], dim=2)      # [2, I, 64]
        sums, nobs = ops._BACKEND['cond_mean_sum'](feature, response, mask, row_index)                  # [B, 64], [B]
        lam, smu = sums[:, :A], sums[:, A:2 * A]
        if self.replace_missing_with_prior:
            lam = lam + (I - nobs.unsqueeze(1)) * (1.0 / (1.0 + 1e-8))
        return smu / lam, torch.log(1.0 / lam)

    def _run_decoder(self, response, mask, *, eps_item=None, eps_ability=None, row_index=None):
        """forward() with a per-term MLP decoder: item sample, posterior from the row counts, sample, flows."""
        # (person-sharded: plain autograd on this rank's persons; allreduce_grads() sums the gradients after backward)
        item_feat, item_mu, item_lv = self._item_side(eps_item)
        if self.ability_merge == 'mean':
            counts = None if self.conditional_posterior else ops.row_counts(response, mask, row_index)
            amu, alv = torch.chunk(self._mean_posterior(response, mask, row_index, item_feat, counts, reduce_in_backward=False), 2, dim=1)
        elif self.conditional_posterior:
            amu, alv = self._conditional_posterior_poe(response, mask, row_index, item_feat)
        else:
            amu, alv = self._posterior_from_counts(ops.row_counts(response, mask, row_index))
        if eps_ability is None:
            eps_ability = self._randn(amu.shape, item_mu, self._ability_gen)
        ctx = DecoderContext(self, response, mask, row_index)
        ctx.eps_item, ctx.eps_ability = self._last_eps_item, eps_ability
        ctx.ability_mu, ctx.ability_logvar = amu, alv
        ctx.ability = eps_ability * torch.exp(0.5 * alv) + amu
        ctx.item_feat, ctx.item_mu, ctx.item_lv = item_feat, item_mu, item_lv
        if self.n_norm_flows > 0:
            ctx.ability_k, ctx.ability_ladj = self.ability_norm_flows(ctx.ability)
            ctx.item_k, ctx.item_ladj = self.item_norm_flows(item_feat)
        else:
            ctx.ability_k, ctx.ability_ladj, ctx.item_k, ctx.item_ladj = ctx.ability, None, item_feat, None
        self._last_ctx = ctx
        return ctx

    # ---- reference method surface --------------------------------------------
    def forward(self, response, mask, eps_item=None, eps_ability=None, row_index=None):
        run = self._run_fused if self.generative_model == 'irt' else self._run_decoder
        ctx = run(response, mask, eps_item=eps_item, eps_ability=eps_ability, row_index=row_index)
        if self.n_norm_flows > 0:
            rmu = DeferredResponseMu(ctx, ctx.ability_k, ctx.item_k)
            return (response, mask, rmu, ctx.ability_k, ctx.ability, ctx.ability_mu, ctx.ability_logvar,
                    ctx.ability_ladj, ctx.item_k, ctx.item_feat, ctx.item_mu, ctx.item_lv, ctx.item_ladj)
        rmu = DeferredResponseMu(ctx, ctx.ability, ctx.item_feat)
        return (response, mask, rmu, ctx.ability, ctx.ability_mu, ctx.ability_logvar,
                ctx.item_feat, ctx.item_mu, ctx.item_lv)

    def encode(self, response, mask, row_index=None):
        """(ability, ability_mu, ability_logvar, item_feat, item_feat_mu, item_feat_logvar)
        (models.py:356-371): forward-only kernel, no gradients through the ability side."""
        item_feat, item_mu, item_lv = self._item_side()
        with torch.no_grad():
            if self.ability_merge == 'mean':
                amu, alv = torch.chunk(self._mean_posterior(response, mask, row_index, item_feat), 2, dim=1)
            else:
                table = self.ability_encoder.expert_table(item_feat if self.conditional_posterior else None)
                amu, alv = encode_posterior(self.spec, table, response, mask, row_index=row_index)
            ability = self.reparameterize_gaussian(
                amu, alv, self._randn(amu.shape, amu, self._ability_gen))
        return ability, amu, alv, item_feat, item_mu, item_lv

    def decode(self, ability, item_feat):
        """response_mu [B,I,1] (models.py:373-378, 529-533, 544-548)."""
        if self.generative_model != 'irt':
            return self.decoder(ability, item_feat)
        return decode_probs(self.spec, ability, item_feat).unsqueeze(2)

    def elbo(self, response, mask, response_mu, ability, ability_mu, ability_logvar,
             item_feat, item_feat_mu, item_feat_logvar, annealing_factor=1, use_kl_divergence=True,
             ability_k=None, item_feat_k=None, ability_logabsdetjac=None, item_logabsdetjac=None):
        """-ELBO summed over the minibatch (models.py:380-443)."""
        if isinstance(response_mu, DeferredResponseMu):
            ctx = response_mu.ctx
        else:
            # a caller that materialised response_mu through decode() first (vibo.py:379-style code): the fused step of
            # the forward() that produced `ability` is still the one to score -- the tensor itself is not needed
            last = self._last_ctx
            ctx = last if (last is not None and (ability is last.ability or ability is last.ability_k)) else None
            if ctx is None:
                raise TypeError('elbo() expects the outputs of this model\'s forward(); a response_mu tensor that does '
                                'not come from it would need a second pass over the responses')
        if isinstance(ctx, DecoderContext):
            return self._decoder_elbo(ctx, annealing_factor, use_kl_divergence)
        want_mode = _lib.REG_SAMPLED if (self.n_norm_flows > 0 or not use_kl_divergence) else _lib.REG_KL
        if want_mode != ctx.reg_mode:
            if torch.is_grad_enabled() and ctx.ll.requires_grad:
                # rare: use_kl_divergence=False asked of a KL-mode forward -> redo the step in SAMPLED mode
                ctx = self._run_fused(ctx.response, ctx.mask, eps_item=ctx.eps_item,
                                      eps_ability=ctx.eps_ability, reg_mode=want_mode, row_index=ctx.row_index)
                item_feat, item_feat_mu, item_feat_logvar = ctx.item_feat, ctx.item_mu, ctx.item_lv
                reg = ctx.reg
            else:
                sc = ctx.scalars
                reg = (sc[_lib.S_LOGQ0] - sc[_lib.S_LADJ] - sc[_lib.S_LOGP]) if want_mode == _lib.REG_SAMPLED \
                    else sc[_lib.S_KL]
        else:
            reg = ctx.reg
        ll = ctx.ll
        if self.n_norm_flows > 0:
            assert item_feat_k is not None and item_logabsdetjac is not None
            log_p_d, log_q_d = _item_log_terms(item_feat, item_feat_mu, item_feat_logvar, item_feat_k, item_logabsdetjac)
            return -(ll + log_p_d - reg - log_q_d)
        if use_kl_divergence:
            kl_d = (-0.5 * (1.0 + item_feat_logvar - item_feat_mu.pow(2) - item_feat_logvar.exp())).sum()
            return -(ll - annealing_factor * reg - annealing_factor * kl_d)
        log_p_d, log_q_d = _item_log_terms(item_feat, item_feat_mu, item_feat_logvar, item_feat, None)
        return -(ll + log_p_d - reg - log_q_d)

    def _decoder_elbo(self, ctx, annealing_factor, use_kl_divergence):
        """models.py:380-443 with the decoder kernel's log-likelihood; the small per-person / per-item terms are autograd.
        Person-sharded: this rank's persons and 1 / world of the (replicated) item-side terms -- the ranks' losses and
        gradients add up to the unsharded ones (allreduce_grads)."""
        ll = ctx.ll
        iw = 1.0 / self._shard_world if self._reducer is not None else 1.0
        if self.n_norm_flows > 0:
            log_q = (_normal_logpdf(ctx.ability, ctx.ability_mu, ctx.ability_logvar).sum() - ctx.ability_ladj.sum()
                     + iw * (_normal_logpdf(ctx.item_feat, ctx.item_mu, ctx.item_lv).sum() - ctx.item_ladj.sum()))
            log_p = ll + _std_normal_logpdf(ctx.ability_k).sum() + iw * _std_normal_logpdf(ctx.item_k).sum()
            return -(log_p - log_q)
        if use_kl_divergence:
            kl_u = (-0.5 * (1.0 + ctx.ability_logvar - ctx.ability_mu.pow(2) - ctx.ability_logvar.exp())).sum()
            kl_d = (-0.5 * (1.0 + ctx.item_lv - ctx.item_mu.pow(2) - ctx.item_lv.exp())).sum()
            return -(ll - annealing_factor * kl_u - annealing_factor * iw * kl_d)
        log_p = ll + _std_normal_logpdf(ctx.ability).sum() + iw * _std_normal_logpdf(ctx.item_feat).sum()
        log_q = (_normal_logpdf(ctx.ability, ctx.ability_mu, ctx.ability_logvar).sum()
                 + iw * _normal_logpdf(ctx.item_feat, ctx.item_mu, ctx.item_lv).sum())
        return -(log_p - log_q)

    @property
    def needs_grad_allreduce(self):
        """True for a person-sharded MLP-decoder model: call allreduce_grads() between backward() and the optimizer step."""
        return self._reducer is not None and self.generative_model != 'irt'

    def allreduce_grads(self, loss=None):
        """Sum every parameter gradient (and, if given, the detached loss) over the person shards: ONE flat collective."""
        ps = [p for p in self.parameters() if p.requires_grad]
        flat = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for p in ps]
                         + ([loss.detach().reshape(1)] if loss is not None else []))
        self._reducer(flat)
        off = 0
        for p in ps:
            n = p.numel()
            g = flat[off:off + n].view_as(p)
            if p.grad is None:
                p.grad = g.clone()
            else:
                p.grad.copy_(g)
            off += n
        return flat[off] if loss is not None else None

    def allreduce_loss(self, loss):
        """The detached shard-local loss of a person-sharded MLP-decoder model summed over the ranks (evaluation loops,
        vibo.py:291-312 under sharding: one scalar collective per step)."""
        t = loss.detach().reshape(1).clone()
        self._reducer(t)
        return t[0]

    def log_marginal(self, response, mask, num_samples=100, eps_item=None, eps_ability=None):
        """Importance-weighted bound with batch-level weights (models.py:445-504).  eps_item [S,I,D] / eps_ability
        [S,B,A] replay a fixed noise sequence (tests); by default it is drawn item-then-ability per sample like the
        reference's loop.  The S forwards share one pass over the responses: the unconditional product of experts
        (vibo_elbo_multi_forward); --ability-merge mean, whose posterior reaches the kernel as given
        (vibo_elbo_multi_forward_given: one [B, 2A] posterior for all samples, or with --conditional-posterior one per sample);
        product of experts x conditional posterior, whose per-sample encoder tables go in stacked (vibo_elbo_multi_forward_cond:
        the experts' sums of up to 64 / 2A samples per contraction pass over the cell codes); the MLP-decoder models
        (--generative-model link | deep | residual: vibo_decoder_multi_forward, _decoder_multi_log_weights; person-sharded ones keep
        the loop).  Otherwise -- a person-sharded
        mean-merge or conditional model (its heads go through the collective), a backend that answers None -- one forward launch
        per sample."""
        with torch.no_grad():
            S = int(num_samples)
            if self.generative_model != 'irt':
                if self._reducer is None and not decoder_multi_declined(response):
                    # all S samples through one decoder launch (asked before anything is drawn or stacked); where the backend still
                    # answers None the loop below replays the noise
                    log_w, eps_item, eps_ability = self._decoder_multi_log_weights(response, mask, S, eps_item, eps_ability)
                    if log_w is not None:
                        return _log_mean_exp(log_w)
                log_w = []
                for s in range(S):
                    ctx = self._run_decoder(response, mask, eps_item=None if eps_item is None else eps_item[s],
                                            eps_ability=None if eps_ability is None else eps_ability[s])
                    log_w.append(-self._decoder_elbo(ctx, 1.0, False))
                return _log_mean_exp(torch.stack(log_w))
            draws = None
            # (person-sharded mean merge or conditional posterior: the loop reduces its heads through the collective)
            if self._reducer is None or not (self.ability_merge == 'mean' or self.conditional_posterior):
                response, mask = ops.chunkable_rows(response, mask)
                draws = self._draw_samples(response, mask, S, eps_item, eps_ability)
            if draws is not None:
                log_w = _multi_log_weights(self.spec, response, mask, draws)
                if log_w is not None:
                    return _log_mean_exp(log_w)
                # not covered (fewer than 4 items, ...): the loop below replays the noise already drawn and, for mean merge,
                # takes the posteriors already computed from it
                eps_item, eps_ability = draws.eps_item, draws.eps_ability
            log_w = []
            for s in range(S):
                ctx = self._run_fused(response, mask, reg_mode=_lib.REG_SAMPLED,
                                      eps_item=None if eps_item is None else eps_item[s],
                                      eps_ability=None if eps_ability is None else eps_ability[s],
                                      posterior=None if draws is None else draws.posterior(s))
                log_pd, log_qd = _item_log_terms(ctx.item_feat, ctx.item_mu, ctx.item_lv, ctx.item_k, ctx.item_ladj)
                log_w.append(ctx.ll + log_pd - ctx.reg - log_qd)
            return _log_mean_exp(torch.stack(log_w))

    def _decoder_multi_log_weights(self, response, mask, S, eps_item, eps_ability):
        """log_marginal of an MLP-decoder model (not person-sharded) with its S samples stacked: -> (log w [S], eps_item [S, I, D],
        eps_ability [S, B, A]); log w is None where the multi-sample decoder launch does not cover the call -- the noise, drawn in
        the loop's order (item then ability, per sample), is then the loop's to replay.  The posterior is computed once where it
        does not depend on the sample (from the row counts, counted once) and once per item sample where it does (conditional
        posterior, through the loop's own calls); flows act on the stacked rows; one ops._BACKEND['decoder_multi'] call gives the
        S log-likelihoods; the remaining terms are _decoder_elbo(ctx, 1.0, False)'s, per sample."""
        item_mu, item_lv = self.item_encoder()
        B, A = response.shape[0], self.ability_dim
        if eps_item is None or eps_ability is None:
            drawn_i, drawn_a = [], []
            for s in range(S):
                drawn_i.append(self._randn(item_mu.shape, item_mu, self._item_gen) if eps_item is None else eps_item[s])
                drawn_a.append(self._randn((B, A), item_mu, self._ability_gen) if eps_ability is None else eps_ability[s])
            eps_item, eps_ability = torch.stack(drawn_i), torch.stack(drawn_a)
        else:
            eps_item, eps_ability = (t[:S] if torch.is_tensor(t) else torch.stack(list(t[:S])) for t in (eps_item, eps_ability))
        item_feat = eps_item * torch.exp(0.5 * item_lv) + item_mu                       # [S, I, D]
        if self.conditional_posterior:      # depends on the item sample (in front of the item flows, as _run_decoder)
            if self.ability_merge == 'mean':
                per = [torch.chunk(self._mean_posterior(response, mask, None, item_feat[s], None, reduce_in_backward=False), 2, dim=1)
                       for s in range(S)]
            else:
                per = [self._conditional_posterior_poe(response, mask, None, item_feat[s]) for s in range(S)]
            amu, alv = torch.stack([p[0] for p in per]), torch.stack([p[1] for p in per])
        else:
            counts = ops.row_counts(response, mask, None)
            if self.ability_merge == 'mean':
                amu, alv = torch.chunk(self._mean_posterior(response, mask, None, None, counts, reduce_in_backward=False), 2, dim=1)
            else:
                amu, alv = self._posterior_from_counts(counts)
            amu, alv = amu.unsqueeze(0), alv.unsqueeze(0)
        ability = eps_ability * torch.exp(0.5 * alv) + amu                              # [S, B, A]
        if self.n_norm_flows > 0:           # FlowStack is row-wise: the samples' rows go through stacked
            ability_k, ability_ladj = self.ability_norm_flows(ability.reshape(S * B, A))
            item_k, item_ladj = self.item_norm_flows(item_feat.reshape(S * item_feat.shape[1], -1))
            ability_k, item_k = ability_k.reshape(ability.shape), item_k.reshape(item_feat.shape)
            ladj = ability_ladj.reshape(S, B).sum(1), item_ladj.reshape(S, -1).sum(1)
        else:
            ability_k, item_k, ladj = ability, item_feat, None
        ll = self.decoder.multi_log_lik(response, mask, ability_k, item_k)
        if ll is None:
            return None, eps_item, eps_ability
        per_sample = lambda t: t.flatten(1).sum(1)
        log_q_u = per_sample(_normal_logpdf(ability, amu, alv))
        log_q_d = per_sample(_normal_logpdf(item_feat, item_mu, item_lv))
        if ladj is not None:
            log_q_u, log_q_d = log_q_u - ladj[0], log_q_d - ladj[1]
        log_p = ll + per_sample(_std_normal_logpdf(ability_k)) + per_sample(_std_normal_logpdf(item_k))
        return log_p - (log_q_u + log_q_d), eps_item, eps_ability

    def _draw_samples(self, response, mask, S, eps_item, eps_ability):
        """The S samples of log_marginal as the multi-sample forward kernel takes them (_Draws), or None -- nothing drawn, nothing
        stacked -- for an int64 mask and where the native backend's workspace query already declines the call.
        --ability-merge mean: the posterior goes to the kernel as given -- _mean_posterior once for all samples, or (conditional
        posterior: it depends on the item sample) once per sample, stacked to [S, B, 2A].  Product of experts x conditional
        posterior: the encoder's table of every item sample (expert_table of the sample in front of the item flows, as _run_fused),
        stacked to [S, 2, I, 2A]; the kernel forms the posteriors.  Memory: the stacked noise is S B A floats
        and the per-sample posteriors S B 2A (1M persons, A = 8, S = 16: 0.5 + 1 GB): a caller with a whole resident split and many
        samples passes it in minibatches."""
        rows, mask2, code = ops.prepare_rows(response, mask)
        B = rows.shape[0]
        if code == _lib.MASK_I64 or ops.multi_forward_declined(self.spec, rows, mask2, code, S, B):
            return None
        mean_merge = self.ability_merge == 'mean'
        item_mu, item_lv = self.item_encoder()
        drawn_items, items, eps_ab, log_pd, log_qd, tables = [], [], [], [], [], []
        for s in range(S):                      # draw order of the reference's loop: item eps, then ability eps
            e_i = self._randn(item_mu.shape, item_mu, self._item_gen) if eps_item is None else eps_item[s]
            drawn_items.append(e_i)
            item_feat = e_i * torch.exp(0.5 * item_lv) + item_mu
            item_k, item_ladj = self.item_norm_flows(item_feat) if self.n_norm_flows > 0 else (item_feat, None)
            lp, lq = _item_log_terms(item_feat, item_mu, item_lv, item_k, item_ladj)
            if self.conditional_posterior:      # (from the item sample in front of the item flows, as _run_fused)
                tables.append(self._mean_posterior(response, mask, None, item_feat) if mean_merge
                              else self.ability_encoder.expert_table(item_feat))
            items.append(item_k)
            log_pd.append(lp)
            log_qd.append(lq)
            eps_ab.append(self._randn((B, self.ability_dim), item_mu, self._ability_gen)
                          if eps_ability is None else eps_ability[s])
        if self.conditional_posterior:
            table = torch.stack(tables)
        else:
            table = self._mean_posterior(response, mask, None, None) if mean_merge else self.ability_encoder.expert_table(None)
        return _Draws(eps_item=drawn_items if eps_item is None else eps_item, items=torch.stack(items).contiguous(),
                      eps_ability=torch.stack(eps_ab), log_pd=torch.stack(log_pd), log_qd=torch.stack(log_qd),
                      table=table.contiguous(), given=mean_merge,
                      flow_packed=self.ability_norm_flows.packed() if self.n_norm_flows > 0 else None)

    # ---- fast path for training loops (no tuple round trip) -------------------
    def elbo_step(self, response, mask, annealing_factor=1.0, row_index=None):
        """loss = model.elbo(*model(response, mask), annealing_factor) in one call."""
        out = self.forward(response, mask, row_index=row_index)
        if self.n_norm_flows > 0:
            (r, m, rmu, ak, a0, amu, alv, aladj, ik, i0, imu, ilv, iladj) = out
            loss = self.elbo(r, m, rmu, a0, amu, alv, i0, imu, ilv, annealing_factor=annealing_factor,
                             use_kl_divergence=False, ability_k=ak, item_feat_k=ik,
                             ability_logabsdetjac=aladj, item_logabsdetjac=iladj)
        else:
            loss = self.elbo(*out, annealing_factor=annealing_factor, use_kl_divergence=True)
        # the step's context (autograd graph, row references, the decoder kernel's gradient records) has been consumed: do not
        # keep it alive until the next forward (it exists for elbo() calls with a materialised response_mu)
        self._last_ctx = None
        return loss


class VIBO_2PL(VIBO_1PL):
    IRT = 2


class VIBO_3PL(VIBO_2PL):
    IRT = 3


# ---------------------------------------------------------------------------
# un-amortized VI (reference models.py:100-243; training script vi.py): per-person posteriors in two embeddings
# ---------------------------------------------------------------------------

class VI_1PL(nn.Module):
    """Drop-in for the reference's VI_1PL/2PL/3PL: forward(index, response, mask) -> the 9-tuple, elbo(*outputs).
    The per-person (mu, logvar) rows looked up by `index` go to the fused kernel as a caller-supplied posterior
    (VIBO_POSTERIOR_GIVEN); its per-person gradients flow back into the embeddings through autograd."""
    IRT = 1

    def __init__(self, latent_dim, num_person, num_item):
        super().__init__()
        self.latent_dim = self.ability_dim = latent_dim
        self.response_dim = 1
        self.num_person, self.num_item = num_person, num_item
        self.item_feat_dim = item_feat_dim(self.IRT, latent_dim)
        self.spec = ElboSpec(irt_model=self.IRT, ability_dim=latent_dim, given=True)
        self.spec.check_supported(num_item)
        # construction order = the reference's (models.py:113-117): N(0,1) embeddings drawn in this order
        self.ability_mu_lookup = nn.Embedding(num_person, latent_dim)
        self.ability_logvar_lookup = nn.Embedding(num_person, latent_dim)
        self.item_mu_lookup = nn.Embedding(num_item, self.item_feat_dim)
        self.item_logvar_lookup = nn.Embedding(num_item, self.item_feat_dim)

    @staticmethod
    def reparameterize_gaussian(mean, logvar, eps=None):
        std = torch.exp(0.5 * logvar)
        return (torch.randn_like(std) if eps is None else eps) * std + mean

    def _posterior_rows(self, index):
        idx = index.reshape(-1).long()
        return self.ability_mu_lookup(idx), self.ability_logvar_lookup(idx)

    def _run(self, index, response, mask, eps_item=None, eps_ability=None, reg_mode=_lib.REG_KL, row_index=None):
        item_mu, item_lv = self.item_mu_lookup.weight, self.item_logvar_lookup.weight
        item_feat = self.reparameterize_gaussian(item_mu, item_lv, eps_item)          # item eps first (models.py:128-135)
        amu, alv = self._posterior_rows(index)
        B = amu.shape[0]
        if eps_ability is None:
            eps_ability = torch.randn(B, self.ability_dim, dtype=amu.dtype, device=amu.device)
        response, mask, row_index = ops.chunkable_rows(response, mask, row_index)
        table = torch.cat([amu, alv], dim=1)
        heads = fused_elbo(self.spec, table, item_feat, None, response, mask, eps_ability, reg_mode=reg_mode,
                           row_index=row_index)
        ctx = FusedContext(self, response, mask, eps_ability, table, item_feat, None, reg_mode, heads)
        ctx.item_feat, ctx.item_mu, ctx.item_lv, ctx.eps_item = item_feat, item_mu, item_lv, eps_item
        ctx.index, ctx.row_index, ctx.amu, ctx.alv = index, row_index, amu, alv
        return ctx

    def forward(self, index, response, mask, eps_item=None, eps_ability=None, row_index=None):
        """(response, mask, response_mu, ability, ability_mu, ability_logvar, item_feat, item_feat_mu,
        item_feat_logvar) (models.py:120-126).  `row_index` gathers the rows from a resident matrix in-kernel."""
        ctx = self._run(index, response, mask, eps_item, eps_ability, row_index=row_index)
        return (response, mask, DeferredResponseMu(ctx, ctx.ability, ctx.item_feat), ctx.ability, ctx.amu, ctx.alv,
                ctx.item_feat, ctx.item_mu, ctx.item_lv)

    def encode(self, index, response=None, mask=None):
        """models.py:127-139 (plain lookups + reparameterisation; no pass over the responses)."""
        item_mu, item_lv = self.item_mu_lookup.weight, self.item_logvar_lookup.weight
        item_feat = self.reparameterize_gaussian(item_mu, item_lv)
        amu, alv = self._posterior_rows(index)
        return self.reparameterize_gaussian(amu, alv), amu, alv, item_feat, item_mu, item_lv

    def decode(self, ability, item_feat):
        return decode_probs(self.spec, ability, item_feat).unsqueeze(2)

    def elbo(self, response, mask, response_mu, ability, ability_mu, ability_logvar, item_feat, item_feat_mu,
             item_feat_logvar, annealing_factor=1, use_kl_divergence=True):
        """-ELBO summed over the minibatch (models.py:144-172)."""
        if not isinstance(response_mu, DeferredResponseMu):
            raise TypeError('elbo() expects the outputs of this model\'s forward()')
        ctx = response_mu.ctx
        want_mode = _lib.REG_KL if use_kl_divergence else _lib.REG_SAMPLED
        if want_mode != ctx.reg_mode:
            if torch.is_grad_enabled() and ctx.ll.requires_grad:
                ctx = self._run(ctx.index, ctx.response, ctx.mask, ctx.eps_item, ctx.eps_ability, reg_mode=want_mode,
                                row_index=ctx.row_index)
                item_feat, item_feat_mu, item_feat_logvar = ctx.item_feat, ctx.item_mu, ctx.item_lv
                reg = ctx.reg
            else:
                sc = ctx.scalars
                reg = (sc[_lib.S_LOGQ0] - sc[_lib.S_LOGP]) if want_mode == _lib.REG_SAMPLED else sc[_lib.S_KL]
        else:
            reg = ctx.reg
        if use_kl_divergence:
            kl_d = (-0.5 * (1.0 + item_feat_logvar - item_feat_mu.pow(2) - item_feat_logvar.exp())).sum()
            return -(ctx.ll - annealing_factor * reg - annealing_factor * kl_d)
        log_p_d, log_q_d = _item_log_terms(item_feat, item_feat_mu, item_feat_logvar, item_feat, None)
        return -(ctx.ll + log_p_d - reg - log_q_d)

    def log_marginal(self, index, response, mask, num_samples=100):
        """Batch-level importance-weighted bound (models.py:174-207; the reference's own loop there omits `index` in its
        forward call and cannot run -- this is the same estimator with the index passed)."""
        with torch.no_grad():
            S = int(num_samples)
            response, mask = ops.chunkable_rows(response, mask)      # (as _run pads compact ragged rows)
            draws = self._draw_samples(index, S)
            log_w = _multi_log_weights(self.spec, response, mask, draws)
            if log_w is None:      # not covered by the multi-sample kernel: one forward per sample on the noise already drawn
                log_w = []
                for s in range(S):
                    outs = self.forward(index, response, mask, eps_item=draws.eps_item[s], eps_ability=draws.eps_ability[s])
                    log_w.append(-self.elbo(*outs, annealing_factor=1, use_kl_divergence=False))
                log_w = torch.stack(log_w)
            return _log_mean_exp(log_w)

    def _draw_samples(self, index, S):
        """The S samples of log_marginal for the multi-sample forward (vibo_elbo_multi_forward_given: the looked-up (mu | logvar)
        rows are the posterior of every sample).  The noise comes from the default generator in _run's order: item randn_like, then
        randn(B, A), per sample."""
        item_mu, item_lv = self.item_mu_lookup.weight, self.item_logvar_lookup.weight
        amu, alv = self._posterior_rows(index)
        B = amu.shape[0]
        std = torch.exp(0.5 * item_lv)
        eps_item, eps_ab = [], []
        for _ in range(S):
            eps_item.append(torch.randn_like(std))
            eps_ab.append(torch.randn(B, self.ability_dim, dtype=amu.dtype, device=amu.device))
        eps_item, eps_ab = torch.stack(eps_item), torch.stack(eps_ab)
        items = eps_item * std + item_mu                                              # [S, I, D]
        return _Draws(eps_item=eps_item, items=items.contiguous(), eps_ability=eps_ab,
                      log_pd=_std_normal_logpdf(items).sum((1, 2)), log_qd=_normal_logpdf(items, item_mu, item_lv).sum((1, 2)),
                      table=torch.cat([amu, alv], dim=1).contiguous(), flow_packed=None, given=True)


class VI_2PL(VI_1PL):
    IRT = 2


class VI_3PL(VI_2PL):
    IRT = 3


# ---------------------------------------------------------------------------
# maximum-likelihood point estimates (reference models.py:22-97; training script mle.py)
# ---------------------------------------------------------------------------

class MLE_1PL(nn.Module):
    """Drop-in for the reference's MLE_1PL/2PL/3PL (keys ability.weight [P,A], item_feat.weight [I,D]).

    forward(index, response, mask) returns the materialised response_mu [B,I,1] with autograd, as the reference's
    training loop needs it (mle.py:193-197 computes the masked BCE itself) -- that is an O(B I) PyTorch tensor by
    contract.  `nll_step` is the same loss (mean over ALL B x I cells of mask x BCE) through the fused kernel: the persons'
    rows are a caller-supplied posterior with zero noise, so the sample is the point estimate and the kernel's d LL/d mu,
    d LL/d item are the gradients; one pass over the response rows, nothing of size B x I is stored."""
    IRT = 1

    def __init__(self, latent_dim, num_person, num_item):
        super().__init__()
        self.latent_dim = self.ability_dim = latent_dim
        self.response_dim = 1
        self.num_person, self.num_item = num_person, num_item
        self.item_feat_dim = item_feat_dim(self.IRT, latent_dim)
        self.spec = ElboSpec(irt_model=self.IRT, ability_dim=latent_dim, given=True)
        self.spec.check_supported(num_item)
        self.ability = nn.Embedding(num_person, latent_dim)                 # models.py:41-42, N(0,1) init
        self.item_feat = nn.Embedding(num_item, self.item_feat_dim)

    def encode(self, index, response=None, mask=None):
        return self.ability(index.reshape(-1).long()), self.item_feat.weight       # models.py:49-53

    def decode(self, ability, item_feat):
        return decode_probs(self.spec, ability, item_feat).unsqueeze(2)

    def forward(self, index, response=None, mask=None):
        ability, item = self.encode(index)
        A = self.ability_dim
        if self.IRT == 1:                                                       # models.py:729-735
            logit = ability.sum(1, keepdim=True) + item[:, 0].unsqueeze(0)
        else:                                                                    # models.py:738-766
            logit = -(ability @ item[:, :A].t()) + item[:, A].unsqueeze(0)
        p = torch.sigmoid(logit)
        if self.IRT == 3:
            guess = torch.sigmoid(item[:, A + 1]).unsqueeze(0)
            p = guess + (1.0 - guess) * p
        return p.unsqueeze(2)

    def nll_step(self, index, response, mask, row_index=None):
        """mean_{B x I}(mask * BCE(response_mu, response)) (mle.py:193-196) without materialising response_mu."""
        ability, item = self.encode(index)
        B = ability.shape[0]
        response, mask, row_index = ops.chunkable_rows(response, mask, row_index)
        table = torch.cat([ability, torch.zeros_like(ability)], dim=1)          # (mu | logvar = 0), eps = 0: theta = mu
        heads = fused_elbo(self.spec, table, item, None, response, mask, torch.zeros_like(ability), reg_mode=_lib.REG_KL,
                           row_index=row_index)
        return -heads[0] / float(B * self.num_item)


class MLE_2PL(MLE_1PL):
    IRT = 2


class MLE_3PL(MLE_2PL):
    IRT = 3


def _normal_logpdf(x, mu, logvar):
    return -0.5 * LOG_2PI - 0.5 * logvar - 0.5 * (x - mu) ** 2 / logvar.exp()


def _std_normal_logpdf(x):
    return -0.5 * LOG_2PI - 0.5 * x * x


def _item_log_terms(item_feat, item_mu, item_lv, item_k, item_ladj):
    """The item side of an importance weight ll + log_pd - reg - log_qd: (log p(d) at the item sample behind the item flows,
    log q(d) of the sample in front of them minus the flows' log-determinant).  Without flows item_k is item_feat, item_ladj None."""
    log_qd = _normal_logpdf(item_feat, item_mu, item_lv).sum()
    if item_ladj is not None:
        log_qd = log_qd - item_ladj.sum()
    return _std_normal_logpdf(item_k).sum(), log_qd


def _log_mean_exp(log_w):
    """log of the mean of the S weights exp(log_w[s])."""
    return torch.logsumexp(log_w, 0) - math.log(log_w.shape[0])


@dataclasses.dataclass
class _Draws:
    """What log_marginal drew for its S samples, stacked as the multi-sample forward takes it.  eps_item (the caller's [S, I, D]
    or the S tensors drawn), items [S, I, D] behind the item flows, eps_ability [S, B, A], log_pd / log_qd [S]
    (_item_log_terms), flow_packed (the ability flows, or None) and `table` as the backend reads it: the expert table [2, 2A] or,
    conditional posterior, one per sample [S, 2, I, 2A]; given=True: the posterior (mu | logvar) [B, 2A] or one per sample
    [S, B, 2A]."""
    eps_item: object
    items: torch.Tensor
    eps_ability: torch.Tensor
    log_pd: torch.Tensor
    log_qd: torch.Tensor
    table: torch.Tensor
    flow_packed: object
    given: bool

    def posterior(self, s):
        """The given posterior [B, 2A] of sample s for a forward of that sample alone; None where the kernel forms it itself."""
        if not self.given:
            return None
        return self.table[s] if self.table.dim() == 3 else self.table


def _multi_log_weights(spec, response, mask, draws):
    """log w_s [S] of the samples `draws` in one pass over the rows (ops._BACKEND['multi']), or None where the backend does not
    cover the call: the caller then runs one forward per sample on the same draws."""
    response, mask, code = ops.prepare_rows(response, mask)
    sc = ops._BACKEND['multi'](spec, response, mask, code, None, draws.table, draws.items, draws.eps_ability, draws.flow_packed,
                               _lib.REG_SAMPLED, draws.eps_ability.shape[1])
    if sc is None:
        return None
    return sc[:, _lib.S_LL] - sc[:, _lib.S_REG] + draws.log_pd - draws.log_qd
