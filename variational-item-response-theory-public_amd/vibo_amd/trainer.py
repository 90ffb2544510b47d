"""Fused train step: the whole `loss = model.elbo(*model(r, m), beta); loss.backward(); adam.step()` of the
reference loop (vibo.py:243-268) as TWO kernel launches instead of ~80.

    trainer = FusedTrainer(model, lr=5e-3)
    loss = trainer.step(response, mask, beta=1.0, row_index=rows)      # device scalar, parameters updated in place

What runs (the folded step, `fold=True` with rng='native', the default of the CLI and the benchmark):
    vibo_elbo_fwd_bwd_step     the fused ELBO forward + backward over the rows (ticks Adam's step counter); on the matrix
                               row-split kernel it draws the ability noise itself (vibo_elbo_fwd_bwd_step_noise) and leaves
                               the posterior's mean / log-variance and the sample unwritten: `trainer.last.ability_mu` /
                               `.ability_logvar` are None there, `.flat` is what it always was, and `trainer.last.ability` is
                               rebuilt when read (_StepSample: two extra launches, the same values bit for bit; valid until the
                               next update(), raises afterwards and under capture) -- nothing is materialised otherwise
    [person-sharded: finalize inside that call, then ONE all-reduce of the flat buffer]
    vibo_train_epilogue_fused  finalize (one GPU), loss, encoder-MLP / item backward, Adam -- and the NEXT step's head: Philox
                               noise, item sample, item KL, the 2-row encoder table from the parameters just updated
                               (the table this step ran on is kept behind it: `trainer.table_prev`)
The step is software-pipelined across its own iterations: when the ELBO kernel starts, everything it reads is in memory.  The
first step's head comes from vibo_fill_normal x 2 + vibo_train_prime ("priming"), repeated whenever the parameters were
changed from outside between two steps (load_state_dict, optimizers, `.copy_`: detected through the tensors' version
counters) or a larger minibatch than ever before arrives.  Writes torch does not count -- through `p.data`, through
`trainer.mlp_flat`, from another native kernel -- are NOT seen: call `trainer.invalidate()` after them (the next step then
re-primes), or build the trainer with fold=False, whose four-launch step recomputes its head from the parameters every time.
A folded forward_backward() has to be followed by update() before the next one (it raises otherwise: the second call would
tick Adam's counter and flip the double-buffered item-KL half under the pending update).  The ability-noise buffer never
moves once a hipGraph may have captured it: size it up front with `max_batch`, a larger minibatch arriving later bumps
`trainer.generation` (GraphedTrainStep re-captures when it changes).  From the first step that draws its own noise on, no
epilogue fills that buffer any more (32 MB written and read back per 1M x 8 step saved); a later step on another kernel (a
short minibatch on the VALU kernel) fills it itself in front of its ELBO launch, and `generation` is bumped once at the switch.
`fold=False`, rng='torch' (noise from torch's generators: not known a step ahead) and shapes the folded step does not cover
(more than 1024 items, int64 masks, unaligned rows) take the four-launch form (vibo_train_prologue[_noise] ->
vibo_elbo_fwd_bwd = kernel + finalize -> vibo_train_epilogue); the two forms agree bit for bit (tests/test_gpu_trainer.py).
Same arithmetic as the PyTorch path (tests/test_gpu_trainer.py compares parameters after several steps); `.grad` fields are not
populated.
One entry point: `FusedTrainer(model, ...)` returns the class that runs the model's step natively -- fused_trainer_for() is the
table: FusedTrainer itself (plain), FusedCondFlowTrainer (vibo_ctrain_*: --conditional-posterior / --n-norm-flows), FusedMeanTrainer
(vibo_mtrain_*: --ability-merge mean), FusedDecoderTrainer (vibo_dtrain_*[_cond]: --generative-model link | deep | residual; the
conditional posterior asked for with `conditional=True`), FusedVITrainer / FusedMLETrainer (vibo_ptrain_*: the un-amortized VI_*PL /
MLE_*PL models, dense Adam over their per-person tables) -- or says why none does: those train through the module + torch.optim.
All share _FusedStep: the state, the noise, and step() = forward_backward() -> reduce_shards() -> update().
"""
import ctypes

import torch

from . import _lib, ops

_MODULE_PATH = 'use model.elbo_step + torch.optim.Adam otherwise'


def fused_trainer_for(model, hidden_dim=None, conditional=False):
    """THE coverage table -> (the trainer class that runs the model's whole train step natively, None), or (None, why none does:
    the constructors' NotImplementedError).  hidden_dim: the encoder's width when the caller knows it (else read from the model);
    conditional: FusedDecoderTrainer was asked for the conditional posterior (conditional=True).  Reads the model's
    generative_model, ability_merge, conditional_posterior, n_norm_flows, ability_dim, num_item and _reducer, nothing else -- but for
    the two un-amortized models (no encoder: a caller-supplied posterior, `spec.given`, and per-person nn.Embedding tables), which
    are known by their embeddings: VI_*PL -> FusedVITrainer, MLE_*PL -> FusedMLETrainer."""
    if getattr(getattr(model, 'spec', None), 'given', False) and not hasattr(model, 'ability_encoder'):
        vi = all(hasattr(model, name) for name in ('ability_mu_lookup', 'ability_logvar_lookup', 'item_mu_lookup', 'item_logvar_lookup'))
        if vi or (hasattr(model, 'ability') and hasattr(model, 'item_feat')):
            cls = FusedVITrainer if vi else FusedMLETrainer
            if model.ability_dim > _lib.MAX_ABILITY_DIM_FAST:
                return None, (f'{cls.__name__}: ability_dim <= {_lib.MAX_ABILITY_DIM_FAST} (the caller-supplied posterior runs on the '
                              f'row-split kernels); {_MODULE_PATH}')
            return cls, None
    kind, merge, A = getattr(model, 'generative_model', 'irt'), model.ability_merge, model.ability_dim
    cond, flows = bool(model.conditional_posterior), model.n_norm_flows > 0

    def hidden():
        if hidden_dim is not None:
            return hidden_dim
        enc = model.ability_encoder
        return (enc.mlp1 if merge == 'mean' else enc.mlp)[0].weight.shape[0]

    if kind in _lib.DECODER_KINDS:
        # product encoder, no flows, one GPU, the packed row counts' 65 535 items, the decoder kernel's width
        why = (f'--ability-merge {merge}' if merge != 'product' else
               'the conditional posterior (unless built with conditional=True)' if cond and not conditional else
               'normalizing flows' if flows else
               'person sharding' if model._reducer is not None else
               'more than 65 535 items (the packed row counts)' if model.num_item > 65535 else
               f'ability_dim above {_lib.MAX_ABILITY_DIM}' if A > _lib.MAX_ABILITY_DIM else None)
        if why is not None:
            return None, f'FusedDecoderTrainer does not cover {why}; use model.elbo_step + torch.optim.Adam'
        if hidden() > 64:
            return None, f"FusedDecoderTrainer: hidden_dim <= 64 (the per-term decoder kernel's width); {_MODULE_PATH}"
        return FusedDecoderTrainer, None
    if kind != 'irt' or merge not in ('product', 'mean'):
        return None, f'the fused trainers cover the product-of-experts encoder with the IRT decoder; {_MODULE_PATH}'
    if merge == 'mean':
        if cond or flows or hidden() > 128 or A > _lib.MAX_ABILITY_DIM_FAST:
            return None, ('FusedMeanTrainer: --ability-merge mean with the unconditional posterior, the IRT decoder, no flows, '
                          f'hidden_dim <= 128, ability_dim <= 8; {_MODULE_PATH}')
        return FusedMeanTrainer, None
    if cond or flows:
        if hidden() > 64:
            return None, f'FusedCondFlowTrainer: hidden_dim <= 64 (one 64-wide tile of the matrix-pipe table MLP); {_MODULE_PATH}'
        if A > _lib.MAX_ABILITY_DIM_FAST:
            return None, f'FusedCondFlowTrainer: ability_dim <= 8 (the row-split kernels of vibo_ctrain_*); {_MODULE_PATH}'
        return FusedCondFlowTrainer, None
    if hidden() > 256:
        return None, f'FusedTrainer: hidden_dim <= 256; {_MODULE_PATH}'
    return FusedTrainer, None


def fused_trainer_covers(model, hidden_dim=None):
    """True when FusedTrainer, FusedCondFlowTrainer, FusedMeanTrainer, FusedVITrainer or FusedMLETrainer runs the model's whole train
    step natively (the IRT decoder)."""
    return fused_trainer_for(model, hidden_dim)[0] not in (None, FusedDecoderTrainer)


def fused_decoder_trainer_covers(model, hidden_dim=None, conditional=False):
    """True when FusedDecoderTrainer(model, conditional=conditional) runs the model's whole train step natively (the MLP decoders)."""
    return fused_trainer_for(model, hidden_dim, conditional)[0] is FusedDecoderTrainer


class _FusedStep:
    """What the trainers share: the state every step reads, the noise, and the step protocol."""

    def __init__(self, model, lr, rng, seed, fold=False, conditional=False, keep_item_noise=True):
        covering, why = fused_trainer_for(model, conditional=conditional)
        if covering is None or not isinstance(self, covering):
            raise NotImplementedError(why or f'{type(self).__name__} does not cover this model ({covering.__name__} does)')
        if rng not in ('torch', 'native'):
            raise ValueError("rng must be 'torch' or 'native'")
        self.model = model
        self.generation = 0                   # bumped when a buffer a captured hipGraph points at was replaced (re-capture then)
        self.fold = bool(fold)                # FusedTrainer: two launches per step (train hook + fused epilogue) where the shape allows
        self._primed_for = None               # folded step: (noise capacity, parameter versions) the next step's head was prepared for
        self._folded_open = False             # a folded forward_backward() whose update() has not run yet
        self._pending = None                  # what forward_backward() leaves for update(): the arguments of the class's _update()
        self.last = None                      # RawElbo of the last step (posterior outputs, scalars)
        enc = getattr(model, 'ability_encoder', None)      # (None: the un-amortized models have no encoder)
        self.hidden = 0 if enc is None else (enc.mlp1 if model.ability_merge == 'mean' else enc.mlp)[0].weight.shape[0]
        # the item tensors and their moments, Adam's counters and scalars, the item sample, the loss
        # (item_lv None: the item table is not variational -- MLE -- and is its own "sample"; its moments are one table's)
        self.item_mu, self.item_lv = self._item_tensors(model)
        variational = self.item_lv is not None
        assert self.item_mu.is_contiguous() and (not variational or self.item_lv.is_contiguous())
        dev, n_item = self.item_mu.device, self.item_mu.numel()
        self.item_m = torch.zeros((2 if variational else 1) * n_item, device=dev)
        self.item_v = torch.zeros((2 if variational else 1) * n_item, device=dev)
        self._steps = torch.zeros(2, dtype=torch.int32, device=dev)      # [Adam step t, completed steps (noise counter)]
        self.lr = torch.tensor(float(lr), device=dev)
        self.beta = torch.tensor(1.0, device=dev)
        self._beta_host = 1.0
        self.item_feat = torch.empty_like(self.item_mu) if variational else self.item_mu
        self.loss = torch.zeros((), device=dev)
        # Reparameterisation noise: 'torch' = torch.randn on the model's generators (the reference's stream for a given seed),
        # 'native' = Philox4x32-10 keyed by `seed` (vibo_fill_normal's streams, ~5x faster on [1M, 8]).
        # (person-sharded: item noise is the same on every rank, ability noise uses stream 1 + rank)
        self.rng, self.seed = rng, int(seed)
        self.fused_noise = True               # rng='native': the noise is drawn inside the prologue launch
        self._eps_item = torch.empty_like(self.item_mu) if keep_item_noise and variational else None
        self._eps_ab = {}

    @staticmethod
    def _item_tensors(model):
        """Where the model keeps its item tensors -> (mean, log-variance)."""
        return model.item_encoder.mu_lookup.weight, model.item_encoder.logvar_lookup.weight

    @staticmethod
    def _flatten(plist):
        """One flat buffer of the parameters in plist's order -- the nn.Parameters become views of it (state_dict unchanged) --
        and Adam's two moments in the same layout."""
        flat = torch.cat([p.detach().reshape(-1) for p in plist]).contiguous()
        off = 0
        for p in plist:
            n = p.numel()
            p.data = flat[off:off + n].view_as(p)
            off += n
        return flat, torch.zeros_like(flat), torch.zeros_like(flat)

    def _check_layout(self, param_floats):
        if param_floats != self.par_flat.numel():
            raise RuntimeError(f'{type(self).__name__}: parameter layout mismatch')

    def _begin(self, response, mask, beta, row_index, reg_mode):
        """What every forward_backward() starts with: the KL weight, the rows as the kernels read them, the descriptor of this
        call.  Returns (response, mask, code, B, I, stream, descriptor, ab_stream)."""
        if beta is not None:
            self.set_beta(beta)
        response, mask, code = ops.prepare_rows(response, mask)
        B = int(row_index.numel()) if row_index is not None else response.shape[0]
        I = response.shape[1]
        stream = ops._stream(response.device)
        d = ops._rows_desc(self.model.spec, B, response, mask, code, reg_mode, True)
        ab_stream = 1 + getattr(self.model, '_shard_rank', 0)      # item noise: the same on every rank; ability noise: per rank
        return response, mask, code, B, I, stream, d, ab_stream

    @staticmethod
    def _resident_step():
        """Keywords of an ELBO launch under a caller-supplied posterior (mean merge, VI, MLE): the HIP launcher is told that this is
        a trainer's step on its resident matrix -- a whole-matrix step may then go out on the matrix' tile image (ops._tile_rows
        decides).  Any other backend (the CPU stand-in, a test's fake) keeps its signature."""
        return {'resident_step': True} if ops._BACKEND['elbo'] is ops._hip_launch_elbo else {}

    def _ab_buffer(self, B, dev):
        # one buffer per batch size, never freed or replaced: a captured hipGraph keeps the pointer it was recorded
        # with, and the epoch's last, shorter minibatch runs eagerly in between the replays
        eps_ab = self._eps_ab.get(B)
        if eps_ab is None:
            eps_ab = self._eps_ab[B] = torch.empty(B, self.model.ability_dim, device=dev)
        return eps_ab

    def _choose_noise(self, B, dev, eps_item, eps_ability):
        """The noise of a step -> (eps_item, eps_ab, native): the caller's (given), this trainer's buffers for the native draws to
        fill (native), or torch's generators in the reference's draw order, item eps then ability eps (models.py:361,368) -- the
        item draw happens here, eps_ab is None and the caller draws it after the prologue (_draw_ability)."""
        if eps_item is not None or eps_ability is not None:
            if eps_item is None or eps_ability is None:
                raise ValueError('pass both eps_item and eps_ability, or neither')
            return eps_item.contiguous().float(), eps_ability.contiguous().float(), False
        if self.rng == 'native':
            return self._eps_item, self._ab_buffer(B, dev), True
        return self.model._randn(self.item_mu.shape, self.item_mu, self.model._item_gen), None, False

    def _draw_ability(self, B):
        return self.model._randn((B, self.model.ability_dim), self.item_mu, self.model._ability_gen)

    def set_beta(self, beta):
        """KL weight (vibo.py:223-230).  A device scalar: update it between graph replays when annealing."""
        if float(beta) != self._beta_host:
            self.beta.fill_(float(beta))
            self._beta_host = float(beta)

    def invalidate(self):
        """Tell the folded step that the parameters were written behind torch's back (`p.data` edits, `trainer.mlp_flat`,
        another kernel): the head the previous epilogue left behind -- item sample, item KL, expert table, saved activations --
        is stale, the next step rebuilds it from the parameters as they are then (vibo_train_prime).  load_state_dict and other
        writes torch counts are detected without this call.  The pending noise draws are repeated for the same step counter.
        Also the way out after a step that died between its two halves (an exception in the all-reduce, a hipGraph capture that
        was aborted after forward_backward() had run on the host): the half-open folded step is forgotten."""
        self._primed_for = None
        self._folded_open = False
        self._pending = None

    reprime = invalidate

    @property
    def step_count(self):
        """Adam's step number (device int32 scalar)."""
        return self._steps[0]

    @torch.no_grad()
    def step(self, response, mask, beta=None, row_index=None, eps_item=None, eps_ability=None):
        """One train step; returns the loss (device scalar).  = forward_backward(); reduce_shards(); update().
        eps_item [I, D] / eps_ability [B, A]: replay given reparameterisation noise instead of drawing it (parity tests against
        the reference's recorded steps; FusedTrainer takes the four-launch form)."""
        self._forward_backward(response, mask, beta, row_index, eps_item, eps_ability)
        self.reduce_shards()
        return self._finish()

    @torch.no_grad()
    def forward_backward(self, response, mask, beta=None, row_index=None, eps_item=None, eps_ability=None):
        """Noise, prologue and the fused ELBO forward+backward of this rank's persons (the class's _forward_backward).  Returns the
        step's outputs (`trainer.last`), whose `.flat` buffer [scalars | grads] a person-sharded caller all-reduces before `update()`.
        (Split from `update()` so that a multi-GPU loop can replay the two halves as hipGraphs around an eager collective.)"""
        return self._forward_backward(response, mask, beta, row_index, eps_item, eps_ability)

    def reduce_shards(self):
        """Person-sharded: ONE all-reduce per step, of the flat buffer [scalars | grads] forward_backward() returned."""
        if self.model._reducer is not None:
            self.model._reducer(self.last.flat)

    @torch.no_grad()
    def update(self):
        """Loss, backward of everything outside the ELBO call and Adam from the (all-reduced) buffers of forward_backward()
        (the class's _update)."""
        return self._finish()

    def _finish(self):
        if self._pending is None:
            raise RuntimeError(f'{type(self).__name__}.update(): no forward_backward() is pending')
        return self._update(*self._pending)


class _StepSample:
    """`trainer.last.ability` of a folded step that drew its own noise: the kernel stored no sample, this rebuilds it when asked
    -- vibo_fill_normal at the step's noise counter, then vibo_elbo_fwd_bwd (the same kernel, given noise) on the step's rows with
    the expert table the step ran on; its `ability` is the step's, bit for bit (tests/test_gpu_step_noise.py, test_gpu_noise.py:
    a given-noise call returns the drawing call's sample; the sample does not depend on the item sample, so today's serves).
    The table is in `trainer.table` until the step's update() has run and in `trainer.table_prev` from then until the next
    update(); the counter is step_count[1], less one once the update has ticked it.  Afterwards -- and while the stream is
    capturing -- the call raises.  An eager step's sample is cached; a step captured into a hipGraph is rebuilt on every read, from
    what the last replay left (read it before an eager step or another graph moves the trainer on: replays are not seen here)."""

    def __init__(self, trainer, rows, B, ab_stream):
        self.trainer, self.rows, self.B, self.ab_stream = trainer, rows, B, ab_stream
        self.flags = ops.DESC_FLAGS           # (the rebuild has to run the kernel the step ran)
        self.captured = rows[0].is_cuda and torch.cuda.is_current_stream_capturing()
        self.sample = None

    def __call__(self):
        if self.sample is not None:
            return self.sample
        tr = self.trainer
        if tr._head_of is self:
            table, ticked = tr.table, 0
        elif tr._kept_of is self:
            table, ticked = tr.table_prev, 1
        else:
            raise RuntimeError('FusedTrainer: this step stored no ability sample (it drew its own noise), and a later step has replaced '
                               'the expert table it would be rebuilt from: read `last.ability` before the next update()')
        response, mask, code, row_index = self.rows
        if response.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError('FusedTrainer: `last.ability` of a step that drew its own noise is rebuilt by two extra launches, which '
                               'do not belong in a captured step: read it after the capture')
        counter = tr._steps[1:2] - 1 if ticked else tr._steps[1:2]
        eps = torch.empty(self.B, tr.model.ability_dim, device=tr.table.device)
        ops._call('vibo_fill_normal', ops._ptr(eps), eps.numel(), tr.seed, ops._ptr(counter), self.ab_stream, ops._stream(eps.device))
        with ops.desc_flags(self.flags):
            sample = ops._BACKEND['elbo'](tr.model.spec, response, mask, code, row_index, table, tr.item_feat, eps, None, _lib.REG_KL,
                                          True, self.B).ability
        if not self.captured:
            self.sample, self.rows = sample, None
        return sample


class FusedTrainer(_FusedStep):
    def __new__(cls, model=None, *args, **kwargs):
        # one entry point: the class the coverage table names is built and returned (not an instance of this one: no second __init__)
        # (model=None: copy / pickle re-create the object through cls.__new__(cls) and fill __dict__ themselves)
        if cls is FusedTrainer and model is not None:
            covering, why = fused_trainer_for(model, conditional=kwargs.get('conditional', False))
            if covering is None:
                raise NotImplementedError(why)
            if covering is not cls:
                return covering(model, *args, **kwargs)
        return super().__new__(cls)

    def __init__(self, model, lr=5e-3, rng='torch', seed=0, fused_noise=True, fold=True, max_batch=None):
        super().__init__(model, lr, rng, seed, fold=fold, keep_item_noise=rng == 'native')
        self._eps_cap = None                  # folded step: the ability-noise buffer [capacity] every step's epilogue refills
        self._eps_keep = []                   # (outgrown buffers stay alive: a captured graph may still write to them)
        self._max_batch = int(max_batch) if max_batch else 0      # persons of the largest minibatch to expect (sizes _eps_cap once)
        self._draw_mode = False               # a folded step drew its own ability noise: epilogues no longer fill _eps_cap
        mlp = model.ability_encoder.mlp
        plist = [mlp[0].weight, mlp[0].bias, mlp[2].weight, mlp[2].bias, mlp[4].weight, mlp[4].bias]
        self.mlp_flat, self.mlp_m, self.mlp_v = self._flatten(plist)      # W0 | b0 | W1 | b1 | W2 | b2
        self._watched = plist + [self.mlp_flat, self.item_mu, self.item_lv]
        dev, n_item = self.item_mu.device, self.item_mu.numel()
        # the expert table, and behind it in the same allocation the one the last folded step ran on (vibo_train_epilogue_fused
        # keeps it there before it writes the next): what a step that stored no sample is rebuilt from (_StepSample)
        self.table, self.table_prev = torch.empty(2, 2, 2 * model.ability_dim, device=dev).unbind(0)
        self._head_of = None                  # the open folded step's _StepSample: `table` is still the table it ran on
        self._kept_of = None                  # the last finished folded step's: `table_prev` is, and step_count[1] - 1 its noise counter
        self.saved_h = torch.empty(4 * self.hidden, device=dev)
        self.kl_parts = torch.empty(2 * ((n_item + 63) // 64), device=dev)      # (two halves: the folded step double-buffers them)
        self.fused_noise = bool(fused_noise)      # rng='native': draw the noise inside the prologue launch (2 launches fewer)

    def _forward_backward(self, response, mask, beta, row_index, eps_item, eps_ability):
        model, lib, p = self.model, _lib.load(), ops._ptr
        response, mask, code, B, I, stream, d, ab_stream = self._begin(response, mask, beta, row_index, _lib.REG_KL)
        given = eps_item is not None or eps_ability is not None      # (given noise: the four-launch form; _choose_noise checks it)
        step_bits = lib.vibo_train_step_supported(ctypes.byref(d)) if (self.fold and self.rng == 'native' and self.fused_noise and not given) else 0
        if step_bits & 1:
            return self._forward_backward_folded(d, step_bits, response, mask, code, row_index, B, ab_stream, stream)
        # ---- the four-launch form ----
        eps_item, eps_ab, native = self._choose_noise(B, response.device, eps_item, eps_ability)
        self._primed_for = None               # (these draws move on without refilling the folded step's buffers)
        self._head_of = None                  # (... and the prologue replaces the table of a folded step left open)
        prologue = (ctypes.byref(d), self.hidden, p(self.mlp_flat), p(self.item_mu), p(self.item_lv), p(eps_item), p(self.item_feat),
                    p(self.table), p(self.saved_h), p(self.kl_parts), p(self._steps))
        if native and self.fused_noise:       # noise drawn inside the prologue launch
            ops._call('vibo_train_prologue_noise', *prologue, self.seed, p(eps_ab), ab_stream, stream)
        else:
            if native:
                noise_step = ctypes.c_void_p(self._steps.data_ptr() + 4)          # completed steps (step_count[1])
                ops._call('vibo_fill_normal', p(eps_item), eps_item.numel(), self.seed, noise_step, 0, stream)
                ops._call('vibo_fill_normal', p(eps_ab), eps_ab.numel(), self.seed, noise_step, ab_stream, stream)
            ops._call('vibo_train_prologue', *prologue, stream)
        if eps_ab is None:
            eps_ab = self._draw_ability(B)
        raw = ops._BACKEND['elbo'](model.spec, response, mask, code, row_index, self.table, self.item_feat, eps_ab, None,
                                   _lib.REG_KL, True, B)
        self._pending = (d, eps_item, raw, None)
        self._folded_open = False             # (a four-launch step replaces whatever was pending)
        self.last = raw
        return raw

    def _param_versions(self):
        # (torch bumps a tensor's version on every in-place write it knows of -- load_state_dict, optimizers, .copy_ -- while
        #  this library's kernels update the same memory without touching it: a change means somebody else wrote)
        return tuple(t._version for t in self._watched)

    def _forward_backward_folded(self, d, step_bits, response, mask, code, row_index, B, ab_stream, stream):
        """The folded step's first launch: vibo_elbo_fwd_bwd_step (+ the stand-alone finalize when an all-reduce follows)."""
        model, spec, lib, p = self.model, self.model.spec, _lib.load(), ops._ptr
        dev = response.device
        A = model.ability_dim
        # The head of a step (noise, item sample, item KL, expert table) is left behind by the previous step's epilogue in
        # buffers that never move (a captured hipGraph keeps their pointers); the ability noise goes into ONE buffer of fixed
        # capacity -- the streams are indexed by element, so a step of fewer persons reads a prefix of the same values a fresh
        # draw would give (the epoch's last, shorter minibatch between two replays).  Before the first step, when a larger
        # batch than ever before arrives, or when somebody else wrote the parameters, the head is (re)built here.
        if self._folded_open:
            raise RuntimeError('FusedTrainer: forward_backward() was called twice without update() in between (the folded step '
                               'ticks Adam\'s counter in its first launch; use fold=False to evaluate gradients without updating)')
        need = B * A
        if self._eps_cap is None or self._eps_cap.numel() < need:
            if self._eps_cap is not None:
                # a hipGraph captured before this moment keeps reading -- and its epilogue refilling -- the old buffer, while
                # eager steps move on with the new one: captured steps have to be re-captured (GraphedTrainStep does, on
                # `generation`); pass max_batch to the constructor to never get here
                self._eps_keep.append(self._eps_cap)
                self.generation += 1
            self._eps_cap = torch.empty(max(need, self._max_batch * A), device=dev)
            self._primed_for = None
        # On the matrix kernel the step draws its ability noise in the kernel (the same Philox values the fill would leave):
        # from then on the epilogues skip the fill, and a step on another kernel fills the buffer itself.  A graph captured
        # before the switch expects the epilogue's fill: re-capture (`generation`).
        draws = bool(lib.vibo_train_step_draws_noise(ctypes.byref(d)))
        if draws and not self._draw_mode:
            self._draw_mode = True
            self.generation += 1
        state = (self._eps_cap.numel(),) + self._param_versions()
        noise_step = ctypes.c_void_p(self._steps.data_ptr() + 4)              # completed steps (step_count[1])
        if self._primed_for != state:
            ops._call('vibo_fill_normal', p(self._eps_item), self._eps_item.numel(), self.seed, noise_step, 0, stream)
            if not self._draw_mode:
                ops._call('vibo_fill_normal', p(self._eps_cap), self._eps_cap.numel(), self.seed, noise_step, ab_stream, stream)
            ops._call('vibo_train_prime', ctypes.byref(d), self.hidden, p(self.mlp_flat), p(self.item_mu), p(self.item_lv), p(self._eps_item),
                      p(self.item_feat), p(self.table), p(self.saved_h), p(self.kl_parts), p(self._steps), stream)
            self._primed_for = state
        eps_item, eps_ab = self._eps_item, self._eps_cap[:need].view(B, A)
        if self._draw_mode and not draws:
            ops._call('vibo_fill_normal', p(eps_ab), need, self.seed, noise_step, ab_stream, stream)
        fused_finalize = bool(step_bits & 2) and model._reducer is None
        # A drawing step stores no sample where the library lets it: `raw.ability` rebuilds it on demand, from the rows this call was handed
        lazy = bool(lib.vibo_train_step_sample_optional(ctypes.byref(d), int(row_index is not None)))
        step = ops.TrainStepCall(self._steps, fused_finalize, (self.seed, ab_stream) if draws else None, no_sample=lazy)
        raw = ops._BACKEND['elbo'](spec, response, mask, code, row_index, self.table, self.item_feat, None if draws else eps_ab, None,
                                   _lib.REG_KL, True, B, train_step=step)
        raw.ability_source = self._head_of = _StepSample(self, (response, mask, code, row_index), B, ab_stream) if lazy else None
        self._pending = (d, eps_item, raw, ab_stream)
        self._folded_open = True
        self.last = raw
        return raw

    def _update(self, d, eps_item, raw, folded_stream):
        p = ops._ptr
        stream = ops._stream(raw.flat.device)
        self._kept_of, self._head_of = raw.ability_source if folded_stream is not None else None, None
        if folded_stream is not None:
            self._folded_open = False
            ops._call('vibo_train_epilogue_fused', ctypes.byref(d), self.hidden, p(raw.workspace), p(raw.flat), p(self.saved_h),
                      p(self.kl_parts), p(eps_item), p(self.beta), p(self.lr), p(self._steps),
                      p(self.mlp_flat), p(self.mlp_m), p(self.mlp_v), p(self.item_mu), p(self.item_lv),
                      p(self.item_m), p(self.item_v), p(self.loss), self.seed, p(self.item_feat),
                      p(self.table), None if self._draw_mode else p(self._eps_cap),
                      0 if self._draw_mode else self._eps_cap.numel(), folded_stream, stream)
            return self.loss
        ops._call('vibo_train_epilogue', ctypes.byref(d), self.hidden, p(raw.flat), p(self.saved_h), p(self.kl_parts),
                  p(eps_item), p(self.beta), p(self.lr), p(self._steps), p(self.mlp_flat),
                  p(self.mlp_m), p(self.mlp_v), p(self.item_mu), p(self.item_lv), p(self.item_m),
                  p(self.item_v), p(self.loss), stream)
        return self.loss


class FusedCondFlowTrainer(_FusedStep):
    """The fused train step for --conditional-posterior and / or --n-norm-flows models (vibo.py:243-268 with
    models.py:337-354, 380-443, 664-710, flows.py:21-66): vibo_ctrain_prologue (item sample, item-side flows, ability-flow
    packing, the encoder MLP on the 2 x I rows [c, item_i] -> expert table; optionally the Philox noise) -> vibo_elbo_fwd_bwd
    -> [one all-reduce when person-sharded] -> vibo_ctrain_epilogue (loss, table-MLP / flow / sample backward, Adam on
    everything).  No PyTorch autograd node: the step replays from a hipGraph like FusedTrainer's.  Same interface
    (`FusedTrainer(model, ...)` returns this class for such models).  Hidden width <= 64."""

    def __init__(self, model, lr=5e-3, rng='torch', seed=0, fused_noise=True, fold=True, max_batch=None):
        # (fold: FusedTrainer's two-launch form; this class's step is prologue / ELBO call / epilogue either way)
        super().__init__(model, lr, rng, seed)
        if not fused_noise:
            raise NotImplementedError('FusedCondFlowTrainer draws the native noise inside vibo_ctrain_prologue (there is no '
                                      'separate vibo_fill_normal form of this step): fused_noise=False is not available')
        mlp = model.ability_encoder.mlp
        plist = [mlp[0].weight, mlp[0].bias, mlp[2].weight, mlp[2].bias, mlp[4].weight, mlp[4].bias]
        F = model.n_norm_flows
        if F > 0:
            for st in (model.ability_norm_flows, model.item_norm_flows):
                for fl in st.flows:
                    plist += [fl.u, fl.w, fl.b]
        self.par_flat, self.par_m, self.par_v = self._flatten(plist)      # (the layout of include/vibo_hip.h: vibo_ctrain_*)
        dev, I, A = self.item_mu.device, self.item_mu.shape[0], model.ability_dim
        self.item_k = torch.empty_like(self.item_mu) if F > 0 else self.item_feat
        self.table = torch.empty((2, I, 2 * A) if model.conditional_posterior else (2, 2 * A), device=dev)
        self.flow_packed = torch.empty(F, 2 * A + 1, device=dev) if F > 0 else None
        self._desc0 = ops._make_desc(model.spec, 1, I, _lib.MASK_NONE, _lib.REG_SAMPLED if F > 0 else _lib.REG_KL, True, I, 0)
        lib = _lib.load()
        self._check_layout(lib.vibo_ctrain_param_floats(ctypes.byref(self._desc0), self.hidden))
        self.scratch = torch.empty(int(lib.vibo_ctrain_scratch_floats(ctypes.byref(self._desc0), self.hidden)), device=dev)

    def _forward_backward(self, response, mask, beta, row_index, eps_item, eps_ability):
        model, spec, p = self.model, self.model.spec, ops._ptr
        reg_mode = _lib.REG_SAMPLED if model.n_norm_flows > 0 else _lib.REG_KL
        response, mask, code, B, I, stream, d, ab_stream = self._begin(response, mask, beta, row_index, reg_mode)
        eps_item, eps_ab, native = self._choose_noise(B, response.device, eps_item, eps_ability)
        ops._call('vibo_ctrain_prologue', ctypes.byref(d), self.hidden, p(self.par_flat), p(self.item_mu), p(self.item_lv),
                  p(eps_item), self.seed, 1 if native else 0, p(eps_ab) if native else None, ab_stream,
                  p(self.item_feat), p(self.item_k), p(self.table), p(self.flow_packed), p(self.scratch),
                  p(self._steps), stream)
        if eps_ab is None:
            eps_ab = self._draw_ability(B)
        raw = ops._BACKEND['elbo'](spec, response, mask, code, row_index, self.table, self.item_k, eps_ab, self.flow_packed,
                                   reg_mode, True, B)
        self._pending = (d, eps_item, raw)
        self.last = raw
        return raw

    def _update(self, d, eps_item, raw):
        p = ops._ptr
        ops._call('vibo_ctrain_epilogue', ctypes.byref(d), self.hidden, p(raw.flat), p(eps_item), p(self.item_feat), p(self.item_k),
                  p(self.beta), p(self.lr), p(self._steps), p(self.par_flat), p(self.par_m), p(self.par_v),
                  p(self.item_mu), p(self.item_lv), p(self.item_m), p(self.item_v), p(self.scratch),
                  p(self.loss), ops._stream(raw.flat.device))
        return self.loss


class FusedMeanTrainer(_FusedStep):
    """The fused train step for --ability-merge mean models with the unconditional posterior (vibo.py:243-268 with
    models.py:584-594, 631-650): vibo_mtrain_prologue (item sample, item KL, the 2-row mlp1 forward and the u, v collapse of
    mlp2[0]; optionally the Philox noise) -> vibo_mean_encoder_forward (per-person posterior from the row counts) ->
    vibo_elbo_fwd_bwd in VIBO_POSTERIOR_GIVEN mode -> vibo_mean_encoder_backward_sets -> vibo_mtrain_epilogue (loss, the
    backward through u, v and mlp1 by hand, Adam on everything).  No PyTorch autograd node: the step replays from a hipGraph
    like FusedTrainer's (eight launches since the GIVEN call reads / writes the posterior itself: DESIGN 3.6).  Same interface (`FusedTrainer(model, ...)` returns this class for such models).
    The packed row counts of the resident matrix are computed once (ops.row_counts keeps them in the matrix's ops.ResidentMatrix record while the same tensors come back, under capture too).
    Person-sharded (round 5): `reduce_shards()` between the two halves all-reduces [scalars | item gradient | encoder gradient sums]
    in one collective; the per-person posterior gradients stay on their rank."""

    def __init__(self, model, lr=5e-3, rng='torch', seed=0, fused_noise=True, fold=True, max_batch=None):
        super().__init__(model, lr, rng, seed)
        enc = model.ability_encoder
        plist = [enc.mlp1[0].weight, enc.mlp1[0].bias, enc.mlp1[2].weight, enc.mlp1[2].bias,
                 enc.mlp2[0].weight, enc.mlp2[0].bias, enc.mlp2[2].weight, enc.mlp2[2].bias]
        self.par_flat, self.par_m, self.par_v = self._flatten(plist)      # (the layout of include/vibo_hip.h: vibo_mtrain_*)
        dev, n_item = self.item_mu.device, self.item_mu.numel()
        I, A, H = self.item_mu.shape[0], model.ability_dim, self.hidden
        self._desc0 = ops._make_desc(model.spec, 1, I, _lib.MASK_NONE, _lib.REG_KL, True, I, 0)
        lib = _lib.load()
        self._check_layout(lib.vibo_mtrain_param_floats(ctypes.byref(self._desc0), H))
        self.uv = torch.empty(2 * H, device=dev)
        self.saved = torch.empty(4 * H, device=dev)
        self.grad_sums = torch.empty(2 * H + 2 * A * H + 2 * A, device=dev)
        self.kl_parts = torch.empty((n_item + 63) // 64, device=dev)
        o = 2 * H + H * H + H + H * H + H
        self._w22 = self.par_flat[o:o + 2 * A * H]
        self._b22 = self.par_flat[o + 2 * A * H:o + 2 * A * H + 2 * A]
        self._parts = {}

    def _forward_backward(self, response, mask, beta, row_index, eps_item, eps_ability):
        model, spec, lib, p = self.model, self.model.spec, _lib.load(), ops._ptr
        counts = ops.row_counts(response, mask)             # packed (n_correct << 16 | n_observed) of every resident row, cached
        if row_index is not None:
            counts = counts[row_index]
        response, mask, code, B, I, stream, d, ab_stream = self._begin(response, mask, beta, row_index, _lib.REG_KL)
        dev = response.device
        A, H = model.ability_dim, self.hidden
        eps_item, eps_ab, native = self._choose_noise(B, dev, eps_item, eps_ability)
        ops._call('vibo_mtrain_prologue', ctypes.byref(d), H, p(self.par_flat), p(self.item_mu), p(self.item_lv), p(eps_item), self.seed,
                  1 if native else 0, p(eps_ab) if native else None, ab_stream, p(self.item_feat), p(self.uv),
                  p(self.saved), p(self.kl_parts), p(self._steps), stream)
        if eps_ab is None:
            eps_ab = self._draw_ability(B)
        post = torch.empty(B, 2 * A, device=dev)
        dm = ops._mean_desc(counts, A)
        ops._call('vibo_mean_encoder_forward', ctypes.byref(dm), H, p(counts), p(self.uv[:H]), p(self.uv[H:]), p(self._w22), p(self._b22),
                  p(post), stream)
        raw = ops._BACKEND['elbo'](spec, response, mask, code, row_index, post, self.item_feat, eps_ab, None, _lib.REG_KL, True, B,
                                   **self._resident_step())
        n_part = lib.vibo_mean_encoder_partials(ctypes.byref(dm))
        parts = self._parts.get(n_part)
        if parts is None:
            parts = self._parts[n_part] = torch.empty(n_part, 2 * H + 2 * A * H + 2 * A, device=dev)
        grad_sets = raw.flat[_lib.NUM_SCALARS:_lib.NUM_SCALARS + 2 * B * 2 * A]
        ops._call('vibo_mean_encoder_backward_sets', ctypes.byref(dm), H, p(counts), p(self.uv[:H]), p(self.uv[H:]), p(self._w22),
                  p(grad_sets), p(self.beta), p(parts), n_part, stream)
        self._pending = (d, eps_item, raw, parts, n_part)
        self.last = raw
        return raw

    @torch.no_grad()
    def reduce_shards(self):
        """Person sharding (round 5): ONE all-reduce per step of [8 scalars | item gradient | the encoder's gradient sums] -- what
        is a sum over persons.  The per-person posterior gradients inside raw.flat (2 x B x 2A: this rank's persons) stay local;
        the per-wave encoder partial records are summed on this rank first (their count depends on the shard size)."""
        model = self.model
        if model._reducer is None:
            return
        d, eps_item, raw, parts, n_part = self._pending
        B, A = raw.ability_mu.shape[0], model.ability_dim
        ns = _lib.NUM_SCALARS
        o = ns + 2 * B * 2 * A                              # item gradient behind the per-person sets
        n_item = self.item_mu.numel()
        psum = parts[:n_part].sum(0, keepdim=True)
        buf = torch.cat([raw.flat[:ns], raw.flat[o:o + n_item], psum.reshape(-1)])
        model._reducer(buf)
        raw.flat[:ns].copy_(buf[:ns])
        raw.flat[o:o + n_item].copy_(buf[ns:ns + n_item])
        psum.copy_(buf[ns + n_item:].view_as(psum))
        self._pending = (d, eps_item, raw, psum, 1)

    def _update(self, d, eps_item, raw, parts, n_part):
        p = ops._ptr
        ops._call('vibo_mtrain_epilogue', ctypes.byref(d), self.hidden, p(raw.flat), p(parts), n_part, p(self.grad_sums), p(self.saved),
                  p(self.kl_parts), p(eps_item), p(self.beta), p(self.lr), p(self._steps), p(self.par_flat),
                  p(self.par_m), p(self.par_v), p(self.item_mu), p(self.item_lv), p(self.item_m), p(self.item_v),
                  p(self.loss), ops._stream(raw.flat.device))
        return self.loss


class _DecoderStep:
    """What a FusedDecoderTrainer step leaves behind (`trainer.last`): flat = [LL, KL_ability, ...] (8 floats), the posterior and
    the ability sample -- views of the step's scratch buffer."""
    __slots__ = ('flat', 'ability_mu', 'ability_logvar', 'ability')

    def __init__(self, flat, ability_mu, ability_logvar, ability):
        self.flat, self.ability_mu, self.ability_logvar, self.ability = flat, ability_mu, ability_logvar, ability

    scalars = property(lambda self: self.flat)


class FusedDecoderTrainer(_FusedStep):
    """The fused train step for --generative-model link | deep | residual (vibo.py:243-268 with models.py:337-443, 596-629,
    769-919): vibo_dtrain_prologue (item sample, item KL, 2-row encoder table, mlp_item_feat and U; optionally the Philox noise) ->
    vibo_dtrain_forward_backward (per chunk of decoder.PERSON_CHUNK persons: product of experts from the packed row counts, ability
    sample, mlp_ability and V, IRT logit; vibo_decoder_fwd_bwd; the backward of all that into fixed-order records) ->
    vibo_dtrain_epilogue (record sums, loss, mlp_item_feat / guess / encoder / item backward, Adam on everything).  No PyTorch
    autograd node and no torch.optim: the step replays from a hipGraph like FusedTrainer's, bitwise reproducible.  Same interface
    (`FusedTrainer(model, ...)` returns this class for such models).  The decoder kernel walks dense fp32 rows: a `row_index`
    minibatch is gathered into a persistent buffer (torch.index_select(out=)), cell codes are unpacked per step.
    Covers the product encoder's unconditional posterior without flows, analytic KL, hidden width <= 64, one GPU.
    conditional=True: the conditional posterior q(ability | responses, items) too (vibo_dtrain_*_cond: the encoder MLP over the
    2 x I rows [c, item_i], the experts' sums as vibo_code_table_sum_forward / _backward on the minibatch's 1-byte cell codes --
    the CellCodes rows themselves, gathered for a `row_index` minibatch, or packed from the dense rows by vibo_pack_codes into a
    persistent buffer -- and the backward of both, in the same three calls).  The default keeps refusing such a model."""

    def __init__(self, model, lr=5e-3, rng='torch', seed=0, fused_noise=True, fold=True, max_batch=None, conditional=False):
        super().__init__(model, lr, rng, seed, conditional=conditional)
        kind = model.generative_model
        self.kind = _lib.DECODER_KINDS[kind]
        self.cond = bool(model.conditional_posterior)
        # the three calls of a step: vibo_dtrain_* / vibo_dtrain_*_cond
        self._prologue, self._fwd_bwd, self._epilogue = ('vibo_dtrain_' + call + ('_cond' if self.cond else '')
                                                         for call in ('prologue', 'forward_backward', 'epilogue'))
        mlp, dec = model.ability_encoder.mlp, model.decoder
        stacks = [dec.link] if kind == 'link' else [dec.mlp_item_feat, dec.mlp_ability, dec.mlp_concat]
        plist = [t for st in [mlp] + stacks for k in (0, 2, 4) for t in (st[k].weight, st[k].bias)]
        self.par_flat, self.par_m, self.par_v = self._flatten(plist)      # (the layout of include/vibo_hip.h: vibo_dtrain_*)
        I = self.item_mu.shape[0]
        self._desc0 = ops._make_desc(model.spec, 1, I, _lib.MASK_NONE, _lib.REG_KL, True, I, 0)
        lib = _lib.load()
        self._check_layout(lib.vibo_dtrain_param_floats(ctypes.byref(self._desc0), self.kind, self.hidden))
        self._scratch = {}                    # (persons, chunk) -> scratch buffer: never freed or replaced (captured graphs point at it)
        self._rows = {}                       # (persons, mask given) -> the gathered minibatch's dense rows: never replaced
        self._codes = {}                      # (persons, source) -> the minibatch's cell codes (conditional posterior): never replaced

    def _dense_rows(self, response, mask, row_index):
        """The minibatch as the decoder kernel reads it: fp32 rows + u8 mask (or None), no autograd node."""
        if isinstance(response, ops.CellCodes):
            if mask is not None:
                raise ValueError('CellCodes rows carry their own missingness: pass mask=None')
            r, m = (response.rows(row_index) if row_index is not None else response).unpack()
            return r, m.view(torch.uint8)
        response = ops.prepare_response(response)
        if mask is not None and mask.dtype == torch.int64:
            raise NotImplementedError('FusedDecoderTrainer reads bool / uint8 masks; use model.elbo_step + torch.optim.Adam for int64 masks')
        mask = ops.prepare_mask(mask)[0]
        if row_index is None:
            return response, mask
        B = int(row_index.numel())
        key = (B, mask is not None)           # one entry per kind of call: a captured graph keeps pointing at its own
        bufs = self._rows.get(key)
        if bufs is None:
            I = response.shape[1]
            bufs = self._rows[key] = (torch.empty(B, I, device=response.device),
                                      None if mask is None else torch.empty(B, I, dtype=torch.uint8, device=response.device))
        torch.index_select(response, 0, row_index, out=bufs[0])
        if mask is not None:
            torch.index_select(mask, 0, row_index, out=bufs[1])
        return bufs

    def _cell_codes(self, response, row_index, r, m, d, stream):
        """The minibatch's 1-byte cell codes (conditional posterior) -> (tensor, row stride): CellCodes rows as they are, gathered
        for a `row_index` minibatch (torch.index_select(out=)), or packed from the dense rows by vibo_pack_codes -- into a buffer
        that is kept per kind of call and never replaced (a captured graph points at it), padding cells 'missing'."""
        B, I = r.shape
        if isinstance(response, ops.CellCodes):
            c = response.codes
            if row_index is None:
                return c, c.stride(0)
            stride = c.stride(0)
            buf = self._codes.get((B, 'gathered'))
            if buf is None:
                buf = self._codes[(B, 'gathered')] = torch.full((B, stride), 2, dtype=torch.uint8, device=c.device)
            torch.index_select(c.as_strided((c.shape[0], stride), (stride, 1)), 0, row_index, out=buf)
            return buf, stride
        stride = (I + 15) // 16 * 16
        buf = self._codes.get((B, 'packed'))
        if buf is None:
            buf = self._codes[(B, 'packed')] = torch.full((B, stride), 2, dtype=torch.uint8, device=r.device)
        ops._call('vibo_pack_codes', ctypes.byref(d), ops._ptr(r), ops._ptr(m), ops._ptr(buf), ctypes.c_int64(stride), stream)
        return buf, stride

    def _forward_backward(self, response, mask, beta, row_index, eps_item, eps_ability):
        from . import decoder
        model, lib, p = self.model, _lib.load(), ops._ptr
        if beta is not None:
            self.set_beta(beta)
        if mask is not None and mask.dtype == torch.int64:
            raise NotImplementedError('FusedDecoderTrainer reads bool / uint8 masks; use model.elbo_step + torch.optim.Adam for int64 masks')
        counts = ops.row_counts(response, mask)             # packed (n_correct << 16 | n_observed) of every resident row, cached
        if row_index is not None:
            counts = counts[row_index]
        r, m = self._dense_rows(response, mask, row_index)
        B, I = r.shape
        dev = r.device
        A, H = model.ability_dim, self.hidden
        stream = ops._stream(dev)
        d = ops._rows_desc(model.spec, B, r, m, _lib.MASK_NONE if m is None else _lib.MASK_U8, _lib.REG_KL, True)
        code_args = ()                                      # conditional posterior: the minibatch's cell codes and their row stride
        if self.cond:
            codes, stride = self._cell_codes(response, row_index, r, m, d, stream)
            code_args = (p(codes), ctypes.c_int64(stride))
        chunk = min(int(decoder.PERSON_CHUNK), B)
        scratch = self._scratch.get((B, chunk))
        if scratch is None:
            n = int(lib.vibo_dtrain_scratch_floats(ctypes.byref(d), self.kind, H, chunk))
            if n <= 0:
                _lib.check(-6, 'vibo_dtrain_scratch_floats')
            scratch = self._scratch[(B, chunk)] = torch.empty(n, device=dev)
            scratch[:_lib.NUM_SCALARS].zero_()
        eps_item, eps_ab, native = self._choose_noise(B, dev, eps_item, eps_ability)
        ops._call(self._prologue, ctypes.byref(d), self.kind, H, chunk, p(self.par_flat), p(self.item_mu), p(self.item_lv),
                  p(eps_item), self.seed, 1 if native else 0, p(eps_ab) if native else None, 1, p(self.item_feat),
                  p(scratch), p(self._steps), stream)
        if eps_ab is None:
            eps_ab = self._draw_ability(B)
        ops._call(self._fwd_bwd, ctypes.byref(d), self.kind, H, chunk, p(self.par_flat), p(r), p(m), p(counts), *code_args, p(eps_ab),
                  p(self.item_feat), p(scratch), stream)
        off = [int(lib.vibo_dtrain_scratch_offset(ctypes.byref(d), self.kind, H, chunk, w))
               for w in (_lib.DTRAIN_SCALARS, _lib.DTRAIN_POSTERIOR, _lib.DTRAIN_ABILITY)]
        post = scratch[off[1]:off[1] + B * 2 * A].view(B, 2 * A)
        self.last = _DecoderStep(scratch[off[0]:off[0] + _lib.NUM_SCALARS], post[:, :A], post[:, A:],
                                 scratch[off[2]:off[2] + B * A].view(B, A))
        self._pending = (d, eps_item, scratch, chunk)
        return self.last

    def reduce_shards(self):
        """Nothing to reduce: this trainer refuses person sharding."""

    def _update(self, d, eps_item, scratch, chunk):
        self._pending = None
        p = ops._ptr
        ops._call(self._epilogue, ctypes.byref(d), self.kind, self.hidden, chunk, p(scratch), p(eps_item), p(self.item_feat),
                  p(self.beta), p(self.lr), p(self._steps), p(self.par_flat), p(self.par_m), p(self.par_v),
                  p(self.item_mu), p(self.item_lv), p(self.item_m), p(self.item_v), p(self.loss), ops._stream(scratch.device))
        return self.loss


class _PersonTableStep(_FusedStep):
    """The fused train step of the two un-amortized methods, whose person side is nn.Embedding tables with one row per person
    (include/vibo_hip_person_tables.h): vibo_ptrain_prologue (Adam's tick, the minibatch's rows gathered into the [B, 2A] posterior
    the ELBO call reads, the inverse map person -> minibatch position; VI: item sample, item KL, optionally the Philox noise) ->
    vibo_elbo_fwd_bwd in VIBO_POSTERIOR_GIVEN mode -> vibo_ptrain_epilogue (loss, item backward + Adam, and Adam over EVERY row of the
    person tables with the minibatch's gradients scattered in: torch.optim.Adam on a dense embedding, not a lazy variant -- rows
    outside the minibatch decay their moments and move on momentum).  No PyTorch autograd node, no torch.optim: with rng='native'
    the step is those three calls and replays from a hipGraph.  The parameters are updated in place in the Embedding weights
    (state_dict unchanged); the tables' moments are `person_m` / `person_v` [tables, P, A].

        step(response, mask, beta=None, row_index=None, eps_item=None, eps_ability=None, index=None)

    index [B] int64 on the trainer's device: the person of every minibatch position; default `row_index` (person = row of the resident
    split), else arange(B).  A person named twice gets the sum of its positions' gradients (embedding backward); an index outside
    the tables is never dereferenced: its position runs on the posterior (0 | 0), its gradient is dropped and `bad_index_count`
    counts it.  Rows: fp32 + bool / uint8 mask, CellCodes, a `row_index` gather from a resident matrix."""
    MODE = None

    def __init__(self, model, lr=5e-3, rng='torch', seed=0, fused_noise=True, fold=True, max_batch=None):
        # (fused_noise / fold / max_batch: FusedTrainer's keywords; this step is prologue / ELBO call / epilogue either way)
        super().__init__(model, lr, rng, seed)
        self.tables = self._person_tables(model)
        P, A = self.tables[0].shape
        dev = self.item_mu.device
        assert all(t.shape == (P, A) and t.is_contiguous() and t.dtype == torch.float32 and t.device == dev for t in self.tables)
        self.num_person = P
        # each table's moments start 16 bytes aligned (the update's vector path): the stride between them is P A rounded up to 4
        n, self._moment_stride = P * A, (P * A + 3) // 4 * 4
        self.person_m, self.person_v = (torch.zeros(len(self.tables), self._moment_stride, device=dev)[:, :n].view(-1, P, A)
                                        for _ in range(2))
        self.slot = torch.full((P,), -1, dtype=torch.int32, device=dev)      # person -> owning minibatch position; all -1 between steps
        self._bad = torch.zeros(1, dtype=torch.int32, device=dev)
        self.kl_parts = torch.empty((self.item_mu.numel() + 63) // 64, device=dev) if self.item_lv is not None else None
        # per batch size, never freed or replaced (a captured hipGraph keeps the pointers): the posterior table, the default index
        self._post, self._arange = {}, {}

    @property
    def bad_index_count(self):
        """Minibatch positions so far whose index was outside the tables (sticky; one device read)."""
        return int(self._bad)

    def invalidate(self):
        """_FusedStep.invalidate, and the inverse map is all -1 again (the way out after a step that died between its two halves)."""
        super().invalidate()
        self.slot.fill_(-1)

    reprime = invalidate

    @torch.no_grad()
    def step(self, response, mask, beta=None, row_index=None, eps_item=None, eps_ability=None, index=None):
        """One train step; returns the loss (device scalar).  = forward_backward(); update()."""
        self._forward_backward(response, mask, beta, row_index, eps_item, eps_ability, index)
        return self._finish()

    @torch.no_grad()
    def forward_backward(self, response, mask, beta=None, row_index=None, eps_item=None, eps_ability=None, index=None):
        return self._forward_backward(response, mask, beta, row_index, eps_item, eps_ability, index)

    def reduce_shards(self):
        """Nothing to reduce: the person tables are not sharded."""

    def _index(self, index, row_index, B, dev):
        """The step's person index, checked on the host before anything is launched."""
        name = type(self).__name__
        if index is None:
            index = row_index
        if index is None:
            if B > self.num_person:
                raise ValueError(f'{name}: {B} rows for tables of {self.num_person} persons: pass `index`')
            index = self._arange.get(B)
            if index is None:
                index = self._arange[B] = torch.arange(B, dtype=torch.int64, device=dev)
            return index
        if index.device != dev:
            raise ValueError(f'{name}: `index` is on {index.device}, the tables are on {dev}')
        if index.dtype != torch.int64:
            raise TypeError(f'{name}: `index` must be int64 (got {index.dtype})')
        if index.numel() != B:
            raise ValueError(f'{name}: `index` names {index.numel()} persons for a minibatch of {B}')
        return index.reshape(-1) if index.is_contiguous() else index.reshape(-1).contiguous()

    def _forward_backward(self, response, mask, beta, row_index, eps_item, eps_ability, index=None):
        name, p = type(self).__name__, ops._ptr
        if mask is not None and mask.dtype == torch.int64:
            raise NotImplementedError(f'{name} reads bool / uint8 masks; use the module step + torch.optim.Adam for int64 masks')
        dev = self.item_mu.device
        B = int(row_index.numel()) if row_index is not None else len(response)
        index = self._index(index, row_index, B, dev)
        if self._pending is not None:         # a forward_backward() whose update() never ran left its claims in the map
            self.slot.fill_(-1)
        # (rows the kernels cannot read in chunks of 4 cells -- a width that is no multiple of 4, not padded -- are copied, as the module path does)
        response, mask, row_index = ops.chunkable_rows(response, mask, row_index)
        response, mask, code, B, I, stream, d, ab_stream = self._begin(response, mask, beta, row_index, _lib.REG_KL)
        A = self.model.ability_dim
        post = self._post.get(B)
        if post is None:
            post = self._post[B] = torch.empty(B, 2 * A, device=dev)
        eps_item, eps_ab, native = self._noise(B, dev, eps_item, eps_ability)
        lv = self.item_lv
        ops._call('vibo_ptrain_prologue', ctypes.byref(d), self.MODE, self.num_person, p(self.tables[0]),
                  p(self.tables[1]) if len(self.tables) > 1 else None, p(index), p(post), p(self.slot), p(self._bad),
                  p(self.item_mu) if lv is not None else None, p(lv), p(eps_item), self.seed, 1 if native else 0,
                  p(eps_ab) if native else None, ab_stream, p(self.item_feat) if lv is not None else None, p(self.kl_parts),
                  p(self._steps), stream)
        if eps_ab is None:                    # rng='torch': the reference's order, item noise then ability noise
            eps_ab = torch.randn(B, A, dtype=torch.float32, device=dev)
        raw = ops._BACKEND['elbo'](self.model.spec, response, mask, code, row_index, post, self.item_feat, eps_ab, None, _lib.REG_KL,
                                   True, B, **self._resident_step())
        self._pending = (d, eps_item, raw, index)
        self.last = raw
        return raw

    def _update(self, d, eps_item, raw, index):
        self._pending = None
        p = ops._ptr
        ops._call('vibo_ptrain_epilogue', ctypes.byref(d), self.MODE, self.num_person, p(raw.flat), p(index), p(self.kl_parts),
                  p(eps_item), p(self.beta), p(self.lr), p(self._steps), p(self.tables[0]),
                  p(self.tables[1]) if len(self.tables) > 1 else None, p(self.person_m), p(self.person_v), self._moment_stride,
                  p(self.slot), p(self.item_mu), p(self.item_lv), p(self.item_m), p(self.item_v), p(self.loss),
                  ops._stream(raw.flat.device))
        return self.loss


class FusedVITrainer(_PersonTableStep):
    """_PersonTableStep for VI_1PL / 2PL / 3PL (vi.py's loop, models.py:100-172): tables ability_mu_lookup / ability_logvar_lookup,
    variational items in item_mu_lookup / item_logvar_lookup.  rng='torch' draws torch.randn_like(item std), then
    torch.randn(B, A), from the default generator -- VI_1PL._run's order, so the same torch.manual_seed gives the module step's
    draws; rng='native' draws both inside the prologue; given eps_item / eps_ability replay recorded noise.
    (`FusedTrainer(vi_model, ...)` returns this class.)"""
    MODE = _lib.PTRAIN_VI

    @staticmethod
    def _item_tensors(model):
        return model.item_mu_lookup.weight, model.item_logvar_lookup.weight

    @staticmethod
    def _person_tables(model):
        return [model.ability_mu_lookup.weight, model.ability_logvar_lookup.weight]

    def _noise(self, B, dev, eps_item, eps_ability):
        """-> (eps_item, eps_ab, native): the caller's; this trainer's buffers for the prologue to fill; or the item draw from
        torch's default generator, eps_ab None (drawn behind the prologue)."""
        if eps_item is not None or eps_ability is not None:
            if eps_item is None or eps_ability is None:
                raise ValueError('pass both eps_item and eps_ability, or neither')
            return eps_item.contiguous().float(), eps_ability.contiguous().float(), False
        if self.rng == 'native':
            return self._eps_item, self._ab_buffer(B, dev), True
        return torch.randn_like(self.item_lv), None, False


class FusedMLETrainer(_PersonTableStep):
    """_PersonTableStep for MLE_1PL / 2PL / 3PL (mle.py's loop, models.py:22-97; MLE_1PL.nll_step's loss, the mean over all
    B x num_item cells of mask x BCE): one table, `ability`; the item table `item_feat` is a plain parameter.  No noise: the ELBO
    call runs on (ability | logvar 0) with a persistent zero eps, so the sample is the point estimate; beta, rng and given noise
    are accepted and not used.  (`FusedTrainer(mle_model, ...)` returns this class.)"""
    MODE = _lib.PTRAIN_MLE

    @staticmethod
    def _item_tensors(model):
        return model.item_feat.weight, None

    @staticmethod
    def _person_tables(model):
        return [model.ability.weight]

    def _noise(self, B, dev, eps_item, eps_ability):
        zero = self._eps_ab.get(B)
        if zero is None:
            zero = self._eps_ab[B] = torch.zeros(B, self.model.ability_dim, device=dev)
        return None, zero, False
