"""What the fused trainers hand to the library, step by step, without a GPU: every native call of two (or three) step() calls by
name, and for each pointer argument the trainer attribute whose memory it is.  The library's launches (ops._call), the ELBO
launch and the row count are replaced by recorders; the host-only exports (vibo_train_step_supported, *_param_floats, ...) are
the real ones.  The expected lists are a characterisation of the code as it is: `python tests/test_trainer_call_sequence.py`
prints them.  Also here: the state and the step protocol every trainer class shares."""
import copy
import ctypes
import pprint

import pytest
import torch

from decoder_trainer_common import CLS, _model
from vibo_amd import _lib, ops
from vibo_amd.trainer import FusedCondFlowTrainer, FusedDecoderTrainer, FusedMeanTrainer, FusedTrainer

PERSONS = 64


def _tensors(value):
    if isinstance(value, torch.Tensor):
        yield value
    elif isinstance(value, dict):
        for v in value.values():
            yield from _tensors(v)
    elif isinstance(value, tuple):
        for v in value:
            yield from _tensors(v)


def owner(trainer, address):
    """Name of the trainer attribute (a tensor, or a dict of the trainer's persistent buffers) whose memory holds `address`: the
    largest such buffer, so a slice is named by the flat buffer it is cut from; the first name in the alphabet among equals;
    '?' for a per-step temporary, 'NULL' for a null pointer."""
    if not address:
        return 'NULL'
    best = None
    for name, value in vars(trainer).items():
        for t in _tensors(value) if name != '_pending' else ():      # (the open step's record owns nothing: it names temporaries too)
            size = t.numel() * t.element_size()
            if t.data_ptr() <= address < t.data_ptr() + size and (best is None or (-size, name) < best):
                best = (-size, name)
    return best[1] if best else '?'


def trace(trainer, monkeypatch, steps):
    """[[(call, (owner of every pointer argument, ...)), ...] per step] of trainer.step(**kwargs) for kwargs in steps."""
    log = []

    def named(args):
        return tuple(owner(trainer, a.value if isinstance(a, ctypes.c_void_p) else None if a is None else a.data_ptr())
                     for a in args if a is None or isinstance(a, (ctypes.c_void_p, torch.Tensor)))

    def call(name, *args):
        log.append((name, named(args)))

    def elbo(spec, response, mask, code, row_index, table, item, eps, flow, reg_mode, want_grad, num_person, train_step=None):
        own_noise = train_step is not None and train_step[2] is not None
        if own_noise:
            assert len(train_step[2]) == 2 and eps is None
        log.append(('elbo' + ('' if train_step is None else '[step+noise]' if own_noise else '[step]'), named((table, item, eps, flow))))
        B, A, I = int(num_person), spec.ability_dim, response.shape[1]
        n_table, n_item, n_flow = table.numel(), I * spec.item_dim, spec.n_flows * (2 * A + 1)
        post = [None if own_noise else torch.zeros(B, A) for _ in range(2)]
        return ops.RawElbo(flat=torch.zeros(_lib.NUM_SCALARS + 2 * n_table + n_item + 2 * n_flow), n_table=n_table, n_item=n_item,
                           n_flow=n_flow, table_shape=tuple(table.shape), ability_mu=post[0], ability_logvar=post[1],
                           ability=torch.zeros(B, A), ability_k=None, ability_ladj=None, workspace=torch.zeros(256, dtype=torch.uint8))

    def counts(response, mask, code, row_index):
        log.append(('counts', ()))
        B, I = (response.shape[0] if row_index is None else int(row_index.numel())), response.shape[1]
        return torch.full((B,), (I // 2) << 16 | I, dtype=torch.int32)

    monkeypatch.setattr(ops, '_call', call)
    monkeypatch.setattr(ops, '_stream', lambda dev: None)
    monkeypatch.setitem(ops._BACKEND, 'elbo', elbo)
    monkeypatch.setitem(ops._BACKEND, 'counts', counts)
    out = []
    for kwargs in steps:
        del log[:]
        trainer.step(**kwargs)
        out.append(list(log))
    return out


def rows(persons, items, seed=0):
    g = torch.Generator().manual_seed(seed)
    return dict(response=(torch.rand(persons, items, generator=g) < 0.5).float(), mask=torch.rand(persons, items, generator=g) < 0.9)


# name -> (model, trainer keyword arguments): 12 items, ability_dim 2, hidden width 64
CASES = {
    'plain native folded': (lambda: _model('irt'), dict(rng='native')),
    'plain native four-launch': (lambda: _model('irt'), dict(rng='native', fold=False)),
    'plain native four-launch separate noise': (lambda: _model('irt'), dict(rng='native', fold=False, fused_noise=False)),
    'plain torch': (lambda: _model('irt'), dict(rng='torch')),
    'conditional native': (lambda: _model('irt', cond=True), dict(rng='native')),
    'flows torch': (lambda: _model('irt', flows=2), dict(rng='torch')),
    'mean merge': (lambda: _model('irt', merge='mean'), dict()),
    'deep decoder': (lambda: _model('deep'), dict()),
    'link decoder conditional': (lambda: _model('link', cond=True), dict(conditional=True)),
}
CLASS_OF = {'plain native folded': FusedTrainer, 'conditional native': FusedCondFlowTrainer, 'mean merge': FusedMeanTrainer,
            'deep decoder': FusedDecoderTrainer, 'link decoder conditional': FusedDecoderTrainer}

PROLOGUE = ('mlp_flat', 'item_mu', 'item_lv', '_eps_item', 'item_feat', 'table', 'saved_h', 'kl_parts', '_steps')
PROLOGUE_TORCH = PROLOGUE[:3] + ('?',) + PROLOGUE[4:]
EPILOGUE = ('?', 'saved_h', 'kl_parts', '_eps_item', 'beta', 'lr', '_steps', 'mlp_flat', 'mlp_m', 'mlp_v', 'item_mu', 'item_lv',
            'item_m', 'item_v', 'loss', 'NULL')
EPILOGUE_TORCH = EPILOGUE[:3] + ('?',) + EPILOGUE[4:]
FUSED = ('?', '?', 'saved_h', 'kl_parts', '_eps_item', 'beta', 'lr', '_steps', 'mlp_flat', 'mlp_m', 'mlp_v', 'item_mu', 'item_lv',
         'item_m', 'item_v', 'loss', 'item_feat', 'table')
EXPECTED = {}      # filled below: name -> [first step, second step(, third step)]


def _expect(name, first, second=None):
    EXPECTED[name] = [first, first if second is None else second]


_folded = [('elbo[step]', ('table', 'item_feat', '_eps_cap', 'NULL')), ('vibo_train_epilogue_fused', FUSED + ('_eps_cap', 'NULL'))]
_expect('plain native folded',
        [('vibo_fill_normal', ('_eps_item', '_steps', 'NULL')), ('vibo_fill_normal', ('_eps_cap', '_steps', 'NULL')),
         ('vibo_train_prime', PROLOGUE + ('NULL',))] + _folded, _folded)
_four = [('elbo', ('table', 'item_feat', '_eps_ab', 'NULL')), ('vibo_train_epilogue', EPILOGUE)]
_expect('plain native four-launch', [('vibo_train_prologue_noise', PROLOGUE + ('_eps_ab', 'NULL'))] + _four)
_expect('plain native four-launch separate noise',
        [('vibo_fill_normal', ('_eps_item', '_steps', 'NULL')), ('vibo_fill_normal', ('_eps_ab', '_steps', 'NULL')),
         ('vibo_train_prologue', PROLOGUE + ('NULL',))] + _four)
_expect('plain torch', [('vibo_train_prologue', PROLOGUE_TORCH + ('NULL',)), ('elbo', ('table', 'item_feat', '?', 'NULL')),
                        ('vibo_train_epilogue', EPILOGUE_TORCH)])
_expect('conditional native',
        [('vibo_ctrain_prologue', ('par_flat', 'item_mu', 'item_lv', '_eps_item', '_eps_ab', 'item_feat', 'item_feat', 'table', 'NULL',
                                   'scratch', '_steps', 'NULL')),
         ('elbo', ('table', 'item_feat', '_eps_ab', 'NULL')),
         ('vibo_ctrain_epilogue', ('?', '_eps_item', 'item_feat', 'item_feat', 'beta', 'lr', '_steps', 'par_flat', 'par_m', 'par_v',
                                   'item_mu', 'item_lv', 'item_m', 'item_v', 'scratch', 'loss', 'NULL'))])
_expect('flows torch',
        [('vibo_ctrain_prologue', ('par_flat', 'item_mu', 'item_lv', '?', 'NULL', 'item_feat', 'item_k', 'table', 'flow_packed',
                                   'scratch', '_steps', 'NULL')),
         ('elbo', ('table', 'item_k', '?', 'flow_packed')),
         ('vibo_ctrain_epilogue', ('?', '?', 'item_feat', 'item_k', 'beta', 'lr', '_steps', 'par_flat', 'par_m', 'par_v',
                                   'item_mu', 'item_lv', 'item_m', 'item_v', 'scratch', 'loss', 'NULL'))])
_mean = [('vibo_mtrain_prologue', ('par_flat', 'item_mu', 'item_lv', '?', 'NULL', 'item_feat', 'uv', 'saved', 'kl_parts', '_steps', 'NULL')),
         ('vibo_mean_encoder_forward', ('?', 'uv', 'uv', 'par_flat', 'par_flat', '?', 'NULL')),
         ('elbo', ('?', 'item_feat', '?', 'NULL')),
         ('vibo_mean_encoder_backward_sets', ('?', 'uv', 'uv', 'par_flat', '?', 'beta', '_parts', 'NULL')),
         ('vibo_mtrain_epilogue', ('?', '_parts', 'grad_sums', 'saved', 'kl_parts', '?', 'beta', 'lr', '_steps', 'par_flat', 'par_m',
                                   'par_v', 'item_mu', 'item_lv', 'item_m', 'item_v', 'loss', 'NULL'))]
_expect('mean merge', [('counts', ())] + _mean, _mean)
_dec_epilogue = ('_scratch', '?', 'item_feat', 'beta', 'lr', '_steps', 'par_flat', 'par_m', 'par_v', 'item_mu', 'item_lv', 'item_m',
                 'item_v', 'loss', 'NULL')
_deep = [('vibo_dtrain_prologue', ('par_flat', 'item_mu', 'item_lv', '?', 'NULL', 'item_feat', '_scratch', '_steps', 'NULL')),
         ('vibo_dtrain_forward_backward', ('par_flat', '?', '?', '?', '?', 'item_feat', '_scratch', 'NULL')),
         ('vibo_dtrain_epilogue', _dec_epilogue)]
_expect('deep decoder', [('counts', ())] + _deep, _deep)
_link = [('vibo_pack_codes', ('?', '?', '_codes', 'NULL')),
         ('vibo_dtrain_prologue_cond', ('par_flat', 'item_mu', 'item_lv', '?', 'NULL', 'item_feat', '_scratch', '_steps', 'NULL')),
         ('vibo_dtrain_forward_backward_cond', ('par_flat', '?', '?', '?', '_codes', '?', 'item_feat', '_scratch', 'NULL')),
         ('vibo_dtrain_epilogue_cond', _dec_epilogue)]
_expect('link decoder conditional', [('counts', ())] + _link, _link)


def build(name):
    torch.manual_seed(0)
    make, kwargs = CASES[name]
    return FusedTrainer(make(), **kwargs)


@pytest.mark.parametrize('name', sorted(CASES))
def test_native_calls_and_their_buffers(name, monkeypatch):
    trainer = build(name)
    got = trace(trainer, monkeypatch, [rows(PERSONS, 12)] * 2)
    assert got == EXPECTED[name]
    assert trainer.generation == 0


def test_the_step_that_draws_its_own_noise(monkeypatch):
    """The bench's shape class -- 2PL, ability_dim 8, 1000 items, 4096 persons: the planner (256 compute units: the library's
    assumption without a device, and the MI355X's) gives it to the matrix row-split kernel, whose folded step draws the ability
    noise itself; a short gathered minibatch then runs on the VALU kernel and fills the buffer in front of its launch."""
    torch.manual_seed(0)
    trainer = FusedTrainer(CLS[2](8, 1000, hidden_dim=64, ability_merge='product'), rng='native')
    data = rows(4096, 1000)
    got = trace(trainer, monkeypatch, [data, data, dict(data, row_index=torch.arange(16))])
    step = [('elbo[step+noise]', ('table', 'item_feat', 'NULL', 'NULL')), ('vibo_train_epilogue_fused', FUSED + ('NULL', 'NULL'))]
    assert got[0] == [('vibo_fill_normal', ('_eps_item', '_steps', 'NULL')), ('vibo_train_prime', PROLOGUE + ('NULL',))] + step
    assert got[1] == step
    assert got[2] == [('vibo_fill_normal', ('_eps_cap', '_steps', 'NULL')), ('elbo[step]', ('table', 'item_feat', '_eps_cap', 'NULL')),
                      step[1]]
    assert trainer.generation == 1


# every field the shared base declares: the state the inherited methods read
BASE_FIELDS = ('model', 'generation', 'fold', 'hidden', '_primed_for', '_folded_open', '_pending', 'last', 'item_mu', 'item_lv',
               'item_m', 'item_v', '_steps', 'lr', 'beta', 'item_feat', 'loss', 'rng', 'seed', '_eps_item', '_eps_ab')


@pytest.mark.parametrize('name', sorted(CLASS_OF))
def test_every_class_has_the_shared_state_and_protocol(name):
    trainer = build(name)
    assert type(trainer) is CLASS_OF[name]
    missing = [f for f in BASE_FIELDS if not hasattr(trainer, f)]
    assert not missing, missing
    assert trainer.generation == 0 and trainer._pending is None and trainer.last is None and not trainer._folded_open
    with pytest.raises(RuntimeError, match=type(trainer).__name__ + r'\.update\(\): no forward_backward\(\) is pending'):
        trainer.update()
    trainer.invalidate()
    with pytest.raises(RuntimeError):
        trainer.update()
    twin = copy.copy(trainer)
    assert type(twin) is type(trainer) and vars(twin).keys() == vars(trainer).keys()
    assert all(getattr(twin, f) is getattr(trainer, f) for f in ('model', 'item_mu', '_steps', 'loss'))
    assert int(trainer.step_count) == 0


if __name__ == '__main__':
    mp = pytest.MonkeyPatch()
    for case in sorted(CASES):
        print(case)
        pprint.pprint(trace(build(case), mp, [rows(PERSONS, 12)] * 2), width=160)
    mp.undo()
