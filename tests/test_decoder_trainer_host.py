"""FusedDecoderTrainer / vibo_dtrain_* without a GPU: the exported symbols, the flat parameter layout against the models'
state_dict, argument validation (negative codes before any launch), the coverage predicates and the CLI flag."""
import ctypes
import os
import re

import pytest

from decoder_trainer_common import CLS, _args, _model, built_objects, desc, kernel_notes
from vibo_amd import _lib, ops
from vibo_amd.torch_core import vibo as cli
from vibo_amd.trainer import fused_decoder_trainer_covers, fused_trainer_covers

NEW_SYMBOLS = ('vibo_dtrain_param_floats', 'vibo_dtrain_scratch_floats', 'vibo_dtrain_scratch_offset', 'vibo_dtrain_prologue',
               'vibo_dtrain_forward_backward', 'vibo_dtrain_epilogue')


def test_new_symbols_are_exported():
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS
        getattr(lib, name)
    header = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'vibo_hip.h')).read()
    for name in NEW_SYMBOLS:
        assert re.search(r'\b' + name + r'\(', header), name


@pytest.mark.parametrize('kind', ['link', 'deep', 'residual'])
@pytest.mark.parametrize('irt', [1, 2, 3])
@pytest.mark.parametrize('A,H', [(1, 64), (3, 16), (8, 48), (12, 64)])
def test_param_floats_is_the_state_dict_without_the_item_embeddings(kind, irt, A, H):
    """The flat buffer holds every state_dict entry but the two item embeddings (their own tensors, as for the sibling trainers),
    in state_dict order."""
    model = CLS[irt](A, 20, hidden_dim=H, ability_merge='product', generative_model=kind)
    sd = model.state_dict()
    want = sum(v.numel() for k, v in sd.items() if not k.startswith('item_encoder.'))
    assert sum(v.numel() for k, v in sd.items() if k.startswith('item_encoder.')) == 2 * 20 * ops.item_feat_dim(irt, A)
    d = desc(irt, A)
    assert _lib.load().vibo_dtrain_param_floats(ctypes.byref(d), _lib.DECODER_KINDS[kind], H) == want
    keys = [k for k in sd if not k.startswith('item_encoder.')]
    assert keys[:6] == [f'ability_encoder.mlp.{i}.{w}' for i in (0, 2, 4) for w in ('weight', 'bias')]
    assert all(k.startswith('decoder.') for k in keys[6:])


def test_bad_descriptors_are_refused_before_any_launch():
    """No device pointer is valid here (and there may be no GPU at all): the codes come from the host-side checks."""
    lib = _lib.load()
    nul = ctypes.c_void_p(0)

    def prologue(d, kind=2, H=64):
        return lib.vibo_dtrain_prologue(ctypes.byref(d), kind, H, 0, nul, nul, nul, nul, 0, 0, nul, 1, nul, nul, nul, nul)

    def fwd_bwd(d, kind=2, H=64):
        return lib.vibo_dtrain_forward_backward(ctypes.byref(d), kind, H, 0, nul, nul, nul, nul, nul, nul, nul, nul)

    def epilogue(d, kind=2, H=64):
        return lib.vibo_dtrain_epilogue(ctypes.byref(d), kind, H, 0, *([nul] * 15))

    for call in (prologue, fwd_bwd, epilogue):
        assert call(desc(2, 2), H=65) == -6                                   # decoder width above 64
        assert call(desc(2, 2), H=128) == -6
        assert call(desc(2, 2, conditional=True)) == -6                       # conditional posterior
        assert call(desc(2, 2, n_flows=2)) == -6                              # flows
        assert call(desc(2, 2, mask=_lib.MASK_I64)) == -8                     # int64 masks
        assert call(desc(2, 2, I=70000)) == -3                                # the packed row counts
        assert call(desc(2, 2), kind=7) == -3
        assert call(desc(2, 2)) == -5                                         # a good descriptor: the null pointers are next
    assert lib.vibo_dtrain_scratch_floats(ctypes.byref(desc(2, 2)), 2, 65, 0) == 0
    assert lib.vibo_dtrain_scratch_floats(ctypes.byref(desc(2, 2)), 2, 64, 0) > 0
    assert lib.vibo_dtrain_scratch_offset(ctypes.byref(desc(2, 2)), 2, 64, 0, 99) == -1


def test_fused_decoder_trainer_covers_truth_table():
    for gen in ('link', 'deep', 'residual'):
        for irt in (1, 2, 3):
            assert fused_decoder_trainer_covers(_model(gen, irt=irt))
        assert fused_decoder_trainer_covers(_model(gen, H=16)) and fused_decoder_trainer_covers(_model(gen, A=12))
        assert not fused_decoder_trainer_covers(_model(gen, cond=True))
        assert not fused_decoder_trainer_covers(_model(gen, flows=2))
        assert not fused_decoder_trainer_covers(_model(gen, merge='mean'))
        assert not fused_decoder_trainer_covers(_model(gen), hidden_dim=128)
        sharded = _model(gen)
        sharded._reducer = lambda flat: flat
        assert not fused_decoder_trainer_covers(sharded)
    assert not fused_decoder_trainer_covers(_model('irt'))


def test_fused_trainer_covers_is_unchanged():
    assert fused_trainer_covers(_model('irt'))
    assert fused_trainer_covers(_model('irt', cond=True)) and fused_trainer_covers(_model('irt', flows=2))
    assert not fused_trainer_covers(_model('irt', cond=True, H=128))
    assert fused_trainer_covers(_model('irt', merge='mean'))
    assert not fused_trainer_covers(_model('irt', merge='mean', cond=True))
    for gen in ('link', 'deep', 'residual'):
        for kw in ({}, {'cond': True}, {'flows': 2}, {'merge': 'mean'}):
            assert fused_trainer_covers(_model(gen, **kw)) is False


BASE = ['--irt-model', '2pl', '--dataset', '2pl_simulation', '--cuda', '--generative-model', 'deep']


def test_cli_flag_is_parsed_and_off_by_default():
    assert _args(BASE).native_decoder_step is False
    a = _args(BASE + ['--native-decoder-step'])
    assert a.native_decoder_step is True
    cli.check_supported(a)                                       # covered: passes
    for gen in ('link', 'residual'):
        cli.check_supported(_args(['--irt-model', '3pl', '--dataset', '3pl_simulation', '--cuda', '--generative-model', gen,
                                   '--native-decoder-step']))


@pytest.mark.parametrize('extra,needle', [(['--torch-optimizer'], '--torch-optimizer'),
                                          (['--conditional-posterior'], '--conditional-posterior'),
                                          (['--n-norm-flows', '2'], '--n-norm-flows'),
                                          (['--ability-merge', 'mean'], '--ability-merge mean'),
                                          (['--generative-model', 'irt'], '--generative-model irt')])
def test_cli_flag_with_an_uncovered_configuration_says_so(extra, needle):
    with pytest.raises(SystemExit) as e:
        cli.check_supported(_args(BASE + ['--native-decoder-step'] + extra))
    msg = str(e.value)
    assert '--native-decoder-step' in msg and needle in msg and 'torch.optim' in msg


def test_cli_flag_needs_cuda():
    with pytest.raises(SystemExit) as e:
        cli.check_supported(_args([a for a in BASE if a != '--cuda'] + ['--native-decoder-step']))
    assert '--cuda' in str(e.value)


def test_new_unit_carries_no_scratch():
    """csrc/vibo_dtrainer.hip is built without spilled vector registers or private memory: read from the code-object notes of the
    in-tree object, the way test_matrix_kernel_instantiations_carry_no_scratch does; skipped when the build directory or the LLVM
    tools are not there."""
    notes = kernel_notes(built_objects('vibo_dtrainer.o')[0])
    for name, (spill, scratch) in notes.items():
        assert spill == 0 and scratch == 0, (name, spill, scratch)
    assert len(notes) >= 8
