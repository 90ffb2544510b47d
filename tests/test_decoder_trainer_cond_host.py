"""FusedDecoderTrainer(conditional=True) / vibo_dtrain_*_cond without a GPU: the exported symbols, the flat parameter layout of a
conditional descriptor against the models' state_dict, argument validation (negative codes before any launch), the scratch size,
the coverage predicates, the CLI flag and the new kernels' code-object notes."""
import ctypes
import functools
import os
import re

import pytest

import decoder_trainer_common as common
from decoder_trainer_common import CLS, _args, built_objects, kernel_notes
from vibo_amd import _lib, ops
from vibo_amd.torch_core import vibo as cli
from vibo_amd.trainer import fused_decoder_trainer_covers

desc = functools.partial(common.desc, conditional=True)          # (this file's descriptors and models: the conditional posterior's)
_model = functools.partial(common._model, cond=True)
NEW_SYMBOLS = ('vibo_dtrain_prologue_cond', 'vibo_dtrain_forward_backward_cond', 'vibo_dtrain_epilogue_cond')
COND_KERNELS = ('dt_prologue_cond_kernel', 'dt_table_fwd_kernel', 'dt_person_fwd_cond_kernel', 'dt_person_bwd_cond_kernel',
                'dt_table_bwd_kernel', 'dt_epilogue_cond_kernel')


def test_new_symbols_are_exported():
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'vibo_hip.h')).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS
        getattr(lib, name)
        assert re.search(r'\b' + name + r'\(', header), name


@pytest.mark.parametrize('kind', ['link', 'deep', 'residual'])
@pytest.mark.parametrize('irt', [1, 2, 3])
@pytest.mark.parametrize('A,H', [(1, 64), (3, 16), (8, 48), (12, 64)])
def test_param_floats_of_a_conditional_descriptor_is_the_state_dict_without_the_item_embeddings(kind, irt, A, H):
    """The encoder comes first with W0 [H][1 + D]; everything behind it as for the unconditional posterior."""
    model = CLS[irt](A, 20, hidden_dim=H, ability_merge='product', generative_model=kind, conditional_posterior=True)
    sd = model.state_dict()
    D = ops.item_feat_dim(irt, A)
    assert tuple(sd['ability_encoder.mlp.0.weight'].shape) == (H, 1 + D)
    want = sum(v.numel() for k, v in sd.items() if not k.startswith('item_encoder.'))
    lib = _lib.load()
    got = lib.vibo_dtrain_param_floats(ctypes.byref(desc(irt, A)), _lib.DECODER_KINDS[kind], H)
    assert got == want
    assert got - lib.vibo_dtrain_param_floats(ctypes.byref(desc(irt, A, conditional=False)), _lib.DECODER_KINDS[kind], H) == H * D
    keys = [k for k in sd if not k.startswith('item_encoder.')]
    assert keys[:6] == [f'ability_encoder.mlp.{i}.{w}' for i in (0, 2, 4) for w in ('weight', 'bias')]


def test_bad_descriptors_are_refused_before_any_launch():
    """No device pointer is valid here (and there may be no GPU at all): the codes come from the host-side checks."""
    lib = _lib.load()
    nul = ctypes.c_void_p(0)

    def prologue(d, kind=2, H=64):
        return lib.vibo_dtrain_prologue_cond(ctypes.byref(d), kind, H, 0, nul, nul, nul, nul, 0, 0, nul, 1, nul, nul, nul, nul)

    def fwd_bwd(d, kind=2, H=64):
        return lib.vibo_dtrain_forward_backward_cond(ctypes.byref(d), kind, H, 0, nul, nul, nul, nul, nul, 20, nul, nul, nul, nul)

    def epilogue(d, kind=2, H=64):
        return lib.vibo_dtrain_epilogue_cond(ctypes.byref(d), kind, H, 0, *([nul] * 15))

    for call in (prologue, fwd_bwd, epilogue):
        assert call(desc(2, 2), H=65) == -6                                   # decoder width above 64
        assert call(desc(2, 2, n_flows=2)) == -6                              # flows
        assert call(desc(2, 2, conditional=False)) == -6                      # the unconditional posterior has its own calls
        assert call(desc(2, 2, mask=_lib.MASK_I64)) == -8                     # int64 masks
        assert call(desc(2, 2, I=70000)) == -3                                # the packed row counts
        assert call(desc(2, 17)) == -3                                        # ability_dim above 16
        assert call(desc(2, 2), kind=7) == -3
        assert call(desc(2, 2)) == -5                                         # a good descriptor: the null pointers are next
    for A in (1, 8, 16):
        assert prologue(desc(3, A)) == -5
    mean = ops._make_desc(ops.ElboSpec(irt_model=2, ability_dim=2, given=True), 16, 20, _lib.MASK_U8, _lib.REG_KL, True, 20, 20)
    for call in (prologue, fwd_bwd, epilogue):
        assert call(mean) == -6                                               # mean merge: VIBO_POSTERIOR_GIVEN
    assert lib.vibo_dtrain_scratch_floats(ctypes.byref(desc(2, 2)), 2, 65, 0) == 0
    assert lib.vibo_dtrain_scratch_floats(ctypes.byref(desc(2, 2, n_flows=2)), 2, 64, 0) == 0
    assert lib.vibo_dtrain_scratch_offset(ctypes.byref(desc(2, 2)), 2, 64, 0, 99) == -1


@pytest.mark.parametrize('kind', [1, 2, 3])
@pytest.mark.parametrize('irt,A,I,B,chunk', [(2, 2, 20, 16, 0), (3, 12, 95, 77, 26), (1, 1, 200, 33, 0)])
def test_scratch_grows_for_the_conditional_descriptor_and_keeps_the_unconditional_prefix(kind, irt, A, I, B, chunk):
    lib = _lib.load()
    c, u = desc(irt, A, I=I, B=B), desc(irt, A, I=I, B=B, conditional=False)
    nc, nu = (lib.vibo_dtrain_scratch_floats(ctypes.byref(d), kind, 48, chunk) for d in (c, u))
    # at least: the input rows, three activation sets, the feature, its gradient, two backward buffers over the 2 I table rows and
    # the sums and their gradient over the B persons, 64 wide
    assert nc >= nu + 2 * I * 64 * 7 + 2 * B * 64 > nu > 0
    for which in (_lib.DTRAIN_SCALARS, _lib.DTRAIN_POSTERIOR, _lib.DTRAIN_ABILITY):
        oc, ou = (lib.vibo_dtrain_scratch_offset(ctypes.byref(d), kind, 48, chunk, which) for d in (c, u))
        assert oc == ou >= 0


def test_coverage_of_the_conditional_posterior_is_asked_for():
    for gen in ('link', 'deep', 'residual'):
        for irt in (1, 2, 3):
            assert fused_decoder_trainer_covers(_model(gen, irt=irt), conditional=True)
            assert not fused_decoder_trainer_covers(_model(gen, irt=irt))
        assert fused_decoder_trainer_covers(_model(gen, H=16), conditional=True)
        assert fused_decoder_trainer_covers(_model(gen, A=12), conditional=True)
        assert fused_decoder_trainer_covers(_model(gen, cond=False), conditional=True)
        assert not fused_decoder_trainer_covers(_model(gen, flows=2), conditional=True)
        assert not fused_decoder_trainer_covers(_model(gen, merge='mean'), conditional=True)
        assert not fused_decoder_trainer_covers(_model(gen), hidden_dim=128, conditional=True)
        sharded = _model(gen)
        sharded._reducer = lambda flat: flat
        assert not fused_decoder_trainer_covers(sharded, conditional=True)
    assert not fused_decoder_trainer_covers(_model('irt'), conditional=True)


BASE = ['--irt-model', '2pl', '--dataset', '2pl_simulation', '--cuda', '--generative-model', 'deep', '--native-decoder-step',
        '--conditional-posterior']


def test_cli_flag_for_the_native_conditional_step():
    assert _args(BASE).native_conditional_step is False
    with pytest.raises(SystemExit) as e:
        cli.check_supported(_args(BASE))
    assert '--native-conditional-step' in str(e.value)                        # the refusal names the way in
    cli.check_supported(_args(BASE + ['--native-conditional-step']))
    for gen in ('link', 'residual'):
        cli.check_supported(_args(['--irt-model', '3pl', '--dataset', '3pl_simulation', '--cuda', '--generative-model', gen,
                                   '--native-decoder-step', '--conditional-posterior', '--native-conditional-step']))
    for extra, needle in ((['--n-norm-flows', '2'], '--n-norm-flows'), (['--ability-merge', 'mean'], '--ability-merge mean')):
        with pytest.raises(SystemExit) as e:
            cli.check_supported(_args(BASE + ['--native-conditional-step'] + extra))
        assert needle in str(e.value) and 'torch.optim' in str(e.value)


def test_new_kernels_carry_no_scratch():
    """The conditional kernels of csrc/vibo_dtrainer.hip are built without spilled vector registers or private memory: read from
    the code-object notes of the in-tree object, the way test_new_unit_carries_no_scratch does; skipped when the build directory
    or the LLVM tools are not there."""
    notes = kernel_notes(built_objects('vibo_dtrainer.o')[0])
    for name, (spill, scratch) in notes.items():
        assert spill == 0 and scratch == 0, (name, spill, scratch)
    assert {k for k in COND_KERNELS for name in notes if k in name} == set(COND_KERNELS)
