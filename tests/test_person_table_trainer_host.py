"""The native VI / MLE train step (include/vibo_hip_person_tables.h, trainer.FusedVITrainer / FusedMLETrainer) without a GPU: the
binding, what the entry points' validation answers, the coverage table, every native call of a step by name with the owner of each
pointer argument (recorders as in test_trainer_call_sequence.py), the host-side validation, the CLI flags, and the admission of
the GPU tests' inputs (person_table_common.py)."""
import ctypes
import os
import subprocess

import pytest
import torch

import person_table_common as pt
from decoder_trainer_common import _model
from vibo_amd import _lib, ops
from vibo_amd.torch_core import mle as mle_cli
from vibo_amd.torch_core import vi as vi_cli
from vibo_amd.trainer import (FusedCondFlowTrainer, FusedDecoderTrainer, FusedMeanTrainer, FusedMLETrainer, FusedTrainer, FusedVITrainer,
                              fused_trainer_covers, fused_trainer_for)

SYMBOLS = ('vibo_ptrain_prologue', 'vibo_ptrain_epilogue', 'vibo_person_table_adam')


def desc(B=16, I=100, A=2, irt=2, mask=_lib.MASK_U8, posterior=_lib.POSTERIOR_GIVEN, n_flows=0):
    d = _lib.ViboDesc()
    d.abi_version, d.num_person, d.num_item, d.ability_dim, d.irt_model = _lib.ABI_VERSION, B, I, A, irt
    d.posterior, d.missing_mode, d.mask_dtype, d.reg_mode, d.n_flows = posterior, _lib.MISSING_PRIOR, mask, _lib.REG_KL, n_flows
    d.want_grad, d.deterministic, d.response_row_stride, d.mask_row_stride = 1, 1, I, 0 if mask == _lib.MASK_SIGN else I
    return d


# ---------------------------------------------------------------------------
# binding
# ---------------------------------------------------------------------------
def test_the_header_is_bound_and_the_other_lists_are_what_they_were():
    assert 'vibo_hip_person_tables.h' in _lib.EXTRA_HEADERS
    assert _lib.PERSON_TABLE_SYMBOLS == SYMBOLS
    assert set(SYMBOLS) <= {name for name, _, _ in _lib.EXTRA_PROTOTYPES}
    assert not set(SYMBOLS) & set(_lib.EXPORTED_SYMBOLS) and len(_lib.EXPORTED_SYMBOLS) == 59
    assert not set(SYMBOLS) & (set(_lib.EXTRA_SYMBOLS) | set(_lib.SIGN_ROWS_SYMBOLS))
    lib = _lib.load()
    for name in SYMBOLS:
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and fn.argtypes[0] is ctypes.POINTER(_lib.ViboDesc), name
    with open(os.path.join(os.path.dirname(_lib.HEADER_PATH), 'vibo_hip_person_tables.h')) as f:
        text = f.read()
    assert f'#define VIBO_PTRAIN_VI {_lib.PTRAIN_VI}\n' in text and f'#define VIBO_PTRAIN_MLE {_lib.PTRAIN_MLE}\n' in text
    assert f'#define VIBO_PTRAIN_MAX_BLOCKS {_lib.PTRAIN_MAX_BLOCKS}\n' in text
    assert (FusedVITrainer.MODE, FusedMLETrainer.MODE) == (_lib.PTRAIN_VI, _lib.PTRAIN_MLE)


def test_the_built_library_exports_the_symbols():
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(SYMBOLS) <= exported


# ---------------------------------------------------------------------------
# entry-point checks: decided before anything is launched
# ---------------------------------------------------------------------------
def _null_call(fn, d, mode=_lib.PTRAIN_VI, rows=64):
    """mode and table_rows as given, every pointer NULL, the other integers 64."""
    args = [mode, rows]
    for t in fn.argtypes[3:]:
        args.append(None if t is ctypes.c_void_p else 64)
    return fn(ctypes.byref(d), *args)


@pytest.mark.parametrize('name', SYMBOLS)
def test_entry_points_validate_without_a_gpu(name):
    fn = getattr(_lib.load(), name)
    for mode in (_lib.PTRAIN_VI, _lib.PTRAIN_MLE):
        assert _null_call(fn, desc(), mode) == -5                                        # NULL pointers
        assert _null_call(fn, desc(mask=_lib.MASK_SIGN, posterior=_lib.POSTERIOR_UNCONDITIONAL), mode) == -8
        assert _null_call(fn, desc(mask=_lib.MASK_SIGN), mode) == -8
        assert _null_call(fn, desc(posterior=_lib.POSTERIOR_UNCONDITIONAL), mode) == -6     # not a caller-supplied posterior
        assert _null_call(fn, desc(n_flows=2), mode) == -6
        assert _null_call(fn, desc(A=9), mode) == -3                                     # ability_dim <= VIBO_MAX_ABILITY_DIM
        assert _null_call(fn, desc(), mode, rows=0) == -3
    assert _null_call(fn, desc(), mode=2) == -6
    d = desc()
    d.abi_version = 1
    assert _null_call(fn, d) == -2


# ---------------------------------------------------------------------------
# coverage
# ---------------------------------------------------------------------------
def _vi(irt=2, A=2, P=40, I=12):
    return pt.VI_CLS[irt](A, P, I)


def _mle(irt=2, A=2, P=40, I=12):
    return pt.MLE_CLS[irt](A, P, I)


def test_the_coverage_table_names_the_two_trainers_and_keeps_its_old_answers():
    for irt in (1, 2, 3):
        assert fused_trainer_for(_vi(irt)) == (FusedVITrainer, None)
        assert fused_trainer_for(_mle(irt)) == (FusedMLETrainer, None)
        assert fused_trainer_covers(_vi(irt)) and fused_trainer_covers(_mle(irt))
    assert type(FusedTrainer(_vi())) is FusedVITrainer and type(FusedTrainer(_mle())) is FusedMLETrainer
    cls, why = fused_trainer_for(_vi(A=9))
    assert cls is None and 'ability_dim <= 8' in why
    with pytest.raises(NotImplementedError, match='ability_dim <= 8'):
        FusedTrainer(_mle(A=9))
    with pytest.raises(NotImplementedError, match='FusedVITrainer does'):
        FusedMLETrainer(_vi())
    # the models the existing tests build
    old = {FusedTrainer: _model('irt'), FusedCondFlowTrainer: _model('irt', cond=True), FusedMeanTrainer: _model('irt', merge='mean'),
           FusedDecoderTrainer: _model('deep')}
    for cls, model in old.items():
        assert fused_trainer_for(model) == (cls, None)
    assert fused_trainer_for(_model('irt', flows=2))[0] is FusedCondFlowTrainer
    assert fused_trainer_for(_model('link', cond=True))[0] is None and fused_trainer_for(_model('link', cond=True), conditional=True)[0] is FusedDecoderTrainer
    assert fused_trainer_for(_model('irt', merge='mean', cond=True))[0] is None
    with pytest.raises(ValueError, match="rng must be 'torch' or 'native'"):
        FusedTrainer(_vi(), rng='philox')


def test_state_the_trainers_keep():
    torch.manual_seed(0)
    vi, mle = _vi(A=3, P=7), _mle(A=3, P=7)
    keys = list(vi.state_dict()), list(mle.state_dict())
    tv, tm = FusedTrainer(vi, rng='native'), FusedTrainer(mle)
    assert (list(vi.state_dict()), list(mle.state_dict())) == keys
    assert tv.person_m.shape == tv.person_v.shape == (2, 7, 3) and tm.person_m.shape == (1, 7, 3)
    assert tv.person_m.data_ptr() % 16 == 0 and tv.person_m[1].data_ptr() % 16 == 0          # 21 entries per table: the stride is 24
    assert tv.tables[0] is vi.ability_mu_lookup.weight and tv.tables[1] is vi.ability_logvar_lookup.weight
    assert tm.tables[0] is mle.ability.weight and tm.item_mu is mle.item_feat.weight and tm.item_lv is None and tm.item_feat is tm.item_mu
    assert tv.item_m.numel() == 2 * tv.item_mu.numel() and tm.item_m.numel() == tm.item_mu.numel()
    for tr in (tv, tm):
        assert tr.slot.dtype == torch.int32 and tr.slot.shape == (7,) and bool((tr.slot == -1).all())
        assert tr.bad_index_count == 0 and int(tr.step_count) == 0
        slot = tr.slot
        tr.slot[3] = 5
        tr.invalidate()
        assert tr.slot is slot and bool((tr.slot == -1).all())
        with pytest.raises(RuntimeError, match=type(tr).__name__ + r'\.update\(\): no forward_backward\(\) is pending'):
            tr.update()


# ---------------------------------------------------------------------------
# call sequence
# ---------------------------------------------------------------------------
def _tensors(value):
    if isinstance(value, torch.Tensor):
        yield value
    elif isinstance(value, dict):
        for v in value.values():
            yield from _tensors(v)
    elif isinstance(value, (tuple, list)):
        for v in value:
            yield from _tensors(v)


def owner(trainer, address):
    """Name of the trainer attribute whose memory holds `address` (the largest, then the first in the alphabet); '?' for a
    temporary or a caller's tensor, 'NULL' for a null pointer."""
    if not address:
        return 'NULL'
    best = None
    for name, value in vars(trainer).items():
        for t in _tensors(value) if name not in ('_pending', 'last') else ():
            size = max(1, t.numel()) * t.element_size()
            if t.data_ptr() <= address < t.data_ptr() + size and (best is None or (-size, name) < best):
                best = (-size, name)
    return best[1] if best else '?'


def trace(trainer, monkeypatch, steps):
    log = []

    def named(args):
        return tuple(owner(trainer, a.value if isinstance(a, ctypes.c_void_p) else None if a is None else a.data_ptr())
                     for a in args if a is None or isinstance(a, (ctypes.c_void_p, torch.Tensor)))

    def call(name, *args):
        log.append((name, named(args)))

    def elbo(spec, response, mask, code, row_index, table, item, eps, flow, reg_mode, want_grad, num_person, train_step=None):
        assert train_step is None and spec.given and reg_mode == _lib.REG_KL and want_grad
        log.append(('elbo', named((row_index, table, item, eps, flow))))
        B, A, I = int(num_person), spec.ability_dim, response.shape[1]
        assert tuple(table.shape) == (B, 2 * A)
        n_table, n_item = table.numel(), I * spec.item_dim
        return ops.RawElbo(flat=torch.zeros(_lib.NUM_SCALARS + 2 * n_table + n_item), n_table=n_table, n_item=n_item, n_flow=0,
                           table_shape=tuple(table.shape), ability_mu=torch.zeros(B, A), ability_logvar=torch.zeros(B, A),
                           ability=torch.zeros(B, A), ability_k=None, ability_ladj=None)

    monkeypatch.setattr(ops, '_call', call)
    monkeypatch.setattr(ops, '_stream', lambda dev: None)
    monkeypatch.setitem(ops._BACKEND, 'elbo', elbo)
    out = []
    for kwargs in steps:
        del log[:]
        trainer.step(**kwargs)
        out.append(list(log))
    return out, log


def rows(persons, items, seed=0):
    g = torch.Generator().manual_seed(seed)
    return dict(response=(torch.rand(persons, items, generator=g) < 0.5).float(), mask=torch.rand(persons, items, generator=g) < 0.9)


VI_PROLOGUE = ('tables', 'tables', '?', '_post', 'slot', '_bad', 'item_mu', 'item_lv', '_eps_item', '_eps_ab', 'item_feat', 'kl_parts',
               '_steps', 'NULL')
VI_EPILOGUE = ('?', '?', 'kl_parts', '_eps_item', 'beta', 'lr', '_steps', 'tables', 'tables', 'person_m', 'person_v', 'slot', 'item_mu',
               'item_lv', 'item_m', 'item_v', 'loss', 'NULL')


def test_a_native_rng_vi_step_is_prologue_elbo_epilogue(monkeypatch):
    torch.manual_seed(0)
    trainer = FusedTrainer(_vi(), rng='native')
    data = rows(40, 12)
    where = torch.arange(16) * 2
    got, _ = trace(trainer, monkeypatch, [dict(data, row_index=where), dict(data, row_index=where), dict(rows(16, 12))])
    step = [('vibo_ptrain_prologue', VI_PROLOGUE), ('elbo', ('?', '_post', 'item_feat', '_eps_ab', 'NULL')), ('vibo_ptrain_epilogue', VI_EPILOGUE)]
    assert got[0] == step and got[1] == step
    # no row_index, no index: the persistent arange is the index
    own = [(step[0][0], VI_PROLOGUE[:2] + ('_arange',) + VI_PROLOGUE[3:]), ('elbo', ('NULL',) + step[1][1][1:]),
           (step[2][0], VI_EPILOGUE[:1] + ('_arange',) + VI_EPILOGUE[2:])]
    assert got[2] == own
    assert trainer.generation == 0 and len(trainer._post) == 1 and len(trainer._eps_ab) == 1


def test_a_torch_rng_vi_step_draws_item_noise_then_ability_noise(monkeypatch):
    torch.manual_seed(0)
    model = _vi()
    trainer = FusedTrainer(model)
    seen = []
    trace(trainer, monkeypatch, [])
    recorder = ops._BACKEND['elbo']
    monkeypatch.setitem(ops._BACKEND, 'elbo', lambda *a, **k: (seen.append(a[7]), recorder(*a, **k))[1])
    torch.manual_seed(7)
    want_item = torch.randn_like(torch.exp(0.5 * model.item_logvar_lookup.weight))      # VI_1PL._run: item noise first
    want_ab = torch.randn(16, 2)
    torch.manual_seed(7)
    trainer.forward_backward(**rows(16, 12))
    assert torch.equal(seen[0], want_ab) and torch.equal(trainer._pending[1], want_item)


def test_an_mle_step_is_prologue_elbo_epilogue(monkeypatch):
    torch.manual_seed(0)
    trainer = FusedTrainer(_mle(), rng='native')
    data = rows(40, 12)
    where = torch.arange(16) * 2
    got, _ = trace(trainer, monkeypatch, [dict(data, row_index=where)] * 2)
    step = [('vibo_ptrain_prologue', ('tables', 'NULL', '?', '_post', 'slot', '_bad', 'NULL', 'NULL', 'NULL', 'NULL', 'NULL', 'NULL',
                                      '_steps', 'NULL')),
            ('elbo', ('?', '_post', 'item_feat', '_eps_ab', 'NULL')),      # (item_feat IS item_mu here: the first name in the alphabet)
            ('vibo_ptrain_epilogue', ('?', '?', 'NULL', 'NULL', 'beta', 'lr', '_steps', 'tables', 'NULL', 'person_m', 'person_v', 'slot',
                                      'item_feat', 'NULL', 'item_m', 'item_v', 'loss', 'NULL'))]
    assert got == [step, step]
    assert not bool(trainer._eps_ab[16].any())


# ---------------------------------------------------------------------------
# host validation
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('make', [_vi, _mle], ids=['vi', 'mle'])
def test_a_wrong_index_or_mask_raises_before_any_call(make, monkeypatch):
    torch.manual_seed(0)
    trainer = FusedTrainer(make(), rng='native')
    _, log = trace(trainer, monkeypatch, [])
    data = rows(16, 12)
    with pytest.raises(TypeError, match='`index` must be int64'):
        trainer.step(**data, index=torch.arange(16, dtype=torch.int32))
    with pytest.raises(ValueError, match='names 15 persons for a minibatch of 16'):
        trainer.step(**data, index=torch.arange(15))
    with pytest.raises(ValueError, match='`index` is on meta'):
        trainer.step(**data, index=torch.arange(16, device='meta'))
    with pytest.raises(ValueError, match='41 rows for tables of 40 persons'):
        trainer.step(**rows(41, 12))
    with pytest.raises(NotImplementedError, match='reads bool / uint8 masks'):
        trainer.step(data['response'], data['mask'].long())
    if make is _vi:
        with pytest.raises(ValueError, match='pass both eps_item and eps_ability, or neither'):
            trainer.step(**data, eps_item=torch.zeros(12, 3))
    assert log == [] and trainer._pending is None


# ---------------------------------------------------------------------------
# CLI
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('cli', [vi_cli, mle_cli], ids=['vi', 'mle'])
def test_cli_flags(cli, tmp_path):
    args = cli.build_parser().parse_args([])
    assert (args.native_step, args.no_graph, args.rng) == (False, False, 'torch')
    args = cli.build_parser().parse_args(['--native-step', '--no-graph', '--rng', 'native'])
    assert (args.native_step, args.no_graph, args.rng) == (True, True, 'native')
    with pytest.raises(SystemExit, match='--native-step needs --cuda'):
        cli.main(['--native-step', '--out-dir', str(tmp_path), '--num-person', '20', '--num-item', '8', '--epochs', '1'])
    assert not os.listdir(tmp_path)


# ---------------------------------------------------------------------------
# input admission
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('method', ['vi', 'mle'])
@pytest.mark.parametrize('case', pt.CASES, ids=pt.ident)
def test_inputs_keep_the_float32_reference_near_float64(method, case):
    dist, name, step = pt.float32_distance(pt.make_problem(method, *case))
    print(f'{method} {pt.ident(case)}: float32-oracle distance {dist:.2e} ({name}, step {step})')
    assert dist <= pt.ADMIT, (dist, name, step)
