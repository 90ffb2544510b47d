"""The folded step that draws its own noise stores no ability sample; `trainer.last.ability` rebuilds it when read.  Without a GPU:
what the trainer hands to the library for that (the recorders of test_trainer_call_sequence.py, with an ELBO stand-in that, like
the real launch, returns no sample for a drawing step), and when the rebuild is refused."""
import pytest
import torch

from decoder_trainer_common import CLS
from test_trainer_call_sequence import FUSED, owner, rows
from vibo_amd import _lib, ops
from vibo_amd.trainer import FusedTrainer

B, I, A = 4096, 1000, 8       # the bench's shape class: the planner gives it to the matrix kernel, whose folded step draws


@pytest.fixture
def traced(monkeypatch):
    """-> (trainer, log): every native call as (name, owners of its pointer arguments); the ELBO stand-in logs 'elbo[step+noise]' /
    'elbo[step]' / 'elbo' and returns a RawElbo whose sample is None exactly where the real launch allocates none."""
    torch.manual_seed(0)
    trainer = FusedTrainer(CLS[2](A, I, hidden_dim=64, ability_merge='product'), rng='native')
    log = []

    def named(args):
        import ctypes
        return tuple(owner(trainer, a.value if isinstance(a, ctypes.c_void_p) else None if a is None else a.data_ptr())
                     for a in args if a is None or isinstance(a, (ctypes.c_void_p, torch.Tensor)))

    def elbo(spec, response, mask, code, row_index, table, item, eps, flow, reg_mode, want_grad, num_person, train_step=None):
        own_noise = train_step is not None and train_step[2] is not None
        log.append(('elbo' + ('' if train_step is None else '[step+noise]' if own_noise else '[step]'), named((table, item, eps, flow))))
        n, n_table, n_item = int(num_person), table.numel(), response.shape[1] * spec.item_dim
        assert not own_noise or train_step[3] is True            # (the trainer asks a drawing step for no sample)
        post = [None if own_noise else torch.zeros(n, spec.ability_dim) for _ in range(3)]
        return ops.RawElbo(flat=torch.zeros(_lib.NUM_SCALARS + 2 * n_table + n_item), n_table=n_table, n_item=n_item, n_flow=0,
                           table_shape=tuple(table.shape), ability_mu=post[0], ability_logvar=post[1], ability=post[2], ability_k=None,
                           ability_ladj=None, workspace=torch.zeros(256, dtype=torch.uint8))

    monkeypatch.setattr(ops, '_call', lambda name, *args: log.append((name, named(args))))
    monkeypatch.setattr(ops, '_stream', lambda dev: None)
    monkeypatch.setitem(ops._BACKEND, 'elbo', elbo)
    return trainer, log


STEP = [('elbo[step+noise]', ('table', 'item_feat', 'NULL', 'NULL')), ('vibo_train_epilogue_fused', FUSED + ('NULL', 'NULL'))]


def test_a_drawing_step_keeps_no_sample_and_rebuilds_nothing_unless_asked(traced):
    trainer, log = traced
    data = rows(B, I)
    trainer.step(**data)
    del log[:]
    trainer.step(**data)
    assert trainer._draw_mode and log == STEP                     # no fill, no second ELBO call: nothing is materialised
    raw = trainer.last
    assert raw.ability_mu is None and raw._ability is None and raw.ability_source is trainer._kept_of
    assert not any(isinstance(v, torch.Tensor) and tuple(v.shape) == (B, A) for v in vars(raw).values())
    # the table the step ran on: the second half of the allocation the epilogue is handed (it keeps it there itself)
    assert trainer.table.is_contiguous() and trainer.table_prev.shape == trainer.table.shape
    assert trainer.table_prev.data_ptr() == trainer.table.data_ptr() + 4 * trainer.table.numel()
    del log[:]
    sample = raw.ability
    assert tuple(sample.shape) == (B, A)
    # the noise at a counter of its own (step_count[1] - 1: a temporary), then the plain ELBO call on the kept table
    assert log == [('vibo_fill_normal', ('?', '?', 'NULL')), ('elbo', ('table_prev', 'item_feat', '?', 'NULL'))]
    del log[:]
    assert raw.ability is sample and log == []                    # an eager step's sample is rebuilt once


def test_the_rebuild_reads_the_live_table_while_the_step_is_open_and_raises_once_it_is_gone(traced):
    trainer, log = traced
    data = rows(B, I)
    first = trainer.forward_backward(**data)
    assert first.ability_source is trainer._head_of
    del log[:]
    first.ability                                                # update() has not run: `table` still is the step's
    assert log == [('vibo_fill_normal', ('?', '_steps', 'NULL')), ('elbo', ('table', 'item_feat', '?', 'NULL'))]
    trainer.update()
    second = trainer.forward_backward(**data)
    del log[:]
    trainer.update()                                             # `table_prev` moves on to the second step's table
    trainer.step(**data)
    third = trainer.last
    assert trainer._kept_of is third.ability_source
    with pytest.raises(RuntimeError, match='before the next update'):
        second.ability
    assert tuple(first.ability.shape) == (B, A)                  # (what was rebuilt in time stays)
    trainer.step(**dict(data, row_index=torch.arange(16)))       # a short minibatch on the VALU kernel stores its sample
    assert trainer.last.ability_source is None and tuple(trainer.last.ability.shape) == (16, A)
    with pytest.raises(RuntimeError, match='before the next update'):
        third.ability
