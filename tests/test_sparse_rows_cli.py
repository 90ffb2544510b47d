"""--row-format sparse in the CLI (torch_core/vibo.py), on the CPU stand-ins: the refusals of check_supported, a two-epoch run with
the checkpoint keys of the other formats, and the block-shuffled minibatch order."""
import os

import numpy as np
import pytest
import torch

import sparse_rows_common as S
from oracle import cpu_backend
from vibo_amd import config, ops
from vibo_amd.sparse import RowBlock, SparseRows
from vibo_amd.torch_core import vibo as cli


@pytest.fixture()
def standins():
    restore_dense, restore_sparse = cpu_backend.install(ops), S.install_standin()
    yield
    restore_sparse()
    restore_dense()


def _args(*extra):
    return cli.finalize_args(cli.build_parser().parse_args(['--irt-model', '2pl', '--dataset', '2pl_simulation', '--num-item', '40',
                                                            '--row-format', 'sparse', *extra]))


def test_auto_never_chooses_sparse_and_help_says_what_it_is():
    p = cli.build_parser()
    assert p.parse_args([]).row_format == 'auto'
    text = ''.join(p.format_help().split())          # (argparse wraps at hyphens too: compare without white space)
    assert 'block-shuffledSGD' in text and 'profiles/sparse_rows_record.txt' in text and 'above32767items' in text


@pytest.mark.parametrize('extra,word', [(['--conditional-posterior'], '--conditional-posterior'), (['--n-norm-flows', '2'], '--n-norm-flows'),
                                        (['--ability-merge', 'mean'], '--ability-merge mean'), (['--generative-model', 'deep'], 'MLP decoder'),
                                        (['--ability-dim', '9'], '--ability-dim above 8'), ([], 'WORLD_SIZE'), ([], 'no --cuda'),
                                        (['--num-item', '40000'], '--no-marginal')])
def test_check_supported_refuses_in_one_line_before_data_is_loaded(standins, monkeypatch, extra, word):
    if word == 'WORLD_SIZE':
        monkeypatch.setenv('WORLD_SIZE', '2')
    if word == 'no --cuda':          # (the native launch installed: the CPU cannot run it)
        monkeypatch.setitem(ops._BACKEND, 'sparse_elbo', ops._sparse._hip_sparse_elbo)
    with pytest.raises(SystemExit) as e:
        cli.check_supported(_args(*extra))
    msg = str(e.value)
    assert '--row-format sparse' in msg and word in msg and '\n' not in msg


def test_check_supported_takes_the_plain_model(standins):
    cli.check_supported(_args())
    cli.check_supported(_args('--num-item', '40000', '--no-marginal', '--drop-missing', '--ability-dim', '8'))


class _Matrix:
    def __init__(self, P, I, seed):
        g = np.random.RandomState(seed)
        self.m = g.rand(P, I) < 0.3
        self.r = np.where(self.m, (g.rand(P, I) < 0.5), -1).astype(np.float32)
        self.num_person, self.num_item = P, I

    def matrix(self):
        return self.r, self.m


def test_batches_are_blocks_in_a_fresh_order_every_epoch():
    data = _Matrix(103, 9, 0)
    split = cli.ResidentSplit(data, torch.device('cpu'), None, 'sparse')
    assert isinstance(split.response, SparseRows) and split.mask is None and (split.num_person, split.num_item) == (103, 9)
    ordered = list(split.batches(16, shuffle=False))
    assert all(isinstance(b, RowBlock) for b in ordered)
    assert [(b.start, b.stop) for b in ordered] == [(s, min(103, s + 16)) for s in range(0, 103, 16)] and split.num_batches(16) == 7
    torch.manual_seed(0)
    epochs = [[(b.start, b.stop) for b in split.batches(16, shuffle=True)] for _ in range(3)]
    for e in epochs:
        assert sorted(e) == [(b.start, b.stop) for b in ordered]                       # every person once
        assert sorted(p for a, b in e for p in range(a, b)) == list(range(103))
    assert epochs[0] != epochs[1] or epochs[1] != epochs[2]
    r, m = split.rows(ordered[2])                                                     # (log_marginal's densified block)
    assert np.array_equal(m.numpy(), data.m[32:48]) and np.array_equal(r.numpy(), data.r[32:48])


def test_two_epoch_run_writes_the_checkpoint_keys_of_the_other_formats(standins, tmp_path, monkeypatch):
    monkeypatch.setattr(config, 'DATA_DIR', str(tmp_path / 'data'))
    keys = {}
    for fmt in ('sparse', 'f32'):
        out = tmp_path / ('out_' + fmt)
        cli.main(['--irt-model', '2pl', '--dataset', '2pl_simulation', '--num-person', '75', '--num-item', '40', '--epochs', '2',
                  '--batch-size', '16', '--num-posterior-samples', '2', '--row-format', fmt, '--out-dir', str(out)])
        (run_dir,) = os.listdir(out)
        assert {'checkpoint.pth.tar', 'model_best.pth.tar', 'train_losses.npy', 'test_losses.npy'} <= set(os.listdir(out / run_dir))
        ck = torch.load(out / run_dir / 'checkpoint.pth.tar', weights_only=False)
        keys[fmt] = (set(ck), set(ck['infer_dict']), set(ck['model_state_dict']))
        assert ck['infer_dict']['ability_mu'].shape == (60, 1) and ck['posterior_predict_samples']['response'].shape[1:] == (60, 40, 1)
        assert np.isfinite(ck['train_logp']) and np.isfinite(ck['test_logp'])
        losses = np.load(out / run_dir / 'train_losses.npy')
        assert losses.shape == (2,) and np.isfinite(losses).all()
    assert keys['sparse'] == keys['f32']
