"""--sparse-shuffle in the CLI (torch_core/vibo.py), on the CPU stand-ins: person-shuffled minibatches as RowGathers, unshuffled
passes as RowBlocks, the refusal without --row-format sparse, and a two-epoch run with the checkpoint keys of the `blocks` run."""
import os

import numpy as np
import pytest
import torch

import sparse_rows_common as S
from oracle import cpu_backend
from vibo_amd import config, ops
from vibo_amd.sparse import RowBlock, RowGather, SparseRows
from vibo_amd.torch_core import vibo as cli


@pytest.fixture()
def standins():
    restore_dense, restore_sparse = cpu_backend.install(ops), S.install_standin()
    yield
    restore_sparse()
    restore_dense()


class _Matrix:
    def __init__(self, P, I, seed):
        g = np.random.RandomState(seed)
        self.m = g.rand(P, I) < 0.3
        self.r = np.where(self.m, (g.rand(P, I) < 0.5), -1).astype(np.float32)
        self.num_person, self.num_item = P, I

    def matrix(self):
        return self.r, self.m


def test_flag_defaults_to_blocks_and_its_help_states_the_price():
    p = cli.build_parser()
    assert p.parse_args([]).sparse_shuffle == 'blocks'
    assert p.parse_args(['--sparse-shuffle', 'persons']).sparse_shuffle == 'persons'
    text = ''.join(p.format_help().split())
    assert 'WHOLEcolumnside' in text and 'profiles/sparse_gather_record.txt' in text


def test_persons_yields_gathers_that_cover_every_person_once_in_a_fresh_order_every_epoch():
    data = _Matrix(103, 9, 0)
    split = cli.ResidentSplit(data, torch.device('cpu'), None, 'sparse', sparse_shuffle='persons')
    assert isinstance(split.response, SparseRows) and split.mask is None
    torch.manual_seed(0)
    epochs = []
    for _ in range(3):
        batches = list(split.batches(16, shuffle=True))
        assert all(isinstance(b, RowGather) for b in batches) and len(batches) == split.num_batches(16) == 7
        assert [b.numel() for b in batches] == [16] * 6 + [7]
        assert all(b.index.dtype == torch.int64 for b in batches)
        order = torch.cat([b.index for b in batches]).tolist()
        assert sorted(order) == list(range(103))                                      # every person once
        epochs.append(order)
    assert epochs[0] != epochs[1] and epochs[1] != epochs[2] and epochs[0] != epochs[2]
    assert epochs[0] != sorted(epochs[0])                                             # persons, not blocks: the order inside a batch is random too
    # the same draw as the dense branch: one randperm over persons, cut into batch_size pieces
    dense = cli.ResidentSplit(data, torch.device('cpu'), None, 'f32')
    torch.manual_seed(7)
    a = [b.index.tolist() for b in split.batches(16, shuffle=True)]
    torch.manual_seed(7)
    assert a == [b.tolist() for b in dense.batches(16, shuffle=True)]
    r, m = split.rows(batches[1])                                                     # (log_marginal's densified minibatch)
    q = batches[1].index.numpy()
    assert np.array_equal(m.numpy(), data.m[q]) and np.array_equal(r.numpy(), data.r[q])


def test_unshuffled_passes_and_the_default_stay_blocks():
    data = _Matrix(103, 9, 0)
    for mode in ('persons', 'blocks'):
        split = cli.ResidentSplit(data, torch.device('cpu'), None, 'sparse', sparse_shuffle=mode)
        ordered = list(split.batches(16, shuffle=False))
        assert all(isinstance(b, RowBlock) for b in ordered)
        assert [(b.start, b.stop) for b in ordered] == [(s, min(103, s + 16)) for s in range(0, 103, 16)]
    assert cli.ResidentSplit(data, torch.device('cpu'), None, 'sparse').sparse_shuffle == 'blocks'
    assert all(isinstance(b, RowBlock) for b in split.batches(16, shuffle=True))      # (mode == 'blocks')


@pytest.mark.parametrize('fmt', ['auto', 'f32', 'codes'])
def test_flag_is_refused_without_sparse_rows_in_one_line(fmt):
    args = cli.finalize_args(cli.build_parser().parse_args(['--irt-model', '2pl', '--dataset', '2pl_simulation', '--num-item', '40',
                                                            '--row-format', fmt, '--sparse-shuffle', 'persons']))
    with pytest.raises(SystemExit) as e:
        cli.check_supported(args)
    msg = str(e.value)
    assert '--sparse-shuffle persons' in msg and '--row-format sparse' in msg and '\n' not in msg


def test_flag_is_taken_with_sparse_rows(standins):
    cli.check_supported(cli.finalize_args(cli.build_parser().parse_args(['--irt-model', '2pl', '--dataset', '2pl_simulation', '--num-item', '40',
                                                                         '--row-format', 'sparse', '--sparse-shuffle', 'persons'])))


def test_two_epoch_run_writes_the_checkpoint_keys_of_the_blocks_run(standins, tmp_path, monkeypatch):
    monkeypatch.setattr(config, 'DATA_DIR', str(tmp_path / 'data'))
    keys = {}
    for mode in ('persons', 'blocks'):
        out = tmp_path / ('out_' + mode)
        cli.main(['--irt-model', '2pl', '--dataset', '2pl_simulation', '--num-person', '75', '--num-item', '40', '--epochs', '2',
                  '--batch-size', '16', '--num-posterior-samples', '2', '--row-format', 'sparse', '--sparse-shuffle', mode,
                  '--out-dir', str(out)])
        (run_dir,) = os.listdir(out)
        assert {'checkpoint.pth.tar', 'model_best.pth.tar', 'train_losses.npy', 'test_losses.npy'} <= set(os.listdir(out / run_dir))
        ck = torch.load(out / run_dir / 'checkpoint.pth.tar', weights_only=False)
        keys[mode] = (set(ck), set(ck['infer_dict']), set(ck['model_state_dict']))
        assert ck['infer_dict']['ability_mu'].shape == (60, 1) and ck['posterior_predict_samples']['response'].shape[1:] == (60, 40, 1)
        assert np.isfinite(ck['train_logp']) and np.isfinite(ck['test_logp'])
        losses = np.load(out / run_dir / 'train_losses.npy')
        assert losses.shape == (2,) and np.isfinite(losses).all()
    assert keys['persons'] == keys['blocks']
