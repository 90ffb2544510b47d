"""The row-driven item pass of gathered minibatches on sparse response rows, host side (no GPU): the binding of
include/vibo_hip_sparse_row_driven.h, its workspace query and the return codes of its call before anything is launched, the key layout's
arithmetic, item_pass on RowGather / SparseRows.take and max_row_cells, the CPU stand-in on a view that asks for the row-driven pass,
and --sparse-item-pass in the CLI."""
import ctypes
import os

import numpy as np
import pytest
import torch

import sparse_rows_common as S
from oracle import cpu_backend
from row_format_common import _null_call, desc
from vibo_amd import _lib, ops, sparse
from vibo_amd.sparse import RowGather, SparseRows
from vibo_amd.torch_core import vibo as cli
from vibo_amd.torch_core.models import VIBO_2PL

HEADER = os.path.join(os.path.dirname(S.HEADER), 'vibo_hip_sparse_row_driven.h')
EXPORTS = ('vibo_sparse_row_driven_workspace_bytes', 'vibo_sparse_elbo_fwd_bwd_gather_rows')


def err():
    return _lib.load().vibo_last_error_string().decode()


# ---- binding ----
def test_header_is_bound_and_every_export_typed_from_it():
    assert 'vibo_hip_sparse_row_driven.h' in _lib.EXTRA_HEADERS and _lib.SPARSE_ROW_DRIVEN_SYMBOLS == EXPORTS
    lib = _lib.load()
    with open(HEADER) as f:
        text = f.read()
    assert '#include "vibo_hip_sparse_gather.h"' in text and '#define VIBO_SPARSE' not in text          # no constant of its own
    protos = {name: (res, args) for name, res, args in _lib.parse_prototypes(text)}
    assert tuple(protos) == EXPORTS
    for name, (res, args) in protos.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    img, vp, i64 = ctypes.POINTER(_lib.ViboSparseImage), ctypes.c_void_p, ctypes.c_int64
    assert protos[EXPORTS[0]] == (ctypes.c_size_t, [ctypes.POINTER(_lib.ViboDesc), i64, i64, i64])
    rows_args = protos[EXPORTS[1]][1]
    gather_args = dict((n, a) for n, _, a in _lib.EXTRA_PROTOTYPES)['vibo_sparse_elbo_fwd_bwd_gather']
    assert rows_args[:5] == [ctypes.POINTER(_lib.ViboDesc), img, vp, vp, i64]
    assert rows_args[:4] + rows_args[5:] == gather_args          # the column-driven call's arguments with max_row_cells put in


# ---- the workspace query ----
def query(d, I, P, max_row):
    return _lib.load().vibo_sparse_row_driven_workspace_bytes(ctypes.byref(d), ctypes.c_int64(I), ctypes.c_int64(P), ctypes.c_int64(max_row))


def test_workspace_query_is_zero_for_what_the_call_refuses_and_grows_with_max_row_cells():
    lib = _lib.load()
    good = desc(B=100, I=1000, mask=_lib.MASK_NONE)
    for kw in (dict(posterior=_lib.POSTERIOR_CONDITIONAL), dict(posterior=_lib.POSTERIOR_GIVEN), dict(n_flows=2), dict(A=9), dict(irt=7)):
        assert query(desc(**{'mask': _lib.MASK_NONE, 'B': 100, **kw}), 1000, 5000, 30) == 0, kw
    assert query(good, 999, 5000, 30) == 0                      # the image's items are not the descriptor's
    assert query(good, 1000, 0, 30) == 0 and query(good, 1000, 2 ** 31, 30) == 0
    assert query(good, 1000, 5000, 0) == 0 and query(good, 1000, 5000, -4) == 0
    sizes = [query(good, 1000, 5000, m) for m in (1, 2, 30, 31, 1000, 100_000)]
    assert all(s > 0 and s % 256 == 0 for s in sizes) and sizes == sorted(set(sizes))
    records = lib.vibo_sparse_workspace_bytes(ctypes.byref(good), ctypes.c_int64(0))
    assert records > 0 and sizes[0] > records
    # two buffers of cap 8-byte keys and the sort's 4 bytes per key, at least
    assert sizes[-1] - records >= 100 * 100_000 * 20
    assert query(good, 1000, 5000, 30) == query(good, 1000, 70_000, 30)          # (the image's persons fix the key, not the size)
    # forward only: the column-driven call's forward workspace, whatever max_row_cells says
    fwd = desc(B=100, I=1000, mask=_lib.MASK_NONE, grad=0)
    assert query(fwd, 1000, 5000, 30) == query(fwd, 1000, 5000, 0) == lib.vibo_sparse_workspace_bytes(ctypes.byref(fwd), ctypes.c_int64(0))


def test_cell_capacity_of_two_to_the_31_is_refused_by_the_query_and_by_the_call_before_anything_else():
    lib = _lib.load()
    fn = lib.vibo_sparse_elbo_fwd_bwd_gather_rows
    d = desc(B=1 << 16, I=1000, mask=_lib.MASK_NONE)
    assert query(d, 1000, 1 << 20, (1 << 15) - 1) > 0
    assert query(d, 1000, 1 << 20, 1 << 15) == 0                 # cap = 2^31
    assert query(d, 1000, 1 << 20, 1 << 40) == 0

    def null_call(max_row):
        return fn(ctypes.byref(d), None, None, None, ctypes.c_int64(max_row), *([None] * 11), 0, None)

    for m in (1 << 15, 1 << 40, 0, -1):
        assert null_call(m) == -8, m
        assert 'sparse rows' in err() and 'vibo_sparse_elbo_fwd_bwd_gather' in err() and 'column-driven' in err()
    assert null_call((1 << 15) - 1) == -5 and 'sparse rows' in err()          # in range: the next check is the image


# ---- return codes: every call below returns before a launch ----
def _fake_image(columns=True, P=1000, I=1000):
    im = _lib.ViboSparseImage()
    im.num_person, im.num_item, im.nnz, im.num_chunk = P, I, 10, (3 if columns else 0)
    im.row_ptr = im.row_cell = 256
    if columns:
        im.col_ptr = im.col_cell = im.col_chunk = im.chunk_item = im.chunk_first = 256
    return im


def test_return_codes_on_null_and_mismatched_arguments():
    lib = _lib.load()
    fn, p = lib.vibo_sparse_elbo_fwd_bwd_gather_rows, ctypes.c_void_p(256)
    good, fwd = desc(B=100, mask=_lib.MASK_NONE), desc(B=100, mask=_lib.MASK_NONE, grad=0)

    def call(d, im, index=p, slot=p, ws=p, ws_bytes=1 << 30, table=p, max_row=30):
        return fn(ctypes.byref(d), ctypes.byref(im) if im is not None else None, index, slot, ctypes.c_int64(max_row), table, p, p, p, p, p,
                  p, p, p, None, ws, ws_bytes, None)

    for columns in (True, False):          # an image without a column side is not refused: the next check answers
        assert call(good, _fake_image(columns), index=None) == -5 and 'person_index' in err()
        assert call(good, _fake_image(columns), slot=None) == -5 and 'person_slot' in err()
        assert call(good, _fake_image(columns), table=None) == -5 and 'sparse rows' in err()
        assert call(good, _fake_image(columns), ws=None) == -7 and 'sparse rows' in err()
        assert call(good, _fake_image(columns), ws_bytes=query(good, 1000, 1000, 30) - 1) == -7
        assert call(good, _fake_image(columns), ws=ctypes.c_void_p(264)) == -7                      # not 256-byte aligned
    assert call(good, None) == -5 and 'sparse rows' in err()
    assert call(good, _fake_image(I=999)) == -3 and 'sparse rows' in err()
    # forward only goes the column-driven call's way: no map, max_row_cells not read; next the workspace
    assert call(fwd, _fake_image(columns=False), slot=None, ws=None, max_row=0) == -7
    for kw in (dict(posterior=_lib.POSTERIOR_CONDITIONAL), dict(posterior=_lib.POSTERIOR_GIVEN), dict(n_flows=2), dict(A=9)):
        d = desc(**{'mask': _lib.MASK_NONE, 'B': 100, **kw})
        assert _null_call(fn, d) == -8 and 'sparse rows' in err(), kw


# ---- the key ----
@pytest.mark.parametrize('I', [1, 2, 2 ** 31 - 1])
@pytest.mark.parametrize('P', [1, 2, 2 ** 31 - 1])
def test_key_layout(P, I):
    bp, end_bit, pad = sparse.key_layout(P, I)
    assert bp == {1: 1, 2: 1, 2 ** 31 - 1: 31}[P]                       # bit_length(P - 1), at least 1
    assert end_bit == bp + 1 + {1: 1, 2: 2, 2 ** 31 - 1: 31}[I] <= 63
    largest = ((I - 1) << (bp + 1)) | ((P - 1) << 1) | 1                # the last item's cell of the last person, answered right
    smallest_of_next_item = lambda i: i << (bp + 1)
    assert ((P - 1) << 1 | 1) < (1 << (bp + 1))                         # person and answer stay below the item's place
    assert largest < pad == smallest_of_next_item(I) < (1 << end_bit) <= 1 << 63
    # a key splits back into its parts
    assert largest >> (bp + 1) == I - 1 and (largest >> 1) & ((1 << bp) - 1) == P - 1 and largest & 1 == 1
    if I > 1:
        assert ((I - 2) << (bp + 1)) | ((P - 1) << 1) | 1 < smallest_of_next_item(I - 1)          # items order the keys, persons inside


def test_key_layout_of_the_wide_key_test():
    assert sparse.key_layout(40_000, 70_000)[:2] == (16, 34)


# ---- RowGather / take / max_row_cells ----
def _dense_cases():
    g = torch.Generator().manual_seed(3)
    mask = torch.rand(23, 37, generator=g) < 0.3
    mask[5] = False                      # a row with no cell
    mask[7] = True                       # a full row
    resp = torch.where(mask, (torch.rand(23, 37, generator=g) < 0.5).float(), torch.tensor(-1.0))
    return resp, mask


def test_item_pass_is_checked_carried_by_the_view_and_defaults_to_columns():
    resp, mask = _dense_cases()
    rows = SparseRows.from_dense(resp, mask)
    idx = torch.tensor([7, 0, 22, 5])
    assert RowGather(idx).item_pass == 'columns' and RowGather(idx, item_pass='rows').item_pass == 'rows'
    assert RowGather(idx, 'rows').index is idx
    assert rows.item_pass == 'columns' and rows.rows(range(2, 9)).item_pass == 'columns'
    assert rows.take(idx).item_pass == 'columns' and rows.take(RowGather(idx)).item_pass == 'columns'
    assert rows.take(idx, item_pass='rows').item_pass == 'rows' and rows.take(idx, 'rows').index is idx
    assert rows.take(RowGather(idx, item_pass='rows')).item_pass == 'rows'
    assert rows.take(RowGather(idx, item_pass='rows'), item_pass='columns').item_pass == 'columns'
    assert rows.rows(range(3, 20)).take(torch.tensor([2, 0]), item_pass='rows').item_pass == 'rows'
    assert sparse._view(rows, None, RowGather(idx, item_pass='rows')).item_pass == 'rows'
    assert sparse._view(rows, None, RowGather(idx)).item_pass == 'columns'
    for bad in ('auto', 'row', None, 1, ''):
        with pytest.raises(ValueError, match='sparse rows.*item_pass'):
            RowGather(idx, item_pass=bad)
    for bad in ('auto', 'cols', 3):
        with pytest.raises(ValueError, match='sparse rows.*item_pass'):
            rows.take(idx, item_pass=bad)
    for bad in (torch.arange(4, dtype=torch.int32), torch.zeros(0, dtype=torch.int64), [1, 2]):
        with pytest.raises(ValueError, match='sparse rows'):
            RowGather(bad, item_pass='rows')
        with pytest.raises(ValueError, match='sparse rows'):
            rows.take(bad, item_pass='rows')


def test_max_row_cells_is_the_base_images_computed_once_and_shared_by_the_views():
    resp, mask = _dense_cases()
    rows = SparseRows.from_dense(resp, mask)
    assert rows._max_row == [None]
    view = rows.rows(range(0, 5)).take(torch.tensor([1, 2]), item_pass='rows')          # rows that are not the longest
    assert view.max_row_cells == 37 == int(mask.sum(1).max()) and rows._max_row == [37] and view._max_row is rows._max_row
    rows._max_row[0] = 99                                                                # a second look reads the holder, not row_ptr
    assert rows.max_row_cells == 99 and rows.take(torch.tensor([3])).max_row_cells == 99
    empty = SparseRows.from_dense(torch.full((3, 4), -1.0), torch.zeros(3, 4, dtype=torch.bool))
    assert empty.max_row_cells == 1                                                      # (the call takes max_row_cells >= 1)


# ---- the stand-in ignores the attribute ----
@pytest.fixture
def standin():
    restore_dense, restore_sparse = cpu_backend.install(ops), S.install_standin()
    yield
    restore_sparse()
    restore_dense()


def test_standin_serves_a_view_that_asks_for_the_row_driven_pass(standin):
    P, I, A = 41, 29, 2
    g = torch.Generator().manual_seed(11)
    mask = torch.rand(P, I, generator=g) < 0.4
    resp = torch.where(mask, (torch.rand(P, I, generator=g) < 0.5).float(), torch.tensor(-1.0))
    rows = SparseRows.from_dense(resp, mask)
    idx = torch.randperm(P, generator=g)[:17]
    torch.manual_seed(5)
    model = VIBO_2PL(A, I, ability_merge='product')
    losses, grads = [], []
    for response, m, ri in ((resp, mask, idx), (rows, None, RowGather(idx, item_pass='rows')), (rows.take(idx, item_pass='rows'), None, None),
                            (rows, None, RowGather(idx))):
        model.zero_grad(set_to_none=True)
        torch.manual_seed(9)
        loss = model.elbo_step(response, m, annealing_factor=0.6, row_index=ri)
        loss.backward()
        losses.append(float(loss.detach()))
        grads.append({k: p.grad.clone() for k, p in model.named_parameters()})
    for b in (1, 2, 3):
        assert losses[0] == pytest.approx(losses[b], rel=1e-6)
        for k in grads[0]:
            assert torch.allclose(grads[0][k], grads[b][k], rtol=1e-5, atol=1e-6), k
    assert rows._max_row == [None] and rows._slot == [None]          # the stand-in needed neither


def test_the_native_call_is_chosen_by_the_views_item_pass_and_the_map_refilled_when_it_raises(monkeypatch):
    resp, mask = _dense_cases()
    rows = SparseRows.from_dense(resp, mask)
    spec = ops.ElboSpec(irt_model=2, ability_dim=2)
    seen = []

    def failing_call(name, *args):
        seen.append((name, len(args)))
        rows.slot_map()[[4, 9, 1]] = torch.tensor([0, 1, 2], dtype=torch.int32)
        raise _lib.ViboLibraryError('planted')

    monkeypatch.setattr(ops, '_require_device', lambda *tensors: None)
    monkeypatch.setattr(ops, '_stream', lambda device: None)
    monkeypatch.setattr(ops, '_call', failing_call)
    for item_pass, name, n_args in (('rows', 'vibo_sparse_elbo_fwd_bwd_gather_rows', 18), ('columns', 'vibo_sparse_elbo_fwd_bwd_gather', 17)):
        view = rows.take(torch.tensor([4, 9, 1]), item_pass=item_pass)
        with pytest.raises(_lib.ViboLibraryError, match='planted'):
            sparse._hip_sparse_elbo(spec, view, torch.zeros(2, 4), torch.zeros(37, 3), torch.zeros(3, 2), _lib.REG_KL, True)
        assert seen[-1] == (name, n_args)
        assert bool((rows.slot_map() == _lib.SPARSE_NO_SLOT).all())
    assert rows._max_row == [37]


# ---- the CLI ----
class _Matrix:
    def __init__(self, P, I, seed):
        g = np.random.RandomState(seed)
        self.m = g.rand(P, I) < 0.3
        self.r = np.where(self.m, (g.rand(P, I) < 0.5), -1).astype(np.float32)
        self.num_person, self.num_item = P, I

    def matrix(self):
        return self.r, self.m


BASE = ['--irt-model', '2pl', '--dataset', '2pl_simulation', '--num-item', '40']


def test_flag_defaults_to_columns_and_names_the_record():
    p = cli.build_parser()
    assert p.parse_args([]).sparse_item_pass == 'columns'
    assert p.parse_args(['--sparse-item-pass', 'rows']).sparse_item_pass == 'rows'
    with pytest.raises(SystemExit):
        p.parse_args(['--sparse-item-pass', 'auto'])
    assert 'profiles/sparse_row_driven_record.txt' in ''.join(p.format_help().split())


@pytest.mark.parametrize('extra', [[], ['--row-format', 'f32'], ['--row-format', 'codes', '--sparse-shuffle', 'persons'], ['--row-format', 'sparse'],
                                   ['--row-format', 'sparse', '--sparse-shuffle', 'blocks']])
def test_flag_is_refused_without_gathered_sparse_minibatches(standin, extra):
    args = cli.finalize_args(cli.build_parser().parse_args(BASE + extra + ['--sparse-item-pass', 'rows']))
    with pytest.raises(SystemExit) as e:
        cli.check_supported(args)
    msg = str(e.value)
    assert '--sparse-item-pass rows' in msg and '--row-format sparse --sparse-shuffle persons' in msg and '\n' not in msg


def test_flag_is_taken_with_gathered_sparse_minibatches_and_reaches_the_row_gathers(standin):
    for choice in ('rows', 'columns'):
        cli.check_supported(cli.finalize_args(cli.build_parser().parse_args(
            BASE + ['--row-format', 'sparse', '--sparse-shuffle', 'persons', '--sparse-item-pass', choice])))
    cli.check_supported(cli.finalize_args(cli.build_parser().parse_args(BASE + ['--sparse-item-pass', 'columns'])))      # the default, anywhere
    data = _Matrix(103, 9, 0)
    split = cli.ResidentSplit(data, torch.device('cpu'), None, 'sparse', sparse_shuffle='persons', sparse_item_pass='rows')
    batches = list(split.batches(16, shuffle=True))
    assert len(batches) == 7 and all(isinstance(b, RowGather) and b.item_pass == 'rows' for b in batches)
    default = cli.ResidentSplit(data, torch.device('cpu'), None, 'sparse', sparse_shuffle='persons')
    assert default.sparse_item_pass == 'columns' and all(b.item_pass == 'columns' for b in default.batches(16, shuffle=True))


def test_two_epoch_run_with_the_flag(standin, tmp_path, monkeypatch):
    from vibo_amd import config
    monkeypatch.setattr(config, 'DATA_DIR', str(tmp_path / 'data'))
    out = tmp_path / 'out'
    cli.main(['--irt-model', '2pl', '--dataset', '2pl_simulation', '--num-person', '75', '--num-item', '40', '--epochs', '2', '--batch-size', '16',
              '--num-posterior-samples', '2', '--row-format', 'sparse', '--sparse-shuffle', 'persons', '--sparse-item-pass', 'rows',
              '--out-dir', str(out)])
    (run_dir,) = os.listdir(out)
    losses = np.load(out / run_dir / 'train_losses.npy')
    assert losses.shape == (2,) and np.isfinite(losses).all()
