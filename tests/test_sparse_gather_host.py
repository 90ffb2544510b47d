"""Gathered minibatches on sparse response rows, host side (no GPU): the binding of include/vibo_hip_sparse_gather.h, its constant, the
return codes of its two exports before anything is launched, SparseRows.take / RowGather / to_dense against resp[index], the refusals,
and the models on a gathered view against the dense model's row_index step, with the CPU stand-in for the sparse launch."""
import ctypes
import os
import re

import pytest
import torch

import sparse_rows_common as S
from oracle import cpu_backend
from row_format_common import _null_call, desc
from vibo_amd import _lib, ops, sparse
from vibo_amd.sparse import RowBlock, RowGather, SparseRows
from vibo_amd.torch_core.models import VIBO_1PL, VIBO_2PL, VIBO_3PL

HEADER = os.path.join(os.path.dirname(S.HEADER), 'vibo_hip_sparse_gather.h')
EXPORTS = ('vibo_sparse_elbo_fwd_bwd_gather', 'vibo_sparse_encode_gather')


def err():
    return _lib.load().vibo_last_error_string().decode()


# ---- binding ----
def test_header_is_bound_and_every_export_typed_from_it():
    assert 'vibo_hip_sparse_gather.h' in _lib.EXTRA_HEADERS
    assert _lib.SPARSE_GATHER_SYMBOLS == EXPORTS
    lib = _lib.load()
    with open(HEADER) as f:
        text = f.read()
    assert '#include "vibo_hip_sparse_rows.h"' in text
    protos = {name: (res, args) for name, res, args in _lib.parse_prototypes(text)}
    assert tuple(protos) == EXPORTS
    for name, (res, args) in protos.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    img, vp = ctypes.POINTER(_lib.ViboSparseImage), ctypes.c_void_p
    assert protos['vibo_sparse_elbo_fwd_bwd_gather'][1][:4] == [ctypes.POINTER(_lib.ViboDesc), img, vp, vp]
    assert len(protos['vibo_sparse_elbo_fwd_bwd_gather'][1]) == 17 and protos['vibo_sparse_elbo_fwd_bwd_gather'][1][-2] is ctypes.c_size_t
    assert protos['vibo_sparse_encode_gather'][1] == [ctypes.POINTER(_lib.ViboDesc), img, vp, vp, vp, vp, vp, vp]


def test_no_slot_mirrors_the_header():
    with open(HEADER) as f:
        defines = dict(re.findall(r'^#define (VIBO_SPARSE_\w+) (\w+)', f.read(), flags=re.M))
    assert defines == {'VIBO_SPARSE_NO_SLOT': '0x7fffffff'}          # the one constant this header adds
    assert _lib.SPARSE_NO_SLOT == int(defines['VIBO_SPARSE_NO_SLOT'], 16) == torch.iinfo(torch.int32).max


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
    fn, enc, p = lib.vibo_sparse_elbo_fwd_bwd_gather, lib.vibo_sparse_encode_gather, ctypes.c_void_p(256)
    good, fwd = desc(B=100, mask=_lib.MASK_NONE), desc(B=100, mask=_lib.MASK_NONE, grad=0)

    def call(d, im, index=p, slot=p, ws=p, ws_bytes=1 << 30, table=p):
        return fn(ctypes.byref(d), ctypes.byref(im) if im is not None else None, index, slot, table, p, p, p, p, p, p, p, p, None, ws,
                  ws_bytes, None)

    assert call(good, _fake_image(), index=None) == -5 and 'sparse rows' in err() and 'person_index' in err()
    assert call(good, _fake_image(), slot=None) == -5 and 'sparse rows' in err() and 'person_slot' in err()
    assert call(fwd, _fake_image(columns=False), slot=None, ws=None) == -7          # forward only: no map, no column side; next the workspace
    assert call(good, None) == -5 and 'sparse rows' in err()
    assert call(good, _fake_image(), table=None) == -5 and 'sparse rows' in err()
    assert call(good, _fake_image(I=999)) == -3 and 'sparse rows' in err()          # the image's items are not the descriptor's
    assert call(desc(B=100, irt=7, mask=_lib.MASK_NONE), _fake_image()) == -3 and 'sparse rows' in err()
    assert call(good, _fake_image(columns=False)) == -8 and 'column side' in err() and 'sparse rows' in err()
    assert call(good, _fake_image(), ws=None) == -7 and 'sparse rows' in err()
    assert call(good, _fake_image(), ws_bytes=16) == -7
    assert call(good, _fake_image(), ws=ctypes.c_void_p(264)) == -7                  # not 256-byte aligned
    assert call(desc(B=5000, mask=_lib.MASK_NONE), _fake_image(), ws=None) == -7     # more rows than persons is no error of its own (repeats)
    for kw in (dict(posterior=_lib.POSTERIOR_CONDITIONAL), dict(posterior=_lib.POSTERIOR_GIVEN), dict(n_flows=2), dict(A=9)):
        d = desc(**{'mask': _lib.MASK_NONE, 'B': 100, **kw})
        assert lib.vibo_sparse_rows_supported(ctypes.byref(d)) == 0
        for f in (fn, enc):
            assert _null_call(f, d) == -8 and 'sparse rows' in err(), (kw, f)

    def encode(d, im, index=p, table=p):
        return enc(ctypes.byref(d), ctypes.byref(im) if im is not None else None, index, table, p, p, None, None)

    assert encode(good, _fake_image(columns=False), index=None) == -5 and 'person_index' in err()
    assert encode(good, _fake_image(columns=False), table=None) == -5 and 'sparse rows' in err()
    assert encode(good, None) == -5 and 'sparse rows' in err()
    assert encode(good, _fake_image(I=7)) == -3 and 'sparse rows' in err()


# ---- take / RowGather / to_dense ----
def _dense_cases():
    g = torch.Generator().manual_seed(3)
    mask = torch.rand(23, 37, generator=g) < 0.3
    mask[5] = False                      # a row with no cell
    mask[:, 11] = False                  # a column with no cell
    mask[7] = True                       # a full row
    resp = torch.where(mask, (torch.rand(23, 37, generator=g) < 0.5).float(), torch.tensor(-1.0))
    return resp, mask


def test_take_round_trips_against_the_indexed_dense_rows():
    resp, mask = _dense_cases()
    rows = SparseRows.from_dense(resp, mask)
    assert rows.index is None and rows.rows(range(2, 9)).index is None
    idx = torch.tensor([7, 0, 22, 5, 5, 13, 7])                   # the full row, the ends, the empty row, repeats
    for view in (rows.take(idx), rows.take(RowGather(idx))):
        assert (view.num_person, view.shape, len(view), view.image_persons) == (7, (7, 37), 7, 23) and view.index is idx
        r, m = view.to_dense()
        assert torch.equal(m, mask[idx]) and torch.equal(r, resp[idx])
        r, m = view.to_dense(range(2, 5))
        assert torch.equal(m, mask[idx[2:5]]) and torch.equal(r, resp[idx[2:5]])
    sub = rows.rows(range(3, 20)).take(torch.tensor([2, 0, 16]))  # persons relative to the range view: 5, 3, 19
    assert sub.image_index.tolist() == [5, 3, 19] and sub.num_person == 3
    r, m = sub.to_dense()
    assert torch.equal(m, mask[[5, 3, 19]]) and torch.equal(r, resp[[5, 3, 19]])
    outside = rows.rows(range(3, 20)).take(torch.tensor([2, 17, -1]))      # 17 and -1 are not persons of that view: no launch follows them
    assert outside.image_index.tolist() == [5, -1, -1]
    with pytest.raises(ValueError, match='sparse rows'):
        outside.to_dense()
    g = RowGather(idx)
    assert g.numel() == len(g) == 7 and g.index is idx
    assert view.slot_map() is rows.slot_map() and rows.slot_map().dtype == torch.int32 and rows.slot_map().shape == (23,)
    assert bool((rows.slot_map() == _lib.SPARSE_NO_SLOT).all())


def test_refusals_name_the_format():
    resp, mask = _dense_cases()
    rows = SparseRows.from_dense(resp, mask)
    view = rows.take(torch.arange(4))
    with pytest.raises(NotImplementedError, match='sparse rows.*rows\\(\\) of a gathered view'):
        view.rows(range(0, 2))
    with pytest.raises(NotImplementedError, match='sparse rows.*take\\(\\) of a gathered view'):
        view.take(torch.arange(2))
    with pytest.raises(ValueError, match='sparse rows'):
        view.to('cpu')
    for bad in (torch.arange(4, dtype=torch.int32), torch.zeros(2, 2, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), [1, 2]):
        with pytest.raises(ValueError, match='sparse rows'):
            rows.take(bad)
        with pytest.raises(ValueError, match='sparse rows'):
            RowGather(bad)
    with pytest.raises(NotImplementedError, match='sparse rows.*tensor row_index.*RowGather'):
        rows.rows(torch.arange(4))
    with pytest.raises(NotImplementedError, match='sparse rows.*tensor row_index'):
        sparse._view(rows, None, torch.arange(4))
    with pytest.raises(NotImplementedError, match='sparse rows.*sharding'):
        sparse._view(rows, None, RowGather(torch.arange(4)), reducer=lambda flat: None)
    assert sparse._view(rows, None, RowGather(torch.arange(4))).num_person == 4
    assert sparse._view(rows, None, RowBlock(1, 4)).index is None


# ---- the models, with the CPU stand-in ----
@pytest.fixture
def standin():
    restore_dense, restore_sparse = cpu_backend.install(ops), S.install_standin()
    yield
    restore_sparse()
    restore_dense()


@pytest.mark.parametrize('cls,A,drop', [(VIBO_1PL, 1, False), (VIBO_2PL, 3, False), (VIBO_3PL, 2, True)])
def test_model_on_a_gathered_view_matches_the_dense_row_index_step(standin, cls, A, drop):
    P, I = 41, 29
    g = torch.Generator().manual_seed(11)
    mask = torch.rand(P, I, generator=g) < 0.4
    mask[:, 0] = True                                  # (every row observes something: --drop-missing needs it)
    resp = torch.where(mask, (torch.rand(P, I, generator=g) < 0.5).float(), torch.tensor(-1.0))
    rows = SparseRows.from_dense(resp, mask)
    idx = torch.randperm(P, generator=g)[:17]
    torch.manual_seed(5)
    model = cls(A, I, ability_merge='product', replace_missing_with_prior=not drop)
    losses, grads, posts = [], [], []
    for response, m, ri in ((resp, mask, idx), (rows, None, RowGather(idx)), (rows.take(idx), None, None), (resp, mask, None)):
        model.zero_grad(set_to_none=True)
        torch.manual_seed(9)
        loss = model.elbo_step(response, m, annealing_factor=0.6, row_index=ri)
        loss.backward()
        losses.append(float(loss.detach()))
        grads.append({k: p.grad.clone() for k, p in model.named_parameters()})
        torch.manual_seed(10)
        posts.append(model.encode(response, m, row_index=ri)[1:3])
    for b in (1, 2):
        assert losses[0] == pytest.approx(losses[b], rel=1e-6)
        for k in grads[0]:
            assert torch.allclose(grads[0][k], grads[b][k], rtol=1e-5, atol=1e-6), k
        for x, y in zip(posts[0], posts[b]):
            assert x.shape == (17, A) and torch.allclose(x, y, rtol=1e-6, atol=1e-6)
    assert losses[0] != pytest.approx(losses[3], rel=1e-3)        # the index was honoured: other persons, another loss


def test_ops_take_a_row_gather_and_still_refuse_a_bare_tensor(standin):
    resp, mask = _dense_cases()
    rows = SparseRows.from_dense(resp, mask)
    spec, I = ops.ElboSpec(irt_model=2, ability_dim=2), rows.num_item
    idx = torch.tensor([4, 9, 1, 20, 7, 12])

    def call(row_index):
        return ops.fused_elbo(spec, torch.zeros(spec.table_shape(I, 6)), torch.zeros(I, spec.item_dim), None, rows, None, torch.zeros(6, 2),
                              row_index=row_index)

    assert call(RowGather(idx))[3].shape == (6, 2)
    mu, lv = ops.encode_posterior(spec, torch.zeros(2, 4), rows, None, row_index=RowGather(idx))
    assert mu.shape == lv.shape == (6, 2)
    with pytest.raises(NotImplementedError, match='sparse rows.*tensor row_index'):
        call(idx)
    with pytest.raises(NotImplementedError, match='sparse rows.*tensor row_index'):
        ops.encode_posterior(spec, torch.zeros(2, 4), rows, None, row_index=idx)


def test_the_map_is_refilled_when_a_gathered_call_raises(monkeypatch):
    """A call that stops between the map's build and its clear must not leave entries for the next one: _hip_sparse_elbo refills
    the map before the exception propagates.  The launch is replaced by one that dirties the map and fails; nothing runs on a device."""
    resp, mask = _dense_cases()
    rows = SparseRows.from_dense(resp, mask)
    view = rows.take(torch.tensor([4, 9, 1]))
    spec = ops.ElboSpec(irt_model=2, ability_dim=2)
    seen = []

    def failing_call(name, *args):
        seen.append(name)
        rows.slot_map()[[4, 9, 1]] = torch.tensor([0, 1, 2], dtype=torch.int32)
        raise _lib.ViboLibraryError('planted')

    monkeypatch.setattr(ops, '_require_device', lambda *tensors: None)
    monkeypatch.setattr(ops, '_stream', lambda device: None)
    monkeypatch.setattr(ops, '_call', failing_call)
    with pytest.raises(_lib.ViboLibraryError, match='planted'):
        sparse._hip_sparse_elbo(spec, view, torch.zeros(2, 4), torch.zeros(37, 3), torch.zeros(3, 2), _lib.REG_KL, True)
    assert seen == ['vibo_sparse_elbo_fwd_bwd_gather']
    assert bool((rows.slot_map() == _lib.SPARSE_NO_SLOT).all())
