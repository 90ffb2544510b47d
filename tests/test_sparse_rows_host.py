"""Sparse response rows, host side (no GPU): the header's binding and constants, the return codes of the five exports on NULL
buffers, the SparseRows builders and their chunk list, the host mirror of the validation pass, and the dispatch and refusals of
vibo_amd.ops / the models with a CPU stand-in for the sparse launch."""
import ctypes

import pytest
import torch

import sparse_rows_common as S
from oracle import cpu_backend
from row_format_common import _null_call, desc
from vibo_amd import _lib, ops, sparse
from vibo_amd.sparse import RowBlock, SparseRows
from vibo_amd.torch_core.models import VIBO_1PL, VIBO_2PL, VIBO_3PL

CHUNK = S.CHUNK
EXPORTS = ('vibo_sparse_rows_supported', 'vibo_sparse_workspace_bytes', 'vibo_sparse_rows_check', 'vibo_sparse_elbo_fwd_bwd',
           'vibo_sparse_encode')


def err():
    return _lib.load().vibo_last_error_string().decode()


# ---- binding ----
def test_header_is_bound_and_every_export_typed_from_it():
    assert 'vibo_hip_sparse_rows.h' in _lib.EXTRA_HEADERS
    assert _lib.SPARSE_ROWS_SYMBOLS == EXPORTS
    lib = _lib.load()
    with open(S.HEADER) as f:
        protos = {name: (res, args) for name, res, args in _lib.parse_prototypes(f.read())}
    assert tuple(protos) == EXPORTS
    for name, (res, args) in protos.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    img = ctypes.POINTER(_lib.ViboSparseImage)
    assert protos['vibo_sparse_elbo_fwd_bwd'][1][:3] == [ctypes.POINTER(_lib.ViboDesc), img, ctypes.c_int64]
    assert protos['vibo_sparse_rows_check'][1][0] is img and protos['vibo_sparse_workspace_bytes'][0] is ctypes.c_size_t


def test_constants_and_struct_mirror_the_header():
    c = S.header_constants()
    assert c == {'VIBO_SPARSE_CHUNK': _lib.SPARSE_CHUNK, 'VIBO_SPARSE_ROWS_PER_BLOCK': _lib.SPARSE_ROWS_PER_BLOCK,
                 'VIBO_SPARSE_MAX_BLOCKS': _lib.SPARSE_MAX_BLOCKS, 'VIBO_SPARSE_RECORD_FLOATS': _lib.SPARSE_RECORD_FLOATS}
    with open(S.HEADER) as f:
        body = f.read().split('typedef struct vibo_sparse_image {')[1].split('}')[0]
    import re
    fields = re.findall(r'^\s*(?:const\s+)?(\w+)\s*(\*?)\s*(\w+);', body, flags=re.M)
    assert [n for _, _, n in fields] == [n for n, _ in _lib.ViboSparseImage._fields_]
    for (ctype_name, star, _), (_, ct) in zip(fields, _lib.ViboSparseImage._fields_):
        assert ct is (ctypes.c_void_p if star else {'int64_t': ctypes.c_int64}[ctype_name])
    assert ctypes.sizeof(_lib.ViboSparseImage) == 4 * 8 + 7 * ctypes.sizeof(ctypes.c_void_p)


# ---- return codes ----
SUPPORTED = [dict(irt=irt, A=A) for irt in (1, 2, 3) for A in (1, 3, 8)] + [dict(I=1), dict(I=100_000), dict(mask=99), dict(stride=-7),
                                                                           dict(flags=12345)]
REFUSED = [dict(posterior=_lib.POSTERIOR_CONDITIONAL), dict(posterior=_lib.POSTERIOR_GIVEN), dict(n_flows=2), dict(A=9), dict(A=16)]


def _variants(kw):
    for missing in (_lib.MISSING_PRIOR, _lib.MISSING_DROP):
        for reg in ((_lib.REG_SAMPLED,) if kw.get('n_flows') else (_lib.REG_KL, _lib.REG_SAMPLED)):
            d = desc(**{'mask': _lib.MASK_NONE, **kw})
            d.missing_mode, d.reg_mode = missing, reg
            yield d


@pytest.mark.parametrize('kw', SUPPORTED, ids=str)
def test_supported_descriptors_and_their_workspace(kw):
    lib = _lib.load()
    for d in _variants(kw):
        assert lib.vibo_sparse_rows_supported(ctypes.byref(d)) == 1
        D = ops.item_feat_dim(d.irt_model, d.ability_dim)
        up = lambda b: (b + 255) & ~255
        for B, chunks in ((1, 0), (33, 7), (5_000_000, 123_457)):
            d.num_person = B
            records = up(S.person_waves(B) * _lib.SPARSE_RECORD_FLOATS * 4)
            for grad in (0, 1):
                d.want_grad = grad
                assert lib.vibo_sparse_workspace_bytes(ctypes.byref(d), chunks) == records + (up(chunks * D * 4) if grad else 0)


@pytest.mark.parametrize('kw', REFUSED, ids=str)
def test_refusals_return_minus_8_and_name_the_format(kw):
    lib = _lib.load()
    for d in _variants(kw):
        assert lib.vibo_sparse_rows_supported(ctypes.byref(d)) == 0
        assert lib.vibo_sparse_workspace_bytes(ctypes.byref(d), 10) == 0
        for name in ('vibo_sparse_elbo_fwd_bwd', 'vibo_sparse_encode'):
            assert _null_call(getattr(lib, name), d) == -8 and 'sparse rows' in err(), name


def _fake_image(columns=True, P=1000, I=1000):
    """An image whose pointers are never dereferenced: every call below returns before a launch."""
    im = _lib.ViboSparseImage()
    im.num_person, im.num_item, im.nnz, im.num_chunk = P, I, 10, (3 if columns else 0)
    im.row_ptr = im.row_cell = 256
    if columns:
        im.col_ptr = im.col_cell = im.col_chunk = im.chunk_item = im.chunk_first = 256
    return im


def test_the_other_codes_before_anything_is_launched():
    lib = _lib.load()
    fn, p = lib.vibo_sparse_elbo_fwd_bwd, ctypes.c_void_p(256)
    good = desc(B=100, mask=_lib.MASK_NONE)

    def call(d, im, row0=0, ws=p, ws_bytes=1 << 30, table=p):
        return fn(ctypes.byref(d), ctypes.byref(im) if im is not None else None, row0, table, p, p, p, p, p, p, p, p, None, ws, ws_bytes, None)

    bad = desc(B=100, irt=7, mask=_lib.MASK_NONE)
    assert call(bad, _fake_image()) == -3 and 'sparse rows' in err()
    assert call(good, None) == -5 and 'sparse rows' in err()
    assert call(good, _fake_image(), table=None) == -5
    assert call(good, _fake_image(columns=False)) == -8 and 'column side' in err() and 'sparse rows' in err()
    fwd = desc(B=100, mask=_lib.MASK_NONE, grad=0)
    assert call(fwd, _fake_image(columns=False), ws=None) == -7          # (forward only: the row side is enough, next comes the workspace)
    assert call(good, _fake_image(), ws=None) == -7 and 'sparse rows' in err()
    assert call(good, _fake_image(), ws_bytes=16) == -7
    assert call(good, _fake_image(), ws=ctypes.c_void_p(264)) == -7       # not 256-byte aligned
    assert call(good, _fake_image(I=999)) == -3                           # the image's items are not the descriptor's
    assert call(good, _fake_image(), row0=950) == -3                      # persons [950, 1050) of 1000
    assert call(good, _fake_image(), row0=-1) == -3
    assert lib.vibo_sparse_rows_check(None, p, None) == -5
    assert lib.vibo_sparse_rows_check(ctypes.byref(_fake_image()), None, None) == -5
    assert lib.vibo_sparse_encode(ctypes.byref(good), ctypes.byref(_fake_image(columns=False)), 0, None, p, p, None, None) == -5


# ---- builders ----
def _dense_cases():
    g = torch.Generator().manual_seed(3)
    mask = torch.rand(23, 37, generator=g) < 0.3
    mask[5] = False                      # a row with no cell
    mask[:, 11] = False                  # a column with no cell
    mask[7] = True                       # a full row
    resp = torch.where(mask, (torch.rand(23, 37, generator=g) < 0.5).float(), torch.tensor(-1.0))
    return resp, mask


def test_from_dense_round_trip_with_empty_rows_and_columns():
    resp, mask = _dense_cases()
    assert resp.shape[1] % 4 != 0
    rows = SparseRows.from_dense(resp, mask)
    assert (rows.num_person, rows.num_item, rows.nnz) == (23, 37, int(mask.sum())) and rows.shape == (23, 37)
    assert rows.density == int(mask.sum()) / (23 * 37)
    r, m = rows.to_dense()
    assert torch.equal(m, mask) and torch.equal(r, resp)
    r, m = rows.to_dense(range(4, 9))
    assert torch.equal(m, mask[4:9]) and torch.equal(r, resp[4:9])
    view = rows.rows(range(3, 20)).rows(RowBlock(2, 6))          # a view of a view: persons 5..8
    assert (view.row0, view.num_person, view.image_persons) == (5, 4, 23)
    r, m = view.to_dense()
    assert torch.equal(m, mask[5:9]) and torch.equal(r, resp[5:9])
    assert rows.violations() == 0                                 # (host tensors: the mirror)


def test_the_three_constructors_agree_and_both_sides_list_the_same_cells():
    resp, mask = _dense_cases()
    a = SparseRows.from_dense(resp.unsqueeze(2), mask.unsqueeze(2))
    codes = torch.where(mask, (resp == 1).to(torch.uint8), torch.tensor(2, dtype=torch.uint8))
    b = SparseRows.from_cell_codes(codes)
    pi = mask.nonzero()
    shuffle = torch.randperm(pi.shape[0], generator=torch.Generator().manual_seed(1))
    c = SparseRows.from_coo(pi[shuffle, 0], pi[shuffle, 1], resp[mask][shuffle] == 1, 23, 37)
    d = SparseRows.from_arrays(a.row_ptr, a.row_cell, a.col_ptr, a.col_cell, 23, 37)
    for other in (b, c, d):
        for name in ('row_ptr', 'row_cell', 'col_ptr', 'col_cell', 'col_chunk', 'chunk_item', 'chunk_first'):
            assert torch.equal(getattr(a, name), getattr(other, name)), name
    by_row, by_col = S.cells_of(a)
    assert by_row == by_col == {(int(p), int(i), int(resp[p, i] == 1)) for p, i in pi.tolist()}
    cells = (a.row_cell.to(torch.int64) & 0xffffffff) >> 1
    for p in range(23):
        run = cells[a.row_ptr[p]:a.row_ptr[p + 1]]
        assert bool((run[1:] > run[:-1]).all())


def test_from_coo_refuses_cells_outside_the_matrix_and_duplicates():
    p, i, r = torch.tensor([0, 1, 5]), torch.tensor([0, 2, 1]), torch.tensor([1, 0, 1])
    with pytest.raises(ValueError, match='sparse rows'):
        SparseRows.from_coo(p, i, r, 5, 3)
    with pytest.raises(ValueError, match='sparse rows'):
        SparseRows.from_coo(p, torch.tensor([0, 3, 1]), r, 6, 3)
    with pytest.raises(ValueError, match='invariants'):
        SparseRows.from_coo(torch.tensor([0, 1, 1]), torch.tensor([0, 2, 2]), r, 6, 3)      # one cell twice: found by check()


def test_chunk_list_at_every_column_length():
    lengths = [0, 1, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 7]
    resp, mask = S.matrix_with_column_lengths(lengths, 3 * CHUNK + 7, seed=5)
    rows = SparseRows.from_dense(resp, mask)
    n = [0, 1, 1, 1, 2, 4]
    assert rows.col_chunk.tolist() == [0, 0, 1, 2, 3, 5, 9] and rows.num_chunk == 9
    assert rows.chunk_item.dtype == torch.int32 and rows.chunk_item.tolist() == [1, 2, 3, 4, 4, 5, 5, 5, 5]
    col_ptr = rows.col_ptr.tolist()
    assert [col_ptr[i + 1] - col_ptr[i] for i in range(6)] == lengths
    first = rows.chunk_first.tolist()
    for i in range(6):
        c0 = rows.col_chunk[i]
        assert [first[c0 + t] for t in range(n[i])] == [col_ptr[i] + t * CHUNK for t in range(n[i])]
    # every entry of col_cell lies in exactly one chunk, chunks of at most CHUNK entries, in order
    ends = [min(first[c] + CHUNK, col_ptr[rows.chunk_item[c] + 1]) for c in range(9)]
    assert first[0] == 0 and ends[-1] == rows.nnz and all(first[c + 1] == ends[c] for c in range(8))
    assert rows.violations() == 0


def test_host_mirror_of_the_validation_pass_counts_each_kind_of_damage():
    resp, mask = _dense_cases()
    good = SparseRows.from_dense(resp, mask)

    def damaged(**change):
        t = {k: getattr(good, k).clone() for k in ('row_ptr', 'row_cell', 'col_ptr', 'col_cell')}
        for k, f in change.items():
            f(t[k])
        return SparseRows(t['row_ptr'], t['row_cell'], t['col_ptr'], t['col_cell'], 23, 37)

    def flip_right(cells):          # a column-side cell the row side does not have (the answer differs)
        cells[4] ^= 1

    assert sparse.check_host(damaged(col_cell=flip_right)) == 1

    def out_of_range(cells):        # the last cell of row 7 (the full row): item 36 -> item 40
        cells[good.row_ptr[8] - 1] = (40 << 1) | 1

    # the item is out of range (1), and the column side's cell (7, 36) is no longer found (1)
    assert sparse.check_host(damaged(row_cell=out_of_range)) == 2

    def backwards(ptr):
        ptr[3] = ptr[4] + 1
    assert sparse.check_host(damaged(row_ptr=backwards)) >= 1

    def swap(cells):                # the first two cells of row 7: one pair out of order, and a bisection of that row may miss cells
        k = int(good.row_ptr[7])
        cells[k], cells[k + 1] = cells[k + 1].clone(), cells[k].clone()
    assert sparse.check_host(damaged(row_cell=swap)) >= 1
    with pytest.raises(ValueError, match='sparse rows'):
        damaged(col_cell=flip_right).check()

    bad_chunks = SparseRows.from_dense(resp, mask)
    bad_chunks.chunk_first[2] += 1
    bad_chunks.chunk_item[0] = 5
    assert sparse.check_host(bad_chunks) == 2


# ---- dispatch and refusals, with the CPU stand-in ----
@pytest.fixture
def standin():
    restore_dense, restore_sparse = cpu_backend.install(ops), S.install_standin()
    yield
    restore_sparse()
    restore_dense()


def test_backend_has_the_sparse_entries():
    assert ops._BACKEND['sparse_elbo'] is sparse._hip_sparse_elbo and ops._BACKEND['sparse_encode'] is sparse._hip_sparse_encode
    assert ops._BACKEND['sparse_check'] is sparse._hip_sparse_check


@pytest.mark.parametrize('cls,A,drop', [(VIBO_1PL, 1, False), (VIBO_2PL, 3, False), (VIBO_3PL, 2, True)])
def test_model_on_sparse_rows_matches_the_dense_rows(standin, cls, A, drop):
    P, I = 41, 29
    g = torch.Generator().manual_seed(11)
    mask = torch.rand(P, I, generator=g) < 0.4
    mask[:, 0] = True                                  # (every row observes something: --drop-missing needs it)
    resp = torch.where(mask, (torch.rand(P, I, generator=g) < 0.5).float(), torch.tensor(-1.0))
    rows = SparseRows.from_dense(resp, mask)
    torch.manual_seed(5)
    model = cls(A, I, ability_merge='product', replace_missing_with_prior=not drop)
    losses, grads, posts = [], [], []
    for response, m, ri in ((resp, mask, None), (rows, None, None), (rows.rows(range(7, 30)), None, None), (rows, None, RowBlock(7, 30)),
                            (resp[7:30], mask[7:30], None)):
        model.zero_grad(set_to_none=True)
        torch.manual_seed(9)
        loss = model.elbo_step(response, m, annealing_factor=0.6, row_index=ri)
        loss.backward()
        losses.append(float(loss.detach()))
        grads.append({k: p.grad.clone() for k, p in model.named_parameters()})
        torch.manual_seed(10)
        posts.append(model.encode(response, m, row_index=ri)[1:3])
    for a, b in ((0, 1), (4, 2), (4, 3)):
        assert losses[a] == pytest.approx(losses[b], rel=1e-6)
        for k in grads[a]:
            assert torch.allclose(grads[a][k], grads[b][k], rtol=1e-5, atol=1e-6), k
        for x, y in zip(posts[a], posts[b]):
            assert torch.allclose(x, y, rtol=1e-6, atol=1e-6)
    assert losses[0] != pytest.approx(losses[4], rel=1e-3)        # the range was honoured: other persons, another loss


def test_ops_refuse_what_the_format_does_not_cover(standin):
    resp, mask = _dense_cases()
    rows = SparseRows.from_dense(resp, mask)
    I = rows.num_item

    def call(spec, row_index=None, reducer=None, mask_arg=None, B=23):
        A = min(spec.ability_dim, 8)
        table = torch.zeros(spec.table_shape(I, B))
        return ops.fused_elbo(spec, table, torch.zeros(I, spec.item_dim), None, rows, mask_arg, torch.zeros(B, A), row_index=row_index,
                              reducer=reducer)

    plain = ops.ElboSpec(irt_model=2, ability_dim=2)
    assert call(plain)[0].shape == ()
    assert call(plain, row_index=range(3, 9), B=6)[3].shape == (6, 2)
    for spec in (ops.ElboSpec(2, 2, conditional=True), ops.ElboSpec(2, 2, given=True), ops.ElboSpec(2, 2, n_flows=2), ops.ElboSpec(2, 9)):
        with pytest.raises(NotImplementedError, match='sparse rows'):
            call(spec)
        with pytest.raises(NotImplementedError, match='sparse rows'):
            ops.encode_posterior(spec, torch.zeros(2, 4), rows, None)
    with pytest.raises(NotImplementedError, match='sparse rows.*tensor row_index'):
        call(plain, row_index=torch.arange(6), B=6)
    with pytest.raises(NotImplementedError, match='sparse rows'):
        call(plain, row_index=range(0, 12, 2), B=6)
    with pytest.raises(NotImplementedError, match='sparse rows.*sharding'):
        call(plain, reducer=lambda flat: None)
    with pytest.raises(ValueError, match='mask=None'):
        call(plain, mask_arg=mask)
    with pytest.raises(ValueError, match='sparse rows'):
        call(plain, row_index=range(20, 30), B=10)
    with pytest.raises(NotImplementedError, match='sparse rows'):
        ops.encode_posterior(plain, torch.zeros(2, 4), rows, None, row_index=torch.arange(4))
