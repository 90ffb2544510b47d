"""The row-driven item pass of gathered minibatches on sparse response rows, on the GPU: vibo_sparse_elbo_fwd_bwd_gather_rows of
include/vibo_hip_sparse_row_driven.h against the fp64 oracle on resp[idx], mask[idx] (gpu_common.compare_raw's bounds: 2e-5 on heads and
per-person outputs, TOL_GRAD on gradients), the header's four bit-level statements, an image without a column side, input that cannot be
trusted (the index, the row side's items, the caller's max_row_cells, the cell capacity), keys wider than 32 bits, and three Adam steps
through the module path.  Every test calls the new entry point, directly or through item_pass='rows'.

Image A is test_gpu_sparse_gather.py's: P = 1 100 persons x I = 40 items; item 0 is answered by every person who answers anything
(1 095 entries: a segment of 18 lane trips for one wave), item 1 by one person, item 2 by nobody; five rows are empty, three hold one
cell, the longest 36.  Image B (I = 140) has rows of 63, 64, 65 and 130 cells.  Every test leaves the map all NO_SLOT."""
import copy
import ctypes
import math

import pytest
import torch

import sparse_rows_common as S
from gpu_common import TOL_GRAD, check, compare_raw, dev
from conftest import rel_err
from vibo_amd import _lib, ops, sparse
from vibo_amd.sparse import RowGather, SparseRows
from vibo_amd.torch_core.models import VIBO_2PL

pytestmark = pytest.mark.gpu
KL, SAMPLED = _lib.REG_KL, _lib.REG_SAMPLED
NO_SLOT = _lib.SPARSE_NO_SLOT
P, I = 1100, 40
EMPTY = (3, 64, 500, 777, 1098)
ONE_CELL = (5, 600, 1001)              # rows of one cell (item 0)
LONE = 333                             # the one person who answers item 1


def _image():
    lengths = [(7 * r + 5) % 36 + 1 for r in range(P)]
    resp, mask = S.matrix_with_row_lengths(lengths, I, seed=121)
    g = torch.Generator().manual_seed(122)
    mask[:, 0] = True
    mask[:, 1] = False
    mask[LONE, 1] = True
    mask[:, 2] = False
    mask[list(ONE_CELL)] = False
    mask[list(ONE_CELL), 0] = True
    mask[list(EMPTY)] = False
    resp = torch.where(mask, (torch.rand(P, I, generator=g) < 0.5).float(), torch.tensor(-1.0))
    return resp, mask


@pytest.fixture(scope='module')
def image():
    resp, mask = _image()
    rows = SparseRows.from_dense(resp.to(dev()), mask.to(dev()))
    n = mask.sum(1)
    assert (n[list(EMPTY)] == 0).all() and (n[list(ONE_CELL)] == 1).all() and n[0] > 1 and n[P - 1] > 1
    per_item = mask.sum(0)
    assert per_item[0] == P - len(EMPTY) and per_item[1] == 1 and per_item[2] == 0
    assert math.ceil(int(per_item[0]) / 64) == 18 and rows.max_row_cells == int(n.max()) == 36
    return resp, mask, rows


@pytest.fixture(autouse=True)
def map_is_clear_after_every_call(image):
    yield
    torch.cuda.synchronize()
    slot = image[2]._slot[0]
    assert slot is None or bool((slot == NO_SLOT).all()), 'a gathered call left entries in the map'


def launch(spec, view, table, item, eps, reg_mode=KL, want_grad=True):
    """The module's own launch path on a view; item_pass='rows' views go to the new entry point."""
    d = dev()
    raw = sparse._hip_sparse_elbo(spec, view, table.to(d).contiguous(), item.to(d).contiguous(), eps.to(d).contiguous(), reg_mode, want_grad)
    torch.cuda.synchronize()
    slot = view._slot[0]
    assert slot is None or bool((slot == NO_SLOT).all())
    return raw


def by_rows(rows, idx):
    return rows.take(idx.to(dev()), item_pass='rows')


def by_columns(rows, idx):
    return rows.take(idx.to(dev()))


def direct(name, spec, rows, im, idx, max_row, table, item, eps, reg_mode=KL):
    """One of the two gathered entry points called by hand, with gradients, on the image struct `im` -> (return code, ops.RawElbo):
    for what the module path would not pass (an image without its column side to the column-driven call, an understated max_row_cells)."""
    d, lib = dev(), _lib.load()
    B, A, D = idx.numel(), spec.ability_dim, spec.item_dim
    table, item, eps, index = table.to(d).contiguous(), item.to(d).contiguous(), eps.to(d).contiguous(), idx.to(d).contiguous()
    n_table, n_item = table.numel(), rows.num_item * D
    flat = torch.zeros(_lib.NUM_SCALARS + 2 * n_table + n_item, dtype=torch.float32, device=d)
    post = torch.zeros(3, B, A, dtype=torch.float32, device=d)
    desc = sparse._desc(spec, B, rows.num_item, reg_mode, True)
    by_row = name.endswith('_rows')
    if by_row:
        ws_bytes = lib.vibo_sparse_row_driven_workspace_bytes(ctypes.byref(desc), ctypes.c_int64(rows.num_item), ctypes.c_int64(rows.image_persons),
                                                              ctypes.c_int64(max_row))
    else:
        ws_bytes = lib.vibo_sparse_workspace_bytes(ctypes.byref(desc), ctypes.c_int64(rows.num_chunk))
    assert ws_bytes > 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=d)
    vp, fbase = ctypes.c_void_p, flat.data_ptr()
    head = (ctypes.byref(desc), ctypes.byref(im), ops._ptr(index), ops._ptr(rows.slot_map())) + ((ctypes.c_int64(max_row),) if by_row else ())
    rc = getattr(lib, name)(*head, ops._ptr(table), ops._ptr(item), ops._ptr(eps), vp(fbase), ops._ptr(post[0]), ops._ptr(post[1]),
                            ops._ptr(post[2]), vp(fbase + 4 * _lib.NUM_SCALARS), vp(fbase + 4 * (_lib.NUM_SCALARS + 2 * n_table)),
                            ops._ptr(rows.bad_cells), ops._ptr(ws), ctypes.c_size_t(ws_bytes), ops._stream(d))
    torch.cuda.synchronize()
    assert bool((rows.slot_map() == NO_SLOT).all())
    return rc, ops.RawElbo(flat=flat, n_table=n_table, n_item=n_item, n_flow=0, table_shape=tuple(table.shape), ability_mu=post[0],
                           ability_logvar=post[1], ability=post[2], ability_k=None, ability_ladj=None)


def against_oracle(spec, rows, resp, mask, idx, table, item, eps, reg_mode=KL, view=None):
    """One row-driven launch on the persons idx compared with the oracle on the dense rows resp[idx], mask[idx]."""
    before = rows.bad_index_count
    ref = S.oracle(spec, table, item, resp[idx], mask[idx], eps, reg_mode)
    raw = launch(spec, by_rows(rows, idx) if view is None else view, table, item, eps, reg_mode)
    sc = raw.scalars.cpu().double()
    print('heads B=%d' % idx.numel(), ' '.join(f'{k} {float(sc[j]):.6f} ref {float(ref[k]):.6f}' for k, j in (
        ('ll', _lib.S_LL), ('reg', _lib.S_REG), ('kl_ability', _lib.S_KL), ('logq0', _lib.S_LOGQ0), ('logp', _lib.S_LOGP))))
    compare_raw(raw, ref, (rows.num_item, spec.item_dim))
    assert float(raw.scalars[_lib.S_NOBS]) == float(mask[idx].sum()) and float(raw.scalars[_lib.S_LADJ]) == 0.0
    empty = mask[idx].sum(0) == 0
    assert bool(empty.any())
    assert bool((raw.grad_item((rows.num_item, spec.item_dim))[empty.to(dev())] == 0).all()), 'an item with no cell in the batch: exact zeros'
    assert rows.bad_index_count == before
    return raw


def index_cases(drop, seed):
    """The four index vectors of the column-driven gathered test: 70 persons of a permutation, one person, every person permuted, and
    one that holds persons 0 and P - 1.  Under VIBO_MISSING_DROP a row without a cell has no posterior: the empty rows stay out."""
    g = torch.Generator().manual_seed(seed)
    perm = torch.randperm(P, generator=g)
    if drop:
        perm = perm[~torch.isin(perm, torch.tensor(EMPTY))]
    ends = torch.tensor([P - 1, 17, 0, LONE, 250])
    return {'70 of a permutation': perm[:70], 'one person': perm[70:71], 'every person': perm, 'the ends': ends}


# ---- 1. the oracle ----
@pytest.mark.parametrize('reg', [KL, SAMPLED], ids=['kl', 'sampled'])
@pytest.mark.parametrize('drop', [False, True], ids=['prior', 'drop'])
@pytest.mark.parametrize('A', [1, 3, 8])
@pytest.mark.parametrize('irt', [1, 2, 3])
def test_against_the_oracle(image, irt, A, drop, reg):
    resp, mask, rows = image
    spec = ops.ElboSpec(irt_model=irt, ability_dim=A, drop_missing=drop)
    for n, (name, idx) in enumerate(index_cases(drop, seed=1000 * irt + 10 * A + drop).items()):
        table, item, eps = S.problem(irt, A, I, idx.numel(), seed=100 * irt + A + n)
        # compare_raw bounds a head by 2e-5 of the head itself, so a head must not be a sum that cancels: with S.problem's experts
        # (log-variance about 0) and rows of about 19 cells a person's logq0 term has mean 0.05 under VIBO_MISSING_DROP -- over 1 095
        # persons x A dims a random walk about zero against an fp32 rounding of 1e-4 .. 4e-4.  Experts sharper by e^2 move the term's
        # mean to about 1 and the head to its terms' scale (the conditioning, and the reason, of test_gpu_sparse_gather.py).
        table[:, A:] -= 2.0
        against_oracle(spec, rows, resp, mask, idx, table, item, eps, reg)


# rows of every length at which a lane loop over a row's cells takes another number of trips
LONG_LENGTHS = {0: 0, 1: 1, 2: 63, 3: 64, 4: 65, 5: 130, 640: 130, 1099: 65}
LONG_I = 140


@pytest.fixture(scope='module')
def long_image():
    lengths = [LONG_LENGTHS.get(r, (11 * r) % 90 + 1) for r in range(P)]
    resp, mask = S.matrix_with_row_lengths(lengths, LONG_I, seed=131)
    assert mask.sum(1).tolist() == lengths
    rows = SparseRows.from_dense(resp.to(dev()), mask.to(dev()))
    assert rows.max_row_cells == 130
    return resp, mask, rows


@pytest.mark.parametrize('irt,A,reg', [(2, 3, SAMPLED), (3, 8, KL), (1, 1, KL), (2, 8, KL)])
def test_row_lengths_around_the_wave_width(long_image, irt, A, reg):
    resp, mask, rows = long_image
    spec = ops.ElboSpec(irt_model=irt, ability_dim=A)
    g = torch.Generator().manual_seed(41)
    pool = torch.tensor([r for r in range(P) if r not in LONG_LENGTHS])
    idx = torch.cat([torch.tensor(list(LONG_LENGTHS)), pool[torch.randperm(pool.numel(), generator=g)[:62]]])
    idx = idx[torch.randperm(70, generator=g)]
    assert idx.numel() == 70 and idx.unique().numel() == 70 and set(mask[idx].sum(1).tolist()) >= {0, 1, 63, 64, 65, 130}
    table, item, eps = S.problem(irt, A, LONG_I, 70, seed=42 + irt)
    ref = S.oracle(spec, table, item, resp[idx], mask[idx], eps, reg)
    raw = launch(spec, by_rows(rows, idx), table, item, eps, reg)
    compare_raw(raw, ref, (LONG_I, spec.item_dim))
    assert float(raw.scalars[_lib.S_NOBS]) == float(mask[idx].sum()) and rows.bad_index_count == 0


# ---- 2. bits ----
def same_person_pass_bits(a, b):
    assert torch.equal(a.scalars, b.scalars)
    for k in ('ability_mu', 'ability_logvar', 'ability'):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    for s in range(2):
        assert torch.equal(a.grad_table(s), b.grad_table(s)), s


def test_two_launches_agree_bit_for_bit(image):
    _, _, rows = image
    spec = ops.ElboSpec(irt_model=3, ability_dim=8)
    idx = index_cases(False, seed=61)['every person'][:700]
    table, item, eps = S.problem(3, 8, I, 700, seed=62)
    a, b = launch(spec, by_rows(rows, idx), table, item, eps), launch(spec, by_rows(rows, idx.clone()), table, item, eps)
    assert torch.equal(a.flat, b.flat)
    same_person_pass_bits(a, b)
    assert bool((a.grad_item((I, spec.item_dim)) != 0).any())


@pytest.mark.parametrize('irt,A,reg', [(2, 3, SAMPLED), (3, 8, KL), (1, 1, KL)])
@pytest.mark.parametrize('case', ['70 of a permutation', 'every person', 'the ends'])
def test_person_pass_outputs_are_the_column_driven_calls_bits_and_grad_item_agrees_to_rounding(image, case, irt, A, reg):
    _, _, rows = image
    spec = ops.ElboSpec(irt_model=irt, ability_dim=A)
    idx = index_cases(False, seed=71)[case]
    table, item, eps = S.problem(irt, A, I, idx.numel(), seed=72)
    r, c = launch(spec, by_rows(rows, idx), table, item, eps, reg), launch(spec, by_columns(rows, idx), table, item, eps, reg)
    same_person_pass_bits(r, c)
    shape = (I, spec.item_dim)
    check('row-driven grad_item against the column-driven call', rel_err(r.grad_item(shape).cpu(), c.grad_item(shape).cpu().double()), TOL_GRAD)
    zero = (c.grad_item(shape) == 0).all(1)
    assert bool(zero.any()) and bool((r.grad_item(shape)[zero] == 0).all())
    # forward only: the column-driven call's path, the same bits
    fr, fc = (launch(spec, v, table, item, eps, reg, want_grad=False) for v in (by_rows(rows, idx), by_columns(rows, idx)))
    assert torch.equal(fr.scalars, fc.scalars) and torch.equal(fr.ability, fc.ability) and torch.equal(fr.scalars, r.scalars)


@pytest.mark.parametrize('irt,A', [(2, 3), (3, 8)])
@pytest.mark.parametrize('case', ['70 of a permutation', 'every person'])
def test_grad_item_has_the_same_bits_under_any_order_of_the_batch(image, case, irt, A):
    """person_index and the rows of eps permuted together: the same set of persons, the same theta per person, hence the same sorted keys
    and the same lanes -- an arrival order that leaked into a sum would show here."""
    _, _, rows = image
    spec = ops.ElboSpec(irt_model=irt, ability_dim=A)
    idx = index_cases(False, seed=81)[case]
    B = idx.numel()
    table, item, eps = S.problem(irt, A, I, B, seed=82)
    base = launch(spec, by_rows(rows, idx), table, item, eps)
    shape = (I, spec.item_dim)
    assert bool((base.grad_item(shape)[0] != 0).any())
    g = torch.Generator().manual_seed(83)
    for name, perm in (('reversed', torch.arange(B - 1, -1, -1)), ('shuffled', torch.randperm(B, generator=g))):
        assert not torch.equal(perm, torch.arange(B))
        got = launch(spec, by_rows(rows, idx[perm]), table, item, eps[perm])
        assert torch.equal(got.grad_item(shape), base.grad_item(shape)), name
        for k in ('ability_mu', 'ability_logvar', 'ability'):
            assert torch.equal(getattr(got, k), getattr(base, k)[perm.to(dev())]), (name, k)


# ---- 3. no column side ----
def test_an_image_without_a_column_side_serves_gradients(image):
    resp, mask, rows = image
    spec = ops.ElboSpec(irt_model=2, ability_dim=3)
    idx = index_cases(False, seed=91)['70 of a permutation']
    table, item, eps = S.problem(2, 3, I, 70, seed=92)
    im = rows.image(columns=False)
    assert im.col_ptr is None and im.col_cell is None and im.num_chunk == 0
    rc, raw = direct('vibo_sparse_elbo_fwd_bwd_gather_rows', spec, rows, im, idx, rows.max_row_cells, table, item, eps)
    assert rc == 0
    compare_raw(raw, S.oracle(spec, table, item, resp[idx], mask[idx], eps), (I, spec.item_dim))
    empty = (mask[idx].sum(0) == 0).to(dev())
    assert bool(empty.any()) and bool((raw.grad_item((I, spec.item_dim))[empty] == 0).all())
    # the module path passes no column side either: the same bits
    assert torch.equal(launch(spec, by_rows(rows, idx), table, item, eps).flat, raw.flat)
    # the column-driven call refuses the same image
    rc, _ = direct('vibo_sparse_elbo_fwd_bwd_gather', spec, rows, im, idx, 0, table, item, eps)
    err = _lib.load().vibo_last_error_string().decode()
    assert rc == -8 and 'column side' in err and 'sparse rows' in err


# ---- 4. input that cannot be trusted ----
def test_out_of_range_and_repeated_entries_are_skipped_zeroed_and_counted(image):
    resp, mask, rows = image
    spec = ops.ElboSpec(irt_model=2, ability_dim=3)
    good = index_cases(False, seed=101)['70 of a permutation']
    idx = good.clone().tolist()
    idx.insert(10, P)                          # one past the image
    idx.insert(30, -1)
    idx.insert(55, idx[4])                     # a person an earlier row owns already
    idx = torch.tensor(idx)
    bad_rows = [10, 30, 55]
    keep = torch.ones(73, dtype=torch.bool)
    keep[bad_rows] = False
    assert torch.equal(idx[keep], good)
    table, item, eps = S.problem(2, 3, I, 73, seed=102)
    before = rows.bad_index_count
    dirty = launch(spec, by_rows(rows, idx), table, item, eps)
    assert rows.bad_index_count == before + 3
    column = launch(spec, by_columns(rows, idx), table, item, eps)
    assert rows.bad_index_count == before + 6          # the column-driven call counts the same three
    same_person_pass_bits(dirty, column)
    clean = launch(spec, by_rows(rows, good), table, item, eps[keep])
    assert rows.bad_index_count == before + 6
    for k in ('ability_mu', 'ability_logvar', 'ability'):
        got = getattr(dirty, k)
        assert bool((got[bad_rows] == 0).all()), k
        assert torch.equal(got[keep.to(dev())], getattr(clean, k)), k
    shape = (I, spec.item_dim)
    # the same set of live persons with the same thetas: the rows that are not live leave no key behind
    assert torch.equal(dirty.grad_item(shape), clean.grad_item(shape))
    compare_raw(clean, S.oracle(spec, table, item, resp[good], mask[good], eps[keep]), shape)


def test_row_side_cells_that_name_no_item_are_skipped_and_counted_once(image):
    resp, mask, rows = image
    spec = ops.ElboSpec(irt_model=2, ability_dim=3)
    idx = index_cases(False, seed=111)['70 of a permutation']
    victims = [int(q) for q in idx[[0, 5, 40]] if mask[q].sum() > 1]
    assert len(victims) >= 2
    row_cell, masked = rows.row_cell.clone(), mask.clone()
    for n, q in enumerate(victims):            # the person's first cell: its item becomes I + 3, or the largest a cell can hold
        k = int(rows.row_ptr[q])
        first = int(mask[q].nonzero()[0])
        assert (int(row_cell[k]) & 0xffffffff) >> 1 == first
        row_cell[k] = ((I + 3) << 1 | (int(row_cell[k]) & 1)) if n else -1          # (-1: the bits 0xffffffff, item 2^31 - 1)
        masked[q, first] = False
    bad = SparseRows(rows.row_ptr, row_cell, rows.col_ptr, rows.col_cell, P, I)      # (no check(): the point is an image that fails it)
    table, item, eps = S.problem(2, 3, I, 70, seed=112)
    raw = launch(spec, by_rows(bad, idx), table, item, eps)
    assert bad.bad_index_count == len(victims)                                       # counted by the person pass, not again by the emit
    compare_raw(raw, S.oracle(spec, table, item, torch.where(masked, resp, torch.tensor(-1.0))[idx], masked[idx], eps), (I, spec.item_dim))
    column = launch(spec, by_columns(bad, idx), table, item, eps)
    assert bad.bad_index_count == 2 * len(victims)                                   # the column-driven call: the same count
    same_person_pass_bits(raw, column)
    assert bool((bad.slot_map() == NO_SLOT).all())


def test_an_understated_max_row_cells_cuts_the_rows_counts_the_cut_and_returns_zero(image):
    resp, mask, rows = image
    spec = ops.ElboSpec(irt_model=2, ability_dim=3)
    idx = index_cases(False, seed=121)['70 of a permutation']
    table, item, eps = S.problem(2, 3, I, 70, seed=122)
    CUT = 20
    lengths = (rows.row_ptr[1:] - rows.row_ptr[:-1]).cpu()[idx]                      # from row_ptr, on the host
    n_cut = int((lengths - CUT).clamp_min(0).sum())
    assert int(lengths.max()) > CUT and n_cut > 0
    kept = mask[idx].clone()                                                         # a row's first CUT cells in item order stay
    kept &= kept.long().cumsum(1) <= CUT
    assert int(mask[idx].sum() - kept.sum()) == n_cut
    before = rows.bad_index_count
    rc, raw = direct('vibo_sparse_elbo_fwd_bwd_gather_rows', spec, rows, rows.image(), idx, CUT, table, item, eps)
    assert rc == 0 and rows.bad_index_count == before + n_cut
    # the person pass sees whole rows: everything but grad_item is the full call's
    full = launch(spec, by_rows(rows, idx), table, item, eps)
    same_person_pass_bits(raw, full)
    # grad_item: the oracle on the matrix without the cut cells, with the noise that gives every person the full rows' theta there
    ref_full = S.oracle(spec, table, item, resp[idx], mask[idx], eps)
    resp_kept = torch.where(kept, resp[idx], torch.tensor(-1.0))
    ref_kept = S.oracle(spec, table, item, resp_kept, kept, eps)
    eps_kept = (ref_full['ability'] - ref_kept['ability_mu']) / (0.5 * ref_kept['ability_logvar']).exp()
    ref = S.oracle(spec, table, item, resp_kept, kept, eps_kept)
    assert (ref['ability'] - ref_full['ability']).abs().max() < 1e-12
    shape = (I, spec.item_dim)
    check('g_item of the kept cells', rel_err(raw.grad_item(shape).cpu(), ref['g_item']), TOL_GRAD)
    assert rel_err(full.grad_item(shape).cpu(), ref['g_item']) > 10 * TOL_GRAD      # (the cut is visible: the test would see it missing)


def test_a_cell_capacity_of_two_to_the_31_is_refused_before_any_launch():
    lib = _lib.load()
    d = sparse._desc(ops.ElboSpec(irt_model=2, ability_dim=2), 1 << 16, 1000, KL, True)

    def size(max_row):
        return lib.vibo_sparse_row_driven_workspace_bytes(ctypes.byref(d), ctypes.c_int64(1000), ctypes.c_int64(1 << 20), ctypes.c_int64(max_row))

    assert size((1 << 15) - 1) > 0 and size(1 << 15) == 0
    rc = lib.vibo_sparse_elbo_fwd_bwd_gather_rows(ctypes.byref(d), None, None, None, ctypes.c_int64(1 << 15), *([None] * 11), 0, None)
    err = lib.vibo_last_error_string().decode()
    assert rc == -8 and 'sparse rows' in err and 'vibo_sparse_elbo_fwd_bwd_gather' in err and 'column-driven' in err


# ---- 5. keys wider than 32 bits ----
def test_keys_wider_than_32_bits():
    Pw, Iw, A, per_row, B = 40_000, 70_000, 2, 8, 33
    assert sparse.key_layout(Pw, Iw)[:2] == (16, 34)
    g = torch.Generator().manual_seed(131)
    first = torch.randint(0, Iw, (Pw, 1), generator=g)
    item_of = (first + 8747 * torch.arange(per_row).unsqueeze(0)) % Iw                # eight different items per person
    person_of = torch.arange(Pw).unsqueeze(1).expand(Pw, per_row)
    right = torch.rand(Pw, per_row, generator=g) < 0.5
    rows = SparseRows.from_coo(person_of.to(dev()), item_of.to(dev()), right.to(dev()), Pw, Iw)
    assert rows.max_row_cells == per_row
    idx = torch.randperm(Pw, generator=g)[:B]
    idx[0], idx[1] = Pw - 1, 0                                                        # the largest person of the key, and the smallest
    assert idx.unique().numel() == B
    resp = torch.full((B, Iw), -1.0)                                                  # those rows alone, from the COO vectors
    mask = torch.zeros(B, Iw, dtype=torch.bool)
    r = torch.arange(B).unsqueeze(1).expand(B, per_row)
    resp[r, item_of[idx]] = right[idx].float()
    mask[r, item_of[idx]] = True
    assert mask.sum(1).tolist() == [per_row] * B
    spec = ops.ElboSpec(irt_model=2, ability_dim=A)
    table, item, eps = S.problem(2, A, Iw, B, seed=132)
    view = by_rows(rows, idx)
    raw = against_oracle(spec, rows, resp, mask, torch.arange(B), table, item, eps, view=view)
    touched = mask.any(0).to(dev())
    assert bool((raw.grad_item((Iw, spec.item_dim))[touched] != 0).any(1).all())      # every item of the batch got its row
    assert bool((rows.slot_map() == NO_SLOT).all())


# ---- 6. autograd end to end ----
def test_three_adam_steps_follow_the_dense_row_index_steps():
    Pm, Im, A, bs = 600, 120, 2, 200
    g = torch.Generator().manual_seed(91)
    mask = torch.rand(Pm, Im, generator=g) < 0.25
    resp = torch.where(mask, (torch.rand(Pm, Im, generator=g) < 0.5).float(), torch.tensor(-1.0))
    d = dev()
    rows = SparseRows.from_dense(resp.to(d), mask.to(d))
    r_d, m_d = ops.pad_rows(resp.to(d), mask.to(d))
    torch.manual_seed(3)
    dense_model = VIBO_2PL(A, Im, ability_merge='product').to(d)
    sparse_model = copy.deepcopy(dense_model)
    order = torch.randperm(Pm, generator=g).to(d)

    def step(model, response, m, ri):
        model.zero_grad(set_to_none=True)
        loss = model.elbo_step(response, m, annealing_factor=0.8, row_index=ri)
        loss.backward()
        return loss

    opt_a = torch.optim.Adam(dense_model.parameters(), lr=5e-3)
    opt_b = torch.optim.Adam(sparse_model.parameters(), lr=5e-3)
    for k in range(3):
        idx = order[k * bs:(k + 1) * bs]
        torch.manual_seed(10 + k)
        step(dense_model, r_d, m_d, idx)
        opt_a.step()
        torch.manual_seed(10 + k)
        step(sparse_model, rows, None, RowGather(idx, item_pass='rows'))
        opt_b.step()
    for (k, pa), (_, pb) in zip(dense_model.named_parameters(), sparse_model.named_parameters()):
        check(f'row-driven adam x3 {k}', rel_err(pb.detach().cpu(), pa.detach().cpu()), TOL_GRAD)
    assert rows.bad_index_count == 0 and bool((rows.slot_map() == NO_SLOT).all())
    assert rows._max_row[0] == int(mask.sum(1).max())          # the row-driven call was the one taken
