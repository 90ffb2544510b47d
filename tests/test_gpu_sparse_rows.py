"""Sparse response rows on the GPU: the ELBO call, the encode call and the validation pass of include/vibo_hip_sparse_rows.h
against the fp64 oracle on the densified rows (gpu_common.compare_raw's bounds: 2e-5 on heads and per-person outputs, TOL_GRAD on
gradients), at every row and column shape where the passes take another path, over person ranges, past the dense formats' item
ceiling, bit for bit across launches, with planted out-of-range cells that stay inside their allocation, and through autograd."""
import copy
import ctypes

import pytest
import torch

import sparse_rows_common as S
from gpu_common import TOL_ELBO, TOL_GRAD, check, compare_raw, dev, launch_elbo
from conftest import rel_err
from row_format_common import desc
from vibo_amd import _lib, ops, sparse
from vibo_amd.sparse import RowBlock, SparseRows
from vibo_amd.torch_core.models import VIBO_2PL

pytestmark = pytest.mark.gpu
CHUNK = S.CHUNK
KL, SAMPLED = _lib.REG_KL, _lib.REG_SAMPLED


def launch(spec, rows, table, item, eps, reg_mode=KL, want_grad=True):
    d = dev()
    raw = sparse._hip_sparse_elbo(spec, rows, table.to(d).contiguous(), item.to(d).contiguous(), eps.to(d).contiguous(), reg_mode, want_grad)
    torch.cuda.synchronize()
    return raw


def against_oracle(spec, rows, resp, mask, table, item, eps, reg_mode=KL, want_grad=True):
    """One launch on the view `rows` compared with the oracle on the dense rows (resp, mask) of the same persons."""
    ref = S.oracle(spec, table, item, resp, mask, eps, reg_mode, want_grad)
    raw = launch(spec, rows, table, item, eps, reg_mode, want_grad)
    compare_raw(raw, ref, (rows.num_item, spec.item_dim), want_grad=want_grad)
    assert float(raw.scalars[_lib.S_NOBS]) == float(mask.sum()) and float(raw.scalars[_lib.S_LADJ]) == 0.0
    if want_grad:
        empty = mask.sum(0) == 0
        assert bool((raw.grad_item((rows.num_item, spec.item_dim))[empty.to(dev())] == 0).all()), 'an item with no cell in range: exact zeros'
    assert rows.bad_index_count == 0
    return raw


# ---- row shapes ----
ROW_LENGTHS = [0, 1, 63, 64, 65, 129, 130] + [7, 20, 33, 2, 90, 11, 5, 48] * 4 + [9]
ROW_I = 130


@pytest.fixture(scope='module')
def row_image():
    resp, mask = S.matrix_with_row_lengths(ROW_LENGTHS, ROW_I, seed=21)
    assert mask.sum(1).tolist() == ROW_LENGTHS
    return resp, mask, SparseRows.from_dense(resp.to(dev()), mask.to(dev()))


def test_every_wave_of_the_person_pass_takes_two_rows():
    for B in (len(ROW_LENGTHS), len(ROW_LENGTHS) - 1):
        assert all(S.rows_of_wave(B, w) >= 2 for w in range(S.person_waves(B)))


@pytest.mark.parametrize('irt,A,reg,drop,grad', [(1, 1, KL, False, True), (2, 3, SAMPLED, True, True), (3, 8, KL, False, True),
                                                 (2, 8, SAMPLED, False, False), (3, 1, SAMPLED, True, True), (1, 3, KL, True, False),
                                                 (2, 1, KL, False, True), (3, 3, SAMPLED, False, True), (1, 8, SAMPLED, False, True),
                                                 (2, 2, KL, True, True), (3, 5, KL, False, False)])
def test_row_shapes(row_image, irt, A, reg, drop, grad):
    resp, mask, rows = row_image
    first = 1 if drop else 0              # (the row without a cell has no posterior under VIBO_MISSING_DROP)
    P = len(ROW_LENGTHS)
    spec = ops.ElboSpec(irt_model=irt, ability_dim=A, drop_missing=drop)
    table, item, eps = S.problem(irt, A, ROW_I, P - first, seed=100 * irt + A)
    against_oracle(spec, rows.rows(range(first, P)), resp[first:], mask[first:], table, item, eps, reg, grad)
    amu, alv = sparse._hip_sparse_encode(spec, rows.rows(range(first, P)), table.to(dev()))
    ref = S.oracle(spec, table, item, resp[first:], mask[first:], eps, reg, want_grad=False)
    for got, want in ((amu, ref['ability_mu']), (alv, ref['ability_logvar'])):
        assert (got.cpu() - want.float()).abs().max() < 2e-5 * max(1.0, float(want.abs().max()))


# ---- column shapes and ranges ----
COL_P = 2 * CHUNK + 1
COL_LENGTHS = [COL_P, 0, 1, CHUNK, CHUNK + 1, 300, 17]


@pytest.fixture(scope='module')
def col_image():
    resp, mask = S.matrix_with_column_lengths(COL_LENGTHS, COL_P, seed=22)
    rows = SparseRows.from_dense(resp.to(dev()), mask.to(dev()))
    assert (rows.col_chunk[1:] - rows.col_chunk[:-1]).tolist() == [3, 0, 1, 1, 2, 1, 1]
    return resp, mask, rows


@pytest.mark.parametrize('irt,A', [(2, 2), (3, 4), (1, 1)])
def test_column_shapes(col_image, irt, A):
    resp, mask, rows = col_image
    spec = ops.ElboSpec(irt_model=irt, ability_dim=A)
    table, item, eps = S.problem(irt, A, len(COL_LENGTHS), COL_P, seed=31 + irt)
    raw = against_oracle(spec, rows, resp, mask, table, item, eps)
    assert bool((raw.grad_item((len(COL_LENGTHS), spec.item_dim))[1] == 0).all())


@pytest.mark.parametrize('a,b', [(0, COL_P), (37, 37 + 64), (COL_P - 5, COL_P), (500, 501)])
def test_ranges(col_image, a, b):
    resp, mask, rows = col_image
    spec = ops.ElboSpec(irt_model=2, ability_dim=3)
    table, item, eps = S.problem(2, 3, len(COL_LENGTHS), b - a, seed=41)
    against_oracle(spec, rows.rows(range(a, b)), resp[a:b], mask[a:b], table, item, eps, SAMPLED)


# ---- past the dense formats' ceiling ----
def test_past_the_dense_ceiling():
    P, I, A = 300, 40_000, 2
    lib = _lib.load()
    # the dense fast path (cell codes) on this shape: refused before anything is launched or a pointer is read (32 767 items)
    p = ctypes.c_void_p(256)
    assert lib.vibo_elbo_fwd_bwd(ctypes.byref(desc(B=P, I=I, A=A, mask=_lib.MASK_CODES)), None, p, None, p, p, p, None, p, p, p, p, None, None,
                                 p, p, None, p, 1 << 30, None) == -8
    assert '32767 items' in lib.vibo_last_error_string().decode()
    g = torch.Generator().manual_seed(51)
    item_of = torch.stack([torch.randperm(I, generator=g)[:30] for _ in range(P)])
    person_of = torch.arange(P).unsqueeze(1).expand(P, 30)
    right = torch.rand(P, 30, generator=g) < 0.5
    rows = SparseRows.from_coo(person_of.to(dev()), item_of.to(dev()), right.to(dev()), P, I)
    assert rows.nnz == 30 * P
    resp, mask = rows.to_dense()
    spec = ops.ElboSpec(irt_model=2, ability_dim=A)
    table, item, eps = S.problem(2, A, I, P, seed=52)
    against_oracle(spec, rows, resp.cpu(), mask.cpu(), table, item, eps)


# ---- reproducibility ----
def test_two_launches_and_a_rebuilt_image_agree_bit_for_bit(col_image):
    resp, mask, rows = col_image
    spec = ops.ElboSpec(irt_model=3, ability_dim=8)
    table, item, eps = S.problem(3, 8, len(COL_LENGTHS), COL_P, seed=61)
    rebuilt = SparseRows.from_dense(resp.to(dev()), mask.to(dev()))
    a, b, c = launch(spec, rows, table, item, eps), launch(spec, rows, table, item, eps), launch(spec, rebuilt, table, item, eps)
    for other in (b, c):
        assert torch.equal(a.flat, other.flat)
        for k in ('ability_mu', 'ability_logvar', 'ability'):
            assert torch.equal(getattr(a, k), getattr(other, k)), k


# ---- agreement with the dense engine ----
def test_agrees_with_the_dense_engine_on_codes_and_fp32_rows():
    P, I, A = 2500, 200, 4
    g = torch.Generator().manual_seed(71)
    mask = torch.rand(P, I, generator=g) < 0.3
    resp = torch.where(mask, (torch.rand(P, I, generator=g) < 0.5).float(), torch.tensor(0.0))
    spec = ops.ElboSpec(irt_model=2, ability_dim=A)
    table, item, eps = S.problem(2, A, I, P, seed=72)
    raw = launch(spec, SparseRows.from_dense(resp.to(dev()), mask.to(dev())), table, item, eps)
    for codes in (True, False):
        dense = launch_elbo(spec, resp, mask, table, item, eps, codes=codes)
        sc = dense.scalars.cpu().double()
        ref = {'ll': sc[_lib.S_LL], 'reg': sc[_lib.S_REG], 'kl_ability': sc[_lib.S_KL], 'logq0': sc[_lib.S_LOGQ0], 'logp': sc[_lib.S_LOGP],
               'ability_mu': dense.ability_mu.cpu().double(), 'ability_logvar': dense.ability_logvar.cpu().double(),
               'ability': dense.ability.cpu().double(), 'g_table': [dense.grad_table(s).cpu().double() for s in range(2)],
               'g_item': dense.grad_item((I, spec.item_dim)).cpu().double()}
        compare_raw(raw, ref, (I, spec.item_dim))
        assert float(raw.scalars[_lib.S_NOBS]) == float(dense.scalars[_lib.S_NOBS])


# ---- index safety, without risk ----
def test_planted_out_of_range_items_are_skipped_and_counted(row_image):
    resp, mask, rows = row_image
    I, extra, P = ROW_I, 16, len(ROW_LENGTHS)
    spec = ops.ElboSpec(irt_model=2, ability_dim=3)
    table, item, eps = S.problem(2, 3, I + extra, P, seed=81)          # `item` has I + 16 rows: a planted index stays inside it
    # plant cells with items in [I, I + 16) at the END of rows 2, 5 and 9 (the row side stays sorted; the column side is as it was)
    plant = {2: [I, I + 3], 5: [I + 15], 9: [I + 1, I + 2, I + 7]}
    row_ptr, row_cell = rows.row_ptr.cpu().tolist(), rows.row_cell.cpu().tolist()
    new_ptr, new_cell = [0], []
    for p in range(P):
        new_cell += row_cell[row_ptr[p]:row_ptr[p + 1]] + [(i << 1) | 1 for i in plant.get(p, [])]
        new_ptr.append(len(new_cell))
    n_planted = sum(len(v) for v in plant.values())
    assert all(I <= i < I + extra for v in plant.values() for i in v) and len(new_cell) == rows.nnz + n_planted
    d = dev()
    planted = SparseRows(torch.tensor(new_ptr, device=d), torch.tensor(new_cell, dtype=torch.int32, device=d), rows.col_ptr,
                         torch.cat([rows.col_cell, rows.col_cell.new_zeros(n_planted)]), P, I)      # (col_ptr ends at the true cells)
    clean = launch(spec, rows, table, item, eps)
    dirty = launch(spec, planted, table, item, eps)
    assert torch.equal(clean.flat, dirty.flat)
    for k in ('ability_mu', 'ability_logvar', 'ability'):
        assert torch.equal(getattr(clean, k), getattr(dirty, k)), k
    assert planted.bad_index_count == n_planted and rows.bad_index_count == 0


# ---- check() ----
def test_check_counts_the_damage_of_a_hand_damaged_copy(row_image):
    _, _, rows = row_image
    assert rows.violations() == 0
    P = len(ROW_LENGTHS)

    def copy_with(**change):
        t = {k: getattr(rows, k).clone() for k in ('row_ptr', 'row_cell', 'col_ptr', 'col_cell')}
        for k, f in change.items():
            f(t[k])
        return SparseRows(t['row_ptr'], t['row_cell'], t['col_ptr'], t['col_cell'], P, ROW_I)

    def unsorted(cells):            # row 4 (65 cells): its first two cells swapped
        k = int(rows.row_ptr[4])
        cells[k], cells[k + 1] = cells[k + 1].clone(), cells[k].clone()

    def missing(cells):             # a column-side cell whose answer the row side does not list
        cells[10] ^= 1

    for change, exact in ((dict(row_cell=unsorted), None), (dict(col_cell=missing), 1), (dict(row_cell=unsorted, col_cell=missing), None)):
        bad = copy_with(**change)
        n = bad.violations()                                   # (a number read back; no ELBO launch on a damaged image)
        host = sparse.check_host(bad.to('cpu'))
        assert n == host and n >= 1 and (exact is None or n == exact), (n, host)
        with pytest.raises(ValueError, match='sparse rows'):
            bad.check()


# ---- autograd end to end ----
def test_model_and_three_adam_steps_follow_the_dense_rows():
    P, I, A, bs = 600, 120, 2, 200
    g = torch.Generator().manual_seed(91)
    mask = torch.rand(P, I, generator=g) < 0.25
    resp = torch.where(mask, (torch.rand(P, I, generator=g) < 0.5).float(), torch.tensor(-1.0))
    d = dev()
    rows = SparseRows.from_dense(resp.to(d), mask.to(d))
    r_d, m_d = ops.pad_rows(resp.to(d), mask.to(d))
    torch.manual_seed(3)
    dense_model = VIBO_2PL(A, I, ability_merge='product').to(d)
    sparse_model = copy.deepcopy(dense_model)

    def step(model, response, m, ri):
        model.zero_grad(set_to_none=True)
        loss = model.elbo_step(response, m, annealing_factor=0.8, row_index=ri)
        loss.backward()
        return loss

    torch.manual_seed(4)
    la = step(dense_model, r_d, m_d, None)
    torch.manual_seed(4)
    lb = step(sparse_model, rows, None, None)
    check('sparse elbo_step loss', abs(float(la.detach()) - float(lb.detach())) / abs(float(la.detach())), TOL_ELBO)
    for (k, pa), (_, pb) in zip(dense_model.named_parameters(), sparse_model.named_parameters()):
        check(f'sparse elbo_step grad {k}', rel_err(pb.grad.cpu(), pa.grad.cpu()), TOL_GRAD)

    # three Adam steps of the CLI's module path: consecutive blocks of persons
    opt_a = torch.optim.Adam(dense_model.parameters(), lr=5e-3)
    opt_b = torch.optim.Adam(sparse_model.parameters(), lr=5e-3)
    for k in range(3):
        torch.manual_seed(10 + k)
        step(dense_model, r_d, m_d, torch.arange(k * bs, (k + 1) * bs, device=d))
        opt_a.step()
        torch.manual_seed(10 + k)
        step(sparse_model, rows, None, RowBlock(k * bs, (k + 1) * bs))
        opt_b.step()
    for (k, pa), (_, pb) in zip(dense_model.named_parameters(), sparse_model.named_parameters()):
        check(f'sparse adam x3 {k}', rel_err(pb.detach().cpu(), pa.detach().cpu()), TOL_GRAD)
