"""Gathered minibatches on sparse response rows, on the GPU: vibo_sparse_elbo_fwd_bwd_gather and vibo_sparse_encode_gather of
include/vibo_hip_sparse_gather.h against the fp64 oracle on resp[idx], mask[idx] (gpu_common.compare_raw's bounds: 2e-5 on heads and
per-person outputs, TOL_GRAD on gradients), the header's three bit-level statements against the range call, an index vector that
cannot be trusted, and three Adam steps through the module path against the dense engine's row_index steps.

The image: P = 1 100 persons x I = 40 items.  Item 0 is answered by every person who answers anything (1 095 entries: three chunks),
item 1 by one person, item 2 by nobody; five rows are empty, some hold one cell.  Rows of 63, 64, 65 and 130 cells do not fit 40
items: they have an image of their own at I = 140.  Every test leaves the image's map all NO_SLOT (the autouse fixture below)."""
import copy

import pytest
import torch

import sparse_rows_common as S
from gpu_common import TOL_GRAD, check, compare_raw, dev
from conftest import rel_err
from vibo_amd import _lib, ops, sparse
from vibo_amd.sparse import RowGather, SparseRows
from vibo_amd.torch_core.models import VIBO_2PL

pytestmark = pytest.mark.gpu
CHUNK = S.CHUNK
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
    assert (rows.col_chunk[1:4] - rows.col_chunk[0:3]).tolist() == [3, 1, 0]
    return resp, mask, rows


@pytest.fixture(autouse=True)
def map_is_clear_after_every_call(image):
    yield
    torch.cuda.synchronize()
    slot = image[2]._slot[0]
    assert slot is None or bool((slot == NO_SLOT).all()), 'a gathered call left entries in the map'


def launch(spec, view, table, item, eps, reg_mode=KL, want_grad=True):
    d = dev()
    raw = sparse._hip_sparse_elbo(spec, view, table.to(d).contiguous(), item.to(d).contiguous(), eps.to(d).contiguous(), reg_mode, want_grad)
    torch.cuda.synchronize()
    slot = view._slot[0]
    assert slot is None or bool((slot == NO_SLOT).all())
    return raw


def against_oracle(spec, rows, resp, mask, idx, table, item, eps, reg_mode=KL, want_grad=True):
    """One gathered launch on rows.take(idx) compared with the oracle on the dense rows resp[idx], mask[idx]."""
    before = rows.bad_index_count
    ref = S.oracle(spec, table, item, resp[idx], mask[idx], eps, reg_mode, want_grad)
    raw = launch(spec, rows.take(idx.to(dev())), table, item, eps, reg_mode, want_grad)
    sc = raw.scalars.cpu().double()
    print('heads B=%d' % idx.numel(), ' '.join(f'{k} {float(sc[j]):.6f} ref {float(ref[k]):.6f}' for k, j in (
        ('ll', _lib.S_LL), ('reg', _lib.S_REG), ('kl_ability', _lib.S_KL), ('logq0', _lib.S_LOGQ0), ('logp', _lib.S_LOGP))))
    compare_raw(raw, ref, (rows.num_item, spec.item_dim), want_grad=want_grad)
    assert float(raw.scalars[_lib.S_NOBS]) == float(mask[idx].sum()) and float(raw.scalars[_lib.S_LADJ]) == 0.0
    if want_grad:
        empty = mask[idx].sum(0) == 0
        assert bool(empty.any())
        assert bool((raw.grad_item((rows.num_item, spec.item_dim))[empty.to(dev())] == 0).all()), 'an item with no cell in the batch: exact zeros'
    assert rows.bad_index_count == before
    return raw


def index_cases(drop, seed):
    """The issue's four index vectors: 70 persons of a permutation (12 waves, 5 or 6 rows each), one person, every person permuted,
    and one that holds persons 0 and P - 1.  Under VIBO_MISSING_DROP a row without a cell has no posterior: the empty rows stay out."""
    g = torch.Generator().manual_seed(seed)
    perm = torch.randperm(P, generator=g)
    if drop:
        perm = perm[~torch.isin(perm, torch.tensor(EMPTY))]
    ends = torch.tensor([P - 1, 17, 0, LONE, 250])
    return {'70 of a permutation': perm[:70], 'one person': perm[70:71], 'every person': perm, 'the ends': ends}


def test_seventy_rows_are_twelve_waves_of_uneven_length():
    assert S.person_waves(70) == 12 and sorted({S.rows_of_wave(70, w) for w in range(12)}) == [5, 6]


# ---- the oracle ----
@pytest.mark.parametrize('reg', [KL, SAMPLED], ids=['kl', 'sampled'])
@pytest.mark.parametrize('drop', [False, True], ids=['prior', 'drop'])
@pytest.mark.parametrize('A', [1, 3, 8])
@pytest.mark.parametrize('irt', [1, 2, 3])
def test_against_the_oracle(image, irt, A, drop, reg):
    resp, mask, rows = image
    spec = ops.ElboSpec(irt_model=irt, ability_dim=A, drop_missing=drop)
    for n, (name, idx) in enumerate(index_cases(drop, seed=1000 * irt + 10 * A + drop).items()):
        table, item, eps = S.problem(irt, A, I, idx.numel(), seed=100 * irt + A + n)
        # compare_raw bounds a head by 2e-5 of the head itself, so a head must not be a sum that cancels.  With S.problem's experts
        # (log-variance about 0) and this image's rows (about 19 cells) a person's logq0 term, -0.5 log 2 pi - 0.5 logvar - 0.5 eps^2
        # with logvar = -log(sum of the cells' precisions), has mean -0.92 + 1.47 - 0.5 = 0.05 under VIBO_MISSING_DROP: over 1 095
        # persons x A dims a random walk about zero, a few units, against an fp32 rounding of 1e-4 .. 4e-4 that every head of that
        # size of sum carries.  Experts sharper by e^2 move the term's mean to about 1 and the head to its terms' scale.
        table[:, A:] -= 2.0
        against_oracle(spec, rows, resp, mask, idx, table, item, eps, reg)
        amu, alv = sparse._hip_sparse_encode(spec, rows.take(idx.to(dev())), table.to(dev()))
        ref = S.oracle(spec, table, item, resp[idx], mask[idx], eps, reg, want_grad=False)
        for got, want in ((amu, ref['ability_mu']), (alv, ref['ability_logvar'])):
            assert (got.cpu() - want.float()).abs().max() < 2e-5 * max(1.0, float(want.abs().max())), name


@pytest.mark.parametrize('irt,A,reg', [(2, 3, KL), (3, 8, SAMPLED), (1, 1, KL)])
def test_forward_only_without_a_column_side_and_with_repeats(image, irt, A, reg):
    """d->want_grad == 0: the image goes without its column side (SparseRows.image(columns=False)) and there is no map, so a person
    named twice is two ordinary rows."""
    resp, mask, rows = image
    assert rows.image(columns=False).col_ptr is None and rows.image(columns=False).num_chunk == 0
    spec = ops.ElboSpec(irt_model=irt, ability_dim=A)
    idx = torch.cat([index_cases(False, seed=7)['70 of a permutation'], torch.tensor([LONE, 0, LONE, 3])])
    table, item, eps = S.problem(irt, A, I, idx.numel(), seed=17)
    against_oracle(spec, rows, resp, mask, idx, table, item, eps, reg, want_grad=False)


# rows of every length at which the person pass's lane loop takes another number of trips
LONG_LENGTHS = {0: 0, 1: 1, 2: 63, 3: 64, 4: 65, 5: 130, 640: 130, 1099: 65}
LONG_I = 140


@pytest.fixture(scope='module')
def long_image():
    lengths = [LONG_LENGTHS.get(r, (11 * r) % 90 + 1) for r in range(P)]
    resp, mask = S.matrix_with_row_lengths(lengths, LONG_I, seed=131)
    assert mask.sum(1).tolist() == lengths
    return resp, mask, SparseRows.from_dense(resp.to(dev()), mask.to(dev()))


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
    # (every item is answered by someone in this batch or not: the oracle comparison covers both; exact zeros are the main image's test)
    ref = S.oracle(spec, table, item, resp[idx], mask[idx], eps, reg)
    raw = launch(spec, rows.take(idx.to(dev())), table, item, eps, reg)
    compare_raw(raw, ref, (LONG_I, spec.item_dim))
    assert float(raw.scalars[_lib.S_NOBS]) == float(mask[idx].sum()) and rows.bad_index_count == 0


def test_past_the_dense_ceiling():
    Pw, Iw, A = 200, 40_000, 2
    g = torch.Generator().manual_seed(51)
    item_of = torch.stack([torch.randperm(Iw, generator=g)[:30] for _ in range(Pw)])
    person_of = torch.arange(Pw).unsqueeze(1).expand(Pw, 30)
    right = torch.rand(Pw, 30, generator=g) < 0.5
    rows = SparseRows.from_coo(person_of.to(dev()), item_of.to(dev()), right.to(dev()), Pw, Iw)
    idx = torch.randperm(Pw, generator=g)[:64]
    resp, mask = rows.to_dense()
    assert mask[idx.to(dev())].sum(1).tolist() == [30] * 64
    spec = ops.ElboSpec(irt_model=2, ability_dim=A)
    table, item, eps = S.problem(2, A, Iw, 64, seed=52)
    against_oracle(spec, rows, resp.cpu(), mask.cpu(), idx, table, item, eps)
    assert bool((rows.slot_map() == NO_SLOT).all())


# ---- bits ----
def same_bits(a, b, spec, num_item, grad_item=True):
    assert torch.equal(a.scalars, b.scalars)
    for k in ('ability_mu', 'ability_logvar', 'ability'):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    for s in range(2):
        assert torch.equal(a.grad_table(s), b.grad_table(s)), s
    if grad_item:
        assert torch.equal(a.grad_item((num_item, spec.item_dim)), b.grad_item((num_item, spec.item_dim)))


def test_two_launches_agree_bit_for_bit(image):
    _, _, rows = image
    spec = ops.ElboSpec(irt_model=3, ability_dim=8)
    idx = index_cases(False, seed=61)['every person'][:700].to(dev())
    table, item, eps = S.problem(3, 8, I, 700, seed=62)
    a, b = launch(spec, rows.take(idx), table, item, eps), launch(spec, rows.take(idx.clone()), table, item, eps)
    assert torch.equal(a.flat, b.flat)
    same_bits(a, b, spec, I)


@pytest.mark.parametrize('a,b', [(0, P), (37, 37 + 64), (P - 5, P), (500, 501), (0, 600)])
@pytest.mark.parametrize('irt,A,reg', [(2, 3, SAMPLED), (3, 8, KL)])
def test_consecutive_index_against_the_range_call(image, a, b, irt, A, reg):
    _, _, rows = image
    spec = ops.ElboSpec(irt_model=irt, ability_dim=A)
    table, item, eps = S.problem(irt, A, I, b - a, seed=71)
    by_range = launch(spec, rows.rows(range(a, b)), table, item, eps, reg)
    by_index = launch(spec, rows.take(torch.arange(a, b, device=dev())), table, item, eps, reg)
    same_bits(by_index, by_range, spec, I, grad_item=(a, b) == (0, P))          # the whole image: the bisection window is the whole chunk
    shape = (I, spec.item_dim)
    check('gathered grad_item against the range call', rel_err(by_index.grad_item(shape).cpu(), by_range.grad_item(shape).cpu().double()), TOL_GRAD)
    # forward only, and the encode call
    fwd_range = launch(spec, rows.rows(range(a, b)), table, item, eps, reg, want_grad=False)
    fwd_index = launch(spec, rows.take(torch.arange(a, b, device=dev())), table, item, eps, reg, want_grad=False)
    assert torch.equal(fwd_index.scalars, fwd_range.scalars) and torch.equal(fwd_index.ability, fwd_range.ability)
    assert torch.equal(fwd_index.scalars, by_index.scalars)


def test_a_persons_posterior_has_the_same_bits_at_any_position(image):
    _, _, rows = image
    spec = ops.ElboSpec(irt_model=2, ability_dim=8)
    table, item, eps = S.problem(2, 8, I, P, seed=81)
    whole = launch(spec, rows, table, item, eps)
    mu_r, lv_r = sparse._hip_sparse_encode(spec, rows, table.to(dev()))
    assert torch.equal(mu_r, whole.ability_mu) and torch.equal(lv_r, whole.ability_logvar)
    g = torch.Generator().manual_seed(82)
    for n in (P, 70, 1):
        perm = torch.randperm(P, generator=g)[:n].to(dev())
        got = launch(spec, rows.take(perm), table, item, eps[:n])
        mu_g, lv_g = sparse._hip_sparse_encode(spec, rows.take(perm), table.to(dev()))
        for x, want in ((got.ability_mu, whole.ability_mu), (got.ability_logvar, whole.ability_logvar), (mu_g, mu_r), (lv_g, lv_r)):
            assert torch.equal(x, want[perm]), n


def test_a_chunk_with_no_batch_member_contributes_exact_zeros(image):
    """Item 0 has three chunks.  A batch among the persons of its first chunk alone: chunks two and three hold no member, so the
    item finish adds 0 + record + 0 + 0.  The same persons on an image cut off after that first chunk (item 0: one chunk, written by
    its wave directly) hold every column's entries at the same places of their lists, hence on the same lanes: grad_item is the
    same bits exactly if the two empty chunks gave exact zeros."""
    resp, mask, rows = image
    K = int((mask[:, 0].cumsum(0) == CHUNK).nonzero()[0]) + 1          # the first K persons hold item 0's first CHUNK entries
    assert int(mask[:K, 0].sum()) == CHUNK and K < P
    cut = SparseRows.from_dense(resp[:K].to(dev()), mask[:K].to(dev()))
    assert int(cut.col_chunk[1]) == 1
    spec = ops.ElboSpec(irt_model=2, ability_dim=3)
    idx = torch.randperm(K, generator=torch.Generator().manual_seed(91))[:70].to(dev())
    table, item, eps = S.problem(2, 3, I, 70, seed=92)
    full, short = launch(spec, rows.take(idx), table, item, eps), launch(spec, cut.take(idx), table, item, eps)
    same_bits(full, short, spec, I)
    g_item = full.grad_item((I, spec.item_dim))
    assert bool((g_item[0] != 0).any()) and bool((g_item[2] == 0).all())
    assert bool((cut.slot_map() == NO_SLOT).all())


def test_an_item_with_no_cell_in_the_batch_gets_exact_zeros(image):
    resp, mask, rows = image
    spec = ops.ElboSpec(irt_model=3, ability_dim=2)
    idx = torch.tensor([25, 61, 97, 133])                         # short rows, not the one person of item 1; nobody answers item 2
    few = mask[idx].sum(0) == 0
    assert few[1] and few[2] and int(few.sum()) > 2
    table, item, eps = S.problem(3, 2, I, 4, seed=95)
    raw = against_oracle(spec, rows, resp, mask, idx, table, item, eps)
    g_item = raw.grad_item((I, spec.item_dim))
    assert bool((g_item[few.to(dev())] == 0).all()) and bool((g_item[0] != 0).any())
    with_lone = against_oracle(spec, rows, resp, mask, torch.tensor([LONE, 9]), table, item, eps[:2])
    assert bool((with_lone.grad_item((I, spec.item_dim))[1] != 0).any())


# ---- an index that cannot be trusted ----
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
    dirty = launch(spec, rows.take(idx.to(dev())), table, item, eps)
    assert rows.bad_index_count == before + 3
    assert bool((rows.slot_map() == NO_SLOT).all())
    clean = launch(spec, rows.take(good.to(dev())), table, item, eps[keep])
    assert rows.bad_index_count == before + 3
    for k in ('ability_mu', 'ability_logvar', 'ability'):
        got = getattr(dirty, k)
        assert bool((got[bad_rows] == 0).all()), k
        assert torch.equal(got[keep.to(dev())], getattr(clean, k)), k          # (a live row's outputs do not depend on its position)
    sd, sc = dirty.scalars.cpu().double(), clean.scalars.cpu().double()
    for k in (_lib.S_LL, _lib.S_REG, _lib.S_KL, _lib.S_LOGQ0, _lib.S_LOGP):
        assert abs(float(sd[k]) - float(sc[k])) < 2e-5 * max(1.0, abs(float(sc[k]))), k
    assert float(sd[_lib.S_NOBS]) == float(sc[_lib.S_NOBS]) == float(mask[good].sum())
    shape = (I, spec.item_dim)
    for s in range(2):
        check(f'untrusted index g_table[{s}]', rel_err(dirty.grad_table(s).cpu(), clean.grad_table(s).cpu().double()), TOL_GRAD)
    check('untrusted index g_item', rel_err(dirty.grad_item(shape).cpu(), clean.grad_item(shape).cpu().double()), TOL_GRAD)
    compare_raw(clean, S.oracle(spec, table, item, resp[good], mask[good], eps[keep]), shape)

    # encode has no map: a repeat is an ordinary row, an entry outside the image zeros and one more in the count
    mu, lv = sparse._hip_sparse_encode(spec, rows.take(idx.to(dev())), table.to(dev()))
    torch.cuda.synchronize()
    assert rows.bad_index_count == before + 5
    assert torch.equal(mu[55], mu[4]) and torch.equal(lv[55], lv[4]) and bool((mu[4] != 0).any())
    assert bool((mu[[10, 30]] == 0).all()) and bool((lv[[10, 30]] == 0).all())
    assert torch.equal(mu[keep.to(dev())], clean.ability_mu) and torch.equal(lv[keep.to(dev())], clean.ability_logvar)


# ---- autograd end to end ----
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
        step(sparse_model, rows, None, RowGather(idx))
        opt_b.step()
    for (k, pa), (_, pb) in zip(dense_model.named_parameters(), sparse_model.named_parameters()):
        check(f'gathered adam x3 {k}', rel_err(pb.detach().cpu(), pa.detach().cpu()), TOL_GRAD)
    assert rows.bad_index_count == 0 and bool((rows.slot_map() == NO_SLOT).all())
