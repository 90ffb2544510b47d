"""Sparse response rows: a matrix held as its observed cells only (include/vibo_hip_sparse_rows.h states the image; this module
builds it with torch ops on the data's device and calls the exports that read it: the range calls of that header, the gathered
calls of include/vibo_hip_sparse_gather.h and the gathered call with a row-driven item pass of include/vibo_hip_sparse_row_driven.h).

    rows = SparseRows.from_dense(response, mask)          # or from_cell_codes / from_coo / from_arrays
    ops.fused_elbo(spec, table, item, None, rows, None, eps, row_index=range(a, b))
    model.elbo_step(rows.rows(range(a, b)), None)         # a range view goes wherever a `response` goes, with mask=None
    model.elbo_step(rows, None, row_index=RowGather(idx)) # a gathered minibatch: idx int64 [B] on the image's device
    model.encode(rows.take(idx), None)                    # the same as a view
    model.elbo_step(rows, None, row_index=RowGather(idx, item_pass='rows'))      # ... with the row-driven item pass (opt-in)

Covered: the plain model (unconditional product-of-experts posterior, IRT decoder, no flows, ability_dim 1..8) on contiguous person
ranges and on index vectors of persons.  A range call costs its persons' cells.  A gathered call's person pass costs the batch's
cells, but its item pass streams the image's whole column side whatever the batch size (the header says why): small batches of a
large image pay for it.  item_pass='rows' (RowGather, take) selects the row-driven item pass instead: the batch's own cells, ordered
by item once per call; its cost follows B x the image's longest row, and it never reads the column side.  The default stays
'columns'; which one wins where is measured, not guessed (profiles/sparse_row_driven_record.txt).  With gradients a person named twice in one index vector is owned by its first row; the later rows come
back as zeros and are counted in bad_index_count, as is an index outside the image.
Everything else raises NotImplementedError naming the format: a bare tensor row_index (wrap it in RowGather), person sharding
(a reducer), the conditional and caller-supplied posteriors, flows, ability_dim 9..16.
"""
import ctypes
import math

import torch

from . import _lib

FORMAT = 'sparse rows'
CHUNK = _lib.SPARSE_CHUNK
ITEM_PASSES = ('columns', 'rows')      # a gathered call's item pass: vibo_hip_sparse_gather.h | vibo_hip_sparse_row_driven.h


def _check_item_pass(item_pass):
    if item_pass not in ITEM_PASSES:
        raise ValueError(f"{FORMAT}: item_pass must be 'columns' or 'rows', not {item_pass!r}")
    return item_pass


def key_layout(num_person, num_item):
    """THE KEY of include/vibo_hip_sparse_row_driven.h for an image of P persons x I items -> (bP, end_bit, pad_key): a cell's key is
    item << (bP + 1) | person << 1 | right, sorted over the bits [0, end_bit); the pad key is above every real key."""
    bp = max(1, (int(num_person) - 1).bit_length())
    return bp, bp + 1 + int(num_item).bit_length(), int(num_item) << (bp + 1)


class RowBlock:
    """A block of consecutive persons, range(start, stop): what a resident split on sparse rows yields as a minibatch's `row_index`.
    It answers numel() like the index tensors of the other formats, so the loops that weight a loss by the batch size need no change."""
    __slots__ = ('start', 'stop')

    def __init__(self, start, stop):
        self.start, self.stop = int(start), int(stop)

    def numel(self):
        return self.stop - self.start

    __len__ = numel

    def as_range(self):
        return range(self.start, self.stop)

    def __repr__(self):
        return f'RowBlock({self.start}, {self.stop})'


class RowGather:
    """An index vector of persons (int64 [B], on the image's device, relative to the view it is applied to): what a resident split on
    sparse rows yields as a person-shuffled minibatch's `row_index`, beside RowBlock.  item_pass: the item pass of the calls with
    gradients on these persons, 'columns' (the image's column side) or 'rows' (the batch's own cells, ordered per call)."""
    __slots__ = ('index', 'item_pass')

    def __init__(self, index, item_pass='columns'):
        if not isinstance(index, torch.Tensor) or index.dtype != torch.int64 or index.dim() != 1 or index.numel() < 1:
            raise ValueError(f'{FORMAT}: RowGather takes a non-empty 1-d int64 tensor of persons')
        self.index, self.item_pass = index, _check_item_pass(item_pass)

    def numel(self):
        return int(self.index.numel())

    __len__ = numel

    def __repr__(self):
        return f'RowGather({self.numel()} persons)'


def _as_range(rows, num_person):
    """None / range (step 1) / RowBlock -> range inside [0, num_person); anything else is refused by name."""
    if rows is None:
        return range(0, num_person)
    if isinstance(rows, RowBlock):
        rows = rows.as_range()
    if isinstance(rows, torch.Tensor):
        raise NotImplementedError(f'{FORMAT}: a bare tensor row_index is not taken -- wrap it, row_index=sparse.RowGather(index), or pass '
                                  f'the view rows.take(index) (a gathered call has its own cost and its own rule for repeats)')
    if not isinstance(rows, range) or rows.step != 1:
        raise NotImplementedError(f'{FORMAT}: row_index must be None or a range with step 1, not {rows!r}')
    if len(rows) < 1 or rows.start < 0 or rows.stop > num_person:
        raise ValueError(f'{FORMAT}: persons {rows!r} are not a non-empty range inside [0, {num_person})')
    return rows


def check_spec(spec):
    """The ElboSpecs the format does not cover raise here, by name, instead of surfacing as the library's -8."""
    if spec.conditional:
        raise NotImplementedError(f'{FORMAT}: the conditional posterior is not covered (unconditional product of experts only)')
    if spec.given:
        raise NotImplementedError(f'{FORMAT}: a caller-supplied posterior (--ability-merge mean, VI) is not covered')
    if spec.n_flows > 0:
        raise NotImplementedError(f'{FORMAT}: planar flows are not covered (n_flows must be 0)')
    if not (1 <= spec.ability_dim <= _lib.MAX_ABILITY_DIM_FAST):
        raise NotImplementedError(f'{FORMAT}: ability_dim={spec.ability_dim} is not covered (1..{_lib.MAX_ABILITY_DIM_FAST})')


def _cells(index, right):
    """index << 1 | right as the image stores it: the uint32's bits in an int32 tensor."""
    return ((index.to(torch.int64) << 1) | right.to(torch.int64)).to(torch.int32)


def _index_of(cells):
    return (cells.to(torch.int64) & 0xffffffff) >> 1


def _ptr_from_counts(index, n):
    counts = torch.bincount(index, minlength=n)
    return torch.cat([counts.new_zeros(1), torch.cumsum(counts, 0)])


def chunk_list(col_ptr, chunk=CHUNK):
    """(col_chunk int64 [I + 1], chunk_item int32 [n], chunk_first int64 [n]) of a column pointer array: every column's list cut into
    pieces of at most `chunk` entries, columns in order, pieces in order."""
    lens = col_ptr[1:] - col_ptr[:-1]
    n = (lens + (chunk - 1)) // chunk
    col_chunk = torch.cat([n.new_zeros(1), torch.cumsum(n, 0)])
    items = torch.repeat_interleave(torch.arange(lens.numel(), device=col_ptr.device), n)
    piece = torch.arange(items.numel(), device=col_ptr.device) - col_chunk[items]
    return col_chunk, items.to(torch.int32), col_ptr[items] + chunk * piece


class SparseRows:
    """The device arrays of an image of P persons x I items, or a view of its persons: a range (rows()) or an index vector (take(),
    with an `index` attribute; None on every other object).  Passed wherever a `response` goes, with mask=None."""

    def __init__(self, row_ptr, row_cell, col_ptr, col_cell, num_person, num_item, *, _view=None):
        self.row_ptr, self.row_cell, self.col_ptr, self.col_cell = row_ptr, row_cell, col_ptr, col_cell
        self.image_persons, self.num_item = int(num_person), int(num_item)
        if not (1 <= self.image_persons < 2 ** 31 and 1 <= self.num_item < 2 ** 31):
            raise ValueError(f'{FORMAT}: 1 <= P, I < 2^31')
        for name, t, dt in (('row_ptr', row_ptr, torch.int64), ('row_cell', row_cell, torch.int32), ('col_ptr', col_ptr, torch.int64),
                            ('col_cell', col_cell, torch.int32)):
            if t.dtype != dt or t.dim() != 1 or not t.is_contiguous():
                raise ValueError(f'{FORMAT}: {name} must be a contiguous 1-d {dt} tensor (cells: the uint32 bits)')
        if row_ptr.numel() != self.image_persons + 1 or col_ptr.numel() != self.num_item + 1 or row_cell.numel() != col_cell.numel():
            raise ValueError(f'{FORMAT}: row_ptr [P + 1], col_ptr [I + 1], row_cell and col_cell [nnz]')
        self.nnz = int(row_cell.numel())
        if _view is None:
            self.col_chunk, self.chunk_item, self.chunk_first = chunk_list(col_ptr)
            self.bad_cells = torch.zeros(1, dtype=torch.int64, device=row_ptr.device)      # the library's sticky counter
            self._slot = [None]          # the gathered calls' person_slot map, made on first use; views share the holder
            self._max_row = [None]       # the longest row's cells, read back on first use; views share the holder
            self.row0, self.num_person, self.index, self.image_index = 0, self.image_persons, None, None
            self.item_pass = 'columns'
        else:
            base, rng, index, self.item_pass = _view
            self.col_chunk, self.chunk_item, self.chunk_first, self.bad_cells = base.col_chunk, base.chunk_item, base.chunk_first, base.bad_cells
            self._slot, self._max_row = base._slot, base._max_row
            if index is None:
                self.row0, self.num_person, self.index, self.image_index = base.row0 + rng.start, len(rng), None, None
            else:
                # image_index: the same persons counted from the image's first.  Of the whole image: the index as it is (the launches
                # check it); of a range view: an entry outside the view becomes -1, which no launch follows
                self.row0, self.num_person, self.index = base.row0, int(index.numel()), index
                if base.row0 == 0 and base.num_person == base.image_persons:
                    self.image_index = index
                else:
                    inside = (index >= 0) & (index < base.num_person)
                    self.image_index = torch.where(inside, index + base.row0, torch.full_like(index, -1)).contiguous()
        self.num_chunk = int(self.chunk_item.numel())

    # ---- builders ----
    @classmethod
    def from_coo(cls, person, item, right, num_person, num_item, check=True):
        """From the observed cells as three equally long vectors (any order; a cell listed twice fails check())."""
        person, item = person.to(torch.int64).reshape(-1), item.to(torch.int64).reshape(-1)
        right = (right.reshape(-1) != 0)
        if person.numel() and (int(person.min()) < 0 or int(person.max()) >= num_person or int(item.min()) < 0 or int(item.max()) >= num_item):
            raise ValueError(f'{FORMAT}: a cell outside {num_person} persons x {num_item} items')
        by_row = torch.argsort(person * num_item + item)
        by_col = torch.argsort(item * num_person + person)
        self = cls(_ptr_from_counts(person, num_person), _cells(item[by_row], right[by_row]),
                   _ptr_from_counts(item, num_item), _cells(person[by_col], right[by_col]), num_person, num_item)
        if check:
            self.check()
        return self

    @classmethod
    def from_arrays(cls, row_ptr, row_cell, col_ptr, col_cell, num_person, num_item):
        """From a caller's CSR + CSC arrays as the header lays them out (the chunk list is built here); runs check() once."""
        self = cls(row_ptr, row_cell, col_ptr, col_cell, num_person, num_item)
        self.check()
        return self

    @classmethod
    def _from_observed(cls, observed, right):
        """observed, right: bool [P, I].  Both sides come out of nonzero() in their order: valid by construction, no check()."""
        P, I = observed.shape
        rc = observed.nonzero()
        row_ptr = _ptr_from_counts(rc[:, 0], P)
        row_cell = _cells(rc[:, 1], right[rc[:, 0], rc[:, 1]])
        del rc
        cr = observed.t().nonzero()
        col_ptr = _ptr_from_counts(cr[:, 0], I)
        col_cell = _cells(cr[:, 1], right[cr[:, 1], cr[:, 0]])
        return cls(row_ptr, row_cell, col_ptr, col_cell, P, I)

    @classmethod
    def from_dense(cls, response, mask):
        """From [P, I(, 1)] responses (1.0 = right) and a mask (nonzero = observed; None: every cell)."""
        response = response.reshape(response.shape[0], response.shape[1])
        observed = torch.ones_like(response, dtype=torch.bool) if mask is None else (mask.reshape(response.shape) != 0)
        return cls._from_observed(observed, response == 1)

    @classmethod
    def from_cell_codes(cls, codes):
        """From 1-byte cell codes (ops.CellCodes, or its [P, I] uint8 tensor): 0 wrong, 1 right, 2 missing."""
        c = codes.codes if hasattr(codes, 'codes') else codes
        return cls._from_observed(c != 2, c == 1)

    # ---- the image ----
    shape = property(lambda self: (self.num_person, self.num_item))
    device = property(lambda self: self.row_ptr.device)
    density = property(lambda self: self.nnz / (self.image_persons * self.num_item))

    def dim(self):
        return 2

    def __len__(self):
        return self.num_person

    def _no_gathered(self, what):
        if self.index is not None:
            raise NotImplementedError(f'{FORMAT}: {what} of a gathered view is not covered -- index the vector instead: take(index[...]) '
                                      f'of the view it was taken from')

    def rows(self, rng):
        """The persons `rng` (a range with step 1, or a RowBlock) of this image as a view: the same arrays, another range."""
        self._no_gathered('rows()')
        return SparseRows(self.row_ptr, self.row_cell, self.col_ptr, self.col_cell, self.image_persons, self.num_item,
                          _view=(self, _as_range(rng, self.num_person), None, 'columns'))

    def take(self, index, item_pass=None):
        """The persons index[0..B) of this image or range view (int64 [B] on its device, or a RowGather; persons relative to this view)
        as a view of B rows: row r is person index[r].  Nothing is copied and nothing is read back: an entry outside the view is left
        to the launches, which skip it, return zeros for its row and count it (bad_index_count).  item_pass ('columns' | 'rows';
        default: a RowGather's own, else 'columns') is carried by the view as its `item_pass` attribute."""
        self._no_gathered('take()')
        if isinstance(index, RowGather):
            index, item_pass = index.index, index.item_pass if item_pass is None else item_pass
        item_pass = _check_item_pass('columns' if item_pass is None else item_pass)
        if not isinstance(index, torch.Tensor) or index.dtype != torch.int64 or index.dim() != 1 or index.numel() < 1:
            raise ValueError(f'{FORMAT}: take() needs a non-empty 1-d int64 tensor of persons')
        if index.device != self.device:
            raise ValueError(f'{FORMAT}: the index is on {index.device}, the image on {self.device}')
        return SparseRows(self.row_ptr, self.row_cell, self.col_ptr, self.col_cell, self.image_persons, self.num_item,
                          _view=(self, None, index.contiguous(), item_pass))

    def slot_map(self):
        """The gathered calls' person_slot map of this image (int32 [P], all NO_SLOT between calls), made on first use."""
        if self._slot[0] is None:
            self._slot[0] = torch.full((self.image_persons,), _lib.SPARSE_NO_SLOT, dtype=torch.int32, device=self.device)
        return self._slot[0]

    @property
    def max_row_cells(self):
        """The cells of the image's longest row (at least 1), computed from row_ptr on first use (one read-back) and shared by the views:
        what the row-driven item pass sizes its key buffers by."""
        if self._max_row[0] is None:
            self._max_row[0] = max(1, int((self.row_ptr[1:] - self.row_ptr[:-1]).max()))
        return self._max_row[0]

    def to(self, device):
        if self.index is not None or self.row0 != 0 or self.num_person != self.image_persons:
            raise ValueError(f'{FORMAT}: move the whole image, not a view')
        return SparseRows(self.row_ptr.to(device), self.row_cell.to(device), self.col_ptr.to(device), self.col_cell.to(device),
                          self.image_persons, self.num_item)

    def image(self, columns=True):
        """struct vibo_sparse_image of the arrays (device pointers); columns=False: the row side alone."""
        im = _lib.ViboSparseImage()
        im.num_person, im.num_item, im.nnz = self.image_persons, self.num_item, self.nnz
        im.row_ptr, im.row_cell = self.row_ptr.data_ptr(), self.row_cell.data_ptr()
        if columns:
            im.num_chunk = self.num_chunk
            im.col_ptr, im.col_cell, im.col_chunk = self.col_ptr.data_ptr(), self.col_cell.data_ptr(), self.col_chunk.data_ptr()
            im.chunk_item, im.chunk_first = self.chunk_item.data_ptr(), self.chunk_first.data_ptr()
        return im

    def to_dense(self, rng=None):
        """(response fp32 [n, I] with -1 at missing cells, mask bool [n, I]) of the persons `rng` of this view; of a gathered view
        its rows in the index's order (dense[index]; the index must lie inside the view it was taken from)."""
        rng = _as_range(rng, self.num_person)
        if self.index is not None:
            q = self.image_index[rng.start:rng.stop]
            if int(q.min()) < 0 or int(q.max()) >= self.image_persons:
                raise ValueError(f'{FORMAT}: the index names a person outside the view it was taken from')
            first, counts = self.row_ptr[q], self.row_ptr[q + 1] - self.row_ptr[q]
            n = int(q.numel())
            person = torch.repeat_interleave(torch.arange(n, device=self.device), counts)
            within = torch.arange(person.numel(), device=self.device) - (torch.cumsum(counts, 0) - counts)[person]
            cells = self.row_cell[first[person] + within].to(torch.int64) & 0xffffffff
        else:
            a, b = self.row0 + rng.start, self.row0 + rng.stop
            n = b - a
            k0, k1 = int(self.row_ptr[a]), int(self.row_ptr[b])
            counts = self.row_ptr[a + 1:b + 1] - self.row_ptr[a:b]
            person = torch.repeat_interleave(torch.arange(n, device=self.device), counts)
            cells = self.row_cell[k0:k1].to(torch.int64) & 0xffffffff
        response = torch.full((n, self.num_item), -1.0, dtype=torch.float32, device=self.device)
        mask = torch.zeros(n, self.num_item, dtype=torch.bool, device=self.device)
        response[person, cells >> 1] = (cells & 1).float()
        mask[person, cells >> 1] = True
        return response, mask

    @property
    def bad_index_count(self):
        """Cells the launches on this image skipped because their index was out of range (sticky; 0 on a valid image)."""
        return int(self.bad_cells.item())

    def check(self):
        """Run the validation pass (vibo_sparse_rows_check; on host tensors its mirror check_host) and raise with the count."""
        from . import ops
        n = ops._BACKEND['sparse_check'](self)
        if n:
            raise ValueError(f'{FORMAT}: the image fails {n} of its invariants (pointers monotone, indices in range, lists sorted, '
                             f'both sides the same cells, chunk list consistent with col_ptr)')

    def violations(self):
        """The validation pass's count, as a number."""
        from . import ops
        return ops._BACKEND['sparse_check'](self)


def check_host(rows):
    """vibo_sparse_rows_check restated on the host, check by check (csrc/vibo_sparse.hip): the count of failed checks.  Plain Python
    loops: for tests and small images."""
    P, I, nnz = rows.image_persons, rows.num_item, rows.nnz
    row_ptr, col_ptr = rows.row_ptr.cpu().tolist(), rows.col_ptr.cpu().tolist()
    row_cell = (rows.row_cell.cpu().to(torch.int64) & 0xffffffff).tolist()
    col_cell = (rows.col_cell.cpu().to(torch.int64) & 0xffffffff).tolist()
    col_chunk, chunk_item, chunk_first = rows.col_chunk.cpu().tolist(), rows.chunk_item.cpu().tolist(), rows.chunk_first.cpu().tolist()
    num_chunk = len(chunk_item)

    def sane(a, b):
        return 0 <= a <= b <= nnz

    def lower_bound(cell, lo, hi, key):
        while lo < hi:
            mid = lo + ((hi - lo) >> 1)
            if (cell[mid] >> 1) < key:
                lo = mid + 1
            else:
                hi = mid
        return lo

    def side(ptr, cell, n_lists, limit, other=None):
        v = 0
        for q in range(n_lists):
            a, b = ptr[q], ptr[q + 1]
            v += (q == 0 and a != 0) + (q == n_lists - 1 and b != nnz)
            if not sane(a, b):
                v += 1
                continue
            for k in range(a, b):
                idx = cell[k] >> 1
                v += idx >= limit
                v += k > a and (cell[k - 1] >> 1) >= idx
                if other is not None and idx < other[2]:
                    ra, rb = other[0][idx], other[0][idx + 1]
                    found = False
                    if sane(ra, rb):
                        pos = lower_bound(other[1], ra, rb, q)
                        found = pos < rb and other[1][pos] == ((q << 1) | (cell[k] & 1))
                    v += not found
        return v

    v = side(row_ptr, row_cell, P, I) + side(col_ptr, col_cell, I, P, (row_ptr, row_cell, P))
    for i in range(I):
        c0, c1 = col_chunk[i], col_chunk[i + 1]
        v += (i == 0 and c0 != 0) + (i == I - 1 and c1 != num_chunk)
        a, b = col_ptr[i], col_ptr[i + 1]
        if sane(a, b):
            expect = (b - a + CHUNK - 1) // CHUNK
            if c0 < 0 or c1 > num_chunk or c1 - c0 != expect:
                v += 1
            else:
                v += sum(chunk_item[c0 + t] != i or chunk_first[c0 + t] != a + t * CHUNK for t in range(expect))
    return int(v)


# ---- the native calls (ops._BACKEND['sparse_elbo' | 'sparse_encode' | 'sparse_check']) ----
def _desc(spec, B, I, reg_mode, want_grad):
    from . import ops
    return ops._make_desc(spec, B, I, _lib.MASK_NONE, reg_mode, want_grad, 0, 0)      # (mask_dtype and the strides are not read)


def _hip_sparse_check(rows):
    if not rows.row_ptr.is_cuda:
        return check_host(rows)
    from . import ops
    out = torch.zeros(1, dtype=torch.int64, device=rows.device)
    im = rows.image()
    ops._call('vibo_sparse_rows_check', ctypes.byref(im), ops._ptr(out), ops._stream(rows.device))
    return int(out.item())


def _hip_sparse_elbo(spec, rows, table, item, eps, reg_mode, want_grad):
    """vibo_sparse_elbo_fwd_bwd on the view's persons, or on a gathered view's vibo_sparse_elbo_fwd_bwd_gather (item_pass 'columns') or
    vibo_sparse_elbo_fwd_bwd_gather_rows (item_pass 'rows': the column side is not passed), on the current stream -> ops.RawElbo."""
    from . import ops
    ops._require_device(rows.row_ptr, table, item, eps)
    dev = rows.device
    B, I, A, D = rows.num_person, rows.num_item, spec.ability_dim, spec.item_dim
    table_shape = tuple(table.shape)
    n_table, n_item = math.prod(table_shape), I * D
    flat = torch.empty(_lib.NUM_SCALARS + 2 * n_table + n_item, dtype=torch.float32, device=dev)
    post = torch.empty(3, B, A, dtype=torch.float32, device=dev)
    d = _desc(spec, B, I, reg_mode, want_grad)
    by_rows = rows.index is not None and getattr(rows, 'item_pass', 'columns') == 'rows'
    im = rows.image(columns=bool(want_grad) and not by_rows)
    if by_rows:
        max_row = ctypes.c_int64(rows.max_row_cells)
        ws_bytes = _lib.load().vibo_sparse_row_driven_workspace_bytes(ctypes.byref(d), ctypes.c_int64(I), ctypes.c_int64(rows.image_persons), max_row)
        if ws_bytes == 0:
            raise _lib.ViboLibraryError(f'{FORMAT}: the row-driven item pass does not take this call (item_pass=\'rows\' needs '
                                        f'{B} persons x {rows.max_row_cells} cells of the longest row < 2^31 and a supported descriptor): '
                                        f'use item_pass=\'columns\'')
    else:
        ws_bytes = _lib.load().vibo_sparse_workspace_bytes(ctypes.byref(d), ctypes.c_int64(im.num_chunk))
        if ws_bytes == 0:
            _lib.check(-8, 'vibo_sparse_workspace_bytes')
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    vp, fbase = ctypes.c_void_p, flat.data_ptr()
    tail = (ops._ptr(table), ops._ptr(item), ops._ptr(eps), vp(fbase), ops._ptr(post[0]), ops._ptr(post[1]), ops._ptr(post[2]),
            vp(fbase + 4 * _lib.NUM_SCALARS), vp(fbase + 4 * (_lib.NUM_SCALARS + 2 * n_table)), ops._ptr(rows.bad_cells), ops._ptr(ws),
            ctypes.c_size_t(ws_bytes), ops._stream(dev))
    if rows.index is None:
        ops._call('vibo_sparse_elbo_fwd_bwd', ctypes.byref(d), ctypes.byref(im), ctypes.c_int64(rows.row0), *tail)
    else:
        slot = rows.slot_map() if want_grad else None
        try:
            if by_rows:
                ops._call('vibo_sparse_elbo_fwd_bwd_gather_rows', ctypes.byref(d), ctypes.byref(im), ops._ptr(rows.image_index),
                          ops._ptr(slot), max_row, *tail)
            else:
                ops._call('vibo_sparse_elbo_fwd_bwd_gather', ctypes.byref(d), ctypes.byref(im), ops._ptr(rows.image_index),
                          ops._ptr(slot), *tail)
        except BaseException:
            if slot is not None:          # (a call that stopped between the map's build and its clear: the next one needs it empty)
                slot.fill_(_lib.SPARSE_NO_SLOT)
            raise
    return ops.RawElbo(flat=flat, n_table=n_table, n_item=n_item, n_flow=0, table_shape=table_shape, ability_mu=post[0],
                       ability_logvar=post[1], ability=post[2], ability_k=None, ability_ladj=None)


def _hip_sparse_encode(spec, rows, table):
    from . import ops
    ops._require_device(rows.row_ptr, table)
    dev = rows.device
    out = torch.empty(2, rows.num_person, spec.ability_dim, dtype=torch.float32, device=dev)
    d = _desc(spec, rows.num_person, rows.num_item, _lib.REG_KL, False)
    im = rows.image(columns=False)
    tail = (ops._ptr(table), ops._ptr(out[0]), ops._ptr(out[1]), ops._ptr(rows.bad_cells), ops._stream(dev))
    if rows.index is None:
        ops._call('vibo_sparse_encode', ctypes.byref(d), ctypes.byref(im), ctypes.c_int64(rows.row0), *tail)
    else:          # (no map: every row is independent)
        ops._call('vibo_sparse_encode_gather', ctypes.byref(d), ctypes.byref(im), ops._ptr(rows.image_index), *tail)
    return out[0], out[1]


class SparseFusedELBO(torch.autograd.Function):
    """ops.FusedELBO on sparse rows: (table, item) -> the same eight outputs, the same composition g_ll grad[0] + g_reg grad[1]."""

    @staticmethod
    def forward(ctx, table, item, rows, eps, spec, reg_mode):
        from . import ops
        need_grad = any(ctx.needs_input_grad[:2])
        raw = ops._BACKEND['sparse_elbo'](spec, rows, table.detach().contiguous(), item.detach().contiguous(), eps.contiguous(),
                                          reg_mode, need_grad)
        ctx.raw, ctx.item_shape, ctx.need_grad = raw, tuple(item.shape), need_grad
        sc = raw.scalars
        outs = (sc[_lib.S_LL].clone(), sc[_lib.S_REG].clone(), sc.clone(), raw.ability_mu, raw.ability_logvar, raw.ability,
                raw.ability, sc.new_zeros(()))
        ctx.mark_non_differentiable(*outs[2:])
        return outs

    @staticmethod
    def backward(ctx, g_ll, g_reg, *_):
        raw = ctx.raw
        if not ctx.need_grad:
            return (None,) * 6
        g_table = g_ll * raw.grad_table(0) + g_reg * raw.grad_table(1) if ctx.needs_input_grad[0] else None
        g_item = g_ll * raw.grad_item(ctx.item_shape) if ctx.needs_input_grad[1] else None
        return (g_table, g_item) + (None,) * 4


def _view(rows, mask, row_index, reducer=None):
    if mask is not None:
        raise ValueError(f'{FORMAT} carry their own missingness: pass mask=None')
    if reducer is not None:
        raise NotImplementedError(f'{FORMAT}: person sharding (a reducer) is not covered')
    if row_index is None:
        return rows
    return rows.take(row_index) if isinstance(row_index, RowGather) else rows.rows(row_index)


def fused_elbo(spec, table, item, flow, rows, mask, eps, *, reg_mode=_lib.REG_KL, row_index=None, reducer=None):
    """ops.fused_elbo's branch for a SparseRows `response`."""
    check_spec(spec)
    rows = _view(rows, mask, row_index, reducer)
    B, I = rows.shape
    if flow is not None:
        raise NotImplementedError(f'{FORMAT}: planar flows are not covered')
    if tuple(table.shape) != spec.table_shape(I, B):
        raise ValueError(f'table shape {tuple(table.shape)} != {spec.table_shape(I, B)}')
    if tuple(item.shape) != (I, spec.item_dim):
        raise ValueError(f'item shape {tuple(item.shape)} != {(I, spec.item_dim)}')
    if tuple(eps.shape) != (B, spec.ability_dim):
        raise ValueError(f'eps shape {tuple(eps.shape)} != {(B, spec.ability_dim)}')
    return SparseFusedELBO.apply(table, item, rows, eps, spec, reg_mode)


def encode_posterior(spec, table, rows, mask, row_index=None):
    """ops.encode_posterior's branch for a SparseRows `response`."""
    from . import ops
    check_spec(spec)
    return ops._BACKEND['sparse_encode'](spec, _view(rows, mask, row_index), table.detach().contiguous())
