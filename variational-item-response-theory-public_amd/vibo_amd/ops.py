"""Host side of the fused ELBO op: launches libvibo_hip.so through the C ABI and
wires its outputs into torch.autograd.

Reference seam: VIBO_*PL.forward/encode/decode/elbo of
src/torch_core/models.py:337-443 as called from src/torch_core/vibo.py:237-268.

What stays in PyTorch (tiny, O(I) work): the 2-row (or 2xI-row) encoder MLP that
produces the expert table, the item-side reparameterisation / flows / KL, the
optimizer.  Everything O(B x I) is inside the HIP kernel.
"""
import contextlib
import ctypes
import math
import weakref
from collections import namedtuple
from dataclasses import dataclass, field, replace
from typing import Callable, NamedTuple, Optional

import torch

from . import _lib
from . import sparse as _sparse
from .sparse import SparseRows


def item_feat_dim(irt_model, ability_dim):
    """models.py:331-332, 523-524, 538-539."""
    return {1: 1, 2: ability_dim + 1, 3: ability_dim + 2}[int(irt_model)]


@dataclass(frozen=True)
class ElboSpec:
    """Static configuration of one fused-ELBO problem family."""
    irt_model: int
    ability_dim: int
    conditional: bool = False
    drop_missing: bool = False       # --drop-missing (vibo.py:52,217)
    n_flows: int = 0
    given: bool = False              # the caller supplies q(theta_p) per person (--ability-merge mean): VIBO_POSTERIOR_GIVEN

    @property
    def item_dim(self):
        return item_feat_dim(self.irt_model, self.ability_dim)

    def table_shape(self, num_item, num_person=None):
        A = self.ability_dim
        if self.given:
            return (num_person, 2 * A)
        return (2, num_item, 2 * A) if self.conditional else (2, 2 * A)

    def check_supported(self, num_item):
        if not (1 <= self.ability_dim <= _lib.MAX_ABILITY_DIM):
            raise NotImplementedError(
                f'ability_dim={self.ability_dim}: the HIP kernel supports 1..{_lib.MAX_ABILITY_DIM}')
        if not (0 <= self.n_flows <= _lib.MAX_FLOWS):
            raise NotImplementedError(f'n_norm_flows={self.n_flows}: supported 0..{_lib.MAX_FLOWS}')


@dataclass
class RawElbo:
    """Everything one kernel call produces (device tensors)."""
    flat: torch.Tensor              # [8 scalars | grad_table(2*T) | grad_item(I*D) | grad_flow(2*F)]
    n_table: int
    n_item: int
    n_flow: int
    table_shape: tuple
    ability_mu: Optional[torch.Tensor]      # (None: the folded train step that draws its own noise)
    ability_logvar: Optional[torch.Tensor]
    ability: Optional[torch.Tensor] = field(repr=False, compare=False)      # (a property, below: where the call stored no sample, reading it asks `ability_source`)
    ability_k: Optional[torch.Tensor]
    ability_ladj: Optional[torch.Tensor]
    workspace: Optional[torch.Tensor] = None      # folded train step: the partial records vibo_train_epilogue_fused sums
    # The folded train step that draws its own noise stores no sample (ability None): its trainer hangs the rebuild here, a
    # callable -> [B, A] tensor that raises once the step's table and noise counter are gone (trainer._StepSample)
    ability_source: Optional[Callable[[], torch.Tensor]] = field(default=None, repr=False, compare=False)

    @property
    def scalars(self):
        return self.flat[:_lib.NUM_SCALARS]

    def grad_table(self, s):
        o = _lib.NUM_SCALARS + s * self.n_table
        return self.flat[o:o + self.n_table].view(self.table_shape)

    def grad_item(self, shape):
        o = _lib.NUM_SCALARS + 2 * self.n_table
        return self.flat[o:o + self.n_item].view(shape)

    def grad_flow(self, s):
        o = _lib.NUM_SCALARS + 2 * self.n_table + self.n_item + s * self.n_flow
        return self.flat[o:o + self.n_flow]


def _stored_or_rebuilt_ability(self):
    if self._ability is None and self.ability_source is not None:
        return self.ability_source()
    return self._ability


# (the dataclass field stays, so RawElbo(ability=...) is what it was; the stored tensor lives in `_ability`)
RawElbo.ability = property(_stored_or_rebuilt_ability, lambda self, value: setattr(self, '_ability', value))


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _call(name, *args):
    """One call into the library by its export's name; a non-zero return code raises (_lib.check)."""
    _lib.check(getattr(_lib.load(), name)(*args), name)


def _not_saved(self):
    """__reduce__ of the bookkeeping this module hangs on callers' tensors: torch.save / pickle / deepcopy of the tensor see None."""
    return type(None), ()


class _Seen:
    """A tensor as it was when last looked at: identity (held weakly) and version counter.  THE test of "the same tensor,
    unmodified" in this module: the resident-matrix record and the narrowed masks both go through is_()."""
    __slots__ = ('ref', 'version')
    __reduce__ = _not_saved

    def __init__(self, t):
        self.ref, self.version = weakref.ref(t), t._version

    def is_(self, t):
        return t is not None and self.ref() is t and self.version == t._version


class _Note(tuple):
    __slots__ = ()
    __reduce__ = _not_saved


def _narrowed(mask):
    """The uint8 form of a caller's bool / int64 mask: ONE object while that mask is alive and neither has been edited.  It hangs on
    the mask (`_vibo_u8`) and points back weakly (`_vibo_mask`, see _caller_mask), so it is freed with the mask and never pins it.
    A bool mask's shares its bytes AND its version counter (an edit through either shows in both); an int64 mask's is a copy."""
    kept = getattr(mask, '_vibo_u8', None)
    if kept is None or not (kept[0] is None or (kept[0].is_(mask) and _caller_mask(kept[1]) is mask)):
        if mask.dtype == torch.bool:
            # through detach(): whatever a view keeps of its base (`_base`) is then not the mask itself -- hung on the mask, that
            # would be a cycle only the garbage collector frees, with the mask's GPU memory in it
            m8, kept = mask.detach().view(torch.uint8), None
        else:
            m8, kept = (mask != 0).contiguous().view(torch.uint8), _Seen(mask)
        m8._vibo_mask = _Note((weakref.ref(mask), None if kept is None else _Seen(m8)))
        kept = mask._vibo_u8 = _Note((kept, m8))
    return kept[1]


def _caller_mask(mask):
    """The caller's own tensor behind a mask _narrowed() made -- while that tensor lives and the narrowed copy of an int64 mask has
    not been edited itself --, any other mask as it is."""
    link = getattr(mask, '_vibo_mask', None)
    if link is None or (link[1] is not None and not link[1].is_(mask)):
        return mask
    src = link[0]()
    return mask if src is None else src


def prepare_mask(mask, keep_int64=False):
    """-> (2-D mask tensor the kernel can read, VIBO_MASK_* code).

    bool / uint8 masks (datasets.py:938 yields bool) are read in place, strided rows included.  int64 masks (the
    reference loop converts with `.long()`, vibo.py:240) cost 8 B per cell and are only understood by the fallback
    kernels, so they are narrowed to uint8 once per tensor (_narrowed: a resident mask is converted a single
    time); `keep_int64=True` hands them to the library unchanged (VIBO_MASK_I64)."""
    if mask is None:
        return None, _lib.MASK_NONE
    if mask.dim() == 3:
        mask = mask.squeeze(2)
    if mask.dtype == torch.bool or mask.dtype == torch.uint8:
        # rows may be strided (e.g. padded to 16 bytes, see pad_rows); only the cells must be unit-stride
        if mask.stride(-1) != 1:
            mask = mask.contiguous()
        return (mask if mask.dtype == torch.uint8 else _narrowed(mask)), _lib.MASK_U8
    if mask.dtype == torch.int64 and keep_int64:
        return mask.contiguous(), _lib.MASK_I64
    if mask.dtype == torch.int64:
        return _narrowed(mask), _lib.MASK_U8
    return (mask != 0).contiguous().view(torch.uint8), _lib.MASK_U8


class CellCodes:
    """"Format P" rows: one byte per cell holding the whole cell (0 = answered wrong, 1 = answered right, 2 = missing;
    VIBO_MASK_CODES of include/vibo_hip.h) instead of an fp32 response plus a mask byte -- 1 B instead of 5 B of HBM
    per cell.  `codes` is a [P, I] uint8 view of rows whose stride is a multiple of 4 cells (pack_cell_codes pads to whole 16-
    or 64-byte pieces, which the matrix-pipe passes of the conditional posterior read fastest).  Passed wherever a `response`
    tensor goes (with mask=None): model.forward / elbo_step / encode / log_marginal, FusedTrainer.step, fused_elbo."""
    __slots__ = ('codes',)

    def __init__(self, codes):
        if codes.dtype != torch.uint8 or codes.dim() != 2 or codes.stride(1) != 1 or codes.stride(0) % 4 != 0:
            raise ValueError('CellCodes: [P, I] uint8 rows with a stride that is a multiple of 4 (see pack_cell_codes)')
        self.codes = codes

    shape = property(lambda self: self.codes.shape)
    device = property(lambda self: self.codes.device)

    def dim(self):
        return 2

    def __len__(self):
        return self.codes.shape[0]

    def rows(self, index):
        """CellCodes of the persons `index` (a copy, rows still padded to a multiple of 4 cells)."""
        c = self.codes
        stride = c.stride(0)
        padded = c.as_strided((c.shape[0], stride), (stride, 1)) if c.shape[1] != stride else c
        return CellCodes(padded[index][:, :c.shape[1]])

    def unpack(self):
        """-> (response fp32 [P, I] with -1 at missing cells, mask bool [P, I]) as the reference stores them
        (datasets.py:928-940)."""
        c = self.codes
        mask = c != 2
        return torch.where(mask, c.float(), c.new_full((), -1, dtype=torch.float32)), mask


def pack_cell_codes(response, mask):
    """Repack device-resident [P, I(,1)] responses (+ mask or None) into CellCodes with vibo_pack_codes (one pass)."""
    response = prepare_response(response)
    mask, code = prepare_mask(mask, keep_int64=True)
    _require_device(response, mask)
    P, I = response.shape
    # row stride: whole 64-byte pieces for wide matrices (the matrix-pipe passes of the conditional posterior fetch 64 bytes
    # per row and load: 16-byte aligned, never straddling a 128-byte line), 16-byte rows otherwise
    I4 = (I + 63) // 64 * 64 if I >= 256 else (I + 15) // 16 * 16
    codes = torch.full((P, I4), 2, dtype=torch.uint8, device=response.device)       # padding cells read as missing
    spec = ElboSpec(irt_model=1, ability_dim=1)
    d = _rows_desc(spec, P, response, mask, code, _lib.REG_KL, False)
    _call('vibo_pack_codes', ctypes.byref(d), _ptr(response), _ptr(mask), _ptr(codes), ctypes.c_int64(I4), _stream(response.device))
    return CellCodes(codes[:, :I])


def prepare_rows(response, mask, keep_int64=False):
    """-> (response tensor, mask tensor or None, VIBO_MASK_* code) as the library reads them.  CellCodes rows come back
    as (codes, codes, MASK_CODES): the library ignores the response pointer then."""
    if isinstance(response, CellCodes):
        if mask is not None:
            raise ValueError('CellCodes rows carry their own missingness: pass mask=None')
        return response.codes, response.codes, _lib.MASK_CODES
    response = prepare_response(response)
    mask, code = prepare_mask(mask, keep_int64=keep_int64)
    return response, mask, code


def pad_rows(response, mask):
    """Device-resident copies of a [P, I] response / mask pair whose row strides are padded to a multiple of 4
    cells, returned as [P, I] views.  With I % 4 != 0 (CritLangAcq: 95 items) this keeps every row 16-byte aligned
    so the row-split kernel's vector loads apply; the padding cells are never interpreted (masked in the kernel)."""
    P, I = response.shape
    I4 = (I + 3) // 4 * 4
    if I4 == I:
        return response.contiguous(), (mask.contiguous() if mask is not None else None)
    r = torch.zeros(P, I4, dtype=response.dtype, device=response.device)
    r[:, :I] = response
    m = None
    if mask is not None:
        m = torch.zeros(P, I4, dtype=mask.dtype, device=mask.device)
        m[:, :I] = mask
        m = m[:, :I]
    return r[:, :I], m


def prepare_response(response):
    if response.dim() == 3:
        response = response.squeeze(2)
    if response.dtype != torch.float32:
        response = response.float()
    if response.stride(-1) != 1:
        response = response.contiguous()
    return response

_NOT_GIVEN = object()


def chunkable_rows(response, mask, row_index=_NOT_GIVEN):
    """-> (response, mask), or with a `row_index` argument (a tensor or None) -> (response, mask, row_index): rows that the kernels
    can read in chunks of 4 cells.  The caller-supplied-posterior modes (mean merge, VI, MLE) and the multi-sample forward have no
    fallback kernel for unchunkable rows, so a compact copy of rows whose width is no multiple of 4 (CritLangAcq: 95 items) is
    padded here (pad_rows); a row index is gathered first -- only the minibatch is copied -- and comes back as None.  CellCodes,
    widths that are multiples of 4 and rows that are padded already come back as they are."""
    if not isinstance(response, CellCodes):
        response = prepare_response(response)
        if response.shape[1] % 4 != 0 and response.stride(0) < (response.shape[1] + 3) // 4 * 4:
            mask = prepare_mask(mask)[0]
            if row_index is not _NOT_GIVEN and row_index is not None:
                response, mask, row_index = response[row_index], (mask[row_index] if mask is not None else None), None
            response, mask = pad_rows(response, mask)
    return (response, mask) if row_index is _NOT_GIVEN else (response, mask, row_index)


# vibo_desc.flags of every descriptor this module builds (_lib.FLAG_*): 0 = the planner chooses.  Tests and A/B tools
# pin one row-split kernel here; the library itself reads no environment variable.
DESC_FLAGS = 0


@contextlib.contextmanager
def desc_flags(flags):
    """`with ops.desc_flags(_lib.FLAG_KERNEL_MATRIX): ...` -- pin vibo_desc.flags for the calls inside and restore the
    previous value on the way out, also when the body raises (a bare assignment would leave a kernel pinned for the
    rest of the process)."""
    global DESC_FLAGS
    saved, DESC_FLAGS = DESC_FLAGS, int(flags)
    try:
        yield
    finally:
        DESC_FLAGS = saved


class InsituTimer:
    """The fused kernel's duration measured by the kernel itself (vibo_set_insitu_timer, include/vibo_hip.h): usable where HIP
    events are not -- inside a replayed hipGraph -- and without a tracer.  While armed (`with timer:`), every matrix row-split
    launch this host thread enqueues or captures stamps the block; `read()` returns the sums since the last `reset()`.
    A measurement hook for bench.py and tools/: the data path never looks at it."""

    TICK_MS = 1e-5      # s_memrealtime: 100 MHz

    def __init__(self, device):
        self.block = torch.zeros(8, dtype=torch.int64, device=device)
        self.reset()

    def reset(self):
        _call('vibo_insitu_timer_reset', _ptr(self.block), _stream(self.block.device))

    def arm(self):
        _call('vibo_set_insitu_timer', _ptr(self.block))

    @staticmethod
    def disarm():
        _call('vibo_set_insitu_timer', ctypes.c_void_p(0))

    def __enter__(self):
        self.arm()
        return self

    def __exit__(self, *exc):
        self.disarm()
        return False

    def counters(self):
        """(sum of ticks, launches) since the last reset, after synchronising the device."""
        torch.cuda.synchronize(self.block.device)
        w = self.block.cpu().tolist()
        return w[3], w[4]

    def read(self):
        torch.cuda.synchronize(self.block.device)
        w = self.block.cpu().tolist()
        n = w[4]
        if n <= 0:
            return {'launches': 0}
        k = self.TICK_MS
        return {'launches': n, 'mean_ms': w[3] / n * k, 'min_ms': w[5] * k, 'max_ms': w[6] * k, 'last_ms': w[7] * k,
                'in_flight': w[2] != 0}


def plan_kernel(spec, num_person, num_item, mask_code=_lib.MASK_U8, want_grad=True):
    """Name of the fused kernel the planner picks for a call of this shape (vibo_plan_kernel)."""
    d = _make_desc(spec, num_person, num_item, mask_code, _lib.REG_SAMPLED if spec.n_flows else _lib.REG_KL, want_grad,
                   (num_item + 3) & ~3, (num_item + 3) & ~3)
    k = _lib.load().vibo_plan_kernel(ctypes.byref(d))
    if k < 0:
        _lib.check(k, 'vibo_plan_kernel')
    return _lib.KERNEL_NAMES[k]


def _make_desc(spec, B, I, mask_code, reg_mode, want_grad, resp_stride, mask_stride):
    d = _lib.ViboDesc()
    d.flags = DESC_FLAGS
    d.abi_version = _lib.ABI_VERSION
    d.num_person = B
    d.num_item = I
    d.ability_dim = spec.ability_dim
    d.irt_model = spec.irt_model
    d.posterior = (_lib.POSTERIOR_GIVEN if spec.given else
                   _lib.POSTERIOR_CONDITIONAL if spec.conditional else _lib.POSTERIOR_UNCONDITIONAL)
    d.missing_mode = _lib.MISSING_DROP if spec.drop_missing else _lib.MISSING_PRIOR
    d.mask_dtype = mask_code
    d.reg_mode = reg_mode
    d.n_flows = spec.n_flows
    d.want_grad = 1 if want_grad else 0
    d.deterministic = 1
    d.response_row_stride = resp_stride
    d.mask_row_stride = mask_stride
    return d


def _rows_desc(spec, B, response, mask, mask_code, reg_mode, want_grad):
    """The descriptor of a call on B rows of (response, mask) as the library reads them (prepare_rows)."""
    return _make_desc(spec, B, response.shape[1], mask_code, reg_mode, want_grad, response.stride(0),
                      mask.stride(0) if mask is not None else 0)


def _stream(device):
    """torch's current stream on `device` as the hipStream_t argument of the library's calls."""
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _require_device(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError('vibo_amd: the fused ELBO runs on the GPU only (tensor on %s); '
                               'there is no CPU path' % t.device)


ROW_COUNT_CACHE = True     # (tests / A-B runs switch it off)


class ResidentMatrix:
    """One (response, mask) pair this process keeps calling with, as last seen, and what is known about it: the packed whole-row
    counts (vibo_row_counts; None until the matrix has come back), the stream they were produced on and an event behind them.
    ONE record per response tensor: a response that alternates between two masks is counted again at every switch.
    The record lives ON the response tensor (`_vibo_row_counts`): the counts are freed with the data they describe and never
    before -- a captured hipGraph that holds the data's address holds the counts' too.
    THE PROTOCOL of every fact kept here (the counts: _lookup_counts; `sign_is_mask`: _sign_rows; `tiles`: _tile_rows), once:
    - Eligibility comes first: a call its decider does not cover is never looked up and leaves no record.
    - The first sighting of a pair records it (lookup()), a later one produces the fact -- one pass over the matrix; that launch
      still goes out as the caller sent it --, the ones after it are served.  A "no" is remembered like a "yes".
    - An in-place write to response or mask (is_() reads the version counters), or another mask, starts over with a fresh record.
    - While the stream is capturing there are two regimes, and nothing is produced: _capture_bars."""
    __slots__ = ('response', 'has_mask', 'mask', 'counts', 'stream', 'event', 'in_graph', 'sign_is_mask', 'tiles')
    __reduce__ = _not_saved
    KNOWN, REPLACED, NEVER_SEEN = 'known', 'replaced', 'never seen'          # what lookup() found

    def __init__(self, response, mask):
        self.response, self.has_mask = _Seen(response), mask is not None
        self.mask = _Seen(_caller_mask(mask)) if self.has_mask else None
        self.counts = self.stream = self.event = None
        self.sign_is_mask = None              # does the responses' sign bit say what the mask says?  None: not verified yet (_sign_rows)
        self.in_graph = False                 # the count was recorded into a hipGraph: run when that graph replays
        self.tiles = None                     # the matrix' tile image (_tile_rows): None not decided yet, False none, else the uint8 tensor

    def is_(self, response, mask):
        """THE predicate: the same response, unmodified; a mask given then and now, or neither time (whatever became of the
        tensors); the same mask -- the caller's own or its narrowed form (prepare_mask) --, unmodified."""
        if self.has_mask != (mask is not None) or not self.response.is_(response):
            return False
        return not self.has_mask or self.mask.is_(_caller_mask(mask))

    @classmethod
    def lookup(cls, response, mask):
        """-> (the response's record for exactly this pair, what was found): KNOWN -- the record that was there --, or a fresh one
        planted in its place: REPLACED a stale record (an in-place write, another mask), NEVER_SEEN none."""
        rec = getattr(response, '_vibo_row_counts', None)
        if rec is not None and rec.is_(response, mask):
            return rec, cls.KNOWN
        response._vibo_row_counts = fresh = cls(response, mask)
        return fresh, cls.NEVER_SEEN if rec is None else cls.REPLACED


def _capture_bars(capturing, *, resident=False, gathered=False):
    """THE capture rule of the ELBO launch -> True: the stream is capturing and that keeps the launch from the ResidentMatrix record.
    A fact serves a captured launch only when that is a trainer's resident step (the contract "counted once") or reads gathered rows: a
    plain launch's captured input IS the matrix, and a replay after `response.copy_(new)` has to read what is there then.  Nothing is
    produced under capture (ask without the keywords).  capturing(): asked only where the answer matters."""
    return not (resident or gathered) and capturing()


def _lookup_counts(response, mask, rows, row_index, num_person, *, for_elbo, capturing, stream):
    """The one decision about a resident matrix' whole-row counts -> the counts, or None: the caller counts its own rows.
    response / mask: the tensors it is known by (CellCodes rows: the codes and None); rows: (response, mask, code) as
    _BACKEND['counts'] reads them, or a callable that prepares them; stream: the consumer's torch stream (None off the GPU), whose own
    methods do the ordering.  The ELBO launch (for_elbo): ResidentMatrix' protocol; gathered minibatches of the matrix are served too.
    row_counts(): a whole-matrix request counts and keeps at once, the first gathered minibatch of a tensor never seen gets None, and
    capture changes nothing -- but counts recorded into a graph are not handed to the ELBO launch: they exist once it has replayed."""
    whole = row_index is None
    if for_elbo and whole and num_person != response.shape[0]:
        return None
    rec, found = ResidentMatrix.lookup(response, mask)
    if found is not ResidentMatrix.KNOWN and (for_elbo or (found is ResidentMatrix.NEVER_SEEN and not whole)):
        return None
    if rec.counts is None:
        in_graph = stream is not None and _capture_bars(capturing)
        if for_elbo and in_graph:
            return None              # (a count recorded into a hipGraph would not have run when the next eager call reads it)
        rec.counts, rec.in_graph = _BACKEND['counts'](*(rows() if callable(rows) else rows), None), in_graph
        if stream is not None and not in_graph:
            rec.stream, rec.event = stream, stream.record_event()
    elif for_elbo and (rec.in_graph or _capture_bars(capturing, gathered=not whole)):
        return None
    elif rec.stream is not None and stream is not None and stream != rec.stream and not capturing():
        stream.wait_event(rec.event)     # (a capturing stream cannot wait on an eager event: its capture began behind the count)
    return rec.counts


def _resident_row_counts(spec, response, mask, mask_code, row_index, num_person, stream, *, capturing=torch.cuda.is_current_stream_capturing):
    """Whole-row counts for vibo_elbo_fwd_bwd_counts, or None.  Rows of more than 1024 items under the unconditional posterior are counted
    in a pass of their own in front of the panels (half of the call: 5 B/cell); a matrix that comes back is counted once: _lookup_counts."""
    I = response.shape[1]
    if (not ROW_COUNT_CACHE or spec.conditional or spec.given or I <= 1024 or I > 32767
            or mask_code not in (_lib.MASK_NONE, _lib.MASK_U8, _lib.MASK_CODES)):
        return None
    return _lookup_counts(response, None if mask_code == _lib.MASK_CODES else mask, (response, mask, mask_code), row_index,
                          num_person, for_elbo=True, capturing=capturing, stream=stream)


SIGN_ROWS = True           # (tests / A-B runs switch it off)


def _sign_rows(spec, response, mask, mask_code, row_index, num_person, reg_mode, want_grad, train_step, *, capturing):
    """The one decision about the row format of an ELBO launch -> (mask, mask_code) it goes out with: the caller's, or
    (None, MASK_SIGN) -- the matrix kernel then reads no mask bytes (4 instead of 5 B per cell) and takes a cell as missing where its
    response's sign bit is set, which is how the reference stores its data (-1 at missing cells, every mask built from that).
    Whether that holds for THESE tensors is verified, never assumed: the fact (`sign_is_mask`) follows the protocol of ResidentMatrix.
    Eligible: fp32 responses with a u8 mask, the whole matrix in order, rows the matrix kernel's 16-byte loads can take (base 16-byte
    aligned, stride a multiple of 4: a MASK_U8 call on other rows falls back to the tiled kernel, a MASK_SIGN call is refused), and
    a shape the library takes the format for (vibo_sign_rows_supported).  Producing the fact is one streaming pass and one .item();
    the resident step of the capture rule is the trainers' folded step here (train_step given)."""
    keep = (mask, mask_code)
    if (not SIGN_ROWS or mask is None or mask_code != _lib.MASK_U8 or response is None or response.dtype != torch.float32
            or row_index is not None or num_person != response.shape[0]
            or response.data_ptr() % 16 != 0 or response.stride(0) % 4 != 0):
        return keep
    if not _BACKEND['sign_supported'](_rows_desc(spec, num_person, response, None, _lib.MASK_SIGN, reg_mode, want_grad)):
        return keep
    rec, found = ResidentMatrix.lookup(response, mask)
    if found is not ResidentMatrix.KNOWN:
        return keep
    if rec.sign_is_mask is None:
        if not _capture_bars(capturing):
            rec.sign_is_mask = bool(_BACKEND['sign_verify'](response, mask))
        return keep                  # (the verifying launch itself still carries the mask)
    if not rec.sign_is_mask or _capture_bars(capturing, resident=train_step is not None):
        return keep
    return None, _lib.MASK_SIGN


def _hip_sign_rows_supported(d):
    return _lib.load().vibo_sign_rows_supported(ctypes.byref(d)) == 1


def _hip_sign_is_mask(response, mask):
    """vibo_rows_sign_is_mask on the current stream, waited for: True where every cell's mask byte and sign bit agree."""
    _require_device(response, mask)
    differs = torch.empty(1, dtype=torch.int32, device=response.device)
    d = _rows_desc(ElboSpec(irt_model=1, ability_dim=1), response.shape[0], response, mask, _lib.MASK_U8, _lib.REG_KL, False)
    _call('vibo_rows_sign_is_mask', ctypes.byref(d), _ptr(response), _ptr(mask), _ptr(differs), _stream(response.device))
    return int(differs.item()) == 0


TILE_ROWS = True                   # (tests / A-B runs switch it off)
# From this many persons on, every workgroup of an 8-wave launch on 256 compute units runs the matrix kernel's batch loop at least once
# (2 x 32 x 256 rows): below it the launch is that kernel's one-shot prologue and end code, and the loop the image shortens does not run.
TILE_ROWS_MIN_PERSONS = 16384
# Plain launches (fused_elbo, evaluation: no train_step) too?  Off: they run as they ran before the format existed -- an eager plain
# launch and the same launch replayed from a hipGraph, which must read the caller's rows in any case (_capture_bars), stay one kernel
# (the in-situ timer's test holds them within 25 % of each other).  On: an eager plain launch is a sighting and uses the image.
TILE_ROWS_PLAIN_LAUNCHES = False
# The image under a caller-supplied posterior (spec.given: the mean-merge, VI and MLE trainers' ELBO launch;
# include/vibo_hip_given_tiles.h).  Those launches are no folded step: the trainers mark theirs `resident_step`.
TILE_ROWS_GIVEN = True             # (tests / A-B runs switch it off; TILE_ROWS off turns this off too)
# ... and a minimum of its own on top of TILE_ROWS_MIN_PERSONS (0: none) for shapes that measure slower on the image
TILE_ROWS_GIVEN_MIN_PERSONS = 0


def _tile_rows(spec, response, mask, mask_code, row_index, num_person, reg_mode, want_grad, train_step, *, capturing,
               resident_step=False):
    """The one decision about a resident matrix' tile image (include/vibo_hip_tile_rows.h) -> the image this ELBO launch goes out on
    (a uint8 tensor: the launch is (image, None, MASK_TILES)), False (the launch keeps the caller's rows as they are: the matrix is
    on its way to an image, or a plain launch is being captured), or None (no image for this call: _sign_rows decides as ever).
    The matrix kernel then loads a batch's code words and counts instead of forming them from 4-5 bytes per cell: about 1.06 bytes
    per cell, no pack.  The image (`tiles`) follows the protocol of ResidentMatrix; it costs a byte per cell of device memory.
    Eligible: a trainer's resident step -- the folded step (train_step given), under a caller-supplied posterior (spec.given) the
    mean-merge, VI and MLE trainers' launch marked `resident_step` --, or any launch with TILE_ROWS_PLAIN_LAUNCHES on; the whole matrix
    in order -- fp32 responses with or without a u8 mask, or CellCodes -- in rows the matrix kernel itself can load
    (_matrix_kernel_rows); the thresholds above; a shape the library takes the format for.  Producing the image is one streaming pass,
    waited for, and only if it takes at most half of the free device memory -- an allocation that fails all the same is a "no".
    A matrix with a "no" is _sign_rows' from then on, and so is every launch not eligible here: with TILE_ROWS_PLAIN_LAUNCHES off, a
    plain launch on a matrix that has an image is _sign_rows', which verifies the pair as ever.  One image serves the plain and the
    given spec: it is built as the spec's plain twin would build it, under the matrix-kernel pin (no engine threshold in its answer)."""
    resident = resident_step if spec.given else train_step is not None       # (the two marks of a trainer's step on its resident matrix)
    if (not TILE_ROWS or (spec.given and (not TILE_ROWS_GIVEN or num_person < TILE_ROWS_GIVEN_MIN_PERSONS))
            or not (resident or TILE_ROWS_PLAIN_LAUNCHES) or response is None or row_index is not None or num_person != response.shape[0]
            or num_person < TILE_ROWS_MIN_PERSONS or mask_code not in (_lib.MASK_U8, _lib.MASK_NONE, _lib.MASK_CODES)
            or (mask_code != _lib.MASK_CODES and (response.dtype != torch.float32 or (mask is None) != (mask_code == _lib.MASK_NONE)))
            or not _matrix_kernel_rows(response, mask, mask_code)):
        return None
    if not _BACKEND['tile_given_supported' if spec.given else 'tile_supported'](_tile_desc(spec, num_person, response.shape[1], reg_mode, want_grad)):
        return None
    rec, found = ResidentMatrix.lookup(response, None if mask_code == _lib.MASK_CODES else mask)      # (CellCodes: known by the codes alone)
    if found is not ResidentMatrix.KNOWN:
        return False
    if rec.tiles is None:
        if _capture_bars(capturing):
            return False
        rec.tiles = False                                              # (a "no" until the image stands)
        with desc_flags(DESC_FLAGS | _lib.FLAG_KERNEL_MATRIX) if spec.given else contextlib.nullcontext():
            build_spec = replace(spec, given=False) if spec.given else spec
            need = _BACKEND['tile_bytes'](_tile_desc(build_spec, num_person, response.shape[1], reg_mode, want_grad))
            if 0 < need <= _BACKEND['tile_free'](response.device) // 2:        # (0 bytes: the builder may still refuse the shape)
                with contextlib.suppress(torch.cuda.OutOfMemoryError):
                    rec.tiles = _BACKEND['tile_build'](build_spec, response, mask, mask_code, num_person, reg_mode, want_grad, need)
        return False if rec.tiles is not False else None               # (the building launch itself still reads the caller's rows)
    if rec.tiles is False:
        return None
    return False if _capture_bars(capturing, resident=resident) else rec.tiles


def _matrix_kernel_rows(response, mask, mask_code):
    """Can the matrix kernel's chunk loads take these rows as they are -- bases aligned (16 bytes fp32, 4 bytes masks / codes), strides
    multiples of 4 that pad every row to whole chunks?  (A call on other rows falls back to the tiled kernel, whose last bits are
    its own: an image would change the results of such a matrix.)"""
    i4 = (response.shape[1] + 3) & ~3
    for t, align in ((None if mask_code == _lib.MASK_CODES else response, 16), (mask, 4)):
        if t is not None and (t.data_ptr() % align != 0 or t.stride(0) % 4 != 0 or t.stride(0) < i4):
            return False
    return True


def _tile_desc(spec, num_person, num_item, reg_mode, want_grad):
    """The descriptor of a launch on the tile image of a num_person x num_item matrix (the row strides are not read)."""
    i4 = (num_item + 3) & ~3
    return _make_desc(spec, num_person, num_item, _lib.MASK_TILES, reg_mode, want_grad, i4, i4)


def _hip_tile_rows_supported(d):
    return _lib.load().vibo_tile_rows_supported(ctypes.byref(d)) == 1


def _hip_given_tile_rows_supported(d):
    return _lib.load().vibo_given_tile_rows_supported(ctypes.byref(d)) == 1


def _hip_tile_rows_bytes(d):
    return int(_lib.load().vibo_tile_rows_bytes(ctypes.byref(d)))


def _hip_free_bytes(device):
    return int(torch.cuda.mem_get_info(device)[0])


def _hip_tile_rows_build(spec, response, mask, mask_code, num_person, reg_mode, want_grad, nbytes):
    """vibo_tile_rows_build on the current stream, waited for (any stream may read the image afterwards)."""
    _require_device(response, mask)
    image = torch.empty(nbytes, dtype=torch.uint8, device=response.device)
    src = _rows_desc(spec, num_person, response, mask, mask_code, reg_mode, want_grad)
    _call('vibo_tile_rows_build', ctypes.byref(src), _ptr(response), _ptr(mask), _ptr(image), ctypes.c_size_t(nbytes),
          _stream(response.device))
    torch.cuda.current_stream(response.device).synchronize()
    return image


class TrainStepCall(NamedTuple):
    """The folded train step's ELBO launch (trainer.FusedTrainer): vibo_elbo_fwd_bwd_step, the call that also ticks Adam's step counter."""
    step_count: torch.Tensor          # the trainer's int32[2] counters
    skip_finalize: bool               # the partial records stay in RawElbo.workspace and vibo_train_epilogue_fused fills `flat`
    # (seed, stream) where vibo_train_step_draws_noise says so (eps None): the kernel draws Philox stream `stream` at counter step_count[1] itself
    noise: Optional[tuple] = None     # ... and writes no posterior mean / log-variance (RawElbo.ability_mu / ability_logvar: None)
    # with noise, where vibo_train_step_sample_optional says so: ability = NULL, no [B, A] buffer; the caller sets RawElbo.ability_source
    no_sample: bool = False           # ... which rebuilds `ability` when read (trainer._StepSample)


# What one ELBO launch knows about its rows (_launch_rows): the tensors the library reads -- the caller's rows, or the matrix' tile image
# and no mask -- with their VIBO_MASK_* code, the launch's vibo_desc, by name the export that sizes the workspace for it and the one the
# launch goes into, the caller's row counts (vibo_elbo_fwd_bwd_counts) or None, and: is it on the image under a caller-supplied posterior?
LaunchRows = namedtuple('LaunchRows', 'response mask mask_code desc workspace_query entry counts given_tiles')


def _launch_rows(spec, response, mask, mask_code, row_index, num_person, reg_mode, want_grad, train_step, *, resident_step=False, capturing, stream):
    """THE decision about the rows of an ELBO launch -> LaunchRows, from the three deciders of the ResidentMatrix record in their one
    order: the tile image first (_tile_rows); the sign rows (_sign_rows) only where that answered "no image for this call" (None -- on
    False the caller's rows go out as they are); the resident counts (_resident_row_counts) only for a launch without train_step that
    is not on an image.  (With the library's shapes the three never meet on one matrix: the formats end at 1024 items, the counts
    begin above.)  train_step: None, a TrainStepCall or a plain tuple of its fields; capturing / stream: as the deciders take them."""
    launch = (spec, response, mask, mask_code, row_index, num_person, reg_mode, want_grad, train_step)
    image = _tile_rows(*launch, capturing=capturing, resident_step=resident_step)
    if image is None:
        mask, mask_code = _sign_rows(*launch, capturing=capturing)
    if image is None or image is False:
        d, given_tiles = _rows_desc(spec, num_person, response, mask, mask_code, reg_mode, want_grad), False
    else:
        d, given_tiles = _tile_desc(spec, num_person, response.shape[1], reg_mode, want_grad), spec.given
        response, mask, mask_code = image, None, _lib.MASK_TILES
    counts = None
    if train_step is not None:
        entry = 'vibo_elbo_fwd_bwd_step_noise' if len(train_step) > 2 and train_step[2] is not None else 'vibo_elbo_fwd_bwd_step'
    else:
        if mask_code != _lib.MASK_TILES:
            counts = _resident_row_counts(spec, response, mask, mask_code, row_index, num_person, stream, capturing=capturing)
        entry = 'vibo_elbo_fwd_bwd_given_tiles' if given_tiles else 'vibo_elbo_fwd_bwd' if counts is None else 'vibo_elbo_fwd_bwd_counts'
    return LaunchRows(response, mask, mask_code, d, 'vibo_given_tiles_workspace_bytes' if given_tiles else 'vibo_workspace_bytes',
                      entry, counts, given_tiles)


def _hip_launch_elbo(spec, response, mask, mask_code, row_index, table, item, eps, flow, reg_mode,
                     want_grad, num_person, train_step=None, *, resident_step=False):
    """Single call into the ELBO export _launch_rows names, on the current stream.  train_step: a TrainStepCall -- the folded step;
    resident_step: a trainer's whole-matrix launch under a caller-supplied posterior (spec.given), see _tile_rows."""
    _require_device(response, mask, table, item, eps)
    dev = response.device
    I = response.shape[1]
    B = int(num_person)
    A, D = spec.ability_dim, spec.item_dim
    table_shape = tuple(table.shape) if table is not None else tuple(spec.table_shape(I))
    n_table, n_item, n_flow = math.prod(table_shape), I * D, spec.n_flows * (2 * A + 1)
    flat = torch.empty(_lib.NUM_SCALARS + 2 * n_table + n_item + 2 * n_flow, dtype=torch.float32, device=dev)
    train_step = None if train_step is None else TrainStepCall(*train_step)      # (a plain tuple of the same fields is taken too)
    own_noise = train_step is not None and train_step.noise is not None
    no_sample = own_noise and bool(train_step.no_sample)
    # posterior mean | log-variance | sample: the drawing step writes the sample alone, or nothing
    post = None if no_sample else torch.empty(1 if own_noise else 3, B, A, dtype=torch.float32, device=dev)
    ability_k = torch.empty(B, A, dtype=torch.float32, device=dev) if spec.n_flows else None
    ladj = torch.empty(B, dtype=torch.float32, device=dev) if spec.n_flows else None
    stream = torch.cuda.current_stream(dev)
    sent = _launch_rows(spec, response, mask, mask_code, row_index, B, reg_mode, want_grad, train_step, resident_step=resident_step,
                        capturing=torch.cuda.is_current_stream_capturing, stream=stream)
    ws_bytes = getattr(_lib.load(), sent.workspace_query)(ctypes.byref(sent.desc))
    if ws_bytes == 0:
        _lib.check(-1, sent.workspace_query)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    vp, fbase, o_item = ctypes.c_void_p, flat.data_ptr(), _lib.NUM_SCALARS + 2 * n_table
    # the argument runs the exports share (include/vibo_hip.h): the rows, the gradients, workspace and stream
    rows = (_ptr(sent.response), _ptr(sent.mask), _ptr(row_index))
    grads = (vp(fbase + 4 * _lib.NUM_SCALARS), vp(fbase + 4 * o_item))
    tail = (_ptr(ws), ctypes.c_size_t(ws_bytes), vp(stream.cuda_stream))
    if own_noise:
        args = (_ptr(train_step.step_count), 1 if train_step.skip_finalize else 0, *rows, _ptr(table), _ptr(item), None,
                ctypes.c_uint64(train_step.noise[0]), ctypes.c_uint32(train_step.noise[1]), vp(fbase), None, None,
                None if no_sample else _ptr(post[0]), *grads, *tail)
    elif train_step is not None:
        args = (_ptr(train_step.step_count), 1 if train_step.skip_finalize else 0, *rows, _ptr(table), _ptr(item), _ptr(eps), vp(fbase),
                _ptr(post[0]), _ptr(post[1]), _ptr(post[2]), *grads, *tail)
    else:
        args = (*rows, *(() if sent.counts is None else (_ptr(sent.counts),)), _ptr(table), _ptr(item), _ptr(eps), _ptr(flow), vp(fbase),
                _ptr(post[0]), _ptr(post[1]), _ptr(post[2]), _ptr(ability_k), _ptr(ladj), *grads,
                vp(fbase + 4 * (o_item + n_item)) if n_flow else vp(0), *tail)
    _call(sent.entry, ctypes.byref(sent.desc), *args)
    raw = RawElbo(flat=flat, n_table=n_table, n_item=n_item, n_flow=n_flow, table_shape=table_shape,
                  ability_mu=None if own_noise else post[0], ability_logvar=None if own_noise else post[1],
                  ability=None if no_sample else post[-1],
                  ability_k=ability_k, ability_ladj=ladj)
    if train_step is not None and train_step.skip_finalize:
        raw.workspace = ws          # (kept alive until the epilogue has summed the partial records)
    return raw


def multi_forward_declined(spec, response, mask, mask_code, num_samples, num_person):
    """True where the native multi-sample backend is installed and its workspace query already says that it does not cover the
    call (vibo_multi_cond_workspace_bytes == 0: cell codes at ability_dim >= 3, int64 masks, ...) -- asked from the descriptor
    alone, before a caller draws noise or stacks S tables for a call that would answer None.  False for any other backend (the CPU
    stand-in, a test's fake: they answer for themselves) and for rows off the device."""
    if _BACKEND['multi'] is not _hip_multi_forward or _multi_mode(spec) != 'cond' or not response.is_cuda:
        return False
    d = _rows_desc(spec, int(num_person), response, mask, mask_code, _lib.REG_SAMPLED, False)
    return _lib.load().vibo_multi_cond_workspace_bytes(ctypes.byref(d), int(num_samples)) == 0


# The three multi-sample entries by posterior mode: workspace query, entry, what `table` must be (None: unchecked) and the shapes
# that means, and the arguments that entry alone takes: (those after `table`, those after `out_scalars`)
_MULTI_CALLS = {
    'plain': ('vibo_multi_workspace_bytes', 'vibo_elbo_multi_forward', None, None,
              lambda table, B, A: ((), ())),
    'given': ('vibo_multi_given_workspace_bytes', 'vibo_elbo_multi_forward_given',
              'the posterior is a contiguous [B, 2A] or [S, B, 2A] tensor', lambda S, B, I, A: ((B, 2 * A), (S, B, 2 * A)),
              lambda table, B, A: ((ctypes.c_int64(B * 2 * A if table.dim() == 3 else 0),), ())),      # posterior_sample_stride
    'cond': ('vibo_multi_cond_workspace_bytes', 'vibo_elbo_multi_forward_cond',
             'the conditional posterior takes a contiguous [S, 2, I, 2A] table', lambda S, B, I, A: ((S, 2, I, 2 * A),),
             lambda table, B, A: ((), (None,))),                                                        # posterior_out
}


def _multi_mode(spec):
    return 'given' if spec.given else 'cond' if spec.conditional else 'plain'


def _hip_multi_forward(spec, response, mask, mask_code, row_index, table, items, eps, flow, reg_mode, num_person):
    """vibo_elbo_multi_forward: S forward evaluations in one pass.  items [S,I,D], eps [S,B,A] -> scalars [S,8], or
    None when the configuration is not on the row-split path (the caller then loops over single launches).
    spec.given (vibo_elbo_multi_forward_given): `table` is the caller's posterior (mu | logvar) in minibatch order, [B, 2A] shared
    by the samples or [S, B, 2A] one per sample.
    spec.conditional without given (vibo_elbo_multi_forward_cond): `table` is the encoder's table of every item sample,
    [S, 2, I, 2A]; rows that are not on the device also answer None (the caller's loop then meets its own backend)."""
    mode = _multi_mode(spec)
    query, name, table_rule, table_shapes, extra = _MULTI_CALLS[mode]
    if mode == 'cond' and not response.is_cuda:
        return None
    lib = _lib.load()
    _require_device(response, mask, table, items, eps)
    S, B, I, A = int(items.shape[0]), int(num_person), response.shape[1], spec.ability_dim
    d = _rows_desc(spec, B, response, mask, mask_code, reg_mode, False)
    ws_bytes = getattr(lib, query)(ctypes.byref(d), S)
    if ws_bytes == 0:
        return None
    if table_rule is not None and (tuple(table.shape) not in table_shapes(S, B, I, A) or not table.is_contiguous()):
        raise ValueError('multi-sample forward: %s, got %s' % (table_rule, tuple(table.shape)))
    after_table, after_out = extra(table, B, A)
    dev = response.device
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    out = torch.empty(S, _lib.NUM_SCALARS, dtype=torch.float32, device=dev)
    rc = getattr(lib, name)(ctypes.byref(d), S, _ptr(response), _ptr(mask), _ptr(row_index), _ptr(table), *after_table,
                            _ptr(items), _ptr(eps), _ptr(flow), _ptr(out), *after_out, _ptr(ws), ctypes.c_size_t(ws_bytes), _stream(dev))
    if rc == -8:
        return None
    _lib.check(rc, name)
    return out


def _hip_encode(spec, response, mask, mask_code, row_index, table, num_person):
    lib = _lib.load()
    _require_device(response, mask, table)
    dev = response.device
    B, A = int(num_person), spec.ability_dim
    out = torch.empty(2, B, A, dtype=torch.float32, device=dev)
    # (the posterior does not depend on the flows; the descriptor only has to be self-consistent)
    d = _rows_desc(spec, B, response, mask, mask_code, _lib.REG_SAMPLED if spec.n_flows else _lib.REG_KL, False)
    ws_bytes = lib.vibo_workspace_bytes(ctypes.byref(d))          # scratch for the row statistics of the fast path
    ws = torch.empty(max(ws_bytes, 256), dtype=torch.uint8, device=dev)
    _call('vibo_encode', ctypes.byref(d), _ptr(response), _ptr(mask), _ptr(row_index), _ptr(table),
          _ptr(out[0]), _ptr(out[1]), _ptr(ws), ctypes.c_size_t(ws_bytes), _stream(dev))
    return out[0], out[1]


def _hip_decode(spec, ability, item):
    _require_device(ability, item)
    B, I = ability.shape[0], item.shape[0]
    out = torch.empty(B, I, dtype=torch.float32, device=ability.device)
    d = _make_desc(spec, B, I, _lib.MASK_NONE, _lib.REG_SAMPLED if spec.n_flows else _lib.REG_KL, False, I, 0)
    _call('vibo_decode', ctypes.byref(d), _ptr(ability), _ptr(item), _ptr(out), _stream(ability.device))
    return out


def _hip_row_counts(response, mask, mask_code, row_index):
    """vibo_row_counts: int32 [B], n_correct << 16 | n_observed per person row."""
    _require_device(response, mask)
    B = int(row_index.numel()) if row_index is not None else response.shape[0]
    out = torch.empty(B, dtype=torch.int32, device=response.device)
    d = _rows_desc(ElboSpec(irt_model=1, ability_dim=1), B, response, mask, mask_code, _lib.REG_KL, False)
    _call('vibo_row_counts', ctypes.byref(d), _ptr(response), _ptr(mask), _ptr(row_index), _ptr(out), _stream(response.device))
    return out


def row_counts(response, mask, row_index=None):
    """int32 [B]: n_correct << 16 | n_observed per person -- the sufficient statistics of a Bernoulli response row for
    the unconditional encoders (here: the masked mean of --ability-merge mean, models.py:631-650).  The counts of a whole
    matrix are kept while the same (unmodified) tensors come back -- a resident dataset is counted once, not per step;
    minibatches gathered through `row_index` index into them.  Under hipGraph capture too: the mean-merge and decoder trainers'
    captured steps read their resident matrix's counts, computed once (unlike the ELBO launch, _lookup_counts)."""
    key = response.codes if isinstance(response, CellCodes) else response       # the caller's own tensor objects
    cnt = _lookup_counts(key, mask, lambda: prepare_rows(response, mask, keep_int64=True), row_index, key.shape[0], for_elbo=False,
                         capturing=torch.cuda.is_current_stream_capturing,
                         stream=torch.cuda.current_stream(key.device) if key.is_cuda else None)
    if cnt is None:
        # a gathered minibatch of a matrix seen for the first time: count those rows only; the whole matrix is counted
        # (once) when the same tensor comes back
        return _BACKEND['counts'](*prepare_rows(response, mask, keep_int64=True), row_index)
    return cnt if row_index is None else cnt[row_index]


def _mean_desc(counts, A):
    return _make_desc(ElboSpec(irt_model=1, ability_dim=A), int(counts.numel()), 1, _lib.MASK_NONE, _lib.REG_KL, False, 1, 0)


def _hip_mean_encoder_fwd(counts, u, v, w2, b2):
    _require_device(counts, u, v, w2, b2)
    A2, H = w2.shape
    post = torch.empty(counts.numel(), A2, dtype=torch.float32, device=counts.device)
    d = _mean_desc(counts, A2 // 2)
    _call('vibo_mean_encoder_forward', ctypes.byref(d), H, _ptr(counts), _ptr(u), _ptr(v), _ptr(w2), _ptr(b2), _ptr(post),
          _stream(counts.device))
    return post


def _hip_mean_encoder_bwd(counts, u, v, w2, gpost):
    """-> (d/du [H], d/dv [H], d/dW2 [2A,H], d/db2 [2A]) summed over the persons."""
    lib = _lib.load()
    _require_device(counts, u, v, w2, gpost)
    A2, H = w2.shape
    d = _mean_desc(counts, A2 // 2)
    n_part = lib.vibo_mean_encoder_partials(ctypes.byref(d))
    part = torch.empty(n_part, 2 * H + A2 * H + A2, dtype=torch.float32, device=counts.device)
    _call('vibo_mean_encoder_backward', ctypes.byref(d), H, _ptr(counts), _ptr(u), _ptr(v), _ptr(w2), _ptr(gpost), _ptr(part),
          n_part, _stream(counts.device))
    tot = part.sum(0)
    return tot[:H], tot[H:2 * H], tot[2 * H:2 * H + A2 * H].view(A2, H), tot[2 * H + A2 * H:]


class MeanEncoderFn(torch.autograd.Function):
    """(u, v, W2, b2) -> posterior [B, 2A] = W2 elu(u + w_p v) + b2 with w_p from the packed row counts
    (vibo_mean_encoder_forward / _backward; see include/vibo_hip.h)."""

    @staticmethod
    def forward(ctx, u, v, w2, b2, counts):
        u, v, w2, b2 = (t.detach().contiguous().float() for t in (u, v, w2, b2))
        ctx.save_for_backward(u, v, w2, counts)
        return _BACKEND['mean_fwd'](counts, u, v, w2, b2)

    @staticmethod
    def backward(ctx, g):
        u, v, w2, counts = ctx.saved_tensors
        gu, gv, gw2, gb2 = _BACKEND['mean_bwd'](counts, u, v, w2, g.contiguous().float())
        return gu, gv, gw2, gb2, None


class FlowStackFn(torch.autograd.Function):
    """(z [N, D], packed [K, 2D+1] = uhat | w | b) -> (z_K [N, D], ladj [N]): a stack of planar flows in two launches
    (vibo_flow_stack_forward / _backward) instead of ~35 small PyTorch kernels per flow and direction."""

    @staticmethod
    def forward(ctx, z, packed):
        z, packed = z.detach().contiguous().float(), packed.detach().contiguous().float()
        _require_device(z, packed)
        N, D = z.shape
        K = packed.shape[0]
        z_out, ladj, th = torch.empty_like(z), torch.empty(N, dtype=torch.float32, device=z.device), torch.empty(N, K, dtype=torch.float32, device=z.device)
        _call('vibo_flow_stack_forward', N, D, K, _ptr(z), _ptr(packed), _ptr(z_out), _ptr(ladj), _ptr(th), _stream(z.device))
        ctx.save_for_backward(z_out, packed, th)
        return z_out, ladj

    @staticmethod
    def backward(ctx, g_z, g_l):
        z_out, packed, th = ctx.saved_tensors
        N, D = z_out.shape
        K = packed.shape[0]
        g_z = torch.zeros_like(z_out) if g_z is None else g_z.contiguous().float()
        g_l = torch.zeros(N, dtype=torch.float32, device=z_out.device) if g_l is None else g_l.contiguous().float()
        g_in = torch.empty_like(z_out)
        parts = torch.empty((N + 255) // 256, K, 2 * D + 1, dtype=torch.float32, device=z_out.device)
        _call('vibo_flow_stack_backward', N, D, K, _ptr(z_out), _ptr(packed), _ptr(th), _ptr(g_z), _ptr(g_l), _ptr(g_in),
              _ptr(parts), _stream(z_out.device))
        return g_in, parts.sum(0)


def _hip_flow_stack(z, packed):
    return FlowStackFn.apply(z, packed)


def _hip_decode_mean(spec, abilities, items):
    """vibo_decode_mean: abilities [S,B,A], items [S,I,D] -> mean over S of P(response = 1) [B,I]."""
    _require_device(abilities, items)
    S, B, I = int(abilities.shape[0]), int(abilities.shape[1]), int(items.shape[1])
    out = torch.empty(B, I, dtype=torch.float32, device=abilities.device)
    d = _make_desc(spec, B, I, _lib.MASK_NONE, _lib.REG_SAMPLED if spec.n_flows else _lib.REG_KL, False, I, 0)
    _call('vibo_decode_mean', ctypes.byref(d), S, _ptr(abilities), _ptr(items), _ptr(out), _stream(abilities.device))
    return out


class CodeTableSumFn(torch.autograd.Function):
    """S[p, :] = sum over person p's observed cells of feature[code_pi, i, :]  (vibo_code_table_sum_forward / _backward: the
    one-hot [B, 2I] x [2I, H] contraction of --ability-merge mean with --conditional-posterior and its transpose, on the
    matrix pipe from the 1-byte cell codes).  feature [2, I, 64] fp32; codes = CellCodes of the minibatch's rows."""

    @staticmethod
    def forward(ctx, feature, cell_codes):
        lib = _lib.load()
        codes = cell_codes.codes
        B, I = codes.shape
        H = feature.shape[2]
        feat = feature.detach().contiguous().float()
        _require_device(feat, codes)
        out = torch.empty(B, H, dtype=torch.float32, device=codes.device)
        nbytes = lib.vibo_code_table_scratch_bytes(B, I, H)
        if nbytes == 0:
            raise _lib.ViboLibraryError('vibo_code_table_sum: hidden_dim must be 64')
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=codes.device)
        _call('vibo_code_table_sum_forward', B, I, H, _ptr(codes), codes.stride(0), _ptr(feat), _ptr(out), _ptr(scratch), nbytes,
              _stream(codes.device))
        ctx.cell_codes, ctx.shape = cell_codes, (I, H)
        return out

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        codes = ctx.cell_codes.codes
        B = codes.shape[0]
        I, H = ctx.shape
        g = g.contiguous().float()
        dfeat = torch.empty(2, I, H, dtype=torch.float32, device=codes.device)
        nbytes = lib.vibo_code_table_scratch_bytes(B, I, H)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=codes.device)
        _call('vibo_code_table_sum_backward', B, I, H, _ptr(codes), codes.stride(0), _ptr(g), _ptr(dfeat), _ptr(scratch), nbytes,
              _stream(codes.device))
        return dfeat, None


def _hip_cond_mean_sum(feature, response, mask, row_index):
    """(S [B, H], n_observed [B]) for the minibatch: the cells as CellCodes (packed here from fp32 rows + mask if need be),
    the sum on the matrix pipe (CodeTableSumFn), the observed counts from vibo_row_counts."""
    if isinstance(response, CellCodes):
        cc = response.rows(row_index) if row_index is not None else response
    else:
        r = prepare_response(response)
        m = None if mask is None else prepare_mask(mask)[0]
        if row_index is not None:
            r, m = r[row_index], (None if m is None else m[row_index])
        cc = pack_cell_codes(r, m)
    if cc.codes.shape[1] > 32767:
        # (vibo_row_counts packs n_correct << 16 | n_observed into an int32: wider rows are counted by torch -- one more pass over
        #  the codes, on a width the reference itself never trains at)
        nobs = (cc.codes != 2).sum(dim=1).to(feature.dtype)
    else:
        counts = _BACKEND['counts'](cc.codes, cc.codes, _lib.MASK_CODES, None)
        nobs = (counts & 0xffff).to(feature.dtype)
    return CodeTableSumFn.apply(feature, cc), nobs


# The entry points of the native library.  tests/ swap these for the CPU
# oracle to exercise the host logic without a GPU (never done by product code).
_BACKEND = {'elbo': _hip_launch_elbo, 'encode': _hip_encode, 'decode': _hip_decode, 'multi': _hip_multi_forward,
            'decode_mean': _hip_decode_mean, 'counts': _hip_row_counts, 'mean_fwd': _hip_mean_encoder_fwd,
            'mean_bwd': _hip_mean_encoder_bwd, 'flow_stack': _hip_flow_stack, 'cond_mean_sum': _hip_cond_mean_sum,
            'sign_supported': _hip_sign_rows_supported, 'sign_verify': _hip_sign_is_mask,
            'tile_supported': _hip_tile_rows_supported, 'tile_bytes': _hip_tile_rows_bytes, 'tile_free': _hip_free_bytes,
            'tile_build': _hip_tile_rows_build, 'tile_given_supported': _hip_given_tile_rows_supported,
            # sparse rows (vibo_amd/sparse.py): the launch, the encode and the validation pass
            'sparse_elbo': _sparse._hip_sparse_elbo, 'sparse_encode': _sparse._hip_sparse_encode, 'sparse_check': _sparse._hip_sparse_check}


class FusedELBO(torch.autograd.Function):
    """(table, item, flow) -> (LL, REG, scalars, ability_mu, ability_logvar,
    ability, ability_k, ability_ladj).

    LL  = sum of masked Bernoulli log-likelihoods (utils.py:46-49, models.py:399)
    REG = sum_p KL(q(theta_p)||N(0,1))  (reg_mode KL,  models.py:428) or
          sum_p [log q(theta_p) - log p(theta_p)] at the sample (SAMPLED, models.py:412-418,433-435)
    The kernel has already produced d LL/d(.) and d REG/d(.); backward only scales
    and adds them, so loss.backward() costs no second pass over the responses.
    """

    @staticmethod
    def forward(ctx, table, item, flow, response, mask, mask_code, row_index, eps, spec, reg_mode,
                num_person, reducer):
        need_grad = any(ctx.needs_input_grad[:3])
        table_c = table.detach().contiguous()
        item_c = item.detach().contiguous()
        flow_c = flow.detach().contiguous() if flow is not None else None
        raw = _BACKEND['elbo'](spec, response, mask, mask_code, row_index, table_c, item_c,
                               eps.contiguous(), flow_c, reg_mode, need_grad, num_person)
        if reducer is not None:      # person-sharded data parallelism: ONE all-reduce (RCCL) per step
            if spec.given:           # (the per-person posterior gradients in the middle of the buffer stay local)
                reducer(raw.flat[:_lib.NUM_SCALARS])
                if raw.n_item + 2 * raw.n_flow:
                    reducer(raw.flat[_lib.NUM_SCALARS + 2 * raw.n_table:])
            else:
                reducer(raw.flat)
        ctx.raw = raw
        ctx.item_shape = tuple(item.shape)
        ctx.has_flow = flow is not None
        ctx.need_grad = need_grad
        sc = raw.scalars
        outs = (sc[_lib.S_LL].clone(), sc[_lib.S_REG].clone(), sc.clone(),
                raw.ability_mu, raw.ability_logvar, raw.ability,
                raw.ability_k if raw.ability_k is not None else raw.ability,
                raw.ability_ladj if raw.ability_ladj is not None else sc.new_zeros(()))
        ctx.mark_non_differentiable(*outs[2:])
        return outs

    @staticmethod
    def backward(ctx, g_ll, g_reg, *_):
        raw = ctx.raw
        if not ctx.need_grad:
            return (None,) * 12
        g_table = g_item = g_flow = None
        if ctx.needs_input_grad[0]:
            g_table = g_ll * raw.grad_table(0) + g_reg * raw.grad_table(1)
        if ctx.needs_input_grad[1]:
            g_item = g_ll * raw.grad_item(ctx.item_shape)
        if ctx.has_flow and ctx.needs_input_grad[2]:
            g_flow = (g_ll * raw.grad_flow(0) + g_reg * raw.grad_flow(1)).view(-1, 2 * raw.ability_mu.shape[1] + 1)
        return (g_table, g_item, g_flow) + (None,) * 9


def fused_elbo(spec, table, item, flow, response, mask, eps, *, reg_mode=_lib.REG_KL, row_index=None,
               reducer=None):
    """Functional front end.  response [B,I(,1)] fp32, mask [B,I(,1)] bool/int64/None,
    table per ElboSpec.table_shape, item [I,D], eps [B,A], flow [n_flows,2A+1] or None.
    With row_index (int64 [B]) the rows response[row_index] / mask[row_index] are
    gathered inside the kernel (device-resident dataset, shuffled minibatches).
    response may be a SparseRows (mask None, row_index None or a range of consecutive persons): vibo_amd/sparse.py."""
    if isinstance(response, SparseRows):
        return _sparse.fused_elbo(spec, table, item, flow, response, mask, eps, reg_mode=reg_mode, row_index=row_index, reducer=reducer)
    response, mask, code = prepare_rows(response, mask)
    I = response.shape[1]
    spec.check_supported(I)
    B = int(row_index.numel()) if row_index is not None else response.shape[0]
    if tuple(table.shape) != spec.table_shape(I, B):
        raise ValueError(f'table shape {tuple(table.shape)} != {spec.table_shape(I, B)}')
    if tuple(item.shape) != (I, spec.item_dim):
        raise ValueError(f'item shape {tuple(item.shape)} != {(I, spec.item_dim)}')
    if tuple(eps.shape) != (B, spec.ability_dim):
        raise ValueError(f'eps shape {tuple(eps.shape)} != {(B, spec.ability_dim)}')
    return FusedELBO.apply(table, item, flow, response, mask, code, row_index, eps, spec, reg_mode, B, reducer)


def encode_posterior(spec, table, response, mask, row_index=None):
    """Forward-only q(ability | responses): (mu, logvar) [B,A] (models.py:356-371 under no_grad)."""
    if isinstance(response, SparseRows):
        return _sparse.encode_posterior(spec, table, response, mask, row_index=row_index)
    response, mask, code = prepare_rows(response, mask)
    B = int(row_index.numel()) if row_index is not None else response.shape[0]
    return _BACKEND['encode'](spec, response, mask, code, row_index, table.detach().contiguous(), B)


def decode_probs_mean(spec, abilities, items):
    """Mean over S posterior draws of P(response = 1): abilities [S,B,A], items [S,I,D] -> [B,I]
    (vibo.py:363-390 reduced as at :504-548, without the [S,B,I] stack)."""
    return _BACKEND['decode_mean'](spec, abilities.detach().contiguous().float(), items.detach().contiguous().float())


def decode_probs(spec, ability, item):
    """P(response = 1) [B,I] (models.py:729-766)."""
    return _BACKEND['decode'](spec, ability.detach().contiguous().float(), item.detach().contiguous().float())
