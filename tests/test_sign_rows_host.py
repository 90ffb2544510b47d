"""Sign-as-mask fp32 rows (include/vibo_hip_sign_rows.h, VIBO_MASK_SIGN) without a GPU: what the library's validation answers for the
format, that the new header is bound while vibo_hip.h keeps its lists, and ops._sign_rows -- the one place that decides whether an
ELBO launch goes out without its mask -- driven with fake backend entries and a fake capturing()."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT
from row_format_common import _null_call, desc, matrix
from vibo_amd import _lib, ops

SIGN_ENTRY_POINTS = {'vibo_elbo_fwd_bwd', 'vibo_elbo_fwd_bwd_step', 'vibo_elbo_fwd_bwd_step_noise', 'vibo_workspace_bytes',
                     'vibo_plan_kernel', 'vibo_train_step_supported', 'vibo_train_step_draws_noise', 'vibo_train_step_sample_optional'}


GRID = {'headline': {}, 'ability_dim 1': dict(A=1), '3PL forward only': dict(irt=3, grad=0), '132 items pinned': dict(B=500, I=132, flags=_lib.FLAG_KERNEL_MATRIX),
        'conditional': dict(posterior=_lib.POSTERIOR_CONDITIONAL), 'flows': dict(n_flows=2), '2000 items': dict(I=2000),
        'VALU pinned': dict(flags=_lib.FLAG_KERNEL_VALU), '16 persons': dict(B=16), 'rows not chunkable': dict(I=997, stride=997),
        'narrow rows': dict(I=96, A=1), 'caller-supplied posterior': dict(posterior=_lib.POSTERIOR_GIVEN)}
SUPPORTED = {'headline', 'ability_dim 1', '3PL forward only', '132 items pinned'}


@pytest.mark.parametrize('case', sorted(GRID))
def test_supported_query_and_plan(case):
    lib = _lib.load()
    d = desc(**GRID[case])
    ok = case in SUPPORTED
    assert lib.vibo_sign_rows_supported(ctypes.byref(d)) == (1 if ok else 0)
    plan = lib.vibo_plan_kernel(ctypes.byref(d))
    if ok:
        assert plan == 1 and _lib.KERNEL_NAMES[plan].startswith('matrix') and lib.vibo_workspace_bytes(ctypes.byref(d)) > 0
    else:
        assert plan == -8 and b'VIBO_MASK_SIGN' in lib.vibo_last_error_string() and lib.vibo_workspace_bytes(ctypes.byref(d)) == 0
    # the two step queries: what they answer for the same descriptor with a u8 mask
    u8 = desc(**{**GRID[case], 'mask': _lib.MASK_U8})
    for fn in (lib.vibo_train_step_supported, lib.vibo_train_step_draws_noise):
        assert fn(ctypes.byref(d)) == fn(ctypes.byref(u8)), fn
    assert lib.vibo_train_step_sample_optional(ctypes.byref(d), 0) == lib.vibo_train_step_sample_optional(ctypes.byref(u8), 0)
    assert lib.vibo_workspace_bytes(ctypes.byref(d)) in (0, lib.vibo_workspace_bytes(ctypes.byref(u8)))


def test_supported_query_wants_the_format_itself():
    lib = _lib.load()
    assert lib.vibo_sign_rows_supported(ctypes.byref(desc(mask=_lib.MASK_U8))) == 0 and lib.vibo_sign_rows_supported(None) == 0
    assert lib.vibo_plan_kernel(ctypes.byref(desc(mask=5))) == -3


def test_every_other_export_refuses_the_format_before_any_launch():
    """Every export of vibo_hip.h that takes a descriptor, with a VIBO_MASK_SIGN descriptor of the headline shape and NULL pointers: the
    entry points of the format get past the descriptor (-5: the NULL pointers), all others answer -8 -- size queries 0, the one
    offset query -1 -- from validation (nothing can launch on NULL pointers, and there is no GPU here)."""
    lib = _lib.load()
    d = desc()
    dp = ctypes.POINTER(_lib.ViboDesc)
    seen = 0
    for name, restype, argtypes in _lib.PROTOTYPES:
        if not argtypes or argtypes[0] is not dp:
            continue
        seen += 1
        rc = _null_call(getattr(lib, name), d)
        if name in SIGN_ENTRY_POINTS:
            if name.startswith('vibo_elbo'):
                assert rc == -5, (name, rc)
            continue
        if restype is ctypes.c_size_t or name in ('vibo_ctrain_param_floats', 'vibo_ctrain_scratch_floats', 'vibo_dtrain_param_floats',
                                                  'vibo_dtrain_scratch_floats', 'vibo_mtrain_param_floats', 'vibo_mean_encoder_partials'):
            assert rc == 0, (name, rc)
        elif name == 'vibo_dtrain_scratch_offset':
            assert rc == -1, (name, rc)
        else:
            assert rc == -8, (name, rc)
    assert seen >= 40
    # the format's own entry points refuse what is not implemented: gathered rows, caller-supplied counts (through its own export above)
    assert lib.vibo_elbo_fwd_bwd(ctypes.byref(d), None, None, ctypes.c_void_p(64), *([None] * 14), 0, None) == -8
    assert b'row_index' in lib.vibo_last_error_string()
    assert lib.vibo_rows_sign_is_mask(ctypes.byref(d), None, None, None, None) == -8          # (the verifier reads u8-mask rows)
    assert lib.vibo_rows_sign_is_mask(ctypes.byref(desc(mask=_lib.MASK_U8)), None, None, None, None) == -5


def test_new_header_is_bound_and_the_main_header_keeps_its_lists():
    assert 'vibo_hip_sign_rows.h' in _lib.EXTRA_HEADERS and _lib.MASK_SIGN == 4
    assert _lib.SIGN_ROWS_SYMBOLS == ('vibo_sign_rows_supported', 'vibo_rows_sign_is_mask')
    assert set(_lib.SIGN_ROWS_SYMBOLS) <= {name for name, _, _ in _lib.EXTRA_PROTOTYPES}
    lib = _lib.load()
    dp, vp = ctypes.POINTER(_lib.ViboDesc), ctypes.c_void_p
    assert lib.vibo_sign_rows_supported.argtypes == [dp] and lib.vibo_rows_sign_is_mask.argtypes == [dp, vp, vp, vp, vp]
    new = open(os.path.join(ROOT, 'include', 'vibo_hip_sign_rows.h')).read()
    assert re.search(r'#define\s+VIBO_MASK_SIGN\s+4\b', new)
    # vibo_hip.h itself: the lists tests/test_capi_symbols.py computes from it, 58 prototypes + vibo_train_step_sample_optional, no new constant
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'vibo_hip.h')).read(), flags=re.S)
    assert len(re.findall(r'\b(vibo_[a-z_0-9]+)\s*\(', src)) == 59 == len(_lib.EXPORTED_SYMBOLS)
    assert not set(_lib.SIGN_ROWS_SYMBOLS) & set(_lib.EXPORTED_SYMBOLS)
    header = dict(re.findall(r'\bVIBO_([A-Z0-9_]+)\s*=\s*(\d+)', src) + re.findall(r'#define\s+VIBO_([A-Z0-9_]+)\s+(\d+)', src))
    assert 'MASK_SIGN' not in header and len(header) == 33 + 2 + 3 + 6 + 1      # mirrored + the two dim limits + DECODER_ + KERNEL_ + S_RESERVED
    assert 'SIGN' not in src


# ---------------------------------------------------------------------------
# ops._sign_rows
# ---------------------------------------------------------------------------
SPEC = ops.ElboSpec(irt_model=2, ability_dim=8)


@pytest.fixture()
def fake(monkeypatch):
    """Fake backend entries: the shape is always supported; the verifier compares on the host and logs its calls."""
    log = {'supported': 0, 'verify': 0, 'capturing': 0}

    def supported(d):
        log['supported'] += 1
        assert d.mask_dtype == _lib.MASK_SIGN and d.mask_row_stride == 0
        return True

    def verify(response, mask):
        log['verify'] += 1
        return bool(((mask != 0) == ~torch.signbit(response)).all())

    monkeypatch.setitem(ops._BACKEND, 'sign_supported', supported)
    monkeypatch.setitem(ops._BACKEND, 'sign_verify', verify)
    monkeypatch.setattr(ops, 'SIGN_ROWS', True)
    return log


def decide(log, resp, mask, row_index=None, B=None, capturing=False, train_step=None, keep_int64=False):
    r, m, code = ops.prepare_rows(resp, mask, keep_int64=keep_int64)
    B = (r.shape[0] if row_index is None else int(row_index.numel())) if B is None else B

    def cap():
        log['capturing'] += 1
        return capturing
    got = ops._sign_rows(SPEC, r, m, code, row_index, B, _lib.REG_KL, True, train_step, capturing=cap)
    if got[1] == _lib.MASK_SIGN:
        assert got[0] is None
        return 'sign'
    assert got[0] is m and got[1] == code
    return 'mask'


def test_first_sighting_keeps_second_verifies_third_sends_sign(fake):
    resp, mask = matrix()
    assert decide(fake, resp, mask) == 'mask' and fake['verify'] == 0
    assert decide(fake, resp, mask) == 'mask' and fake['verify'] == 1          # verified eagerly; this launch still carries the mask
    for _ in range(3):
        assert decide(fake, resp, mask) == 'sign'
    assert fake['verify'] == 1 and resp._vibo_row_counts.sign_is_mask is True
    assert resp._vibo_row_counts.is_(resp, mask)


@pytest.mark.parametrize('edit', ['response', 'mask'])
def test_an_in_place_write_returns_to_the_mask_and_verifies_again(fake, edit):
    resp, mask = matrix()
    assert [decide(fake, resp, mask) for _ in range(4)] == ['mask', 'mask', 'sign', 'sign']
    if edit == 'response':
        resp[2, 1] = 1.0
        mask[2, 1] = True
        assert resp._vibo_row_counts.sign_is_mask is True                       # (the stale record: is_() is what throws it away)
    else:
        mask[2, 1] = False
        resp[2, 1] = 1.0
        resp[2, 1] = -1.0
    assert decide(fake, resp, mask) == 'mask' and fake['verify'] == 1
    assert decide(fake, resp, mask) == 'mask' and fake['verify'] == 2
    assert decide(fake, resp, mask) == 'sign' and fake['verify'] == 2


def test_an_edit_that_breaks_the_equivalence_is_seen(fake):
    resp, mask = matrix()
    assert [decide(fake, resp, mask) for _ in range(3)] == ['mask', 'mask', 'sign']
    resp[5, 5], mask[5, 5] = 1.0, False                                          # observed-looking value under a mask 0
    assert [decide(fake, resp, mask) for _ in range(3)] == ['mask', 'mask', 'mask'] and fake['verify'] == 2


def test_another_mask_on_the_same_response_does_not_inherit_the_fact(fake):
    resp, mask = matrix()
    assert [decide(fake, resp, mask) for _ in range(3)] == ['mask', 'mask', 'sign']
    other = mask.clone()
    other[0, 0] = not bool(other[0, 0])
    assert decide(fake, resp, other) == 'mask' and fake['verify'] == 1          # a first sighting of this pair
    assert decide(fake, resp, other) == 'mask' and fake['verify'] == 2          # verified: no
    assert decide(fake, resp, mask) == 'mask' and fake['verify'] == 2           # ONE record per response: the first pair starts over


def test_a_no_is_remembered(fake):
    resp, mask = matrix(consistent=False)
    assert [decide(fake, resp, mask) for _ in range(5)] == ['mask'] * 5
    assert fake['verify'] == 1 and resp._vibo_row_counts.sign_is_mask is False


def test_an_ineligible_call_never_verifies(fake):
    resp, mask = matrix()
    rows = torch.tensor([5, 1, 7])
    for _ in range(3):
        assert decide(fake, resp, mask, row_index=rows) == 'mask'               # gathered rows
        assert decide(fake, resp, mask, B=5) == 'mask'                          # fewer persons than the matrix has rows
        assert decide(fake, resp, mask.long(), keep_int64=True) == 'mask'       # an int64 mask handed over as it is
    assert fake == {'supported': 0, 'verify': 0, 'capturing': 0} and not hasattr(resp, '_vibo_row_counts')
    for _ in range(3):
        r, m, code = ops.prepare_rows(resp, None)
        assert ops._sign_rows(SPEC, r, m, code, None, r.shape[0], _lib.REG_KL, True, None, capturing=lambda: False) == (None, _lib.MASK_NONE)
    assert fake['verify'] == 0 and fake['supported'] == 0
    # cell codes: the library is handed (codes, codes, MASK_CODES)
    codes = torch.zeros(12, 8, dtype=torch.uint8)
    for _ in range(3):
        assert ops._sign_rows(SPEC, codes, codes, _lib.MASK_CODES, None, 12, _lib.REG_KL, True, None, capturing=lambda: False) == (codes, _lib.MASK_CODES)
    assert fake['verify'] == 0 and fake['supported'] == 0


def test_rows_the_matrix_kernel_cannot_load_never_leave_the_mask_path(fake):
    """The launch needs 16-byte aligned rows with a stride that is a multiple of 4 (a MASK_U8 call on other rows falls back to the
    tiled kernel and works; a MASK_SIGN call would be refused): such responses are not eligible -- nothing is asked, recorded or
    verified, however often they come back."""
    resp, mask = matrix()
    shifted = torch.empty(12 * 8 + 1)[1:].view(12, 8)                  # base 4 bytes past a 16-byte boundary
    shifted.copy_(resp)
    wide = torch.empty(12, 12)
    inner = wide[:, 1:9]                                                # stride 12, base off by 4 bytes
    inner.copy_(resp)
    odd = torch.empty(12, 10)[:, :8]                                    # I % 4 == 0, stride 10: chunkable, but not a multiple of 4
    odd.copy_(resp)
    for r in (shifted, inner, odd):
        assert r.data_ptr() % 16 != 0 or r.stride(0) % 4 != 0
        assert [decide(fake, r, mask) for _ in range(5)] == ['mask'] * 5
        assert not hasattr(r, '_vibo_row_counts')
    assert fake == {'supported': 0, 'verify': 0, 'capturing': 0}
    padded = torch.empty(12, 12)[:, :8]                                 # stride 12 at an aligned base: eligible
    padded.copy_(resp)
    assert padded.data_ptr() % 16 == 0 and [decide(fake, padded, mask) for _ in range(3)] == ['mask', 'mask', 'sign']


def test_an_unsupported_shape_is_not_looked_up(fake, monkeypatch):
    monkeypatch.setitem(ops._BACKEND, 'sign_supported', lambda d: False)
    resp, mask = matrix()
    assert [decide(fake, resp, mask) for _ in range(3)] == ['mask'] * 3
    assert fake['verify'] == 0 and not hasattr(resp, '_vibo_row_counts')


def test_bool_and_int64_masks_go_through_their_narrowed_form(fake):
    resp, mask = matrix()
    assert [decide(fake, resp, mask) for _ in range(3)] == ['mask', 'mask', 'sign']          # bool (shares bytes and version counter)
    resp2, mask2 = matrix(seed=1)
    m64 = mask2.long()
    assert [decide(fake, resp2, m64) for _ in range(3)] == ['mask', 'mask', 'sign']          # int64 narrowed once (prepare_mask)
    m64[1, 1] = 1 - m64[1, 1]
    assert decide(fake, resp2, m64) == 'mask'


def test_while_capturing(fake):
    """The two regimes of ops._lookup_counts: the plain launch on the whole matrix keeps the mask, the trainers' folded step uses a
    verified fact; neither verifies."""
    step = (torch.zeros(2, dtype=torch.int32), True)
    resp, mask = matrix()
    assert decide(fake, resp, mask, capturing=True) == 'mask'                               # first sighting
    assert decide(fake, resp, mask, capturing=True) == 'mask' and decide(fake, resp, mask, capturing=True, train_step=step) == 'mask'
    assert fake['verify'] == 0                                                               # a capture never verifies
    assert decide(fake, resp, mask) == 'mask' and fake['verify'] == 1                        # eager: verified
    assert decide(fake, resp, mask) == 'sign'
    assert decide(fake, resp, mask, capturing=True) == 'mask'                                # plain launch under capture
    assert decide(fake, resp, mask, capturing=True, train_step=step) == 'sign'               # the folded step under capture
    assert decide(fake, resp, mask, train_step=step) == 'sign' and fake['verify'] == 1
    bad_r, bad_m = matrix(consistent=False)
    assert [decide(fake, bad_r, bad_m, train_step=step) for _ in range(2)] == ['mask', 'mask']
    assert decide(fake, bad_r, bad_m, capturing=True, train_step=step) == 'mask' and fake['verify'] == 2


def test_the_switch_turns_all_of_it_off(fake, monkeypatch):
    monkeypatch.setattr(ops, 'SIGN_ROWS', False)
    resp, mask = matrix()
    assert [decide(fake, resp, mask) for _ in range(4)] == ['mask'] * 4
    assert fake == {'supported': 0, 'verify': 0, 'capturing': 0} and not hasattr(resp, '_vibo_row_counts')


def test_the_record_is_the_row_counts_record(fake):
    """One record per response tensor: the fact sits beside the whole-row counts and goes with them."""
    resp, mask = matrix()
    assert [decide(fake, resp, mask) for _ in range(3)] == ['mask', 'mask', 'sign']
    rec = resp._vibo_row_counts
    assert isinstance(rec, ops.ResidentMatrix) and 'sign_is_mask' in ops.ResidentMatrix.__slots__
    assert ops.ResidentMatrix(resp, mask).sign_is_mask is None
