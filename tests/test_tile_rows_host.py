"""Tile rows (include/vibo_hip_tile_rows.h, VIBO_MASK_TILES) without a GPU: what the library's validation answers for the format,
that the new header is bound while vibo_hip.h keeps its lists, and ops._tile_rows -- the one place that decides whether an ELBO
launch goes out on a resident matrix' image -- driven with fake backend entries and a fake capturing()."""
import ctypes
import os
import re

import pytest
import torch

import tile_rows_common as T
from conftest import ROOT
from row_format_common import _null_call, desc as sign_desc, matrix
from vibo_amd import _lib, ops

TILE_ENTRY_POINTS = {'vibo_elbo_fwd_bwd', 'vibo_elbo_fwd_bwd_step', 'vibo_elbo_fwd_bwd_step_noise', 'vibo_workspace_bytes',
                     'vibo_plan_kernel', 'vibo_train_step_supported', 'vibo_train_step_draws_noise', 'vibo_train_step_sample_optional'}


def desc(**kw):
    return sign_desc(**{'mask': _lib.MASK_TILES, **kw})


# ---------------------------------------------------------------------------
# the library's validation
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('I,ok', [(4, True), (130, True), (896, True), (897, True), (1000, True), (1024, True), (1025, False), (3, False)])
@pytest.mark.parametrize('B', [1, 33, 1_000_000])
def test_supported_and_bytes_over_shapes(I, ok, B):
    lib = _lib.load()
    d = desc(B=B, I=I, flags=_lib.FLAG_KERNEL_MATRIX, stride=0)             # (the row strides of the descriptor are not read)
    assert lib.vibo_tile_rows_supported(ctypes.byref(d)) == (1 if ok else 0)
    assert lib.vibo_tile_rows_bytes(ctypes.byref(d)) == (T.image_bytes(B, I) if ok else 0)
    plan = lib.vibo_plan_kernel(ctypes.byref(d))
    if ok:
        assert plan == 1 and lib.vibo_workspace_bytes(ctypes.byref(d)) > 0
    else:
        assert plan == -8 and b'VIBO_MASK_TILES' in lib.vibo_last_error_string() and lib.vibo_workspace_bytes(ctypes.byref(d)) == 0


GRID = {'headline': {}, 'ability_dim 1': dict(A=1), '3PL forward only': dict(irt=3, grad=0), '132 items pinned': dict(B=500, I=132, flags=_lib.FLAG_KERNEL_MATRIX),
        'conditional': dict(posterior=_lib.POSTERIOR_CONDITIONAL), 'flows': dict(n_flows=2), '2000 items': dict(I=2000),
        'VALU pinned': dict(flags=_lib.FLAG_KERNEL_VALU), '16 persons': dict(B=16), 'narrow rows': dict(I=96, A=1),
        'caller-supplied posterior': dict(posterior=_lib.POSTERIOR_GIVEN)}
SUPPORTED = {'headline', 'ability_dim 1', '3PL forward only', '132 items pinned'}


@pytest.mark.parametrize('case', sorted(GRID))
def test_supported_query_plan_and_step_queries(case):
    lib = _lib.load()
    d = desc(**GRID[case])
    ok = case in SUPPORTED
    assert lib.vibo_tile_rows_supported(ctypes.byref(d)) == (1 if ok else 0)
    assert (lib.vibo_tile_rows_bytes(ctypes.byref(d)) > 0) == ok
    plan = lib.vibo_plan_kernel(ctypes.byref(d))
    if ok:
        assert plan == 1 and _lib.KERNEL_NAMES[plan].startswith('matrix')
    else:
        assert plan == -8 and b'VIBO_MASK_TILES' in lib.vibo_last_error_string() and lib.vibo_workspace_bytes(ctypes.byref(d)) == 0
    # the three step queries and the workspace: what they answer for the same descriptor with a u8 mask
    u8 = desc(**{**GRID[case], 'mask': _lib.MASK_U8})
    for fn in (lib.vibo_train_step_supported, lib.vibo_train_step_draws_noise):
        assert fn(ctypes.byref(d)) == fn(ctypes.byref(u8)), fn
    assert lib.vibo_train_step_sample_optional(ctypes.byref(d), 0) == lib.vibo_train_step_sample_optional(ctypes.byref(u8), 0)
    assert lib.vibo_workspace_bytes(ctypes.byref(d)) == (lib.vibo_workspace_bytes(ctypes.byref(u8)) if ok else 0)


def test_queries_want_the_format_itself():
    lib = _lib.load()
    for other in (_lib.MASK_U8, _lib.MASK_SIGN, _lib.MASK_CODES):
        assert lib.vibo_tile_rows_supported(ctypes.byref(desc(mask=other))) == 0 and lib.vibo_tile_rows_bytes(ctypes.byref(desc(mask=other))) == 0
    assert lib.vibo_tile_rows_supported(None) == 0 and lib.vibo_tile_rows_bytes(None) == 0
    assert lib.vibo_plan_kernel(ctypes.byref(desc(mask=5))) == -3 and lib.vibo_plan_kernel(ctypes.byref(desc(mask=7))) == -3
    # gathered rows: refused by the launch itself, before anything runs
    assert lib.vibo_elbo_fwd_bwd(ctypes.byref(desc()), None, None, ctypes.c_void_p(64), *([None] * 14), 0, None) == -8
    assert b'row_index' in lib.vibo_last_error_string() and b'VIBO_MASK_TILES' in lib.vibo_last_error_string()


def test_every_other_export_refuses_the_format_before_any_launch():
    """Every export of vibo_hip.h that takes a descriptor, with a VIBO_MASK_TILES descriptor of the headline shape and NULL pointers: the
    entry points of the format get past the descriptor (-5: the NULL pointers), all others answer -8 -- size queries 0, the one
    offset query -1 -- from validation (nothing can launch on NULL pointers, and there is no GPU here)."""
    lib = _lib.load()
    d = desc()
    dp = ctypes.POINTER(_lib.ViboDesc)
    seen = 0
    for name, restype, argtypes in _lib.PROTOTYPES + [p for p in _lib.EXTRA_PROTOTYPES if p[0] in _lib.SIGN_ROWS_SYMBOLS]:
        if not argtypes or argtypes[0] is not dp:
            continue
        seen += 1
        rc = _null_call(getattr(lib, name), d)
        if name in TILE_ENTRY_POINTS:
            if name.startswith('vibo_elbo'):
                assert rc == -5, (name, rc)
            continue
        if restype is ctypes.c_size_t or name in ('vibo_ctrain_param_floats', 'vibo_ctrain_scratch_floats', 'vibo_dtrain_param_floats',
                                                  'vibo_dtrain_scratch_floats', 'vibo_mtrain_param_floats', 'vibo_mean_encoder_partials',
                                                  'vibo_sign_rows_supported'):
            assert rc == 0, (name, rc)
        elif name == 'vibo_dtrain_scratch_offset':
            assert rc == -1, (name, rc)
        else:
            assert rc == -8, (name, rc)
    assert seen >= 40
    # the builder: a tile image is no source format; NULL pointers; any other source format
    assert lib.vibo_tile_rows_build(ctypes.byref(d), None, None, None, 0, None) == -8
    assert lib.vibo_tile_rows_build(ctypes.byref(desc(mask=_lib.MASK_I64)), None, None, None, 0, None) == -8
    for src in (_lib.MASK_U8, _lib.MASK_NONE, _lib.MASK_SIGN, _lib.MASK_CODES):
        assert lib.vibo_tile_rows_build(ctypes.byref(desc(mask=src)), None, None, None, 0, None) == -5
    assert lib.vibo_tile_rows_build(ctypes.byref(desc(mask=_lib.MASK_U8, I=1025)), None, None, None, 0, None) == -8
    assert lib.vibo_tile_rows_build(None, None, None, None, 0, None) == -1


def test_new_header_is_bound_and_the_main_header_keeps_its_lists():
    assert 'vibo_hip_tile_rows.h' in _lib.EXTRA_HEADERS and _lib.MASK_TILES == 6 and _lib.TILE_WAVE_BLOCK_BYTES == T.WAVE_BLOCK
    assert _lib.TILE_ROWS_SYMBOLS == ('vibo_tile_rows_supported', 'vibo_tile_rows_bytes', 'vibo_tile_rows_build')
    assert set(_lib.TILE_ROWS_SYMBOLS) <= {name for name, _, _ in _lib.EXTRA_PROTOTYPES}
    assert _lib.SIGN_ROWS_SYMBOLS == ('vibo_sign_rows_supported', 'vibo_rows_sign_is_mask')
    lib = _lib.load()
    dp, vp = ctypes.POINTER(_lib.ViboDesc), ctypes.c_void_p
    assert lib.vibo_tile_rows_supported.argtypes == [dp] and lib.vibo_tile_rows_bytes.argtypes == [dp]
    assert lib.vibo_tile_rows_bytes.restype is ctypes.c_size_t
    assert lib.vibo_tile_rows_build.argtypes == [dp, vp, vp, vp, ctypes.c_size_t, vp]
    new = open(os.path.join(ROOT, 'include', 'vibo_hip_tile_rows.h')).read()
    assert re.search(r'#define\s+VIBO_MASK_TILES\s+6\b', new)
    # vibo_hip.h itself: 59 prototypes, 33 mirrored constants, no word of the new format; ABI version unchanged
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'vibo_hip.h')).read(), flags=re.S)
    assert len(re.findall(r'\b(vibo_[a-z_0-9]+)\s*\(', src)) == 59 == len(_lib.EXPORTED_SYMBOLS)
    assert not set(_lib.TILE_ROWS_SYMBOLS) & set(_lib.EXPORTED_SYMBOLS)
    header = dict(re.findall(r'\bVIBO_([A-Z0-9_]+)\s*=\s*(\d+)', src) + re.findall(r'#define\s+VIBO_([A-Z0-9_]+)\s+(\d+)', src))
    assert 'MASK_TILES' not in header and len(header) == 33 + 2 + 3 + 6 + 1
    assert 'TILES' not in src and lib.vibo_version() == _lib.ABI_VERSION == 2


# ---------------------------------------------------------------------------
# ops._tile_rows
# ---------------------------------------------------------------------------
SPEC = ops.ElboSpec(irt_model=2, ability_dim=8)


@pytest.fixture()
def fake(monkeypatch):
    """Fake backend entries: the shape is always supported, plenty of memory, the 'image' is a host tensor; every call is logged."""
    log = {'supported': 0, 'bytes': 0, 'free': 0, 'build': 0, 'capturing': 0, 'sign': 0}
    state = {'free': 1 << 40, 'oom': False}

    def supported(d):
        log['supported'] += 1
        assert d.mask_dtype == _lib.MASK_TILES
        return True

    def nbytes(d):
        log['bytes'] += 1
        return T.image_bytes(d.num_person, d.num_item)

    def free(device):
        log['free'] += 1
        return state['free']

    def build(spec, response, mask, mask_code, num_person, reg_mode, want_grad, need):
        log['build'] += 1
        if state['oom']:
            raise torch.cuda.OutOfMemoryError('fake')
        assert need == T.image_bytes(num_person, response.shape[1])
        return torch.zeros(need, dtype=torch.uint8)

    def sign_supported(d):
        log['sign'] += 1
        return True
    for key, fn in (('tile_supported', supported), ('tile_bytes', nbytes), ('tile_free', free), ('tile_build', build),
                    ('sign_supported', sign_supported), ('sign_verify', lambda r, m: True)):
        monkeypatch.setitem(ops._BACKEND, key, fn)
    monkeypatch.setattr(ops, 'TILE_ROWS', True)
    monkeypatch.setattr(ops, 'SIGN_ROWS', True)
    monkeypatch.setattr(ops, 'TILE_ROWS_MIN_PERSONS', 8)
    monkeypatch.setattr(ops, 'TILE_ROWS_PLAIN_LAUNCHES', True)          # (the decision itself: plain launches included)
    log['state'] = state
    return log


def decide(log, resp, mask, row_index=None, B=None, capturing=False, train_step=None):
    """'tiles' / 'rows' (the caller's rows, _sign_rows not asked) / 'sign rows decide' (None: the call is _sign_rows')."""
    r, m, code = ops.prepare_rows(resp, mask)
    B = (r.shape[0] if row_index is None else int(row_index.numel())) if B is None else B

    def cap():
        log['capturing'] += 1
        return capturing
    got = ops._tile_rows(SPEC, r, m, code, row_index, B, _lib.REG_KL, True, train_step, capturing=cap)
    if got is None:
        return 'sign rows decide'
    if got is False:
        return 'rows'
    assert got is r._vibo_row_counts.tiles and got.dtype == torch.uint8
    return 'tiles'


def test_first_sighting_records_second_builds_third_uses(fake):
    resp, mask = matrix()
    assert decide(fake, resp, mask) == 'rows' and fake['build'] == 0
    assert decide(fake, resp, mask) == 'rows' and fake['build'] == 1           # built eagerly; this launch still reads the rows
    for _ in range(3):
        assert decide(fake, resp, mask) == 'tiles'
    assert fake['build'] == 1 and resp._vibo_row_counts.is_(resp, mask)
    assert resp._vibo_row_counts.sign_is_mask is None                          # a matrix with an image is never sign-verified


@pytest.mark.parametrize('edit', ['response', 'mask'])
def test_an_in_place_write_starts_over(fake, edit):
    resp, mask = matrix()
    assert [decide(fake, resp, mask) for _ in range(4)] == ['rows', 'rows', 'tiles', 'tiles']
    old = resp._vibo_row_counts
    if edit == 'response':
        resp[2, 1] = 1.0
    else:
        mask[2, 1] = not bool(mask[2, 1])
    assert old.tiles is not None                                                # (the stale record: is_() is what throws it away)
    assert [decide(fake, resp, mask) for _ in range(3)] == ['rows', 'rows', 'tiles'] and fake['build'] == 2
    assert resp._vibo_row_counts is not old


def test_another_mask_on_the_same_response_does_not_inherit_the_image(fake):
    resp, mask = matrix()
    assert [decide(fake, resp, mask) for _ in range(3)] == ['rows', 'rows', 'tiles']
    other = mask.clone()
    other[0, 0] = not bool(other[0, 0])
    assert decide(fake, resp, other) == 'rows' and fake['build'] == 1           # a first sighting of this pair
    assert decide(fake, resp, other) == 'rows' and fake['build'] == 2
    assert decide(fake, resp, other) == 'tiles'
    assert decide(fake, resp, mask) == 'rows' and fake['build'] == 2            # ONE record per response: the first pair starts over


def test_while_capturing(fake):
    """The two regimes of ops._lookup_counts / _sign_rows: the plain launch on the whole matrix keeps the caller's rows, the
    trainers' folded step uses the image; neither builds."""
    step = (torch.zeros(2, dtype=torch.int32), True)
    resp, mask = matrix()
    assert decide(fake, resp, mask, capturing=True) == 'rows'                                # first sighting
    assert decide(fake, resp, mask, capturing=True) == 'rows' and decide(fake, resp, mask, capturing=True, train_step=step) == 'rows'
    assert fake['build'] == 0                                                                # a capture never builds
    assert decide(fake, resp, mask) == 'rows' and fake['build'] == 1                         # eager: built
    assert decide(fake, resp, mask) == 'tiles'
    assert decide(fake, resp, mask, capturing=True) == 'rows'                                # plain launch under capture
    assert decide(fake, resp, mask, capturing=True, train_step=step) == 'tiles'              # the folded step under capture
    assert decide(fake, resp, mask, train_step=step) == 'tiles' and fake['build'] == 1


def test_the_switch_turns_all_of_it_off(fake, monkeypatch):
    monkeypatch.setattr(ops, 'TILE_ROWS', False)
    resp, mask = matrix()
    assert [decide(fake, resp, mask) for _ in range(4)] == ['sign rows decide'] * 4
    assert fake['supported'] == fake['build'] == fake['capturing'] == 0 and not hasattr(resp, '_vibo_row_counts')


def test_plain_launches_are_left_alone_by_default(fake, monkeypatch):
    """ops.TILE_ROWS_PLAIN_LAUNCHES off (the default): a launch without train_step is _sign_rows' and is no sighting; the trainers'
    folded step records, builds and uses -- and a plain launch in between still reads the rows."""
    monkeypatch.setattr(ops, 'TILE_ROWS_PLAIN_LAUNCHES', False)
    step = (torch.zeros(2, dtype=torch.int32), True)
    resp, mask = matrix()
    assert [decide(fake, resp, mask) for _ in range(4)] == ['sign rows decide'] * 4
    assert fake['supported'] == fake['build'] == 0 and not hasattr(resp, '_vibo_row_counts')
    assert [decide(fake, resp, mask, train_step=step) for _ in range(3)] == ['rows', 'rows', 'tiles']
    assert decide(fake, resp, mask) == 'sign rows decide' and decide(fake, resp, mask, capturing=True) == 'sign rows decide'
    assert decide(fake, resp, mask, train_step=step, capturing=True) == 'tiles' and fake['build'] == 1


def test_the_size_threshold(fake, monkeypatch):
    assert ops.TILE_ROWS_MIN_PERSONS == 8                                       # (the fixture's; the module's own is checked below)
    resp, mask = matrix(P=7)
    assert [decide(fake, resp, mask) for _ in range(4)] == ['sign rows decide'] * 4
    assert fake['supported'] == fake['build'] == 0 and not hasattr(resp, '_vibo_row_counts')
    resp, mask = matrix(P=8)
    assert [decide(fake, resp, mask) for _ in range(3)] == ['rows', 'rows', 'tiles']
    monkeypatch.undo()
    assert ops.TILE_ROWS_MIN_PERSONS == 16384 and ops.TILE_ROWS is True and ops.TILE_ROWS_PLAIN_LAUNCHES is False


def test_below_the_threshold_sign_rows_is_reached_unchanged(fake, monkeypatch):
    """The launch's order of the two decisions (ops._launch_rows), with both faked: a small matrix goes U8, U8, SIGN as before this format."""
    resp, mask = matrix(P=7)
    r, m, code = ops.prepare_rows(resp, mask)
    sent = [ops._launch_rows(SPEC, r, m, code, None, 7, _lib.REG_KL, True, None, capturing=lambda: False, stream=None).mask_code for _ in range(4)]
    assert sent == [_lib.MASK_U8, _lib.MASK_U8, _lib.MASK_SIGN, _lib.MASK_SIGN] and fake['build'] == 0
    assert fake['supported'] == 0 and r._vibo_row_counts.tiles is None         # (no image for these calls: never asked for, never decided)


@pytest.mark.parametrize('why', ['half of the free memory', 'the allocator'])
def test_the_memory_guard_and_a_remembered_no(fake, why):
    resp, mask = matrix()
    if why == 'half of the free memory':
        fake['state']['free'] = 2 * T.image_bytes(12, 8) - 1
    else:
        fake['state']['oom'] = True
    assert decide(fake, resp, mask) == 'rows'
    assert decide(fake, resp, mask) == 'sign rows decide'                       # no image: this launch is _sign_rows' already
    builds = fake['build']
    assert builds == (0 if why == 'half of the free memory' else 1)
    fake['state'].update(free=1 << 40, oom=False)                               # (memory comes back: the "no" stays)
    assert [decide(fake, resp, mask) for _ in range(3)] == ['sign rows decide'] * 3
    assert fake['build'] == builds and fake['free'] == 1 and resp._vibo_row_counts.tiles is False
    # exactly half is enough
    resp2, mask2 = matrix(seed=1)
    fake['state']['free'] = 2 * T.image_bytes(12, 8)
    assert [decide(fake, resp2, mask2) for _ in range(3)] == ['rows', 'rows', 'tiles']


def test_cell_codes_and_rows_without_a_mask(fake):
    resp, mask = matrix()
    codes = ops.CellCodes(torch.where(mask, resp.to(torch.uint8), torch.tensor(2, dtype=torch.uint8)))
    assert [decide(fake, codes, None) for _ in range(3)] == ['rows', 'rows', 'tiles']
    assert codes.codes._vibo_row_counts.has_mask is False                       # (known by the codes alone)
    codes.codes[1, 1] = 2
    assert [decide(fake, codes, None) for _ in range(3)] == ['rows', 'rows', 'tiles'] and fake['build'] == 2
    plain = (resp > 0).float()
    assert [decide(fake, plain, None) for _ in range(3)] == ['rows', 'rows', 'tiles']


def test_an_ineligible_call_is_never_looked_up(fake, monkeypatch):
    resp, mask = matrix()
    rows = torch.tensor([5, 1, 7, 2, 3, 4, 6, 8])
    for _ in range(3):
        assert decide(fake, resp, mask, row_index=rows) == 'sign rows decide'   # gathered rows
        assert decide(fake, resp, mask, B=9) == 'sign rows decide'              # fewer persons than the matrix has rows
    assert fake['supported'] == fake['build'] == 0 and not hasattr(resp, '_vibo_row_counts')
    # rows the matrix kernel cannot load as they are (the launch on them runs the tiled kernel, whose last bits are its own)
    shifted = torch.empty(12 * 8 + 1)[1:].view(12, 8)
    shifted.copy_(resp)
    odd = torch.empty(12, 10)[:, :8]
    odd.copy_(resp)
    ragged, ragged_mask = matrix(I=6)                                           # 6 items in a stride of 6: no whole chunks
    for r, m in ((shifted, mask), (odd, mask), (ragged, ragged_mask)):
        assert [decide(fake, r, m) for _ in range(3)] == ['sign rows decide'] * 3 and not hasattr(r, '_vibo_row_counts')
    assert fake['supported'] == 0
    # an unsupported shape
    monkeypatch.setitem(ops._BACKEND, 'tile_supported', lambda d: False)
    assert [decide(fake, resp, mask) for _ in range(3)] == ['sign rows decide'] * 3 and not hasattr(resp, '_vibo_row_counts')


def test_the_record_is_the_row_counts_record(fake):
    resp, mask = matrix()
    assert [decide(fake, resp, mask) for _ in range(3)] == ['rows', 'rows', 'tiles']
    rec = resp._vibo_row_counts
    assert isinstance(rec, ops.ResidentMatrix) and 'tiles' in ops.ResidentMatrix.__slots__
    assert ops.ResidentMatrix(resp, mask).tiles is None
