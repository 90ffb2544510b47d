"""Tile rows under a caller-supplied posterior (include/vibo_hip_given_tiles.h: VIBO_MASK_TILES with VIBO_POSTERIOR_GIVEN) without a
GPU: the header is bound and the older headers keep their lists, what the two queries and the entry point's validation answer, that
the older exports still refuse the combination, and ops._tile_rows with a given spec -- driven with fake backend entries and a fake
capturing(), as tests/test_tile_rows_host.py drives it for the plain model."""
import ctypes
import os
import re

import pytest
import torch

import tile_rows_common as T
from conftest import ROOT
from row_format_common import desc as sign_desc, matrix
from vibo_amd import _lib, ops

GIVEN, MATRIX = _lib.POSTERIOR_GIVEN, _lib.FLAG_KERNEL_MATRIX
ENTRY_ARGS = 19        # vibo_elbo_fwd_bwd's arguments behind the descriptor: 17 pointers, workspace_bytes, stream


def desc(**kw):
    return sign_desc(**{'mask': _lib.MASK_TILES, 'posterior': GIVEN, 'flags': MATRIX, **kw})


def entry(d, *, response=None, row_index=None):
    """vibo_elbo_fwd_bwd_given_tiles on (fake) host addresses: validation answers before anything could launch."""
    args = [response, None, row_index] + [None] * 14 + [0, None]
    assert len(args) == ENTRY_ARGS
    return _lib.load().vibo_elbo_fwd_bwd_given_tiles(ctypes.byref(d), *args)


# ---------------------------------------------------------------------------
# the header and the binding
# ---------------------------------------------------------------------------
def test_header_is_bound_and_the_older_headers_keep_their_lists():
    assert 'vibo_hip_given_tiles.h' in _lib.EXTRA_HEADERS
    assert _lib.GIVEN_TILES_SYMBOLS == ('vibo_given_tile_rows_supported', 'vibo_given_tiles_workspace_bytes', 'vibo_elbo_fwd_bwd_given_tiles')
    assert set(_lib.GIVEN_TILES_SYMBOLS) <= {name for name, _, _ in _lib.EXTRA_PROTOTYPES}
    lib = _lib.load()
    dp, vp = ctypes.POINTER(_lib.ViboDesc), ctypes.c_void_p
    assert lib.vibo_given_tile_rows_supported.argtypes == [dp] and lib.vibo_given_tile_rows_supported.restype is ctypes.c_int
    assert lib.vibo_given_tiles_workspace_bytes.argtypes == [dp] and lib.vibo_given_tiles_workspace_bytes.restype is ctypes.c_size_t
    # the argument list of vibo_elbo_fwd_bwd: ops._hip_launch_elbo shares the call
    assert lib.vibo_elbo_fwd_bwd_given_tiles.argtypes == lib.vibo_elbo_fwd_bwd.argtypes == [dp] + [vp] * 17 + [ctypes.c_size_t, vp]
    # vibo_hip.h and vibo_hip_tile_rows.h: their export lists as they were
    main = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'vibo_hip.h')).read(), flags=re.S)
    assert len(re.findall(r'\b(vibo_[a-z_0-9]+)\s*\(', main)) == 59 == len(_lib.EXPORTED_SYMBOLS)
    assert 'given_tile' not in main and 'TILES' not in main and lib.vibo_version() == _lib.ABI_VERSION == 2
    assert _lib.TILE_ROWS_SYMBOLS == ('vibo_tile_rows_supported', 'vibo_tile_rows_bytes', 'vibo_tile_rows_build')
    assert not set(_lib.GIVEN_TILES_SYMBOLS) & (set(_lib.EXPORTED_SYMBOLS) | set(_lib.TILE_ROWS_SYMBOLS) | set(_lib.SIGN_ROWS_SYMBOLS))
    assert 'GIVEN_TILES_SYMBOLS' in open(os.path.join(ROOT, '__graft_entry__.py')).read()      # (build() asks the library for them too)


# ---------------------------------------------------------------------------
# the two queries
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('A', [1, 8])
@pytest.mark.parametrize('I,ok', [(4, True), (130, True), (896, True), (897, True), (1000, True), (1024, True), (3, False), (1025, False)])
def test_supported_and_workspace_over_shapes(I, ok, A):
    lib = _lib.load()
    for B in (33, 1_000_000):
        d = desc(B=B, I=I, A=A, stride=0)                                      # (the row strides of the descriptor are not read)
        assert lib.vibo_given_tile_rows_supported(ctypes.byref(d)) == (1 if ok else 0)
        u8 = desc(B=B, I=I, A=A, mask=_lib.MASK_U8)
        want = lib.vibo_workspace_bytes(ctypes.byref(u8))
        if ok:
            assert want > 0
        assert lib.vibo_given_tiles_workspace_bytes(ctypes.byref(d)) == (want if ok else 0)


REFUSED = {'flows': dict(n_flows=2), 'unconditional posterior': dict(posterior=_lib.POSTERIOR_UNCONDITIONAL),
           'conditional posterior': dict(posterior=_lib.POSTERIOR_CONDITIONAL), 'u8 mask': dict(mask=_lib.MASK_U8),
           'sign rows': dict(mask=_lib.MASK_SIGN), 'cell codes': dict(mask=_lib.MASK_CODES), 'no mask': dict(mask=_lib.MASK_NONE),
           'VALU pinned': dict(flags=_lib.FLAG_KERNEL_VALU), '16 persons by the thresholds': dict(B=16, flags=0),
           'ability_dim 9': dict(A=9), '2000 items': dict(I=2000)}


@pytest.mark.parametrize('case', sorted(REFUSED))
def test_refused_descriptors(case):
    lib = _lib.load()
    d = desc(**REFUSED[case])
    assert lib.vibo_given_tile_rows_supported(ctypes.byref(d)) == 0
    assert lib.vibo_given_tiles_workspace_bytes(ctypes.byref(d)) == 0
    rc = entry(d)
    assert rc == -8, (case, rc, lib.vibo_last_error_string())
    assert lib.vibo_last_error_string()


def test_null_descriptor_and_the_thresholds():
    lib = _lib.load()
    assert lib.vibo_given_tile_rows_supported(None) == 0 and lib.vibo_given_tiles_workspace_bytes(None) == 0
    assert lib.vibo_elbo_fwd_bwd_given_tiles(None, *([None] * 17), 0, None) == -1
    # without the pin the planner's thresholds decide the engine: the headline shape is the matrix kernel's
    assert lib.vibo_given_tile_rows_supported(ctypes.byref(desc(flags=0))) == 1
    assert lib.vibo_given_tile_rows_supported(ctypes.byref(desc(flags=0, A=1))) == 1
    assert lib.vibo_given_tile_rows_supported(ctypes.byref(desc(flags=0, B=1000))) == 0


# ---------------------------------------------------------------------------
# the entry point's validation
# ---------------------------------------------------------------------------
def test_entry_point_validation():
    lib = _lib.load()
    for kw in ({}, dict(A=1, irt=3), dict(I=130, B=500), dict(grad=0)):
        d = desc(**kw)
        assert lib.vibo_given_tile_rows_supported(ctypes.byref(d)) == 1
        assert entry(d) == -5, kw                                               # NULL required pointers, before anything launches
        assert entry(d, response=ctypes.c_void_p(4096)) == -5
        assert entry(d, row_index=ctypes.c_void_p(64)) == -8 and b'row_index' in lib.vibo_last_error_string()
        assert entry(d, response=ctypes.c_void_p(4096), row_index=ctypes.c_void_p(64)) == -8 and b'row_index' in lib.vibo_last_error_string()
    # a mask, or a flow argument: pointers that must be NULL
    d = desc()
    args = [None] * 17
    args[1] = ctypes.c_void_p(64)
    assert lib.vibo_elbo_fwd_bwd_given_tiles(ctypes.byref(d), *args, 0, None) == -5 and b'must be NULL' in lib.vibo_last_error_string()
    args = [None] * 17
    args[6] = ctypes.c_void_p(64)
    assert lib.vibo_elbo_fwd_bwd_given_tiles(ctypes.byref(d), *args, 0, None) == -5 and b'must be NULL' in lib.vibo_last_error_string()


def test_the_older_exports_still_refuse_the_combination():
    lib = _lib.load()
    for kw in ({}, dict(flags=0), dict(A=1)):
        d = desc(**kw)
        assert lib.vibo_tile_rows_supported(ctypes.byref(d)) == 0 and lib.vibo_tile_rows_bytes(ctypes.byref(d)) == 0
        assert lib.vibo_workspace_bytes(ctypes.byref(d)) == 0
        assert lib.vibo_plan_kernel(ctypes.byref(d)) == -8 and b'VIBO_MASK_TILES' in lib.vibo_last_error_string()
        assert lib.vibo_elbo_fwd_bwd(ctypes.byref(d), *([None] * 17), 0, None) == -8
        assert lib.vibo_elbo_fwd_bwd_step(ctypes.byref(d), None, 0, *([None] * 13), 0, None) == -5      # (its NULL step_count comes first)
        assert lib.vibo_elbo_fwd_bwd_step(ctypes.byref(d), ctypes.c_void_p(64), 0, *([None] * 13), 0, None) == -8
        assert lib.vibo_tile_rows_build(ctypes.byref(d), None, None, None, 0, None) == -8
    # ... and the new entry point takes no plain tile descriptor
    plain = desc(posterior=_lib.POSTERIOR_UNCONDITIONAL)
    assert lib.vibo_tile_rows_supported(ctypes.byref(plain)) == 1 and entry(plain) == -8


# ---------------------------------------------------------------------------
# ops._tile_rows with a given spec
# ---------------------------------------------------------------------------
GIVEN_SPEC = ops.ElboSpec(irt_model=2, ability_dim=8, given=True)
PLAIN_SPEC = ops.ElboSpec(irt_model=2, ability_dim=8)


@pytest.fixture()
def fake(monkeypatch):
    """Fake backend entries (the fixture of tests/test_tile_rows_host.py, with the new query): every shape is supported, plenty of
    memory, the 'image' is a host tensor; every call is logged, the build with the spec and the descriptor flags it was asked under."""
    log = {'supported': 0, 'given_supported': 0, 'bytes': 0, 'free': 0, 'build': [], 'capturing': 0}

    def supported(d):
        log['supported'] += 1
        assert d.mask_dtype == _lib.MASK_TILES and d.posterior == _lib.POSTERIOR_UNCONDITIONAL
        return True

    def given_supported(d):
        log['given_supported'] += 1
        assert d.mask_dtype == _lib.MASK_TILES and d.posterior == GIVEN
        return True

    def nbytes(d):
        log['bytes'] += 1
        assert d.mask_dtype == _lib.MASK_TILES and d.posterior == _lib.POSTERIOR_UNCONDITIONAL      # (the builder's descriptor: the plain twin)
        log['bytes_flags'] = d.flags
        return T.image_bytes(d.num_person, d.num_item)

    def free(device):
        log['free'] += 1
        return 1 << 40

    def build(spec, response, mask, mask_code, num_person, reg_mode, want_grad, need):
        log['build'].append((spec, ops.DESC_FLAGS))
        assert need == T.image_bytes(num_person, response.shape[1])
        return torch.zeros(need, dtype=torch.uint8)
    for key, fn in (('tile_supported', supported), ('tile_given_supported', given_supported), ('tile_bytes', nbytes), ('tile_free', free),
                    ('tile_build', build)):
        monkeypatch.setitem(ops._BACKEND, key, fn)
    monkeypatch.setattr(ops, 'TILE_ROWS', True)
    monkeypatch.setattr(ops, 'TILE_ROWS_GIVEN', True)
    monkeypatch.setattr(ops, 'TILE_ROWS_GIVEN_MIN_PERSONS', 0)
    monkeypatch.setattr(ops, 'TILE_ROWS_MIN_PERSONS', 8)
    monkeypatch.setattr(ops, 'TILE_ROWS_PLAIN_LAUNCHES', False)
    return log


def decide(log, resp, mask, spec=GIVEN_SPEC, row_index=None, B=None, capturing=False, train_step=None, **kw):
    """'tiles' / 'rows' (the caller's rows, on the way to an image or under capture) / None (no image for this call)."""
    r, m, code = ops.prepare_rows(resp, mask)
    B = (r.shape[0] if row_index is None else int(row_index.numel())) if B is None else B

    def cap():
        log['capturing'] += 1
        return capturing
    got = ops._tile_rows(spec, r, m, code, row_index, B, _lib.REG_KL, True, train_step, capturing=cap, **kw)
    if got is None or got is False:
        return None if got is None else 'rows'
    assert got is r._vibo_row_counts.tiles and got.dtype == torch.uint8
    return 'tiles'


def test_the_keyword_is_keyword_only_and_defaults_to_off():
    import inspect
    for fn in (ops._tile_rows, ops._hip_launch_elbo):
        par = inspect.signature(fn).parameters['resident_step']
        assert par.kind is inspect.Parameter.KEYWORD_ONLY and par.default is False
    assert 'tile_given_supported' in ops._BACKEND and ops._BACKEND['tile_given_supported'] is ops._hip_given_tile_rows_supported
    assert isinstance(ops.TILE_ROWS_GIVEN, bool)


def test_without_resident_step_nothing_is_looked_up(fake):
    resp, mask = matrix()
    assert [decide(fake, resp, mask) for _ in range(4)] == [None] * 4
    assert [decide(fake, resp, mask, resident_step=False, capturing=True) for _ in range(2)] == [None] * 2
    assert fake['given_supported'] == fake['supported'] == fake['bytes'] == fake['capturing'] == 0 and not fake['build']
    assert not hasattr(resp, '_vibo_row_counts')


def test_resident_step_records_builds_uses(fake):
    resp, mask = matrix()
    assert decide(fake, resp, mask, resident_step=True) == 'rows' and not fake['build']
    assert decide(fake, resp, mask, resident_step=True) == 'rows' and len(fake['build']) == 1      # built; this launch still reads the rows
    for _ in range(3):
        assert decide(fake, resp, mask, resident_step=True) == 'tiles'
    assert len(fake['build']) == 1 and fake['supported'] == 0 and fake['given_supported'] == 5
    # the build is requested with the plain twin of the spec, under the matrix-kernel pin -- and the pin does not outlive the build
    spec, flags = fake['build'][0]
    assert spec == PLAIN_SPEC and spec.given is False
    assert flags & MATRIX and fake['bytes_flags'] & MATRIX and ops.DESC_FLAGS == 0
    # a plain launch of the same spec in between keeps the caller's rows undecided (plain launches are off)
    assert decide(fake, resp, mask) is None


def test_plain_launches_switch_makes_a_given_launch_eligible(fake, monkeypatch):
    monkeypatch.setattr(ops, 'TILE_ROWS_PLAIN_LAUNCHES', True)
    resp, mask = matrix()
    assert [decide(fake, resp, mask) for _ in range(3)] == ['rows', 'rows', 'tiles']
    assert decide(fake, resp, mask, capturing=True) == 'rows'                   # a plain launch under capture keeps the caller's rows
    assert decide(fake, resp, mask, capturing=True, resident_step=True) == 'tiles'


def test_while_capturing(fake):
    resp, mask = matrix()
    assert decide(fake, resp, mask, resident_step=True, capturing=True) == 'rows'      # first sighting
    assert decide(fake, resp, mask, resident_step=True, capturing=True) == 'rows' and not fake['build']      # a capture never builds
    assert decide(fake, resp, mask, capturing=True) is None and not fake['build']      # nor does a plain launch, eligible or not
    assert decide(fake, resp, mask, resident_step=True) == 'rows' and len(fake['build']) == 1
    assert decide(fake, resp, mask, resident_step=True, capturing=True) == 'tiles'     # the resident step under capture
    assert decide(fake, resp, mask, resident_step=True) == 'tiles' and len(fake['build']) == 1


def test_the_switch_turns_all_of_it_off(fake, monkeypatch):
    monkeypatch.setattr(ops, 'TILE_ROWS_GIVEN', False)
    monkeypatch.setattr(ops, 'TILE_ROWS_PLAIN_LAUNCHES', True)
    resp, mask = matrix()
    assert [decide(fake, resp, mask, resident_step=True) for _ in range(4)] == [None] * 4
    assert fake['given_supported'] == fake['capturing'] == 0 and not fake['build'] and not hasattr(resp, '_vibo_row_counts')
    # the plain model's own switch covers the given path too
    monkeypatch.setattr(ops, 'TILE_ROWS_GIVEN', True)
    monkeypatch.setattr(ops, 'TILE_ROWS', False)
    assert [decide(fake, resp, mask, resident_step=True) for _ in range(4)] == [None] * 4
    assert fake['given_supported'] == 0 and not hasattr(resp, '_vibo_row_counts')
    # ... and TILE_ROWS_GIVEN off leaves the plain model's decisions alone
    monkeypatch.setattr(ops, 'TILE_ROWS', True)
    monkeypatch.setattr(ops, 'TILE_ROWS_GIVEN', False)
    step = (torch.zeros(2, dtype=torch.int32), True)
    assert [decide(fake, resp, mask, spec=PLAIN_SPEC, train_step=step) for _ in range(3)] == ['rows', 'rows', 'tiles']


def test_thresholds_and_ineligible_calls(fake, monkeypatch):
    small, small_mask = matrix(P=7)
    assert [decide(fake, small, small_mask, resident_step=True) for _ in range(3)] == [None] * 3
    resp, mask = matrix()
    rows = torch.tensor([5, 1, 7, 2, 3, 4, 6, 8])
    assert decide(fake, resp, mask, row_index=rows, resident_step=True) is None          # gathered rows
    assert decide(fake, resp, mask, B=9, resident_step=True) is None                     # fewer persons than the matrix has rows
    ragged, ragged_mask = matrix(I=6)                                                    # rows the matrix kernel cannot load as they are
    assert decide(fake, ragged, ragged_mask, resident_step=True) is None
    assert fake['given_supported'] == 0 and not hasattr(resp, '_vibo_row_counts')
    # the given path's own minimum on top of the shared one
    monkeypatch.setattr(ops, 'TILE_ROWS_GIVEN_MIN_PERSONS', 13)
    assert [decide(fake, resp, mask, resident_step=True) for _ in range(3)] == [None] * 3 and fake['given_supported'] == 0
    step = (torch.zeros(2, dtype=torch.int32), True)
    assert [decide(fake, resp, mask, spec=PLAIN_SPEC, train_step=step) for _ in range(3)] == ['rows', 'rows', 'tiles']
    # a shape the library refuses
    monkeypatch.setattr(ops, 'TILE_ROWS_GIVEN_MIN_PERSONS', 0)
    monkeypatch.setitem(ops._BACKEND, 'tile_given_supported', lambda d: False)
    other, other_mask = matrix(seed=2)
    assert [decide(fake, other, other_mask, resident_step=True) for _ in range(3)] == [None] * 3 and not hasattr(other, '_vibo_row_counts')


def test_a_builder_that_refuses_the_shape_is_a_remembered_no(fake, monkeypatch):
    monkeypatch.setitem(ops._BACKEND, 'tile_bytes', lambda d: 0)
    resp, mask = matrix()
    assert decide(fake, resp, mask, resident_step=True) == 'rows'
    assert [decide(fake, resp, mask, resident_step=True) for _ in range(3)] == [None] * 3
    assert not fake['build'] and resp._vibo_row_counts.tiles is False


def test_one_image_serves_the_plain_and_the_given_spec(fake):
    step = (torch.zeros(2, dtype=torch.int32), True)
    resp, mask = matrix()
    assert [decide(fake, resp, mask, spec=PLAIN_SPEC, train_step=step) for _ in range(3)] == ['rows', 'rows', 'tiles']
    image = resp._vibo_row_counts.tiles
    assert decide(fake, resp, mask, resident_step=True) == 'tiles' and resp._vibo_row_counts.tiles is image
    assert len(fake['build']) == 1 and fake['build'][0] == (PLAIN_SPEC, 0)
    # and the other way round: built by a given-spec step, used by the plain model's folded step
    resp2, mask2 = matrix(seed=1)
    assert [decide(fake, resp2, mask2, resident_step=True) for _ in range(3)] == ['rows', 'rows', 'tiles']
    assert decide(fake, resp2, mask2, spec=PLAIN_SPEC, train_step=step) == 'tiles' and len(fake['build']) == 2
    # an in-place write starts over for both
    resp2[2, 1] = 1.0
    assert [decide(fake, resp2, mask2, resident_step=True) for _ in range(3)] == ['rows', 'rows', 'tiles'] and len(fake['build']) == 3


def test_the_trainers_mark_their_launch_only_for_the_hip_launcher(monkeypatch):
    from vibo_amd import trainer
    assert trainer._FusedStep._resident_step() == {'resident_step': True}
    monkeypatch.setitem(ops._BACKEND, 'elbo', lambda *a: None)                  # any other backend keeps its signature
    assert trainer._FusedStep._resident_step() == {}
