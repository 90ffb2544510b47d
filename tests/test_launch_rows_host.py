"""ops._launch_rows -- the one decision about the rows of an ELBO launch: format, descriptor, workspace query, entry point, counts --
without a GPU or the library: sequences of launches on host tensors with fake backend entries and a fake capturing(), launch by launch.

Every expectation below is a literal, recorded from the launcher as it composed its three deciders by hand before _launch_rows existed
(the tile image first; the sign rows only where that answered "no image for this call"; the resident counts only for a launch without
train_step that is not on an image).  They are that launcher's behaviour, not a design: scenario A's sixth launch sign-verifies a
matrix that has an image, and scenario D's second launch is looked up by two deciders."""
import pytest
import torch

import tile_rows_common as T
from row_format_common import matrix
from vibo_amd import _lib, ops

PLAIN = ops.ElboSpec(irt_model=2, ability_dim=8)
GIVEN = ops.ElboSpec(irt_model=2, ability_dim=8, given=True)
U8, SIGN, TILES, CODES = _lib.MASK_U8, _lib.MASK_SIGN, _lib.MASK_TILES, _lib.MASK_CODES
FWD, COUNTS, STEP, NOISE = 'vibo_elbo_fwd_bwd', 'vibo_elbo_fwd_bwd_counts', 'vibo_elbo_fwd_bwd_step', 'vibo_elbo_fwd_bwd_step_noise'
GIVEN_TILES = 'vibo_elbo_fwd_bwd_given_tiles'
WS, GIVEN_WS = 'vibo_workspace_bytes', 'vibo_given_tiles_workspace_bytes'
# the record after a launch: (tiles: '?' not decided / 'no' / 'image', sign_is_mask, counts kept), or None: the response carries none
NEW = ('?', None, False)


def folded():
    return (torch.zeros(2, dtype=torch.int32), True)


def drawing():
    return (torch.zeros(2, dtype=torch.int32), True, (1234, 3), True)


def install_fakes(mp, tile_supported=True, sign_supported=True, sign_verify=True, tile_free=1 << 40):
    """Fake backend entries on host tensors -> the list the backend work is logged to ('build', 'verify', 'count'; a build with the spec
    and the descriptor flags it ran under).  sign_supported: a bool, or 'not given' -- no for a POSTERIOR_GIVEN descriptor, as the library."""
    work = []

    def sign_ok(d):
        assert d.mask_dtype == SIGN and d.mask_row_stride == 0
        return d.posterior != _lib.POSTERIOR_GIVEN if sign_supported == 'not given' else sign_supported

    def verify(response, mask):
        work.append('verify')
        return sign_verify

    def tile_ok(d):
        assert d.mask_dtype == TILES
        return tile_supported

    def build(spec, response, mask, mask_code, num_person, reg_mode, want_grad, need):
        work.append(('build', spec, ops.DESC_FLAGS))
        assert need == T.image_bytes(num_person, response.shape[1])
        return torch.zeros(need, dtype=torch.uint8)

    def counts(response, mask, mask_code, row_index):
        work.append('count')
        return torch.zeros(response.shape[0], dtype=torch.int32)
    for key, fn in (('tile_supported', tile_ok), ('tile_given_supported', tile_ok), ('sign_supported', sign_ok), ('sign_verify', verify),
                    ('tile_bytes', lambda d: T.image_bytes(d.num_person, d.num_item)), ('tile_free', lambda device: tile_free),
                    ('tile_build', build), ('counts', counts)):
        mp.setitem(ops._BACKEND, key, fn)
    mp.setattr(ops, 'TILE_ROWS_MIN_PERSONS', 8)          # (every other switch at its default)
    return work


def state(key):
    rec = getattr(key, '_vibo_row_counts', None)
    if rec is None:
        return None
    return ('?' if rec.tiles is None else 'no' if rec.tiles is False else 'image'), rec.sign_is_mask, rec.counts is not None


def launch(work, resp, mask, spec=PLAIN, row_index=None, train_step=None, resident_step=False, capturing=False):
    """One launch through ops._launch_rows -> (format, entry point, workspace query, backend work, the record afterwards); the
    descriptor and the tensors sent are checked here."""
    r, m, code = ops.prepare_rows(resp, mask)
    B, I = (r.shape[0] if row_index is None else int(row_index.numel())), r.shape[1]
    del work[:]
    got = ops._launch_rows(spec, r, m, code, row_index, B, _lib.REG_KL, True, train_step, resident_step=resident_step,
                           capturing=lambda: capturing, stream=None)
    rec = getattr(r, '_vibo_row_counts', None)
    if got.mask_code == TILES:
        assert got.response is rec.tiles and got.mask is None
        assert got.desc.mask_dtype == _lib.MASK_TILES
        assert got.desc.response_row_stride == got.desc.mask_row_stride == (I + 3) & ~3
        assert (got.desc.num_person, got.desc.num_item, got.desc.posterior) == (B, I, _lib.POSTERIOR_GIVEN if spec.given else _lib.POSTERIOR_UNCONDITIONAL)
    else:
        assert got.response is r and got.mask is (None if got.mask_code == SIGN else m)
        assert bytes(got.desc) == bytes(ops._rows_desc(spec, B, got.response, got.mask, got.mask_code, _lib.REG_KL, True))
    assert got.given_tiles is (got.entry == GIVEN_TILES)
    assert got.counts is (rec.counts if got.entry == COUNTS else None) and (got.entry != COUNTS or got.counts is not None)
    return got.mask_code, got.entry, got.workspace_query, tuple(w if isinstance(w, str) else w[0] for w in work), state(r)


@pytest.fixture()
def mp():
    with pytest.MonkeyPatch.context() as m:
        yield m


def test_a_one_matrix_through_every_kind_of_launch(mp):
    work = install_fakes(mp)
    resp, mask = matrix()
    seen = [launch(work, resp, mask, train_step=folded()) for _ in range(4)]
    seen.append(launch(work, resp, mask, train_step=drawing(), capturing=True))
    seen.append(launch(work, resp, mask))
    seen.append(launch(work, resp, mask, capturing=True))
    seen += [launch(work, resp, mask) for _ in range(2)]
    assert seen == [(U8, STEP, WS, (), NEW),
                    (U8, STEP, WS, ('build',), ('image', None, False)),
                    (TILES, STEP, WS, (), ('image', None, False)),
                    (TILES, STEP, WS, (), ('image', None, False)),
                    (TILES, NOISE, WS, (), ('image', None, False)),
                    (U8, FWD, WS, ('verify',), ('image', True, False)),          # (a plain launch is _sign_rows': it verifies)
                    (U8, FWD, WS, (), ('image', True, False)),
                    (SIGN, FWD, WS, (), ('image', True, False)),
                    (SIGN, FWD, WS, (), ('image', True, False))]


def test_b_plain_launches_on_a_fresh_matrix(mp):
    work = install_fakes(mp)
    resp, mask = matrix()
    assert [launch(work, resp, mask) for _ in range(4)] == [(U8, FWD, WS, (), NEW),
                                                            (U8, FWD, WS, ('verify',), ('?', True, False)),
                                                            (SIGN, FWD, WS, (), ('?', True, False)),
                                                            (SIGN, FWD, WS, (), ('?', True, False))]


def test_c_below_the_threshold_the_folded_step_goes_to_sign_rows(mp):
    work = install_fakes(mp)
    resp, mask = matrix(P=7)
    assert [launch(work, resp, mask, train_step=folded()) for _ in range(4)] == [(U8, STEP, WS, (), NEW),
                                                                                 (U8, STEP, WS, ('verify',), ('?', True, False)),
                                                                                 (SIGN, STEP, WS, (), ('?', True, False)),
                                                                                 (SIGN, STEP, WS, (), ('?', True, False))]


def test_d_no_memory_for_the_image_is_a_remembered_no(mp):
    work = install_fakes(mp, tile_free=1)
    resp, mask = matrix()
    assert [launch(work, resp, mask, train_step=folded()) for _ in range(4)] == [(U8, STEP, WS, (), NEW),
                                                                                 (U8, STEP, WS, ('verify',), ('no', True, False)),
                                                                                 (SIGN, STEP, WS, (), ('no', True, False)),
                                                                                 (SIGN, STEP, WS, (), ('no', True, False))]


def test_e_neither_format(mp):
    work = install_fakes(mp, tile_supported=False, sign_verify=False)
    resp, mask = matrix()
    assert [launch(work, resp, mask, train_step=folded()) for _ in range(4)] == [(U8, STEP, WS, (), NEW),
                                                                                 (U8, STEP, WS, ('verify',), ('?', False, False)),
                                                                                 (U8, STEP, WS, (), ('?', False, False)),
                                                                                 (U8, STEP, WS, (), ('?', False, False))]


def test_f_a_caller_supplied_posterior(mp):
    work = install_fakes(mp, sign_supported='not given')
    resp, mask = matrix()
    seen = [launch(work, resp, mask, spec=GIVEN, resident_step=True)]
    seen.append(launch(work, resp, mask, spec=GIVEN, resident_step=True))
    # the build: with the plain twin of the spec under the matrix-kernel pin, which does not outlive it
    assert work == [('build', PLAIN, _lib.FLAG_KERNEL_MATRIX)] and ops.DESC_FLAGS == 0
    seen += [launch(work, resp, mask, spec=GIVEN, resident_step=True) for _ in range(2)]
    seen.append(launch(work, resp, mask, spec=GIVEN))
    seen.append(launch(work, resp, mask, train_step=folded()))
    assert seen == [(U8, FWD, WS, (), NEW),
                    (U8, FWD, WS, ('build',), ('image', None, False)),
                    (TILES, GIVEN_TILES, GIVEN_WS, (), ('image', None, False)),
                    (TILES, GIVEN_TILES, GIVEN_WS, (), ('image', None, False)),
                    (U8, FWD, WS, (), ('image', None, False)),
                    (TILES, STEP, WS, (), ('image', None, False))]


def test_g_gathered_rows_are_never_looked_up(mp):
    work = install_fakes(mp)
    resp, mask = matrix()
    rows = torch.tensor([5, 1, 7, 2, 3, 4, 6, 8])
    assert [launch(work, resp, mask, row_index=rows, train_step=folded()) for _ in range(3)] == [(U8, STEP, WS, (), None)] * 3
    assert not hasattr(resp, '_vibo_row_counts')


def test_h_wide_rows_and_the_resident_counts(mp):
    work = install_fakes(mp, tile_supported=False, sign_supported=False)
    resp, mask = matrix(I=1028)
    rows = torch.tensor([5, 1, 7, 2, 3, 4, 6, 8])
    seen = [launch(work, resp, mask) for _ in range(3)]
    seen.append(launch(work, resp, mask, row_index=rows))
    seen.append(launch(work, resp, mask, capturing=True))
    seen.append(launch(work, resp, mask, row_index=rows, capturing=True))
    seen.append(launch(work, resp, mask))
    resp[0, 0] = 1.0
    seen += [launch(work, resp, mask) for _ in range(3)]
    assert seen == [(U8, FWD, WS, (), NEW),
                    (U8, COUNTS, WS, ('count',), ('?', None, True)),
                    (U8, COUNTS, WS, (), ('?', None, True)),
                    (U8, COUNTS, WS, (), ('?', None, True)),
                    (U8, FWD, WS, (), ('?', None, True)),                        # (the captured input IS the matrix)
                    (U8, COUNTS, WS, (), ('?', None, True)),
                    (U8, COUNTS, WS, (), ('?', None, True)),
                    (U8, FWD, WS, (), NEW),                                      # (the in-place write starts over)
                    (U8, COUNTS, WS, ('count',), ('?', None, True)),
                    (U8, COUNTS, WS, (), ('?', None, True))]


def test_i_cell_codes(mp):
    work = install_fakes(mp)
    resp, mask = matrix()
    codes = ops.CellCodes(torch.where(mask, resp.to(torch.uint8), torch.tensor(2, dtype=torch.uint8)))
    assert [launch(work, codes, None, train_step=folded()) for _ in range(3)] == [(CODES, STEP, WS, (), NEW),
                                                                                  (CODES, STEP, WS, ('build',), ('image', None, False)),
                                                                                  (TILES, STEP, WS, (), ('image', None, False))]
    assert codes.codes._vibo_row_counts.has_mask is False                       # (known by the codes alone)
